"""ctypes binding of include/emsar_hip.h (the C ABI that replaces run_MLE_threads(),
/root/reference/src/emsar_main.c:446).  Thin: argument marshalling and error mapping only."""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# EMSAR_HIP_LIB: experiment hook -- another build of the same library (timing-only ablations, compile-time variants)
_LIB_PATH = os.environ.get("EMSAR_HIP_LIB") or os.path.join(_PKG, "libemsar_hip.so")
_lib = None

LAYOUT_AUTO, LAYOUT_CSR, LAYOUT_TILED = 0, 1, 3
FLAG_MERGE_ROWS = 0x100

# every symbol include/emsar_hip.h declares (tests check that the library exports exactly these)
SYMBOLS = [
    "emsar_hip_create", "emsar_hip_destroy", "emsar_hip_strerror", "emsar_hip_last_error",
    "emsar_hip_upload_structure", "emsar_hip_upload_sample", "emsar_hip_solve",
    "emsar_hip_reset_theta", "emsar_hip_set_theta", "emsar_hip_get_theta", "emsar_hip_run_passes",
    "emsar_hip_ieuma", "emsar_hip_normalise", "emsar_hip_get_info",
    "emsar_hip_layout_selfcheck_tiled", "emsar_hip_sets_selfcheck", "emsar_hip_upload_euma", "emsar_hip_adj_euma", "emsar_hip_collapse_rows",
    "emsar_hip_set_deterministic", "emsar_hip_bootstrap", "emsar_hip_bootstrap_weights", "emsar_hip_bootstrap_draw_host",
    "emsar_hip_set_gene_map", "emsar_hip_gene_sums", "emsar_hip_bootstrap_genes",
    "emsar_hip_subsample", "emsar_hip_subsample_weights", "emsar_hip_subsample_draw_host",
    "emsar_hip_bootstrap_quantiles", "emsar_hip_quantiles_host",
    "emsar_hip_isoform_usage", "emsar_hip_isoform_usage_host", "emsar_hip_bootstrap_isoforms",
    "emsar_hip_model_fit", "emsar_hip_model_fit_host",
    "emsar_hip_presence", "emsar_hip_presence_pvalue_host",
    "emsar_hip_profile", "emsar_hip_profile_cut_host",
    "emsar_hip_compare", "emsar_hip_compare_pvalue_host", "emsar_hip_compare_genes",
    "emsar_hip_profile_genes", "emsar_hip_gene_presence_pvalue_host",
    "emsar_hip_compare_usage", "emsar_hip_profile_usage",
    "emsar_hip_compare_groups", "emsar_hip_compare_groups_pvalue_host", "emsar_hip_compare_groups_genes",
    "emsar_hip_asymptotic", "emsar_hip_asymptotic_host",
]

# status of a transcript in the presence test (include/emsar_hip.h "presence test"), by value
PRESENCE_STATUS = ("TESTED", "ABSENT", "ESSENTIAL", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED")

# status of a transcript's profile-likelihood interval (include/emsar_hip.h "profile-likelihood intervals"), by value
PROFILE_STATUS = ("TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED")

# status of a transcript in the two-sample test (include/emsar_hip.h "two-sample test"), by value
COMPARE_STATUS = ("TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED")
COMPARE_OUTPUTS = ("lambda", "pvalue", "log2fc", "theta_a", "theta_b", "theta_null", "multiplier", "gap", "raw_lambda")

# status of a gene in the gene-level two-sample test (include/emsar_hip.h "gene-level two-sample test"), by value
COMPARE_GENE_STATUS = COMPARE_STATUS + ("TOO_LARGE",)
COMPARE_GENE_OUTPUTS = ("lambda", "pvalue", "log2fc", "gene_a", "gene_b", "gene_null", "multiplier", "gap", "raw_lambda")

# status of a transcript in the two-sample test of isoform usage (include/emsar_hip.h "two-sample test of isoform usage"), by value
USAGE_STATUS = ("TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE", "UNDEFINED", "SINGLE")
USAGE_OUTPUTS = ("lambda", "raw_lambda", "pvalue", "usage_a", "usage_b", "usage_null", "dlogit", "slope")
USAGE_COUNTS = ("status", "outer_evals", "evals", "parts")

# status of a transcript in the K-sample test across replicate groups (include/emsar_hip.h "K-sample test"), by value
GROUPS_STATUS = ("TESTED", "ALL_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED")
GROUPS_OUTPUTS = ("lambda_between", "p_between", "lambda_within", "p_within", "raw_between", "raw_within", "theta_common", "slope")
GROUPS_COUNTS = ("status", "outer", "evals")
GROUPS_MAX = 32
# status of a gene in the gene-level K-sample test (include/emsar_hip.h "gene-level K-sample test"), by value
GROUPS_GENE_STATUS = GROUPS_STATUS + ("TOO_LARGE",)
GROUPS_GENE_OUTPUTS = ("lambda_between", "p_between", "lambda_within", "p_within", "raw_between", "raw_within", "gene_common", "slope")
GROUPS_GENE_COUNTS = ("status", "outer", "evals", "parts")

# status of a gene's profile-likelihood interval (include/emsar_hip.h "gene-level profile intervals"), by value
PROFILE_GENE_STATUS = PROFILE_STATUS + ("TOO_LARGE",)
PROFILE_GENE_OUTPUTS = ("lower", "upper", "dev_lower", "dev_upper", "lambda", "pvalue", "gene_hat")

# status of a transcript's profile-likelihood interval of isoform usage (include/emsar_hip.h "profile-likelihood intervals of isoform
# usage"), by value
PROFILE_USAGE_STATUS = PROFILE_GENE_STATUS + ("UPPER_ONE", "UNIT", "UNDEFINED", "SINGLE")
PROFILE_USAGE_OUTPUTS = ("usage", "lower", "upper", "dev_lower", "dev_upper", "lambda_zero", "lambda_one")
PROFILE_USAGE_COUNTS = ("status", "outer_evals", "evals", "parts", "members")

# status of a transcript in the asymptotic standard errors (include/emsar_hip.h "asymptotic standard errors"), by value
ASYM_STATUS = ("ESTIMATED", "BOUNDARY", "UNIDENTIFIABLE", "TOO_LARGE", "INFEASIBLE")
ASYM_MAX_N = 192
ASYM_DEFAULT_CUT = 5e-7


class EmsarHipError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__("%s: %s (status %d)%s" % (what, _strerror(status), status, (" -- " + detail) if detail else ""))


class EmParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("accel", C.c_int32), ("tol", C.c_double), ("abs_floor", C.c_double),
                ("check_every", C.c_int32), ("set_mode", C.c_int32), ("count_floor", C.c_double), ("zero_cut", C.c_double), ("abs_step", C.c_double),
                ("newton_after", C.c_int32), ("reserved0", C.c_int32)]


class EmStats(C.Structure):
    _fields_ = [("iters", C.c_int32), ("converged", C.c_int32), ("final_delta", C.c_double), ("loglik", C.c_double),
                ("solve_ms", C.c_double), ("kernel_ms", C.c_double), ("bytes_per_pass", C.c_int64),
                ("stored_bytes_per_pass", C.c_int64),
                ("sets_resident", C.c_int32), ("sets_streamed", C.c_int32), ("set_passes_max", C.c_int32),
                ("sets_unconverged", C.c_int32), ("set_passes_sum", C.c_int64), ("sets_build_ms", C.c_double),
                ("sets_kernel_ms", C.c_double), ("sets_cluster", C.c_int32), ("cluster_passes_max", C.c_int32), ("cluster_kernel_ms", C.c_double)]


class CollapseStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("n_rows", C.c_int64), ("nnz", C.c_int64),
                ("n_unique", C.c_int64), ("nnz_unique", C.c_int64), ("table_slots", C.c_int64), ("algorithmic_bytes", C.c_int64), ("rounds", C.c_int64)]


class BootStats(C.Structure):
    _fields_ = [("n_replicates", C.c_int32), ("batch", C.c_int32), ("replicates_unconverged", C.c_int32), ("set_passes_max", C.c_int32),
                ("draws", C.c_int64), ("draw_ms", C.c_double), ("sets_ms", C.c_double), ("stream_ms", C.c_double), ("reduce_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SubsampleStats(C.Structure):
    _fields_ = [("n_fractions", C.c_int32), ("n_replicates", C.c_int32), ("batch", C.c_int32), ("replicates_unconverged", C.c_int32),
                ("draws", C.c_int64), ("draw_ms", C.c_double), ("sets_ms", C.c_double), ("stream_ms", C.c_double), ("reduce_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class QuantileStats(C.Structure):
    _fields_ = [("n_quantiles", C.c_int32), ("reserved0", C.c_int32), ("held_bytes", C.c_int64), ("quantile_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IsoformOutputs(C.Structure):
    _fields_ = [("usage_mean", C.POINTER(C.c_double)), ("usage_sd", C.POINTER(C.c_double)), ("dominant_count", C.POINTER(C.c_int32)),
                ("usage_q", C.POINTER(C.c_double))]


class FitOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("row_mu", "row_chi2", "row_dev", "tx_chi2", "tx_dev", "tx_miss", "tx_df")] + [
        ("tx_worst_row", C.POINTER(C.c_int32))] + [(k, C.POINTER(C.c_double)) for k in ("gene_chi2", "gene_dev", "gene_miss", "gene_df")]


class FitStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("rows_inside", C.c_int64), ("rows_infeasible", C.c_int64),
                ("index_slots", C.c_int64), ("index_bytes", C.c_int64), ("sum_chi2", C.c_double), ("sum_dev", C.c_double),
                ("sum_miss", C.c_double), ("rows_ms", C.c_double), ("tx_ms", C.c_double), ("genes_ms", C.c_double), ("totals_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PresenceOutputs(C.Structure):
    _fields_ = [("lambda_", C.POINTER(C.c_double)), ("pvalue", C.POINTER(C.c_double)), ("heir", C.POINTER(C.c_int32)),
                ("heir_share", C.POINTER(C.c_double)), ("status", C.POINTER(C.c_int32)), ("theta_hat", C.POINTER(C.c_double))]


class PresenceStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 6), ("items_launched", C.c_int64), ("drop_passes_sum", C.c_int64), ("drop_passes_max", C.c_int32),
                ("reserved0", C.c_int32), ("min_raw_lambda", C.c_double), ("baseline_ms", C.c_double), ("drop_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(PRESENCE_STATUS, d["n_status"]))
        return d


class ProfileParams(C.Structure):
    _fields_ = [("level", C.c_double), ("dev_tol", C.c_double), ("max_evals", C.c_int32), ("max_outer", C.c_int32)]


class ProfileOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda_", "theta_hat")] + [
        ("status", C.POINTER(C.c_int32)), ("evals", C.POINTER(C.c_int32))]


class ProfileStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 5), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("cut", C.c_double), ("baseline_ms", C.c_double), ("drop_ms", C.c_double),
                ("search_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(PROFILE_STATUS, d["n_status"]))
        return d


class CompareParams(C.Structure):
    _fields_ = [("ratio", C.c_double), ("dev_tol", C.c_double), ("max_evals", C.c_int32), ("reserved0", C.c_int32)]


class CompareOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("lambda_", "pvalue", "log2fc", "theta_a", "theta_b", "theta_null", "multiplier", "gap",
                                                     "raw_lambda")] + [("status", C.POINTER(C.c_int32)), ("evals", C.POINTER(C.c_int32))]


class CompareStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 5), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("min_raw_lambda", C.c_double), ("device_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(COMPARE_STATUS, d["n_status"]))
        return d


class CompareGeneOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("lambda_", "pvalue", "log2fc", "gene_a", "gene_b", "gene_null", "multiplier", "gap",
                                                     "raw_lambda")] + [(k, C.POINTER(C.c_int32)) for k in ("status", "evals", "parts")]


class CompareGeneStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 6), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("parts_max", C.c_int32), ("reserved0", C.c_int32),
                ("min_raw_lambda", C.c_double), ("device_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(COMPARE_GENE_STATUS, d["n_status"]))
        return d


class UsageParams(C.Structure):
    _fields_ = [("dev_tol", C.c_double), ("max_evals", C.c_int32), ("max_outer", C.c_int32)]


class UsageOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("lambda_", "raw_lambda", "pvalue", "usage_a", "usage_b", "usage_null", "dlogit", "slope")] + \
               [(k, C.POINTER(C.c_int32)) for k in USAGE_COUNTS]


class UsageStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 8), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("outer_sum", C.c_int64), ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("parts_max", C.c_int32),
                ("outer_max", C.c_int32), ("min_raw_lambda", C.c_double), ("device_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(USAGE_STATUS, d["n_status"]))
        return d


class GroupsParams(C.Structure):
    _fields_ = [("dev_tol", C.c_double), ("max_evals", C.c_int32), ("max_outer", C.c_int32)]


class GroupsOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in GROUPS_OUTPUTS + ("theta_group", "theta_hat")] + \
               [(k, C.POINTER(C.c_int32)) for k in GROUPS_COUNTS]


class GroupsStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 5), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("outer_sum", C.c_int64), ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("outer_max", C.c_int32),
                ("reserved0", C.c_int32), ("df_between", C.c_int32), ("df_within", C.c_int32), ("min_raw_lambda", C.c_double),
                ("device_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(GROUPS_STATUS, d["n_status"]))
        return d


class GroupsGeneOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in GROUPS_GENE_OUTPUTS + ("gene_group", "gene_hat")] + \
               [(k, C.POINTER(C.c_int32)) for k in GROUPS_GENE_COUNTS]


class GroupsGeneStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 6), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("outer_sum", C.c_int64), ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("outer_max", C.c_int32),
                ("parts_max", C.c_int32), ("df_between", C.c_int32), ("df_within", C.c_int32), ("min_raw_lambda", C.c_double),
                ("device_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(GROUPS_GENE_STATUS, d["n_status"]))
        return d


class ProfileGeneOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda_", "pvalue", "gene_hat")] + \
               [(k, C.POINTER(C.c_int32)) for k in ("status", "evals", "parts", "members")]


class ProfileGeneStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 6), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("parts_max", C.c_int32), ("reserved0", C.c_int32),
                ("min_raw_lambda", C.c_double), ("cut", C.c_double), ("baseline_ms", C.c_double), ("search_ms", C.c_double),
                ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(PROFILE_GENE_STATUS, d["n_status"]))
        return d


class ProfileUsageOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in PROFILE_USAGE_OUTPUTS] + [(k, C.POINTER(C.c_int32)) for k in PROFILE_USAGE_COUNTS]


class ProfileUsageStats(C.Structure):
    _fields_ = [("n_status", C.c_int64 * 10), ("items_launched", C.c_int64), ("evals_sum", C.c_int64), ("passes_sum", C.c_int64),
                ("outer_sum", C.c_int64), ("evals_max", C.c_int32), ("passes_max", C.c_int32), ("parts_max", C.c_int32),
                ("outer_max", C.c_int32), ("min_raw_lambda", C.c_double), ("cut", C.c_double), ("baseline_ms", C.c_double),
                ("search_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(PROFILE_USAGE_STATUS, d["n_status"]))
        return d


class AsymParams(C.Structure):
    _fields_ = [("boundary_cut", C.c_double), ("pivot_tol", C.c_double), ("block_tid", C.c_int32), ("reserved0", C.c_int32)]


class AsymOutputs(C.Structure):
    _fields_ = [(k, C.POINTER(C.c_double)) for k in ("var", "sd_fpkm", "sd_tpm", "rowsum", "usage_sd")] + [
        ("status", C.POINTER(C.c_int32)), ("partner", C.POINTER(C.c_int32)), ("partner_cov", C.POINTER(C.c_double)),
        ("blocker", C.POINTER(C.c_int32)), ("gene_sd", C.POINTER(C.c_double)), ("gene_status", C.POINTER(C.c_int32)),
        ("block_n", C.POINTER(C.c_int32)), ("block_tids", C.POINTER(C.c_int32)), ("block_cov", C.POINTER(C.c_double))]


class AsymStats(C.Structure):
    _fields_ = [("components", C.c_int64), ("components_too_large", C.c_int64), ("components_infeasible", C.c_int64),
                ("components_class", C.c_int64 * 4), ("components_unidentifiable", C.c_int64), ("n_status", C.c_int64 * 5),
                ("rows_infeasible", C.c_int64), ("max_n", C.c_int32), ("reserved0", C.c_int32), ("min_pivot_ratio", C.c_double),
                ("theta_unestimated_share", C.c_double), ("plan_ms", C.c_double), ("rows_ms", C.c_double), ("sets_ms", C.c_double),
                ("genes_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["n_status"] = dict(zip(ASYM_STATUS, d["n_status"]))
        d["components_class"] = list(d["components_class"])
        return d


class SetsInfo(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("sets_resident", C.c_int64 * 3), ("max_lds_bytes", C.c_int64 * 3),
                ("sets_streamed", C.c_int64), ("tids_closed", C.c_int64), ("tids_resident", C.c_int64),
                ("tids_streamed", C.c_int64), ("rows_in", C.c_int64), ("rows_stored", C.c_int64),
                ("sets_cluster", C.c_int64), ("tids_cluster", C.c_int64), ("max_lds_cluster", C.c_int64)]


class Info(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("nnz", C.c_int64), ("n_tx", C.c_int32), ("layout", C.c_int32),
                ("n_chunks", C.c_int64), ("n_slices", C.c_int64), ("padded_entries", C.c_int64),
                ("far_entries", C.c_int64), ("window", C.c_int32), ("device_id", C.c_int32),
                ("bytes_per_pass", C.c_int64), ("stored_bytes_per_pass", C.c_int64),
                ("tiled_entries", C.c_int64), ("tiled_ids", C.c_int64), ("n_units", C.c_int64), ("renumbered", C.c_int32), ("reserved0", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def load_library():
    """dlopen the in-tree HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise EmsarHipError(-4, "load_library", "%s missing: run python -m emsar_amd._build" % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    vp, u64p, i32p, f64p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    L.emsar_hip_create.argtypes = [C.POINTER(vp), C.c_int]
    L.emsar_hip_destroy.argtypes = [vp]
    L.emsar_hip_destroy.restype = None
    L.emsar_hip_strerror.argtypes = [C.c_int]
    L.emsar_hip_strerror.restype = C.c_char_p
    L.emsar_hip_last_error.argtypes = [vp]
    L.emsar_hip_last_error.restype = C.c_char_p
    L.emsar_hip_upload_structure.argtypes = [vp, C.c_int64, C.c_int32, u64p, i32p, C.c_int]
    L.emsar_hip_upload_sample.argtypes = [vp, i32p, f64p, f64p]
    L.emsar_hip_solve.argtypes = [vp, C.POINTER(EmParams), f64p, C.POINTER(EmStats)]
    L.emsar_hip_reset_theta.argtypes = [vp]
    L.emsar_hip_set_theta.argtypes = [vp, f64p]
    L.emsar_hip_get_theta.argtypes = [vp, f64p]
    L.emsar_hip_run_passes.argtypes = [vp, C.c_int32, C.POINTER(C.c_float), f64p]
    L.emsar_hip_ieuma.argtypes = [vp, f64p, f64p]
    L.emsar_hip_normalise.argtypes = [vp, f64p, f64p, C.c_int64, f64p, f64p, i32p]
    L.emsar_hip_get_info.argtypes = [vp, C.POINTER(Info)]
    L.emsar_hip_layout_selfcheck_tiled.argtypes = [C.c_int64, C.c_int32, u64p, i32p, C.c_int, C.POINTER(Info)]
    L.emsar_hip_set_deterministic.argtypes = [vp, C.c_int]
    L.emsar_hip_set_deterministic.restype = C.c_int
    L.emsar_hip_collapse_rows.argtypes = [vp, C.c_int64, C.c_int32, u64p, i32p, i32p, C.POINTER(C.c_int64), u64p, i32p, i32p, i32p,
                                          C.POINTER(CollapseStats)]
    L.emsar_hip_upload_euma.argtypes = [vp, i32p, C.c_int32]
    L.emsar_hip_adj_euma.argtypes = [vp, f64p, f64p]
    L.emsar_hip_sets_selfcheck.argtypes = [C.c_int64, C.c_int32, u64p, i32p, i32p, C.POINTER(SetsInfo)]
    L.emsar_hip_bootstrap.argtypes = [vp, C.POINTER(EmParams), C.c_uint64, C.c_int32, C.c_int32, f64p, f64p, f64p, f64p, C.POINTER(BootStats)]
    L.emsar_hip_bootstrap_weights.argtypes = [vp, C.c_uint64, C.c_int32, i32p]
    L.emsar_hip_bootstrap_draw_host.argtypes = [C.c_uint64, C.c_int32, C.c_int64, i32p, i32p]
    L.emsar_hip_set_gene_map.argtypes = [vp, C.c_int32, i32p]
    L.emsar_hip_gene_sums.argtypes = [vp, C.c_int32, f64p, f64p]
    L.emsar_hip_bootstrap_genes.argtypes = [vp, C.POINTER(EmParams), C.c_uint64, C.c_int32, C.c_int32, f64p, f64p, f64p, f64p,
                                            f64p, f64p, f64p, C.POINTER(BootStats)]
    L.emsar_hip_subsample.argtypes = [vp, C.POINTER(EmParams), C.c_uint64, C.c_int32, f64p, C.c_int32, f64p, f64p, f64p, f64p, f64p, f64p,
                                      f64p, f64p, f64p, C.POINTER(SubsampleStats)]
    L.emsar_hip_subsample_weights.argtypes = [vp, C.c_uint64, C.c_int32, C.c_double, i32p]
    L.emsar_hip_subsample_draw_host.argtypes = [C.c_uint64, C.c_int32, C.c_double, C.c_int64, i32p, i32p]
    L.emsar_hip_bootstrap_quantiles.argtypes = [vp, C.POINTER(EmParams), C.c_uint64, C.c_int32, C.c_int32, C.c_int32, f64p] + [f64p] * 12 + [
        C.POINTER(BootStats), C.POINTER(QuantileStats)]
    L.emsar_hip_quantiles_host.argtypes = [C.c_int32, C.c_int64, f64p, C.c_int32, f64p, f64p]
    L.emsar_hip_isoform_usage.argtypes = [vp, C.c_int32, f64p, f64p, i32p]
    L.emsar_hip_isoform_usage_host.argtypes = [C.c_int32, C.c_int32, i32p, C.c_int32, f64p, f64p, i32p]
    L.emsar_hip_bootstrap_isoforms.argtypes = L.emsar_hip_bootstrap_quantiles.argtypes + [C.POINTER(IsoformOutputs)]
    L.emsar_hip_model_fit.argtypes = [vp, f64p, f64p, C.POINTER(FitOutputs), C.POINTER(FitStats)]
    L.emsar_hip_model_fit_host.argtypes = [C.c_int64, C.c_int32, u64p, i32p, i32p, f64p, f64p, C.c_int32, i32p, C.POINTER(FitOutputs),
                                           C.POINTER(FitStats)]
    L.emsar_hip_presence.argtypes = [vp, C.POINTER(EmParams), C.c_int32, i32p, C.POINTER(PresenceOutputs), C.POINTER(PresenceStats)]
    L.emsar_hip_presence_pvalue_host.argtypes = [C.c_int64, f64p, f64p]
    L.emsar_hip_profile.argtypes = [vp, C.POINTER(EmParams), C.POINTER(ProfileParams), C.c_int32, i32p, C.POINTER(ProfileOutputs),
                                    C.POINTER(ProfileStats)]
    L.emsar_hip_profile_cut_host.argtypes = [C.c_double, f64p]
    L.emsar_hip_compare.argtypes = [vp, vp, C.POINTER(EmParams), C.POINTER(CompareParams), C.c_int32, i32p, C.POINTER(CompareOutputs),
                                    C.POINTER(CompareStats)]
    L.emsar_hip_compare_pvalue_host.argtypes = [C.c_int64, f64p, f64p]
    L.emsar_hip_compare_genes.argtypes = [vp, vp, C.POINTER(EmParams), C.POINTER(CompareParams), C.c_int32, i32p, C.POINTER(CompareGeneOutputs),
                                          C.POINTER(CompareGeneStats)]
    L.emsar_hip_compare_usage.argtypes = [vp, vp, C.POINTER(EmParams), C.POINTER(UsageParams), C.c_int32, i32p, C.POINTER(UsageOutputs),
                                          C.POINTER(UsageStats)]
    L.emsar_hip_compare_groups.argtypes = [C.POINTER(vp), C.c_int32, i32p, f64p, C.POINTER(EmParams), C.POINTER(GroupsParams), C.c_int32, i32p,
                                           C.POINTER(GroupsOutputs), C.POINTER(GroupsStats)]
    L.emsar_hip_compare_groups_pvalue_host.argtypes = [C.c_int64, f64p, i32p, f64p]
    L.emsar_hip_compare_groups_genes.argtypes = [C.POINTER(vp), C.c_int32, i32p, f64p, C.POINTER(EmParams), C.POINTER(GroupsParams), C.c_int32,
                                                 i32p, C.POINTER(GroupsGeneOutputs), C.POINTER(GroupsGeneStats)]
    L.emsar_hip_profile_usage.argtypes = [vp, C.POINTER(EmParams), C.POINTER(ProfileParams), C.c_int32, i32p, C.POINTER(ProfileUsageOutputs),
                                          C.POINTER(ProfileUsageStats)]
    L.emsar_hip_profile_genes.argtypes = [vp, C.POINTER(EmParams), C.POINTER(ProfileParams), C.c_int32, i32p, C.POINTER(ProfileGeneOutputs),
                                          C.POINTER(ProfileGeneStats)]
    L.emsar_hip_gene_presence_pvalue_host.argtypes = [C.c_int64, f64p, i32p, f64p]
    L.emsar_hip_asymptotic.argtypes = [vp, f64p, C.POINTER(AsymParams), C.POINTER(AsymOutputs), C.POINTER(AsymStats)]
    L.emsar_hip_asymptotic_host.argtypes = [C.c_int64, C.c_int32, u64p, i32p, i32p, f64p, f64p, C.c_int32, i32p, C.POINTER(AsymParams),
                                            C.POINTER(AsymOutputs), C.POINTER(AsymStats)]
    _lib = L
    return L


def _strerror(status):
    try:
        return load_library().emsar_hip_strerror(status).decode()
    except Exception:
        return "?"


def _p(a, ct):
    return None if a is None else a.ctypes.data_as(C.POINTER(ct))


def _arr(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def sets_selfcheck(n_tx, row_ptr, col_idx, row_weight=None):
    """Host-only: find + pack the connected sets for the set-resident solver and check the records (no GPU needed)."""
    L = load_library()
    row_ptr, col_idx = _arr(row_ptr, np.uint64), _arr(col_idx, np.int32)
    w = None if row_weight is None else _arr(row_weight, np.int32)
    info = SetsInfo()
    rc = L.emsar_hip_sets_selfcheck(len(row_ptr) - 1, n_tx, _p(row_ptr, C.c_uint64), _p(col_idx, C.c_int32),
                                    None if w is None else _p(w, C.c_int32), C.byref(info))
    if rc != 0:
        raise EmsarHipError(rc, "sets_selfcheck")
    d = {k: getattr(info, k) for k, _ in SetsInfo._fields_}
    d["sets_resident"] = list(d["sets_resident"])
    d["max_lds_bytes"] = list(d["max_lds_bytes"])
    return d


def bootstrap_draw_host(seed, replicate, row_weight=None, n_rows=None):
    """Host-only: the Poisson draws of bootstrap replicate `replicate` of `seed` (no GPU needed), the same function the device
    evaluates.  row_weight None = 1 per row (then n_rows is required)."""
    L = load_library()
    w = None if row_weight is None else _arr(row_weight, np.int32)
    n = len(w) if w is not None else int(n_rows)
    out = np.zeros(max(n, 1), dtype=np.int32)
    rc = L.emsar_hip_bootstrap_draw_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(replicate), n, _p(w, C.c_int32), _p(out, C.c_int32))
    if rc != 0:
        raise EmsarHipError(rc, "bootstrap_draw_host")
    return out[:n]


def subsample_draw_host(seed, replicate, fraction, row_weight=None, n_rows=None):
    """Host-only: the binomial draws w ~ Binomial(row_weight, fraction) of subsampling replicate `replicate` of `seed` (no GPU
    needed), the same function the device evaluates.  row_weight None = 1 per row (then n_rows is required)."""
    L = load_library()
    w = None if row_weight is None else _arr(row_weight, np.int32)
    n = len(w) if w is not None else int(n_rows)
    out = np.zeros(max(n, 1), dtype=np.int32)
    rc = L.emsar_hip_subsample_draw_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(replicate), float(fraction), n, _p(w, C.c_int32), _p(out, C.c_int32))
    if rc != 0:
        raise EmsarHipError(rc, "subsample_draw_host")
    return out[:n]


def quantiles_host(values, q):
    """Host-only: the library's quantile definition (include/emsar_hip.h "bootstrap quantiles") over axis 0 of values [n_rep][n] (or
    [n_rep]) for the probabilities q -> [n_q][n] (or [n_q]); no GPU needed, the same function the device evaluates."""
    L = load_library()
    v = _arr(values, np.float64)
    one = v.ndim == 1
    v = np.ascontiguousarray(v.reshape(v.shape[0], -1))
    qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    out = np.zeros((max(len(qa), 1), v.shape[1]))
    rc = L.emsar_hip_quantiles_host(v.shape[0], v.shape[1], _p(v, C.c_double), len(qa), _p(qa, C.c_double), _p(out, C.c_double))
    if rc != 0:
        raise EmsarHipError(rc, "quantiles_host")
    return out[:, 0] if one else out


def isoform_usage_host(gene_of_tx, n_genes, cols, want_dominant=False):
    """Host-only: the library's isoform usage (include/emsar_hip.h "isoform usage") of cols [n_cols][n_tx] (or [n_tx]) under the gene map
    gene_of_tx (-1 = no gene) -> usage of the same shape; with want_dominant (usage, dominant [n_cols][n_genes] or [n_genes]: the
    tid of every gene's dominant isoform, -1 for a gene whose sum is 0).  No GPU needed, the same function the device evaluates."""
    L = load_library()
    g = _arr(gene_of_tx, np.int32)
    x = _arr(cols, np.float64)
    one = x.ndim == 1
    x = np.ascontiguousarray(np.atleast_2d(x))
    if x.shape[1] != len(g):
        raise ValueError("columns of n_tx values expected")
    usage = np.zeros(x.shape)
    dom = np.zeros((x.shape[0], max(int(n_genes), 1)), dtype=np.int32) if want_dominant else None
    rc = L.emsar_hip_isoform_usage_host(len(g), int(n_genes), _p(g, C.c_int32), x.shape[0], _p(x, C.c_double), _p(usage, C.c_double),
                                        _p(dom, C.c_int32))
    if rc != 0:
        raise EmsarHipError(rc, "isoform_usage_host")
    if not want_dominant:
        return usage[0] if one else usage
    dom = dom[:, :max(int(n_genes), 0)]
    return (usage[0], dom[0]) if one else (usage, dom)


def _fit_buffers(n_rows, n_tx, n_genes, rows, genes):
    """the output arrays of a model fit (never of length 0) and the struct that points at them"""
    res = {k: np.zeros(max(n_tx, 1)) for k in ("tx_chi2", "tx_dev", "tx_miss", "tx_df")}
    res["tx_worst_row"] = np.zeros(max(n_tx, 1), dtype=np.int32)
    if rows:
        res.update({k: np.zeros(max(n_rows, 1)) for k in ("row_mu", "row_chi2", "row_dev")})
    if genes:
        res.update({k: np.zeros(max(n_genes, 1)) for k in ("gene_chi2", "gene_dev", "gene_miss", "gene_df")})
    o = FitOutputs()
    for k, a in res.items():
        setattr(o, k, _p(a, C.c_int32 if k == "tx_worst_row" else C.c_double))
    return res, o


def _fit_result(res, n_rows, n_tx, n_genes, st):
    out = {k: v[:(n_rows if k.startswith("row_") else n_genes if k.startswith("gene_") else n_tx)] for k, v in res.items()}
    out["stats"] = st
    return out


def model_fit_host(n_tx, row_ptr, col_idx, theta, row_weight=None, E=None, rows=False, gene_of_tx=None, n_genes=0, genes=None):
    """Host-only: the library's model fit (include/emsar_hip.h "model fit") of theta against the rows' weights (None = 1 per row) and
    E (None = 1.0), no GPU needed, the same functions the device evaluates.  Returns a dict: tx_chi2, tx_dev, tx_miss, tx_df, tx_worst_row
    ([n_tx]), with rows also row_mu, row_chi2, row_dev ([n_rows]), with a gene map (gene_of_tx, n_genes; genes=False leaves them out)
    also gene_chi2, gene_dev, gene_miss, gene_df ([n_genes]), and stats."""
    L = load_library()
    row_ptr, col_idx, th = _arr(row_ptr, np.uint64), _arr(col_idx, np.int32), _arr(theta, np.float64)
    w, e, g = _arr(row_weight, np.int32), _arr(E, np.float64), _arr(gene_of_tx, np.int32)
    n_rows = len(row_ptr) - 1
    for a, n in ((th, n_tx), (w, n_rows), (e, n_rows), (g, n_tx)):
        if a is not None and a.shape != (n,):
            raise ValueError("array of length %d expected" % n)
    want_genes = (g is not None) if genes is None else bool(genes)
    res, o = _fit_buffers(n_rows, n_tx, int(n_genes), rows, want_genes)
    st = FitStats()
    rc = L.emsar_hip_model_fit_host(n_rows, int(n_tx), _p(row_ptr, C.c_uint64), _p(col_idx, C.c_int32), _p(w, C.c_int32), _p(e, C.c_double),
                                    _p(th, C.c_double), int(n_genes), _p(g, C.c_int32), C.byref(o), C.byref(st))
    if rc != 0:
        raise EmsarHipError(rc, "model_fit_host")
    return _fit_result(res, n_rows, int(n_tx), int(n_genes), st)


def _asym_buffers(n_tx, n_genes, genes, block):
    """the output arrays of the asymptotic standard errors (never of length 0) and the struct that points at them"""
    T = max(n_tx, 1)
    res = {k: np.zeros(T) for k in ("var", "sd_fpkm", "sd_tpm", "rowsum", "partner_cov")}
    res.update({k: np.zeros(T, dtype=np.int32) for k in ("status", "partner", "blocker")})
    if genes:
        res.update(usage_sd=np.zeros(T), gene_sd=np.zeros(max(n_genes, 1)), gene_status=np.zeros(max(n_genes, 1), dtype=np.int32))
    if block:
        res.update(block_n=np.zeros(1, dtype=np.int32), block_tids=np.zeros(ASYM_MAX_N, dtype=np.int32), block_cov=np.zeros(ASYM_MAX_N * ASYM_MAX_N))
    o = AsymOutputs()
    for k, a in res.items():
        setattr(o, k, _p(a, C.c_int32 if a.dtype == np.int32 else C.c_double))
    return res, o


def _asym_result(res, n_tx, n_genes, st):
    out = {k: v[:(n_genes if k.startswith("gene_") else n_tx)] for k, v in res.items() if not k.startswith("block_")}
    if "block_n" in res:
        n = int(res["block_n"][0])
        out["block_tids"] = res["block_tids"][:n]
        out["block_cov"] = res["block_cov"][:n * n].reshape(n, n)
    out["stats"] = st
    return out


def asymptotic_host(n_tx, row_ptr, col_idx, theta, row_weight=None, E=None, gene_of_tx=None, n_genes=0, boundary_cut=None, pivot_tol=0.0,
                    block_tid=-1):
    """Host-only: the asymptotic standard errors (include/emsar_hip.h "asymptotic standard errors") of theta from the inverse of the
    observed information, no GPU needed, the same functions the device evaluates.  Rows with E == 0 count no reads; boundary_cut None =
    ASYM_DEFAULT_CUT.  Returns a dict:
    var, sd_fpkm, sd_tpm, rowsum, partner_cov, status (index into ASYM_STATUS), partner, blocker ([n_tx]); with a gene map also
    usage_sd ([n_tx]), gene_sd, gene_status ([n_genes]); with block_tid >= 0 also block_tids [n] and block_cov [n][n]; stats."""
    L = load_library()
    row_ptr, col_idx, th = _arr(row_ptr, np.uint64), _arr(col_idx, np.int32), _arr(theta, np.float64)
    w, e, g = _arr(row_weight, np.int32), _arr(E, np.float64), _arr(gene_of_tx, np.int32)
    n_rows = len(row_ptr) - 1
    for a, n in ((th, n_tx), (w, n_rows), (e, n_rows), (g, n_tx)):
        if a is not None and a.shape != (n,):
            raise ValueError("array of length %d expected" % n)
    res, o = _asym_buffers(int(n_tx), int(n_genes), g is not None, block_tid >= 0)
    p, st = AsymParams(ASYM_DEFAULT_CUT if boundary_cut is None else boundary_cut, pivot_tol, int(block_tid), 0), AsymStats()
    rc = L.emsar_hip_asymptotic_host(n_rows, int(n_tx), _p(row_ptr, C.c_uint64), _p(col_idx, C.c_int32), _p(w, C.c_int32), _p(e, C.c_double),
                                     _p(th, C.c_double), int(n_genes), _p(g, C.c_int32), C.byref(p), C.byref(o), C.byref(st))
    if rc != 0:
        raise EmsarHipError(rc, "asymptotic_host")
    return _asym_result(res, int(n_tx), int(n_genes), st)


def presence_pvalue_host(lam):
    """Host-only: the presence test's p-value of the statistic Lambda under the boundary mixture 1/2 chi2_0 + 1/2 chi2_1 (include/emsar_hip.h
    "presence test"): 1 for Lambda <= 0, 0.5 erfc(sqrt(Lambda / 2)) above, 0 for +inf, NaN for NaN.  A scalar or an array; no GPU needed."""
    L = load_library()
    x = np.ascontiguousarray(np.atleast_1d(np.asarray(lam, dtype=np.float64)))
    out = np.zeros(max(x.size, 1))
    rc = L.emsar_hip_presence_pvalue_host(x.size, _p(x.reshape(-1), C.c_double), _p(out, C.c_double))
    if rc != 0:
        raise EmsarHipError(rc, "presence_pvalue_host")
    out = out[:x.size].reshape(x.shape)
    return float(out[0]) if np.ndim(lam) == 0 else out


def compare_pvalue_host(lam):
    """Host-only: the two-sample test's p-value of the statistic Lambda under chi2 with one degree of freedom (include/emsar_hip.h
    "two-sample test"): 1 for Lambda <= 0, erfc(sqrt(Lambda / 2)) above, 0 for +inf, NaN for NaN.  A scalar or an array; no GPU needed."""
    L = load_library()
    x = np.ascontiguousarray(np.atleast_1d(np.asarray(lam, dtype=np.float64)))
    out = np.zeros(max(x.size, 1))
    rc = L.emsar_hip_compare_pvalue_host(x.size, _p(x.reshape(-1), C.c_double), _p(out, C.c_double))
    if rc != 0:
        raise EmsarHipError(rc, "compare_pvalue_host")
    out = out[:x.size].reshape(x.shape)
    return float(out[0]) if np.ndim(lam) == 0 else out


def debug_compare_closed(u_a, den_a, u_b, den_b, ratio=1.0, dev_tol=0.0, max_evals=0):
    """Host-only diagnostic: what compare() gives a transcript that is a one-transcript component in both samples (u reads, den each):
    the multiplier search as the host runs it for such pairs (no GPU needed).  Returns a dict of scalars keyed like compare()'s arrays."""
    f = load_library().emsar_hip_debug_compare_closed       # not declared in the header: bound here, not in load_library
    f.argtypes = [C.c_double] * 4 + [C.POINTER(CompareParams), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    cp, vals, status, evals = CompareParams(float(ratio), float(dev_tol), int(max_evals), 0), (C.c_double * 9)(), C.c_int32(), C.c_int32()
    rc = f(float(u_a), float(den_a), float(u_b), float(den_b), C.byref(cp), vals, C.byref(status), C.byref(evals))
    if rc != 0:
        raise EmsarHipError(rc, "debug_compare_closed")
    out = dict(zip(COMPARE_OUTPUTS, list(vals)))
    out.update(status=status.value, evals=evals.value)
    return out


def debug_compare_genes_closed(u_a, den_a, u_b, den_b, ratio=1.0, dev_tol=0.0, max_evals=0):
    """Host-only diagnostic: what compare_genes() gives a gene whose parts are all closed form -- one-transcript components with u_a[i]
    reads and den_a[i] in sample A, u_b[j] and den_b[j] in B: the multiplier search as the host runs it for such genes (no GPU needed).
    Returns a dict of scalars keyed like compare_genes()'s arrays."""
    f = load_library().emsar_hip_debug_compare_genes_closed       # not declared in the header: bound here, not in load_library
    f.restype = C.c_int
    dp = C.POINTER(C.c_double)
    f.argtypes = [C.c_int32, dp, dp, C.c_int32, dp, dp, C.POINTER(CompareParams), dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    ua, da, ub, db = (np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (u_a, den_a, u_b, den_b))
    if ua.shape != da.shape or ub.shape != db.shape:
        raise ValueError("u and den of a sample must have the same length")
    cp, vals, status, evals = CompareParams(float(ratio), float(dev_tol), int(max_evals), 0), (C.c_double * 9)(), C.c_int32(), C.c_int32()
    rc = f(len(ua), _p(ua, C.c_double), _p(da, C.c_double), len(ub), _p(ub, C.c_double), _p(db, C.c_double), C.byref(cp), vals,
           C.byref(status), C.byref(evals))
    if rc != 0:
        raise EmsarHipError(rc, "debug_compare_genes_closed")
    out = dict(zip(COMPARE_GENE_OUTPUTS, list(vals)))
    out.update(status=status.value, evals=evals.value)
    return out


def _groups_layout(groups, sizes):
    g = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(-1))
    s = None if sizes is None else np.ascontiguousarray(np.asarray(sizes, dtype=np.float64).reshape(-1))
    if s is not None and len(s) != len(g):
        raise ValueError("sizes must hold one factor per sample")
    n_groups = int(g.max()) + 1 if len(g) and 0 <= int(g.max()) < GROUPS_MAX else 1
    return g, s, n_groups


def compare_groups_pvalue_host(lam, df):
    """Host-only: P(chi2_df > Lambda), the K-sample test's p-value (include/emsar_hip.h "K-sample test"): 1 for Lambda <= 0, 0 for +inf,
    NaN for NaN or df < 0; df 0 is the point mass at 0 (1 for Lambda <= 0, 0 above).  Arrays of equal length, or a scalar df for all;
    no GPU needed."""
    x = np.ascontiguousarray(np.atleast_1d(np.asarray(lam, dtype=np.float64)).reshape(-1))
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(df, dtype=np.int32), x.shape))
    out = np.zeros(max(x.size, 1))
    rc = load_library().emsar_hip_compare_groups_pvalue_host(x.size, _p(x, C.c_double), _p(k, C.c_int32), _p(out, C.c_double))
    if rc != 0:
        raise EmsarHipError(rc, "compare_groups_pvalue_host")
    return out[:x.size]


def debug_compare_groups_closed(u, den, groups, sizes=None, dev_tol=0.0, max_evals=0, max_outer=0):
    """Host-only diagnostic: what compare_groups() gives a transcript that is a one-transcript component in each of the K samples
    (u[k] reads, den[k]): the two-level searches as the host runs them for such transcripts (no GPU needed).  Returns a dict keyed like
    compare_groups()'s arrays: scalars, theta_group [G] and theta_hat [K]."""
    f = load_library().emsar_hip_debug_compare_groups_closed       # not declared in the header: bound here, not in load_library
    f.restype = C.c_int
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    f.argtypes = [C.c_int32, dp, dp, ip, dp, C.POINTER(GroupsParams), dp, dp, dp, ip]
    uu, dd = (np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (u, den))
    g, s, n_groups = _groups_layout(groups, sizes)
    if not (len(uu) == len(dd) == len(g)):
        raise ValueError("u, den and groups must have the same length")
    gp, vals, counts = GroupsParams(float(dev_tol), int(max_evals), int(max_outer)), (C.c_double * 8)(), (C.c_int32 * 3)()
    tg, th = np.zeros(n_groups), np.zeros(max(len(uu), 1))
    rc = f(len(uu), _p(uu, C.c_double), _p(dd, C.c_double), _p(g, C.c_int32), _p(s, C.c_double), C.byref(gp), vals, _p(tg, C.c_double),
           _p(th, C.c_double), counts)
    if rc != 0:
        raise EmsarHipError(rc, "debug_compare_groups_closed")
    out = dict(zip(GROUPS_OUTPUTS, list(vals)))
    out.update(zip(GROUPS_COUNTS, list(counts)))
    out.update(theta_group=tg, theta_hat=th[:len(uu)])
    return out


def debug_compare_groups_genes_closed(members, groups, sizes=None, dev_tol=0.0, max_evals=0, max_outer=0):
    """Host-only diagnostic: what compare_groups_genes() gives a gene whose parts are all closed form in each of the K samples --
    members[k] = a list of (u, den) pairs, the gene's one-transcript components in sample k: the two-level searches as the host runs
    them for such genes (no GPU needed).  Returns a dict keyed like compare_groups_genes()'s arrays: scalars, gene_group [G] and
    gene_hat [K]."""
    f = load_library().emsar_hip_debug_compare_groups_genes_closed  # not declared in the header: bound here, not in load_library
    f.restype = C.c_int
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    f.argtypes = [C.c_int32, ip, dp, dp, ip, dp, C.POINTER(GroupsParams), dp, dp, dp, ip]
    lists = [np.asarray(m, dtype=np.float64).reshape(-1, 2) for m in members]
    n = np.ascontiguousarray([len(m) for m in lists], dtype=np.int32)
    flat = np.concatenate(lists) if lists else np.zeros((0, 2))
    uu, dd = np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])
    g, s, n_groups = _groups_layout(groups, sizes)
    if len(g) != len(lists):
        raise ValueError("members and groups must have the same length")
    gp, vals, counts = GroupsParams(float(dev_tol), int(max_evals), int(max_outer)), (C.c_double * 8)(), (C.c_int32 * 4)()
    tg, th = np.zeros(n_groups), np.zeros(max(len(lists), 1))
    rc = f(len(lists), _p(n, C.c_int32), _p(uu, C.c_double), _p(dd, C.c_double), _p(g, C.c_int32), _p(s, C.c_double), C.byref(gp), vals,
           _p(tg, C.c_double), _p(th, C.c_double), counts)
    if rc != 0:
        raise EmsarHipError(rc, "debug_compare_groups_genes_closed")
    out = dict(zip(GROUPS_GENE_OUTPUTS, list(vals)))
    out.update(zip(GROUPS_GENE_COUNTS, list(counts)))
    out.update(gene_group=tg, gene_hat=th[:len(lists)])
    return out


def debug_compare_usage_closed(u_a, den_a, u_b, den_b, t=0, t_b=None, dev_tol=0.0, max_evals=0, max_outer=0):
    """Host-only diagnostic: what compare_usage() gives member `t` of a gene whose members are all one-transcript components -- u_a[i]
    reads and den_a[i] in sample A, u_b[j] and den_b[j] in B (den 0 = takes no part; t_b = the transcript's place in B's lists when it
    differs): the host's statuses and the two-level search as the host runs it for such genes (no GPU needed).  Returns a dict of
    scalars keyed like compare_usage()'s arrays."""
    f = load_library().emsar_hip_debug_compare_usage_closed       # not declared in the header: bound here, not in load_library
    f.restype = C.c_int
    dp = C.POINTER(C.c_double)
    f.argtypes = [C.c_int32, dp, dp, C.c_int32, C.c_int32, dp, dp, C.c_int32, C.POINTER(UsageParams), dp, C.POINTER(C.c_int32)]
    ua, da, ub, db = (np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (u_a, den_a, u_b, den_b))
    if ua.shape != da.shape or ub.shape != db.shape:
        raise ValueError("u and den of a sample must have the same length")
    up, vals, counts = UsageParams(float(dev_tol), int(max_evals), int(max_outer)), (C.c_double * 8)(), (C.c_int32 * 4)()
    rc = f(len(ua), _p(ua, C.c_double), _p(da, C.c_double), int(t), len(ub), _p(ub, C.c_double), _p(db, C.c_double), int(t if t_b is None else t_b),
           C.byref(up), vals, counts)
    if rc != 0:
        raise EmsarHipError(rc, "debug_compare_usage_closed")
    out = dict(zip(USAGE_OUTPUTS, list(vals)))
    out.update(zip(USAGE_COUNTS, list(counts)))
    return out


def debug_profile_genes_closed(u, den, level=0.95, dev_tol=0.0, max_evals=0):
    """Host-only diagnostic: what profile_genes() gives a gene whose parts are all closed form -- one-transcript components with u[i]
    reads and den[i] each: the searches as the host runs them for such genes, the end-of-range rule included (no GPU needed).  Returns
    a dict of scalars keyed like profile_genes()'s arrays, and evals_upper: the evaluations of the upper search alone."""
    f = load_library().emsar_hip_debug_profile_genes_closed       # not declared in the header: bound here, not in load_library
    f.restype = C.c_int
    dp = C.POINTER(C.c_double)
    f.argtypes = [C.c_int32, dp, dp, C.POINTER(ProfileParams), dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    uu, dd = (np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (u, den))
    if uu.shape != dd.shape:
        raise ValueError("u and den must have the same length")
    pp, vals, status, evals = ProfileParams(float(level), float(dev_tol), int(max_evals), 0), (C.c_double * 8)(), C.c_int32(), C.c_int32()
    rc = f(len(uu), _p(uu, C.c_double), _p(dd, C.c_double), C.byref(pp), vals, C.byref(status), C.byref(evals))
    if rc != 0:
        raise EmsarHipError(rc, "debug_profile_genes_closed")
    out = dict(zip(PROFILE_GENE_OUTPUTS, list(vals)))
    out.update(status=status.value, evals=evals.value, evals_upper=int(vals[7]))
    return out


def debug_profile_usage_closed(u, den, t=0, level=0.95, dev_tol=0.0, max_evals=0, max_outer=0):
    """Host-only diagnostic: what profile_usage() gives member `t` of a gene whose members are all one-transcript components -- u[i]
    reads and den[i] each (den 0 = takes no part): the host's statuses and the searches as the host runs them for such genes (no GPU
    needed).  Returns a dict of scalars keyed like profile_usage()'s arrays."""
    f = load_library().emsar_hip_debug_profile_usage_closed       # not declared in the header: bound here, not in load_library
    f.restype = C.c_int
    dp = C.POINTER(C.c_double)
    f.argtypes = [C.c_int32, dp, dp, C.c_int32, C.POINTER(ProfileParams), dp, C.POINTER(C.c_int32)]
    uu, dd = (np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (u, den))
    if uu.shape != dd.shape:
        raise ValueError("u and den must have the same length")
    pp, vals, counts = ProfileParams(float(level), float(dev_tol), int(max_evals), int(max_outer)), (C.c_double * 7)(), (C.c_int32 * 5)()
    rc = f(len(uu), _p(uu, C.c_double), _p(dd, C.c_double), int(t), C.byref(pp), vals, counts)
    if rc != 0:
        raise EmsarHipError(rc, "debug_profile_usage_closed")
    out = dict(zip(PROFILE_USAGE_OUTPUTS, list(vals)))
    out.update(zip(PROFILE_USAGE_COUNTS, list(counts)))
    return out


def gene_presence_pvalue_host(lam, members):
    """Host-only: the p-value bound of the gene presence test (include/emsar_hip.h "gene-level profile intervals"): P(chi2_k > Lambda)
    with k = members, conservative whatever the weights of the chi-bar-square mixture are; 1 for Lambda <= 0, 0 for +inf, NaN for NaN
    or k < 1.  No GPU needed."""
    lam = np.ascontiguousarray(np.asarray(lam, dtype=np.float64).reshape(-1))
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(members, dtype=np.int32).reshape(-1), lam.shape))
    out = np.zeros(max(len(lam), 1))
    rc = load_library().emsar_hip_gene_presence_pvalue_host(len(lam), _p(lam, C.c_double), _p(k, C.c_int32), _p(out, C.c_double))
    if rc != 0:
        raise EmsarHipError(rc, "gene_presence_pvalue_host")
    return out[:len(lam)]


def profile_cut_host(level):
    """Host-only: the cut q of a profile-likelihood interval (include/emsar_hip.h "profile-likelihood intervals"): the `level` quantile
    of chi2 with one degree of freedom, erf(sqrt(q / 2)) = level; 0 < level < 1.  No GPU needed."""
    out = C.c_double(0.0)
    rc = load_library().emsar_hip_profile_cut_host(float(level), C.byref(out))
    if rc != 0:
        raise EmsarHipError(rc, "profile_cut_host")
    return out.value


def layout_selfcheck_tiled(n_tx, row_ptr, col_idx, merge_rows=False):
    """Host-only: build the TILED layout, check its descriptors and decode it again (no GPU needed).  Returns its statistics."""
    L = load_library()
    row_ptr, col_idx = _arr(row_ptr, np.uint64), _arr(col_idx, np.int32)
    info = Info()
    rc = L.emsar_hip_layout_selfcheck_tiled(len(row_ptr) - 1, n_tx, _p(row_ptr, C.c_uint64), _p(col_idx, C.c_int32),
                                            int(merge_rows), C.byref(info))
    if rc != 0:
        raise EmsarHipError(rc, "layout_selfcheck_tiled")
    d = info.as_dict()
    d["folded_single_rows"] = d.pop("bytes_per_pass")
    return d


def debug_pass_kernel(weighted, mode, n_tiles, tiled_multi=1, weighted_unit=1):
    """Host-only diagnostic: the name of the TILED pass kernel launch_pass picks for a weighted or unweighted sample, a mode (0: EM,
    1: EM with the likelihood, 2: scatter), a tile count and the values of EMSAR_HIP_TILED_MULTI and EMSAR_HIP_WEIGHTED_UNIT (no GPU needed)."""
    f = load_library().emsar_hip_debug_pass_kernel          # not declared in the header: bound here, not in load_library
    f.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(64)
    rc = f(int(bool(weighted)), int(mode), int(n_tiles), int(tiled_multi), int(weighted_unit), buf, len(buf))
    if rc != 0:
        raise EmsarHipError(rc, "debug_pass_kernel")
    return buf.value.decode()


class EmsarHip:
    """One context = one GPU.  Mirrors the call sequence of the reference's per-sample loop
    (emsar_main.c:380-488): upload_structure once per rsh, upload_sample + solve per alignment file."""

    def __init__(self, device_id=0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.emsar_hip_create(C.byref(h), device_id)
        if rc != 0:
            raise EmsarHipError(rc, "emsar_hip_create")
        self._h = h
        self.n_tx = 0
        self.n_rows = 0
        self.n_genes = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.emsar_hip_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise EmsarHipError(rc, what, self._L.emsar_hip_last_error(self._h).decode())

    def upload_structure(self, n_tx, row_ptr, col_idx, layout=LAYOUT_AUTO, merge_rows=False):
        row_ptr, col_idx = _arr(row_ptr, np.uint64), _arr(col_idx, np.int32)
        if merge_rows:
            layout |= FLAG_MERGE_ROWS
        self._chk(self._L.emsar_hip_upload_structure(self._h, len(row_ptr) - 1, n_tx, _p(row_ptr, C.c_uint64),
                                                     _p(col_idx, C.c_int32), layout), "upload_structure")
        self.n_tx = int(n_tx)
        self.n_rows = len(row_ptr) - 1
        self.n_genes = 0                                  # the library drops the gene map

    def upload_sample(self, row_weight=None, row_E=None, den=None):
        w, e, d = _arr(row_weight, np.int32), _arr(row_E, np.float64), _arr(den, np.float64)
        for a, n in ((w, self.n_rows), (e, self.n_rows), (d, self.n_tx)):
            if a is not None and a.shape != (n,):
                raise ValueError("array of length %d expected" % n)
        self._chk(self._L.emsar_hip_upload_sample(self._h, _p(w, C.c_int32), _p(e, C.c_double), _p(d, C.c_double)),
                  "upload_sample")

    def solve(self, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6, check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0,
              newton_after=0):
        """set_mode 0: connected sets that fit a CU's LDS are solved by one workgroup each; 1: streaming passes only.
        newton_after: resident sets get projected-Newton steps once they have used this many passes (0 = 60, < 0 = never)."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        st = EmStats()
        out = np.zeros(self.n_tx)
        self._chk(self._L.emsar_hip_solve(self._h, C.byref(p), _p(out, C.c_double), C.byref(st)), "solve")
        return out, st

    def bootstrap(self, n, seed, first=0, want_replicates=False, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6, check_every=8,
                  count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Poisson bootstrap of the current sample: replicates first .. first+n-1, each solved like solve() with these parameters.
        Returns (fpkm_mean, fpkm_sd, tpm_sd, replicates [n][n_tx] or None, stats)."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        mean, sd, tsd = np.zeros(self.n_tx), np.zeros(self.n_tx), np.zeros(self.n_tx)
        reps = np.zeros((n, self.n_tx)) if (want_replicates and n > 0) else None
        st = BootStats()
        self._chk(self._L.emsar_hip_bootstrap(self._h, C.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(n), _p(mean, C.c_double),
                                              _p(sd, C.c_double), _p(tsd, C.c_double), _p(reps, C.c_double), C.byref(st)), "bootstrap")
        return mean, sd, tsd, reps, st

    def set_gene_map(self, gene_of_tx, n_genes):
        """gene_of_tx[t] = gene of transcript t (caller numbering) in 0 .. n_genes-1, -1 = no gene.  After upload_structure."""
        g = _arr(gene_of_tx, np.int32)
        if self.n_tx and g.shape != (self.n_tx,):          # (before upload_structure the library answers: ERR_STATE)
            raise ValueError("gene_of_tx must have n_tx entries")
        self._chk(self._L.emsar_hip_set_gene_map(self._h, int(n_genes), _p(g, C.c_int32)), "set_gene_map")
        self.n_genes = int(n_genes)

    def gene_sums(self, cols):
        """Per-gene sums of transcript values in the library's fixed order (include/emsar_hip.h): cols [n_cols][n_tx] -> [n_cols][n_genes],
        a single vector [n_tx] -> [n_genes]."""
        x = _arr(cols, np.float64)
        one = x.ndim == 1
        x = np.ascontiguousarray(np.atleast_2d(x))
        if x.shape[1] != self.n_tx:
            raise ValueError("columns of n_tx values expected")
        out = np.zeros((x.shape[0], max(self.n_genes, 1)))
        self._chk(self._L.emsar_hip_gene_sums(self._h, x.shape[0], _p(x, C.c_double), _p(out, C.c_double)), "gene_sums")
        out = out[:, :self.n_genes]
        return out[0] if one else out

    def bootstrap_genes(self, n, seed, first=0, want_replicates=False, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6, check_every=8,
                        count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """bootstrap() plus per-gene statistics over the same replicates.  Returns a dict: fpkm_mean, fpkm_sd, tpm_sd, replicates
        ([n][n_tx] or None), gene_fpkm_mean, gene_fpkm_sd, gene_tpm_sd, stats."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        T, G = self.n_tx, max(self.n_genes, 1)
        mean, sd, tsd = np.zeros(T), np.zeros(T), np.zeros(T)
        gm, gs, gt = np.zeros(G), np.zeros(G), np.zeros(G)
        reps = np.zeros((n, T)) if (want_replicates and n > 0) else None
        st = BootStats()
        self._chk(self._L.emsar_hip_bootstrap_genes(self._h, C.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(n), _p(mean, C.c_double),
                                                    _p(sd, C.c_double), _p(tsd, C.c_double), _p(reps, C.c_double), _p(gm, C.c_double),
                                                    _p(gs, C.c_double), _p(gt, C.c_double), C.byref(st)), "bootstrap_genes")
        k = self.n_genes
        return {"fpkm_mean": mean, "fpkm_sd": sd, "tpm_sd": tsd, "replicates": reps, "gene_fpkm_mean": gm[:k], "gene_fpkm_sd": gs[:k],
                "gene_tpm_sd": gt[:k], "stats": st}

    def bootstrap_quantiles(self, n, q, seed, first=0, want_replicates=False, want_genes=False, max_iter=100000, accel=1, tol=1e-10,
                            abs_floor=1e-6, check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """bootstrap() / bootstrap_genes() plus, per transcript (with want_genes: and per gene), the q-quantiles of FPKM and TPM over the
        same replicates (definition: include/emsar_hip.h; n <= 4096).  Returns a dict: fpkm_mean, fpkm_sd, tpm_sd, replicates ([n][n_tx]
        or None), replicate_sums ([n], the TPM denominators), fpkm_q, tpm_q ([n_q][n_tx]), with want_genes also gene_fpkm_mean,
        gene_fpkm_sd, gene_tpm_sd ([n_genes]), gene_fpkm_q, gene_tpm_q ([n_q][n_genes]), stats, qstats."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        K, T, G = len(qa), self.n_tx, max(self.n_genes, 1)
        Ka, na = max(K, 1), max(int(n), 1)
        out = {k: np.zeros(T) for k in ("fpkm_mean", "fpkm_sd", "tpm_sd")}
        out.update(fpkm_q=np.zeros((Ka, T)), tpm_q=np.zeros((Ka, T)), replicate_sums=np.zeros(na))
        reps = np.zeros((n, T)) if (want_replicates and n > 0) else None
        gene = {k: np.zeros(G) for k in ("gene_fpkm_mean", "gene_fpkm_sd", "gene_tpm_sd")} if want_genes else {}
        if want_genes:
            gene.update(gene_fpkm_q=np.zeros((Ka, G)), gene_tpm_q=np.zeros((Ka, G)))
        st, qs = BootStats(), QuantileStats()
        d = lambda a: _p(a, C.c_double)
        self._chk(self._L.emsar_hip_bootstrap_quantiles(
            self._h, C.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(n), K, d(qa), d(out["fpkm_mean"]), d(out["fpkm_sd"]),
            d(out["tpm_sd"]), d(reps), d(out["replicate_sums"]), d(out["fpkm_q"]), d(out["tpm_q"]), d(gene.get("gene_fpkm_mean")),
            d(gene.get("gene_fpkm_sd")), d(gene.get("gene_tpm_sd")), d(gene.get("gene_fpkm_q")), d(gene.get("gene_tpm_q")),
            C.byref(st), C.byref(qs)), "bootstrap_quantiles")
        k = self.n_genes
        out.update({key: (v[:, :k] if v.ndim == 2 else v[:k]) for key, v in gene.items()})
        out.update(replicates=reps, stats=st, qstats=qs)
        return out

    def isoform_usage(self, cols, want_dominant=False):
        """Each transcript's share of its gene's sum (include/emsar_hip.h "isoform usage"): cols [n_cols][n_tx] -> usage [n_cols][n_tx],
        a single vector [n_tx] -> [n_tx]; with want_dominant (usage, dominant [n_cols][n_genes] or [n_genes]: the tid of every
        gene's dominant isoform, -1 for a gene whose sum is 0).  After set_gene_map."""
        x = _arr(cols, np.float64)
        one = x.ndim == 1
        x = np.ascontiguousarray(np.atleast_2d(x))
        if x.shape[1] != self.n_tx:
            raise ValueError("columns of n_tx values expected")
        usage = np.zeros(x.shape)
        dom = np.zeros((x.shape[0], max(self.n_genes, 1)), dtype=np.int32) if want_dominant else None
        self._chk(self._L.emsar_hip_isoform_usage(self._h, x.shape[0], _p(x, C.c_double), _p(usage, C.c_double), _p(dom, C.c_int32)),
                  "isoform_usage")
        if not want_dominant:
            return usage[0] if one else usage
        dom = dom[:, :self.n_genes]
        return (usage[0], dom[0]) if one else (usage, dom)

    def bootstrap_isoforms(self, n, seed, q=None, first=0, want_replicates=False, want_genes=False, max_iter=100000, accel=1, tol=1e-10,
                           abs_floor=1e-6, check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """bootstrap_quantiles() (q given) or bootstrap() / bootstrap_genes() (q None) plus the isoform statistics over the same
        replicates: usage_mean, usage_sd ([n_tx]: mean and sample sd of each transcript's share of its gene), dominant_count ([n_tx] int32:
        replicates in which it is its gene's dominant isoform) and, with q, usage_q ([n_q][n_tx]).  The other keys are those of
        bootstrap_quantiles; without q there are no *_q, replicate_sums and qstats.  After set_gene_map."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        qa = None if q is None else np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        K, T, G = (0 if qa is None else len(qa)), self.n_tx, max(self.n_genes, 1)
        Ka, na = max(K, 1), max(int(n), 1)
        out = {k: np.zeros(T) for k in ("fpkm_mean", "fpkm_sd", "tpm_sd", "usage_mean", "usage_sd")}
        out["dominant_count"] = np.zeros(max(T, 1), dtype=np.int32)
        gene = {k: np.zeros(G) for k in ("gene_fpkm_mean", "gene_fpkm_sd", "gene_tpm_sd")} if want_genes else {}
        if qa is not None:
            out.update(fpkm_q=np.zeros((Ka, T)), tpm_q=np.zeros((Ka, T)), replicate_sums=np.zeros(na), usage_q=np.zeros((Ka, T)))
            if want_genes:
                gene.update(gene_fpkm_q=np.zeros((Ka, G)), gene_tpm_q=np.zeros((Ka, G)))
        reps = np.zeros((n, T)) if (want_replicates and n > 0) else None
        st, qs = BootStats(), QuantileStats()
        d = lambda a: _p(a, C.c_double)
        iso = IsoformOutputs(d(out["usage_mean"]), d(out["usage_sd"]), _p(out["dominant_count"], C.c_int32), d(out.get("usage_q")))
        self._chk(self._L.emsar_hip_bootstrap_isoforms(
            self._h, C.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(n), K, d(qa), d(out["fpkm_mean"]), d(out["fpkm_sd"]),
            d(out["tpm_sd"]), d(reps), d(out.get("replicate_sums")), d(out.get("fpkm_q")), d(out.get("tpm_q")), d(gene.get("gene_fpkm_mean")),
            d(gene.get("gene_fpkm_sd")), d(gene.get("gene_tpm_sd")), d(gene.get("gene_fpkm_q")), d(gene.get("gene_tpm_q")),
            C.byref(st), C.byref(qs), C.byref(iso)), "bootstrap_isoforms")
        k = self.n_genes
        out["dominant_count"] = out["dominant_count"][:T]
        out.update({key: (v[:, :k] if v.ndim == 2 else v[:k]) for key, v in gene.items()})
        out.update(replicates=reps, stats=st)
        if qa is not None:
            out["qstats"] = qs
        return out

    def model_fit(self, theta, E=None, rows=False, genes=False):
        """Does theta explain the current sample's reads (include/emsar_hip.h "model fit")?  E None = 1.0 per row.  Returns a dict:
        tx_chi2, tx_dev, tx_miss, tx_df, tx_worst_row ([n_tx]; the row whose miss weighs most on the transcript, -1 = none), with rows
        also row_mu, row_chi2, row_dev ([n_rows]), with genes (after set_gene_map) also gene_chi2, gene_dev, gene_miss, gene_df
        ([n_genes]), and stats.  After upload_sample; the context is left as it was."""
        th, e = _arr(theta, np.float64), _arr(E, np.float64)
        for a, n in ((th, self.n_tx), (e, self.n_rows)):
            if a is not None and a.shape != (n,):
                raise ValueError("array of length %d expected" % n)
        res, o = _fit_buffers(self.n_rows, self.n_tx, self.n_genes, rows, genes)
        st = FitStats()
        self._chk(self._L.emsar_hip_model_fit(self._h, _p(th, C.c_double), _p(e, C.c_double), C.byref(o), C.byref(st)), "model_fit")
        return _fit_result(res, self.n_rows, self.n_tx, self.n_genes, st)

    def presence(self, query=None, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6, check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0,
                 abs_step=0.0, newton_after=0):
        """Likelihood-ratio test of each queried transcript (include/emsar_hip.h "presence test"): is it needed to explain the reads, or
        would the rest of its connected set do as well?  query: tids in any order, repeats allowed, None = all transcripts; the solver
        parameters are those of solve().  Returns a dict of arrays in query order: lambda, pvalue, heir (tid, -1 = none), heir_share,
        status (index into PRESENCE_STATUS), theta_hat, and stats.  After upload_sample; the context is left as it was."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_tx if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in ("lambda", "pvalue", "heir_share", "theta_hat")}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in ("heir", "status")})
        o = PresenceOutputs(_p(res["lambda"], C.c_double), _p(res["pvalue"], C.c_double), _p(res["heir"], C.c_int32), _p(res["heir_share"], C.c_double),
                            _p(res["status"], C.c_int32), _p(res["theta_hat"], C.c_double))
        st = PresenceStats()
        self._chk(self._L.emsar_hip_presence(self._h, C.byref(p), nq, _p(q, C.c_int32), C.byref(o), C.byref(st)), "presence")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def profile(self, query=None, level=0.95, dev_tol=0.0, max_evals=0, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6, check_every=8,
                count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Profile-likelihood interval of each queried transcript (include/emsar_hip.h "profile-likelihood intervals"): the values of
        theta_t whose best achievable likelihood lies within the chi2_1 cut of `level` of the maximum; one-sided by itself where the
        transcript cannot be told from absent.  query: tids in any order, repeats allowed, None = all transcripts; dev_tol, max_evals 0 =
        the defaults (1e-4, 40); the solver parameters are those of solve().  Returns a dict of arrays in query order: lower, upper,
        dev_lower, dev_upper, lambda, theta_hat, status (index into PROFILE_STATUS), evals, and stats.  After upload_sample; the context
        is left as it was."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        pp = ProfileParams(float(level), float(dev_tol), int(max_evals), 0)
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_tx if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda", "theta_hat")}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in ("status", "evals")})
        o = ProfileOutputs(*[_p(res[k], C.c_double) for k in ("lower", "upper", "dev_lower", "dev_upper", "lambda", "theta_hat")],
                           _p(res["status"], C.c_int32), _p(res["evals"], C.c_int32))
        st = ProfileStats()
        self._chk(self._L.emsar_hip_profile(self._h, C.byref(p), C.byref(pp), nq, _p(q, C.c_int32), C.byref(o), C.byref(st)), "profile")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def compare(self, other, query=None, ratio=1.0, dev_tol=0.0, max_evals=0, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6, check_every=8,
                count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Two-sample likelihood-ratio test of each queried transcript (include/emsar_hip.h "two-sample test"): this context holds sample
        A, `other` -- a second context on the same device with the same structure -- sample B; H0: theta_t^A = ratio * theta_t^B with
        every other transcript free in both samples.  query: tids in any order, repeats allowed, None = all transcripts; dev_tol,
        max_evals 0 = the defaults (1e-4, 40); the solver parameters are those of solve().  Returns a dict of arrays in query order:
        lambda, pvalue, log2fc, theta_a, theta_b, theta_null, multiplier, gap, raw_lambda, status (index into COMPARE_STATUS), evals, and
        stats.  After upload_sample on both; both contexts are left as they were."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        cp = CompareParams(float(ratio), float(dev_tol), int(max_evals), 0)
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_tx if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in COMPARE_OUTPUTS}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in ("status", "evals")})
        o = CompareOutputs(*[_p(res[k], C.c_double) for k in COMPARE_OUTPUTS], _p(res["status"], C.c_int32), _p(res["evals"], C.c_int32))
        st = CompareStats()
        self._chk(self._L.emsar_hip_compare(self._h, getattr(other, "_h", None), C.byref(p), C.byref(cp), nq, _p(q, C.c_int32), C.byref(o), C.byref(st)),
                  "compare")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def compare_genes(self, other, query=None, ratio=1.0, dev_tol=0.0, max_evals=0, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6,
                      check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Two-sample likelihood-ratio test of each queried gene (include/emsar_hip.h "gene-level two-sample test"): this context holds
        sample A and the gene map (set_gene_map), `other` sample B; H0: the gene's sum of theta in A = ratio * its sum in B, with the
        isoforms and every other transcript free in both samples.  query: gene ids in any order, repeats allowed, None = all genes; the
        other parameters are compare()'s.  Returns a dict of arrays in query order: lambda, pvalue, log2fc, gene_a, gene_b, gene_null,
        multiplier, gap, raw_lambda, status (index into COMPARE_GENE_STATUS), evals, parts, and stats.  After upload_sample on both; both
        contexts are left as they were."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        cp = CompareParams(float(ratio), float(dev_tol), int(max_evals), 0)
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_genes if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in COMPARE_GENE_OUTPUTS}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in ("status", "evals", "parts")})
        o = CompareGeneOutputs(*[_p(res[k], C.c_double) for k in COMPARE_GENE_OUTPUTS],
                               *[_p(res[k], C.c_int32) for k in ("status", "evals", "parts")])
        st = CompareGeneStats()
        self._chk(self._L.emsar_hip_compare_genes(self._h, getattr(other, "_h", None), C.byref(p), C.byref(cp), nq, _p(q, C.c_int32), C.byref(o),
                                                  C.byref(st)), "compare_genes")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def compare_usage(self, other, query=None, dev_tol=0.0, max_evals=0, max_outer=0, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6,
                      check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Two-sample test of isoform usage (include/emsar_hip.h "two-sample test of isoform usage"): did the share of each queried
        transcript in its gene change between this context's sample A and `other`'s sample B?  H0: theta_t / (the gene sum) is the same
        in both samples, everything else free.  This context holds the gene map (set_gene_map).  query: tids in any order, repeats
        allowed, None = all transcripts; dev_tol, max_evals, max_outer 0 = the defaults (1e-4, 40, 12); the solver parameters are those
        of solve().  Returns a dict of arrays in query order: lambda, raw_lambda, pvalue, usage_a, usage_b, usage_null, dlogit, slope,
        status (index into USAGE_STATUS), outer_evals, evals, parts, and stats.  After upload_sample on both; both contexts are left as
        they were."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        up = UsageParams(float(dev_tol), int(max_evals), int(max_outer))
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_tx if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in USAGE_OUTPUTS}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in USAGE_COUNTS})
        o = UsageOutputs(*[_p(res[k], C.c_double) for k in USAGE_OUTPUTS], *[_p(res[k], C.c_int32) for k in USAGE_COUNTS])
        st = UsageStats()
        self._chk(self._L.emsar_hip_compare_usage(self._h, getattr(other, "_h", None), C.byref(p), C.byref(up), nq, _p(q, C.c_int32), C.byref(o),
                                                  C.byref(st)), "compare_usage")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def compare_groups(self, others, groups, sizes=None, query=None, dev_tol=0.0, max_evals=0, max_outer=0, max_iter=100000, accel=1, tol=1e-10,
                       abs_floor=1e-6, check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """K-sample test across replicate groups (include/emsar_hip.h "K-sample test"): this context holds sample 0, `others` -- a list of
        contexts on the same device with the same structure -- samples 1 .. K-1; groups[k] in 0 .. G-1 names sample k's group, sizes[k] > 0
        its size factor (None: all 1).  Lambda_between tests "the groups differ" with the replicates of a group pooled inside the
        likelihood, Lambda_within "the replicates of a group disagree".  query: tids in any order, repeats allowed, None = all
        transcripts; dev_tol, max_evals, max_outer 0 = the defaults (1e-4, 40, 12); the solver parameters are those of solve().  Returns
        a dict of arrays in query order: lambda_between, p_between, lambda_within, p_within, raw_between, raw_within, theta_common, slope,
        theta_group [n, G], theta_hat [n, K], status (index into GROUPS_STATUS), outer, evals, and stats.  After upload_sample on every
        context; all are left as they were."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        gp = GroupsParams(float(dev_tol), int(max_evals), int(max_outer))
        ctxs = [self] + list(others)
        g, s, n_groups = _groups_layout(groups, sizes)
        if len(g) != len(ctxs):
            raise ValueError("groups must hold one id per sample")
        handles = (C.c_void_p * len(ctxs))(*[getattr(c, "_h", None) for c in ctxs])
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_tx if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in GROUPS_OUTPUTS}
        res["theta_group"] = np.zeros((max(nq, 1), n_groups))
        res["theta_hat"] = np.zeros((max(nq, 1), len(ctxs)))
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in GROUPS_COUNTS})
        o = GroupsOutputs(*[_p(res[k], C.c_double) for k in GROUPS_OUTPUTS + ("theta_group", "theta_hat")],
                          *[_p(res[k], C.c_int32) for k in GROUPS_COUNTS])
        st = GroupsStats()
        self._chk(self._L.emsar_hip_compare_groups(handles, len(ctxs), _p(g, C.c_int32), _p(s, C.c_double), C.byref(p), C.byref(gp), nq,
                                                   _p(q, C.c_int32), C.byref(o), C.byref(st)), "compare_groups")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def compare_groups_genes(self, others, groups, sizes=None, genes=None, dev_tol=0.0, max_evals=0, max_outer=0, max_iter=100000, accel=1,
                             tol=1e-10, abs_floor=1e-6, check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Gene-level K-sample test across replicate groups (include/emsar_hip.h "gene-level K-sample test"): compare_groups() asked of
        each gene's SUM of theta, the isoforms and every other transcript free in every sample.  This context holds sample 0 and the gene
        map (set_gene_map), `others` samples 1 .. K-1; groups, sizes and the parameters are compare_groups()'s.  genes: gene ids in any
        order, repeats allowed, None = all genes.  Returns a dict of arrays in query order: lambda_between, p_between, lambda_within,
        p_within, raw_between, raw_within, gene_common, slope, gene_group [n, G], gene_hat [n, K], status (index into
        GROUPS_GENE_STATUS), outer, evals, parts, and stats.  After upload_sample on every context; all are left as they were."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        gp = GroupsParams(float(dev_tol), int(max_evals), int(max_outer))
        ctxs = [self] + list(others)
        g, s, n_groups = _groups_layout(groups, sizes)
        if len(g) != len(ctxs):
            raise ValueError("groups must hold one id per sample")
        handles = (C.c_void_p * len(ctxs))(*[getattr(c, "_h", None) for c in ctxs])
        q = None if genes is None else np.ascontiguousarray(np.asarray(genes, dtype=np.int32).reshape(-1))
        nq = self.n_genes if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in GROUPS_GENE_OUTPUTS}
        res["gene_group"] = np.zeros((max(nq, 1), n_groups))
        res["gene_hat"] = np.zeros((max(nq, 1), len(ctxs)))
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in GROUPS_GENE_COUNTS})
        o = GroupsGeneOutputs(*[_p(res[k], C.c_double) for k in GROUPS_GENE_OUTPUTS + ("gene_group", "gene_hat")],
                              *[_p(res[k], C.c_int32) for k in GROUPS_GENE_COUNTS])
        st = GroupsGeneStats()
        self._chk(self._L.emsar_hip_compare_groups_genes(handles, len(ctxs), _p(g, C.c_int32), _p(s, C.c_double), C.byref(p), C.byref(gp), nq,
                                                         _p(q, C.c_int32), C.byref(o), C.byref(st)), "compare_groups_genes")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def profile_genes(self, query=None, level=0.95, dev_tol=0.0, max_evals=0, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6,
                      check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Profile-likelihood interval of each queried gene's total and the gene presence test (include/emsar_hip.h "gene-level profile
        intervals"): the values of the gene's sum of theta whose best achievable likelihood -- the isoforms and every other transcript
        free -- lies within the chi2_1 cut of `level` of the maximum, and Lambda = the deviance of the sum 0.  query: gene ids in any
        order, repeats allowed, None = all genes; the other parameters are profile()'s.  Returns a dict of arrays in query order: lower,
        upper, dev_lower, dev_upper, lambda, pvalue, gene_hat, status (index into PROFILE_GENE_STATUS), evals, parts, members, and
        stats.  After upload_sample and set_gene_map; the context is left as it was."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        pp = ProfileParams(float(level), float(dev_tol), int(max_evals), 0)
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_genes if q is None else len(q)
        ints = ("status", "evals", "parts", "members")
        res = {k: np.zeros(max(nq, 1)) for k in PROFILE_GENE_OUTPUTS}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in ints})
        o = ProfileGeneOutputs(*[_p(res[k], C.c_double) for k in PROFILE_GENE_OUTPUTS], *[_p(res[k], C.c_int32) for k in ints])
        st = ProfileGeneStats()
        self._chk(self._L.emsar_hip_profile_genes(self._h, C.byref(p), C.byref(pp), nq, _p(q, C.c_int32), C.byref(o), C.byref(st)), "profile_genes")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def profile_usage(self, query=None, level=0.95, dev_tol=0.0, max_evals=0, max_outer=0, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6,
                      check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Profile-likelihood interval of each queried transcript's share of its gene (include/emsar_hip.h "profile-likelihood
        intervals of isoform usage"): the shares theta_t / (the gene sum) whose best achievable likelihood -- everything else free --
        lies within the chi2_1 cut of `level` of the maximum.  query: tids in any order, repeats allowed, None = all transcripts; level,
        dev_tol, max_evals as in profile(), max_outer 0 = 24 outer points per limit; the solver parameters are those of solve().
        Returns a dict of arrays in query order: usage, lower, upper, dev_lower, dev_upper, lambda_zero, lambda_one, status (index into
        PROFILE_USAGE_STATUS), outer_evals, evals, parts, members, and stats.  After upload_sample and set_gene_map; the context is left
        as it was."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        pp = ProfileParams(float(level), float(dev_tol), int(max_evals), int(max_outer))
        q = None if query is None else np.ascontiguousarray(np.asarray(query, dtype=np.int32).reshape(-1))
        nq = self.n_tx if q is None else len(q)
        res = {k: np.zeros(max(nq, 1)) for k in PROFILE_USAGE_OUTPUTS}
        res.update({k: np.zeros(max(nq, 1), dtype=np.int32) for k in PROFILE_USAGE_COUNTS})
        o = ProfileUsageOutputs(*[_p(res[k], C.c_double) for k in PROFILE_USAGE_OUTPUTS], *[_p(res[k], C.c_int32) for k in PROFILE_USAGE_COUNTS])
        st = ProfileUsageStats()
        self._chk(self._L.emsar_hip_profile_usage(self._h, C.byref(p), C.byref(pp), nq, _p(q, C.c_int32), C.byref(o), C.byref(st)), "profile_usage")
        out = {k: v[:nq] for k, v in res.items()}
        out["stats"] = st
        return out

    def asymptotic(self, theta, boundary_cut=None, pivot_tol=0.0, block_tid=-1, genes=False):
        """Asymptotic standard errors of theta from the inverse of the observed information of the current sample (include/emsar_hip.h
        "asymptotic standard errors"); asymptotic_host describes the result.  genes (after set_gene_map) adds usage_sd, gene_sd and
        gene_status.  After upload_sample; the context is left as it was."""
        th = _arr(theta, np.float64)
        if th.shape != (self.n_tx,):
            raise ValueError("array of length %d expected" % self.n_tx)
        res, o = _asym_buffers(self.n_tx, self.n_genes, genes, block_tid >= 0)
        p, st = AsymParams(ASYM_DEFAULT_CUT if boundary_cut is None else boundary_cut, pivot_tol, int(block_tid), 0), AsymStats()
        self._chk(self._L.emsar_hip_asymptotic(self._h, _p(th, C.c_double), C.byref(p), C.byref(o), C.byref(st)), "asymptotic")
        return _asym_result(res, self.n_tx, self.n_genes, st)

    def bootstrap_weights(self, seed, replicate):
        """The drawn row weights of one bootstrap replicate (caller row order), drawn on the device."""
        out = np.zeros(max(self.n_rows, 1), dtype=np.int32)
        self._chk(self._L.emsar_hip_bootstrap_weights(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(replicate), _p(out, C.c_int32)),
                  "bootstrap_weights")
        return out[:self.n_rows]

    def subsample(self, fractions, n, seed, want_replicates=False, want_genes=False, max_iter=100000, accel=1, tol=1e-10, abs_floor=1e-6,
                  check_every=8, count_floor=0.0, set_mode=0, zero_cut=0.0, abs_step=0.0, newton_after=0):
        """Binomial depth subsampling of the current sample: for each fraction f in (0, 1], n replicates with w ~ Binomial(R, f), each
        solved like solve() with these parameters and scaled to its own depth.  Returns a dict: fpkm_mean, fpkm_sd, tpm_mean, tpm_sd
        ([n_fractions][n_tx]), depth_mean ([n_fractions]), replicates ([n_fractions][n][n_tx] or None), with want_genes also
        gene_fpkm_mean, gene_fpkm_sd, gene_tpm_mean ([n_fractions][n_genes]), stats."""
        p = EmParams(max_iter, accel, tol, abs_floor, check_every, set_mode, count_floor, zero_cut, abs_step, newton_after, 0)
        fr = np.ascontiguousarray(np.atleast_1d(np.asarray(fractions, dtype=np.float64)))
        K, T, G = len(fr), self.n_tx, max(self.n_genes, 1)
        Ka = max(K, 1)
        out = {k: np.zeros((Ka, T)) for k in ("fpkm_mean", "fpkm_sd", "tpm_mean", "tpm_sd")}
        depth = np.zeros(Ka)
        reps = np.zeros((Ka, n, T)) if (want_replicates and n > 0) else None
        gene = {k: np.zeros((Ka, G)) for k in ("gene_fpkm_mean", "gene_fpkm_sd", "gene_tpm_mean")} if want_genes else {}
        st = SubsampleStats()
        self._chk(self._L.emsar_hip_subsample(self._h, C.byref(p), int(seed) & 0xFFFFFFFFFFFFFFFF, K, _p(fr, C.c_double), int(n),
                                              _p(out["fpkm_mean"], C.c_double), _p(out["fpkm_sd"], C.c_double), _p(out["tpm_mean"], C.c_double),
                                              _p(out["tpm_sd"], C.c_double), _p(depth, C.c_double), _p(reps, C.c_double),
                                              _p(gene.get("gene_fpkm_mean"), C.c_double), _p(gene.get("gene_fpkm_sd"), C.c_double),
                                              _p(gene.get("gene_tpm_mean"), C.c_double), C.byref(st)), "subsample")
        out.update(depth_mean=depth, replicates=reps, stats=st)
        out.update({k: v[:, :self.n_genes] for k, v in gene.items()})
        return out

    def subsample_weights(self, seed, replicate, fraction):
        """The drawn row weights of one subsampling replicate at one fraction (caller row order), drawn on the device."""
        out = np.zeros(max(self.n_rows, 1), dtype=np.int32)
        self._chk(self._L.emsar_hip_subsample_weights(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(replicate), float(fraction), _p(out, C.c_int32)),
                  "subsample_weights")
        return out[:self.n_rows]

    def collapse_rows(self, n_tx, row_ptr, col_idx, row_weight=None, want_map=True):
        """Read -> segment collapse on the device: rows with the same multiset of ids become one weighted row.
        Returns (row_ptr, col_idx, weight, row_map, stats); unique rows in order of first occurrence, ids sorted."""
        row_ptr, col_idx = _arr(row_ptr, np.uint64), _arr(col_idx, np.int32)
        n_rows = len(row_ptr) - 1
        w = None if row_weight is None else _arr(row_weight, np.int32)
        rp_o = np.zeros(n_rows + 1, dtype=np.uint64)
        ci_o = np.zeros(max(len(col_idx), 1), dtype=np.int32)
        w_o = np.zeros(max(n_rows, 1), dtype=np.int32)
        m_o = np.zeros(max(n_rows, 1), dtype=np.int32) if want_map else None
        nu = C.c_int64(0)
        st = CollapseStats()
        self._chk(self._L.emsar_hip_collapse_rows(self._h, n_rows, n_tx, _p(row_ptr, C.c_uint64), _p(col_idx, C.c_int32),
                                                  None if w is None else _p(w, C.c_int32), C.byref(nu), _p(rp_o, C.c_uint64),
                                                  _p(ci_o, C.c_int32), _p(w_o, C.c_int32), None if m_o is None else _p(m_o, C.c_int32),
                                                  C.byref(st)), "collapse_rows")
        u = nu.value
        return rp_o[:u + 1], ci_o[:int(rp_o[u])], w_o[:u], (None if m_o is None else m_o[:n_rows]), st

    def upload_euma(self, euma):
        """EUMA[n_rows][nfl] (int32, 0 where absent): once per rsh, after upload_structure."""
        euma = _arr(euma, np.int32)
        if euma.ndim != 2 or euma.shape[0] != self.n_rows:
            raise ValueError("euma must be [n_rows][nfl]")
        self.nfl = int(euma.shape[1])
        self._chk(self._L.emsar_hip_upload_euma(self._h, _p(euma, C.c_int32), self.nfl), "upload_euma")

    def adj_euma(self, wf):
        """L_c = sum_i Wf[i] * EUMA_c[i] (compute_adjEUMA), bit-identical to the host loop."""
        wf = _arr(wf, np.float64)
        if wf.shape != (getattr(self, "nfl", -1),):
            raise ValueError("wf must have nfl entries")
        out = np.zeros(self.n_rows)
        self._chk(self._L.emsar_hip_adj_euma(self._h, _p(wf, C.c_double), _p(out, C.c_double)), "adj_euma")
        return out

    def reset_theta(self):
        self._chk(self._L.emsar_hip_reset_theta(self._h), "reset_theta")

    def set_theta(self, theta):
        theta = _arr(theta, np.float64)
        if theta.shape != (self.n_tx,):
            raise ValueError("theta must have n_tx entries")
        self._chk(self._L.emsar_hip_set_theta(self._h, _p(theta, C.c_double)), "set_theta")

    def get_theta(self):
        out = np.zeros(self.n_tx)
        self._chk(self._L.emsar_hip_get_theta(self._h, _p(out, C.c_double)), "get_theta")
        return out

    def set_deterministic(self, on=True):
        """Fixed-point sums in the streaming passes: two solves of the same input are bit-identical (include/emsar_hip.h)."""
        self._chk(self._L.emsar_hip_set_deterministic(self._h, 1 if on else 0), "set_deterministic")

    def run_passes(self, n, want_loglik=False):
        ms = C.c_float(0)
        ll = C.c_double(0)
        self._chk(self._L.emsar_hip_run_passes(self._h, n, C.byref(ms), C.byref(ll) if want_loglik else None),
                  "run_passes")
        return (ms.value, ll.value) if want_loglik else ms.value

    def ieuma(self, row_L):
        row_L = _arr(row_L, np.float64)
        out = np.zeros(self.n_tx)
        self._chk(self._L.emsar_hip_ieuma(self._h, _p(row_L, C.c_double), _p(out, C.c_double)), "ieuma")
        return out

    def normalise(self, mean_fpkm, ieuma, total_read_count):
        m, ie = _arr(mean_fpkm, np.float64), _arr(ieuma, np.float64)
        tpm, ir = np.zeros(self.n_tx), np.zeros(self.n_tx)
        iri = np.zeros(self.n_tx, dtype=np.int32)
        self._chk(self._L.emsar_hip_normalise(self._h, _p(m, C.c_double), _p(ie, C.c_double), int(total_read_count),
                                              _p(tpm, C.c_double), _p(ir, C.c_double), _p(iri, C.c_int32)), "normalise")
        return tpm, ir, iri

    def info(self):
        i = Info()
        self._chk(self._L.emsar_hip_get_info(self._h, C.byref(i)), "get_info")
        return i.as_dict()
