/* emsar_hip.h -- C ABI of libemsar_hip.so, the MI355X (gfx950) abundance-estimation core.
 *
 * Drop-in boundary: the reference has no plugin API; the seam is the call
 *     run_MLE_threads();                                   /root/reference/src/emsar_main.c:446
 * bracketed by construct_EUMAps() (emsar_main.c:436) and construct_FPKMfinal(round) (emsar_main.c:448),
 * which reads the globals CT, ReadCount, EUMAps, SC, ST (emsar.h:129-170) and writes FPKM[0..max_tid].
 * This library replaces that call, plus compute_iEUMA (emsar_functions.c:3218-3232) and the numeric part
 * of print_FPKMfinal (emsar_functions.c:3176-3207).  Plain C types only: a C host (ours: emsar_amd/csrc/host,
 * or the reference's emsar_main.c with the stub shown in INTEGRATION.md) links it directly.
 *
 * Conventions: every entry point returns 0 on success or a negative emsar_hip_status; nothing exits the
 * process (the reference exit(1)s, e.g. emsar_functions.c:3133).  The caller keeps ownership of all host
 * arrays; they may be freed as soon as the call returns.  One context per GPU; contexts share nothing, so
 * the -M multi-sample path (emsar_main.c:380-488) runs one host thread or process per device.
 *
 * Matrix convention: row c = one segment (a distinct tid multiset, CT[c], emsar.h:129) or one read;
 * columns = transcript ids; a tid may repeat inside a row and then counts twice, exactly as lambdap and
 * compute_iEUMA count it (emsar_functions.c:2969-2973, 3226-3228).
 */
#ifndef EMSAR_HIP_H
#define EMSAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emsar_hip_ctx emsar_hip_ctx; /* opaque; one per GPU */

typedef enum {
    EMSAR_HIP_OK = 0,
    EMSAR_HIP_ERR_ARG = -1,        /* NULL / out-of-range argument, malformed CSR (tid outside [0,n_tx)) */
    EMSAR_HIP_ERR_NO_DEVICE = -2,  /* no HIP device, or device_id out of range */
    EMSAR_HIP_ERR_OOM = -3,        /* host or device allocation failed */
    EMSAR_HIP_ERR_HIP = -4,        /* a HIP runtime call or kernel failed (see emsar_hip_last_error) */
    EMSAR_HIP_ERR_STATE = -5,      /* call order: upload_structure -> upload_sample -> solve */
    EMSAR_HIP_ERR_NUMERIC = -6     /* NaN/Inf met in theta (infeasible input such as R>0 on an all-zero row) */
} emsar_hip_status;

/* How the structure is laid out in HBM (DESIGN.md "Data layout"). */
typedef enum {
    EMSAR_LAYOUT_AUTO = 0,   /* TILED when it applies, else CSR */
    EMSAR_LAYOUT_CSR = 1,    /* rows as given; lane-per-row walk, FP64 atomics straight to HBM/L2 */
    /* 2 was the WINDOWED layout of round 1 (4x slower than TILED, removed) */
    EMSAR_LAYOUT_TILED = 3    /* units of <= 8 slices x 768 rows with a unit-local dictionary of <= 240 transcripts, kept in LDS as the 16
                                 subset sums of every block of 4 neighbouring slots; a stored operand is 10 bits (three to a dword)
                                 and names a block and a subset of it, so one LDS gather serves every transcript of the block that
                                 a row hits; forward index for the E-step and a per-slice transposed index for the M-step (no
                                 atomics in the inner loops); single-tid rows folded into a per-transcript count; rows longer than
                                 237 tids go to a small CSR of their own; transcripts numbered by co-occurrence inside when the
                                 caller's numbering packs poorly (ids at this ABI stay the caller's) */
} emsar_hip_layout;

/* OR-ed into the layout argument of emsar_hip_upload_structure (TILED only): store rows with the same tid multiset
 * once, weighted by the sum of their members' weights -- the read -> segment collapse the reference does while it
 * counts reads (update_ReadCounts, emsar_functions.c:838-943).  Exact up to summation order; per-row inputs of
 * upload_sample / ieuma keep referring to the caller's rows. */
#define EMSAR_LAYOUT_FLAG_MERGE_ROWS 0x100

/* Replaces the solver knobs -e/-r/-i/-l/-n of the reference (emsar_main.c:86-91): the pattern search's
 * step/F epsilons have no meaning for an EM; they map to tol / max_iter. */
typedef struct {
    int32_t max_iter;     /* cap on EM passes (one pass = one sweep over the matrix); <=0 -> 100000 */
    int32_t accel;        /* 0 plain EM; 1 SQUAREM (3 passes per cycle, likelihood-safeguarded) */
    double  tol;          /* stop when max_t |dtheta_t| / (theta_t + abs_floor) < tol; <=0 -> 1e-10 */
    double  abs_floor;    /* <=0 -> 1e-6, the %lf print quantum of the reference's .fpkm */
    int32_t check_every;  /* host looks at the device convergence word every this many cycles; <=0 -> 8 */
    int32_t set_mode;     /* 0 = split the problem into its connected sets (run_MLE_threads' unit of work, emsar_main.c:446-474):
                             sets that fit a CU's LDS are solved by one workgroup each with no kernel launch per pass,
                             one-transcript sets in closed form, only the rest by the streaming passes;
                             1 = streaming passes over the whole matrix only */
    double  count_floor;  /* optional second floor, in READS: the floor of transcript t becomes max(abs_floor, count_floor/den_t).
                             Transcripts whose optimum is the boundary theta = 0 with zero gradient decay like 1/k; a floor of
                             e.g. 1e-3 inferred reads stops the solve once only such components still move.  0 = off. */
    double  zero_cut;     /* > 0: a component that is below this value AND still decreasing no longer holds the solve up.  The
                             reference prints FPKM with "%lf" (emsar_functions.c:3207): anything below 5e-7 is written as
                             0.000000, so with zero_cut = 2.5e-7 the .fpkm file is the same while the 1/k decay of boundary
                             components (optimum theta = 0 with zero gradient) stops costing tens of thousands of passes.
                             <= 0 = off (every component must meet tol). */
    double  abs_step;     /* > 0: a component counts as converged, whatever its relative change, once its change in one plain
                             EM step (in FPKM) is below abs_step * 200000 / K at pass K (K >= 1000).  Nearly flat directions
                             converge sublinearly (|dtheta_k| ~ k^-p, p >= 2): what is left after stopping at |dtheta| < a in
                             pass K is at most ~a*K, so the rule bounds the remaining drift by abs_step * 2e5 at every K --
                             2e-8 FPKM, a fiftieth of the .fpkm print quantum, for 1e-13 -- while the relative rule at 1e-10
                             keeps such components going for 10^5 passes.  <= 0 = off. */
    /* (zero_cut and abs_step apply to the streaming passes, and to the resident sets only when newton_after < 0: a set that gets
       Newton steps reaches a boundary optimum in a few of them and is held to the strict rule) */
    int32_t newton_after; /* set_mode 0, resident sets: a set that has not converged after this many passes gets one safeguarded
                             projected-Newton step (direction by matrix-free conjugate gradients, accepted only if F does not
                             fall) after every SQUAREM cycle.  0 -> 60, < 0 = never (EM / SQUAREM only). */
    int32_t reserved0;
} emsar_em_params;

typedef struct {
    int32_t iters;            /* EM passes executed */
    int32_t converged;        /* 1 if tol was met */
    double  final_delta;      /* last max_t |dtheta|/(theta+abs_floor) */
    double  loglik;           /* F(theta) = sum_c R_c log(E_c S_c) - E_c S_c, rows with E_c != 0 (Fp, emsar_functions.c:2946) */
    double  solve_ms;         /* wall time of the solve, upload excluded */
    double  kernel_ms;        /* device time of all EM passes (HIP events on the context's stream) */
    int64_t bytes_per_pass;   /* algorithmic bytes of one pass, SURVEY.md 8d: 4 nnz + P (rows+1) + W rows + 32 T */
    int64_t stored_bytes_per_pass; /* bytes the chosen layout actually streams per pass */
    /* set_mode 0 only (else 0): how the transcripts were split and what the LDS-resident sets cost */
    int32_t sets_resident;    /* connected sets solved inside one workgroup's LDS */
    int32_t sets_streamed;    /* connected sets too large for that, solved by the streaming passes */
    int32_t set_passes_max;   /* EM passes of the slowest resident set (iters = streaming passes + this) */
    int32_t sets_unconverged; /* resident sets that hit max_iter */
    int64_t set_passes_sum;   /* EM passes summed over the resident sets */
    double  sets_build_ms;    /* host time spent finding and packing the sets (once per upload_sample) */
    double  sets_kernel_ms;   /* device time of the resident-set kernels (clusters included) */
    int32_t sets_cluster;     /* connected sets solved by a cluster of 2-8 workgroups inside one launch (too large for one workgroup's LDS) */
    int32_t cluster_passes_max; /* EM passes of the slowest of them (set_passes_max covers them too) */
    double  cluster_kernel_ms;  /* device time from the first to the last cluster launch */
} emsar_em_stats;

/* ---- lifetime ---------------------------------------------------------------------------------- */
int  emsar_hip_create(emsar_hip_ctx **out, int device_id);
void emsar_hip_destroy(emsar_hip_ctx *ctx);
const char *emsar_hip_strerror(int status);
const char *emsar_hip_last_error(const emsar_hip_ctx *ctx); /* text of the last HIP failure, "" if none */

/* ---- inputs ------------------------------------------------------------------------------------
 * upload_structure: the incidence CT (emsar.h:129, built by scan_rshbucket emsar_functions.c:2135-2192) as
 * CSR; called once per rsh.  The library validates 0 <= col_idx < n_tx and monotone row_ptr on the host
 * before anything reaches a kernel. */
int emsar_hip_upload_structure(emsar_hip_ctx *ctx, int64_t n_rows, int32_t n_tx,
                               const uint64_t *row_ptr /* n_rows+1 */, const int32_t *col_idx /* nnz */,
                               int layout /* emsar_hip_layout */);

/* upload_sample: per-sample vectors; called once per alignment file (the body of the loop emsar_main.c:380).
 *   row_weight = ReadCount[c] (emsar.h:142), NULL = every row counts 1 (read-level matrix)
 *   row_E      = EUMAps[c]   (construct_EUMAps, emsar_functions.c:3148-3154), NULL = 1.0 everywhere;
 *                rows with E == 0 are outside the likelihood (emsar_functions.c:2952)
 *   den        = optional precomputed sum_c m_ct E_c per transcript; NULL = computed on the device */
int emsar_hip_upload_sample(emsar_hip_ctx *ctx, const int32_t *row_weight, const double *row_E,
                            const double *den);

/* ---- the hot path: replaces run_MLE_threads() (emsar_main.c:446) --------------------------------
 * Starts from the uniform interior point (theta = 1 where den > 0, else 0), runs EM to tol and copies
 * theta (= FPKM[], emsar.h:160) to fpkm_out[n_tx].  stats may be NULL. */
int emsar_hip_solve(emsar_hip_ctx *ctx, const emsar_em_params *p, double *fpkm_out, emsar_em_stats *stats);

/* Lower-level stepping, used by bench.py and the parity tests:
 *   reset        theta <- uniform start
 *   set/get      move theta between host and device
 *   run_passes   n plain EM passes back to back on the context's stream, no host synchronisation inside;
 *                *elapsed_ms (may be NULL) = device time between HIP events recorded on that stream around
 *                the n passes, *last_loglik_terms (may be NULL) = sum_c R_c log S_c at the input of the last pass */
int emsar_hip_reset_theta(emsar_hip_ctx *ctx);
int emsar_hip_set_theta(emsar_hip_ctx *ctx, const double *theta /* n_tx */);
int emsar_hip_get_theta(emsar_hip_ctx *ctx, double *theta /* n_tx */);
int emsar_hip_run_passes(emsar_hip_ctx *ctx, int32_t n_passes, float *elapsed_ms, double *last_loglik_terms);

/* ---- post-processing: compute_iEUMA + print_FPKMfinal arithmetic --------------------------------
 * ieuma[t] = sum over ALL rows of m_ct * row_L[c]  (adjEUMA, emsar_functions.c:3224-3231). */
int emsar_hip_ieuma(emsar_hip_ctx *ctx, const double *row_L /* n_rows */, double *ieuma_out /* n_tx */);
/* From the mean FPKM: TPM = mean*1e6/sum(mean); iReadcount = ieuma/1e3 * mean * N/1e6  (emsar_functions.c:3203,3207). */
int emsar_hip_normalise(emsar_hip_ctx *ctx, const double *mean_fpkm, const double *ieuma, int64_t total_read_count,
                        double *tpm_out, double *ireadcount_out, int32_t *ireadcount_int_out);

/* ---- per-sample effective lengths: compute_adjEUMA (emsar_functions.c:2517-2523) ----------------
 * upload_euma: EUMA_c[i], the effective position counts per fragment length of every row (emsar.h:141, read from the rsh
 *   by construct_rsh_from_rshfile, emsar_functions.c:1351-1510), row-major [n_rows][nfl], 0 where a row has no entry;
 *   once per rsh, after upload_structure.  Stored transposed in HBM ([nfl][n_rows]) so that one lane owns one row.
 * adj_euma: L_c = sum_i Wf[i] * (double)EUMA_c[i], i ascending, multiply and add rounded separately -- the reference's
 *   loop, operation for operation, so L is bit-identical to the host's.  Wf = the sample's normalised fragment-length
 *   histogram (transfer_fraglendist_to_Wf, emsar_functions.c:2503-2513).  HBM-bound: 4 * n_rows * nfl bytes per call. */
int emsar_hip_upload_euma(emsar_hip_ctx *ctx, const int32_t *euma /* n_rows * nfl */, int32_t nfl);
int emsar_hip_adj_euma(emsar_hip_ctx *ctx, const double *wf /* nfl */, double *adj_euma_out /* n_rows */);

/* ---- read -> segment collapse: the integer core of update_ReadCounts (emsar_functions.c:838-943) ----------------
 * Rows with the same MULTISET of transcript ids (order inside a row does not matter, repeats do: SURVEY.md A2) become
 * one row whose weight is the sum of its members' weights (row_weight NULL = 1 each; rows with weight 0 and empty
 * rows vanish).  Output rows are numbered by first occurrence -- the order in which the reference meets the segments
 * -- with their ids sorted ascending.  Exact: hash matches are confirmed by comparing the rows themselves.
 * The caller provides the output arrays at worst-case size (row_ptr_out n_rows+1, col_idx_out nnz, weight_out n_rows,
 * row_map_out n_rows or NULL: original row -> output row, -1 for vanished rows).  Error if a sum exceeds INT32_MAX. */
typedef struct {
    double  kernel_ms;          /* device time of the collapse kernels (HIP events), transfers excluded */
    double  total_ms;           /* wall time of the call */
    int64_t n_rows, nnz, n_unique, nnz_unique;
    int64_t table_slots;        /* LDS table slots over all partitions (one workgroup each) of the largest round */
    int64_t algorithmic_bytes;  /* CSR read twice (hash, compare) + weights + the unique rows written */
    int64_t rounds;             /* 1 unless rows had to be hashed again (a 64-bit hash collision, a crowded partition table) */
} emsar_hip_collapse_stats;
int emsar_hip_collapse_rows(emsar_hip_ctx *ctx, int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                            const int32_t *row_weight, int64_t *n_unique_out, uint64_t *row_ptr_out, int32_t *col_idx_out,
                            int32_t *weight_out, int32_t *row_map_out, emsar_hip_collapse_stats *stats);

/* ---- deterministic mode ------------------------------------------------------------------------------------------
 * The streaming passes add with floating atomics, so two runs of the same solve agree to ~1e-9 relative, not bit for bit (the
 * per-set solver of set_mode 0 has no atomics and is reproducible either way).  With the mode on, every sum that workgroups share
 * is kept as a 64-bit integer in fixed point (integer adds commute): the M-step accumulators hold the reads assigned to a
 * transcript at a resolution of N * 2^-61 reads (N = the sample's total weight), the log-likelihood sums at N * 2^-51, the
 * SQUAREM norms are added up in a fixed order.  Two solves of the same input are then bit-identical, whatever the layout's
 * tile order.  Costs a few percent of a pass.  Default: off, or EMSAR_HIP_DETERMINISTIC=1 in the environment at create time. */
int emsar_hip_set_deterministic(emsar_hip_ctx *ctx, int on);

/* ---- Poisson bootstrap of the estimates -------------------------------------------------------------------------------
 * Replicate b re-draws every row c of the current sample: w_c ~ Poisson(R_c) (R_c = the uploaded weight, 0 for rows with E == 0; such
 * rows keep 0), E and den unchanged, and solves it to the MLE with the caller's parameters (set_mode as in solve).  The draws are
 * keyed by (seed, b) and by the caller's row index (Philox4x64-10, see DESIGN.md "Bootstrap"): they do not depend on the layout, the
 * set partition, the batch or the device.  Poisson(1) per read and Poisson(R) per segment have the same distribution, so read-level
 * and segment-level uploads give statistically equivalent bootstraps (not the same bits).
 *   bootstrap         replicates first_replicate .. first_replicate + n_replicates - 1: per transcript the mean and the sample sd (n - 1)
 *                     of theta (= FPKM) and the sd of TPM_b = theta_b * 1e6 / sum theta_b; replicates (may be NULL): [n_replicates][n_tx].
 *                     Reduced in replicate order: the results are the same whatever batch size the library picks.  The context is left
 *                     as it was (a following solve returns the same bits).  ERR_STATE before upload_sample, ERR_ARG for n_replicates < 1,
 *                     first_replicate < 0 or a replicate index past INT32_MAX, ERR_NUMERIC as solve.
 *   bootstrap_weights the drawn weights of one replicate, caller row order (computed on the device).
 *   bootstrap_draw_host  the same draws on the host, no HIP call (row_weight NULL = 1 per row). */
typedef struct {
    int32_t n_replicates, batch, replicates_unconverged, set_passes_max;
    int64_t draws;                                   /* rows with R > 0 x replicates */
    double  draw_ms, sets_ms, stream_ms, reduce_ms;  /* device time per stage (HIP events) */
    double  total_ms;                                /* wall time of the call */
} emsar_boot_stats;
int emsar_hip_bootstrap(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate,
                        int32_t n_replicates, double *fpkm_mean, double *fpkm_sd, double *tpm_sd,
                        double *replicates /* n_replicates * n_tx, or NULL */, emsar_boot_stats *stats);
int emsar_hip_bootstrap_weights(emsar_hip_ctx *ctx, uint64_t seed, int32_t replicate, int32_t *w_out /* n_rows */);

/* ---- gene-level sums (the reference's util/FPKM2gFPKM.pl, on the device) -----------------------------------------------------
 *   set_gene_map      gene_of_tx[t] = gene of caller transcript t in 0 .. n_genes-1, -1 = in no gene.  After upload_structure
 *                     (ERR_STATE before); a later upload_structure drops the map.  ERR_ARG for n_genes < 1 or an id < -1 or >= n_genes.
 *   gene_sums         gene_out[c][g] = sum of tx_values[c][t] over the transcripts t of gene g (0 for a gene without any), for
 *                     n_cols >= 1 columns of n_tx values in caller order.  ERR_STATE without a map.
 *   bootstrap_genes   emsar_hip_bootstrap (same arguments, same transcript outputs bit for bit) plus, per gene, the mean and the
 *                     sample sd (n - 1) over the replicates of G_b,g = the gene sum of theta_b, and the sd of the gene TPM
 *                     G_b,g * 1e6 / S_b (S_b = sum_t theta_b,t; 0 when S_b = 0), reduced in replicate order like the transcripts.
 *                     Its sd includes the covariance of a gene's isoforms, which sqrt(sum_t sd_t^2) leaves out.  Their device time is
 *                     part of emsar_boot_stats.reduce_ms.  ERR_STATE without a map.
 * Summation order (fixed, so that results are bit for bit the same across layouts, renumbering, batch sizes and devices): a gene's
 * transcripts in ascending caller tid are cut into consecutive chunks of 256; each chunk is added left to right starting from its
 * first value, then the chunk sums left to right starting from the first.  A gene of up to 256 transcripts gets the plain sequential
 * sum; a one-transcript gene gets that transcript's value. */
int emsar_hip_set_gene_map(emsar_hip_ctx *ctx, int32_t n_genes, const int32_t *gene_of_tx /* n_tx, caller numbering, -1 = no gene */);
int emsar_hip_gene_sums(emsar_hip_ctx *ctx, int32_t n_cols, const double *tx_values /* n_cols * n_tx */, double *gene_out /* n_cols * n_genes */);
int emsar_hip_bootstrap_genes(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                              double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates /* or NULL */,
                              double *gene_fpkm_mean, double *gene_fpkm_sd, double *gene_tpm_sd /* n_genes each */, emsar_boot_stats *stats);
int emsar_hip_bootstrap_draw_host(uint64_t seed, int32_t replicate, int64_t n_rows, const int32_t *row_weight /* NULL = 1 */,
                                  int32_t *w_out);

/* ---- bootstrap quantiles: percentile intervals and medians over the replicates ---------------------------------------------------
 * Definition (fixed, so that host and device agree bit for bit): for the order statistics x_(0) <= ... <= x_(B-1) of one transcript's
 * (or gene's) B replicate values and a probability q in [0, 1],
 *     h = q * (double)(B - 1),  i = (int64)floor(h),  g = h - (double)i,
 *     result = x_(i) when g == 0 or i == B - 1, else x_(i) + g * (x_(i+1) - x_(i)),
 * subtract, multiply and add rounded separately (no fused multiply-add) -- numpy's default "linear" method up to rounding.  Sorting
 * does not round, so the result does not depend on the batch size, the layout, the numbering or the device; q = 0 is the minimum,
 * q = 1 the maximum, q = 0.5 with odd B the middle value, and B = 1 gives the single value for every q.
 *   bootstrap_quantiles  emsar_hip_bootstrap / emsar_hip_bootstrap_genes (same arguments, the same mean, sd and replicates bit for bit)
 *                        that also keeps every replicate on the device -- theta_b, S_b = sum_t theta_b,t and, with gene outputs, the
 *                        gene sums G_b -- and returns per transcript the q-quantiles of FPKM (theta_b) and of TPM_b = S_b > 0 ?
 *                        theta_b * 1e6 / S_b : 0, [n_q][n_tx] each in the order of q, per gene those of G_b and of the gene TPM,
 *                        [n_q][n_genes].  S_b of the quantiles is added up in the caller's transcript order (same reduction tree as the sd's
 *                        S_b, which is added in the library's order: the two are the same bits unless the library numbered the
 *                        transcripts itself), so no quantile depends on the library's numbering.  replicate_sums (may be NULL): that
 *                        S_b, n_replicates values.  Gene outputs: all five NULL, or
 *                        all five given after set_gene_map.
 *                        Limits: 1 <= n_replicates <= 4096 (a column is sorted in a workgroup's LDS: 32 KiB of doubles), ERR_ARG
 *                        above; the held replicates, 8 * n_replicates * (n_tx + 1 + n_genes) bytes (held_bytes), plus the quantile stage's
 *                        own buffers (16 * n_q * (n_tx + n_genes) bytes and a few vectors) must fit half of the free device memory and
 *                        are allocated first, else ERR_OOM before any replicate is drawn.
 *                        ERR_ARG for n_q < 1, a q that is not finite or outside [0, 1], a gene output group only partly given, and
 *                        as bootstrap; ERR_STATE before upload_sample and for gene outputs without a map; ERR_NUMERIC as solve.  The
 *                        context is left as it was.  quantile_ms: device time of the quantile stage (HIP events).
 *   quantiles_host       the same definition on the host, no HIP call: values [n_rep][n] -> out [n_q][n].  ERR_ARG for n_rep < 1,
 *                        n_q < 1 or a q that is not finite or outside [0, 1]. */
typedef struct { int32_t n_quantiles, reserved0; int64_t held_bytes; double quantile_ms; } emsar_quantile_stats;
int emsar_hip_bootstrap_quantiles(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                                  int32_t n_q, const double *q,
                                  double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates /* or NULL */,
                                  double *replicate_sums /* n_replicates, or NULL: S_b as used for TPM */,
                                  double *fpkm_q, double *tpm_q /* [n_q][n_tx] */,
                                  double *gene_fpkm_mean, double *gene_fpkm_sd, double *gene_tpm_sd,
                                  double *gene_fpkm_q, double *gene_tpm_q /* all five NULL, or all five given after set_gene_map */,
                                  emsar_boot_stats *stats, emsar_quantile_stats *qstats);
int emsar_hip_quantiles_host(int32_t n_rep, int64_t n, const double *values /* [n_rep][n] */,
                             int32_t n_q, const double *q, double *out /* [n_q][n] */);

/* ---- isoform usage: each transcript's share of its gene, the dominant isoform, and their bootstrap -------------------------------
 * Definitions (fixed, so that host and device agree bit for bit), for one column x[0 .. n_tx) of non-negative transcript values in
 * caller numbering and the gene map of set_gene_map:
 *     G_g     the gene sum of x in the order documented for gene_sums (chunks of 256 by ascending caller tid, left to right);
 *     usage   u_t = G_g(t) > 0 ? x_t / G_g(t) : 0.0, one IEEE division; 0.0 for a transcript in no gene.  0 <= u_t <= 1 holds exactly
 *             (a rounded sum of non-negative addends is never below an addend), and a gene's only transcript with x_t > 0 has
 *             u_t == 1.0.  Usage is the same for FPKM and TPM -- the replicate's scale cancels -- so it is defined on theta and
 *             reported once;
 *     dominant  dom_g = the transcript of gene g with the largest x_t, the smallest caller tid among equal maxima; -1 when G_g == 0
 *             (a gene without transcripts included).  Values are compared, not usages, so nothing is rounded.
 * Over B bootstrap replicates, per transcript and reduced in replicate order (the results do not depend on the batch size, the layout
 * or the library's own transcript numbering): usage_mean / usage_sd = the Welford recurrence of bootstrap's mean and sd on u_b,t
 * (sample sd with n - 1, 0 for B = 1; subtract, divide, multiply and add rounded separately); dominant_count[t] = the number of
 * replicates b with dom_b,g(t) == t; with n_q > 0, usage_q[k][t] = the q[k]-quantile of u_.,t by the definition of bootstrap_quantiles.
 *   isoform_usage        n_cols >= 1 columns of n_tx values in caller order -> usage_out [n_cols][n_tx] and, unless NULL, dominant_out
 *                        [n_cols][n_genes] (caller tid or -1).  ERR_STATE without a map; ERR_ARG for n_cols < 1, a NULL tx_values or
 *                        usage_out, and for a negative or non-finite value (checked on the host before anything is uploaded).
 *   isoform_usage_host   the same definition on the host, no HIP call, no context; the same checks plus those of set_gene_map
 *                        (n_genes < 1, an id < -1 or >= n_genes: ERR_ARG).
 *   bootstrap_isoforms   bootstrap_quantiles' arguments and outputs (the same bits; with gene outputs the same bits as bootstrap_genes
 *                        too) plus the isoform statistics, so that one run of the replicates feeds every file of emsar-hip.  n_q == 0:
 *                        q, the quantile outputs and qstats may be NULL, nothing is held on the device and n_replicates is not limited
 *                        to 4096; the gene outputs are then the three statistics, all NULL or all given.  n_q > 0: the limits of
 *                        bootstrap_quantiles apply, the held replicates always include the gene sums (held_bytes = 8 * n_replicates *
 *                        (n_tx + 1 + n_genes)), and a call with usage_q adds 8 * n_q * n_tx bytes for it to what must fit half of
 *                        the free device memory.  The replicates' gene sums are computed whether or not gene outputs are asked for.
 *                        ERR_NUMERIC is decided on theta, as in bootstrap: a gene sum of finite values that itself overflows to +inf
 *                        is not an error -- every isoform of that gene then has usage 0 in that replicate (x / inf) and the
 *                        largest value is still its dominant isoform; gene outputs, when asked for, report it as bootstrap_genes does.
 *                        ERR_STATE without a gene map or before upload_sample; ERR_ARG for iso == NULL, n_q < 0, usage_q given with
 *                        n_q == 0, and for everything bootstrap_quantiles rejects; ERR_NUMERIC as solve.  The context is left as it was.
 *                        The device time of the usage and dominance kernels is part of reduce_ms, that of the usage quantiles of
 *                        quantile_ms. */
typedef struct {
    double  *usage_mean, *usage_sd;  /* [n_tx], may each be NULL */
    int32_t *dominant_count;         /* [n_tx], may be NULL */
    double  *usage_q;                /* [n_q][n_tx]; NULL iff not wanted; needs n_q > 0 */
} emsar_isoform_outputs;
int emsar_hip_isoform_usage(emsar_hip_ctx *ctx, int32_t n_cols, const double *tx_values /* n_cols * n_tx */,
                            double *usage_out /* n_cols * n_tx */, int32_t *dominant_out /* n_cols * n_genes, or NULL */);
int emsar_hip_isoform_usage_host(int32_t n_tx, int32_t n_genes, const int32_t *gene_of_tx /* n_tx, -1 = no gene */, int32_t n_cols,
                                 const double *tx_values, double *usage_out, int32_t *dominant_out /* or NULL */);
int emsar_hip_bootstrap_isoforms(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed, int32_t first_replicate, int32_t n_replicates,
                                 int32_t n_q, const double *q,
                                 double *fpkm_mean, double *fpkm_sd, double *tpm_sd, double *replicates /* or NULL */,
                                 double *replicate_sums /* or NULL */, double *fpkm_q, double *tpm_q,
                                 double *gene_fpkm_mean, double *gene_fpkm_sd, double *gene_tpm_sd,
                                 double *gene_fpkm_q, double *gene_tpm_q,
                                 emsar_boot_stats *stats, emsar_quantile_stats *qstats, const emsar_isoform_outputs *iso);

/* ---- binomial depth subsampling: the estimates at a fraction of the reads ---------------------------------------------------
 * "Did we sequence deep enough": keeping every read of the sample with probability f, independently (what samtools view -s does),
 * gives row c the weight w_c ~ Binomial(R_c, f) (a read-level row has R = 1, a segment the sum of its reads: the same law).  For
 * each fraction f_k in the caller's order, replicates b = 0 .. n_replicates-1 are drawn and solved exactly like bootstrap replicates
 * (same kernels, set_mode 0 and 1, E and den unchanged, the context left as it was, ERR_NUMERIC as solve).
 * Keying: Philox4x64-10 with key (seed, b) and counter (row, j, 1, bits of the double f_k), see DESIGN.md "Subsampling".  A draw is a
 * pure function of (seed, b, row, R_c, f_k): it does not depend on where f_k stands in the list, on the layout, the set partition, the
 * batch or the device, and it is independent of the bootstrap's draws (counter (row, j, 0, 0)) under the same seed.  f = 1 gives w = R.
 * Normalisation: E_c carries the full sample's read total N, so the raw MLE of a thinned replicate is about f times the FPKM.  The
 * fixed point is linear in that scale: the FPKM of replicate b at its own depth is theta_b * N_R / N_b with N_b = sum_c w_c and
 * N_R = sum_c R_c over the rows that are drawn (E != 0); 0 when N_b = 0.  TPM_b = theta_b * 1e6 / sum theta_b does not depend on it.
 *   subsample            per fraction and transcript the mean and the sample sd (n - 1) over the replicates of the normalised FPKM and
 *                        of TPM_b, reduced in replicate order (the same results for any batch size); depth_mean[k] = mean of N_b.
 *                        Gene outputs (all three NULL, or all three given after set_gene_map: ERR_STATE without a map): mean / sd of
 *                        the gene sums of the normalised FPKM (the order of gene_sums), mean of the gene TPM.  replicates (may be
 *                        NULL): [n_fractions][n_replicates][n_tx], the normalised FPKM.  ERR_STATE before upload_sample; ERR_ARG for
 *                        n_fractions < 1, n_replicates < 1, a fraction that is not finite or not in (0, 1].
 *   subsample_weights    the drawn weights of one replicate at one fraction, caller row order (computed on the device).
 *   subsample_draw_host  the same draws on the host, no HIP call (row_weight NULL = 1 per row). */
typedef struct {
    int32_t n_fractions, n_replicates, batch, replicates_unconverged;
    int64_t draws;                                   /* rows with R > 0 x replicates x fractions */
    double  draw_ms, sets_ms, stream_ms, reduce_ms;  /* device time per stage, summed over the fractions */
    double  total_ms;                                /* wall time of the call */
} emsar_subsample_stats;
int emsar_hip_subsample(emsar_hip_ctx *ctx, const emsar_em_params *p, uint64_t seed,
                        int32_t n_fractions, const double *fractions, int32_t n_replicates,
                        double *fpkm_mean, double *fpkm_sd, double *tpm_mean, double *tpm_sd /* [n_fractions][n_tx] each */,
                        double *depth_mean /* n_fractions */, double *replicates /* or NULL */,
                        double *gene_fpkm_mean, double *gene_fpkm_sd, double *gene_tpm_mean /* [n_fractions][n_genes] or NULL */,
                        emsar_subsample_stats *stats);
int emsar_hip_subsample_weights(emsar_hip_ctx *ctx, uint64_t seed, int32_t replicate, double fraction, int32_t *w_out /* n_rows */);
int emsar_hip_subsample_draw_host(uint64_t seed, int32_t replicate, double fraction, int64_t n_rows,
                                  const int32_t *row_weight /* NULL = 1 */, int32_t *w_out);

/* ---- model fit: does the fitted model explain the reads? ------------------------------------------------------------------------
 * Per-row residuals of one column theta against the sample, and a per-transcript and per-gene digest of them with a pointer to the
 * worst row.  Everything is in caller numbering and caller row order, so no result depends on the layout, on merged rows, on the
 * library's own transcript numbering or on the device.
 * Inputs: the structure of upload_structure; R_c = the row weights of upload_sample (0 where E was 0 at that call); row_E of THIS call
 * (NULL = 1.0; finite and >= 0); theta[n_tx] (finite and >= 0; both checked on the host before anything is uploaded).
 * Per row c.  A row is OUTSIDE if it is empty or row_E[c] == 0: all its outputs are 0.  For the others
 *     S_c  = sum of theta[col] over the row's entries, left to right (a repeated tid counts twice),   mu_c = row_E[c] * S_c,
 *   mu_c > 0:            q_c = (R - mu) * (R - mu) / mu     the Pearson term
 *                        a_c = |R - mu|                     the miss in reads
 *                        d_c = max(0, 2 * ((R > 0 ? R * log(R / mu) : 0) - (R - mu)))     the Poisson deviance term
 *   mu_c == 0, R_c == 0: all outputs 0
 *   mu_c == 0, R_c > 0:  the likelihood is -inf there: q_c = d_c = +inf, a_c = R; the row is INFEASIBLE, counted in rows_infeasible
 *                        and reaches no transcript (every share in it is 0).
 * No fused multiply-add: every output except d is a pure function of IEEE +, -, *, / and the same bits on host and device; d goes
 * through log (libm on the host, the device's log, both within 1 ulp).
 * Per entry k = (c, t): the share p_k = theta_t / S_c, one division, for a row that is inside with mu_c > 0; other entries add nothing.
 * Per transcript t: its entries ordered by (caller row ascending, position in the row ascending) are summed by the rule of gene_sums --
 * consecutive chunks of 256, each added left to right from its first term, then the chunk sums left to right:
 *     tx_chi2 = sum p_k q_c      tx_dev = sum p_k d_c      tx_miss = sum p_k a_c
 *     tx_df   = sum p_k          the effective number of segments attributed to t
 *     tx_worst_row = the caller row of the entry with the largest p_k * a_c, the smallest row among equal maxima, -1 when no entry
 *                    has p_k * a_c > 0.  Products are compared, so nothing is rounded twice.
 * Per gene (after set_gene_map): the gene sums of the four tx columns, in gene_sums' own order.  All four NULL, or all four given.
 *   model_fit       ERR_STATE before upload_sample and for gene outputs without a map; ERR_ARG for a NULL theta, a negative or
 *                   non-finite theta or E, a gene output group only partly given, and n_rows > INT32_MAX (the index holds int32 row
 *                   ids); ERR_OOM if the index does not fit.  out may be NULL (statistics only).  The first call after
 *                   upload_structure builds the transposed index (DESIGN.md "Model fit") and keeps it, with the caller-order CSR
 *                   and 32 bytes per row, until the next upload_structure.  The context is left as it was: a following solve
 *                   returns the same bits.
 *   model_fit_host  the same definition with no HIP call and no context: the CSR, the weights (NULL = 1 per row; negative: ERR_ARG),
 *                   E, theta and the gene map (gene_of_tx NULL = none: gene outputs then give ERR_STATE; else the checks of
 *                   set_gene_map) are given directly.  kernel_ms and the stage times stay 0.
 * The three totals are added over the rows that are not infeasible in a fixed order (one workgroup: lane l of 1024 takes the rows l,
 * l + 1024, .. in order, a wave is folded by a butterfly, the 16 wave sums left to right); the host function restates that order. */
typedef struct {
    double  *row_mu, *row_chi2, *row_dev;               /* [n_rows] mu_c, q_c, d_c; may each be NULL */
    double  *tx_chi2, *tx_dev, *tx_miss, *tx_df;        /* [n_tx]; may each be NULL */
    int32_t *tx_worst_row;                              /* [n_tx]; may be NULL */
    double  *gene_chi2, *gene_dev, *gene_miss, *gene_df; /* [n_genes]; all four NULL, or all four given after set_gene_map */
} emsar_fit_outputs;
typedef struct {
    double  kernel_ms;                       /* device time of all stages (HIP events) */
    double  total_ms;                        /* wall time of the call, the index build of a first call included */
    int64_t rows_inside, rows_infeasible;    /* rows that are not outside; of these, rows with mu == 0 and R > 0 */
    int64_t index_slots, index_bytes;        /* int32 row ids of the transposed index, padding included (<= nnz + 64 * 255); bytes of the index and its tables */
    double  sum_chi2, sum_dev, sum_miss;     /* sum_c q_c, d_c, a_c over the inside rows that are not infeasible */
    double  rows_ms, tx_ms, genes_ms, totals_ms;   /* device time per stage: rows, transcripts (both kernels), gene sums, totals */
} emsar_fit_stats;
int emsar_hip_model_fit(emsar_hip_ctx *ctx, const double *theta /* n_tx */, const double *row_E /* n_rows, or NULL */,
                        const emsar_fit_outputs *out /* or NULL */, emsar_fit_stats *stats /* or NULL */);
int emsar_hip_model_fit_host(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                             const int32_t *row_weight /* NULL = 1 */, const double *row_E /* or NULL */, const double *theta,
                             int32_t n_genes, const int32_t *gene_of_tx /* n_tx, or NULL = no gene map */,
                             const emsar_fit_outputs *out /* or NULL */, emsar_fit_stats *stats /* or NULL */);

/* ---- presence test: a likelihood-ratio test for each transcript ----------------------------------
 * Is transcript t needed to explain the reads of the current sample, or would the other transcripts of its connected set explain them
 * as well?  For the sample of upload_structure + upload_sample and solver parameters p, with s the packed connected set of t
 * (set_mode 0; the sets are found on first use, as by solve):
 *     F_s(theta) = sum_c R_c log S_c + sum_t u_t log theta_t - sum_t theta_t den_t     over the rows and transcripts of s, u_t = the
 *                  reads of the rows whose only transcript is t -- the sums the set solver's Newton step forms
 *     baseline     theta_hat = the set solver's result for s with p (the bits solve returns for these transcripts)
 *     drop-t       the same set with den_t taken as 0: theta_t is then 0 and t's entries add nothing to any S_c.  Same solver, same
 *                  start, same stopping rule; only t's own set changes when t is dropped, so one test is one workgroup's work
 *     Lambda_t     = 2 * (F_s(theta_hat) - F_s(theta_hat_without_t)); both F from the same epilogue of the same kernel.  A value below 0
 *                  (rounding, the stopping rule) is reported as 0; the most negative raw value goes into the statistics
 *     p_t          of the boundary mixture (1/2) chi2_0 + (1/2) chi2_1:  1 for Lambda <= 0,  0.5 * erfc(sqrt(Lambda / 2)) for
 *                  Lambda > 0,  0 for +inf,  NaN for NaN; computed on the host (presence_pvalue_host is the same function)
 *     heir_t       the transcript s != t of the set with the largest gain in expected reads (theta_without_t,s - theta_hat_s) * den_s,
 *                  the lowest position in the set among equal gains; heir_share_t = that gain / (theta_hat_t * den_t).  -1 / NaN
 *                  when no transcript gains.  It names the sibling t cannot be told apart from.
 * status, per transcript:
 *     TESTED        Lambda, p, heir as above
 *     ABSENT        theta_hat_t is exactly 0: Lambda = 0, p = 1, nothing is solved.  Also a one-transcript component without reads
 *     ESSENTIAL     without t some row with reads has no transcript left to explain it: u_t > 0 (decided before anything is launched;
 *                   a row {t,t} is such a row), or the drop solve's epilogue finds a row with R > 0 and S = 0 (its other
 *                   members all have den = 0).  Lambda = +inf, p = 0.  Also a one-transcript component with reads
 *     OUTSIDE       den_t = 0 (outside the likelihood).  Lambda, p, heir_share are NaN, heir -1, theta_hat 0
 *     NOT_RESIDENT  t lies in a streamed or a cluster set, one component holds most transcripts, or set_mode = 1: testing it would
 *                   cost one streaming solve of its set per transcript, which this call does not do.  All outputs NaN / -1
 *     UNCONVERGED   values are given, but the baseline or the drop solve hit max_iter
 * Outputs are indexed by query position (by tid when query_tids is NULL; n_query is then ignored); a tid may repeat and the order is
 * free: a transcript's result depends on its set, itself and p alone, not on what else is asked.  Any output pointer may be NULL, as
 * may out and stats.  ERR_STATE before upload_sample; ERR_ARG for a tid outside 0 .. n_tx-1, n_query < 0, and the parameters solve
 * rejects.  The context's theta, weights and scales are not touched: a following solve returns the same bits. */
enum {
    EMSAR_PRESENCE_TESTED = 0, EMSAR_PRESENCE_ABSENT = 1, EMSAR_PRESENCE_ESSENTIAL = 2, EMSAR_PRESENCE_OUTSIDE = 3,
    EMSAR_PRESENCE_NOT_RESIDENT = 4, EMSAR_PRESENCE_UNCONVERGED = 5
};
typedef struct {
    double  *lambda, *pvalue;     /* [n_query] */
    int32_t *heir;                /* [n_query] caller tid, -1 = none */
    double  *heir_share;          /* [n_query] */
    int32_t *status;              /* [n_query] EMSAR_PRESENCE_* */
    double  *theta_hat;           /* [n_query] the baseline: solve's value for a resident or closed-form transcript */
} emsar_presence_outputs;
typedef struct {
    int64_t n_status[6];          /* distinct queried transcripts per status */
    int64_t items_launched;       /* set solves: baselines and drops */
    int64_t drop_passes_sum;      /* passes summed over the drop solves */
    int32_t drop_passes_max;      /* passes of the slowest drop solve */
    int32_t reserved0;
    double  min_raw_lambda;       /* the most negative Lambda before clamping, 0 if none was negative */
    double  baseline_ms, drop_ms; /* device time of the two phases (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_presence_stats;
int emsar_hip_presence(emsar_hip_ctx *ctx, const emsar_em_params *p, int32_t n_query, const int32_t *query_tids /* NULL = all transcripts */,
                       const emsar_presence_outputs *out /* or NULL */, emsar_presence_stats *stats /* or NULL */);
int emsar_hip_presence_pvalue_host(int64_t n, const double *lambda, double *p_out);

/* ---- profile-likelihood intervals: limits that hold at the boundary --------------------------------
 * How much of transcript t could be present without the reads contradicting it -- also where theta_hat_t is 0 or close to it, where the
 * asymptotic standard errors do not hold and the bootstrap's percentile interval is [0, 0].  For the sample of upload_structure +
 * upload_sample and solver parameters p, with s the packed connected set of t (set_mode 0) and F_s as the presence test defines it:
 *     D_t(x)       = 2 * (F_s(theta_hat) - max{ F_s(theta) : theta_t = x }) for x >= 0, the deviance of the value x.  D_t(theta_hat_t) = 0;
 *                  F is concave, so D_t does not rise towards theta_hat_t from either side; D_t(0) is the presence test's Lambda_t
 *     cut          q with erf(sqrt(q / 2)) = level, the `level` quantile of chi2 with 1 degree of freedom (profile_cut_host: bisection on
 *                  std::erf until the bracket cannot be halved, no HIP call; 0.95 -> 3.841458820694124; ERR_ARG unless 0 < level < 1)
 *     lower, upper = inf / sup {x >= 0 : D_t(x) <= q}.  upper always exists (F -> -inf as theta_t -> inf)
 *     path         the maximiser of F(theta) - lambda * theta_t is the same set problem with den_t replaced by m * den_t
 *                  (lambda = (m - 1) den_t), and it is the constrained maximum of F at x = theta_t(m): m = 1 is the MLE, m -> inf the
 *                  presence test's drop solve, 0 < m < 1 the upper side.  Every point of the path is one solve of the set with
 *                  m * den_t in LDS -- same solver, same start, same stopping rule as solve; its F is summed with the ORIGINAL den_t
 *     search       a limit is a root search over log m on sqrt(D) - sqrt(q): from m0 = 1 + sqrt(q / n_t) (lower) or its reciprocal
 *                  (upper), n_t = theta_hat_t den_t, doubling log m until D >= q, then Illinois steps with a bisection safeguard;
 *                  on the upper side with n_t < q (theta_hat_t = 0 included) from m = 1/2, quartering.  It stops when |D - q| <= dev_tol * q (dev_tol <= 0: 1e-4) or after
 *                  max_evals solves (<= 0: 40; then UNCONVERGED).  The reported limit is the x = theta_t(m) of the search's last
 *                  solve and dev_lower / dev_upper that solve's deviance: each pair lies on the profile curve.  One workgroup
 *                  runs one search, at most max_evals * max_iter passes
 *     lambda       the presence test's value for t, computed by the same drop solve: its bits; +inf for an essential, 0 for an absent t
 *     closed form  a one-transcript component has F(x) = u log x - x den: the same search on the host; u = 0 gives lower = 0,
 *                  upper = q / (2 den) with no search
 * status, per transcript:
 *     TWO_SIDED     both limits were found by search, lower > 0
 *     LOWER_ZERO    Lambda_t <= q (theta_hat_t == 0 included): lower = 0.0 exactly and dev_lower = Lambda_t -- at this level t cannot be
 *                   told from absent; upper is found by search
 *     OUTSIDE, NOT_RESIDENT   as in the presence test; every output NaN (evals 0)
 *     UNCONVERGED   values are given, but the baseline, the drop solve, a solve of a search or a search itself hit its cap
 * Outputs are indexed by query position (by tid when query_tids is NULL; n_query is then ignored); repeats and any order are allowed.  A
 * transcript's result depends on its set, itself, p and the profile parameters alone -- not on what else is asked, the batch, the
 * layout or the library's numbering.  The context's theta, weights and scales are not touched: a following solve or presence returns
 * the same bits.  ERR_STATE before upload_sample; ERR_ARG for a tid outside 0 .. n_tx-1, n_query < 0, a level outside (0, 1), a
 * non-finite dev_tol and the parameters solve rejects; ERR_NUMERIC for a non-finite baseline F.  EMSAR_HIP_PROFILE_BATCH = items per
 * launch and class (a testing aid; the bits do not change). */
enum {
    EMSAR_PROFILE_TWO_SIDED = 0, EMSAR_PROFILE_LOWER_ZERO = 1, EMSAR_PROFILE_OUTSIDE = 2, EMSAR_PROFILE_NOT_RESIDENT = 3,
    EMSAR_PROFILE_UNCONVERGED = 4
};
typedef struct { double level, dev_tol; int32_t max_evals, max_outer; } emsar_profile_params;      /* NULL: 0.95 and the defaults; max_outer: read by emsar_hip_profile_usage alone, ignored by emsar_hip_profile and _profile_genes */
typedef struct {
    double  *lower, *upper, *dev_lower, *dev_upper, *lambda, *theta_hat;    /* [n_query]; may each be NULL */
    int32_t *status, *evals;                                                /* [n_query] EMSAR_PROFILE_*; solves spent on the two searches */
} emsar_profile_outputs;
typedef struct {
    int64_t n_status[5];          /* distinct queried transcripts per status */
    int64_t items_launched;       /* workgroups: baselines, drops and searches */
    int64_t evals_sum;            /* solves summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over those solves */
    int32_t evals_max, passes_max; /* the search with the most solves / the most passes */
    double  cut;                  /* q */
    double  baseline_ms, drop_ms, search_ms; /* device time of the three phases (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_profile_stats;
int emsar_hip_profile(emsar_hip_ctx *ctx, const emsar_em_params *p, const emsar_profile_params *pp /* or NULL */, int32_t n_query,
                      const int32_t *query_tids /* NULL = all transcripts */, const emsar_profile_outputs *out /* or NULL */,
                      emsar_profile_stats *stats /* or NULL */);
int emsar_hip_profile_cut_host(double level, double *cut_out);

/* ---- two-sample test: does a transcript's abundance differ between two samples? -------------------
 * Two contexts on the same device hold the same structure (n_rows, n_tx, nnz, row_ptr and col_idx equal; compared on the host copies the
 * contexts keep, nothing is uploaded for the check) and each its own sample: A in ctx_a, B in ctx_b.  For transcript t, solver
 * parameters p and ratio r (0 means 1), with s_A / s_B the packed connected sets of t in A / B (set_mode 0) -- they may differ and lie
 * in different size classes, because sets depend on which rows carry reads -- and F_s as the presence test defines it:
 *     H1           theta^A, theta^B free:                     F1 = F_sA(theta_hat^A) + F_sB(theta_hat^B)
 *     H0           theta_t^A = r * theta_t^B, all else free:  F0 = the maximum of F_sA + F_sB under that constraint
 *     Lambda_t     = 2 (F1 - F0) >= 0,  p_t = erfc(sqrt(Lambda_t / 2)), chi2 with 1 degree of freedom.  The siblings of t stay free in
 *                  both samples, so reads that merely move to a sibling do not count as a difference.  THE P-VALUE IS CONSERVATIVE WHEN
 *                  ONE ESTIMATE SITS ON THE BOUNDARY (theta_hat_t = 0 in one sample): the statistic is then stochastically smaller
 *                  than chi2_1.  E carries each sample's read total, so theta is depth-normalised; r != 1 tests against a fold change
 *                  or applies a size factor.
 *     path         for a multiplier lambda the dual L(lambda) = max [F_sA - lambda theta_t^A] + max [F_sB + r lambda theta_t^B] is two
 *                  independent set problems: den_tA replaced by den_tA + lambda (scale_A = 1 + lambda / den_tA), den_tB by
 *                  den_tB - r lambda (scale_B = 1 - r lambda / den_tB), lambda in (-den_tA, den_tB / r).  Each is one solve of the set
 *                  with the scaled den_t in LDS -- same solver, same start, same stopping rule as solve, F summed with the ORIGINAL
 *                  den_t, as the profile intervals do.  With x_A, x_B the two values of t: g(lambda) = x_A - r x_B falls in lambda and has
 *                  one root lambda*; L(lambda) = F_A + F_B - lambda g(lambda) >= F0 for every lambda, with equality at lambda*.
 *     search       one workgroup runs it.  Evaluation 0 is lambda = 0 and gives theta_hat_tA, theta_hat_tB and F1 from the code path of
 *                  every later evaluation; g(0) == 0 exactly ends it with Lambda = 0.0, evals = 1.  Otherwise the root lies on the side
 *                  of sign g(0): lambda = v * lambda_end, v in [0, 1), lambda_end = den_tB / r or -den_tA; Illinois steps with a
 *                  midpoint safeguard on h = (x_A - r x_B) / (x_A + r x_B), h(1) = -+1 known without a solve.  It stops when
 *                  2 |lambda g(lambda)| <= dev_tol (<= 0: 1e-4, absolute, on the chi-square scale), or when
 *                  2 |g(lambda)| * (the width of the bracket in lambda) <= dev_tol -- L is convex with slope -g and the root lies in
 *                  the bracket, so the dual value cannot fall further than that; this is the rule that ends a search whose root is the
 *                  end of the range itself (t has no read to its name in the sample that would have to grow: x stays 0 there) --, or
 *                  after max_evals evaluations (<= 0: 40; then UNCONVERGED); an evaluation is one solve per sample.
 *     lambda       the dual value max(0, 2 (F1 - L(lambda_last))): a lower bound of the statistic at every lambda, stationary at
 *                  lambda*, so its error is of second order in the gap; the stopping quantity is the distance between the primal and
 *                  the dual value.  raw_lambda is the value before clamping, gap = g(lambda_last), multiplier = lambda_last,
 *                  theta_null = the last x_A (the common value under H0, on A's scale)
 *     log2fc       log2(theta_hat_A / (r theta_hat_B)); +-inf when exactly one estimate is 0, NaN when both are
 *     closed form  a one-transcript component of either sample has x = u / den', F = u log x - x den (u = 0: x = 0); the kernel takes
 *                  it in place of a set.  When both samples' components are closed form the host runs the same search and nothing is
 *                  launched.
 * status, per transcript:
 *     TESTED        outputs as above
 *     BOTH_ABSENT   theta_hat_t is exactly 0 in both samples: Lambda 0, p 1, evals 1
 *     OUTSIDE       den_t == 0 in either sample.  Every numeric output NaN (evals 0)
 *     NOT_RESIDENT  t lies in a streamed or a cluster set in either sample, one component holds most transcripts, or set_mode = 1.
 *                   Every numeric output NaN (evals 0)
 *     UNCONVERGED   values are given, but a solve hit max_iter or the search hit max_evals
 * Outputs are indexed by query position (by tid when query_tids is NULL; n_query is then ignored); repeats and any order are allowed.  A
 * transcript's result depends on its two sets, itself, p and cp alone -- not on what else is asked, the batch, the layout, MERGE_ROWS
 * or the library's numbering.  Both contexts are left as they were: a following solve, presence or profile on either returns the same
 * bits.  ERR_STATE when either context is before upload_sample; ERR_ARG for a NULL context, the same context twice, different devices
 * or structures, a tid outside 0 .. n_tx-1, n_query < 0, a ratio or dev_tol that is not finite, a negative ratio and the parameters
 * solve rejects; ERR_NUMERIC for a non-finite F at lambda = 0.  EMSAR_HIP_COMPARE_BATCH = items per launch and class (a testing aid;
 * the bits do not change).  compare_pvalue_host: 1 for Lambda <= 0, erfc(sqrt(Lambda / 2)) above, 0 for +inf, NaN for NaN; no HIP call. */
enum {
    EMSAR_COMPARE_TESTED = 0, EMSAR_COMPARE_BOTH_ABSENT = 1, EMSAR_COMPARE_OUTSIDE = 2, EMSAR_COMPARE_NOT_RESIDENT = 3,
    EMSAR_COMPARE_UNCONVERGED = 4
};
typedef struct { double ratio, dev_tol; int32_t max_evals, reserved0; } emsar_compare_params;      /* NULL: ratio 1 and the defaults */
typedef struct {
    double  *lambda, *pvalue, *log2fc, *theta_a, *theta_b, *theta_null, *multiplier, *gap, *raw_lambda;    /* [n_query]; may each be NULL */
    int32_t *status, *evals;                                                /* [n_query] EMSAR_COMPARE_*; evaluations of the search */
} emsar_compare_outputs;
typedef struct {
    int64_t n_status[5];          /* distinct queried transcripts per status */
    int64_t items_launched;       /* workgroups: one search each */
    int64_t evals_sum;            /* evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over their solves, both samples */
    int32_t evals_max, passes_max; /* the search with the most evaluations / the most passes */
    double  min_raw_lambda;       /* the most negative Lambda before clamping, 0 if none was negative */
    double  device_ms;            /* device time of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_compare_stats;
int emsar_hip_compare(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_compare_params *cp /* or NULL */,
                      int32_t n_query, const int32_t *query_tids /* NULL = all transcripts */, const emsar_compare_outputs *out /* or NULL */,
                      emsar_compare_stats *stats /* or NULL */);
int emsar_hip_compare_pvalue_host(int64_t n, const double *lambda, double *p_out);

/* ---- gene-level two-sample test: does a gene's total abundance differ between two samples? --------
 * The per-transcript Lambdas above cannot be added up: a gene whose isoforms trade reads at an unchanged total gets several small
 * p-values, a gene whose total moved but whose isoforms are confounded with each other gets none.  Here the null is imposed on the gene
 * sum inside the likelihood, the isoforms staying free.  Contexts, structure check, p and cp (ratio r, dev_tol, max_evals) are those of
 * emsar_hip_compare; the gene map is the one set on ctx_a (emsar_hip_set_gene_map) -- a map on ctx_b must be the same map -- and each
 * context translates caller tids to its own library numbering.  For gene g:
 *     members      in one sample the members of g that TAKE PART are those with den_t > 0 there; a member with den_t == 0 is held at 0
 *                  in that sample.  They fall into PARTS: every packed connected set (set_mode 0) that holds at least one of them, and
 *                  every member that is a one-transcript component (closed form: x = u / den', F = u log x - x den).  X = the sum of
 *                  theta over the members, F = the sum of the parts' F (as the presence test defines it).
 *     H1           everything free in both samples:                       F1 = F^A + F^B at lambda = 0
 *     H0           X^A = r * X^B, all else (the isoforms too) free:        F0 = the maximum of F^A + F^B under that constraint
 *     Lambda_g     = 2 (F1 - F0) >= 0,  p_g = erfc(sqrt(Lambda_g / 2)), chi2 with 1 degree of freedom.  THE P-VALUE IS CONSERVATIVE WHEN
 *                  ONE GENE SUM SITS ON THE BOUNDARY (X = 0 in one sample): the statistic is then stochastically smaller than chi2_1.
 *     path         the dual L(lambda) = max [F^A - lambda X^A] + max [F^B + r lambda X^B] falls apart into the parts: den_t of EVERY
 *                  member becomes den_t + lambda in A and den_t - r lambda in B, lambda in (-min_A, min_B / r) with min_S the smallest
 *                  den_t of the members taking part in S (beyond it the dual is unbounded).  On the side that shrinks the member(s) at
 *                  the minimum take min_S * (1 - v), v in [0, 1) the point of the search, and the others den_t - v * min_S: both stay
 *                  positive in floating point.  Each set part is one solve with the shifted den in LDS -- same solver, start and
 *                  stopping rule as solve --, F summed with the ORIGINAL den.  g(lambda) = X^A - r X^B falls in lambda, L is convex
 *                  with slope -g.
 *     search       emsar_hip_compare's, unchanged, with den_tA := min_A, den_tB := min_B and the gene sums for the two values of t: one
 *                  workgroup runs it, an evaluation loops over the set parts of A, then of B (each side by the smallest caller tid of a
 *                  part's members), then the closed-form parts.  A gene whose parts are all closed form is searched on the host and
 *                  nothing is launched for it.
 *     outputs      lambda, raw_lambda, multiplier, gap as emsar_hip_compare defines them; gene_a, gene_b = X^A, X^B at lambda = 0;
 *                  gene_null = the last X^A; log2fc = log2(gene_a / (r gene_b)), +-inf when exactly one sum is 0, NaN when both are;
 *                  parts = the set and closed-form parts of both samples together
 * status, per gene (EMSAR_COMPARE_* and EMSAR_GENE_COMPARE_TOO_LARGE):
 *     TESTED        outputs as above
 *     BOTH_ABSENT   both gene sums at lambda = 0 are exactly 0: Lambda 0, p 1, evals 1
 *     OUTSIDE       in either sample no member has den > 0, or the gene has no transcript.  Every numeric output NaN (evals 0, parts 0)
 *     NOT_RESIDENT  a member taking part lies in a streamed or a cluster set in either sample, one component holds most transcripts,
 *                   or set_mode = 1.  Every numeric output NaN (evals 0, parts 0)
 *     TOO_LARGE     more than 64 parts in either sample: one workgroup's work is bounded by 2 * 64 * max_evals * max_iter passes.
 *                   Every numeric output NaN (evals 0, parts 0)
 *     UNCONVERGED   values are given, but a solve hit max_iter or the search hit max_evals
 * Outputs are indexed by query position (by gene id when query_genes is NULL; n_query is then ignored); repeats and any order are
 * allowed.  A gene's result depends on its parts, p and cp alone -- not on what else is asked, the batch, the layout, MERGE_ROWS or the
 * library's numbering.  Both contexts are left as they were: a following solve, presence, profile or compare on either returns the
 * same bits.  ERR_STATE when either context is before upload_sample or ctx_a has no gene map; ERR_ARG for what emsar_hip_compare
 * rejects, a different map on ctx_b and a gene id outside 0 .. n_genes-1; ERR_NUMERIC for a non-finite F at lambda = 0.
 * EMSAR_HIP_COMPARE_GENES_BATCH = items per launch and class (a testing aid; the bits do not change). */
enum { EMSAR_GENE_COMPARE_TOO_LARGE = 5 };                              /* the statuses above, and this one */
typedef struct {
    double  *lambda, *pvalue, *log2fc, *gene_a, *gene_b, *gene_null, *multiplier, *gap, *raw_lambda;       /* [n_query]; may each be NULL */
    int32_t *status, *evals, *parts;                                        /* [n_query] EMSAR_COMPARE_*; evaluations; parts of both samples */
} emsar_compare_gene_outputs;
typedef struct {
    int64_t n_status[6];          /* distinct queried genes per status */
    int64_t items_launched;       /* workgroups: one search each */
    int64_t evals_sum;            /* evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over their solves, every part of both samples */
    int32_t evals_max, passes_max; /* the search with the most evaluations / the most passes */
    int32_t parts_max, reserved0; /* the most parts of a gene that was searched */
    double  min_raw_lambda;       /* the most negative Lambda before clamping, 0 if none was negative */
    double  device_ms;            /* device time of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_compare_gene_stats;
int emsar_hip_compare_genes(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_compare_params *cp /* or NULL */,
                            int32_t n_query, const int32_t *query_genes /* NULL = all genes */, const emsar_compare_gene_outputs *out /* or NULL */,
                            emsar_compare_gene_stats *stats /* or NULL */);

/* ---- two-sample test of isoform usage: did a transcript's share of its gene change? ---------------
 * An isoform switch (differential transcript usage).  emsar_hip_compare lights up every transcript of a gene whose total doubled at
 * unchanged shares, emsar_hip_compare_genes does not see isoforms that swap at an unchanged total, and the bootstrap sd of the share
 * (emsar_hip_isoform_usage) is per sample and fails where the share is 0 or 1 -- which is where switches live.  Here the null is imposed
 * on the share inside the likelihood.  Contexts, structure check, p and the gene map rules are those of emsar_hip_compare_genes (the map
 * is the one on ctx_a; a map on ctx_b must be the same one); members, parts, X and F are defined as there.  For transcript t of gene g,
 * share = theta_t / X (FPKM is proportional to theta within a sample: this is the share emsar_hip_isoform_usage reports):
 *     H1           everything free in both samples:                        F1 = F^A + F^B at lambda = 0
 *     H0           theta_t^A / X^A = theta_t^B / X^B (= u, free):           F0 = max_u [P_A(u) + P_B(u)],
 *                  P_k(u) = max {F^k : theta_t = u X} in sample k
 *     Lambda       = 2 (F1 - F0) >= 0,  p = erfc(sqrt(Lambda / 2)), chi2 with 1 degree of freedom.  THE P-VALUE IS CONSERVATIVE WHEN A
 *                  SHARE SITS AT 0 OR 1 IN ONE SAMPLE.  No ratio parameter: the share is scale-free, the samples' depths drop out.
 *     inner level  u fixed: the samples decouple and theta_t - u X = 0 is linear.  Its Lagrangian is the ordinary problem with
 *                  den_t + lambda (1 - u) on t and den_s - lambda u on every other member s taking part, lambda in
 *                  (-den_t / (1 - u), mn / u), mn = the smallest den of the others (beyond it the dual is unbounded).  The gap
 *                  g(lambda) = theta_t - u X falls in lambda, the dual D(lambda) = F - lambda g is convex with slope -g and
 *                  D >= P_k(u), with equality at the root.  The search is emsar_hip_compare's on h = g / (theta_t + u X), in
 *                  v in [0, 1) with lambda = v * (the end of the range on the side of sign g(0)); g(0) comes from evaluation 0 and
 *                  costs no solve.  On the side that shrinks the member(s) at the limiting den take den * (1 - v), the others
 *                  den - v * (their share of the limit); at lambda = 0 every den keeps its own bits.  It stops when
 *                  2 |lambda g| <= dev_tol, when 2 |g| * (the width of the bracket in lambda) <= dev_tol, or after max_evals
 *                  evaluations.  Its value is D at the last lambda: an upper bound of P_k(u) whose error is of second order in g.
 *     outer level  P_k is quasi-concave in u with its maximum at the estimated share u_hat_k, so the maximum of P_A + P_B lies in
 *                  [min u_hat, max u_hat].  dP_k / du = lambda_k Xc^k (envelope theorem), where Xc is the gene sum of the point ON
 *                  the constraint: an inner search ends short of its root, so Xc is taken from the feasible point next to its last
 *                  evaluation -- (X - theta_t) / (1 - u) when t is the member in deficit (t filled up to the share u), theta_t / u when
 *                  the others are; both equal X at a root, and they differ from it where the root is the end of the multiplier's
 *                  range (the member in deficit has no read to its name and stays 0 at every evaluated point, while at the end its
 *                  value is free and the constraint sets it).  Illinois steps on s(u) = lambda_A Xc^A + lambda_B Xc^B, normalised by
 *                  |lambda_A Xc^A| + |lambda_B Xc^B|, over that bracket; the signs at
 *                  its ends are known without evaluation (at u = u_hat_k that sample's multiplier is 0).  Evaluation 0 is lambda = 0
 *                  in both samples and gives u_hat_A, u_hat_B and F1 from the code path of every later evaluation;
 *                  u_hat_A == u_hat_B ends the search with Lambda = 0.0 and outer_evals = 1.  It stops when
 *                  2 |s| * (the width of the bracket in u) <= dev_tol or after max_outer outer points, evaluation 0 counted (at least
 *                  one point of the null is evaluated whatever max_outer says).  F0 is the largest P_A + P_B among the points
 *                  evaluated.  BETWEEN THE TWO ESTIMATED SHARES THE SUM OF A RISING AND A FALLING QUASI-CONCAVE FUNCTION NEED NOT BE
 *                  CONCAVE: the search then finds a stationary point that need not be the maximum, which makes Lambda too large at
 *                  worst (anti-conservative).
 *     cost         one workgroup runs one (gene, t) search: at most max(max_outer, 2) * 2 * max_evals * parts * max_iter passes,
 *                  parts <= 64 per sample.  A gene whose parts are all closed form in both samples is searched on the host with the
 *                  same code and nothing is launched for it.
 *     outputs      lambda, raw_lambda (before clamping at 0), pvalue; usage_a, usage_b = the shares at lambda = 0; usage_null = u of the
 *                  best outer point; dlogit = logit(usage_a) - logit(usage_b), +-inf when exactly one share sits at an end or they sit
 *                  at opposite ends, NaN when both sit at the same end; slope = the outer stopping quantity of the last point;
 *                  outer_evals; evals = inner evaluations summed, evaluation 0's two included; parts = the parts of both samples
 * status, per queried transcript:
 *     TESTED        outputs as above
 *     BOTH_ABSENT   theta_t is exactly 0 in both samples at lambda = 0, both gene sums positive: Lambda 0, p 1
 *     UNDEFINED     a gene sum is exactly 0 at lambda = 0 in either sample: usage and Lambda NaN, the counters are given
 *     SINGLE        fewer than two members take part in either sample: the share is 1 by construction
 *     OUTSIDE       den_t == 0 in either sample, or t has no gene
 *     NOT_RESIDENT  as in emsar_hip_compare_genes
 *     TOO_LARGE     more than 64 parts in a sample
 *     UNCONVERGED   values are given, but a solve, an inner search or the outer search hit its cap
 *   For SINGLE, OUTSIDE, NOT_RESIDENT and TOO_LARGE every numeric output is NaN and the counters are 0.
 * Outputs are indexed by query position (by tid when query_tids is NULL; n_query is then ignored); repeats and any order are allowed.  A
 * result depends on the gene's parts, t, p and up alone -- not on what else is asked, the batch, the layout, MERGE_ROWS or the library's
 * numbering.  Both contexts are left as they were.  Errors as emsar_hip_compare_genes, with tids for gene ids; ERR_ARG for a non-finite
 * dev_tol.  EMSAR_HIP_COMPARE_USAGE_BATCH = items per launch and class (a testing aid; the bits do not change). */
enum {
    EMSAR_USAGE_TESTED = 0, EMSAR_USAGE_BOTH_ABSENT = 1, EMSAR_USAGE_OUTSIDE = 2, EMSAR_USAGE_NOT_RESIDENT = 3, EMSAR_USAGE_UNCONVERGED = 4,
    EMSAR_USAGE_TOO_LARGE = 5, EMSAR_USAGE_UNDEFINED = 6, EMSAR_USAGE_SINGLE = 7
};
typedef struct { double dev_tol; int32_t max_evals, max_outer; } emsar_usage_params;    /* NULL or <= 0: 1e-4 (both levels), 40, 12 */
typedef struct {
    double  *lambda, *raw_lambda, *pvalue, *usage_a, *usage_b, *usage_null, *dlogit, *slope;               /* [n_query]; may each be NULL */
    int32_t *status, *outer_evals, *evals, *parts;                          /* [n_query] EMSAR_USAGE_*; outer points; inner evaluations; parts */
} emsar_usage_outputs;
typedef struct {
    int64_t n_status[8];          /* distinct queried transcripts per status */
    int64_t items_launched;       /* workgroups: one search each */
    int64_t evals_sum;            /* inner evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over their solves, every part of both samples */
    int64_t outer_sum;            /* outer points summed over the searches on the device */
    int32_t evals_max, passes_max; /* the search with the most inner evaluations / the most passes */
    int32_t parts_max, outer_max; /* the most parts of a gene that was searched; the search with the most outer points */
    double  min_raw_lambda;       /* the most negative Lambda before clamping, 0 if none was negative */
    double  device_ms;            /* device time of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_usage_stats;
int emsar_hip_compare_usage(emsar_hip_ctx *ctx_a, emsar_hip_ctx *ctx_b, const emsar_em_params *p, const emsar_usage_params *up /* or NULL */,
                            int32_t n_query, const int32_t *query_tids /* NULL = all transcripts */, const emsar_usage_outputs *out /* or NULL */,
                            emsar_usage_stats *stats /* or NULL */);

/* ---- gene-level profile intervals and the gene presence test --------------------------------------
 * How much of gene g could be there, and is g needed to explain the reads at all?  Also where the gene sum is 0 or close to it, where
 * the asymptotic errors do not hold and the bootstrap's percentile interval is [0, 0].  The per-transcript profile limits cannot be
 * added up -- isoforms that are confounded with each other each get LOWER_ZERO and a wide upper while their sum may be pinned tightly
 * by the reads --, and neither can the per-transcript presence Lambdas, for the reason given at the gene-level two-sample test.  For
 * the sample of upload_structure + upload_sample, solver parameters p, the gene map of emsar_hip_set_gene_map, pp (level, dev_tol,
 * max_evals and their defaults as in emsar_hip_profile) and q = the chi2_1 cut of emsar_hip_profile_cut_host, for gene g:
 *     members, parts, X, F   exactly as emsar_hip_compare_genes defines them for one sample: the members with den_t > 0 take part; the
 *                  parts are the packed sets that hold one and the one-transcript members in closed form, set parts by the smallest
 *                  caller tid of their members, then closed-form parts by tid; mn = the smallest den of the members taking part;
 *                  members (output) = how many take part
 *     baseline     X_hat, F_hat = X and F with every den its own, computed through the code path of every later evaluation.
 *                  gene_hat = X_hat agrees with gene_sums(solve) up to summation order
 *     D_g(x)       = 2 (F_hat - max{F : X = x}), x >= 0
 *     path         the maximiser of F - lambda X is the same problem with den_t + lambda on every member taking part, lambda in
 *                  (-mn, inf); coordinate s = 1 + lambda / mn.  The member(s) at mn take mn * s in LDS, the others den_t + mn (s - 1):
 *                  both stay positive in floating point.  Each set part is one solve -- same solver, start and stopping rule as solve
 *                  --, F summed with the ORIGINAL den, X from the same reduction.  Each point (X(s), F(s)) lies on the profile curve;
 *                  s > 1 is the lower side, 0 < s < 1 the upper side
 *     search       emsar_hip_profile's, unchanged, with den_t := mn, theta_hat := X_hat and F_hat: the first guess uses n = X_hat mn,
 *                  an upper bound of the gene's Poisson information, so the first step is short and the doubling takes over.  One
 *                  workgroup runs one limit: at most max_evals evaluations of at most 64 set solves.  The reported limit is X of the
 *                  last evaluation, dev_lower / dev_upper that evaluation's deviance
 *     end of the range (upper side)   Z = the closed-form members with u = 0 reads, mn0 = their smallest den.  They add nothing to X for
 *                  lambda > -mn0 and absorb any amount at lambda = -mn0 at a cost of mn0 per unit.  If mn0 is strictly below the den of
 *                  every other member taking part, the first evaluation of the upper search is at s = 0 exactly (the others get
 *                  den_t - mn0 > 0): if D_end < q then upper = X_end + (q - D_end) / (2 mn0), dev_upper = q, evals 1 -- beyond X_end the
 *                  profile is linear --, otherwise the ordinary search runs with one evaluation less to spend.  A gene whose parts are
 *                  all closed forms without reads gets upper = q / (2 mn), the transcript profile's rule.  Without this rule such
 *                  genes never bracket
 *     Lambda_g     = D_g(0): F_hat against the solve with den of EVERY member taken as 0 in LDS.  +inf (the gene is essential) when a
 *                  member has reads only it explains (a folded single-transcript row, or a closed form with u > 0; decided before the
 *                  launch) or when the drop leaves a row with reads that nothing explains; 0.0 when X_hat is exactly 0 (the baseline is
 *                  then the maximum under X = 0).  Negative raw values are reported as 0, the most negative goes to the statistics
 *     pvalue       the null X = 0 puts k = members parameters on the boundary: the statistic is a chi-bar-square mixture of
 *                  chi2_0 .. chi2_k whose weights depend on the information matrix, NOT the transcript test's half/half mixture.
 *                  Reported is the bound that is conservative whatever the weights, p = P(chi2_k > Lambda): with x = Lambda / 2,
 *                  exp(-x) sum_{j < k/2} x^j / j! for even k, erfc(sqrt x) + exp(-x) sum_{j=1}^{(k-1)/2} x^(j-1/2) / Gamma(j+1/2) for odd
 *                  k; 1 for Lambda <= 0, 0 for +inf, NaN for NaN or k < 1 (gene_presence_pvalue_host: the same function, no HIP call).
 *                  THE DECISION lower = 0 IS MADE WITH THE chi2_1 CUT q AND IS THEREFORE ANTI-CONSERVATIVE FOR k > 1: lambda and members
 *                  are reported so that a caller can apply a cut of their own
 *     closed form  a gene whose parts are all closed form is finished on the host with the same search, nothing is launched for it
 * status, per gene (EMSAR_PROFILE_* and EMSAR_GENE_PROFILE_TOO_LARGE):
 *     TWO_SIDED     Lambda_g > q, both limits searched
 *     LOWER_ZERO    Lambda_g <= q: lower = 0.0 exactly, dev_lower = Lambda_g; upper searched
 *     OUTSIDE       no member with den > 0, or the gene has no transcript
 *     NOT_RESIDENT  a member taking part lies in a streamed or a cluster set, one component holds most transcripts, or set_mode = 1
 *     TOO_LARGE     more than 64 parts
 *     UNCONVERGED   values are given, but a search or a solve hit its cap
 *   For OUTSIDE, NOT_RESIDENT and TOO_LARGE every numeric output is NaN and evals, parts, members are 0.
 * Outputs are indexed by query position (by gene id when query_genes is NULL; n_query is then ignored); repeats and any order are
 * allowed.  A gene's result depends on its parts, p and pp alone -- not on what else is asked, the batch, the layout, MERGE_ROWS or the
 * library's numbering.  The context is left as it was: a following solve or profile returns the same bits.  ERR_STATE before
 * upload_sample and without a gene map; ERR_ARG for a gene id outside 0 .. n_genes-1, n_query < 0, a level outside (0, 1), a non-finite
 * dev_tol and the parameters solve rejects; ERR_NUMERIC for a non-finite F_hat.  EMSAR_HIP_PROFILE_GENES_BATCH = items per launch and
 * class (a testing aid; the bits do not change). */
enum { EMSAR_GENE_PROFILE_TOO_LARGE = 5 };                              /* the EMSAR_PROFILE_* statuses, and this one */
typedef struct {
    double  *lower, *upper, *dev_lower, *dev_upper, *lambda, *pvalue, *gene_hat;       /* [n_query]; may each be NULL */
    int32_t *status, *evals, *parts, *members;                              /* [n_query] status; evaluations of both searches; parts; k */
} emsar_profile_gene_outputs;
typedef struct {
    int64_t n_status[6];          /* distinct queried genes per status */
    int64_t items_launched;       /* workgroups: one per gene for baseline and drop, one per limit searched */
    int64_t evals_sum;            /* evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over their solves, every part */
    int32_t evals_max, passes_max; /* the search with the most evaluations / the most passes */
    int32_t parts_max, reserved0; /* the most parts of a gene that was searched */
    double  min_raw_lambda;       /* the most negative Lambda before clamping, 0 if none was negative */
    double  cut;                  /* q */
    double  baseline_ms, search_ms; /* device time of baseline + drop, and of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_profile_gene_stats;
int emsar_hip_profile_genes(emsar_hip_ctx *ctx, const emsar_em_params *p, const emsar_profile_params *pp /* or NULL */, int32_t n_query,
                            const int32_t *query_genes /* NULL = all genes */, const emsar_profile_gene_outputs *out /* or NULL */,
                            emsar_profile_gene_stats *stats /* or NULL */);
int emsar_hip_gene_presence_pvalue_host(int64_t n, const double *lambda, const int32_t *members, double *p_out);

/* ---- profile-likelihood intervals of isoform usage: what could a transcript's share of its gene be? ----
 * The interval of the third quantity the library asks its questions of, next to emsar_hip_profile (a transcript's abundance) and
 * emsar_hip_profile_genes (a gene's total).  The bootstrap's percentile interval of a share is [0, 0] where the estimate is 0, and
 * usage_sd says nothing about how far the reads allow two confounded isoforms to move; the profile holds at the boundary.  One sample:
 * the gene map of emsar_hip_set_gene_map, solver parameters p, pp (level, dev_tol, max_evals and their defaults as in emsar_hip_profile;
 * max_outer <= 0: 24), q = the chi2_1 cut of emsar_hip_profile_cut_host.  Members, parts, X, F, mn (the smallest den of the OTHER members
 * taking part) and the 64-part limit are exactly emsar_hip_compare_usage's definitions for one sample.  For transcript t of gene g:
 *     baseline     theta_hat_t, X_hat, F_hat at lambda = 0, computed through the code path of every later evaluation, so every den keeps
 *                  its own bits.  usage = theta_hat_t / X_hat, one IEEE division; it agrees with emsar_hip_isoform_usage up to
 *                  summation order
 *     D_t(u)       = 2 (F_hat - P(u)), P(u) = max {F : theta_t = u X} with everything else free, u in [0, 1].  On each side of usage
 *                  the constraint set {theta_t <= u X} (>=) is a convex cone and F is concave: P is monotone on each side and each
 *                  limit a unique root
 *     ends         lambda_zero = D_t(0): F_hat against the solves with den_t taken as 0 in LDS (the transcript presence statistic,
 *                  here summed over the gene's parts); lambda_one = D_t(1): F_hat against the solves with the den of every other
 *                  member taking part taken as 0.  Each is +inf where a dropped member has reads only it explains (a folded
 *                  single-transcript row, or a closed-form part with u > 0: decided on the host before the launch) or where the drop
 *                  leaves a row with reads that nothing explains; 0.0 where the baseline already lies there (usage exactly 0,
 *                  respectively 1).  Negative raw values are reported as 0, the most negative goes to the statistics
 *     limits       lower = 0.0 exactly and dev_lower = lambda_zero where lambda_zero <= q; upper = 1.0 exactly and
 *                  dev_upper = lambda_one where lambda_one <= q; otherwise the root of D_t(u) = q in (0, usage), respectively (usage, 1)
 *     outer point  one point of a limit search is one inner multiplier search of emsar_hip_compare_usage at fixed u, run on this one
 *                  sample by the same code (den_t + lambda (1 - u) on t, den_s - lambda u on the others; range, coordinate, h and the
 *                  evaluation cap max_evals as there), stopped when 2 |g| * (the width of the bracket in lambda) <= dev_tol q / 4,
 *                  a quarter of what the outer rule allows (the product rule 2 |lambda g| is not used: next to usage it would stop a
 *                  search at its first, small multiplier while the root lies at the end of the range).  The point's value is the
 *                  dual value F - lambda g >= P(u), so the reported D is a lower bound of the true one with an error of second
 *                  order in g, and the interval errs wide.  Its slope is dD/du = -2 lambda Xc, Xc as emsar_hip_compare_usage
 *                  defines it
 *     outer search the coordinate is u itself, the function h(u) = sqrt(D) - sqrt(q): -sqrt(q) at usage, sqrt(D_end) - sqrt(q) > 0 or
 *                  +inf at the end of the side (lambda_zero, lambda_one), both known without an evaluation, and the search never
 *                  leaves the bracket they span.  First point: the Poisson guess for t's own expected reads, c = den_t X_hat
 *                  (t alone with every read unambiguously its own: an upper bound of the information, so a short step):
 *                  usage - sqrt(q usage / c) below, usage + sqrt(q usage / c) + q / (2 c) above; the midpoint of the bracket where
 *                  that falls outside it.  Later points: a Newton step on h with the known slope (h' = D' / (2 sqrt D)) where
 *                  D > 0, the slope has the sign of its side and the step falls strictly inside the bracket; else, while no point
 *                  beyond the root has been seen, twice the distance from usage; else the Illinois step of the bracket (bisection
 *                  while its far end is +inf).  It stops when |D - q| <= dev_tol q (dev_tol <= 0: 1e-4), when the larger |dD/du| of
 *                  the bracket's ends times its width is <= dev_tol q (the end at usage has slope 0, an end not yet evaluated +inf),
 *                  or after max_outer points (then UNCONVERGED).  The reported limit is u of the last outer point and dev_lower /
 *                  dev_upper its D
 *     cost         one workgroup per (gene, t) for the baseline and the two drops, one per limit searched: at most
 *                  max_outer * max_evals * parts * max_iter passes.  A gene whose parts are all closed form is finished on the host
 *                  by the same code and nothing is launched for it
 *     outputs      usage, lower, upper, dev_lower, dev_upper, lambda_zero, lambda_one; outer_evals = outer points of both searches,
 *                  evals = their inner evaluations summed, parts, members = how many take part
 * status, per queried transcript (the first six are EMSAR_PROFILE_* and EMSAR_GENE_PROFILE_TOO_LARGE):
 *     TWO_SIDED     both limits were found by search
 *     LOWER_ZERO    lambda_zero <= q: lower = 0.0; upper searched
 *     UPPER_ONE     lambda_one <= q: upper = 1.0; lower searched
 *     UNIT          both: the interval is [0, 1] -- at this level the isoform cannot be told from its siblings
 *     UNDEFINED     X_hat is exactly 0: usage, limits and Lambdas NaN, the counters are given
 *     SINGLE        fewer than two members take part: the share is 1 by construction
 *     OUTSIDE       den_t == 0, or t has no gene
 *     NOT_RESIDENT  as in emsar_hip_profile_genes
 *     TOO_LARGE     more than 64 parts
 *     UNCONVERGED   values are given, but a solve, an inner search or an outer search hit its cap
 *   For SINGLE, OUTSIDE, NOT_RESIDENT and TOO_LARGE every numeric output is NaN and the counters are 0.
 * Outputs are indexed by query position (by tid when query_tids is NULL; n_query is then ignored); repeats and any order are allowed.  A
 * result depends on the gene's parts, t, p and pp alone -- not on what else is asked, the batch, the layout, MERGE_ROWS or the library's
 * numbering.  The context is left as it was.  Errors as emsar_hip_profile_genes, with tids for gene ids.
 * EMSAR_HIP_PROFILE_USAGE_BATCH = items per launch and class (a testing aid; the bits do not change). */
enum { EMSAR_UPROFILE_UPPER_ONE = 6, EMSAR_UPROFILE_UNIT = 7, EMSAR_UPROFILE_UNDEFINED = 8, EMSAR_UPROFILE_SINGLE = 9 };
typedef struct {
    double  *usage, *lower, *upper, *dev_lower, *dev_upper, *lambda_zero, *lambda_one;     /* [n_query]; may each be NULL */
    int32_t *status, *outer_evals, *evals, *parts, *members;                /* [n_query] */
} emsar_profile_usage_outputs;
typedef struct {
    int64_t n_status[10];         /* distinct queried transcripts per status */
    int64_t items_launched;       /* workgroups: one per (gene, t) for baseline and drops, one per limit searched */
    int64_t evals_sum;            /* inner evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over the searches' solves, every part (baseline and drops not counted) */
    int64_t outer_sum;            /* outer points summed over the searches on the device */
    int32_t evals_max, passes_max; /* the search with the most inner evaluations / the most passes */
    int32_t parts_max, outer_max; /* the most parts of a gene that was searched; the search with the most outer points */
    double  min_raw_lambda;       /* the most negative lambda_zero / lambda_one before clamping, 0 if none was negative */
    double  cut;                  /* q */
    double  baseline_ms, search_ms; /* device time of baseline + drops, and of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_profile_usage_stats;
int emsar_hip_profile_usage(emsar_hip_ctx *ctx, const emsar_em_params *p, const emsar_profile_params *pp /* or NULL */, int32_t n_query,
                            const int32_t *query_tids /* NULL = all transcripts */, const emsar_profile_usage_outputs *out /* or NULL */,
                            emsar_profile_usage_stats *stats /* or NULL */);

/* ---- K-sample test across replicate groups: did a transcript change between conditions? -----------
 * Many samples over one index are quantified to compare CONDITIONS, each with replicates, or the points of a time course.  Pairwise
 * Lambdas of emsar_hip_compare cannot be put together for that: they share a sample and are not independent, and replicates cannot be
 * pooled from outside the likelihood.  Here K contexts (2 <= K <= EMSAR_COMPARE_GROUPS_MAX) on one device hold one structure (checked
 * as emsar_hip_compare checks it) and each its own sample; group_of[k] in 0 .. G-1 names sample k's group, every group non-empty; the
 * size factors s_k > 0 (size NULL: all 1) play the role of emsar_hip_compare's ratio.  F^k is sample k's F_s as the presence test
 * defines it; t's packed set may differ from sample to sample and lie in another size class.  For transcript t and a subset S of the
 * samples, the COMMON-VALUE FIT is
 *     C(S)         = the maximum of sum_{k in S} F^k under theta_t^k = s_k x for every k in S, over x >= 0 and everything else
 *                  = max_x sum_{k in S} P_k(s_k x),  P_k(y) = max {F^k : theta_t^k = y};  C({k}) = F_hat^k, the free fit
 *     Lambda_between = 2 (sum_g C(S_g) - C(all)),         df_between = G - 1: the conditions differ, replicates pooled inside the likelihood
 *     Lambda_within  = 2 (sum_k F_hat^k - sum_g C(S_g)),  df_within = K - G:  the replicates of a condition disagree with each other
 *     p_*          = P(chi2_df > Lambda_*), the tail of emsar_hip_gene_presence_pvalue_host; df 0: 1 for Lambda <= 0.  CONSERVATIVE WHERE
 *                  AN ESTIMATE SITS ON THE BOUNDARY, as for emsar_hip_compare.  THE POISSON LIKELIHOOD HAS NO OVER-DISPERSION TERM: for
 *                  biological replicates Lambda_within will often be large -- that is why it is reported next to Lambda_between --, AND
 *                  p_between IS THEN ANTI-CONSERVATIVE.  No dispersion model is fitted.
 *                  G = K tests "any difference among the K samples" (Lambda_within 0, df 0); G = 1 swaps the roles; K = 2, G = 2,
 *                  s = (r, 1) is emsar_hip_compare's statistic at ratio r, reached by another search.
 *     inner level  one sample k at a target y = s_k x > 0: the maximiser of F^k - lambda theta_t is the set problem with den_t + lambda
 *                  in LDS, F summed with the ORIGINAL den_t (the path of emsar_hip_compare and of the profile intervals).  The gap
 *                  g(lambda) = theta_t(lambda) - y falls in lambda in (-den_t, inf); the dual D(lambda) = F - lambda g >= P_k(y) is convex
 *                  with slope -g, equal to P_k(y) at the root, and dP_k/dy = lambda there.  The side is the sign of theta_hat^k - y
 *                  and needs no solve.  Where t must grow den' = den_t (1 - v); where it must shrink den' = den_t / (1 - v), unbounded
 *                  above, v -> 1 the drop solve.  emsar_hip_compare's search runs on h = g / (theta_t + y) in v in [0, 1), h(1) = -+1
 *                  known without a solve.  It stops when 2 |lambda g| <= dev_tol at an evaluation BEYOND the root (g has changed sign
 *                  since lambda = 0: there |lambda - root| <= |lambda|), when 2 |g| * (the width of the bracket in lambda) <= dev_tol
 *                  (the shrinking side has no finite end: the rule waits for a bracket whose upper end is an evaluation), or after
 *                  max_evals evaluations; both rules bound D - P_k(y) by dev_tol / 2.  The search leaves D at its last evaluation and,
 *                  as the slope dP_k/dy, the multiplier of the bracket's next Illinois point (an estimate of the root whose error is
 *                  of second order in the bracket).  A one-transcript component is the closed form of emsar_hip_compare.
 *     outer level  sum_k P_k(s_k x) is concave in x with slope Gs(x) = sum_k s_k lambda_k(x).  At x_lo = min_k theta_hat^k / s_k no
 *                  sample has to rise above its estimate: every lambda_k >= 0 and Gs >= 0; at x_hi = max_k theta_hat^k / s_k every
 *                  lambda_k <= 0.  So the signs at the two ends are known without an evaluation.  Illinois steps on
 *                  h = Gs / sum_k |s_k lambda_k| over (x_lo, x_hi); every evaluated x lies strictly inside, so a target is never 0.
 *                  Outer point 0 is lambda = 0 in every sample and gives theta_hat^k and F_hat^k from the code path of every later
 *                  evaluation; if all theta_hat^k / s_k are equal the search ends there with C = sum F_hat and outer = 1.  It stops
 *                  when 2 |Gs| (x_hi - x_lo) <= dev_tol or after max_outer points, point 0 counted (at least one point of the null is
 *                  evaluated whatever max_outer says).  C(S) is the largest sum of the samples' dual values among the outer points,
 *                  x_S that point.
 *     cost         per transcript one search for all samples and one per group of two or more (a single group is the all-samples
 *                  search itself); one workgroup runs one search, the samples in ascending index: at most
 *                  max(max_outer, 2) * |S| * max_evals * max_iter passes.  A transcript that is a one-transcript component in every
 *                  sample is searched on the host by the same code and nothing is launched for it.
 *     outputs      lambda_between, lambda_within (clamped at 0), raw_between, raw_within (before clamping), p_between, p_within;
 *                  theta_common = x of C(all), on the scale of size 1; theta_group[i][g] = x of C(S_g) (theta_hat^k / s_k for a group
 *                  of one); theta_hat[i][k]; slope = the outer stopping quantity of the all-samples search, outer = its outer points;
 *                  evals = the inner evaluations of all the transcript's searches.  Each Lambda is computed from the deficits
 *                  sum_{k in S} F_hat^k - C(S), exactly 0 for a search that ended at outer point 0.
 * status, per transcript:
 *     TESTED        outputs as above
 *     ALL_ABSENT    theta_hat_t is exactly 0 in every sample: both Lambdas 0, p 1
 *     OUTSIDE       den_t == 0 in any sample.  Every numeric output NaN, the counters 0
 *     NOT_RESIDENT  as in emsar_hip_compare, in any sample.  Every numeric output NaN, the counters 0
 *     UNCONVERGED   values are given, but a solve, an inner search or an outer search hit its cap
 * Outputs are indexed by query position (by tid when query_tids is NULL; n_query is then ignored); repeats and any order are allowed.  A
 * transcript's result depends on its K sets, itself, the groups and sizes, p and gp alone -- not on what else is asked, the batch, the
 * layout, MERGE_ROWS or the library's numbering.  All contexts are left as they were.  ERR_STATE when any context is before
 * upload_sample; ERR_ARG for a NULL context, a context given twice, different devices or structures, K outside 2 .. 32, a group id
 * outside 0 .. G-1 or an empty group (G = the largest id + 1), a size that is not finite and positive, a tid outside 0 .. n_tx-1,
 * n_query < 0, a non-finite dev_tol and the parameters solve rejects; ERR_NUMERIC for a non-finite F at lambda = 0.
 * EMSAR_HIP_GROUPS_BATCH = items per launch and class (a testing aid; the bits do not change).  compare_groups_pvalue_host:
 * P(chi2_df > Lambda) per element, df 0: 1 for Lambda <= 0 and 0 above; NaN for NaN or df < 0; no HIP call. */
#define EMSAR_COMPARE_GROUPS_MAX 32
enum {
    EMSAR_GROUPS_TESTED = 0, EMSAR_GROUPS_ALL_ABSENT = 1, EMSAR_GROUPS_OUTSIDE = 2, EMSAR_GROUPS_NOT_RESIDENT = 3, EMSAR_GROUPS_UNCONVERGED = 4
};
typedef struct { double dev_tol; int32_t max_evals, max_outer; } emsar_groups_params;  /* NULL or <= 0: 1e-4 (both levels), 40, 12 */
typedef struct {
    double  *lambda_between, *p_between, *lambda_within, *p_within, *raw_between, *raw_within, *theta_common, *slope;  /* [n_query]; may each be NULL */
    double  *theta_group;         /* [n_query][G] */
    double  *theta_hat;           /* [n_query][K] */
    int32_t *status, *outer, *evals;                                        /* [n_query] EMSAR_GROUPS_*; outer points; inner evaluations */
} emsar_groups_outputs;
typedef struct {
    int64_t n_status[5];          /* distinct queried transcripts per status */
    int64_t items_launched;       /* workgroups: one search each */
    int64_t evals_sum;            /* inner evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over their solves, every sample */
    int64_t outer_sum;            /* outer points summed over the searches on the device */
    int32_t evals_max, passes_max; /* the search with the most inner evaluations / the most passes */
    int32_t outer_max, reserved0; /* the search with the most outer points */
    int32_t df_between, df_within; /* G - 1, K - G */
    double  min_raw_lambda;       /* the most negative of both Lambdas before clamping, 0 if none was negative */
    double  device_ms;            /* device time of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_groups_stats;
int emsar_hip_compare_groups(emsar_hip_ctx *const *ctx /* [n_samples] */, int32_t n_samples, const int32_t *group_of /* [n_samples] */,
                             const double *size /* [n_samples] or NULL */, const emsar_em_params *p, const emsar_groups_params *gp /* or NULL */,
                             int32_t n_query, const int32_t *query_tids /* NULL = all transcripts */, const emsar_groups_outputs *out /* or NULL */,
                             emsar_groups_stats *stats /* or NULL */);
int emsar_hip_compare_groups_pvalue_host(int64_t n, const double *lambda, const int32_t *df, double *p_out);

/* ---- gene-level K-sample test across replicate groups: which genes changed between conditions? ----
 * The per-transcript lines of emsar_hip_compare_groups cannot be added up, for the reasons given at the gene-level two-sample test
 * (isoforms that trade reads at an unchanged total give several small p-values, a gene whose total moved but whose isoforms are
 * confounded gives none), and the pairwise emsar_hip_compare_genes share a sample and cannot be combined.  The contexts, group_of, the
 * size factors s_k, the degrees of freedom and gp are emsar_hip_compare_groups'; the gene map is that of the FIRST context
 * (emsar_hip_set_gene_map; another context may hold the same map or none).  For gene g:
 *     members, parts, X^k, F^k   exactly as emsar_hip_compare_genes defines them, per sample: the members with den_t > 0 in sample k take
 *                  part there; the parts are the packed sets that hold one (by the smallest caller tid of their members), then the
 *                  one-transcript members in closed form (by tid); X^k = the sum of theta over the members taking part, F^k = the sum
 *                  of the parts' F; mn^k = the smallest den of the members taking part.  The parts of a gene may differ from sample to
 *                  sample and lie in other size classes
 *     C_g(S)       = max_x sum_{k in S} P_k(s_k x),  P_k(y) = max {F^k : X^k = y}: the isoforms and everything else stay free in every
 *                  sample;  C_g({k}) = F_hat^k
 *     Lambda_between = 2 (sum_g' C_g(S_g') - C_g(all)),         df_between = G - 1
 *     Lambda_within  = 2 (sum_k F_hat^k - sum_g' C_g(S_g')),    df_within = K - G;   p_* as emsar_hip_compare_groups, WITH ITS CAVEATS: no
 *                  over-dispersion term, conservative where an estimate sits on the boundary
 *     path         emsar_hip_compare_groups' two-level search, the same code, with theta_t := X^k and den_t := mn^k.  The maximiser of
 *                  F^k - lambda X^k is the problem with den_t + lambda on EVERY member taking part, lambda in (-mn^k, inf).  Where the
 *                  gene must grow the member(s) at mn^k take mn^k (1 - v) in LDS and the others den_t - v mn^k; where it must shrink
 *                  mn^k / (1 - v) and den_t + mn^k v / (1 - v): both stay positive in floating point (emsar_hip_compare_genes' rule).
 *                  Each set part is one solve -- same solver, start and stopping rule as solve --, F summed with the ORIGINAL den, X
 *                  from the same reduction; the dual value of a sample is F - lambda (X - y).  Outer point 0 is lambda = 0 in every
 *                  sample and gives X_hat^k and F_hat^k from the code path of every later evaluation.  Stopping rules, caps and the
 *                  choice of C_g(S) among the outer points are emsar_hip_compare_groups'.
 *     end of the range   a sample in which the member(s) at mn^k have no reads cannot raise X^k by any lambda > -mn^k; the inner search
 *                  then runs to v -> 1 and its dual value tends to the true P_k(y) = P_k(X_end) - mn^k (y - X_end), within dev_tol / 2
 *                  by the bracket rule, as the transcript test treats a transcript without reads
 *     cost         per gene one search for all samples and one per group of two or more (a single group is the all-samples search
 *                  itself); one workgroup runs one search, the samples in ascending index: at most
 *                  max(max_outer, 2) * |S| * max_evals * parts * max_iter passes, parts <= 64 per sample.  A gene whose parts are all
 *                  closed form in every sample is searched on the host by the same code and nothing is launched for it.
 *     outputs      lambda_between, lambda_within (clamped at 0), raw_between, raw_within, p_between, p_within; gene_common = x of
 *                  C_g(all), on the scale of size 1; gene_group[i][g'] = x of C_g(S_g') (X_hat^k / s_k for a group of one);
 *                  gene_hat[i][k] = X_hat^k, which agrees with gene_sums(solve) up to summation order; slope, outer = the all-samples
 *                  search's; evals = the inner evaluations of all the gene's searches; parts = the parts summed over the samples
 * status, per gene (EMSAR_GROUPS_* and EMSAR_GENE_GROUPS_TOO_LARGE), decided in this order:
 *     NOT_RESIDENT  a member taking part lies in a streamed or a cluster set in any sample, one component holds most transcripts, or
 *                   set_mode = 1
 *     OUTSIDE       in some sample no member has den > 0, or the gene has no transcript
 *     TOO_LARGE     more than 64 parts in a sample
 *     TESTED        outputs as above
 *     ALL_ABSENT    X_hat^k is exactly 0 in every sample: both Lambdas 0, p 1
 *     UNCONVERGED   values are given, but a solve, an inner search or an outer search hit its cap
 *   For NOT_RESIDENT, OUTSIDE and TOO_LARGE every numeric output is NaN and the counters are 0.
 * Outputs are indexed by query position (by gene id when query_genes is NULL; n_query is then ignored); repeats and any order are
 * allowed.  A gene's result depends on its parts, p, gp, the groups and the sizes alone -- not on what else is asked, the batch, the
 * layout, MERGE_ROWS, the library's numbering or which of the other contexts hold the map.  All contexts are left as they were: a
 * following solve, compare_groups or compare_genes returns the same bits.  Errors as emsar_hip_compare_groups, with gene ids for tids;
 * in addition ERR_STATE when the first context has no gene map and ERR_ARG when another context holds a different one.
 * EMSAR_HIP_GROUPS_GENES_BATCH = items per launch and class (a testing aid; the bits do not change). */
enum { EMSAR_GENE_GROUPS_TOO_LARGE = 5 };                               /* the EMSAR_GROUPS_* statuses, and this one */
typedef struct {
    double  *lambda_between, *p_between, *lambda_within, *p_within, *raw_between, *raw_within, *gene_common, *slope;   /* [n_query]; may each be NULL */
    double  *gene_group;          /* [n_query][G] */
    double  *gene_hat;            /* [n_query][K] */
    int32_t *status, *outer, *evals, *parts;                                /* [n_query] status; outer points; inner evaluations; parts */
} emsar_groups_gene_outputs;
typedef struct {
    int64_t n_status[6];          /* distinct queried genes per status */
    int64_t items_launched;       /* workgroups: one search each */
    int64_t evals_sum;            /* inner evaluations summed over the searches on the device */
    int64_t passes_sum;           /* passes summed over their solves, every part of every sample */
    int64_t outer_sum;            /* outer points summed over the searches on the device */
    int32_t evals_max, passes_max; /* the search with the most inner evaluations / the most passes */
    int32_t outer_max, parts_max; /* the search with the most outer points; the most parts (all samples) of a gene that was searched */
    int32_t df_between, df_within; /* G - 1, K - G */
    double  min_raw_lambda;       /* the most negative of both Lambdas before clamping, 0 if none was negative */
    double  device_ms;            /* device time of the searches (HIP events) */
    double  total_ms;             /* wall time of the call, a first call's set building included */
} emsar_groups_gene_stats;
int emsar_hip_compare_groups_genes(emsar_hip_ctx *const *ctx /* [n_samples] */, int32_t n_samples, const int32_t *group_of /* [n_samples] */,
                                   const double *size /* [n_samples] or NULL */, const emsar_em_params *p, const emsar_groups_params *gp /* or NULL */,
                                   int32_t n_query, const int32_t *query_genes /* NULL = all genes */,
                                   const emsar_groups_gene_outputs *out /* or NULL */, emsar_groups_gene_stats *stats /* or NULL */);

/* ---- asymptotic standard errors: the inverse of the observed information at the MLE ---------------
 * How sure is theta_t, without resampling?  For a theta that maximises the likelihood of the current sample, the observed information
 * of the ACTIVE transcripts is J_ij = sum_c m_ci m_cj R_c / S_c^2 (m_ci = how often i stands in row c); its inverse is the asymptotic
 * covariance of the estimates.  J is block diagonal over the connected components of the active transcripts, so one dense
 * factorisation per component replaces the B solves of the bootstrap.  The function does not check that theta is an MLE.
 * ASYMPTOTIC NORMALITY DOES NOT HOLD AT THE BOUNDARY: a transcript whose estimate is (about) 0 has a one-sided, non-normal
 * distribution.  Such transcripts are held fixed here and get variance 0; the bootstrap (emsar_hip_bootstrap*) is the tool there, and
 * for transcripts that are nearly confounded with a sibling (a tiny pivot; see min_pivot_ratio and partner).
 * Everything is in caller numbering and caller row order: no result depends on the layout, on MERGE_ROWS, on the library's own
 * transcript numbering or on the device.  Every operation below is rounded on its own (no fused multiply-add).
 * Inputs: the structure of upload_structure; R_c = the row weights of upload_sample (0 where E was 0 at that call); theta[n_tx],
 * finite and >= 0, checked on the host; the parameters: boundary_cut (params NULL means EMSAR_ASYM_DEFAULT_CUT, 5e-7, the .fpkm
 * print quantum; 0 is allowed; a negative cut is taken as it stands and makes every transcript active, theta_t = 0 included),
 * pivot_tol (<= 0 means 1e-10), block_tid (-1 = none).
 * Active set.  t is ACTIVE iff theta_t > boundary_cut.  Inactive transcripts are held fixed: they still count in every S_c, and get
 *   status BOUNDARY, var 0, rowsum 0, partner -1, partner_cov NaN.
 * Rows.  S_c = sum of theta over the row's entries, left to right (a repeated tid counts twice).  w_c = R_c / (S_c * S_c) when
 *   R_c > 0 and S_c > 0, else 0.  A row with entries, R_c > 0 and S_c == 0 is INFEASIBLE (counted in rows_infeasible); only an infeasible row
 *   that holds an ACTIVE transcript marks a component, which can only be when boundary_cut < 0 was given (theta_t = 0 > cut).  Its
 *   component gets status INFEASIBLE (numeric outputs NaN).  An infeasible row without an active transcript belongs to no component.
 * Components: the connected components of the ACTIVE transcripts, linked by the rows with w_c != 0 and by infeasible rows.  Local
 *   indices 0 .. n-1 by ascending caller tid; components are ordered by their smallest tid.  A component of more than 192 active
 *   transcripts is TOO_LARGE (numeric outputs NaN); TOO_LARGE wins over INFEASIBLE.
 * Information matrix, n x n, lower triangle.  J_ij starts from 0.0; over the entries k of transcript i in (caller row ascending,
 *   position ascending) order, and for each over the entries k' of transcript j in the same row in position order: J_ij = J_ij + w_c.
 *   A tid that stands twice in a row adds w_c four times to its diagonal.
 * LDL^T without square roots.  For j = 0 .. n-1 and i >= j:  acc = J_ij;  for k < j ascending  acc = acc - (L_ik * D_k) * L_jk;
 *   i == j: D_j = acc;  i > j: L_ij = acc / D_j.  Pivot rule: D_j must be finite and D_j > pivot_tol * J_jj (the original diagonal);
 *   otherwise the component is UNIDENTIFIABLE: var = rowsum = +inf, partner -1, partner_cov NaN, and blocker = the caller tid of
 *   local j, the first failing pivot.  A one-transcript component with J_tt == 0 (no row with reads holds it) fails the same way.
 * M = L^-1, row by row; for j < i:  acc = L_ij;  for k = j+1 .. i-1  acc = acc + L_ik * M_kj;  M_ij = -acc;  M_ii = 1.
 * Covariance.  Sigma_ij = sum over k = max(i,j) .. n-1 ascending of (M_ki * M_kj) / D_k, starting from the first term.
 * Per ESTIMATED transcript (local i):
 *   var         = Sigma_ii
 *   rowsum      = sum_j Sigma_ij, j ascending, starting from the first term
 *   genesum     = the same sum over the j with gene(j) == gene(i) >= 0; 0 without a gene map or for gene -1 (internal: it feeds gene_sd)
 *   partner     = the caller tid of the j != i that minimises Sigma_ij * |Sigma_ij| / Sigma_jj (the most negative correlation, signed
 *                 and squared, times var: only *, / and comparisons), the lowest local index among equal values, the first j when
 *                 no value compares below it; -1 when n == 1.  partner_cov = that Sigma_ij (NaN when none).  It names the sibling t
 *                 is most confounded with.
 * Block output: with block_tid >= 0 the component of that transcript whole: block_n = n, block_tids[0 .. n-1] and block_cov, the
 *   first n * n entries row-major with rows of n, symmetric.  block_n = 0 when the transcript is not ESTIMATED or block_tid = -1.
 *   All three pointers given, or none.
 * Host finish: one function for the device path and the host path, evaluated as written, left to right.  "chunked sum" = gene_sums'
 *   rule over ascending tid: consecutive chunks of 256 added left to right from their first term, then the chunk sums left to right.
 *   sd_fpkm  = sqrt(var)
 *   S        = the chunked sum of theta over all transcripts;  V_S = the chunked sum of rowsum over the ESTIMATED transcripts (the
 *              others count 0.0).  V_S LEAVES OUT the variance of active transcripts that are not ESTIMATED; their share of S is
 *              theta_unestimated_share = (chunked sum of theta over the active, not ESTIMATED transcripts) / S, 0 for S == 0.
 *   a = theta_t / S;  var_tpm = ((1e6 / S) * (1e6 / S)) * max(0, var - 2 * a * rowsum + a * a * V_S);  sd_tpm = sqrt(var_tpm) for an
 *              ESTIMATED or BOUNDARY transcript, +inf for UNIDENTIFIABLE, NaN for TOO_LARGE and INFEASIBLE; 0 for all when S == 0.
 *              max(0, x) is x when x > 0, else 0.
 *   per gene   V_G = gene_sums of genesum (its own order; on the device path the device's gene_sums), gene_sd = sqrt(V_G).
 *              gene_status = TOO_LARGE if a transcript of the gene is, else INFEASIBLE, else UNIDENTIFIABLE, else ESTIMATED if one
 *              is, else BOUNDARY; gene_sd = NaN for TOO_LARGE and INFEASIBLE, +inf for UNIDENTIFIABLE.
 *   usage_sd   G = gene_sums of theta, u = theta_t / G:  sqrt(max(0, var - 2 * u * genesum + u * u * V_G)) / G; 0 for G == 0; NaN /
 *              +inf where gene_sd is; NaN for a transcript without a gene.  Needs the gene map.
 *   asymptotic       ERR_STATE before upload_sample and for gene outputs (gene_sd, gene_status, usage_sd) without a map; ERR_ARG for
 *                    a NULL, negative or non-finite theta, a block_tid outside -1 .. n_tx-1, a gene group or a block group only
 *                    partly given.  out, stats and params may be NULL.  The first call after upload_structure uploads the
 *                    caller-order CSR model_fit shares.  The context is left as it was: a following solve returns the same bits.
 *   asymptotic_host  the same definition with no HIP call and no context; row_E NULL or given: rows with E == 0 have R = 0.  The
 *                    stage times of the device stay 0.  Device and host return the same bits in every output.
 * Device: EMSAR_HIP_ASYM_CLASS = 1 | 2 runs every component in at least the 64-lane / the 256-thread kernel (a testing aid; the bits
 * do not change). */
enum {
    EMSAR_ASYM_ESTIMATED = 0, EMSAR_ASYM_BOUNDARY = 1, EMSAR_ASYM_UNIDENTIFIABLE = 2, EMSAR_ASYM_TOO_LARGE = 3, EMSAR_ASYM_INFEASIBLE = 4
};
#define EMSAR_ASYM_MAX_N 192
#define EMSAR_ASYM_DEFAULT_CUT 5e-7
typedef struct { double boundary_cut, pivot_tol; int32_t block_tid, reserved0; } emsar_asym_params;
typedef struct {
    double  *var, *sd_fpkm, *sd_tpm, *rowsum, *usage_sd;    /* [n_tx]; may each be NULL; usage_sd needs the gene map */
    int32_t *status, *partner;                              /* [n_tx] EMSAR_ASYM_*; caller tid or -1 */
    double  *partner_cov;                                   /* [n_tx] */
    int32_t *blocker;                                       /* [n_tx] caller tid of the first failing pivot of an UNIDENTIFIABLE component, else -1 */
    double  *gene_sd;                                       /* [n_genes]; gene_sd and gene_status both NULL, or both given after set_gene_map */
    int32_t *gene_status;                                   /* [n_genes] */
    int32_t *block_n, *block_tids;                          /* [1], [192] */
    double  *block_cov;                                     /* [192 * 192] */
} emsar_asym_outputs;
typedef struct {
    int64_t components;                  /* all components of active transcripts, the next two included */
    int64_t components_too_large, components_infeasible;
    int64_t components_class[4];         /* factorised: by one lane (n == 1), 8 lanes, one wave, 256 threads (the host path counts by n) */
    int64_t components_unidentifiable;
    int64_t n_status[5];                 /* transcripts per status */
    int64_t rows_infeasible;             /* rows with R_c > 0 and S_c == 0 */
    int32_t max_n, reserved0;            /* the largest component, TOO_LARGE ones included */
    double  min_pivot_ratio;             /* the smallest D_j / J_jj over every pivot up to a component's first failing one; +inf if none */
    double  theta_unestimated_share;
    double  plan_ms;                     /* host: active set, components, records */
    double  rows_ms, sets_ms, genes_ms;  /* device time per stage (HIP events); 0 on the host path */
    double  total_ms;                    /* wall time of the call */
} emsar_asym_stats;
int emsar_hip_asymptotic(emsar_hip_ctx *ctx, const double *theta /* n_tx */, const emsar_asym_params *params /* or NULL: defaults */,
                         const emsar_asym_outputs *out /* or NULL */, emsar_asym_stats *stats /* or NULL */);
int emsar_hip_asymptotic_host(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                              const int32_t *row_weight /* NULL = 1 */, const double *row_E /* or NULL */, const double *theta,
                              int32_t n_genes, const int32_t *gene_of_tx /* n_tx, or NULL = no gene map */,
                              const emsar_asym_params *params /* or NULL */, const emsar_asym_outputs *out /* or NULL */,
                              emsar_asym_stats *stats /* or NULL */);

/* ---- introspection ------------------------------------------------------------------------------ */
typedef struct {
    int64_t n_rows, nnz;
    int32_t n_tx;
    int32_t layout;            /* layout in use (flags included) */
    int64_t n_chunks;          /* TILED: tiles (one workgroup each, or one per pair of tiles) */
    int64_t n_slices;          /* TILED: 768-row slices (one wavefront at a time) */
    int64_t padded_entries;    /* stored forward slots incl. padding */
    int64_t far_entries;       /* entries outside their tile's contiguous tid range */
    int32_t window;            /* transcripts per dictionary */
    int32_t device_id;
    int64_t bytes_per_pass;        /* SURVEY.md 8d formula */
    int64_t stored_bytes_per_pass; /* what the layout streams */
    int64_t tiled_entries;         /* TILED: stored operands without padding (an operand = a block of 3 dictionary slots + a subset) */
    int64_t tiled_ids;             /* TILED: transcript ids of the tiled rows; tiled_ids / tiled_entries = ids served per operand */
    int64_t n_units;               /* TILED: workgroups of k_pass_tiled_unit (tiles that share a dictionary) */
    int32_t renumbered;            /* TILED: 1 = the library numbered the transcripts by co-occurrence (theta / den are mapped at this ABI) */
    int32_t reserved0;
} emsar_hip_info;
int emsar_hip_get_info(const emsar_hip_ctx *ctx, emsar_hip_info *out);

/* Host-only diagnostic (no HIP call, works without a GPU): build the TILED layout for a CSR (forward index, transposed index,
 * dictionaries, folded and leftover rows), check every descriptor against the arrays it indexes, decode the layout
 * again and check that it stores exactly the input rows. */
int emsar_hip_layout_selfcheck_tiled(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                                     int merge_rows, emsar_hip_info *info_out);

/* The same for the set-resident solver's records (set_mode 0): find the connected sets of the rows with weight > 0
 * (row_weight NULL = every row counts 1), pack the ones that fit a workgroup's LDS and check the records against the CSR. */
typedef struct {
    int64_t n_components;        /* connected sets with at least two transcripts */
    int64_t sets_resident[3];    /* by workgroup class: 64 / 256 / 512 threads */
    int64_t max_lds_bytes[3];    /* largest LDS footprint in each class */
    int64_t sets_streamed;       /* sets too large for one workgroup */
    int64_t tids_closed, tids_resident, tids_streamed;
    int64_t rows_in, rows_stored; /* weighted multi-transcript rows before / after merging identical ones */
    int64_t sets_cluster, tids_cluster, max_lds_cluster;   /* sets packed for a cluster of workgroups, their transcripts, the largest LDS footprint of one of their workgroups */
} emsar_hip_sets_info;
int emsar_hip_sets_selfcheck(int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                             const int32_t *row_weight, emsar_hip_sets_info *info_out);

#ifdef __cplusplus
}
#endif
#endif /* EMSAR_HIP_H */
