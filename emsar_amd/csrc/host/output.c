/* output.c -- the reference's three output files, byte for byte in layout:
 *   .fpkm               print_FPKMfinal      emsar_functions.c:3184,3207   "%s\t%lf\t%lf\t%lf\t%lf\t%d\t%lf\n"
 *   .fraglength_effect  print_FraglengthDist emsar_functions.c:2489-2490   "%d\t%d\t%lg\n"
 *   .segments           print_aEUMA_3        emsar_functions.c:2274-2297
 * and the bootstrap's own file (no counterpart in the reference):
 *   .bootstrap          "%s\t%lf\t%lf\t%lf\t%lf\t%lf\n"  FPKM and TPM as in .fpkm, then the Poisson bootstrap's mean / sd
 * and, with --g2t, the gene files:
 *   .gfpkm              util/FPKM2gFPKM.pl's header byte for byte, rows "%s\t%lf\t%lf\t%d\t%lf\n" (the script prints Perl's
 *                       default number format; merge_gTPM.pl / merge_gReadcount.pl read either)
 *   .gbootstrap         the columns of .bootstrap per gene
 * and the bootstrap quantiles' files (--bootstrap-quantiles):
 *   .bootq              a header naming the probabilities (FPKM@q.. then TPM@q.., q as "%.17g"), then per transcript the quantiles of
 *                       FPKM at each q and of TPM at each q over the bootstrap replicates, all "%lf"
 *   .gbootq             the same per gene, in the order of .gfpkm
 * and the isoform usage's file (--g2t --isoforms):
 *   .isoforms           per transcript that is in a gene, in the order of .fpkm: transcript_ID gene_ID FPKM usage dominant
 *                       ("%s\t%s\t%lf\t%lf\t%d"), with --bootstrap also usage_mean usage_sd dominant_freq, with --bootstrap-quantiles
 *                       also usage_q<q> per probability (q as "%.17g"), all "%lf"
 * and the model fit's files (--fit):
 *   .fit                per transcript, in the order of .fpkm: transcriptID FPKM eff_segments chi2 deviance miss_reads miss_fraction
 *                       worst_segment ("%s\t%lf\t%lf\t%lf\t%lf\t%lf\t%lf\t%s"; worst_segment is the c<row> id of .segments, or "-")
 *   .gfit               per gene, in the order of .gfpkm: geneID eff_segments chi2 deviance miss_reads miss_fraction
 * and the depth subsampling's files (--subsample):
 *   .saturation         "# fractions=.. replicates=.. seed=.. depth_mean=..", a header, then per transcript FPKM and TPM as in .fpkm and
 *                       per fraction mean_FPKM sd_FPKM mean_TPM sd_TPM, all "%lf"
 *   .gsaturation        the same per gene, per fraction mean_FPKM sd_FPKM mean_TPM
 * and the files of the tests and intervals, each with a status word (one table per family below) and "nan" / "inf" for a value that is
 * not finite:
 *   .presence, .profile, .asym, .gasym     see emsar_host.h; an infinity is written without a sign
 *   .gprofile           per gene, in the order of .gfpkm: gene gFPKM lower upper Lambda p members status
 *   .compare            per queried transcript: tid transcriptID FPKM FPKM_ref log2FC Lambda p status evals
 *   .gcompare           per gene, in the order of .gfpkm: gene gFPKM gFPKM_ref log2FC Lambda p status evals parts
 *   .ucompare           per queried transcript: transcript gene usage usage_ref dlogit Lambda p status outer evals
 *   .uprofile           per queried transcript: transcript gene usage lower upper Lambda_zero Lambda_one status outer evals
 *                       in these four the numbers are "%lf", p is "%.6g" and a negative infinity is written "-inf"
 *   .groups             "# samples=.. groups=g0,.. sizes=s0,.. df_between=.. df_within=..", a header, then per queried transcript:
 *                       transcript FPKM_common FPKM_g0 .. Lambda_between df p_between Lambda_within df p_within status outer evals,
 *                       numbers and p as in .compare
 *   .ggroups            the same "#" line, then per gene, in the order of .gfpkm: gene gFPKM_common gFPKM_g0 .. and .groups' columns, then parts
 * Column order of .fpkm is a contract: the reference's Perl utilities read columns 0,1,4,6 (util/FPKM2gFPKM.pl:19).
 */
#include "emsar_host.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

int emsar_write_fpkm(const char *path, const emsar_rsh *r, const double *mean, const double *sd, const double *ieuma,
                     const double *ireadcount, const int32_t *ireadcount_int, const double *tpm, int64_t *total_ir) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    int64_t tot = 0;
    fprintf(f, "transcriptID\tFPKM\tsd.of.FPKM\teff.length\tiReadcount\tiReadcount.int\tTPM\n");
    for (int32_t t = 0; t < r->n_tx; t++) {
        tot += ireadcount_int[t];
        fprintf(f, "%s\t%lf\t%lf\t%lf\t%lf\t%d\t%lf\n", r->names[t], mean[t], sd[t], ieuma[t], ireadcount[t],
                ireadcount_int[t], tpm[t]);
    }
    if (total_ir) *total_ir = tot;
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_bootstrap(const char *path, const emsar_rsh *r, const double *fpkm, const double *boot_mean, const double *boot_sd,
                          const double *tpm, const double *boot_tpm_sd) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "transcriptID\tFPKM\tboot.mean.FPKM\tboot.sd.FPKM\tTPM\tboot.sd.TPM\n");
    for (int32_t t = 0; t < r->n_tx; t++)
        fprintf(f, "%s\t%lf\t%lf\t%lf\t%lf\t%lf\n", r->names[t], fpkm[t], boot_mean[t], boot_sd[t], tpm[t], boot_tpm_sd[t]);
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* FPKM2gFPKM.pl's roundoff: ($x - int($x) >= 0.5) ? int($x) + 1 : int($x), int() truncating toward zero */
static int roundoff(double x) {
    const double i = trunc(x);
    return (int)i + (x - i >= 0.5 ? 1 : 0);
}

int emsar_write_gfpkm(const char *path, const emsar_genes *g, const double *fpkm, const double *ir, const double *tpm) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "geneID\tFPKM\tiReadcount\tiReadcount.int\tTPM\n");
    for (int32_t k = 0; k < g->n_genes; k++)
        fprintf(f, "%s\t%lf\t%lf\t%d\t%lf\n", g->names[k], fpkm[k], ir[k], roundoff(ir[k]), tpm[k]);
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_gbootstrap(const char *path, const emsar_genes *g, const double *fpkm, const double *boot_mean, const double *boot_sd,
                           const double *tpm, const double *boot_tpm_sd) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "geneID\tFPKM\tboot.mean.FPKM\tboot.sd.FPKM\tTPM\tboot.sd.TPM\n");
    for (int32_t k = 0; k < g->n_genes; k++)
        fprintf(f, "%s\t%lf\t%lf\t%lf\t%lf\t%lf\n", g->names[k], fpkm[k], boot_mean[k], boot_sd[k], tpm[k], boot_tpm_sd[k]);
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* the rows of .bootq / .gbootq: n names, fpkm_q and tpm_q = [n_q][n] */
static int write_bootq(const char *path, const char *id, char **names, int64_t n, int n_q, const double *q, const double *fpkm_q, const double *tpm_q) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "%s", id);
    for (int k = 0; k < n_q; k++) fprintf(f, "\tFPKM@%.17g", q[k]);
    for (int k = 0; k < n_q; k++) fprintf(f, "\tTPM@%.17g", q[k]);
    fprintf(f, "\n");
    for (int64_t t = 0; t < n; t++) {
        fprintf(f, "%s", names[t]);
        for (int k = 0; k < n_q; k++) fprintf(f, "\t%lf", fpkm_q[(int64_t)k * n + t]);
        for (int k = 0; k < n_q; k++) fprintf(f, "\t%lf", tpm_q[(int64_t)k * n + t]);
        fprintf(f, "\n");
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_bootq(const char *path, const emsar_rsh *r, int n_q, const double *q, const double *fpkm_q, const double *tpm_q) {
    return write_bootq(path, "transcriptID", r->names, r->n_tx, n_q, q, fpkm_q, tpm_q);
}

int emsar_write_gbootq(const char *path, const emsar_genes *g, int n_q, const double *q, const double *fpkm_q, const double *tpm_q) {
    return write_bootq(path, "geneID", g->names, g->n_genes, n_q, q, fpkm_q, tpm_q);
}

int emsar_write_isoforms(const char *path, const emsar_rsh *r, const emsar_genes *g, const double *fpkm, const double *usage,
                         const int32_t *dominant, int n_boot, const double *usage_mean, const double *usage_sd,
                         const int32_t *dominant_count, int n_q, const double *q, const double *usage_q) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    if (n_boot <= 0) n_q = 0;
    fprintf(f, "transcript_ID\tgene_ID\tFPKM\tusage\tdominant");
    if (n_boot > 0) fprintf(f, "\tusage_mean\tusage_sd\tdominant_freq");
    for (int k = 0; k < n_q; k++) fprintf(f, "\tusage_q%.17g", q[k]);
    fprintf(f, "\n");
    for (int32_t t = 0; t < r->n_tx; t++) {
        const int32_t k = g->gene_of_tx[t];
        if (k < 0) continue;
        fprintf(f, "%s\t%s\t%lf\t%lf\t%d", r->names[t], g->names[k], fpkm[t], usage[t], dominant[k] == t ? 1 : 0);
        if (n_boot > 0) fprintf(f, "\t%lf\t%lf\t%lf", usage_mean[t], usage_sd[t], (double)dominant_count[t] / (double)n_boot);
        for (int j = 0; j < n_q; j++) fprintf(f, "\t%lf", usage_q[(int64_t)j * r->n_tx + t]);
        fprintf(f, "\n");
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_fit(const char *path, const emsar_rsh *r, const double *fpkm, const double *den, const double *df, const double *chi2,
                    const double *dev, const double *miss, const int32_t *worst_row) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "transcriptID\tFPKM\teff_segments\tchi2\tdeviance\tmiss_reads\tmiss_fraction\tworst_segment\n");
    for (int32_t t = 0; t < r->n_tx; t++) {
        const double expected = fpkm[t] * den[t];
        fprintf(f, "%s\t%lf\t%lf\t%lf\t%lf\t%lf\t%lf\t", r->names[t], fpkm[t], df[t], chi2[t], dev[t], miss[t], expected != 0.0 ? miss[t] / expected : 0.0);
        if (worst_row[t] >= 0) fprintf(f, "c%d\n", worst_row[t]); else fprintf(f, "-\n");
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_gfit(const char *path, const emsar_rsh *r, const emsar_genes *g, const double *fpkm, const double *den, const double *df,
                     const double *chi2, const double *dev, const double *miss) {
    double *expected = (double *)calloc(g->n_genes > 0 ? (size_t)g->n_genes : 1, sizeof(double));
    if (!expected) return EMSAR_HOST_ERR_OOM;
    for (int32_t t = 0; t < r->n_tx; t++) if (g->gene_of_tx[t] >= 0) expected[g->gene_of_tx[t]] += fpkm[t] * den[t];
    FILE *f = fopen(path, "w");
    if (!f) { free(expected); return EMSAR_HOST_ERR_IO; }
    fprintf(f, "geneID\teff_segments\tchi2\tdeviance\tmiss_reads\tmiss_fraction\n");
    for (int32_t k = 0; k < g->n_genes; k++)
        fprintf(f, "%s\t%lf\t%lf\t%lf\t%lf\t%lf\n", g->names[k], df[k], chi2[k], dev[k], miss[k], expected[k] != 0.0 ? miss[k] / expected[k] : 0.0);
    free(expected);
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* The status words, one table per family of enums in include/emsar_hip.h; a file whose enum stops earlier uses the table's first words:
 * .profile the first 5 of the intervals' (.gprofile all 6), .compare the first 5 and .gcompare the first 6 of the two-sample tests'
 * (.ucompare all 8), .uprofile the 10 of the usage intervals', .groups the first 5 of the K-sample tests' (.ggroups all 6).  A number outside the file's range is written as "?". */
static const char *const presence_word[6] = {"TESTED", "ABSENT", "ESSENTIAL", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED"};
static const char *const interval_word[6] = {"TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE"};
static const char *const usage_interval_word[10] = {"TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE", "UPPER_ONE", "UNIT",
                                                    "UNDEFINED", "SINGLE"};
static const char *const two_sample_word[8] = {"TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE", "UNDEFINED", "SINGLE"};
static const char *const groups_word[6] = {"TESTED", "ALL_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE"};
static const char *const asym_word[5] = {"ESTIMATED", "BOUNDARY", "UNIDENTIFIABLE", "TOO_LARGE", "INFEASIBLE"};

static const char *status_word(const char *const *table, int n, int32_t v) { return v >= 0 && v < n ? table[v] : "?"; }

/* a value that may not be finite: fmt ("%lf" / "%.6g"), or the words nan / inf.  signed_inf = 0 for .presence, .profile, .asym and .gasym
 * and .uprofile (no sign: their Lambda, limits, shares and sd are not negative), 1 for .compare, .gcompare, .ucompare and .gprofile ("-inf") */
static void put_value(FILE *f, const char *fmt, double v, int signed_inf) {
    if (isnan(v)) fputs("nan", f); else if (isinf(v)) fputs(signed_inf && v < 0 ? "-inf" : "inf", f); else fprintf(f, fmt, v);
}

/* the number columns of a .compare, .gcompare, .ucompare or .gprofile line: n - 1 values "%lf" and the p-value "%.6g", tab-separated */
static void put_test_columns(FILE *f, int n, const double *v) {
    for (int k = 0; k < n; k++) { put_value(f, k + 1 < n ? "%lf" : "%.6g", v[k], 1); if (k + 1 < n) fputc('\t', f); }
}

int emsar_write_presence(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const double *fpkm, const double *lambda,
                         const double *pvalue, const int32_t *status, const int32_t *heir, const double *heir_share) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "tid\ttranscriptID\tFPKM\tLambda\tp\tstatus\their\their_share\n");
    if (!query) n_query = r->n_tx;
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i;
        fprintf(f, "%d\t%s\t%lf\t", t, r->names[t], fpkm[t]);
        put_value(f, "%lf", lambda[i], 0); fputc('\t', f);
        put_value(f, "%.6g", pvalue[i], 0);
        fprintf(f, "\t%s\t%s\t", status_word(presence_word, 6, status[i]), heir[i] >= 0 && heir[i] < r->n_tx ? r->names[heir[i]] : "-");
        put_value(f, "%lf", heir_share[i], 0); fputc('\n', f);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_profile(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const double *fpkm, const double *lower,
                        const double *upper, const double *lambda, const int32_t *status) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "tid\ttranscriptID\tFPKM\tlower\tupper\tLambda\tstatus\n");
    if (!query) n_query = r->n_tx;
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i;
        fprintf(f, "%d\t%s\t%lf\t", t, r->names[t], fpkm[t]);
        put_value(f, "%lf", lower[i], 0); fputc('\t', f);
        put_value(f, "%lf", upper[i], 0); fputc('\t', f);
        put_value(f, "%lf", lambda[i], 0);
        fprintf(f, "\t%s\n", status_word(interval_word, 5, status[i]));
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_gprofile(const char *path, const emsar_genes *g, const double *gfpkm, const double *lower, const double *upper, const double *lambda,
                         const double *pvalue, const int32_t *members, const int32_t *status) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "gene\tgFPKM\tlower\tupper\tLambda\tp\tmembers\tstatus\n");
    for (int32_t k = 0; k < g->n_genes; k++) {
        const double v[4] = {lower[k], upper[k], lambda[k], pvalue[k]};
        fprintf(f, "%s\t%lf\t", g->names[k], gfpkm[k]);
        put_test_columns(f, 4, v);
        fprintf(f, "\t%d\t%s\n", members[k], status_word(interval_word, 6, status[k]));
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_compare(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const double *fpkm_a, const double *fpkm_b,
                        const double *log2fc, const double *lambda, const double *pvalue, const int32_t *status, const int32_t *evals) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "tid\ttranscriptID\tFPKM\tFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\n");
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i;
        const double v[5] = {fpkm_a[i], fpkm_b[i], log2fc[i], lambda[i], pvalue[i]};
        fprintf(f, "%d\t%s\t", t, r->names[t]);
        put_test_columns(f, 5, v);
        fprintf(f, "\t%s\t%d\n", status_word(two_sample_word, 5, status[i]), evals[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_gcompare(const char *path, const emsar_genes *g, const double *gene_a, const double *gene_b, const double *log2fc, const double *lambda,
                         const double *pvalue, const int32_t *status, const int32_t *evals, const int32_t *parts) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "gene\tgFPKM\tgFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\tparts\n");
    for (int32_t k = 0; k < g->n_genes; k++) {
        const double v[5] = {gene_a[k], gene_b[k], log2fc[k], lambda[k], pvalue[k]};
        fprintf(f, "%s\t", g->names[k]);
        put_test_columns(f, 5, v);
        fprintf(f, "\t%s\t%d\t%d\n", status_word(two_sample_word, 6, status[k]), evals[k], parts[k]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_ucompare(const char *path, const emsar_rsh *r, const emsar_genes *g, int32_t n_query, const int32_t *query, const double *usage_a,
                         const double *usage_b, const double *dlogit, const double *lambda, const double *pvalue, const int32_t *status,
                         const int32_t *outer_evals, const int32_t *evals) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "transcript\tgene\tusage\tusage_ref\tdlogit\tLambda\tp\tstatus\touter\tevals\n");
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i, k = g->gene_of_tx[t];
        const double v[5] = {usage_a[i], usage_b[i], dlogit[i], lambda[i], pvalue[i]};
        fprintf(f, "%s\t%s\t", r->names[t], k >= 0 ? g->names[k] : "");
        put_test_columns(f, 5, v);
        fprintf(f, "\t%s\t%d\t%d\n", status_word(two_sample_word, 8, status[i]), outer_evals[i], evals[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* what .groups and .ggroups share: the "#" line, the header behind the name column (`value` = FPKM / gFPKM) and the number columns of a line */
static void put_groups_head(FILE *f, const char *name, const char *value, int32_t n_samples, int32_t G, const int32_t *group_of, const double *size,
                            const char *tail) {
    fprintf(f, "# samples=%d groups=", n_samples);
    for (int32_t k = 0; k < n_samples; k++) fprintf(f, "%s%d", k ? "," : "", group_of[k]);
    fprintf(f, " sizes=");
    for (int32_t k = 0; k < n_samples; k++) fprintf(f, "%s%g", k ? "," : "", size ? size[k] : 1.0);
    fprintf(f, " df_between=%d df_within=%d\n", G - 1, n_samples - G);
    fprintf(f, "%s\t%s_common", name, value);
    for (int32_t g = 0; g < G; g++) fprintf(f, "\t%s_g%d", value, g);
    fprintf(f, "\tLambda_between\tdf\tp_between\tLambda_within\tdf\tp_within\tstatus\touter\tevals%s\n", tail);
}
static void put_groups_columns(FILE *f, int32_t n_samples, int32_t G, double common, const double *group, double lambda_between, double p_between,
                               double lambda_within, double p_within) {
    put_value(f, "%lf", common, 1);
    for (int32_t g = 0; g < G; g++) { fputc('\t', f); put_value(f, "%lf", group[g], 1); }
    fputc('\t', f); put_value(f, "%lf", lambda_between, 1); fprintf(f, "\t%d\t", G - 1); put_value(f, "%.6g", p_between, 1);
    fputc('\t', f); put_value(f, "%lf", lambda_within, 1); fprintf(f, "\t%d\t", n_samples - G); put_value(f, "%.6g", p_within, 1);
}
static int32_t groups_count(int32_t n_samples, const int32_t *group_of) {
    int32_t G = 0;
    for (int32_t k = 0; k < n_samples; k++) if (group_of[k] + 1 > G) G = group_of[k] + 1;
    return G;
}

int emsar_write_groups(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, int32_t n_samples, const int32_t *group_of,
                       const double *size, const double *theta_common, const double *theta_group, const double *lambda_between, const double *p_between,
                       const double *lambda_within, const double *p_within, const int32_t *status, const int32_t *outer, const int32_t *evals) {
    const int32_t G = groups_count(n_samples, group_of);
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    put_groups_head(f, "transcript", "FPKM", n_samples, G, group_of, size, "");
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i;
        fprintf(f, "%s\t", r->names[t]);
        put_groups_columns(f, n_samples, G, theta_common[i], theta_group + (size_t)i * (size_t)G, lambda_between[i], p_between[i], lambda_within[i],
                           p_within[i]);
        fprintf(f, "\t%s\t%d\t%d\n", status_word(groups_word, 5, status[i]), outer[i], evals[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_ggroups(const char *path, const emsar_genes *g, int32_t n_samples, const int32_t *group_of, const double *size,
                        const double *gene_common, const double *gene_group, const double *lambda_between, const double *p_between,
                        const double *lambda_within, const double *p_within, const int32_t *status, const int32_t *outer, const int32_t *evals,
                        const int32_t *parts) {
    const int32_t G = groups_count(n_samples, group_of);
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    put_groups_head(f, "gene", "gFPKM", n_samples, G, group_of, size, "\tparts");
    for (int32_t k = 0; k < g->n_genes; k++) {
        fprintf(f, "%s\t", g->names[k]);
        put_groups_columns(f, n_samples, G, gene_common[k], gene_group + (size_t)k * (size_t)G, lambda_between[k], p_between[k], lambda_within[k],
                           p_within[k]);
        fprintf(f, "\t%s\t%d\t%d\t%d\n", status_word(groups_word, 6, status[k]), outer[k], evals[k], parts[k]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_uprofile(const char *path, const emsar_rsh *r, const emsar_genes *g, int32_t n_query, const int32_t *query, const double *usage,
                         const double *lower, const double *upper, const double *lambda_zero, const double *lambda_one, const int32_t *status,
                         const int32_t *outer_evals, const int32_t *evals) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "transcript\tgene\tusage\tlower\tupper\tLambda_zero\tLambda_one\tstatus\touter\tevals\n");
    if (!query) n_query = r->n_tx;
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i, k = g->gene_of_tx[t];
        const double v[5] = {usage[i], lower[i], upper[i], lambda_zero[i], lambda_one[i]};
        fprintf(f, "%s\t%s", r->names[t], k >= 0 ? g->names[k] : "");
        for (int c = 0; c < 5; c++) { fputc('\t', f); put_value(f, "%lf", v[c], 0); }
        fprintf(f, "\t%s\t%d\t%d\n", status_word(usage_interval_word, 10, status[i]), outer_evals[i], evals[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_asym(const char *path, const emsar_rsh *r, const double *fpkm, const double *tpm, const double *sd_fpkm, const double *sd_tpm,
                     const double *var, const int32_t *status, const int32_t *partner, const double *partner_cov, const double *usage_sd) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "tid\ttranscriptID\tFPKM\tsd_FPKM\tTPM\tsd_TPM\tstatus\tpartner\tpartner_corr%s\n", usage_sd ? "\tusage_sd" : "");
    for (int32_t t = 0; t < r->n_tx; t++) {
        const int32_t q = partner[t] >= 0 && partner[t] < r->n_tx ? partner[t] : -1;
        fprintf(f, "%d\t%s\t%lf\t", t, r->names[t], fpkm[t]);
        put_value(f, "%.6g", sd_fpkm[t], 0);
        fprintf(f, "\t%lf\t", tpm[t]);
        put_value(f, "%.6g", sd_tpm[t], 0);
        fprintf(f, "\t%s\t%s\t", status_word(asym_word, 5, status[t]), q >= 0 ? r->names[q] : "-");
        put_value(f, "%.6g", q >= 0 ? partner_cov[t] / sqrt(var[t] * var[q]) : NAN, 0);
        if (usage_sd) { fputc('\t', f); put_value(f, "%.6g", usage_sd[t], 0); }
        fputc('\n', f);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_gasym(const char *path, const emsar_genes *g, const double *gfpkm, const double *gene_sd, const int32_t *gene_status) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "geneID\tgFPKM\tsd\tstatus\n");
    for (int32_t k = 0; k < g->n_genes; k++) {
        fprintf(f, "%s\t%lf\t", g->names[k], gfpkm[k]);
        put_value(f, "%.6g", gene_sd[k], 0);
        fprintf(f, "\t%s\n", status_word(asym_word, 5, gene_status[k]));
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* the rows of .saturation / .gsaturation: n names, per fraction ncol columns col[j] = [n_fractions][n] */
static int write_saturation(const char *path, const char *id, char **names, int64_t n, const double *fpkm, const double *tpm, int n_fractions,
                            const double *fractions, int n_replicates, uint64_t seed, const double *depth_mean, int ncol,
                            const double *const *col, const char *const *colname) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "# fractions=");
    for (int k = 0; k < n_fractions; k++) fprintf(f, "%s%.17g", k ? "," : "", fractions[k]);
    fprintf(f, " replicates=%d seed=%llu depth_mean=", n_replicates, (unsigned long long)seed);
    for (int k = 0; k < n_fractions; k++) fprintf(f, "%s%lf", k ? "," : "", depth_mean[k]);
    fprintf(f, "\n%s\tFPKM\tTPM", id);
    for (int k = 0; k < n_fractions; k++)
        for (int j = 0; j < ncol; j++) fprintf(f, "\t%s@%.17g", colname[j], fractions[k]);
    fprintf(f, "\n");
    for (int64_t t = 0; t < n; t++) {
        fprintf(f, "%s\t%lf\t%lf", names[t], fpkm[t], tpm[t]);
        for (int k = 0; k < n_fractions; k++)
            for (int j = 0; j < ncol; j++) fprintf(f, "\t%lf", col[j][(int64_t)k * n + t]);
        fprintf(f, "\n");
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_saturation(const char *path, const emsar_rsh *r, const double *fpkm, const double *tpm, int n_fractions,
                           const double *fractions, int n_replicates, uint64_t seed, const double *depth_mean, const double *fpkm_mean,
                           const double *fpkm_sd, const double *tpm_mean, const double *tpm_sd) {
    const double *col[4] = {fpkm_mean, fpkm_sd, tpm_mean, tpm_sd};
    const char *name[4] = {"mean_FPKM", "sd_FPKM", "mean_TPM", "sd_TPM"};
    return write_saturation(path, "transcriptID", r->names, r->n_tx, fpkm, tpm, n_fractions, fractions, n_replicates, seed, depth_mean, 4, col, name);
}

int emsar_write_gsaturation(const char *path, const emsar_genes *g, const double *fpkm, const double *tpm, int n_fractions,
                            const double *fractions, int n_replicates, uint64_t seed, const double *depth_mean, const double *fpkm_mean,
                            const double *fpkm_sd, const double *tpm_mean) {
    const double *col[3] = {fpkm_mean, fpkm_sd, tpm_mean};
    const char *name[3] = {"mean_FPKM", "sd_FPKM", "mean_TPM"};
    return write_saturation(path, "geneID", g->names, g->n_genes, fpkm, tpm, n_fractions, fractions, n_replicates, seed, depth_mean, 3, col, name);
}

int emsar_write_fraglength(const char *path, const emsar_rsh *r, const emsar_counts *c, const emsar_model *m) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "Fragment.length\tObs.Counts\tnormalized.Fragment.length.sampling.prob\n");
    for (int i = 0; i < r->nfl; i++) {
        int fl = i + r->frag_min;
        fprintf(f, "%d\t%d\t%lg\n", fl, fl < c->n_frag ? c->frag_counts[fl] : 0, m->Wf[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

int emsar_write_segments(const char *path, const emsar_rsh *r, const emsar_counts *c, const emsar_model *m,
                         const double *mean_fpkm) {
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "segment_id\tsequence_sharing_set_id\ttranscript_id\ttranscript_names\teff.length\tReadcount\texpected_Readcount\n");
    const double nm = (double)c->total_reads / 1E6;
    for (int64_t cid = 0; cid < r->n_rows; cid++) {
        uint64_t b = r->row_ptr[cid], e = r->row_ptr[cid + 1];
        fprintf(f, "c%lld\ts%d\t", (long long)cid, m->CS[cid]);
        for (uint64_t k = b; k < e; k++) fprintf(f, "%st%d", k > b ? "," : "", r->col_idx[k]);
        fprintf(f, "\t");
        for (uint64_t k = b; k < e; k++) fprintf(f, "%s%s", k > b ? "+" : "", r->names[r->col_idx[k]]);
        fprintf(f, "\t%lf", m->L[cid]);
        double expc = 0;
        for (uint64_t k = b; k < e; k++) expc += mean_fpkm[r->col_idx[k]] * (m->L[cid] / 1E3) * nm;   /* 2295 */
        fprintf(f, "\t%d\t%f\n", c->R[cid], expc);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}
