/* emsar_host.h -- C host side of the MI355X EMSAR core (stays on the CPU by design: BASELINE north_star
 * "alignment parsing and rsh I/O untouched").  It re-states, on flat arrays, what the reference does between
 * reading its inputs and calling the solver, and what it prints afterwards:
 *
 *   rsh text reader           construct_rsh_from_rshfile      /root/reference/src/emsar_functions.c:1351-1510
 *   alignment readers         read_bowtie_SE/PE, read_BAM_* (SAM text and BAM)  emsar_functions.c:323-836
 *   per-read collapse         add_alignment_to_list + update_ReadCounts       alignment.c:29-95, emsar_functions.c:838-943
 *   fragment-length weights   transfer_fraglendist_to_Wf, compute_adjEUMA     emsar_functions.c:2503-2523
 *   row order (cid)           scan_rshbucket                                  emsar_functions.c:2135-2192
 *   connected sets            build_TC_from_CT_2, propagate_2, EUMAcut loop   emsar_functions.c:2201-2259, emsar_main.c:411-425
 *   EUMAps                    construct_EUMAps                                emsar_functions.c:3148-3154
 *   outputs                   print_FPKMfinal, print_FraglengthDist, print_aEUMA_3   emsar_functions.c:3163-3212, 2477-2493, 2262-2300
 *
 * Nothing here exits the process: functions return 0 or a negative code and fill a message buffer.
 */
#ifndef EMSAR_HOST_H
#define EMSAR_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMSAR_HOST_OK 0
#define EMSAR_HOST_ERR_IO (-1)
#define EMSAR_HOST_ERR_FORMAT (-2)
#define EMSAR_HOST_ERR_OOM (-3)
#define EMSAR_HOST_ERR_ARG (-4)

#define EMSAR_MAX_NTID_PER_SID 5000   /* emsar.h:17 */
#define EMSAR_EUMACUT_INCREMENT 2.0   /* emsar.h:18 */

typedef struct emsar_rsh {
    int32_t n_tx;            /* max_tid + 1 */
    char **names;            /* IndexTable: tid -> transcript name */
    int32_t hdr_minfrag, hdr_maxfrag, hdr_readlength, max_t_size;   /* header line "#max_tid,max_t_size,minfrag,maxfrag,readlength" */
    int32_t frag_min, frag_max, nfl;    /* Fraglengths after determine_fraglength_range (emsar_functions.c:2471-2475) */
    int64_t n_rows;          /* max_cid + 1 = n_tx single-tid rows + multi-tid rows, in cid order */
    uint64_t *row_ptr;       /* n_rows + 1 */
    int32_t *col_idx;        /* CT: tids of each row; a tid may repeat (internal repeats) */
    int32_t *euma;           /* n_rows * nfl effective position counts per fragment length (0 where absent) */
    uint8_t *has_node;       /* 0 for a single-tid row whose transcript has no unique region (no rsh node) */
    void *name_index;        /* opaque: name -> tid */
    void *set_index;         /* opaque: sorted tid multiset -> row */
} emsar_rsh;

int  emsar_rsh_read(const char *path, emsar_rsh **out, char *err, size_t errlen);
void emsar_rsh_free(emsar_rsh *r);
/* binary cache of the parsed arrays (a human PE rsh is gigabytes of text): write after a text parse, read instead of
 * one.  read_cache refuses a file that is not ours, is truncated or inconsistent, or -- when src_path is given -- was
 * made from a text of another size / mtime; the caller then parses the text. */
int  emsar_rsh_write_cache(const emsar_rsh *r, const char *src_path, const char *cache_path);
int  emsar_rsh_read_cache(const char *src_path /* may be NULL: no staleness check */, const char *cache_path, emsar_rsh **out,
                          char *err, size_t errlen);
int32_t emsar_rsh_tid_of(const emsar_rsh *r, const char *name);                 /* -1 if unknown */
int64_t emsar_rsh_row_of(const emsar_rsh *r, const int32_t *sorted_tids, int n); /* -1 if no such segment */

/* host thread budget of the parallel readers (hostutil.c): min(online cores, 16) by default; a caller that runs several
 * readers at once (emsar-hip -M: one worker per GPU) divides it; EMSAR_HOST_THREADS overrides both */
void emsar_host_set_thread_budget(int n);   /* 0 = default */
int  emsar_host_threads(void);

/* parallel BGZF inflate (pbgzf.c): NULL from open = not a seekable BGZF file, use zlib's gzread instead.
 * read returns the bytes delivered (< n only at the end of the file), -1 on a damaged block. */
struct emsar_pbgzf;
struct emsar_pbgzf *emsar_pbgzf_open(const char *path);
long emsar_pbgzf_read(struct emsar_pbgzf *p, void *dst, size_t n);
void emsar_pbgzf_close(struct emsar_pbgzf *p);
const char *emsar_pbgzf_engine(void);   /* "libdeflate" when libdeflate.so.0 could be loaded (EMSAR_HOST_INFLATE=zlib: never), else "zlib" */

/* Optional collapse of read-level rows OUTSIDE this library (emsar_hip_collapse_rows has exactly this signature behind a
 * context): rows with the same multiset of ids become one row with the number of members as its weight; ids sorted in the
 * output; the caller provides the three output arrays at worst-case size.  0 = ok. */
typedef int (*emsar_collapse_fn)(void *user, int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                                 int64_t *n_unique_out, uint64_t *row_ptr_out, int32_t *col_idx_out, int32_t *weight_out);

typedef struct {
    int pe;              /* -P */
    char strand;         /* library_strand_type: 0, '+', '-'  (set_library_strand_type, emsar_functions.c:16-22) */
    int max_repeat;      /* -k, default 100 */
    int format;          /* 0 default-bowtie text, 1 SAM text, 2 BAM */
    /* update_ReadCounts (emsar_functions.c:838-943) in two halves: the filters stay here, read by read; with `collapse` set, the
     * kept reads with two or more transcripts are not looked up one by one but gathered as read-level rows (sorted ids) and handed
     * to `collapse` in batches of `collapse_batch_rows`; only the UNIQUE rows that come back are looked up in the rsh, their
     * weights added to ReadCount.  Same counts as the per-read path, by construction.  NULL = per-read lookup.
     * Threading: the ranged / batched parsers flush from their worker threads; the library serialises the calls (one at a time,
     * process-wide), so the function need not be re-entrant -- but it may be entered from a thread other than the caller's. */
    emsar_collapse_fn collapse;
    void *collapse_user;
    int64_t collapse_batch_rows;     /* <= 0: 4M rows */
} emsar_aln_opts;

typedef struct {
    int64_t n_rows;
    int32_t *R;              /* ReadCount per row */
    int32_t n_frag;          /* hdr_maxfrag + 1 */
    int32_t *frag_counts;    /* FraglengthCounts[0..hdr_maxfrag] */
    int64_t total_reads;     /* TotalReadCount */
    int64_t reads_seen, reads_over_k, reads_bad_fraglen, reads_discrepant, reads_no_segment;   /* bookkeeping only */
    int32_t readlength;      /* PE: learnt from the data when the header says -1 */
    void *batch;             /* private: read-level rows waiting for emsar_aln_opts.collapse */
} emsar_counts;

int  emsar_set_strand(const char *strand_type, int pe, char *out);   /* "ns","ssf","ssr","ssfr","ssrf" */
int  emsar_count_alignments(const emsar_rsh *r, const char *path, const emsar_aln_opts *o, emsar_counts **out,
                            char *err, size_t errlen);
void emsar_counts_free(emsar_counts *c);

typedef struct {
    int64_t n_rows;
    int32_t n_tx, nfl;
    double *Wf;              /* nfl */
    double *L;               /* adjEUMA per row */
    double *E;               /* EUMAps per row */
    double *E_solver;        /* E with the rows left out of every set (CS == -1) zeroed: what the solver sees */
    int32_t *CS, *TS;        /* set id per row / per transcript (-1 = in no set) */
    int32_t n_sets;
    double eumacut;
} emsar_model;

/* eumacut_io persists across samples like the reference's global (never reset between -M samples). */
int  emsar_model_build(const emsar_rsh *r, const emsar_counts *c, int delta, double *eumacut_io, emsar_model **out,
                       char *err, size_t errlen);
/* the two halves separately, for callers that compute L_c = sum_i Wf[i] * EUMA_c[i] elsewhere (emsar_hip_adj_euma):
 * model_wf fills wf[nfl] (error if no read falls inside the fragment-length range); build_L takes L (NULL = host loop) */
int  emsar_model_wf(const emsar_rsh *r, const emsar_counts *c, double *wf);
int  emsar_model_build_L(const emsar_rsh *r, const emsar_counts *c, int delta, double *eumacut_io, const double *L,
                         emsar_model **out, char *err, size_t errlen);
void emsar_model_free(emsar_model *m);

/* mean/sd over rounds exactly as print_FPKMfinal does (sd = sqrt(sum sq/(n-1))/n; n = 1 gives NaN like the reference) */
void emsar_mean_sd(int32_t n_tx, int32_t n_round, const double *rounds, double *mean, double *sd);

int emsar_write_fpkm(const char *path, const emsar_rsh *r, const double *mean, const double *sd, const double *ieuma,
                     const double *ireadcount, const int32_t *ireadcount_int, const double *tpm, int64_t *total_ireadcount);
/* .bootstrap (emsar-hip --bootstrap): transcriptID FPKM boot.mean.FPKM boot.sd.FPKM TPM boot.sd.TPM, "%lf" like .fpkm */
int emsar_write_bootstrap(const char *path, const emsar_rsh *r, const double *fpkm, const double *boot_mean, const double *boot_sd,
                          const double *tpm, const double *boot_tpm_sd);
/* gene map of a g2t file (genes.c: util/FPKM2gFPKM.pl's rules, last line wins, unlisted transcripts in one gene with an empty ID;
 * plain or gzipped).  gene_of_tx[t] in 0 .. n_genes-1 for every index transcript; genes in order of first appearance in the file,
 * the empty-ID gene (if any transcript falls into it) last. */
typedef struct {
    int32_t n_genes, n_tx;
    char **names;            /* n_genes; "" = the gene of the transcripts the g2t does not list */
    int32_t *gene_of_tx;     /* n_tx */
    int64_t n_unknown;       /* g2t lines whose transcript is not in the index (ignored) */
    int32_t n_unmapped;      /* index transcripts in the empty-ID gene */
} emsar_genes;
int  emsar_genes_read(const emsar_rsh *r, const char *g2t_path, emsar_genes **out, char *err, size_t errlen);
void emsar_genes_free(emsar_genes *g);

/* .gfpkm (emsar-hip --g2t): FPKM2gFPKM.pl's header and columns, "%s\t%lf\t%lf\t%d\t%lf\n"; iReadcount.int is the script's half-up
 * roundoff of the gene's iReadcount.  Per-gene arrays of n_genes. */
int emsar_write_gfpkm(const char *path, const emsar_genes *g, const double *fpkm, const double *ireadcount, const double *tpm);
/* .gbootstrap (emsar-hip --g2t --bootstrap): the columns of .bootstrap per gene */
int emsar_write_gbootstrap(const char *path, const emsar_genes *g, const double *fpkm, const double *boot_mean, const double *boot_sd,
                           const double *tpm, const double *boot_tpm_sd);
/* .bootq / .gbootq (emsar-hip --bootstrap B --bootstrap-quantiles q1,..): name, then the quantiles of FPKM at each q, then of TPM at each
 * q over the bootstrap replicates ([n_q][n_tx] / [n_q][n_genes] each), "%lf"; the header names the probabilities */
int emsar_write_bootq(const char *path, const emsar_rsh *r, int n_q, const double *q, const double *fpkm_q, const double *tpm_q);
int emsar_write_gbootq(const char *path, const emsar_genes *g, int n_q, const double *q, const double *fpkm_q, const double *tpm_q);
/* .isoforms (emsar-hip --g2t --isoforms): one line per transcript that is in a gene (gene_of_tx >= 0), in the order of .fpkm:
 * transcript_ID gene_ID FPKM usage dominant, "%s\t%s\t%lf\t%lf\t%d"; usage [n_tx] and dominant [n_genes] (tid of the gene's dominant
 * isoform or -1) as emsar_hip_isoform_usage returns them for fpkm.  n_boot > 0 (--bootstrap B) adds usage_mean usage_sd dominant_freq
 * (= dominant_count / n_boot), n_q > 0 as well (--bootstrap-quantiles) one usage_q<q> column per probability (usage_q [n_q][n_tx]),
 * all "%lf".  With n_boot == 0 the bootstrap arguments are not read. */
int emsar_write_isoforms(const char *path, const emsar_rsh *r, const emsar_genes *g, const double *fpkm, const double *usage,
                         const int32_t *dominant, int n_boot, const double *usage_mean, const double *usage_sd,
                         const int32_t *dominant_count, int n_q, const double *q, const double *usage_q);
/* .fit (emsar-hip --fit): one line per transcript, in the order of .fpkm: transcriptID FPKM eff_segments chi2 deviance miss_reads
 * miss_fraction worst_segment, "%s\t%lf\t%lf\t%lf\t%lf\t%lf\t%lf\t%s"; the four sums and worst_row [n_tx] as emsar_hip_model_fit returns them for
 * fpkm; miss_fraction = miss / (fpkm * den), the missed share of the transcript's expected reads, 0 when that product is 0; worst_segment =
 * "c<row>", the id .segments uses, or "-" */
int emsar_write_fit(const char *path, const emsar_rsh *r, const double *fpkm, const double *den, const double *df, const double *chi2,
                    const double *dev, const double *miss, const int32_t *worst_row);
/* .gfit (with --g2t): per gene, in the order of .gfpkm: geneID eff_segments chi2 deviance miss_reads miss_fraction, the gene sums [n_genes] of
 * the four columns; miss_fraction = miss / the sum of fpkm * den over the gene's transcripts in ascending tid, 0 when that sum is 0 */
int emsar_write_gfit(const char *path, const emsar_rsh *r, const emsar_genes *g, const double *fpkm, const double *den, const double *df,
                     const double *chi2, const double *dev, const double *miss);
/* .presence (emsar-hip --presence): one line per queried transcript -- query [n_query] tids, NULL = all n_tx in order; the result arrays are
 * [n_query] as emsar_hip_presence returns them, fpkm is [n_tx] --: tid transcriptID FPKM Lambda p status heir heir_share,
 * "%d\t%s\t%lf\t%lf\t%.6g\t%s\t%s\t%lf"; status is the word of the header's enum (TESTED, ABSENT, ESSENTIAL, OUTSIDE, NOT_RESIDENT,
 * UNCONVERGED), heir the heir's transcriptID or "-"; a value that is not finite is written as "inf" or "nan" */
int emsar_write_presence(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const double *fpkm, const double *lambda,
                         const double *pvalue, const int32_t *status, const int32_t *heir, const double *heir_share);

/* .profile (emsar-hip --profile): one line per queried transcript, query and arrays as for .presence, the arrays as emsar_hip_profile returns
 * them --: tid transcriptID FPKM lower upper Lambda status, "%d\t%s\t%lf\t%lf\t%lf\t%lf\t%s"; status is the word of the header's enum
 * (TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED); a value that is not finite is written as "inf" or "nan" */
int emsar_write_profile(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const double *fpkm, const double *lower,
                        const double *upper, const double *lambda, const int32_t *status);
/* .gprofile (emsar-hip --profile --g2t): one line per gene in the order of .gfpkm -- gene gFPKM lower upper Lambda p members status; the
 * arrays are [n_genes] as emsar_hip_profile_genes returns them for every gene, gfpkm the FPKM column of .gfpkm; the status words of .profile
 * and TOO_LARGE; numbers "%lf", p "%.6g", a value that is not finite "nan", "inf" or "-inf" */
int emsar_write_gprofile(const char *path, const emsar_genes *g, const double *gfpkm, const double *lower, const double *upper, const double *lambda,
                         const double *pvalue, const int32_t *members, const int32_t *status);
/* .uprofile (emsar-hip --profile-usage --g2t): one line per queried transcript, query as for .profile -- transcript gene usage lower upper
 * Lambda_zero Lambda_one status outer evals; the arrays as emsar_hip_profile_usage returns them; the gene field of a transcript in no gene is
 * empty; the status words of .gprofile and UPPER_ONE, UNIT, UNDEFINED, SINGLE; numbers "%lf", a value that is not finite "nan" or "inf" */
int emsar_write_uprofile(const char *path, const emsar_rsh *r, const emsar_genes *g, int32_t n_query, const int32_t *query, const double *usage,
                         const double *lower, const double *upper, const double *lambda_zero, const double *lambda_one, const int32_t *status,
                         const int32_t *outer_evals, const int32_t *evals);

/* The two-sample files (emsar-hip -M --compare / --compare-usage, every sample i >= 1 against sample 0); numbers, p and values that are
 * not finite as in .gprofile; the arrays as emsar_hip_compare, _compare_genes and _compare_usage return them.
 * .compare: one line per queried transcript (query [n_query] tids, NULL = 0 .. n_query-1) -- tid transcriptID FPKM FPKM_ref log2FC Lambda p
 * status evals; status TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT or UNCONVERGED */
int emsar_write_compare(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const double *fpkm_a, const double *fpkm_b,
                        const double *log2fc, const double *lambda, const double *pvalue, const int32_t *status, const int32_t *evals);
/* .gcompare (with --g2t): one line per gene in the order of .gfpkm -- gene gFPKM gFPKM_ref log2FC Lambda p status evals parts; also TOO_LARGE */
int emsar_write_gcompare(const char *path, const emsar_genes *g, const double *gene_a, const double *gene_b, const double *log2fc, const double *lambda,
                         const double *pvalue, const int32_t *status, const int32_t *evals, const int32_t *parts);
/* .ucompare: one line per queried transcript, query as for .compare -- transcript gene usage usage_ref dlogit Lambda p status outer evals; the
 * gene field of a transcript in no gene (gene_of_tx < 0) is empty; also TOO_LARGE, UNDEFINED and SINGLE */
int emsar_write_ucompare(const char *path, const emsar_rsh *r, const emsar_genes *g, int32_t n_query, const int32_t *query, const double *usage_a,
                         const double *usage_b, const double *dlogit, const double *lambda, const double *pvalue, const int32_t *status,
                         const int32_t *outer_evals, const int32_t *evals);

/* .groups (emsar-hip -M --compare-groups; one file per job, <prefix>.groups): a "#" line (samples, the group of every sample, the size
 * factors -- size NULL: all 1 --, the two degrees of freedom), a header, then one line per queried transcript, query as for .compare --
 * transcript FPKM_common FPKM_g0 .. FPKM_g(G-1) Lambda_between df p_between Lambda_within df p_within status outer evals; G = the largest
 * group id + 1, theta_group [n_query][G]; the arrays as emsar_hip_compare_groups returns them; numbers, p and values that are not finite
 * as in .compare; status TESTED, ALL_ABSENT, OUTSIDE, NOT_RESIDENT or UNCONVERGED */
int emsar_write_groups(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, int32_t n_samples, const int32_t *group_of,
                       const double *size, const double *theta_common, const double *theta_group, const double *lambda_between, const double *p_between,
                       const double *lambda_within, const double *p_within, const int32_t *status, const int32_t *outer, const int32_t *evals);
/* .ggroups (with --g2t; one file per job, <prefix>.ggroups): .groups' "#" line, then one line per gene in the order of .gfpkm -- gene
 * gFPKM_common gFPKM_g0 .. gFPKM_g(G-1) Lambda_between df p_between Lambda_within df p_within status outer evals parts; gene_group [n_genes][G];
 * the arrays as emsar_hip_compare_groups_genes returns them for every gene; number formats as in .groups; also TOO_LARGE */
int emsar_write_ggroups(const char *path, const emsar_genes *g, int32_t n_samples, const int32_t *group_of, const double *size,
                        const double *gene_common, const double *gene_group, const double *lambda_between, const double *p_between,
                        const double *lambda_within, const double *p_within, const int32_t *status, const int32_t *outer, const int32_t *evals,
                        const int32_t *parts);

/* .asym (emsar-hip --asymptotic): one line per transcript -- tid transcriptID FPKM sd_FPKM TPM sd_TPM status partner partner_corr, and
 * usage_sd when it is given (--g2t); the arrays are [n_tx] as emsar_hip_asymptotic returns them.  partner_corr = partner_cov /
 * sqrt(var_t * var_partner); "-" and nan where there is no partner.  sd values are written "%.6g", or the words inf / nan.
 * .gasym: one line per gene -- geneID gFPKM sd status. */
int emsar_write_asym(const char *path, const emsar_rsh *r, const double *fpkm, const double *tpm, const double *sd_fpkm, const double *sd_tpm,
                     const double *var, const int32_t *status, const int32_t *partner, const double *partner_cov, const double *usage_sd);
int emsar_write_gasym(const char *path, const emsar_genes *g, const double *gfpkm, const double *gene_sd, const int32_t *gene_status);

/* .saturation (emsar-hip --subsample): a "#" line (fractions, replicates, seed, depth_mean per fraction), a header, then per
 * transcript its name, FPKM and TPM as in .fpkm and per fraction mean_FPKM sd_FPKM mean_TPM sd_TPM ([n_fractions][n_tx] each) */
int emsar_write_saturation(const char *path, const emsar_rsh *r, const double *fpkm, const double *tpm, int n_fractions,
                           const double *fractions, int n_replicates, uint64_t seed, const double *depth_mean, const double *fpkm_mean,
                           const double *fpkm_sd, const double *tpm_mean, const double *tpm_sd);
/* .gsaturation (with --g2t): per gene FPKM and TPM as in .gfpkm and per fraction mean_FPKM sd_FPKM mean_TPM ([n_fractions][n_genes]) */
int emsar_write_gsaturation(const char *path, const emsar_genes *g, const double *fpkm, const double *tpm, int n_fractions,
                            const double *fractions, int n_replicates, uint64_t seed, const double *depth_mean, const double *fpkm_mean,
                            const double *fpkm_sd, const double *tpm_mean);
int emsar_write_fraglength(const char *path, const emsar_rsh *r, const emsar_counts *c, const emsar_model *m);
int emsar_write_segments(const char *path, const emsar_rsh *r, const emsar_counts *c, const emsar_model *m,
                         const double *mean_fpkm);

#ifdef __cplusplus
}
#endif
#endif
