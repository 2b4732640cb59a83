/* emsar_hip_main.c -- command-line driver: the per-sample loop of the reference's main()
 * (/root/reference/src/emsar_main.c:380-488) with run_MLE_threads() replaced by the HIP library.
 *
 *   emsar-hip [options] -I index.rsh outdir outprefix alignmentfile            (single sample)
 *   emsar-hip [options] -M -I index.rsh outdir outprefix alignmentfilelist     (one alignment file per line)
 *
 * Same option letters as the reference for everything that reaches this path (emsar_main.c:100-214):
 *   -I rsh  -P  -s strand  -k max_repeat  -n rounds  -e tol  -i max_passes  -d delta  -g  -M  -S  -B  -q  -v  -p threads(ignored)
 * plus  --gpus N (devices used by -M, default all), --devices a,b,.. (one -M worker per entry; an id may repeat, so that
 *       several workers share one card), --device D (single sample), --plain (no SQUAREM), --stats-json FILE.
 * Not taken over: -x fasta (index build, emsar-build's job), -m positional bias
 * (unfinished in the reference, emsar_main.c:371), -F/-f (the reference overwrites both from the rsh header,
 * emsar_functions.c:1419-1420, so they have no effect with -I).
 *
 * Outputs: <outdir>/<prefix>.<i>.fpkm, .fraglength_effect and, with -g, .segments -- i = 0-based index of the
 * alignment file (emsar_main.c:459-469).  Column 3 (sd.of.FPKM) is 0: the EM is deterministic, the reference's
 * spread comes from its random restarts (documented deviation).  For an uncertainty measure,
 * --bootstrap B writes <prefix>.<i>.bootstrap: mean and sd of FPKM and sd of TPM over B Poisson bootstrap replicates
 * (emsar_hip_bootstrap; seed --bootstrap-seed + i).  .fpkm, .fraglength_effect and .segments do not change with it.
 * --g2t FILE adds the reference's gene step (util/FPKM2gFPKM.pl, run by util/post_processing.pl): <prefix>.<i>.gfpkm, the per-gene
 * sums of FPKM, iReadcount and TPM (emsar_hip_gene_sums; the map is read once, genes.c), which merge_gTPM.pl / merge_gReadcount.pl
 * read as they are; with --bootstrap also <prefix>.<i>.gbootstrap, the genes' bootstrap mean and sd from the same replicates
 * (emsar_hip_bootstrap_genes).  The other files are the same bytes with and without it.
 * --bootstrap-quantiles q1,q2,.. (needs --bootstrap B, B <= 4096) adds percentile intervals: <prefix>.<i>.bootq holds, per transcript, the
 * q-quantiles of FPKM and then of TPM over the same B replicates (emsar_hip_bootstrap_quantiles: q = 0.025,0.5,0.975 gives the 95 %
 * percentile interval and the median), with --g2t also <prefix>.<i>.gbootq per gene.  The other files are the same bytes with and without it.
 * --isoforms (needs --g2t) adds the isoform usage: <prefix>.<i>.isoforms holds, per transcript that is in a gene, its gene, its FPKM, its share
 * of the gene's FPKM and whether it is the gene's dominant isoform (emsar_hip_isoform_usage on the .fpkm column); with --bootstrap B also the
 * mean and sd of that share and how often the transcript dominates over the same B replicates, with --bootstrap-quantiles also the share's
 * quantiles (emsar_hip_bootstrap_isoforms, which gives the other bootstrap files the same bytes).  The other files do not change with it.
 * --fit answers "does the fitted model explain the reads": <prefix>.<i>.fit holds, per transcript, its FPKM, the effective number of segments
 * attributed to it, the Pearson chi2, the Poisson deviance and the missed reads of those segments (each segment's residual shared out by
 * theta_t / S_c), the missed share of its expected reads and the segment that misses most, by the id .segments uses (emsar_hip_model_fit on
 * the .fpkm column and the E of the solve); with --g2t also <prefix>.<i>.gfit per gene.  The other files do not change with it.
 * --presence answers "is this isoform needed to explain the reads at all": <prefix>.<i>.presence holds, per transcript (or per transcript named in
 * --presence-list FILE, one name per line), the likelihood-ratio statistic Lambda of dropping it from its connected set, its p-value, a status
 * word and the sibling that would take over its reads (emsar_hip_presence with the solve's parameters).  The other files do not change with it.
 * --profile answers "how much of this isoform could be present": <prefix>.<i>.profile holds, per transcript (or per transcript named in
 * --profile-list FILE), the limits of its profile-likelihood interval at --profile-level (0.95) in the units of the FPKM column, the
 * presence test's Lambda and a status word (emsar_hip_profile with the solve's parameters).  The interval is one-sided by itself where the
 * transcript cannot be told from absent, FPKM 0 included.  With --g2t also <prefix>.<i>.gprofile: per gene, in the order of .gfpkm, its gFPKM,
 * the limits of the profile-likelihood interval of the gene's total (the isoforms free), the gene presence test's Lambda, the p-value bound
 * P(chi2_members > Lambda), the members taking part and a status word (emsar_hip_profile_genes; --profile-list filters transcripts only).  The
 * other files do not change with it.
 * --compare (with -M and at least two samples) answers "does this isoform's abundance differ from sample 0": every sample i >= 1 writes
 * <prefix>.<i>.compare with, per transcript (or per transcript named in --compare-list FILE), its FPKM in sample i and in sample 0, log2 of their
 * ratio, the likelihood-ratio statistic Lambda of H0: theta_i = r * theta_0 (--compare-ratio r, default 1) with every sibling free in both samples,
 * its chi2_1 p-value, a status word and the evaluations spent (emsar_hip_compare with the solve's parameters: sample i is A, sample 0 is B).
 * Sample 0's solver inputs (R, E, den) are kept on the host and uploaded into a second context on each worker's device.  With --g2t every
 * sample i >= 1 also writes <prefix>.<i>.gcompare: per gene, in the order of .gfpkm, the gene sums of FPKM in sample i and in sample 0, log2 of
 * their ratio, Lambda of H0: the gene's sum in i = r * its sum in 0 with the isoforms free in both samples, p, status, evaluations and parts
 * (emsar_hip_compare_genes); --compare-list filters transcripts only.  The other files do not change with it.
 * --compare-usage (with -M, at least two samples and --g2t) answers "did this isoform's share of its gene change against sample 0" (an
 * isoform switch): every sample i >= 1 writes <prefix>.<i>.ucompare with, per transcript (or per transcript named in --compare-list FILE), its
 * gene, its share of the gene in sample i and in sample 0, the difference of their logits, the likelihood-ratio statistic Lambda of H0: equal
 * shares, its chi2_1 p-value, a status word, the outer points and the inner evaluations spent (emsar_hip_compare_usage with the solve's
 * parameters: sample i is A, sample 0 is B).  The other files do not change with it.
 * --asymptotic answers "how sure is this FPKM" without resampling: <prefix>.<i>.asym holds, per transcript, the standard errors of FPKM and
 * TPM from the inverse of the observed information at the .fpkm column (emsar_hip_asymptotic), a status word and the sibling it is most
 * confounded with; with --g2t also <prefix>.<i>.gasym per gene and a usage_sd column.  Transcripts with FPKM <= --boundary-cut (5e-7) are held
 * fixed: the normal approximation does not hold there, --bootstrap is the tool.  The other files do not change with it.
 * --subsample f1,f2,.. answers "was the sample sequenced deep enough": <prefix>.<i>.saturation holds, per transcript and fraction,
 * the mean and sd of FPKM (at the thinned depth) and TPM over --subsample-reps replicates in which every read is kept with
 * probability f (emsar_hip_subsample; seed --subsample-seed + i), with --g2t also <prefix>.<i>.gsaturation per gene.  The other
 * files are the same bytes with and without it.
 *
 * -M: samples are independent (emsar_main.c:380-488 resets every count per file), so sample i runs on GPU
 * i mod G with one host thread per GPU; no collective.  The only cross-sample state of the reference, EUMAcut
 * (never reset, emsar_main.c:95,418), is carried in sample order.
 */
#include <getopt.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <errno.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "../../../include/emsar_hip.h"
#include "emsar_host.h"

typedef struct {
    const char *rsh_path, *outdir, *prefix;
    char **aln; int n_aln;
    emsar_aln_opts ao;
    int n_round, delta, print_segments, verbose, accel, set_mode, device_collapse, no_deterministic;
    double tol, count_floor, zero_cut, abs_step; int max_iter;
    const char *stats_json;
    const char *rsh_cache;      /* NULL = off, "" = <rsh>.bin, else the path */
    int boot_n; uint64_t boot_seed;   /* --bootstrap B (0 = off), --bootstrap-seed: sample i uses seed + i */
    int bq_n; double bq[64];          /* --bootstrap-quantiles q1,.. (0 = off) */
    int sub_nf, sub_reps; double sub_f[64]; uint64_t sub_seed;   /* --subsample f1,.. (0 = off), --subsample-reps, --subsample-seed: sample i uses seed + i */
    const char *g2t;                  /* --g2t FILE (NULL = off) */
    int isoforms;                     /* --isoforms (needs --g2t) */
    int fit;                          /* --fit */
    int presence;                     /* --presence */
    int asymptotic; double boundary_cut;   /* --asymptotic [--boundary-cut X] */
    int32_t *pres_q; int pres_nq;     /* --presence-list FILE: the tids it names, in file order (NULL = all transcripts) */
    int profile, profile_evals; double profile_level; /* --profile [--profile-level L] [--profile-evals N] */
    int32_t *prof_q; int prof_nq;     /* --profile-list FILE, as --presence-list */
    int compare; double compare_ratio; /* --compare [--compare-ratio r] */
    int compare_usage;                /* --compare-usage (needs --g2t): also a two-sample run, shares sample 0 with --compare */
    int32_t *cmp_q; int cmp_nq;       /* --compare-list FILE, as --presence-list */
    struct compare_ref *ref;          /* --compare: sample 0's solver inputs, shared by the workers */
    const emsar_genes *genes;         /* its gene map, read once by main() and shared read-only by the workers */
} config;

/* --compare: what sample 0 was solved from, published once by the worker that runs it (under the workers' mutex; ready: 0 = not yet,
 * 1 = the arrays stand, -1 = sample 0 failed before it had them) and read by every other sample */
typedef struct compare_ref { int ready; int32_t *R; double *E, *den; } compare_ref;

typedef struct {
    config *cfg; const emsar_rsh *rsh;
    int device, n_workers, worker;
    /* ordered hand-over of EUMAcut between samples */
    pthread_mutex_t *mu; pthread_cond_t *cv; int *next_model; double *eumacut;
    int *status;          /* per sample */
    emsar_em_stats *stats; /* per sample */
    emsar_boot_stats *bstats; /* per sample (--bootstrap) */
    emsar_subsample_stats *sstats; /* per sample (--subsample) */
    emsar_quantile_stats *qstats; /* per sample (--bootstrap-quantiles) */
    double *parse_s;
    double *model_s, *host_s;   /* per sample: model preparation, and all host work of run_sample outside the library calls */
    int *go;              /* start gate: the workers wait until main() knows how many of them exist */
    emsar_aln_opts ao;    /* the job's alignment options, plus this worker's collapse device when --device-collapse */
    struct { emsar_hip_ctx *ctx; pthread_mutex_t mu; } cdev;
    emsar_hip_ctx *ref_ctx; /* --compare: sample 0 in a second context on this worker's device, made on first use */
} worker_arg;

/* --compare: sample 0's inputs for the other samples (NULL arrays: it failed) */
static void publish_ref(worker_arg *w, const emsar_rsh *r, const int32_t *R, const double *E, const double *den) {
    compare_ref *ref = w->cfg->ref;
    const size_t nr = (size_t)(r->n_rows > 0 ? r->n_rows : 1), nt = (size_t)(r->n_tx > 0 ? r->n_tx : 1);
    int32_t *cR = R ? (int32_t *)malloc(nr * 4) : NULL;
    double *cE = R ? (double *)malloc(nr * 8) : NULL, *cd = R ? (double *)malloc(nt * 8) : NULL;
    const int ok = cR && cE && cd;
    if (ok) { memcpy(cR, R, (size_t)r->n_rows * 4); memcpy(cE, E, (size_t)r->n_rows * 8); memcpy(cd, den, (size_t)r->n_tx * 8); }
    else { free(cR); free(cE); free(cd); cR = NULL; cE = cd = NULL; }
    pthread_mutex_lock(w->mu);
    ref->R = cR; ref->E = cE; ref->den = cd; ref->ready = ok ? 1 : -1;
    pthread_cond_broadcast(w->cv);
    pthread_mutex_unlock(w->mu);
}

/* .compare: one line per queried transcript -- tid transcriptID FPKM FPKM_ref log2FC Lambda p status evals; a value that is not finite is
 * written as "inf", "-inf" or "nan" */
static void put_num(FILE *f, const char *fmt, double v) {
    if (isnan(v)) fputs("nan", f); else if (isinf(v)) fputs(v > 0 ? "inf" : "-inf", f); else fprintf(f, fmt, v);
}
static int write_compare(const char *path, const emsar_rsh *r, int32_t n_query, const int32_t *query, const emsar_compare_outputs *o) {
    static const char *const word[5] = {"TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED"};
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "tid\ttranscriptID\tFPKM\tFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\n");
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i;
        fprintf(f, "%d\t%s\t", t, r->names[t]);
        put_num(f, "%lf", o->theta_a[i]); fputc('\t', f);
        put_num(f, "%lf", o->theta_b[i]); fputc('\t', f);
        put_num(f, "%lf", o->log2fc[i]); fputc('\t', f);
        put_num(f, "%lf", o->lambda[i]); fputc('\t', f);
        put_num(f, "%.6g", o->pvalue[i]);
        fprintf(f, "\t%s\t%d\n", o->status[i] >= 0 && o->status[i] < 5 ? word[o->status[i]] : "?", o->evals[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* .gcompare (--compare --g2t): one line per gene in the order of .gfpkm -- gene gFPKM gFPKM_ref log2FC Lambda p status evals parts; numbers
 * as in .compare */
static int write_gcompare(const char *path, const emsar_genes *g, const emsar_compare_gene_outputs *o) {
    static const char *const word[6] = {"TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE"};
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "gene\tgFPKM\tgFPKM_ref\tlog2FC\tLambda\tp\tstatus\tevals\tparts\n");
    for (int32_t k = 0; k < g->n_genes; k++) {
        fprintf(f, "%s\t", g->names[k]);
        put_num(f, "%lf", o->gene_a[k]); fputc('\t', f);
        put_num(f, "%lf", o->gene_b[k]); fputc('\t', f);
        put_num(f, "%lf", o->log2fc[k]); fputc('\t', f);
        put_num(f, "%lf", o->lambda[k]); fputc('\t', f);
        put_num(f, "%.6g", o->pvalue[k]);
        fprintf(f, "\t%s\t%d\t%d\n", o->status[k] >= 0 && o->status[k] < 6 ? word[o->status[k]] : "?", o->evals[k], o->parts[k]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* .ucompare (--compare-usage): one line per queried transcript -- transcript gene usage usage_ref dlogit Lambda p status outer evals; numbers
 * as in .compare */
static int write_ucompare(const char *path, const emsar_rsh *r, const emsar_genes *g, int32_t n_query, const int32_t *query, const emsar_usage_outputs *o) {
    static const char *const word[8] = {"TESTED", "BOTH_ABSENT", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE", "UNDEFINED", "SINGLE"};
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "transcript\tgene\tusage\tusage_ref\tdlogit\tLambda\tp\tstatus\touter\tevals\n");
    for (int32_t i = 0; i < n_query; i++) {
        const int32_t t = query ? query[i] : i, k = g->gene_of_tx[t];
        fprintf(f, "%s\t%s\t", r->names[t], k >= 0 ? g->names[k] : "");
        put_num(f, "%lf", o->usage_a[i]); fputc('\t', f);
        put_num(f, "%lf", o->usage_b[i]); fputc('\t', f);
        put_num(f, "%lf", o->dlogit[i]); fputc('\t', f);
        put_num(f, "%lf", o->lambda[i]); fputc('\t', f);
        put_num(f, "%.6g", o->pvalue[i]);
        fprintf(f, "\t%s\t%d\t%d\n", o->status[i] >= 0 && o->status[i] < 8 ? word[o->status[i]] : "?", o->outer_evals[i], o->evals[i]);
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* .gprofile (--profile --g2t): one line per gene in the order of .gfpkm -- gene gFPKM lower upper Lambda p members status; numbers as in
 * .profile, p as in .compare */
static int write_gprofile(const char *path, const emsar_genes *g, const double *gfpkm, const emsar_profile_gene_outputs *o) {
    static const char *const word[6] = {"TWO_SIDED", "LOWER_ZERO", "OUTSIDE", "NOT_RESIDENT", "UNCONVERGED", "TOO_LARGE"};
    FILE *f = fopen(path, "w");
    if (!f) return EMSAR_HOST_ERR_IO;
    fprintf(f, "gene\tgFPKM\tlower\tupper\tLambda\tp\tmembers\tstatus\n");
    for (int32_t k = 0; k < g->n_genes; k++) {
        fprintf(f, "%s\t%lf\t", g->names[k], gfpkm[k]);
        put_num(f, "%lf", o->lower[k]); fputc('\t', f);
        put_num(f, "%lf", o->upper[k]); fputc('\t', f);
        put_num(f, "%lf", o->lambda[k]); fputc('\t', f);
        put_num(f, "%.6g", o->pvalue[k]);
        fprintf(f, "\t%d\t%s\n", o->members[k], o->status[k] >= 0 && o->status[k] < 6 ? word[o->status[k]] : "?");
    }
    return fclose(f) == 0 ? EMSAR_HOST_OK : EMSAR_HOST_ERR_IO;
}

/* emsar_aln_opts.collapse on the GPU (--device-collapse): the parse threads of a worker hand their read-level rows to a context
 * of their own on the worker's device (the solve context is busy with the sample before); one call at a time */
static int cli_collapse(void *user, int64_t n_rows, int32_t n_tx, const uint64_t *row_ptr, const int32_t *col_idx,
                        int64_t *n_unique, uint64_t *row_ptr_out, int32_t *col_idx_out, int32_t *weight_out) {
    worker_arg *w = (worker_arg *)user;
    pthread_mutex_lock(&w->cdev.mu);
    const int rc = emsar_hip_collapse_rows(w->cdev.ctx, n_rows, n_tx, row_ptr, col_idx, NULL, n_unique, row_ptr_out, col_idx_out, weight_out, NULL, NULL);
    pthread_mutex_unlock(&w->cdev.mu);
    return rc;
}

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

/* The alignments of a sample are counted on a thread of their own: the first sample of a worker while its GPU context, the
 * device layout and the EUMA table are being set up, every later one while the sample before it is being solved. */
typedef struct { worker_arg *w; int i; emsar_counts *cnt; int rc; char err[512]; double secs; pthread_t th; int started; } parse_job;
static void *parse_main(void *a) {
    parse_job *j = (parse_job *)a;
    double t0 = now_s();
    j->rc = emsar_count_alignments(j->w->rsh, j->w->cfg->aln[j->i], &j->w->ao, &j->cnt, j->err, sizeof j->err);
    j->secs = now_s() - t0;
    return NULL;
}
static void parse_start(parse_job *j, worker_arg *w, int i) {
    memset(j, 0, sizeof *j);
    j->w = w; j->i = i;
    if (pthread_create(&j->th, NULL, parse_main, j) == 0) j->started = 1;
}
static void parse_wait(parse_job *j) {
    if (j->started) { pthread_join(j->th, NULL); j->started = 0; }
    else if (j->w) parse_main(j);                                    /* no thread to be had: count here */
    j->w = NULL;
}

static int run_sample(worker_arg *w, emsar_hip_ctx *ctx, int i, parse_job *parsed) {
    config *cfg = w->cfg; const emsar_rsh *r = w->rsh;
    char err[512] = "", path[4096];
    emsar_counts *cnt = parsed->cnt; emsar_model *m = NULL;
    double *theta = NULL, *rounds = NULL, *mean = NULL, *sd = NULL, *ieuma = NULL, *tpm = NULL, *ir = NULL, *den = NULL; int32_t *iri = NULL;
    double *gcols = NULL, *gsums = NULL;     /* --g2t: [3][n_tx] FPKM, iReadcount, TPM and their [3][n_genes] gene sums */
    double *iso_u = NULL; int32_t *dom = NULL;   /* --isoforms: [n_tx] usage and [n_genes] dominant isoform of the .fpkm column */
    int rc = parsed->rc, published = 0;
    parsed->cnt = NULL;
    snprintf(err, sizeof err, "%s", parsed->err);
    w->parse_s[i] = parsed->secs;
    /* compute_adjEUMA (emsar_main.c:403): L = EUMA . Wf on the device, bit-identical to the host loop */
    double *Ldev = NULL;
    if (rc == 0) {
        double *wf = (double *)malloc(sizeof(double) * (size_t)r->nfl);
        Ldev = (double *)malloc(sizeof(double) * (size_t)(r->n_rows > 0 ? r->n_rows : 1));
        if (!wf || !Ldev) rc = EMSAR_HOST_ERR_OOM;
        else if (emsar_model_wf(r, cnt, wf) == EMSAR_HOST_OK) {
            int hrc = emsar_hip_adj_euma(ctx, wf, Ldev);
            if (hrc) { snprintf(err, sizeof err, "adj_euma: %s (%s)", emsar_hip_strerror(hrc), emsar_hip_last_error(ctx)); rc = EMSAR_HOST_ERR_IO; }
        } else { free(Ldev); Ldev = NULL; }            /* model_build reports the empty fragment-length window */
        free(wf);
    }
    /* Model preparation.  EUMAcut carries over in sample order (emsar_main.c:95,418: never reset), but it only ever changes
     * when a set exceeds 5000 transcripts (emsar_main.c:417-423).  So every worker builds its model at once, without the
     * lock, from the value it sees now; at its turn in the sample order it checks that the samples before it have left
     * that value in place and publishes its own (possibly raised) one.  Only if an earlier sample did raise the cut in
     * the meantime is the model rebuilt, at the turn, from the value that sample left. */
    double t_model = now_s();
    pthread_mutex_lock(w->mu);
    const double cut_seen = *w->eumacut;
    pthread_mutex_unlock(w->mu);
    double cut_mine = cut_seen;
    if (rc == 0) rc = emsar_model_build_L(r, cnt, cfg->delta, &cut_mine, Ldev, &m, err, sizeof err);
    pthread_mutex_lock(w->mu);
    while (*w->next_model != i) pthread_cond_wait(w->cv, w->mu);
    if (rc == 0 && *w->eumacut != cut_seen) {
        emsar_model_free(m); m = NULL;
        cut_mine = *w->eumacut;
        rc = emsar_model_build_L(r, cnt, cfg->delta, &cut_mine, Ldev, &m, err, sizeof err);
    }
    if (rc == 0) *w->eumacut = cut_mine;
    (*w->next_model)++;
    pthread_cond_broadcast(w->cv);
    pthread_mutex_unlock(w->mu);
    free(Ldev);
    w->model_s[i] = now_s() - t_model;
    if (rc) { fprintf(stderr, "alnfile[%d]=%s: %s\n", i, cfg->aln[i], err); goto done; }
    if (cfg->verbose > 0)
        fprintf(stdout, "alnfile[%d]=%s  reads=%lld (seen %lld, >k %lld, bad fraglen %lld, discrepant %lld, no segment %lld)  sets=%d  gpu=%d\n",
                i, cfg->aln[i], (long long)cnt->total_reads, (long long)cnt->reads_seen, (long long)cnt->reads_over_k,
                (long long)cnt->reads_bad_fraglen, (long long)cnt->reads_discrepant, (long long)cnt->reads_no_segment, m->n_sets, w->device);

    const size_t T = (size_t)r->n_tx;
    theta = (double *)malloc(T * 8); mean = (double *)malloc(T * 8); sd = (double *)malloc(T * 8);
    ieuma = (double *)malloc(T * 8); tpm = (double *)malloc(T * 8); ir = (double *)malloc(T * 8); iri = (int32_t *)malloc(T * 4);
    rounds = (double *)malloc(T * 8 * (size_t)cfg->n_round);
    if (!theta || !mean || !sd || !ieuma || !tpm || !ir || !iri || !rounds) { rc = EMSAR_HOST_ERR_OOM; goto done; }

    /* ---- the replaced call: run_MLE_threads() + construct_FPKMfinal, emsar_main.c:444-450 ---- */
    emsar_em_params p = {cfg->max_iter, cfg->accel, cfg->tol, 0.0, 0, cfg->set_mode, cfg->count_floor, cfg->zero_cut, cfg->abs_step};
    /* den_t = sum_c m_ct E_c in row order on the host: the device's own scatter adds with atomics, whose order (and with it
     * the last bits of den, of theta and now and then the sixth printed decimal) changes from run to run */
    double t_host = now_s();
    den = (double *)calloc(T, sizeof(double));
    if (!den) { rc = EMSAR_HOST_ERR_OOM; goto done; }
    /* ... and compute_iEUMA (emsar_functions.c:3218: iEUMA_t = sum of adjEUMA over the segments that hold t) in the same sweep, for the
     * same reason: the eff.length and iReadcount columns are then the same bytes in every run */
    memset(ieuma, 0, T * 8);
    for (int64_t c = 0; c < r->n_rows; c++) {
        const double e = m->E_solver[c], l = m->L[c];
        if (e != 0.0) for (uint64_t k = r->row_ptr[c]; k < r->row_ptr[c + 1]; k++) den[r->col_idx[k]] += e;
        if (l != 0.0) for (uint64_t k = r->row_ptr[c]; k < r->row_ptr[c + 1]; k++) ieuma[r->col_idx[k]] += l;
    }
    w->host_s[i] = w->model_s[i] + (now_s() - t_host);
    if ((cfg->compare || cfg->compare_usage) && i == 0) { publish_ref(w, r, cnt->R, m->E_solver, den); published = 1; }
    if ((rc = emsar_hip_upload_sample(ctx, cnt->R, m->E_solver, den)) ||
        (rc = emsar_hip_solve(ctx, &p, theta, &w->stats[i]))) {
        fprintf(stderr, "alnfile[%d]: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        goto done;
    }
    for (int k = 0; k < cfg->n_round; k++) memcpy(rounds + (size_t)k * T, theta, T * 8);   /* deterministic solver: rounds coincide */
    emsar_mean_sd(r->n_tx, cfg->n_round, rounds, mean, sd);
    /* ---- compute_iEUMA + print_FPKMfinal, emsar_main.c:454-460 ---- */
    if ((rc = emsar_hip_normalise(ctx, mean, ieuma, cnt->total_reads, tpm, ir, iri))) {
        fprintf(stderr, "alnfile[%d]: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        goto done;
    }
    int64_t tot = 0;
    t_host = now_s();
    snprintf(path, sizeof path, "%s/%s.%d.fpkm", cfg->outdir, cfg->prefix, i);
    if ((rc = emsar_write_fpkm(path, r, mean, sd, ieuma, ir, iri, tpm, &tot))) { fprintf(stderr, "can't write %s\n", path); goto done; }
    if (cfg->verbose > 0) fprintf(stdout, "Total inferred readcount=%lld\n", (long long)tot);
    snprintf(path, sizeof path, "%s/%s.%d.fraglength_effect", cfg->outdir, cfg->prefix, i);
    if ((rc = emsar_write_fraglength(path, r, cnt, m))) { fprintf(stderr, "can't write %s\n", path); goto done; }
    if (cfg->print_segments) {
        snprintf(path, sizeof path, "%s/%s.%d.segments", cfg->outdir, cfg->prefix, i);
        if ((rc = emsar_write_segments(path, r, cnt, m, mean))) { fprintf(stderr, "can't write %s\n", path); goto done; }
    }
    w->host_s[i] += now_s() - t_host;
    /* ---- gene level (--g2t): FPKM2gFPKM.pl's sums of columns FPKM, iReadcount and TPM per gene, on the device ---- */
    const emsar_genes *G = cfg->genes;
    const size_t NG = G ? (size_t)G->n_genes : 0;
    if (G) {
        gcols = (double *)malloc(T * 8 * 3); gsums = (double *)malloc(NG * 8 * 3);
        if (!gcols || !gsums) { rc = EMSAR_HOST_ERR_OOM; goto done; }
        memcpy(gcols, mean, T * 8); memcpy(gcols + T, ir, T * 8); memcpy(gcols + 2 * T, tpm, T * 8);
        if ((rc = emsar_hip_gene_sums(ctx, 3, gcols, gsums))) {
            fprintf(stderr, "alnfile[%d]: gene sums: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
            goto done;
        }
        snprintf(path, sizeof path, "%s/%s.%d.gfpkm", cfg->outdir, cfg->prefix, i);
        if ((rc = emsar_write_gfpkm(path, G, gsums, gsums + NG, gsums + 2 * NG))) { fprintf(stderr, "can't write %s\n", path); goto done; }
    }
    /* ---- isoform usage (--isoforms): each transcript's share of its gene's FPKM and the gene's dominant isoform, on the device ---- */
    const int ISO = G && cfg->isoforms;
    if (ISO) {
        iso_u = (double *)malloc((T > 0 ? T : 1) * 8); dom = (int32_t *)malloc((NG > 0 ? NG : 1) * 4);
        if (!iso_u || !dom) { rc = EMSAR_HOST_ERR_OOM; goto done; }
        if ((rc = emsar_hip_isoform_usage(ctx, 1, mean, iso_u, dom))) {
            fprintf(stderr, "alnfile[%d]: isoform usage: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
            goto done;
        }
        if (cfg->boot_n <= 0) {
            snprintf(path, sizeof path, "%s/%s.%d.isoforms", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_isoforms(path, r, G, mean, iso_u, dom, 0, NULL, NULL, NULL, 0, NULL, NULL))) { fprintf(stderr, "can't write %s\n", path); goto done; }
        }
    }
    /* ---- model fit (--fit): the residuals of the printed FPKM against the sample's segments, per transcript and per gene, on the device ---- */
    if (cfg->fit) {
        const size_t Ta = T > 0 ? T : 1, Ga = NG > 0 ? NG : 1;
        double *fv = (double *)malloc(Ta * 8 * 4), *gv = G ? (double *)malloc(Ga * 8 * 4) : NULL;
        int32_t *fw = (int32_t *)malloc(Ta * 4);
        const emsar_fit_outputs fo = {NULL, NULL, NULL, fv, fv ? fv + T : NULL, fv ? fv + 2 * T : NULL, fv ? fv + 3 * T : NULL, fw,
                                      gv, gv ? gv + NG : NULL, gv ? gv + 2 * NG : NULL, gv ? gv + 3 * NG : NULL};
        if (!fv || !fw || (G && !gv)) rc = EMSAR_HOST_ERR_OOM;
        else if ((rc = emsar_hip_model_fit(ctx, mean, m->E_solver, &fo, NULL)))
            fprintf(stderr, "alnfile[%d]: model fit: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        else {
            snprintf(path, sizeof path, "%s/%s.%d.fit", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_fit(path, r, mean, den, fo.tx_df, fo.tx_chi2, fo.tx_dev, fo.tx_miss, fw))) fprintf(stderr, "can't write %s\n", path);
            else if (G) {
                snprintf(path, sizeof path, "%s/%s.%d.gfit", cfg->outdir, cfg->prefix, i);
                if ((rc = emsar_write_gfit(path, r, G, mean, den, fo.gene_df, fo.gene_chi2, fo.gene_dev, fo.gene_miss))) fprintf(stderr, "can't write %s\n", path);
            }
        }
        free(fv); free(gv); free(fw);
        if (rc) goto done;
    }
    /* ---- presence test (--presence): one likelihood-ratio test per transcript on its connected set, on the device ---- */
    if (cfg->presence) {
        const size_t Q = cfg->pres_q ? (size_t)cfg->pres_nq : T, Qa = Q > 0 ? Q : 1;
        double *pv = (double *)malloc(Qa * 8 * 3);
        int32_t *pi = (int32_t *)malloc(Qa * 4 * 2);
        const emsar_presence_outputs po = {pv, pv ? pv + Q : NULL, pi, pv ? pv + 2 * Q : NULL, pi ? pi + Q : NULL, NULL};
        if (!pv || !pi) rc = EMSAR_HOST_ERR_OOM;
        else if ((rc = emsar_hip_presence(ctx, &p, (int32_t)Q, cfg->pres_q, &po, NULL)))
            fprintf(stderr, "alnfile[%d]: presence: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        else {
            snprintf(path, sizeof path, "%s/%s.%d.presence", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_presence(path, r, (int32_t)Q, cfg->pres_q, mean, po.lambda, po.pvalue, po.status, po.heir, po.heir_share)))
                fprintf(stderr, "can't write %s\n", path);
        }
        free(pv); free(pi);
        if (rc) goto done;
    }
    /* ---- profile-likelihood intervals (--profile): two confidence limits per transcript on its connected set, on the device ---- */
    if (cfg->profile) {
        const size_t Q = cfg->prof_q ? (size_t)cfg->prof_nq : T, Qa = Q > 0 ? Q : 1;
        double *pv = (double *)malloc(Qa * 8 * 3);
        int32_t *pi = (int32_t *)malloc(Qa * 4);
        const emsar_profile_params pp = {cfg->profile_level, 0.0, cfg->profile_evals, 0};
        const emsar_profile_outputs po = {pv, pv ? pv + Q : NULL, NULL, NULL, pv ? pv + 2 * Q : NULL, NULL, pi, NULL};
        if (!pv || !pi) rc = EMSAR_HOST_ERR_OOM;
        else if ((rc = emsar_hip_profile(ctx, &p, &pp, (int32_t)Q, cfg->prof_q, &po, NULL)))
            fprintf(stderr, "alnfile[%d]: profile: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        else {
            snprintf(path, sizeof path, "%s/%s.%d.profile", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_profile(path, r, (int32_t)Q, cfg->prof_q, mean, po.lower, po.upper, po.lambda, po.status)))
                fprintf(stderr, "can't write %s\n", path);
        }
        free(pv); free(pi);
        if (rc) goto done;
        /* with --g2t the same question per gene, and whether the gene is needed at all (emsar_hip_profile_genes; --profile-list names
         * transcripts and does not filter it): .gprofile */
        if (G) {
            const size_t Ga = NG > 0 ? NG : 1;
            double *gv = (double *)malloc(Ga * 8 * 4);
            int32_t *gi = (int32_t *)malloc(Ga * 4 * 2);
            const emsar_profile_gene_outputs go = {gv, gv ? gv + NG : NULL, NULL, NULL, gv ? gv + 2 * NG : NULL, gv ? gv + 3 * NG : NULL, NULL,
                                                   gi, NULL, NULL, gi ? gi + NG : NULL};
            if (!gv || !gi) rc = EMSAR_HOST_ERR_OOM;
            else if ((rc = emsar_hip_profile_genes(ctx, &p, &pp, (int32_t)NG, NULL, &go, NULL)))
                fprintf(stderr, "alnfile[%d]: profile_genes: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
            else {
                snprintf(path, sizeof path, "%s/%s.%d.gprofile", cfg->outdir, cfg->prefix, i);
                if ((rc = write_gprofile(path, G, gsums, &go))) fprintf(stderr, "can't write %s\n", path);
            }
            free(gv); free(gi);
            if (rc) goto done;
        }
    }
    /* ---- two-sample tests (--compare, --compare-usage): this sample (A) against sample 0 (B, in a second context on this device), on the device ---- */
    if ((cfg->compare || cfg->compare_usage) && i > 0) {
        compare_ref *ref = cfg->ref;
        pthread_mutex_lock(w->mu);
        while (!ref->ready) pthread_cond_wait(w->cv, w->mu);
        const int have_ref = ref->ready > 0;
        pthread_mutex_unlock(w->mu);
        if (!have_ref) { fprintf(stderr, "alnfile[%d]: compare: sample 0 gave no solver inputs\n", i); rc = EMSAR_HOST_ERR_IO; goto done; }
        if (!w->ref_ctx) {
            emsar_hip_ctx *rc_ctx = NULL;
            if ((rc = emsar_hip_create(&rc_ctx, w->device)) || (rc = emsar_hip_set_deterministic(rc_ctx, !cfg->no_deterministic)) ||
                (rc = emsar_hip_upload_structure(rc_ctx, r->n_rows, r->n_tx, r->row_ptr, r->col_idx, EMSAR_LAYOUT_AUTO)) ||
                (rc = emsar_hip_upload_sample(rc_ctx, ref->R, ref->E, ref->den))) {
                fprintf(stderr, "alnfile[%d]: compare: sample 0's context: %s (%s)\n", i, emsar_hip_strerror(rc), rc_ctx ? emsar_hip_last_error(rc_ctx) : "");
                emsar_hip_destroy(rc_ctx);
                goto done;
            }
            w->ref_ctx = rc_ctx;
        }
        const size_t Q = cfg->cmp_q ? (size_t)cfg->cmp_nq : T, Qa = Q > 0 ? Q : 1;
        /* the share of its gene (emsar_hip_compare_usage: this context's gene map serves both samples): .ucompare */
        if (cfg->compare_usage) {
            double *uv = (double *)malloc(Qa * 8 * 5);
            int32_t *ui = (int32_t *)malloc(Qa * 4 * 3);
            const emsar_usage_outputs uo = {uv, NULL, uv ? uv + Q : NULL, uv ? uv + 2 * Q : NULL, uv ? uv + 3 * Q : NULL, NULL, uv ? uv + 4 * Q : NULL, NULL,
                                            ui, ui ? ui + Q : NULL, ui ? ui + 2 * Q : NULL, NULL};
            if (!uv || !ui) rc = EMSAR_HOST_ERR_OOM;
            else if ((rc = emsar_hip_compare_usage(ctx, w->ref_ctx, &p, NULL, (int32_t)Q, cfg->cmp_q, &uo, NULL)))
                fprintf(stderr, "alnfile[%d]: compare_usage: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
            else {
                snprintf(path, sizeof path, "%s/%s.%d.ucompare", cfg->outdir, cfg->prefix, i);
                if ((rc = write_ucompare(path, r, G, (int32_t)Q, cfg->cmp_q, &uo))) fprintf(stderr, "can't write %s\n", path);
            }
            free(uv); free(ui);
            if (rc) goto done;
        }
        if (cfg->compare) {
            double *cv = (double *)malloc(Qa * 8 * 5);
            int32_t *ci = (int32_t *)malloc(Qa * 4 * 2);
            const emsar_compare_params cp = {cfg->compare_ratio, 0.0, 0, 0};
            const emsar_compare_outputs co = {cv, cv ? cv + Q : NULL, cv ? cv + 2 * Q : NULL, cv ? cv + 3 * Q : NULL, cv ? cv + 4 * Q : NULL, NULL, NULL, NULL, NULL,
                                              ci, ci ? ci + Q : NULL};
            if (!cv || !ci) rc = EMSAR_HOST_ERR_OOM;
            else if ((rc = emsar_hip_compare(ctx, w->ref_ctx, &p, &cp, (int32_t)Q, cfg->cmp_q, &co, NULL)))
                fprintf(stderr, "alnfile[%d]: compare: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
            else {
                snprintf(path, sizeof path, "%s/%s.%d.compare", cfg->outdir, cfg->prefix, i);
                if ((rc = write_compare(path, r, (int32_t)Q, cfg->cmp_q, &co))) fprintf(stderr, "can't write %s\n", path);
            }
            free(cv); free(ci);
            if (rc) goto done;
            /* with --g2t the same question per gene (emsar_hip_compare_genes: this context's gene map serves both samples): .gcompare */
            if (G) {
                const size_t Ga = NG > 0 ? NG : 1;
                double *gv = (double *)malloc(Ga * 8 * 5);
                int32_t *gi = (int32_t *)malloc(Ga * 4 * 3);
                const emsar_compare_gene_outputs go = {gv, gv ? gv + NG : NULL, gv ? gv + 2 * NG : NULL, gv ? gv + 3 * NG : NULL, gv ? gv + 4 * NG : NULL, NULL,
                                                       NULL, NULL, NULL, gi, gi ? gi + NG : NULL, gi ? gi + 2 * NG : NULL};
                if (!gv || !gi) rc = EMSAR_HOST_ERR_OOM;
                else if ((rc = emsar_hip_compare_genes(ctx, w->ref_ctx, &p, &cp, (int32_t)NG, NULL, &go, NULL)))
                    fprintf(stderr, "alnfile[%d]: compare_genes: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
                else {
                    snprintf(path, sizeof path, "%s/%s.%d.gcompare", cfg->outdir, cfg->prefix, i);
                    if ((rc = write_gcompare(path, G, &go))) fprintf(stderr, "can't write %s\n", path);
                }
                free(gv); free(gi);
                if (rc) goto done;
            }
        }
    }
    /* ---- asymptotic standard errors (--asymptotic): the inverse of the observed information at the printed FPKM, on the device ---- */
    if (cfg->asymptotic) {
        const size_t Ta = T > 0 ? T : 1, Ga = NG > 0 ? NG : 1;
        double *av = (double *)malloc(Ta * 8 * 5), *gv = G ? (double *)malloc(Ga * 8) : NULL;
        int32_t *ai = (int32_t *)malloc(Ta * 4 * 2), *gi = G ? (int32_t *)malloc(Ga * 4) : NULL;
        const emsar_asym_params ap = {cfg->boundary_cut, 0.0, -1, 0};
        const emsar_asym_outputs ao = {av, av ? av + T : NULL, av ? av + 2 * T : NULL, NULL, G && av ? av + 4 * T : NULL, ai, ai ? ai + T : NULL,
                                       av ? av + 3 * T : NULL, NULL, gv, gi, NULL, NULL, NULL};
        if (!av || !ai || (G && (!gv || !gi))) rc = EMSAR_HOST_ERR_OOM;
        else if ((rc = emsar_hip_asymptotic(ctx, mean, &ap, &ao, NULL)))
            fprintf(stderr, "alnfile[%d]: asymptotic: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        else {
            snprintf(path, sizeof path, "%s/%s.%d.asym", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_asym(path, r, mean, tpm, ao.sd_fpkm, ao.sd_tpm, ao.var, ao.status, ao.partner, ao.partner_cov, ao.usage_sd)))
                fprintf(stderr, "can't write %s\n", path);
            else if (G) {
                snprintf(path, sizeof path, "%s/%s.%d.gasym", cfg->outdir, cfg->prefix, i);
                if ((rc = emsar_write_gasym(path, G, gsums, gv, gi))) fprintf(stderr, "can't write %s\n", path);
            }
        }
        free(av); free(gv); free(ai); free(gi);
        if (rc) goto done;
    }
    /* ---- Poisson bootstrap (--bootstrap B): its own file; .fpkm keeps the reference's column 3.  With --g2t the same replicates
     *      give the genes' sd as well (bootstrap_genes: the transcript outputs are the same bits as bootstrap's), and with --isoforms
     *      the usage statistics (bootstrap_isoforms: every other output is the same bits) ---- */
    if (cfg->boot_n > 0) {
        double *bm = (double *)malloc(T * 8), *bs = (double *)malloc(T * 8), *bt = (double *)malloc(T * 8);
        double *gb = G ? (double *)malloc(NG * 8 * 3) : NULL;
        /* --bootstrap-quantiles: [2][n_q][n_tx] FPKM then TPM quantiles, with --g2t also [2][n_q][n_genes] */
        const size_t NQ = (size_t)cfg->bq_n;
        double *bq = NQ ? (double *)malloc((T > 0 ? T : 1) * 8 * 2 * NQ) : NULL, *gq = NQ && G ? (double *)malloc((NG > 0 ? NG : 1) * 8 * 2 * NQ) : NULL;
        /* --isoforms: [2][n_tx] mean and sd of the usage, [n_tx] dominance counts, [n_q][n_tx] usage quantiles */
        double *ub = ISO ? (double *)malloc((T > 0 ? T : 1) * 8 * (2 + NQ)) : NULL;
        int32_t *uc = ISO ? (int32_t *)malloc((T > 0 ? T : 1) * 4) : NULL;
        const emsar_isoform_outputs iso = {ub, ub ? ub + T : NULL, uc, ub && NQ ? ub + 2 * T : NULL};
        if (!bm || !bs || !bt || (G && !gb) || (NQ && !bq) || (NQ && G && !gq) || (ISO && (!ub || !uc))) rc = EMSAR_HOST_ERR_OOM;
        else if ((rc = ISO ? emsar_hip_bootstrap_isoforms(ctx, &p, cfg->boot_seed + (uint64_t)i, 0, cfg->boot_n, cfg->bq_n, cfg->bq, bm, bs, bt, NULL, NULL,
                                                          bq, NQ ? bq + NQ * T : NULL, gb, gb + NG, gb + 2 * NG, gq, NQ ? gq + NQ * NG : NULL,
                                                          &w->bstats[i], &w->qstats[i], &iso)
                         : NQ ? emsar_hip_bootstrap_quantiles(ctx, &p, cfg->boot_seed + (uint64_t)i, 0, cfg->boot_n, cfg->bq_n, cfg->bq, bm, bs, bt, NULL, NULL,
                                                          bq, bq + NQ * T, gb, G ? gb + NG : NULL, G ? gb + 2 * NG : NULL, gq, G ? gq + NQ * NG : NULL,
                                                          &w->bstats[i], &w->qstats[i])
                         : G ? emsar_hip_bootstrap_genes(ctx, &p, cfg->boot_seed + (uint64_t)i, 0, cfg->boot_n, bm, bs, bt, NULL, gb, gb + NG, gb + 2 * NG,
                                                     &w->bstats[i])
                         : emsar_hip_bootstrap(ctx, &p, cfg->boot_seed + (uint64_t)i, 0, cfg->boot_n, bm, bs, bt, NULL, &w->bstats[i])))
            fprintf(stderr, "alnfile[%d]: bootstrap: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        else {
            snprintf(path, sizeof path, "%s/%s.%d.bootstrap", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_bootstrap(path, r, mean, bm, bs, tpm, bt))) fprintf(stderr, "can't write %s\n", path);
            else if (G) {
                snprintf(path, sizeof path, "%s/%s.%d.gbootstrap", cfg->outdir, cfg->prefix, i);
                if ((rc = emsar_write_gbootstrap(path, G, gsums, gb, gb + NG, gsums + 2 * NG, gb + 2 * NG))) fprintf(stderr, "can't write %s\n", path);
            }
            if (!rc && NQ) {
                snprintf(path, sizeof path, "%s/%s.%d.bootq", cfg->outdir, cfg->prefix, i);
                if ((rc = emsar_write_bootq(path, r, cfg->bq_n, cfg->bq, bq, bq + NQ * T))) fprintf(stderr, "can't write %s\n", path);
                else if (G) {
                    snprintf(path, sizeof path, "%s/%s.%d.gbootq", cfg->outdir, cfg->prefix, i);
                    if ((rc = emsar_write_gbootq(path, G, cfg->bq_n, cfg->bq, gq, gq + NQ * NG))) fprintf(stderr, "can't write %s\n", path);
                }
            }
            if (!rc && ISO) {
                snprintf(path, sizeof path, "%s/%s.%d.isoforms", cfg->outdir, cfg->prefix, i);
                if ((rc = emsar_write_isoforms(path, r, G, mean, iso_u, dom, cfg->boot_n, iso.usage_mean, iso.usage_sd, iso.dominant_count, cfg->bq_n, cfg->bq,
                                               iso.usage_q)))
                    fprintf(stderr, "can't write %s\n", path);
            }
        }
        free(bm); free(bs); free(bt); free(gb); free(bq); free(gq); free(ub); free(uc);
        if (rc) goto done;
    }
    /* ---- depth subsampling (--subsample f1,f2,..): its own files ---- */
    if (cfg->sub_nf > 0) {
        const size_t K = (size_t)cfg->sub_nf;
        const uint64_t seed = cfg->sub_seed + (uint64_t)i;
        double *sv = (double *)malloc((T > 0 ? T : 1) * 8 * 4 * K), *gv = G ? (double *)malloc(NG * 8 * 3 * K) : NULL;
        double depth[64];
        if (!sv || (G && !gv)) rc = EMSAR_HOST_ERR_OOM;
        else if ((rc = emsar_hip_subsample(ctx, &p, seed, cfg->sub_nf, cfg->sub_f, cfg->sub_reps, sv, sv + K * T, sv + 2 * K * T, sv + 3 * K * T, depth, NULL,
                                           gv, gv ? gv + K * NG : NULL, gv ? gv + 2 * K * NG : NULL, &w->sstats[i])))
            fprintf(stderr, "alnfile[%d]: subsample: %s (%s)\n", i, emsar_hip_strerror(rc), emsar_hip_last_error(ctx));
        else {
            snprintf(path, sizeof path, "%s/%s.%d.saturation", cfg->outdir, cfg->prefix, i);
            if ((rc = emsar_write_saturation(path, r, mean, tpm, cfg->sub_nf, cfg->sub_f, cfg->sub_reps, seed, depth, sv, sv + K * T, sv + 2 * K * T,
                                             sv + 3 * K * T)))
                fprintf(stderr, "can't write %s\n", path);
            else if (G) {
                snprintf(path, sizeof path, "%s/%s.%d.gsaturation", cfg->outdir, cfg->prefix, i);
                if ((rc = emsar_write_gsaturation(path, G, gsums, gsums + 2 * NG, cfg->sub_nf, cfg->sub_f, cfg->sub_reps, seed, depth, gv, gv + K * NG,
                                                  gv + 2 * K * NG)))
                    fprintf(stderr, "can't write %s\n", path);
            }
        }
        free(sv); free(gv);
        if (rc) goto done;
    }
    if (cfg->verbose > 0)
        fprintf(stdout, "Complete: %s/%s.%d.fpkm  (EM passes %d, converged %d, solve %.1f ms, logL %.6f)\n", cfg->outdir, cfg->prefix, i,
                w->stats[i].iters, w->stats[i].converged, w->stats[i].solve_ms, w->stats[i].loglik);
done:
    if ((cfg->compare || cfg->compare_usage) && i == 0 && !published) publish_ref(w, r, NULL, NULL, NULL);     /* the other samples must not wait for it */
    free(theta); free(rounds); free(mean); free(sd); free(ieuma); free(tpm); free(ir); free(iri); free(den); free(gcols); free(gsums); free(iso_u); free(dom);
    emsar_counts_free(cnt); emsar_model_free(m);
    return rc;
}

static void *worker_main(void *a) {
    worker_arg *w = (worker_arg *)a;
    emsar_hip_ctx *ctx = NULL;
    parse_job slot[2];                                               /* the sample in hand and the one being counted ahead */
    int c = 0;
    memset(slot, 0, sizeof slot);
    pthread_mutex_lock(w->mu);
    while (!*w->go) pthread_cond_wait(w->cv, w->mu);                 /* n_workers is final from here on */
    pthread_mutex_unlock(w->mu);
    w->ao = w->cfg->ao;
    int crc = 0;
    if (w->cfg->device_collapse) {                                    /* before the first parse thread starts: it needs the device */
        pthread_mutex_init(&w->cdev.mu, NULL);
        crc = emsar_hip_create(&w->cdev.ctx, w->device);
        if (crc == 0) { w->ao.collapse = cli_collapse; w->ao.collapse_user = w; }
        else fprintf(stderr, "GPU %d: %s (--device-collapse)\n", w->device, emsar_hip_strerror(crc));
    }
    if (w->worker < w->cfg->n_aln) parse_start(&slot[c], w, w->worker);
    int rc = crc ? crc : emsar_hip_create(&ctx, w->device);
    if (rc == 0) rc = emsar_hip_set_deterministic(ctx, !w->cfg->no_deterministic);     /* the streamed part of a solve: same bytes every run */
    if (rc == 0) rc = emsar_hip_upload_structure(ctx, w->rsh->n_rows, w->rsh->n_tx, w->rsh->row_ptr, w->rsh->col_idx, EMSAR_LAYOUT_AUTO);
    if (rc == 0) rc = emsar_hip_upload_euma(ctx, w->rsh->euma, w->rsh->nfl);     /* once per rsh: compute_adjEUMA runs on the device */
    if (rc == 0 && w->cfg->genes) rc = emsar_hip_set_gene_map(ctx, w->cfg->genes->n_genes, w->cfg->genes->gene_of_tx);
    if (rc) fprintf(stderr, "GPU %d: %s\n", w->device, emsar_hip_strerror(rc));
    for (int i = w->worker; i < w->cfg->n_aln; i += w->n_workers) {
        parse_job *cur = &slot[c];
        parse_wait(cur);
        if (i + w->n_workers < w->cfg->n_aln) parse_start(&slot[c ^ 1], w, i + w->n_workers);
        if (rc) {   /* keep the ordered hand-over alive so the other workers are not stuck */
            emsar_counts_free(cur->cnt); cur->cnt = NULL;
            pthread_mutex_lock(w->mu);
            while (*w->next_model != i) pthread_cond_wait(w->cv, w->mu);
            (*w->next_model)++;
            pthread_cond_broadcast(w->cv);
            pthread_mutex_unlock(w->mu);
            w->status[i] = rc;
            if ((w->cfg->compare || w->cfg->compare_usage) && i == 0) publish_ref(w, w->rsh, NULL, NULL, NULL);
        } else {
            w->status[i] = run_sample(w, ctx, i, cur);
        }
        c ^= 1;
    }
    emsar_hip_destroy(w->ref_ctx);
    emsar_hip_destroy(ctx);
    if (w->cfg->device_collapse) { emsar_hip_destroy(w->cdev.ctx); pthread_mutex_destroy(&w->cdev.mu); }
    return NULL;
}

static void usage(const char *a0) {
    fprintf(stderr,
            "Usage : %s <options> -I rshfile outdir outprefix alignmentfile|alignmentfilelist\n"
            "  -I, --rsh <file>        rsh index (from emsar-build)            [required]\n"
            "  -M, --multisample       last argument lists one alignment file per line; samples are spread over GPUs\n"
            "  -P, --PE                paired-end          -s, --strand_type ns|ssf|ssr|ssfr|ssrf (default ns)\n"
            "  -S, --SAM / -B, --BAM   SAM text / BAM input (default: default bowtie output)\n"
            "  -k, --max_repeat <n>    reads with more alignments are discarded (default 100)\n"
            "  -n, --nround <n>        rounds reported in the mean/sd columns (default 4; the EM is deterministic)\n"
            "  -e, --epsilon <tol>     EM stops when max |dtheta|/(theta+1e-6) < tol (default 1e-10)\n"
            "  -i, --max_niter_mle <n> cap on EM passes (default 200000)\n"
            "  -d, --delta <d>         10^d scaling of the effective lengths (default 0)\n"
            "  -g, --print_segments    also write .segments\n"
            "      --count-floor <reads> stopping-rule floor in inferred reads (default 0 = off; e.g. 1e-3 for large samples)\n"
            "      --zero-cut <x>        components below x and still falling do not hold the solve up (default 2.5e-7: they print as\n"
            "                            0.000000 either way; 0 = every component must meet -e)\n"
            "      --abs-step <x>        components that move by less than x FPKM per pass count as converged (default 1e-13; 0 = off)\n"
            "      --rsh-cache[=file]    read the parsed index from a binary cache (default <rshfile>.bin), write it after a text parse\n"
            "      --streaming-only      do not split the problem into connected sets (every pass streams the whole matrix)\n"
            "      --no-deterministic    streaming passes with floating atomics (run-to-run differences in the last digits) instead of\n"
            "                            the fixed-point sums that make two runs of the same input print the same bytes\n"
            "      --device-collapse     reads with two or more transcripts are merged into weighted segments on the GPU\n"
            "                            (emsar_hip_collapse_rows) instead of one index lookup per read on the host; same counts\n"
            "      --bootstrap <B>       also write <outdir>/<prefix>.<i>.bootstrap: mean and sd of FPKM and sd of TPM over B Poisson\n"
            "                            bootstrap replicates of the sample (default 0 = off; .fpkm is the same either way)\n"
            "      --bootstrap-seed <n>  seed of the replicates' draws (default 1; sample i of -M uses n + i)\n"
            "      --bootstrap-quantiles <q1,q2,..> with --bootstrap B (B <= 4096): also write <prefix>.<i>.bootq, per transcript the quantiles of\n"
            "                            FPKM and of TPM over the replicates at each probability q in [0, 1] (at most 64; 0.025,0.5,0.975 = the\n"
            "                            95 %% percentile interval and the median), and with --g2t <prefix>.<i>.gbootq per gene\n"
            "      --subsample <f1,f2,..> also write <prefix>.<i>.saturation: per fraction f in (0, 1] (at most 64) the mean and sd of FPKM and\n"
            "                            TPM over replicates that keep every read with probability f (with --g2t also .gsaturation per gene)\n"
            "      --subsample-reps <B>  replicates per fraction (default 10)\n"
            "      --subsample-seed <n>  seed of their draws (default 1; sample i of -M uses n + i)\n"
            "      --g2t <file>          gene map (gene<TAB>transcript per line, plain or gzipped): also write <prefix>.<i>.gfpkm, the\n"
            "                            per-gene sums of util/FPKM2gFPKM.pl, and with --bootstrap <prefix>.<i>.gbootstrap (gene sd)\n"
            "      --isoforms            with --g2t: also write <prefix>.<i>.isoforms, per transcript its share of its gene's FPKM (usage) and whether\n"
            "                            it is the gene's dominant isoform; with --bootstrap the mean and sd of the usage and the frequency of\n"
            "                            dominance over the replicates, with --bootstrap-quantiles the usage's quantiles as well\n"
            "      --fit                 also write <prefix>.<i>.fit: per transcript the effective number of segments, Pearson chi2, Poisson deviance and\n"
            "                            missed reads of the fitted model on its segments, the missed share of its expected reads and its worst\n"
            "                            segment (the id of .segments); with --g2t also <prefix>.<i>.gfit per gene\n"
            "      --presence            also write <prefix>.<i>.presence: per transcript the likelihood-ratio statistic Lambda of solving its connected\n"
            "                            set without it, the p-value, a status word (TESTED, ABSENT, ESSENTIAL, OUTSIDE, NOT_RESIDENT, UNCONVERGED)\n"
            "                            and the sibling that takes over most of its reads, with the share it takes\n"
            "      --presence-list <file> with --presence: test only the transcripts named in the file, one name per line\n"
            "      --profile             also write <prefix>.<i>.profile: per transcript the lower and upper limit of its profile-likelihood interval, the\n"
            "                            presence test's Lambda and a status word (TWO_SIDED, LOWER_ZERO, OUTSIDE, NOT_RESIDENT, UNCONVERGED); valid at FPKM 0;\n"
            "                            with --g2t also <prefix>.<i>.gprofile: per gene, in the order of .gfpkm, the limits of its total's interval, the gene\n"
            "                            presence test's Lambda, its p-value bound, the members taking part and a status word (also TOO_LARGE)\n"
            "      --profile-level <l>   with --profile: the confidence level, 0 < l < 1 (default 0.95)\n"
            "      --profile-evals <n>   with --profile: at most n set solves per limit (default 40); a search that needs more is UNCONVERGED\n"
            "      --profile-list <file> with --profile: only the transcripts named in the file, one name per line (.gprofile always holds every gene)\n"
            "      --compare             with -M and at least two samples: every sample i >= 1 also writes <prefix>.<i>.compare: per transcript its FPKM\n"
            "                            in sample i and in sample 0, log2 of the ratio, the likelihood-ratio statistic Lambda of equal abundance\n"
            "                            (siblings free in both samples), its p-value, a status word (TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT,\n"
            "                            UNCONVERGED) and the evaluations spent; with --g2t also <prefix>.<i>.gcompare: per gene, in the order of\n"
            "                            .gfpkm, the same test of the gene's summed FPKM with its isoforms free (status TOO_LARGE: more than 64\n"
            "                            connected sets and lone transcripts in one sample), the evaluations and the parts searched over\n"
            "      --compare-ratio <r>   with --compare: test theta_i = r * theta_0 (default 1; a fold change or a size factor)\n"
            "      --compare-list <file> with --compare or --compare-usage: only the transcripts named in the file, one name per line\n"
            "      --compare-usage       with -M, at least two samples and --g2t: every sample i >= 1 also writes <prefix>.<i>.ucompare: per transcript its\n"
            "                            gene, its share of the gene in sample i and in sample 0, the difference of their logits, Lambda of H0: equal\n"
            "                            shares (an isoform switch otherwise), its chi2_1 p-value, a status word, outer points and evaluations\n"
            "      --asymptotic          also write <prefix>.<i>.asym: per transcript the asymptotic standard error of FPKM and TPM from the inverse of\n"
            "                            the observed information, a status word and the sibling it is most confounded with; with --g2t also\n"
            "                            <prefix>.<i>.gasym (per gene) and a usage_sd column.  Not valid at the boundary (FPKM about 0): use --bootstrap there\n"
            "      --boundary-cut <x>    with --asymptotic: transcripts with FPKM <= x are held fixed (default 5e-7, the .fpkm print quantum)\n"
            "      --gpus <n> / --devices <a,b,..> (-M: one worker per entry, ids may repeat) / --device <d> / --plain /\n"
            "      --stats-json <file> / -q / -v\n", a0);
}

/* --presence-list / --profile-list FILE: the tids of the transcripts it names, one name per line, in file order */
static int read_name_list(const char *what, const char *file, const emsar_rsh *rsh, int32_t **q_out, int *nq_out) {
    FILE *f = fopen(file, "r");
    if (!f) { fprintf(stderr, "Can't open the %s list %s.\n", what, file); return 1; }
    char line[4096];
    int32_t *q = (int32_t *)malloc(sizeof(int32_t));
    int nq = 0;
    while (q && fgets(line, sizeof line, f)) {
        size_t n = strlen(line);
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r' || line[n - 1] == ' ' || line[n - 1] == '\t')) line[--n] = 0;
        if (!n) continue;
        const int32_t t = emsar_rsh_tid_of(rsh, line);
        if (t < 0) { fprintf(stderr, "--%s-list: no transcript %s in the index.\n", what, line); fclose(f); free(q); return 1; }
        int32_t *grown = (int32_t *)realloc(q, sizeof(int32_t) * (size_t)(nq + 1));
        if (!grown) { free(q); q = NULL; break; }
        q = grown;
        q[nq++] = t;
    }
    fclose(f);
    if (!q) { fprintf(stderr, "out of memory\n"); return 1; }
    *q_out = q; *nq_out = nq;
    return 0;
}

int main(int argc, char **argv) {
    config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.ao.max_repeat = 100; cfg.n_round = 4; cfg.verbose = 1; cfg.accel = 1; cfg.tol = 1e-10; cfg.max_iter = 200000;
    cfg.zero_cut = 2.5e-7;      /* a quarter of the "%lf" print quantum of the .fpkm file */
    cfg.abs_step = 1e-13;       /* see emsar_em_params.abs_step */
    cfg.boot_seed = 1;
    cfg.sub_reps = 10; cfg.sub_seed = 1;
    const char *strand = "ns"; int multisample = 0, gpus = 0, device = 0;
    int dev_map[64], n_dev_map = 0;
    const char *presence_list = NULL, *profile_list = NULL, *compare_list = NULL;
    int compare_ratio_given = 0;
    compare_ref ref; memset(&ref, 0, sizeof ref);
    int profile_level_given = 0;
    int boundary_cut_given = 0;
    static struct option lo[] = {
        {"rsh", required_argument, 0, 'I'}, {"PE", no_argument, 0, 'P'}, {"strand_type", required_argument, 0, 's'},
        {"maxthread", required_argument, 0, 'p'}, {"max_repeat", required_argument, 0, 'k'}, {"nround", required_argument, 0, 'n'},
        {"epsilon", required_argument, 0, 'e'}, {"max_niter_mle", required_argument, 0, 'i'}, {"delta", required_argument, 0, 'd'},
        {"print_segments", no_argument, 0, 'g'}, {"multisample", no_argument, 0, 'M'}, {"SAM", no_argument, 0, 'S'}, {"BAM", no_argument, 0, 'B'},
        {"verbose", no_argument, 0, 'v'}, {"no_verbose", no_argument, 0, 'q'}, {"gpus", required_argument, 0, 1000},
        {"device", required_argument, 0, 1001}, {"plain", no_argument, 0, 1002}, {"stats-json", required_argument, 0, 1003},
        {"count-floor", required_argument, 0, 1004}, {"streaming-only", no_argument, 0, 1005}, {"rsh-cache", optional_argument, 0, 1006}, {"zero-cut", required_argument, 0, 1007}, {"abs-step", required_argument, 0, 1008}, {"devices", required_argument, 0, 1009}, {"device-collapse", no_argument, 0, 1010}, {"no-deterministic", no_argument, 0, 1011},
        {"bootstrap", required_argument, 0, 1012}, {"bootstrap-seed", required_argument, 0, 1013}, {"g2t", required_argument, 0, 1014},
        {"subsample", required_argument, 0, 1015}, {"subsample-reps", required_argument, 0, 1016}, {"subsample-seed", required_argument, 0, 1017},
        {"bootstrap-quantiles", required_argument, 0, 1018}, {"isoforms", no_argument, 0, 1019}, {"fit", no_argument, 0, 1020},
        {"presence", no_argument, 0, 1021}, {"presence-list", required_argument, 0, 1022},
        {"asymptotic", no_argument, 0, 1023}, {"boundary-cut", required_argument, 0, 1024},
        {"profile", no_argument, 0, 1025}, {"profile-level", required_argument, 0, 1026}, {"profile-list", required_argument, 0, 1027},
        {"profile-evals", required_argument, 0, 1028},
        {"compare", no_argument, 0, 1029}, {"compare-ratio", required_argument, 0, 1030}, {"compare-list", required_argument, 0, 1031}, {"compare-usage", no_argument, 0, 1040},
        {"maxfraglen", required_argument, 0, 'F'}, {"minfraglen", required_argument, 0, 'f'}, {0, 0, 0, 0}};
    int c;
    while ((c = getopt_long(argc, argv, "vqPs:p:F:f:n:e:d:gMSBk:i:I:", lo, NULL)) != -1) {
        switch (c) {
            case 'I': cfg.rsh_path = optarg; break;
            case 'P': cfg.ao.pe = 1; break;
            case 's': strand = optarg; break;
            case 'p': break;                       /* CPU threads of the reference's solver: no meaning here */
            case 'F': case 'f': break;             /* overwritten by the rsh header in the reference too */
            case 'k': cfg.ao.max_repeat = atoi(optarg); break;
            case 'n': cfg.n_round = atoi(optarg); if (cfg.n_round <= 0) { fprintf(stderr, "option -n must be a natural number.\n"); return 1; } break;
            case 'e': cfg.tol = atof(optarg); if (cfg.tol <= 0) { fprintf(stderr, "option -e must be positive.\n"); return 1; } break;
            case 'i': cfg.max_iter = atoi(optarg); if (cfg.max_iter <= 0) { fprintf(stderr, "option -i must be positive.\n"); return 1; } break;
            case 'd': cfg.delta = atoi(optarg); break;
            case 'g': cfg.print_segments = 1; break;
            case 'M': multisample = 1; break;
            case 'S': cfg.ao.format = 1; break;
            case 'B': cfg.ao.format = 2; break;
            case 'v': cfg.verbose = 2; break;
            case 'q': cfg.verbose = 0; break;
            case 1000: gpus = atoi(optarg); break;
            case 1001: device = atoi(optarg); break;
            case 1002: cfg.accel = 0; break;
            case 1003: cfg.stats_json = optarg; break;
            case 1004: cfg.count_floor = atof(optarg); if (cfg.count_floor < 0) { fprintf(stderr, "--count-floor must be >= 0.\n"); return 1; } break;
            case 1005: cfg.set_mode = 1; break;
            case 1006: cfg.rsh_cache = optarg ? optarg : ""; break;
            case 1007: cfg.zero_cut = atof(optarg); break;
            case 1008: cfg.abs_step = atof(optarg); break;
            case 1010: cfg.device_collapse = 1; break;
            case 1011: cfg.no_deterministic = 1; break;
            case 1012: {
                char *end; errno = 0;
                long v = strtol(optarg, &end, 10);
                if (end == optarg || *end || errno || v < 0 || v > 1000000) { fprintf(stderr, "--bootstrap wants a number of replicates (0 .. 1000000).\n"); return 1; }
                cfg.boot_n = (int)v;
                break;
            }
            case 1013: {
                char *end; errno = 0;
                unsigned long long v = strtoull(optarg, &end, 10);
                if (end == optarg || *end || errno || optarg[0] == '-') { fprintf(stderr, "--bootstrap-seed wants a non-negative integer.\n"); return 1; }
                cfg.boot_seed = (uint64_t)v;
                break;
            }
            case 1014: cfg.g2t = optarg; break;
            case 1015: {
                const char *q = optarg;
                cfg.sub_nf = 0;
                for (;;) {
                    char *end; errno = 0;
                    const double v = strtod(q, &end);
                    if (end == q || (*end && *end != ',') || errno || !isfinite(v) || !(v > 0.0 && v <= 1.0) || cfg.sub_nf >= 64) {
                        fprintf(stderr, "--subsample wants a comma-separated list of 1 to 64 fractions in (0, 1].\n"); return 1;
                    }
                    cfg.sub_f[cfg.sub_nf++] = v;
                    if (!*end) break;
                    q = end + 1;
                }
                break;
            }
            case 1016: {
                char *end; errno = 0;
                long v = strtol(optarg, &end, 10);
                if (end == optarg || *end || errno || v < 1 || v > 1000000) { fprintf(stderr, "--subsample-reps wants a number of replicates (1 .. 1000000).\n"); return 1; }
                cfg.sub_reps = (int)v;
                break;
            }
            case 1017: {
                char *end; errno = 0;
                unsigned long long v = strtoull(optarg, &end, 10);
                if (end == optarg || *end || errno || optarg[0] == '-') { fprintf(stderr, "--subsample-seed wants a non-negative integer.\n"); return 1; }
                cfg.sub_seed = (uint64_t)v;
                break;
            }
            case 1018: {
                const char *q = optarg;
                cfg.bq_n = 0;
                for (;;) {
                    char *end; errno = 0;
                    const double v = strtod(q, &end);
                    if (end == q || (*end && *end != ',') || errno || !isfinite(v) || !(v >= 0.0 && v <= 1.0) || cfg.bq_n >= 64) {
                        fprintf(stderr, "--bootstrap-quantiles wants a comma-separated list of 1 to 64 probabilities in [0, 1].\n"); return 1;
                    }
                    cfg.bq[cfg.bq_n++] = v;
                    if (!*end) break;
                    q = end + 1;
                }
                break;
            }
            case 1019: cfg.isoforms = 1; break;
            case 1020: cfg.fit = 1; break;
            case 1021: cfg.presence = 1; break;
            case 1022: presence_list = optarg; break;
            case 1023: cfg.asymptotic = 1; break;
            case 1024: cfg.boundary_cut = atof(optarg); boundary_cut_given = 1; break;
            case 1025: cfg.profile = 1; break;
            case 1026: cfg.profile_level = atof(optarg); profile_level_given = 1; break;
            case 1027: profile_list = optarg; break;
            case 1028: cfg.profile_evals = atoi(optarg); if (cfg.profile_evals <= 0) { fprintf(stderr, "--profile-evals must be positive.\n"); return 1; } break;
            case 1029: cfg.compare = 1; break;
            case 1040: cfg.compare_usage = 1; break;
            case 1030: cfg.compare_ratio = atof(optarg); compare_ratio_given = 1; break;
            case 1031: compare_list = optarg; break;
            case 1009: {
                const char *q = optarg;
                while (*q && n_dev_map < 64) {
                    char *end; long d = strtol(q, &end, 10);
                    if (end == q || d < 0 || d > 1023) { fprintf(stderr, "--devices wants a comma-separated list of device ids.\n"); return 1; }
                    dev_map[n_dev_map++] = (int)d;
                    q = *end == ',' ? end + 1 : end;
                    if (*end && *end != ',') { fprintf(stderr, "--devices wants a comma-separated list of device ids.\n"); return 1; }
                }
                if (!n_dev_map) { fprintf(stderr, "--devices wants a comma-separated list of device ids.\n"); return 1; }
                break;
            }
            default: usage(argv[0]); return 1;
        }
    }
    if (cfg.bq_n > 0 && (cfg.boot_n < 1 || cfg.boot_n > 4096)) {
        fprintf(stderr, "--bootstrap-quantiles needs --bootstrap B with 1 <= B <= 4096 replicates.\n"); return 1;
    }
    if (cfg.isoforms && !cfg.g2t) { fprintf(stderr, "--isoforms needs --g2t FILE.\n"); return 1; }
    if (boundary_cut_given && !cfg.asymptotic) { fprintf(stderr, "--boundary-cut needs --asymptotic.\n"); return 1; }
    if (boundary_cut_given && !(cfg.boundary_cut >= 0.0)) { fprintf(stderr, "--boundary-cut must be >= 0.\n"); return 1; }
    if (!boundary_cut_given) cfg.boundary_cut = EMSAR_ASYM_DEFAULT_CUT;
    if (presence_list && !cfg.presence) { fprintf(stderr, "--presence-list needs --presence.\n"); return 1; }
    if ((profile_list || profile_level_given || cfg.profile_evals) && !cfg.profile) {
        fprintf(stderr, "--profile-list, --profile-level and --profile-evals need --profile.\n"); return 1;
    }
    if (profile_level_given && !(cfg.profile_level > 0.0 && cfg.profile_level < 1.0)) { fprintf(stderr, "--profile-level must lie in (0, 1).\n"); return 1; }
    if (!profile_level_given) cfg.profile_level = 0.95;
    if (compare_ratio_given && !cfg.compare) { fprintf(stderr, "--compare-ratio needs --compare.\n"); return 1; }
    if (compare_list && !cfg.compare && !cfg.compare_usage) { fprintf(stderr, "--compare-list needs --compare or --compare-usage.\n"); return 1; }
    if (cfg.compare_usage && !cfg.g2t) { fprintf(stderr, "--compare-usage needs --g2t FILE.\n"); usage(argv[0]); return 1; }
    if (compare_ratio_given && !(cfg.compare_ratio > 0.0 && isfinite(cfg.compare_ratio))) { fprintf(stderr, "--compare-ratio must be positive.\n"); return 1; }
    if (!compare_ratio_given) cfg.compare_ratio = 1.0;
    if (cfg.compare && !multisample) { fprintf(stderr, "--compare needs -M and at least two samples.\n"); usage(argv[0]); return 1; }
    if (cfg.compare_usage && !multisample) { fprintf(stderr, "--compare-usage needs -M and at least two samples.\n"); usage(argv[0]); return 1; }
    cfg.ref = &ref;
    if (!cfg.rsh_path || optind + 2 >= argc) { usage(argv[0]); return 1; }
    if (emsar_set_strand(strand, cfg.ao.pe, &cfg.ao.strand)) { fprintf(stderr, "error: invalid strand type.\n"); return 1; }
    cfg.outdir = argv[optind]; cfg.prefix = argv[optind + 1];
    const char *last = argv[optind + 2];
    char **list = NULL; int n_list = 0;
    if (!multisample) { list = (char **)malloc(sizeof(char *)); list[0] = strdup(last); n_list = 1; }
    else {
        FILE *f = fopen(last, "r");
        if (!f) { fprintf(stderr, "Can't open alignment list file.\n"); return 1; }
        char line[4096];
        while (fgets(line, sizeof line, f)) {
            size_t n = strlen(line);
            while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
            if (!n) continue;
            list = (char **)realloc(list, sizeof(char *) * (size_t)(n_list + 1));
            list[n_list++] = strdup(line);
        }
        fclose(f);
        if (!n_list) { fprintf(stderr, "No alignment files in the alignment list\n"); return 1; }
    }
    if (cfg.compare && n_list < 2) { fprintf(stderr, "--compare needs -M and at least two samples.\n"); usage(argv[0]); return 1; }
    if (cfg.compare_usage && n_list < 2) { fprintf(stderr, "--compare-usage needs -M and at least two samples.\n"); usage(argv[0]); return 1; }
    cfg.aln = list; cfg.n_aln = n_list;
    /* the reference runs `mkdir -p outdir` (emsar_main.c:284-285); find out now, not after the solve, that it cannot be written */
    {
        char tmp[4096];
        size_t n = strlen(cfg.outdir);
        if (n == 0 || n >= sizeof tmp) { fprintf(stderr, "can't create output directory %s\n", cfg.outdir); return 1; }
        memcpy(tmp, cfg.outdir, n + 1);
        for (size_t k = 1; k <= n; k++)
            if (tmp[k] == '/' || tmp[k] == 0) {
                const char keep = tmp[k];
                tmp[k] = 0;
                if (mkdir(tmp, 0777) != 0 && errno != EEXIST) { fprintf(stderr, "can't create output directory %s\n", tmp); return 1; }
                tmp[k] = keep;
            }
        if (access(cfg.outdir, W_OK | X_OK) != 0) { fprintf(stderr, "can't write to output directory %s\n", cfg.outdir); return 1; }
    }

    char err[512];
    emsar_rsh *rsh = NULL;
    double t0 = now_s();
    int rc = -1, from_cache = 0;
    char *cache_path = NULL;
    if (cfg.rsh_cache) {                       /* <rsh>.bin next to the text unless a path was given */
        size_t n = strlen(cfg.rsh_cache[0] ? cfg.rsh_cache : cfg.rsh_path) + 8;
        cache_path = (char *)malloc(n);
        if (!cache_path) { fprintf(stderr, "out of memory\n"); return 1; }
        if (cfg.rsh_cache[0]) snprintf(cache_path, n, "%s", cfg.rsh_cache); else snprintf(cache_path, n, "%s.bin", cfg.rsh_path);
        rc = emsar_rsh_read_cache(cfg.rsh_path, cache_path, &rsh, err, sizeof err);
        if (rc == 0) from_cache = 1;
        else if (cfg.verbose > 1) fprintf(stdout, "rsh cache not used (%s)\n", err);
    }
    if (rc) rc = emsar_rsh_read(cfg.rsh_path, &rsh, err, sizeof err);
    if (rc) { fprintf(stderr, "%s\n", err); return 1; }
    if (cache_path && !from_cache && emsar_rsh_write_cache(rsh, cfg.rsh_path, cache_path) != 0)
        fprintf(stderr, "warning: can't write the rsh cache %s\n", cache_path);
    if (cfg.verbose > 0 && from_cache) fprintf(stdout, "rsh: binary cache %s\n", cache_path);
    free(cache_path);
    if (cfg.verbose > 0) fprintf(stdout, "rsh: %d transcripts, %lld segments, fragment lengths %d-%d (%.2fs)\n", rsh->n_tx,
                                 (long long)rsh->n_rows, rsh->frag_min, rsh->frag_max, now_s() - t0);
    /* before any sample: an unknown name ends the run here */
    if (presence_list && read_name_list("presence", presence_list, rsh, &cfg.pres_q, &cfg.pres_nq)) { emsar_rsh_free(rsh); return 1; }
    if (profile_list && read_name_list("profile", profile_list, rsh, &cfg.prof_q, &cfg.prof_nq)) { emsar_rsh_free(rsh); return 1; }
    if (compare_list && read_name_list("compare", compare_list, rsh, &cfg.cmp_q, &cfg.cmp_nq)) { emsar_rsh_free(rsh); return 1; }
    emsar_genes *genes = NULL;
    if (cfg.g2t) {                             /* before any sample: a bad gene map ends the run here */
        if (emsar_genes_read(rsh, cfg.g2t, &genes, err, sizeof err)) { fprintf(stderr, "%s\n", err); emsar_rsh_free(rsh); return 1; }
        cfg.genes = genes;
        if (cfg.verbose > 1)
            fprintf(stdout, "g2t: %d genes; %lld g2t lines name a transcript not in the index (ignored); %d index transcripts in no gene%s\n",
                    genes->n_genes, (long long)genes->n_unknown, genes->n_unmapped, genes->n_unmapped ? " (empty geneID)" : "");
    }

    int n_workers = 1;
    if (multisample) {
        /* one worker per GPU; a probe context tells us how many devices exist without touching HIP here */
        int avail = 0;
        for (int d = 0; d < 64; d++) { emsar_hip_ctx *probe = NULL; if (emsar_hip_create(&probe, d) != 0) break; emsar_hip_destroy(probe); avail++; }
        if (avail == 0) { fprintf(stderr, "%s\n", emsar_hip_strerror(EMSAR_HIP_ERR_NO_DEVICE)); return 1; }
        if (n_dev_map) {
            for (int g = 0; g < n_dev_map; g++)
                if (dev_map[g] >= avail) { fprintf(stderr, "--devices: device %d does not exist (%d found)\n", dev_map[g], avail); return 1; }
            n_workers = n_dev_map;
        } else {
            n_workers = gpus > 0 && gpus < avail ? gpus : avail;
            for (int g = 0; g < n_workers && g < 64; g++) dev_map[g] = g;
            if (n_workers > 64) n_workers = 64;
        }
        if (n_workers > n_list) n_workers = n_list;
    }
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER; pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
    int next_model = 0; double eumacut = 0.0;
    int *status = (int *)calloc((size_t)n_list, sizeof(int));
    emsar_em_stats *stats = (emsar_em_stats *)calloc((size_t)n_list, sizeof(emsar_em_stats));
    emsar_boot_stats *bstats = (emsar_boot_stats *)calloc((size_t)n_list, sizeof(emsar_boot_stats));
    emsar_subsample_stats *sstats = (emsar_subsample_stats *)calloc((size_t)n_list, sizeof(emsar_subsample_stats));
    emsar_quantile_stats *qstats = (emsar_quantile_stats *)calloc((size_t)n_list, sizeof(emsar_quantile_stats));
    double *parse_s = (double *)calloc((size_t)n_list, sizeof(double));
    double *model_s = (double *)calloc((size_t)n_list, sizeof(double)), *host_s = (double *)calloc((size_t)n_list, sizeof(double));
    worker_arg *wa = (worker_arg *)calloc((size_t)n_workers, sizeof(worker_arg));
    pthread_t *th = (pthread_t *)calloc((size_t)n_workers, sizeof(pthread_t));
    if (!status || !stats || !bstats || !sstats || !qstats || !parse_s || !model_s || !host_s || !wa || !th) { fprintf(stderr, "out of memory\n"); return 1; }
    t0 = now_s();
    /* Workers wait at a gate until their number is final: a thread that cannot be started must not leave the others
     * waiting for samples nobody will take (the EUMAcut hand-over is in sample order). */
    int go = 0, n_started = 1;
    for (int g = 0; g < n_workers; g++)
        wa[g] = (worker_arg){&cfg, rsh, multisample ? dev_map[g] : device, n_workers, g, &mu, &cv, &next_model, &eumacut, status, stats, bstats, sstats, qstats, parse_s,
                             model_s, host_s, &go, cfg.ao, {NULL, PTHREAD_MUTEX_INITIALIZER}, NULL};
    for (int g = 1; g < n_workers; g++) {
        if (pthread_create(&th[g], NULL, worker_main, &wa[g]) != 0) { fprintf(stderr, "warning: worker %d could not be started, using %d\n", g, g); break; }
        n_started++;
    }
    /* every parallel host step of a worker gets its share of the cores: G workers x 16 reader threads each would
     * oversubscribe the host (parse and inflate pools, emsar_host_threads) */
    {
        long nc = sysconf(_SC_NPROCESSORS_ONLN);
        int share = (int)((nc < 1 ? 1 : nc) / n_started);
        emsar_host_set_thread_budget(share < 1 ? 1 : share > 16 ? 16 : share);
    }
    pthread_mutex_lock(&mu);
    n_workers = n_started;
    for (int g = 0; g < n_workers; g++) wa[g].n_workers = n_workers;
    go = 1;
    pthread_cond_broadcast(&cv);
    pthread_mutex_unlock(&mu);
    worker_main(&wa[0]);
    for (int g = 1; g < n_workers; g++) pthread_join(th[g], NULL);
    double wall = now_s() - t0;
    int bad = 0;
    for (int i = 0; i < n_list; i++) if (status[i]) bad++;
    if (cfg.stats_json) {
        FILE *f = fopen(cfg.stats_json, "w");
        if (f) {
            fprintf(f, "{\"samples\": %d, \"gpus\": %d, \"wall_s\": %.6f, \"failed\": %d, \"per_sample\": [", n_list, n_workers, wall, bad);
            for (int i = 0; i < n_list; i++) {
                fprintf(f, "%s{\"status\": %d, \"parse_s\": %.6f, \"model_s\": %.6f, \"host_s\": %.6f, \"em_passes\": %d, \"converged\": %d, \"solve_ms\": %.4f, \"kernel_ms\": %.4f, \"loglik\": %.9g, \"bytes_per_pass\": %lld, "
                           "\"sets_resident\": %d, \"sets_streamed\": %d, \"set_passes_max\": %d, \"set_passes_sum\": %lld, \"sets_build_ms\": %.4f, \"sets_kernel_ms\": %.4f",
                        i ? ", " : "", status[i], parse_s[i], model_s[i], host_s[i], stats[i].iters, stats[i].converged, stats[i].solve_ms, stats[i].kernel_ms, stats[i].loglik,
                        (long long)stats[i].bytes_per_pass, stats[i].sets_resident, stats[i].sets_streamed, stats[i].set_passes_max,
                        (long long)stats[i].set_passes_sum, stats[i].sets_build_ms, stats[i].sets_kernel_ms);
                if (cfg.boot_n > 0) {
                    const emsar_boot_stats *b = &bstats[i];
                    fprintf(f, ", \"boot_replicates\": %d, \"boot_batch\": %d, \"boot_replicates_unconverged\": %d, \"boot_set_passes_max\": %d, "
                               "\"boot_draws\": %lld, \"boot_draw_ms\": %.4f, \"boot_sets_ms\": %.4f, \"boot_stream_ms\": %.4f, \"boot_reduce_ms\": %.4f, \"boot_total_ms\": %.4f",
                            b->n_replicates, b->batch, b->replicates_unconverged, b->set_passes_max, (long long)b->draws, b->draw_ms, b->sets_ms,
                            b->stream_ms, b->reduce_ms, b->total_ms);
                }
                if (cfg.boot_n > 0 && cfg.bq_n > 0)
                    fprintf(f, ", \"bootq_quantiles\": %d, \"bootq_held_bytes\": %lld, \"bootq_ms\": %.4f", qstats[i].n_quantiles,
                            (long long)qstats[i].held_bytes, qstats[i].quantile_ms);
                if (cfg.sub_nf > 0) {
                    const emsar_subsample_stats *b = &sstats[i];
                    fprintf(f, ", \"sub_fractions\": %d, \"sub_replicates\": %d, \"sub_batch\": %d, \"sub_replicates_unconverged\": %d, "
                               "\"sub_draws\": %lld, \"sub_draw_ms\": %.4f, \"sub_sets_ms\": %.4f, \"sub_stream_ms\": %.4f, \"sub_reduce_ms\": %.4f, \"sub_total_ms\": %.4f",
                            b->n_fractions, b->n_replicates, b->batch, b->replicates_unconverged, (long long)b->draws, b->draw_ms, b->sets_ms,
                            b->stream_ms, b->reduce_ms, b->total_ms);
                }
                fprintf(f, "}");
            }
            fprintf(f, "]}\n");
            fclose(f);
        }
    }
    emsar_rsh_free(rsh);
    emsar_genes_free(genes);
    free(cfg.pres_q); free(cfg.prof_q); free(cfg.cmp_q); free(ref.R); free(ref.E); free(ref.den);
    for (int i = 0; i < n_list; i++) free(list[i]);
    free(list); free(status); free(stats); free(bstats); free(sstats); free(qstats); free(parse_s); free(model_s); free(host_s); free(wa); free(th);
    return bad ? 1 : 0;
}
