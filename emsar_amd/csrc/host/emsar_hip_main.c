/* emsar_hip_main.c -- command-line driver: the per-sample loop of the reference's main()
 * (the reference's src/emsar_main.c:380-488) with run_MLE_threads() replaced by the HIP library.  One function per analysis
 * (stage_model .. stage_subsample, called in that order by run_sample()), every file format in output.c, the argument parsers in cli_parse.h.
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
 * --profile-usage (with --g2t) answers "what could this isoform's share of its gene be": <prefix>.<i>.uprofile holds, per transcript (or per
 * transcript named in --profile-list FILE), its share, the limits of the share's profile-likelihood interval at --profile-level, the deviances
 * of the shares 0 and 1, a status word, the outer points and the inner evaluations spent (emsar_hip_profile_usage with the solve's parameters
 * and --profile-evals).  A switch of its own: --profile writes no .uprofile, and the other files do not change with it.
 * --compare (with -M and at least two samples) answers "does this isoform's abundance differ from sample 0": every sample i >= 1 writes
 * <prefix>.<i>.compare with, per transcript (or per transcript named in --compare-list FILE), its FPKM in sample i and in sample 0, log2 of their
 * ratio, the likelihood-ratio statistic Lambda of H0: theta_i = r * theta_0 (--compare-ratio r, default 1) with every sibling free in both samples,
 * its chi2_1 p-value, a status word and the evaluations spent (emsar_hip_compare with the solve's parameters: sample i is A, sample 0 is B).
 * Sample 0's solver inputs (R, E, den) are kept on the host and uploaded into a second context on each worker's device.  With --g2t every
 * sample i >= 1 also writes <prefix>.<i>.gcompare: per gene, in the order of .gfpkm, the gene sums of FPKM in sample i and in sample 0, log2 of
 * their ratio, Lambda of H0: the gene's sum in i = r * its sum in 0 with the isoforms free in both samples, p, status, evaluations and parts
 * (emsar_hip_compare_genes); --compare-list filters transcripts only.  The other files do not change with it.
 * --compare-groups g0,g1,.. (with -M; one group id per alignment file, 0 .. G-1, 2 to 32 samples) answers the question a run over many samples is
 * made for, "did this isoform change between the conditions, and do the replicates of a condition agree": after every sample has been solved,
 * ONE file <prefix>.groups holds, per transcript (or per transcript named in --compare-list FILE), the common FPKM of all samples and of each
 * group, Lambda_between (the groups differ, replicates pooled inside the likelihood) and Lambda_within (the replicates of a group disagree)
 * with their degrees of freedom and chi2 p-values, a status word, the outer points and the inner evaluations spent (emsar_hip_compare_groups
 * with the solve's parameters on K contexts on the first worker's device).  --compare-sizes s0,s1,.. gives every sample a size factor.  With
 * --g2t also ONE file <prefix>.ggroups: the same "#" line, then per gene, in the order of .gfpkm, the common gFPKM of all samples and of each
 * group and the same columns for the gene's SUM with the isoforms free in every sample, then the parts (emsar_hip_compare_groups_genes);
 * --compare-list filters transcripts only.  The other files do not change with it.
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
#include "cli_parse.h"

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
    int profile_usage;                /* --profile-usage (needs --g2t): .uprofile; takes --profile-level, --profile-evals and --profile-list */
    int compare; double compare_ratio; /* --compare [--compare-ratio r] */
    int compare_usage;                /* --compare-usage (needs --g2t): also a two-sample run, shares sample 0 with --compare */
    int32_t *cmp_q; int cmp_nq;       /* --compare-list FILE, as --presence-list */
    struct compare_ref *ref;          /* --compare: sample 0's solver inputs, shared by the workers */
    int compare_groups, n_groups, n_sizes;   /* --compare-groups g0,.. [--compare-sizes s0,..]: the ids and factors as given (up to 33 are kept) */
    int32_t group_of[33]; double group_size[33];
    struct compare_ref *inputs;       /* --compare-groups: every sample's solver inputs [n_aln], each written by the worker that runs the sample */
    const emsar_genes *genes;         /* its gene map, read once by main() and shared read-only by the workers */
    /* what only main() reads: the options as given, before the index, the lists and the devices they name have been looked at */
    const char *strand; int multisample, gpus, device;
    int dev_map[64], n_dev_map;       /* --devices */
    const char *presence_list, *profile_list, *compare_list;
    int boundary_cut_given, profile_level_given, compare_ratio_given;
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

/* --compare-groups: sample i's inputs for the stage after the workers (ready stays 0 if it failed before it had them) */
static void keep_inputs(const config *cfg, int i, const emsar_rsh *r, const int32_t *R, const double *E, const double *den) {
    compare_ref *in = &cfg->inputs[i];
    const size_t nr = (size_t)(r->n_rows > 0 ? r->n_rows : 1), nt = (size_t)(r->n_tx > 0 ? r->n_tx : 1);
    in->R = (int32_t *)malloc(nr * 4); in->E = (double *)malloc(nr * 8); in->den = (double *)malloc(nt * 8);
    if (!in->R || !in->E || !in->den) return;
    memcpy(in->R, R, (size_t)r->n_rows * 4); memcpy(in->E, E, (size_t)r->n_rows * 8); memcpy(in->den, den, (size_t)r->n_tx * 8);
    in->ready = 1;
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

/* One sample on its way through the stages below.  run_sample() calls them in a fixed order and stops at the first that fails; a stage owns
 * and frees its own buffers and reads what an earlier stage left only through the fields here, which run_sample() alone frees. */
typedef struct {
    worker_arg *w; emsar_hip_ctx *ctx; int i;      /* sample i of the job on this worker's context */
    const config *cfg; const emsar_rsh *r; const emsar_genes *G;   /* G = the gene map, NULL without --g2t */
    size_t T, NG;                                  /* transcripts, genes (0 without --g2t) */
    emsar_counts *cnt; emsar_model *m;             /* the counted alignments, taken over from the parse job; stage_model's model */
    emsar_em_params p;                             /* the solve's parameters, which every test, interval and replicate solve reuses */
    double *theta, *rounds, *mean, *sd, *ieuma, *tpm, *ir, *den; int32_t *iri;   /* stage_solve: the columns of .fpkm ([T]; rounds [n_round][T]) and den */
    double *gcols, *gsums;                         /* stage_genes: [3][T] FPKM, iReadcount, TPM and their [3][NG] gene sums */
    double *iso_u; int32_t *dom;                   /* stage_isoforms: [T] usage and [NG] dominant isoform of the .fpkm column */
    int published;                                 /* sample 0 of a two-sample job has handed its solver inputs on */
    char path[4096];                               /* the file being written */
} sample;

/* <outdir>/<prefix>.<i>.<ext> */
static const char *out_path(sample *s, const char *ext) {
    snprintf(s->path, sizeof s->path, "%s/%s.%d.%s", s->cfg->outdir, s->cfg->prefix, s->i, ext);
    return s->path;
}
/* the status of a writer that was given out_path(): reported if it failed */
static int wrote(const sample *s, int rc) {
    if (rc) fprintf(stderr, "can't write %s\n", s->path);
    return rc;
}
/* the status of a library call: reported if it failed, as "alnfile[i]: <what>: <status> (<the context's last error>)" */
static int lib_call(const sample *s, const char *what, int rc) {
    if (rc) fprintf(stderr, "alnfile[%d]: %s%s%s (%s)\n", s->i, what, *what ? ": " : "", emsar_hip_strerror(rc), emsar_hip_last_error(s->ctx));
    return rc;
}
/* n elements of `size` bytes for a stage to carve its arrays from; never a request of length 0, whose NULL would read as out of memory */
static void *slab(size_t n, size_t size) { return malloc((n ? n : 1) * size); }

/* Model preparation: compute_adjEUMA (emsar_main.c:403: L = EUMA . Wf on the device, bit-identical to the host loop) and the model.
 * EUMAcut carries over in sample order (emsar_main.c:95,418: never reset), but it only ever changes when a set exceeds 5000 transcripts
 * (emsar_main.c:417-423).  So every worker builds its model at once, without the lock, from the value it sees now; at its turn in the
 * sample order it checks that the samples before it have left that value in place and publishes its own (possibly raised) one.  Only if
 * an earlier sample did raise the cut in the meantime is the model rebuilt, at the turn, from the value that sample left.
 * Invariant: *w->next_model advances exactly once per sample whatever has failed -- run_sample() calls this stage unconditionally and the
 * hand-over below is not skipped by any rc -- or the workers behind this sample would wait for ever. */
static int stage_model(sample *s, int rc, const char *parse_err) {
    worker_arg *w = s->w; const emsar_rsh *r = s->r;
    char err[512];
    double *Ldev = NULL;
    snprintf(err, sizeof err, "%s", parse_err);
    if (rc == 0) {
        double *wf = (double *)slab((size_t)r->nfl, 8);
        Ldev = (double *)slab((size_t)r->n_rows, 8);
        if (!wf || !Ldev) rc = EMSAR_HOST_ERR_OOM;
        else if (emsar_model_wf(r, s->cnt, wf) == EMSAR_HOST_OK) {
            int hrc = emsar_hip_adj_euma(s->ctx, wf, Ldev);
            if (hrc) { snprintf(err, sizeof err, "adj_euma: %s (%s)", emsar_hip_strerror(hrc), emsar_hip_last_error(s->ctx)); rc = EMSAR_HOST_ERR_IO; }
        } else { free(Ldev); Ldev = NULL; }            /* model_build reports the empty fragment-length window */
        free(wf);
    }
    double t_model = now_s();                          /* model_s: from here to the end of the hand-over */
    pthread_mutex_lock(w->mu);
    const double cut_seen = *w->eumacut;
    pthread_mutex_unlock(w->mu);
    double cut_mine = cut_seen;
    if (rc == 0) rc = emsar_model_build_L(r, s->cnt, s->cfg->delta, &cut_mine, Ldev, &s->m, err, sizeof err);
    pthread_mutex_lock(w->mu);
    while (*w->next_model != s->i) pthread_cond_wait(w->cv, w->mu);
    if (rc == 0 && *w->eumacut != cut_seen) {
        emsar_model_free(s->m); s->m = NULL;
        cut_mine = *w->eumacut;
        rc = emsar_model_build_L(r, s->cnt, s->cfg->delta, &cut_mine, Ldev, &s->m, err, sizeof err);
    }
    if (rc == 0) *w->eumacut = cut_mine;
    (*w->next_model)++;
    pthread_cond_broadcast(w->cv);
    pthread_mutex_unlock(w->mu);
    free(Ldev);
    w->model_s[s->i] = now_s() - t_model;
    if (rc) fprintf(stderr, "alnfile[%d]=%s: %s\n", s->i, s->cfg->aln[s->i], err);
    else if (s->cfg->verbose > 0)
        fprintf(stdout, "alnfile[%d]=%s  reads=%lld (seen %lld, >k %lld, bad fraglen %lld, discrepant %lld, no segment %lld)  sets=%d  gpu=%d\n",
                s->i, s->cfg->aln[s->i], (long long)s->cnt->total_reads, (long long)s->cnt->reads_seen, (long long)s->cnt->reads_over_k,
                (long long)s->cnt->reads_bad_fraglen, (long long)s->cnt->reads_discrepant, (long long)s->cnt->reads_no_segment, s->m->n_sets, w->device);
    return rc;
}

/* den_t = sum_c m_ct E_c in row order on the host: the device's own scatter adds with atomics, whose order (and with it the last bits of
 * den, of theta and now and then the sixth printed decimal) changes from run to run; and compute_iEUMA (emsar_functions.c:3218: iEUMA_t =
 * sum of adjEUMA over the segments that hold t) in the same sweep, for the same reason: the eff.length and iReadcount columns are then
 * the same bytes in every run.  Both arrays arrive zeroed. */
static void row_sums(const emsar_rsh *r, const emsar_model *m, double *den, double *ieuma) {
    for (int64_t c = 0; c < r->n_rows; c++) {
        const double e = m->E_solver[c], l = m->L[c];
        if (e != 0.0) for (uint64_t k = r->row_ptr[c]; k < r->row_ptr[c + 1]; k++) den[r->col_idx[k]] += e;
        if (l != 0.0) for (uint64_t k = r->row_ptr[c]; k < r->row_ptr[c + 1]; k++) ieuma[r->col_idx[k]] += l;
    }
}

/* The replaced call -- run_MLE_threads() + construct_FPKMfinal, emsar_main.c:444-450 -- then compute_iEUMA + print_FPKMfinal
 * (emsar_main.c:454-460): .fpkm, .fraglength_effect and, with -g, .segments.  host_s = model_s + the row sums + the three writers. */
static int stage_solve(sample *s) {
    worker_arg *w = s->w; const config *cfg = s->cfg; const emsar_rsh *r = s->r;
    const size_t T = s->T;
    const int i = s->i;
    int rc;
    s->theta = (double *)slab(T, 8); s->mean = (double *)slab(T, 8); s->sd = (double *)slab(T, 8); s->tpm = (double *)slab(T, 8);
    s->ir = (double *)slab(T, 8); s->iri = (int32_t *)slab(T, 4); s->rounds = (double *)slab(T * (size_t)cfg->n_round, 8);
    if (!s->theta || !s->mean || !s->sd || !s->tpm || !s->ir || !s->iri || !s->rounds) return EMSAR_HOST_ERR_OOM;
    double t_host = now_s();
    s->den = (double *)calloc(T ? T : 1, sizeof(double)); s->ieuma = (double *)calloc(T ? T : 1, sizeof(double));
    if (!s->den || !s->ieuma) return EMSAR_HOST_ERR_OOM;
    row_sums(r, s->m, s->den, s->ieuma);
    w->host_s[i] = w->model_s[i] + (now_s() - t_host);
    /* Invariant: with --compare or --compare-usage sample 0 publishes its inputs exactly once -- the arrays here, or, if it ends before
     * this line, the failure marker in run_sample() -- so that no other sample waits for them in vain. */
    if ((cfg->compare || cfg->compare_usage) && i == 0) { publish_ref(w, r, s->cnt->R, s->m->E_solver, s->den); s->published = 1; }
    if (cfg->compare_groups) keep_inputs(cfg, i, r, s->cnt->R, s->m->E_solver, s->den);
    if ((rc = lib_call(s, "", emsar_hip_upload_sample(s->ctx, s->cnt->R, s->m->E_solver, s->den))) ||
        (rc = lib_call(s, "", emsar_hip_solve(s->ctx, &s->p, s->theta, &w->stats[i])))) return rc;
    for (int k = 0; k < cfg->n_round; k++) memcpy(s->rounds + (size_t)k * T, s->theta, T * 8);   /* deterministic solver: rounds coincide */
    emsar_mean_sd(r->n_tx, cfg->n_round, s->rounds, s->mean, s->sd);
    if ((rc = lib_call(s, "", emsar_hip_normalise(s->ctx, s->mean, s->ieuma, s->cnt->total_reads, s->tpm, s->ir, s->iri)))) return rc;
    int64_t tot = 0;
    t_host = now_s();
    if ((rc = wrote(s, emsar_write_fpkm(out_path(s, "fpkm"), r, s->mean, s->sd, s->ieuma, s->ir, s->iri, s->tpm, &tot)))) return rc;
    if (cfg->verbose > 0) fprintf(stdout, "Total inferred readcount=%lld\n", (long long)tot);
    if ((rc = wrote(s, emsar_write_fraglength(out_path(s, "fraglength_effect"), r, s->cnt, s->m)))) return rc;
    if (cfg->print_segments && (rc = wrote(s, emsar_write_segments(out_path(s, "segments"), r, s->cnt, s->m, s->mean)))) return rc;
    w->host_s[i] += now_s() - t_host;
    return 0;
}

/* Gene level (--g2t): FPKM2gFPKM.pl's sums of columns FPKM, iReadcount and TPM per gene, on the device: .gfpkm */
static int stage_genes(sample *s) {
    const size_t T = s->T, NG = s->NG;
    int rc;
    s->gcols = (double *)slab(3 * T, 8); s->gsums = (double *)slab(3 * NG, 8);
    if (!s->gcols || !s->gsums) return EMSAR_HOST_ERR_OOM;
    memcpy(s->gcols, s->mean, T * 8); memcpy(s->gcols + T, s->ir, T * 8); memcpy(s->gcols + 2 * T, s->tpm, T * 8);
    if ((rc = lib_call(s, "gene sums", emsar_hip_gene_sums(s->ctx, 3, s->gcols, s->gsums)))) return rc;
    return wrote(s, emsar_write_gfpkm(out_path(s, "gfpkm"), s->G, s->gsums, s->gsums + NG, s->gsums + 2 * NG));
}

/* Isoform usage (--isoforms): each transcript's share of its gene's FPKM and the gene's dominant isoform, on the device.  .isoforms is
 * written here unless a bootstrap follows: stage_bootstrap writes it then, with the replicates' columns next to these. */
static int stage_isoforms(sample *s) {
    int rc;
    s->iso_u = (double *)slab(s->T, 8); s->dom = (int32_t *)slab(s->NG, 4);
    if (!s->iso_u || !s->dom) return EMSAR_HOST_ERR_OOM;
    if ((rc = lib_call(s, "isoform usage", emsar_hip_isoform_usage(s->ctx, 1, s->mean, s->iso_u, s->dom))) || s->cfg->boot_n > 0) return rc;
    return wrote(s, emsar_write_isoforms(out_path(s, "isoforms"), s->r, s->G, s->mean, s->iso_u, s->dom, 0, NULL, NULL, NULL, 0, NULL, NULL));
}

/* Model fit (--fit): the residuals of the printed FPKM against the sample's segments, per transcript and per gene, on the device: .fit, .gfit */
static int stage_fit(sample *s) {
    const size_t T = s->T, NG = s->NG;
    double *fv = (double *)slab(4 * T, 8), *gv = s->G ? (double *)slab(4 * NG, 8) : NULL;
    int32_t *fw = (int32_t *)slab(T, 4);
    int rc = fv && fw && (gv || !s->G) ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_fit_outputs o = {.tx_chi2 = fv, .tx_dev = fv + T, .tx_miss = fv + 2 * T, .tx_df = fv + 3 * T, .tx_worst_row = fw,
                                     .gene_chi2 = gv, .gene_dev = gv ? gv + NG : NULL, .gene_miss = gv ? gv + 2 * NG : NULL, .gene_df = gv ? gv + 3 * NG : NULL};
        if (!(rc = lib_call(s, "model fit", emsar_hip_model_fit(s->ctx, s->mean, s->m->E_solver, &o, NULL))) &&
            !(rc = wrote(s, emsar_write_fit(out_path(s, "fit"), s->r, s->mean, s->den, o.tx_df, o.tx_chi2, o.tx_dev, o.tx_miss, o.tx_worst_row))) && s->G)
            rc = wrote(s, emsar_write_gfit(out_path(s, "gfit"), s->r, s->G, s->mean, s->den, o.gene_df, o.gene_chi2, o.gene_dev, o.gene_miss));
    }
    free(fv); free(gv); free(fw);
    return rc;
}

/* Presence test (--presence): one likelihood-ratio test per transcript on its connected set, on the device: .presence */
static int stage_presence(sample *s) {
    const int32_t *query = s->cfg->pres_q;
    const size_t Q = query ? (size_t)s->cfg->pres_nq : s->T;
    double *v = (double *)slab(3 * Q, 8);
    int32_t *iv = (int32_t *)slab(2 * Q, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_presence_outputs o = {.lambda = v, .pvalue = v + Q, .heir_share = v + 2 * Q, .heir = iv, .status = iv + Q};
        if (!(rc = lib_call(s, "presence", emsar_hip_presence(s->ctx, &s->p, (int32_t)Q, query, &o, NULL))))
            rc = wrote(s, emsar_write_presence(out_path(s, "presence"), s->r, (int32_t)Q, query, s->mean, o.lambda, o.pvalue, o.status, o.heir, o.heir_share));
    }
    free(v); free(iv);
    return rc;
}

/* --profile with --g2t: the same question per gene, and whether the gene is needed at all (emsar_hip_profile_genes; --profile-list names
 * transcripts and does not filter it): .gprofile */
static int profile_genes(sample *s, const emsar_profile_params *pp) {
    const size_t NG = s->NG;
    double *v = (double *)slab(4 * NG, 8);
    int32_t *iv = (int32_t *)slab(2 * NG, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_profile_gene_outputs o = {.lower = v, .upper = v + NG, .lambda = v + 2 * NG, .pvalue = v + 3 * NG, .status = iv, .members = iv + NG};
        if (!(rc = lib_call(s, "profile_genes", emsar_hip_profile_genes(s->ctx, &s->p, pp, (int32_t)NG, NULL, &o, NULL))))
            rc = wrote(s, emsar_write_gprofile(out_path(s, "gprofile"), s->G, s->gsums, o.lower, o.upper, o.lambda, o.pvalue, o.members, o.status));
    }
    free(v); free(iv);
    return rc;
}

/* Profile-likelihood intervals (--profile): two confidence limits per transcript on its connected set, on the device: .profile, then .gprofile */
static int stage_profile(sample *s) {
    const int32_t *query = s->cfg->prof_q;
    const size_t Q = query ? (size_t)s->cfg->prof_nq : s->T;
    const emsar_profile_params pp = {.level = s->cfg->profile_level, .max_evals = s->cfg->profile_evals};
    double *v = (double *)slab(3 * Q, 8);
    int32_t *iv = (int32_t *)slab(Q, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_profile_outputs o = {.lower = v, .upper = v + Q, .lambda = v + 2 * Q, .status = iv};
        if (!(rc = lib_call(s, "profile", emsar_hip_profile(s->ctx, &s->p, &pp, (int32_t)Q, query, &o, NULL))))
            rc = wrote(s, emsar_write_profile(out_path(s, "profile"), s->r, (int32_t)Q, query, s->mean, o.lower, o.upper, o.lambda, o.status));
    }
    free(v); free(iv);
    return !rc && s->G ? profile_genes(s, &pp) : rc;
}

/* Profile-likelihood intervals of isoform usage (--profile-usage --g2t): two limits of each transcript's share of its gene: .uprofile */
static int stage_profile_usage(sample *s) {
    const int32_t *query = s->cfg->prof_q;
    const size_t Q = query ? (size_t)s->cfg->prof_nq : s->T;
    const emsar_profile_params pp = {.level = s->cfg->profile_level, .max_evals = s->cfg->profile_evals};
    double *v = (double *)slab(5 * Q, 8);
    int32_t *iv = (int32_t *)slab(3 * Q, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_profile_usage_outputs o = {.usage = v, .lower = v + Q, .upper = v + 2 * Q, .lambda_zero = v + 3 * Q, .lambda_one = v + 4 * Q,
                                               .status = iv, .outer_evals = iv + Q, .evals = iv + 2 * Q};
        if (!(rc = lib_call(s, "profile_usage", emsar_hip_profile_usage(s->ctx, &s->p, &pp, (int32_t)Q, query, &o, NULL))))
            rc = wrote(s, emsar_write_uprofile(out_path(s, "uprofile"), s->r, s->G, (int32_t)Q, query, o.usage, o.lower, o.upper, o.lambda_zero,
                                               o.lambda_one, o.status, o.outer_evals, o.evals));
    }
    free(v); free(iv);
    return rc;
}

/* Two-sample tests: sample 0 in a second context on this worker's device, made on the first sample that needs it and kept by the worker */
static int reference_context(sample *s) {
    worker_arg *w = s->w; const emsar_rsh *r = s->r;
    compare_ref *ref = s->cfg->ref;
    emsar_hip_ctx *c = NULL;
    int rc;
    pthread_mutex_lock(w->mu);
    while (!ref->ready) pthread_cond_wait(w->cv, w->mu);
    const int have_ref = ref->ready > 0;
    pthread_mutex_unlock(w->mu);
    if (!have_ref) { fprintf(stderr, "alnfile[%d]: compare: sample 0 gave no solver inputs\n", s->i); return EMSAR_HOST_ERR_IO; }
    if (w->ref_ctx) return 0;
    if ((rc = emsar_hip_create(&c, w->device)) || (rc = emsar_hip_set_deterministic(c, !s->cfg->no_deterministic)) ||
        (rc = emsar_hip_upload_structure(c, r->n_rows, r->n_tx, r->row_ptr, r->col_idx, EMSAR_LAYOUT_AUTO)) ||
        (rc = emsar_hip_upload_sample(c, ref->R, ref->E, ref->den))) {
        fprintf(stderr, "alnfile[%d]: compare: sample 0's context: %s (%s)\n", s->i, emsar_hip_strerror(rc), c ? emsar_hip_last_error(c) : "");
        emsar_hip_destroy(c);
        return rc;
    }
    w->ref_ctx = c;
    return 0;
}

/* --compare-usage: the share of its gene (emsar_hip_compare_usage: this context's gene map serves both samples): .ucompare */
static int compare_usage(sample *s, size_t Q, const int32_t *query) {
    double *v = (double *)slab(5 * Q, 8);
    int32_t *iv = (int32_t *)slab(3 * Q, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_usage_outputs o = {.lambda = v, .pvalue = v + Q, .usage_a = v + 2 * Q, .usage_b = v + 3 * Q, .dlogit = v + 4 * Q,
                                       .status = iv, .outer_evals = iv + Q, .evals = iv + 2 * Q};
        if (!(rc = lib_call(s, "compare_usage", emsar_hip_compare_usage(s->ctx, s->w->ref_ctx, &s->p, NULL, (int32_t)Q, query, &o, NULL))))
            rc = wrote(s, emsar_write_ucompare(out_path(s, "ucompare"), s->r, s->G, (int32_t)Q, query, o.usage_a, o.usage_b, o.dlogit, o.lambda, o.pvalue,
                                               o.status, o.outer_evals, o.evals));
    }
    free(v); free(iv);
    return rc;
}

/* --compare: the abundance (emsar_hip_compare): .compare */
static int compare_transcripts(sample *s, const emsar_compare_params *cp, size_t Q, const int32_t *query) {
    double *v = (double *)slab(5 * Q, 8);
    int32_t *iv = (int32_t *)slab(2 * Q, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_compare_outputs o = {.lambda = v, .pvalue = v + Q, .log2fc = v + 2 * Q, .theta_a = v + 3 * Q, .theta_b = v + 4 * Q, .status = iv, .evals = iv + Q};
        if (!(rc = lib_call(s, "compare", emsar_hip_compare(s->ctx, s->w->ref_ctx, &s->p, cp, (int32_t)Q, query, &o, NULL))))
            rc = wrote(s, emsar_write_compare(out_path(s, "compare"), s->r, (int32_t)Q, query, o.theta_a, o.theta_b, o.log2fc, o.lambda, o.pvalue, o.status, o.evals));
    }
    free(v); free(iv);
    return rc;
}

/* --compare with --g2t: the same question per gene (emsar_hip_compare_genes: this context's gene map serves both samples; --compare-list
 * names transcripts and does not filter it): .gcompare */
static int compare_genes(sample *s, const emsar_compare_params *cp) {
    const size_t NG = s->NG;
    double *v = (double *)slab(5 * NG, 8);
    int32_t *iv = (int32_t *)slab(3 * NG, 4);
    int rc = v && iv ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_compare_gene_outputs o = {.lambda = v, .pvalue = v + NG, .log2fc = v + 2 * NG, .gene_a = v + 3 * NG, .gene_b = v + 4 * NG,
                                              .status = iv, .evals = iv + NG, .parts = iv + 2 * NG};
        if (!(rc = lib_call(s, "compare_genes", emsar_hip_compare_genes(s->ctx, s->w->ref_ctx, &s->p, cp, (int32_t)NG, NULL, &o, NULL))))
            rc = wrote(s, emsar_write_gcompare(out_path(s, "gcompare"), s->G, o.gene_a, o.gene_b, o.log2fc, o.lambda, o.pvalue, o.status, o.evals, o.parts));
    }
    free(v); free(iv);
    return rc;
}

/* Two-sample tests (--compare, --compare-usage; every sample but the first): this sample (A) against sample 0 (B), on the device */
static int stage_two_sample(sample *s) {
    const config *cfg = s->cfg;
    const int32_t *query = cfg->cmp_q;
    const size_t Q = query ? (size_t)cfg->cmp_nq : s->T;
    const emsar_compare_params cp = {.ratio = cfg->compare_ratio};
    int rc = reference_context(s);
    if (!rc && cfg->compare_usage) rc = compare_usage(s, Q, query);
    if (!rc && cfg->compare) rc = compare_transcripts(s, &cp, Q, query);
    if (!rc && cfg->compare && s->G) rc = compare_genes(s, &cp);
    return rc;
}

/* Asymptotic standard errors (--asymptotic): the inverse of the observed information at the printed FPKM, on the device: .asym, .gasym */
static int stage_asymptotic(sample *s) {
    const size_t T = s->T, NG = s->NG;
    double *v = (double *)slab(5 * T, 8), *gv = s->G ? (double *)slab(NG, 8) : NULL;
    int32_t *iv = (int32_t *)slab(2 * T, 4), *gi = s->G ? (int32_t *)slab(NG, 4) : NULL;
    int rc = v && iv && (!s->G || (gv && gi)) ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const emsar_asym_params ap = {.boundary_cut = s->cfg->boundary_cut, .block_tid = -1};
        const emsar_asym_outputs o = {.var = v, .sd_fpkm = v + T, .sd_tpm = v + 2 * T, .partner_cov = v + 3 * T, .usage_sd = s->G ? v + 4 * T : NULL,
                                      .status = iv, .partner = iv + T, .gene_sd = gv, .gene_status = gi};
        if (!(rc = lib_call(s, "asymptotic", emsar_hip_asymptotic(s->ctx, s->mean, &ap, &o, NULL))) &&
            !(rc = wrote(s, emsar_write_asym(out_path(s, "asym"), s->r, s->mean, s->tpm, o.sd_fpkm, o.sd_tpm, o.var, o.status, o.partner, o.partner_cov,
                                             o.usage_sd))) && s->G)
            rc = wrote(s, emsar_write_gasym(out_path(s, "gasym"), s->G, s->gsums, gv, gi));
    }
    free(v); free(gv); free(iv); free(gi);
    return rc;
}

/* what stage_bootstrap asked the library for: mean and sd of FPKM and sd of TPM [T]; with --g2t the same per gene [NG]; with
 * --bootstrap-quantiles the quantiles of FPKM and of TPM [n_q][T] and per gene [n_q][NG]; with --isoforms the usage statistics */
typedef struct { double *mean, *sd, *tpm_sd, *g_mean, *g_sd, *g_tpm_sd, *q_fpkm, *q_tpm, *gq_fpkm, *gq_tpm; emsar_isoform_outputs iso; } boot_arrays;

/* .bootstrap, and what the options add to it: .gbootstrap, .bootq, .gbootq, .isoforms */
static int write_bootstrap_files(sample *s, const boot_arrays *b, int iso) {
    const config *cfg = s->cfg;
    int rc = wrote(s, emsar_write_bootstrap(out_path(s, "bootstrap"), s->r, s->mean, b->mean, b->sd, s->tpm, b->tpm_sd));
    if (!rc && s->G)
        rc = wrote(s, emsar_write_gbootstrap(out_path(s, "gbootstrap"), s->G, s->gsums, b->g_mean, b->g_sd, s->gsums + 2 * s->NG, b->g_tpm_sd));
    if (!rc && cfg->bq_n) rc = wrote(s, emsar_write_bootq(out_path(s, "bootq"), s->r, cfg->bq_n, cfg->bq, b->q_fpkm, b->q_tpm));
    if (!rc && cfg->bq_n && s->G) rc = wrote(s, emsar_write_gbootq(out_path(s, "gbootq"), s->G, cfg->bq_n, cfg->bq, b->gq_fpkm, b->gq_tpm));
    if (!rc && iso)
        rc = wrote(s, emsar_write_isoforms(out_path(s, "isoforms"), s->r, s->G, s->mean, s->iso_u, s->dom, cfg->boot_n, b->iso.usage_mean, b->iso.usage_sd,
                                           b->iso.dominant_count, cfg->bq_n, cfg->bq, b->iso.usage_q));
    return rc;
}

/* Poisson bootstrap (--bootstrap B): its own file; .fpkm keeps the reference's column 3.  With --g2t the same replicates give the genes' sd
 * as well (bootstrap_genes: the transcript outputs are the same bits as bootstrap's), with --bootstrap-quantiles the percentiles
 * (bootstrap_quantiles) and with --isoforms the usage statistics (bootstrap_isoforms: every other output is the same bits) */
static int stage_bootstrap(sample *s) {
    const config *cfg = s->cfg; worker_arg *w = s->w;
    const size_t T = s->T, NG = s->NG, NQ = (size_t)cfg->bq_n;
    const int i = s->i, iso = s->G && cfg->isoforms;
    const uint64_t seed = cfg->boot_seed + (uint64_t)i;
    double *tv = (double *)slab(3 * T, 8), *gv = s->G ? (double *)slab(3 * NG, 8) : NULL;
    double *tq = NQ ? (double *)slab(2 * NQ * T, 8) : NULL, *gq = NQ && s->G ? (double *)slab(2 * NQ * NG, 8) : NULL;
    double *uv = iso ? (double *)slab((2 + NQ) * T, 8) : NULL;
    int32_t *uc = iso ? (int32_t *)slab(T, 4) : NULL;
    int rc = tv && (gv || !s->G) && (tq || !NQ) && (gq || !NQ || !s->G) && (!iso || (uv && uc)) ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        const boot_arrays b = {.mean = tv, .sd = tv + T, .tpm_sd = tv + 2 * T, .g_mean = gv, .g_sd = gv ? gv + NG : NULL, .g_tpm_sd = gv ? gv + 2 * NG : NULL,
                               .q_fpkm = tq, .q_tpm = tq ? tq + NQ * T : NULL, .gq_fpkm = gq, .gq_tpm = gq ? gq + NQ * NG : NULL,
                               .iso = {.usage_mean = uv, .usage_sd = uv ? uv + T : NULL, .dominant_count = uc, .usage_q = uv && NQ ? uv + 2 * T : NULL}};
        rc = iso ? emsar_hip_bootstrap_isoforms(s->ctx, &s->p, seed, 0, cfg->boot_n, cfg->bq_n, cfg->bq, b.mean, b.sd, b.tpm_sd, NULL, NULL, b.q_fpkm, b.q_tpm,
                                                b.g_mean, b.g_sd, b.g_tpm_sd, b.gq_fpkm, b.gq_tpm, &w->bstats[i], &w->qstats[i], &b.iso)
           : NQ ? emsar_hip_bootstrap_quantiles(s->ctx, &s->p, seed, 0, cfg->boot_n, cfg->bq_n, cfg->bq, b.mean, b.sd, b.tpm_sd, NULL, NULL, b.q_fpkm, b.q_tpm,
                                                b.g_mean, b.g_sd, b.g_tpm_sd, b.gq_fpkm, b.gq_tpm, &w->bstats[i], &w->qstats[i])
           : s->G ? emsar_hip_bootstrap_genes(s->ctx, &s->p, seed, 0, cfg->boot_n, b.mean, b.sd, b.tpm_sd, NULL, b.g_mean, b.g_sd, b.g_tpm_sd, &w->bstats[i])
           : emsar_hip_bootstrap(s->ctx, &s->p, seed, 0, cfg->boot_n, b.mean, b.sd, b.tpm_sd, NULL, &w->bstats[i]);
        if (!(rc = lib_call(s, "bootstrap", rc))) rc = write_bootstrap_files(s, &b, iso);
    }
    free(tv); free(gv); free(tq); free(gq); free(uv); free(uc);
    return rc;
}

/* Depth subsampling (--subsample f1,f2,..): its own files, .saturation and .gsaturation */
static int stage_subsample(sample *s) {
    const config *cfg = s->cfg;
    const size_t T = s->T, NG = s->NG, K = (size_t)cfg->sub_nf;
    const uint64_t seed = cfg->sub_seed + (uint64_t)s->i;
    double *v = (double *)slab(4 * K * T, 8), *gv = s->G ? (double *)slab(3 * K * NG, 8) : NULL;
    double depth[64];
    int rc = v && (gv || !s->G) ? 0 : EMSAR_HOST_ERR_OOM;
    if (!rc) {
        double *fpkm_mean = v, *fpkm_sd = v + K * T, *tpm_mean = v + 2 * K * T, *tpm_sd = v + 3 * K * T;
        double *g_mean = gv, *g_sd = gv ? gv + K * NG : NULL, *g_tpm = gv ? gv + 2 * K * NG : NULL;
        if (!(rc = lib_call(s, "subsample", emsar_hip_subsample(s->ctx, &s->p, seed, cfg->sub_nf, cfg->sub_f, cfg->sub_reps, fpkm_mean, fpkm_sd, tpm_mean, tpm_sd,
                                                                depth, NULL, g_mean, g_sd, g_tpm, &s->w->sstats[s->i]))) &&
            !(rc = wrote(s, emsar_write_saturation(out_path(s, "saturation"), s->r, s->mean, s->tpm, cfg->sub_nf, cfg->sub_f, cfg->sub_reps, seed, depth,
                                                   fpkm_mean, fpkm_sd, tpm_mean, tpm_sd))) && s->G)
            rc = wrote(s, emsar_write_gsaturation(out_path(s, "gsaturation"), s->G, s->gsums, s->gsums + 2 * NG, cfg->sub_nf, cfg->sub_f, cfg->sub_reps, seed,
                                                  depth, g_mean, g_sd, g_tpm));
    }
    free(v); free(gv);
    return rc;
}

/* One sample: the stages in the order of the files' dependencies.  Invariant: the first stage that fails ends the sample -- every later
 * call is behind !rc -- and the files written before it stay.  The sample's arrays are freed here and nowhere else. */
static int run_sample(worker_arg *w, emsar_hip_ctx *ctx, int i, parse_job *parsed) {
    const config *cfg = w->cfg;
    sample s = {.w = w, .ctx = ctx, .i = i, .cfg = cfg, .r = w->rsh, .G = cfg->genes, .T = (size_t)w->rsh->n_tx,
                .NG = cfg->genes ? (size_t)cfg->genes->n_genes : 0, .cnt = parsed->cnt,
                .p = {.max_iter = cfg->max_iter, .accel = cfg->accel, .tol = cfg->tol, .set_mode = cfg->set_mode, .count_floor = cfg->count_floor,
                      .zero_cut = cfg->zero_cut, .abs_step = cfg->abs_step}};
    parsed->cnt = NULL;
    w->parse_s[i] = parsed->secs;
    int rc = stage_model(&s, parsed->rc, parsed->err);
    if (!rc) rc = stage_solve(&s);
    if (!rc && s.G) rc = stage_genes(&s);
    if (!rc && s.G && cfg->isoforms) rc = stage_isoforms(&s);
    if (!rc && cfg->fit) rc = stage_fit(&s);
    if (!rc && cfg->presence) rc = stage_presence(&s);
    if (!rc && cfg->profile) rc = stage_profile(&s);
    if (!rc && cfg->profile_usage) rc = stage_profile_usage(&s);
    if (!rc && (cfg->compare || cfg->compare_usage) && i > 0) rc = stage_two_sample(&s);
    if (!rc && cfg->asymptotic) rc = stage_asymptotic(&s);
    if (!rc && cfg->boot_n > 0) rc = stage_bootstrap(&s);
    if (!rc && cfg->sub_nf > 0) rc = stage_subsample(&s);
    if (!rc && cfg->verbose > 0)
        fprintf(stdout, "Complete: %s/%s.%d.fpkm  (EM passes %d, converged %d, solve %.1f ms, logL %.6f)\n", cfg->outdir, cfg->prefix, i,
                w->stats[i].iters, w->stats[i].converged, w->stats[i].solve_ms, w->stats[i].loglik);
    if ((cfg->compare || cfg->compare_usage) && i == 0 && !s.published) publish_ref(w, s.r, NULL, NULL, NULL);     /* the other samples must not wait for it */
    free(s.theta); free(s.rounds); free(s.mean); free(s.sd); free(s.ieuma); free(s.tpm); free(s.ir); free(s.iri); free(s.den);
    free(s.gcols); free(s.gsums); free(s.iso_u); free(s.dom);
    emsar_counts_free(s.cnt); emsar_model_free(s.m);
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

/* K-sample test (--compare-groups), after every worker has joined: K contexts on `device` hold the samples' solver inputs, one call
 * (emsar_hip_compare_groups with the solve's parameters) answers for all of them: <prefix>.groups.  With --g2t the first context takes the
 * gene map and a second call (emsar_hip_compare_groups_genes, every gene; --compare-list names transcripts and does not filter it) answers
 * per gene: <prefix>.ggroups */
static int stage_groups(const config *cfg, const emsar_rsh *r, int device) {
    const int K = cfg->n_aln;
    const int32_t *query = cfg->cmp_q;
    const size_t Q = query ? (size_t)cfg->cmp_nq : (size_t)r->n_tx;
    const size_t NG = cfg->genes ? (size_t)cfg->genes->n_genes : 0;
    const double *size = cfg->n_sizes ? cfg->group_size : NULL;
    int32_t G = 0;
    for (int k = 0; k < K; k++) {
        if (!cfg->inputs[k].ready) { fprintf(stderr, "compare-groups: sample %d gave no solver inputs\n", k); return EMSAR_HOST_ERR_IO; }
        if (cfg->group_of[k] + 1 > G) G = cfg->group_of[k] + 1;
    }
    const emsar_em_params p = {.max_iter = cfg->max_iter, .accel = cfg->accel, .tol = cfg->tol, .set_mode = cfg->set_mode, .count_floor = cfg->count_floor,
                               .zero_cut = cfg->zero_cut, .abs_step = cfg->abs_step};
    emsar_hip_ctx *ctx[32] = {0};
    double *v = (double *)slab((6 + (size_t)G) * Q, 8), *gv = cfg->genes ? (double *)slab((5 + (size_t)G) * NG, 8) : NULL;
    int32_t *iv = (int32_t *)slab(3 * Q, 4), *gi = cfg->genes ? (int32_t *)slab(4 * NG, 4) : NULL;
    int rc = v && iv && (!cfg->genes || (gv && gi)) ? 0 : EMSAR_HOST_ERR_OOM;
    for (int k = 0; k < K && !rc; k++) {
        const compare_ref *in = &cfg->inputs[k];
        if ((rc = emsar_hip_create(&ctx[k], device)) || (rc = emsar_hip_set_deterministic(ctx[k], !cfg->no_deterministic)) ||
            (rc = emsar_hip_upload_structure(ctx[k], r->n_rows, r->n_tx, r->row_ptr, r->col_idx, EMSAR_LAYOUT_AUTO)) ||
            (rc = emsar_hip_upload_sample(ctx[k], in->R, in->E, in->den)))
            fprintf(stderr, "compare-groups: sample %d's context: %s (%s)\n", k, emsar_hip_strerror(rc), ctx[k] ? emsar_hip_last_error(ctx[k]) : "");
    }
    if (!rc) {
        const emsar_groups_outputs o = {.theta_common = v, .lambda_between = v + Q, .p_between = v + 2 * Q, .lambda_within = v + 3 * Q, .p_within = v + 4 * Q,
                                        .theta_group = v + 6 * Q, .status = iv, .outer = iv + Q, .evals = iv + 2 * Q};
        char path[4096];
        snprintf(path, sizeof path, "%s/%s.groups", cfg->outdir, cfg->prefix);
        rc = emsar_hip_compare_groups(ctx, K, cfg->group_of, size, &p, NULL, (int32_t)Q, query, &o, NULL);
        if (rc) fprintf(stderr, "compare-groups: %s (%s)\n", emsar_hip_strerror(rc), emsar_hip_last_error(ctx[0]));
        else if ((rc = emsar_write_groups(path, r, (int32_t)Q, query, K, cfg->group_of, size, o.theta_common, o.theta_group,
                                          o.lambda_between, o.p_between, o.lambda_within, o.p_within, o.status, o.outer, o.evals)))
            fprintf(stderr, "can't write %s\n", path);
    }
    if (!rc && cfg->genes) {
        const emsar_groups_gene_outputs o = {.gene_common = gv, .lambda_between = gv + NG, .p_between = gv + 2 * NG, .lambda_within = gv + 3 * NG,
                                             .p_within = gv + 4 * NG, .gene_group = gv + 5 * NG, .status = gi, .outer = gi + NG, .evals = gi + 2 * NG,
                                             .parts = gi + 3 * NG};
        char path[4096];
        snprintf(path, sizeof path, "%s/%s.ggroups", cfg->outdir, cfg->prefix);
        if ((rc = emsar_hip_set_gene_map(ctx[0], cfg->genes->n_genes, cfg->genes->gene_of_tx)) ||
            (rc = emsar_hip_compare_groups_genes(ctx, K, cfg->group_of, size, &p, NULL, (int32_t)NG, NULL, &o, NULL)))
            fprintf(stderr, "compare-groups (genes): %s (%s)\n", emsar_hip_strerror(rc), emsar_hip_last_error(ctx[0]));
        else if ((rc = emsar_write_ggroups(path, cfg->genes, K, cfg->group_of, size, o.gene_common, o.gene_group, o.lambda_between, o.p_between,
                                           o.lambda_within, o.p_within, o.status, o.outer, o.evals, o.parts)))
            fprintf(stderr, "can't write %s\n", path);
    }
    for (int k = 0; k < K; k++) emsar_hip_destroy(ctx[k]);
    free(v); free(iv); free(gv); free(gi);
    return rc;
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
            "      --profile-usage       with --g2t: also write <prefix>.<i>.uprofile: per transcript its share of its gene, the lower and upper limit of\n"
            "                            the share's profile-likelihood interval, the deviances of the shares 0 and 1, a status word (TWO_SIDED, LOWER_ZERO,\n"
            "                            UPPER_ONE, UNIT, UNDEFINED, SINGLE, OUTSIDE, NOT_RESIDENT, TOO_LARGE, UNCONVERGED), the outer points and the inner\n"
            "                            evaluations spent; takes --profile-level, --profile-evals and --profile-list as --profile does\n"
            "      --compare             with -M and at least two samples: every sample i >= 1 also writes <prefix>.<i>.compare: per transcript its FPKM\n"
            "                            in sample i and in sample 0, log2 of the ratio, the likelihood-ratio statistic Lambda of equal abundance\n"
            "                            (siblings free in both samples), its p-value, a status word (TESTED, BOTH_ABSENT, OUTSIDE, NOT_RESIDENT,\n"
            "                            UNCONVERGED) and the evaluations spent; with --g2t also <prefix>.<i>.gcompare: per gene, in the order of\n"
            "                            .gfpkm, the same test of the gene's summed FPKM with its isoforms free (status TOO_LARGE: more than 64\n"
            "                            connected sets and lone transcripts in one sample), the evaluations and the parts searched over\n"
            "      --compare-ratio <r>   with --compare: test theta_i = r * theta_0 (default 1; a fold change or a size factor)\n"
            "      --compare-list <file> with --compare or --compare-usage: only the transcripts named in the file, one name per line\n"
            "      --compare-groups <g0,g1,..>  with -M and 2 to 32 samples: one group id (0 .. G-1) per alignment file; after all samples ONE file\n"
            "                            <prefix>.groups: per transcript the common FPKM of all samples and of each group, Lambda_between (the groups\n"
            "                            differ, replicates pooled inside the likelihood) and Lambda_within (the replicates of a group disagree), their\n"
            "                            degrees of freedom and chi2 p-values, a status word (TESTED, ALL_ABSENT, OUTSIDE, NOT_RESIDENT, UNCONVERGED), outer\n"
            "                            points and evaluations.  No over-dispersion is modelled: a large Lambda_within makes p_between anti-conservative.\n"
            "                            With --g2t also ONE file <prefix>.ggroups: per gene, in the order of .gfpkm, the same columns for the gene's summed\n"
            "                            FPKM with its isoforms free in every sample (also TOO_LARGE), and the parts searched over\n"
            "      --compare-sizes <s0,s1,..>   with --compare-groups: one positive size factor per sample (default 1); --compare-list filters it too\n"
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

static int bad(const char *msg) { fprintf(stderr, "%s\n", msg); return 1; }
static int bad_usage(const char *msg, const char *a0) { bad(msg); usage(a0); return 1; }

/* The option switch: 0, or 1 after the message of the first argument that is wrong (the usage text for an unknown option). */
static int parse_options(int argc, char **argv, config *cfg) {
    static struct option lo[] = {
        {"rsh", required_argument, 0, 'I'}, {"PE", no_argument, 0, 'P'}, {"strand_type", required_argument, 0, 's'},
        {"maxthread", required_argument, 0, 'p'}, {"max_repeat", required_argument, 0, 'k'}, {"nround", required_argument, 0, 'n'},
        {"epsilon", required_argument, 0, 'e'}, {"max_niter_mle", required_argument, 0, 'i'}, {"delta", required_argument, 0, 'd'},
        {"print_segments", no_argument, 0, 'g'}, {"multisample", no_argument, 0, 'M'}, {"SAM", no_argument, 0, 'S'}, {"BAM", no_argument, 0, 'B'},
        {"verbose", no_argument, 0, 'v'}, {"no_verbose", no_argument, 0, 'q'}, {"gpus", required_argument, 0, 1000},
        {"device", required_argument, 0, 1001}, {"plain", no_argument, 0, 1002}, {"stats-json", required_argument, 0, 1003},
        {"count-floor", required_argument, 0, 1004}, {"streaming-only", no_argument, 0, 1005}, {"rsh-cache", optional_argument, 0, 1006},
        {"zero-cut", required_argument, 0, 1007}, {"abs-step", required_argument, 0, 1008}, {"devices", required_argument, 0, 1009},
        {"device-collapse", no_argument, 0, 1010}, {"no-deterministic", no_argument, 0, 1011},
        {"bootstrap", required_argument, 0, 1012}, {"bootstrap-seed", required_argument, 0, 1013}, {"g2t", required_argument, 0, 1014},
        {"subsample", required_argument, 0, 1015}, {"subsample-reps", required_argument, 0, 1016}, {"subsample-seed", required_argument, 0, 1017},
        {"bootstrap-quantiles", required_argument, 0, 1018}, {"isoforms", no_argument, 0, 1019}, {"fit", no_argument, 0, 1020},
        {"presence", no_argument, 0, 1021}, {"presence-list", required_argument, 0, 1022},
        {"asymptotic", no_argument, 0, 1023}, {"boundary-cut", required_argument, 0, 1024},
        {"profile", no_argument, 0, 1025}, {"profile-level", required_argument, 0, 1026}, {"profile-list", required_argument, 0, 1027},
        {"profile-evals", required_argument, 0, 1028},
        {"compare", no_argument, 0, 1029}, {"compare-ratio", required_argument, 0, 1030}, {"compare-list", required_argument, 0, 1031},
        {"compare-usage", no_argument, 0, 1040}, {"profile-usage", no_argument, 0, 1041},
        {"compare-groups", required_argument, 0, 1042}, {"compare-sizes", required_argument, 0, 1043},
        {"maxfraglen", required_argument, 0, 'F'}, {"minfraglen", required_argument, 0, 'f'}, {0, 0, 0, 0}};
    int c;
    while ((c = getopt_long(argc, argv, "vqPs:p:F:f:n:e:d:gMSBk:i:I:", lo, NULL)) != -1) {
        switch (c) {
            case 'I': cfg->rsh_path = optarg; break;
            case 'P': cfg->ao.pe = 1; break;
            case 's': cfg->strand = optarg; break;
            case 'p': break;                       /* CPU threads of the reference's solver: no meaning here */
            case 'F': case 'f': break;             /* overwritten by the rsh header in the reference too */
            case 'k': cfg->ao.max_repeat = atoi(optarg); break;
            case 'n': if ((cfg->n_round = atoi(optarg)) <= 0) return bad("option -n must be a natural number."); break;
            case 'e': if ((cfg->tol = atof(optarg)) <= 0) return bad("option -e must be positive."); break;
            case 'i': if ((cfg->max_iter = atoi(optarg)) <= 0) return bad("option -i must be positive."); break;
            case 'd': cfg->delta = atoi(optarg); break;
            case 'g': cfg->print_segments = 1; break;
            case 'M': cfg->multisample = 1; break;
            case 'S': cfg->ao.format = 1; break;
            case 'B': cfg->ao.format = 2; break;
            case 'v': cfg->verbose = 2; break;
            case 'q': cfg->verbose = 0; break;
            case 1000: cfg->gpus = atoi(optarg); break;
            case 1001: cfg->device = atoi(optarg); break;
            case 1002: cfg->accel = 0; break;
            case 1003: cfg->stats_json = optarg; break;
            case 1004: if ((cfg->count_floor = atof(optarg)) < 0) return bad("--count-floor must be >= 0."); break;
            case 1005: cfg->set_mode = 1; break;
            case 1006: cfg->rsh_cache = optarg ? optarg : ""; break;
            case 1007: cfg->zero_cut = atof(optarg); break;
            case 1008: cfg->abs_step = atof(optarg); break;
            case 1009: if (parse_device_list(optarg, cfg->dev_map, &cfg->n_dev_map)) return bad("--devices wants a comma-separated list of device ids."); break;
            case 1010: cfg->device_collapse = 1; break;
            case 1011: cfg->no_deterministic = 1; break;
            case 1012: if (parse_count(optarg, 0, 1000000, &cfg->boot_n)) return bad("--bootstrap wants a number of replicates (0 .. 1000000)."); break;
            case 1013: if (parse_seed(optarg, &cfg->boot_seed)) return bad("--bootstrap-seed wants a non-negative integer."); break;
            case 1014: cfg->g2t = optarg; break;
            case 1015:
                if (parse_fraction_list(optarg, 0.0, 1, cfg->sub_f, &cfg->sub_nf)) return bad("--subsample wants a comma-separated list of 1 to 64 fractions in (0, 1].");
                break;
            case 1016: if (parse_count(optarg, 1, 1000000, &cfg->sub_reps)) return bad("--subsample-reps wants a number of replicates (1 .. 1000000)."); break;
            case 1017: if (parse_seed(optarg, &cfg->sub_seed)) return bad("--subsample-seed wants a non-negative integer."); break;
            case 1018:
                if (parse_fraction_list(optarg, 0.0, 0, cfg->bq, &cfg->bq_n))
                    return bad("--bootstrap-quantiles wants a comma-separated list of 1 to 64 probabilities in [0, 1].");
                break;
            case 1019: cfg->isoforms = 1; break;
            case 1020: cfg->fit = 1; break;
            case 1021: cfg->presence = 1; break;
            case 1022: cfg->presence_list = optarg; break;
            case 1023: cfg->asymptotic = 1; break;
            case 1024: cfg->boundary_cut = atof(optarg); cfg->boundary_cut_given = 1; break;
            case 1025: cfg->profile = 1; break;
            case 1026: cfg->profile_level = atof(optarg); cfg->profile_level_given = 1; break;
            case 1027: cfg->profile_list = optarg; break;
            case 1028: if ((cfg->profile_evals = atoi(optarg)) <= 0) return bad("--profile-evals must be positive."); break;
            case 1029: cfg->compare = 1; break;
            case 1040: cfg->compare_usage = 1; break;
            case 1041: cfg->profile_usage = 1; break;
            case 1030: cfg->compare_ratio = atof(optarg); cfg->compare_ratio_given = 1; break;
            case 1031: cfg->compare_list = optarg; break;
            case 1042:
                if (parse_group_list(optarg, cfg->group_of, &cfg->n_groups)) return bad("--compare-groups wants a comma-separated list of group ids (0 .. 31).");
                cfg->compare_groups = 1;
                break;
            case 1043:
                if (parse_size_list(optarg, cfg->group_size, &cfg->n_sizes)) return bad("--compare-sizes wants a comma-separated list of positive size factors.");
                break;
            default: usage(argv[0]); return 1;
        }
    }
    return 0;
}

/* What the options ask of one another, and the defaults that depend on whether an option was given.  The order of the checks is the order of
 * their messages: an argument list that trips two of them hears of the first. */
static int check_options(config *cfg, const char *a0) {
    if (cfg->bq_n > 0 && (cfg->boot_n < 1 || cfg->boot_n > 4096)) return bad("--bootstrap-quantiles needs --bootstrap B with 1 <= B <= 4096 replicates.");
    if (cfg->isoforms && !cfg->g2t) return bad("--isoforms needs --g2t FILE.");
    if (cfg->boundary_cut_given && !cfg->asymptotic) return bad("--boundary-cut needs --asymptotic.");
    if (cfg->boundary_cut_given && !(cfg->boundary_cut >= 0.0)) return bad("--boundary-cut must be >= 0.");
    if (!cfg->boundary_cut_given) cfg->boundary_cut = EMSAR_ASYM_DEFAULT_CUT;
    if (cfg->presence_list && !cfg->presence) return bad("--presence-list needs --presence.");
    if ((cfg->profile_list || cfg->profile_level_given || cfg->profile_evals) && !cfg->profile && !cfg->profile_usage)
        return bad("--profile-list, --profile-level and --profile-evals need --profile.");
    if (cfg->profile_level_given && !(cfg->profile_level > 0.0 && cfg->profile_level < 1.0)) return bad("--profile-level must lie in (0, 1).");
    if (!cfg->profile_level_given) cfg->profile_level = 0.95;
    if (cfg->compare_ratio_given && !cfg->compare) return bad("--compare-ratio needs --compare.");
    if (cfg->compare_list && !cfg->compare && !cfg->compare_usage && !cfg->compare_groups)
        return bad("--compare-list needs --compare or --compare-usage.");
    if (cfg->n_sizes && !cfg->compare_groups) return bad_usage("--compare-sizes needs --compare-groups.", a0);
    if (cfg->compare_usage && !cfg->g2t) return bad_usage("--compare-usage needs --g2t FILE.", a0);
    if (cfg->profile_usage && !cfg->g2t) return bad_usage("--profile-usage needs --g2t FILE.", a0);
    if (cfg->compare_ratio_given && !(cfg->compare_ratio > 0.0 && isfinite(cfg->compare_ratio))) return bad("--compare-ratio must be positive.");
    if (!cfg->compare_ratio_given) cfg->compare_ratio = 1.0;
    if (cfg->compare && !cfg->multisample) return bad_usage("--compare needs -M and at least two samples.", a0);
    if (cfg->compare_usage && !cfg->multisample) return bad_usage("--compare-usage needs -M and at least two samples.", a0);
    if (cfg->compare_groups && !cfg->multisample) return bad_usage("--compare-groups needs -M and at least two samples.", a0);
    return 0;
}

/* cfg->aln: the alignment file itself, or with -M the files its last argument lists, one per line */
static int read_sample_list(config *cfg, const char *last) {
    if (!cfg->multisample) {
        cfg->aln = (char **)malloc(sizeof(char *)); cfg->aln[0] = strdup(last); cfg->n_aln = 1;
        return 0;
    }
    FILE *f = fopen(last, "r");
    if (!f) return bad("Can't open alignment list file.");
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        size_t n = strlen(line);
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
        if (!n) continue;
        cfg->aln = (char **)realloc(cfg->aln, sizeof(char *) * (size_t)(cfg->n_aln + 1));
        cfg->aln[cfg->n_aln++] = strdup(line);
    }
    fclose(f);
    if (!cfg->n_aln) { fprintf(stderr, "No alignment files in the alignment list\n"); return 1; }
    return 0;
}

/* the reference runs `mkdir -p outdir` (emsar_main.c:284-285); find out now, not after the solve, that it cannot be written */
static int make_outdir(const char *outdir) {
    char tmp[4096];
    size_t n = strlen(outdir);
    if (n == 0 || n >= sizeof tmp) { fprintf(stderr, "can't create output directory %s\n", outdir); return 1; }
    memcpy(tmp, outdir, n + 1);
    for (size_t k = 1; k <= n; k++)
        if (tmp[k] == '/' || tmp[k] == 0) {
            const char keep = tmp[k];
            tmp[k] = 0;
            if (mkdir(tmp, 0777) != 0 && errno != EEXIST) { fprintf(stderr, "can't create output directory %s\n", tmp); return 1; }
            tmp[k] = keep;
        }
    if (access(outdir, W_OK | X_OK) != 0) { fprintf(stderr, "can't write to output directory %s\n", outdir); return 1; }
    return 0;
}

/* the index: from its binary cache (--rsh-cache: <rsh>.bin next to the text unless a path was given) or from the text, which then writes the cache */
static emsar_rsh *read_index(const config *cfg) {
    char err[512];
    emsar_rsh *rsh = NULL;
    double t0 = now_s();
    int rc = -1, from_cache = 0;
    char *cache_path = NULL;
    if (cfg->rsh_cache) {
        size_t n = strlen(cfg->rsh_cache[0] ? cfg->rsh_cache : cfg->rsh_path) + 8;
        cache_path = (char *)malloc(n);
        if (!cache_path) { fprintf(stderr, "out of memory\n"); return NULL; }
        if (cfg->rsh_cache[0]) snprintf(cache_path, n, "%s", cfg->rsh_cache); else snprintf(cache_path, n, "%s.bin", cfg->rsh_path);
        rc = emsar_rsh_read_cache(cfg->rsh_path, cache_path, &rsh, err, sizeof err);
        if (rc == 0) from_cache = 1;
        else if (cfg->verbose > 1) fprintf(stdout, "rsh cache not used (%s)\n", err);
    }
    if (rc) rc = emsar_rsh_read(cfg->rsh_path, &rsh, err, sizeof err);
    if (rc) { fprintf(stderr, "%s\n", err); return NULL; }
    if (cache_path && !from_cache && emsar_rsh_write_cache(rsh, cfg->rsh_path, cache_path) != 0)
        fprintf(stderr, "warning: can't write the rsh cache %s\n", cache_path);
    if (cfg->verbose > 0 && from_cache) fprintf(stdout, "rsh: binary cache %s\n", cache_path);
    free(cache_path);
    if (cfg->verbose > 0) fprintf(stdout, "rsh: %d transcripts, %lld segments, fragment lengths %d-%d (%.2fs)\n", rsh->n_tx,
                                  (long long)rsh->n_rows, rsh->frag_min, rsh->frag_max, now_s() - t0);
    return rsh;
}

/* -M: one worker per GPU, or per entry of --devices (cfg->dev_map holds their devices afterwards); 0 after a message if that cannot be had.
 * A probe context tells how many devices exist without touching HIP here. */
static int count_workers(config *cfg) {
    int avail = 0, n_workers;
    for (int d = 0; d < 64; d++) { emsar_hip_ctx *probe = NULL; if (emsar_hip_create(&probe, d) != 0) break; emsar_hip_destroy(probe); avail++; }
    if (avail == 0) { fprintf(stderr, "%s\n", emsar_hip_strerror(EMSAR_HIP_ERR_NO_DEVICE)); return 0; }
    if (cfg->n_dev_map) {
        for (int g = 0; g < cfg->n_dev_map; g++)
            if (cfg->dev_map[g] >= avail) { fprintf(stderr, "--devices: device %d does not exist (%d found)\n", cfg->dev_map[g], avail); return 0; }
        n_workers = cfg->n_dev_map;
    } else {
        n_workers = cfg->gpus > 0 && cfg->gpus < avail ? cfg->gpus : avail;
        for (int g = 0; g < n_workers && g < 64; g++) cfg->dev_map[g] = g;
        if (n_workers > 64) n_workers = 64;
    }
    return n_workers > cfg->n_aln ? cfg->n_aln : n_workers;
}

/* --stats-json FILE: the job and, per sample, its status, its host times and the statistics of the library calls it made (w: any worker --
 * the per-sample arrays are shared) */
static void write_stats_json(const config *cfg, const worker_arg *w, int n_workers, double wall, int n_bad) {
    FILE *f = fopen(cfg->stats_json, "w");
    if (!f) return;
    fprintf(f, "{\"samples\": %d, \"gpus\": %d, \"wall_s\": %.6f, \"failed\": %d, \"per_sample\": [", cfg->n_aln, n_workers, wall, n_bad);
    for (int i = 0; i < cfg->n_aln; i++) {
        const emsar_em_stats *e = &w->stats[i];
        fprintf(f, "%s{\"status\": %d, \"parse_s\": %.6f, \"model_s\": %.6f, \"host_s\": %.6f, \"em_passes\": %d, \"converged\": %d, \"solve_ms\": %.4f, \"kernel_ms\": %.4f, \"loglik\": %.9g, \"bytes_per_pass\": %lld, "
                   "\"sets_resident\": %d, \"sets_streamed\": %d, \"set_passes_max\": %d, \"set_passes_sum\": %lld, \"sets_build_ms\": %.4f, \"sets_kernel_ms\": %.4f",
                i ? ", " : "", w->status[i], w->parse_s[i], w->model_s[i], w->host_s[i], e->iters, e->converged, e->solve_ms, e->kernel_ms, e->loglik,
                (long long)e->bytes_per_pass, e->sets_resident, e->sets_streamed, e->set_passes_max, (long long)e->set_passes_sum, e->sets_build_ms,
                e->sets_kernel_ms);
        if (cfg->boot_n > 0) {
            const emsar_boot_stats *b = &w->bstats[i];
            fprintf(f, ", \"boot_replicates\": %d, \"boot_batch\": %d, \"boot_replicates_unconverged\": %d, \"boot_set_passes_max\": %d, "
                       "\"boot_draws\": %lld, \"boot_draw_ms\": %.4f, \"boot_sets_ms\": %.4f, \"boot_stream_ms\": %.4f, \"boot_reduce_ms\": %.4f, \"boot_total_ms\": %.4f",
                    b->n_replicates, b->batch, b->replicates_unconverged, b->set_passes_max, (long long)b->draws, b->draw_ms, b->sets_ms,
                    b->stream_ms, b->reduce_ms, b->total_ms);
        }
        if (cfg->boot_n > 0 && cfg->bq_n > 0)
            fprintf(f, ", \"bootq_quantiles\": %d, \"bootq_held_bytes\": %lld, \"bootq_ms\": %.4f", w->qstats[i].n_quantiles,
                    (long long)w->qstats[i].held_bytes, w->qstats[i].quantile_ms);
        if (cfg->sub_nf > 0) {
            const emsar_subsample_stats *b = &w->sstats[i];
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

int main(int argc, char **argv) {
    config cfg = {.ao = {.max_repeat = 100}, .n_round = 4, .verbose = 1, .accel = 1, .tol = 1e-10, .max_iter = 200000,
                  .zero_cut = 2.5e-7,      /* a quarter of the "%lf" print quantum of the .fpkm file */
                  .abs_step = 1e-13,       /* see emsar_em_params.abs_step */
                  .boot_seed = 1, .sub_reps = 10, .sub_seed = 1, .strand = "ns"};
    compare_ref ref = {0};
    if (parse_options(argc, argv, &cfg) || check_options(&cfg, argv[0])) return 1;
    cfg.ref = &ref;
    if (!cfg.rsh_path || optind + 2 >= argc) { usage(argv[0]); return 1; }
    if (emsar_set_strand(cfg.strand, cfg.ao.pe, &cfg.ao.strand)) return bad("error: invalid strand type.");
    cfg.outdir = argv[optind]; cfg.prefix = argv[optind + 1];
    if (read_sample_list(&cfg, argv[optind + 2])) return 1;
    if (cfg.compare && cfg.n_aln < 2) return bad_usage("--compare needs -M and at least two samples.", argv[0]);
    if (cfg.compare_usage && cfg.n_aln < 2) return bad_usage("--compare-usage needs -M and at least two samples.", argv[0]);
    if (cfg.compare_groups) {
        const char *wrong = check_groups(cfg.n_aln, cfg.n_groups, cfg.group_of, cfg.n_sizes);
        if (wrong) return bad_usage(wrong, argv[0]);
        if (!(cfg.inputs = (compare_ref *)calloc((size_t)cfg.n_aln, sizeof(compare_ref)))) return bad("out of memory");
    }
    if (make_outdir(cfg.outdir)) return 1;
    emsar_rsh *rsh = read_index(&cfg);
    if (!rsh) return 1;
    /* before any sample: an unknown name ends the run here */
    if ((cfg.presence_list && read_name_list("presence", cfg.presence_list, rsh, &cfg.pres_q, &cfg.pres_nq)) ||
        (cfg.profile_list && read_name_list("profile", cfg.profile_list, rsh, &cfg.prof_q, &cfg.prof_nq)) ||
        (cfg.compare_list && read_name_list("compare", cfg.compare_list, rsh, &cfg.cmp_q, &cfg.cmp_nq))) { emsar_rsh_free(rsh); return 1; }
    emsar_genes *genes = NULL;
    if (cfg.g2t) {                             /* before any sample: a bad gene map ends the run here */
        char err[512];
        if (emsar_genes_read(rsh, cfg.g2t, &genes, err, sizeof err)) { fprintf(stderr, "%s\n", err); emsar_rsh_free(rsh); return 1; }
        cfg.genes = genes;
        if (cfg.verbose > 1)
            fprintf(stdout, "g2t: %d genes; %lld g2t lines name a transcript not in the index (ignored); %d index transcripts in no gene%s\n",
                    genes->n_genes, (long long)genes->n_unknown, genes->n_unmapped, genes->n_unmapped ? " (empty geneID)" : "");
    }
    int n_workers = cfg.multisample ? count_workers(&cfg) : 1;
    if (n_workers < 1) return 1;
    const size_t n = (size_t)cfg.n_aln;
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER; pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
    int next_model = 0, go = 0, n_started = 1; double eumacut = 0.0;
    /* what every worker shares: the hand-over's state and the per-sample results */
    const worker_arg shared = {.cfg = &cfg, .rsh = rsh, .n_workers = n_workers, .mu = &mu, .cv = &cv, .next_model = &next_model, .eumacut = &eumacut, .go = &go,
                               .status = (int *)calloc(n, sizeof(int)), .stats = (emsar_em_stats *)calloc(n, sizeof(emsar_em_stats)),
                               .bstats = (emsar_boot_stats *)calloc(n, sizeof(emsar_boot_stats)),
                               .sstats = (emsar_subsample_stats *)calloc(n, sizeof(emsar_subsample_stats)),
                               .qstats = (emsar_quantile_stats *)calloc(n, sizeof(emsar_quantile_stats)), .parse_s = (double *)calloc(n, sizeof(double)),
                               .model_s = (double *)calloc(n, sizeof(double)), .host_s = (double *)calloc(n, sizeof(double)), .ao = cfg.ao,
                               .cdev = {.ctx = NULL, .mu = PTHREAD_MUTEX_INITIALIZER}};
    worker_arg *wa = (worker_arg *)calloc((size_t)n_workers, sizeof(worker_arg));
    pthread_t *th = (pthread_t *)calloc((size_t)n_workers, sizeof(pthread_t));
    if (!shared.status || !shared.stats || !shared.bstats || !shared.sstats || !shared.qstats || !shared.parse_s || !shared.model_s || !shared.host_s || !wa || !th)
        return bad("out of memory");
    double t0 = now_s();
    /* Workers wait at a gate until their number is final: a thread that cannot be started must not leave the others
     * waiting for samples nobody will take (the EUMAcut hand-over is in sample order). */
    for (int g = 0; g < n_workers; g++) { wa[g] = shared; wa[g].worker = g; wa[g].device = cfg.multisample ? cfg.dev_map[g] : cfg.device; }
    for (int g = 1; g < n_workers; g++) {
        if (pthread_create(&th[g], NULL, worker_main, &wa[g]) != 0) { fprintf(stderr, "warning: worker %d could not be started, using %d\n", g, g); break; }
        n_started++;
    }
    /* every parallel host step of a worker gets its share of the cores: G workers x 16 reader threads each would
     * oversubscribe the host (parse and inflate pools, emsar_host_threads) */
    const long nc = sysconf(_SC_NPROCESSORS_ONLN);
    const int share = (int)((nc < 1 ? 1 : nc) / n_started);
    emsar_host_set_thread_budget(share < 1 ? 1 : share > 16 ? 16 : share);
    pthread_mutex_lock(&mu);
    n_workers = n_started;
    for (int g = 0; g < n_workers; g++) wa[g].n_workers = n_workers;
    go = 1;
    pthread_cond_broadcast(&cv);
    pthread_mutex_unlock(&mu);
    worker_main(&wa[0]);
    for (int g = 1; g < n_workers; g++) pthread_join(th[g], NULL);
    int n_bad = 0;
    for (int i = 0; i < cfg.n_aln; i++) if (shared.status[i]) n_bad++;
    if (cfg.compare_groups && !n_bad && stage_groups(&cfg, rsh, wa[0].device)) n_bad++;
    const double wall = now_s() - t0;
    if (cfg.stats_json) write_stats_json(&cfg, &shared, n_workers, wall, n_bad);
    emsar_rsh_free(rsh);
    emsar_genes_free(genes);
    free(cfg.pres_q); free(cfg.prof_q); free(cfg.cmp_q); free(ref.R); free(ref.E); free(ref.den);
    for (int i = 0; cfg.inputs && i < cfg.n_aln; i++) { free(cfg.inputs[i].R); free(cfg.inputs[i].E); free(cfg.inputs[i].den); }
    free(cfg.inputs);
    for (int i = 0; i < cfg.n_aln; i++) free(cfg.aln[i]);
    free(cfg.aln); free(shared.status); free(shared.stats); free(shared.bstats); free(shared.sstats); free(shared.qstats); free(shared.parse_s);
    free(shared.model_s); free(shared.host_s); free(wa); free(th);
    return n_bad ? 1 : 0;
}
