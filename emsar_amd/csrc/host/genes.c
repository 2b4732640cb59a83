/* genes.c -- the gene map of the reference's util/FPKM2gFPKM.pl (g2tfile FPKMfile -> <prefix>.gfpkm), read once per index.
 *
 * The script's rules, kept here:
 *   - a line is split on tabs; field 0 is the gene, field 1 the transcript, further fields are ignored;
 *   - a transcript listed twice belongs to the gene of its LAST line ($t2g{$t} = $g);
 *   - g2t transcripts that are not in the index are ignored (counted in n_unknown);
 *   - a gene exists only if at least one index transcript maps to it after the last-wins rule;
 *   - index transcripts missing from the g2t sum into one gene with an EMPTY geneID (the script's undef hash key); a g2t line with an
 *     empty gene field maps its transcript to that same gene, as in the script.
 * Deliberate deviations: a trailing '\r' is stripped (the line reader does it; the script would keep it in the transcript name and
 * then miss that transcript), and lines without a tab are skipped (the script maps no index transcript through them either).  The
 * output order is ours, since Perl's hash order is random: genes in order of their first appearance in the g2t, the empty-ID gene last.
 * The file is read through the alignments' line reader, so a gzipped g2t works too.  A file that cannot be opened, holds no line
 * or no line with a tab is an error.
 */
#include "emsar_host.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void *emsar_lr_open(const char *path);
char *emsar_lr_next(void *h);
void emsar_lr_close(void *h);

/* gene name -> index of first appearance (open addressing, FNV-1a) */
typedef struct { uint32_t cap, n; int32_t *slot; char **names; } gene_table;

static uint64_t fnv1a(const char *s) {
    uint64_t h = 1469598103934665603ull;
    for (; *s; s++) { h ^= (unsigned char)*s; h *= 1099511628211ull; }
    return h;
}

static int gt_grow(gene_table *g) {
    uint32_t cap = g->cap ? g->cap * 2 : 1024;
    int32_t *slot = (int32_t *)malloc(sizeof(int32_t) * cap);
    char **names = (char **)realloc(g->names, sizeof(char *) * (cap / 2));
    if (!slot || !names) { free(slot); if (names) g->names = names; return -1; }
    g->names = names;
    for (uint32_t i = 0; i < cap; i++) slot[i] = -1;
    for (uint32_t k = 0; k < g->n; k++) {
        uint32_t i = (uint32_t)fnv1a(g->names[k]) & (cap - 1);
        while (slot[i] >= 0) i = (i + 1) & (cap - 1);
        slot[i] = (int32_t)k;
    }
    free(g->slot);
    g->slot = slot; g->cap = cap;
    return 0;
}

/* index of `name`, added if new; -1 when out of memory */
static int32_t gt_get(gene_table *g, const char *name) {
    if ((g->n + 1) * 2 > g->cap && gt_grow(g)) return -1;
    uint32_t i = (uint32_t)fnv1a(name) & (g->cap - 1);
    while (g->slot[i] >= 0) {
        if (strcmp(g->names[g->slot[i]], name) == 0) return g->slot[i];
        i = (i + 1) & (g->cap - 1);
    }
    char *copy = strdup(name);
    if (!copy) return -1;
    g->names[g->n] = copy;
    g->slot[i] = (int32_t)g->n;
    return (int32_t)g->n++;
}

static void gt_free(gene_table *g, int keep_names) {
    if (!keep_names) for (uint32_t k = 0; k < g->n; k++) free(g->names[k]);
    free(g->names); free(g->slot);
}

#define EMPTY_GENE (-2)   /* last_gene[t]: the empty-ID gene */

static int fail(char *err, size_t errlen, int rc, const char *fmt, ...) {
    if (err && errlen) { va_list ap; va_start(ap, fmt); vsnprintf(err, errlen, fmt, ap); va_end(ap); }
    return rc;
}

int emsar_genes_read(const emsar_rsh *r, const char *g2t_path, emsar_genes **out, char *err, size_t errlen) {
    if (!r || !g2t_path || !out) return fail(err, errlen, EMSAR_HOST_ERR_ARG, "genes: bad argument");
    *out = NULL;
    void *lr = emsar_lr_open(g2t_path);
    if (!lr) return fail(err, errlen, EMSAR_HOST_ERR_IO, "can't open g2t file %s", g2t_path);
    const int32_t n = r->n_tx;
    int32_t *last = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));   /* gene of the last line naming t; -1 = none */
    gene_table gt; memset(&gt, 0, sizeof gt);
    int rc = EMSAR_HOST_OK;
    int64_t lines = 0, mapped_lines = 0, unknown = 0;
    if (!last) { emsar_lr_close(lr); return fail(err, errlen, EMSAR_HOST_ERR_OOM, "out of memory"); }
    for (int32_t t = 0; t < n; t++) last[t] = -1;
    char *line;
    while ((line = emsar_lr_next(lr)) != NULL) {
        lines++;
        char *tab = strchr(line, '\t');
        if (!tab) continue;
        *tab = 0;
        char *tx = tab + 1, *end = strchr(tx, '\t');
        if (end) *end = 0;
        mapped_lines++;
        int32_t g = EMPTY_GENE;
        if (line[0] && (g = gt_get(&gt, line)) < 0) { rc = fail(err, errlen, EMSAR_HOST_ERR_OOM, "out of memory"); break; }
        const int32_t t = emsar_rsh_tid_of(r, tx);
        if (t < 0) unknown++;
        else last[t] = g;
    }
    emsar_lr_close(lr);
    if (rc == 0 && lines == 0) rc = fail(err, errlen, EMSAR_HOST_ERR_FORMAT, "g2t file %s is empty", g2t_path);
    if (rc == 0 && mapped_lines == 0) rc = fail(err, errlen, EMSAR_HOST_ERR_FORMAT, "g2t file %s has no tab-separated gene/transcript line", g2t_path);
    emsar_genes *G = NULL;
    int32_t *num = NULL;
    if (rc == 0) {
        G = (emsar_genes *)calloc(1, sizeof *G);
        num = (int32_t *)malloc(sizeof(int32_t) * (gt.n + 1));
        if (G) {
            G->gene_of_tx = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
            G->names = (char **)calloc(gt.n + 1, sizeof(char *));
        }
        if (!G || !num || !G->gene_of_tx || !G->names) rc = fail(err, errlen, EMSAR_HOST_ERR_OOM, "out of memory");
    }
    if (rc == 0) {
        /* genes that keep an index transcript, numbered in order of first appearance; then the empty-ID gene */
        uint8_t *used = (uint8_t *)calloc(gt.n + 1, 1);
        if (!used) rc = fail(err, errlen, EMSAR_HOST_ERR_OOM, "out of memory");
        else {
            int32_t unmapped = 0;
            for (int32_t t = 0; t < n; t++) {
                if (last[t] >= 0) used[last[t]] = 1;
                else unmapped++;
            }
            int32_t k = 0;
            for (uint32_t g = 0; g < gt.n; g++) {
                if (used[g]) { num[g] = k; G->names[k++] = gt.names[g]; gt.names[g] = NULL; }
                else num[g] = -1;
            }
            const int32_t empty = unmapped > 0 ? k : -1;
            if (unmapped > 0) {
                G->names[k] = strdup("");
                if (!G->names[k]) rc = fail(err, errlen, EMSAR_HOST_ERR_OOM, "out of memory");
                k++;
            }
            for (int32_t t = 0; t < n; t++) G->gene_of_tx[t] = last[t] >= 0 ? num[last[t]] : empty;
            G->n_genes = k; G->n_tx = n; G->n_unknown = unknown; G->n_unmapped = unmapped;
            free(used);
        }
    }
    for (uint32_t g = 0; g < gt.n; g++) free(gt.names[g]);   /* the names not handed over */
    gt_free(&gt, 1);
    free(last); free(num);
    if (rc) { emsar_genes_free(G); return rc; }
    *out = G;
    return EMSAR_HOST_OK;
}

void emsar_genes_free(emsar_genes *g) {
    if (!g) return;
    if (g->names) for (int32_t k = 0; k < g->n_genes; k++) free(g->names[k]);
    free(g->names); free(g->gene_of_tx); free(g);
}
