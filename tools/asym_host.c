/* asym_host.c -- a stand-alone run of emsar_hip_asymptotic_host (no HIP call, no GPU) on a builder problem, meant to be built with the
 * library's sources under a sanitiser on the host side:
 *
 *     hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
 *           emsar_amd/csrc/emsar_hip.hip emsar_amd/csrc/collapse.hip -c        (two objects)
 *     clang -O1 -g -fsanitize=address,undefined -Iinclude -c tools/asym_host.c
 *     hipcc -fsanitize=address,undefined emsar_hip.o collapse.o asym_host.o -o asym_host && ./asym_host
 *
 * The problem: components of 1, 2, 8, 9, 64, 65, 192 and 193 transcripts (a chain of pairs, one single-tid row each, triples, a row
 * with a repeated tid), two confounded transcripts, a boundary transcript inside a row, a row with E == 0, a gene map with a gene across
 * components; every output is asked for, the block of each component in turn.  Prints the statistics and a checksum; exits 0 when the
 * statuses are the expected ones. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "emsar_hip.h"

static uint64_t rng_state = 12345;
static uint32_t rnd(uint32_t n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33) % n;
}

#define MAX_ROWS 4096
#define MAX_NNZ 16384
static uint64_t row_ptr[MAX_ROWS + 1];
static int32_t col[MAX_NNZ], weight[MAX_ROWS];
static double E[MAX_ROWS];
static int64_t n_rows;

static void add_row(const int32_t *t, int k, int32_t w, double e) {
    if (n_rows >= MAX_ROWS || row_ptr[n_rows] + (uint64_t)k > MAX_NNZ) { fprintf(stderr, "problem too large\n"); exit(2); }
    for (int i = 0; i < k; i++) col[row_ptr[n_rows] + (uint64_t)i] = t[i];
    weight[n_rows] = w; E[n_rows] = e;
    row_ptr[n_rows + 1] = row_ptr[n_rows] + (uint64_t)k;
    n_rows++;
}

int main(void) {
    static const int sizes[8] = {1, 2, 8, 9, 64, 65, 192, 193};
    int32_t first[8], n_tx = 0;
    for (int c = 0; c < 8; c++) {
        const int n = sizes[c];
        first[c] = n_tx;
        for (int i = 0; i < n; i++) {
            int32_t t[4] = {n_tx + i, n_tx + i + 1, 0, 0};
            add_row(t, 1, 1 + (int32_t)rnd(40), 1.0);
            if (i + 1 < n) add_row(t, 2, 1 + (int32_t)rnd(40), 1.5);
            if (i + 2 < n && i % 5 == 0) { t[2] = n_tx + i + 2; add_row(t, 3, 1 + (int32_t)rnd(40), 0.5); }
        }
        int32_t rep[3] = {n_tx, n_tx, n_tx + (n > 1)};
        add_row(rep, n > 1 ? 3 : 2, 3, 1.0);
        n_tx += n;
    }
    const int32_t ca = n_tx, cb = n_tx + 1, bnd = n_tx + 2;     /* two confounded transcripts, a boundary one */
    n_tx += 3;
    { int32_t t[3] = {ca, cb, bnd}; add_row(t, 2, 9, 1.0); add_row(t, 3, 4, 1.0); add_row(t + 2, 1, 2, 1.0); }
    { int32_t t[2] = {first[2], first[3]}; add_row(t, 2, 50, 0.0); }                    /* E == 0: ties nothing */
    double *theta = (double *)malloc((size_t)n_tx * 8);
    int32_t *gene = (int32_t *)malloc((size_t)n_tx * 4);
    const int32_t n_genes = 40;
    for (int32_t t = 0; t < n_tx; t++) { theta[t] = 0.1 + 49.9 * (double)rnd(1000000) / 1e6; gene[t] = (int32_t)rnd((uint32_t)n_genes + 1) - 1; }
    theta[bnd] = 0.0;
    gene[first[2]] = gene[first[4]] = 0;

    double *v = (double *)malloc((size_t)n_tx * 8 * 6), *gsd = (double *)malloc((size_t)n_genes * 8);
    int32_t *iv = (int32_t *)malloc((size_t)n_tx * 4 * 3), *gst = (int32_t *)malloc((size_t)n_genes * 4);
    int32_t block_n, *block_tids = (int32_t *)malloc(EMSAR_ASYM_MAX_N * 4);
    double *block_cov = (double *)malloc((size_t)EMSAR_ASYM_MAX_N * EMSAR_ASYM_MAX_N * 8);
    const size_t T = (size_t)n_tx;
    const emsar_asym_outputs out = {v, v + T, v + 2 * T, v + 3 * T, v + 4 * T, iv, iv + T, v + 5 * T, iv + 2 * T, gsd, gst, &block_n, block_tids, block_cov};
    emsar_asym_stats st;
    double check = 0.0;
    int bad = 0;
    for (int c = 0; c < 9; c++) {
        const emsar_asym_params p = {EMSAR_ASYM_DEFAULT_CUT, 0.0, c < 8 ? first[c] : ca, 0};
        const int rc = emsar_hip_asymptotic_host(n_rows, n_tx, row_ptr, col, weight, E, theta, n_genes, gene, &p, &out, &st);
        if (rc) { fprintf(stderr, "asymptotic_host: %d\n", rc); return 1; }
        const int want_n = c < 7 ? sizes[c] : 0;                /* 193 is TOO_LARGE, the confounded pair UNIDENTIFIABLE */
        if (block_n != want_n) { fprintf(stderr, "block of component %d: n = %d, expected %d\n", c, block_n, want_n); bad = 1; }
        for (int i = 0; i < block_n; i++) check += block_cov[(size_t)i * (size_t)block_n + (size_t)i];
    }
    for (int32_t t = 0; t < n_tx; t++) {
        const int32_t want = t == bnd ? EMSAR_ASYM_BOUNDARY : (t == ca || t == cb) ? EMSAR_ASYM_UNIDENTIFIABLE
                             : t >= first[7] && t < ca ? EMSAR_ASYM_TOO_LARGE : EMSAR_ASYM_ESTIMATED;
        if (iv[t] != want) { fprintf(stderr, "transcript %d: status %d, expected %d\n", t, iv[t], want); bad = 1; }
        if (iv[t] == EMSAR_ASYM_ESTIMATED) check += v[T + (size_t)t] + v[2 * T + (size_t)t];
    }
    printf("rows %lld, transcripts %d, components %lld (too large %lld), max n %d, min pivot ratio %.6g, checksum %.17g\n", (long long)n_rows,
           n_tx, (long long)st.components, (long long)st.components_too_large, st.max_n, st.min_pivot_ratio, check);
    free(theta); free(gene); free(v); free(gsd); free(iv); free(gst); free(block_tids); free(block_cov);
    return bad;
}
