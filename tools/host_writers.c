/* host_writers.c -- the writers of the test and interval files (.compare, .gcompare, .ucompare, .gprofile, .uprofile, .groups and their neighbours
 * .presence, .profile, .asym, .gasym; output.c) and the driver's argument parsers (cli_parse.h) on the inputs of their CPU tests, as a plain program to
 * put under the sanitizers:
 *   gcc -O1 -g -std=c11 -D_POSIX_C_SOURCE=200809L -fsanitize=address,undefined -fno-sanitize-recover=all -Iemsar_amd/csrc/host \
 *       tools/host_writers.c emsar_amd/csrc/host/output.c -lm -o host_writers && ./host_writers <scratch directory>
 * Every array is allocated at exactly the length the writer may read, so that a read past a query list or a gene table is caught; the
 * statuses run from below to above every family's range.  Exit status 0 and "host_writers ok" if every writer succeeded and every parser
 * took and refused what the tests say it does.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_parse.h"
#include "emsar_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static double *doubles(int n, const double *v) { double *p = (double *)malloc(sizeof(double) * (size_t)n); memcpy(p, v, sizeof(double) * (size_t)n); return p; }
static int32_t *ints(int n, const int32_t *v) { int32_t *p = (int32_t *)malloc(sizeof(int32_t) * (size_t)n); memcpy(p, v, sizeof(int32_t) * (size_t)n); return p; }

static void writers(const char *dir) {
    enum { NQ = 9, NT = 5, NGENES = 3 };
    char *tx[NT] = {"tA", "tB", "tC", "tD", "tE"}, *gn[NGENES] = {"g1", "", "g3"};
    const int32_t gmap_v[NT] = {0, 2, -1, 0, 1}, query_v[NQ] = {3, 0, 4, 0, 1, 2, 4, 2, 1};
    const int32_t status_v[NQ] = {0, 1, 2, 3, 4, 5, 6, 7, 8}, wild_v[NQ] = {-1, INT32_MIN, INT32_MAX, 8, 6, 5, 4, 0, -2}, heir_v[NQ] = {-1, 0, 4, 5, 1, 2, 3, -7, 1 << 30};
    const double a_v[NQ] = {0.25, NAN, INFINITY, -INFINITY, 0.0, 1.0, 1e-7, 0.5, 12345678.5}, p_v[NQ] = {0.0714, NAN, INFINITY, -INFINITY, 1.0, 1e-300, 0.123456789, 1.0, 0.5};
    const double fpkm_v[NT] = {1.5, 0.0, 9.0, 4.5, 2.25}, var_v[NT] = {1.0, 0.0, 4.0, INFINITY, NAN};
    const int32_t partner_v[NT] = {1, -1, 0, 9, 2};
    int32_t *gmap = ints(NT, gmap_v), *query = ints(NQ, query_v), *status = ints(NQ, status_v), *wild = ints(NQ, wild_v), *heir = ints(NQ, heir_v);
    int32_t *partner = ints(NT, partner_v);
    double *a = doubles(NQ, a_v), *p = doubles(NQ, p_v), *fpkm = doubles(NT, fpkm_v), *var = doubles(NT, var_v);
    const emsar_rsh r = {.n_tx = NT, .names = tx};
    const emsar_genes g = {.n_genes = NGENES, .n_tx = NT, .names = gn, .gene_of_tx = gmap};
    char path[4096];
    snprintf(path, sizeof path, "%s/host_writers.out", dir);
    for (int pass = 0; pass < 2; pass++) {
        const int32_t *st = pass ? wild : status;
        CHECK(emsar_write_compare(path, &r, NQ, query, a, p, a, p, p, st, query) == EMSAR_HOST_OK);
        CHECK(emsar_write_compare(path, &r, NT, NULL, a, p, a, p, p, st, query) == EMSAR_HOST_OK);
        CHECK(emsar_write_ucompare(path, &r, &g, NQ, query, a, p, a, p, p, st, query, query) == EMSAR_HOST_OK);
        CHECK(emsar_write_ucompare(path, &r, &g, NT, NULL, a, p, a, p, p, st, query, query) == EMSAR_HOST_OK);
        CHECK(emsar_write_uprofile(path, &r, &g, NQ, query, a, p, a, p, a, st, query, query) == EMSAR_HOST_OK);
        CHECK(emsar_write_uprofile(path, &r, &g, NT, NULL, a, p, a, p, a, st, query, query) == EMSAR_HOST_OK);
        {                                                           /* .groups: three samples in two groups, theta_group [NQ][2] */
            const int32_t group_v[3] = {0, 1, 0};
            const double size_v[3] = {1.0, 0.5, 2.0};
            int32_t *group_of = ints(3, group_v);
            double *size = doubles(3, size_v), *tg = (double *)malloc(sizeof(double) * 2 * NQ);
            for (int k = 0; k < 2 * NQ; k++) tg[k] = a_v[k % NQ];
            CHECK(emsar_write_groups(path, &r, NQ, query, 3, group_of, size, a, tg, a, p, a, p, st, query, query) == EMSAR_HOST_OK);
            CHECK(emsar_write_groups(path, &r, NT, NULL, 3, group_of, NULL, a, tg, a, p, a, p, st, query, query) == EMSAR_HOST_OK);
            free(group_of); free(size); free(tg);
        }
        CHECK(emsar_write_presence(path, &r, NQ, query, fpkm, a, p, st, heir, a) == EMSAR_HOST_OK);
        CHECK(emsar_write_profile(path, &r, NQ, query, fpkm, a, p, a, st) == EMSAR_HOST_OK);
        for (int k = 0; k + NGENES <= NQ; k += NGENES) {           /* three genes at a time: the gene writers read n_genes entries */
            double *ga = doubles(NGENES, a_v + k), *gp = doubles(NGENES, p_v + k);
            int32_t *gs = ints(NGENES, (pass ? wild_v : status_v) + k);
            CHECK(emsar_write_gcompare(path, &g, ga, gp, ga, gp, gp, gs, gs, gs) == EMSAR_HOST_OK);
            CHECK(emsar_write_gprofile(path, &g, ga, gp, ga, gp, gp, gs, gs) == EMSAR_HOST_OK);
            CHECK(emsar_write_gasym(path, &g, ga, gp, gs) == EMSAR_HOST_OK);
            free(ga); free(gp); free(gs);
        }
        CHECK(emsar_write_asym(path, &r, fpkm, fpkm, a, p, var, st, partner, a, pass ? p : NULL) == EMSAR_HOST_OK);
    }
    snprintf(path, sizeof path, "%s/no/such/directory/x", dir);
    CHECK(emsar_write_compare(path, &r, NQ, query, a, p, a, p, p, status, query) == EMSAR_HOST_ERR_IO);
    CHECK(emsar_write_gcompare(path, &g, a, p, a, p, p, status, status, status) == EMSAR_HOST_ERR_IO);
    CHECK(emsar_write_ucompare(path, &r, &g, NQ, query, a, p, a, p, p, status, query, query) == EMSAR_HOST_ERR_IO);
    CHECK(emsar_write_gprofile(path, &g, a, p, a, p, p, status, status) == EMSAR_HOST_ERR_IO);
    CHECK(emsar_write_uprofile(path, &r, &g, NQ, query, a, p, a, p, a, status, query, query) == EMSAR_HOST_ERR_IO);
    snprintf(path, sizeof path, "%s/host_writers.out", dir);
    remove(path);
    free(gmap); free(query); free(status); free(wild); free(heir); free(partner); free(a); free(p); free(fpkm); free(var);
}

/* a list of n equal entries, comma-separated, in a buffer of exactly its length */
static char *repeated(const char *entry, int n) {
    const size_t len = strlen(entry);
    char *s = (char *)malloc((len + 1) * (size_t)n), *q = s;
    for (int k = 0; k < n; k++) { memcpy(q, entry, len); q += len; *q++ = k + 1 < n ? ',' : 0; }
    return s;
}

static void parsers(void) {
    static const char *const bad_count[] = {"", "x", "3x", " ", "-1", "1000001", "99999999999999999999"};
    static const char *const bad_seed[] = {"", "x", "7x", "-1", "99999999999999999999"};
    static const char *const bad_list[] = {"", "x", "0.5;1", "0.5,", ",0.5", "0.5,,1", "-0.5", "1.5", "nan", "inf", "1e999"};
    static const char *const bad_devices[] = {"", "x", "0,x", "0x", "0,,1", ",0", "-1", "0,-1", "1024", "99999999999999999999"};
    int v = -5, n = 0, map[64];
    uint64_t seed = 0;
    double list[64];
    for (size_t k = 0; k < sizeof bad_count / sizeof *bad_count; k++) CHECK(parse_count(bad_count[k], 0, 1000000, &v) == 1 && v == -5);
    CHECK(parse_count("0", 1, 1000000, &v) == 1 && parse_count("0", 0, 1000000, &v) == 0 && v == 0 && parse_count("1000000", 1, 1000000, &v) == 0 && v == 1000000);
    for (size_t k = 0; k < sizeof bad_seed / sizeof *bad_seed; k++) CHECK(parse_seed(bad_seed[k], &seed) == 1 && seed == 0);
    CHECK(parse_seed("18446744073709551615", &seed) == 0 && seed == UINT64_MAX && parse_seed("0", &seed) == 0 && seed == 0);
    for (size_t k = 0; k < sizeof bad_list / sizeof *bad_list; k++)
        CHECK(parse_fraction_list(bad_list[k], 0.0, 1, list, &n) == 1 && parse_fraction_list(bad_list[k], 0.0, 0, list, &n) == 1);
    CHECK(parse_fraction_list("0", 0.0, 1, list, &n) == 1 && parse_fraction_list("0,1", 0.0, 0, list, &n) == 0 && n == 2 && list[0] == 0.0 && list[1] == 1.0);
    CHECK(parse_fraction_list("1e-300,0.5", 0.0, 1, list, &n) == 0 && n == 2 && list[1] == 0.5);
    char *l64 = repeated("0.5", 64), *l65 = repeated("0.5", 65), *d64 = repeated("0", 64), *d65 = repeated("1023", 65);
    CHECK(parse_fraction_list(l64, 0.0, 1, list, &n) == 0 && n == 64 && parse_fraction_list(l65, 0.0, 1, list, &n) == 1);
    CHECK(parse_fraction_list("1", 0.0, 1, list, &n) == 0 && n == 1);                         /* a list replaces the one before it */
    for (size_t k = 0; k < sizeof bad_devices / sizeof *bad_devices; k++) { n = 0; CHECK(parse_device_list(bad_devices[k], map, &n) == 1); }
    n = 0;
    CHECK(parse_device_list("0,1023", map, &n) == 0 && n == 2 && map[1] == 1023 && parse_device_list("3,", map, &n) == 0 && n == 3 && map[2] == 3);   /* appends */
    CHECK(parse_device_list(d64, map, &n) == 0 && n == 64 && map[63] == 0 && parse_device_list("x", map, &n) == 0 && n == 64);      /* full: not read */
    n = 0;
    CHECK(parse_device_list(d65, map, &n) == 0 && n == 64 && map[63] == 1023);
    free(l64); free(l65); free(d64); free(d65);
    static const char *const bad_groups[] = {"", "x", "0,x", "0,", ",0", "0,,1", "-1", "0,-1", "32", "99999999999999999999", "0.5"};
    static const char *const bad_sizes[] = {"", "x", "1,x", "1,", ",1", "0", "1,0", "-1", "nan", "inf", "1e999"};
    int32_t ids[33];
    double sizes[33];
    for (size_t k = 0; k < sizeof bad_groups / sizeof *bad_groups; k++) CHECK(parse_group_list(bad_groups[k], ids, &n) == 1);
    for (size_t k = 0; k < sizeof bad_sizes / sizeof *bad_sizes; k++) CHECK(parse_size_list(bad_sizes[k], sizes, &n) == 1);
    char *g32 = repeated("0", 32), *g40 = repeated("31", 40), *s40 = repeated("0.5", 40);
    CHECK(parse_group_list("0,0,1", ids, &n) == 0 && n == 3 && ids[2] == 1 && parse_group_list(g32, ids, &n) == 0 && n == 32);
    CHECK(parse_group_list(g40, ids, &n) == 0 && n == 33 && ids[32] == 31);                   /* what follows the 33rd entry is not stored */
    CHECK(parse_size_list("1,0.5,1e-300", sizes, &n) == 0 && n == 3 && sizes[1] == 0.5 && parse_size_list(s40, sizes, &n) == 0 && n == 33);
    const int32_t g001[3] = {0, 0, 1}, g002[3] = {0, 0, 2}, g111[3] = {1, 1, 1};
    CHECK(check_groups(3, 3, g001, 0) == 0 && check_groups(3, 3, g001, 3) == 0 && check_groups(3, 3, g001, 2) != 0);
    CHECK(check_groups(3, 3, g002, 0) != 0 && check_groups(3, 3, g111, 0) != 0 && check_groups(2, 3, g001, 0) != 0 && check_groups(1, 1, g001, 0) != 0);
    parse_group_list(g40, ids, &n);
    CHECK(check_groups(33, n, ids, 0) != 0 && check_groups(40, n, ids, 0) != 0);
    for (int k = 0; k < 32; k++) ids[k] = k;
    CHECK(check_groups(32, 32, ids, 0) == 0);
    free(g32); free(g40); free(s40);
}

int main(int argc, char **argv) {
    writers(argc > 1 ? argv[1] : ".");
    parsers();
    if (failures) { fprintf(stderr, "host_writers: %d checks failed\n", failures); return 1; }
    printf("host_writers ok\n");
    return 0;
}
