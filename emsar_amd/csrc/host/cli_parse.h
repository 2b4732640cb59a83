/* cli_parse.h -- the argument parsers of emsar-hip's option switch (emsar_hip_main.c).  Each returns 0 and stores the value, or 1, after
 * which the call site prints its option's own message and the run ends.  They are static and include nothing of the driver, so that
 * tools/host_writers.c can run them under the sanitizers. */
#ifndef EMSAR_CLI_PARSE_H
#define EMSAR_CLI_PARSE_H
#include <errno.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* a whole decimal number in lo .. hi: --bootstrap, --subsample-reps */
static int parse_count(const char *s, long lo, long hi, int *out) {
    char *end; errno = 0;
    const long v = strtol(s, &end, 10);
    if (end == s || *end || errno || v < lo || v > hi) return 1;
    *out = (int)v;
    return 0;
}

/* a non-negative whole number up to 2^64 - 1: --bootstrap-seed, --subsample-seed (strtoull alone would take "-1") */
static int parse_seed(const char *s, uint64_t *out) {
    char *end; errno = 0;
    const unsigned long long v = strtoull(s, &end, 10);
    if (end == s || *end || errno || s[0] == '-') return 1;
    *out = (uint64_t)v;
    return 0;
}

/* a comma-separated list of 1 to 64 numbers in [lo, 1], in (lo, 1] with lo_open: --bootstrap-quantiles, --subsample.  out[64]; the list
 * replaces what an earlier use of the option stored */
static int parse_fraction_list(const char *s, double lo, int lo_open, double *out, int *n) {
    *n = 0;
    for (;;) {
        char *end; errno = 0;
        const double v = strtod(s, &end);
        if (end == s || (*end && *end != ',') || errno || !isfinite(v) || !(lo_open ? v > lo : v >= lo) || !(v <= 1.0) || *n >= 64) return 1;
        out[(*n)++] = v;
        if (!*end) return 0;
        s = end + 1;
    }
}

/* --devices a,b,..: device ids 0 .. 1023, appended to map[64] (the option may repeat, as may an id); what follows the 64th entry is not read */
static int parse_device_list(const char *s, int *map, int *n) {
    while (*s && *n < 64) {
        char *end;
        const long d = strtol(s, &end, 10);
        if (end == s || d < 0 || d > 1023 || (*end && *end != ',')) return 1;
        map[(*n)++] = (int)d;
        s = *end == ',' ? end + 1 : end;
    }
    return *n == 0;
}

/* --compare-groups g0,g1,..: one group id per sample, whole numbers 0 .. 31, at most 33 are stored in out[33] (a 33rd tells the caller that
 * there are too many); the list replaces what an earlier use of the option stored */
static int parse_group_list(const char *s, int32_t *out, int *n) {
    *n = 0;
    for (;;) {
        char *end; errno = 0;
        const long v = strtol(s, &end, 10);
        if (end == s || (*end && *end != ',') || errno || v < 0 || v > 31) return 1;
        if (*n < 33) out[(*n)++] = (int32_t)v;
        if (!*end) return 0;
        s = end + 1;
    }
}

/* --compare-sizes s0,s1,..: one size factor per sample, finite and positive, stored like the group ids */
static int parse_size_list(const char *s, double *out, int *n) {
    *n = 0;
    for (;;) {
        char *end; errno = 0;
        const double v = strtod(s, &end);
        if (end == s || (*end && *end != ',') || errno || !isfinite(v) || !(v > 0.0)) return 1;
        if (*n < 33) out[(*n)++] = v;
        if (!*end) return 0;
        s = end + 1;
    }
}

/* The groups of a K-sample job: n_groups ids for n_samples samples.  0, or the message of what is wrong: a length that is not the number
 * of samples, fewer than two or more than 32 samples, an id that is not 0 .. G-1 without gaps (G = the largest id + 1: an empty group) */
static const char *check_groups(int n_samples, int n_groups, const int32_t *group_of, int n_sizes) {
    if (n_samples < 2) return "--compare-groups needs -M and at least two samples.";
    if (n_samples > 32) return "--compare-groups takes at most 32 samples.";
    if (n_groups != n_samples) return "--compare-groups wants one group id per sample.";
    if (n_sizes && n_sizes != n_samples) return "--compare-sizes wants one size factor per sample.";
    int32_t G = 0;
    uint32_t seen = 0;
    for (int k = 0; k < n_groups; k++) { seen |= 1u << group_of[k]; if (group_of[k] + 1 > G) G = group_of[k] + 1; }
    if (seen != (G == 32 ? 0xffffffffu : (1u << G) - 1u)) return "--compare-groups: the group ids must be 0 .. G-1 with no group empty.";
    return 0;
}
#endif
