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
#endif
