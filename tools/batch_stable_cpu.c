/* batch_stable_cpu.c -- the one-thread CPU column of tools/batch_stable_bench.py: the oracle's EllStable update
 * (oracle/ell_oracle.c, orc_ellstable_update, a restatement of EllStable::update_core) called in a plain C loop, B spaces x K
 * central cuts per round, no Python per call.  Each round starts the B spaces again from the same packed buffer (a copy of
 * n^2 doubles per space and round, the CPU's counterpart of the engine's HBM load per launch), so that long runs do not
 * drift into subnormal numbers.
 *
 * Usage: batch_stable_cpu n B K seconds       prints one JSON line */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "ell_oracle.h"

static uint64_t lcg = 0x5EEDULL;
static double urand(void) {
    lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(lcg >> 11) * (1.0 / 9007199254740992.0);
}
static double now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s n B K seconds\n", argv[0]);
        return 2;
    }
    const int64_t n = atoll(argv[1]), B = atoll(argv[2]), K = atoll(argv[3]);
    const double budget = atof(argv[4]);
    double *mq0 = (double *)malloc((size_t)(n * n) * sizeof(double));
    double *grads = (double *)malloc((size_t)(K * B * n) * sizeof(double));
    /* random factor: diagonal 0.5 .. 1.5, factor and scratch ~ 0.1 / sqrt(n) (tests/util.py: random_factor) */
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) mq0[i * n + j] = (i == j) ? 0.5 + urand() : (urand() - 0.5) * 0.2 / sqrt((double)n);
    for (int64_t c = 0; c < K * B; ++c) {
        double s = 0.0;
        for (int64_t i = 0; i < n; ++i) s += (grads[c * n + i] = urand() - 0.5) * grads[c * n + i];
        for (int64_t i = 0; i < n; ++i) grads[c * n + i] /= sqrt(s);
    }
    orc_ellstable **sp = (orc_ellstable **)malloc((size_t)B * sizeof(*sp));
    for (int64_t b = 0; b < B; ++b) sp[b] = orc_ellstable_new(n, 1.0, mq0, NULL, NULL);
    int64_t updates = 0, fails = 0;
    double used = 0.0;
    while (used < budget) {
        for (int64_t b = 0; b < B; ++b) { /* (not timed) */
            memcpy(orc_ellstable_mq(sp[b]), mq0, (size_t)(n * n) * sizeof(double));
            memset(orc_ellstable_xc(sp[b]), 0, (size_t)n * sizeof(double));
            sp[b]->kappa = 1.0;
        }
        const double t0 = now();
        for (int64_t k = 0; k < K; ++k)
            for (int64_t b = 0; b < B; ++b) fails += orc_ellstable_update(sp[b], 1, grads + (k * B + b) * n, 0.0, 0, 0.0) != 0;
        used += now() - t0;
        updates += K * B;
    }
    printf("{\"n\": %lld, \"B\": %lld, \"K\": %lld, \"updates\": %lld, \"failed\": %lld, \"seconds\": %.4f, "
           "\"updates_per_s\": %.6g}\n",
           (long long)n, (long long)B, (long long)K, (long long)updates, (long long)fails, used, (double)updates / used);
    for (int64_t b = 0; b < B; ++b) orc_ellstable_free(sp[b]);
    free(sp);
    free(grads);
    free(mq0);
    return 0;
}
