/* batch_maxcut_cpu.c -- the one-thread CPU column of tools/batch_maxcut_bench.py: cutting_plane_optim
 * (src/cutting_plane.rs:286-313) over MaxcutOracle (src/oracles/maxcut_oracle.rs:4-50) for every problem of a file, one after
 * the other, in plain C.  The search space is the oracle's Ell (oracle/ell_oracle.c, orc_ell_update, a restatement of
 * Ell::update_core); the oracle below is a literal restatement of assess_optim: the signs, the cut value folded over the
 * upper triangle in row-major order, the gradient folded over full rows, both with the reference's branches.
 *
 * Input (written by the bench tool): int64 B, n, max_iters; double tol; double w[n][n] (one table for every problem);
 * double xc0[B][n].  Problem b starts from Ell::new_with_scalar(100, xc0[b]) with gamma = -inf.
 * Output file: per problem int64 niter, int64 has_best, double gamma, double x_best[n].
 *
 * Usage: batch_maxcut_cpu in.bin out.bin [stable]      prints one JSON line
 * stable: the search space is the oracle's EllStable (orc_ellstable_update, a restatement of EllStable::update_core). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "ell_oracle.h"

static double now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc != 3 && !(argc == 4 && !strcmp(argv[3], "stable"))) {
        fprintf(stderr, "usage: %s in.bin out.bin [stable]\n", argv[0]);
        return 2;
    }
    const int stable = argc == 4;
    FILE *f = fopen(argv[1], "rb");
    int64_t head[3];
    double tol;
    if (!f || fread(head, sizeof(int64_t), 3, f) != 3 || fread(&tol, sizeof tol, 1, f) != 1) return 2;
    const int64_t B = head[0], n = head[1], max_iters = head[2];
    double *w = (double *)malloc((size_t)(n * n) * sizeof(double));
    double *xc0 = (double *)malloc((size_t)(B * n) * sizeof(double));
    double *x = (double *)malloc((size_t)n * sizeof(double));
    double *g = (double *)malloc((size_t)n * sizeof(double));
    double *xbest = (double *)malloc((size_t)n * sizeof(double));
    if (fread(w, sizeof(double), (size_t)(n * n), f) != (size_t)(n * n)) return 2;
    if (fread(xc0, sizeof(double), (size_t)(B * n), f) != (size_t)(B * n)) return 2;
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    int64_t rounds = 0;
    double used = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        orc_ell *space = stable ? NULL : orc_ell_new(n, 100.0, NULL, NULL, xc0 + b * n);
        orc_ellstable *sspace = stable ? orc_ellstable_new(n, 100.0, NULL, NULL, xc0 + b * n) : NULL;
        double gamma = -INFINITY;
        int64_t niter = max_iters, has_best = 0;
        memset(xbest, 0, (size_t)n * sizeof(double));
        const double t0 = now();
        for (int64_t it = 0; it < max_iters; ++it) {
            const double *xc = stable ? orc_ellstable_xc(sspace) : orc_ell_xc(space);
            for (int64_t i = 0; i < n; ++i) x[i] = xc[i] >= 0.0 ? 1.0 : -1.0; /*    maxcut_oracle.rs:22 */
            double cut_value = 0.0; /*                                               :24-31 */
            for (int64_t i = 0; i < n; ++i)
                for (int64_t j = i + 1; j < n; ++j)
                    if (x[i] != x[j]) cut_value += w[i * n + j];
            for (int64_t i = 0; i < n; ++i) { /*                                     :33-41 */
                double gi = 0.0;
                for (int64_t j = 0; j < n; ++j)
                    if (x[i] != x[j]) gi += w[i * n + j];
                g[i] = -(gi * 2.0);
            }
            int status;
            if (cut_value > gamma) { /*                                              :43-45, cutting_plane.rs:301-304 */
                gamma = cut_value;
                memcpy(xbest, xc, (size_t)n * sizeof(double));
                has_best = 1;
                status = stable ? orc_ellstable_update(sspace, 1, g, -cut_value, 0, 0.0) : orc_ell_update(space, 1, g, -cut_value, 0, 0.0);
            } else { /*                                                              :47, cutting_plane.rs:306 */
                status = stable ? orc_ellstable_update(sspace, 0, g, gamma, 0, 0.0) : orc_ell_update(space, 0, g, gamma, 0, 0.0);
            }
            rounds += 1;
            if (status != 0 || (stable ? orc_ellstable_tsq(sspace) : orc_ell_tsq(space)) < tol) { /* :308 */
                niter = it;
                break;
            }
        }
        used += now() - t0;
        fwrite(&niter, sizeof niter, 1, out);
        fwrite(&has_best, sizeof has_best, 1, out);
        fwrite(&gamma, sizeof gamma, 1, out);
        fwrite(xbest, sizeof(double), (size_t)n, out);
        if (stable) orc_ellstable_free(sspace);
        else orc_ell_free(space);
    }
    fclose(out);
    printf("{\"B\": %lld, \"n\": %lld, \"rounds\": %lld, \"seconds\": %.6f, \"iters_per_s\": %.6g}\n", (long long)B,
           (long long)n, (long long)rounds, used, (double)rounds / used);
    free(xbest);
    free(g);
    free(x);
    free(xc0);
    free(w);
    return 0;
}
