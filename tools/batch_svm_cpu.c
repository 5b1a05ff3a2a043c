/* batch_svm_cpu.c -- the one-thread CPU column of tools/batch_svm_bench.py: cutting_plane_optim (src/cutting_plane.rs:286-313)
 * over SvmOracle (src/oracles/svm_oracle.rs:4-58) for every problem of a file, one after the other, in plain C.  The search
 * space is the oracle's Ell (oracle/ell_oracle.c, orc_ell_update, a restatement of Ell::update_core); the scan below is a
 * literal restatement of assess_optim: margins folded left to right from -0.0, the minimum replaced only by `<`.
 *
 * Input (written by the bench tool): int64 B, m, nfeat, max_iters; double tol; double data[B][m][nfeat];
 * int32 labels[B][m].  Every problem starts from Ell::new_with_scalar(100, 0) with gamma = +inf.
 * Output file: per problem int64 niter, double gamma, double x_best[nfeat + 1].
 *
 * Usage: batch_svm_cpu in.bin out.bin [stable]      prints one JSON line
 * stable: the search space is the oracle's EllStable (orc_ellstable_update, a restatement of EllStable::update_core),
 * from EllStable::new_with_scalar(100, 0). */
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
    int64_t head[4];
    double tol;
    if (!f || fread(head, sizeof(int64_t), 4, f) != 4 || fread(&tol, sizeof tol, 1, f) != 1) return 2;
    const int64_t B = head[0], m = head[1], nfeat = head[2], max_iters = head[3], n = nfeat + 1;
    double *data = (double *)malloc((size_t)(B * m * nfeat) * sizeof(double));
    int32_t *labels = (int32_t *)malloc((size_t)(B * m) * sizeof(int32_t));
    double *g = (double *)malloc((size_t)n * sizeof(double));
    double *xbest = (double *)malloc((size_t)n * sizeof(double));
    if (fread(data, sizeof(double), (size_t)(B * m * nfeat), f) != (size_t)(B * m * nfeat)) return 2;
    if (fread(labels, sizeof(int32_t), (size_t)(B * m), f) != (size_t)(B * m)) return 2;
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    int64_t rounds = 0;
    double used = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const double *d = data + b * m * nfeat;
        const int32_t *lab = labels + b * m;
        orc_ell *space = stable ? NULL : orc_ell_new(n, 100.0, NULL, NULL, NULL);
        orc_ellstable *sspace = stable ? orc_ellstable_new(n, 100.0, NULL, NULL, NULL) : NULL;
        double gamma = INFINITY;
        int64_t niter = max_iters;
        memset(xbest, 0, (size_t)n * sizeof(double));
        const double t0 = now();
        for (int64_t it = 0; it < max_iters; ++it) {
            const double *x = stable ? orc_ellstable_xc(sspace) : orc_ell_xc(space);
            double min_val = INFINITY; /*                                   svm_oracle.rs:28-40 */
            int64_t min_idx = 0;
            for (int64_t i = 0; i < m; ++i) {
                double a = -0.0;
                for (int64_t j = 0; j < nfeat; ++j) a = a + x[j] * d[i * nfeat + j];
                const double margin = (double)lab[i] * (a + x[nfeat]);
                if (margin < min_val) {
                    min_val = margin;
                    min_idx = i;
                }
            }
            double beta;
            if (min_val >= 1.0) { /*                                        :42-45 */
                for (int64_t j = 0; j < n; ++j) g[j] = 0.0;
                beta = 0.0;
                gamma = 0.0;
            } else { /*                                                     :47-57 */
                const double ny = -(double)lab[min_idx];
                for (int64_t j = 0; j < nfeat; ++j) g[j] = ny * d[min_idx * nfeat + j];
                g[nfeat] = ny;
                beta = min_val;
                gamma = min_val;
            }
            memcpy(xbest, x, (size_t)n * sizeof(double)); /*                cutting_plane.rs:303 */
            const int status = stable ? orc_ellstable_update(sspace, 1, g, beta, 0, 0.0) : orc_ell_update(space, 1, g, beta, 0, 0.0);
            rounds += 1;
            if (status != 0 || (stable ? orc_ellstable_tsq(sspace) : orc_ell_tsq(space)) < tol) { /* :308 */
                niter = it;
                break;
            }
        }
        used += now() - t0;
        fwrite(&niter, sizeof niter, 1, out);
        fwrite(&gamma, sizeof gamma, 1, out);
        fwrite(xbest, sizeof(double), (size_t)n, out);
        if (stable) orc_ellstable_free(sspace);
        else orc_ell_free(space);
    }
    fclose(out);
    printf("{\"B\": %lld, \"m\": %lld, \"nfeat\": %lld, \"rounds\": %lld, \"seconds\": %.6f, \"iters_per_s\": %.6g}\n",
           (long long)B, (long long)m, (long long)nfeat, (long long)rounds, used, (double)rounds / used);
    free(xbest);
    free(g);
    free(labels);
    free(data);
    return 0;
}
