// batch_profit_cpu.cpp -- the one-thread CPU column of tools/batch_profit_bench.py: cutting_plane_optim
// (src/cutting_plane.rs:286-313) over ProfitOracle / ProfitRbOracle and cutting_plane_optim_q (:331-374) over ProfitOracleQ
// (src/oracles/profit_oracle.rs) for every problem of a file, one after the other.  The search space is the oracle's Ell or
// EllStable (oracle/ell_oracle.c); exp and log are csrc/ell_math.hpp, so the results can be compared with the device's bit for
// bit.
//
// Input (written by the bench tool): int64 B, kind, max_iters, stable, passes; double tol; double cst[B][8] (ln(p A), ln k, v[2], a[2],
// uie[2]: the constructor's work is the caller's); double xc0[B][2].  Problem b starts from new_with_scalar(100, xc0[b]), gamma = 0.
// The whole file is solved `passes` times, so that the clock runs for a while; the output is the first pass's.
// Output file: per problem int64 niter, int64 has_best, double gamma, double x_best[2].
//
// Usage: batch_profit_cpu in.bin out.bin      prints one JSON line
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <vector>

#include "ell_math.hpp"
#include "ell_oracle.h"

using ellhip::ell_exp;
using ellhip::ell_log;

static double now() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

struct Oracle {
    const double* c;  // log_p_scale, log_k, v0, v1, a0, a1, uie0, uie1
    int idx = -1;
    double a0 = 0, a1 = 0, log_cobb = 0, vx = 0, q0 = 0, q1 = 0, yd0 = 0, yd1 = 0;

    bool feas(const double* y, double gamma, double* g, double& beta) {  // :35-65
        for (int t = 0; t < 2; ++t) {
            idx += 1;
            if (idx == 2) idx = 0;
            double fj;
            if (idx == 0) {
                fj = y[0] - c[1];
            } else {
                log_cobb = c[0] + ((0.0 + a0 * y[0]) + a1 * y[1]);
                q0 = c[2] * ell_exp(y[0]);
                q1 = c[3] * ell_exp(y[1]);
                vx = q0 + q1;
                fj = ell_log(gamma + vx) - log_cobb;
            }
            if (fj > 0.0) {
                if (idx == 0) {
                    g[0] = 1.0;
                    g[1] = 0.0;
                } else {
                    g[0] = q0 / (gamma + vx) - a0;
                    g[1] = q1 / (gamma + vx) - a1;
                }
                beta = fj;
                return true;
            }
        }
        return false;
    }
    bool optim(const double* y, double& gamma, double* g, double& beta) {  // :70-78; returns shrunk
        if (feas(y, gamma, g, beta)) return false;
        const double exp_val = ell_exp(log_cobb);
        gamma = exp_val - vx;
        g[0] = q0 / exp_val - a0;
        g[1] = q1 / exp_val - a1;
        beta = 0.0;
        return true;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    int64_t head[5];
    double tol;
    if (!f || fread(head, sizeof(int64_t), 5, f) != 5 || fread(&tol, sizeof tol, 1, f) != 1) return 2;
    const int64_t B = head[0], kind = head[1], max_iters = head[2], stable = head[3], passes = head[4];
    std::vector<double> cst((size_t)B * 8), xc0((size_t)B * 2);
    if (fread(cst.data(), sizeof(double), cst.size(), f) != cst.size()) return 2;
    if (fread(xc0.data(), sizeof(double), xc0.size(), f) != xc0.size()) return 2;
    fclose(f);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    int64_t rounds = 0;
    double used = 0.0;
    for (int64_t pass = 0; pass < passes; ++pass)
    for (int64_t b = 0; b < B; ++b) {
        orc_ell* space = stable ? nullptr : orc_ell_new(2, 100.0, nullptr, nullptr, &xc0[2 * b]);
        orc_ellstable* sspace = stable ? orc_ellstable_new(2, 100.0, nullptr, nullptr, &xc0[2 * b]) : nullptr;
        auto update = [&](int k, const double* g, double beta) {
            return stable ? orc_ellstable_update(sspace, k, g, beta, 0, 0.0) : orc_ell_update(space, k, g, beta, 0, 0.0);
        };
        Oracle om;
        om.c = &cst[8 * b];
        om.a0 = om.c[4];
        om.a1 = om.c[5];
        double gamma = 0.0, xbest[2] = {0.0, 0.0}, g[2], beta = 0.0;
        int64_t niter = max_iters, has_best = 0;
        bool retry = false;
        const double t0 = now();
        for (int64_t it = 0; it < max_iters; ++it) {
            const double* xc = stable ? orc_ellstable_xc(sspace) : orc_ell_xc(space);
            const double y[2] = {xc[0], xc[1]};
            rounds += 1;
            if (kind != 2) {
                if (kind == 1) {  // :115-123
                    om.a0 = om.c[4] + (y[0] > 0.0 ? -om.c[6] : om.c[6]);
                    om.a1 = om.c[5] + (y[1] > 0.0 ? -om.c[7] : om.c[7]);
                }
                const bool shrunk = om.optim(y, gamma, g, beta);
                if (shrunk) {
                    memcpy(xbest, y, sizeof xbest);
                    has_best = 1;
                }
                const int status = update(shrunk ? 1 : 0, g, beta);
                if (status != 0 || (stable ? orc_ellstable_tsq(sspace) : orc_ell_tsq(space)) < tol) {
                    niter = it;
                    break;
                }
                continue;
            }
            bool shrunk = false, more_alt = !retry, at_y = false;  // :145-162
            if (!retry) {
                at_y = om.feas(y, gamma, g, beta);
                if (!at_y) {
                    double d0 = round(ell_exp(y[0])), d1 = round(ell_exp(y[1]));
                    if (d0 == 0.0) d0 = 1.0;
                    if (d1 == 0.0) d1 = 1.0;
                    om.yd0 = ell_log(d0);
                    om.yd1 = ell_log(d1);
                }
            }
            double xq[2] = {y[0], y[1]};
            if (!at_y) {
                const double yd[2] = {om.yd0, om.yd1};
                shrunk = om.optim(yd, gamma, g, beta);
                beta = beta + ((0.0 + g[0] * (yd[0] - y[0])) + g[1] * (yd[1] - y[1]));
                xq[0] = yd[0];
                xq[1] = yd[1];
            }
            if (shrunk) {  // src/cutting_plane.rs:347-371
                memcpy(xbest, xq, sizeof xbest);
                has_best = 1;
                retry = false;
            }
            const int status = update(2, g, beta);
            if (status == 0) retry = false;
            if (status == 1 || (status == 2 && !more_alt)) {
                niter = it;
                break;
            }
            if (status == 2) retry = true;
            if ((stable ? orc_ellstable_tsq(sspace) : orc_ell_tsq(space)) < tol) {
                niter = it;
                break;
            }
        }
        used += now() - t0;
        if (pass == 0) {
            fwrite(&niter, sizeof niter, 1, out);
            fwrite(&has_best, sizeof has_best, 1, out);
            fwrite(&gamma, sizeof gamma, 1, out);
            fwrite(xbest, sizeof(double), 2, out);
        }
        if (stable) orc_ellstable_free(sspace);
        else orc_ell_free(space);
    }
    fclose(out);
    printf("{\"B\": %lld, \"rounds\": %lld, \"seconds\": %.6f, \"iters_per_s\": %.6g}\n", (long long)B, (long long)rounds, used,
           (double)rounds / used);
    return 0;
}
