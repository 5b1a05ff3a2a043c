// batch_bsearch_cpu.cpp -- the one-thread CPU baseline of tools/batch_bsearch_bench.py: bsearch over BSearchAdaptor
// (src/cutting_plane.rs:403-419, :441-466) with the linear feasibility oracle of include/ellhip_batch_bsearch.h, restated
// over the CPU oracle's spaces (oracle/ell_oracle.h: clone, update, xc, tsq).  Built with -ffp-contract=off.
//
//   batch_bsearch_cpu in.bin out.bin
// in.bin:  int64 D, n, J, stable, passes, inner_max, outer_max; double inner_tol, outer_tol, lower, upper, kappa;
//          then per problem a[J][n], c[J], xc0[n]
// out.bin: per problem 4 doubles: feasible, niter, upper, rounds (the counts as doubles)
// stdout:  one JSON line with the best pass's time
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" {
#include "ell_oracle.h"
}

namespace {

template <bool STABLE>
struct Space;
template <>
struct Space<false> {
    using T = orc_ell;
    static T* make(int64_t n, double kappa, const double* xc) { return orc_ell_new(n, kappa, nullptr, nullptr, xc); }
    static T* clone(const T* s) { return orc_ell_clone(s); }
    static void free(T* s) { orc_ell_free(s); }
    static int cut(T* s, const double* g, double b) { return orc_ell_update(s, 0, g, b, 0, 0.0); }
    static double* xc(T* s) { return orc_ell_xc(s); }
    static double tsq(const T* s) { return orc_ell_tsq(s); }
};
template <>
struct Space<true> {
    using T = orc_ellstable;
    static T* make(int64_t n, double kappa, const double* xc) { return orc_ellstable_new(n, kappa, nullptr, nullptr, xc); }
    static T* clone(const T* s) { return orc_ellstable_clone(s); }
    static void free(T* s) { orc_ellstable_free(s); }
    static int cut(T* s, const double* g, double b) { return orc_ellstable_update(s, 0, g, b, 0, 0.0); }
    static double* xc(T* s) { return orc_ellstable_xc(s); }
    static double tsq(const T* s) { return orc_ellstable_tsq(s); }
};

struct Oracle {
    const double* a;
    const double* c;
    int64_t n, J, idx = -1;
    double target = -1e100;
    // the row that answers and its fj, or -1; rows are folded as the walk reaches them (src/example3.rs:29-54)
    int64_t assess(const double* x, double& fj) {
        for (int64_t t = 0; t < J; ++t) {
            idx += 1;
            if (idx == J) idx = 0;
            const double* row = a + idx * n;
            double f = 0.0;
            for (int64_t k = 0; k < n; ++k) f += row[k] * x[k];
            fj = f - (idx == J - 1 ? target : c[idx]);
            if (fj > 0.0) return idx;
        }
        return -1;
    }
};

struct Result {
    double feasible, niter, upper, rounds;
};

template <bool STABLE>
Result solve(Oracle om, int64_t n, const double* xc0, double kappa, double lower, double upper, int64_t inner_max,
             double inner_tol, int64_t outer_max, double outer_tol) {
    using S = Space<STABLE>;
    typename S::T* space = S::make(n, kappa, xc0);
    const double u_orig = upper;
    int64_t niter = outer_max, rounds = 0;
    for (int64_t it = 0; it < outer_max; ++it) {
        const double tau = (upper - lower) / 2.0;
        if (tau < outer_tol) {
            niter = it;
            break;
        }
        double gamma = lower;
        gamma += tau;
        typename S::T* probe = S::clone(space);
        om.target = gamma;
        bool feasible = false;
        for (int64_t k = 0; k < inner_max; ++k) {
            double fj = 0.0;
            const int64_t row = om.assess(S::xc(probe), fj);
            rounds += 1;
            if (row < 0) {
                feasible = true;
                break;
            }
            if (S::cut(probe, om.a + row * n, fj) != 0 || S::tsq(probe) < inner_tol) break;
        }
        if (feasible) {
            const double* x = S::xc(probe);
            double* dst = S::xc(space);
            for (int64_t k = 0; k < n; ++k) dst[k] = x[k];
            upper = gamma;
        } else {
            lower = gamma;
        }
        S::free(probe);
    }
    S::free(space);
    return Result{upper != u_orig ? 1.0 : 0.0, (double)niter, upper, (double)rounds};
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[7];
    double d[5];
    if (fread(h, sizeof(int64_t), 7, f) != 7 || fread(d, sizeof(double), 5, f) != 5) return 2;
    const int64_t D = h[0], n = h[1], J = h[2], stable = h[3], passes = h[4], inner_max = h[5], outer_max = h[6];
    const size_t per = (size_t)(J * n + J + n);
    std::vector<double> in((size_t)D * per);
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
    fclose(f);
    std::vector<Result> out((size_t)D);
    double best = 1e300;
    for (int64_t pass = 0; pass < passes; ++pass) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int64_t b = 0; b < D; ++b) {
            const double* p = in.data() + (size_t)b * per;
            Oracle om{p, p + J * n, n, J};
            out[(size_t)b] = stable ? solve<true>(om, n, p + J * n + J, d[4], d[2], d[3], inner_max, d[0], outer_max, d[1])
                                    : solve<false>(om, n, p + J * n + J, d[4], d[2], d[3], inner_max, d[0], outer_max, d[1]);
        }
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (s < best) best = s;
    }
    double probes = 0.0, rounds = 0.0;
    for (const Result& r : out) {
        probes += r.niter;
        rounds += r.rounds;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(Result), out.size(), f) != out.size()) return 2;
    fclose(f);
    printf("{\"cpu_s\": %.9g, \"probes\": %.0f, \"rounds\": %.0f, \"probes_per_s\": %.9g, \"rounds_per_s\": %.9g}\n", best, probes,
           rounds, probes / best, rounds / best);
    return 0;
}
