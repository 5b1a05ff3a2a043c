// lmi_loop_runner.cpp -- the round-robin LMI problem through the C++ host mirror (ellalgo-rs_amd/host/ellhip/lmi_loop_hip.hpp),
// one JSON object per case: the generic host drivers of cutting_plane.hpp with RoundRobinLmiHost behind the oracle interface
// (one ellhip_lmi_assess_feas and one ellhip_update per iteration), and the device-resident loops of LmiLoopHip, on separate
// handles built from the same matrices and the same kind of search space.  Doubles are printed as their bit patterns.
//
//   lmi_loop_runner                                   the test cases
//   lmi_loop_runner bench <n> <m> <J> <optim|feas> <iters>
//                                                     host clock around both loops (median of 3 after a warm-up), printed only
//                                                     when the two sides agree bit for bit (tools/lmi_loop_bench.py)
//   lmi_loop_runner device <n> <m> <J> <optim|feas> <iters>
//                                                     the host-driven loop once (it counts the block calls of the walk), then
//                                                     the device loop once: what a kernel trace is taken of
//                                                     (tools/lmi_loop_trace.py)
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../ellalgo-rs_amd/host/ellhip/lmi_loop_hip.hpp"

using namespace ellhip;

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static void emit(const std::string& name, size_t niter, const std::optional<Arr>& x, double gamma, double tsq, int idx) {
    printf("{\"case\": \"%s\", \"niter\": %zu, \"has_x\": %s, \"idx\": %d, \"gamma\": \"%016llx\", \"tsq\": \"%016llx\", \"x\": [",
           name.c_str(), niter, x ? "true" : "false", idx, (unsigned long long)bits(gamma), (unsigned long long)bits(tsq));
    if (x)
        for (size_t i = 0; i < x->size(); ++i) printf("%s\"%016llx\"", i ? ", " : "", (unsigned long long)bits((*x)[i]));
    printf("]}\n");
}

// J random pencils that are strictly feasible at x = 0 (B_j diagonally dominant), symmetric F_jk, an objective; a fixed LCG
struct Problem {
    size_t n, m, J;
    std::vector<std::vector<Arr>> F;  // [J][n] m*m
    std::vector<Arr> B;               // [J] m*m
    Arr c;
};

static Problem make_problem(size_t n, size_t m, size_t J, double bscale = 1.0) {
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto uni = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return ((double)(s >> 11) * (1.0 / 9007199254740992.0) - 0.5) * 3.0;
    };
    Problem p{n, m, J, {}, {}, {}};
    for (size_t j = 0; j < J; ++j) {
        std::vector<Arr> fs;
        for (size_t k = 0; k < n; ++k) {
            Arr f(m * m);
            for (size_t a = 0; a < m; ++a)
                for (size_t b = 0; b <= a; ++b) f[a * m + b] = f[b * m + a] = uni();
            fs.push_back(std::move(f));
        }
        p.F.push_back(std::move(fs));
        Arr b(m * m, 0.0);  // symmetric, strictly diagonally dominant: |off-diagonal row sum| <= 1.5 m < 2 m
        for (size_t a = 0; a < m; ++a) {
            for (size_t q = 0; q < a; ++q) b[a * m + q] = b[q * m + a] = bscale * uni();
            b[a * m + a] = bscale * 2.0 * (double)m;
        }
        p.B.push_back(std::move(b));
    }
    for (size_t k = 0; k < n; ++k) p.c.push_back(uni());
    return p;
}

struct Blocks {
    std::vector<std::unique_ptr<LMIOracleHip>> own;
    std::vector<ellhip_lmi*> raw;
    explicit Blocks(const Problem& p) {
        for (size_t j = 0; j < p.J; ++j) {
            own.push_back(std::make_unique<LMIOracleHip>(p.F[j], p.B[j], p.m));
            raw.push_back(own.back()->handle());
        }
    }
};

struct Result {
    size_t niter = 0;
    std::optional<Arr> x;
    double gamma = 0.0, tsq = 0.0, seconds = 0.0;
    int idx = -1;
    size_t block_calls = 0;  // host-driven side: stations that ran a block's oracle
    bool same(const Result& o) const {
        if (niter != o.niter || idx != o.idx || bits(gamma) != bits(o.gamma) || bits(tsq) != bits(o.tsq)) return false;
        if (x.has_value() != o.x.has_value()) return false;
        if (x)
            for (size_t i = 0; i < x->size(); ++i)
                if (bits((*x)[i]) != bits((*o.x)[i])) return false;
        return true;
    }
};

template <int VARIANT>
static Result run_side(const Problem& p, bool optim, bool device, double kappa, double centre, size_t max_iters, double tol) {
    Blocks blocks(p);
    auto space = SpaceHip<VARIANT>::new_with_scalar(kappa, Arr(p.n, centre));
    Result r;
    r.gamma = std::numeric_limits<double>::infinity();
    const auto t0 = std::chrono::steady_clock::now();
    if (device) {
        LmiLoopHip omega(blocks.raw, p.n, optim ? std::optional<Arr>(p.c) : std::nullopt);
        const auto t1 = std::chrono::steady_clock::now();  // (the handle is made once per problem, not per loop)
        std::tie(r.x, r.niter) = optim ? omega.optim(space, r.gamma, Options(max_iters, tol)) : omega.feas(space, Options(max_iters, tol));
        r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        r.idx = omega.idx();
    } else {
        RoundRobinLmiHost omega(blocks.raw, p.n, optim ? std::optional<Arr>(p.c) : std::nullopt);
        std::tie(r.x, r.niter) = optim ? cutting_plane_optim(omega, space, r.gamma, Options(max_iters, tol))
                                       : cutting_plane_feas(omega, space, Options(max_iters, tol));
        r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        r.idx = omega.idx();
        r.block_calls = omega.block_calls();
    }
    r.tsq = space.tsq();
    return r;
}

template <int VARIANT>
static void run(const std::string& name, size_t n, size_t m, size_t J, bool optim, double kappa, double centre,
                size_t max_iters, double tol) {
    const Problem p = make_problem(n, m, J);
    for (int device = 0; device < 2; ++device) {
        const Result r = run_side<VARIANT>(p, optim, device != 0, kappa, centre, max_iters, tol);
        emit(name + (device ? "_device" : "_host"), r.niter, r.x, r.gamma, r.tsq, r.idx);
    }
}

static int bench(size_t n, size_t m, size_t J, bool optim, size_t iters) {
    // feasibility form: B scaled down so that the feasible set around 0 is small against the first ellipsoid and the loop
    // runs for hundreds of iterations, with failing pivots all over the blocks, before it finds a point
    const Problem p = make_problem(n, m, J, optim ? 1.0 : 1e-6);
    const double kappa = 400.0, centre = optim ? 0.0 : 6.0;
    std::vector<double> th, td;
    Result h, d;
    for (int rep = 0; rep < 4; ++rep) {  // the first one warms up
        h = run_side<ELLHIP_SPACE_ELL>(p, optim, false, kappa, centre, iters, 0.0);
        d = run_side<ELLHIP_SPACE_ELL>(p, optim, true, kappa, centre, iters, 0.0);
        if (!h.same(d)) {
            fprintf(stderr, "host-driven and device loops disagree (niter %zu / %zu)\n", h.niter, d.niter);
            return 1;
        }
        if (rep) {
            th.push_back(h.seconds);
            td.push_back(d.seconds);
        }
    }
    std::sort(th.begin(), th.end());
    std::sort(td.begin(), td.end());
    const size_t calls = h.niter < iters ? h.niter + 1 : iters;  // oracle calls made: the stopping iteration counts
    printf("{\"bench\": \"lmi_loop\", \"form\": \"%s\", \"n\": %zu, \"m\": %zu, \"J\": %zu, \"max_iters\": %zu, \"niter\": %zu, "
           "\"oracle_calls\": %zu, \"host_s\": %.6e, \"device_s\": %.6e, \"host_us_per_iter\": %.3f, \"device_us_per_iter\": %.3f, "
           "\"speedup\": %.3f, \"bit_identical\": true}\n",
           optim ? "optim" : "feas", n, m, J, iters, h.niter, calls, th[1], td[1], th[1] * 1e6 / (double)calls,
           td[1] * 1e6 / (double)calls, th[1] / td[1]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 7 && std::string(argv[1]) == "bench")
        return bench((size_t)atoll(argv[2]), (size_t)atoll(argv[3]), (size_t)atoll(argv[4]), std::string(argv[5]) == "optim",
                     (size_t)atoll(argv[6]));
    if (argc == 7 && std::string(argv[1]) == "device") {
        const bool optim = std::string(argv[5]) == "optim";
        const Problem p = make_problem((size_t)atoll(argv[2]), (size_t)atoll(argv[3]), (size_t)atoll(argv[4]), optim ? 1.0 : 1e-6);
        // the host-driven walk first (its kernels are no part of the traced loop): the two walks are the same to the bit, so its
        // count of block calls is the exact number of station slots of the device loop that are not skipped
        const size_t iters = (size_t)atoll(argv[6]);
        const Result h = run_side<ELLHIP_SPACE_ELL>(p, optim, false, 400.0, optim ? 0.0 : 6.0, iters, 0.0);
        const Result r = run_side<ELLHIP_SPACE_ELL>(p, optim, true, 400.0, optim ? 0.0 : 6.0, iters, 0.0);
        if (!h.same(r)) {
            fprintf(stderr, "host-driven and device loops disagree (niter %zu / %zu)\n", h.niter, r.niter);
            return 1;
        }
        printf("{\"device_run\": \"lmi_loop\", \"niter\": %zu, \"active_block_slots\": %zu}\n", r.niter, h.block_calls);
        return 0;
    }
    if (argc != 1) {
        fprintf(stderr, "usage: %s [bench|device n m J optim|feas iters]\n", argv[0]);
        return 2;
    }
    run<ELLHIP_SPACE_ELL>("m70_ell", 8, 70, 2, true, 400.0, 0.0, 2000, 1e-8);
    run<ELLHIP_SPACE_ELL_STABLE>("m70_stable", 8, 70, 2, true, 400.0, 0.0, 2000, 1e-8);
    run<ELLHIP_SPACE_ELL>("feas", 8, 70, 2, false, 400.0, 6.0, 2000, 1e-20);
    return 0;
}
