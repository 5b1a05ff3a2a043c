// batch_stable_runner.cpp -- the reference's three EllStable quasi-convex cases (src/quasicvx.rs:101-133) solved side by
// side on the batched engine through EllStableBatchHip (one launch for the bias cuts and one for the central cuts per
// round), and each of them once more on its own EllStableHip handle with the generic cutting_plane_optim driver.
// Prints one JSON object per case.
#include <cmath>
#include <cstdio>
#include <limits>
#include <optional>
#include <string>

#include "../../ellalgo-rs_amd/host/ellhip/ell_batch_hip.hpp"
#include "example_oracles.hpp"

using namespace ellhip;

struct Case {
    std::string name;
    double kappa;  // new_with_scalar(kappa, xc) or new(diag, xc) with kappa = 1
    Arr diag, xc;
    double gamma0;
    Options options;
};

int main() {
    const double INF = std::numeric_limits<double>::infinity();
    const std::vector<Case> cases = {
        {"quasicvx_feasible_stable", 1.0, {10.0, 10.0}, {0.0, 0.0}, 0.0, Options(2000, 1e-8)},
        {"quasicvx_infeasible1_stable", 10.0, {1.0, 1.0}, {100.0, 100.0}, 0.0, Options{}},
        {"quasicvx_infeasible2_stable", 1.0, {10.0, 10.0}, {0.0, 0.0}, 100.0, Options{}},
    };
    const size_t B = cases.size(), n = 2;
    // ---- one by one (the reference's way)
    std::vector<size_t> niter_single(B);
    std::vector<double> gamma_single(B);
    std::vector<std::optional<Arr>> x_single(B);
    for (size_t b = 0; b < B; ++b) {
        EllStableHip space = cases[b].kappa != 1.0 ? EllStableHip::new_with_scalar(cases[b].kappa, cases[b].xc)
                                                   : EllStableHip::make(cases[b].diag, cases[b].xc);
        examples::QuasiCvx omega;
        double gamma = cases[b].gamma0;
        auto [x, niter] = cutting_plane_optim(omega, space, gamma, cases[b].options);
        niter_single[b] = niter;
        gamma_single[b] = gamma;
        x_single[b] = x;
    }
    // ---- all together: cutting_plane_optim's loop over the batch.  A space that is not due in a launch gets a cut that
    // fails (bias: beta = +inf; central: a parallel cut with beta1 < 0), which leaves D, U, xc and kappa untouched.
    Arr kappa(B);
    std::vector<Arr> mq(B, Arr(n * n, 0.0)), xc0(B);
    for (size_t b = 0; b < B; ++b) {
        kappa[b] = cases[b].kappa;
        for (size_t i = 0; i < n; ++i) mq[b][i * n + i] = cases[b].diag[i];
        xc0[b] = cases[b].xc;
    }
    EllStableBatchHip batch = EllStableBatchHip::new_with_matrix(kappa, mq, xc0);
    std::vector<examples::QuasiCvx> omegas(B);
    std::vector<double> gamma(B);
    std::vector<std::optional<Arr>> x_best(B);
    std::vector<size_t> niter(B);
    std::vector<bool> done(B, false);
    for (size_t b = 0; b < B; ++b) {
        gamma[b] = cases[b].gamma0;
        niter[b] = cases[b].options.max_iters;
    }
    const std::pair<Arr, ParallelCut> noop_bias{Arr(n, 1.0), ParallelCut{INF, std::nullopt}};
    const std::pair<Arr, ParallelCut> noop_central{Arr(n, 1.0), ParallelCut{0.0, -1.0}};
    for (size_t it = 0;; ++it) {
        bool any = false;
        for (size_t b = 0; b < B; ++b)
            if (!done[b] && it >= cases[b].options.max_iters) done[b] = true;
            else any = any || !done[b];
        if (!any) break;
        const std::vector<Arr> xc = batch.xc();
        std::vector<std::pair<Arr, ParallelCut>> a(B, noop_bias), c(B, noop_central);
        std::vector<bool> shrunk(B, false);
        for (size_t b = 0; b < B; ++b) {
            if (done[b]) continue;
            auto [cut, sh] = omegas[b].assess_optim(xc[b], gamma[b]);
            shrunk[b] = sh;
            const std::pair<Arr, ParallelCut> pc{cut.first, ParallelCut{cut.second.beta, std::nullopt}};
            if (sh) {
                x_best[b] = xc[b];
                c[b] = pc;
            } else {
                a[b] = pc;
            }
        }
        // (a failed cut still rewrites tsq, so tsq is read after the launch that carried the real cut)
        const auto st_a = batch.update_bias_cut(a);
        const Arr tsq_a = batch.tsq();
        const auto st_c = batch.update_central_cut(c);
        const Arr tsq_c = batch.tsq();
        for (size_t b = 0; b < B; ++b) {
            if (done[b]) continue;
            const CutStatus st = shrunk[b] ? st_c[b] : st_a[b];
            const double tsq_b = shrunk[b] ? tsq_c[b] : tsq_a[b];
            if (st != CutStatus::Success || tsq_b < cases[b].options.tolerance) {
                done[b] = true;
                niter[b] = it;
            }
        }
    }
    for (size_t b = 0; b < B; ++b) {
        double dx = 0.0;
        const bool same_has_x = x_best[b].has_value() == x_single[b].has_value();
        if (same_has_x && x_best[b])
            for (size_t i = 0; i < n; ++i) dx = std::fmax(dx, std::fabs((*x_best[b])[i] - (*x_single[b])[i]));
        printf("{\"case\": \"%s\", \"niter_batch\": %zu, \"niter_single\": %zu, \"has_x_batch\": %s, "
               "\"has_x_single\": %s, \"gamma_batch\": %.17g, \"gamma_single\": %.17g, \"max_dx\": %.3g}\n",
               cases[b].name.c_str(), niter[b], niter_single[b], x_best[b] ? "true" : "false",
               x_single[b] ? "true" : "false", gamma[b], gamma_single[b], dx);
    }
    return 0;
}
