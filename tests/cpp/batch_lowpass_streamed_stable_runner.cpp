// batch_lowpass_streamed_stable_runner.cpp -- seven low-pass design problems past the LDS engine's filter lengths (n = 130:
// the test family wp = 0.08 + 0.01 (s % 6), ws = wp + 0.08 + 0.01 (s % 3), d = 0.02 + 0.01 (s % 6), limits (1 - d)^2,
// (1 + d)^2, 0.1 for s = 0 .. 5, then the loose specification 0.12, 0.20, 0.5, 1.5, 0.3) on EllStable::new_with_scalar(40, 0),
// max_iters 1500, tolerance 1e-14, through the C++ mirror of the batched device loop on a streamed EllStable batch handle
// (host/ellhip/batch_lowpass_hip.hpp).  Prints one JSON object per specification.
#include <cstdio>

#include "../../ellalgo-rs_amd/host/ellhip/batch_lowpass_hip.hpp"

using namespace ellhip;

int main() {
    const size_t n = 130;
    std::vector<LowpassSpec> specs;
    Arr gamma;
    for (size_t s = 0; s < 6; ++s) {
        const double wp = 0.08 + 0.01 * (double)(s % 6);
        const double ws = wp + 0.08 + 0.01 * (double)(s % 3);
        const double d = 0.02 + 0.01 * (double)(s % 6);
        specs.push_back(LowpassSpec{wp, ws, (1 - d) * (1 - d), (1 + d) * (1 + d), 0.1});
        gamma.push_back(0.1);
    }
    specs.push_back(LowpassSpec{0.12, 0.20, 0.5, 1.5, 0.3});
    gamma.push_back(0.3);
    const size_t B = specs.size();
    BatchLowpassHip problems = BatchLowpassHip::streamed(n, specs);
    EllStableBatchStreamedHip spaces = EllStableBatchStreamedHip::new_with_scalar(Arr(B, 40.0), std::vector<Arr>(B, Arr(n, 0.0)));
    if (!spaces.is_streamed()) return 1;
    const BatchLowpassResult r = problems.optim(spaces, gamma, Options(1500, 1e-14));
    const std::vector<BatchLowpassHip::Fields> f = problems.fields();
    for (size_t b = 0; b < B; ++b) {
        const Arr x = r.x_best[b].value_or(Arr(n, 0.0));
        printf("{\"case\": \"sweep_%zu\", \"niter\": %zu, \"gamma\": %.17g, \"status\": %d, \"has_best\": %d, \"idx1\": %d, "
               "\"idx2\": %d, \"idx3\": %d, \"kmax\": %d, \"x_best\": [",
               b, r.niter[b], gamma[b], (int)r.status[b], r.x_best[b].has_value() ? 1 : 0, f[b].idx1, f[b].idx2, f[b].idx3,
               f[b].kmax);
        for (size_t j = 0; j < n; ++j) printf("%s%.17g", j ? ", " : "", x[j]);
        printf("]}\n");
    }
    // cutting_plane_feas on fresh spaces and cursors: the family has no feasible point, the loose specification has
    problems.reset();
    EllStableBatchStreamedHip again = EllStableBatchStreamedHip::new_with_scalar(Arr(B, 40.0), std::vector<Arr>(B, Arr(n, 0.0)));
    const BatchLowpassResult q = problems.feas(again, Options(1500, 1e-14));
    for (size_t b = 0; b < B; ++b)
        printf("{\"case\": \"feas_%zu\", \"niter\": %zu, \"status\": %d, \"has_best\": %d}\n", b, q.niter[b], (int)q.status[b],
               q.x_best[b].has_value() ? 1 : 0);
    return 0;
}
