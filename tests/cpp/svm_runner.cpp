// svm_runner.cpp -- the SVM oracle through the C++ host mirror (ellalgo-rs_amd/host/ellhip/svm_hip.hpp), one JSON object
// per case: the generic host driver of cutting_plane.hpp with SvmOracleHip behind the OracleOptim interface, and the
// device-resident loop, on the same data and the same kind of search space.  Doubles are printed as their bit patterns.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ellalgo-rs_amd/host/ellhip/svm_hip.hpp"

using namespace ellhip;

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

static void emit(const std::string& name, size_t niter, const std::optional<Arr>& x, double gamma, double tsq) {
    printf("{\"case\": \"%s\", \"niter\": %zu, \"has_x\": %s, \"gamma\": \"%016llx\", \"tsq\": \"%016llx\", \"x\": [", name.c_str(),
           niter, x ? "true" : "false", (unsigned long long)bits(gamma), (unsigned long long)bits(tsq));
    if (x)
        for (size_t i = 0; i < x->size(); ++i) printf("%s\"%016llx\"", i ? ", " : "", (unsigned long long)bits((*x)[i]));
    printf("]}\n");
}

// two clouds around +-c (separable when `shift` is large), labels +-1; a fixed LCG
static void make_data(size_t m, size_t nfeat, double shift, Arr& data, std::vector<int32_t>& labels) {
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto uni = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    };
    data.assign(m * nfeat, 0.0);
    labels.assign(m, 0);
    for (size_t i = 0; i < m; ++i) {
        labels[i] = (i % 3 == 0) ? -1 : 1;
        for (size_t j = 0; j < nfeat; ++j) data[i * nfeat + j] = uni() + (j == 0 ? shift * labels[i] : 0.0);
    }
}

template <int VARIANT>
static void run(const std::string& name, size_t m, size_t nfeat, double shift, double kappa, size_t max_iters, double tol) {
    Arr data;
    std::vector<int32_t> labels;
    make_data(m, nfeat, shift, data, labels);
    SvmOracleHip omega(data, nfeat, labels);
    {
        auto space = SpaceHip<VARIANT>::new_with_scalar(kappa, Arr(nfeat + 1, 0.0));
        double gamma = -1.0;
        auto [x, niter] = cutting_plane_optim(omega, space, gamma, Options(max_iters, tol));
        emit(name + "_host", niter, x, gamma, space.tsq());
    }
    {
        auto space = SpaceHip<VARIANT>::new_with_scalar(kappa, Arr(nfeat + 1, 0.0));
        double gamma = -1.0;
        auto [x, niter] = cutting_plane_optim_device(omega, space, gamma, Options(max_iters, tol));
        emit(name + "_device", niter, x, gamma, space.tsq());
    }
}

int main() {
    run<ELLHIP_SPACE_ELL>("separable_ell", 1000, 7, 2.0, 10.0, 2000, 1e-14);
    run<ELLHIP_SPACE_ELL>("overlap_ell", 777, 5, 0.1, 10.0, 2000, 1e-8);
    run<ELLHIP_SPACE_ELL_STABLE>("overlap_stable", 777, 5, 0.1, 10.0, 2000, 1e-8);
    run<ELLHIP_SPACE_ELL>("max_iters_ell", 4099, 63, 0.1, 10.0, 150, 1e-30);
    return 0;
}
