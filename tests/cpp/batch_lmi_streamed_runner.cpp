// batch_lmi_streamed_runner.cpp -- one small sweep of LMI problems past the LDS engine's n = 128 through the C++ mirror of
// the batched device loops (host/ellhip/batch_lmi_hip.hpp) on a streamed batch handle, Ell or EllStable, gamma = +inf.  The
// problems come from a file the test writes: int64 B, n, J, max_iters, stable, feas, shared, m[J]; double tol; double
// kappa[B]; double xc[B][n]; double c[B][n]; then per block j double f[B or 1][n][m_j][m_j] and double b[B][m_j][m_j].
// Prints one JSON object per problem; doubles are printed as their bit patterns.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../ellalgo-rs_amd/host/ellhip/batch_lmi_hip.hpp"

using namespace ellhip;

static unsigned long long bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return (unsigned long long)u;
}

static bool read(FILE* f, Arr& a, size_t count) {
    a.resize(count);
    return fread(a.data(), sizeof(double), count, f) == count;
}

template <class Spaces>
static int run(BatchLmiHip& problems, size_t B, size_t n, const Arr& kappa, const std::vector<Arr>& xc, bool feas,
               size_t max_iters, double tol) {
    Spaces spaces = Spaces::new_with_scalar(kappa, xc);
    if (!spaces.is_streamed()) return 1;
    Arr gamma(B, INFINITY);
    const BatchLmiResult r = feas ? problems.feas(spaces, Options(max_iters, tol)) : problems.optim(spaces, gamma, Options(max_iters, tol));
    const std::vector<int32_t> idx = problems.idx();
    for (size_t b = 0; b < B; ++b) {
        printf("{\"case\": \"sweep_%zu\", \"niter\": %zu, \"gamma\": \"%016llx\", \"status\": %d, \"has_x\": %d, \"idx\": %d, \"x\": [",
               b, r.niter[b], bits(gamma[b]), (int)r.status[b], r.x_best[b].has_value() ? 1 : 0, (int)idx[b]);
        if (r.x_best[b])
            for (size_t j = 0; j < n; ++j) printf("%s\"%016llx\"", j ? ", " : "", bits((*r.x_best[b])[j]));
        printf("]}\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[7];
    if (fread(head, sizeof(int64_t), 7, f) != 7) return 2;
    const size_t B = (size_t)head[0], n = (size_t)head[1], J = (size_t)head[2];
    const bool stable = head[4] != 0, feas = head[5] != 0, shared = head[6] != 0;
    std::vector<int64_t> m64(J);
    double tol;
    if (fread(m64.data(), sizeof(int64_t), J, f) != J || fread(&tol, sizeof tol, 1, f) != 1) return 2;
    const std::vector<size_t> m(m64.begin(), m64.end());
    Arr kappa, flat;
    if (!read(f, kappa, B)) return 2;
    std::vector<Arr> xc(B);
    std::vector<LmiProblem> problems(B);
    for (size_t b = 0; b < B; ++b)
        if (!read(f, xc[b], n)) return 2;
    for (size_t b = 0; b < B; ++b) {
        if (!read(f, problems[b].c, n)) return 2;
        if (feas) problems[b].c.clear();
        problems[b].mat_f.resize(J);
        problems[b].mat_b.resize(J);
    }
    for (size_t j = 0; j < J; ++j) {
        for (size_t b = 0; b < (shared ? 1 : B); ++b)
            if (!read(f, problems[b].mat_f[j], n * m[j] * m[j])) return 2;
        for (size_t b = 1; shared && b < B; ++b) problems[b].mat_f[j] = problems[0].mat_f[j];
        for (size_t b = 0; b < B; ++b)
            if (!read(f, problems[b].mat_b[j], m[j] * m[j])) return 2;
    }
    fclose(f);
    BatchLmiHip handle = shared ? BatchLmiHip::streamed_shared(problems, n, m) : BatchLmiHip::streamed(problems, n, m);
    return stable ? run<EllStableBatchStreamedHip>(handle, B, n, kappa, xc, feas, (size_t)head[3], tol)
                  : run<EllBatchStreamedHip>(handle, B, n, kappa, xc, feas, (size_t)head[3], tol);
}
