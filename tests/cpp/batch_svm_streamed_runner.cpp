// batch_svm_streamed_runner.cpp -- one small sweep of SVM problems past the LDS engine's 127 features through the C++ mirror
// of the batched device loop (host/ellhip/batch_svm_hip.hpp) on a streamed batch handle: Ell::new_with_scalar(100, 0) or
// EllStable::new_with_scalar(100, 0), gamma = +inf.  The problems come from a file the test writes: int64 B, m, nfeat,
// max_iters, stable; double tol; double data[B][m][nfeat]; int32 labels[B][m].  Prints one JSON object per problem; doubles
// are printed as their bit patterns.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../ellalgo-rs_amd/host/ellhip/batch_svm_hip.hpp"

using namespace ellhip;

static unsigned long long bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof u);
    return (unsigned long long)u;
}

template <class Spaces>
static int run(BatchSvmHip& problems, size_t B, size_t n, size_t max_iters, double tol) {
    Spaces spaces = Spaces::new_with_scalar(Arr(B, 100.0), std::vector<Arr>(B, Arr(n, 0.0)));
    if (!spaces.is_streamed()) return 1;
    Arr gamma(B, INFINITY);
    const BatchSvmResult r = problems.optim(spaces, gamma, Options(max_iters, tol));
    const std::vector<BatchSvmHip::Last> last = problems.last();
    for (size_t b = 0; b < B; ++b) {
        printf("{\"case\": \"sweep_%zu\", \"niter\": %zu, \"gamma\": \"%016llx\", \"status\": %d, \"has_best\": %d, "
               "\"min_idx\": %zu, \"min_val\": \"%016llx\", \"x_best\": [",
               b, r.niter[b], bits(gamma[b]), (int)r.status[b], r.x_best[b].has_value() ? 1 : 0, last[b].min_idx,
               bits(last[b].min_val));
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
    int64_t head[5];
    double tol;
    if (fread(head, sizeof(int64_t), 5, f) != 5 || fread(&tol, sizeof tol, 1, f) != 1) return 2;
    const size_t B = (size_t)head[0], m = (size_t)head[1], nfeat = (size_t)head[2], n = nfeat + 1;
    Arr data(B * m * nfeat);
    std::vector<int32_t> labels(B * m);
    if (fread(data.data(), sizeof(double), data.size(), f) != data.size()) return 2;
    if (fread(labels.data(), sizeof(int32_t), labels.size(), f) != labels.size()) return 2;
    fclose(f);
    BatchSvmHip problems = BatchSvmHip::streamed(B, m, nfeat, data, false, labels);
    return head[4] ? run<EllStableBatchStreamedHip>(problems, B, n, (size_t)head[3], tol)
                   : run<EllBatchStreamedHip>(problems, B, n, (size_t)head[3], tol);
}
