// batch_svm_runner.cpp -- one small sweep of SVM problems through the C++ mirror of the batched device loop
// (host/ellhip/batch_svm_hip.hpp) on Ell::new_with_scalar(100, 0) with gamma = +inf.  The problems come from a file the
// test writes: int64 B, m, nfeat, max_iters; double tol; double data[B][m][nfeat]; int32 labels[B][m].  Prints one JSON
// object per problem; doubles are printed as their bit patterns.
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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[4];
    double tol;
    if (fread(head, sizeof(int64_t), 4, f) != 4 || fread(&tol, sizeof tol, 1, f) != 1) return 2;
    const size_t B = (size_t)head[0], m = (size_t)head[1], nfeat = (size_t)head[2], n = nfeat + 1;
    Arr data(B * m * nfeat);
    std::vector<int32_t> labels(B * m);
    if (fread(data.data(), sizeof(double), data.size(), f) != data.size()) return 2;
    if (fread(labels.data(), sizeof(int32_t), labels.size(), f) != labels.size()) return 2;
    fclose(f);
    BatchSvmHip problems(B, m, nfeat, data, false, labels);
    EllBatchHip spaces = EllBatchHip::new_with_scalar(Arr(B, 100.0), std::vector<Arr>(B, Arr(n, 0.0)));
    Arr gamma(B, INFINITY);
    const BatchSvmResult r = problems.optim(spaces, gamma, Options((size_t)head[3], tol));
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
