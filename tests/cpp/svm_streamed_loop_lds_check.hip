// svm_streamed_loop_lds_check.hip -- host-only: the LDS need of k_batch_streamed_loop<BatchSvmOracle>
// (csrc/batch_streamed_loop_kernels.hpp) and of k_batch_streamed_loop_stable<BatchSvmOracle>
// (csrc/batch_streamed_stable_loop_kernels.hpp), from the very functions the host drivers size their launches with, at every
// n the streamed engine takes.  It launches nothing and makes no HIP call, so it needs no device.  It checks both needs against
// the closed formulas of include/ellhip_batch_svm_streamed.h, that they grow with n and stay within the 64 KiB the drivers
// refuse beyond, and prints the needs at n = 1024.
#include <cstdio>

#include "batch_svm_kernels.hpp"
#include "batch_streamed_loop_kernels.hpp"
#include "batch_streamed_stable_loop_kernels.hpp"

int main() {
    using namespace ellhip;
    BatchSvmOracle::Args A{};
    size_t prev_ell = 0, prev_stable = 0;
    for (int n = 1; n <= BATCH_STREAMED_NMAX; ++n) {
        const size_t e = ((size_t)n + 1) & ~(size_t)1;  // n rounded up to even
        const size_t oracle = ((size_t)n + 10) | 1;
        const size_t ell = batch_streamed_loop_lds_doubles<BatchSvmOracle>(A, n);
        const size_t stable = batch_streamed_stable_loop_lds_doubles<BatchSvmOracle>(A, n);
        if (ell != 5 * e + 8 + oracle || stable != 4 * e + 72 + oracle || oracle != batch_svm_lds_doubles(n)) {
            printf("n = %d: %zu and %zu doubles, expected %zu and %zu\n", n, ell, stable, 5 * e + 8 + oracle, 4 * e + 72 + oracle);
            return 1;
        }
        if (ell <= prev_ell || stable <= prev_stable || ell * sizeof(double) > 64 * 1024 || stable * sizeof(double) > 64 * 1024) {
            printf("n = %d: %zu and %zu bytes\n", n, ell * sizeof(double), stable * sizeof(double));
            return 1;
        }
        // the oracle's block starts on an even double, past the engine's own arrays
        if ((batch_streamed_lds_doubles(n) & 1) != 0 || ((batch_streamed_stable_lds_doubles(n) + e) & 1) != 0) return 1;
        prev_ell = ell;
        prev_stable = stable;
    }
    printf("bytes at n = %d: %zu (Ell) %zu (EllStable)\nsvm_streamed_loop_lds_check: ok\n", BATCH_STREAMED_NMAX,
           prev_ell * sizeof(double), prev_stable * sizeof(double));
    return 0;
}
