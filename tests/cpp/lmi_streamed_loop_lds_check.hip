// lmi_streamed_loop_lds_check.hip -- host-only: the LDS need of k_batch_streamed_loop<BatchLmiOracle>
// (csrc/batch_streamed_loop_kernels.hpp) and of k_batch_streamed_loop_stable<BatchLmiOracle>
// (csrc/batch_streamed_stable_loop_kernels.hpp), from the very functions the host drivers size their launches with, at every
// n the streamed engine takes and every largest block size M.  It launches nothing and makes no HIP call, so it needs no
// device.  It checks both needs against the closed formulas of include/ellhip_batch_lmi_streamed.h, that they grow with n and
// with M and stay within the 159 KiB the drivers refuse beyond, that the wide oracle call stays within 64 KiB, and prints the
// needs at n = 1024, M = 64.
#include <cstdio>

#include "batch_lmi_kernels.hpp"
#include "batch_streamed_loop_kernels.hpp"
#include "batch_streamed_stable_loop_kernels.hpp"

int main() {
    using namespace ellhip;
    size_t last_ell = 0, last_stable = 0, last_assess = 0;
    for (int M = 1; M <= BATCH_LMI_MMAX; ++M) {
        BatchLmiOracle::Args A{};
        A.L.mmax = M;
        A.L.pm = M | 1;
        size_t prev_ell = 0, prev_stable = 0;
        for (int n = 1; n <= BATCH_STREAMED_NMAX; ++n) {
            const size_t e = ((size_t)n + 1) & ~(size_t)1;  // n rounded up to even
            const size_t oracle = (2 * (size_t)n + (size_t)M * (M | 1) + M + 16) | 1;
            const size_t ell = batch_streamed_loop_lds_doubles<BatchLmiOracle>(A, n);
            const size_t stable = batch_streamed_stable_loop_lds_doubles<BatchLmiOracle>(A, n);
            const size_t assess = batch_lmi_lds_doubles(n, M) + (size_t)n;
            if (ell != 5 * e + 8 + oracle || stable != 4 * e + 72 + oracle || oracle != batch_lmi_lds_doubles(n, M)) {
                printf("n = %d, M = %d: %zu and %zu doubles, expected %zu and %zu\n", n, M, ell, stable, 5 * e + 8 + oracle,
                       4 * e + 72 + oracle);
                return 1;
            }
            if (ell <= prev_ell || stable <= prev_stable || ell * sizeof(double) > 159 * 1024 ||
                stable * sizeof(double) > 159 * 1024 || assess * sizeof(double) > 64 * 1024) {
                printf("n = %d, M = %d: %zu, %zu and %zu bytes\n", n, M, ell * sizeof(double), stable * sizeof(double),
                       assess * sizeof(double));
                return 1;
            }
            // the oracle's scalars lie inside its block, 16 of them before the block's end
            if (BatchLmiOracle::lds_doubles(A, n) < 2 * (size_t)n + (size_t)M * A.L.pm + M + 16) return 1;
            prev_ell = ell;
            prev_stable = stable;
            last_assess = assess;
        }
        if (prev_ell <= last_ell || prev_stable <= last_stable) return 1;
        last_ell = prev_ell;
        last_stable = prev_stable;
    }
    printf("bytes at n = %d, M = %d: %zu (Ell) %zu (EllStable) %zu (assess)\nlmi_streamed_loop_lds_check: ok\n",
           BATCH_STREAMED_NMAX, BATCH_LMI_MMAX, last_ell * sizeof(double), last_stable * sizeof(double),
           last_assess * sizeof(double));
    return 0;
}
