// maxcut_loop_lds_check.hip -- host-only: the LDS need of the four loop instantiations that take BatchMaxcutOracle
// (csrc/batch_maxcut_kernels.hpp) -- k_batch_loop<T, false, .>, k_batch_loop<T, true, .> (csrc/batch_loop_kernels.hpp),
// k_batch_streamed_loop<.> and k_batch_streamed_loop_stable<.> -- from the very functions the host driver sizes its launches
// with (batch_loop_run, csrc/batch_loop_capi.inc.hpp), at every n each engine takes.  It launches nothing and makes no HIP
// call, so it needs no device.  It checks the needs against the closed formulas of include/ellhip_batch_maxcut.h and the
// 159 KiB the driver refuses beyond, walks the chain's term-to-pair map (batch_maxcut_row_of) over every term of every n,
// and prints the needs at n = 128 and n = 1024.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "batch_maxcut_kernels.hpp"
#include "batch_streamed_loop_kernels.hpp"
#include "batch_streamed_stable_loop_kernels.hpp"

// instances per workgroup of the LDS engine's loop: batch_row_shape (csrc/batch_loop_capi.inc.hpp), which is also how the
// batch engine shapes an Ell handle at its default thread count
static int row_epw(int n, size_t space_doubles) {
    const int T = n <= 64 ? 256 : 128;
    int epw = std::min(64, T / n);
    while (epw > 1 && (size_t)epw * space_doubles * sizeof(double) > 64 * 1024) epw -= 1;
    return epw;
}

int main() {
    using namespace ellhip;
    BatchMaxcutOracle::Args A{};
    const size_t LDS_MAX = 159 * 1024;
    size_t lds_ell = 0, lds_stable = 0, str_ell = 0, str_stable = 0;
    for (int n = 1; n <= BATCH_STREAMED_NMAX; ++n) {
        const size_t e = ((size_t)n + 1) & ~(size_t)1;  // n rounded up to even
        const size_t p = (size_t)n | 1;
        const size_t oracle = (3 * (size_t)n + 8) | 1;
        if (oracle != BatchMaxcutOracle::lds_doubles(A, n) || BatchMaxcutOracle::scalars_at(A, n) != 3 * (size_t)n ||
            oracle < 3 * (size_t)n + BATCH_MAXCUT_SCALARS) {
            printf("n = %d: the oracle's block is %zu doubles, expected %zu\n", n, BatchMaxcutOracle::lds_doubles(A, n), oracle);
            return 1;
        }
        str_ell = batch_streamed_loop_lds_doubles<BatchMaxcutOracle>(A, n) * sizeof(double);
        str_stable = batch_streamed_stable_loop_lds_doubles<BatchMaxcutOracle>(A, n) * sizeof(double);
        if (str_ell != 8 * (5 * e + 8 + oracle) || str_stable != 8 * (4 * e + 72 + oracle) || str_ell > LDS_MAX ||
            str_stable > LDS_MAX) {
            printf("n = %d: streamed %zu and %zu bytes\n", n, str_ell, str_stable);
            return 1;
        }
        if (n <= BATCH_NMAX) {
            const size_t se = batch_space_lds_doubles<false>(n), ss = batch_space_lds_doubles<true>(n);
            lds_ell = (size_t)row_epw(n, se) * (se + oracle) * sizeof(double);
            lds_stable = (size_t)row_epw(n, ss) * (ss + oracle) * sizeof(double);
            if (se != ((n * p + 2 * n + 8) | 1) || ss != ((n * p + 3 * n + 8) | 1) || lds_ell > LDS_MAX || lds_stable > LDS_MAX) {
                printf("n = %d: LDS engines %zu and %zu bytes\n", n, lds_ell, lds_stable);
                return 1;
            }
            if (n == BATCH_NMAX) printf("bytes at n = %d: %zu (Ell) %zu (EllStable)\n", n, lds_ell, lds_stable);
        }
        // every term of the chain: the pair the closed form gives is the pair a walk over the upper triangle gives
        int k = 0;
        for (int i = 0; i < n; ++i) {
            if (batch_maxcut_row_start(n, i) != k) {
                printf("n = %d: row %d starts at %d, not %d\n", n, i, k, batch_maxcut_row_start(n, i));
                return 1;
            }
            for (int j = i + 1; j < n; ++j, ++k) {
                const int ri = batch_maxcut_row_of(n, k);
                const double root = std::sqrt((double)((2 * n - 1) * (2 * n - 1) - 8 * k));  // and a root 1e-12 off either way
                if (batch_maxcut_row_from(n, k, root * (1.0 + 1e-12)) != i || batch_maxcut_row_from(n, k, root * (1.0 - 1e-12)) != i ||
                    ri != i || k - batch_maxcut_row_start(n, ri) + ri + 1 != j) {
                    printf("n = %d: term %d is (%d, %d), not row %d\n", n, k, i, j, ri);
                    return 1;
                }
            }
        }
        if (k != batch_maxcut_terms(n)) return 1;
    }
    printf("bytes at n = %d: %zu (Ell) %zu (EllStable)\nmaxcut_loop_lds_check: ok\n", BATCH_STREAMED_NMAX, str_ell, str_stable);
    return 0;
}
