// streamed_stable_loop_lds_check.hip -- host-only: the LDS need of k_batch_streamed_loop_stable<BatchLpOracle>
// (csrc/batch_streamed_stable_loop_kernels.hpp), from the very function the host driver sizes its launches with, at every
// n the streamed engine takes.  It launches nothing and makes no HIP call, so it needs no device.  It checks that the need
// is the sum of its three parts, grows with n and stays within the 64 KiB a launch may ask for without an opt-in, and prints
// the need at n = 1024.
#include <cstdio>

#include "batch_lowpass_kernels.hpp"
#include "batch_streamed_stable_loop_kernels.hpp"

int main() {
    using namespace ellhip;
    BatchLpOracle::Args A{};
    size_t prev = 0;
    for (int n = 1; n <= BATCH_STREAMED_NMAX; ++n) {
        A.mdim = 15 * n;
        const size_t d = batch_streamed_stable_loop_lds_doubles<BatchLpOracle>(A, n);
        const size_t np = (size_t)batch_streamed_np(n);
        const size_t want = (3 * np + 72) + np + (((size_t)n + 20) | 1);
        if (d != want || d != batch_streamed_stable_lds_doubles(n) + np + batch_lowpass_lds_doubles(n)) {
            printf("n = %d: %zu doubles, expected %zu\n", n, d, want);
            return 1;
        }
        if (d <= prev || d * sizeof(double) > 64 * 1024) {
            printf("n = %d: %zu bytes (n - 1: %zu)\n", n, d * sizeof(double), prev * sizeof(double));
            return 1;
        }
        // the gradient vector and the oracle's block start on even doubles, past the engine's own arrays
        if ((batch_streamed_stable_lds_doubles(n) & 1) != 0 || ((batch_streamed_stable_lds_doubles(n) + np) & 1) != 0) return 1;
        prev = d;
    }
    printf("bytes at n = %d: %zu\nstreamed_stable_loop_lds_check: ok\n", BATCH_STREAMED_NMAX, prev * sizeof(double));
    return 0;
}
