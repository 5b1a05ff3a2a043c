// streamed_stable_layout_check.cpp -- the scratch-triangle map of the streamed EllStable engine
// (ellalgo-rs_amd/csrc/batch_streamed_stable_layout.hpp), on the CPU: for each n the map must send the strict lower
// triangle one-to-one onto the slots that U (strict upper) and D (diagonal) do not use, be its own inverse, and put the
// elements of one column side by side.  Built with AddressSanitizer + UBSan by tests/test_batch_streamed_stable_cpu.py:
// the marks live in an array of exactly n * n bytes, so a slot outside the buffer fails the run.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "batch_streamed_stable_layout.hpp"

static int check(int n) {
    std::vector<unsigned char> used((std::size_t)n * n, 0);
    std::size_t count = 0;
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j) {
            const std::size_t slot = ellhip::bss_scratch_slot(n, i, j);
            if (slot >= used.size()) return std::printf("n=%d: S[%d][%d] -> slot %zu outside the buffer\n", n, i, j, slot);
            const int r = (int)(slot / n), c = (int)(slot % n);
            if (r <= c) return std::printf("n=%d: S[%d][%d] -> [%d][%d], a slot of U or D\n", n, i, j, r, c);
            if (used[slot]) return std::printf("n=%d: slot [%d][%d] used twice\n", n, r, c);
            used[slot] = 1;
            count += 1;
            if (ellhip::bss_scratch_slot(n, r, c) != (std::size_t)i * n + j)
                return std::printf("n=%d: the map is not its own inverse at S[%d][%d]\n", n, i, j);
            if (i + 1 < n && ellhip::bss_scratch_slot(n, i + 1, j) + 1 != slot)
                return std::printf("n=%d: column %d is not contiguous at row %d\n", n, j, i);
        }
    if (count != (std::size_t)n * (n - 1) / 2) return std::printf("n=%d: %zu slots, not n (n-1) / 2\n", n, count);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c)
            if ((used[(std::size_t)r * n + c] != 0) != (r > c))
                return std::printf("n=%d: slot [%d][%d] %s\n", n, r, c, r > c ? "is never used" : "belongs to U or D");
    return 0;
}

int main() {
    for (int n : {1, 2, 3, 64, 65, 1000, 1024})
        if (check(n)) return EXIT_FAILURE;
    std::printf("streamed_stable_layout_check: ok\n");
    return EXIT_SUCCESS;
}
