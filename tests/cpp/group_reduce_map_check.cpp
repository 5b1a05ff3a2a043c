// group_reduce_map_check.cpp -- host test (built with g++ by tests/test_group_reduce_map.py): walks group_reduce_slot
// (csrc/group_reduce_map.hpp, the function k_group_reduce_p calls) over whole grids in launch order (x fastest, then y) and checks
// that the (blk, p) it hands out are exactly the grid, each once, and -- heavy first -- never go back to a heavier column block.
// Prints one JSON line per grid.
#include <cstdio>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/group_reduce_map.hpp"

static bool walk(bool heavy_first, unsigned gx, unsigned gy) {
    std::vector<int> seen((size_t)gx * gy, 0);
    long long outside = 0, back = 0, last_blk = -1, last_p = -1;
    bool pairs_in_order = true;
    for (unsigned by = 0; by < gy; ++by)
        for (unsigned bx = 0; bx < gx; ++bx) {
            long long blk = -1, p = -1;
            ellhip::group_reduce_slot(heavy_first, bx, by, gx, gy, blk, p);
            if (blk < 0 || blk >= gx || p < 0 || p >= gy) {
                ++outside;
                continue;
            }
            ++seen[(size_t)p * gx + blk];
            if (heavy_first && blk < last_blk) ++back;
            if (heavy_first && blk == last_blk && p != last_p + 1) pairs_in_order = false;
            last_blk = blk;
            last_p = p;
        }
    long long missed = 0, twice = 0;
    for (int c : seen) {
        missed += c == 0;
        twice += c > 1;
    }
    const bool ok = outside == 0 && missed == 0 && twice == 0 && back == 0 && pairs_in_order;
    printf("{\"heavy_first\": %s, \"gx\": %u, \"gy\": %u, \"outside\": %lld, \"missed\": %lld, \"twice\": %lld, \"went_back\": %lld, "
           "\"ok\": %s}\n", heavy_first ? "true" : "false", gx, gy, outside, missed, twice, back, ok ? "true" : "false");
    return ok;
}

int main() {
    bool ok = true;
    // column blocks of n = 128 .. 32768 (and odd counts), pairs of groups of 1 .. 32
    const unsigned gxs[] = {1, 2, 3, 33, 65, 128, 256};
    const unsigned gys[] = {1, 2, 7, 8, 15, 16};
    for (unsigned gx : gxs)
        for (unsigned gy : gys)
            for (int hf = 0; hf < 2; ++hf) ok &= walk(hf != 0, gx, gy);
    return ok ? 0 : 1;
}
