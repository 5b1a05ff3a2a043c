// group_reduce_map.hpp -- which (column block, pair of cuts) a workgroup of k_group_reduce_p takes.  Plain C++ (no HIP header), so
// that a host program can walk the same function (tests/cpp/group_reduce_map_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define ELLHIP_MAP_HD __host__ __device__
#else
#define ELLHIP_MAP_HD
#endif

namespace ellhip {

// Column block `blk` (128 columns) of the lower triangle has nstrips - 2 blk (- 1) strips of column sums to add: block 0 is the
// heaviest and the last one the lightest.  Workgroups start in the order x fastest, then y.
//   heavy_first = false   blk = x, p = y: every pair runs heavy to light by itself, so every pair ends in a run of two-strip
//                         workgroups and the card drains grid.y times per launch
//   heavy_first = true    the launch as a whole goes heavy to light: all pairs of block 0, then all pairs of block 1, ...
// Either way every (blk, p) of the grid is taken exactly once, and the output addressing (by blk and p) does not change.
ELLHIP_MAP_HD inline void group_reduce_slot(bool heavy_first, unsigned bx, unsigned by, unsigned gx, unsigned gy, long long& blk,
                                            long long& p) {
    if (!heavy_first) {
        blk = bx;
        p = by;
        return;
    }
    const unsigned long long lin = (unsigned long long)by * gx + bx;
    blk = (long long)(lin / gy);
    p = (long long)(lin % gy);
}

}  // namespace ellhip
