// batch_streamed_stable_layout.hpp -- where the streamed EllStable engine keeps the scratch triangle
// (batch_streamed_stable_kernels.hpp).  No HIP includes: tests/cpp/streamed_stable_layout_check.cpp
// builds this header alone on the CPU.
//
// The reference packs an EllStable into one n x n buffer: diagonal = D, strict upper = the factor U (mq.at(j, i) = L[i][j]),
// strict lower = scratch, row-major: S[i][j], i > j, at [i][j] (src/ell_stable.rs:61-69).  The engine walks the scratch
// triangle three times per cut, each time with j fixed and i moving (across lanes, or along one lane's chain), which in the
// reference's position is a stride of n doubles.  So inside a streamed handle S[i][j] lives at [n-1-j][n-1-i]: the upper
// triangle's position (j, i) turned by 180 degrees.  That slot is in the strict lower triangle again (n-1-j > n-1-i), the
// map is one-to-one and its own inverse, and for a fixed j the slots of i = j+1 .. n-1 are n-1-j consecutive doubles at
// the start of row n-1-j.  D and U keep the reference's positions.
#pragma once

#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ELLHIP_LAYOUT_HD __host__ __device__
#else
#define ELLHIP_LAYOUT_HD
#endif

namespace ellhip {

// offset, inside one ellipsoid's n x n buffer, of the reference's scratch element S[i][j] (0 <= j < i < n)
ELLHIP_LAYOUT_HD inline std::size_t bss_scratch_slot(int n, int i, int j) {
    return (std::size_t)(n - 1 - j) * (std::size_t)n + (std::size_t)(n - 1 - i);
}

}  // namespace ellhip
