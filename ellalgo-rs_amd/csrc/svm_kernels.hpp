// svm_kernels.hpp -- SvmOracle (src/oracles/svm_oracle.rs:4-58) evaluated on the device.
//
// One assess_optim takes, for each of m samples, margin_i = y_i * (dot(w, x_i) + b) with w = xc[0..nfeat),
// b = xc[nfeat], y_i = labels[i] as f64, and the argmin over i under the reference's scan: min_val starts at
// +inf, min_idx at 0, and i replaces the minimum only when margin_i < min_val (ascending i).  So ties go to the
// first index, the winner keeps its own value (-0.0 vs +0.0 included), and NaN or +inf margins never win.
//
// Layout: the table is stored feature-major, XT[j * ld + i] = data[i][j], ld = m rounded up to SVM_LD_ALIGN.
// Each lane owns two adjacent samples and reads them with one 16-byte load per feature, so a wave's loads for
// one feature cover one contiguous 1 KiB segment.  Each lane folds its samples' products left to right from
// -0.0, exactly as Arr::dot (src/arr.rs:443-451: `.map(|(a, b)| a * b).sum()`, and current Rust starts that
// sum at -0.0; the start only decides the sign of a dot product that is an exact zero).  The build passes
// -ffp-contract=off, so every product is rounded before it is added.  The margins are therefore the
// reference's to the bit, and since the argmin rule does not depend on the visiting order, so are the chosen
// index, the gradient and the cut value.
//
// Reduction: each workgroup reduces its lanes' (value, index) pairs with a fixed butterfly and one LDS step and
// writes one partial; k_svm_final (one workgroup) reduces the partials and builds the cut.  No persistent grids,
// no waits between workgroups.  Both return at once when the device loop's `halted` word is set.
#pragma once

#include "ell_kernels.hpp"

namespace ellhip {

constexpr int SVM_THREADS = 256;
constexpr int SVM_SPL = 2;                                // samples per lane (one double2 per feature)
constexpr int SVM_SPW = SVM_THREADS * SVM_SPL;            // samples per workgroup
constexpr int SVM_UNROLL = 8;                             // features whose loads are in flight per lane
constexpr long long SVM_LD_ALIGN = 8;                     // ld in doubles: 64-byte aligned feature rows
constexpr long long SVM_NONE = 0x7fffffffffffffffLL;      // partial index: no sample below +inf

struct SvmParams {
    long long m, nfeat, ld;
};

// What the last scan found (the reference's locals min_val / min_idx) and the loop's outputs.
struct SvmState {
    long long min_idx;
    double min_val;
    double gamma;   // *gamma after the last assess_optim
    int has_best;   // device loop: x_best is Some
    int pad;
};

struct SvmPartial {
    double v;
    long long i;
};

// (va, ia) <- the better of the two under the reference's rule: a strictly smaller value wins, an equal one
// (==, so -0.0 ties +0.0) goes to the smaller index.  Partials only ever hold values that passed `<` against
// +inf, so NaN never reaches this.
__device__ __forceinline__ void svm_pick(double& va, long long& ia, double vb, long long ib) {
    if (vb < va || (vb == va && ib < ia)) {
        va = vb;
        ia = ib;
    }
}

// all threads of the workgroup call it; thread 0 gets the result
__device__ __forceinline__ void svm_block_argmin(double& v, long long& idx) {
    __shared__ double sv[SVM_THREADS / 64];
    __shared__ long long si[SVM_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const long long oi = __shfl_xor(idx, off, 64);
        svm_pick(v, idx, ov, oi);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sv[wave] = v;
        si[wave] = idx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SVM_THREADS / 64; ++w) svm_pick(v, idx, sv[w], si[w]);
    }
}

// Tiled transpose of one slab of the caller's row-major table (rows [r0, r0 + rows), nfeat columns) into XT.
constexpr int SVM_TILE = 32;
__global__ __launch_bounds__(256) void k_svm_transpose(const double* __restrict__ slab, long long rows, long long r0,
                                                       SvmParams P, double* __restrict__ XT) {
    __shared__ double tile[SVM_TILE][SVM_TILE + 1];
    const long long tcols = (P.nfeat + SVM_TILE - 1) / SVM_TILE;
    const long long trows = (rows + SVM_TILE - 1) / SVM_TILE;
    const int tx = threadIdx.x & (SVM_TILE - 1), ty = threadIdx.x / SVM_TILE;  // 32 x 8
    for (long long t = blockIdx.x; t < tcols * trows; t += gridDim.x) {
        const long long rb = (t / tcols) * SVM_TILE, cb = (t % tcols) * SVM_TILE;
        for (int k = ty; k < SVM_TILE; k += 256 / SVM_TILE) {
            const long long r = rb + k, c = cb + tx;
            if (r < rows && c < P.nfeat) tile[k][tx] = slab[r * P.nfeat + c];
        }
        __syncthreads();
        for (int k = ty; k < SVM_TILE; k += 256 / SVM_TILE) {
            const long long c = cb + k, r = rb + tx;
            if (r < rows && c < P.nfeat) XT[c * P.ld + r0 + r] = tile[tx][k];
        }
        __syncthreads();
    }
}

// Margins of samples [2 l, 2 l + 2) for lane l, then the workgroup's argmin as one partial.  `margins`
// (optional) receives all m margins.  NT: non-temporal loads for tables larger than the Infinity Cache share
// (same rule as the Q stream), plain loads for tables that stay cached from one call to the next.
template <bool NT>
__global__ __launch_bounds__(SVM_THREADS) void k_svm_margins(const double* __restrict__ XT, const int* __restrict__ labels,
                                                             SvmParams P, const double* __restrict__ x,
                                                             double* __restrict__ margins, SvmPartial* __restrict__ part,
                                                             const int* __restrict__ halted) {
    if (*halted) return;
    const long long i0 = ((long long)blockIdx.x * SVM_THREADS + threadIdx.x) * SVM_SPL;
    double best = __builtin_inf();
    long long bidx = SVM_NONE;
    if (i0 < P.m) {
        const double* col = XT + i0;
        double a0 = -0.0, a1 = -0.0;
        long long j = 0;
        for (; j + SVM_UNROLL <= P.nfeat; j += SVM_UNROLL) {
            double2_t v[SVM_UNROLL];
#pragma unroll
            for (int u = 0; u < SVM_UNROLL; ++u) v[u] = ld_stream<NT, double2_t>(col + (j + u) * P.ld);
#pragma unroll
            for (int u = 0; u < SVM_UNROLL; ++u) {
                const double wj = x[j + u];
                a0 = a0 + wj * v[u].x;
                a1 = a1 + wj * v[u].y;
            }
        }
        for (; j < P.nfeat; ++j) {
            const double2_t v = ld_stream<NT, double2_t>(col + j * P.ld);
            const double wj = x[j];
            a0 = a0 + wj * v.x;
            a1 = a1 + wj * v.y;
        }
        const double b = x[P.nfeat];
        const double m0 = (double)labels[i0] * (a0 + b);
        if (margins) margins[i0] = m0;
        if (m0 < best) {
            best = m0;
            bidx = i0;
        }
        if (i0 + 1 < P.m) {
            const double m1 = (double)labels[i0 + 1] * (a1 + b);
            if (margins) margins[i0 + 1] = m1;
            if (m1 < best) {
                best = m1;
                bidx = i0 + 1;
            }
        }
    }
    svm_block_argmin(best, bidx);
    if (threadIdx.x == 0) part[blockIdx.x] = SvmPartial{best, bidx};
}

// One workgroup: the argmin over the partials (fixed order), then the cut (src/oracles/svm_oracle.rs:42-57):
//   min_val >= 1.0 (also: nothing below +inf)  ->  g = 0 (n = nfeat + 1), beta = 0.0, gamma = +0.0
//   otherwise                                  ->  g = [(-y) x_min,j ...] ++ [-y], beta = gamma = min_val
// The cut is central (`shrunk` is always true).  With `xbest` (device loop) it also plays the caller of
// src/cutting_plane.rs:300-303: x_best = Some(xc).
__global__ __launch_bounds__(SVM_THREADS) void k_svm_final(const double* __restrict__ XT, const int* __restrict__ labels,
                                                           SvmParams P, const SvmPartial* __restrict__ part, long long nparts,
                                                           const double* __restrict__ x, SvmState* __restrict__ ss,
                                                           double* __restrict__ g, CutParams* __restrict__ cp,
                                                           double* __restrict__ xbest, const int* __restrict__ halted) {
    if (*halted) return;
    __shared__ long long sh_idx;
    __shared__ double sh_y;
    double v = __builtin_inf();
    long long idx = SVM_NONE;
    for (long long p = threadIdx.x; p < nparts; p += SVM_THREADS) svm_pick(v, idx, part[p].v, part[p].i);
    svm_block_argmin(v, idx);
    if (threadIdx.x == 0) {
        const long long min_idx = idx == SVM_NONE ? 0 : idx;
        const double min_val = v;
        ss->min_idx = min_idx;
        ss->min_val = min_val;
        CutParams c;
        c.kind = 1;  // update_central_cut (src/cutting_plane.rs:304)
        c.has_b1 = 0;
        c.b1 = 0.0;
        if (min_val >= 1.0) {  // :42-45
            c.b0 = 0.0;
            ss->gamma = 0.0;
            sh_idx = -1;
        } else {               // :47-57
            c.b0 = min_val;
            ss->gamma = min_val;
            sh_idx = min_idx;
            sh_y = (double)labels[min_idx];
        }
        if (xbest) ss->has_best = 1;
        *cp = c;
    }
    __syncthreads();
    const long long row = sh_idx;
    if (row < 0) {
        for (long long j = threadIdx.x; j <= P.nfeat; j += SVM_THREADS) g[j] = 0.0;
    } else {
        const double ny = -sh_y;
        for (long long j = threadIdx.x; j < P.nfeat; j += SVM_THREADS) g[j] = ny * XT[j * P.ld + row];
        if (threadIdx.x == 0) g[P.nfeat] = ny;
    }
    if (xbest)
        for (long long j = threadIdx.x; j <= P.nfeat; j += SVM_THREADS) xbest[j] = x[j];
}

}  // namespace ellhip
