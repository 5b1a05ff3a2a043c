// batch_maxcut_kernels.hpp -- the oracle of B independent MaxcutOracle problems of one size n, as a policy of the loop
// kernels (include/ellhip_batch_maxcut.h; the loops: batch_loop_kernels.hpp,
// batch_streamed_loop_kernels.hpp, batch_streamed_stable_loop_kernels.hpp).
//
// One round is
//     oracle (MaxcutOracle::assess_optim, src/oracles/maxcut_oracle.rs:21-49)
//  -> improved: x_best = xc and a central cut; otherwise a deep cut with beta = gamma (src/cutting_plane.rs:300-307)
// The oracle's arithmetic is `+`, one `* 2.0`, negation and comparisons, and both of its folds keep the reference's order,
// so the cut, gamma and with them the whole loop are bit-identical to cutting_plane_optim over MaxcutOracle on the CPU.
//
// Layout.  W[t][n][n] is the caller's row-major table and WT[t][n][n] its transpose (t = 0 for a table shared by all
// problems, t = b otherwise), made on the device at create.  When every table is symmetric to the bit the handle keeps ONE
// copy and WT == W: w[i][j] and w[j][i] are then the same bits, and the kernels never ask which of the two layouts they
// run on.
//
// cut_value (:24-31) is one left fold over the upper triangle in row-major order: term k = 0 .. L-1, L = n (n-1) / 2, is
// w[i][j] of the k-th pair i < j.  It is a single chain of L dependent adds and is never re-associated.  Thread 0 of the
// instance (the chain lane) does nothing but those adds: the n threads stage n terms at a time through LDS -- thread t takes
// term s n + t of step s, finds its pair (i, j) in closed form, loads w[i][j] from the row-major copy (consecutive k are
// consecutive addresses inside a row) and stores it MASKED, the value where x[i] != x[j] and +0.0 elsewhere -- into one
// half of a double buffer, while the chain lane folds the other half; one barrier per step, ceil(L / n) steps.  The loads of
// step s + 1 are issued before the chain of step s and consumed after it, so the chain lane's wave meets its global loads
// only when they have had a whole step to land, and the chain itself reads LDS only, one group of eight values ahead of the
// group it adds.
// Adding a skipped term as +0.0 changes no bit: a fold that starts at +0.0 never reaches -0.0 (x + y is -0.0 only when both
// are, and exact cancellation rounds to +0.0), so s + (+0.0) has the bits of s for every reachable s, NaN and infinities
// included.  The gradient's masked adds below rest on the same fact.
//
// Gradient (:33-41).  Thread i owns row i and folds w[i][j] over j = 0 .. n-1 in ascending order where x[i] != x[j] (the
// diagonal never passes), reading WT[j][i]: at step j the n threads of an instance read n consecutive doubles.  The folds
// ride on the chain's steps, two columns a step (ceil(L / n) is (n - 1) / 2 rounded up), and what is left is finished after
// the last step.  Then grad[i] * 2.0 and the negation, so a zero sum is handed out as -0.0.  The signs are read from an LDS
// copy.
//
// Barriers are workgroup-wide; threads that take no part (live = false: a stopped or absent instance, a thread i >= n of a
// padded block) skip the loads and stores and take part in every barrier.  Every loop is bounded by n; no thread waits on
// another workgroup or on a memory word; there is no atomic here.  Index arithmetic is 64-bit.
//
// Nothing is tied to the number of instances in a workgroup or to n <= 128: k_batch_loop<T, STABLE, BatchMaxcutOracle> runs
// n threads per instance with epw instances per workgroup, k_batch_streamed_loop<BatchMaxcutOracle> and
// k_batch_streamed_loop_stable<BatchMaxcutOracle> one instance per workgroup of n rounded up to 64 threads, n <= 1024.
// Resources (gfx950, no scratch anywhere): see the table in include/ellhip_batch_maxcut.h.
#pragma once

#include "batch_loop_kernels.hpp"

namespace ellhip {

// oracle scalars (LDS, per instance), after the loop's own (batch_loop_kernels.hpp)
enum : int {
    MC_GAMMA = BL_GAMMA,  // the loop's gamma
    MC_B0 = 5,        // the cut's beta: -cut_value when improved, gamma otherwise
    MC_SHRUNK = 6,    // 1.0: improved
    MC_CUT = 7,       // the last cut_value
    BATCH_MAXCUT_SCALARS = 8,
};
static_assert(MC_B0 == BL_SCALARS, "the oracle's scalars follow the loop's");

// doubles of LDS the oracle needs per instance: the signs, the chain's double buffer and the scalars
__host__ __device__ inline size_t batch_maxcut_lds_doubles(int n) { return (3 * (size_t)n + BATCH_MAXCUT_SCALARS) | 1; }

// terms of the chain: pairs i < j
__host__ __device__ inline int batch_maxcut_terms(int n) { return n * (n - 1) / 2; }

// first term of row i: rows 0 .. i-1 hold n-1, n-2, .. terms
__host__ __device__ inline int batch_maxcut_row_start(int n, int i) { return i * (2 * n - 1 - i) / 2; }

// the row of term k, 0 <= k < n (n-1) / 2, n <= 1024, from `root`, an estimate of sqrt((2n-1)^2 - 8k): the closed form and
// one step either way, so any estimate that puts the closed form within a row of the answer will do -- a correctly rounded
// root or one a few ulp off (tests/cpp/maxcut_loop_lds_check.hip walks every k of every n with both)
__host__ __device__ inline int batch_maxcut_row_from(int n, int k, double root) {
    int i = (int)(((double)(2 * n - 1) - root) * 0.5);
    if (i > n - 2) i = n - 2;
    if (i < 0) i = 0;
    if (batch_maxcut_row_start(n, i) > k) i -= 1;
    else if (batch_maxcut_row_start(n, i + 1) <= k) i += 1;
    return i;
}
__host__ __device__ inline int batch_maxcut_row_of(int n, int k) {
    const int d = 2 * n - 1;
    return batch_maxcut_row_from(n, k, sqrt((double)(d * d - 8 * k)));
}

constexpr int BATCH_MAXCUT_UNROLL = 8;  // values in a group of LDS reads the chain lane has in flight ahead of its adds

// One assess_optim for the workgroup's instances, collectively (it contains barriers: every thread of the workgroup calls
// it).  live: this thread belongs to an instance that takes part.  w / wt: the instance's table and its transpose (the same
// pointer for a handle that keeps one copy).  xci: this thread's coordinate of the point.  sx: the instance's signs (LDS,
// n), buf: its double buffer (LDS, 2 n).  osc[MC_GAMMA] holds gamma.  On return (after a barrier) gout is the gradient,
// osc[MC_B0] beta, osc[MC_SHRUNK] whether gamma improved, osc[MC_GAMMA] the new gamma and osc[MC_CUT] the cut value.
__device__ __forceinline__ void batch_maxcut_oracle(const bool live, const int i, const int n,
                                                    const double* w, const double* wt, const double xci, double* sx,
                                                    double* buf, double* osc, double* gout) {
    const int L = batch_maxcut_terms(n);
    const int steps = (L + n - 1) / n;
    if (live) sx[i] = xci >= 0.0 ? 1.0 : -1.0;  // -0.0 -> +1, NaN -> -1                            maxcut_oracle.rs:22
    __syncthreads();
    const double si = live ? sx[i] : 1.0;
    // this thread's term of a step: the value, masked
    auto term = [&](const int k, bool& differ) -> double {
        differ = false;
        if (!live || k >= L) return 0.0;
        const int ri = batch_maxcut_row_of(n, k);
        const int rj = k - batch_maxcut_row_start(n, ri) + ri + 1;
        differ = sx[ri] != sx[rj];
        return w[(long long)ri * n + rj];
    };
    {
        bool differ;
        const double v = term(i, differ);
        if (live) buf[i] = differ ? v : 0.0;
    }
    __syncthreads();
    double cv = 0.0;  // the chain lane's                                                            :24
    double gs = 0.0;  // grad[i]                                                                     :33
    for (int s = 0; s < steps; ++s) {
        const double* cur = buf + (size_t)(s & 1) * n;
        double* nxt = buf + (size_t)((s + 1) & 1) * n;
        // the loads of the next step's term and of this step's two gradient columns, issued before the chain
        bool differ = false;
        const double v = s + 1 < steps ? term((s + 1) * n + i, differ) : 0.0;
        const int j0 = 2 * s, j1 = 2 * s + 1;  // j1 <= n - 1: 2 steps <= n
        double a0 = 0.0, a1 = 0.0;
        bool d0 = false, d1 = false;
        if (live) {
            d0 = si != sx[j0];
            d1 = si != sx[j1];
            a0 = wt[(long long)j0 * n + i];
            a1 = wt[(long long)j1 * n + i];
        }
        if (live && i == 0) {  // the chain: terms s n .. of the fold, in order                      :25-31
            const int cnt = L - s * n < n ? L - s * n : n;
            int t = 0;
            if (cnt >= BATCH_MAXCUT_UNROLL) {
                // two groups of values in turn: one is read while the other is added, so the reads run ahead and the adds
                // stay in order.  Entering an iteration, ca holds the group at t.
                constexpr int U = BATCH_MAXCUT_UNROLL;
                double ca[U], cb[U];
#pragma unroll
                for (int u = 0; u < U; ++u) ca[u] = cur[u];
                for (; t + 3 * U <= cnt; t += 2 * U) {
#pragma unroll
                    for (int u = 0; u < U; ++u) cb[u] = cur[t + U + u];
#pragma unroll
                    for (int u = 0; u < U; ++u) cv = cv + ca[u];
#pragma unroll
                    for (int u = 0; u < U; ++u) ca[u] = cur[t + 2 * U + u];
#pragma unroll
                    for (int u = 0; u < U; ++u) cv = cv + cb[u];
                }
                const bool two = t + 2 * U <= cnt;
                if (two) {
#pragma unroll
                    for (int u = 0; u < U; ++u) cb[u] = cur[t + U + u];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) cv = cv + ca[u];
                if (two) {
#pragma unroll
                    for (int u = 0; u < U; ++u) cv = cv + cb[u];
                }
                t += two ? 2 * U : U;
            }
            for (; t < cnt; ++t) cv = cv + cur[t];
        }
        if (live) {
            if (s + 1 < steps) nxt[i] = differ ? v : 0.0;
            gs = gs + (d0 ? a0 : 0.0);  // a masked add: +0.0 where the signs agree                  :35-39
            gs = gs + (d1 ? a1 : 0.0);
        }
        __syncthreads();
    }
    if (live) {
        for (int j = 2 * steps; j < n; ++j) {  // n odd: one column left; n = 1: the diagonal alone
            const double a = wt[(long long)j * n + i];
            gs = gs + (si != sx[j] ? a : 0.0);
        }
        gout[i] = -(gs * 2.0);  //                                                                   :41, :45 / :47
        if (i == 0) {
            const double gamma = osc[MC_GAMMA];
            const bool improved = cv > gamma;  // strict; NaN is false                               :43
            osc[MC_CUT] = cv;
            osc[MC_SHRUNK] = improved ? 1.0 : 0.0;
            osc[MC_B0] = improved ? -cv : gamma;  //                                                 :45 / :47
            if (improved) osc[MC_GAMMA] = cv;  //                                                    :44
        }
    }
    __syncthreads();
}

// The oracle as the loop kernels' policy (batch_loop_kernels.hpp).  Per instance in HBM: the table and, unless every table
// is symmetric to the bit, its transpose.  The oracle keeps no state between calls other than gamma, which is the loop's.
struct BatchMaxcutOracle {
    struct Args {
        const double* W;       // [ntab][n][n] row-major
        const double* WT;      // [ntab][n][n] the transposes; == W when every table is symmetric to the bit
        long long tab_stride;  // n * n for per-problem tables, 0 for a shared one
    };
    struct Regs {
        const double* w;  // this instance's table and its transpose
        const double* wt;
    };
    static __host__ __device__ inline size_t lds_doubles(const Args&, int n) { return batch_maxcut_lds_doubles(n); }
    static __host__ __device__ __forceinline__ size_t scalars_at(const Args&, int n) { return 3 * (size_t)n; }
    static __device__ __forceinline__ void load(const Args& A, bool active, long long b, int i, int n, double* blk, Regs& r) {
        r.w = A.W + (active ? b : 0) * A.tab_stride;
        r.wt = A.WT + (active ? b : 0) * A.tab_stride;
        if (active && i == 0) {
            double* osc = blk + 3 * (size_t)n;
            osc[MC_B0] = 0.0;
            osc[MC_SHRUNK] = 0.0;
            osc[MC_CUT] = 0.0;
        }
    }
    static __device__ __forceinline__ void assess(const Args& A, const BatchLoopRun&, bool live, int i, int n, double xci,
                                                  double* blk, Regs& r, double* g) {
        batch_maxcut_oracle(live, i, n, r.w, r.wt, xci, blk, blk + n, blk + 3 * (size_t)n, g);
    }
    // improved: the centre is the best point so far and the cut is central (the beta is carried and ignored); otherwise a
    // deep cut with beta = gamma                                                     src/cutting_plane.rs:300-307
    static __device__ __forceinline__ BatchOutcome outcome(const Args&, int, const double* osc) {
        return BatchOutcome{osc[MC_SHRUNK] != 0.0 ? BOUT_SHRUNK : BOUT_CUT, osc[MC_B0], 0, 0.0};
    }
    static __device__ __forceinline__ void store(const Args&, long long, const double*, const Regs&) {}
};

// One assess_optim per instance at x[B][n] with gamma[B]: the same device function, without an ellipsoid.  Two launch
// shapes: epw instances packed into T = 128 or 256 threads (n <= 128), or the wide one past it -- epw = 1, one workgroup
// per instance, blockDim.x = n rounded up to 64 (T = 1024 only bounds the block); threads tid >= n belong to no instance
// (e = 1 >= epw), are inactive in the oracle and take part in its barriers.  LDS: epw * (batch_maxcut_lds_doubles(n) + n)
// doubles.  Every loop is bounded by n; no thread waits on another workgroup or on a memory word.
template <int T>
__global__ __launch_bounds__(T) void k_batch_maxcut_assess(long long B, int n, int epw, BatchMaxcutOracle::Args A,
                                                           const double* __restrict__ x, double* __restrict__ gamma,
                                                           double* __restrict__ grad_out, double* __restrict__ beta_out,
                                                           double* __restrict__ shrunk_out, double* __restrict__ cut_out) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * epw + e;
    const bool active = e < epw && b < B;
    const size_t lper = batch_maxcut_lds_doubles(n) + (size_t)n;
    double* blk = sm + (size_t)(e < epw ? e : 0) * lper;
    double* osc = blk + 3 * (size_t)n;
    double* g = osc + BATCH_MAXCUT_SCALARS;
    const double* w = A.W;
    const double* wt = A.WT;
    double xi = 0.0;
    if (active) {
        xi = x[b * n + i];
        w = A.W + b * A.tab_stride;
        wt = A.WT + b * A.tab_stride;
        if (i == 0) osc[MC_GAMMA] = gamma[b];
    }
    batch_maxcut_oracle(active, i, n, w, wt, xi, blk, blk + n, osc, g);
    if (active) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        gamma[b] = osc[MC_GAMMA];
        beta_out[b] = osc[MC_B0];
        shrunk_out[b] = osc[MC_SHRUNK];
        cut_out[b] = osc[MC_CUT];
    }
}

// Tiled transpose of the tables on the device: W is taken as one [rows][n] matrix of ntab * n rows, row r being row r % n of
// table r / n; WT[tab][c][s] = W[tab][s][c].  Grid-stride over the tiles, so the grid is bounded.
constexpr int BATCH_MAXCUT_TILE = 32;
__global__ __launch_bounds__(256) void k_batch_maxcut_transpose(const double* __restrict__ W, long long rows, long long n,
                                                                double* __restrict__ WT) {
    __shared__ double tile[BATCH_MAXCUT_TILE][BATCH_MAXCUT_TILE + 1];
    const long long tcols = (n + BATCH_MAXCUT_TILE - 1) / BATCH_MAXCUT_TILE;
    const long long trows = (rows + BATCH_MAXCUT_TILE - 1) / BATCH_MAXCUT_TILE;
    const int tx = threadIdx.x & (BATCH_MAXCUT_TILE - 1), ty = threadIdx.x / BATCH_MAXCUT_TILE;  // 32 x 8
    for (long long t = blockIdx.x; t < tcols * trows; t += gridDim.x) {
        const long long rb = (t / tcols) * BATCH_MAXCUT_TILE, cb = (t % tcols) * BATCH_MAXCUT_TILE;
        for (int k = ty; k < BATCH_MAXCUT_TILE; k += 256 / BATCH_MAXCUT_TILE) {
            const long long r = rb + k, c = cb + tx;
            if (r < rows && c < n) tile[k][tx] = W[r * n + c];
        }
        __syncthreads();
        for (int k = ty; k < BATCH_MAXCUT_TILE; k += 256 / BATCH_MAXCUT_TILE) {
            const long long c = cb + k, r = rb + tx;
            if (r < rows && c < n) {
                const long long tab = r / n, s = r - tab * n;
                WT[(tab * n + c) * n + s] = tile[tx][k];
            }
        }
        __syncthreads();
    }
}

}  // namespace ellhip
