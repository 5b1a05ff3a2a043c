// batch_svm_kernels.hpp -- the oracle of B independent SvmOracle problems of one shape (m samples, nfeat features), as a
// policy of the loop kernel (include/ellhip_batch_svm.h; the loop itself: batch_loop_kernels.hpp).
//
// For every ellipsoid of its workgroup k_batch_loop<T, STABLE, BatchSvmOracle> runs rounds of
//     oracle (SvmOracle::assess_optim, src/oracles/svm_oracle.rs:27-57)
//  -> x_best = xc (src/cutting_plane.rs:303; `shrunk` is always true)
//  -> scalar stage + rank-1 (batch_cut_apply with a central cut, the same code k_batch_update runs)
// without leaving the kernel.  margin_s = (double)label[s] * (a + x[nfeat]) with a folded from -0.0 in ascending j as
// a = a + x[j] * d[s][j], every product rounded before its add (Arr::dot, src/arr.rs:443-451; the build passes
// -ffp-contract=off) -- k_svm_margins' fold -- so the margins, the chosen sample, the cut and with them the whole loop are
// bit-identical to cutting_plane_optim over SvmOracle on the CPU.
//
// Mapping of the scan onto the n = nfeat + 1 threads of an instance (parallel over samples, never inside a fold): thread
// i takes samples i, i + n, i + 2n, ... in ascending order, reads x from the instance's LDS copy of the centre and keeps
// the strict-`<` minimum of its own samples (they ascend, so the first of equal values stays; NaN and +inf never pass `<`
// against +inf).  The n minima are merged in two LDS steps whose result does not depend on the order the threads arrive
// in: an atomic minimum over an order-preserving key of the value in which -0.0 is mapped to +0.0 FOR THE KEY ONLY (the
// reference's `==` ties the two zeros), then, after a barrier, an atomic minimum over the sample indices of the threads
// whose own minimum `==` the winning value.  The thread that holds the winning index writes its own value, so the winner
// keeps its own bits (the sign of a zero included).
//
// The table is stored feature-major, XT[t][j][ld] with ld = m rounded up to 8 doubles and t = 0 for a table shared by all
// problems, t = b otherwise: at fold step j the n threads of an instance read n consecutive doubles.  The gradient's
// nfeat strided reads of row idx come from the same table.  Labels are [B][m] int32.  Index arithmetic is 64-bit.
//
// Barriers are workgroup-wide; instances that take no part are masked off.  Every loop is bounded by ceil(m / n), nfeat
// and n; no thread waits on another workgroup.
//
// Nothing here is tied to the number of instances in a workgroup or to n <= 128: the streamed loops
// (k_batch_streamed_loop<BatchSvmOracle>, k_batch_streamed_loop_stable<BatchSvmOracle>; batch_svm_streamed_capi.inc.hpp,
// DESIGN section 9.10) take this policy unchanged with one instance per workgroup of n rounded up to 64 threads, n <= 1024.
// Bounded for 1024 threads (128 VGPRs a wave) they take 92 and 102 VGPRs and no scratch with BATCH_SVM_UNROLL = 8, so the
// unroll is the same for every instantiation.
#pragma once

#include <climits>

#include "batch_loop_kernels.hpp"

namespace ellhip {

// oracle scalars (LDS, per instance), after the loop's own (batch_loop_kernels.hpp)
enum : int {
    SV_GAMMA = BL_GAMMA,  // the loop's gamma
    SV_B0 = 5,        // the cut's beta
    SV_MINIDX = 6,    // the last scan's min_idx
    SV_MINVAL = 7,    // the last scan's min_val
    SV_KEY = 8,       // unsigned long long: smallest key of the threads' minima
    SV_WIDX = 9,      // int: smallest sample index among the threads that hold the winning value
    BATCH_SVM_SCALARS = 10,
};
static_assert(SV_B0 == BL_SCALARS, "the oracle's scalars follow the loop's");

// doubles of LDS the oracle needs per instance: x and the scalars
__host__ __device__ inline size_t batch_svm_lds_doubles(int n) { return ((size_t)n + BATCH_SVM_SCALARS) | 1; }

constexpr unsigned long long BATCH_SVM_NOKEY = ~0ull;  // above the key of every value: no sample below +inf

// order-preserving map of a non-NaN double onto unsigned integers, the two zeros on one key
__device__ __forceinline__ unsigned long long batch_svm_key(double v) {
    if (v == 0.0) v = 0.0;  // -0.0 -> +0.0
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double batch_svm_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

constexpr int BATCH_SVM_UNROLL = 8;  // features whose loads are in flight per thread, as in k_svm_margins

// One assess_optim for the workgroup's instances, collectively (it contains barriers: every thread of the workgroup calls
// it).  live: this thread belongs to an instance that takes part.  xt: the instance's table (nfeat x ld), lab: its m
// labels.  x: the instance's point (LDS, n); the caller has stored x[i] and has NOT synchronised yet.  margins (optional):
// the instance's m margins.  On return (after a barrier) gout is the gradient, osc[SV_B0] beta, osc[SV_GAMMA] the new
// gamma and osc[SV_MINIDX / SV_MINVAL] what the scan found.
__device__ __forceinline__ void batch_svm_oracle(const bool live, const int i, const int n, const int m, const long long ld,
                                                 const double* __restrict__ xt, const int* __restrict__ lab,
                                                 const double* x, double* osc, double* gout,
                                                 double* __restrict__ margins) {
    const int nfeat = n - 1;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(osc + SV_KEY);
    int* widx = reinterpret_cast<int*>(osc + SV_WIDX);
    if (live && i == 0) {
        *key = BATCH_SVM_NOKEY;
        *widx = INT_MAX;
    }
    __syncthreads();
    // ---- the scan: this thread's samples in ascending order               src/oracles/svm_oracle.rs:31-40
    double best = __builtin_inf();
    int bidx = -1;
    if (live) {
        const double bias = x[nfeat];
        for (int s = i; s < m; s += n) {
            const double* col = xt + s;
            double a = -0.0;  //                                              Arr::dot, src/arr.rs:443-451
            int j = 0;
            for (; j + BATCH_SVM_UNROLL <= nfeat; j += BATCH_SVM_UNROLL) {
                double v[BATCH_SVM_UNROLL];
#pragma unroll
                for (int u = 0; u < BATCH_SVM_UNROLL; ++u) v[u] = col[(long long)(j + u) * ld];
#pragma unroll
                for (int u = 0; u < BATCH_SVM_UNROLL; ++u) a = a + x[j + u] * v[u];  // loads run ahead, the adds stay in order
            }
            for (; j < nfeat; ++j) a = a + x[j] * col[(long long)j * ld];
            const double mg = (double)lab[s] * (a + bias);  //               :32
            if (margins) margins[s] = mg;
            if (mg < best) {  //                                              :33
                best = mg;
                bidx = s;
            }
        }
        if (bidx >= 0) atomicMin(key, batch_svm_key(best));
    }
    __syncthreads();
    const unsigned long long wkey = live ? *key : BATCH_SVM_NOKEY;
    // (`==` on the values, not on the keys: the two say the same, since no NaN ever becomes a thread's minimum)
    const bool holds = live && bidx >= 0 && best == batch_svm_unkey(wkey);
    if (holds) atomicMin(widx, bidx);
    __syncthreads();
    // ---- the cut                                                          :42-57
    if (live) {
        const int w = *widx;
        const bool none = w == INT_MAX;  // nothing below +inf: min_idx = 0, min_val = +inf
        const bool zero = none || batch_svm_unkey(wkey) >= 1.0;  //           :42 (the sign of a zero does not matter here)
        if (zero) {
            gout[i] = 0.0;
        } else {
            const double ny = -(double)lab[w];  //                            :47
            gout[i] = i < nfeat ? ny * xt[(long long)i * ld + w] : ny;  //    :49-52
        }
        if (none ? i == 0 : (holds && bidx == w)) {  // the winner writes its own value
            osc[SV_MINIDX] = none ? 0.0 : (double)w;
            osc[SV_MINVAL] = best;
            osc[SV_B0] = zero ? 0.0 : best;     //                            :44 / :56
            osc[SV_GAMMA] = zero ? 0.0 : best;  //                            :43 / :55
        }
    }
    __syncthreads();
}

// The oracle as the loop kernel's policy (batch_loop_kernels.hpp).  Per instance in HBM: the table, the labels and what
// the last scan found.
struct BatchSvmOracle {
    struct Args {
        const double* XT;      // [ntab][nfeat][ld]
        const int* labels;     // [B][m]
        long long tab_stride;  // nfeat * ld for per-problem tables, 0 for a shared one
        long long* min_idx;    // [B]
        double* min_val;       // [B]
        int m;
        long long ld;
    };
    struct Regs {
        const double* xt;  // this instance's table and labels
        const int* lab;
    };
    static __host__ __device__ inline size_t lds_doubles(const Args&, int n) { return batch_svm_lds_doubles(n); }
    static __device__ __forceinline__ size_t scalars_at(const Args&, int n) { return (size_t)n; }
    static __device__ __forceinline__ void load(const Args& A, bool active, long long b, int i, int n, double* blk, Regs& r) {
        r.xt = A.XT + (active ? b : 0) * A.tab_stride;
        r.lab = A.labels + (active ? b : 0) * (long long)A.m;
        if (active && i == 0) {
            double* osc = blk + n;
            osc[SV_B0] = 0.0;
            osc[SV_MINIDX] = (double)A.min_idx[b];
            osc[SV_MINVAL] = A.min_val[b];
        }
    }
    // (no barrier after the store of x: the oracle synchronises before it reads it)
    static __device__ __forceinline__ void assess(const Args& A, const BatchLoopRun&, bool live, int i, int n, double xci,
                                                  double* blk, Regs& r, double* g) {
        if (live) blk[i] = xci;
        batch_svm_oracle(live, i, n, A.m, A.ld, r.xt, r.lab, blk, blk + n, g, nullptr);
    }
    // `shrunk` is always true (src/oracles/svm_oracle.rs:44, :56)
    static __device__ __forceinline__ BatchOutcome outcome(const Args&, int, const double* osc) {
        return BatchOutcome{BOUT_SHRUNK, osc[SV_B0], 0, 0.0};
    }
    static __device__ __forceinline__ void store(const Args& A, long long b, const double* osc, const Regs&) {
        A.min_idx[b] = (long long)osc[SV_MINIDX];
        A.min_val[b] = osc[SV_MINVAL];
    }
};

// One assess_optim per instance at x[B][n]: the same device function, without an ellipsoid.  keep_last: record the scan in
// A.min_idx / A.min_val (the margins entry point looks without touching the oracle's state).  margins: [B][m] or null.
// Two launch shapes: epw instances packed into T = 128 or 256 threads (n <= 128), or the wide one past it -- epw = 1, one
// workgroup per instance, blockDim.x = n rounded up to 64 (T = 1024 only bounds the block); threads tid >= n belong to no
// instance (e = 1 >= epw), are inactive in the oracle and take part in its barriers.  LDS: epw * (batch_svm_lds_doubles(n) +
// n) doubles.  Every loop is bounded by ceil(m / n), nfeat and n; no thread waits on another workgroup or on a memory word.
template <int T>
__global__ __launch_bounds__(T) void k_batch_svm_assess(long long B, int n, int epw, int keep_last, BatchSvmOracle::Args A,
                                                        const double* __restrict__ x, double* __restrict__ gamma_out,
                                                        double* __restrict__ grad_out, double* __restrict__ beta_out,
                                                        double* __restrict__ margins) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * epw + e;
    const bool active = e < epw && b < B;
    const size_t lper = batch_svm_lds_doubles(n) + (size_t)n;
    double* lx = sm + (size_t)(e < epw ? e : 0) * lper;
    double* osc = lx + n;
    double* g = osc + BATCH_SVM_SCALARS;
    const double* xt = A.XT;
    const int* lab = A.labels;
    double* mg = nullptr;
    if (active) {
        lx[i] = x[b * n + i];
        xt = A.XT + b * A.tab_stride;
        lab = A.labels + b * (long long)A.m;
        if (margins) mg = margins + b * (long long)A.m;
    }
    batch_svm_oracle(active, i, n, A.m, A.ld, xt, lab, lx, osc, g, mg);
    if (active && grad_out) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        if (gamma_out) gamma_out[b] = osc[SV_GAMMA];
        if (beta_out) beta_out[b] = osc[SV_B0];
        if (keep_last) BatchSvmOracle::store(A, b, osc, BatchSvmOracle::Regs{});
    }
}

// Tiled transpose of one slab of the caller's row-major tables into XT.  The tables are taken as one [ntab * m][nfeat]
// matrix; the slab holds its rows [r0, r0 + rows).  Row r is sample r % m of table r / m.
constexpr int BATCH_SVM_TILE = 32;
__global__ __launch_bounds__(256) void k_batch_svm_transpose(const double* __restrict__ slab, long long rows, long long r0,
                                                             long long m, long long nfeat, long long ld,
                                                             double* __restrict__ XT) {
    __shared__ double tile[BATCH_SVM_TILE][BATCH_SVM_TILE + 1];
    const long long tcols = (nfeat + BATCH_SVM_TILE - 1) / BATCH_SVM_TILE;
    const long long trows = (rows + BATCH_SVM_TILE - 1) / BATCH_SVM_TILE;
    const int tx = threadIdx.x & (BATCH_SVM_TILE - 1), ty = threadIdx.x / BATCH_SVM_TILE;  // 32 x 8
    for (long long t = blockIdx.x; t < tcols * trows; t += gridDim.x) {
        const long long rb = (t / tcols) * BATCH_SVM_TILE, cb = (t % tcols) * BATCH_SVM_TILE;
        for (int k = ty; k < BATCH_SVM_TILE; k += 256 / BATCH_SVM_TILE) {
            const long long r = rb + k, c = cb + tx;
            if (r < rows && c < nfeat) tile[k][tx] = slab[r * nfeat + c];
        }
        __syncthreads();
        for (int k = ty; k < BATCH_SVM_TILE; k += 256 / BATCH_SVM_TILE) {
            const long long c = cb + k, r = rb + tx;
            if (r < rows && c < nfeat) {
                const long long gr = r0 + r, tab = gr / m, s = gr - tab * m;
                XT[(tab * nfeat + c) * ld + s] = tile[tx][k];
            }
        }
        __syncthreads();
    }
}

}  // namespace ellhip
