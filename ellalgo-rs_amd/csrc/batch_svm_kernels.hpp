// batch_svm_kernels.hpp -- B independent SvmOracle problems of one shape (m samples, nfeat features), oracle and ellipsoid
// update in one kernel (include/ellhip_batch_svm.h).
//
// A workgroup owns the ellipsoids the batch engine gives it (batch_kernels.hpp: thread (e, i) = row i of local ellipsoid
// e, Q in LDS) and, for each of them, runs up to `iters` rounds of
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
// Barriers are workgroup-wide; stopped instances are masked off and the loop is driven by __syncthreads_or votes.  Every
// loop is bounded by iters, ceil(m / n), nfeat and n; no thread waits on another workgroup.
#pragma once

#include <climits>

#include "batch_stable_apply.hpp"

namespace ellhip {

// oracle and loop scalars (LDS, per instance)
enum : int {
    SV_B0 = 0,        // the cut's beta
    SV_GAMMA = 1,     // the loop's gamma
    SV_MINIDX = 2,    // the last scan's min_idx
    SV_MINVAL = 3,    // the last scan's min_val
    SV_NITER = 4,
    SV_STOPPED = 5,
    SV_HASBEST = 6,
    SV_STATUS = 7,
    SV_KEY = 8,       // unsigned long long: smallest key of the threads' minima
    SV_WIDX = 9,      // int: smallest sample index among the threads that hold the winning value
    BATCH_SVM_SCALARS = 10,
};

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

struct BatchSvmArrays {
    const double* XT;      // [ntab][nfeat][ld]
    const int* labels;     // [B][m]
    long long tab_stride;  // nfeat * ld for per-problem tables, 0 for a shared one
    long long* min_idx;    // [B]
    double* min_val;       // [B]
    double* gamma;         // [B]
    double* xbest;         // [B][n]
    int* has_best;         // [B]
    long long* niter;      // [B]
    int* stopped;          // [B]
    int* status;           // [B]
    int* nstopped;         // [1]
};

struct BatchSvmLoop {
    int iters;  // iterations this launch may run
    int m;
    long long ld;
    long long max_iters;
    double tol;
};

// cutting_plane_optim (src/cutting_plane.rs:286-313) for every instance of the workgroup.  Loop state per instance lives in
// HBM between launches (BatchSvmArrays).  STABLE: the spaces are EllStable buffers and a cut is batch_stable_cut_apply
// (batch_stable_apply.hpp).
template <int T, bool STABLE = false>
__global__ __launch_bounds__(T) void k_batch_svm_loop(BatchParams P, BatchSvmLoop R, double* __restrict__ Q,
                                                      double* __restrict__ xc, double* __restrict__ kappa,
                                                      double* __restrict__ tsq, BatchSvmArrays A, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, pitch = P.pitch;
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * P.epw + e;
    const bool active = e < P.epw && b < P.B;
    if (!__syncthreads_or(active && A.stopped[b] == 0)) return;  // all of this workgroup's instances have stopped

    const size_t per = batch_space_lds_doubles<STABLE>(n);
    const size_t lper = batch_svm_lds_doubles(n);
    const int el = e < P.epw ? e : 0;
    double* q = sm + (size_t)el * per;
    double* g = q + (size_t)n * pitch;
    double* sc = q + batch_space_scalars_at<STABLE>(n);  // as in k_batch_update
    double* lx = sm + (size_t)P.epw * per + (size_t)el * lper;
    double* osc = lx + n;

    const long long b_first = (long long)blockIdx.x * P.epw;
    const int nb = (int)((P.B - b_first < P.epw) ? P.B - b_first : P.epw);
    double* Qwg = Q + b_first * (long long)n * n;
    batch_copy<T, true>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
    double xci = 0.0, xb = 0.0;
    const double* xt = A.XT;
    const int* lab = A.labels;
    if (active) {
        xci = xc[b * n + i];
        xb = A.xbest[b * n + i];
        xt = A.XT + b * A.tab_stride;
        lab = A.labels + b * (long long)R.m;
    }
    if (active && i == 0) {
        sc[3] = (double)ST_SUCCESS;
        sc[4] = kappa[b];
        sc[5] = tsq[b];
        osc[SV_B0] = 0.0;
        osc[SV_GAMMA] = A.gamma[b];
        osc[SV_MINIDX] = (double)A.min_idx[b];
        osc[SV_MINVAL] = A.min_val[b];
        osc[SV_NITER] = (double)A.niter[b];
        osc[SV_STOPPED] = (double)A.stopped[b];
        osc[SV_HASBEST] = (double)A.has_best[b];
        osc[SV_STATUS] = (double)A.status[b];
    }
    __syncthreads();

    const bool lane_ok = tid < P.epw && b_first + tid < P.B;
    const int es = tid < P.epw ? tid : 0;
    double* q_s = sm + (size_t)es * per;
    const double* osc_s = sm + (size_t)P.epw * per + (size_t)es * lper + n;

    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && osc[SV_STOPPED] == 0.0;
        if (!__syncthreads_or(live)) break;
        if (live) lx[i] = xci;
        batch_svm_oracle(live, i, n, R.m, R.ld, xt, lab, lx, osc, g, nullptr);
        if (live) xb = xci;  // x_best = Some(space.xc())                    src/cutting_plane.rs:303
        const bool lane = lane_ok && osc_s[SV_STOPPED] == 0.0;
        const double b0 = lane ? osc_s[SV_B0] : 0.0;
        batch_space_cut_apply<STABLE>(P, calc, live, i, q, xci, lane, q_s, CUT_CENTRAL, b0, 0, 0.0,
                                      [](int, double) {});  //                :304
        if (live && i == 0) {
            osc[SV_HASBEST] = 1.0;
            bool stop;
            if (sc[3] != (double)ST_SUCCESS || sc[5] < R.tol) {  //          :308
                osc[SV_STATUS] = sc[3];
                stop = true;
            } else {
                const double done = osc[SV_NITER] + 1.0;
                osc[SV_NITER] = done;
                osc[SV_STATUS] = (double)ST_SUCCESS;
                stop = done >= (double)R.max_iters;
            }
            if (stop) {
                osc[SV_STOPPED] = 1.0;
                atomicAdd(A.nstopped, 1);
            }
        }
        __syncthreads();
    }

    if (active) {
        xc[b * n + i] = xci;
        if (osc[SV_HASBEST] != 0.0) A.xbest[b * n + i] = xb;
    }
    if (active && i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
        A.gamma[b] = osc[SV_GAMMA];
        A.min_idx[b] = (long long)osc[SV_MINIDX];
        A.min_val[b] = osc[SV_MINVAL];
        A.niter[b] = (long long)osc[SV_NITER];
        A.stopped[b] = (int)osc[SV_STOPPED];
        A.has_best[b] = (int)osc[SV_HASBEST];
        A.status[b] = (int)osc[SV_STATUS];
    }
    batch_copy<T, false>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
}

// One assess_optim per instance at x[B][n]: the same device function, without an ellipsoid.  keep_last: record the scan in
// A.min_idx / A.min_val (the margins entry point looks without touching the oracle's state).  margins: [B][m] or null.
template <int T>
__global__ __launch_bounds__(T) void k_batch_svm_assess(long long B, int n, int epw, int m, long long ld, int keep_last,
                                                        BatchSvmArrays A, const double* __restrict__ x,
                                                        double* __restrict__ gamma_out, double* __restrict__ grad_out,
                                                        double* __restrict__ beta_out, double* __restrict__ margins) {
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
        lab = A.labels + b * (long long)m;
        if (margins) mg = margins + b * (long long)m;
    }
    batch_svm_oracle(active, i, n, m, ld, xt, lab, lx, osc, g, mg);
    if (active && grad_out) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        if (gamma_out) gamma_out[b] = osc[SV_GAMMA];
        if (beta_out) beta_out[b] = osc[SV_B0];
        if (keep_last) {
            A.min_idx[b] = (long long)osc[SV_MINIDX];
            A.min_val[b] = osc[SV_MINVAL];
        }
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
