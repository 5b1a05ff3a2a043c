// batch_linfeas_kernels.hpp -- B independent linear feasibility oracles with a movable target (MyOracle3, src/example3.rs, as
// a family) as one policy of the loop kernel (include/ellhip_batch_bsearch.h; the loop:
// batch_loop_kernels.hpp), and k_batch_bsearch, the kernel that runs bsearch over BSearchAdaptor (src/cutting_plane.rs:403-419,
// :441-466) for every problem without a host in the loop.
//
// The oracle.  Problem b has J rows A[j][0..n) and offsets c[j], a cursor idx (-1 at first) and a target (-1e100 at first).
// assess_feas(x) walks at most J rows cyclically after the cursor (idx += 1; if idx == J { idx = 0 }, src/example3.rs:29-33);
// for each it takes
//     f = 0.0;  for k ascending: f += A[j][k] * x[k]        (two roundings per term: the file is compiled -ffp-contract=off)
//     fj = f - c[j]  for j < J - 1,   fj = f - target  for j = J - 1      (the last row has no offset of its own)
// and answers the first fj > 0.0 with (A[j], SingleCut(fj)) (:41-52), or None (:54).  update(gamma) sets the target (:57-59).
//
// MyOracle3 is A = [[-1, 0], [0, -1], [1, 1], [2, -3]], c = (1, 2, 1, .).  Its four expressions (:35-38) against the folds,
// for finite x = (x, y): a product with +-1 is exact and a product with 0 is a zero, so
//     row 0   (0.0 + -x) + 0 y  against  -x            row 1   (0.0 + 0 x) + -y  against  -y
//     row 2   (0.0 + x) + y     against  x + y         row 3   (0.0 + 2 x) + -3 y  against  2 x - 3 y
// differ in nothing but the sign of a zero: 0.0 + v == v for every v but -0.0, u + (-w) is u - w, (-3) y is -(3 y), and a
// zero added to a non-zero changes nothing.  Rows 0 to 2 then subtract a non-zero offset, which forgets the sign of a zero:
// their fj have the same bits as the reference's.  Row 3 subtracts the target: the same bits whenever the target or
// 2 x - 3 y is non-zero; with both zero the two fj are zeros whose signs may differ (x = -0.0, y = 0.0: the reference has
// -0.0 - 0.0 = -0.0, the fold 0.0 - 0.0 = 0.0), neither is > 0.0, and a fj that is not > 0.0 is never handed out.  So the
// answers -- which row, and its fj -- have the same bits for every finite x and every target.  For a non-finite x the fold
// is the definition (0 * inf is NaN in the fold and absent from the reference's expression).
//
// Work split.  Thread t of an instance (it has n) folds rows t, t + n, ... into J doubles of the oracle's LDS block; after a
// barrier the instance's first thread walks the cursor over them and names the row; after another every thread fetches its
// element of that row as the gradient.  All J rows are evaluated whether or not the walk reaches them (a lane that skipped
// one would wait for its neighbours): J n multiply-adds per call against the update's about 2 n^2.  The rows are read from
// HBM (L2 for a shared table) in every call: J n doubles do not fit beside the ellipsoids in LDS.
//
// Barriers are workgroup-wide; threads that take no part (live = false) skip the loads and stores and take part in every
// barrier.  Every loop is bounded by J, n or the launch's iteration count; no thread waits on another workgroup.
#pragma once

#include "batch_loop_kernels.hpp"

namespace ellhip {

constexpr int BATCH_LINFEAS_JMAX = 512;  // (the tests' family has J = 2 n + 3 = 259 rows at n = 128)

// oracle scalars, after the loop's own (batch_loop_kernels.hpp)
enum : int {
    LF_B0 = 5,      // the cut's beta
    LF_FEAS = 6,    // 1.0: no row was violated
    LF_IDX = 7,     // the cursor
    LF_TARGET = 8,  // the movable offset of the last row
    BATCH_LINFEAS_SCALARS = 9,
};
static_assert(LF_B0 == BL_SCALARS, "the oracle's scalars follow the loop's");

// an instance's LDS block: the point x [n], the folds f [J], the scalars
__host__ __device__ inline size_t batch_linfeas_lds_doubles(int n, int J) {
    return ((size_t)n + (size_t)J + BATCH_LINFEAS_SCALARS) | 1;
}

struct BatchLinFeasOracle {
    struct Args {
        const double* a;     // rows: [J][n] (a_stride = 0) or [B][J][n] (a_stride = J n)
        const double* c;     // offsets: [J] (c_stride = 0) or [B][J]; entry J - 1 is never read
        long long a_stride;
        long long c_stride;
        int J;
        int* idx;            // [B]
        double* target;      // [B]
    };
    struct Regs {
        const double* a;  // this instance's rows and offsets
        const double* c;
    };
    static __host__ __device__ inline size_t lds_doubles(const Args& A, int n) { return batch_linfeas_lds_doubles(n, A.J); }
    static __host__ __device__ __forceinline__ size_t scalars_at(const Args& A, int n) { return (size_t)n + (size_t)A.J; }
    static __device__ __forceinline__ void load(const Args& A, bool active, long long b, int i, int n, double* blk, Regs& r) {
        r.a = A.a;
        r.c = A.c;
        if (active) {
            r.a = A.a + b * A.a_stride;
            r.c = A.c + b * A.c_stride;
            if (i == 0) {
                double* osc = blk + scalars_at(A, n);
                osc[LF_B0] = 0.0;
                osc[LF_FEAS] = 0.0;
                osc[LF_IDX] = (double)A.idx[b];
                osc[LF_TARGET] = A.target[b];
            }
        }
    }
    // update(gamma)                                                                                   src/example3.rs:57-59
    static __device__ __forceinline__ void update(double* osc, double gamma) { osc[LF_TARGET] = gamma; }
    static __device__ __forceinline__ void assess(const Args& A, const BatchLoopRun&, bool live, int i, int n, double xci,
                                                  double* blk, Regs& r, double* g) {
        const int J = A.J;
        double* f = blk + n;
        double* osc = f + J;
        if (live) blk[i] = xci;
        __syncthreads();
        if (live) {
            for (int j = i; j < J; j += n) {
                const double* row = r.a + (size_t)j * n;
                double acc = 0.0;
#pragma unroll 4
                for (int k = 0; k < n; ++k) acc += row[k] * blk[k];
                f[j] = acc;
            }
        }
        __syncthreads();
        if (live && i == 0) {  //                                                                              :29-54
            int idx = (int)osc[LF_IDX];
            const double target = osc[LF_TARGET];
            bool cut = false;
            double fj = 0.0;
            for (int t = 0; t < J; ++t) {
                idx += 1;
                if (idx == J) idx = 0;
                fj = f[idx] - (idx == J - 1 ? target : r.c[idx]);
                if (fj > 0.0) {
                    cut = true;
                    break;
                }
            }
            osc[LF_IDX] = (double)idx;
            osc[LF_B0] = cut ? fj : 0.0;
            osc[LF_FEAS] = cut ? 0.0 : 1.0;
        }
        __syncthreads();
        if (live) g[i] = osc[LF_FEAS] != 0.0 ? 0.0 : r.a[(size_t)(int)osc[LF_IDX] * n + i];
        __syncthreads();
    }
    static __device__ __forceinline__ BatchOutcome outcome(const Args&, int, const double* osc) {
        return BatchOutcome{osc[LF_FEAS] != 0.0 ? BOUT_FEAS : BOUT_CUT, osc[LF_B0], 0, 0.0};
    }
    static __device__ __forceinline__ void store(const Args& A, long long b, const double* osc, const Regs&) {
        A.idx[b] = (int)osc[LF_IDX];
        A.target[b] = osc[LF_TARGET];
    }
};

// One assess_feas per instance at x[B][n], without an ellipsoid: the same device function.  Shaped as the loop is (n threads
// per instance, epw instances per workgroup); cut_out[b] = the row of the cut or -1.
template <int T>
__global__ __launch_bounds__(T) void k_batch_linfeas_assess(long long B, int n, int epw, BatchLinFeasOracle::Args A,
                                                            const double* __restrict__ x, double* __restrict__ grad_out,
                                                            double* __restrict__ beta_out, int* __restrict__ cut_out) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * epw + e;
    const bool active = e < epw && b < B;
    const size_t lper = BatchLinFeasOracle::lds_doubles(A, n) + (size_t)n;
    double* blk = sm + (size_t)(e < epw ? e : 0) * lper;
    double* osc = blk + BatchLinFeasOracle::scalars_at(A, n);
    double* g = blk + BatchLinFeasOracle::lds_doubles(A, n);
    BatchLinFeasOracle::Regs r;
    BatchLinFeasOracle::load(A, active, b, i, n, blk, r);
    const double xi = active ? x[b * n + i] : 0.0;
    BatchLoopRun R{1, 1, 1, 0.0};
    BatchLinFeasOracle::assess(A, R, active, i, n, xi, blk, r, g);  // (its first barrier orders load's scalars)
    if (active) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        const bool feas = osc[LF_FEAS] != 0.0;
        beta_out[b] = osc[LF_B0];
        cut_out[b] = feas ? -1 : (int)osc[LF_IDX];
        BatchLinFeasOracle::store(A, b, osc, r);
    }
}

// ---- bsearch over BSearchAdaptor ---------------------------------------------------------------------------------------------
// the bisection's scalars per instance: [B][BS_N] doubles in HBM beside the cursor, and in LDS while a launch runs
enum : int {
    BS_LOWER = 0,
    BS_UPPER = 1,
    BS_UORIG = 2,
    BS_GAMMA = 3,     // the probe's gamma
    BS_OUTER = 4,     // probes finished
    BS_INNER = 5,     // cuts applied in this probe: cutting_plane_feas's niter
    BS_CLONE = 6,     // 1.0: a probe has begun and its space is still to be cloned
    BS_STOPPED = 7,
    BS_NITER = 8,     // bsearch's second result
    BS_ROUNDS = 9,    // oracle calls
    BS_END = 10,      // [4] how the probes ended: feasible, a failed cut, the tolerance, inner_max_iters
    BS_N = 15,        // (odd: the first threads of a wave's instances hit different LDS banks)
};

struct BatchBsRun {
    int iters;  // rounds this launch may run
    long long inner_max_iters;
    double inner_tol;
    long long max_iters;
    double tol;
};

struct BatchBsBuffers {
    double* state;  // [B][BS_N]
    int* nstopped;  // [1]
    // the probe's space, laid out as the batch handle's
    double* Q;      // [B][n][n]
    double* xc;     // [B][n]
    double* kappa;  // [B]
    double* tsq;    // [B]
};

// Between two probes, on the instance's first thread: bsearch's loop head (:451-457) and the adaptor's update(gamma) (:411),
// until a probe begins (BS_CLONE) or the search stops.  A probe with inner_max_iters = 0 ends without an oracle call
// (:215, :226), so the loop goes on at once; it is bounded by max_iters.
template <class Oracle>
__device__ __forceinline__ void batch_bs_outer_step(const BatchBsRun& R, double* bs, double* osc, int* nstopped) {
    bs[BS_CLONE] = 0.0;
    for (;;) {
        const double outer = bs[BS_OUTER];
        const double lower = bs[BS_LOWER], upper = bs[BS_UPPER];
        bool stop = outer >= (double)R.max_iters;  //                                                              :465
        if (!stop) {
            const double tau = (upper - lower) / 2.0;  //                                                          :452
            stop = tau < R.tol;                        //                                                          :453
            if (!stop) {
                double gamma = lower;  //                                                                      :456-457
                gamma += tau;
                bs[BS_GAMMA] = gamma;
                Oracle::update(osc, gamma);
                if (R.inner_max_iters > 0) {
                    bs[BS_INNER] = 0.0;
                    bs[BS_CLONE] = 1.0;
                    return;
                }
                bs[BS_END + 3] += 1.0;
                bs[BS_LOWER] = gamma;  //                                                                          :462
                bs[BS_OUTER] = outer + 1.0;
            }
        }
        if (stop) {
            bs[BS_NITER] = outer;
            bs[BS_STOPPED] = 1.0;
            atomicAdd(nstopped, 1);
            return;
        }
    }
}

// bsearch (:441-466) with BSearchAdaptor::assess_bs (:409-418) as its oracle, per instance, up to R.iters rounds (a round is
// one oracle call of one probe's cutting_plane_feas, :215-225).  A sibling of k_batch_loop: the same thread layout, LDS
// layout and barrier discipline, the same Oracle policy, batch_copy and batch_space_cut_apply; what is its own is the
// two-level state.  The instances of a workgroup are at different probes in the same round, so a probe's end, the outer step
// and the clone are per-instance phases behind the workgroup-wide barriers, masked as `live` is.
//
// Qb, kb, tb: the adaptor's space, read only; xcb: its centre, written by set_xc (:414).  W: the probe's space and the
// bisection state between launches.  A clone (:410) is the instance's n^2 doubles read again from Qb into its LDS block,
// with xcb, kb and tb; the other instances keep theirs.
template <int T, bool STABLE, class Oracle>
__global__ __launch_bounds__(T) void k_batch_bsearch(BatchParams P, BatchBsRun R, const double* __restrict__ Qb,
                                                     double* __restrict__ xcb, const double* __restrict__ kb,
                                                     const double* __restrict__ tb, BatchBsBuffers W,
                                                     typename Oracle::Args A, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, pitch = P.pitch;
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * P.epw + e;
    const bool active = e < P.epw && b < P.B;
    if (!__syncthreads_or(active && W.state[b * BS_N + BS_STOPPED] == 0.0)) return;

    const size_t per = batch_space_lds_doubles<STABLE>(n);
    const size_t lper = Oracle::lds_doubles(A, n);
    const size_t lsc = Oracle::scalars_at(A, n);
    const int el = e < P.epw ? e : 0;
    double* q = sm + (size_t)el * per;
    double* g = q + (size_t)n * pitch;
    double* sc = q + batch_space_scalars_at<STABLE>(n);
    double* blk = sm + (size_t)P.epw * per + (size_t)el * lper;
    double* osc = blk + lsc;
    double* bs = sm + (size_t)P.epw * (per + lper) + (size_t)el * BS_N;

    const long long b_first = (long long)blockIdx.x * P.epw;
    const int nb = (int)((P.B - b_first < P.epw) ? P.B - b_first : P.epw);
    double* Qwg = W.Q + b_first * (long long)n * n;
    batch_copy<T, true>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
    double xci = 0.0;
    typename Oracle::Regs r;
    if (active) xci = W.xc[b * n + i];
    Oracle::load(A, active, b, i, n, blk, r);
    if (active && i == 0) {
        sc[3] = (double)ST_SUCCESS;
        sc[4] = W.kappa[b];
        sc[5] = W.tsq[b];
        for (int k = 0; k < BS_N; ++k) bs[k] = W.state[b * BS_N + k];
        osc[BL_STOPPED] = 0.0;
        if (bs[BS_STOPPED] == 0.0 && bs[BS_INNER] < 0.0)  // a call begins between two probes
            batch_bs_outer_step<Oracle>(R, bs, osc, W.nstopped);
    }
    __syncthreads();

    const bool lane_ok = tid < P.epw && b_first + tid < P.B;
    const int es = tid < P.epw ? tid : 0;
    double* q_s = sm + (size_t)es * per;
    const double* osc_s = sm + (size_t)P.epw * per + (size_t)es * lper + lsc;
    const double* bs_s = sm + (size_t)P.epw * (per + lper) + (size_t)es * BS_N;
    const double* Qmine = Qb + (active ? b : 0) * (long long)n * n;
    BatchLoopRun RL{R.iters, 1, R.inner_max_iters, R.inner_tol};

    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && bs[BS_STOPPED] == 0.0;  // not stopped: in a probe
        if (!__syncthreads_or(live)) break;
        if (live && bs[BS_CLONE] != 0.0) {  // let mut space = self.space.clone()                                  :410
            for (int k = 0; k < n; ++k) q[(size_t)k * pitch + i] = Qmine[(size_t)k * n + i];
            xci = xcb[b * n + i];
            if (i == 0) {
                sc[4] = kb[b];
                sc[5] = tb[b];
            }
        }
        Oracle::assess(A, RL, live, i, n, xci, blk, r, g);  // (its barriers order the clone before the cut)
        const BatchOutcome mine = Oracle::outcome(A, 1, osc);
        const bool found = live && mine.what == BOUT_FEAS;  //                                                 :217-220
        const bool upd = live && mine.what == BOUT_CUT;
        const BatchOutcome its = Oracle::outcome(A, 1, osc_s);
        const bool lane = lane_ok && bs_s[BS_STOPPED] == 0.0 && its.what == BOUT_CUT;
        const double b0 = lane ? its.b0 : 0.0;
        batch_space_cut_apply<STABLE>(P, calc, upd, i, q, xci, lane, q_s, CUT_BIAS, b0, 0, 0.0, [](int, double) {});
        if (found) xcb[b * n + i] = xci;  // self.space.set_xc(x)                                                   :414
        if (live && i == 0) {
            bs[BS_ROUNDS] += 1.0;
            int end = -1;
            if (found) {
                end = 0;
            } else if (!upd) {  // (an oracle of this driver always answers)
                end = 1;
            } else if (sc[3] != (double)ST_SUCCESS) {  //                                                          :222
                end = 1;
            } else if (sc[5] < R.inner_tol) {
                end = 2;
            } else {
                const double done = bs[BS_INNER] + 1.0;
                bs[BS_INNER] = done;
                if (done >= (double)R.inner_max_iters) end = 3;  //                                                :226
            }
            if (end < 0) {
                bs[BS_CLONE] = 0.0;
            } else {
                bs[BS_END + end] += 1.0;
                if (end == 0) bs[BS_UPPER] = bs[BS_GAMMA];  //                                                     :460
                else bs[BS_LOWER] = bs[BS_GAMMA];           //                                                     :462
                bs[BS_OUTER] += 1.0;
                bs[BS_INNER] = -1.0;
                batch_bs_outer_step<Oracle>(R, bs, osc, W.nstopped);
            }
        }
        __syncthreads();
    }

    if (active) W.xc[b * n + i] = xci;
    if (active && i == 0) {
        W.kappa[b] = sc[4];
        W.tsq[b] = sc[5];
        Oracle::store(A, b, osc, r);
        for (int k = 0; k < BS_N; ++k) W.state[b * BS_N + k] = bs[k];
    }
    batch_copy<T, false>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
}

}  // namespace ellhip
