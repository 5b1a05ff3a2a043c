// batch_loop_kernels.hpp -- the one cutting-plane loop kernel of the batched device-resident solves.
//
// A workgroup owns the ellipsoids the batch engine gives it (batch_kernels.hpp: thread (e, i) = row i of local
// ellipsoid e, Q in LDS) and, for each of them, runs up to `iters` rounds of
//     oracle -> x_best -> scalar stage + rank-1 (batch_space_cut_apply, the code k_batch_update runs) -> stop test
// without leaving the kernel: cutting_plane_optim (src/cutting_plane.rs:286-313) and cutting_plane_feas (:205-227), once, and
// under DRIVER = BATCH_DRIVER_OPTIM_Q cutting_plane_optim_q (:331-374), whose rounds differ where marked Q below.
// What differs between the problems is the Oracle policy (batch_lmi_kernels.hpp, batch_lowpass_kernels.hpp,
// batch_svm_kernels.hpp): a type with
//     struct Args                     what the oracle reads and keeps in HBM; a kernel argument, by value
//     struct Regs                     what a thread keeps of its instance in registers
//     lds_doubles(A, n)               doubles of LDS per instance: the point x first, the scalars at scalars_at(A, n)
//     load(A, active, b, i, n, blk, r)    the instance's constants and oracle state into blk and r (before a barrier)
//     assess(A, R, live, i, n, xci, blk, r, g)    collective: x = xc, one oracle call, gradient into g; ends in a barrier
//     outcome(A, feas, osc)           the answer found in an instance's scalars
//     store(A, b, osc, r)             the oracle state back to HBM (thread 0 of the instance)
// all static __device__ __forceinline__.  The skeleton never asks which oracle it serves.  An oracle of the optim_q driver
// (an OracleOptimQ) also names two of its scalars, Q_RETRY and Q_MORE_ALT: its assess reads `retry` from the first, leaves
// `more_alt` in the second and the point x_q in the first n doubles of its block; load and store carry Q_RETRY through HBM.
//
// Barriers are workgroup-wide; stopped instances are masked off and the loop is driven by __syncthreads_or votes.  Every
// loop is bounded by iters and the oracle's own bounds; no thread waits on another workgroup.
#pragma once

#include "batch_stable_apply.hpp"

namespace ellhip {

// the loop's scalars (LDS, per instance): the first slots of every oracle's scalars, whose own slots follow
enum : int {
    BL_GAMMA = 0,    // best-so-far objective value
    BL_NITER = 1,
    BL_STOPPED = 2,
    BL_HASBEST = 3,
    BL_STATUS = 4,
    BL_SCALARS = 5,
};

// loop state per instance, in HBM between launches
struct BatchLoopState {
    double* gamma;     // [B]
    double* xbest;     // [B][n]
    int* has_best;     // [B]
    long long* niter;  // [B]
    int* stopped;      // [B]
    int* status;       // [B]
    int* nstopped;     // [1]
};

struct BatchLoopRun {
    int iters;  // iterations this launch may run
    int feas;   // 1: cutting_plane_feas
    long long max_iters;
    double tol;
};

// what one oracle call gave the loop
enum : int {
    BOUT_NONE = 0,    // nothing to cut with: the loop stops with ST_UNKNOWN
    BOUT_CUT = 1,     // a cut through or beside the centre
    BOUT_SHRUNK = 2,  // the centre is the best point so far, and a central cut
    BOUT_FEAS = 3,    // cutting_plane_feas: the centre is feasible
};
struct BatchOutcome {
    int what;
    double b0;
    int has_b1;
    double b1;
};

// which of the reference's drivers a loop kernel runs
enum : int {
    BATCH_DRIVER_OPTIM = 0,    // cutting_plane_optim and, with R.feas, cutting_plane_feas
    BATCH_DRIVER_OPTIM_Q = 1,  // cutting_plane_optim_q: discrete cuts (CUT_Q) and the retry after NoEffect
};

// STABLE: the spaces are EllStable buffers and a cut is batch_stable_cut_apply (batch_stable_apply.hpp).
template <int T, bool STABLE, class Oracle, int DRIVER = BATCH_DRIVER_OPTIM>
__global__ __launch_bounds__(T) void k_batch_loop(BatchParams P, BatchLoopRun R, double* __restrict__ Q,
                                                  double* __restrict__ xc, double* __restrict__ kappa,
                                                  double* __restrict__ tsq, BatchLoopState S, typename Oracle::Args A,
                                                  EllCalcDev calc) {
    extern __shared__ double sm[];
    constexpr bool DRIVER_Q = DRIVER == BATCH_DRIVER_OPTIM_Q;
    const int n = P.n, pitch = P.pitch;
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * P.epw + e;
    const bool active = e < P.epw && b < P.B;
    if (!__syncthreads_or(active && S.stopped[b] == 0)) return;  // all of this workgroup's instances have stopped

    const size_t per = batch_space_lds_doubles<STABLE>(n);
    const size_t lper = Oracle::lds_doubles(A, n);
    const size_t lsc = Oracle::scalars_at(A, n);
    const int el = e < P.epw ? e : 0;
    double* q = sm + (size_t)el * per;
    double* g = q + (size_t)n * pitch;
    double* sc = q + batch_space_scalars_at<STABLE>(n);  // as in k_batch_update
    double* blk = sm + (size_t)P.epw * per + (size_t)el * lper;
    double* osc = blk + lsc;

    const long long b_first = (long long)blockIdx.x * P.epw;
    const int nb = (int)((P.B - b_first < P.epw) ? P.B - b_first : P.epw);
    double* Qwg = Q + b_first * (long long)n * n;
    batch_copy<T, true>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
    double xci = 0.0, xb = 0.0;
    typename Oracle::Regs r;
    if (active) {
        xci = xc[b * n + i];
        xb = S.xbest[b * n + i];
    }
    Oracle::load(A, active, b, i, n, blk, r);
    if (active && i == 0) {
        sc[3] = (double)ST_SUCCESS;
        sc[4] = kappa[b];
        sc[5] = tsq[b];
        osc[BL_GAMMA] = S.gamma[b];
        osc[BL_NITER] = (double)S.niter[b];
        osc[BL_STOPPED] = (double)S.stopped[b];
        osc[BL_HASBEST] = (double)S.has_best[b];
        osc[BL_STATUS] = (double)S.status[b];
    }
    __syncthreads();

    const bool lane_ok = tid < P.epw && b_first + tid < P.B;
    const int es = tid < P.epw ? tid : 0;
    double* q_s = sm + (size_t)es * per;
    const double* osc_s = sm + (size_t)P.epw * per + (size_t)es * lper + lsc;

    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && osc[BL_STOPPED] == 0.0;
        if (!__syncthreads_or(live)) break;
        Oracle::assess(A, R, live, i, n, xci, blk, r, g);
        const BatchOutcome mine = Oracle::outcome(A, R.feas, osc);
        const bool found = live && mine.what == BOUT_FEAS;  // cutting_plane_feas: a feasible point ends the loop  :217-220
        const bool best = live && (mine.what == BOUT_SHRUNK || mine.what == BOUT_FEAS);
        if constexpr (DRIVER_Q) {
            if (best) xb = blk[i];  // Q: x_best = Some(x_q), the oracle's point                                    :349
        } else {
            if (best) xb = xci;  // x_best = Some(space.xc())                                                       :303
        }
        const bool upd = live && (mine.what == BOUT_CUT || mine.what == BOUT_SHRUNK);
        const BatchOutcome its = Oracle::outcome(A, R.feas, osc_s);
        const bool lane = lane_ok && osc_s[BL_STOPPED] == 0.0 && (its.what == BOUT_CUT || its.what == BOUT_SHRUNK);
        // Q: update_q on every path                                                                       :301-307 / :352
        const int kind = DRIVER_Q ? CUT_Q : its.what == BOUT_SHRUNK ? CUT_CENTRAL : CUT_BIAS;
        const double b0 = lane ? its.b0 : 0.0;
        const double b1 = lane ? its.b1 : 0.0;
        const int hb1 = lane ? its.has_b1 : 0;
        batch_space_cut_apply<STABLE>(P, calc, upd, i, q, xci, lane, q_s, kind, b0, hb1, b1, [](int, double) {});
        if (live && i == 0) {
            if (best) osc[BL_HASBEST] = 1.0;
            bool stop;
            if (found) {
                osc[BL_STATUS] = (double)ST_SUCCESS;
                stop = true;
            } else if (!upd) {  // the oracle found nothing to cut with
                osc[BL_STATUS] = (double)ST_UNKNOWN;
                stop = true;
            } else if constexpr (DRIVER_Q) {  //                                                                    :347-371
                const double st = sc[3];
                if (best || st == (double)ST_SUCCESS) osc[Oracle::Q_RETRY] = 0.0;
                if (st == (double)ST_NOSOLN || (st == (double)ST_NOEFFECT && osc[Oracle::Q_MORE_ALT] == 0.0)) {
                    osc[BL_STATUS] = st;
                    stop = true;
                } else {
                    if (st == (double)ST_NOEFFECT) osc[Oracle::Q_RETRY] = 1.0;  // the space is as it was; tsq was written
                    osc[BL_STATUS] = (double)ST_SUCCESS;
                    if (sc[5] < R.tol) {
                        stop = true;
                    } else {
                        const double done = osc[BL_NITER] + 1.0;
                        osc[BL_NITER] = done;
                        stop = done >= (double)R.max_iters;
                    }
                }
            } else if (sc[3] != (double)ST_SUCCESS || sc[5] < R.tol) {  //                                          :308 / :222
                osc[BL_STATUS] = sc[3];
                stop = true;
            } else {
                const double done = osc[BL_NITER] + 1.0;
                osc[BL_NITER] = done;
                osc[BL_STATUS] = (double)ST_SUCCESS;
                stop = done >= (double)R.max_iters;
            }
            if (stop) {
                osc[BL_STOPPED] = 1.0;
                atomicAdd(S.nstopped, 1);
            }
        }
        __syncthreads();
    }

    if (active) {
        xc[b * n + i] = xci;
        if (osc[BL_HASBEST] != 0.0) S.xbest[b * n + i] = xb;
    }
    if (active && i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
        Oracle::store(A, b, osc, r);
        S.gamma[b] = osc[BL_GAMMA];
        S.niter[b] = (long long)osc[BL_NITER];
        S.stopped[b] = (int)osc[BL_STOPPED];
        S.has_best[b] = (int)osc[BL_HASBEST];
        S.status[b] = (int)osc[BL_STATUS];
    }
    batch_copy<T, false>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
}

}  // namespace ellhip
