// batch_streamed_stable_loop_kernels.hpp -- the cutting-plane loop kernel of the batched device-resident solves on a streamed
// EllStable batch handle (include/ellhip_batch_lowpass_streamed_stable.h).
//
// k_batch_streamed_loop (batch_streamed_loop_kernels.hpp) runs the loop on streamed Ell spaces; here the spaces are streamed
// EllStable buffers (batch_streamed_stable_kernels.hpp: the packed buffer in HBM, the scratch triangle turned by 180 degrees,
// one workgroup per ellipsoid, thread i for index i) and the loop
//     oracle -> x_best -> EllStable::update_core (bs_stable_cut, the code k_batch_streamed_update_stable runs) -> stop test
// runs inside the kernel for up to `iters` rounds: cutting_plane_optim (src/cutting_plane.rs:286-313) and cutting_plane_feas
// (:205-227).  The Oracle policy is the one k_batch_loop takes, so the bits are those of the CPU arithmetic and of the LDS
// engine's EllStable loop, the scratch triangle included.
//
// No fusion across rounds: the centre of round k is final only after the back solve (src/ell_stable.rs:93-104), the oracle
// of round k + 1 needs that centre, and the forward solve of round k + 1 needs both the new factor and the new gradient, so
// the early oracle call of k_batch_streamed_loop has nothing to ride on.  Every successful round moves 24 n^2 bytes.
//
// Every thread of the padded block takes part in every barrier and vote (active = i < n), also after its instance has
// stopped inside the launch; every loop is bounded by iters, the oracle's own bounds and n; no thread waits on another
// workgroup or on a memory word; the only atomic is the count of stopped instances the host polls between launches.
#pragma once

#include "batch_loop_kernels.hpp"
#include "batch_streamed_stable_kernels.hpp"

namespace ellhip {

// doubles of LDS of one workgroup: the streamed EllStable engine's arrays (w, z, gg, the scalars and the back solve's
// staging), one gradient vector, then the oracle's block (x, the loop's scalars, its own)
template <class Oracle>
__host__ __device__ inline size_t batch_streamed_stable_loop_lds_doubles(const typename Oracle::Args& A, int n) {
    return batch_streamed_stable_lds_doubles(n) + (size_t)batch_streamed_np(n) + Oracle::lds_doubles(A, n);
}

// blockDim.x = n rounded up to a multiple of 64, one workgroup per instance, dynamic LDS =
// batch_streamed_stable_loop_lds_doubles doubles.  One instantiation per oracle for every n: bounded for 1024 threads (128
// VGPRs a wave) the low-pass loop takes 109 VGPRs and no scratch with the oracle's registers, xb and the loop scalars live
// across the cut, so nothing is parked in LDS and there is no second instantiation for n <= 512.
template <class Oracle>
__global__ __launch_bounds__(1024) void k_batch_streamed_loop_stable(BatchStreamedParams P, BatchLoopRun R,
                                                                     double* __restrict__ Q, double* __restrict__ xc,
                                                                     double* __restrict__ kappa, double* __restrict__ tsq,
                                                                     BatchLoopState S, typename Oracle::Args A,
                                                                     EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, np = P.np;
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    if (!__syncthreads_or(active && S.stopped[b] == 0)) return;  // this instance has stopped

    double* w = sm;
    double* z = w + np;
    double* gg = z + np;
    double* sc = gg + np;  // as in k_batch_streamed_update_stable: [0] rho/omega  [3] status  [4] kappa  [5] tsq  [8..71]
    double* g = sm + batch_streamed_stable_lds_doubles(n);
    double* blk = g + np;
    double* osc = blk + Oracle::scalars_at(A, n);
    double* Qb = Q + (size_t)b * n * n;

    double xci = 0.0, xb = 0.0;
    typename Oracle::Regs r;
    if (active) {
        xci = xc[b * n + i];
        xb = S.xbest[b * n + i];
    }
    Oracle::load(A, active, b, i, n, blk, r);
    if (i == 0) {
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

    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && osc[BL_STOPPED] == 0.0;
        if (!__syncthreads_or(live)) break;
        Oracle::assess(A, R, live, i, n, xci, blk, r, g);
        const BatchOutcome mine = Oracle::outcome(A, R.feas, osc);
        const bool found = mine.what == BOUT_FEAS;  // cutting_plane_feas: a feasible point ends the loop                :217-220
        const bool best = mine.what == BOUT_SHRUNK || mine.what == BOUT_FEAS;
        if (live && best) xb = xci;  // x_best = Some(space.xc())                                                        :303
        const bool upd = mine.what == BOUT_CUT || mine.what == BOUT_SHRUNK;  // the same for every thread
        if (upd) {
            const double gi = live ? g[i] : 0.0;
            const int kind = mine.what == BOUT_SHRUNK ? CUT_CENTRAL : CUT_BIAS;  //                                      :301-307
            // a failed cut changes tsq and the scratch triangle only, as the CPU EllStable does
            bs_stable_cut(Qb, n, i, live, gi, w, z, gg, sc, xci, calc, kind, mine.b0, mine.has_b1, mine.b1,
                          [](const int, const double) {});
        }
        if (live && i == 0) {
            if (best) osc[BL_HASBEST] = 1.0;
            bool stop;
            if (found) {
                osc[BL_STATUS] = (double)ST_SUCCESS;
                stop = true;
            } else if (!upd) {  // the oracle found nothing to cut with
                osc[BL_STATUS] = (double)ST_UNKNOWN;
                stop = true;
            } else if (sc[3] != (double)ST_SUCCESS || sc[5] < R.tol) {  //                                               :308 / :222
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
    if (i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
        Oracle::store(A, b, osc, r);
        S.gamma[b] = osc[BL_GAMMA];
        S.niter[b] = (long long)osc[BL_NITER];
        S.stopped[b] = (int)osc[BL_STOPPED];
        S.has_best[b] = (int)osc[BL_HASBEST];
        S.status[b] = (int)osc[BL_STATUS];
    }
}

}  // namespace ellhip
