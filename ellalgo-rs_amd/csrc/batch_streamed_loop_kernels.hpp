// batch_streamed_loop_kernels.hpp -- the cutting-plane loop kernel of the batched device-resident solves on a streamed batch
// handle (include/ellhip_batch_lowpass_streamed.h).
//
// k_batch_loop (batch_loop_kernels.hpp) keeps every matrix in LDS and so stops at n = 128.  Here the matrix stays in HBM as
// the streamed engine holds it (batch_streamed_kernels.hpp: [B][n][n] row-major, one workgroup per ellipsoid, thread i for
// row i, a flag per ellipsoid that says whether the matrix is symmetric to the bit) and the loop
//     oracle -> x_best -> scalar stage -> centre -> stop test -> rank-1
// runs inside the kernel for up to `iters` rounds: cutting_plane_optim (src/cutting_plane.rs:286-313) and cutting_plane_feas
// (:205-227).  The Oracle policy is the one k_batch_loop takes; the pieces of the update are the streamed engine's own
// (bs_product, bs_scalar_stage, bs_sweep, bs_sweep_mirror), so the bits are those of the CPU arithmetic and of both engines.
//
// Order inside one round.  The centre after cut k is final before the matrix sweep of cut k starts (src/ell.rs:111-115
// precedes :117-128) and the oracle reads nothing but the centre, so the oracle call of round k + 1 runs BEFORE the sweep of
// round k, and the sweep folds the product Q_new g_next along the way (bs_sweep<true>): 16 n^2 bytes of matrix traffic per
// round instead of 24 n^2.  That early call happens only when round k + 1 will run in this launch: the instance has not
// stopped and the launch has rounds left.  The oracle's cursors and gamma are state the caller reads, so it is never called
// for a round the reference would not run.
//
// Every thread of the padded block takes part in every barrier and vote (active = i < n); every loop is bounded by iters,
// the oracle's own bounds and n; no thread waits on another workgroup or on a memory word; the only atomic is the count of
// stopped instances the host polls between launches.
#pragma once

#include "batch_loop_kernels.hpp"
#include "batch_streamed_kernels.hpp"

namespace ellhip {

// doubles of LDS of one workgroup: the streamed engine's arrays, then the oracle's block (x, the loop's scalars, its own)
template <class Oracle>
__host__ __device__ inline size_t batch_streamed_loop_lds_doubles(const typename Oracle::Args& A, int n) {
    return batch_streamed_lds_doubles(n) + Oracle::lds_doubles(A, n);
}

// blockDim.x = n rounded up to a multiple of 64, one workgroup per instance, dynamic LDS = batch_streamed_loop_lds_doubles
// doubles.  One instantiation per oracle for every n: bounded for 1024 threads (128 VGPRs a wave) the low-pass loop takes 106
// VGPRs and no scratch, fewer than variants bounded for 256 and 512 threads were given (116).
template <class Oracle>
__global__ __launch_bounds__(1024) void k_batch_streamed_loop(BatchStreamedParams P, BatchLoopRun R, double* __restrict__ Q,
                                                              double* __restrict__ xc, double* __restrict__ kappa,
                                                              double* __restrict__ tsq, int* __restrict__ sym,
                                                              BatchLoopState S, typename Oracle::Args A, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, np = P.np;
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    if (!__syncthreads_or(active && S.stopped[b] == 0)) return;  // this instance has stopped

    double* gbuf = sm;  // [2][np]
    double* gt = sm + 2 * np;
    double* sg = gt + np;
    double* pr = sg + np;
    double* sc = pr + np;  // [0] rho/omega  [1] sigma/omega  [2] scale  [3] status  [4] kappa  [5] tsq  [6] symmetric
    double* blk = sm + batch_streamed_lds_doubles(n);
    double* osc = blk + Oracle::scalars_at(A, n);
    double* Qb = Q + (size_t)b * n * n;
    double* col = Qb + (active ? i : 0);

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
        sc[6] = (double)sym[b];
        osc[BL_GAMMA] = S.gamma[b];
        osc[BL_NITER] = (double)S.niter[b];
        osc[BL_STOPPED] = (double)S.stopped[b];
        osc[BL_HASBEST] = (double)S.has_best[b];
        osc[BL_STATUS] = (double)S.status[b];
    }
    __syncthreads();

    int cur = 0;            // the g buffer of this round
    bool have_g = false;    // the oracle has been called for this round already (by the round before)
    bool have_gt = false;   // acc already holds this round's gt[i], folded by the sweep of the round before
    double acc = 0.0;
    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && osc[BL_STOPPED] == 0.0;
        if (!__syncthreads_or(live)) break;
        double* g = gbuf + cur * np;
        double* gn = gbuf + (cur ^ 1) * np;
        if (!have_g) Oracle::assess(A, R, live, i, n, xci, blk, r, g);
        const BatchOutcome mine = Oracle::outcome(A, R.feas, osc);
        const bool found = mine.what == BOUT_FEAS;  // cutting_plane_feas: a feasible point ends the loop                :217-220
        const bool best = mine.what == BOUT_SHRUNK || mine.what == BOUT_FEAS;
        if (live && best) xb = xci;  // x_best = Some(space.xc())                                                        :303
        const bool upd = mine.what == BOUT_CUT || mine.what == BOUT_SHRUNK;
        const bool symm = sc[6] != 0.0;
        if (live && upd) {
            if (!have_gt) acc = symm ? bs_product(col, (size_t)n, n, g) : bs_product(Qb + (size_t)i * n, 1, n, g);  // ell.rs:102
            gt[i] = acc;
            pr[i] = g[i] * acc;
        }
        __syncthreads();
        if (live && i == 0) {
            if (upd) {
                const int kind = mine.what == BOUT_SHRUNK ? CUT_CENTRAL : CUT_BIAS;  //                                  :301-307
                (void)bs_scalar_stage(sc, pr, n, P.no_defer_trick, calc, kind, mine.b0, mine.has_b1, mine.b1);
            }
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
        const bool ok = upd && sc[3] == (double)ST_SUCCESS;  // the same for every thread
        if (live && ok) {
            xci = xci - sc[0] * gt[i];  //                                                                   src/ell.rs:113-115
            sg[i] = sc[1] * gt[i];
        }
        // the next round's oracle call, at the centre this round leaves: only for a round that will run in this launch
        const bool next = osc[BL_STOPPED] == 0.0 && it + 1 < R.iters;
        bool fuse = false;
        if (next) {
            Oracle::assess(A, R, active, i, n, xci, blk, r, gn);
            const BatchOutcome nx = Oracle::outcome(A, R.feas, osc);
            fuse = nx.what == BOUT_CUT || nx.what == BOUT_SHRUNK;  // gn holds a gradient
        } else {
            __syncthreads();  // sg
        }
        have_gt = false;
        if (ok) {
            const bool scaled = P.no_defer_trick != 0;
            const double scale = sc[2];
            if (symm) {
                if (live) {
                    if (fuse) acc = bs_sweep<true>(col, n, i, gt, sg, scaled, scale, gn);
                    else (void)bs_sweep<false>(col, n, i, gt, sg, scaled, scale, gn);
                }
                have_gt = fuse;
            } else {
                bs_sweep_mirror(Qb, n, i, live, gt, sg, scaled, scale);
                if (i == 0) sc[6] = 1.0;
            }
        }
        have_g = next;
        if (next) cur ^= 1;
        __syncthreads();
    }

    if (active) {
        xc[b * n + i] = xci;
        if (osc[BL_HASBEST] != 0.0) S.xbest[b * n + i] = xb;
    }
    if (i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
        sym[b] = sc[6] != 0.0 ? 1 : 0;
        Oracle::store(A, b, osc, r);
        S.gamma[b] = osc[BL_GAMMA];
        S.niter[b] = (long long)osc[BL_NITER];
        S.stopped[b] = (int)osc[BL_STOPPED];
        S.has_best[b] = (int)osc[BL_HASBEST];
        S.status[b] = (int)osc[BL_STATUS];
    }
}

}  // namespace ellhip
