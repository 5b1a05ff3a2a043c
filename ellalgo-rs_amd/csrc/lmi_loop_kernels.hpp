// lmi_loop_kernels.hpp -- the round-robin walk over J large LMI blocks and an objective (tests/lmi_tests.rs:142-171
// generalised to J blocks), decided on the device so that a whole batch of cutting-plane iterations can be enqueued
// without the host knowing where the walk stands.  include/ellhip_lmi_loop.h, DESIGN section 10.
//
// The host enqueues, per iteration, a fixed window of station slots that covers every cyclic walk (stations
// 0 .. S-1, then 0 .. S-2, with S = J + 1 stations when there is an objective and J without).  Per slot:
//   k_ll_gate       one thread: is this slot the walk's next station?  Writes LmiLoopState.active and the block's
//                   LmiState.skip, on which every kernel of the block's oracle call returns early (lmi_kernels.hpp)
//   (the block's oracle call, lmi_capi.inc.hpp lmi_issue)
//   k_ll_station    the block failed: its gradient and ep become the iteration's bias cut and the walk is done;
//                   it passed: the cursor moves on
//   k_ll_objective  the objective station, gate included: f0 = c.x, the cut (c, f0 - gamma) or gamma = f0
// and after the window
//   k_ll_close      nothing cut: the central cut (c, 0.0) at x_best = xc (optimisation form), or the loop halts
//                   feasible (feasibility form)
// Ordinary launches on one stream; no kernel waits for another workgroup.
#pragma once

#include "lmi_kernels.hpp"

namespace ellhip {

constexpr int LMI_LOOP_JMAX = 8;

struct LmiLoopState {
    int idx;       // the round-robin cursor: the station visited last, -1 when new
    int steps;     // stations the current walk has visited
    int done;      // the current walk has produced its cut
    int active;    // the slot being issued is the walk's station (k_ll_gate -> k_ll_station)
    int station;   // what the last walk ended on: < J a block cut, J the objective cut, J + 1 shrunk, -1 feasible
    int has_best;  // device loop: x_best holds a point
    int ran[LMI_LOOP_JMAX];  // block j ran an oracle call since the API call began
    double gamma;
};

// next station behind the cursor: `idx = if idx >= S - 1 { 0 } else { idx + 1 }` (lmi_tests.rs:150-154 with S = 3)
__device__ __forceinline__ int ll_next(int idx, int nstations) { return (idx >= nstations - 1) ? 0 : idx + 1; }

__device__ __forceinline__ int ll_is_active(const LmiLoopState* ls, const int* halted, int station, int nstations) {
    return !*halted && !ls->done && ls->steps < nstations && ll_next(ls->idx, nstations) == station;
}

__global__ __launch_bounds__(64) void k_ll_gate(LmiLoopState* __restrict__ ls, const int* __restrict__ halted,
                                                int station, int nstations, int first, LmiState* __restrict__ blk) {
    if (threadIdx.x != 0) return;
    if (first) {  // slot 0 opens the iteration's walk
        ls->steps = 0;
        ls->done = 0;
    }
    const int active = ll_is_active(ls, halted, station, nstations);
    ls->active = active;
    blk->skip = !active;
}

__global__ __launch_bounds__(64) void k_ll_station(LmiLoopState* __restrict__ ls, LmiState* __restrict__ blk,
                                                   const double* __restrict__ blk_g, long long n,
                                                   double* __restrict__ g, CutParams* __restrict__ cp, int station) {
    const int active = ls->active;
    const int p = blk->pos1;
    if (threadIdx.x == 0) blk->skip = 0;  // the block answers ellhip_lmi_assess_feas again
    if (!active) return;
    if (p)
        for (long long k = threadIdx.x; k < n; k += 64) g[k] = blk_g[k];
    if (threadIdx.x == 0) {
        ls->idx = station;
        ls->steps += 1;
        ls->ran[station] = 1;
        if (p) {  // update_bias_cut(g, ep)
            CutParams c;
            c.kind = 0;
            c.has_b1 = 0;
            c.b0 = blk->ep;
            c.b1 = 0.0;
            *cp = c;
            ls->done = 1;
            ls->station = station;
        }
    }
}

// station J of the optimisation form (lmi_tests.rs:161-167)
__global__ __launch_bounds__(64) void k_ll_objective(LmiLoopState* __restrict__ ls, const int* __restrict__ halted,
                                                     const double* __restrict__ c, const double* __restrict__ x,
                                                     long long n, double* __restrict__ g, CutParams* __restrict__ cp,
                                                     int J) {
    __shared__ int sh_cut;
    if (threadIdx.x == 0) {
        int cut = 0;
        if (ll_is_active(ls, halted, J, J + 1)) {
            double f0 = 0.0;  // a left fold from 0.0 in ascending k, product and sum rounded separately
            for (long long k = 0; k < n; ++k) f0 = f0 + c[k] * x[k];
            const double fj = f0 - ls->gamma;
            ls->idx = J;
            ls->steps += 1;
            if (fj > 0.0) {
                CutParams q;
                q.kind = 0;
                q.has_b1 = 0;
                q.b0 = fj;
                q.b1 = 0.0;
                *cp = q;
                ls->done = 1;
                ls->station = J;
                cut = 1;
            } else {
                ls->gamma = f0;
            }
        }
        sh_cut = cut;
    }
    __syncthreads();
    if (sh_cut)
        for (long long k = threadIdx.x; k < n; k += 64) g[k] = c[k];
}

// optim = 1: every station passed -> ((c, 0.0), shrunk): update_central_cut at x_best = xc (src/cutting_plane.rs:302-304)
// optim = 0: every block passed -> None: cutting_plane_feas returns (Some(xc), niter) (src/cutting_plane.rs:216-219)
// drv: the search space's DevState inside a device loop, NULL for a single call at a host point
__global__ __launch_bounds__(64) void k_ll_close(LmiLoopState* __restrict__ ls, const int* halted,
                                                 const double* __restrict__ c, const double* __restrict__ x, long long n,
                                                 double* __restrict__ g, CutParams* __restrict__ cp,
                                                 double* __restrict__ xbest, DevState* drv, int optim, int J) {
    const int stop = *halted || ls->done;
    __syncthreads();  // everyone has read `halted` before thread 0 may set it
    if (stop) return;
    if (optim)
        for (long long k = threadIdx.x; k < n; k += 64) g[k] = c[k];
    if (drv)
        for (long long k = threadIdx.x; k < n; k += 64) xbest[k] = x[k];
    if (threadIdx.x == 0) {
        if (optim) {
            CutParams q;
            q.kind = 1;
            q.has_b1 = 0;
            q.b0 = 0.0;
            q.b1 = 0.0;
            *cp = q;
            ls->station = J + 1;
            if (drv) ls->has_best = 1;
        } else {
            ls->station = -1;
            if (drv) {
                ls->has_best = 1;
                drv->halted = 1;
                drv->stop = STOP_FEASIBLE;
            }
        }
    }
}

}  // namespace ellhip
