// batch_linfeas_streamed_kernels.hpp -- bsearch over BSearchAdaptor (src/cutting_plane.rs:403-419, :441-466) on streamed batch
// handles, n <= 1024 (include/ellhip_batch_bsearch_streamed.h): k_batch_streamed_bsearch for streamed
// Ell spaces and k_batch_streamed_bsearch_stable for streamed EllStable ones, and the one-workgroup-per-problem form of the
// oracle's assess_feas.
//
// The two kernels are siblings of k_batch_bsearch (batch_linfeas_kernels.hpp) as k_batch_streamed_loop and
// k_batch_streamed_loop_stable are siblings of k_batch_loop: the launch shape is the streamed engines' (one workgroup per
// problem, thread i for row i, n rounded up to 64 threads), the oracle policy with its update(osc, gamma) hook, the outer step
// (batch_bs_outer_step), BatchBsRun, the BS_* state and the probe buffers are k_batch_bsearch's, and the update arithmetic is
// the streamed engines' own (bs_product, bs_scalar_stage, the sweeps; bs_stable_cut), so the bits are those of the CPU
// restatement.
//
// The clone (:410).  The adaptor's matrix lives in HBM and is read-only here; the probe's matrix lives in the probe buffer
// W.Q.  BSS_OWN says which of the two the probe reads; it is cleared when a probe ends and carried across launches.
//   Ell        A probe reads the ADAPTOR's matrix (with its sym flag) for its products until its first successful cut.  That
//              cut's sweep reads the adaptor's matrix and writes the probe buffer (bs_sweep_to, bs_sweep_mirror_to), and
//              from then on the probe owns a matrix that is symmetric to the bit.  So a probe that is feasible at once, or
//              whose first cut fails, moves no matrix bytes for the clone, and a probe of K successful cuts moves what K cuts
//              move in k_batch_streamed_loop.  The round order is that kernel's: the oracle call of round k + 1 comes before
//              the sweep of round k and its product rides on the sweep, only when the probe goes on and the launch has
//              rounds left (the cursor is state the caller reads).  The sweep of a probe's last cut is skipped: nothing reads
//              a finished probe's matrix.
//   EllStable  bs_stable_cut writes the scratch triangle even when the cut fails, so the packed buffer is copied adaptor ->
//              probe buffer by the whole workgroup, coalesced, right before the probe's first cut; not at all for a probe
//              that is feasible at once.  No fusion across rounds.
// xc, kappa and tsq are cloned at the probe's first round; set_xc (:414) writes the adaptor's centre; the adaptor's matrix,
// kappa, tsq and sym flag are never written.
//
// Every thread of the padded block takes part in every barrier and vote (active = i < n); every loop is bounded by the
// launch's rounds, J, n or max_iters; no thread waits on another workgroup or on a memory word; the only global atomic is
// the stopped count.
#pragma once

#include "batch_linfeas_kernels.hpp"
#include "batch_streamed_loop_kernels.hpp"
#include "batch_streamed_stable_loop_kernels.hpp"

namespace ellhip {

constexpr int BATCH_LINFEAS_STREAMED_JMAX = 4096;

// the streamed kernels' state record: the BS_* words, then their own
enum : int {
    BSS_OWN = BS_N,  // 1.0: the probe's matrix is in the probe buffer; 0.0: it is still the adaptor's
    BSS_N = 17,
};

// bs_sweep out of place: column i of `src` (symmetric to the bit, read-only) updated into column i of `dst`.
template <bool FUSE>
__device__ __forceinline__ double bs_sweep_to(const double* __restrict__ src, double* __restrict__ dst, const int n,
                                              const int i, const double* gt, const double* sg, const bool scaled,
                                              const double scale, const double* gn) {
    const double gti = gt[i], sgi = sg[i];
    double acc = 0.0;
    auto one = [&](const int a, const double q) {
        const bool low = a <= i;
        const double m1 = low ? sgi : sg[a];   // sigma/omega * gt[max]                                     src/ell.rs:117
        const double m2 = low ? gt[a] : gti;   // gt[min]
        double v = q - m1 * m2;                //                                                           :121
        if (scaled) v = v * scale;             //                                                           :132-135
        dst[(size_t)a * n] = v;
        if (FUSE) acc += v * gn[a];
    };
    int a = 0;
    for (; a + 8 <= n; a += 8) {
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = src[(size_t)(a + u) * n];
#pragma unroll
        for (int u = 0; u < 8; ++u) one(a + u, q[u]);
    }
    for (; a < n; ++a) one(a, src[(size_t)a * n]);
    return acc;
}

// bs_sweep_mirror out of place: the lower triangle and the diagonal of `Qs` updated into `Qd`, then Qd's upper triangle is
// the mirror image of Qd's lower one.  Collective: one barrier inside.
__device__ __forceinline__ void bs_sweep_mirror_to(const double* __restrict__ Qs, double* __restrict__ Qd, const int n,
                                                   const int i, const bool active, const double* gt, const double* sg,
                                                   const bool scaled, const double scale) {
    const int ia = active ? i : 0;
    if (active) {
        const double gti = gt[i];
        for (int r = i; r < n; ++r) {
            double v = Qs[(size_t)r * n + ia] - sg[r] * gti;
            if (scaled) v = v * scale;
            Qd[(size_t)r * n + ia] = v;
        }
    }
    __syncthreads();  // the workgroup's own stores to Qd are visible to its loads after the barrier
    if (active) {
        const double* row = Qd + (size_t)i * n;
        for (int r = 0; r < i; ++r) Qd[(size_t)r * n + ia] = row[r];
    }
}

// One round's bookkeeping on thread 0 after the cut: how the probe goes on or ends, then the outer step.  Shared by the two
// kernels below; the same statements as in k_batch_bsearch.
template <class Oracle>
__device__ __forceinline__ void batch_bss_round_end(const BatchBsRun& R, double* bs, double* osc, const double* sc,
                                                    const bool found, const bool upd, int* nstopped) {
    bs[BS_ROUNDS] += 1.0;
    int end = -1;
    if (found) {
        end = 0;
    } else if (!upd) {  // (an oracle of this driver always answers)
        end = 1;
    } else if (sc[3] != (double)ST_SUCCESS) {  //                                                                  :222
        end = 1;
    } else if (sc[5] < R.inner_tol) {
        end = 2;
    } else {
        const double done = bs[BS_INNER] + 1.0;
        bs[BS_INNER] = done;
        if (done >= (double)R.inner_max_iters) end = 3;  //                                                        :226
    }
    if (end < 0) {
        bs[BS_CLONE] = 0.0;
        bs[BSS_OWN] = 1.0;  // a successful cut has written the probe buffer (Ell: its sweep follows in this round)
    } else {
        bs[BS_END + end] += 1.0;
        if (end == 0) bs[BS_UPPER] = bs[BS_GAMMA];  //                                                             :460
        else bs[BS_LOWER] = bs[BS_GAMMA];           //                                                             :462
        bs[BS_OUTER] += 1.0;
        bs[BS_INNER] = -1.0;
        bs[BSS_OWN] = 0.0;
        batch_bs_outer_step<Oracle>(R, bs, osc, nstopped);
    }
}

template <class Oracle>
__host__ __device__ inline size_t batch_streamed_bsearch_lds_doubles(const typename Oracle::Args& A, int n, bool stable) {
    return (stable ? batch_streamed_stable_loop_lds_doubles<Oracle>(A, n) : batch_streamed_loop_lds_doubles<Oracle>(A, n)) + BSS_N;
}

// Qa, ka, ta, syma: the adaptor's space, read only; xca: its centre, written by set_xc.  W: the probe's space and the
// bisection state ([B][BSS_N]) between launches.  blockDim.x = n rounded up to a multiple of 64, one workgroup per problem,
// dynamic LDS = batch_streamed_bsearch_lds_doubles(A, n, false) doubles.
template <class Oracle>
__global__ __launch_bounds__(1024) void k_batch_streamed_bsearch(BatchStreamedParams P, BatchBsRun R,
                                                                 const double* __restrict__ Qa, double* __restrict__ xca,
                                                                 const double* __restrict__ ka, const double* __restrict__ ta,
                                                                 const int* __restrict__ syma, BatchBsBuffers W,
                                                                 typename Oracle::Args A, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, np = P.np;
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    if (!__syncthreads_or(active && W.state[b * BSS_N + BS_STOPPED] == 0.0)) return;  // this problem's search has stopped

    double* gbuf = sm;  // [2][np]
    double* gt = sm + 2 * np;
    double* sg = gt + np;
    double* pr = sg + np;
    double* sc = pr + np;  // [0] rho/omega  [1] sigma/omega  [2] scale  [3] status  [4] kappa  [5] tsq  [6] the adaptor's sym
    double* blk = sm + batch_streamed_lds_doubles(n);
    double* osc = blk + Oracle::scalars_at(A, n);
    double* bs = blk + Oracle::lds_doubles(A, n);
    const int ia = active ? i : 0;
    const double* Qab = Qa + (size_t)b * n * n;
    double* Qpb = W.Q + (size_t)b * n * n;

    double xci = 0.0;
    typename Oracle::Regs r;
    if (active) xci = W.xc[b * n + i];
    Oracle::load(A, active, b, i, n, blk, r);
    if (i == 0) {
        sc[3] = (double)ST_SUCCESS;
        sc[4] = W.kappa[b];
        sc[5] = W.tsq[b];
        sc[6] = (double)syma[b];
        for (int k = 0; k < BSS_N; ++k) bs[k] = W.state[b * BSS_N + k];
        osc[BL_STOPPED] = 0.0;
        if (bs[BS_STOPPED] == 0.0 && bs[BS_INNER] < 0.0)  // a call begins between two probes
            batch_bs_outer_step<Oracle>(R, bs, osc, W.nstopped);
    }
    __syncthreads();

    const BatchLoopRun RL{R.iters, 1, R.inner_max_iters, R.inner_tol};
    int cur = 0;           // the g buffer of this round
    bool have_g = false;   // the oracle has been called for this round already (by the round before)
    bool have_gt = false;  // acc already holds this round's gt[i], folded by the sweep of the round before
    double acc = 0.0;
    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && bs[BS_STOPPED] == 0.0;  // not stopped: in a probe
        if (!__syncthreads_or(live)) break;
        double* g = gbuf + cur * np;
        double* gn = gbuf + (cur ^ 1) * np;
        if (!have_g) {
            if (bs[BS_CLONE] != 0.0) {  // let mut space = self.space.clone(): the centre and the scalars        :410
                if (active) xci = xca[b * n + i];
                if (i == 0) {
                    sc[4] = ka[b];
                    sc[5] = ta[b];
                }
            }
            Oracle::assess(A, RL, live, i, n, xci, blk, r, g);
        }
        const BatchOutcome mine = Oracle::outcome(A, 1, osc);
        const bool found = mine.what == BOUT_FEAS;  //                                                         :217-220
        const bool upd = mine.what == BOUT_CUT;
        const bool own = bs[BSS_OWN] != 0.0;
        const bool symm = own || sc[6] != 0.0;
        const double* Qr = own ? Qpb : Qab;  // the probe's matrix
        if (live && upd) {
            if (!have_gt) acc = symm ? bs_product(Qr + ia, (size_t)n, n, g) : bs_product(Qr + (size_t)ia * n, 1, n, g);
            gt[i] = acc;
            pr[i] = g[i] * acc;
        }
        if (live && found) xca[b * n + i] = xci;  // self.space.set_xc(x)                                          :414
        __syncthreads();
        if (live && i == 0) {
            if (upd) (void)bs_scalar_stage(sc, pr, n, P.no_defer_trick, calc, CUT_BIAS, mine.b0, 0, 0.0);
            batch_bss_round_end<Oracle>(R, bs, osc, sc, found, upd, W.nstopped);
        }
        __syncthreads();
        const bool goon = bs[BS_STOPPED] == 0.0 && bs[BS_CLONE] == 0.0;  // the probe goes on: its cut succeeded
        if (live && goon) {
            xci = xci - sc[0] * gt[i];  //                                                               src/ell.rs:113-115
            sg[i] = sc[1] * gt[i];
        }
        // the next round's oracle call, at the centre this round leaves: only for a round of this probe in this launch
        const bool next = goon && it + 1 < R.iters;
        bool fuse = false;
        if (next) {
            Oracle::assess(A, RL, active, i, n, xci, blk, r, gn);
            fuse = Oracle::outcome(A, 1, osc).what == BOUT_CUT;  // gn holds a gradient
        } else {
            __syncthreads();  // sg
        }
        have_gt = false;
        if (goon) {  // (the sweep of a probe's last cut is skipped)
            const bool scaled = P.no_defer_trick != 0;
            const double scale = sc[2];
            if (symm) {
                if (live) {
                    if (own) {
                        if (fuse) acc = bs_sweep<true>(Qpb + ia, n, i, gt, sg, scaled, scale, gn);
                        else (void)bs_sweep<false>(Qpb + ia, n, i, gt, sg, scaled, scale, gn);
                    } else {
                        if (fuse) acc = bs_sweep_to<true>(Qab + ia, Qpb + ia, n, i, gt, sg, scaled, scale, gn);
                        else (void)bs_sweep_to<false>(Qab + ia, Qpb + ia, n, i, gt, sg, scaled, scale, gn);
                    }
                }
                have_gt = fuse;
            } else {
                bs_sweep_mirror_to(Qab, Qpb, n, i, live, gt, sg, scaled, scale);
            }
        }
        have_g = next;
        if (next) cur ^= 1;
        __syncthreads();
    }

    if (active) W.xc[b * n + i] = xci;
    if (i == 0) {
        W.kappa[b] = sc[4];
        W.tsq[b] = sc[5];
        Oracle::store(A, b, osc, r);
        for (int k = 0; k < BSS_N; ++k) W.state[b * BSS_N + k] = bs[k];
    }
}

// The same on streamed EllStable spaces.  Dynamic LDS = batch_streamed_bsearch_lds_doubles(A, n, true) doubles.
template <class Oracle>
__global__ __launch_bounds__(1024) void k_batch_streamed_bsearch_stable(BatchStreamedParams P, BatchBsRun R,
                                                                        const double* __restrict__ Qa,
                                                                        double* __restrict__ xca,
                                                                        const double* __restrict__ ka,
                                                                        const double* __restrict__ ta, BatchBsBuffers W,
                                                                        typename Oracle::Args A, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, np = P.np;
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    if (!__syncthreads_or(active && W.state[b * BSS_N + BS_STOPPED] == 0.0)) return;  // this problem's search has stopped

    double* w = sm;
    double* z = w + np;
    double* gg = z + np;
    double* sc = gg + np;  // as in k_batch_streamed_update_stable: [0] rho/omega  [3] status  [4] kappa  [5] tsq  [8..71]
    double* g = sm + batch_streamed_stable_lds_doubles(n);
    double* blk = g + np;
    double* osc = blk + Oracle::scalars_at(A, n);
    double* bs = blk + Oracle::lds_doubles(A, n);
    const double* Qab = Qa + (size_t)b * n * n;
    double* Qpb = W.Q + (size_t)b * n * n;

    double xci = 0.0;
    typename Oracle::Regs r;
    if (active) xci = W.xc[b * n + i];
    Oracle::load(A, active, b, i, n, blk, r);
    if (i == 0) {
        sc[3] = (double)ST_SUCCESS;
        sc[4] = W.kappa[b];
        sc[5] = W.tsq[b];
        for (int k = 0; k < BSS_N; ++k) bs[k] = W.state[b * BSS_N + k];
        osc[BL_STOPPED] = 0.0;
        if (bs[BS_STOPPED] == 0.0 && bs[BS_INNER] < 0.0)  // a call begins between two probes
            batch_bs_outer_step<Oracle>(R, bs, osc, W.nstopped);
    }
    __syncthreads();

    const BatchLoopRun RL{R.iters, 1, R.inner_max_iters, R.inner_tol};
    const int nn = n * n;  // (n <= 1024)
    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && bs[BS_STOPPED] == 0.0;  // not stopped: in a probe
        if (!__syncthreads_or(live)) break;
        if (bs[BS_CLONE] != 0.0) {  // let mut space = self.space.clone(): the centre and the scalars             :410
            if (active) xci = xca[b * n + i];
            if (i == 0) {
                sc[4] = ka[b];
                sc[5] = ta[b];
            }
        }
        Oracle::assess(A, RL, live, i, n, xci, blk, r, g);
        const BatchOutcome mine = Oracle::outcome(A, 1, osc);
        const bool found = mine.what == BOUT_FEAS;  //                                                         :217-220
        const bool upd = mine.what == BOUT_CUT;     // the same for every thread
        if (upd) {
            if (bs[BSS_OWN] == 0.0) {  // the clone's packed buffer, right before the probe's first cut
                for (int k = i; k < nn; k += (int)blockDim.x) Qpb[k] = Qab[k];
                __syncthreads();  // the workgroup's own stores to Qpb are visible to its loads after the barrier
            }
            const double gi = live ? g[i] : 0.0;
            // a failed cut changes tsq and the scratch triangle only, as the CPU EllStable does
            bs_stable_cut(Qpb, n, i, live, gi, w, z, gg, sc, xci, calc, CUT_BIAS, mine.b0, 0, 0.0, [](const int, const double) {});
        }
        if (live && found) xca[b * n + i] = xci;  // self.space.set_xc(x)                                          :414
        if (live && i == 0) batch_bss_round_end<Oracle>(R, bs, osc, sc, found, upd, W.nstopped);
        __syncthreads();
    }

    if (active) W.xc[b * n + i] = xci;
    if (i == 0) {
        W.kappa[b] = sc[4];
        W.tsq[b] = sc[5];
        Oracle::store(A, b, osc, r);
        for (int k = 0; k < BSS_N; ++k) W.state[b * BSS_N + k] = bs[k];
    }
}

// One assess_feas per problem at x[B][n] for n past the LDS engines' block: one workgroup per problem, n rounded up to 64
// threads, the device function k_batch_linfeas_assess runs.  Dynamic LDS = lds_doubles(A, n) + n doubles.
__global__ __launch_bounds__(1024) void k_batch_linfeas_assess_wg(int n, BatchLinFeasOracle::Args A,
                                                                  const double* __restrict__ x, double* __restrict__ grad_out,
                                                                  double* __restrict__ beta_out, int* __restrict__ cut_out) {
    extern __shared__ double sm[];
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    double* blk = sm;
    double* osc = blk + BatchLinFeasOracle::scalars_at(A, n);
    double* g = blk + BatchLinFeasOracle::lds_doubles(A, n);
    BatchLinFeasOracle::Regs r;
    BatchLinFeasOracle::load(A, active, b, i, n, blk, r);
    const double xi = active ? x[b * n + i] : 0.0;
    BatchLoopRun R{1, 1, 1, 0.0};
    BatchLinFeasOracle::assess(A, R, active, i, n, xi, blk, r, g);  // (its first barrier orders load's scalars)
    if (active) grad_out[b * n + i] = g[i];
    if (i == 0) {
        const bool feas = osc[LF_FEAS] != 0.0;
        beta_out[b] = osc[LF_B0];
        cut_out[b] = feas ? -1 : (int)osc[LF_IDX];
        BatchLinFeasOracle::store(A, b, osc, r);
    }
}

}  // namespace ellhip
