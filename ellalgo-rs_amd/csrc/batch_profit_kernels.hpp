// batch_profit_kernels.hpp -- the oracles of B independent profit-maximisation problems (two variables each) as one policy of
// the loop kernel (include/ellhip_batch_profit.h; the loop: batch_loop_kernels.hpp), and ell_exp / ell_log
// over an array (k_math_eval).
//
// Three kinds, a per-handle constant (Args::kind) except that the discrete one is the policy's template argument, because it
// is the one that runs under the optim_q driver and hands out x_q, more_alt and retry:
//     plain     ProfitOracle::assess_optim                     src/oracles/profit_oracle.rs:35-78
//     robust    ProfitRbOracle::assess_optim: a[i] -+ uie[i] by the sign of y[i], then the plain oracle with the
//               constructor's shifted parameters               :111-125
//     discrete  ProfitOracleQ::assess_optim_q                  :145-162
// Every operation is taken in the reference's order, exp and log are ell_exp and ell_log (ell_math.hpp), and the file is
// compiled with -ffp-contract=off, so cuts, gamma and with them the whole loop are bit-identical to the CPU restatement that
// uses the same two functions (tests/batch_profit_reference.py).
//
// Work split.  n = 2: an instance has two threads.  Thread i takes ell_exp of coordinate i of the point the oracle will be
// asked at -- the centre y, or yd on a retry -- and leaves it in LDS; after one barrier thread 0 of the instance (its scalar
// lane) does the rest: the cursor, the constraints, ell_log(gamma + vx), ell_exp(log_cobb) when feasible and, in the discrete
// kind's feasible round, the rounding, two ell_log for yd and two more ell_exp at yd.  Those two are the only exps the scalar
// lane takes that the two threads could have shared; sharing them would cost a second barrier pair in every round of every
// kind, and they occur in the discrete kind's feasible rounds only.  exp(y) is taken whether or not the cursor reaches
// constraint 1 in this call: the lanes of a wave run in lockstep, so a lane that skipped it would wait for its neighbours.
//
// Barriers are workgroup-wide; threads that take no part (live = false) skip the loads and stores and take part in every
// barrier.  There is no loop here other than the two constraints; no thread waits on another workgroup or on a memory word.
#pragma once

#include <math.h>

#include "batch_loop_kernels.hpp"
#include "ell_math.hpp"

namespace ellhip {

enum : int { PROFIT_PLAIN = 0, PROFIT_ROBUST = 1, PROFIT_DISCRETE = 2 };

// an instance's constants in HBM: [B][PF_NCONST]
enum : int {
    PFC_LOG_P_SCALE = 0,  // ell_log(p A), the robust kind's from the shifted p
    PFC_LOG_K = 1,        // ell_log(k)
    PFC_PRICE = 2,        // price_out[2], the robust kind's shifted by e5
    PFC_A = 4,            // elasticities[2]
    PFC_UIE = 6,          // the robust kind's uie[2]
    PF_NCONST = 8,
};

// an instance's LDS block: the point (on return x_q), the exps, yd, then the scalars
enum : int { PFL_X = 0, PFL_EXP = 2, PFL_YD = 4, PFL_SCALARS = 6 };
// oracle scalars, after the loop's own (batch_loop_kernels.hpp)
enum : int {
    PF_GAMMA = BL_GAMMA,
    PF_B0 = 5,        // the cut's beta
    PF_SHRUNK = 6,    // 1.0: gamma improved
    PF_RETRY = 7,     // optim_q: the driver's retry flag, read by the oracle, written by the driver
    PF_MORE_ALT = 8,  // optim_q: 1.0 while the oracle has another cut to offer
    PF_IDX = 9,       // the constraint cursor
    PF_CONST = 10,    // the PF_NCONST constants
    BATCH_PROFIT_SCALARS = PF_CONST + PF_NCONST,
};
static_assert(PF_B0 == BL_SCALARS, "the oracle's scalars follow the loop's");

__host__ __device__ inline size_t batch_profit_lds_doubles() { return (size_t)(PFL_SCALARS + BATCH_PROFIT_SCALARS) | 1; }

struct ProfitCut {
    double g0, g1, beta;
    bool shrunk;
};

// what assess_feas leaves in the oracle for assess_optim (:13-15)
struct ProfitWork {
    double log_cobb, vx, q0, q1;
};

// ProfitOracle::assess_feas at p with ep = exp(p), elasticities (a0, a1) (:35-65); true: a cut was found
__device__ __forceinline__ bool batch_profit_feas(const double* cst, const double a0, const double a1, const double p0,
                                                  const double p1, const double ep0, const double ep1, const double gamma,
                                                  int& idx, ProfitWork& w, ProfitCut& c) {
    for (int t = 0; t < 2; ++t) {
        idx += 1;
        if (idx == 2) idx = 0;
        double fj;
        if (idx == 0) {
            fj = p0 - cst[PFC_LOG_K];
        } else {
            w.log_cobb = cst[PFC_LOG_P_SCALE] + ((0.0 + a0 * p0) + a1 * p1);
            w.q0 = cst[PFC_PRICE] * ep0;
            w.q1 = cst[PFC_PRICE + 1] * ep1;
            w.vx = w.q0 + w.q1;
            fj = ell_log(gamma + w.vx) - w.log_cobb;
        }
        if (fj > 0.0) {
            if (idx == 0) {
                c.g0 = 1.0;
                c.g1 = 0.0;
            } else {
                const double den = gamma + w.vx;
                c.g0 = w.q0 / den - a0;
                c.g1 = w.q1 / den - a1;
            }
            c.beta = fj;
            c.shrunk = false;
            return true;
        }
    }
    return false;
}

// ProfitOracle::assess_optim (:70-78)
__device__ __forceinline__ void batch_profit_optim(const double* cst, const double a0, const double a1, const double p0,
                                                   const double p1, const double ep0, const double ep1, double& gamma,
                                                   int& idx, ProfitCut& c) {
    ProfitWork w{0.0, 0.0, 0.0, 0.0};
    if (batch_profit_feas(cst, a0, a1, p0, p1, ep0, ep1, gamma, idx, w, c)) return;
    const double exp_val = ell_exp(w.log_cobb);
    gamma = exp_val - w.vx;
    c.g0 = w.q0 / exp_val - a0;
    c.g1 = w.q1 / exp_val - a1;
    c.beta = 0.0;
    c.shrunk = true;
}

// One oracle call for the workgroup's instances, collectively (it contains barriers: every thread of the workgroup calls it).
// blk: the instance's LDS block, blk[PFL_X + i] = the centre on entry; osc = blk + PFL_SCALARS with gamma, the cursor, the
// constants and (Q) retry; blk[PFL_YD ..] = yd (Q).  On return (after a barrier) gout is the gradient, osc[PF_B0] beta,
// osc[PF_SHRUNK], osc[PF_GAMMA], osc[PF_IDX] and, Q, blk[PFL_X ..] = x_q, osc[PF_MORE_ALT] and yd.
template <bool Q>
__device__ __forceinline__ void batch_profit_oracle(const int kind, const bool live, const int i, const double xci,
                                                    double* blk, double* gout) {
    double* osc = blk + PFL_SCALARS;
    if (live) {
        const bool retry = Q && osc[PF_RETRY] != 0.0;
        blk[PFL_X + i] = xci;
        blk[PFL_EXP + i] = ell_exp(retry ? blk[PFL_YD + i] : xci);
    }
    __syncthreads();
    if (live && i == 0) {
        const double* cst = osc + PF_CONST;
        const double y0 = blk[PFL_X], y1 = blk[PFL_X + 1];
        double gamma = osc[PF_GAMMA];
        int idx = (int)osc[PF_IDX];
        double a0 = cst[PFC_A], a1 = cst[PFC_A + 1];
        if (kind == PROFIT_ROBUST) {  //                                                        :115-123
            a0 = a0 + (y0 > 0.0 ? -cst[PFC_UIE] : cst[PFC_UIE]);
            a1 = a1 + (y1 > 0.0 ? -cst[PFC_UIE + 1] : cst[PFC_UIE + 1]);
        }
        ProfitCut c{0.0, 0.0, 0.0, false};
        if constexpr (!Q) {
            batch_profit_optim(cst, a0, a1, y0, y1, blk[PFL_EXP], blk[PFL_EXP + 1], gamma, idx, c);
        } else {
            const bool retry = osc[PF_RETRY] != 0.0;
            bool at_y = false;
            double e0 = blk[PFL_EXP], e1 = blk[PFL_EXP + 1];  // exp(yd) on a retry
            if (!retry) {  //                                                                   :146-158
                ProfitWork w{0.0, 0.0, 0.0, 0.0};
                at_y = batch_profit_feas(cst, a0, a1, y0, y1, e0, e1, gamma, idx, w, c);
                if (!at_y) {
                    double d0 = round(e0), d1 = round(e1);  // half away from zero, as f64::round
                    if (d0 == 0.0) d0 = 1.0;
                    if (d1 == 0.0) d1 = 1.0;
                    const double yd0 = ell_log(d0), yd1 = ell_log(d1);
                    blk[PFL_YD] = yd0;
                    blk[PFL_YD + 1] = yd1;
                    e0 = ell_exp(yd0);
                    e1 = ell_exp(yd1);
                }
            }
            if (!at_y) {  //                                                                    :159-161
                const double yd0 = blk[PFL_YD], yd1 = blk[PFL_YD + 1];
                batch_profit_optim(cst, a0, a1, yd0, yd1, e0, e1, gamma, idx, c);
                c.beta = c.beta + ((0.0 + c.g0 * (yd0 - y0)) + c.g1 * (yd1 - y1));
                blk[PFL_X] = yd0;
                blk[PFL_X + 1] = yd1;
            }
            osc[PF_MORE_ALT] = retry ? 0.0 : 1.0;
        }
        gout[0] = c.g0;
        gout[1] = c.g1;
        osc[PF_B0] = c.beta;
        osc[PF_SHRUNK] = c.shrunk ? 1.0 : 0.0;
        osc[PF_GAMMA] = gamma;
        osc[PF_IDX] = (double)idx;
    }
    __syncthreads();
}

// The oracle as the loop kernel's policy (batch_loop_kernels.hpp).  Per instance in HBM: the constants, the cursor and, Q, yd
// and the driver's retry flag, so that a chunk boundary may fall between a NoEffect and its retry.
template <bool Q>
struct BatchProfitOracle {
    struct Args {
        const double* cst;  // [B][PF_NCONST]
        int* idx;           // [B]
        double* yd;         // [B][2]
        int* retry;         // [B]
        int kind;
    };
    struct Regs {};
    static constexpr int Q_RETRY = PF_RETRY, Q_MORE_ALT = PF_MORE_ALT;  // where the optim_q driver finds its two flags
    static __host__ __device__ inline size_t lds_doubles(const Args&, int) { return batch_profit_lds_doubles(); }
    static __host__ __device__ __forceinline__ size_t scalars_at(const Args&, int) { return PFL_SCALARS; }
    static __device__ __forceinline__ void load(const Args& A, bool active, long long b, int i, int, double* blk, Regs&) {
        if (active && i == 0) {
            double* osc = blk + PFL_SCALARS;
            osc[PF_B0] = 0.0;
            osc[PF_SHRUNK] = 0.0;
            osc[PF_RETRY] = Q ? (double)A.retry[b] : 0.0;
            osc[PF_MORE_ALT] = 0.0;
            osc[PF_IDX] = (double)A.idx[b];
            for (int c = 0; c < PF_NCONST; ++c) osc[PF_CONST + c] = A.cst[b * PF_NCONST + c];
            blk[PFL_YD] = Q ? A.yd[2 * b] : 0.0;
            blk[PFL_YD + 1] = Q ? A.yd[2 * b + 1] : 0.0;
        }
    }
    static __device__ __forceinline__ void assess(const Args& A, const BatchLoopRun&, bool live, int i, int, double xci,
                                                  double* blk, Regs&, double* g) {
        batch_profit_oracle<Q>(A.kind, live, i, xci, blk, g);
    }
    static __device__ __forceinline__ BatchOutcome outcome(const Args&, int, const double* osc) {
        return BatchOutcome{osc[PF_SHRUNK] != 0.0 ? BOUT_SHRUNK : BOUT_CUT, osc[PF_B0], 0, 0.0};
    }
    static __device__ __forceinline__ void store(const Args& A, long long b, const double* osc, const Regs&) {
        A.idx[b] = (int)osc[PF_IDX];
        if (Q) {
            const double* blk = osc - PFL_SCALARS;
            A.yd[2 * b] = blk[PFL_YD];
            A.yd[2 * b + 1] = blk[PFL_YD + 1];
            A.retry[b] = (int)osc[PF_RETRY];
        }
    }
};

// One oracle call per instance at x[B][2] with gamma[B]: the same device function, without an ellipsoid.  128 instances of
// two threads in a workgroup of 256.  Q: retry_in[B] is the caller's, and x_q and more_alt are handed out; the cursor and yd
// are read from and written to the handle either way.
template <bool Q>
__global__ __launch_bounds__(256) void k_batch_profit_assess(long long B, typename BatchProfitOracle<Q>::Args A,
                                                             const double* __restrict__ x, double* __restrict__ gamma,
                                                             const int* __restrict__ retry_in, double* __restrict__ grad_out,
                                                             double* __restrict__ beta_out, int* __restrict__ shrunk_out,
                                                             double* __restrict__ xq_out, int* __restrict__ more_out) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid >> 1, i = tid & 1;
    const long long b = (long long)blockIdx.x * (blockDim.x >> 1) + e;
    const bool active = b < B;
    const size_t lper = batch_profit_lds_doubles() + 2;
    double* blk = sm + (size_t)e * lper;
    double* osc = blk + PFL_SCALARS;
    double* g = blk + batch_profit_lds_doubles();
    typename BatchProfitOracle<Q>::Regs r;
    BatchProfitOracle<Q>::load(A, active, b, i, 2, blk, r);
    double xi = 0.0;
    if (active) {
        xi = x[2 * b + i];
        if (i == 0) {
            osc[PF_GAMMA] = gamma[b];
            if (Q) osc[PF_RETRY] = retry_in[b] != 0 ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    batch_profit_oracle<Q>(A.kind, active, i, xi, blk, g);
    if (active) {
        grad_out[2 * b + i] = g[i];
        if (Q) xq_out[2 * b + i] = blk[PFL_X + i];
    }
    if (active && i == 0) {
        gamma[b] = osc[PF_GAMMA];
        beta_out[b] = osc[PF_B0];
        shrunk_out[b] = osc[PF_SHRUNK] != 0.0;
        if (Q) more_out[b] = osc[PF_MORE_ALT] != 0.0;
        BatchProfitOracle<Q>::store(A, b, osc, r);  // (the retry flag it keeps is zeroed when a loop begins)
    }
}

// out[j] = ell_exp(x[j]) (fn = 0) or ell_log(x[j]) (fn = 1); grid-stride
__global__ __launch_bounds__(256) void k_math_eval(int fn, long long count, const double* __restrict__ x,
                                                   double* __restrict__ out) {
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (long long)gridDim.x * blockDim.x)
        out[j] = fn == 0 ? ell_exp(x[j]) : ell_log(x[j]);
}

}  // namespace ellhip
