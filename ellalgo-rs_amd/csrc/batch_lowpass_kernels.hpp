// batch_lowpass_kernels.hpp -- the oracle of B independent FIR low-pass design problems of one filter length, as a policy
// of the loop kernel (include/ellhip_batch_lowpass.h; the loop itself: batch_loop_kernels.hpp).
//
// For every ellipsoid of its workgroup k_batch_loop<T, STABLE, BatchLpOracle> runs rounds of
//     oracle (LowpassOracle::assess_feas / assess_optim, src/oracles/lowpass_oracle.rs:58-150)
//  -> scalar stage + rank-1 (batch_cut_apply, the same code k_batch_update runs)
// without leaving the kernel.  Every `row . x` is the reference's left fold from 0.0 with a separately rounded multiply
// and add, every beta the expression the reference writes, so the loop is bit-identical to cutting_plane_optim /
// cutting_plane_feas over LowpassOracle on the CPU.
//
// Mapping of the oracle onto the n threads of an instance (parallel over rows, never inside a fold): in one step thread
// i takes position t0 + i of the current band's visiting order (positions past the band's length are not taken, so a
// band shorter than n is never visited twice) and folds its row against x.  The first violating position in visiting
// order wins (an LDS minimum over the positions that violate); the band's cursor ends on it.  Without a violation the
// instance moves n positions on, or to the next band: passband, stopband, transition band, then the x[0] < 0 station.
// fmax / kmax: every thread keeps the strict-`>` maximum of its own stopband positions (they ascend, so the first of
// equal values stays); when the stopband ends, the positions before the winner are merged by an LDS maximum over an
// order-preserving key of the value and an LDS minimum over the positions that hold it -- the first position of the
// largest value, which is what the reference's sequential fold keeps.  (A fold that starts at +0.0 never yields -0.0,
// so equal keys and equal values are the same thing.)  NaN fails every comparison exactly as on the CPU.
//
// The table is shared by all instances and stays in HBM / L2 in two layouts: row-major [row][j] for the gradient (the
// n threads read one row) and transposed [j][row] for the folds (the n threads read n consecutive rows).
//
// Barriers are workgroup-wide and the instances of a workgroup sit in different bands, so the walk is driven by
// __syncthreads_or votes; every loop is bounded by 15 + 4 steps and n; no thread waits on another workgroup.
#pragma once

#include <climits>

#include "batch_loop_kernels.hpp"

namespace ellhip {

// oracle scalars (LDS, per instance), after the loop's own (batch_loop_kernels.hpp)
enum : int {
    BO_GAMMA = BL_GAMMA,  // the loop's gamma
    BO_B0 = 5,       // the cut's beta0
    BO_B1 = 6,       // beta1
    BO_HB1 = 7,      // 1: the cut is ParallelCut(beta0, Some(beta1))
    BO_RES = 8,      // the walk's answer (BLP_*), written where the walk ends
    BO_ROW = 9,      // the row the gradient is taken from; -1: the x[0] < 0 station (g = -e0)
    BO_NEG = 10,     // 1: g = -row
    BO_FMAX = 11,
    BO_KMAX = 12,
    BO_SPSQ = 13,    // the oracle's sp_sq field
    BO_KEY = 14,     // unsigned long long: largest key of the stopband values
    BO_FIRST = 15,   // int: first violating position
    BO_KPOS = 16,    // int: first position that holds the largest value
    BO_ANS = 17,     // the call's answer (BLP_*), after the assess_optim tail
    BATCH_LP_SCALARS = 20,
};
static_assert(BO_B0 == BL_SCALARS, "the oracle's scalars follow the loop's");
enum : int { BLP_WALK = -1, BLP_FEAS = 0, BLP_CUT = 1, BLP_SHRUNK = 2, BLP_ERR = 3 };

// doubles of LDS the oracle needs per instance: x and the scalars
__host__ __device__ inline size_t batch_lowpass_lds_doubles(int n) { return ((size_t)n + BATCH_LP_SCALARS) | 1; }

struct BatchLpBands {  // per instance, constant
    int nwpass, nwstop;
    double lp_sq, up_sq;
};
struct BatchLpCursor {  // per instance, persists across calls; every thread of the instance keeps the same copy
    int idx1, idx2, idx3, more_alt;
};

// order-preserving map of a non-NaN double onto unsigned integers
__device__ __forceinline__ unsigned long long batch_lp_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// One oracle call for the workgroup's instances, collectively (it contains barriers: every thread of the workgroup calls
// it).  live: this thread belongs to an instance that takes part.  spec / specT: the table, [row][j] and [j][row].
// x: the instance's point (LDS, n), stored and synchronised by the caller together with osc[BO_SPSQ] (and osc[BO_GAMMA]
// when optim).  On return (after a barrier) osc[BO_ANS] is the answer, osc[BO_B0 / BO_HB1 / BO_B1] the cut, gout the
// gradient (BLP_CUT, BLP_SHRUNK), osc[BO_FMAX / BO_KMAX / BO_GAMMA] and c are updated.
__device__ __forceinline__ void batch_lowpass_oracle(const int mdim, const bool live, const int i, const int n,
                                                     const bool optim, const double* __restrict__ spec,
                                                     const double* __restrict__ specT, const BatchLpBands& K,
                                                     BatchLpCursor& c, const double* x, double* osc, double* gout) {
    int* first = reinterpret_cast<int*>(osc + BO_FIRST);
    int* kpos = reinterpret_cast<int*>(osc + BO_KPOS);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(osc + BO_KEY);
    const double sp_sq = osc[BO_SPSQ];
    bool walking = live;
    int band = 0, t0 = 0;  // 0 passband, 1 stopband, 2 transition band
    double bv = -__builtin_inf();  // this thread's stopband maximum and its position
    int bp = -1;
    if (live) {
        c.more_alt = 1;  //                                                 src/oracles/lowpass_oracle.rs:59
        if (i == 0) {
            osc[BO_RES] = (double)BLP_WALK;
            *first = INT_MAX;
            *kpos = INT_MAX;
            *key = 0ull;  // below the key of every value
        }
    }
    const int nsteps = mdim / n + 5;  // three bands of 15 n rows together, n positions per step, one vote to leave
    for (int step = 0; step < nsteps; ++step) {
        if (!__syncthreads_or(walking)) break;
        int t = -1, row = 0, hi = 0, len = 0, cur = 0;
        double val = 0.0;
        if (walking) {
            int lo;
            if (band == 0) {
                lo = 0, hi = K.nwpass, cur = c.idx1;  //                    :62-84
            } else if (band == 1) {
                lo = K.nwstop, hi = mdim, cur = c.idx3;  //                 :89-112
            } else {
                lo = K.nwpass, hi = K.nwstop, cur = c.idx2;  //             :115-124
            }
            len = hi - lo;
            t = t0 + i;
            if (t < len) {
                row = cur + 1 + t;  // idx += 1; if idx == end { idx = start }, t + 1 times
                if (row >= hi) row -= len;
                const double* a = specT + row;
                double s = 0.0;  //                                         Arr::dot, src/arr.rs:443-451
#pragma unroll 8
                for (int j = 0; j < n; ++j) s += a[(size_t)j * mdim] * x[j];
                val = s;
                bool viol;
                if (band == 0) viol = val > K.up_sq || val < K.lp_sq;
                else if (band == 1) viol = val > sp_sq || val < 0.0;
                else viol = val < 0.0;
                if (viol) atomicMin(first, t);
            }
        }
        __syncthreads();
        const int f = walking ? *first : INT_MAX;
        const bool hit = f != INT_MAX;
        const bool ends = walking && (hit || t0 + n >= len);  // the band ends in this step
        if (walking && band == 1 && t < len && (!hit || t < f) && val > bv) {  //     :106-109, positions before the winner
            bv = val;
            bp = t;
        }
        const bool stop_ends = ends && band == 1;
        const unsigned long long mykey = batch_lp_key(bv);
        if (stop_ends && bp >= 0) atomicMax(key, mykey);
        if (__syncthreads_or(stop_ends)) {
            const bool holds = stop_ends && bp >= 0 && mykey == *key;
            if (holds) atomicMin(kpos, bp);
            __syncthreads();
            if (holds && bp == *kpos) {
                int r = cur + 1 + bp;
                if (r >= hi) r -= len;
                osc[BO_FMAX] = bv;
                osc[BO_KMAX] = (double)r;
            }
        }
        if (walking) {
            if (hit) {
                if (t == f) {  // the winner
                    double b0, b1;
                    int hb1 = 1, neg = 0;
                    if (band == 0) {
                        if (val > K.up_sq) {
                            b0 = val - K.up_sq, b1 = val - K.lp_sq;  //     :69-75
                        } else {
                            b0 = -val + K.lp_sq, b1 = -val + K.up_sq, neg = 1;  // :76-83
                        }
                    } else if (band == 1) {
                        if (val > sp_sq) {
                            b0 = val - sp_sq, b1 = val;  //                 :96-99
                        } else {
                            b0 = -val, b1 = -val + sp_sq, neg = 1;  //      :100-105
                        }
                    } else {
                        b0 = -val, b1 = 0.0, hb1 = 0, neg = 1;  //          :119-123
                    }
                    osc[BO_B0] = b0;
                    osc[BO_B1] = b1;
                    osc[BO_HB1] = (double)hb1;
                    osc[BO_ROW] = (double)row;
                    osc[BO_NEG] = (double)neg;
                    osc[BO_RES] = (double)BLP_CUT;
                }
                int r = cur + 1 + f;  // the cursor ends on the winner
                if (r >= hi) r -= len;
                if (band == 0) c.idx1 = r;
                else if (band == 1) c.idx3 = r;
                else c.idx2 = r;
                walking = false;
            } else if (ends) {
                if (len > 0) {  // the cursor has gone once round the band
                    int r = cur + len;
                    if (r >= hi) r -= len;
                    if (band == 0) c.idx1 = r;
                    else if (band == 1) c.idx3 = r;
                    else c.idx2 = r;
                }
                if (band == 0 && i == 0) {  //                              :86-87
                    osc[BO_FMAX] = -__builtin_inf();
                    osc[BO_KMAX] = -1.0;
                }
                int nb = band + 1;
                if (nb == 1 && K.nwstop >= mdim) nb = 2;       // no stopband
                if (nb == 2 && K.nwstop <= K.nwpass) nb = 3;   // no transition band
                band = nb;
                t0 = 0;
                if (nb == 3) {
                    c.more_alt = 0;  //                                     :125
                    walking = false;
                    if (i == 0) {
                        const double x0 = x[0];
                        if (x0 < 0.0) {  //                                 :126-130
                            osc[BO_B0] = -x0;
                            osc[BO_B1] = 0.0;
                            osc[BO_HB1] = 0.0;
                            osc[BO_ROW] = -1.0;
                            osc[BO_NEG] = 0.0;
                            osc[BO_RES] = (double)BLP_CUT;
                        } else {
                            osc[BO_RES] = (double)BLP_FEAS;
                        }
                    }
                }
            } else {
                t0 += n;
            }
        }
    }
    // ---- the gradient, and the tail of assess_optim                      :139-150
    if (live) {
        int ans = (int)osc[BO_RES];
        if (ans == BLP_CUT) {
            const int row = (int)osc[BO_ROW];
            if (row < 0) {
                gout[i] = i == 0 ? -1.0 : 0.0;
            } else {
                const double v = spec[(size_t)row * n + i];
                gout[i] = osc[BO_NEG] != 0.0 ? -v : v;
            }
        } else if (optim && ans == BLP_FEAS) {
            const int kmax = (int)osc[BO_KMAX];
            if (kmax < 0) {
                ans = BLP_ERR;  // spectrum[usize::MAX]: the reference panics
            } else {
                ans = BLP_SHRUNK;
                gout[i] = spec[(size_t)kmax * n + i];
                if (i == 0) {
                    const double fmax = osc[BO_FMAX];
                    osc[BO_B0] = 0.0;
                    osc[BO_B1] = fmax;
                    osc[BO_HB1] = 1.0;
                    osc[BO_GAMMA] = fmax;  //                               :148
                }
            }
        } else if (ans != BLP_FEAS) {
            ans = BLP_ERR;  // (a walk that did not end: cannot happen within nsteps)
        }
        if (i == 0) osc[BO_ANS] = (double)ans;
    }
    __syncthreads();
}

// The oracle as the loop kernel's policy (batch_loop_kernels.hpp).  Per instance in HBM: the bands and limits (constant),
// the cursor, fmax / kmax and sp_sq.
struct BatchLpOracle {
    struct Args {
        const double* spec;   // [15 n][n]
        const double* specT;  // [n][15 n]
        const int* bands;     // [B][2]: nwpass, nwstop
        const double* lims;   // [B][2]: lp_sq, up_sq
        int* cursor;          // [B][4]: idx1, idx2, idx3, more_alt
        int* kmax;            // [B]
        double* fmax;         // [B]
        double* spsq;         // [B]
        int mdim;             // 15 n
    };
    struct Regs {
        BatchLpBands K{1, 1, 0.0, 0.0};
        BatchLpCursor c{-1, 0, 0, 1};
    };
    static __host__ __device__ inline size_t lds_doubles(const Args&, int n) { return batch_lowpass_lds_doubles(n); }
    static __device__ __forceinline__ size_t scalars_at(const Args&, int n) { return (size_t)n; }
    static __device__ __forceinline__ void load(const Args& A, bool active, long long b, int i, int n, double* blk, Regs& r) {
        if (active) {
            r.K.nwpass = A.bands[2 * b];
            r.K.nwstop = A.bands[2 * b + 1];
            r.K.lp_sq = A.lims[2 * b];
            r.K.up_sq = A.lims[2 * b + 1];
            r.c.idx1 = A.cursor[4 * b];
            r.c.idx2 = A.cursor[4 * b + 1];
            r.c.idx3 = A.cursor[4 * b + 2];
            r.c.more_alt = A.cursor[4 * b + 3];
        }
        if (active && i == 0) {
            double* osc = blk + n;
            osc[BO_FMAX] = A.fmax[b];
            osc[BO_KMAX] = (double)A.kmax[b];
            osc[BO_SPSQ] = A.spsq[b];
        }
    }
    static __device__ __forceinline__ void assess(const Args& A, const BatchLoopRun& R, bool live, int i, int n, double xci,
                                                  double* blk, Regs& r, double* g) {
        double* osc = blk + n;
        const bool optim = R.feas == 0;
        if (live) {
            blk[i] = xci;
            if (optim && i == 0) osc[BO_SPSQ] = osc[BO_GAMMA];  //          self.sp_sq = *sp_sq, lowpass_oracle.rs:140
        }
        __syncthreads();
        batch_lowpass_oracle(A.mdim, live, i, n, optim, A.spec, A.specT, r.K, r.c, blk, osc, g);
    }
    // BLP_FEAS under cutting_plane_optim never leaves the oracle (it shrinks, or has no stopband row to take the
    // objective from: BLP_ERR)
    static __device__ __forceinline__ BatchOutcome outcome(const Args&, int feas, const double* osc) {
        const int ans = (int)osc[BO_ANS];
        const int what = ans == BLP_CUT ? BOUT_CUT
                         : ans == BLP_SHRUNK ? BOUT_SHRUNK
                         : (feas && ans == BLP_FEAS) ? BOUT_FEAS
                                                     : BOUT_NONE;
        return BatchOutcome{what, osc[BO_B0], (int)osc[BO_HB1], osc[BO_B1]};
    }
    static __device__ __forceinline__ void store(const Args& A, long long b, const double* osc, const Regs& r) {
        A.cursor[4 * b] = r.c.idx1;
        A.cursor[4 * b + 1] = r.c.idx2;
        A.cursor[4 * b + 2] = r.c.idx3;
        A.cursor[4 * b + 3] = r.c.more_alt;
        A.fmax[b] = osc[BO_FMAX];
        A.kmax[b] = (int)osc[BO_KMAX];
        A.spsq[b] = osc[BO_SPSQ];
    }
};

// One oracle call per instance at x[B][n]: the same device function, without an ellipsoid.  optim: assess_optim with
// gamma in and out; ans_out[B] = BLP_*; grad_out rows and the cut values are written for BLP_CUT and BLP_SHRUNK only.
template <int T>
__global__ __launch_bounds__(T) void k_batch_lowpass_assess(long long B, int n, int epw, int optim, BatchLpOracle::Args A,
                                                            double* __restrict__ gamma_io, const double* __restrict__ x,
                                                            double* __restrict__ grad_out, double* __restrict__ beta0,
                                                            int* __restrict__ has_beta1, double* __restrict__ beta1,
                                                            int* __restrict__ ans_out) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * epw + e;
    const bool active = e < epw && b < B;
    const size_t lper = batch_lowpass_lds_doubles(n) + (size_t)n;
    double* lx = sm + (size_t)(e < epw ? e : 0) * lper;
    double* osc = lx + n;
    double* g = osc + BATCH_LP_SCALARS;
    BatchLpOracle::Regs r;
    BatchLpOracle::load(A, active, b, i, n, lx, r);
    if (active) lx[i] = x[b * n + i];
    if (active && i == 0) {
        osc[BO_GAMMA] = gamma_io[b];
        if (optim) osc[BO_SPSQ] = gamma_io[b];  //                          self.sp_sq = *sp_sq, lowpass_oracle.rs:140
    }
    __syncthreads();
    batch_lowpass_oracle(A.mdim, active, i, n, optim != 0, A.spec, A.specT, r.K, r.c, lx, osc, g);
    const int ans = active ? (int)osc[BO_ANS] : BLP_ERR;
    if (active && (ans == BLP_CUT || ans == BLP_SHRUNK)) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        BatchLpOracle::store(A, b, osc, r);
        gamma_io[b] = osc[BO_GAMMA];
        ans_out[b] = ans;
        if (ans == BLP_CUT || ans == BLP_SHRUNK) {
            beta0[b] = osc[BO_B0];
            has_beta1[b] = (int)osc[BO_HB1];
            beta1[b] = osc[BO_B1];
        }
    }
}

}  // namespace ellhip
