// batch_lmi_kernels.hpp -- B independent LMI-constrained cutting-plane solves, oracle and ellipsoid update in one kernel
// (include/ellhip_batch_lmi.h).
//
// A workgroup owns the ellipsoids the batch engine gives it (batch_kernels.hpp: thread (e, i) = row i of local
// ellipsoid e, Q in LDS) and, for each of them, runs up to `iters` rounds of
//     oracle (round-robin over J LMI blocks and the objective, tests/lmi_tests.rs:142-171)
//  -> scalar stage + rank-1 (batch_cut_apply, the same code k_batch_update runs)
// without leaving the kernel.  Everything is + - * / in the reference's fold order, so the loop is bit-identical to
// cutting_plane_optim / cutting_plane_feas over LMIOracle / LMI0Oracle on the CPU.
//
// Mapping of the oracle onto the n threads of an instance (parallel over independent outputs only, never inside a fold):
//   F(x)      one thread per element of the lower triangle: s = B[a][b]; s -= F_k[a][b] * x[k], k ascending
//             (src/oracles/lmi_oracle.rs:28-34; LMI0: s = 0.0; s += ..., src/oracles/lmi0_oracle.rs:18-24)
//   factor    one thread per row, one barrier per column (LDLTMgr::factor, src/oracles/ldlt_mgr.rs:29-55): at column c row
//             r >= c folds s += L[r][k] * U[k][c] over k < c and keeps diag = elem(r, c) - s as U[c][r]; the reference
//             runs the same folds row after row, and row r never reads anything a later row writes, so the order of rows is
//             free.  The first diag <= 0 on the diagonal ends the factorisation exactly where the reference breaks.
//   witness   thread 0, the back substitution as written (:98-111)
//   sym_quad  one thread per quadratic form k: result += (wit[a] * F_k[a][b]) * wit[b], a-major from 0.0 (:115-124)
// The pencil stays in HBM / L2, k fastest: F[inst][block][a][b][k], so the n threads of sym_quad read consecutive
// doubles and a thread of F(x) walks n consecutive doubles; B[inst][block][a][b].
//
// Barriers are workgroup-wide, so the walk over stations runs in lockstep: every instance of the workgroup takes its
// next station in the same step, and the column loop runs to the largest block size.  Every loop is bounded by iters,
// J + 1, M and n; no thread waits on another workgroup.
#pragma once

#include "batch_stable_apply.hpp"

namespace ellhip {

constexpr int BATCH_LMI_JMAX = 8;
constexpr int BATCH_LMI_MMAX = 64;

struct BatchLmiParams {
    int J;                        // blocks
    int m[BATCH_LMI_JMAX];        // block sizes
    int foff[BATCH_LMI_JMAX];     // offset of block j inside an instance's pencil, in doubles
    int boff[BATCH_LMI_JMAX];     // offset of block j inside an instance's B matrices
    int fstride;                  // n * sum m_j^2
    int bstride;                  // sum m_j^2
    int mmax;                     // max m_j
    int pm;                       // LDS pitch of the factorisation (odd)
    int has_b;                    // 0: LMI0 form
    int has_c;                    // 0: feasibility problem
    int nstation;                 // J + has_c
};

// doubles of LDS the oracle needs per instance: x, c, the factorisation, the witness, 16 scalars
__host__ __device__ inline size_t batch_lmi_lds_doubles(int n, int mmax) {
    return (2 * (size_t)n + (size_t)mmax * (size_t)(mmax | 1) + (size_t)mmax + 16) | 1;
}

// oracle scalars (LDS, per instance)
enum : int {
    LO_GAMMA = 0,    // best-so-far objective value
    LO_IDX = 1,      // round-robin index
    LO_F0 = 2,       // c . x
    LO_BETA = 3,     // the cut's beta
    LO_STATION = 4,  // -1 while walking; the station that cut; nstation = every station passed
    LO_CUR = 5,      // block under factorisation in this step, -1 = none
    LO_NITER = 8,
    LO_STOPPED = 9,
    LO_HASBEST = 10,
    LO_STATUS = 11,
};

// The oracle for the workgroup's instances, collectively (it contains barriers: every thread of the workgroup calls it).
// live: this thread belongs to an instance that takes part.  x, cl: the instance's point and objective vector (LDS, n
// each); fa: m x pm factorisation; wit; osc: scalars; gout: n doubles for the gradient.  F, Bm: this instance's pencil.
// On return (after a barrier) osc[LO_STATION], osc[LO_BETA], osc[LO_GAMMA], osc[LO_IDX] and gout hold the answer.
__device__ __forceinline__ void batch_lmi_oracle(const BatchLmiParams& L, const bool live, const int i, const int n,
                                                 const double* __restrict__ F, const double* __restrict__ Bm,
                                                 const double* x, const double* cl, double* fa, double* wit, double* osc,
                                                 double* gout) {
    const int pm = L.pm;
    if (live && i == 0) {
        double f0 = 0.0;  //                                                tests/lmi_tests.rs:146
        if (L.has_c)
            for (int k = 0; k < n; ++k) f0 += cl[k] * x[k];
        osc[LO_F0] = f0;
        osc[LO_STATION] = -1.0;
    }
    for (int step = 0; step < L.nstation; ++step) {
        if (i == 0 && live) {
            int cur = -1;
            if (osc[LO_STATION] < 0.0) {
                int idx = (int)osc[LO_IDX];
                idx = (idx >= L.nstation - 1) ? 0 : idx + 1;  //            :148
                osc[LO_IDX] = (double)idx;
                if (idx == L.J) {  // the objective                         :160-166
                    const double fj = osc[LO_F0] - osc[LO_GAMMA];
                    if (fj > 0.0) {
                        osc[LO_BETA] = fj;
                        osc[LO_STATION] = (double)L.J;
                    } else {
                        osc[LO_GAMMA] = osc[LO_F0];
                    }
                } else {
                    cur = idx;
                }
            }
            osc[LO_CUR] = (double)cur;
        }
        __syncthreads();
        const int cur = live ? (int)osc[LO_CUR] : -1;
        const bool walking = live && osc[LO_STATION] < 0.0;
        if (!__syncthreads_or(cur >= 0)) {
            if (!__syncthreads_or(walking)) break;
            continue;
        }
        const int m = cur >= 0 ? L.m[cur] : 0;
        // ---- F(x), lower triangle                                        src/oracles/lmi_oracle.rs:28-34
        if (cur >= 0) {
            const double* Fb = F + L.foff[cur];
            const double* Bb = Bm + L.boff[cur];
            int a = i / m, b = i - a * m;
            const int da = n / m, db = n - da * m;
            for (int el = i; el < m * m; el += n) {
                if (b <= a) {
                    const double* f = Fb + (size_t)el * n;
                    double s;
                    if (L.has_b) {
                        s = Bb[el];
                        for (int k = 0; k < n; ++k) s -= f[k] * x[k];
                    } else {
                        s = 0.0;  //                                        src/oracles/lmi0_oracle.rs:18-24
                        for (int k = 0; k < n; ++k) s += f[k] * x[k];
                    }
                    fa[a * pm + b] = s;
                }
                a += da;
                b += db;
                if (b >= m) {
                    b -= m;
                    a += 1;
                }
            }
        }
        __syncthreads();
        // ---- LDLTMgr::factor, column by column                           src/oracles/ldlt_mgr.rs:29-55
        int p = -1;  // the row whose diagonal came out <= 0 (pos = (0, p + 1)); -1 = positive definite so far
        for (int c = 0; c < L.mmax; ++c) {
            const bool go = cur >= 0 && c < m && p < 0;
            if (go) {
                for (int r = i; r < m; r += n) {
                    if (r < c) continue;
                    double* row = fa + r * pm;
                    double diag;
                    if (c == 0) {
                        diag = row[0];  //                                  :33
                    } else {
                        row[c - 1] = fa[(c - 1) * pm + r] / fa[(c - 1) * pm + (c - 1)];  // L[r][c-1]   :38-39
                        double s = 0.0;
                        for (int k = 0; k < c; ++k) s += row[k] * fa[k * pm + c];  //    :42-45
                        diag = row[c] - s;  //                                           :46
                    }
                    fa[c * pm + r] = diag;  // "keep for later" (:37); r == c: the diagonal (:48)
                }
            }
            __syncthreads();
            if (go && fa[c * pm + c] <= 0.0) p = c;  //                     :49-52
        }
        // ---- witness                                                     :98-111
        if (p >= 0 && i == 0) {
            wit[p] = 1.0;
            for (int r = p; r >= 1; --r) {
                double s = 0.0;
                for (int k = r; k <= p; ++k) s += fa[k * pm + (r - 1)] * wit[k];
                wit[r - 1] = -s;
            }
            osc[LO_BETA] = -fa[p * pm + p];
            osc[LO_STATION] = (double)cur;
        }
        __syncthreads();
        // ---- the n quadratic forms                                       :115-124, lmi_oracle.rs:39-42
        if (p >= 0) {
            const double* Fk = F + L.foff[cur] + i;
            double q = 0.0;
            for (int a = 0; a <= p; ++a) {
                const double wa = wit[a];
                const double* fr = Fk + (size_t)a * m * n;
                for (int b = 0; b <= p; ++b) q += wa * fr[(size_t)b * n] * wit[b];
            }
            gout[i] = L.has_b ? q : -q;  //                                 lmi0_oracle.rs:31
        }
    }
    if (live && i == 0 && osc[LO_STATION] < 0.0) {  // every station passed  tests/lmi_tests.rs:170
        osc[LO_BETA] = 0.0;
        osc[LO_STATION] = (double)(L.J + 1);
    }
    __syncthreads();
    if (live && L.has_c && osc[LO_STATION] >= (double)L.J) gout[i] = cl[i];
    __syncthreads();
}

struct BatchLmiLoop {
    int iters;            // iterations this launch may run
    int feas;             // 1: cutting_plane_feas
    long long max_iters;
    double tol;
};

// cutting_plane_optim (src/cutting_plane.rs:286-313) / cutting_plane_feas (:205-227) for every instance of the workgroup.
// Loop state per instance lives in HBM between launches: idx, gamma, x_best, has_best, niter, stopped, status.
// STABLE: the spaces are EllStable buffers and a cut is batch_stable_cut_apply (batch_stable_apply.hpp).
template <int T, bool STABLE = false>
__global__ __launch_bounds__(T) void k_batch_lmi_loop(BatchParams P, BatchLmiParams L, BatchLmiLoop R,
                                                      double* __restrict__ Q, double* __restrict__ xc,
                                                      double* __restrict__ kappa, double* __restrict__ tsq,
                                                      const double* __restrict__ pencil, const double* __restrict__ matb,
                                                      const double* __restrict__ cvec, int* __restrict__ idx_io,
                                                      double* __restrict__ gamma_io, double* __restrict__ xbest,
                                                      int* __restrict__ has_best, long long* __restrict__ niter_io,
                                                      int* __restrict__ stopped_io, int* __restrict__ status_io,
                                                      int* __restrict__ nstopped, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, pitch = P.pitch;
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * P.epw + e;
    const bool active = e < P.epw && b < P.B;
    if (!__syncthreads_or(active && stopped_io[b] == 0)) return;  // all of this workgroup's instances have stopped

    const size_t per = batch_space_lds_doubles<STABLE>(n);
    const size_t lper = batch_lmi_lds_doubles(n, L.mmax);
    const int el = e < P.epw ? e : 0;
    double* q = sm + (size_t)el * per;
    double* g = q + (size_t)n * pitch;
    double* sc = q + batch_space_scalars_at<STABLE>(n);  // as in k_batch_update
    double* lx = sm + (size_t)P.epw * per + (size_t)el * lper;
    double* cl = lx + n;
    double* fa = cl + n;
    double* wit = fa + (size_t)L.mmax * L.pm;
    double* osc = wit + L.mmax;

    const long long b_first = (long long)blockIdx.x * P.epw;
    const int nb = (int)((P.B - b_first < P.epw) ? P.B - b_first : P.epw);
    double* Qwg = Q + b_first * (long long)n * n;
    batch_copy<T, true>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
    double xci = 0.0, xb = 0.0;
    if (active) {
        xci = xc[b * n + i];
        xb = xbest[b * n + i];
        cl[i] = L.has_c ? cvec[b * n + i] : 0.0;
    }
    if (active && i == 0) {
        sc[3] = (double)ST_SUCCESS;
        sc[4] = kappa[b];
        sc[5] = tsq[b];
        osc[LO_GAMMA] = gamma_io[b];
        osc[LO_IDX] = (double)idx_io[b];
        osc[LO_NITER] = (double)niter_io[b];
        osc[LO_STOPPED] = (double)stopped_io[b];
        osc[LO_HASBEST] = (double)has_best[b];
        osc[LO_STATUS] = (double)status_io[b];
    }
    __syncthreads();

    const bool lane_ok = tid < P.epw && b_first + tid < P.B;
    const int es = tid < P.epw ? tid : 0;
    double* q_s = sm + (size_t)es * per;
    const double* osc_s = sm + (size_t)P.epw * per + (size_t)es * lper + 2 * (size_t)n + (size_t)L.mmax * L.pm + L.mmax;
    const double* F = pencil + (active ? b : 0) * (long long)L.fstride;
    const double* Bm = matb ? matb + (active ? b : 0) * (long long)L.bstride : nullptr;
    const double shrunk_station = (double)(L.J + 1);

    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && osc[LO_STOPPED] == 0.0;
        if (!__syncthreads_or(live)) break;
        if (live) lx[i] = xci;
        __syncthreads();
        batch_lmi_oracle(L, live, i, n, F, Bm, lx, cl, fa, wit, osc, g);
        const bool all_pass = live && osc[LO_STATION] == shrunk_station;
        const bool found = R.feas && all_pass;  // cutting_plane_feas: a feasible point ends the loop   :217-220
        if (all_pass) xb = xci;                 // x_best = Some(space.xc())                            :303
        const bool upd = live && !found;
        const bool lane = lane_ok && osc_s[LO_STOPPED] == 0.0 && !(R.feas && osc_s[LO_STATION] == shrunk_station);
        const int kind = (lane && osc_s[LO_STATION] == shrunk_station) ? CUT_CENTRAL : CUT_BIAS;  // :301-307
        const double beta = lane ? osc_s[LO_BETA] : 0.0;
        batch_space_cut_apply<STABLE>(P, calc, upd, i, q, xci, lane, q_s, kind, beta, 0, 0.0, [](int, double) {});
        if (live && i == 0) {
            if (all_pass) osc[LO_HASBEST] = 1.0;
            bool stop;
            if (found) {
                osc[LO_STATUS] = (double)ST_SUCCESS;
                stop = true;
            } else if (sc[3] != (double)ST_SUCCESS || sc[5] < R.tol) {  //                              :308 / :222
                osc[LO_STATUS] = sc[3];
                stop = true;
            } else {
                const double done = osc[LO_NITER] + 1.0;
                osc[LO_NITER] = done;
                osc[LO_STATUS] = (double)ST_SUCCESS;
                stop = done >= (double)R.max_iters;
            }
            if (stop) {
                osc[LO_STOPPED] = 1.0;
                atomicAdd(nstopped, 1);
            }
        }
        __syncthreads();
    }

    if (active) {
        xc[b * n + i] = xci;
        if (osc[LO_HASBEST] != 0.0) xbest[b * n + i] = xb;
    }
    if (active && i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
        gamma_io[b] = osc[LO_GAMMA];
        idx_io[b] = (int)osc[LO_IDX];
        niter_io[b] = (long long)osc[LO_NITER];
        stopped_io[b] = (int)osc[LO_STOPPED];
        has_best[b] = (int)osc[LO_HASBEST];
        status_io[b] = (int)osc[LO_STATUS];
    }
    batch_copy<T, false>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
}

// One oracle call per instance at x[B][n]: the same device function, without an ellipsoid.
template <int T>
__global__ __launch_bounds__(T) void k_batch_lmi_assess(long long B, int n, int epw, BatchLmiParams L,
                                                        const double* __restrict__ pencil, const double* __restrict__ matb,
                                                        const double* __restrict__ cvec, const double* __restrict__ x,
                                                        int* __restrict__ idx_io, double* __restrict__ gamma_io,
                                                        double* __restrict__ grad_out, double* __restrict__ beta_out,
                                                        int* __restrict__ station_out) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * epw + e;
    const bool active = e < epw && b < B;
    const size_t lper = batch_lmi_lds_doubles(n, L.mmax) + (size_t)n;
    double* lx = sm + (size_t)(e < epw ? e : 0) * lper;
    double* cl = lx + n;
    double* fa = cl + n;
    double* wit = fa + (size_t)L.mmax * L.pm;
    double* osc = wit + L.mmax;
    double* g = osc + 16;
    if (active) {
        lx[i] = x[b * n + i];
        cl[i] = L.has_c ? cvec[b * n + i] : 0.0;
        g[i] = grad_out[b * n + i];
    }
    if (active && i == 0) {
        osc[LO_GAMMA] = gamma_io[b];
        osc[LO_IDX] = (double)idx_io[b];
    }
    __syncthreads();
    const double* F = pencil + (active ? b : 0) * (long long)L.fstride;
    const double* Bm = matb ? matb + (active ? b : 0) * (long long)L.bstride : nullptr;
    batch_lmi_oracle(L, active, i, n, F, Bm, lx, cl, fa, wit, osc, g);
    if (active) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        gamma_io[b] = osc[LO_GAMMA];
        idx_io[b] = (int)osc[LO_IDX];
        beta_out[b] = osc[LO_BETA];
        station_out[b] = (int)osc[LO_STATION];
    }
}

}  // namespace ellhip
