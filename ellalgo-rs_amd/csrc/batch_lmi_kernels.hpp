// batch_lmi_kernels.hpp -- the oracle of B independent LMI-constrained cutting-plane solves, as a policy of the loop kernel
// (include/ellhip_batch_lmi.h; the loop itself: batch_loop_kernels.hpp).
//
// For every ellipsoid of its workgroup k_batch_loop<T, STABLE, BatchLmiOracle> runs rounds of
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
// Second layout for F(x) (handles of ellhip_batch_lmi_create_streamed; Args::tri non-null): beside the k-fastest pencil a
// copy of the lower triangle only, element fastest: T[inst][block][k][t], t = a (a + 1) / 2 + b, b <= a.  Thread i then takes
// the elements t = i, i + n, ... of the m (m + 1) / 2 and folds the same s -= T[k][t] * x[k], k ascending: the loads of a wave
// are consecutive doubles, x[k] is a broadcast from LDS and no thread idles on b > a.  At n = 1024, m = 64 the k-fastest walk
// makes every load instruction of a wave touch 64 cache lines 8 KiB apart, with half the threads idle in each of four passes.
// The fold per element is the same sequence of operations, so the bits are the same.  Handles of ellhip_batch_lmi_create keep
// tri null and run the code they always ran.
//
// Barriers are workgroup-wide, so the walk over stations runs in lockstep: every instance of the workgroup takes its
// next station in the same step, and the column loop runs to the largest block size.  Every loop is bounded by J + 1, M
// and n; no thread waits on another workgroup.
//
// Nothing here is tied to the number of instances in a workgroup or to n <= 128: the streamed loops
// (k_batch_streamed_loop<BatchLmiOracle>, k_batch_streamed_loop_stable<BatchLmiOracle>; batch_lmi_streamed_capi.inc.hpp,
// DESIGN section 9.11) take this policy unchanged with one instance per workgroup of n rounded up to 64 threads, n <= 1024.
// Threads i >= n are not live, own no element, row or quadratic form, and reach every barrier and vote.  One pencil may
// serve every instance (ellhip_batch_lmi_create_streamed, shared_f): Args::L.fstride is then 0, and load() is the only place
// that applies it.
#pragma once

#include "batch_loop_kernels.hpp"

namespace ellhip {

constexpr int BATCH_LMI_JMAX = 8;
constexpr int BATCH_LMI_MMAX = 64;

struct BatchLmiParams {
    int J;                        // blocks
    int m[BATCH_LMI_JMAX];        // block sizes
    int foff[BATCH_LMI_JMAX];     // offset of block j inside an instance's pencil, in doubles
    int boff[BATCH_LMI_JMAX];     // offset of block j inside an instance's B matrices
    int fstride;                  // n * sum m_j^2; 0 in the Args of a handle whose instances share one pencil
    int toff[BATCH_LMI_JMAX];     // offset of block j inside an instance's triangle copy: n * sum_{j' < j} m_j' (m_j' + 1) / 2
    int tstride;                  // n * sum m_j (m_j + 1) / 2; 0 when shared, like fstride
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

// oracle scalars (LDS, per instance), after the loop's own (batch_loop_kernels.hpp)
enum : int {
    LO_GAMMA = BL_GAMMA,          // best-so-far objective value
    LO_IDX = BL_SCALARS,          // round-robin index
    LO_F0 = BL_SCALARS + 1,       // c . x
    LO_BETA = BL_SCALARS + 2,     // the cut's beta
    LO_STATION = BL_SCALARS + 3,  // -1 while walking; the station that cut; nstation = every station passed
    LO_CUR = BL_SCALARS + 4,      // block under factorisation in this step, -1 = none
};

// The oracle for the workgroup's instances, collectively (it contains barriers: every thread of the workgroup calls it).
// live: this thread belongs to an instance that takes part.  x, cl: the instance's point and objective vector (LDS, n
// each); fa: m x pm factorisation; wit; osc: scalars; gout: n doubles for the gradient.  F, Bm: this instance's pencil;
// Tr: its triangle copy, or null.
// On return (after a barrier) osc[LO_STATION], osc[LO_BETA], osc[LO_GAMMA], osc[LO_IDX] and gout hold the answer.
__device__ __forceinline__ void batch_lmi_oracle(const BatchLmiParams& L, const bool live, const int i, const int n,
                                                 const double* __restrict__ F, const double* __restrict__ Bm,
                                                 const double* __restrict__ Tr, const double* x, const double* cl,
                                                 double* fa, double* wit, double* osc, double* gout) {
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
        if (cur >= 0 && Tr) {  // the element-fastest triangle copy: t = a (a + 1) / 2 + b
            const int nt = m * (m + 1) / 2;
            const double* Tb = Tr + L.toff[cur];
            const double* Bb = Bm + L.boff[cur];
            for (int t = i; t < nt; t += n) {
                // 8 t + 1 <= 16633 and sqrt is correctly rounded, so the floor is exact; the two steps only guard it
                int a = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
                if (a * (a + 1) / 2 > t) a -= 1;
                if ((a + 1) * (a + 2) / 2 <= t) a += 1;
                const int b = t - a * (a + 1) / 2;
                const double* f = Tb + t;
                double s;
                if (L.has_b) {
                    s = Bb[a * m + b];
                    for (int k = 0; k < n; ++k) s -= f[(size_t)k * nt] * x[k];
                } else {
                    s = 0.0;  //                                            src/oracles/lmi0_oracle.rs:18-24
                    for (int k = 0; k < n; ++k) s += f[(size_t)k * nt] * x[k];
                }
                fa[a * pm + b] = s;
            }
        } else if (cur >= 0) {
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

// The oracle as the loop kernel's policy (batch_loop_kernels.hpp).  Per instance in HBM: the pencil, the objective vector
// and the round-robin index.
struct BatchLmiOracle {
    struct Args {
        BatchLmiParams L;
        const double* pencil;  // [B][block][a][b][k]; [block][a][b][k] when L.fstride == 0
        const double* tri;     // [B][block][k][t] ([block][k][t] when L.tstride == 0), or null: F(x) reads the pencil
        const double* matb;    // [B][block][a][b], or null
        const double* cvec;    // [B][n], or null
        int* idx;              // [B]
    };
    struct Regs {
        const double *F, *Bm, *T;  // this instance's pencil and its triangle copy
    };
    struct Lds {
        double *x, *cl, *fa, *wit, *osc;
    };
    static __host__ __device__ inline size_t lds_doubles(const Args& A, int n) { return batch_lmi_lds_doubles(n, A.L.mmax); }
    static __device__ __forceinline__ size_t scalars_at(const Args& A, int n) {
        return 2 * (size_t)n + (size_t)A.L.mmax * A.L.pm + A.L.mmax;
    }
    static __device__ __forceinline__ Lds carve(const Args& A, int n, double* blk) {
        Lds d;
        d.x = blk;
        d.cl = d.x + n;
        d.fa = d.cl + n;
        d.wit = d.fa + (size_t)A.L.mmax * A.L.pm;
        d.osc = d.wit + A.L.mmax;
        return d;
    }
    static __device__ __forceinline__ void load(const Args& A, bool active, long long b, int i, int n, double* blk, Regs& r) {
        const Lds d = carve(A, n, blk);
        if (active) d.cl[i] = A.L.has_c ? A.cvec[b * n + i] : 0.0;
        if (active && i == 0) d.osc[LO_IDX] = (double)A.idx[b];
        r.F = A.pencil + (active ? b : 0) * (long long)A.L.fstride;
        r.Bm = A.matb ? A.matb + (active ? b : 0) * (long long)A.L.bstride : nullptr;
        r.T = A.tri ? A.tri + (active ? b : 0) * (long long)A.L.tstride : nullptr;
    }
    static __device__ __forceinline__ void assess(const Args& A, const BatchLoopRun&, bool live, int i, int n, double xci,
                                                  double* blk, Regs& r, double* g) {
        const Lds d = carve(A, n, blk);
        if (live) d.x[i] = xci;
        __syncthreads();
        batch_lmi_oracle(A.L, live, i, n, r.F, r.Bm, r.T, d.x, d.cl, d.fa, d.wit, d.osc, g);
    }
    // every station passed: cutting_plane_optim shrinks (tests/lmi_tests.rs:170), cutting_plane_feas has its point
    static __device__ __forceinline__ BatchOutcome outcome(const Args& A, int feas, const double* osc) {
        const bool all_pass = osc[LO_STATION] == (double)(A.L.J + 1);
        return BatchOutcome{all_pass ? (feas ? BOUT_FEAS : BOUT_SHRUNK) : BOUT_CUT, osc[LO_BETA], 0, 0.0};
    }
    static __device__ __forceinline__ void store(const Args& A, long long b, const double* osc, const Regs&) {
        A.idx[b] = (int)osc[LO_IDX];
    }
};

// One oracle call per instance at x[B][n]: the same device function, without an ellipsoid.
// Two launch shapes: epw instances packed into T = 128 or 256 threads (n <= 128), or the wide one past it -- epw = 1, one
// workgroup per instance, blockDim.x = n rounded up to 64 (T = 1024 only bounds the block); threads tid >= n belong to no
// instance (e = 1 >= epw), are inactive in the oracle and take part in its barriers.  LDS: epw * (batch_lmi_lds_doubles(n, M)
// + n) doubles, 57.1 KiB at n = 1024, M = 64.  Every loop is bounded by J + 1, M and n; no thread waits on another workgroup
// or on a memory word.
template <int T>
__global__ __launch_bounds__(T) void k_batch_lmi_assess(long long B, int n, int epw, BatchLmiOracle::Args A,
                                                        const double* __restrict__ x, double* __restrict__ gamma_io,
                                                        double* __restrict__ grad_out, double* __restrict__ beta_out,
                                                        int* __restrict__ station_out) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * epw + e;
    const bool active = e < epw && b < B;
    const size_t lper = batch_lmi_lds_doubles(n, A.L.mmax) + (size_t)n;
    double* blk = sm + (size_t)(e < epw ? e : 0) * lper;
    const BatchLmiOracle::Lds d = BatchLmiOracle::carve(A, n, blk);
    double* g = d.osc + 16;
    BatchLmiOracle::Regs r;
    BatchLmiOracle::load(A, active, b, i, n, blk, r);
    if (active) {
        d.x[i] = x[b * n + i];
        g[i] = grad_out[b * n + i];
    }
    if (active && i == 0) d.osc[LO_GAMMA] = gamma_io[b];
    __syncthreads();
    batch_lmi_oracle(A.L, active, i, n, r.F, r.Bm, r.T, d.x, d.cl, d.fa, d.wit, d.osc, g);
    if (active) grad_out[b * n + i] = g[i];
    if (active && i == 0) {
        gamma_io[b] = d.osc[LO_GAMMA];
        BatchLmiOracle::store(A, b, d.osc, r);
        beta_out[b] = d.osc[LO_BETA];
        station_out[b] = (int)d.osc[LO_STATION];
    }
}

}  // namespace ellhip
