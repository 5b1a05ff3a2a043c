// batch_streamed_kernels.hpp -- many independent ellipsoids of up to 1024 dimensions, streamed from HBM
// (include/ellhip_batch_streamed.h).
//
// The LDS engine (batch_kernels.hpp) stops at n = 128 because it keeps each matrix in LDS.  Here the matrix stays in HBM
// ([B][n][n] row-major, exactly what ellhip_batch_get_mq returns) and only g, Q g, sigma/omega * Q g, the omega terms and
// the scalars of one ellipsoid live in LDS.  One workgroup per ellipsoid, thread i for row i.
//
// Arithmetic: the reference's statement order, as in the LDS engine, so the results are bit-identical to the CPU path.
//   gt[i]  = left fold of Q[i][j] * g[j], j ascending, by thread i (Arr::dot_mv, src/arr.rs:426-442)
//   omega  = left fold of g[j] * gt[j] by one lane (Arr::dot, :443-451); the products are formed by thread j beforehand,
//            which changes no bit: multiply and add are never contracted (-ffp-contract=off)
//   rank-1 : Q[r][c] = L(max, min) - (sigma/omega * gt[max]) * gt[min], L the lower-triangle element (src/ell.rs:117-128),
//            then `* kappa_new` with no_defer_trick (:132-135)
//
// Coalescing rests on symmetry.  A lane per row over a row-major matrix would read addresses n doubles apart, so thread i
// walks COLUMN i instead (element (a, i) for a = 0, 1, ...: consecutive lanes, consecutive addresses).  For a matrix that is
// symmetric to the bit, column i holds row i's values in row i's order, and every element of the rank-1 reads itself.  Each
// ellipsoid carries a flag (sym[b]) that says whether its matrix is symmetric to the bit: set by the constructors (identity
// and diag: yes; a matrix from the caller or a cloned handle: compared bit by bit by k_bs_symcheck), and set by the first
// successful cut, which mirrors the lower triangle as the reference does.  While the flag is clear the product walks the true
// rows (uncoalesced) and the rank-1 takes its input from the lower triangle only, in two phases with a barrier between.
//
// Fusion: when cut k succeeds on a symmetric matrix and cut k + 1 follows in the same launch, the sweep that applies cut k
// also folds cut k + 1's product: thread i accumulates Q_new[a][i] * g_next[a] over a ascending, which is row i's fold
// because Q_new is symmetric to the bit.  Bytes per ellipsoid, with n^2 doubles = 8 n^2 bytes per matrix pass:
//   first cut of a launch, or a cut after a failed one     8 n^2 (product)  + 16 n^2 (sweep, read + write)  = 24 n^2
//   a cut whose predecessor succeeded                                          16 n^2 (sweep)                = 16 n^2
//   a failed cut                                            the product it needed (8 n^2 or 0), no sweep
// so K successful cuts in a launch move (16 K + 8) n^2 bytes per ellipsoid, 24 n^2 at K = 1.
//
// In the symmetric state a thread only ever touches its own column of the matrix, so there is no cross-thread dependence
// through global memory at all; nothing here waits on memory words, uses atomics or talks to another workgroup.
#pragma once

#include "ell_kernels.hpp"

namespace ellhip {

struct BatchStreamedParams {
    long long B;  // ellipsoids
    int n;        // dimension, 1..1024
    int np;       // LDS array pitch in doubles (>= n)
    int K;        // cuts per ellipsoid in this launch
    int no_defer_trick;
};

constexpr int BATCH_STREAMED_NMAX = 1024;

__host__ __device__ inline int batch_streamed_np(int n) { return (n + 1) & ~1; }
// doubles of LDS of one workgroup: g (two buffers: this cut's and the next one's), gt, sigma/omega * gt, g * gt, 8 scalars
__host__ __device__ inline size_t batch_streamed_lds_doubles(int n) { return 5 * (size_t)batch_streamed_np(n) + 8; }

// The rank-1 of a successful cut over column i of a matrix that is symmetric to the bit, eight rows in flight; with FUSE the
// fold of the next cut's product rides along.  Returns that fold (0.0 without FUSE).
template <bool FUSE>
__device__ __forceinline__ double bs_sweep(double* __restrict__ col, const int n, const int i, const double* gt,
                                           const double* sg, const bool scaled, const double scale, const double* gn) {
    const double gti = gt[i], sgi = sg[i];
    double acc = 0.0;
    auto one = [&](const int a, const double q) {
        const bool low = a <= i;               // (max, min) = (i, a) on and above the diagonal of column i, (a, i) below
        const double m1 = low ? sgi : sg[a];   // sigma/omega * gt[max]                                     src/ell.rs:117
        const double m2 = low ? gt[a] : gti;   // gt[min]
        double v = q - m1 * m2;                //                                                           :121
        if (scaled) v = v * scale;             //                                                           :132-135
        col[(size_t)a * n] = v;
        if (FUSE) acc += v * gn[a];            // row i's fold of the next product: Q_new[i][a] = Q_new[a][i]
    };
    int a = 0;
    for (; a + 8 <= n; a += 8) {
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = col[(size_t)(a + u) * n];  // the loads run ahead, the adds stay in order
#pragma unroll
        for (int u = 0; u < 8; ++u) one(a + u, q[u]);
    }
    for (; a < n; ++a) one(a, col[(size_t)a * n]);
    return acc;
}

// gt[i] = sum_j Q[i][j] g[j], left fold.  p walks row i with stride 1 (true rows) or column i with stride n (symmetric).
__device__ __forceinline__ double bs_product(const double* __restrict__ p, const size_t stride, const int n, const double* g) {
    double acc = 0.0;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        double q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = p[(size_t)(j + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += q[u] * g[j + u];
    }
    for (; j < n; ++j) acc += p[(size_t)j * stride] * g[j];
    return acc;
}

// The scalar stage of one cut, by one lane: omega, tsq, the cut's coefficients, and what the centre, the rank-1 and kappa
// take from them.  sc: [0] rho/omega  [1] sigma/omega  [2] scale  [3] status  [4] kappa  [5] tsq; pr[j] = g[j] * gt[j].
__device__ __forceinline__ int bs_scalar_stage(double* sc, const double* pr, const int n, const int no_defer_trick,
                                               const EllCalcDev& calc, const int kind, const double b0, const int hb1,
                                               const double b1) {
    double omega = 0.0;  //                                                                                src/ell.rs:103
    for (int j = 0; j < n; ++j) omega += pr[j];
    const double kap = sc[4];
    const double t = kap * omega;  //                                                                      :105
    Coef cf;
    const int st = calc.dispatch(kind, b0, hb1, b1, t, cf);  //                                            :106
    sc[5] = t;
    sc[3] = (double)st;
    if (st == ST_SUCCESS) {
        sc[0] = cf.rho / omega;    //                                                                      :112
        sc[1] = cf.sigma / omega;  //                                                                      :117
        const double knew = kap * cf.delta;  //                                                            :130
        if (no_defer_trick) {      //                                                                      :132-135
            sc[2] = knew;
            sc[4] = 1.0;
        } else {
            sc[2] = 1.0;
            sc[4] = knew;
        }
    }
    return st;
}

// The rank-1 of a successful cut on a matrix that is not symmetric yet (a matrix from the caller before its first successful
// cut): the lower triangle and the diagonal update themselves, then the upper triangle is their mirror image (:119-128).
// Collective: one barrier inside.
__device__ __forceinline__ void bs_sweep_mirror(double* Qb, const int n, const int i, const bool active,
                                                const double* gt, const double* sg, const bool scaled, const double scale) {
    double* col = Qb + (active ? i : 0);
    if (active) {
        const double gti = gt[i];
        for (int r = i; r < n; ++r) {
            double v = col[(size_t)r * n] - sg[r] * gti;
            if (scaled) v = v * scale;
            col[(size_t)r * n] = v;
        }
    }
    __syncthreads();  // the workgroup's own stores to Qb are visible to its loads after the barrier
    if (active) {
        const double* row = Qb + (size_t)i * n;
        for (int r = 0; r < i; ++r) col[(size_t)r * n] = row[r];
    }
}

// Cut k of ellipsoid b: kinds / beta arrays are [K][B], grads [K][B][n]; status / tsq outputs [K][B].  One workgroup per
// ellipsoid, blockDim.x = n rounded up to a multiple of 64, dynamic LDS = batch_streamed_lds_doubles(n) doubles.  One
// instantiation for every n: bounded for 1024 threads it needs 73 VGPRs, fewer than a variant bounded for 256 was given.
__global__ __launch_bounds__(1024) void k_batch_streamed_update(
    BatchStreamedParams P, double* __restrict__ Q, double* __restrict__ xc, double* __restrict__ kappa,
    double* __restrict__ tsq, int* __restrict__ sym, const int* __restrict__ kinds, const double* __restrict__ grads,
    const double* __restrict__ beta0, const int* __restrict__ has_b1, const double* __restrict__ beta1,
    int* __restrict__ status_out, double* __restrict__ tsq_out, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, np = P.np;
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    double* gbuf = sm;            // [2][np]
    double* gt = sm + 2 * np;
    double* sg = gt + np;
    double* pr = sg + np;
    double* sc = pr + np;  // [0] rho/omega  [1] sigma/omega  [2] scale  [3] status  [4] kappa  [5] tsq  [6] symmetric
    double* Qb = Q + (size_t)b * n * n;
    double* col = Qb + (active ? i : 0);

    double xci = 0.0;
    if (active) {
        xci = xc[b * n + i];
        gbuf[i] = grads[b * n + i];
    }
    if (i == 0) {
        sc[4] = kappa[b];
        sc[5] = tsq[b];
        sc[6] = (double)sym[b];
    }
    __syncthreads();

    bool have_gt = false;  // acc already holds this cut's gt[i], folded by the sweep of the cut before
    double acc = 0.0;
    for (int k = 0; k < P.K; ++k) {
        const long long cut = (long long)k * P.B + b;
        const double* g = gbuf + (k & 1) * np;
        double* gn = gbuf + ((k + 1) & 1) * np;
        const bool more = k + 1 < P.K;
        if (more && active) gn[i] = grads[(cut + P.B) * n + i];
        const bool symm = sc[6] != 0.0;
        if (active) {
            if (!have_gt) acc = symm ? bs_product(col, (size_t)n, n, g) : bs_product(Qb + (size_t)i * n, 1, n, g);  // :102
            gt[i] = acc;
            pr[i] = g[i] * acc;
        }
        __syncthreads();
        if (i == 0) {
            const int st = bs_scalar_stage(sc, pr, n, P.no_defer_trick, calc, kinds[cut], beta0[cut], has_b1[cut], beta1[cut]);
            status_out[cut] = st;
            if (tsq_out) tsq_out[cut] = sc[5];
        }
        __syncthreads();
        const bool ok = sc[3] == (double)ST_SUCCESS;
        have_gt = false;
        if (ok) {
            if (active) {
                xci = xci - sc[0] * gt[i];  //                                                             :113-115
                sg[i] = sc[1] * gt[i];
            }
            __syncthreads();
            const bool scaled = P.no_defer_trick != 0;
            const double scale = sc[2];
            if (symm) {
                if (active) {
                    if (more) acc = bs_sweep<true>(col, n, i, gt, sg, scaled, scale, gn);
                    else (void)bs_sweep<false>(col, n, i, gt, sg, scaled, scale, gn);
                }
                have_gt = more;
            } else {
                bs_sweep_mirror(Qb, n, i, active, gt, sg, scaled, scale);
                if (i == 0) sc[6] = 1.0;
            }
        }
        __syncthreads();
    }

    if (active) xc[b * n + i] = xci;
    if (i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
        sym[b] = sc[6] != 0.0 ? 1 : 0;
    }
}

// sym[b] = 1 when Q[b] is symmetric to the bit (NaNs by their bit patterns), else 0.  One workgroup per ellipsoid.
__global__ __launch_bounds__(256) void k_bs_symcheck(const double* __restrict__ Q, int n, int* __restrict__ sym) {
    __shared__ int bad;
    const long long* Qb = reinterpret_cast<const long long*>(Q) + (size_t)blockIdx.x * n * n;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int r = 1; r < n; ++r)
        for (int c = threadIdx.x; c < r; c += blockDim.x)
            if (Qb[(size_t)r * n + c] != Qb[(size_t)c * n + r]) mine = 1;
    if (mine) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) sym[blockIdx.x] = bad ? 0 : 1;
}

__global__ __launch_bounds__(256) void k_bs_fill_int(int* __restrict__ p, long long count, int value) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < count; idx += (long long)gridDim.x * blockDim.x)
        p[idx] = value;
}

}  // namespace ellhip
