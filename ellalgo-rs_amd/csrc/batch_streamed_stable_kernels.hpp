// batch_streamed_stable_kernels.hpp -- many independent EllStable spaces of up to 1024 dimensions, streamed from HBM
// (include/ellhip_batch_streamed_stable.h).
//
// The streamed engine's launch shape (batch_streamed_kernels.hpp: one workgroup per ellipsoid, thread i for index i, K cuts
// per launch) around EllStable::update_core (src/ell_stable.rs:52-125), with the packed buffer left in HBM: diagonal = D and
// strict upper = the factor U at the reference's positions, the scratch triangle at bss_scratch_slot
// (batch_streamed_stable_layout.hpp), so that all three walks over it are unit-stride.  LDS holds three n-vectors and the
// scalars of the one ellipsoid.
//
// Mapping: batch_stable_apply.hpp's, moved from LDS to HBM.  It parallelises over independent outputs only, never inside a
// fold, so every element is formed by the same expression from the same operands in the same order as in
// k_batch_update_stable and in the oracle; compiled with -ffp-contract=off the results are BIT-IDENTICAL to the CPU
// arithmetic, the scratch triangle included.
//
//   forward solve   right-looking: at step j thread j publishes its final w[j], z_j = w_j * D[j] and gg_j = z_j * w_j; after
//   (:61-83)        one barrier thread i > j forms val = U[j][i] * w[j], stores it as S[i][j] and does w_i -= val in a
//                   register, so w_i is still folded in ascending j.  The factor is read-only in this phase: a thread's
//                   loads of U[j+4..j+7][i] are issued while the barrier chain works through U[j..j+3][i].
//   scalar stage    thread 0: omega folded from +0.0 in ascending i, tsq = kappa * omega, the dispatch, the status.  A failed
//   (:78-90)        cut ends here: tsq and the scratch triangle are all it changed.  On success the same lane runs the add
//                   chain temp_j = oldt + gg[j], oldt = temp_j (:111, :118) and leaves temp_j in the dead w slot; the two
//                   divisions of step j, beta2_j = z[j] / temp_j and oldt_j / temp_j (:112-113), have no chain between them
//                   and are formed by thread j afterwards, beta2_j into the dead gg slot.
//   factor update   thread l owns column l: U[j][l] += beta2_j * S[l][j] for j < l, eight loads in flight, and
//   (:107-121)      D[l] *= oldt_l / temp_l.  It reads scratch and writes the upper triangle and the diagonal.
//   back solve      at the same time, by wave 0, in place on z (g_t = z, :93-98).  The fold for g_t[c] starts with the term
//   (:93-98)        that needs g_t[c+1], so the chain of n (n-1) / 2 subtractions stays serial in c and in j.  The wave's 64
//                   lanes fetch 64 consecutive scratch elements of column c per load (BSS_PF loads in flight, across column
//                   ends), each lane forms its product S[j][c] * g_t[j] -- rounded separately, so no bit changes -- and
//                   parks it in LDS, and the chain takes the 64 products in ascending j; every lane of the wave carries
//                   the same running value.  It reads scratch only, which the factor update never writes.
//   xc, kappa       xc[i] -= (rho / omega) * g_t[i] per thread (:101-104); kappa *= delta on thread 0 (:122).
//
// Bytes per successful cut and ellipsoid, 8 n^2 per full matrix pass: the factor read 4 n^2, the scratch written 4 n^2 and
// read twice 8 n^2, the factor read and written 8 n^2: 24 n^2 in all; a failed cut 8 n^2.
//
// n + 4 workgroup barriers per cut; every loop is bounded by n and K; nothing here waits on a memory word, uses atomics or
// talks to another workgroup.
#pragma once

#include "batch_streamed_kernels.hpp"
#include "batch_streamed_stable_layout.hpp"

namespace ellhip {

// doubles of LDS of one workgroup: w (then temp), z (then g_t), gg (then beta2), 8 scalars, the back solve's 64 products
__host__ __device__ inline size_t batch_streamed_stable_lds_doubles(int n) { return 3 * (size_t)batch_streamed_np(n) + 72; }

constexpr int BSS_CHUNK = 4;  // rows of the factor in a chunk of loads; the forward solve has two chunks in flight
constexpr int BSS_PF = 4;     // 64-element pieces of the scratch triangle the back solve keeps in flight
constexpr int BSS_FOLD = 16;  // products the back solve's chain takes from LDS at a time

// g_t = inv(L') z in place on z, by one whole wave (all 64 lanes active), src/ell_stable.rs:93-98.  Column c = n-2 .. 0 has
// the m = n-1-c terms S[j][c] * g_t[j], j = c+1 .. n-1, and S[j][c] is element m-1-(j-c-1) of row m of the buffer
// (bss_scratch_slot).  A piece is up to 64 consecutive terms of one column, one per lane: the lanes park their products in
// `stage` (64 doubles of LDS that only this wave touches: a wave's LDS accesses execute in order, so no barrier) and every
// lane folds them in ascending j, so every lane carries the same running value; a short piece is folded up to the next
// multiple of BSS_FOLD over parked zeros.  The loads are unconditional (a lane with no term reads the buffer's first element):
// under a branch they would turn every wait into a wait for all of them.
__device__ __forceinline__ void bss_back_solve(const double* __restrict__ Qb, const int n, const int lane, double* z,
                                               double* stage) {
    if (n < 2) return;
    int lc = n - 2, lq = 0;  // the piece the next load fetches
    auto fetch = [&]() -> double {
        const int m = n - 1 - lc, e = 64 * lq + lane;
        const double* from = (lc >= 0 && e < m) ? Qb + ((size_t)m * n + (m - 1 - e)) : Qb;
        if (64 * (lq + 1) >= m) {
            lc -= 1;
            lq = 0;
        } else {
            lq += 1;
        }
        return *from;
    };
    double s[BSS_PF];
#pragma unroll
    for (int u = 0; u < BSS_PF; ++u) s[u] = fetch();
    int c = n - 2, q = 0;  // the piece the chain takes next
    double acc = 0.0, zprev = z[n - 1];
    while (c >= 0) {
#pragma unroll
        for (int u = 0; u < BSS_PF; ++u) {
            if (c < 0) break;
            const int m = n - 1 - c, e0 = 64 * q, e = e0 + lane;
            if (q == 0) acc = z[c];
            double p = 0.0;  // a lane past the column's end parks +0.0, and x - (+0.0) is x to the bit for every x
            if (e < m) p = s[u] * (e == 0 ? zprev : z[c + 1 + e]);  // g_t[c+1] has just left the chain
            stage[lane] = p;
            s[u] = fetch();
            __builtin_amdgcn_wave_barrier();
            // BSS_FOLD products at a time: their reads from LDS all go out ahead of the subtractions
            const int cnt = m - e0;
#pragma unroll
            for (int t0 = 0; t0 < 64; t0 += BSS_FOLD) {
                if (t0 >= cnt) break;
                double pr[BSS_FOLD];
#pragma unroll
                for (int t = 0; t < BSS_FOLD; ++t) pr[t] = stage[t0 + t];
#pragma unroll
                for (int t = 0; t < BSS_FOLD; ++t) acc -= pr[t];
            }
            __builtin_amdgcn_wave_barrier();
            if (e0 + 64 >= m) {
                if (lane == 0) z[c] = acc;
                zprev = acc;
                c -= 1;
                q = 0;
            } else {
                q += 1;
            }
        }
    }
}

// One cut of EllStable::update_core on the ellipsoid at Qb, by the whole workgroup.  Thread i < n (`active`) brings gi, its
// element of the gradient, and xci, its xc[i]; thread 0 runs the scalar stage on the cut (kind, b0, hb1, b1) and hands the
// status and tsq to `emit`.  w, z, gg: np doubles of LDS each; sc: [0] rho/omega  [3] status  [4] kappa  [5] tsq
// [6] omega/mu  [8..71] the back solve's staging.  The caller has synchronised since anyone touched w, z, gg or sc; the
// function ends with a barrier.
template <class Emit>
__device__ __forceinline__ void bs_stable_cut(double* __restrict__ Qb, const int n, const int i, const bool active,
                                              const double gi, double* w, double* z, double* gg, double* sc, double& xci,
                                              const EllCalcDev& calc, const int kind, const double b0, const int hb1,
                                              const double b1, Emit emit) {
    const int ia = active ? i : 0;
    double* ucol = Qb + ia;                                // U[j][i] = ucol[j * n]
    double* srow = Qb + bss_scratch_slot(n, ia, 0);        // S[i][j] = srow[-j * n]
    double* dptr = Qb + (size_t)ia * n + ia;
    const double dl = active ? *dptr : 0.0;
    // ---- forward solve, right-looking                                     src/ell_stable.rs:61-69
    double wi = gi;
    // (a lane loads unconditionally, rows it does not need from the buffer's first element: a load under a branch would
    // make every wait in the chain below a wait for all of them)
    const double* up = ucol;  // the next row of column i to fetch
    auto rows = [&](double* dst, const int j0) {
#pragma unroll
        for (int u = 0; u < BSS_CHUNK; ++u) {
            const double* from = (active && j0 + u < i) ? up : Qb;
            dst[u] = *from;
            up += n;
        }
    };
    double* sp = srow;  // S[i][j] of the step at hand
    auto step = [&](const int j, const double uji) {
        if (i == j) {  // w[j] is final                                      :72-80
            w[j] = wi;
            const double zi = wi * dl;
            z[j] = zi;
            gg[j] = zi * wi;
        }
        __syncthreads();
        if (active && i > j) {
            const double val = uji * w[j];
            *sp = val;  // "keep for rank-one update"
            wi -= val;
        }
        sp -= n;
    };
    double cur[BSS_CHUNK], nxt[BSS_CHUNK];
    rows(cur, 0);
    int j = 0;
    for (; j + BSS_CHUNK <= n - 1; j += BSS_CHUNK) {
        rows(nxt, j + BSS_CHUNK);  // in flight while the barrier chain below works through cur
#pragma unroll
        for (int u = 0; u < BSS_CHUNK; ++u) step(j + u, cur[u]);
#pragma unroll
        for (int u = 0; u < BSS_CHUNK; ++u) cur[u] = nxt[u];
    }
    for (; j < n - 1; ++j) step(j, (active && j < i) ? ucol[(size_t)j * n] : 0.0);
    if (i == n - 1) {
        const double zi = wi * dl;
        z[i] = zi;
        gg[i] = zi * wi;
    }
    __syncthreads();
    // ---- omega, EllCalc and the add chain of the rank-one update
    if (i == 0) {
        double omega = 0.0;  //                                              :81-83
#pragma unroll 8
        for (int j = 0; j < n; ++j) omega += gg[j];
        const double kap = sc[4];
        const double t = kap * omega;  //                                    :85
        Coef cf;
        const int st = calc.dispatch(kind, b0, hb1, b1, t, cf);  //          :86
        sc[5] = t;
        sc[3] = (double)st;
        if (st == ST_SUCCESS) {  //                                          :88-90
            sc[0] = cf.rho / omega;  //                                      :101
            const double mu = cf.sigma / (1.0 - cf.sigma);  //               :107
            double oldt = omega / mu;  //                                    :108
            sc[6] = oldt;
#pragma unroll 8
            for (int j = 0; j < n; ++j) {  //                                :111, :118, :120
                oldt = oldt + gg[j];
                w[j] = oldt;
            }
            sc[4] = kap * cf.delta;  //                                      :122
        }
        emit(st, t);
    }
    __syncthreads();
    const bool ok = sc[3] == (double)ST_SUCCESS;
    if (ok) {
        double ratio = 0.0;
        if (active) {
            const double temp = w[i];
            const double oldt = i > 0 ? w[i - 1] : sc[6];
            if (i < n - 1) gg[i] = z[i] / temp;  // beta2                    :112
            ratio = oldt / temp;  //                                         :113, :121
        }
        __syncthreads();
        if (active) {  // column i of the factor and the diagonal element    :113-117, :121
            double* uq = ucol;
            const double* sq = srow;
            int j = 0;
            for (; j + BSS_CHUNK <= i; j += BSS_CHUNK) {
                double u[BSS_CHUNK], sv[BSS_CHUNK];
#pragma unroll
                for (int r = 0; r < BSS_CHUNK; ++r) {
                    u[r] = uq[(size_t)r * n];
                    sv[r] = *sq;
                    sq -= n;
                }
#pragma unroll
                for (int r = 0; r < BSS_CHUNK; ++r) {
                    *uq = u[r] + gg[j + r] * sv[r];
                    uq += n;
                }
            }
            for (; j < i; ++j) {
                *uq = *uq + gg[j] * *sq;
                uq += n;
                sq -= n;
            }
            *dptr = dl * ratio;
        }
        if (i < 64) bss_back_solve(Qb, n, i, z, sc + 8);  //                         :93-98
        __syncthreads();
        if (active) xci = xci - sc[0] * z[i];  //                            :101-104
    }
    __syncthreads();
}

// Cut k of ellipsoid b: kinds / beta arrays are [K][B], grads [K][B][n]; status / tsq outputs [K][B].  One workgroup per
// ellipsoid, blockDim.x = n rounded up to a multiple of 64, dynamic LDS = batch_streamed_stable_lds_doubles(n) doubles (at
// most 24.6 KiB).  Bounded for 1024 threads (128 VGPRs a wave) the compiler's resource-usage remark reads: 123 VGPRs, no
// scratch memory (ScratchSize 0, no VGPR spilled); 23 SGPRs are parked in VGPR lanes, all of them around the scalar stage,
// none inside the forward solve, the factor update or the back solve.
__global__ __launch_bounds__(1024) void k_batch_streamed_update_stable(
    BatchStreamedParams P, double* __restrict__ Q, double* __restrict__ xc, double* __restrict__ kappa,
    double* __restrict__ tsq, const int* __restrict__ kinds, const double* __restrict__ grads,
    const double* __restrict__ beta0, const int* __restrict__ has_b1, const double* __restrict__ beta1,
    int* __restrict__ status_out, double* __restrict__ tsq_out, EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, np = P.np;
    const int i = threadIdx.x;
    const long long b = blockIdx.x;
    const bool active = i < n;
    double* w = sm;
    double* z = w + np;
    double* gg = z + np;
    double* sc = gg + np;
    double* Qb = Q + (size_t)b * n * n;

    double xci = 0.0, gi = 0.0;
    if (active) {
        xci = xc[b * n + i];
        gi = grads[b * n + i];
    }
    if (i == 0) {
        sc[4] = kappa[b];
        sc[5] = tsq[b];
    }
    __syncthreads();

    for (int k = 0; k < P.K; ++k) {
        const long long cut = (long long)k * P.B + b;
        double gnext = 0.0;  // the next cut's gradient travels while this cut runs
        if (k + 1 < P.K && active) gnext = grads[(cut + P.B) * n + i];
        bs_stable_cut(Qb, n, i, active, gi, w, z, gg, sc, xci, calc, kinds[cut], beta0[cut], has_b1[cut], beta1[cut],
                      [&](const int st, const double t) {
                          status_out[cut] = st;
                          if (tsq_out) tsq_out[cut] = t;
                      });
        gi = gnext;
    }

    if (active) xc[b * n + i] = xci;
    if (i == 0) {
        kappa[b] = sc[4];
        tsq[b] = sc[5];
    }
}

// The reference's packed buffer <-> the engine's (batch_streamed_stable_layout.hpp), in place.  The map swaps S[i][j] with
// the element at its slot and is its own inverse, so one kernel serves both directions; elements with i + j = n - 1 stay.
// A workgroup takes the pairs whose first member (i > j, i + j < n - 1) lies in its 32 x 32 tile, reads both members of each
// pair along rows, turns them in LDS and writes them along rows again.  blockIdx.y / .z: the tile; blockIdx.x strides over
// the ellipsoids; 256 threads.
constexpr int BSS_TILE = 32;
__global__ __launch_bounds__(256) void k_bss_rotate(double* __restrict__ Q, const long long B, const int n) {
    __shared__ double first[BSS_TILE][BSS_TILE + 1], second[BSS_TILE][BSS_TILE + 1];
    const int i0 = blockIdx.y * BSS_TILE, j0 = blockIdx.z * BSS_TILE;
    if (j0 > i0 || i0 + j0 >= n - 1) return;  // no first member in this tile
    const int tx = threadIdx.x % BSS_TILE, ty0 = threadIdx.x / BSS_TILE;
    auto is_first = [&](const int i, const int j) { return i < n && j < i && i + j < n - 1; };
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        double* Qb = Q + (size_t)b * n * n;
        for (int ty = ty0; ty < BSS_TILE; ty += 256 / BSS_TILE) {
            if (is_first(i0 + ty, j0 + tx)) first[ty][tx] = Qb[(size_t)(i0 + ty) * n + (j0 + tx)];
            if (is_first(i0 + tx, j0 + ty)) second[tx][ty] = Qb[bss_scratch_slot(n, i0 + tx, j0 + ty)];
        }
        __syncthreads();
        for (int ty = ty0; ty < BSS_TILE; ty += 256 / BSS_TILE) {
            if (is_first(i0 + ty, j0 + tx)) Qb[(size_t)(i0 + ty) * n + (j0 + tx)] = second[ty][tx];
            if (is_first(i0 + tx, j0 + ty)) Qb[bss_scratch_slot(n, i0 + tx, j0 + ty)] = first[tx][ty];
        }
        __syncthreads();
    }
}

}  // namespace ellhip
