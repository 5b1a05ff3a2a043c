// batch_stable_kernels.hpp -- the batched small-n engine for EllStable (include/ellhip_batch.h).
//
// Same storage and launch contract as k_batch_update (batch_kernels.hpp): B packed EllStable buffers side by side in HBM
// ([B][n][n] row-major: diagonal = D, strict upper = the factor U with mq.at(j, i) = L[i][j], strict lower = scratch), one
// launch applies K cuts to each of them out of LDS and writes them back -- 16 n^2 / K + 8 n bytes of HBM per update.
//
// Mapping: ONE LANE PER ELLIPSOID for the whole update.  EllStable::update_core (src/ell_stable.rs:52-125) is two dependent
// chains of n (n - 1) / 2 subtractions each (the forward solve's w[i] folds, and the back solve, whose fold for g_t[i-1]
// starts with the term that needs g_t[i]) plus a factor update whose only serial part is the `temp` add chain.  A lane
// that owns an ellipsoid keeps the running value of each fold in a register and streams its operands from LDS; the loads
// do not depend on the chain, so they are issued ahead of the subtractions.  Throughput comes from running the chains of
// many ellipsoids side by side: every owner lane executes the same instruction stream (n is uniform), so a wave is fully
// used as long as it owns 64 ellipsoids, and the LDS budget per workgroup is sized so that four one-wave workgroups (one
// per SIMD) fit on a CU.  Splitting the parallel phases over rows would need a barrier per step of the right-looking
// forward solve and would leave the back solve -- a third of the work and the longest chain -- on one lane anyway.
//
// Arithmetic: statement for statement the reference's (the oracle's orc_ellstable_update restates it), compiled with
// -ffp-contract=off, so the results are BIT-IDENTICAL to the CPU arithmetic, the scratch triangle included.  The z, gg and
// omega loops are fused into the forward solve and the xc update into the back solve: each element is formed by the same
// expression from the same operands, and omega is still folded in ascending i from +0.0.
#pragma once

#include "batch_kernels.hpp"

namespace ellhip {

// doubles of LDS one EllStable ellipsoid needs: the buffer (rows of batch_pitch), w (reused as g_t), z, gg, xc.  Odd, so
// that the owner lanes -- one ellipsoid each, same offset -- hit different LDS banks.
__host__ __device__ inline size_t batch_stable_lds_doubles(int n) {
    return ((size_t)n * batch_pitch(n) + 4 * (size_t)n) | 1;
}
constexpr int BATCH_ST_T = 64;      // threads per workgroup: one wave
constexpr int BATCH_ST_GREGS = 8;   // gradient prefetch registers per lane: epw * n <= BATCH_ST_GREGS * BATCH_ST_T
// Loops that store into the same LDS array they read are run in chunks whose loads all come first: the compiler cannot
// prove that a scratch store and the next element's load differ, so a plain loop waits for every load in turn.
constexpr int BATCH_ST_CHUNK = 8;

// Copy `count` contiguous doubles of per-ellipsoid vectors ([e][i] dense in HBM) to / from LDS slot `off` of each
// ellipsoid's block of `per` doubles.
template <int T, bool TO_LDS>
__device__ __forceinline__ void batch_vec_copy(double* __restrict__ sm, double* __restrict__ glob, int count, int n,
                                               int per, int off, int tid) {
    int e = tid / n, i = tid - e * n;
    const int de = T / n, di = T - de * n;
    for (int idx = tid; idx < count; idx += T) {
        double* l = sm + (size_t)e * per + off + i;
        if (TO_LDS) *l = glob[idx];
        else glob[idx] = *l;
        e += de;
        i += di;
        if (i >= n) {
            i -= n;
            e += 1;
        }
    }
}

// Cut k of ellipsoid b: kinds / beta arrays are [K][B], grads [K][B][n]; status / tsq outputs [K][B].
__global__ __launch_bounds__(BATCH_ST_T) void k_batch_update_stable(
    BatchParams P, double* __restrict__ Q, double* __restrict__ xc, double* __restrict__ kappa, double* __restrict__ tsq,
    const int* __restrict__ kinds, const double* __restrict__ grads, const double* __restrict__ beta0,
    const int* __restrict__ has_b1, const double* __restrict__ beta1, int* __restrict__ status_out,
    double* __restrict__ tsq_out, EllCalcDev calc) {
    constexpr int T = BATCH_ST_T;
    extern __shared__ double sm[];
    const int n = P.n, pitch = P.pitch;
    const int tid = threadIdx.x;
    const int per = (int)batch_stable_lds_doubles(n);
    const int o_w = n * pitch, o_z = o_w + n, o_gg = o_z + n, o_xc = o_gg + n;
    const long long b_first = (long long)blockIdx.x * P.epw;
    const int nb = (int)((P.B - b_first < P.epw) ? P.B - b_first : P.epw);
    const bool owner = tid < nb;  // lane tid runs every step of ellipsoid b_first + tid
    const long long b = b_first + tid;

    // ---- buffers and xc -> LDS (coalesced over the workgroup's contiguous ellipsoids)
    batch_copy<T, true>(sm, Q + b_first * (long long)n * n, nb * n * n, n, pitch, per, tid);
    batch_vec_copy<T, true>(sm, xc + b_first * n, nb * n, n, per, o_xc, tid);
    double kap = 0.0, ts = 0.0;
    if (owner) {
        kap = kappa[b];
        ts = tsq[b];
    }

    // The workgroup's gradients of one cut are nb * n contiguous doubles; they are loaded one cut ahead into registers
    // (their LDS destinations are the same for every cut).
    const int gcount = nb * n;
    int goff[BATCH_ST_GREGS];
    double gnext[BATCH_ST_GREGS];
#pragma unroll
    for (int r = 0; r < BATCH_ST_GREGS; ++r) {
        const int idx = tid + r * T;
        goff[r] = 0;
        gnext[r] = 0.0;
        if (idx < gcount) {
            const int e = idx / n;
            goff[r] = e * per + o_w + (idx - e * n);
            gnext[r] = grads[b_first * n + idx];
        }
    }
    int kind_next = 0, hb1_next = 0;
    double b0_next = 0.0, b1_next = 0.0;
    if (owner) {
        kind_next = kinds[b];
        b0_next = beta0[b];
        hb1_next = has_b1[b];
        b1_next = beta1[b];
    }
    double* q = sm + (size_t)(owner ? tid : 0) * per;
    double* w = q + o_w;  // w = inv(L) g; once z and gg are formed, the same slot holds g_t
    double* z = q + o_z;
    double* gg = q + o_gg;
    double* xl = q + o_xc;

    for (int k = 0; k < P.K; ++k) {
        const long long cut = (long long)k * P.B + b;
        const int kind_k = kind_next, hb1_k = hb1_next;
        const double b0_k = b0_next, b1_k = b1_next;
        __syncthreads();  // (the previous cut's owners are done with their w slots)
#pragma unroll
        for (int r = 0; r < BATCH_ST_GREGS; ++r)
            if (tid + r * T < gcount) sm[goff[r]] = gnext[r];
        __syncthreads();
        if (k + 1 < P.K) {
            const double* gn = grads + ((long long)(k + 1) * P.B + b_first) * n;
#pragma unroll
            for (int r = 0; r < BATCH_ST_GREGS; ++r)
                if (tid + r * T < gcount) gnext[r] = gn[tid + r * T];
            if (owner) {
                const long long nxt = cut + P.B;
                kind_next = kinds[nxt];
                b0_next = beta0[nxt];
                hb1_next = has_b1[nxt];
                b1_next = beta1[nxt];
            }
        }
        if (!owner) continue;

        // forward solve, src/ell_stable.rs:61-69 (products parked in the scratch triangle), with z = D w (:72-75),
        // gg = z w and the omega fold (:78-83) as each w[i] becomes final
        double omega = 0.0;
        for (int i = 0; i < n; ++i) {
            double wi = w[i];
            double* srow = q + (size_t)i * pitch;
            const double* ucol = q + i;
            int j = 0;
            for (; j + BATCH_ST_CHUNK <= i; j += BATCH_ST_CHUNK) {
                double u[BATCH_ST_CHUNK], wj[BATCH_ST_CHUNK];
#pragma unroll
                for (int r = 0; r < BATCH_ST_CHUNK; ++r) {
                    u[r] = ucol[(size_t)(j + r) * pitch];
                    wj[r] = w[j + r];
                }
#pragma unroll
                for (int r = 0; r < BATCH_ST_CHUNK; ++r) {
                    const double val = u[r] * wj[r];
                    srow[j + r] = val;
                    wi -= val;
                }
            }
            for (; j < i; ++j) {
                const double val = ucol[(size_t)j * pitch] * w[j];
                srow[j] = val;
                wi -= val;
            }
            w[i] = wi;
            const double zi = wi * srow[i];
            z[i] = zi;
            const double ggi = zi * wi;
            gg[i] = ggi;
            omega += ggi;
        }
        const double t = kap * omega;  //                                      :85
        ts = t;
        Coef cf;
        const int st = calc.dispatch(kind_k, b0_k, hb1_k, b1_k, t, cf);  //    :86
        status_out[cut] = st;
        if (tsq_out) tsq_out[cut] = t;
        if (st != ST_SUCCESS) continue;  //                                    :88-90

        // back solve on the scratch triangle, g_t = z (:93-98), and xc -= (rho / omega) g_t (:101-104)
        const double ro = cf.rho / omega;
        double* gt = w;
        gt[n - 1] = z[n - 1];
        xl[n - 1] -= ro * z[n - 1];
        for (int i = n - 1; i >= 1; --i) {
            double acc = z[i - 1];
            const double* scol = q + (i - 1);
#pragma unroll 8
            for (int j = i; j < n; ++j) acc -= scol[(size_t)j * pitch] * gt[j];
            gt[i - 1] = acc;
            xl[i - 1] -= ro * acc;
        }

        // rank-one update of the factor (:107-121)
        const double mu = cf.sigma / (1.0 - cf.sigma);
        double oldt = omega / mu;
        for (int j = 0; j < n - 1; ++j) {
            const double temp = oldt + gg[j];
            const double beta2 = z[j] / temp;
            double* urow = q + (size_t)j * pitch;
            urow[j] *= oldt / temp;
            const double* scol = q + j;
            int l = j + 1;
            for (; l + BATCH_ST_CHUNK <= n; l += BATCH_ST_CHUNK) {
                double u[BATCH_ST_CHUNK], sv[BATCH_ST_CHUNK];
#pragma unroll
                for (int r = 0; r < BATCH_ST_CHUNK; ++r) {
                    u[r] = urow[l + r];
                    sv[r] = scol[(size_t)(l + r) * pitch];
                }
#pragma unroll
                for (int r = 0; r < BATCH_ST_CHUNK; ++r) urow[l + r] = u[r] + beta2 * sv[r];
            }
            for (; l < n; ++l) urow[l] += beta2 * scol[(size_t)l * pitch];
            oldt = temp;
        }
        {
            const double temp = oldt + gg[n - 1];
            q[(size_t)(n - 1) * pitch + (n - 1)] *= oldt / temp;
        }
        kap *= cf.delta;  //                                                   :122
    }

    // ---- LDS -> buffers, xc, kappa, tsq
    __syncthreads();
    if (owner) {
        kappa[b] = kap;
        tsq[b] = ts;
    }
    batch_vec_copy<T, false>(sm, xc + b_first * n, nb * n, n, per, o_xc, tid);
    batch_copy<T, false>(sm, Q + b_first * (long long)n * n, nb * n * n, n, pitch, per, tid);
}

}  // namespace ellhip
