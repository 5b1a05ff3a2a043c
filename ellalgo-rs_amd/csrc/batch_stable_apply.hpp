// batch_stable_apply.hpp -- one EllStable cut for the instances of a loop kernel, spread over the n threads of each
// instance (include/ellhip_batch_stable_loops.h).
//
// k_batch_update_stable (batch_stable_kernels.hpp) gives an ellipsoid to ONE lane.  A loop kernel cannot: its oracle owns
// the n threads of an instance (thread (e, i), e = tid / n, i = tid - e * n, as in batch_cut_apply), and they would idle
// while one of them ran the whole update.  batch_stable_cut_apply restates EllStable::update_core
// (src/ell_stable.rs:52-125) on that thread layout, on the same packed buffer in LDS (diagonal = D, strict upper = the
// factor U with mq.at(j, i) = L[i][j], strict lower = scratch, rows of batch_pitch(n)).
//
// The mapping parallelises over independent outputs only, never inside a fold, so every element is formed by the same
// expression from the same operands in the same order as in k_batch_update_stable and in orc_ellstable_update; compiled
// with -ffp-contract=off the results are BIT-IDENTICAL to both, the scratch triangle included:
//
//   forward solve   right-looking: at step j = 0 .. n-2 w[j] is final and published; thread i > j forms
//   (:61-69)        val = U[j][i] * w[j], parks it at scratch [i][j] and does w_i -= val in a register, so w_i is still
//                   folded in ascending j.  One barrier per step.  Thread i forms z_i = w_i * D[i] and gg_i = z_i * w_i
//                   (:72-80) when its w_i becomes final.
//   omega, EllCalc  one scalar lane per instance: omega folded from +0.0 in ascending i (:81-83), tsq = kappa * omega,
//   (:81-90)        the dispatch, the status.  A failed cut ends here: tsq and the scratch triangle are all it changed.
//   temp chain      the same lane: temp = oldt + gg[j], beta2_j = z[j] / temp, oldt / temp, oldt = temp (:107-121); it
//                   leaves beta2_j in the dead w slot and oldt / temp in place of gg[j].
//   back solve      thread 0 of the instance, in place on z (g_t = z, :93-98): the fold for g_t[i-1] starts with the
//                   term that needs g_t[i], so the subtraction chain stays serial.  It reads the scratch triangle and
//                   changes nothing there.
//   factor update   at the same time: thread l owns column l of the factor, U[j][l] += beta2_j * S[l][j] for j < l, and
//   (:107-121)      the diagonal element D[l] *= oldt / temp of step l.  It reads scratch and writes the upper triangle
//                   and the diagonal, which the back solve never touches.
//   xc, kappa       xc[i] -= (rho / omega) * g_t[i] per thread (:101-104); kappa *= delta on the scalar lane (:122).
//
// n + 2 workgroup barriers per update; every loop is bounded by n; no thread waits on another workgroup.
#pragma once

#include "batch_kernels.hpp"

namespace ellhip {

// doubles of LDS one EllStable instance of a loop kernel needs: the buffer, three n-vectors (w, reused for beta2; z,
// reused for g_t; gg, reused for oldt / temp) and the 8 scalars of batch_cut_apply.  Odd, as batch_lds_doubles.
__host__ __device__ inline size_t batch_stable_apply_lds_doubles(int n) {
    return ((size_t)n * batch_pitch(n) + 3 * (size_t)n + 8) | 1;
}

// One cut of EllStable::update_core for the workgroup's instances, out of LDS.  Thread (e, i) belongs to local instance e
// (q: its buffer, w / z / gg / sc: its LDS blocks, xci: its xc[i]); `scalar_lane` t of wave 0 runs the scalar stage for
// local instance t (gg_s, z_s, w_s, sc_s; kind_k, b0_k, hb1_k, b1_k: that instance's cut) and hands its status and tsq to
// `emit`.  The caller has stored the gradient in w and synchronised; the function ends with a barrier.  sc as in
// batch_cut_apply: [0] rho/omega  [3] status  [4] kappa  [5] tsq.
template <class Emit>
__device__ __forceinline__ void batch_stable_cut_apply(const BatchParams& P, const EllCalcDev& calc, const bool active,
                                                       const int i, double* q, double* w, double* z, double* gg, double* sc,
                                                       double& xci, const bool scalar_lane, double* w_s, double* z_s,
                                                       double* gg_s, double* sc_s, const int kind_k, const double b0_k,
                                                       const int hb1_k, const double b1_k, Emit emit) {
    const int n = P.n, pitch = P.pitch;
    // ---- forward solve, right-looking                                     src/ell_stable.rs:61-69
    double wi = active ? w[i] : 0.0;
    double* srow = q + (size_t)i * pitch;
    for (int j = 0; j < n - 1; ++j) {
        if (active && i == j) {  // w[j] is final                            :72-80
            w[j] = wi;
            const double zi = wi * srow[i];
            z[i] = zi;
            gg[i] = zi * wi;
        }
        __syncthreads();
        if (active && i > j) {
            const double val = q[(size_t)j * pitch + i] * w[j];
            srow[j] = val;  // "keep for rank-one update"
            wi -= val;
        }
    }
    if (active && i == n - 1) {
        const double zi = wi * srow[i];
        z[i] = zi;
        gg[i] = zi * wi;
    }
    __syncthreads();
    // ---- omega, EllCalc and the temp chain
    if (scalar_lane) {
        double omega = 0.0;  //                                              :81-83
#pragma unroll 8
        for (int j = 0; j < n; ++j) omega += gg_s[j];
        const double kap = sc_s[4];
        const double t = kap * omega;  //                                    :85
        Coef cf;
        const int st = calc.dispatch(kind_k, b0_k, hb1_k, b1_k, t, cf);  //  :86
        sc_s[5] = t;
        sc_s[3] = (double)st;
        if (st == ST_SUCCESS) {  //                                          :88-90
            sc_s[0] = cf.rho / omega;
            const double mu = cf.sigma / (1.0 - cf.sigma);  //               :107
            double oldt = omega / mu;  //                                    :108
            for (int j = 0; j < n; ++j) {  //                                :110-121
                const double temp = oldt + gg_s[j];
                if (j < n - 1) w_s[j] = z_s[j] / temp;  // beta2
                gg_s[j] = oldt / temp;
                oldt = temp;
            }
            sc_s[4] = kap * cf.delta;  //                                    :122
        }
        emit(st, t);
    }
    __syncthreads();
    const bool ok = active && sc[3] == (double)ST_SUCCESS;
    if (ok) {
        if (i == 0) {  // back solve on the scratch triangle, g_t = z        :93-98
            for (int r = n - 1; r >= 1; --r) {
                double acc = z[r - 1];
                const double* scol = q + (r - 1);
#pragma unroll 8
                for (int j = r; j < n; ++j) acc -= scol[(size_t)j * pitch] * z[j];
                z[r - 1] = acc;
            }
        }
        // column i of the factor and the diagonal element                   :110-121
        double* ucol = q + i;
#pragma unroll 4
        for (int j = 0; j < i; ++j) ucol[(size_t)j * pitch] = ucol[(size_t)j * pitch] + w[j] * srow[j];
        srow[i] = srow[i] * gg[i];
    }
    __syncthreads();
    if (ok) xci = xci - sc[0] * z[i];  //                                    :101-104
}

// The space of a loop kernel, chosen at compile time: STABLE = false is Ell (batch_cut_apply, batch_kernels.hpp), true
// is EllStable.  Both lay an instance out as the buffer, the gradient's n doubles, their other vectors and 8 scalars.
template <bool STABLE>
__host__ __device__ inline size_t batch_space_lds_doubles(int n) {
    return STABLE ? batch_stable_apply_lds_doubles(n) : batch_lds_doubles(n);
}
template <bool STABLE>
__host__ __device__ inline size_t batch_space_scalars_at(int n) {  // offset of the 8 scalars inside an instance's block
    return (size_t)n * batch_pitch(n) + (STABLE ? 3 : 2) * (size_t)n;
}

// q: this thread's instance block, q_s: the scalar lane's.  The gradient is at q + n * pitch.
template <bool STABLE, class Emit>
__device__ __forceinline__ void batch_space_cut_apply(const BatchParams& P, const EllCalcDev& calc, const bool active,
                                                      const int i, double* q, double& xci, const bool scalar_lane,
                                                      double* q_s, const int kind_k, const double b0_k, const int hb1_k,
                                                      const double b1_k, Emit emit) {
    const int n = P.n;
    double* g = q + (size_t)n * P.pitch;
    double* g_s = q_s + (size_t)n * P.pitch;
    if constexpr (STABLE) {
        batch_stable_cut_apply(P, calc, active, i, q, g, g + n, g + 2 * n, g + 3 * n, xci, scalar_lane, g_s, g_s + n,
                               g_s + 2 * n, g_s + 3 * n, kind_k, b0_k, hb1_k, b1_k, emit);
    } else {
        batch_cut_apply(P, calc, active, i, q, g, g + n, g + 2 * n, xci, scalar_lane, g_s, g_s + n, g_s + 2 * n, kind_k,
                        b0_k, hb1_k, b1_k, emit);
    }
}

}  // namespace ellhip
