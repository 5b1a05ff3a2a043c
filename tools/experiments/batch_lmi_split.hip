// batch_lmi_split.hip -- how one round of k_batch_loop over the LMI oracle splits between the oracle and the ellipsoid update.
//
// A copy of the loop kernel (ellalgo-rs_amd/csrc/batch_loop_kernels.hpp, optim only) with the constant 100 MHz wall clock read by
// thread 0 of every workgroup before the oracle, between the oracle and the update, and after the update; each of
// these points follows a barrier, so thread 0's clock is the workgroup's.  The oracle and the update themselves are the
// product's device functions.  Problems: random strictly feasible pencils of the requested shape (F_jk symmetric normal,
// B_j = M M' + m I, c normal), Ell::new_with_scalar(10, 0); with `stable` EllStable::new_with_scalar(10, 0) and the
// row-parallel update of batch_stable_apply.hpp, launched as the _stable entry points launch it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o batch_lmi_split batch_lmi_split.hip
//   ./batch_lmi_split n m J B tol [stable]   -> one JSON line: ns per round in the oracle and in the update
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/batch_lmi_kernels.hpp"

using namespace ellhip;

#define CHK(x)                                                                          \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                     \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

template <int T, bool STABLE>
__global__ __launch_bounds__(T) void k_loop_clocked(BatchParams P, BatchLmiParams L, BatchLoopRun R, double* Q, double* xc,
                                                    double* kappa, const double* pencil, const double* matb,
                                                    const double* cvec, double* state /* [B][4]: gamma idx niter stopped */,
                                                    long long* clocks /* [grid][3]: oracle, update, rounds */,
                                                    EllCalcDev calc) {
    extern __shared__ double sm[];
    const int n = P.n, pitch = P.pitch, tid = threadIdx.x;
    const int e = tid / n, i = tid - e * n;
    const long long b = (long long)blockIdx.x * P.epw + e;
    const bool active = e < P.epw && b < P.B;
    if (!__syncthreads_or(active && state[b * 4 + 3] == 0.0)) return;
    const size_t per = batch_space_lds_doubles<STABLE>(n), lper = batch_lmi_lds_doubles(n, L.mmax);
    const int el = e < P.epw ? e : 0;
    double* q = sm + (size_t)el * per;
    double* g = q + (size_t)n * pitch;
    double* sc = q + batch_space_scalars_at<STABLE>(n);
    double* lx = sm + (size_t)P.epw * per + (size_t)el * lper;
    double* cl = lx + n;
    double* fa = cl + n;
    double* wit = fa + (size_t)L.mmax * L.pm;
    double* osc = wit + L.mmax;
    const long long b_first = (long long)blockIdx.x * P.epw;
    const int nb = (int)((P.B - b_first < P.epw) ? P.B - b_first : P.epw);
    double* Qwg = Q + b_first * (long long)n * n;
    batch_copy<T, true>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
    double xci = 0.0;
    if (active) {
        xci = xc[b * n + i];
        cl[i] = cvec[b * n + i];
    }
    if (active && i == 0) {
        sc[3] = 0.0;
        sc[4] = kappa[b];
        sc[5] = 0.0;
        osc[LO_GAMMA] = state[b * 4 + 0];
        osc[LO_IDX] = state[b * 4 + 1];
        osc[BL_NITER] = state[b * 4 + 2];
        osc[BL_STOPPED] = state[b * 4 + 3];
    }
    __syncthreads();
    const bool lane_ok = tid < P.epw && b_first + tid < P.B;
    const int es = tid < P.epw ? tid : 0;
    double* q_s = sm + (size_t)es * per;
    const double* osc_s = sm + (size_t)P.epw * per + (size_t)es * lper + 2 * (size_t)n + (size_t)L.mmax * L.pm + L.mmax;
    const double* F = pencil + (active ? b : 0) * (long long)L.fstride;
    const double* Bm = matb + (active ? b : 0) * (long long)L.bstride;
    const double shrunk_station = (double)(L.J + 1);
    long long t_oracle = 0, t_update = 0, rounds = 0;
    for (int it = 0; it < R.iters; ++it) {
        const bool live = active && osc[BL_STOPPED] == 0.0;
        if (!__syncthreads_or(live)) break;
        if (live) lx[i] = xci;
        __syncthreads();
        const long long t0 = wall_clock64();
        batch_lmi_oracle(L, live, i, n, F, Bm, nullptr, lx, cl, fa, wit, osc, g);
        const long long t1 = wall_clock64();
        const bool lane = lane_ok && osc_s[BL_STOPPED] == 0.0;
        const int kind = (lane && osc_s[LO_STATION] == shrunk_station) ? CUT_CENTRAL : CUT_BIAS;
        batch_space_cut_apply<STABLE>(P, calc, live, i, q, xci, lane, q_s, kind, lane ? osc_s[LO_BETA] : 0.0, 0, 0.0,
                                      [](int, double) {});
        const long long t2 = wall_clock64();
        t_oracle += t1 - t0;
        t_update += t2 - t1;
        rounds += 1;
        if (live && i == 0) {
            if (sc[3] != 0.0 || sc[5] < R.tol) osc[BL_STOPPED] = 1.0;
            else osc[BL_NITER] += 1.0;
        }
        __syncthreads();
    }
    if (active) xc[b * n + i] = xci;
    if (active && i == 0) {
        kappa[b] = sc[4];
        state[b * 4 + 0] = osc[LO_GAMMA];
        state[b * 4 + 1] = osc[LO_IDX];
        state[b * 4 + 2] = osc[BL_NITER];
        state[b * 4 + 3] = osc[BL_STOPPED];
    }
    if (tid == 0) {
        clocks[blockIdx.x * 3 + 0] += t_oracle;
        clocks[blockIdx.x * 3 + 1] += t_update;
        clocks[blockIdx.x * 3 + 2] += rounds;
    }
    batch_copy<T, false>(sm, Qwg, nb * n * n, n, pitch, (int)per, tid);
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 16, m = argc > 2 ? atoi(argv[2]) : 12, J = argc > 3 ? atoi(argv[3]) : 3;
    const long long B = argc > 4 ? atoll(argv[4]) : 1024;
    const double tol = argc > 5 ? atof(argv[5]) : 1e-8;
    const bool stable = argc > 6 && !strcmp(argv[6], "stable");
    if (n < 1 || n > BATCH_NMAX || m < 1 || m > BATCH_LMI_MMAX || J < 1 || J > BATCH_LMI_JMAX || B < 1) return 2;
    BatchLmiParams L{};
    L.J = J;
    for (int j = 0; j < J; ++j) {
        L.m[j] = m;
        L.foff[j] = j * m * m * n;
        L.boff[j] = j * m * m;
    }
    L.fstride = J * m * m * n;
    L.bstride = J * m * m;
    L.mmax = m;
    L.pm = m | 1;
    L.has_b = L.has_c = 1;
    L.nstation = J + 1;
    // the batch engine's shape for n (batch_shape in batch_capi.inc.hpp)
    const int T = n <= 64 ? 256 : 128;
    int epw = std::min(64, T / n);
    const size_t space_doubles = stable ? batch_stable_apply_lds_doubles(n) : batch_lds_doubles(n);
    const size_t per_bytes = space_doubles * sizeof(double);
    while (epw > 1 && (size_t)epw * per_bytes > 64 * 1024) epw -= 1;
    const size_t lds = (size_t)epw * (space_doubles + batch_lmi_lds_doubles(n, m)) * sizeof(double);
    if (lds > 159 * 1024) return 3;
    std::mt19937_64 rng(7);
    std::normal_distribution<double> nd;
    std::vector<double> pk((size_t)B * L.fstride), pb((size_t)B * L.bstride), c((size_t)B * n), Q((size_t)B * n * n, 0.0);
    std::vector<double> mm((size_t)m * m);
    for (long long b = 0; b < B; ++b) {
        for (int j = 0; j < J; ++j) {
            double* f = pk.data() + b * L.fstride + L.foff[j];
            for (int k = 0; k < n; ++k)
                for (int a = 0; a < m; ++a)
                    for (int d = 0; d <= a; ++d) f[(a * m + d) * n + k] = f[(d * m + a) * n + k] = nd(rng);
            for (double& v : mm) v = nd(rng);
            double* bm = pb.data() + b * L.bstride + L.boff[j];
            for (int a = 0; a < m; ++a)
                for (int d = 0; d < m; ++d) {
                    double s = a == d ? (double)m : 0.0;
                    for (int k = 0; k < m; ++k) s += mm[a * m + k] * mm[d * m + k];
                    bm[a * m + d] = s;
                }
        }
        for (int k = 0; k < n; ++k) c[b * n + k] = nd(rng);
        for (int k = 0; k < n; ++k) Q[(b * n + k) * n + k] = 1.0;
    }
    const unsigned grid = (unsigned)((B + epw - 1) / epw);
    std::vector<double> state((size_t)B * 4, 0.0), kap((size_t)B, 10.0);
    for (long long b = 0; b < B; ++b) {
        state[b * 4 + 0] = __builtin_inf();
        state[b * 4 + 1] = -1.0;
    }
    double *d_pk, *d_pb, *d_c, *d_Q, *d_xc, *d_kap, *d_state;
    long long* d_clk;
    CHK(hipMalloc(&d_pk, pk.size() * 8));
    CHK(hipMalloc(&d_pb, pb.size() * 8));
    CHK(hipMalloc(&d_c, c.size() * 8));
    CHK(hipMalloc(&d_Q, Q.size() * 8));
    CHK(hipMalloc(&d_xc, (size_t)B * n * 8));
    CHK(hipMalloc(&d_kap, (size_t)B * 8));
    CHK(hipMalloc(&d_state, state.size() * 8));
    CHK(hipMalloc(&d_clk, (size_t)grid * 3 * 8));
    CHK(hipMemcpy(d_pk, pk.data(), pk.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_pb, pb.data(), pb.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_c, c.data(), c.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_Q, Q.data(), Q.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_kap, kap.data(), kap.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_state, state.data(), state.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemset(d_xc, 0, (size_t)B * n * 8));
    CHK(hipMemset(d_clk, 0, (size_t)grid * 3 * 8));
    CHK(hipDeviceSynchronize());
    BatchParams P{B, n, batch_pitch(n), epw, 0, 0};
    BatchLoopRun R{256, 0, 2000, tol};
    const EllCalcDev calc = EllCalcDev::make(n, 1);
    auto kernel = T == 256 ? (stable ? &k_loop_clocked<256, true> : &k_loop_clocked<256, false>)
                           : (stable ? &k_loop_clocked<128, true> : &k_loop_clocked<128, false>);
    CHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int launch = 0; launch < 8; ++launch) {  // 8 x 256 >= max_iters; a workgroup whose instances have stopped leaves at once
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), lds, 0, P, L, R, d_Q, d_xc, d_kap, d_pk, d_pb, d_c, d_state, d_clk, calc);
        CHK(hipGetLastError());
        CHK(hipDeviceSynchronize());
    }
    std::vector<long long> clk((size_t)grid * 3);
    CHK(hipMemcpy(clk.data(), d_clk, clk.size() * 8, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(state.data(), d_state, state.size() * 8, hipMemcpyDeviceToHost));
    long long t_or = 0, t_up = 0, rounds = 0;
    for (unsigned w = 0; w < grid; ++w) {
        t_or += clk[w * 3];
        t_up += clk[w * 3 + 1];
        rounds += clk[w * 3 + 2];
    }
    double nit_min = 1e300, nit_max = 0;
    long long stopped = 0;
    for (long long b = 0; b < B; ++b) {
        nit_min = std::min(nit_min, state[b * 4 + 2]);
        nit_max = std::max(nit_max, state[b * 4 + 2]);
        stopped += state[b * 4 + 3] != 0.0;
    }
    const double tick_ns = 10.0;  // wall_clock64: 100 MHz
    printf("{\"probe\": \"batch_lmi_split\", \"space\": \"%s\", \"n\": %d, \"m\": %d, \"J\": %d, \"B\": %lld, \"epw\": %d, \"threads\": %d, \"lds_bytes\": %zu, "
           "\"workgroup_rounds\": %lld, \"oracle_ns_per_round\": %.1f, \"update_ns_per_round\": %.1f, \"oracle_share\": %.3f, "
           "\"niter_min\": %.0f, \"niter_max\": %.0f, \"stopped\": %lld}\n",
           stable ? "stable" : "ell", n, m, J, B, epw, T, lds, rounds, tick_ns * t_or / rounds, tick_ns * t_up / rounds, (double)t_or / (double)(t_or + t_up),
           nit_min, nit_max, stopped);
    return 0;
}
