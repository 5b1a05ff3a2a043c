// batch_lmi_capi.inc.hpp -- C ABI of the batched device-resident LMI cutting-plane loop (include/ellhip_batch_lmi.h).
// Included at the end of ellhip_capi.hip, after batch_loop_capi.inc.hpp (the loop state, the launch shapes and the driver).
//
// Reference: tests/lmi_tests.rs:142-171 (oracle), src/oracles/lmi_oracle.rs, lmi0_oracle.rs, ldlt_mgr.rs,
// src/cutting_plane.rs:205-227, 286-313 (loops).
#include "../../include/ellhip_batch_lmi.h"

#include "batch_lmi_kernels.hpp"

struct ellhip_batch_lmi {
    BatchLoopBuffers loop;        // device, B, n, stream, the loop state (d_gamma: also assess; d_ints: also its stations)
    long long B = 0;
    int n = 0;
    BatchLmiParams L{};
    double* d_pencil = nullptr;   // [B][block][a][b][k]
    double* d_matb = nullptr;     // [B][block][a][b], or null
    double* d_c = nullptr;        // [B][n], or null
    int* d_idx = nullptr;         // [B]
    double* d_tri = nullptr;      // [B][block][k][t], the lower triangles element-fastest, or null (batch_lmi_kernels.hpp)
    int shared_f = 0;             // d_pencil (and d_tri) is one pencil, [block][a][b][k], that every problem reads
    double* d_x = nullptr;        // assess: [B][n]
    double* d_grad = nullptr;     // assess: [B][n]
    double* d_beta = nullptr;     // assess: [B]
};

namespace {

BatchLmiOracle::Args batch_lmi_args(const ellhip_batch_lmi* o) {
    BatchLmiOracle::Args A;
    A.L = o->L;
    if (o->shared_f) A.L.fstride = A.L.tstride = 0;  // BatchLmiOracle::load: every instance reads the one pencil
    A.pencil = o->d_pencil;
    A.tri = o->d_tri;
    A.matb = o->d_matb;
    A.cvec = o->d_c;
    A.idx = o->d_idx;
    return A;
}

// The loops of all four headers (ellhip_batch_lmi.h, ellhip_batch_stable_loops.h, ellhip_batch_lmi_streamed.h) on `engine`.
// Which of optim and feas a handle serves is refused in the words of the engine's Ell entry points.
int batch_lmi_run(ellhip_batch* s, ellhip_batch_lmi* o, int feas, double* gamma_inout, int64_t max_iters, double tol,
                  double* x_out, int32_t* has_out, int64_t* niter_out, int32_t* status_out, BatchLoopEngine engine) {
    if (!s || !o || !has_out || !niter_out || !status_out || (!feas && !gamma_inout))
        return fail(ELLHIP_E_INVALID, "NULL argument");
    const std::string what = batch_loop_what("LMI", {engine.streamed, false});
    if (!feas && !o->L.has_c) return fail(ELLHIP_E_INVALID, (what + ": optim needs a handle made with c").c_str());
    if (feas && o->L.has_c) return fail(ELLHIP_E_INVALID, (what + ": feas needs a handle made without c").c_str());
    return batch_loop_run<BatchLmiOracle>(s, o->loop, batch_lmi_args(o), {"LMI", "(n, m)", ""}, engine, feas, gamma_inout,
                                          max_iters, tol, x_out, has_out, niter_out, status_out);
}

// The constructor of both headers.  nmax: 128 for ellhip_batch_lmi_create, 1024 for ellhip_batch_lmi_create_streamed
// (batch_lmi_streamed_capi.inc.hpp); shared_f: one pencil [n][m_j][m_j] per block for every problem; tri: keep the
// element-fastest copy of the lower triangles that F(x) then reads (half the pencil's size again).
int batch_lmi_create(ellhip_batch_lmi** out, int64_t B, int64_t n, int64_t J, const int64_t* m, const double* mat_f,
                     int32_t shared_f, const double* mat_b, const double* c, int device, int nmax, bool tri) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (B < 1 || n < 1 || n > nmax)
        return fail(ELLHIP_E_INVALID, ("batched LMI: need B >= 1 and 1 <= n <= " + std::to_string(nmax)).c_str());
    if (J < 1 || J > BATCH_LMI_JMAX) return fail(ELLHIP_E_INVALID, "batched LMI: need 1 <= J <= 8 blocks");
    if (!m || !mat_f) return fail(ELLHIP_E_INVALID, "NULL argument");
    BatchLmiParams L{};
    L.J = (int)J;
    long long sum_mm = 0, sum_tri = 0;
    for (int j = 0; j < (int)J; ++j) {
        if (m[j] < 1 || m[j] > BATCH_LMI_MMAX) return fail(ELLHIP_E_INVALID, "batched LMI: need 1 <= m_j <= 64");
        L.m[j] = (int)m[j];
        L.foff[j] = (int)(sum_mm * n);  // at most 7 * 64^2 * 1024 < 2^31
        L.boff[j] = (int)sum_mm;
        L.toff[j] = (int)(sum_tri * n);
        sum_mm += m[j] * m[j];
        sum_tri += m[j] * (m[j] + 1) / 2;
        L.mmax = std::max(L.mmax, L.m[j]);
    }
    L.fstride = (int)(sum_mm * n);
    L.bstride = (int)sum_mm;
    L.tstride = (int)(sum_tri * n);
    L.pm = L.mmax | 1;
    L.has_b = mat_b ? 1 : 0;
    L.has_c = c ? 1 : 0;
    L.nstation = L.J + L.has_c;
    const size_t sB = (size_t)B, sn = (size_t)n;
    const size_t npencil = shared_f ? 1 : sB;  // pencils kept on the device
    if ((double)npencil * ((double)L.fstride + (tri ? (double)L.tstride : 0.0)) * 8.0 > 100e9)
        return fail(ELLHIP_E_NOMEM, "batched LMI: the pencils are too large");
    const int ndev = ellhip_device_count();
    if (ndev <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the batched LMI loop has no CPU path");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    if (device >= ndev) return fail(ELLHIP_E_INVALID, "device index out of range");
    ellhip_batch_lmi* o = new (std::nothrow) ellhip_batch_lmi();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->B = B;
    o->n = (int)n;
    o->L = L;
    o->shared_f = shared_f ? 1 : 0;
    DeviceGuard guard(device);
    auto bail = [&](int code) {
        ellhip_batch_lmi_destroy(o);
        return code;
    };
    // B matrices: the caller's [block][B][a][b] becomes [B][block][a][b]
    std::vector<double> pb(mat_b ? sB * (size_t)L.bstride : 0);
    if (mat_b) {
        size_t src_b = 0;
        for (int j = 0; j < L.J; ++j) {
            const size_t mm = (size_t)L.m[j] * L.m[j];
            for (size_t b = 0; b < sB; ++b)
                memcpy(pb.data() + b * (size_t)L.bstride + L.boff[j], mat_b + src_b + b * mm, mm * sizeof(double));
            src_b += sB * mm;
        }
    }
    hipError_t e = batch_loop_alloc(o->loop, device, B, (int)n);
    if (e == hipSuccess) e = o->loop.mem.device(o->d_pencil, npencil * (size_t)L.fstride * sizeof(double));
    if (e == hipSuccess && tri) e = o->loop.mem.device(o->d_tri, npencil * (size_t)L.tstride * sizeof(double));
    if (e == hipSuccess && mat_b) e = o->loop.mem.device(o->d_matb, pb.size() * sizeof(double));
    if (e == hipSuccess && c) e = o->loop.mem.device(o->d_c, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_idx, sB * sizeof(int));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_x, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_grad, sB * sn * sizeof(double));
    if (e == hipSuccess) e = o->loop.mem.device(o->d_beta, sB * sizeof(double));
    if (e != hipSuccess) return bail(fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "batched LMI allocation", e));
    // pencils, one at a time (the host never holds more than one repacked): the caller's [block][B or 1][k][a][b] becomes
    // [B or 1][block][a][b][k], and its lower triangles [B or 1][block][k][t]
    std::vector<double> pk((size_t)L.fstride), tk(tri ? (size_t)L.tstride : 0);
    for (size_t b = 0; b < npencil && e == hipSuccess; ++b) {
        size_t src_f = 0;
        for (int j = 0; j < L.J; ++j) {
            const size_t mm = (size_t)L.m[j] * L.m[j];
            double* dst = pk.data() + L.foff[j];
            const double* src = mat_f + src_f + b * sn * mm;
            for (size_t k = 0; k < sn; ++k)
                for (size_t el = 0; el < mm; ++el) dst[el * sn + k] = src[k * mm + el];
            if (tri) {
                const size_t mj = (size_t)L.m[j], nt = mj * (mj + 1) / 2;
                double* dt = tk.data() + L.toff[j];
                for (size_t k = 0; k < sn; ++k)
                    for (size_t a = 0, t = 0; a < mj; ++a)
                        for (size_t bb = 0; bb <= a; ++bb, ++t) dt[k * nt + t] = src[k * mm + a * mj + bb];
            }
            src_f += npencil * sn * mm;
        }
        e = hipMemcpy(o->d_pencil + b * (size_t)L.fstride, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess && tri)
            e = hipMemcpy(o->d_tri + b * (size_t)L.tstride, tk.data(), tk.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && mat_b) e = hipMemcpy(o->d_matb, pb.data(), pb.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && c) e = hipMemcpy(o->d_c, c, sB * sn * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = fill_now(o->d_idx, 0xff, sB * sizeof(int), o->loop.stream);  // idx = -1
    if (e != hipSuccess) return bail(fail(ELLHIP_E_HIP, "batched LMI upload", e));
    *out = o;
    return 0;
}

}  // namespace

extern "C" {

int ellhip_batch_lmi_create(ellhip_batch_lmi** out, int64_t B, int64_t n, int64_t J, const int64_t* m, const double* mat_f,
                            const double* mat_b, const double* c, int device) {
    return batch_lmi_create(out, B, n, J, m, mat_f, 0, mat_b, c, device, BATCH_NMAX, false);
}

void ellhip_batch_lmi_destroy(ellhip_batch_lmi* o) {
    if (!o) return;
    DeviceGuard guard(o->loop.device);
    batch_loop_free(o->loop);
    delete o;
}

int ellhip_batch_lmi_assess_optim(ellhip_batch_lmi* o, const double* x, double* gamma_inout, double* grad_out, double* beta_out,
                                  int32_t* station_out) {
    if (!o || !x || !gamma_inout || !grad_out || !beta_out || !station_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    const size_t B = (size_t)o->B, n = (size_t)o->n;
    const size_t per = batch_lmi_lds_doubles(o->n, o->L.mmax) + n;
    // past the LDS engine's n (batch_row_shape has no instance per workgroup to offer): one instance per workgroup, n threads
    // rounded up to whole waves, as the streamed engine shapes its own
    const bool wide = o->n > BATCH_NMAX;
    const BatchRowShape sh = batch_row_shape(o->n, per);
    const int T = wide ? (o->n + 63) / 64 * 64 : sh.T, epw = wide ? 1 : sh.epw;
    // at most (2*128 + 64*65 + 64 + 17 + 128) * 8 < 64 KiB for one instance, or 57.1 KiB at n = 1024, M = 64
    const size_t lds = (size_t)epw * per * sizeof(double);
    const unsigned grid = (unsigned)((o->B + epw - 1) / epw);
    int* d_station = o->loop.d_ints;
    HIPCHK(hipMemcpy(o->d_x, x, B * n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->d_grad, grad_out, B * n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(o->loop.d_gamma, gamma_inout, B * sizeof(double), hipMemcpyHostToDevice));
#define BATCH_LMI_ASSESS(TT)                                                                                           \
    hipLaunchKernelGGL(k_batch_lmi_assess<TT>, dim3(grid), dim3(T), lds, o->loop.stream, o->B, o->n, epw,             \
                       batch_lmi_args(o), (const double*)o->d_x, o->loop.d_gamma, o->d_grad, o->d_beta, d_station)
    if (wide) BATCH_LMI_ASSESS(1024);  // (the template argument bounds the block; the block is T threads)
    else if (T == 128) BATCH_LMI_ASSESS(128);
    else BATCH_LMI_ASSESS(256);
#undef BATCH_LMI_ASSESS
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(grad_out, o->d_grad, B * n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(beta_out, o->d_beta, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(gamma_inout, o->loop.d_gamma, B * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(station_out, d_station, B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_lmi_get_idx(ellhip_batch_lmi* o, int32_t* idx_out) {
    if (!o || !idx_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    HIPCHK(hipMemcpy(idx_out, o->d_idx, (size_t)o->B * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int ellhip_batch_lmi_set_idx(ellhip_batch_lmi* o, const int32_t* idx) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    DeviceGuard guard(o->loop.device);
    HIPCHK(hipStreamSynchronize(o->loop.stream));
    if (!idx) {
        HIPCHK(fill_now(o->d_idx, 0xff, (size_t)o->B * sizeof(int), o->loop.stream));
        return 0;
    }
    for (long long b = 0; b < o->B; ++b)
        if (idx[b] < -1 || idx[b] > o->L.J) return fail(ELLHIP_E_INVALID, "batched LMI: idx must be in -1..J");
    HIPCHK(hipMemcpy(o->d_idx, idx, (size_t)o->B * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

int ellhip_batch_lmi_optim(ellhip_batch* spaces, ellhip_batch_lmi* o, double* gamma_inout, int64_t max_iters, double tol,
                           double* x_best_out, int32_t* has_best_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 0, gamma_inout, max_iters, tol, x_best_out, has_best_out, niter_out, status_out,
                         BATCH_ENGINE_LDS);
}

int ellhip_batch_lmi_feas(ellhip_batch* spaces, ellhip_batch_lmi* o, int64_t max_iters, double tol, double* x_out,
                          int32_t* feasible_out, int64_t* niter_out, int32_t* status_out) {
    return batch_lmi_run(spaces, o, 1, nullptr, max_iters, tol, x_out, feasible_out, niter_out, status_out, BATCH_ENGINE_LDS);
}

int ellhip_batch_lmi_set_chunk(ellhip_batch_lmi* o, int64_t iters) {
    return batch_loop_set_chunk(o ? &o->loop : nullptr, iters, "batched LMI");
}

}  // extern "C"
