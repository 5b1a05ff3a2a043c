// lmi_loop_capi.inc.hpp -- C ABI of the round-robin problem handle over large LMI blocks and of the device-resident
// cutting-plane loops built on it (include/ellhip_lmi_loop.h).  Included at the end of ellhip_capi.hip, after
// lmi_capi.inc.hpp (struct ellhip_lmi, lmi_issue) and svm_capi.inc.hpp (the Stage this one is written beside).
//
// Reference: tests/lmi_tests.rs:142-171 (the oracle), src/cutting_plane.rs:205-227,286-313 (the loops).
#include "../../include/ellhip_lmi_loop.h"

#include "lmi_loop_kernels.hpp"
#include "device_loop.inc.hpp"

static_assert(LMI_LOOP_JMAX == ELLHIP_LMI_LOOP_JMAX, "header and kernels disagree on the block limit");

struct ellhip_lmi_loop {
    int device = 0;
    long long n = 0;
    int J = 0;
    bool has_c = false;
    ellhip_lmi* blocks[LMI_LOOP_JMAX] = {};  // borrowed: the caller's handles
    Allocs mem;
    double* d_c = nullptr;      // n (optimisation form)
    double* d_x = nullptr;      // n: the point of a single call
    double* d_g = nullptr;      // n: the iteration's gradient
    double* d_xbest = nullptr;  // n
    LmiLoopState* d_ls = nullptr;
    CutParams* d_cp = nullptr;
    int* d_zero = nullptr;
    hipStream_t stream = nullptr;
    LmiLoopState* h_ls = nullptr;
    CutParams* h_cp = nullptr;
    double* h_vec = nullptr;    // n
};

namespace {

int ll_stations(const ellhip_lmi_loop* o) { return o->has_c ? o->J + 1 : o->J; }

// One oracle call at x_dev on `st`: the window of station slots that covers every cyclic walk, then the closing kernel.
int ll_window(ellhip_lmi_loop* o, hipStream_t st, const double* x_dev, const int* halted, DevState* drv) {
    const int S = ll_stations(o), slots = 2 * S - 1;
    for (int p = 0; p < slots; ++p) {
        const int station = p < S ? p : p - S;
        if (station < o->J) {
            ellhip_lmi* b = o->blocks[station];
            hipLaunchKernelGGL(k_ll_gate, dim3(1), dim3(64), 0, st, o->d_ls, halted, station, S, p == 0 ? 1 : 0, b->d_st);
            const int rc = lmi_issue(b, st, x_dev);
            if (rc) {
                // a launch failed between the gate and the station kernel: do not leave the borrowed block skipping
                (void)hipMemsetAsync(reinterpret_cast<char*>(b->d_st) + offsetof(LmiState, skip), 0, sizeof(int), st);
                return rc;
            }
            hipLaunchKernelGGL(k_ll_station, dim3(1), dim3(64), 0, st, o->d_ls, b->d_st, (const double*)b->d_g, o->n,
                               o->d_g, o->d_cp, station);
        } else {
            hipLaunchKernelGGL(k_ll_objective, dim3(1), dim3(64), 0, st, o->d_ls, halted, (const double*)o->d_c, x_dev,
                               o->n, o->d_g, o->d_cp, o->J);
        }
    }
    hipLaunchKernelGGL(k_ll_close, dim3(1), dim3(64), 0, st, o->d_ls, halted, (const double*)o->d_c, x_dev, o->n, o->d_g,
                       o->d_cp, o->d_xbest, drv, o->has_c ? 1 : 0, o->J);
    HIPCHK(hipGetLastError());
    return 0;
}

int ll_drain_blocks(ellhip_lmi_loop* o) {
    for (int j = 0; j < o->J; ++j) HIPCHK(hipStreamSynchronize(o->blocks[j]->stream));
    return 0;
}

// h_ls holds the loop state read back on `st`: every block that ran gets its host copy of LmiState refreshed, so that
// ellhip_lmi_pos reports the block's last executed call as after ellhip_lmi_assess_feas
int ll_refresh_blocks(ellhip_lmi_loop* o, hipStream_t st) {
    bool any = false;
    for (int j = 0; j < o->J; ++j)
        if (o->h_ls->ran[j]) {
            ellhip_lmi* b = o->blocks[j];
            HIPCHK(hipMemcpyAsync(b->h_st, b->d_st, sizeof(LmiState), hipMemcpyDeviceToHost, st));
            b->factored = true;
            any = true;
        }
    if (any) HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// walk state for a new API call: `gamma` in (optimisation form), nothing ran, no best point; the cursor stays
int ll_reset(ellhip_lmi_loop* o, hipStream_t st, const double* gamma) {
    HIPCHK(hipMemcpyAsync(o->h_ls, o->d_ls, sizeof(LmiLoopState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    o->h_ls->steps = 0;
    o->h_ls->done = 0;
    o->h_ls->active = 0;
    o->h_ls->has_best = 0;
    for (int j = 0; j < LMI_LOOP_JMAX; ++j) o->h_ls->ran[j] = 0;
    if (gamma) o->h_ls->gamma = *gamma;
    HIPCHK(hipMemcpyAsync(o->d_ls, o->h_ls, sizeof(LmiLoopState), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int ll_assess_host(ellhip_lmi_loop* o, const double* x, double* gamma_inout, double* g_out, double* beta_out,
                   int* station_out) {
    DeviceGuard guard(o->device);
    int rc = ll_drain_blocks(o);
    if (rc) return rc;
    hipStream_t st = o->stream;
    const size_t vbytes = (size_t)o->n * sizeof(double);
    memcpy(o->h_vec, x, vbytes);
    HIPCHK(hipMemcpyAsync(o->d_x, o->h_vec, vbytes, hipMemcpyHostToDevice, st));
    rc = ll_reset(o, st, gamma_inout);
    if (rc) return rc;
    rc = ll_window(o, st, o->d_x, o->d_zero, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(o->h_ls, o->d_ls, sizeof(LmiLoopState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(o->h_cp, o->d_cp, sizeof(CutParams), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(o->h_vec, o->d_g, vbytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    rc = ll_refresh_blocks(o, st);
    if (rc) return rc;
    if (station_out) *station_out = o->h_ls->station;
    if (gamma_inout) *gamma_inout = o->h_ls->gamma;
    if (o->h_ls->station < 0) return 0;  // feasibility form: None
    memcpy(g_out, o->h_vec, vbytes);
    *beta_out = o->h_cp->b0;
    return 1;
}

// The oracle's side of the device-resident loop (device_loop.inc.hpp): has_c = cutting_plane_optim
// (src/cutting_plane.rs:286-313), otherwise cutting_plane_feas (:205-227).
struct LmiLoopStage {
    ellhip_lmi_loop* o;
    double* gamma_inout;
    double* x_best_out;
    int* has_best_out;
    int64_t* niter_out;

    hipStream_t stream() { return o->stream; }
    const double* grad() { return o->d_g; }
    const CutParams* cut() { return o->d_cp; }
    int begin(hipStream_t st) {
        const int rc = ll_drain_blocks(o);  // the whole loop runs on the space's stream
        if (rc) return rc;
        return ll_reset(o, st, gamma_inout);
    }
    int issue(hipStream_t st, ellhip_space* s, const int* halted) { return ll_window(o, st, s->d_xc, halted, s->d_st); }
    int finish(hipStream_t st, long long niter) {
        HIPCHK(hipMemcpyAsync(o->h_ls, o->d_ls, sizeof(LmiLoopState), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const int rc = ll_refresh_blocks(o, st);
        if (rc) return rc;
        *niter_out = niter;
        *has_best_out = o->h_ls->has_best;
        if (o->h_ls->has_best && x_best_out) {
            const size_t vbytes = (size_t)o->n * sizeof(double);
            HIPCHK(hipMemcpyAsync(o->h_vec, o->d_xbest, vbytes, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            memcpy(x_best_out, o->h_vec, vbytes);
        }
        if (gamma_inout) *gamma_inout = o->h_ls->gamma;
        return 0;
    }
};

}  // namespace

extern "C" {

void ellhip_lmi_loop_destroy(ellhip_lmi_loop* o) {
    if (!o) return;
    DeviceGuard guard(o->device);
    if (o->stream) (void)hipStreamSynchronize(o->stream);
    o->mem.release_all();  // (its own buffers; the blocks are borrowed)
    if (o->stream) (void)hipStreamDestroy(o->stream);
    delete o;
}

int ellhip_lmi_loop_create(ellhip_lmi_loop** out, ellhip_lmi* const* blocks, int64_t J, const double* c) {
    if (!out) return fail(ELLHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (J < 1 || J > ELLHIP_LMI_LOOP_JMAX) return fail(ELLHIP_E_INVALID, "lmi loop: need 1 <= J <= 8 blocks");
    if (!blocks) return fail(ELLHIP_E_INVALID, "lmi loop: blocks is NULL");
    if (ellhip_device_count() <= 0) return fail(ELLHIP_E_NODEVICE, "no HIP device: the LMI loop has no CPU path");
    for (int64_t j = 0; j < J; ++j) {
        if (!blocks[j]) return fail(ELLHIP_E_INVALID, "lmi loop: a block is NULL");
        if (blocks[j]->n < 1) return fail(ELLHIP_E_INVALID, "lmi loop: a block has no variables (n == 0)");
        if (blocks[j]->n != blocks[0]->n) return fail(ELLHIP_E_INVALID, "lmi loop: blocks differ in n");
        if (blocks[j]->device != blocks[0]->device) return fail(ELLHIP_E_INVALID, "lmi loop: blocks live on different devices");
    }
    ellhip_lmi_loop* o = new (std::nothrow) ellhip_lmi_loop();
    if (!o) return fail(ELLHIP_E_NOMEM, "host allocation failed");
    o->device = blocks[0]->device;
    o->n = blocks[0]->n;
    o->J = (int)J;
    o->has_c = c != nullptr;
    for (int64_t j = 0; j < J; ++j) o->blocks[j] = blocks[j];
    DeviceGuard guard(o->device);
    const size_t vbytes = (size_t)o->n * sizeof(double);
    hipError_t e = hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = o->mem.device(o->d_c, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_x, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_g, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_xbest, vbytes);
    if (e == hipSuccess) e = o->mem.device(o->d_ls, sizeof(LmiLoopState));
    if (e == hipSuccess) e = o->mem.device(o->d_cp, sizeof(CutParams));
    if (e == hipSuccess) e = o->mem.device(o->d_zero, sizeof(int));
    if (e == hipSuccess) e = o->mem.pinned(o->h_ls, sizeof(LmiLoopState), hipHostMallocDefault);
    if (e == hipSuccess) e = o->mem.pinned(o->h_cp, sizeof(CutParams), hipHostMallocDefault);
    if (e == hipSuccess) e = o->mem.pinned(o->h_vec, vbytes, hipHostMallocDefault);
    if (e == hipSuccess) e = fill_now(o->d_c, 0, vbytes, o->stream);
    if (e == hipSuccess) e = fill_now(o->d_g, 0, vbytes, o->stream);
    if (e == hipSuccess) e = fill_now(o->d_xbest, 0, vbytes, o->stream);
    if (e == hipSuccess) e = fill_now(o->d_cp, 0, sizeof(CutParams), o->stream);
    if (e == hipSuccess) e = fill_now(o->d_zero, 0, sizeof(int), o->stream);
    if (e == hipSuccess && c) e = hipMemcpy(o->d_c, c, vbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        memset(o->h_ls, 0, sizeof(LmiLoopState));
        o->h_ls->idx = -1;
        o->h_ls->station = -1;
        e = hipMemcpy(o->d_ls, o->h_ls, sizeof(LmiLoopState), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        ellhip_lmi_loop_destroy(o);
        return fail(e == hipErrorOutOfMemory ? ELLHIP_E_NOMEM : ELLHIP_E_HIP, "lmi loop create", e);
    }
    *out = o;
    return 0;
}

int ellhip_lmi_loop_get_idx(ellhip_lmi_loop* o, int* idx_out) {
    if (!o || !idx_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    DeviceGuard guard(o->device);
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(hipMemcpy(o->h_ls, o->d_ls, sizeof(LmiLoopState), hipMemcpyDeviceToHost));
    *idx_out = o->h_ls->idx;
    return 0;
}

int ellhip_lmi_loop_set_idx(ellhip_lmi_loop* o, int idx) {
    if (!o) return fail(ELLHIP_E_INVALID, "NULL handle");
    if (idx < -1 || idx > ll_stations(o) - 1) return fail(ELLHIP_E_INVALID, "lmi loop: idx out of range");
    DeviceGuard guard(o->device);
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(hipMemcpy(reinterpret_cast<char*>(o->d_ls) + offsetof(LmiLoopState, idx), &idx, sizeof(int),
                     hipMemcpyHostToDevice));
    return 0;
}

int ellhip_lmi_loop_assess_optim(ellhip_lmi_loop* o, const double* x, double* gamma_inout, double* g_out,
                                 double* beta_out, int* station_out) {
    if (!o || !x || !gamma_inout || !g_out || !beta_out || !station_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    if (!o->has_c) return fail(ELLHIP_E_INVALID, "lmi loop: assess_optim needs a handle created with an objective");
    return ll_assess_host(o, x, gamma_inout, g_out, beta_out, station_out);
}

int ellhip_lmi_loop_assess_feas(ellhip_lmi_loop* o, const double* x, double* g_out, double* beta_out, int* station_out) {
    if (!o || !x || !g_out || !beta_out || !station_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    if (o->has_c) return fail(ELLHIP_E_INVALID, "lmi loop: assess_feas needs a handle created without an objective");
    return ll_assess_host(o, x, nullptr, g_out, beta_out, station_out);
}

int ellhip_lmi_loop_optim(ellhip_space* s, ellhip_lmi_loop* o, double* gamma_inout, int64_t max_iters, double tol,
                          double* x_best_out, int* has_best_out, int64_t* niter_out) {
    if (!s || !o || !gamma_inout || !has_best_out || !niter_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    if (!o->has_c) return fail(ELLHIP_E_INVALID, "lmi loop: optim needs a handle created with an objective");
    LmiLoopStage stage{o, gamma_inout, x_best_out, has_best_out, niter_out};
    return drive_device_loop(s, stage, o->n, o->device, max_iters, tol);
}

int ellhip_lmi_loop_feas(ellhip_space* s, ellhip_lmi_loop* o, int64_t max_iters, double tol, double* x_out,
                         int* feasible_out, int64_t* niter_out) {
    if (!s || !o || !feasible_out || !niter_out) return fail(ELLHIP_E_INVALID, "NULL argument");
    if (o->has_c) return fail(ELLHIP_E_INVALID, "lmi loop: feas needs a handle created without an objective");
    LmiLoopStage stage{o, nullptr, x_out, feasible_out, niter_out};
    return drive_device_loop(s, stage, o->n, o->device, max_iters, tol);
}

}  // extern "C"
