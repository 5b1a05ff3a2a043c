// apply_symm_check.hip -- GPU test (built with hipcc by tests/test_gpu_apply_symm.py): the fused apply + product pass
// (k_apply_symm_q: NP recorded updates applied to each block of the lower triangle in registers, then the next group's column and
// row products formed from the updated block) against the two passes it replaces, k_apply_mfma<NP> followed by k_symm_mfma_q
// (<= 16 gradients) or k_symm_mfma_q2 (<= 32), on random Q (upper triangle included), pending vectors, coefficients and
// gradients.  Q, rowpart and colpart are compared BIT FOR BIT (on the device, word by word); with the queue halted the update must
// still land and the products must not be written.  Prints one JSON line per case.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/ell_kernels.hpp"
using namespace ellhip;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__global__ void k_fill(double* p, long long m, unsigned long long salt, double scale) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        unsigned long long h = ((unsigned long long)i + salt) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29; h *= 0x94D049BB133111EBull; h ^= h >> 32;
        p[i] = scale * ((double)(h & 0xFFFFFFFFFFFFFull) / 4503599627370496.0 - 0.5);
    }
}

// words that differ between a and b (bit patterns)
__global__ void k_diff(const unsigned long long* a, const unsigned long long* b, long long m, unsigned long long* count) {
    unsigned long long c = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) c += a[i] != b[i];
    if (c) atomicAdd(count, c);
}

static unsigned long long diff(const double* a, const double* b, long long m, unsigned long long* d_cnt) {
    CK(hipMemset(d_cnt, 0, 8));
    hipLaunchKernelGGL(k_diff, dim3(1024), dim3(256), 0, 0, (const unsigned long long*)a, (const unsigned long long*)b, m, d_cnt);
    unsigned long long h = 0;
    CK(hipMemcpy(&h, d_cnt, 8, hipMemcpyDeviceToHost));
    return h;
}

template <int NP, int SEG>
static bool run_case(long long n, int lv, bool halted) {
    const long long ld = n + 16, nrows = n;
    const long long nstrips = nrows / SYMV_H, nsegs = (n + SEG - 1) / SEG, rs = nsegs * n, cs = nstrips * n;
    const bool wide = lv > 16;
    const int nvw = wide ? 32 : 16;
    double *Q0, *Q[2], *pend, *cpend, *g, *gT, *rp[2], *cp[2];
    DevState* st;
    unsigned long long* d_cnt;
    CK(hipMalloc(&Q0, (size_t)nrows * ld * 8));
    for (int k = 0; k < 2; ++k) {
        CK(hipMalloc(&Q[k], (size_t)nrows * ld * 8));
        CK(hipMalloc(&rp[k], (size_t)32 * rs * 8));
        CK(hipMalloc(&cp[k], (size_t)32 * cs * 8));
        CK(hipMemset(rp[k], 0, (size_t)32 * rs * 8));
        CK(hipMemset(cp[k], 0, (size_t)32 * cs * 8));
    }
    CK(hipMalloc(&pend, (size_t)MAXPEND * n * 8));
    CK(hipMalloc(&cpend, (size_t)MAXPEND * 8));
    CK(hipMalloc(&g, (size_t)32 * n * 8));
    CK(hipMalloc(&gT, (size_t)32 * n * 8));
    CK(hipMalloc(&st, sizeof(DevState)));
    CK(hipMalloc(&d_cnt, 8));
    DevState hs;
    memset(&hs, 0, sizeof(hs));
    hs.halted = halted ? 1 : 0;
    CK(hipMemcpy(st, &hs, sizeof(hs), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, Q0, nrows * ld, 1ull + (unsigned long long)n, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, pend, (long long)MAXPEND * n, 5ull + (unsigned long long)lv, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, 0, cpend, (long long)MAXPEND, 9ull, 0.01);
    hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, 0, g, 32 * n, 77ull, 1.0);
    for (int k = 0; k < 2; ++k) CK(hipMemcpy(Q[k], Q0, (size_t)nrows * ld * 8, hipMemcpyDeviceToDevice));
    std::vector<SymmTile> tl;
    for (long long I = nstrips - 1; I >= 0; --I)
        for (long long J = 0; J < nsegs; ++J)
            if (J * SEG <= I * SYMV_H + SYMV_H - 1) tl.push_back({(int)I, (int)J});
    auto blocks_of = [&](const SymmTile& t) {
        const long long r0 = (long long)t.I * SYMV_H, c0 = (long long)t.J * SEG;
        return (std::min<long long>(c0 + SEG, r0 + SYMV_H) - c0) / 16;
    };
    std::stable_sort(tl.begin(), tl.end(), [&](const SymmTile& a, const SymmTile& b) { return blocks_of(a) > blocks_of(b); });
    SymmTile* d_tl;
    unsigned* d_q;
    CK(hipMalloc(&d_tl, tl.size() * sizeof(SymmTile)));
    CK(hipMalloc(&d_q, 256));
    CK(hipMemcpy(d_tl, tl.data(), tl.size() * sizeof(SymmTile), hipMemcpyHostToDevice));
    const int ntiles = (int)tl.size(), wgs = 512;
    // the two passes -> Q[0], sets 0
    const dim3 g2((unsigned)((nrows + APM_ROWS - 1) / APM_ROWS), (unsigned)((n + APM_COLS - 1) / APM_COLS));
    hipLaunchKernelGGL((k_apply_mfma<NP, true>), g2, dim3(256), 0, 0, Q[0], ld, n, nrows, 0ll, (const double*)pend, (const double*)cpend,
                       (const DevState*)st);
    hipLaunchKernelGGL(k_pack_grads, dim3((unsigned)((n * nvw + 255) / 256)), dim3(256), 0, 0, (const double*)g, n, lv, n, gT, d_q, nvw);
    if (!wide)
        hipLaunchKernelGGL((k_symm_mfma_q<true, SEG>), dim3((unsigned)wgs), dim3(256), 0, 0, (const double*)Q[0], ld, n, 0ll, (const double*)gT, lv,
                           rp[0], cp[0], rs, cs, (const DevState*)st, (const SymmTile*)d_tl, ntiles, d_q);
    else
        hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG>), dim3((unsigned)wgs), dim3(256), 0, 0, (const double*)Q[0], ld, n, 0ll, (const double*)gT, lv,
                           rp[0], cp[0], rs, cs, (const DevState*)st, (const SymmTile*)d_tl, ntiles, d_q);
    CK(hipGetLastError());
    // the fused pass -> Q[1], sets 1 (k_pack_grads rewinds the counter, as in the product)
    hipLaunchKernelGGL(k_pack_grads, dim3((unsigned)((n * nvw + 255) / 256)), dim3(256), 0, 0, (const double*)g, n, lv, n, gT, d_q, nvw);
    if (!wide)
        hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false>), dim3((unsigned)wgs), dim3(256), 0, 0, Q[1], ld, n, (const double*)pend,
                           (const double*)cpend, (const double*)gT, lv, rp[1], cp[1], rs, cs, (const DevState*)st, (const SymmTile*)d_tl, ntiles, d_q);
    else
        hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true>), dim3((unsigned)wgs), dim3(256), 0, 0, Q[1], ld, n, (const double*)pend,
                           (const double*)cpend, (const double*)gT, lv, rp[1], cp[1], rs, cs, (const DevState*)st, (const SymmTile*)d_tl, ntiles, d_q);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const unsigned long long dq = diff(Q[0], Q[1], nrows * ld, d_cnt);
    const unsigned long long dr = diff(rp[0], rp[1], 32 * rs, d_cnt);
    const unsigned long long dcn = diff(cp[0], cp[1], 32 * cs, d_cnt);
    const unsigned long long moved = diff(Q0, Q[1], nrows * ld, d_cnt);  // elements the update changed
    std::vector<double> h((size_t)32 * rs);
    CK(hipMemcpy(h.data(), rp[1], (size_t)32 * rs * 8, hipMemcpyDeviceToHost));
    double rsum = 0.0;
    for (double v : h) rsum += v * v;
    unsigned hq = 0;
    CK(hipMemcpy(&hq, d_q, 4, hipMemcpyDeviceToHost));
    // the update reaches every element of the trapezoid k_apply_mfma writes (all but a few that round back to themselves)
    const long long trap = (nstrips * (nstrips + 1) / 2) * SYMV_H * SYMV_H;
    const bool applied = moved > (unsigned long long)(trap * 9 / 10) && moved <= (unsigned long long)trap;
    const bool products = halted ? rsum == 0.0 : rsum > 0.0;
    printf("{\"n\": %lld, \"np\": %d, \"seg\": %d, \"gradients\": %d, \"halted\": %s, \"tiles\": %d, \"q_words_differing\": %llu, "
           "\"rowpart_words_differing\": %llu, \"colpart_words_differing\": %llu, \"q_words_updated\": %llu, \"trapezoid\": %lld, "
           "\"applied\": %s, \"products_as_expected\": %s, \"queue_drawn\": %u}\n",
           n, NP, SEG, lv, halted ? "true" : "false", ntiles, dq, dr, dcn, moved, trap, applied ? "true" : "false",
           products ? "true" : "false", hq);
    fflush(stdout);
    for (int k = 0; k < 2; ++k) {
        CK(hipFree(Q[k]));
        CK(hipFree(rp[k]));
        CK(hipFree(cp[k]));
    }
    CK(hipFree(Q0)); CK(hipFree(pend)); CK(hipFree(cpend)); CK(hipFree(g)); CK(hipFree(gT)); CK(hipFree(st)); CK(hipFree(d_cnt));
    CK(hipFree(d_tl)); CK(hipFree(d_q));
    return dq == 0 && dr == 0 && dcn == 0 && applied && products;
}

int main() {
    bool ok = true;
    // n = 5120 takes the narrow segments (fewer than 200 tiles of 64 x 2048), n = 16384 the wide ones, as a handle does
    ok = run_case<48, SYMV_SEG_SMALL>(5120, 32, false) && ok;
    ok = run_case<24, SYMV_SEG_SMALL>(5120, 17, false) && ok;
    ok = run_case<48, SYMV_SEG_SMALL>(5120, 2, false) && ok;
    ok = run_case<24, SYMV_SEG_SMALL>(5120, 16, false) && ok;
    ok = run_case<48, SYMV_SEG_SMALL>(5120, 20, true) && ok;
    ok = run_case<48, SYMV_SEG>(16384, 32, false) && ok;
    ok = run_case<48, SYMV_SEG>(16384, 16, false) && ok;
    ok = run_case<24, SYMV_SEG>(16384, 20, false) && ok;
    ok = run_case<48, SYMV_SEG>(16384, 8, false) && ok;
    ok = run_case<24, SYMV_SEG>(16384, 2, false) && ok;
    ok = run_case<48, SYMV_SEG>(16384, 17, true) && ok;
    return ok ? 0 : 1;
}
