// packed_operands_check.hip -- GPU test (built with hipcc by tests/test_gpu_packed_operands.py): the packed forms of the
// matrix-core passes (ELLHIP_OPT_PACKED_OPERANDS: k_pack_operands, k_apply_symm_q<.., true>, k_symm_mfma_q / _q2<.., true>,
// k_group_reduce_p) against the unpacked kernels on the same random Q, recorded vectors, coefficients and gradients.  Compared BIT
// FOR BIT on the device: Q after the fused pass, rowpart, colpart (after undoing the pairing of colpart2), and Y / gpart of the two
// reduce forms for 0, 16 and 48 recorded slots.  Small shapes with full tiles, diagonal tiles and a partial last segment; one
// shape with more than 64 strips for the reduce kernels' unrolled strip loops.  Prints one JSON line per case.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/group_kernels.hpp"
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

// colpart2[p][I][c][2] -> colpart[v][I][c] for the cuts v < lv (cs = strips x n)
__global__ void k_unpair(const double* cp2, double* cp, long long cs, int lv) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)lv * cs; i += (long long)gridDim.x * blockDim.x) {
        const long long v = i / cs, k = i % cs;
        cp[i] = cp2[2 * ((v >> 1) * cs + k) + (v & 1)];
    }
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
    const long long nb = (n + 127) / 128, gp_elems = 32 * nb * (NP + 1);
    const bool wide = lv > 16;
    const int nvt = wide ? 2 : 1, nvw = 16 * nvt;
    // [0]: unpacked, [1]: packed; rp / cp: the fused pass' sets, rq / cq: the product pass' sets; cu: colpart2 with the pairing undone
    double *Q0, *Q[2], *pend, *pendP, *cpend, *g, *gT[2], *rp[2], *cp[2], *rq[2], *cq[2], *cu, *Y[2], *gpart[2];
    DevState* st;
    unsigned long long* d_cnt;
    CK(hipMalloc(&Q0, (size_t)nrows * ld * 8));
    for (int k = 0; k < 2; ++k) {
        CK(hipMalloc(&Q[k], (size_t)nrows * ld * 8));
        CK(hipMalloc(&gT[k], (size_t)32 * n * 8));
        CK(hipMalloc(&rp[k], (size_t)32 * rs * 8));
        CK(hipMalloc(&cp[k], (size_t)32 * cs * 8));
        CK(hipMalloc(&rq[k], (size_t)32 * rs * 8));
        CK(hipMalloc(&cq[k], (size_t)32 * cs * 8));
        CK(hipMalloc(&Y[k], (size_t)32 * n * 8));
        CK(hipMalloc(&gpart[k], (size_t)gp_elems * 8));
        CK(hipMemset(rp[k], 0, (size_t)32 * rs * 8));
        CK(hipMemset(cp[k], 0, (size_t)32 * cs * 8));
        CK(hipMemset(rq[k], 0, (size_t)32 * rs * 8));
        CK(hipMemset(cq[k], 0, (size_t)32 * cs * 8));
    }
    CK(hipMalloc(&cu, (size_t)32 * cs * 8));
    CK(hipMalloc(&pend, (size_t)MAXPEND * n * 8));
    CK(hipMalloc(&pendP, (size_t)MAXPEND * n * 8));
    CK(hipMalloc(&cpend, (size_t)MAXPEND * 8));
    CK(hipMalloc(&g, (size_t)32 * n * 8));
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
    const int ntiles = (int)tl.size(), wgs = 64;
    const dim3 gu((unsigned)((n * nvw + 255) / 256)), gpk((unsigned)(n * nvt / 32)), gpk2((unsigned)(n * nvt / 32 + n * (NP / 8) / 64));
#define ARGS_APPLY(k) Q[k], ld, n, (const double*)pend, (const double*)cpend, (const double*)gT[k], lv, rp[k], cp[k], rs, cs, (const DevState*)st, \
                      (const SymmTile*)d_tl, ntiles, d_q
#define ARGS_SYMM(k) (const double*)Q[k], ld, n, 0ll, (const double*)gT[k], lv, rq[k], cq[k], rs, cs, (const DevState*)st, (const SymmTile*)d_tl, ntiles, d_q
    // the fused pass, unpacked -> Q[0], sets 0; packed -> Q[1], sets 1
    hipLaunchKernelGGL(k_pack_grads, gu, dim3(256), 0, 0, (const double*)g, n, lv, n, gT[0], d_q, nvw);
    if (!wide) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(0));
    else hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(0));
    hipLaunchKernelGGL(k_pack_operands, gpk2, dim3(256), 0, 0, (const double*)g, n, lv, n, gT[1], d_q, nvt, (const double*)pend, pendP, NP / 8);
    if (!wide) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false, true>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(1), (const double*)pendP);
    else hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true, true>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(1), (const double*)pendP);
    CK(hipGetLastError());
    // the product passes on the updated matrices (equal, if the fused passes agree)
    hipLaunchKernelGGL(k_pack_grads, gu, dim3(256), 0, 0, (const double*)g, n, lv, n, gT[0], d_q, nvw);
    if (!wide) hipLaunchKernelGGL((k_symm_mfma_q<true, SEG>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_SYMM(0));
    else hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_SYMM(0));
    hipLaunchKernelGGL(k_pack_operands, gpk, dim3(256), 0, 0, (const double*)g, n, lv, n, gT[1], d_q, nvt, (const double*)nullptr, (double*)nullptr, 0);
    if (!wide) hipLaunchKernelGGL((k_symm_mfma_q<true, SEG, true>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_SYMM(1));
    else hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG, true>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_SYMM(1));
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
#undef ARGS_APPLY
#undef ARGS_SYMM
    unsigned hq = 0;
    CK(hipMemcpy(&hq, d_q, 4, hipMemcpyDeviceToHost));
    const unsigned long long dq = diff(Q[0], Q[1], nrows * ld, d_cnt);
    const unsigned long long moved = diff(Q0, Q[1], nrows * ld, d_cnt);
    const unsigned long long dr = diff(rp[0], rp[1], 32 * rs, d_cnt) + diff(rq[0], rq[1], 32 * rs, d_cnt);
    unsigned long long dcn = 0;
    for (double* c2 : {cp[1], cq[1]}) {
        CK(hipMemset(cu, 0, (size_t)32 * cs * 8));
        hipLaunchKernelGGL(k_unpair, dim3(1024), dim3(256), 0, 0, (const double*)c2, cu, cs, lv);
        dcn += diff(c2 == cp[1] ? cp[0] : cq[0], cu, 32 * cs, d_cnt);
    }
    // the products are there (or, halted, are not)
    std::vector<double> h((size_t)32 * cs);
    CK(hipMemcpy(h.data(), cq[1], (size_t)32 * cs * 8, hipMemcpyDeviceToHost));
    double csum = 0.0;
    for (double v : h) csum += v * v;
    const bool products = halted ? csum == 0.0 : csum > 0.0;
    const long long trap = (nstrips * (nstrips + 1) / 2) * SYMV_H * SYMV_H;
    const bool applied = moved > (unsigned long long)(trap * 9 / 10) && moved <= (unsigned long long)trap;
    // the two reduce forms on the product pass' sets, for 0 / 16 / 48 recorded slots
    unsigned long long dy = 0, dg = 0;
    double ysum = 0.0;
    for (int np_used : {0, 16, 48}) {
        for (int k = 0; k < 2; ++k) {
            CK(hipMemset(Y[k], 0, (size_t)32 * n * 8));
            CK(hipMemset(gpart[k], 0, (size_t)gp_elems * 8));
        }
        hipLaunchKernelGGL(k_group_reduce<NP>, dim3((unsigned)nb, (unsigned)lv), dim3(256), 0, 0, n, 0ll, nrows, (long long)SEG, (const double*)rq[0],
                           (const double*)cq[0], rs, cs, Y[0], (const double*)g, n, (const double*)pend, gpart[0], (const DevState*)st, np_used);
        hipLaunchKernelGGL(k_group_reduce_p<NP>, dim3((unsigned)nb, (unsigned)(lv + 1) / 2), dim3(256), 0, 0, n, 0ll, nrows, (long long)SEG,
                           (const double*)rq[1], (const double*)cq[1], rs, cs, Y[1], (const double*)g, n, (const double*)pend, gpart[1],
                           (const DevState*)st, lv, np_used);
        CK(hipGetLastError());
        dy += diff(Y[0], Y[1], 32 * n, d_cnt);
        dg += diff(gpart[0], gpart[1], gp_elems, d_cnt);
        std::vector<double> hy((size_t)32 * n);
        CK(hipMemcpy(hy.data(), Y[1], (size_t)32 * n * 8, hipMemcpyDeviceToHost));
        for (double v : hy) ysum += v * v;
    }
    const bool reduced = halted ? ysum == 0.0 : ysum > 0.0;
    printf("{\"n\": %lld, \"np\": %d, \"seg\": %d, \"gradients\": %d, \"halted\": %s, \"tiles\": %d, \"strips\": %lld, \"q_words_differing\": %llu, "
           "\"rowpart_words_differing\": %llu, \"colpart_words_differing\": %llu, \"y_words_differing\": %llu, "
           "\"gpart_words_differing\": %llu, \"applied\": %s, \"products_as_expected\": %s, \"reduced_as_expected\": %s, "
           "\"queue_drawn\": %u}\n",
           n, NP, SEG, lv, halted ? "true" : "false", ntiles, nstrips, dq, dr, dcn, dy, dg, applied ? "true" : "false",
           products ? "true" : "false", reduced ? "true" : "false", hq);
    fflush(stdout);
    for (int k = 0; k < 2; ++k) {
        CK(hipFree(Q[k])); CK(hipFree(gT[k])); CK(hipFree(rp[k])); CK(hipFree(cp[k])); CK(hipFree(rq[k])); CK(hipFree(cq[k]));
        CK(hipFree(Y[k])); CK(hipFree(gpart[k]));
    }
    CK(hipFree(Q0)); CK(hipFree(cu)); CK(hipFree(pend)); CK(hipFree(pendP)); CK(hipFree(cpend)); CK(hipFree(g)); CK(hipFree(st));
    CK(hipFree(d_cnt)); CK(hipFree(d_tl)); CK(hipFree(d_q));
    return dq == 0 && dr == 0 && dcn == 0 && dy == 0 && dg == 0 && applied && products && reduced;
}

int main() {
    bool ok = true;
    // narrow segments: n = 320 is one partial segment, n = 1088 two full ones and a partial one of 64 columns
    const int lvs[7] = {2, 15, 16, 17, 20, 31, 32};
    for (long long n : {320ll, 1088ll})
        for (int k = 0; k < 7; ++k) {
            if ((k + (n == 320)) & 1) ok = run_case<48, SYMV_SEG_SMALL>(n, lvs[k], false) && ok;
            else ok = run_case<24, SYMV_SEG_SMALL>(n, lvs[k], false) && ok;
        }
    ok = run_case<48, SYMV_SEG_SMALL>(320, 20, true) && ok;
    // wide segments: every tile ends at the diagonal
    ok = run_case<48, SYMV_SEG>(320, 32, false) && ok;
    ok = run_case<24, SYMV_SEG>(320, 17, false) && ok;
    ok = run_case<48, SYMV_SEG>(1088, 2, false) && ok;
    ok = run_case<24, SYMV_SEG>(1088, 15, false) && ok;
    ok = run_case<48, SYMV_SEG>(1088, 32, false) && ok;
    ok = run_case<24, SYMV_SEG>(1088, 17, true) && ok;
    // 65 strips: the first columns go through the reduce kernels' 16- and 8-deep strip loops
    ok = run_case<48, SYMV_SEG_SMALL>(4160, 31, false) && ok;
    return ok ? 0 : 1;
}
