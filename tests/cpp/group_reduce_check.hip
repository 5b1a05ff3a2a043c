// group_reduce_check.hip -- GPU test (built with hipcc by tests/test_gpu_group_reduce.py): the packed group reduction in its two
// shipped forms (k_group_reduce_p<NP, GROUP_REDUCE_PL_STREAM>, <NP, GROUP_REDUCE_PL_CACHED>, and all three pieces together) against
// the form kept as PL = 0 (group_kernels.hpp), BIT FOR BIT (on the device, word by word) on Y and gpart, from random partial sums.
// Every place the kernel must not read holds a NaN: strips above a column's first strip, row-sum segments beyond i / seg, recorded
// slots >= slot0, the second cut of an odd group's last pair.  The outputs start as NaN words in every run, so a word one form
// leaves unwritten shows as a difference, and a NaN that reaches an output shows in the NaN count.
// Prints one JSON line per case.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/group_kernels.hpp"
using namespace ellhip;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__device__ __forceinline__ double rnd(long long i, unsigned long long salt) {
    unsigned long long h = ((unsigned long long)i + salt) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29; h *= 0x94D049BB133111EBull; h ^= h >> 32;
    return (double)(h & 0xFFFFFFFFFFFFFull) / 4503599627370496.0 - 0.5;
}
__global__ void k_fill(double* p, long long m, unsigned long long salt, double scale) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) p[i] = scale * rnd(i, salt);
}
__global__ void k_set(double* p, long long m, double v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}
// colpart2[p][I][c][2]: NaN where I < c / SYMV_H, and in the .y of the last pair of an odd group; mode 1: every other word -0.0;
// mode 2: the words of columns 70 and n - 1 -0.0
__global__ void k_prep_col(double* cp, long long n, long long nstrips, int npairs, int G, int mode) {
    const long long m = (long long)npairs * nstrips * n * 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(i & 1);
        const long long c = (i >> 1) % n, I = ((i >> 1) / n) % nstrips, p = (i >> 1) / (n * nstrips);
        if (mode == 1 || (mode == 2 && (c == 70 || c == n - 1))) cp[i] = -0.0;
        if (I < c / SYMV_H || (e == 1 && 2 * p + 1 >= G)) cp[i] = __builtin_nan("");
    }
}
// rowpart[l][J][i]: NaN where J > i / seg; modes as above
__global__ void k_prep_row(double* rp, long long n, long long nsegs, long long seg, int G, int mode) {
    const long long m = (long long)G * nsegs * n;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (long long)gridDim.x * blockDim.x) {
        const long long i = k % n, J = (k / n) % nsegs;
        if (mode == 1 || (mode == 2 && (i == 70 || i == n - 1))) rp[k] = -0.0;
        if (J > i / seg) rp[k] = __builtin_nan("");
    }
}
// words that differ between a and b (bit patterns), NaNs in b, negative zeros in b
__global__ void k_diff(const unsigned long long* a, const unsigned long long* b, long long m, unsigned long long* count) {
    unsigned long long c = 0, nn = 0, nz = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        c += a[i] != b[i];
        nn += (b[i] & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
        nz += b[i] == 0x8000000000000000ull;
    }
    if (c) atomicAdd(count, c);
    if (nn) atomicAdd(count + 1, nn);
    if (nz) atomicAdd(count + 2, nz);
}
struct Diff { unsigned long long differing, nans, negzeros; };
static Diff diff(const double* a, const double* b, long long m, unsigned long long* d_cnt) {
    CK(hipMemset(d_cnt, 0, 24));
    hipLaunchKernelGGL(k_diff, dim3(1024), dim3(256), 0, 0, (const unsigned long long*)a, (const unsigned long long*)b, m, d_cnt);
    unsigned long long h[3] = {0, 0, 0};
    CK(hipMemcpy(h, d_cnt, 24, hipMemcpyDeviceToHost));
    return {h[0], h[1], h[2]};
}
static double* dalloc(long long m) {
    double* p = nullptr;
    CK(hipMalloc(&p, (size_t)m * 8));
    return p;
}
static void fill(double* p, long long m, unsigned long long salt, double scale = 1.0) {
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, p, m, salt, scale);
}
static void set(double* p, long long m, double v) { hipLaunchKernelGGL(k_set, dim3(1024), dim3(256), 0, 0, p, m, v); }

template <int NP>
static bool reduce_case(long long n, long long seg, int G, int slot0, int mode) {
    const long long nstrips = (n + SYMV_H - 1) / SYMV_H, nsegs = (n + seg - 1) / seg, nb = (n + 127) / 128;
    const int npairs = (G + 1) / 2;
    const long long rs = nsegs * n, cs = nstrips * n;
    const double nan = __builtin_nan("");
    double* rowp = dalloc(G * rs);
    double* colp = dalloc(2 * npairs * cs);
    double* g = dalloc((long long)G * n);
    double* pend = dalloc((long long)NP * n);
    constexpr int NF = 4;  // PL = 0 and the forms compared with it
    double *Y[NF], *gpart[NF];
    const long long my = (long long)G * n, mg = (long long)G * nb * (NP + 1);
    for (int k = 0; k < NF; ++k) {
        Y[k] = dalloc(my);
        gpart[k] = dalloc(mg);
        set(Y[k], my, nan);
        set(gpart[k], mg, nan);
    }
    DevState* st;
    unsigned long long* d_cnt;
    CK(hipMalloc(&st, sizeof(DevState)));
    CK(hipMemset(st, 0, sizeof(DevState)));
    CK(hipMalloc(&d_cnt, 24));
    fill(rowp, G * rs, 11ull + (unsigned long long)n);
    fill(colp, 2 * npairs * cs, 23ull + (unsigned long long)G);
    fill(g, (long long)G * n, 77ull);
    fill(pend, (long long)NP * n, 5ull);
    if (slot0 < NP) set(pend + (long long)slot0 * n, (long long)(NP - slot0) * n, nan);
    hipLaunchKernelGGL(k_prep_col, dim3(1024), dim3(256), 0, 0, colp, n, nstrips, npairs, G, mode);
    hipLaunchKernelGGL(k_prep_row, dim3(1024), dim3(256), 0, 0, rowp, n, nsegs, seg, G, mode);
    CK(hipGetLastError());
    const dim3 grid((unsigned)nb, (unsigned)npairs);
#define REDUCE_FORM(PL, K)                                                                                                           \
    hipLaunchKernelGGL((k_group_reduce_p<NP, PL>), grid, dim3(256), 0, 0, n, 0ll, n, seg, (const double*)rowp, (const double*)colp, rs, cs, \
                       Y[K], (const double*)g, n, (const double*)pend, gpart[K], (const DevState*)st, G, slot0)
    REDUCE_FORM(0, 0);
    REDUCE_FORM(GROUP_REDUCE_PL_STREAM, 1);
    REDUCE_FORM(GROUP_REDUCE_PL_CACHED, 2);
    REDUCE_FORM(RED_LOOP | RED_NT | RED_HEAVY, 3);
#undef REDUCE_FORM
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    Diff dy = {0, 0, 0}, dg = {0, 0, 0};  // (summed over the forms; the negative zeros: of the streaming form)
    for (int k = 1; k < NF; ++k) {
        const Diff a = diff(Y[0], Y[k], my, d_cnt), b = diff(gpart[0], gpart[k], mg, d_cnt);
        dy.differing += a.differing; dy.nans += a.nans; dg.differing += b.differing; dg.nans += b.nans;
        if (k == 1) dy.negzeros = a.negzeros;
    }
    // (the kept form by itself: it must have written every word from the words it may read)
    const Diff py = diff(Y[1], Y[0], my, d_cnt), pg = diff(gpart[1], gpart[0], mg, d_cnt);
    const bool ok = dy.differing == 0 && dg.differing == 0 && dy.nans == 0 && dg.nans == 0 && py.nans == 0 && pg.nans == 0;
    printf("{\"kernel\": \"reduce\", \"n\": %lld, \"seg\": %lld, \"G\": %d, \"np\": %d, \"slot0\": %d, \"mode\": %d, \"strips\": %lld, "
           "\"y_words_differing\": %llu, \"gpart_words_differing\": %llu, \"y_nans\": %llu, \"gpart_nans\": %llu, \"parent_nans\": %llu, "
           "\"y_negzeros\": %llu, \"forms\": %d, \"ok\": %s}\n",
           n, seg, G, NP, slot0, mode, nstrips, dy.differing, dg.differing, dy.nans, dg.nans, py.nans + pg.nans, dy.negzeros, NF - 1,
           ok ? "true" : "false");
    for (int k = 0; k < NF; ++k) {
        CK(hipFree(Y[k]));
        CK(hipFree(gpart[k]));
    }
    CK(hipFree(rowp)); CK(hipFree(colp)); CK(hipFree(g)); CK(hipFree(pend)); CK(hipFree(st)); CK(hipFree(d_cnt));
    return ok;
}

int main() {
    bool ok = true;
    // n = 192: 3 strips, the clamped trip only; 4096: 64 strips, wave 0 of block 0 ends exactly at 4 u + w = nstrips (one full trip and
    // no clamped one); 4160: 65 strips, a second, clamped trip for wave 0 only; 8256: 129 strips
    ok &= reduce_case<48>(192, 512, 1, 0, 0);
    ok &= reduce_case<48>(192, 2048, 2, 16, 0);
    ok &= reduce_case<48>(192, 512, 15, 32, 0);
    ok &= reduce_case<24>(192, 512, 31, 8, 0);
    ok &= reduce_case<48>(4096, 512, 16, 32, 0);
    ok &= reduce_case<48>(4096, 2048, 32, 0, 0);
    ok &= reduce_case<48>(4160, 512, 32, 16, 0);
    ok &= reduce_case<48>(4160, 2048, 15, 0, 0);
    ok &= reduce_case<24>(4160, 512, 2, 8, 0);
    ok &= reduce_case<48>(8256, 2048, 32, 0, 0);
    ok &= reduce_case<48>(8256, 512, 31, 32, 0);
    ok &= reduce_case<48>(8256, 2048, 16, 16, 0);
    ok &= reduce_case<24>(8256, 512, 1, 8, 0);
    // negative zero: every partial sum -0.0; two columns whose true sum is -0.0 among random ones
    ok &= reduce_case<48>(4160, 512, 32, 16, 1);
    ok &= reduce_case<48>(4160, 512, 31, 16, 2);
    return ok ? 0 : 1;
}
