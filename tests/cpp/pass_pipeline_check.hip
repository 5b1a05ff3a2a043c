// pass_pipeline_check.hip -- GPU test (built with hipcc by tests/test_gpu_pass_pipeline.py): the block loops of the 32-wide product
// pass (k_symm_mfma_q2) and of the fused apply + product pass (k_apply_symm_q) as shipped -- rotated, with the strip's A operands
// in pairs and the update accumulators taken one after the other (PL_ROTATE | PL_SGR2 | PL_ACC, csrc/ell_kernels.hpp) -- against
// the loops they replace (PL = 0) on the same random Q, recorded vectors, coefficients and gradients.  Q, rowpart and colpart are
// compared BIT FOR BIT on the device.  NaN sits in the strict upper triangle of Q (and its padding columns) and in every slot of
// the partial sums before a pass runs: a prefetch that strays, a mask that slips or a slot written by one loop only shows as a
// differing word, and the number of slots written is held against the count the tile table gives.
// Shapes: n = 64 (one block: three waves of a workgroup have none), 128 (a diagonal block as a wave's only block), 576, 1088
// (full and partial segments of 512 columns), 2112 and 4160 (segments of 2048: 32 and 33 blocks per wave); 1 .. 32 gradients, ranks
// 24 and 48, queue halted and not, packed and unpacked operands.  Prints one JSON line per case.
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
__global__ void k_nan(unsigned long long* p, long long m) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) p[i] = 0x7FF8000000000000ull;
}
// NaN right of the diagonal (padding columns included)
__global__ void k_nan_upper(unsigned long long* q, long long nrows, long long ld) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nrows * ld; i += (long long)gridDim.x * blockDim.x)
        if (i % ld > i / ld) q[i] = 0x7FF8000000000000ull;
}
// [0]: words that differ between a and b (bit patterns), [1]: words of b that are not NaN
__global__ void k_diff(const unsigned long long* a, const unsigned long long* b, const double* bd, long long m, unsigned long long* count) {
    unsigned long long c = 0, f = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        c += a[i] != b[i];
        f += bd[i] == bd[i];
    }
    if (c) atomicAdd(count, c);
    if (f) atomicAdd(count + 1, f);
}

struct Diff {
    unsigned long long differing, written;
};
static Diff diff(const double* a, const double* b, long long m, unsigned long long* d_cnt) {
    CK(hipMemset(d_cnt, 0, 16));
    hipLaunchKernelGGL(k_diff, dim3(1024), dim3(256), 0, 0, (const unsigned long long*)a, (const unsigned long long*)b, b, m, d_cnt);
    unsigned long long h[2] = {0, 0};
    CK(hipMemcpy(h, d_cnt, 16, hipMemcpyDeviceToHost));
    return {h[0], h[1]};
}
static void fill_nan(double* p, long long m) {
    hipLaunchKernelGGL(k_nan, dim3(1024), dim3(256), 0, 0, (unsigned long long*)p, m);
}

// the buffers of the largest case, allocated once
struct Buffers {
    double *Q0, *Q[2], *pend, *pendP, *cpend, *g, *gT, *rp[2], *cp[2];
    DevState* st;
    unsigned long long* d_cnt;
    SymmTile* d_tl;
    unsigned* d_q;
};
constexpr long long NMAX = 4160, TILES_MAX = 4096;

static Buffers allocate() {
    Buffers B;
    const long long ld = NMAX + 16, rs = ((NMAX + SYMV_SEG_SMALL - 1) / SYMV_SEG_SMALL) * NMAX, cs = (NMAX / SYMV_H) * NMAX;
    CK(hipMalloc(&B.Q0, (size_t)NMAX * ld * 8));
    for (int k = 0; k < 2; ++k) {
        CK(hipMalloc(&B.Q[k], (size_t)NMAX * ld * 8));
        CK(hipMalloc(&B.rp[k], (size_t)32 * rs * 8));
        CK(hipMalloc(&B.cp[k], (size_t)32 * cs * 8));
    }
    CK(hipMalloc(&B.pend, (size_t)MAXPEND * NMAX * 8));
    CK(hipMalloc(&B.pendP, (size_t)MAXPEND * NMAX * 8));
    CK(hipMalloc(&B.cpend, (size_t)MAXPEND * 8));
    CK(hipMalloc(&B.g, (size_t)32 * NMAX * 8));
    CK(hipMalloc(&B.gT, (size_t)32 * NMAX * 8));
    CK(hipMalloc(&B.st, sizeof(DevState)));
    CK(hipMalloc(&B.d_cnt, 16));
    CK(hipMalloc(&B.d_tl, TILES_MAX * sizeof(SymmTile)));
    CK(hipMalloc(&B.d_q, 256));
    return B;
}

template <int NP, int SEG, bool PK>
static bool run_case(const Buffers& B, long long n, int lv, bool halted) {
    const long long ld = n + 16, nrows = n;
    const long long nstrips = nrows / SYMV_H, nsegs = (n + SEG - 1) / SEG, rs = nsegs * n, cs = nstrips * n;
    const bool wide = lv > 16;
    const int nvt = wide ? 2 : 1;
    DevState hs;
    memset(&hs, 0, sizeof(hs));
    hs.halted = halted ? 1 : 0;
    CK(hipMemcpy(B.st, &hs, sizeof(hs), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, B.Q0, nrows * ld, 1ull + (unsigned long long)n, 1.0);
    hipLaunchKernelGGL(k_nan_upper, dim3(1024), dim3(256), 0, 0, (unsigned long long*)B.Q0, nrows, ld);
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, B.pend, (long long)MAXPEND * n, 5ull + (unsigned long long)lv, 1.0);
    hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, 0, B.cpend, (long long)MAXPEND, 9ull, 0.01);
    hipLaunchKernelGGL(k_fill, dim3(256), dim3(256), 0, 0, B.g, 32 * n, 77ull, 1.0);
    std::vector<SymmTile> tl;
    for (long long I = nstrips - 1; I >= 0; --I)
        for (long long J = 0; J < nsegs; ++J)
            if (J * SEG <= I * SYMV_H + SYMV_H - 1) tl.push_back({(int)I, (int)J});
    auto blocks_of = [&](const SymmTile& t) {
        const long long r0 = (long long)t.I * SYMV_H, c0 = (long long)t.J * SEG;
        return (std::min<long long>(c0 + SEG, r0 + SYMV_H) - c0) / 16;
    };
    std::stable_sort(tl.begin(), tl.end(), [&](const SymmTile& a, const SymmTile& b) { return blocks_of(a) > blocks_of(b); });
    if ((long long)tl.size() > TILES_MAX) exit(3);
    long long nblocks = 0;
    for (const SymmTile& t : tl) nblocks += blocks_of(t);
    CK(hipMemcpy(B.d_tl, tl.data(), tl.size() * sizeof(SymmTile), hipMemcpyHostToDevice));
    const int ntiles = (int)tl.size(), wgs = 64;
    // slots a pass writes: 64 rows per tile and gradient; 16 columns per block and gradient (packed: per gradient of a started pair)
    const unsigned long long rows_written = halted ? 0 : (unsigned long long)ntiles * 64 * lv;
    const unsigned long long cols_written = halted ? 0 : (unsigned long long)nblocks * 16 * (PK ? 2 * ((lv + 1) / 2) : lv);
    auto pack = [&](int t) {  // the operands of a pass over t 16-wide column tiles; both forms rewind the tile queue
        if (PK)
            hipLaunchKernelGGL(k_pack_operands, dim3((unsigned)(n * t / 32 + n * (NP / 8) / 64)), dim3(256), 0, 0, (const double*)B.g, n, lv, n, B.gT,
                               B.d_q, t, (const double*)B.pend, B.pendP, NP / 8);
        else
            hipLaunchKernelGGL(k_pack_grads, dim3((unsigned)((n * 16 * t + 255) / 256)), dim3(256), 0, 0, (const double*)B.g, n, lv, n, B.gT, B.d_q, 16 * t);
    };
    unsigned long long dq = 0, dr = 0, dcn = 0, moved = 0;
    bool counts = true;
    unsigned drawn = ~0u;
    auto note_queue = [&] {
        unsigned hq = 0;
        CK(hipMemcpy(&hq, B.d_q, 4, hipMemcpyDeviceToHost));
        drawn = std::min(drawn, hq);
    };
    // 1. the 32-wide product pass on Q0: sets 0 from the old loop, sets 1 from the shipped one
    for (int k = 0; k < 2; ++k) {
        fill_nan(B.rp[k], 32 * rs);
        fill_nan(B.cp[k], 32 * cs);
    }
#define ARGS_SYMM(k) (const double*)B.Q0, ld, n, 0ll, (const double*)B.gT, lv, B.rp[k], B.cp[k], rs, cs, (const DevState*)B.st, (const SymmTile*)B.d_tl, ntiles, B.d_q
    pack(2);
    hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG, PK, 0>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_SYMM(0));
    pack(2);
    hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG, PK>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_SYMM(1));
#undef ARGS_SYMM
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (!halted) note_queue();
    {
        const Diff r = diff(B.rp[0], B.rp[1], 32 * rs, B.d_cnt), c = diff(B.cp[0], B.cp[1], 32 * cs, B.d_cnt);
        dr += r.differing, dcn += c.differing;
        counts = counts && r.written == rows_written && c.written == cols_written;
    }
    // 2. the fused pass: Q[0] and sets 0 from the old loop, Q[1] and sets 1 from the shipped one
    for (int k = 0; k < 2; ++k) {
        CK(hipMemcpy(B.Q[k], B.Q0, (size_t)nrows * ld * 8, hipMemcpyDeviceToDevice));
        fill_nan(B.rp[k], 32 * rs);
        fill_nan(B.cp[k], 32 * cs);
    }
#define ARGS_APPLY(k) B.Q[k], ld, n, (const double*)B.pend, (const double*)B.cpend, (const double*)B.gT, lv, B.rp[k], B.cp[k], rs, cs, (const DevState*)B.st, \
                      (const SymmTile*)B.d_tl, ntiles, B.d_q, (const double*)B.pendP
    pack(nvt);
    if (wide) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true, PK, 0>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(0));
    else hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false, PK, 0>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(0));
    pack(nvt);
    if (wide) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true, PK>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(1));
    else hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false, PK>), dim3((unsigned)wgs), dim3(256), 0, 0, ARGS_APPLY(1));
#undef ARGS_APPLY
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    note_queue();
    {
        const Diff q = diff(B.Q[0], B.Q[1], nrows * ld, B.d_cnt), r = diff(B.rp[0], B.rp[1], 32 * rs, B.d_cnt),
                   c = diff(B.cp[0], B.cp[1], 32 * cs, B.d_cnt);
        dq += q.differing, dr += r.differing, dcn += c.differing;
        counts = counts && r.written == rows_written && c.written == cols_written;
        // NaN stays where it was: the lower triangle of the updated matrix is finite, nothing right of the diagonal is
        counts = counts && q.written == (unsigned long long)(nrows * (nrows + 1) / 2);
        moved = diff(B.Q0, B.Q[1], nrows * ld, B.d_cnt).differing;  // elements the update changed
    }
    const long long tri = nrows * (nrows + 1) / 2;
    const bool applied = moved > (unsigned long long)(tri * 9 / 10);  // (all but a few that round back to themselves)
    printf("{\"n\": %lld, \"np\": %d, \"seg\": %d, \"packed\": %s, \"gradients\": %d, \"halted\": %s, \"tiles\": %d, \"blocks\": %lld, "
           "\"q_words_differing\": %llu, \"rowpart_words_differing\": %llu, \"colpart_words_differing\": %llu, \"applied\": %s, "
           "\"slots_written_as_expected\": %s, \"queue_drawn\": %u}\n",
           n, NP, SEG, PK ? "true" : "false", lv, halted ? "true" : "false", ntiles, nblocks, dq, dr, dcn, applied ? "true" : "false",
           counts ? "true" : "false", drawn);
    fflush(stdout);
    return dq == 0 && dr == 0 && dcn == 0 && applied && counts;
}

template <int SEG>
static bool run_shape(const Buffers& B, long long n) {
    bool ok = true;
    for (int lv : {1, 16, 17, 31, 32})
        for (int halted = 0; halted < 2; ++halted) {
            ok = run_case<24, SEG, false>(B, n, lv, halted != 0) && ok;
            ok = run_case<24, SEG, true>(B, n, lv, halted != 0) && ok;
            ok = run_case<48, SEG, false>(B, n, lv, halted != 0) && ok;
            ok = run_case<48, SEG, true>(B, n, lv, halted != 0) && ok;
        }
    return ok;
}

int main() {
    static_assert(SYMV_SEG_SMALL == 512 && SYMV_SEG == 2048, "segment widths of the cases below");
    static_assert(SYMM2_PL != 0 && APPLY_SYMM_PL != 0, "the shipped loops are the old ones: nothing to compare");
    const Buffers B = allocate();
    bool ok = true;
    for (long long n : {64ll, 128ll, 576ll, 1088ll}) ok = run_shape<SYMV_SEG_SMALL>(B, n) && ok;
    for (long long n : {2112ll, 4160ll}) ok = run_shape<SYMV_SEG>(B, n) && ok;
    return ok ? 0 : 1;
}
