// matrix_core_reference_check.hip -- GPU test (built with hipcc by tests/test_gpu_matrix_core_reference.py): every FP64 matrix-core
// pass of csrc/ell_kernels.hpp, each BY ITSELF, against the extended-precision reference of the same operation
// (tests/cpp/ext_reference.hpp), ELEMENT BY ELEMENT under the derived bounds
//     products:  |yhat[r] - y[r]| <= (n + nstrips + nsegs + 8) 2^-53 S[r],  S = sum |Q| |g| over the row's terms
//     apply:     |xhat - X|       <= 2 NP 2^-53 M,                          M = |x| + sum_k |a_k| |v_k[c]|
// where the other kernel-level checks (symm_queue_check, apply_symm_check, packed_operands_check) compare kernel with kernel.
//
// Inputs are graded so that every element sits at its own scale: Q = D S D (S random in [-0.5, 0.5), D = diag(2^e), e random in
// [-30, 30]), gradients g_v = D^-1 h_v, recorded vectors v_k = D w_k, coefficients about 0.01.  Poison is DATA: every element right
// of the diagonal, the ld - n padding columns, the gradient / recorded-vector slots a pass must not read and a guard band of 4096
// doubles before and after every buffer (inside the same allocation) hold a quiet NaN.  A correct pass never reads them into a
// result and never writes them; nothing here reads or writes outside an allocation.  Partial-sum buffers hold zeros (what the
// handle's multi_fill gives them) in the sets the pass writes and NaN in those it must leave alone: the sets v >= lv, for the
// packed layout the pairs 2 p >= lv (pk_store_colsums).
//
//   argv[1] = products:  k_symm_mfma (grid form; it has no packed form), k_symm_mfma_q, k_symm_mfma_q2 (PK false / true)
//             apply:     k_apply_mfma<24 | 48> under the apply bound, k_apply_lower<8 | 16> BIT FOR BIT against the two-rounding
//                        sequence its header claims
//             fused:     k_apply_symm_q<24 | 48, ., SEG, WIDE, PK>: Q under the apply bound, the products against ref_symm of the
//                        extended-precision updated matrix
// One JSON line per case; exit code 2 on any HIP error, 1 if a case fails.
//
// Shapes (the smallest that reach each edge; n < 512 is below what the C ABI gives these passes -- handles that small run other
// schedules -- the kernels' own contract, n % 64 == 0, still covers them):
//   n = 64 one strip, one tile, the diagonal block only | 128 the first full off-diagonal block row | 320 block counts that are
//   no multiple of the four waves | 576 a second narrow segment holding only a diagonal block | 1088 two full narrow segments
//   plus 64, k_apply_mfma's second column slab with one 64-column step | 2112 the wide segment boundary (17 gradients only)
//   row shards (n, row0, nrows) = (576, 64, 256), (576, 320, 256), (1088, 512, 576) for the product passes and k_apply_mfma;
//   (1000, 0, 1000), a ragged last strip, for the apply kernels alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/group_kernels.hpp"
#include "ext_reference.hpp"
using namespace ellhip;
using namespace extref;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static const long long GUARD = 4096;
static double poison() {
    const unsigned long long bits = 0x7FF8C0DEC0DEC0DEull;  // a quiet NaN with a payload of its own
    double d;
    memcpy(&d, &bits, 8);
    return d;
}
static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// A device buffer with its guard bands and its host images: h = what was uploaded, got = what came back.
struct Buf {
    double* d = nullptr;
    long long m = 0;
    std::vector<double> h, got;
    explicit Buf(long long m_) : m(m_), h((size_t)(m_ + 2 * GUARD), poison()) { CK(hipMalloc(&d, (size_t)(m + 2 * GUARD) * 8)); }
    Buf(const Buf&) = delete;
    ~Buf() { (void)hipFree(d); }
    double* host() { return h.data() + GUARD; }
    const double* out() const { return got.data() + GUARD; }
    double* dev() const { return d + GUARD; }
    void upload() { CK(hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice)); }
    void download() {
        got.resize(h.size());
        CK(hipMemcpy(got.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
    }
    bool guards_kept() const {
        for (long long i = 0; i < GUARD; ++i)
            if (!same_bits(got[(size_t)i], h[(size_t)i]) || !same_bits(got[(size_t)(GUARD + m + i)], h[(size_t)(GUARD + m + i)])) return false;
        return true;
    }
    long long words_changed() const {  // payload words whose bits differ from what was uploaded
        long long c = 0;
        for (long long i = 0; i < m; ++i) c += !same_bits(got[(size_t)(GUARD + i)], h[(size_t)(GUARD + i)]);
        return c;
    }
};

struct Rng {
    unsigned long long s;
    unsigned long long next() {
        unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double unit() { return (double)(next() >> 11) / 9007199254740992.0; }  // [0, 1)
};

// ---- inputs and references, one set per n (shared by the cases) ------------------------------------------------------------
struct Inputs {
    long long n, ld;
    std::vector<int> e;
    std::vector<double> Q;      // [n][ld]: lower triangle D S D, NaN right of the diagonal and in the padding
    std::vector<double> g;      // [32][n]
    std::vector<double> pend;   // [MAXPEND][n]
    std::vector<double> cpend;  // [MAXPEND]
};
static const Inputs& inputs(long long n) {
    static std::map<long long, Inputs> cache;
    auto it = cache.find(n);
    if (it != cache.end()) return it->second;
    Inputs& in = cache[n];
    in.n = n, in.ld = n + 16;
    Rng rng{0x5EEDull + (unsigned long long)n};
    in.e.resize((size_t)n);
    for (auto& e : in.e) e = (int)(rng.next() % 61) - 30;
    in.Q.assign((size_t)n * in.ld, poison());
    for (long long r = 0; r < n; ++r)
        for (long long c = 0; c <= r; ++c) in.Q[(size_t)(r * in.ld + c)] = std::ldexp(rng.unit() - 0.5, in.e[(size_t)r] + in.e[(size_t)c]);
    in.g.resize((size_t)32 * n);
    for (int v = 0; v < 32; ++v)
        for (long long c = 0; c < n; ++c) in.g[(size_t)(v * n + c)] = std::ldexp(rng.unit() - 0.5, -in.e[(size_t)c]);
    in.pend.resize((size_t)MAXPEND * n);
    for (int k = 0; k < MAXPEND; ++k)
        for (long long c = 0; c < n; ++c) in.pend[(size_t)(k * n + c)] = std::ldexp(rng.unit() - 0.5, in.e[(size_t)c]);
    in.cpend.resize(MAXPEND);
    for (auto& c : in.cpend) c = 0.01 * (0.5 + rng.unit());
    return in;
}
static int max_lv(long long n) { return n >= 2112 ? 17 : 32; }  // (bounds the host time of the largest shape)

static const SymmRef& symm_ref(long long n, long long row0, long long nrows) {
    static std::map<std::tuple<long long, long long, long long>, SymmRef> cache;
    const auto key = std::make_tuple(n, row0, nrows);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const Inputs& in = inputs(n);
    return cache[key] = ref_symm(in.Q.data() + row0 * in.ld, in.ld, n, row0, nrows, in.g.data(), n, max_lv(n));
}
struct ApplyRefs {
    ApplyRef ext;
    std::vector<double> two, fused;
};
static const ApplyRefs& apply_ref(long long n, long long row0, long long nrows, int np) {
    static std::map<std::tuple<long long, long long, long long, int>, ApplyRefs> cache;
    const auto key = std::make_tuple(n, row0, nrows, np);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const Inputs& in = inputs(n);
    ApplyRefs& r = cache[key];
    const double* Q = in.Q.data() + row0 * in.ld;
    r.ext = ref_apply(Q, in.ld, in.pend.data(), in.cpend.data(), np, n, row0, nrows);
    r.two = ref_apply_two_roundings(Q, in.ld, in.pend.data(), in.cpend.data(), np, n, row0, nrows);
    r.fused = ref_apply_fused_chain(Q, in.ld, in.pend.data(), in.cpend.data(), np, n, row0, nrows);
    return r;
}
static const SymmRef& fused_symm_ref(long long n, int np) {  // the products of the extended-precision UPDATED matrix
    static std::map<std::pair<long long, int>, SymmRef> cache;
    const auto key = std::make_pair(n, np);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const ApplyRef& a = apply_ref(n, 0, n, np).ext;
    return cache[key] = ref_symm_of([&](long long r, long long c) { return a.at(r, c); }, n, 0, n, inputs(n).g.data(), n, max_lv(n));
}

// ---- the pieces the product and fused cases share --------------------------------------------------------------------------
struct Geometry {
    long long n, ld, row0, nrows, seg, nstrips, nsegs, rs, cs, nb;
    std::vector<SymmTile> tiles;  // the host table, largest first, as the handle builds it
};
static Geometry geometry(long long n, long long row0, long long nrows, long long seg) {
    Geometry G;
    G.n = n, G.ld = n + 16, G.row0 = row0, G.nrows = nrows, G.seg = seg;
    G.nstrips = nrows / SYMV_H, G.nsegs = (n + seg - 1) / seg, G.rs = G.nsegs * n, G.cs = G.nstrips * n, G.nb = (n + 127) / 128;
    for (long long I = G.nstrips - 1; I >= 0; --I)
        for (long long J = 0; J < G.nsegs; ++J)
            if (J * seg <= row0 + I * SYMV_H + SYMV_H - 1) G.tiles.push_back({(int)I, (int)J});
    auto blocks_of = [&](const SymmTile& t) {
        const long long r0 = row0 + (long long)t.I * SYMV_H, c0 = (long long)t.J * seg;
        return (std::min<long long>(c0 + seg, r0 + SYMV_H) - c0) / 16;
    };
    std::stable_sort(G.tiles.begin(), G.tiles.end(), [&](const SymmTile& a, const SymmTile& b) { return blocks_of(a) > blocks_of(b); });
    return G;
}

// The buffers of a product pass: gradients (the slots v >= lv poisoned), the packed / transposed operands, the partial sums, Y.
struct ProductBufs {
    Buf g, gT, rp, cp, Y, gpart, st;
    SymmTile* d_tiles = nullptr;
    unsigned* d_queue = nullptr;
    const Geometry& G;
    int lv;
    bool pk;
    static long long cp_index(bool pk, long long cs, int v, long long k) { return pk ? 2 * ((long long)(v >> 1) * cs + k) + (v & 1) : (long long)v * cs + k; }
    ProductBufs(const Geometry& G_, int lv_, bool pk_, bool halted)
        : g(32 * G_.n), gT(32 * G_.n), rp(32 * G_.rs), cp(32 * G_.cs), Y(32 * G_.n), gpart(32 * G_.nb * 25),
          st((long long)(sizeof(DevState) / 8)), G(G_), lv(lv_), pk(pk_) {
        const Inputs& in = inputs(G.n);
        std::copy(in.g.begin(), in.g.begin() + (size_t)lv * G.n, g.host());
        for (int v = 0; v < lv; ++v) std::fill(rp.host() + (long long)v * G.rs, rp.host() + (long long)(v + 1) * G.rs, 0.0);
        const int cv = pk ? 2 * ((lv + 1) / 2) : lv;  // the packed form writes whole pairs
        for (int v = 0; v < cv; ++v)
            for (long long k = 0; k < G.cs; ++k) cp.host()[cp_index(pk, G.cs, v, k)] = 0.0;
        DevState hs;
        memset(&hs, 0, sizeof(hs));
        hs.halted = halted ? 1 : 0;
        memcpy(st.host(), &hs, sizeof(hs));
        for (Buf* b : {&g, &gT, &rp, &cp, &Y, &gpart, &st}) b->upload();
        CK(hipMalloc(&d_tiles, G.tiles.size() * sizeof(SymmTile)));
        CK(hipMalloc(&d_queue, 256));
        CK(hipMemcpy(d_tiles, G.tiles.data(), G.tiles.size() * sizeof(SymmTile), hipMemcpyHostToDevice));
        CK(hipMemset(d_queue, 0, 256));
    }
    ~ProductBufs() {
        (void)hipFree(d_tiles);
        (void)hipFree(d_queue);
    }
    const DevState* dst() const { return (const DevState*)st.dev(); }
    // the operands as the pass wants them (this also rewinds the tile queue); pend / pendP / ks2: the fused pass' packed vectors
    void pack(bool wide, const double* pend = nullptr, double* pendP = nullptr, int ks2 = 0) {
        const int nvt = wide ? 2 : 1;
        if (pk)
            hipLaunchKernelGGL(k_pack_operands, dim3((unsigned)(G.n * nvt / 32 + G.n * ks2 / 64)), dim3(256), 0, 0, (const double*)g.dev(), G.n, lv,
                               G.n, gT.dev(), d_queue, nvt, pend, pendP, ks2);
        else
            hipLaunchKernelGGL(k_pack_grads, dim3((unsigned)((G.n * 16 * nvt + 255) / 256)), dim3(256), 0, 0, (const double*)g.dev(), G.n, lv, G.n,
                               gT.dev(), d_queue, 16 * nvt);
        CK(hipGetLastError());
    }
    // the project's own reduction of the partial sums (the packed one forms dot products: unsharded handles only)
    bool reduce() {
        if (pk && (G.row0 != 0 || G.nrows != G.n)) return false;
        if (pk)
            hipLaunchKernelGGL(k_group_reduce_p<24>, dim3((unsigned)G.nb, (unsigned)(lv + 1) / 2), dim3(256), 0, 0, G.n, G.row0, G.nrows, G.seg,
                               (const double*)rp.dev(), (const double*)cp.dev(), G.rs, G.cs, Y.dev(), (const double*)g.dev(), G.n,
                               (const double*)g.dev(), gpart.dev(), dst(), lv, 0);
        else
            hipLaunchKernelGGL(k_group_reduce<0>, dim3((unsigned)G.nb, (unsigned)lv), dim3(256), 0, 0, G.n, G.row0, G.nrows, G.seg,
                               (const double*)rp.dev(), (const double*)cp.dev(), G.rs, G.cs, Y.dev(), (const double*)g.dev(), G.n,
                               (const double*)g.dev(), gpart.dev(), dst(), 0);
        CK(hipGetLastError());
        return true;
    }
    struct Verdict {
        double ratio_partials = 0.0, ratio_y = -1.0;
        long long first_bad = -1, stray = 0;
        bool untouched = true, guards = true;
        unsigned drawn = 0;
    };
    // after the launches: the partial sums over exactly the host table's tiles against ref, Y against ref, and everything else
    Verdict judge(const SymmRef& ref, bool reduced, bool halted) {
        CK(hipDeviceSynchronize());
        Verdict V;
        for (Buf* b : {&g, &gT, &rp, &cp, &Y, &gpart, &st}) {
            b->download();
            V.guards = V.guards && b->guards_kept();
        }
        CK(hipMemcpy(&V.drawn, d_queue, 4, hipMemcpyDeviceToHost));
        V.untouched = g.words_changed() == 0 && st.words_changed() == 0;
        const double K = products_K(G.n, G.nstrips, G.nsegs);
        if (halted) {  // nothing is written
            V.untouched = V.untouched && rp.words_changed() == 0 && cp.words_changed() == 0 && Y.words_changed() == 0;
            return V;
        }
        std::vector<dd> y((size_t)lv * G.n, dd{0.0, 0.0});
        std::vector<char> rmark((size_t)rp.m, 0), cmark((size_t)cp.m, 0);
        const int cv = pk ? 2 * ((lv + 1) / 2) : lv;
        for (const SymmTile& t : G.tiles) {
            const long long r0 = G.row0 + (long long)t.I * SYMV_H, c0 = (long long)t.J * G.seg;
            const long long cend = std::min<long long>(c0 + G.seg, r0 + SYMV_H);
            for (int v = 0; v < cv; ++v) {
                for (long long c = c0; c < cend; ++c) {
                    const long long k = cp_index(pk, G.cs, v, (long long)t.I * G.n + c);
                    cmark[(size_t)k] = 1;
                    if (v < lv) y[(size_t)(v * G.n + c)] = dd_add_d(y[(size_t)(v * G.n + c)], cp.out()[k]);
                }
                if (v >= lv) continue;
                for (long long r = r0; r < r0 + SYMV_H; ++r) {
                    const long long k = (long long)v * G.rs + (long long)t.J * G.n + r;
                    rmark[(size_t)k] = 1;
                    y[(size_t)(v * G.n + r)] = dd_add_d(y[(size_t)(v * G.n + r)], rp.out()[k]);
                }
            }
        }
        // outside the tiles' footprint, and in the sets the pass must not write, every word keeps its bits
        for (long long k = 0; k < rp.m; ++k) V.stray += !rmark[(size_t)k] && !same_bits(rp.out()[k], rp.host()[k]);
        for (long long k = 0; k < cp.m; ++k) V.stray += !cmark[(size_t)k] && !same_bits(cp.out()[k], cp.host()[k]);
        const Worst wp = cmp_products(y.data(), ref.y.data(), ref.S.data(), (long long)lv * G.n, K);
        V.ratio_partials = wp.ratio, V.first_bad = wp.index;
        if (reduced) {
            const Worst wy = cmp_products(Y.out(), ref.y.data(), ref.S.data(), (long long)lv * G.n, K);
            V.ratio_y = wy.ratio;
            if (V.first_bad < 0) V.first_bad = wy.index;
            for (long long k = (long long)lv * G.n; k < Y.m; ++k) V.stray += !same_bits(Y.out()[k], Y.host()[k]);
        } else {
            V.untouched = V.untouched && Y.words_changed() == 0;
        }
        return V;
    }
};

static void print_ratio(const char* key, double r) {
    if (std::isinf(r)) printf("\"%s\": Infinity, ", key);
    else printf("\"%s\": %.6g, ", key, r);
}
static const char* tf(bool b) { return b ? "true" : "false"; }

// ---- product passes ---------------------------------------------------------------------------------------------------------
enum Kind { GRID, QUEUE, QUEUE2 };
static const char* kind_name(Kind k) { return k == GRID ? "k_symm_mfma" : k == QUEUE ? "k_symm_mfma_q" : "k_symm_mfma_q2"; }

template <int SEG>
static bool product_case(Kind kind, bool pk, long long n, long long row0, long long nrows, int lv, bool halted) {
    const Geometry G = geometry(n, row0, nrows, SEG);
    const Inputs& in = inputs(n);
    Buf Q(nrows * G.ld);
    std::copy(in.Q.begin() + (size_t)(row0 * G.ld), in.Q.begin() + (size_t)((row0 + nrows) * G.ld), Q.host());
    Q.upload();
    ProductBufs B(G, lv, pk, halted);
    B.pack(kind == QUEUE2);
    const int ntiles = (int)G.tiles.size(), wgs = std::min(ntiles, 64);
#define SYMM_ARGS (const double*)Q.dev(), G.ld, n, row0, (const double*)B.gT.dev(), lv, B.rp.dev(), B.cp.dev(), G.rs, G.cs, B.dst(), \
                  (const SymmTile*)B.d_tiles, ntiles, B.d_queue
    if (kind == GRID)
        hipLaunchKernelGGL((k_symm_mfma<true, SEG>), dim3((unsigned)G.nstrips, (unsigned)G.nsegs), dim3(256), 0, 0, (const double*)Q.dev(), G.ld, n,
                           row0, nrows, (const double*)B.gT.dev(), lv, B.rp.dev(), B.cp.dev(), G.rs, G.cs, B.dst());
    else if (kind == QUEUE && !pk) hipLaunchKernelGGL((k_symm_mfma_q<true, SEG, false>), dim3((unsigned)wgs), dim3(256), 0, 0, SYMM_ARGS);
    else if (kind == QUEUE) hipLaunchKernelGGL((k_symm_mfma_q<true, SEG, true>), dim3((unsigned)wgs), dim3(256), 0, 0, SYMM_ARGS);
    else if (!pk) hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG, false>), dim3((unsigned)wgs), dim3(256), 0, 0, SYMM_ARGS);
    else hipLaunchKernelGGL((k_symm_mfma_q2<true, SEG, true>), dim3((unsigned)wgs), dim3(256), 0, 0, SYMM_ARGS);
#undef SYMM_ARGS
    CK(hipGetLastError());
    const bool reduced = B.reduce();
    const ProductBufs::Verdict V = B.judge(symm_ref(n, row0, nrows), reduced, halted);
    Q.download();
    const bool q_kept = Q.words_changed() == 0, guards = V.guards && Q.guards_kept();
    const bool drawn_ok = kind == GRID || halted || V.drawn >= (unsigned)ntiles;
    const bool ok = V.ratio_partials <= 1.0 && V.ratio_y <= 1.0 && V.stray == 0 && V.untouched && q_kept && guards && drawn_ok;
    printf("{\"group\": \"products\", \"kernel\": \"%s\", \"pk\": %s, \"n\": %lld, \"seg\": %d, \"lv\": %d, \"row0\": %lld, \"nrows\": %lld, "
           "\"halted\": %s, \"tiles\": %d, ",
           kind_name(kind), tf(pk), n, SEG, lv, row0, nrows, tf(halted), ntiles);
    print_ratio("ratio_partials", V.ratio_partials);
    print_ratio("ratio_y", V.ratio_y);
    printf("\"reduced\": %s, \"first_bad\": %lld, \"stray_words\": %lld, \"untouched_kept\": %s, \"q_kept\": %s, \"guards_kept\": %s, "
           "\"queue_ok\": %s}\n",
           tf(reduced), V.first_bad, V.stray, tf(V.untouched), tf(q_kept), tf(guards), tf(drawn_ok));
    fflush(stdout);
    return ok;
}

static bool product_shape(long long n, int seg, long long row0, long long nrows) {
    bool ok = true;
    auto run = [&](Kind k, bool pk, int lv, bool halted) {
        return seg == SYMV_SEG_SMALL ? product_case<SYMV_SEG_SMALL>(k, pk, n, row0, nrows, lv, halted)
                                     : product_case<SYMV_SEG>(k, pk, n, row0, nrows, lv, halted);
    };
    if (n >= 2112) {
        for (bool pk : {false, true}) ok = run(QUEUE2, pk, 17, false) && ok;
        return ok;
    }
    for (int lv : {1, 2, 15, 16}) {
        ok = run(GRID, false, lv, false) && ok;
        for (bool pk : {false, true}) ok = run(QUEUE, pk, lv, false) && ok;
    }
    for (int lv : {17, 31, 32})
        for (bool pk : {false, true}) ok = run(QUEUE2, pk, lv, false) && ok;
    return ok;
}

static bool products_group() {
    bool ok = true;
    ok = product_shape(64, 512, 0, 64) && ok;
    ok = product_shape(128, 512, 0, 128) && ok;
    ok = product_shape(320, 512, 0, 320) && ok;
    ok = product_shape(320, 2048, 0, 320) && ok;
    ok = product_shape(576, 512, 0, 576) && ok;
    ok = product_shape(1088, 512, 0, 1088) && ok;
    ok = product_shape(1088, 2048, 0, 1088) && ok;
    ok = product_shape(576, 512, 64, 256) && ok;
    ok = product_shape(576, 512, 320, 256) && ok;
    ok = product_shape(1088, 512, 512, 576) && ok;
    ok = product_shape(2112, 2048, 0, 2112) && ok;
    // a halted queue: nothing is written
    ok = product_case<SYMV_SEG_SMALL>(GRID, false, 320, 0, 320, 16, true) && ok;
    for (bool pk : {false, true}) {
        ok = product_case<SYMV_SEG_SMALL>(QUEUE, pk, 320, 0, 320, 15, true) && ok;
        ok = product_case<SYMV_SEG_SMALL>(QUEUE2, pk, 320, 0, 320, 31, true) && ok;
    }
    return ok;
}

// ---- apply passes -----------------------------------------------------------------------------------------------------------
// elements at or right of the end of the row's strip (TR rows: 64 for k_apply_mfma, 16 for k_apply_lower), padding included,
// that changed their bits
static long long right_of_strip_changed(const Buf& Q, long long ld, long long n, long long row0, long long nrows, long long TR) {
    long long changed = 0;
    for (long long lr = 0; lr < nrows; ++lr) {
        const long long last = std::min((lr / TR + 1) * TR, nrows) - 1 + row0;
        const long long cend = std::min((last / 2 + 1) * 2, n);
        for (long long c = cend; c < ld; ++c) changed += !same_bits(Q.out()[lr * ld + c], Q.h[(size_t)(GUARD + lr * ld + c)]);
    }
    return changed;
}

// the recorded vectors and coefficients of a pass of rank np: the slots k >= np poisoned
static void fill_pending(Buf& pend, Buf& cpend, const Inputs& in, int np) {
    std::copy(in.pend.begin(), in.pend.begin() + (size_t)np * in.n, pend.host());
    std::copy(in.cpend.begin(), in.cpend.begin() + np, cpend.host());
    pend.upload();
    cpend.upload();
}

template <int NP, bool MFMA>
static bool apply_case(long long n, long long row0, long long nrows) {
    const Inputs& in = inputs(n);
    const long long ld = in.ld;
    Buf Q(nrows * ld), pend((long long)MAXPEND * n), cpend(MAXPEND), st((long long)(sizeof(DevState) / 8));
    std::copy(in.Q.begin() + (size_t)(row0 * ld), in.Q.begin() + (size_t)((row0 + nrows) * ld), Q.host());
    Q.upload();
    fill_pending(pend, cpend, in, NP);
    memset(st.host(), 0, sizeof(DevState));
    st.upload();
    if constexpr (MFMA) {
        const dim3 g2((unsigned)((nrows + APM_ROWS - 1) / APM_ROWS), (unsigned)((n + APM_COLS - 1) / APM_COLS));
        hipLaunchKernelGGL((k_apply_mfma<NP, true>), g2, dim3(256), 0, 0, Q.dev(), ld, n, nrows, row0, (const double*)pend.dev(),
                           (const double*)cpend.dev(), (const DevState*)st.dev());
    } else {
        hipLaunchKernelGGL((k_apply_lower<NP, true>), dim3((unsigned)((nrows + APL_TR - 1) / APL_TR)), dim3(256), 0, 0, Q.dev(), ld, n, nrows, row0,
                           (const double*)pend.dev(), (const double*)cpend.dev(), (const DevState*)st.dev());
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    bool guards = true;
    for (Buf* b : {&Q, &pend, &cpend, &st}) {
        b->download();
        guards = guards && b->guards_kept();
    }
    const ApplyRefs& R = apply_ref(n, row0, nrows, NP);
    const Worst w = cmp_apply(Q.out(), ld, R.ext, NP);
    const long long vs_two = lower_words_differing(Q.out(), R.two.data(), ld, row0, nrows);
    const long long vs_fused = lower_words_differing(Q.out(), R.fused.data(), ld, row0, nrows);
    const long long right = right_of_strip_changed(Q, ld, n, row0, nrows, MFMA ? APM_ROWS : APL_TR);
    const bool inputs_kept = pend.words_changed() == 0 && cpend.words_changed() == 0 && st.words_changed() == 0;
    long long lower = 0;
    for (long long lr = 0; lr < nrows; ++lr) lower += row0 + lr + 1;
    const bool ok = w.ratio <= 1.0 && (MFMA || vs_two == 0) && right == 0 && inputs_kept && guards;
    printf("{\"group\": \"apply\", \"kernel\": \"%s\", \"np\": %d, \"n\": %lld, \"row0\": %lld, \"nrows\": %lld, ", MFMA ? "k_apply_mfma" : "k_apply_lower",
           NP, n, row0, nrows);
    print_ratio("ratio_q", w.ratio);
    printf("\"first_bad\": %lld, \"lower_elements\": %lld, \"differ_from_two_roundings\": %lld, \"differ_from_fused_chain\": %lld, "
           "\"right_of_strip_changed\": %lld, \"inputs_kept\": %s, \"guards_kept\": %s}\n",
           w.index, lower, vs_two, vs_fused, right, tf(inputs_kept), tf(guards));
    fflush(stdout);
    return ok;
}

static bool apply_group() {
    bool ok = true;
    for (long long n : {64ll, 128ll, 320ll, 576ll, 1088ll, 2112ll, 1000ll}) {  // (1000: a ragged last strip of 40 rows, last tile of 8)
        ok = apply_case<24, true>(n, 0, n) && ok;
        ok = apply_case<48, true>(n, 0, n) && ok;
        ok = apply_case<8, false>(n, 0, n) && ok;
        ok = apply_case<16, false>(n, 0, n) && ok;
    }
    const long long shards[3][3] = {{576, 64, 256}, {576, 320, 256}, {1088, 512, 576}};
    for (const auto& s : shards) {
        ok = apply_case<24, true>(s[0], s[1], s[2]) && ok;
        ok = apply_case<48, true>(s[0], s[1], s[2]) && ok;
    }
    return ok;
}

// ---- the fused pass ----------------------------------------------------------------------------------------------------------
template <int NP, int SEG>
static bool fused_case(bool pk, long long n, int lv, bool halted) {
    const Geometry G = geometry(n, 0, n, SEG);
    const Inputs& in = inputs(n);
    const bool wide = lv > 16;
    Buf Q(n * G.ld), pend((long long)MAXPEND * n), cpend(MAXPEND), pendP((long long)MAXPEND * n);
    std::copy(in.Q.begin(), in.Q.end(), Q.host());
    Q.upload();
    pendP.upload();
    fill_pending(pend, cpend, in, NP);
    ProductBufs B(G, lv, pk, halted);
    B.pack(wide, (const double*)pend.dev(), pendP.dev(), pk ? NP / 8 : 0);
    const int ntiles = (int)G.tiles.size(), wgs = std::min(ntiles, 64);
#define FUSED_ARGS Q.dev(), G.ld, n, (const double*)pend.dev(), (const double*)cpend.dev(), (const double*)B.gT.dev(), lv, B.rp.dev(), B.cp.dev(), \
                   G.rs, G.cs, B.dst(), (const SymmTile*)B.d_tiles, ntiles, B.d_queue, (const double*)pendP.dev()
    if (!wide && !pk) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false, false>), dim3((unsigned)wgs), dim3(256), 0, 0, FUSED_ARGS);
    else if (!wide) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, false, true>), dim3((unsigned)wgs), dim3(256), 0, 0, FUSED_ARGS);
    else if (!pk) hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true, false>), dim3((unsigned)wgs), dim3(256), 0, 0, FUSED_ARGS);
    else hipLaunchKernelGGL((k_apply_symm_q<NP, true, SEG, true, true>), dim3((unsigned)wgs), dim3(256), 0, 0, FUSED_ARGS);
#undef FUSED_ARGS
    CK(hipGetLastError());
    const bool reduced = B.reduce();
    const ProductBufs::Verdict V = B.judge(fused_symm_ref(n, NP), reduced, halted);
    bool guards = V.guards;
    for (Buf* b : {&Q, &pend, &cpend, &pendP}) {
        b->download();
        guards = guards && b->guards_kept();
    }
    const Worst w = cmp_apply(Q.out(), G.ld, apply_ref(n, 0, n, NP).ext, NP);
    const long long right = right_of_strip_changed(Q, G.ld, n, 0, n, SYMV_H);
    const bool inputs_kept = pend.words_changed() == 0 && cpend.words_changed() == 0;
    const bool drawn_ok = V.drawn >= (unsigned)ntiles;  // (the update is owed whether or not the queue has halted)
    const bool ok = w.ratio <= 1.0 && V.ratio_partials <= 1.0 && V.ratio_y <= 1.0 && V.stray == 0 && V.untouched && right == 0 && inputs_kept &&
                    guards && drawn_ok;
    printf("{\"group\": \"fused\", \"kernel\": \"k_apply_symm_q\", \"np\": %d, \"pk\": %s, \"n\": %lld, \"seg\": %d, \"lv\": %d, \"row0\": 0, "
           "\"nrows\": %lld, \"halted\": %s, \"tiles\": %d, ",
           NP, tf(pk), n, SEG, lv, n, tf(halted), ntiles);
    print_ratio("ratio_q", w.ratio);
    print_ratio("ratio_partials", V.ratio_partials);
    print_ratio("ratio_y", V.ratio_y);
    printf("\"reduced\": %s, \"first_bad\": %lld, \"stray_words\": %lld, \"untouched_kept\": %s, \"right_of_strip_changed\": %lld, "
           "\"inputs_kept\": %s, \"guards_kept\": %s, \"queue_ok\": %s}\n",
           tf(reduced), w.index >= 0 ? w.index : V.first_bad, V.stray, tf(V.untouched), right, tf(inputs_kept), tf(guards), tf(drawn_ok));
    fflush(stdout);
    return ok;
}

template <int SEG>
static bool fused_shape(long long n) {
    bool ok = true;
    const int lvs[7] = {1, 2, 15, 16, 17, 31, 32};
    for (int i = 0; i < 7; ++i)
        for (int p = 0; p < 2; ++p) {  // ranks 24 and 48 alternate over (lv, PK): each meets both widths and both layouts
            if ((i + p + (SEG == SYMV_SEG)) & 1) ok = fused_case<48, SEG>(p == 1, n, lvs[i], false) && ok;
            else ok = fused_case<24, SEG>(p == 1, n, lvs[i], false) && ok;
        }
    return ok;
}

static bool fused_group() {
    bool ok = true;
    ok = fused_shape<SYMV_SEG_SMALL>(64) && ok;
    ok = fused_shape<SYMV_SEG_SMALL>(128) && ok;
    ok = fused_shape<SYMV_SEG_SMALL>(320) && ok;
    ok = fused_shape<SYMV_SEG>(320) && ok;
    ok = fused_shape<SYMV_SEG_SMALL>(576) && ok;
    ok = fused_shape<SYMV_SEG_SMALL>(1088) && ok;
    ok = fused_shape<SYMV_SEG>(1088) && ok;
    ok = fused_case<48, SYMV_SEG>(false, 2112, 17, false) && ok;
    ok = fused_case<24, SYMV_SEG>(true, 2112, 17, false) && ok;
    // a halted queue: the update lands, no product is written
    ok = fused_case<48, SYMV_SEG_SMALL>(false, 320, 16, true) && ok;
    ok = fused_case<24, SYMV_SEG_SMALL>(true, 320, 31, true) && ok;
    return ok;
}

int main(int argc, char** argv) {
    const std::string group = argc > 1 ? argv[1] : "";
    bool ok;
    if (group == "products") ok = products_group();
    else if (group == "apply") ok = apply_group();
    else if (group == "fused") ok = fused_group();
    else return 2;
    return ok ? 0 : 1;
}
