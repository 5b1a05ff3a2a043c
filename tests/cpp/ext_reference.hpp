// ext_reference.hpp -- plain C++ (no HIP): an extended-precision reference of the two operations the FP64 matrix-core passes
// perform (csrc/ell_kernels.hpp: k_symm_mfma / _q / _q2, k_apply_mfma, k_apply_lower, k_apply_symm_q), and the ELEMENTWISE
// comparators that hold a kernel's output to it.  Used by tests/cpp/ext_reference_main.cpp (CPU: tests/test_ext_reference_cpu.py)
// and by tests/cpp/matrix_core_reference_check.hip (GPU: tests/test_gpu_matrix_core_reference.py).
//
// Arithmetic: double-double (an unevaluated sum hi + lo, |lo| <= ulp(hi) / 2) built from the error-free transformations
// two_sum (Knuth, 6 flops, no assumption on the magnitudes) and two_prod (through std::fma).  A product of two doubles is
// EXACT in this format; dd_add is the accurate ("IEEE") addition with relative error <= 3 * 2^-106 of the exact sum of its
// operands, cancellation included; dd_mul_d has relative error <= 3 * 2^-106 as well.
//     unit roundoff of every operation below:  U_EXT = 2^-100  (<= 2^-64, which is all the bounds below need:
//     a sum of m terms carries an error of at most m U_EXT S, S = the sum of the terms' magnitudes, and m <= 2^23 here).
// Nothing here multiplies and adds in one expression outside std::fma, so the header means the same with and without
// -ffp-contract; ref_apply_two_roundings is the exception and says so: whatever compiles it keeps -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace extref {

constexpr double U_EXT = 0x1p-100;
static_assert(U_EXT <= 0x1p-64, "the reference must be at least 11 bits finer than the bounds it anchors");
static_assert(std::numeric_limits<double>::is_iec559 && std::numeric_limits<double>::digits == 53, "IEEE binary64");
constexpr double U_DBL = 0x1p-53;  // unit roundoff of the kernels' arithmetic

struct dd {
    double hi, lo;
};

inline dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
inline dd quick_two_sum(double a, double b) {  // |a| >= |b| or a == 0
    const double s = a + b;
    return {s, b - (s - a)};
}
inline dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, std::fma(a, b, -p)};
}
inline dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return quick_two_sum(s.hi, s.lo);
}
inline dd dd_add_d(dd a, double b) { return dd_add(a, dd{b, 0.0}); }
inline dd dd_add_prod(dd a, double x, double y) { return dd_add(a, two_prod(x, y)); }  // a + x y, the product exact
inline dd dd_mul_d(dd a, double b) {
    dd p = two_prod(a.hi, b);
    p.lo += a.lo * b;
    return quick_two_sum(p.hi, p.lo);
}
inline dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
inline double dd_abs(dd a) { return std::fabs(a.hi + a.lo); }
inline double dd_to_double(dd a) { return a.hi + a.lo; }

// ------------------------------------------------------------------------------------------------ the product passes ---
// The shard's partial product over its lower trapezoid, exactly as the passes define it (k_symm_mfma's header, symm_tile):
//     y_v[r] += Q[r][c] g_v[c]   for c <= r      (row sums: the diagonal counts once, here)
//     y_v[c] += Q[r][c] g_v[r]   for c <  r      (column sums: strictly below the diagonal)
// for r in [row0, row0 + nrows), and S_v[i] = the sum of |Q| |g| over the same terms.  An element with c > r is never read.
// q(r, c) yields the element of GLOBAL row r as a dd (a plain matrix, or the extended-precision result of ref_apply).
struct SymmRef {
    long long n = 0;
    int lv = 0;
    std::vector<dd> y;      // [lv][n]
    std::vector<double> S;  // [lv][n]
};

template <class QF>
inline SymmRef ref_symm_of(QF q, long long n, long long row0, long long nrows, const double* g, long long g_stride, int lv) {
    SymmRef out;
    out.n = n;
    out.lv = lv;
    out.y.assign((size_t)lv * n, dd{0.0, 0.0});
    std::vector<dd> S((size_t)lv * n, dd{0.0, 0.0});
    for (long long r = row0; r < row0 + nrows; ++r)
        for (long long c = 0; c <= r; ++c) {
            const dd x = q(r, c);
            const double ax = std::fabs(x.hi + x.lo);
            for (int v = 0; v < lv; ++v) {
                const double gc = g[v * g_stride + c], gr = g[v * g_stride + r];
                dd& yr = out.y[(size_t)v * n + r];
                yr = dd_add(yr, dd_mul_d(x, gc));
                S[(size_t)v * n + r] = dd_add_prod(S[(size_t)v * n + r], ax, std::fabs(gc));
                if (c < r) {
                    dd& yc = out.y[(size_t)v * n + c];
                    yc = dd_add(yc, dd_mul_d(x, gr));
                    S[(size_t)v * n + c] = dd_add_prod(S[(size_t)v * n + c], ax, std::fabs(gr));
                }
            }
        }
    out.S.resize(S.size());
    for (size_t i = 0; i < S.size(); ++i) out.S[i] = dd_to_double(S[i]);
    return out;
}

// Q: the shard's rows, Q[(r - row0) * ld + c] (what the kernels receive)
inline SymmRef ref_symm(const double* Q, long long ld, long long n, long long row0, long long nrows, const double* g,
                        long long g_stride, int lv) {
    return ref_symm_of([=](long long r, long long c) { return dd{Q[(r - row0) * ld + c], 0.0}; }, n, row0, nrows, g, g_stride, lv);
}

// ------------------------------------------------------------------------------------------------- the apply passes ---
// NP recorded updates on the rows [row0, row0 + nrows) of the lower triangle.  a_k = -(cpend[k] * pend[k][r]), rounded once
// in double: the coefficient of src/ell.rs:119, as the kernel headers specify it.  For every c <= r:
//     X[r][c] = x + sum_k a_k pend[k][c]   (extended precision),      M[r][c] = |x| + sum_k |a_k| |pend[k][c]|.
// X and M are [nrows][n] (local row, column); elements with c > r are left at zero and never read from Q.
struct ApplyRef {
    long long n = 0, row0 = 0, nrows = 0;
    std::vector<dd> X;
    std::vector<double> M;
    dd at(long long r, long long c) const { return X[(size_t)(r - row0) * n + c]; }
};

inline ApplyRef ref_apply(const double* Q, long long ld, const double* pend, const double* cpend, int NP, long long n,
                          long long row0, long long nrows) {
    ApplyRef out;
    out.n = n, out.row0 = row0, out.nrows = nrows;
    out.X.assign((size_t)nrows * n, dd{0.0, 0.0});
    out.M.assign((size_t)nrows * n, 0.0);
    std::vector<double> a((size_t)NP);
    for (long long r = row0; r < row0 + nrows; ++r) {
        for (int k = 0; k < NP; ++k) {
            const double t = cpend[k] * pend[(long long)k * n + r];  // (a statement of its own: rounded before the negation)
            a[k] = -t;
        }
        for (long long c = 0; c <= r; ++c) {
            const double x = Q[(r - row0) * ld + c];
            dd X = {x, 0.0}, M = {std::fabs(x), 0.0};
            for (int k = 0; k < NP; ++k) {
                const double v = pend[(long long)k * n + c];
                X = dd_add_prod(X, a[k], v);
                M = dd_add_prod(M, std::fabs(a[k]), std::fabs(v));
            }
            out.X[(size_t)(r - row0) * n + c] = X;
            out.M[(size_t)(r - row0) * n + c] = dd_to_double(M);
        }
    }
    return out;
}

// Plain double, x <- x - (cpend[k] * pend[k][r]) * pend[k][c] for k in recording order, the product rounded BEFORE the
// subtraction: the sequence k_apply_lower's header claims for itself.  Needs -ffp-contract=off (every rounding is a statement
// of its own besides, so that a contracting compiler has nothing adjacent to fuse).  Returns the shard's rows [nrows][ld]:
// a copy of Q with the elements c <= r replaced.
inline std::vector<double> ref_apply_two_roundings(const double* Q, long long ld, const double* pend, const double* cpend, int NP,
                                                   long long n, long long row0, long long nrows) {
    std::vector<double> out(Q, Q + (size_t)nrows * ld);
    for (long long r = row0; r < row0 + nrows; ++r)
        for (long long c = 0; c <= r; ++c) {
            volatile double x = Q[(r - row0) * ld + c];
            for (int k = 0; k < NP; ++k) {
                volatile double cf = cpend[k] * pend[(long long)k * n + r];
                volatile double p = cf * pend[(long long)k * n + c];
                x = x - p;
            }
            out[(size_t)(r - row0) * ld + c] = x;
        }
    return out;
}

// The chain k_apply_mfma's header claims: x <- fma(a_k, pend[k][c], x), k in recording order, one rounding per update.
inline std::vector<double> ref_apply_fused_chain(const double* Q, long long ld, const double* pend, const double* cpend, int NP,
                                                 long long n, long long row0, long long nrows) {
    std::vector<double> out(Q, Q + (size_t)nrows * ld);
    for (long long r = row0; r < row0 + nrows; ++r)
        for (long long c = 0; c <= r; ++c) {
            double x = Q[(r - row0) * ld + c];
            for (int k = 0; k < NP; ++k) {
                const double t = cpend[k] * pend[(long long)k * n + r];
                x = std::fma(-t, pend[(long long)k * n + c], x);
            }
            out[(size_t)(r - row0) * ld + c] = x;
        }
    return out;
}

// ------------------------------------------------------------------------------------------------------ comparators ---
struct Worst {
    double ratio = 0.0;    // the largest error / bound (infinity: a NaN, or an error where the bound is zero)
    long long index = -1;  // the FIRST index whose error exceeds its bound (-1: none)
};

inline void worst_take(Worst& w, double err, double bound, long long index) {
    double ratio;
    if (!(err == err)) ratio = std::numeric_limits<double>::infinity();
    else if (err == 0.0) ratio = 0.0;
    else ratio = bound > 0.0 ? err / bound : std::numeric_limits<double>::infinity();
    if (ratio > w.ratio) w.ratio = ratio;
    if (ratio > 1.0 && w.index < 0) w.index = index;
}

// Products:  |yhat[i] - y[i]| <= K 2^-53 S[i].
// Why it holds for ANY association, fused or not: write yhat as the sum of its terms, each multiplied by (1 + d)^p with
// |d| <= 2^-53 and p = the roundings on the term's path to the result (its product, if the multiply-add is not fused, and every
// addition after it); |(1 + d)^p - 1| <= p 2^-53 / (1 - p 2^-53), and the denominator (p <= 2^13 here) is covered by the slack
// in the count of p below.  K = the largest p on any path.  The count, in symm_tile / symm_tile2 / symv_reduce_block:
//   row sums:    a wave's accumulator dr[jj] takes 4 MFMAs of 4 products per 16-column block, over its share of the tile's blocks:
//                at most min(SEG, n) / 4 terms in one chain, one rounding per term at most (the product is fused into the MFMA's
//                sum; the first addition to the zero accumulator is exact)                                    <= n / 4
//                ((s0 + s1) + s2) + s3 over the waves                                                             3
//                r += rowpart[J][i] over the segments (the first to zero is exact)                                <= nsegs
//                r += (column part)                                                                               1
//   column sums: dc takes 16 MFMAs of 4 products, one chain per strip and column                                  64
//                s += colpart[I][i], a wave's strips I0 + w, I0 + w + 4, ...                                      <= nstrips / 4 + 1
//                ((c0 + c1) + c2) + c3, then the addition into r                                                  4
// A term is on ONE of the two paths: p <= max(n / 4 + nsegs + 4, nstrips / 4 + 69) <= n + nstrips + nsegs + 8 for every
// n >= 64.  (The host's own combination of the partial sums, in extended precision, adds nothing.)  The count does not ask for
// a larger K.
inline double products_K(long long n, long long nstrips, long long nsegs) { return (double)(n + nstrips + nsegs + 8); }

inline Worst cmp_products(const double* yhat, const dd* y, const double* S, long long m, double K) {
    Worst w;
    for (long long i = 0; i < m; ++i) worst_take(w, yhat[i] == yhat[i] ? dd_abs(dd_add_d(y[i], -yhat[i])) : yhat[i], K * U_DBL * S[i], i);
    return w;
}

// (yhat itself in extended precision: the host's combination of a pass' partial sums)
inline Worst cmp_products(const dd* yhat, const dd* y, const double* S, long long m, double K) {
    Worst w;
    for (long long i = 0; i < m; ++i) {
        const double h = yhat[i].hi + yhat[i].lo;
        worst_take(w, h == h ? dd_abs(dd_add(y[i], dd_neg(yhat[i]))) : h, K * U_DBL * S[i], i);
    }
    return w;
}

// Apply:  |xhat - X| <= 2 NP 2^-53 M  at every c <= r.
// The count: a fused chain x <- fma(a_k, v_k[c], x) rounds once per update -- NP roundings on the path of x and of the first
// product, fewer on the later ones; the MFMA takes four updates per instruction in its own association, still at most one
// rounding per product entering the sum.  The form that rounds the product and the difference separately (k_apply_lower, the
// reference) has two per update: 2 NP.  The rounding of a_k itself is part of the operation's definition (ref_apply uses the
// rounded coefficient), not of the error.
inline Worst cmp_apply(const double* Qhat, long long ld, const ApplyRef& ref, int NP) {
    Worst w;
    for (long long lr = 0; lr < ref.nrows; ++lr)
        for (long long c = 0; c <= ref.row0 + lr; ++c) {
            const double xh = Qhat[lr * ld + c];
            const size_t k = (size_t)lr * ref.n + c;
            worst_take(w, xh == xh ? dd_abs(dd_add_d(ref.X[k], -xh)) : xh, 2.0 * NP * U_DBL * ref.M[k], lr * ref.n + c);
        }
    return w;
}

// words that differ (bit patterns) at c <= r between two [nrows][ld] images
inline long long lower_words_differing(const double* a, const double* b, long long ld, long long row0, long long nrows) {
    long long d = 0;
    for (long long lr = 0; lr < nrows; ++lr)
        for (long long c = 0; c <= row0 + lr; ++c) d += std::memcmp(&a[lr * ld + c], &b[lr * ld + c], 8) != 0;
    return d;
}

}  // namespace extref
