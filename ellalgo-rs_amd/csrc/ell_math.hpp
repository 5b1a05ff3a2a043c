// ell_math.hpp -- exp and log of the device-resident oracles, the same roundings on the host and on the device
// (DESIGN section 9.13).
//
// The device library's exp / log and glibc's do not agree in the last bit, so an oracle that takes one on the device and
// the other in its CPU restatement is not bit-identical to it.  ell_exp and ell_log are written with + - * /, comparisons,
// one double -> int conversion and integer operations on the representation, and nothing else: no fma, no library call, no
// table.  Every one of those is correctly rounded on both sides, so compiled with -ffp-contract=off the host and the device
// run the same sequence of roundings and return the same bits.  Plain g++ can include this header (tests/cpp/ell_math_host.cpp;
// tests/batch_profit_reference.py restates it operation by operation).
//
// ell_exp   k = x / ln 2 rounded to nearest (ties away), r = (x - k ln2_hi) - k ln2_lo with k ln2_hi exact (ln2_hi has 21
//           trailing zero bits, |k| <= 1077), e = the rounding error of that last subtraction; exp(r) = 1 + r + q with q the
//           Taylor terms r^2/2! .. r^15/15! (|r| <= 0.3466: the first term left out is below 2^-64); 1 + r is split into its
//           rounded sum t and its exact error, so the result t + (err + (q + e)) has one rounding of size half an ulp and the
//           rest is small.  2^k goes into the exponent field; a result below 2^-1022 is scaled in two steps, the second a
//           multiplication by 2^-1000 that rounds once into the subnormals, a k of 1024 in two steps the second of which
//           overflows to +inf where libm does.
// ell_log   x = 2^k m with m in [sqrt(2)/2, sqrt(2)) read off the representation (a subnormal x is multiplied by 2^54
//           first), f = m - 1 exact, s = f / (2 + f), z = s^2, R = z (2/3 + z (2/5 + .. + z 2/25)): log(1 + f) = 2 s + s R.
//           The sum is taken in the order fdlibm documents for this series, with hfsq = f^2 / 2:
//               k ln2_hi - ((hfsq - (s (hfsq + R) + k ln2_lo)) - f)
//           so that the rounding error of s meets a factor of the order f^2, not f.
// Special values as libm has them: exp(NaN) = NaN, exp(+inf) = +inf, exp(-inf) = +0, overflow to +inf, gradual underflow to
// +0; log(NaN) = NaN, log(+-0) = -inf, log(x < 0) = NaN, log(+inf) = +inf.
// Measured against mpmath (tests/test_batch_profit_cpu.py): see DESIGN section 9.13.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ELL_MATH_HD __host__ __device__
#else
#define ELL_MATH_HD
#endif

namespace ellhip {

ELL_MATH_HD inline uint64_t ell_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
ELL_MATH_HD inline double ell_from_bits(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

constexpr uint64_t ELL_BITS_INF = 0x7ff0000000000000ULL;
constexpr uint64_t ELL_BITS_NAN = 0x7ff8000000000000ULL;
constexpr double ELL_LN2_HI = 6.93147180369123816490e-01;  // 0x3fe62e42fee00000
constexpr double ELL_LN2_LO = 1.90821492927058770002e-10;  // 0x3dea39ef35793c76
constexpr double ELL_INV_LN2 = 1.44269504088896338700e+00; // 0x3ff71547652b82fe

ELL_MATH_HD inline double ell_exp(double x) {
    if (x != x) return x + x;
    if (x > 710.0) return ell_from_bits(ELL_BITS_INF);
    if (x < -746.0) return 0.0;
    const double kf = x * ELL_INV_LN2;
    const int k = (int)(x < 0.0 ? kf - 0.5 : kf + 0.5);
    const double kd = (double)k;
    const double hi = x - kd * ELL_LN2_HI;
    const double lo = kd * ELL_LN2_LO;
    const double r = hi - lo;
    const double e = (hi - r) - lo;
    double p = 1.0 / 1307674368000.0;  // 1 / 15!
    p = p * r + 1.0 / 87178291200.0;
    p = p * r + 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    const double q = (r * r) * p;
    const double t = 1.0 + r;
    const double terr = (1.0 - t) + r;
    const double y = t + (terr + (q + e));  // in (0.70, 1.42)
    if (k > 1023) return ell_from_bits(ell_bits(y) + ((uint64_t)(k - 1) << 52)) * 2.0;
    if (k < -1021) return ell_from_bits(ell_bits(y) + ((uint64_t)(int64_t)(k + 1000) << 52)) * ell_from_bits(0x0170000000000000ULL);
    return ell_from_bits(ell_bits(y) + ((uint64_t)(int64_t)k << 52));
}

ELL_MATH_HD inline double ell_log(double x) {
    if (x != x) return x + x;
    uint64_t u = ell_bits(x);
    if ((u << 1) == 0) return ell_from_bits(0xfff0000000000000ULL);  // log(+-0) = -inf
    if ((u >> 63) != 0) return ell_from_bits(ELL_BITS_NAN);
    if (u == ELL_BITS_INF) return x;
    int k = 0;
    if ((u >> 52) == 0) {  // subnormal
        u = ell_bits(x * 18014398509481984.0);  // 2^54
        k = -54;
    }
    k += (int)(u >> 52) - 1023;
    uint64_t mant = u & 0x000fffffffffffffULL;
    if (mant >= 0x0006a09e667f3bcdULL) {  // m >= sqrt(2): halve it
        mant |= 0x3fe0000000000000ULL;
        k += 1;
    } else {
        mant |= 0x3ff0000000000000ULL;
    }
    const double f = ell_from_bits(mant) - 1.0;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double R = 2.0 / 25.0;
    R = R * z + 2.0 / 23.0;
    R = R * z + 2.0 / 21.0;
    R = R * z + 2.0 / 19.0;
    R = R * z + 2.0 / 17.0;
    R = R * z + 2.0 / 15.0;
    R = R * z + 2.0 / 13.0;
    R = R * z + 2.0 / 11.0;
    R = R * z + 2.0 / 9.0;
    R = R * z + 2.0 / 7.0;
    R = R * z + 2.0 / 5.0;
    R = R * z + 2.0 / 3.0;
    R = R * z;
    const double hfsq = (0.5 * f) * f;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return dk * ELL_LN2_HI - ((hfsq - (s * (hfsq + R) + dk * ELL_LN2_LO)) - f);
}

}  // namespace ellhip
