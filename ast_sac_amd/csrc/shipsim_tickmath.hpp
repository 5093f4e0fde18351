// shipsim_tickmath.hpp — the three device-library functions on the headline stream tick's steady path (sincos of the
// heading, the LOS course correction's atan, the reward's exp), restated operation for operation from the device
// library of ROCm 7.2.0 (ocml: sincos / trigredsmall / sincosred2, atan / atanred, exp for f64): the same products,
// sums, explicit fmas, rint, ldexp and selects in the same order, so with contraction off the results are the
// library's bits. Plain C++17 with no HIP include, in the manner of shipsim_sbmpc_nominal.hpp: shipsim_device.hpp
// includes it for the kernels, tests/tickmath_host_check.cpp compiles it with the host compiler.
//
// Every fp64 constant the three functions use is an entry of one table (kTm); a function reads its constants through
// a provider K (`K.template k<I>()`), so the form with literal constants (TmLiteral) and the kernels' form, which
// holds the table in registers and delivers an entry by a row broadcast (shipsim_device.hpp: TmRow), read the same
// bits. tm_sincos is the library's |x| < 2^30 path alone: outside tm_sincos_small_ok(x) (larger, or not finite) the
// caller uses the library's sincos.
#pragma once
#include <math.h>
#include <stdint.h>

#include "shipsim_types.hpp"  // SHIPSIM_HD

namespace shipsim {
namespace tickmath {

constexpr int kSinCos0 = 0, kAtan0 = 16, kExp0 = 38, kCount = 51;
constexpr double kTm[kCount] = {
    // sincos: 2/π; −π/2 in three pieces (the second is also used negated); cos polynomial; sin polynomial
    0x1.45f306dc9c883p-1,     //  0  0x3FE45F306DC9C883
    -0x1.921fb54442d18p+0,    //  1  0xBFF921FB54442D18
    -0x1.1a62633145c00p-54,   //  2  0xBC91A62633145C00
    -0x1.b839a252049c0p-104,  //  3  0xB97B839A252049C0
    -0x1.907db46cc5e42p-37,   //  4  0xBDA907DB46CC5E42
    0x1.1eeb69037ab78p-29,    //  5  0x3E21EEB69037AB78
    -0x1.27e4fa17f65f6p-22,   //  6  0xBE927E4FA17F65F6
    0x1.a01a019f4ec90p-16,    //  7  0x3EFA01A019F4EC90
    -0x1.6c16c16c16967p-10,   //  8  0xBF56C16C16C16967
    0x1.5555555555555p-5,     //  9  0x3FA5555555555555
    0x1.5e0b2f9a43bb8p-33,    // 10  0x3DE5E0B2F9A43BB8
    -0x1.ae600b42fdfa7p-26,   // 11  0xBE5AE600B42FDFA7
    0x1.71de3796cde01p-19,    // 12  0x3EC71DE3796CDE01
    -0x1.a01a019e83e5cp-13,   // 13  0xBF2A01A019E83E5C
    0x1.1111111110bb3p-7,     // 14  0x3F81111111110BB3
    -0x1.5555555555555p-3,    // 15  0xBFC5555555555555
    // atan: the reduced polynomial, highest power first; π/2 as a product of two
    0x1.ba404b5e68a13p-17,   // 16  0x3EEBA404B5E68A13
    -0x1.3e260bd3237f4p-13,  // 17  0xBF23E260BD3237F4
    0x1.b2bb069efb384p-11,   // 18  0x3F4B2BB069EFB384
    -0x1.7952daf56de9bp-9,   // 19  0xBF67952DAF56DE9B
    0x1.d6d43a595c56fp-8,    // 20  0x3F7D6D43A595C56F
    -0x1.c6ea4a57d9582p-7,   // 21  0xBF8C6EA4A57D9582
    0x1.67e295f08b19fp-6,    // 22  0x3F967E295F08B19F
    -0x1.e9ae6fc27006ap-6,   // 23  0xBF9E9AE6FC27006A
    0x1.2c15b5711927ap-5,    // 24  0x3FA2C15B5711927A
    -0x1.59976e82d3ff0p-5,   // 25  0xBFA59976E82D3FF0
    0x1.82d5d6ef28734p-5,    // 26  0x3FA82D5D6EF28734
    -0x1.ae5ce6a214619p-5,   // 27  0xBFAAE5CE6A214619
    0x1.e1bb48427b883p-5,    // 28  0x3FAE1BB48427B883
    -0x1.110e48b207f05p-4,   // 29  0xBFB110E48B207F05
    0x1.3b13657b87036p-4,    // 30  0x3FB3B13657B87036
    -0x1.745d119378e4fp-4,   // 31  0xBFB745D119378E4F
    0x1.c71c717e1913cp-4,    // 32  0x3FBC71C717E1913C
    -0x1.2492492376b7dp-3,   // 33  0xBFC2492492376B7D
    0x1.99999999952ccp-3,    // 34  0x3FC99999999952CC
    -0x1.5555555555523p-2,   // 35  0xBFD5555555555523
    0x1.dd9ad336a0500p-1,    // 36  0x3FEDD9AD336A0500
    0x1.af154eeb562d6p+0,    // 37  0x3FFAF154EEB562D6
    // exp: log2(e); ln 2 in two pieces; the polynomial, highest power first
    0x1.71547652b82fep+0,   // 38  0x3FF71547652B82FE
    0x1.62e42fefa39efp-1,   // 39  0x3FE62E42FEFA39EF
    0x1.abc9e3b39803fp-56,  // 40  0x3C7ABC9E3B39803F
    0x1.ade156a5dcb37p-26,  // 41  0x3E5ADE156A5DCB37
    0x1.28af3fca7ab0cp-22,  // 42  0x3E928AF3FCA7AB0C
    0x1.71dee623fde64p-19,  // 43  0x3EC71DEE623FDE64
    0x1.a01997c89e6b0p-16,  // 44  0x3EFA01997C89E6B0
    0x1.a01a014761f6ep-13,  // 45  0x3F2A01A014761F6E
    0x1.6c16c1852b7b0p-10,  // 46  0x3F56C16C1852B7B0
    0x1.1111111122322p-7,   // 47  0x3F81111111122322
    0x1.55555555502a1p-5,   // 48  0x3FA55555555502A1
    0x1.5555555555511p-3,   // 49  0x3FC5555555555511
    0x1.000000000000bp-1,   // 50  0x3FE000000000000B
};

// entry i of the table, 0 past its end (the kernels' per-lane set-up reads it with a lane's index)
SHIPSIM_HD double tm_entry(int i) { return (i >= 0 && i < kCount) ? kTm[i] : 0.0; }

// the constants as literals
struct TmLiteral {
  template <int I>
  SHIPSIM_HD double k() const {
    static_assert(I >= 0 && I < kCount, "tickmath table index");
    return kTm[I];
  }
  // the entry for a use that follows the last use of `dead` (a value of the same evaluation that is not read again):
  // a provider that delivers into a register takes `dead`'s, which keeps the delivery next to its use; here, nothing
  template <int I>
  SHIPSIM_HD double kd(double dead) const {
    (void)dead;
    return k<I>();
  }
};

SHIPSIM_HD uint64_t tm_bits(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
SHIPSIM_HD double tm_from_bits(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}
// double -> int32 of an integral double: the device's conversion saturates and takes NaN to 0; the callers' results
// do not depend on it outside int32 (exp's range selects; sincos's guard), so the host only has to stay defined
SHIPSIM_HD int tm_to_int(double y) {
#ifdef __HIP_DEVICE_COMPILE__
  return (int)y;
#else
  return (y >= -2147483648.0 && y <= 2147483647.0) ? (int)y : 0;
#endif
}

// the range of tm_sincos: the library's small-argument reduction (false for NaN and ±inf)
SHIPSIM_HD bool tm_sincos_small_ok(double x) { return fabs(x) < 0x1.0p+30; }

// sincos(x) for tm_sincos_small_ok(x): the reduction by π/2 in three pieces with the compensated tail
// (trigredsmall), the two polynomials on the reduced pair (sincosred2), the quadrant's swap and signs
template <class K>
SHIPSIM_HD void tm_sincos(double x, const K& T, double* sp, double* cp) {
  constexpr int B = kSinCos0;
  const double ax = fabs(x);
  const double y = rint(ax * T.template k<B + 0>());
  const double r4 = fma(y, T.template k<B + 1>(), ax);
  const double r5 = fma(y, T.template k<B + 2>(), r4);
  const double pm = -T.template k<B + 2>();  // (the library's fourth reduction constant: the third, negated)
  const double r6 = y * pm;
  const double r8 = fma(y, pm, -r6);
  const double r9 = r4 - r6;
  const double r10 = r4 - r9;
  const double r11 = r10 - r6;
  const double r12 = r9 - r5;
  const double r13 = r12 + r11;
  const double r14 = r13 - r8;
  const double r15 = fma(y, T.template k<B + 3>(), r14);
  const double hi = r5 + r15;
  const double r17 = hi - r5;
  const double lo = r15 - r17;
  const int q = tm_to_int(y) & 3;
  // sincosred2(hi, lo)
  const double x2 = hi * hi;
  const double h = x2 * 0.5;
  const double c5 = 1.0 - h;
  const double c6 = 1.0 - c5;
  const double c7 = c6 - h;
  const double x4 = x2 * x2;
  const double p0 = fma(x2, T.template kd<B + 4>(r12), T.template kd<B + 5>(r13));
  const double p1 = fma(x2, p0, T.template kd<B + 6>(r14));
  const double p2 = fma(x2, p1, T.template kd<B + 7>(p0));
  const double p3 = fma(x2, p2, T.template kd<B + 8>(p1));
  const double p = fma(x2, p3, T.template kd<B + 9>(p2));
  const double nlo = -lo;
  const double c15 = fma(hi, nlo, c7);
  const double c16 = fma(x4, p, c15);
  const double cc = c5 + c16;
  const double s0 = fma(x2, T.template kd<B + 10>(r10), T.template kd<B + 11>(r11));
  const double s1 = fma(x2, s0, T.template kd<B + 12>(r17));
  const double s2 = fma(x2, s1, T.template kd<B + 13>(s0));
  const double s = fma(x2, s2, T.template kd<B + 14>(s1));
  const double x3n = hi * (-x2);
  const double hl = lo * 0.5;
  const double s25 = fma(x3n, s, hl);
  const double s26 = fma(x2, s25, nlo);
  const double s27 = fma(x3n, T.template kd<B + 15>(s2), s26);
  const double ss = hi - s27;
  // the quadrant: swap on odd, negate from the second on; the sine takes the argument's sign
  const uint64_t flip = q > 1 ? 0x8000000000000000ull : 0ull;
  const bool even = (q & 1) == 0;
  const uint64_t sb = tm_bits(even ? ss : cc) ^ (tm_bits(x) & 0x8000000000000000ull) ^ flip;
  const uint64_t cb = tm_bits(even ? cc : -ss) ^ flip;
  *sp = tm_from_bits(sb);
  *cp = tm_from_bits(cb);
}

// atan(x): the reduced polynomial on min(|x|, 1 / |x|), π/2 minus it above 1, the argument's sign
template <class K>
SHIPSIM_HD double tm_atan(double x, const K& T) {
  constexpr int B = kAtan0;
  const double ax = fabs(x);
  const bool big = ax > 1.0;
  const double rc = 1.0 / ax;
  const double v = big ? rc : ax;
  const double t = v * v;
  const double q0 = fma(t, T.template kd<B + 0>(rc), T.template kd<B + 1>(ax));
  const double q1 = fma(t, q0, T.template k<B + 2>());
  const double q2 = fma(t, q1, T.template kd<B + 3>(q0));
  const double q3 = fma(t, q2, T.template kd<B + 4>(q1));
  const double q4 = fma(t, q3, T.template kd<B + 5>(q2));
  const double q5 = fma(t, q4, T.template kd<B + 6>(q3));
  const double q6 = fma(t, q5, T.template kd<B + 7>(q4));
  const double q7 = fma(t, q6, T.template kd<B + 8>(q5));
  const double q8 = fma(t, q7, T.template kd<B + 9>(q6));
  const double q9 = fma(t, q8, T.template kd<B + 10>(q7));
  const double q10 = fma(t, q9, T.template kd<B + 11>(q8));
  const double q11 = fma(t, q10, T.template kd<B + 12>(q9));
  const double q12 = fma(t, q11, T.template kd<B + 13>(q10));
  const double q13 = fma(t, q12, T.template kd<B + 14>(q11));
  const double q14 = fma(t, q13, T.template kd<B + 15>(q12));
  const double q15 = fma(t, q14, T.template kd<B + 16>(q13));
  const double q16 = fma(t, q15, T.template kd<B + 17>(q14));
  const double q17 = fma(t, q16, T.template kd<B + 18>(q15));
  const double q18 = fma(t, q17, T.template kd<B + 19>(q16));
  const double p = q18;
  const double tp = t * p;
  const double red = fma(v, tp, v);
  const double hi = fma(T.template k<B + 20>(), T.template k<B + 21>(), -red);
  const double r = big ? hi : red;
  return copysign(r, x);
}

// exp(x): x = n ln 2 + r with n = rint(x log2 e), the polynomial in r, the scaling, the two range selects
template <class K>
SHIPSIM_HD double tm_exp(double x, const K& T) {
  constexpr int B = kExp0;
  const double xl = x * T.template k<B + 0>();
  const double n = rint(xl);
  const double nn = -n;
  const double r0 = fma(nn, T.template k<B + 1>(), x);
  const double r = fma(nn, T.template kd<B + 2>(xl), r0);
  const double e0 = fma(r, T.template kd<B + 3>(r0), T.template kd<B + 4>(nn));
  const double e1 = fma(r, e0, T.template k<B + 5>());
  const double e2 = fma(r, e1, T.template kd<B + 6>(e0));
  const double e3 = fma(r, e2, T.template kd<B + 7>(e1));
  const double e4 = fma(r, e3, T.template kd<B + 8>(e2));
  const double e5 = fma(r, e4, T.template kd<B + 9>(e3));
  const double e6 = fma(r, e5, T.template kd<B + 10>(e4));
  const double e7 = fma(r, e6, T.template kd<B + 11>(e5));
  const double e8 = fma(r, e7, T.template kd<B + 12>(e6));
  double p = e8;
  p = fma(r, p, 1.0);
  p = fma(r, p, 1.0);
  double z = ldexp(p, tm_to_int(n));
  z = x > 1024.0 ? (double)INFINITY : z;
  z = x < -1075.0 ? 0.0 : z;
  return z;
}

}  // namespace tickmath
}  // namespace shipsim
