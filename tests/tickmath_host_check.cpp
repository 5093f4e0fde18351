// Stand-alone driver of the tick math's host form (ast_sac_amd/csrc/shipsim_tickmath.hpp), built by
// tests/test_tick_math_cpu.py with -ffp-contract=off and -fsanitize=address,undefined. Without arguments: the table's
// indexing (pinned bit patterns, the bounds of tm_entry), the range predicate of tm_sincos, the functions' special
// values, and a sweep against libm. With `eval`: reads "fn n" (fn 0 sincos, 1 atan, 2 exp) and n arguments as 64-bit
// hex patterns from stdin and prints each argument's result patterns (two per line; the second is 0 for atan / exp), for
// the test's comparison with the device library's recorded bits. Outside tm_sincos_small_ok a sincos row prints 0 0:
// there the caller uses the library.
#include <inttypes.h>
#include <math.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "shipsim_tickmath.hpp"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                               \
    }                                                         \
  } while (0)

using namespace shipsim::tickmath;

static int eval_mode() {
  int fn = -1, n = 0;
  if (scanf("%d %d", &fn, &n) != 2 || fn < 0 || fn > 2 || n < 0) return 2;
  std::vector<uint64_t> xs((size_t)n);
  for (uint64_t& v : xs)
    if (scanf("%" SCNx64, &v) != 1) return 2;
  const TmLiteral T;
  for (uint64_t u : xs) {
    const double x = tm_from_bits(u);
    double a = 0.0, b = 0.0;
    if (fn == 0) {
      if (tm_sincos_small_ok(x)) tm_sincos(x, T, &a, &b);
    } else if (fn == 1) {
      a = tm_atan(x, T);
    } else {
      a = tm_exp(x, T);
    }
    printf("%016" PRIx64 " %016" PRIx64 "\n", tm_bits(a), tm_bits(b));
  }
  return 0;
}

static double ulps(double got, double want) {
  if (got == want) return 0.0;
  const double u = nextafter(fabs(want), INFINITY) - fabs(want);
  return fabs(got - want) / u;
}

int main(int argc, char** argv) {
  if (argc > 1) return eval_mode();
  const TmLiteral T;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // the table: its sections, pinned patterns at their ends, and tm_entry's bounds
  CHECK(kSinCos0 == 0 && kAtan0 == 16 && kExp0 == 38 && kCount == 51);
  CHECK(sizeof(kTm) == sizeof(double) * kCount);
  CHECK(tm_bits(kTm[0]) == 0x3FE45F306DC9C883ull && tm_bits(kTm[15]) == 0xBFC5555555555555ull);
  CHECK(tm_bits(kTm[16]) == 0x3EEBA404B5E68A13ull && tm_bits(kTm[37]) == 0x3FFAF154EEB562D6ull);
  CHECK(tm_bits(kTm[38]) == 0x3FF71547652B82FEull && tm_bits(kTm[50]) == 0x3FE000000000000Bull);
  CHECK(tm_bits(T.k<kAtan0 + 20>()) == 0x3FEDD9AD336A0500ull && tm_bits(T.k<kExp0 + 2>()) == 0x3C7ABC9E3B39803Full);
  for (int i = 0; i < kCount; ++i) CHECK(tm_bits(tm_entry(i)) == tm_bits(kTm[i]) && kTm[i] != 0.0);
  CHECK(tm_entry(-1) == 0.0 && tm_entry(kCount) == 0.0 && tm_entry(kCount + 12) == 0.0 && tm_entry(1 << 30) == 0.0);
  CHECK(kTm[kAtan0 + 20] * kTm[kAtan0 + 21] > 1.5707963 && kTm[kAtan0 + 20] * kTm[kAtan0 + 21] < 1.5707964);
  // the range predicate: below 2^30 in magnitude, and finite
  const double lim = 1073741824.0;
  CHECK(!tm_sincos_small_ok(lim) && !tm_sincos_small_ok(-lim) && tm_sincos_small_ok(nextafter(lim, 0.0)));
  CHECK(tm_sincos_small_ok(-nextafter(lim, 0.0)) && !tm_sincos_small_ok(nextafter(lim, inf)));
  CHECK(!tm_sincos_small_ok(inf) && !tm_sincos_small_ok(-inf) && !tm_sincos_small_ok(nan));
  CHECK(tm_sincos_small_ok(0.0) && tm_sincos_small_ok(-0.0) && tm_sincos_small_ok(5e-324));
  // the conversion stays defined where the device's saturates
  CHECK(tm_to_int(3.0) == 3 && tm_to_int(-7.0) == -7 && tm_to_int(1e300) == 0 && tm_to_int(nan) == 0);
  // special values
  double s, c;
  tm_sincos(0.0, T, &s, &c);
  CHECK(s == 0.0 && !signbit(s) && c == 1.0);
  tm_sincos(-0.0, T, &s, &c);
  CHECK(s == 0.0 && signbit(s) && c == 1.0);
  CHECK(tm_atan(0.0, T) == 0.0 && signbit(tm_atan(-0.0, T)) && isnan(tm_atan(nan, T)));
  CHECK(ulps(tm_atan(inf, T), M_PI / 2) <= 1 && ulps(tm_atan(-inf, T), -M_PI / 2) <= 1);
  CHECK(ulps(tm_atan(1.0, T), M_PI / 4) <= 1 && ulps(tm_atan(1e300, T), M_PI / 2) <= 1);
  CHECK(tm_exp(0.0, T) == 1.0 && tm_exp(-0.0, T) == 1.0 && isnan(tm_exp(nan, T)));
  CHECK(tm_exp(inf, T) == inf && tm_exp(-inf, T) == 0.0 && tm_exp(1025.0, T) == inf && tm_exp(-1080.0, T) == 0.0);
  CHECK(tm_exp(-745.0, T) > 0.0 && tm_exp(-745.0, T) < 1e-322 && tm_exp(709.0, T) < inf);
  // a sweep against libm: the library's functions are good to 2 ulp
  double worst = 0.0;
  for (int i = -4000; i <= 4000; ++i) {
    const double x = i * 0.37 + 1e-3 * i * i;
    tm_sincos(x, T, &s, &c);
    if (fabs(sin(x)) > 1e-3) worst = fmax(worst, ulps(s, sin(x)));
    if (fabs(cos(x)) > 1e-3) worst = fmax(worst, ulps(c, cos(x)));
    const double a = i * 0.0173;
    worst = fmax(worst, ulps(tm_atan(a, T), atan(a)));
    worst = fmax(worst, ulps(tm_atan(a * a * a, T), atan(a * a * a)));
    const double e = i * 0.17;
    worst = fmax(worst, ulps(tm_exp(e, T), exp(e)));
  }
  CHECK(worst <= 2.0);
  printf("tickmath host OK worst %.3f ulp\n", worst);
  return 0;
}
