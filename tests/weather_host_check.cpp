// Stand-alone driver of shipsim_set_weather's host half (ast_sac_amd/csrc/shipsim_weather_host.hpp), built by
// tests/test_weather_cpu.py with -fsanitize=address,undefined: validation and the device array's rows on
// exactly-sized heap arrays, so that a read or write past n_envs entries is caught.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "shipsim_weather_host.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                          \
    }                                                    \
  } while (0)

int main() {
  namespace W = weather_host;
  CHECK(W::unsupported(SHIPSIM_KIND_AST, SHIPSIM_MACH_DETAILED, SHIPSIM_COLLAV_SBMPC, false) == nullptr);
  CHECK(W::unsupported(SHIPSIM_KIND_AST, SHIPSIM_MACH_DETAILED, SHIPSIM_COLLAV_NONE, false) == nullptr);
  CHECK(W::unsupported(SHIPSIM_KIND_SINGLE, SHIPSIM_MACH_DETAILED, SHIPSIM_COLLAV_NONE, false) != nullptr);
  CHECK(W::unsupported(SHIPSIM_KIND_NONIW, SHIPSIM_MACH_SIMPLIFIED, SHIPSIM_COLLAV_SBMPC, false) != nullptr);
  CHECK(W::unsupported(SHIPSIM_KIND_AST, SHIPSIM_MACH_SIMPLIFIED, SHIPSIM_COLLAV_NONE, false) != nullptr);
  CHECK(W::unsupported(SHIPSIM_KIND_AST, SHIPSIM_MACH_DETAILED, SHIPSIM_COLLAV_SIMPLE, false) != nullptr);
  CHECK(W::unsupported(SHIPSIM_KIND_AST, SHIPSIM_MACH_DETAILED, SHIPSIM_COLLAV_SBMPC, true) != nullptr);

  for (size_t n : {(size_t)1, (size_t)7, (size_t)64, (size_t)4097}) {
    std::vector<double> ws(n), wd(n), vn(n), ve(n), out(W::kCols * n, -7.0);
    for (size_t i = 0; i < n; ++i) {
      ws[i] = 0.5 * (double)(i % 25);
      wd[i] = -3.0 + 0.37 * (double)(i % 17);
      vn[i] = 0.1 * (double)(i % 9) - 0.4;
      ve[i] = 0.4 - 0.1 * (double)(i % 7);
    }
    CHECK(W::check(ws.data(), wd.data(), vn.data(), ve.data(), n) == -1);
    W::rows(ws.data(), wd.data(), vn.data(), ve.data(), n, out.data());
    for (size_t i = 0; i < n; ++i) {
      CHECK(out[W::kWindSpeed * n + i] == ws[i]);
      CHECK(out[W::kWindSin * n + i] == sin(wd[i]));
      CHECK(out[W::kWindCos * n + i] == cos(wd[i]));
      CHECK(out[W::kCurrentN * n + i] == vn[i]);
      CHECK(out[W::kCurrentE * n + i] == ve[i]);
    }
    // the last env is looked at, and the first offender is the one reported
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<double>* cols[4] = {&ws, &wd, &vn, &ve};
    for (int k = 0; k < 4; ++k)
      for (double bad : {nan, inf, -inf}) {
        const double keep = (*cols[k])[n - 1];
        (*cols[k])[n - 1] = bad;
        CHECK(W::check(ws.data(), wd.data(), vn.data(), ve.data(), n) == (int64_t)(n - 1));
        (*cols[k])[n - 1] = keep;
      }
    const double keep = ws[0];
    ws[0] = -1e-300;
    CHECK(W::check(ws.data(), wd.data(), vn.data(), ve.data(), n) == 0);
    ws[0] = 0.0;  // a calm is weather too
    CHECK(W::check(ws.data(), wd.data(), vn.data(), ve.data(), n) == -1);
    ws[0] = keep;
  }
  printf("weather host OK\n");
  return 0;
}
