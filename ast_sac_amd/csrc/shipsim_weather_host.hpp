// shipsim_weather_host.hpp — the host half of shipsim_set_weather, free of the device and of the handle so that
// it can be compiled and driven on its own (tests/test_weather_cpu.py builds it into a stand-alone program with
// -fsanitize=address,undefined): which handles can run per-env weather, which values are refused, and the rows
// of the device array the weather kernels read.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "shipsim.h"
#include "shipsim_launch_host.hpp"

namespace weather_host {

// columns of the device array (kCols rows of n_envs doubles; shipsim_device.hpp WX_* are the same indices)
constexpr int kCols = 5;
constexpr int kWindSpeed = 0, kWindSin = 1, kWindCos = 2, kCurrentN = 3, kCurrentE = 4;

// why a handle of this kind cannot run per-env weather (NULL: it can); the kernels' side of it is launch_host::select
inline const char* unsupported(int kind, int machinery, int collav, bool recording, int n_ships = 2) {
  if (kind != SHIPSIM_KIND_AST) return "SHIPSIM_KIND_AST only (the SINGLE and NONIW kernels run the config's weather)";
  return launch_host::select(machinery, collav, n_ships, 16, recording, true, launch_host::kStep).why;
}

// the first env whose values are refused — a non-finite value or a negative wind speed — or -1
inline int64_t check(const double* ws, const double* wd, const double* vn, const double* ve, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!isfinite(ws[i]) || !isfinite(wd[i]) || !isfinite(vn[i]) || !isfinite(ve[i]) || ws[i] < 0) return (int64_t)i;
  return -1;
}

// the device array's rows: wind speed, sin and cos of the wind direction (the libm calls shipsim_create makes
// for Params::wind_sin / wind_cos), current from north, current from east
inline void rows(const double* ws, const double* wd, const double* vn, const double* ve, size_t n, double* out) {
  for (size_t i = 0; i < n; ++i) {
    out[kWindSpeed * n + i] = ws[i];
    out[kWindSin * n + i] = sin(wd[i]);
    out[kWindCos * n + i] = cos(wd[i]);
    out[kCurrentN * n + i] = vn[i];
    out[kCurrentE * n + i] = ve[i];
  }
}

}  // namespace weather_host
