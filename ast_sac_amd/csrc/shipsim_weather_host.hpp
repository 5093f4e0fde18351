// shipsim_weather_host.hpp — the host half of shipsim_set_weather, free of the device and of the handle so that
// it can be compiled and driven on its own (tests/test_weather_cpu.py builds it into a stand-alone program with
// -fsanitize=address,undefined): which handles can run per-env weather, which values are refused, and the rows
// of the device array the weather kernels read. Below them the host half of the calls that move weather on the
// device (shipsim_weather_store / _load / _fork; tests/test_weather_carry_cpu.py drives it the same way): the stored
// table's sizes and row offsets, the reasons a call is refused, and the gather of shipsim_weather.hip restated.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "shipsim.h"
#include "shipsim_launch_host.hpp"

#if defined(__HIPCC__)
#define WXH_HD __host__ __device__
#else
#define WXH_HD
#endif

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

// ---- weather that moves on the device: the stored table ----
// The handle's table and a caller's weather buffer are kStoreRows rows of n_slots doubles: the kCols rows the kernels
// read (above, where they were) and below them the wind direction as it was set. shipsim_get_weather reads the
// direction back from that row: it cannot be recomputed from its sin and cos bit for bit, so it travels with them.
constexpr int kStoreRows = 6;
constexpr int kDirection = 5;
constexpr int32_t kMaxSlots = 1 << 22;  // SHIPSIM_ARCHIVE_MAX_CELLS
static_assert(kDirection == kCols && kStoreRows == kCols + 1, "the direction row follows the rows the kernels read");

constexpr bool slots_ok(int32_t n_slots) { return n_slots >= 1 && n_slots <= kMaxSlots; }
// row r of a table of n_slots slots starts at this byte; the table's size
constexpr int64_t row_offset(int r, int64_t n_slots) { return (int64_t)r * n_slots * (int64_t)sizeof(double); }
constexpr int64_t store_bytes(int64_t n_slots) { return row_offset(kStoreRows, n_slots); }
static_assert(store_bytes(1) == 48 && row_offset(kDirection, 300) == 12000 && store_bytes(kMaxSlots) == (int64_t)192 << 20,
              "six rows of n_slots doubles");

// the rows of the stored table: rows() and the direction as given
inline void store_rows(const double* ws, const double* wd, const double* vn, const double* ve, size_t n, double* out) {
  rows(ws, wd, vn, ve, n, out);
  for (size_t i = 0; i < n; ++i) out[kDirection * n + i] = wd[i];
}

// why shipsim_weather_fork refuses a call (NULL: it serves it): it has no buffer
inline const char* fork_refusal(bool weather_on) {
  return weather_on ? nullptr : "the handle runs the config's weather (no per-env weather is in force: shipsim_set_weather)";
}
// ... and shipsim_weather_store / _load, in the order they test
inline const char* carry_refusal(bool weather_on, const void* wx, int64_t bytes, int32_t n_slots, int32_t n_envs,
                                 const void* index) {
  if (const char* why = fork_refusal(weather_on)) return why;
  if (!wx) return "the weather buffer is NULL";
  if (!slots_ok(n_slots)) return "n_slots is not in 1..4194304 (SHIPSIM_ARCHIVE_MAX_CELLS)";
  if (bytes != store_bytes(n_slots)) return "bytes is not shipsim_weather_bytes(n_slots)";
  if ((uintptr_t)wx & 15) return "the weather buffer is not 16-byte aligned";
  if (!index && n_slots != n_envs) return "a NULL index is the identity and needs n_slots == n_envs";
  return nullptr;
}

// an index is served when it names a slot of the source: tested before any address is formed from it (a negative
// one is >= 2^31 as unsigned)
WXH_HD constexpr bool index_ok(int32_t index, uint32_t n_src) { return (uint32_t)index < n_src; }
static_assert(index_ok(0, 1) && !index_ok(1, 1) && !index_ok(-1, 1u << 22) && !index_ok(INT32_MIN, 1u << 22) &&
                  !index_ok(INT32_MAX, 1u << 22), "indices outside [0, n_src) are not served");

// The gather as the kernel runs it: slot d of dst (n_dst slots) takes slot index[d] of src (n_src slots), all
// kStoreRows rows; index NULL is the identity. An index that names no slot of the source leaves slot d untouched —
// or, with `own` (the in-place fork, which gathers into a staging table that is then copied back; n_src == n_dst),
// slot d takes slot d of the source, so that the copy back leaves it as it was.
inline void gather(const double* src, double* dst, const int32_t* index, uint32_t n_dst, uint32_t n_src, bool own) {
  for (uint32_t d = 0; d < n_dst; ++d) {
    int32_t from = index ? index[d] : (int32_t)d;
    if (!index_ok(from, n_src)) {
      if (!own) continue;
      from = (int32_t)d;
    }
    for (int r = 0; r < kStoreRows; ++r) dst[(size_t)r * n_dst + d] = src[(size_t)r * n_src + (uint32_t)from];
  }
}

}  // namespace weather_host
