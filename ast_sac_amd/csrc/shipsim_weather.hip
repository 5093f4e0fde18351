// shipsim_weather.hip — per-env weather that moves on the device (include/shipsim.h: shipsim_weather_store / _load /
// _fork); the sixth object of libshipsim. The arithmetic is shipsim_weather_host.hpp's; this file is one kernel and
// its launch.
//
//   weather_gather_kernel  [n_dst / 256]  slot d of the destination table takes slot index[d] of the source table,
//                                         all six rows: the handle's table into a caller's buffer (store), a buffer
//                                         into the handle's table (load), the handle's table into its staging table
//                                         (fork; the caller copies it back)
//
// One thread per destination slot: consecutive lanes store consecutive doubles of every row and only the loads are
// gathered. No atomics and no two threads write one address, so duplicate indices are harmless. src and dst are
// different allocations.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "shipsim_state.hpp"  // the launch function's declaration
#include "shipsim_weather_host.hpp"

namespace WX = weather_host;

static_assert(WX::kMaxSlots == SHIPSIM_ARCHIVE_MAX_CELLS, "shipsim.h and shipsim_weather_host.hpp name the same number");

namespace {

constexpr int kThreads = 256;

// An index that names no slot of the source is tested before any address is formed from it: slot d is not written,
// or (own: n_src == n_dst, the staging table of a fork) takes slot d of the source.
__global__ __launch_bounds__(kThreads) void weather_gather_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                  const int32_t* __restrict__ index, uint32_t n_dst,
                                                                  uint32_t n_src, int own) {
  const uint32_t d = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (d >= n_dst) return;
  int32_t from = index[d];
  if (!WX::index_ok(from, n_src)) {
    if (!own) return;
    from = (int32_t)d;
  }
  double v[WX::kStoreRows];
#pragma unroll
  for (int r = 0; r < WX::kStoreRows; ++r) v[r] = src[(size_t)r * n_src + (uint32_t)from];
#pragma unroll
  for (int r = 0; r < WX::kStoreRows; ++r) dst[(size_t)r * n_dst + d] = v[r];
}

}  // namespace

void shipsim_weather_gather_launch(hipStream_t st, const double* src, double* dst, const int32_t* index, int32_t n_dst,
                                   int32_t n_src, bool own) {
  const unsigned blocks = ((unsigned)n_dst + kThreads - 1) / kThreads;  // (n_dst <= 2^22: 16384 blocks at the most)
  hipLaunchKernelGGL(weather_gather_kernel, dim3(blocks), dim3(kThreads), 0, st, src, dst, index, (uint32_t)n_dst,
                     (uint32_t)n_src, own ? 1 : 0);
}
