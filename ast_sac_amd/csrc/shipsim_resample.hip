// shipsim_resample.hip — weighted splitting on the device (include/shipsim.h: shipsim_resample,
// shipsim_level_distance); the third object of libshipsim. The arithmetic is shipsim_resample_host.hpp's; this file is
// its launch structure. No block waits on another inside a launch: what one stage hands the next goes through the
// caller's workspace, and the order is the stream's.
//
//   rs_mass_kernel     [tiles]   p = weight * potential; the tile's largest, or -1 for a negative / non-finite one
//   rs_head_kernel     [1]       m, e, status over the tiles' results
//   rs_quant_kernel    [tiles]   q and its inclusive sum within the tile (cl), the tile's sum; clears first / last
//   rs_offsets_kernel  [1]       sum of the tiles before each tile; after the q scan also Q, U, s, r, total_out
//   rs_select_kernel   [n / 256] slot j's systematic position and the env it falls on (sel); env j's clone weight
//   sorted:   rs_finish_kernel   src_out = sel and the weights
//   in place: rs_runs_kernel     where each selected env's run in sel begins and ends
//             rs_pair_kernel     [tiles]  inclusive sum within the tile of (surplus | empty << 32)
//             rs_offsets_kernel  [1]
//             rs_finish_kernel   an empty slot searches its clone's source; the weights
//   level_distance_kernel        per env, the own ship's distance to the nearest obstacle ship
//
// The scans have two levels (a tile of 1024 envs; one workgroup striding over the at most 4096 tile sums) and stay in
// that form: the searches go through both levels (resample_host::search2), so no pass adds the offsets back.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "shipsim.h"
#include "shipsim_resample_host.hpp"
#include "shipsim_state.hpp"  // DevState (level_distance_kernel)

namespace RS = resample_host;

static_assert(RS::kMaxN == SHIPSIM_RESAMPLE_MAX_N && RS::kSorted == SHIPSIM_RESAMPLE_SORTED &&
                  RS::kInPlace == SHIPSIM_RESAMPLE_IN_PLACE,
              "shipsim.h and shipsim_resample_host.hpp name the same numbers");

namespace {

constexpr int kThreads = 256;
constexpr int kItems = RS::kTile / kThreads;  // a thread's share of a tile, kThreads apart (coalesced)
static_assert(kItems * kThreads == RS::kTile, "a tile is a whole number of rounds of the block");

// inclusive scan over the wave through cross-lane moves (each a pair of 32-bit moves)
__device__ __forceinline__ uint64_t wave_scan(uint64_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

// inclusive scan over the block's 256 threads; *total: the block's sum. lds: 4 words, free again on return
__device__ __forceinline__ uint64_t block_scan(uint64_t x, uint64_t* lds, uint64_t* total) {
  x = wave_scan(x);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) lds[wave] = x;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const uint64_t v = lds[w];
    if (w < wave) before += v;
    all += v;
  }
  __syncthreads();
  *total = all;
  return x + before;
}

// the tile's inclusive scan of v(i) into loc, its sum into tsum[tile]
template <class F>
__device__ __forceinline__ void tile_scan(int n, uint64_t* __restrict__ loc, uint64_t* __restrict__ tsum, F v) {
  __shared__ uint64_t lds[kThreads / 64];
  const int base = blockIdx.x * RS::kTile;
  uint64_t carry = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int i = base + k * kThreads + threadIdx.x;
    uint64_t total;
    const uint64_t x = block_scan(i < n ? v(i) : 0, lds, &total);
    if (i < n) loc[i] = carry + x;
    carry += total;
  }
  if (threadIdx.x == 0) tsum[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void rs_mass_kernel(int n, const double* __restrict__ weight,
                                                           const double* __restrict__ potential,
                                                           double* __restrict__ part) {
  __shared__ double lds[kThreads / 64];
  const int base = blockIdx.x * RS::kTile;
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int i = base + k * kThreads + threadIdx.x;
    if (i < n) {
      const double p = weight[i] * potential[i];
      if (!RS::mass_ok(p)) m = -1.0;
      else if (m >= 0.0 && p > m) m = p;
    }
  }
  // -1 wins over every mass: the reduction takes the smaller if either is negative, the larger otherwise
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(m, o, 64);
    m = (m < 0.0 || y < 0.0) ? -1.0 : (y > m ? y : m);
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      const double y = lds[w];
      m = (m < 0.0 || y < 0.0) ? -1.0 : (y > m ? y : m);
    }
    part[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(kThreads) void rs_head_kernel(int nt, const double* __restrict__ part,
                                                           RS::Head* __restrict__ hd, double* __restrict__ total_out,
                                                           int32_t* __restrict__ status_out) {
  __shared__ double lds[kThreads / 64];
  double m = 0.0;
  for (int b = threadIdx.x; b < nt; b += kThreads) {
    const double y = part[b];
    m = (m < 0.0 || y < 0.0) ? -1.0 : (y > m ? y : m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(m, o, 64);
    m = (m < 0.0 || y < 0.0) ? -1.0 : (y > m ? y : m);
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      const double y = lds[w];
      m = (m < 0.0 || y < 0.0) ? -1.0 : (y > m ? y : m);
    }
    const int status = m < 0.0 ? RS::kBadMass : (m == 0.0 ? RS::kNoMass : RS::kOk);
    int e = 0;
    if (status == RS::kOk) (void)frexp(m, &e);
    hd->m = m;
    hd->e = e;
    hd->status = status;
    hd->Q = 0; hd->U = 0; hd->s = 0; hd->r = 0; hd->qd = 0.0;
    if (status_out) *status_out = status;
    if (total_out && status != RS::kOk) *total_out = 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void rs_quant_kernel(int n, const double* __restrict__ weight,
                                                            const double* __restrict__ potential,
                                                            const RS::Head* __restrict__ hd, uint64_t* __restrict__ cl,
                                                            uint64_t* __restrict__ tsum, int32_t* __restrict__ first,
                                                            int32_t* __restrict__ last) {
  if (hd->status != RS::kOk) return;
  const int e = hd->e;
  tile_scan(n, cl, tsum, [&](int i) {
    first[i] = 0;
    last[i] = 0;
    return RS::quantise(weight[i] * potential[i], e);
  });
}

// Exclusive scan of the tile sums by one workgroup striding over them. With `counter` (after the q scan): one thread
// goes on to the grand total Q, the offset U and the rest of the head.
__global__ __launch_bounds__(kThreads) void rs_offsets_kernel(int n, int nt, const uint64_t* __restrict__ tsum,
                                                              uint64_t* __restrict__ toff, RS::Head* __restrict__ hd,
                                                              uint64_t seed, const int64_t* __restrict__ counter,
                                                              double* __restrict__ total_out) {
  __shared__ uint64_t lds[kThreads / 64];
  if (hd->status != RS::kOk) return;
  uint64_t carry = 0;
  for (int b0 = 0; b0 < nt; b0 += kThreads) {
    const int b = b0 + threadIdx.x;
    const uint64_t v = b < nt ? tsum[b] : 0;
    uint64_t total;
    const uint64_t x = block_scan(v, lds, &total);
    if (b < nt) toff[b] = carry + x - v;
    carry += total;
  }
  if (counter && threadIdx.x == 0) {
    const uint64_t Q = carry;
    uint64_t hi, lo;
    RS::offset_bits(seed, *counter, &hi, &lo);
    hd->Q = Q;
    hd->U = RS::mod128(hi, lo, Q);
    hd->s = Q / (uint64_t)n;
    hd->r = Q % (uint64_t)n;
    hd->qd = (double)Q;
    if (total_out) *total_out = RS::total_mass(Q, hd->e);
  }
}

__global__ __launch_bounds__(kThreads) void rs_select_kernel(int n, const double* __restrict__ weight,
                                                             const RS::Head* __restrict__ hd,
                                                             const uint64_t* __restrict__ toff,
                                                             const uint64_t* __restrict__ cl, int32_t* __restrict__ sel,
                                                             double* __restrict__ wsrc) {
  if (hd->status != RS::kOk) return;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint64_t t = RS::position((uint64_t)j, hd->s, hd->r, hd->U, (uint64_t)n);
  sel[j] = RS::search2(toff, cl, n, t, RS::kAll);
  const uint64_t q = RS::q_of(cl, j);
  wsrc[j] = q ? RS::clone_weight(weight[j], hd->qd, n, q) : 0.0;  // (an env with q = 0 is never a source)
}

__global__ __launch_bounds__(kThreads) void rs_runs_kernel(int n, const RS::Head* __restrict__ hd,
                                                           const int32_t* __restrict__ sel, int32_t* __restrict__ first,
                                                           int32_t* __restrict__ last) {
  if (hd->status != RS::kOk) return;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const int s = sel[j];
  if (j == 0 || sel[j - 1] != s) first[s] = j;
  if (j == n - 1 || sel[j + 1] != s) last[s] = j + 1;
}

__global__ __launch_bounds__(kThreads) void rs_pair_kernel(int n, const RS::Head* __restrict__ hd,
                                                           const int32_t* __restrict__ first,
                                                           const int32_t* __restrict__ last, uint64_t* __restrict__ al,
                                                           uint64_t* __restrict__ tsum2) {
  if (hd->status != RS::kOk) return;
  tile_scan(n, al, tsum2, [&](int i) { return RS::packed_pair(last[i] - first[i]); });
}

// The last stage of both arrangements: slot j's source and weight. Without usable mass (status != 0) every slot keeps
// itself and its weight. weight_out may be weight: a slot reads either its own weight or wsrc.
__global__ __launch_bounds__(kThreads) void rs_finish_kernel(int n, int arrangement, const double* weight,
                                                             const RS::Head* __restrict__ hd,
                                                             const int32_t* __restrict__ sel,
                                                             const int32_t* __restrict__ first,
                                                             const int32_t* __restrict__ last,
                                                             const uint64_t* __restrict__ toff2,
                                                             const uint64_t* __restrict__ al,
                                                             const double* __restrict__ wsrc, int32_t* __restrict__ src_out,
                                                             double* weight_out) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  if (hd->status != RS::kOk) {
    src_out[j] = j;
    weight_out[j] = weight[j];
    return;
  }
  const int s = arrangement == RS::kSorted ? sel[j] : RS::in_place_source(j, last[j] - first[j], toff2, al, n);
  src_out[j] = s;
  weight_out[j] = wsrc[s];
}

// min over the obstacle ships k = 1..K of sqrt(dn * dn + de * de) from the own ship (ship 0), as written: one
// multiply, one multiply, one add and one square root per ship, each rounded on its own
__global__ __launch_bounds__(kThreads) void level_distance_kernel(const DevState S, int n_envs, int n_ships,
                                                                  double* __restrict__ out) {
  const int env = blockIdx.x * kThreads + threadIdx.x;
  if (env >= n_envs) return;
  const double* north = S.f(SF_N) + (size_t)env * n_ships;
  const double* east = S.f(SF_E) + (size_t)env * n_ships;
  const double n0 = north[0], e0 = east[0];
  double best = INFINITY;
  for (int k = 1; k < n_ships; ++k) {
    const double dn = n0 - north[k], de = e0 - east[k];
    const double d = sqrt(dn * dn + de * de);
    if (d < best) best = d;
  }
  out[env] = best;
}

}  // namespace

void shipsim_level_distance_launch(hipStream_t st, const DevState& S, int n_envs, int n_ships, double* out) {
  hipLaunchKernelGGL(level_distance_kernel, dim3((n_envs + kThreads - 1) / kThreads), dim3(kThreads), 0, st, S, n_envs,
                     n_ships, out);
}

extern "C" {

int64_t shipsim_resample_workspace_bytes(int32_t n) {
  if (n < 1 || n > RS::kMaxN) return SHIPSIM_EINVAL;
  return RS::layout(n).bytes;
}

int shipsim_resample(int32_t n, const double* weight, const double* potential, uint64_t seed, const int64_t* counter,
                     int32_t arrangement, void* workspace, int64_t workspace_bytes, int32_t* src_out,
                     double* weight_out, double* total_out, int32_t* status_out, void* stream) {
  if (n < 1 || n > RS::kMaxN) return SHIPSIM_EINVAL;
  if (!weight || !potential || !counter || !workspace || !src_out || !weight_out) return SHIPSIM_EINVAL;
  if (arrangement != RS::kSorted && arrangement != RS::kInPlace) return SHIPSIM_EINVAL;
  const RS::Layout L = RS::layout(n);
  if (workspace_bytes < L.bytes || ((uintptr_t)workspace & 15)) return SHIPSIM_EINVAL;
  char* ws = (char*)workspace;
  RS::Head* hd = (RS::Head*)(ws + L.head);
  double* part = (double*)(ws + L.part);
  uint64_t *tsum = (uint64_t*)(ws + L.tsum), *toff = (uint64_t*)(ws + L.toff);
  uint64_t *tsum2 = (uint64_t*)(ws + L.tsum2), *toff2 = (uint64_t*)(ws + L.toff2);
  uint64_t *cl = (uint64_t*)(ws + L.cl), *al = (uint64_t*)(ws + L.al);
  double* wsrc = (double*)(ws + L.wsrc);
  int32_t *sel = (int32_t*)(ws + L.sel), *first = (int32_t*)(ws + L.first), *last = (int32_t*)(ws + L.last);
  const hipStream_t st = (hipStream_t)stream;
  const int nt = RS::tiles(n);
  const dim3 per_tile(nt), per_env((n + kThreads - 1) / kThreads), one(1), block(kThreads);
  hipLaunchKernelGGL(rs_mass_kernel, per_tile, block, 0, st, n, weight, potential, part);
  hipLaunchKernelGGL(rs_head_kernel, one, block, 0, st, nt, part, hd, total_out, status_out);
  hipLaunchKernelGGL(rs_quant_kernel, per_tile, block, 0, st, n, weight, potential, hd, cl, tsum, first, last);
  hipLaunchKernelGGL(rs_offsets_kernel, one, block, 0, st, n, nt, tsum, toff, hd, seed, counter, total_out);
  hipLaunchKernelGGL(rs_select_kernel, per_env, block, 0, st, n, weight, hd, toff, cl, sel, wsrc);
  if (arrangement == RS::kInPlace) {
    hipLaunchKernelGGL(rs_runs_kernel, per_env, block, 0, st, n, hd, sel, first, last);
    hipLaunchKernelGGL(rs_pair_kernel, per_tile, block, 0, st, n, hd, first, last, al, tsum2);
    hipLaunchKernelGGL(rs_offsets_kernel, one, block, 0, st, n, nt, tsum2, toff2, hd, (uint64_t)0,
                       (const int64_t*)nullptr, (double*)nullptr);
  }
  hipLaunchKernelGGL(rs_finish_kernel, per_env, block, 0, st, n, arrangement, weight, hd, sel, first, last, toff2, al,
                     wsrc, src_out, weight_out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

}  // extern "C"
