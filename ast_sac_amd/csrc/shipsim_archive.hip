// shipsim_archive.hip — the state archive on the device (include/shipsim.h: shipsim_archive_store / _load / _elect);
// the fourth object of libshipsim. The arithmetic is shipsim_archive_host.hpp's; this file is its launch structure.
// No block waits on another inside a launch: what one stage of the election hands the next goes through the caller's
// workspace, and the order is the stream's.
//
//   archive_gather_kernel  [blocks, columns]  slot d of the destination takes slot index[d] of the source: the live
//                                             block into an archive (store) or an archive into the live block (load)
//   ar_clear_kernel   [n_cells / 256]  best = 0, winner = none, count = 0; *n_improved_out = 0
//   ar_max_kernel     [n_envs / 256]   best[cell] = max of the candidates' score images; count[cell] += 1
//   ar_min_kernel     [n_envs / 256]   winner[cell] = min env index among the candidates that hold best[cell]
//                                      (both: the lanes of a wave that name one cell send one atomic between them)
//   ar_fill_kernel    [n_cells / 256]  the winner takes the cell if it is empty or strictly improved; cell_seen,
//                                      *n_improved_out
//
// Every combination across envs is an unsigned max, a signed min or an integer add: associative and commutative, so
// the result does not depend on the order in which lanes, waves or blocks arrive.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "shipsim.h"
#include "shipsim_archive_host.hpp"
#include "shipsim_state.hpp"  // the launch functions' declarations

namespace AR = archive_host;

static_assert(AR::kMaxCells == SHIPSIM_ARCHIVE_MAX_CELLS, "shipsim.h and shipsim_archive_host.hpp name the same number");

namespace {

constexpr int kThreads = 256;
constexpr int64_t kGatherMaxBlocks = 1024;  // blocks per column (they stride over its units)

struct TablePair {
  state_host::Table src, dst;
};

// blockIdx.y is the column; the blocks of a column stride over the destination's units, so consecutive lanes store
// consecutive units and only the loads are gathered. src and dst are different allocations. An index that names no
// slot of the source is tested before any address is formed from it: that destination slot is not written.
__global__ __launch_bounds__(kThreads) void archive_gather_kernel(const TablePair T, const char* __restrict__ src,
                                                                  char* __restrict__ dst,
                                                                  const int32_t* __restrict__ index, uint32_t n_dst,
                                                                  uint32_t n_src) {
  const state_host::Column cs = T.src.col[blockIdx.y], cd = T.dst.col[blockIdx.y];
  const uint32_t total = n_dst * state_host::units_per_env(cd);  // (<= 2^31, and the stride <= 2^18: AR::kMaxUnits)
  const uint32_t stride = gridDim.x * (uint32_t)kThreads;
  for (uint32_t t = blockIdx.x * (uint32_t)kThreads + threadIdx.x; t < total; t += stride) {
    const int32_t from = index[AR::slot_of(cd, t)];
    if (!AR::index_ok(from, n_src)) continue;
    const char* p = src + AR::load_at(cs, (uint32_t)from, AR::piece_of(cd, t));
    char* q = dst + AR::store_at(cd, t);
    if (cd.unit == 16) *(uint4*)q = *(const uint4*)p;
    else if (cd.unit == 8) *(uint2*)q = *(const uint2*)p;
    else *(uint32_t*)q = *(const uint32_t*)p;
  }
}

__global__ __launch_bounds__(kThreads) void ar_clear_kernel(int n_cells, unsigned long long* __restrict__ best,
                                                            int32_t* __restrict__ winner, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ n_improved_out) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c == 0 && n_improved_out) *n_improved_out = 0;
  if (c >= n_cells) return;
  best[c] = 0;
  winner[c] = AR::kNoWinner;
  count[c] = 0;
}

// largest of x over the wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long wave_max(unsigned long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

// The two per-env stages combine the lanes of a wave that name the same cell before they go to memory: the wave
// peels one cell at a time (the cell of its lowest pending lane), and that group sends one atomic max and one add,
// or one atomic min, instead of one per lane; a group of one lane sends its own. With every env in one cell this is
// one atomic per wave on that address instead of 64 (profiles/archive.json: the A/B). Max, min and add are
// associative and commutative, so the grouping changes nothing in the result. `pending` and `group` are ballots,
// uniform over the wave: every lane runs the loop and its cross-lane moves, env or not.
__global__ __launch_bounds__(kThreads) void ar_max_kernel(int n_envs, uint32_t n_cells, const int32_t* __restrict__ cell,
                                                          const double* __restrict__ score, unsigned long long* best,
                                                          int32_t* count) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t c = -1;
  unsigned long long im = 0;
  bool cand = false;
  if (i < n_envs) {
    c = cell[i];
    const double s = score[i];
    cand = AR::candidate(c, n_cells, s);
    if (cand) im = AR::image_of_bits(AR::bits_of(s));
  }
  unsigned long long pending = __ballot(cand);
  while (pending) {
    const int leader = __ffsll(pending) - 1;
    const int32_t lc = __shfl(c, leader, 64);
    const bool mine = cand && c == lc;
    const unsigned long long group = __ballot(mine);
    if (__popcll(group) == 1) {
      if (mine) {
        atomicMax(&best[c], im);
        atomicAdd(&count[c], 1);
      }
    } else {
      const unsigned long long g = wave_max(mine ? im : 0ull);
      if (lane == leader) {
        atomicMax(&best[lc], g);
        atomicAdd(&count[lc], (int32_t)__popcll(group));
      }
    }
    pending &= ~group;
  }
}

// (the lanes of a wave hold increasing env indices: the lowest lane of a group holds its smallest)
__global__ __launch_bounds__(kThreads) void ar_min_kernel(int n_envs, uint32_t n_cells, const int32_t* __restrict__ cell,
                                                          const double* __restrict__ score,
                                                          const unsigned long long* __restrict__ best, int32_t* winner) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t c = -1;
  bool holds = false;
  if (i < n_envs) {
    c = cell[i];
    const double s = score[i];
    if (AR::candidate(c, n_cells, s)) holds = (unsigned long long)AR::image_of_bits(AR::bits_of(s)) == best[c];
  }
  unsigned long long pending = __ballot(holds);
  while (pending) {
    const int leader = __ffsll(pending) - 1;
    const int32_t lc = __shfl(c, leader, 64);
    const unsigned long long group = __ballot(holds && c == lc);
    if (lane == leader) atomicMin(&winner[lc], (int32_t)i);
    pending &= ~group;
  }
}

__global__ __launch_bounds__(kThreads) void ar_fill_kernel(int n_cells, const double* __restrict__ score,
                                                           const int32_t* __restrict__ winner,
                                                           const int32_t* __restrict__ count,
                                                           double* __restrict__ cell_score, int32_t* __restrict__ cell_seen,
                                                           int32_t* __restrict__ env_of_cell_out,
                                                           int32_t* n_improved_out) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  bool took = false;
  if (c < n_cells) {
    const int32_t w = winner[c];
    const int32_t got = AR::fill_cell(w, w == AR::kNoWinner ? 0.0 : score[w], &cell_score[c]);
    env_of_cell_out[c] = got;
    if (cell_seen) cell_seen[c] = (int32_t)((uint32_t)cell_seen[c] + (uint32_t)count[c]);
    took = got >= 0;
  }
  if (n_improved_out) {  // one add per wave: the number of its lanes whose cell was taken
    const unsigned long long m = __ballot(took);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_improved_out, (int32_t)__popcll(m));
  }
}

}  // namespace

void shipsim_archive_gather_launch(hipStream_t st, const state_host::Table& src_table,
                                   const state_host::Table& dst_table, const void* src, void* dst,
                                   const int32_t* index, int32_t n_dst, int32_t n_src) {
  TablePair T;
  T.src = src_table;
  T.dst = dst_table;
  const int64_t units = state_host::max_units(dst_table, n_dst);
  int64_t blocks = (units + kThreads - 1) / kThreads;
  if (blocks > kGatherMaxBlocks) blocks = kGatherMaxBlocks;
  hipLaunchKernelGGL(archive_gather_kernel, dim3((unsigned)blocks, state_host::kColumns), dim3(kThreads), 0, st, T,
                     (const char*)src, (char*)dst, index, (uint32_t)n_dst, (uint32_t)n_src);
}

extern "C" {

int64_t shipsim_archive_workspace_bytes(int32_t n_cells) {
  if (n_cells < 1 || n_cells > AR::kMaxCells) return SHIPSIM_EINVAL;
  return AR::layout(n_cells).bytes;
}

int shipsim_archive_elect(int32_t n_envs, int32_t n_cells, const int32_t* cell, const double* score,
                          double* cell_score, int32_t* cell_seen, void* workspace, int64_t workspace_bytes,
                          int32_t* env_of_cell_out, int32_t* n_improved_out, void* stream) {
  if (!AR::elect_args_ok(n_envs, n_cells, cell, score, cell_score, workspace, workspace_bytes, env_of_cell_out))
    return SHIPSIM_EINVAL;
  const AR::Layout L = AR::layout(n_cells);
  char* ws = (char*)workspace;
  unsigned long long* best = (unsigned long long*)(ws + L.best);
  int32_t *winner = (int32_t*)(ws + L.winner), *count = (int32_t*)(ws + L.count);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 per_cell((n_cells + kThreads - 1) / kThreads), per_env((n_envs + kThreads - 1) / kThreads), block(kThreads);
  hipLaunchKernelGGL(ar_clear_kernel, per_cell, block, 0, st, n_cells, best, winner, count, n_improved_out);
  hipLaunchKernelGGL(ar_max_kernel, per_env, block, 0, st, n_envs, (uint32_t)n_cells, cell, score, best, count);
  hipLaunchKernelGGL(ar_min_kernel, per_env, block, 0, st, n_envs, (uint32_t)n_cells, cell, score, best, winner);
  hipLaunchKernelGGL(ar_fill_kernel, per_cell, block, 0, st, n_cells, score, winner, count, cell_score, cell_seen,
                     env_of_cell_out, n_improved_out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

}  // extern "C"
