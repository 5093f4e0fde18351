// shipsim_tree.hip — the search tree on the device (include/shipsim.h: shipsim_tree_init / _select / _expand /
// _backup); the fifth object of libshipsim. The arithmetic is shipsim_tree_host.hpp's; this file is its launch
// structure. No block waits on another inside a launch: what one launch hands the next goes through the caller's
// workspace, and the order is the stream's.
//
//   tr_init_kernel    [1]              the header and the root
//   select
//   tr_clear_kernel   [n_nodes / 256]  stay = newc = 0; the level counts; the root as level 0's frontier with W arrivals
//   tr_level_kernel   [frontier / 4]   once per level 0..max_depth, a wave per node with arrivals and a child per lane:
//                                      the node's arrivals are routed one after the other (widen, stay, or the child of
//                                      the largest score: max across the wave, then the lowest lane that holds it);
//                                      the children that got arrivals are appended to the next level's frontier
//   tr_tile_kernel    [n / 1024]       the sum of a tile's counts (stay + newc per node; widening workers in expand)
//   tr_offset_kernel  [n / 1024]       off[v]: the sums of the tiles before, then an exclusive scan inside the tile
//   tr_leaf_kernel    [W / 256]        worker w finds its node in off[] by bisection: leaf_out, expand_out
//   expand
//   tr_slot_kernel    [W / 256]        the child slot of every widening worker, from the tree as it was
//   tr_tile_kernel, then tr_expand_kernel [W / 1024]  rank among the widening workers, the new node, its parent's
//                                      child[] and n_children, node_out, dropped
//   tr_count_kernel   [1]              n_nodes advances by the sum of the tile sums, up to max_nodes
//   backup
//   tr_backup_kernel  [W / 256]        visits += 1 and value_sum += q from node[w] up to, not including, the root;
//                                      the root takes one add per wave: every path ends there
//
// Every combination across workers is an integer add or an OR, so the result does not depend on the order in which
// lanes, waves or blocks arrive; the frontier's order does not matter either (a node is in it once and writes only
// its own entries). Every index read from memory is tested before an address is formed from it, and every loop has a
// bound that does not depend on the tree's contents being sane.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "shipsim.h"
#include "shipsim_tree_host.hpp"

namespace TR = tree_host;

static_assert(TR::kMaxNodes == SHIPSIM_ARCHIVE_MAX_CELLS && TR::kMaxChildren == SHIPSIM_TREE_MAX_CHILDREN &&
                  TR::kMaxDepth == SHIPSIM_TREE_MAX_DEPTH && TR::kMaxWorkers == SHIPSIM_TREE_MAX_WORKERS &&
                  TR::kScanTile == SHIPSIM_TREE_SCAN_TILE && TR::kLayoutFields == SHIPSIM_TREE_LAYOUT_FIELDS,
              "shipsim.h and shipsim_tree_host.hpp name the same numbers");

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kPerThread = TR::kScanTile / kThreads;  // consecutive counts per thread of the scan
constexpr int kLevelMaxBlocks = 1024;                 // the waves of a level stride over its frontier
static_assert(kPerThread * kThreads == TR::kScanTile && TR::kMaxTiles % kThreads == 0, "the tiles divide evenly");

__global__ void tr_init_kernel(const TR::Tree T) {
  if (blockIdx.x == 0 && threadIdx.x == 0) TR::init(T);
}

__global__ __launch_bounds__(kThreads) void tr_clear_kernel(const TR::Tree T, int32_t n_workers, int32_t* __restrict__ stay,
                                                            int32_t* __restrict__ newc, int32_t* __restrict__ level_count,
                                                            int32_t* __restrict__ fnode, int32_t* __restrict__ fcnt) {
  const uint32_t n = TR::node_count(T.hdr[TR::kHdrNodes], T.M);
  const uint32_t v = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (v < (uint32_t)(TR::kMaxDepth + 2)) level_count[v] = (v == 0 && n) ? 1 : 0;
  if (v == 0) {
    fnode[0] = 0;
    fcnt[0] = n_workers;
  }
  if (v < n) {
    stay[v] = 0;
    newc[v] = 0;
  }
}

// largest of x over the wave's 64 lanes, in every lane
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

__device__ __forceinline__ int64_t wave_sum(int64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += (int64_t)__shfl_xor((long long)x, o, 64);
  return x;
}

// One wave per node of the level's frontier. Lane l holds child slot l: its id, its visits and its mean value, read
// once, and the workers sent to it so far. The node, its arrivals and every count that steers the loop are the same
// in all 64 lanes, so every lane runs every cross-lane move.
__global__ __launch_bounds__(kThreads) void tr_level_kernel(const TR::Tree T, int level, int32_t max_depth, int32_t wnum,
                                                            int32_t wden, double c_explore, int32_t n_workers,
                                                            const int32_t* __restrict__ fnode,
                                                            const int32_t* __restrict__ fcnt, int32_t* __restrict__ next_node,
                                                            int32_t* __restrict__ next_cnt, int32_t* level_count,
                                                            int32_t* __restrict__ stay, int32_t* __restrict__ newc) {
  const int lane = threadIdx.x & 63;
  const uint32_t n = TR::node_count(T.hdr[TR::kHdrNodes], T.M);
  const int32_t n_front = TR::clamp_count(level_count[level], n_workers);  // a frontier holds at most W nodes
  const int32_t waves = (int32_t)gridDim.x * kWavesPerBlock;
  const int32_t C = T.C;
  for (int32_t i = (int32_t)blockIdx.x * kWavesPerBlock + ((int32_t)threadIdx.x >> 6); i < n_front; i += waves) {
    const int32_t v = __builtin_amdgcn_readfirstlane(fnode[i]);
    const int32_t A = TR::clamp_count(__builtin_amdgcn_readfirstlane(fcnt[i]), n_workers);
    if (!TR::index_ok(v, n)) continue;
    int32_t st = 0, nw = 0, arrived = 0, a = -1, va = 0;
    double q = 0.0;
    bool cand = false;
    const int32_t nc = TR::clamp_count(T.n_children[v], C);
    if ((T.flags[v] & TR::kTerminal) || T.depth[v] >= max_depth) {
      st = A;
    } else {
      if (lane < nc) {
        a = T.child[(int64_t)v * C + lane];
        if (TR::index_ok(a, n)) {
          cand = true;
          va = T.visits[a];
          q = TR::q_of(va, T.value_sum[a]);
        }
      }
      const bool any = __ballot(cand) != 0ull;
      const int64_t N0 = T.visits[v];
      for (int32_t t = 0; t < A; ++t) {
        const int64_t N = N0 + t;
        if (TR::widens(nc + nw, C, wnum, wden, N)) {
          ++nw;
        } else if (!any) {
          ++st;
        } else {
          const double s = cand ? TR::score(q, c_explore, N, va, arrived) : -__builtin_huge_val();
          const double top = wave_max(s);
          const unsigned long long holds = __ballot(cand && s == top);
          if (!holds) ++st;  // (no score compares equal to the largest: none is a number)
          else if (lane == __ffsll(holds) - 1) ++arrived;
        }
      }
    }
    if (lane == 0) {
      stay[v] = st;
      newc[v] = nw;
    }
    const unsigned long long sent = __ballot(arrived > 0);
    if (sent && level < TR::kMaxDepth) {
      int32_t base = 0;
      if (lane == 0) base = atomicAdd(&level_count[level + 1], (int32_t)__popcll(sent));
      base = __shfl(base, 0, 64);
      const int32_t pos = base + (int32_t)__popcll(sent & ((1ull << lane) - 1ull));
      if (arrived > 0 && TR::index_ok(pos, (uint32_t)n_workers)) {
        next_node[pos] = a;
        next_cnt[pos] = arrived;
      }
    }
  }
}

// ---- the scan: a tile of kScanTile counts per block, kPerThread consecutive ones per thread ----
// kNodes: the count of node i is stay[i] + newc[i], over the tree's nodes; else the count of worker i is whether it
// has a child slot (x[i] >= 0), over n_given workers.
template <bool kNodes>
__device__ __forceinline__ int32_t scan_n(const TR::Tree& T, int32_t n_given) {
  return kNodes ? (int32_t)TR::node_count(T.hdr[TR::kHdrNodes], T.M) : n_given;
}
template <bool kNodes>
__device__ __forceinline__ int32_t scan_count(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int32_t i) {
  return kNodes ? x[i] + y[i] : (x[i] >= 0 ? 1 : 0);
}

// the sum of v over the block, in every thread (red: kWavesPerBlock ints of LDS)
__device__ __forceinline__ int32_t block_sum(int32_t v, int32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kWavesPerBlock; ++k) s += red[k];
  return s;
}

// the sum of v over the threads of the block before this one (red: kWavesPerBlock ints of LDS)
__device__ __forceinline__ int32_t block_exclusive(int32_t v, int32_t* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int32_t before = 0;
#pragma unroll
  for (int k = 0; k < kWavesPerBlock; ++k)
    if (k < wave) before += red[k];
  return before + inc - v;
}

template <bool kNodes>
__global__ __launch_bounds__(kThreads) void tr_tile_kernel(const TR::Tree T, int32_t n_given, const int32_t* __restrict__ x,
                                                           const int32_t* __restrict__ y, int32_t* __restrict__ tile_sum) {
  __shared__ int32_t red[kWavesPerBlock];
  const int32_t n = scan_n<kNodes>(T, n_given);
  const int32_t first = (int32_t)blockIdx.x * TR::kScanTile + (int32_t)threadIdx.x * kPerThread;
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k)
    if (first + k < n) s += scan_count<kNodes>(x, y, first + k);
  s = block_sum(s, red);
  if (threadIdx.x == 0 && blockIdx.x < (unsigned)TR::kMaxTiles) tile_sum[blockIdx.x] = s;
}

// the counts before this block's tile (every earlier tile's sum) plus those before this thread inside it
template <bool kNodes>
__device__ __forceinline__ int32_t scan_before(const int32_t* __restrict__ x, const int32_t* __restrict__ y, int32_t n,
                                               const int32_t* __restrict__ tile_sum, int32_t* red, int32_t c[kPerThread]) {
  const int32_t tiles = blockIdx.x < (unsigned)TR::kMaxTiles ? (int32_t)blockIdx.x : TR::kMaxTiles;
  int32_t earlier = 0;
  for (int32_t k = (int32_t)threadIdx.x; k < tiles; k += kThreads) earlier += tile_sum[k];  // (at most 16 rounds)
  earlier = block_sum(earlier, red);
  const int32_t first = (int32_t)blockIdx.x * TR::kScanTile + (int32_t)threadIdx.x * kPerThread;
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    c[k] = first + k < n ? scan_count<kNodes>(x, y, first + k) : 0;
    s += c[k];
  }
  return earlier + block_exclusive(s, red);
}

__global__ __launch_bounds__(kThreads) void tr_offset_kernel(const TR::Tree T, const int32_t* __restrict__ stay,
                                                             const int32_t* __restrict__ newc,
                                                             const int32_t* __restrict__ tile_sum, int32_t* __restrict__ off) {
  __shared__ int32_t red[kWavesPerBlock];
  const int32_t n = scan_n<true>(T, 0);
  if ((int64_t)blockIdx.x * TR::kScanTile >= n) return;  // (the whole block)
  int32_t c[kPerThread];
  int32_t o = scan_before<true>(stay, newc, n, tile_sum, red, c);
  const int32_t first = (int32_t)blockIdx.x * TR::kScanTile + (int32_t)threadIdx.x * kPerThread;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    if (first + k < n) off[first + k] = o;
    o += c[k];
  }
}

// Worker w belongs to the last node v with off[v] <= w (the nodes after it up to the next count are empty): found by
// bisection over [0, n), at most 23 halvings. Among a node's workers the staying ones come first.
__global__ __launch_bounds__(kThreads) void tr_leaf_kernel(const TR::Tree T, int32_t n_workers, const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ stay, const int32_t* __restrict__ newc,
                                                           int32_t* __restrict__ leaf_out, int32_t* __restrict__ expand_out) {
  const int32_t w = (int32_t)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
  if (w >= n_workers) return;
  const int32_t n = (int32_t)TR::node_count(T.hdr[TR::kHdrNodes], T.M);
  int32_t leaf = -1, widen = 0;
  if (n > 0) {
    int32_t lo = 0, hi = n;  // off[lo] <= w (off[0] = 0), and off[hi] > w or hi == n
    for (int it = 0; it < 24 && hi - lo > 1; ++it) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (off[mid] <= w) lo = mid;
      else hi = mid;
    }
    const int32_t k = w - off[lo], s = stay[lo];
    if (k >= 0 && k < s + newc[lo]) {
      leaf = lo;
      widen = k >= s;
    }
  }
  leaf_out[w] = leaf;
  expand_out[w] = widen;
}

__global__ __launch_bounds__(kThreads) void tr_slot_kernel(const TR::Tree T, int32_t n_workers, const int32_t* __restrict__ leaf,
                                                           const int32_t* __restrict__ expand, int32_t* __restrict__ slot) {
  const int32_t w = (int32_t)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
  if (w >= n_workers) return;
  slot[w] = TR::slot_of(T, TR::node_count(T.hdr[TR::kHdrNodes], T.M), leaf, expand, w);
}

// (reads n_nodes, which tr_count_kernel advances after this launch; a parent's n_children was read by tr_slot_kernel
// in the launch before, so the adds here race with no read)
__global__ __launch_bounds__(kThreads) void tr_expand_kernel(const TR::Tree T, int32_t n_workers, const int32_t* __restrict__ leaf,
                                                             const int32_t* __restrict__ expand,
                                                             const float* __restrict__ action, const int32_t* __restrict__ slot,
                                                             const int32_t* __restrict__ tile_sum, int32_t* __restrict__ node_out) {
  __shared__ int32_t red[kWavesPerBlock];
  const uint32_t n = TR::node_count(T.hdr[TR::kHdrNodes], T.M);
  int32_t c[kPerThread];
  int32_t rank = scan_before<false>(slot, nullptr, n_workers, tile_sum, red, c);
  const int32_t first = (int32_t)blockIdx.x * TR::kScanTile + (int32_t)threadIdx.x * kPerThread;
  int32_t dropped = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int32_t w = first + k;
    if (w >= n_workers) break;
    if (!expand[w]) {
      node_out[w] = leaf[w];
      continue;
    }
    const int64_t id = (int64_t)n + rank;
    rank += c[k];
    const int32_t v = leaf[w], s = slot[w];
    // (a slot >= 0 says that v is a node and s < C: TR::slot_of)
    if (s < 0 || n == 0 || id >= T.M || !TR::index_ok(v, n)) {
      node_out[w] = -1;
      ++dropped;
      continue;
    }
    TR::fill_node(T, (int32_t)id, v, s, action[w]);
    atomicAdd(&T.n_children[v], 1);
    node_out[w] = (int32_t)id;
  }
  dropped = block_sum(dropped, red);
  if (threadIdx.x == 0 && dropped) atomicAdd(&T.hdr[TR::kHdrDropped], dropped);
}

__global__ __launch_bounds__(kThreads) void tr_count_kernel(const TR::Tree T, int32_t n_tiles, const int32_t* __restrict__ tile_sum) {
  __shared__ int32_t red[kWavesPerBlock];
  int32_t s = 0;
  for (int32_t k = (int32_t)threadIdx.x; k < n_tiles && k < TR::kMaxTiles; k += kThreads) s += tile_sum[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const uint32_t n = TR::node_count(T.hdr[TR::kHdrNodes], T.M);
    if (n) {
      const int64_t grown = (int64_t)n + s;
      T.hdr[TR::kHdrNodes] = grown > T.M ? T.M : (int32_t)grown;
    }
  }
}

__global__ __launch_bounds__(kThreads) void tr_backup_kernel(const TR::Tree T, int32_t n_workers, const int32_t* __restrict__ node,
                                                             const double* __restrict__ value,
                                                             const uint8_t* __restrict__ terminal) {
  const int32_t w = (int32_t)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
  const uint32_t n = TR::node_count(T.hdr[TR::kHdrNodes], T.M);
  bool taken = false, at_root = false;
  int64_t q = 0;
  if (w < n_workers) {
    int32_t v = node[w];
    const double x = value[w];
    taken = TR::backup_ok(v, n, x);
    if (taken) {
      q = TR::quantize(x);
      if (terminal && terminal[w]) atomicOr(&T.flags[v], TR::kTerminal);
      for (int step = 0; step <= TR::kMaxDepth && TR::index_ok(v, n); ++step) {
        if (v == 0) {
          at_root = true;
          break;
        }
        atomicAdd(&T.visits[v], 1);
        atomicAdd((unsigned long long*)&T.value_sum[v], (unsigned long long)q);
        v = T.parent[v];
      }
    }
  }
  // every lane of the wave is here: the root's adds and the skipped count go out once per wave
  const unsigned long long root_mask = __ballot(at_root);
  const int64_t root_q = wave_sum(at_root ? q : 0);
  const unsigned long long skip_mask = __ballot(w < n_workers && !taken);
  if ((threadIdx.x & 63) == 0) {
    if (root_mask) {
      atomicAdd(&T.visits[0], (int32_t)__popcll(root_mask));
      atomicAdd((unsigned long long*)&T.value_sum[0], (unsigned long long)root_q);
    }
    if (skip_mask) atomicAdd(&T.hdr[TR::kHdrSkipped], (int32_t)__popcll(skip_mask));
  }
}

// ---- the forest: R roots in one pool (shipsim_tree_init_forest / _select_forest) ----
//   tr_init_forest_kernel  [R / 256]   the header and root r per thread
//   select_forest: as select, with two launches in the place of tr_clear_kernel and level 0 as wide as the roots
//   tr_roots_tile_kernel   [R / 1024]  the sum, saturating at W, of a tile of root_workers (clamped to 0..W)
//   tr_clear_forest_kernel [max_nodes / 1024]  stay = newc = 0; the level counts; root r as entry r of level
//                                      0's frontier with a_r arrivals: the tiles before (saturating), then an exclusive
//                                      saturating scan inside the tile
// Every term of the prefix is in 0..W and every add saturates at W <= 2^22, so no int32 overflows whatever
// root_workers holds, and the adds being associative, the scan's order does not show.
__global__ __launch_bounds__(kThreads) void tr_init_forest_kernel(const TR::Tree T, int32_t n_roots) {
  const int32_t r = (int32_t)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
  if (r == 0) TR::init_forest_header(T, n_roots);
  if (r < n_roots && r < T.M) TR::init_root(T, r);
}

// the saturating sum of v (0..W) over the block, in every thread (red: kWavesPerBlock ints of LDS)
__device__ __forceinline__ int32_t block_sum_sat(int32_t v, int32_t W, int32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = TR::sat_add(v, __shfl_xor(v, o, 64), W);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kWavesPerBlock; ++k) s = TR::sat_add(s, red[k], W);
  return s;
}

// the saturating sum of v (0..W) over the threads of the block before this one (red: kWavesPerBlock ints of LDS)
__device__ __forceinline__ int32_t block_exclusive_sat(int32_t v, int32_t W, int32_t* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc = TR::sat_add(y, inc, W);
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int32_t before = 0;
#pragma unroll
  for (int k = 0; k < kWavesPerBlock; ++k)
    if (k < wave) before = TR::sat_add(before, red[k], W);
  const int32_t prev = __shfl_up(inc, 1, 64);  // (the inclusive sum of the lane before: saturating adds have no inverse)
  return lane ? TR::sat_add(before, prev, W) : before;
}

// the roots this call serves: the same number in every kernel of the call
__device__ __forceinline__ int32_t forest_roots(const TR::Tree& T, int32_t n_roots) {
  return TR::root_count(n_roots, T.hdr[TR::kHdrRoots], TR::node_count(T.hdr[TR::kHdrNodes], T.M));
}

__global__ __launch_bounds__(kThreads) void tr_roots_tile_kernel(const TR::Tree T, int32_t n_workers, int32_t n_roots,
                                                                 const int32_t* __restrict__ root_workers,
                                                                 int32_t* __restrict__ tile_sum) {
  __shared__ int32_t red[kWavesPerBlock];
  const int32_t R = forest_roots(T, n_roots);  // (<= n_roots, the entries root_workers has)
  const int32_t first = (int32_t)blockIdx.x * TR::kScanTile + (int32_t)threadIdx.x * kPerThread;
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k)
    if (first + k < R) s = TR::sat_add(s, TR::root_ask(root_workers[first + k], n_workers), n_workers);
  s = block_sum_sat(s, n_workers, red);
  if (threadIdx.x == 0 && blockIdx.x < (unsigned)TR::kMaxTiles) tile_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void tr_clear_forest_kernel(const TR::Tree T, int32_t n_workers, int32_t n_roots,
                                                                   const int32_t* __restrict__ root_workers,
                                                                   const int32_t* __restrict__ tile_sum,
                                                                   int32_t* __restrict__ stay, int32_t* __restrict__ newc,
                                                                   int32_t* __restrict__ level_count,
                                                                   int32_t* __restrict__ fnode, int32_t* __restrict__ fcnt) {
  __shared__ int32_t red[kWavesPerBlock];
  const uint32_t n = TR::node_count(T.hdr[TR::kHdrNodes], T.M);
  const int32_t R = forest_roots(T, n_roots), W = n_workers;  // (R <= n_roots <= W: the frontier's entries)
  const int32_t first = (int32_t)blockIdx.x * TR::kScanTile + (int32_t)threadIdx.x * kPerThread;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const uint32_t v = (uint32_t)(first + k);
    if (v < (uint32_t)(TR::kMaxDepth + 2)) level_count[v] = v == 0 ? R : 0;
    if (v < n) {
      stay[v] = 0;
      newc[v] = 0;
    }
  }
  if ((int64_t)blockIdx.x * TR::kScanTile >= n_roots) return;  // (the whole block: a host argument)
  const int32_t tiles = blockIdx.x < (unsigned)TR::kMaxTiles ? (int32_t)blockIdx.x : TR::kMaxTiles;
  int32_t earlier = 0;
  for (int32_t k = (int32_t)threadIdx.x; k < tiles; k += kThreads) earlier = TR::sat_add(earlier, TR::clamp_count(tile_sum[k], W), W);
  earlier = block_sum_sat(earlier, W, red);  // (at most 16 rounds)
  int32_t c[kPerThread];
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    c[k] = first + k < R ? root_workers[first + k] : 0;
    s = TR::sat_add(s, TR::root_ask(c[k], W), W);
  }
  int32_t before = TR::sat_add(earlier, block_exclusive_sat(s, W, red), W);
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    if (first + k < R) {
      fnode[first + k] = first + k;
      fcnt[first + k] = TR::root_arrival(c[k], before, W);
    }
    before = TR::sat_add(before, TR::root_ask(c[k], W), W);
  }
}

inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

extern "C" {

int64_t shipsim_tree_bytes(int32_t max_nodes, int32_t max_children) {
  if (!TR::sizes_ok(max_nodes, max_children)) return SHIPSIM_EINVAL;
  return TR::layout(max_nodes, max_children).bytes;
}

int shipsim_tree_layout(int32_t max_nodes, int32_t max_children, int64_t* offsets_out) {
  if (!TR::sizes_ok(max_nodes, max_children) || !offsets_out) return SHIPSIM_EINVAL;
  const TR::Layout L = TR::layout(max_nodes, max_children);
  const int64_t o[TR::kLayoutFields] = {L.header, L.parent, L.depth,  L.n_children, L.child,
                                        L.visits, L.value_sum, L.action, L.flags,   L.bytes};
  for (int i = 0; i < TR::kLayoutFields; ++i) offsets_out[i] = o[i];
  return SHIPSIM_OK;
}

int64_t shipsim_tree_workspace_bytes(int32_t max_nodes, int32_t n_workers) {
  if (max_nodes < 1 || max_nodes > TR::kMaxNodes || !TR::workers_ok(n_workers)) return SHIPSIM_EINVAL;
  return TR::ws_layout(max_nodes, n_workers).bytes;
}

int shipsim_tree_init(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, void* stream) {
  if (!TR::tree_args_ok(tree, tree_bytes, max_nodes, max_children)) return SHIPSIM_EINVAL;
  hipLaunchKernelGGL(tr_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, TR::view(tree, max_nodes, max_children));
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_tree_select(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_workers,
                        int32_t max_depth, int32_t wnum, int32_t wden, double c_explore, void* workspace,
                        int64_t workspace_bytes, int32_t* leaf_out, int32_t* expand_out, void* stream) {
  if (!TR::select_args_ok(tree, tree_bytes, max_nodes, max_children, n_workers, max_depth, wnum, wden, c_explore,
                          workspace, workspace_bytes, leaf_out, expand_out))
    return SHIPSIM_EINVAL;
  const TR::Tree T = TR::view((void*)tree, max_nodes, max_children);  // (select writes nothing through it)
  const TR::Workspace S = TR::ws_view(workspace, max_nodes, n_workers);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(kThreads);
  const int32_t clear_n = max_nodes > TR::kMaxDepth + 2 ? max_nodes : TR::kMaxDepth + 2;
  hipLaunchKernelGGL(tr_clear_kernel, dim3(blocks_for(clear_n, kThreads)), block, 0, st, T, n_workers, S.stay, S.newc,
                     S.level_count, S.fnode[0], S.fcnt[0]);
  // level d holds at most min(W, max_nodes, C^d) nodes
  const int64_t most = n_workers < max_nodes ? n_workers : max_nodes;
  int64_t width = 1;
  for (int d = 0; d <= max_depth; ++d) {
    unsigned blocks = blocks_for(width, kWavesPerBlock);
    if (blocks > (unsigned)kLevelMaxBlocks) blocks = kLevelMaxBlocks;
    hipLaunchKernelGGL(tr_level_kernel, dim3(blocks), block, 0, st, T, d, max_depth, wnum, wden, c_explore, n_workers,
                       S.fnode[d & 1], S.fcnt[d & 1], S.fnode[(d + 1) & 1], S.fcnt[(d + 1) & 1], S.level_count, S.stay,
                       S.newc);
    width = width * max_children < most ? width * max_children : most;
  }
  const dim3 tiles(blocks_for(max_nodes, TR::kScanTile));
  hipLaunchKernelGGL(tr_tile_kernel<true>, tiles, block, 0, st, T, 0, S.stay, S.newc, S.tile_sum);
  hipLaunchKernelGGL(tr_offset_kernel, tiles, block, 0, st, T, S.stay, S.newc, S.tile_sum, S.off);
  hipLaunchKernelGGL(tr_leaf_kernel, dim3(blocks_for(n_workers, kThreads)), block, 0, st, T, n_workers, S.off, S.stay,
                     S.newc, leaf_out, expand_out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_tree_expand(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_workers,
                        const int32_t* leaf, const int32_t* expand, const float* action, void* workspace,
                        int64_t workspace_bytes, int32_t* node_out, void* stream) {
  if (!TR::expand_args_ok(tree, tree_bytes, max_nodes, max_children, n_workers, leaf, expand, action, workspace,
                          workspace_bytes, node_out))
    return SHIPSIM_EINVAL;
  const TR::Tree T = TR::view(tree, max_nodes, max_children);
  const TR::Workspace S = TR::ws_view(workspace, max_nodes, n_workers);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(kThreads), tiles(blocks_for(n_workers, TR::kScanTile));
  hipLaunchKernelGGL(tr_slot_kernel, dim3(blocks_for(n_workers, kThreads)), block, 0, st, T, n_workers, leaf, expand, S.slot);
  hipLaunchKernelGGL(tr_tile_kernel<false>, tiles, block, 0, st, T, n_workers, S.slot, (const int32_t*)nullptr, S.tile_sum);
  hipLaunchKernelGGL(tr_expand_kernel, tiles, block, 0, st, T, n_workers, leaf, expand, action, S.slot, S.tile_sum, node_out);
  hipLaunchKernelGGL(tr_count_kernel, dim3(1), block, 0, st, T, (int32_t)tiles.x, S.tile_sum);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_tree_backup(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_workers,
                        const int32_t* node, const double* value, const uint8_t* terminal, void* stream) {
  if (!TR::backup_args_ok(tree, tree_bytes, max_nodes, max_children, n_workers, node, value)) return SHIPSIM_EINVAL;
  const TR::Tree T = TR::view(tree, max_nodes, max_children);
  hipLaunchKernelGGL(tr_backup_kernel, dim3(blocks_for(n_workers, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, T,
                     n_workers, node, value, terminal);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_tree_init_forest(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_roots,
                             void* stream) {
  if (!TR::forest_init_args_ok(tree, tree_bytes, max_nodes, max_children, n_roots)) return SHIPSIM_EINVAL;
  hipLaunchKernelGGL(tr_init_forest_kernel, dim3(blocks_for(n_roots, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     TR::view(tree, max_nodes, max_children), n_roots);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_tree_select_forest(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                               int32_t n_workers, int32_t n_roots, const int32_t* root_workers, int32_t max_depth,
                               int32_t wnum, int32_t wden, double c_explore, void* workspace, int64_t workspace_bytes,
                               int32_t* leaf_out, int32_t* expand_out, void* stream) {
  if (!TR::forest_select_args_ok(tree, tree_bytes, max_nodes, max_children, n_workers, n_roots, root_workers, max_depth,
                                 wnum, wden, c_explore, workspace, workspace_bytes, leaf_out, expand_out))
    return SHIPSIM_EINVAL;
  const TR::Tree T = TR::view((void*)tree, max_nodes, max_children);  // (select writes nothing through it)
  const TR::Workspace S = TR::ws_view(workspace, max_nodes, n_workers);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(kThreads);
  hipLaunchKernelGGL(tr_roots_tile_kernel, dim3(blocks_for(n_roots, TR::kScanTile)), block, 0, st, T, n_workers, n_roots,
                     root_workers, S.tile_sum);
  const int32_t clear_n = max_nodes > TR::kMaxDepth + 2 ? max_nodes : TR::kMaxDepth + 2;  // (n_roots <= max_nodes)
  hipLaunchKernelGGL(tr_clear_forest_kernel, dim3(blocks_for(clear_n, TR::kScanTile)), block, 0, st, T, n_workers, n_roots,
                     root_workers, S.tile_sum, S.stay, S.newc, S.level_count, S.fnode[0], S.fcnt[0]);
  // level d holds at most min(W, max_nodes, R * C^d) nodes
  const int64_t most = n_workers < max_nodes ? n_workers : max_nodes;
  int64_t width = n_roots;
  for (int d = 0; d <= max_depth; ++d) {
    unsigned blocks = blocks_for(width, kWavesPerBlock);
    if (blocks > (unsigned)kLevelMaxBlocks) blocks = kLevelMaxBlocks;
    hipLaunchKernelGGL(tr_level_kernel, dim3(blocks), block, 0, st, T, d, max_depth, wnum, wden, c_explore, n_workers,
                       S.fnode[d & 1], S.fcnt[d & 1], S.fnode[(d + 1) & 1], S.fcnt[(d + 1) & 1], S.level_count, S.stay,
                       S.newc);
    width = width * max_children < most ? width * max_children : most;
  }
  const dim3 tiles(blocks_for(max_nodes, TR::kScanTile));
  hipLaunchKernelGGL(tr_tile_kernel<true>, tiles, block, 0, st, T, 0, S.stay, S.newc, S.tile_sum);
  hipLaunchKernelGGL(tr_offset_kernel, tiles, block, 0, st, T, S.stay, S.newc, S.tile_sum, S.off);
  hipLaunchKernelGGL(tr_leaf_kernel, dim3(blocks_for(n_workers, kThreads)), block, 0, st, T, n_workers, S.off, S.stay,
                     S.newc, leaf_out, expand_out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

}  // extern "C"
