// shipsim_tree_host.hpp — the host half of the search tree (include/shipsim.h: shipsim_tree_init / _select / _expand /
// _backup): the tree buffer and the workspace as tables of offsets, the argument checks, the arithmetic of the three
// operations (the widening rule, the score, the fixed-point image of a value) and the operations themselves restated
// on the host, one worker or one node after the other. Free of the device (plain C++17), so that it can be compiled
// and driven on its own: tests/test_tree_cpu.py builds it into a stand-alone program (tests/tree_host_check.cpp) with
// -fsanitize=address,undefined. The kernels of shipsim_tree.hip call the same functions, so GPU, host program and the
// Python restatement (tests/tree_ref.py) agree bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TR_HD __host__ __device__
#else
#define TR_HD
#endif

namespace tree_host {

constexpr int32_t kMaxNodes = 1 << 22;    // SHIPSIM_ARCHIVE_MAX_CELLS: a node id is an archive cell id
constexpr int32_t kMaxChildren = 64;      // SHIPSIM_TREE_MAX_CHILDREN: one child per lane of a wave
constexpr int32_t kMaxDepth = 32;         // SHIPSIM_TREE_MAX_DEPTH
constexpr int32_t kMaxWorkers = 1 << 22;  // SHIPSIM_TREE_MAX_WORKERS
constexpr int32_t kMaxWiden = 1 << 15;    // wnum and wden: m * m * wden stays under 2^27
constexpr int32_t kScanTile = 1024;       // nodes (select) or workers (expand) numbered by one block of the scan
constexpr int32_t kMaxTiles = kMaxNodes / kScanTile;
constexpr int kFracBits = 24;                   // a value is kept as round(value * 2^24)
constexpr int64_t kQClamp = (int64_t)1 << 40;   // ... within +-2^40: 2^22 workers cannot overflow a sum in one call
static_assert(kMaxWorkers == kMaxNodes && kMaxTiles * kScanTile == kMaxNodes, "one tile count serves both scans");

// ---- the tree buffer: structure of arrays, every array on a multiple of 256 bytes ----
//   header     int32[4]: n_nodes, dropped (new nodes the pool had no room for), skipped (backups not taken), 0
//   parent     [M] int32 (-1: the root)          depth    [M] int32       n_children [M] int32
//   child      [M * C] int32, creation order     visits   [M] int32       value_sum  [M] int64 (fixed point, 24 bits)
//   action     [M] float32 (the edge from the parent)                     flags      [M] int32 (bit 0: terminal)
struct Layout {
  int64_t header, parent, depth, n_children, child, visits, value_sum, action, flags, bytes;
};
constexpr int kLayoutFields = 10;
enum Header { kHdrNodes = 0, kHdrDropped = 1, kHdrSkipped = 2, kHdrInts = 4 };
constexpr int32_t kTerminal = 1;

constexpr int64_t r256(int64_t b) { return (b + 255) & ~(int64_t)255; }
constexpr bool sizes_ok(int32_t max_nodes, int32_t max_children) {
  return max_nodes >= 1 && max_nodes <= kMaxNodes && max_children >= 1 && max_children <= kMaxChildren;
}
constexpr Layout layout(int32_t max_nodes, int32_t max_children) {
  Layout L{};
  const int64_t M = max_nodes, C = max_children;
  int64_t o = 0;
  L.header = o; o += r256(kHdrInts * 4);
  L.parent = o; o += r256(M * 4);
  L.depth = o; o += r256(M * 4);
  L.n_children = o; o += r256(M * 4);
  L.child = o; o += r256(M * C * 4);
  L.visits = o; o += r256(M * 4);
  L.value_sum = o; o += r256(M * 8);
  L.action = o; o += r256(M * 4);
  L.flags = o; o += r256(M * 4);
  L.bytes = o;
  return L;
}
static_assert(layout(1, 1).bytes == 9 * 256 && layout(kMaxNodes, kMaxChildren).bytes < ((int64_t)5 << 28),
              "the smallest tree is nine rows of 256 bytes, the largest under 1.25 GiB");

// the arrays of a tree buffer (no ownership)
struct Tree {
  int32_t *hdr, *parent, *depth, *n_children, *child, *visits;
  int64_t* value_sum;
  float* action;
  int32_t* flags;
  int32_t M, C;
};
inline Tree view(void* base, int32_t max_nodes, int32_t max_children) {
  const Layout L = layout(max_nodes, max_children);
  char* p = (char*)base;
  Tree T;
  T.hdr = (int32_t*)(p + L.header);
  T.parent = (int32_t*)(p + L.parent);
  T.depth = (int32_t*)(p + L.depth);
  T.n_children = (int32_t*)(p + L.n_children);
  T.child = (int32_t*)(p + L.child);
  T.visits = (int32_t*)(p + L.visits);
  T.value_sum = (int64_t*)(p + L.value_sum);
  T.action = (float*)(p + L.action);
  T.flags = (int32_t*)(p + L.flags);
  T.M = max_nodes;
  T.C = max_children;
  return T;
}

// ---- the workspace: what the launches of one call hand one another ----
//   stay, newc [M] int32: the workers that stay at a node, the children being created there
//   off        [M] int32: the exclusive scan of stay + newc over the nodes (select's output order)
//   slot       [W] int32: the child slot a widening worker fills, -1 for every other worker (expand)
//   fnode, fcnt 2 x [W] int32: the frontier of a level, nodes with arrivals and their counts, and the next level's
//   level_count [kMaxDepth + 2] int32: the length of each level's frontier
//   tile_sum   [kMaxTiles] int32: the scan's sums per tile
struct WsLayout {
  int64_t stay, newc, off, slot, fnode[2], fcnt[2], level_count, tile_sum, bytes;
};
constexpr WsLayout ws_layout(int32_t max_nodes, int32_t n_workers) {
  WsLayout L{};
  const int64_t M = max_nodes, W = n_workers;
  int64_t o = 0;
  L.stay = o; o += r256(M * 4);
  L.newc = o; o += r256(M * 4);
  L.off = o; o += r256(M * 4);
  L.slot = o; o += r256(W * 4);
  for (int i = 0; i < 2; ++i) {
    L.fnode[i] = o; o += r256(W * 4);
    L.fcnt[i] = o; o += r256(W * 4);
  }
  L.level_count = o; o += r256((kMaxDepth + 2) * 4);
  L.tile_sum = o; o += r256((int64_t)kMaxTiles * 4);
  L.bytes = o;
  return L;
}
static_assert(ws_layout(1, 1).bytes <= ws_layout(2, 1).bytes && ws_layout(1, 1).bytes <= ws_layout(1, 2).bytes &&
                  ws_layout(64, 64).bytes < ws_layout(65, 64).bytes && ws_layout(64, 64).bytes < ws_layout(64, 65).bytes &&
                  ws_layout(kMaxNodes, kMaxWorkers).bytes < ((int64_t)1 << 28),
              "the workspace does not decrease in either argument and stays under 256 MiB");

struct Workspace {
  int32_t *stay, *newc, *off, *slot, *fnode[2], *fcnt[2], *level_count, *tile_sum;
};
inline Workspace ws_view(void* base, int32_t max_nodes, int32_t n_workers) {
  const WsLayout L = ws_layout(max_nodes, n_workers);
  char* p = (char*)base;
  Workspace S;
  S.stay = (int32_t*)(p + L.stay);
  S.newc = (int32_t*)(p + L.newc);
  S.off = (int32_t*)(p + L.off);
  S.slot = (int32_t*)(p + L.slot);
  for (int i = 0; i < 2; ++i) {
    S.fnode[i] = (int32_t*)(p + L.fnode[i]);
    S.fcnt[i] = (int32_t*)(p + L.fcnt[i]);
  }
  S.level_count = (int32_t*)(p + L.level_count);
  S.tile_sum = (int32_t*)(p + L.tile_sum);
  return S;
}

// ---- what the calls refuse before any device call ----
inline bool tree_args_ok(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children) {
  if (!tree || !sizes_ok(max_nodes, max_children)) return false;
  return tree_bytes == layout(max_nodes, max_children).bytes && !((uintptr_t)tree & 15);
}
constexpr bool workers_ok(int32_t n_workers) { return n_workers >= 1 && n_workers <= kMaxWorkers; }
inline bool ws_args_ok(const void* workspace, int64_t workspace_bytes, int32_t max_nodes, int32_t n_workers) {
  return workspace && !((uintptr_t)workspace & 15) && workspace_bytes >= ws_layout(max_nodes, n_workers).bytes;
}
inline bool select_args_ok(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                           int32_t n_workers, int32_t max_depth, int32_t wnum, int32_t wden, double c_explore,
                           const void* workspace, int64_t workspace_bytes, const void* leaf_out,
                           const void* expand_out) {
  if (!tree_args_ok(tree, tree_bytes, max_nodes, max_children) || !workers_ok(n_workers)) return false;
  if (max_depth < 0 || max_depth > kMaxDepth || wnum < 1 || wnum > kMaxWiden || wden < 1 || wden > kMaxWiden) return false;
  if (!(c_explore >= 0.0) || !(c_explore <= 1.7976931348623157e308)) return false;  // negative, NaN or infinite
  return ws_args_ok(workspace, workspace_bytes, max_nodes, n_workers) && leaf_out && expand_out;
}
inline bool expand_args_ok(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                           int32_t n_workers, const void* leaf, const void* expand, const void* action,
                           const void* workspace, int64_t workspace_bytes, const void* node_out) {
  if (!tree_args_ok(tree, tree_bytes, max_nodes, max_children) || !workers_ok(n_workers)) return false;
  return leaf && expand && action && node_out && ws_args_ok(workspace, workspace_bytes, max_nodes, n_workers);
}
inline bool backup_args_ok(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                           int32_t n_workers, const void* node, const void* value) {
  return tree_args_ok(tree, tree_bytes, max_nodes, max_children) && workers_ok(n_workers) && node && value;
}

// ---- the arithmetic ----
// an index is served when it names a node of the tree: tested before any address is formed from it
TR_HD constexpr bool index_ok(int32_t index, uint32_t n) { return (uint32_t)index < n; }
// the header's node count as the bound every index is tested against (0 for a header that is not a tree's)
TR_HD constexpr uint32_t node_count(int32_t n_nodes, int32_t max_nodes) {
  return n_nodes >= 1 && n_nodes <= max_nodes ? (uint32_t)n_nodes : 0u;
}
TR_HD constexpr int32_t clamp_count(int32_t x, int32_t hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// A node with m children (those being created in this call included) and N visits (the virtual ones included) takes
// one more when m < C and m < k * sqrt(N + 1), k^2 = wnum / wden: in integers
TR_HD constexpr bool widens(int32_t m, int32_t C, int32_t wnum, int32_t wden, int64_t N) {
  return m < C && (uint64_t)m * (uint64_t)m * (uint64_t)wden < (uint64_t)wnum * (uint64_t)(N + 1);
}
// the mean value of a child: the fixed-point sum over the visits, scaled back (exact); 0 for an unvisited one
TR_HD inline double q_of(int32_t visits, int64_t value_sum) {
  return visits > 0 ? ldexp((double)value_sum / (double)visits, -kFracBits) : 0.0;
}
// the score of a child for the worker that sees N visits at the parent and `arrived` workers sent to the child before
// it: five IEEE operations in this order (the libraries are built without contraction)
TR_HD inline double score(double q, double c_explore, int64_t N, int32_t visits, int32_t arrived) {
  const double root = sqrt((double)(N + 1));
  const double num = c_explore * root;
  const double den = (double)((int64_t)1 + visits + arrived);
  const double bonus = num / den;
  return q + bonus;
}
TR_HD inline bool is_finite(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
// the fixed-point image of a finite value: round to nearest even, clamped
TR_HD inline int64_t quantize(double value) {
  const double x = nearbyint(ldexp(value, kFracBits));
  if (x >= (double)kQClamp) return kQClamp;
  if (x <= -(double)kQClamp) return -kQClamp;
  return (int64_t)x;
}
// a backup is taken when its node exists and its value is finite
TR_HD inline bool backup_ok(int32_t node, uint32_t n_nodes, double value) { return index_ok(node, n_nodes) && is_finite(value); }

// ---- the operations on the host ----
TR_HD inline void init(const Tree& T) {
  for (int i = 0; i < kHdrInts; ++i) T.hdr[i] = 0;
  T.hdr[kHdrNodes] = 1;
  T.parent[0] = -1;
  T.depth[0] = 0;
  T.n_children[0] = 0;
  T.visits[0] = 0;
  T.value_sum[0] = 0;
  T.action[0] = 0.0f;
  T.flags[0] = 0;
}

// What one node does with the A workers that arrive at it, one after the other: *stay and *newc, and arrived[l] for
// child slot l (C entries).
inline void route_node(const Tree& T, uint32_t n_nodes, int32_t v, int32_t A, int32_t max_depth, int32_t wnum,
                       int32_t wden, double c_explore, int32_t* stay, int32_t* newc, int32_t* arrived) {
  const int32_t C = T.C;
  for (int l = 0; l < C; ++l) arrived[l] = 0;
  *stay = 0;
  *newc = 0;
  if ((T.flags[v] & kTerminal) || T.depth[v] >= max_depth) {
    *stay = A;
    return;
  }
  const int32_t nc = clamp_count(T.n_children[v], C);
  const int64_t N0 = T.visits[v];
  for (int32_t t = 0; t < A; ++t) {
    const int64_t N = N0 + t;
    if (widens(nc + *newc, C, wnum, wden, N)) {
      *newc += 1;
      continue;
    }
    int best = -1;
    double best_score = 0.0;
    for (int l = 0; l < nc; ++l) {
      const int32_t a = T.child[(int64_t)v * C + l];
      if (!index_ok(a, n_nodes)) continue;
      const double s = score(q_of(T.visits[a], T.value_sum[a]), c_explore, N, T.visits[a], arrived[l]);
      if (best < 0 || s > best_score) {
        best = l;
        best_score = s;
      }
    }
    if (best < 0) *stay += 1;
    else arrived[best] += 1;
  }
}

// shipsim_tree_select on the host, in the stages of the launches: clear, the levels, the scan, the leaves
inline void select(const Tree& T, int32_t n_workers, int32_t max_depth, int32_t wnum, int32_t wden, double c_explore,
                   const Workspace& S, int32_t* leaf_out, int32_t* expand_out) {
  const uint32_t n = node_count(T.hdr[kHdrNodes], T.M);
  for (uint32_t v = 0; v < n; ++v) S.stay[v] = S.newc[v] = 0;
  for (int d = 0; d < kMaxDepth + 2; ++d) S.level_count[d] = 0;
  if (n) {
    S.level_count[0] = 1;
    S.fnode[0][0] = 0;
    S.fcnt[0][0] = n_workers;
  }
  int32_t arrived[kMaxChildren];
  for (int d = 0; d <= max_depth; ++d) {
    const int32_t* fn = S.fnode[d & 1];
    const int32_t* fc = S.fcnt[d & 1];
    int32_t* nn = S.fnode[(d + 1) & 1];
    int32_t* ncn = S.fcnt[(d + 1) & 1];
    for (int32_t i = 0; i < S.level_count[d]; ++i) {
      const int32_t v = fn[i];
      route_node(T, n, v, fc[i], max_depth, wnum, wden, c_explore, &S.stay[v], &S.newc[v], arrived);
      for (int l = 0; l < T.C; ++l)
        if (arrived[l] > 0) {
          const int32_t pos = S.level_count[d + 1]++;
          nn[pos] = T.child[(int64_t)v * T.C + l];
          ncn[pos] = arrived[l];
        }
    }
  }
  int32_t o = 0;
  for (uint32_t v = 0; v < n; ++v) {
    S.off[v] = o;
    o += S.stay[v] + S.newc[v];
  }
  for (int32_t w = 0; w < n_workers; ++w) {
    leaf_out[w] = -1;
    expand_out[w] = 0;
  }
  for (uint32_t v = 0; v < n; ++v)
    for (int32_t k = 0; k < S.stay[v] + S.newc[v]; ++k) {
      leaf_out[S.off[v] + k] = (int32_t)v;
      expand_out[S.off[v] + k] = k >= S.stay[v];
    }
}

// The child slot a widening worker fills, or -1. The widening workers of one node are adjacent, as select emits
// them: worker w's slot is the node's child count plus the run of such workers right before it (at most C - 1 are
// looked at). -1 for a worker that does not widen, names no node, names one at the depth limit or finds no free slot.
TR_HD inline int32_t slot_of(const Tree& T, uint32_t n_nodes, const int32_t* leaf, const int32_t* expand, int32_t w) {
  if (!expand[w]) return -1;
  const int32_t v = leaf[w];
  if (!index_ok(v, n_nodes) || T.depth[v] >= kMaxDepth) return -1;
  int32_t k = 0;
  while (k < T.C && w - k - 1 >= 0 && expand[w - k - 1] && leaf[w - k - 1] == v) ++k;
  const int32_t slot = clamp_count(T.n_children[v], T.C) + k;
  return slot < T.C ? slot : -1;
}
// the new node `id`, child `slot` of v (the parent's n_children is the caller's to advance)
TR_HD inline void fill_node(const Tree& T, int32_t id, int32_t v, int32_t slot, float action) {
  T.parent[id] = v;
  T.depth[id] = T.depth[v] + 1;
  T.n_children[id] = 0;
  T.visits[id] = 0;
  T.value_sum[id] = 0;
  T.action[id] = action;
  T.flags[id] = 0;
  T.child[(int64_t)v * T.C + slot] = id;
}

inline void expand(const Tree& T, int32_t n_workers, const int32_t* leaf, const int32_t* expand_in, const float* action,
                   const Workspace& S, int32_t* node_out) {
  const uint32_t n = node_count(T.hdr[kHdrNodes], T.M);
  for (int32_t w = 0; w < n_workers; ++w) S.slot[w] = slot_of(T, n, leaf, expand_in, w);
  int32_t rank = 0, made = 0;
  for (int32_t w = 0; w < n_workers; ++w) {
    if (!expand_in[w]) {
      node_out[w] = leaf[w];
      continue;
    }
    node_out[w] = -1;
    const int64_t id = (int64_t)n + rank;
    if (S.slot[w] >= 0) ++rank;
    if (S.slot[w] < 0 || n == 0 || id >= T.M) {
      T.hdr[kHdrDropped] = (int32_t)((uint32_t)T.hdr[kHdrDropped] + 1u);
      continue;
    }
    fill_node(T, (int32_t)id, leaf[w], S.slot[w], action[w]);
    T.n_children[leaf[w]] += 1;
    node_out[w] = (int32_t)id;
    ++made;
  }
  if (n) T.hdr[kHdrNodes] = (int32_t)n + made;
}

inline void backup(const Tree& T, int32_t n_workers, const int32_t* node, const double* value, const uint8_t* terminal) {
  const uint32_t n = node_count(T.hdr[kHdrNodes], T.M);
  for (int32_t w = 0; w < n_workers; ++w) {
    if (!backup_ok(node[w], n, value[w])) {
      T.hdr[kHdrSkipped] = (int32_t)((uint32_t)T.hdr[kHdrSkipped] + 1u);
      continue;
    }
    const int64_t q = quantize(value[w]);
    if (terminal && terminal[w]) T.flags[node[w]] |= kTerminal;
    int32_t v = node[w];
    for (int step = 0; step <= kMaxDepth && index_ok(v, n); ++step) {
      T.visits[v] = (int32_t)((uint32_t)T.visits[v] + 1u);
      T.value_sum[v] = (int64_t)((uint64_t)T.value_sum[v] + (uint64_t)q);
      v = T.parent[v];
    }
  }
}

// ---- the forest: R roots in one node pool (include/shipsim.h: shipsim_tree_init_forest / _select_forest) ----
// The header's fourth int is n_roots (0, as shipsim_tree_init writes it, reads as 1). Roots are nodes 0..R-1: parent
// -1, depth 0, action 0, no children. Everything under a root is a tree as above; expand and backup do not know roots.
constexpr int kHdrRoots = 3;

inline bool forest_init_args_ok(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                                int32_t n_roots) {
  return tree_args_ok(tree, tree_bytes, max_nodes, max_children) && n_roots >= 1 && n_roots <= max_nodes;
}
// the level-0 frontier lives in the W-entry frontier arrays: n_roots <= n_workers
inline bool forest_select_args_ok(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                                  int32_t n_workers, int32_t n_roots, const void* root_workers, int32_t max_depth,
                                  int32_t wnum, int32_t wden, double c_explore, const void* workspace,
                                  int64_t workspace_bytes, const void* leaf_out, const void* expand_out) {
  if (!select_args_ok(tree, tree_bytes, max_nodes, max_children, n_workers, max_depth, wnum, wden, c_explore, workspace,
                      workspace_bytes, leaf_out, expand_out))
    return false;
  return n_roots >= 1 && n_roots <= max_nodes && n_roots <= n_workers && root_workers;
}

// the roots a select serves: the caller's, the header's (0 reads as 1; a negative one as none) and the nodes there are
TR_HD constexpr int32_t root_count(int32_t n_roots, int32_t hdr_roots, uint32_t n_nodes) {
  const int32_t h = hdr_roots == 0 ? 1 : (hdr_roots < 0 ? 0 : hdr_roots);
  const int32_t r = n_roots < h ? n_roots : h;
  return r < 0 ? 0 : ((uint32_t)r < n_nodes ? r : (int32_t)n_nodes);
}
// a + b, at most W, for a and b in 0..W: associative, so any order of a scan gives the same prefix, and no int32
// overflows whatever the array holds
TR_HD constexpr int32_t sat_add(int32_t a, int32_t b, int32_t W) { return a >= W - b ? W : a + b; }
// what root_workers[r] asks for, as the prefix sees it
TR_HD constexpr int32_t root_ask(int32_t c, int32_t W) { return clamp_count(c, W); }
// the arrivals of a root that asks for c when the roots before it asked for `before` (saturated at W): the roots are
// served in id order until the W workers are used up
TR_HD constexpr int32_t root_arrival(int32_t c, int32_t before, int32_t W) {
  const int32_t ask = root_ask(c, W), left = W - clamp_count(before, W);
  return ask < left ? ask : left;
}

TR_HD inline void init_root(const Tree& T, int32_t r) {
  T.parent[r] = -1;
  T.depth[r] = 0;
  T.n_children[r] = 0;
  T.visits[r] = 0;
  T.value_sum[r] = 0;
  T.action[r] = 0.0f;
  T.flags[r] = 0;
}
TR_HD inline void init_forest_header(const Tree& T, int32_t n_roots) {
  for (int i = 0; i < kHdrInts; ++i) T.hdr[i] = 0;
  T.hdr[kHdrNodes] = n_roots;
  T.hdr[kHdrRoots] = n_roots;
}
// shipsim_tree_init_forest on the host (1 <= n_roots <= max_nodes)
inline void init_forest(const Tree& T, int32_t n_roots) {
  init_forest_header(T, n_roots);
  for (int32_t r = 0; r < n_roots; ++r) init_root(T, r);
}

// a_r for r in [0, n_roots): the saturating prefix rule (arrivals_out: n_roots entries)
inline void root_arrivals(const int32_t* root_workers, int32_t n_roots, int32_t n_workers, int32_t* arrivals_out) {
  int32_t before = 0;
  for (int32_t r = 0; r < n_roots; ++r) {
    arrivals_out[r] = root_arrival(root_workers[r], before, n_workers);
    before = sat_add(before, root_ask(root_workers[r], n_workers), n_workers);
  }
}

// shipsim_tree_select_forest on the host, in the stages of the launches: the tile sums of root_workers, the clear
// with the roots as level 0's frontier, the levels, the scan, the leaves
inline void select_forest(const Tree& T, int32_t n_workers, int32_t n_roots, const int32_t* root_workers,
                          int32_t max_depth, int32_t wnum, int32_t wden, double c_explore, const Workspace& S,
                          int32_t* leaf_out, int32_t* expand_out) {
  const uint32_t n = node_count(T.hdr[kHdrNodes], T.M);
  const int32_t R = root_count(n_roots, T.hdr[kHdrRoots], n), W = n_workers;
  const int32_t tiles = (R + kScanTile - 1) / kScanTile;
  for (int32_t b = 0; b < tiles; ++b) {
    int32_t s = 0;
    for (int32_t r = b * kScanTile; r < R && r < (b + 1) * kScanTile; ++r) s = sat_add(s, root_ask(root_workers[r], W), W);
    S.tile_sum[b] = s;
  }
  for (uint32_t v = 0; v < n; ++v) S.stay[v] = S.newc[v] = 0;
  for (int d = 0; d < kMaxDepth + 2; ++d) S.level_count[d] = 0;
  S.level_count[0] = R;
  for (int32_t b = 0; b < tiles; ++b) {
    int32_t before = 0;
    for (int32_t k = 0; k < b; ++k) before = sat_add(before, S.tile_sum[k], W);
    for (int32_t r = b * kScanTile; r < R && r < (b + 1) * kScanTile; ++r) {
      S.fnode[0][r] = r;
      S.fcnt[0][r] = root_arrival(root_workers[r], before, W);
      before = sat_add(before, root_ask(root_workers[r], W), W);
    }
  }
  int32_t arrived[kMaxChildren];
  for (int d = 0; d <= max_depth; ++d) {
    const int32_t* fn = S.fnode[d & 1];
    const int32_t* fc = S.fcnt[d & 1];
    int32_t* nn = S.fnode[(d + 1) & 1];
    int32_t* ncn = S.fcnt[(d + 1) & 1];
    for (int32_t i = 0; i < S.level_count[d]; ++i) {
      const int32_t v = fn[i];
      route_node(T, n, v, fc[i], max_depth, wnum, wden, c_explore, &S.stay[v], &S.newc[v], arrived);
      for (int l = 0; l < T.C; ++l)
        if (arrived[l] > 0) {
          const int32_t pos = S.level_count[d + 1]++;
          nn[pos] = T.child[(int64_t)v * T.C + l];
          ncn[pos] = arrived[l];
        }
    }
  }
  int32_t o = 0;
  for (uint32_t v = 0; v < n; ++v) {
    S.off[v] = o;
    o += S.stay[v] + S.newc[v];
  }
  for (int32_t w = 0; w < n_workers; ++w) {
    leaf_out[w] = -1;
    expand_out[w] = 0;
  }
  for (uint32_t v = 0; v < n; ++v)
    for (int32_t k = 0; k < S.stay[v] + S.newc[v]; ++k) {
      leaf_out[S.off[v] + k] = (int32_t)v;
      expand_out[S.off[v] + k] = k >= S.stay[v];
    }
}

}  // namespace tree_host
