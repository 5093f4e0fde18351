// tree_host_check.cpp — the host half of the search tree (ast_sac_amd/csrc/shipsim_tree_host.hpp) as a stand-alone
// program, built by tests/test_tree_cpu.py with -fsanitize=address,undefined (the runtimes linked in statically).
//   tree_host_check hand                       cases worked by hand: the layouts, the argument checks, the arithmetic
//   tree_host_check run M C in.bin out.bin     reads a tree buffer, runs the operations named on stdin on exactly-sized
//                                              heap blocks, prints what they return and writes the buffer back
// Operations (every number in hex; doubles and floats as their bits):
//   select W max_depth wnum wden c_explore                  -> "leaf ...", "expand ..."
//   expand W / leaf ... / expand ... / action ...           -> "node ..."
//   backup W has_terminal / node ... / value ... [/ terminal ...]
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "shipsim.h"
#include "shipsim_tree_host.hpp"

namespace TR = tree_host;

#define CHECK(x)                                                    \
  do {                                                              \
    if (!(x)) {                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);         \
      return 1;                                                     \
    }                                                               \
  } while (0)

static double from_bits(uint64_t b) {
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
}

static int hand() {
  static_assert(TR::kMaxNodes == SHIPSIM_ARCHIVE_MAX_CELLS && TR::kMaxChildren == SHIPSIM_TREE_MAX_CHILDREN &&
                    TR::kMaxDepth == SHIPSIM_TREE_MAX_DEPTH && TR::kScanTile == SHIPSIM_TREE_SCAN_TILE,
                "the header's numbers");
  // the layouts: every array inside the buffer, none overlapping, in the order of the table
  for (int32_t M : {1, 5, 64, 1025}) {
    for (int32_t C : {1, 3, 64}) {
      const TR::Layout L = TR::layout(M, C);
      const int64_t o[] = {L.header, L.parent, L.depth, L.n_children, L.child, L.visits, L.value_sum, L.action, L.flags, L.bytes};
      const int64_t need[] = {16, 4LL * M, 4LL * M, 4LL * M, 4LL * M * C, 4LL * M, 8LL * M, 4LL * M, 4LL * M};
      for (int i = 0; i < 9; ++i) CHECK(o[i] % 256 == 0 && o[i] + need[i] <= o[i + 1]);
      const TR::WsLayout S = TR::ws_layout(M, 7);
      CHECK(S.stay + 4LL * M <= S.newc && S.newc + 4LL * M <= S.off && S.off + 4LL * M <= S.slot &&
            S.slot + 28 <= S.fnode[0] && S.fnode[0] + 28 <= S.fcnt[0] && S.fcnt[0] + 28 <= S.fnode[1] &&
            S.fnode[1] + 28 <= S.fcnt[1] && S.fcnt[1] + 28 <= S.level_count &&
            S.level_count + 4 * (TR::kMaxDepth + 2) <= S.tile_sum && S.tile_sum + 4LL * TR::kMaxTiles <= S.bytes);
    }
  }
  // the argument checks
  alignas(16) static char buf[64];
  const int64_t tb = TR::layout(4, 2).bytes, wb = TR::ws_layout(4, 8).bytes;
  CHECK(TR::tree_args_ok(buf, tb, 4, 2) && !TR::tree_args_ok(nullptr, tb, 4, 2) && !TR::tree_args_ok(buf + 8, tb, 4, 2));
  CHECK(!TR::tree_args_ok(buf, tb - 1, 4, 2) && !TR::tree_args_ok(buf, tb, 0, 2) && !TR::tree_args_ok(buf, tb, 4, 65) &&
        !TR::tree_args_ok(buf, tb, TR::kMaxNodes + 1, 2) && !TR::tree_args_ok(buf, tb, 4, 0));
  CHECK(TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 0, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, TR::kMaxWorkers + 1, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 33, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, -1, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 0, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, (1 << 15) + 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, -1e-300, buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, from_bits(0x7FF8000000000000ull), buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, from_bits(0x7FF0000000000000ull), buf, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, 0.0, buf, wb - 1, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, 0.0, buf + 4, wb, buf, buf));
  CHECK(!TR::select_args_ok(buf, tb, 4, 2, 8, 9, 1, 1, 0.0, buf, wb, nullptr, buf));
  CHECK(TR::backup_args_ok(buf, tb, 4, 2, 8, buf, buf) && !TR::backup_args_ok(buf, tb, 4, 2, 8, buf, nullptr));
  // the widening rule: m < k sqrt(N + 1); k^2 = 1: the second child at N + 1 = 2, the third at 5, never past C
  CHECK(TR::widens(0, 3, 1, 1, 0) && !TR::widens(1, 3, 1, 1, 0) && TR::widens(1, 3, 1, 1, 1) && !TR::widens(2, 3, 1, 1, 3) &&
        TR::widens(2, 3, 1, 1, 4) && !TR::widens(3, 3, 1, 1, 1000000) && TR::widens(63, 64, 1 << 15, 1, 0) &&
        !TR::widens(63, 64, 1, 1 << 15, ((int64_t)1 << 26)) && TR::widens(1, 64, 1, 1 << 15, ((int64_t)1 << 31) + (1 << 22)));
  // the value image: to nearest even at 2^-25, clamped, exact back
  CHECK(TR::quantize(1.0) == 1 << 24 && TR::quantize(-0.5) == -(1 << 23) && TR::quantize(ldexp(1.0, -25)) == 0 &&
        TR::quantize(ldexp(3.0, -25)) == 2 && TR::quantize(-ldexp(3.0, -25)) == -2 && TR::quantize(1e300) == TR::kQClamp &&
        TR::quantize(-1e300) == -TR::kQClamp && TR::quantize(65536.0) == TR::kQClamp && TR::quantize(65535.0) == 65535LL << 24);
  CHECK(TR::q_of(0, 12345) == 0.0 && TR::q_of(2, 3LL << 24) == 1.5 && TR::q_of(4, -(1LL << 24)) == -0.25);
  CHECK(TR::score(0.25, 2.0, 8, 1, 1) == 0.25 + 6.0 / 3.0 && TR::score(-1.0, 0.0, 99, 0, 0) == -1.0);
  CHECK(!TR::backup_ok(-1, 5, 1.0) && !TR::backup_ok(5, 5, 1.0) && TR::backup_ok(4, 5, -1e300) &&
        !TR::backup_ok(0, 5, from_bits(0x7FF0000000000000ull)) && !TR::backup_ok(0, 5, from_bits(0xFFF8000000000001ull)));
  printf("tree host OK: layouts, argument checks, widening, value image\n");
  return 0;
}

template <class T>
static bool read_row(const char* want, std::vector<T>& out, int32_t n) {
  char name[32];
  if (scanf("%31s", name) != 1 || std::string(name) != want) return false;
  out.resize((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    unsigned long long v;
    if (scanf("%llx", &v) != 1) return false;
    if constexpr (sizeof(T) == 8) {
      uint64_t b = v;
      memcpy(&out[(size_t)i], &b, 8);
    } else if constexpr (sizeof(T) == 4) {
      uint32_t b = (uint32_t)v;
      memcpy(&out[(size_t)i], &b, 4);
    } else {
      out[(size_t)i] = (T)v;
    }
  }
  return true;
}

static void print_row(const char* name, const int32_t* x, int32_t n) {
  printf("%s", name);
  for (int32_t i = 0; i < n; ++i) printf(" %x", (unsigned)x[i]);
  printf("\n");
}

static int run(int32_t M, int32_t C, const char* in_path, const char* out_path) {
  CHECK(TR::sizes_ok(M, C));
  const int64_t bytes = TR::layout(M, C).bytes;
  char* tree = (char*)aligned_alloc(256, (size_t)bytes);
  CHECK(tree);
  FILE* f = fopen(in_path, "rb");
  CHECK(f && fread(tree, 1, (size_t)bytes, f) == (size_t)bytes);
  fclose(f);
  const TR::Tree T = TR::view(tree, M, C);
  char op[32];
  while (scanf("%31s", op) == 1) {
    unsigned w_in;
    CHECK(scanf("%x", &w_in) == 1);
    const int32_t W = (int32_t)w_in;
    CHECK(TR::workers_ok(W));
    char* ws = (char*)aligned_alloc(256, (size_t)TR::ws_layout(M, W).bytes);  // (exactly sized: the sanitizer's bound)
    CHECK(ws);
    const TR::Workspace S = TR::ws_view(ws, M, W);
    const std::string name(op);
    if (name == "select") {
      unsigned max_depth, wnum, wden;
      unsigned long long cb;
      CHECK(scanf("%x %x %x %llx", &max_depth, &wnum, &wden, &cb) == 4);
      std::vector<int32_t> leaf((size_t)W), flags((size_t)W);
      CHECK(TR::select_args_ok(tree, bytes, M, C, W, (int32_t)max_depth, (int32_t)wnum, (int32_t)wden, from_bits(cb), ws,
                               TR::ws_layout(M, W).bytes, leaf.data(), flags.data()));
      TR::select(T, W, (int32_t)max_depth, (int32_t)wnum, (int32_t)wden, from_bits(cb), S, leaf.data(), flags.data());
      print_row("leaf", leaf.data(), W);
      print_row("expand", flags.data(), W);
    } else if (name == "expand") {
      std::vector<int32_t> leaf, flags, node((size_t)W);
      std::vector<float> action;
      CHECK(read_row("leaf", leaf, W) && read_row("expand", flags, W) && read_row("action", action, W));
      TR::expand(T, W, leaf.data(), flags.data(), action.data(), S, node.data());
      print_row("node", node.data(), W);
    } else if (name == "backup") {
      unsigned has_terminal;
      CHECK(scanf("%x", &has_terminal) == 1);
      std::vector<int32_t> node;
      std::vector<double> value;
      std::vector<uint8_t> terminal;
      CHECK(read_row("node", node, W) && read_row("value", value, W));
      if (has_terminal) CHECK(read_row("terminal", terminal, W));
      TR::backup(T, W, node.data(), value.data(), has_terminal ? terminal.data() : nullptr);
    } else {
      CHECK(!"an operation");
    }
    free(ws);
  }
  f = fopen(out_path, "wb");
  CHECK(f && fwrite(tree, 1, (size_t)bytes, f) == (size_t)bytes);
  fclose(f);
  free(tree);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "hand") return hand();
  if (argc == 6 && std::string(argv[1]) == "run") return run(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5]);
  printf("usage: tree_host_check hand | run M C in.bin out.bin\n");
  return 2;
}
