// forest_host_check.cpp — the forest additions of the search tree's host half (ast_sac_amd/csrc/shipsim_tree_host.hpp:
// init_forest, root_arrivals, select_forest, forest_select_args_ok) as a stand-alone program, built by
// tests/test_forest_cpu.py with -fsanitize=address,undefined (the runtimes linked in statically).
//   forest_host_check hand                     cases worked by hand: the prefix rule, the argument checks, the roots
//   forest_host_check init M C R out.bin       writes the buffer init_forest leaves (the rest zero)
//   forest_host_check run M C in.bin out.bin   reads a tree buffer, runs the operations named on stdin on exactly-sized
//                                              heap blocks, prints what they return and writes the buffer back
// Operations (every number in hex; doubles and floats as their bits):
//   select_forest W R max_depth wnum wden c_explore / roots ... -> "leaf ...", "expand ..."
//   expand W / leaf ... / expand ... / action ...                -> "node ..."
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

static bool arrivals_are(std::vector<int32_t> c, int32_t W, const std::vector<int32_t>& want) {
  std::vector<int32_t> a(c.size(), -7);  // (exactly sized: the sanitizer's bound)
  TR::root_arrivals(c.data(), (int32_t)c.size(), W, a.data());
  return a == want;
}

static int hand() {
  static_assert(TR::kHdrRoots == 3 && TR::kHdrRoots < TR::kHdrInts, "the header's fourth int");
  // the prefix rule: the roots are served in id order until the W workers are used up
  CHECK(arrivals_are({3, 3, 3}, 7, {3, 3, 1}));
  CHECK(arrivals_are({3, -2, 3, 3}, 7, {3, 0, 3, 1}));             // a negative entry asks for nothing
  CHECK(arrivals_are({2, 100, 5}, 7, {2, 5, 0}));                  // an entry above W takes what is left
  CHECK(arrivals_are({0x7FFFFFFF, 1}, 7, {7, 0}) && arrivals_are({(int32_t)0x80000000, 1}, 7, {0, 1}));
  CHECK(arrivals_are({0, 0, 0, 0}, 7, {0, 0, 0, 0}));              // all zero
  CHECK(arrivals_are({1, 2, 0, 1}, 7, {1, 2, 0, 1}));              // a sum below W
  CHECK(arrivals_are({7}, 7, {7}) && arrivals_are({0, 7, 1}, 7, {0, 7, 0}));
  {  // 4096 entries of 2^22 at W = 2^22: a plain int32 sum of them overflows
    const int32_t W = 1 << 22;
    std::vector<int32_t> c(4096, W), want(4096, 0);
    want[0] = W;
    CHECK(arrivals_are(c, W, want));
    std::vector<int32_t> big(4096, 0x7FFFFFFF);
    CHECK(arrivals_are(big, W, want));
  }
  CHECK(TR::sat_add(0, 0, 5) == 0 && TR::sat_add(2, 3, 5) == 5 && TR::sat_add(5, 5, 5) == 5 && TR::sat_add(1, 3, 5) == 4 &&
        TR::sat_add(1 << 22, 1 << 22, 1 << 22) == 1 << 22);
  for (int32_t a = 0; a <= 6; ++a)  // associative: any order of a scan gives the same prefix
    for (int32_t b = 0; b <= 6; ++b)
      for (int32_t c = 0; c <= 6; ++c)
        CHECK(TR::sat_add(TR::sat_add(a, b, 6), c, 6) == TR::sat_add(a, TR::sat_add(b, c, 6), 6) &&
              TR::sat_add(a, b, 6) == (a + b < 6 ? a + b : 6));
  // the roots a select serves: the caller's, the header's (0 reads as 1), the nodes there are
  CHECK(TR::root_count(1, 0, 9) == 1 && TR::root_count(5, 0, 9) == 1 && TR::root_count(5, 3, 9) == 3 && TR::root_count(2, 3, 9) == 2 &&
        TR::root_count(5, 7, 4) == 4 && TR::root_count(5, -1, 9) == 0 && TR::root_count(5, 5, 0) == 0 &&
        TR::root_count(5, (int32_t)0x80000000, 9) == 0 && TR::root_count(0x7FFFFFFF, 0x7FFFFFFF, 3) == 3);
  // the argument checks
  alignas(16) static char buf[64];
  const int64_t tb = TR::layout(4, 2).bytes, wb = TR::ws_layout(4, 8).bytes;
  CHECK(TR::forest_init_args_ok(buf, tb, 4, 2, 1) && TR::forest_init_args_ok(buf, tb, 4, 2, 4));
  CHECK(!TR::forest_init_args_ok(buf, tb, 4, 2, 0) && !TR::forest_init_args_ok(buf, tb, 4, 2, -1) &&
        !TR::forest_init_args_ok(buf, tb, 4, 2, 5) && !TR::forest_init_args_ok(nullptr, tb, 4, 2, 1) &&
        !TR::forest_init_args_ok(buf, tb - 1, 4, 2, 1) && !TR::forest_init_args_ok(buf + 8, tb, 4, 2, 1));
  CHECK(TR::forest_select_args_ok(buf, tb, 4, 2, 8, 1, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(TR::forest_select_args_ok(buf, tb, 4, 2, 8, 4, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 0, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, -1, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 5, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));  // more roots than nodes
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 3, 4, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));  // more roots than workers
  CHECK(TR::forest_select_args_ok(buf, tb, 4, 2, 4, 4, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, nullptr, 9, 1, 1, 0.0, buf, wb, buf, buf));
  // ... and everything select refuses
  CHECK(!TR::forest_select_args_ok(nullptr, tb, 4, 2, 8, 2, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 0, 2, buf, 9, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 33, 1, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 0, 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, (1 << 15) + 1, 0.0, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, 1, -1e-300, buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, 1, from_bits(0x7FF8000000000000ull), buf, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, 1, 0.0, buf, wb - 1, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, 1, 0.0, buf + 4, wb, buf, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, 1, 0.0, buf, wb, nullptr, buf));
  CHECK(!TR::forest_select_args_ok(buf, tb, 4, 2, 8, 2, buf, 9, 1, 1, 0.0, buf, wb, buf, nullptr));
  printf("forest host OK: prefix rule, root count, argument checks\n");
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

static int write_tree(const char* path, const char* tree, int64_t bytes) {
  FILE* f = fopen(path, "wb");
  CHECK(f && fwrite(tree, 1, (size_t)bytes, f) == (size_t)bytes);
  fclose(f);
  return 0;
}

static int init(int32_t M, int32_t C, int32_t R, const char* out_path) {
  CHECK(TR::sizes_ok(M, C));
  const int64_t bytes = TR::layout(M, C).bytes;
  char* tree = (char*)aligned_alloc(256, (size_t)bytes);
  CHECK(tree && TR::forest_init_args_ok(tree, bytes, M, C, R));
  memset(tree, 0, (size_t)bytes);
  TR::init_forest(TR::view(tree, M, C), R);
  const int rc = write_tree(out_path, tree, bytes);
  free(tree);
  return rc;
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
    if (name == "select_forest") {
      unsigned n_roots, max_depth, wnum, wden;
      unsigned long long cb;
      CHECK(scanf("%x %x %x %x %llx", &n_roots, &max_depth, &wnum, &wden, &cb) == 5);
      std::vector<int32_t> roots, leaf((size_t)W), flags((size_t)W);
      CHECK(read_row("roots", roots, (int32_t)n_roots));
      CHECK(TR::forest_select_args_ok(tree, bytes, M, C, W, (int32_t)n_roots, roots.data(), (int32_t)max_depth,
                                      (int32_t)wnum, (int32_t)wden, from_bits(cb), ws, TR::ws_layout(M, W).bytes,
                                      leaf.data(), flags.data()));
      TR::select_forest(T, W, (int32_t)n_roots, roots.data(), (int32_t)max_depth, (int32_t)wnum, (int32_t)wden,
                        from_bits(cb), S, leaf.data(), flags.data());
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
  const int rc = write_tree(out_path, tree, bytes);
  free(tree);
  return rc;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "hand") return hand();
  if (argc == 6 && std::string(argv[1]) == "init") return init(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argv[5]);
  if (argc == 6 && std::string(argv[1]) == "run") return run(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5]);
  printf("usage: forest_host_check hand | init M C R out.bin | run M C in.bin out.bin\n");
  return 2;
}
