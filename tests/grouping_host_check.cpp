// Stand-alone driver of the stream grouping's host half (ast_sac_amd/csrc/shipsim_grouping_host.hpp), built by
// tests/test_stream_grouping_cpu.py with -fsanitize=address,undefined. Without arguments: which launches group, the
// buffer's size, the key's edge cases, and rank-by-counting (what the device kernel does) against the reference
// ordering on exactly-sized heap arrays. With `order`: reads "n dt" and n clock values from stdin and prints each
// env's key, then the reference ordering, for the test's comparison with a Python sort.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "shipsim_grouping_host.hpp"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                               \
    }                                                         \
  } while (0)

namespace G = grouping_host;
namespace L = launch_host;

static int order_mode() {
  int n = 0;
  double dt = 0;
  if (scanf("%d %lf", &n, &dt) != 2 || n < 1) return 2;
  std::vector<double> time((size_t)n);
  for (double& t : time)
    if (scanf("%lf", &t) != 1) return 2;
  std::vector<int32_t> keys((size_t)n), order((size_t)n);
  for (int i = 0; i < n; ++i) keys[(size_t)i] = G::key_of(time[(size_t)i], dt);
  G::reference_order(keys.data(), n, order.data());
  for (int i = 0; i < n; ++i) printf("%d%c", keys[(size_t)i], i + 1 < n ? ' ' : '\n');
  for (int i = 0; i < n; ++i) printf("%d%c", order[(size_t)i], i + 1 < n ? ' ' : '\n');
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "order")) return order_mode();

  // which launches group: the decision streams, with the switch on, up to kMaxEnvs envs
  for (int on = 0; on <= 1; ++on)
    for (int entry = 0; entry <= 2; ++entry)
      for (int32_t n : {1, 4, 61, 4096, G::kMaxEnvs, G::kMaxEnvs + 1, 1 << 20}) {
        const bool want = on && entry != L::kStep && n <= G::kMaxEnvs;
        CHECK(G::groups((L::Entry)entry, n, on != 0) == want);
      }
  CHECK(!G::groups(L::kTable, 0, true) && !G::groups(L::kPolicy, -3, true));
  // the switch from create: two-ship envs with collav sbmpc
  for (int collav = 0; collav <= 2; ++collav)
    for (int n_ships = 2; n_ships <= SHIPSIM_MAX_SHIPS; ++n_ships)
      CHECK(G::default_on(collav, n_ships) == (collav == SHIPSIM_COLLAV_SBMPC && n_ships == 2));
  CHECK(G::buffer_len(1) == 1 && G::buffer_len(4096) == 4096 && G::buffer_len(G::kMaxEnvs) == (size_t)G::kMaxEnvs);
  CHECK(G::buffer_len(G::kMaxEnvs + 1) == 0 && G::buffer_len(0) == 0 && G::buffer_len(-1) == 0);

  // the key: ticks since the reset from an accumulated clock, whatever its rounding; the odd clocks sort first
  for (double dt : {4.0, 0.5, 0.1, 1.0 / 3.0}) {
    double t = 0.0;
    for (int k = 0; k <= 5000; ++k) {
      CHECK(G::key_of(t, dt) == k);
      t = t + dt;  // (as the kernels advance it)
    }
  }
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(G::key_of(nan, 4.0) == 0 && G::key_of(-inf, 4.0) == 0 && G::key_of(-8.0, 4.0) == 0 && G::key_of(0.0, 4.0) == 0);
  CHECK(G::key_of(inf, 4.0) == G::kMaxKey && G::key_of(1e300, 4.0) == G::kMaxKey);
  CHECK(G::key_of(4.0, nan) == 0 && G::key_of(4.0, -4.0) == 0);  // (shipsim_create refuses a time step <= 0)

  // rank by counting is the reference ordering's inverse: a permutation, ascending in the key, ties by index
  uint32_t lcg = 12345u;
  for (int32_t n : {1, 2, 3, 61, 64, 257, 1000}) {
    for (int32_t span : {1, 3, 50, 1 << 20}) {
      std::vector<int32_t> keys((size_t)n), order((size_t)n), by_rank((size_t)n, -1);
      for (int32_t& k : keys) {
        lcg = lcg * 1664525u + 1013904223u;
        k = (int32_t)((lcg >> 8) % (uint32_t)span);
      }
      G::reference_order(keys.data(), n, order.data());
      for (int32_t i = 0; i < n; ++i) {
        const int32_t r = G::rank_of(keys.data(), n, i);
        CHECK(r >= 0 && r < n && by_rank[(size_t)r] == -1);
        by_rank[(size_t)r] = i;
      }
      for (int32_t s = 0; s < n; ++s) {
        CHECK(by_rank[(size_t)s] == order[(size_t)s]);
        if (s) {
          const int32_t a = order[(size_t)s - 1], b = order[(size_t)s];
          CHECK(keys[(size_t)a] < keys[(size_t)b] || (keys[(size_t)a] == keys[(size_t)b] && a < b));
        }
      }
    }
  }
  printf("grouping host OK\n");
  return 0;
}
