// Stand-alone driver of the host half of shipsim_weather_store / _load / _fork
// (ast_sac_amd/csrc/shipsim_weather_host.hpp), built by tests/test_weather_carry_cpu.py with
// -fsanitize=address,undefined.
//   weather_carry_host_check self    sizes, row offsets, the stored rows and every refusal reason
//   weather_carry_host_check gather  gathers read from stdin, on exactly-sized heap tables so that a read or a write
//                                    outside them is caught. Per gather three lines of hexadecimal words:
//                                      n_dst n_src own / the n_dst indices (two's complement) / the 6 * n_src source
//                                    doubles then the 6 * n_dst destination doubles as bits; the answer is one line,
//                                    the destination's bits after the gather.
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "shipsim_weather_host.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                          \
    }                                                    \
  } while (0)

namespace W = weather_host;

static bool says(const char* why, const char* word) { return why && strstr(why, word); }

static int self_check() {
  // sizes and offsets
  CHECK(W::kCols == 5 && W::kStoreRows == 6 && W::kDirection == 5);
  CHECK(W::kMaxSlots == SHIPSIM_ARCHIVE_MAX_CELLS);
  CHECK(!W::slots_ok(0) && !W::slots_ok(-1) && W::slots_ok(1) && W::slots_ok(W::kMaxSlots) &&
        !W::slots_ok(W::kMaxSlots + 1) && !W::slots_ok(std::numeric_limits<int32_t>::min()));
  for (int64_t n : {(int64_t)1, (int64_t)5, (int64_t)300, (int64_t)65536, (int64_t)W::kMaxSlots}) {
    CHECK(W::store_bytes(n) == 6 * n * 8);
    for (int r = 0; r < W::kStoreRows; ++r) CHECK(W::row_offset(r, n) == (int64_t)r * n * 8);
    CHECK(W::row_offset(W::kStoreRows, n) == W::store_bytes(n));
  }
  // the stored rows: the five the kernels read as rows() writes them, then the direction as given
  for (size_t n : {(size_t)1, (size_t)7, (size_t)300}) {
    std::vector<double> ws(n), wd(n), vn(n), ve(n), five(W::kCols * n, -7.0), six(W::kStoreRows * n, -7.0);
    for (size_t i = 0; i < n; ++i) {
      ws[i] = 0.5 * (double)(i % 25);
      wd[i] = -3.0 + 0.37 * (double)(i % 17);
      vn[i] = 0.1 * (double)(i % 9) - 0.4;
      ve[i] = 0.4 - 0.1 * (double)(i % 7);
    }
    W::rows(ws.data(), wd.data(), vn.data(), ve.data(), n, five.data());
    W::store_rows(ws.data(), wd.data(), vn.data(), ve.data(), n, six.data());
    CHECK(memcmp(five.data(), six.data(), sizeof(double) * W::kCols * n) == 0);
    CHECK(memcmp(six.data() + W::kDirection * n, wd.data(), sizeof(double) * n) == 0);
  }
  // every refusal reason, in the order they are tested
  alignas(16) unsigned char buf[64];
  const int32_t idx[4] = {0, 1, 2, 3};
  const int32_t n_envs = 4;
  const int64_t bytes = W::store_bytes(n_envs);
  CHECK(W::fork_refusal(true) == nullptr);
  CHECK(says(W::fork_refusal(false), "no per-env weather"));
  CHECK(W::carry_refusal(true, buf, bytes, n_envs, n_envs, idx) == nullptr);
  CHECK(W::carry_refusal(true, buf, bytes, n_envs, n_envs, nullptr) == nullptr);  // the identity
  CHECK(W::carry_refusal(true, buf, W::store_bytes(7), 7, n_envs, idx) == nullptr);
  CHECK(says(W::carry_refusal(false, buf, bytes, n_envs, n_envs, idx), "no per-env weather"));
  CHECK(says(W::carry_refusal(false, nullptr, 0, 0, n_envs, nullptr), "no per-env weather"));
  CHECK(says(W::carry_refusal(true, nullptr, bytes, n_envs, n_envs, idx), "buffer is NULL"));
  for (int32_t bad : {0, -1, W::kMaxSlots + 1, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max()})
    CHECK(says(W::carry_refusal(true, buf, bytes, bad, n_envs, idx), "n_slots"));
  for (int64_t wrong : {bytes - 8, bytes + 8, (int64_t)0, (int64_t)-1, W::store_bytes(n_envs + 1), bytes * 5 / 6})
    CHECK(says(W::carry_refusal(true, buf, wrong, n_envs, n_envs, idx), "bytes"));
  CHECK(says(W::carry_refusal(true, buf + 8, bytes, n_envs, n_envs, idx), "16-byte aligned"));
  CHECK(says(W::carry_refusal(true, buf + 1, bytes, n_envs, n_envs, idx), "16-byte aligned"));
  CHECK(says(W::carry_refusal(true, buf, W::store_bytes(7), 7, n_envs, nullptr), "NULL index"));
  CHECK(says(W::carry_refusal(true, buf, W::store_bytes(3), 3, n_envs, nullptr), "NULL index"));
  // which indices are served
  CHECK(W::index_ok(0, 1) && W::index_ok(299, 300) && !W::index_ok(300, 300) && !W::index_ok(-1, 300));
  CHECK(!W::index_ok(std::numeric_limits<int32_t>::min(), 300) && !W::index_ok(std::numeric_limits<int32_t>::max(), 300));
  // a NULL index is the identity
  {
    std::vector<double> src(W::kStoreRows * 5), dst(W::kStoreRows * 5, -1.0);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (double)i;
    W::gather(src.data(), dst.data(), nullptr, 5, 5, false);
    CHECK(src == dst);
  }
  printf("weather carry host OK\n");
  return 0;
}

static int gather_check() {
  uint32_t n_dst, n_src, own;
  int n_done = 0;
  while (scanf("%" SCNx32 " %" SCNx32 " %" SCNx32, &n_dst, &n_src, &own) == 3) {
    CHECK(n_dst >= 1 && n_src >= 1 && n_dst <= (1u << 20) && n_src <= (1u << 20) && own <= 1);
    std::vector<int32_t> index(n_dst);
    std::vector<double> src((size_t)W::kStoreRows * n_src), dst((size_t)W::kStoreRows * n_dst);
    for (auto& x : index) {
      uint32_t u;
      CHECK(scanf("%" SCNx32, &u) == 1);
      memcpy(&x, &u, 4);
    }
    for (std::vector<double>* t : {&src, &dst})
      for (auto& x : *t) {
        uint64_t u;
        CHECK(scanf("%" SCNx64, &u) == 1);
        memcpy(&x, &u, 8);
      }
    W::gather(src.data(), dst.data(), index.data(), n_dst, n_src, own != 0);
    for (size_t i = 0; i < dst.size(); ++i) {
      uint64_t u;
      memcpy(&u, &dst[i], 8);
      printf("%" PRIx64 "%c", u, i + 1 == dst.size() ? '\n' : ' ');
    }
    ++n_done;
  }
  CHECK(n_done > 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return self_check();
  if (argc == 2 && !strcmp(argv[1], "gather")) return gather_check();
  fprintf(stderr, "usage: weather_carry_host_check self | gather\n");
  return 2;
}
