// Stand-alone driver of the state block's column table (ast_sac_amd/csrc/shipsim_state_host.hpp), built by
// tests/test_fork_cpu.py with -fsanitize=address,undefined. For n_envs in {1, 5, 64} and 1..SHIPSIM_MAX_SHIPS ships:
// the columns are disjoint, lie inside the block, respect the 256-byte strides and cover every ship, route and env
// array exactly once (against the block's layout restated here from DevState's accessors); then the gather's own
// arithmetic moves a numbered block on exactly-sized heap buffers, so that an access past the block is caught, and
// every env must arrive whole.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "shipsim_state_host.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                          \
    }                                                    \
  } while (0)

namespace H = state_host;

// fork_gather_kernel on the host: every column, every unit, with the kernel's range test
static void gather(const H::Table& T, const unsigned char* src, unsigned char* dst, const int32_t* src_env,
                   uint32_t n_envs, bool own_fallback) {
  for (int ci = 0; ci < H::kColumns; ++ci) {
    const H::Column c = T.col[ci];
    const uint32_t per_env = H::units_per_env(c), total = n_envs * per_env;
    for (uint32_t t = 0; t < total; ++t) {
      const uint32_t env = t / per_env, piece = t - env * per_env;
      uint32_t from = env;
      if (src_env) {
        const uint32_t s = (uint32_t)src_env[env];
        if (s < n_envs) from = s;
        else if (!own_fallback) continue;
      }
      memcpy(dst + H::unit_dst(c, t), src + H::unit_src(c, from, piece), (size_t)c.unit);
    }
  }
}

int main() {
  int configs = 0;
  for (int64_t n : {(int64_t)1, (int64_t)5, (int64_t)64})
    for (int ns = 1; ns <= SHIPSIM_MAX_SHIPS; ++ns) {
      const H::Layout L = H::layout(n, ns);
      const H::Table T = H::table(L, ns);
      // the strides: multiples of 256 that hold their arrays (what shipsim_create allocated before the table existed)
      CHECK(L.ship_stride % 256 == 0 && L.ship_stride >= n * ns * 8 && L.ship_stride < n * ns * 8 + 256);
      CHECK(L.route_stride % 256 == 0 && L.route_stride >= n * ns * 128 && L.route_stride < n * ns * 128 + 256);
      CHECK(L.env_stride % 256 == 0 && L.env_stride >= n * 32 && L.env_stride < n * 32 + 256);
      CHECK(L.env_off == 22 * L.ship_stride + 2 * L.route_stride);
      CHECK(L.bytes == L.env_off + 19 * L.env_stride);
      // the arrays of the block as DevState addresses them: (offset, stride it lives in, bytes per env)
      struct Want { int64_t off, stride; int env_bytes; };
      std::vector<Want> want;
      for (int k = 0; k < 19; ++k) want.push_back({k * L.ship_stride, L.ship_stride, 8 * ns});   // f(k)
      for (int k = 19; k < 22; ++k) want.push_back({k * L.ship_stride, L.ship_stride, 4 * ns});  // next_wpt, stop, n_route
      want.push_back({22 * L.ship_stride, L.route_stride, 128 * ns});                            // route_n
      want.push_back({22 * L.ship_stride + L.route_stride, L.route_stride, 128 * ns});           // route_e
      const int env_bytes[19] = {4, 8, 8, 8, 8, 8, 8, 8, 8, 16, 32, 4, 4, 4, 32, 4, 4, 4, 32};   // ev(0..18)
      for (int k = 0; k < 19; ++k) want.push_back({L.env_off + k * L.env_stride, L.env_stride, env_bytes[k]});
      CHECK((int)want.size() == H::kColumns);
      // every array exactly once
      std::vector<int> hits(want.size(), 0);
      for (int c = 0; c < H::kColumns; ++c) {
        const H::Column& col = T.col[c];
        int found = -1;
        for (size_t w = 0; w < want.size(); ++w)
          if (want[w].off == col.offset) found = (int)w;
        CHECK(found >= 0);
        hits[found]++;
        CHECK(col.env_bytes == want[found].env_bytes);
        // inside its stride, so inside the block, and aligned for its access width
        CHECK(col.offset % 256 == 0);
        CHECK(n * col.env_bytes <= want[found].stride);
        CHECK(col.offset + n * col.env_bytes <= L.bytes);
        CHECK(col.unit == 4 || col.unit == 8 || col.unit == 16);
        CHECK(col.env_bytes % col.unit == 0 && col.env_bytes > 0);
      }
      for (int x : hits) CHECK(x == 1);
      // disjoint
      std::vector<std::pair<int64_t, int64_t>> ext;
      for (int c = 0; c < H::kColumns; ++c) ext.push_back({T.col[c].offset, T.col[c].offset + n * T.col[c].env_bytes});
      std::sort(ext.begin(), ext.end());
      CHECK(ext.front().first == 0);
      for (size_t i = 1; i < ext.size(); ++i) CHECK(ext[i - 1].second <= ext[i].first);
      CHECK(ext.back().second <= L.bytes);
      CHECK(H::max_units(T, n) == n * ns * 8);  // the route arrays: 8 16-byte pieces per ship

      // the gather on a numbered block: byte b of env e's share of column c carries (c, e, b)
      std::vector<unsigned char> src((size_t)L.bytes, 0xEE), dst((size_t)L.bytes, 0xDD);
      auto mark = [](int c, int64_t e, int b) { return (unsigned char)(1 + (c * 131 + e * 17 + b * 7) % 250); };
      for (int c = 0; c < H::kColumns; ++c)
        for (int64_t e = 0; e < n; ++e)
          for (int b = 0; b < T.col[c].env_bytes; ++b)
            src[(size_t)(T.col[c].offset + e * T.col[c].env_bytes + b)] = mark(c, e, b);
      std::vector<int32_t> idx((size_t)n);
      for (int64_t e = 0; e < n; ++e) idx[(size_t)e] = (int32_t)((e * 3 + 2) % n);  // (a broadcast for n = 1)
      if (n >= 5) { idx[0] = -1; idx[1] = (int32_t)n; idx[2] = 2; }                // out of range twice, a fixed point
      for (int own = 0; own < 2; ++own) {
        std::fill(dst.begin(), dst.end(), (unsigned char)0xDD);
        gather(T, src.data(), dst.data(), idx.data(), (uint32_t)n, own != 0);
        size_t written = 0;
        for (int c = 0; c < H::kColumns; ++c)
          for (int64_t e = 0; e < n; ++e) {
            const int32_t s = idx[(size_t)e];
            const bool in_range = s >= 0 && s < n;
            for (int b = 0; b < T.col[c].env_bytes; ++b) {
              const unsigned char got = dst[(size_t)(T.col[c].offset + e * T.col[c].env_bytes + b)];
              if (in_range) CHECK(got == mark(c, s, b));
              else if (own) CHECK(got == mark(c, e, b));
              else CHECK(got == 0xDD);
              written += got != 0xDD;
            }
          }
        // nothing outside the columns is written (the padding stays as it was)
        size_t touched = 0;
        for (unsigned char x : dst) touched += x != 0xDD;
        CHECK(touched == written);
      }
      // no index array: the identity
      std::fill(dst.begin(), dst.end(), (unsigned char)0xDD);
      gather(T, src.data(), dst.data(), nullptr, (uint32_t)n, false);
      for (int c = 0; c < H::kColumns; ++c)
        CHECK(memcmp(dst.data() + T.col[c].offset, src.data() + T.col[c].offset, (size_t)(n * T.col[c].env_bytes)) == 0);
      ++configs;
    }
  printf("state host OK: %d configurations, %d columns\n", configs, H::kColumns);
  return 0;
}
