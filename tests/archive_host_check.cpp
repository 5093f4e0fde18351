// Stand-alone driver of the state archive's host half (ast_sac_amd/csrc/shipsim_archive_host.hpp), built by
// tests/test_archive_cpu.py with -fsanitize=address,undefined.
//   archive_host_check gather   for (n_envs, n_cells) in {(48, 7), (5, 300), (64, 64)} and 1..SHIPSIM_MAX_SHIPS ships:
//                               the two-table gather's own arithmetic moves a numbered block between exactly-sized
//                               heap buffers, a store and a load, so that an access past either is caught; every unit
//                               of every column lands inside its slot's bytes on both sides, out-of-range indices and
//                               the padding are left alone. Then the argument checks.
//   archive_host_check elect    reads elections from stdin (hex words: n_envs n_cells n_rounds, then per round n_envs
//                               cells and n_envs score bits) and runs archive_host::elect on them one after the
//                               other, cell_score starting NaN and cell_seen 0; prints, per round, env_of_cell, the
//                               bits of cell_score, cell_seen and n_improved.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "shipsim_archive_host.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                          \
    }                                                    \
  } while (0)

namespace H = state_host;
namespace A = archive_host;

static unsigned char mark(int c, int64_t e, int b) { return (unsigned char)(1 + (c * 131 + e * 17 + b * 7) % 250); }

// a block of n slots whose byte b of slot e's share of column c carries mark(c, e, b), everything else `pad`
static std::vector<unsigned char> numbered(const H::Layout& L, const H::Table& T, int64_t n, unsigned char pad) {
  std::vector<unsigned char> blk((size_t)L.bytes, pad);
  for (int c = 0; c < H::kColumns; ++c)
    for (int64_t e = 0; e < n; ++e)
      for (int b = 0; b < T.col[c].env_bytes; ++b)
        blk[(size_t)(T.col[c].offset + e * T.col[c].env_bytes + b)] = mark(c, e, b);
  return blk;
}

// dst (n_dst slots, 0xDD before the gather) against what index asks for from a numbered source of n_src slots
static int verify(const H::Table& Td, const std::vector<unsigned char>& dst, const std::vector<int32_t>& index,
                  int64_t n_dst, int64_t n_src) {
  size_t written = 0;
  for (int c = 0; c < H::kColumns; ++c)
    for (int64_t d = 0; d < n_dst; ++d) {
      const int32_t s = index[(size_t)d];
      const bool in_range = s >= 0 && s < n_src;
      for (int b = 0; b < Td.col[c].env_bytes; ++b) {
        const unsigned char got = dst[(size_t)(Td.col[c].offset + d * Td.col[c].env_bytes + b)];
        if (in_range) CHECK(got == mark(c, s, b));
        else CHECK(got == 0xDD);
        written += got != 0xDD;
      }
    }
  size_t touched = 0;  // nothing outside the columns is written (the padding stays as it was)
  for (unsigned char x : dst) touched += x != 0xDD;
  CHECK(touched == written);
  return 0;
}

static int gather_checks() {
  int configs = 0;
  const int64_t shapes[3][2] = {{48, 7}, {5, 300}, {64, 64}};
  for (const auto& shape : shapes)
    for (int ns = 1; ns <= SHIPSIM_MAX_SHIPS; ++ns) {
      const int64_t n_envs = shape[0], n_cells = shape[1];
      const H::Layout Le = H::layout(n_envs, ns), Lc = H::layout(n_cells, ns);
      const H::Table Te = H::table(Le, ns), Tc = H::table(Lc, ns);
      CHECK(A::tables_match(Te, Tc));
      CHECK(A::archive_bytes(n_cells, ns) == Lc.bytes);
      if (n_envs == n_cells) CHECK(Le.bytes == Lc.bytes && memcmp(&Te, &Tc, sizeof Te) == 0);
      // every unit of every column: inside its slot's bytes on both sides, whatever in-range index it is given
      for (int c = 0; c < H::kColumns; ++c)
        for (int dir = 0; dir < 2; ++dir) {
          const H::Column cs = dir ? Tc.col[c] : Te.col[c], cd = dir ? Te.col[c] : Tc.col[c];
          const int64_t n_src = dir ? n_cells : n_envs, n_dst = dir ? n_envs : n_cells;
          const uint32_t total = (uint32_t)n_dst * H::units_per_env(cd);
          for (uint32_t t = 0; t < total; ++t) {
            const uint32_t d = A::slot_of(cd, t), p = A::piece_of(cd, t);
            CHECK(d < n_dst && p < H::units_per_env(cs));
            const int64_t q = A::store_at(cd, t);
            CHECK(q >= cd.offset + (int64_t)d * cd.env_bytes && q + cd.unit <= cd.offset + (int64_t)(d + 1) * cd.env_bytes);
            CHECK(q % cd.unit == 0);
            for (int64_t from : {(int64_t)0, n_src / 2, n_src - 1}) {
              const int64_t r = A::load_at(cs, (uint32_t)from, p);
              CHECK(r >= cs.offset + from * cs.env_bytes && r + cs.unit <= cs.offset + (from + 1) * cs.env_bytes);
              CHECK(r % cs.unit == 0);
              CHECK(r - (cs.offset + from * cs.env_bytes) == q - (cd.offset + (int64_t)d * cd.env_bytes));
            }
          }
        }
      CHECK(!A::index_ok(-1, (uint32_t)n_envs) && !A::index_ok((int32_t)n_envs, (uint32_t)n_envs) &&
            !A::index_ok(2147483647, (uint32_t)n_envs) && !A::index_ok(-2147483647 - 1, (uint32_t)n_envs) &&
            A::index_ok(0, (uint32_t)n_envs) && A::index_ok((int32_t)n_envs - 1, (uint32_t)n_envs));

      // store: a permutation with repeats of the envs into the cells, some cells left out
      const std::vector<unsigned char> live = numbered(Le, Te, n_envs, 0xEE);
      std::vector<unsigned char> arch((size_t)Lc.bytes, 0xDD);
      std::vector<int32_t> env_of_cell((size_t)n_cells);
      for (int64_t c = 0; c < n_cells; ++c) env_of_cell[(size_t)c] = (int32_t)((c * 5 + 3) % n_envs);
      env_of_cell[0] = -1;
      if (n_cells > 4) { env_of_cell[1] = (int32_t)n_envs; env_of_cell[2] = 2147483647; env_of_cell[3] = (int32_t)n_cells; }
      A::gather(Te, Tc, live.data(), arch.data(), env_of_cell.data(), (uint32_t)n_cells, (uint32_t)n_envs);
      {
        std::vector<int32_t> want = env_of_cell;  // (n_cells as an index is in range when n_cells < n_envs)
        if (verify(Tc, arch, want, n_cells, n_envs)) return 1;
      }
      // load: from a numbered archive into the envs under another index array
      const std::vector<unsigned char> full = numbered(Lc, Tc, n_cells, 0xEE);
      std::vector<unsigned char> blk((size_t)Le.bytes, 0xDD);
      std::vector<int32_t> cell_of_env((size_t)n_envs);
      for (int64_t e = 0; e < n_envs; ++e) cell_of_env[(size_t)e] = (int32_t)((e * 7 + 1) % n_cells);
      cell_of_env[(size_t)(n_envs - 1)] = (int32_t)n_cells;
      if (n_envs > 4) { cell_of_env[0] = -1; cell_of_env[1] = 2147483647; cell_of_env[2] = (int32_t)n_envs; }
      A::gather(Tc, Te, full.data(), blk.data(), cell_of_env.data(), (uint32_t)n_envs, (uint32_t)n_cells);
      if (verify(Te, blk, cell_of_env, n_envs, n_cells)) return 1;
      ++configs;
    }

  // the argument checks
  alignas(16) static unsigned char buf[64];
  int32_t idx[4] = {0, 0, 0, 0};
  const int64_t b7 = A::archive_bytes(7, 2);
  CHECK(A::check_args(buf, idx, b7, 7, 2) == A::kArgOk);
  CHECK(A::check_args(nullptr, idx, b7, 7, 2) == A::kArgNullArchive);
  CHECK(A::check_args(buf, nullptr, b7, 7, 2) == A::kArgNullIndex);
  CHECK(A::check_args(buf, idx, b7, 0, 2) == A::kArgCells && A::check_args(buf, idx, b7, -1, 2) == A::kArgCells &&
        A::check_args(buf, idx, b7, A::kMaxCells + 1, 2) == A::kArgCells);
  CHECK(A::check_args(buf, idx, b7 - 1, 7, 2) == A::kArgBytes && A::check_args(buf, idx, b7, 7, 3) == A::kArgBytes);
  CHECK(A::check_args(buf + 8, idx, b7, 7, 2) == A::kArgAlign && A::check_args(buf + 4, idx, b7, 7, 2) == A::kArgAlign);
  CHECK(A::check_args(buf, idx, A::archive_bytes(A::kMaxCells, 5), A::kMaxCells, 5) == A::kArgOk);
  const int64_t w = A::layout(9).bytes;
  CHECK(A::elect_args_ok(4, 9, idx, buf, buf, buf, w, idx));
  CHECK(!A::elect_args_ok(0, 9, idx, buf, buf, buf, w, idx) && !A::elect_args_ok(A::kMaxEnvs + 1, 9, idx, buf, buf, buf, w, idx));
  CHECK(!A::elect_args_ok(4, 0, idx, buf, buf, buf, w, idx) && !A::elect_args_ok(4, A::kMaxCells + 1, idx, buf, buf, buf, w, idx));
  CHECK(!A::elect_args_ok(4, 9, nullptr, buf, buf, buf, w, idx) && !A::elect_args_ok(4, 9, idx, nullptr, buf, buf, w, idx) &&
        !A::elect_args_ok(4, 9, idx, buf, nullptr, buf, w, idx) && !A::elect_args_ok(4, 9, idx, buf, buf, nullptr, w, idx) &&
        !A::elect_args_ok(4, 9, idx, buf, buf, buf, w, nullptr));
  CHECK(!A::elect_args_ok(4, 9, idx, buf, buf, buf, w - 1, idx) && !A::elect_args_ok(4, 9, idx, buf, buf, buf + 8, w, idx));
  int64_t last = 0;
  for (int32_t m : {1, 2, 63, 64, 65, 255, 257, 4097, 1 << 20, A::kMaxCells}) {
    CHECK(A::layout(m).bytes >= last && A::layout(m).bytes >= (int64_t)m * 16);
    last = A::layout(m).bytes;
  }
  printf("archive host OK: %d configurations, %d columns\n", configs, H::kColumns);
  return 0;
}

static int elect_rounds() {
  unsigned n_envs, n_cells, n_rounds;
  CHECK(scanf("%x %x %x", &n_envs, &n_cells, &n_rounds) == 3);
  CHECK(A::elect_sizes_ok((int32_t)n_envs, (int32_t)n_cells));
  const uint64_t nan_bits = 0x7FF8000000000000ull;
  std::vector<double> cell_score(n_cells);
  for (double& x : cell_score) memcpy(&x, &nan_bits, 8);
  std::vector<int32_t> cell_seen(n_cells, 0), env_of_cell(n_cells), cell(n_envs);
  std::vector<double> score(n_envs);
  // exactly the workspace's bytes, filled with junk: elect clears what it reads
  std::vector<unsigned char> ws((size_t)A::layout((int32_t)n_cells).bytes, 0xA5);
  for (unsigned r = 0; r < n_rounds; ++r) {
    for (unsigned i = 0; i < n_envs; ++i) {
      unsigned c;
      CHECK(scanf("%x", &c) == 1);
      cell[i] = (int32_t)c;
    }
    for (unsigned i = 0; i < n_envs; ++i) {
      uint64_t b;
      CHECK(scanf("%" SCNx64, &b) == 1);
      memcpy(&score[i], &b, 8);
    }
    int32_t n_improved = -7;
    A::elect((int32_t)n_envs, (int32_t)n_cells, cell.data(), score.data(), cell_score.data(), cell_seen.data(),
             ws.data(), env_of_cell.data(), &n_improved);
    printf("env_of_cell");
    for (int32_t e : env_of_cell) printf(" %x", (unsigned)e);
    printf("\ncell_score");
    for (double x : cell_score) printf(" %" PRIx64, A::bits_of(x));
    printf("\ncell_seen");
    for (int32_t x : cell_seen) printf(" %x", (unsigned)x);
    printf("\nn_improved %x\n", (unsigned)n_improved);
    // the optional outputs left out: the same cells, nothing else written
    std::vector<double> cs2 = cell_score;
    std::vector<int32_t> eoc2(n_cells);
    A::elect((int32_t)n_envs, (int32_t)n_cells, cell.data(), score.data(), cs2.data(), nullptr, ws.data(), eoc2.data(),
             nullptr);
    for (unsigned c = 0; c < n_cells; ++c) CHECK(eoc2[c] == -1 && A::bits_of(cs2[c]) == A::bits_of(cell_score[c]));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "gather")) return gather_checks();
  if (argc == 2 && !strcmp(argv[1], "elect")) return elect_rounds();
  fprintf(stderr, "usage: %s gather | elect < rounds\n", argv[0]);
  return 2;
}
