// shipsim_archive_host.hpp — the host half of the state archive (include/shipsim.h: shipsim_archive_store / _load /
// _elect): the argument checks, the gather between two column tables (the live block's and the archive's: the same
// columns, other strides), the election's workspace as a table of offsets, the order-preserving image of a score
// and the election itself restated on the host. Free of the device and of the handle (plain C++17), so that it can
// be compiled and driven on its own: tests/test_archive_cpu.py builds it into a stand-alone program
// (tests/archive_host_check.cpp) with -fsanitize=address,undefined. The kernels of shipsim_archive.hip call the same
// functions, so GPU, host program and the Python restatement (tests/archive_ref.py) agree bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "shipsim_state_host.hpp"

#if defined(__HIPCC__)
#define AR_HD __host__ __device__
#else
#define AR_HD
#endif

namespace archive_host {

constexpr int32_t kMaxCells = 1 << 22;  // SHIPSIM_ARCHIVE_MAX_CELLS
constexpr int32_t kMaxEnvs = 1 << 22;   // the most envs one election takes (the resampler's limit)
constexpr int64_t kMaxUnits = (int64_t)1 << 31;  // the gather counts a column's units in 32 bits

// ---- the archive: the state block of n_cells envs ----
constexpr int64_t archive_bytes(int64_t n_cells, int n_ships) { return state_host::layout(n_cells, n_ships).bytes; }

// what shipsim_archive_store / _load refuse before they look at the handle's state
enum Arg { kArgOk = 0, kArgNullArchive, kArgNullIndex, kArgCells, kArgBytes, kArgAlign };

inline Arg check_args(const void* archive, const void* index, int64_t bytes, int32_t n_cells, int n_ships) {
  if (!archive) return kArgNullArchive;
  if (!index) return kArgNullIndex;
  if (n_cells < 1 || n_cells > kMaxCells) return kArgCells;
  if (bytes != archive_bytes(n_cells, n_ships)) return kArgBytes;
  if ((uintptr_t)archive & 15) return kArgAlign;
  return kArgOk;
}

constexpr bool elect_sizes_ok(int32_t n_envs, int32_t n_cells) {
  return n_envs >= 1 && n_envs <= kMaxEnvs && n_cells >= 1 && n_cells <= kMaxCells;
}

// ---- the gather between two tables ----
// Slot d of the destination (a cell on a store, an env on a load) takes the share of slot index[d] of the source in
// every column. Both tables list the same columns at the same bytes per env and the same access width (they are
// state_host::table() of two layouts of one ship count): only the offsets differ.
constexpr bool tables_match(const state_host::Table& a, const state_host::Table& b) {
  for (int c = 0; c < state_host::kColumns; ++c)
    if (a.col[c].env_bytes != b.col[c].env_bytes || a.col[c].unit != b.col[c].unit) return false;
  return true;
}

// an index is served when it names a slot of the source: tested before any address is formed from it (a negative
// one is >= 2^31 as unsigned)
AR_HD constexpr bool index_ok(int32_t index, uint32_t n_src) { return (uint32_t)index < n_src; }

// Unit t of a destination column belongs to slot t / units_per_env, and is piece t % units_per_env of its share
AR_HD constexpr uint32_t slot_of(const state_host::Column& dst, uint32_t t) { return t / state_host::units_per_env(dst); }
AR_HD constexpr uint32_t piece_of(const state_host::Column& dst, uint32_t t) { return t % state_host::units_per_env(dst); }
// ... it is stored at store_at (consecutive t: consecutive units) and loaded from load_at in the source column
AR_HD constexpr int64_t store_at(const state_host::Column& dst, uint32_t t) { return state_host::unit_dst(dst, t); }
AR_HD constexpr int64_t load_at(const state_host::Column& src, uint32_t from, uint32_t piece) {
  return state_host::unit_src(src, from, piece);
}

// the gather as the kernel runs it, one unit after the other (the host's restatement: memcpy for the vector moves)
inline void gather(const state_host::Table& Ts, const state_host::Table& Td, const unsigned char* src,
                   unsigned char* dst, const int32_t* index, uint32_t n_dst, uint32_t n_src) {
  for (int ci = 0; ci < state_host::kColumns; ++ci) {
    const state_host::Column cs = Ts.col[ci], cd = Td.col[ci];
    const uint32_t total = n_dst * state_host::units_per_env(cd);
    for (uint32_t t = 0; t < total; ++t) {
      const int32_t from = index[slot_of(cd, t)];
      if (!index_ok(from, n_src)) continue;
      memcpy(dst + store_at(cd, t), src + load_at(cs, (uint32_t)from, piece_of(cd, t)), (size_t)cd.unit);
    }
  }
}

// ---- the election ----
// The caller's workspace: byte offsets of its arrays (every one on a multiple of 256) and its size.
//   best   [n_cells] u64: the largest image of a score among the cell's candidates (0: no candidate)
//   winner [n_cells] int32: the lowest env index among the candidates that hold it
//   count  [n_cells] int32: the cell's candidates
struct Layout {
  int64_t best, winner, count, bytes;
};
constexpr int64_t r256(int64_t b) { return (b + 255) & ~(int64_t)255; }
constexpr Layout layout(int32_t n_cells) {
  Layout L{};
  const int64_t M = n_cells;
  int64_t o = 0;
  L.best = o; o += r256(M * 8);
  L.winner = o; o += r256(M * 4);
  L.count = o; o += r256(M * 4);
  L.bytes = o;
  return L;
}
static_assert(layout(1).bytes <= layout(2).bytes && layout(64).bytes < layout(65).bytes &&
                  layout(kMaxCells).bytes < ((int64_t)1 << 27),
              "the workspace does not decrease with n_cells and stays under 128 MiB");

// what shipsim_archive_elect refuses before any device call
inline bool elect_args_ok(int32_t n_envs, int32_t n_cells, const void* cell, const void* score, const void* cell_score,
                          const void* workspace, int64_t workspace_bytes, const void* env_of_cell_out) {
  if (!elect_sizes_ok(n_envs, n_cells)) return false;
  if (!cell || !score || !cell_score || !workspace || !env_of_cell_out) return false;
  return workspace_bytes >= layout(n_cells).bytes && !((uintptr_t)workspace & 15);
}

constexpr int32_t kNoWinner = 0x7FFFFFFF;  // above every env index
constexpr uint64_t kSign = (uint64_t)1 << 63;

// The order-preserving image of a score that is not NaN, from its bits: a > b (IEEE) exactly when image(a) >
// image(b), -0.0 and +0.0 share one image, and every image is > 0 (-inf, the smallest, is 0x000FFFFFFFFFFFFF), so 0
// stands for "no candidate yet" under an unsigned max.
AR_HD constexpr uint64_t image_of_bits(uint64_t b) {
  if (b == kSign) b = 0;  // -0.0 as +0.0
  return (b & kSign) ? ~b : (b | kSign);
}
AR_HD constexpr bool bits_are_nan(uint64_t b) { return (b & ~kSign) > 0x7FF0000000000000ull; }
static_assert(image_of_bits(kSign) == image_of_bits(0) && image_of_bits(0xFFF0000000000000ull) == 0x000FFFFFFFFFFFFFull &&
                  image_of_bits(0x7FF0000000000000ull) == 0xFFF0000000000000ull &&
                  image_of_bits(0xBFF0000000000000ull) < image_of_bits(0x8000000000000001ull) &&
                  image_of_bits(0x8000000000000001ull) < image_of_bits(0) &&
                  image_of_bits(0) < image_of_bits(1) && image_of_bits(1) < image_of_bits(0x3FF0000000000000ull),
              "-inf < -1 < -denormal < 0 < denormal < 1 < inf");

AR_HD inline uint64_t bits_of(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return b;
}

// env i is a candidate of cell `cell` when the cell exists and the score is not NaN
AR_HD inline bool candidate(int32_t cell, uint32_t n_cells, double score) {
  return (uint32_t)cell < n_cells && !bits_are_nan(bits_of(score));
}

// What the last stage does for one cell, given its winner (kNoWinner: none) and the winner's score as given: the
// winner takes the cell when it is empty (a NaN cell_score) or its score is strictly greater. Returns the env that
// takes the cell or -1, and then writes *cell_score.
AR_HD inline int32_t fill_cell(int32_t winner, double winner_score, double* cell_score) {
  if (winner == kNoWinner) return -1;
  const double held = *cell_score;
  if (!(bits_are_nan(bits_of(held)) || winner_score > held)) return -1;
  *cell_score = winner_score;
  return winner;
}

// shipsim_archive_elect on the host, in the stages of the launches: clear, max and count, min, fill. workspace:
// layout(n_cells).bytes bytes. cell_seen and n_improved_out may be NULL.
inline void elect(int32_t n_envs, int32_t n_cells, const int32_t* cell, const double* score, double* cell_score,
                  int32_t* cell_seen, void* workspace, int32_t* env_of_cell_out, int32_t* n_improved_out) {
  const Layout L = layout(n_cells);
  uint64_t* best = (uint64_t*)((char*)workspace + L.best);
  int32_t* winner = (int32_t*)((char*)workspace + L.winner);
  int32_t* count = (int32_t*)((char*)workspace + L.count);
  for (int32_t c = 0; c < n_cells; ++c) {
    best[c] = 0;
    winner[c] = kNoWinner;
    count[c] = 0;
  }
  if (n_improved_out) *n_improved_out = 0;
  for (int32_t i = 0; i < n_envs; ++i)
    if (candidate(cell[i], (uint32_t)n_cells, score[i])) {
      const uint64_t im = image_of_bits(bits_of(score[i]));
      if (im > best[cell[i]]) best[cell[i]] = im;
      count[cell[i]] += 1;
    }
  for (int32_t i = 0; i < n_envs; ++i)
    if (candidate(cell[i], (uint32_t)n_cells, score[i]) && image_of_bits(bits_of(score[i])) == best[cell[i]] &&
        i < winner[cell[i]])
      winner[cell[i]] = i;
  for (int32_t c = 0; c < n_cells; ++c) {
    const int32_t w = winner[c];
    const int32_t got = fill_cell(w, w == kNoWinner ? 0.0 : score[w], &cell_score[c]);
    env_of_cell_out[c] = got;
    if (cell_seen) cell_seen[c] = (int32_t)((uint32_t)cell_seen[c] + (uint32_t)count[c]);
    if (n_improved_out && got >= 0) *n_improved_out += 1;
  }
}

}  // namespace archive_host
