// shipsim_state_host.hpp — the device state block (DevState) as a table of columns: where each state array lies
// in the block, how many bytes of it belong to one env, and the access width that moves it. Free of the device
// and of the handle (plain C++17), so that it can be compiled and driven on its own: tests/test_fork_cpu.py builds
// it into a stand-alone program with -fsanitize=address,undefined. shipsim_create sizes the block with layout();
// shipsim_snapshot / shipsim_restore copy layout().bytes; shipsim_fork hands table() to its gather kernel, which
// moves every column of every env in one launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "shipsim.h"

namespace state_host {

// The arrays of the block, in block order (DevState's accessors index them the same way):
//   ship arrays, one element per [env][ship] slot: kShipDoubles doubles (DevState::f(k): the 17 SHIPSIM_F_* doubles
//   and the logged position SF_LOG_N / SF_LOG_E), then kShipInts int32 (next_wpt, stop, n_route);
//   route arrays, SHIPSIM_MAX_ROUTE doubles per [env][ship] slot: north, east;
//   env arrays (DevState::ev(k)), kEnvBytes[k] bytes per env.
constexpr int kShipDoubles = 19;
constexpr int kShipInts = 3;
constexpr int kShipArrays = kShipDoubles + kShipInts;
constexpr int kRouteArrays = 2;
constexpr int kRouteSlotBytes = SHIPSIM_MAX_ROUTE * (int)sizeof(double);  // 128 B per ship
// bytes per env of env array k: sampling_count | travel_dist, travel_time, acc, n_base, e_base, p_last, chi_last,
// mach_dt | states4 [4] f32 | next_obs8 [8] f32 | snap_bits, was_reset, dec_flags | legacy_states [4] f64 |
// legacy_flags, dec_ticks, dec_action | dec_obs0 [8] f32
constexpr int kEnvBytes[] = {4, 8, 8, 8, 8, 8, 8, 8, 8, 16, 32, 4, 4, 4, 32, 4, 4, 4, 32};
constexpr int kEnvArrays = (int)(sizeof(kEnvBytes) / sizeof(kEnvBytes[0]));
constexpr int kEnvSlotBytes = 32;  // the widest env array: what an env array's stride is sized for
constexpr int kColumns = kShipArrays + kRouteArrays + kEnvArrays;
constexpr int64_t kAlign = 256;  // every array starts on a multiple of it

static_assert(kShipArrays == 22 && kRouteArrays == 2 && kEnvArrays == 19 && kColumns == 43,
              "a state array was added or removed: give it its bytes per env above (shipsim_fork moves the columns "
              "of this table and nothing else), then change these counts");

constexpr bool env_bytes_fit() {
  for (int k = 0; k < kEnvArrays; ++k)
    if (kEnvBytes[k] > kEnvSlotBytes || kEnvBytes[k] % 4) return false;
  return true;
}
static_assert(env_bytes_fit(), "an env array is wider than its slot, or not made of 4-byte words");

// the strides of the block (DevState's) and its size, for n_envs envs of n_ships ships
struct Layout {
  int64_t ship_stride;   // bytes of one ship array
  int64_t route_stride;  // bytes of one route array
  int64_t env_stride;    // bytes of one env array
  int64_t env_off;       // start of the env arrays
  int64_t bytes;         // the whole block
};

constexpr int64_t round_up(int64_t b) { return (b + kAlign - 1) & ~(kAlign - 1); }

constexpr Layout layout(int64_t n_envs, int n_ships) {
  const int64_t slots = n_envs * n_ships;
  const int64_t ship = round_up(slots * (int64_t)sizeof(double));
  const int64_t route = round_up(slots * kRouteSlotBytes);
  const int64_t env = round_up(n_envs * kEnvSlotBytes);
  const int64_t env_off = kShipArrays * ship + kRouteArrays * route;
  return {ship, route, env, env_off, env_off + kEnvArrays * env};
}

// One array of the block as the gather sees it: env i owns bytes [offset + i * env_bytes, offset + (i + 1) *
// env_bytes), moved `unit` bytes at a time (4, 8 or 16; it divides env_bytes, and offset is a multiple of kAlign,
// so every access is aligned to its width in a block aligned to 16).
struct Column {
  int64_t offset;
  int32_t env_bytes;
  int32_t unit;
};

struct Table {
  Column col[kColumns];
};

constexpr int unit_of(int elem_bytes) { return elem_bytes >= 16 ? 16 : elem_bytes; }

constexpr Table table(const Layout& L, int n_ships) {
  Table t = {};
  int c = 0;
  for (int k = 0; k < kShipArrays; ++k) {
    const int elem = k < kShipDoubles ? 8 : 4;
    t.col[c++] = {k * L.ship_stride, elem * n_ships, elem};
  }
  for (int k = 0; k < kRouteArrays; ++k)
    t.col[c++] = {kShipArrays * L.ship_stride + k * L.route_stride, kRouteSlotBytes * n_ships, 16};
  for (int k = 0; k < kEnvArrays; ++k) t.col[c++] = {L.env_off + k * L.env_stride, kEnvBytes[k], unit_of(kEnvBytes[k])};
  return t;
}

// The gather's arithmetic (fork_gather_kernel runs these; constexpr, so the device compiler takes them as they
// are): a column is n_envs * units_per_env(c) units; unit t belongs to env t / units_per_env and is stored at
// unit_dst(c, t); when that env takes the state of env `from` it is loaded from unit_src(c, from, piece), piece =
// t % units_per_env.
constexpr uint32_t units_per_env(const Column& c) { return (uint32_t)(c.env_bytes / c.unit); }
constexpr int64_t unit_dst(const Column& c, uint32_t t) { return c.offset + (int64_t)t * c.unit; }
constexpr int64_t unit_src(const Column& c, uint32_t from, uint32_t piece) {
  return c.offset + (int64_t)from * c.env_bytes + (int64_t)piece * c.unit;
}

// the most units any column holds (what the gather's grid is sized from)
constexpr int64_t max_units(const Table& t, int64_t n_envs) {
  int64_t m = 0;
  for (int c = 0; c < kColumns; ++c) {
    const int64_t u = n_envs * (int64_t)units_per_env(t.col[c]);
    if (u > m) m = u;
  }
  return m;
}

}  // namespace state_host
