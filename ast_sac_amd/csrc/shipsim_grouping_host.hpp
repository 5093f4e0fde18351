// shipsim_grouping_host.hpp — the host half of the decision streams' slot -> env grouping (shipsim_set_stream_grouping),
// free of the device and of the handle so that it can be compiled and driven on its own (tests/test_stream_grouping_cpu.py
// builds it into a stand-alone program with -fsanitize=address,undefined): which launches group, the size of the
// handle's permutation buffer, an env's sort key, and the ordering the device's rank-by-counting kernel must produce.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "shipsim_launch_host.hpp"

namespace grouping_host {

// The rank kernel compares every env with every other (n^2 key comparisons per launch, against a launch's
// thousands of ticks): cheap up to this many envs, and left off above.
constexpr int32_t kMaxEnvs = 65536;
// keys are clamped to [0, kMaxKey] (an episode is a few thousand ticks)
constexpr int32_t kMaxKey = 1 << 30;

// The switch as shipsim_create leaves it: on for two-ship envs with collav sbmpc, off otherwise (either can be
// changed with shipsim_set_stream_grouping). What grouping shares is the wave's SBMPC pass, so a handle that never
// runs one would pay the ordering kernel for nothing; and waves of like phase do unlike amounts of work, which the
// two-ship streams' launch tail absorbs and the K > 1 streams, which have no tail, do not (measured on the C5
// streams: K = 2 slower by 4 % with grouping, K = 4 faster by 1.4 %; profiles/stream_grouping_ab.json).
inline bool default_on(int collav, int n_ships) { return collav == SHIPSIM_COLLAV_SBMPC && n_ships == 2; }

// whether a launch at this entry point of a handle of n_envs envs runs its envs in grouped order: the decision
// streams only (the sliced step and the recording kernels keep slot = env), when the switch is on
inline bool groups(launch_host::Entry entry, int32_t n_envs, bool on) {
  return on && entry != launch_host::kStep && n_envs >= 1 && n_envs <= kMaxEnvs;
}

// int32 entries of the handle's permutation buffer (0: the handle never groups and holds none)
inline size_t buffer_len(int32_t n_envs) { return n_envs >= 1 && n_envs <= kMaxEnvs ? (size_t)n_envs : 0; }

// An env's key: the ticks since its last reset, from the test ship's clock (reset to 0, advanced by dt per tick) —
// time / dt rounded to the nearest integer, so the clock's accumulated rounding does not reach the key. Anything
// else (a non-finite clock, dt <= 0) sorts first, as key 0. The device forms the same IEEE quotient and rounding.
inline int32_t key_of(double time, double dt) {
  const double q = rint(time / dt);
  if (!(q > 0.0)) return 0;  // (NaN included)
  return q >= (double)kMaxKey ? kMaxKey : (int32_t)q;
}

// env i's slot: the envs that sort before it — a smaller key, or the same key and a smaller index (what one thread
// of the device kernel counts)
inline int32_t rank_of(const int32_t* keys, int32_t n, int32_t i) {
  int32_t r = 0;
  for (int32_t j = 0; j < n; ++j) r += (keys[j] < keys[i] || (keys[j] == keys[i] && j < i)) ? 1 : 0;
  return r;
}

// the reference ordering: slot_env[slot] = env, ascending key, ties by env index (a stable sort of 0 .. n - 1)
inline void reference_order(const int32_t* keys, int32_t n, int32_t* slot_env) {
  for (int32_t i = 0; i < n; ++i) slot_env[i] = i;
  std::stable_sort(slot_env, slot_env + n, [keys](int32_t a, int32_t b) { return keys[a] < keys[b]; });
}

}  // namespace grouping_host
