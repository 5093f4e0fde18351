// shipsim_launch_host.hpp — which ast_step_kernel instantiations the library holds, and which of them serves a
// handle at an entry point. Free of the device and of the handle (plain C++17), so that it can be compiled and
// driven on its own: tests/test_launch_host_cpu.py builds it into a stand-alone program with
// -fsanitize=address,undefined and walks every input. shipsim_kernels.hip expands the list once into its table
// of kernels and launches through launch_host::select(); shipsim_create, shipsim_set_weather and the refusals
// ask the same function.
#pragma once
#include "shipsim.h"

// The step kernels, one row per instantiation: X(DETAILED, COLLAV, LPE, REC, MODE, SLOTS), MODE = entry point
// (0 shipsim_step, 1 shipsim_run_table, 2 shipsim_run_policy) | 4 for per-env weather. DESIGN.md §2 has the families.
// two-ship envs, the config's weather: every machinery and collav; steps at 2..16 lanes per env and the recording
// step at 16, streams at 4..16
#define SHIPSIM_STEP_KERNELS_UNIFORM(X, D, CA)                                                               \
  X(D, CA, 2, false, 0, 2) X(D, CA, 4, false, 0, 2) X(D, CA, 8, false, 0, 2) X(D, CA, 16, false, 0, 2)       \
  X(D, CA, 16, true, 0, 2)                                                                                   \
  X(D, CA, 4, false, 1, 2) X(D, CA, 8, false, 1, 2) X(D, CA, 16, false, 1, 2)                                \
  X(D, CA, 4, false, 2, 2) X(D, CA, 8, false, 2, 2) X(D, CA, 16, false, 2, 2)
// detailed machinery, collav none / sbmpc, per entry point E: K > 1 obstacle ships (16 lanes in 4 or 8 ship slots),
// and per-env weather (two-ship envs at 8 or 16 lanes, K > 1 as without it)
#define SHIPSIM_STEP_KERNELS_DETAILED(X, CA, E)                                                              \
  X(true, CA, 16, false, E, 4) X(true, CA, 16, false, E, 8)                                                  \
  X(true, CA, 8, false, E + 4, 2) X(true, CA, 16, false, E + 4, 2)                                           \
  X(true, CA, 16, false, E + 4, 4) X(true, CA, 16, false, E + 4, 8)
#define SHIPSIM_STEP_KERNELS_COLLAV(X, CA)                                                                   \
  SHIPSIM_STEP_KERNELS_DETAILED(X, CA, 0) SHIPSIM_STEP_KERNELS_DETAILED(X, CA, 1) SHIPSIM_STEP_KERNELS_DETAILED(X, CA, 2)
#define SHIPSIM_STEP_KERNELS(X)                                                                              \
  SHIPSIM_STEP_KERNELS_UNIFORM(X, false, 0) SHIPSIM_STEP_KERNELS_UNIFORM(X, false, 1)                        \
  SHIPSIM_STEP_KERNELS_UNIFORM(X, false, 2) SHIPSIM_STEP_KERNELS_UNIFORM(X, true, 0)                         \
  SHIPSIM_STEP_KERNELS_UNIFORM(X, true, 1) SHIPSIM_STEP_KERNELS_UNIFORM(X, true, 2)                          \
  SHIPSIM_STEP_KERNELS_COLLAV(X, 0) SHIPSIM_STEP_KERNELS_COLLAV(X, 2)

namespace launch_host {

static_assert(SHIPSIM_COLLAV_NONE == 0 && SHIPSIM_COLLAV_SIMPLE == 1 && SHIPSIM_COLLAV_SBMPC == 2,
              "the list above spells collav as 0 / 1 / 2");

// a row of the list as one integer
constexpr int step_key(bool detailed, int collav, int lpe, bool rec, int mode, int slots) {
  return (int)detailed | collav << 1 | (int)rec << 3 | mode << 4 | lpe << 8 | slots << 16;
}

// the entry points (the kernels' CHAIN) and the weather bit of MODE
enum Entry { kStep = 0, kTable = 1, kPolicy = 2 };
constexpr int kWeatherMode = 4;

struct Selection {
  int key;          // step_key of the kernel
  int lpe;          // lanes per env the launch runs at
  bool tail;        // whether the launch may use the stream tail (shipsim_set_stream_tail)
  const char* why;  // NULL, or why no kernel serves this handle at this entry point (key, lpe, tail unset)
};

// ship slots per env: 2 for the two-ship envs, 4 or 8 with K > 1 obstacle ships (n_ships = 1 + K)
constexpr int ship_slots(int n_ships) { return n_ships <= 2 ? 2 : (n_ships <= 4 ? 4 : 8); }

// obstacles the SBMPC optimiser of a kernel with this many ship slots is built for (sbmpc_cooperative_multi<NOB>):
// every slot but the ship under test's, at most SHIPSIM_MAX_OBS (slots past K duplicate a ship)
constexpr int sbmpc_nob(int slots) { return slots - 1 < SHIPSIM_MAX_OBS ? slots - 1 : SHIPSIM_MAX_OBS; }

// The kernel of a handle with this machinery, collav and ship count, whose uniform-weather lanes per env are
// lpe_uniform (2, 4, 8 or 16: shipsim_create), with trajectory recording and per-env weather on or off, at an entry
// point. Results are the same at every lanes-per-env, so where a family has no kernel at lpe_uniform the nearest
// one runs.
inline Selection select(int machinery, int collav, int n_ships, int lpe_uniform, bool recording, bool weather,
                        Entry entry) {
  const bool detailed = machinery == SHIPSIM_MACH_DETAILED;
  const int slots = ship_slots(n_ships);
  if (slots > 2 && (!detailed || collav == SHIPSIM_COLLAV_SIMPLE))
    return {0, 0, false, "detailed machinery and collav none / sbmpc only"};
  if (weather && !detailed)
    return {0, 0, false, "detailed machinery only (no weather kernels for the simplified machinery)"};
  if (weather && collav == SHIPSIM_COLLAV_SIMPLE)
    return {0, 0, false, "collav none / sbmpc only (no weather kernels for collav simple)"};
  if (weather && recording)
    return {0, 0, false, "trajectory recording is on (the recording kernels run the config's weather)"};
  if (entry != kStep && recording) return {0, 0, false, "trajectory recording is on (use shipsim_step)"};
  // (recording is two-ship envs only, shipsim_set_trajectory: with K > 1 there is nothing to record)
  const bool rec = recording && slots == 2;
  const bool l248 = lpe_uniform == 2 || lpe_uniform == 4 || lpe_uniform == 8;
  int lpe = 16;  // K > 1, recording (built for the default layout only), and the default
  if (slots == 2 && !rec) {
    if (weather) lpe = l248 ? 8 : 16;
    else if (entry == kStep) lpe = l248 ? lpe_uniform : 16;
    else lpe = lpe_uniform == 2 ? 4 : (l248 ? lpe_uniform : 16);  // the streams start at 4 lanes
  }
  const int mode = (int)entry | (weather ? kWeatherMode : 0);
  return {step_key(detailed, collav, lpe, rec, mode, slots), lpe, entry != kStep && slots == 2, nullptr};
}

}  // namespace launch_host
