// shipsim_kernels.hip — HIP kernels (gfx950) + C ABI (include/shipsim.h) of the batched
// ship-in-transit simulator -> ast_sac_amd/lib/libshipsim.so, linked from this file's object and
// shipsim_c2_pipe.hip's (ast_sac_amd/build_hash.py OBJECTS: this one is built without machine-level LICM, the tick
// loops' constants are rematerialised rather than held in registers).
// The shared device state is shipsim_state.hpp, the ship model shipsim_device.hpp (types: shipsim_types.hpp); the host
// halves that need no device are the shipsim_*_host.hpp headers, shipsim_create's being shipsim_config_host.hpp.
//
// Kernels
//   init_kernel    : state as constructed (ShipModelAST/SimpleShipModel.__init__, controllers,
//                    NavigationSystem, MultiShipRLEnv.__init__ :54-141)
//   reset_kernel   : MultiShipRLEnv.reset (env.py:238-295) incl. init_step (:297-342)
//   ast_step_kernel: MultiShipRLEnv.step (env.py:624-773) — event-driven: each env ticks
//                    (_step :563-622) until its decision point (RoA + 1 tick) or done
//   single_tick_kernel: C2 single-ship loop body (run_colav/run_simplified_model.py:248-249 shape)
//   single_tick_pipe_kernel: the same for the simplified machinery, three waves per 64 ships (shipsim_c2_pipe.hip)
//   fork_gather_kernel: shipsim_fork — env i takes env src_env[i]'s share of every column of the state block
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>

#include "shipsim.h"
#include "shipsim_device.hpp"
#include "shipsim_state.hpp"         // DevState, ConstBuf, load_ship / store_ship, stage_consts
#include "shipsim_config_host.hpp"   // shipsim_default_config and shipsim_create's host half
#include "shipsim_launch_host.hpp"   // the list of step kernels and the choice among them
#include "shipsim_weather_host.hpp"  // shipsim_set_weather's host half
#include "shipsim_grouping_host.hpp" // shipsim_set_stream_grouping's host half
#include "shipsim_state_host.hpp"    // the state block as a table of columns (snapshot / restore / fork)
#include "shipsim_archive_host.hpp"  // shipsim_archive_store / _load's host half

#include "shipsim_diag.hpp"  // diagnostics / ablation hooks (none in the product build)

// Steps of the headline sbmpc streams' pass-free SBMPC answer (ast_step_kernel: SB_NOM, SB_NOM_ALG), a bit per step
// for the narrowed timing variants of scripts/build_variant.sh: 1 the test, 2 its course terms without the atan;
// 0 is the tick without the test. The product has both.
#ifndef SHIPSIM_SB_NOMINAL
#define SHIPSIM_SB_NOMINAL 3
#endif
// Steps of the headline streams' own evaluation of the tick's math-library calls (ast_step_kernel: TMB; TickMath,
// shipsim_device.hpp), a bit per step the same way: 1 atan and exp restated, 2 sincos(yaw) as the restated
// small-argument path under one guard, 4 the constants by row broadcast; 0 is the tick on the device library.
#ifndef SHIPSIM_TICK_MATH
#define SHIPSIM_TICK_MATH 7
#endif

using namespace shipsim;
static_assert(kWeatherCols == weather_host::kCols && WX_WIND_SPEED == weather_host::kWindSpeed &&
                  WX_WIND_SIN == weather_host::kWindSin && WX_WIND_COS == weather_host::kWindCos &&
                  WX_VC_N == weather_host::kCurrentN && WX_VC_E == weather_host::kCurrentE,
              "the weather array's columns: device and host agree");

// Trajectory record (shipsim_set_trajectory): simulation_results rows per ship, RewardTracker rows per
// env. Row t of a ship is its t-th store_simulation_data since reset (row 0 = init_step); env row t is
// the reward of tick t + 1 of the episode. Rows past `cap` are dropped; len keeps counting.
struct Traj {
  double* ship;   // [q][cap][SHIPSIM_TRAJ_SHIP_COLS]
  double* env;    // [env][cap][SHIPSIM_TRAJ_ENV_COLS] (may be null)
  double* fuel;   // [q][3] fuel accumulators (library-owned)
  int32_t* len;   // [env] ship rows recorded since reset
  int32_t cap;
  __device__ __forceinline__ double* ship_row(int q, int t) const {
    return (t >= 0 && t < cap) ? ship + ((size_t)q * cap + t) * SHIPSIM_TRAJ_SHIP_COLS : nullptr;
  }
  __device__ __forceinline__ double* env_row(int e, int t) const {
    return (env && t >= 0 && t < cap) ? env + ((size_t)e * cap + t) * SHIPSIM_TRAJ_ENV_COLS : nullptr;
  }
};

// control half of one ship tick: autopilot -> speed control -> (simple collav) -> store
// (env.py test_step :389-433 / obs_step :481-512 / init_step :309-339); returns (ctrl, rudder)
// PRE: (pre_q, pre_e) = los_q at (s.n, s.e) on the current segment, evaluated earlier in the tick; used unless the
// waypoint index advances here
// PP: Params, or its register copy in the kernels that hold one (TickConstRegs)
// TM: how the course correction's atan is evaluated (TickMath; the device library's unless the caller says otherwise)
template <bool DETAILED, bool REC, bool PRE = false, class PP, class TM = TickMath<0>>
__device__ __forceinline__ void control_and_store(const ShipConst& c, const PP& P, Ship& s,
                                                  const double* __restrict__ rn, const double* __restrict__ re,
                                                  double offset, double speed_factor, double mach_dt,
                                                  int simple_collav_flag /*0 none, 1 rl(-15deg), 2 noniw(+15)*/,
                                                  bool imminent, double* row, double* fuel, double& ctrl_out,
                                                  double& rudder_out, double pre_q = 0.0, double pre_e = 0.0,
                                                  const TM& tm = TM()) {
  const double N = s.n, E = s.e, H = s.yaw, U = s.u;
  double href;
  if constexpr (PRE) {
    double q = pre_q, e_ct = pre_e;
    if (next_wpt_advance(c, s, N, E)) {
      s.next_wpt += 1;
      load_segment(s, rn, re);
      q = los_q(c, s, N, E, e_ct);
    }
    s.e_ct = e_ct;
    href = s.seg_alpha + tm.atan_los(los_windup(c, s, q));
  } else {
    if (next_wpt_advance(c, s, N, E)) {
      s.next_wpt += 1;
      load_segment(s, rn, re);
    }
    href = los_guidance(c, s, N, E);
  }
  double rudder = heading_ctrl(c, s, href + offset, H, P.dt, c.rcp_dt);
  double ctrl = speed_ctrl(c, s, c.desired_speed * speed_factor, U, P.dt, DETAILED, c.rcp_dt);
  if (simple_collav_flag && imminent) {
    ctrl *= 0.5;
    ctrl = py_min(py_max(ctrl, 0.0), 1.1);
    rudder += (simple_collav_flag == 1 ? -15.0 : 15.0) * (kPi / 180.0);
    rudder = py_min(py_max(rudder, -c.max_rudder), c.max_rudder);
  }
  // store_simulation_data (the fields later read back through simulation_results[-1])
  s.log_rudder = rudder;
  s.log_ect = s.e_ct;
  s.log_n = N;
  s.log_e = E;
  s.log_thrust = DETAILED ? (c.thrust_coeff * s.omega * fabs(s.omega)) / 1000 : ctrl;
  if (REC) {  // the full store_simulation_data row (ship_model.py:903-942) + ShipAssets trackers
    if (DETAILED) fuel_consumption(c, ctrl, mach_dt, fuel);
    if (row) {
      row[SHIPSIM_TS_TIME] = s.time; row[SHIPSIM_TS_NORTH] = N; row[SHIPSIM_TS_EAST] = E;
      row[SHIPSIM_TS_YAW] = H; row[SHIPSIM_TS_RUDDER] = rudder; row[SHIPSIM_TS_U] = U;
      row[SHIPSIM_TS_V] = s.v; row[SHIPSIM_TS_R] = s.r; row[SHIPSIM_TS_OMEGA] = DETAILED ? s.omega : 0.0;
      row[SHIPSIM_TS_THRUST] = DETAILED ? c.thrust_coeff * s.omega * fabs(s.omega) : ctrl;
      row[SHIPSIM_TS_E_CT] = s.e_ct; row[SHIPSIM_TS_E_PSI] = fabs(H - href); row[SHIPSIM_TS_LOAD] = ctrl;
      row[SHIPSIM_TS_FUEL_ME] = DETAILED ? fuel[0] : 0.0; row[SHIPSIM_TS_FUEL_EL] = DETAILED ? fuel[1] : 0.0;
      row[SHIPSIM_TS_FUEL] = DETAILED ? fuel[2] : 0.0; row[SHIPSIM_TS_E_CT_INT] = s.e_ct_int;
      row[SHIPSIM_TS_NEXT_WPT] = (double)s.next_wpt; row[SHIPSIM_TS_REPEAT] = 0.0;
      row[SHIPSIM_TS_TIME_LIST] = s.time;
    }
  }
  ctrl_out = ctrl;
  rudder_out = rudder;
}

// one controlled ship tick: autopilot -> speed control -> store -> update -> integrate -> next_time
// with the reference's angle-form wind force (PAIRED: sub-lanes 2k / 2k+1 share the batched sincos
// calls, odd = this lane is 2k+1) or the algebraic one (ALGW, (wsin, wcos) = sin/cos(wind_direction)).
// The legacy per-tick kernel and the C2 single-ship kernel use this form.
template <bool DETAILED, bool REC = false, bool PAIRED = false, bool ALGW = false>
__device__ __forceinline__ void control_and_integrate(const ShipConst& c, const Params& P, Ship& s,
                                                      const double* __restrict__ rn, const double* __restrict__ re,
                                                      double offset, double speed_factor, double mach_dt,
                                                      int simple_collav_flag, bool imminent, double* row = nullptr,
                                                      double* fuel = nullptr, bool odd = false, double wsin = 0.0,
                                                      double wcos = 1.0) {
  double ctrl, rudder;
  control_and_store<DETAILED, REC>(c, P, s, rn, re, offset, speed_factor, mach_dt, simple_collav_flag, imminent, row,
                                   fuel, ctrl, rudder);
  Deriv d = differentials<PAIRED, ALGW>(c, P, s, ctrl, rudder, DETAILED, odd, wsin, wcos);
  integrate(s, d, P.dt, mach_dt, DETAILED);
}

// the same tick in the AST kernels (step, decision stream, reset / init_step): algebraic wind force
// and sin/cos(yaw) carried in (sy, cy) — valid for s.yaw on entry, refreshed after the integration
// step, so one sincos per ship-tick serves both the kinematics and the reward's encounter angle.
// W: the weather's source, Params or the env's LaneWeather (differentials_sc).
template <bool DETAILED, bool REC = false, bool PRE = false, class W = Params, class PP>
__device__ __forceinline__ void control_and_integrate_sc(const ShipConst& c, const PP& P, const W& wx, Ship& s,
                                                         const double* __restrict__ rn,
                                                         const double* __restrict__ re, double offset,
                                                         double speed_factor, double mach_dt, int simple_collav_flag,
                                                         bool imminent, double* row, double* fuel, double& sy,
                                                         double& cy, double pre_q = 0.0, double pre_e = 0.0) {
  double ctrl, rudder;
  control_and_store<DETAILED, REC, PRE>(c, P, s, rn, re, offset, speed_factor, mach_dt, simple_collav_flag, imminent,
                                        row, fuel, ctrl, rudder, pre_q, pre_e);
  Deriv d = differentials_sc(c, wx, s, ctrl, rudder, DETAILED, sy, cy);
  integrate(s, d, P.dt, mach_dt, DETAILED);
  sincos(s.yaw, &sy, &cy);
}
// the same with the tick's new position (n1, e1) formed by the caller before the control chain (early_pose); TM: the
// atan and the sincos as the caller's TickMath evaluates them
template <bool DETAILED, bool REC = false, bool PRE = false, class W = Params, class PP, class TM = TickMath<0>>
__device__ __forceinline__ void control_and_integrate_sc(const ShipConst& c, const PP& P, const W& wx, Ship& s,
                                                         const double* __restrict__ rn,
                                                         const double* __restrict__ re, double offset,
                                                         double speed_factor, double mach_dt, double n1, double e1,
                                                         double& sy, double& cy, double pre_q, double pre_e,
                                                         const TM& tm = TM()) {
  double ctrl, rudder;
  control_and_store<DETAILED, REC, PRE>(c, P, s, rn, re, offset, speed_factor, mach_dt, 0, false, nullptr, nullptr, ctrl,
                                        rudder, pre_q, pre_e, tm);
  Deriv d = differentials_sc(c, wx, s, ctrl, rudder, DETAILED, sy, cy);
  integrate(s, d, n1, e1, P.dt, mach_dt, DETAILED);
  tm.sincos_yaw(s.yaw, &sy, &cy);
}

// store_last_simulation_data (ship_model.py:946-957) of a stopped ship: the previous row repeated
// with the current time; ShipAssets.time_list gets the time after the first next_time (env.py:451-465)
__device__ __forceinline__ void record_last(const Traj& T, int q, int t, double time, double time_list) {
  double* row = T.ship_row(q, t);
  const double* prev = T.ship_row(q, t - 1);
  if (!row || !prev) return;
  for (int k = 0; k < SHIPSIM_TRAJ_SHIP_COLS; ++k) row[k] = prev[k];
  row[SHIPSIM_TS_TIME] = time;
  row[SHIPSIM_TS_REPEAT] = 1.0;
  row[SHIPSIM_TS_TIME_LIST] = time_list;
}

#include "shipsim_sbmpc.hpp"  // the wave-cooperative SBMPC optimiser

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// fresh state as constructed; for AST also env-level fields of MultiShipRLEnv.__init__
__global__ void init_kernel(const Params P, DevState S, ConstBuf K) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq = P.n_envs * P.n_ships;
  if (q >= nq) return;
  const int ship = q % P.n_ships;
  const int env = q / P.n_ships;
  const ShipConst& c = K.ships()[ship];
  Ship s;
  s.n = c.init_n; s.e = c.init_e; s.yaw = c.init_yaw; s.u = c.init_u; s.v = c.init_v; s.r = c.init_r;
  s.omega = c.init_omega; s.time = 0.0;
  s.e_ct = 0; s.e_ct_int = 0; s.hdg_ei = 0; s.hdg_prev = 0;
  s.spd_a = 0; s.spd_b = (P.machinery == SHIPSIM_MACH_DETAILED) ? c.init_shaft_ei : 0.0;
  s.log_rudder = 0; s.log_thrust = 0; s.log_ect = 0; s.log_n = s.n; s.log_e = s.e;
  s.next_wpt = 1; s.stop = 0; s.n_route = c.n_route;
  double* rn = S.route_n() + (size_t)q * kMaxRoute;
  double* re = S.route_e() + (size_t)q * kMaxRoute;
  for (int i = 0; i < kMaxRoute; ++i) {
    rn[i] = K.cfg_route_n()[ship * kMaxRoute + i];
    re[i] = K.cfg_route_e()[ship * kMaxRoute + i];
  }
  store_ship(S, q, s);
  if (ship == 0) {
    S.sampling_count()[env] = 0;
    S.travel_dist()[env] = 0; S.travel_time()[env] = 0; S.acc()[env] = 0;
    S.n_base()[env] = P.n_base0; S.e_base()[env] = P.e_base0;
    S.p_last()[env] = 1.0; S.chi_last()[env] = 0.0;  // SBMPCParams defaults (sbmpc.py:28-29)
    S.mach_dt()[env] = P.mach_dt_init;
    for (int i = 0; i < 4; ++i) S.states4()[env * 4 + i] = P.initial_states[i < 2 ? i : i + 1];
    for (int i = 0; i < 8; ++i) S.next_obs8()[env * 8 + i] = P.initial_states[i];
    S.snap_bits()[env] = 0;
    S.was_reset()[env] = 0;
    S.dec_flags()[env] = DF_AWAITING;
    for (int i = 0; i < 4; ++i) S.legacy_states()[env * 4 + i] = 0.0;
    S.legacy_flags()[env] = 1;
  }
}

// Per-env weather (shipsim_set_weather) in the AST kernels. WX kernels read the five values of the lane's env
// once per launch from the handle's weather array (load_weather) and hold them in registers; every other kernel
// reads Params where the value is used, as before (weather_of picks the source at compile time, so the uniform
// kernels see the expressions they always had and compile to the code they had).
struct NoWeather {};
template <class PP>  // (PP: Params or its register copy)
__device__ __forceinline__ const PP& weather_of(const PP& P, const NoWeather&) { return P; }
template <class PP>
__device__ __forceinline__ const LaneWeather& weather_of(const PP&, const LaneWeather& w) { return w; }
__device__ __forceinline__ void load_weather(NoWeather&, const double*, int, int) {}
__device__ __forceinline__ void load_weather(LaneWeather& w, const double* __restrict__ wx, int n_envs, int env) {
  w.wind_speed = wx[(size_t)WX_WIND_SPEED * n_envs + env];
  w.wind_sin = wx[(size_t)WX_WIND_SIN * n_envs + env];
  w.wind_cos = wx[(size_t)WX_WIND_COS * n_envs + env];
  w.vc_n = wx[(size_t)WX_VC_N * n_envs + env];
  w.vc_e = wx[(size_t)WX_VC_E * n_envs + env];
}

// MultiShipRLEnv.reset (env.py:238-295): reset assets + IW sampler + snapshot, then init_step
template <bool DETAILED, bool REC>
__global__ __launch_bounds__(256) void reset_kernel(const Params P, DevState S, ConstBuf K, Traj T,
                                                   const uint8_t* mask, float* obs_out) {
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  const ShipConst* SC = stage_consts(K, lds_sc, P.n_ships, P.dt);
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq = P.n_envs * P.n_ships;
  if (q >= nq) return;
  const int ship = q % P.n_ships;
  const int env = q / P.n_ships;
  if (mask && !mask[env]) return;
  const ShipConst& c = SC[ship];
  Ship s;
  s.n = c.init_n; s.e = c.init_e; s.yaw = c.init_yaw; s.u = c.init_u; s.v = c.init_v; s.r = c.init_r;
  s.omega = c.init_omega; s.time = 0.0;
  s.e_ct = 0; s.e_ct_int = 0; s.hdg_ei = 0; s.hdg_prev = 0;
  s.spd_a = 0; s.spd_b = DETAILED ? c.init_shaft_ei : 0.0;
  s.next_wpt = 1; s.stop = 0; s.n_route = c.n_route;
  double* rn = S.route_n() + (size_t)q * kMaxRoute;
  double* re = S.route_e() + (size_t)q * kMaxRoute;
  for (int i = 0; i < c.n_route; ++i) {
    rn[i] = K.cfg_route_n()[ship * kMaxRoute + i];
    re[i] = K.cfg_route_e()[ship * kMaxRoute + i];
  }
  load_segment(s, rn, re);
  const double mach_dt = P.mach_dt_reset;
  // init_step (env.py:307-339): one control + integrate tick, no collision avoidance
  double fuel[3] = {0.0, 0.0, 0.0};  // machinery reset restores the fuel accumulators (ship_engine.py:468-481)
  double sy, cy;
  sincos(s.yaw, &sy, &cy);
  control_and_integrate_sc<DETAILED, REC>(c, P, P, s, rn, re, 0.0, 1.0, mach_dt, 0, false,
                                          REC ? T.ship_row(q, 0) : nullptr, fuel, sy, cy);
  store_ship(S, q, s);
  if (REC) {
    for (int k = 0; k < 3; ++k) T.fuel[(size_t)q * 3 + k] = fuel[k];
    if (ship == 0) T.len[env] = 1;
  }
  if (ship == 0) {
    S.sampling_count()[env] = 0;
    S.travel_dist()[env] = 0; S.travel_time()[env] = 0; S.acc()[env] = 0;
    S.n_base()[env] = P.n_base0; S.e_base()[env] = P.e_base0;
    S.mach_dt()[env] = mach_dt;
    for (int i = 0; i < 8; ++i) S.next_obs8()[env * 8 + i] = P.initial_states[i];
    S.snap_bits()[env] = 0;
    S.was_reset()[env] = 1;
    S.dec_flags()[env] = DF_AWAITING;
    if (obs_out)
      for (int i = 0; i < 8; ++i) obs_out[env * 8 + i] = P.initial_states[i];
  }
}

// reset_kernel for a handle with per-env weather (detailed machinery, no recording: shipsim_set_weather): the
// same statements, the init_step under the env's weather. Its own kernel, so that reset_kernel stays the code it was.
__global__ __launch_bounds__(256) void reset_wx_kernel(const Params P, DevState S, ConstBuf K, const uint8_t* mask,
                                                      float* obs_out, const double* __restrict__ wx) {
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  const ShipConst* SC = stage_consts(K, lds_sc, P.n_ships, P.dt);
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int nq = P.n_envs * P.n_ships;
  if (q >= nq) return;
  const int ship = q % P.n_ships;
  const int env = q / P.n_ships;
  if (mask && !mask[env]) return;
  const ShipConst& c = SC[ship];
  Ship s;
  s.n = c.init_n; s.e = c.init_e; s.yaw = c.init_yaw; s.u = c.init_u; s.v = c.init_v; s.r = c.init_r;
  s.omega = c.init_omega; s.time = 0.0;
  s.e_ct = 0; s.e_ct_int = 0; s.hdg_ei = 0; s.hdg_prev = 0;
  s.spd_a = 0; s.spd_b = c.init_shaft_ei;
  s.next_wpt = 1; s.stop = 0; s.n_route = c.n_route;
  double* rn = S.route_n() + (size_t)q * kMaxRoute;
  double* re = S.route_e() + (size_t)q * kMaxRoute;
  for (int i = 0; i < c.n_route; ++i) {
    rn[i] = K.cfg_route_n()[ship * kMaxRoute + i];
    re[i] = K.cfg_route_e()[ship * kMaxRoute + i];
  }
  load_segment(s, rn, re);
  const double mach_dt = P.mach_dt_reset;
  double sy, cy;
  sincos(s.yaw, &sy, &cy);
  LaneWeather lw;
  load_weather(lw, wx, P.n_envs, env);
  control_and_integrate_sc<true, false>(c, P, lw, s, rn, re, 0.0, 1.0, mach_dt, 0, false, nullptr, nullptr, sy, cy);
  store_ship(S, q, s);
  if (ship == 0) {
    S.sampling_count()[env] = 0;
    S.travel_dist()[env] = 0; S.travel_time()[env] = 0; S.acc()[env] = 0;
    S.n_base()[env] = P.n_base0; S.e_base()[env] = P.e_base0;
    S.mach_dt()[env] = mach_dt;
    for (int i = 0; i < 8; ++i) S.next_obs8()[env * 8 + i] = P.initial_states[i];
    S.snap_bits()[env] = 0;
    S.was_reset()[env] = 1;
    S.dec_flags()[env] = DF_AWAITING;
    if (obs_out)
      for (int i = 0; i < 8; ++i) obs_out[env * 8 + i] = P.initial_states[i];
  }
}

// Map edge table with the per-edge constants of GEOS pointToSegment, staged in LDS.
struct EdgeX {
  double ax, ay, bx, by, dx, dy, len2, inv_len2;
};

// min over this lane's share of the edges (i = sub, sub + nsub, ...) of the squared point-segment
// distance. Equivalent to GEOS Distance::pointToSegment up to rounding (sqrt taken once at the end).
__device__ __forceinline__ double map_dist2_part(const EdgeX* __restrict__ E, int n_edges, double n, double e,
                                                 int sub, int nsub) {
  const double px = e, py = n;
  double best = INFINITY;
  for (int i = sub; i < n_edges; i += nsub) {
    const EdgeX ed = E[i];
    const double qx = px - ed.ax, qy = py - ed.ay;
    const double t = qx * ed.dx + qy * ed.dy;
    const double da = qx * qx + qy * qy;
    const double rx = px - ed.bx, ry = py - ed.by;
    const double db = rx * rx + ry * ry;
    const double c = (ed.ay - py) * ed.dx - (ed.ax - px) * ed.dy;
    const double dp = c * c * ed.inv_len2;
    const double d2 = (t <= 0.0) ? da : ((t >= ed.len2) ? db : dp);
    best = py_min(best, d2);
  }
  return best;
}

// this sub-lane's share of grid cell c's candidate edges: the set bits of rank = sub (mod nsub), read from the
// host-split masks (rank mod 8; nsub divides 8) — the min over the shares is over the same edges either way
__device__ __forceinline__ uint64_t grid_share(const ConstBuf& K, int c, int sub, int nsub) {
  uint64_t m = 0;
  for (int q = sub; q < 8; q += nsub) m |= K.grid_part[(size_t)c * 8 + q];
  return m;
}

// map_dist2_part over the edges of mask m (a grid cell's share): the same value as map_dist2_part over every edge
// when the true distance is <= kGroundReach (see above)
__device__ __forceinline__ double map_dist2_mask(const EdgeX* __restrict__ E, uint64_t m, double n, double e) {
  const double px = e, py = n;
  double best = INFINITY;
  while (m) {
    const int i = __builtin_ctzll(m);
    m &= m - 1;
    const EdgeX ed = E[i];
    const double qx = px - ed.ax, qy = py - ed.ay;
    const double t = qx * ed.dx + qy * ed.dy;
    const double da = qx * qx + qy * qy;
    const double rx = px - ed.bx, ry = py - ed.by;
    const double db = rx * rx + ry * ry;
    const double cc = (ed.ay - py) * ed.dx - (ed.ax - px) * ed.dy;
    const double dp = cc * cc * ed.inv_len2;
    const double d2 = (t <= 0.0) ? da : ((t >= ed.len2) ? db : dp);
    best = py_min(best, d2);
  }
  return best;
}

// a double as a value of its own: an expression the compiler can neither sink into a branch nor re-evaluate
__device__ __forceinline__ double pinned_d(double x) {
  asm("" : "+v"(x));
  return x;
}

// map_dist2_mask with the next set bit's edge read from LDS before the current edge's arithmetic, and every field
// of an edge read at once: the same expressions on the same values, the min taken in the same order
__device__ __forceinline__ double map_dist2_mask_pf(const EdgeX* __restrict__ E, uint64_t m, double n, double e) {
  const double px = e, py = n;
  double best = INFINITY;
  if (m) {
    EdgeX ed = E[__builtin_ctzll(m)];
    m &= m - 1;
    bool more;
    do {
      more = m != 0;
      const EdgeX nx = E[more ? __builtin_ctzll(m) : 0];  // (no further bit: edge 0, read and not used)
      m &= m - 1;
      __builtin_amdgcn_sched_barrier(0);  // (the reads issue here, not after the arithmetic they run under)
      const double qx = px - ed.ax, qy = py - ed.ay;
      const double t = qx * ed.dx + qy * ed.dy;
      const double da = qx * qx + qy * qy;
      const double rx = px - ed.bx, ry = py - ed.by;
      const double db = rx * rx + ry * ry;
      const double cc = (ed.ay - py) * ed.dx - (ed.ax - px) * ed.dy;
      const double dp = cc * cc * ed.inv_len2;
      // (the three candidates as values the selects cannot be turned back into branches around)
      const double va = pinned_d(da), vb = pinned_d(db), vp = pinned_d(dp);
      const double d2 = (t <= 0.0) ? va : ((t >= ed.len2) ? vb : vp);
      best = py_min(best, d2);
      ed = nx;
    } while (more);
    // the last look-ahead read has a use, so the reads stay ahead of the arithmetic instead of moving into the
    // next iteration (it completed under the last edge's arithmetic)
    asm volatile("" ::"v"(ed.ax), "v"(ed.ay), "v"(ed.bx), "v"(ed.by), "v"(ed.dx), "v"(ed.dy), "v"(ed.len2), "v"(ed.inv_len2));
  }
  return best;
}

// if_pos_inside_obstacles with the grid's exact cell classification (full test on mixed cells)
__device__ __forceinline__ bool corner_inside(const ConstBuf& K, const Edge* __restrict__ edges,
                                              const PolyBox* __restrict__ boxes, int n_polys, double n, double e) {
  const int c = K.cell(n, e);
  if (c >= 0) {
    const int f = K.grid_flag[c];
    if (f != GRID_MIXED) return f == GRID_IN;
  }
  return map_inside(edges, boxes, n_polys, n, e);
}

__device__ __forceinline__ double xor_shfl_d(double x, int mask) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __shfl_xor(lo, mask, 64);
  hi = __shfl_xor(hi, mask, 64);
  return __hiloint2double(hi, lo);
}


// Open-loop decision stream (shipsim_run_table, the C3 workload of SURVEY.md §8(d)): actions come
// from a device table, a completed decision is followed at once by the next one and an ended
// episode is reset in place, so an env never idles inside a launch while it has ticks left.
struct ChainArgs {
  const float* table;  // [n_eps][n_dec][n_envs] scoping angles
  int32_t n_eps, n_dec;
  int32_t* ep_idx;     // [env] episode counter (table row = ep % n_eps)
  int32_t* dec_idx;    // [env] decision index within the episode
  int32_t* decisions;  // [env] decisions completed in this call (may be null)
  double* log;         // [env][log_cap][SHIPSIM_DECLOG_COLS] per-decision record (may be null)
  int32_t* log_len;    // [env] records written (counts on past log_cap)
  int32_t log_cap;
  int32_t log_stop;    // an env whose log is full stops for the launch, its next decision pending
  // work-conserving launch tail (shipsim_set_stream_tail): a wave whose envs met max_ticks keeps ticking in chunks
  // of kTailChunk while tail_ctr (waves that met it, zeroed per launch) < the grid, up to tail_extra more ticks
  int32_t* tail_ctr;
  int32_t tail_extra;
  int32_t tail_waves;  // waves of the launch (the grid: one wave per block)
  // shipsim_run_policy: actions from the policy instead of the table (policy != null)
  const float* policy;  // TanhGaussianPolicy parameters, torch order (shipsim_policy.params)
  const float* w2t;     // its fc1 weight transposed, [H][H] (shipsim_policy.w2t)
  int32_t pol_obs, pol_hidden, pol_det;
  uint64_t pol_seed;
  const int64_t* pol_counter;
};


// A copy of the state table whose base pointer the compiler cannot see through: addresses derived
// from it are recomputed where they are used (a few SALU) instead of being hoisted out of the tick
// loop and kept alive in SGPRs for the whole launch (the big kernels are at the SGPR limit).
__device__ __forceinline__ DevState opaque(const DevState& S) {
  DevState o = S;
  asm volatile("" : "+s"(o.base));
  return o;
}

// ---------------------------------------------------------------------------------------------
// The collector's policy inside the decision stream (shipsim_run_policy): TanhGaussianPolicy.forward
// + TanhNormal.sample (gaussian_policy.py:105-118, distributions.py:394-425) or MakeDeterministic's
// tanh(mean) (policies/base.py:54-64) on the observation of every env of the wave that needs its next
// action, evaluated by the whole wave (wave-uniform control flow): up to kPolMaxRows envs per pass share every
// weight load; lane l computes hidden units l, l + 64, ... (fmaf chains from the bias in input order,
// h1 staged in LDS); the heads are reduced across the wave. fp32 as the policy.
// ---------------------------------------------------------------------------------------------
constexpr int kPolMaxRows = 8;
constexpr int kPolMultiRows = 4;  // the K > 1 kernels: 16 lanes per env, so a wave never holds more than 4 envs
constexpr int kPolMaxHidden = 512;

__device__ inline void philox_env(uint32_t c[4], uint32_t k0, uint32_t k1) {  // Philox4x32-10
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ float wave_sum_f(float x) {  // butterfly: every lane gets the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// Must be called by every lane of the wave. want: this lane's env needs its next action (all lanes of an
// env agree); ns: its observation; seq: the env's decisions completed in this call (noise stream index).
// Returns the normalized action a in (-1, 1) for lanes whose env wanted one. The hidden units are taken in slices
// of 256 (one slice up to H = 256, two above): in slice c lane l owns the nj = min(4, (H - 256c) / 64) consecutive
// units [256c + l·nj, 256c + l·nj + nj), so one row of the transposed fc1 weight is one coalesced load per lane (a
// float4 in a full slice) and the h1 rows in LDS are read as broadcast float4s; the fc1 accumulators of one slice
// are live at a time (the register budget of H = 256 at every width), and each lane's head partials run on across
// the slices in unit order. ROWS: the envs served per pass (the acc / pm / ps registers and the rows of lds_h1).
template <int ROWS>
__device__ __forceinline__ float policy_actions(bool want, const float ns[8], int env, bool env_leader, int env_lane0,
                                                int seq, const ChainArgs& CH, float* lds_h1) {
  SHIPSIM_LANE_CHECK(64, 5);
  uint64_t req = __ballot(want && env_leader);
  float act = 0.0f;
  const int lane = threadIdx.x & 63;
  const int H = CH.pol_hidden, n_slices = (H + 255) / 256;
  const float* W1 = CH.policy;  // [H][8] (obs_dim 8: checked by the host)
  asm volatile("" : "+s"(W1));  // (the weight addresses below derived per call, not held across the tick loop)
  // the parameter blocks after W1 [H][8]: b1 [H], W2 [H][H], b2 [H], wm [H], bm, ws [H], bs — their addresses
  // derived where each is read, from a copy of W1 the compiler cannot hoist (no pointer pair live across the pass)
  auto blk = [&](int which) __attribute__((always_inline)) {
    const float* w = W1;
    asm volatile("" : "+s"(w));
    const size_t b1 = (size_t)H * 8, b2 = b1 + H + (size_t)H * H;
    return w + (which == 0 ? b1 : which == 1 ? b2 : which == 2 ? b2 + H : b2 + 2 * (size_t)H + 1);
  };
  constexpr int kJ = 4;  // units per lane per slice, at most
  while (req) {
    // the next (up to) ROWS requesting envs: the lowest set bits of req (no indexed arrays: row e's
    // source lane is recomputed from the mask, so nothing lands in scratch)
    const uint64_t rows = req;
    int E = 0;
    for (uint64_t m = req; m && E < ROWS; m &= m - 1) ++E;
    for (int e = 0; e < E; ++e) req &= req - 1;
    // fc0 + relu for every row, into LDS: unit u = b1[u] + sum_i W1[u][i] x[i], i ascending
    {
      uint64_t m = rows;
      for (int e = 0; e < E; ++e, m &= m - 1) {
        const int src = __ffsll((unsigned long long)m) - 1;
        float x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = __shfl(ns[i], src, 64);
#pragma nounroll
        for (int c = 0; c < n_slices; ++c) {
          const int nj = min(4, (H - 256 * c) >> 6), u0 = 256 * c + lane * nj;
#pragma unroll
          for (int j = 0; j < kJ; ++j) {
            if (j < nj) {
              const int u = u0 + j;
              float h = blk(0)[u];  // (the parameters are 4-byte aligned only: log α leads them)
#pragma unroll
              for (int i = 0; i < 8; ++i) h = fmaf(W1[(size_t)u * 8 + i], x[i], h);
              lds_h1[e * kPolMaxHidden + u] = fmaxf(h, 0.0f);
            }
          }
        }
      }
    }
    __syncthreads();  // (one wave per block)
    // per slice: fc1 + relu, acc[e][j] = b2[u] + sum_k W2[u][k] h1[e][k], k ascending (W2T row k is [H]
    // contiguous), folded into this lane's head partials pm / ps (fmaf chains over its units in order)
    float pm[ROWS], ps[ROWS];
#pragma unroll
    for (int e = 0; e < ROWS; ++e) pm[e] = ps[e] = 0.0f;
#pragma nounroll
    for (int c = 0; c < n_slices; ++c) {
      const int nj = min(4, (H - 256 * c) >> 6), u0 = 256 * c + lane * nj;
      float acc[ROWS][kJ];
      const float* b2 = blk(1);
#pragma unroll
      for (int j = 0; j < kJ; ++j) {
        const float bj = j < nj ? b2[u0 + j] : 0.0f;
#pragma unroll
        for (int e = 0; e < ROWS; ++e) acc[e][j] = bj;
      }
      for (int k = 0; k < H; k += 4) {
        float w[4][kJ];
        if (nj == 4) {  // a full slice: one float4 per row
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const float4 v = *reinterpret_cast<const float4*>(CH.w2t + (size_t)(k + kk) * H + u0);
            w[kk][0] = v.x; w[kk][1] = v.y; w[kk][2] = v.z; w[kk][3] = v.w;
          }
        } else {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < kJ; ++j) w[kk][j] = j < nj ? CH.w2t[(size_t)(k + kk) * H + u0 + j] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < ROWS; ++e) {
          if (e < E) {
            const float4 h4 = *reinterpret_cast<const float4*>(lds_h1 + e * kPolMaxHidden + k);
#pragma unroll
            for (int j = 0; j < kJ; ++j) {
              acc[e][j] = fmaf(w[0][j], h4.x, acc[e][j]);
              acc[e][j] = fmaf(w[1][j], h4.y, acc[e][j]);
              acc[e][j] = fmaf(w[2][j], h4.z, acc[e][j]);
              acc[e][j] = fmaf(w[3][j], h4.w, acc[e][j]);
            }
          }
        }
      }
      float wmj[kJ], wsj[kJ];
      const float *wm = blk(2), *ws = blk(3);
#pragma unroll
      for (int j = 0; j < kJ; ++j) {
        wmj[j] = j < nj ? wm[u0 + j] : 0.0f;
        wsj[j] = j < nj ? ws[u0 + j] : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < ROWS; ++e) {
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
          const float y = fmaxf(acc[e][j], 0.0f);
          pm[e] = fmaf(wmj[j], y, pm[e]);
          ps[e] = fmaf(wsj[j], y, ps[e]);
        }
      }
    }
    // heads (mean, log_std) reduced across the wave, the sample, and the hand-over to the env's lanes
    const float bm = blk(2)[H], bs = blk(3)[H];
    const uint64_t ctr = CH.pol_counter ? (uint64_t)*CH.pol_counter : 0;
    uint64_t m = rows;
#pragma unroll
    for (int e = 0; e < ROWS; ++e) {
      if (e < E) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const float mean = wave_sum_f(pm[e]) + bm;
        const float log_std = fminf(fmaxf(wave_sum_f(ps[e]) + bs, -20.0f), 2.0f);
        float z = mean;
        if (!CH.pol_det) {
          const int e_env = __shfl(env, src, 64), e_seq = __shfl(seq, src, 64);
          uint32_t c[4] = {(uint32_t)e_env, (uint32_t)ctr, (uint32_t)(ctr >> 32), 0x5A100000u ^ (uint32_t)e_seq};
          philox_env(c, (uint32_t)CH.pol_seed, (uint32_t)(CH.pol_seed >> 32));
          const float u1 = ((float)c[0] + 1.0f) * 2.3283064365386963e-10f;
          const float u2 = (float)c[1] * 2.3283064365386963e-10f;
          z = mean + expf(log_std) * (sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2));
        }
        const float a = tanhf(z);
        if (env_lane0 == src) act = a;
      }
    }
    __syncthreads();  // lds_h1 free for the next pass
  }
  return act;
}

// NormalizedBoxEnv's float32 rule (normalized_box_env.py:48-51): lb + (a + 1) * 0.5 * (ub - lb), clipped
__device__ __forceinline__ float denormalize_f32(float a, float lb, float ub) {
  const float x = lb + ((a + 1.0f) * 0.5f) * (ub - lb);
  return fminf(fmaxf(x, lb), ub);
}

// lanes of the env: value of lane k of the env (LPE 16: the env is one DPP row)
template <int LPE, int K>
__device__ __forceinline__ double env_lane_d(double x, int env_lane0) {
  SHIPSIM_LANE_CHECK(LPE, 1);
  if constexpr (LPE == 16) return dpp_d<kDppRowBcast + K>(x);
  else return shfl_d(x, env_lane0 + K);
}
template <int LPE, int K>
__device__ __forceinline__ int env_lane_i(int x, int env_lane0) {
  SHIPSIM_LANE_CHECK(LPE, 2);
  if constexpr (LPE == 16) return dpp_i<kDppRowBcast + K>(x);
  else return __shfl(x, env_lane0 + K, 64);
}

// The env lane that evaluates each reward term's exp (LPE >= 8), and the term of env lane j < 5. Two-ship envs
// (lanes alternate test / obstacle ship, each computing from its own perspective): the obstacle ship's lanes 1 and 3
// take the terms of its own ground distance and cross-track error.
struct RewardTerm {
  double t, o, y, pad;  // target, scale, div_rcp(scale)
};
template <int SLOTS>
__host__ __device__ constexpr int reward_lane(int k) {
  return SLOTS != 2 ? k : k == 0 ? 0 : k == 1 ? 2 : k == 2 ? 4 : k == 3 ? 1 : 3;
}
template <int SLOTS>
__host__ __device__ constexpr int reward_term(int j) {
  return SLOTS != 2 ? j : j == 0 ? 0 : j == 1 ? 3 : j == 2 ? 1 : j == 3 ? 4 : 2;
}
// min of a double / OR of an int over the sub-lanes of one ship (same lane parity) of a 16-lane env:
// quad_perm [2,3,0,1], row_ror 4, row_ror 8 (parity-preserving) — DPP only, no LDS permute
template <int LPE, int SLOTS = 2>
__device__ __forceinline__ void ship_reduce(double& d2, int& gri) {
  SHIPSIM_LANE_CHECK(LPE, 3);
  if constexpr (LPE == 16) {  // sub-lanes of a ship are the lanes of equal index mod SLOTS
    if constexpr (SLOTS == 2) {
      d2 = py_min(d2, dpp_d<kDppQuadXor2>(d2));
      gri |= dpp_i<kDppQuadXor2>(gri);
    }
    if constexpr (SLOTS <= 4) {
      d2 = py_min(d2, dpp_d<kDppRowRor4>(d2));
      gri |= dpp_i<kDppRowRor4>(gri);
    }
    d2 = py_min(d2, dpp_d<kDppRowRor8>(d2));
    gri |= dpp_i<kDppRowRor8>(gri);
  } else {
#pragma unroll
    for (int m = SLOTS; m < LPE; m <<= 1) {
      d2 = py_min(d2, xor_shfl_d(d2, m));
      gri |= __shfl_xor(gri, m, 64);
    }
  }
}

// the OR of an int over the same sub-lanes (ship_reduce without the double)
template <int LPE, int SLOTS = 2>
__device__ __forceinline__ void ship_or(int& gri) {
  SHIPSIM_LANE_CHECK(LPE, 3);
  if constexpr (LPE == 16) {
    if constexpr (SLOTS == 2) gri |= dpp_i<kDppQuadXor2>(gri);
    if constexpr (SLOTS <= 4) gri |= dpp_i<kDppRowRor4>(gri);
    gri |= dpp_i<kDppRowRor8>(gri);
  } else {
#pragma unroll
    for (int m = SLOTS; m < LPE; m <<= 1) gri |= __shfl_xor(gri, m, 64);
  }
}

// |beta| > 165° of get_distance_and_encounter_type (compute_distance.py:16-40): beta =
// wrap(atan2(dy, dx) - heading) and cos(beta) = (dx cos h + dy sin h) / dist, so the overtaking
// sector is c < cos(165°)·dist with c = dx·cos h + dy·sin h (sin/cos(h) carried from the test ship's
// integration step). Within 1e-9·dist of the boundary (and at dist = 0) the reference expression
// itself decides, so the boolean equals the reference's.
__device__ __forceinline__ bool overtaking_sector(double dx, double dy, double dist, double sh, double ch, double h) {
  constexpr double kCos165 = -0.96592582628906831;  // cos(165°)
  const double c = dx * ch + dy * sh;
  const double m = c - kCos165 * dist;
  if (fabs(m) > 1e-9 * dist) return m < 0;
  const double beta = floor_mod((atan2(dy, dx) - h) + kPi, 2 * kPi) - kPi;
  return fabs(beta) > 165.0 * (kPi / 180.0);
}

// Everything ast_step_kernel is launched with, as its one by-value kernel argument. The kernel reads
// it through step_args(): the kernarg segment pointer laundered through an empty asm, so every read is
// a scalar load (constant cache) issued where the value is used. Read as ordinary kernel parameters
// these ~120 loop-invariant dwords were loaded at the entry and held in SGPRs for the whole launch,
// which put the kernel past the SGPR limit and spilled them to VGPR lanes.
struct StepArgs {
  Params P;
  DevState S;
  ConstBuf K;
  Traj T;
  const float* action;
  const uint8_t* active_mask;
  float* obs_out;
  double* reward_out;
  uint8_t* done_out;
  uint32_t* events_out;
  int32_t* ticks_out;
  uint8_t* ready_out;
  ChainArgs CH;
  int32_t max_ticks;
  const double* weather;  // WX kernels: the handle's per-env weather array (kWeatherCols x n_envs), else unread
  // decision streams: the env that slot (block * envs per wave + env row of the wave) runs, a permutation of
  // 0 .. n_envs - 1 (shipsim_set_stream_grouping); NULL, and every other kernel: slot = env
  const int32_t* slot_env;
};
typedef const __attribute__((address_space(4))) StepArgs* StepArgsPtr;
__device__ __forceinline__ const StepArgs& step_args() {
  StepArgsPtr q = (StepArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();  // the kernel's first argument
  asm volatile("" : "+s"(q));
  return *(const StepArgs*)q;
}

// env flag bits exchanged between the two ships of an env every tick
#define XF_GROUND 1
#define XF_END 2
#define XF_OUTSIDE 4
#define XF_ROA 8
#define XF_NONFINITE 16

// MultiShipRLEnv.step (env.py:624-773), sliced: every env of the launch ticks (_step :563-622)
// until its decision point (RoA + one tick, or done) or until `max_ticks` ticks have run in this
// call; an env that paused resumes in the next call without consuming an action. Envs waiting
// for a decision consume action[env] first (IW sampling). LPE lanes per env: lane & 1 selects the
// ship, the LPE/2 sub-lanes of a ship hold identical state, run the control chain redundantly and
// split the map queries (edges for the coastline distance, hull corners for grounding).
// CHAIN (shipsim_run_table): decisions from the device table, chained and episodes reset in place.
// An env whose state goes non-finite completes its decision at once, done, with
// SHIPSIM_EV_NONFINITE | SHIPSIM_EV_TERMINAL, and is counted in S.nonfinite (shipsim_synchronize).
// SLOTS (2, 4, 8): ship slots per env. 2 is the reference's two-ship env (lane & 1 = ship); with
// K > 1 obstacle ships (shipsim_create) ship k sits on the lanes of index k mod SLOTS, and slots past
// the env's last ship repeat that ship (ghost lanes: same state and arithmetic, never stored).
// MODE: CHAIN (0 shipsim_step, 1 shipsim_run_table, 2 shipsim_run_policy), plus kStepWeather for the kernels of a
// handle with per-env weather (shipsim_set_weather): MODE 4, 5, 6. (One parameter for both, so that the kernels
// without weather keep the names, and the code, they had.)
constexpr int kStepWeather = 4;
template <bool DETAILED, int COLLAV, int LPE, bool REC, int MODE = 0, int SLOTS = 2>
__global__ __launch_bounds__(64) void ast_step_kernel(const StepArgs A_arg) {
  constexpr int CHAIN = MODE & 3;
  constexpr bool WX = (MODE & kStepWeather) != 0;
  static_assert(CHAIN <= 2 && MODE < 2 * kStepWeather, "MODE: CHAIN | kStepWeather");
  constexpr bool POLICY = CHAIN == 2;
  (void)A_arg;  // read through step_args() only (see StepArgs)
  const StepArgs& A0 = step_args();
  const Params& P = A0.P;
  const DevState& S = A0.S;
  const ConstBuf& K = A0.K;
  const Traj& T = A0.T;
  const int max_ticks = A0.max_ticks;
  static_assert(!(REC && CHAIN), "trajectory recording runs the per-decision step only");
  static_assert(SLOTS == 2 || (LPE == 16 && !REC && COLLAV != SHIPSIM_COLLAV_SIMPLE), "multi-obstacle layout");
  static_assert(!WX || (DETAILED && !REC && COLLAV != SHIPSIM_COLLAV_SIMPLE), "per-env weather kernels");
  constexpr int NSUB = LPE / SLOTS;
  static_assert(NSUB >= 1 && 8 % NSUB == 0, "sub-lanes per ship must divide 8 (grid_part shares)");
  static_assert(LPE >= 2 && (LPE & (LPE - 1)) == 0 && LPE <= 16, "LPE must be a power of two in [2, 16]");
  constexpr bool SIMPLE = COLLAV == SHIPSIM_COLLAV_SIMPLE;
  constexpr bool OPQ = LPE != 16 || POLICY || SLOTS > 2;  // see opaque_if (measured: LPE-16 two-slot table kernels hold no spills without)
  // the K > 1 policy streams: the policy pass on top of the tightest env kernels. What else would sit in SGPRs
  // across the tick loop (the env-leader mask, the want / stalled / started flags as lane masks, the scalar half
  // of the route addresses, the ship count for the epilogue) is laundered or re-derived where it is used
  constexpr bool OPM = POLICY && SLOTS > 2;
  // The numbers of Params and of ConstBuf's map grid that a tick reads, held in accumulator registers (TickConstRegs,
  // shipsim_device.hpp) for the launch instead of re-read from the kernarg segment on every tick: the two-slot
  // LPE-16 decision streams with detailed machinery, whose ticks otherwise park on those scalar loads with nothing
  // else to issue. ShipConst and RewardTerm stay in LDS: register copies of them measured
  // slower (profiles/reg_consts_ab.json). Every other instantiation reads P / K as before.
  constexpr bool RC_PAR = DETAILED && LPE == 16 && !REC && SLOTS == 2 && (MODE == 1 || MODE == 2) && !SIMPLE;
  // The same streams form the position after the tick's Euler step before the control chain and request a new grid
  // cell's edge share and class there (the ship tick below), and walk the cell's edges with the next edge's LDS
  // reads issued ahead of the current edge's arithmetic (map_dist2_mask_pf): the map query's loads run under other
  // work instead of in front of their first use. The sliced step kernels (MODE 0) keep the query as
  // it was: the tests' independent reference.
  constexpr bool EARLY_MAP = RC_PAR;
  // The same streams run a flattened tick (profiles/tick_waits.md "The tick's control flow"): one
  // `going` region from the pass's hand-out to the end of the tick body instead of a guard per section, with the
  // lane exchanges inside it, and the decision ladder as selects. Every other instantiation keeps the guarded tick
  // (the sliced step kernels: the tests' independent reference).
  constexpr bool FLAT = RC_PAR;
  // Legal because an env is exactly one 16-lane DPP row here and `going` is per env: every exchange after the pass
  // (pair_swap, ship_reduce, ship_or, env_lane_*, the hull corners' shuffle by 4·SLOTS lanes) reads lanes of its own
  // row, so inside one `if (going)` a source lane is active exactly when its destination is. (The SBMPC pass itself
  // is wave-cooperative across envs and stays outside the region.)
  static_assert(!FLAT || (LPE == 16 && SLOTS == 2), "the flat tick: env = one DPP row, going per env");
  // The same streams shorten the tick's serial stream over the ship's idle sub-lanes and by dropping branches whose
  // two sides are pure (DESIGN.md §9 "Roots over sub-lanes, pure branches"). LM_POST: the three square roots after
  // the Euler step (each ship's ground distance, the reward's distance, the obstacle ship's travel step) in one call
  // over the env row, one argument per sub-lane parity and ship, exchanged by DPP (sqrt3_row, shipsim_device.hpp);
  // the call sits inside the flat `going` region and outside every per-ship guard, where the whole row is active.
  // LM_OUT: the map bounds test without short-circuit branches. LM_REQ: the test ship's request block in front of
  // the SBMPC pass on every lane, the obstacle ship's lanes keeping their state by selects. (SHIPSIM_LANE_MATH: a
  // bit per step, for the narrowed timing variants of scripts/build_variant.sh; the product has all three.)
#ifndef SHIPSIM_LANE_MATH
#define SHIPSIM_LANE_MATH 7
#endif
  constexpr bool LM_POST = FLAT && (SHIPSIM_LANE_MATH & 1);
  constexpr bool LM_OUT = FLAT && (SHIPSIM_LANE_MATH & 2);
  constexpr bool LM_REQ = FLAT && (SHIPSIM_LANE_MATH & 4);
  // The same streams with collav sbmpc answer a request whose nominal scenario provably wins (sbmpc_nominal_holds,
  // shipsim_sbmpc_nominal.hpp: memory at rest and the closest approach far enough that the nominal scenario's
  // collision cost stays below every other scenario's own terms) on the requesting env's own lanes: the pass would
  // return (1.0, +0.0) bit for bit, and runs only for the requests left (DESIGN.md §9 "The nominal scenario wins").
  // SB_NOM_ALG: sin / cos of the desired course from the segment's and 1 / sqrt(1 + los_arg²); the atan is left to
  // the requests that go to the pass (sbmpc_nominal_holds_seg). (SHIPSIM_SB_NOMINAL, at the top of the file: a bit per
  // step.)
  constexpr bool SB_NOM = LM_REQ && COLLAV == SHIPSIM_COLLAV_SBMPC && (SHIPSIM_SB_NOMINAL & 1);
  constexpr bool SB_NOM_ALG = SB_NOM && (SHIPSIM_SB_NOMINAL & 2);
  // Three of them (the table streams, and the policy stream with collav sbmpc) evaluate the three math-library calls
  // of the steady tick themselves (TickMath, shipsim_device.hpp; shipsim_tickmath.hpp restates the library operation
  // for operation, so the values are its bits): sincos(yaw) after the Euler step, the LOS course correction's atan and
  // the reward's exp, with their fp64 constants delivered from a table in registers by one row broadcast each
  // (DESIGN.md §9 "The tick's math"). With the tick loop tested at its top only the headline kernel gained by the
  // table (collav none −3.3 %, the policy stream −1.6 %: what the allocator moved to accumulator registers); tested
  // at its bottom, collav none gains 1.4 % and the policy stream 2.5 % (§9 "The tick loop, bottom-tested"). The policy
  // stream with collav none has no bench line of its own and keeps the library's calls. (SHIPSIM_TICK_MATH, at the
  // top of the file: a bit per step.)
  constexpr bool TM_KERNEL = FLAT && !(POLICY && COLLAV != SHIPSIM_COLLAV_SBMPC);
  constexpr int TMB = TM_KERNEL ? ((SHIPSIM_TICK_MATH & 4) ? 7 : (SHIPSIM_TICK_MATH & 3)) : 0;
  using flag_t = std::conditional_t<OPM, int, bool>;  // (OPM: an int in a VGPR, not a lane mask)
  // a flag read / set through the VGPR where OPM. Elsewhere the plain expression, so that every other
  // instantiation compiles to the code it had (the dead arm of a constant condition is not emitted)
#define OPM_GET(x) (OPM ? (decltype(x))opaque_v((int)(x)) : (x))
#define OPM_SET(x, v)                                  \
  {                                                    \
    if constexpr (OPM) x = opaque_v((v) ? 1 : 0);      \
    else x = (v);                                      \
  }
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  __shared__ EdgeX lds_edges[SHIPSIM_MAX_VERTS];
  __shared__ Edge lds_edges_raw[SHIPSIM_MAX_VERTS];
  __shared__ PolyBox lds_boxes[SHIPSIM_MAX_POLYS];
  constexpr int kPolRows = SLOTS > 2 ? kPolMultiRows : kPolMaxRows;  // (64 / LPE <= 4 envs per wave with SLOTS > 2)
  static_assert(SLOTS == 2 || 64 / LPE <= kPolMultiRows, "a policy pass serves every env of the wave");
  __shared__ float lds_pol[POLICY ? kPolRows * kPolMaxHidden : 1];  // shipsim_run_policy: h1 rows
  __shared__ RewardTerm lds_rterm[8];  // the reward exp each lane of an env evaluates: its term's constants
  if constexpr (diag::kPoisonLds) {  // (stale-LDS diagnostics build only)
    diag::poison_lds(lds_sc, sizeof(lds_sc)); diag::poison_lds(lds_edges, sizeof(lds_edges));
    diag::poison_lds(lds_edges_raw, sizeof(lds_edges_raw)); diag::poison_lds(lds_boxes, sizeof(lds_boxes));
    __syncthreads();
  }
  const ShipConst* SC = stage_consts(K, lds_sc, P.n_ships, P.dt);
  for (int i = threadIdx.x; i < K.n_edges; i += blockDim.x) {
    const Edge ed = K.edges()[i];
    EdgeX x;
    x.ax = ed.ax; x.ay = ed.ay; x.bx = ed.bx; x.by = ed.by;
    x.dx = ed.bx - ed.ax; x.dy = ed.by - ed.ay;
    x.len2 = x.dx * x.dx + x.dy * x.dy;
    x.inv_len2 = x.len2 > 0 ? 1.0 / x.len2 : 0.0;
    lds_edges[i] = x;
    lds_edges_raw[i] = ed;
  }
  for (int i = threadIdx.x; i < P.n_polys; i += blockDim.x) lds_boxes[i] = K.boxes()[i];
  if (threadIdx.x < 8) {  // reward_designs.py:33-55 targets / scales, term reward_term(j) for env lane j
    const int j = threadIdx.x, t = j < 5 ? reward_term<SLOTS>(j) : 0;
    const double tg[5] = {0.0, 0.0, 3000.0, 0.0, 500.0};
    const double of[5] = {200000000.0, 175000.0, 1250000.0, 50000.0, 12500.0};
    const double o = j < 5 ? of[t] : 1.0;
    lds_rterm[j] = RewardTerm{j < 5 ? tg[t] : 0.0, o, div_rcp(o), 0.0};
  }
  __syncthreads();

  // one wave per block: envs [blockIdx.x * epw, + epw) on lanes [0, epw * LPE); lanes past them idle
  const int epw = P.epw > 0 && P.epw <= 64 / LPE ? P.epw : 64 / LPE;  // (as step_blocks)
  const int eslot = (int)(threadIdx.x & 63) / LPE;
  int env = (int)blockIdx.x * epw + eslot;
  // The decision streams run the env their slot is given (stream_order_kernel: envs of like episode phase share a
  // wave, so their SBMPC requests fall on the same ticks and share passes). Nothing below knows the slot: state,
  // route, table column, record ring, counters, weather and the policy's noise key all go through env / envc / qc,
  // and an env's results do not depend on its wave-mates. A slot past n_envs stays invalid (slot_env is a
  // permutation, so its entries are < n_envs).
  if constexpr (CHAIN != 0) {
    if (A0.slot_env != nullptr && eslot < epw && env < P.n_envs) env = A0.slot_env[env];
  }
  const int lie = (int)(threadIdx.x & 63) % LPE;
  const int ship = lie % SLOTS;
  const int sub = lie / SLOTS;
  const bool is_test = ship == 0;
  const int nsh = (SLOTS == 2) ? 2 : P.n_ships;
  const bool ghost = (SLOTS > 2) && ship >= nsh;
  const int shipc = ghost ? nsh - 1 : ship;  // the ship this lane simulates
  const bool is_obs1 = shipc == 1;            // "the" obstacle ship (sampling, decisions, observation)
  const int lane = threadIdx.x & 63;
  const int env_lane0 = lane - lie;
  const bool valid = eslot < epw && env < P.n_envs;
  const int envc = valid ? env : 0;
  const int qc = envc * nsh + shipc;
  const ShipConst& c = SC[shipc];
  TickConstRegs rc_par;  // (written and read only where RC_PAR: otherwise no code)
  if constexpr (RC_PAR) rc_par.load(P, K);
  double* rn = S.route_n() + (size_t)qc * kMaxRoute;
  double* re = S.route_e() + (size_t)qc * kMaxRoute;
  if constexpr (OPM) {  // whole addresses in VGPRs: no scalar base held for reset_env / decision_prologue
    asm volatile("" : "+v"(rn));
    asm volatile("" : "+v"(re));
  }

  // (an int laundered where it is set, as have_iw: a bool here stayed a lane mask across the tick loop)
  int running = opaque_if<OPQ>((valid && (A0.active_mask == nullptr || A0.active_mask[envc]) && S.was_reset()[envc]) ? 1 : 0);
  // (ints in VGPRs read by the epilogue: not lane masks held in SGPRs for the whole launch)
  const int touched = opaque_v(running && valid ? 1 : 0);

  Ship s;
  load_ship(S, qc, s);
  double sy, cy;  // sin/cos(s.yaw), refreshed by every integration step
  sincos(s.yaw, &sy, &cy);
  std::conditional_t<WX, LaneWeather, NoWeather> lw;  // WX: this env's weather for the whole launch
  load_weather(lw, A0.weather, P.n_envs, envc);
  int sampling_count = S.sampling_count()[envc];
  double travel_dist = S.travel_dist()[envc], travel_time = S.travel_time()[envc], acc = S.acc()[envc];
  double n_base = S.n_base()[envc], e_base = S.e_base()[envc];
  double p_last = S.p_last()[envc], chi_last = S.chi_last()[envc];
  double mach_dt = S.mach_dt()[envc];
  float st4[4] = {0.f, 0.f, 0.f, 0.f};  // self.states (read by the simple collision check only)
  if (SIMPLE)
    for (int i = 0; i < 4; ++i) st4[i] = S.states4()[envc * 4 + i];
  uint32_t snap_bits = S.snap_bits()[envc];
  int dflags = S.dec_flags()[envc];
  // (an int laundered where it is set and read: a bool here was kept as a lane mask across the tick loop and
  // spilled in the LPE-8 policy kernels)
  int have_iw = opaque_if<OPQ>((dflags & DF_HAVE_IW) ? 1 : 0);
  int phase = (dflags >> DF_PHASE_SHIFT) & 3;
  int dec_ticks = S.dec_ticks()[envc];  // ticks of the decision in progress (across calls)

  float ns[8];
  for (int i = 0; i < 8; ++i) ns[i] = S.next_obs8()[envc * 8 + i];
  int rec_t = 0;
  double fuel[3] = {0.0, 0.0, 0.0};
  if (REC) {
    rec_t = T.len[envc];
    for (int k = 0; k < 3; ++k) fuel[k] = T.fuel[(size_t)qc * 3 + k];
  }
  double out_r = 0.0;
  bool out_done = false;
  flag_t stalled = false;
  int ready = 0;  // (an int: OPQ kernels keep it in a VGPR, not a lane mask merged across the tick loop)
  uint32_t out_bits = 0;
  int out_ticks = 0;
  int ticks = 0;
  int budget = opaque_v(max_ticks);  // this launch's tick quota per env (CHAIN: extended in the launch tail; a VGPR)
  int tail_arrived = 0;  // this wave counted itself on the tail counter (an int: no lane mask held)
  int n_nonfinite = 0;

  SHIPSIM_DEBUG_PRINT(valid ? env : -1, "[dbg] env %d lie %d start: running %d dflags %d sc %d n_base %f phase %d\n", env,
                      lie, (int)running, dflags, sampling_count, n_base, phase);
  // ---- intermediate waypoint sampling (env.py:659-696) for an env that waits for a decision ----
  // CHAIN: episode / decision counters, decisions completed and records written in this call
  int ep_i = 0, dec_i = 0, n_decided = 0, log_n = 0;
  flag_t started_here = false;  // POLICY: the decision in progress started in this launch (its record row holds
                              // its action and observation-of-choice already)
  auto decision_prologue = [&](float sa, float a_log) __attribute__((always_inline)) {
    const StepArgs& A = step_args();
    const Params& P = A.P;
    const ConstBuf& K = A.K;
    if (POLICY && OPM_GET(lie) == 0) {  // what the decision record will report: the action and the observation it saw,
                               // into the record row it will complete in (stores only) and, for a decision
                               // that completes in a later launch, the state
      const DevState So = opaque(A.S);
      So.dec_action()[envc] = a_log;
      for (int i = 0; i < 8; ++i) So.dec_obs0()[envc * 8 + i] = ns[i];
      const ChainArgs& CH = A.CH;
      if (CH.log && log_n < CH.log_cap) {
        double* rec = CH.log + ((size_t)env * CH.log_cap + log_n) * SHIPSIM_DECLOG_COLS;
        rec[SHIPSIM_DL_ACTION] = (double)a_log;
        for (int i = 0; i < 8; ++i) rec[SHIPSIM_DL_OBS0 + i] = (double)ns[i];
      }
    }
    OPM_SET(started_here, true);
    if (P.normalize_action) sa = (sa + 1.0f) / 2.0f * (P.action_high - P.action_low) + P.action_low;
    phase = 0;
    have_iw = opaque_if<OPQ>(0);
    dec_ticks = 0;
    const auto& PT = regs_or<RC_PAR>(rc_par, P);
    if (sampling_count < PT.max_sampling) {
      sampling_count += 1;
      float tn = (float)tan((double)sa);  // np.tan on the float32 scoping angle
      double l_s = fabs(PT.AB_seg * (double)tn);
      double e_s = l_s * P.iw_cos;
      double n_s = l_s * P.iw_sin;
      if (sa > 0) e_s *= -1;
      else n_s *= -1;
      double iw_n = n_base + n_s, iw_e = e_base + e_s;
      n_base = iw_n + P.AB_seg_n;
      e_base = iw_e + P.AB_seg_e;
      if (opaque_if<OPQ>(shipc) == 1) {  // auto_pilot.update_route: list.insert(-1, IW); every sub-lane writes the same bytes
        int L = s.n_route;
        rn[L] = s.end_n; re[L] = s.end_e;
        rn[L - 1] = iw_n; re[L - 1] = iw_e;
        if (s.next_wpt == L - 1) {
          s.wp_n = iw_n;
          s.wp_e = iw_e;
          segment_changed(s);
        }
        s.n_route = L + 1;
      }
      travel_dist = 0;
      travel_time = 0;
      have_iw = opaque_if<OPQ>(1);
      bool fail = corner_inside(K, lds_edges_raw, lds_boxes, P.n_polys, iw_n, iw_e) ||
                  ((iw_n < PT.min_north || iw_n > PT.max_north) || (iw_e < PT.min_east || iw_e > PT.max_east));
      if (fail) {  // env.py:673-693 with obs_ship_IW_sampling_failure_reward (multiplier 2)
        out_r = (acc >= 0) ? -acc * 2.0 : acc * 2.0;
        snap_bits = (snap_bits | SHIPSIM_EV_SAMPLING_FAILURE | SHIPSIM_EV_TERMINAL) &
                    ~(uint32_t)(SHIPSIM_EV_TEST_STOP | SHIPSIM_EV_OBS_STOP);
        out_bits = snap_bits;
        out_done = true;
        out_ticks = 0;
        ready = opaque_if<OPQ>(1);
      } else {
        acc = 0;
      }
    }
  };

  // ---- CHAIN: in-place reset (env.py:238-342, as reset_kernel) and the next decision ----
  if (CHAIN) {
    const ChainArgs& CH = A0.CH;
    ep_i = CH.ep_idx[envc];
    dec_i = CH.dec_idx[envc];
    log_n = CH.log_len ? CH.log_len[envc] : 0;
    if (running && CH.log_stop && log_n >= CH.log_cap) {  // log already full: sit this launch out
      running = opaque_if<OPQ>(0);
      OPM_SET(stalled, (dflags & DF_AWAITING) != 0);
    }
  }
  auto table_action = [&]() __attribute__((always_inline)) -> float {
    const StepArgs& A = step_args();
    const Params& P = A.P;
    const ChainArgs& CH = A.CH;
    SHIPSIM_INDEX_CHECK(ep_i >= 0 && dec_i >= 0 && dec_i < CH.n_dec && envc < P.n_envs, 10);
    return CH.table[((size_t)(ep_i % CH.n_eps) * CH.n_dec + dec_i) * P.n_envs + envc];
  };
  auto reset_env = [&]() __attribute__((always_inline)) {
    const StepArgs& A = step_args();
    const Params& P = A.P;
    const ConstBuf& K = A.K;
    const ShipConst& c = lds_sc[opaque_v(shipc)];
    SHIPSIM_INDEX_CHECK(c.n_route >= 2 && c.n_route <= kMaxRoute, 11);
    s.n = c.init_n; s.e = c.init_e; s.yaw = c.init_yaw; s.u = c.init_u; s.v = c.init_v; s.r = c.init_r;
    s.omega = c.init_omega; s.time = 0.0;
    s.e_ct = 0; s.e_ct_int = 0; s.hdg_ei = 0; s.hdg_prev = 0;
    s.spd_a = 0; s.spd_b = DETAILED ? c.init_shaft_ei : 0.0;
    s.next_wpt = 1; s.stop = 0; s.n_route = c.n_route;
    for (int i = 0; i < c.n_route; ++i) {
      rn[i] = K.cfg_route_n()[shipc * kMaxRoute + i];
      re[i] = K.cfg_route_e()[shipc * kMaxRoute + i];
    }
    load_segment(s, rn, re);
    mach_dt = P.mach_dt_reset;
    sincos(s.yaw, &sy, &cy);
    const auto& PT = regs_or<RC_PAR>(rc_par, P);
    control_and_integrate_sc<DETAILED, false>(c, PT, weather_of(PT, lw), s, rn, re, 0.0, 1.0, mach_dt, 0, false, nullptr,
                                              nullptr, sy, cy);  // init_step
    sampling_count = 0;
    travel_dist = 0; travel_time = 0; acc = 0;
    n_base = P.n_base0; e_base = P.e_base0;
    for (int i = 0; i < 8; ++i) ns[i] = P.initial_states[i];
    snap_bits = 0;
    phase = 0;
    have_iw = opaque_if<OPQ>(0);
  };
  // A decision just completed (ready): record it, reset if the episode ended (done, or n_dec decisions
  // = the rollout's max_path_length), consume the next table action. A sampling failure completes the
  // new decision at once (no tick), hence the loop; after kChainBurst such back-to-back decisions (a
  // table whose actions all fail their sampling) the env stops for this launch with the last decision
  // recorded and the next one pending (DF_AWAITING): the wave keeps ticking its other envs and the
  // next launch resumes exactly there, so results do not depend on the burst bound.
  constexpr int kChainBurst = 8;
  constexpr int kTailChunk = 32;  // launch tail: ticks per extension
  // the next action of every env of the wave that needs one (want): the table entry, or the policy's
  // sample (wave-cooperative, shipsim_run_policy). Wave-uniform. sa: the scoping angle to run, a_log:
  // the action as the decision record reports it (the table's angle / the policy's normalized action).
  auto chain_action = [&](bool want, float& a_log) __attribute__((always_inline)) -> float {
    if constexpr (!POLICY) {
      a_log = want ? table_action() : 0.0f;
      return a_log;
    } else {
      const StepArgs& A = step_args();
      a_log = policy_actions<kPolRows>(want, ns, envc, OPM_GET(lie) == 0, env_lane0, n_decided, A.CH, lds_pol);
      const Params& P = A.P;
      const float lb = P.normalize_action ? -1.0f : P.action_low, ub = P.normalize_action ? 1.0f : P.action_high;
      return denormalize_f32(a_log, lb, ub);  // NormalizedBoxEnv in front of the env
    }
  };
  // Decisions of the wave just completed (ready): record them, reset envs whose episode ended (done, or
  // n_dec decisions = the rollout's max_path_length), start each env's next decision. A sampling failure
  // completes the new decision at once (no tick), hence the loop; after kChainBurst such back-to-back
  // decisions (actions that all fail their sampling) the env stops for this launch with the last decision
  // recorded and the next one pending (DF_AWAITING): the wave keeps ticking its other envs and the next
  // launch resumes exactly there, so results do not depend on the burst bound. With the policy the loop is
  // wave-uniform (the policy is evaluated by the whole wave); with the table each env loops on its own.
  auto chain_next = [&]() __attribute__((always_inline)) {
    for (int burst = 0; POLICY ? __any(ready && running) : (ready && running); ++burst) {
      flag_t want = false;
      if (ready && running) {
        const ChainArgs& CH = step_args().CH;
        if (CH.log && opaque_if<OPQ>(lie) == 0 && log_n < CH.log_cap) {
          double* rec = CH.log + ((size_t)env * CH.log_cap + log_n) * SHIPSIM_DECLOG_COLS;
          rec[SHIPSIM_DL_REWARD] = out_r; rec[SHIPSIM_DL_EVENTS] = (double)out_bits;
          rec[SHIPSIM_DL_DONE] = out_done ? 1.0 : 0.0; rec[SHIPSIM_DL_EPISODE] = (double)ep_i;
          rec[SHIPSIM_DL_DECISION] = (double)dec_i; rec[SHIPSIM_DL_TICKS] = (double)out_ticks;
          for (int i = 0; i < 8; ++i) rec[SHIPSIM_DL_OBS + i] = (double)ns[i];
          if (POLICY && !OPM_GET(started_here)) {  // started in an earlier launch: from the state
            const DevState So = opaque(step_args().S);
            rec[SHIPSIM_DL_ACTION] = (double)So.dec_action()[envc];
            for (int i = 0; i < 8; ++i) rec[SHIPSIM_DL_OBS0 + i] = (double)So.dec_obs0()[envc * 8 + i];
          }
        }
        log_n += 1;
        n_decided += 1;
        OPM_SET(started_here, false);
        if (out_done || dec_i + 1 >= CH.n_dec) {
          reset_env();
          ep_i += 1;
          dec_i = 0;
        } else {
          dec_i += 1;
        }
        if (opaque_if<OPQ>(lie) == 0) {
          const DevState So = opaque(step_args().S);
          for (int i = 0; i < 8; ++i) So.next_obs8()[envc * 8 + i] = ns[i];  // self.next_observations
        }
        ready = opaque_if<OPQ>(0);
        out_done = false;
        if (burst + 1 >= kChainBurst || (CH.log_stop && log_n >= CH.log_cap)) {
          OPM_SET(stalled, true);  // next decision pending: resumed by the next launch
          running = opaque_if<OPQ>(0);
        } else {
          OPM_SET(want, true);
        }
      }
      float a_log;
      const float sa = chain_action(want, a_log);
      if (OPM_GET(want)) decision_prologue(sa, a_log);
    }
  };

  {
    const flag_t want = OPM ? (flag_t)opaque_v((running && (dflags & DF_AWAITING)) ? 1 : 0)
                            : (flag_t)(running && (dflags & DF_AWAITING));
    if (CHAIN) {
      float a_log;
      const float sa = chain_action(want, a_log);
      if (OPM_GET(want)) decision_prologue(sa, a_log);
    } else if (want) {
      decision_prologue(A0.action[envc], A0.action[envc]);
    }
  }

  // The grid cell of the ship's position at its last map query, this sub-lane's share of the cell's candidate
  // edges and the cell's class: a ship moves a few metres per tick through 200 m cells, so the two dependent
  // global loads of a query are only issued when the cell changes (-2: none yet)
  int g_cell = -2, g_flag = GRID_MIXED;
  uint64_t g_mask = 0;
  TickMath<TMB> tmath;
  tmath.row_lane0 = env_lane0;
  if constexpr (TMB & 4) tmath.row.load(lie);  // the table's entries on the env row's lanes, for the launch
  // (an int: OPQ kernels hold it in a VGPR, not as a lane mask live across the whole tick loop)
  int going = opaque_if<OPQ>((running && !ready && (budget <= 0 || ticks < budget)) ? 1 : 0);
  PT_DECL;
  // CHAIN: the tick loop hands over to the (rare) chaining code below whenever a decision of the
  // wave completes, so the loop body itself is the per-decision kernel's.
  // The streams' loop is tested at its bottom (a guard, then the test after the body; one spelling of the condition
  // for both): with the test in the header the exits to the chaining code leave from there, and the register
  // allocator carried the whole loop-carried state (Ship, sy / cy, the travel tracker, the small ints) to the outer
  // code's registers in the header and back in front of the going region, about 150 moves per wave-tick (DESIGN.md
  // §9 "The tick loop, bottom-tested"). The body has no continue and no goto, and its breaks are a switch's, so the
  // two forms run the same statements. shipsim_step's kernels keep the test at the top and the code they had.
  constexpr bool TICK_ROT = CHAIN != 0;
#define TICK_LOOP_ON (__any(opaque_if<OPQ>(going)) && !(CHAIN && __any(opaque_if<OPQ>(ready) && opaque_if<OPQ>(running))))
  for (;;) {
  if (!TICK_ROT || TICK_LOOP_ON) for (;;) {
    if (!TICK_ROT && !TICK_LOOP_ON) break;
    // this tick's constants: re-read (scalar loads, LDS) rather than kept in registers across ticks
    const StepArgs& A = step_args();
    const Params& P = A.P;
    const ConstBuf& K = A.K;
    const Traj& T = A.T;
    const auto& PT = regs_or<RC_PAR>(rc_par, P);  // Params' numbers: the register copies where held
    const auto& KT = regs_or<RC_PAR>(rc_par, K);  // the map grid's
    // the lane's roles re-derived per tick where OPQ (shadowing the entry's): the run-time ship count and the
    // slot tests of the K > 1 kernels otherwise stay lane masks and scalars held across the loop, and spill
    const int lie_t = opaque_if<OPQ>(lie);
    const int ship = lie_t % SLOTS;
    const int sub = lie_t / SLOTS;
    const bool is_test = ship == 0;
    const int nsh = (SLOTS == 2) ? 2 : P.n_ships;
    const bool ghost = (SLOTS > 2) && ship >= nsh;
    const int shipc = ghost ? nsh - 1 : ship;
    const bool is_obs1 = shipc == 1;
    (void)ghost;
    // partner ship's pre-tick state (the test ship's SBMPC reads the obstacle ship before it moves)
    SHIPSIM_LANE_CHECK(LPE, 7);
    const double pn = pair_swap(s.n), pe = pair_swap(s.e);
    double sf = 1.0, off = 0.0;
    constexpr bool LOS_PRE = COLLAV == SHIPSIM_COLLAV_SBMPC && SLOTS == 2;  // the LOS term evaluated once per tick
    double los_pre_q = 0.0, los_pre_e = 0.0;
    bool sb_active = false;
    double sb_pb = 1.0, sb_cb = 0.0;  // (FLAT) the pass's result, handed out inside the going region
    if (COLLAV == SHIPSIM_COLLAV_SBMPC && SLOTS > 2) {  // do_list of every obstacle ship (env.py:366-370)
      constexpr int NOB = launch_host::sbmpc_nob(SLOTS);  // (slots past K duplicate a ship)
      SbMulti<NOB> in;
      double obn[NOB], obe[NOB];
#pragma unroll
      for (int k = 0; k < NOB; ++k) {
        double x = 0, y = 0, psi = 0, u = 0, v = 0;
        switch (k + 1) {  // slot k + 1's first lane of the env row (row broadcast)
#define SB_GATHER(M)                              \
  case M:                                         \
    if constexpr (M < SLOTS) {                    \
      x = env_lane_d<LPE, M>(s.e, env_lane0);     \
      y = env_lane_d<LPE, M>(s.n, env_lane0);     \
      psi = env_lane_d<LPE, M>(s.yaw, env_lane0); \
      u = env_lane_d<LPE, M>(s.u, env_lane0);     \
      v = env_lane_d<LPE, M>(s.v, env_lane0);     \
    }                                             \
    break;
          SB_GATHER(1) SB_GATHER(2) SB_GATHER(3) SB_GATHER(4) SB_GATHER(5) SB_GATHER(6) SB_GATHER(7)
#undef SB_GATHER
          default: break;
        }
        const ShipConst& ck = SC[(k + 1 < nsh) ? k + 1 : nsh - 1];
        in.ob_x[k] = x; in.ob_y[k] = y; in.ob_psi[k] = -psi; in.ob_u[k] = u; in.ob_v[k] = v;
        in.obs_l[k] = ck.obs_l_cfg; in.obs_w[k] = ck.obs_w_cfg;
        obn[k] = y; obe[k] = x;
      }
      bool need = false;
      in.u_d = 0; in.chi_d = 0; in.os_x = 0; in.os_y = 0; in.os_v = 0; in.p_last = 0; in.chi_last = 0;
      if (going && is_test) {
        const double los_arg = los_update(c, s, s.n, s.e);
#pragma unroll
        for (int k = 0; k < NOB; ++k) {  // sbmpc.py:150-156: active when any obstacle is within D_INIT
          const double d0 = obe[k] - s.e, d1 = obn[k] - s.n;
          need = need || sqrt_lt(d0 * d0 + d1 * d1, 2000.0);
        }
        if (need) in.chi_d = -(s.seg_alpha + atan(los_arg));
        in.u_d = c.desired_speed;
        in.os_x = s.e; in.os_y = s.n; in.os_v = s.v;
        in.p_last = p_last; in.chi_last = chi_last;
      }
      double pb = 1.0, cb = 0.0;
      need = diag::sb_request(need, P.max_sampling);  // (the product: need itself)
      diag::sb_stat_lanes(6, (need && sub == 0) ? 1u : 0u);
      diag::sb_stat_lanes(7, (going && is_test && sub == 0) ? 1u : 0u);
      sbmpc_cooperative_multi<NOB>(need && sub == 0, in, nsh - 1, P.sbmpc_nsamp, P.sbmpc_dt, pb, cb);
      pb = env_lane_d<LPE, 0>(pb, env_lane0);
      cb = env_lane_d<LPE, 0>(cb, env_lane0);
      const int need0 = env_lane_i<LPE, 0>((int)need, env_lane0);
      sb_active = need0;
      if (opaque_if<OPQ>(going)) {  // (tested here, not held as a lane mask across the optimiser's loop)
        if (need0) { p_last = pb; chi_last = cb; }
        else { p_last = 1; chi_last = 0; }
        if (opaque_if<OPQ>(is_test ? 1 : 0) && need0) { sf = pb; off = cb; }
      }
    } else if (COLLAV == SHIPSIM_COLLAV_SBMPC) {
      bool need = false;
      double los_arg = 0.0;
      if constexpr (FLAT) {  // the flat tick: the two guards below as one
        if (going) {
          los_pre_q = los_q(c, s, s.n, s.e, los_pre_e);
          if constexpr (LM_REQ) {
            // the block below on every lane, without the role guard: its updates are pure, and the obstacle ship's
            // lanes keep their state by selects (their los_arg and need are not read)
            const double ect0 = s.e_ct, eint0 = s.e_ct_int;
            s.e_ct = los_pre_e;
            los_arg = los_windup(c, s, los_pre_q);
            s.e_ct = is_test ? s.e_ct : ect0;
            s.e_ct_int = is_test ? s.e_ct_int : eint0;
            double d0 = pe - s.e, d1 = pn - s.n;
            need = (int)is_test & (int)sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_
            need = diag::sb_request(need, PT.max_sampling);
          } else
          if (is_test) {
            s.e_ct = los_pre_e;
            los_arg = los_windup(c, s, los_pre_q);
            double d0 = pe - s.e, d1 = pn - s.n;
            need = sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_
            need = diag::sb_request(need, PT.max_sampling);
          }
        }
      } else {
      if (going) {
        // the LOS cross-track term at this position, for every ship: its control below reuses it (its position
        // and segment are the same there unless the waypoint index advances)
        los_pre_q = los_q(c, s, s.n, s.e, los_pre_e);
      }
      if (going && is_test) {
        // env.py:362-363: next_wpt result discarded; los_guidance integrates e_ct_int (Q3). The
        // course (atan) only feeds the optimisation, so it is evaluated for requesting envs only.
        s.e_ct = los_pre_e;
        los_arg = los_windup(c, s, los_pre_q);
        double d0 = pe - s.e, d1 = pn - s.n;
        need = sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_
        need = diag::sb_request(need, PT.max_sampling);  // (the product: need itself)
      }
      }
      double pb = 1.0, cb = 0.0;
      int need0 = 0;
      diag::sb_stat_lanes(6, (need && sub == 0) ? 1u : 0u);  // (statistics builds: as the multi-obstacle branch)
      diag::sb_stat_lanes(7, (going && is_test && sub == 0) ? 1u : 0u);
      // the optimiser's inputs, pass and hand-out only in a wave where some env requests it this tick (a
      // wave-uniform branch: every lane takes part in the exchanges inside)
      if (__any(need)) {
        const double pyaw = pair_swap(s.yaw), pu = pair_swap(s.u), pv = pair_swap(s.v);
        const double psy = pair_swap(sy), pcy = pair_swap(cy);  // sin/cos(pyaw), carried by the partner
        SbIn in = SbIn{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        in.u_d = SC[0].desired_speed;  // the same in every lane (sbmpc_cooperative<true>)
        in.obs_l = SC[1].obs_l_cfg; in.obs_w = SC[1].obs_w_cfg;
        if (going && is_test) {
          if constexpr (!SB_NOM_ALG) {
            if (need) in.chi_d = -(s.seg_alpha + atan(los_arg));
          }
          in.os_x = s.e; in.os_y = s.n; in.os_v = s.v;
          in.ob_x = pe; in.ob_y = pn; in.ob_psi = -pyaw; in.ob_u = pu; in.ob_v = pv;
          in.ob_so = -psy; in.ob_co = pcy;  // sin(-yaw) = -sin(yaw), cos(-yaw) = cos(yaw)
          in.p_last = p_last; in.chi_last = chi_last;
        }
        if constexpr (SB_NOM) {
          // every request of the wave tested at once, on all lanes (a ship's sub-lanes redundantly, like the rest of
          // the chain; the obstacle ship's lanes on zeros, their result masked by need)
          bool fast;
          if constexpr (SB_NOM_ALG) {
            fast = need & sbmpc_nominal_holds_seg(in, s.seg_sin, s.seg_cos, los_arg, PT.sbmpc_nsamp, PT.sbmpc_dt).holds;
            if (need & !fast) in.chi_d = -(s.seg_alpha + atan(los_arg));
          } else {
            fast = need & sbmpc_nominal_holds(in, PT.sbmpc_nsamp, PT.sbmpc_dt).holds;
          }
          diag::sb_stat_lanes(8, (fast && sub == 0) ? 1u : 0u);
          const bool pass = need & !fast;
          diag::sb_stat_wave(9, __any(pass) ? 0u : 1u);
          if (__any(pass)) sbmpc_cooperative<true>(pass && sub == 0, in, PT.sbmpc_nsamp, PT.sbmpc_dt, pb, cb);
          // an accepted request's answer: the nominal scenario's (P_ca, Chi_ca), as the pass forms them
          pb = fast ? p_ca_of(kSbNominalP) : pb;
          cb = fast ? (-30.0 + 10.0 * kSbNominalChi) * (kPi / 180.0) : cb;
        } else
        sbmpc_cooperative<true>(need && sub == 0, in, PT.sbmpc_nsamp, PT.sbmpc_dt, pb, cb);
        pb = env_lane_d<LPE, 0>(pb, env_lane0);
        cb = env_lane_d<LPE, 0>(cb, env_lane0);
        need0 = env_lane_i<LPE, 0>((int)need, env_lane0);
      }
      sb_active = need0;
      if constexpr (FLAT) {
        sb_pb = pb; sb_cb = cb;
      } else {
      if (opaque_if<OPQ>(going)) {  // (tested here, not held as a lane mask across the optimiser's loop)
        if (need0) { p_last = pb; chi_last = cb; }
        else { p_last = 1; chi_last = 0; }
        if (opaque_if<OPQ>(is_test ? 1 : 0) && need0) { sf = pb; off = cb; }
      }
      }
    }

    PT_MARK(0);
    // The flat tick: one `going` region from here to the end of the tick body (FLAT, above), its body's own guards
    // constant-true. (Not re-indented: the body is every instantiation's.)
    if (!FLAT || opaque_if<OPQ>(going)) {
    if constexpr (FLAT) SHIPSIM_LANE_CHECK(LPE, 9);  // (diagnostics build: an env's whole row enters together)
    if constexpr (FLAT && COLLAV == SHIPSIM_COLLAV_SBMPC) {  // the pass's hand-out
      if (sb_active) { p_last = sb_pb; chi_last = sb_cb; }
      else { p_last = 1; chi_last = 0; }
      if (opaque_if<OPQ>(is_test ? 1 : 0) && sb_active) { sf = sb_pb; off = sb_cb; }
    }
    // ---- ship ticks (test_step :345-445 / obs_step :447-536) ----
    double my_speed_out = 0.0, dtravel = 0.0, dtime = 0.0;
    double dtravel2 = 0.0;  // (LM_POST) the obstacle ship's squared travel step; 0 where it has none (frozen)
    double ep_n = 0.0, ep_e = 0.0, ep_dt = 0.0;  // (EARLY_MAP) the position after this tick's step, and the step
    if (FLAT || going) {
      if constexpr (EARLY_MAP) {
        // The map query's cell and, where it changes, the cell's edge share and class, requested here: the query
        // needs only the position after the tick's Euler step, which the state at the tick's start fixes (a frozen
        // obstacle ship keeps its position), so its two global loads run under the control chain instead of in
        // front of the edge loop. g_cell is the query's cell from here on.
        ep_dt = PT.dt;
        early_pose(s, sy, cy, ep_dt, ep_n, ep_e);
        const bool frozen = !is_test && s.stop;
        const int cc = grid_cell(KT, frozen ? s.n : ep_n, frozen ? s.e : ep_e);
        if (cc != g_cell) {
          g_cell = cc;
          g_mask = 0;
          g_flag = GRID_MIXED;
          if (cc >= 0) {  // (one block: the two arrays' addresses in one fetch, the two loads back to back)
            g_mask = grid_share(K, cc, sub, NSUB);
            g_flag = (int)K.grid_flag[cc];
          }
        }
      }
      if (!is_test && s.stop) {
        // frozen obstacle ship: store_last_simulation_data + two next_time (Q9)
        if (REC && sub == 0) record_last(T, qc, rec_t, s.time, s.time + PT.dt);
        s.time = s.time + PT.dt;
        s.time = s.time + PT.dt;
      } else {
        const double prev_log_n = s.log_n, prev_log_e = s.log_e;
        const double U = s.u;
        bool imminent = false;
        if (SIMPLE && is_test) {  // check_condition.py:130 on float32 self.states
          float dn = st4[0] - st4[2], de = st4[1] - st4[3];
          imminent = (dn * dn + de * de) < 9000000.0f;
        }
        SHIPSIM_SHIP_CHECK(LPE, SLOTS, 6);  // (its DPP exchanges pair sub-lanes of one ship)
        if constexpr (RC_PAR) {
          // each register copy read once for the ship tick (a read is two moves per double): the step and the
          // weather as plain values under Params' names
          const LaneWeather wxr = {PT.vc_n, PT.vc_e, PT.wind_speed, PT.wind_sin, PT.wind_cos};
          static_assert(EARLY_MAP == RC_PAR, "the step and the new position were formed at the top of the ship tick");
          const TickStep pd = {ep_dt};
          if constexpr (TMB & 4)  // (diagnostics build: the table's source lanes, the row's even ones, are active)
            SHIPSIM_INDEX_CHECK(((__builtin_amdgcn_read_exec() >> env_lane0) & 0x5555u) == 0x5555u, 14);
          control_and_integrate_sc<DETAILED, REC, LOS_PRE>(c, pd, wxr, s, rn, re, -off, sf, mach_dt, ep_n, ep_e, sy, cy,
                                                           los_pre_q, los_pre_e, tmath);
        } else {
          control_and_integrate_sc<DETAILED, REC, LOS_PRE>(c, P, weather_of(P, lw), s, rn, re, -off, sf, mach_dt,
                                                           (SIMPLE && is_test) ? 1 : 0, imminent,
                                                           (REC && sub == 0) ? T.ship_row(qc, rec_t) : nullptr, fuel, sy,
                                                           cy, los_pre_q, los_pre_e);
        }
        my_speed_out = U;
        if (is_obs1) {  // travel tracker (env.py:527-534, Q6)
          double tn = s.log_n - prev_log_n, te = s.log_e - prev_log_e;
          if constexpr (LM_POST) dtravel2 = tn * tn + te * te;  // (its root: with the ground distance's, below)
          else dtravel = sqrt(tn * tn + te * te);
          dtime = PT.dt;
        }
      }
    }
    PT_MARK(1);
    // ---- own-ship map queries, split over the ship's sub-lanes ----
    double d2 = INFINITY;
    bool gr = false;
    if (FLAT || going) {
      int cc;
      if constexpr (EARLY_MAP) {
        cc = g_cell;  // this position's cell, its share and class already requested (the top of the ship tick)
      } else {
        cc = grid_cell(KT, s.n, s.e);
        if (cc != g_cell) {  // (rare) a new cell: its edge share and class
          g_cell = cc;
          g_mask = cc >= 0 ? grid_share(K, cc, sub, NSUB) : 0;
          g_flag = cc >= 0 ? (int)K.grid_flag[cc] : GRID_MIXED;
        }
      }
      if constexpr (!diag::kNoMapDist) {
        if constexpr (EARLY_MAP)
          d2 = cc >= 0 ? map_dist2_mask_pf(lds_edges, g_mask, s.n, s.e) : map_dist2_part(lds_edges, K.n_edges, s.n, s.e, sub, NSUB);
        else
          d2 = cc >= 0 ? map_dist2_mask(lds_edges, g_mask, s.n, s.e) : map_dist2_part(lds_edges, K.n_edges, s.n, s.e, sub, NSUB);
      }
      const double margin = c.l_ship / 2;  // check_condition.py:50-78 hull hard points
      // Every hull corner is within margin·√2 of the centre. With no coastline edge that close (the
      // ship's min over its cell's candidate edges, which hold every edge within kGroundReach) and the
      // centre's cell entirely outside / inside the land, the segment centre → corner crosses no edge:
      // each corner has the centre cell's status, exactly what the four point-in-polygon tests return.
      double d2s = d2;
      int dummy = 0;
      ship_reduce<LPE, SLOTS>(d2s, dummy);
      const double lim = margin * 1.4142135623730951 + 1e-3;
      const int fcen = g_flag;
      const bool far_shore = d2s > lim * lim && fcen != GRID_MIXED && lim < kGroundReach;
      if constexpr (diag::kNoGround) {
      } else if (far_shore) {
        gr = fcen == GRID_IN;
      } else if constexpr (NSUB == 8) {
        // 8 sub-lanes for 4 corners: sub-lanes k and k + 4 split corner k's ring edges (every other
        // edge) and combine the crossing parity (XOR) and the boundary flag (OR) per polygon — the
        // same boolean as corner_inside (the partner lane is 4·SLOTS lanes away, same env and ship)
        const int sv = opaque_if<OPQ>(sub);  // (recomputed in the loop: no lane masks kept across it)
        const int k = sv & 3, half = sv >> 2;
        const double cn = (k < 2) ? s.n - margin : s.n + margin;
        const double ce = (k & 1) ? s.e + margin : s.e - margin;
        const int c = grid_cell(KT, cn, ce);
        const int f = c >= 0 ? (int)K.grid_flag[c] : GRID_MIXED;
        uint32_t par = 0, bnd = 0;
        if (f == GRID_MIXED) map_inside_half(lds_edges_raw, lds_boxes, P.n_polys, cn, ce, half, par, bnd);
        const uint32_t par_o = (uint32_t)__shfl_xor((int)par, 4 * SLOTS, 64);
        const uint32_t bnd_o = (uint32_t)__shfl_xor((int)bnd, 4 * SLOTS, 64);
        if (f == GRID_MIXED ? (((par ^ par_o) & ~(bnd | bnd_o)) != 0) : (f == GRID_IN)) gr = true;
      } else {
        for (int k = opaque_if<OPQ>(sub); k < 4; k += NSUB) {  // (opaque: no lane masks kept across the loop)
          const double cn = (k < 2) ? s.n - margin : s.n + margin;
          const double ce = (k & 1) ? s.e + margin : s.e - margin;
          if (corner_inside(K, lds_edges_raw, lds_boxes, P.n_polys, cn, ce)) gr = true;
        }
      }
      d2 = d2s;  // the ship's min over its sub-lanes' edge shares (reduced once, above)
    }
    int gri = gr ? XF_GROUND : 0;
    ship_or<LPE, SLOTS>(gri);
    double my_ground, lm_on = 0.0, lm_oe = 0.0, lm_dist = 0.0, lm_odtravel = 0.0;
    if constexpr (LM_POST) {
      // the three roots after the step in one call: each ship's ground distance on its even sub-lanes; on the odd
      // ones the reward's distance (the test ship's lanes: the same bits from either ship, (-x)² = x²) and the
      // obstacle ship's travel step (its own lanes; 0 when frozen, whose root is the 0 the guarded tick adds)
      SHIPSIM_LANE_CHECK(LPE, 13);
      lm_on = pair_swap(s.n); lm_oe = pair_swap(s.e);
      const double dx = lm_on - s.n, dy = lm_oe - s.e;
      sqrt3_row(d2, dx * dx + dy * dy, dtravel2, sub & 1, is_test, my_ground, lm_dist, lm_odtravel);
    } else {
      my_ground = sqrt(d2);
    }
    PT_MARK(2);
    bool my_end = false, my_outside = false, my_roa = false, my_nf = false;
    if (FLAT || going) {
      my_end = sqrt_le((s.n - s.end_n) * (s.n - s.end_n) + (s.e - s.end_e) * (s.e - s.end_e), 200.0);
      double margin = c.l_ship / 2;
      if constexpr (LM_OUT)  // (the four comparisons are pure: no short-circuit branches)
        my_outside = ((int)(s.n < PT.min_north + margin) | (int)(s.n > PT.max_north - margin) |
                      (int)(s.e < PT.min_east + margin) | (int)(s.e > PT.max_east - margin)) != 0;
      else
      my_outside = (s.n < PT.min_north + margin || s.n > PT.max_north - margin) ||
                   (s.e < PT.min_east + margin || s.e > PT.max_east - margin);
      double rdn = s.n - s.wp_n, rde = s.e - s.wp_e;  // is_reach_radius_of_acceptance (obstacle ship)
      my_roa = (rdn * rdn + rde * rde) < PT.roa2;
      // a NaN / Inf anywhere in the dynamic state poisons this sum (boundary error contract)
      my_nf = !isfinite(((s.n + s.e) + (s.yaw + s.u)) + ((s.v + s.r) + (s.omega + s.e_ct_int)));
    }
    const int my_flags = gri | (my_end ? XF_END : 0) | (my_outside ? XF_OUTSIDE : 0) | (my_roa ? XF_ROA : 0) |
                         (my_nf ? XF_NONFINITE : 0);
    // env-level view of the tick: the ship under test (T), the obstacle ship (O) and the nearest
    // obstacle ship (C; = O with one obstacle ship)
    double Tn, Te, Th, Tsh, Tch, Tect, Tground, Ttime, On, Oe, Oyaw, Oect, Oground, Ospeed, Odtravel, Odtime, Cn, Ce;
    int Tf, Of;
    bool any_nf;
    if constexpr (SLOTS == 2) {
      // each lane's own perspective: T = its own ship, O = the partner lane's (lane ^ 1). That is the env's view
      // on the test ship's lanes; the env's outcome is the test ship's first lane's (its event bits, taken by every
      // lane of the env below), so the obstacle ship's lanes need no role selects
      SHIPSIM_LANE_CHECK(LPE, 8);
      Tn = s.n; Te = s.e; Th = s.yaw; Tsh = sy; Tch = cy; Tect = s.log_ect; Tground = my_ground; Ttime = s.time;
      Tf = my_flags;
      Of = pair_swap_i(my_flags);
      if constexpr (LM_POST) { On = lm_on; Oe = lm_oe; }  // (exchanged in front of the batched roots)
      else { On = pair_swap(s.n); Oe = pair_swap(s.e); }
      Oyaw = pair_swap(s.yaw);
      Oect = pair_swap(s.log_ect); Oground = pair_swap(my_ground);
      Ospeed = pair_swap(my_speed_out);
      if constexpr (LM_POST) Odtravel = lm_odtravel;  // (sqrt3_row: the partner's root, crossed already)
      else Odtravel = pair_swap(dtravel);
      Odtime = pair_swap(dtime);
      Cn = On; Ce = Oe;
      any_nf = (my_flags | Of) & XF_NONFINITE;
    } else {  // slot k's first lane of the env row holds ship k
      Tn = env_lane_d<LPE, 0>(s.n, env_lane0); Te = env_lane_d<LPE, 0>(s.e, env_lane0);
      Th = env_lane_d<LPE, 0>(s.yaw, env_lane0); Tsh = env_lane_d<LPE, 0>(sy, env_lane0);
      Tch = env_lane_d<LPE, 0>(cy, env_lane0); Tect = env_lane_d<LPE, 0>(s.log_ect, env_lane0);
      Tground = env_lane_d<LPE, 0>(my_ground, env_lane0); Ttime = env_lane_d<LPE, 0>(s.time, env_lane0);
      Tf = env_lane_i<LPE, 0>(my_flags, env_lane0);
      On = env_lane_d<LPE, 1>(s.n, env_lane0); Oe = env_lane_d<LPE, 1>(s.e, env_lane0);
      Oyaw = env_lane_d<LPE, 1>(s.yaw, env_lane0); Oect = env_lane_d<LPE, 1>(s.log_ect, env_lane0);
      Oground = env_lane_d<LPE, 1>(my_ground, env_lane0); Ospeed = env_lane_d<LPE, 1>(my_speed_out, env_lane0);
      Odtravel = env_lane_d<LPE, 1>(dtravel, env_lane0); Odtime = env_lane_d<LPE, 1>(dtime, env_lane0);
      Of = env_lane_i<LPE, 1>(my_flags, env_lane0);
      int nf = Tf | Of;
      Cn = On; Ce = Oe;
      double cd = (Tn - On) * (Tn - On) + (Te - Oe) * (Te - Oe);
#define NEAREST(M)                                                                                  \
  if constexpr (M < SLOTS) {                                                                        \
    const double kn = env_lane_d<LPE, M>(s.n, env_lane0), ke = env_lane_d<LPE, M>(s.e, env_lane0); \
    nf |= env_lane_i<LPE, M>(my_flags, env_lane0);                                                  \
    const double kd = (Tn - kn) * (Tn - kn) + (Te - ke) * (Te - ke);                                \
    if (kd < cd) { cd = kd; Cn = kn; Ce = ke; }                                                     \
  }
      NEAREST(2) NEAREST(3) NEAREST(4) NEAREST(5) NEAREST(6) NEAREST(7)
#undef NEAREST
      any_nf = nf & XF_NONFINITE;
    }
    if (FLAT || going) {
      travel_dist += Odtravel;
      travel_time += Odtime;
      // next_states (env.py:582-591) and self.states
      ns[0] = (float)Tn; ns[1] = (float)Te; ns[2] = (float)Tect;
      ns[3] = (float)On; ns[4] = (float)Oe; ns[5] = (float)Oyaw; ns[6] = (float)Ospeed; ns[7] = (float)Oect;
      if (SIMPLE) { st4[0] = ns[0]; st4[1] = ns[1]; st4[2] = ns[3]; st4[3] = ns[4]; }
      // get_reward_and_env_info (reward_function.py:59-270)
      const bool is_collision = ((Tn - Cn) * (Tn - Cn) + (Te - Ce) * (Te - Ce)) < 2500.0;
      const bool is_tg = Tf & XF_GROUND, is_og = Of & XF_GROUND;
      const bool is_tnav = fabs(Tect) > 3000;
      const bool is_onav = (travel_dist > PT.AB_seg * 2) || (travel_time > INFINITY) || (fabs(Oect) > 500);
      double dx = Cn - Tn, dy = Ce - Te;
      double dist;
      if constexpr (LM_POST) dist = lm_dist;
      else dist = sqrt(dx * dx + dy * dy);
      const bool enc_ok = !overtaking_sector(dx, dy, dist, Tsh, Tch, Th);  // head-on or crossing (Q5)
      // the five shaped terms of reward_designs.py:33-55 (RewardDesign4 / 3): one exp each,
      // evaluated by five lanes of the env in one call when LPE >= 8, then gathered
      const double xv[5] = {dist, Tground, fabs(Tect), Oground, fabs(Oect)};
      const double tg[5] = {0.0, 0.0, 3000.0, 0.0, 500.0};
      const double of[5] = {200000000.0, 175000.0, 1250000.0, 50000.0, 12500.0};
      double ex[5];
      if (LPE >= 8) {
        const int j = opaque_v(lie) & 7;  // (recomputed in the loop: no lane masks kept across it)
        double xj;
        if constexpr (SLOTS == 2)  // lanes 1 / 3 (obstacle ship): its own ground / |e_ct| (terms 3 / 4)
          xj = (j == 0) ? dist : (j < 3) ? Tground : fabs(Tect);
        else
          xj = (j == 0) ? xv[0] : (j == 1) ? xv[1] : (j == 2) ? xv[2] : (j == 3) ? xv[3] : xv[4];
        const RewardTerm to = lds_rterm[j];
        if constexpr (TMB & 4) SHIPSIM_LANE_CHECK(LPE, 15);  // (the exp entries' source lanes: the whole row)
        const double ej = tmath.exp_reward(div_by(-((xj - to.t) * (xj - to.t)), to.o, to.y));
        ex[0] = env_lane_d<LPE, reward_lane<SLOTS>(0)>(ej, env_lane0);
        ex[1] = env_lane_d<LPE, reward_lane<SLOTS>(1)>(ej, env_lane0);
        ex[2] = env_lane_d<LPE, reward_lane<SLOTS>(2)>(ej, env_lane0);
        ex[3] = env_lane_d<LPE, reward_lane<SLOTS>(3)>(ej, env_lane0);
        ex[4] = env_lane_d<LPE, reward_lane<SLOTS>(4)>(ej, env_lane0);
      } else {
#pragma unroll
        for (int k = 0; k < 5; ++k) ex[k] = exp(-((xv[k] - tg[k]) * (xv[k] - tg[k])) / of[k]);
      }
      // rd4(t, off, v) = v < t ? 1 : exp(.), rd3(t, off, v) = v < t ? exp(.) : 1
      double r0 = (dist < 10000 && enc_ok) ? ((xv[0] < 0.0) ? 1.0 : ex[0]) : 0.0;
      double r1 = (Tground <= 1000) ? ((xv[1] < 0.0) ? 1.0 : ex[1]) : 0.0;
      double r2 = (xv[2] < 3000.0) ? ex[2] : 1.0;
      double r3 = (Oground <= 1000) ? -((xv[3] < 0.0) ? 1.0 : ex[3]) : 0.0;
      double r4 = -((xv[4] < 500.0) ? ex[4] : 1.0);
      double r = (r0 + ((((0.0 + r1) + r2) + r3) + r4)) / 5;  // np.sum(5 terms) / 5
      if (is_collision || is_tg || is_tnav || is_og || is_onav) {  // :272-314
        const double reward = r + acc;
        double o = 0;
        const bool cond[5] = {is_collision, is_tg, is_tnav, is_og, is_onav};
        const double mult[5] = {10.0, 5.0, 5.0, -2.5, -2.5};
        for (int i = 0; i < 5; ++i) {
          if (acc > 0 && cond[i]) o += reward * mult[i];
          else if (acc < 0 && cond[i]) o += reward * -mult[i];
        }
        r = o;
      }
      const bool t6 = Tf & XF_END, t7 = Tf & XF_OUTSIDE, t8 = Of & XF_END, t9 = Of & XF_OUTSIDE;
      const bool t10 = Ttime > PT.sim_time;
      constexpr uint32_t kRoaBit = 1u << 31;  // (private: the obstacle ship reached its waypoint radius)
      uint32_t bits = (is_collision ? SHIPSIM_EV_COLLISION : 0) | (is_tg ? SHIPSIM_EV_TEST_GROUNDING : 0) |
                      (is_tnav ? SHIPSIM_EV_TEST_NAV_FAILURE : 0) | (is_og ? SHIPSIM_EV_OBS_GROUNDING : 0) |
                      (is_onav ? SHIPSIM_EV_OBS_NAV_FAILURE : 0) | (t6 ? SHIPSIM_EV_TEST_REACHES_END : 0) |
                      (t7 ? SHIPSIM_EV_TEST_OUTSIDE_MAP : 0) | (t8 ? SHIPSIM_EV_OBS_REACHES_END : 0) |
                      (t9 ? SHIPSIM_EV_OBS_OUTSIDE_MAP : 0) | (t10 ? SHIPSIM_EV_TIME_LIMIT : 0) |
                      ((Of & XF_ROA) ? kRoaBit : 0u);
      if constexpr (SLOTS == 2) bits = (uint32_t)env_lane_i<LPE, 0>((int)bits, env_lane0);  // the test ship's view
      const bool roa_o = bits & kRoaBit;
      bits &= ~kRoaBit;
      const bool terminal = bits & 0x1F;
      const bool test_stop = bits & (SHIPSIM_EV_COLLISION | SHIPSIM_EV_TEST_GROUNDING | SHIPSIM_EV_TEST_NAV_FAILURE |
                                     SHIPSIM_EV_TEST_REACHES_END | SHIPSIM_EV_TEST_OUTSIDE_MAP | SHIPSIM_EV_TIME_LIMIT);
      const bool obs_stop = bits & (SHIPSIM_EV_COLLISION | SHIPSIM_EV_OBS_GROUNDING | SHIPSIM_EV_OBS_NAV_FAILURE |
                                    SHIPSIM_EV_OBS_REACHES_END | SHIPSIM_EV_OBS_OUTSIDE_MAP | SHIPSIM_EV_TIME_LIMIT);
      if (terminal) bits |= SHIPSIM_EV_TERMINAL;
      if (test_stop) bits |= SHIPSIM_EV_TEST_STOP;
      if (obs_stop) bits |= SHIPSIM_EV_OBS_STOP;
      if (obs_stop && !terminal && is_obs1) s.stop = 1;
      if (SLOTS > 2 && shipc >= 2 && (my_flags & (XF_END | XF_OUTSIDE | XF_GROUND)))
        s.stop = 1;  // further obstacle ships freeze at their last waypoint / off the map / aground
      bool combined_done = terminal || (test_stop && !terminal);
      const bool nonfinite = any_nf;
      if (nonfinite) {  // not a reference outcome: the env ends its episode here, flagged
        bits |= SHIPSIM_EV_NONFINITE | SHIPSIM_EV_TERMINAL;
        combined_done = true;
        n_nonfinite += 1;
      }
      if (REC) {  // RewardTracker.update (reward_function.py:181-186) + env.py:613-620 animation lists
        double* er = (lie == 0) ? T.env_row(env, rec_t - 1) : nullptr;
        if (er) {
          er[SHIPSIM_TE_R_COLLISION] = r0 / 5; er[SHIPSIM_TE_R_TEST_GROUNDING] = r1 / 5;
          er[SHIPSIM_TE_R_TEST_NAV] = r2 / 5; er[SHIPSIM_TE_R_OBS_GROUNDING] = r3 / 5;
          er[SHIPSIM_TE_R_OBS_NAV] = r4 / 5; er[SHIPSIM_TE_R_TOTAL] = r; er[SHIPSIM_TE_BITS] = (double)bits;
          const bool imm = (COLLAV == SHIPSIM_COLLAV_SBMPC)
                               ? sb_active
                               : ((Tn - On) * (Tn - On) + (Te - Oe) * (Te - Oe)) < 9000000.0;
          er[SHIPSIM_TE_FLAGS] = (double)((is_collision ? SHIPSIM_TE_FLAG_COLLISION : 0) |
                                          (imm ? SHIPSIM_TE_FLAG_IMMINENT : 0));
        }
        rec_t += 1;
      }
      // ---- env.py:700-771 decision logic ----
      acc += r;
      ticks += 1;
      dec_ticks += 1;
      bool finish = nonfinite;
      if constexpr (FLAT) {
        // the ladder below as selects over the env's few ints (both sides of every rung are side-effect-free):
        // phase 0: done finishes, else the RoA moves to phase 1 with an IW and finishes without; phase 1: finishes
        // unless the last IW was sampled, which resets the travel tracker and (not done) moves to phase 2; phase 2:
        // done finishes
        const bool p0 = phase == 0, p1 = phase == 1;
        const bool iw = opaque_if<OPQ>(have_iw) != 0;
        const bool last_iw = sampling_count == PT.max_sampling;
        const bool roa = roa_o && !combined_done;
        const bool fin = p0 ? (combined_done || (roa && !iw)) : p1 ? (!last_iw || combined_done) : combined_done;
        const bool clear = p1 && last_iw;
        travel_dist = clear ? 0.0 : travel_dist;
        travel_time = clear ? 0.0 : travel_time;
        phase = (p0 && roa && iw) ? 1 : (clear && !combined_done) ? 2 : phase;
        finish = finish || fin;
      } else
      if (phase == 0) {
        const bool roa = roa_o;
        if (combined_done) finish = true;
        else if (roa) {
          if (opaque_if<OPQ>(have_iw) != 0) phase = 1;
          else finish = true;
        }
      } else if (phase == 1) {
        if (sampling_count == PT.max_sampling) {
          travel_dist = 0;
          travel_time = 0;
          if (combined_done) finish = true;
          else phase = 2;
        } else {
          finish = true;
        }
      } else {
        if (combined_done) finish = true;
      }
      if (finish) {
        out_r = acc;
        out_done = combined_done;
        out_bits = bits;
        out_ticks = dec_ticks;
        snap_bits = bits;
        ready = opaque_if<OPQ>(1);
      }
      const int mt = OPQ ? opaque_v(budget) : budget;  // (OPQ: its test not held across the loop)
      going = opaque_if<OPQ>((!OPM_GET(ready) && (mt <= 0 || ticks < mt)) ? 1 : 0);
    }
    }  // (the flat tick's going region)
    PT_MARK(3);
    if (TICK_ROT && !TICK_LOOP_ON) break;
  }
#undef TICK_LOOP_ON
  if (!CHAIN) break;
  if (POLICY || (ready && running)) chain_next();  // (policy: wave-uniform, a no-op unless a decision completed)
  {
    const int mt = OPQ ? opaque_v(budget) : budget;
    going = opaque_if<OPQ>((running && !OPM_GET(ready) && (mt <= 0 || ticks < mt)) ? 1 : 0);
  }
  if (!__any(opaque_if<OPQ>(going))) {
    // Launch tail: this wave's envs met the quota. While any wave of the launch has not, keep ticking in chunks
    // instead of idling the SIMD until the slowest wave ends (an env's results do not depend on where a launch
    // ends: slicing is exact). Bounded by tail_extra, so a wave that is not co-resident delays nothing forever.
    // (One exit, every test wave-uniform: no flow masks held across the loop.)
    const ChainArgs& CT = step_args().CH;
    if (SLOTS == 2 && CT.tail_ctr && budget < step_args().max_ticks + CT.tail_extra) {  // (two-ship envs)
      const bool lead = (opaque_v(threadIdx.x) & 63) == 0;  // (re-derived here: no lane mask held across the loop)
      if (lead && opaque_v(tail_arrived) == 0)
        __hip_atomic_fetch_add(CT.tail_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tail_arrived = opaque_v(1);
      int n_met = 0;
      if (lead) n_met = __hip_atomic_load(CT.tail_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__builtin_amdgcn_readfirstlane(n_met) < CT.tail_waves) {
        budget += kTailChunk;
        going = opaque_if<OPQ>((running && !ready && ticks < budget) ? 1 : 0);
      }
    }
    if (!__any(opaque_if<OPQ>(going))) break;  // (quota met, or every env of the wave stalled)
  }
  }
  PT_FLUSH();

  if (touched == 0) return;  // (!valid || !touched)
  const StepArgs& AE = step_args();  // not the values loaded before the loop (no live range across it)
  const ChainArgs& CH = AE.CH;
  const Traj& TE = AE.T;
  SHIPSIM_DEBUG_PRINT(env, "[dbg] env %d lie %d end: ready %d ticks %d sc %d n_base %f phase %d have_iw %d\n", env, lie,
                      (int)ready, ticks, sampling_count, n_base, phase, (int)have_iw);
  if constexpr (OPM) ready = opaque_v(ready);  // (tested from the VGPR below: no ready / !ready masks kept from the loop)
  const DevState So = opaque(AE.S);  // addresses recomputed here, not carried through the loop
  // the lane's role re-derived here (opaque), not lane masks carried through the loop
  const int lie_e = opaque_v(lie), sub_e = lie_e / SLOTS, ship_e = lie_e % SLOTS;
  const bool ghost_e = (SLOTS > 2) && ship_e >= (OPM ? AE.P.n_ships : nsh);
  if (sub_e == 0 && !ghost_e) store_ship(So, qc, s);
  if (REC) {
    if (sub_e == 0)
      for (int k = 0; k < 3; ++k) TE.fuel[(size_t)qc * 3 + k] = fuel[k];
    if (lie_e == 0) TE.len[env] = rec_t;
  }
  if (CHAIN && lie_e == 0) {
    CH.ep_idx[env] = ep_i;
    CH.dec_idx[env] = dec_i;
    if (CH.decisions) CH.decisions[env] = n_decided;
    if (CH.log_len) CH.log_len[env] = log_n;
    So.mach_dt()[env] = mach_dt;
  }
  if (lie_e == 0) {
    So.sampling_count()[env] = sampling_count;
    So.travel_dist()[env] = travel_dist; So.travel_time()[env] = travel_time; So.acc()[env] = acc;
    So.n_base()[env] = n_base; So.e_base()[env] = e_base;
    So.p_last()[env] = p_last; So.chi_last()[env] = chi_last;
    if (SIMPLE)
      for (int i = 0; i < 4; ++i) So.states4()[env * 4 + i] = st4[i];
    if (ready)
      for (int i = 0; i < 8; ++i) So.next_obs8()[env * 8 + i] = ns[i];
    So.snap_bits()[env] = snap_bits;
    So.dec_flags()[env] = ((ready || OPM_GET(stalled)) ? DF_AWAITING : 0) | (have_iw ? DF_HAVE_IW : 0) |
                          (phase << DF_PHASE_SHIFT);
    So.dec_ticks()[env] = dec_ticks;
    if (n_nonfinite) atomicAdd(So.nonfinite, n_nonfinite);
    if (ready) {
      if (AE.reward_out) AE.reward_out[env] = out_r;
      if (AE.done_out) AE.done_out[env] = out_done ? 1 : 0;
      if (AE.events_out) AE.events_out[env] = out_bits;
    }
    if (AE.ticks_out) AE.ticks_out[env] = ticks;
    if (AE.ready_out) AE.ready_out[env] = ready ? 1 : 0;
  }
  if (ready && AE.obs_out && lie_e == 0) {  // the test ship's first lane holds the env's observation
#pragma unroll
    for (int i = 0; i < 8; ++i) AE.obs_out[env * 8 + i] = ns[i];
  }
}

#undef OPM_GET
#undef OPM_SET

// C2 single-ship loop body, k ticks per launch (one lane per ship; algebraic wind force)
template <bool DETAILED>
__global__ __launch_bounds__(64) void single_tick_kernel(const Params P, DevState S, ConstBuf K, int k) {
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  const ShipConst* SC = stage_consts(K, lds_sc, P.n_ships, P.dt);
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P.n_envs) return;
  const ShipConst& c = SC[0];
  const double* rn = S.route_n() + (size_t)q * kMaxRoute;
  const double* re = S.route_e() + (size_t)q * kMaxRoute;
  Ship s;
  load_ship(S, q, s);
  const double mach_dt = S.mach_dt()[q];
  double wsin, wcos;
  sincos(P.wind_dir, &wsin, &wcos);
  for (int i = 0; i < k; ++i)
    control_and_integrate<DETAILED, false, false, true>(c, P, s, rn, re, 0.0, 1.0, mach_dt, 0, false, nullptr, nullptr,
                                                        false, wsin, wcos);
  store_ship(S, q, s);
}

// Legacy per-tick MultiShipEnv.step (rl_env/ship_in_transit/env.py:1104-1173), k steps per launch.
// Two lanes per env (lane & 1 = ship); the termination flags of get_termination_status
// (termination_flags.py:5-70) are evaluated in fp64 on the next_states, as the reference does on
// its Python-float list.
// Arguments read through the kernarg segment pointer (as step_args): the Params block and the state base
// addresses are scalar loads where a tick uses them, not argument SGPRs held (and spilled) across the loop.
struct LegacyArgs {
  Params P;
  DevState S;
  ConstBuf K;
  int k;
  double* states_out;
  uint8_t* done_out;
  uint32_t* status_out;
};
typedef const __attribute__((address_space(4))) LegacyArgs* LegacyArgsPtr;
__device__ __forceinline__ const LegacyArgs& legacy_args() {
  LegacyArgsPtr q = (LegacyArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(q));
  return *(const LegacyArgs*)q;
}

template <bool DETAILED, int COLLAV>
__global__ __launch_bounds__(64) void legacy_step_kernel(LegacyArgs a_arg) {
  (void)a_arg;  // read through legacy_args()
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  __shared__ Edge lds_edges_raw[SHIPSIM_MAX_VERTS];
  __shared__ PolyBox lds_boxes[SHIPSIM_MAX_POLYS];
  const LegacyArgs& A0 = legacy_args();
  const ShipConst* SC = stage_consts(A0.K, lds_sc, A0.P.n_ships, A0.P.dt);
  for (int i = threadIdx.x; i < A0.K.n_edges; i += blockDim.x) lds_edges_raw[i] = A0.K.edges()[i];
  for (int i = threadIdx.x; i < A0.P.n_polys; i += blockDim.x) lds_boxes[i] = A0.K.boxes()[i];
  __syncthreads();

  const int gl = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = gl >> 1;
  const int ship = gl & 1;
  const bool is_test = ship == 0;
  const bool valid = env < A0.P.n_envs;
  const int envc = valid ? env : 0;
  const int qc = envc * 2 + ship;
  const ShipConst& c = SC[ship];
  const double* rn = A0.S.route_n() + (size_t)qc * kMaxRoute;
  const double* re = A0.S.route_e() + (size_t)qc * kMaxRoute;
  Ship s;
  load_ship(A0.S, qc, s);
  double p_last = A0.S.p_last()[envc], chi_last = A0.S.chi_last()[envc];
  const double mach_dt = A0.S.mach_dt()[envc];
  const double* lst = A0.S.legacy_states() + (size_t)envc * 4;  // self.states [test n, e, obs n, e]
  double st[4] = {lst[0], lst[1], lst[2], lst[3]};
  bool st_f32 = A0.S.legacy_flags()[envc] & 1;
  const int n_samp = (int)(A0.P.sbmpc_tf / A0.P.sbmpc_dt);

  double out8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t status = 0;
  bool done = false, ticked = false;
  bool going = valid;
  for (int it = 0; it < legacy_args().k; ++it) {
    if (!__any(going)) break;
    // this tick's constants: re-read through the kernarg pointer rather than kept in registers across ticks
    const LegacyArgs& A = legacy_args();
    const Params& P = A.P;
    const ConstBuf& K = A.K;
    const double pn = pair_swap(s.n), pe = pair_swap(s.e), pyaw = pair_swap(s.yaw);
    const double pu = pair_swap(s.u), pv = pair_swap(s.v);
    double sf = 1.0, off = 0.0;
    if (COLLAV == SHIPSIM_COLLAV_SBMPC) {  // test_step :938-963 (obstacle ship before it moves)
      bool need = false;
      SbIn in = SbIn{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      in.u_d = SC[0].desired_speed;  // the same in every lane (sbmpc_cooperative<true>)
      in.obs_l = SC[1].obs_l_cfg; in.obs_w = SC[1].obs_w_cfg;
      if (going && is_test) {
        const double los_arg = los_update(c, s, s.n, s.e);
        const double d0 = pe - s.e, d1 = pn - s.n;
        need = sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_
        need = diag::sb_request(need, P.max_sampling);  // (the product: need itself)
        if (need) in.chi_d = -(s.seg_alpha + atan(los_arg));
        in.os_x = s.e; in.os_y = s.n; in.os_v = s.v;
        in.ob_x = pe; in.ob_y = pn; in.ob_psi = -pyaw; in.ob_u = pu; in.ob_v = pv;
        sb_set_heading_trig(in);
        in.p_last = p_last; in.chi_last = chi_last;
      }
      double pb = 1.0, cb = 0.0;
      sbmpc_cooperative<true>(need, in, n_samp, P.sbmpc_dt, pb, cb);
      if (going && is_test) {
        if (need) { p_last = pb; chi_last = cb; sf = pb; off = cb; }
        else { p_last = 1; chi_last = 0; }
      }
    }
    double speed_out = 0.0;
    if (going) {
      if (!is_test && s.stop) {  // obs_step :1029-1056: store_last + two next_time, speed reported 0
        s.time = s.time + P.dt;
        s.time = s.time + P.dt;
      } else {
        bool imminent = false;
        if (COLLAV == SHIPSIM_COLLAV_SIMPLE && is_test) {  // is_collision_imminent(self.states[0:2], [3:5])
          if (st_f32) {
            const float dn = P.initial_states[0] - P.initial_states[3], de = P.initial_states[1] - P.initial_states[4];
            imminent = (dn * dn + de * de) < 9000000.0f;
          } else {
            imminent = ((st[0] - st[2]) * (st[0] - st[2]) + (st[1] - st[3]) * (st[1] - st[3])) < 9000000.0;
          }
        }
        speed_out = s.u;
        control_and_integrate<DETAILED>(c, P, s, rn, re, -off, sf, mach_dt,
                                        (COLLAV == SHIPSIM_COLLAV_SIMPLE && is_test) ? 1 : 0, imminent);
      }
    }
    // own-ship flags on the post-tick state (check_condition.py)
    bool my_end = false, my_out = false, my_gr = false;
    if (going) {
      const double margin = c.l_ship / 2;
      my_end = sqrt_le((s.n - s.end_n) * (s.n - s.end_n) + (s.e - s.end_e) * (s.e - s.end_e), 200.0);
      my_out = (s.n < P.min_north + margin || s.n > P.max_north - margin) ||
               (s.e < P.min_east + margin || s.e > P.max_east - margin);
      for (int q = 0; q < 4; ++q) {
        const double cn = (q < 2) ? s.n - margin : s.n + margin;
        const double ce = (q & 1) ? s.e + margin : s.e - margin;
        if (corner_inside(K, lds_edges_raw, lds_boxes, P.n_polys, cn, ce)) my_gr = true;
      }
    }
    const bool my_nav = fabs(s.log_ect) > 500;  // is_ship_navigation_failure (e_tol 500, both ships)
    const int my_flags = (my_end ? 1 : 0) | (my_out ? 2 : 0) | (my_gr ? 4 : 0) | (my_nav ? 8 : 0);
    const int o_flags = pair_swap_i(my_flags);
    const double o_n = pair_swap(s.n), o_e = pair_swap(s.e), o_yaw = pair_swap(s.yaw);
    const double o_ect = pair_swap(s.log_ect), o_speed = pair_swap(speed_out);
    if (going) {
      const double Tn = is_test ? s.n : o_n, Te = is_test ? s.e : o_e;
      const double On = is_test ? o_n : s.n, Oe = is_test ? o_e : s.e;
      const int Tf = is_test ? my_flags : o_flags, Of = is_test ? o_flags : my_flags;
      out8[0] = Tn; out8[1] = Te; out8[2] = is_test ? s.log_ect : o_ect;
      out8[3] = On; out8[4] = Oe; out8[5] = is_test ? o_yaw : s.yaw;
      out8[6] = is_test ? o_speed : speed_out; out8[7] = is_test ? o_ect : s.log_ect;
      const double cd = (Tn - On) * (Tn - On) + (Te - Oe) * (Te - Oe);
      status = (uint32_t)(Tf & 15) | (cd < 9000000.0 ? SHIPSIM_LT_NEAR_COLLISION : 0u) |
               (cd < 2500.0 ? SHIPSIM_LT_COLLISION : 0u) | ((uint32_t)(Of & 15) << 6);
      done = (status & (SHIPSIM_LT_TEST_REACHED | SHIPSIM_LT_TEST_OUTSIDE | SHIPSIM_LT_TEST_GROUNDED |
                        SHIPSIM_LT_TEST_NAV_FAILURE | SHIPSIM_LT_COLLISION | SHIPSIM_LT_OBS_GROUNDED |
                        SHIPSIM_LT_OBS_NAV_FAILURE)) != 0;
      // stop_int_obs = obs_is_outside and obs_is_reached (:1168-1171)
      if (!is_test && (Of & 2) && (Of & 1)) s.stop = 1;
      st[0] = Tn; st[1] = Te; st[2] = On; st[3] = Oe;
      st_f32 = false;
      ticked = true;
      going = !done;
    }
  }
  if (!valid) return;
  const LegacyArgs& A = legacy_args();
  const DevState S = opaque(A.S);
  store_ship(S, qc, s);
  if (is_test) {
    S.p_last()[env] = p_last; S.chi_last()[env] = chi_last;
    double* lsto = S.legacy_states() + (size_t)env * 4;
    for (int i = 0; i < 4; ++i) lsto[i] = st[i];
    S.legacy_flags()[env] = st_f32 ? 1 : 0;
    if (ticked) {
      if (A.states_out)
        for (int i = 0; i < 8; ++i) A.states_out[(size_t)env * 8 + i] = out8[i];
      if (A.done_out) A.done_out[env] = done ? 1 : 0;
      if (A.status_out) A.status_out[env] = status;
    }
  }
}

// C1: MultiShipNonIWEnv._step (run_colav/env.py:613-676) inside the run_simplified_model.py:245-249 loop, k ticks per
// launch (shipsim_tick). Two lanes per env (lane & 1 = ship); both ships follow fixed routes. Per tick, in the
// reference's order: the test ship's step (test_step :326-455: the SBMPC block when collav is sbmpc, control with the
// simple collision avoidance's +15° when imminent, one ship tick), then the obstacle ship's (obs_step :457-586: the
// same SBMPC block — its own LOS course and desired speed, the test ship's state after its tick as the own ship, the
// obstacle ship itself as the obstacle — then control and tick), each frozen ship storing its last row and advancing
// its clock twice instead; then get_env_info (:53-225, the flags of reward_function.py without the rewards) on the
// post-tick states and the stop flags (:658-664). The env's SBMPC memory (P_ca_last, Chi_ca_last) is one object that
// both ships' blocks update in turn. Event bits of the last tick to events_out.
// (its arguments as one struct read through the laundered kernarg pointer, as ast_step_kernel's StepArgs: a field is
// a scalar load where it is used, not ~100 dwords held in SGPRs across the tick loop, which spilled)
struct NoniwArgs {
  Params P;
  DevState S;
  ConstBuf K;
  int k;
  uint32_t* events_out;
};
typedef const __attribute__((address_space(4))) NoniwArgs* NoniwArgsPtr;
__device__ __forceinline__ const NoniwArgs& noniw_args() {
  NoniwArgsPtr q = (NoniwArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(q));
  return *(const NoniwArgs*)q;
}
template <int COLLAV>
__global__ __launch_bounds__(64) void noniw_tick_kernel(NoniwArgs A_arg) {
  (void)A_arg;  // read through noniw_args()
#define P (noniw_args().P)
#define S (noniw_args().S)
#define K (noniw_args().K)
  const int k = noniw_args().k;
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  __shared__ Edge lds_edges_raw[SHIPSIM_MAX_VERTS];
  __shared__ PolyBox lds_boxes[SHIPSIM_MAX_POLYS];
  const ShipConst* SC = stage_consts(K, lds_sc, P.n_ships, P.dt);
  for (int i = threadIdx.x; i < K.n_edges; i += blockDim.x) lds_edges_raw[i] = K.edges()[i];
  for (int i = threadIdx.x; i < P.n_polys; i += blockDim.x) lds_boxes[i] = K.boxes()[i];
  __syncthreads();
  const int gl = blockIdx.x * blockDim.x + threadIdx.x;
  const int env = gl >> 1, ship = gl & 1;
  const bool is_test = ship == 0;
  const bool valid = env < P.n_envs;  // (invalid lanes run along: every lane takes part in the exchanges)
  const int envc = valid ? env : 0, qc = envc * 2 + ship;
  const ShipConst& c = SC[ship];
  const double* rn = S.route_n() + (size_t)qc * kMaxRoute;
  const double* re = S.route_e() + (size_t)qc * kMaxRoute;
  Ship s;
  load_ship(S, qc, s);
  double sy, cy;
  sincos(s.yaw, &sy, &cy);
  double p_last = S.p_last()[envc], chi_last = S.chi_last()[envc];
  float st[4];  // self.states (float32): test (n, e), obstacle (n, e) as the previous tick left them
  for (int i = 0; i < 4; ++i) st[i] = S.states4()[envc * 4 + i];
  const int n_samp = (int)(P.sbmpc_tf / P.sbmpc_dt);
  constexpr int kFlag = COLLAV == SHIPSIM_COLLAV_SIMPLE ? 2 : 0;  // the +15° avoidance (control_and_store)
  uint32_t bits = 0;
  for (int it = 0; it < k; ++it) {
    const float dn = st[0] - st[2], de = st[1] - st[3];
    const bool imminent = (dn * dn + de * de) < 9000000.0f;  // is_collision_imminent on self.states
    // one ship's step: its SBMPC block (need: the own ship within D_INIT of the obstacle) and control + tick
    auto ship_step = [&](int who, double os_n, double os_e, double os_v, double ob_n, double ob_e, double ob_yaw,
                         double ob_u, double ob_v) __attribute__((always_inline)) {
      const bool mine = ship == who;
      double sf = 1.0, off = 0.0;
      if constexpr (COLLAV == SHIPSIM_COLLAV_SBMPC) {
        const bool act = valid && mine && !s.stop;
        bool need = false;
        double los_arg = 0.0;
        if (act) {  // next_wpt's result discarded; los_guidance integrates e_ct_int (Q3)
          los_arg = los_update(c, s, s.n, s.e);
          const double d0 = ob_e - os_e, d1 = ob_n - os_n;
          need = sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_
        }
        double pb = 1.0, cb = 0.0;
        if (__any(need)) {
          SbIn in = SbIn{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
          in.u_d = SC[who].desired_speed;  // (every request of this pass is ship `who`'s: the same in each lane)
          in.obs_l = SC[1].obs_l_cfg; in.obs_w = SC[1].obs_w_cfg;
          if (need) {
            in.chi_d = -(s.seg_alpha + atan(los_arg));
            in.os_x = os_e; in.os_y = os_n; in.os_v = os_v;
            in.ob_x = ob_e; in.ob_y = ob_n; in.ob_psi = -ob_yaw; in.ob_u = ob_u; in.ob_v = ob_v;
            sb_set_heading_trig(in);
            in.p_last = p_last; in.chi_last = chi_last;
          }
          sbmpc_cooperative<true, true>(need, in, n_samp, P.sbmpc_dt, pb, cb);
        }
        if (act) {
          if (need) { p_last = pb; chi_last = cb; sf = pb; off = cb; }
          else { p_last = 1; chi_last = 0; }
        }
      }
      if (valid && mine) {
        if (s.stop) {  // store_last_simulation_data + two next_time
          s.time = s.time + P.dt;
          s.time = s.time + P.dt;
        } else {
          control_and_integrate_sc<false, false>(c, P, P, s, rn, re, -off, sf, 0.0, kFlag, imminent, nullptr, nullptr,
                                                 sy, cy);
        }
      }
    };
    {  // the test ship: the obstacle ship before it moves
      const double pn = pair_swap(s.n), pe = pair_swap(s.e), pyaw = pair_swap(s.yaw);
      const double pu = pair_swap(s.u), pv = pair_swap(s.v);
      ship_step(0, s.n, s.e, s.v, pn, pe, pyaw, pu, pv);
    }
    {  // the obstacle ship: the test ship after its tick, the env's SBMPC memory as the test ship's block left it
      const double tn = pair_swap(s.n), te = pair_swap(s.e), tv = pair_swap(s.v);
      const double pl = pair_swap(p_last), cl = pair_swap(chi_last);
      if (!is_test) { p_last = pl; chi_last = cl; }
      ship_step(1, tn, te, tv, s.n, s.e, s.yaw, s.u, s.v);
      const double pl2 = pair_swap(p_last), cl2 = pair_swap(chi_last);
      if (is_test) { p_last = pl2; chi_last = cl2; }
    }
    // get_env_info on the post-tick states (check_condition.py), both ships' own flags exchanged
    const double margin = c.l_ship / 2;
    const bool my_end = sqrt_le((s.n - s.end_n) * (s.n - s.end_n) + (s.e - s.end_e) * (s.e - s.end_e), 200.0);
    const bool my_out = (s.n < P.min_north + margin || s.n > P.max_north - margin) ||
                        (s.e < P.min_east + margin || s.e > P.max_east - margin);
    bool my_gr = false;
    for (int q = 0; q < 4; ++q) {
      const double cn = (q < 2) ? s.n - margin : s.n + margin;
      const double ce = (q & 1) ? s.e + margin : s.e - margin;
      if (corner_inside(K, lds_edges_raw, lds_boxes, P.n_polys, cn, ce)) my_gr = true;
    }
    const bool my_nav = fabs(s.log_ect) > (is_test ? 3000.0 : 500.0);  // is_tnav / is_onav (no travel tracker)
    const int my_flags = (my_end ? 1 : 0) | (my_out ? 2 : 0) | (my_gr ? 4 : 0) | (my_nav ? 8 : 0);
    const int o_flags = pair_swap_i(my_flags);
    const double on = pair_swap(s.n), oe = pair_swap(s.e);
    const int Tf = is_test ? my_flags : o_flags, Of = is_test ? o_flags : my_flags;
    const double cd = (s.n - on) * (s.n - on) + (s.e - oe) * (s.e - oe);
    const bool t10 = pair_swap(s.time) > P.sim_time;  // (the test ship's clock: read on its partner lane too)
    const bool t10_t = s.time > P.sim_time;
    const bool f[10] = {cd < 2500.0, (Tf & 4) != 0, (Tf & 8) != 0, (Of & 4) != 0, (Of & 8) != 0,
                        (Tf & 1) != 0, (Tf & 2) != 0, (Of & 1) != 0, (Of & 2) != 0, is_test ? t10_t : t10};
    bits = 0;
    for (int i = 0; i < 10; ++i)
      if (f[i]) bits |= 1u << i;
    if (bits & 0x1Fu) bits |= SHIPSIM_EV_TERMINAL;
    if (bits & 0x267u) bits |= SHIPSIM_EV_TEST_STOP;  // collision, test grounding / nav, test end / outside, time
    if (bits & 0x399u) bits |= SHIPSIM_EV_OBS_STOP;   // collision, obs grounding / nav, obs end / outside, time
    const bool terminal = bits & SHIPSIM_EV_TERMINAL;
    if (valid && !terminal && (bits & (is_test ? SHIPSIM_EV_TEST_STOP : SHIPSIM_EV_OBS_STOP))) s.stop = 1;
    const double Tn = is_test ? s.n : on, Te = is_test ? s.e : oe, On = is_test ? on : s.n, Oe = is_test ? oe : s.e;
    st[0] = (float)Tn; st[1] = (float)Te; st[2] = (float)On; st[3] = (float)Oe;
  }
  if (!valid) return;
  store_ship(S, qc, s);
  if (is_test) {
    S.p_last()[env] = p_last; S.chi_last()[env] = chi_last;
    for (int i = 0; i < 4; ++i) S.states4()[env * 4 + i] = st[i];
    uint32_t* events_out = noniw_args().events_out;
    if (events_out && k > 0) events_out[env] = bits;
  }
#undef P
#undef S
#undef K
}

// SBMPC.get_optimal_ctrl_offset (sbmpc.py:113-185) for a batch of independent single-obstacle
// requests (shipsim_sbmpc_eval): one request per lane, optimisations served wave-cooperatively.
__global__ __launch_bounds__(64) void sbmpc_eval_kernel(int n, double tf, double dt, const double* __restrict__ in,
                                                        double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const bool valid = i < n;
  const double* r = in + (size_t)(valid ? i : 0) * SHIPSIM_SBMPC_IN;
  SbIn q;
  q.p_last = r[0]; q.chi_last = r[1]; q.u_d = r[2]; q.chi_d = r[3];
  q.os_x = r[4]; q.os_y = r[5]; q.os_v = r[8];  // os_state (x, y, psi, u, v, r): linear_pred uses x, y, v
  q.ob_x = r[10]; q.ob_y = r[11]; q.ob_psi = r[12]; q.ob_u = r[13]; q.ob_v = r[14];
  sb_set_heading_trig(q);
  q.obs_l = r[15]; q.obs_w = r[16];
  const double d0 = q.ob_x - q.os_x, d1 = q.ob_y - q.os_y;
  const bool active = valid && sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_ (sbmpc.py:154-159)
  double pb = 1.0, cb = 0.0;
  sbmpc_cooperative(active, q, (int)(tf / dt), dt, pb, cb);
  if (valid) {
    out[(size_t)i * 3 + 0] = active ? pb : 1.0;
    out[(size_t)i * 3 + 1] = active ? cb : 0.0;
    out[(size_t)i * 3 + 2] = active ? 1.0 : 0.0;
  }
}

// sbmpc_nominal_holds (shipsim_sbmpc_nominal.hpp) over shipsim_sbmpc_eval's request rows (shipsim_sbmpc_nominal): one
// request per lane, reachable for requests the streams' trajectories never form. flag_out[i] bit 0: the test with
// sin / cos(chi_d); bit 1: the form the streams' tick evaluates (sbmpc_nominal_holds_seg), on the course split into
// a segment angle and a correction's argument by sbmpc_nominal_split_course.
__global__ __launch_bounds__(64) void sbmpc_nominal_kernel(int n, double tf, double dt, const double* __restrict__ in,
                                                           int32_t* __restrict__ flag_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* r = in + (size_t)i * SHIPSIM_SBMPC_IN;
  SbIn q;
  q.p_last = r[0]; q.chi_last = r[1]; q.u_d = r[2]; q.chi_d = r[3];
  q.os_x = r[4]; q.os_y = r[5]; q.os_v = r[8];
  q.ob_x = r[10]; q.ob_y = r[11]; q.ob_psi = r[12]; q.ob_u = r[13]; q.ob_v = r[14];
  sb_set_heading_trig(q);
  q.obs_l = r[15]; q.obs_w = r[16];
  double seg_sin, seg_cos, a;
  sbmpc_nominal_split_course(q.chi_d, seg_sin, seg_cos, a);
  const int n_samp = (int)(tf / dt);
  flag_out[i] = (sbmpc_nominal_holds(q, n_samp, dt).holds ? 1 : 0) |
                (sbmpc_nominal_holds_seg(q, seg_sin, seg_cos, a, n_samp, dt).holds ? 2 : 0);
}

// The tick's three math-library calls over n arguments, one per lane (shipsim_tickmath_eval): the device library's
// value, the restated form's with literal constants (TickMath<3>) and the row-broadcast form's (TickMath<7>), as the
// headline streams call them. fn 0 sincos (sine, cosine), 1 atan, 2 exp (second value 0). Lanes past n evaluate the
// last argument and write nothing, so every lane of a row is active at the broadcasts.
__global__ __launch_bounds__(64) void tickmath_eval_kernel(int fn, int n, const double* __restrict__ x,
                                                           double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const double a = x[i < n ? i : n - 1];
  const int lane = (int)(threadIdx.x & 63);
  TickMath<3> lit;
  lit.row_lane0 = lane & ~15;
  TickMath<7> row;
  row.row_lane0 = lane & ~15;
  row.row.load(lane & 15);
  double v[6] = {0, 0, 0, 0, 0, 0};
  if (fn == 0) {
    sincos(a, &v[0], &v[1]);
    lit.sincos_yaw(a, &v[2], &v[3]);
    row.sincos_yaw(a, &v[4], &v[5]);
  } else if (fn == 1) {
    v[0] = atan(a);
    v[2] = lit.atan_los(a);
    v[4] = row.atan_los(a);
  } else {
    v[0] = exp(a);
    v[2] = lit.exp_reward(a);
    v[4] = row.exp_reward(a);
  }
  if (i < n) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[(size_t)i * 6 + k] = v[k];
  }
}

// SBMPC.get_optimal_ctrl_offset over a do_list of n_obs obstacles (sbmpc.py:113-185) for n independent requests
// (shipsim_sbmpc_eval_multi): one request per lane, the optimisations served wave-cooperatively by the optimiser the
// multi-obstacle env kernels run (sbmpc_cooperative_multi<NOB>), in the instantiations they run it in: the service
// mirrors the env kernels of the same K (shipsim_sbmpc_eval_multi picks NOB), and reads NOB slots of a row
template <int NOB>
__global__ __launch_bounds__(64) void sbmpc_multi_eval_kernel(int n, int n_obs, int n_samp, double dt,
                                                              const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const bool valid = i < n;
  const double* r = in + (size_t)(valid ? i : 0) * SHIPSIM_SBMPC_MULTI_IN;
  SbMulti<NOB> q;
  q.p_last = r[0]; q.chi_last = r[1]; q.u_d = r[2]; q.chi_d = r[3];
  q.os_x = r[4]; q.os_y = r[5]; q.os_v = r[8];  // os_state (x, y, psi, u, v, r): linear_pred uses x, y, v
  bool active = false;
#pragma unroll
  for (int k = 0; k < NOB; ++k) {
    const double* o = r + 10 + 7 * k;
    q.ob_x[k] = o[0]; q.ob_y[k] = o[1]; q.ob_psi[k] = o[2]; q.ob_u[k] = o[3]; q.ob_v[k] = o[4];
    q.obs_l[k] = o[5]; q.obs_w[k] = o[6];
    const double d0 = o[0] - q.os_x, d1 = o[1] - q.os_y;
    if (k < n_obs) active = active || sqrt_lt(d0 * d0 + d1 * d1, 2000.0);  // D_INIT_ (sbmpc.py:153-159)
  }
  active = valid && active;
  double pb = 1.0, cb = 0.0;
  sbmpc_cooperative_multi<NOB>(active, q, n_obs, n_samp, dt, pb, cb);  // (n_samp: int(tf / dt))
  if (valid) {
    out[(size_t)i * 3 + 0] = active ? pb : 1.0;
    out[(size_t)i * 3 + 1] = active ? cb : 0.0;
    out[(size_t)i * 3 + 2] = active ? 1.0 : 0.0;
  }
}

// shipsim_div_check: div_by with div_rcp (the kernels' division by a reused divisor) beside the plain division
__global__ __launch_bounds__(256) void div_check_kernel(int n, const double* __restrict__ num,
                                                        const double* __restrict__ den, double* __restrict__ fast,
                                                        double* __restrict__ ref) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = num[i], d = den[i];
  fast[i] = div_by(a, d, div_rcp(d));
  ref[i] = a / d;
}

// The decision streams' slot -> env order (shipsim_set_stream_grouping; host half: shipsim_grouping_host.hpp):
// slot_env sorted by the envs' ticks since their last reset, ties by env index. Rank by counting: thread i counts the
// envs that sort before env i, over tiles of kOrderThreads keys staged in LDS, and stores i at that slot — ranks of
// a total order are a permutation, so every slot is written exactly once, without atomics and in bounded loops.
// Every thread of a block takes part in the staging and its barriers; threads past n_envs store nothing.
constexpr int kOrderThreads = 256;
__device__ __forceinline__ int32_t stream_order_key(double time, double dt) {  // grouping_host::key_of
  const double q = rint(time / dt);
  if (!(q > 0.0)) return 0;
  return q >= (double)grouping_host::kMaxKey ? grouping_host::kMaxKey : (int32_t)q;
}
__global__ __launch_bounds__(kOrderThreads) void stream_order_kernel(const double* __restrict__ time, int n_envs,
                                                                     int n_ships, double dt,
                                                                     int32_t* __restrict__ slot_env) {
  __shared__ int32_t tile[kOrderThreads];
  const int i = blockIdx.x * kOrderThreads + threadIdx.x;
  const int32_t mine = i < n_envs ? stream_order_key(time[(size_t)i * n_ships], dt) : 0;  // (the test ship's clock)
  int32_t rank = 0;
  for (int base = 0; base < n_envs; base += kOrderThreads) {
    const int j = base + (int)threadIdx.x;
    // (a tile's slots past n_envs hold a key above every env's: never counted)
    tile[threadIdx.x] = j < n_envs ? stream_order_key(time[(size_t)j * n_ships], dt) : INT32_MAX;
    __syncthreads();
    // the envs of an earlier tile have smaller indices than this block's, those of a later one larger: one
    // comparison per env there, the index only within the block's own tile (block-uniform branches)
    const int own = (int)blockIdx.x * kOrderThreads;
    if (base < own) {
#pragma unroll 8
      for (int t = 0; t < kOrderThreads; ++t) rank += tile[t] <= mine ? 1 : 0;
    } else if (base > own) {
#pragma unroll 8
      for (int t = 0; t < kOrderThreads; ++t) rank += tile[t] < mine ? 1 : 0;
    } else {
#pragma unroll 8
      for (int t = 0; t < kOrderThreads; ++t) {
        const int32_t k = tile[t];
        rank += (k < mine || (k == mine && t < (int)threadIdx.x)) ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (i < n_envs) slot_env[rank] = i;  // (rank < n_envs: it counts envs other than i)
}
__global__ __launch_bounds__(kOrderThreads) void stream_identity_kernel(int n_envs, int32_t* __restrict__ slot_env) {
  const int i = blockIdx.x * kOrderThreads + threadIdx.x;
  if (i < n_envs) slot_env[i] = i;
}

// shipsim_fork: env i of dst becomes env src_env[i] of src, for every column of the state block in one launch.
// blockIdx.y is the column (state_host::table); a column of n_envs * env_bytes bytes is n_envs * (env_bytes / unit)
// units, unit t of it lying at offset + t * unit, so consecutive lanes store consecutive units (consecutive envs for
// the one-element columns, the 16-byte pieces of one env's route rows for the routes) and only the loads are
// gathered. The blocks of a column stride over its units. src and dst never overlap (a fork from the live state
// goes through the staging block). An index outside [0, n_envs) is tested before any address is formed from it:
// env i then keeps src's env i (own_fallback: dst is the staging copy of src) or is not written at all (dst is the
// live block, src a snapshot).
__global__ __launch_bounds__(256) void fork_gather_kernel(const state_host::Table T, const char* __restrict__ src,
                                                          char* __restrict__ dst, const int32_t* __restrict__ src_env,
                                                          uint32_t n_envs, int own_fallback) {
  const state_host::Column c = T.col[blockIdx.y];
  const uint32_t per_env = state_host::units_per_env(c);
  const uint32_t total = n_envs * per_env;  // (<= 2^31, and the stride <= 2^18: the host's kForkMaxUnits / -Blocks)
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < total; t += stride) {
    const uint32_t env = t / per_env, piece = t - env * per_env;
    uint32_t from = env;
    if (src_env) {
      const uint32_t s = (uint32_t)src_env[env];
      if (s < n_envs) from = s;       // (a negative index is >= 2^31 here)
      else if (!own_fallback) continue;
    }
    const char* p = src + state_host::unit_src(c, from, piece);
    char* q = dst + state_host::unit_dst(c, t);
    if (c.unit == 16) *(uint4*)q = *(const uint4*)p;
    else if (c.unit == 8) *(uint2*)q = *(const uint2*)p;
    else *(uint32_t*)q = *(const uint32_t*)p;
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct shipsim_handle {
  shipsim_config cfg;
  Params P;
  DevState S;
  ConstBuf K;
  int device;
  hipStream_t stream;
  void* dev_block;
  void* const_block;
  void* fuel_block;  // trajectory fuel accumulators
  int32_t* nonfinite_dev;   // device counter (DevState::nonfinite)
  int32_t nonfinite_seen;   // its value at the last shipsim_synchronize
  Traj T;
  size_t dev_bytes;
  int ever_reset;
  int lpe;  // lanes per AST env of the step / stream kernels (lanes_per_env)
  int32_t tail_extra;  // shipsim_set_stream_tail (0: off)
  int32_t* tail_ctr;   // its device counter (one int, zeroed before every stream launch)
  // shipsim_set_weather: the per-env weather table on the device (weather_host::kStoreRows x n_envs, an allocation of
  // its own: the kWeatherCols rows the kernels read, then the wind direction as set), the caller's four arrays as
  // given (4 x n_envs, host: shipsim_get_weather), whether the handle runs on them, and the lanes per env the
  // handle runs without them (lpe while they are set: the nearest weather kernel's)
  double* wx_dev;
  double* wx_host;
  int wx_on;
  int lpe_uniform;
  // shipsim_weather_fork gathers into this table of the same size and copies it back (allocated with wx_dev); and
  // whether a weather_store / _load / _fork has ever been called on the handle, a capture included: from then on the
  // device table, which a graph replay changes without a host call, is what shipsim_get_weather reads
  double* wx_stage;
  int wx_moved;
  // shipsim_fork from the live state gathers into this block of dev_bytes and copies it back (allocated at the
  // first such call)
  void* fork_block;
  // shipsim_set_stream_grouping: the switch (grouping_host::default_on from create), the slot -> env permutation on
  // the device (grouping_host::buffer_len entries, the identity from create; NULL: more envs than the handle
  // groups), and whether it holds the identity now (what a launch with the switch off leaves behind)
  int group_on;
  int32_t* slot_env;
  int slot_identity;
  char err[512];
};

static int fail(shipsim_handle* h, int code, const char* fmt, ...) {
  if (h) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h->err, sizeof(h->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define HIPCHK(h, x)                                                              \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) return fail(h, SHIPSIM_EHIP, "%s: %s", #x, hipGetErrorString(e_)); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Lanes per AST env. The kernels hold ~350-450 registers per lane, so a SIMD runs one wave and the
// throughput is (envs per wave) / (per-tick wave latency): pick the fewest lanes per env that still
// put a wave on every SIMD of the device (n_envs * LPE / 64 >= SIMDs), in [4, 16]. Measured on
// MI355X (profiles/round2_lpe_sweep.md): 4096 envs -> 16, 8192 -> 8 (1.5-1.8x over 16), 65536 -> 4
// (2.2-3.1x). cfg->lanes_per_env (or $SHIPSIM_LPE) overrides; results are identical at every LPE.
static int lanes_per_env(const shipsim_config* cfg, int n_envs, int device) {
  int lpe = cfg->lanes_per_env;
  if (lpe <= 0) {
    const char* e = getenv("SHIPSIM_LPE");
    lpe = e ? atoi(e) : 0;
  }
  if (lpe == 2 || lpe == 4 || lpe == 8 || lpe == 16) return lpe;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  const long simds = 4L * cus;
  lpe = 4;
  while (lpe < 16 && (long)n_envs * lpe < 64L * simds) lpe *= 2;
  return lpe;
}

// blocks (one wave each) of an AST step / stream launch at lpe lanes per env
static int step_blocks(const shipsim_handle* h, int lpe) {
  const int epw = h->P.epw > 0 && h->P.epw <= 64 / lpe ? h->P.epw : 64 / lpe;
  return (h->P.n_envs + epw - 1) / epw;
}

// The step kernels of the library: shipsim_launch_host.hpp's list, expanded here and nowhere else. A register-usage
// inspection build (scripts/regcheck.sh N) holds one kernel set only: the other rows are not instantiated and
// their entries are null.
constexpr bool step_kernel_built(bool d, int ca, int lpe, bool rec, int mode, int slots) {
#ifdef SHIPSIM_REGCHECK
  const bool stream2 = (mode == 1 || mode == 2) && slots == 2;  // a two-ship decision stream, the config's weather
  return SHIPSIM_REGCHECK == 2 ? stream2 && ca == SHIPSIM_COLLAV_SBMPC && lpe == 8  // the C4 shard's collector
         : SHIPSIM_REGCHECK == 3                                                    // K > 1: steps and streams
             ? slots > 2 && mode < kStepWeather && !(mode == 1 && ca == SHIPSIM_COLLAV_NONE)
             : stream2 && d && ca != SHIPSIM_COLLAV_SIMPLE && lpe == 16;            // the headline streams
#else
  return true;
#endif
}
typedef void (*StepKernel)(const StepArgs);
template <bool BUILT, bool D, int CA, int LPE, bool REC, int MODE, int SLOTS>
constexpr StepKernel step_kernel_if() {
  if constexpr (BUILT) return &ast_step_kernel<D, CA, LPE, REC, MODE, SLOTS>;
  else return nullptr;
}
static const struct { int key; StepKernel kern; } kStepKernels[] = {
#define ROW(D, CA, LPE, REC, MODE, SLOTS)          \
  {launch_host::step_key(D, CA, LPE, REC, MODE, SLOTS), \
   step_kernel_if<step_kernel_built(D, CA, LPE, REC, MODE, SLOTS), D, CA, LPE, REC, MODE, SLOTS>()},
    SHIPSIM_STEP_KERNELS(ROW)
#undef ROW
};
static_assert(launch_host::kWeatherMode == kStepWeather, "MODE's weather bit");

// what launch_host::select says of this handle at an entry point
static launch_host::Selection selection(const shipsim_handle* h, launch_host::Entry entry) {
  return launch_host::select(h->P.machinery, h->P.collav, h->P.n_ships, h->lpe_uniform, h->T.ship != nullptr,
                             h->wx_on != 0, entry);
}

// the launch tail is used when it is on and every wave of the launch is resident at once (one 64-thread block per
// wave): a wave that is not resident yet would only start after the resident ones ran their whole extension
static bool tail_on(const shipsim_handle* h, const void* kern, int blocks) {
  if (h->tail_extra <= 0 || !h->tail_ctr) return false;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64, 0) != hipSuccess) return false;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) return false;
  return (int64_t)blocks <= (int64_t)per_cu * cus;
}

// Every launch of a step kernel: shipsim_step, shipsim_run_table and shipsim_run_policy.
static int launch_ast(shipsim_handle* h, launch_host::Entry entry, const float* action, const uint8_t* active,
                      int32_t max_ticks, float* obs_out, double* reward_out, uint8_t* done_out, uint32_t* events_out,
                      int32_t* ticks_out, uint8_t* ready_out, ChainArgs ch) {
  static const char* const kEntryName[] = {"step", "run_table", "run_policy"};
  const launch_host::Selection sel = selection(h, entry);
  if (sel.why) return fail(h, SHIPSIM_EINVAL, "%s: %s", kEntryName[entry], sel.why);
  StepKernel kern = nullptr;
  for (const auto& row : kStepKernels)
    if (row.key == sel.key) kern = row.kern;
  if (!kern) return fail(h, SHIPSIM_EINVAL, "REGCHECK build");  // (every selection is a row: test_launch_host_cpu.py)
  DeviceGuard g(h->device);
  const int blocks = step_blocks(h, sel.lpe);
  if (sel.tail && tail_on(h, reinterpret_cast<const void*>(kern), blocks)) {
    (void)hipMemsetAsync(h->tail_ctr, 0, sizeof(int32_t), h->stream);
    ch.tail_ctr = h->tail_ctr;
    ch.tail_extra = h->tail_extra;
    ch.tail_waves = blocks;
  }
  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.P = h->P; a.S = h->S; a.K = h->K; a.T = h->T;
  a.action = action; a.active_mask = active; a.max_ticks = max_ticks;
  a.obs_out = obs_out; a.reward_out = reward_out; a.done_out = done_out; a.events_out = events_out;
  a.ticks_out = ticks_out; a.ready_out = ready_out; a.CH = ch;
  a.weather = h->wx_on ? h->wx_dev : nullptr;
  // the decision streams' slot -> env order, formed on the stream in front of the launch (no readback: the
  // collector replays both in a graph); with the switch off the buffer goes back to the identity once and the
  // kernel runs slot = env
  if (entry != launch_host::kStep && h->slot_env) {
    const int n = h->P.n_envs, ob = (n + kOrderThreads - 1) / kOrderThreads;
    if (grouping_host::groups(entry, n, h->group_on != 0)) {
      hipLaunchKernelGGL(stream_order_kernel, dim3(ob), dim3(kOrderThreads), 0, h->stream,
                         (const double*)h->S.f(SF_TIME), n, (int)h->P.n_ships, h->P.dt, h->slot_env);
      HIPCHK(h, hipGetLastError());
      h->slot_identity = 0;
      a.slot_env = h->slot_env;
    } else if (!h->slot_identity) {
      hipLaunchKernelGGL(stream_identity_kernel, dim3(ob), dim3(kOrderThreads), 0, h->stream, n, h->slot_env);
      HIPCHK(h, hipGetLastError());
      h->slot_identity = 1;
    }
  }
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return SHIPSIM_OK;
}

extern "C" {

int32_t shipsim_abi_version(void) { return SHIPSIM_ABI_VERSION; }

#ifdef SHIPSIM_PHASE_TIMING
// timing builds only (not part of the ABI): read and clear the per-phase cycle sums
int shipsim_debug_phase_cycles(unsigned long long* out8) {
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(diag::g_phase_cycles), sizeof(unsigned long long) * 8) != hipSuccess) return -2;
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(diag::g_phase_cycles), z, sizeof(z)) == hipSuccess ? 0 : -2;
}
#endif

#ifndef SHIPSIM_SRC_HASH
#define SHIPSIM_SRC_HASH "unknown"
#endif
const char* shipsim_build_info(void) {
  return "shipsim gfx950 HIP (fp64, lane-pair AST kernel, wave-cooperative SBMPC) src " SHIPSIM_SRC_HASH;
}

int shipsim_default_config(int32_t kind, int32_t machinery, int32_t collav, double time_step, shipsim_config* cfg) {
  return config_host::default_config(kind, machinery, collav, time_step, cfg);
}

// message of this thread's last failed shipsim_create (shipsim_last_error(NULL)); set on every failing path
static thread_local char g_create_err[512];

int shipsim_create(const shipsim_config* cfg_in, int32_t n_envs, int32_t n_obs_ships, int32_t device, void* stream,
                   shipsim_handle** out) {
  g_create_err[0] = 0;
  if (!cfg_in || !out || n_envs <= 0) {
    snprintf(g_create_err, sizeof(g_create_err), "shipsim_create: %s", !cfg_in ? "config is NULL" : !out ? "out is NULL"
             : "n_envs must be > 0");
    return SHIPSIM_EINVAL;
  }
  *out = nullptr;
  shipsim_handle* h = new (std::nothrow) shipsim_handle();
  if (!h) {
    snprintf(g_create_err, sizeof(g_create_err), "shipsim_create: out of host memory");
    return SHIPSIM_ENOMEM;
  }
  memset(h, 0, sizeof(*h));
  h->cfg = *cfg_in;
  if (n_obs_ships > 0 && h->cfg.kind == SHIPSIM_KIND_AST) h->cfg.n_ships = 1 + n_obs_ships;
  const shipsim_config* cfg = &h->cfg;
  if (config_host::validate(cfg, h->err, sizeof(h->err))) {
    snprintf(g_create_err, sizeof(g_create_err), "%s", h->err);
    delete h;
    return SHIPSIM_EINVAL;
  }
  *out = h;  // from here on a failure leaves the handle to the caller, with its message (shipsim_last_error)
  h->device = device;
  h->stream = (hipStream_t)stream;
  DeviceGuard g(device);
  h->lpe = launch_host::select(cfg->machinery, cfg->collav, cfg->n_ships, lanes_per_env(cfg, n_envs, device), false,
                               false, launch_host::kStep).lpe;
  h->lpe_uniform = h->lpe;
  // the host half (shipsim_config_host.hpp): parameters, per-ship constants, the constant block with the map grid
  config_host::params(cfg, n_envs, h->P);
  const int ns = cfg->n_ships;
  ShipConst sc[SHIPSIM_MAX_SHIPS];
  memset(sc, 0, sizeof(sc));
  for (int i = 0; i < ns; ++i) config_host::ship_const(&cfg->ship[i], &sc[i]);
  config_host::ConstBlock cb;
  if (!config_host::const_block(cfg, sc, cb))
    return fail(h, SHIPSIM_ENOMEM, "shipsim_create: out of host memory (constant block, %zu B)", cb.bytes);
  hipError_t e = hipMalloc(&h->const_block, cb.bytes);
  if (e != hipSuccess) {
    free(cb.host);
    return fail(h, SHIPSIM_EHIP, "hipMalloc(const): %s", hipGetErrorString(e));
  }
  e = hipMemcpy(h->const_block, cb.host, cb.bytes, hipMemcpyHostToDevice);
  free(cb.host);
  if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "hipMemcpy(const): %s", hipGetErrorString(e));
  const char* kb = (const char*)h->const_block;
  const size_t flag_off = cb.grid_off + (size_t)cb.gnx * cb.gny * sizeof(uint64_t);
  h->K.base = kb; h->K.n_edges = cb.n_edges; h->K.gnx = cb.gnx; h->K.gny = cb.gny;
  h->K.gx0 = cb.gx0; h->K.gy0 = cb.gy0; h->K.ginv = 1.0 / config_host::kGridCell;
  h->K.grid_mask = cb.use_grid ? (const uint64_t*)(kb + cb.grid_off) : nullptr;
  h->K.grid_flag = cb.use_grid ? (const uint8_t*)(kb + flag_off) : nullptr;
  h->K.grid_part = cb.use_grid ? (const uint64_t*)(kb + cb.part_off) : nullptr;

  // state block (DevState layout: ship arrays | routes | env arrays)
  const size_t S = (size_t)n_envs * ns;
  const state_host::Layout lay = state_host::layout(n_envs, ns);
  h->S.ship_stride = lay.ship_stride; h->S.route_stride = lay.route_stride;
  h->S.env_stride = lay.env_stride; h->S.env_off = lay.env_off;
  size_t bytes = (size_t)lay.bytes;
  e = hipMalloc(&h->dev_block, bytes);
  if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "hipMalloc(state %zu B): %s", bytes, hipGetErrorString(e));
  h->dev_bytes = bytes;
  h->S.base = (char*)h->dev_block;
  e = hipMalloc(&h->nonfinite_dev, sizeof(int32_t));
  if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "hipMalloc(counter): %s", hipGetErrorString(e));
  h->S.nonfinite = h->nonfinite_dev;
  (void)hipMemsetAsync(h->nonfinite_dev, 0, sizeof(int32_t), h->stream);
  e = hipMemsetAsync(h->dev_block, 0, bytes, h->stream);
  if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
  int threads = 256, blocks = (int)((S + threads - 1) / threads);
  hipLaunchKernelGGL(init_kernel, dim3(blocks), dim3(threads), 0, h->stream, h->P, h->S, h->K);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "init_kernel: %s", hipGetErrorString(e));
  // the decision streams' slot -> env permutation (AST handles of up to grouping_host::kMaxEnvs envs): the identity
  h->group_on = grouping_host::default_on(cfg->collav, cfg->n_ships) ? 1 : 0;
  if (const size_t len = cfg->kind == SHIPSIM_KIND_AST ? grouping_host::buffer_len(n_envs) : 0) {
    e = hipMalloc(&h->slot_env, len * sizeof(int32_t));
    if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "hipMalloc(stream order): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(stream_identity_kernel, dim3((n_envs + kOrderThreads - 1) / kOrderThreads), dim3(kOrderThreads),
                       0, h->stream, n_envs, h->slot_env);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, SHIPSIM_EHIP, "stream_identity_kernel: %s", hipGetErrorString(e));
    h->slot_identity = 1;
  }
  return SHIPSIM_OK;
}

int shipsim_destroy(shipsim_handle* h) {
  if (!h) return SHIPSIM_EINVAL;
  {
    DeviceGuard g(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    else (void)hipDeviceSynchronize();
    if (h->dev_block) (void)hipFree(h->dev_block);
    if (h->const_block) (void)hipFree(h->const_block);
    if (h->fuel_block) (void)hipFree(h->fuel_block);
    if (h->nonfinite_dev) (void)hipFree(h->nonfinite_dev);
    if (h->tail_ctr) (void)hipFree(h->tail_ctr);
    if (h->wx_dev) (void)hipFree(h->wx_dev);
    if (h->wx_stage) (void)hipFree(h->wx_stage);
    if (h->fork_block) (void)hipFree(h->fork_block);
    if (h->slot_env) (void)hipFree(h->slot_env);
  }
  free(h->wx_host);
  delete h;
  return SHIPSIM_OK;
}

const char* shipsim_last_error(const shipsim_handle* h) { return h ? h->err : g_create_err; }

int shipsim_set_stream(shipsim_handle* h, void* stream) {
  if (!h) return SHIPSIM_EINVAL;
  h->stream = (hipStream_t)stream;
  return SHIPSIM_OK;
}
int32_t shipsim_num_envs(const shipsim_handle* h) { return h ? h->P.n_envs : -1; }
int32_t shipsim_lanes_per_env(const shipsim_handle* h) { return h ? h->lpe : -1; }

int shipsim_reset(shipsim_handle* h, const uint8_t* env_mask, float* obs_out) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (h->P.kind < SHIPSIM_KIND_SINGLE || h->P.kind > SHIPSIM_KIND_AST)
    return fail(h, SHIPSIM_EINVAL, "reset: kind %d not supported on device", h->P.kind);
  DeviceGuard g(h->device);
  int S = h->P.n_envs * h->P.n_ships, threads = 256, blocks = (S + threads - 1) / threads;
  static const decltype(&reset_kernel<true, true>) kReset[2][2] = {  // [detailed machinery][recording]
      {reset_kernel<false, false>, reset_kernel<false, true>}, {reset_kernel<true, false>, reset_kernel<true, true>}};
  if (h->wx_on)  // (detailed machinery, no recording: shipsim_set_weather)
    hipLaunchKernelGGL(reset_wx_kernel, dim3(blocks), dim3(threads), 0, h->stream, h->P, h->S, h->K, env_mask, obs_out,
                       (const double*)h->wx_dev);
  else
    hipLaunchKernelGGL(kReset[h->P.machinery == SHIPSIM_MACH_DETAILED][h->T.ship != nullptr], dim3(blocks),
                       dim3(threads), 0, h->stream, h->P, h->S, h->K, h->T, env_mask, obs_out);
  HIPCHK(h, hipGetLastError());
  h->ever_reset = 1;
  return SHIPSIM_OK;
}

int shipsim_step(shipsim_handle* h, const float* action, const uint8_t* active, int32_t max_ticks, float* obs_out,
                 double* reward_out, uint8_t* done_out, uint32_t* events_out, int32_t* ticks_out,
                 uint8_t* ready_out) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (h->P.kind != SHIPSIM_KIND_AST) return fail(h, SHIPSIM_EINVAL, "step: only SHIPSIM_KIND_AST has decision steps");
  if (!action) return fail(h, SHIPSIM_EINVAL, "step: action is NULL");
  if (!h->ever_reset) return fail(h, SHIPSIM_ESTATE, "step before reset");
  return launch_ast(h, launch_host::kStep, action, active, max_ticks, obs_out, reward_out, done_out, events_out,
                    ticks_out, ready_out, ChainArgs{});
}

int shipsim_tick(shipsim_handle* h, int32_t k, uint32_t* events_out) {
  if (!h || !h->dev_block || k < 0) return SHIPSIM_EINVAL;
  if (h->P.kind != SHIPSIM_KIND_SINGLE && h->P.kind != SHIPSIM_KIND_NONIW)
    return fail(h, SHIPSIM_EINVAL, "tick: device raw ticks for SHIPSIM_KIND_SINGLE and SHIPSIM_KIND_NONIW");
  if (k == 0) return SHIPSIM_OK;
  DeviceGuard g(h->device);
  if (h->P.kind == SHIPSIM_KIND_NONIW) {  // two lanes per env
    if (h->P.machinery != SHIPSIM_MACH_SIMPLIFIED)
      return fail(h, SHIPSIM_EINVAL, "tick: KIND_NONIW runs the simplified machinery (run_colav SimpleShipModel)");
    const int blocks = (2 * h->P.n_envs + 63) / 64;
    static const decltype(&noniw_tick_kernel<0>) kNoniw[3] = {  // [collav]
        noniw_tick_kernel<SHIPSIM_COLLAV_NONE>, noniw_tick_kernel<SHIPSIM_COLLAV_SIMPLE>,
        noniw_tick_kernel<SHIPSIM_COLLAV_SBMPC>};
    hipLaunchKernelGGL(kNoniw[h->P.collav], dim3(blocks), dim3(64), 0, h->stream,
                       NoniwArgs{h->P, h->S, h->K, k, events_out});
    HIPCHK(h, hipGetLastError());
    return SHIPSIM_OK;
  }
  const int threads = 64, blocks = (h->P.n_envs + threads - 1) / threads;
  if (h->P.machinery == SHIPSIM_MACH_DETAILED)
    hipLaunchKernelGGL(single_tick_kernel<true>, dim3(blocks), dim3(threads), 0, h->stream, h->P, h->S, h->K, k);
  else if (diag::kC2OneWave)  // (comparison builds: the one-wave form)
    hipLaunchKernelGGL(single_tick_kernel<false>, dim3(blocks), dim3(threads), 0, h->stream, h->P, h->S, h->K, k);
  else
    shipsim_c2_pipe_launch(blocks, h->stream, h->P, h->S, h->K, k);
  HIPCHK(h, hipGetLastError());
  return SHIPSIM_OK;
}

}  // extern "C"

// the decision-stream launch shared by shipsim_run_table and shipsim_run_policy
static int run_chain(shipsim_handle* h, launch_host::Entry entry, const ChainArgs& ch, int32_t max_ticks,
                     int32_t* ticks_out) {
  return launch_ast(h, entry, nullptr, nullptr, max_ticks, nullptr, nullptr, nullptr, nullptr, ticks_out, nullptr, ch);
}

extern "C" {

int shipsim_run_table(shipsim_handle* h, const float* table, int32_t n_eps, int32_t n_dec, int32_t max_ticks,
                      int32_t* ep_idx, int32_t* dec_idx, int32_t* ticks_out, int32_t* decisions_out, double* log,
                      int32_t log_cap, int32_t* log_len) {
  if (!h || !h->dev_block || !table || !ep_idx || !dec_idx || n_eps < 1 || n_dec < 1 || max_ticks < 1 ||
      (log && (!log_len || log_cap < 1)))
    return SHIPSIM_EINVAL;
  if (h->P.kind != SHIPSIM_KIND_AST) return fail(h, SHIPSIM_EINVAL, "run_table: AST kind only");
  ChainArgs ch = {};
  ch.table = table; ch.n_eps = n_eps; ch.n_dec = n_dec; ch.ep_idx = ep_idx; ch.dec_idx = dec_idx;
  ch.decisions = decisions_out; ch.log = log; ch.log_len = log_len; ch.log_cap = log_cap;
  return run_chain(h, launch_host::kTable, ch, max_ticks, ticks_out);
}

int shipsim_run_policy(shipsim_handle* h, const float* policy, const float* w2t, int32_t obs_dim, int32_t hidden,
                       int32_t deterministic, uint64_t seed, const int64_t* counter, int32_t n_dec,
                       int32_t max_ticks, int32_t* ep_idx, int32_t* dec_idx, int32_t* ticks_out,
                       int32_t* decisions_out, double* log, int32_t log_cap, int32_t* log_len) {
  if (!h || !h->dev_block || !policy || !w2t || !ep_idx || !dec_idx || n_dec < 1 || max_ticks < 1 ||
      (log && (!log_len || log_cap < 1)) || (!deterministic && !counter))
    return SHIPSIM_EINVAL;
  if (h->P.kind != SHIPSIM_KIND_AST) return fail(h, SHIPSIM_EINVAL, "run_policy: AST kind only");
  if (const char* why = selection(h, launch_host::kPolicy).why)  // (before the policy's shape, as ever)
    return fail(h, SHIPSIM_EINVAL, "run_policy: %s", why);
  if (obs_dim != 8) return fail(h, SHIPSIM_EINVAL, "run_policy: observation dim %d (the AST observation has 8)", obs_dim);
  if (hidden < 64 || hidden > kPolMaxHidden || hidden % 64)
    return fail(h, SHIPSIM_EINVAL, "run_policy: hidden %d (a multiple of 64 up to 512)", hidden);
  ChainArgs ch = {};
  ch.n_eps = 1; ch.n_dec = n_dec; ch.ep_idx = ep_idx; ch.dec_idx = dec_idx;
  ch.decisions = decisions_out; ch.log = log; ch.log_len = log_len; ch.log_cap = log_cap;
  ch.log_stop = log ? 1 : 0;
  ch.policy = policy; ch.w2t = w2t; ch.pol_obs = obs_dim; ch.pol_hidden = hidden; ch.pol_det = deterministic ? 1 : 0;
  ch.pol_seed = seed; ch.pol_counter = counter;
  return run_chain(h, launch_host::kPolicy, ch, max_ticks, ticks_out);
}

int shipsim_set_stream_tail(shipsim_handle* h, int32_t extra_ticks) {
  if (!h || extra_ticks < 0) return SHIPSIM_EINVAL;
  if (extra_ticks > 0 && !h->tail_ctr) {
    DeviceGuard g(h->device);
    HIPCHK(h, hipMalloc(&h->tail_ctr, sizeof(int32_t)));
  }
  h->tail_extra = extra_ticks;
  return SHIPSIM_OK;
}

int shipsim_set_stream_grouping(shipsim_handle* h, int32_t on) {
  if (!h) return SHIPSIM_EINVAL;
  h->group_on = on != 0;
  return SHIPSIM_OK;
}

int shipsim_get_stream_grouping(shipsim_handle* h, int32_t* slot_env_out) {
  if (!h || !h->dev_block || !slot_env_out) return SHIPSIM_EINVAL;
  if (!h->slot_env)
    return fail(h, SHIPSIM_EINVAL, "get_stream_grouping: AST handles of up to %d envs hold a stream order",
                (int)grouping_host::kMaxEnvs);
  DeviceGuard g(h->device);
  HIPCHK(h, hipMemcpyAsync(slot_env_out, h->slot_env, (size_t)h->P.n_envs * sizeof(int32_t), hipMemcpyDefault,
                           h->stream));
  return SHIPSIM_OK;
}

int shipsim_legacy_step(shipsim_handle* h, int32_t k, double* states_out, uint8_t* done_out, uint32_t* status_out) {
  if (!h || !h->dev_block || k < 0) return SHIPSIM_EINVAL;
  if (h->P.kind != SHIPSIM_KIND_AST) return fail(h, SHIPSIM_EINVAL, "legacy_step: AST kind only");
  if (h->P.n_ships != 2) return fail(h, SHIPSIM_EINVAL, "legacy_step: the legacy MultiShipEnv has one obstacle ship");
  if (h->wx_on) return fail(h, SHIPSIM_EINVAL, "legacy_step: per-env weather is set (the legacy kernels run the config's)");
  if (k == 0) return SHIPSIM_OK;
  DeviceGuard g(h->device);
  const int threads = 64, blocks = (2 * h->P.n_envs + threads - 1) / threads;
  const LegacyArgs la{h->P, h->S, h->K, k, states_out, done_out, status_out};
#ifdef SHIPSIM_REGCHECK  // (register-usage inspection builds hold no legacy kernels)
  return fail(h, SHIPSIM_EINVAL, "REGCHECK build");
#else
#define LEGACY(D) {legacy_step_kernel<D, 0>, legacy_step_kernel<D, 1>, legacy_step_kernel<D, 2>}
  static const decltype(&legacy_step_kernel<true, 0>) kLegacy[2][3] = {LEGACY(false), LEGACY(true)};  // [detailed][collav]
#undef LEGACY
  hipLaunchKernelGGL(kLegacy[h->P.machinery == SHIPSIM_MACH_DETAILED][h->P.collav], dim3(blocks), dim3(threads), 0,
                     h->stream, la);
  HIPCHK(h, hipGetLastError());
#endif
  return SHIPSIM_OK;
}

static int field_ptr(shipsim_handle* h, int32_t field, void** p, size_t* bytes) {
  const size_t S = (size_t)h->P.n_envs * h->P.n_ships, N = (size_t)h->P.n_envs;
  if (field >= 0 && field < SHIPSIM_N_SHIP_FIELDS) {
    if (field == SHIPSIM_F_NEXT_WPT) { *p = h->S.next_wpt(); *bytes = S * 4; return 0; }
    if (field == SHIPSIM_F_STOP) { *p = h->S.stop(); *bytes = S * 4; return 0; }
    *p = h->S.f(field); *bytes = S * 8;
    return 0;
  }
  switch (field) {
    case SHIPSIM_E_SAMPLING_COUNT: *p = h->S.sampling_count(); *bytes = N * 4; return 0;
    case SHIPSIM_E_TRAVEL_DIST: *p = h->S.travel_dist(); *bytes = N * 8; return 0;
    case SHIPSIM_E_TRAVEL_TIME: *p = h->S.travel_time(); *bytes = N * 8; return 0;
    case SHIPSIM_E_ACC_REWARD: *p = h->S.acc(); *bytes = N * 8; return 0;
    case SHIPSIM_E_N_BASE: *p = h->S.n_base(); *bytes = N * 8; return 0;
    case SHIPSIM_E_E_BASE: *p = h->S.e_base(); *bytes = N * 8; return 0;
    case SHIPSIM_E_SBMPC_P_LAST: *p = h->S.p_last(); *bytes = N * 8; return 0;
    case SHIPSIM_E_SBMPC_CHI_LAST: *p = h->S.chi_last(); *bytes = N * 8; return 0;
    case SHIPSIM_E_ROUTE_LEN: *p = h->S.n_route(); *bytes = S * 4; return 0;
    case SHIPSIM_E_ROUTE_NORTH: *p = h->S.route_n(); *bytes = S * kMaxRoute * 8; return 0;
    case SHIPSIM_E_ROUTE_EAST: *p = h->S.route_e(); *bytes = S * kMaxRoute * 8; return 0;
  }
  return 1;
}

int shipsim_get_state(shipsim_handle* h, int32_t field, void* dst) {
  if (!h || !dst) return SHIPSIM_EINVAL;
  void* p;
  size_t b;
  if (field_ptr(h, field, &p, &b)) return fail(h, SHIPSIM_EINVAL, "unknown field %d", field);
  DeviceGuard g(h->device);
  HIPCHK(h, hipMemcpyAsync(dst, p, b, hipMemcpyDefault, h->stream));
  return SHIPSIM_OK;
}

int shipsim_set_state(shipsim_handle* h, int32_t field, const void* src) {
  if (!h || !src) return SHIPSIM_EINVAL;
  void* p;
  size_t b;
  if (field_ptr(h, field, &p, &b)) return fail(h, SHIPSIM_EINVAL, "unknown field %d", field);
  DeviceGuard g(h->device);
  HIPCHK(h, hipMemcpyAsync(p, src, b, hipMemcpyDefault, h->stream));
  return SHIPSIM_OK;
}

// ---- snapshot / restore / fork: the whole state block (shipsim_state_host.hpp) ----
int64_t shipsim_state_bytes(const shipsim_handle* h) { return h && h->dev_block ? (int64_t)h->dev_bytes : SHIPSIM_EINVAL; }

// what the three calls refuse alike: NULL buffer (where one is required), another size, a recording handle
static int state_call_check(shipsim_handle* h, const char* what, const void* buf, bool need_buf, int64_t bytes) {
  if (need_buf && !buf) return fail(h, SHIPSIM_EINVAL, "%s: the buffer is NULL", what);
  if (bytes != (int64_t)h->dev_bytes)
    return fail(h, SHIPSIM_EINVAL, "%s: %lld bytes, the state of this handle has %lld (shipsim_state_bytes)", what,
                (long long)bytes, (long long)h->dev_bytes);
  if (h->T.ship)
    return fail(h, SHIPSIM_EINVAL, "%s: trajectory recording is on (rows, lengths and fuel are not part of a snapshot)",
                what);
  return SHIPSIM_OK;
}

int shipsim_snapshot(shipsim_handle* h, void* dst, int64_t bytes) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (int rc = state_call_check(h, "snapshot", dst, true, bytes)) return rc;
  if (!h->ever_reset) return fail(h, SHIPSIM_ESTATE, "snapshot before reset");
  DeviceGuard g(h->device);
  HIPCHK(h, hipMemcpyAsync(dst, h->dev_block, h->dev_bytes, hipMemcpyDeviceToDevice, h->stream));
  return SHIPSIM_OK;
}

int shipsim_restore(shipsim_handle* h, const void* src, int64_t bytes) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (int rc = state_call_check(h, "restore", src, true, bytes)) return rc;
  DeviceGuard g(h->device);
  HIPCHK(h, hipMemcpyAsync(h->dev_block, src, h->dev_bytes, hipMemcpyDeviceToDevice, h->stream));
  h->ever_reset = 1;
  return SHIPSIM_OK;
}

constexpr int64_t kForkMaxUnits = (int64_t)1 << 31;  // fork_gather_kernel counts a column's units in 32 bits
constexpr int64_t kForkMaxBlocks = 1024;             // blocks per column (they stride over its units)

int shipsim_fork(shipsim_handle* h, const void* from, int64_t bytes, const int32_t* src_env) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (int rc = state_call_check(h, "fork", from, false, bytes)) return rc;
  if (from && ((uintptr_t)from & 15)) return fail(h, SHIPSIM_EINVAL, "fork: the snapshot is not 16-byte aligned");
  if (!from && !h->ever_reset) return fail(h, SHIPSIM_ESTATE, "fork from the live state before reset");
  if (!src_env) {  // identity: a restore, or nothing
    if (!from) return SHIPSIM_OK;
    return shipsim_restore(h, from, bytes);
  }
  const state_host::Layout lay = {h->S.ship_stride, h->S.route_stride, h->S.env_stride, h->S.env_off,
                                  (int64_t)h->dev_bytes};
  const state_host::Table tab = state_host::table(lay, h->P.n_ships);
  const int64_t units = state_host::max_units(tab, h->P.n_envs);
  if (units > kForkMaxUnits) return fail(h, SHIPSIM_EINVAL, "fork: %d envs are more than the gather counts", h->P.n_envs);
  DeviceGuard g(h->device);
  if (!from && !h->fork_block) {
    // zeroed once, so that the padding between the arrays, which the gather leaves alone, goes back as it is in
    // the state block (zero since shipsim_create). The memset is ordered on the stream of this first fork only, as
    // are this fork's gather and copy back behind it: after a shipsim_set_stream the staging block is ordered
    // against the new stream the way the state block itself is, by the caller's ordering of the two streams.
    // (Sizing: every grid row below gets the block count of the widest column, the routes; the blocks a narrower
    // column does not need find t >= total and exit. Per-column counts and a reciprocal for the per-unit divide are
    // what to do next should the gather's cost over a plain copy of the block ever matter: DESIGN.md §9.)
    hipError_t e = hipMalloc(&h->fork_block, h->dev_bytes);
    if (e != hipSuccess) {
      h->fork_block = nullptr;
      return fail(h, e == hipErrorOutOfMemory ? SHIPSIM_ENOMEM : SHIPSIM_EHIP, "hipMalloc(fork staging %zu B): %s",
                  h->dev_bytes, hipGetErrorString(e));
    }
    e = hipMemsetAsync(h->fork_block, 0, h->dev_bytes, h->stream);
    if (e != hipSuccess) {
      (void)hipFree(h->fork_block);
      h->fork_block = nullptr;
      return fail(h, SHIPSIM_EHIP, "hipMemsetAsync(fork staging): %s", hipGetErrorString(e));
    }
  }
  int64_t blocks = (units + 255) / 256;
  if (blocks > kForkMaxBlocks) blocks = kForkMaxBlocks;
  const char* src = from ? (const char*)from : (const char*)h->dev_block;
  char* dst = from ? (char*)h->dev_block : (char*)h->fork_block;
  hipLaunchKernelGGL(fork_gather_kernel, dim3((unsigned)blocks, state_host::kColumns), dim3(256), 0, h->stream, tab,
                     src, dst, src_env, (uint32_t)h->P.n_envs, from ? 0 : 1);
  HIPCHK(h, hipGetLastError());
  if (!from) HIPCHK(h, hipMemcpyAsync(h->dev_block, h->fork_block, h->dev_bytes, hipMemcpyDeviceToDevice, h->stream));
  h->ever_reset = 1;
  return SHIPSIM_OK;
}

// the splitting level of shipsim_resample's callers (the kernel is shipsim_resample.hip's)
int shipsim_level_distance(shipsim_handle* h, double* out) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (!out) return fail(h, SHIPSIM_EINVAL, "level_distance: the output is NULL");
  if (h->P.kind != SHIPSIM_KIND_AST && h->P.kind != SHIPSIM_KIND_NONIW)
    return fail(h, SHIPSIM_EINVAL, "level_distance: a single-ship handle has no obstacle ship to measure to");
  if (!h->ever_reset) return fail(h, SHIPSIM_ESTATE, "level_distance before reset");
  DeviceGuard g(h->device);
  shipsim_level_distance_launch(h->stream, h->S, h->P.n_envs, h->P.n_ships, out);
  HIPCHK(h, hipGetLastError());
  return SHIPSIM_OK;
}

// ---- the state archive: the state block of n_cells envs in the caller's memory (the kernel is shipsim_archive.hip's,
// the checks and the arithmetic shipsim_archive_host.hpp's) ----
int64_t shipsim_archive_bytes(const shipsim_handle* h, int32_t n_cells) {
  if (!h || !h->dev_block || n_cells < 1 || n_cells > archive_host::kMaxCells) return SHIPSIM_EINVAL;
  return archive_host::archive_bytes(n_cells, h->P.n_ships);
}

// what store and load refuse alike; on success the two tables: the live block's and the archive's
static int archive_call_check(shipsim_handle* h, const char* what, const void* archive, int64_t bytes, int32_t n_cells,
                              const void* index, const char* index_name, state_host::Table* live,
                              state_host::Table* arch) {
  switch (archive_host::check_args(archive, index, bytes, n_cells, h->P.n_ships)) {
    case archive_host::kArgOk: break;
    case archive_host::kArgNullArchive: return fail(h, SHIPSIM_EINVAL, "%s: the archive is NULL", what);
    case archive_host::kArgNullIndex: return fail(h, SHIPSIM_EINVAL, "%s: %s is NULL", what, index_name);
    case archive_host::kArgCells:
      return fail(h, SHIPSIM_EINVAL, "%s: n_cells = %d, not in 1..%d (SHIPSIM_ARCHIVE_MAX_CELLS)", what, n_cells,
                  archive_host::kMaxCells);
    case archive_host::kArgBytes:
      return fail(h, SHIPSIM_EINVAL, "%s: %lld bytes, an archive of %d cells of this handle has %lld "
                  "(shipsim_archive_bytes)", what, (long long)bytes, n_cells,
                  (long long)archive_host::archive_bytes(n_cells, h->P.n_ships));
    case archive_host::kArgAlign: return fail(h, SHIPSIM_EINVAL, "%s: the archive is not 16-byte aligned", what);
  }
  if (h->T.ship)
    return fail(h, SHIPSIM_EINVAL, "%s: trajectory recording is on (rows, lengths and fuel are not part of a snapshot)",
                what);
  const state_host::Layout lay = {h->S.ship_stride, h->S.route_stride, h->S.env_stride, h->S.env_off,
                                  (int64_t)h->dev_bytes};
  *live = state_host::table(lay, h->P.n_ships);
  *arch = state_host::table(state_host::layout(n_cells, h->P.n_ships), h->P.n_ships);
  const int64_t most = h->P.n_envs > n_cells ? h->P.n_envs : n_cells;
  if (state_host::max_units(*live, most) > archive_host::kMaxUnits)
    return fail(h, SHIPSIM_EINVAL, "%s: %lld slots are more than the gather counts", what, (long long)most);
  return SHIPSIM_OK;
}

int shipsim_archive_store(shipsim_handle* h, void* archive, int64_t bytes, int32_t n_cells, const int32_t* env_of_cell) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  state_host::Table live, arch;
  if (int rc = archive_call_check(h, "archive_store", archive, bytes, n_cells, env_of_cell, "env_of_cell", &live, &arch))
    return rc;
  if (!h->ever_reset) return fail(h, SHIPSIM_ESTATE, "archive_store before reset");
  DeviceGuard g(h->device);
  shipsim_archive_gather_launch(h->stream, live, arch, h->dev_block, archive, env_of_cell, n_cells, h->P.n_envs);
  HIPCHK(h, hipGetLastError());
  return SHIPSIM_OK;
}

int shipsim_archive_load(shipsim_handle* h, const void* archive, int64_t bytes, int32_t n_cells,
                         const int32_t* cell_of_env) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  state_host::Table live, arch;
  if (int rc = archive_call_check(h, "archive_load", archive, bytes, n_cells, cell_of_env, "cell_of_env", &live, &arch))
    return rc;
  DeviceGuard g(h->device);
  shipsim_archive_gather_launch(h->stream, arch, live, archive, h->dev_block, cell_of_env, h->P.n_envs, n_cells);
  HIPCHK(h, hipGetLastError());
  h->ever_reset = 1;
  return SHIPSIM_OK;
}

int shipsim_set_trajectory(shipsim_handle* h, double* ship_rows, double* env_rows, int32_t capacity,
                           int32_t* lengths) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (h->P.kind != SHIPSIM_KIND_AST) return fail(h, SHIPSIM_EINVAL, "set_trajectory: SHIPSIM_KIND_AST only");
  if (h->P.n_ships != 2 && ship_rows) return fail(h, SHIPSIM_EINVAL, "set_trajectory: one obstacle ship only");
  if (!ship_rows) {
    memset(&h->T, 0, sizeof(h->T));
    return SHIPSIM_OK;
  }
  if (h->wx_on)
    return fail(h, SHIPSIM_EINVAL, "set_trajectory: per-env weather is set (the recording kernels run the config's "
                "weather: replay the env on a uniform handle)");
  if (capacity <= 0 || !lengths) return fail(h, SHIPSIM_EINVAL, "set_trajectory: capacity %d / lengths", capacity);
  DeviceGuard g(h->device);
  const size_t fb = (size_t)h->P.n_envs * h->P.n_ships * 3 * sizeof(double);
  if (!h->fuel_block) HIPCHK(h, hipMalloc(&h->fuel_block, fb));
  HIPCHK(h, hipMemsetAsync(h->fuel_block, 0, fb, h->stream));
  HIPCHK(h, hipMemsetAsync(lengths, 0, (size_t)h->P.n_envs * sizeof(int32_t), h->stream));
  h->T.ship = ship_rows;
  h->T.env = env_rows;
  h->T.fuel = (double*)h->fuel_block;
  h->T.len = lengths;
  h->T.cap = capacity;
  return SHIPSIM_OK;
}

int shipsim_set_weather(shipsim_handle* h, const double* wind_speed, const double* wind_direction,
                        const double* current_from_north, const double* current_from_east) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  const int n_null = !wind_speed + !wind_direction + !current_from_north + !current_from_east;
  if (n_null == 4) {  // back to the config's uniform weather and the uniform kernels
    h->wx_on = 0;
    h->lpe = h->lpe_uniform;
    return SHIPSIM_OK;
  }
  if (n_null) return fail(h, SHIPSIM_EINVAL, "set_weather: %d of the four arrays are NULL (all or none)", n_null);
  const char* why = weather_host::unsupported(h->P.kind, h->P.machinery, h->P.collav, h->T.ship != nullptr, h->P.n_ships);
  if (why) return fail(h, SHIPSIM_EINVAL, "set_weather: %s", why);
  const size_t n = (size_t)h->P.n_envs;
  const int64_t bad = weather_host::check(wind_speed, wind_direction, current_from_north, current_from_east, n);
  if (bad >= 0)
    return fail(h, SHIPSIM_EINVAL, "set_weather: env %lld: wind speed %g, wind direction %g, current (%g, %g) "
                "(finite values and a wind speed >= 0)", (long long)bad, wind_speed[bad], wind_direction[bad],
                current_from_north[bad], current_from_east[bad]);
  const size_t table_bytes = (size_t)weather_host::store_bytes((int64_t)n);
  double* dev_rows = (double*)malloc(table_bytes);
  double* host = h->wx_host ? h->wx_host : (double*)malloc(sizeof(double) * 4 * n);
  if (!dev_rows || !host) {
    free(dev_rows);
    if (!h->wx_host) free(host);
    return fail(h, SHIPSIM_ENOMEM, "set_weather: out of host memory");
  }
  DeviceGuard g(h->device);
  if (!h->wx_dev) {  // the table and shipsim_weather_fork's staging table: nothing allocates after this
    hipError_t e = hipMalloc(&h->wx_dev, table_bytes);
    if (e == hipSuccess) {
      e = hipMalloc(&h->wx_stage, table_bytes);
      if (e != hipSuccess) (void)hipFree(h->wx_dev);
    }
    if (e != hipSuccess) {
      free(dev_rows);
      if (!h->wx_host) free(host);
      h->wx_dev = h->wx_stage = nullptr;
      return fail(h, SHIPSIM_EHIP, "hipMalloc(weather): %s", hipGetErrorString(e));
    }
  }
  h->wx_host = host;
  weather_host::store_rows(wind_speed, wind_direction, current_from_north, current_from_east, n, dev_rows);
  // the upload is ordered on the handle's stream behind the launches already queued, and complete on return
  // (the staging rows are freed here): a change takes effect at the next launch
  hipError_t e = hipMemcpyAsync(h->wx_dev, dev_rows, table_bytes, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  free(dev_rows);
  if (e != hipSuccess) {  // the device array is in an unknown state: the handle runs the config's weather
    h->wx_on = 0;
    h->lpe = h->lpe_uniform;
    return fail(h, SHIPSIM_EHIP, "set_weather upload: %s", hipGetErrorString(e));
  }
  memcpy(host, wind_speed, sizeof(double) * n);
  memcpy(host + n, wind_direction, sizeof(double) * n);
  memcpy(host + 2 * n, current_from_north, sizeof(double) * n);
  memcpy(host + 3 * n, current_from_east, sizeof(double) * n);
  h->wx_on = 1;
  h->lpe = selection(h, launch_host::kStep).lpe;
  return SHIPSIM_OK;
}

int shipsim_get_weather(shipsim_handle* h, double* wind_speed, double* wind_direction, double* current_from_north,
                        double* current_from_east) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (!wind_speed || !wind_direction || !current_from_north || !current_from_east)
    return fail(h, SHIPSIM_EINVAL, "get_weather: an output array is NULL");
  const size_t n = (size_t)h->P.n_envs;
  double* out[4] = {wind_speed, wind_direction, current_from_north, current_from_east};
  const double uniform[4] = {h->cfg.wind_speed, h->cfg.wind_direction, h->cfg.current_velocity_component_from_north,
                             h->cfg.current_velocity_component_from_east};
  if (h->wx_on && h->wx_moved) {
    // weather has moved on the device, maybe by a graph replay that made no host call: the table is the record.
    // Wait for what is queued, then read the four rows the caller set (the direction from its own row).
    static const int row_of[4] = {weather_host::kWindSpeed, weather_host::kDirection, weather_host::kCurrentN,
                                  weather_host::kCurrentE};
    DeviceGuard g(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 4; ++k)
      HIPCHK(h, hipMemcpy(out[k], h->wx_dev + (size_t)row_of[k] * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    return SHIPSIM_OK;
  }
  for (int k = 0; k < 4; ++k)
    for (size_t i = 0; i < n; ++i) out[k][i] = h->wx_on ? h->wx_host[k * n + i] : uniform[k];
  return SHIPSIM_OK;
}

// ---- weather that moves with the state: the handle's table gathered by index (the kernel is shipsim_weather.hip's,
// the sizes and the refusals shipsim_weather_host.hpp's) ----
int64_t shipsim_weather_bytes(int32_t n_slots) {
  return weather_host::slots_ok(n_slots) ? weather_host::store_bytes(n_slots) : SHIPSIM_EINVAL;
}

int shipsim_weather_store(shipsim_handle* h, void* wx, int64_t bytes, int32_t n_slots, const int32_t* env_of_slot) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (const char* why = weather_host::carry_refusal(h->wx_on, wx, bytes, n_slots, h->P.n_envs, env_of_slot))
    return fail(h, SHIPSIM_EINVAL, "weather_store: %s", why);
  DeviceGuard g(h->device);
  h->wx_moved = 1;
  if (!env_of_slot) {  // a weather snapshot
    HIPCHK(h, hipMemcpyAsync(wx, h->wx_dev, (size_t)bytes, hipMemcpyDeviceToDevice, h->stream));
    return SHIPSIM_OK;
  }
  shipsim_weather_gather_launch(h->stream, h->wx_dev, (double*)wx, env_of_slot, n_slots, h->P.n_envs, false);
  HIPCHK(h, hipGetLastError());
  return SHIPSIM_OK;
}

int shipsim_weather_load(shipsim_handle* h, const void* wx, int64_t bytes, int32_t n_slots, const int32_t* slot_of_env) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (const char* why = weather_host::carry_refusal(h->wx_on, wx, bytes, n_slots, h->P.n_envs, slot_of_env))
    return fail(h, SHIPSIM_EINVAL, "weather_load: %s", why);
  DeviceGuard g(h->device);
  h->wx_moved = 1;
  if (!slot_of_env) {  // a restore
    HIPCHK(h, hipMemcpyAsync(h->wx_dev, wx, (size_t)bytes, hipMemcpyDeviceToDevice, h->stream));
    return SHIPSIM_OK;
  }
  shipsim_weather_gather_launch(h->stream, (const double*)wx, h->wx_dev, slot_of_env, h->P.n_envs, n_slots, false);
  HIPCHK(h, hipGetLastError());
  return SHIPSIM_OK;
}

int shipsim_weather_fork(shipsim_handle* h, const int32_t* src_env) {
  if (!h || !h->dev_block) return SHIPSIM_EINVAL;
  if (const char* why = weather_host::fork_refusal(h->wx_on)) return fail(h, SHIPSIM_EINVAL, "weather_fork: %s", why);
  if (!src_env) return SHIPSIM_OK;  // the identity: nothing moves
  DeviceGuard g(h->device);
  h->wx_moved = 1;
  // gathered into the staging table and copied back, as shipsim_fork does with the state: the table never moves
  shipsim_weather_gather_launch(h->stream, h->wx_dev, h->wx_stage, src_env, h->P.n_envs, h->P.n_envs, true);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(h->wx_dev, h->wx_stage, (size_t)weather_host::store_bytes(h->P.n_envs),
                           hipMemcpyDeviceToDevice, h->stream));
  return SHIPSIM_OK;
}

int shipsim_sbmpc_eval(int32_t n, double tf, double dt, const double* in, double* out, void* stream) {
  if (n < 0 || (n > 0 && (!in || !out)) || !(dt > 0) || tf / dt > 4096) return SHIPSIM_EINVAL;
  if (n == 0) return SHIPSIM_OK;
  hipLaunchKernelGGL(sbmpc_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, tf, dt, in, out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_sbmpc_nominal(int32_t n, double tf, double dt, const double* in, int32_t* flag_out, void* stream) {
  if (n < 0 || (n > 0 && (!in || !flag_out)) || !(dt > 0) || tf / dt > 4096) return SHIPSIM_EINVAL;
  if (n == 0) return SHIPSIM_OK;
  hipLaunchKernelGGL(sbmpc_nominal_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, n, tf, dt, in,
                     flag_out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_tickmath_eval(int32_t fn, int32_t n, const double* in, double* out, void* stream) {
  if (fn < 0 || fn > 2 || n < 0 || (n > 0 && (!in || !out))) return SHIPSIM_EINVAL;
  if (n == 0) return SHIPSIM_OK;
  hipLaunchKernelGGL(tickmath_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, fn, n, in, out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_sbmpc_eval_multi(int32_t n, int32_t n_obs, double tf, double dt, const double* in, double* out,
                             void* stream) {
  if (n < 0 || n_obs < 1 || n_obs > SHIPSIM_MAX_OBS || (n > 0 && (!in || !out)) || !(dt > 0) || tf / dt > 4096)
    return SHIPSIM_EINVAL;
  if (n == 0) return SHIPSIM_OK;
  // The service mirrors the env kernels of the same K: the optimiser instantiation (NOB) of the step kernel an env
  // of 1 + n_obs ships runs, by the step kernels' own expressions (launch_host::ship_slots, sbmpc_nob). Those are
  // the 4-slot kernels' (K = 2, 3) and the 8-slot kernels' (K = 4); K = 1, whose env kernels run the
  // single-obstacle optimiser, is served by the 4-slot instantiation.
  constexpr int kNob4 = launch_host::sbmpc_nob(4), kNob8 = launch_host::sbmpc_nob(8);
  static_assert(kNob4 < kNob8 && kNob8 == SHIPSIM_MAX_OBS, "every n_obs <= SHIPSIM_MAX_OBS has an instantiation");
  const bool wide = launch_host::sbmpc_nob(launch_host::ship_slots(1 + n_obs)) > kNob4;
  const dim3 grid((n + 63) / 64), block(64);
  const int n_samp = (int)(tf / dt);
  if (wide)
    hipLaunchKernelGGL(sbmpc_multi_eval_kernel<kNob8>, grid, block, 0, (hipStream_t)stream, n, n_obs, n_samp, dt, in,
                       out);
  else
    hipLaunchKernelGGL(sbmpc_multi_eval_kernel<kNob4>, grid, block, 0, (hipStream_t)stream, n, n_obs, n_samp, dt, in,
                       out);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_div_check(int32_t n, const double* num, const double* den, double* fast, double* ref, void* stream) {
  if (n < 0 || (n > 0 && (!num || !den || !fast || !ref))) return SHIPSIM_EINVAL;
  if (n == 0) return SHIPSIM_OK;
  hipLaunchKernelGGL(div_check_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, num, den, fast,
                     ref);
  return hipGetLastError() == hipSuccess ? SHIPSIM_OK : SHIPSIM_EHIP;
}

int shipsim_synchronize(shipsim_handle* h) {
  if (!h) return SHIPSIM_EINVAL;
  DeviceGuard g(h->device);
  if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
  else HIPCHK(h, hipDeviceSynchronize());
  if (h->nonfinite_dev) {
    int32_t n = 0;
    HIPCHK(h, hipMemcpy(&n, h->nonfinite_dev, sizeof(n), hipMemcpyDeviceToHost));
    if (n > h->nonfinite_seen) {
      const int32_t fresh = n - h->nonfinite_seen;
      h->nonfinite_seen = n;
      return fail(h, SHIPSIM_ENONFINITE,
                  "%d env decision(s) ended on a non-finite ship state since the last synchronize (%d in all): "
                  "flagged SHIPSIM_EV_NONFINITE, done", fresh, n);
    }
  }
  return SHIPSIM_OK;
}

int32_t shipsim_nonfinite_count(const shipsim_handle* h) { return h ? h->nonfinite_seen : -1; }

int shipsim_diag_lane_faults(uint32_t* out32) {
  if (!out32) return SHIPSIM_EINVAL;
  for (int i = 0; i < 32; ++i) out32[i] = 0;
#ifdef SHIPSIM_LANECHECK
  if (hipDeviceSynchronize() != hipSuccess) return SHIPSIM_EHIP;
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(diag::g_lane_diag), 32 * sizeof(uint32_t)) != hipSuccess) return SHIPSIM_EHIP;
  const uint32_t zero[32] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(diag::g_lane_diag), zero, sizeof(zero)) != hipSuccess) return SHIPSIM_EHIP;
  return SHIPSIM_OK;
#elif defined(SHIPSIM_SB_STATS)
  if (hipDeviceSynchronize() != hipSuccess) return SHIPSIM_EHIP;
  // counters 0..7 in out32[16..31] (as before), the later ones from out32[0] on
  uint64_t v[diag::kSbStats];
  static_assert(diag::kSbStats >= 8 && diag::kSbStats <= 16, "the read-out's 32 words");
  if (hipMemcpyFromSymbol(v, HIP_SYMBOL(diag::g_sb_stats), sizeof(v)) != hipSuccess) return SHIPSIM_EHIP;
  memcpy(out32 + 16, v, 8 * sizeof(uint64_t));
  memcpy(out32, v + 8, (diag::kSbStats - 8) * sizeof(uint64_t));
  const uint64_t zero[diag::kSbStats] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(diag::g_sb_stats), zero, sizeof(zero)) != hipSuccess) return SHIPSIM_EHIP;
  return SHIPSIM_OK;
#else
  return SHIPSIM_EINVAL;  // not a diagnostics build
#endif
}

}  // extern "C"