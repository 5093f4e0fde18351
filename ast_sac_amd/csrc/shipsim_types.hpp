// shipsim_types.hpp — the simulator's constant data as both sides see it: the per-ship constants, the launch
// parameters, the map's edges and boxes with the point-in-polygon test, and the layout of the constant block.
// Plain C++17 with no HIP include: the host's configuration half (shipsim_config_host.hpp) and its stand-alone check
// (tests/config_host_check.cpp) compile it with the host compiler; shipsim_device.hpp includes it for the kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "shipsim.h"

// the functions both sides run: host and device, always inlined, under hipcc; plain inline functions without it
#ifdef __HIPCC__
#define SHIPSIM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SHIPSIM_HD inline
#endif

namespace shipsim {

constexpr double kPi = 3.141592653589793;
constexpr int kMaxRoute = SHIPSIM_MAX_ROUTE;

// ---------------------------------------------------------------------------------------------
// constants (computed once on the host, identical arithmetic to the reference constructors)
// ---------------------------------------------------------------------------------------------
struct ShipConst {
  // BaseShipModel.__init__ (ship_model.py:412-474)
  double mass, i_z, x_du, y_dv, n_dr;
  double inv_m0, inv_m1, inv_m2;    // inv(mass_matrix()) diagonal (x_g = 0)
  double dlin0, dlin1, dlin2;       // linear_damping_matrix diagonal: mass/t_surge, mass/t_sway, i_z/t_yaw
  double ku, kv, kr;
  double l_ship, w_ship, obs_l_cfg, obs_w_cfg;  // ship_config.length/width (SBMPC do_list)
  double rho_a, proj_area_f, proj_area_l, cx, cy, cn;
  double c_rudder_v, c_rudder_r, max_rudder;
  // ShipMachineryModel (ship_engine.py:341-443) with the active MachineryMode
  double avail_me, avail_el, cap_me, cap_el;   // available powers; torque caps avail/5*pi/30
  double d_me, d_hsg, r_me, r_hsg, jp, kp_prop, thrust_coeff, shaft_speed_max;
  double init_omega;
  // MachineryMode.distribute_load / BaseMachineryModel.fuel_consumption (ship_engine.py:46-76, 259-295):
  // logging only (trajectory recording); capacities of the active mode, hotel load, fuel coefficients
  double mode_me, mode_el, hotel, avail_prop;
  double fa_me, fb_me, fc_me, fa_dg, fb_dg, fc_dg;
  int32_t sg_state, pad_sg_;
  // controllers (controllers.py:45-209; run_colav ThrustFromSpeedSetPoint)
  double kp_ship_speed, ki_ship_speed, kp_shaft_speed, ki_shaft_speed, init_shaft_ei;
  double spd_kp, spd_ki, spd_kd, max_thrust;
  double hdg_kp, hdg_kd, hdg_ki;
  // NavigationSystem (LOS_guidance.py:38-58)
  double ra2, los_r, los_r2, los_ki, los_limit;
  double desired_speed;
  // SimulationConfiguration
  double init_n, init_e, init_yaw, init_u, init_v, init_r;
  int32_t n_route, pad_;
  // filled on the device by stage_consts (the host leaves them 0): div_rcp of r_me, r_hsg, jp and of the step dt
  double rcp_r_me, rcp_r_hsg, rcp_jp, rcp_dt;
};

struct Params {
  int32_t kind, machinery, collav, n_ships;
  int32_t max_sampling, n_envs, n_polys;
  int32_t epw;  // envs per wave of the AST step / stream kernels (0: 64 / lanes per env; fewer leave lanes idle)
  double dt, sim_time, mach_dt_reset, mach_dt_init;
  double vc_n, vc_e, wind_dir, wind_speed;
  double roa2;                       // args.radius_of_acceptance ** 2
  double sbmpc_tf, sbmpc_dt;
  // IW sampler (env.py:143-161), identical for every env of a handle
  double AB_seg, AB_seg_n, AB_seg_e, omega_iw, n_base0, e_base0;
  double min_north, max_north, min_east, max_east;
  float action_low, action_high;
  int32_t normalize_action, sbmpc_nsamp;  // sbmpc_nsamp = int(sbmpc_tf / sbmpc_dt) (sbmpc.py:121), host-evaluated
  float initial_states[8];           // env.py:107-109
  // host-evaluated sin/cos of uniform angles: wind_direction (algebraic wind force of the AST
  // kernels) and the IW sampler's omega (env.py:151-161)
  double wind_sin, wind_cos, iw_cos, iw_sin;
};

// Map edges (obstacle.py PolygonObstacle). Stored as a flat read-only device table; every lane
// walks it with the same (wave-uniform) index, so loads are scalar/broadcast.
struct Edge {
  double ax, ay, bx, by;   // (east, north) of the edge endpoints
};
struct PolyBox {
  double minx, maxx, miny, maxy;
  int32_t first, count, pad0, pad1;
};

// Python min/max semantics: min(a, b) returns a unless b < a
SHIPSIM_HD double py_min(double a, double b) { return (b < a) ? b : a; }
SHIPSIM_HD double py_max(double a, double b) { return (b > a) ? b : a; }

// ---------------------------------------------------------------------------------------------
// map queries (obstacle.py:126-141 over shapely/GEOS; restated GEOS semantics)
// ---------------------------------------------------------------------------------------------
// GEOS RayCrossingCounter for one polygon, boundary -> not contained
SHIPSIM_HD bool poly_contains(const Edge* __restrict__ edges, int first, int count, double px, double py) {
  int crossings = 0;
  bool boundary = false;
  for (int i = 0; i < count; ++i) {
    const Edge ed = edges[first + i];
    double x1 = ed.ax, y1 = ed.ay, x2 = ed.bx, y2 = ed.by;
    if (x1 < px && x2 < px) continue;
    if (px == x2 && py == y2) boundary = true;
    if (y1 == py && y2 == py) {
      double mn = py_min(x1, x2), mx = py_max(x1, x2);
      if (mn <= px && px <= mx) boundary = true;
      continue;
    }
    if ((y1 > py && y2 <= py) || (y2 > py && y1 <= py)) {
      double det = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1);
      int sign = (det > 0) - (det < 0);
      if (sign == 0) boundary = true;
      if (y2 < y1) sign = -sign;
      if (sign > 0) crossings++;
    }
  }
  return !boundary && (crossings & 1);
}

// if_pos_inside_obstacles :126-129 (bbox rejection is exact for the crossing rule)
SHIPSIM_HD bool map_inside(const Edge* __restrict__ edges, const PolyBox* __restrict__ boxes, int n_polys, double n,
                           double e) {
  bool inside = false;
  for (int p = 0; p < n_polys; ++p) {
    const PolyBox b = boxes[p];
    if (e < b.minx || e > b.maxx || n < b.miny || n > b.maxy) continue;
    if (poly_contains(edges, b.first, b.count, e, n)) inside = true;
  }
  return inside;
}

// a map grid cell's containment flag (ConstBuf::grid_flag)
#define GRID_OUT 0
#define GRID_IN 1
#define GRID_MIXED 2

// The ground-distance reward terms only use the coastline distance when it is <= 1000 m
// (reward_function.py:109-117: test_ship_grounding_reward / obs_ship_grounding_reward clip at 1 km),
// so a cell only needs the edges that can come within 1000 m of it: the min over that subset equals
// the min over all edges whenever the true min is <= 1000 m, and is > 1000 m (or +inf) otherwise.
constexpr double kGroundReach = 1000.0;

// The constant block (ConstBuf, shipsim_state.hpp): edges [SHIPSIM_MAX_VERTS] | boxes [SHIPSIM_MAX_POLYS] | config
// routes n / e [MAX_SHIPS][kMaxRoute] each | ShipConst [MAX_SHIPS], then the map grid at offsets of its own
// (config_host::const_block)
constexpr size_t kConstBoxesOff = sizeof(Edge) * SHIPSIM_MAX_VERTS;
constexpr size_t kConstRoutesOff = kConstBoxesOff + sizeof(PolyBox) * SHIPSIM_MAX_POLYS;
constexpr size_t kConstShipsOff = kConstRoutesOff + sizeof(double) * 2 * SHIPSIM_MAX_SHIPS * kMaxRoute;
constexpr size_t kConstBytes = kConstShipsOff + sizeof(ShipConst) * SHIPSIM_MAX_SHIPS;

}  // namespace shipsim
