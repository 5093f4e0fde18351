// shipsim_config_host.hpp — the half of shipsim_create that never touches the device: the default configurations,
// the config's validation, the per-ship constants, the launch parameters and the constant block with the map grid.
// Plain C++17, free of HIP and of the handle, so that it can be compiled and driven on its own:
// tests/test_config_host_cpu.py builds tests/config_host_check.cpp with -fsanitize=address,undefined and checks the
// block's layout, the grid's exactness, the parameters and every rule of validate. Every expression restates the
// reference's operand order (the library is built with -ffp-contract=off and the values feed bit-exact tests).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "shipsim.h"
#include "shipsim_launch_host.hpp"
#include "shipsim_types.hpp"

namespace config_host {

using namespace shipsim;

// the ship both default ships start from (run/env_setup.py, run_colav/run_simplified_model.py)
inline void fill_ship_common(shipsim_ship_config* s, double n, double e, double yaw, double u) {
  memset(s, 0, sizeof(*s));
  s->coefficient_of_deadweight_to_displacement = 0.7;
  s->bunkers = 200000;
  s->ballast = 200000;
  s->length_of_ship = 80;
  s->width_of_ship = 16;
  s->added_mass_coefficient_in_surge = 0.4;
  s->added_mass_coefficient_in_sway = 0.4;
  s->added_mass_coefficient_in_yaw = 0.4;
  s->dead_weight_tonnage = 3850000;
  s->mass_over_linear_friction_coefficient_in_surge = 130;
  s->mass_over_linear_friction_coefficient_in_sway = 18;
  s->mass_over_linear_friction_coefficient_in_yaw = 90;
  s->nonlinear_friction_coefficient_in_surge = 2400;
  s->nonlinear_friction_coefficient_in_sway = 4000;
  s->nonlinear_friction_coefficient_in_yaw = 400;
  s->initial_north_position_m = n;
  s->initial_east_position_m = e;
  s->initial_yaw_angle_rad = yaw;
  s->initial_forward_speed_m_per_s = u;
  s->rudder_angle_to_sway_force_coefficient = 50e3;
  s->rudder_angle_to_yaw_force_coefficient = 500e3;
  s->max_rudder_angle_degrees = 30;
  s->hotel_load = 200000;
  s->main_engine_capacity = 0;
  s->electrical_capacity = 2 * 510e3;
  s->shaft_generator_state = SHIPSIM_SG_MOTOR;
  s->rated_speed_main_engine_rpm = 1000;
  s->linear_friction_main_engine = 68;
  s->linear_friction_hybrid_shaft_generator = 57;
  s->gear_ratio_between_main_engine_and_propeller = 0.6;
  s->gear_ratio_between_hybrid_shaft_generator_and_propeller = 0.6;
  s->propeller_inertia = 6000;
  s->propeller_diameter = 3.1;
  s->propeller_speed_to_torque_coefficient = 7.5;
  s->propeller_speed_to_thrust_force_coefficient = 1.7;
  s->kp_ship_speed = 205.25;
  s->ki_ship_speed = 0.0525;
  s->kp_shaft_speed = 50;
  s->ki_shaft_speed = 0.00025;
  s->initial_shaft_speed_integral_error = 114;
  s->max_thrust = INFINITY;
  s->radius_of_acceptance = 300;
  s->lookahead_distance = 1000;
  s->los_integral_gain = 0.002;
  s->los_integrator_windup_limit = 4000;
}

inline void set_route(shipsim_ship_config* s, const double (*r)[2], int n) {
  s->n_route = n;
  for (int i = 0; i < n; ++i) {
    s->route_north[i] = r[i][0];
    s->route_east[i] = r[i][1];
  }
}

// shipsim_default_config (include/shipsim.h)
inline int default_config(int32_t kind, int32_t machinery, int32_t collav, double time_step, shipsim_config* cfg) {
  if (!cfg || kind < 0 || kind > 2 || machinery < 0 || machinery > 1 || collav < 0 || collav > 2) return SHIPSIM_EINVAL;
  static const double map_e_n[][2] = {
      {0, 10000}, {10000, 10000}, {9200, 9000}, {7600, 8500}, {6700, 7300}, {4900, 6500}, {4300, 5400},
      {4700, 4500}, {6000, 4000}, {5800, 3600}, {4200, 3200}, {3200, 4100}, {2000, 4500}, {1000, 4000},
      {900, 3500}, {500, 2600}, {0, 2350},
      {10000, 0}, {11500, 750}, {12000, 2000}, {11700, 3000}, {11000, 3600}, {11250, 4250}, {12300, 4000},
      {13000, 3800}, {14000, 3000}, {14500, 2300}, {15000, 1700}, {16000, 800}, {17500, 0},
      {15500, 10000}, {16000, 9000}, {18000, 8000}, {19000, 7500}, {20000, 6000}, {20000, 10000},
      {5500, 5300}, {6000, 5000}, {6800, 4500}, {8000, 5000}, {8700, 5500}, {9200, 6700}, {8000, 7000},
      {6700, 6300}, {6000, 6000},
      {15000, 5000}, {14000, 5500}, {12500, 5000}, {14000, 4100}, {16000, 2000}, {15700, 3700},
      {11000, 2000}, {10300, 3200}, {9000, 1500}, {10000, 1000}};
  static const int poly_counts[6] = {17, 13, 6, 9, 6, 4};
  static const double test_route[7][2] = {{0, 0}, {2000, 4500}, {2500, 7500}, {7000, 12000}, {6500, 16000},
                                          {3000, 17500}, {0, 20000}};
  static const double obs_route[2][2] = {{10000, 15000}, {0, 5000}};
  static const double obs_route_noniw[11][2] = {{10000, 15000}, {9500, 13500}, {8000, 13000}, {6500, 12500},
                                                {6000, 11000}, {5500, 9500}, {4000, 9000}, {2500, 8500},
                                                {2000, 7000}, {1500, 5500}, {0, 5000}};
  memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = SHIPSIM_ABI_VERSION;
  cfg->kind = kind;
  cfg->machinery = machinery;
  cfg->collav = collav;
  cfg->max_sampling_frequency = 9;
  cfg->machinery_dt_quirk = 1;
  cfg->normalize_action = 0;
  cfg->n_ships = kind == SHIPSIM_KIND_SINGLE ? 1 : 2;
  cfg->time_step = time_step;
  cfg->simulation_time = 10000;
  cfg->env_radius_of_acceptance = 300;
  cfg->current_velocity_component_from_north = -1;
  cfg->current_velocity_component_from_east = -1;
  cfg->wind_speed = 2;
  cfg->wind_direction = -M_PI / 4;
  cfg->sbmpc_tf = 1000;
  cfg->sbmpc_dt = 20;
  shipsim_ship_config* t = &cfg->ship[0];
  shipsim_ship_config* o = &cfg->ship[1];
  fill_ship_common(t, 100, 100, 60 * M_PI / 180, 4.25);
  fill_ship_common(o, 9900, 14900, -135 * M_PI / 180, 3.5);
  set_route(t, test_route, 7);
  t->desired_forward_speed = 4.5;
  o->desired_forward_speed = 4.0;
  if (kind == SHIPSIM_KIND_AST) {  // run/env_setup.py
    t->initial_propeller_shaft_speed_rad_per_s = 420 * M_PI / 30;
    o->initial_propeller_shaft_speed_rad_per_s = 200 * M_PI / 30;
    for (int i = 0; i < 2; ++i) {
      cfg->ship[i].heading_kp = 1.65; cfg->ship[i].heading_kd = 75; cfg->ship[i].heading_ki = 0.001;
      cfg->ship[i].speed_kp = 150; cfg->ship[i].speed_ki = 150; cfg->ship[i].speed_kd = 75;
    }
    set_route(o, obs_route, 2);
    cfg->action_low = (float)(-(30 * (M_PI / 180.0)));
    cfg->action_high = (float)(30 * (M_PI / 180.0));
  } else {  // run_colav/run_simplified_model.py
    t->speed_kp = 150; t->speed_ki = 150; t->speed_kd = 75;
    o->speed_kp = .025; o->speed_ki = 700.5; o->speed_kd = 550.5;
    t->heading_kp = .5; t->heading_ki = 0.01; t->heading_kd = 84;
    o->heading_kp = .65; o->heading_ki = 0.001; o->heading_kd = 50;
    set_route(o, obs_route_noniw, 11);
    cfg->action_low = (float)(-M_PI / 6);
    cfg->action_high = (float)(M_PI / 6);
  }
  int k = 0, p = 0;
  for (p = 0; p < 6; ++p) {
    cfg->poly_start[p] = k;
    for (int i = 0; i < poly_counts[p]; ++i, ++k) {
      cfg->poly_east[k] = map_e_n[k][0];
      cfg->poly_north[k] = map_e_n[k][1];
    }
  }
  cfg->poly_start[6] = k;
  cfg->n_polys = 6;
  return SHIPSIM_OK;
}

// host restatement of the constructors' derived constants (ship_model.py:412-474,
// ship_engine.py:32-44, 341-401)
inline void ship_const(const shipsim_ship_config* c, ShipConst* k) {
  memset(k, 0, sizeof(*k));
  double payload = 0.9 * (c->dead_weight_tonnage - c->bunkers);
  double lsw = c->dead_weight_tonnage / c->coefficient_of_deadweight_to_displacement - c->dead_weight_tonnage;
  k->mass = lsw + payload + c->bunkers + c->ballast;
  k->l_ship = c->length_of_ship;
  k->w_ship = c->width_of_ship;
  k->obs_l_cfg = c->length_of_ship;
  k->obs_w_cfg = c->width_of_ship;
  k->i_z = k->mass * (k->l_ship * k->l_ship + k->w_ship * k->w_ship) / 12;
  k->x_du = k->mass * c->added_mass_coefficient_in_surge;
  k->y_dv = k->mass * c->added_mass_coefficient_in_sway;
  k->n_dr = k->i_z * c->added_mass_coefficient_in_yaw;
  k->inv_m0 = 1.0 / (k->mass + k->x_du);
  k->inv_m1 = 1.0 / (k->mass + k->y_dv);
  k->inv_m2 = 1.0 / (k->i_z + k->n_dr);
  k->dlin0 = k->mass / c->mass_over_linear_friction_coefficient_in_surge;
  k->dlin1 = k->mass / c->mass_over_linear_friction_coefficient_in_sway;
  k->dlin2 = k->i_z / c->mass_over_linear_friction_coefficient_in_yaw;
  k->ku = c->nonlinear_friction_coefficient_in_surge;
  k->kv = c->nonlinear_friction_coefficient_in_sway;
  k->kr = c->nonlinear_friction_coefficient_in_yaw;
  k->rho_a = 1.2;
  k->proj_area_f = k->w_ship * 8.0;
  k->proj_area_l = k->l_ship * 8.0;
  k->cx = 0.5;
  k->cy = 0.7;
  k->cn = 0.08;
  k->c_rudder_v = c->rudder_angle_to_sway_force_coefficient;
  k->c_rudder_r = c->rudder_angle_to_yaw_force_coefficient;
  k->max_rudder = c->max_rudder_angle_degrees * M_PI / 180;
  double me = c->main_engine_capacity, el = c->electrical_capacity, hl = c->hotel_load;
  if (c->shaft_generator_state == SHIPSIM_SG_MOTOR) {
    k->avail_me = me;
    k->avail_el = el - hl;
  } else if (c->shaft_generator_state == SHIPSIM_SG_GEN) {
    k->avail_me = me - hl;
    k->avail_el = 0;
  } else {
    k->avail_me = me;
    k->avail_el = 0;
  }
  k->cap_me = k->avail_me / 5 * M_PI / 30;
  k->cap_el = k->avail_el / 5 * M_PI / 30;
  k->d_me = c->linear_friction_main_engine;
  k->d_hsg = c->linear_friction_hybrid_shaft_generator;
  k->r_me = c->gear_ratio_between_main_engine_and_propeller;
  k->r_hsg = c->gear_ratio_between_hybrid_shaft_generator_and_propeller;
  k->jp = c->propeller_inertia;
  k->kp_prop = c->propeller_speed_to_torque_coefficient;
  k->thrust_coeff = pow(c->propeller_diameter, 4) * c->propeller_speed_to_thrust_force_coefficient;
  k->shaft_speed_max = 1.1 * (c->rated_speed_main_engine_rpm * M_PI / 30) * k->r_me;
  k->init_omega = c->initial_propeller_shaft_speed_rad_per_s;
  k->mode_me = me;
  k->mode_el = el;
  k->hotel = hl;
  k->avail_prop = (c->shaft_generator_state == SHIPSIM_SG_MOTOR) ? me + el - hl
                  : (c->shaft_generator_state == SHIPSIM_SG_GEN) ? me - hl : me;  // :32-44
  k->sg_state = c->shaft_generator_state;
  // run/env_setup.py:85-104: SpecificFuelConsumptionWartila6L26 (ME) / Baudouin6M26Dot3 (DG),
  // ship_engine.py:88-112 (BaseMachineryModel.fuel_consumption uses these, not the
  // ShipMachineryModel.specific_fuel_coeffs_* literals)
  k->fa_me = 128.9; k->fb_me = -168.9; k->fc_me = 246.8;
  k->fa_dg = 108.7; k->fb_dg = -289.9; k->fc_dg = 324.9;
  k->kp_ship_speed = c->kp_ship_speed;
  k->ki_ship_speed = c->ki_ship_speed;
  k->kp_shaft_speed = c->kp_shaft_speed;
  k->ki_shaft_speed = c->ki_shaft_speed;
  k->init_shaft_ei = c->initial_shaft_speed_integral_error;
  k->spd_kp = c->speed_kp;
  k->spd_ki = c->speed_ki;
  k->spd_kd = c->speed_kd;
  k->max_thrust = c->max_thrust;
  k->hdg_kp = c->heading_kp;
  k->hdg_kd = c->heading_kd;
  k->hdg_ki = c->heading_ki;
  k->ra2 = c->radius_of_acceptance * c->radius_of_acceptance;
  k->los_r = c->lookahead_distance;
  k->los_r2 = c->lookahead_distance * c->lookahead_distance;
  k->los_ki = c->los_integral_gain;
  k->los_limit = c->los_integrator_windup_limit;
  k->desired_speed = c->desired_forward_speed;
  k->init_n = c->initial_north_position_m;
  k->init_e = c->initial_east_position_m;
  k->init_yaw = c->initial_yaw_angle_rad;
  k->init_u = c->initial_forward_speed_m_per_s;
  k->init_v = c->initial_sideways_speed_m_per_s;
  k->init_r = c->initial_yaw_rate_rad_per_s;
  k->n_route = c->n_route;
}

// 0, or 1 with the first broken rule's message in err[n]
inline int validate(const shipsim_config* cfg, char* err, size_t n) {
  if (cfg->abi_version != SHIPSIM_ABI_VERSION) return snprintf(err, n, "abi_version %d != %d", cfg->abi_version, SHIPSIM_ABI_VERSION), 1;
  if (cfg->kind < 0 || cfg->kind > 2) return snprintf(err, n, "bad kind %d", cfg->kind), 1;
  if (cfg->machinery < 0 || cfg->machinery > 1) return snprintf(err, n, "bad machinery %d", cfg->machinery), 1;
  if (cfg->collav < 0 || cfg->collav > 2) return snprintf(err, n, "bad collav %d", cfg->collav), 1;
  int ns = cfg->kind == SHIPSIM_KIND_SINGLE ? 1 : 2;
  if (cfg->kind == SHIPSIM_KIND_AST) {
    ns = cfg->n_ships;
    if (ns < 2 || ns > SHIPSIM_MAX_SHIPS)
      return snprintf(err, n, "n_ships %d: 1 ship under test + 1..%d obstacle ships", ns, SHIPSIM_MAX_OBS), 1;
    const char* why = launch_host::select(cfg->machinery, cfg->collav, ns, 16, false, false, launch_host::kStep).why;
    if (why) return snprintf(err, n, "%d obstacle ships: %s", ns - 1, why), 1;
  }
  if (cfg->n_ships != ns) return snprintf(err, n, "n_ships %d != %d for kind %d", cfg->n_ships, ns, cfg->kind), 1;
  if (!(cfg->time_step > 0)) return snprintf(err, n, "time_step must be > 0"), 1;
  if (cfg->max_sampling_frequency < 0 || cfg->max_sampling_frequency + 2 > SHIPSIM_MAX_ROUTE)
    return snprintf(err, n, "max_sampling_frequency %d out of range", cfg->max_sampling_frequency), 1;
  for (int i = 0; i < ns; ++i) {
    int nr = cfg->ship[i].n_route;
    if (nr < 2 || nr > SHIPSIM_MAX_ROUTE) return snprintf(err, n, "ship %d route length %d out of range", i, nr), 1;
    if (cfg->kind == SHIPSIM_KIND_AST && i == 1 && nr + cfg->max_sampling_frequency > SHIPSIM_MAX_ROUTE)
      return snprintf(err, n, "obstacle route %d + samplings %d exceeds %d", nr, cfg->max_sampling_frequency, SHIPSIM_MAX_ROUTE), 1;
  }
  if (cfg->n_polys < 0 || cfg->n_polys > SHIPSIM_MAX_POLYS) return snprintf(err, n, "n_polys %d out of range", cfg->n_polys), 1;
  if (cfg->poly_start[0] != 0 || cfg->poly_start[cfg->n_polys] > SHIPSIM_MAX_VERTS)
    return snprintf(err, n, "bad poly_start"), 1;
  for (int p = 0; p < cfg->n_polys; ++p)
    if (cfg->poly_start[p + 1] - cfg->poly_start[p] < 3) return snprintf(err, n, "polygon %d has < 3 vertices", p), 1;
  if (cfg->sbmpc_dt <= 0 || cfg->sbmpc_tf / cfg->sbmpc_dt > 4096) return snprintf(err, n, "bad sbmpc horizon"), 1;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// map grid (host): exact, conservative cell classification used by corner_inside / map_dist2_mask
// ---------------------------------------------------------------------------------------------
constexpr double kGridCell = 200.0;     // m
constexpr double kGridPad = 2000.0;     // m of grid beyond the polygon bounding box
constexpr double kGridEps = 1e-3;       // m: cells are enlarged by this before classification

// segment vs closed axis-aligned rectangle (Liang-Barsky clip)
inline bool seg_hits_rect(const Edge& ed, double x0, double y0, double x1, double y1) {
  double t0 = 0.0, t1 = 1.0;
  const double dx = ed.bx - ed.ax, dy = ed.by - ed.ay;
  const double p[4] = {-dx, dx, -dy, dy};
  const double q[4] = {ed.ax - x0, x1 - ed.ax, ed.ay - y0, y1 - ed.ay};
  for (int i = 0; i < 4; ++i) {
    if (p[i] == 0.0) {
      if (q[i] < 0.0) return false;
    } else {
      const double t = q[i] / p[i];
      if (p[i] < 0.0) { if (t > t1) return false; if (t > t0) t0 = t; }
      else { if (t < t0) return false; if (t < t1) t1 = t; }
    }
  }
  return true;
}
inline double point_seg_dist(double px, double py, const Edge& ed) {
  const double dx = ed.bx - ed.ax, dy = ed.by - ed.ay, l2 = dx * dx + dy * dy;
  double t = l2 > 0 ? ((px - ed.ax) * dx + (py - ed.ay) * dy) / l2 : 0.0;
  t = t < 0 ? 0 : (t > 1 ? 1 : t);
  const double ex = ed.ax + t * dx - px, ey = ed.ay + t * dy - py;
  return sqrt(ex * ex + ey * ey);
}
inline double point_rect_dist(double px, double py, double x0, double y0, double x1, double y1) {
  const double dx = px < x0 ? x0 - px : (px > x1 ? px - x1 : 0.0);
  const double dy = py < y0 ? y0 - py : (py > y1 ? py - y1 : 0.0);
  return sqrt(dx * dx + dy * dy);
}
inline double seg_rect_dist(const Edge& ed, double x0, double y0, double x1, double y1) {
  if (seg_hits_rect(ed, x0, y0, x1, y1)) return 0.0;
  double d = point_rect_dist(ed.ax, ed.ay, x0, y0, x1, y1);
  d = py_min(d, point_rect_dist(ed.bx, ed.by, x0, y0, x1, y1));
  d = py_min(d, point_seg_dist(x0, y0, ed));
  d = py_min(d, point_seg_dist(x1, y0, ed));
  d = py_min(d, point_seg_dist(x0, y1, ed));
  d = py_min(d, point_seg_dist(x1, y1, ed));
  return d;
}
// Fills mask/flag for a gnx x gny grid. A cell no edge touches is uniformly inside or outside
// (the polygons' boundary is the union of their edges), so its center decides it; any cell an
// edge touches is MIXED and gets the full test. Edge masks keep every edge within kGroundReach of
// the enlarged cell (+1 mm slack on the reach for rounding).
inline void build_grid(const Edge* E, int n_edges, const PolyBox* B, int n_polys, double gx0, double gy0, int gnx,
                       int gny, uint64_t* mask, uint8_t* flag) {
  for (int j = 0; j < gny; ++j)
    for (int i = 0; i < gnx; ++i) {
      const double x0 = gx0 + i * kGridCell - kGridEps, x1 = gx0 + (i + 1) * kGridCell + kGridEps;
      const double y0 = gy0 + j * kGridCell - kGridEps, y1 = gy0 + (j + 1) * kGridCell + kGridEps;
      uint64_t m = 0;
      bool touched = false;
      for (int k = 0; k < n_edges; ++k) {
        const double d = seg_rect_dist(E[k], x0, y0, x1, y1);
        if (d <= kGroundReach + kGridEps) m |= (uint64_t)1 << k;
        if (d == 0.0) touched = true;
      }
      mask[(size_t)j * gnx + i] = m;
      const double cx = 0.5 * (x0 + x1), cy = 0.5 * (y0 + y1);
      flag[(size_t)j * gnx + i] = touched ? GRID_MIXED : (map_inside(E, B, n_polys, cy, cx) ? GRID_IN : GRID_OUT);
    }
}

// the bounding box of the map's vertices (of poly_east[0] / poly_north[0] alone for a map without polygons)
struct MapBounds {
  double mn_e, mx_e, mn_n, mx_n;
};
inline MapBounds map_bounds(const shipsim_config* cfg) {
  const int nv = cfg->poly_start[cfg->n_polys];
  double mn_e = cfg->poly_east[0], mx_e = mn_e, mn_n = cfg->poly_north[0], mx_n = mn_n;
  for (int i = 0; i < nv; ++i) {
    if (cfg->poly_east[i] < mn_e) mn_e = cfg->poly_east[i];
    if (cfg->poly_east[i] > mx_e) mx_e = cfg->poly_east[i];
    if (cfg->poly_north[i] < mn_n) mn_n = cfg->poly_north[i];
    if (cfg->poly_north[i] > mx_n) mx_n = cfg->poly_north[i];
  }
  return {mn_e, mx_e, mn_n, mx_n};
}

// Everything shipsim_create writes into Params, for a validated config and n_envs envs
inline void params(const shipsim_config* cfg, int32_t n_envs, Params& P) {
  memset(&P, 0, sizeof(P));
  P.epw = cfg->envs_per_wave;  // performance knob (0 = full waves; results identical)
  const int ns = cfg->n_ships;
  P.kind = cfg->kind;
  P.machinery = cfg->machinery;
  P.collav = cfg->collav;
  P.n_ships = ns;
  P.max_sampling = cfg->max_sampling_frequency;
  P.n_envs = n_envs;
  P.n_polys = cfg->n_polys;
  P.dt = cfg->time_step;
  P.sim_time = cfg->simulation_time;
  P.mach_dt_init = cfg->time_step;
  P.mach_dt_reset = cfg->machinery_dt_quirk ? 0.01 : cfg->time_step;
  P.vc_n = cfg->current_velocity_component_from_north;
  P.vc_e = cfg->current_velocity_component_from_east;
  P.wind_dir = cfg->wind_direction;
  P.wind_speed = cfg->wind_speed;
  P.roa2 = cfg->env_radius_of_acceptance * cfg->env_radius_of_acceptance;
  P.sbmpc_tf = cfg->sbmpc_tf;
  P.sbmpc_nsamp = (int32_t)(cfg->sbmpc_tf / cfg->sbmpc_dt);
  P.sbmpc_dt = cfg->sbmpc_dt;
  P.wind_sin = sin(cfg->wind_direction);
  P.wind_cos = cos(cfg->wind_direction);
  P.action_low = cfg->action_low;
  P.action_high = cfg->action_high;
  P.normalize_action = cfg->normalize_action;
  if (ns >= 2) {  // init_get_intermediate_waypoints env.py:143-161 (ship 1 samples)
    const shipsim_ship_config* o = &cfg->ship[1];
    double ABn = o->route_north[o->n_route - 1] - o->route_north[0];
    double ABe = o->route_east[o->n_route - 1] - o->route_east[0];
    int msf = cfg->max_sampling_frequency;
    double AB_length = sqrt(ABn * ABn + ABe * ABe);
    P.AB_seg = AB_length / (msf + 1);
    P.AB_seg_n = ABn / (msf + 1);
    P.AB_seg_e = ABe / (msf + 1);
    double AB_alpha = atan2(ABe, ABn);
    double AB_beta = M_PI / 2 - AB_alpha;
    P.omega_iw = M_PI / 2 - AB_beta;
    P.iw_cos = cos(P.omega_iw);  // np.cos / np.sin of the scalar omega (env.py:226-227): glibc, as NumPy
    P.iw_sin = sin(P.omega_iw);
    P.n_base0 = P.AB_seg_n + o->route_north[0];
    P.e_base0 = P.AB_seg_e + o->route_east[0];
    P.initial_states[0] = (float)cfg->ship[0].initial_north_position_m;
    P.initial_states[1] = (float)cfg->ship[0].initial_east_position_m;
    P.initial_states[2] = 0.0f;
    P.initial_states[3] = (float)o->initial_north_position_m;
    P.initial_states[4] = (float)o->initial_east_position_m;
    P.initial_states[5] = (float)o->initial_yaw_angle_rad;
    P.initial_states[6] = 0.0f;
    P.initial_states[7] = (float)o->initial_forward_speed_m_per_s;
  }
  const MapBounds mb = map_bounds(cfg);
  P.min_east = mb.mn_e; P.max_east = mb.mx_e; P.min_north = mb.mn_n; P.max_north = mb.mx_n;
}

// The constant block as shipsim_create copies it to the device (ConstBuf's layout): edges | boxes | config routes |
// ShipConsts (ship_consts: SHIPSIM_MAX_SHIPS of them, those past the config's ships zero) | the map grid's cell masks
// and containment flags at grid_off | the masks split by bit rank mod 8 at part_off. The grid is built for a map of
// 1..64 vertices with map_query SHIPSIM_MAP_GRID; without it gnx = gny = 0 and bytes == part_off.
struct ConstBlock {
  char* host;  // the block, from calloc: the caller frees it
  size_t bytes, grid_off, part_off;
  int32_t n_edges, gnx, gny;
  double gx0, gy0;  // grid origin (east, north)
  bool use_grid;
};
// false: out of host memory (out.host is NULL, the sizes are set)
inline bool const_block(const shipsim_config* cfg, const ShipConst* ship_consts, ConstBlock& out) {
  const int ns = cfg->n_ships, nv = cfg->poly_start[cfg->n_polys];
  const MapBounds mb = map_bounds(cfg);
  const double mn_e = mb.mn_e, mx_e = mb.mx_e, mn_n = mb.mn_n, mx_n = mb.mx_n;
  const bool use_grid = nv <= 64 && nv > 0 && cfg->map_query == SHIPSIM_MAP_GRID;
  const int gnx = use_grid ? (int)ceil((mx_e - mn_e + 2 * kGridPad) / kGridCell) : 0;
  const int gny = use_grid ? (int)ceil((mx_n - mn_n + 2 * kGridPad) / kGridCell) : 0;
  const size_t gcells = (size_t)gnx * gny;
  const size_t grid_off = (kConstBytes + 255) & ~(size_t)255;
  const size_t part_off = (grid_off + gcells * (sizeof(uint64_t) + 1) + 7) & ~(size_t)7;
  const size_t cbytes = part_off + gcells * 8 * sizeof(uint64_t);
  char* hostc = (char*)calloc(1, cbytes);
  out = {hostc, cbytes, grid_off, part_off, nv, gnx, gny, mn_e - kGridPad, mn_n - kGridPad, use_grid};
  if (!hostc) return false;
  Edge* E = (Edge*)hostc;
  PolyBox* B = (PolyBox*)(hostc + kConstBoxesOff);
  double* R = (double*)(hostc + kConstRoutesOff);
  for (int p = 0; p < cfg->n_polys; ++p) {
    int s0 = cfg->poly_start[p], cnt = cfg->poly_start[p + 1] - s0;
    B[p].first = s0;
    B[p].count = cnt;
    B[p].minx = B[p].maxx = cfg->poly_east[s0];
    B[p].miny = B[p].maxy = cfg->poly_north[s0];
    for (int i = 0; i < cnt; ++i) {
      int j = (i + 1 == cnt) ? 0 : i + 1;
      E[s0 + i].ax = cfg->poly_east[s0 + i];
      E[s0 + i].ay = cfg->poly_north[s0 + i];
      E[s0 + i].bx = cfg->poly_east[s0 + j];
      E[s0 + i].by = cfg->poly_north[s0 + j];
      if (E[s0 + i].ax < B[p].minx) B[p].minx = E[s0 + i].ax;
      if (E[s0 + i].ax > B[p].maxx) B[p].maxx = E[s0 + i].ax;
      if (E[s0 + i].ay < B[p].miny) B[p].miny = E[s0 + i].ay;
      if (E[s0 + i].ay > B[p].maxy) B[p].maxy = E[s0 + i].ay;
    }
  }
  for (int s = 0; s < ns; ++s)
    for (int i = 0; i < cfg->ship[s].n_route; ++i) {
      R[s * kMaxRoute + i] = cfg->ship[s].route_north[i];
      R[SHIPSIM_MAX_SHIPS * kMaxRoute + s * kMaxRoute + i] = cfg->ship[s].route_east[i];
    }
  memcpy(hostc + kConstShipsOff, ship_consts, sizeof(ShipConst) * SHIPSIM_MAX_SHIPS);
  if (use_grid) {
    build_grid(E, nv, B, cfg->n_polys, mn_e - kGridPad, mn_n - kGridPad, gnx, gny, (uint64_t*)(hostc + grid_off),
               (uint8_t*)(hostc + grid_off + gcells * sizeof(uint64_t)));
    const uint64_t* gm = (const uint64_t*)(hostc + grid_off);
    uint64_t* gp = (uint64_t*)(hostc + part_off);
    for (size_t c = 0; c < gcells; ++c) {
      int rank = 0;
      for (int k = 0; k < 64; ++k)
        if (gm[c] >> k & 1) gp[c * 8 + (rank++ & 7)] |= (uint64_t)1 << k;
    }
  }
  return true;
}

}  // namespace config_host
