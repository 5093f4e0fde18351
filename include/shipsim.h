/*
 * shipsim.h — C ABI of the MI355X-native batched ship-in-transit simulator.
 *
 * The reference (AndreasKing-Goks/ast-sac) has no FFI: its boundary is the Python object API of
 * MultiShipRLEnv (rl_env/ship_in_transit/env.py:41) — reset() (:238) / step(action) (:624) —
 * plus run_colav/env.py:MultiShipNonIWEnv._step (:613) for the C1 loop and the
 * SimpleShipModel/controller loop of run_colav/run_simplified_model.py:245-249 for single ships.
 * These entry points are what that object API lowers to when N environments are batched on one
 * device; the Python facade in ast_sac_amd/ re-exposes the reference's reset/step signatures on
 * top of them (INTEGRATION.md shows the ctypes binding).
 *
 * Conventions
 *   - every function returns 0 on success or a negative SHIPSIM_E* code; never aborts or throws;
 *     shipsim_last_error(h) gives the message of the last failure on that handle.
 *   - one handle <-> one device <-> one HIP stream; calls are asynchronous on that stream.
 *     A handle is not thread-safe; handles on different devices are independent.
 *   - the library owns all device state (SoA ship state, per-env route tables, map);
 *     every I/O buffer below is a caller-owned DEVICE pointer (e.g. a torch tensor's data_ptr()).
 *   - no host allocation or synchronisation inside reset/step/tick.
 */
#ifndef SHIPSIM_H
#define SHIPSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHIPSIM_ABI_VERSION 12  /* 12: shipsim_set_weather / shipsim_get_weather (per-env wind and current) */
/* (shipsim_state_bytes / shipsim_snapshot / shipsim_restore / shipsim_fork came later and are additive: no struct
 * layout and no existing call changed, so the version stays 12; a binding looks the four symbols up on their own;
 * likewise shipsim_resample_workspace_bytes / shipsim_resample / shipsim_level_distance after them) */

#define SHIPSIM_MAX_ROUTE 16   /* waypoints per ship route (obs ship: 2 + max_sampling_frequency) */
#define SHIPSIM_MAX_POLYS 16   /* land polygons in the map */
#define SHIPSIM_MAX_VERTS 128  /* total polygon vertices */
#define SHIPSIM_MAX_OBS 4      /* obstacle ships per AST env (configs[4] C5: K in {1, 2, 4}) */
#define SHIPSIM_MAX_SHIPS (1 + SHIPSIM_MAX_OBS)

/* status codes */
#define SHIPSIM_OK 0
#define SHIPSIM_EINVAL -1   /* bad argument / config */
#define SHIPSIM_EHIP -2     /* HIP runtime failure */
#define SHIPSIM_ESTATE -3   /* call not valid in the current state (e.g. step before reset) */
#define SHIPSIM_ENOMEM -4
#define SHIPSIM_ENONFINITE -5 /* shipsim_synchronize: an env's ship state went NaN/Inf (see SHIPSIM_EV_NONFINITE) */

/* environment kinds */
#define SHIPSIM_KIND_SINGLE 0  /* one ship per env, no termination (config C2; run_simplified_model loop) */
#define SHIPSIM_KIND_NONIW 1   /* two ships, fixed routes, env_info flags only (C1; run_colav/env.py:37) */
#define SHIPSIM_KIND_AST 2     /* two-ship AST env with IW sampling + reward (C3/C4/C5; rl_env/.../env.py:41) */

/* collision avoidance of the ship under test (env.py:53, args.collav_mode) */
#define SHIPSIM_COLLAV_NONE 0
#define SHIPSIM_COLLAV_SIMPLE 1
#define SHIPSIM_COLLAV_SBMPC 2

/* propulsion model */
#define SHIPSIM_MACH_SIMPLIFIED 0 /* SimpleShipModel + ThrustFromSpeedSetPoint (run_colav) */
#define SHIPSIM_MACH_DETAILED 1   /* ShipModelAST + ShipMachineryModel + EngineThrottleFromSpeedSetPoint */

/* MachineryMode.shaft_generator_state (ship_engine.py:32-76) */
#define SHIPSIM_SG_GEN 0   /* PTO */
#define SHIPSIM_SG_MOTOR 1 /* PTI */
#define SHIPSIM_SG_OFF 2   /* MEC */

/* event bits, in the order get_reward_and_env_info appends its strings (reward_function.py:204-262) */
#define SHIPSIM_EV_COLLISION (1u << 0)
#define SHIPSIM_EV_TEST_GROUNDING (1u << 1)
#define SHIPSIM_EV_TEST_NAV_FAILURE (1u << 2)
#define SHIPSIM_EV_OBS_GROUNDING (1u << 3)
#define SHIPSIM_EV_OBS_NAV_FAILURE (1u << 4)
#define SHIPSIM_EV_TEST_REACHES_END (1u << 5)
#define SHIPSIM_EV_TEST_OUTSIDE_MAP (1u << 6)
#define SHIPSIM_EV_OBS_REACHES_END (1u << 7)
#define SHIPSIM_EV_OBS_OUTSIDE_MAP (1u << 8)
#define SHIPSIM_EV_TIME_LIMIT (1u << 9)
#define SHIPSIM_EV_SAMPLING_FAILURE (1u << 10) /* env.py:684 */
#define SHIPSIM_EV_TERMINAL (1u << 16)          /* env_info['terminal'] */
#define SHIPSIM_EV_TEST_STOP (1u << 17)         /* env_info['test_ship_stop'] */
#define SHIPSIM_EV_OBS_STOP (1u << 18)          /* env_info['obs_ship_stop'] */
#define SHIPSIM_EV_NONFINITE (1u << 24)         /* build-only, not a reference outcome: a ship state went
                                                   NaN/Inf in this decision; the decision ends at once with
                                                   done = 1 and SHIPSIM_EV_TERMINAL (boundary error contract) */

/* One ship: ShipConfiguration (ship_model.py:20), SimulationConfiguration (:45), rudder / machinery
 * (ship_engine.py:121,160), controller gains (controllers.py:16-38), LOS (LOS_guidance.py:15) and
 * the route file contents. Field names follow the reference's NamedTuple fields. */
typedef struct shipsim_ship_config {
  double dead_weight_tonnage;
  double coefficient_of_deadweight_to_displacement;
  double bunkers;
  double ballast;
  double length_of_ship;
  double width_of_ship;
  double added_mass_coefficient_in_surge;
  double added_mass_coefficient_in_sway;
  double added_mass_coefficient_in_yaw;
  double mass_over_linear_friction_coefficient_in_surge;
  double mass_over_linear_friction_coefficient_in_sway;
  double mass_over_linear_friction_coefficient_in_yaw;
  double nonlinear_friction_coefficient_in_surge;
  double nonlinear_friction_coefficient_in_sway;
  double nonlinear_friction_coefficient_in_yaw;
  /* initial state (SimulationConfiguration) */
  double initial_north_position_m;
  double initial_east_position_m;
  double initial_yaw_angle_rad;
  double initial_forward_speed_m_per_s;
  double initial_sideways_speed_m_per_s;
  double initial_yaw_rate_rad_per_s;
  /* rudder */
  double rudder_angle_to_sway_force_coefficient;
  double rudder_angle_to_yaw_force_coefficient;
  double max_rudder_angle_degrees;
  /* detailed machinery (MachinerySystemConfiguration, one active MachineryMode) */
  double hotel_load;
  double main_engine_capacity;
  double electrical_capacity;
  double rated_speed_main_engine_rpm;
  double linear_friction_main_engine;
  double linear_friction_hybrid_shaft_generator;
  double gear_ratio_between_main_engine_and_propeller;
  double gear_ratio_between_hybrid_shaft_generator_and_propeller;
  double propeller_inertia;
  double propeller_speed_to_torque_coefficient;
  double propeller_diameter;
  double propeller_speed_to_thrust_force_coefficient;
  double initial_propeller_shaft_speed_rad_per_s;
  /* EngineThrottleFromSpeedSetPoint gains (detailed) */
  double kp_ship_speed;
  double ki_ship_speed;
  double kp_shaft_speed;
  double ki_shaft_speed;
  double initial_shaft_speed_integral_error;
  /* ThrustFromSpeedSetPoint PID (simplified); max_thrust may be +inf */
  double speed_kp;
  double speed_ki;
  double speed_kd;
  double max_thrust;
  /* heading autopilot PID */
  double heading_kp;
  double heading_kd;
  double heading_ki;
  /* LOS guidance */
  double radius_of_acceptance;
  double lookahead_distance;
  double los_integral_gain;
  double los_integrator_windup_limit;
  double desired_forward_speed;
  int32_t shaft_generator_state; /* SHIPSIM_SG_* */
  int32_t n_route;               /* waypoints in route_north/route_east */
  double route_north[SHIPSIM_MAX_ROUTE];
  double route_east[SHIPSIM_MAX_ROUTE];
} shipsim_ship_config;

typedef struct shipsim_config {
  int32_t abi_version;            /* = SHIPSIM_ABI_VERSION */
  int32_t kind;                   /* SHIPSIM_KIND_* */
  int32_t machinery;              /* SHIPSIM_MACH_* */
  int32_t collav;                 /* SHIPSIM_COLLAV_* */
  int32_t max_sampling_frequency; /* args.max_sampling_frequency (9) */
  int32_t machinery_dt_quirk;     /* 1: machinery integrates with dt 0.01 after reset */
  int32_t normalize_action;       /* args.normalize_action: env denormalizes [-1,1] itself */
  int32_t n_ships;                /* 1 (SINGLE), 2 (NONIW), 1 + K obstacle ships (AST, K <= SHIPSIM_MAX_OBS) */
  double time_step;               /* args.time_step */
  double simulation_time;         /* SimulationConfiguration.simulation_time */
  double env_radius_of_acceptance;/* args.radius_of_acceptance used by is_reach_radius_of_acceptance */
  /* EnvironmentConfiguration */
  double current_velocity_component_from_north;
  double current_velocity_component_from_east;
  double wind_speed;
  double wind_direction;
  /* SBMPC(tf, dt) (env.py:123) */
  double sbmpc_tf;
  double sbmpc_dt;
  /* action box of the wrapped env (env.py:93-104), float32 as in the reference */
  float action_low;
  float action_high;
  /* [0] ship under test, [1] the obstacle ship (intermediate-waypoint sampling, the decisions, the
   * observation), [2..K] further obstacle ships (AST with K > 1, see shipsim_create) */
  shipsim_ship_config ship[SHIPSIM_MAX_SHIPS];
  /* PolygonObstacle map: polygon p owns vertices [poly_start[p], poly_start[p+1]), (east, north) */
  int32_t n_polys;
  int32_t poly_start[SHIPSIM_MAX_POLYS + 1];
  double poly_east[SHIPSIM_MAX_VERTS];
  double poly_north[SHIPSIM_MAX_VERTS];
  /* performance knob (no effect on results): device lanes per AST env, 2/4/8/16 (the decision
   * stream runs 4/8/16); 0 = $SHIPSIM_LPE or automatic (shipsim_lanes_per_env) */
  int32_t lanes_per_env;
  /* performance knobs (no effect on results; ABI 8): envs per wave (0 = as many as the wave holds, 64 / LPE;
   * fewer leave idle lanes), and the coastline query (SHIPSIM_MAP_GRID: the candidate edges of the ship's
   * 200 m grid cell; SHIPSIM_MAP_ALL_EDGES: every edge, the reference's own loop) */
  int32_t envs_per_wave;
  int32_t map_query;
  int32_t reserved[5];
} shipsim_config;

#define SHIPSIM_MAP_GRID 0
#define SHIPSIM_MAP_ALL_EDGES 1

/* Per-ship state fields for get/set_state (SoA, double unless noted; [env][ship], n_ships = 1 + K) */
#define SHIPSIM_F_NORTH 0
#define SHIPSIM_F_EAST 1
#define SHIPSIM_F_YAW 2
#define SHIPSIM_F_U 3
#define SHIPSIM_F_V 4
#define SHIPSIM_F_R 5
#define SHIPSIM_F_OMEGA 6        /* propeller shaft speed (detailed) */
#define SHIPSIM_F_TIME 7         /* ship_model.int.time */
#define SHIPSIM_F_E_CT 8         /* navigate.e_ct */
#define SHIPSIM_F_E_CT_INT 9     /* navigate.e_ct_int */
#define SHIPSIM_F_HDG_EI 10      /* heading PID error_i */
#define SHIPSIM_F_HDG_PREV 11    /* heading PID prev_error */
#define SHIPSIM_F_SPD_A 12       /* ship-speed PI error_i (detailed) | thrust PID error_i (simplified) */
#define SHIPSIM_F_SPD_B 13       /* shaft-speed PI error_i (detailed) | thrust PID prev_error (simplified) */
#define SHIPSIM_F_RUDDER 14      /* last commanded rudder angle (logged) */
#define SHIPSIM_F_THRUST 15      /* last thrust force [N] (logged) */
#define SHIPSIM_F_LOG_ECT 16     /* last logged cross-track error */
#define SHIPSIM_F_NEXT_WPT 17    /* int32: auto_pilot.next_wpt */
#define SHIPSIM_F_STOP 18        /* int32: ShipAssets.stop_flag */
#define SHIPSIM_N_SHIP_FIELDS 19

/* Per-env fields (AST / NONIW) */
#define SHIPSIM_E_SAMPLING_COUNT 100 /* int32 */
#define SHIPSIM_E_TRAVEL_DIST 101
#define SHIPSIM_E_TRAVEL_TIME 102
#define SHIPSIM_E_ACC_REWARD 103
#define SHIPSIM_E_N_BASE 104
#define SHIPSIM_E_E_BASE 105
#define SHIPSIM_E_SBMPC_P_LAST 106
#define SHIPSIM_E_SBMPC_CHI_LAST 107
#define SHIPSIM_E_ROUTE_LEN 108      /* int32: obstacle-ship route length */
#define SHIPSIM_E_ROUTE_NORTH 109    /* double[SHIPSIM_MAX_ROUTE] per env, env-major */
#define SHIPSIM_E_ROUTE_EAST 110

typedef struct shipsim_handle shipsim_handle;

/* Build info / ABI version of the loaded library. */
int32_t shipsim_abi_version(void);
const char* shipsim_build_info(void);

/* Fill *cfg with the reference scenario of record:
 *   kind SHIPSIM_KIND_AST : run/env_setup.py:17-254 (two ShipModelAST, PTI machinery, time_step 4,
 *                           runner defaults run/ast-sac_runner.py:27-43), collav as given;
 *   kind SHIPSIM_KIND_NONIW / SINGLE : run_colav/run_simplified_model.py:55-233 (SimpleShipModel,
 *                           ThrustFromSpeedSetPoint, time_step 30).
 * Routes and the 6-polygon map are the reference data files' contents. */
int shipsim_default_config(int32_t kind, int32_t machinery, int32_t collav, double time_step,
                           shipsim_config* cfg);

/* Allocate device state for n_envs environments on `device`, bound to `stream` (hipStream_t;
 * NULL = default stream). The handle starts un-reset.
 * n_obs_ships (AST kind): obstacle ships per env, 1..SHIPSIM_MAX_OBS (<= 0: cfg->n_ships - 1), configured
 * in cfg->ship[1..K]. K = 1 is the reference env (rl_env/ship_in_transit/env.py:76 unpacks [test, obs]).
 * K > 1 generalises it the way the reference's own pieces already do — parity unpinned beyond them:
 *   - SBMPC of the ship under test sees every obstacle ship (env.py:366-370 builds do_list from
 *     assets[1::]; sbmpc.py:150-176: active when any is within D_INIT, worst obstacle per scenario);
 *   - ship 1 is "the" obstacle ship: it samples the intermediate waypoints from the action, its radius
 *     of acceptance ends a decision, its grounding / navigation failure terms enter the reward and the
 *     observation reports it (env.py:538-773, reward_function.py:59-270);
 *   - ships 2..K follow their own routes with the same autopilot / throttle controllers (obs_step
 *     without sampling) and freeze (obs_step's stop branch) once they reach their last waypoint, leave
 *     the map or ground;
 *   - the collision reward / termination and the encounter angle use the nearest obstacle ship.
 * K > 1 needs detailed machinery and collav none or sbmpc. */
int shipsim_create(const shipsim_config* cfg, int32_t n_envs, int32_t n_obs_ships, int32_t device, void* stream,
                   shipsim_handle** out);
int shipsim_destroy(shipsim_handle* h);
/* Message of the last failed call on h; with h == NULL, of the calling thread's last shipsim_create that
 * failed before it could hand out a handle (every such path sets it; it is per thread). */
const char* shipsim_last_error(const shipsim_handle* h);
/* Launches of this handle go to `stream` from now on (e.g. a graph-capturing stream; ABI 6). */
int shipsim_set_stream(shipsim_handle* h, void* stream);
int32_t shipsim_num_envs(const shipsim_handle* h);
/* Lanes per AST env the step / stream kernels run at (config lanes_per_env, or chosen at create from
 * n_envs and the device's SIMD count; a performance knob only, results are identical). */
int32_t shipsim_lanes_per_env(const shipsim_handle* h);

/* MultiShipRLEnv.reset(): every env with env_mask[i] != 0 (NULL = all) is reset and placed with
 * init_step (one control + integrate tick, env.py:297); obs_out (N x 8 float32, device, may be NULL)
 * receives the reference's constant initial_states row for reset envs (Q11). */
int shipsim_reset(shipsim_handle* h, const uint8_t* env_mask, float* obs_out);

/* MultiShipRLEnv.step(action) for all N envs at once (AST kind only), sliced.
 * Every active env ticks (_step, env.py:563) until its decision point (RoA + one tick, or done —
 * env.py:700-771) or until it has run `max_ticks` ticks in this call (<= 0: no limit). An env that
 * paused keeps its decision in progress and resumes in the next call WITHOUT consuming an action;
 * an env waiting for a decision (after reset or after its previous decision completed) first
 * consumes action[i] (intermediate-waypoint sampling, env.py:659-696).
 *   action     N float32 scoping angles in radians (already denormalized, i.e. what
 *              NormalizedBoxEnv passes to the wrapped env), device.
 *   active     optional N uint8 mask (NULL = all): envs with 0 are left untouched.
 * Outputs (device, each may be NULL):
 *   ready  N uint8: 1 if the env completed a decision in this call; then obs (N x 8 float32),
 *          reward (N double, un-scaled accumulated reward of the decision), done (N uint8,
 *          combined_done) and events (N uint32, SHIPSIM_EV_* bits) hold that decision's result;
 *          rows of envs that did not complete are left untouched.
 *   ticks  N int32: _step calls executed by the env in this call. */
int shipsim_step(shipsim_handle* h, const float* action, const uint8_t* active, int32_t max_ticks,
                 float* obs_out, double* reward_out, uint8_t* done_out, uint32_t* events_out,
                 int32_t* ticks_out, uint8_t* ready_out);

/* Raw ticks for the SINGLE and NONIW kinds: advance every env by k ticks of the reference loop body
 * (run_simplified_model.py:248-249; for NONIW MultiShipNonIWEnv._step, run_colav/env.py:613-676: both ships'
 * steps with their SBMPC blocks in the reference's order, get_env_info's flags and the stop flags; simplified
 * machinery only). events_out (N uint32, may be NULL) receives the env_info bits (SHIPSIM_EV_*) of the last tick
 * (NONIW). The C1 loop runs while the test ship's F_TIME < simulation_time. */
int shipsim_tick(shipsim_handle* h, int32_t k, uint32_t* events_out);

/* Read / write one state field for all envs (device pointer dst/src). Ship fields are laid out
 * env-major [env][ship] (the device lane order), env fields [env], routes [env][ship][SHIPSIM_MAX_ROUTE]. */
int shipsim_get_state(shipsim_handle* h, int32_t field, void* dst);
int shipsim_set_state(shipsim_handle* h, int32_t field, const void* src);

/* ---- snapshot, restore and fork: exact clones of env states on the device --------------------------------
 * The fields above are a view; what an env continues from is the whole state block of the handle: every ship
 * array (the 19 fields, the logged position, the route length), both route arrays and every env array — the
 * decision flags and phase, the ticks of the decision in progress, the reset flag, the machinery dt, the
 * observations and states the collision checks and the decision record read. These calls move that block,
 * shipsim_state_bytes(h) bytes for this handle (a negative SHIPSIM_E* code for a NULL handle).
 *   shipsim_snapshot  copies it into dst, a caller-owned device buffer of that size.
 *   shipsim_restore   puts a snapshot back: from the next launch on shipsim_step, shipsim_run_table,
 *                     shipsim_run_policy, shipsim_tick, shipsim_legacy_step and shipsim_get_state give, bit for bit,
 *                     what they gave after the snapshot was taken — provided the caller also puts back the arrays
 *                     it owns (ep_idx, dec_idx, log_len, the policy's counter).
 *   shipsim_fork      after the call env i holds the state env src_env[i] had before it. src_env: n_envs int32 on
 *                     the device; NULL = identity. from: a snapshot (16-byte aligned) of a handle of the same shape,
 *                     or NULL for the handle's own state as it is. Any index array is served — permutations,
 *                     broadcasts, cycles: a fork from the handle's own state is gathered into a library-owned
 *                     staging block of the same size (allocated at the first such call; SHIPSIM_ENOMEM /
 *                     SHIPSIM_EHIP if that fails) and copied back, one kernel launch and one copy; from a snapshot
 *                     it is one launch (src_env == NULL: a restore). An index outside [0, n_envs) leaves env i as
 *                     it is (defined behaviour; the kernel tests the index before it forms an address). The state
 *                     block never moves: captured graphs that hold its address stay valid.
 * All three are asynchronous on the handle's stream, without host synchronisation or host allocation (but for
 * the staging block's allocation), and may be captured into a graph once the staging block exists.
 * Not state, staying with the handle and the slot: the config, per-env weather, the stream tail, lanes per env, the
 * non-finite counter, trajectory buffers. So a clone sails under the weather of the slot it lands in, unless the
 * caller moves the weather with it (shipsim_weather_fork / _store / _load, by the same index array); under a
 * stochastic policy it draws its slot's noise (Philox is keyed by env index), which is what splitting wants; an env
 * cloned while paused mid-decision resumes without consuming an action, one cloned while awaiting a decision
 * consumes its new slot's action. A snapshot may go into another handle of the same kind, n_envs and ship count,
 * whatever its lanes per env (results do not depend on them); restoring, or forking from a snapshot, onto a handle
 * never reset is allowed and marks it reset. All kinds (AST with K = 1..4, NONIW, SINGLE).
 * SHIPSIM_EINVAL with the reason in shipsim_last_error: bytes != shipsim_state_bytes(h); a NULL dst / src; a
 * handle with trajectory recording enabled (rows, lengths and fuel are not part of a snapshot). SHIPSIM_ESTATE:
 * a snapshot, or a fork from the handle's own state, before the first reset. */
int64_t shipsim_state_bytes(const shipsim_handle* h);
int shipsim_snapshot(shipsim_handle* h, void* dst, int64_t bytes);
int shipsim_restore(shipsim_handle* h, const void* src, int64_t bytes);
int shipsim_fork(shipsim_handle* h, const void* from, int64_t bytes, const int32_t* src_env);

/* ---- weighted splitting: resample a population of envs in proportion to weight x potential -----------------
 * shipsim_resample turns n weights and n potentials into the index array a shipsim_fork takes and the weights the
 * clones carry, such that sum_j weight_out[j] * f(x[src_out[j]]) is an unbiased estimate of sum_i weight[i] * f(x[i])
 * for any potential > 0 (systematic resampling). It is stateless like shipsim_sbmpc_eval_multi: no handle, device
 * pointers, asynchronous on `stream`, no host synchronisation and no allocation, so it can be captured into a graph
 * next to shipsim_fork. Everything it keeps between its launches lives in `workspace`, a caller-owned device buffer
 * of at least shipsim_resample_workspace_bytes(n) bytes, 16-byte aligned (contents undefined before and after).
 * weight_out may be weight. *counter is read by the launch and not changed, as in shipsim_run_policy.
 *
 * The arithmetic is in integers, so that any association order of the scans — and the restatement in
 * tests/resample_ref.py — gives the same bits (ast_sac_amd/csrc/shipsim_resample_host.hpp):
 *   mass      p_i = weight[i] * potential[i] (one IEEE multiply); m = max_i p_i.
 *             *status_out = 2 if any p_i is negative or not finite, 1 if m == 0; then src_out[j] = j,
 *             weight_out = weight, *total_out = 0: defined behaviour, nothing to check on the host. 0 otherwise.
 *   quantise  m = f * 2^e with f in [0.5, 1) (frexp): q_i = (uint64) ceil(ldexp(p_i, 40 - e)), so q_i >= 1 exactly
 *             when p_i > 0 and the largest is in [2^39, 2^40].
 *   scan      C_i = q_0 + ... + q_i in uint64; Q = C_{n-1} <= 2^62.
 *   offset    one Philox4x32-10 block keyed by seed {lo, hi} on the counter words {*counter lo, *counter hi,
 *             0x52455341, 0} gives c0..c3; U = ((c0 | c1 << 32) * 2^64 + (c2 | c3 << 32)) mod Q.
 *   positions t_j = floor((j * Q + U) / n), formed as j * s + (j * r + U) / n with Q = s * n + r; sel[j] = the
 *             smallest i with C_i > t_j. Env i is selected floor(n q_i / Q) or ceil(n q_i / Q) times, n q_i / Q in
 *             the mean over U.
 *   arrange   SHIPSIM_RESAMPLE_SORTED: src_out = sel. SHIPSIM_RESAMPLE_IN_PLACE: every selected env keeps its slot
 *             (src_out[i] = i); its further clones, in increasing source order, fill the slots of the envs that
 *             were not selected, in increasing slot order — a survivor never moves, so it keeps its slot's weather,
 *             noise and table columns, and shipsim_fork leaves it untouched.
 *   weights   weight_out[j] = weight[s] * ((double)Q / ((double)n * (double)q_s)), s = src_out[j] (conversions to
 *             nearest, three IEEE operations, no contraction); *total_out = ldexp((double)Q, e - 40), the total
 *             mass the weights preserve: in [sum p, sum p * (1 + n * 2^-39)].
 * total_out and status_out may be NULL. SHIPSIM_EINVAL, before any device call: n < 1 or n >
 * SHIPSIM_RESAMPLE_MAX_N; a NULL weight, potential, counter, workspace, src_out or weight_out; an arrangement other
 * than the two; workspace_bytes too small or a workspace not 16-byte aligned. shipsim_resample_workspace_bytes gives
 * SHIPSIM_EINVAL for such an n and does not decrease with n.
 *
 * shipsim_level_distance writes, per env, min over the obstacle ships k = 1..K of sqrt(dn * dn + de * de) with
 * dn = north[0] - north[k], de = east[0] - east[k] (n_envs doubles on the device, asynchronous on the handle's
 * stream): the level a distance-based potential is built from, as the plain expression, so that it has the bits of
 * the same expression on shipsim_get_state's values. AST handles with K = 1..4 and NONIW handles; SHIPSIM_EINVAL on
 * a SINGLE handle or a NULL out, SHIPSIM_ESTATE before the first reset (the reason in shipsim_last_error). */
#define SHIPSIM_RESAMPLE_SORTED 0
#define SHIPSIM_RESAMPLE_IN_PLACE 1
#define SHIPSIM_RESAMPLE_MAX_N (1 << 22)
int64_t shipsim_resample_workspace_bytes(int32_t n);
int shipsim_resample(int32_t n, const double* weight, const double* potential, uint64_t seed, const int64_t* counter,
                     int32_t arrangement, void* workspace, int64_t workspace_bytes, int32_t* src_out,
                     double* weight_out, double* total_out, int32_t* status_out, void* stream);
int shipsim_level_distance(shipsim_handle* h, double* out);

/* ---- state archive: elect per cell, store, start envs from it (additive to ABI 12) --------------------------
 * An archive is a caller-owned device buffer, 16-byte aligned, that holds the state block of n_cells envs of the
 * handle's ship count: the same 43 columns at the same bytes per env as the handle's own block, laid out for n_cells
 * instead of n_envs (only the strides differ), shipsim_archive_bytes(h, n_cells) bytes (SHIPSIM_EINVAL for a NULL
 * handle or n_cells outside 1..SHIPSIM_ARCHIVE_MAX_CELLS). Its size is the caller's choice, single cells of it are
 * overwritten, and any env starts from any cell: the node pool of a tree search, the cell store of Go-Explore. An
 * archive of n_cells == n_envs is byte for byte a snapshot, and shipsim_fork(h, archive, ...) takes it. The padding
 * between the columns is never written: zero the buffer once if its bytes are to be compared.
 *   shipsim_archive_store  cell c takes the live state of env env_of_cell[c] (n_cells int32 on the device). An index
 *                          outside [0, n_envs) leaves cell c as it is. SHIPSIM_ESTATE before the first reset.
 *   shipsim_archive_load   env i takes the state of cell cell_of_env[i] (n_envs int32 on the device), written
 *                          straight into the live block: archive and block never overlap, so there is no staging
 *                          block, and the block does not move (captured graphs stay valid). An index outside
 *                          [0, n_cells) leaves env i alone. Marks the handle reset, as shipsim_restore does.
 * Both are one kernel launch, asynchronous on the handle's stream, without allocation or synchronisation, and may
 * be captured into a graph. The index is tested before any address is formed from it; the loads are gathered and
 * the stores consecutive, so duplicate indices are harmless and no state can be torn. All kinds that shipsim_fork
 * serves (AST with K = 1..4, NONIW, SINGLE); what is not state (weather, the config, the stream tail) stays with the
 * slot, as under shipsim_fork (per-env weather goes into a weather buffer of n_cells slots beside the archive:
 * shipsim_weather_store / _load with the same index arrays), and the arrays the caller owns (ep_idx, dec_idx, log_len) are the caller's to keep
 * per cell. SHIPSIM_EINVAL with the reason in shipsim_last_error: a NULL archive or index array; n_cells < 1 or
 * above SHIPSIM_ARCHIVE_MAX_CELLS; bytes != shipsim_archive_bytes(h, n_cells); an archive not 16-byte aligned; a
 * handle with trajectory recording enabled.
 *
 * shipsim_archive_elect decides which env each cell takes. It is stateless like shipsim_resample: no handle, device
 * pointers, asynchronous on `stream`, no host synchronisation and no allocation, capturable; what its launches hand
 * one another lives in `workspace`, a caller-owned device buffer of at least shipsim_archive_workspace_bytes(n_cells)
 * bytes, 16-byte aligned (contents undefined before and after).
 *   candidates  env i (of n_envs) is a candidate of cell cell[i] when that index is in [0, n_cells) and score[i] is
 *               not NaN.
 *   winner      of a cell: its candidate with the largest score by IEEE > (-0.0 and +0.0 compare equal); ties go to
 *               the lowest env index.
 *   fill        the winner takes the cell when cell_score[c] is NaN (the cell is empty) or its score is strictly
 *               greater: env_of_cell_out[c] = the winner and cell_score[c] = its score as given. Otherwise
 *               env_of_cell_out[c] = -1 and cell_score[c] stays. env_of_cell_out (n_cells int32) is what
 *               shipsim_archive_store takes.
 *   counts      cell_seen[c] (n_cells int32, may be NULL) += the cell's candidates; *n_improved_out (may be NULL) =
 *               the number of cells taken.
 * The result does not depend on the order in which anything runs: across envs it is a 64-bit unsigned max over an
 * order-preserving image of the score, then a 32-bit min of the env index among the envs that hold the cell's max,
 * and integer adds (ast_sac_amd/csrc/shipsim_archive_host.hpp; restated in tests/archive_ref.py). SHIPSIM_EINVAL,
 * before any device call: n_envs < 1 or above 2^22; n_cells < 1 or above SHIPSIM_ARCHIVE_MAX_CELLS; a NULL cell,
 * score, cell_score, workspace or env_of_cell_out; workspace_bytes too small or a workspace not 16-byte aligned.
 * shipsim_archive_workspace_bytes gives SHIPSIM_EINVAL for such an n_cells and does not decrease with n_cells. */
#define SHIPSIM_ARCHIVE_MAX_CELLS (1 << 22)
int64_t shipsim_archive_bytes(const shipsim_handle* h, int32_t n_cells);
int shipsim_archive_store(shipsim_handle* h, void* archive, int64_t bytes, int32_t n_cells,
                          const int32_t* env_of_cell);
int shipsim_archive_load(shipsim_handle* h, const void* archive, int64_t bytes, int32_t n_cells,
                         const int32_t* cell_of_env);
int64_t shipsim_archive_workspace_bytes(int32_t n_cells);
int shipsim_archive_elect(int32_t n_envs, int32_t n_cells, const int32_t* cell, const double* score,
                          double* cell_score, int32_t* cell_seen, void* workspace, int64_t workspace_bytes,
                          int32_t* env_of_cell_out, int32_t* n_improved_out, void* stream);

/* ---- search tree over archived states: select, expand, back up (additive to ABI 12) ------------------------------
 * The env is deterministic given its action sequence, so a node of the tree is a state: node id i is cell i of a
 * state archive of max_nodes cells, and only actions are widened progressively. A tree is a caller-owned device
 * buffer, 16-byte aligned, of shipsim_tree_bytes(max_nodes, max_children) bytes: max_nodes in
 * 1..SHIPSIM_ARCHIVE_MAX_CELLS, max_children (C) in 1..SHIPSIM_TREE_MAX_CHILDREN. It is a structure of arrays whose
 * byte offsets shipsim_tree_layout writes into offsets_out[SHIPSIM_TREE_LAYOUT_FIELDS], in this order:
 *   header      int32[4]: n_nodes; dropped, the new nodes the pool had no room for; skipped, the backups not taken;
 *               hdr[3] = n_roots, the roots of a forest (0, as shipsim_tree_init writes it, reads as 1)
 *   parent      int32 [max_nodes], -1 for the root        depth      int32 [max_nodes]
 *   n_children  int32 [max_nodes]                         child      int32 [max_nodes * C], in creation order
 *   visits      int32 [max_nodes]                         value_sum  int64 [max_nodes], round(value * 2^24) summed
 *   action      float32 [max_nodes], the edge from the parent         flags  int32 [max_nodes], bit 0: terminal
 *   and the buffer's size.
 * The calls are stateless like shipsim_archive_elect: no handle, device pointers, asynchronous on `stream` (a
 * hipStream_t, NULL for the default stream), no allocation and no host synchronisation, so that a linear graph can
 * capture them. What their launches hand one another lives in `workspace`, a caller-owned device buffer, 16-byte
 * aligned, of at least shipsim_tree_workspace_bytes(max_nodes, n_workers) bytes, which does not decrease in either
 * argument; select and expand of one round may share it. n_workers (W) is in 1..SHIPSIM_TREE_MAX_WORKERS.
 *
 * shipsim_tree_init writes the one-node tree: the root, node 0, and zero counters.
 *
 * shipsim_tree_select sends W interchangeable workers down the tree, "one after the other from the root, each seeing
 * the virtual visits of those before it". The t-th worker (t = 0, 1, ...) to arrive at node v in this call:
 *   - stays at v if v is terminal or depth(v) == max_depth (0..SHIPSIM_TREE_MAX_DEPTH); otherwise, with
 *     m = n_children(v) + the children being created at v in this call and N = visits(v) + t,
 *   - widens v iff m < C and (u64)m * m * wden < (u64)wnum * (N + 1), that is m < k * sqrt(N + 1) with
 *     k^2 = wnum / wden (both in 1..2^15), and is then counted among the children being created;
 *   - otherwise stays at v if v has no child;
 *   - otherwise goes to the child a of the largest score, ties to the lowest child slot, and counts as arrived at a:
 *       Q_a   = visits(a) > 0 ? ldexp((double)value_sum(a) / (double)visits(a), -24) : 0.0
 *       score = Q_a + (c_explore * sqrt((double)(N + 1))) / (double)(1 + visits(a) + arrived_a)
 *     five IEEE operations in this order, without contraction. Children being created in this call are no candidates.
 * Output: nodes by increasing id; per node its staying workers, then its widening ones. Worker w starts from the
 * state of node leaf_out[w] and creates a child there iff expand_out[w] == 1. The tree is not written.
 *
 * shipsim_tree_expand takes select's leaf and expand arrays (the widening workers of one node adjacent, as select
 * emits them) and an action per worker. The widening workers get the ids n_nodes + rank in worker order; a new node
 * has its parent, depth + 1, action[w] and zero statistics, and is appended to its parent's child[] in worker order;
 * n_nodes advances. An id >= max_nodes is dropped: node_out[w] = -1 and dropped += 1 (as for a widening worker whose
 * leaf names no node or no free child slot). Every other worker gets node_out[w] = leaf[w].
 *
 * shipsim_tree_backup adds one value along the whole path: q = (int64)nearbyint(ldexp(value[w], 24)) clamped to
 * +-2^40, and every node from node[w] up to the root gets visits += 1 and value_sum += q (integer atomics: the
 * result does not depend on the order). A worker with node[w] outside the tree (-1: dropped) or a non-finite value is
 * skipped: skipped += 1. terminal (may be NULL): terminal[w] != 0 ORs the terminal bit into node[w].
 *
 * SHIPSIM_EINVAL, before any device call: a NULL tree, workspace or required array; sizes out of range;
 * tree_bytes != shipsim_tree_bytes(...); a tree or workspace not 16-byte aligned; a workspace too small; c_explore
 * negative or not finite. The arithmetic is ast_sac_amd/csrc/shipsim_tree_host.hpp, restated in tests/tree_ref.py.
 *
 * A forest is R = n_roots roots in one node pool, sharing one archive and one round of calls: nodes 0..R-1, each with
 * parent -1, depth 0, action 0 and no children. Everything under a root is a tree as above: R trees of one problem
 * (root-parallel search), or one tree per weather when root r is the reset state of env r under env r's weather.
 *
 * shipsim_tree_init_forest writes n_nodes = n_roots, hdr[3] = n_roots, zero counters and the R roots
 * (1 <= n_roots <= max_nodes).
 *
 * shipsim_tree_select_forest is shipsim_tree_select with the R roots, not node 0, as where the workers start.
 * root_workers is a device array of n_roots int32, the workers asked for per root; the roots are served in id order
 * until the W workers are used up: root r receives
 *     a_r = min(max(c_r, 0), W - min(W, sum over r' < r of max(c_r', 0)))
 * arrivals (the sum formed with adds that saturate at W, so the result is defined whatever the array holds) and routes
 * them exactly as the root of a tree routes its W. It serves min(n_roots, the header's roots, n_nodes) roots. The
 * output order is select's: by increasing node id, a node's staying workers before its widening ones. When the a_r sum
 * to less than W, the trailing workers get leaf_out[w] = -1 and expand_out[w] = 0: shipsim_tree_expand passes them
 * through (node_out[w] = -1) and shipsim_tree_backup counts them as skipped. With n_roots = 1 and root_workers = {W} it
 * returns what shipsim_tree_select returns. Refused with SHIPSIM_EINVAL, beside everything shipsim_tree_select
 * refuses: n_roots < 1, n_roots > max_nodes, n_roots > n_workers (level 0 holds a root per worker at the most), a NULL
 * root_workers.
 *
 * shipsim_tree_expand and shipsim_tree_backup serve a forest as they are: expand does not know roots, and backup
 * walks up to the node whose parent is -1. */
#define SHIPSIM_TREE_MAX_CHILDREN 64
#define SHIPSIM_TREE_MAX_DEPTH 32
#define SHIPSIM_TREE_MAX_WORKERS (1 << 22)
#define SHIPSIM_TREE_SCAN_TILE 1024 /* nodes numbered by one block of select's scan */
#define SHIPSIM_TREE_LAYOUT_FIELDS 10
int64_t shipsim_tree_bytes(int32_t max_nodes, int32_t max_children);
int shipsim_tree_layout(int32_t max_nodes, int32_t max_children, int64_t* offsets_out);
int64_t shipsim_tree_workspace_bytes(int32_t max_nodes, int32_t n_workers);
int shipsim_tree_init(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, void* stream);
int shipsim_tree_select(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                        int32_t n_workers, int32_t max_depth, int32_t wnum, int32_t wden, double c_explore,
                        void* workspace, int64_t workspace_bytes, int32_t* leaf_out, int32_t* expand_out, void* stream);
int shipsim_tree_expand(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_workers,
                        const int32_t* leaf, const int32_t* expand, const float* action, void* workspace,
                        int64_t workspace_bytes, int32_t* node_out, void* stream);
int shipsim_tree_backup(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_workers,
                        const int32_t* node, const double* value, const uint8_t* terminal, void* stream);
int shipsim_tree_init_forest(void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children, int32_t n_roots,
                             void* stream);
int shipsim_tree_select_forest(const void* tree, int64_t tree_bytes, int32_t max_nodes, int32_t max_children,
                               int32_t n_workers, int32_t n_roots, const int32_t* root_workers, int32_t max_depth,
                               int32_t wnum, int32_t wden, double c_explore, void* workspace, int64_t workspace_bytes,
                               int32_t* leaf_out, int32_t* expand_out, void* stream);

/* ---- trajectory recording (f1: simulation_results export) ----------------------------------
 * Per-tick rows of ShipModelAST/SimpleShipModel.store_simulation_data (ship_model.py:903-957,
 * run_colav/.../ship_model.py:418-444) for both ships, plus the RewardTracker entry of every tick
 * (reward_function.py:30-57, 181-186) and the animation lists of env.py:612-620. Row t of a ship is its
 * t-th store since the env's last reset (row 0 = init_step, env.py:329); env row t belongs to tick
 * t + 1. Values are raw (SI units, radians); the Python facade derives the reference's keys and units.
 * Ship row columns: */
#define SHIPSIM_TRAJ_SHIP_COLS 20
#define SHIPSIM_TS_TIME 0       /* int.time at the store */
#define SHIPSIM_TS_NORTH 1
#define SHIPSIM_TS_EAST 2
#define SHIPSIM_TS_YAW 3        /* rad */
#define SHIPSIM_TS_RUDDER 4     /* rad */
#define SHIPSIM_TS_U 5
#define SHIPSIM_TS_V 6
#define SHIPSIM_TS_R 7          /* rad/s */
#define SHIPSIM_TS_OMEGA 8      /* propeller shaft speed rad/s (detailed) */
#define SHIPSIM_TS_THRUST 9     /* N: propeller thrust (detailed) | commanded thrust force (simplified) */
#define SHIPSIM_TS_E_CT 10      /* auto_pilot.get_cross_track_error() */
#define SHIPSIM_TS_E_PSI 11     /* auto_pilot.get_heading_error() = |heading_mea - heading_ref| (rad, Q8) */
#define SHIPSIM_TS_LOAD 12      /* engine throttle = load_perc (detailed) | thrust command (simplified) */
#define SHIPSIM_TS_FUEL_ME 13   /* accumulated fuel kg (detailed; machinery int.dt, Q1) */
#define SHIPSIM_TS_FUEL_EL 14
#define SHIPSIM_TS_FUEL 15
#define SHIPSIM_TS_E_CT_INT 16  /* navigate.e_ct_int after the tick (ShipAssets.integrator_term) */
#define SHIPSIM_TS_NEXT_WPT 17
#define SHIPSIM_TS_REPEAT 18    /* 1: store_last_simulation_data row of a stopped ship */
#define SHIPSIM_TS_TIME_LIST 19 /* ShipAssets.time_list entry of the tick */
/* Env row columns: */
#define SHIPSIM_TRAJ_ENV_COLS 8
#define SHIPSIM_TE_R_COLLISION 0      /* RewardTracker.ship_collision (already / 5) */
#define SHIPSIM_TE_R_TEST_GROUNDING 1
#define SHIPSIM_TE_R_TEST_NAV 2
#define SHIPSIM_TE_R_OBS_GROUNDING 3
#define SHIPSIM_TE_R_OBS_NAV 4
#define SHIPSIM_TE_R_TOTAL 5          /* RewardTracker.total (after the termination multipliers) */
#define SHIPSIM_TE_BITS 6             /* SHIPSIM_EV_* bits of the tick */
#define SHIPSIM_TE_FLAGS 7            /* SHIPSIM_TE_FLAG_* */
#define SHIPSIM_TE_FLAG_COLLISION 1   /* is_collision_list entry */
#define SHIPSIM_TE_FLAG_IMMINENT 2    /* is_collision_imminent_list entry (simple: distance, sbmpc: active) */

/* Enable recording into caller-owned device buffers: ship_rows n_envs*n_ships x capacity x
 * SHIPSIM_TRAJ_SHIP_COLS doubles ([env][ship][row][col]), env_rows n_envs x capacity x
 * SHIPSIM_TRAJ_ENV_COLS doubles (may be NULL), lengths n_envs int32 (ship rows recorded since the env's
 * last reset; rows past capacity are dropped while the count goes on). Lengths are zeroed here and by
 * every reset; enable before the reset that starts the episodes to record. ship_rows NULL disables.
 * AST kind only; recording steps run the lanes_per_env = 16 kernels (identical results). */
int shipsim_set_trajectory(shipsim_handle* h, double* ship_rows, double* env_rows, int32_t capacity,
                           int32_t* lengths);

/* SBMPC.get_optimal_ctrl_offset (sbmpc.py:113-185) for n independent single-obstacle requests on the
 * device, stateless (P_ca_last_ / Chi_ca_last_ are inputs). in: n x SHIPSIM_SBMPC_IN doubles
 * [P_ca_last, Chi_ca_last, u_d, chi_d, os_state(6: x, y, psi, u, v, r), obstacle(5: x, y, psi, u, v),
 *  obstacle length, obstacle width]; out: n x 3 doubles [speed factor, course offset, active].
 * SBMPC(tf, dt) horizon; stream is a hipStream_t (NULL = default); device pointers. */
#define SHIPSIM_SBMPC_IN 17
int shipsim_sbmpc_eval(int32_t n, double tf, double dt, const double* in, double* out, void* stream);

/* The test by which the two-ship decision streams (collav sbmpc) answer a request without the optimiser's pass, for
 * n of shipsim_sbmpc_eval's request rows (additive to ABI 12): flag_out[i] = 1 where the nominal scenario (speed
 * factor 1, course offset 0) provably wins request i — the memory at (1, 0) and a closed-form upper bound on that
 * scenario's collision cost below every other scenario's own terms (ast_sac_amd/csrc/shipsim_sbmpc_nominal.hpp) —
 * else 0. For such a row shipsim_sbmpc_eval returns (1.0, 0.0, active). The D_INIT test of the request is not part
 * of it. flag_out[i] holds two bits: bit 0 the test with the sine and cosine of chi_d; bit 1 the form the streams'
 * tick evaluates (sbmpc_nominal_holds_seg: the course as a segment angle's sine and cosine with the argument of the
 * LOS correction, no atan), on the split of chi_d that sbmpc_nominal_split_course defines. The two agree except
 * within rounding of the decision. Device pointers (flag_out: n int32); stateless, asynchronous on `stream`. */
int shipsim_sbmpc_nominal(int32_t n, double tf, double dt, const double* in, int32_t* flag_out, void* stream);

/* The three math-library calls of the two-ship decision streams' steady tick, for n arguments (additive to ABI 12):
 * fn 0 sincos, 1 atan, 2 exp. out: n x 6 doubles per argument — the device library's value, the restated form's
 * (ast_sac_amd/csrc/shipsim_tickmath.hpp, constants as literals) and the form the headline kernel runs (the table
 * stream with collav sbmpc at 16 lanes per env: constants by row broadcast), two doubles each: (sine, cosine) for fn 0, (value, 0) otherwise. The three agree bit for bit. Device
 * pointers; stateless, asynchronous on `stream`. */
int shipsim_tickmath_eval(int32_t fn, int32_t n, const double* in, double* out, void* stream);

/* SBMPC.get_optimal_ctrl_offset (sbmpc.py:113-185) over a do_list of n_obs dynamic obstacles (1 <= n_obs <=
 * SHIPSIM_MAX_OBS; active when any of them is within D_INIT, per scenario the worst obstacle's cost, the least worst
 * scenario: :149-178) for n independent requests, stateless like shipsim_sbmpc_eval (ABI 10). in: n x
 * SHIPSIM_SBMPC_MULTI_IN doubles [P_ca_last, Chi_ca_last, u_d, chi_d, os_state(6: x, y, psi, u, v, r), then per
 * obstacle slot k < SHIPSIM_MAX_OBS: x, y, psi, u, v, length, width (the do_list tuple's state and size; slots
 * k >= n_obs are ignored)]; out: n x 3 doubles [speed factor, course offset, active]. The optimiser is the one the
 * multi-obstacle env kernels (n_obs_ships > 1) run. Replaces, per request, one call of the reference method with a
 * do_list of n_obs entries. */
#define SHIPSIM_SBMPC_MULTI_IN (10 + 7 * SHIPSIM_MAX_OBS)
int shipsim_sbmpc_eval_multi(int32_t n, int32_t n_obs, double tf, double dt, const double* in, double* out,
                             void* stream);

/* Diagnostics: the kernels' division by a reused divisor (the divisor's refined reciprocal formed once, the rest of
 * the compiler's fp64 division sequence per quotient) next to the plain IEEE division, for n operand
 * pairs: fast[i] = num[i] / den[i] as the kernels form it, ref[i] = num[i] / den[i]. Device pointers (n doubles
 * each); stream a hipStream_t (NULL = default). The two agree bit for bit for operands away from the ends of the
 * exponent range (tests/test_gpu_div_identity.py). */
int shipsim_div_check(int32_t n, const double* num, const double* den, double* fast, double* ref, void* stream);

/* ---- open-loop decision stream (the C3 workload of SURVEY.md §8(d)) -------------------------
 * Every env draws the scoping angle (radians, already denormalised) of decision d of its episode e from
 * table[((e % n_eps) * n_dec + d) * n_envs + env] and runs decisions back to back inside the call: a
 * completed decision (MultiShipRLEnv.step, env.py:624-773) is followed at once by the next one, and an
 * episode that ends — done, or n_dec decisions (the rollout's max_path_length, rollout_functions.py:
 * 106-160) — is reset in place (reset + init_step, env.py:238-342) before its next decision. Each env
 * runs at most max_ticks (>= 1) _step ticks per call; an env paused mid-decision resumes in the next
 * call. Results are those of shipsim_step / shipsim_reset driven by the same table.
 *   ep_idx, dec_idx  N int32 (device, in/out): episode counter and decision index of every env
 *   ticks_out        N int32: _step ticks run in this call (may be NULL)
 *   decisions_out    N int32: decisions completed in this call (may be NULL)
 *   log              N x log_cap x SHIPSIM_DECLOG_COLS doubles: one record per completed decision
 *                    (may be NULL); log_len N int32 (in/out) counts records (past log_cap too). */
#define SHIPSIM_DECLOG_COLS 23
#define SHIPSIM_DL_REWARD 0   /* accumulated (un-scaled) reward of the decision */
#define SHIPSIM_DL_EVENTS 1   /* SHIPSIM_EV_* bits */
#define SHIPSIM_DL_DONE 2     /* combined_done */
#define SHIPSIM_DL_EPISODE 3  /* ep_idx of the decision */
#define SHIPSIM_DL_DECISION 4 /* dec_idx of the decision */
#define SHIPSIM_DL_TICKS 5    /* _step ticks of the decision (across launches; 0 for a sampling failure) */
#define SHIPSIM_DL_OBS 6      /* 8 columns: the observation returned */
#define SHIPSIM_DL_ACTION 14  /* shipsim_run_policy only: the policy's normalized action a */
#define SHIPSIM_DL_OBS0 15    /* shipsim_run_policy only, 8 columns: the observation a was chosen from */
/* (shipsim_run_table leaves columns 14..22 as they were: its actions are the caller's table) */
int shipsim_run_table(shipsim_handle* h, const float* table, int32_t n_eps, int32_t n_dec, int32_t max_ticks,
                      int32_t* ep_idx, int32_t* dec_idx, int32_t* ticks_out, int32_t* decisions_out, double* log,
                      int32_t log_cap, int32_t* log_len);

/* The same decision stream with the collector's policy in the loop (ABI 7; also new in 7: the 23-column decision record): every decision's action is
 * sampled inside the launch from the observation the env returned, by the TanhGaussianPolicy
 * (gaussian_policy.py:105-118: fc0, relu, fc1, relu, mean / clamped log_std heads) then TanhNormal.sample
 * (distributions.py:394-425: tanh(mean + std * eps), eps ~ N(0, 1)) or, deterministic != 0,
 * MakeDeterministic's tanh(mean) (policies/base.py:54-64), and denormalized as NormalizedBoxEnv does
 * (normalized_box_env.py:48-51) — the rollout loop of rollout_functions.py:53-91 for every env at once,
 * without a host round trip. fp32 as the policy; the env in fp64.
 *   policy   the policy's parameters in torch order (fcs[0].weight [H][obs_dim], .bias, fcs[1].weight
 *            [H][H], .bias, last_fc.weight [1][H], .bias, last_fc_log_std.weight, .bias), device
 *   w2t      fcs[1].weight transposed ([H][H], w2t[k][u] = W2[u][k]), device (sacf_policy_weights)
 *   obs_dim  8; hidden a multiple of 64 up to 512
 *   seed, counter  the noise: eps of env i's s-th decision of a call is Philox4x32-10 keyed by seed on
 *            {i, *counter (64 bits), 0x5A100000 ^ s} then Box-Muller; *counter is read, not changed —
 *            advance it between calls (ignored when deterministic; counter may then be NULL)
 *   n_dec    decisions per episode (max_path_length); other arguments as shipsim_run_table, and the
 *            decision record's SHIPSIM_DL_ACTION column holds the normalized action a in (-1, 1).
 *            With a log, an env stops for the launch once it holds log_cap records (log_len starts where
 *            the caller left it), its next decision pending for the next call: no record is lost.
 * K obstacle ships as for shipsim_run_table (ABI 11): K > 1 with the detailed machinery and collav none or sbmpc,
 * as shipsim_create requires. SHIPSIM_EINVAL for a bad obs_dim / hidden. */
int shipsim_run_policy(shipsim_handle* h, const float* policy, const float* w2t, int32_t obs_dim, int32_t hidden,
                       int32_t deterministic, uint64_t seed, const int64_t* counter, int32_t n_dec,
                       int32_t max_ticks, int32_t* ep_idx, int32_t* dec_idx, int32_t* ticks_out,
                       int32_t* decisions_out, double* log, int32_t log_cap, int32_t* log_len);

/* Work-conserving launch tail of the decision streams (shipsim_run_table / shipsim_run_policy; ABI 8): a wave
 * whose envs all met max_ticks keeps ticking, 32 ticks at a time, while any wave of the same launch has not, up to
 * extra_ticks more (0, the default: off). Per-env results do not change (a decision stream is exact whatever its
 * launch boundaries); ticks_out / decisions_out then exceed max_ticks by up to extra_ticks for the envs of the
 * faster waves. Used only when every wave of the launch is resident at once (otherwise the launch runs as with 0),
 * and for one obstacle ship per env (the K > 1 streams run as with 0). */
int shipsim_set_stream_tail(shipsim_handle* h, int32_t extra_ticks);

/* Grouping of the decision streams' envs into waves by episode phase (additive to ABI 12). The
 * stream kernels run several envs per wave, and a wave's SBMPC pass stalls all of them while it serves at most two
 * requests; envs whose episodes are out of phase request on different ticks and every pass serves one. In front of
 * every shipsim_run_table / shipsim_run_policy launch a small kernel on the handle's stream therefore orders the
 * envs by the ticks since their last reset (the test ship's clock over the time step; ties by env index) and the
 * launch's slot s runs env slot_env[s], so wave-mates meet their obstacle on the same ticks again. Per-env results
 * do not change, bit for bit: an env's records do not depend on its wave-mates. No host readback or
 * synchronisation (graph-capturable). Handles of up to 65536 envs; larger ones run slot = env whatever the switch
 * says, and shipsim_step and the recording kernels always do. shipsim_create leaves the switch on for two-ship envs
 * with collav sbmpc (the headline stream: +2.7 %) and off otherwise: collav none / simple never run a pass, and the
 * K > 1 streams have no launch tail to absorb the unlike amounts of work of waves of unlike phase (K = 2 measured
 * slower with grouping, K = 4 faster).
 *   shipsim_set_stream_grouping  on != 0: group; 0: slot = env, from the next launch on.
 *   shipsim_get_stream_grouping  slot_env_out: n_envs int32 (host or device), the last stream launch's permutation
 *                                (the identity before the first and after a launch with grouping off), copied on
 *                                the handle's stream. SHIPSIM_EINVAL for a handle that holds none. */
int shipsim_set_stream_grouping(shipsim_handle* h, int32_t on);
int shipsim_get_stream_grouping(shipsim_handle* h, int32_t* slot_env_out);

/* ---- per-env weather (ABI 12) ---------------------------------------------------------------
 * By default every env of a handle runs the config's weather (wind_speed, wind_direction,
 * current_velocity_component_from_north / _from_east). shipsim_set_weather gives every env its own: four HOST
 * arrays of n_envs doubles (m/s, rad, m/s, m/s) — a setup call like the config, not a per-step one. The library
 * takes sin and cos of the direction on the host (the libm calls shipsim_create makes for the config's direction),
 * copies the arrays, uploads on the handle's stream and waits for the upload: do not call it during graph capture
 * (the first call also allocates the device table and the staging table of shipsim_weather_fork).
 * From the next launch on shipsim_reset, shipsim_step, shipsim_run_table and shipsim_run_policy (in-kernel resets
 * included) run env i under its values, with the results, bit for bit, of a uniform handle whose config carries
 * them. The values persist across resets until set again.
 *   - four NULL pointers: back to the config's weather (and the uniform kernels); a mix of NULL and non-NULL,
 *     a non-finite value or a negative wind speed: SHIPSIM_EINVAL, and nothing changes.
 *   - AST kind, detailed machinery, collav none / sbmpc, K = 1..4 obstacle ships, no trajectory recording:
 *     anything else is SHIPSIM_EINVAL with the reason in shipsim_last_error, as are shipsim_set_trajectory and
 *     shipsim_legacy_step on a handle with per-env weather. (A recorded replay of env i: a uniform handle whose
 *     config carries env i's values.)
 *   - the weather kernels exist at 8 and 16 lanes per env (two-ship envs; 16 for K > 1): a handle whose automatic
 *     or requested lanes_per_env is 2 or 4 runs at 8 while per-env weather is set, and shipsim_lanes_per_env
 *     reports what runs (results do not depend on it).
 * shipsim_get_weather fills four host arrays of n_envs doubles with what was set, or with the config's values on
 * a handle without per-env weather. */
int shipsim_set_weather(shipsim_handle* h, const double* wind_speed, const double* wind_direction,
                        const double* current_from_north, const double* current_from_east);
int shipsim_get_weather(shipsim_handle* h, double* wind_speed, double* wind_direction,
                        double* current_from_north, double* current_from_east);

/* ---- per-env weather that moves with the state: store, load, fork (additive to ABI 12) ----------------------
 * Weather is not part of the state block, so shipsim_fork, shipsim_restore and shipsim_archive_load leave every slot's
 * weather where it is. These calls move it, by the index arrays those calls take, so that a clone goes on under the
 * weather that shaped its past. The handle's weather table on the device is six rows of n_envs doubles: wind speed,
 * sin and cos of the wind direction (what the kernels read), current from north, current from east, and the wind
 * direction as set (which its sin and cos do not give back bit for bit). A weather buffer is a caller-owned device
 * buffer, 16-byte aligned, of six such rows of n_slots doubles, row r at byte r * n_slots * 8:
 * shipsim_weather_bytes(n_slots) bytes (SHIPSIM_EINVAL outside 1..SHIPSIM_ARCHIVE_MAX_CELLS); with n_slots == n_envs
 * it is byte for byte the handle's table.
 *   shipsim_weather_store  slot c takes the weather of env env_of_slot[c] (n_slots int32 on the device). NULL: the
 *                          identity, n_slots == n_envs only — a weather snapshot.
 *   shipsim_weather_load   env i takes the weather of slot slot_of_env[i] (n_envs int32 on the device), written
 *                          straight into the handle's table. NULL: the identity, n_slots == n_envs only — a restore;
 *                          with n_slots == n_envs and an index, a fork from a snapshot. Values are not validated: a
 *                          buffer holds what shipsim_weather_store wrote, and loading a slot never stored is the
 *                          caller's error as loading an empty cell of a state archive is (defined, no fault).
 *   shipsim_weather_fork   env i takes the weather env src_env[i] had before the call (n_envs int32 on the device;
 *                          NULL: the identity): gathered into a library-owned staging table and copied back, one
 *                          launch and one copy, as shipsim_fork does with the state.
 * An index that names no slot of the source leaves the destination slot as it is; the kernel tests the index before
 * it forms an address from it, its loads are gathered and its stores consecutive, and there are no atomics, so
 * duplicate indices are harmless. All are asynchronous on the handle's stream, without host synchronisation or
 * allocation (shipsim_set_weather allocated the table and the staging table), and may be captured into a graph from
 * the first call on; the table never moves, so captured env launches stay valid.
 * shipsim_get_weather follows: once one of the three has been called on a handle (during a capture too — a replay
 * moves weather without a host call), it waits for the handle's stream and reads the four arrays back from the
 * device table. On a handle that never called one it returns the host copy of what was set, as before.
 * SHIPSIM_EINVAL with the reason in shipsim_last_error: a handle without per-env weather in force; a NULL buffer;
 * n_slots outside 1..SHIPSIM_ARCHIVE_MAX_CELLS; bytes != shipsim_weather_bytes(n_slots); a buffer not 16-byte
 * aligned; a NULL index with n_slots != n_envs. */
int64_t shipsim_weather_bytes(int32_t n_slots);
int shipsim_weather_store(shipsim_handle* h, void* wx, int64_t bytes, int32_t n_slots, const int32_t* env_of_slot);
int shipsim_weather_load(shipsim_handle* h, const void* wx, int64_t bytes, int32_t n_slots,
                         const int32_t* slot_of_env);
int shipsim_weather_fork(shipsim_handle* h, const int32_t* src_env);

/* ---- legacy per-tick MultiShipEnv (rl_env/ship_in_transit/env.py:783-1181) ----
 * AST kind. Each of the k ticks is one MultiShipEnv.step() (:1104-1173) of every env: test_step
 * (:923-1023, SBMPC / simple collision avoidance as configured) + obs_step (:1025-1102) +
 * get_termination_status (evaluation/termination_flags.py:5-70). No intermediate waypoints, no reward.
 * Envs start from shipsim_reset (MultiShipEnv.reset/init_step, :855-921 — same placement as the RL
 * reset); the simple collision check reads the previous step's next_states (the float32
 * initial_states before the first step after create), which survive reset, as in the reference.
 * An env whose step reports done stops ticking for the rest of the call (k = 1: the reference's
 * per-call semantics). Outputs of the env's last tick (device, each may be NULL):
 *   states  N x 8 doubles: next_states [test n, e, e_ct, obs n, e, yaw, speed, e_ct]
 *   done    N uint8: test reached/outside/grounded/nav failure, collision, obs grounded/nav failure
 *   status  N uint32: bit i = termination_conditions[i] (SHIPSIM_LT_*) */
#define SHIPSIM_LT_TEST_REACHED (1u << 0)
#define SHIPSIM_LT_TEST_OUTSIDE (1u << 1)
#define SHIPSIM_LT_TEST_GROUNDED (1u << 2)
#define SHIPSIM_LT_TEST_NAV_FAILURE (1u << 3)  /* |e_ct| > 500 */
#define SHIPSIM_LT_NEAR_COLLISION (1u << 4)    /* distance < 3000 m */
#define SHIPSIM_LT_COLLISION (1u << 5)         /* distance < 50 m */
#define SHIPSIM_LT_OBS_REACHED (1u << 6)
#define SHIPSIM_LT_OBS_OUTSIDE (1u << 7)
#define SHIPSIM_LT_OBS_GROUNDED (1u << 8)
#define SHIPSIM_LT_OBS_NAV_FAILURE (1u << 9)
int shipsim_legacy_step(shipsim_handle* h, int32_t k, double* states_out, uint8_t* done_out, uint32_t* status_out);

/* Block until all work queued on the handle's stream is done. Returns SHIPSIM_ENONFINITE (message in
 * shipsim_last_error) when env decisions ended on a non-finite ship state since the previous call. */
int shipsim_synchronize(shipsim_handle* h);
/* Decisions flagged SHIPSIM_EV_NONFINITE since create, as of the last shipsim_synchronize. */
int32_t shipsim_nonfinite_count(const shipsim_handle* h);
/* Diagnostics builds only (-DSHIPSIM_LANECHECK): out32 = {violations, first site, its exec mask lo, hi,
 * 0 x 4, violations of site 0..15 x 16, 0 x 8} of the cross-lane / index checks since the last call (then
 * cleared; synchronizes the current device). SHIPSIM_EINVAL (out32 zeroed) in the default build, which
 * compiles the checks out. */
int shipsim_diag_lane_faults(uint32_t* out32);

#ifdef __cplusplus
}
#endif
#endif /* SHIPSIM_H */
