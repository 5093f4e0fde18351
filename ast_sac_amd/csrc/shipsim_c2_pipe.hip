// shipsim_c2_pipe.hip — the C2 three-wave kernel and its launch: libshipsim's second object. It is compiled with
// machine-level LICM, which shipsim_kernels.hip's object is built without (ast_sac_amd/build_hash.py OBJECTS): the
// kernel's three short loops have registers to spare, and hoisting the fp64 constants of atan / sincos out of the
// tick loop shortens the tick.
#include <hip/hip_runtime.h>

#include "shipsim.h"
#include "shipsim_device.hpp"
#include "shipsim_state.hpp"

using namespace shipsim;


// C2 with the simplified machinery (the C2 configuration, SimpleShipModel + ThrustFromSpeedSetPoint): the same ticks
// as single_tick_kernel<false>, bit for bit, on THREE waves per 64 ships, software-pipelined so that one workgroup
// barrier per tick separates them. A tick t only needs, besides its own (u, v, r):
//   sin/cos ψ_t    — ψ_t = ψ_{t-1} + r_{t-1} dt is known one tick early;
//   the rudder_t   — waypoint switch, LOS guidance (sqrt, divide, atan) and heading PID on (n, e, ψ)_t, which follow
//                    from tick t - 1's state by the explicit Euler step before tick t - 1's kinetics matter.
// So in interval t
//   wave 0 (guidance): (n, e, ψ)_{t+1} from (u, v, r)_t and sin/cos ψ_t, then the rudder of tick t + 1;
//   wave 1 (heading):  ψ_{t+1} and sin/cos ψ_{t+1};
//   wave 2 (dynamics): tick t's thrust (speed PID), wind force and kinetics -> (u, v, r)_{t+1};
// each reading what the others wrote in interval t - 1 (LDS, double-buffered by tick parity). Every value is formed
// by the same expression as in the one-wave tick (control_and_store, differentials, integrate): the same bits.
template <bool POW2_DT>  // dt a power of two: the PIDs' derivative division as the exact multiplication (pid)
__global__ __launch_bounds__(192) void single_tick_pipe_kernel(const Params P, DevState S, ConstBuf K, int k) {
  __shared__ ShipConst lds_sc[SHIPSIM_MAX_SHIPS];
  __shared__ double x_uvr[2][3][64];  // (u, v, r) of a tick, by tick parity
  __shared__ double x_sc[2][2][64];   // sin / cos ψ of a tick
  __shared__ double x_rud[2][64];     // rudder of a tick
  const ShipConst* SC = stage_consts(K, lds_sc, P.n_ships, P.dt);
  const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;  // (wave-uniform)
  const int q0 = blockIdx.x * 64 + lane, q = min(q0, P.n_envs - 1);  // (every lane takes part in the barriers)
  const bool live = q0 < P.n_envs;
  const ShipConst& c = SC[0];
  const double dt = P.dt, inv_dt = pow2_inverse(dt);  // (the PIDs' derivative terms: see pid)
  Ship s;
  load_ship(S, q, s);
  // the kinematic rates of integrate's Euler step (differentials_body's expressions)
  auto advance_pose = [&](double u, double v, double r, double sy, double cy) __attribute__((always_inline)) {
    // (the rotation's structural zero terms dropped: a ±0 addend leaves every non-zero rate's bits as they are)
    const double dn = cy * u + (-sy) * v;
    const double de = sy * u + cy * v;
    const double dyaw = r;
    s.n = s.n + dn * dt;
    s.e = s.e + de * dt;
    s.yaw = s.yaw + dyaw * dt;
  };
  if (role == 0) {
    // guidance: the rudder of tick j from (n, e, ψ)_j — control_and_store's route half (DETAILED false, no collav)
    const double* rn = S.route_n() + (size_t)q * kMaxRoute;
    const double* re = S.route_e() + (size_t)q * kMaxRoute;
    auto guide = [&]() __attribute__((always_inline)) {
      const double N = s.n, E = s.e, H = s.yaw;
      if (next_wpt_advance(c, s, N, E)) {
        s.next_wpt += 1;
        load_segment(s, rn, re);
      }
      const double href = los_guidance(c, s, N, E);
      const double rudder = heading_ctrl<POW2_DT>(c, s, href + 0.0, H, dt, POW2_DT ? inv_dt : c.rcp_dt);
      s.log_rudder = rudder;
      s.log_ect = s.e_ct;
      s.log_n = N;
      s.log_e = E;
      return rudder;
    };
    x_rud[0][lane] = guide();
    __syncthreads();
    for (int t = 0; t < k; ++t) {
      const int b = t & 1;
      advance_pose(x_uvr[b][0][lane], x_uvr[b][1][lane], x_uvr[b][2][lane], x_sc[b][0][lane], x_sc[b][1][lane]);
      if (t + 1 < k) x_rud[b ^ 1][lane] = guide();
      __syncthreads();
    }
    if (live) {
      S.f(SF_N)[q] = s.n; S.f(SF_E)[q] = s.e; S.f(SF_YAW)[q] = s.yaw;
      S.f(SF_ECT)[q] = s.e_ct; S.f(SF_ECT_INT)[q] = s.e_ct_int;
      S.f(SF_HDG_EI)[q] = s.hdg_ei; S.f(SF_HDG_PREV)[q] = s.hdg_prev;
      S.f(SF_RUDDER)[q] = s.log_rudder; S.f(SF_LOG_ECT)[q] = s.log_ect;
      S.f(SF_LOG_N)[q] = s.log_n; S.f(SF_LOG_E)[q] = s.log_e;
      S.next_wpt()[q] = s.next_wpt;
    }
  } else if (role == 1) {
    // heading: sin/cos ψ of the next tick (differentials' sincos(s.yaw))
    double sy, cy;
    sincos(s.yaw, &sy, &cy);
    x_sc[0][0][lane] = sy; x_sc[0][1][lane] = cy;
    __syncthreads();
    for (int t = 0; t < k; ++t) {
      const int b = t & 1;
      const double r = x_uvr[b][2][lane];
      s.yaw = s.yaw + r * dt;  // (advance_pose's ψ rate)
      if (t + 1 < k) {
        sincos(s.yaw, &sy, &cy);
        x_sc[b ^ 1][0][lane] = sy; x_sc[b ^ 1][1][lane] = cy;
      }
      __syncthreads();
    }
  } else {
    // dynamics: tick t's thrust, wind force and kinetics (control_and_store's speed half, differentials, integrate)
    double wsin, wcos;
    sincos(P.wind_dir, &wsin, &wcos);
    x_uvr[0][0][lane] = s.u; x_uvr[0][1][lane] = s.v; x_uvr[0][2][lane] = s.r;
    __syncthreads();
    for (int t = 0; t < k; ++t) {
      const int b = t & 1;
      const double sy = x_sc[b][0][lane], cy = x_sc[b][1][lane], rudder = x_rud[b][lane];
      const double thrust = speed_ctrl<POW2_DT>(c, s, c.desired_speed * 1.0, s.u, dt, false, POW2_DT ? inv_dt : c.rcp_dt);
      s.log_thrust = thrust;
      double tau[3];
      wind_force_alg(c, P, s, sy, cy, wsin, wcos, tau);
      const Deriv d = differentials_body(c, P, s, thrust, rudder, false, sy, cy, tau);
      s.u = s.u + d.du * dt;
      s.v = s.v + d.dv * dt;
      s.r = s.r + d.dr * dt;
      s.time = s.time + dt;
      x_uvr[b ^ 1][0][lane] = s.u; x_uvr[b ^ 1][1][lane] = s.v; x_uvr[b ^ 1][2][lane] = s.r;
      __syncthreads();
    }
    if (live) {
      S.f(SF_U)[q] = s.u; S.f(SF_V)[q] = s.v; S.f(SF_R)[q] = s.r; S.f(SF_TIME)[q] = s.time;
      S.f(SF_SPD_A)[q] = s.spd_a; S.f(SF_SPD_B)[q] = s.spd_b; S.f(SF_THRUST)[q] = s.log_thrust;
    }
  }
}

void shipsim_c2_pipe_launch(int blocks, hipStream_t st, const Params& P, const DevState& S, const ConstBuf& K, int k) {
  if (pow2_inverse(P.dt) != 0.0)
    hipLaunchKernelGGL(single_tick_pipe_kernel<true>, dim3(blocks), dim3(192), 0, st, P, S, K, k);
  else
    hipLaunchKernelGGL(single_tick_pipe_kernel<false>, dim3(blocks), dim3(192), 0, st, P, S, K, k);
}
