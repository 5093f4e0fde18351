// shipsim_state.hpp — what both objects of libshipsim share of the device state: the state block (DevState) and the
// constant block (ConstBuf) as the kernels address them, a ship's load / store between the block and registers, the
// staging of the per-ship constants into LDS, and the launch of the C2 pipe kernel (shipsim_c2_pipe.hip), which
// shipsim_kernels.hip calls.
#pragma once
#include <hip/hip_runtime.h>

#include "shipsim_device.hpp"
#include "shipsim_state_host.hpp"  // the state block as a table of columns (snapshot / restore / fork)

using namespace shipsim;


// ---------------------------------------------------------------------------------------------
// device state (SoA). Ship arrays are indexed q = env * n_ships + ship (lane order).
// ---------------------------------------------------------------------------------------------
struct DevState {
  // One device block; every array lives at base + (index * stride). Keeping the table as one base
  // pointer + strides (instead of ~40 pointers) keeps it out of the SGPR budget of the big kernel.
  char* base;
  int64_t ship_stride;   // bytes of one [env][ship] array (doubles)
  int64_t route_stride;  // bytes of one [env][ship][kMaxRoute] route array
  int64_t env_stride;    // bytes of one per-env array (sized for the widest: 8 floats)
  int64_t env_off;       // start of the per-env arrays
  __host__ __device__ double* f(int k) const { return (double*)(base + k * ship_stride); }
  __host__ __device__ int32_t* next_wpt() const { return (int32_t*)(base + 19 * ship_stride); }
  __host__ __device__ int32_t* stop() const { return (int32_t*)(base + 20 * ship_stride); }
  __host__ __device__ int32_t* n_route() const { return (int32_t*)(base + 21 * ship_stride); }
  __host__ __device__ double* route_n() const { return (double*)(base + 22 * ship_stride); }
  __host__ __device__ double* route_e() const { return (double*)(base + 22 * ship_stride + route_stride); }
  __host__ __device__ char* ev(int k) const { return base + env_off + k * env_stride; }
  __host__ __device__ int32_t* sampling_count() const { return (int32_t*)ev(0); }
  __host__ __device__ double* travel_dist() const { return (double*)ev(1); }
  __host__ __device__ double* travel_time() const { return (double*)ev(2); }
  __host__ __device__ double* acc() const { return (double*)ev(3); }
  __host__ __device__ double* n_base() const { return (double*)ev(4); }
  __host__ __device__ double* e_base() const { return (double*)ev(5); }
  __host__ __device__ double* p_last() const { return (double*)ev(6); }
  __host__ __device__ double* chi_last() const { return (double*)ev(7); }
  __host__ __device__ double* mach_dt() const { return (double*)ev(8); }
  __host__ __device__ float* states4() const { return (float*)ev(9); }      // [env][4] self.states (simple collav)
  __host__ __device__ float* next_obs8() const { return (float*)ev(10); }   // [env][8] self.next_observations
  __host__ __device__ uint32_t* snap_bits() const { return (uint32_t*)ev(11); }
  __host__ __device__ int32_t* was_reset() const { return (int32_t*)ev(12); }
  __host__ __device__ int32_t* dec_flags() const { return (int32_t*)ev(13); }  // DF_* (sliced stepping)
  __host__ __device__ double* legacy_states() const { return (double*)ev(14); }  // [env][4] legacy self.states
  __host__ __device__ int32_t* legacy_flags() const { return (int32_t*)ev(15); }  // 1: still the f32 initial_states
  __host__ __device__ int32_t* dec_ticks() const { return (int32_t*)ev(16); }  // ticks of the decision in progress
  // the decision in progress as the stream logs it (SHIPSIM_DL_ACTION / _OBS0): its action, the observation it
  // was chosen from
  __host__ __device__ float* dec_action() const { return (float*)ev(17); }
  __host__ __device__ float* dec_obs0() const { return (float*)ev(18); }  // [env][8]
  int32_t* nonfinite;  // device counter: envs flagged SHIPSIM_EV_NONFINITE (read by shipsim_synchronize)
  static constexpr int kEnvArrays = 19;
  static constexpr int kShipArrays = 22;
};
// shipsim_fork moves the columns of state_host::table(): an array added here gets its row there
static_assert(DevState::kEnvArrays == state_host::kEnvArrays && DevState::kShipArrays == state_host::kShipArrays &&
                  kMaxRoute * sizeof(double) == state_host::kRouteSlotBytes,
              "DevState and the column table (shipsim_state_host.hpp) list the same arrays");
// dec_flags bits (per env, persistent across calls)
#define DF_AWAITING 1
#define DF_HAVE_IW 2
#define DF_PHASE_SHIFT 2

enum { SF_N = 0, SF_E, SF_YAW, SF_U, SF_V, SF_R, SF_OMEGA, SF_TIME, SF_ECT, SF_ECT_INT, SF_HDG_EI, SF_HDG_PREV,
       SF_SPD_A, SF_SPD_B, SF_RUDDER, SF_THRUST, SF_LOG_ECT, SF_LOG_N, SF_LOG_E };

struct ConstBuf {
  // edges [SHIPSIM_MAX_VERTS] | boxes [SHIPSIM_MAX_POLYS] | config routes n/e [MAX_SHIPS][kMaxRoute] each
  // | ShipConst [MAX_SHIPS] | map grid: cell edge masks [gny][gnx] uint64 | cell containment flags [gny][gnx] uint8
  // | (8-B aligned) cell edge masks split by bit rank mod 8 [gny][gnx][8] uint64
  const char* base;
  int32_t n_edges;
  int32_t gnx, gny;            // grid cells (0 = no grid: every query runs over the full map)
  double gx0, gy0, ginv;       // grid origin (east, north) and 1 / cell size
  const uint64_t* grid_mask;   // edges whose distance to the (slightly enlarged) cell is <= kGroundReach
  const uint8_t* grid_flag;    // GRID_OUT: cell entirely outside every polygon, GRID_IN: inside one, GRID_MIXED
  const uint64_t* grid_part;   // [cell][8]: the cell's mask split by bit rank mod 8 (sub-lane shares, no bit skipping)
  __host__ __device__ const Edge* edges() const { return (const Edge*)base; }
  __host__ __device__ const PolyBox* boxes() const { return (const PolyBox*)(base + sizeof(Edge) * SHIPSIM_MAX_VERTS); }
  __host__ __device__ const double* cfg_route_n() const {
    return (const double*)(base + sizeof(Edge) * SHIPSIM_MAX_VERTS + sizeof(PolyBox) * SHIPSIM_MAX_POLYS);
  }
  __host__ __device__ const double* cfg_route_e() const { return cfg_route_n() + SHIPSIM_MAX_SHIPS * kMaxRoute; }
  // per-ship constants (config_host::ship_const), [ship] for the 1 + K ships of an env
  static constexpr size_t kShipsOff = kConstShipsOff;
  __host__ __device__ const ShipConst* ships() const { return (const ShipConst*)(base + kShipsOff); }
  static constexpr size_t kBytes = kConstBytes;
  // grid cell of (north, east), or -1 outside the grid / no grid / non-finite position
  __device__ __forceinline__ int cell(double n, double e) const { return grid_cell(*this, n, e); }
};

__device__ __forceinline__ void load_ship(const DevState& S, int q, Ship& s) {
  s.n = S.f(SF_N)[q]; s.e = S.f(SF_E)[q]; s.yaw = S.f(SF_YAW)[q];
  s.u = S.f(SF_U)[q]; s.v = S.f(SF_V)[q]; s.r = S.f(SF_R)[q];
  s.omega = S.f(SF_OMEGA)[q]; s.time = S.f(SF_TIME)[q];
  s.e_ct = S.f(SF_ECT)[q]; s.e_ct_int = S.f(SF_ECT_INT)[q];
  s.hdg_ei = S.f(SF_HDG_EI)[q]; s.hdg_prev = S.f(SF_HDG_PREV)[q];
  s.spd_a = S.f(SF_SPD_A)[q]; s.spd_b = S.f(SF_SPD_B)[q];
  s.log_rudder = S.f(SF_RUDDER)[q]; s.log_thrust = S.f(SF_THRUST)[q]; s.log_ect = S.f(SF_LOG_ECT)[q];
  s.log_n = S.f(SF_LOG_N)[q]; s.log_e = S.f(SF_LOG_E)[q];
  s.next_wpt = S.next_wpt()[q]; s.stop = S.stop()[q]; s.n_route = S.n_route()[q];
  load_segment(s, S.route_n() + (size_t)q * kMaxRoute, S.route_e() + (size_t)q * kMaxRoute);
}
__device__ __forceinline__ void store_ship(const DevState& S, int q, const Ship& s) {
  S.f(SF_N)[q] = s.n; S.f(SF_E)[q] = s.e; S.f(SF_YAW)[q] = s.yaw;
  S.f(SF_U)[q] = s.u; S.f(SF_V)[q] = s.v; S.f(SF_R)[q] = s.r;
  S.f(SF_OMEGA)[q] = s.omega; S.f(SF_TIME)[q] = s.time;
  S.f(SF_ECT)[q] = s.e_ct; S.f(SF_ECT_INT)[q] = s.e_ct_int;
  S.f(SF_HDG_EI)[q] = s.hdg_ei; S.f(SF_HDG_PREV)[q] = s.hdg_prev;
  S.f(SF_SPD_A)[q] = s.spd_a; S.f(SF_SPD_B)[q] = s.spd_b;
  S.f(SF_RUDDER)[q] = s.log_rudder; S.f(SF_THRUST)[q] = s.log_thrust; S.f(SF_LOG_ECT)[q] = s.log_ect;
  S.f(SF_LOG_N)[q] = s.log_n; S.f(SF_LOG_E)[q] = s.log_e;
  S.next_wpt()[q] = s.next_wpt; S.stop()[q] = s.stop; S.n_route()[q] = s.n_route;
}

// per-block LDS copy of the ships' ShipConst (lanes of one ship read one address)
// (and the reciprocals div_by uses, formed here on the device: the bits of the division sequence's own)
__device__ __forceinline__ const ShipConst* stage_consts(const ConstBuf& K, ShipConst* lds, int n_ships, double dt) {
  const int nwords = (int)(sizeof(ShipConst) * n_ships / sizeof(double));
  const double* src = reinterpret_cast<const double*>(K.ships());
  double* dst = reinterpret_cast<double*>(lds);
  for (int i = threadIdx.x; i < nwords; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
  if ((int)threadIdx.x < n_ships) {
    ShipConst& c = lds[threadIdx.x];
    c.rcp_r_me = div_rcp(c.r_me); c.rcp_r_hsg = div_rcp(c.r_hsg); c.rcp_jp = div_rcp(c.jp); c.rcp_dt = div_rcp(dt);
  }
  __syncthreads();
  return lds;
}

// single_tick_pipe_kernel<POW2_DT> on `blocks` blocks of 192 threads (shipsim_c2_pipe.hip)
void shipsim_c2_pipe_launch(int blocks, hipStream_t st, const Params& P, const DevState& S, const ConstBuf& K, int k);

// level_distance_kernel over n_envs envs of n_ships ships (shipsim_resample.hip)
void shipsim_level_distance_launch(hipStream_t st, const DevState& S, int n_envs, int n_ships, double* out);

// archive_gather_kernel (shipsim_archive.hip): slot d of the n_dst slots of dst (laid out by dst_table) takes slot
// index[d] of the n_src slots of src (src_table); an index outside [0, n_src) leaves slot d alone
void shipsim_archive_gather_launch(hipStream_t st, const state_host::Table& src_table,
                                   const state_host::Table& dst_table, const void* src, void* dst,
                                   const int32_t* index, int32_t n_dst, int32_t n_src);

// weather_gather_kernel (shipsim_weather.hip): slot d of the n_dst slots of the weather table dst takes slot index[d]
// of the n_src slots of src, all six rows (weather_host::kStoreRows); an index outside [0, n_src) leaves slot d alone,
// or — own, n_src == n_dst: a fork's staging table — gives it slot d of src
void shipsim_weather_gather_launch(hipStream_t st, const double* src, double* dst, const int32_t* index, int32_t n_dst,
                                   int32_t n_src, bool own);
