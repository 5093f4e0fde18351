// shipsim_sbmpc.hpp — the wave-cooperative SBMPC optimiser (device functions) that the env kernels and the two batch
// kernels behind shipsim_sbmpc_eval / shipsim_sbmpc_eval_multi run. Part of shipsim_kernels.hip's object: included
// there, once, after the ship model.
#pragma once
#include <hip/hip_runtime.h>

#include "shipsim_device.hpp"
#include "shipsim_sbmpc_nominal.hpp"  // SbIn, p_ca_of, sbmpc_h2, sbmpc_nominal_holds

using namespace shipsim;

// ---------------------------------------------------------------------------------------------
// SBMPC (sbmpc.py:113-298), wave-cooperative: each requesting env's 7 x 4 scenarios are spread
// over 28 lanes of a half-wave; two envs are served per pass.
// ---------------------------------------------------------------------------------------------
// (SbIn, the request, with p_ca_of and sbmpc_h2: shipsim_sbmpc_nominal.hpp, shared with the host)
// sin/cos(ob_psi) of a request built from its heading alone
__device__ __forceinline__ void sb_set_heading_trig(SbIn& q) { sincos(q.ob_psi, &q.ob_so, &q.ob_co); }

// a lane value the compiler must re-derive after this point (loads indexed by it cannot be hoisted)
__device__ __forceinline__ int opaque_v(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
// a wave-uniform value the compiler must re-derive after this point (comparisons on it cannot be hoisted)
__device__ __forceinline__ int opaque_s(int x) {
  asm volatile("" : "+s"(x));
  return x;
}
// opaque_v where OPQ (the kernels whose allocation otherwise spills the lane masks derived from x), x as is
// elsewhere (there the recomputation costs more than the held mask)
template <bool OPQ>
__device__ __forceinline__ int opaque_if(int x) {
  if constexpr (OPQ) return opaque_v(x);
  return x;
}

__device__ __forceinline__ double shfl_d(double x, int src) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __shfl(lo, src, 64);
  hi = __shfl(hi, src, 64);
  return __hiloint2double(hi, lo);
}

constexpr double kCosPhiAh = 0.36650122672429719;  // cos(68.5°) (only used against a 1e-9 band)
constexpr double kSinPhiAh = 0.93041756798202460;  // sin(68.5°)

// sqrt(a) < c and sqrt(a) <= c (c > 0) decided on a against c², except within a relative 1e-12 of
// it where the correctly rounded square root itself decides: the reference's boolean, without the
// ~20-instruction f64 sqrt on every tick (NaN compares false either way)
__device__ __forceinline__ bool sqrt_lt(double a, double c) {
  const double c2 = c * c;
  if (a < c2 * (1.0 - 1e-12)) return true;
  if (!(a <= c2 * (1.0 + 1e-12))) return false;
  return sqrt(a) < c;
}
__device__ __forceinline__ bool sqrt_le(double a, double c) {
  const double c2 = c * c;
  if (a < c2 * (1.0 - 1e-12)) return true;
  if (!(a <= c2 * (1.0 + 1e-12))) return false;
  return sqrt(a) <= c;
}

// (d_safe / dist) ** Q_ with Q_ = 4 (sbmpc.py:262): x² = h + l and h² = h2 + e exactly (fma), so
// h2 + (e + (2hl + l²)) carries ~100 bits into its one final rounding — the correctly rounded x⁴, which
// is glibc's pow(x, 4.0) except where that pow's last 0.02 ulp decides (85 per 10⁵ random d_safe / dist
// in (0.9, 1000]) — in 11 VALU instructions instead of the general pow's 214. An infinite x⁴ (dist -> 0)
// is returned as is.
__device__ __forceinline__ double pow4(double x) {
  const double h = x * x, l = fma(x, x, -h);
  const double h2 = h * h;
  if (!(h2 < INFINITY)) return h2;
  const double e = fma(h, h, -h2);
  return h2 + (e + (2.0 * h * l + l * l));
}

// Per-sample collision cost H0 = C·R of sbmpc.py:205-289 (KAPPA_ = 0) for one prediction sample with
// obstacle-minus-own-ship offset (d0, d1); (ss, cs, sv) are the own ship's sin/cos(psi_) and sway
// at that sample. R and C stay 0 unless dist < d_safe_i <= max_d_safe, so the sector geometry (atan2,
// wrap, norms) is only evaluated there; identical results to the reference's `dist < d_close` block.
__device__ __forceinline__ double sbmpc_sample_cost(const SbIn& in, double so, double co, double vo0, double vo1,
                                                    double no, double t, double d0, double d1, double d2s,
                                                    double ss, double cs, double ud, double sv, double max_d_safe,
                                                    double lim2, double cos_ot) {
  const double os_l = 25.0, d_safe = 1000.0, d_close = 2000.0;
  const double PHI_AH = 68.5 * (kPi / 180.0), PHI_OT = 68.5 * (kPi / 180.0);
  if (!(d2s < lim2)) return 0.0;  // d2s >= lim2 already implies sqrt(d2s) >= max_d_safe
  const double dist = sqrt(d2s);
  if (!(dist < d_close && dist < max_d_safe)) return 0.0;
  double vs0 = -ss * ud + cs * sv;
  double vs1 = cs * ud + ss * sv;
  // sector of phi_o = wrap(atan2(-d1, -d0) - psi_o + pi/2) against PHI_AH == PHI_OT = θ: e is
  // (-d0, -d1) rotated by pi/2 - psi_o, so phi_o = angle(e); phi_o > θ <=> sin(angle(e) - θ) >= 0
  // and e_y > 0. Within 1e-9 rad of a decision boundary the reference expression is evaluated.
  const double ex = so * (-d0) - co * (-d1), ey = co * (-d0) + so * (-d1);
  const double cr = kCosPhiAh * ey - kSinPhiAh * ex;
  int sector;  // 0: phi_o < PHI_AH, 1: phi_o > PHI_OT, 2: equal
  if (fabs(cr) > 1e-9 * dist && fabs(ey) > 1e-9 * dist) {
    sector = (cr >= 0 && ey > 0) ? 1 : 0;
  } else {
    const double phi_o = wrap_pmpi(atan2(-d1, -d0) - in.ob_psi + kPi / 2);
    sector = (phi_o < PHI_AH) ? 0 : ((phi_o > PHI_OT) ? 1 : 2);
  }
  double d_safe_i;
  if (sector == 0) d_safe_i = d_safe + in.obs_l / 2;
  else if (sector == 1) d_safe_i = 0.5 * d_safe + in.obs_l / 2;
  else d_safe_i = d_safe + in.obs_w / 2;
  double dot = vs0 * vo0 + vs1 * vo1;
  double ns = sqrt(vs0 * vs0 + vs1 * vs1);
  if (dot > cos_ot * ns * no && ns > no) d_safe_i = d_safe + os_l / 2 + in.obs_l / 2;
  if (!(dist < d_safe_i)) return 0.0;
  const double R = (1 / fabs(t - 0.0)) * pow4(d_safe / dist);  // pow(|t|, 1.0) == |t| exactly
  const double k_coll = 1e-6 * os_l * in.obs_l;
  const double w0 = vs0 - vo0, w1 = vs1 - vo1;
  const double nrm = sqrt(w0 * w0 + w1 * w1);
  const double C = k_coll * (nrm * nrm);
  return C * R + 0.0 * 0;
}

// sbmpc.py:190-298 cost_func for one (Chi_ca, P_ca) scenario, sample by sample as the reference.
// Kept as the exact fallback of sbmpc_scenario_cost (near-ties between samples).
__device__ __forceinline__ double sbmpc_scenario_cost_direct(const SbIn& in, int n_samp, double DT, double ud,
                                                          double sp, double cp, double sp0, double cp0, double so,
                                                          double co, double vo0, double vo1, double no,
                                                          double max_d_safe, double lim2, double cos_ot, double H2) {
  const double r11 = -so, r12 = co, r21 = co, r22 = so;
  const double q11 = -sp, q12 = cp, q21 = cp, q22 = sp;
  double ox = in.ob_x, oy = in.ob_y, sx = in.os_x, sy = in.os_y, sv = in.os_v;
  double H1 = 0, t = 0;
  for (int i = 0; i < n_samp; ++i) {
    if (i > 0) {
      ox = ox + (r11 * in.ob_u + r12 * in.ob_v) * DT;
      oy = oy + (r21 * in.ob_u + r22 * in.ob_v) * DT;
      sx = sx + DT * (q11 * ud + q12 * sv);
      sy = sy + DT * (q21 * ud + q22 * sv);
      sv = 0.0;
    }
    t += DT;
    const double d0 = ox - sx, d1 = oy - sy;
    const double H0 = sbmpc_sample_cost(in, so, co, vo0, vo1, no, t, d0, d1, d0 * d0 + d1 * d1, (i == 0) ? sp0 : sp,
                                        (i == 0) ? cp0 : cp, ud, sv, max_d_safe, lim2, cos_ot);
    if (H0 > H1) H1 = H0;
  }
  return H1 + H2;
}


// No scenario can bring this obstacle within max_d_safe over the horizon: the distance now minus the
// most either ship can travel (own ship: sample 0 at its current sway, then straight at <= u_d; the
// obstacle: straight at its speed) stays beyond max_d_safe with a 1 m margin (the incremental
// predictions round at ~1e-12 relative). Then every scenario's cost for it is exactly sbmpc_h2.
__device__ __forceinline__ bool sbmpc_far(const SbIn& in, int n_samp, double DT) {
  const double os_l = 25.0, d_safe = 1000.0;
  const double max_d_safe = py_max(py_max(d_safe + in.obs_l / 2, 0.5 * d_safe + in.obs_l / 2),
                                   py_max(d_safe + in.obs_w / 2, d_safe + os_l / 2 + in.obs_l / 2));
  const double ex = in.ob_x - in.os_x, ey = in.ob_y - in.os_y;
  const double own = DT * sqrt(in.u_d * in.u_d + in.os_v * in.os_v) + (n_samp - 2 > 0 ? n_samp - 2 : 0) * DT * in.u_d;
  const double obs = (n_samp - 1) * DT * sqrt(in.ob_u * in.ob_u + in.ob_v * in.ob_v);
  const double lim = max_d_safe + 1.0 + own + obs;
  return ex * ex + ey * ey > lim * lim;
}

// running state of a scenario's horizon: best (s1 at time t1, squared distance q1) and runner-up s2 of the
// ranking t·d², and whether any in-range sample sat within a rounding band of a decision (unc)
struct HzBest {
  double s1, s2, t1, q1;
  bool unc;
};
struct HzConst {
  double so, co, ovr2, ot2, ah2, cl2;  // obstacle heading sin/cos, squared thresholds
  bool ovr;                            // the overtaking override of d_safe_i holds for every sample
};
// one horizon sample (time tt, offset (d0, d1), d2s = |.|²) into the running state; inr: the sample is within
// max_d_safe (one beyond it contributes nothing and flags nothing). Branch-free (& | on bools).
__device__ __forceinline__ void hz_sample(HzBest& h, const HzConst c, double tt, double d0, double d1, double d2s,
                                          bool inr) {
  constexpr double kEps = 1e-12;
  // sector of phi_o (see sbmpc_sample_cost): overtaking sector iff cr >= 0 and ey > 0
  const double ex = c.so * (-d0) - c.co * (-d1), ey = c.co * (-d0) + c.so * (-d1);
  const double cr = kCosPhiAh * ey - kSinPhiAh * ex;
  const bool sec_ok = (cr * cr > 1e-18 * d2s) & (ey * ey > 1e-18 * d2s);
  const double D2 = c.ovr ? c.ovr2 : (((cr >= 0) & (ey > 0)) ? c.ot2 : c.ah2);
  const bool member = inr & (d2s < D2 * (1.0 - kEps)) & (d2s < c.cl2 * (1.0 - kEps));
  h.unc = h.unc | (inr & (((!c.ovr) & (!sec_ok)) | (fabs(d2s - D2) <= kEps * D2) | (fabs(d2s - c.cl2) <= kEps * c.cl2)));
  const double sc = member ? tt * d2s * d2s : INFINITY;
  const bool lt1 = sc < h.s1;
  h.s2 = fmin(h.s2, fmax(h.s1, sc));  // runner-up: the old best if sc takes the lead, else min(s2, sc)
  h.t1 = lt1 ? tt : h.t1;
  h.q1 = lt1 ? d2s : h.q1;
  h.s1 = fmin(h.s1, sc);
}

// part -1: the whole horizon on this lane. part 0 / 1: this lane and its partner (lane ^ 32: the same scenario of the
// same request) split the horizon's sample loop — part 0 takes the samples before i_split, part 1 the rest — and merge
// their running bests (every other step is computed by both; the result is the same bits as part -1)
__device__ double sbmpc_scenario_cost(const SbIn& in, int n_samp, double DT, int ichi, int jp, int part = -1) {
  SB_TIMER;
  const double os_l = 25.0;  // ShipLinearModel default length (sbmpc_misc.py:86, Q7)
  const double d_safe = 1000.0, d_close = 2000.0;
  // np.cos(np.deg2rad(PHI_OT_)) — PHI_OT_ is already in radians (sbmpc.py:248): a constant, taken
  // as the correctly rounded double of cos(68.5·(π/180)²) (NumPy and glibc agree on it)
  constexpr double cos_ot = 0.9997823068017366;
  const double max_d_safe = py_max(py_max(d_safe + in.obs_l / 2, 0.5 * d_safe + in.obs_l / 2),
                                   py_max(d_safe + in.obs_w / 2, d_safe + os_l / 2 + in.obs_l / 2));
  const double CHI_DEG = -30.0 + 10.0 * ichi;
  const double P_ca = p_ca_of(jp);
  const double Chi_ca = CHI_DEG * (kPi / 180.0);
  const double ud = in.u_d * P_ca;
  const double psi_d = in.chi_d + Chi_ca;
  // Obstacle trajectory (sbmpc_misc.py:65-83) and linear_pred (:103-123), advanced incrementally
  // the obstacle heading's sin/cos come with the request (ob_so, ob_co): the same values as
  // sincos(in.ob_psi) — in the AST kernels they are the obstacle ship's own carried sin/cos(yaw) with
  // ob_psi = -yaw, and the device sin is odd and cos even (both reduce |x|), so nothing is recomputed
  // per scenario
  const double so = in.ob_so, co = in.ob_co;
  const double r11 = -so, r12 = co, r21 = co, r22 = so;
  const double vo0 = -so * in.ob_u + co * in.ob_v;  // rot2d(obstacle.psi_, [u, v])
  const double vo1 = co * in.ob_u + so * in.ob_v;
  const double no = sqrt(vo0 * vo0 + vo1 * vo1);
  double sp, cp;
  sincos(psi_d, &sp, &cp);
  const double q11 = -sp, q12 = cp, q21 = cp, q22 = sp;
  double sp0 = sp, cp0 = cp;
  const double psi_w = wrap_pmpi(psi_d);
  if (psi_w != psi_d) sincos(psi_w, &sp0, &cp0);
  const double H2 = sbmpc_h2(in, ichi, jp);
  int i_last = n_samp - 1;  // (set by the skip test below)
  int i_first = 1;          // first sample that can be within range (ditto; only places the split)
  int i_past = n_samp + 1;  // first sample past the closest approach, with a one-sample margin (ditto)
  // Exact skip of the horizon loop: H0 can only be non-zero at samples with dist < max_d_safe.
  // After sample 0 both predictions are straight lines (the own ship's sway is zeroed after the
  // first step), so the relative position is P1 + k·W, k = 0..n_samp-2; if its continuous minimum
  // (and sample 0) stays above max_d_safe by a margin far beyond the rounding of the incremental
  // update below, every sample's H0 is 0 and the cost is H2 alone.
  {
    const double vox = r11 * in.ob_u + r12 * in.ob_v, voy = r21 * in.ob_u + r22 * in.ob_v;
    const double e0x = in.ob_x - in.os_x, e0y = in.ob_y - in.os_y;
    const double p1x = (in.ob_x + vox * DT) - (in.os_x + DT * (q11 * ud + q12 * in.os_v));
    const double p1y = (in.ob_y + voy * DT) - (in.os_y + DT * (q21 * ud + q22 * in.os_v));
    const double wx = (vox - q11 * ud) * DT, wy = (voy - q21 * ud) * DT;
    const double ww = wx * wx + wy * wy;
    const double iww = ww > 0 ? 1.0 / ww : 0.0;  // (k and j2 below only place bounds with margins)
    double k = ww > 0 ? -(p1x * wx + p1y * wy) * iww : 0.0;
    k = k < 0 ? 0 : (k > n_samp - 2 ? n_samp - 2 : k);
    const double mx = p1x + k * wx, my = p1y + k * wy;
    const double lim = max_d_safe + 1e-3;
    SB_MARK(0);
    if (e0x * e0x + e0y * e0y > lim * lim && mx * mx + my * my > lim * lim) return 0.0 + H2;
    // Last sample that can still be within max_d_safe: |P1 + j·W| is convex in j, so past the larger
    // root j2 of |P1 + j·W| = lim every later sample stays out of range (the incremental positions
    // below differ from this closed form by ~1e-10 m, far inside the 1e-3 m of lim). Sample i = j + 1.
    const double b = p1x * wx + p1y * wy, cq = p1x * p1x + p1y * p1y - lim * lim;
    const double disc = b * b - ww * cq;
    const double j2 = (ww > 0 && disc >= 0) ? (-b + sqrt(disc)) * iww : (double)n_samp;
    i_last = (j2 < (double)(n_samp - 2)) ? (int)floor(j2) + 2 : n_samp - 1;
    const double j1 = (ww > 0 && disc >= 0) ? (-b - sqrt(disc)) * iww : 0.0;
    i_first = (j1 > 1.0) ? (int)fmin(floor(j1), (double)(n_samp - 1)) : 1;
    // Past the continuous minimum k of |P1 + j·W| both t and the distance grow, so the ranking t·d⁴ grows
    // sample by sample: once a sample there ranks beyond the best so far by more than the runner-up band,
    // no later sample can win or tie (and a later sample's flags cannot change the result). Sample i = j + 1;
    // k is clamped to the horizon, so a minimum at its end never stops the loop.
    i_past = (int)ceil(k) + 3;
  }
  const double lim2 = (max_d_safe * (1.0 + 1e-9)) * (max_d_safe * (1.0 + 1e-9));
  // Sample 0 (own ship at wrap(psi_d) with its current sway) exactly as the reference.
  const double e0x = in.ob_x - in.os_x, e0y = in.ob_y - in.os_y;
  double H1 = 0;
  {
    const double H0 = sbmpc_sample_cost(in, so, co, vo0, vo1, no, DT, e0x, e0y, e0x * e0x + e0y * e0y, sp0, cp0, ud,
                                        in.os_v, max_d_safe, lim2, cos_ot);
    if (H0 > H1) H1 = H0;
  }
  SB_MARK(1);
  // Samples 1..n-1: the own ship's velocity is constant (sway zeroed), so C and the overtaking
  // override of d_safe_i are sample-independent, and H0 = C·R with R = d_safe^4 / (t·dist^4).
  // max_i fl(C·R_i) = fl(C·max_i R_i) (rounding is monotone), so only the sample with the largest
  // R needs the exact pow: members are ranked by s = t·d2s² (within ~1e-14 of the exact ordering);
  // a runner-up within 1e-10 of the best sends the scenario to the sample-by-sample evaluation.
  const double vs0 = -sp * ud + cp * 0.0, vs1 = cp * ud + sp * 0.0;
  const double dot1 = vs0 * vo0 + vs1 * vo1;
  const double ns1 = sqrt(vs0 * vs0 + vs1 * vs1);
  const bool ovr = dot1 > cos_ot * ns1 * no && ns1 > no;
  const double ds_ah = d_safe + in.obs_l / 2, ds_ot = 0.5 * d_safe + in.obs_l / 2;  // :239-242
  const double ds_ovr = d_safe + os_l / 2 + in.obs_l / 2;
  // Branch-free horizon: membership dist < d_safe_i (and < d_close) is decided on d2s against the
  // squared thresholds; a sample within 1e-12 of a threshold, or whose sector is within 1e-9 of
  // the PHI_AH / PHI_OT boundary, marks the scenario `unc` and it is re-evaluated sample by sample.
  constexpr double kEps = 1e-12;
  const double ah2 = ds_ah * ds_ah, ot2 = ds_ot * ds_ot, ovr2 = ds_ovr * ds_ovr, cl2 = d_close * d_close;
  // position increments: the obstacle's are constant, the own ship's use its sway at sample 1
  // only (linear_pred zeroes v after the first step)
  const double dox = (r11 * in.ob_u + r12 * in.ob_v) * DT, doy = (r21 * in.ob_u + r22 * in.ob_v) * DT;
  const double dsx = DT * (q11 * ud + q12 * 0.0), dsy = DT * (q21 * ud + q22 * 0.0);
  double ox = in.ob_x, oy = in.ob_y;
  double sx = in.os_x + DT * (q11 * ud + q12 * in.os_v), sy = in.os_y + DT * (q21 * ud + q22 * in.os_v);
  double t = DT;
  if constexpr (diag::kNoSbLoop) n_samp = 1;  // (ablation build only: no horizon samples after sample 0)
  HzBest hb{INFINITY, INFINITY, 0.0, 0.0, false};
  const HzConst hc{so, co, ovr2, ot2, ah2, cl2, ovr};
  auto sample = [&](double tt, double d0, double d1, double d2s, bool inr) __attribute__((always_inline)) {
    hz_sample(hb, hc, tt, d0, d1, d2s, inr);
  };
  // two samples per iteration (i, i + 1): their bodies are independent chains the one wave of the SIMD
  // can interleave; the positions are the same incremental sums as one per iteration, and the samples
  // enter the running best in order (ties keep the earlier sample).
  // Split (part 0 / 1): the window of samples that can be in range, [i_first, min(i_last, i_past + 2)], is cut at
  // its middle; part 1 first advances its positions to the cut by the loop's own sums (a uniform loop, the other
  // lanes predicated off), then both parts run the loop side by side on their own sample indices.
  int i_stop = n_samp, i = 1;
  if (part >= 0) {
    const int w0 = max(i_first, 1), w1 = max(w0, min(i_last, i_past + 2));
    const int i_split = min(w0 + (w1 - w0 + 1) / 2, n_samp);
    if (part == 0) i_stop = i_split;
    const int i_start = part == 1 ? i_split : 1;
    for (int c = 1; __any(c < i_start); ++c) {
      const bool adv = c < i_start, adv_s = adv & (c > 1);
      ox = adv ? ox + dox : ox;
      oy = adv ? oy + doy : oy;
      sx = adv_s ? sx + dsx : sx;
      sy = adv_s ? sy + dsy : sy;
      t = adv ? t + DT : t;
    }
    i = i_start;
  }
  bool done = false;  // past the minimum and beyond the best (see i_past)
  for (;; i += 2) {
    // (per lane: a split part has its own sample index; unsplit every lane has the same one)
    if (!__any((i + 1 < n_samp) & (i <= i_last) & !done & (i < i_stop))) break;  // every lane past its useful samples
    const double oxa = ox + dox, oya = oy + doy;
    const double sxa = (i > 1) ? sx + dsx : sx, sya = (i > 1) ? sy + dsy : sy;
    const double ta = t + DT;
    ox = oxa + dox;
    oy = oya + doy;
    sx = sxa + dsx;
    sy = sya + dsy;
    t = ta + DT;
    const double d0a = oxa - sxa, d1a = oya - sya, d0b = ox - sx, d1b = oy - sy;
    const double d2a = d0a * d0a + d1a * d1a, d2b = d0b * d0b + d1b * d1b;
    const bool ia = (d2a < lim2) & (i + 1 < n_samp) & (i < i_stop);
    const bool ib = (d2b < lim2) & (i + 1 < n_samp) & (i + 1 < i_stop);
    if (ia | ib) {
      sample(ta, d0a, d1a, d2a, ia);
      sample(t, d0b, d1b, d2b, ib);
    }
    done = done | ((i + 1 >= i_past) & (hb.s1 < INFINITY) & (t * d2b * d2b > hb.s1 * (1.0 + 2e-10)));
  }
  {
    const bool lo = (i < n_samp) & (i < i_stop);
    if (__any(lo & (i <= i_last) & !done)) {  // the last sample of an odd count
      ox = ox + dox;
      oy = oy + doy;
      if (i > 1) {
        sx = sx + dsx;
        sy = sy + dsy;
      }
      t += DT;
      const double d0 = ox - sx, d1 = oy - sy;
      const double d2s = d0 * d0 + d1 * d1;
      if ((d2s < lim2) & lo) sample(t, d0, d1, d2s, true);
    }
  }
  if (part >= 0) {  // the two parts' running bests in sample order: part 0's samples come first
    // the partner lane (lane ^ 32) by v_permlane32_swap: after the swap of a value with itself the lower half holds
    // the upper half's value in the second result, the upper half the lower half's in the first
    const bool upper = part == 1;
    auto other_u = [&](unsigned x) __attribute__((always_inline)) {
      const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
      return upper ? r[0] : r[1];
    };
    auto other_d = [&](double x) __attribute__((always_inline)) {
      const unsigned lo = other_u((unsigned)__double2loint(x)), hi = other_u((unsigned)__double2hiint(x));
      return __hiloint2double((int)hi, (int)lo);
    };
    HzBest o;
    o.s1 = other_d(hb.s1);
    o.s2 = other_d(hb.s2);
    o.t1 = other_d(hb.t1);
    o.q1 = other_d(hb.q1);
    o.unc = other_u((unsigned)hb.unc) != 0u;
    const HzBest A = part == 0 ? hb : o, Bp = part == 0 ? o : hb;
    const bool bwin = Bp.s1 < A.s1;  // (ties keep the earlier sample)
    hb.s1 = fmin(A.s1, Bp.s1);
    hb.s2 = fmin(fmin(A.s2, Bp.s2), fmax(A.s1, Bp.s1));  // the second smallest of both
    hb.t1 = bwin ? Bp.t1 : A.t1;
    hb.q1 = bwin ? Bp.q1 : A.q1;
    hb.unc = A.unc | Bp.unc;
  }
  const double s1 = hb.s1, s2 = hb.s2, t1 = hb.t1, q1 = hb.q1;
  if (hb.unc)
    return sbmpc_scenario_cost_direct(in, n_samp, DT, ud, sp, cp, sp0, cp0, so, co, vo0, vo1, no, max_d_safe, lim2,
                                      cos_ot, H2);
  SB_MARK(2);
  if (s1 < INFINITY) {
    if (s2 <= s1 * (1.0 + 1e-10))
      return sbmpc_scenario_cost_direct(in, n_samp, DT, ud, sp, cp, sp0, cp0, so, co, vo0, vo1, no, max_d_safe, lim2,
                                        cos_ot, H2);
    const double R = (1 / fabs(t1 - 0.0)) * pow4(d_safe / sqrt(q1));
    const double k_coll = 1e-6 * os_l * in.obs_l;
    const double w0 = vs0 - vo0, w1 = vs1 - vo1;
    const double nrm = sqrt(w0 * w0 + w1 * w1);
    const double H0 = (k_coll * (nrm * nrm)) * R + 0.0 * 0;
    if (H0 > H1) H1 = H0;
  }
  return H1 + H2;
}

// Argmin of (cost, index) over each half-wave (its 32 scenario lanes), every lane of the half ending with the
// result; ties -> the lower index. The order (cost, then index) is a total order on non-NaN costs, so any pairing
// gives the same result: inside each 16-lane row by DPP (quad xor 1, quad xor 2, row_ror 4, row_ror 8: every lane
// then holds its row's minimum), then one LDS permute across the half-wave's two rows. Every lane of the wave
// must be active (the cooperative passes are called wave-uniformly).
// SHFL: the cross-row step by an LDS permute instead (the multi-obstacle and C1 kernels: the swap's lane-mask select
// costs them SGPRs they do not have; the same result)
template <bool SHFL = false>
__device__ __forceinline__ void scenario_argmin(double& cost, int& idx, int lane) {
  auto take = [&](double oc, int oi) __attribute__((always_inline)) {
    if (oc < cost || (oc == cost && oi < idx)) { cost = oc; idx = oi; }
  };
  take(dpp_d<kDppQuadXor1>(cost), dpp_i<kDppQuadXor1>(idx));
  take(dpp_d<kDppQuadXor2>(cost), dpp_i<kDppQuadXor2>(idx));
  take(dpp_d<kDppRowRor4>(cost), dpp_i<kDppRowRor4>(idx));
  take(dpp_d<kDppRowRor8>(cost), dpp_i<kDppRowRor8>(idx));
  // the other row of the half-wave (lane ^ 16) by v_permlane16_swap: after the swap of a value with itself the even
  // rows hold their partner row's value in the second result, the odd rows in the first
  if constexpr (SHFL) {
    take(shfl_d(cost, lane ^ 16), __shfl(idx, lane ^ 16, 64));
    return;
  }
  const bool odd_row = (lane >> 4) & 1;
  const auto sl = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(cost), (unsigned)__double2loint(cost), false, false);
  const auto sh = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(cost), (unsigned)__double2hiint(cost), false, false);
  const auto si = __builtin_amdgcn_permlane16_swap((unsigned)idx, (unsigned)idx, false, false);
  const double oc = __hiloint2double((int)(odd_row ? sh[0] : sh[1]), (int)(odd_row ? sl[0] : sl[1]));
  take(oc, (int)(odd_row ? si[0] : si[1]));
}

// Must be called by every lane of the wave (wave-uniform control flow). `need` marks lanes that
// request an optimisation with inputs `in`; they receive (P_best, Chi_best). SHIP_UNIFORM: u_d, obs_l and
// obs_w are the same for every request and set in every lane's `in` (the AST kernels: the ships'
// configured desired speed and obstacle size), so they are not gathered from the requesting lane.
template <bool SHIP_UNIFORM = false, bool SHFL_ARGMIN = false>
__device__ void sbmpc_cooperative(bool need, const SbIn& in, int n_samp, double DT, double& p_best,
                                  double& chi_best) {
  SHIPSIM_LANE_CHECK(64, 4);
  const int lane = opaque_v(threadIdx.x) & 63;  // (opaque: no lane masks held across the caller's loop)
  const int half = lane >> 5;
  const int scen = lane & 31;
  uint64_t req = __ballot(need);
  diag::sb_stat_wave(0, req ? 1u : 0u);  // (the counters of sbmpc_cooperative_multi; nothing in the product build)
  while (req) {
    int src0 = __ffsll((unsigned long long)req) - 1;
    req &= req - 1;
    int src1 = -1;
    if (req) {
      src1 = __ffsll((unsigned long long)req) - 1;
      req &= req - 1;
    }
    diag::sb_stat_wave(1, 1u);
    diag::sb_stat_wave(2, src1 < 0 ? 1u : 0u);
    diag::sb_stat_wave(3, src1 < 0 ? 1u : 2u);
    int src = half ? src1 : src0;
    int srcc = src < 0 ? src0 : src;
    SbIn g;
    if constexpr (SHIP_UNIFORM) {
      g.u_d = in.u_d; g.obs_l = in.obs_l; g.obs_w = in.obs_w;
    } else {
      g.u_d = shfl_d(in.u_d, srcc); g.obs_l = shfl_d(in.obs_l, srcc); g.obs_w = shfl_d(in.obs_w, srcc);
    }
    g.chi_d = shfl_d(in.chi_d, srcc);
    g.os_x = shfl_d(in.os_x, srcc); g.os_y = shfl_d(in.os_y, srcc); g.os_v = shfl_d(in.os_v, srcc);
    g.ob_x = shfl_d(in.ob_x, srcc); g.ob_y = shfl_d(in.ob_y, srcc); g.ob_psi = shfl_d(in.ob_psi, srcc);
    g.ob_u = shfl_d(in.ob_u, srcc); g.ob_v = shfl_d(in.ob_v, srcc);
    g.p_last = shfl_d(in.p_last, srcc); g.chi_last = shfl_d(in.chi_last, srcc);
    g.ob_so = shfl_d(in.ob_so, srcc); g.ob_co = shfl_d(in.ob_co, srcc);
    double cost = INFINITY;
    int idx = 64;
    const bool split = src1 < 0;  // (uniform) one request this pass: both halves take it, each half of every horizon
    if ((split || src >= 0) && scen < 28) {
      cost = sbmpc_scenario_cost(g, n_samp, DT, scen >> 2, scen & 3, split ? half : -1);
      idx = scen;
    }
    // argmin over the half-wave; ties -> lowest scenario index (first strict improvement in the
    // reference's i-major / j-minor loop)
    scenario_argmin<SHFL_ARGMIN>(cost, idx, lane);
    const int best0 = __builtin_amdgcn_readlane(idx, 0);
    const int best1 = __builtin_amdgcn_readlane(idx, 32);
    if (lane == src0) {
      p_best = p_ca_of(best0 & 3);
      chi_best = (-30.0 + 10.0 * (best0 >> 2)) * (kPi / 180.0);
    }
    if (src1 >= 0 && lane == src1) {
      p_best = p_ca_of(best1 & 3);
      chi_best = (-30.0 + 10.0 * (best1 >> 2)) * (kPi / 180.0);
    }
  }
}

// SBMPC over a do_list of NOB obstacles (sbmpc.py:150-183; env.py:366-370 passes every obstacle ship):
// per scenario the worst obstacle's cost (cost_i = -1, then every strictly larger cost_k: the max of the costs),
// the scenario with the least worst cost wins (lowest index on ties). Slots of an env that duplicate its last
// ship repeat an obstacle, which changes neither the max nor the D_INIT test, and are not evaluated.
// Lanes: scenario = lane & 31 (28 used). With two or more requests pending a pass serves two, one per half-wave,
// each lane taking its scenario's obstacles in turn; with one request both halves serve it and split its
// obstacles — half h takes obstacles h, h + 2, … — and the two halves' worst costs are merged (lane ^ 32) before
// the argmin, so a lone request costs ⌈K / 2⌉ scenario evaluations per lane instead of K (the max over the same
// set of costs: the same value in either order).
template <int NOB>
struct SbMulti {
  double u_d, chi_d, os_x, os_y, os_v, p_last, chi_last;
  double ob_x[NOB], ob_y[NOB], ob_psi[NOB], ob_u[NOB], ob_v[NOB], obs_l[NOB], obs_w[NOB];
};

template <int NOB>
__device__ __forceinline__ void sbmpc_cooperative_multi(bool need, const SbMulti<NOB>& in, int n_obs, int n_samp, double DT,
                                        double& p_best, double& chi_best) {
  SHIPSIM_LANE_CHECK(64, 4);
  const int lane = opaque_v(threadIdx.x) & 63;
  const int half = lane >> 5;
  const int scen = lane & 31;
  uint64_t req = __ballot(need);
  diag::sb_stat_wave(0, req ? 1u : 0u);
  while (req) {
    // the counts re-derived per pass: tests on them are not hoisted out of this loop and held across it
    const int n_obs_p = opaque_s(n_obs), n_samp_p = opaque_s(n_samp);
    int src0 = __ffsll((unsigned long long)req) - 1;
    req &= req - 1;
    int src1 = -1;
    if (req) {
      src1 = __ffsll((unsigned long long)req) - 1;
      req &= req - 1;
    }
    const bool split = src1 < 0;  // (uniform) one request this pass: the halves split its obstacles
    diag::sb_stat_wave(1, 1u);
    diag::sb_stat_wave(2, split ? 1u : 0u);
    diag::sb_stat_wave(3, split ? 1u : 2u);
    int src = half ? src1 : src0;
    const int srcc = src < 0 ? src0 : src;
    SbIn g;
    g.u_d = shfl_d(in.u_d, srcc); g.chi_d = shfl_d(in.chi_d, srcc);
    g.os_x = shfl_d(in.os_x, srcc); g.os_y = shfl_d(in.os_y, srcc); g.os_v = shfl_d(in.os_v, srcc);
    g.p_last = shfl_d(in.p_last, srcc); g.chi_last = shfl_d(in.chi_last, srcc);
    double cost = INFINITY;
    int idx = 64;
    double worst = -1.0;
    bool any_far = false;
    const bool act = (split || src >= 0) && scen < 28;
    // obstacles in pairs (2j, 2j + 1): split, half h takes obstacle 2j + h; otherwise each lane both, in order
#pragma unroll
    for (int j = 0; j < (NOB + 1) / 2; ++j) {
      const int ka = 2 * j, kb = 2 * j + 1 < NOB ? 2 * j + 1 : 2 * j;
      if (ka >= n_obs_p) break;  // (wave-uniform) slots past the env's K obstacles duplicate the last one
      const bool b_ok = 2 * j + 1 < NOB && 2 * j + 1 < n_obs_p;
      for (int t = 0; t < (split ? 1 : 2); ++t) {  // (uniform trip count)
        const bool use_b = split ? half == 1 : t == 1;
        // this lane's obstacle, field by field (both candidates gathered, one kept: short live ranges)
        auto pick = [&](const double (&f)[NOB]) __attribute__((always_inline)) {
          const double a = shfl_d(f[ka], srcc);
          const double b = shfl_d(f[kb], srcc);
          return use_b ? b : a;
        };
        SbIn q = g;
        q.ob_x = pick(in.ob_x); q.ob_y = pick(in.ob_y); q.ob_psi = pick(in.ob_psi);
        q.ob_u = pick(in.ob_u); q.ob_v = pick(in.ob_v); q.obs_l = pick(in.obs_l); q.obs_w = pick(in.obs_w);
        const bool ok = act && (use_b ? b_ok : true);
        // an obstacle out of reach costs exactly sbmpc_h2 in every scenario (added once below)
        const bool far = ok && sbmpc_far(q, n_samp_p, DT);
        any_far = any_far || far;
        diag::sb_stat_lanes(4, (ok && !far) ? 1u : 0u);
        diag::sb_stat_lanes(5, far ? 1u : 0u);
        if (ok && !far) {
          sb_set_heading_trig(q);
          const double ck = sbmpc_scenario_cost(q, opaque_s(n_samp_p), DT, scen >> 2, scen & 3);
          if (ck > worst) worst = ck;
        }
      }
    }
    if (act && any_far) {
      const double h2 = sbmpc_h2(g, scen >> 2, scen & 3);
      if (h2 > worst) worst = h2;
    }
    if (split) {  // (uniform) the other half's worst over its obstacles (lane ^ 32)
      const double ow = shfl_d(worst, lane ^ 32);
      if (ow > worst) worst = ow;
    }
    if (act) {
      cost = worst;
      idx = scen;
    }
    scenario_argmin<true>(cost, idx, lane);
    const int best0 = __builtin_amdgcn_readlane(idx, 0);
    const int best1 = __builtin_amdgcn_readlane(idx, 32);
    if (lane == src0) {
      p_best = p_ca_of(best0 & 3);
      chi_best = (-30.0 + 10.0 * (best0 >> 2)) * (kPi / 180.0);
    }
    if (src1 >= 0 && lane == src1) {
      p_best = p_ca_of(best1 & 3);
      chi_best = (-30.0 + 10.0 * (best1 >> 2)) * (kPi / 180.0);
    }
  }
}
