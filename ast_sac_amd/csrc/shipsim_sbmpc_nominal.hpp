// shipsim_sbmpc_nominal.hpp — the SBMPC request as both sides see it, the scenarios' own cost terms, and the test that
// answers a request without the optimiser's pass: "the nominal scenario (P_ca = 1, Chi_ca = 0) provably wins".
// Plain C++17 with no HIP include, in the manner of the *_host.hpp halves: shipsim_sbmpc.hpp includes it for the
// kernels, tests/sbmpc_nominal_host_check.cpp compiles it with the host compiler.
#pragma once
#include <math.h>

#include "shipsim_types.hpp"  // SHIPSIM_HD, kPi

namespace shipsim {

struct SbIn {
  double u_d, chi_d, os_x, os_y, os_v, ob_x, ob_y, ob_psi, ob_u, ob_v, obs_l, obs_w, p_last, chi_last;
  double ob_so, ob_co;  // sin / cos(ob_psi): the AST kernels pass the obstacle ship's carried sin/cos(yaw)
};

constexpr int kSbNChi = 7, kSbNP = 4;  // Chi_ca_ = -30 .. 30 deg in steps of 10, P_ca_ = [0.4, 0.6, 0.8, 1.0]
constexpr int kSbNominalChi = 3, kSbNominalP = 3;  // the nominal scenario: Chi_ca = 0, P_ca = 1 (scenario index 15)

// SBMPCParams.P_ca_ = [0.4, 0.6, 0.8, 1.0] (sbmpc.py:36) by selects: a per-lane indexed constant array would be
// a memory load on the scenario's critical path
SHIPSIM_HD double p_ca_of(int jp) {
  return jp == 0 ? 0.4 : (jp == 1 ? 0.6 : (jp == 2 ? 0.8 : 1.0));
}
SHIPSIM_HD double chi_ca_of(int ichi) { return (-30.0 + 10.0 * ichi) * (kPi / 180.0); }

// the scenario's own terms of the cost (sbmpc.py:200-214: P_ca, Chi_ca and their changes); the whole
// cost when no obstacle sample comes within max_d_safe
SHIPSIM_HD double sbmpc_h2(const SbIn& in, int ichi, int jp) {
  const double P_ca = p_ca_of(jp);
  const double Chi_ca = (-30.0 + 10.0 * ichi) * (kPi / 180.0);
  const double dChi0 = Chi_ca - in.chi_last;
  return 25 * (1 - P_ca) + 30 * (Chi_ca * Chi_ca) + 20 * fabs(in.p_last - P_ca) +
         ((dChi0 > 0) ? 20 * dChi0 * dChi0 : (dChi0 < 0 ? 30 * dChi0 * dChi0 : 0));
}

// With the optimiser's memory at its rest value (p_last = 1, chi_last = 0) the nominal scenario's own terms are 0
// exactly, and the least own terms of the other 27 scenarios are those of (Chi_ca = +10 deg, P_ca = 1):
// 50 · (10π/180)² ≈ 1.523 (tests/sbmpc_nominal_host_check.cpp asserts both). Every scenario's cost is its own terms
// plus a collision cost H1 >= 0, so the nominal scenario wins outright, with no tie, once H1(nominal) < this gap.
SHIPSIM_HD double sbmpc_nominal_gap() {
  SbIn rest = SbIn{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  rest.p_last = 1.0;
  rest.chi_last = 0.0;
  return sbmpc_h2(rest, kSbNominalChi + 1, kSbNominalP);
}

struct SbNominal {
  bool holds;    // the pass would return (p_ca_of(3), chi_ca_of(3)) = (1.0, +0.0): it need not run
  double ratio;  // ub / gap, ub with its slack (tests; finite inputs): at the rest memory holds is ratio < 1, up to the
                 // rounding of the ratio's own division
};

// An upper bound on the nominal scenario's collision cost that needs no horizon, against the gap. Each sample costs
// k_coll · |vs − vo|² · (1/t) · (d_safe/dist)⁴ or 0, with k_coll = 1e-6 · 25 · obs_l, t >= DT,
// |vs − vo|² <= (|vs| + |vo|)², |vs|² <= u_d² + os_v² (sample 0 carries the sway, later ones none), and
// dist² >= d2 = min(|e0|², |P1 + k·W|²): the distance now and the continuous closest approach of the two straight
// lines after sample 0, k clamped to [0, n_samp − 2], formed as sbmpc_scenario_cost's skip test forms them for
// psi_d = chi_d, ud = u_d. So
//   H1 <= ub = k_coll · (|vs| + |vo|)² · d_safe⁴ / (d2² · DT) · slack
// where slack = (1 + 1e-6) / (1 − 1e-3)⁴ swallows every rounding difference between this evaluation and the pass's
// own (positions differ by ~1e-10 m against a factor that shrinks every distance of 1 m or more by at least 1e-3 m,
// that test's margin; velocities and the cost's own products by ulps against 1e-6). The comparison is written
// without a division, and so that a NaN anywhere makes it false. (sp, cp): sin / cos(chi_d); they need not be the
// pass's own bits, the margins cover any correctly formed pair.
SHIPSIM_HD SbNominal sbmpc_nominal_holds_sc(const SbIn& in, double sp, double cp, int n_samp, double DT) {
  const double os_l = 25.0, d_safe = 1000.0;
  const double ud = in.u_d;
  const double q11 = -sp, q12 = cp, q21 = cp, q22 = sp;
  const double vox = -in.ob_so * in.ob_u + in.ob_co * in.ob_v, voy = in.ob_co * in.ob_u + in.ob_so * in.ob_v;
  const double e0x = in.ob_x - in.os_x, e0y = in.ob_y - in.os_y;
  const double p1x = (in.ob_x + vox * DT) - (in.os_x + DT * (q11 * ud + q12 * in.os_v));
  const double p1y = (in.ob_y + voy * DT) - (in.os_y + DT * (q21 * ud + q22 * in.os_v));
  const double wx = (vox - q11 * ud) * DT, wy = (voy - q21 * ud) * DT;
  const double ww = wx * wx + wy * wy;
  const double iww = ww > 0 ? 1.0 / ww : 0.0;
  double k = ww > 0 ? -(p1x * wx + p1y * wy) * iww : 0.0;
  k = k < 0 ? 0 : (k > n_samp - 2 ? n_samp - 2 : k);
  const double mx = p1x + k * wx, my = p1y + k * wy;
  const double e2 = e0x * e0x + e0y * e0y, m2 = mx * mx + my * my;
  // (|vs| + |vo|)² = |vs|² + |vo|² + 2·sqrt(|vs|²·|vo|²): one root
  const double vs2 = ud * ud + in.os_v * in.os_v, vo2 = vox * vox + voy * voy;
  const double v2 = vs2 + vo2 + 2.0 * sqrt(vs2 * vo2);
  const double k_coll = 1e-6 * os_l * in.obs_l;
  constexpr double shrink = (1.0 - 1e-3) * (1.0 - 1e-3) * (1.0 - 1e-3) * (1.0 - 1e-3);
  const double num = k_coll * v2 * ((d_safe * d_safe) * (d_safe * d_safe)) * (1.0 + 1e-6);  // ub · (d2² · den)
  const double den = sbmpc_nominal_gap() * DT * shrink;                                     // gap · (... / d2²)
  const bool rest = (in.p_last == 1.0) & (in.chi_last == 0.0);
  // both distances at least 1 m (the relative shrink covers the absolute margin) and finite, and the bound below the
  // gap at each
  const double re = den * (e2 * e2), rm = den * (m2 * m2);
  const bool far = (e2 >= 1.0) & (m2 >= 1.0) & (num < re) & (num < rm) & (re < INFINITY) & (rm < INFINITY);
  SbNominal r;
  r.holds = rest & far;
  const double d2 = m2 < e2 ? m2 : e2;
  r.ratio = num / (den * (d2 * d2));
  return r;
}

SHIPSIM_HD SbNominal sbmpc_nominal_holds(const SbIn& in, int n_samp, double DT) {
  return sbmpc_nominal_holds_sc(in, sin(in.chi_d), cos(in.chi_d), n_samp, DT);
}

// The test as the streams' tick evaluates it, without chi_d: the desired course is chi_d = -(seg_alpha + atan(a)),
// seg_alpha the LOS segment's angle with its carried sine and cosine (seg_sin, seg_cos) and a the course
// correction's argument, so its sine and cosine follow from cos(atan(a)) = 1 / sqrt(1 + a²) and
// sin(atan(a)) = a · cos(atan(a)) by the angle addition, and the atan is left to the requests that go to the pass
// (in.chi_d is not read). An infinite a gives NaN and refuses.
SHIPSIM_HD SbNominal sbmpc_nominal_holds_seg(const SbIn& in, double seg_sin, double seg_cos, double a, int n_samp,
                                             double DT) {
#ifdef __HIP_DEVICE_COMPILE__
  const double ct = rsqrt(1.0 + a * a);
#else
  const double ct = 1.0 / sqrt(1.0 + a * a);
#endif
  const double st = a * ct;
  const double sp = -(seg_sin * ct + seg_cos * st), cp = seg_cos * ct - seg_sin * st;
  return sbmpc_nominal_holds_sc(in, sp, cp, n_samp, DT);
}

// A course split into a segment angle and a correction's argument that give it back, for checking the form above
// on requests that come with chi_d alone (shipsim_sbmpc_nominal, tests/sbmpc_nominal_host_check.cpp): the correction
// takes half of the wrapped course, atan(a) = -w / 2 with w = chi_d wrapped to [-π, π], so a runs over all reals, and
// seg_alpha = -chi_d + w / 2.
SHIPSIM_HD void sbmpc_nominal_split_course(double chi_d, double& seg_sin, double& seg_cos, double& a) {
  const double w = atan2(sin(chi_d), cos(chi_d));
  const double alpha = -chi_d + 0.5 * w;
  seg_sin = sin(alpha);
  seg_cos = cos(alpha);
  a = -tan(0.5 * w);
}

}  // namespace shipsim
