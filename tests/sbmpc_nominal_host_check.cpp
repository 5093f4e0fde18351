// Stand-alone driver of the SBMPC nominal-scenario test's host half (ast_sac_amd/csrc/shipsim_sbmpc_nominal.hpp), built
// by tests/test_sbmpc_nominal_cpu.py with -fsanitize=address,undefined. Without arguments: the gap is the least own
// terms of the 27 other scenarios and the nominal scenario's are 0 at the rest memory, the answer's constants, the
// memory and NaN guards, and the bound's monotony in the distance. With `eval`: reads "n tf dt" and n request rows of
// shipsim_sbmpc_eval's layout from stdin and prints each row's flag and ratio, of the test with sin / cos(chi_d) and of
// the form the streams' tick evaluates on the split course, for the tests' comparisons with the oracle and the device.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "shipsim_sbmpc_nominal.hpp"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                               \
    }                                                         \
  } while (0)

using namespace shipsim;

// a request row (SHIPSIM_SBMPC_IN doubles) as the device entry reads it
static SbIn from_row(const double* r) {
  SbIn q;
  q.p_last = r[0]; q.chi_last = r[1]; q.u_d = r[2]; q.chi_d = r[3];
  q.os_x = r[4]; q.os_y = r[5]; q.os_v = r[8];
  q.ob_x = r[10]; q.ob_y = r[11]; q.ob_psi = r[12]; q.ob_u = r[13]; q.ob_v = r[14];
  q.ob_so = sin(q.ob_psi); q.ob_co = cos(q.ob_psi);
  q.obs_l = r[15]; q.obs_w = r[16];
  return q;
}

static int eval_mode() {
  int n = 0;
  double tf = 0, dt = 0;
  if (scanf("%d %lf %lf", &n, &tf, &dt) != 3 || n < 0 || !(dt > 0)) return 2;
  std::vector<double> rows((size_t)n * SHIPSIM_SBMPC_IN);
  for (double& v : rows)
    if (scanf("%lf", &v) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    const SbIn q = from_row(&rows[(size_t)i * SHIPSIM_SBMPC_IN]);
    const SbNominal r = sbmpc_nominal_holds(q, (int)(tf / dt), dt);
    double seg_sin, seg_cos, a;  // the form the streams' tick evaluates, on the split course (as the device entry)
    sbmpc_nominal_split_course(q.chi_d, seg_sin, seg_cos, a);
    const SbNominal g = sbmpc_nominal_holds_seg(q, seg_sin, seg_cos, a, (int)(tf / dt), dt);
    printf("%d %.17g %d %.17g\n", r.holds ? 1 : 0, r.ratio, g.holds ? 1 : 0, g.ratio);
  }
  return 0;
}

// own ship at the origin heading north (chi_d = 0) at 5 m/s, the obstacle ship `east` metres abeam on the opposite
// course: the closest approach is `east`
static SbIn abeam(double east) {
  SbIn q = SbIn{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  q.p_last = 1.0; q.chi_last = 0.0; q.u_d = 5.0; q.chi_d = 0.0;
  q.ob_x = east; q.ob_y = 1500.0; q.ob_psi = kPi; q.ob_u = 5.0;
  q.ob_so = sin(q.ob_psi); q.ob_co = cos(q.ob_psi);
  q.obs_l = 80.0; q.obs_w = 16.0;
  return q;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "eval")) return eval_mode();

  // the rest memory: the nominal scenario's own terms are 0 exactly, the gap is the least of the 27 others'
  SbIn rest = SbIn{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  rest.p_last = 1.0;
  const double gap = sbmpc_nominal_gap();
  CHECK(sbmpc_h2(rest, kSbNominalChi, kSbNominalP) == 0.0);
  double least = std::numeric_limits<double>::infinity();
  for (int ichi = 0; ichi < kSbNChi; ++ichi)
    for (int jp = 0; jp < kSbNP; ++jp) {
      const double h2 = sbmpc_h2(rest, ichi, jp);
      CHECK(h2 >= 0.0);
      if (ichi != kSbNominalChi || jp != kSbNominalP) {
        CHECK(h2 >= gap);
        least = h2 < least ? h2 : least;
      }
    }
  CHECK(least == gap && gap > 0.0);
  const double ten = 10.0 * kPi / 180.0;
  CHECK(fabs(gap - 50.0 * ten * ten) <= 1e-15 * gap && gap > 1.52 && gap < 1.53);
  rest.chi_last = -0.0;  // (a negative zero is the rest value too: every difference from it is the same)
  CHECK(sbmpc_h2(rest, kSbNominalChi, kSbNominalP) == 0.0 && sbmpc_h2(rest, kSbNominalChi + 1, kSbNominalP) == gap);
  // the answer: scenario 15's (P_ca, Chi_ca) as the pass forms them, 1.0 and +0.0
  CHECK(kSbNominalChi * kSbNP + kSbNominalP == 15);
  CHECK(p_ca_of(kSbNominalP) == 1.0);
  const double chi15 = (-30.0 + 10.0 * kSbNominalChi) * (kPi / 180.0);
  CHECK(chi15 == 0.0 && !signbit(chi15) && chi_ca_of(kSbNominalChi) == chi15);

  // far abeam holds, near does not; the ratio falls with the fourth power of the closest approach
  const int n_samp = 50;
  const double DT = 20.0;
  CHECK(sbmpc_nominal_holds(abeam(1200.0), n_samp, DT).holds);
  CHECK(!sbmpc_nominal_holds(abeam(100.0), n_samp, DT).holds);
  CHECK(!sbmpc_nominal_holds(abeam(0.5), n_samp, DT).holds);  // (closer than 1 m: refused whatever the bound)
  double prev = std::numeric_limits<double>::infinity();
  int flips = 0;
  bool was = false;
  for (double east = 50.0; east <= 1500.0; east += 12.5) {
    const SbNominal r = sbmpc_nominal_holds(abeam(east), n_samp, DT);
    CHECK(r.ratio > 0.0 && r.ratio < prev);
    CHECK(r.holds == (r.ratio < 1.0));
    flips += (r.holds != was);
    was = r.holds;
    prev = r.ratio;
  }
  CHECK(flips == 1 && was);
  {
    const SbNominal a = sbmpc_nominal_holds(abeam(400.0), n_samp, DT), b = sbmpc_nominal_holds(abeam(800.0), n_samp, DT);
    CHECK(fabs(a.ratio / b.ratio - 16.0) < 1e-9);
  }
  // the closest approach counts, not the distance now: the same 1500 m away, but dead ahead on the opposite course
  {
    SbIn q = abeam(0.0);
    CHECK(!sbmpc_nominal_holds(q, n_samp, DT).holds);
    q.ob_psi = 0.0; q.ob_so = 0.0; q.ob_co = 1.0;  // same course and speed: the distance stays 1500 m
    CHECK(sbmpc_nominal_holds(q, n_samp, DT).holds);
  }
  // the form the streams' tick evaluates: the same verdict and, to rounding, the same ratio for any split of the
  // course into a segment angle and a correction's argument, small, large and infinite arguments included
  for (double chi : {-4.0, -kPi, -1.0, -1e-9, 0.0, 0.3, kPi / 2, 3.0, kPi, 4.0})
    for (double east : {150.0, 250.0, 350.0, 1200.0}) {
      SbIn q = abeam(east);
      q.chi_d = chi;
      const SbNominal r = sbmpc_nominal_holds(q, n_samp, DT);
      double ss, sc, a;
      sbmpc_nominal_split_course(chi, ss, sc, a);
      const SbNominal g = sbmpc_nominal_holds_seg(q, ss, sc, a, n_samp, DT);
      CHECK(fabs(g.ratio / r.ratio - 1.0) < 1e-9 && (g.holds == r.holds || fabs(r.ratio - 1.0) < 1e-9));
      for (double arg : {-1e6, -7.0, -0.5, 0.0, 1e-12, 2.0, 1e9}) {  // chi = -(alpha + atan(arg))
        const double alpha = -chi - atan(arg);
        const SbNominal h = sbmpc_nominal_holds_seg(q, sin(alpha), cos(alpha), arg, n_samp, DT);
        CHECK(fabs(h.ratio / r.ratio - 1.0) < 1e-6 && (h.holds == r.holds || fabs(r.ratio - 1.0) < 1e-6));
      }
      CHECK(!sbmpc_nominal_holds_seg(q, 0.0, 1.0, std::numeric_limits<double>::infinity(), n_samp, DT).holds);
      CHECK(!sbmpc_nominal_holds_seg(q, 0.0, 1.0, std::numeric_limits<double>::quiet_NaN(), n_samp, DT).holds);
    }
  // any other memory value refuses
  for (int ichi = 0; ichi < kSbNChi; ++ichi)
    for (int jp = 0; jp < kSbNP; ++jp) {
      SbIn q = abeam(1200.0);
      q.p_last = p_ca_of(jp);
      q.chi_last = chi_ca_of(ichi);
      CHECK(sbmpc_nominal_holds(q, n_samp, DT).holds == (ichi == kSbNominalChi && jp == kSbNominalP));
    }
  // a NaN in any field it reads refuses (obs_w and ob_psi are not read), and so does an infinite position, speed or
  // course
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double SbIn::*fields[] = {&SbIn::u_d,  &SbIn::chi_d, &SbIn::os_x, &SbIn::os_y,  &SbIn::os_v,   &SbIn::ob_x,     &SbIn::ob_y,
                            &SbIn::ob_u, &SbIn::ob_v,  &SbIn::ob_so, &SbIn::ob_co, &SbIn::obs_l, &SbIn::p_last, &SbIn::chi_last};
  for (double bad : {nan, inf, -inf}) {
    int k = 0;
    for (double SbIn::*f : fields) {
      if (bad != bad || k++ < 11) {  // (the first eleven: positions, speeds, course and heading terms)
        SbIn q = abeam(1200.0);
        q.*f = bad;
        CHECK(!sbmpc_nominal_holds(q, n_samp, DT).holds);
      }
    }
    CHECK(!sbmpc_nominal_holds(abeam(1200.0), n_samp, bad).holds);
  }
  // degenerate horizons: no relative motion (ww = 0), one sample
  {
    SbIn q = abeam(1200.0);
    q.ob_psi = 0.0; q.ob_so = 0.0; q.ob_co = 1.0;
    CHECK(sbmpc_nominal_holds(q, 1, DT).holds && sbmpc_nominal_holds(q, 2, DT).holds);
  }
  printf("sbmpc nominal host OK gap %.17g\n", gap);
  return 0;
}
