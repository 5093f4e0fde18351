// Stand-alone driver of shipsim_resample's arithmetic (ast_sac_amd/csrc/shipsim_resample_host.hpp), built by
// tests/test_resample_cpu.py with -fsanitize=address,undefined. It runs the stages of shipsim_resample.hip in their
// order, sequentially, on exactly-sized heap arrays — so that an index past an array is caught — through the same
// functions the kernels call, and prints what they give for tests/resample_ref.py to be compared with.
//
// Input (stdin, or the file named by the first argument), every number in hex:
//   n, then n weights and n potentials as the bits of doubles, then k and k pairs "hi lo" of offset bits.
// Output: "status", "e", "q" (n words), "Q", "total" (bits), then per pair "U", "sorted" (n), "wsorted" (n, bits),
// "inplace" (n), "winplace" (n, bits). With a status other than 0 the q / Q lines are left out and each pair prints
// the identity and the weights as given.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "shipsim_resample_host.hpp"

namespace RS = resample_host;

static double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
static uint64_t to_bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

// the two-level inclusive scan: loc within the tile, off before the tile
static void scan2(const std::vector<uint64_t>& v, std::vector<uint64_t>& loc, std::vector<uint64_t>& off) {
  const int n = (int)v.size();
  loc.assign(n, 0);
  off.assign(RS::tiles(n), 0);
  uint64_t before = 0;
  for (int b = 0; b < RS::tiles(n); ++b) {
    off[b] = before;
    uint64_t acc = 0;
    for (int i = b * RS::kTile; i < n && i < (b + 1) * RS::kTile; ++i) loc[i] = acc += v[i];
    before += acc;
  }
}

template <class T>
static void print(const char* name, const std::vector<T>& v) {
  printf("%s", name);
  for (const T& x : v) printf(" %" PRIx64, (uint64_t)x);
  printf("\n");
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  uint64_t n64;
  if (fscanf(f, "%" SCNx64, &n64) != 1 || n64 < 1 || n64 > (uint64_t)RS::kMaxN) return 2;
  const int n = (int)n64;
  std::vector<double> w(n), pot(n);
  for (std::vector<double>* a : {&w, &pot})
    for (int i = 0; i < n; ++i) {
      uint64_t b;
      if (fscanf(f, "%" SCNx64, &b) != 1) return 2;
      (*a)[i] = from_bits(b);
    }
  uint64_t k;
  if (fscanf(f, "%" SCNx64, &k) != 1) return 2;
  std::vector<uint64_t> his(k), los(k);
  for (uint64_t c = 0; c < k; ++c)
    if (fscanf(f, "%" SCNx64 " %" SCNx64, &his[c], &los[c]) != 2) return 2;

  // mass, maximum, validity (rs_mass_kernel, rs_head_kernel)
  double m = 0.0;
  for (int i = 0; i < n; ++i) {
    const double p = w[i] * pot[i];
    if (!RS::mass_ok(p)) m = -1.0;
    else if (m >= 0.0 && p > m) m = p;
  }
  const int status = m < 0.0 ? RS::kBadMass : (m == 0.0 ? RS::kNoMass : RS::kOk);
  int e = 0;
  if (status == RS::kOk) (void)frexp(m, &e);
  printf("status %x\ne %x\n", status, (unsigned)e);

  std::vector<uint64_t> q(n, 0), cl, toff;
  uint64_t Q = 0;
  if (status == RS::kOk) {
    // quantise and scan (rs_quant_kernel, rs_offsets_kernel)
    for (int i = 0; i < n; ++i) q[i] = RS::quantise(w[i] * pot[i], e);
    scan2(q, cl, toff);
    Q = toff.back() + cl.back();
    for (int i = 0; i < n; ++i)
      if (RS::q_of(cl.data(), i) != q[i]) return 3;
    print("q", q);
    printf("Q %" PRIx64 "\n", Q);
  }
  printf("total %" PRIx64 "\n", status == RS::kOk ? to_bits(RS::total_mass(Q, e)) : to_bits(0.0));

  for (uint64_t c = 0; c < k; ++c) {
    std::vector<int32_t> sorted(n), inplace(n);
    std::vector<double> wsorted(n), winplace(n);
    uint64_t U = 0;
    if (status != RS::kOk) {
      for (int j = 0; j < n; ++j) sorted[j] = inplace[j] = j, wsorted[j] = winplace[j] = w[j];
    } else {
      U = RS::mod128(his[c], los[c], Q);
      const uint64_t s = Q / (uint64_t)n, r = Q % (uint64_t)n;
      const double qd = (double)Q;
      // select, and the clone weight per source (rs_select_kernel)
      std::vector<double> wsrc(n);
      for (int j = 0; j < n; ++j) {
        sorted[j] = RS::search2(toff.data(), cl.data(), n, RS::position((uint64_t)j, s, r, U, (uint64_t)n), RS::kAll);
        wsrc[j] = q[j] ? RS::clone_weight(w[j], qd, n, q[j]) : 0.0;
      }
      // runs, the packed scan, the fill (rs_runs_kernel, rs_pair_kernel, rs_offsets_kernel, rs_finish_kernel)
      std::vector<int32_t> first(n, 0), last(n, 0);
      for (int j = 0; j < n; ++j) {
        const int sj = sorted[j];
        if (j == 0 || sorted[j - 1] != sj) first[sj] = j;
        if (j == n - 1 || sorted[j + 1] != sj) last[sj] = j + 1;
      }
      std::vector<uint64_t> pair(n), al, toff2;
      for (int i = 0; i < n; ++i) pair[i] = RS::packed_pair(last[i] - first[i]);
      scan2(pair, al, toff2);
      for (int i = 0; i < n; ++i) inplace[i] = RS::in_place_source(i, last[i] - first[i], toff2.data(), al.data(), n);
      for (int j = 0; j < n; ++j) wsorted[j] = wsrc[sorted[j]], winplace[j] = wsrc[inplace[j]];
    }
    printf("U %" PRIx64 "\n", U);
    print("sorted", sorted);
    std::vector<uint64_t> bits(n);
    for (int j = 0; j < n; ++j) bits[j] = to_bits(wsorted[j]);
    print("wsorted", bits);
    print("inplace", inplace);
    for (int j = 0; j < n; ++j) bits[j] = to_bits(winplace[j]);
    print("winplace", bits);
  }
  if (f != stdin) fclose(f);
  return 0;
}
