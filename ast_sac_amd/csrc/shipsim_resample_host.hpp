// shipsim_resample_host.hpp — the integer arithmetic of shipsim_resample (include/shipsim.h): quantisation of the
// masses, the 128-by-64 remainder, the systematic positions, the searches, the in-place arrangement, the weights and
// the caller's workspace as a table of offsets. Free of the device and of the handle (plain C++17), so that it can be
// compiled and driven on its own: tests/test_resample_cpu.py builds it into a stand-alone program
// (tests/resample_host_check.cpp) with -fsanitize=address,undefined. The kernels of shipsim_resample.hip call the same
// functions, so GPU, host program and the Python restatement (tests/resample_ref.py) agree bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace resample_host {

constexpr int kTile = 1024;       // the scan tile T: envs per block of the tile scans (256 threads x 4)
constexpr int kMaxN = 1 << 22;    // SHIPSIM_RESAMPLE_MAX_N
constexpr int kShift = 40;        // the largest mass quantises into [2^39, 2^40]
constexpr uint32_t kPhiloxTag = 0x52455341u;  // third counter word of the offset's Philox block
constexpr int kSorted = 0, kInPlace = 1;      // SHIPSIM_RESAMPLE_SORTED / _IN_PLACE
constexpr int kOk = 0, kNoMass = 1, kBadMass = 2;  // status

RS_HD constexpr int tiles(int n) { return (n + kTile - 1) / kTile; }

// What one thread works out once per call and every later stage reads (the head of the workspace).
struct Head {
  double m;        // the largest mass
  int32_t e;       // m = f * 2^e, f in [0.5, 1)
  int32_t status;  // kOk / kNoMass / kBadMass
  uint64_t Q;      // sum of the quantised masses
  uint64_t U;      // the offset, uniform on [0, Q)
  uint64_t s, r;   // Q = s * n + r
  double qd;       // (double)Q
};

// The caller's workspace: byte offsets of its arrays (every one on a multiple of 256) and its size.
//   head      Head
//   part      [tiles] double: the largest mass of a tile, -1 for a tile holding a negative or non-finite one
//   tsum/toff [tiles] u64: a tile's sum of q, and the sum of the tiles before it
//   tsum2/toff2 [tiles] u64: the same of the in-place stage's packed pair (surplus | empty << 32)
//   cl        [n] u64: inclusive sum of q within the env's tile
//   al        [n] u64: inclusive sum of the packed pair within the env's tile
//   wsrc      [n] double: the weight a clone of env i gets
//   sel       [n] int32: the sorted selection
//   first/last [n] int32: where env i's run in sel begins and ends (both 0: not selected)
struct Layout {
  int64_t head, part, tsum, toff, tsum2, toff2, cl, al, wsrc, sel, first, last, bytes;
};
constexpr int64_t r256(int64_t b) { return (b + 255) & ~(int64_t)255; }
constexpr Layout layout(int n) {
  Layout L{};
  const int64_t nt = tiles(n), N = n;
  int64_t o = 0;
  L.head = o; o += r256((int64_t)sizeof(Head));
  L.part = o; o += r256(nt * 8);
  L.tsum = o; o += r256(nt * 8);
  L.toff = o; o += r256(nt * 8);
  L.tsum2 = o; o += r256(nt * 8);
  L.toff2 = o; o += r256(nt * 8);
  L.cl = o; o += r256(N * 8);
  L.al = o; o += r256(N * 8);
  L.wsrc = o; o += r256(N * 8);
  L.sel = o; o += r256(N * 4);
  L.first = o; o += r256(N * 4);
  L.last = o; o += r256(N * 4);
  L.bytes = o;
  return L;
}
static_assert(layout(1).bytes < layout(kTile + 1).bytes && layout(kMaxN).bytes < ((int64_t)1 << 28),
              "the workspace grows with n and stays under 256 MiB");

// a mass is usable if it is finite and not negative (-0 counts as 0)
RS_HD inline bool mass_ok(double p) { return p >= 0.0 && p <= 1.7976931348623157e308; }

// q = ceil(p * 2^(40 - e)) for 0 <= p <= m < 2^e: at most 2^40, and >= 1 whenever p > 0
RS_HD inline uint64_t quantise(double p, int e) { return (uint64_t)ceil(ldexp(p, kShift - e)); }

// Philox4x32-10 on one counter block
RS_HD inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
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
// the offset's 128 bits: the block keyed by seed on {counter lo, counter hi, tag, 0}
RS_HD inline void offset_bits(uint64_t seed, int64_t counter, uint64_t* hi, uint64_t* lo) {
  uint32_t c[4] = {(uint32_t)(uint64_t)counter, (uint32_t)((uint64_t)counter >> 32), kPhiloxTag, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  *hi = (uint64_t)c[0] | ((uint64_t)c[1] << 32);
  *lo = (uint64_t)c[2] | ((uint64_t)c[3] << 32);
}

// ((hi << 64) | lo) mod Q for 1 <= Q <= 2^62, without a 128-bit division: the remainder so far stays below Q, so
// doubling it and taking in one bit stays below 2^63
RS_HD constexpr uint64_t mod128(uint64_t hi, uint64_t lo, uint64_t Q) {
  uint64_t x = hi % Q;
  for (int b = 63; b >= 0; --b) {
    x = (x << 1) | ((lo >> b) & 1u);
    if (x >= Q) x -= Q;
  }
  return x;
}
static_assert(mod128(0, 17, 5) == 2 && mod128(1, 0, 10) == 6 && mod128(~0ull, ~0ull, 1ull << 62) == (1ull << 62) - 1 &&
                  mod128(3, 1, 7) == (3 * 2 + 1) % 7,  // 2^64 = 2 (mod 7)
              "mod128");

// the j-th systematic position floor((j * Q + U) / n) with Q = s * n + r; every term below 2^63
RS_HD constexpr uint64_t position(uint64_t j, uint64_t s, uint64_t r, uint64_t U, uint64_t n) {
  return j * s + (j * r + U) / n;
}

// smallest i in [lo, hi) with (a[i] & mask) > t, or hi: a is non-decreasing under the mask
RS_HD inline int upper_bound(const uint64_t* a, int lo, int hi, uint64_t t, uint64_t mask) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((a[mid] & mask) > t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The scans are kept in two levels — loc[i], the inclusive sum within env i's tile, and off[b], the sum of the tiles
// before tile b — so that no pass has to add the two. The smallest i with (off[tile(i)] + loc[i]) & mask > t, for
// t below the grand total: the last tile whose offset is <= t holds it (its own sum is then positive).
RS_HD inline int search2(const uint64_t* off, const uint64_t* loc, int n, uint64_t t, uint64_t mask) {
  const int b = upper_bound(off, 0, tiles(n), t, mask) - 1;
  const int lo = b * kTile, hi = lo + kTile < n ? lo + kTile : n;
  const int i = upper_bound(loc, lo, hi, t - (off[b] & mask), mask);
  return i < n ? i : n - 1;  // (never taken for t below the total; keeps a caller's index inside the arrays)
}

constexpr uint64_t kAll = ~(uint64_t)0, kLo32 = 0xFFFFFFFFull;

// q of env i from the tile-local scan
RS_HD inline uint64_t q_of(const uint64_t* cl, int i) { return cl[i] - (i % kTile ? cl[i - 1] : 0); }

// the weight of a clone of an env of weight w and quantised mass q > 0 among n: three IEEE operations
RS_HD inline double clone_weight(double w, double qd, int n, uint64_t q) { return w * (qd / ((double)n * (double)q)); }

// the estimate of the total mass that the weights preserve
RS_HD inline double total_mass(uint64_t Q, int e) { return ldexp((double)Q, e - kShift); }

// in-place arrangement: what env i adds to the packed scan, from its count c in the sorted selection
RS_HD constexpr uint64_t packed_pair(int c) { return (uint64_t)(c > 1 ? c - 1 : 0) | ((uint64_t)(c == 0) << 32); }
// ... and slot i's source: itself if it was selected; otherwise, being the k-th empty slot (k = empties up to and
// including i, minus one), the source of the k-th surplus clone
RS_HD inline int in_place_source(int i, int c, const uint64_t* toff2, const uint64_t* al, int n) {
  if (c > 0) return i;
  const uint64_t k = ((toff2[i / kTile] + al[i]) >> 32) - 1;
  return search2(toff2, al, n, k, kLo32);
}

}  // namespace resample_host
