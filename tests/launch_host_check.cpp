// Stand-alone driver of the step kernels' list and selection (ast_sac_amd/csrc/shipsim_launch_host.hpp), built by
// tests/test_launch_host_cpu.py with -fsanitize=address,undefined: every handle the library can hold, at every
// entry point, against the list the library expands into its table of kernels.
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "shipsim_launch_host.hpp"

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                               \
    }                                                         \
  } while (0)

namespace L = launch_host;

struct Row {
  int key;
  bool detailed;
  int collav, lpe;
  bool rec;
  int mode, slots;
};
static const Row kRows[] = {
#define ROW(D, CA, LPE, REC, MODE, SLOTS) {L::step_key(D, CA, LPE, REC, MODE, SLOTS), D, CA, LPE, REC, MODE, SLOTS},
    SHIPSIM_STEP_KERNELS(ROW)
#undef ROW
};

static const Row* find(int key) {
  for (const Row& r : kRows)
    if (r.key == key) return &r;
  return nullptr;
}

int main() {
  // (c) the list: 102 rows, no row twice
  const size_t n_rows = sizeof(kRows) / sizeof(kRows[0]);
  CHECK(n_rows == 102);
  std::set<int> keys;
  for (const Row& r : kRows) keys.insert(r.key);
  CHECK(keys.size() == n_rows);

  std::set<int> selected;
  int refused = 0, served = 0;
  const int lpes[4] = {2, 4, 8, 16};
  for (int mach = 0; mach <= 1; ++mach)
    for (int collav = 0; collav <= 2; ++collav)
      for (int n_ships = 2; n_ships <= SHIPSIM_MAX_SHIPS; ++n_ships)
        for (int lpe : lpes)
          for (int rec = 0; rec <= 1; ++rec)
            for (int wx = 0; wx <= 1; ++wx)
              for (int entry = 0; entry <= 2; ++entry) {
                const L::Selection s = L::select(mach, collav, n_ships, lpe, rec != 0, wx != 0, (L::Entry)entry);
                // (d) refused: K > 1 with simplified machinery or collav simple; weather with simplified machinery,
                // collav simple or recording; streams with recording — and nothing else
                const bool narrow = mach == SHIPSIM_MACH_SIMPLIFIED || collav == SHIPSIM_COLLAV_SIMPLE;
                const bool want_refused = (n_ships > 2 && narrow) || (wx && (narrow || rec)) || (entry != L::kStep && rec);
                CHECK((s.why != nullptr) == want_refused);
                if (s.why) {
                  CHECK(strlen(s.why) > 0);
                  ++refused;
                  continue;
                }
                ++served;
                // (a) a row of the list, and the row this handle asked for
                const Row* r = find(s.key);
                CHECK(r != nullptr);
                selected.insert(s.key);
                CHECK(r->detailed == (mach == SHIPSIM_MACH_DETAILED) && r->collav == collav && r->lpe == s.lpe);
                CHECK(r->mode == (entry | (wx ? 4 : 0)));
                CHECK(r->slots == (n_ships <= 2 ? 2 : (n_ships <= 4 ? 4 : 8)));
                CHECK(!r->rec || rec);
                // (e) the pinned cases
                CHECK(s.tail == (entry != L::kStep && r->slots == 2));
                if (n_ships > 2) {
                  CHECK(s.lpe == 16 && !r->rec);
                } else if (wx) {
                  CHECK(s.lpe == (lpe <= 8 ? 8 : 16) && !r->rec);
                } else if (entry == L::kStep) {
                  CHECK(r->rec == (rec != 0) && s.lpe == (rec ? 16 : lpe));
                } else {
                  CHECK(s.lpe == (lpe == 2 ? 4 : lpe));
                }
              }
  // (b) no dead kernel: every row serves some handle
  for (const Row& r : kRows) {
    if (!selected.count(r.key))
      fprintf(stderr, "never selected: <%d, %d, %d, %d, %d, %d>\n", r.detailed, r.collav, r.lpe, r.rec, r.mode, r.slots);
  }
  CHECK(selected.size() == n_rows);

  // (e) again, spelled out
  const int D = SHIPSIM_MACH_DETAILED, S = SHIPSIM_MACH_SIMPLIFIED, SB = SHIPSIM_COLLAV_SBMPC, NO = SHIPSIM_COLLAV_NONE;
  L::Selection s = L::select(S, NO, 2, 2, false, false, L::kTable);  // a stream at 2 lanes runs at 4
  CHECK(!s.why && s.lpe == 4 && s.tail && s.key == L::step_key(false, NO, 4, false, 1, 2));
  s = L::select(D, SB, 2, 2, false, false, L::kPolicy);
  CHECK(!s.why && s.lpe == 4 && s.tail && s.key == L::step_key(true, SB, 4, false, 2, 2));
  s = L::select(D, SB, 2, 2, false, false, L::kStep);  // (the step does run at 2)
  CHECK(!s.why && s.lpe == 2 && !s.tail && s.key == L::step_key(true, SB, 2, false, 0, 2));
  s = L::select(D, SB, 2, 4, true, false, L::kStep);  // a recording step: 16 lanes, REC
  CHECK(!s.why && s.lpe == 16 && !s.tail && s.key == L::step_key(true, SB, 16, true, 0, 2));
  s = L::select(D, SB, 2, 4, false, true, L::kPolicy);  // weather at 4 lanes runs at 8
  CHECK(!s.why && s.lpe == 8 && s.tail && s.key == L::step_key(true, SB, 8, false, 2 | 4, 2));
  s = L::select(D, NO, 2, 16, false, true, L::kStep);
  CHECK(!s.why && s.lpe == 16 && !s.tail && s.key == L::step_key(true, NO, 16, false, 4, 2));
  for (int n_ships = 3; n_ships <= SHIPSIM_MAX_SHIPS; ++n_ships)  // K > 1: 16 lanes, 4 slots for 3..4 ships, 8 for 5
    for (int wx = 0; wx <= 1; ++wx) {
      s = L::select(D, SB, n_ships, 4, false, wx != 0, L::kTable);
      CHECK(!s.why && s.lpe == 16 && !s.tail);
      CHECK(s.key == L::step_key(true, SB, 16, false, 1 | (wx ? 4 : 0), n_ships <= 4 ? 4 : 8));
    }
  // the SBMPC optimiser a K-obstacle env's kernel is built for (and shipsim_sbmpc_eval_multi mirrors): three
  // obstacles in the 4-slot kernels (K = 2, 3), four in the 8-slot ones (K = 4)
  static_assert(L::ship_slots(2) == 2 && L::ship_slots(3) == 4 && L::ship_slots(4) == 4 && L::ship_slots(5) == 8, "");
  static_assert(L::sbmpc_nob(L::ship_slots(1 + 2)) == 3 && L::sbmpc_nob(L::ship_slots(1 + 3)) == 3, "");
  static_assert(L::sbmpc_nob(L::ship_slots(1 + 4)) == 4 && L::sbmpc_nob(8) == SHIPSIM_MAX_OBS, "");
  CHECK(L::select(S, SB, 3, 16, false, false, L::kStep).why != nullptr);
  CHECK(L::select(D, SHIPSIM_COLLAV_SIMPLE, 5, 16, false, false, L::kPolicy).why != nullptr);
  CHECK(L::select(D, SB, 2, 16, true, false, L::kTable).why != nullptr);
  CHECK(L::select(D, SB, 2, 16, true, true, L::kStep).why != nullptr);

  printf("launch host OK: %zu rows, %d selections served, %d refused\n", n_rows, served, refused);
  return 0;
}
