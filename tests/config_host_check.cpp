// Stand-alone driver of shipsim_create's host half (ast_sac_amd/csrc/shipsim_config_host.hpp), built by
// tests/test_config_host_cpu.py with -fsanitize=address,undefined. For the 18 default configs and five small maps on
// a two-ship AST config: the constant block's layout (against ConstBuf's accessors, restated here), the edges and
// boxes, the map grid's exactness on a 5 x 5 lattice of points per cell (against a brute-force point-segment distance
// and map_inside), the rank-mod-8 parts, the Params of the default AST config, and every rule of validate. Every
// check holds exactly, by construction; the block is the exactly-sized heap block const_block allocates, so a write
// past it is caught.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <vector>

#include "shipsim_config_host.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      return 1;                                          \
    }                                                    \
  } while (0)

namespace H = config_host;
using shipsim::Edge;
using shipsim::PolyBox;
using shipsim::ShipConst;

// ConstBuf's accessors (shipsim_state.hpp), restated: edges(), boxes(), cfg_route_n(), cfg_route_e(), ships(), kBytes
constexpr size_t kBoxesOff = sizeof(Edge) * SHIPSIM_MAX_VERTS;
constexpr size_t kRouteNOff = sizeof(Edge) * SHIPSIM_MAX_VERTS + sizeof(PolyBox) * SHIPSIM_MAX_POLYS;
constexpr size_t kRouteEOff = kRouteNOff + sizeof(double) * SHIPSIM_MAX_SHIPS * SHIPSIM_MAX_ROUTE;
constexpr size_t kShipsOff = sizeof(Edge) * SHIPSIM_MAX_VERTS + sizeof(PolyBox) * SHIPSIM_MAX_POLYS +
                             sizeof(double) * 2 * SHIPSIM_MAX_SHIPS * SHIPSIM_MAX_ROUTE;
static_assert(shipsim::kConstBoxesOff == kBoxesOff && shipsim::kConstRoutesOff == kRouteNOff &&
                  shipsim::kConstShipsOff == kShipsOff &&
                  shipsim::kConstBytes == kShipsOff + sizeof(ShipConst) * SHIPSIM_MAX_SHIPS,
              "the layout constants are the accessors' offsets");

// GEOS Distance::pointToSegment, as the device's map_distance forms it (not the grid builder's own helper)
static double brute_dist(double px, double py, const Edge& ed) {
  const double ax = ed.ax, ay = ed.ay, bx = ed.bx, by = ed.by;
  if (ax == bx && ay == by) return hypot(px - ax, py - ay);
  const double dx = bx - ax, dy = by - ay, len2 = dx * dx + dy * dy;
  const double r = ((px - ax) * dx + (py - ay) * dy) / len2;
  if (r <= 0.0) return hypot(px - ax, py - ay);
  if (r >= 1.0) return hypot(px - bx, py - by);
  return fabs(((ay - py) * dx - (ax - px) * dy) / len2) * sqrt(len2);
}

// the map of a config replaced by polygons given as (east, north) rings
typedef std::vector<std::vector<std::pair<double, double>>> Map;
static void set_map(shipsim_config* cfg, const Map& polys) {
  memset(cfg->poly_start, 0, sizeof(cfg->poly_start));
  memset(cfg->poly_east, 0, sizeof(cfg->poly_east));
  memset(cfg->poly_north, 0, sizeof(cfg->poly_north));
  int k = 0;
  cfg->n_polys = (int)polys.size();
  for (size_t p = 0; p < polys.size(); ++p) {
    cfg->poly_start[p] = k;
    for (const auto& v : polys[p]) {
      cfg->poly_east[k] = v.first;
      cfg->poly_north[k] = v.second;
      ++k;
    }
  }
  cfg->poly_start[polys.size()] = k;
}
static std::vector<std::pair<double, double>> ring(int n, double ce, double cn, double radius) {
  std::vector<std::pair<double, double>> r;
  for (int i = 0; i < n; ++i) r.push_back({ce + radius * cos(2 * M_PI * i / n), cn + radius * sin(2 * M_PI * i / n)});
  return r;
}

struct GridSeen {
  size_t in = 0, out = 0, mixed = 0;
  bool bit63 = false;
};

// the constant block of one validated config: layout, edges and boxes, parts, and (lattice) the grid's exactness
static int check_block(const shipsim_config& cfg, bool lattice, GridSeen* seen) {
  const int ns = cfg.n_ships, nv = cfg.poly_start[cfg.n_polys];
  ShipConst sc[SHIPSIM_MAX_SHIPS];
  memset(sc, 0, sizeof(sc));
  for (int i = 0; i < ns; ++i) H::ship_const(&cfg.ship[i], &sc[i]);
  H::ConstBlock cb;
  CHECK(H::const_block(&cfg, sc, cb) && cb.host);
  struct Free {
    char* p;
    ~Free() { free(p); }
  } guard{cb.host};
  const size_t cells = (size_t)cb.gnx * cb.gny;
  // layout
  CHECK(cb.n_edges == nv);
  CHECK(cb.grid_off % 256 == 0 && cb.grid_off >= shipsim::kConstBytes && cb.grid_off < shipsim::kConstBytes + 256);
  CHECK(cb.part_off % 8 == 0 && cb.part_off >= cb.grid_off + cells * 9 && cb.part_off < cb.grid_off + cells * 9 + 8);
  CHECK(cb.bytes == cb.part_off + cells * 64);
  const bool want_grid = nv >= 1 && nv <= 64 && cfg.map_query == SHIPSIM_MAP_GRID;
  CHECK(cb.use_grid == want_grid);
  if (!want_grid) CHECK(cb.gnx == 0 && cb.gny == 0 && cb.bytes == cb.part_off);
  else CHECK(cb.gnx > 0 && cb.gny > 0);
  const Edge* E = (const Edge*)cb.host;
  const PolyBox* B = (const PolyBox*)(cb.host + kBoxesOff);
  const double* Rn = (const double*)(cb.host + kRouteNOff);
  const double* Re = (const double*)(cb.host + kRouteEOff);
  CHECK(memcmp(cb.host + kShipsOff, sc, sizeof(sc)) == 0);
  for (int s = 0; s < SHIPSIM_MAX_SHIPS; ++s)
    for (int i = 0; i < SHIPSIM_MAX_ROUTE; ++i) {
      const bool set = s < ns && i < cfg.ship[s].n_route;
      CHECK(Rn[s * SHIPSIM_MAX_ROUTE + i] == (set ? cfg.ship[s].route_north[i] : 0.0));
      CHECK(Re[s * SHIPSIM_MAX_ROUTE + i] == (set ? cfg.ship[s].route_east[i] : 0.0));
    }
  // edges close around every polygon; every box bounds its vertices
  for (int p = 0; p < cfg.n_polys; ++p) {
    const int s0 = cfg.poly_start[p], cnt = cfg.poly_start[p + 1] - s0;
    CHECK(B[p].first == s0 && B[p].count == cnt);
    bool on_minx = false, on_maxx = false, on_miny = false, on_maxy = false;
    for (int i = 0; i < cnt; ++i) {
      const Edge& ed = E[s0 + i];
      const Edge& nx = E[s0 + (i + 1 == cnt ? 0 : i + 1)];
      CHECK(ed.ax == cfg.poly_east[s0 + i] && ed.ay == cfg.poly_north[s0 + i]);
      CHECK(ed.bx == nx.ax && ed.by == nx.ay);
      CHECK(B[p].minx <= ed.ax && ed.ax <= B[p].maxx && B[p].miny <= ed.ay && ed.ay <= B[p].maxy);
      on_minx |= ed.ax == B[p].minx; on_maxx |= ed.ax == B[p].maxx;
      on_miny |= ed.ay == B[p].miny; on_maxy |= ed.ay == B[p].maxy;
    }
    CHECK(on_minx && on_maxx && on_miny && on_maxy);  // (the box is tight)
  }
  for (int i = nv; i < SHIPSIM_MAX_VERTS; ++i) CHECK(E[i].ax == 0 && E[i].ay == 0 && E[i].bx == 0 && E[i].by == 0);
  if (!want_grid) return 0;
  // the grid covers the map's bounding box with kGridPad around it
  const H::MapBounds mb = H::map_bounds(&cfg);
  CHECK(cb.gx0 == mb.mn_e - H::kGridPad && cb.gy0 == mb.mn_n - H::kGridPad);
  CHECK(cb.gx0 + cb.gnx * H::kGridCell >= mb.mx_e + H::kGridPad && cb.gy0 + cb.gny * H::kGridCell >= mb.mx_n + H::kGridPad);
  const uint64_t* mask = (const uint64_t*)(cb.host + cb.grid_off);
  const uint8_t* flag = (const uint8_t*)(cb.host + cb.grid_off + cells * sizeof(uint64_t));
  const uint64_t* part = (const uint64_t*)(cb.host + cb.part_off);
  const double reach_far = shipsim::kGroundReach + H::kGridEps + sqrt(2.0) * (H::kGridCell + 2 * H::kGridEps);
  for (int j = 0; j < cb.gny; ++j)
    for (int i = 0; i < cb.gnx; ++i) {
      const size_t c = (size_t)j * cb.gnx + i;
      const uint64_t m = mask[c];
      if (nv < 64) CHECK(m >> nv == 0);
      // parts: a partition of the mask by bit rank mod 8
      uint64_t all = 0, want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int rank = 0;
      for (int k = 0; k < 64; ++k)
        if (m >> k & 1) want[rank++ % 8] |= (uint64_t)1 << k;
      for (int r = 0; r < 8; ++r) {
        CHECK(part[c * 8 + r] == want[r]);
        CHECK((all & part[c * 8 + r]) == 0);
        all |= part[c * 8 + r];
      }
      CHECK(all == m);
      CHECK(flag[c] == GRID_OUT || flag[c] == GRID_IN || flag[c] == GRID_MIXED);
      if (seen) {
        seen->in += flag[c] == GRID_IN; seen->out += flag[c] == GRID_OUT; seen->mixed += flag[c] == GRID_MIXED;
        seen->bit63 |= (m >> 63 & 1) != 0;
      }
      if (!lattice) continue;
      const double x0 = cb.gx0 + i * H::kGridCell, y0 = cb.gy0 + j * H::kGridCell;
      for (int k = 0; k < nv; ++k)  // no edge far from the cell is kept
        if (m >> k & 1) CHECK(brute_dist(x0 + 0.5 * H::kGridCell, y0 + 0.5 * H::kGridCell, E[k]) <= reach_far);
      for (int b = 0; b < 5; ++b)
        for (int a = 0; a < 5; ++a) {
          const double px = x0 + a * (H::kGridCell / 4), py = y0 + b * (H::kGridCell / 4);
          for (int k = 0; k < nv; ++k)  // every edge within reach of a point of the cell is kept
            if (brute_dist(px, py, E[k]) <= shipsim::kGroundReach) CHECK(m >> k & 1);
          if (flag[c] != GRID_MIXED)
            CHECK(shipsim::map_inside(E, B, cfg.n_polys, py, px) == (flag[c] == GRID_IN));
        }
    }
  return 0;
}

// one config broken in one field is refused with a message
static int check_refused(const shipsim_config& base, const std::function<void(shipsim_config&)>& breakit) {
  shipsim_config cfg = base;
  breakit(cfg);
  char err[256];
  err[0] = 0;
  CHECK(H::validate(&cfg, err, sizeof(err)) != 0);
  CHECK(err[0] != 0 && strlen(err) < sizeof(err));
  return 0;
}

int main() {
  int configs = 0;
  char err[256];
  // the 18 default configs: accepted wherever a step kernel serves them (all of them do), their blocks laid out
  for (int kind = 0; kind < 3; ++kind)
    for (int mach = 0; mach < 2; ++mach)
      for (int collav = 0; collav < 3; ++collav) {
        shipsim_config cfg;
        CHECK(H::default_config(kind, mach, collav, 4.0, &cfg) == SHIPSIM_OK);
        CHECK(cfg.n_ships == (kind == SHIPSIM_KIND_SINGLE ? 1 : 2) && cfg.n_polys == 6 && cfg.poly_start[6] == 55);
        CHECK(launch_host::select(mach, collav, cfg.n_ships, 16, false, false, launch_host::kStep).why == nullptr);
        err[0] = 0;
        CHECK(H::validate(&cfg, err, sizeof(err)) == 0 && err[0] == 0);
        GridSeen seen;
        if (check_block(cfg, configs == 0, &seen)) return 1;  // (one map for all 18: its lattice is walked once)
        CHECK(seen.in > 0 && seen.out > 0 && seen.mixed > 0);
        ++configs;
      }
  shipsim_config none;
  CHECK(H::default_config(3, 0, 0, 4.0, &none) == SHIPSIM_EINVAL && H::default_config(0, 2, 0, 4.0, &none) == SHIPSIM_EINVAL &&
        H::default_config(0, 0, -1, 4.0, &none) == SHIPSIM_EINVAL && H::default_config(0, 0, 0, 4.0, nullptr) == SHIPSIM_EINVAL);

  // five small maps on the two-ship AST config
  shipsim_config ast;
  CHECK(H::default_config(SHIPSIM_KIND_AST, SHIPSIM_MACH_DETAILED, SHIPSIM_COLLAV_SBMPC, 4.0, &ast) == SHIPSIM_OK);
  {
    shipsim_config cfg = ast;  // one triangle
    set_map(&cfg, {{{5000, 5000}, {6000, 5000}, {5500, 6000}}});
    CHECK(H::validate(&cfg, err, sizeof(err)) == 0);
    GridSeen seen;
    if (check_block(cfg, true, &seen)) return 1;
    CHECK(seen.out > 0 && seen.mixed > 0);
    ++configs;
  }
  {
    shipsim_config cfg = ast;  // a concave polygon and a 1000 m square on the cell lines: cells wholly inside it
    set_map(&cfg, {{{0, 0}, {3000, 0}, {3000, 1000}, {1000, 1000}, {1000, 3000}, {0, 3000}},
                   {{5000, 5000}, {6000, 5000}, {6000, 6000}, {5000, 6000}}});
    CHECK(H::validate(&cfg, err, sizeof(err)) == 0);
    GridSeen seen;
    if (check_block(cfg, true, &seen)) return 1;
    CHECK(seen.in >= 9 && seen.out > 0 && seen.mixed > 0);  // (at least the square's 3 x 3 inner cells)
    ++configs;
  }
  {
    shipsim_config cfg = ast;  // exactly 64 vertices: the grid is on and bit 63 is in use
    set_map(&cfg, {ring(40, 3000, 3000, 1500), ring(24, 7000, 4000, 800)});
    CHECK(cfg.poly_start[cfg.n_polys] == 64 && H::validate(&cfg, err, sizeof(err)) == 0);
    GridSeen seen;
    if (check_block(cfg, true, &seen)) return 1;
    CHECK(seen.bit63 && seen.in > 0 && seen.out > 0 && seen.mixed > 0);
    ++configs;
  }
  {
    shipsim_config cfg = ast;  // 65 vertices: no grid (check_block: gnx == gny == 0, bytes == part_off)
    set_map(&cfg, {ring(40, 3000, 3000, 1500), ring(25, 7000, 4000, 800)});
    CHECK(cfg.poly_start[cfg.n_polys] == 65 && H::validate(&cfg, err, sizeof(err)) == 0);
    if (check_block(cfg, true, nullptr)) return 1;
    cfg = ast;  // (and the default map with the grid switched off)
    cfg.map_query = SHIPSIM_MAP_ALL_EDGES;
    if (check_block(cfg, true, nullptr)) return 1;
    ++configs;
  }
  {
    shipsim_config cfg = ast;  // no polygons
    set_map(&cfg, {});
    CHECK(cfg.n_polys == 0 && H::validate(&cfg, err, sizeof(err)) == 0);
    if (check_block(cfg, true, nullptr)) return 1;
    ++configs;
  }

  // Params of the default AST config
  {
    shipsim::Params P;
    H::params(&ast, 7, P);
    const shipsim_ship_config& t = ast.ship[0];
    const shipsim_ship_config& o = ast.ship[1];
    CHECK(P.kind == SHIPSIM_KIND_AST && P.machinery == SHIPSIM_MACH_DETAILED && P.collav == SHIPSIM_COLLAV_SBMPC);
    CHECK(P.n_ships == 2 && P.n_envs == 7 && P.n_polys == 6 && P.max_sampling == 9 && P.epw == 0);
    CHECK(P.sbmpc_nsamp == 50 && P.sbmpc_tf == 1000 && P.sbmpc_dt == 20 && P.roa2 == 90000);
    CHECK(P.dt == 4.0 && P.mach_dt_init == 4.0 && P.sim_time == 10000);
    CHECK(ast.machinery_dt_quirk == 1 && P.mach_dt_reset == 0.01);
    CHECK(P.min_east == 0 && P.max_east == 20000 && P.min_north == 0 && P.max_north == 10000);
    const float want[8] = {(float)t.initial_north_position_m, (float)t.initial_east_position_m, 0.0f,
                           (float)o.initial_north_position_m, (float)o.initial_east_position_m,
                           (float)o.initial_yaw_angle_rad, 0.0f, (float)o.initial_forward_speed_m_per_s};
    CHECK(memcmp(P.initial_states, want, sizeof(want)) == 0);
    CHECK(P.AB_seg_n == (o.route_north[o.n_route - 1] - o.route_north[0]) / 10);
    CHECK(P.AB_seg_e == (o.route_east[o.n_route - 1] - o.route_east[0]) / 10);
    CHECK(P.n_base0 == P.AB_seg_n + o.route_north[0] && P.e_base0 == P.AB_seg_e + o.route_east[0]);
    CHECK(P.wind_sin == sin(ast.wind_direction) && P.wind_cos == cos(ast.wind_direction));
    CHECK(P.iw_cos == cos(P.omega_iw) && P.iw_sin == sin(P.omega_iw));
    CHECK(P.action_low == ast.action_low && P.action_high == ast.action_high);
    shipsim_config plain = ast;
    plain.machinery_dt_quirk = 0;
    plain.time_step = 0.5;
    H::params(&plain, 7, P);
    CHECK(P.mach_dt_reset == 0.5 && P.dt == 0.5 && P.mach_dt_init == 0.5);
  }

  // validate: one config per rule, broken in that one field
  {
    shipsim_config single, noniw;
    CHECK(H::default_config(SHIPSIM_KIND_SINGLE, 0, 0, 0.5, &single) == SHIPSIM_OK);
    CHECK(H::default_config(SHIPSIM_KIND_NONIW, 0, 0, 0.5, &noniw) == SHIPSIM_OK);
    typedef shipsim_config C;
    const std::pair<const C*, std::function<void(C&)>> rules[] = {
        {&ast, [](C& c) { c.abi_version = SHIPSIM_ABI_VERSION + 1; }},
        {&ast, [](C& c) { c.kind = -1; }},
        {&ast, [](C& c) { c.kind = 3; }},
        {&ast, [](C& c) { c.machinery = -1; }},
        {&ast, [](C& c) { c.machinery = 2; }},
        {&ast, [](C& c) { c.collav = -1; }},
        {&ast, [](C& c) { c.collav = 3; }},
        {&ast, [](C& c) { c.n_ships = 1; }},
        {&ast, [](C& c) { c.n_ships = SHIPSIM_MAX_SHIPS + 1; }},
        {&ast, [](C& c) { c.n_ships = 3; c.ship[2] = c.ship[1]; c.machinery = SHIPSIM_MACH_SIMPLIFIED; }},  // no kernel
        {&ast, [](C& c) { c.n_ships = 3; c.ship[2] = c.ship[1]; c.collav = SHIPSIM_COLLAV_SIMPLE; }},       // no kernel
        {&single, [](C& c) { c.n_ships = 2; }},
        {&noniw, [](C& c) { c.n_ships = 1; }},
        {&ast, [](C& c) { c.time_step = 0; }},
        {&ast, [](C& c) { c.time_step = NAN; }},
        {&ast, [](C& c) { c.max_sampling_frequency = -1; }},
        {&ast, [](C& c) { c.max_sampling_frequency = SHIPSIM_MAX_ROUTE - 1; }},
        {&ast, [](C& c) { c.ship[0].n_route = 1; }},
        {&ast, [](C& c) { c.ship[0].n_route = SHIPSIM_MAX_ROUTE + 1; }},
        {&single, [](C& c) { c.ship[0].n_route = 0; }},
        {&ast, [](C& c) { c.ship[1].n_route = SHIPSIM_MAX_ROUTE - 8; }},  // 8 + 9 samplings: one too many
        {&ast, [](C& c) { c.n_polys = -1; }},
        {&ast, [](C& c) { c.n_polys = SHIPSIM_MAX_POLYS + 1; }},
        {&ast, [](C& c) { c.poly_start[0] = 1; }},
        {&ast, [](C& c) { c.poly_start[c.n_polys] = SHIPSIM_MAX_VERTS + 1; }},
        {&ast, [](C& c) { c.poly_start[1] = c.poly_start[2] - 2; }},  // polygon 1 with two vertices
        {&ast, [](C& c) { c.sbmpc_dt = 0; }},
        {&ast, [](C& c) { c.sbmpc_dt = c.sbmpc_tf / 4097; }},
    };
    for (const auto& r : rules) {
      err[0] = 0;
      CHECK(H::validate(r.first, err, sizeof(err)) == 0);  // (sound before it is broken)
      if (check_refused(*r.first, r.second)) return 1;
    }
    // (the ship count the refused multi-obstacle configs ask for is served with the detailed machinery)
    shipsim_config multi = ast;
    multi.n_ships = 3;
    multi.ship[2] = multi.ship[1];
    CHECK(H::validate(&multi, err, sizeof(err)) == 0);
    // the obstacle route's bound is met with equality
    shipsim_config edge = ast;
    edge.ship[1].n_route = SHIPSIM_MAX_ROUTE - 9;
    CHECK(H::validate(&edge, err, sizeof(err)) == 0);
  }
  printf("config host OK: %d configurations\n", configs);
  return 0;
}
