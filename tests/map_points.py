"""Maps and adversarial positions for the coastline query's tests (test_map_query_cpu.py, test_gpu_map_query.py).

Maps (integer vertex coordinates, inside the reference map's bounds 0..20000 m east, 0..10000 m north):
  A     the reference map;
  B     a concave L and a 1000 m square whose edges lie on grid cell lines (cells wholly inside land, horizontal and
        vertical edges). Its bounding box is the reference map's, so the configured routes and the map horizon hold.
        The L's edges sit 20 m, 5 m and 20 m off cell lines, which the far-shore seam and the reach family need;
  C     two rings of 40 + 24 vertices, 64 in all: the grid is on and bit 63 of the candidate masks is in use;
  D65   the same with 40 + 25 vertices: no grid;
  D128  128 vertices in 16 polygons: no grid, every table full;
  E     a slanted sliver island 3 m wide, narrower than the hull, crossing several cells;
  F     no polygons.

Positions: per map a dict family -> (k, 2) array of (north, east). Unless a family says otherwise the coordinates are
multiples of 2**-11 m (0.49 mm: the half-millimetre offsets around the 1 mm cell enlargement need the bit below
2**-10), so the hull corners n +- 40, e +- 40 are exact in double (asserted by `points`). The families:
  cell_lines  centres on a grid cell line (gx0 + 200 i; the grid's origin is the bounding box less 2000 m), one ulp
              either side (not multiples of 2**-11), and 2**-11 and 3 * 2**-11 m (0.49 / 1.46 mm) either side, next to
              cells of differing class (IN | MIXED, OUT | MIXED);
  reach       the same offsets on the near side of a cell whose distance to a vertex is within (990, 1000] m while the
              neighbouring cell's is more, so the vertex's edges are candidates of one cell only, and on to the point
              exactly 1000 m from the vertex;
  threshold   centres exactly 1000 m from a vertex by the integer offsets (+-600, +-800), (+-800, +-600) where that
              vertex is the nearest shore, and the same with one coordinate one representable step further out and one
              further in (nextafter: the other family that is not a multiple of 2**-11);
  seam        (B) shore distances lim -+ {1e-3, 1e-6, 1e-9} m, lim = 40 sqrt(2) + 1e-3, off a vertical edge that lies
              20 m inside the neighbouring cell column, the centre in an unmixed water cell and in an unmixed land
              cell (coordinates multiples of 2**-30 m); and diagonally off a land corner across a cell corner, at
              vertex distances from 42 m to lim + 1e-3 (multiples of 2**-30 m), where the hull corner nearest the
              vertex lies in land for distances under 40 sqrt(2) while the centre's cell is unmixed water;
  corners     a hull corner exactly on a vertex, on an edge's midpoint, on a horizontal edge's span and on its
              extension, and corners in other cells than the centre;
  sliver      (E) the hull astride the sliver with no corner in it (not aground, the centre in land) and with one in;
  off_grid    the centre in land, beyond the padded grid (cell -1), just inside the grid's last row and column;
  ring        (C, D65, D128) 30 m and 600 m outside every edge's midpoint and every vertex;
  edge_1000   (B) exactly 1000 m from the interior of a horizontal and of a vertical edge. There a query in double is
              not pinned: c^2 / len^2 (the device) and |c / len^2| sqrt(len^2) (GEOS) round to either side of the
              gate. Their hull tests are asserted; their distances are counted, agreeing or not, and reported;
  on_route    (A, B) ON_ROUTE positions on the first leg of the ship under test's route and as many on the first
              900 m of the obstacle ship's, in open water: a pair of ships placed there fails no navigation test, so
              its decision goes on past the placed tick (the other positions' mostly end on it).
Test infrastructure only."""
import math

import numpy as np

from ast_sac_amd import shipsim_abi as abi

CELL, PAD, EPS = 200.0, 2000.0, 1e-3  # the grid's cell, padding and cell enlargement [m] (csrc/shipsim_config_host.hpp)
HALF = 40.0  # half the ships' length: the hull's hard points are (n -+ HALF, e -+ HALF)
LIM = HALF * 1.4142135623730951 + 1e-3  # the far-shore shortcut's limit (csrc/shipsim_kernels.hip)
Q = 2.0 ** -11
GRID_OUT, GRID_IN, GRID_MIXED = 0, 1, 2


def set_map(cfg, rings):
    """tests/config_host_check.cpp's set_map: rings of (east, north) into poly_start / poly_east / poly_north."""
    for i in range(abi.MAX_POLYS + 1):
        cfg.poly_start[i] = 0
    for i in range(abi.MAX_VERTS):
        cfg.poly_east[i] = cfg.poly_north[i] = 0.0
    assert len(rings) <= abi.MAX_POLYS and sum(len(r) for r in rings) <= abi.MAX_VERTS
    k = 0
    cfg.n_polys = len(rings)
    for p, ring in enumerate(rings):
        cfg.poly_start[p] = k
        for e, n in ring:
            cfg.poly_east[k], cfg.poly_north[k] = e, n
            k += 1
    cfg.poly_start[len(rings)] = k
    return cfg


def _ring(n, ce, cn, radius):
    """A counter-clockwise ring of n integer vertices around (ce, cn) (east, north)."""
    return [(float(round(ce + radius * math.cos(2 * math.pi * i / n))),
             float(round(cn + radius * math.sin(2 * math.pi * i / n)))) for i in range(n)]


B_L = [(0.0, 10000.0), (0.0, 7005.0), (1005.0, 7005.0), (1005.0, 8820.0), (2980.0, 8820.0), (2980.0, 10000.0)]
B_SQUARE = [(19000.0, 0.0), (20000.0, 0.0), (20000.0, 1000.0), (19000.0, 1000.0)]
E_SLIVER = [(5010.0, 5090.0), (5890.0, 5290.0), (5890.0, 5293.0), (5010.0, 5093.0)]

MAPS = {
    "A": [[(float(e), float(n)) for e, n in poly] for poly in abi.MAP_DATA],
    "B": [B_L, B_SQUARE],
    "C": [_ring(40, 3000, 3000, 1500), _ring(24, 7000, 4000, 800)],
    "D65": [_ring(40, 3000, 3000, 1500), _ring(25, 7000, 4000, 800)],
    "D128": [_ring(8, 2500 + 5000 * i, 1500 + 2300 * j, 600) for j in range(4) for i in range(4)],
    "E": [E_SLIVER],
    "F": [],
}
NAMES = tuple(MAPS)
N_VERTS = {"A": 55, "B": 10, "C": 64, "D65": 65, "D128": 128, "E": 4, "F": 0}


def config(name, collav="none", **kw):
    cfg = abi.ast_config(collav, **kw)
    return set_map(cfg, MAPS[name])


def default_bounds(name):
    """True where the map's bounding box is the reference map's (the configured routes lie inside the horizon)."""
    return name in ("A", "B")


class Grid:
    """The map grid as csrc/shipsim_config_host.hpp lays it out, and each cell's class restated: MIXED where an edge
    meets the cell enlarged by 1 mm, else the class of its centre. Used to choose positions only: what a position's
    query must return comes from map_ref."""

    def __init__(self, cfg):
        nv = cfg.poly_start[cfg.n_polys]
        self.nv = nv
        xs, ys = np.array(cfg.poly_east[:max(nv, 1)]), np.array(cfg.poly_north[:max(nv, 1)])
        self.mn_e, self.mx_e, self.mn_n, self.mx_n = xs.min(), xs.max(), ys.min(), ys.max()
        self.on = 0 < nv <= 64
        self.gx0, self.gy0 = self.mn_e - PAD, self.mn_n - PAD
        self.gnx = int(math.ceil((self.mx_e - self.mn_e + 2 * PAD) / CELL))
        self.gny = int(math.ceil((self.mx_n - self.mn_n + 2 * PAD) / CELL))
        self.edges = []
        for p in range(cfg.n_polys):
            a, b = cfg.poly_start[p], cfg.poly_start[p + 1]
            for k in range(a, b):
                j = a + (k + 1 - a) % (b - a)
                self.edges.append((cfg.poly_east[k], cfg.poly_north[k], cfg.poly_east[j], cfg.poly_north[j]))
        self.edges = np.array(self.edges).reshape(-1, 4)
        self.slices = [(cfg.poly_start[p], cfg.poly_start[p + 1]) for p in range(cfg.n_polys)]
        self.flag = self._classes() if self.on else None

    def cell(self, n, e):
        fx, fy = math.floor((e - self.gx0) / CELL), math.floor((n - self.gy0) / CELL)
        return (fy, fx) if 0 <= fx < self.gnx and 0 <= fy < self.gny else None

    def _classes(self):
        i, j = np.meshgrid(np.arange(self.gnx), np.arange(self.gny))
        x0, x1 = self.gx0 + i * CELL - EPS, self.gx0 + (i + 1) * CELL + EPS
        y0, y1 = self.gy0 + j * CELL - EPS, self.gy0 + (j + 1) * CELL + EPS
        touched = np.zeros(i.shape, bool)
        for ax, ay, bx, by in self.edges:  # Liang-Barsky against every cell's closed rectangle
            t0, t1 = np.zeros(i.shape), np.ones(i.shape)
            ok = np.ones(i.shape, bool)
            for p, q in ((ax - bx, ax - x0), (bx - ax, x1 - ax), (ay - by, ay - y0), (by - ay, y1 - ay)):
                if p == 0:
                    ok &= q >= 0
                else:
                    t = q / p
                    if p < 0:
                        ok &= t <= t1
                        t0 = np.maximum(t0, t)
                    else:
                        ok &= t >= t0
                        t1 = np.minimum(t1, t)
            touched |= ok & (t0 <= t1)
        cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
        inside = np.zeros(i.shape, bool)
        for a, b in self.slices:
            cross = np.zeros(i.shape, int)
            for ax, ay, bx, by in self.edges[a:b]:
                if ay != by:
                    cross += ((ay > cy) != (by > cy)) & (cx < ax + (cy - ay) * (bx - ax) / (by - ay))
            inside |= cross % 2 == 1
        return np.where(touched, GRID_MIXED, np.where(inside, GRID_IN, GRID_OUT))

    def shore(self, n, e):
        """Approximate (double) distance to the nearest edge and that edge's index: for choosing positions."""
        if not len(self.edges):
            return math.inf, -1
        ax, ay, bx, by = self.edges.T
        dx, dy = bx - ax, by - ay
        t = np.clip(((e - ax) * dx + (n - ay) * dy) / (dx * dx + dy * dy), 0, 1)
        d = np.hypot(ax + t * dx - e, ay + t * dy - n)
        return float(d.min()), int(d.argmin())


def _ulp(x, k):
    return float(np.nextafter(x, math.inf if k > 0 else -math.inf))


def _across(line):
    """A coordinate on a cell line and either side of it: one ulp, 2**-11 m, 3 * 2**-11 m."""
    return [line, _ulp(line, 1), _ulp(line, -1), line + Q, line - Q, line + 3 * Q, line - 3 * Q]


def _cell_lines(g, per_kind=3):
    out = []
    if not g.on:
        return out
    f = g.flag
    for axis in (1, 0):  # neighbours in east (a north-south line between them), then in north
        a, b = (f[:, :-1], f[:, 1:]) if axis == 1 else (f[:-1, :], f[1:, :])
        for ka, kb in ((GRID_IN, GRID_MIXED), (GRID_MIXED, GRID_IN), (GRID_OUT, GRID_MIXED), (GRID_MIXED, GRID_OUT)):
            jj, ii = np.nonzero((a == ka) & (b == kb))
            # spread over the map, and away from coordinate 0 (its neighbours in double are denormals)
            for k in np.linspace(0, len(jj) - 1, min(per_kind, len(jj))).astype(int) if len(jj) else []:
                j, i = int(jj[k]), int(ii[k])
                if axis == 1:
                    line, other = g.gx0 + (i + 1) * CELL, g.gy0 + j * CELL + 137.25
                else:
                    line, other = g.gy0 + (j + 1) * CELL, g.gx0 + i * CELL + 137.25
                if line == 0.0:
                    continue
                out += [(other, x) if axis == 1 else (x, other) for x in _across(line)]
    return out


def _reach(g):
    """For a vertex v and a direction along an axis: the first cell line at 990 m or more from v. Where it is within
    (990, 1000) m, the cell beyond it has v's edges as candidates by less than 10 m of the reach: positions on that
    cell's near side level with v, either side of the line, and on to exactly 1000 m and a step past it."""
    out = []
    for k in range(g.nv):
        vx, vy = g.edges[k, 0], g.edges[k, 1]
        for axis, sgn in ((0, 1), (0, -1), (1, 1), (1, -1)):
            v, o = (vx, vy) if axis == 0 else (vy, vx)
            g0 = g.gx0 if axis == 0 else g.gy0
            steps = (v + sgn * 990.0 - g0) / CELL
            line = g0 + CELL * (math.ceil(steps) if sgn > 0 else math.floor(steps))
            gap = abs(line - v)
            if not 990.0 < gap < 1000.0 or line == 0.0:
                continue
            for off in (-2.5, 0.0):
                along = _across(line) + [v + sgn * 997.0, v + sgn * 1000.0, v + sgn * (1000.0 + 3 * Q)]
                pts = [(o + off, x) if axis == 0 else (x, o + off) for x in along]
                # kept where the vertex's edges are the shore (no other edge nearer than 985 m)
                if all(g.shore(n, e)[0] > 985.0 for n, e in pts):
                    out += pts
    return out


_345 = [(sa * a, sb * b) for a, b in ((600.0, 800.0), (800.0, 600.0)) for sa in (1, -1) for sb in (1, -1)]


def _threshold(g, most=10):
    """Triples: exactly 1000 m from a vertex, one representable step further out, one further in. The stepped
    coordinate is one of magnitude >= 1024 m: its ulp is two or more of the 600 / 800 m offset's, so the offset, its
    square (3 ulps of 1e6 off) and the root (3 ulps of 1000 inward, 1.6 outward) all resolve the step in double."""
    out = []
    for k in np.linspace(0, g.nv - 1, min(g.nv, 4 * most)).astype(int) if g.nv else []:
        vx, vy = g.edges[k, 0], g.edges[k, 1]
        for de, dn in _345:
            n, e = vy + dn, vx + de
            d, _ = g.shore(n, e)
            if abs(d - 1000.0) < 1e-6 and len(out) < 3 * most and max(abs(n), abs(e)) >= 1024.0:
                # (this vertex is the nearest shore)
                if abs(e) >= 1024.0:
                    outer, inner = (n, _ulp(e, 1 if de > 0 else -1)), (n, _ulp(e, -1 if de > 0 else 1))
                if abs(n) >= 1024.0:
                    inner = (_ulp(n, -1 if dn > 0 else 1), e)
                    if abs(e) < 1024.0:
                        outer = (_ulp(n, 1 if dn > 0 else -1), e)
                out += [(n, e), outer, inner]
                break
    return out


def _seam_b():
    r = 2.0 ** 30
    out = []
    for d in (LIM - 1e-3, LIM - 1e-6, LIM - 1e-9, LIM + 1e-9, LIM + 1e-6, LIM + 1e-3):
        d = round(d * r) / r
        out.append((9400.25, 2980.0 + d))   # water, cell column [3000, 3200): unmixed (the edge is at 2980)
        out.append((8000.25, 1005.0 - d))   # land, cell column [800, 1000): unmixed (the edge is at 1005)
        out.append((8820.0 - d, 2000.25))   # water south of the arm's edge at 8820, cell row [8600, 8800): unmixed
    # diagonally off the land corner (2980, 8820) (land to its north-west) into the water cell south-east of the
    # cell corner (3000, 8800): the hull's north-west corner is in land for vertex distances under 40 sqrt(2)
    for d in (42.0, 49.5, 56.0, LIM - 1e-3 - 1e-3, LIM - 1e-3 - 1e-6, LIM - 1e-3 + 1e-6, LIM - 1e-6, LIM + 1e-6,
              LIM + 1e-3):
        a = round(d / math.sqrt(2.0) * r) / r
        out.append((8820.0 - a, 2980.0 + a))
    return out


def _corners(g, most=6):
    out = []
    idx = np.linspace(0, g.nv - 1, min(g.nv, most)).astype(int) if g.nv else []
    for k in idx:
        ax, ay, bx, by = g.edges[k]
        for sn, se in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            out.append((ay + sn * HALF, ax + se * HALF))  # a hull corner on the vertex
        mx, my = (ax + bx) / 2, (ay + by) / 2  # exact: integer coordinates
        out += [(my + HALF, mx + HALF), (my - HALF, mx - HALF)]  # a hull corner on the edge's midpoint
    for ax, ay, bx, by in g.edges:
        if ay == by and abs(bx - ax) > 300.0:  # a horizontal edge: a corner on its span, and on its extension
            lo, hi = min(ax, bx), max(ax, bx)
            for sn in (1, -1):
                out += [(ay + sn * HALF, lo + 130.0 + HALF), (ay + sn * HALF, hi + 100.0 + HALF),
                        (ay + sn * HALF, lo - 100.0 - HALF), (ay + sn * HALF, hi + HALF)]
    # corners in other cells than the centre, next to shore: 45 m off the first edges' midpoints on either side
    for k in idx:
        ax, ay, bx, by = g.edges[k]
        ln = math.hypot(bx - ax, by - ay)
        for s in (1, -1):
            n = round(((ay + by) / 2 - s * 45.0 * (bx - ax) / ln) / Q) * Q
            e = round(((ax + bx) / 2 + s * 45.0 * (by - ay) / ln) / Q) * Q
            out.append((n, e))
    return out


def _sliver_e():
    out = []
    for e in (5230.0, 5450.0, 5670.0, 5802.5):  # the sliver's lower edge at east e: n = 5090 + (e - 5010) * 200 / 880
        mid = round((5090.0 + (e - 5010.0) * 200.0 / 880.0 + 1.5) / Q) * Q
        out += [(mid, e),                 # astride: the centre in the sliver, every corner 40 m off it
                (mid + HALF, e - HALF),   # the south-east corner (n - 40, e + 40) in the sliver, on (mid, e)
                (mid - HALF, e + HALF)]   # the north-west corner
    return out


def _off_grid(g, cfg):
    out = []
    for p in range(cfg.n_polys):  # the centre in land: the mean of a polygon's first three vertices (a convex corner)
        a = cfg.poly_start[p]
        if cfg.poly_start[p + 1] - a >= 3:
            out.append((round(sum(cfg.poly_north[a:a + 3]) / 3 / Q) * Q,
                        round(sum(cfg.poly_east[a:a + 3]) / 3 / Q) * Q))
    mid_e, mid_n = (g.mn_e + g.mx_e) / 2 + 0.25, (g.mn_n + g.mx_n) / 2 + 0.25
    out += [(g.mn_n - PAD - 3000.5, mid_e), (mid_n, g.mx_e + PAD + 3000.5), (g.mn_n - PAD - Q, mid_e)]
    top, right = g.gy0 + g.gny * CELL, g.gx0 + g.gnx * CELL
    out += [(top - Q, mid_e), (_ulp(top, -1), mid_e), (top, mid_e), (mid_n, right - Q), (mid_n, _ulp(right, -1)),
            (mid_n, right), (top - Q, right - Q), (g.gy0, g.gx0), (g.gy0 + Q, _ulp(g.gx0, -1))]
    return out


def _ring_points(g, cfg):
    out = []
    for p in range(cfg.n_polys):
        a, b = cfg.poly_start[p], cfg.poly_start[p + 1]
        for k in range(a, b):
            ax, ay, bx, by = g.edges[k]
            px, py = g.edges[a + (k - 1 - a) % (b - a), :2]  # the previous vertex
            n1 = np.array([by - ay, -(bx - ax)]) / math.hypot(bx - ax, by - ay)  # outward (east, north) of a
            n0 = np.array([ay - py, -(ax - px)]) / math.hypot(ax - px, ay - py)  # counter-clockwise ring
            bis = (n0 + n1) / np.linalg.norm(n0 + n1)
            for dist in (30.0, 600.0):
                for (x, y), nrm in ((((ax + bx) / 2, (ay + by) / 2), n1), ((ax, ay), bis)):
                    out.append((round((y + dist * nrm[1]) / Q) * Q, round((x + dist * nrm[0]) / Q) * Q))
    return out


def _edge_1000_b():
    # south of the arm's edge at north 8820 (east 1005 .. 2980), east of its edge at east 2980 (north 8820 .. 10000),
    # east of the leg's edge at east 1005 (north 7005 .. 8820): level with the edges' interiors, no vertex as near
    return [(7820.0, 2300.25), (7820.0, 2500.5), (9400.25, 3980.0), (9811.5, 3980.0), (7500.25, 2005.0)]


ON_ROUTE = 8


def _on_route():
    """The ship under test's first leg runs (0, 0) -> (2000, 4500) (north, east): positions at 1/10 .. 8/10 of it,
    cross-track error 0. The obstacle ship's leg runs from (10000, 15000) to its first sampled waypoint, which lies
    within 30 degrees of the configured course (south-west): 150 .. 850 m down that course the cross-track error is
    under 850 sin 30 = 425 m, inside its 500 m limit."""
    test = [(200.0 * k, 450.0 * k) for k in range(1, ON_ROUTE + 1)]
    obs = []
    for k in range(ON_ROUTE):
        s = round((150.0 + 100.0 * k) / math.sqrt(2.0) / Q) * Q
        obs.append((10000.0 - s, 15000.0 - s))
    return test + obs


FAMILIES = ("cell_lines", "reach", "threshold", "seam", "corners", "sliver", "off_grid", "ring", "edge_1000",
            "on_route")
# the maps each family applies to (its positions are asserted non-empty there: test_map_query_cpu.py)
APPLIES = {
    "cell_lines": ("A", "B", "C", "E"),   # maps with a grid
    "reach": ("B", "E"),                  # a vertex under 10 m short of a cell line (A's lie on 50 m multiples)
    "threshold": ("A", "B", "C", "D65", "D128", "E"),
    "seam": ("B",),
    "corners": ("A", "B", "C", "D65", "D128", "E"),
    "sliver": ("E",),
    "off_grid": NAMES,
    "ring": ("C", "D65", "D128"),
    "edge_1000": ("B",),
    "on_route": ("A", "B"),   # the maps whose bounding box keeps the configured routes inside the horizon
}
NOT_ON_Q = ("cell_lines", "reach", "threshold", "seam", "off_grid")  # families with finer coordinates (see above)

_cache = {}


def points(name):
    """dict family -> (k, 2) float64 array of (north, east) for the map `name`; every family a key, empty where it
    does not apply. Built once per map."""
    if name in _cache:
        return _cache[name]
    cfg = config(name)
    g = Grid(cfg)
    fam = {f: [] for f in FAMILIES}
    if g.nv:
        fam["cell_lines"] = _cell_lines(g)
        fam["reach"] = _reach(g)
        fam["threshold"] = _threshold(g)
        fam["corners"] = _corners(g)
    if name == "B":
        fam["seam"] = _seam_b()
        fam["edge_1000"] = _edge_1000_b()
    if name == "E":
        fam["sliver"] = _sliver_e()
    fam["off_grid"] = _off_grid(g, cfg)
    if name in APPLIES["on_route"]:
        fam["on_route"] = _on_route()
    if name in APPLIES["ring"]:
        fam["ring"] = _ring_points(g, cfg)
    out = {}
    for f, pts in fam.items():
        a = np.array(pts, np.float64).reshape(-1, 2)
        if f not in NOT_ON_Q:
            assert (a / Q == np.round(a / Q)).all(), f
        for c in (a[:, 0], a[:, 1]):  # the hull's hard points are exact in double (but for the one-ulp neighbours:
            c = c[c * 2.0 ** 30 == np.round(c * 2.0 ** 30)]  # theirs are the doubles n -+ 40 rounds to, on every side)
            for h in (HALF, -HALF):
                assert ((c + h) - c == h).all() and ((c + h) - h == c).all(), f
        out[f] = a
    _cache[name] = out
    return out


def all_points(name):
    """Every position of the map, the families concatenated in FAMILIES order: ((k, 2) array, list of family names)."""
    p = points(name)
    return np.concatenate([p[f] for f in FAMILIES]), [f for f in FAMILIES for _ in range(len(p[f]))]


_expected = {}


def expected(name):
    """map_ref on every position of the map, computed once: dict of pts (k, 2), family (list), inside (centre in
    land), grounded (any hull corner in land), d2 (exact squared shore distances, Fractions; None without edges),
    edge (the nearest edge's index), d (the shore distance as a double, inf without edges), terms (k, 2): the
    grounding terms' shares of the reward as the trajectory record keeps them (a fifth of each)."""
    if name not in _expected:
        import map_ref as R
        cfg = config(name)
        pts, family = all_points(name)
        q = [R.dist2(cfg, n, e) for n, e in pts]
        d = np.array([math.inf if x is None else R.sqrt_f64(x) for x, _ in q])
        _expected[name] = dict(
            pts=pts, family=family, inside=np.array([R.inside(cfg, n, e) for n, e in pts]),
            grounded=np.array([R.hull_grounded(cfg, n, e, 2 * HALF) for n, e in pts]), d2=[x for x, _ in q],
            edge=np.array([k for _, k in q]), d=d, terms=np.array([R.grounding_terms(x, 5) for x in d]).reshape(-1, 2))
    return _expected[name]
