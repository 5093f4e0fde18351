"""An exact reference of the coastline query (obstacle.py:126-141 over shapely / GEOS), in rational arithmetic on the
doubles' exact values: point in polygon by the ray-crossing rule with GEOS' boundary convention (a point on a
polygon's ring is not contained), and the squared point-to-segment distance minimised over every edge. Pure Python, no
float rounding anywhere but the final rounding of sqrt_f64 and of grounding_terms. Test infrastructure only.

Every coordinate is a dyadic rational, so the work is done on integers scaled by 2**_K (exact: asserted), and only the
results are Fractions."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

_K = 64  # doubles of magnitude >= 2**-11 below 2**53 are multiples of 2**-64; 0 is too


def _fix(x):
    """The double x as an integer multiple of 2**-_K, exactly."""
    f = Fraction(float(x)) * (1 << _K)
    assert f.denominator == 1, x
    return f.numerator


def rings(cfg):
    """The map's polygons as lists of (east, north) doubles."""
    return [[(cfg.poly_east[k], cfg.poly_north[k]) for k in range(cfg.poly_start[p], cfg.poly_start[p + 1])]
            for p in range(cfg.n_polys)]


class Map:
    """The polygons' edges in scaled integers: edge k of the flat vertex table runs from vertex k to the next vertex
    of its ring (the table order of the config, which the device's edge table and candidate masks share)."""

    def __init__(self, cfg):
        self.polys = []
        self.edges = []
        for ring in rings(cfg):
            pts = [(_fix(x), _fix(y)) for x, y in ring]
            first = len(self.edges)
            for i, a in enumerate(pts):
                self.edges.append((a, pts[(i + 1) % len(pts)]))
            self.polys.append((first, len(pts)))


_maps = {}


def _map(cfg):
    key = (cfg.n_polys, tuple(cfg.poly_start[:cfg.n_polys + 1]), tuple(cfg.poly_east), tuple(cfg.poly_north))
    if key not in _maps:
        _maps[key] = Map(cfg)
    return _maps[key]


def _on_segment(px, py, a, b):
    (ax, ay), (bx, by) = a, b
    if (bx - ax) * (py - ay) - (by - ay) * (px - ax) != 0:
        return False
    return min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)


def _contains(m, first, count, px, py):
    """Strictly inside the ring: an odd number of edges crossed by the ray from the point towards +east, and the point
    on none of them."""
    crossings = 0
    for a, b in m.edges[first:first + count]:
        if _on_segment(px, py, a, b):
            return False
        (ax, ay), (bx, by) = a, b
        if (ay > py) != (by > py):  # the edge spans the ray's line, its upper end excluded
            # the crossing's east coordinate ax + (py - ay) (bx - ax) / (by - ay) against px, by the exact sign
            det = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
            if (det > 0) == (by > ay):
                crossings += 1
    return crossings % 2 == 1


def inside(cfg, n, e):
    """if_pos_inside_obstacles: any polygon contains (north n, east e); a point on a polygon's ring is not in it."""
    m = _map(cfg)
    px, py = _fix(e), _fix(n)
    return any(_contains(m, first, count, px, py) for first, count in m.polys)


def dist2(cfg, n, e):
    """(the exact squared distance from (n, e) to the nearest edge as a Fraction [m^2], the lowest index of an edge
    attaining it); (None, -1) for a map without edges."""
    m = _map(cfg)
    px, py = _fix(e), _fix(n)
    best, arg = None, -1
    for k, ((ax, ay), (bx, by)) in enumerate(m.edges):
        dx, dy = bx - ax, by - ay
        qx, qy = px - ax, py - ay
        t, len2 = qx * dx + qy * dy, dx * dx + dy * dy
        if t <= 0:
            d = Fraction(qx * qx + qy * qy)
        elif t >= len2:
            d = Fraction((px - bx) ** 2 + (py - by) ** 2)
        else:
            c = qx * dy - qy * dx
            d = Fraction(c * c, len2)
        if best is None or d < best:
            best, arg = d, k
    if best is None:
        return None, -1
    return best / (1 << (2 * _K)), arg


def hull_corners(n, e, L):
    """check_condition.py:50-78: the hull's hard points (n -+ L/2, e -+ L/2), formed in double as the code under test
    forms them (exact for the positions of map_points.py: asserted there)."""
    h = L / 2
    return [(n - h, e - h), (n - h, e + h), (n + h, e - h), (n + h, e + h)]


def hull_grounded(cfg, n, e, L):
    return any(inside(cfg, cn, ce) for cn, ce in hull_corners(n, e, L))


def sqrt_f64(q):
    """The Fraction q's square root, correctly rounded to double (from 2**-100 relative precision)."""
    s = 200
    r = math.isqrt((q.numerator << (2 * s)) // q.denominator)
    return float(Fraction(r, 1 << s))


U = 2.0 ** -53  # the unit roundoff of double


def dist_err_bound(cfg, n, e, d):
    """A bound [m] on |computed - exact| shore distance for a query that evaluates GEOS' pointToSegment in double
    (the oracle's pt_seg; the device's map_dist2_*, which takes one root of the least squared distance instead),
    from its operation count. With C the largest coordinate magnitude of the map and the point, len an edge's length:
      * a vertex's distance: two differences (relative U each) and hypot (or two squares, a sum and a root): under
        4 U d;
      * an edge interior's: c = (ay - py) dx - (ax - px) dy with dx, dy exact (integer vertices); either product
        carries 2 U (its difference's rounding and its own) on a magnitude of at most 2 C len, so the cancelling
        difference is off by at most 2 U (2 C len + 2 C len) + U |c|, where |c| = d len; the division by len^2 (or
        the product with its reciprocal: a rounding more), the root of len^2 and the last product add 4 U d:
        |error| <= 8 U C + 5 U d.
    The nearest edge is the least of values each within that bound, so the least is too."""
    nv = cfg.poly_start[cfg.n_polys]
    C = max([abs(n), abs(e)] + [abs(x) for x in cfg.poly_east[:nv]] + [abs(y) for y in cfg.poly_north[:nv]])
    return U * (8.0 * C + 5.0 * d)


def _exp_neg_sq(d, scale, share):
    """exp(-d^2 / scale) / share of the double d, correctly rounded to double (50 digits in between)."""
    with localcontext() as c:
        c.prec = 50
        return float((-(Decimal(d) * Decimal(d)) / Decimal(scale)).exp() / Decimal(share))


def grounding_terms(d, share=1):
    """reward_function.py:109-117 with reward_designs.py:33-55: the ship under test's grounding term
    exp(-d^2 / 175000) and the obstacle ship's -exp(-d^2 / 50000) for a shore distance d <= 1000 m, 0 beyond; each a
    double, the correctly rounded value of the term at the double d. share: the divisor of the term's share of the
    reward as RewardTracker keeps it (5: the mean of five terms)."""
    if not d <= 1000.0:
        return 0.0, 0.0
    return _exp_neg_sq(d, 175000, share), -_exp_neg_sq(d, 50000, share)
