"""The CPU oracle's coastline query (oracle_map_query: if_pos_inside_obstacles and obstacles_distance, as the episode
loop calls them) against the exact reference of map_ref.py, on every position of every map of map_points.py; and the
conditions the positions themselves must meet, asserted on the exact reference alone. The worst distance error over
its bound (map_ref.dist_err_bound, the yardstick of test_gpu_map_query.py's tolerance) is printed per map, or appended
to $SHIPSIM_PARITY_LOG (parity.record; a committed copy: profiles/map_query_parity.jsonl)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import map_points as M
import map_ref as R
import oracle_ffi as O
from parity import parity_row, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_maps_are_valid_and_sized(tmp_path):
    """shipsim_create's validate accepts every map, and the grid its host half builds has the cell classes
    map_points.Grid restates (tests/map_config_check.cpp, a stand-alone program of the library's host code)."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "map_config_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ast_sac_amd", "csrc"),
                    os.path.join(ROOT, "tests", "map_config_check.cpp"), "-o", exe], check=True)
    for name in M.NAMES:
        cfg = M.config(name, "sbmpc")
        assert cfg.poly_start[cfg.n_polys] == M.N_VERTS[name], name
        path = tmp_path / f"{name}.cfg"
        path.write_bytes(bytes(cfg))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        g = M.Grid(cfg)
        head, flags = r.stdout.splitlines() if g.on else (r.stdout.strip(), "")
        assert head == (f"ok 1 {g.gnx} {g.gny}" if g.on else "ok 0 0 0"), (name, head)
        if g.on:
            np.testing.assert_array_equal(np.array(list(flags), int).reshape(g.gny, g.gnx), g.flag, err_msg=name)
        assert g.on == (name in ("A", "B", "C", "E")), name
        if M.default_bounds(name):
            assert (g.mn_e, g.mx_e, g.mn_n, g.mx_n) == (0.0, 20000.0, 0.0, 10000.0), name
        for ring in M.MAPS[name]:
            for e, n in ring:
                assert e == int(e) and n == int(n) and 0 <= e <= 20000 and 0 <= n <= 10000, (name, e, n)
    assert len(M.MAPS["D128"]) == 16
    f = M.Grid(M.config("B")).flag
    assert (f == M.GRID_IN).sum() >= 9 and (f == M.GRID_OUT).any() and (f == M.GRID_MIXED).any()


@pytest.mark.parametrize("name", M.NAMES)
def test_positions_meet_their_conditions(name):
    x = M.expected(name)
    pts, fam = x["pts"], np.array(x["family"])
    count = {f: int((fam == f).sum()) for f in M.FAMILIES}
    print(f"\n[map {name}] {len(pts)} positions: {count}")
    for f in M.FAMILIES:  # each family is non-empty on each map it applies to
        assert count[f] > 0 or name not in M.APPLIES[f], (name, f)
    assert len(pts) >= (12 if name == "F" else 150)
    # no position's exact shore distance lies within 1e-9 m of 1000 m, but for those exactly there; only the
    # threshold family comes nearer than a micrometre, and its members are exactly 1000 m or a representable step off
    lo, hi = Fraction(1000) - Fraction(1, 10 ** 9), Fraction(1000) + Fraction(1, 10 ** 9)
    for k, q in enumerate(x["d2"]):
        if q is None:
            continue
        if lo * lo < q < hi * hi and q != 10 ** 6:
            assert fam[k] == "threshold", (name, fam[k], pts[k], float(q))
    if name != "F":
        exact = [q == 10 ** 6 for q in x["d2"]]
        thr = fam == "threshold"
        # exactly 1000 m otherwise only where a family is made for it: from a vertex (reach, exact on every side:
        # two exact squares) and from an edge's interior (edge_1000: unpinned, counted)
        assert set(fam[np.array(exact)]) <= {"threshold", "reach", "edge_1000"}, name
        assert np.array(exact)[fam == "edge_1000"].all()
        assert np.array(exact)[thr][0::3].all() and not np.array(exact)[thr][1::3].any(), name
        assert not np.array(exact)[thr][2::3].any()
        d2 = np.array([float(q) for q in x["d2"]])
        assert (d2[thr][1::3] > 1e6).all() and (d2[thr][2::3] < 1e6).all()  # a step out, a step in
        assert x["inside"][fam == "off_grid"].any()  # a centre in land
    if name in ("C", "D128"):  # every edge is the exact nearest edge of at least one position
        assert set(x["edge"]) == set(range(M.N_VERTS[name])), sorted(set(range(M.N_VERTS[name])) - set(x["edge"]))
    if name == "B":
        d = x["d"]
        assert ((d > 990.0) & (d <= 1000.0))[fam == "reach"].sum() >= 10
        seam = fam == "seam"
        assert ((d < M.LIM) & seam).sum() >= 9 and ((d > M.LIM) & seam).sum() >= 9
        assert (np.abs(d - M.LIM) < 2e-9)[seam].sum() >= 4
        # a hull corner in land across a cell line, the centre in an unmixed water cell, nearer shore than lim and
        # further than half the hull
        g = M.Grid(M.config("B"))
        far = [k for k in np.nonzero(seam)[0] if x["grounded"][k] and not x["inside"][k] and 40.001 < d[k] < M.LIM
               and g.flag[g.cell(*pts[k])] == M.GRID_OUT]
        assert len(far) >= 3, far
        assert any(g.flag[g.cell(*pts[k])] == M.GRID_IN for k in np.nonzero(seam)[0])
    if name in M.APPLIES["on_route"]:  # in open water inside the horizon, test ship's then obstacle ship's
        r = fam == "on_route"
        assert r.sum() == 2 * M.ON_ROUTE and (np.nonzero(r)[0] == np.arange(len(pts) - 2 * M.ON_ROUTE, len(pts))).all()
        assert not x["grounded"][r].any() and not x["inside"][r].any() and (x["d"][r] > 100.0).all()
        assert (pts[r] > 40.0).all() and (pts[r, 0] < 9960.0).all() and (pts[r, 1] < 19960.0).all()
    if name == "E":
        s = fam == "sliver"
        assert (x["inside"][s] & ~x["grounded"][s]).sum() >= 4  # astride: the centre in the sliver, no corner
        assert (~x["inside"][s] & x["grounded"][s]).sum() >= 4  # a corner in it
    if name in ("A", "B", "C", "D65", "D128", "E"):
        c = fam == "corners"
        on_ring = 0  # hull corners exactly on a ring: not inside, at exact distance 0
        cfg = M.config(name)
        for n, e in pts[c]:
            for cn, ce in R.hull_corners(n, e, 2 * M.HALF):
                if R.dist2(cfg, cn, ce)[0] == 0:
                    assert not R.inside(cfg, cn, ce)
                    on_ring += 1
        assert on_ring >= 12, on_ring


@pytest.mark.parametrize("name", M.NAMES)
def test_oracle_query_equals_exact_reference(name):
    cfg = M.config(name)
    x = M.expected(name)
    pts = x["pts"]
    inside, dist = O.map_query(cfg, pts)
    np.testing.assert_array_equal(inside != 0, x["inside"])
    # the hull test as the episode loop asks it: the four hard points
    h = M.HALF
    corners = np.concatenate([pts + [sn * h, se * h] for sn in (-1, 1) for se in (-1, 1)])
    ci, _ = O.map_query(cfg, corners)
    np.testing.assert_array_equal(ci.reshape(4, -1).any(0), x["grounded"])
    if name == "F":
        assert np.isinf(dist).all()
        worst = 0.0
    else:
        bound = np.array([R.dist_err_bound(cfg, n, e, d) for (n, e), d in zip(pts, x["d"])])
        err = np.array([abs(float(Fraction(float(got)) - _sqrt_hi(q))) for got, q in zip(dist, x["d2"])])
        ratio = err / bound
        worst = float(ratio.max())
        k = int(ratio.argmax())
        print(f"\n[map {name}] oracle distance: worst error / bound {worst:.3f} at {pts[k]} ({x['family'][k]}), "
              f"error {err[k]:.3e} m of {x['d'][k]:.3f} m")
        assert worst <= 1.0
        # the reward's gate, exactly: the threshold family's members on the threshold are on it in the oracle too.
        # Exactly 1000 m from an edge's interior the oracle's |c / len^2| sqrt(len^2) may round past it: counted
        pinned = np.array(x["family"]) != "edge_1000"
        np.testing.assert_array_equal((dist <= 1000.0)[pinned], (x["d"] <= 1000.0)[pinned])
        off_gate = int(((dist <= 1000.0) != (x["d"] <= 1000.0)).sum())
        print(f"[map {name}] exactly 1000 m from an edge's interior: {int((~pinned).sum())} positions, the oracle off "
              f"the gate at {off_gate}")
    record(parity_row(f"map_query_oracle_vs_exact[{name}]", envs_checked=len(pts), worst_over_tolerance=worst,
                      families={f: x["family"].count(f) for f in M.FAMILIES},
                      edge_interior_at_1000=x["family"].count("edge_1000"),
                      edge_interior_at_1000_off_gate=off_gate if name != "F" else 0))


def _sqrt_hi(q):
    """sqrt of the Fraction q to 2**-200 relative, as a Fraction."""
    import math
    s = 200
    return Fraction(math.isqrt((q.numerator << (2 * s)) // q.denominator), 1 << s)
