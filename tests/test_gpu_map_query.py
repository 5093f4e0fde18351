"""The device's coastline query against the exact reference of map_ref.py, at the placed positions of map_points.py
(maps A .. F; a few hundred adversarial positions each: cell lines, the 1000 m gate, the far-shore seam, hull corners
on rings, a sliver narrower than the hull, positions off the grid, a ring of positions around every edge).

Every ship of a launch is put on a position with F_NORTH / F_EAST and F_U = F_V = 0, five ticks into a decision
(as test_gpu_sbmpc_nominal._begin does); the tick's Euler step then leaves the position bit for bit where it was put
(asserted), and the tick's map query, hull test and grounding terms are the placed position's. Env i has its test
ship on position i and its obstacle ship on position i + P / 2, so every position is asked in both roles. A ship put
far from its route fails its navigation on the tick, which ends most decisions there; the envs whose ships are put
on their own routes (map_points.py's on_route family) go on. Only the bits named below are compared.
  (a) the recording step kernel (16 lanes per env, the split corner test on sub-lanes k and k + 4): the recorded
      TE_R_TEST_GROUNDING / TE_R_OBS_GROUNDING against map_ref.grounding_terms within TERM_RTOL plus the distance's
      share, EV_TEST_GROUNDING / EV_OBS_GROUNDING against map_ref.hull_grounded exactly; collav none on every map,
      sbmpc too on A and B;
  (b) every other form that asks the map, from the same placed state, after one tick and on to the decision's end:
      MAP_GRID and MAP_ALL_EDGES, 2 / 4 / 8 / 16 lanes per env, 3 and 4 envs per wave, of shipsim_step,
      shipsim_run_table and shipsim_run_policy (hidden 64, deterministic): ready / events / reward (E_ACC_REWARD where
      the decision goes on) and the ship state equal the recording kernel's bit for bit (it records the placed tick;
      the decisions that go on are finished without the record, whose capacity a decision would exceed). The streams
      have no kernel at 2 lanes per env: a handle created with 2 runs them at 4, an error if that kernel were missing
      (launch_host::select, pinned on the host by tests/launch_host_check.cpp; shipsim_lanes_per_env reports the
      step's lanes, asserted to be the configured ones);
  (c) the K = 2 and K = 3 kernels (a further obstacle ship placed aground freezes), noniw_tick_kernel through
      sim.tick(1, events) and legacy_step_kernel through its status bits: grounding bits equal hull_grounded on A, B, E;
  (d) the sampled intermediate waypoint: E_N_BASE / E_E_BASE put it on a position (scoping angle 0), read back from
      the route table; EV_SAMPLING_FAILURE equals map_ref.inside there, or the waypoint is off the map.
The worst error over tolerance per map is printed, or appended to $SHIPSIM_PARITY_LOG (parity.record; a committed
copy: profiles/map_query_parity.jsonl). Needs an MI355X."""
import numpy as np
import pytest
import torch

import map_points as M
import map_ref as R
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim
from parity import parity_row, record
from test_gpu_stream_reg_consts import _state, _table

pytestmark = pytest.mark.gpu

# The recorded term is exp(-d^2 / o) / 5 of the tick's shore distance d <= 1000 m, o = 175000 (the ship under test)
# or 50000 (the obstacle ship), so the exponent is at most 5.72 resp. 20. Beyond d's own error (dist_tol below):
# the kernel squares d (one rounding, relative U = 2**-53), divides by o through a reciprocal (at most two), which
# moves the exponent by 3 U * 20 = 60 U absolute = the term by 60 U relative; its exp is good to one ulp (2 U) and
# the division by 5 rounds once (U): 63 U. The reference (map_ref.grounding_terms) is the correctly rounded value
# at its d: U. Together 64 U.
TERM_RTOL = 64 * R.U
_GROUND = abi.EV_TEST_GROUNDING | abi.EV_OBS_GROUNDING


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(sim, field):
    return sim.get(field).cpu().numpy()


def _layout(name):
    """(expected values, N, the position index of every env's test ship, of its obstacle ship). The obstacle ship's
    position is half the list on from the test ship's: neighbours in the list are often millimetres apart, which
    would be a collision. On the maps with on-route positions, ON_ROUTE further envs have both ships on their own
    routes (the list's last 2 ON_ROUTE positions: the test ship's, then the obstacle ship's): their decisions go on.
    N is made no multiple of 4 (a partial last wave at 16 lanes per env) by one more env of the first kind."""
    x = M.expected(name)
    P = len(x["pts"])
    t, o = np.arange(P), (np.arange(P) + P // 2) % P
    if name in M.APPLIES["on_route"]:
        t = np.concatenate([t, P - 2 * M.ON_ROUTE + np.arange(M.ON_ROUTE)])
        o = np.concatenate([o, P - M.ON_ROUTE + np.arange(M.ON_ROUTE)])
    if len(t) % 4 == 0:
        t, o = np.append(t, 0), np.append(o, P // 2)
    return x, len(t), t, o


def _dist_tol(name, x):
    """Per position, the relative tolerance of exp(-d^2 / o) that the shore distance's error accounts for, over
    2 d / o: map_ref.dist_err_bound (the bound test_map_query_cpu.py holds the oracle's distance to) covers the
    kernel's operations on the distance, root included, and the reference's own rounding of d."""
    cfg = M.config(name)
    return np.array([R.dist_err_bound(cfg, n, e, d) if np.isfinite(d) else 0.0
                     for (n, e), d in zip(x["pts"], x["d"])])


def _place(sim, name, table, x, t, o, n_ships=2, extra=None):
    """The decision begun, then every ship put on its position at rest. On a map whose bounding box is not the
    reference map's the configured routes leave the horizon, so no waypoint is sampled (the sampling count at its
    maximum from the start: a sampled waypoint off the map would end every decision without a tick). Returns the
    placed (north, east) per ship row and the ticks of the decision in progress per env (0: one is about to start)."""
    N = len(t)
    if not M.default_bounds(name):
        sim.set(abi.E_SAMPLING_COUNT, torch.full((N,), sim.cfg.max_sampling_frequency, dtype=torch.int32))
    out = sim.step(torch.from_numpy(table[0, 0]).cuda(), max_ticks=5)  # (test_gpu_sbmpc_nominal._begin)
    pre = np.where(out["ready"].cpu().numpy() != 0, 0, out["ticks"].cpu().numpy())
    n, e = _np(sim, abi.F_NORTH), _np(sim, abi.F_EAST)
    for k, idx in enumerate((t, o) + tuple(extra or ())):
        n[k::n_ships], e[k::n_ships] = x["pts"][idx, 0], x["pts"][idx, 1]
    sim.set(abi.F_NORTH, torch.from_numpy(n))
    sim.set(abi.F_EAST, torch.from_numpy(e))
    for f in (abi.F_U, abi.F_V):
        sim.set(f, torch.zeros(len(n), dtype=torch.float64))
    sim.set(abi.F_STOP, torch.zeros(len(n), dtype=torch.int32))
    # (the tracker counts the obstacle ship's jump as travel: far below its limit, so that the decision goes on where
    # nothing else ends it)
    sim.set(abi.E_TRAVEL_DIST, torch.full((N,), -1e9, dtype=torch.float64))
    return np.stack([n, e], 1), pre


def _assert_in_place(sim, placed):
    got = np.stack([_np(sim, abi.F_NORTH), _np(sim, abi.F_EAST)], 1)
    np.testing.assert_array_equal(got, placed, err_msg="the tick moved a ship placed at rest")


# ---- (a) the recording step kernel against the reference ----------------------------------------------------------
CASES_A = [(name, "none") for name in M.NAMES] + [("A", "sbmpc"), ("B", "sbmpc")]


@pytest.mark.parametrize("name,collav", CASES_A)
def test_recording_step_kernel_equals_exact_reference(name, collav):
    x, N, t, o = _layout(name)
    assert N % 4 and N >= 13
    cfg = M.config(name, collav)
    sim = ShipSim(cfg, N)
    traj = sim.set_trajectory(16)
    sim.reset()
    placed, _ = _place(sim, name, _table(1, 1, N, seed=5), x, t, o)
    before = traj["len"].cpu().numpy().copy()
    assert sim.lanes_per_env == 16
    sim.step(torch.zeros(N, dtype=torch.float32), max_ticks=1)
    _assert_in_place(sim, placed)
    ln = traj["len"].cpu().numpy()
    np.testing.assert_array_equal(ln, before + 1)  # exactly one tick, recorded
    # (len counts the ships' rows, which start with the reset's: the env rows are one fewer)
    row = traj["env"].cpu().numpy()[np.arange(N), ln - 2]
    bits = row[:, abi.TE_BITS].astype(np.int64)
    want = np.where(x["grounded"][t], abi.EV_TEST_GROUNDING, 0) | np.where(x["grounded"][o], abi.EV_OBS_GROUNDING, 0)
    bad = np.nonzero((bits & _GROUND) != want)[0]
    assert not len(bad), [(int(i), x["family"][t[i]], x["pts"][t[i]], x["family"][o[i]], x["pts"][o[i]],
                           hex(bits[i]), hex(want[i])) for i in bad[:8]]
    dtol = _dist_tol(name, x)
    worst, unpinned, off_gate = 0.0, 0, 0
    for col, idx, k, scale in ((abi.TE_R_TEST_GROUNDING, t, 0, 175000.0), (abi.TE_R_OBS_GROUNDING, o, 1, 50000.0)):
        got, ref, d = row[:, col], x["terms"][idx, k], x["d"][idx]
        tol = np.abs(ref) * (TERM_RTOL + np.where(np.isfinite(d), 2.0 * d, 0.0) * dtol[idx] / scale)
        err = np.abs(got - ref)
        # exactly 1000 m from an edge's interior the kernel's c^2 / len^2 and the reference round apart (DESIGN.md
        # section 5: parity unpinned there): map_points.py's edge_1000 family, counted and not held to the tolerance
        edge_1000 = np.array([q == 10 ** 6 for q in x["d2"]])[idx] & ~_vertex_attains(name, x)[idx]
        assert (np.array(x["family"])[idx][edge_1000] == "edge_1000").all()
        unpinned += int(edge_1000.sum())
        off_gate += int(((got != 0) != (ref != 0))[edge_1000].sum())
        err = np.where(edge_1000, 0.0, err)
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
        i = int(ratio.argmax())
        print(f"\n[map {name} {collav}] term {col}: worst error / tolerance {ratio[i]:.3f} at {x['pts'][idx[i]]} "
              f"({x['family'][idx[i]]}): got {got[i]!r} ref {ref[i]!r} d {d[i]!r}")
        worst = max(worst, float(ratio[i]))
        assert ratio[i] <= 1.0, (name, col, x["family"][idx[i]], x["pts"][idx[i]], got[i], ref[i], d[i])
    print(f"[map {name} {collav}] exactly 1000 m from an edge's interior: {unpinned} queries, {off_gate} off the gate")
    fam = np.array(x["family"])
    record(parity_row(f"map_query_recording_step_vs_exact[{name}-{collav}]", envs_checked=N, worst_over_tolerance=worst,
                      families={f: int((fam == f).sum()) for f in M.FAMILIES}, edge_interior_at_1000=unpinned,
                      edge_interior_at_1000_off_gate=off_gate,
                      grounded=int(x["grounded"].sum())))
    sim.close()


_vertex_cache = {}


def _vertex_attains(name, x):
    """Per position: the exact shore distance is a vertex's (both sides then compute it from two exact squares)."""
    if name not in _vertex_cache:
        from fractions import Fraction
        cfg = M.config(name)
        verts = [(Fraction(e), Fraction(n)) for ring in R.rings(cfg) for e, n in ring]
        out = []
        for (n, e), q in zip(x["pts"], x["d2"]):
            fn, fe = Fraction(float(n)), Fraction(float(e))
            out.append(q is not None and any((fe - ve) ** 2 + (fn - vn) ** 2 == q for ve, vn in verts))
        _vertex_cache[name] = np.array(out)
    return _vertex_cache[name]


# ---- (b) every other form that asks the map -----------------------------------------------------------------------
def _config(name, collav, mq, lpe, epw, **kw):
    cfg = M.config(name, collav, **kw)
    cfg.map_query, cfg.lanes_per_env, cfg.envs_per_wave = mq, lpe, epw
    return cfg


def _step_run(cfg, name, table, x, t, o, record_rows=False):
    """The sliced step from the placed state: one tick, then on to the decision's end. Returns what the forms are
    compared in."""
    N = len(t)
    sim = ShipSim(cfg, N)
    if record_rows:
        sim.set_trajectory(8, env_rows=True)
    sim.reset()
    placed, pre = _place(sim, name, table, x, t, o)
    a = torch.from_numpy(table[0, 0]).cuda()
    o1 = {k: v.cpu().numpy().copy() for k, v in sim.step(a, max_ticks=1).items()}
    _assert_in_place(sim, placed)
    r = dict(pre=pre, ready=o1["ready"] != 0, state1=_state(sim), acc1=_np(sim, abi.E_ACC_REWARD),
             lpe=sim.lanes_per_env)
    first = {k: o1[k].copy() for k in ("reward", "events", "done", "ticks", "obs")}
    if record_rows:
        sim.clear_trajectory()
    go = ~r["ready"]
    o2 = {k: v.cpu().numpy() for k, v in sim.step(a, active=torch.from_numpy(go.astype(np.uint8)), max_ticks=0).items()}
    assert (o2["ready"][go] != 0).all()
    for k in first:  # every env's first completed decision from the placed state
        first[k][go] = o2[k][go]
    first["ticks"] = first["ticks"] + np.where(go, 1, 0) + pre
    r.update(first=first, state2=_state(sim))
    sim.close()
    return r


def _stream_run(cfg, name, table, x, t, o, policy=None):
    N = len(t)
    sim = ShipSim(cfg, N)
    sim.reset()
    placed, pre = _place(sim, name, table, x, t, o)
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, 16, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    tab = torch.from_numpy(np.repeat(table, 4, 0)).cuda()

    def launch(T):
        if policy is None:
            return sim.run_table(tab, T, ep, dec, log=log, log_len=log_len)
        return sim.run_policy(policy, T, 1, ep, dec, deterministic=True, log=log, log_len=log_len)

    launch(1)
    ready = log_len.cpu().numpy() >= 1
    r = dict(pre=pre, ready=ready, state1=_state(sim), acc1=_np(sim, abi.E_ACC_REWARD), lpe=sim.lanes_per_env)
    if not ready.all():
        _assert_in_place_rows(sim, placed, np.repeat(~ready, 2))
    for _ in range(4):  # on to the end of every env's decision (a launch stops an env at a full log)
        if (log_len.cpu().numpy() >= 1).all():
            break
        launch(1500)
    ln, L = log_len.cpu().numpy(), log.cpu().numpy()
    assert (ln >= 1).all()
    rec = L[:, 0]
    r["first"] = dict(reward=rec[:, abi.DL_REWARD], events=rec[:, abi.DL_EVENTS].astype(np.int64).astype(np.int32),
                      done=rec[:, abi.DL_DONE].astype(np.uint8), ticks=rec[:, abi.DL_TICKS].astype(np.int32),
                      obs=rec[:, abi.DL_OBS:abi.DL_OBS + 8].astype(np.float32))
    sim.close()
    return r


def _assert_in_place_rows(sim, placed, rows):
    got = np.stack([_np(sim, abi.F_NORTH), _np(sim, abi.F_EAST)], 1)
    np.testing.assert_array_equal(got[rows], placed[rows], err_msg="the tick moved a ship placed at rest")


def _assert_same(ref, got, what, stream):
    np.testing.assert_array_equal(got["pre"], ref["pre"], err_msg=what)
    np.testing.assert_array_equal(got["ready"], ref["ready"], err_msg=what + ": ready after one tick")
    go = ~ref["ready"]
    rows = np.repeat(go, 2)
    # where the decision goes on: the reward so far and the ship state, after one tick (a stream has reset the others)
    np.testing.assert_array_equal(got["acc1"][go], ref["acc1"][go], err_msg=what + ": E_ACC_REWARD")
    np.testing.assert_array_equal(got["state1"][rows], ref["state1"][rows], err_msg=what + ": ship state, one tick")
    if not stream:
        np.testing.assert_array_equal(got["acc1"], ref["acc1"], err_msg=what + ": E_ACC_REWARD")
        np.testing.assert_array_equal(got["state1"], ref["state1"], err_msg=what + ": ship state, one tick")
        np.testing.assert_array_equal(got["state2"], ref["state2"], err_msg=what + ": ship state, decision's end")
    for k in ("reward", "events", "done", "ticks", "obs"):  # (obs: both ships' positions at the decision's end)
        np.testing.assert_array_equal(got["first"][k], ref["first"][k], err_msg=f"{what}: first decision's {k}")


_policy = {}


def _policy_weights():
    if not _policy:
        from test_gpu_policy_act import _trainer
        tr, _ = _trainer(64)
        _policy["tr"], _policy["dp"] = tr, tr.device_policy(True)
    return _policy["dp"].weights()


@pytest.mark.parametrize("name", M.NAMES)
def test_every_form_equals_the_recording_kernel(name):
    x, N, t, o = _layout(name)
    collav = "sbmpc" if name == "B" else "none"
    table = _table(1, 1, N, seed=9)
    ref = _step_run(_config(name, collav, abi.MAP_GRID, 16, 0), name, table, x, t, o, record_rows=True)
    assert ref["lpe"] == 16
    # the recorded tick's grounding bits where it completed the decision are the reference's (the link to (a))
    done1 = ref["ready"]
    ev = ref["first"]["events"].astype(np.int64)
    want = np.where(x["grounded"][t], abi.EV_TEST_GROUNDING, 0) | np.where(x["grounded"][o], abi.EV_OBS_GROUNDING, 0)
    np.testing.assert_array_equal((ev & _GROUND)[done1], want[done1])
    assert (want[~done1] == 0).all()  # (a grounding ends the decision on its tick)
    runs = 0
    for mq in (abi.MAP_GRID, abi.MAP_ALL_EDGES):
        for lpe in (2, 4, 8, 16):
            for epw in (3, 4):
                what = f"map {name} map_query {mq} lanes {lpe} envs per wave {epw}"
                cfg = _config(name, collav, mq, lpe, epw)
                got = _step_run(cfg, name, table, x, t, o)
                _assert_same(ref, got, what + " step", stream=False)
                assert got["lpe"] == lpe  # (the lanes the step kernel ran at: shipsim_lanes_per_env)
                got = _stream_run(cfg, name, table, x, t, o)
                _assert_same(ref, got, what + " table stream", stream=True)
                got = _stream_run(cfg, name, table, x, t, o, policy=_policy_weights())
                _assert_same(ref, got, what + " policy stream", stream=True)
                runs += 3
    assert runs == 48
    # decisions that go on past the placed tick: every env whose ships are on their own routes, at the least
    if name in M.APPLIES["on_route"]:
        on = np.arange(len(x["pts"]), len(x["pts"]) + M.ON_ROUTE)
        assert not done1[on].any() and (ref["first"]["ticks"][on] >= 10).all(), (done1[on], ref["first"]["ticks"][on])
    print(f"\n[map {name}] {int(done1.sum())} of {N} decisions ended on the placed tick, the others after "
          f"{int(ref['first']['ticks'][~done1].min()) if (~done1).any() else 0} .. "
          f"{int(ref['first']['ticks'][~done1].max()) if (~done1).any() else 0} ticks")


# ---- (c) the other kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_multi_obstacle_kernels_ground_as_the_reference(name, K):
    """Env i: the test ship on position i, obstacle ship 1 on i + P / 2, obstacle ships 2 .. K on i + 2 ..; the travel
    tracker past its limit, so the placed tick ends the decision and the step returns its event bits. A further
    obstacle ship whose hull is aground freezes (F_STOP), one in open water inside the horizon does not."""
    x, N, t, o = _layout(name)
    P = len(x["pts"])
    extra = [(np.arange(N) + k) % P for k in range(2, K + 1)]
    cfg = M.config(name, "none", n_obs_ships=K)
    sim = ShipSim(cfg, N)
    sim.reset()
    placed, _ = _place(sim, name, _table(1, 1, N, seed=7), x, t, o, n_ships=K + 1, extra=extra)
    sim.set(abi.E_TRAVEL_DIST, torch.full((N,), 1e9, dtype=torch.float64))
    out = sim.step(torch.zeros(N, dtype=torch.float32), max_ticks=1)
    assert (out["ready"].cpu().numpy() != 0).all() and (out["ticks"].cpu().numpy() == 1).all()
    _assert_in_place(sim, placed)
    ev = out["events"].cpu().numpy().astype(np.int64)
    g = x["grounded"]
    np.testing.assert_array_equal(ev & _GROUND, np.where(g[t], abi.EV_TEST_GROUNDING, 0) |
                                  np.where(g[o], abi.EV_OBS_GROUNDING, 0))
    stop = _np(sim, abi.F_STOP).reshape(N, K + 1)
    b = M.Grid(cfg)
    for k, idx in enumerate(extra, start=2):
        assert stop[g[idx], k].all(), (name, K, k)
        n, e = x["pts"][idx].T
        s = cfg.ship[k]
        open_water = ~g[idx] & (n > b.mn_n + 40) & (n < b.mx_n - 40) & (e > b.mn_e + 40) & (e < b.mx_e - 40) & \
            (np.hypot(n - s.route_north[s.n_route - 1], e - s.route_east[s.n_route - 1]) > 201.0)
        assert not stop[open_water, k].any(), (name, K, k)
        assert g[idx].sum() >= 10 and (open_water.sum() >= 10 or not M.default_bounds(name))
    sim.close()


@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_noniw_tick_kernel_grounds_as_the_reference(name):
    x, N, t, o = _layout(name)
    cfg = M.set_map(abi.c1_config("none"), M.MAPS[name])
    sim = ShipSim(cfg, N)
    sim.reset()
    n, e = _np(sim, abi.F_NORTH), _np(sim, abi.F_EAST)
    n[0::2], e[0::2], n[1::2], e[1::2] = x["pts"][t, 0], x["pts"][t, 1], x["pts"][o, 0], x["pts"][o, 1]
    sim.set(abi.F_NORTH, torch.from_numpy(n))
    sim.set(abi.F_EAST, torch.from_numpy(e))
    for f in (abi.F_U, abi.F_V):
        sim.set(f, torch.zeros(2 * N, dtype=torch.float64))
    ev = torch.zeros(N, dtype=torch.int32, device=sim.device)
    sim.tick(1, ev)
    _assert_in_place(sim, np.stack([n, e], 1))
    bits = ev.cpu().numpy().astype(np.int64)
    g = x["grounded"]
    np.testing.assert_array_equal(bits & _GROUND, np.where(g[t], abi.EV_TEST_GROUNDING, 0) |
                                  np.where(g[o], abi.EV_OBS_GROUNDING, 0))
    sim.close()


@pytest.mark.parametrize("name", ["A", "B", "E"])
def test_legacy_step_kernel_grounds_as_the_reference(name):
    x, N, t, o = _layout(name)
    sim = ShipSim(M.config(name, "none"), N)
    sim.reset()
    n, e = _np(sim, abi.F_NORTH), _np(sim, abi.F_EAST)
    n[0::2], e[0::2], n[1::2], e[1::2] = x["pts"][t, 0], x["pts"][t, 1], x["pts"][o, 0], x["pts"][o, 1]
    sim.set(abi.F_NORTH, torch.from_numpy(n))
    sim.set(abi.F_EAST, torch.from_numpy(e))
    for f in (abi.F_U, abi.F_V):
        sim.set(f, torch.zeros(2 * N, dtype=torch.float64))
    out = sim.legacy_step(1)
    _assert_in_place(sim, np.stack([n, e], 1))
    status = out["status"].cpu().numpy().astype(np.int64)
    g = x["grounded"]
    np.testing.assert_array_equal(status & (abi.LT_TEST_GROUNDED | abi.LT_OBS_GROUNDED),
                                  np.where(g[t], abi.LT_TEST_GROUNDED, 0) | np.where(g[o], abi.LT_OBS_GROUNDED, 0))
    sim.close()


# ---- (d) the sampled waypoint ---------------------------------------------------------------------------------------
def _waypoints(name):
    """The map's positions, and points exactly on its rings: every vertex and every edge's midpoint (exact: integer
    vertices). (k, 2) of (north, east)."""
    cfg = M.config(name)
    g = M.Grid(cfg)
    on = [(ay, ax) for ax, ay, bx, by in g.edges] + [((ay + by) / 2, (ax + bx) / 2) for ax, ay, bx, by in g.edges]
    return cfg, g, np.concatenate([M.expected(name)["pts"], np.array(on).reshape(-1, 2)]), len(on)


@pytest.mark.parametrize("lpe", [16, 4])
@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_sampled_waypoint_fails_where_the_reference_is_inside(name, lpe):
    """A scoping angle of 0 samples the base point itself (l_s = 0), so E_N_BASE / E_E_BASE choose the waypoint: cells
    wholly in land, wholly in water, mixed cells on land and on water, and points exactly on a ring (not inside)."""
    cfg, g, wp, n_on = _waypoints(name)
    cfg.lanes_per_env = lpe
    N = len(wp)
    x = M.expected(name)
    inside = np.concatenate([x["inside"], np.zeros(n_on, bool)])
    assert all(not R.inside(cfg, n, e) and R.dist2(cfg, n, e)[0] == 0 for n, e in wp[-n_on:])
    off_map = (wp[:, 0] < g.mn_n) | (wp[:, 0] > g.mx_n) | (wp[:, 1] < g.mn_e) | (wp[:, 1] > g.mx_e)
    cls = np.array([g.flag[c] if (c := g.cell(n, e)) is not None else -1 for n, e in wp])
    for kind, land in ((M.GRID_IN, True), (M.GRID_OUT, False), (M.GRID_MIXED, True), (M.GRID_MIXED, False)):
        assert ((cls == kind) & (inside == land) & ~off_map).any() or (kind == M.GRID_IN and name == "E"), (kind, land)
    sim = ShipSim(cfg, N)
    sim.reset()
    sim.set(abi.E_N_BASE, torch.from_numpy(wp[:, 0].copy()))
    sim.set(abi.E_E_BASE, torch.from_numpy(wp[:, 1].copy()))
    out = sim.step(torch.zeros(N, dtype=torch.float32), max_ticks=1)
    rl = _np(sim, abi.E_ROUTE_LEN)[1::2]
    rn, re = _np(sim, abi.E_ROUTE_NORTH)[1::2], _np(sim, abi.E_ROUTE_EAST)[1::2]
    got = np.stack([rn[np.arange(N), rl - 2], re[np.arange(N), rl - 2]], 1)  # inserted in front of the route's end
    np.testing.assert_array_equal(got, wp)
    ready, ticks = out["ready"].cpu().numpy() != 0, out["ticks"].cpu().numpy()
    failed = ready & (ticks == 0) & ((out["events"].cpu().numpy().astype(np.int64) & abi.EV_SAMPLING_FAILURE) != 0)
    np.testing.assert_array_equal(failed, inside | off_map)
    assert (ticks[~failed] == 1).all()
    sim.close()
