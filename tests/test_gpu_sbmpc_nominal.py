"""The two-ship decision streams (shipsim_run_table / shipsim_run_policy, collav sbmpc, 16 lanes per env) answer an
SBMPC request whose nominal scenario provably wins (csrc/shipsim_sbmpc_nominal.hpp) on the requesting env's own lanes
and run the wave-cooperative pass only for the requests left. The sliced shipsim_step kernels always run the pass, so
the host-driven step loop (the harness of test_gpu_flat_tick.py) is the independent reference.
  1. the device entry (shipsim_sbmpc_nominal) against the host's flags on the CPU test's batch, both forms: the test on
     sin / cos(chi_d) and the form the streams' tick evaluates (segment sine and cosine with the correction's argument)
     on the split course; and the unchanged pass (shipsim_sbmpc_eval) on every accepted row: exactly (1.0, 0.0, 1);
  2. the table stream against the host-driven loop, bit for bit, with the test ship placed relative to the obstacle
     ship five ticks into a decision so that the first tick's requests are, per wave: all accepted; two accepted beside
     two refused (a paired pass beside answered lanes); one refused beside three accepted (a lone, split pass); an env
     whose memory is off (1, 0) at an accepted distance; a request on the tick of a waypoint advance, the obstacle
     ship's and the test ship's own (its segment's angle, sine and cosine re-formed on that tick). N = 16 at four envs
     per wave, N = 5 and 9 at three (partial waves). Which requests are accepted is asserted from the host test on the
     placed state;
  3. the policy stream the same way at N = 9, three envs per wave (a lone pass, a paired pass, the memory-off and both
     advance cases), its logged actions replayed through the host-driven loop.
Needs an MI355X."""
import numpy as np
import pytest
import torch

import oracle_ffi as O
from ast_sac_amd import shipsim, shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim
from test_gpu_flat_tick import _PRE, _begin, _Host
from test_gpu_flat_tick import _Stream as _PlacedStream
from test_gpu_stream_reg_consts import _KEEP, _state, _table
from test_sbmpc_nominal_cpu import host_flags, nominal_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(sim, field):
    return sim.get(field).cpu().numpy()


def test_device_test_equals_host_test_and_the_pass_agrees():
    req, flags, ratio = nominal_batch()
    assert len(req) == 4096 and (np.abs(ratio - 1) > 1e-9).all()
    sflags, sratio = host_flags(req, seg=True)  # the form the streams' tick evaluates, on the split course
    assert (np.abs(sratio - 1) > 1e-9).all()
    got = shipsim.sbmpc_nominal(req).cpu().numpy()
    np.testing.assert_array_equal((got & 1) != 0, flags)
    np.testing.assert_array_equal((got & 2) != 0, sflags)
    assert ((got & ~3) == 0).all()
    out = shipsim.sbmpc_eval(req).cpu().numpy()
    acc = out[flags | sflags]
    assert len(acc) >= 0.2 * len(req)
    np.testing.assert_array_equal(acc, np.tile([1.0, 0.0, 1.0], (len(acc), 1)))  # (1.0, 0.0, active) on every row
    assert not np.signbit(acc[:, 1]).any()
    assert (out[~flags][:, :2] != [1.0, 0.0]).any()  # (the pass does choose other scenarios among the refused)
    # other memory values: refused on the device as on the host
    other = req[flags][:108].copy()
    p = np.tile(np.repeat([0.4, 0.6, 0.8, 1.0], 7), 4)[:108]
    c = np.tile(np.deg2rad(np.arange(-30, 31, 10)), 16)[:108]
    keep = ~((p == 1.0) & (c == 0.0))
    other[:, 0], other[:, 1] = p, c
    assert not shipsim.sbmpc_nominal(other[keep]).cpu().numpy().any()
    # a NaN in a field the test reads refuses
    bad = req[flags][:15].copy()
    for k, col in enumerate((0, 1, 2, 3, 4, 5, 8, 10, 11, 12, 13, 14, 15)):
        bad[k, col] = np.nan
    got = shipsim.sbmpc_nominal(bad).cpu().numpy()
    assert not got[:13].any() and (got[13:] == 3).all()


_WP_OFF = (-3.0, 2.0)  # "tadv": the test ship's next waypoint, from the ship (inside its radius of acceptance)


def _request_rows(cfg, st, n_t, e_t, own_wp=()):
    """The request rows (N, SBMPC_IN) the next tick forms from the state `st` with the test ships at (n_t, e_t):
    csrc's LOS term and its windup restated (los_q, los_windup), the obstacle ship as the tick's start has it.
    own_wp: envs whose test ship's next waypoint is moved to _WP_OFF from the ship."""
    N = len(n_t)
    c = cfg.ship[0]
    t, o = np.arange(N) * 2, np.arange(N) * 2 + 1
    nw = st["nw"][t]
    pn, pe = st["rn"][t, nw - 1], st["re"][t, nw - 1]
    wn, we = st["rn"][t, nw].copy(), st["re"][t, nw].copy()
    for i in own_wp:
        wn[i], we[i] = n_t[i] + _WP_OFF[0], e_t[i] + _WP_OFF[1]
    alpha = np.arctan2(we - pe, wn - pn)
    e_ct = -(n_t - pn) * np.sin(alpha) + (e_t - pe) * np.cos(alpha)
    r = c.lookahead_distance
    e_ct = np.where(e_ct * e_ct >= r * r, 0.99 * r, e_ct)
    q = e_ct / np.maximum(1e-6, np.sqrt(r * r - e_ct * e_ct))
    ei = st["ei"][t]
    ei = np.where(np.abs(ei + q) <= c.los_integrator_windup_limit, ei + q, ei)
    chi_d = -(alpha + np.arctan(-q - ei * c.los_integral_gain))
    z = np.zeros(N)
    return np.stack([st["p_last"], st["chi_last"], np.full(N, c.desired_forward_speed), chi_d, e_t, n_t, z, z,
                     st["v"][t], z, st["e"][o], st["n"][o], -st["yaw"][o], st["u"][o], st["v"][o],
                     np.full(N, cfg.ship[1].length_of_ship), np.full(N, cfg.ship[1].width_of_ship)], 1)


def _read(sim):
    return dict(n=_np(sim, abi.F_NORTH).astype(np.float64), e=_np(sim, abi.F_EAST).astype(np.float64),
                yaw=_np(sim, abi.F_YAW), u=_np(sim, abi.F_U), v=_np(sim, abi.F_V), ei=_np(sim, abi.F_E_CT_INT),
                nw=_np(sim, abi.F_NEXT_WPT), rn=_np(sim, abi.E_ROUTE_NORTH), re=_np(sim, abi.E_ROUTE_EAST),
                rl=_np(sim, abi.E_ROUTE_LEN), p_last=_np(sim, abi.E_SBMPC_P_LAST).astype(np.float64),
                chi_last=_np(sim, abi.E_SBMPC_CHI_LAST).astype(np.float64))


def _place(cfg, sim, plan, seen):
    """Move the test ship of every planned env to an offset from its obstacle ship, inside D_INIT, at which the host
    test accepts ("acc", "mem", "adv", "tadv": ratio < 0.5) or refuses ("ref": ratio > 2) the request the next tick
    forms. "mem": the memory set off (1, 0). "adv": the obstacle ship put on its next waypoint first (its advance on the
    tick). "tadv": the test ship's own next waypoint moved next to the placed ship (the route table rewritten), so the
    test ship's index advances and its segment's angle, sine and cosine are re-formed on the requesting tick.
    The offsets are searched on a polar grid around the obstacle ship, per env, on the state itself."""
    st = _read(sim)
    N = len(st["p_last"])
    for i, kind in plan.items():
        if kind == "adv":
            o = 2 * i + 1
            assert st["rl"][o] > st["nw"][o] + 1, (st["rl"][o], st["nw"][o])
            st["n"][o], st["e"][o] = st["rn"][o, st["nw"][o]] + 3.0, st["re"][o, st["nw"][o]] - 2.0
        if kind == "mem":
            st["p_last"][i], st["chi_last"][i] = 0.8, np.deg2rad(10.0)
    rest = dict(st, p_last=np.ones(N), chi_last=np.zeros(N))  # (the geometry's verdict: the rest memory)
    n_t, e_t = st["n"][0::2].copy(), st["e"][0::2].copy()
    grid = [(r, a) for r in (1800.0, 1500.0, 1200.0, 900.0, 750.0, 600.0, 450.0, 300.0)
            for a in np.deg2rad(np.arange(0, 360, 7.5))]
    cand = [(st["n"][1::2] + r * np.cos(a), st["e"][1::2] + r * np.sin(a)) for r, a in grid]
    tadv = [i for i, kind in plan.items() if kind == "tadv"]
    for i in tadv:
        assert st["rl"][2 * i] > st["nw"][2 * i] + 1, (st["rl"][2 * i], st["nw"][2 * i])
    _, ratio = host_flags(np.concatenate([_request_rows(cfg, rest, cn, ce, tadv) for cn, ce in cand]))  # (one call)
    ratio = ratio.reshape(len(grid), N)
    # in open water, well inside the map: the placed ship does not end the episode on the tick by grounding
    ne = np.concatenate([np.stack([cn, ce], 1) for cn, ce in cand])
    inside, shore = O.map_query(cfg, ne)
    water = ((inside == 0) & (shore > 300.0) & (ne[:, 0] > 300.0) & (ne[:, 0] < 9700.0) & (ne[:, 1] > 300.0) &
             (ne[:, 1] < 19700.0)).reshape(len(grid), N)
    todo = dict(plan)
    for i, kind in plan.items():
        ok = np.nonzero((ratio[:, i] > 2.0 if kind == "ref" else ratio[:, i] < 0.5) & water[:, i])[0]
        if len(ok):
            n_t[i], e_t[i] = cand[ok[0]][0][i], cand[ok[0]][1][i]
            del todo[i]
    assert not todo, todo
    st["n"][0::2], st["e"][0::2] = n_t, e_t
    for i in tadv:
        st["rn"][2 * i, st["nw"][2 * i]] = n_t[i] + _WP_OFF[0]
        st["re"][2 * i, st["nw"][2 * i]] = e_t[i] + _WP_OFF[1]
    rows = _request_rows(cfg, st, n_t, e_t)
    flags, ratio = host_flags(rows)
    dist = np.hypot(rows[:, 10] - rows[:, 4], rows[:, 11] - rows[:, 5])
    for i, kind in plan.items():
        assert dist[i] < 1999.0, (i, dist[i])  # a requesting tick
        assert flags[i] == (kind in ("acc", "adv", "tadv")), (i, kind, ratio[i])
        assert ratio[i] > 2.0 if kind == "ref" else ratio[i] < 0.5, (i, kind, ratio[i])
    idle = [i for i in range(N) if i not in plan]
    assert (dist[idle] > 2001.0).all()  # the others do not request on the first tick
    seen.update(nw=st["nw"].copy(), flags=flags, ratio=ratio, dist=dist)
    sim.set(abi.F_NORTH, torch.from_numpy(st["n"]))
    sim.set(abi.F_EAST, torch.from_numpy(st["e"]))
    sim.set(abi.E_SBMPC_P_LAST, torch.from_numpy(st["p_last"]))
    sim.set(abi.E_SBMPC_CHI_LAST, torch.from_numpy(st["chi_last"]))
    if tadv:
        sim.set(abi.E_ROUTE_NORTH, torch.from_numpy(st["rn"]))
        sim.set(abi.E_ROUTE_EAST, torch.from_numpy(st["re"]))


_PLANS = {
    # four envs per wave: (a) all accepted; (b) two accepted, two refused; (c) one refused, three accepted;
    # (d) memory off (1, 0), (e) a request on the tick of a waypoint advance, the obstacle ship's and the test ship's
    # own, and an env that does not request
    (16, 0): {0: "acc", 1: "acc", 2: "acc", 3: "acc", 4: "acc", 5: "ref", 6: "acc", 7: "ref",
              8: "acc", 9: "acc", 10: "ref", 11: "acc", 12: "mem", 13: "adv", 14: "tadv"},
    # three envs per wave, a partial last wave: one refused between two accepted; an accepted one beside an idle one
    (5, 3): {0: "acc", 1: "ref", 2: "acc", 3: "acc"},
    # all accepted; two refused beside one accepted; memory off, the obstacle ship's advance, the test ship's advance
    (9, 3): {0: "acc", 1: "acc", 2: "acc", 3: "ref", 4: "ref", 5: "acc", 6: "mem", 7: "adv", 8: "tadv"},
}


def _compare_first_tick(host_sim, stream_sim, plan, seen):
    for sim in (host_sim, stream_sim):
        nw = _np(sim, abi.F_NEXT_WPT)
        for i, kind in plan.items():
            if kind == "adv":
                assert nw[2 * i + 1] == seen["nw"][2 * i + 1] + 1, nw  # advanced on the requesting tick
            if kind == "tadv":
                assert nw[2 * i] == seen["nw"][2 * i] + 1, nw  # the test ship's own advance on the requesting tick
    for f in (abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST, abi.F_E_CT, abi.F_E_CT_INT):
        np.testing.assert_array_equal(_np(stream_sim, f), _np(host_sim, f))
    np.testing.assert_array_equal(_state(stream_sim), _state(host_sim))
    p, c = _np(stream_sim, abi.E_SBMPC_P_LAST), _np(stream_sim, abi.E_SBMPC_CHI_LAST)
    acc = [i for i, kind in plan.items() if kind in ("acc", "adv", "tadv")]
    assert (p[acc] == 1.0).all() and (c[acc] == 0.0).all() and not np.signbit(c[acc]).any()
    return p, c


@pytest.mark.parametrize("N,epw", sorted(_PLANS))
def test_table_stream_with_placed_requests_equals_host_driven_loop(N, epw):
    cfg = abi.ast_config("sbmpc")
    if epw:
        cfg.envs_per_wave = epw
    plan = _PLANS[(N, epw)]
    table = _table(2, 3, N, seed=61 + N)
    for i, kind in plan.items():
        if kind == "adv":  # a small scoping angle: the jump to the sampled waypoint stays inside the travel tracker's
            table[0, 0, i] = 0.2  # limit of two route segments (it counts the move as travel)
    seen = {}

    def prepare(sim):
        _begin(sim, table)
        _place(cfg, sim, plan, seen)

    host, stream = _Host(cfg, N, table, prepare), _PlacedStream(cfg, N, table, 64, prepare)
    assert stream.sim.lanes_per_env == 16
    host.dticks[:] = _PRE
    host.launch(stream.launch(1))
    assert all(len(host.recs[i]) == 0 and len(stream.recs[i]) == 0 for i in plan)  # the tick ended no decision
    p, c = _compare_first_tick(host.sim, stream.sim, plan, seen)
    print(f"\n[placed N={N}] ratios {np.round(seen['ratio'][sorted(plan)], 3)} -> p_last {p[sorted(plan)]} "
          f"chi_last {np.round(c[sorted(plan)], 4)}")
    for _ in range(2):
        host.launch(stream.launch(150))
    hs, ss = host.records(), stream.records()
    for i in range(N):
        k = len(hs[i])
        assert 1 <= k <= len(ss[i]) <= k + 8, (i, k, len(ss[i]))
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"env {i}")
    same = np.repeat(np.array([len(h) == len(s) for h, s in zip(hs, ss)]), 2)
    assert same.sum() >= 2 * (N - 2), same
    np.testing.assert_array_equal(_state(stream.sim)[same], _state(host.sim)[same])
    for f in (abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST):
        np.testing.assert_array_equal(_np(stream.sim, f)[same[0::2]], _np(host.sim, f)[same[0::2]])
    for f in (abi.F_E_CT, abi.F_E_CT_INT):
        np.testing.assert_array_equal(_np(stream.sim, f)[same], _np(host.sim, f)[same])
    host.sim.close()
    stream.sim.close()


def test_policy_stream_with_placed_requests_equals_host_driven_loop():
    """shipsim_run_policy (MODE 2 of the same kernels), N = 9 at three envs per wave (partial waves), hidden 64,
    deterministic, from the placed state: wave 0 one refused between two accepted (a lone pass), wave 1 two refused
    beside one accepted (a paired pass), wave 2 a memory off (1, 0), the obstacle ship's advance and the test ship's own
    advance on the requesting tick. The actions it logged, replayed decision by decision through the host-driven step
    loop from the same placed state, give its records, final state, memory and LOS integrator."""
    from test_gpu_policy_act import _trainer
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = abi.ast_config("sbmpc")
    cfg.envs_per_wave = 3
    N, n_dec, cap = 9, 3, 64
    plan = {0: "acc", 1: "ref", 2: "acc", 3: "ref", 4: "ref", 5: "acc", 6: "mem", 7: "adv", 8: "tadv"}
    first = _table(1, n_dec, N, seed=67)  # the actions of the decision in progress at the placement
    first[0, 0, 7] = 0.2  # (the obstacle ship's jump to its sampled waypoint stays inside the travel tracker's limit)
    seen = {}

    def prepare(sim):
        _begin(sim, first)
        _place(cfg, sim, plan, seen)

    sim = ShipSim(cfg, N)
    sim.reset()
    prepare(sim)
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    ticks = []
    for T in (1, 150, 150):
        o = sim.run_policy(dp.weights(), T, n_dec, ep, dec, deterministic=True, log=log, log_len=log_len)
        ticks.append(o["ticks"].cpu().numpy())
        if T == 1:
            assert int(log_len.max()) == 0  # the requesting tick ended no decision
            p, c = _np(sim, abi.E_SBMPC_P_LAST), _np(sim, abi.E_SBMPC_CHI_LAST)
            acc = [i for i, kind in plan.items() if kind in ("acc", "adv", "tadv")]
            assert (p[acc] == 1.0).all() and (c[acc] == 0.0).all()
            nw = _np(sim, abi.F_NEXT_WPT)
            assert nw[2 * 7 + 1] == seen["nw"][2 * 7 + 1] + 1 and nw[2 * 8] == seen["nw"][2 * 8] + 1, nw
            first_tick = [_np(sim, f) for f in (abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST, abi.F_E_CT, abi.F_E_CT_INT)]
    ln = log_len.cpu().numpy()
    assert ln.min() >= 1 and ln.max() < cap
    L = log.cpu().numpy()
    recs = [L[i, :ln[i]] for i in range(N)]
    n_eps = int(max(r[:, abi.DL_EPISODE].max() for r in recs)) + 2
    table = np.zeros((n_eps, n_dec, N), np.float32)
    for i in range(N):  # (as test_gpu_stream_reg_consts.py: logged actions, and the row past each env's last record)
        r = recs[i]
        table[r[:, abi.DL_EPISODE].astype(int), r[:, abi.DL_DECISION].astype(int), i] = \
            abi.normalized_to_scoping(r[:, abi.DL_ACTION].astype(np.float32))
        last = r[-1]
        e, d = int(last[abi.DL_EPISODE]), int(last[abi.DL_DECISION]) + 1
        if last[abi.DL_DONE] or d >= n_dec:
            e, d = e + 1, 0
        table[e, d, i] = abi.normalized_to_scoping(np.float32(L[i, ln[i], abi.DL_ACTION]))
    table[0, 0] = first[0, 0]  # the decision the placement happened in was started by the sliced step
    host = _Host(cfg, N, table, prepare)
    host.dticks[:] = _PRE
    for k, t in enumerate(ticks):
        host.launch(t)
        if k == 0:  # after the requesting tick: the memory and both ships' LOS state
            for f, x in zip((abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST, abi.F_E_CT, abi.F_E_CT_INT), first_tick):
                np.testing.assert_array_equal(x, _np(host.sim, f))
    hs = host.records()
    for i in range(N):
        k = len(hs[i])
        assert 1 <= k <= ln[i] <= k + 8, (i, k, ln[i])
        np.testing.assert_array_equal(recs[i][:k][:, _KEEP], hs[i], err_msg=f"policy env {i}")
    same = np.repeat(np.array([len(h) == k for h, k in zip(hs, ln)]), 2)
    assert same.sum() >= 2 * (N - 2), same
    np.testing.assert_array_equal(_state(sim)[same], _state(host.sim)[same])
    for f in (abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST):
        np.testing.assert_array_equal(_np(sim, f)[same[0::2]], _np(host.sim, f)[same[0::2]])
    host.sim.close()
    sim.close()
