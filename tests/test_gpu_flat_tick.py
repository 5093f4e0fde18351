"""The flat tick of the two-slot, 16-lane decision streams (shipsim_run_table / shipsim_run_policy, detailed machinery):
one `going` region per tick, from the SBMPC pass's hand-out to the end of the tick body, with the lane exchanges inside
it, and the decision ladder as selects. The sliced shipsim_step kernels keep the guarded tick and the nested ladder, so
the host-driven step loop (the harness of test_gpu_stream_reg_consts.py) is an independent reference. The cases are
the paths a flattened tick can get wrong: rows of a wave that stop while others go on, the threshold tests' bands, a
frozen ship's lanes beside ticking ones, every rung of the ladder, a poisoned state, a waypoint advance with a cell
change. Every comparison is bit for bit: decision records
(reward, events, done, episode, decision, ticks, observation), per-launch tick counts and the final ship state.
  1. rows that stop beside rows that go on: 5 and 9 envs at 3 envs per wave, the middle env of each wave stopping
     mid-launch (after eight zero-tick decisions in a row: the table stream's stall; its log-capacity stall belongs to
     the policy stream) while its wave neighbours keep ticking; launches ending mid-decision; in-kernel resets;
  2. the sqrt bands: test-to-obstacle distances of exactly 2000.0 m and a few position ulps either side of it (the
     D_INIT test of the SBMPC request), a frozen obstacle ship exactly 200.0 m from its route end and a few ulps either
     side (the reaches-end test);
  3. a frozen obstacle ship, and the travel tracker running into the travel_dist > 2·AB_seg event;
  4. the rungs of the decision ladder, on the all-failing table of test_gpu_contract.py;
  5. a NaN position (EV_NONFINITE), and a waypoint advance in the same tick as a cell change;
  6. the policy stream (MODE 2 of the same kernels) once, at N = 8.
Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim, ShipSimNonFiniteError
from test_gpu_stream_reg_consts import _HostLoop, _KEEP, _state, _table
# 6. the policy stream against the host-driven loop, N = 8, three launches with boundaries mid-decision: the
# comparison of test_gpu_stream_reg_consts.py runs the kernels this file is about, collected here under its own name
from test_gpu_stream_reg_consts import test_policy_stream_equals_host_driven_loop as test_policy_stream_flat_tick  # noqa: F401

pytestmark = pytest.mark.gpu

_EV, _DONE, _EP, _DEC, _TICKS = 1, 2, 3, 4, 5  # columns of _KEEP


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


class _Host(_HostLoop):
    """_HostLoop advanced by a tick count per env (an env of the stream that stalled ran fewer ticks than its
    neighbours): the same loop with the target an array."""

    def __init__(self, cfg, N, table, prepare=None):
        super().__init__(cfg, N, table)
        self.target = np.zeros(N, int)
        if prepare:
            prepare(self.sim)

    def launch(self, ticks):
        self.target = self.target + np.asarray(ticks, int)
        n_eps, n_dec = self.table.shape[:2]
        ar = np.arange(self.N)
        for _ in range(100 * int(np.max(ticks)) + 100):
            left = self.target - self.total
            active = left > 0
            if not active.any():
                return
            a = torch.from_numpy(self.table[self.ep % n_eps, self.dec, ar]).cuda()
            out = self.sim.step(a, active=torch.from_numpy(active.astype(np.uint8)).cuda(),
                                max_ticks=int(left[active].min()))
            o = {k: v.cpu().numpy() for k, v in out.items()}
            ev = o["events"].view(np.uint32)
            t = np.where(active, o["ticks"], 0)
            ready = active & (o["ready"] != 0)
            self.total += t
            self.dticks += t
            for i in np.nonzero(ready)[0]:
                self.recs[i].append(np.concatenate([[o["reward"][i], float(ev[i]), float(o["done"][i]), self.ep[i],
                                                     self.dec[i], self.dticks[i]], o["obs"][i].astype(np.float64)]))
            end = ready & ((o["done"] != 0) | (self.dec + 1 >= n_dec))
            self.dec += ready
            self.dec[end] = 0
            self.ep += end
            self.dticks[ready] = 0
            self.sim.reset(mask=torch.from_numpy(end.astype(np.uint8)).cuda())
        raise AssertionError("host loop did not reach the launch's tick counts")


class _Stream:
    """run_table launches with a decision log of `cap` rows, read and emptied after every launch."""

    def __init__(self, cfg, N, table, cap, prepare=None):
        self.sim = ShipSim(cfg, N)
        self.sim.reset()
        if prepare:
            prepare(self.sim)
        self.N, self.cap = N, cap
        self.table = torch.from_numpy(table).cuda()
        self.ep = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.dec = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.log = torch.zeros((N, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
        self.log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.recs = [[] for _ in range(N)]

    def launch(self, ticks):
        o = self.sim.run_table(self.table, ticks, self.ep, self.dec, log=self.log, log_len=self.log_len)
        ln, L = self.log_len.cpu().numpy(), self.log.cpu().numpy()
        assert ln.max() <= self.cap  # (run_table drops records past the log's end: none here)
        for i in range(self.N):
            self.recs[i].extend(L[i, :ln[i]][:, _KEEP])
        self.count = ln.copy()
        self.log_len.zero_()
        return o["ticks"].cpu().numpy()

    def records(self):
        return [np.array(r).reshape(-1, len(_KEEP)) for r in self.recs]


_PRE = 5  # ticks of _begin


def _begin(sim, table):
    """The first decision started and _PRE ticks in (a sliced step with the table's first actions), so that a test's
    changes to the state are not overwritten by the decision's start (it samples a waypoint and zeroes the travel
    tracker)."""
    sim.step(torch.from_numpy(table[0, 0]).cuda(), max_ticks=_PRE)


def _run(cfg, N, table, launches, T, cap, prepare=None, min_records=1, pre_ticks=0, skip=(), ahead=2):
    """The stream and the host loop side by side: per launch the stream's tick counts drive the host loop. Returns the
    stream's records, per-launch tick counts and record counts after asserting records, tick totals and final state
    equal. pre_ticks: ticks of the decision in progress that `prepare` ran on both (the records count them). skip: envs
    that never tick (every sampling fails: the stream completes a burst of zero-tick decisions per launch, the host
    loop, driven by tick counts, none), left to the caller. ahead: envs that may end with the stream's zero-tick records
    ahead of the host's (their final states are not compared: the stream has reset them)."""
    host, stream = _Host(cfg, N, table, prepare), _Stream(cfg, N, table, cap, prepare)
    host.dticks[:] = pre_ticks
    assert stream.sim.lanes_per_env == 16
    ticks, full = [], []
    for _ in range(launches):
        t = stream.launch(T)
        assert (t <= T).all()
        host.launch(t)
        ticks.append(t)
        full.append(stream.count)
    hs, ss = host.records(), stream.records()
    cmp = np.array([i not in skip for i in range(N)])
    for i in np.nonzero(cmp)[0]:
        # a decision that completed on the launch's last tick and failed its next sampling at once is ahead in the
        # stream by those zero-tick records (it starts the next decision inside the launch): the host's are a prefix
        k = len(hs[i])
        assert min_records <= k <= len(ss[i]) <= k + 8, (i, k, len(ss[i]))
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"env {i}")
        assert (ss[i][k:, _TICKS] == 0).all()
    same = np.array([len(h) == len(s) for h, s in zip(hs, ss)]) & cmp
    assert same.sum() >= cmp.sum() - ahead, same
    rows = np.repeat(same, 2)  # two ships per env
    np.testing.assert_array_equal(_state(stream.sim)[rows], _state(host.sim)[rows], err_msg="final ship state")
    np.testing.assert_array_equal(host.total, np.sum(ticks, 0))
    host.sim.close()
    stream.sim.close()
    return ss, np.array(ticks), np.array(full)


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
@pytest.mark.parametrize("N", [5, 9])
def test_rows_that_stop_beside_rows_that_go_on(collav, N):
    """3 envs per wave. The middle env of every wave runs one good decision and then only samplings that fail (its
    second decision, and the first of the nine following table episodes): after eight such zero-tick decisions in a
    row the env stops for the launch, about 100 ticks in, while its wave neighbours tick on to the launch's end; the
    next launch takes it up again. The launches of 200 ticks end inside the other envs' decisions (77 .. 131 ticks
    each)."""
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 3
    T, launches = 200, 8
    table = _table(10, 3, N, seed=47 + N)
    burst = np.arange(N) % 3 == 1
    table[0, 1, burst] = 1.5  # tan(1.5) * AB_seg: the intermediate waypoint leaves the map
    table[1:, 0, burst] = 1.5
    ss, ticks, count = _run(cfg, N, table, launches, T, cap=64, ahead=2 + int(burst.sum()))
    assert sum(len(r) for r in ss) >= 3 * N
    assert max(r[:, _EP].max() for r in ss) >= 1  # episodes were reset inside the kernel
    wave = np.arange(N) // 3
    mixed = [(0 < ticks[l][wave == w]).all() and (ticks[l][wave == w] < T).any() and (ticks[l][wave == w] == T).any()
             for l in range(launches) for w in range(wave.max() + 1) if (wave == w).sum() > 1]
    assert any(mixed)  # an env stopped mid-launch in a wave whose other envs ran the launch out
    assert (ticks[:, ~burst] == T).all()
    ends = [np.cumsum(ss[i][:, _TICKS]) for i in np.nonzero(~burst)[0]]  # the ticks at which an env's decisions ended
    assert any(T * l not in c for c in ends for l in range(1, launches))  # launch boundaries inside decisions


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_sqrt_bands(collav):
    """Envs 0..4: the obstacle ship 2000 m from the test ship (1200 m east, 1600 m north) with the east offset moved by
    -2, -1, 0, 1, 2 ulps of the position: d² lands inside the relative 1e-12 band around 2000², on both sides of it and
    on it. Envs 5..7: the obstacle ship frozen (120, 160) m from its route end, the offset moved by -1, 0, 1 ulps:
    exactly 200.0 m, and the band either side; their travel tracker is past its limit, so the next tick completes the
    decision and its record shows that tick's event bits."""
    cfg = abi.ast_config(collav)
    N = 8
    seen = {}

    table = _table(2, 3, N, seed=3)

    def prepare(sim):
        _begin(sim, table)
        n, e = sim.get(abi.F_NORTH).cpu().numpy(), sim.get(abi.F_EAST).cpu().numpy()
        stop = sim.get(abi.F_STOP).cpu().numpy()
        td = sim.get(abi.E_TRAVEL_DIST).cpu().numpy()
        td[5:] = 1e9  # (past 2·AB_seg: the next tick ends the decision, its event bits in the record)
        rn, re = sim.get(abi.E_ROUTE_NORTH).cpu().numpy(), sim.get(abi.E_ROUTE_EAST).cpu().numpy()
        rl = sim.get(abi.E_ROUTE_LEN).cpu().numpy()
        d2, e2 = [], []
        for i, k in enumerate((-2, -1, 0, 1, 2)):
            t, o = 2 * i, 2 * i + 1
            n[t], e[t] = np.round(n[t]), np.round(e[t])  # whole metres: the offsets below are exact
            n[o], e[o] = n[t] + 1600.0, _ulps(e[t] + 1200.0, k)
            d2.append((e[o] - e[t]) * (e[o] - e[t]) + (n[o] - n[t]) * (n[o] - n[t]))
        for i, k in zip((5, 6, 7), (-1, 0, 1)):
            o = 2 * i + 1
            en, ee = rn[o, rl[o] - 1], re[o, rl[o] - 1]
            n[o], e[o] = en - 160.0, _ulps(ee - 120.0, k)
            stop[o] = 1
            e2.append((n[o] - en) * (n[o] - en) + (e[o] - ee) * (e[o] - ee))
        seen["d2"], seen["e2"] = np.array(d2), np.array(e2)
        sim.set(abi.F_NORTH, torch.from_numpy(n))
        sim.set(abi.F_EAST, torch.from_numpy(e))
        sim.set(abi.F_STOP, torch.from_numpy(stop))
        sim.set(abi.E_TRAVEL_DIST, torch.from_numpy(td))

    ss, _, _ = _run(cfg, N, table, launches=2, T=120, cap=64, prepare=prepare, min_records=0, pre_ticks=_PRE)
    d2, e2 = seen["d2"], seen["e2"]
    # the placements are what the docstring says: inside the band, the sqrt deciding both ways, and exact hits
    assert (np.abs(d2 - 4e6) <= 4e6 * 1e-12).all() and d2[2] == 4e6 and d2.min() < 4e6 < d2.max()
    assert (np.sqrt(d2) < 2000.0).any() and not (np.sqrt(d2) < 2000.0).all()
    assert (np.abs(e2 - 4e4) <= 4e4 * 1e-12).all() and e2[1] == 4e4 and e2.min() < 4e4 < e2.max()
    for i, a in zip((5, 6, 7), e2):  # the first tick's event bits: reaches-end exactly when sqrt(a) <= 200
        assert len(ss[i]) >= 1 and ss[i][0, _TICKS] == _PRE + 1
        assert bool(int(ss[i][0, _EV]) & abi.EV_OBS_REACHES_END) == bool(np.sqrt(a) <= 200.0)


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_frozen_obstacle_ship_and_travel_event(collav):
    """Envs 0..3: the obstacle ship frozen from the start (its lanes take the frozen branch beside ticking test-ship
    lanes). Envs 4..7: the travel tracker a few ticks short of 2·AB_seg, so the obstacle ship's navigation failure
    fires from travel_dist; its event bits are compared like every record's."""
    cfg = abi.ast_config(collav)
    N = 8

    table = _table(2, 3, N, seed=11)

    def prepare(sim):
        _begin(sim, table)
        stop = sim.get(abi.F_STOP).cpu().numpy()
        stop[1:8:2] = 1
        sim.set(abi.F_STOP, torch.from_numpy(stop))

    probe = ShipSim(cfg, N)  # AB_seg: the obstacle ship's configured route over max_sampling_frequency + 1 segments
    probe.reset()
    rn, re = probe.get(abi.E_ROUTE_NORTH).cpu().numpy(), probe.get(abi.E_ROUTE_EAST).cpu().numpy()
    rl = probe.get(abi.E_ROUTE_LEN).cpu().numpy()
    probe.close()
    ab = np.hypot(rn[1, rl[1] - 1] - rn[1, 0], re[1, rl[1] - 1] - re[1, 0]) / (cfg.max_sampling_frequency + 1)

    def prepare_both(sim):
        prepare(sim)
        td = sim.get(abi.E_TRAVEL_DIST).cpu().numpy()
        td[4:] = 2 * ab - 60.0 - 10.0 * np.arange(4)
        sim.set(abi.E_TRAVEL_DIST, torch.from_numpy(td))

    ss, _, _ = _run(cfg, N, table, launches=2, T=150, cap=64, prepare=prepare_both, min_records=0, pre_ticks=_PRE)
    for i in range(4, 8):  # 60 .. 90 m short at about 14 m per tick: the obstacle ship's navigation failure, ticks later
        first = ss[i][0]
        assert int(first[_EV]) & abi.EV_OBS_NAV_FAILURE and first[_DONE] == 1, first[:6]
        assert _PRE + 2 <= first[_TICKS] <= _PRE + 20, first[:6]
    assert len({ss[i][0, _TICKS] for i in range(4, 8)}) > 1  # (the event came from the tracker's sum, not at once)


def test_decision_ladder_rungs():
    """The table of test_gpu_contract.py's all-failing case (every third env's samplings leave the map; nine decisions
    per episode). Each rung, reached and shown by the records:
      * done in phase 0: env 0's travel tracker is set past its limit inside the first decision, before any radius of
        acceptance: the next tick ends the decision, done;
      * phase 1 with waypoints left to sample: every ordinary decision (radius of acceptance plus one tick, not done);
      * phase 1 at max_sampling, then phase 2: env 2's sampling count is set to the maximum inside the first decision:
        at its radius of acceptance the decision does not finish but runs on, until done;
      * no intermediate waypoint left: env 3's sampling count is at the maximum before the first decision starts and
        its obstacle ship 1000 m short of its route's end, so no waypoint is sampled and phase 0 finishes at the radius
        of acceptance of the route's end, not done; its following decisions finish on their first tick, to the ninth;
      * nine decisions: an episode's ninth decision is followed by the next episode's first."""
    cfg = abi.ast_config("sbmpc")
    N, n_dec = 12, cfg.max_sampling_frequency
    assert n_dec == 9
    g = np.random.Generator(np.random.PCG64(7))
    tab = abi.normalized_to_scoping(g.uniform(-1, 1, (2, n_dec, N)).astype(np.float32))
    failing = np.arange(N) % 3 == 1
    tab[:, :, failing] = 1.5  # tan(1.5) * AB_seg: the intermediate waypoint leaves the map

    def prepare(sim):
        sc = sim.get(abi.E_SAMPLING_COUNT).cpu().numpy()
        sc[3] = n_dec
        sim.set(abi.E_SAMPLING_COUNT, torch.from_numpy(sc))
        n, e = sim.get(abi.F_NORTH).cpu().numpy(), sim.get(abi.F_EAST).cpu().numpy()
        rn, re = sim.get(abi.E_ROUTE_NORTH).cpu().numpy(), sim.get(abi.E_ROUTE_EAST).cpu().numpy()
        rl = sim.get(abi.E_ROUTE_LEN).cpu().numpy()
        o = 2 * 3 + 1
        dn, de = rn[o, 0] - rn[o, rl[o] - 1], re[o, 0] - re[o, rl[o] - 1]
        n[o] = rn[o, rl[o] - 1] + 1000.0 * dn / np.hypot(dn, de)
        e[o] = re[o, rl[o] - 1] + 1000.0 * de / np.hypot(dn, de)
        sim.set(abi.F_NORTH, torch.from_numpy(n))
        sim.set(abi.F_EAST, torch.from_numpy(e))
        td = sim.get(abi.E_TRAVEL_DIST).cpu().numpy()
        td[3] = -1e6  # (the tracker counts the move above as travel, and no sampling resets it: far below its limit)
        sim.set(abi.E_TRAVEL_DIST, torch.from_numpy(td))
        _begin(sim, tab)
        sc = sim.get(abi.E_SAMPLING_COUNT).cpu().numpy()
        sc[2] = n_dec
        sim.set(abi.E_SAMPLING_COUNT, torch.from_numpy(sc))
        td = sim.get(abi.E_TRAVEL_DIST).cpu().numpy()
        td[0] = 1e9
        sim.set(abi.E_TRAVEL_DIST, torch.from_numpy(td))

    ss, _, _ = _run(cfg, N, tab, launches=7, T=700, cap=64, prepare=prepare, pre_ticks=_PRE,
                    skip=set(np.nonzero(failing)[0]))
    first = ss[0][0]  # done in phase 0
    assert first[_DONE] == 1 and first[_TICKS] == _PRE + 1 and int(first[_EV]) & abi.EV_OBS_NAV_FAILURE, first[:6]
    ordinary = np.concatenate([ss[i] for i in (5, 6, 8, 9, 11)])  # phase 1, waypoints left
    assert ((ordinary[:, _DONE] == 0) & (ordinary[:, _TICKS] > 50) & (ordinary[:, _DEC] < n_dec - 1)).any()
    longest = ordinary[ordinary[:, _DEC] < n_dec - 1][:, _TICKS].max()
    first = ss[2][0]  # phase 1 at max_sampling, on through phase 2 until done
    assert first[_DEC] == 0 and first[_DONE] == 1 and first[_TICKS] > 2 * longest, (first[:6], longest)
    r = ss[3]  # no intermediate waypoint left
    assert r[0, _DONE] == 0 and 20 < r[0, _TICKS] < longest and not int(r[0, _EV]) & abi.EV_SAMPLING_FAILURE, r[0, :6]
    assert len(r) >= n_dec and (r[1:n_dec, _TICKS] == 1).all() and (r[1:n_dec, _DONE] == 0).all(), r[:n_dec, :6]
    assert r[n_dec - 1, _DEC] == n_dec - 1 and r[n_dec, _DEC] == 0 and r[n_dec, _EP] == r[n_dec - 1, _EP] + 1
    nine = [x for x in ss if ((x[:-1, _DEC] == n_dec - 1) & (x[1:, _DEC] == 0) & (x[1:, _EP] == x[:-1, _EP] + 1)).any()]
    assert nine  # nine decisions
    for i in np.nonzero(failing)[0]:
        assert len(ss[i]) == 8 * 7  # a burst of 8 zero-tick decisions per launch
        assert (ss[i][:, _EV].astype(np.int64) & abi.EV_SAMPLING_FAILURE).all() and (ss[i][:, _TICKS] == 0).all()


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_nonfinite_position_and_waypoint_advance_with_cell_change(collav):
    """Env 2: the test ship's north position NaN: its decision completes on the first tick with EV_NONFINITE. Envs 4..7:
    the obstacle ship placed on its next waypoint with a further one behind it, so the launch's first tick advances the
    waypoint index in the tick that also fetches a new grid cell (every ship's first tick of a launch does)."""
    cfg = abi.ast_config(collav)
    N = 8
    table = _table(2, 3, N, seed=23)
    seen = {}

    def prepare(sim):  # one decision in, so that the obstacle ship's route holds an intermediate waypoint
        _begin(sim, table)
        n, e = sim.get(abi.F_NORTH).cpu().numpy(), sim.get(abi.F_EAST).cpu().numpy()
        rn, re = sim.get(abi.E_ROUTE_NORTH).cpu().numpy(), sim.get(abi.E_ROUTE_EAST).cpu().numpy()
        rl, nw = sim.get(abi.E_ROUTE_LEN).cpu().numpy(), sim.get(abi.F_NEXT_WPT).cpu().numpy()
        for i in range(4, 8):
            o = 2 * i + 1
            assert rl[o] > nw[o] + 1, (rl[o], nw[o])
            n[o], e[o] = rn[o, nw[o]] + 3.0, re[o, nw[o]] - 2.0
        n[2 * 2] = np.nan
        seen["nw"] = nw.copy()
        sim.set(abi.F_NORTH, torch.from_numpy(n))
        sim.set(abi.F_EAST, torch.from_numpy(e))

    host, stream = _Host(cfg, N, table, prepare), _Stream(cfg, N, table, 64, prepare)
    # (both sims took the prepare step: the host loop's bookkeeping starts from that state, five ticks into decision 0)
    host.dticks[:] = _PRE
    stream_t = stream.launch(1)
    host.launch(stream_t)
    for sim in (host.sim, stream.sim):
        nw = sim.get(abi.F_NEXT_WPT).cpu().numpy()
        assert (nw[9:16:2] == seen["nw"][9:16:2] + 1).all(), nw  # advanced in that tick
    for _ in range(2):
        host.launch(stream.launch(150))
    hs, ss = host.records(), stream.records()
    bad = ss[2][0]
    assert int(bad[_EV]) & abi.EV_NONFINITE and int(bad[_EV]) & abi.EV_TERMINAL and bad[_DONE] == 1
    for i in range(N):
        k = len(hs[i])
        assert 1 <= k <= len(ss[i]) <= k + 8
        # (the stream counts a decision's ticks from the state's own counter, which the prepare step left at 5 too)
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"env {i}")
    same = np.repeat(np.array([len(h) == len(s) for h, s in zip(hs, ss)]), 2)
    np.testing.assert_array_equal(_state(stream.sim)[same], _state(host.sim)[same])
    for sim in (host.sim, stream.sim):
        with pytest.raises(ShipSimNonFiniteError):
            sim.synchronize()
        sim.close()
