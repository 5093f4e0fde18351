"""The tick loop of the chained ast_step_kernel instantiations (shipsim_run_table, shipsim_run_policy) is tested at its
bottom: a guard, then the tick, then the same condition again (shipsim_kernels.hip, TICK_LOOP_ON, TICK_ROT), inside
the kernels' for (;;) with the chaining code behind it; shipsim_step's kernels keep the test at the top. The cases
are the edges such a loop can get wrong, each bit for bit against the host-driven step loop (_HostLoop of
tests/test_gpu_stream_reg_consts.py, per-env tick counts as in tests/test_gpu_flat_tick.py): decision records
(reward, events, done, episode, decision, ticks, observation), per-launch tick counts and the final ship state.
  1. launches of 1 and of 2 ticks, N = 5 at three envs per wave: the body runs exactly once, and twice;
  2. a launch boundary one tick before a decision of env 0 completes: the next launch leaves the loop for the
     chaining code at its first latch test and enters it again through the guard;
  3. a launch that ends on the very tick a decision completes: both halves of the condition end the loop at once;
  4. a wave whose envs all stall before their first tick (every sampling fails: eight zero-tick decisions, then the
     env stops for the launch): the guard is false and the body never runs, beside a wave that ticks;
     and the policy stream's own stall, a launch entered with every env's log full;
  5. the policy stream at N = 8, launches of 1, 2 and 700 ticks;
  6. a K = 2 table stream at N = 3;
  7. shipsim_step with max_ticks = 1: the unchained kernels' loop (one spelling with the streams'), left by its break
     after one tick.
Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim
from test_gpu_flat_tick import _Host, _Stream
from test_gpu_stream_reg_consts import _KEEP, _state, _table

pytestmark = pytest.mark.gpu

_EV, _DONE, _EP, _DEC, _TICKS = 1, 2, 3, 4, 5  # columns of _KEEP


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _run(cfg, N, table, schedule, cap=64, skip=(), min_records=1, expect_full=True):
    """The stream over the launches of `schedule` (ticks each), the host loop driven by the stream's tick counts.
    Returns the stream's records and the per-launch tick counts after asserting records and final state equal."""
    host, stream = _Host(cfg, N, table), _Stream(cfg, N, table, cap)
    ticks = []
    keep = np.array([i not in skip for i in range(N)])
    for T in schedule:
        t = stream.launch(T)
        if expect_full:
            np.testing.assert_array_equal(t[keep], np.full(keep.sum(), T))
        host.launch(np.where(keep, t, 0))
        ticks.append(t)
    hs, ss = host.records(), stream.records()
    n_ships = len(_state(host.sim)) // N
    for i in np.nonzero(keep)[0]:
        # (a decision that completed on a launch's last tick and failed its next sampling at once is ahead in the
        # stream by those zero-tick records: the host's are a prefix)
        k = len(hs[i])
        assert min_records <= k <= len(ss[i]) <= k + 8, (i, k, len(ss[i]))
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"env {i}")
        assert (ss[i][k:, _TICKS] == 0).all()
    same = np.array([len(h) == len(s) for h, s in zip(hs, ss)]) & keep
    assert same.sum() >= keep.sum() - 1, same
    rows = np.repeat(same, n_ships)
    np.testing.assert_array_equal(_state(stream.sim)[rows], _state(host.sim)[rows], err_msg="final ship state")
    np.testing.assert_array_equal(host.total[keep], np.sum(ticks, 0)[keep])
    host.sim.close()
    stream.sim.close()
    return ss, np.array(ticks)


def _cfg3(collav, **kw):
    cfg = abi.ast_config(collav, **kw)
    cfg.envs_per_wave = 3
    return cfg


@pytest.fixture(scope="module")
def first_decisions():
    """Ticks at which the first two decisions of every env of the N = 5 sbmpc stream end (one probe run, shared)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    N = 5
    table = _table(4, 3, N, seed=71)
    s = _Stream(_cfg3("sbmpc"), N, table, 64)
    s.launch(700)
    ends = [np.cumsum(r[:, _TICKS]).astype(int) for r in s.records()]
    s.sim.close()
    assert all(len(e) >= 2 and e[0] > 2 for e in ends), ends
    return table, ends


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
@pytest.mark.parametrize("slice_ticks", [1, 2])
def test_body_runs_once_and_twice(collav, slice_ticks):
    """Launches of one tick and of two between ordinary ones: every env reports exactly that many ticks, and the
    records and the state go on as the host loop's."""
    N = 5
    table = _table(4, 3, N, seed=61 + slice_ticks)
    ss, ticks = _run(_cfg3(collav), N, table, [slice_ticks] * 3 + [300] + [slice_ticks] * 3 + [300, slice_ticks])
    assert (ticks[:3] == slice_ticks).all() and (ticks[-1] == slice_ticks).all()
    assert sum(len(r) for r in ss) >= 3 * N


def test_decision_completes_on_first_tick_of_a_launch(first_decisions):
    """Env 0's first decision ends on tick e: a launch of e - 1 ticks, then one whose first tick completes it (the
    loop is left at its first latch test, the chaining code starts the next decision, the guard lets the loop in
    again), the same for its second decision; the wave's other envs are mid-decision at both."""
    table, ends = first_decisions
    e0, e1 = ends[0][0], ends[0][1]
    assert all(e0 not in e[:3] and e1 not in e[:3] for e in ends[1:3]), ends  # (wave-mates: envs 1, 2)
    ss, _ = _run(_cfg3("sbmpc"), 5, table, [e0 - 1, e1 - e0, 700 - e1 + 1])
    assert ss[0][0, _TICKS] == e0 and ss[0][1, _TICKS] == e1 - e0
    # the same boundary as a one-tick launch: loop entered, decision completes, chaining, quota met
    _run(_cfg3("sbmpc"), 5, table, [e0 - 1, 1, 1, 700 - e0 - 1])


def test_decision_completes_on_last_tick_of_a_launch(first_decisions):
    """A launch of exactly e ticks: on its last tick env 0's decision completes and its quota is met."""
    table, ends = first_decisions
    e0, e1 = ends[0][0], ends[0][1]
    ss, ticks = _run(_cfg3("sbmpc"), 5, table, [e0, e1 - e0, 700 - e1])
    assert ss[0][0, _TICKS] == e0 and ss[0][1, _TICKS] == e1 - e0
    assert (ticks[0] == e0).all()  # (the wave-mates' quota is met on that tick as well: no lane is going)


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_wave_that_stalls_before_its_first_tick(collav):
    """Envs 0..2 (wave 0): every sampling fails, so each launch completes eight zero-tick decisions at its entry and
    the envs stop for the launch: the wave's guard is false, no tick runs. Envs 3, 4 (wave 1) tick on as ever."""
    N, launches = 5, 3
    table = _table(4, 3, N, seed=83)
    table[:, :, :3] = 1.5  # tan(1.5) * AB_seg: the intermediate waypoint leaves the map
    ss, ticks = _run(_cfg3(collav), N, table, [1, 2, 300], skip={0, 1, 2})
    assert (ticks[:, :3] == 0).all() and (ticks[:, 3:] == np.array([[1], [2], [300]])).all()
    for i in range(3):
        assert len(ss[i]) == 8 * launches and (ss[i][:, _TICKS] == 0).all()
        assert (ss[i][:, _EV].astype(np.int64) & abi.EV_SAMPLING_FAILURE).all()


def test_policy_stream_short_launches_and_full_log_stall():
    """shipsim_run_policy, N = 8, hidden 64, deterministic: launches of 1, 2 and 700 ticks, and one launch that every
    env enters with its log full (the policy stream's stall: no env runs, nothing changes). The logged actions
    replayed through the host-driven step loop give the stream's records and final state."""
    from test_gpu_policy_act import _trainer
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = abi.ast_config("sbmpc")
    N, N_DEC, CAP = 8, 3, 256
    sim = ShipSim(cfg, N)
    sim.reset()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    full_log = torch.zeros((N, 1, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    full_len = torch.ones(N, dtype=torch.int32, device="cuda")
    schedule = [1, 2, 700, 1, 2, 700, 700]
    for k, T in enumerate(schedule):
        o = sim.run_policy(dp.weights(), T, N_DEC, ep, dec, deterministic=True, log=log, log_len=log_len)
        np.testing.assert_array_equal(o["ticks"].cpu().numpy(), np.full(N, T))
        if k == 3:  # every env's log full: the launch is sat out
            before = (_state(sim), ep.clone(), dec.clone())
            o = sim.run_policy(dp.weights(), 50, N_DEC, ep, dec, deterministic=True, log=full_log, log_len=full_len)
            np.testing.assert_array_equal(o["ticks"].cpu().numpy(), np.zeros(N, int))
            np.testing.assert_array_equal(_state(sim), before[0])
            assert torch.equal(ep, before[1]) and torch.equal(dec, before[2])
            assert (full_len == 1).all() and (full_log == 0).all()
    ln = log_len.cpu().numpy()
    assert ln.min() >= 3 and ln.max() < CAP
    L = log.cpu().numpy()
    recs = [L[i, :ln[i]] for i in range(N)]
    n_eps = int(max(r[:, abi.DL_EPISODE].max() for r in recs)) + 2
    # the action of every decision the stream started: the logged ones, and the row past each env's last record
    # (a decision still running at the end has its action in its record row already)
    table = np.zeros((n_eps, N_DEC, N), np.float32)
    for i in range(N):
        r = recs[i]
        table[r[:, abi.DL_EPISODE].astype(int), r[:, abi.DL_DECISION].astype(int), i] = \
            abi.normalized_to_scoping(r[:, abi.DL_ACTION].astype(np.float32))
        last = r[-1]
        e, d = int(last[abi.DL_EPISODE]), int(last[abi.DL_DECISION]) + 1
        if last[abi.DL_DONE] or d >= N_DEC:
            e, d = e + 1, 0
        table[e, d, i] = abi.normalized_to_scoping(np.float32(L[i, ln[i], abi.DL_ACTION]))
    host = _Host(cfg, N, table)
    for T in schedule:
        host.launch(np.full(N, T))
    hs = host.records()
    for i in range(N):
        k = len(hs[i])
        assert 3 <= k <= ln[i] <= k + 8, (i, k, ln[i])
        np.testing.assert_array_equal(recs[i][:k][:, _KEEP], hs[i], err_msg=f"policy env {i}")
    same = np.repeat(np.array([len(h) == n for h, n in zip(hs, ln)]), 2)
    assert same.sum() >= 2 * (N - 1)
    np.testing.assert_array_equal(_state(sim)[same], _state(host.sim)[same], err_msg="policy final ship state")
    host.sim.close()
    sim.close()


def test_two_obstacle_table_stream():
    """K = 2 (three ships per env, the slot kernels) at N = 3: launches of 1, 2 and 400 ticks."""
    cfg = abi.ast_config("sbmpc", n_obs_ships=2)
    N = 3
    table = _table(4, 3, N, seed=97)
    ss, ticks = _run(cfg, N, table, [1, 2, 400, 1, 400])
    assert sum(len(r) for r in ss) >= N


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_step_one_tick_at_a_time(collav):
    """shipsim_step with max_ticks = 1 (the unchained kernel: one pass of the body, then its break) 40 times, against
    the same handle configuration stepped once with max_ticks = 40: ticks, readiness, outputs and state; and the
    decision both then finish against the table stream's first record."""
    N = 5
    cfg = _cfg3(collav)
    a = torch.from_numpy(_table(1, 1, N, seed=5)[0, 0]).cuda()
    one, many = ShipSim(cfg, N), ShipSim(cfg, N)
    for s in (one, many):
        s.reset()
    ref = {k: v.cpu().numpy() for k, v in many.step(a, max_ticks=40).items()}
    assert (ref["ticks"] == 40).all() and (ref["ready"] == 0).all()  # (a decision takes longer than 40 ticks)
    for _ in range(40):
        out = {k: v.cpu().numpy() for k, v in one.step(a, max_ticks=1).items()}
        assert (out["ticks"] == 1).all() and (out["ready"] == 0).all()
    np.testing.assert_array_equal(_state(one), _state(many))
    for s in (one, many):  # both run on to the decision's end: the same record
        s_out = {k: v.cpu().numpy() for k, v in s.step(a).items()}
        if s is one:
            first = s_out
    for k in ("obs", "reward", "done", "events", "ticks", "ready"):
        np.testing.assert_array_equal(first[k], s_out[k], err_msg=k)
    assert (s_out["ready"] != 0).all()
    np.testing.assert_array_equal(_state(one), _state(many))
    stream = _Stream(cfg, N, a.cpu().numpy().reshape(1, 1, N), 64)
    stream.launch(700)
    for i, r in enumerate(stream.records()):
        mine = np.concatenate([[first["reward"][i], float(first["events"].view(np.uint32)[i]), float(first["done"][i]),
                                0, 0, 40 + first["ticks"][i]], first["obs"][i].astype(np.float64)])
        np.testing.assert_array_equal(r[0], mine, err_msg=f"env {i}")
    stream.sim.close()
    one.close()
    many.close()
