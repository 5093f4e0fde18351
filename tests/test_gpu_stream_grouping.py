"""Grouping of the decision streams' envs into waves by episode phase (shipsim_set_stream_grouping): each stream
launch orders the envs by ticks since their last reset and slot s of the launch runs env slot_env[s]. An env's
results do not depend on its wave-mates, so every decision record, counter and state field must be bitwise what the
same stream gives with grouping off (slot = env), and the permutation the launch used must be the stable sort of the
keys. lanes_per_env = 16 throughout, so a wave holds four envs. Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim

pytestmark = pytest.mark.gpu

_FIELDS = list(range(abi.N_SHIP_FIELDS)) + list(range(abi.E_SAMPLING_COUNT, abi.E_ROUTE_EAST + 1))
_MAX_KEY = 1 << 30  # grouping_host::kMaxKey


def _cfg(collav="sbmpc", n_obs=1):
    cfg = abi.ast_config(collav, n_obs_ships=n_obs)
    cfg.lanes_per_env = 16
    return cfg


def _table(n_dec, N, n_eps=3, seed=20251015):
    g = np.random.Generator(np.random.PCG64(seed))
    a = g.uniform(-1, 1, (n_eps, n_dec, N)).astype(np.float32)
    return torch.from_numpy(abi.normalized_to_scoping(a)).cuda()


def _keys(sim):
    """grouping_host::key_of of every env, from the state as it is now: the test ship's clock over the time step."""
    t = sim.get(abi.F_TIME).cpu().numpy().reshape(sim.n_envs, sim.n_ships)[:, 0]
    q = np.rint(t / float(sim.cfg.time_step))
    return np.where(q > 0, np.minimum(q, _MAX_KEY), 0).astype(np.int64)


def _stream(cfg, N, launch, n_calls, grouping, n_obs=0, cap=256, tail=0, reset_mask=None, weather=None):
    """n_calls stream launches on a fresh handle with grouping on or off: per-env decision records, per-launch
    ticks / decisions, the final state, and (grouping on) each launch's permutation beside the keys it sorted."""
    sim = ShipSim(cfg, N, n_obs_ships=n_obs)
    assert sim.lanes_per_env == 16
    if weather is not None:
        sim.set_weather(*weather)
    if tail:
        sim.set_stream_tail(tail)
    assert np.array_equal(sim.get_stream_grouping().cpu().numpy(), np.arange(N))  # the identity from create
    sim.set_stream_grouping(grouping)
    sim.reset(mask=reset_mask)
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    ticks, decisions, perms, keys = [], [], [], []
    for c in range(n_calls):
        keys.append(_keys(sim))
        o = launch(sim, c, ep, dec, log, log_len)
        ticks.append(o["ticks"].cpu().numpy().copy())
        decisions.append(o["decisions"].cpu().numpy().copy())
        perms.append(sim.get_stream_grouping().cpu().numpy().copy())
    sim.synchronize()
    ln = log_len.cpu().numpy()
    assert ln.max() <= cap
    L = log.cpu().numpy()
    state = {f: sim.get(f).cpu().numpy() for f in _FIELDS}
    sim.close()
    return dict(recs=[L[i, :ln[i]] for i in range(N)], ticks=ticks, decisions=decisions, state=state, perms=perms,
                keys=keys, ep=ep.cpu().numpy(), dec=dec.cpu().numpy())


def _check_perms(run, N):
    """Every launch's slot_env is a permutation of range(N), ascending in the key, ties by env index."""
    for key, perm in zip(run["keys"], run["perms"]):
        assert np.array_equal(np.sort(perm), np.arange(N))
        np.testing.assert_array_equal(perm, np.argsort(key, kind="stable"))


def _same(on, off, N, tail=False):
    assert sum(len(r) for r in off["recs"]) > 0
    if not tail:
        for a, b in zip(on["ticks"] + on["decisions"], off["ticks"] + off["decisions"]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(on["ep"], off["ep"])
        np.testing.assert_array_equal(on["dec"], off["dec"])
        for f in _FIELDS:
            assert on["state"][f].tobytes() == off["state"][f].tobytes(), f"state field {f}"
        for i in range(N):
            assert on["recs"][i].tobytes() == off["recs"][i].tobytes(), f"env {i}"
    for run in (off,):
        for perm in run["perms"]:
            assert np.array_equal(perm, np.arange(N))  # grouping off: slot = env


def _run_table(table, T):
    return lambda sim, c, ep, dec, log, ln: sim.run_table(table, T, ep, dec, log=log, log_len=ln)


@pytest.mark.parametrize("N,masked", [(64, False), (61, False), (61, True)])
def test_table_stream_bitwise_with_grouping(N, masked):
    """collav sbmpc, detailed machinery, 8 launches of 512 ticks with in-kernel resets: episodes end at different
    ticks, so the envs' phases diverge and the launches after the second run a permutation other than the identity.
    61 envs leave the last wave partly filled; `masked` drops every fifth env (never reset, so the stream leaves it
    alone: the decision streams take no active mask of their own)."""
    cfg = _cfg()
    table = _table(cfg.max_sampling_frequency, N)
    mask = None
    if masked:
        mask = torch.from_numpy((np.arange(N) % 5 != 2).astype(np.uint8))
    on = _stream(cfg, N, _run_table(table, 512), 8, True, reset_mask=mask)
    off = _stream(cfg, N, _run_table(table, 512), 8, False, reset_mask=mask)
    _check_perms(on, N)
    if not masked:  # from a synchronised reset every key is equal (masked: the envs never reset sort first)
        assert np.array_equal(on["perms"][0], np.arange(N))
    assert any(not np.array_equal(p, np.arange(N)) for p in on["perms"][2:])
    _same(on, off, N)
    if masked:
        dropped = np.arange(N) % 5 == 2
        assert all(len(on["recs"][i]) == 0 for i in np.nonzero(dropped)[0])
        assert all(int(t[dropped].sum()) == 0 for t in on["ticks"])
    for i in range(N):  # every running env went through an in-kernel reset
        if not (masked and i % 5 == 2):
            assert on["recs"][i][-1, abi.DL_EPISODE] >= 1, i


@pytest.mark.parametrize("collav,n_obs,want", [("sbmpc", 1, True), ("none", 1, False), ("sbmpc", 2, False)])
def test_switch_as_create_leaves_it(collav, n_obs, want):
    """On for two-ship envs with collav sbmpc, off otherwise (grouping_host::default_on): after two launches from
    handles nobody switched, only the first kind ran anything but slot = env."""
    N, cfg = 32, _cfg(collav, n_obs)
    table = _table(cfg.max_sampling_frequency, N, seed=17)
    sim = ShipSim(cfg, N, n_obs_ships=n_obs if n_obs > 1 else 0)
    sim.reset()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    moved = False
    for _ in range(3):
        sim.run_table(table, 700, ep, dec)
        moved |= not np.array_equal(sim.get_stream_grouping().cpu().numpy(), np.arange(N))
    sim.close()
    assert moved == want


def test_collav_none_stream_bitwise_with_grouping():
    """collav none never runs a pass and is not grouped unless asked; asked, it is as exact as the others."""
    N, cfg = 32, _cfg("none")
    table = _table(cfg.max_sampling_frequency, N, seed=19)
    on = _stream(cfg, N, _run_table(table, 512), 4, True)
    off = _stream(cfg, N, _run_table(table, 512), 4, False)
    _check_perms(on, N)
    assert any(not np.array_equal(p, np.arange(N)) for p in on["perms"])
    _same(on, off, N)


def test_multi_obstacle_stream_bitwise_with_grouping():
    """K = 2 obstacle ships (four ship slots, the multi-obstacle SBMPC pass)."""
    N, cfg = 32, _cfg(n_obs=2)
    table = _table(cfg.max_sampling_frequency, N, seed=11)
    on = _stream(cfg, N, _run_table(table, 512), 4, True, n_obs=2)
    off = _stream(cfg, N, _run_table(table, 512), 4, False, n_obs=2)
    _check_perms(on, N)
    _same(on, off, N)


@pytest.mark.parametrize("deterministic", [True, False])
def test_policy_stream_bitwise_with_grouping(deterministic):
    """shipsim_run_policy: the wave-cooperative policy pass serves whichever envs share the wave; an env's action
    (and, stochastic, its noise: keyed by the env, the counter and its decision's sequence number) is its own."""
    from test_gpu_policy_act import _trainer
    tr, _ = _trainer(64)
    seed = 0x1234_5678_9ABC
    dp = tr.device_policy(True) if deterministic else tr.device_policy(False, seed=seed)
    N, cfg = 32, _cfg()
    n_dec = int(cfg.max_sampling_frequency)

    def launch(counter):
        def f(sim, c, ep, dec, log, ln):
            o = sim.run_policy(dp.weights(), 512, n_dec, ep, dec, deterministic=deterministic, seed=seed,
                               counter=counter, log=log, log_len=ln)
            counter.add_(1)
            return o
        return f

    on = _stream(cfg, N, launch(torch.full((1,), 5, dtype=torch.int64, device="cuda")), 4, True)
    off = _stream(cfg, N, launch(torch.full((1,), 5, dtype=torch.int64, device="cuda")), 4, False)
    _check_perms(on, N)
    _same(on, off, N)


def test_weather_stream_bitwise_with_grouping():
    """Per-env weather: the weather stays with the env, not with the slot."""
    import weather_harness as WH
    N, cfg = 32, _cfg()
    w = WH.interleaved(WH.four_weathers(cfg), N)
    weather = [w[k] for k in WH.KEYS]
    table = _table(cfg.max_sampling_frequency, N, seed=13)
    on = _stream(cfg, N, _run_table(table, 512), 4, True, weather=weather)
    off = _stream(cfg, N, _run_table(table, 512), 4, False, weather=weather)
    _check_perms(on, N)
    _same(on, off, N)


def test_launch_tail_with_grouping_keeps_every_record():
    """With the work-conserving launch tail the ticks a launch gives an env depend on its wave-mates by design, so
    launch boundaries differ between the two runs; the record of a given (env, episode, decision) does not."""
    N, cfg = 64, _cfg()
    table = _table(cfg.max_sampling_frequency, N)
    on = _stream(cfg, N, _run_table(table, 512), 8, True, tail=64)
    off = _stream(cfg, N, _run_table(table, 512), 8, False, tail=64)
    _check_perms(on, N)
    _same(on, off, N, tail=True)
    assert all(int(t.max()) <= 512 + 64 for t in on["ticks"])
    n_cmp = 0
    for i in range(N):
        a = {(r[abi.DL_EPISODE], r[abi.DL_DECISION]): r.tobytes() for r in on["recs"][i]}
        b = {(r[abi.DL_EPISODE], r[abi.DL_DECISION]): r.tobytes() for r in off["recs"][i]}
        both = set(a) & set(b)
        assert len(both) == min(len(a), len(b)) >= 2  # one run's records are a prefix of the other's
        for k in both:
            assert a[k] == b[k], (i, k)
        n_cmp += len(both)
    assert n_cmp > 8 * N
