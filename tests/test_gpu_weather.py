"""Per-env wind and current on the device (shipsim_set_weather; ast_step_kernel<.., MODE 4..6, ..>, reset_wx_kernel).

The weather kernels evaluate the uniform kernels' expressions on lane values, so env i of a weather batch must
equal, bit for bit, env i of a uniform handle whose config carries env i's weather: in the step path, the table
stream (in-kernel resets) and the policy stream, for K = 1..4 obstacle ships. Weathers are interleaved (env i gets
weather i % 4): at 16 lanes per env a wave holds 4 envs, and the bug to catch is an env running a neighbour's.
Against the CPU oracle every env has a weather of its own. Needs an MI355X."""
import pickle

import numpy as np
import pytest
import torch

import gpu_harness as H
import weather_harness as WH
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.weather import KEYS, config_weather, env_weather, sample_weather
from ast_sac_amd.shipsim import ShipSim, ShipSimError
from parity import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _cfg(collav, k):
    return abi.ast_config(collav, n_obs_ships=k)


# ---- 1. step path -------------------------------------------------------------------------------------------
_uniform_step = {}


def _uniform_step_runs(collav, k):
    """The four uniform handles' runs of the shared tables (computed once per case)."""
    if (collav, k) not in _uniform_step:
        cfg = _cfg(collav, k)
        tables = H.make_tables(30, 2, seed=77)
        _uniform_step[collav, k] = [H.run_gpu(WH.cfg_with(cfg, w), tables) for w in WH.four_weathers(cfg)]
    return _uniform_step[collav, k]


@pytest.mark.parametrize("collav,k,lpe", [("none", 1, 0), ("sbmpc", 1, 0), ("sbmpc", 2, 0), ("none", 4, 0),
                                          ("none", 1, 8), ("sbmpc", 1, 8)])
def test_step_path_bitwise_against_uniform_handles(collav, k, lpe):
    n = 30  # not a multiple of the 4 (or 8) envs of a wave
    cfg = _cfg(collav, k)
    cfg.lanes_per_env = lpe
    tables = H.make_tables(n, 2, seed=77)
    ws = WH.four_weathers(cfg)
    gpu, fields, env_fields, ran_lpe = WH.run_gpu_weather(cfg, tables, WH.interleaved(ws, n))
    assert ran_lpe == (8 if lpe == 8 else 16)
    uni = _uniform_step_runs(collav, k)
    got = WH.records(gpu)
    want = [WH.records(u[0]) for u in uni]
    ns = 1 + k
    for i in range(n):
        assert got[i] == want[i % 4][i], f"env {i} (weather {i % 4})"
        for f in fields:
            np.testing.assert_array_equal(fields[f].reshape(n, ns, -1)[i], uni[i % 4][1][f].reshape(n, ns, -1)[i],
                                          err_msg=f"env {i} field {f}")
        for f in env_fields:
            assert env_fields[f][i] == uni[i % 4][2][f][i], (i, f)
    # the weathers matter: some env differs from the same env under the config's weather
    assert any(got[i] != want[0][i] for i in range(n) if i % 4)


# ---- 2. table stream ----------------------------------------------------------------------------------------
def _table(n, n_dec, n_eps=3, seed=4242):
    a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (n_eps, n_dec, n)).astype(np.float32)
    return torch.from_numpy(abi.normalized_to_scoping(a)).cuda()


def _table_launch(table):
    return lambda sim, ep, dec, log, ln: sim.run_table(table, 1024, ep, dec, log=log, log_len=ln)


_uniform_table = {}


def _uniform_table_runs(k):
    if k not in _uniform_table:
        cfg = _cfg("sbmpc", k)
        t = _table(32, cfg.max_sampling_frequency)
        _uniform_table[k] = [WH.run_stream(WH.cfg_with(cfg, w), 32, None, _table_launch(t))
                             for w in WH.four_weathers(cfg)]
    return _uniform_table[k]


@pytest.mark.parametrize("k,tail", [(1, 0), (2, 0), (1, 256)])
def test_table_stream_bitwise_against_uniform_handles(k, tail):
    n = 32
    cfg = _cfg("sbmpc", k)
    t = _table(n, cfg.max_sampling_frequency)
    ws = WH.four_weathers(cfg)
    got = WH.run_stream(cfg, n, WH.interleaved(ws, n), _table_launch(t), tail=tail, cap=128)
    uni = _uniform_table_runs(k)
    n_resets = 0
    for i in range(n):
        want = uni[i % 4][i]
        if tail:  # where a launch ends depends on timing: the records, decision by decision, do not
            m = min(len(got[i]), len(want))
            assert len(got[i]) >= len(want) and m >= 4
            np.testing.assert_array_equal(got[i][:m], want[:m], err_msg=f"env {i}")
        else:
            assert len(got[i]) == len(want) >= 4, f"env {i} log_len"
            np.testing.assert_array_equal(got[i], want, err_msg=f"env {i}")
        n_resets += int(got[i][-1, abi.DL_EPISODE])
    assert n_resets >= n  # the in-kernel reset ran under weather


# ---- 3. policy stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("collav,k", [("sbmpc", 1), ("none", 4)])
def test_policy_stream_bitwise_against_uniform_handles(collav, k):
    from test_gpu_policy_act import _trainer
    n = 32
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = _cfg(collav, k)
    n_dec = int(cfg.max_sampling_frequency)

    def launch(sim, ep, dec, log, ln):
        sim.run_policy(dp.weights(), 1024, n_dec, ep, dec, deterministic=True, log=log, log_len=ln)

    ws = WH.four_weathers(cfg)
    got = WH.run_stream(cfg, n, WH.interleaved(ws, n), launch, cap=128)
    uni = [WH.run_stream(WH.cfg_with(cfg, w), n, None, launch, cap=128) for w in ws]
    for i in range(n):
        want = uni[i % 4][i]
        assert len(got[i]) == len(want) >= 4, f"env {i} log_len"
        np.testing.assert_array_equal(got[i], want, err_msg=f"env {i}")


# ---- 4. weather equal to the config's is the plain handle ---------------------------------------------------
def test_config_weather_set_per_env_is_the_plain_handle():
    n = 30
    cfg = _cfg("sbmpc", 1)
    tables = H.make_tables(n, 2, seed=77)
    same = WH.interleaved([config_weather(cfg)], n)
    a, fa, ea, lpe = WH.run_gpu_weather(cfg, tables, same)
    b, fb, eb, _ = _uniform_step_runs("sbmpc", 1)[0]
    assert lpe == 16
    assert WH.records(a) == WH.records(b)
    for f in fa:
        np.testing.assert_array_equal(fa[f], fb[f])
    for f in ea:
        np.testing.assert_array_equal(ea[f], eb[f])
    t = _table(32, cfg.max_sampling_frequency)
    got = WH.run_stream(cfg, 32, WH.interleaved([config_weather(cfg)], 32), _table_launch(t))
    want = _uniform_table_runs(1)[0]
    for i in range(32):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"env {i}")


# ---- 5. against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("collav,k,n", [("none", 1, 64), ("sbmpc", 1, 64), ("sbmpc", 2, 32), ("sbmpc", 3, 24),
                                        ("none", 4, 32)])
def test_weather_vs_oracle(collav, k, n):
    """Every env under its own draw against the CPU oracle configured with that draw: counts, bits and done exact,
    obs and reward within 1e-5, no env off every perturbed variant, at most 10 % on a perturbed one."""
    cfg = _cfg(collav, k)
    tables = H.make_tables(n, 2, seed=11, special=False)
    w = sample_weather(n, seed=WH.SEED, **WH.RANGES)
    gpu, fields, env_fields, _ = WH.run_gpu_weather(cfg, tables, w)
    orc, perturbed, all_msgs, worst = [], 0, [], 0.0
    for i in range(n):
        cfg_i = WH.cfg_with(cfg, env_weather(w, i))
        o = H.run_oracle(cfg_i, [tables[i]])
        e, msgs, _ = H.compare([gpu[i]], [o])
        if msgs:  # (the perturbed variants only for an env that misses the exact one)
            variants = H.run_oracle_variants(cfg_i, [tables[i]], eps_list=H.PERTURBATIONS[1:])
            e, msgs, chosen = H.compare([gpu[i]], variants)
            o = variants[int(chosen[0])]
            perturbed += 1
        all_msgs += [f"env {i}: {m}" for m in msgs]
        worst = max(worst, e)
        orc.append(o[0])
    print(f"\n[weather vs oracle {collav} K={k} n={n}] envs accepted on a perturbed variant: {perturbed}, "
          f"worst rel err {worst:.3e}")
    assert not all_msgs, "\n".join(all_msgs[:20])
    assert worst <= 1e-5
    assert perturbed <= 0.1 * n, perturbed
    ships = np.array([o[1] for o in orc])  # (n, 1 + k, 20)
    for f, col in ((abi.F_NORTH, 0), (abi.F_EAST, 1), (abi.F_YAW, 2), (abi.F_U, 3), (abi.F_TIME, 7)):
        assert_close(fields[f].reshape(n, 1 + k), ships[:, :, col], what=f"K={k} field {f}")
    np.testing.assert_array_equal(fields[abi.F_STOP].reshape(n, 1 + k), ships[:, :, 18])
    np.testing.assert_array_equal(fields[abi.F_NEXT_WPT].reshape(n, 1 + k), ships[:, :, 17])


# ---- 6. surface ---------------------------------------------------------------------------------------------
def _first_decision(sim, n):
    sim.reset()
    out = sim.step(torch.zeros(n, device="cuda"))
    sim.synchronize()
    return (out["obs"].cpu().numpy().tobytes(), out["reward"].cpu().numpy().tobytes(),
            out["events"].cpu().numpy().tobytes(), out["ticks"].cpu().numpy().tobytes())


def test_weather_round_trip_clear_and_reset():
    n = 12
    cfg = _cfg("sbmpc", 1)
    w = sample_weather(n, seed=WH.SEED, **WH.RANGES)
    sim = ShipSim(cfg, n)
    auto_lpe = sim.lanes_per_env
    assert sim.weather() is None
    plain = _first_decision(sim, n)
    sim.set_weather(*[w[k] for k in KEYS])
    got = sim.weather()
    assert sorted(got) == sorted(KEYS)
    for k in KEYS:
        assert got[k].dtype == np.float64
        np.testing.assert_array_equal(got[k], w[k])
    under = _first_decision(sim, n)
    assert under != plain
    # reset(mask) keeps the weather: the same first decision again after a masked and a full reset
    sim.reset(mask=torch.ones(n, dtype=torch.uint8))
    np.testing.assert_array_equal(sim.weather()["wind_speed"], w["wind_speed"])
    assert _first_decision(sim, n) == under
    # a scalar broadcasts
    sim.set_weather(3.0, w["wind_direction"], 0.25, w["current_east"])
    np.testing.assert_array_equal(sim.weather()["wind_speed"], np.full(n, 3.0))
    np.testing.assert_array_equal(sim.weather()["current_north"], np.full(n, 0.25))
    sim.clear_weather()
    assert sim.weather() is None and sim.lanes_per_env == auto_lpe
    assert _first_decision(sim, n) == plain
    sim.close()


def test_small_lanes_per_env_runs_the_nearest_weather_kernel():
    cfg = _cfg("none", 1)
    cfg.lanes_per_env = 4
    sim = ShipSim(cfg, 8)
    assert sim.lanes_per_env == 4
    sim.set_weather(1.0, 0.5, 0.1, -0.1)
    assert sim.lanes_per_env == 8 == int(sim.L.shipsim_lanes_per_env(sim.h))
    sim.clear_weather()
    assert sim.lanes_per_env == 4
    sim.close()


def test_set_weather_refusals():
    n = 4
    ok = (np.full(n, 2.0), np.full(n, 0.3), np.full(n, -0.5), np.full(n, 0.5))
    for cfg, msg in ((abi.ast_config("none", machinery=abi.MACH_SIMPLIFIED), "detailed machinery"),
                     (abi.ast_config("simple"), "collav simple"),
                     (abi.c1_config("sbmpc"), "SHIPSIM_KIND_AST")):
        sim = ShipSim(cfg, n)
        with pytest.raises(ShipSimError, match=msg):
            sim.set_weather(*ok)
        assert sim.weather() is None
        sim.close()
    sim = ShipSim(_cfg("sbmpc", 1), n)
    sim.set_trajectory(16)
    with pytest.raises(ShipSimError, match="trajectory recording"):
        sim.set_weather(*ok)
    sim.clear_trajectory()
    sim.set_weather(*ok)
    for bad, msg in (((np.array([2.0, np.nan, 2.0, 2.0]),) + ok[1:], "env 1"),
                     ((ok[0], ok[1], np.array([0.0, 0.0, np.inf, 0.0]), ok[3]), "env 2"),
                     ((np.array([2.0, 2.0, 2.0, -0.1]),) + ok[1:], "wind speed")):
        with pytest.raises(ShipSimError, match=msg):
            sim.set_weather(*bad)
        np.testing.assert_array_equal(sim.weather()["wind_speed"], ok[0])  # nothing changed
    with pytest.raises(ShipSimError, match="entries"):
        sim.set_weather(np.full(n + 1, 2.0), *ok[1:])
    # a mix of NULL and non-NULL arrays
    p = [ok[0].ctypes.data, None, ok[2].ctypes.data, ok[3].ctypes.data]
    assert sim.L.shipsim_set_weather(sim.h, *p) == -1
    assert b"NULL" in sim.L.shipsim_last_error(sim.h)
    # recording and the legacy step on a weather handle
    with pytest.raises(ShipSimError, match="per-env weather"):
        sim.set_trajectory(16)
    sim.reset()
    with pytest.raises(ShipSimError, match="per-env weather"):
        sim.legacy_step(1)
    sim.close()


def test_env_facade_weather_recording_legacy_and_pickle():
    from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args
    n = 8
    w = sample_weather(n, seed=WH.SEED, **WH.RANGES)
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n, weather=w)
    for k in KEYS:
        np.testing.assert_array_equal(env.weather()[k], w[k])
    with pytest.raises(ShipSimError, match="per-env weather"):
        env.record_trajectories()
    env.reset()
    with pytest.raises(ShipSimError, match="per-env weather"):
        env.legacy_step(1)
    env2 = pickle.loads(pickle.dumps(env))
    for k in KEYS:
        np.testing.assert_array_equal(env2.weather()[k], w[k])
    a = torch.zeros((n, 1), device=env.device)
    outs = []
    for e in (env, env2):
        e.reset()
        o, r, d, info = e.step(a)
        outs.append((o.cpu().numpy().tobytes(), r.cpu().numpy().tobytes(), info["events"].cpu().numpy().tobytes()))
    assert outs[0] == outs[1]
    # a snapshot without the key (an older one) loads as before: uniform
    st = env.__getstate__()
    del st["weather"]
    env3 = BatchedMultiShipRLEnv.__new__(BatchedMultiShipRLEnv)
    env3.__setstate__(st)
    assert env3.weather() is None
    env.set_weather(None)
    assert env.weather() is None
    for e in (env, env2, env3):
        e.close()


# ---- 7. collector -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_fused_collector_on_a_weather_env(k):
    """The fused collector needs nothing beyond what run_policy does: on a weather env its replay rows are the
    transitions of run_policy driven by hand on an equally configured handle (as
    test_gpu_multi_obstacle_training.py does for K = 2)."""
    from test_gpu_policy_act import _trainer
    from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args
    from ast_sac_amd.ast_sac.env_wrapper.normalized_box_env import BatchedNormalizedBoxEnv
    from ast_sac_amd.ast_sac.samplers.data_collector.batched_collector import BatchedPathCollector
    from ast_sac_amd.ast_sac.data_management.replay_buffer import DeviceReplayBuffer
    tr, pol = _trainer(64)
    N, T, ticks, P, scale = 16, 9, 320, 8, 0.75
    w = WH.interleaved(WH.four_weathers(_cfg("sbmpc", k)), N)
    args = default_args(collav_mode="sbmpc", n_obs_ships=k)
    base = BatchedMultiShipRLEnv(args, N, weather=w)
    env = BatchedNormalizedBoxEnv(base, scale)
    dp = tr.device_policy(True)
    coll = BatchedPathCollector(env, pol, max_path_length=T, max_ticks=ticks, deterministic=True, device_policy=dp,
                                use_graph=False, stream_tail=0)
    assert coll.fused
    rb = DeviceReplayBuffer(20000, 8, 1, "cuda")
    coll._take_over()
    coll._enter("fused")
    for _ in range(P):
        coll._fused_pass(rb, True)
    coll._drain_ring()
    torch.cuda.synchronize()
    env2 = BatchedMultiShipRLEnv(args, N, weather=w)
    sim = env2.sim
    sim.reset()
    cap = coll._log_cap()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    ln = torch.zeros(N, dtype=torch.int32, device="cuda")
    rows = []
    for _ in range(P):
        ln.zero_()
        sim.run_policy(dp.weights(), ticks, T, ep, dec, deterministic=True, log=log, log_len=ln)
        L, n = log.cpu().numpy(), ln.cpu().numpy()
        assert n.max() <= cap
        for i in range(N):
            for r in L[i, :n[i]]:
                ev = int(r[abi.DL_EVENTS])
                if not ev & abi.EV_NONFINITE:
                    rows.append((r[abi.DL_OBS0:abi.DL_OBS0 + 8].astype(np.float32), np.float32(r[abi.DL_ACTION]),
                                 np.float32(r[abi.DL_REWARD] * scale), r[abi.DL_OBS:abi.DL_OBS + 8].astype(np.float32),
                                 np.float32(bool(ev & abi.EV_TERMINAL))))
    n_rows = rb.num_steps_can_sample()
    assert n_rows == len(rows) > 0
    st = {key: v[:n_rows].cpu().numpy() for key, v in rb._store.items()}
    np.testing.assert_array_equal(st["observations"], np.stack([r[0] for r in rows]))
    np.testing.assert_array_equal(st["actions"][:, 0], np.array([r[1] for r in rows]))
    np.testing.assert_array_equal(st["rewards"][:, 0], np.array([r[2] for r in rows]))
    np.testing.assert_array_equal(st["next_observations"], np.stack([r[3] for r in rows]))
    np.testing.assert_array_equal(st["terminals"][:, 0], np.array([r[4] for r in rows]))
    base.close()
    env2.close()
