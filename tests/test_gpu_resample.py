"""Weighted splitting on the device: shipsim_resample against the Python-integer restatement (tests/resample_ref.py,
exact), shipsim_level_distance against numpy on get_state (bit-equal), BatchedMultiShipRLEnv.split against the envs'
state before it, and resample + fork captured in one graph. Needs an MI355X."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import resample_ref as R
from ast_sac_amd import shipsim, shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args
from ast_sac_amd.shipsim import ShipSim, ShipSimError

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678EF01
T = R.tile()
# 1, 2; around one tile and past two; every level of the scan: more tiles than the 256 tile sums the offsets
# kernel takes per round, so that its carry between rounds is used; and the CPU test's largest
ALL_LEVELS = 256 * T + T + 3
SIZES = [1, 2, T - 1, T, T + 1, 2 * T + 1, ALL_LEVELS, 4099]
ARR = {"sorted": R.SORTED, "in_place": R.IN_PLACE}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _counter(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def _ref(n, counter, arrangement):
    w, pot = R.inputs(n)
    hi, lo = R.offset_bits(SEED, counter)
    return R.resample(w, pot, hi, lo, ARR[arrangement])


def _device(w, pot, counter, arrangement, alias=False):
    wd = torch.from_numpy(np.asarray(w, np.float64)).cuda()
    pd = torch.from_numpy(np.asarray(pot, np.float64)).cuda()
    src, wout, total, status = shipsim.resample(wd, pd, SEED, _counter(counter), arrangement=arrangement,
                                                out_weight=wd if alias else None)
    torch.cuda.synchronize()
    if alias:
        assert wout.data_ptr() == wd.data_ptr()
    else:  # the inputs are read, not written
        np.testing.assert_array_equal(wd.cpu().numpy().view(np.uint64), np.asarray(w, np.float64).view(np.uint64))
    return src.cpu().numpy(), wout.cpu().numpy(), float(total.cpu()[0]), int(status.cpu()[0])


def _check(got, ref):
    src, wout, total, status = got
    assert status == ref["status"]
    np.testing.assert_array_equal(src, ref["src"])
    assert src.dtype == np.int32
    np.testing.assert_array_equal(wout.view(np.uint64), ref["weight"].view(np.uint64))
    assert np.float64(total).view(np.uint64) == np.float64(ref["total"]).view(np.uint64)


@pytest.mark.parametrize("arrangement", ["sorted", "in_place"])
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_restatement(n, arrangement):
    w, pot = R.inputs(n)
    ref = _ref(n, 5, arrangement)
    assert ref["status"] == 0
    _check(_device(w, pot, 5, arrangement), ref)


@pytest.mark.parametrize("arrangement", ["sorted", "in_place"])
def test_counter_and_seed_reach_the_offset(arrangement):
    n = 2 * T + 1
    w, pot = R.inputs(n)
    big = 2**40 + 5  # both counter words
    _check(_device(w, pot, big, arrangement), _ref(n, big, arrangement))
    assert _ref(n, big, arrangement)["U"] != _ref(n, 5, arrangement)["U"]


@pytest.mark.parametrize("arrangement", ["sorted", "in_place"])
@pytest.mark.parametrize("n", [T + 1, 4099])
def test_weight_out_may_be_weight(n, arrangement):
    w, pot = R.inputs(n)
    _check(_device(w, pot, 5, arrangement, alias=True), _ref(n, 5, arrangement))


@pytest.mark.parametrize("arrangement", ["sorted", "in_place"])
@pytest.mark.parametrize("n", [2, 2 * T + 1])
def test_equal_masses_select_every_env_once(n, arrangement):
    w, pot = np.full(n, 1.0 / n), np.full(n, 0.375)
    hi, lo = R.offset_bits(SEED, 9)
    ref = R.resample(w, pot, hi, lo, ARR[arrangement])
    np.testing.assert_array_equal(ref["src"], np.arange(n))
    got = _device(w, pot, 9, arrangement)
    _check(got, ref)
    np.testing.assert_array_equal(got[0], np.arange(n))


@pytest.mark.parametrize("arrangement", ["sorted", "in_place"])
@pytest.mark.parametrize("n,k", [(5, 3), (2 * T + 1, T + 7)])
def test_one_env_holding_all_the_mass_fills_every_slot(n, k, arrangement):
    w, pot = np.zeros(n), np.ones(n)
    w[k] = 0.25
    hi, lo = R.offset_bits(SEED, 9)
    ref = R.resample(w, pot, hi, lo, ARR[arrangement])
    got = _device(w, pot, 9, arrangement)
    _check(got, ref)
    np.testing.assert_array_equal(got[0], np.full(n, k))  # (in place: k keeps its own slot, as every slot holds k)
    # n clones of weight w / n: q = Q, so the factor is 1 / n exactly
    np.testing.assert_array_equal(got[1], np.full(n, 0.25 * (1.0 / n)))
    assert got[2] == 0.25


@pytest.mark.parametrize("arrangement", ["sorted", "in_place"])
@pytest.mark.parametrize("case,status", [("zero", 1), ("nan", 2), ("negative", 2)])
def test_without_usable_mass_nothing_moves(case, status, arrangement):
    n = 2 * T + 1
    w, pot = R.inputs(n)
    w = w + 0.125
    if case == "zero":
        pot = np.zeros(n)
    elif case == "nan":
        pot[T + 3] = np.nan
    else:
        pot[n - 1] = -1.0
    src, wout, total, st = _device(w, pot, 5, arrangement)
    assert st == status and total == 0.0
    np.testing.assert_array_equal(src, np.arange(n))
    np.testing.assert_array_equal(wout.view(np.uint64), w.view(np.uint64))
    hi, lo = R.offset_bits(SEED, 5)
    assert R.resample(w, pot, hi, lo, ARR[arrangement])["status"] == status


def test_binding_refuses_what_the_library_would():
    w = torch.ones(8, dtype=torch.float64, device="cuda")
    with pytest.raises(ShipSimError, match="arrangement"):
        shipsim.resample(w, w, 0, _counter(0), arrangement="shuffled")
    with pytest.raises(ShipSimError, match="potentials"):
        shipsim.resample(w, w[:4], 0, _counter(0))
    with pytest.raises(ShipSimError, match="counter"):
        shipsim.resample(w, w, 0, torch.zeros(1, dtype=torch.int32, device="cuda"))


# ---- the level ------------------------------------------------------------------------------------------------
def _stream_env(n, k=1, collav="none", ticks=64, seed=77):
    env = BatchedMultiShipRLEnv(default_args(collav_mode=collav, n_obs_ships=k), n)
    n_dec = int(env.cfg.max_sampling_frequency)
    a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (4, n_dec, n)).astype(np.float32)
    table = torch.from_numpy(abi.normalized_to_scoping(a)).cuda()
    ep = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec = torch.zeros(n, dtype=torch.int32, device="cuda")
    env.reset()
    env.sim.run_table(table, ticks, ep, dec)
    env.sim.synchronize()
    return env, table, ep, dec


@pytest.mark.parametrize("k", [1, 3])
def test_level_distance_is_numpy_on_get_state(k):
    n = 8
    env, *_ = _stream_env(n, k=k)
    sim = env.sim
    north = sim.get(abi.F_NORTH).cpu().numpy().reshape(n, k + 1)
    east = sim.get(abi.F_EAST).cpu().numpy().reshape(n, k + 1)
    dn, de = north[:, :1] - north[:, 1:], east[:, :1] - east[:, 1:]
    want = np.sqrt(dn * dn + de * de).min(axis=1)
    got = sim.level_distance().cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(want > 0) and np.all(np.isfinite(want))
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert env.level_distance(out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))
    env.close()


def test_level_distance_refusals():
    sim = ShipSim(abi.c2_config(), 4)
    sim.reset()
    with pytest.raises(ShipSimError, match="single-ship handle"):
        sim.level_distance()
    sim.close()
    sim = ShipSim(abi.ast_config("none"), 4)
    with pytest.raises(ShipSimError, match="level_distance before reset"):
        sim.level_distance()
    sim.close()


# ---- split ----------------------------------------------------------------------------------------------------
def _env_bytes(sim, data):
    """A whole-state snapshot cut into envs: per env, the bytes of its share of every array of the state block
    (csrc/shipsim_state_host.hpp's table, restated)."""
    hdr = open(os.path.join(os.path.dirname(R.HOST_HEADER), "shipsim_state_host.hpp")).read()
    env_bytes = [int(x) for x in re.search(r"kEnvBytes\[\] = \{([^}]*)\}", hdr).group(1).split(",")]
    n, ns = sim.n_envs, sim.n_ships
    r256 = lambda b: (b + 255) & ~255  # noqa: E731
    ship, route, env = r256(n * ns * 8), r256(n * ns * abi.MAX_ROUTE * 8), r256(n * 32)
    cols = [(k * ship, (8 if k < 19 else 4) * ns) for k in range(22)]
    cols += [(22 * ship + k * route, abi.MAX_ROUTE * 8 * ns) for k in range(2)]
    env_off = 22 * ship + 2 * route
    cols += [(env_off + k * env, b) for k, b in enumerate(env_bytes)]
    assert env_off + len(env_bytes) * env == sim.state_bytes == data.size
    return [b"".join(data[o + i * b:o + (i + 1) * b].tobytes() for o, b in cols) for i in range(n)]


def test_split_moves_whole_envs_and_leaves_survivors_untouched():
    n = 16
    env, table, ep, dec = _stream_env(n)
    sim = env.sim
    fields = (abi.F_NORTH, abi.F_EAST, abi.F_YAW, abi.F_U)
    # every env told apart from every other, whatever the 64 ticks did: env j's ships j metres further north
    sim.set(abi.F_NORTH, sim.get(abi.F_NORTH) + torch.arange(n, device="cuda").repeat_interleave(2))
    before = {f: sim.get(f).cpu().numpy().reshape(n, 2) for f in fields}
    ep.copy_(torch.arange(n, dtype=torch.int32) % 3)  # (told apart after the gather)
    dec.copy_(torch.arange(n, dtype=torch.int32) % 5)
    ep0, dec0 = ep.cpu().numpy().copy(), dec.cpu().numpy().copy()
    snap0 = _env_bytes(sim, env.snapshot().data.cpu().numpy())
    w = np.full(n, 1.0 / n)
    w[[2, 11]] = 0.0
    pot = np.exp(-sim.level_distance().cpu().numpy() / 4000.0)
    pot[[0, 5, 6, 13]] *= 1e-3  # some envs all but starved, so that slots do change hands
    wd = torch.from_numpy(w).cuda()
    src, wout, total, status = env.split(wd, torch.from_numpy(pot).cuda(), SEED, _counter(3), ep, dec)
    sim.synchronize()
    hi, lo = R.offset_bits(SEED, 3)
    ref = R.resample(w, pot, hi, lo, R.IN_PLACE)
    s = src.cpu().numpy()
    np.testing.assert_array_equal(s, ref["src"])
    np.testing.assert_array_equal(wout.cpu().numpy().view(np.uint64), ref["weight"].view(np.uint64))
    assert int(status.cpu()[0]) == 0 and float(total.cpu()[0]) == ref["total"]
    moved = s != np.arange(n)
    assert moved.any() and not moved.all()
    for f in fields:
        np.testing.assert_array_equal(sim.get(f).cpu().numpy().reshape(n, 2).view(np.uint64),
                                      before[f][s].view(np.uint64))
    np.testing.assert_array_equal(ep.cpu().numpy(), ep0[s])
    np.testing.assert_array_equal(dec.cpu().numpy(), dec0[s])
    snap1 = _env_bytes(sim, env.snapshot().data.cpu().numpy())
    for j in range(n):
        assert snap1[j] == snap0[s[j]], j  # survivors (s[j] == j) untouched, clones whole
    env.close()


# ---- graph capture --------------------------------------------------------------------------------------------
def test_resample_and_fork_in_one_graph():
    n = 16
    env, table, ep, dec = _stream_env(n)
    sim = env.sim
    snap = env.snapshot()
    w = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    pot = torch.exp(-sim.level_distance() / 4000.0)
    pot[::3] *= 1e-3
    ctr = _counter(1)
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    wout = torch.empty(n, dtype=torch.float64, device="cuda")
    # eager once: the workspace, and the fork's staging block, exist before the capture
    shipsim.resample(w, pot, SEED, ctr, out_src=src, out_weight=wout)
    sim.fork(src)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            _, _, total, status = shipsim.resample(w, pot, SEED, ctr, out_src=src, out_weight=wout)
            sim.fork(src)
    for value in (7, 2**33 + 1):
        sim.restore(snap)
        ctr.fill_(value)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (src.cpu().numpy().copy(), wout.cpu().numpy().copy(), float(total.cpu()[0]), int(status.cpu()[0]))
        state = sim.snapshot().data.cpu().numpy().copy()
        # the eager call with that counter, from the same state
        sim.restore(snap)
        es, ew, et, est = shipsim.resample(w, pot, SEED, _counter(value))
        sim.fork(es)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[0], es.cpu().numpy())
        np.testing.assert_array_equal(got[1].view(np.uint64), ew.cpu().numpy().view(np.uint64))
        assert got[2] == float(et.cpu()[0]) and got[3] == int(est.cpu()[0]) == 0
        np.testing.assert_array_equal(state, sim.snapshot().data.cpu().numpy())
        hi, lo = R.offset_bits(SEED, value)
        np.testing.assert_array_equal(got[0], R.resample(w.cpu().numpy(), pot.cpu().numpy(), hi, lo, R.IN_PLACE)["src"])
    assert (got[0] != np.arange(n)).any()
    env.close()
