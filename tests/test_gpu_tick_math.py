"""The headline decision stream (shipsim_run_table with collav sbmpc, two-slot, 16 lanes, detailed machinery)
evaluates the steady tick's three math-library calls itself: sincos(yaw), the LOS atan and the reward's exp restated
from the device library operation for operation (csrc/shipsim_tickmath.hpp), their constants delivered from a table in
registers by a row broadcast.
  1. The functions, by shipsim_tickmath_eval: one launch per function over about 2^20 arguments (every exponent, ±0,
     subnormals, ±inf, NaN, and each function's own edges); the library's value, the restated form's and the broadcast
     form's are the same bit patterns, and where the library returns NaN the others do.
  2. The streams, bit for bit against the host-driven shipsim_step loop (whose kernels keep calling the library): one
     wave and a partial second wave, a frozen obstacle ship beside a sailing test ship (partial rows at the sincos and
     atan sites), a heading above 2^30 beside ordinary envs in the same wave (the guard's library side; on the test
     ship, and on the obstacle ship alone), envs of one wave finishing and stalling at different ticks, collav sbmpc
     with a pass served in the wave, and collav none (whose kernel keeps the library's calls). These are table
     streams; the policy stream (whose kernels keep the library's calls too) has no case of its own here:
     test_gpu_stream_reg_consts.py (from reset) and test_gpu_sbmpc_nominal.py (placed requests, lone and paired
     passes) compare it with the host-driven loop.
Needs an MI355X."""
import functools
import os

import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim, shipsim_abi as abi
from test_gpu_flat_tick import _PRE, _begin, _Host, _run
from test_gpu_flat_tick import _Stream as _PlacedStream
from test_gpu_sbmpc_nominal import _PLANS, _compare_first_tick, _place
from test_gpu_stream_reg_consts import _state, _table

pytestmark = pytest.mark.gpu

_SIGN = np.uint64(1) << np.uint64(63)
_TWO30 = 2.0 ** 30


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _near(x, k=3):
    """x and its neighbours up to k ulps either side"""
    b = _bits(np.asarray(x, np.float64).reshape(-1)).astype(np.int64)
    return np.concatenate([b + d for d in range(-k, k + 1)]).astype(np.uint64).view(np.float64)


def _both_signs(x):
    return np.concatenate([x, -x])


def common_args(g, per_exp):
    """every exponent (0 .. 2046) with `per_exp` random mantissas, both signs; ±0, subnormals, ±inf, NaNs"""
    e = np.repeat(np.arange(2047, dtype=np.uint64), per_exp)
    m = g.integers(0, 1 << 52, len(e), dtype=np.uint64)
    pos = ((e << np.uint64(52)) | m).view(np.float64)
    # the powers of two (and +0), and the largest mantissa of every exponent
    edge = (np.arange(2047, dtype=np.uint64) << np.uint64(52)).view(np.float64)
    top = ((np.arange(2047, dtype=np.uint64) << np.uint64(52)) | np.uint64((1 << 52) - 1)).view(np.float64)
    sub = np.array([1, 2, 3, (1 << 51), (1 << 52) - 1], np.uint64).view(np.float64)
    nan = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FF8000000000123, 0x7FFFFFFFFFFFFFFF],
                   np.uint64).view(np.float64)
    return np.concatenate([_both_signs(np.concatenate([pos, edge, top, sub, [0.0, np.inf]])), nan,
                           (_bits(nan) | _SIGN).view(np.float64)])


@functools.lru_cache(maxsize=None)
def fn_args(fn, seed=2026, per_exp=96):
    """The arguments of one function: the common ones and its own edges (made once per process, read-only)"""
    g = np.random.Generator(np.random.PCG64(seed + {"sincos": 0, "atan": 1, "exp": 2}[fn]))
    parts = [common_args(g, per_exp)]
    if fn == "sincos":
        kmax = int(_TWO30 * 2 / np.pi)
        k = np.concatenate([np.arange(0, 4096), g.integers(0, kmax, 20000), [kmax - 1, kmax, kmax + 1]])
        parts.append(_both_signs(_near(k * (np.pi / 2))))           # neighbours of k·π/2
        parts.append(_both_signs(_near((k + 0.5) * (np.pi / 2))))   # the rint's ties of x·2/π
        parts.append(_both_signs(_near(_TWO30, 2)))                  # the guard's two sides
        parts.append(g.uniform(-8.0, 8.0, 200000))            # headings
        parts.append(g.uniform(-_TWO30, _TWO30, 100000))
    elif fn == "atan":
        parts.append(_both_signs(_near(1.0)))                        # the one internal threshold: |x| > 1
        parts.append(_both_signs(_near([0.5, 2.0, 1e-300, 1e300, 1e-8, 1e8, 2.0 ** -27, 2.0 ** 53])))
        parts.append(g.uniform(-4.0, 4.0, 300000))            # the LOS correction's arguments
        parts.append(np.tan(g.uniform(-np.pi / 2, np.pi / 2, 100000)))
    else:
        ln2 = np.log(2.0)
        parts.append(g.uniform(-1100.0, 0.0, 300000))         # the tick's range, past underflow
        parts.append(g.uniform(0.0, 1030.0, 100000))          # up to overflow and past it
        parts.append(-g.uniform(0.0, 1.0, 100000) ** 4 * 50)  # the reward terms' arguments, dense near 0
        m = np.arange(-1080, 1030)
        parts.append(_near((m + 0.5) * ln2))                         # the rint's ties of x / ln 2
        parts.append(_near(m * ln2))
        parts.append(_near([1024.0, -1075.0, -745.13321910194122, 709.78271289338397, -708.39641853226408]))
    x = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in parts])
    x.setflags(write=False)
    return x


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tickmath_device.npz")
_GOLDEN_N = 3000


def fixture_args(fn):
    """The CPU test's arguments (tests/golden/tickmath_device.npz): a fixed sample of fn_args and the specials"""
    x = fn_args(fn)
    g = np.random.Generator(np.random.PCG64(77))
    pick = x[g.choice(len(x), _GOLDEN_N, replace=False)]
    must = [0.0, 1.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308, 1e-300, 1e300, 1024.0, -1075.0, -745.2, 709.8]
    return np.concatenate([pick, _both_signs(np.array(must)), _both_signs(_near(_TWO30, 2)),
                           _both_signs(_near(1.0, 2))])


def record_fixture(path=GOLDEN):
    """Record the device library's result bits for fixture_args (run once on the GPU; the CPU test reads the file)"""
    d = {}
    for fn in ("sincos", "atan", "exp"):
        x = fixture_args(fn)
        out = shipsim.tickmath_eval(fn, x).cpu().numpy()
        d[fn + "_x"] = _bits(x)
        d[fn + "_lib"] = _bits(out[:, 0]) if fn == "sincos" else _bits(out[:, 0, 0])
    np.savez_compressed(path, **d)


def test_golden_fixture_holds_the_device_librarys_bits():
    """tests/golden/tickmath_device.npz (the CPU test's reference) is what this device's library returns today"""
    z = np.load(GOLDEN)
    for fn in ("sincos", "atan", "exp"):
        x = fixture_args(fn)
        np.testing.assert_array_equal(z[fn + "_x"], _bits(x))
        out = shipsim.tickmath_eval(fn, x).cpu().numpy()
        got = _bits(out[:, 0]) if fn == "sincos" else _bits(out[:, 0, 0])
        nan = np.isnan(z[fn + "_lib"].view(np.float64))
        np.testing.assert_array_equal(got[~nan], z[fn + "_lib"][~nan])
        assert np.isnan(got.view(np.float64)[nan]).all()


@functools.lru_cache(maxsize=None)
def device_values(fn):
    """(arguments, (n, 3, 2) values: library, restated, broadcast) of one launch, read-only"""
    x = fn_args(fn)
    out = shipsim.tickmath_eval(fn, x).cpu().numpy()
    out.setflags(write=False)
    return x, out


@pytest.mark.parametrize("fn", ["sincos", "atan", "exp"])
def test_restated_and_broadcast_forms_are_the_librarys_bits(fn):
    x, out = device_values(fn)
    assert 2 ** 19 <= len(x) <= 2 ** 21
    lib, lit, row = (_bits(out[:, k]) for k in range(3))
    nan = np.isnan(out[:, 0])
    for name, got in (("restated", lit), ("broadcast", row)):
        diff = (got != lib) & ~nan
        n = int(diff.sum())
        where = np.nonzero(diff.any(1))[0][:5]
        print(f"\n[tick math {fn}] {name}: {n} differing patterns of {lib.size} ({int(nan.sum())} library NaNs)")
        assert n == 0, [(float(x[i]).hex(), [hex(int(v)) for v in lib[i]], [hex(int(v)) for v in got[i]])
                        for i in where]
        assert np.isnan(got.view(np.float64)[nan]).all()  # where the library returns NaN the others do
    if fn == "sincos":  # sanity of the reference itself, and that both sides of the guard are in the batch
        ok = np.isfinite(x) & (np.abs(x) < 1e6)
        assert np.abs(out[ok, 0, 0] - np.sin(x[ok])).max() < 1e-9 and np.abs(out[ok, 0, 1] - np.cos(x[ok])).max() < 1e-9
        assert (np.abs(x) < _TWO30).sum() > 1000 and (np.abs(x[np.isfinite(x)]) >= _TWO30).sum() > 1000
        assert nan[~np.isfinite(x)].all()
    elif fn == "atan":
        ok = ~np.isnan(x)
        assert np.abs(out[ok, 0, 0] - np.arctan(x[ok])).max() < 1e-15 * 4 and (out[:, :, 1] == 0).all()
    else:
        ok = np.isfinite(x) & (x < 700) & (x > -700)
        assert np.abs(out[ok, 0, 0] / np.exp(x[ok]) - 1).max() < 1e-15 * 4
        assert (out[x > 1024.0, 0, 0] == np.inf).all() and (out[x < -1075.0, 0, 0] == 0).all()


def test_partial_last_block_and_unaligned_counts():
    """counts that are no multiple of the wave or of the row: lanes past n write nothing"""
    x = np.linspace(-3.0, 3.0, 64 * 3 + 21)
    for n in (1, 15, 17, 64, 65, len(x)):
        out = shipsim.tickmath_eval("sincos", x[:n]).cpu().numpy()
        assert out.shape == (n, 3, 2)
        np.testing.assert_array_equal(_bits(out[:, 1]), _bits(out[:, 0]))
        np.testing.assert_array_equal(_bits(out[:, 2]), _bits(out[:, 0]))
        assert np.abs(out[:, 0, 0] - np.sin(x[:n])).max() < 1e-15


# ---- the streams -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("collav", ["sbmpc", "none"])
@pytest.mark.parametrize("N", [4, 6])
def test_one_wave_and_a_partial_second_wave(collav, N):
    """Four envs per wave: N = 4 fills one wave, N = 6 leaves half of the second idle. Env 1 runs one good decision and
    then only failing samplings, so it stalls mid-launch beside wave neighbours that tick on; decisions of different
    envs finish at different ticks; in-kernel resets; launches ending inside decisions."""
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 4
    table = _table(10, 3, N, seed=83 + N)
    table[0, 1, 1] = 1.5
    table[1:, 0, 1] = 1.5
    ss, ticks, _ = _run(cfg, N, table, launches=3, T=200, cap=64, ahead=3)
    assert sum(len(r) for r in ss) >= 2 * N
    assert (ticks[:, 1] < 200).any() and (ticks[:, [0, 2, 3]] == 200).all()
    ends = {int(r[0, 5]) for i, r in enumerate(ss) if i != 1 and len(r)}
    assert len(ends) > 1  # the wave's envs completed their first decisions at different ticks


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_frozen_obstacle_ship_beside_sailing_test_ship(collav):
    """Envs 0 and 2 of a wave: the obstacle ship frozen from the start, so its lanes sit out the ship tick while the
    test ship's lanes of the same row evaluate the atan and the sincos (their constants come from the test ship's
    lanes). Envs 1, 3 and the second wave's sail on whole."""
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 4
    N = 6
    table = _table(2, 3, N, seed=19)

    def prepare(sim):
        _begin(sim, table)
        stop = sim.get(abi.F_STOP).cpu().numpy()
        stop[[1, 5]] = 1
        sim.set(abi.F_STOP, torch.from_numpy(stop))

    host, stream = _Host(cfg, N, table, prepare), _PlacedStream(cfg, N, table, 64, prepare)
    host.dticks[:] = _PRE
    before = _state(stream.sim)
    for k, T in enumerate((1, 20, 150, 150)):
        host.launch(stream.launch(T))
        if k < 2:  # while no episode has ended: the frozen ships are still frozen where they were, the others moved
            np.testing.assert_array_equal(_state(stream.sim), _state(host.sim))
            stop = stream.sim.get(abi.F_STOP).cpu().numpy()
            assert (stop[[1, 5]] == 1).all() and (stop[[0, 2, 3, 4]] == 0).all(), stop
            now = _state(stream.sim)
            np.testing.assert_array_equal(now[[1, 5], :7], before[[1, 5], :7])  # (all but the time)
            assert (now[[0, 4], :2] != before[[0, 4], :2]).any(1).all()  # their test ships sailed on
    hs, ss = host.records(), stream.records()
    for i in range(N):
        k = len(hs[i])
        assert k <= len(ss[i]) <= k + 8, (i, k, len(ss[i]))
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"env {i}")
    same = np.repeat(np.array([len(h) == len(s) for h, s in zip(hs, ss)]), 2)
    assert same.sum() >= 2 * (N - 2), same
    np.testing.assert_array_equal(_state(stream.sim)[same], _state(host.sim)[same])
    assert sum(len(r) for r in ss) >= 2  # decisions completed and were compared
    host.sim.close()
    stream.sim.close()


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_heading_above_two_to_the_thirty(collav):
    """Env 1: the test ship's heading just above 2^30; env 2: the obstacle ship's alone (its row's test ship
    ordinary); env 5 (second wave): both. Their sincos is the library's large-argument path, taken by the whole row,
    beside ordinary envs of the same wave on the restated path."""
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 4
    N = 6
    table = _table(2, 3, N, seed=23)
    big = {2: _TWO30 + 4096.0, 5: 1.5 * _TWO30, 10: 3.0 * _TWO30, 11: -(_TWO30 + 1.0)}

    def prepare(sim):
        _begin(sim, table)
        yaw = sim.get(abi.F_YAW).cpu().numpy().astype(np.float64)
        for q, v in big.items():
            yaw[q] = v + np.copysign(yaw[q] % (2 * np.pi), v)  # (the heading's own phase, away from zero)
        sim.set(abi.F_YAW, torch.from_numpy(yaw))

    host, stream = _Host(cfg, N, table, prepare), _PlacedStream(cfg, N, table, 64, prepare)
    host.dticks[:] = _PRE
    host.launch(stream.launch(1))
    np.testing.assert_array_equal(_state(stream.sim), _state(host.sim))
    yaw = stream.sim.get(abi.F_YAW).cpu().numpy()
    assert (np.abs(yaw[list(big)]) > _TWO30).all()  # the tick's sincos saw a heading past the guard
    for _ in range(2):
        host.launch(stream.launch(120))
    hs, ss = host.records(), stream.records()
    for i in range(N):
        k = len(hs[i])
        assert k <= len(ss[i]) <= k + 8, (i, k, len(ss[i]))
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"env {i}")
    same = np.repeat(np.array([len(h) == len(s) for h, s in zip(hs, ss)]), 2)
    assert same.sum() >= 2 * (N - 2), same
    np.testing.assert_array_equal(_state(stream.sim)[same], _state(host.sim)[same])
    host.sim.close()
    stream.sim.close()


def test_table_stream_across_a_served_pass():
    """collav sbmpc, five envs at three per wave: a refused request between two accepted ones, so the wave runs the
    cooperative pass with the table live across it, and the ticks after it still read their constants."""
    cfg = abi.ast_config("sbmpc")
    cfg.envs_per_wave = 3
    N = 5
    plan = _PLANS[(5, 3)]
    table = _table(2, 3, N, seed=61 + N)
    seen = {}

    def prepare(sim):
        _begin(sim, table)
        _place(cfg, sim, plan, seen)

    host, stream = _Host(cfg, N, table, prepare), _PlacedStream(cfg, N, table, 64, prepare)
    host.dticks[:] = _PRE
    host.launch(stream.launch(1))
    _compare_first_tick(host.sim, stream.sim, plan, seen)
    assert not seen["flags"][1] and seen["flags"][[0, 2]].all()  # env 1 went to the pass
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
    host.sim.close()
    stream.sim.close()
