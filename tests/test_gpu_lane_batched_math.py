"""The two-slot, 16-lane decision streams (shipsim_run_table / shipsim_run_policy, detailed machinery) take the three
square roots after a tick's Euler step (each ship's ground distance, the reward's distance, the obstacle ship's travel
step) in one call over the env row, one argument per sub-lane parity and ship, exchanged by DPP; they test the map
bounds without short-circuit branches; and with SBMPC the test ship's request block in front of the pass runs on every
lane, the obstacle ship's lanes keeping their LOS state by selects. The sliced shipsim_step kernels do none of this, so
the host-driven step loop of test_gpu_stream_reg_consts.py is the independent reference. Every comparison is bit for
bit: decision records (reward, events, done, episode, decision, ticks, observation), per-launch tick counts and the
final ship state.
  1. partial waves: 5 and 9 envs at 3 envs per wave (idle lanes beside a lone env; a row whose neighbours are not going
     while it ticks), in-kernel resets, launch boundaries mid-decision;
  2. waypoint advances: ships placed on their next waypoint, so the launch's first tick advances the index after the
     request block has used the LOS term of the old segment; with SBMPC, envs whose ships start the tick inside 2 km (a
     requesting tick) with and without an advance on that tick, the pass's carried result and the LOS integrator of
     both ships compared after it; the ordinary advances inside the launches are asserted from the state as well;
  3. a frozen obstacle ship: its lanes skip the ship tick while the test ship's lanes still receive their roots (and
     the obstacle ship's travel step is the 0 the guarded tick adds);
  4. placed states: inside the hull margin of a coastline edge (the corner tests instead of the far-shore shortcut),
     a shaft speed that makes omega + 0.1 tiny, and a NaN position (the non-finite contract).
Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSimNonFiniteError
from test_gpu_early_pose import FROZEN_SEED, _coast_point
from test_gpu_flat_tick import _PRE, _begin, _Host
from test_gpu_flat_tick import _Stream as _PlacedStream
from test_gpu_stream_reg_consts import (LAUNCHES, N_DEC, T, _assert_equal, _HostLoop, _state, _Stream, _table)

pytestmark = pytest.mark.gpu

_EV, _DONE = 1, 2  # columns of the kept record


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _np(sim, field):
    return sim.get(field).cpu().numpy()


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
@pytest.mark.parametrize("N", [5, 9])
def test_partial_waves_and_ordinary_waypoint_advances(collav, N):
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 3
    table = _table(4, N_DEC, N, seed=73 + N)
    host, stream = _HostLoop(cfg, N, table), _Stream(cfg, N, table)
    assert stream.sim.lanes_per_env == 16
    wpt0 = _np(stream.sim, abi.F_NEXT_WPT).copy()
    advanced = np.zeros(2 * N, bool)
    for _ in range(LAUNCHES):
        np.testing.assert_array_equal(stream.launch(T), np.full(N, T))
        host.launch(T)
        advanced |= _np(stream.sim, abi.F_NEXT_WPT) > wpt0
    assert _assert_equal(host, stream, f"{collav} N={N}") >= 3 * N
    eps = np.concatenate([r[:, 3] for r in stream.records()])
    assert eps.max() >= 1  # episodes were reset inside the kernel
    ends = [np.cumsum(r[:, 5]) for r in stream.records()]
    assert any(T * l not in c for c in ends for l in range(1, LAUNCHES))  # launch boundaries inside decisions
    assert advanced.any()  # a ship's waypoint index advanced inside a launch (read at the launches' ends)
    host.sim.close()
    stream.sim.close()


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_waypoint_advance_and_sbmpc_request_on_one_tick(collav):
    """Five ticks into the first decision (the obstacle ship's route then holds its sampled waypoint):
      env 0, 1: the test ship 1500 m from the obstacle ship: a requesting tick, no advance;
      env 2, 3: the test ship on its next waypoint, far from the obstacle ship: its advance, no request;
      env 4:    the obstacle ship on its next waypoint, far from the test ship: its advance, no request;
      env 5:    the obstacle ship on its next waypoint and the test ship 1500 m from it: a request and the obstacle
                ship's advance on the same tick;
      env 6, 7: as they were.
    (Only the test ship is moved off its route: an obstacle ship moved that far would end the episode on the tick by
    its travel tracker and its cross-track limit.)"""
    cfg = abi.ast_config(collav)
    N = 8
    table = _table(2, 3, N, seed=29)
    seen = {}

    def prepare(sim):
        _begin(sim, table)
        n, e = _np(sim, abi.F_NORTH), _np(sim, abi.F_EAST)
        rn, re = _np(sim, abi.E_ROUTE_NORTH), _np(sim, abi.E_ROUTE_EAST)
        rl, nw = _np(sim, abi.E_ROUTE_LEN), _np(sim, abi.F_NEXT_WPT)
        for i in (2, 3):
            t = 2 * i
            assert rl[t] > nw[t] + 1, (rl[t], nw[t])
            n[t], e[t] = rn[t, nw[t]] + 3.0, re[t, nw[t]] - 2.0
        for i in (4, 5):
            o = 2 * i + 1
            assert rl[o] > nw[o] + 1, (rl[o], nw[o])
            n[o], e[o] = rn[o, nw[o]] + 3.0, re[o, nw[o]] - 2.0
        for i in (0, 1, 5):
            n[2 * i], e[2 * i] = n[2 * i + 1] - 900.0, e[2 * i + 1] - 1200.0 - 7.0 * i
        seen["nw"], seen["n"], seen["e"] = nw.copy(), n.copy(), e.copy()
        sim.set(abi.F_NORTH, torch.from_numpy(n))
        sim.set(abi.F_EAST, torch.from_numpy(e))

    host, stream = _Host(cfg, N, table, prepare), _PlacedStream(cfg, N, table, 64, prepare)
    assert stream.sim.lanes_per_env == 16
    host.dticks[:] = _PRE
    n, e = seen["n"], seen["e"]
    dist = np.hypot(n[0::2] - n[1::2], e[0::2] - e[1::2])
    inside = dist < 2000.0  # the test of the SBMPC request (D_INIT), on the state the tick starts from
    assert inside[[0, 1, 5]].all() and (dist[[0, 1, 5]] > 1400.0).all() and not inside[[2, 3, 4, 6, 7]].any(), dist
    host.launch(stream.launch(1))
    placed = [4, 6, 9, 11]  # the test ships of envs 2, 3 and the obstacle ships of envs 4, 5
    for sim in (host.sim, stream.sim):
        nw = _np(sim, abi.F_NEXT_WPT)
        assert (nw[placed] == seen["nw"][placed] + 1).all(), nw  # advanced in that tick
    # the pass's carried result after the requesting tick (1, 0 where no pass ran), and the state after it
    for f in (abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST, abi.F_E_CT, abi.F_E_CT_INT):
        np.testing.assert_array_equal(_np(stream.sim, f), _np(host.sim, f))
    np.testing.assert_array_equal(_state(stream.sim), _state(host.sim))
    if collav == "sbmpc":
        assert (_np(stream.sim, abi.E_SBMPC_P_LAST)[[2, 3, 4, 6, 7]] == 1.0).all()
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


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_frozen_obstacle_ship(collav):
    """Whole episodes (9 decisions), the seed and the oracle check of test_gpu_early_pose.py: an obstacle ship that
    reaches its route's end or leaves the map stops there while the ship under test sails on for some hundred ticks."""
    import oracle_ffi as O
    cfg = abi.ast_config(collav)
    N, n_dec = 8, cfg.max_sampling_frequency
    table = _table(2, n_dec, N, seed=FROZEN_SEED)
    _, ticks, _, _, bits = O.ast_rollouts(cfg, np.ascontiguousarray(table[0].T))
    bits = bits.astype(np.int64)

    def held(b):  # the obstacle ship stopped on its own account, the episode ended later by the test ship's
        return (b & abi.EV_OBS_STOP != 0) & (b & abi.EV_TERMINAL == 0) & (b & abi.EV_TEST_STOP != 0) & \
            (b & (abi.EV_OBS_REACHES_END | abi.EV_OBS_OUTSIDE_MAP) != 0)

    frozen = held(bits)
    assert frozen.any(), [hex(b) for b in bits]
    assert ticks[frozen].max() < LAUNCHES * T  # those episodes end inside the launches
    host, stream = _HostLoop(cfg, N, table), _Stream(cfg, N, table)
    assert stream.sim.lanes_per_env == 16
    for _ in range(LAUNCHES):
        np.testing.assert_array_equal(stream.launch(T), np.full(N, T))
        host.launch(T)
    _assert_equal(host, stream, f"frozen obstacle ship {collav}")
    recs = stream.records()
    for i in np.nonzero(frozen)[0]:
        last = recs[i][recs[i][:, 3] == 0][-1]  # the last record of episode 0
        assert last[2] == 1 and held(int(last[1])), (i, hex(int(last[1])))
    host.sim.close()
    stream.sim.close()


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_placed_states(collav):
    cfg = abi.ast_config(collav)
    N = 8
    table = _table(4, N_DEC, N, seed=17)
    host, stream = _HostLoop(cfg, N, table), _Stream(cfg, N, table)
    assert stream.sim.lanes_per_env == 16
    north, east, omega = (_np(stream.sim, f).astype(np.float64).copy() for f in (abi.F_NORTH, abi.F_EAST, abi.F_OMEGA))
    # env 0, test ship: 45 m (inside l_ship / 2 * sqrt(2) = 56.6 m) off a coastline edge: far_shore false
    north[0], east[0] = _coast_point(cfg, 45.0)
    # env 1, both ships: omega + 0.1 = 2^-40 (the engine torques' shared denominator)
    omega[2] = omega[3] = -0.1 + 2.0 ** -40
    assert 0.0 < omega[2] + 0.1 < 1e-11
    # env 3, obstacle ship: a NaN north (the non-finite contract)
    north[7] = np.nan
    for sim in (host.sim, stream.sim):
        sim.set(abi.F_NORTH, torch.from_numpy(north).cuda())
        sim.set(abi.F_EAST, torch.from_numpy(east).cuda())
        sim.set(abi.F_OMEGA, torch.from_numpy(omega).cuda())
    for _ in range(LAUNCHES):
        np.testing.assert_array_equal(stream.launch(T), np.full(N, T))
        host.launch(T)
    _assert_equal(host, stream, f"placed {collav}")
    ev = [r[:, _EV].astype(np.int64) for r in stream.records()]
    assert ev[3][0] & abi.EV_NONFINITE and ev[3][0] & abi.EV_TERMINAL
    assert not any((ev[i] & abi.EV_NONFINITE).any() for i in range(N) if i != 3)
    assert not (ev[3][1:] & abi.EV_NONFINITE).any()  # reset in place, then normal
    for sim in (host.sim, stream.sim):
        with pytest.raises(ShipSimNonFiniteError):
            sim.synchronize()
        sim.close()
