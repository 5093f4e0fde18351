"""The two-slot, 16-lane decision streams (shipsim_run_table / shipsim_run_policy, detailed machinery) form the
position after a tick's Euler step before the control chain, take the map query's grid cell from it and request a
new cell's edge share and class there, so those loads run under the control chain; their edge loop reads the next
edge ahead of the current one's arithmetic. The
sliced shipsim_step kernels do none of this (they compute the cell at the query), so the host-driven step loop of
test_gpu_stream_reg_consts.py is the independent reference. Every comparison is bit for bit: decision records,
per-launch tick counts and the final ship state.
  1. partial waves with in-kernel resets (a reset moves a ship to another cell between two queries), launch
     boundaries mid-decision (the first tick of a launch has no cell yet), ships crossing >= 10 grid cells;
  2. placed positions: next to a cell line, next to a coastline edge with hull corners in another cell than the
     centre, beyond the padded grid (cell -1: the full-map loop) and a NaN position (cell -1, EV_NONFINITE);
  3. a frozen obstacle ship (stopped at its route's end while the episode goes on): it keeps its position and cell
     while its time advances;
  4. the policy stream (MODE 2 of the same kernels).
Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim, ShipSimNonFiniteError
from test_gpu_stream_reg_consts import (CAP, LAUNCHES, N_DEC, T, _assert_equal, _assert_state_equal, _HostLoop,
                                        _Stream, _table)

pytestmark = pytest.mark.gpu

CELL = 200.0       # the map grid's cell size [m]; its lines lie at multiples of it on the reference map
GRID_PAD = 2000.0  # grid beyond the polygons' bounding box [m]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _pos(sim):
    return np.stack([sim.get(abi.F_NORTH).cpu().numpy(), sim.get(abi.F_EAST).cpu().numpy()], 1).astype(np.float64)


def _cells_between(a, b):
    """Grid lines between positions a and b (rows of north, east), north-south and east-west ones together: a ship
    that went from a to b crossed each at least once, entering a new cell every time."""
    return np.abs(np.floor(b / CELL) - np.floor(a / CELL)).sum(1)


def _events(stream):
    return [r[:, 1].astype(np.int64) for r in stream.records()]  # (_KEEP column 1: DL_EVENTS)


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
@pytest.mark.parametrize("N", [5, 9])
def test_partial_waves_resets_and_cell_changes(collav, N):
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 3
    table = _table(4, N_DEC, N, seed=57 + N)
    host, stream = _HostLoop(cfg, N, table), _Stream(cfg, N, table)
    assert stream.sim.lanes_per_env == 16
    start = _pos(stream.sim)
    far = np.zeros(2 * N)
    for _ in range(LAUNCHES):
        np.testing.assert_array_equal(stream.launch(T), np.full(N, T))
        host.launch(T)
        far = np.maximum(far, _cells_between(start, _pos(stream.sim)))
    assert _assert_equal(host, stream, f"{collav} N={N}") >= 3 * N
    eps = np.concatenate([r[:, 3] for r in stream.records()])
    assert eps.max() >= 1  # episodes were reset inside the kernel
    # every ship was read back >= 10 cell changes from where its episodes start
    assert far.min() >= 10, far
    host.sim.close()
    stream.sim.close()


def _coast_point(cfg, reach):
    """A water position `reach` metres off a coastline edge of the config's map whose hull corners (+-40 m along
    north and east) do not all lie in the centre's grid cell: (north, east)."""
    def inside(n, e):
        hit = False
        for p in range(cfg.n_polys):
            a, b = cfg.poly_start[p], cfg.poly_start[p + 1]
            x, y = np.array(cfg.poly_east[a:b]), np.array(cfg.poly_north[a:b])
            x2, y2 = np.roll(x, -1), np.roll(y, -1)
            cross = ((y > n) != (y2 > n)) & (e < (x2 - x) * (n - y) / np.where(y2 == y, 1.0, y2 - y) + x)
            hit = hit or bool(cross.sum() % 2)
        return hit

    a, b = cfg.poly_start[5], cfg.poly_start[6]  # (a small island)
    x, y = np.array(cfg.poly_east[a:b]), np.array(cfg.poly_north[a:b])
    for k in range(b - a):
        ax, ay, bx, by = x[k], y[k], x[(k + 1) % (b - a)], y[(k + 1) % (b - a)]
        L = np.hypot(bx - ax, by - ay)
        for sgn in (1.0, -1.0):
            nx, ny = sgn * (by - ay) / L, -sgn * (bx - ax) / L
            for t in np.linspace(0.2, 0.8, 61):
                e, n = ax + t * (bx - ax) + reach * nx, ay + t * (by - ay) + reach * ny
                if inside(n, e):
                    continue
                cells = {(np.floor((n + dn) / CELL), np.floor((e + de) / CELL)) for dn in (-40, 40) for de in (-40, 40)}
                if len(cells) > 1:
                    return float(n), float(e)
    raise AssertionError("no such position on this map")


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_placed_positions(collav):
    cfg = abi.ast_config(collav)
    N = 8
    table = _table(4, N_DEC, N, seed=91)
    host, stream = _HostLoop(cfg, N, table), _Stream(cfg, N, table)
    assert stream.sim.lanes_per_env == 16
    north, east = _pos(stream.sim).T.copy()
    # env 0, test ship (heading 60 deg, north-east): half a metre south of a cell line, crossed on the first tick
    north[0], east[0] = 2 * CELL - 0.5, 150.0
    # env 1, test ship: 45 m (inside l_ship / 2 * sqrt(2) = 56.6 m) off a coastline edge, corners in another cell
    north[2], east[2] = _coast_point(cfg, 45.0)
    # env 2, test ship: 5 km south of the map, beyond the padded grid (cell -1), outside the map at once
    north[4] = min(cfg.poly_north[:cfg.poly_start[cfg.n_polys]]) - GRID_PAD - 3000.0
    # env 3, obstacle ship: a NaN north (cell -1, the non-finite contract)
    north[7] = np.nan
    for sim in (host.sim, stream.sim):
        sim.set(abi.F_NORTH, torch.from_numpy(north).cuda())
        sim.set(abi.F_EAST, torch.from_numpy(east).cuda())
    for _ in range(LAUNCHES):
        np.testing.assert_array_equal(stream.launch(T), np.full(N, T))
        host.launch(T)
    _assert_equal(host, stream, f"placed {collav}")
    ev = _events(stream)
    assert ev[2][0] & abi.EV_TEST_OUTSIDE_MAP and ev[2][0] & abi.EV_TEST_STOP
    assert ev[3][0] & abi.EV_NONFINITE and ev[3][0] & abi.EV_TERMINAL
    assert not any((ev[i] & abi.EV_NONFINITE).any() for i in range(N) if i != 3)
    assert not (ev[3][1:] & abi.EV_NONFINITE).any()  # reset in place, then normal
    for sim in (host.sim, stream.sim):
        with pytest.raises(ShipSimNonFiniteError):
            sim.synchronize()
        sim.close()


FROZEN_SEED = 1  # (chosen with the oracle: see the assertion on its event bits below)


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
def test_frozen_obstacle_ship(collav):
    """Whole episodes (9 decisions): an obstacle ship that reaches the end of its route or leaves the map stops there
    (EV_OBS_STOP without EV_TERMINAL) while the ship under test sails on for some hundred ticks, so for the rest
    of the episode its position and its grid cell are held and only its time advances."""
    import oracle_ffi as O
    cfg = abi.ast_config(collav)
    N, n_dec = 8, cfg.max_sampling_frequency
    table = _table(2, n_dec, N, seed=FROZEN_SEED)
    # the CPU oracle's first episode of every env: the event bits of its last tick and its length
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


def test_policy_stream_moves_through_cells():
    """shipsim_run_policy, N = 8, hidden 64, deterministic: its logged actions replayed decision by decision
    through the host-driven step loop give the stream's records and final state."""
    from test_gpu_policy_act import _trainer
    from test_gpu_stream_reg_consts import _KEEP
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = abi.ast_config("none")  # (test_gpu_stream_reg_consts.py replays the sbmpc policy stream)
    N = 8
    sim = ShipSim(cfg, N)
    sim.reset()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    start = _pos(sim)
    far = np.zeros(2 * N)
    for _ in range(LAUNCHES):
        o = sim.run_policy(dp.weights(), T, N_DEC, ep, dec, deterministic=True, log=log, log_len=log_len)
        np.testing.assert_array_equal(o["ticks"].cpu().numpy(), np.full(N, T))
        far = np.maximum(far, _cells_between(start, _pos(sim)))
    assert far.min() >= 10, far
    ln = log_len.cpu().numpy()
    assert ln.min() >= 3 and ln.max() < CAP
    L = log.cpu().numpy()
    recs = [L[i, :ln[i]] for i in range(N)]
    n_eps = int(max(r[:, abi.DL_EPISODE].max() for r in recs)) + 2
    # the action of every decision the stream started: the logged ones and, past each env's last record, the one
    # still running at the end (its action is in its record row already)
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
    host = _HostLoop(cfg, N, table)
    for _ in range(LAUNCHES):
        host.launch(T)
    hs = host.records()
    for i in range(N):
        k = len(hs[i])
        assert 3 <= k <= ln[i] <= k + 8, (i, k, ln[i])
        np.testing.assert_array_equal(recs[i][:k][:, _KEEP], hs[i], err_msg=f"policy env {i}")
    _assert_state_equal(host, sim, ln, "policy")
    host.sim.close()
    sim.close()
