"""Per-env weather that moves with the state on the device (shipsim_weather_store / _load / _fork,
weather_gather_kernel; fork / split under weather="carry", Snapshot and StateArchive with weather): the gather
against the numpy restatement tests/weather_carry_ref.py, "carry" against the host-side "follow", snapshots and
archives against twins that never changed, graph capture, the refusals. Everything is compared bit for bit.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import archive_ref as A
import weather_carry_ref as R
import weather_harness as WH
from ast_sac_amd import shipsim
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv
from ast_sac_amd.shipsim import ShipSim, ShipSimError, Snapshot, StateArchive

pytestmark = pytest.mark.gpu

N_DEC = 3
CAP = 32
FIRST, TICKS = 96, 128  # launch 1 leaves envs paused mid-decision; episodes end and restart inside the launches
EINVAL = -1
SEED = 0x1234ABCD5678EF01


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _i32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64).astype(np.int32), device="cuda")


def _own_or(src, n):
    s = np.asarray(src, dtype=np.int64).reshape(-1)
    ok = (s >= 0) & (s < n)
    return np.where(ok, s, np.arange(n)), ok


def _same(got, want, what=""):
    """Two weather dicts, bit for bit."""
    assert set(got) == set(want) == set(R.KEYS)
    for k in R.KEYS:
        np.testing.assert_array_equal(np.asarray(got[k]).view(np.uint64), np.asarray(want[k]).view(np.uint64),
                                      err_msg=f"{what}: {k}")


# ---- 1. the gather, no env launch beyond the reset -------------------------------------------------------------------
def _raw(sim):
    """The handle's six-row table, through an identity store."""
    buf = torch.full((R.ROWS, sim.n_envs), -7.0, dtype=torch.float64, device="cuda")
    sim._follow_stream()
    sim._weather_store(buf, None)
    sim.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("n", [300, 5])
def test_gather_equals_the_numpy_restatement(n):
    """fork, store into 7 and into 1000 slots and load back, over the index sets of the CPU test: weather() on all
    four keys, and the raw six rows (sin and cos permute with the rest), equal the numpy restatement."""
    w0 = R.random_weather(n, 2026 + n)
    sim = ShipSim(abi.ast_config("sbmpc"), n)
    sim.set_weather(*[w0[k] for k in R.KEYS])
    sim.reset()
    _same(sim.weather(), w0, "a handle that never carried returns what it was given")
    t0 = _raw(sim)
    assert t0.tobytes() == R.table(w0).tobytes()  # the table as set: five rows for the kernels, then the direction
    _same(sim.weather(), w0, "read back from the device")

    def put_back():
        sim.set_weather(*[w0[k] for k in R.KEYS])
        assert _raw(sim).tobytes() == t0.tobytes()

    # fork in place
    for name, idx in R.index_sets(n, n).items():
        sim.fork(idx, weather=True)
        want = R.fork(t0, idx)
        _same(sim.weather(), R.keys_of(want), f"fork {name}")
        assert _raw(sim).tobytes() == want.tobytes(), f"fork {name}: the six rows"
        put_back()
    # store into m slots, load back
    for m in (7, 1000):
        nbytes = int(sim.L.shipsim_weather_bytes(m))
        assert nbytes == R.ROWS * m * 8
        stale = R.table(R.random_weather(m, 99 + m))
        loads = R.index_sets(n, m)
        for name, idx in R.index_sets(m, n).items():
            buf = torch.from_numpy(stale).cuda()
            sim._weather_store(buf, _i32(idx))
            cells = R.gather(t0, idx, stale)
            sim.synchronize()
            assert buf.cpu().numpy().tobytes() == cells.tobytes(), f"store {name} into {m} slots"
            _same(sim.weather(), w0, "a store leaves the handle's weather alone")
            back = loads[name if name in loads else "duplicates"]
            sim._weather_load(buf, _i32(back))
            want = R.gather(cells, back, t0)
            _same(sim.weather(), R.keys_of(want), f"load {name} from {m} slots")
            assert _raw(sim).tobytes() == want.tobytes(), f"load {name} from {m} slots: the six rows"
            put_back()
    # n_slots == n_envs: a buffer is the table; a fork from a weather snapshot, and a restore
    snap = torch.from_numpy(t0).cuda()
    other = R.random_weather(n, 4)
    sim.set_weather(*[other[k] for k in R.KEYS])
    idx = R.index_sets(n, n)["out_of_range"]
    sim._weather_load(snap, _i32(idx))
    assert _raw(sim).tobytes() == R.gather(t0, idx, R.table(other)).tobytes()
    sim._weather_load(snap, None)
    assert _raw(sim).tobytes() == t0.tobytes()
    sim.close()


# ---- a handle on a table stream and what its caller owns -----------------------------------------------------------
class _Stream:
    def __init__(self, cfg, n, weather, seed=777):
        self.env = BatchedMultiShipRLEnv(n_envs=n, cfg=abi.Config.from_buffer_copy(cfg), weather=weather)
        self.sim, self.n = self.env.sim, n
        self.ep = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.dec = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.log = torch.zeros((n, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
        self.ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (4, N_DEC, n)).astype(np.float32)
        self.table = torch.from_numpy(abi.normalized_to_scoping(a)).cuda()
        self.sim.reset()

    def report(self, out):
        self.sim.synchronize()
        L, ln = self.log.cpu().numpy(), self.ln.cpu().numpy()
        t, d = out["ticks"].cpu().numpy(), out["decisions"].cpu().numpy()
        assert ln.max() <= CAP
        return [(int(t[i]), int(d[i]), L[i, :ln[i]].tobytes()) for i in range(self.n)]

    def advance(self, ticks=TICKS):
        self.ln.zero_()
        return self.report(self.sim.run_table(self.table, ticks, self.ep, self.dec, log=self.log, log_len=self.ln))

    def state(self):
        """The state block, one bytes object per env."""
        return A.per_env_bytes(self.sim.snapshot().data.cpu().numpy(), self.n, self.sim.n_ships)

    def caller(self):
        return self.ep.clone(), self.dec.clone(), self.table.clone()

    def set_caller(self, saved):
        self.ep.copy_(saved[0])
        self.dec.copy_(saved[1])
        self.table = saved[2].clone()

    def fork_caller(self, src, saved=None):
        """The caller's side of a fork: env i goes on at its source's place in the episode with its source's
        actions (from the arrays saved with a snapshot, or its own); an out-of-range entry keeps what it has."""
        idx, ok = _own_or(src, self.n)
        ep, dec, table = saved if saved is not None else self.caller()
        it, okt = torch.from_numpy(idx).cuda(), torch.from_numpy(ok).cuda()
        self.ep.copy_(torch.where(okt, ep[it], self.ep))
        self.dec.copy_(torch.where(okt, dec[it], self.dec))
        self.table = torch.where(okt, table[:, :, it], self.table).contiguous()

    def close(self):
        self.env.close()


def _shape(name):
    """(config, n_envs, per-env weather: four weathers interleaved, so that neighbours never share one)"""
    cfg, n = (abi.ast_config("sbmpc"), 64) if name == "two_ship" else (abi.ast_config("sbmpc", n_obs_ships=2), 16)
    ws = WH.four_weathers(cfg)
    return cfg, n, WH.interleaved(ws, n)


def _sources(n):
    perm = [(5 * i + 3) % n for i in range(n)]  # 5 is odd and n a power of two: a permutation; i % 4 -> (i + 3) % 4
    mixed = [(7 * i + 1) % n for i in range(n)]
    for j, bad in enumerate((-1, n, R.INT32_MIN, R.INT32_MAX, -5, n + 64)):
        mixed[(3 * j + 1) % n] = bad
    return {"permutation": perm, "broadcast": [n // 2 + 1] * n, "mixed": mixed}


# ---- 2. carry equals follow -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["permutation", "broadcast", "mixed"])
@pytest.mark.parametrize("shape", ["two_ship", "k2"])
def test_carry_equals_follow(shape, kind):
    """One table launch, fork(src, weather=mode), a second launch: the decision records, the state block's bytes and
    weather() under "carry" are those under "follow", the host-side move."""
    cfg, n, weather = _shape(shape)
    src = _sources(n)[kind]
    idx, ok = _own_or(src, n)
    if kind == "permutation":
        assert sorted(src) == list(range(n)) and all(s % 4 != i % 4 for i, s in enumerate(src))
    if kind == "mixed":
        assert 0 < (~ok).sum() < n
    runs = {}
    for mode in ("carry", "follow"):
        d = _Stream(cfg, n, weather)
        first = d.advance(FIRST)
        d.fork_caller(src)
        d.env.fork(src, weather=mode)
        runs[mode] = (first, d.advance(), d.state(), d.env.weather())
        d.close()
    c, f = runs["carry"], runs["follow"]
    assert c[0] == f[0]
    _same(f[3], {k: weather[k][idx] for k in R.KEYS}, "follow")
    _same(c[3], f[3], "carry")
    assert any(not np.array_equal(c[3][k], weather[k]) for k in R.KEYS)  # weather did move
    for i in range(n):
        assert c[1][i] == f[1][i], f"env {i} <- {src[i]}: ticks, decisions, records of the launch after the fork"
        assert c[2][i] == f[2][i], f"env {i} <- {src[i]}: state bytes"
    assert kind == "broadcast" or len(set(c[2])) > n // 2  # (a broadcast: one state, weather and table column)


# ---- 3. a snapshot with weather --------------------------------------------------------------------------------------
def test_snapshot_restore_and_fork_with_the_snapshots_weather():
    cfg, n, weather = _shape("two_ship")
    n = 16
    weather = {k: v[:n] for k, v in weather.items()}
    other = {k: np.roll(v, 1) for k, v in weather.items()}  # every env under its neighbour's weather
    twin = _Stream(cfg, n, weather)
    twin.advance(FIRST)
    want, want_state = twin.advance(), twin.state()
    twin.close()

    d = _Stream(cfg, n, weather)
    d.advance(FIRST)
    snap, saved = d.env.snapshot(weather=True), d.caller()
    assert snap.weather.shape == (R.ROWS, n) and snap.weather.dtype == torch.float64
    assert snap.weather.cpu().numpy().tobytes() == R.table(weather).tobytes()
    kept = snap.clone()
    assert kept.weather.data_ptr() != snap.weather.data_ptr() and torch.equal(kept.weather, snap.weather)
    d.env.set_weather(other)
    strayed = d.advance()
    assert strayed != want  # the weathers matter
    d.env.restore(snap, weather=True)
    d.set_caller(saved)
    _same(d.env.weather(), weather, "restore")
    assert d.advance() == want and d.state() == want_state
    # without weather=True the weather stays as it is
    d.env.set_weather(other)
    d.env.restore(snap)
    _same(d.env.weather(), other, "restore without weather")
    d.close()

    # a fork from the snapshot under "carry" takes the weather of the snapshot's time, on another env object
    src = _sources(n)["mixed"]
    idx, ok = _own_or(src, n)
    e = _Stream(cfg, n, other)
    e.advance(FIRST)
    own_state = e.state()
    e.fork_caller(src, saved)
    e.env.fork(src, source=kept, weather="carry")
    _same(e.env.weather(), {k: np.where(ok, weather[k][idx], other[k]) for k in R.KEYS}, "fork from a snapshot")
    at_fork = e.state()
    got, got_state = e.advance(), e.state()
    for i in range(n):
        if ok[i]:
            assert got[i] == want[src[i]] and got_state[i] == want_state[src[i]], f"env {i} <- {src[i]}"
        else:
            assert at_fork[i] == own_state[i], f"env {i} was left alone"
    e.close()


# ---- 4. an archive with weather --------------------------------------------------------------------------------------
def test_archive_with_weather():
    """32 envs, 7 cells: update(cell, score) elects and stores state and weather, the envs run on, load(cell_of_env)
    with duplicates and -1: env i continues as the stored env did, under the stored weather — as a twin does that
    forks under "follow" from a snapshot taken at the store."""
    cfg = abi.ast_config("sbmpc")
    n, m = 32, 7
    weather = WH.interleaved(WH.four_weathers(cfg), n)
    d, t = _Stream(cfg, n, weather), _Stream(cfg, n, weather)
    assert d.advance(64) == t.advance(64)
    arch = d.env.archive(m, weather=True)
    assert isinstance(arch, StateArchive) and arch.weather.shape == (R.ROWS, m) and not arch.weather.any()
    g = np.random.Generator(np.random.PCG64(5))
    cell = (np.arange(n) * 3) % (m + 1) - 1  # -1: no candidate; cells 0..6 named by several envs each
    cell[cell == 4] = -1  # cell 4 stays empty
    score = g.normal(size=n)
    env_of_cell, n_improved = arch.update(_i32(cell), torch.from_numpy(score).cuda(),
                                          carry=dict(ep=d.ep, dec=d.dec, actions=d.table.permute(2, 0, 1).contiguous()))
    env_of_cell = env_of_cell.cpu().numpy().astype(np.int64)
    want_eoc = np.array([max((i for i in range(n) if cell[i] == c), key=lambda i: (score[i], -i), default=-1)
                         for c in range(m)])
    np.testing.assert_array_equal(env_of_cell, want_eoc)
    assert int(n_improved.cpu()[0]) == 6 and env_of_cell[4] == -1
    snap, saved = t.sim.snapshot(), t.caller()  # the twin's snapshot at the store
    assert arch.weather.cpu().numpy().tobytes() == R.gather(R.table(weather), env_of_cell, np.zeros((R.ROWS, m))).tobytes()
    assert arch.as_snapshot().weather is arch.weather
    assert d.advance() == t.advance()  # both run on
    cell_of_env = np.array([(5 * i) % m for i in range(n)])  # duplicates; cell 4 is empty: never loaded below
    cell_of_env[cell_of_env == 4] = -1
    cell_of_env[[0, 9, 31]] = (-1, m, R.INT32_MAX)
    ok = (cell_of_env >= 0) & (cell_of_env < m)
    src = np.where(ok, env_of_cell[np.clip(cell_of_env, 0, m - 1)], -1)
    assert ok.sum() > n // 2 and (~ok).sum() >= 3 and len(set(src[ok])) >= 5
    actions = d.table.permute(2, 0, 1).contiguous()
    arch.load(_i32(cell_of_env), carry=dict(ep=d.ep, dec=d.dec, actions=actions))
    d.table = actions.permute(1, 2, 0).contiguous()
    t.fork_caller(src, saved)
    t.env.fork(src, source=snap, weather="follow")
    w = d.env.weather()
    _same(w, {k: np.where(ok, weather[k][np.clip(src, 0, n - 1)], weather[k]) for k in R.KEYS}, "archive load")
    _same(w, t.env.weather(), "the twin's")
    assert any(not np.array_equal(w[k], weather[k]) for k in R.KEYS)
    assert torch.equal(d.ep, t.ep) and torch.equal(d.dec, t.dec) and torch.equal(d.table, t.table)
    assert d.state() == t.state()
    got, want = d.advance(), t.advance()
    end_d, end_t = d.state(), t.state()
    for i in range(n):
        assert got[i] == want[i], f"env {i} <- cell {cell_of_env[i]} <- env {src[i]}: ticks, decisions, records"
        assert end_d[i] == end_t[i], f"env {i} <- cell {cell_of_env[i]} <- env {src[i]}: state bytes"
    d.close()
    t.close()


# ---- 5. capture ------------------------------------------------------------------------------------------------------
def test_split_under_carry_and_a_launch_in_one_graph():
    """split(..., weather="carry") and a table launch captured into one (linear) graph, replayed twice with an
    advanced counter: records and weather() equal those of a twin that splits eagerly under "follow" — no host call
    of the replays touches weather, so this also pins shipsim_get_weather's read back from the device."""
    cfg, n = abi.ast_config("sbmpc"), 16
    weather = WH.interleaved(WH.four_weathers(cfg), n)
    d, t = _Stream(cfg, n, weather), _Stream(cfg, n, weather)
    assert d.advance(FIRST) == t.advance(FIRST)
    w = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    pot = torch.exp(-d.sim.level_distance() / 4000.0)
    pot[::3] *= 1e-3  # some envs all but starved, so that slots change hands
    ctr = torch.tensor([1], dtype=torch.int64, device="cuda")
    # eager once: the resampler's workspace and the state fork's staging block exist before the capture (an identity
    # fork moves nothing); the weather calls need nothing of the kind
    shipsim.resample(w, pot, SEED, ctr)
    d.sim.fork(list(range(n)))
    out = dict(ticks=torch.zeros(n, dtype=torch.int32, device="cuda"),
               decisions=torch.zeros(n, dtype=torch.int32, device="cuda"))
    before = d.state()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            src, wout, total, status = d.env.split(w, pot, SEED, ctr, d.ep, d.dec, weather="carry")
            d.sim.run_table(d.table, TICKS, d.ep, d.dec, out=out, log=d.log, log_len=d.ln)
    torch.cuda.synchronize()
    assert d.state() == before  # the capture ran nothing
    _same(d.env.weather(), weather, "after the capture")
    moved = False
    for value in (7, 2 ** 33 + 1):
        ctr.fill_(value)
        d.ln.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got, got_w, got_src = d.report(out), d.env.weather(), src.cpu().numpy().copy()
        es, ew, _, est = t.env.split(w, pot, SEED, torch.tensor([value], dtype=torch.int64, device="cuda"), t.ep, t.dec,
                                     weather="follow")
        want, want_w = t.advance(), t.env.weather()
        np.testing.assert_array_equal(got_src, es.cpu().numpy())
        np.testing.assert_array_equal(wout.cpu().numpy().view(np.uint64), ew.cpu().numpy().view(np.uint64))
        assert int(status.cpu()[0]) == int(est.cpu()[0]) == 0
        _same(got_w, want_w, f"counter {value}")
        assert got == want, f"counter {value}: ticks, decisions, records"
        assert d.state() == t.state()
        moved = moved or any(got_src[i] % 4 != i % 4 for i in range(n))
    assert moved  # some clone landed in a slot of another weather
    assert any(not np.array_equal(got_w[k], weather[k]) for k in R.KEYS)
    d.close()
    t.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages():
    n = 8
    sim = ShipSim(abi.ast_config("sbmpc"), n)
    sim.reset()
    L, h = sim.L, sim.h
    nbytes = int(L.shipsim_weather_bytes(n))
    buf = torch.zeros(nbytes // 8 + 8, dtype=torch.float64, device="cuda")
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    p, ip = C.c_void_p(buf.data_ptr()), C.c_void_p(idx.data_ptr())
    assert buf.data_ptr() % 16 == 0

    def refused(rc, word):
        assert rc == EINVAL, (rc, L.shipsim_last_error(h))
        assert word in L.shipsim_last_error(h).decode(), L.shipsim_last_error(h)

    assert L.shipsim_weather_bytes(0) == L.shipsim_weather_bytes(abi.ARCHIVE_MAX_CELLS + 1) == EINVAL
    # a handle without per-env weather in force: never set, or cleared
    for _ in range(2):
        refused(L.shipsim_weather_store(h, p, nbytes, n, ip), "no per-env weather")
        refused(L.shipsim_weather_load(h, p, nbytes, n, ip), "no per-env weather")
        refused(L.shipsim_weather_fork(h, ip), "no per-env weather")
        with pytest.raises(ShipSimError, match="per-env weather"):
            sim.fork(idx, weather=True)
        with pytest.raises(ShipSimError, match="per-env weather"):
            sim.snapshot(weather=True)
        with pytest.raises(ShipSimError, match="per-env weather"):
            StateArchive(sim, 7, weather=True)
        with pytest.raises(ShipSimError, match="per-env weather"):
            sim.archive(7, weather=True)
        sim.set_weather(1.0, 0.5, 0.1, -0.1)
        sim.clear_weather()
    bare = sim.snapshot()
    assert bare.weather is None
    sim.set_weather(np.arange(n) * 1.0, 0.5, 0.1, -0.1)
    given = sim.weather()
    for call in (L.shipsim_weather_store, L.shipsim_weather_load):
        refused(call(h, None, nbytes, n, ip), "buffer is NULL")
        for wrong in (nbytes - 8, nbytes + 8, 0, -1, nbytes * 5 // 6):
            refused(call(h, p, wrong, n, ip), "bytes")
        refused(call(h, C.c_void_p(buf.data_ptr() + 8), nbytes, n, ip), "16-byte aligned")
        for bad in (0, -1, abi.ARCHIVE_MAX_CELLS + 1):
            refused(call(h, p, nbytes, bad, ip), "n_slots")
        refused(call(h, p, int(L.shipsim_weather_bytes(7)), 7, None), "NULL index")
        refused(call(h, p, int(L.shipsim_weather_bytes(n + 1)), n + 1, None), "NULL index")
        assert call(h, p, nbytes, n, None) == 0  # the identity
    assert L.shipsim_weather_fork(h, None) == 0
    sim.synchronize()
    _same(sim.weather(), given, "nothing refused moved anything")
    # a source without weather is refused before the library is called
    with pytest.raises(ShipSimError, match="carries no weather"):
        sim.restore(bare, weather=True)
    with pytest.raises(ShipSimError, match="carries no weather"):
        sim.fork(idx, source=bare, weather=True)
    with pytest.raises(ShipSimError, match="carries no weather"):
        sim.snapshot(out=bare, weather=True)
    env = BatchedMultiShipRLEnv(n_envs=n, cfg=abi.ast_config("sbmpc"), weather=given)
    env.reset()
    with pytest.raises(ValueError, match="carries no weather"):
        env.fork(idx, source=Snapshot(bare.data, bare.kind, bare.n_envs, bare.n_ships, bare.build), weather="carry")
    with pytest.raises(ValueError, match="'keep', 'follow' or 'carry'"):
        env.fork(idx, weather="drift")
    env.close()
    # an archive that carries weather refuses a uniform handle
    arch = sim.archive(7, weather=True)
    uniform = ShipSim(abi.ast_config("sbmpc"), n)
    uniform.reset()
    with pytest.raises(ShipSimError, match="no per-env weather"):
        arch.store([0] * 7, sim=uniform)
    # without per-env weather "carry" has nothing to move, as "follow": a plain fork
    plain = BatchedMultiShipRLEnv(n_envs=n, cfg=abi.ast_config("sbmpc"))
    plain.reset()
    plain.fork(list(range(n)), weather="carry")
    assert plain.weather() is None
    plain.close()
    uniform.close()
    sim.close()


# ---- 7. a handle that never carries ----------------------------------------------------------------------------------
def test_a_handle_that_never_carries_returns_what_it_was_given():
    """(with the existing weather suite, unedited) "keep" and the uniform path: weather() is the host copy of what
    was set, whatever forks in between."""
    n = 8
    w0 = R.random_weather(n, 1)
    env = BatchedMultiShipRLEnv(n_envs=n, cfg=abi.ast_config("sbmpc"), weather=w0)
    env.reset()
    env.fork([(i + 1) % n for i in range(n)], weather="keep")
    env.sim.synchronize()
    _same(env.weather(), w0, "keep")
    env.set_weather(None)
    assert env.weather() is None
    env.close()
