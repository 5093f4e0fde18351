"""Snapshot, restore and fork of env states on the device (shipsim_snapshot / shipsim_restore / shipsim_fork,
fork_gather_kernel).

Every test compares against a twin: a second handle, built the same way and driven with the same inputs, that is never
snapshotted or forked. The twin's launches are kept one by one (its decision records, ticks and decisions of every
launch, and every get_state field after it), so "env i continues as the twin's env j did from launch L" is a
comparison of bytes: records and fields alike. The first launch is 96 ticks and the others 128 (64 each on the
host-driven step path and for the raw ticks) with n_dec = 3 decisions per episode, so that envs are paused
mid-decision at the launch boundaries and episodes end and restart inside launches; the twin's run asserts both.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import weather_harness as WH
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv
from ast_sac_amd.shipsim import ShipSim, ShipSimError, Snapshot

pytestmark = pytest.mark.gpu

N_DEC = 3
FIRST = 96   # ticks of launch 1
TICKS = 128  # and of every other
CAP = 32
SHIP_FIELDS = tuple(range(abi.N_SHIP_FIELDS))
ENV_FIELDS = (abi.E_SAMPLING_COUNT, abi.E_TRAVEL_DIST, abi.E_TRAVEL_TIME, abi.E_ACC_REWARD, abi.E_N_BASE, abi.E_E_BASE,
              abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST)
SLOT_FIELDS = (abi.E_ROUTE_LEN, abi.E_ROUTE_NORTH, abi.E_ROUTE_EAST)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _copy(cfg, lpe=0):
    c = abi.Config.from_buffer_copy(cfg)
    c.lanes_per_env = lpe
    return c


def _own_or(src, n):
    """(indices with every out-of-range entry replaced by the env's own, mask of the in-range entries)."""
    s = np.asarray(src, dtype=np.int64).reshape(-1)
    ok = (s >= 0) & (s < n)
    return np.where(ok, s, np.arange(n)), ok


def _state(sim):
    """Every get_state field, per env, as bytes."""
    n, ns = sim.n_envs, sim.n_ships
    per_env = [[] for _ in range(n)]
    for f in SHIP_FIELDS + SLOT_FIELDS + ENV_FIELDS:
        a = sim.get(f).cpu().numpy().reshape(n, -1)
        assert a.shape[1] in (1, ns, ns * abi.MAX_ROUTE)
        for i in range(n):
            per_env[i].append(a[i].tobytes())
    return [tuple(x) for x in per_env]


class _Driver:
    """A handle and what its caller owns. advance() is one launch and returns, per env, what the launch reported;
    caller() / set_caller() save and put back the caller's arrays; fork_caller(src, saved) is the caller's side of
    fork(src[, source]): its arrays gathered like the envs (from the arrays saved with the snapshot, or its own), an
    out-of-range entry keeping what it has."""
    sim = None

    def state(self):
        return _state(self.sim)

    def close(self):
        self.sim.close()


class _StreamDriver(_Driver):
    def __init__(self, cfg, n, lpe=0, weather=None, seed=4242):
        self.env = BatchedMultiShipRLEnv(n_envs=n, cfg=_copy(cfg, lpe), weather=weather)
        self.sim, self.n = self.env.sim, n
        self.ep = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.dec = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.log = torch.zeros((n, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
        self.ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (4, N_DEC, n)).astype(np.float32)
        self.table = torch.from_numpy(abi.normalized_to_scoping(a)).cuda()
        self.sim.reset()

    def _launch(self, ticks):
        return self.sim.run_table(self.table, ticks, self.ep, self.dec, log=self.log, log_len=self.ln)

    def advance(self, ticks=TICKS):
        self.ln.zero_()
        out = self._launch(ticks)
        self.sim.synchronize()
        L, ln = self.log.cpu().numpy(), self.ln.cpu().numpy()
        t, d = out["ticks"].cpu().numpy(), out["decisions"].cpu().numpy()
        assert ln.max() <= CAP
        return [(int(t[i]), int(d[i]), L[i, :ln[i]].tobytes()) for i in range(self.n)]

    def caller(self):
        return self.ep.clone(), self.dec.clone()

    def set_caller(self, saved):
        self.ep.copy_(saved[0])
        self.dec.copy_(saved[1])

    def fork_caller(self, src, saved=None):
        idx, ok = _own_or(src, self.n)
        if saved is None:  # a fork from the live state: the facade's helper
            self.env.fork_stream_state(src, self.ep, self.dec)
        else:
            it, okt = torch.from_numpy(idx).cuda(), torch.from_numpy(ok).cuda()
            self.ep.copy_(torch.where(okt, saved[0][it], self.ep))
            self.dec.copy_(torch.where(okt, saved[1][it], self.dec))
        self.table = self.table[:, :, torch.from_numpy(idx).cuda()].contiguous()  # clone i gets its source's actions


class _PolicyDriver(_StreamDriver):
    def __init__(self, cfg, n, policy, **kw):
        super().__init__(cfg, n, **kw)
        self.policy = policy

    def _launch(self, ticks):
        return self.sim.run_policy(self.policy.weights(), ticks, N_DEC, self.ep, self.dec, deterministic=True,
                                   log=self.log, log_len=self.ln)


class _StepDriver(_Driver):
    """The host-driven shipsim_step path, max_ticks = 64: env i, awaiting its d-th decision, is given
    acts[d % 8][slot i]; an env that reports done is reset before the next call."""

    def __init__(self, cfg, n, lpe=0, seed=4242):
        self.sim, self.n = ShipSim(_copy(cfg, lpe), n), n
        a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (8, n)).astype(np.float32)
        self.acts = abi.normalized_to_scoping(a)
        self.count = np.zeros(n, np.int64)  # decisions completed by the env (the caller's array)
        self.slot = np.arange(n)            # whose action column the slot is given
        self.sim.reset()

    def advance(self, ticks=None):
        a = self.acts[self.count % 8, self.slot]
        out = self.sim.step(torch.from_numpy(a), max_ticks=64)
        self.sim.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        res = []
        for i in range(self.n):
            r = bool(o["ready"][i])
            res.append((int(o["ticks"][i]), r) + ((o["obs"][i].tobytes(), o["reward"][i].tobytes(), int(o["done"][i]),
                                                   int(o["events"][i])) if r else ()))
        ready = o["ready"].astype(bool)
        self.count += ready
        need = ready & o["done"].astype(bool)
        if need.any():
            self.sim.reset(mask=torch.from_numpy(need.astype(np.uint8)))
        return res

    def caller(self):
        return self.count.copy(), self.slot.copy()

    def set_caller(self, saved):
        self.count, self.slot = saved[0].copy(), saved[1].copy()

    def fork_caller(self, src, saved=None):
        idx, ok = _own_or(src, self.n)
        base = saved if saved is not None else self.caller()
        self.count = np.where(ok, base[0][idx], self.count)
        self.slot = np.where(ok, base[1][idx], self.slot)


class _TickDriver(_Driver):
    """Raw ticks of the NONIW / SINGLE kinds, 64 per launch, from perturbed initial states (the envs differ)."""

    def __init__(self, cfg, n, lpe=0, seed=4242):
        self.sim, self.n = ShipSim(_copy(cfg, lpe), n), n
        self.sim.reset()
        rng = np.random.Generator(np.random.PCG64(seed))
        S = n * self.sim.n_ships
        for f, spread in ((abi.F_NORTH, 150.0), (abi.F_EAST, 150.0), (abi.F_YAW, 0.15), (abi.F_U, 0.5)):
            self.sim.set(f, self.sim.get(f) + torch.from_numpy(rng.uniform(-spread, spread, S)).cuda())
        self.events = torch.zeros(n, dtype=torch.int32, device="cuda")

    def advance(self, ticks=None):
        noniw = self.sim.cfg.kind == abi.KIND_NONIW
        self.sim.tick(64, self.events if noniw else None)
        self.sim.synchronize()
        ev = self.events.cpu().numpy()
        return [(int(ev[i]),) for i in range(self.n)]

    def caller(self):
        return ()

    def set_caller(self, saved):
        pass

    def fork_caller(self, src, saved=None):
        pass


class _LegacyDriver(_TickDriver):
    """shipsim_legacy_step, 64 ticks per launch, collav simple: its collision check reads the previous step's
    states (legacy_states, and legacy_flags while they are still the float32 initial_states)."""

    def advance(self, ticks=None):
        out = self.sim.legacy_step(64)
        self.sim.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        return [(o["states"][i].tobytes(), int(o["done"][i]), int(o["status"][i])) for i in range(self.n)]


_policy = {}


def _device_policy():
    if not _policy:
        from test_gpu_policy_act import _trainer
        tr, _ = _trainer(64)
        _policy["tr"] = tr  # (kept alive: the device policy reads its parameters)
        _policy["dp"] = tr.device_policy(True)
    return _policy["dp"]


# shape name -> (driver factory(lpe=...), n_envs)
def _make(shape, n, lpe=0, weather=None):
    if shape == "sbmpc":
        return _StreamDriver(abi.ast_config("sbmpc"), n, lpe=lpe, weather=weather)
    if shape == "policy":
        return _PolicyDriver(abi.ast_config("sbmpc"), n, _device_policy(), lpe=lpe)
    if shape == "k3":
        return _StreamDriver(abi.ast_config("sbmpc", n_obs_ships=3), n, lpe=lpe)
    if shape == "none":
        return _StreamDriver(abi.ast_config("none"), n, lpe=lpe)
    if shape == "step":
        return _StepDriver(abi.ast_config("sbmpc"), n, lpe=lpe)
    if shape == "noniw":
        return _TickDriver(abi.c1_config("sbmpc"), n)
    if shape == "single":
        return _TickDriver(abi.c2_config(), n)
    if shape == "legacy":
        return _LegacyDriver(abi.ast_config("simple"), n)
    raise KeyError(shape)


_twins = {}


def _twin(shape, n, launches=5):
    """The twin's run, computed once per shape and shared: (reports[l][env] of launch l = 1.., states[l][env] after
    launch l), never snapshotted or forked."""
    if (shape, n) not in _twins:
        d = _make(shape, n)
        reports, states = [None], [d.state()]
        for l in range(launches):
            reports.append(d.advance(FIRST if l == 0 else TICKS))
            states.append(d.state())
        d.close()
        if isinstance(d, _StreamDriver):
            rec_bytes = abi.DECLOG_COLS * 8
            first = [len(reports[1][i][2]) // rec_bytes for i in range(n)]
            rows = [np.frombuffer(b"".join(reports[l][i][2] for l in range(1, launches + 1)), np.float64)
                    .reshape(-1, abi.DECLOG_COLS) for i in range(n)]
            # launch 1 leaves envs paused mid-decision: ticks run that belong to no completed decision
            assert any(reports[1][i][0] > sum(rows[i][:first[i], abi.DL_TICKS]) for i in range(n))
            # and episodes end (n_dec = 3) and restart inside the launches
            assert any(r[:, abi.DL_EPISODE].max() >= 1 for r in rows if len(r))
        # the envs differ: a fork that moved nothing would be seen
        assert len(set(states[1])) > 1 or shape == "policy"  # (one deterministic policy: every env sails alike)
        _twins[shape, n] = (reports, states)
    return _twins[shape, n]


def _assert_env(got_report, got_state, want_report, want_state, what):
    assert got_report == want_report, f"{what}: the launch's report (ticks, decisions, records)"
    for k, (a, b) in enumerate(zip(got_state, want_state)):
        assert a == b, f"{what}: get_state field #{k}"


PERM16 = [0, 1, 3, 4, 2, 6, 5] + [15 - i for i in range(9)]  # fixed points 0, 1; 3-cycle 2 3 4; swap 5 6; the rest mirrored
BROADCAST16 = [5] * 16


def _perm(n):
    """Two fixed points, a 3-cycle, a swap; what is left (n > 7) mirrored."""
    return [0, 1, 3, 4, 2, 6, 5] + [n - 1 - i for i in range(n - 7)]


def test_the_permutation_is_what_it_says():
    assert sorted(PERM16) == list(range(16)) and PERM16[:7] == [0, 1, 3, 4, 2, 6, 5]
    assert sorted(_perm(8)) == list(range(8))


# ---- 1. rewind ----------------------------------------------------------------------------------------------
def _rewind(shape, n, lpe=0, lpe_to=None, fresh=False):
    """Launch 1, snapshot, launches 2..4 (A); restore, launches 2..4 again (B): A == B == the twin. With lpe_to the
    snapshot goes into a fresh handle at that many lanes per env, which then runs launches 2..4; with `fresh` into
    a fresh handle as it comes."""
    reports, states = _twin(shape, n)
    d = _make(shape, n, lpe=lpe)
    assert d.advance(FIRST) == reports[1]
    snap = d.sim.snapshot()
    assert isinstance(snap, Snapshot) and snap.data.dtype == torch.uint8 and snap.data.numel() == d.sim.state_bytes
    assert (snap.kind, snap.n_envs, snap.n_ships) == (d.sim.cfg.kind, n, d.sim.n_ships)
    saved = d.caller()
    runs = []
    a = [d.advance() for _ in range(3)]
    runs.append((a, d.state()))
    if fresh:
        e = _make(shape, n)
    elif lpe_to is None:
        e = d
    else:
        e = _make(shape, n, lpe=lpe_to)  # reset, never stepped: the snapshot replaces all of it
        assert e.sim.lanes_per_env == lpe_to and d.sim.lanes_per_env == lpe
    e.sim.restore(snap)
    e.set_caller(saved)
    b = [e.advance() for _ in range(3)]
    runs.append((b, e.state()))
    for name, (rep, st) in zip("AB", runs):
        for l in range(3):
            for i in range(n):
                assert rep[l][i] == reports[2 + l][i], f"run {name}, launch {2 + l}, env {i}"
        for i in range(n):
            _assert_env(None, st[i], None, states[4][i], f"run {name}, env {i} after launch 4")
    d.close()
    if e is not d:
        e.close()


@pytest.mark.parametrize("shape", ["sbmpc", "policy"])
def test_rewind(shape):
    _rewind(shape, 8)


# ---- 2. broadcast, 3. permutation, 6. out of range: forks from the live state -----------------------------------
def _fork_live(shape, n, src, lpe=0):
    """Launch 1, fork(src), launches 2 and 3: env i reports and ends as the twin's env src[i] (its own where src[i]
    is out of range)."""
    reports, states = _twin(shape, n)
    d = _make(shape, n, lpe=lpe)
    assert d.advance(FIRST) == reports[1]
    d.fork_caller(src)
    d.sim.fork(src)
    idx, _ = _own_or(src, n)
    st = d.state()
    for i in range(n):  # the clone is in place before anything runs
        _assert_env(None, st[i], None, states[1][idx[i]], f"env {i} <- {idx[i]} at the fork")
    for l in (2, 3):
        rep = d.advance()
        st = d.state()
        for i in range(n):
            _assert_env(rep[i], st[i], reports[l][idx[i]], states[l][idx[i]], f"env {i} <- {idx[i]}, launch {l}")
    d.close()


def test_broadcast():
    _fork_live("sbmpc", 16, BROADCAST16)


def test_permutation():
    _fork_live("sbmpc", 16, PERM16)


def test_out_of_range_indices_leave_the_env_alone():
    n = 16
    src = [-1, n, 0, 1] + [(3 * i + 5) % n for i in range(4, n - 2)] + [2 ** 31 - 1, -2 ** 31]
    _fork_live("sbmpc", n, src)


# ---- 4. from an archive ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [PERM16, [-1, 16] + PERM16[2:]], ids=["permutation", "out-of-range"])
def test_fork_from_an_archived_snapshot(src):
    """Snapshot at launch 1, on to launch 3, then fork(src, source=snap): env i continues as the twin's env src[i]
    did from launch 1 — and an env whose index is out of range as itself from launch 3."""
    n = 16
    reports, states = _twin("sbmpc", n)
    d = _make("sbmpc", n)
    d.advance(FIRST)
    snap, saved = d.sim.snapshot(), d.caller()
    d.advance()
    assert d.advance() == reports[3]
    d.fork_caller(src, saved)
    d.sim.fork(src, source=snap)
    idx, ok = _own_or(src, n)
    for l in (1, 2):
        rep, st = d.advance(), d.state()
        for i in range(n):
            at = l + (1 if ok[i] else 3)
            _assert_env(rep[i], st[i], reports[at][idx[i]], states[at][idx[i]], f"env {i} <- {idx[i]}, launch +{l}")
    d.close()


def test_fork_without_indices_is_a_restore_or_nothing():
    n = 8
    reports, states = _twin("sbmpc", n)
    d = _make("sbmpc", n)
    d.advance(FIRST)
    snap, saved = d.sim.snapshot(), d.caller()
    d.advance()
    nbytes = d.sim.state_bytes
    d.sim._check(d.sim.L.shipsim_fork(d.sim.h, None, nbytes, None), "shipsim_fork")  # live, identity: nothing
    assert d.state() == states[2]
    d.sim._check(d.sim.L.shipsim_fork(d.sim.h, C.c_void_p(snap.data.data_ptr()), nbytes, None), "shipsim_fork")
    d.set_caller(saved)
    assert d.state() == states[1]
    assert d.advance() == reports[2]
    d.close()


def test_fork_and_snapshot_replayed_from_a_captured_graph():
    """Once the staging block exists (an identity fork allocates it and moves nothing), fork and snapshot are
    captured into a HIP graph: the capture runs nothing, every replay forks the state then held and snapshots the
    result, and the state block is where the graph's kernel arguments say it is."""
    n = 8
    src = _perm(n)
    reports, states = _twin("sbmpc", n)
    d = _make("sbmpc", n)
    assert d.advance(FIRST) == reports[1]
    d.sim.fork(list(range(n)))
    snap = d.sim.snapshot()
    s = torch.tensor(src, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d.sim.fork(s)
        d.sim.snapshot(out=snap)
    assert d.state() == states[1]
    d.fork_caller(src)
    g.replay()
    saved = d.caller()
    st = d.state()
    for i in range(n):
        _assert_env(None, st[i], None, states[1][src[i]], f"env {i} <- {src[i]} after the replay")
    first = d.advance()
    for i in range(n):
        assert first[i] == reports[2][src[i]], f"env {i} <- {src[i]}, launch 2"
    d.sim.restore(snap)  # (the snapshot the graph took after its fork)
    d.set_caller(saved)
    assert d.advance() == first
    d.close()


# ---- 5. shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["k3", "none", "noniw", "single", "step"])
def test_rewind_shapes(shape):
    _rewind(shape, 8)


@pytest.mark.parametrize("shape", ["k3", "none", "noniw", "single", "step"])
def test_permutation_shapes(shape):
    _fork_live(shape, 8, _perm(8))


@pytest.mark.parametrize("fresh", [False, True], ids=["same-handle", "fresh-handle"])
def test_rewind_legacy_step(fresh):
    """shipsim_legacy_step continues from a restored snapshot as it did: the legacy env's previous-step states and
    the flag that says whether they are still the float32 initial_states are part of the block (on a fresh handle
    that flag is set, in the snapshot it is not)."""
    _rewind("legacy", 8, fresh=fresh)


def test_permutation_legacy_step():
    _fork_live("legacy", 8, _perm(8))


def test_rewind_from_4_lanes_per_env_into_16():
    _rewind("sbmpc", 8, lpe=4, lpe_to=16)


def test_permutation_from_4_lanes_per_env_into_16():
    """The snapshot of a handle at 4 lanes per env forked, permuted, into a handle at 16."""
    n = 8
    src = _perm(n)
    reports, states = _twin("sbmpc", n)
    d = _make("sbmpc", n, lpe=4)
    d.advance(FIRST)
    snap, saved = d.sim.snapshot(), d.caller()
    e = _make("sbmpc", n, lpe=16)
    assert (d.sim.lanes_per_env, e.sim.lanes_per_env) == (4, 16)
    e.fork_caller(src, saved)
    e.sim.fork(src, source=snap)
    for l in (2, 3):
        rep, st = e.advance(), e.state()
        for i in range(n):
            _assert_env(rep[i], st[i], reports[l][src[i]], states[l][src[i]], f"env {i} <- {src[i]}, launch {l}")
    d.close()
    e.close()


# ---- 7. weather -------------------------------------------------------------------------------------------------
def _weather_run(n, cfg, weather, src=None, mode="keep", source=None):
    """A handle of `cfg` under per-env `weather` (None: the config's, a uniform handle): launch 1, then — with
    src — the fork, then launches 2 and 3. With `source` = (snapshot, caller arrays saved with it) the handle forks
    from that instead of running launch 1. Returns the two launches' (report, state), the (snapshot, caller arrays)
    taken after launch 1, and the weather in force at the end."""
    d = _StreamDriver(cfg, n, weather=weather)
    at_fork = None
    if source is None:
        d.advance(FIRST)
        if src is not None:
            at_fork = (d.sim.snapshot(), d.caller())
            d.fork_caller(src)
            d.env.fork(src, weather=mode)
    else:
        d.fork_caller(src, source[1])
        d.env.fork(src, source=source[0])
    out = [(d.advance(), d.state()) for _ in range(2)]
    w = d.env.weather()
    d.close()
    return out, at_fork, w


def test_fork_under_per_env_weather_keep_and_follow():
    n = 8
    cfg = abi.ast_config("sbmpc")
    ws = WH.four_weathers(cfg)
    weather = WH.interleaved(ws, n)
    src = _perm(n)  # (moves envs between weathers: src[i] % 4 != i % 4 for most i)
    assert sum(s % 4 != i % 4 for i, s in enumerate(src)) >= 4
    twin, _, _ = _weather_run(n, cfg, weather)
    # follow: the weather moves with the state, so env i is the twin's env src[i]
    got, _, w = _weather_run(n, cfg, weather, src, "follow")
    for k in WH.KEYS:
        np.testing.assert_array_equal(w[k], weather[k][src])
    for l in range(2):
        for i in range(n):
            _assert_env(got[l][0][i], got[l][1][i], twin[l][0][src[i]], twin[l][1][src[i]], f"follow, env {i}")
    # keep: env i runs on under slot i's weather — as a uniform handle whose config carries that weather does
    # from the same cloned state
    got, at_fork, w = _weather_run(n, cfg, weather, src, "keep")
    for k in WH.KEYS:
        np.testing.assert_array_equal(w[k], weather[k])
    uniform = [_weather_run(n, WH.cfg_with(cfg, ws[j]), None, src, source=at_fork)[0] for j in range(4)]
    for l in range(2):
        for i in range(n):
            u = uniform[i % 4][l]
            _assert_env(got[l][0][i], got[l][1][i], u[0][i], u[1][i], f"keep, env {i} under weather {i % 4}")
    # the weathers matter: some clone that changed weather no longer runs as its source does
    assert any(got[1][1][i] != twin[1][1][src[i]] for i in range(n) if src[i] % 4 != i % 4)


# ---- 8. refusals ------------------------------------------------------------------------------------------------
def test_refusals():
    n = 4
    sim = ShipSim(abi.ast_config("sbmpc"), n)
    nbytes = sim.state_bytes
    assert nbytes > 0 and nbytes % 256 == 0
    buf = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    p, ip = C.c_void_p(buf.data_ptr()), C.c_void_p(idx.data_ptr())
    L, h = sim.L, sim.h

    def refused(rc, code, word):
        assert rc == code, (rc, L.shipsim_last_error(h))
        assert word in L.shipsim_last_error(h).decode(), L.shipsim_last_error(h)

    # before the first reset: no snapshot, no fork from the live state
    refused(L.shipsim_snapshot(h, p, nbytes), -3, "before reset")
    refused(L.shipsim_fork(h, None, nbytes, ip), -3, "before reset")
    with pytest.raises(ShipSimError, match="before reset"):
        sim.snapshot()
    sim.reset()
    # another size
    for wrong in (nbytes - 256, nbytes + 256, 0, -1):
        refused(L.shipsim_snapshot(h, p, wrong), -1, "bytes")
        refused(L.shipsim_restore(h, p, wrong), -1, "bytes")
        refused(L.shipsim_fork(h, p, wrong, ip), -1, "bytes")
        refused(L.shipsim_fork(h, None, wrong, ip), -1, "bytes")
    # no buffer
    refused(L.shipsim_snapshot(h, None, nbytes), -1, "NULL")
    refused(L.shipsim_restore(h, None, nbytes), -1, "NULL")
    # a recording handle
    sim.set_trajectory(16)
    refused(L.shipsim_snapshot(h, p, nbytes), -1, "trajectory recording")
    refused(L.shipsim_restore(h, p, nbytes), -1, "trajectory recording")
    refused(L.shipsim_fork(h, None, nbytes, ip), -1, "trajectory recording")
    refused(L.shipsim_fork(h, p, nbytes, ip), -1, "trajectory recording")
    with pytest.raises(ShipSimError, match="trajectory recording"):
        sim.fork(idx)
    sim.clear_trajectory()
    snap = sim.snapshot()
    # a Snapshot of another shape is refused before the library is called
    for other in (ShipSim(abi.ast_config("sbmpc"), n + 1), ShipSim(abi.ast_config("sbmpc", n_obs_ships=2), n),
                  ShipSim(abi.c1_config("sbmpc"), n)):
        for call in (lambda: other.restore(snap), lambda: other.fork(list(range(other.n_envs)), source=snap)):
            with pytest.raises(ShipSimError, match=r"\(kind, n_envs, n_ships\)"):
                call()
        other.close()
    with pytest.raises(ShipSimError, match="another build"):
        sim.restore(Snapshot(snap.data, snap.kind, snap.n_envs, snap.n_ships, "some other build"))
    with pytest.raises(ShipSimError, match="entries"):
        sim.fork([0] * (n + 1))
    with pytest.raises(ValueError, match="keep"):
        BatchedMultiShipRLEnv.fork(None, [0], weather="drift")
    # onto a fresh handle a snapshot is welcome, and marks it reset
    fresh = ShipSim(abi.ast_config("sbmpc"), n)
    fresh.restore(snap)
    assert _state(fresh) == _state(sim)
    fresh.snapshot()
    fresh.close()
    sim.close()
