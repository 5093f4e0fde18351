"""The two-slot, 16-lane decision streams (shipsim_run_table / shipsim_run_policy, detailed machinery) keep their
launch constants in accumulator registers for the whole launch: each lane's copy is written once at the kernel's
entry and read back where the tick uses it. The sliced shipsim_step kernels do not (they re-read the kernarg segment
and LDS), so the host-driven step loop is an independent reference. Every comparison is bit for bit: decision
records (reward, events, done, episode, decision, ticks, observation), per-launch tick counts and the final ship
state.
  1. partial waves and per-lane ship constants: 5 and 9 envs at 3 envs per wave (one env alone in the last wave,
     idle lanes beside it), three 700-tick launches whose boundaries fall mid-decision, in-kernel episode resets;
  2. the constants belong to the launch, not to the process: two handles alive at once whose configs differ in dt
     (4 s and 5 s: 1 / dt not a power of two), wind, current and radius of acceptance, their launches alternating;
  3. the policy stream: its logged actions replayed through the host-driven step loop.
Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim

pytestmark = pytest.mark.gpu

_KEEP = [abi.DL_REWARD, abi.DL_EVENTS, abi.DL_DONE, abi.DL_EPISODE, abi.DL_DECISION, abi.DL_TICKS] + \
    list(range(abi.DL_OBS, abi.DL_OBS + 8))
_STATE = [abi.F_NORTH, abi.F_EAST, abi.F_YAW, abi.F_U, abi.F_V, abi.F_R, abi.F_OMEGA, abi.F_TIME]
T, LAUNCHES, N_DEC, CAP = 700, 3, 3, 256  # (3 decisions per episode: every env resets in the kernel several times)


def _table(n_eps, n_dec, N, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return abi.normalized_to_scoping(g.uniform(-1, 1, (n_eps, n_dec, N)).astype(np.float32))


def _state(sim):
    return np.stack([sim.get(f).cpu().numpy().astype(np.float64) for f in _STATE], 1)


class _HostLoop:
    """The host-driven reference of one handle, advanced launch by launch: shipsim_step slices (every env to exactly
    `T` more ticks, by its own count) and masked shipsim_reset between them; an env's action is table[ep, dec]."""

    def __init__(self, cfg, N, table):
        self.sim = ShipSim(cfg, N)
        self.sim.reset()
        self.N, self.table = N, table  # table: (n_eps, n_dec, N) float32 numpy
        self.ep = np.zeros(N, int)
        self.dec = np.zeros(N, int)
        self.total = np.zeros(N, int)
        self.dticks = np.zeros(N, int)
        self.recs = [[] for _ in range(N)]
        self.target = 0

    def launch(self, ticks):
        self.target += ticks
        n_eps, n_dec = self.table.shape[:2]
        ar = np.arange(self.N)
        for _ in range(100 * ticks):
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
                self.recs[i].append(np.concatenate([[o["reward"][i], float(ev[i]), float(o["done"][i]),
                                                     self.ep[i], self.dec[i], self.dticks[i]], o["obs"][i].astype(np.float64)]))
            end = ready & ((o["done"] != 0) | (self.dec + 1 >= n_dec))
            self.dec += ready
            self.dec[end] = 0
            self.ep += end
            self.dticks[ready] = 0
            self.sim.reset(mask=torch.from_numpy(end.astype(np.uint8)).cuda())
        raise AssertionError("host loop did not reach the launch's tick count")

    def records(self):
        return [np.array(r).reshape(-1, len(_KEEP)) for r in self.recs]


class _Stream:
    """The same handle configuration on the decision stream: run_table launches of `T` ticks, every decision logged."""

    def __init__(self, cfg, N, table):
        self.sim = ShipSim(cfg, N)
        self.sim.reset()
        self.N = N
        self.table = torch.from_numpy(table).cuda()
        self.ep = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.dec = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.log = torch.zeros((N, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
        self.log_len = torch.zeros(N, dtype=torch.int32, device="cuda")

    def launch(self, ticks):
        o = self.sim.run_table(self.table, ticks, self.ep, self.dec, log=self.log, log_len=self.log_len)
        return o["ticks"].cpu().numpy()

    def records(self):
        ln = self.log_len.cpu().numpy()
        assert ln.max() < CAP
        L = self.log.cpu().numpy()
        return [L[i, :ln[i]][:, _KEEP] for i in range(self.N)]


def _assert_equal(host, stream, what):
    hs, ss = host.records(), stream.records()
    n = 0
    for i in range(host.N):
        # a decision that completed on the launch's last tick and failed its next sampling at once is one record
        # ahead in the stream (it starts the next decision inside the launch): the host loop's are a prefix
        k = len(hs[i])
        assert k >= 3 and k <= len(ss[i]) <= k + 8, (what, i, k, len(ss[i]))
        np.testing.assert_array_equal(ss[i][:k], hs[i], err_msg=f"{what} env {i}")
        n += k
    _assert_state_equal(host, stream.sim, [len(x) for x in ss], what)
    return n


def _assert_state_equal(host, sim, n_stream, what):
    """Final ship state, for the envs whose record counts agree (an env one record ahead in the stream, see above,
    has been reset by it already)."""
    same = np.array([len(h) == k for h, k in zip(host.records(), n_stream)])
    assert same.sum() >= host.N - 1, (what, same)
    rows = np.repeat(same, 2)  # two ships per env
    np.testing.assert_array_equal(_state(sim)[rows], _state(host.sim)[rows], err_msg=f"{what} final ship state")


@pytest.mark.parametrize("collav", ["sbmpc", "none"])
@pytest.mark.parametrize("N", [5, 9])
def test_partial_waves_equal_host_driven_loop(collav, N):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg = abi.ast_config(collav)
    cfg.envs_per_wave = 3
    table = _table(4, N_DEC, N, seed=31 + N)
    host, stream = _HostLoop(cfg, N, table), _Stream(cfg, N, table)
    assert stream.sim.lanes_per_env == 16
    for _ in range(LAUNCHES):
        np.testing.assert_array_equal(stream.launch(T), np.full(N, T))
        host.launch(T)
    assert _assert_equal(host, stream, f"{collav} N={N}") >= 3 * N
    eps = np.concatenate([r[:, 3] for r in stream.records()])
    assert eps.max() >= 1  # episodes were reset inside the kernel
    host.sim.close()
    stream.sim.close()


def test_two_handles_keep_their_own_constants():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    N = 8
    a = abi.ast_config("sbmpc", time_step=4)
    b = abi.ast_config("sbmpc", time_step=5)
    b.wind_speed, b.wind_direction = a.wind_speed + 3.5, a.wind_direction + 1.1
    b.current_velocity_component_from_north = a.current_velocity_component_from_north + 0.4
    b.current_velocity_component_from_east = a.current_velocity_component_from_east - 0.3
    b.env_radius_of_acceptance = a.env_radius_of_acceptance * 1.5
    tables = [_table(4, N_DEC, N, seed=5), _table(4, N_DEC, N, seed=6)]
    streams = [_Stream(c, N, t) for c, t in zip((a, b), tables)]  # both handles alive, launches alternating
    for _ in range(LAUNCHES):
        for s in streams:
            np.testing.assert_array_equal(s.launch(T), np.full(N, T))
    for k, (c, t) in enumerate(zip((a, b), tables)):
        host = _HostLoop(c, N, t)
        for _ in range(LAUNCHES):
            host.launch(T)
        _assert_equal(host, streams[k], f"handle {k}")
        host.sim.close()
    ra, rb = streams[0].records(), streams[1].records()
    assert any(len(x) != len(y) or not np.array_equal(x, y) for x, y in zip(ra, rb))  # the configs do differ
    for s in streams:
        s.sim.close()


def test_policy_stream_equals_host_driven_loop():
    """shipsim_run_policy (MODE 2 of the same kernels), N = 8, hidden 64, deterministic: the actions it logged,
    replayed decision by decision through the host-driven step loop, give the stream's records and final state."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from test_gpu_policy_act import _trainer
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = abi.ast_config("sbmpc")
    N = 8
    sim = ShipSim(cfg, N)
    sim.reset()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    for _ in range(LAUNCHES):
        o = sim.run_policy(dp.weights(), T, N_DEC, ep, dec, deterministic=True, log=log, log_len=log_len)
        np.testing.assert_array_equal(o["ticks"].cpu().numpy(), np.full(N, T))
    ln = log_len.cpu().numpy()
    assert ln.min() >= 3 and ln.max() < CAP
    L = log.cpu().numpy()
    recs = [L[i, :ln[i]] for i in range(N)]
    n_eps = int(max(r[:, abi.DL_EPISODE].max() for r in recs)) + 2
    # the action of every decision the stream started: logged ones, and (a decision still running at the end has
    # its action in its record row already) the row past each env's last record
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
