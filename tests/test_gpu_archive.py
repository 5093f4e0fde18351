"""The state archive on the device (shipsim_archive_store / _load / _elect; archive_gather_kernel and the ar_*
kernels): a clone started from an archive cell continues as its source, bit for bit; an archive of n_envs cells is a
snapshot; out-of-range indices, the refusals, graph capture; the election against tests/archive_ref.py, exactly;
StateArchive's carry tensors; relative_cells against numpy. Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import archive_ref as A
from ast_sac_amd import shipsim
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv
from ast_sac_amd.shipsim import ShipSim, ShipSimError, StateArchive

pytestmark = pytest.mark.gpu

N_DEC = 3
CAP = 32
EINVAL = -1


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _i32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64).astype(np.int32), device="cuda")


def _env_bytes(sim):
    """The handle's whole state, one bytes object per env."""
    return A.per_env_bytes(sim.snapshot().data.cpu().numpy(), sim.n_envs, sim.n_ships)


class _Stream:
    """A handle on a table stream and what its caller owns (two built alike run alike)."""

    def __init__(self, cfg, n, seed=777):
        self.env = BatchedMultiShipRLEnv(n_envs=n, cfg=abi.Config.from_buffer_copy(cfg))
        self.sim, self.n = self.env.sim, n
        self.ep = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.dec = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.log = torch.zeros((n, CAP, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
        self.ln = torch.zeros(n, dtype=torch.int32, device="cuda")
        a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (4, N_DEC, n)).astype(np.float32)
        self.table = torch.from_numpy(abi.normalized_to_scoping(a)).cuda()
        self.sim.reset()

    def advance(self, ticks):
        self.ln.zero_()
        out = self.sim.run_table(self.table, ticks, self.ep, self.dec, log=self.log, log_len=self.ln)
        self.sim.synchronize()
        L, ln = self.log.cpu().numpy(), self.ln.cpu().numpy()
        t, d = out["ticks"].cpu().numpy(), out["decisions"].cpu().numpy()
        assert ln.max() <= CAP
        return [(int(t[i]), int(d[i]), L[i, :ln[i]].tobytes()) for i in range(self.n)]

    def close(self):
        self.env.close()


def _indices(n, m):
    """env_of_cell: the envs over the cells with repeats (m > n) or a subset (m < n), one cell left empty;
    cell_of_env: another walk over the filled cells."""
    env_of_cell = [(7 * c + 3) % n for c in range(m)]
    env_of_cell[m // 2] = -1
    filled = [c for c in range(m) if env_of_cell[c] >= 0]
    cell_of_env = [filled[(7 * i + 1) % len(filled)] for i in range(n)]
    return env_of_cell, cell_of_env


# ---- a clone continues as its source ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(48, 7), (5, 300)])
@pytest.mark.parametrize("collav,k", [("sbmpc", 1), ("none", 2), ("sbmpc", 4)])
def test_a_clone_from_a_cell_continues_as_its_source(collav, k, n, m):
    """Two handles alike, 64 ticks of a table stream; envs of the first go into an archive (a permutation with
    repeats), envs of the second start from its cells under another index array; 128 ticks more on both: env i of
    the second reports the decision records, and ends on the snapshot bytes, of the env it came from."""
    cfg = abi.ast_config(collav, n_obs_ships=k)
    a, b = _Stream(cfg, n), _Stream(cfg, n)
    first = a.advance(64)
    assert b.advance(64) == first
    done = [np.frombuffer(r[2], np.float64).reshape(-1, abi.DECLOG_COLS)[:, abi.DL_TICKS].sum() for r in first]
    assert any(first[i][0] > done[i] for i in range(n))  # envs are paused mid-decision
    env_of_cell, cell_of_env = _indices(n, m)
    arch = a.sim.archive(m)
    assert isinstance(arch, StateArchive) and arch.data.numel() == A.columns(m, 1 + k)[1]
    arch.store(env_of_cell)
    before = _env_bytes(a.sim)
    cells = A.per_env_bytes(arch.data.cpu().numpy(), m, 1 + k)
    for c in range(m):
        assert cells[c] == (before[env_of_cell[c]] if env_of_cell[c] >= 0 else bytes(len(cells[c]))), c
    arch.load(cell_of_env, sim=b.sim)
    src = [env_of_cell[c] for c in cell_of_env]
    assert len(set(src)) > 1 and src != list(range(n))
    st = torch.as_tensor(src, device="cuda")
    b.ep.copy_(a.ep[st])
    b.dec.copy_(a.dec[st])
    b.table = a.table[:, :, st].contiguous()  # clone i gets its source's actions
    at_load = _env_bytes(b.sim)
    for i in range(n):
        assert at_load[i] == before[src[i]], i
    want, got = a.advance(128), b.advance(128)
    end_a, end_b = _env_bytes(a.sim), _env_bytes(b.sim)
    assert len(set(end_a)) > 1
    for i in range(n):
        assert got[i] == want[src[i]], f"env {i} <- {src[i]}: ticks, decisions, records"
        assert end_b[i] == end_a[src[i]], f"env {i} <- {src[i]}: snapshot bytes"
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ["noniw", "single"])
def test_raw_tick_kinds_move_whole(kind):
    n, m = 48, 7
    cfg = abi.c1_config("sbmpc") if kind == "noniw" else abi.c2_config()
    sims = [ShipSim(abi.Config.from_buffer_copy(cfg), n) for _ in range(2)]
    rng = np.random.Generator(np.random.PCG64(5))
    S = n * sims[0].n_ships
    spreads = [(f, torch.from_numpy(rng.uniform(-s, s, S)).cuda())
               for f, s in ((abi.F_NORTH, 150.0), (abi.F_EAST, 150.0), (abi.F_YAW, 0.15), (abi.F_U, 0.5))]
    for s in sims:
        s.reset()
        for f, d in spreads:
            s.set(f, s.get(f) + d)
        s.tick(64)
    a, b = sims
    env_of_cell, cell_of_env = _indices(n, m)
    arch = a.archive(m)
    arch.store(env_of_cell)
    arch.load(cell_of_env, sim=b)
    src = [env_of_cell[c] for c in cell_of_env]
    before, at_load = _env_bytes(a), _env_bytes(b)
    assert len(set(before)) > 1
    for i in range(n):
        assert at_load[i] == before[src[i]], i
    a.tick(64)
    b.tick(64)
    end_a, end_b = _env_bytes(a), _env_bytes(b)
    for i in range(n):
        assert end_b[i] == end_a[src[i]] and end_a[i] != before[i], i
    for s in sims:
        s.close()


# ---- n_cells == n_envs: a snapshot ------------------------------------------------------------------------------
def test_an_archive_of_n_envs_cells_is_a_snapshot():
    n = 16
    d = _Stream(abi.ast_config("sbmpc"), n)
    d.advance(64)
    arch = d.sim.archive(n)
    assert arch.data.numel() == d.sim.state_bytes and not arch.data.any()
    arch.store(list(range(n)))
    snap = d.sim.snapshot()
    np.testing.assert_array_equal(arch.data.cpu().numpy(), snap.data.cpu().numpy())
    d.advance(64)
    src = [(3 * i + 1) % n for i in range(n - 2)] + [-1, n]
    d.sim.fork(src, source=arch.as_snapshot())
    got = d.sim.snapshot().data.cpu().numpy().copy()
    d.advance(32)
    d.sim.fork(src, source=snap)
    d.sim.synchronize()
    # (the two envs left alone moved on between the forks: compare the forked ones, which is every byte they own)
    a = A.per_env_bytes(got, n, 2)
    b = A.per_env_bytes(d.sim.snapshot().data.cpu().numpy(), n, 2)
    whole = A.per_env_bytes(snap.data.cpu().numpy(), n, 2)
    for i in range(n - 2):
        assert a[i] == b[i] == whole[src[i]], i
    d.close()


# ---- out of range -----------------------------------------------------------------------------------------------
def test_out_of_range_indices_leave_the_cell_or_env_alone():
    n, m = 16, 9
    d = _Stream(abi.ast_config("sbmpc"), n)
    d.advance(64)
    arch = d.sim.archive(m)
    arch.store([i % n for i in range(m)])
    d.advance(64)
    live = _env_bytes(d.sim)
    cells0 = A.per_env_bytes(arch.data.cpu().numpy(), m, 2)
    bad_env = [-1, n, m, 2**31 - 1, -2**31]  # (m < n: m is an env)
    idx = bad_env + [3, 3, 15, 0]
    arch.store(idx)
    cells1 = A.per_env_bytes(arch.data.cpu().numpy(), m, 2)
    for c in range(m):
        ok = 0 <= idx[c] < n
        assert cells1[c] == (live[idx[c]] if ok else cells0[c]), c
    assert cells1[2] == live[m] and cells1[0] == cells0[0] and cells0[0] != live[0]
    bad_cell = [-1, n, m, 2**31 - 1, -2**31]  # (n > m: n is no cell)
    cidx = bad_cell + [(2 * i) % m for i in range(n - 5)]
    arch.load(cidx)
    after = _env_bytes(d.sim)
    for i in range(n):
        ok = 0 <= cidx[i] < m
        assert after[i] == (cells1[cidx[i]] if ok else live[i]), i
    assert sum(0 <= c < m for c in cidx) == n - 5
    d.close()


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_and_their_messages():
    n, m = 8, 5
    sim = ShipSim(abi.ast_config("sbmpc"), n)
    arch = sim.archive(m)
    with pytest.raises(ShipSimError, match="archive_store before reset"):
        arch.store([0] * m)
    sim.reset()
    L, h = sim.L, sim.h
    nb = arch.data.numel()
    assert int(L.shipsim_archive_bytes(h, m)) == nb == A.columns(m, 2)[1]
    assert L.shipsim_archive_bytes(h, 0) == EINVAL and L.shipsim_archive_bytes(h, abi.ARCHIVE_MAX_CELLS + 1) == EINVAL
    idx_c = torch.zeros(m, dtype=torch.int32, device="cuda")
    idx_e = torch.zeros(n, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    before = arch.data.clone()
    for fn, name, idx in ((L.shipsim_archive_store, "archive_store", idx_c), (L.shipsim_archive_load, "archive_load", idx_e)):
        for args, msg in (((None, nb, m, P(idx)), "the archive is NULL"),
                          ((P(arch.data), nb, m, None), "is NULL"),
                          ((P(arch.data), nb - 1, m, P(idx)), "(shipsim_archive_bytes)"),
                          ((P(arch.data), nb, m + 1, P(idx)), "(shipsim_archive_bytes)"),
                          ((P(arch.data), nb, 0, P(idx)), "SHIPSIM_ARCHIVE_MAX_CELLS"),
                          ((P(arch.data), nb, abi.ARCHIVE_MAX_CELLS + 1, P(idx)), "SHIPSIM_ARCHIVE_MAX_CELLS"),
                          ((C.c_void_p(arch.data.data_ptr() + 8), nb, m, P(idx)), "not 16-byte aligned")):
            assert fn(h, *args) == EINVAL, (name, msg)
            err = L.shipsim_last_error(h).decode()
            assert err.startswith(name + ":") and msg in err, err
    torch.cuda.synchronize()
    assert torch.equal(arch.data, before)
    with pytest.raises(ShipSimError, match="entries, expected 5"):
        arch.store([0] * n)
    with pytest.raises(ShipSimError, match="entries, expected 8"):
        arch.load([0] * m)
    other = ShipSim(abi.ast_config("sbmpc", n_obs_ships=2), n)
    with pytest.raises(ShipSimError, match="the archive is of"):
        arch.load([0] * n, sim=other)
    other.close()
    sim.close()
    # a recording handle: the refusal of snapshot / restore / fork
    env = BatchedMultiShipRLEnv(n_envs=4, cfg=abi.ast_config("sbmpc"))
    arch = env.archive(3)
    env.record_trajectories(capacity=8)
    env.reset()
    for call in (lambda: arch.store([0, 1, 2]), lambda: arch.load([0, 1, 2, 0])):
        with pytest.raises(ShipSimError, match="trajectory recording is on"):
            call()
    env.close()


# ---- the election -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", A.N_CELLS)
@pytest.mark.parametrize("n_envs", A.N_ENVS)
def test_elect_equals_the_python_restatement(n_envs, n_cells):
    cell_score = torch.full((n_cells,), float("nan"), dtype=torch.float64, device="cuda")
    cell_seen = torch.zeros(n_cells, dtype=torch.int32, device="cuda")
    ref_score, ref_seen = [A.NAN] * n_cells, [0] * n_cells
    taken = 0
    for name, cell, score in A.rounds(n_envs, n_cells):
        eoc, k = shipsim.archive_elect(torch.from_numpy(cell).cuda(), torch.from_numpy(score).cuda(), cell_score, cell_seen)
        want, ref_score, ref_seen, n_improved = A.elect(cell, score, ref_score, ref_seen, n_cells)
        np.testing.assert_array_equal(eoc.cpu().numpy(), np.array(want, dtype=np.int32), err_msg=name)
        np.testing.assert_array_equal(cell_score.cpu().numpy().view(np.uint64), A.bits(ref_score), err_msg=name)
        np.testing.assert_array_equal(cell_seen.cpu().numpy(), np.array(ref_seen, dtype=np.int64), err_msg=name)
        assert int(k.cpu()[0]) == n_improved, name
        taken += n_improved
    assert taken > 0
    # the optional outputs left out
    cs = cell_score.clone()
    L = shipsim.load_library()
    ws = torch.empty(int(L.shipsim_archive_workspace_bytes(n_cells)), dtype=torch.uint8, device="cuda")
    eoc = torch.zeros(n_cells, dtype=torch.int32, device="cuda")
    c, s = torch.from_numpy(cell).cuda(), torch.from_numpy(score).cuda()
    rc = L.shipsim_archive_elect(n_envs, n_cells, c.data_ptr(), s.data_ptr(), cs.data_ptr(), None, ws.data_ptr(),
                                 ws.numel(), eoc.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert (eoc == -1).all() and torch.equal(cs.view(torch.int64), cell_score.view(torch.int64))  # nothing strictly better


# ---- update / load with carry, and capture -----------------------------------------------------------------------
def _scores(d):
    return -d.sim.level_distance()


def test_update_and_load_carry_the_callers_tensors_with_the_states():
    n, bins = 48, 3
    d = _Stream(abi.ast_config("sbmpc"), n)
    d.advance(64)
    m = d.env.relative_cells_count(bins)
    arch = d.env.archive(m)
    cell = d.env.relative_cells(bins, 6000.0)
    score = _scores(d)
    tag = torch.arange(n, dtype=torch.float64, device="cuda").view(n, 1).repeat(1, 2) + 0.5
    carry = dict(ep_idx=d.ep, dec_idx=d.dec, tag=tag)
    live = _env_bytes(d.sim)
    ep0, dec0 = d.ep.cpu().numpy().copy(), d.dec.cpu().numpy().copy()
    eoc, k = arch.update(cell, score, carry=carry)
    want, ref_score, ref_seen, n_improved = A.elect(cell.cpu().numpy(), score.cpu().numpy(), [A.NAN] * m, [0] * m, m)
    e = eoc.cpu().numpy()
    np.testing.assert_array_equal(e, np.array(want))
    assert int(k.cpu()[0]) == n_improved >= 1
    np.testing.assert_array_equal(arch.cell_seen.cpu().numpy(), np.array(ref_seen))
    cells = A.per_env_bytes(arch.data.cpu().numpy(), m, 2)
    for c in range(m):
        if e[c] >= 0:
            assert cells[c] == live[e[c]]
            assert int(arch.carry["ep_idx"][c]) == ep0[e[c]] and int(arch.carry["dec_idx"][c]) == dec0[e[c]]
            assert arch.carry["tag"][c].tolist() == [e[c] + 0.5] * 2
        else:
            assert cells[c] == bytes(len(cells[c])) and arch.carry["tag"][c].tolist() == [0.0, 0.0]
    # on: the envs move, a second update improves some cells only; then every env starts from a filled cell
    d.advance(64)
    eoc2 = arch.update(d.env.relative_cells(bins, 6000.0), _scores(d), carry=dict(ep_idx=d.ep, dec_idx=d.dec, tag=tag))[0]
    e2 = eoc2.cpu().numpy()
    filled = np.flatnonzero((e >= 0) | (e2 >= 0))
    cells = A.per_env_bytes(arch.data.cpu().numpy(), m, 2)
    kept = {k_: v.cpu().numpy().copy() for k_, v in arch.carry.items()}
    cidx = [int(filled[i % len(filled)]) for i in range(n - 1)] + [-1]
    live = _env_bytes(d.sim)
    ep1, tag1 = d.ep.cpu().numpy().copy(), tag.cpu().numpy().copy()
    arch.load(cidx, carry=dict(ep_idx=d.ep, dec_idx=d.dec, tag=tag))
    after = _env_bytes(d.sim)
    for i in range(n - 1):
        assert after[i] == cells[cidx[i]]
        assert int(d.ep[i]) == kept["ep_idx"][cidx[i]] and int(d.dec[i]) == kept["dec_idx"][cidx[i]]
        assert tag[i].tolist() == kept["tag"][cidx[i]].tolist()
    assert after[n - 1] == live[n - 1] and int(d.ep[n - 1]) == ep1[n - 1] and tag[n - 1].tolist() == tag1[n - 1].tolist()
    with pytest.raises(ShipSimError, match="no update"):
        arch.load(cidx, carry=dict(weights=tag))
    d.close()


def test_store_elect_and_load_in_one_graph():
    n, bins = 16, 2
    d = _Stream(abi.ast_config("sbmpc"), n)
    d.advance(64)
    sim = d.sim
    snap = sim.snapshot()
    m = d.env.relative_cells_count(bins)
    cell = d.env.relative_cells(bins, 6000.0)
    score = _scores(d)
    cidx = _i32([(5 * i) % m for i in range(n)])

    def fresh():
        a = d.env.archive(m)
        a.update(cell, score)  # eager once: nothing is allocated under capture
        a.data.zero_()
        a.cell_score.fill_(float("nan"))
        a.cell_seen.zero_()
        return a

    cap, eag = fresh(), fresh()
    sim.restore(snap)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            cap.update(cell, score)
            cap.load(cidx)
    results = []
    for replay in range(2):
        sim.restore(snap)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        results.append((cap.env_of_cell.cpu().numpy().copy(), int(cap.n_improved.cpu()[0]),
                        cap.cell_score.cpu().numpy().view(np.uint64).copy(), cap.cell_seen.cpu().numpy().copy(),
                        cap.data.cpu().numpy().copy(), sim.snapshot().data.cpu().numpy().copy()))
        sim.restore(snap)
        eag.update(cell, score)
        eag.load(cidx)
        torch.cuda.synchronize()
        want = (eag.env_of_cell.cpu().numpy(), int(eag.n_improved.cpu()[0]), eag.cell_score.cpu().numpy().view(np.uint64),
                eag.cell_seen.cpu().numpy(), eag.data.cpu().numpy(), sim.snapshot().data.cpu().numpy())
        for x, y in zip(results[-1], want):
            np.testing.assert_array_equal(x, y)
    assert results[0][1] >= 1 and results[1][1] == 0  # the second replay finds every cell held by an equal score
    assert (results[1][3] == 2 * results[0][3]).all() and not (results[0][5] == snap.data.cpu().numpy()).all()
    d.close()


# ---- relative_cells -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_relative_cells_equals_numpy_on_get_state(k):
    n, bins, radius = 65, 5, 3000.0
    d = _Stream(abi.ast_config("sbmpc", n_obs_ships=k), n)
    d.advance(192)
    ns = 1 + k
    north = d.sim.get(abi.F_NORTH).cpu().numpy().reshape(n, ns)
    east = d.sim.get(abi.F_EAST).cpu().numpy().reshape(n, ns)
    sc = d.sim.get(abi.E_SAMPLING_COUNT).cpu().numpy().astype(np.int64)
    dn, de = north[:, 1] - north[:, 0], east[:, 1] - east[:, 0]
    inv = bins / (2.0 * radius)
    bn = np.clip(np.floor((dn + radius) * inv), 0, bins - 1).astype(np.int64)
    be = np.clip(np.floor((de + radius) * inv), 0, bins - 1).astype(np.int64)
    want = (np.clip(sc, 0, d.env.cfg.max_sampling_frequency) * bins + bn) * bins + be
    got = d.env.relative_cells(bins, radius).cpu().numpy()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    assert len(set(got.tolist())) > 1 and got.min() >= 0 and got.max() < d.env.relative_cells_count(bins)
    # a NaN position names no cell
    pos = d.sim.get(abi.F_NORTH)
    pos[1] = float("nan")
    d.sim.set(abi.F_NORTH, pos)
    got = d.env.relative_cells(bins, radius).cpu().numpy()
    assert got[0] == -1 and (got[1:] == want[1:]).all()
    d.close()
