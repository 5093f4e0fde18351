"""The forest on the device (shipsim_tree_init_forest / _select_forest; tr_init_forest_kernel, tr_roots_tile_kernel,
tr_clear_forest_kernel) against the Python restatement tests/forest_ref.py, bit for bit: the buffer init leaves; select
over root counts, worker counts, fan-outs and root_workers that sum to W, to less and to more; roots across a scan
tile; a one-root forest against shipsim_tree_select; rounds with the whole buffer compared; backup under contention
below a root other than 0; one linear graph of a forest round; and TreeSearch(n_roots=4) over real envs, one tree per
weather, replayed on uniform handles. Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

import forest_ref as F
import tree_ref as R
import weather_harness as WH
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, config_from_args, default_args
from ast_sac_amd.rl_env.ship_in_transit.tree_search import TreeSearch
from ast_sac_amd.rl_env.ship_in_transit.weather import KEYS
from ast_sac_amd.shipsim import SearchTree, ShipSimError, tree_backup, tree_expand, tree_select

pytestmark = pytest.mark.gpu

PARAMS = ((6, 1, 1, 1.0), (6, 4, 1, 0.0), (3, 1, 9, 0.37), (6, 100, 3, 5.0))  # max_depth, wnum, wden, c_explore


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _i32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64).astype(np.int32), device="cuda")


class Dev:
    """A SearchTree holding the bytes of a restatement's forest, with the three operations on plain lists."""

    def __init__(self, T, W, n_roots=None):
        self.t = SearchTree(T.M, T.C, W, n_roots=T.n_roots if n_roots is None else n_roots)
        self.t.data.copy_(torch.from_numpy(T.to_bytes()))

    def select(self, W, root_workers, max_depth, wnum, wden, c):
        assert W == self.t.n_workers
        leaf, flags = tree_select(self.t, max_depth, (wnum, wden), c, root_workers=_i32(root_workers))
        return leaf.cpu().tolist(), flags.cpu().tolist()

    def expand(self, leaf, flags, action):
        node = tree_expand(self.t, torch.tensor(action, dtype=torch.float32), _i32(leaf), _i32(flags))
        return node.cpu().tolist()

    def backup(self, node, value, terminal=None):
        term = None if terminal is None else torch.tensor(terminal, dtype=torch.uint8)
        tree_backup(self.t, torch.tensor(value, dtype=torch.float64), _i32(node), term)

    def bytes(self):
        return self.t.data.cpu().numpy()


def patterns(W, n_roots):
    """root_workers: even, all on the last root, zeros interleaved, a sum below W, a sum above W, a negative entry,
    an entry above W."""
    even = F.even_split(W, n_roots)
    return [even, [0] * (n_roots - 1) + [W], [2 * c if r % 2 == 0 else 0 for r, c in enumerate(even)],
            [c // 2 for c in even], [c + 1 for c in even], [-3] + even[1:], even[:-1] + [W + 5] if n_roots > 1 else [W + 5]]


# ---- 1. init --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_roots", [1, 2, 65, 1025])
def test_init_forest_leaves_the_restatements_bytes(n_roots):
    M, Cc = 1100, 3
    t = SearchTree(M, Cc, 1100, n_roots=n_roots)
    want = F.init_forest(M, Cc, n_roots).to_bytes()
    if n_roots == 1:  # (a SearchTree of one root is shipsim_tree_init's: the call itself, on its buffer)
        t._call("shipsim_tree_init_forest", 1)
    np.testing.assert_array_equal(t.data.cpu().numpy(), want)
    assert t.n_nodes == n_roots == t.n_roots and int(t.header[abi.TREE_HDR_ROOTS]) == n_roots
    # over a used buffer: the counters and the roots are written, nothing else
    t.data.fill_(0x5A)
    t._call("shipsim_tree_init_forest", n_roots)
    got = t.data.cpu().numpy()
    L = R.layout(M, Cc)
    assert got[:16].view(np.int32).tolist() == [n_roots, 0, 0, n_roots]
    for name, dt in (("parent", np.int32), ("depth", np.int32), ("n_children", np.int32), ("visits", np.int32),
                     ("value_sum", np.int64), ("action", np.float32), ("flags", np.int32)):
        a = got[L[name]:L[name] + M * np.dtype(dt).itemsize].view(dt)
        np.testing.assert_array_equal(a[:n_roots], np.full(n_roots, -1 if name == "parent" else 0, dtype=dt), err_msg=name)
        assert (a[n_roots:].view(np.uint8) == 0x5A).all(), name
    assert (got[L["child"]:L["visits"]] == 0x5A).all()


# ---- 2. select ------------------------------------------------------------------------------------------------------
_FORESTS = {}


def _forest(n_roots, Cc):
    """One random forest per case (<= 400 nodes, value sums beyond 2^53 among them), shared and left unchanged."""
    if (n_roots, Cc) not in _FORESTS:
        n = {1: 7, 2: 90, 5: 200, 64: 300, 65: 260, 300: 400}[n_roots]
        _FORESTS[n_roots, Cc] = F.random_forest(100 + n_roots + Cc, 400, Cc, n_roots, n_nodes=n, big=True)
    return _FORESTS[n_roots, Cc]


@pytest.mark.parametrize("n_roots,W,Cc", [(1, 1, 1), (2, 63, 3), (5, 64, 64), (64, 65, 3), (65, 300, 3), (300, 300, 64)])
def test_select_forest_equals_the_restatement(n_roots, W, Cc):
    T = _forest(n_roots, Cc)
    d = Dev(T, W)
    before = T.to_bytes()
    for rw in patterns(W, n_roots):
        for p in PARAMS:
            assert d.select(W, rw, *p) == F.select_forest(T, W, rw, *p), (rw[:8], p)
    np.testing.assert_array_equal(d.bytes(), before)  # select writes nothing to the tree
    # the default of a forest is the even split
    leaf, flags = d.t.select(6, (1, 1), 1.0)
    assert (leaf.cpu().tolist(), flags.cpu().tolist()) == F.select_forest(T, W, F.even_split(W, n_roots), 6, 1, 1, 1.0)


def test_select_forest_serves_no_more_roots_than_the_header_names():
    T = _forest(5, 64)
    W = 64
    d = Dev(T, W)
    rw = F.even_split(W, 5)
    d.t.header[abi.TREE_HDR_ROOTS] = 3  # the caller says 5, the buffer 3: roots 3 and 4 get nobody
    T3 = F.random_forest(100 + 5 + 64, 400, 64, 5, n_nodes=200, big=True)
    T3.n_roots = 3
    got = d.select(W, rw, 6, 1, 1, 1.0)
    assert got == F.select_forest(T3, W, rw, 6, 1, 1, 1.0)
    assert got[0].count(-1) == rw[3] + rw[4]


# ---- 3. roots across a scan tile ------------------------------------------------------------------------------------
def test_select_forest_with_roots_past_the_scan_tile():
    n_roots, W, M = abi.TREE_SCAN_TILE + 1, 1100, 4096
    T = F.random_forest(9, M, 5, n_roots, n_nodes=1500, max_depth=8)
    last = n_roots - 1
    v = last
    for _ in range(4):  # the way down from the last root pays: its workers spread below it
        v = T.add(v, action=0.1, visits=2, value_sum=64 << 24)
        T.add(T.parent[v], action=-0.1, visits=1, value_sum=1 << 24)
    T.flags[last], T.visits[last] = 0, 40
    rw = [0 if r % 7 == 3 else 1 for r in range(last)]
    rw.append(W - sum(rw))
    assert rw[last] > 64 and sum(rw) == W
    d = Dev(T, W)
    for p in ((9, 1, 1, 1.0), (9, 9, 1, 3.0)):
        leaf, flags = d.select(W, rw, *p)
        assert (leaf, flags) == F.select_forest(T, W, rw, *p)
        assert -1 not in leaf and sum(1 for x in leaf if F.root_of(T, x) == last) == rw[last]
    # the prefix saturates inside the first tile: every root past it gets nobody, the one at the tile's edge the rest
    rw = [1] * 1000 + [0] * 23 + [W, W]
    leaf, flags = d.select(W, rw, 9, 1, 1, 1.0)
    assert (leaf, flags) == F.select_forest(T, W, rw, 9, 1, 1, 1.0)
    assert all(F.root_of(T, x) != last for x in leaf) and sum(1 for x in leaf if F.root_of(T, x) == last - 1) == 100
    big = [(1 << 31) - 1] * n_roots  # (plain int32 sums of these overflow)
    assert d.select(W, big, 9, 1, 1, 1.0) == F.select_forest(T, W, big, 9, 1, 1, 1.0)


# ---- 4. one root ----------------------------------------------------------------------------------------------------
def test_a_one_root_forest_equals_select_on_a_tree():
    W, M, Cc = 300, 2048, 5
    t = SearchTree(M, Cc, W)  # shipsim_tree_init's tree: the header's fourth int is 0
    assert int(t.header[abi.TREE_HDR_ROOTS]) == 0 and t.n_roots == 1
    for r in range(5):
        leaf, flags = t.select(6, (3, 1), 25.0)
        want = leaf.clone(), flags.clone()
        got = t.select(6, (3, 1), 25.0, root_workers=[W])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"round {r}"
        node = t.expand(leaf.float() * 0.01 - 0.3)
        t.backup(torch.remainder(node.double() * 0.37, 5.0) - 2.0, terminal=(torch.remainder(node, 9) == 4).to(torch.uint8))
    assert t.n_nodes > 100


# ---- 5. rounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Cc,W,n_roots", [(4096, 3, 300, 7), (700, 64, 65, 65)])
def test_twenty_rounds_leave_the_reference_forest(M, Cc, W, n_roots):
    T = F.init_forest(M, Cc, n_roots)
    d = Dev(T, W)
    rw = F.even_split(W, n_roots)
    want = F.play_rounds(T, W, rw, 20, 6, 3, 1, 25.0)
    got = F.play_rounds(None, W, rw, 20, 6, 3, 1, 25.0, ops=(d.select, d.expand, d.backup))
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"round {r}"
    np.testing.assert_array_equal(d.bytes(), T.to_bytes())
    assert T.n_nodes > 300 and T.skipped > 0 and (T.dropped > 0) == (M == 700)


# ---- 6. backup ------------------------------------------------------------------------------------------------------
def test_backup_under_contention_below_a_root_other_than_0():
    T = F.init_forest(64, 4, 3)
    a = T.add(2)
    b = T.add(a)
    c = T.add(2)
    x, y = T.add(0), T.add(1)  # (roots 0 and 1 have children of their own, which nobody backs up)
    W = 300
    d = Dev(T, W)
    three = (a, b, c)
    node = [-1 if w % 29 == 7 else three[(w * 5) % 3] for w in range(W)]
    value = [math.nan if w % 11 == 3 else math.inf if w % 13 == 5 else 1e300 if w % 19 == 4 else (w - 150) / 3.0 + 2.0 ** -25
             for w in range(W)]
    term = [1 if w % 50 == 1 else 0 for w in range(W)]
    d.backup(node, value, term)
    R.backup(T, node, value, term)
    np.testing.assert_array_equal(d.bytes(), T.to_bytes())
    taken = [w for w in range(W) if node[w] >= 0 and math.isfinite(value[w])]
    assert T.visits[2] == len(taken) and T.value_sum[2] == sum(R.quantize(value[w]) for w in taken)
    assert T.visits[0] == T.visits[1] == 0 and T.value_sum[0] == T.value_sum[1] == 0 and T.visits[x] == T.visits[y] == 0
    assert T.skipped == W - len(taken) > 40 and T.visits[a] == T.visits[b] + sum(1 for w in taken if node[w] == a)
    assert any(T.flags[v] & 1 for v in three) and T.flags[2] == 0


# ---- 7. graph capture -----------------------------------------------------------------------------------------------
def test_one_linear_graph_of_a_forest_round_equals_eager():
    W, M, Cc, n_roots = 300, 2048, 5, 5
    rw = _i32([100, 0, 120, 30, 40])  # (ten workers are left over: leaf -1, skipped by the backup)

    def one_round(t):
        leaf, flags = t.select(6, (3, 1), 25.0, root_workers=rw)
        node = t.expand(leaf.float() * 0.01 - 0.3)
        value = torch.remainder(node.double() * 0.37, 5.0) - 2.0
        t.backup(value, terminal=(torch.remainder(node, 9) == 4).to(torch.uint8))

    cap, eag = SearchTree(M, Cc, W, n_roots=n_roots), SearchTree(M, Cc, W, n_roots=n_roots)
    one_round(cap)  # eager once: nothing is allocated under capture
    cap.data.zero_()
    cap.init()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            one_round(cap)
    cap.data.zero_()
    cap.init()
    torch.cuda.synchronize()
    for r in range(6):
        g.replay()
        one_round(eag)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(cap.data.cpu().numpy(), eag.data.cpu().numpy(), err_msg=f"round {r}")
        np.testing.assert_array_equal(cap.node.cpu().numpy(), eag.node.cpu().numpy())
    visits = eag.visits[:n_roots].cpu().tolist()
    assert eag.n_nodes > 100 and visits[1] == 0 and int(eag.header[2]) >= 6 * 10
    assert sum(visits) == 6 * W - int(eag.header[2])


# ---- 8 - 10. end to end ---------------------------------------------------------------------------------------------
def _policies(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lim = float(np.deg2rad(30))

    def draw(obs):
        return (torch.rand(n, generator=g, device="cuda", dtype=torch.float32) * 2.0 - 1.0) * lim

    return draw, draw


def _structure(ts, rounds, n_roots, arrivals):
    """Conservation and structure of a forest search: (n_nodes, parent, depth, node_root)."""
    t = ts.tree
    nn = t.n_nodes
    assert nn > n_roots and int(t.header[1]) == 0 and int(t.header[2]) == 0 and int(t.header[abi.TREE_HDR_ROOTS]) == n_roots
    assert t.visits[:n_roots].cpu().tolist() == [rounds * a for a in arrivals]  # every backup reaches its root
    parent, depth = t.parent[:nn].cpu().numpy(), t.depth[:nn].cpu().numpy()
    node_root = ts.node_root[:nn].cpu().numpy()
    assert (parent[:n_roots] == -1).all() and (depth[:n_roots] == 0).all() and (parent[n_roots:] >= 0).all()
    assert (node_root[:n_roots] == np.arange(n_roots)).all()
    assert (depth[n_roots:] == depth[parent[n_roots:]] + 1).all() and depth.max() <= ts.max_depth
    assert (node_root[n_roots:] == node_root[parent[n_roots:]]).all()  # (a parent's id is below its child's)
    for r in range(n_roots):
        actions, nodes = ts.best_path(root=r)
        assert nodes[0] == r and len(actions) == len(nodes) - 1 >= 1 and all(node_root[v] == r for v in nodes)
    return nn, parent, depth, node_root


def test_forest_search_one_tree_per_weather_replays_on_uniform_handles():
    n, n_roots, rounds = 64, 4, 2
    args = default_args(collav_mode="sbmpc")
    cfg = config_from_args(args)
    ws = WH.four_weathers(cfg)
    assert len({tuple(w[k] for k in KEYS) for w in ws}) == 4
    env = BatchedMultiShipRLEnv(args, n, weather=WH.interleaved(ws, n))
    ts = TreeSearch(env, 512, max_children=4, widen=(4, 1), c_explore=50.0, n_roots=n_roots)
    assert ts.archive.weather is not None
    propose, rollout = _policies(n, 7)
    for _ in range(rounds):
        out = ts.round(propose, rollout)
        leaf, root = out["leaf"].cpu().numpy(), out["root"].cpu().numpy()
        assert (root == ts.node_root[out["leaf"].long()].cpu().numpy()).all() and (leaf >= 0).all()
        assert np.bincount(root, minlength=n_roots).tolist() == F.even_split(n, n_roots)
    torch.cuda.synchronize()
    nn, parent, depth, node_root = _structure(ts, rounds, n_roots, F.even_split(n, n_roots))
    action = ts.tree.action[:nn].cpu()
    kept_obs, kept_reward = ts.node_obs[:nn].cpu().numpy(), ts.node_reward[:nn].cpu().numpy()
    for r in range(n_roots):
        mine = [v for v in range(nn) if node_root[v] == r and depth[v] >= 1]
        assert mine
        v = max(mine, key=lambda i: (depth[i], i))  # the deepest node below root r
        path = []
        while parent[v] >= 0:
            path.append(v)
            v = int(parent[v])
        uni = BatchedMultiShipRLEnv(args, n, cfg=WH.cfg_with(cfg, ws[r]))  # (root r's weather as it was set)
        obs = uni.reset()
        assert obs[0].cpu().numpy().tobytes() == kept_obs[r].tobytes()
        cum = torch.zeros(n, dtype=torch.float64, device="cuda")
        for v in reversed(path):
            obs, rew, done, info = uni.step(action[v].repeat(n).cuda())
            cum = cum + rew
            assert obs[0].cpu().numpy().tobytes() == kept_obs[v].tobytes(), f"root {r} node {v}: the observation"
            assert cum[0].cpu().numpy().tobytes() == kept_reward[v].tobytes(), f"root {r} node {v}: the reward"
        uni.close()
    env.close()


def test_forest_search_under_uniform_weather_is_root_parallel_search():
    n, n_roots, rounds = 64, 4, 2
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n)
    ts = TreeSearch(env, 512, max_children=4, widen=(4, 1), c_explore=50.0, n_roots=n_roots)
    assert ts.archive.weather is None
    propose, rollout = _policies(n, 7)
    for _ in range(rounds):
        ts.round(propose, rollout)
    torch.cuda.synchronize()
    _structure(ts, rounds, n_roots, F.even_split(n, n_roots))
    env.close()


def test_forest_search_with_workers_left_over_and_a_root_without_any():
    """root_workers sums to 40 of 64: the 24 trailing workers get no leaf, take no decision and are skipped by the
    backup; root 1, asked for nothing, stays a lone node."""
    n, n_roots, rounds, asked = 64, 4, 2, [10, 0, 20, 10]
    args = default_args(collav_mode="sbmpc")
    ws = WH.four_weathers(config_from_args(args))
    env = BatchedMultiShipRLEnv(args, n, weather=WH.interleaved(ws, n))
    ts = TreeSearch(env, 512, max_children=4, widen=(4, 1), c_explore=50.0, n_roots=n_roots, root_workers=asked)
    propose, rollout = _policies(n, 11)
    served = sum(asked)
    for _ in range(rounds):
        out = {k: v.cpu().numpy() for k, v in ts.round(propose, rollout).items()}
        idle = np.arange(n) >= served  # (select's output order: the workers no root received come last)
        assert (out["leaf"][idle] == -1).all() and (out["root"][idle] == -1).all() and (out["node"][idle] == -1).all()
        assert (out["expand"][idle] == 0).all() and (out["ticks"][idle] == 0).all() and (out["events"][idle] == 0).all()
        assert not out["terminal"][idle].any()
        assert (out["leaf"][~idle] >= 0).all() and (out["node"][~idle] >= 0).all() and out["ticks"][~idle].sum() > 0
        assert np.bincount(out["root"][~idle], minlength=n_roots).tolist() == asked
        assert (out["root"][~idle] == ts.node_root[torch.as_tensor(out["leaf"][~idle]).long().cuda()].cpu().numpy()).all()
    torch.cuda.synchronize()
    t = ts.tree
    nn = t.n_nodes
    assert t.visits[:n_roots].cpu().tolist() == [rounds * a for a in asked]
    assert int(t.header[1]) == 0 and int(t.header[2]) == rounds * (n - served)  # skipped: the idle workers, nobody else
    parent, node_root = t.parent[:nn].cpu().numpy(), ts.node_root[:nn].cpu().numpy()
    assert nn > n_roots and int(t.n_children[1]) == 0 and (node_root[n_roots:] != 1).all()
    assert (node_root[n_roots:] == node_root[parent[n_roots:]]).all() and (node_root[:n_roots] == np.arange(n_roots)).all()
    assert ts.best_path(root=1) == ([], [1]) and len(ts.best_path(root=2)[0]) >= 1
    env.close()


def test_forest_search_refuses_more_roots_than_envs_and_wrong_root_workers():
    n = 4
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n)
    with pytest.raises(ValueError, match="n_roots"):
        TreeSearch(env, 16, n_roots=n + 1)
    with pytest.raises(ValueError, match="n_roots"):
        TreeSearch(env, 16, n_roots=0)
    with pytest.raises(ValueError, match="root_workers"):
        TreeSearch(env, 16, n_roots=2, root_workers=[1, 2, 1])
    with pytest.raises(ShipSimError, match="n_roots"):
        SearchTree(16, 2, 4, n_roots=5)
    env.close()
