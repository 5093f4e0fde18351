"""The search tree on the device (shipsim_tree_init / _select / _expand / _backup; the tr_* kernels) against the Python
restatement tests/tree_ref.py, bit for bit: select over worker counts, fan-outs and the cases the rule turns on;
expand's ids and child slots; backup under contention; rounds of all three with the whole tree buffer compared; one
linear graph of a round; and TreeSearch over real envs end to end. Needs an MI355X."""
import math

import numpy as np
import pytest
import torch

import archive_ref as A
import tree_ref as R
from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args
from ast_sac_amd.rl_env.ship_in_transit.tree_search import TreeSearch
from ast_sac_amd.shipsim import SearchTree, tree_backup, tree_expand, tree_select

pytestmark = pytest.mark.gpu

PARAMS = ((6, 1, 1, 1.0), (6, 4, 1, 0.0), (3, 1, 9, 0.37), (6, 100, 3, 5.0))  # max_depth, wnum, wden, c_explore


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _i32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64).astype(np.int32), device="cuda")


class Dev:
    """A SearchTree holding the bytes of a restatement's tree, with the three operations on plain lists."""

    def __init__(self, T, W):
        self.t = SearchTree(T.M, T.C, W)
        self.t.data.copy_(torch.from_numpy(T.to_bytes()))

    def select(self, W, max_depth, wnum, wden, c):
        assert W == self.t.n_workers
        leaf, flags = tree_select(self.t, max_depth, (wnum, wden), c)
        return leaf.cpu().tolist(), flags.cpu().tolist()

    def expand(self, leaf, flags, action):
        node = tree_expand(self.t, torch.tensor(action, dtype=torch.float32), _i32(leaf), _i32(flags))
        return node.cpu().tolist()

    def backup(self, node, value, terminal=None):
        term = None if terminal is None else torch.tensor(terminal, dtype=torch.uint8)
        tree_backup(self.t, torch.tensor(value, dtype=torch.float64), _i32(node), term)

    def bytes(self):
        return self.t.data.cpu().numpy()


_TREES = {}


def _tree(Cc):
    """One random tree per fan-out (<= 200 nodes, value sums beyond 2^53 among them), shared and left unchanged."""
    if Cc not in _TREES:
        _TREES[Cc] = R.random_tree(11 + Cc, 200, Cc, n_nodes={1: 7, 3: 90, 64: 200}[Cc], big=True)
    return _TREES[Cc]


# ---- select ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [1, 3, 64])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 300])
def test_select_equals_the_restatement(W, Cc):
    T = _tree(Cc)
    d = Dev(T, W)
    before = T.to_bytes()
    for p in PARAMS:
        assert d.select(W, *p) == R.select(T, W, *p), p
    np.testing.assert_array_equal(d.bytes(), before)  # select writes nothing to the tree


def test_select_one_node_past_the_scan_tile():
    n = abi.TREE_SCAN_TILE + 1
    T = R.random_tree(5, n, 5, n_nodes=n, max_depth=8)
    assert T.n_nodes == n
    v = n - 1  # the way to the last node pays: workers end on both sides of the tile's edge
    while v > 0:
        T.visits[v], T.value_sum[v], T.flags[v] = 2, 64 << 24, 0
        v = T.parent[v]
    T.flags[0] = 0
    d = Dev(T, 300)
    for p in ((9, 1, 1, 1.0), (9, 9, 1, 3.0)):
        leaf, flags = d.select(300, *p)
        assert (leaf, flags) == R.select(T, 300, *p)
        assert leaf[-1] == n - 1 and leaf[0] < abi.TREE_SCAN_TILE


def test_select_on_the_cases_the_rule_turns_on():
    W = 65
    # a terminal root keeps everybody
    T = R.Tree(16, 3)
    T.add(0, visits=1, value_sum=1 << 24)
    T.flags[0] = 1
    assert Dev(T, W).select(W, 9, 1, 1, 1.0) == ([0] * W, [0] * W)
    # a leaf at max_depth: the children of the root are as deep as a worker goes
    T = R.Tree(16, 3)
    a = T.add(0, visits=3, value_sum=15 << 24)  # Q = 5
    b = T.add(0, visits=3, value_sum=15 << 24)  # equal statistics: a tie, to the lower slot first
    c = T.add(0)                               # a child with zero visits: Q = 0
    T.add(a, visits=1)
    T.visits[0] = 6
    for p in ((1, 1, 1, 1.0), (1, 1, 1, 0.0), (9, 1, 1, 0.5), (9, 1, 1, 0.0)):
        got = Dev(T, W).select(W, *p)
        assert got == R.select(T, W, *p), p
    leaf, flags = Dev(T, W).select(W, 1, 1, 1, 0.0)
    assert leaf == [a] * W and flags == [0] * W  # c_explore = 0: everyone to the first of the two best
    # c_explore = 1: the tie goes to a (5 + sqrt(7) / 4 against c's sqrt(7)), and a's virtual visit sends the second
    # worker to b (5 + sqrt(8) / 4 against a's 5 + sqrt(8) / 5)
    assert Dev(T, 2).select(2, 1, 1, 1, 1.0) == ([a, b], [0, 0]) == R.select(T, 2, 1, 1, 1, 1.0)
    assert c in Dev(T, W).select(W, 1, 1, 1, 50.0)[0]  # enough exploration reaches the unvisited child
    # negative values, and sums beyond 2^53 whose means differ in the last bits
    T = R.Tree(16, 4)
    big = (1 << 60) + 12345
    ids = [T.add(0, visits=1 << 20, value_sum=-big), T.add(0, visits=1 << 20, value_sum=-big - 1024),
           T.add(0, visits=7, value_sum=-(3 << 24)), T.add(0, visits=(1 << 20) - 1, value_sum=big)]
    T.visits[0] = (1 << 22) + 6
    for p in ((1, 1, 1, 0.0), (1, 1, 1, 1e3), (1, 1, 1 << 15, 1e9)):
        assert Dev(T, W).select(W, *p) == R.select(T, W, *p), p
    assert abs(T.value_sum[ids[0]]) > 1 << 53


# ---- expand ---------------------------------------------------------------------------------------------------------
def test_expand_ids_slots_and_a_pool_full_by_one():
    T = R.random_tree(0, 64, 4, n_nodes=40)
    W = 65
    leaf, flags = R.select(T, W, 6, 30, 1, 1.0)
    k = sum(flags)
    assert k >= 6 and max(sum(1 for w in range(W) if flags[w] and leaf[w] == v) for v in set(leaf)) >= 2
    for room in (k, k - 1):  # the pool takes every new node; the pool is full by one
        Tm = R.random_tree(0, 40 + room, 4, n_nodes=40)
        d = Dev(Tm, W)
        action = [R.synthetic_action(w, leaf[w]) for w in range(W)]
        node = d.expand(leaf, flags, action)
        assert node == R.expand(Tm, leaf, flags, action)
        np.testing.assert_array_equal(d.bytes(), Tm.to_bytes())
        assert Tm.dropped == k - room and node.count(-1) == k - room and Tm.n_nodes == 40 + room
        new = [i for w, i in enumerate(node) if flags[w] and i >= 0]
        assert new == list(range(40, 40 + room))  # ids in worker order
        for w, i in enumerate(node):
            if flags[w] and i >= 0:
                assert Tm.parent[i] == leaf[w] and i in Tm.child[leaf[w]][:Tm.n_children[leaf[w]]]


# ---- backup ---------------------------------------------------------------------------------------------------------
def test_backup_under_contention_duplicates_skips_and_the_terminal_bit():
    T = R.Tree(64, 2)
    v = 0
    for _ in range(R.MAX_DEPTH):  # one chain as deep as a tree gets
        v = T.add(v)
    side = T.add(0)
    W = 300
    d = Dev(T, W)
    node = [v] * W
    value = [((w * 7919) % 1001 - 500) / 7.0 for w in range(W)]
    d.backup(node, value)
    R.backup(T, node, value)
    np.testing.assert_array_equal(d.bytes(), T.to_bytes())
    assert T.visits[0] == T.visits[v] == W
    # duplicates at several depths, nodes outside the tree, non-finite and huge values, the terminal bit
    node = [(w * 5) % (T.n_nodes + 3) - 1 for w in range(W)]
    value = [math.nan if w % 11 == 3 else math.inf if w % 13 == 5 else -math.inf if w % 17 == 2 else
             1e300 if w % 19 == 4 else -65536.5 if w % 23 == 1 else (w - 150) / 3.0 + 2.0 ** -25 for w in range(W)]
    term = [1 if w % 4 == 1 else 0 for w in range(W)]
    d.backup(node, value, term)
    R.backup(T, node, value, term)
    np.testing.assert_array_equal(d.bytes(), T.to_bytes())
    assert T.skipped > 40 and T.flags[side] in (0, 1) and sum(T.flags) > 5


# ---- rounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Cc,W", [(4096, 3, 300), (700, 64, 65)])
def test_twenty_rounds_leave_the_reference_tree(M, Cc, W):
    T = R.Tree(M, Cc)
    d = Dev(T, W)
    want = R.play_rounds(T, W, 20, 6, 3, 1, 25.0)
    got = R.play_rounds(None, W, 20, 6, 3, 1, 25.0, ops=(d.select, d.expand, d.backup))
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"round {r}"
    np.testing.assert_array_equal(d.bytes(), T.to_bytes())
    assert T.n_nodes > 300 and T.skipped > 0 and (T.dropped > 0) == (M == 700)


def test_one_linear_graph_of_a_round_equals_eager():
    W, M, Cc = 300, 2048, 5

    def one_round(t):
        leaf, flags = t.select(6, (3, 1), 25.0)
        node = t.expand(leaf.float() * 0.01 - 0.3)
        value = torch.remainder(node.double() * 0.37, 5.0) - 2.0
        t.backup(value, terminal=(torch.remainder(node, 9) == 4).to(torch.uint8))

    cap, eag = SearchTree(M, Cc, W), SearchTree(M, Cc, W)
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
    assert eag.n_nodes > 100 and int(eag.visits[0]) == 6 * W - int(eag.header[2])


# ---- end to end -----------------------------------------------------------------------------------------------------
def _policies(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lim = float(np.deg2rad(30))

    def draw(obs):
        return (torch.rand(n, generator=g, device="cuda", dtype=torch.float32) * 2.0 - 1.0) * lim

    return draw, draw


@pytest.mark.parametrize("k,rounds", [(1, 3), (2, 1)])
def test_tree_search_over_envs(k, rounds):
    n = 64
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc", n_obs_ships=k), n)
    ts = TreeSearch(env, 512, max_children=4, widen=(4, 1), c_explore=50.0)
    propose, rollout = _policies(n, 7)
    backed = 0
    for _ in range(rounds):
        out = ts.round(propose, rollout)
        backed += int(((out["node"] >= 0) & torch.isfinite(out["value"])).sum())
    torch.cuda.synchronize()
    t = ts.tree
    nn = t.n_nodes
    assert nn > 1 and int(t.visits[0]) == backed == n * rounds - int(t.header[2])
    depth, parent = t.depth[:nn].cpu().numpy(), t.parent[:nn].cpu().numpy()
    assert depth[0] == 0 and (depth[1:] == depth[parent[1:]] + 1).all() and depth.max() <= ts.max_depth
    actions, nodes = ts.best_path()
    assert len(actions) == len(nodes) - 1 >= 1 and nodes[0] == 0 and all(abs(a) <= np.deg2rad(30) + 1e-6 for a in actions)
    # loading a node and stepping with a child's action reproduces that child's archived state, bit for bit
    for c in sorted({1, nn // 2, nn - 1}):
        p = int(parent[c])
        cells = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        cells[0], cells[1] = p, c
        ts.archive.load(cells)
        active = torch.zeros(n, dtype=torch.uint8, device="cuda")
        active[0] = 1
        env.step(t.action[c].repeat(n), active=active)
        torch.cuda.synchronize()
        per_env = A.per_env_bytes(env.sim.snapshot().data.cpu().numpy(), n, env.sim.n_ships)
        assert per_env[0] == per_env[1], f"node {c} from its parent {p}"
    env.close()


def test_tree_search_refuses_per_env_weather():
    n = 4
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n)
    env.set_weather(dict(wind_speed=np.full(n, 3.0), wind_direction=np.zeros(n), current_north=np.zeros(n),
                         current_east=np.full(n, 0.1)))
    with pytest.raises(ValueError, match="weather"):
        TreeSearch(env, 16)
    env.close()
