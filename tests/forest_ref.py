"""The forest (include/shipsim.h: shipsim_tree_init_forest / _select_forest) restated over tests/tree_ref.py, which it
leaves as it is: R roots, nodes 0..R-1, in one node pool; the saturating prefix rule that hands the W workers to the
roots; select in two forms — by arrival counts, level by level from the roots, and literally, per root in id order, one
worker after the other from that root — and rounds of select -> expand -> backup (expand and backup are tree_ref's:
neither knows roots). The device kernels, the host half (csrc/shipsim_tree_host.hpp) and this file agree bit for bit."""
import random

import numpy as np

import tree_ref as R

HDR_ROOTS = 3


class Forest(R.Tree):
    """A tree_ref.Tree whose first n_roots nodes are roots; the header's fourth int holds n_roots."""

    def __init__(self, max_nodes, max_children, n_roots=1):
        assert 1 <= n_roots <= max_nodes
        super().__init__(max_nodes, max_children)
        self.n_roots = n_roots
        self.n_nodes = n_roots
        for r in range(n_roots):
            self.parent[r] = -1

    def to_bytes(self):
        buf = super().to_bytes()
        o = R.layout(self.M, self.C)["header"] + 4 * HDR_ROOTS
        buf[o:o + 4] = np.asarray([self.n_roots], dtype=np.int32).view(np.uint8)
        return buf


def init_forest(max_nodes, max_children, n_roots):
    """shipsim_tree_init_forest: n_nodes = hdr[3] = n_roots, zero counters, the roots."""
    return Forest(max_nodes, max_children, n_roots)


def root_arrivals(root_workers, W):
    """a_r = min(max(c_r, 0), W - min(W, sum of max(c_r', 0) over r' < r)): in Python integers, which do not overflow."""
    out, before = [], 0
    for c in root_workers:
        c = max(int(c), 0)
        out.append(min(c, W - min(W, before)))
        before += c
    return out


def root_of(T, v):
    while T.parent[v] >= 0:
        v = T.parent[v]
    return v


def _roots(T, root_workers):
    return min(len(root_workers), T.n_roots, T.n_nodes)


def _ordered(T, stay, newc, W):
    """tree_ref's output order, the trailing workers that no root received with leaf -1."""
    leaf, expand = [], []
    for v in range(T.n_nodes):
        leaf += [v] * (stay.get(v, 0) + newc.get(v, 0))
        expand += [0] * stay.get(v, 0) + [1] * newc.get(v, 0)
    assert len(leaf) <= W
    return leaf + [-1] * (W - len(leaf)), expand + [0] * (W - len(expand))


def select_forest(T, W, root_workers, max_depth, wnum, wden, c_explore):
    """By arrival counts: level 0's frontier is the roots with their a_r; then as tree_ref.select."""
    n = _roots(T, root_workers)
    a = root_arrivals(root_workers[:n], W)
    stay, newc, arrived = {}, {}, {}
    frontier = {r: a[r] for r in range(n)}
    while frontier:
        nxt = {}
        for v, A in frontier.items():
            stay[v] = newc[v] = 0
            if R._closed(T, v, max_depth):
                stay[v] = A
                continue
            for t in range(A):
                N = T.visits[v] + t
                if R.widens(T.n_children[v] + newc[v], T.C, wnum, wden, N):
                    newc[v] += 1
                elif T.n_children[v] == 0:
                    stay[v] += 1
                else:
                    b = R._best_child(T, v, N, c_explore, arrived)
                    arrived[b] = arrived.get(b, 0) + 1
                    nxt[b] = nxt.get(b, 0) + 1
        frontier = nxt
    return _ordered(T, stay, newc, W)


def select_forest_literal(T, W, root_workers, max_depth, wnum, wden, c_explore):
    """Per root in id order, one worker after the other from that root, each seeing the virtual visits of those
    before it; then the fixed output order."""
    n = _roots(T, root_workers)
    a = root_arrivals(root_workers[:n], W)
    came, stay, newc = {}, {}, {}
    for r in range(n):
        for _ in range(a[r]):
            v = r
            while True:
                t = came.get(v, 0)
                came[v] = t + 1
                if R._closed(T, v, max_depth):
                    stay[v] = stay.get(v, 0) + 1
                    break
                N = T.visits[v] + t
                if R.widens(T.n_children[v] + newc.get(v, 0), T.C, wnum, wden, N):
                    newc[v] = newc.get(v, 0) + 1
                    break
                if T.n_children[v] == 0:
                    stay[v] = stay.get(v, 0) + 1
                    break
                v = R._best_child(T, v, N, c_explore, came)
    return _ordered(T, stay, newc, W)


def even_split(W, n_roots):
    return [W // n_roots + (1 if r < W % n_roots else 0) for r in range(n_roots)]


def random_forest(seed, max_nodes, max_children, n_roots, n_nodes, max_depth=6, big=False):
    """tree_ref.random_tree's recipe over n_roots roots: random shape under every root, visits (zeros among them),
    value sums of both signs, ties among siblings, a few terminal nodes, a terminal root now and then."""
    rng = random.Random(seed)
    T = Forest(max_nodes, max_children, n_roots)
    for r in range(n_roots):
        T.visits[r] = rng.randrange(0, 500)
        T.value_sum[r] = rng.randrange(-1 << 30, 1 << 30)
        if rng.randrange(17) == 0:
            T.flags[r] = R.TERMINAL
    while T.n_nodes < n_nodes:
        open_ = [v for v in range(T.n_nodes) if T.n_children[v] < T.C and T.depth[v] < max_depth]
        if not open_:
            break
        p = rng.choice(open_[:8] + open_[-8:] + [rng.choice(open_)])
        kind = rng.randrange(6)
        visits = 0 if kind == 0 else rng.randrange(1, 200)
        vs = rng.randrange(-1 << 34, 1 << 34) if visits else 0
        if big and kind == 1:
            vs = rng.choice((-1, 1)) * ((1 << 60) + rng.randrange(1 << 20))
        if kind == 2 and T.n_children[p]:
            sib = T.child[p][T.n_children[p] - 1]
            visits, vs = T.visits[sib], T.value_sum[sib]
        T.add(p, action=rng.uniform(-1, 1), visits=visits, value_sum=vs, flags=R.TERMINAL if rng.randrange(9) == 0 else 0)
    return T


def extract(T, r):
    """The tree under root r as a tree_ref.Tree of its own, ids relabelled in increasing order (the root becomes 0):
    (tree, ids), ids[new] = old."""
    ids = [v for v in range(T.n_nodes) if root_of(T, v) == r]
    new = {old: i for i, old in enumerate(ids)}
    S = R.Tree(max(len(ids), 1), T.C)
    S.n_nodes = len(ids)
    for i, old in enumerate(ids):
        S.parent[i] = new[T.parent[old]] if T.parent[old] >= 0 else -1
        S.depth[i], S.n_children[i] = T.depth[old], T.n_children[old]
        S.child[i] = [new.get(c, 0) if l < T.n_children[old] else 0 for l, c in enumerate(T.child[old])]
        S.visits[i], S.value_sum[i], S.action[i], S.flags[i] = T.visits[old], T.value_sum[old], T.action[old], T.flags[old]
    return S, ids


def play_rounds(T, W, root_workers, rounds, max_depth, wnum, wden, c_explore, ops=None):
    """tree_ref.play_rounds over a forest: `rounds` rounds of select_forest -> expand -> backup with tree_ref's
    synthetic action, value and terminal flag (a worker without a leaf takes part in all three and is passed through);
    `ops` (select, expand, backup callables on plain lists, select taking root_workers after W) replaces this file's
    own. Returns the per-round outputs."""
    sel = ops[0] if ops else (lambda *a: select_forest(T, *a))
    exp = ops[1] if ops else (lambda *a: R.expand(T, *a))
    bak = ops[2] if ops else (lambda *a: R.backup(T, *a))
    log = []
    for _ in range(rounds):
        leaf, flags = sel(W, root_workers, max_depth, wnum, wden, c_explore)
        action = [R.synthetic_action(w, leaf[w]) for w in range(W)]
        node = exp(leaf, flags, action)
        value = [R.synthetic_value(i) for i in node]
        term = [R.synthetic_terminal(i) if flags[w] else 0 for w, i in enumerate(node)]
        bak(node, value, term)
        log.append((list(leaf), list(flags), list(node)))
    return log
