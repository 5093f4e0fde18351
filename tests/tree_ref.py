"""The search tree (include/shipsim.h: shipsim_tree_*) restated in Python integers and IEEE doubles (Python floats;
NumPy only for the buffer's bytes): the layout of the tree buffer, select in two forms — by arrival counts, node by
node, as the header states it, and literally, one worker after the other from the root with shared virtual counters —
expand and backup. The device kernels, the host half (csrc/shipsim_tree_host.hpp) and this file agree bit for bit."""
import math
import random
import struct

import numpy as np

MAX_NODES = 1 << 22
MAX_CHILDREN = 64
MAX_DEPTH = 32
MAX_WORKERS = 1 << 22
SCAN_TILE = 1024
FRAC_BITS = 24
Q_CLAMP = 1 << 40
TERMINAL = 1
FIELDS = ("header", "parent", "depth", "n_children", "child", "visits", "value_sum", "action", "flags")


def r256(b):
    return (b + 255) & ~255


def layout(max_nodes, max_children):
    M, Cc = max_nodes, max_children
    sizes = dict(header=16, parent=4 * M, depth=4 * M, n_children=4 * M, child=4 * M * Cc, visits=4 * M, value_sum=8 * M,
                 action=4 * M, flags=4 * M)
    out, o = {}, 0
    for name in FIELDS:
        out[name] = o
        o += r256(sizes[name])
    out["bytes"] = o
    return out


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


class Tree:
    """The tree as Python lists: value_sum in Python integers, action as floats that float32 holds exactly."""

    def __init__(self, max_nodes, max_children):
        self.M, self.C = max_nodes, max_children
        self.n_nodes, self.dropped, self.skipped = 1, 0, 0
        M = max_nodes
        self.parent, self.depth, self.n_children = [0] * M, [0] * M, [0] * M
        self.child = [[0] * max_children for _ in range(M)]
        self.visits, self.value_sum, self.action, self.flags = [0] * M, [0] * M, [0.0] * M, [0] * M
        self.parent[0] = -1

    def add(self, parent, action=0.0, visits=0, value_sum=0, flags=0):
        """A node by hand (building a tree for a test): the new id."""
        i = self.n_nodes
        assert i < self.M and self.n_children[parent] < self.C
        self.parent[i], self.depth[i], self.action[i] = parent, self.depth[parent] + 1, f32(action)
        self.visits[i], self.value_sum[i], self.flags[i], self.n_children[i] = visits, value_sum, flags, 0
        self.child[parent][self.n_children[parent]] = i
        self.n_children[parent] += 1
        self.n_nodes += 1
        return i

    def to_bytes(self):
        """The tree buffer as the device holds it (zero where nothing was written)."""
        L = layout(self.M, self.C)
        buf = np.zeros(L["bytes"], dtype=np.uint8)

        def put(name, values, dtype):
            a = np.asarray(values, dtype=dtype).reshape(-1)
            buf[L[name]:L[name] + a.nbytes] = a.view(np.uint8)

        wrap = lambda x: ((x + (1 << 31)) % (1 << 32)) - (1 << 31)  # noqa: E731
        put("header", [self.n_nodes, wrap(self.dropped), wrap(self.skipped), 0], np.int32)
        put("parent", self.parent, np.int32)
        put("depth", self.depth, np.int32)
        put("n_children", self.n_children, np.int32)
        put("child", self.child, np.int32)
        put("visits", self.visits, np.int32)
        put("value_sum", [((v + (1 << 63)) % (1 << 64)) - (1 << 63) for v in self.value_sum], np.int64)
        put("action", self.action, np.float32)
        put("flags", self.flags, np.int32)
        return buf


# ---- the arithmetic ----
def widens(m, C, wnum, wden, N):
    return m < C and m * m * wden < wnum * (N + 1)


def q_of(visits, value_sum):
    return math.ldexp(float(value_sum) / float(visits), -FRAC_BITS) if visits > 0 else 0.0


def score(q, c_explore, N, visits, arrived):
    return q + (c_explore * math.sqrt(float(N + 1))) / float(1 + visits + arrived)


def quantize(value):
    try:
        x = math.ldexp(value, FRAC_BITS)
    except OverflowError:
        x = math.copysign(math.inf, value)
    if x >= Q_CLAMP:
        return Q_CLAMP
    if x <= -Q_CLAMP:
        return -Q_CLAMP
    return int(round(x))  # (round half to even, as nearbyint in the default rounding mode)


def _closed(T, v, max_depth):
    return bool(T.flags[v] & TERMINAL) or T.depth[v] >= max_depth


def _best_child(T, v, N, c_explore, arrived):
    best, best_score = -1, 0.0
    for l in range(T.n_children[v]):
        a = T.child[v][l]
        s = score(q_of(T.visits[a], T.value_sum[a]), c_explore, N, T.visits[a], arrived.get(a, 0))
        if best < 0 or s > best_score:
            best, best_score = a, s
    return best


def _ordered(T, stay, newc, W):
    leaf, expand = [], []
    for v in range(T.n_nodes):
        leaf += [v] * (stay.get(v, 0) + newc.get(v, 0))
        expand += [0] * stay.get(v, 0) + [1] * newc.get(v, 0)
    assert len(leaf) == W
    return leaf, expand


def select(T, W, max_depth, wnum, wden, c_explore):
    """By arrival counts: a node routes its arrivals t = 0, 1, ... one after the other; level by level."""
    stay, newc, arrived = {}, {}, {}
    frontier = {0: W}
    while frontier:
        nxt = {}
        for v, A in frontier.items():
            stay[v] = newc[v] = 0
            if _closed(T, v, max_depth):
                stay[v] = A
                continue
            for t in range(A):
                N = T.visits[v] + t
                if widens(T.n_children[v] + newc[v], T.C, wnum, wden, N):
                    newc[v] += 1
                elif T.n_children[v] == 0:
                    stay[v] += 1
                else:
                    a = _best_child(T, v, N, c_explore, arrived)
                    arrived[a] = arrived.get(a, 0) + 1
                    nxt[a] = nxt.get(a, 0) + 1
        frontier = nxt
    return _ordered(T, stay, newc, W)


def select_literal(T, W, max_depth, wnum, wden, c_explore):
    """One worker after the other from the root, each seeing the virtual visits of those before it; then the fixed
    output order (workers are interchangeable)."""
    came, stay, newc = {}, {}, {}
    for _ in range(W):
        v = 0
        while True:
            t = came.get(v, 0)
            came[v] = t + 1
            if _closed(T, v, max_depth):
                stay[v] = stay.get(v, 0) + 1
                break
            N = T.visits[v] + t
            if widens(T.n_children[v] + newc.get(v, 0), T.C, wnum, wden, N):
                newc[v] = newc.get(v, 0) + 1
                break
            if T.n_children[v] == 0:
                stay[v] = stay.get(v, 0) + 1
                break
            # (the workers sent to a child before this one are those that arrived at it)
            v = _best_child(T, v, N, c_explore, came)
    return _ordered(T, stay, newc, W)


def expand(T, leaf, expand_flags, action):
    """node_out; the tree is changed in place. The widening workers of one node are adjacent."""
    n, W = T.n_nodes, len(leaf)
    slot = []
    for w in range(W):
        s = -1
        v = leaf[w]
        if expand_flags[w] and 0 <= v < n and T.depth[v] < MAX_DEPTH:
            k = 0
            while k < T.C and w - k - 1 >= 0 and expand_flags[w - k - 1] and leaf[w - k - 1] == v:
                k += 1
            if T.n_children[v] + k < T.C:
                s = T.n_children[v] + k
        slot.append(s)
    node_out, rank = [], 0
    for w in range(W):
        if not expand_flags[w]:
            node_out.append(leaf[w])
            continue
        i = n + rank
        if slot[w] >= 0:
            rank += 1
        if slot[w] < 0 or i >= T.M:
            T.dropped += 1
            node_out.append(-1)
            continue
        v = leaf[w]
        T.parent[i], T.depth[i], T.n_children[i], T.visits[i], T.value_sum[i] = v, T.depth[v] + 1, 0, 0, 0
        T.action[i], T.flags[i] = f32(action[w]), 0
        T.child[v][slot[w]] = i
        T.n_children[v] += 1
        T.n_nodes += 1
        node_out.append(i)
    return node_out


def backup(T, node, value, terminal=None):
    n = T.n_nodes
    for w in range(len(node)):
        if not (0 <= node[w] < n) or not math.isfinite(value[w]):
            T.skipped += 1
            continue
        q = quantize(value[w])
        if terminal is not None and terminal[w]:
            T.flags[node[w]] |= TERMINAL
        v = node[w]
        for _ in range(MAX_DEPTH + 1):
            if not 0 <= v < n:
                break
            T.visits[v] += 1
            T.value_sum[v] += q
            v = T.parent[v]


# ---- trees and rounds for the tests ----
def random_tree(seed, max_nodes, max_children, n_nodes, max_depth=6, big=False):
    """A seeded tree of n_nodes: random shape, visits (zeros among them), value sums of both signs (beyond 2^53 with
    `big`), equal statistics among siblings now and then, a few terminal nodes."""
    rng = random.Random(seed)
    T = Tree(max_nodes, max_children)
    T.visits[0] = rng.randrange(0, 500)
    T.value_sum[0] = rng.randrange(-1 << 30, 1 << 30)
    while T.n_nodes < n_nodes:
        open_ = [v for v in range(T.n_nodes) if T.n_children[v] < T.C and T.depth[v] < max_depth]
        if not open_:
            break
        p = rng.choice(open_[:8] + open_[-8:])
        kind = rng.randrange(6)
        visits = 0 if kind == 0 else rng.randrange(1, 200)
        vs = rng.randrange(-1 << 34, 1 << 34) if visits else 0
        if big and kind == 1:
            vs = rng.choice((-1, 1)) * ((1 << 60) + rng.randrange(1 << 20))
        if kind == 2 and T.n_children[p]:  # a tie with the sibling before
            sib = T.child[p][T.n_children[p] - 1]
            visits, vs = T.visits[sib], T.value_sum[sib]
        T.add(p, action=rng.uniform(-1, 1), visits=visits, value_sum=vs, flags=TERMINAL if rng.randrange(9) == 0 else 0)
    return T


def synthetic_action(w, leaf):
    return f32(((w * 37 + leaf * 11) % 201 - 100) / 100.0)


def synthetic_value(node):
    """A value that is a function of the node id: both signs, non-finite now and then (skipped)."""
    if node >= 0 and node % 13 == 5:
        return math.inf if node % 2 else math.nan
    return ((node * 2654435761) % 2001 - 1000) / 37.0


def synthetic_terminal(node):
    return 1 if node >= 0 and node % 11 == 7 else 0


def play_rounds(T, W, rounds, max_depth, wnum, wden, c_explore, ops=None):
    """`rounds` rounds of select -> expand -> backup with the synthetic action, value and terminal flag; `ops`
    (select, expand, backup callables on plain lists) replaces this file's own. Returns the per-round outputs."""
    sel = ops[0] if ops else (lambda *a: select(T, *a))
    exp = ops[1] if ops else (lambda *a: expand(T, *a))
    bak = ops[2] if ops else (lambda *a: backup(T, *a))
    log = []
    for _ in range(rounds):
        leaf, flags = sel(W, max_depth, wnum, wden, c_explore)
        action = [synthetic_action(w, leaf[w]) for w in range(W)]
        node = exp(leaf, flags, action)
        value = [synthetic_value(i) for i in node]
        term = [synthetic_terminal(i) if flags[w] else 0 for w, i in enumerate(node)]
        bak(node, value, term)
        log.append((list(leaf), list(flags), list(node)))
    return log
