"""Times the search tree's three operations next to the env launches of a round. Writes profiles/tree_search.json.

Trees: complete trees of 2^16 and 2^20 nodes (16 children per inner node out of max_children = 32, so that well-visited
nodes still widen; visits the subtree sizes, seeded mean values in [-1, 1]), laid out on the device, with room for one
round's new nodes. Per tree and W in {4096, 65536}: select, expand (of that
select's workers) and backup (of that expand's nodes), each the median of `--reps` timed calls between device events;
the tree is put back before every expand and backup. select is also timed with widening shut (every worker goes down
to a leaf: the longest descent) and with c_explore = 0.

Env launches: a TreeSearch over K = 1 sbmpc envs with W = n_envs runs `--rounds` rounds; its tree calls are timed
inside the round, and what remains of the round (archive load and store, the widening decision, the rollout) is
the env's share.

    python scripts/tree_bench.py [--out FILE] [--reps R] [--rounds N]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.tree_search import TreeSearch  # noqa: E402
from ast_sac_amd.shipsim import SearchTree  # noqa: E402

FAN = 16


def complete_tree(n, W, dev, seed=1):
    """A SearchTree whose first n nodes are a complete FAN-ary tree in breadth-first order."""
    t = SearchTree(n + W, 2 * FAN, W, device=dev)
    i = torch.arange(n, device=dev)
    parent = torch.where(i > 0, (i - 1) // FAN, -1)
    first = i * FAN + 1
    nc = (n - first).clamp(0, FAN)
    depth = torch.zeros(n, dtype=torch.int64, device=dev)
    lo, d = 0, 0
    while lo < n:  # level d holds ids [lo, lo + FAN^d)
        depth[lo:lo + FAN ** d] = d
        lo, d = lo + FAN ** d, d + 1
    visits = torch.ones(n, dtype=torch.int64, device=dev)
    for level in range(d - 1, 0, -1):  # a node's visits: its subtree's size
        at = (depth == level).nonzero().reshape(-1)
        visits.index_add_(0, parent[at], visits[at])
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 2.0 - 1.0
    t.parent[:n], t.depth[:n], t.n_children[:n] = parent.int(), depth.int(), nc.int()
    t.child[:n, :FAN] = (first[:, None] + torch.arange(FAN, device=dev)[None, :]).int()
    t.visits[:n] = visits.int()
    t.value_sum[:n] = torch.round(q * visits.double() * float(1 << 24)).long()
    t.header[0] = n
    return t, d - 1


def timed(fn, reps, before=None):
    ms = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def bench_ops(n, W, dev, reps):
    t, depth = complete_tree(n, W, dev)
    saved = t.data.clone()
    restore = lambda: t.data.copy_(saved)  # noqa: E731
    action = torch.zeros(W, dtype=torch.float32, device=dev)
    value = torch.linspace(-1.0, 1.0, W, dtype=torch.float64, device=dev)
    res = dict(nodes=n, workers=W, tree_depth=depth)
    res["select_ms"] = timed(lambda: t.select(9, (4, 1), 1.0), reps)
    leaf, expand = t.select(9, (4, 1), 1.0)
    res["widening_workers"] = int(expand.sum())
    res["expand_ms"] = timed(lambda: t.expand(action), reps, before=restore)
    res["backup_ms"] = timed(lambda: t.backup(value), reps, before=restore)
    restore()
    res["select_no_widening_ms"] = timed(lambda: t.select(9, (1, 1 << 15), 1.0), reps)
    res["select_c0_ms"] = timed(lambda: t.select(9, (4, 1), 0.0), reps)
    res["round_ms"] = res["select_ms"] + res["expand_ms"] + res["backup_ms"]
    return res


def bench_env(W, dev, rounds):
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), W, device=dev)
    ts = TreeSearch(env, 4 * W, max_children=2 * FAN, widen=(4, 1), c_explore=50.0)
    g = torch.Generator(device=dev).manual_seed(5)
    lim = float(np.deg2rad(30))
    policy = lambda obs: (torch.rand(W, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0) * lim  # noqa: E731
    spans = []

    def wrap(name):
        inner = getattr(ts.tree, name)

        def call(*a, **k):
            e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e[0].record()
            out = inner(*a, **k)
            e[1].record()
            spans.append(e)
            return out

        setattr(ts.tree, name, call)

    for name in ("select", "expand", "backup"):
        wrap(name)
    ts.round(policy, policy)  # warm-up: allocations
    per_round = []
    for _ in range(rounds):
        spans.clear()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = ts.round(policy, policy)
        b.record()
        b.synchronize()
        tree_ms = sum(x.elapsed_time(y) for x, y in spans)
        per_round.append((a.elapsed_time(b), tree_ms, int(out["ticks"].sum())))
    res = dict(workers=W, rounds=rounds, nodes_after=ts.tree.n_nodes,
               round_ms=statistics.median(r[0] for r in per_round), tree_ms=statistics.median(r[1] for r in per_round),
               env_ticks_per_round=statistics.median(r[2] for r in per_round))
    res["env_ms"] = res["round_ms"] - res["tree_ms"]
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_search.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_bench.py needs a HIP device")
    dev = torch.device("cuda", 0)
    envs = {W: bench_env(W, dev, args.rounds) for W in (4096, 65536)}
    ops = []
    for n in (1 << 16, 1 << 20):
        for W in (4096, 65536):
            r = bench_ops(n, W, dev, args.reps)
            r["env_ms_same_workers"] = envs[W]["env_ms"]
            r["share_of_round"] = r["round_ms"] / (r["round_ms"] + envs[W]["env_ms"])
            ops.append(r)
            print(json.dumps(r), flush=True)
    res = dict(device=torch.cuda.get_device_name(dev), fan_out=FAN, max_children=2 * FAN, reps=args.reps, collav="sbmpc", obstacle_ships=1,
               note="times in ms, medians; share_of_round = tree / (tree + env launches of a round of as many workers)",
               operations=ops, env_rounds=list(envs.values()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(env_rounds=res["env_rounds"])))


if __name__ == "__main__":
    main()
