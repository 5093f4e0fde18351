"""Times select over a forest next to select over one tree. Writes profiles/forest_search.json.

Forests: R complete trees in one pool of 2^20 nodes, grown the way scripts/tree_bench.py grows its tree (16 children per
inner node out of max_children = 32, visits the subtree sizes, seeded mean values in [-1, 1]), breadth-first over the
whole forest: the roots are nodes 0..R-1, and R = 1 is tree_bench's tree node for node. Per W in {4096, 65536}:
shipsim_tree_select on the one tree (the code of the parent commit, timed before and after the forests: the run's own
spread), and for R in {1, 64, 1024, W} and root_workers even, all on root 0 or all on root 1 (a root that backup does
not combine per wave): shipsim_tree_select_forest, then expand (of that select's workers) and backup (of that expand's
nodes), each the median of `--reps` timed calls between device events with the least and the most beside it. The
buffer is put back before every expand as it was before the select, and before every backup as that expand left it
(the new nodes in the tree, so that their backups are taken); beside backup's time are the backups taken (W less the
change of the header's skipped count) and the most that one root took (the change of its visits).

    python scripts/forest_bench.py [--out FILE] [--reps R]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ast_sac_amd.shipsim import SearchTree  # noqa: E402

FAN = 16
NODES = 1 << 20


def complete_forest(n, R, W, dev, seed=1):
    """A SearchTree whose first n nodes are R complete FAN-ary trees, breadth-first over the forest: level d holds
    R * FAN^d nodes, and child k of the j-th node of a level is the (j * FAN + k)-th of the next."""
    t = SearchTree(n + W, 2 * FAN, W, n_roots=R, device=dev)
    i = torch.arange(n, device=dev)
    depth = torch.zeros(n, dtype=torch.int64, device=dev)
    lo_of = []
    lo, d = 0, 0
    while lo < n:  # level d holds ids [lo, lo + R * FAN^d)
        depth[lo:lo + R * FAN ** d] = d
        lo_of.append(lo)
        lo, d = lo + R * FAN ** d, d + 1
    lo_of.append(lo)
    lo_t = torch.tensor(lo_of, device=dev)
    j = i - lo_t[depth]
    first = lo_t[depth + 1] + j * FAN
    parent = torch.where(depth > 0, lo_t[(depth - 1).clamp(min=0)] + j // FAN, -1)
    nc = (n - first).clamp(0, FAN)
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
    """(median, least, most) of `reps` timed calls, in ms."""
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
    return statistics.median(ms), min(ms), max(ms)


def put(res, name, t3):
    res[name + "_ms"], res[name + "_min_ms"], res[name + "_max_ms"] = t3


def bench_tree(W, dev):
    t, depth = complete_forest(NODES, 1, W, dev)
    assert t.n_roots == 1 and int(t.header[3]) == 0  # shipsim_tree_init's tree: select takes shipsim_tree_select
    t.select(9, (4, 1), 1.0)
    return t, depth


def bench_forest(R, W, dev, reps, split):
    t, depth = complete_forest(NODES, R, W, dev)
    saved = t.data.clone()
    restore = lambda: t.data.copy_(saved)  # noqa: E731
    action = torch.zeros(W, dtype=torch.float32, device=dev)
    value = torch.linspace(-1.0, 1.0, W, dtype=torch.float64, device=dev)
    if split == "even":
        rw = t.even_workers.clone()
    else:  # all on root 0, or all on root 1
        rw = torch.zeros(R, dtype=torch.int32, device=dev)
        rw[int(split[-1])] = W
    res = dict(roots=R, workers=W, nodes=NODES, split=split, tree_depth=depth, most_arrivals_at_a_root=int(rw.max()))
    sel = lambda: t.select(9, (4, 1), 1.0, root_workers=rw)  # noqa: E731  (R = 1 too: the forest call)
    sel()
    put(res, "select_forest", timed(sel, reps))
    leaf, expand = sel()
    res["widening_workers"] = int(expand.sum())
    res["workers_without_a_leaf"] = int((leaf < 0).sum())
    put(res, "expand", timed(lambda: t.expand(action), reps, before=restore))
    # backup on the buffer as expand left it: the new nodes are in the tree and their backups are taken
    restore()
    sel()
    node = t.expand(action).clone()
    after = t.data.clone()
    put(res, "backup", timed(lambda: t.backup(value, node=node), reps, before=lambda: t.data.copy_(after)))
    t.data.copy_(after)
    skipped, visits = int(t.header[2]), t.visits[:R].clone()
    t.backup(value, node=node)
    res["backups_taken"] = W - (int(t.header[2]) - skipped)
    res["most_backups_at_a_root"] = int((t.visits[:R] - visits).max())
    res["new_nodes"] = int((node >= NODES).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_search.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("forest_bench.py needs a HIP device")
    dev = torch.device("cuda", 0)
    rows, trees = [], []
    for W in (4096, 65536):
        t, depth = bench_tree(W, dev)
        base = dict(workers=W, nodes=NODES, tree_depth=depth)
        put(base, "select_before", timed(lambda: t.select(9, (4, 1), 1.0), args.reps))
        for R in (1, 64, 1024, W):
            for split in ("even", "all_on_root_0", "all_on_root_1"):
                if R == 1 and split != "even":
                    continue
                r = bench_forest(R, W, dev, args.reps, split)
                rows.append(r)
                print(json.dumps(r), flush=True)
        put(base, "select_after", timed(lambda: t.select(9, (4, 1), 1.0), args.reps))
        base["select_ms"] = 0.5 * (base["select_before_ms"] + base["select_after_ms"])
        trees.append(base)
        print(json.dumps(base), flush=True)
    res = dict(device=torch.cuda.get_device_name(dev), fan_out=FAN, max_children=2 * FAN, reps=args.reps,
               note="times in ms: medians, with the least and the most of the reps; tree_select: shipsim_tree_select on the "
                    "one tree of as many nodes, timed before and after the forests of the same W",
               tree_select=trees, forests=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
