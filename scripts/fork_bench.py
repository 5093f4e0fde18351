"""What a fork costs next to what it forks: shipsim_fork (a random permutation and a broadcast, both from the live
state: one gather launch through the staging block and one copy back), shipsim_snapshot and shipsim_restore, timed in
the same process as a plain hipMemcpyAsync of the same block and as one 1024-tick shipsim_run_table launch on the same
handle. sbmpc, 16 lanes per env, launch tail off; 4096 and 65,536 envs at K = 1 obstacle ship and 4096 envs at K = 4.
Every operation is timed three times, the operations alternating inside each repetition, each window at least 0.5 s
of back-to-back calls after warm-up calls of the same shape and closed by a device synchronise (so a time is what one
more call adds to a stream that is kept busy, enqueue included); the seconds every window lasted are recorded. A
splitting loop forks once per launch: the condition is that a fork costs under 1 % of the launch measured here.
Writes medians and spreads, the fork : launch and fork : copy ratios and the condition to profiles/fork.json
(DESIGN.md §9).

    python scripts/fork_bench.py [--out FILE] [--reps R] [--shapes 4096x1,65536x1,4096x4]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ast_sac_amd import shipsim_abi as abi  # noqa: E402
from ast_sac_amd.shipsim import ShipSim  # noqa: E402

TICKS = 1024
WINDOW_S = 0.5
WARMUP = 3
HIP_MEMCPY_D2D = 3  # hipMemcpyDeviceToDevice


def _hip_runtime():
    """The HIP runtime this process already runs on (the one torch loaded), for the plain hipMemcpyAsync."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        raise SystemExit("fork_bench.py: no libamdhip64 in this process")
    lib = C.CDLL(sorted(paths)[0])
    lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.hipMemcpyAsync.restype = C.c_int
    return lib


def _window(call, dev, n):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def _time(call, dev, min_calls=3):
    """(seconds per call, calls, seconds of the window): WARMUP calls, then one window of calls back to back, closed
    by a synchronise, that lasts at least WINDOW_S. Three calls and their synchronise overstate a short asynchronous
    call several times over, so the count is sized from pilot windows, each 8x the last until one lasts a tenth of
    WINDOW_S, and a window that still ends early is not kept: it is run again with more calls."""
    _window(call, dev, WARMUP)
    n = max(min_calls, 8)
    dt = _window(call, dev, n)
    while dt < 0.1 * WINDOW_S:
        n *= 8
        dt = _window(call, dev, n)
    while True:
        n = max(min_calls, int(math.ceil(1.1 * WINDOW_S * n / dt)))
        dt = _window(call, dev, n)
        if dt >= WINDOW_S:
            return dt / n, n, dt


def _stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return dict(median=med, min=xs[0], max=xs[-1], spread=(xs[-1] - xs[0]) / med)


def _shape(dev, hip, n_envs, k, reps):
    cfg = abi.ast_config("sbmpc", machinery=abi.MACH_DETAILED, n_obs_ships=k)
    cfg.lanes_per_env = 16
    sim = ShipSim(cfg, n_envs, device=dev)
    sim.reset()
    sim.set_stream_tail(0)
    n_dec = int(cfg.max_sampling_frequency)
    gen = np.random.Generator(np.random.PCG64(20251015))
    table = torch.from_numpy(abi.normalized_to_scoping(
        gen.uniform(-1, 1, (8, n_dec, n_envs)).astype(np.float32))).to(dev)
    ep = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    dec = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    out = dict(ticks=torch.zeros(n_envs, dtype=torch.int32, device=dev),
               decisions=torch.zeros(n_envs, dtype=torch.int32, device=dev))
    perm = torch.from_numpy(gen.permutation(n_envs).astype(np.int32)).to(dev)
    one = torch.full((n_envs,), n_envs // 3, dtype=torch.int32, device=dev)
    nbytes = sim.state_bytes
    snap = sim.snapshot()
    other = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L, h = sim.L, sim.h
    perm_p, one_p = C.c_void_p(perm.data_ptr()), C.c_void_p(one.data_ptr())
    snap_p, other_p = C.c_void_p(snap.data.data_ptr()), C.c_void_p(other.data_ptr())

    def chk(rc):
        if rc:
            raise SystemExit(f"fork_bench.py: call failed ({rc}): {L.shipsim_last_error(h).decode()}")

    # (the C calls themselves: the cost of the binding's argument checks is not the library's)
    ops = dict(
        launch=lambda: sim.run_table(table, TICKS, ep, dec, out=out),
        fork_permutation=lambda: chk(L.shipsim_fork(h, None, nbytes, perm_p)),
        fork_broadcast=lambda: chk(L.shipsim_fork(h, None, nbytes, one_p)),
        fork_from_snapshot=lambda: chk(L.shipsim_fork(h, snap_p, nbytes, perm_p)),
        snapshot=lambda: chk(L.shipsim_snapshot(h, snap_p, nbytes)),
        restore=lambda: chk(L.shipsim_restore(h, snap_p, nbytes)),
        memcpy=lambda: chk(hip.hipMemcpyAsync(other_p, snap_p, nbytes, HIP_MEMCPY_D2D, stream)),
    )
    runs = {name: [] for name in ops}
    calls, windows = {name: [] for name in ops}, {name: [] for name in ops}
    try:
        sim.run_table(table, TICKS, ep, dec, out=out)  # the envs under way, mid-decision, before anything is timed
        sim.fork(perm)                                 # (and the staging block allocated)
        for rep in range(reps):
            # the launch (first in the order) runs episodes from their start, with the caller's counters to match;
            # nothing after it in the repetition steps the states it shuffles
            sim.reset()
            ep.zero_()
            dec.zero_()
            for name, call in ops.items():
                sec, n, window = _time(call, dev)
                runs[name].append(sec)
                calls[name].append(n)
                windows[name].append(window)
                print(f"[fork] {n_envs} envs K={k} rep {rep} {name:18s}: {sec * 1e6:10.1f} us x {n} "
                      f"({window:.3f} s)", flush=True)
        sim.synchronize()
    finally:
        sim.close()
    assert min(min(w) for w in windows.values()) >= WINDOW_S
    res = dict(envs=n_envs, obstacle_ships=k, state_bytes=nbytes, calls_per_window=calls, window_seconds=windows,
               seconds={name: dict(runs=v, **_stats(v)) for name, v in runs.items()})
    for name in ("fork_permutation", "fork_broadcast", "fork_from_snapshot", "snapshot", "restore"):
        for base in ("launch", "memcpy"):  # the ratio inside each repetition (its windows ran back to back)
            r = [a / b for a, b in zip(runs[name], runs[base])]
            res[f"{name}_over_{base}"] = dict(runs=r, **_stats(r))
    worst = max(max(res["fork_permutation_over_launch"]["runs"]), max(res["fork_broadcast_over_launch"]["runs"]))
    res["worst_fork_over_launch"] = worst
    res["fork_under_1_percent_of_launch"] = bool(worst < 0.01)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fork.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="4096x1,65536x1,4096x4", help="comma list of ENVSxK")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fork_bench.py needs a HIP device: there is no time to report without one")
    dev = torch.device("cuda", 0)
    hip = _hip_runtime()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    res = dict(collav="sbmpc", lanes_per_env=16, slice_ticks=TICKS, tail_ticks=0, reps=args.reps, window_s=WINDOW_S,
               warmup_calls=WARMUP, unit="seconds per call", device=torch.cuda.get_device_name(dev),
               shapes=[_shape(dev, hip, n, k, args.reps) for n, k in shapes])
    res["fork_under_1_percent_of_launch"] = all(s["fork_under_1_percent_of_launch"] for s in res["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({f"{s['envs']}x{s['obstacle_ships']}": dict(
        fork_us=s["seconds"]["fork_permutation"]["median"] * 1e6, launch_ms=s["seconds"]["launch"]["median"] * 1e3,
        fork_over_launch=s["fork_permutation_over_launch"]["median"],
        fork_over_memcpy=s["fork_permutation_over_memcpy"]["median"]) for s in res["shapes"]}))
    if not res["fork_under_1_percent_of_launch"]:
        raise SystemExit("fork_bench.py: a fork cost 1 % or more of the 1024-tick launch it was measured against")


if __name__ == "__main__":
    main()
