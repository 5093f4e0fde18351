"""What it costs to move per-env weather with the state: BatchedMultiShipRLEnv.fork under weather = keep / carry /
follow and split under keep / carry, each as an eager call and (where it can be captured: not "follow", which copies
the indices to the host and uploads) as the replay of a captured graph, at 4096 and 65,536 two-ship sbmpc envs under
sampled per-env weather; and StateArchive.update + load with and without weather at 65,536 envs / 16,384 cells.

Timed the way scripts/fork_bench.py times a fork: warm-up calls of the same shape, then a window of calls back to back
that lasts at least 0.5 s and is closed by a device synchronise (a time is what one more call adds to a stream that
is kept busy, enqueue included); every operation three times, the operations alternating inside each repetition.
Writes medians, spreads and the carry : keep ratios to profiles/weather_carry.json. Nothing is
asserted: these are the first measurements of these calls.

    python scripts/weather_carry_bench.py [--out FILE] [--reps R] [--envs 4096,65536]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ast_sac_amd import shipsim  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.weather import sample_weather  # noqa: E402

WINDOW_S = 0.5
WARMUP = 3
TICKS = 256
SEED = 20251015
RANGES = dict(wind_speed=(0, 12), wind_direction_deg=(-180, 180), current_speed=(0, 1.5),
              current_direction_deg=(-180, 180))
ARCHIVE_ENVS, ARCHIVE_CELLS = 65536, 16384


def _window(call, dev, n):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def _time(call, dev, min_calls=3):
    """(seconds per call, calls, seconds of the window): scripts/fork_bench.py's procedure."""
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


def _graph(body, dev):
    """`body` captured once into a graph on a side stream; the call that replays it."""
    body()  # eager once: what allocates does so before the capture
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            body()
    torch.cuda.synchronize(dev)
    return g.replay, g


def _run(ops, reps, dev, tag):
    runs = {name: [] for name in ops}
    calls, windows = {name: [] for name in ops}, {name: [] for name in ops}
    for rep in range(reps):
        for name, call in ops.items():
            sec, n, window = _time(call, dev)
            runs[name].append(sec)
            calls[name].append(n)
            windows[name].append(window)
            print(f"[weather-carry] {tag} rep {rep} {name:24s}: {sec * 1e6:10.1f} us x {n} ({window:.3f} s)", flush=True)
    assert min(min(w) for w in windows.values()) >= WINDOW_S
    return dict(calls_per_window=calls, window_seconds=windows,
                seconds={name: dict(runs=v, **_stats(v)) for name, v in runs.items()}), runs


def _ratio(runs, a, b):
    r = [x / y for x, y in zip(runs[a], runs[b])]  # inside each repetition: its windows ran back to back
    return dict(runs=r, **_stats(r))


def _env(n, dev):
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n, device=dev,
                                weather=sample_weather(n, seed=SEED, **RANGES))
    n_dec = int(env.cfg.max_sampling_frequency)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    lim = float(np.deg2rad(30))
    table = (torch.rand((2, n_dec, n), generator=gen, device=dev, dtype=torch.float32) * 2 - 1) * lim
    ep = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n, dtype=torch.int32, device=dev)
    env.reset()
    env.sim.run_table(table, TICKS, ep, dec)  # the envs under way, mid-decision, before anything is timed
    env.sim.synchronize()
    return env, ep, dec


def bench_fork_split(n, dev, reps):
    env, ep, dec = _env(n, dev)
    sim = env.sim
    gen = np.random.Generator(np.random.PCG64(SEED))
    perm = torch.from_numpy(gen.permutation(n).astype(np.int32)).to(dev)
    weight = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
    potential = torch.exp(-sim.level_distance() / 1500.0)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    sim.fork(perm)  # the state fork's staging block exists
    ops, keep = {}, []
    for mode in ("keep", "carry", "follow"):
        ops[f"fork_{mode}_eager"] = lambda mode=mode: env.fork(perm, weather=mode)
    for mode in ("keep", "carry"):
        ops[f"fork_{mode}_graph"], g = _graph(lambda mode=mode: env.fork(perm, weather=mode), dev)
        keep.append(g)
    for mode in ("keep", "carry"):
        body = lambda mode=mode: env.split(weight, potential, SEED, counter, ep, dec, weather=mode)  # noqa: E731
        ops[f"split_{mode}_eager"] = body
        ops[f"split_{mode}_graph"], g = _graph(body, dev)
        keep.append(g)
    try:
        res, runs = _run(ops, reps, dev, f"{n} envs")
        sim.synchronize()
    finally:
        env.close()
    res.update(envs=n, obstacle_ships=1, lanes_per_env=env.sim.lanes_per_env)
    for what in ("fork", "split"):
        for how in ("eager", "graph"):
            res[f"{what}_carry_over_keep_{how}"] = _ratio(runs, f"{what}_carry_{how}", f"{what}_keep_{how}")
    res["fork_follow_over_keep_eager"] = _ratio(runs, "fork_follow_eager", "fork_keep_eager")
    res["fork_follow_over_carry_eager"] = _ratio(runs, "fork_follow_eager", "fork_carry_eager")
    res["fork_carry_minus_keep_graph_us"] = 1e6 * (res["seconds"]["fork_carry_graph"]["median"]
                                                   - res["seconds"]["fork_keep_graph"]["median"])
    return res


def bench_archive(dev, reps):
    n, m = ARCHIVE_ENVS, ARCHIVE_CELLS
    env, ep, dec = _env(n, dev)
    gen = torch.Generator(device=dev).manual_seed(SEED + 1)
    cell = torch.randint(0, m, (n,), generator=gen, device=dev, dtype=torch.int32)
    score = torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    cell_of_env = torch.randint(0, m, (n,), generator=gen, device=dev, dtype=torch.int32)
    ops = {}
    for name, flag in (("update_load_state", False), ("update_load_state_weather", True)):
        arch = env.archive(m, weather=flag)

        def body(arch=arch):
            arch.cell_score.fill_(float("nan"))  # every cell empty again: each call stores every elected env
            arch.update(cell, score)
            arch.load(cell_of_env)

        ops[name] = body
    try:
        res, runs = _run(ops, reps, dev, f"archive {n} envs / {m} cells")
        env.sim.synchronize()
    finally:
        env.close()
    res.update(envs=n, cells=m, obstacle_ships=1)
    res["weather_over_state"] = _ratio(runs, "update_load_state_weather", "update_load_state")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weather_carry.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--envs", default="4096,65536", help="comma list of env counts for fork and split")
    ap.add_argument("--no-archive", action="store_true", help="skip the archive measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weather_carry_bench.py needs a HIP device: there is no time to report without one")
    dev = torch.device("cuda", 0)
    res = dict(collav="sbmpc", reps=args.reps, window_s=WINDOW_S, warmup_calls=WARMUP, unit="seconds per call",
               device=torch.cuda.get_device_name(dev), build=shipsim.load_library().shipsim_build_info().decode(),
               weather_ranges={k: list(v) for k, v in RANGES.items()},
               note="eager: the Python call, enqueue included, on a stream kept busy; graph: the replay of the same "
                    "call captured once ('follow' cannot be captured: it copies the indices to the host, uploads and "
                    "waits). Reported, not asserted.",
               shapes=[bench_fork_split(int(n), dev, args.reps) for n in args.envs.split(",")])
    if not args.no_archive:
        res["archive"] = bench_archive(dev, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    line = {str(s["envs"]): {k: round(s["seconds"][k]["median"] * 1e6, 2) for k in s["seconds"]} for s in res["shapes"]}
    if "archive" in res:
        line["archive"] = {k: round(v["median"] * 1e6, 2) for k, v in res["archive"]["seconds"].items()}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
