"""What a splitting step costs next to the fork it ends in: shipsim_resample in both arrangements (the C call), and
BatchedMultiShipRLEnv.split (resample in place, the caller's stream arrays gathered, the fork), timed in the same
process as shipsim_fork with a random permutation and as one 1024-tick shipsim_run_table launch on the same handle.
sbmpc, 16 lanes per env, launch tail off, K = 1; 4096 and 65,536 envs. The windows are fork_bench.py's: every
operation three times, alternating inside each repetition, each window at least 0.5 s of back-to-back calls after
warm-up and closed by a device synchronise. Weights 1 / n with a fifth zeroed and potentials exp(-30 u), the tests'
inputs: the mass is concentrated, so most slots change hands in a split (the count is recorded), more than in a run
of the estimator. Writes profiles/resample.json.

    python scripts/resample_bench.py [--out FILE] [--reps R] [--envs 4096,65536]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ast_sac_amd import shipsim, shipsim_abi as abi  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv  # noqa: E402
from fork_bench import TICKS, WARMUP, WINDOW_S, _stats, _time  # noqa: E402


def _shape(dev, n, reps):
    cfg = abi.ast_config("sbmpc", machinery=abi.MACH_DETAILED)
    cfg.lanes_per_env = 16
    env = BatchedMultiShipRLEnv(n_envs=n, cfg=cfg, device=dev)
    sim = env.sim
    sim.reset()
    sim.set_stream_tail(0)
    n_dec = int(cfg.max_sampling_frequency)
    gen = np.random.Generator(np.random.PCG64(20251015))
    table = torch.from_numpy(abi.normalized_to_scoping(gen.uniform(-1, 1, (8, n_dec, n)).astype(np.float32))).to(dev)
    ep = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n, dtype=torch.int32, device=dev)
    out = dict(ticks=torch.zeros(n, dtype=torch.int32, device=dev),
               decisions=torch.zeros(n, dtype=torch.int32, device=dev))
    perm = torch.from_numpy(gen.permutation(n).astype(np.int32)).to(dev)
    w = np.full(n, 1.0 / n)
    w[gen.random(n) < 0.2] = 0.0
    weight = torch.from_numpy(w).to(dev)
    potential = torch.from_numpy(np.exp(-30.0 * gen.random(n))).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    wout = torch.empty(n, dtype=torch.float64, device=dev)
    L, h = sim.L, sim.h
    need = int(L.shipsim_resample_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nbytes = sim.state_bytes

    def chk(rc):
        if rc:
            raise SystemExit(f"resample_bench.py: call failed ({rc}): {L.shipsim_last_error(h).decode()}")

    def resample(arrangement):
        return lambda: chk(L.shipsim_resample(n, p(weight), p(potential), 7, p(counter), arrangement, p(ws), need,
                                              p(src), p(wout), p(total), p(status), stream))

    # (resample and fork as the C calls themselves, split as the Python method a caller uses: its binding's checks
    # and the three torch gathers of fork_stream_state are part of what it costs)
    ops = dict(
        launch=lambda: sim.run_table(table, TICKS, ep, dec, out=out),
        fork_permutation=lambda: chk(L.shipsim_fork(h, None, nbytes, p(perm))),
        resample_sorted=resample(shipsim.RESAMPLE_SORTED),
        resample_in_place=resample(shipsim.RESAMPLE_IN_PLACE),
        split=lambda: env.split(weight, potential, 7, counter, ep, dec),
    )
    runs = {name: [] for name in ops}
    calls, windows = {name: [] for name in ops}, {name: [] for name in ops}
    try:
        sim.run_table(table, TICKS, ep, dec, out=out)  # the envs under way before anything is timed
        sim.fork(perm)                                 # (and the staging block allocated)
        for rep in range(reps):
            sim.reset()
            ep.zero_()
            dec.zero_()
            for name, call in ops.items():
                sec, k, window = _time(call, dev)
                runs[name].append(sec)
                calls[name].append(k)
                windows[name].append(window)
                print(f"[resample] {n} envs rep {rep} {name:18s}: {sec * 1e6:10.1f} us x {k} ({window:.3f} s)",
                      flush=True)
        resample(shipsim.RESAMPLE_IN_PLACE)()
        sim.synchronize()
        moved = int((src != torch.arange(n, dtype=torch.int32, device=dev)).sum())
        ok = int(status[0]) == 0
    finally:
        env.close()
    assert ok and min(min(v) for v in windows.values()) >= WINDOW_S
    res = dict(envs=n, obstacle_ships=1, workspace_bytes=need, state_bytes=nbytes, slots_refilled_per_split=moved,
               calls_per_window=calls, window_seconds=windows,
               seconds={name: dict(runs=v, **_stats(v)) for name, v in runs.items()})
    for name in ("resample_sorted", "resample_in_place", "split"):
        for base in ("fork_permutation", "launch"):  # the ratio inside each repetition
            r = [a / b for a, b in zip(runs[name], runs[base])]
            res[f"{name}_over_{base}"] = dict(runs=r, **_stats(r))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--envs", default="4096,65536")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench.py needs a HIP device: there is no time to report without one")
    dev = torch.device("cuda", 0)
    res = dict(collav="sbmpc", lanes_per_env=16, slice_ticks=TICKS, tail_ticks=0, reps=args.reps, window_s=WINDOW_S,
               warmup_calls=WARMUP, unit="seconds per call", device=torch.cuda.get_device_name(dev),
               build=shipsim.load_library().shipsim_build_info().decode(),
               shapes=[_shape(dev, int(n), args.reps) for n in args.envs.split(",")])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({str(s["envs"]): dict(
        fork_us=s["seconds"]["fork_permutation"]["median"] * 1e6,
        resample_sorted_us=s["seconds"]["resample_sorted"]["median"] * 1e6,
        resample_in_place_us=s["seconds"]["resample_in_place"]["median"] * 1e6,
        split_us=s["seconds"]["split"]["median"] * 1e6, launch_ms=s["seconds"]["launch"]["median"] * 1e3,
        split_over_fork=s["split_over_fork_permutation"]["median"],
        split_over_launch=s["split_over_launch"]["median"]) for s in res["shapes"]}))


if __name__ == "__main__":
    main()
