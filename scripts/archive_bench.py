"""What the state archive costs: shipsim_archive_store and shipsim_archive_load under random index arrays,
shipsim_archive_elect with the envs spread over the cells and with every env in one cell (the most contended
atomics), and StateArchive.update (the Python method: elect, then store of what was elected), timed in the same
process as the yardsticks — shipsim_fork from a snapshot under a random permutation and shipsim_resample in place.
sbmpc, 16 lanes per env, K = 1; 4096 and 65,536 envs, each with n_envs / 4 and 4 x n_envs cells. The windows are
fork_bench.py's: every operation `reps` times, alternating inside each repetition, each window at least 0.5 s of
back-to-back calls after warm-up and closed by a device synchronise. The cells are emptied before every window of an
election (its later calls find them held, which costs the same launches) and before every call of update (one fill
kernel more), so that each update stores what it elected. Writes profiles/archive.json.

    python scripts/archive_bench.py [--out FILE] [--reps R] [--envs 4096,65536]
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


def _shape(dev, n, m, reps):
    cfg = abi.ast_config("sbmpc", machinery=abi.MACH_DETAILED)
    cfg.lanes_per_env = 16
    env = BatchedMultiShipRLEnv(n_envs=n, cfg=cfg, device=dev)
    sim = env.sim
    sim.reset()
    sim.set_stream_tail(0)
    n_dec = int(cfg.max_sampling_frequency)
    gen = np.random.Generator(np.random.PCG64(20251020))
    table = torch.from_numpy(abi.normalized_to_scoping(gen.uniform(-1, 1, (8, n_dec, n)).astype(np.float32))).to(dev)
    ep = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n, dtype=torch.int32, device=dev)
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)  # noqa: E731
    env_of_cell = i32(gen.integers(0, n, m))
    cell_of_env = i32(gen.integers(0, m, n))
    spread = i32(gen.integers(0, m, n))
    one_cell = torch.full((n,), m // 2, dtype=torch.int32, device=dev)
    score = torch.from_numpy(gen.normal(size=n)).to(dev)
    perm = i32(gen.permutation(n))
    weight = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
    potential = torch.from_numpy(np.exp(-30.0 * gen.random(n))).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    wout = torch.empty(n, dtype=torch.float64, device=dev)
    L, h = sim.L, sim.h
    rs_need = int(L.shipsim_resample_workspace_bytes(n))
    rs_ws = torch.empty(rs_need, dtype=torch.uint8, device=dev)
    arch = env.archive(m)
    nb, ws_need = arch.data.numel(), arch.workspace.numel()
    eoc = torch.empty(m, dtype=torch.int32, device=dev)
    k_out = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    state_bytes = sim.state_bytes

    def chk(rc):
        if rc:
            raise SystemExit(f"archive_bench.py: call failed ({rc}): {L.shipsim_last_error(h).decode()}")

    def elect(cell):
        return lambda: chk(L.shipsim_archive_elect(n, m, p(cell), p(score), p(arch.cell_score), p(arch.cell_seen),
                                                   p(arch.workspace), ws_need, p(eoc), p(k_out), stream))

    sim.run_table(table, TICKS, ep, dec)  # the envs under way before anything is timed
    snap = sim.snapshot()
    ops = dict(
        store=lambda: chk(L.shipsim_archive_store(h, p(arch.data), nb, m, p(env_of_cell))),
        load=lambda: chk(L.shipsim_archive_load(h, p(arch.data), nb, m, p(cell_of_env))),
        elect_spread=elect(spread),
        elect_one_cell=elect(one_cell),
        update=lambda: (arch.cell_score.fill_(float("nan")), arch.update(spread, score)),
        fork_snapshot=lambda: chk(L.shipsim_fork(h, p(snap.data), state_bytes, p(perm))),
        resample_in_place=lambda: chk(L.shipsim_resample(n, p(weight), p(potential), 7, p(counter), 1, p(rs_ws), rs_need,
                                                         p(src), p(wout), None, None, stream)),
    )
    runs = {name: [] for name in ops}
    calls, windows = {name: [] for name in ops}, {name: [] for name in ops}
    try:
        arch.store(gen.integers(0, n, m))  # every cell holds a state before a load is timed
        for rep in range(reps):
            for name, call in ops.items():
                arch.cell_score.fill_(float("nan"))
                sec, k, window = _time(call, dev)
                runs[name].append(sec)
                calls[name].append(k)
                windows[name].append(window)
                print(f"[archive] {n} envs {m} cells rep {rep} {name:18s}: {sec * 1e6:10.1f} us x {k} ({window:.3f} s)",
                      flush=True)
        sim.synchronize()
    finally:
        env.close()
    assert min(min(v) for v in windows.values()) >= WINDOW_S
    res = dict(envs=n, cells=m, obstacle_ships=1, archive_bytes=nb, workspace_bytes=ws_need, state_bytes=state_bytes,
               calls_per_window=calls, window_seconds=windows,
               seconds={name: dict(runs=v, **_stats(v)) for name, v in runs.items()})
    for name, base in (("store", "fork_snapshot"), ("load", "fork_snapshot"), ("update", "fork_snapshot"),
                       ("elect_spread", "resample_in_place"), ("elect_one_cell", "elect_spread")):
        r = [a / b for a, b in zip(runs[name], runs[base])]  # the ratio inside each repetition
        res[f"{name}_over_{base}"] = dict(runs=r, **_stats(r))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--envs", default="4096,65536")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("archive_bench.py needs a HIP device: there is no time to report without one")
    dev = torch.device("cuda", 0)
    shapes = [_shape(dev, n, m, args.reps) for n in map(int, args.envs.split(",")) for m in (n // 4, 4 * n)]
    res = dict(collav="sbmpc", lanes_per_env=16, reps=args.reps, window_s=WINDOW_S, warmup_calls=WARMUP,
               unit="seconds per call", device=torch.cuda.get_device_name(dev),
               build=shipsim.load_library().shipsim_build_info().decode(), shapes=shapes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({f"{s['envs']}x{s['cells']}": {k: round(v["median"] * 1e6, 2) for k, v in s["seconds"].items()}
                      for s in shapes}))


if __name__ == "__main__":
    main()
