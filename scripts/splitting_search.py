"""A worked example of fork(): a greedy splitting search for collisions on the K = 1 sbmpc table stream.

4096 envs run shipsim_run_table in launches of 256 ticks. After every launch the envs are ranked by the distance
between the ship under test and the obstacle ship (get_state); the farthest quarter is replaced by clones of the
nearest quarter (ShipSim.fork from the live state, the caller's episode / decision counters gathered with
fork_stream_state), and every clone gets a fresh column of the action table, so that it explores from its source's
state instead of repeating it. The same stream with the same tick budget runs once more without forking. Counted on
both legs: the episodes that ended, and those that ended in SHIPSIM_EV_COLLISION. An illustration of the primitive,
not an estimator: the clones carry no weights, so the counts are not probabilities, and whether the search finds
more collisions than the plain stream is reported, not asserted. Writes profiles/splitting_search.json.

    python scripts/splitting_search.py [--out FILE] [--envs N] [--launches L] [--ticks T]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ast_sac_amd import shipsim_abi as abi  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args  # noqa: E402

CAP = 32  # decision records per env and launch


def _columns(gen, n_eps, n_dec, n):
    return torch.from_numpy(abi.normalized_to_scoping(gen.uniform(-1, 1, (n_eps, n_dec, n)).astype(np.float32)))


def run(dev, n, launches, ticks, split, seed=20251015):
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n, device=dev)
    sim = env.sim
    n_dec = int(env.cfg.max_sampling_frequency)
    gen = np.random.Generator(np.random.PCG64(seed))
    table = _columns(gen, 8, n_dec, n).to(dev)
    fresh = np.random.Generator(np.random.PCG64(seed + 1))  # the clones' columns
    ep = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n, dtype=torch.int32, device=dev)
    log = torch.zeros((n, CAP, abi.DECLOG_COLS), dtype=torch.float64, device=dev)
    ln = torch.zeros(n, dtype=torch.int32, device=dev)
    row = torch.arange(CAP, device=dev)[None, :]
    own = torch.arange(n, dtype=torch.int32, device=dev)
    q = n // 4
    episodes = collisions = dropped = forks = 0
    nearest = []
    env.reset()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(launches):
        ln.zero_()
        sim.run_table(table, ticks, ep, dec, log=log, log_len=ln)
        have = row < ln.clamp(max=CAP)[:, None]
        ev = log[:, :, abi.DL_EVENTS].long()
        done = (log[:, :, abi.DL_DONE] != 0) & have
        last = (log[:, :, abi.DL_DECISION].long() == n_dec - 1) & have  # the episode's last decision ends it too
        episodes += int((done | last).sum())
        collisions += int((done & ((ev & abi.EV_COLLISION) != 0)).sum())
        dropped += int((ln - ln.clamp(max=CAP)).sum())
        pn = sim.get(abi.F_NORTH).view(n, 2)
        pe = sim.get(abi.F_EAST).view(n, 2)
        dist = torch.hypot(pn[:, 0] - pn[:, 1], pe[:, 0] - pe[:, 1])
        order = torch.argsort(dist)
        nearest.append(float(dist[order[0]]))
        if split:
            near, far = order[:q], order[n - q:]
            src = own.clone()
            src[far] = near.int()
            env.fork_stream_state(src, ep, dec)
            env.fork(src)
            table[:, :, far] = _columns(fresh, 8, n_dec, q).to(dev)
            forks += 1
    sim.synchronize()
    dt = time.perf_counter() - t0
    env.close()
    return dict(split=bool(split), episodes_ended=episodes, collision_episodes=collisions, records_dropped=dropped,
                forks=forks, clones_per_fork=q if split else 0, nearest_approach_m=min(nearest), seconds=dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splitting_search.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=64)
    ap.add_argument("--ticks", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splitting_search.py needs a HIP device")
    dev = torch.device("cuda", 0)
    legs = [run(dev, args.envs, args.launches, args.ticks, split) for split in (False, True)]
    res = dict(envs=args.envs, collav="sbmpc", obstacle_ships=1, launches=args.launches, ticks_per_launch=args.ticks,
               env_ticks_budget=args.envs * args.launches * args.ticks, device=torch.cuda.get_device_name(dev),
               note="unweighted clones: the counts illustrate the search and are not probabilities",
               plain=legs[0], splitting=legs[1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(plain=legs[0], splitting=legs[1])))


if __name__ == "__main__":
    main()
