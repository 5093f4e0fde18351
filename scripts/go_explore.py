"""A worked example of the state archive: Go-Explore on the K = 1 sbmpc table stream.

4096 envs run shipsim_run_table in launches of 256 ticks. After every launch each env names its cell
(BatchedMultiShipRLEnv.relative_cells: where the obstacle ship lies relative to the ship under test, by the number of
waypoints sampled so far) and its score, minus the distance between the two ships (level_distance); the archive keeps,
per cell, the closest approach seen (StateArchive.update, the episode and decision counters carried along). The envs
whose episode ended in the launch do not start over: each draws a filled cell with probability proportional to
1 / sqrt(seen + 1) (torch.multinomial), starts from its state (StateArchive.load) and gets a fresh column of the
action table. The same stream with the same tick budget runs once more without the archive (it fills one of its own,
for the count, and loads nothing). Reported for both legs: the cells filled, the episodes that ended and those that
ended in SHIPSIM_EV_COLLISION. An illustration of the primitive, not an estimator: the restarts carry no weights, so
the counts are not probabilities, and whether the exploration reaches more cells or collisions than the plain stream
is reported, not asserted. Writes profiles/go_explore.json.

    python scripts/go_explore.py [--out FILE] [--envs N] [--launches L] [--ticks T] [--bins B] [--radius R]
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


def run(dev, n, launches, ticks, bins, radius, explore, seed=20251020):
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n, device=dev)
    sim = env.sim
    n_dec = int(env.cfg.max_sampling_frequency)
    gen = np.random.Generator(np.random.PCG64(seed))
    table = _columns(gen, 8, n_dec, n).to(dev)
    fresh = np.random.Generator(np.random.PCG64(seed + 1))  # the restarted envs' columns
    torch.manual_seed(seed)
    ep = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n, dtype=torch.int32, device=dev)
    log = torch.zeros((n, CAP, abi.DECLOG_COLS), dtype=torch.float64, device=dev)
    ln = torch.zeros(n, dtype=torch.int32, device=dev)
    row = torch.arange(CAP, device=dev)[None, :]
    arch = env.archive(env.relative_cells_count(bins))
    episodes = collisions = dropped = restarts = 0
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
        ended = (done | last).any(dim=1)
        episodes += int((done | last).sum())
        collisions += int((done & ((ev & abi.EV_COLLISION) != 0)).sum())
        dropped += int((ln - ln.clamp(max=CAP)).sum())
        dist = env.level_distance()
        nearest.append(float(dist.min()))
        arch.update(env.relative_cells(bins, radius), -dist, carry=dict(ep_idx=ep, dec_idx=dec))
        if explore:
            filled = ~torch.isnan(arch.cell_score)
            p = torch.where(filled, 1.0 / torch.sqrt(arch.cell_seen.double() + 1.0), 0.0)
            pick = torch.multinomial(p, n, replacement=True).int()
            cell_of_env = torch.where(ended, pick, -1)  # (-1: the env goes on as it is)
            arch.load(cell_of_env, carry=dict(ep_idx=ep, dec_idx=dec))
            k = int(ended.sum())
            if k:
                table[:, :, ended] = _columns(fresh, 8, n_dec, k).to(dev)
            restarts += k
    sim.synchronize()
    dt = time.perf_counter() - t0
    cells = int((~torch.isnan(arch.cell_score)).sum())
    best = float(-arch.cell_score[~torch.isnan(arch.cell_score)].max())
    env.close()
    return dict(explore=bool(explore), cells_filled=cells, cells=arch.n_cells, episodes_ended=episodes,
                collision_episodes=collisions, records_dropped=dropped, restarts_from_cells=restarts,
                nearest_approach_m=min(nearest), nearest_archived_m=best, seconds=dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "go_explore.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=64)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--radius", type=float, default=8000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("go_explore.py needs a HIP device")
    dev = torch.device("cuda", 0)
    legs = [run(dev, args.envs, args.launches, args.ticks, args.bins, args.radius, e) for e in (False, True)]
    res = dict(envs=args.envs, collav="sbmpc", obstacle_ships=1, launches=args.launches, ticks_per_launch=args.ticks,
               bins=args.bins, radius_m=args.radius, env_ticks_budget=args.envs * args.launches * args.ticks,
               device=torch.cuda.get_device_name(dev),
               note="unweighted restarts: the counts illustrate the exploration and are not probabilities",
               plain=legs[0], go_explore=legs[1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(plain=legs[0], go_explore=legs[1])))


if __name__ == "__main__":
    main()
