"""A worked example of the search tree: tree search for collisions on the K = 1 sbmpc env.

4096 envs search one tree (TreeSearch: select, archive load, one widening decision, rollout, backup), with uniform
random scoping angles both for a new edge and for the rollout, and the episode's return as the value. The same env then
runs plain uniform-random episodes until it has spent the same number of env ticks. Reported for both legs: the
episodes run, those that ended in SHIPSIM_EV_COLLISION, and the ticks; for the tree also its size, its depth and the
most-visited action sequence. A worker that stays at a terminal leaf takes no decision and counts as no episode. An
illustration, not an estimator: whether the tree finds more collisions than random search is reported, not asserted.
Writes profiles/tree_search_example.json.

--roots R searches a forest: R trees in the one node pool, the envs split evenly over their roots, every root the
reset state (root-parallel search). With a weather range flag, env i draws a weather of its own (weather.py:
sample_weather, seed --weather_seed) and root r is the reset state of env r under env r's weather: one tree per
weather, which needs --roots >= 2 (one tree stands for one weather); the envs beyond the roots draw weathers too, but
sail under the weather of the node they play from their first load on. Reported per root then: its visits and its
most-visited action sequence (visits_per_root, best_path_deg_per_root; root_visits and best_path_deg stay root 0's).
The random leg sails under the same drawn weathers.

    python scripts/tree_search.py [--out FILE] [--envs N] [--rounds R] [--max-nodes M] [--children C] [--roots R]
        [--wind_speed_range LO HI] [--wind_direction_range LO HI] [--current_speed_range LO HI]
        [--current_direction_range LO HI] [--weather_seed S]
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
from ast_sac_amd.rl_env.ship_in_transit.tree_search import TreeSearch  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.weather import sample_weather  # noqa: E402

# the runner's four range flags -> sample_weather's keyword arguments
WEATHER_RANGE_FLAGS = (("wind_speed_range", "wind_speed", "m/s"), ("wind_direction_range", "wind_direction_deg", "degrees"),
                       ("current_speed_range", "current_speed", "m/s"),
                       ("current_direction_range", "current_direction_deg", "degrees"))

LIMIT = float(np.deg2rad(30))


def uniform_policy(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return lambda obs: (torch.rand(n, generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0) * LIMIT


def tree_leg(dev, n, rounds, max_nodes, children, widen, c_explore, seed, roots=1, weather=None):
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n, device=dev, weather=weather)
    ts = TreeSearch(env, max_nodes, max_children=children, widen=widen, c_explore=c_explore, n_roots=roots)
    policy = uniform_policy(n, dev, seed)
    episodes = torch.zeros((), dtype=torch.int64, device=dev)
    collisions, ticks = torch.zeros_like(episodes), torch.zeros_like(episodes)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(rounds):
        out = ts.round(policy, policy)
        episodes += (out["ticks"] > 0).sum()
        collisions += ((out["events"] & abi.EV_COLLISION) != 0).sum()
        ticks += out["ticks"].sum()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    t = ts.tree
    nn = t.n_nodes
    actions, nodes = ts.best_path()
    res = dict(episodes=int(episodes), collision_episodes=int(collisions), env_ticks=int(ticks), rounds=rounds,
               nodes=nn, max_nodes=max_nodes, dropped=int(t.header[1]), skipped=int(t.header[2]),
               depth=int(t.depth[:nn].max()), terminal_nodes=int((t.flags[:nn] & 1).sum()),
               root_visits=int(t.visits[0]), best_path_deg=[float(np.rad2deg(a)) for a in actions],
               best_path_visits=[int(t.visits[v]) for v in nodes], seconds=dt)
    if roots > 1:
        res["roots"] = roots
        res["visits_per_root"] = t.visits[:roots].cpu().tolist()
        res["best_path_deg_per_root"] = [[float(np.rad2deg(a)) for a in ts.best_path(root=r)[0]] for r in range(min(roots, 16))]
    env.close()
    return res


def random_leg(dev, n, tick_budget, seed, weather=None):
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc"), n, device=dev, weather=weather)
    policy = uniform_policy(n, dev, seed)
    n_dec = int(env.cfg.max_sampling_frequency)
    episodes = collisions = ticks = 0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    while ticks < tick_budget:
        obs = env.reset()
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        events = torch.zeros(n, dtype=torch.int32, device=dev)
        spent = torch.zeros(n, dtype=torch.int64, device=dev)
        for _ in range(n_dec):
            obs, _, d, info = env.step(policy(obs), active=alive)
            events |= torch.where(alive, info["events"], 0)
            spent += torch.where(alive, info["ticks"], 0)
            alive = alive & ~d
        episodes += n
        collisions += int(((events & abi.EV_COLLISION) != 0).sum())
        ticks += int(spent.sum())
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    env.close()
    return dict(episodes=episodes, collision_episodes=collisions, env_ticks=ticks, seconds=dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_search_example.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--max-nodes", type=int, default=1 << 18)
    ap.add_argument("--children", type=int, default=16)
    ap.add_argument("--widen", type=int, nargs=2, default=(4, 1))
    ap.add_argument("--c-explore", type=float, default=50.0)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--roots", type=int, default=1, metavar="R", help="search a forest of R trees (envs 0..R-1 are the roots)")
    for flag, _, unit in WEATHER_RANGE_FLAGS:
        ap.add_argument("--" + flag, type=float, nargs=2, default=None, metavar=("LO", "HI"), help=f"per-env draw, {unit}")
    ap.add_argument("--weather_seed", type=int, default=0, metavar="S", help="env i draws its weather from PCG64(S + i)")
    args = ap.parse_args()
    ranges = {kw: tuple(getattr(args, flag)) for flag, kw, _ in WEATHER_RANGE_FLAGS if getattr(args, flag) is not None}
    if not 1 <= args.roots <= args.envs:
        ap.error("--roots must be in 1..--envs")
    if ranges and args.roots < 2:
        ap.error("a weather range needs --roots >= 2: one tree stands for one weather")
    if not torch.cuda.is_available():
        raise SystemExit("tree_search.py needs a HIP device")
    dev = torch.device("cuda", 0)
    weather = sample_weather(args.envs, seed=args.weather_seed, **ranges) if ranges else None
    tree = tree_leg(dev, args.envs, args.rounds, args.max_nodes, args.children, tuple(args.widen), args.c_explore, args.seed,
                    roots=args.roots, weather=weather)
    rand = random_leg(dev, args.envs, tree["env_ticks"], args.seed + 1, weather=weather)
    res = dict(envs=args.envs, collav="sbmpc", obstacle_ships=1, max_children=args.children, widen=list(args.widen),
               c_explore=args.c_explore, device=torch.cuda.get_device_name(dev), roots=args.roots,
               **({} if weather is None else dict(weather=dict(seed=args.weather_seed, ranges={k: list(v) for k, v in ranges.items()}))),
               note="collision counts of one seeded run each: an illustration, not an estimate of a probability",
               tree_search=tree, uniform_random=rand)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(tree_search=tree, uniform_random=rand)))


if __name__ == "__main__":
    main()
