"""A fixed-effort weighted splitting estimate of P(collision within an episode) on the K = 1 sbmpc table stream, next to
plain Monte Carlo with the same env-tick budget. What splitting_search.py leaves out — the weights — is here.

One repetition: n envs are reset together with weights 1 / n and run shipsim_run_table in launches of --ticks ticks.
After each launch
  * an env whose decision records hold the end of its episode 0 banks weight x [collision];
  * envs past episode 0 (ep_idx > 0) are retired: weight 0, never selected again, their slots refilled;
  * the live envs are resampled in proportion to weight x exp(-d / lambda), d = level_distance (the own ship's
    distance to the obstacle ship), in place, and forked (BatchedMultiShipRLEnv.split): nothing leaves the device;
  * every slot that changed hands (src[j] != j) gets fresh table columns drawn on the device from the same uniform
    law. A survivor keeps its columns: its unread future actions are independent of the state the potential saw.
It stops when no env is live. The banked sum is the estimate: the reweighting of shipsim_resample keeps it unbiased
for any lambda. The plain leg runs the same number of launches without splitting and counts the envs whose own
episode 0 ended in a collision over those whose episode 0 ended (the episodes after it are cut short by the budget,
which favours the short ones, so they are counted but not used). Both are repeated --reps times with other seeds; means and sample standard deviations are written to
profiles/splitting_estimate.json. Reported, not asserted: nobody has measured this scenario's collision probability.

With one of the runner's four weather range flags every env sails under its own wind and current (weather.
sample_weather, drawn once with --weather_seed and set again before every leg), and --weather says what a clone does
about it: "carry" (the default then) takes its source's weather along on the device, which is the process the weights
are unbiased for — weather has shaped the clone's whole past; "keep" leaves a clone under the weather of the slot it
lands in, a process that changes weather mid-episode. The output then goes to profiles/splitting_estimate_weather.json.

    python scripts/splitting_estimate.py [--out FILE] [--envs N] [--reps R] [--ticks T] [--lambda METRES]
        [--wind_speed_range LO HI] [--wind_direction_range LO HI] [--current_speed_range LO HI]
        [--current_direction_range LO HI] [--weather_seed S] [--weather {keep,carry}]
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
from ast_sac_amd import shipsim, shipsim_abi as abi  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.weather import sample_weather  # noqa: E402

# the runner's four range flags -> sample_weather's keyword arguments
WEATHER_RANGE_FLAGS = (("wind_speed_range", "wind_speed", "m/s"), ("wind_direction_range", "wind_direction_deg", "degrees"),
                       ("current_speed_range", "current_speed", "m/s"),
                       ("current_direction_range", "current_direction_deg", "degrees"))

CAP = 32   # decision records per env and launch
N_EPS = 2  # table rows (a retired env reads row ep % 2 until its slot is refilled)
LOW, HIGH = np.float32(-np.deg2rad(30)), np.float32(np.deg2rad(30))


def _columns(gen, n_dec, n, dev):
    """Scoping angles of uniform normalised actions (abi.normalized_to_scoping's mapping), drawn on the device."""
    a = torch.rand((N_EPS, n_dec, n), generator=gen, device=dev, dtype=torch.float32) * 2 - 1
    return (float(LOW) + (a + 1) * 0.5 * float(HIGH - LOW)).clamp(float(LOW), float(HIGH))


def _ended(log, ln, n_dec, row):
    """(records that end an episode, those that do so in a collision, records dropped): masks over (n, CAP)."""
    have = row < ln.clamp(max=CAP)[:, None]
    done = (log[:, :, abi.DL_DONE] != 0) & have
    last = (log[:, :, abi.DL_DECISION].long() == n_dec - 1) & have  # the episode's last decision ends it too
    coll = done & ((log[:, :, abi.DL_EVENTS].long() & abi.EV_COLLISION) != 0)
    return done | last, coll, (ln - ln.clamp(max=CAP)).sum()


def run(env, ticks, lam, seed, split, launches=None, max_launches=512, weather=None, weather_mode="keep"):
    dev, n, sim = env.device, env.n_envs, env.sim
    if weather is not None:  # every leg starts from the weather as drawn: a leg under "carry" has moved it
        env.set_weather(weather)
    n_dec = int(env.cfg.max_sampling_frequency)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    table = _columns(gen, n_dec, n, dev)
    ep = torch.zeros(n, dtype=torch.int32, device=dev)
    dec = torch.zeros(n, dtype=torch.int32, device=dev)
    log = torch.zeros((n, CAP, abi.DECLOG_COLS), dtype=torch.float64, device=dev)
    ln = torch.zeros(n, dtype=torch.int32, device=dev)
    row = torch.arange(CAP, device=dev)[None, :]
    own = torch.arange(n, dtype=torch.int32, device=dev)
    weight = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    bank = torch.zeros((), dtype=torch.float64, device=dev)
    episodes = torch.zeros((), dtype=torch.int64, device=dev)
    collisions = torch.zeros((), dtype=torch.int64, device=dev)
    first_ended = torch.zeros((), dtype=torch.int64, device=dev)
    first_collisions = torch.zeros((), dtype=torch.int64, device=dev)
    dropped = torch.zeros((), dtype=torch.int64, device=dev)
    refilled = torch.zeros((), dtype=torch.int64, device=dev)
    env.reset()
    done_launches = 0
    while done_launches < (launches if launches is not None else max_launches):
        ln.zero_()
        sim.run_table(table, ticks, ep, dec, log=log, log_len=ln)
        done_launches += 1
        ended, coll, drop = _ended(log, ln, n_dec, row)
        dropped += drop
        episodes += ended.sum()
        collisions += coll.sum()
        first = log[:, :, abi.DL_EPISODE].long() == 0
        if not split:  # each env's own episode 0 is one draw: later episodes are cut short by the budget
            first_ended += (ended & first).any(dim=1).sum()
            first_collisions += (coll & first).any(dim=1).sum()
            continue
        bank += (weight * (coll & first).any(dim=1)).sum()
        weight = torch.where(ep > 0, torch.zeros_like(weight), weight)
        if not bool((weight > 0).any()):  # the loop's only look at the device: is anybody live
            break
        potential = torch.exp(-sim.level_distance() / lam)
        src, weight, _, _ = env.split(weight, potential, seed, counter, ep, dec, weather=weather_mode)
        counter += 1
        moved = src != own
        refilled += moved.sum()
        table = torch.where(moved[None, None, :], _columns(gen, n_dec, n, dev), table)
    sim.synchronize()
    return dict(launches=done_launches, env_ticks=done_launches * ticks * n, episodes_ended=int(episodes),
                collision_episodes=int(collisions), records_dropped=int(dropped), slots_refilled=int(refilled),
                estimate=float(bank) if split else (float(first_collisions) / max(int(first_ended), 1)),
                first_episodes_ended=None if split else int(first_ended),
                first_episode_collisions=None if split else int(first_collisions),
                live_at_end=int((weight > 0).sum()) if split else None)


def _mean_std(xs):
    xs = np.asarray(xs, np.float64)
    return dict(mean=float(xs.mean()), std=float(xs.std(ddof=1)) if len(xs) > 1 else None, runs=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/splitting_estimate.json, or with a weather range "
                    "flag profiles/splitting_estimate_weather.json")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--lambda", dest="lam", type=float, default=1500.0, help="length scale of the potential [m]")
    ap.add_argument("--collav", default="sbmpc", choices=("sbmpc", "simple", "none"),
                    help="the own ship's collision avoidance (sbmpc: the scenario of record)")
    ap.add_argument("--seed", type=int, default=20251015, help="repetition r uses seed + 2 r and seed + 2 r + 1")
    for flag, _, unit in WEATHER_RANGE_FLAGS:
        ap.add_argument("--" + flag, type=float, nargs=2, default=None, metavar=("LO", "HI"),
                        help=f"every env draws its own value, uniform in [LO, HI] {unit}")
    ap.add_argument("--weather_seed", type=int, default=0, metavar="S", help="env i draws its weather from PCG64(S + i)")
    ap.add_argument("--weather", default=None, choices=("keep", "carry"),
                    help="what a clone does about per-env weather (default with a range flag: carry)")
    args = ap.parse_args()
    ranges = {kw: tuple(getattr(args, flag)) for flag, kw, _ in WEATHER_RANGE_FLAGS if getattr(args, flag) is not None}
    if args.weather is not None and not ranges:
        ap.error("--weather needs one of the weather range flags")
    if not torch.cuda.is_available():
        raise SystemExit("splitting_estimate.py needs a HIP device")
    dev = torch.device("cuda", 0)
    env = BatchedMultiShipRLEnv(default_args(collav_mode=args.collav), args.envs, device=dev)
    weather, mode = None, "keep"
    if ranges:
        weather = sample_weather(args.envs, seed=args.weather_seed, cfg=env.cfg, **ranges)
        mode = args.weather or "carry"
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "splitting_estimate_weather.json")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "splitting_estimate.json")
    legs = dict(splitting=[], plain=[])
    t0 = time.perf_counter()
    for rep in range(args.reps):
        s = run(env, args.ticks, args.lam, args.seed + 2 * rep, True, weather=weather, weather_mode=mode)
        p = run(env, args.ticks, args.lam, args.seed + 2 * rep + 1, False, launches=s["launches"],  # the same budget
                weather=weather)
        legs["splitting"].append(s)
        legs["plain"].append(p)
        print(f"[estimate] rep {rep}: splitting {s['estimate']:.3e} ({s['launches']} launches, "
              f"{s['slots_refilled']} slots refilled), plain {p['estimate']:.3e} "
              f"({p['first_episode_collisions']} / {p['first_episodes_ended']} first episodes)", flush=True)
    dt = time.perf_counter() - t0
    env.close()
    res = dict(envs=args.envs, collav=args.collav, obstacle_ships=1, ticks_per_launch=args.ticks, lambda_m=args.lam,
               reps=args.reps, seed=args.seed, device=torch.cuda.get_device_name(dev),
               build=shipsim.load_library().shipsim_build_info().decode(), seconds=dt,
               note="reported, not asserted: the scenario's collision probability has not been measured otherwise",
               **({} if weather is None else dict(weather=dict(mode=mode, seed=args.weather_seed,
                                                               ranges={k: list(v) for k, v in ranges.items()}))),
               splitting=dict(_mean_std([x["estimate"] for x in legs["splitting"]]), legs=legs["splitting"]),
               plain=dict(_mean_std([x["estimate"] for x in legs["plain"]]), legs=legs["plain"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: dict(mean=res[k]["mean"], std=res[k]["std"]) for k in ("splitting", "plain")}))


if __name__ == "__main__":
    main()
