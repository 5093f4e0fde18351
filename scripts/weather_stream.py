"""Per-env weather against the config's uniform weather, decision streams side by side: shipsim_run_table and
shipsim_run_policy (a 2 x 256 TanhGaussianPolicy sampled in-kernel at every decision, stochastic) on a uniform handle
and on a handle whose envs each drew their own wind and current (rl_env/ship_in_transit/weather.py).
4096 envs, sbmpc, K = 1, 16 lanes per env, launch tail off, 1024-tick launches, one process on one GPU. Every leg is
timed three times, uniform and weather handles alternating (handle, then stream, inside each repetition), each window
long enough (>= 0.5 s of launches after warm-up launches of the same shape) and closed by a device synchronise.
A third handle separates the kernels' cost from the episodes': per-env weather with every env at the config's
values runs the weather kernels on exactly the uniform handle's episodes ("same_sea"), while the drawn weather
also changes what the envs do (SBMPC activity, episode endings). Writes the rates and the weather : uniform and
same_sea : uniform ratios per stream, with the spread over the repetitions, to profiles/weather_stream.json
(DESIGN.md §9). No threshold: the ratios are reported.

    python scripts/weather_stream.py [--out FILE] [--envs N] [--reps R]
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
from ast_sac_amd import shipsim_abi as abi  # noqa: E402
from ast_sac_amd.rl_env.ship_in_transit.weather import KEYS, config_weather, sample_weather  # noqa: E402
from ast_sac_amd.shipsim import ShipSim  # noqa: E402

TICKS = 1024
WINDOW_S = 0.5
WARMUP = 3
RANGES = dict(wind_speed=(0, 12), wind_direction_deg=(-180, 180), current_speed=(0, 1.5),
              current_direction_deg=(-180, 180))
SEED = 2026


class _Env:
    class action_space:
        shape = (1,)


def _policy(dev, hidden=256):
    from ast_sac_amd.ast_sac.torch.networks.mlp import ConcatMlp
    from ast_sac_amd.ast_sac.torch.sac.policies.gaussian_policy import TanhGaussianPolicy
    from ast_sac_amd.ast_sac.torch.sac.sac_fused import FusedSACTrainer
    torch.manual_seed(0)
    q = [ConcatMlp(input_size=9, output_size=1, hidden_sizes=[hidden, hidden]).to(dev) for _ in range(4)]
    pol = TanhGaussianPolicy(obs_dim=8, action_dim=1, hidden_sizes=[hidden, hidden]).to(dev)
    tr = FusedSACTrainer(env=_Env, policy=pol, qf1=q[0], qf2=q[1], target_qf1=q[2], target_qf2=q[3],
                         discount=0.965, soft_target_tau=1e-3, policy_lr=8e-5, qf_lr=8e-5, reward_scale=0.75,
                         batch_size=256, backend="hip")
    return tr, tr.device_policy(deterministic=False, seed=20251017)


def _leg(dev, n_envs, weather, stream, dp, table):
    """env-ticks/s of one stream on a fresh handle: WARMUP launches, then >= WINDOW_S of launches."""
    cfg = abi.ast_config("sbmpc", machinery=abi.MACH_DETAILED)
    cfg.lanes_per_env = 16
    sim = ShipSim(cfg, n_envs, device=dev)
    if weather is not None:
        sim.set_weather(*[weather[k] for k in KEYS])
    sim.reset()
    sim.set_stream_tail(0)
    n_dec = int(cfg.max_sampling_frequency)
    ep = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    dec = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    out = dict(ticks=torch.zeros(n_envs, dtype=torch.int32, device=dev),
               decisions=torch.zeros(n_envs, dtype=torch.int32, device=dev))
    ticks = torch.zeros((), dtype=torch.int64, device=dev)
    decs = torch.zeros((), dtype=torch.int64, device=dev)

    def launch():
        if stream == "table":
            sim.run_table(table, TICKS, ep, dec, out=out)
        else:
            sim.run_policy(dp.weights(), TICKS, n_dec, ep, dec, deterministic=False, seed=dp.seed,
                           counter=dp.counter, out=out)
            dp.counter.add_(1)
        ticks.add_(out["ticks"].sum())
        decs.add_(out["decisions"].sum())

    try:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(WARMUP):
            launch()
        torch.cuda.synchronize(dev)
        per = (time.perf_counter() - t0) / WARMUP
        n = max(8, int(math.ceil(WINDOW_S / max(per, 1e-6))))
        ticks.zero_()
        decs.zero_()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            launch()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        return dict(env_ticks_per_s=float(ticks.item()) / dt, decisions_per_s=float(decs.item()) / dt,
                    launches=n, ms_per_launch=dt / n * 1e3, lanes_per_env=sim.lanes_per_env)
    finally:
        sim.close()


def _stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return dict(median=med, min=xs[0], max=xs[-1], spread=(xs[-1] - xs[0]) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weather_stream.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weather_stream.py needs a HIP device: there is no rate to report without one")
    dev = torch.device("cuda", 0)
    tr, dp = _policy(dev)
    n_dec = int(abi.ast_config("sbmpc").max_sampling_frequency)
    gen = np.random.Generator(np.random.PCG64(20251015))
    table = torch.from_numpy(abi.normalized_to_scoping(
        gen.uniform(-1, 1, (8, n_dec, args.envs)).astype(np.float32))).to(dev)
    weather = sample_weather(args.envs, seed=SEED, **RANGES)
    same_sea = {k: np.full(args.envs, v) for k, v in config_weather(abi.ast_config("sbmpc")).items()}
    handles = (("uniform", None), ("same_sea", same_sea), ("weather", weather))
    runs = {(h, s): [] for h, _ in handles for s in ("table", "policy")}
    for rep in range(args.reps):
        for s in ("table", "policy"):
            for h, w in handles:
                r = _leg(dev, args.envs, w, s, dp, table)
                runs[(h, s)].append(r)
                print(f"[weather] rep {rep} {s:6s} {h:8s}: {r['env_ticks_per_s'] / 1e6:8.2f} M env-ticks/s, "
                      f"{r['ms_per_launch']:.2f} ms per launch x {r['launches']}", flush=True)
    res = dict(envs=args.envs, collav="sbmpc", obstacle_ships=1, lanes_per_env=16, slice_ticks=TICKS, tail_ticks=0,
               policy="2x256 stochastic", weather=dict(seed=SEED, **{k: list(v) for k, v in RANGES.items()}),
               reps=args.reps, window_s=WINDOW_S, warmup_launches=WARMUP, unit="env-ticks/s",
               device=torch.cuda.get_device_name(dev), streams={})
    for s in ("table", "policy"):
        leg = {}
        for h, _ in handles:
            rs = runs[(h, s)]
            leg[h] = dict(runs=[r["env_ticks_per_s"] for r in rs], ms_per_launch=[r["ms_per_launch"] for r in rs],
                          decisions_per_s=[r["decisions_per_s"] for r in rs],
                          **_stats([r["env_ticks_per_s"] for r in rs]))
        for h in ("weather", "same_sea"):  # the ratio inside each repetition (its legs ran back to back)
            ratios = [w["env_ticks_per_s"] / u["env_ticks_per_s"] for w, u in zip(runs[(h, s)], runs[("uniform", s)])]
            leg[h + "_over_uniform"] = dict(runs=ratios, **_stats(ratios))
        res["streams"][s] = leg
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({s: {h: v[h + "_over_uniform"]["median"] for h in ("weather", "same_sea")}
                      for s, v in res["streams"].items()}))


if __name__ == "__main__":
    main()
