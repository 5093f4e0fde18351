"""CPU model of how the headline stream's envs share SBMPC passes, by how they are grouped into waves of four
(no GPU): bench.py's kind of stream replayed on the CPU oracle (tests/oracle_ffi.py) — a PCG64 U(-1, 1) table of 8 rows
x 9 decisions per env, episodes chained for `ticks` ticks per env — with an env "requesting" at a tick when its two
ships are within 2000 m (SBMPC's D_INIT) in the per-tick log. A wave's optimiser serves two requests per pass, so a
wave-tick with r requesting envs costs ceil(r / 2) passes, the odd one lone. Compared: adjacent env indices (slot = env),
regrouping every 4096 ticks by ticks since the env's last reset (what shipsim_set_stream_grouping does, launch
boundaries idealised to every 4096 ticks), regrouping by time to the next request (not causal: a bound for any key),
the first 4096 ticks from the synchronised reset, and the floor of two requests in every pass.
  python scripts/sbmpc_grouping_model.py [n_envs=1024] [ticks=20480] > profiles/stream_grouping_model.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import oracle_ffi as O  # noqa: E402
from ast_sac_amd import shipsim_abi as abi  # noqa: E402

LAUNCH, WAVE, D_INIT = 4096, 4, 2000.0


def replay(n_envs, ticks, seed=20251015):
    """requesting[env, tick] and since_reset[env, tick] of the chained episodes, and the episode lengths."""
    cfg = abi.ast_config("sbmpc")
    n_dec = int(cfg.max_sampling_frequency)
    a = np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (8, n_dec, n_envs)).astype(np.float32)
    table = abi.normalized_to_scoping(a)
    req = np.zeros((n_envs, ticks), bool)
    since = np.zeros((n_envs, ticks), np.int32)
    lengths = []
    for i in range(n_envs):
        env = O.OracleEnv(cfg, log_cap=4096)
        t, ep = 0, 0
        while t < ticks:
            env.reset()
            n = 0
            for d in range(n_dec):
                _, _, done, _, k = env.step(table[ep % 8, d, i])
                n += k
                if done:
                    break
            la, lb = env.log(0), env.log(1)
            m = min(len(la), len(lb))
            dist = np.hypot(la[:m, 1] - lb[:m, 1], la[:m, 2] - lb[:m, 2])
            # one log row per tick (a leading row of the reset state, where the log holds one, is the state the
            # first tick's request sees)
            r = dist[:n] if m > n else np.concatenate([dist, np.repeat(dist[-1:], n - m)])
            take = min(n, ticks - t)
            req[i, t:t + take] = r[:take] < D_INIT
            since[i, t:t + take] = np.arange(take)
            lengths.append(n)
            t += take
            ep += 1
    return req, since, np.array(lengths)


def wave_stats(req_waves):
    """req_waves: [waves, WAVE, ticks] bool."""
    r = req_waves.sum(1)
    passes = (r + 1) // 2
    lone = r % 2
    active = r > 0
    wt = r.size
    return {"passes_per_wave_tick": float(passes.sum() / wt), "wave_ticks_with_pass": float(active.mean()),
            "requests_per_active_wave_tick": float(r.sum() / max(active.sum(), 1)),
            "lone_pass_share": float(lone.sum() / max(passes.sum(), 1)),
            "requests_per_pass": float(r.sum() / max(passes.sum(), 1))}


def regrouped(req, key_at, t0, t1):
    """Waves re-formed at every launch boundary in [t0, t1) by a stable sort of key_at(boundary tick)."""
    n = req.shape[0] // WAVE * WAVE
    parts = []
    for b in range(t0, t1, LAUNCH):
        order = np.argsort(key_at(b)[:n], kind="stable")
        parts.append(req[order, b:min(b + LAUNCH, t1)].reshape(n // WAVE, WAVE, -1))
    return np.concatenate(parts, 2)


def main():
    n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 20480
    req, since, lengths = replay(n_envs, ticks)
    n = n_envs // WAVE * WAVE

    def to_next(b):  # ticks until the env's next request at or after tick b (never: past the end)
        nxt = np.full(n_envs, ticks, np.int64)
        for i in range(n_envs):
            w = np.nonzero(req[i, b:])[0]
            if len(w):
                nxt[i] = w[0]
        return nxt

    steady = (LAUNCH, ticks)
    rows = {
        "adjacent": wave_stats(req[:n, steady[0]:].reshape(n // WAVE, WAVE, -1)),
        "by_ticks_since_reset": wave_stats(regrouped(req, lambda b: since[:, b], *steady)),
        "by_time_to_next_request": wave_stats(regrouped(req, to_next, *steady)),
        "first_launch_adjacent": wave_stats(req[:n, :LAUNCH].reshape(n // WAVE, WAVE, -1)),
    }
    rate = float(req[:, LAUNCH:].mean())
    out = {"what": "CPU model (oracle replay), not a GPU measurement", "n_envs": n_envs, "ticks_per_env": ticks,
           "launch_ticks": LAUNCH, "envs_per_wave": WAVE, "steady_state_ticks": list(steady),
           "episode_ticks": {"mean": float(lengths.mean()), "median": float(np.median(lengths)),
                             "p5": float(np.percentile(lengths, 5)), "max": int(lengths.max())},
           "requesting_fraction": rate, "floor_passes_per_wave_tick": WAVE * rate / 2, "groupings": rows,
           "passes_saved_by_ticks_since_reset": 1.0 - rows["by_ticks_since_reset"]["passes_per_wave_tick"] /
           rows["adjacent"]["passes_per_wave_tick"]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
