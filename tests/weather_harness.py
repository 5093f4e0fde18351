"""Helpers of the per-env weather tests: the host-driven step loop of gpu_harness.run_gpu on a handle with
per-env weather, the decision streams on such handles, and configs carrying one env's weather."""
import copy

import numpy as np

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.rl_env.ship_in_transit.weather import (KEYS, apply_to_config, config_weather, env_weather,
                                                         sample_weather)

RANGES = dict(wind_speed=(0, 12), wind_direction_deg=(-180, 180), current_speed=(0, 1.5),
              current_direction_deg=(-180, 180))
SEED = 2026


def four_weathers(cfg):
    """W0..W3: the config's own weather and three draws."""
    w = sample_weather(3, seed=SEED, **RANGES)
    return [config_weather(cfg)] + [env_weather(w, i) for i in range(3)]


def interleaved(ws, n):
    """Env i gets weather i % len(ws): neighbours in a wave never share one."""
    return {k: np.array([ws[i % len(ws)][k] for i in range(n)]) for k in KEYS}


def cfg_with(cfg, values):
    return apply_to_config(copy.deepcopy(cfg), values)


def run_gpu_weather(cfg, tables, weather, device="cuda", max_ticks=0, before=None):
    """gpu_harness.run_gpu on a handle with per-env weather (a dict of arrays, or None: never set).
    `before(sim)` runs on the fresh handle first."""
    import torch
    from ast_sac_amd.shipsim import ShipSim
    n = len(tables)
    sim = ShipSim(cfg, n, device=device)
    if before is not None:
        before(sim)
    if weather is not None:
        sim.set_weather(*[weather[k] for k in KEYS])
    lpe = sim.lanes_per_env
    o0 = sim.reset().cpu().numpy()
    ep = np.zeros(n, int)
    dec = np.zeros(n, int)
    acc_ticks = np.zeros(n, int)
    rec = [[(o0[i].copy(), [])] for i in range(n)]
    n_eps = np.array([len(t) for t in tables])
    while True:
        active = ep < n_eps
        if not active.any():
            break
        acts = np.zeros(n, np.float32)
        for i in np.nonzero(active)[0]:
            acts[i] = abi.normalized_to_scoping(tables[i][ep[i]][dec[i]])
        out = sim.step(torch.from_numpy(acts), active=torch.from_numpy(active.astype(np.uint8)), max_ticks=max_ticks)
        o = out["obs"].cpu().numpy()
        r = out["reward"].cpu().numpy()
        d = out["done"].cpu().numpy().astype(bool)
        b = out["events"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        t = out["ticks"].cpu().numpy()
        rd = out["ready"].cpu().numpy().astype(bool)
        need_reset = np.zeros(n, bool)
        for i in np.nonzero(active)[0]:
            acc_ticks[i] += t[i]
            if not rd[i]:
                continue
            rec[i][-1][1].append((o[i].copy(), float(r[i]), bool(d[i]), int(b[i]), int(acc_ticks[i])))
            acc_ticks[i] = 0
            dec[i] += 1
            if d[i] or dec[i] >= len(tables[i][ep[i]]):
                ep[i] += 1
                dec[i] = 0
                if ep[i] < n_eps[i]:
                    need_reset[i] = True
        if need_reset.any():
            o0 = sim.reset(mask=torch.from_numpy(need_reset.astype(np.uint8))).cpu().numpy()
            for i in np.nonzero(need_reset)[0]:
                rec[i].append((o0[i].copy(), []))
    fields = {f: sim.get(f).cpu().numpy() for f in range(abi.N_SHIP_FIELDS)}
    env_fields = {f: sim.get(f).cpu().numpy() for f in (abi.E_SAMPLING_COUNT, abi.E_TRAVEL_DIST, abi.E_TRAVEL_TIME,
                                                         abi.E_ACC_REWARD, abi.E_N_BASE, abi.E_E_BASE,
                                                         abi.E_SBMPC_P_LAST, abi.E_SBMPC_CHI_LAST)}
    sim.close()
    return rec, fields, env_fields, lpe


def records(gpu):
    """Decision records with the observations as bytes: equality is bit equality."""
    return [[(o0.tobytes(), [(o.tobytes(), r, d, b, t) for (o, r, d, b, t) in decs]) for (o0, decs) in env]
            for env in gpu]


def run_stream(cfg, n, weather, launch, n_calls=3, cap=96, tail=0):
    """n_calls stream launches (launch(sim, ep, dec, log, log_len)) on a fresh, reset handle: per-env arrays of
    the decision records, in order."""
    import torch
    from ast_sac_amd.shipsim import ShipSim
    sim = ShipSim(cfg, n)
    if weather is not None:
        sim.set_weather(*[weather[k] for k in KEYS])
    if tail:
        sim.set_stream_tail(tail)
    sim.reset()
    ep = torch.zeros(n, dtype=torch.int32, device="cuda")
    dec = torch.zeros(n, dtype=torch.int32, device="cuda")
    log = torch.zeros((n, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(n_calls):
        launch(sim, ep, dec, log, log_len)
    sim.synchronize()
    L, ln = log.cpu().numpy(), log_len.cpu().numpy()
    sim.close()
    assert ln.max() <= cap
    return [L[i, :ln[i]] for i in range(n)]
