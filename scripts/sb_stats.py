"""SBMPC activity of the decision streams, from a diagnostics build with -DSHIPSIM_SB_STATS run through SHIPSIM_LIB
on the GPU box:  SHIPSIM_LIB=ast_sac_amd/lib/abl/NAME.so python scripts/sb_stats.py K [launches] [on|off|both]
  K > 1  the C5 stream (bench.py's bench_c5 workload; scripts/build_variant.sh NAME -DSHIPSIM_REGCHECK=3 -DSHIPSIM_SB_STATS)
  K = 1  the headline stream (bench.py's: 4096 envs, its PCG64 table, 4096-tick launches with the 1024-tick tail;
         scripts/build_variant.sh NAME -DSHIPSIM_SB_STATS), counted over `launches` launches after one warm-up launch
         from the synchronised reset, i.e. in the bench's timed regime
The third argument is the stream grouping (shipsim_set_stream_grouping): on (the default), off, or both legs, one
after the other, each on a fresh handle. Prints one JSON line per leg: per env-tick request rate, passes per optimiser
call, lone-request share, requests per pass, horizons per pass (K > 1), and (K = 1) the share of the requests the
nominal-scenario test answered without a pass with the passes per wave-tick that remain."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from ast_sac_amd import shipsim_abi as abi  # noqa: E402
from ast_sac_amd.shipsim import ShipSim, load_library  # noqa: E402

NAMES = ["wave_ticks_with_pass", "passes", "lone_passes", "requests_served", "horizon_lanes", "far_lanes",
         "env_ticks_requesting", "env_ticks", "requests_answered_nominal", "wave_ticks_all_answered"]


def read_stats(L):
    out = (C.c_uint32 * 32)()
    assert L.shipsim_diag_lane_faults(out) == 0, "not an SHIPSIM_SB_STATS build"
    # counters 0..7 in words 16..31, the later ones from word 0 on (shipsim_diag_lane_faults)
    return [out[16 + 2 * i] | (out[17 + 2 * i] << 32) for i in range(8)] + \
        [out[2 * i] | (out[2 * i + 1] << 32) for i in range(len(NAMES) - 8)]


def headline(L, dev, launches, grouping, n_envs=4096, slice_ticks=4096, tail_ticks=1024):
    """bench.py's headline stream; the counters cover the launches after the warm-up one."""
    cfg = abi.ast_config("sbmpc")
    sim = ShipSim(cfg, n_envs, device=dev)
    sim.set_stream_grouping(grouping)
    n_dec = cfg.max_sampling_frequency
    gen = np.random.Generator(np.random.PCG64(20251015))
    table = torch.from_numpy(abi.normalized_to_scoping(gen.uniform(-1, 1, (8, n_dec, n_envs)).astype(np.float32))).to(dev)
    ep = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    dec = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    cap = max(8, (slice_ticks + tail_ticks) // 32 + 16)
    log = torch.zeros((n_envs, cap, abi.DECLOG_COLS), dtype=torch.float64, device=dev)
    log_len = torch.zeros(n_envs, dtype=torch.int32, device=dev)
    sim.reset()
    sim.set_stream_tail(tail_ticks)
    ticks = 0
    for i in range(1 + launches):
        if i == 1:
            read_stats(L)  # (synchronizes and zeroes the counters)
        log_len.zero_()
        o = sim.run_table(table, slice_ticks, ep, dec, log=log, log_len=log_len)
        if i >= 1:
            ticks += int(o["ticks"].sum())
    v = read_stats(L)
    sim.close()
    return v, dict(env_ticks_out=ticks, lanes_per_env=sim.lanes_per_env, warmup_launches=1)


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    legs = {"on": [True], "off": [False], "both": [False, True]}[sys.argv[3] if len(sys.argv) > 3 else "on"]
    L = load_library()
    dev = torch.device("cuda", 0)
    for grouping in legs:
        read_stats(L)  # zero the counters
        if K == 1:
            v, extra = headline(L, dev, launches, grouping)
        else:
            assert grouping, "the C5 leg runs the library's default (grouping on)"
            r = bench.bench_c5(dev, 1, 4096, K, launches=launches, warmup=0)
            torch.cuda.synchronize()
            v, extra = read_stats(L), dict(env_ticks_per_s=r["env_ticks_per_s"])
        d = dict(zip(NAMES, v))
        d.update(K=K, launches=launches, grouping=bool(grouping), **extra)
        d.update(request_rate=v[6] / max(v[7], 1), passes_per_call=v[1] / max(v[0], 1), lone_share=v[2] / max(v[1], 1),
                 requests_per_pass=v[3] / max(v[1], 1), horizon_lanes_per_pass=v[4] / max(v[1], 1),
                 far_lanes_per_pass=v[5] / max(v[1], 1), wave_ticks_with_pass_per_env_tick=v[0] / max(v[7], 1),
                 passes_per_env_tick=v[1] / max(v[7], 1))
        if K == 1:  # (four envs per wave at 16 lanes per env: a wave-tick is four env-ticks)
            d.update(nominal_share=v[8] / max(v[6], 1), passes_per_wave_tick=4.0 * v[1] / max(v[7], 1),
                     requests_left_per_wave_tick=4.0 * (v[6] - v[8]) / max(v[7], 1))
        print(json.dumps(d), flush=True)


if __name__ == "__main__":
    main()
