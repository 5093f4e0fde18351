"""The gather that moves per-env weather (shipsim_weather_store / _load / _fork) restated in numpy, with the index
sets and tables the CPU and GPU tests share. A weather table is ROWS rows of n slots: wind speed, sin and cos of the
wind direction, current from north, current from east, and the wind direction as set."""
import math

import numpy as np

ROWS = 6
KEYS = ("wind_speed", "wind_direction", "current_north", "current_east")
KEY_ROWS = (0, 5, 3, 4)  # the row each key of ShipSim.weather() is read from
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def gather(src, idx, dst):
    """Slot d of dst takes slot idx[d] of src, all rows; an index outside [0, n_src) leaves slot d as it is."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    assert src.shape[0] == dst.shape[0] == ROWS and idx.size == dst.shape[1]
    ok = (idx >= 0) & (idx < src.shape[1])
    out = dst.copy()
    out[:, ok] = src[:, idx[ok]]
    return out


def fork(table, idx):
    """The in-place fork: every slot takes from the table as it was before the call."""
    return gather(table, idx, table)


def table(weather):
    """The six rows of a dict of the four per-env arrays (sin and cos by math: the host libm's, as the library's)."""
    w = {k: np.asarray(weather[k], dtype=np.float64).reshape(-1) for k in KEYS}
    wd = w["wind_direction"]
    return np.stack([w["wind_speed"], np.array([math.sin(x) for x in wd]), np.array([math.cos(x) for x in wd]),
                     w["current_north"], w["current_east"], wd])


def keys_of(tab):
    return {k: tab[r].copy() for k, r in zip(KEYS, KEY_ROWS)}


def random_weather(n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return dict(wind_speed=g.uniform(0, 12, n), wind_direction=g.uniform(-np.pi, np.pi, n),
                current_north=g.uniform(-1.5, 1.5, n), current_east=g.uniform(-1.5, 1.5, n))


def index_sets(n_dst, n_src, seed=7):
    """name -> int32 index array of n_dst entries into n_src slots: permutations (where the sizes allow), broadcasts, a
    cycle, duplicates, and entries outside [0, n_src): -1, n_src, INT32_MIN, INT32_MAX."""
    g = np.random.Generator(np.random.PCG64(seed + 1000 * n_dst + n_src))
    d = np.arange(n_dst, dtype=np.int64)
    sets = {"cycle": (d + 1) % n_src, "broadcast_first": np.zeros(n_dst, np.int64),
            "broadcast_last": np.full(n_dst, n_src - 1), "duplicates": g.integers(0, n_src, n_dst)}
    if n_dst <= n_src:
        sets["permutation"] = g.permutation(n_src)[:n_dst]
        sets["reversed"] = (n_src - 1 - d)
    out = g.integers(0, n_src, n_dst)
    bad = np.array([-1, n_src, INT32_MIN, INT32_MAX], dtype=np.int64)
    out[g.random(n_dst) < 0.4] = -1
    for j in range(min(n_dst, 8)):  # every kind of outsider, the first and the last slot among them
        out[(j * 37) % n_dst] = bad[j % 4]
    out[0], out[n_dst - 1] = (n_src, INT32_MAX) if n_dst > 1 else (INT32_MIN, INT32_MIN)
    sets["out_of_range"] = out
    sets["none_served"] = bad[d % 4]
    return {k: v.astype(np.int32) for k, v in sets.items()}
