"""Per-env weather for the batched env: one draw of wind and current per env (beyond the reference, whose
env has one sea; ShipSim.set_weather / shipsim_set_weather run it).

Env i draws from its own generator, np.random.Generator(np.random.PCG64(seed + first_env + i)), four uniforms in
the order wind speed, wind direction, current speed, current direction: an env's weather depends on its global
index alone, not on the batch size or on how the envs are spread over ranks (rank r of a run with n envs per
rank passes first_env = r * n).
"""
import numpy as np

from ... import shipsim_abi as abi

KEYS = ("wind_speed", "wind_direction", "current_north", "current_east")
RANGES = ("wind_speed", "wind_direction_deg", "current_speed", "current_direction_deg")


def config_weather(cfg=None):
    """The config's own (uniform) weather as the four values shipsim_set_weather takes per env."""
    cfg = cfg if cfg is not None else abi.ast_config("sbmpc")
    return dict(wind_speed=float(cfg.wind_speed), wind_direction=float(cfg.wind_direction),
                current_north=float(cfg.current_velocity_component_from_north),
                current_east=float(cfg.current_velocity_component_from_east))


def _check_range(name, r, nonneg):
    if r is None:
        return None
    lo, hi = (float(x) for x in r)
    if not (np.isfinite(lo) and np.isfinite(hi)) or hi < lo or (nonneg and lo < 0):
        raise ValueError(f"{name}: a finite range (lo, hi) with lo <= hi{' and lo >= 0' if nonneg else ''}, not {r!r}")
    return lo, hi


def sample_weather(n_envs, wind_speed=None, wind_direction_deg=None, current_speed=None, current_direction_deg=None,
                   seed=0, first_env=0, cfg=None):
    """Weather of envs first_env .. first_env + n_envs - 1: dict of four float64 arrays (KEYS: wind speed [m/s],
    wind direction [rad], current from north and from east [m/s]) as ShipSim.set_weather takes them.

    Each range is (lo, hi), uniform; directions in degrees. The current's components are speed * cos(direction)
    from north and speed * sin(direction) from east. A range left None keeps the value of `cfg` (default: the
    scenario of record) for that quantity: its wind speed, its wind direction, the speed or the direction of its
    current; with both current ranges None its two components exactly."""
    base = config_weather(cfg)
    rs = [_check_range(n, r, nonneg) for n, r, nonneg in
          zip(RANGES, (wind_speed, wind_direction_deg, current_speed, current_direction_deg),
              (True, False, True, False))]
    n_envs = int(n_envs)
    u = np.empty((n_envs, 4), dtype=np.float64)
    for i in range(n_envs):
        rng = np.random.Generator(np.random.PCG64(int(seed) + int(first_env) + i))
        u[i] = [rng.random(), rng.random(), rng.random(), rng.random()]

    def draw(k):
        lo, hi = rs[k]
        return lo + (hi - lo) * u[:, k]

    ws = draw(0) if rs[0] else np.full(n_envs, base["wind_speed"])
    wd = np.deg2rad(draw(1)) if rs[1] else np.full(n_envs, base["wind_direction"])
    if rs[2] is None and rs[3] is None:
        vn, ve = np.full(n_envs, base["current_north"]), np.full(n_envs, base["current_east"])
    else:
        cs = draw(2) if rs[2] else np.full(n_envs, np.hypot(base["current_north"], base["current_east"]))
        cd = np.deg2rad(draw(3)) if rs[3] else np.full(n_envs, np.arctan2(base["current_east"], base["current_north"]))
        vn, ve = cs * np.cos(cd), cs * np.sin(cd)
    return dict(zip(KEYS, (ws, wd, vn, ve)))


def env_weather(weather, i):
    """Env i's four values of a weather dict."""
    return {k: float(np.asarray(weather[k]).reshape(-1)[i]) for k in KEYS}


def apply_to_config(cfg, values):
    """Write one env's four values (env_weather) into a config: the uniform handle that reproduces that env,
    e.g. to replay a found failure with trajectory recording."""
    cfg.wind_speed = values["wind_speed"]
    cfg.wind_direction = values["wind_direction"]
    cfg.current_velocity_component_from_north = values["current_north"]
    cfg.current_velocity_component_from_east = values["current_east"]
    return cfg
