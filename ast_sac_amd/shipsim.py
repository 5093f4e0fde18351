"""Python binding of libshipsim.so (include/shipsim.h) over torch device tensors.

The library is the product path: there is no CPU fallback. If the shared library is missing or
cannot be loaded, importing/constructing raises — build it with `python -c "import
__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).
"""
import ctypes as C
import os

import numpy as np
import torch  # noqa: F401  (loads torch's HIP runtime first; libshipsim binds to the same libamdhip64.so.7)

from . import shipsim_abi as abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SHIPSIM_LIB") or os.path.join(_HERE, "lib", "libshipsim.so")

_lib = None


class ShipSimError(RuntimeError):
    pass


class ShipSimNonFiniteError(ShipSimError):
    """shipsim_synchronize: env decisions ended on a NaN/Inf ship state (SHIPSIM_EV_NONFINITE)."""


def load_library(path=LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ShipSimError(f"native library {path} not found: build it first (__graft_entry__.build())")
    L = C.CDLL(path)
    P = C.c_void_p
    cfgp = C.POINTER(abi.Config)
    L.shipsim_abi_version.restype = C.c_int32
    L.shipsim_build_info.restype = C.c_char_p
    L.shipsim_default_config.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, cfgp]
    L.shipsim_create.argtypes = [cfgp, C.c_int32, C.c_int32, C.c_int32, P, C.POINTER(P)]
    L.shipsim_destroy.argtypes = [P]
    L.shipsim_last_error.argtypes = [P]
    L.shipsim_last_error.restype = C.c_char_p
    L.shipsim_set_stream.argtypes = [P, P]
    L.shipsim_num_envs.argtypes = [P]
    L.shipsim_num_envs.restype = C.c_int32
    L.shipsim_lanes_per_env.argtypes = [P]
    L.shipsim_lanes_per_env.restype = C.c_int32
    L.shipsim_reset.argtypes = [P, P, P]
    L.shipsim_step.argtypes = [P, P, P, C.c_int32, P, P, P, P, P, P]
    L.shipsim_tick.argtypes = [P, C.c_int32, P]
    L.shipsim_get_state.argtypes = [P, C.c_int32, P]
    L.shipsim_set_state.argtypes = [P, C.c_int32, P]
    L.shipsim_synchronize.argtypes = [P]
    L.shipsim_nonfinite_count.argtypes = [P]
    L.shipsim_nonfinite_count.restype = C.c_int32
    L.shipsim_set_trajectory.argtypes = [P, P, P, C.c_int32, P]
    L.shipsim_sbmpc_eval.argtypes = [C.c_int32, C.c_double, C.c_double, P, P, P]
    L.shipsim_legacy_step.argtypes = [P, C.c_int32, P, P, P]
    L.shipsim_run_table.argtypes = [P, P, C.c_int32, C.c_int32, C.c_int32, P, P, P, P, P, C.c_int32, P]
    L.shipsim_set_stream_tail.argtypes = [P, C.c_int32]
    # entry points added in later ABI versions: each bound on its own, so an explicitly chosen older build (SHIPSIM_LIB,
    # A/B timing only) that lacks one still gets the argument types of every other
    for name, argtypes in (("shipsim_div_check", [C.c_int32, P, P, P, P, P]),
                           ("shipsim_diag_lane_faults", [P]),
                           ("shipsim_run_policy", [P, P, P, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, P, C.c_int32,
                                                   C.c_int32, P, P, P, P, P, C.c_int32, P]),
                           ("shipsim_sbmpc_eval_multi", [C.c_int32, C.c_int32, C.c_double, C.c_double, P, P, P]),
                           ("shipsim_set_weather", [P, P, P, P, P]),
                           ("shipsim_get_weather", [P, P, P, P, P]),
                           ("shipsim_state_bytes", [P]),
                           ("shipsim_snapshot", [P, P, C.c_int64]),
                           ("shipsim_restore", [P, P, C.c_int64]),
                           ("shipsim_fork", [P, P, C.c_int64, P]),
                           ("shipsim_resample_workspace_bytes", [C.c_int32]),
                           ("shipsim_resample", [C.c_int32, P, P, C.c_uint64, P, C.c_int32, P, C.c_int64, P, P, P, P, P]),
                           ("shipsim_level_distance", [P, P]),
                           ("shipsim_archive_bytes", [P, C.c_int32]),
                           ("shipsim_archive_store", [P, P, C.c_int64, C.c_int32, P]),
                           ("shipsim_archive_load", [P, P, C.c_int64, C.c_int32, P]),
                           ("shipsim_archive_workspace_bytes", [C.c_int32]),
                           ("shipsim_archive_elect", [C.c_int32, C.c_int32, P, P, P, P, P, C.c_int64, P, P, P]),
                           ("shipsim_set_stream_grouping", [P, C.c_int32]),
                           ("shipsim_get_stream_grouping", [P, P]),
                           ("shipsim_sbmpc_nominal", [C.c_int32, C.c_double, C.c_double, P, P, P]),
                           ("shipsim_tickmath_eval", [C.c_int32, C.c_int32, P, P, P]),
                           ("shipsim_tree_bytes", [C.c_int32, C.c_int32]),
                           ("shipsim_tree_layout", [C.c_int32, C.c_int32, P]),
                           ("shipsim_tree_workspace_bytes", [C.c_int32, C.c_int32]),
                           ("shipsim_tree_init", [P, C.c_int64, C.c_int32, C.c_int32, P]),
                           ("shipsim_tree_select", [P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_double, P, C.c_int64, P, P, P]),
                           ("shipsim_tree_expand", [P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, P, P, P, P, C.c_int64,
                                                    P, P]),
                           ("shipsim_tree_backup", [P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, P, P, P, P]),
                           ("shipsim_tree_init_forest", [P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, P]),
                           ("shipsim_tree_select_forest", [P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P,
                                                           C.c_int32, C.c_int32, C.c_int32, C.c_double, P, C.c_int64, P,
                                                           P, P]),
                           ("shipsim_weather_bytes", [C.c_int32]),
                           ("shipsim_weather_store", [P, P, C.c_int64, C.c_int32, P]),
                           ("shipsim_weather_load", [P, P, C.c_int64, C.c_int32, P]),
                           ("shipsim_weather_fork", [P, P])):
        try:
            getattr(L, name).argtypes = argtypes
            if name in ("shipsim_state_bytes", "shipsim_resample_workspace_bytes", "shipsim_archive_bytes",
                        "shipsim_archive_workspace_bytes", "shipsim_tree_bytes", "shipsim_tree_workspace_bytes",
                        "shipsim_weather_bytes"):
                getattr(L, name).restype = C.c_int64
        except AttributeError:
            if "SHIPSIM_LIB" not in os.environ:
                raise
    if L.shipsim_abi_version() != abi.ABI_VERSION:
        raise ShipSimError(f"ABI mismatch: library {L.shipsim_abi_version()} vs binding {abi.ABI_VERSION}")
    from .build_hash import check_library
    try:
        check_library("shipsim", L.shipsim_build_info().decode(), path, explicit="SHIPSIM_LIB" in os.environ)
    except RuntimeError as e:
        raise ShipSimError(str(e)) from None
    _lib = L
    return L


EXPORTED_SYMBOLS = ("shipsim_abi_version", "shipsim_build_info", "shipsim_default_config", "shipsim_create",
                    "shipsim_destroy", "shipsim_last_error", "shipsim_num_envs", "shipsim_reset", "shipsim_step",
                    "shipsim_tick", "shipsim_get_state", "shipsim_set_state", "shipsim_synchronize",
                    "shipsim_set_trajectory", "shipsim_sbmpc_eval", "shipsim_legacy_step", "shipsim_run_table",
                    "shipsim_nonfinite_count", "shipsim_lanes_per_env", "shipsim_set_stream",
                    "shipsim_run_policy", "shipsim_diag_lane_faults", "shipsim_set_stream_tail", "shipsim_div_check",
                    "shipsim_sbmpc_eval_multi", "shipsim_set_weather", "shipsim_get_weather",
                    "shipsim_state_bytes", "shipsim_snapshot", "shipsim_restore", "shipsim_fork",
                    "shipsim_resample_workspace_bytes", "shipsim_resample", "shipsim_level_distance",
                    "shipsim_archive_bytes", "shipsim_archive_store", "shipsim_archive_load",
                    "shipsim_archive_workspace_bytes", "shipsim_archive_elect", "shipsim_set_stream_grouping",
                    "shipsim_get_stream_grouping", "shipsim_sbmpc_nominal", "shipsim_tree_bytes", "shipsim_tree_layout",
                    "shipsim_tree_workspace_bytes", "shipsim_tree_init", "shipsim_tree_select", "shipsim_tree_expand",
                    "shipsim_tree_backup", "shipsim_weather_bytes", "shipsim_weather_store", "shipsim_weather_load",
                    "shipsim_weather_fork", "shipsim_tickmath_eval", "shipsim_tree_init_forest",
                    "shipsim_tree_select_forest")


class Snapshot:
    """The complete dynamic state of every env of a handle (ShipSim.snapshot): `data`, a uint8 device tensor of
    state_bytes, and the shape it belongs to — kind, n_envs, n_ships — with the build string of the library that
    wrote it (the layout of the bytes is that build's). `weather`: None, or the per-env weather in force when it
    was taken (snapshot(weather=True)), a (WEATHER_ROWS, n_envs) float64 device tensor (shipsim_weather_store)."""

    __slots__ = ("data", "kind", "n_envs", "n_ships", "build", "weather")

    def __init__(self, data, kind, n_envs, n_ships, build, weather=None):
        self.data, self.kind, self.n_envs, self.n_ships, self.build = data, int(kind), int(n_envs), int(n_ships), build
        self.weather = weather

    def clone(self):
        return Snapshot(self.data.clone(), self.kind, self.n_envs, self.n_ships, self.build,
                        None if self.weather is None else self.weather.clone())


class StateArchive:
    """A store of env states whose size is the caller's choice (ShipSim.archive): `data`, a zero-initialised uint8
    device tensor holding the state block of n_cells envs (include/shipsim.h: shipsim_archive_store), with what an
    archive keeps per cell beside it — `cell_score` (float64, NaN: the cell is empty), `cell_seen` (int32: the
    candidates the cell has had) and `carry`, the per-cell copies of the caller's per-env tensors — and the shape it
    belongs to: kind, n_ships and the build string of the library that laid it out. Any handle of that kind, ship
    count and build, whatever its n_envs, may store into it and load from it (`sim`; default: the handle it was
    made by). Weather is not state: it stays with the slot, as under fork(weather="keep") — unless the archive
    was made with weather=True: then it owns `weather`, a zeroed (WEATHER_ROWS, n_cells) float64 tensor, and store,
    load and update move the per-env weather of the handle (which must have it in force) by the same index arrays
    they move the state with (shipsim_weather_store / _load). Every method is
    asynchronous on the current stream, without a host round trip or an allocation after the first call with the
    same carry keys, and can be captured into a graph."""

    def __init__(self, sim, n_cells, weather=False):
        n_cells = int(n_cells)
        if not 1 <= n_cells <= abi.ARCHIVE_MAX_CELLS:
            raise ShipSimError(f"archive: n_cells must be in 1..{abi.ARCHIVE_MAX_CELLS}, not {n_cells}")
        if weather and not sim._weather_on:
            raise ShipSimError("archive: weather=True needs a handle with per-env weather in force (set_weather)")
        self.sim, self.n_cells, self.device = sim, n_cells, sim.device
        self.kind, self.n_ships, self.build = int(sim.cfg.kind), sim.n_ships, sim.L.shipsim_build_info().decode()
        nbytes = int(sim.L.shipsim_archive_bytes(sim.h, n_cells))
        if nbytes < 0:
            raise ShipSimError(f"shipsim_archive_bytes failed ({nbytes})")
        dev = self.device
        self.data = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.cell_score = torch.full((n_cells,), float("nan"), dtype=torch.float64, device=dev)
        self.cell_seen = torch.zeros(n_cells, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(int(sim.L.shipsim_archive_workspace_bytes(n_cells)), dtype=torch.uint8, device=dev)
        self.env_of_cell = torch.full((n_cells,), -1, dtype=torch.int32, device=dev)
        self.n_improved = torch.zeros(1, dtype=torch.int32, device=dev)
        self.carry = {}
        self.weather = torch.zeros((abi.WEATHER_ROWS, n_cells), dtype=torch.float64, device=dev) if weather else None

    def as_snapshot(self):
        """The archive's bytes as a Snapshot of n_cells envs (they share the memory): what restore() and
        fork(source=) of a handle of n_envs == n_cells take."""
        return Snapshot(self.data, self.kind, self.n_cells, self.n_ships, self.build, self.weather)

    def _handle(self, sim, what):
        sim = self.sim if sim is None else sim
        mine = (self.kind, self.n_ships)
        if (int(sim.cfg.kind), sim.n_ships) != mine:
            raise ShipSimError(f"{what}: the archive is of (kind, n_ships) = {mine}, the handle of "
                               f"{(int(sim.cfg.kind), sim.n_ships)}")
        build = sim.L.shipsim_build_info().decode()
        if self.build != build:
            raise ShipSimError(f"{what}: the archive was laid out by another build ({self.build!r}, this is {build!r})")
        if sim.device != self.device:
            raise ShipSimError(f"{what}: the archive is on {self.device}, the handle on {sim.device}")
        if self.weather is not None and not sim._weather_on:
            raise ShipSimError(f"{what}: the archive carries weather, the handle has no per-env weather in force")
        return sim

    def _index(self, x, n, what):
        t = torch.as_tensor(x, dtype=torch.int32, device=self.device).contiguous().reshape(-1)
        if t.numel() != n:
            raise ShipSimError(f"{what}: the index array has {t.numel()} entries, expected {n}")
        return t

    def store(self, env_of_cell, sim=None):
        """Cell c takes the live state of env env_of_cell[c] (shipsim_archive_store); an index outside [0, n_envs)
        leaves the cell as it is. Returns the index tensor used."""
        sim = self._handle(sim, "archive store")
        idx = self._index(env_of_cell, self.n_cells, "archive store")
        sim._follow_stream()
        sim._check(sim.L.shipsim_archive_store(sim.h, _ptr(self.data), self.data.numel(), self.n_cells, _ptr(idx)),
                   "shipsim_archive_store")
        if self.weather is not None:
            sim._weather_store(self.weather, idx)
        self._keep = idx
        return idx

    def load(self, cell_of_env, carry=None, sim=None):
        """Env i takes the state of cell cell_of_env[i] (shipsim_archive_load), and entry i of every tensor of
        `carry` — a dict of per-env tensors under keys update() has carried — the cell's copy; an index outside
        [0, n_cells) leaves env i and its entries alone. Returns the index tensor used."""
        sim = self._handle(sim, "archive load")
        idx = self._index(cell_of_env, sim.n_envs, "archive load")
        for k in (carry or {}):
            if k not in self.carry:
                raise ShipSimError(f"archive load: no update() has carried {k!r}")
        sim._follow_stream()
        sim._check(sim.L.shipsim_archive_load(sim.h, _ptr(self.data), self.data.numel(), self.n_cells, _ptr(idx)),
                   "shipsim_archive_load")
        if self.weather is not None:
            sim._weather_load(self.weather, idx)
        if carry:
            ok = (idx >= 0) & (idx < self.n_cells)
            at = idx.clamp(0, self.n_cells - 1).long()
            for k, t in carry.items():
                kept = self.carry[k][at]
                t.copy_(torch.where(ok.view(-1, *([1] * (t.dim() - 1))), kept, t))
        self._keep = idx
        return idx

    def update(self, cell, score, carry=None, sim=None):
        """Elect, then store, in one call: per cell the best-scoring env among those cell[i] names (archive_elect:
        NaN scores and cells outside [0, n_cells) do not take part, ties go to the lowest env index) takes the cell if
        it is empty or strictly improved — its state (store), its score (cell_score) and its entries of `carry`, a
        dict of per-env tensors (ep_idx, dec_idx, log_len, a policy counter, weights ...) of which the archive keeps a
        per-cell copy under the same key. Returns (env_of_cell, n_improved): (n_cells,) and (1,) int32 device
        tensors owned by the archive (the next update overwrites them), -1 where a cell stayed; nothing is copied to
        the host."""
        sim = self._handle(sim, "archive update")
        archive_elect(cell, score, self.cell_score, self.cell_seen, workspace=self.workspace,
                      out_env_of_cell=self.env_of_cell, out_n_improved=self.n_improved, n_envs=sim.n_envs)
        self.store(self.env_of_cell, sim=sim)
        if carry:
            took = self.env_of_cell >= 0
            at = self.env_of_cell.clamp(min=0).long()
            for k, t in carry.items():
                if t.shape[0] != sim.n_envs or t.device != self.device:
                    raise ShipSimError(f"archive update: carry[{k!r}] must be a device tensor of {sim.n_envs} rows")
                if k not in self.carry:
                    self.carry[k] = torch.zeros((self.n_cells,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
                kept = self.carry[k]
                kept.copy_(torch.where(took.view(-1, *([1] * (t.dim() - 1))), t[at], kept))
        return self.env_of_cell, self.n_improved


def diag_lane_faults():
    """Lane / index check violations of a diagnostics build (-DSHIPSIM_LANECHECK) since the last call:
    dict(violations, site, exec), or None for the default build."""
    out = (C.c_uint32 * 32)()
    if load_library().shipsim_diag_lane_faults(out) != 0:
        return None
    return dict(violations=int(out[0]), site=int(out[1]), exec=(int(out[3]) << 32) | int(out[2]),
                per_site={i: int(out[8 + i]) for i in range(16) if out[8 + i]})


def default_config(kind=abi.KIND_AST, machinery=abi.MACH_DETAILED, collav=abi.COLLAV_SBMPC, time_step=4.0):
    cfg = abi.Config()
    rc = load_library().shipsim_default_config(kind, machinery, collav, time_step, C.byref(cfg))
    if rc:
        raise ShipSimError(f"shipsim_default_config failed ({rc})")
    return cfg


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class ShipSim:
    """N independent environments on one device, state resident in HBM."""

    def __init__(self, cfg, n_envs, device=None, n_obs_ships=0):
        """n_obs_ships: obstacle ships per env (AST; 0 = cfg.n_ships - 1, see shipsim_create)."""
        if not torch.cuda.is_available():
            raise ShipSimError("ShipSim needs a HIP device (torch.cuda.is_available() is False)")
        self.L = load_library()
        # a private copy: the caller's config is left as it was (n_obs_ships only applies to this handle)
        cfg = abi.Config.from_buffer_copy(cfg)
        self.n_envs = int(n_envs)
        if n_obs_ships > 0 and cfg.kind == abi.KIND_AST:
            cfg.n_ships = 1 + int(n_obs_ships)
        self.cfg = cfg
        self.n_ships = int(cfg.n_ships)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream(self.device)
            h = C.c_void_p()
            rc = self.L.shipsim_create(C.byref(cfg), self.n_envs, int(n_obs_ships), self.device.index,
                                       C.c_void_p(self.stream.cuda_stream), C.byref(h))
            if rc:
                msg = self.L.shipsim_last_error(h if h.value else None).decode()
                if h.value:
                    self.L.shipsim_destroy(h)
                raise ShipSimError(f"shipsim_create failed ({rc}): {msg}")
        self.h = h
        self._stream_ptr = self.stream.cuda_stream
        self.lanes_per_env = int(self.L.shipsim_lanes_per_env(h))
        self._weather_on = False

    def _follow_stream(self):
        """Launch on torch's current stream of the device (e.g. a graph-capturing one): shipsim_set_stream
        when it changed since the last call."""
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream_ptr:
            self._check(self.L.shipsim_set_stream(self.h, C.c_void_p(s)), "shipsim_set_stream")
            self._stream_ptr = s

    def _check(self, rc, what):
        if rc:
            raise ShipSimError(f"{what} failed ({rc}): {self.L.shipsim_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.shipsim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, x, dtype):
        if x is None:
            return None
        t = torch.as_tensor(x, dtype=dtype, device=self.device).contiguous()
        return t

    def reset(self, mask=None, obs_out=None):
        m = self._dev(mask, torch.uint8) if mask is not None else None
        obs = obs_out if obs_out is not None else torch.empty((self.n_envs, 8), dtype=torch.float32, device=self.device)
        self._follow_stream()
        self._check(self.L.shipsim_reset(self.h, _ptr(m), _ptr(obs)), "shipsim_reset")
        return obs

    def step(self, action, active=None, max_ticks=0, out=None):
        """One sliced decision step (shipsim_step). action: (N,) or (N,1) float32 scoping angles
        [rad] (already denormalized); consumed only by envs waiting for a decision. With
        max_ticks <= 0 every active env runs to its decision point (out['ready'] all ones)."""
        a = self._dev(action, torch.float32).reshape(-1)
        if a.numel() != self.n_envs:
            raise ShipSimError(f"action has {a.numel()} entries, expected {self.n_envs}")
        act = self._dev(active, torch.uint8) if active is not None else None
        if out is None:
            out = dict(obs=torch.empty((self.n_envs, 8), dtype=torch.float32, device=self.device),
                       reward=torch.empty(self.n_envs, dtype=torch.float64, device=self.device),
                       done=torch.empty(self.n_envs, dtype=torch.uint8, device=self.device),
                       events=torch.empty(self.n_envs, dtype=torch.int32, device=self.device),
                       ticks=torch.empty(self.n_envs, dtype=torch.int32, device=self.device),
                       ready=torch.empty(self.n_envs, dtype=torch.uint8, device=self.device))
        self._follow_stream()
        self._check(self.L.shipsim_step(self.h, _ptr(a), _ptr(act), int(max_ticks), _ptr(out["obs"]), _ptr(out["reward"]),
                                        _ptr(out["done"]), _ptr(out["events"]), _ptr(out["ticks"]),
                                        _ptr(out.get("ready"))), "shipsim_step")
        self._keep = (a, act)
        return out

    def tick(self, k=1, events=None):
        """k raw ticks of the loop body (shipsim_tick: SINGLE, and NONIW's MultiShipNonIWEnv._step). events: an
        optional (N,) int32 / uint32 device tensor for the env_info bits of the last tick (NONIW)."""
        self._follow_stream()
        self._check(self.L.shipsim_tick(self.h, int(k), _ptr(events)), "shipsim_tick")

    def set_stream_tail(self, extra_ticks):
        """Work-conserving launch tail of run_table / run_policy (shipsim_set_stream_tail): a wave whose envs met
        max_ticks keeps ticking, 32 ticks at a time, while any wave of the launch has not, up to extra_ticks more
        (0: off). Per-env results are unchanged; only where launches end moves."""
        self._check(self.L.shipsim_set_stream_tail(self.h, int(extra_ticks)), "shipsim_set_stream_tail")
        self.stream_tail = int(extra_ticks)

    def set_stream_grouping(self, on):
        """Grouping of run_table / run_policy envs into waves by episode phase (shipsim_set_stream_grouping; from
        create on for two-ship envs with collav sbmpc, off otherwise): each launch orders the envs by ticks since
        their last reset, so wave-mates share SBMPC passes. Per-env results are unchanged, bit for bit."""
        self._check(self.L.shipsim_set_stream_grouping(self.h, int(bool(on))), "shipsim_set_stream_grouping")
        self.stream_grouping = bool(on)

    def get_stream_grouping(self):
        """(n_envs,) int32 device tensor: the env each slot of the last stream launch ran
        (shipsim_get_stream_grouping); the identity before the first launch and after one with grouping off."""
        t = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        self._follow_stream()
        self._check(self.L.shipsim_get_stream_grouping(self.h, _ptr(t)), "shipsim_get_stream_grouping")
        return t

    def run_table(self, table, max_ticks, ep_idx, dec_idx, out=None, log=None, log_len=None):
        """Open-loop decision stream (shipsim_run_table): table (n_eps, n_dec, N) float32 scoping angles
        on the device; ep_idx / dec_idx (N,) int32 device counters, updated in place. Returns
        dict(ticks=(N,) int32, decisions=(N,) int32). log: optional (N, cap, DECLOG_COLS) float64 with
        log_len (N,) int32."""
        t = self._dev(table, torch.float32)
        if t.dim() != 3 or t.shape[2] != self.n_envs:
            raise ValueError(f"table must be (n_eps, n_dec, {self.n_envs})")
        for x in (ep_idx, dec_idx):
            if x.dtype != torch.int32 or x.device != self.device or x.numel() != self.n_envs:
                raise ValueError("ep_idx / dec_idx must be int32 device tensors of n_envs elements")
        if out is None:
            out = dict(ticks=torch.zeros(self.n_envs, dtype=torch.int32, device=self.device),
                       decisions=torch.zeros(self.n_envs, dtype=torch.int32, device=self.device))
        cap = int(log.shape[1]) if log is not None else 0
        self._follow_stream()
        self._check(self.L.shipsim_run_table(self.h, _ptr(t), int(t.shape[0]), int(t.shape[1]), int(max_ticks),
                                             _ptr(ep_idx), _ptr(dec_idx), _ptr(out["ticks"]), _ptr(out["decisions"]),
                                             _ptr(log), cap, _ptr(log_len)), "shipsim_run_table")
        self._keep_table = t
        return out

    def run_policy(self, policy, max_ticks, n_dec, ep_idx, dec_idx, deterministic=False, seed=0, counter=None,
                   out=None, log=None, log_len=None):
        """The decision stream with the policy in the loop (shipsim_run_policy). policy: (params_ptr, w2t_ptr,
        obs_dim, hidden) as SacFused.policy_weights() returns; counter: (1,) int64 device tensor read by the
        launch (the caller advances it between calls); n_dec: decisions per episode (max_path_length).
        Other arguments and the result as run_table."""
        params, w2t, obs_dim, hidden = policy
        for x in (ep_idx, dec_idx):
            if x.dtype != torch.int32 or x.device != self.device or x.numel() != self.n_envs:
                raise ValueError("ep_idx / dec_idx must be int32 device tensors of n_envs elements")
        if counter is not None and (counter.dtype != torch.int64 or counter.device != self.device):
            raise ValueError("counter must be an int64 device tensor")
        if out is None:
            out = dict(ticks=torch.zeros(self.n_envs, dtype=torch.int32, device=self.device),
                       decisions=torch.zeros(self.n_envs, dtype=torch.int32, device=self.device))
        cap = int(log.shape[1]) if log is not None else 0
        self._follow_stream()
        self._check(self.L.shipsim_run_policy(self.h, C.c_void_p(params), C.c_void_p(w2t), int(obs_dim), int(hidden),
                                              int(bool(deterministic)), int(seed) & ((1 << 64) - 1), _ptr(counter),
                                              int(n_dec), int(max_ticks), _ptr(ep_idx), _ptr(dec_idx),
                                              _ptr(out["ticks"]), _ptr(out["decisions"]), _ptr(log), cap,
                                              _ptr(log_len)), "shipsim_run_policy")
        return out

    def legacy_step(self, k=1, out=None):
        """k legacy MultiShipEnv.step() ticks of every env (shipsim_legacy_step): dict(states=(N, 8) f64
        next_states, done=(N,) u8, status=(N,) i32 termination bits LT_*) of each env's last tick."""
        N = self.n_envs
        if out is None:
            out = dict(states=torch.zeros((N, 8), dtype=torch.float64, device=self.device),
                       done=torch.zeros(N, dtype=torch.uint8, device=self.device),
                       status=torch.zeros(N, dtype=torch.int32, device=self.device))
        self._follow_stream()
        self._check(self.L.shipsim_legacy_step(self.h, int(k), _ptr(out["states"]), _ptr(out["done"]),
                                               _ptr(out["status"])), "shipsim_legacy_step")
        return out

    def _field_shape(self, field):
        S, N = self.n_envs * self.n_ships, self.n_envs
        if field < abi.N_SHIP_FIELDS:
            return (S,), torch.int32 if field in abi.INT_FIELDS else torch.float64
        if field == abi.E_ROUTE_LEN:
            return (S,), torch.int32
        if field in (abi.E_ROUTE_NORTH, abi.E_ROUTE_EAST):
            return (S, abi.MAX_ROUTE), torch.float64
        return (N,), torch.int32 if field in abi.INT_FIELDS else torch.float64

    def get(self, field):
        shape, dt = self._field_shape(field)
        t = torch.empty(shape, dtype=dt, device=self.device)
        self._follow_stream()
        self._check(self.L.shipsim_get_state(self.h, int(field), _ptr(t)), "shipsim_get_state")
        return t

    def set(self, field, value):
        shape, dt = self._field_shape(field)
        t = self._dev(value, dt).reshape(shape)
        self._follow_stream()
        self._check(self.L.shipsim_set_state(self.h, int(field), _ptr(t)), "shipsim_set_state")
        self._keep_set = t

    # -- snapshot / restore / fork (include/shipsim.h: shipsim_snapshot) --
    @property
    def state_bytes(self):
        """Bytes of the handle's whole state block (shipsim_state_bytes)."""
        n = int(self.L.shipsim_state_bytes(self.h))
        if n < 0:
            raise ShipSimError(f"shipsim_state_bytes failed ({n})")
        return n

    def snapshot(self, out=None, weather=False):
        """The complete state of every env, mid-decision state included, as a Snapshot on the device (asynchronous
        on the current stream). out: a Snapshot of this handle's shape to overwrite instead of allocating. The
        stream arrays a caller owns (ep_idx, dec_idx, log_len, the policy's counter) are the caller's to keep.
        weather=True: the per-env weather in force goes into the Snapshot's `weather` too (shipsim_weather_store;
        the handle must have per-env weather, and an `out` must hold a weather tensor already)."""
        if weather:
            self._need_weather("snapshot")
        if out is None:
            out = Snapshot(torch.empty(self.state_bytes, dtype=torch.uint8, device=self.device), self.cfg.kind,
                           self.n_envs, self.n_ships, self.L.shipsim_build_info().decode(),
                           torch.empty((abi.WEATHER_ROWS, self.n_envs), dtype=torch.float64, device=self.device)
                           if weather else None)
        else:
            self._check_snapshot(out, "snapshot", weather)
        self._follow_stream()
        self._check(self.L.shipsim_snapshot(self.h, _ptr(out.data), out.data.numel()), "shipsim_snapshot")
        if weather:
            self._weather_store(out.weather, None)
        return out

    # weather that moves with the state (include/shipsim.h: shipsim_weather_store)
    def _need_weather(self, what):
        if not self._weather_on:
            raise ShipSimError(f"{what}: weather=True needs per-env weather in force on the handle (set_weather)")

    def _weather_buffer(self, wx, what):
        if wx is None:
            raise ShipSimError(f"{what}: the source carries no weather (it was taken without weather=True)")
        if wx.dtype != torch.float64 or wx.device != self.device or not wx.is_contiguous() or wx.dim() != 2 \
                or wx.shape[0] != abi.WEATHER_ROWS:
            raise ShipSimError(f"{what}: weather must be a contiguous ({abi.WEATHER_ROWS}, n) float64 tensor on "
                               f"{self.device}")
        return wx

    def _weather_store(self, wx, index):
        wx = self._weather_buffer(wx, "weather store")
        self._check(self.L.shipsim_weather_store(self.h, _ptr(wx), wx.numel() * 8, wx.shape[1], _ptr(index)),
                    "shipsim_weather_store")

    def _weather_load(self, wx, index):
        wx = self._weather_buffer(wx, "weather load")
        self._check(self.L.shipsim_weather_load(self.h, _ptr(wx), wx.numel() * 8, wx.shape[1], _ptr(index)),
                    "shipsim_weather_load")

    def _check_snapshot(self, snap, what, weather=False):
        if not isinstance(snap, Snapshot):
            raise ShipSimError(f"{what}: expected a Snapshot, got {type(snap).__name__}")
        if weather:
            self._need_weather(what)
            w = self._weather_buffer(snap.weather, what)
            if w.shape[1] != snap.n_envs:
                raise ShipSimError(f"{what}: the snapshot's weather has {w.shape[1]} slots, its state {snap.n_envs}")
        mine = (int(self.cfg.kind), self.n_envs, self.n_ships)
        if (snap.kind, snap.n_envs, snap.n_ships) != mine:
            raise ShipSimError(f"{what}: the snapshot is of (kind, n_envs, n_ships) = "
                               f"{(snap.kind, snap.n_envs, snap.n_ships)}, this handle of {mine}")
        build = self.L.shipsim_build_info().decode()
        if snap.build != build:
            raise ShipSimError(f"{what}: the snapshot was written by another build ({snap.build!r}, this is {build!r})")
        d = snap.data
        if d.dtype != torch.uint8 or d.device != self.device or not d.is_contiguous() or d.numel() != self.state_bytes:
            raise ShipSimError(f"{what}: the snapshot's data must be a contiguous uint8 tensor of {self.state_bytes} "
                               f"bytes on {self.device}")

    def restore(self, snap, weather=False):
        """Put a Snapshot back (shipsim_restore): from the next launch on the handle continues, bit for bit, as it
        did after the snapshot was taken, given the caller's own stream arrays as they were. A Snapshot of another
        kind, n_envs, ship count or build is refused before the library is called. weather=True: the weather the
        Snapshot carries goes back too (shipsim_weather_load); one without, or a handle without per-env weather,
        is refused before the library is called."""
        self._check_snapshot(snap, "restore", weather)
        self._follow_stream()
        self._check(self.L.shipsim_restore(self.h, _ptr(snap.data), snap.data.numel()), "shipsim_restore")
        if weather:
            self._weather_load(snap.weather, None)

    def fork(self, src, source=None, weather=False):
        """Env i takes the state of env src[i] (shipsim_fork): of this handle as it is (source None), or of a
        Snapshot. src: (n_envs,) device int32 tensor or anything torch.as_tensor takes; any index array is served
        (permutations, broadcasts, cycles), and an index outside [0, n_envs) leaves env i as it is. A clone runs
        under its new slot's noise and actions, and under its new slot's weather unless weather=True: then env i
        also takes the per-env weather of env src[i] (shipsim_weather_fork), or of slot src[i] of the Snapshot's own
        weather (shipsim_weather_load), on the device and capturable like the fork itself. One paused mid-decision
        resumes without consuming an action. Returns the index tensor used."""
        s = self._dev(src, torch.int32).reshape(-1)
        if s.numel() != self.n_envs:
            raise ShipSimError(f"fork: src has {s.numel()} entries, expected {self.n_envs}")
        if source is not None:
            self._check_snapshot(source, "fork", weather)
        elif weather:
            self._need_weather("fork")
        self._follow_stream()
        self._check(self.L.shipsim_fork(self.h, _ptr(source.data) if source is not None else None, self.state_bytes,
                                        _ptr(s)), "shipsim_fork")
        if weather and source is not None:
            self._weather_load(source.weather, s)
        elif weather:
            self._check(self.L.shipsim_weather_fork(self.h, _ptr(s)), "shipsim_weather_fork")
        self._keep_fork = s
        return s

    def level_distance(self, out=None):
        """Per env, the own ship's distance to the nearest obstacle ship (shipsim_level_distance): an (n_envs,)
        float64 device tensor, the level a splitting potential is built from. AST and NONIW handles, after a reset."""
        if out is None:
            out = torch.empty(self.n_envs, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.device != self.device or not out.is_contiguous() \
                or out.numel() != self.n_envs:
            raise ShipSimError(f"level_distance: out must be a contiguous float64 tensor of {self.n_envs} on {self.device}")
        self._follow_stream()
        self._check(self.L.shipsim_level_distance(self.h, _ptr(out)), "shipsim_level_distance")
        return out

    def archive(self, n_cells, weather=False):
        """A StateArchive of n_cells cells for handles of this one's kind and ship count (include/shipsim.h:
        shipsim_archive_store): zeroed, every cell empty. weather=True: it also keeps, per cell, the per-env weather
        of the env stored (this handle must have per-env weather in force). Allocates; call it outside graph
        capture."""
        return StateArchive(self, n_cells, weather=weather)

    # -- per-env weather (include/shipsim.h: shipsim_set_weather) --
    WEATHER_KEYS = ("wind_speed", "wind_direction", "current_north", "current_east")

    def set_weather(self, wind_speed, wind_direction, current_north, current_east):
        """Per-env wind and current (shipsim_set_weather): four array-likes of n_envs values (m/s, rad, m/s from
        north, m/s from east), a scalar broadcasts. From the next launch on env i runs under its values, with the
        results of a uniform handle whose config carries them; they persist across resets. A setup call (it
        waits for the upload): not during graph capture. lanes_per_env follows what the weather kernels run."""
        arrs = []
        for name, x in zip(self.WEATHER_KEYS, (wind_speed, wind_direction, current_north, current_east)):
            a = np.asarray(x, dtype=np.float64)
            if a.ndim == 0:
                a = np.full(self.n_envs, float(a))
            a = np.ascontiguousarray(a.reshape(-1))
            if a.size != self.n_envs:
                raise ShipSimError(f"set_weather: {name} has {a.size} entries, expected {self.n_envs}")
            arrs.append(a)
        self._follow_stream()
        self._check(self.L.shipsim_set_weather(self.h, *[C.c_void_p(a.ctypes.data) for a in arrs]),
                    "shipsim_set_weather")
        self._weather_on = True
        self.lanes_per_env = int(self.L.shipsim_lanes_per_env(self.h))

    def clear_weather(self):
        """Back to the config's uniform weather and the uniform kernels."""
        self._check(self.L.shipsim_set_weather(self.h, None, None, None, None), "shipsim_set_weather")
        self._weather_on = False
        self.lanes_per_env = int(self.L.shipsim_lanes_per_env(self.h))

    def weather(self):
        """dict of four float64 arrays of n_envs (WEATHER_KEYS): what set_weather set, moved as fork, restore and an
        archive's load have moved it since (then read back from the device, after a wait for the handle's stream);
        None when uniform."""
        if not self._weather_on:
            return None
        out = [np.empty(self.n_envs, dtype=np.float64) for _ in self.WEATHER_KEYS]
        self._follow_stream()  # (the stream a readback waits for)
        self._check(self.L.shipsim_get_weather(self.h, *[C.c_void_p(a.ctypes.data) for a in out]),
                    "shipsim_get_weather")
        return dict(zip(self.WEATHER_KEYS, out))

    # -- trajectory recording (include/shipsim.h: shipsim_set_trajectory) --
    def set_trajectory(self, capacity, env_rows=True):
        """Record every tick's simulation_results row (both ships) and RewardTracker row into device
        tensors of `capacity` rows per env; returns dict(ship=(N*2, cap, 20) f64, env=(N, cap, 8) f64,
        len=(N,) int32, cap). Rows start at the next reset."""
        S = self.n_envs * self.n_ships
        cap = int(capacity)
        t = dict(ship=torch.zeros((S, cap, abi.TRAJ_SHIP_COLS), dtype=torch.float64, device=self.device),
                 env=torch.zeros((self.n_envs, cap, abi.TRAJ_ENV_COLS), dtype=torch.float64, device=self.device)
                 if env_rows else None,
                 len=torch.zeros(self.n_envs, dtype=torch.int32, device=self.device), cap=cap)
        self._check(self.L.shipsim_set_trajectory(self.h, _ptr(t["ship"]), _ptr(t["env"]), cap, _ptr(t["len"])),
                    "shipsim_set_trajectory")
        self.traj = t
        return t

    def clear_trajectory(self):
        self._check(self.L.shipsim_set_trajectory(self.h, None, None, 0, None), "shipsim_set_trajectory")
        self.traj = None

    def synchronize(self):
        """Wait for the handle's stream; raises ShipSimNonFiniteError when env decisions ended on a
        non-finite ship state since the previous call (those envs report SHIPSIM_EV_NONFINITE, done)."""
        rc = self.L.shipsim_synchronize(self.h)
        if rc == abi.ENONFINITE:
            raise ShipSimNonFiniteError(self.L.shipsim_last_error(self.h).decode())
        self._check(rc, "shipsim_synchronize")

    def nonfinite_count(self):
        """Decisions flagged SHIPSIM_EV_NONFINITE since create (as of the last synchronize)."""
        return int(self.L.shipsim_nonfinite_count(self.h))


def div_check(num, den, device="cuda"):
    """The kernels' fp64 division by a reused divisor (reciprocal formed once) beside the plain division, on the
    device: (fast, ref) float64 tensors of num / den (shipsim_div_check)."""
    L = load_library()
    a = torch.as_tensor(num, dtype=torch.float64, device=device).contiguous().reshape(-1)
    d = torch.as_tensor(den, dtype=torch.float64, device=device).contiguous().reshape(-1)
    if a.shape != d.shape:
        raise ShipSimError("num and den must have the same size")
    fast, ref = torch.empty_like(a), torch.empty_like(a)
    stream = torch.cuda.current_stream(a.device)
    rc = L.shipsim_div_check(int(a.numel()), _ptr(a), _ptr(d), _ptr(fast), _ptr(ref), C.c_void_p(stream.cuda_stream))
    if rc:
        raise ShipSimError(f"shipsim_div_check failed ({rc})")
    return fast, ref


def sbmpc_eval(requests, tf=1000.0, dt=20.0, device="cuda"):
    """SBMPC.get_optimal_ctrl_offset on the device for a batch of (n, 17) requests
    [P_ca_last, Chi_ca_last, u_d, chi_d, os_state(6), obstacle(5), obs_l, obs_w] -> (n, 3) tensor
    [speed factor, course offset, active] (shipsim_sbmpc_eval)."""
    L = load_library()
    x = torch.as_tensor(requests, dtype=torch.float64, device=device).contiguous()
    if x.dim() != 2 or x.shape[1] != abi.SBMPC_IN:
        raise ShipSimError(f"requests must be (n, {abi.SBMPC_IN})")
    out = torch.empty((x.shape[0], 3), dtype=torch.float64, device=x.device)
    stream = torch.cuda.current_stream(x.device)
    rc = L.shipsim_sbmpc_eval(int(x.shape[0]), float(tf), float(dt), _ptr(x), _ptr(out), C.c_void_p(stream.cuda_stream))
    if rc:
        raise ShipSimError(f"shipsim_sbmpc_eval failed ({rc})")
    return out


def sbmpc_nominal(requests, tf=1000.0, dt=20.0, device="cuda"):
    """The streams' pass-free test on the device for a batch of (n, 17) sbmpc_eval requests -> (n,) int32 tensor of
    two bits, set where the nominal scenario provably wins, so that sbmpc_eval returns (1.0, 0.0, active): bit 0 by
    the test on sin / cos(chi_d), bit 1 by the form the streams' tick evaluates, on the split course
    (shipsim_sbmpc_nominal)."""
    L = load_library()
    x = torch.as_tensor(requests, dtype=torch.float64, device=device).contiguous()
    if x.dim() != 2 or x.shape[1] != abi.SBMPC_IN:
        raise ShipSimError(f"requests must be (n, {abi.SBMPC_IN})")
    out = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
    stream = torch.cuda.current_stream(x.device)
    rc = L.shipsim_sbmpc_nominal(int(x.shape[0]), float(tf), float(dt), _ptr(x), _ptr(out),
                                 C.c_void_p(stream.cuda_stream))
    if rc:
        raise ShipSimError(f"shipsim_sbmpc_nominal failed ({rc})")
    return out


TICKMATH_FN = {"sincos": 0, "atan": 1, "exp": 2}


def tickmath_eval(fn, x, device="cuda"):
    """The steady tick's math-library call `fn` ("sincos", "atan", "exp") on the device for a batch of arguments ->
    (n, 3, 2) float64 tensor: [:, 0] the device library's value, [:, 1] the restated form's (csrc/shipsim_tickmath.hpp,
    literal constants), [:, 2] the row-broadcast form's the headline streams run; the last axis is (sine, cosine) for
    sincos and (value, 0) otherwise (shipsim_tickmath_eval)."""
    L = load_library()
    a = torch.as_tensor(x, dtype=torch.float64, device=device).contiguous().reshape(-1)
    out = torch.zeros((a.shape[0], 3, 2), dtype=torch.float64, device=a.device)
    stream = torch.cuda.current_stream(a.device)
    rc = L.shipsim_tickmath_eval(TICKMATH_FN[fn], int(a.shape[0]), _ptr(a), _ptr(out), C.c_void_p(stream.cuda_stream))
    if rc:
        raise ShipSimError(f"shipsim_tickmath_eval failed ({rc})")
    return out


def sbmpc_eval_multi(requests, n_obs, tf=1000.0, dt=20.0, device="cuda"):
    """SBMPC.get_optimal_ctrl_offset over a do_list of n_obs obstacles on the device, for a batch of
    (n, SBMPC_MULTI_IN) requests [P_ca_last, Chi_ca_last, u_d, chi_d, os_state(6), then per obstacle slot
    (SHIPSIM_MAX_OBS of them) x, y, psi, u, v, length, width] -> (n, 3) tensor [speed factor, course offset, active]
    (shipsim_sbmpc_eval_multi)."""
    L = load_library()
    x = torch.as_tensor(requests, dtype=torch.float64, device=device).contiguous()
    if x.dim() != 2 or x.shape[1] != abi.SBMPC_MULTI_IN:
        raise ShipSimError(f"requests must be (n, {abi.SBMPC_MULTI_IN})")
    out = torch.empty((x.shape[0], 3), dtype=torch.float64, device=x.device)
    stream = torch.cuda.current_stream(x.device)
    rc = L.shipsim_sbmpc_eval_multi(int(x.shape[0]), int(n_obs), float(tf), float(dt), _ptr(x), _ptr(out),
                                    C.c_void_p(stream.cuda_stream))
    if rc:
        if rc != -1:  # (not SHIPSIM_EINVAL: SHIPSIM_EHIP)
            why = "the launch failed"
        elif not 1 <= int(n_obs) <= abi.MAX_OBS:
            why = f"n_obs {int(n_obs)} must be 1..{abi.MAX_OBS}"
        else:
            why = f"bad argument (tf {float(tf)}, dt {float(dt)}: dt > 0 and tf / dt <= 4096)"
        raise ShipSimError(f"shipsim_sbmpc_eval_multi failed ({rc}): {why}")
    return out


RESAMPLE_SORTED, RESAMPLE_IN_PLACE = 0, 1
RESAMPLE_MAX_N = 1 << 22
_ARRANGEMENTS = {"sorted": RESAMPLE_SORTED, "in_place": RESAMPLE_IN_PLACE}
_resample_ws = {}  # (device, n) -> (workspace, total, status): one set per population size, reused by every call


def resample(weight, potential, seed, counter, arrangement="in_place", out_src=None, out_weight=None):
    """Systematic resampling of n envs in proportion to weight * potential (shipsim_resample): returns
    (src int32, weight float64, total float64 (1,), status int32 (1,)), all on the device. src is what fork() takes;
    weight[j] is what clone j carries so that sum_j weight[j] f(x[src[j]]) stays an unbiased estimate of
    sum_i weight_in[i] f(x[i]); total is the mass the weights preserve; status 0, or 1 (no mass) / 2 (a negative or
    non-finite mass) with src the identity and the weights as given. arrangement "in_place": an env that is selected
    keeps its slot and further clones fill the slots of those that are not; "sorted": src non-decreasing.
    counter: (1,) int64 device tensor read by the launch (the caller advances it between calls). Asynchronous on
    the current stream and capturable; the workspace — and total and status, which the next call of the same size
    overwrites — is cached per (device, n). out_weight may be weight."""
    L = load_library()
    w = torch.as_tensor(weight)
    if not w.is_cuda:
        raise ShipSimError("resample: weight must be a device tensor")
    dev = w.device
    w = w.to(torch.float64).contiguous().reshape(-1)
    p = torch.as_tensor(potential, dtype=torch.float64, device=dev).contiguous().reshape(-1)
    n = int(w.numel())
    if p.numel() != n:
        raise ShipSimError(f"resample: {n} weights and {p.numel()} potentials")
    if not 1 <= n <= RESAMPLE_MAX_N:
        raise ShipSimError(f"resample: n must be in 1..{RESAMPLE_MAX_N}, not {n}")
    if arrangement not in _ARRANGEMENTS:
        raise ShipSimError(f"resample: arrangement must be 'in_place' or 'sorted', not {arrangement!r}")
    if counter.dtype != torch.int64 or counter.device != dev or counter.numel() < 1:
        raise ShipSimError("resample: counter must be an int64 device tensor")
    for name, t, dt in (("out_src", out_src, torch.int32), ("out_weight", out_weight, torch.float64)):
        if t is not None and (t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() != n):
            raise ShipSimError(f"resample: {name} must be a contiguous {dt} tensor of {n} on {dev}")
    key = (dev.index, n)
    if key not in _resample_ws:
        need = int(L.shipsim_resample_workspace_bytes(n))
        _resample_ws[key] = (torch.empty(need, dtype=torch.uint8, device=dev),
                             torch.zeros(1, dtype=torch.float64, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev))
    ws, total, status = _resample_ws[key]
    src = out_src if out_src is not None else torch.empty(n, dtype=torch.int32, device=dev)
    wout = out_weight if out_weight is not None else torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        rc = L.shipsim_resample(n, _ptr(w), _ptr(p), int(seed) & ((1 << 64) - 1), _ptr(counter),
                                _ARRANGEMENTS[arrangement], _ptr(ws), ws.numel(), _ptr(src), _ptr(wout), _ptr(total),
                                _ptr(status), C.c_void_p(stream.cuda_stream))
    if rc:
        raise ShipSimError(f"shipsim_resample failed ({rc})")
    return src, wout, total, status


ARCHIVE_MAX_CELLS = abi.ARCHIVE_MAX_CELLS
_elect_ws = {}  # (device, n_cells) -> workspace: one per archive size, reused by every call that brings none


def archive_elect(cell, score, cell_score, cell_seen=None, workspace=None, out_env_of_cell=None, out_n_improved=None,
                  n_envs=None):
    """Which env each cell of an archive takes (shipsim_archive_elect): env i is a candidate of cell cell[i] when that
    index is in [0, n_cells) and score[i] is not NaN; a cell's winner is its candidate of the largest score (IEEE >,
    ties to the lowest env index) and takes the cell when cell_score[c] is NaN (empty) or its score is strictly
    greater. cell: (n_envs,) int32, score: (n_envs,) float64, cell_score: (n_cells,) float64, updated in place,
    cell_seen: optional (n_cells,) int32, += the cell's candidates; all device tensors. Returns (env_of_cell int32
    (n_cells,), -1 where the cell stays; n_improved int32 (1,)): env_of_cell is what StateArchive.store takes.
    Asynchronous on the current stream and capturable; without `workspace` one is cached per (device, n_cells)."""
    L = load_library()
    cs = cell_score
    if not isinstance(cs, torch.Tensor) or not cs.is_cuda or cs.dtype != torch.float64 or not cs.is_contiguous():
        raise ShipSimError("archive_elect: cell_score must be a contiguous float64 device tensor")
    dev, m = cs.device, int(cs.numel())
    c = torch.as_tensor(cell, dtype=torch.int32, device=dev).contiguous().reshape(-1)
    s = torch.as_tensor(score, dtype=torch.float64, device=dev).contiguous().reshape(-1)
    n = int(c.numel())
    if s.numel() != n or (n_envs is not None and n != int(n_envs)):
        raise ShipSimError(f"archive_elect: {n} cells and {s.numel()} scores for {n if n_envs is None else n_envs} envs")
    if not 1 <= m <= ARCHIVE_MAX_CELLS or not 1 <= n <= RESAMPLE_MAX_N:
        raise ShipSimError(f"archive_elect: n_cells must be in 1..{ARCHIVE_MAX_CELLS} and n_envs in 1..{RESAMPLE_MAX_N}, "
                           f"not {m} and {n}")
    for name, t, k in (("cell_seen", cell_seen, m), ("out_env_of_cell", out_env_of_cell, m),
                       ("out_n_improved", out_n_improved, 1)):
        if t is not None and (t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() != k):
            raise ShipSimError(f"archive_elect: {name} must be a contiguous int32 tensor of {k} on {dev}")
    if workspace is None:
        key = (dev.index, m)
        if key not in _elect_ws:
            _elect_ws[key] = torch.empty(int(L.shipsim_archive_workspace_bytes(m)), dtype=torch.uint8, device=dev)
        workspace = _elect_ws[key]
    eoc = out_env_of_cell if out_env_of_cell is not None else torch.empty(m, dtype=torch.int32, device=dev)
    k_out = out_n_improved if out_n_improved is not None else torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        rc = L.shipsim_archive_elect(n, m, _ptr(c), _ptr(s), _ptr(cs), _ptr(cell_seen), _ptr(workspace),
                                     workspace.numel(), _ptr(eoc), _ptr(k_out), C.c_void_p(stream.cuda_stream))
    if rc:
        raise ShipSimError(f"shipsim_archive_elect failed ({rc})")
    return eoc, k_out


TREE_MAX_CHILDREN, TREE_MAX_DEPTH, TREE_MAX_WORKERS = abi.TREE_MAX_CHILDREN, abi.TREE_MAX_DEPTH, abi.TREE_MAX_WORKERS
TREE_FIELDS = ("header", "parent", "depth", "n_children", "child", "visits", "value_sum", "action", "flags")
_TREE_DTYPES = dict(header=torch.int32, parent=torch.int32, depth=torch.int32, n_children=torch.int32, child=torch.int32,
                    visits=torch.int32, value_sum=torch.int64, action=torch.float32, flags=torch.int32)


def tree_layout(max_nodes, max_children):
    """Byte offsets of a tree buffer's arrays (shipsim_tree_layout): dict over TREE_FIELDS, and 'bytes', its size."""
    out = (C.c_int64 * 10)()
    if load_library().shipsim_tree_layout(int(max_nodes), int(max_children), out):
        raise ShipSimError(f"tree: max_nodes must be in 1..{ARCHIVE_MAX_CELLS} and max_children in "
                           f"1..{TREE_MAX_CHILDREN}, not {max_nodes} and {max_children}")
    return dict(zip(TREE_FIELDS + ("bytes",), (int(v) for v in out)))


class SearchTree:
    """A search tree on the device (include/shipsim.h: shipsim_tree_*): `data`, the tree buffer as a uint8 tensor;
    its arrays as tensors that share its memory — header (int32[4]: n_nodes, dropped, skipped), parent, depth,
    n_children, child (max_nodes, max_children), visits, value_sum (int64, 24 fractional bits), action, flags — and
    the workspace of its calls, sized for n_workers. Node i is cell i of a StateArchive of max_nodes cells. Made with
    the one-node tree in it; every method is asynchronous on the current stream, allocates nothing and can be
    captured into a graph. n_roots = R > 1 makes a forest (shipsim_tree_init_forest): R roots, nodes 0..R-1, in the
    one pool, each the root of a tree of its own; header[3] is then R, and select takes the workers per root."""

    def __init__(self, max_nodes, max_children, n_workers, n_roots=1, device="cuda"):
        L = load_library()
        self.max_nodes, self.max_children, self.n_workers = int(max_nodes), int(max_children), int(n_workers)
        self.n_roots = int(n_roots)
        self.layout = tree_layout(self.max_nodes, self.max_children)
        if not 1 <= self.n_workers <= TREE_MAX_WORKERS:
            raise ShipSimError(f"tree: n_workers must be in 1..{TREE_MAX_WORKERS}, not {n_workers}")
        if not 1 <= self.n_roots <= min(self.max_nodes, self.n_workers):
            raise ShipSimError(f"tree: n_roots must be in 1..min(max_nodes, n_workers), not {n_roots}")
        self.device = dev = torch.device(device)
        if dev.index is None:
            self.device = dev = torch.device(dev.type, torch.cuda.current_device())
        self.data = torch.zeros(self.layout["bytes"], dtype=torch.uint8, device=dev)
        M, Cc = self.max_nodes, self.max_children
        for name in TREE_FIELDS:
            dt = _TREE_DTYPES[name]
            count = dict(header=4, child=M * Cc).get(name, M)
            o = self.layout[name]
            setattr(self, name, self.data[o:o + count * dt.itemsize].view(dt))
        self.child = self.child.view(M, Cc)
        self.workspace = torch.empty(int(L.shipsim_tree_workspace_bytes(M, self.n_workers)), dtype=torch.uint8, device=dev)
        self.leaf = torch.empty(self.n_workers, dtype=torch.int32, device=dev)
        self.expand_flag = torch.empty(self.n_workers, dtype=torch.int32, device=dev)
        self.node = torch.empty(self.n_workers, dtype=torch.int32, device=dev)
        # the even split of a forest's workers over its roots: W // R + (r < W % R)
        r = torch.arange(self.n_roots, dtype=torch.int32, device=dev)
        self.even_workers = self.n_workers // self.n_roots + (r < self.n_workers % self.n_roots).int()
        self.init()

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            rc = getattr(load_library(), name)(_ptr(self.data), self.data.numel(), self.max_nodes, self.max_children,
                                               *args, C.c_void_p(stream.cuda_stream))
        if rc:
            raise ShipSimError(f"{name} failed ({rc})")

    def _arg(self, x, dtype, what):
        t = torch.as_tensor(x, dtype=dtype, device=self.device).contiguous().reshape(-1)
        if t.numel() != self.n_workers:
            raise ShipSimError(f"tree {what}: {t.numel()} entries for {self.n_workers} workers")
        return t

    def init(self):
        """The one-node tree: the root, node 0 (shipsim_tree_init); for a forest its n_roots roots
        (shipsim_tree_init_forest)."""
        if self.n_roots > 1:
            self._call("shipsim_tree_init_forest", self.n_roots)
        else:
            self._call("shipsim_tree_init")

    def select(self, max_depth, widen=(1, 1), c_explore=1.0, root_workers=None):
        """Where each of the n_workers workers starts this round (shipsim_tree_select): (leaf, expand), int32 tensors
        owned by the tree — worker w starts from node leaf[w] and creates a child there iff expand[w] == 1.
        root_workers (shipsim_tree_select_forest): n_roots int32, the workers asked for per root, served in root order
        until the n_workers are used up; where they sum to less, the trailing workers get leaf -1 (expand passes them
        through, backup skips them). A forest's default is the even split W // R + (r < W % R); a single tree without
        root_workers takes shipsim_tree_select. Only a contiguous int32 tensor of n_roots entries on the tree's device
        (or the default) keeps the class's promise of no allocation: it is passed as it is, and the caller keeps it
        alive and unchanged for as long as a captured graph reads it. Anything else (a list, a host tensor, another
        dtype) is copied to the device in this call, which allocates and cannot be captured."""
        c = float(c_explore)
        if not (c >= 0.0 and c != float("inf")):
            raise ShipSimError(f"tree select: c_explore must be finite and >= 0, not {c_explore}")
        if root_workers is None and self.n_roots == 1:
            self._call("shipsim_tree_select", self.n_workers, int(max_depth), int(widen[0]), int(widen[1]), C.c_double(c),
                       _ptr(self.workspace), self.workspace.numel(), _ptr(self.leaf), _ptr(self.expand_flag))
            return self.leaf, self.expand_flag
        if root_workers is None:
            rw = self.even_workers
        else:
            rw = torch.as_tensor(root_workers, dtype=torch.int32, device=self.device).contiguous().reshape(-1)
            if rw.numel() != self.n_roots:
                raise ShipSimError(f"tree select: {rw.numel()} entries of root_workers for {self.n_roots} roots")
        self._call("shipsim_tree_select_forest", self.n_workers, self.n_roots, _ptr(rw), int(max_depth), int(widen[0]),
                   int(widen[1]), C.c_double(c), _ptr(self.workspace), self.workspace.numel(), _ptr(self.leaf),
                   _ptr(self.expand_flag))
        self._keep_roots = rw  # (the call is asynchronous: a copy made above must outlive it)
        return self.leaf, self.expand_flag

    def expand(self, action, leaf=None, expand=None):
        """The widening workers' new nodes (shipsim_tree_expand; leaf, expand: select's, by default the last ones):
        node, an int32 tensor owned by the tree — the new id, leaf[w] for a worker that did not widen, -1 where the
        pool was full."""
        leaf = self.leaf if leaf is None else self._arg(leaf, torch.int32, "expand")
        expand = self.expand_flag if expand is None else self._arg(expand, torch.int32, "expand")
        a = self._arg(action, torch.float32, "expand")
        self._call("shipsim_tree_expand", self.n_workers, _ptr(leaf), _ptr(expand), _ptr(a), _ptr(self.workspace),
                   self.workspace.numel(), _ptr(self.node))
        self._keep = (leaf, expand, a)
        return self.node

    def backup(self, value, node=None, terminal=None):
        """visits += 1 and value_sum += round(value[w] * 2^24) from node[w] (default: the last expand's) up to the
        root (shipsim_tree_backup); terminal: optional per-worker flags, the terminal bit of node[w]."""
        node = self.node if node is None else self._arg(node, torch.int32, "backup")
        v = self._arg(value, torch.float64, "backup")
        t = None if terminal is None else self._arg(terminal, torch.uint8, "backup")
        self._call("shipsim_tree_backup", self.n_workers, _ptr(node), _ptr(v), _ptr(t))
        self._keep = (node, v, t)

    @property
    def n_nodes(self):
        """The node count (one copy to the host)."""
        return int(self.header[0].item())


def tree_select(tree, max_depth, widen=(1, 1), c_explore=1.0, root_workers=None):
    """SearchTree.select as a function: (leaf, expand)."""
    return tree.select(max_depth, widen, c_explore, root_workers)


def tree_expand(tree, action, leaf=None, expand=None):
    """SearchTree.expand as a function: node."""
    return tree.expand(action, leaf, expand)


def tree_backup(tree, value, node=None, terminal=None):
    """SearchTree.backup as a function."""
    return tree.backup(value, node, terminal)
