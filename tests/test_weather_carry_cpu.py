"""Per-env weather that moves on the device, below the device (no GPU): the header, the binding and the build lists,
what the calls refuse without a handle, and the host half (csrc/shipsim_weather_host.hpp) in a stand-alone program
under AddressSanitizer and UBSan — sizes, offsets, every refusal reason, and the gather against the numpy
restatement tests/weather_carry_ref.py, bit for bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import weather_carry_ref as R
from ast_sac_amd import shipsim_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
EINVAL = -1  # SHIPSIM_EINVAL
NAMES = ("shipsim_weather_bytes", "shipsim_weather_store", "shipsim_weather_load", "shipsim_weather_fork")


@pytest.fixture(scope="module")
def lib():
    from ast_sac_amd import shipsim
    if not os.path.exists(shipsim.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    return shipsim.load_library()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("weather_carry") / "weather_carry_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "weather_carry_host_check.cpp"), "-o", exe], check=True)
    return exe


def test_header_binding_and_build_lists():
    from ast_sac_amd import shipsim
    from ast_sac_amd.build_hash import OBJECTS, SOURCES
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int64_t\s+shipsim_weather_bytes\s*\(int32_t\s+n_slots\)", src, re.M)
    for name in NAMES:
        assert re.search(r"^int(64_t)?\s+" + name + r"\s*\(", src, re.M), name
        assert name in shipsim.EXPORTED_SYMBOLS
    # additive: the ABI number did not move
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12
    assert "ast_sac_amd/csrc/shipsim_weather.hip" in SOURCES["shipsim"]
    assert "ast_sac_amd/csrc/shipsim_weather_host.hpp" in SOURCES["shipsim"]
    assert ("ast_sac_amd/csrc/shipsim_weather.hip", []) in OBJECTS["shipsim"]
    assert abi.WEATHER_ROWS == R.ROWS == 6
    assert (abi.WEATHER_ROW_WIND_SPEED, abi.WEATHER_ROW_WIND_DIRECTION, abi.WEATHER_ROW_CURRENT_NORTH,
            abi.WEATHER_ROW_CURRENT_EAST) == R.KEY_ROWS
    assert (abi.WEATHER_ROW_WIND_SIN, abi.WEATHER_ROW_WIND_COS) == (1, 2)
    host = open(os.path.join(CSRC, "shipsim_weather_host.hpp")).read()
    assert re.search(r"constexpr int kCols = 5;", host) and re.search(r"constexpr int kStoreRows = 6;", host)
    assert re.search(r"constexpr int kDirection = 5;", host)
    snap = shipsim.Snapshot(None, 1, 4, 2, "b")
    assert snap.weather is None and "weather" in shipsim.Snapshot.__slots__


def test_library_sizes_and_refusals_without_a_handle(lib):
    import ctypes as C
    assert lib.shipsim_weather_bytes.restype is C.c_int64
    for n in (1, 5, 7, 300, 1000, 65536, abi.ARCHIVE_MAX_CELLS):
        assert lib.shipsim_weather_bytes(n) == 6 * 8 * n
    for n in (0, -1, abi.ARCHIVE_MAX_CELLS + 1, R.INT32_MIN, R.INT32_MAX):
        assert lib.shipsim_weather_bytes(n) == EINVAL
    a = (C.c_double * 8)()
    assert lib.shipsim_weather_store(None, a, 48, 1, None) == EINVAL
    assert lib.shipsim_weather_load(None, a, 48, 1, None) == EINVAL
    assert lib.shipsim_weather_fork(None, None) == EINVAL


def test_the_modes_of_the_batched_env_are_refused_before_any_device_call():
    from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv
    with pytest.raises(ValueError, match="'keep', 'follow' or 'carry'"):
        BatchedMultiShipRLEnv.fork(None, [0], weather="drift")


def test_sizes_offsets_and_refusal_reasons_under_asan_and_ubsan(host_program):
    r = subprocess.run([host_program, "self"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "weather carry host OK" in r.stdout


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).reshape(-1)


def run_host(exe, cases):
    """The host program on a list of (src table, dst table, index, own): the destination tables after the gather."""
    text = []
    for src, dst, idx, own in cases:
        text.append(f"{dst.shape[1]:x} {src.shape[1]:x} {int(own):x}")
        text.append(" ".join(f"{int(i) & 0xFFFFFFFF:x}" for i in idx))
        text.append(" ".join(f"{int(b):x}" for b in np.concatenate([_bits(src), _bits(dst)])))
    r = subprocess.run([exe, "gather"], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return [np.array([int(v, 16) for v in line.split()], dtype=np.uint64).view(np.float64).reshape(R.ROWS, -1)
            for line in lines]


def _tables(n_dst, n_src):
    src = R.table(R.random_weather(n_src, 11 + n_src))
    dst = R.table(R.random_weather(n_dst, 5000 + n_dst))
    return src, dst


@pytest.mark.parametrize("n_dst,n_src", [(300, 300), (5, 5), (7, 300), (1000, 300), (300, 7), (1, 1), (1, 300)])
def test_host_gather_equals_the_numpy_restatement(host_program, n_dst, n_src):
    """Store (n_src envs into n_dst slots), load (the other way round) and the square case, over every index set:
    permutations, broadcasts, a cycle, duplicates, and -1, n_src, INT32_MIN, INT32_MAX among and instead of them."""
    src, dst = _tables(n_dst, n_src)
    sets = R.index_sets(n_dst, n_src)
    assert {"cycle", "broadcast_first", "duplicates", "out_of_range", "none_served"} <= set(sets)
    bad = sets["out_of_range"]
    assert {-1, n_src, R.INT32_MIN, R.INT32_MAX} & set(bad.tolist()) and ((bad < 0) | (bad >= n_src)).any()
    names = sorted(sets)
    got = run_host(host_program, [(src, dst, sets[k], False) for k in names])
    for k, g in zip(names, got):
        want = R.gather(src, sets[k], dst)
        assert g.tobytes() == want.tobytes(), k
    assert got[names.index("none_served")].tobytes() == dst.tobytes()
    assert got[names.index("broadcast_first")].tobytes() == np.repeat(src[:, :1], n_dst, axis=1).tobytes()


@pytest.mark.parametrize("n", [300, 5, 1])
def test_host_fork_through_staging_equals_the_in_place_restatement(host_program, n):
    """The in-place fork gathers into a staging table (own: a slot whose index names no env takes its own) that is
    then copied back: whatever the staging table held, the result is the table gathered from itself as it was."""
    tab, stale = _tables(n, n)
    sets = R.index_sets(n, n)
    names = sorted(sets)
    got = run_host(host_program, [(tab, stale, sets[k], True) for k in names])
    for k, g in zip(names, got):
        assert g.tobytes() == R.fork(tab, sets[k]).tobytes(), k
    if n > 1:  # the case staging is for: a reversal read from the table while it is being written would not be one
        assert got[names.index("reversed")].tobytes() == tab[:, ::-1].tobytes()
