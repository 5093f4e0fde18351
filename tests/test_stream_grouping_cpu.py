"""The stream grouping's host half (csrc/shipsim_grouping_host.hpp), host side (no GPU): the header and the binding,
the key and the reference ordering against a Python sort on random clocks with ties, and the stand-alone program
under AddressSanitizer and UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("grouping") / "grouping_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "grouping_host_check.cpp"), "-o", out], check=True)
    return out


def test_grouping_host_half_under_asan_and_ubsan(exe):
    """Which launches group, the buffer's size, the key's edge cases, and rank by counting (the device kernel's
    method) against the reference ordering, in a program built with -fsanitize=address,undefined."""
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grouping host OK" in r.stdout


@pytest.mark.parametrize("n,dt,max_ticks", [(1, 4.0, 10), (61, 4.0, 3), (4096, 4.0, 1400), (1000, 0.5, 40),
                                            (257, 0.1, 100000)])
def test_reference_ordering_equals_a_python_stable_sort(exe, n, dt, max_ticks):
    """Clocks as the kernels form them (k additions of dt from 0), many of them equal: the key is k, and the
    ordering is numpy's stable argsort of the keys (ascending key, ties by env index)."""
    g = np.random.Generator(np.random.PCG64(n))
    ticks = g.integers(0, max_ticks + 1, n)
    if max_ticks <= 1400:
        clock = np.zeros(n)
        for k in range(int(ticks.max())):
            clock = np.where(ticks > k, clock + dt, clock)
    else:  # (too many additions to replay: the product instead of the sum)
        clock = ticks * dt
    text = f"{n} {dt!r}\n" + " ".join(repr(float(t)) for t in clock) + "\n"
    r = subprocess.run([exe, "order"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    keys, order = (np.array(line.split(), dtype=np.int64) for line in r.stdout.strip().splitlines())
    np.testing.assert_array_equal(keys, ticks)
    np.testing.assert_array_equal(keys, np.rint(clock / dt).astype(np.int64))  # (what the GPU test restates)
    np.testing.assert_array_equal(order, np.argsort(ticks, kind="stable"))
    assert sorted(order.tolist()) == list(range(n))


def test_header_declares_and_binding_exports_the_grouping_calls():
    from ast_sac_amd import shipsim_abi as abi
    from ast_sac_amd.shipsim import EXPORTED_SYMBOLS, ShipSim
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    for name in ("shipsim_set_stream_grouping", "shipsim_get_stream_grouping"):
        assert re.search(r"^int\s+" + name + r"\s*\(shipsim_handle\*", src, re.M), name
        assert name in EXPORTED_SYMBOLS
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12  # additive
    assert callable(ShipSim.set_stream_grouping) and callable(ShipSim.get_stream_grouping)


def test_library_refuses_grouping_calls_without_a_handle():
    import ctypes as C
    from ast_sac_amd import shipsim
    if not os.path.exists(shipsim.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    lib = shipsim.load_library()
    a = (C.c_int32 * 4)()
    assert lib.shipsim_set_stream_grouping(None, 1) == -1
    assert lib.shipsim_get_stream_grouping(None, a) == -1


def test_the_step_kernel_takes_its_env_from_the_slot_in_one_place():
    """ast_step_kernel derives its env once; the stream order is read there and nowhere else, and only the host
    half's header decides whether a launch groups."""
    src = open(os.path.join(CSRC, "shipsim_kernels.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert len(re.findall(r"A0\.slot_env\[", code)) == 1
    assert len(re.findall(r"blockIdx\.x \* epw", code)) == 1
    assert code.count("grouping_host::groups(") == 1
    from ast_sac_amd.build_hash import SOURCES
    assert "ast_sac_amd/csrc/shipsim_grouping_host.hpp" in SOURCES["shipsim"]
