"""Snapshot / restore / fork below the device (no GPU): the header and the binding, the calls without a handle, and
the state block's column table (csrc/shipsim_state_host.hpp) with the gather's arithmetic under AddressSanitizer and
UBSan in a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

from ast_sac_amd import shipsim_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
EINVAL = -1  # SHIPSIM_EINVAL
NAMES = ("shipsim_state_bytes", "shipsim_snapshot", "shipsim_restore", "shipsim_fork")


def test_header_declares_and_binding_exports_the_four_calls():
    from ast_sac_amd.shipsim import EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int64_t\s+shipsim_state_bytes\s*\(const shipsim_handle\*", src, re.M)
    assert re.search(r"^int\s+shipsim_snapshot\s*\(shipsim_handle\*\s*h,\s*void\*\s*dst,\s*int64_t\s+bytes\)", src, re.M)
    assert re.search(r"^int\s+shipsim_restore\s*\(shipsim_handle\*\s*h,\s*const void\*\s*src,\s*int64_t\s+bytes\)", src,
                     re.M)
    assert re.search(r"^int\s+shipsim_fork\s*\(shipsim_handle\*\s*h,\s*const void\*\s*from,\s*int64_t\s+bytes,\s*"
                     r"const int32_t\*\s*src_env\)", src, re.M)
    for name in NAMES:
        assert name in EXPORTED_SYMBOLS
    # additive: the ABI number did not move
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12


def test_library_refuses_the_calls_without_a_handle():
    from ast_sac_amd import shipsim
    if not os.path.exists(shipsim.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    lib = shipsim.load_library()
    assert lib.shipsim_abi_version() == 12
    buf = (C.c_uint8 * 64)()
    idx = (C.c_int32 * 4)()
    assert lib.shipsim_state_bytes.restype is C.c_int64
    assert lib.shipsim_state_bytes(None) == EINVAL
    assert lib.shipsim_snapshot(None, buf, 64) == EINVAL
    assert lib.shipsim_restore(None, buf, 64) == EINVAL
    assert lib.shipsim_fork(None, buf, 64, idx) == EINVAL
    assert lib.shipsim_fork(None, None, 64, None) == EINVAL


def test_column_table_and_gather_arithmetic_under_asan_and_ubsan(tmp_path):
    """tests/state_host_check.cpp: n_envs in {1, 5, 64} x 1..SHIPSIM_MAX_SHIPS ships. The columns are disjoint, inside
    the block, within their 256-byte strides and cover every ship, route and env array exactly once; the gather's
    arithmetic, run on exactly-sized heap blocks, moves every env whole, leaves out-of-range envs and the padding
    alone and touches nothing outside the block."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "state_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "state_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "state host OK: 15 configurations, 43 columns" in r.stdout
