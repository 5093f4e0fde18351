"""shipsim_create's host half (csrc/shipsim_config_host.hpp: default configs, validate, the per-ship constants, Params
and the constant block with the map grid) below the device (no GPU), under AddressSanitizer and UBSan in a
stand-alone program."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")


def test_config_half_of_create_under_asan_and_ubsan(tmp_path):
    """tests/config_host_check.cpp: the 18 default configs and five small maps on a two-ship AST config (a triangle; a
    concave polygon with a 1000 m square; exactly 64 vertices; 65 vertices, so no grid; no polygons). The block's
    layout against ConstBuf's accessors, closed edge rings and tight boxes, the grid against a brute-force distance
    and map_inside on a 5 x 5 lattice per cell, the rank-mod-8 parts, the default AST config's Params, and one broken
    config per rule of validate: all exact, on the exactly-sized heap block const_block allocates."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "config_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "config_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "config host OK: 23 configurations"
