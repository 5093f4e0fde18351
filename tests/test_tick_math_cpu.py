"""The tick math's host form (csrc/shipsim_tickmath.hpp), host side (no GPU): the stand-alone program, compiled
-ffp-contract=off under AddressSanitizer and UBSan (table indexing, the range predicate of tm_sincos, special values,
a sweep against libm), and the host form bit for bit against the device library's recorded results
(tests/golden/tickmath_device.npz: a few thousand arguments per function with the library's result bits, recorded on
the GPU by shipsim_tickmath_eval; tests/test_gpu_tick_math.py checks the file against the device)."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tickmath_device.npz")
_FN = {"sincos": 0, "atan": 1, "exp": 2}


@functools.lru_cache(maxsize=None)
def exe():
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    out = os.path.join(tempfile.mkdtemp(prefix="tickmath_"), "tickmath_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "tickmath_host_check.cpp"), "-o", out], check=True)
    return out


def host_bits(fn, xbits):
    """(n, 2) uint64 result patterns of the host form for uint64 argument patterns (sincos rows outside the small
    range: 0, 0)"""
    text = f"{_FN[fn]} {len(xbits)}\n" + "\n".join(f"{int(v):016x}" for v in xbits) + "\n"
    r = subprocess.run([exe(), "eval"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.array([[int(w, 16) for w in line.split()] for line in r.stdout.strip().splitlines()], dtype=np.uint64)
    assert out.shape == (len(xbits), 2)
    return out


def test_host_form_under_asan_and_ubsan():
    r = subprocess.run([exe()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"tickmath host OK worst (\S+) ulp", r.stdout)
    assert m and float(m.group(1)) <= 2.0


@pytest.mark.parametrize("fn", ["sincos", "atan", "exp"])
def test_host_form_is_the_device_librarys_bits(fn):
    z = np.load(GOLDEN)
    x, lib = z[fn + "_x"], z[fn + "_lib"].reshape(len(z[fn + "_x"]), -1)
    assert 2000 <= len(x) <= 8000 and lib.shape[1] == (2 if fn == "sincos" else 1)
    got = host_bits(fn, x)[:, :lib.shape[1]]
    xv = x.view(np.float64)
    use = np.abs(xv) < 2.0 ** 30 if fn == "sincos" else np.ones(len(x), bool)  # (NaN: False)
    nan = np.isnan(lib.view(np.float64)).any(1)
    assert use.sum() >= 1500 and (~use).sum() >= (50 if fn == "sincos" else 0)
    cmp = use & ~nan
    diff = (got[cmp] != lib[cmp]).any(1)
    print(f"\n[tick math host {fn}] {int(diff.sum())} differing of {int(cmp.sum())} rows ({int(nan.sum())} NaN rows)")
    assert not diff.any(), [(hex(int(a)), [hex(int(v)) for v in g], [hex(int(v)) for v in w])
                            for a, g, w in zip(x[cmp][diff][:5], got[cmp][diff][:5], lib[cmp][diff][:5])]
    assert np.isnan(got.view(np.float64)[use & nan]).all()  # where the library returns NaN the host form does
    if fn == "sincos":  # outside the small range the caller uses the library: the program evaluates nothing there
        assert (got[~use] == 0).all()


def test_header_declares_and_binding_exports_the_entry():
    from ast_sac_amd import shipsim, shipsim_abi as abi
    from ast_sac_amd.build_hash import SOURCES
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int\s+shipsim_tickmath_eval\s*\(int32_t fn, int32_t n, const double\* in, double\* out,\s*"
                     r"void\* stream\)", src, re.M)
    assert "shipsim_tickmath_eval" in shipsim.EXPORTED_SYMBOLS and callable(shipsim.tickmath_eval)
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12  # additive
    assert "ast_sac_amd/csrc/shipsim_tickmath.hpp" in SOURCES["shipsim"]
    hdr = open(os.path.join(CSRC, "shipsim_tickmath.hpp")).read()
    assert "hip_runtime" not in hdr and "__device__" not in hdr and "ROCm 7.2.0" in hdr
    assert '#include "shipsim_tickmath.hpp"' in open(os.path.join(CSRC, "shipsim_device.hpp")).read()
