"""Weighted splitting below the device (no GPU): the header and the binding, what the calls refuse without a device,
and the resampling arithmetic (csrc/shipsim_resample_host.hpp) in a stand-alone program under AddressSanitizer and
UBSan against the Python-integer restatement tests/resample_ref.py — exact equality."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as R
from ast_sac_amd import shipsim_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
EINVAL = -1  # SHIPSIM_EINVAL
NAMES = ("shipsim_resample_workspace_bytes", "shipsim_resample", "shipsim_level_distance")
MAX_N = 1 << 22


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
    exe = str(tmp_path_factory.mktemp("resample") / "resample_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "resample_host_check.cpp"), "-o", exe], check=True)
    return exe


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def run_host(exe, w, pot, pairs):
    """The host program on one population and a list of (hi, lo) offset bits: dict(status, e, q, Q, total) and a
    list of dict(U, sorted, wsorted, inplace, winplace) per pair (weights and total as bits)."""
    text = [f"{len(w):x}", " ".join(f"{int(b):x}" for b in _bits(w)), " ".join(f"{int(b):x}" for b in _bits(pot)),
            f"{len(pairs):x}"] + [f"{hi:x} {lo:x}" for hi, lo in pairs]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    head, per = {}, []
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        vals = [int(v, 16) for v in vals]
        if name in ("status", "e", "Q", "total"):
            head[name] = vals[0]
        elif name == "q":
            head["q"] = vals
        elif name == "U":
            per.append(dict(U=vals[0]))
        else:
            per[-1][name] = np.array(vals, dtype=np.uint64)
    if head["e"] >= 1 << 31:
        head["e"] -= 1 << 32
    assert len(per) == len(pairs)
    return head, per


def test_header_declares_and_binding_exports_the_three_calls():
    from ast_sac_amd.shipsim import EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int64_t\s+shipsim_resample_workspace_bytes\s*\(int32_t\s+n\)", src, re.M)
    assert re.search(r"^int\s+shipsim_resample\s*\(int32_t\s+n,\s*const double\*\s*weight,\s*const double\*\s*potential,"
                     r"\s*uint64_t\s+seed,\s*const int64_t\*\s*counter,\s*int32_t\s+arrangement,\s*void\*\s*workspace,"
                     r"\s*int64_t\s+workspace_bytes,\s*int32_t\*\s*src_out,\s*double\*\s*weight_out,\s*double\*\s*"
                     r"total_out,\s*int32_t\*\s*status_out,\s*void\*\s*stream\)", src, re.M)
    assert re.search(r"^int\s+shipsim_level_distance\s*\(shipsim_handle\*\s*h,\s*double\*\s*out\)", src, re.M)
    for name, val in (("SORTED", "0"), ("IN_PLACE", "1"), ("MAX_N", r"\(1 << 22\)")):
        assert re.search(rf"#define\s+SHIPSIM_RESAMPLE_{name}\s+{val}", src)
    for name in NAMES:
        assert name in EXPORTED_SYMBOLS
    # additive: the ABI number did not move
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12


def test_library_exports_and_refuses_without_a_device(lib):
    assert lib.shipsim_abi_version() == 12
    for name in NAMES:
        assert hasattr(lib, name), name
    wb = lib.shipsim_resample_workspace_bytes
    assert wb.restype is C.c_int64
    for n in (0, -1, MAX_N + 1):
        assert wb(n) == EINVAL
    sizes = [wb(n) for n in (1, 2, 5, 64, 257, 1023, 1024, 1025, 4099, 65536, 1 << 20, MAX_N)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert lib.shipsim_level_distance(None, None) == EINVAL

    # host memory stands in for the device pointers: every call below is refused before a device call is made
    n = 8
    w, p = (C.c_double * n)(), (C.c_double * n)()
    ctr = (C.c_int64 * 1)()
    src, wout = (C.c_int32 * n)(), (C.c_double * n)()
    need = wb(n)
    ws = (C.c_uint8 * (need + 32))()
    base = C.addressof(ws)
    base += (-base) % 16

    def call(n_=n, w_=w, p_=p, ctr_=ctr, arr=1, ws_=base, bytes_=need, src_=src, wout_=wout):
        return lib.shipsim_resample(n_, w_, p_, 7, ctr_, arr, ws_, bytes_, src_, wout_, None, None, None)

    assert call(n_=0) == EINVAL and call(n_=-3) == EINVAL and call(n_=MAX_N + 1) == EINVAL
    for k in ("w_", "p_", "ctr_", "ws_", "src_", "wout_"):
        assert call(**{k: None}) == EINVAL, k
    assert call(arr=2) == EINVAL and call(arr=-1) == EINVAL
    assert call(bytes_=need - 1) == EINVAL and call(bytes_=0) == EINVAL
    assert call(ws_=base + 8) == EINVAL  # not 16-byte aligned


@pytest.mark.parametrize("n", [1, 2, 5, 64, 257, 4099])
def test_host_program_equals_the_python_restatement(host_program, n):
    w, pot = R.inputs(n)
    pairs = [R.offset_bits(0x1234ABCD5678EF01, ctr) for ctr in (0, 1, 2**40 + 5)] + [(2**64 - 1, 2**64 - 1), (0, 0)]
    head, per = run_host(host_program, w, pot, pairs)
    status, e, q, p = R.quantise(w, pot)
    assert (head["status"], head["e"]) == (status, e) == (0, e)
    assert head["q"] == q and head["Q"] == sum(q)
    assert all((qi >= 1) == (pi > 0) for qi, pi in zip(q, p)) and 2**39 <= max(q) <= 2**40
    for (hi, lo), got in zip(pairs, per):
        for arrangement, key in ((R.SORTED, "sorted"), (R.IN_PLACE, "inplace")):
            ref = R.resample(w, pot, hi, lo, arrangement)
            assert got["U"] == ref["U"] and head["Q"] == ref["Q"]
            np.testing.assert_array_equal(got[key].astype(np.int64), ref["src"].astype(np.int64))
            np.testing.assert_array_equal(got["w" + key], _bits(ref["weight"]))
            assert head["total"] == int(_bits([ref["total"]])[0])
        # in place: a selected env keeps its slot, and both arrangements hold the same multiset of sources
        sel, inp = got["sorted"].astype(np.int64), got["inplace"].astype(np.int64)
        kept = np.isin(np.arange(n), sel)
        np.testing.assert_array_equal(inp[kept], np.arange(n)[kept])
        np.testing.assert_array_equal(np.sort(inp), sel)
    # total mass: sum p <= total <= sum p * (1 + n * 2^-39)
    total = float(np.array([head["total"]], dtype=np.uint64).view(np.float64)[0])
    sp = math.fsum(p)
    assert sp <= total <= sp * (1 + n * 2.0**-39)


@pytest.mark.parametrize("case", ["zero", "nan", "negative", "inf"])
def test_host_program_without_usable_mass(host_program, case):
    n = 9
    w, pot = R.inputs(n)
    w = np.abs(w) + 0.1
    if case == "zero":
        pot[:] = 0.0
    elif case == "nan":
        pot[4] = np.nan
    elif case == "negative":
        pot[7] = -1.0
    else:
        pot[0] = np.inf
    head, per = run_host(host_program, w, pot, [(5, 6)])
    assert head["status"] == (1 if case == "zero" else 2) and head["total"] == 0
    for key in ("sorted", "inplace"):
        np.testing.assert_array_equal(per[0][key], np.arange(n))
        np.testing.assert_array_equal(per[0]["w" + key], _bits(w))
    assert R.resample(w, pot, 5, 6, R.IN_PLACE)["status"] == head["status"]


@pytest.mark.parametrize("n", [64, 257])
def test_mean_counts_over_1024_counters(host_program, n):
    """Every count is floor or ceil of n q_i / Q, and its mean over 1024 offsets is within 0.094 of n q_i / Q: six
    standard errors of a two-valued count (sigma <= 1/2) over 1024 draws."""
    w, pot = R.inputs(n)
    pairs = [R.offset_bits(99, ctr) for ctr in range(1024)]
    head, per = run_host(host_program, w, pot, pairs)
    q, Q = head["q"], head["Q"]
    counts = np.stack([np.bincount(g["sorted"].astype(np.int64), minlength=n) for g in per])
    lo = np.array([n * qi // Q for qi in q])
    hi = np.array([-((-n * qi) // Q) for qi in q])
    assert np.all((counts == lo) | (counts == hi))
    assert np.all(counts.sum(axis=1) == n)
    expect = np.array([n * qi / Q for qi in q])
    worst = float(np.abs(counts.mean(axis=0) - expect).max())
    print(f"n = {n}: worst |mean count - n q / Q| = {worst:.4f}")
    assert worst < 0.094
