"""The SBMPC nominal-scenario test's host half (csrc/shipsim_sbmpc_nominal.hpp), host side (no GPU): the stand-alone
program under AddressSanitizer and UBSan, and the test against the CPU oracle on requests around its decision: every
request it accepts has the oracle answer (1.0, 0.0, active), no memory value but (1, 0) is accepted, and the batch is
neither all accepted nor all refused. The batch (nominal_batch) and the host evaluation (host_flags) are shared with
tests/test_gpu_sbmpc_nominal.py."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

import oracle_ffi as O
from ast_sac_amd import shipsim_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
SEED, N = 20261, 4096
TF, DT = 1000.0, 20.0
_P = (0.4, 0.6, 0.8, 1.0)
_CHI = tuple(np.deg2rad(np.arange(-30, 31, 10)))


@functools.lru_cache(maxsize=None)
def exe():
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    out = os.path.join(tempfile.mkdtemp(prefix="sbmpc_nominal_"), "sbmpc_nominal_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "sbmpc_nominal_host_check.cpp"), "-o", out], check=True)
    return out


def host_flags(req, tf=TF, dt=DT, seg=False):
    """(flags bool (n,), ratio float64 (n,)) of sbmpc_nominal_holds on the host for (n, SBMPC_IN) requests; seg: of
    sbmpc_nominal_holds_seg, the form the streams' tick evaluates, on the course split by sbmpc_nominal_split_course"""
    req = np.asarray(req, np.float64).reshape(-1, abi.SBMPC_IN)
    text = f"{len(req)} {tf!r} {dt!r}\n" + "\n".join(" ".join(repr(float(v)) for v in r) for r in req) + "\n"
    r = subprocess.run([exe(), "eval"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.array([line.split() for line in r.stdout.strip().splitlines()], dtype=np.float64).reshape(-1, 4)
    assert len(out) == len(req)
    k = 2 if seg else 0
    return out[:, k] != 0, out[:, k + 1]


def requests(rng, n):
    """(n, SBMPC_IN) requests at the rest memory (1, 0) around the test's decision: u_d 3..9, course ±4 rad, sway ±0.5,
    obstacle length 40..140; the obstacle ship placed from the relative velocity of the two straight lines so that
    their closest approach is D (half of the rows 250..500 m, a quarter 50..250 m, a quarter 500..1500 m: the decision
    lies between 150 and 450 m for these speeds and lengths) at a distance now of R (200..2000 m, at
    least D), four fifths of the rows approaching it and the rest past it (then the distance now is the closest)."""
    u_d, chi_d = rng.uniform(3, 9, n), rng.uniform(-4, 4, n)
    os_ = np.stack([rng.uniform(0, 20000, n), rng.uniform(0, 10000, n), rng.uniform(-np.pi, np.pi, n),
                    rng.uniform(0, 6, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.01, 0.01, n)], 1)
    psi, ou, ov = rng.uniform(-np.pi, np.pi, n), rng.uniform(0, 6, n), rng.uniform(-0.5, 0.5, n)
    vs = np.stack([-np.sin(chi_d) * u_d, np.cos(chi_d) * u_d], 1)  # linear_pred after its first step
    vo = np.stack([-np.sin(psi) * ou + np.cos(psi) * ov, np.cos(psi) * ou + np.sin(psi) * ov], 1)
    w = vo - vs
    wh = w / np.linalg.norm(w, axis=1, keepdims=True)
    perp = np.stack([-wh[:, 1], wh[:, 0]], 1) * rng.choice([-1.0, 1.0], n)[:, None]
    pick = rng.uniform(size=n)
    D = np.where(pick < 0.5, rng.uniform(250, 500, n), np.where(pick < 0.75, rng.uniform(50, 250, n),
                                                                rng.uniform(500, 1500, n)))
    R = np.maximum(rng.uniform(200, 2000, n), D)
    along = np.sqrt(R * R - D * D) * np.where(rng.uniform(size=n) < 0.8, -1.0, 1.0)  # (-: the approach lies ahead)
    e0 = D[:, None] * perp + along[:, None] * wh
    ob = np.stack([os_[:, 0] + e0[:, 0], os_[:, 1] + e0[:, 1], psi, ou, ov], 1)
    last = np.stack([np.ones(n), np.zeros(n)], 1)
    return np.concatenate([last, u_d[:, None], chi_d[:, None], os_, ob, rng.uniform(40, 140, (n, 1)),
                           rng.uniform(8, 30, (n, 1))], 1)


@functools.lru_cache(maxsize=None)
def nominal_batch():
    """The tests' batch: (requests, host flags, host ratios), made once per process and read-only."""
    req = requests(np.random.Generator(np.random.PCG64(SEED)), N)
    flags, ratio = host_flags(req)
    for a in (req, flags, ratio):
        a.setflags(write=False)
    return req, flags, ratio


def oracle_one(r):
    return O.sbmpc(r[0], r[1], r[2], r[3], r[4:10], r[10:15], r[15], r[16], TF, DT)[0]


def test_host_half_under_asan_and_ubsan():
    """The gap against sbmpc_h2's 27 other scenarios, the answer's constants, the guards (memory, NaN, infinities) and
    the bound's fall with the distance, in a program built with -fsanitize=address,undefined."""
    r = subprocess.run([exe()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"sbmpc nominal host OK gap (\S+)", r.stdout)
    assert m and abs(float(m.group(1)) - 50 * np.deg2rad(10.0) ** 2) < 1e-12


def test_accepted_requests_have_the_oracle_answer_one_zero():
    req, flags, ratio = nominal_batch()
    share = flags.mean()
    print(f"\n[sbmpc nominal] {N} requests at the rest memory: {flags.sum()} accepted ({share:.3f}), ratio "
          f"{ratio.min():.3g} .. {ratio.max():.3g}, nearest to 1: {np.abs(ratio - 1).min():.3g}")
    assert 0.2 <= share <= 0.8  # (neither vacuous nor all refused)
    assert (np.abs(ratio - 1) > 1e-9).all()  # the seed: no row on the decision (the GPU test compares flags exactly)
    np.testing.assert_array_equal(flags, ratio < 1)
    d = np.hypot(req[:, 10] - req[:, 4], req[:, 11] - req[:, 5])
    assert d.min() >= 200 - 1e-6
    assert d.max() < 2000.0  # every request is inside D_INIT: the answers come from the optimisation
    for r in req[flags]:
        a = oracle_one(r)
        assert a[0] == 1.0 and a[1] == 0.0 and not np.signbit(a[1]) and a[2] == 1.0, (r, a)
    # the refused rows are not all needless: some of their oracle answers differ from (1, 0)
    refused = req[~flags][:256]
    assert any(tuple(oracle_one(r)[:2]) != (1.0, 0.0) for r in refused)


def test_the_streams_form_agrees_with_the_plain_test_on_the_batch():
    """sbmpc_nominal_holds_seg (segment sine and cosine with the correction's argument, no atan) on the split course:
    the same flags as the plain test on the whole batch, the ratios equal to rounding, none within 1e-9 of 1 (the GPU
    test compares the device's flags of this form exactly as well)."""
    _, flags, ratio = nominal_batch()
    req = nominal_batch()[0]
    sflags, sratio = host_flags(req, seg=True)
    assert (np.abs(sratio - 1) > 1e-9).all()
    np.testing.assert_array_equal(sflags, flags)
    np.testing.assert_array_equal(sflags, sratio < 1)
    assert np.abs(sratio / ratio - 1).max() < 1e-9


def test_no_other_memory_value_is_accepted():
    req, flags, _ = nominal_batch()
    far = req[flags][:64]
    assert len(far) == 64
    rows = []
    for p in _P:
        for c in _CHI:
            if (p, c) != (1.0, 0.0):
                x = far.copy()
                x[:, 0], x[:, 1] = p, c
                rows.append(x)
    assert len(rows) == 27
    got, _ = host_flags(np.concatenate(rows))
    assert not got.any()
    again, _ = host_flags(far)  # (the same rows at the rest memory are accepted)
    assert again.all()


def test_header_declares_and_binding_exports_the_entry():
    from ast_sac_amd import shipsim
    from ast_sac_amd.build_hash import SOURCES
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int\s+shipsim_sbmpc_nominal\s*\(int32_t n, double tf, double dt, const double\* in, "
                     r"int32_t\* flag_out,\s*void\* stream\)", src, re.M)
    assert "shipsim_sbmpc_nominal" in shipsim.EXPORTED_SYMBOLS and callable(shipsim.sbmpc_nominal)
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12  # additive
    assert "ast_sac_amd/csrc/shipsim_sbmpc_nominal.hpp" in SOURCES["shipsim"]
    # the header has no HIP dependency, and the optimiser's header takes the request and the own terms from it
    hdr = open(os.path.join(CSRC, "shipsim_sbmpc_nominal.hpp")).read()
    assert "hip_runtime" not in hdr and "__device__" not in hdr
    dev = open(os.path.join(CSRC, "shipsim_sbmpc.hpp")).read()
    assert '#include "shipsim_sbmpc_nominal.hpp"' in dev and "struct SbIn" not in dev
    assert not re.search(r"double\s+sbmpc_h2\s*\(", dev) and not re.search(r"double\s+p_ca_of\s*\(", dev)
