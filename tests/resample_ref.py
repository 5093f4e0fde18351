"""shipsim_resample restated in Python integers (include/shipsim.h: the arithmetic of the resampling call), with the
inputs the resampling tests share. Nothing here touches the library or the device."""
import bisect
import math
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_HEADER = os.path.join(ROOT, "ast_sac_amd", "csrc", "shipsim_resample_host.hpp")
SORTED, IN_PLACE = 0, 1
TAG = 0x52455341
SHIFT = 40


def tile():
    """The scan tile T as the header states it."""
    return int(re.search(r"constexpr int kTile = (\d+);", open(HOST_HEADER).read()).group(1))


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on one counter block (tests/test_gpu_run_policy.py's, on scalars)."""
    return [int(x) for x in philox_words(c0, c1, c2, c3, k0, k1)]


def philox_words(c0, c1, c2, c3, k0, k1):
    """The same rounds on numpy uint64 words: scalars, or arrays of counter blocks under one key."""
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & m32, p1 & m32, n2 & m32, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c


def offset_bits(seed, counter):
    """(hi, lo): the 128 bits the offset is reduced from."""
    seed, counter = int(seed) & (2**64 - 1), int(counter) & (2**64 - 1)
    c = philox(counter & 0xFFFFFFFF, counter >> 32, TAG, 0, seed & 0xFFFFFFFF, seed >> 32)
    return c[0] | (c[1] << 32), c[2] | (c[3] << 32)


def quantise(weight, potential):
    """status, e, q (list of Python ints), p (float64 array)."""
    w = np.asarray(weight, np.float64)
    p = w * np.asarray(potential, np.float64)
    if np.any(~np.isfinite(p) | (p < 0)):
        return 2, 0, None, p
    m = float(p.max())
    if m == 0:
        return 1, 0, None, p
    _, e = math.frexp(m)
    q = [int(x) for x in np.ceil(np.ldexp(p, SHIFT - e))]
    return 0, e, q, p


def resample(weight, potential, hi, lo, arrangement):
    """dict(status, src, weight, total, q, Q, U, sel, e) for the 128 offset bits (hi, lo)."""
    w = np.asarray(weight, np.float64)
    n = len(w)
    status, e, q, _ = quantise(w, potential)
    if status:
        return dict(status=status, src=np.arange(n, dtype=np.int32), weight=w.copy(), total=0.0, q=None, Q=0, U=0)
    C = []
    acc = 0
    for x in q:
        acc += x
        C.append(acc)
    Q = acc
    assert Q <= 2**62
    U = ((hi << 64) | lo) % Q
    s, r = divmod(Q, n)
    t = [j * s + (j * r + U) // n for j in range(n)]
    assert n > 4096 or all(t[j] == (j * Q + U) // n for j in range(n))
    sel = np.array([bisect.bisect_right(C, x) for x in t], dtype=np.int64)
    if arrangement == SORTED:
        src = sel
    else:
        c = np.bincount(sel, minlength=n)
        src = np.arange(n)
        src[np.where(c == 0)[0]] = np.repeat(np.arange(n), np.maximum(c - 1, 0))
    qa = np.array(q, dtype=np.uint64)
    wout = w[src] * (np.float64(Q) / (np.float64(n) * qa[src].astype(np.float64)))
    return dict(status=0, src=src.astype(np.int32), weight=wout, total=float(np.ldexp(np.float64(Q), e - SHIFT)), q=q,
                Q=Q, U=U, sel=sel, e=e)


def inputs(n, seed=0):
    """The shared inputs: weights with a fifth zeroed, potentials exp(-30 u)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    w = rng.random(n) + 0.05
    w[rng.random(n) < 0.2] = 0.0
    if not w.any():
        w[0] = 0.5
    pot = np.exp(-30.0 * rng.random(n))
    return w, pot
