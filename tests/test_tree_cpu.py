"""The search tree below the device (no GPU): the header, the binding and the layout, what the calls refuse without a
device, the two Python restatements of select against one another (tests/tree_ref.py), and the host half
(csrc/shipsim_tree_host.hpp) in a stand-alone program under AddressSanitizer and UBSan against the restatement —
exact equality, the whole tree buffer included."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tree_ref as R
from ast_sac_amd import shipsim_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
EINVAL = -1  # SHIPSIM_EINVAL
NAMES = ("shipsim_tree_bytes", "shipsim_tree_layout", "shipsim_tree_workspace_bytes", "shipsim_tree_init",
         "shipsim_tree_select", "shipsim_tree_expand", "shipsim_tree_backup")


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
    exe = str(tmp_path_factory.mktemp("tree") / "tree_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "tree_host_check.cpp"), "-o", exe], check=True)
    return exe


def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


class HostTree:
    """The host program as the three operations on plain lists: every call runs the program on the buffer so far."""

    def __init__(self, exe, tmp, T):
        self.exe, self.M, self.C = exe, T.M, T.C
        self.path = [os.path.join(str(tmp), n) for n in ("a.bin", "b.bin")]
        T.to_bytes().tofile(self.path[0])

    def _run(self, text):
        r = subprocess.run([self.exe, "run", str(self.M), str(self.C), self.path[0], self.path[1]], input=text,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        self.path.reverse()
        rows = {}
        for line in r.stdout.splitlines():
            name, *vals = line.split()
            rows[name] = np.array([int(v, 16) for v in vals], dtype=np.uint32).view(np.int32).tolist()
        return rows

    @staticmethod
    def _row(name, vals):
        return name + " " + " ".join(f"{int(v) & 0xFFFFFFFFFFFFFFFF:x}" for v in vals) + "\n"

    def select(self, W, max_depth, wnum, wden, c):
        rows = self._run(f"select {W:x} {max_depth:x} {wnum:x} {wden:x} {dbits(c):x}\n")
        return rows["leaf"], rows["expand"]

    def expand(self, leaf, flags, action):
        text = f"expand {len(leaf):x}\n" + self._row("leaf", [v & 0xFFFFFFFF for v in leaf]) + self._row("expand", flags)
        return self._run(text + self._row("action", [fbits(a) for a in action]))["node"]

    def backup(self, node, value, terminal=None):
        text = f"backup {len(node):x} {0 if terminal is None else 1:x}\n" + self._row("node", [v & 0xFFFFFFFF for v in node])
        text += self._row("value", [dbits(v) for v in value])
        if terminal is not None:
            text += self._row("terminal", terminal)
        self._run(text)

    def bytes(self):
        return np.fromfile(self.path[0], dtype=np.uint8)


def test_header_declares_and_binding_exports_the_calls():
    from ast_sac_amd import shipsim
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int64_t\s+shipsim_tree_bytes\s*\(int32_t\s+max_nodes,\s*int32_t\s+max_children\)", src, re.M)
    assert re.search(r"^int64_t\s+shipsim_tree_workspace_bytes\s*\(int32_t\s+max_nodes,\s*int32_t\s+n_workers\)", src, re.M)
    for name in NAMES:
        assert re.search(r"^int(64_t)?\s+" + name + r"\s*\(", src, re.M), name
        assert name in shipsim.EXPORTED_SYMBOLS
    for macro, value, mine in (("MAX_CHILDREN", "64", abi.TREE_MAX_CHILDREN), ("MAX_DEPTH", "32", abi.TREE_MAX_DEPTH),
                               ("MAX_WORKERS", r"\(1 << 22\)", abi.TREE_MAX_WORKERS),
                               ("SCAN_TILE", "1024", abi.TREE_SCAN_TILE)):
        assert re.search(r"#define\s+SHIPSIM_TREE_" + macro + r"\s+" + value, src), macro
        assert mine == getattr(R, macro) == eval(value.replace("\\", ""))
    assert callable(shipsim.tree_select) and callable(shipsim.tree_expand) and callable(shipsim.tree_backup)
    assert shipsim.SearchTree and shipsim.TREE_FIELDS == R.FIELDS
    # additive: the ABI number did not move
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12
    from ast_sac_amd.build_hash import OBJECTS, SOURCES
    assert "ast_sac_amd/csrc/shipsim_tree.hip" in SOURCES["shipsim"]
    assert "ast_sac_amd/csrc/shipsim_tree_host.hpp" in SOURCES["shipsim"]
    assert OBJECTS["shipsim"][0][0].endswith("shipsim_kernels.hip") and OBJECTS["shipsim"][4] == ("ast_sac_amd/csrc/shipsim_tree.hip", [])


def test_layout_of_library_and_restatement_agree(lib):
    from ast_sac_amd import shipsim
    assert lib.shipsim_tree_bytes.restype is C.c_int64 and lib.shipsim_tree_workspace_bytes.restype is C.c_int64
    for M, Cc in ((1, 1), (5, 3), (200, 64), (1025, 3), (1 << 16, 16), (R.MAX_NODES, 64)):
        want = R.layout(M, Cc)
        assert shipsim.tree_layout(M, Cc) == want
        assert lib.shipsim_tree_bytes(M, Cc) == want["bytes"]
    for M, Cc in ((0, 1), (-1, 1), (R.MAX_NODES + 1, 1), (1, 0), (1, 65)):
        assert lib.shipsim_tree_bytes(M, Cc) == EINVAL
        out = (C.c_int64 * 10)()
        assert lib.shipsim_tree_layout(M, Cc, out) == EINVAL
    assert lib.shipsim_tree_layout(4, 4, None) == EINVAL
    wb = lib.shipsim_tree_workspace_bytes
    for M, W in ((0, 1), (1, 0), (R.MAX_NODES + 1, 1), (1, R.MAX_WORKERS + 1), (-5, 5)):
        assert wb(M, W) == EINVAL
    sizes = (1, 2, 63, 64, 65, 1023, 1025, 4097, 1 << 16, 1 << 20, 1 << 22)
    grid = [[wb(m, w) for w in sizes] for m in sizes]
    assert all(v > 0 for row in grid for v in row)
    assert all(row == sorted(row) for row in grid) and all(list(col) == sorted(col) for col in zip(*grid))


def test_library_refuses_without_a_device(lib):
    # host memory stands in for the device pointers: every call below is refused before a device call is made
    M, Cc, W = 5, 3, 8
    tb, need = lib.shipsim_tree_bytes(M, Cc), lib.shipsim_tree_workspace_bytes(M, W)
    raw = (C.c_uint8 * (tb + need + 64))()
    tree = C.addressof(raw)
    tree += (-tree) % 16
    ws = tree + tb + (-tb) % 16
    i32, f32, f64 = (C.c_int32 * W)(), (C.c_float * W)(), (C.c_double * W)()
    nan, inf = float("nan"), float("inf")

    def sel(tree_=tree, tb_=tb, M_=M, C_=Cc, W_=W, d_=9, wn_=1, wd_=1, c_=1.0, ws_=ws, wb_=need, leaf_=i32, exp_=i32):
        return lib.shipsim_tree_select(tree_, tb_, M_, C_, W_, d_, wn_, wd_, C.c_double(c_), ws_, wb_, leaf_, exp_, None)

    def exp(tree_=tree, tb_=tb, M_=M, C_=Cc, W_=W, leaf_=i32, exp_=i32, act_=f32, ws_=ws, wb_=need, out_=i32):
        return lib.shipsim_tree_expand(tree_, tb_, M_, C_, W_, leaf_, exp_, act_, ws_, wb_, out_, None)

    def bak(tree_=tree, tb_=tb, M_=M, C_=Cc, W_=W, node_=i32, val_=f64):
        return lib.shipsim_tree_backup(tree_, tb_, M_, C_, W_, node_, val_, None, None)

    for call in (sel, exp, bak):
        assert call(tree_=None) == EINVAL and call(tree_=tree + 8) == EINVAL
        assert call(tb_=tb - 1) == EINVAL and call(tb_=tb + 256) == EINVAL
        assert call(M_=0) == EINVAL and call(M_=R.MAX_NODES + 1) == EINVAL and call(M_=M + 100) == EINVAL  # (another size of buffer)
        assert call(C_=0) == EINVAL and call(C_=65) == EINVAL
        assert call(W_=0) == EINVAL and call(W_=-1) == EINVAL and call(W_=R.MAX_WORKERS + 1) == EINVAL
    for call in (sel, exp):
        assert call(ws_=None) == EINVAL and call(ws_=ws + 8) == EINVAL
        assert call(wb_=need - 1) == EINVAL and call(wb_=0) == EINVAL
        assert call(W_=W + 4096) == EINVAL  # a workspace sized for fewer workers
    for k in ("leaf_", "exp_"):
        assert sel(**{k: None}) == EINVAL
    for k in ("leaf_", "exp_", "act_", "out_"):
        assert exp(**{k: None}) == EINVAL
    for k in ("node_", "val_"):
        assert bak(**{k: None}) == EINVAL
    assert sel(d_=-1) == EINVAL and sel(d_=33) == EINVAL
    assert sel(wn_=0) == EINVAL and sel(wn_=(1 << 15) + 1) == EINVAL and sel(wd_=0) == EINVAL and sel(wd_=(1 << 15) + 1) == EINVAL
    assert sel(c_=-1.0) == EINVAL and sel(c_=nan) == EINVAL and sel(c_=inf) == EINVAL and sel(c_=-inf) == EINVAL
    assert lib.shipsim_tree_init(None, tb, M, Cc, None) == EINVAL and lib.shipsim_tree_init(tree, tb - 1, M, Cc, None) == EINVAL
    assert lib.shipsim_tree_init(tree + 4, tb, M, Cc, None) == EINVAL


def test_the_restatement_on_cases_worked_by_hand():
    # k = 1: the root's first worker widens (0 < sqrt 1), the second finds one child being made and 1 < sqrt 2
    T = R.Tree(8, 3)
    assert R.select(T, 1, 9, 1, 1, 1.0) == ([0], [1])
    assert R.select(T, 4, 9, 1, 1, 1.0) == ([0, 0, 0, 0], [0, 0, 1, 1])  # m = 2 at N + 1 = 3, 4: they stay
    a = T.add(0, visits=2, value_sum=3 << 24)   # Q = 1.5
    b = T.add(0, visits=2, value_sum=-1 << 24)  # Q = -0.5
    T.visits[0] = 4
    # c = 0: pure exploitation; the root (m = 2, N + 1 = 5: 4 < 5) widens once, then 3 children is C
    leaf, flags = R.select(T, 3, 1, 1, 1, 0.0)
    assert (leaf, flags) == ([0, a, a], [1, 0, 0])  # depth(a) == max_depth: they stay at a
    # a tie goes to the lower slot, then the virtual visit moves the next worker on
    T.value_sum[b] = 3 << 24
    T.n_children[0], T.visits[0] = 2, 2  # (4 < 3, 4 < 4: no worker widens)
    leaf, flags = R.select(T, 2, 1, 1, 1, 1.0)
    assert sorted(leaf) == [a, b] and flags == [0, 0]
    # a terminal root keeps everybody
    T.flags[0] = 1
    assert R.select(T, 5, 9, 1, 1, 1.0) == ([0] * 5, [0] * 5)
    # expand: ids in worker order, slots in worker order, the pool full by one
    T = R.Tree(3, 4)
    assert R.expand(T, [0, 0, 0], [1, 1, 1], [0.5, -0.5, 0.25]) == [1, 2, -1]
    assert T.n_nodes == 3 and T.dropped == 1 and T.child[0][:2] == [1, 2] and T.n_children[0] == 2 and T.depth[2] == 1
    # backup: the whole path, the skipped ones, the terminal bit
    R.backup(T, [2, 2, -1, 1, 0], [1.0, -0.25, 1.0, math.inf, 2.0], [0, 1, 1, 1, 0])
    assert T.visits[:3] == [3, 0, 2] and T.skipped == 2 and T.flags[:3] == [0, 0, 1]
    assert T.value_sum[:3] == [int(2.75 * (1 << 24)), 0, int(0.75 * (1 << 24))]
    assert R.quantize(1e300) == 1 << 40 and R.quantize(-1e308 * 10) == -(1 << 40) and R.quantize(3 / (1 << 25)) == 2


@pytest.mark.parametrize("seed", range(6))
def test_the_two_restatements_of_select_agree_on_random_trees(seed):
    Cc = (1, 3, 64, 5, 2, 8)[seed]
    T = R.random_tree(seed, 200, Cc, n_nodes=(1, 30, 120, 200, 60, 150)[seed], big=seed % 2 == 1)
    for W in (1, 63, 65, 300):
        for wnum, wden, c in ((1, 1, 1.0), (4, 1, 0.0), (1, 9, 0.37), (100, 3, 5.0)):
            a = R.select(T, W, 6, wnum, wden, c)
            assert a == R.select_literal(T, W, 6, wnum, wden, c)
            assert len(a[0]) == W and a[0] == sorted(a[0])


def test_host_half_hand_cases_under_asan_and_ubsan(host_program):
    r = subprocess.run([host_program, "hand"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tree host OK" in r.stdout


@pytest.mark.parametrize("seed,Cc,n,W", [(0, 1, 1, 5), (1, 3, 40, 65), (2, 64, 200, 300), (3, 5, R.SCAN_TILE + 1, 64)])
def test_host_select_equals_the_restatement_on_random_trees(host_program, tmp_path, seed, Cc, n, W):
    T = R.random_tree(seed, max(n, 2), Cc, n_nodes=n, big=True, max_depth=8)
    H = HostTree(host_program, tmp_path, T)
    for max_depth, wnum, wden, c in ((8, 1, 1, 1.0), (3, 7, 2, 0.0), (8, 1, 50, 0.25)):
        assert H.select(W, max_depth, wnum, wden, c) == R.select(T, W, max_depth, wnum, wden, c)
    np.testing.assert_array_equal(H.bytes(), T.to_bytes())  # select writes nothing


@pytest.mark.parametrize("M,Cc,W,drops", [(24, 2, 7, True), (300, 3, 65, False), (150, 64, 64, True)])
def test_host_rounds_equal_the_restatement_buffer_and_all(host_program, tmp_path, M, Cc, W, drops):
    """Rounds of select -> expand -> backup until the pool overflows: outputs and the whole buffer, bit for bit."""
    T = R.Tree(M, Cc)
    H = HostTree(host_program, tmp_path, T)
    want = R.play_rounds(T, W, 8, 5, 3, 1, 25.0)
    got = R.play_rounds(None, W, 8, 5, 3, 1, 25.0, ops=(H.select, H.expand, H.backup))
    assert got == want
    np.testing.assert_array_equal(H.bytes(), T.to_bytes())
    assert T.skipped > 0 and (T.dropped > 0) == drops and (T.n_nodes == M) == drops
