"""The forest below the device (no GPU): the header and the binding, what shipsim_tree_init_forest / _select_forest
refuse without a device, the prefix rule by hand, the two Python restatements of select over a forest against one
another (tests/forest_ref.py), its decomposition into the trees under the roots (tests/tree_ref.py), and the additions
to the host half (csrc/shipsim_tree_host.hpp) in a stand-alone program under AddressSanitizer and UBSan against the
restatement — exact equality, the whole tree buffer included."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import forest_ref as F
import tree_ref as R
from ast_sac_amd import shipsim_abi as abi
from test_tree_cpu import HostTree, dbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
EINVAL = -1  # SHIPSIM_EINVAL
PARAMS = ((6, 1, 1, 1.0), (6, 4, 1, 0.0), (3, 1, 9, 0.37), (6, 100, 3, 5.0))  # max_depth, wnum, wden, c_explore


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
    exe = str(tmp_path_factory.mktemp("forest") / "forest_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "forest_host_check.cpp"), "-o", exe], check=True)
    return exe


class HostForest(HostTree):
    """The host program as the three operations of a forest round on plain lists (expand and backup: HostTree's)."""

    def select(self, W, root_workers, max_depth, wnum, wden, c):
        text = f"select_forest {W:x} {len(root_workers):x} {max_depth:x} {wnum:x} {wden:x} {dbits(c):x}\n"
        rows = self._run(text + self._row("roots", [v & 0xFFFFFFFF for v in root_workers]))
        return rows["leaf"], rows["expand"]


def patterns(W, n_roots):
    """root_workers that sum to W, to less and to more, with zeros, a negative entry and an entry above W."""
    even = F.even_split(W, n_roots)
    out = [even, [0] * (n_roots - 1) + [W], [c if r % 2 == 0 else 0 for r, c in enumerate(even)],
           [c // 2 for c in even], [c + 1 for c in even], [-3] + even[1:], [W + 5] + even[1:],
           even[:-1] + [(1 << 31) - 1]]
    return out


# ---- 1. the header and the binding ---------------------------------------------------------------------------------
def test_header_declares_and_binding_exports_the_forest_calls():
    from ast_sac_amd import shipsim
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int\s+shipsim_tree_init_forest\s*\(void\*\s+tree,\s*int64_t\s+tree_bytes,\s*int32_t\s+max_nodes,"
                     r"\s*int32_t\s+max_children,\s*int32_t\s+n_roots,\s*void\*\s+stream\)", src, re.M)
    assert re.search(r"^int\s+shipsim_tree_select_forest\s*\(const void\*\s+tree,\s*int64_t\s+tree_bytes,\s*int32_t\s+max_nodes,"
                     r"\s*int32_t\s+max_children,\s*int32_t\s+n_workers,\s*int32_t\s+n_roots,\s*const int32_t\*\s+root_workers,"
                     r"\s*int32_t\s+max_depth,\s*int32_t\s+wnum,\s*int32_t\s+wden,\s*double\s+c_explore,\s*void\*\s+workspace,"
                     r"\s*int64_t\s+workspace_bytes,\s*int32_t\*\s+leaf_out,\s*int32_t\*\s+expand_out,\s*void\*\s+stream\)", src, re.M)
    for name in ("shipsim_tree_init_forest", "shipsim_tree_select_forest"):
        assert name in shipsim.EXPORTED_SYMBOLS
    assert re.search(r"hdr\[3\]\s*=\s*n_roots", src)  # the header's fourth int is documented
    host = open(os.path.join(CSRC, "shipsim_tree_host.hpp")).read()
    assert re.search(r"kHdrRoots\s*=\s*3\b", host) and abi.TREE_HDR_ROOTS == F.HDR_ROOTS == 3
    # additive: the ABI number did not move, and the library is linked from the same objects
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12
    from ast_sac_amd.build_hash import OBJECTS
    assert OBJECTS["shipsim"] == [("ast_sac_amd/csrc/shipsim_kernels.hip", ["-mllvm", "-disable-machine-licm"]),
                                  ("ast_sac_amd/csrc/shipsim_c2_pipe.hip", []),
                                  ("ast_sac_amd/csrc/shipsim_resample.hip", []),
                                  ("ast_sac_amd/csrc/shipsim_archive.hip", []),
                                  ("ast_sac_amd/csrc/shipsim_tree.hip", []),
                                  ("ast_sac_amd/csrc/shipsim_weather.hip", [])]
    import inspect
    assert "n_roots" in inspect.signature(shipsim.SearchTree.__init__).parameters
    assert "root_workers" in inspect.signature(shipsim.SearchTree.select).parameters
    assert "root_workers" in inspect.signature(shipsim.tree_select).parameters


# ---- 2. refusals ---------------------------------------------------------------------------------------------------
def test_library_refuses_forest_calls_without_a_device(lib):
    # host memory stands in for the device pointers: every call below is refused before a device call is made
    M, Cc, W = 5, 3, 8
    tb, need = lib.shipsim_tree_bytes(M, Cc), lib.shipsim_tree_workspace_bytes(M, W)
    raw = (C.c_uint8 * (tb + need + 64))()
    tree = C.addressof(raw)
    tree += (-tree) % 16
    ws = tree + tb + (-tb) % 16
    i32 = (C.c_int32 * W)()
    nan, inf = float("nan"), float("inf")

    def sel(tree_=tree, tb_=tb, M_=M, C_=Cc, W_=W, R_=2, rw_=i32, d_=9, wn_=1, wd_=1, c_=1.0, ws_=ws, wb_=need, leaf_=i32,
            exp_=i32):
        return lib.shipsim_tree_select_forest(tree_, tb_, M_, C_, W_, R_, rw_, d_, wn_, wd_, C.c_double(c_), ws_, wb_,
                                              leaf_, exp_, None)

    def ini(tree_=tree, tb_=tb, M_=M, C_=Cc, R_=2):
        return lib.shipsim_tree_init_forest(tree_, tb_, M_, C_, R_, None)

    for R_ in (0, -1, M + 1):
        assert sel(R_=R_) == EINVAL and ini(R_=R_) == EINVAL
    assert sel(W_=3, R_=4) == EINVAL  # n_workers + 1 roots: level 0 holds a root per worker at the most
    assert sel(W_=1, R_=2) == EINVAL
    assert sel(rw_=None) == EINVAL
    for call in (sel, ini):
        assert call(tree_=None) == EINVAL and call(tree_=tree + 8) == EINVAL
        assert call(tb_=tb - 1) == EINVAL and call(tb_=tb + 256) == EINVAL
        assert call(M_=0) == EINVAL and call(M_=R.MAX_NODES + 1) == EINVAL and call(M_=M + 100) == EINVAL
        assert call(C_=0) == EINVAL and call(C_=65) == EINVAL
    # every refusal of select
    assert sel(W_=0) == EINVAL and sel(W_=-1) == EINVAL and sel(W_=R.MAX_WORKERS + 1) == EINVAL
    assert sel(ws_=None) == EINVAL and sel(ws_=ws + 8) == EINVAL
    assert sel(wb_=need - 1) == EINVAL and sel(wb_=0) == EINVAL
    assert sel(W_=W + 4096) == EINVAL  # a workspace sized for fewer workers
    assert sel(leaf_=None) == EINVAL and sel(exp_=None) == EINVAL
    assert sel(d_=-1) == EINVAL and sel(d_=33) == EINVAL
    assert sel(wn_=0) == EINVAL and sel(wn_=(1 << 15) + 1) == EINVAL and sel(wd_=0) == EINVAL and sel(wd_=(1 << 15) + 1) == EINVAL
    assert sel(c_=-1.0) == EINVAL and sel(c_=nan) == EINVAL and sel(c_=inf) == EINVAL and sel(c_=-inf) == EINVAL


# ---- 3. the prefix rule --------------------------------------------------------------------------------------------
def test_root_arrivals_by_hand():
    assert F.root_arrivals([3, 3, 3], 7) == [3, 3, 1]
    assert F.root_arrivals([3, -2, 3, 3], 7) == [3, 0, 3, 1]  # a negative entry asks for nothing
    assert F.root_arrivals([2, 100, 5], 7) == [2, 5, 0]       # an entry above W takes what is left
    assert F.root_arrivals([0, 0, 0, 0], 7) == [0, 0, 0, 0]
    assert F.root_arrivals([1, 2, 0, 1], 7) == [1, 2, 0, 1]   # a sum below W: three workers are left over
    W = 1 << 22
    got = F.root_arrivals([W] * 4096, W)                      # a plain int32 sum of these overflows
    assert got == [W] + [0] * 4095
    for W, c in ((7, [5, 1, 1, 1]), (300, F.even_split(300, 7)), (65, [70, 2])):
        a = F.root_arrivals(c, W)
        assert sum(a) == min(W, sum(c)) and all(0 <= x <= y for x, y in zip(a, c))


def test_init_forest_of_the_restatement():
    T = F.init_forest(9, 2, 4)
    assert T.n_nodes == T.n_roots == 4 and T.parent[:5] == [-1, -1, -1, -1, 0] and T.depth[:4] == [0] * 4
    hdr = T.to_bytes()[:16].view(np.int32).tolist()
    assert hdr == [4, 0, 0, 4]
    assert R.Tree(9, 2).to_bytes()[:16].view(np.int32).tolist() == [1, 0, 0, 0]  # (tree_ref is as it was)


# ---- 4. the two restatements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_the_two_restatements_of_select_forest_agree_on_random_forests(seed):
    Cc = (1, 3, 64, 5, 2, 8)[seed]
    n_roots = (1, 2, 5, 7, 30, 3)[seed]
    T = F.random_forest(seed, 200, Cc, n_roots, n_nodes=(1, 30, 120, 200, 60, 150)[seed], big=seed % 2 == 1)
    for W in (n_roots, 63, 65, 300):
        if W < n_roots:
            continue
        for rw in patterns(W, n_roots):
            for p in PARAMS:
                a = F.select_forest(T, W, rw, *p)
                assert a == F.select_forest_literal(T, W, rw, *p)
                served = sum(F.root_arrivals(rw, W))
                assert len(a[0]) == W and a[0][:served] == sorted(a[0][:served]) and a[0][served:] == [-1] * (W - served)
                assert all(v >= 0 for v in a[0][:served]) and a[1][served:] == [0] * (W - served)


# ---- 5. decomposition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_a_forest_select_is_the_select_of_each_tree_under_its_root(seed):
    Cc, n_roots = (3, 64, 5, 2)[seed], (4, 3, 7, 9)[seed]
    T = F.random_forest(40 + seed, 200, Cc, n_roots, n_nodes=(90, 200, 150, 120)[seed], big=True)
    W = 130
    for rw in patterns(W, n_roots):
        arr = F.root_arrivals(rw, W)
        for p in PARAMS:
            leaf, flags = F.select_forest(T, W, rw, *p)
            for r in range(n_roots):
                if arr[r] == 0:
                    assert all(F.root_of(T, v) != r for v in leaf if v >= 0)
                    continue
                S, ids = F.extract(T, r)
                want_leaf, want_flags = R.select(S, arr[r], *p)
                mine = [(v, f) for v, f in zip(leaf, flags) if v >= 0 and F.root_of(T, v) == r]
                assert [v for v, _ in mine] == [ids[v] for v in want_leaf] and [f for _, f in mine] == want_flags


# ---- 6. one root ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_a_one_root_forest_with_all_workers_is_select(seed):
    T = R.random_tree(seed, 200, (3, 64, 5)[seed], n_nodes=(30, 200, 150)[seed], big=True)
    T.n_roots = 1  # (what a forest of one root is: the tree)
    for W in (1, 65, 300):
        for p in PARAMS:
            assert F.select_forest(T, W, [W], *p) == R.select(T, W, *p) == F.select_forest(T, W, [W + 9], *p)


# ---- 7. the host half under the sanitizers -------------------------------------------------------------------------
def test_host_forest_hand_cases_under_asan_and_ubsan(host_program):
    r = subprocess.run([host_program, "hand"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "forest host OK" in r.stdout


@pytest.mark.parametrize("M,Cc,n_roots", [(1, 1, 1), (9, 2, 4), (1100, 3, 1025), (65, 64, 65)])
def test_host_init_forest_equals_the_restatement(host_program, tmp_path, M, Cc, n_roots):
    out = str(tmp_path / "init.bin")
    r = subprocess.run([host_program, "init", str(M), str(Cc), str(n_roots), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    np.testing.assert_array_equal(np.fromfile(out, dtype=np.uint8), F.init_forest(M, Cc, n_roots).to_bytes())


@pytest.mark.parametrize("seed,Cc,n_roots,n,W", [(0, 1, 1, 1, 5), (1, 3, 5, 40, 65), (2, 64, 64, 200, 300),
                                                 (3, 5, 1025, R.SCAN_TILE + 40, 1100)])
def test_host_select_forest_equals_the_restatement_on_random_forests(host_program, tmp_path, seed, Cc, n_roots, n, W):
    T = F.random_forest(seed, max(n, 2), Cc, n_roots, n_nodes=n, big=True, max_depth=8)
    H = HostForest(host_program, tmp_path, T)
    for rw in patterns(W, n_roots)[:: (1 if n_roots < 1000 else 3)]:
        for max_depth, wnum, wden, c in ((8, 1, 1, 1.0), (3, 7, 2, 0.0), (8, 1, 50, 0.25)):
            assert H.select(W, rw, max_depth, wnum, wden, c) == F.select_forest(T, W, rw, max_depth, wnum, wden, c)
    np.testing.assert_array_equal(H.bytes(), T.to_bytes())  # select writes nothing


@pytest.mark.parametrize("M,Cc,W,n_roots", [(4096, 3, 300, 7), (700, 64, 65, 65)])
def test_host_forest_rounds_equal_the_restatement_buffer_and_all(host_program, tmp_path, M, Cc, W, n_roots):
    """Twenty rounds of select_forest -> expand -> backup: outputs and the whole buffer, bit for bit; the second
    shape runs the pool full."""
    T = F.init_forest(M, Cc, n_roots)
    H = HostForest(host_program, tmp_path, T)
    rw = F.even_split(W, n_roots)
    want = F.play_rounds(T, W, rw, 20, 6, 3, 1, 25.0)
    got = F.play_rounds(None, W, rw, 20, 6, 3, 1, 25.0, ops=(H.select, H.expand, H.backup))
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"round {r}"
    np.testing.assert_array_equal(H.bytes(), T.to_bytes())
    assert T.n_nodes > 300 and T.skipped > 0 and (T.dropped > 0) == (M == 700) and (T.n_nodes == M) == (M == 700)
    for r in range(n_roots):
        assert T.visits[r] > 0 and T.parent[r] == -1
