"""The state archive below the device (no GPU): the header and the binding, what the calls refuse without a device,
and the host half (csrc/shipsim_archive_host.hpp) in a stand-alone program under AddressSanitizer and UBSan: the
two-table gather on exactly-sized heap blocks, the argument checks, and the election against the Python restatement
tests/archive_ref.py — exact equality."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import archive_ref as A
from ast_sac_amd import shipsim_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")
EINVAL = -1  # SHIPSIM_EINVAL
NAMES = ("shipsim_archive_bytes", "shipsim_archive_store", "shipsim_archive_load", "shipsim_archive_workspace_bytes",
         "shipsim_archive_elect")
MAX_CELLS = 1 << 22


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
    exe = str(tmp_path_factory.mktemp("archive") / "archive_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "archive_host_check.cpp"), "-o", exe], check=True)
    return exe


def run_host(exe, n_envs, n_cells, rounds):
    """The host program on a list of (name, cell, score) elections run one after the other: per round
    dict(env_of_cell int64, cell_score bits, cell_seen, n_improved)."""
    text = [f"{n_envs:x} {n_cells:x} {len(rounds):x}"]
    for _, cell, score in rounds:
        text.append(" ".join(f"{int(c) & 0xFFFFFFFF:x}" for c in cell))
        text.append(" ".join(f"{int(b):x}" for b in A.bits(score)))
    r = subprocess.run([exe, "elect"], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = []
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        vals = [int(v, 16) for v in vals]
        if name == "env_of_cell":
            out.append({name: np.array(vals, dtype=np.uint32).view(np.int32).astype(np.int64)})
        elif name == "n_improved":
            out[-1][name] = vals[0]
        else:
            out[-1][name] = np.array(vals, dtype=np.uint64)
    assert len(out) == len(rounds)
    return out


def test_header_declares_and_binding_exports_the_five_calls():
    from ast_sac_amd import shipsim
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    assert re.search(r"^int64_t\s+shipsim_archive_bytes\s*\(const shipsim_handle\*\s*h,\s*int32_t\s+n_cells\)", src, re.M)
    assert re.search(r"^int\s+shipsim_archive_store\s*\(shipsim_handle\*\s*h,\s*void\*\s*archive,\s*int64_t\s+bytes,\s*"
                     r"int32_t\s+n_cells,\s*const int32_t\*\s*env_of_cell\)", src, re.M)
    assert re.search(r"^int\s+shipsim_archive_load\s*\(shipsim_handle\*\s*h,\s*const void\*\s*archive,\s*int64_t\s+bytes,"
                     r"\s*int32_t\s+n_cells,\s*const int32_t\*\s*cell_of_env\)", src, re.M)
    assert re.search(r"^int64_t\s+shipsim_archive_workspace_bytes\s*\(int32_t\s+n_cells\)", src, re.M)
    assert re.search(r"^int\s+shipsim_archive_elect\s*\(int32_t\s+n_envs,\s*int32_t\s+n_cells,\s*const int32_t\*\s*cell,"
                     r"\s*const double\*\s*score,\s*double\*\s*cell_score,\s*int32_t\*\s*cell_seen,\s*void\*\s*"
                     r"workspace,\s*int64_t\s+workspace_bytes,\s*int32_t\*\s*env_of_cell_out,\s*int32_t\*\s*"
                     r"n_improved_out,\s*void\*\s*stream\)", src, re.M)
    assert re.search(r"#define\s+SHIPSIM_ARCHIVE_MAX_CELLS\s+\(1 << 22\)", src)
    assert abi.ARCHIVE_MAX_CELLS == MAX_CELLS
    for name in NAMES:
        assert name in shipsim.EXPORTED_SYMBOLS
    assert callable(shipsim.archive_elect) and hasattr(shipsim.ShipSim, "archive") and shipsim.StateArchive
    # additive: the ABI number did not move
    assert re.search(r"#define\s+SHIPSIM_ABI_VERSION\s+12\b", src) and abi.ABI_VERSION == 12


def test_library_exports_and_refuses_without_a_device(lib):
    assert lib.shipsim_abi_version() == 12
    for name in NAMES:
        assert hasattr(lib, name), name
    wb = lib.shipsim_archive_workspace_bytes
    assert wb.restype is C.c_int64 and lib.shipsim_archive_bytes.restype is C.c_int64
    for m in (0, -1, MAX_CELLS + 1):
        assert wb(m) == EINVAL
    sizes = [wb(m) for m in (1, 2, 5, 64, 255, 257, 1023, 1024, 1025, 4097, 65536, 1 << 20, MAX_CELLS)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)

    # no handle: refused
    buf = (C.c_uint8 * 64)()
    idx = (C.c_int32 * 4)()
    assert lib.shipsim_archive_bytes(None, 4) == EINVAL
    assert lib.shipsim_archive_store(None, buf, 64, 4, idx) == EINVAL
    assert lib.shipsim_archive_load(None, buf, 64, 4, idx) == EINVAL

    # host memory stands in for the device pointers: every call below is refused before a device call is made
    n, m = 8, 5
    cell, score = (C.c_int32 * n)(), (C.c_double * n)()
    cs, seen, eoc = (C.c_double * m)(), (C.c_int32 * m)(), (C.c_int32 * m)()
    need = wb(m)
    ws = (C.c_uint8 * (need + 32))()
    base = C.addressof(ws)
    base += (-base) % 16

    def call(n_=n, m_=m, cell_=cell, score_=score, cs_=cs, seen_=seen, ws_=base, bytes_=need, eoc_=eoc):
        return lib.shipsim_archive_elect(n_, m_, cell_, score_, cs_, seen_, ws_, bytes_, eoc_, None, None)

    assert call(n_=0) == EINVAL and call(n_=-3) == EINVAL and call(n_=(1 << 22) + 1) == EINVAL
    assert call(m_=0) == EINVAL and call(m_=-1) == EINVAL and call(m_=MAX_CELLS + 1) == EINVAL
    for k in ("cell_", "score_", "cs_", "ws_", "eoc_"):
        assert call(**{k: None}) == EINVAL, k
    assert call(bytes_=need - 1) == EINVAL and call(bytes_=0) == EINVAL
    assert call(ws_=base + 8) == EINVAL  # not 16-byte aligned
    assert call(m_=m + 4096) == EINVAL  # a workspace sized for fewer cells


def test_two_table_gather_and_argument_checks_under_asan_and_ubsan(host_program):
    """tests/archive_host_check.cpp gather: (n_envs, n_cells) in {(48, 7), (5, 300), (64, 64)} x 1..SHIPSIM_MAX_SHIPS
    ships. Every unit of every column lands inside its slot's bytes on both sides; a store and a load on exactly-sized
    heap blocks move every slot whole, leave out-of-range indices and the padding alone and touch nothing outside."""
    r = subprocess.run([host_program, "gather"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "archive host OK: 15 configurations, 43 columns" in r.stdout


@pytest.mark.parametrize("n_cells", A.N_CELLS)
@pytest.mark.parametrize("n_envs", [1, 64, 65, 1025])
def test_host_election_equals_the_python_restatement(host_program, n_envs, n_cells):
    rounds = A.rounds(n_envs, n_cells)
    got = run_host(host_program, n_envs, n_cells, rounds)
    cell_score, cell_seen = [A.NAN] * n_cells, [0] * n_cells
    taken = 0
    for (name, cell, score), g in zip(rounds, got):
        eoc, cell_score, cell_seen, n_improved = A.elect(cell, score, cell_score, cell_seen, n_cells)
        np.testing.assert_array_equal(g["env_of_cell"], np.array(eoc, dtype=np.int64), err_msg=name)
        np.testing.assert_array_equal(g["cell_score"], A.bits(cell_score), err_msg=name)
        np.testing.assert_array_equal(g["cell_seen"], np.array(cell_seen, dtype=np.uint64), err_msg=name)
        assert g["n_improved"] == n_improved == sum(e >= 0 for e in eoc), name
        taken += n_improved
    assert taken > 0


def test_the_restatement_on_cases_worked_by_hand():
    nan, inf = A.NAN, float("inf")
    # cell 0: envs 0 and 2 tie at 1.0, the lower wins; cell 1: -0.0 (env 1) and +0.0 (env 3) tie, env 1 wins and its
    # score is stored as given; cell 2: a NaN score is no candidate, -inf is; env 6 names no cell
    cell = [0, 1, 0, 1, 2, 2, 3, -1]
    score = [1.0, -0.0, 1.0, 0.0, nan, -inf, 5.0, 5.0]
    eoc, cs, seen, k = A.elect(cell, score, [nan, nan, nan], [0, 10, 0], 3)
    assert eoc == [0, 1, 5] and k == 3 and seen == [2, 12, 1]
    assert A.bits(cs).tolist() == A.bits([1.0, -0.0, -inf]).tolist()
    # again: equal is not strictly greater; +0.0 does not beat the stored -0.0; -inf is beaten by anything finite
    eoc, cs2, seen, k = A.elect([0, 1, 2], [1.0, 0.0, -1e308], cs, seen, 3)
    assert eoc == [-1, -1, 0 + 2] and k == 1 and seen == [3, 13, 2]
    assert A.bits(cs2).tolist() == A.bits([1.0, -0.0, -1e308]).tolist()
