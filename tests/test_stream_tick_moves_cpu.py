"""Register moves on the tick loop of the headline decision-stream kernels (ast_step_kernel<true, none | sbmpc, 16,
false, 1 | 2, 2>). The loop is tested at its bottom (shipsim_kernels.hip, TICK_LOOP_ON): with the test in the header
the register allocator carried the whole loop-carried state to a second register set in the header block and back in
front of the going region, runs of 61, 61 and 32 pure moves per wave-tick in the sbmpc table stream (56, 50 and 33
in the collav-none one; 67, 37 and 74 in the sbmpc policy stream). This cross-compiles the SHIPSIM_REGCHECK=1 kernel
set for gfx950 with the build's flags to assembly, as tests/test_stream_reg_budget_cpu.py does, and reads the runs
with scripts/tick_moves.py: pure moves (vector register to vector register, or to / from an accumulator register).
  - the two table streams: no run of 24 or more anywhere inside a loop (the parent: 61 and 56; this build: 16 and
    10). Every loop depth counts, not only depth 2 and deeper: the compiler numbers the bottom-tested tick loop of the
    collav-none kernel as part of the enclosing for (;;), depth 1;
  - the two policy streams: the same bound inside their tick loop (the parent: 74 and 65; this build: 22 and 10).
    The tick loop is picked among the kernel's loops of depth 2 by scripts/tick_moves.py tick_loop(): of the two large
    ones, the one with the larger share of fp64 instructions (about 40 % against under 20 %). The other is the
    chaining code's burst loop (records, in-place resets, the policy's f32 layers), which keeps runs of 53 to 77 that
    run once per completed decision, not per tick (profiles/tick_waits.md); they are printed.
Needs hipcc (skipped without), no GPU."""
import importlib.util
import os
import shutil
import subprocess

import pytest

from ast_sac_amd.build_hash import HIPFLAGS, lib_flag_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_RUN = 24
# <DETAILED, COLLAV, LPE, REC, MODE, SLOTS>: MODE 1 the table stream, 2 the policy stream; collav none (0), sbmpc (2)
TABLE = [f"_Z15ast_step_kernelILb1ELi{ca}ELi16ELb0ELi1ELi2EEv8StepArgs" for ca in (0, 2)]
POLICY = [f"_Z15ast_step_kernelILb1ELi{ca}ELi16ELb0ELi2ELi2EEv8StepArgs" for ca in (0, 2)]


def _tick_moves():
    spec = importlib.util.spec_from_file_location("tick_moves", os.path.join(ROOT, "scripts", "tick_moves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if cc is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("tickmoves") / "shipsim.s"
    flags = [f for f in HIPFLAGS if f != "-shared"] + lib_flag_sets("shipsim")[0]  # object 1: every step kernel
    cmd = [cc] + flags + ["-DSHIPSIM_REGCHECK=1", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "ast_sac_amd", "csrc"),
                          os.path.join(ROOT, "ast_sac_amd", "csrc", "shipsim_kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out.read_text()


def _scan(listing, kernel):
    tm = _tick_moves()
    runs, loops = tm.scan(listing, kernel, min_depth=1)
    assert runs and loops, kernel  # the kernel has loops and moves in them: the listing's loop comments were read
    top = sorted(runs, key=lambda r: -r["n"])[:4]
    print(kernel, "runs of pure moves inside loops:", len(runs), "largest:",
          [(r["block"], r["n"]) for r in top], "inverse pairs:",
          [(runs[i]["block"], runs[j]["block"], hit) for i, j, hit, _ in tm.inverse_pairs(runs, MAX_RUN)])
    largest = {h: max((r["n"] for r in runs if r["loop2"] == h), default=0) for h in loops}
    for h, c in loops.items():
        if c["instructions"] >= 1000:
            print("  loop", h, c, "largest run", largest[h], "(the tick loop)" if h == tm.tick_loop(loops) else "")
    return top[0]["n"], largest, loops, tm.tick_loop(loops)


@pytest.mark.parametrize("kernel", TABLE)
def test_table_stream_tick_loop_has_no_long_move_run(listing, kernel):
    assert _scan(listing, kernel)[0] < MAX_RUN


@pytest.mark.parametrize("kernel", POLICY)
def test_policy_stream_tick_loop_has_no_long_move_run(listing, kernel):
    _, largest, loops, tick = _scan(listing, kernel)
    big = [h for h, c in loops.items() if c["instructions"] >= 1000]
    assert len(big) == 2 and tick in big, (big, tick)  # the tick loop and the chaining code's
    share = {h: loops[h]["f64"] / loops[h]["instructions"] for h in big}
    other = next(h for h in big if h != tick)
    assert share[tick] > 1.5 * share[other], share  # (the pick is not a near tie)
    assert largest[tick] < MAX_RUN, largest


def test_run_finder_on_a_synthetic_listing():
    """The run finder itself: depth from the loop comments, literals and scalar sources are no pure moves, a label
    ends a run, two other instructions inside one do not, and the inverse pair is flagged."""
    tm = _tick_moves()
    text = "\n".join([
        "k_main:",
        "\tv_mov_b32_e32 v1, v2",                                  # depth 0: not counted
        ".LBB0_1:                                ; =>This Loop Header: Depth=1",
        "\tv_mov_b32_e32 v1, v2",                                  # depth 1: not counted
        ".LBB0_2:                                ;   Parent Loop BB0_1 Depth=1",
        "                                        ; =>  This Inner Loop Header: Depth=2",
        "\tv_mov_b64_e32 v[30:31], v[42:43]",
        "\tv_accvgpr_write_b32 a42, v52",
        "\tv_mov_b32_e32 v74, 0",                                  # a literal: other instruction 1
        "\tother_op vcc, 0, v161",                                # other instruction 2 (a placeholder)
        "\tv_mov_b32_e32 v5, v6",
        "\tv_mov_b32_e32 v7, s3",                                  # a scalar source: no pure move (other 1)
        "\tother_op v[8:9], v[8:9], v[10:11]",
        "\tother_op v[8:9], v[8:9], v[10:11]",
        "\tother_op v[8:9], v[8:9], v[10:11]",                     # (other 3: the run has ended)
        "\tv_mov_b32_e32 v11, v12",
        ".LBB0_3:                                ;   in Loop: Header=BB0_2 Depth=2",
        "\tv_mov_b64_e32 v[42:43], v[30:31]",
        "\tv_accvgpr_read_b32 v52, a42",
        "\tv_mov_b32_e32 v6, v5",
        ".Lfunc_end0:",
    ])
    runs = tm.move_runs(text, "k_main", min_depth=2)
    assert [r["n"] for r in runs] == [3, 1, 3]
    assert runs[0]["pairs"] == {(("v", 30), ("v", 42)), (("v", 31), ("v", 43)), (("a", 42), ("v", 52)), (("v", 5), ("v", 6))}
    assert [(i, j) for i, j, _, _ in tm.inverse_pairs(runs, min_run=3)] == [(0, 2), (2, 0)]
    assert [r["n"] for r in tm.move_runs(text, "k_main", min_depth=1)][0] == 1
