"""Register budget of the headline decision-stream kernels (ast_step_kernel<true, none | sbmpc, 16, false, 1 | 2, 2>):
they hold their launch constants in accumulator registers for the whole launch, so the budget is what keeps them
correct and fast — no scratch, no spilled SGPRs or VGPRs, one wave per SIMD, and the unified register file's 512.
Cross-compiles the SHIPSIM_REGCHECK=1 kernel set for gfx950 with the build's flags (ast_sac_amd/build_hash.py) to
assembly and reads the resource-usage metadata the compiler writes with each kernel; no instruction is looked at.
Needs hipcc (skipped without), no GPU."""
import os
import re
import shutil
import subprocess

import pytest

from ast_sac_amd.build_hash import HIPFLAGS, lib_flag_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# <DETAILED, COLLAV, LPE, REC, MODE, SLOTS>: table and policy streams, collav none (0) and sbmpc (2)
HEADLINE = [f"_Z15ast_step_kernelILb1ELi{ca}ELi16ELb0ELi{mode}ELi2EEv8StepArgs" for ca in (0, 2) for mode in (1, 2)]


def _hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("regbudget") / "shipsim.s"
    flags = [f for f in HIPFLAGS if f != "-shared"] + lib_flag_sets("shipsim")[0]  # object 1: every step kernel
    cmd = [cc] + flags + ["-DSHIPSIM_REGCHECK=1", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "ast_sac_amd", "csrc"),
                          os.path.join(ROOT, "ast_sac_amd", "csrc", "shipsim_kernels.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    text = out.read_text()
    rows, cur = {}, None
    for line in text.splitlines():  # the "; Kernel info:" comment block that follows each kernel's code
        m = re.match(r"(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r";\s+(TotalNumVgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|TotalNumSgprs):\s+(\d+)", line)
        if m and cur:
            rows.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    # the code object's metadata (amdhsa.kernels): spill counts per kernel
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        for key in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
            m = re.search(rf"\.{key}:\s+(\d+)", blk)
            if m:
                rows.setdefault(name.group(1), {})[key] = int(m.group(1))
    return rows


@pytest.mark.parametrize("kernel", HEADLINE)
def test_headline_stream_register_budget(usage, kernel):
    assert kernel in usage, sorted(k for k in usage if "ast_step" in k)
    u = usage[kernel]
    print(kernel, u)
    assert u["ScratchSize"] == 0 and u["private_segment_fixed_size"] == 0, u
    assert u["Occupancy"] == 1, u
    assert u["TotalNumVgprs"] <= 512, u
    assert u["sgpr_spill_count"] == 0, u
    assert u["vgpr_spill_count"] == 0, u


def test_regcheck_set_is_the_four_headline_streams(usage):
    assert sorted(k for k in usage if "ast_step_kernel" in k) == sorted(HEADLINE)
