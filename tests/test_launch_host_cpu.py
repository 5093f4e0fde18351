"""The list of step kernels and the choice among them (csrc/shipsim_launch_host.hpp), host side (no GPU): a
stand-alone program under AddressSanitizer and UBSan walks every handle at every entry point."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ast_sac_amd", "csrc")


def test_every_selection_is_a_listed_kernel_and_every_listed_kernel_is_selected(tmp_path):
    """tests/launch_host_check.cpp: machinery x collav x 2..SHIPSIM_MAX_SHIPS ships x lanes per env {2, 4, 8, 16} x
    recording x weather x entry point. Every selection that is not refused is a row of the list, every one of the
    102 rows is selected by some input, the refused inputs are K > 1 with simplified machinery or collav simple,
    weather with simplified machinery, collav simple or recording, and streams with recording, and the pinned
    cases hold (a stream at 2 lanes runs at 4, a recording step at 16 with REC, weather at 4 lanes at 8, K > 1 at
    16 lanes in 4 or 8 slots, the launch tail for streams of two-ship envs only)."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "launch_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "launch_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "launch host OK: 102 rows" in r.stdout


def test_step_kernels_are_named_in_the_list_expansion_only():
    """shipsim_kernels.hip names an ast_step_kernel instantiation once, in the expansion of the list; the launchers
    and dispatch macros the table replaced are gone."""
    src = open(os.path.join(CSRC, "shipsim_kernels.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert len(re.findall(r"ast_step_kernel\s*<", code)) == 1
    assert code.count("SHIPSIM_STEP_KERNELS(") == 1
    for gone in ("launch_step", "launch_multi", "launch_weather", "weather_lpe"):
        assert gone not in code, gone
    for macro in ("L", "LM", "LW", "LAUNCH", "CHAINED_L", "CHAINED"):
        assert not re.search(r"#define\s+%s\(" % macro, code), macro
