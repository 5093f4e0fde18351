"""Control-flow bookkeeping of one ast_step_kernel instantiation's tick loop, by source line: from a device assembly
file compiled with line tables (hipcc --save-temps -gline-tables-only, the flags of scripts/isa_kernel.sh), the
exec-mask saves / restores, the branches and the register-to-register VGPR copies attributed to the `.loc` they carry.
    python scripts/tick_conditionals.py FILE.s MANGLED_PREFIX FIRST_LINE LAST_LINE [KERNEL_FIRST_LINE]
FIRST_LINE / LAST_LINE: the tick loop's lines in shipsim_kernels.hip (the `while (__any(going))` line and the loop's
closing brace); instructions between the first and the last instruction attributed to that range are counted,
whichever file their own line is in (helpers inlined into the loop), except the SBMPC pass's interior
(shipsim_sbmpc.hpp past its helpers). Static counts: what a steady-state tick executes of them is read off the
listing by hand (profiles/tick_waits.md)."""
import collections
import re
import sys


def main():
    path, prefix, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    L = open(path).read().split("\n")
    st = next(i for i, l in enumerate(L) if l.startswith(prefix) and ":" in l)
    en = next(i for i in range(st, len(L)) if L[i].startswith(".Lfunc_end"))
    files = {}
    for l in L:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
    ins, loc = [], ("?", 0)
    for l in L[st:en]:
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
        elif l.startswith("\t") and not l.strip().startswith((".", ";")):
            ins.append((l.strip(), loc))
    inloop = [i for i, (_, (f, n)) in enumerate(ins) if f == "shipsim_kernels.hip" and lo <= n <= hi]
    span = ins[inloop[0]:inloop[-1] + 1]
    # the pass's interior: from its first to its last instruction (code laid out in one piece), and the kernel's own
    # lines outside the loop that the block layout put between the loop's (the chaining code: KERNEL_FIRST_LINE..lo)
    sb = [i for i, (_, (f, n)) in enumerate(span) if f == "shipsim_sbmpc.hpp" and n > 120]
    kfirst = int(sys.argv[5]) if len(sys.argv) > 5 else lo
    body = [x for i, x in enumerate(span) if not (sb and sb[0] <= i <= sb[-1])
            and not (x[1][0] == "shipsim_kernels.hip" and (kfirst <= x[1][1] < lo or x[1][1] > hi))]
    cls = collections.OrderedDict(
        saveexec=lambda s: "saveexec" in s,
        exec_op=lambda s: re.match(r"s_(or|and|andn2|xor|mov|not|orn2|andn1)\w*_b64 .*exec", s) and "saveexec" not in s,
        branch=lambda s: s.startswith(("s_cbranch", "s_branch")),
        vcopy=lambda s: re.match(r"v_mov_b(32|64)(_e32)? v\[?[\d:]+\]?, v", s),
        cvt_f32_f64=lambda s: s.startswith("v_cvt_f32_f64"),
        fp64=lambda s: re.match(r"v_\w+_f64", s) and not s.startswith("v_cvt"),
        dpp=lambda s: "dpp" in s or "row_" in s or "quad_perm" in s,
    )
    tot = collections.Counter()
    per = collections.defaultdict(collections.Counter)
    for s, at in body:
        for k, f in cls.items():
            if f(s):
                tot[k] += 1
                if k in ("saveexec", "exec_op", "branch", "vcopy"):
                    per[at][k] += 1
    blocks = sum(1 for l in L[st:en] if re.match(r"\.LBB\d+_\d+:", l))
    print(f"{len(body)} instructions in the tick loop outside the pass ({blocks} basic blocks in the kernel)")
    print("  ".join(f"{k} {tot[k]}" for k in cls))
    print("\nby source line (saveexec / exec_op / branch / vcopy):")
    for at in sorted(per):
        c = per[at]
        if c["saveexec"] or c["branch"] or c["exec_op"] or c["vcopy"] >= 3:
            print(f"  {at[0]}:{at[1]:<5d} {c['saveexec']:3d} {c['exec_op']:3d} {c['branch']:3d} {c['vcopy']:3d}")


if __name__ == "__main__":
    main()
