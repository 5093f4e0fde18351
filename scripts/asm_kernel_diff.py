"""Per-kernel comparison of two device assembly files (hipcc --cuda-device-only -S of the same object before and after
a change that must not alter the device code). Kernels are matched by symbol, so their order in the file may differ.
Compared per kernel: its text from its section directive (`.section .text.<name>`; `.text` for a kernel that is no
template) to the end of its `.amdhsa_kernel` block, and its entry in the `amdhsa.kernels` metadata. Lines naming the
`__hip_cuid_*` symbol are ignored (it hashes the source path), and local labels are compared without the number of
their function in the file.
Usage: python scripts/asm_kernel_diff.py BEFORE.s AFTER.s   (exit status 1 if anything differs)"""
import re
import sys


def kernels(path):
    lines = [l for l in open(path).read().split("\n") if "__hip_cuid_" not in l]
    # (local labels carry the function's number in the file, .LBB<function>_<block>: a kernel added in front of
    # others renumbers theirs without changing their code)
    lines = [re.sub(r"[ \t]+;", " ;", re.sub(r"\bL?BB\d+_(\d+)", r"BB_\1", l)) for l in lines]  # (and comment padding)
    text, meta = {}, {}
    begin = re.compile(r"\s*\.protected\s+(\S+)\s*; -- Begin function")
    for i, l in enumerate(lines):
        m = begin.match(l)
        if not m:
            continue
        j = i + 1  # to the end of the kernel descriptor (a device function kept out of line has none)
        while j < len(lines) and not lines[j].strip().startswith(".end_amdhsa_kernel") and not begin.match(lines[j]):
            j += 1
        if j < len(lines) and lines[j].strip().startswith(".end_amdhsa_kernel"):
            text[m.group(1)] = lines[i - 1:j + 1]  # from its section directive (.section .text.<name>, or .text)
    # amdhsa.kernels: a YAML list, one "  - " item per kernel
    start = next((k for k, l in enumerate(lines) if l.strip() == "amdhsa.kernels:"), None)
    if start is not None:
        item = []
        for l in lines[start + 1:] + ["x"]:
            if l.startswith("  - ") or not l.startswith("  "):
                if item:
                    # (the kernel's own .name sits at the item's indent; its arguments' names are nested deeper)
                    meta[next(m.group(1) for m in (re.match(r"    \.name:\s+(\S+)", x) for x in item) if m)] = item
                item = [l] if l.startswith("  - ") else []
                if not l.startswith("  "):
                    break
            else:
                item.append(l)
    return text, meta


def main():
    (ta, ma), (tb, mb) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for what, a, b in (("text", ta, tb), ("metadata", ma, mb)):
        if set(a) != set(b):
            bad += 1
            print(f"{what}: kernel names differ: only before {sorted(set(a) - set(b))}, only after {sorted(set(b) - set(a))}")
        differ = [n for n in a if n in b and a[n] != b[n]]
        bad += len(differ)
        for n in differ:
            k = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
            print(f"{what} differs: {n} at its line {k}")
    step = sum("ast_step_kernel" in n for n in ta)
    print(f"{len(ta)} kernels ({step} ast_step_kernel), {len(ma)} metadata entries: {bad} differ")
    sys.exit(1 if bad or not ta or len(ta) != len(ma) else 0)


if __name__ == "__main__":
    main()
