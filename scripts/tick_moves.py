"""Runs of pure register moves inside a kernel's loops, from a compiler listing (hipcc --save-temps or -S).

The register allocator splits the live ranges of loop-carried state at block boundaries; where it does so on the
steady path of the stream tick loop the copies are issued every tick ("The tick loop, bottom-tested").
This prints every run of consecutive pure moves in code the compiler's loop comments place at depth >= MIN_DEPTH
(the tick loop of a chained stream kernel is depth 2: for (;;) { tick loop; chaining code }), and flags pairs of
runs in which one run's moves are the inverses of the other's (state carried to a second register set and back).

A pure move: v_mov_b32 / v_mov_b64 from vector registers to vector registers (no literal, no scalar source, no
modifier), or v_accvgpr_read / _write / _mov. A label or a branch ends a run; a fall-through block comment does
not, nor do up to GAP (2) consecutive other instructions among the moves; a run's length counts its moves only.

Usage: python scripts/tick_moves.py LISTING.s KERNEL_PREFIX [--min-run 8] [--min-depth 2] [--gap 2]
  e.g. the headline stream of a -DSHIPSIM_REGCHECK=1 listing: _Z15ast_step_kernelILb1ELi2ELi16ELb0ELi1ELi2EE
"""
import argparse
import re

_REG = r"([va])(?:(\d+)|\[(\d+):(\d+)\])"
_MOVE = re.compile(rf"^\s+(v_mov_b32|v_mov_b64|v_accvgpr_read_b32|v_accvgpr_write_b32|v_accvgpr_mov_b32)(?:_e32|_e64)?\s+{_REG},\s*(\S+)\s*(?:;.*)?$")
_SRC = re.compile(rf"^{_REG}$")
_LABEL = re.compile(r"^([.\w$]+):")
_DEPTH = re.compile(r"(?:in Loop: Header=\w+|This (?:Inner )?Loop Header:)\s+Depth=(\d+)")
_IN_LOOP = re.compile(r"in Loop: Header=(\w+) Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (\w+) Depth=(\d+)")


def _regs(m, g):
    """The 32-bit registers of a matched operand (groups g .. g + 3): ('v', 30), ('v', 31)."""
    bank, one, lo, hi = m.group(g), m.group(g + 1), m.group(g + 2), m.group(g + 3)
    if one is not None:
        return [(bank, int(one))]
    return [(bank, r) for r in range(int(lo), int(hi) + 1)]


def pure_move(line):
    """[(dst, src), ...] per 32-bit register if the line is a pure move, else None."""
    m = _MOVE.match(line)
    if not m:
        return None
    s = _SRC.match(m.group(6))
    if not s:
        return None  # a literal, an SGPR, or a source with a modifier
    dst, src = _regs(m, 2), _regs(s, 1)
    if len(dst) != len(src):
        return None
    return list(zip(dst, src))


def kernel_lines(text, prefix):
    """(line number, line) of the first kernel whose symbol starts with prefix."""
    lines = text.split("\n")
    st = next((i for i, l in enumerate(lines) if l.startswith(prefix) and ":" in l), None)
    if st is None:
        raise KeyError(prefix)
    en = next(i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [(i + 1, lines[i]) for i in range(st, en)]


def _name(label):
    """A block label as the loop comments spell it: .LBB12_358 -> BB12_358."""
    return label[2:] if label.startswith(".L") else label


def scan(text, prefix, min_depth=2, gap=2):
    """One walk over the kernel's listing. Returns (runs, loops).
    runs: every run of pure moves at loop depth >= min_depth, as dicts with line, block, depth, loop2 (the header of
    the enclosing loop of depth 2, "" outside one), n (move instructions), kinds (per mnemonic) and pairs (the 32-bit
    dst <- src set). Up to `gap` consecutive other instructions inside a run do not end it (the scheduler drops a
    compare or a wait into the allocator's copies); a label or a branch does.
    loops: {header of a loop of depth 2: {"instructions": n, "f64": n}} over the code inside it, inner loops
    included."""
    runs, cur = [], None
    loops = {}
    skipped = 0
    outer = {}  # loop header -> its enclosing loop of depth 2 (itself, if it is one)
    loop2 = ""
    block, depth = "", 0
    pending_label = False

    def close():
        nonlocal cur
        if cur is not None:
            runs.append(cur)
        cur = None

    for no, line in kernel_lines(text, prefix):
        lab = _LABEL.match(line)
        bb = line.startswith("; %bb.")
        if lab or bb:
            if lab:
                close()
                block = lab.group(1)
            else:
                block = line.split(":")[0][2:]
            d = _DEPTH.search(line)
            depth = int(d.group(1)) if d else 0
            pending_label = d is None  # the header's depth may follow on continuation comment lines
            inl, par = _IN_LOOP.search(line), _PARENT.search(line)
            loop2 = outer.get(inl.group(1), inl.group(1) if inl.group(2) == "2" else "") if inl else ""
            if par and par.group(2) == "2":
                loop2 = par.group(1)
            continue
        if line.lstrip().startswith(";"):
            if pending_label:
                par = _PARENT.search(line)
                if par and par.group(2) == "2":
                    loop2 = par.group(1)
                d = _DEPTH.search(line)
                if d:
                    depth = int(d.group(1))
                    if depth == 2:
                        loop2 = _name(block)
                    if depth >= 2:
                        outer[_name(block)] = loop2
            continue
        if not line.startswith("\t") or line.strip().startswith("."):
            continue
        pending_label = False
        if depth >= 2 and loop2:
            c = loops.setdefault(loop2, {"instructions": 0, "f64": 0})
            c["instructions"] += 1
            c["f64"] += "_f64" in line.split()[0]
        mv = pure_move(line) if depth >= min_depth else None
        if mv is None:
            skipped += 1
            if skipped > gap or line.split()[0].startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
                close()
            continue
        skipped = 0
        if cur is None:
            cur = {"line": no, "block": block, "depth": depth, "loop2": loop2, "n": 0, "kinds": {}, "pairs": set()}
        cur["n"] += 1
        op = line.split()[0].replace("_e32", "").replace("_e64", "")
        cur["kinds"][op] = cur["kinds"].get(op, 0) + 1
        cur["pairs"].update(mv)
    close()
    return runs, loops


def move_runs(text, prefix, min_depth=2, gap=2):
    """The runs of scan()."""
    return scan(text, prefix, min_depth, gap)[0]


def tick_loop(loops, min_instructions=1000):
    """The header of the tick loop among a chained kernel's loops of depth 2 (scan()'s second result): of the loops
    of at least `min_instructions` instructions, the one with the largest share of fp64 instructions. The tick is
    fp64 dynamics (about 40 % of its instructions); the other large loop, the chaining code's, holds the decision
    record, the in-place reset and, in the policy kernels, the policy's f32 layers (under 20 %). None if the compiler
    numbered no such loop at depth 2."""
    big = {h: c for h, c in loops.items() if c["instructions"] >= min_instructions}
    return max(big, key=lambda h: big[h]["f64"] / big[h]["instructions"]) if big else None


def inverse_pairs(runs, min_run=8, share=0.5):
    """(i, j, matched, of): run j undoes run i — `matched` of its `of` 32-bit moves are inverses of moves of run i."""
    out = []
    big = [k for k, r in enumerate(runs) if r["n"] >= min_run]
    for i in big:
        inv = {(s, d) for d, s in runs[i]["pairs"]}
        for j in big:
            if j == i:
                continue
            hit = len(runs[j]["pairs"] & inv)
            if hit >= share * len(runs[j]["pairs"]):
                out.append((i, j, hit, len(runs[j]["pairs"])))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("listing")
    ap.add_argument("prefix")
    ap.add_argument("--min-run", type=int, default=8, help="shortest run printed (default 8)")
    ap.add_argument("--min-depth", type=int, default=2, help="loop depth from which code is considered (default 2)")
    ap.add_argument("--gap", type=int, default=2, help="other instructions in a row that do not end a run (default 2)")
    a = ap.parse_args()
    text = open(a.listing).read()
    runs, loops = scan(text, a.prefix, a.min_depth, a.gap)
    total = sum(r["n"] for r in runs)
    print(f"{a.prefix}: {len(runs)} runs, {total} pure moves at loop depth >= {a.min_depth}; "
          f"largest {max((r['n'] for r in runs), default=0)}")
    tick = tick_loop(loops)
    for h, c in loops.items():
        mine = [r["n"] for r in runs if r["loop2"] == h]
        print(f"  loop {h:<10s} {c['instructions']:5d} instructions, {c['f64']:4d} fp64; {sum(mine):4d} pure moves, "
              f"largest run {max(mine, default=0)}" + ("  <- the tick loop (largest fp64 share)" if h == tick else ""))
    shown = [k for k, r in enumerate(runs) if r["n"] >= a.min_run]
    for k in shown:
        r = runs[k]
        kinds = ", ".join(f"{n} {op}" for op, n in sorted(r["kinds"].items()))
        print(f"  run {k:3d}  line {r['line']:6d}  {r['block']:<14s} depth {r['depth']} in {r['loop2']:<10s} {r['n']:3d} moves  ({kinds})")
    seen = set()
    for i, j, hit, of in inverse_pairs(runs, a.min_run):
        if frozenset((i, j)) not in seen:  # (a pair is usually found from both sides)
            seen.add(frozenset((i, j)))
            print(f"  INVERSE: run {j} ({runs[j]['block']}) undoes run {i} ({runs[i]['block']}): {hit} of {of} registers")


if __name__ == "__main__":
    main()
