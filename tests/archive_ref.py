"""shipsim_archive_elect restated in Python integers and floats (include/shipsim.h: candidates, winner, fill, counts),
with the cases the archive tests share. Nothing here touches the library or the device."""
import math

import numpy as np

NO_CELL = -1
NAN = float("nan")


def elect(cell, score, cell_score, cell_seen, n_cells):
    """One election. cell: ints, score: floats (per env); cell_score: floats, cell_seen: ints (per cell), neither
    changed. Returns (env_of_cell, cell_score, cell_seen, n_improved) as lists and an int. Envs are visited in
    increasing index and a later one wins only with a strictly greater score (IEEE >, so -0.0 does not beat +0.0 nor
    the other way round): ties go to the lowest index."""
    winner = [None] * n_cells
    count = [0] * n_cells
    for i, (c, s) in enumerate(zip(cell, score)):
        c, s = int(c), float(s)
        if not 0 <= c < n_cells or math.isnan(s):
            continue
        count[c] += 1
        if winner[c] is None or s > float(score[winner[c]]):
            winner[c] = i
    env_of_cell, new_score, n_improved = [], [], 0
    for c in range(n_cells):
        w, held = winner[c], float(cell_score[c])
        if w is not None and (math.isnan(held) or float(score[w]) > held):
            env_of_cell.append(w)
            new_score.append(float(score[w]))
            n_improved += 1
        else:
            env_of_cell.append(NO_CELL)
            new_score.append(held)
    seen = [(int(a) + b) & 0xFFFFFFFF for a, b in zip(cell_seen, count)]
    return env_of_cell, new_score, seen, n_improved


def bits(x):
    """float64 values as their uint64 bits (NaN payloads and the sign of zero included)."""
    return np.asarray(x, dtype=np.float64).view(np.uint64)


N_ENVS = (1, 63, 64, 65, 257, 1025, 4096)
N_CELLS = (1, 255, 257, 4097)


def rounds(n_envs, n_cells, seed=0):
    """The elections of one (n_envs, n_cells), run one after the other on the same cell_score / cell_seen (which start
    NaN / 0): a list of (name, cell int32, score float64)."""
    rng = np.random.default_rng(1000003 * n_envs + n_cells + seed)
    spread = rng.integers(0, n_cells, n_envs).astype(np.int32)
    few = rng.integers(0, min(n_cells, 3), n_envs).astype(np.int32)
    base = np.round(rng.normal(size=n_envs) * 4.0) / 4.0  # a coarse grid: many exact ties between envs
    out = []
    # values far below the rest, spread over the cells: most cells are taken once
    out.append(("first", spread, base - 100.0))
    # the same envs again: improved by 1, equal (not strictly greater: stays), or worse, a third each
    out.append(("second", spread, base - 100.0 + (np.arange(n_envs) % 3 - 1.0)))
    # every env in one cell
    out.append(("one_cell", np.full(n_envs, n_cells - 1, np.int32), base))
    # every score equal: the lowest index of each cell wins
    out.append(("equal", few, np.full(n_envs, 7.25)))
    # zeros of both signs against each other (and against the NaN / negative cells they find)
    z = np.where(np.arange(n_envs) % 2 == 0, -0.0, 0.0)
    out.append(("zeros", few[::-1].copy(), z))
    out.append(("zeros_again", few, -z))
    # infinities, NaN (two payloads, both signs), the largest and smallest finite values, denormals
    palette = np.array([0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000001,
                        0x7FF0000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x0000000000000001,
                        0x8000000000000001, 0x0000000000000000, 0x8000000000000000, 0x3FF0000000000000],
                       dtype=np.uint64).view(np.float64)
    out.append(("special", spread[::-1].copy(), palette[rng.integers(0, len(palette), n_envs)]))
    # cells out of range: negative, n_cells, the ends of int32
    bad = np.array([-1, n_cells, 2**31 - 1, -2**31, n_cells + 1], dtype=np.int64)
    c = spread.astype(np.int64)
    pick = rng.random(n_envs) < 0.5
    c[pick] = bad[rng.integers(0, len(bad), int(pick.sum()))]
    out.append(("out_of_range", c.astype(np.int32), base + 200.0))
    return out


# ---- the state block's columns (ast_sac_amd/csrc/shipsim_state_host.hpp), restated ----
MAX_ROUTE = 16
ENV_BYTES = (4, 8, 8, 8, 8, 8, 8, 8, 8, 16, 32, 4, 4, 4, 32, 4, 4, 4, 32)


def _r256(b):
    return (b + 255) & ~255


def columns(n, n_ships):
    """(list of (offset, bytes per env) of the 43 columns, bytes of the block) for n envs of n_ships ships."""
    ship, route, env = _r256(n * n_ships * 8), _r256(n * n_ships * MAX_ROUTE * 8), _r256(n * 32)
    cols = [(k * ship, (8 if k < 19 else 4) * n_ships) for k in range(22)]
    cols += [(22 * ship + k * route, MAX_ROUTE * 8 * n_ships) for k in range(2)]
    env_off = 22 * ship + 2 * route
    cols += [(env_off + k * env, b) for k, b in enumerate(ENV_BYTES)]
    return cols, env_off + len(ENV_BYTES) * env


def per_env_bytes(block, n, n_ships):
    """A state block (uint8 numpy array: a snapshot's or an archive's data) as one bytes object per env / cell."""
    cols, total = columns(n, n_ships)
    assert block.size == total, (block.size, total)
    return [b"".join(block[o + i * w:o + (i + 1) * w].tobytes() for o, w in cols) for i in range(n)]
