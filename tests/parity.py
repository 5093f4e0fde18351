"""Parity tolerances shared by the oracle and GPU tests.

North-star tolerance: trajectories within 1e-5 relative of the CPU reference. "Relative" is taken
per column against |ref| plus a floor of 1 % of the column's largest magnitude (so that values
crossing zero — rudder angle, sway speed, yaw rate — are judged on the column's own scale).
Integer / event quantities (tick counts, event bits, done flags, waypoint indices) must match
exactly.
"""
import json
import os
import time

import numpy as np

RTOL = 1e-5


def record(row):
    """One parity row of a GPU test (case, envs checked, decisions checked, sensitive, perturbed, off-oracle, worst
    rel err, explained sbmpc mismatches; None where a case has no such figure), stamped with the time and the
    library's build: appended as one JSON line to $SHIPSIM_PARITY_LOG when that is set, printed otherwise."""
    row = dict(row, time=time.strftime("%Y-%m-%dT%H:%M:%S"),
               library=__import__("ast_sac_amd.shipsim", fromlist=["x"]).load_library().shipsim_build_info().decode())
    line = json.dumps(row)
    path = os.environ.get("SHIPSIM_PARITY_LOG")
    if not path:
        print("\n[parity] " + line)
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def parity_row(case, envs_checked=None, decisions_checked=None, sensitive=None, perturbed=None, off_oracle=None,
               worst_rel_err=None, sbmpc_explained=None, **more):
    return dict(case=case, envs_checked=envs_checked, decisions_checked=decisions_checked, sensitive=sensitive,
                perturbed=perturbed, off_oracle=off_oracle, worst_rel_err=worst_rel_err,
                sbmpc_explained=sbmpc_explained, **more)


def rel_err(got, ref, floor_frac=0.01):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.ndim >= 2:
        scale = np.max(np.abs(ref.reshape(-1, ref.shape[-1])), axis=0)
    else:
        scale = np.max(np.abs(ref)) if ref.size else 0.0
    return np.abs(got - ref) / (np.abs(ref) + floor_frac * scale + 1e-12)


def assert_close(got, ref, rtol=RTOL, what=""):
    e = rel_err(got, ref)
    worst = float(e.max()) if e.size else 0.0
    assert worst <= rtol, f"{what}: worst relative error {worst:.3e} > {rtol:.1e} at {np.unravel_index(e.argmax(), e.shape)}"
    return worst
