"""Selections of the step kernels' table (csrc/shipsim_launch_host.hpp) that no other test walks: the table stream
with the simplified machinery at 8 and 4 lanes per env, and the policy stream at 4. Results are the same at every
lanes-per-env, so each is compared bit for bit with the same handle at 16. 32 envs: two waves at 4 lanes, eight
at 16. Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from test_gpu_policy_act import _trainer
from test_gpu_run_policy import _run
from test_gpu_table import _chained, _table

pytestmark = pytest.mark.gpu

N, MAX_TICKS, N_CALLS = 32, 256, 8
_ref = {}


def _table_stream(lpe):
    cfg = abi.ast_config("sbmpc", machinery=abi.MACH_SIMPLIFIED)
    cfg.lanes_per_env = lpe
    table = _table(2, cfg.max_sampling_frequency, N, seed=31)
    return _chained(cfg, N, table, MAX_TICKS, N_CALLS)


def _policy_stream(lpe):
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = abi.ast_config("sbmpc")
    cfg.lanes_per_env = lpe
    n_dec = int(cfg.max_sampling_frequency)
    recs, _, _ = _run(cfg, N, N_CALLS, MAX_TICKS,
                      lambda sim, c, ep, dec, log, ln: sim.run_policy(dp.weights(), MAX_TICKS, n_dec, ep, dec,
                                                                      deterministic=True, log=log, log_len=ln))
    return recs


@pytest.mark.parametrize("lpe", [8, 4])
def test_table_stream_simplified_machinery_lanes_per_env_bitwise(lpe):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    if "table" not in _ref:
        _ref["table"] = _table_stream(16)
    ref, t_ref = _ref["table"]
    got, t_got = _table_stream(lpe)
    assert t_got == t_ref and t_ref > 0
    assert sum(len(r) for r in ref) >= N  # decisions were taken, so there is something to compare
    for i in range(N):
        np.testing.assert_array_equal(got[i], ref[i], err_msg=f"lpe {lpe} env {i}")


def test_policy_stream_four_lanes_per_env_bitwise():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    ref, got = _policy_stream(16), _policy_stream(4)
    assert sum(len(r) for r in ref) >= N
    for i in range(N):
        np.testing.assert_array_equal(got[i], ref[i], err_msg=f"env {i}")
