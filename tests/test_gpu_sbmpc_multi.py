"""shipsim_sbmpc_eval_multi: SBMPC.get_optimal_ctrl_offset over a do_list of K obstacles (sbmpc.py:113-185) on the
device, through the C ABI — the optimiser the multi-obstacle env kernels (n_obs_ships = K > 1, configs[4]) run.

Pinned to the REFERENCE's own answers for K = 2, 3, 4 (tests/golden/sbmpc_multi.npz, made by
tests/golden/gen_golden.py gen_sbmpc_multi: one persistent controller per K, so the last-offset state carries from
call to call), and to the oracle on random batches. The batches cover both ways a wave serves requests: two
requests per pass (each lane taking its scenario's obstacles in turn) and a lone request whose obstacles the two
half-waves split; the lane-placement test puts the requests on chosen lanes of a wave. The service runs the optimiser
instantiations of the env kernels of the same K (three obstacles at K <= 3, four at K = 4), so these tests pin the
code the envs run. Device answers are compared with the oracle's exactly; a mismatch has to be explained by the
oracle itself (tests/sbmpc_requests.py), and on these batches none is."""
import numpy as np
import pytest

import sbmpc_requests as R
from ast_sac_amd import shipsim_abi as abi
from parity import parity_row, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def _requests_from_fixture(g, K):
    ins, outs = g[f"k{K}_in"], g[f"k{K}_out"]
    reqs, refs = [], []
    p_last, chi_last = 1.0, 0.0
    for row, out in zip(ins, outs):
        slots = np.zeros(7 * abi.MAX_OBS)
        slots[:7 * K] = row[8:8 + 7 * K]
        reqs.append(np.concatenate([[p_last, chi_last], row[:8], slots]))
        refs.append(out[:3])
        p_last, chi_last = out[3], out[4]
    return np.array(reqs), np.array(refs)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_sbmpc_eval_multi_matches_reference_known_answers(golden, torch_cuda, K):
    from ast_sac_amd.shipsim import sbmpc_eval_multi
    g = golden("sbmpc_multi")
    reqs, refs = _requests_from_fixture(g, K)
    assert reqs.shape[1] == abi.SBMPC_MULTI_IN
    got = sbmpc_eval_multi(reqs, K).cpu().numpy()  # every request in one launch (two per pass)
    np.testing.assert_array_equal(got, refs)
    for i in range(len(reqs)):  # each alone (one request per wave: the half-waves split its obstacles)
        if i % 7 == 0:
            np.testing.assert_array_equal(sbmpc_eval_multi(reqs[i:i + 1], K).cpu().numpy()[0], refs[i])


_random_requests = R.random_requests


def _far(req):
    """the same requests with every obstacle's x moved out of D_INIT: inactive"""
    far = np.array(req)
    for k in range(abi.MAX_OBS):
        far[:, 10 + 7 * k] += 1e5
    return far


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sbmpc_eval_multi_matches_oracle(torch_cuda, K):
    """2048 random requests (half of the obstacles on a collision course, sizes varied) vs the oracle; then the same
    requests with only every 64th active (each wave serves one lone request: the split path) and every 32nd.
    The oracle's answers for these batches do not move under sbmpc_requests.FAMILY
    (tests/test_sbmpc_inputs_cpu.py), so there is no tie to hide behind: a device answer off the oracle's must be
    returned by the oracle for some member of the family, or the test fails; those that are count against the
    n // 1000 cap and are printed and logged."""
    from ast_sac_amd.shipsim import sbmpc_eval_multi
    n = R.MULTI_N
    req, ref, one = R.multi_batch(K)
    got = sbmpc_eval_multi(req.copy(), K).cpu().numpy()
    assert got[:, 2].sum() > n // 2
    assert ((ref[:, 0] != 1) | (ref[:, 1] != 0)).sum() > n // 10  # the optimiser really chooses
    explained = [R.assert_no_unexplained(f"K={K} dense", req, got, ref, one, n // 1000)]
    for stride in (64, 32):
        far = np.ones(n, bool)
        far[::stride] = False
        sparse = np.where(far[:, None], _far(req), req)  # every other request's obstacles out of D_INIT: inactive
        got_s = sbmpc_eval_multi(sparse, K).cpu().numpy()
        assert got_s[far, 2].sum() == 0 and (got_s[far, :2] == [1.0, 0.0]).all()
        # the active requests' answers do not depend on how a wave served them (lone: split obstacles; paired)
        explained.append(R.assert_no_unexplained(f"K={K} stride {stride}", req[~far], got_s[~far], ref[~far], one,
                                                 n // 1000))
    record(parity_row(f"sbmpc_eval_multi_matches_oracle[{K}]", decisions_checked=n + n // 64 + n // 32,
                      sbmpc_explained=sum(explained)))


@pytest.mark.parametrize("K", [3, 4])
def test_sbmpc_eval_multi_other_horizon(torch_cuda, K):
    """tf = 600, dt = 30 (20 samples; every other test runs 1000 / 20): the out-of-reach test (sbmpc_far) and the
    sample count depend on the horizon. 512 requests against the oracle at the same horizon, exactly: the oracle's
    answers for this batch do not move under the family either (tests/test_sbmpc_inputs_cpu.py)."""
    from ast_sac_amd.shipsim import sbmpc_eval_multi
    req, ref, one = R.horizon_batch(K)
    got = sbmpc_eval_multi(req.copy(), K, tf=R.HORIZON_TF, dt=R.HORIZON_DT).cpu().numpy()
    assert got[:, 2].sum() > len(req) // 2
    assert ((ref[:, 0] != 1) | (ref[:, 1] != 0)).sum() > len(req) // 10
    default = sbmpc_eval_multi(req.copy(), K).cpu().numpy()
    assert (default != got).any()  # the horizon matters to these requests
    explained = R.assert_no_unexplained(f"K={K} tf 600 dt 30", req, got, ref, one, len(req) // 1000)
    record(parity_row(f"sbmpc_eval_multi_other_horizon[{K}]", decisions_checked=len(req), sbmpc_explained=explained))


# Which lanes of a wave raise a request decides how the optimiser serves it (csrc/shipsim_sbmpc.hpp
# sbmpc_cooperative_multi): two requests per pass, one per half-wave; a lone or last odd request split over the
# halves, whichever half its lane is in. The env kernels raise requests from lanes 0, 16, 32 and 48.
LANE_PATTERNS = ([(l,) for l in (0, 1, 15, 16, 31, 32, 33, 47, 48, 63)]
                 + [(0, 1), (3, 5), (40, 50), (31, 32), (0, 63)]
                 + [(0, 16, 32), (5, 6, 7), (33, 40, 63)]
                 + [(0, 16, 32, 48, 63)]
                 + [tuple(range(64))])
LANE_REPEATS = 8


def _lane_batch(pool, tail):
    """Waves of 64 rows, LANE_REPEATS per pattern, the active lanes holding successive pool requests (so which
    request sits on which lane rotates) and every other row an inactive one; then a last partial wave of `tail`
    rows whose only active request is in its last lane. Returns (rows, per row the pool index or -1)."""
    P = len(pool)
    far = _far(pool)
    rows, src, c = [], [], 0
    waves = [(64, lanes) for lanes in LANE_PATTERNS * LANE_REPEATS] + [(tail, (tail - 1,))]
    for width, lanes in waves:
        for lane in range(width):
            if lane in lanes:
                rows.append(pool[c % P])
                src.append(c % P)
                c += 1
            else:
                rows.append(far[(c + lane) % P])
                src.append(-1)
    return np.array(rows), np.array(src)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sbmpc_eval_multi_lane_placement(torch_cuda, K):
    """A request's answer does not depend on the lane that raises it, on the other requests of its wave, or on the
    wave being a partial one. Requests whose oracle answer is active and not the default (1, 0) (a wrong write-back
    or a missed merge shows) are placed on single lanes of either half-wave, pairs in one half and across the halves,
    triples and a quintuple (paired passes, then a split pass), and full waves, every pattern over 8 different sets
    of requests; the batch ends in a partial wave of 1 or of 33 rows whose last lane holds its only request. Active
    rows equal the oracle's answer and the device's answer for the same request in a dense batch, exactly;
    inactive rows are (1, 0, 0)."""
    from ast_sac_amd.shipsim import sbmpc_eval_multi
    req, ref, _ = R.multi_batch(K)
    chooses = (ref[:, 2] == 1) & ((ref[:, 0] != 1) | (ref[:, 1] != 0))
    assert chooses.sum() >= 64
    pool, pool_ref = req[chooses][:256], ref[chooses][:256]
    dense = sbmpc_eval_multi(pool, K).cpu().numpy()
    np.testing.assert_array_equal(dense, pool_ref)
    assert len({tuple(a) for a in pool_ref}) >= 8  # many different answers: a swapped write-back changes a row
    for tail in (1, 33):
        rows, src = _lane_batch(pool, tail)
        assert len(rows) % 64 == tail and len(rows) == 64 * len(LANE_PATTERNS) * LANE_REPEATS + tail
        got = sbmpc_eval_multi(rows, K).cpu().numpy()
        act = src >= 0
        assert act[-1] and not act[len(rows) - tail:-1].any()
        bad = np.nonzero((got[act] != pool_ref[src[act]]).any(axis=1))[0]
        where = np.nonzero(act)[0][bad]
        assert not len(bad), (f"K={K} tail {tail}: (wave, lane) of rows off the oracle",
                              [(int(w) // 64, int(w) % 64) for w in where[:10]], got[where[:3]],
                              pool_ref[src[where[:3]]])
        np.testing.assert_array_equal(got[act], dense[src[act]])
        np.testing.assert_array_equal(got[~act], np.broadcast_to([1.0, 0.0, 0.0], got[~act].shape))


def test_sbmpc_eval_multi_k1_equals_single_obstacle_service(torch_cuda):
    """With one obstacle the multi-obstacle service is the reference's single-obstacle call: the same answers as
    shipsim_sbmpc_eval."""
    from ast_sac_amd.shipsim import sbmpc_eval, sbmpc_eval_multi
    rng = np.random.Generator(np.random.PCG64(9))
    req = _random_requests(rng, 1024, 1)
    single = np.concatenate([req[:, :10], req[:, 10:15], req[:, 15:17]], 1)
    np.testing.assert_array_equal(sbmpc_eval_multi(req, 1).cpu().numpy(), sbmpc_eval(single).cpu().numpy())


def test_sbmpc_eval_multi_rejects_bad_counts(torch_cuda):
    from ast_sac_amd.shipsim import ShipSimError, sbmpc_eval_multi
    req = np.zeros((4, abi.SBMPC_MULTI_IN))
    for k in (0, abi.MAX_OBS + 1):
        with pytest.raises(ShipSimError, match=r"\(-?\d+\).*n_obs"):
            sbmpc_eval_multi(req, k)
    for tf, dt in ((1000.0, 0.0), (1000.0, -20.0), (4097.0 * 20.0, 20.0)):  # dt <= 0, tf / dt > 4096
        with pytest.raises(ShipSimError) as e:
            sbmpc_eval_multi(req, 2, tf=tf, dt=dt)
        assert "n_obs" not in str(e.value) and "tf" in str(e.value)  # (n_obs = 2 is in range: not the reason given)
