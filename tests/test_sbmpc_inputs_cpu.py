"""The premise of the GPU SBMPC service tests' exact comparison, checked on the oracle alone (no GPU): the oracle's
answers for the very batches those tests send (tests/sbmpc_requests.py: PCG64(100 + K) with 2048 requests for
K = 1..4, PCG64(5) with 4096 single-obstacle requests, and the two 512-request batches of the 600 s / 30 s horizon)
do not change under the perturbation family (own-ship x, own-ship y and the first obstacle's x by relative
+-1e-15 and +-1e-13). No request of these batches sits on a tie or a cost discontinuity, so a device answer off the
oracle's has nothing to hide behind. Change a seed or a batch and this is rechecked here."""
import numpy as np
import pytest

import sbmpc_requests as R

BATCHES = ([("multi", K) for K in (1, 2, 3, 4)] + [("single", None)] + [("horizon", K) for K in (3, 4)])


def test_family_is_the_harness_perturbations_and_their_negatives():
    assert R.FACTORS == (-1e-13, -1e-15, 1e-15, 1e-13)
    assert len(R.FAMILY) == 12 and {c for c, _ in R.FAMILY} == {4, 5, 10}
    r = np.arange(1.0, 18.0)
    p = R.perturbed(r, 4, 1e-13)
    assert p[4] == r[4] * (1 + 1e-13) and p[4] != r[4] and (np.delete(p, 4) == np.delete(r, 4)).all()
    assert (r == np.arange(1.0, 18.0)).all()  # (the request itself is left alone)


@pytest.mark.parametrize("kind,K", BATCHES)
def test_oracle_answers_do_not_move_under_the_family(kind, K):
    req, ref, one = {"multi": R.multi_batch, "horizon": R.horizon_batch}[kind](K) if K else R.single_batch()
    assert len(req) == {"multi": R.MULTI_N, "single": R.SINGLE_N, "horizon": R.HORIZON_N}[kind]
    assert ref[:, 2].sum() > len(req) // 2  # (most requests are active: the answers are the optimiser's)
    moved = [i for i, r in enumerate(req)
             if any(not np.array_equal(a, ref[i]) for a in R.oracle_answers_under_family(r, one))]
    assert not moved, (kind, K, len(moved), moved[:10])


def test_explain_splits_mismatches_by_the_family():
    """explain() on hand-made answers: a row equal to the oracle's is no mismatch, a row the oracle gives for no
    member of the family is unexplained (these batches have no sensitive request, so any wrong answer is)."""
    req, ref, one = R.horizon_batch(3)
    got = np.array(ref[:8])
    got[2] = [0.4, np.deg2rad(30.0), 1.0] if ref[2, 0] != 0.4 else [0.6, np.deg2rad(30.0), 1.0]
    assert R.explain(req[:8], got, ref[:8], one) == ([], [2])
    with pytest.raises(AssertionError):
        R.assert_no_unexplained("hand-made", req[:8], got, ref[:8], one, 8)

    def tie(r):  # a stand-in oracle whose answer flips with the sign of own-ship x's perturbation
        return np.array([1.0, 0.0, 1.0]) if r[4] <= 100.0 else np.array([0.4, 0.0, 1.0])
    q = np.zeros((1, 17))
    q[0, 4] = 100.0
    assert R.explain(q, np.array([[0.4, 0.0, 1.0]]), np.array([tie(q[0])]), tie) == ([0], [])
    assert R.assert_no_unexplained("tie", q, np.array([[0.4, 0.0, 1.0]]), np.array([tie(q[0])]), tie, 1) == 1
