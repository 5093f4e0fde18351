"""tests/sac_ref.py checked on the CPU: the float64 step against the torch fp32 backend on the regime inputs, the
float64 Adam against torch.optim.Adam, and the batch draw's Philox, row index and normals."""
import math

import numpy as np
import pytest
import torch

import sac_ref as R
from resample_ref import philox


def _torch_step(case, device="cpu", **over):
    tr = R.make_trainer(case, "torch", device, **over)
    eps = case["eps"].to(device)
    tr.noise_fn = lambda shape: eps
    tr.train_from_torch({k: v.to(device) for k, v in case["batch"].items()})
    o = tr._out
    cols = np.stack([o[k].double().cpu().numpy().reshape(-1) for k in R.COLS])
    losses = np.array([float(x) for x in tr.last_losses()])
    return tr, losses, cols, tr.flat_grad.double().cpu().numpy().copy()


@pytest.mark.parametrize("H,B", R.SHAPES)
def test_ref_step64_matches_torch_fp32_high(H, B):
    """kind="high": float64 is the reference, and torch's fp32 step agrees with it within the project tolerances
    (gradients 1e-4·|ref| + 1e-5·max|ref| per tensor, losses 1e-5·|ref| + 1e-6); the regime shares hold."""
    case = R.regime_case(H, B, "high")
    for k, floor in R.SHARE_FLOORS.items():
        assert case["shares"][k] >= floor, (k, case["shares"])
    assert 0.35 <= case["shares"]["clip_hi"] + case["shares"]["clip_lo"] <= 0.65
    tr, losses, cols, grad = _torch_step(case)
    ref = R.ref_step64(case["nets"], case["log_alpha"], case["batch"], case["eps"], case["hp"])
    ratio, name = R.grad_ratio(grad, ref["flat_grad"], R.grad_blocks(tr))
    col_err = [float(np.abs(cols[i] - ref["cols"][i]).max() / np.abs(ref["cols"][i]).max()) for i in range(6)]
    print(f"high H={H} B={B}: shares {case['shares']} kept {case['kept']:.2f}; torch fp32 vs fp64: gradient "
          f"{ratio:.2f} x tolerance ({name}), columns {max(col_err):.1e} of max")
    assert np.all(np.abs(losses - ref["losses"]) <= 1e-5 * np.abs(ref["losses"]) + 1e-6)
    assert ratio <= 1.0, (ratio, name)
    assert max(col_err) <= 1e-5


@pytest.mark.parametrize("H,B", R.SHAPES)
def test_ref_step64_low_documents_fp32_absorption(H, B):
    """kind="low": std·ε vanishes in fp32 beside the mean, so fp32 log π lacks -ε²/2 on the clamped rows and float64
    is not the reference there. The columns without log π agree (q1_pred, q2_pred, tanh(mean), std); the log π
    discrepancy is present and is ε²/2 on the clamped rows; q_target and the losses agree once that term is accounted."""
    case = R.regime_case(H, B, "low")
    for k, floor in R.SHARE_FLOORS.items():
        assert case["shares"][k] >= floor, (k, case["shares"])
    tr, losses, cols, grad = _torch_step(case)
    ref = R.ref_step64(case["nets"], case["log_alpha"], case["batch"], case["eps"], case["hp"])
    clamped, nclamped = ref["ls_raw"][:B] < -20.0, ref["ls_raw"][B:] < -20.0
    e = case["eps"].double().numpy().reshape(-1)
    lost, nlost = np.where(clamped, 0.5 * e[:B] ** 2, 0.0), np.where(nclamped, 0.5 * e[B:] ** 2, 0.0)
    # q1_pred, q2_pred, tanh(mean), std: no log π in them. 1e-4 of the column's maximum: the raw log_std reaches
    # |40| here, where an fp32 head sum of H terms is good to a few 1e-5 absolute, which is std's relative error
    for i in (0, 1, 4, 5):
        assert np.abs(cols[i] - ref["cols"][i]).max() <= 1e-4 * np.abs(ref["cols"][i]).max(), R.COLS[i]
    d = cols[3] - ref["cols"][3]  # fp32 - fp64 log π: the lost ε²/2 on the clamped rows, rounding elsewhere
    assert np.abs(d[clamped] - lost[clamped]).max() <= 1e-4
    assert np.abs(d[~clamped]).max() <= 1e-3
    ratio, name = R.grad_ratio(grad, ref["flat_grad"], R.grad_blocks(tr))
    rel = float(np.abs(d).max() / np.abs(ref["cols"][3]).max())
    print(f"low H={H} B={B}: shares {case['shares']} kept {case['kept']:.2f}; torch fp32 vs fp64: log π off by "
          f"{rel:.1%} of max, gradient {ratio:.0f} x tolerance ({name})")
    assert float(np.abs(d[clamped]).max()) > 0.1 and ratio > 10.0  # the documented discrepancy is there
    # q_target and the losses see log π too (the next_obs rows' through the target): equal once the float64 values
    # carry the same lost term
    hp, alpha, la = case["hp"], math.exp(case["log_alpha"]), case["log_alpha"]
    term = case["batch"]["terminals"].double().numpy().reshape(-1)
    y = np.clip(ref["target_raw"] - (1.0 - term) * hp["discount"] * alpha * nlost, -hp["clip_val"], hp["clip_val"])
    assert np.abs(cols[2] - y).max() <= 1e-4 * np.abs(y).max()
    want = np.array([ref["losses"][0] + alpha * lost.mean(), np.mean((ref["cols"][0] - y) ** 2),
                     np.mean((ref["cols"][1] - y) ** 2), ref["losses"][3] - la * lost.mean()])
    assert np.all(np.abs(losses - want) <= 1e-5 * np.abs(want) + 1e-6), (losses, want)


def test_only_clamped_case_has_every_obs_row_clamped():
    for kind in ("high", "low"):
        case = R.regime_case(32, 33, kind, only_clamped=True)
        ref = R.ref_step64(case["nets"], case["log_alpha"], case["batch"], case["eps"], case["hp"])
        ls = ref["ls_raw"][:33]
        assert np.all(ls > 2.0) if kind == "high" else np.all(ls < -21.0)
        blocks = dict((n, (a, b)) for n, a, b in R.grad_blocks(R.make_trainer(case, "torch", "cpu")))
        for name in ("pi6", "pi7"):  # last_fc_log_std.weight / .bias
            a, b = blocks[name]
            assert np.all(ref["flat_grad"][a:b] == 0.0)


def test_ref_adam64_matches_torch_adam_two_groups():
    g = torch.Generator().manual_seed(5)
    n_pi, n_q = 37, 2 * 29
    hp = R.adam_hp(3e-4, 1e-3, 0.05)
    p = torch.randn(n_pi + n_q, generator=g, dtype=torch.float64)
    t = torch.randn(n_q, generator=g, dtype=torch.float64)
    a = torch.nn.Parameter(p[:n_pi].clone())
    b = torch.nn.Parameter(p[n_pi:].clone())
    opt = torch.optim.Adam([dict(params=[a], lr=hp["policy_lr"]), dict(params=[b], lr=hp["qf_lr"])],
                           betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"])
    pn, tn, m, v = p.numpy().copy(), t.numpy().copy(), np.zeros(n_pi + n_q), np.zeros(n_pi + n_q)
    tt = t.clone()
    for step in (1, 2, 3):
        grad = torch.randn(n_pi + n_q, generator=g, dtype=torch.float64) * 10.0 ** float(step - 2)
        a.grad, b.grad = grad[:n_pi].clone(), grad[n_pi:].clone()
        opt.step()
        tt = tt * (1.0 - hp["tau"]) + hp["tau"] * b.detach()
        pn, tn, m, v, _ = R.ref_adam64(pn, tn, m, v, grad.numpy(), step, dict(q_base=n_pi), hp)
        np.testing.assert_allclose(pn, torch.cat([a, b]).detach().numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(tn, tt.numpy(), rtol=1e-13, atol=1e-15)
        st = opt.state[a]
        np.testing.assert_allclose(m[:n_pi], st["exp_avg"].numpy(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(v[:n_pi], st["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-300)
    # a fixed entropy weight: slot 0 frozen
    p2, _, m2, v2, d = R.ref_adam64(pn, tn, m, v, np.ones_like(pn), 4, dict(q_base=n_pi), dict(hp, auto_entropy=False))
    assert p2[0] == pn[0] and m2[0] == m[0] and v2[0] == v[0] and d[0] == 0.0 and p2[1] != pn[1]


def test_philox_known_answers():
    assert philox(0, 0, 0, 0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert philox(f, f, f, f, f, f) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # the array form is the scalar one, and the draw's counter block is (item, step lo, step hi, 0x5AC0)
    seed, step = (0x1234ABCD << 32) | 0x0BADF00D, (1 << 32) + 5
    w = R.draw_words(seed, step, 5)
    for i in range(5):
        assert [int(x[i]) for x in w] == philox(i, 5, 1, 0x5AC0, 0x0BADF00D, 0x1234ABCD)
    assert [int(x[3]) for x in R.draw_words(seed, 5, 5)] != [int(x[3]) for x in w]


def test_row_index_range_and_extremes():
    cap = 700
    for size in (0, 1, 3, cap):
        idx = R.row_index(np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint64), size, cap)
        assert idx.min() >= 0 and idx.max() < max(size, 1)
        assert idx[0] == 0 and idx[-1] == max(size, 1) - 1
    assert R.row_index(np.array([0xFFFFFFFF], dtype=np.uint64), cap + 50, cap)[0] == cap - 1  # (capped)


def test_normals_finite_at_the_extremes():
    e0, e1 = R.normals(np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint64),
                       np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF], dtype=np.uint64))
    assert e0.dtype == np.float32 and e1.dtype == np.float32
    assert np.all(np.isfinite(e0)) and np.all(np.isfinite(e1))
    assert abs(float(e0[0]) - math.sqrt(-2.0 * math.log(2.0 ** -32))) < 1e-5  # u1 = 2^-32, u2 = 0
    assert np.all(e0[2:] == 0.0) and np.all(e1[2:] == 0.0)  # u1 = 1: radius 0


def test_draw_moments():
    n = 1 << 16
    idx, e0, e1 = R.draw_batch((0xDEADBEEF << 32) | 0x12345678, 3, n, 7, 700)
    for e in (e0.astype(np.float64), e1.astype(np.float64), np.concatenate([e0, e1]).astype(np.float64)):
        k = e.size
        assert abs(e.mean()) <= 4.0 / math.sqrt(k)
        assert abs(e.var() - 1.0) <= 4.0 * math.sqrt(2.0 / k)
    assert abs(float(np.mean(e0.astype(np.float64) * e1))) <= 4.0 / math.sqrt(n)  # (the pair is uncorrelated)
    p = 1.0 / 7.0
    hits = np.bincount(idx, minlength=7) / n
    assert hits.size == 7 and np.all(np.abs(hits - p) <= 4.0 * math.sqrt(p * (1 - p) / n))


def test_adam_bounds_hold_for_exactly_rounded_fp32():
    """adam_st's arithmetic emulated with numpy float32 (every operation rounded once) stays inside adam_bounds over
    two updates on spread gradients; and bounds relative to the result alone would not hold: where 0.9 m + 0.1 g
    cancels, exactly rounded fp32 is off by far more than 2^-21 of the small result."""
    f = np.float32
    n, qb = 60000, 20000
    hp = R.adam_hp(3e-4, 1e-3, 0.05)
    b1, b2, eps, tau = f(hp["beta1"]), f(hp["beta2"]), f(hp["eps"]), f(hp["tau"])
    rng = np.random.default_rng(2)
    p, t = (rng.standard_normal(n) * 0.1).astype(f), (rng.standard_normal(n - qb) * 0.1).astype(f)
    m, v = np.zeros(n, f), np.zeros(n, f)
    worst_rel_m = 0.0
    for step, g in ((1, np.ones(n, f)), (2, R.spread_gradient(n, 7))):
        ss = np.where(np.arange(n) >= qb, hp["qf_lr"], hp["policy_lr"]) / (1.0 - hp["beta1"] ** step)
        m2 = m + (f(1) - b1) * (g - m)
        v2 = v * b2 + (f(1) - b2) * (g * g)
        p2 = p + (-ss.astype(f)) * (m2 / (np.sqrt(v2) / f(math.sqrt(1.0 - hp["beta2"] ** step)) + eps))
        t2 = t * (f(1) - tau) + p2[qb:] * tau
        ref, bound = R.adam_bounds(p, t, m, v, g, step, dict(q_base=qb), hp)
        for k, x in (("m", m2), ("v", v2), ("p", p2), ("t", t2)):
            assert x.dtype == f and np.all(np.abs(x - ref[k]) <= bound[k]), (step, k)
        worst_rel_m = max(worst_rel_m, float((np.abs(m2 - ref["m"]) / (np.abs(ref["m"]) + 1e-300)).max()))
        p, t, m, v = p2, t2, m2, v2
    assert worst_rel_m > 2.0 ** -21
