"""Adam, the soft target update and the transposed-weight refresh of the split update (sac_apply_kernel in
csrc/sac_kernels.hip) against torch's Adam in float64 (tests/sac_ref.py: ref_adam64), element by element, with unequal
learning rates (policy 3e-4, critics 1e-3: the group of every element shows) and τ = 0.05.

An update here is sacf_grads (which advances the step counter and leaves the step's bias corrections in stats[5..7]),
a gradient of the test's choice written over the flat gradient, then sacf_apply. Bounds: sac_ref.adam_bounds, from the
rounding count of adam_st — 2^-21 relative on m and v, 2^-23·|p| + 2^-20·|step| on p, 2^-22·max(|t_old|, |p|) on the
targets, each relative to the operands where 0.9 m + 0.1 g cancels (tests/test_sac_ref_cpu.py shows exactly rounded
fp32 needs that)."""
import numpy as np
import pytest
import torch

import sac_ref as R
from test_sac import _rand_batch, _seeded_nets

WIDTHS = [32, 64, 96, 128, 160, 192, 224, 256, 320, 384, 448, 512]
B = 32
LR_PI, LR_Q, TAU = 3e-4, 1e-3, 0.05
STATE = (("p", "flat_param"), ("t", "flat_target"), ("m", "_adam_m"), ("v", "_adam_v"))


def _trainer(H, auto=True, lr_pi=LR_PI, lr_q=LR_Q):
    from ast_sac_amd.ast_sac.torch.sac.sac_fused import FusedSACTrainer
    pol, qs = _seeded_nets(H, "cuda", 5)
    return FusedSACTrainer(env=R._Env, policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3],
                           discount=0.965, reward_scale=0.75, policy_lr=lr_pi, qf_lr=lr_q, soft_target_tau=TAU,
                           action_reg_coeff=0.01, clip_val=100.0, use_automatic_entropy_tuning=auto, batch_size=B,
                           use_graph=False, backend="hip", split_update=True)


def _state(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, name).cpu().numpy().copy() for k, name in STATE}


def _update(tr, batch, eps, G):
    """One update with the flat gradient G; returns (state before, state after, step number)."""
    before = _state(tr)
    tr._sf.set_stream()
    tr._sf.grads(batch, eps)
    tr.flat_grad.copy_(torch.as_tensor(G, device="cuda"))
    tr._sf.apply()
    return before, _state(tr), int(tr._step_t)


def _layout(tr):
    return dict(q_base=1 + sum(p.numel() for p in tr.policy.parameters()))


def _inputs():
    batch, eps = _rand_batch(B, "cuda", seed=2)
    return batch, eps.reshape(-1).contiguous()


def _assert_in_bounds(tag, before, after, G, step, layout, hp):
    ref, bound = R.adam_bounds(before["p"], before["t"], before["m"], before["v"], G, step, layout, hp)
    for k in ("m", "v", "p", "t"):
        err = np.abs(after[k].astype(np.float64) - ref[k])
        worst = float((err / np.where(bound[k] > 0, bound[k], 1.0))[bound[k] > 0].max())
        print(f"{tag}: {k} worst |Δ| / bound {worst:.2f}")
        bad = np.flatnonzero(err > bound[k])
        assert bad.size == 0, f"{tag}: {k} out of bounds at {bad.size} elements, first {bad[:5]} (critics from {layout})"
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("H", WIDTHS)
def test_apply_unit_gradient_moves_every_element_once(H):
    """G ≡ 1 at step 1, every compiled width: every element moves by its own group's learning rate (log α and π by
    3e-4, the critics by 1e-3) — none untouched, none twice: the 32 x 32 tiles of the three W2 blocks, the flat path that
    skips them, the boundary between π and the critics —, m = 1 - β1 and v = 1 - β2 everywhere, targets soft-updated."""
    tr = _trainer(H)
    batch, eps = _inputs()
    n, layout, hp = tr.flat_param.numel(), _layout(tr), R.adam_hp(LR_PI, LR_Q, TAU)
    G = np.ones(n, np.float32)
    before, after, step = _update(tr, batch, eps, G)
    assert step == 1
    _assert_in_bounds(f"H={H} G=1", before, after, G, 1, layout, hp)
    lr = np.where(np.arange(n) >= layout["q_base"], LR_Q, LR_PI)
    moved = after["p"].astype(np.float64) - before["p"]
    assert np.all(np.abs(moved + lr) <= 2.0 ** -23 * np.abs(after["p"]) + 2.0 ** -20 * lr)
    # (β1, β2 reach the kernels as float32: 1 - fl(β) is off the nominal 1 - β by up to 2^-25)
    assert np.all(np.abs(after["m"] - 0.1) <= 2.0 ** -25 + 2.0 ** -21 * 0.1)
    assert np.all(np.abs(after["v"] - 1e-3) <= 2.0 ** -25 + 2.0 ** -21 * 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [32, 256, 320, 512])
def test_apply_spread_of_gradients_second_step(H):
    """Step 1 with G = 1 (0 on a tenth of the elements), step 2 with gradients from 1e-12 to 1e4, zeros and normals on
    the carried Adam state, both against the float64 Adam; an element with g = 0 and m = v = 0 keeps its bits."""
    tr = _trainer(H)
    batch, eps = _inputs()
    n, layout, hp = tr.flat_param.numel(), _layout(tr), R.adam_hp(LR_PI, LR_Q, TAU)
    G1 = np.ones(n, np.float32)
    G1[np.random.default_rng(H).random(n) < 0.1] = 0.0
    G2 = R.spread_gradient(n, H + 1)
    idle = (G1 == 0.0) & (G2 == 0.0)
    assert idle.sum() > 0
    start = _state(tr)
    for step, G in ((1, G1), (2, G2)):
        before, after, got_step = _update(tr, batch, eps, G)
        assert got_step == step
        _assert_in_bounds(f"H={H} step {step}", before, after, G, step, layout, hp)
    for k in ("p", "m", "v"):
        assert np.array_equal(after[k][idle].view(np.uint32), start[k][idle].view(np.uint32)), k


@pytest.mark.gpu
def test_apply_fixed_entropy_weight_keeps_slot_0():
    """use_automatic_entropy_tuning=False: slot 0 (log α) keeps its bits in p, m and v whatever its gradient slot holds;
    every other element is updated."""
    tr = _trainer(64, auto=False)
    batch, eps = _inputs()
    with torch.no_grad():
        tr.flat_param[0], tr._adam_m[0], tr._adam_v[0] = -1.3, 0.25, 0.5
    n, layout, hp = tr.flat_param.numel(), _layout(tr), R.adam_hp(LR_PI, LR_Q, TAU, auto_entropy=False)
    G = np.ones(n, np.float32)
    before, after, _ = _update(tr, batch, eps, G)
    _assert_in_bounds("fixed entropy weight", before, after, G, 1, layout, hp)
    for k in ("p", "m", "v"):
        assert after[k][0].view(np.uint32) == before[k][0].view(np.uint32), k
        assert np.all(after[k][1:] != before[k][1:]), k


@pytest.mark.gpu
@pytest.mark.parametrize("H,Bc", [(64, 96), (320, 45)])
def test_apply_refreshes_the_transposed_weights(H, Bc):
    """After a G ≡ 1 update with both learning rates 1e-2 (every weight moves by 0.01) the next hip step's per-row
    columns are the float64 step's on the updated parameters and targets: a stale W2ᵀ copy of the actor, a critic or a
    target would put every row off."""
    case = R.regime_case(H, Bc, "high")
    tr = R.make_trainer(case, "hip", "cuda", policy_lr=1e-2, qf_lr=1e-2, soft_target_tau=TAU, split_update=True)
    batch = {k: v.cuda().contiguous() for k, v in case["batch"].items()}
    eps = case["eps"].cuda().reshape(-1).contiguous()
    n, layout = tr.flat_param.numel(), _layout(tr)
    G = np.ones(n, np.float32)
    before, after, _ = _update(tr, batch, eps, G)
    _assert_in_bounds(f"H={H} lr 1e-2", before, after, G, 1, layout, R.adam_hp(1e-2, 1e-2, TAU))
    stale = R.step_result(tr)["cols"]  # (the step before the update)
    tr._sf.grads(batch, eps)
    hip = R.step_result(tr)["cols"]
    nets = dict(policy=tr.policy, qf1=tr.qf1, qf2=tr.qf2, target_qf1=tr.target_qf1, target_qf2=tr.target_qf2)
    log_alpha = float(tr.flat_param[0])
    ref = R.ref_step64(nets, log_alpha, case["batch"], case["eps"], case["hp"], with_grad=False)["cols"]
    yard_tr = R.make_trainer(case, "torch", "cuda", nets=nets)
    with torch.no_grad():
        yard_tr.log_alpha.fill_(log_alpha)
    yard = R.run_step(yard_tr, case["batch"], case["eps"])["cols"]
    bound = R.col_bounds(ref, yard)
    ratio = np.abs(hip - ref).max(axis=1) / bound
    moved = np.abs(stale.astype(np.float64) - ref).max(axis=1) / bound
    print(f"H={H} B={Bc} after the update: columns {ratio.max():.2f} x bound; the update moved them by {moved.max():.0f} x")
    assert moved[:3].min() > 100.0  # (the update is visible in every critic column)
    assert np.all(ratio <= 1.0), dict(zip(R.COLS, ratio))
