"""The fused SAC step (csrc/sac_kernels.hip) against an independent reference where training takes it: log_std
clamped on either side, tanh saturated, the Q target clamped from above and from below, each critic the smaller one
on a share of rows, terminal rows, an entropy weight != 1 (tests/sac_ref.py: regime_case).

Reference: kind "high" float64 (sac_ref.ref_step64); kind "low" the torch fp32 backend on the GPU (sac_ref's module
docstring: fp32 absorbs std·ε at std = e^-20, so float64 computes another log π).

Tolerances. Gradients: the project's 1e-4·|ref| + 1e-5·max|ref| per parameter tensor; losses 1e-5·|ref| + 1e-6.
Per-row columns: worst |Δ| <= 4 x yardstick + 2^-22 · max|column|, the yardstick being the reference side's own fp32
spread on the same inputs (high: |torch fp32 on the GPU - float64|; low: |torch fp32 on the CPU - on the GPU|): both
sides are fp32 evaluations of the same formulas that differ in summation order and math functions, while a wrong row,
mask or sign moves a column by about 1/B. Where the project's gradient tolerance is below 4 x the yardstick's own ratio
to it, that takes its place; a yardstick above 10 x the project tolerance fails the case as ill-chosen inputs."""
import copy

import numpy as np
import pytest
import torch

import sac_ref as R

KINDS = ("high", "low")
_REFS = {}


def _step(case, backend, device, nets=None, batch=None, **over):
    tr = R.make_trainer(case, backend, device, nets=nets, **over)
    return tr, R.run_step(tr, batch or case["batch"], case["eps"])


def _reference(case, key=None, nets=None, batch=None, **over):
    """(ref, yard): the reference step of the case's kind and the yardstick step, each dict(losses, cols, grad);
    ref also carries target_raw, the unclamped target. Shared between the tests of one case (key)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    tr, tg = _step(case, "torch", "cuda", nets, batch, **over)
    if case["kind"] == "high":
        r = R.ref_step64(nets or case["nets"], case["log_alpha"], batch or case["batch"], case["eps"],
                         R.trainer_hp(case, tr))
        ref, yard = dict(losses=r["losses"], cols=r["cols"], grad=r["flat_grad"], target_raw=r["target_raw"]), tg
    else:
        _, yard = _step(case, "torch", "cpu", nets, batch, **over)
        _, raw = _step(case, "torch", "cuda", nets, batch, **dict(over, clip_val=float("inf")))
        ref = dict(tg, target_raw=raw["cols"][2])
    ref = {k: np.asarray(v, np.float64) for k, v in ref.items()}
    if key is not None:
        _REFS[key] = (ref, yard)
    return ref, yard


def _col_bounds(ref, yard):
    return R.col_bounds(ref["cols"], yard["cols"])


def _check(tag, tr, hip, ref, yard):
    """The comparison of the module docstring; prints the measured worst ratios before it asserts."""
    blocks = R.grad_blocks(tr)
    loss_ratio = float((np.abs(hip["losses"] - ref["losses"]) / (1e-5 * np.abs(ref["losses"]) + 1e-6)).max())
    bounds = _col_bounds(ref, yard)
    col_ratio = np.array([np.abs(hip["cols"][i] - ref["cols"][i]).max() / bounds[i] for i in range(6)])
    col_yard = np.array([np.abs(yard["cols"][i] - ref["cols"][i]).max() / np.abs(ref["cols"][i]).max() for i in range(6)])
    g_hip, g_name = R.grad_ratio(hip["grad"], ref["grad"], blocks)
    g_yard, _ = R.grad_ratio(yard["grad"], ref["grad"], blocks)
    allowed = max(1.0, 4.0 * g_yard)
    print(f"{tag}: loss {loss_ratio:.2f} x tol; columns {col_ratio.max():.2f} x bound ({R.COLS[int(col_ratio.argmax())]}; "
          f"yardstick {col_yard.max():.1e} of max); gradient {g_hip:.2f} x project tol ({g_name}), yardstick "
          f"{g_yard:.2f} x, allowed {allowed:.2f} x")
    assert np.all(np.isfinite(hip["cols"])) and np.all(np.isfinite(hip["grad"])) and np.all(np.isfinite(hip["losses"]))
    assert g_yard <= 10.0, f"{tag}: ill-chosen inputs, the yardstick is {g_yard:.1f} x the project tolerance"
    assert loss_ratio <= 1.0, (tag, hip["losses"], ref["losses"])
    assert np.all(col_ratio <= 1.0), (tag, dict(zip(R.COLS, col_ratio)))
    assert g_hip <= allowed, (tag, g_hip, g_name)
    return bounds


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,B", R.SHAPES)
def test_hip_step_matches_reference_in_regime(H, B, kind):
    """Losses, the six per-row diagnostics and the flat gradient of one hip step on the regime inputs; every row whose
    target the clamp binds carries ±clip_val bit for bit; the log_std head's gradient is finite."""
    case = R.regime_case(H, B, kind)
    for k, floor in R.SHARE_FLOORS.items():
        assert case["shares"][k] >= floor, (k, case["shares"])
    ref, yard = _reference(case, (H, B, kind))
    tr, hip = _step(case, "hip", "cuda")
    bounds = _check(f"{kind} H={H} B={B}", tr, hip, ref, yard)
    clip = np.float32(case["hp"]["clip_val"])
    raw, y = ref["target_raw"], hip["cols"][2]
    over, under = raw > float(clip) + bounds[2], raw < -float(clip) - bounds[2]
    assert over.sum() >= 0.04 * B and under.sum() >= 0.04 * B
    assert np.array_equal(y[over].view(np.uint32), np.full(int(over.sum()), clip).view(np.uint32))
    assert np.array_equal(y[under].view(np.uint32), np.full(int(under.sum()), -clip).view(np.uint32))
    assert np.all(np.abs(y) <= clip)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,B", R.SHAPES)
def test_hip_q_target_without_clip_and_all_terminal(H, B, kind):
    """clip_val=inf (the class default): q_target is the unclamped reference, nothing is NaN. Every terminal 1:
    q_target is fl(reward_scale · reward), clamped, bit for bit."""
    case = R.regime_case(H, B, kind)
    ref, yard = _reference(case, (H, B, kind))
    tr, hip = _step(case, "hip", "cuda", clip_val=float("inf"))
    assert np.all(np.isfinite(hip["cols"])) and np.all(np.isfinite(hip["grad"])) and np.all(np.isfinite(hip["losses"]))
    bound = _col_bounds(ref, yard)[2] + 2.0 ** -22 * np.abs(ref["target_raw"]).max()
    d = float(np.abs(hip["cols"][2] - ref["target_raw"]).max())
    print(f"{kind} H={H} B={B} clip=inf: q_target off by {d:.2e}, bound {bound:.2e}")
    assert d <= bound
    batch = dict(case["batch"], terminals=torch.ones_like(case["batch"]["terminals"]))
    tr, hip = _step(case, "hip", "cuda", batch=batch)
    clip = np.float32(case["hp"]["clip_val"])
    want = np.clip(np.float32(case["hp"]["reward_scale"]) * batch["rewards"].numpy().reshape(-1), -clip, clip)
    assert want.dtype == np.float32 and np.array_equal(hip["cols"][2].view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_hip_log_std_head_gradient_is_zero_on_clamped_rows(kind):
    """A batch (B = 33: 31 padding rows) whose obs rows all have log_std clamped: the clamp's gradient mask leaves the
    log_std head's weight and bias gradient exactly 0; everything else still matches the reference."""
    case = R.regime_case(32, 33, kind, only_clamped=True)
    ref, yard = _reference(case)
    tr, hip = _step(case, "hip", "cuda")
    _check(f"{kind} only clamped rows", tr, hip, ref, yard)
    blocks = {n: (a, b) for n, a, b in R.grad_blocks(tr)}
    for name in ("pi6", "pi7"):  # last_fc_log_std.weight, .bias
        a, b = blocks[name]
        assert np.all(hip["grad"][a:b] == 0.0), name
    a, b = blocks["pi4"]  # (the mean head's is not)
    assert np.abs(hip["grad"][a:b]).max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("H,B", [(64, 96), (320, 45)])
def test_hip_twin_minimum_tie_on_every_row(H, B):
    """qf2 = qf1 and target_qf2 = target_qf1: min(Q1, Q2) ties on every row, torch.minimum's backward gives each critic
    half, and the two critics' gradient blocks are the same bits."""
    case = R.regime_case(H, B, "high")
    nets = {k: copy.deepcopy(v) for k, v in case["nets"].items()}
    nets["qf2"].load_state_dict(nets["qf1"].state_dict())
    nets["target_qf2"].load_state_dict(nets["target_qf1"].state_dict())
    ref, yard = _reference(case, nets=nets)
    tr, hip = _step(case, "hip", "cuda", nets=nets)
    _check(f"tie H={H} B={B}", tr, hip, ref, yard)
    n = sum(p.numel() for p in tr.qf1.parameters())
    g1, g2 = hip["grad"][-2 * n:-n], hip["grad"][-n:]
    assert np.abs(g1).max() > 0 and np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    assert np.array_equal(hip["cols"][0].view(np.uint32), hip["cols"][1].view(np.uint32))


@pytest.mark.gpu
def test_hip_fixed_entropy_weight():
    """use_automatic_entropy_tuning=False on the hip backend: α = 1 in both losses, no α-loss, gradient slot 0 is 0, and
    the fused update leaves log α and its Adam state as they were."""
    case = R.regime_case(64, 96, "high")
    ref, yard = _reference(case, use_automatic_entropy_tuning=False)
    tr = R.make_trainer(case, "hip", "cuda", use_automatic_entropy_tuning=False)
    with torch.no_grad():
        tr.flat_param[0], tr._adam_m[0], tr._adam_v[0] = -1.3, 0.25, 0.5  # (must be neither read nor written)
    before = tr.flat_param[1:].clone()
    hip = R.run_step(tr, case["batch"], case["eps"])
    _check("fixed entropy weight", tr, hip, ref, yard)
    st = tr._stats_t.cpu().numpy()
    assert hip["grad"][0] == 0.0 and st[3] == 0.0 and st[4] == 1.0
    assert float(tr.flat_param[0]) == np.float32(-1.3) and float(tr._adam_m[0]) == 0.25 and float(tr._adam_v[0]) == 0.5
    assert bool((tr.flat_param[1:] != before).any())  # (the rest was updated)


@pytest.mark.gpu
@pytest.mark.parametrize("areg", [None, 0.0])
def test_hip_without_action_regulariser(areg):
    case = R.regime_case(64, 96, "high")
    ref, yard = _reference(case, ("areg0",), action_reg_coeff=areg)
    tr, hip = _step(case, "hip", "cuda", action_reg_coeff=areg)
    _check(f"action_reg_coeff={areg}", tr, hip, ref, yard)
    with_reg, _ = _reference(case, (64, 96, "high"))
    assert abs(ref["losses"][0] - with_reg["losses"][0]) > 1e-4  # (the regulariser is visible in these inputs)
