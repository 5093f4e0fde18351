"""The batch draw of the fused SAC step (batch_item in csrc/sac_kernels.hip: Philox -> replay row, Box-Muller normals)
against its numpy restatement (tests/sac_ref.py: draw_batch), through the steps that use it: a hip trainer S that draws
in the kernel is compared with a hip trainer R that is handed, through train_from_torch, the rows and normals
draw_batch names. Same seed, same networks, so with the normals given the two do the same arithmetic on the same
rows (batch_row only changes the row index) and must agree bit for bit; with in-kernel normals they agree within
the project tolerances (the device's logf / cosf / sinf against numpy's): losses 1e-5·|ref| + 1e-6, gradients
1e-4·|ref| + 1e-5·max|ref| per parameter tensor, and the same per-tensor rule on each per-row column.

Batches of 33 and 45 rows leave 31 / 19 padding rows, which in the sampled path draw a row and normals of their
own: the gradients' equality with R (where padding rows get zero noise) shows they reach no weight-gradient sum."""
import numpy as np
import pytest
import torch

import sac_ref as R
from test_sac import _rand_batch, _trainer

CAP = 700
SEED = (0x1234ABCD << 32) | 0x9E3779B1  # both 32-bit halves in use
KEYS = ("observations", "actions", "rewards", "terminals", "next_observations")
STATE = ("flat_param", "flat_target", "_adam_m", "_adam_v", "_step_t")


def _ring(all_terminal=False):
    """A full ring of CAP distinct rows: rewards[i] and observation column 0 encode i."""
    from ast_sac_amd.ast_sac.data_management.replay_buffer import DeviceReplayBuffer
    rows, _ = _rand_batch(CAP, "cpu", seed=11)
    i = torch.arange(CAP, dtype=torch.float32)
    rows["rewards"] = ((i - 350.0) / 50.0).unsqueeze(1)
    rows["observations"][:, 0] = i
    if all_terminal:
        rows["terminals"] = torch.ones(CAP, 1)
    rb = DeviceReplayBuffer(CAP, 8, 1, "cuda")
    rb.add_batch(*[rows[k].cuda() for k in ("observations", "actions", "rewards", "next_observations", "terminals")])
    assert int(rb._size_t) == CAP
    return rb, rows


def _snap(tr):
    return {k: getattr(tr, k).clone() for k in STATE}


def _restore(tr, snap, step=None):
    """The trainer's parameters, targets, Adam state and step counter as snapshotted (and the kernels' transposed
    weight copies with them)."""
    for k in STATE:
        getattr(tr, k).copy_(snap[k])
    if step is not None:
        tr._step_t.fill_(step)
    tr._sf.sync_params()


def _pair(H, B):
    S, Rt = _trainer("hip", H, B, "cuda", seed=3), _trainer("hip", H, B, "cuda", seed=3)
    S._seed = SEED
    return S, Rt, _snap(S)


def _sampled(S, snap, rb, size, step, eps):
    _restore(S, snap, step)
    rb._size_t.fill_(size)
    S.noise_fn = None if eps is None else (lambda shape: eps)
    S.train_from_buffer(rb, 1)
    res = R.step_result(S)
    assert int(S._step_t) == step + 1
    return res


def _given(Rt, snap, rows, idx, eps, step=0):
    _restore(Rt, snap, step)
    ti = torch.from_numpy(np.asarray(idx, np.int64))
    return R.run_step(Rt, {k: rows[k][ti] for k in KEYS}, eps)


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32))
               for k in ("losses", "cols", "grad"))


def _assert_close(tag, tr, got, ref, widen=1.0):
    """Project tolerances (module docstring); prints the worst ratios first."""
    loss = float((np.abs(got["losses"] - ref["losses"]) / (1e-5 * np.abs(ref["losses"]) + 1e-6)).max())
    col, cname = R.grad_ratio(got["cols"].reshape(-1), ref["cols"].reshape(-1),
                              [(n, i * tr.batch_size, (i + 1) * tr.batch_size) for i, n in enumerate(R.COLS)])
    grad, gname = R.grad_ratio(got["grad"], ref["grad"], R.grad_blocks(tr))
    print(f"{tag}: loss {loss:.2f}, columns {col:.2f} ({cname}), gradient {grad:.2f} ({gname}) x tolerance (x {widen:g})")
    assert loss <= widen and col <= widen and grad <= widen, (tag, loss, col, cname, grad, gname)


@pytest.mark.gpu
@pytest.mark.parametrize("H,B", [(64, 33), (64, 100), (64, 256), (512, 45)])
def test_sampled_rows_are_the_restated_draw(H, B):
    """Normals given, rows drawn in the kernel: bitwise the step on the rows draw_batch names, at ring sizes 1, 3, 257
    and 700 (size 0 draws as size 1) and at step counters 0, 1, 7 and 2^32 + 5 (the counter's high word: another draw
    than step 5)."""
    rb, rows = _ring()
    S, Rt, snap = _pair(H, B)
    eps = torch.randn(2 * B, generator=torch.Generator().manual_seed(B)).cuda()
    hi = (1 << 32) + 5
    seen = {}
    for size, step in [(1, 7), (3, 7), (257, 7), (700, 7), (257, 0), (257, 1), (257, 5), (257, hi), (0, 7)]:
        idx, _, _ = R.draw_batch(SEED, step, B, size, CAP)
        assert idx.min() >= 0 and idx.max() < max(size, 1)
        s = _sampled(S, snap, rb, size, step, eps)
        r = _given(Rt, snap, rows, idx, eps)
        seen[(size, step)] = (idx, s)
        assert _bits_equal(s, r), f"size {size} step {step}: the sampled step is not the step on rows {idx[:8]}..."
    assert _bits_equal(seen[(0, 7)][1], seen[(1, 7)][1])
    assert not np.array_equal(seen[(257, 5)][0], seen[(257, hi)][0])
    assert not _bits_equal(seen[(257, 5)][1], seen[(257, hi)][1])
    assert len(set(seen[(700, 7)][0].tolist())) > B // 2  # (the draw spreads over the ring)


@pytest.mark.gpu
def test_sampled_rows_read_back_exactly():
    """Step 0, every terminal 1, no clip, critics zero except their last bias: q_target is fl(reward_scale · reward)
    of the drawn row, so the q_target column names the rows, in order; q1_pred is the bias."""
    from ast_sac_amd.ast_sac.torch.sac.sac_fused import FusedSACTrainer
    from test_sac import _seeded_nets
    H, B = 64, 100
    rb, rows = _ring(all_terminal=True)
    pol, qs = _seeded_nets(H, "cuda", 3)
    with torch.no_grad():
        for q in qs:
            for name, p in q.named_parameters():
                if name != "last_fc.bias":
                    p.zero_()
        qs[0].last_fc.bias.fill_(0.375)
    tr = FusedSACTrainer(env=R._Env, policy=pol, qf1=qs[0], qf2=qs[1], target_qf1=qs[2], target_qf2=qs[3],
                         reward_scale=0.75, batch_size=B, use_graph=False, backend="hip")
    tr._seed = SEED
    for size in (700, 3):
        rb._size_t.fill_(size)
        tr._step_t.fill_(0)
        tr.train_from_buffer(rb, 1)
        cols = R.step_result(tr)["cols"]
        idx, _, _ = R.draw_batch(SEED, 0, B, size, CAP)
        want = np.float32(0.75) * rows["rewards"].numpy().reshape(-1)[idx]
        assert np.array_equal(cols[2].view(np.uint32), want.view(np.uint32))
        if size == 700:
            assert np.all(cols[0] == np.float32(0.375))


@pytest.mark.gpu
@pytest.mark.parametrize("H,B", [(64, 33), (64, 256), (512, 45)])
def test_in_kernel_normals_are_the_restated_box_muller(H, B):
    """Rows and normals drawn in the kernel against R on draw_batch's rows and float32 normals, from the ring
    (train_from_buffer) and on a given batch (train_from_torch without a noise function: sampled = 0, eps = NULL)."""
    rb, rows = _ring()
    S, Rt, snap = _pair(H, B)
    for step in (0, 7):
        idx, e0, e1 = R.draw_batch(SEED, step, B, 257, CAP)
        eps = torch.from_numpy(np.concatenate([e0, e1])).cuda()
        s = _sampled(S, snap, rb, 257, step, None)
        r = _given(Rt, snap, rows, idx, eps)
        _assert_close(f"H={H} B={B} step {step} ring", S, s, r)
    # a given batch, the normals still the kernel's (the ring above bound the seed)
    given = np.arange(B)[::-1].copy()
    _restore(S, snap, 7)
    s = R.run_step(S, {k: rows[k][torch.from_numpy(given)] for k in KEYS}, None)
    r = _given(Rt, snap, rows, given, eps)
    _assert_close(f"H={H} B={B} step 7 given batch", S, s, r)


@pytest.mark.gpu
@pytest.mark.parametrize("H,B", [(64, 33), (256, 100)])
def test_chained_steps_draw_what_single_steps_draw(H, B):
    """Three consecutive chained steps of S (STAGE_NEXT | FROM_STAGED + STAGE_NEXT | FROM_STAGED: each staged batch is
    the next counter's draw) against R stepping on the restated batches, compared after every step: a free-running
    R within the project tolerance times the step number (as test_hip_sac_matches_reference_step widens), and an R
    set to S's state before each step within the tolerance itself."""
    from ast_sac_amd import sacfused
    rb, rows = _ring()
    S, Rfree, snap = _pair(H, B)
    Rsync = _trainer("hip", H, B, "cuda", seed=3)
    rb._size_t.fill_(257)
    S.train_from_buffer(rb, 1)  # binds the ring and the seed
    _restore(S, snap, 4)
    _restore(Rfree, snap, 4)
    lr = 8e-5
    flags = [sacfused.CHAIN_STAGE_NEXT, sacfused.CHAIN_FROM_STAGED | sacfused.CHAIN_STAGE_NEXT, sacfused.CHAIN_FROM_STAGED]
    for k, fl in enumerate(flags):
        step = 4 + k
        assert int(S._step_t) == step and int(Rfree._step_t) == step
        before = _snap(S)
        S._sf.set_stream()
        S._sf.grads_chain(fl)
        s = R.step_result(S)
        idx, e0, e1 = R.draw_batch(SEED, step, B, 257, CAP)
        eps = torch.from_numpy(np.concatenate([e0, e1])).cuda()
        ti = torch.from_numpy(idx)
        batch = {key: rows[key][ti] for key in KEYS}
        _assert_close(f"H={H} B={B} chain step {k} (same state)", S, s, _given(Rsync, before, rows, idx, eps, step))
        _assert_close(f"H={H} B={B} chain step {k} (free-running)", S, s, R.run_step(Rfree, batch, eps), widen=k + 1.0)
        for name in ("flat_param", "flat_target"):
            a, b = getattr(S, name).cpu().numpy(), getattr(Rfree, name).cpu().numpy()
            d = np.abs(a - b)
            assert d.max() <= 2 * lr * (k + 1) + 1e-6, (name, k, d.max())
            assert int((d > 1e-6 + 1e-5 * np.abs(b)).sum()) <= max(2, d.size // 200), (name, k)
