"""shipsim_run_policy on the multi-obstacle env (K = 2..4 obstacle ships; ast_step_kernel<.., CHAIN 2, SLOTS 4 / 8>):
the policy pass inside the K > 1 env kernels. The K > 1 env itself (shipsim_step, shipsim_run_table) is pinned to the
oracle in test_gpu_multi_obstacle.py; here the policy stream is pinned to that table stream and to the PyTorch policy:
  - deterministic: rollout bookkeeping, logged actions = tanh(mean) of the torch policy on the logged observations
    (5e-6), and the logged actions replayed through run_table on a fresh K-ship handle give the same records bit for bit;
  - the log_stop contract: with a log that fills, an env stops with its next decision pending and no record is lost;
  - stochastic: every logged action is the policy's sample under the kernel's Philox4x32-10 / Box-Muller noise (2e-5).
Needs an MI355X."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.shipsim import ShipSim
from test_gpu_policy_act import _trainer
from test_gpu_run_policy import _KEEP, _check_rollout, _eps, _run

pytestmark = pytest.mark.gpu


# (collav, K, H, N): sbmpc K 2 — one ghost slot, N not a multiple of the 4 envs of a wave (partial last wave);
# sbmpc K 3 — odd K, one hidden unit per lane; sbmpc K 4 — SLOTS 8, three ghost slots, a full fc1 slice and a
# one-unit-per-lane one; none K 4 — partial last wave; none K 2 — two full fc1 slices
@pytest.mark.parametrize("collav,K,H,N", [("sbmpc", 2, 256, 190), ("sbmpc", 3, 64, 64), ("sbmpc", 4, 320, 96),
                                          ("none", 4, 128, 62), ("none", 2, 512, 64)])
def test_policy_stream_multi_deterministic(collav, K, H, N):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    tr, pol = _trainer(H)
    dp = tr.device_policy(True)
    cfg = abi.ast_config(collav, n_obs_ships=K)
    n_dec = int(cfg.max_sampling_frequency)
    max_ticks, n_calls = 96, 40
    recs, _, init = _run(cfg, N, n_calls, max_ticks,
                         lambda sim, c, ep, dec, log, ln: sim.run_policy(dp.weights(), max_ticks, n_dec, ep, dec,
                                                                         deterministic=True, log=log, log_len=ln))
    _check_rollout(recs, n_dec, init)
    n_min = min(len(r) for r in recs)
    print(f"\n[policy stream K={K} {collav} H={H} N={N}] records per env: min {n_min}, "
          f"total {sum(len(r) for r in recs)}")
    assert n_min >= 4
    # the policy: tanh(mean(obs0))
    obs0 = torch.from_numpy(np.concatenate([r[:, abi.DL_OBS0:abi.DL_OBS0 + 8] for r in recs]).astype(np.float32))
    a_log = np.concatenate([r[:, abi.DL_ACTION] for r in recs]).astype(np.float32)
    with torch.no_grad():
        ref = torch.tanh(pol(obs0.cuda()).normal_mean).squeeze(1).cpu().numpy()
    err = float(np.abs(a_log - ref).max())
    print(f"[policy stream K={K}] max |a - tanh(mean)| {err:.3e}")
    assert err < 5e-6
    # the env: the logged actions replayed through the open-loop stream of a fresh K-ship handle
    n_eps = int(max(r[:, abi.DL_EPISODE].max() for r in recs)) + 2
    table = np.zeros((n_eps, n_dec, N), np.float32)
    for i, r in enumerate(recs):
        table[r[:, abi.DL_EPISODE].astype(int), r[:, abi.DL_DECISION].astype(int), i] = \
            abi.normalized_to_scoping(r[:, abi.DL_ACTION].astype(np.float32))
    t = torch.from_numpy(table).cuda()
    rep, _, _ = _run(cfg, N, n_calls, max_ticks,
                     lambda sim, c, ep, dec, log, ln: sim.run_table(t, max_ticks, ep, dec, log=log, log_len=ln))
    for i in range(N):
        k = len(recs[i])
        assert len(rep[i]) >= k
        np.testing.assert_array_equal(rep[i][:k][:, _KEEP], recs[i][:, _KEEP], err_msg=f"{collav} K {K} env {i}")


def test_policy_stream_multi_log_full_stall():
    """The log_stop contract at K = 2, used as the collector uses it (log_len zeroed before every call, a small
    log): an env whose log is full stops for the launch with its next decision pending. Its records over the calls,
    concatenated, equal the records of the same stream run with a log that never fills (on the common prefix)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    tr, _ = _trainer(64)
    dp = tr.device_policy(True)
    cfg = abi.ast_config("sbmpc", n_obs_ships=2)
    n_dec = int(cfg.max_sampling_frequency)
    # (a decision takes about 160 ticks here: launches of 768 ticks let most envs complete the 3 the log holds)
    N, max_ticks, n_calls, cap = 64, 768, 8, 3

    def step(sim, c, ep, dec, log, ln):
        return sim.run_policy(dp.weights(), max_ticks, n_dec, ep, dec, deterministic=True, log=log, log_len=ln)

    ref, _, init = _run(cfg, N, n_calls, max_ticks, step)
    sim = ShipSim(cfg, N)
    sim.reset()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    log_len = torch.zeros(N, dtype=torch.int32, device="cuda")
    got = [[] for _ in range(N)]
    n_full = 0
    for c in range(n_calls):
        log_len.zero_()
        o = step(sim, c, ep, dec, log, log_len)
        assert int(o["ticks"].max()) <= max_ticks
        assert torch.equal(o["decisions"], log_len)
        ln = log_len.cpu().numpy()
        assert ln.max() <= cap  # a full log stops the env: nothing is counted past the capacity
        L = log.cpu().numpy()
        n_full += int((ln == cap).sum())
        for i in range(N):
            got[i].append(L[i, :ln[i]].copy())
    sim.close()
    got = [np.concatenate(g) for g in got]
    _check_rollout(got, n_dec, init)
    keep = _KEEP + [abi.DL_ACTION] + list(range(abi.DL_OBS0, abi.DL_OBS0 + 8))
    for i in range(N):
        n = min(len(got[i]), len(ref[i]))
        assert n > 0
        np.testing.assert_array_equal(got[i][:n][:, keep], ref[i][:n][:, keep], err_msg=f"env {i}")
    print(f"\n[policy stream K=2 log-full] env-launches that filled the log: {n_full} of {N * n_calls}")
    assert n_full > 0


def test_policy_stream_multi_stochastic_noise():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    H = 256
    tr, pol = _trainer(H)
    seed = 0x1234_5678_9ABC
    dp = tr.device_policy(False, seed=seed)
    cfg = abi.ast_config("sbmpc", n_obs_ships=2)
    n_dec = int(cfg.max_sampling_frequency)
    N, max_ticks, n_calls = 128, 128, 24
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")

    def step(sim, c, ep, dec, log, ln):
        o = sim.run_policy(dp.weights(), max_ticks, n_dec, ep, dec, deterministic=False, seed=seed,
                           counter=counter, log=log, log_len=ln)
        counter.add_(1)
        return o

    recs, spans, init = _run(cfg, N, n_calls, max_ticks, step)
    _check_rollout(recs, n_dec, init)
    obs0 = torch.from_numpy(np.concatenate([r[:, abi.DL_OBS0:abi.DL_OBS0 + 8] for r in recs]).astype(np.float32))
    with torch.no_grad():
        d = pol(obs0.cuda())
        mean = d.normal_mean.squeeze(1).cpu().numpy()
        std = d.normal_std.squeeze(1).cpu().numpy()
    a_log = np.concatenate([r[:, abi.DL_ACTION] for r in recs]).astype(np.float32)
    # candidate (counter, seq) of each record's draw (as test_gpu_run_policy.py): chosen in the call it completed
    # in, after the previous completion of that call (seq = completions before it), or — the first completion of a
    # call — at the start of that call (seq 0) or after the last completion of an earlier call
    row = 0
    worst = 0.0
    for i, r in enumerate(recs):
        call_of = np.zeros(len(r), int)
        done_in = []
        for c, (b, a) in enumerate(spans):
            call_of[b[i]:a[i]] = c
            done_in.append(a[i] - b[i])
        for j in range(len(r)):
            c = call_of[j]
            first = spans[c][0][i]
            cands = [(5 + c, j - first)]
            if j == first:
                cands = [(5 + c, 0)] + [(5 + cc, done_in[cc]) for cc in range(c) if done_in[cc] > 0]
            best = min(abs(float(np.tanh(np.float32(mean[row] + std[row] * _eps(np.uint64(i), ctr, seq, seed)))) -
                           float(a_log[row])) for ctr, seq in cands)
            assert best < 2e-5, (i, j, a_log[row], best)
            worst = max(worst, best)
            row += 1
    print(f"\n[policy stream K=2 stochastic] {row} draws, worst |a - sample| {worst:.3e}")
    assert row > 0
    # the actions are not deterministic ones
    assert np.abs(a_log - np.tanh(mean)).max() > 0.05
