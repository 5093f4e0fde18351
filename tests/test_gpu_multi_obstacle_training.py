"""Training against the multi-obstacle env (K > 1 obstacle ships): the fused collector (the policy inside the K-ship
env launch, shipsim_run_policy) keeps its books exactly as with one obstacle ship, and the runner's --obs_ships
builds, collects from and trains on that env. Needs an MI355X."""
import numpy as np
import pytest
import torch

from test_gpu_policy_act import _trainer

pytestmark = pytest.mark.gpu


def test_fused_collector_rows_and_paths_follow_the_decision_log_k2():
    """test_gpu_policy_act.py::test_fused_collector_rows_and_paths_follow_the_decision_log with two obstacle ships:
    the replay rows are the policy stream's decision records with the reward scaled, the epoch paths are the
    episodes those records form — against run_policy driven by hand on a second K = 2 env."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ast_sac_amd import shipsim_abi as abi
    from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args
    from ast_sac_amd.ast_sac.env_wrapper.normalized_box_env import BatchedNormalizedBoxEnv
    from ast_sac_amd.ast_sac.samplers.data_collector.batched_collector import BatchedPathCollector
    from ast_sac_amd.ast_sac.data_management.replay_buffer import DeviceReplayBuffer
    tr, pol = _trainer(128)
    N, T, ticks, P, scale = 128, 9, 320, 8, 0.75  # (2560 ticks: long enough for whole episodes, so paths form)
    base = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc", n_obs_ships=2), N)
    assert base.sim.n_ships == 3 and base.n_obs_ships == 2
    env = BatchedNormalizedBoxEnv(base, scale)
    dp = tr.device_policy(True)
    coll = BatchedPathCollector(env, pol, max_path_length=T, max_ticks=ticks, deterministic=True, device_policy=dp,
                                use_graph=False, stream_tail=0)  # (fixed launch boundaries: compared pass by pass)
    assert coll.fused
    rb = DeviceReplayBuffer(100000, 8, 1, "cuda")
    coll._take_over()
    coll._enter("fused")
    for _ in range(P):
        coll._fused_pass(rb, True)
    coll._drain_ring()
    torch.cuda.synchronize()
    # by hand
    env2 = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc", n_obs_ships=2), N)
    sim = env2.sim
    assert sim.n_ships == 3
    sim.reset()
    cap = coll._log_cap()
    ep = torch.zeros(N, dtype=torch.int32, device="cuda")
    dec = torch.zeros(N, dtype=torch.int32, device="cuda")
    log = torch.zeros((N, cap, abi.DECLOG_COLS), dtype=torch.float64, device="cuda")
    ln = torch.zeros(N, dtype=torch.int32, device="cuda")
    rows, paths, cur = [], [], [[] for _ in range(N)]
    for _ in range(P):
        ln.zero_()
        sim.run_policy(dp.weights(), ticks, T, ep, dec, deterministic=True, log=log, log_len=ln)
        L, n = log.cpu().numpy(), ln.cpu().numpy()
        assert n.max() <= cap
        for i in range(N):
            for r in L[i, :n[i]]:
                ev = int(r[abi.DL_EVENTS])
                if not ev & abi.EV_NONFINITE:
                    rows.append((r[abi.DL_OBS0:abi.DL_OBS0 + 8].astype(np.float32), np.float32(r[abi.DL_ACTION]),
                                 np.float32(r[abi.DL_REWARD] * scale), r[abi.DL_OBS:abi.DL_OBS + 8].astype(np.float32),
                                 np.float32(bool(ev & abi.EV_TERMINAL))))
        for j in range(cap):
            for i in range(N):
                if j >= n[i]:
                    continue
                r = L[i, j]
                ev = int(r[abi.DL_EVENTS])
                if not ev & abi.EV_NONFINITE:
                    cur[i].append((r[abi.DL_REWARD] * scale, np.float32(r[abi.DL_ACTION])))
                if r[abi.DL_DONE] or ev & abi.EV_NONFINITE or r[abi.DL_DECISION] + 1 >= T:
                    if cur[i]:
                        paths.append(cur[i])
                    cur[i] = []
    n_rows = rb.num_steps_can_sample()
    print(f"\n[fused collector K=2] rows {n_rows}, paths {len(paths)}")
    assert n_rows == len(rows) > 0
    st = {k: v[:n_rows].cpu().numpy() for k, v in rb._store.items()}
    np.testing.assert_array_equal(st["observations"], np.stack([r[0] for r in rows]))
    np.testing.assert_array_equal(st["actions"][:, 0], np.array([r[1] for r in rows]))
    np.testing.assert_array_equal(st["rewards"][:, 0], np.array([r[2] for r in rows]))
    np.testing.assert_array_equal(st["next_observations"], np.stack([r[3] for r in rows]))
    np.testing.assert_array_equal(st["terminals"][:, 0], np.array([r[4] for r in rows]))
    got = list(coll.get_epoch_paths())
    assert len(got) == len(paths) > 0
    for g, p in zip(got, paths):
        np.testing.assert_array_equal(g["rewards"][:, 0], np.array([x[0] for x in p]))
        np.testing.assert_array_equal(g["actions"][:, 0], np.array([x[1] for x in p]))
    assert coll.get_diagnostics()["num steps total"] == len(rows)
    # the facade on a K-ship handle: ship 1's route, whatever K
    routes, length = env2.obstacle_routes()
    assert routes.shape == (N, abi.MAX_ROUTE, 2) and length.shape == (N,)
    assert int(length.min()) >= 2


def test_runner_trains_on_two_obstacle_ships():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ast_sac_amd.run.ast_sac_runner import parse_cli_args, make_variant, experiment_device
    args = parse_cli_args(["--obs_ships", "2", "--n_envs", "256", "--layer_size", "256", "--batch_size", "100",
                           "--num_epochs", "1", "--min_num_steps_before_training", "512",
                           "--num_expl_steps_per_train_loop", "512", "--num_eval_steps_per_epoch", "64",
                           "--do_logging", "false", "--seed", "3"])
    torch.manual_seed(3)
    np.random.seed(3)
    algo = experiment_device(make_variant(args), args, torch.device("cuda", 0))
    tr = algo.trainer
    assert algo.expl_data_collector.fused and algo.eval_data_collector.fused
    assert algo.expl_data_collector._base_env().sim.n_ships == 3
    assert algo.eval_data_collector._base_env().sim.n_ships == 3
    before = tr.flat_param.clone()
    algo.log_stats = False
    algo.train()
    torch.cuda.synchronize()
    assert algo.num_train_steps_total > 0
    assert torch.isfinite(tr.flat_param).all() and torch.isfinite(tr.flat_target).all()
    assert not torch.equal(before, tr.flat_param)
    assert int(tr._step_t.item()) == algo.num_train_steps_total


def test_facade_round_trips_the_obstacle_ship_count():
    """BatchedMultiShipRLEnv with K = 3: a pickled env comes back with K = 3 (the collectors' snapshots pickle their
    env), steps, and refuses trajectory recording (two-ship kernels) with a ValueError."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import pickle
    from ast_sac_amd import shipsim_abi as abi
    from ast_sac_amd.rl_env.ship_in_transit.env import BatchedMultiShipRLEnv, default_args
    env = BatchedMultiShipRLEnv(default_args(collav_mode="sbmpc", n_obs_ships=3), 8)
    assert env.n_obs_ships == 3 and env.sim.n_ships == 4
    env2 = pickle.loads(pickle.dumps(env))
    assert env2.n_obs_ships == 3 and env2.sim.n_ships == 4 and env2.n_envs == 8
    assert bytes(env2.cfg) == bytes(env.cfg)
    obs = env2.reset()
    assert obs.shape == (8, 8)
    o, r, d, info = env2.step(torch.zeros((8, 1), device=env2.device))
    assert o.shape == (8, 8) and torch.isfinite(o).all() and torch.isfinite(r).all()
    routes, length = env2.obstacle_routes()
    assert routes.shape == (8, abi.MAX_ROUTE, 2)
    assert int(length.min()) >= 3  # ship 1's route with the waypoint the decision just sampled
    with pytest.raises(ValueError, match="one obstacle ship"):
        env2.record_trajectories()
