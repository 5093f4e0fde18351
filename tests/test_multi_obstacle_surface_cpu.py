"""The multi-obstacle scenario (K = 2..4 obstacle ships) above the C ABI, host side (no GPU): the runner's
--obs_ships reaches the env config, combinations shipsim_create would refuse are rejected by the parser with the
reason, and the collector runs the policy inside the env launch for every K the library supports."""
import numpy as np
import pytest
import torch

from ast_sac_amd import shipsim_abi as abi
from ast_sac_amd.ast_sac.samplers.data_collector.batched_collector import BatchedPathCollector
from ast_sac_amd.rl_env.ship_in_transit.env import config_from_args, default_args
from ast_sac_amd.run.ast_sac_runner import make_variant, parse_cli_args
from test_collector_cpu import _DevicePolicy, _Policy, _PolicyEnv, _PolicySim


def _ship_key(s):
    return (s.initial_north_position_m, s.initial_east_position_m, s.initial_yaw_angle_rad,
            s.initial_forward_speed_m_per_s, s.desired_forward_speed, s.n_route,
            tuple(s.route_north[:s.n_route]), tuple(s.route_east[:s.n_route]))


def test_obs_ships_reaches_the_config():
    args = parse_cli_args(["--obs_ships", "3"])
    assert args.n_obs_ships == 3 and make_variant(args)["n_obs_ships"] == 3
    cfg = config_from_args(args, args.machinery)
    assert cfg.n_ships == 4
    ref = abi.ast_config("sbmpc", n_obs_ships=3)
    for k, (north, east, yaw, u, ud, route) in enumerate(abi.TRAFFIC_SHIPS[:2]):
        s = cfg.ship[2 + k]
        assert _ship_key(s) == _ship_key(ref.ship[2 + k])
        assert (s.initial_north_position_m, s.initial_east_position_m) == (north, east)
        assert s.initial_yaw_angle_rad == np.deg2rad(yaw) and s.initial_forward_speed_m_per_s == u
        assert s.desired_forward_speed == ud and s.n_route == len(route)
        assert [(s.route_north[i], s.route_east[i]) for i in range(s.n_route)] == [tuple(map(float, p)) for p in route]
        # the env arguments apply to every ship of the env
        assert s.radius_of_acceptance == args.radius_of_acceptance and s.lookahead_distance == args.lookahead_distance
    # ships 0 and 1 are the scenario of record, whatever K
    one = config_from_args(parse_cli_args([]), "detailed")
    for k in (0, 1):
        assert _ship_key(cfg.ship[k]) == _ship_key(one.ship[k])


def test_defaults_keep_one_obstacle_ship():
    args = parse_cli_args([])
    assert args.n_obs_ships == 1 and make_variant(args)["n_obs_ships"] == 1
    assert config_from_args(args, args.machinery).n_ships == 2
    assert default_args().n_obs_ships == 1 and config_from_args(default_args()).n_ships == 2
    assert config_from_args(default_args(n_obs_ships=4)).n_ships == 5


@pytest.mark.parametrize("argv,word", [(["--obs_ships", "2", "--machinery", "simplified"], "machinery"),
                                       (["--obs_ships", "2", "--collav_mode", "simple"], "collav_mode"),
                                       (["--obs_ships", "5"], "obs_ships"),
                                       (["--obs_ships", "0"], "obs_ships"),
                                       (["--obs_ships", "2", "--n_envs", "0"], "n_envs")])
def test_parser_rejects_what_the_library_refuses(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse_cli_args(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err  # the reason names the option at fault


def test_parser_accepts_the_supported_multi_obstacle_modes():
    for k in (2, 3, 4):
        for collav in ("sbmpc", "none"):
            a = parse_cli_args(["--obs_ships", str(k), "--collav_mode", collav])
            assert config_from_args(a, a.machinery).n_ships == 1 + k


class _PolicySim3(_PolicySim):
    n_ships = 3  # two obstacle ships


class _PolicySim6(_PolicySim):
    n_ships = 2 + abi.MAX_OBS  # one more than the library builds


def _env(sim_cls, n):
    env = _PolicyEnv(n)
    env.sim = sim_cls(n)
    env._lb, env._ub = env.sim.cfg.action_low, env.sim.cfg.action_high
    return env


def test_collector_fuses_on_a_multi_obstacle_sim():
    from ast_sac_amd.ast_sac.data_management.replay_buffer import DeviceReplayBuffer
    N, T = 12, 4
    env = _env(_PolicySim3, N)
    coll = BatchedPathCollector(env, _Policy(), max_path_length=T, max_ticks=64, deterministic=True,
                                device_policy=_DevicePolicy(), use_graph=False, stream_tail=0)
    assert coll.fused is True
    rb = DeviceReplayBuffer(1000, 8, 1, "cpu")
    got = coll.collect(60, rb, record_paths=True)
    assert env.sim.calls > 0  # collected through the sim's run_policy
    assert got == rb.num_steps_can_sample() >= 60
    assert coll._mode == "fused"
    # the rows are the stand-in's records: action = tanh(0.01 i + 0.1 d - 0.05 ep) on obs (i, d, ep, ...)
    o, a = rb._store["observations"][:got], rb._store["actions"][:got, 0]
    want = torch.tanh(0.01 * o[:, 0].double() + 0.1 * o[:, 1].double() - 0.05 * o[:, 2].double()).float()
    assert torch.equal(a, want)


def test_collector_does_not_fuse_past_the_library_limit():
    env = _env(_PolicySim6, 4)
    coll = BatchedPathCollector(env, _Policy(), max_path_length=4, max_ticks=64, deterministic=True,
                                device_policy=_DevicePolicy(), use_graph=False, stream_tail=0)
    assert coll.fused is False


def test_recording_view_refuses_several_obstacle_ships_before_the_device():
    """The single-env recording view is two-ship ([test, obs], the recording kernels): K > 1 is a ValueError raised
    before any device env is created (so it is raised on a machine without a GPU too)."""
    from ast_sac_amd.rl_env.ship_in_transit.env import MultiShipRLEnv
    with pytest.raises(ValueError, match="one obstacle ship"):
        MultiShipRLEnv(default_args(n_obs_ships=2), record_trajectory=True)
    with pytest.raises(ValueError, match="one obstacle ship"):
        MultiShipRLEnv(cfg=abi.ast_config("sbmpc", n_obs_ships=3), record_trajectory=True)
