"""
-m gpu: the wide width pair (256, 512) with up to 512 inputs per network and mini-batches of up to 1024 rows, behind
PPOPolicy.fused_wide_shapes -- layer-0 panels with a row stride of 256 or 512 floats (csrc/ppo_update_dev.hpp: split_xld;
their writers in csrc/ppo_update_rowtile.hpp and csrc/ppo_update_rowtile_wide.hpp) and the weight-gradient launch in passes
of 32 chunks of 16 rows (csrc/ppo_update_split.hip: split_wgrad_job):

  * one mini-batch against float64 (tests/test_gpu_k12_wide_critic.py: run_wide, with the steering, reference and per-tensor
    bound of tests/test_gpu_k12_gradients.py) at the smallest shapes at which each new piece can go wrong;
  * the rollout buffer (K6+K7 at <16, 32> with a critic in_dim of 258) against float64;
  * a whole iteration at O 86 (critic 258), B 528: hipGraph replay and a second run against eager launches, bitwise;
  * whole iterations inside the older limits with the attribute on against the attribute off, bitwise;
  * two epochs against the CPU port at O 86, B 528 (the assertions and tolerances of
    test_gpu_k12_wide_critic.py::test_mappo_shared_policy_three_agents_actor_256_critic_512).
"""
import numpy as np
import pytest
import torch

from oracle import cpu_ppo_loop

import test_gpu_k12_gradients as g12
import test_gpu_k12_wide_critic as wc
import test_gpu_k12_width_pairs as wp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
WIDE = dict(ha=256, hc=512)


@pytest.fixture
def wide_shapes(monkeypatch):
    """The opt-in, for the class, before any PPO of the test is built."""
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)


# ---------------------------------------------------------------------------------------------------- one mini-batch
K12_CASES = {
    # the first stride-256 panel; a ninth input tile with one live column
    "d1_B17_in129": g12.case(O=129, depth=1, B=17, head=("categorical", 2), act="relu", seed=711, **WIDE),
    # strides 128 (actor, 128 inputs) and 256 (critic, 256) in one launch; the critic's panel exactly full
    "d3_B96_in128x256": g12.case(O=128, wide_critic=True, depth=3, B=96, head=("categorical", 5), act="leaky_relu", seed=712, **WIDE),
    # critic stride 512 (258 inputs: a seventeenth tile with two live columns); fewer rows than lanes
    "d2_B2_in129x258": g12.case(O=129, wide_critic=True, depth=2, B=2, head=("gaussian", 3), act="tanh", seed=713, **WIDE),
    # breakout_ram at the reference's default --hist_size 2
    "d3_B128_in256": g12.case(O=256, depth=3, B=128, head=("categorical", 4), act="relu", seed=714, **WIDE),
    # the 256-wide actor's LDS edge at depth 3
    "d3_B32_in432": g12.case(O=432, depth=3, B=32, head=("categorical", 3), act="relu", seed=715, **WIDE),
    # the upper corner: 64 chunks, two full passes of the weight-gradient launch, the critic's stride-512 panel exactly full
    "d2_B1024_in256x512": g12.case(O=256, wide_critic=True, depth=2, B=1024, head=("gaussian", 4), act="relu", seed=716, **WIDE),
    # the first batch above the old limit: a second pass of one chunk with one live row
    "d1_B513_in8": g12.case(O=8, depth=1, B=513, head=("categorical", 3), act="relu", seed=717, **WIDE),
    # robot_warehouse's MAPPO shape: 63 chunks, a ragged last block
    "d3_B1000_in71x142": g12.case(O=71, wide_critic=True, depth=3, B=1000, head=("categorical", 5), act="relu", seed=718, **WIDE),
    # a second pass of exactly one full chunk
    "d3_B528_in40": g12.case(O=40, depth=3, B=528, head=("gaussian", 2), act="tanh", seed=719, **WIDE),
}

# the seed of the networks' initial weights where g12._ppo's leaves kinks no redraw of the observations removes
# (tests/test_gpu_k12_wide_critic.py: WEIGHT_SEEDS -- seeds changed, not the rule)
WEIGHT_SEEDS = {}


@pytest.mark.parametrize("name", sorted(K12_CASES))
def test_k12_minibatch_against_float64(name, monkeypatch, wide_shapes):
    if name in WEIGHT_SEEDS:
        from ppo_and_friends_amd import ppo as ppo_module
        inner = ppo_module.PPO
        monkeypatch.setattr(ppo_module, "PPO", lambda *a, **k: inner(*a, **dict(k, random_seed=WEIGHT_SEEDS[name])))
    wc.run_wide(K12_CASES[name])


# ---------------------------------------------------------------------------------------------------- a team of three
def _team_ppo(space, E, O, B, graphs=True, verbose=False):
    """wc._team_ppo (3 agents, T 10) with the observation width and the mini-batch size as arguments."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    A, T, seed = 3, 10, 4
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, DEV, reward="uniform", seed=21,
                                              num_agents=A, critic_view="policy", term_prob=0.05)
    sp, csp = Box(-np.inf, np.inf, (O,), np.float32), Box(-np.inf, np.inf, (A * O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=256), critic_kw_args=dict(hidden_size=512))
    return PPO(env_gen, {"team": (None, sp, csp, space, pargs)}, device=DEV, random_seed=seed, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2,
               update_mode="fused", use_graphs=graphs, save_state=False, verbose=verbose)


def test_rollout_buffer_against_float64_with_258_critic_inputs(wide_shapes):
    """3 agents x 5 envs = 15 rows per step, O 86, Box(2): K6+K7 at this pair above 128 inputs."""
    from ppo_and_friends_amd.spaces import Box
    ppo = _team_ppo(Box(-1.0, 1.0, (2,), np.float32), 5, 86, 48)
    assert ppo.policies["team"].fused_step_unsupported_reason() == ""
    ppo.rollout()
    assert ppo.policies["team"].buffer.critic_observations.shape[-1] == 258
    wp._buffer_against_float64(ppo, "team", (256, 512))


def _iteration(E, O, B, graphs, strides, said=""):
    from ppo_and_friends_amd.spaces import Discrete
    ppo = _team_ppo(Discrete(5), E, O, B, graphs)
    ppo.rollout()
    ppo.train_on_rollout()
    torch.cuda.synchronize()
    pol = ppo.policies["team"]
    fused = ppo._fused_updater("team", B)
    assert fused is not None and fused.wide and fused.split
    assert fused.tail_reason() != "" and fused.pairs_reason() != ""
    assert f"stride {strides[0]} (actor) / {strides[1]} (critic) floats{said}" in fused.description(), fused.description()
    return (pol.policy_params.detach().clone(), pol.policy_exp_avg.detach().clone(), pol.policy_exp_avg_sq.detach().clone(),
            pol.buffer.values.clone(), pol.policy_step_counts.tolist())


def _assert_bitwise(what, got, ref):
    for i, name in enumerate(("parameters", "exp_avg", "exp_avg_sq", "values")):
        assert torch.equal(got[i], ref[i]), f"{what}: {name} differ, max |d| {float((got[i] - ref[i]).abs().max()):.3e}"
    assert got[4] == ref[4], (what, got[4], ref[4])


def test_graph_replay_and_a_second_run_are_bitwise_the_eager_run(wide_shapes):
    """3 agents x 22 envs x 10 steps = 660 transitions at B 528: one full mini-batch (33 chunks: a second pass of one) and one
    of 132 rows.  Actor in_dim 86 (stride 128), critic in_dim 258 (stride 512)."""
    run = lambda graphs: _iteration(22, 86, 528, graphs, (128, 512), ", fused_wide_shapes")
    ref = run(False)
    assert ref[4] == [4, 4], ref[4]                      # two mini-batches, two epochs
    assert all(bool(torch.isfinite(t).all()) for t in ref[:4])
    _assert_bitwise("use_graphs=True", run(True), ref)
    _assert_bitwise("the same run again", run(False), ref)


def test_the_opt_in_changes_nothing_inside_the_older_limits(monkeypatch):
    """O 42 (critic 126, B 48): with fused_wide_inputs on, the iteration is bitwise the same with fused_wide_shapes on and off.
    O 18 (critic 54): the iteration with fused_wide_shapes on is bitwise the iteration with both attributes off."""
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    plain = _iteration(6, 18, 48, True, (64, 64))
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_inputs", True)
        inputs = _iteration(6, 42, 48, True, (64, 128), ", fused_wide_inputs")
        mp.setattr(PPOPolicy, "fused_wide_shapes", True)
        both = _iteration(6, 42, 48, True, (64, 128), ", fused_wide_shapes")
    assert both[4] == [8, 8], both[4]                    # 180 transitions: 3 full mini-batches + one of 36, two epochs
    _assert_bitwise("fused_wide_shapes = True beside fused_wide_inputs", both, inputs)
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    _assert_bitwise("fused_wide_shapes = True at 54 critic inputs", _iteration(6, 18, 48, True, (64, 64), ", fused_wide_shapes"), plain)


def test_verbose_names_the_panel_strides_and_the_attribute(wide_shapes, capsys):
    from ppo_and_friends_amd.spaces import Discrete
    ppo = _team_ppo(Discrete(5), 22, 86, 528, verbose=True)
    assert ppo._fused_updater("team", 528) is not None
    assert "layer-0 panel stride 128 (actor) / 512 (critic) floats, fused_wide_shapes\n" in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- a whole iteration
def test_mappo_shared_policy_three_agents_actor_256_critic_512_with_258_critic_inputs_and_528_rows(wide_shapes):
    """wc.test_mappo_shared_policy_three_agents_actor_256_critic_512 at O 86 (critic in_dim 258) and B 528: its assertions and
    its tolerances (each figure is printed before it is asserted)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.spaces import Discrete
    A, E, T, O, NA, B, seed = 3, 22, 10, 86, 5, 528, 4
    ppo = _team_ppo(Discrete(NA), E, O, B)
    pol = ppo.policies["team"]
    assert pol.fused_step_unsupported_reason() == ""
    assert ppo._fused_updater("team", B) is not None, "a 256 / 512 policy with 258 critic inputs and B 528 trains on the fused path"
    cpu = cpu_ppo_loop.CpuPPO(O, NA, hidden=256, batch_size=B, seed=seed, critic_obs_dim=A * O, critic_hidden=512)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
    cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    ds = ppo.rollout()
    env = ppo.env
    assert len(ds) == A * E * T
    wp._buffer_against_float64(ppo, "team", (256, 512))              # K6+K7 at <16, 32>
    ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                      actions=pol.buffer.actions[..., 0].cpu().numpy(),
                      term_table=env.term_table.cpu().numpy(),
                      critic_obs_table=env.critic_obs_table.cpu().numpy())
    tol = dict(rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(ds.critic_observations.cpu().numpy(), ref.critic_observations.numpy())
    np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
    np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    pol.train()
    flat_params = lambda net: torch.cat([p.detach().cpu().reshape(-1) for p in net.parameters()]).numpy()
    figures = []
    for ep in range(2):
        ppo._ppo_batch_train(loader, "team")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            got, want = float(ppo.status_dict["team"][k]), float(r[k])
            figures.append((ep, k, got, want, abs(got - want) / (2e-6 + 2e-5 * abs(want))))
    gp, cp = flat_params(pol.critic), flat_params(cpu.critic)
    figures.append((2, "critic parameters", 0.0, 0.0, float(np.max(np.abs(gp - cp) / (2e-5 + 1e-4 * np.abs(cp))))))
    print("\n" + "\n".join(f"epoch {e} {k:18s} fused {g: .9e} cpu {w: .9e}  |d| / bound {f:.3f}" for e, k, g, w, f in figures))
    for e, k, got, want, _ in figures[:-1]:
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6, err_msg=f"epoch {e} {k}")
    np.testing.assert_allclose(gp, cp, rtol=1e-4, atol=2e-5)
