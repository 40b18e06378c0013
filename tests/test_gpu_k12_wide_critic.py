"""
-m gpu: the wide width pair (256, 512) of K6+K7 and K12 under update_mode="fused" (csrc/ppo_update_wide.hip, the critic's
row-tile body of csrc/ppo_update_rowtile_wide.hpp), on every path such a policy takes:

  * one mini-batch against float64 (the steering, reference and per-tensor bound of tests/test_gpu_k12_gradients.py) on the one
    form the pair has -- fwd_bwd, the wgrad launch, Adam -- at the body's shape edges;
  * hipGraph replay against eager launches and the same run twice, bitwise;
  * a whole iteration against the CPU port (the shape and tolerances of
    tests/test_gpu_k12_width_pairs.py::test_mappo_shared_policy_three_agents_actor_64_critic_256);
  * the rollout buffer (K6+K7 at <16, 32>) against float64 with fewer rows than a tile and with a ragged third tile;
  * the block form of K6+K7 in a multi-policy run beside a MAT team;
  * evaluation on K19 under "fused", on the torch path under "auto".
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ppo_loop

import test_gpu_eval_policy as ev
import test_gpu_k12_gradients as g12
import test_gpu_k12_width_pairs as wp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
WIDE = dict(ha=256, hc=512)

# ---------------------------------------------------------------------------------------------------- one mini-batch
K12_CASES = {
    # ragged second tile, no hidden-to-hidden layer
    "d1_B17_in1": g12.case(O=1, depth=1, B=17, head=("categorical", 2), act="relu", seed=511, **WIDE),
    # fewer rows than lanes
    "d2_B2_in17": g12.case(O=17, depth=2, B=2, head=("gaussian", 3), act="tanh", seed=512, **WIDE),
    # the baseline depth, the panel edge (critic in_dim 64)
    "d3_B96_in64": g12.case(O=32, wide_critic=True, depth=3, B=96, head=("categorical", 5), act="leaky_relu", seed=513, **WIDE),
    # three reloads of h from the panels
    "d4_B40_in40": g12.case(O=40, depth=4, B=40, head=("gaussian", 4), act="relu", seed=514, **WIDE),
    # 32 tiles: the split chain's last B
    "d3_B512_in12": g12.case(O=12, depth=3, B=512, head=("categorical", 3), act="relu", seed=515, **WIDE),
    # loss switches
    "d2_B64_switches": g12.case(O=8, depth=2, B=64, norm_adv=False, norm_values=False, huber=False, kl=0.3, seed=516, **WIDE),
}


def run_wide(c):
    """g12.run_case on the wide pair's one form: the gradient bucket and the eight totals of gradient_only, then one full
    mini-batch from a preset optimiser state with the clip active and inactive."""
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    s = g12.Steered(c)
    pol, B, head, form = s.pol, c["B"], s.head, "wide"
    keep = [t.clone() for t in (pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq, pol.policy_step_counts)]
    pad = g12._padding(s.tables, pol.policy_params.numel())
    rng = np.random.default_rng(c["seed"] + 1)
    g = s.r64["grads"]
    rms = np.sqrt(np.mean(g * g)) + 1e-12
    m0 = np.where(pad, 0.0, 0.5 * g + rng.normal(0, 0.1 * rms, g.size)).astype(np.float32)
    v0 = np.where(pad, 0.0, g * g * rng.uniform(0.5, 2.0, g.size) + (0.1 * rms) ** 2).astype(np.float32)
    steps0 = (6, 9)
    norms = [np.sqrt((g[:s.na] ** 2).sum()), np.sqrt((g[s.na:] ** 2).sum())]
    lr = float(pol.policy_lr[0])
    upd = FusedPolicyUpdate(s.ppo, "p")
    assert upd.wide and upd.split and upd.tail_reason() != "" and upd.pairs_reason() != ""
    assert upd.slabs.numel() <= 4, "a wide pair allocates no slabs"
    # ---- the gradient of one mini-batch
    upd.begin_epoch(s.perm)
    args = upd._args_for(B)
    steps = pol.policy_step_counts.clone()
    upd.gradient_only(args)
    torch.cuda.synchronize()
    pol.policy_step_counts.copy_(steps)
    grads = pol.policy_grads.detach().double().cpu().numpy()
    assert not grads[pad].any(), "padding of the gradient bucket written"
    g12._check(form, head, "gradient", grads, s.r64["grads"], s.r32["grads"], s.tables)
    g12._check(form, head, "totals", upd.totals[:8].cpu().numpy(), s.r64["totals"], s.r32["totals"], g12.TOTALS)
    # ---- one full mini-batch from a non-zero optimiser state, clip active / inactive
    for max_norm in (0.25 * min(norms), 4.0 * max(norms)):
        pol.gradient_clip = float(np.float32(max_norm))
        pol.policy_exp_avg.copy_(torch.from_numpy(m0))
        pol.policy_exp_avg_sq.copy_(torch.from_numpy(v0))
        pol.policy_step_counts.copy_(torch.tensor(steps0))
        pol.policy_params.copy_(keep[0])
        upd.begin_epoch(s.perm)
        args = upd._args_for(B)
        upd._one(args)
        torch.cuda.synchronize()
        upd._check_persistent()
        got = [t.detach().double().cpu().numpy() for t in (pol.policy_grads, pol.policy_params, pol.policy_exp_avg,
                                                            pol.policy_exp_avg_sq)]
        mn = float(np.float32(max_norm))
        want = g12.ko.clip_adam(s.params, s.r64["grads"], m0, v0, steps0, lr, mn, s.na)
        want32 = g12.ko.clip_adam(s.params, s.r32["grads"], m0, v0, steps0, lr, mn, s.na, dtype=torch.float32)
        tag = "clip" if max_norm < min(norms) else "no clip"
        g12._check(form, head, f"{tag} gradient", got[0], s.r64["grads"], s.r32["grads"], s.tables)
        g12._check(form, head, f"{tag} step", got[1] - s.params, want[0] - s.params, want32[0] - s.params, s.tables)
        g12._check(form, head, f"{tag} m", got[2], want[1], want32[1], s.tables)
        g12._check(form, head, f"{tag} v", got[3], want[2], want32[2], s.tables)
        assert (pol.policy_step_counts.cpu().numpy() == np.array(steps0) + 1).all()
    print(f"\ndepth {c['depth']} B {B}: worst deviation / bound of the {head} cases so far {g12.WORST.get((form, head))}")


# The seed of the networks' initial weights where g12._ppo's (3) leaves kinks no redraw of the observations removes: with one
# input and zero initial biases a unit's pre-activation is w_j x, and the rule (|z| < 1e-4 max|z| of its layer) then asks for
# |w_j| >= 1e-4 max|w| of all 512 units -- a property of the draw of W_0, whatever x is.  Seeds changed, not the rule.
WEIGHT_SEEDS = {"d1_B17_in1": 5}


@pytest.mark.parametrize("name", sorted(K12_CASES))
def test_k12_minibatch_against_float64(name, monkeypatch):
    if name in WEIGHT_SEEDS:
        from ppo_and_friends_amd import ppo as ppo_module
        inner = ppo_module.PPO
        monkeypatch.setattr(ppo_module, "PPO", lambda *a, **k: inner(*a, **dict(k, random_seed=WEIGHT_SEEDS[name])))
    run_wide(K12_CASES[name])


# ---------------------------------------------------------------------------------------------------- replay, determinism
def _team_ppo(space, E, update_mode, graphs=True, widths=(256, 512)):
    """wp._team_ppo (3 agents, T 10, O 18, B 48: a ragged last mini-batch) with the graph switch."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    A, T, O, B, seed = 3, 10, 18, 48, 4
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, DEV, reward="uniform", seed=21,
                                              num_agents=A, critic_view="policy", term_prob=0.05)
    sp, csp = Box(-np.inf, np.inf, (O,), np.float32), Box(-np.inf, np.inf, (A * O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=widths[0]), critic_kw_args=dict(hidden_size=widths[1]))
    return PPO(env_gen, {"team": (None, sp, csp, space, pargs)}, device=DEV, random_seed=seed, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2,
               update_mode=update_mode, use_graphs=graphs, save_state=False)


def _iteration(graphs):
    from ppo_and_friends_amd.spaces import Discrete
    ppo = _team_ppo(Discrete(5), 6, "fused", graphs)
    ppo.rollout()
    ppo.train_on_rollout()
    torch.cuda.synchronize()
    pol = ppo.policies["team"]
    fused = ppo._fused_updater("team", 48)
    assert fused is not None and fused.wide and fused.split
    assert fused.tail_reason() != "" and fused.pairs_reason() != ""
    return (pol.policy_params.detach().clone(), pol.policy_exp_avg.detach().clone(), pol.policy_exp_avg_sq.detach().clone(),
            pol.buffer.values.clone(), pol.policy_step_counts.tolist())


def test_graph_replay_and_a_second_run_are_bitwise_the_eager_run():
    ref = _iteration(False)
    assert ref[4] == [8, 8], ref[4]                      # 180 transitions: 3 full mini-batches + one of 36, two epochs
    for what, got in (("use_graphs=True", _iteration(True)), ("the same run again", _iteration(False))):
        for i, name in enumerate(("parameters", "exp_avg", "exp_avg_sq", "values")):
            assert torch.equal(got[i], ref[i]), f"{what}: {name} differ, max |d| {float((got[i] - ref[i]).abs().max()):.3e}"
        assert got[4] == ref[4], (what, got[4], ref[4])


# ---------------------------------------------------------------------------------------------------- a whole iteration
def test_mappo_shared_policy_three_agents_actor_256_critic_512():
    """wp.test_mappo_shared_policy_three_agents_actor_64_critic_256 at 256 / 512 under "fused": its shape, its assertions and
    its tolerances, which hold at this width (each figure is printed before it is asserted)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.spaces import Discrete
    A, E, T, O, NA, B, seed = 3, 6, 10, 18, 5, 48, 4
    ppo = _team_ppo(Discrete(NA), E, "fused")
    pol = ppo.policies["team"]
    assert pol.fused_step_unsupported_reason() == ""
    assert ppo._fused_updater("team", B) is not None, "a 256 / 512 policy trains on the fused path under 'fused'"
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


# ---------------------------------------------------------------------------------------------------- K6+K7 edges
@pytest.mark.parametrize("E,space", [(5, "box"), (11, "discrete")])
def test_rollout_buffer_against_float64_at_the_tile_edges(E, space):
    """3 agents x 5 envs = 15 rows per step (fewer than a tile), Box(2); 3 x 11 = 33 rows (a ragged third tile), Discrete(5)."""
    from ppo_and_friends_amd.spaces import Box, Discrete
    sp = Box(-1.0, 1.0, (2,), np.float32) if space == "box" else Discrete(5)
    ppo = _team_ppo(sp, E, "fused")
    assert ppo.policies["team"].fused_step_unsupported_reason() == ""
    ppo.rollout()
    wp._buffer_against_float64(ppo, "team", (256, 512))


# ---------------------------------------------------------------------------------------------------- multi-policy run
def test_the_wide_member_beside_a_fused_team_runs_the_block_form():
    """Under "fused" the 256 / 512 adversary steps on the block form of K6+K7 and learns on K12 beside the MAT team; each
    equals itself alone.  (Under "auto" it stays on the torch path: tests/test_gpu_mixed_policies.py.)"""
    import mixed_policies as M
    ppo, rec = M.assert_member_equals_alone("ppo_wide+mat", DEV, "fused")
    assert ppo.policies["adversary"].fused_step_unsupported_reason() == ""
    assert ppo.policies["team"].fused_step_unsupported_reason() == ""
    assert ppo._fused_updater("adversary", M.B).wide


# ---------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("space", ["discrete", "box"])
def test_deterministic_inference_actions(space, monkeypatch):
    """get_inference_actions(obs, deterministic=True): K19 under "fused" (it dispatches on the actor's width alone), the torch
    path under "auto"; both are the actor module's arg-max / mean actions."""
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.spaces import Box, Discrete
    sp = Box(-1.0, 1.0, (2,), np.float32) if space == "box" else Discrete(5)
    launches = []
    inner = K.policy_infer
    monkeypatch.setattr(K, "policy_infer", lambda a: (launches.append(a.mode), inner(a))[1])
    obs = torch.randn(33, 18, generator=torch.Generator().manual_seed(9)).to(DEV)
    for mode in ("fused", "auto"):
        pol = _team_ppo(sp, 11, mode).policies["team"]
        assert (pol.inference_unsupported_reason() == "") == (mode == "fused"), pol.inference_unsupported_reason()
        n = len(launches)
        act = pol.get_inference_actions(obs, True)
        assert (len(launches) > n) == (mode == "fused"), "K19 under 'fused', the torch path under 'auto'"
        with torch.no_grad():
            want = pol.actor.distribution.refine_prediction(pol.actor.forward_logits(obs))
        if space == "discrete":
            greedy, near = ev._greedy_and_near(ev._logits64(pol, obs), "categorical")     # near: a tie float32 may break either way
            got = act.reshape(-1).cpu().numpy()
            assert near.mean() < 0.1
            assert not ((got != greedy) & ~near).any() and not ((got != want.reshape(-1).cpu().numpy()) & ~near).any()
        else:
            torch.testing.assert_close(act.reshape(33, -1), want.reshape(33, -1), rtol=1e-5, atol=1e-5)
