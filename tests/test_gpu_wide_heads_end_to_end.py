"""
-m gpu: whole iterations with the wide heads of the wide width pair (256, 512) behind PPOPolicy.fused_wide_heads -- a team of
three agents on one shared 256 / 512 policy (tests/test_gpu_k12_wide_shapes.py: _team_ppo is the model; T 10, B 48, two
epochs):

  * the rollout buffer of a Box(17) policy at O 86 (critic in_dim 258) against float64 (K6+K7's wide-head kernel inside PPO);
  * Box(17) / O 86 and Discrete(18) / O 40: rollout + train_on_rollout under hipGraph replay, and a second eager run, bitwise
    the eager run -- parameters, both moments, the buffer's values, the step counters;
  * Box(4) and Discrete(5) with the attribute on against the attribute off, bitwise: a policy with out_dim <= 8 runs the
    kernels it always ran;
  * testing.test_policy on a Box(17) policy, deterministic and sampled: one K19 launch per step, the result the restatement
    of the env's trace, the actions the torch path's within the Gaussian bound.
"""
import numpy as np
import pytest
import torch

import test_gpu_k12_width_pairs as wp
import test_gpu_policy_step_float64 as k6

ek, hd, philox = k6.ek, k6.cases.hd, k6.cases.philox

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture
def wide_heads(monkeypatch):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)


def _space(kind, n):
    from ppo_and_friends_amd.spaces import Box, Discrete
    return Box(-0.4, 0.4, (n,), np.float32) if kind == "box" else Discrete(n)


def _team_ppo(space, E, O, B, graphs=True):
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
               update_mode="fused", use_graphs=graphs, save_state=False)


def _iteration(space, E, O, B, graphs, out_dim):
    ppo = _team_ppo(space, E, O, B, graphs)
    pol = ppo.policies["team"]
    assert pol.fused_step_unsupported_reason() == ""
    ppo.rollout()
    ppo.train_on_rollout()
    torch.cuda.synchronize()
    fused = ppo._fused_updater("team", B)
    assert fused is not None and fused.wide and fused.split and fused.actor_desc.out_dim == out_dim
    assert ("fused_wide_heads" in fused.description()) == (out_dim > 8), fused.description()
    return (pol.policy_params.detach().clone(), pol.policy_exp_avg.detach().clone(), pol.policy_exp_avg_sq.detach().clone(),
            pol.buffer.values.clone(), pol.buffer.log_probs.clone(), pol.policy_step_counts.tolist())


def _assert_bitwise(what, got, ref):
    for i, name in enumerate(("parameters", "exp_avg", "exp_avg_sq", "values", "log_probs")):
        assert torch.equal(got[i], ref[i]), f"{what}: {name} differ, max |d| {float((got[i] - ref[i]).abs().max()):.3e}"
    assert got[5] == ref[5], (what, got[5], ref[5])


def test_rollout_buffer_of_a_box17_policy_against_float64(wide_heads):
    """3 agents x 5 envs = 15 rows per step: K6+K7's wide-head kernel as PPO launches it."""
    ppo = _team_ppo(_space("box", 17), 5, 86, 48)
    assert ppo.policies["team"].fused_step_unsupported_reason() == ""
    ppo.rollout()
    assert ppo.policies["team"].buffer.actions.shape[-1] == 17
    wp._buffer_against_float64(ppo, "team", (256, 512))


@pytest.mark.parametrize("kind,n,E,O", [("box", 17, 5, 86), ("discrete", 18, 16, 40)])
def test_graph_replay_and_a_second_run_are_bitwise_the_eager_run(kind, n, E, O, wide_heads):
    out_dim = n
    run = lambda graphs: _iteration(_space(kind, n), E, O, 48, graphs, out_dim)
    ref = run(False)
    assert all(bool(torch.isfinite(t).all()) for t in ref[:5])
    assert ref[5][0] == ref[5][1] > 0
    _assert_bitwise("use_graphs=True", run(True), ref)
    _assert_bitwise("the same run again", run(False), ref)


@pytest.mark.parametrize("kind,n,E,O", [("box", 17, 5, 86), ("discrete", 18, 16, 40)])
def test_two_epochs_against_the_cpu_port(kind, n, E, O, wide_heads):
    """tests/test_gpu_k12_wide_critic.py::test_mappo_shared_policy_three_agents_actor_256_critic_512 with a wide head: its
    assertions and its tolerances (each figure is printed before it is asserted).  The CPU port (oracle.cpu_ppo_loop) replays
    the recorded raw actions, trains two epochs on its own autograd graph and Adam, and is compared per epoch on the four
    status figures and at the end on the critic's parameters."""
    from oracle import cpu_ppo_loop
    from ppo_and_friends_amd.ppo import PermutationLoader
    A, T, B, seed = 3, 10, 48, 4
    ppo = _team_ppo(_space(kind, n), E, O, B)
    pol = ppo.policies["team"]
    assert pol.fused_step_unsupported_reason() == ""
    assert ppo._fused_updater("team", B) is not None, "a 256 / 512 policy with a wide head trains on the fused path"
    box = kind == "box"
    cpu = cpu_ppo_loop.CpuPPO(O, n, hidden=256, batch_size=B, seed=seed, critic_obs_dim=A * O, critic_hidden=512,
                              continuous=box, act_low=-0.4, act_high=0.4)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
    cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
    if box:
        with torch.no_grad():
            cpu.log_std.copy_(pol.actor.distribution.log_std.detach().cpu())
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    ds = ppo.rollout()
    env = ppo.env
    assert len(ds) == A * E * T
    wp._buffer_against_float64(ppo, "team", (256, 512))              # K6+K7's wide-head kernel
    recorded = pol.buffer.raw_actions if box else pol.buffer.actions[..., 0]
    ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(), actions=recorded.cpu().numpy(),
                      term_table=env.term_table.cpu().numpy(), critic_obs_table=env.critic_obs_table.cpu().numpy())
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


def test_test_policy_on_a_box17_policy(wide_heads, monkeypatch):
    """testing.test_policy, deterministic and sampled: every step of the loop is ONE ppoaf_policy_infer launch (K19's wide-head
    kernel), the result is the restatement of the env's own trace, and the deterministic actions are the torch path's for the
    same policy state within the Gaussian bound of tests/test_gpu_wide_heads_step.py (k12_bound on the float64 / float32
    restatements); the sampled actions are the restated Philox draws of every launch within the same bound."""
    import eval_restatement as R
    import test_gpu_eval_policy as ev
    from torch import nn
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.testing import test_policy
    E, N = 20, 33
    ppo = ev._synthetic_ppo(_space("box", 17), O=40, E=E, hidden=256, critic_hidden=512, depth=3, mode="fused", act=nn.Tanh)
    pol = ppo.policies["p"]
    assert pol.inference_unsupported_reason() == ""
    log, launches, inner = ev._Log(pol, monkeypatch), [], K.policy_infer
    monkeypatch.setattr(K, "policy_infer", lambda a: (launches.append((int(a.actor.out_dim), int(a.seed), int(a.offset))),
                                                      inner(a))[1])
    bounds = (np.full(17, -0.4, np.float32), np.full(17, 0.4, np.float32))
    log_std = pol.actor.distribution.log_std.detach().cpu().numpy()

    def restated(obs, dtype, draws=None):
        """The env actions of `obs` in `dtype`: tanh(mean), or tanh(mean + sd z) with the launches' Philox draws (row e of a
        launch at counter offset + e), rescaled to the bounds."""
        x = _outputs(pol, obs, dtype)
        if draws is not None:
            sd = hd.gauss_std(log_std, float(np.float32(pol.actor.distribution.min_std)), dtype)
            z = np.concatenate([hd.gauss_normals(seed, philox.counters_u64(off, np.arange(E)), 17, dtype) for _, seed, off in draws])
            x = x + sd * z
        return hd.unit_to_bounds(np.tanh(x), bounds, dtype).astype(np.float64)

    def compare(what, got, obs, draws=None):
        """The bound of tests/test_gpu_wide_heads_step.py: eval_kernels.k12_bound on the float64 and float32 restatements."""
        want, want32 = restated(obs, np.float64, draws), restated(obs, np.float32, draws)
        frac = float((np.abs(got - want) / ek.k12_bound(want, want32)).max())
        print(f"{what}: worst deviation over bound {frac:.3f}")
        assert frac <= 1.0, what

    info = test_policy(ppo, N, deterministic=True, check_every=6, max_steps=4000)
    score, done = ev._trace_arrays(ppo.env, E, ["agent0"])
    assert info == R.score_info(score, done, {"agent0": "p"}, N)
    assert len(launches) == len(log.obs) > 0 and {n for n, _, _ in launches} == {17}
    obs, act = torch.cat(log.obs), torch.cat(log.actions).double().cpu().numpy()
    assert act.shape == (obs.shape[0], 17) and np.abs(act).max() <= 0.4
    compare("K19, deterministic", act, obs)
    with torch.no_grad():
        torch_act = pol.actor.distribution.refine_prediction(pol.actor.forward_logits(obs)).double().cpu().numpy()
    compare("the torch path, deterministic", torch_act, obs)
    # sampled: the same bound, against the restated draws of every launch's (seed, offset)
    ppo.env.trace, n_det = [], len(launches)
    info = test_policy(ppo, 12, deterministic=False, check_every=6, max_steps=4000)
    score, done = ev._trace_arrays(ppo.env, E, ["agent0"])
    assert info == R.score_info(score, done, {"agent0": "p"}, 12)
    assert len(launches) == len(log.obs) > n_det
    draws = launches[n_det:]
    assert len({off for _, _, off in draws}) == len(draws)           # every step draws at counters of its own
    obs, act = torch.cat(log.obs[n_det:]), torch.cat(log.actions[n_det:]).double().cpu().numpy()
    compare("K19, sampled", act, obs, draws)


def _outputs(pol, obs, dtype):
    """The actor's outputs in `dtype` numpy from its Linear layers (test_gpu_eval_policy._logits64 in a chosen dtype)."""
    from torch import nn
    lin = [m for m in pol.actor.sequential_net.modules() if isinstance(m, nn.Linear)]
    h = obs.detach().cpu().numpy().astype(dtype)
    for l, m in enumerate(lin):
        h = h @ m.weight.detach().cpu().numpy().astype(dtype).T + m.bias.detach().cpu().numpy().astype(dtype)
        if l + 1 < len(lin):
            h = np.tanh(h)
    return h


@pytest.mark.parametrize("kind,n", [("box", 4), ("discrete", 5)])
def test_the_opt_in_changes_nothing_at_8_outputs_or_fewer(kind, n, monkeypatch):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    off = _iteration(_space(kind, n), 6, 18, 48, True, n)
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)
    _assert_bitwise("fused_wide_heads = True", _iteration(_space(kind, n), 6, 18, 48, True, n), off)
