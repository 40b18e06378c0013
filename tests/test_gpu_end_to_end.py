"""
-m gpu end-to-end parity: the product's rollout -> dataset build -> mini-batch
update (HIP kernels + torch-ROCm MLPs, hipGraph replay) against the CPU port
with the reference's loop structure (oracle/cpu_ppo_loop.py) on IDENTICAL
rollouts: same initial weights, same observations, same actions, same shuffles.

north_star tolerance: returns / advantages / losses within 1e-5 (fp32).
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ppo_loop

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from initial_weights import load_c1_weights  # noqa: E402

pytestmark = pytest.mark.gpu


def _make(E, T, B, epochs, term_prob=0.0, max_ts=200, use_graphs=True, seed=3, update_mode="auto",
          O=4, act_space=None, policy_args=None):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    act_space = Discrete(2) if act_space is None else act_space
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, act_space, T, dev, reward="uniform",
                                              seed=77, term_prob=term_prob)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"p": (None, sp, sp, act_space, policy_args or {})}, device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False,
              envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=epochs,
              max_ts_per_ep=max_ts, use_graphs=use_graphs, update_mode=update_mode)
    return ppo


def _oracle_like(ppo, B, seed=3):
    pol = ppo.policies["p"]
    cpu = cpu_ppo_loop.CpuPPO(4, 2, batch_size=B, seed=seed)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
    cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
    cpu.loader_generator = torch.Generator().manual_seed(seed)      # PPO seeds its loader with seed + rank
    return cpu


def _flat_params(net):
    return torch.cat([p.detach().cpu().reshape(-1) for p in net.parameters()]).numpy()


@pytest.mark.parametrize("term_prob,max_ts", [(0.0, 200), (0.06, 200), (0.03, 7)])
def test_rollout_and_dataset_match_cpu_port(term_prob, max_ts):
    E, T, B = 24, 40, 64
    ppo = _make(E, T, B, 1, term_prob, max_ts)
    cpu = _oracle_like(ppo, B)
    ds = ppo.rollout()
    env = ppo.env
    buf = ppo.policies["p"].buffer
    actions = buf.actions[..., 0].cpu().numpy()
    term = None if env.term_table is None else env.term_table.cpu().numpy()
    ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(), actions=actions,
                      term_table=term, max_ts_per_ep=max_ts)
    assert len(ds) == len(ref) == E * T
    tol = dict(rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(ds.observations.cpu().numpy(), ref.observations.numpy())
    np.testing.assert_array_equal(ds.actions.cpu().numpy(), ref.actions.numpy())
    np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy(), **tol)
    np.testing.assert_allclose(ds.values[torch.arange(E * T)].cpu().numpy(), ref.values.numpy(), **tol)
    np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
    np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
    np.testing.assert_array_equal(ds.ep_lens.cpu().numpy(), [ep.length for ep in ref.episodes])
    # 13-tuple contract
    item = ds[17]
    assert len(item) == 13 and item[12] == 17
    np.testing.assert_array_equal(item[1].cpu().numpy(), ref[17][1].numpy())


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_c1_config_two_full_iterations_match_cpu_port(update_mode):
    """
    BASELINE.json configs[0] (C1, the reference's own CPU-runnable case) at its exact sizes: CartPole dims,
    E=8 envs x T=128 steps per rollout (N=1024), batch 256, 10 epochs, max_ts_per_ep=200, Bernoulli(0.02)
    terminations.  Two complete iterations (rollout -> GAE / dataset -> 40 mini-batch updates each, the second
    rollout on the updated networks) against the CPU port with the reference's loop structure.
    """
    E, T, B, epochs = 8, 128, 256, 10
    ppo = _make(E, T, B, epochs, term_prob=0.02, max_ts=200, update_mode=update_mode)
    load_c1_weights(ppo)                   # the same initial weights on every host (tests/helpers/initial_weights.py)
    cpu = _oracle_like(ppo, B)
    pol = ppo.policies["p"]
    from ppo_and_friends_amd.ppo import PermutationLoader
    for it in range(2):
        ds = ppo.rollout()
        env = ppo.env
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                          actions=pol.buffer.actions[..., 0].cpu().numpy(),
                          term_table=None if env.term_table is None else env.term_table.cpu().numpy(), max_ts_per_ep=200)
        assert len(ds) == len(ref) == E * T
        tol = dict(rtol=1e-5, atol=1e-5)                                  # north_star: returns / advantages within 1e-5
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy().reshape(-1), **tol)
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator, ppo._perm_cache)   # as train_on_rollout: keeps the prefetched shuffle
        pol.train()
        for _ in range(epochs):
            ppo._ppo_batch_train(loader, "p")
            r = cpu.train_epoch()
            for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
                np.testing.assert_allclose(ppo.status_dict["p"][k], r[k], rtol=5e-5, atol=5e-6, err_msg=f"iteration {it} {k}")
        pol.clear_dataset()
    # 80 Adam steps: float32 association differences (MFMA / rocBLAS dot products vs MKL) pass through m / sqrt(v),
    # which is sign-like where v is tiny.  The statistics above hold to 5e-5 at every epoch; of the weights, all
    # but a fraction of a percent of the 33 793 per network stay within 3e-5 and none moves by more than 5e-4
    for net, ref_net in ((pol.actor, cpu.actor), (pol.critic, cpu.critic)):
        d = np.abs(_flat_params(net) - _flat_params(ref_net))
        assert d.max() < 5e-4 and np.mean(d > 3e-5) < 1e-2, (d.max(), np.mean(d > 3e-5))


@pytest.mark.parametrize("update_mode,use_graphs", [("fused", True), ("fused", False), ("torch", True), ("torch", False)])
def test_update_epochs_match_cpu_port(update_mode, use_graphs, monkeypatch):
    """Both product update paths (fused K12 kernels; torch-ROCm MLPs + K2..K11) against the CPU port.  The fused path
    runs its launch chain graph-replayed / eagerly for use_graphs True / False."""
    E, T, B, epochs = 16, 32, 64, 2
    ppo = _make(E, T, B, epochs, use_graphs=use_graphs, update_mode=update_mode)
    cpu = _oracle_like(ppo, B)
    pol = ppo.policies["p"]
    ppo.rollout()
    env = ppo.env
    cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                actions=pol.buffer.actions[..., 0].cpu().numpy())
    from ppo_and_friends_amd.ppo import PermutationLoader
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    pol.train()
    for _ in range(epochs):
        ppo._ppo_batch_train(loader, "p")
        ref = cpu.train_epoch()
        sd = ppo.status_dict["p"]
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            np.testing.assert_allclose(sd[k], ref[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(_flat_params(pol.actor), _flat_params(cpu.actor), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(_flat_params(pol.critic), _flat_params(cpu.critic), rtol=1e-4, atol=2e-5)
    # value normaliser state after 2 epochs x 8 mini-batches
    vs = ppo.value_normalizers["p"].running_stats
    np.testing.assert_allclose(vs.mean, cpu.value_stats.mean, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(vs.variance, cpu.value_stats.variance, rtol=1e-5, atol=1e-6)
    assert vs.count == cpu.value_stats.count
    # dataset.values write-back (ppo.py:2340)
    N = E * T
    np.testing.assert_allclose(pol.dataset.values[torch.arange(N)].cpu().numpy(),
                               cpu.dataset.values.numpy(), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_tail_minibatch_and_recalc_advantages(update_mode):
    """N % B != 0 exercises the tail mini-batch; recalc_advantages re-runs the scan kernel."""
    E, T, B = 10, 13, 32            # N = 130 -> 4 full batches + a tail of 2
    ppo = _make(E, T, B, 2, update_mode=update_mode)
    ppo.recalc_advantages = True
    cpu = _oracle_like(ppo, B)
    pol = ppo.policies["p"]
    ppo.rollout()
    env = ppo.env
    cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                actions=pol.buffer.actions[..., 0].cpu().numpy())
    from ppo_and_friends_amd.ppo import PermutationLoader
    from oracle import episode_info_oracle as eo
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    ppo._ppo_batch_train(loader, "p")
    ref = cpu.train_epoch()
    np.testing.assert_allclose(ppo.status_dict["p"]["critic loss"], ref["critic loss"], rtol=2e-5)
    pol.dataset.recalculate_advantages()
    # oracle: re-run the scans per episode with the written-back values
    adv = eo.recalculate_advantages(
        np.concatenate([np.asarray(ep.rewards) for ep in cpu.dataset.episodes]),
        cpu.dataset.values.numpy(), [ep.length for ep in cpu.dataset.episodes],
        [ep.ending_value for ep in cpu.dataset.episodes])
    np.testing.assert_allclose(pol.dataset.advantages.cpu().numpy(), adv, rtol=1e-4, atol=2e-5)


def test_learn_runs_two_iterations_with_graph_replay():
    ppo = _make(32, 16, 64, 2)
    ppo.save_state = False
    ppo.learn(2 * 32 * 16)
    gs = ppo.status_dict["global status"]
    assert gs["iteration"] == 2 and gs["timesteps"] == 2 * 32 * 16
    assert np.isfinite(ppo.status_dict["p"]["actor loss"])


def _state(ppo):
    pol = ppo.policies["p"]
    vs = ppo.value_normalizers["p"].running_stats
    return (pol.policy_params.detach().cpu().numpy().copy(), dict(ppo.status_dict["p"]),
            np.array([vs.mean, vs.variance, vs.count], dtype=np.float64),
            pol.buffer.values.detach().cpu().numpy().copy())


@pytest.mark.parametrize("cfg", [
    dict(O=18, act=("d", 5), B=48, hidden=64, depth=2, act_fn="leaky"),       # 3 workgroups, tail of 16
    dict(O=54, act=("d", 5), B=100, hidden=256, depth=3, act_fn="relu"),      # C4 critic width, ragged last workgroup
    dict(O=17, act=("c", 6), B=64, hidden=128, depth=3, act_fn="tanh"),       # C3 dims, tanh-Gaussian head
    dict(O=4, act=("c", 1), B=32, hidden=32, depth=1, act_fn="relu", huber=True),
])
def test_fused_update_equals_torch_update(cfg):
    """
    The fused K12 kernels against the torch-ROCm + K2..K11 path (itself checked against the
    oracle piecewise and end to end above) on widths / depths / activations / heads the CPU
    port does not cover.  Same rollout, same shuffles -> same weights, losses, normaliser state.
    """
    import torch.nn as nn
    from ppo_and_friends_amd.spaces import Box, Discrete
    from ppo_and_friends_amd.ppo import PermutationLoader
    act_fn = {"relu": nn.ReLU, "leaky": nn.LeakyReLU, "tanh": nn.Tanh}[cfg["act_fn"]]
    kind, n = cfg["act"]
    space = Discrete(n) if kind == "d" else Box(-1.0, 1.0, (n,), np.float32)
    E, T = 14, 20                      # N = 280
    results = []
    for mode in ("fused", "torch"):
        kw = dict(hidden_size=cfg["hidden"], hidden_depth=cfg["depth"], activation=act_fn())
        pargs = dict(actor_kw_args=kw, critic_kw_args=dict(kw), use_huber_loss=cfg.get("huber", False))
        ppo = _make(E, T, cfg["B"], 2, update_mode=mode, O=cfg["O"], act_space=space, policy_args=pargs,
                    use_graphs=False)
        ppo.rollout()
        pol = ppo.policies["p"]
        loader = PermutationLoader(pol.dataset, cfg["B"], ppo.loader_generator)
        pol.train()
        for _ in range(2):
            ppo._ppo_batch_train(loader, "p")
        results.append(_state(ppo))
    (w0, s0, v0, val0), (w1, s1, v1, val1) = results
    for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
        np.testing.assert_allclose(s0[k], s1[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(w0, w1, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(v0, v1, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(val0, val1, rtol=1e-4, atol=2e-5)


K12_FORMS = {"chain": {}, "three_launches": {"PPOAF_FUSED_TAIL": "0"}, "slabs": {"PPOAF_SPLIT_WGRAD": "0"}}


@pytest.mark.parametrize("k12_form", sorted(K12_FORMS))
def test_fused_update_fuzz_against_the_torch_path(k12_form, monkeypatch):
    """
    k12_form: which form of K12 the fused path takes -- the default chain (split-wgrad panels, fused tail launch; 256-wide
    networks on workgroup pairs), the same with separate weight-gradient and Adam launches, or weight-gradient slabs +
    the slab reduce (shapes a form does not cover fall back by themselves).
    Randomised shapes (hypothesis, derandomised) for K12 + K6/K7: observation widths that are not multiples of
    4 or 16, 1-8 actions of either kind, every instantiated width pair with equal actor / critic width, depth
    1-3, batch sizes with ragged last workgroups and epoch tails, terminations.  Fused kernels against the
    torch-ROCm path on the same rollout and shuffles.
    """
    import torch.nn as nn
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.spaces import Box, Discrete
    from ppo_and_friends_amd.ppo import PermutationLoader
    for k, v in K12_FORMS[k12_form].items():
        monkeypatch.setenv(k, v)

    @settings(max_examples=24 if k12_form == "chain" else 15, deadline=None, derandomize=True,
              suppress_health_check=list(HealthCheck))
    @given(O=st.integers(1, 70), kind=st.sampled_from(["d", "c"]), n=st.integers(1, 8),
           hidden=st.sampled_from([32, 64, 128, 256]), depth=st.integers(1, 4), B=st.integers(2, 300),
           E=st.integers(1, 12), T=st.integers(2, 24), act_fn=st.sampled_from([nn.ReLU, nn.LeakyReLU, nn.Tanh]),
           huber=st.booleans(), term=st.sampled_from([0.0, 0.1]))
    def run(O, kind, n, hidden, depth, B, E, T, act_fn, huber, term):
        if kind == "d" and n < 2:
            n = 2
        space = Discrete(n) if kind == "d" else Box(-1.0, 1.0, (n,), np.float32)
        results = []
        for mode in ("fused", "torch"):
            kw = dict(hidden_size=hidden, hidden_depth=depth, activation=act_fn())
            pargs = dict(actor_kw_args=kw, critic_kw_args=dict(kw), use_huber_loss=huber)
            ppo = _make(E, T, B, 1, term_prob=term, update_mode=mode, O=O, act_space=space, policy_args=pargs, use_graphs=False)
            if mode == "fused":
                assert ppo._fused_updater("p", B) is not None, "instantiated width pair"
            ppo.rollout()
            pol = ppo.policies["p"]
            loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
            pol.train()
            ppo._ppo_batch_train(loader, "p")
            results.append(_state(ppo))
        (w0, s0, v0, val0), (w1, s1, v1, val1) = results
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            np.testing.assert_allclose(s0[k], s1[k], rtol=5e-5, atol=5e-6, err_msg=k)
        np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)
        np.testing.assert_allclose(v0, v1, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(val0, val1, rtol=2e-4, atol=3e-5)

    run()


@pytest.mark.parametrize("kind,n,O,hidden", [("d", 2, 4, 128), ("d", 5, 18, 64), ("c", 6, 17, 128), ("c", 1, 3, 32)])
def test_fused_rollout_step_equals_torch_rollout(kind, n, O, hidden):
    """K6+K7 (one launch per env step) against the torch-ROCm forward + K6 sampling path: same Philox
    counters -> same actions; log-probs / values / observation rows agree; then both against the oracle
    through the dataset test above."""
    from ppo_and_friends_amd.spaces import Box, Discrete
    space = Discrete(n) if kind == "d" else Box(-2.0, 3.0, (n,), np.float32)
    kw = dict(hidden_size=hidden, hidden_depth=3 if hidden != 32 else 1)
    pargs = dict(actor_kw_args=kw, critic_kw_args=dict(kw))
    bufs = []
    for mode in ("fused", "torch"):
        ppo = _make(20, 12, 32, 1, update_mode=mode, O=O, act_space=space, policy_args=pargs)
        ppo.rollout()
        b = ppo.policies["p"].buffer
        bufs.append({k: getattr(b, k).detach().cpu().numpy().copy() for k in
                     ("observations", "critic_observations", "actions", "raw_actions", "values", "log_probs",
                      "rewards", "advantages", "rewards_to_go")})
    f, t = bufs
    np.testing.assert_array_equal(f["observations"], t["observations"])
    np.testing.assert_array_equal(f["rewards"], t["rewards"])
    if kind == "d":
        np.testing.assert_array_equal(f["actions"], t["actions"])
    else:
        np.testing.assert_allclose(f["raw_actions"], t["raw_actions"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(f["actions"], t["actions"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(f["log_probs"], t["log_probs"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(f["values"], t["values"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(f["advantages"], t["advantages"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_mappo_shared_policy_three_agents(update_mode):
    """
    SURVEY.md §8 C4 shape: 3 agents share one policy (actor 128^3 on O=18, Discrete(5); critic 256^3
    on the concatenated O_c=54 "policy" view); rows are agent-major, the dataset holds A*E*T
    transitions in the reference's completion order (ppo.py:1730-1752, 1810-1819, 1932-1938).
    """
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    A, E, T, O, NA, B, seed = 3, 6, 10, 18, 5, 48, 4
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=21,
                                              num_agents=A, critic_view="policy", term_prob=0.05)
    sp, csp = Box(-np.inf, np.inf, (O,), np.float32), Box(-np.inf, np.inf, (A * O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=128), critic_kw_args=dict(hidden_size=256))
    ppo = PPO(env_gen, {"team": (None, sp, csp, Discrete(NA), pargs)}, device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False,
              envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode=update_mode)
    pol = ppo.policies["team"]
    assert list(pol.agent_ids) == ["agent0", "agent1", "agent2"]
    cpu = cpu_ppo_loop.CpuPPO(O, NA, batch_size=B, seed=seed, critic_obs_dim=A * O, critic_hidden=256)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
    cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    ds = ppo.rollout()
    env = ppo.env
    assert len(ds) == A * E * T
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
    for _ in range(2):
        ppo._ppo_batch_train(loader, "team")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            np.testing.assert_allclose(ppo.status_dict["team"][k], r[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(_flat_params(pol.critic), _flat_params(cpu.critic), rtol=1e-4, atol=2e-5)


def test_icm_bootstrap_surprise_follows_the_reference_device():
    """Quirk Q12 is a property of the reference's CPU device (a numpy view aliases the bootstrap value tensor,
    ppo.py:1115-1141, 1926-1930); with reference_device="cuda" the ICM surprise lands in the ending reward only."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA, B, seed = 6, 12, 5, 3, 24, 9
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    got = {}
    for ref_dev in ("cpu", "cuda"):
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=33)
        ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(enable_icm=True))}, device=dev, random_seed=seed,
                  normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B,
                  epochs_per_iter=1, reference_device=ref_dev, save_state=False)
        pol = ppo.policies["p"]
        cpu = cpu_ppo_loop.CpuPPO(O, NA, batch_size=B, seed=seed, enable_icm=True)
        cpu.reference_device = ref_dev
        strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                            if k.startswith("sequential_net.")}
        cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
        cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
        cpu.icm.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
        ds = ppo.rollout()
        ref = cpu.rollout(ppo.env.obs_table.cpu().numpy(), ppo.env.reward_table.cpu().numpy(),
                          actions=pol.buffer.actions[..., 0].cpu().numpy())
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), rtol=1e-4, atol=1e-4)
        got[ref_dev] = (ds.advantages.cpu().numpy().copy(), ds.rewards_to_go.cpu().numpy().copy())
    np.testing.assert_array_equal(got["cpu"][1], got["cuda"][1])              # the ending REWARD carries the surprise either way
    assert np.abs(got["cpu"][0] - got["cuda"][0]).max() > 1e-3                # the ending VALUE only on the CPU device


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_icm_rollout_rewards_and_training_match_cpu_port(update_mode):
    """
    ICM: intrinsic rewards added per env step (K8 + torch-ROCm MLPs), the bootstrap
    "surprise" term, and the second shuffled pass that trains the ICM -- against the CPU port.
    """
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA, B, seed = 12, 16, 6, 3, 32, 8
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=31, term_prob=0.04)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(enable_icm=True))}, device=dev,
              random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=B, epochs_per_iter=1,
              update_mode=update_mode)
    pol = ppo.policies["p"]
    cpu = cpu_ppo_loop.CpuPPO(O, NA, batch_size=B, seed=seed, enable_icm=True)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
    cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
    cpu.icm.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    for it in range(2):                          # the second rollout sees a non-zero "intrinsic score avg"
        ppo._obs = None                          # restart the table-driven env, as the CPU port does
        ds = ppo.rollout()
        env = ppo.env
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                          actions=pol.buffer.actions[..., 0].cpu().numpy(),
                          term_table=env.term_table.cpu().numpy())
        np.testing.assert_allclose(ppo.status_dict["p"]["intrinsic score avg"], cpu.intrinsic_score_avg,
                                   rtol=1e-4, err_msg=f"iteration {it}")
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), rtol=1e-4, atol=1e-4)
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator, ppo._perm_cache)   # shared prefetch cache
        pol.train()
        ppo._ppo_batch_train(loader, "p")
        r = cpu.train_epoch()
        ppo._icm_batch_train(loader, "p")
        icm_ref = cpu.icm_train_epoch()
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["p"][k], r[k], rtol=5e-5, atol=5e-6, err_msg=k)
        np.testing.assert_allclose(ppo.status_dict["p"]["icm loss"], icm_ref, rtol=2e-5)
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in cpu.icm.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("update_mode,B", [("fused", 32), ("torch", 32), ("fused", 20)])
def test_mat_policy_rollout_and_update_match_cpu_port(update_mode, B):
    """
    Both update paths (K15 fused kernel; torch-ROCm modules + K9) -- B = 20 leaves a tail mini-batch and
    a partly filled 16-row tile.
    SURVEY.md §8 C5 shape: MATPolicy (3 agents, embedding 64, 1 block, 1 head, Discrete(5), critic view
    'local').  Autoregressive rollout, shared-episode dataset ([N, A, .] rows), teacher-forced evaluation,
    one optimiser over actor + critic, Huber value loss -- against oracle/mat_oracle.CpuMATPPO.
    """
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    from oracle import mat_oracle
    dev = torch.device("cuda", 0)
    A, E, T, O, NA, seed = 3, 8, 12, 18, 5, 6
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False,
              envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode=update_mode)
    pol = ppo.policies["mat"]
    assert pol.agent_grouping and sum(p.numel() for p in pol.actor_critic.parameters()) == 78058
    assert (ppo._fused_updater("mat", B) is not None) == (update_mode == "fused")
    cpu = mat_oracle.CpuMATPPO(O, NA, A, batch_size=B, seed=seed)
    cpu.ac.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor_critic.state_dict().items()},
                           strict=False)
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    ds = ppo.rollout()
    env, buf = ppo.env, pol.buffer
    assert len(ds) == E * T and ds.observations.shape == (E * T, A, O)
    order = pol.agent_slot_order()
    obs_t = env.obs_table.view(T + 1, A, E, O)[:, order].transpose(1, 2).cpu().numpy()       # [T+1,E,A,O]
    rew_t = env.reward_table.view(T, A, E)[:, order].transpose(1, 2).cpu().numpy()
    # quirk Q14: the dataset's agent axis keeps the order the policy had BEFORE this rollout's shuffle
    k = np.argsort(order)[pol._dataset_slot_order]                     # dataset slot j <- rollout slot k[j]
    ref = cpu.rollout(obs_t, rew_t, buf.actions[..., 0].cpu().numpy()[:, :, np.argsort(k)], dataset_slot_of=k)
    tol = dict(rtol=2e-5, atol=2e-5)
    np.testing.assert_array_equal(ds.observations.cpu().numpy(), ref.obs.numpy())
    np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.logp.numpy(), **tol)
    np.testing.assert_allclose(ds.values[torch.arange(E * T)].cpu().numpy(), ref.values.numpy(), **tol)
    np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rtg.numpy(), **tol)
    np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.adv.numpy(), **tol)
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    pol.train()
    for _ in range(2):
        ppo._ppo_batch_train(loader, "mat")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            np.testing.assert_allclose(ppo.status_dict["mat"][k], r[k], rtol=5e-5, atol=5e-6, err_msg=k)
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.actor_critic.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in cpu.ac.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=3e-5)


def test_mat_update_with_more_row_tiles_than_one_operand_batch(monkeypatch):
    """
    K15 with 66 row tiles per mini-batch (5 agents: 3 sequences per 16-row tile, B = 196; N = 400: two full mini-batches
    and a tail of 8): the wgrad tile's operand loop (wgrad_tile.hpp: 16 chunks per wave and trip) takes a SECOND trip on
    waves 0 and 1, which no other shape of the suite reaches.  One epoch, graphs off:
      (a) the fused path against this package's torch path on identical rollouts (the bounds of
          test_fused_mat_and_icm_paths_fuzz_against_the_torch_paths);
      (b) the fused tail against the three-launch chain: parameters, moments and the gradient bucket bitwise;
      (c) the slab form against the chain (the bounds of test_c5_mat_split_wgrad_chain_matches_the_slab_form_at_full_size).
    """
    import ctypes as C
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    A, O, NA, B, E, T, seed = 5, 7, 4, 196, 25, 16, 11
    n_mb = (E * T + B - 1) // B

    def make(mode):
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
        sp = Box(-np.inf, np.inf, (O,), np.float32)
        ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=dev, random_seed=seed, normalize_obs=False,
                  normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1,
                  update_mode=mode, use_graphs=False)
        ppo.policies["mat"].fused_step_unsupported_reason = lambda: "torch rollout forced by the test"   # identical rollouts
        return ppo

    def first_minibatch(split):
        """the first mini-batch's gradient bucket and loss totals on their own (no optimiser step)"""
        monkeypatch.setenv("PPOAF_SPLIT_WGRAD", split)
        ppo = make("fused")
        pol = ppo.policies["mat"]
        ppo.rollout()
        pol.train()
        fused = ppo._fused_updater("mat", B)
        assert fused.split == (split == "1") and fused.n_wg == 66
        perm = torch.randperm(len(pol.dataset), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        fused.begin_epoch(perm)
        args, lib, st = fused._args_for(B), _lib.load(), K.stream()
        _lib.check(lib.ppoaf_mat_update_fwd_bwd(C.byref(args), st), "mat fwd_bwd")
        _lib.check(lib.ppoaf_mat_update_reduce(C.byref(args), st), "mat reduce")
        torch.cuda.synchronize()
        return pol.actor_critic.flat_grads.clone(), fused.totals.clone(), pol.buffer.actions.clone()

    def epoch(mode, split="1", tail="1"):
        monkeypatch.setenv("PPOAF_SPLIT_WGRAD", split)
        monkeypatch.setenv("PPOAF_FUSED_TAIL", tail)
        ppo = make(mode)
        pol = ppo.policies["mat"]
        ppo.rollout()
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._ppo_batch_train(loader, "mat")
        sd = ppo.status_dict["mat"]
        opt = pol.actor_critic_optim
        fused = ppo._fused_updater("mat", B)
        assert (fused is not None) == (mode == "fused")
        if fused is not None:
            assert int(opt.step_count.item()) == n_mb and fused.n_wg == 66
            assert fused.split == (split == "1") and (fused.tail_reason() == "") == (split == "1" and tail == "1"), fused.tail_reason()
        return dict(w=pol.actor_critic.flat_params.detach().clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                    g=pol.actor_critic.flat_grads.clone(), actions=pol.buffer.actions.clone(),
                    status=[sd[k] for k in ("actor loss", "critic loss", "kl avg", "weighted entropy")])

    chain, torch_path = epoch("fused"), epoch("torch")
    three, slabs = epoch("fused", tail="0"), epoch("fused", split="0", tail="0")
    for r in (torch_path, three, slabs):
        assert torch.equal(r["actions"], chain["actions"])
    # (a)
    np.testing.assert_allclose(chain["status"], torch_path["status"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(chain["w"].cpu().numpy(), torch_path["w"].cpu().numpy(), rtol=2e-4, atol=3e-5)
    # (b)
    for k, what in (("w", "parameters"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("g", "gradient bucket of the last mini-batch")):
        assert torch.equal(chain[k], three[k]), f"{what} differ, max |d| {float((chain[k] - three[k]).abs().max()):.3e}"
    # (c)
    (g1, t1, a1), (g0, t0, a0) = first_minibatch("1"), first_minibatch("0")
    assert torch.equal(a1, a0)
    scale, d = float(g0.abs().max()), float((g1 - g0).abs().max())
    assert d <= 1e-5 * scale, f"max |dg| {d:.3e} against max |g| {scale:.3e}"
    np.testing.assert_allclose(t1.cpu().numpy(), t0.cpu().numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(chain["status"], slabs["status"], rtol=2e-4, atol=1e-4)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_mat_policy_with_icm_matches_cpu_port(update_mode, shared, tmp_path):
    """
    MATPolicy + ICM (mat_policy.py:132-176, 1012-1090; ppo.py:1219-1288, 2509-2545): per-agent ICM rows
    ((env, agent) pairs), or agent_shared_icm -- one ICM over the group's concatenated observations / actions
    in the original agent order, MultiDiscrete([n] * A) actions, one reward per env for all its agents.
    Two iterations (the second after the policy has re-shuffled its agent ids and with a non-zero
    "intrinsic score avg") against oracle/mat_oracle.CpuMATPPO.
    """
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    from oracle import mat_oracle
    dev = torch.device("cuda", 0)
    A, E, T, O, NA, B, seed = 3, 8, 12, 18, 5, 16, 6
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), dict(enable_icm=True, agent_shared_icm=shared))},
              device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
              ts_per_rollout=T, batch_size=B, epochs_per_iter=1, update_mode=update_mode)
    pol = ppo.policies["mat"]
    assert pol.icm_model.action_dtype == ("multi-discrete" if shared else "discrete")
    cpu = mat_oracle.CpuMATPPO(O, NA, A, batch_size=B, seed=seed, enable_icm=True, agent_shared_icm=shared)
    cpu.ac.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor_critic.state_dict().items()}, strict=False)
    cpu.icm.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    tol = dict(rtol=3e-5, atol=3e-5)
    for it in range(2):
        ds = ppo.rollout()
        env, buf = ppo.env, pol.buffer
        order = pol.agent_slot_order()
        obs_t = env.obs_table.view(T + 1, A, E, O)[:, order].transpose(1, 2).cpu().numpy()       # [T+1,E,A,O]
        rew_t = env.reward_table.view(T, A, E)[:, order].transpose(1, 2).cpu().numpy()
        ism_before = cpu.intrinsic_score_avg
        k = np.argsort(order)[pol._dataset_slot_order]                 # quirk Q14: dataset slot j <- rollout slot k[j]
        ref = cpu.rollout(obs_t, rew_t, buf.actions[..., 0].cpu().numpy()[:, :, np.argsort(k)], slot_order=order,
                          dataset_slot_of=k)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rtg.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.adv.numpy(), **tol)
        np.testing.assert_array_equal(ds.next_observations.cpu().numpy(), ref.next_obs.numpy())
        np.testing.assert_allclose(ppo.status_dict["mat"]["intrinsic score avg"], cpu.intrinsic_score_avg, rtol=1e-4)
        assert it == 0 or ism_before != 0.0
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._ppo_batch_train(loader, "mat")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["mat"][k], r[k], rtol=5e-5, atol=5e-6, err_msg=k)
        ppo._icm_batch_train(loader, "mat")
        icm_loss = cpu.icm_train_epoch(agent_idxs=pol.agent_idxs)
        np.testing.assert_allclose(ppo.status_dict["mat"]["icm loss"], icm_loss, rtol=5e-5)
        pol.clear_dataset()
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in cpu.icm.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=3e-5)
    # checkpoint files of the reference (mat_policy.py:898-990): actor_critic + icm networks and optimisers
    import os
    pol.save(str(tmp_path))
    d = os.path.join(str(tmp_path), "mat-policy", "latest")
    assert sorted(os.listdir(d)) == ["actor_critic_0.model", "actor_critic_optim_0", "icm_0.model", "icm_optim_0"]
    keep = pol.icm_model.flat_params.clone(), pol.icm_optim.exp_avg.clone()
    pol.icm_model.flat_params.zero_(); pol.icm_optim.exp_avg.zero_()
    pol.load(str(tmp_path))
    assert torch.equal(pol.icm_model.flat_params, keep[0]) and torch.equal(pol.icm_optim.exp_avg, keep[1])


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_filter_stack_in_the_loop(update_mode):
    """
    normalize_obs / normalize_rewards / clips around the env: two iterations of
    rollout + update against the CPU port fed with the oracle-filtered observation / reward tables
    (the synthetic env's stream does not depend on the actions, so the tables can be filtered up front;
    every rollout starts with a hard reset that is filtered -- and counted -- again, ppo.py:1580-1586).
    """
    from oracle import filter_oracle
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    E, T, B, O, seed = 16, 24, 64, 4, 3
    dev = torch.device("cuda", 0)
    raw = SyntheticFixedLengthEnv(E, O, Discrete(2), T, dev, reward="uniform", seed=77, term_prob=0.05)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(lambda: raw, {"p": (None, sp, sp, Discrete(2), {})}, device=dev, random_seed=seed,
              obs_clip=(-2.0, 2.0), reward_clip=(-1.5, 1.5), envs_per_proc=E, ts_per_rollout=T, batch_size=B,
              epochs_per_iter=1, update_mode=update_mode)          # normalisers on by default, as the reference
    cpu = _oracle_like(ppo, B)
    orc = filter_oracle.FilteredEnvOracle(1, E, O, O, True, True, (-2.0, 2.0), (-1.5, 1.5), gamma=0.99)
    obs_raw, rew_raw, term = raw.obs_table.cpu().numpy(), raw.reward_table.cpu().numpy(), raw.term_table.cpu().numpy()
    pol = ppo.policies["p"]
    for it in range(2):
        f_obs, f_rew = np.empty_like(obs_raw), np.empty_like(rew_raw)
        f_obs[0], _ = orc.filter_obs(obs_raw[0], obs_raw[0])
        for t in range(T):
            f_obs[t + 1], _, f_rew[t] = orc.filter_step(obs_raw[t + 1], obs_raw[t + 1], rew_raw[t], term[t],
                                                        np.zeros(E, bool))
        ds = ppo.rollout()
        ref = cpu.rollout(f_obs, f_rew, actions=pol.buffer.actions[..., 0].cpu().numpy(), term_table=term,
                          max_ts_per_ep=200)
        tol = dict(rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(ds.observations.cpu().numpy(), ref.observations.numpy(), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), rtol=1e-5, atol=2e-5)
        ppo.train_on_rollout()
        refs = cpu.train_epoch()
        for k in ("actor loss", "critic loss"):
            np.testing.assert_allclose(ppo.status_dict["p"][k], refs[k], rtol=5e-5, atol=5e-6, err_msg=k)


@pytest.mark.parametrize("case", [
    dict(kind="d", NA=3, O=6, H=128, E=12, T=16, B=40),                      # 4 full mini-batches + a tail of 32
    dict(kind="c", NA=6, O=17, H=128, E=12, T=16, B=64),
    dict(kind="d", NA=5, O=18, H=64, E=8, T=12, B=32, d_inv=3, d_fwd=1),
    dict(kind="c", NA=2, O=3, H=64, E=16, T=64, B=16, graphs=True),          # 64 mini-batches: two graph chunks
    # 33 row tiles: the wgrad tile's operand loop (wgrad_tile.hpp, 8 chunks per wave and trip) takes a third trip on waves
    # 0 and 1 of the encoder jobs (66 chunks over both streams) and a second on wave 0 of the model jobs; tail of 32
    dict(kind="d", NA=3, O=6, H=64, E=34, T=32, B=528),
])
@pytest.mark.parametrize("form", ["split", "slabs"])
def test_fused_icm_update_matches_oracle(case, form, monkeypatch):
    """
    K14 (fused ICM mini-batch update: encoder x2, inverse + forward model, both losses, backward, weight
    gradients, Adam) against the torch-CPU ICM of oracle/icm_oracle.py trained on the same mini-batches.
    `split` = the split-wgrad chain (default: panels + icm_wgrad_kernel), `slabs` = per-tile slabs + slab reduce.
    """
    monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "1" if form == "split" else "0")
    from oracle import icm_oracle
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    c = dict(d_inv=2, d_fwd=2, graphs=False); c.update(case)
    E, T, O, NA, B, H = c["E"], c["T"], c["O"], c["NA"], c["B"], c["H"]
    space = Discrete(NA) if c["kind"] == "d" else Box(-1.0, 1.0, (NA,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=5, term_prob=0.05)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    icm_kw = dict(encoded_obs_dim=H, encoder_hidden_size=H, inverse_hidden_size=H, forward_hidden_size=H,
                  inverse_hidden_depth=c["d_inv"], forward_hidden_depth=c["d_fwd"])
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(enable_icm=True, icm_kw_args=icm_kw))}, device=dev,
              random_seed=4, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=B, epochs_per_iter=1, use_graphs=c["graphs"])
    pol = ppo.policies["p"]
    assert FusedIcmUpdate.unsupported_reason(pol) == ""
    ref = icm_oracle.ICM(O, NA, discrete=c["kind"] == "d", enc=H, hidden=H, depth=c["d_inv"])
    if c["d_fwd"] != c["d_inv"]:
        ref.forward_model.sequential_net = cpu_ppo_loop.make_mlp(H + NA, H, H, c["d_fwd"], out_gain=1.0)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    opt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-5)
    ppo.rollout()
    buf = pol.buffer
    N = E * T
    rm = buf.row_map.cpu().long()
    flat = lambda t: t.reshape((N,) + tuple(t.shape[2:])).cpu()[rm]
    obs, nxt, act = flat(buf.observations), flat(buf.next_observations), flat(buf.actions)
    fused = FusedIcmUpdate(ppo, "p")
    g = torch.Generator().manual_seed(9)
    for epoch in range(2):
        perm = torch.randperm(N, generator=g)
        fused.begin_epoch(perm.to(dev))
        fused.run_epoch()
        t = fused.end_epoch()
        tot, cnt = 0.0, 0
        for o in range(0, N, B):
            idx = perm[o:o + B]
            _, inv_loss, f_loss = ref(obs[idx], nxt[idx], act[idx])
            loss = (1.0 - pol.icm_beta) * f_loss + pol.icm_beta * inv_loss
            opt.zero_grad(); loss.backward(); opt.step()
            tot += float(loss); cnt += 1
        assert t[1] == cnt
        np.testing.assert_allclose(t[0] / cnt, tot / cnt, rtol=2e-5, err_msg=f"icm loss, epoch {epoch}")
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=1e-4, atol=2e-5)
    assert int(pol.icm_optim.step_count.item()) == 2 * cnt


@pytest.mark.parametrize("S,max_ts,term_prob", [(4, 7, 0.05), (1, 200, 0.0), (5, 200, 0.08)])
def test_lstm_policy_rollout_windows_and_update_match_cpu_port(S, max_ts, term_prob):
    """
    SURVEY.md §8(f).3 / a20: LSTM actor + critic (torch-ROCm nn.LSTM), hidden states logged per step,
    sequence-window dataset with terminal masks, hidden-state hand-over and write-back in the update --
    against oracle/lstm_oracle.CpuLSTMPPO (the reference's list-based flow on torch-CPU).
    """
    from oracle import lstm_oracle
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA, B, seed, H = 6, 20, 5, 3, 16, 2, 32
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=13, term_prob=term_prob)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    net_kw = dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=H)
    ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(ac_network=LSTMNetwork, actor_kw_args=net_kw,
                                                             critic_kw_args=net_kw))},
              device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
              ts_per_rollout=T, batch_size=B, epochs_per_iter=1, max_ts_per_ep=max_ts)
    pol = ppo.policies["p"]
    assert pol.using_lstm
    cpu = lstm_oracle.CpuLSTMPPO(O, NA, sequence_length=S, lstm_hidden=H, ff_hidden=H, batch_size=B, seed=seed)
    cpu.actor.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor.state_dict().items()})
    cpu.critic.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.critic.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    for it in range(2):
        ds = ppo.rollout()
        env = ppo.env
        term = None if env.term_table is None else env.term_table.cpu().numpy()
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                          pol.buffer.actions[..., 0].cpu().numpy(), term, max_ts_per_ep=max_ts)
        assert len(ds) == len(ref) == E * T - (S - 1)
        tol = dict(rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy().reshape(-1), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(), **tol)
        np.testing.assert_allclose(ds.critic_cell[torch.arange(E * T)].cpu().numpy(), ref.critic_cell.numpy(), **tol)
        for i in (0, 7, len(ds) - 1):                        # 13-tuple items: windows, masks, last-position fields
            got, want = ds[i], ref[i]
            np.testing.assert_allclose(got[0].cpu().numpy(), want[0].numpy(), **tol)     # critic obs window
            np.testing.assert_allclose(got[1].cpu().numpy(), want[1].numpy(), **tol)     # masked obs window
            assert got[12] == want[10]
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator, ppo._perm_cache)
        pol.train()
        ppo._ppo_batch_train(loader, "p")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["p"][k], r[k], rtol=1e-4, atol=1e-5, err_msg=f"{k} it={it}")
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(),
                                   rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(_flat_params(pol.actor), _flat_params(cpu.actor), rtol=2e-4, atol=5e-5)
    np.testing.assert_allclose(_flat_params(pol.critic), _flat_params(cpu.critic), rtol=2e-4, atol=5e-5)


def test_learn_writes_the_reference_state_layout_and_resumes(tmp_path):
    """
    SURVEY.md §8(f).2/4: learn() saves `latest`, `<policy>_best`, numbered tags, env_info statistics,
    state_0.pickle and the curve files in the reference's layout (ppo.py:2144-2161, 2569-2618, 2723-2851);
    a new PPO with load_state=True continues from them.
    """
    import os
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA, B = 8, 16, 5, 3, 32
    sp = Box(-np.inf, np.inf, (O,), np.float32)

    def make(load):
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=3, term_prob=0.05)
        return PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(enable_icm=True))}, device=dev, random_seed=1,
                   obs_clip=(-5.0, 5.0), reward_clip=(-5.0, 5.0), envs_per_proc=E, ts_per_rollout=T, batch_size=B,
                   epochs_per_iter=1, state_path=str(tmp_path), load_state=load, save_train_scores=True,
                   save_avg_ep_len=True, save_running_time=True, save_bs_info=True, checkpoint_every=1)

    ppo = make(False)
    ppo.learn(2 * E * T)
    root = str(tmp_path)
    for tag in ("latest", "p_best", "0", "1"):
        d = os.path.join(root, "p-policy", tag)
        for f in ("actor_0.model", "critic_0.model", "icm_0.model", "actor_optim_0", "critic_optim_0", "icm_optim_0"):
            assert os.path.exists(os.path.join(d, f)), (tag, f)
        for f in ("ActorRunningObsStats_0.pickle", "CriticRunningObsStats_0.pickle", "RunningRewardsStats_0.pickle",
                  "p-value_normalizer_stats_0.pickle"):
            assert os.path.exists(os.path.join(root, "env_info", tag, f)), (tag, f)
    assert os.path.exists(os.path.join(root, "state_0.pickle"))
    curve = np.loadtxt(os.path.join(root, "curves", "scores", "p_scores.npy"))
    assert curve.shape == (2, 2) and curve[0, 0] == 0 and curve[1, 0] == E * T
    for sub, f in (("episode_length", "average_episode.npy"), ("runtime", "running_time.npy"), ("bs_avg", "p_bs_avg.npy")):
        assert os.path.exists(os.path.join(root, "curves", sub, f))
    # reference-side readers: torch.load of a state_dict with its module keys; Adam.load_state_dict
    sd = torch.load(os.path.join(root, "p-policy", "latest", "actor_0.model"))
    assert list(sd.keys())[0] == "sequential_net.0.weight"
    ref_actor = cpu_ppo_loop.make_mlp(O, NA, out_gain=0.01)
    torch.optim.Adam(ref_actor.parameters(), eps=1e-5).load_state_dict(
        torch.load(os.path.join(root, "p-policy", "latest", "actor_optim_0"), weights_only=False))
    # `latest` is written after the rollout and before the update of the same iteration (ppo.py:2153):
    # take a final snapshot so the resumed object can be compared with the live one
    ppo.save()
    resumed = make(True)
    a, b = ppo.policies["p"], resumed.policies["p"]
    assert torch.equal(a.policy_params, b.policy_params) and torch.equal(a.icm_model.flat_params, b.icm_model.flat_params)
    assert torch.equal(a.policy_exp_avg, b.policy_exp_avg) and torch.equal(a.icm_optim.exp_avg_sq, b.icm_optim.exp_avg_sq)
    assert int(a.icm_optim.step_count.item()) == int(b.icm_optim.step_count.item()) > 0
    va, vb = ppo.value_normalizers["p"].running_stats, resumed.value_normalizers["p"].running_stats
    assert np.array_equal(va.mean, vb.mean) and va.count == vb.count
    assert resumed.status_dict["global status"]["timesteps"] == 2 * E * T
    assert resumed.status_dict["global status"]["iteration"] == 2
    ra, rb = ppo.env.running_stats["agent0"], resumed.env.running_stats["agent0"]     # RewardNormalizer under the clipper (attribute forwarding)
    assert ra == rb
    # direct_load_policy (ppo.py:2664-2686): networks from an explicit `<state>/<name>-policy/<tag>` directory
    fresh = make(False)
    assert not torch.equal(fresh.policies["p"].policy_params, a.policy_params)
    fresh.direct_load_policy("p", os.path.join(root, "p-policy", "latest"))
    assert torch.equal(fresh.policies["p"].policy_params, a.policy_params)
    assert torch.equal(fresh.policies["p"].icm_model.flat_params, a.icm_model.flat_params)
    assert np.array_equal(fresh.value_normalizers["p"].running_stats.mean, va.mean)


def test_policy_step_and_reset_constraints_are_applied():
    """ppo.py:1468-1532, ppo_policy.py:1114-1151: a policy may alter what the environment returns."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA = 8, 16, 5, 3
    sp = Box(-np.inf, np.inf, (O,), np.float32)

    # policies/utils.py:45-52 admits exactly PPOPolicy / MATPolicy (no subclasses), as the reference does:
    # the hooks are exercised by patching a built policy, the way MATPolicy switches its own on
    def run(constrained):
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=3)
        ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), {})}, device=dev, random_seed=1, normalize_obs=False,
                  normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=32, epochs_per_iter=1)
        pol = ppo.policies["p"]
        pol.calls = [0, 0]
        if constrained:
            def step(obs, critic_obs, reward, terminated, truncated, info):
                pol.calls[0] += 1
                return obs, critic_obs, reward * 2.0, terminated, truncated, info

            def reset(obs, critic_obs):
                pol.calls[1] += 1
                return obs, critic_obs
            pol.apply_step_constraints, pol.apply_reset_constraints = step, reset
            pol.have_step_constraints = pol.have_reset_constraints = True
            ppo.have_policy_step_constraints = ppo.have_policy_reset_constraints = True
        ppo.rollout()
        return ppo

    plain, con = run(False), run(True)
    assert not plain.have_policy_step_constraints and plain.policies["p"].calls == [0, 0]
    assert con.policies["p"].calls == [T, 1]
    torch.testing.assert_close(con.policies["p"].buffer.rewards, 2.0 * plain.policies["p"].buffer.rewards)


def test_rollout_statistics_in_status_dict():
    """The statistics block of the rollout on a live buffer, against the literal loop of the oracle."""
    from oracle.rollout_stats_oracle import rollout_statistics_loop
    E, T = 10, 24
    ppo = _make(E, T, 32, 1, term_prob=0.06, max_ts=9)
    ppo.rollout()
    buf, env = ppo.policies["p"].buffer, ppo.env
    ek = buf.end_kind.cpu().numpy()
    r = buf.rewards.double().cpu().numpy()
    obs_after = np.concatenate([buf.observations[1:].cpu().numpy(), ppo._obs[0].cpu().numpy()[None]], axis=0)
    want = rollout_statistics_loop(r, env.reward_table.double().cpu().numpy(), np.zeros_like(r),
                                   obs_after.min(axis=(1, 2)), obs_after.max(axis=(1, 2)), ek == 1, ek == 2,
                                   buf.boot_reward.double().cpu().numpy())
    sd, gs = ppo.status_dict["p"], ppo.status_dict["global status"]
    for k in ("score avg", "natural score avg", "top score", "reward range", "natural reward range", "obs range",
              "bootstrap range", "bootstrap avg"):
        np.testing.assert_allclose(sd[k], want[k], rtol=1e-6, atol=1e-6, err_msg=k)
    for k in ("total episodes", "longest episode", "shortest episode", "average episode"):
        np.testing.assert_allclose(gs[k], want[k], rtol=1e-9, err_msg=k)
    assert gs["timesteps"] == E * T


def test_cartpole_learns_like_the_reference_gate():
    """
    The reference's only quantitative gate (test/tests/train/test_gymnasium.py:3-49: CartPole reaches a score
    of 200 within 70 000 timesteps) on the batched device CartPole, with the runner's settings
    (baselines/gymnasium/cart_pole.py: LeakyReLU, lr 2e-3, batch 256, max_ts_per_ep 32, obs / reward
    normalisers and +-10 clips).  Exercises truncation + termination ends, bootstrapped cuts, the filter stack,
    the fused rollout step and update, and the statistics block in one run.
    """
    import torch.nn as nn
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv
    from ppo_and_friends_amd.spaces import Discrete
    dev = torch.device("cuda", 0)
    E = 16
    env_gen = lambda: BatchedCartPoleEnv(E, dev, seed=0)
    probe = env_gen()
    act = dict(activation=nn.LeakyReLU())
    ppo = PPO(env_gen, {"p": (None, probe.observation_space, probe.observation_space, Discrete(2),
                              dict(lr=2e-3, actor_kw_args=act, critic_kw_args=dict(act)))},
              device=dev, random_seed=2, envs_per_proc=E, ts_per_rollout=256, max_ts_per_ep=32, batch_size=256,
              obs_clip=(-10.0, 10.0), reward_clip=(-10.0, 10.0), normalize_obs=True, normalize_rewards=True,
              save_state=False)
    best = 0.0
    while ppo.status_dict["global status"]["timesteps"] < 70000 and best < 195.0:
        ppo.learn(E * 256)
        best = max(best, ppo.status_dict["p"]["natural score avg"])
    assert best >= 195.0, f"best natural score avg {best:.1f} after {ppo.status_dict['global status']['timesteps']} steps"


def test_overlapped_ppo_and_icm_epochs_equal_the_sequential_order():
    """PPO + ICM epochs on two streams (ppo.py:_ppo_icm_epoch_overlapped) vs one after the other: bitwise equal."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    dev = torch.device("cuda", 0)
    E, T, O, B = 32, 64, 17, 64
    space = Box(-1.0, 1.0, (6,), np.float32)
    sp = Box(-np.inf, np.inf, (O,), np.float32)

    def run(overlap):
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=3, term_prob=0.02)
        ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(enable_icm=True))}, device=dev, random_seed=5,
                  envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=3, save_state=False)
        ppo.overlap_icm = overlap
        ppo.learn(2 * E * T)
        pol = ppo.policies["p"]
        return (pol.policy_params.clone(), pol.icm_model.flat_params.clone(), dict(ppo.status_dict["p"]))

    a, b = run(True), run(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in ("actor loss", "critic loss", "kl avg", "icm loss", "intrinsic score avg"):
        assert a[2][k] == b[2][k], k


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_two_policies_in_one_run_match_two_cpu_ports(update_mode):
    """
    `policy_mapping_fn` with two policies (independent PPO, ppo.py:329-345,710-858): each policy sees only its
    agent's rows of the env, logs into its own buffer and is updated from its own dataset; the loaders draw
    from the one shuffle generator in the reference's order (policy by policy).  Against one CPU port per
    policy on that agent's observation / reward tables.
    """
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    A, E, T, O, NA, B, seed = 2, 12, 20, 5, 3, 32, 4
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=21, term_prob=0.04,
                                              num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    settings = {"p0": (None, sp, sp, Discrete(NA), {}), "p1": (None, sp, sp, Discrete(NA), dict(lr=1e-3))}
    ppo = PPO(env_gen, settings, policy_mapping_fn=lambda agent_id: "p0" if agent_id == "agent0" else "p1",
              device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
              ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode=update_mode, save_state=False)
    assert [list(p.agent_ids) for p in ppo.policies.values()] == [["agent0"], ["agent1"]]
    gen = torch.Generator().manual_seed(seed)                    # ONE shuffle stream for both policies
    cpus = {}
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    for pid, lr in (("p0", 3e-4), ("p1", 1e-3)):
        cpu = cpu_ppo_loop.CpuPPO(O, NA, batch_size=B, seed=seed, lr=lr)
        cpu.actor.load_state_dict(strip(ppo.policies[pid].actor.state_dict()))
        cpu.critic.load_state_dict(strip(ppo.policies[pid].critic.state_dict()))
        cpu.loader_generator = gen
        cpus[pid] = cpu
    datasets = ppo.rollout()
    env = ppo.env
    obs_t = env.obs_table.view(T + 1, A, E, O).cpu().numpy()
    rew_t = env.reward_table.view(T, A, E).cpu().numpy()
    term_t = env.term_table.view(T, A, E).cpu().numpy()
    tol = dict(rtol=1e-5, atol=1e-5)
    for a, pid in enumerate(("p0", "p1")):
        ds, pol = datasets[pid], ppo.policies[pid]
        ref = cpus[pid].rollout(obs_t[:, a], rew_t[:, a], actions=pol.buffer.actions[..., 0].cpu().numpy(),
                                term_table=term_t[:, a], max_ts_per_ep=200)
        assert len(ds) == len(ref) == E * T
        np.testing.assert_array_equal(ds.observations.cpu().numpy(), ref.observations.numpy())
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy(), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
    assert ppo.status_dict["global status"]["timesteps"] == E * T
    assert ppo.status_dict["global status"]["total episodes"] > 0
    ppo.train_on_rollout()                                       # p0: 2 epochs, then p1: 2 epochs
    for pid in ("p0", "p1"):
        for _ in range(2):
            r = cpus[pid].train_epoch()
        sd = ppo.status_dict[pid]
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(sd[k], r[k], rtol=5e-5, atol=5e-6, err_msg=f"{pid} {k}")
        np.testing.assert_allclose(_flat_params(ppo.policies[pid].actor), _flat_params(cpus[pid].actor), rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(_flat_params(ppo.policies[pid].critic), _flat_params(cpus[pid].critic), rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("update_mode", ["fused", "torch"])
def test_two_policies_with_different_spaces_match_two_cpu_ports(update_mode):
    """
    The shape of the reference's mixed multi-policy baselines (an adversary and a team with their own
    observation / action spaces, e.g. baselines/pettingzoo/mpe_simple_adversary.py): the env hands over dicts
    keyed by agent id (ppo_env_wrappers.py:1075-1156), `policy_mapping_fn` splits them, the two-agent team
    shares one policy (agent-major rows).  Against one CPU port per policy on its agents' tables.
    """
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, B, seed = 10, 16, 32, 8
    specs = [("adversary_0", 8, Discrete(5)), ("agent_0", 10, Discrete(3)), ("agent_1", 10, Discrete(3))]
    env_gen = lambda: SyntheticMixedAgentsEnv(E, specs, T, dev, reward="uniform", seed=33, term_prob=0.05)
    box = lambda n: Box(-np.inf, np.inf, (n,), np.float32)
    settings = {"adversary": (None, box(8), box(8), Discrete(5), {}),
                "team": (None, box(10), box(10), Discrete(3), dict(lr=1e-3))}
    ppo = PPO(env_gen, settings, policy_mapping_fn=lambda a: "adversary" if a.startswith("adversary") else "team",
              device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
              ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode=update_mode, save_state=False)
    assert [list(p.agent_ids) for p in ppo.policies.values()] == [["adversary_0"], ["agent_0", "agent_1"]]
    gen = torch.Generator().manual_seed(seed)                    # ONE shuffle stream for both policies
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpus = {}
    for pid, O, NA, lr in (("adversary", 8, 5, 3e-4), ("team", 10, 3, 1e-3)):
        cpu = cpu_ppo_loop.CpuPPO(O, NA, batch_size=B, seed=seed, lr=lr)
        cpu.actor.load_state_dict(strip(ppo.policies[pid].actor.state_dict()))
        cpu.critic.load_state_dict(strip(ppo.policies[pid].critic.state_dict()))
        cpu.loader_generator = gen
        cpus[pid] = cpu
    datasets = ppo.rollout()
    env = ppo.env
    tol = dict(rtol=1e-5, atol=1e-5)
    term = env.term_table.cpu().numpy()
    for pid, agents in (("adversary", ["adversary_0"]), ("team", ["agent_0", "agent_1"])):
        ds, pol = datasets[pid], ppo.policies[pid]
        obs_t = np.concatenate([env.obs_table[a].cpu().numpy() for a in agents], axis=1)       # agent-major columns
        rew_t = np.concatenate([env.reward_table[a].cpu().numpy() for a in agents], axis=1)
        ref = cpus[pid].rollout(obs_t, rew_t, actions=pol.buffer.actions[..., 0].cpu().numpy(),
                                term_table=np.tile(term, (1, len(agents))), max_ts_per_ep=200)
        assert len(ds) == len(ref) == len(agents) * E * T
        np.testing.assert_array_equal(ds.observations.cpu().numpy(), ref.observations.numpy())
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy(), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
    assert ppo.status_dict["global status"]["timesteps"] == E * T
    ppo.train_on_rollout()                                       # adversary: 2 epochs, then team: 2 epochs
    for pid in ("adversary", "team"):
        for _ in range(2):
            r = cpus[pid].train_epoch()
        sd = ppo.status_dict[pid]
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(sd[k], r[k], rtol=5e-5, atol=5e-6, err_msg=f"{pid} {k}")
        np.testing.assert_allclose(_flat_params(ppo.policies[pid].actor), _flat_params(cpus[pid].actor), rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(_flat_params(ppo.policies[pid].critic), _flat_params(cpus[pid].critic), rtol=1e-4, atol=2e-5)


def test_fused_mat_and_icm_paths_fuzz_against_the_torch_paths():
    """
    Randomised shapes (hypothesis, derandomised) for the other two fused chains, each against this package's
    torch-ROCm path on the same rollout and shuffles (those paths are the ones checked against the oracles):
    K15 / K16 (MATPolicy: 2-5 agents, observation 1-32, 2-8 actions, batch sizes that are not multiples of the
    sequences per tile, epoch tails) and K14 (ICM: discrete / continuous, widths 64 / 128, depths 1-3).
    """
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)

    @settings(max_examples=10, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(A=st.integers(2, 5), O=st.integers(1, 32), NA=st.integers(2, 8), E=st.integers(1, 9), T=st.integers(2, 14),
           B=st.integers(2, 40), seed=st.integers(0, 50))
    def mat(A, O, NA, E, T, B, seed):
        def make(mode):
            env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
            sp = Box(-np.inf, np.inf, (O,), np.float32)
            return PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=dev, random_seed=seed, normalize_obs=False,
                       normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1,
                       update_mode=mode, use_graphs=False)
        # K16: the rollout kernel's log-probs / values against the torch modules, teacher-forced on its own actions
        ppo = make("fused")
        pol = ppo.policies["mat"]
        assert pol.fused_step_unsupported_reason() == ""
        ppo.rollout()
        buf = pol.buffer
        flat = lambda x: x.reshape((T * E,) + tuple(x.shape[2:]))
        # quirk Q14: the buffer's agent axis is in the dataset's (pre-shuffle) order; the teacher-forced check needs
        # the order the rollout ran in (dataset slot j <- rollout slot k[j])
        k = torch.as_tensor(np.argsort(np.argsort(pol.agent_slot_order())[pol._dataset_slot_order]), device=dev)
        ro = lambda x: flat(x).index_select(1, k)
        with torch.no_grad():
            v, lp, _ = pol.evaluate(ro(buf.critic_observations), ro(buf.observations), ro(buf.raw_actions))
        np.testing.assert_allclose(ro(buf.log_probs).cpu().numpy(), lp.reshape(T * E, A).cpu().numpy(), rtol=3e-5, atol=3e-5)
        vn = ppo.value_normalizers["mat"]
        np.testing.assert_allclose(ro(buf.values).cpu().numpy(), vn.denormalize(v.reshape(T * E, A)).cpu().numpy(),
                                   rtol=3e-5, atol=3e-5)
        # K15: the fused update against the torch update on IDENTICAL rollouts (both sampled by the torch rollout,
        # whose Philox draws differ from K16's one-launch sampler)
        res = []
        for mode in ("fused", "torch"):
            ppo = make(mode)
            pol = ppo.policies["mat"]
            assert (ppo._fused_updater("mat", B) is not None) == (mode == "fused")
            pol.fused_step_unsupported_reason = lambda: "torch rollout forced by the test"
            ppo.rollout()
            loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
            pol.train()
            ppo._ppo_batch_train(loader, "mat")
            sd = ppo.status_dict["mat"]
            res.append((pol.actor_critic.flat_params.detach().cpu().numpy().copy(), pol.buffer.actions.cpu().numpy().copy(),
                        [sd[k] for k in ("actor loss", "critic loss", "kl avg", "weighted entropy")]))
        (w0, a0, s0), (w1, a1, s1) = res
        np.testing.assert_array_equal(a0, a1)
        np.testing.assert_allclose(s0, s1, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)

    @settings(max_examples=10, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(kind=st.sampled_from(["d", "c"]), NA=st.integers(2, 8), O=st.integers(1, 60), H=st.sampled_from([64, 128]),
           d_inv=st.integers(1, 3), d_fwd=st.integers(1, 3), E=st.integers(1, 10), T=st.integers(2, 20), B=st.integers(2, 70))
    def icm(kind, NA, O, H, d_inv, d_fwd, E, T, B):
        space = Discrete(NA) if kind == "d" else Box(-1.0, 1.0, (NA,), np.float32)
        icm_kw = dict(encoded_obs_dim=H, encoder_hidden_size=H, inverse_hidden_size=H, forward_hidden_size=H,
                      inverse_hidden_depth=d_inv, forward_hidden_depth=d_fwd)
        res = []
        for mode in ("fused", "torch"):
            env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=5, term_prob=0.05)
            sp = Box(-np.inf, np.inf, (O,), np.float32)
            ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(enable_icm=True, icm_kw_args=icm_kw))}, device=dev,
                      random_seed=4, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
                      batch_size=B, epochs_per_iter=1, update_mode=mode, use_graphs=False)
            pol = ppo.policies["p"]
            assert (ppo._fused_icm_updater("p") is not None) == (mode == "fused")
            ppo.rollout()
            loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
            ppo._icm_batch_train(loader, "p")
            res.append((pol.icm_model.flat_params.detach().cpu().numpy().copy(), pol.buffer.rewards.cpu().numpy().copy(),
                        ppo.status_dict["p"]["icm loss"]))
        (w0, r0, l0), (w1, r1, l1) = res
        np.testing.assert_allclose(r0, r1, rtol=3e-5, atol=3e-6)                 # rollout-time intrinsic rewards
        np.testing.assert_allclose(l0, l1, rtol=5e-5)
        np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)

    mat()
    icm()


def test_rollout_dataset_order_fuzz_against_the_cpu_port():
    """
    Randomised episode structure (hypothesis, derandomised): any mix of terminations, max_ts_per_ep cuts (down to 1)
    and the end-of-rollout bootstrap; the dataset's completion order, returns, advantages, episode lengths and the
    rollout statistics against the CPU port's per-env Python loop (ppo.py:1804-1983, episode_info.py:44-135).
    """
    from hypothesis import given, settings, strategies as st, HealthCheck

    @settings(max_examples=20, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(E=st.integers(1, 20), T=st.integers(1, 40), term=st.sampled_from([0.0, 0.05, 0.3, 0.9]),
           max_ts=st.sampled_from([1, 2, 3, 7, 200]), fused=st.booleans())
    def run(E, T, term, max_ts, fused):
        ppo = _make(E, T, 32, 1, term, max_ts, update_mode="fused" if fused else "torch")
        cpu = _oracle_like(ppo, 32)
        ds = ppo.rollout()
        env = ppo.env
        buf = ppo.policies["p"].buffer
        t_tab = None if env.term_table is None else env.term_table.cpu().numpy()
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                          actions=buf.actions[..., 0].cpu().numpy(), term_table=t_tab, max_ts_per_ep=max_ts)
        assert len(ds) == len(ref) == E * T
        tol = dict(rtol=1e-5, atol=1e-5)
        np.testing.assert_array_equal(ds.observations.cpu().numpy(), ref.observations.numpy())
        np.testing.assert_array_equal(ds.actions.cpu().numpy(), ref.actions.numpy())
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
        np.testing.assert_array_equal(ds.ep_lens.cpu().numpy(), [ep.length for ep in ref.episodes])

    run()


@pytest.mark.parametrize("k12_form", ["chain", "slabs", "tiles"])
def test_fused_update_fuzz_with_different_actor_and_critic_shapes(k12_form, monkeypatch):
    """
    K12 / K6+K7 with the MAPPO shape: several agents share the policy, the critic sees the
    concatenated observations of the env ("policy" view) and is wider than the actor -- the instantiated mixed
    width pairs (128, 256) and (64, 128).  Fused kernels against the torch-ROCm path, random sizes.
    """
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    from ppo_and_friends_amd import fused_update
    if k12_form == "slabs":
        monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "0")
    if k12_form == "tiles":                                  # one workgroup per 16-row tile of the 256-wide critic instead of a pair
        monkeypatch.setattr(fused_update.FusedPolicyUpdate, "row_pairs", False)

    @settings(max_examples=12, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(A=st.integers(2, 4), O=st.integers(1, 24), NA=st.integers(2, 8), widths=st.sampled_from([(128, 256), (64, 128)]),
           E=st.integers(1, 8), T=st.integers(2, 16), B=st.integers(2, 200), cont=st.booleans())
    def run(A, O, NA, widths, E, T, B, cont):
        space = Box(-1.0, 1.0, (NA,), np.float32) if cont else Discrete(NA)
        res = []
        for mode in ("fused", "torch"):
            env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=21, num_agents=A,
                                                      critic_view="policy", term_prob=0.05)
            sp, csp = Box(-np.inf, np.inf, (O,), np.float32), Box(-np.inf, np.inf, (A * O,), np.float32)
            pargs = dict(actor_kw_args=dict(hidden_size=widths[0]), critic_kw_args=dict(hidden_size=widths[1]))
            ppo = PPO(env_gen, {"team": (None, sp, csp, space, pargs)}, device=dev, random_seed=3, normalize_obs=False,
                      normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1,
                      update_mode=mode, use_graphs=False)
            pol = ppo.policies["team"]
            assert (ppo._fused_updater("team", B) is not None) == (mode == "fused")
            ppo.rollout()
            loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
            pol.train()
            ppo._ppo_batch_train(loader, "team")
            sd = ppo.status_dict["team"]
            res.append((pol.policy_params.detach().cpu().numpy().copy(), pol.buffer.log_probs.cpu().numpy().copy(),
                        pol.buffer.values.cpu().numpy().copy(),
                        [sd[k] for k in ("actor loss", "critic loss", "kl avg", "weighted entropy")]))
        (w0, lp0, v0, s0), (w1, lp1, v1, s1) = res
        np.testing.assert_allclose(lp0, lp1, rtol=3e-5, atol=3e-5)          # same Philox stream in both rollouts
        np.testing.assert_allclose(s0, s1, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)
        np.testing.assert_allclose(v0, v1, rtol=2e-4, atol=3e-5)

    run()


def test_lstm_sequence_path_fuzz_against_the_cpu_port():
    """
    Randomised sequence lengths / episode structures for the LSTM path (hypothesis, derandomised): windows that
    straddle terminations and max_ts cuts, sequence lengths up to the rollout length, single-env rollouts --
    log-probs, returns, advantages, logged hidden states and one update epoch against oracle/lstm_oracle.CpuLSTMPPO.
    """
    from hypothesis import given, settings, strategies as st, HealthCheck
    from oracle import lstm_oracle
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)

    @settings(max_examples=10, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(S=st.integers(1, 6), E=st.integers(1, 6), T=st.integers(6, 18), O=st.integers(1, 9), NA=st.integers(2, 5),
           B=st.integers(2, 24), term=st.sampled_from([0.0, 0.1, 0.4]), max_ts=st.sampled_from([2, 5, 200]))
    def run(S, E, T, O, NA, B, term, max_ts):
        H, seed = 16, 2
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=13, term_prob=term)
        sp = Box(-np.inf, np.inf, (O,), np.float32)
        net_kw = dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=H)
        ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(ac_network=LSTMNetwork, actor_kw_args=net_kw,
                                                                 critic_kw_args=net_kw))},
                  device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
                  ts_per_rollout=T, batch_size=B, epochs_per_iter=1, max_ts_per_ep=max_ts)
        pol = ppo.policies["p"]
        cpu = lstm_oracle.CpuLSTMPPO(O, NA, sequence_length=S, lstm_hidden=H, ff_hidden=H, batch_size=B, seed=seed)
        cpu.actor.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor.state_dict().items()})
        cpu.critic.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.critic.state_dict().items()})
        cpu.loader_generator = torch.Generator().manual_seed(seed)
        ds = ppo.rollout()
        env = ppo.env
        t_tab = None if env.term_table is None else env.term_table.cpu().numpy()
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                          pol.buffer.actions[..., 0].cpu().numpy(), t_tab, max_ts_per_ep=max_ts)
        assert len(ds) == len(ref) == E * T - (S - 1)
        tol = dict(rtol=3e-5, atol=3e-5)
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy().reshape(-1), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(), **tol)
        for i in (0, len(ds) // 2, len(ds) - 1):
            got, want = ds[i], ref[i]
            np.testing.assert_allclose(got[1].cpu().numpy(), want[1].numpy(), **tol)     # masked obs window
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator, ppo._perm_cache)
        pol.train()
        ppo._ppo_batch_train(loader, "p")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["p"][k], r[k], rtol=2e-4, atol=2e-5, err_msg=k)

    run()


def test_graph_chunking_fuzz_equals_eager_launches(monkeypatch):
    """
    hipGraph chunking of the fused chains (32-mini-batch chunks, eager remainder, epoch tail, a second epoch that
    replays the captured chunk): for random small batch sizes and dataset lengths the graph-replayed run and the
    eager run of the same kernels must agree bitwise -- K12 (the launch chain), and K15 for a MATPolicy.
    """
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)

    @settings(max_examples=10, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(B=st.integers(2, 9), E=st.integers(2, 12), T=st.integers(20, 60), mat=st.booleans())
    def run(B, E, T, mat):
        outs = []
        for graphs in (True, False):
            A = 3 if mat else 1
            env_gen = lambda: SyntheticFixedLengthEnv(E, 6, Discrete(4), T, dev, reward="uniform", seed=9, num_agents=A)
            sp = Box(-np.inf, np.inf, (6,), np.float32)
            ppo = PPO(env_gen, {"p": (MATPolicy if mat else None, sp, sp, Discrete(4), {})}, device=dev, random_seed=5,
                      normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B,
                      epochs_per_iter=2, update_mode="fused", use_graphs=graphs, save_state=False)
            ppo.rollout()
            ppo.train_on_rollout()
            pol = ppo.policies["p"]
            w = (pol.actor_critic.flat_params if mat else pol.policy_params).detach().clone()
            sd = ppo.status_dict["p"]
            outs.append((w, [sd[k] for k in ("actor loss", "critic loss", "kl avg")]))
        assert torch.equal(outs[0][0], outs[1][0]), (B, E, T, mat)
        assert outs[0][1] == outs[1][1]

    run()


def test_schedulers_and_freeze_cycling_in_the_training_loop(tmp_path):
    """
    utils/schedulers.py in PPO.learn (ppo.py:2139, 2254, 1406-1428): a LinearScheduler learning rate / entropy weight
    follows the status dict (the lr through the device scalar, the entropy weight as a launch argument of the
    re-captured chains), and a FreezeCyclingScheduler lets one of two policies train at a time -- a frozen
    policy's weights and optimiser state do not move.
    """
    import os
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    from ppo_and_friends_amd.utils.schedulers import LinearScheduler, FreezeCyclingScheduler
    dev = torch.device("cuda", 0)
    A, E, T, O, NA, B = 2, 8, 16, 5, 3, 32
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=21, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    total = 6 * E * T
    sched = lambda hi, lo: LinearScheduler("timesteps", status_max=total, max_value=hi, min_value=lo)
    settings = {"p0": (None, sp, sp, Discrete(NA), dict(lr=sched(1e-3, 1e-4), entropy_weight=sched(0.02, 0.0))),
                "p1": (None, sp, sp, Discrete(NA), {})}
    ppo = PPO(env_gen, settings, policy_mapping_fn=lambda a: "p0" if a == "agent0" else "p1", device=dev, random_seed=3,
              normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B,
              epochs_per_iter=1, state_path=str(tmp_path), freeze_scheduler=FreezeCyclingScheduler([["p0"]], iterations=2))
    snaps, lrs, ews, frozen = [], [], [], []
    for it in range(6):
        before = {k: p.policy_params.clone() for k, p in ppo.policies.items()}
        ppo.learn(E * T)                                           # one iteration
        frozen.append({k: p.frozen for k, p in ppo.policies.items()})
        for k, p in ppo.policies.items():
            moved = not torch.equal(before[k], p.policy_params)
            assert moved == (not frozen[-1][k]), (it, k, frozen[-1])
        lrs.append(float(ppo.policies["p0"].policy_lr.item())); ews.append(ppo.status_dict["p0"]["entropy weight"])
    assert all(sum(f.values()) == 1 for f in frozen) and {f["p0"] for f in frozen} == {True, False}
    assert lrs == sorted(lrs, reverse=True) and lrs[0] > lrs[-1] >= 1e-4 - 1e-9
    assert ews == sorted(ews, reverse=True) and ews[-1] < ews[0]
    assert os.path.exists(os.path.join(str(tmp_path), "FreezeCyclingScheduler.yaml"))
    assert ppo.status_dict["p1"]["lr"] == 3e-4


@pytest.mark.parametrize("term_prob,max_ts", [(0.0, 200), (0.08, 7), (0.3, 3)])
def test_dynamic_bootstrap_clip_matches_cpu_port(term_prob, max_ts):
    """
    dynamic_bs_clip (ppo_policy.py:1086-1112; baselines/gymnasium/pendulum.py:33): the bootstrap reward of every
    cut episode is clipped to the (min, max) of that episode's own rewards -- a per-segment reduction on the
    device buffer -- against the CPU port's per-episode lists; recalculate_advantages keeps it.
    """
    E, T, B = 10, 24, 32
    def biased(ppo):                                   # a critic that bootstraps far outside the reward range
        with torch.no_grad():
            list(ppo.policies["p"].critic.parameters())[-1].fill_(5.0)
        return ppo
    ppo = biased(_make(E, T, B, 1, term_prob, max_ts, policy_args=dict(dynamic_bs_clip=True)))
    cpu = _oracle_like(ppo, B)
    cpu.clip = "dynamic"
    ds = ppo.rollout()
    env, buf = ppo.env, ppo.policies["p"].buffer
    t_tab = None if env.term_table is None else env.term_table.cpu().numpy()
    ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(), actions=buf.actions[..., 0].cpu().numpy(),
                      term_table=t_tab, max_ts_per_ep=max_ts)
    tol = dict(rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
    np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
    # the clip was active somewhere (values ~ N(0,1)-scaled bootstraps vs rewards in [-1, 1])
    plain = biased(_make(E, T, B, 1, term_prob, max_ts))
    ds2 = plain.rollout()
    assert not np.allclose(ds2.rewards_to_go.cpu().numpy(), ds.rewards_to_go.cpu().numpy())
    before = ds.advantages.clone()
    ds.recalculate_advantages()
    torch.testing.assert_close(ds.advantages, before)


@pytest.mark.parametrize("A", [1, 2])
def test_policy_surface_add_episode_info_and_end_episodes(A):
    """
    The reference's per-agent policy surface (ppo_policy.py:545-719; call sites ppo.py:1742-1752, 1813-1819, 1932-1938):
    numpy batches handed over agent by agent with `add_episode_info`, terminal / maxed envs closed with
    `end_episodes` (env index lists, one ending value per listed env or per env), then `finalize_dataset` -- must
    build the very dataset the device rollout builds from the same transitions.
    """
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA, max_ts = 9, 20, 5, 3, 6

    def make():
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=31, term_prob=0.07,
                                                  num_agents=A)
        sp = Box(-np.inf, np.inf, (O,), np.float32)
        return PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), {})}, device=dev, random_seed=2, normalize_obs=False,
                   normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=32, epochs_per_iter=1,
                   max_ts_per_ep=max_ts, save_state=False)

    ref = make()
    want = ref.rollout()
    rb = ref.policies["p"].buffer
    n = lambda x: x.detach().cpu().numpy()
    ppo = make()
    pol = ppo.policies["p"]
    pol.initialize_dataset()
    pol.initialize_episodes(E, ppo.status_dict, ts_per_rollout=ppo.ts_per_rollout)     # total steps over the E envs
    env = ref.env
    term = n(env.term_table.view(T, A, E)[:, 0])                              # agents of an env end together
    ep_ts = np.zeros(E, dtype=np.int64)
    for t in range(T):
        for a, agent_id in enumerate(pol.agent_ids):
            cols = slice(a * E, (a + 1) * E)
            pol.add_episode_info(agent_id=agent_id, critic_observations=n(rb.critic_observations[t, cols]),
                                 observations=n(rb.observations[t, cols]), next_observations=n(rb.observations[t, cols]),
                                 raw_actions=n(rb.raw_actions[t, cols]), actions=n(rb.actions[t, cols]),
                                 values=n(rb.values[t, cols]), log_probs=rb.log_probs[t, cols].reshape(E, 1),
                                 rewards=n(rb.rewards[t, cols]), where_done=np.where(term[t])[0])
        ep_ts += 1
        where_term = np.where(term[t])[0]
        where_maxed = np.setdiff1d(np.arange(E) if t == T - 1 else np.where(ep_ts >= max_ts)[0], where_term)
        for a, agent_id in enumerate(pol.agent_ids):
            cols = slice(a * E, (a + 1) * E)
            if where_term.size:                                               # ppo.py:1813-1819: one (0, 0) per listed env
                pol.end_episodes(agent_id=agent_id, env_idxs=where_term, episode_lengths=ep_ts, terminal=np.ones(where_term.size, bool),
                                 ending_values=np.zeros(where_term.size, np.float32), ending_rewards=np.zeros(where_term.size, np.float32))
            if where_maxed.size:                                              # ppo.py:1932-1938: one value per ENV
                pol.end_episodes(agent_id=agent_id, env_idxs=where_maxed, episode_lengths=ep_ts, terminal=np.zeros(where_maxed.size, bool),
                                 ending_values=n(rb.boot_value[t, cols]), ending_rewards=n(rb.boot_reward[t, cols]))
        ep_ts[where_term] = 0
        ep_ts[where_maxed] = 0
    pol.finalize_dataset()
    got = pol.dataset
    assert len(got) == len(want) == A * E * T
    np.testing.assert_array_equal(n(got.ep_lens), n(want.ep_lens))
    for f in ("observations", "actions", "log_probs", "rewards_to_go", "advantages"):
        np.testing.assert_array_equal(n(getattr(got, f)), n(getattr(want, f)), err_msg=f)


@pytest.mark.parametrize("kind", ["multi-discrete", "multi-binary"])
def test_multi_discrete_and_multi_binary_action_spaces_train(kind):
    """
    MultiDiscrete / MultiBinary action spaces (networks/distributions.py:134-196, 272-438, 1046-1056) through the
    whole loop on the torch-ROCm update path: actions of the right shape / dtype in the buffer, the first
    mini-batch's ratio is exactly 1 (rollout log-probs == evaluation log-probs: kl == 0 before any update), two
    iterations of training with finite statistics and moving weights.
    """
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, MultiBinary, MultiDiscrete
    dev = torch.device("cuda", 0)
    E, T, O, B = 8, 16, 5, 32
    space = MultiDiscrete([3, 4, 2]) if kind == "multi-discrete" else MultiBinary(5)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, {})}, device=dev, random_seed=4, normalize_obs=False,
              normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1, save_state=False)
    pol = ppo.policies["p"]
    assert ppo._fused_updater("p", B) is None                     # torch-ROCm path for these heads
    ppo.rollout()
    buf = pol.buffer
    if kind == "multi-discrete":
        assert buf.actions.shape == (T, E, 3) and buf.actions.dtype == torch.int64
        assert all(int(buf.actions[..., i].max()) < k for i, k in enumerate((3, 4, 2)))
    else:
        assert buf.actions.shape == (T, E, 5) and set(buf.actions.unique().tolist()) <= {0.0, 1.0}
    with torch.no_grad():
        _, lp, _ = pol.evaluate(buf.critic_observations.view(T * E, O), buf.observations.view(T * E, O),
                                buf.raw_actions.view(T * E, -1))
    torch.testing.assert_close(lp.reshape(T, E), buf.log_probs, rtol=1e-5, atol=1e-6)
    w0 = pol.policy_params.clone()
    for _ in range(2):
        ppo.train_on_rollout()
        sd = ppo.status_dict["p"]
        assert all(np.isfinite(sd[k]) for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"))
        ppo.rollout()
    assert not torch.equal(w0, pol.policy_params)


def test_mat_policy_with_continuous_actions_is_self_consistent():
    """
    MATPolicy over a Box action space (mat_policy.py:308-344 continuous token block, :441-519 autoregressive
    sampling with the tanh-Gaussian head): torch-ROCm path.  The autoregressive rollout's log-probs / values must
    equal the teacher-forced evaluation of the same raw actions (kl == 0 before any update), and training moves
    the weights with finite statistics.
    """
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    dev = torch.device("cuda", 0)
    A, E, T, O, D, B = 3, 6, 10, 7, 2, 16
    space = Box(-1.0, 1.0, (D,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, space, {})}, device=dev, random_seed=6, normalize_obs=False,
              normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1, save_state=False)
    pol = ppo.policies["mat"]
    assert ppo._fused_updater("mat", B) is None
    ppo.rollout()
    buf = pol.buffer
    assert buf.actions.shape == (T, E, A, D) and float(buf.actions.abs().max()) <= 1.0
    flat = lambda x: x.reshape((T * E,) + tuple(x.shape[2:]))
    with torch.no_grad():
        v, lp, _ = pol.evaluate(flat(buf.critic_observations), flat(buf.observations), flat(buf.raw_actions))
    torch.testing.assert_close(lp.reshape(T, E, A), buf.log_probs, rtol=2e-5, atol=2e-5)
    w0 = pol.actor_critic.flat_params.clone()
    ppo.train_on_rollout()
    sd = ppo.status_dict["mat"]
    assert all(np.isfinite(sd[k]) for k in ("actor loss", "critic loss", "kl avg"))
    assert not torch.equal(w0, pol.actor_critic.flat_params)


def test_full_pipeline_fuzz_fused_equals_torch():
    """
    The C3-shaped pipeline at random small sizes (hypothesis, derandomised): filter stack (any subset of the four
    wrappers) + tanh-Gaussian or categorical policy + ICM + terminations + value normalisation, one complete
    iteration (rollout, PPO epoch, ICM epoch, overlapped or not) with every fused chain (K6/K7, K12, K13, K14) against
    the torch-ROCm paths on the same seeds.
    """
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)

    @settings(max_examples=26, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(O=st.integers(1, 30), cont=st.booleans(), NA=st.integers(2, 6), E=st.integers(2, 10), T=st.integers(3, 18),
           B=st.integers(2, 48), norm_obs=st.booleans(), norm_rew=st.booleans(), clip=st.booleans(), icm=st.booleans(),
           term=st.sampled_from([0.0, 0.1]), overlap=st.booleans())
    def run(O, cont, NA, E, T, B, norm_obs, norm_rew, clip, icm, term, overlap):
        space = Box(-1.0, 1.0, (NA,), np.float32) if cont else Discrete(NA)
        res = []
        for mode in ("fused", "torch"):
            env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=17, term_prob=term)
            sp = Box(-np.inf, np.inf, (O,), np.float32)
            ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(enable_icm=icm))}, device=dev, random_seed=8,
                      normalize_obs=norm_obs, normalize_rewards=norm_rew, obs_clip=(-2.0, 2.0) if clip else None,
                      reward_clip=(-1.5, 1.5) if clip else None, envs_per_proc=E, ts_per_rollout=T, batch_size=B,
                      epochs_per_iter=1, update_mode=mode, use_graphs=False, save_state=False)
            ppo.overlap_icm = overlap
            ppo.rollout()
            ppo.train_on_rollout()
            pol = ppo.policies["p"]
            sd = ppo.status_dict["p"]
            keys = ["actor loss", "critic loss", "kl avg"] + (["icm loss"] if icm else [])
            res.append((pol.policy_params.detach().cpu().numpy().copy(),
                        pol.icm_model.flat_params.detach().cpu().numpy().copy() if icm else np.zeros(1),
                        pol.buffer.rewards.cpu().numpy().copy(), [sd[k] for k in keys]))
        (w0, i0, r0, s0), (w1, i1, r1, s1) = res
        np.testing.assert_allclose(r0, r1, rtol=5e-5, atol=5e-6)             # filtered (+ intrinsic) rewards
        np.testing.assert_allclose(s0, s1, rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(w0, w1, rtol=3e-4, atol=5e-5)
        np.testing.assert_allclose(i0, i1, rtol=3e-4, atol=5e-5)

    run()

