"""
K18 (csrc/lstm.hip): the HIP LSTM network that PPO(update_mode="fused") runs for LSTM policies, against torch-CPU
nn.LSTM (same module, same weights), the reference's recorded LSTM iterations, the CPU port of the reference's LSTM
flow, and itself (stateful stepping, bitwise reruns, checkpoints read by the MIOpen path).
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# ---- bounds of the quantities that pass through optimiser steps (fixtures g12_lstm_*), starting from the floors of
# tests/test_gpu_reference_golden.py: final weights max |dw| <= 2e-6, epoch statistics max |got - want| / (0.1 + |want|)
# <= 2e-6.  Measured on the MI355X with K18: g12_lstm_term stat_dev 8.3e-08, weight_max 6.0e-08 (actor) / 6.0e-08
# (critic); g12_lstm_cut stat_dev 2.6e-07, weight_max 6.0e-08 / 3.0e-08 (nn.LSTM / MIOpen: 1.7e-07, 3.0e-08 .. 6.0e-08).
WEIGHT_MAX = 2e-6
STAT_DEV = 2e-6


def _act(name):
    return {"relu": nn.ReLU(), "leaky": nn.LeakyReLU(), "tanh": nn.Tanh()}[name]


def _pair(I, O, H, F, depth, act, S, seed):
    """(HIP network on the device, the same module on the CPU)."""
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    torch.manual_seed(seed)
    cpu = LSTMNetwork(I, O, sequence_length=S, activation=_act(act), lstm_hidden_size=H, ff_hidden_size=F,
                      ff_hidden_depth=depth, name="net")
    with torch.no_grad():                          # non-zero biases / affine LayerNorm so that every path is exercised
        for n, p in cpu.named_parameters():
            if "bias" in n or "layer_norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    gpu = copy.deepcopy(cpu)
    gpu.flatten_parameters_(DEV)
    gpu.use_hip = True
    assert gpu.hip_unsupported_reason() == ""
    return gpu, cpu


# H, F, depth, activation, out (2 categorical logits / 6 Gaussian means / 1 value), S, rows, in_dim (K18 instantiates
# lstm_rows_forward<H, false>, K22 the <H, true> form: both pad the input to 16-column chunks, limit 256)
GRID = [
    (32, 16, 1, "leaky", 2, 5, 256, 17),
    (32, 32, 2, "tanh", 1, 1, 2, 4),
    (32, 128, 1, "relu", 6, 16, 2, 4),
    (64, 64, 1, "relu", 6, 3, 256, 17),
    (64, 16, 2, "leaky", 1, 10, 2, 4),
    (64, 32, 1, "tanh", 2, 1, 4096, 17),
    (128, 128, 1, "relu", 6, 10, 256, 17),
    (128, 64, 2, "tanh", 2, 16, 256, 17),
    (128, 16, 1, "leaky", 1, 5, 4096, 17),
    (128, 128, 2, "relu", 8, 1, 256, 17),
    (32, 64, 1, "relu", 3, 3, 4096, 17),
    (32, 16, 1, "relu", 2, 4, 2, 1),
    (128, 32, 2, "tanh", 3, 3, 256, 1),
    (32, 32, 1, "leaky", 6, 5, 256, 16),
    (128, 16, 1, "relu", 1, 2, 2, 16),
    (32, 16, 2, "tanh", 2, 3, 256, 255),
    (128, 128, 2, "relu", 8, 16, 2, 255),
    (32, 64, 1, "leaky", 1, 4, 2, 256),
    (128, 128, 1, "tanh", 6, 6, 256, 256),
]


# (the rows with in_dim 17 / 4 keep the test ids they had before the grid had that column)
@pytest.mark.parametrize("H,F,depth,act,O,S,N,I", [
    pytest.param(*r, id="-".join(map(str, r[:7] if r[7] == (17 if r[6] != 2 else 4) else r))) for r in GRID])
def test_network_matches_torch_cpu(H, F, depth, act, O, S, N, I):
    gpu, cpu = _pair(I, O, H, F, depth, act, S, seed=H + F + S + N)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, S, I, generator=g)
    h0 = 0.5 * torch.randn(1, N, H, generator=g)
    c0 = 0.5 * torch.randn(1, N, H, generator=g)
    w = torch.randn(N, O, generator=g) / N
    cpu.hidden_state = (h0.clone(), c0.clone())
    out_c = cpu.forward_logits(x if S > 1 else x[:, 0])
    torch.autograd.backward(out_c, w)
    gpu.hidden_state = (h0.to(DEV), c0.to(DEV))
    gpu.flat_grads.zero_()
    out_g = gpu.forward_logits((x if S > 1 else x[:, 0]).to(DEV))
    torch.autograd.backward(out_g, w.to(DEV))
    np.testing.assert_allclose(out_g.detach().cpu().numpy(), out_c.detach().numpy(), rtol=1e-5, atol=1e-5)
    for a, b, what in zip(gpu.hidden_state, cpu.hidden_state, ("h", "c")):
        assert tuple(a.shape) == (1, N, H)
        np.testing.assert_allclose(a.cpu().numpy(), b.detach().numpy(), rtol=1e-5, atol=1e-5, err_msg=what)
    for (name, pg), (_, pc) in zip(gpu.named_parameters(), cpu.named_parameters()):
        want = pc.grad.numpy()
        scale = float(np.abs(want).max())
        np.testing.assert_allclose(pg.grad.cpu().numpy(), want, rtol=0, atol=1e-5 * scale + 1e-12,
                                   err_msg=f"{name} (max |g| {scale:.3e})")


def test_single_steps_equal_one_window():
    """The module is stateful: S calls of one step each give the output and (h, c) of one S-step window."""
    gpu, _ = _pair(17, 6, 64, 64, 1, "relu", 7, seed=3)
    x = torch.randn(300, 7, 17, device=DEV)
    with torch.no_grad():
        gpu.reset_hidden_state(300, DEV)
        win = gpu.forward_logits(x)
        h_w, c_w = gpu.hidden_state
        gpu.reset_hidden_state(300, DEV)
        for t in range(7):
            step = gpu.forward_logits(x[:, t])
    np.testing.assert_allclose(step.cpu().numpy(), win.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(gpu.hidden_state[0].cpu().numpy(), h_w.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(gpu.hidden_state[1].cpu().numpy(), c_w.cpu().numpy(), rtol=1e-6, atol=1e-6)


def _lstm_ppo(update_mode, action="discrete", H=32, F=32, S=4, E=8, T=24, B=16, seed=1, epochs=1, term_prob=0.05):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    O = 5
    act_space = Discrete(3) if action == "discrete" else Box(-1.0, 1.0, (2,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, act_space, T, DEV, reward="uniform", seed=13, term_prob=term_prob)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    kw = dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=F)
    return PPO(env_gen, {"p": (None, sp, sp, act_space, dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
               device=DEV, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
               ts_per_rollout=T, batch_size=B, epochs_per_iter=epochs, max_ts_per_ep=7, save_state=False,
               update_mode=update_mode)


def _train(ppo, iterations=1):
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol = ppo.policies["p"]
    for _ in range(iterations):
        ppo.rollout()
        pol.train()
        for _ in range(ppo.epochs_per_iter):
            ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator), "p")
        pol.clear_dataset()
    return pol


@pytest.mark.parametrize("action", ["discrete", "continuous"])
def test_fused_lstm_policy_runs_without_miopen(monkeypatch, action):
    """update_mode='fused': a rollout and an update epoch of an LSTM policy never reach nn.LSTM (MIOpen)."""
    def refuse(*a, **k):
        raise AssertionError("nn.LSTM.forward was called under update_mode='fused'")
    monkeypatch.setattr(torch.nn.LSTM, "forward", refuse)
    ppo = _lstm_ppo("fused", action)
    pol = ppo.policies["p"]
    assert pol.actor.use_hip and pol.critic.use_hip
    w0 = pol.policy_params.clone()
    _train(ppo)
    assert torch.isfinite(pol.policy_params).all()
    assert not torch.equal(w0, pol.policy_params)
    for k in ("actor loss", "critic loss", "kl avg"):
        assert np.isfinite(ppo.status_dict["p"][k]), k


def test_auto_mode_keeps_nn_lstm():
    ppo = _lstm_ppo("auto")
    pol = ppo.policies["p"]
    assert not pol.actor.use_hip and not pol.critic.use_hip


def test_two_seeded_runs_are_bitwise_identical():
    a = _train(_lstm_ppo("fused", "continuous", H=64, F=32, S=5, epochs=2), iterations=2)
    b = _train(_lstm_ppo("fused", "continuous", H=64, F=32, S=5, epochs=2), iterations=2)
    assert torch.equal(a.policy_params, b.policy_params)


def test_fused_checkpoint_loads_into_the_miopen_path(tmp_path):
    pol_f = _train(_lstm_ppo("fused"))
    pol_a = _lstm_ppo("auto", seed=5).policies["p"]
    for tag in ("actor", "critic"):
        net_f, net_a = getattr(pol_f, tag), getattr(pol_a, tag)
        net_f.save(str(tmp_path))
        assert list(net_f.state_dict().keys()) == list(net_a.state_dict().keys())
        net_a.load(str(tmp_path))
        x = torch.randn(40, 4, 5, device=DEV)
        with torch.no_grad():
            net_f.reset_hidden_state(40, DEV)
            net_a.reset_hidden_state(40, DEV)
            y_f, y_a = net_f.forward_logits(x), net_a.forward_logits(x)
        np.testing.assert_allclose(y_f.cpu().numpy(), y_a.cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg=tag)


@pytest.mark.parametrize("S,max_ts,term_prob,H", [(4, 7, 0.05, 32), (10, 200, 0.08, 128)])
def test_fused_lstm_policy_matches_the_cpu_port(S, max_ts, term_prob, H):
    """Two iterations against oracle/lstm_oracle.CpuLSTMPPO (the reference's list-based LSTM flow on torch-CPU), with
    the tolerances of test_gpu_end_to_end.py's nn.LSTM version of this test."""
    from oracle import lstm_oracle
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    E, T, O, NA, B, seed = 6, 20, 5, 3, 16, 2
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, DEV, reward="uniform", seed=13, term_prob=term_prob)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    net_kw = dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=H)
    ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(ac_network=LSTMNetwork, actor_kw_args=net_kw,
                                                             critic_kw_args=net_kw))},
              device=DEV, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
              ts_per_rollout=T, batch_size=B, epochs_per_iter=1, max_ts_per_ep=max_ts, update_mode="fused")
    pol = ppo.policies["p"]
    assert pol.actor.use_hip
    cpu = lstm_oracle.CpuLSTMPPO(O, NA, sequence_length=S, lstm_hidden=H, ff_hidden=H, batch_size=B, seed=seed)
    cpu.actor.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor.state_dict().items()})
    cpu.critic.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.critic.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    flat = lambda net: torch.cat([p.detach().cpu().reshape(-1) for p in net.parameters()]).numpy()
    for it in range(2):
        ds = ppo.rollout()
        env = ppo.env
        term = None if env.term_table is None else env.term_table.cpu().numpy()
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                          pol.buffer.actions[..., 0].cpu().numpy(), term, max_ts_per_ep=max_ts)
        tol = dict(rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy().reshape(-1), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(), **tol)
        np.testing.assert_allclose(ds.critic_cell[torch.arange(E * T)].cpu().numpy(), ref.critic_cell.numpy(), **tol)
        pol.train()
        ppo._ppo_batch_train(PermutationLoader(pol.dataset, B, ppo.loader_generator, ppo._perm_cache), "p")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["p"][k], r[k], rtol=1e-4, atol=1e-5, err_msg=f"{k} it={it}")
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(),
                                   rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(flat(pol.actor), flat(cpu.actor), rtol=2e-4, atol=5e-5)
    np.testing.assert_allclose(flat(pol.critic), flat(cpu.critic), rtol=2e-4, atol=5e-5)


@pytest.mark.parametrize("name,S,n_act", [("g12_lstm_term", 4, 2), ("g12_lstm_cut", 3, 3)])
def test_fused_lstm_reproduces_the_reference_iterations(golden, name, S, n_act):
    """
    Fixtures g12_lstm_* (recorded from the reference's own PPO object) through PPO(update_mode="fused"), i.e. K18 in the
    rollout and the update: logged hidden states, log-probs, returns, advantages at 1e-5; epoch statistics and final
    weights within STAT_DEV / WEIGHT_MAX.
    """
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.spaces import Box, Discrete
    from test_gpu_reference_golden import FixedPermLoader, _cfg, agent_major
    g = golden(name)
    c = _cfg(g)
    E, T, O, B = c["E"], c["T"], c["O"], c["batch_size"]

    class FixtureEnv(SyntheticFixedLengthEnv):
        def __init__(self):
            super().__init__(E, O, Discrete(n_act), T, DEV, term_prob=0.5 if g["term_table"].any() else 0.0)
            self.obs_table = self.critic_obs_table = torch.from_numpy(agent_major(g["obs_table"])).to(DEV)
            self.reward_table = torch.from_numpy(agent_major(g["reward_table"])).to(DEV)
            if g["term_table"].any():
                self.term_table = torch.from_numpy(g["term_table"]).to(DEV)

    kw = dict(sequence_length=S, lstm_hidden_size=32, ff_hidden_size=32)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(FixtureEnv, {"agent": (None, sp, sp, Discrete(n_act), dict(ac_network=LSTMNetwork, actor_kw_args=dict(kw),
                                                                       critic_kw_args=dict(kw)))},
              device=DEV, random_seed=c["seed"], normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
              ts_per_rollout=T, batch_size=B, epochs_per_iter=c["epochs"], max_ts_per_ep=c["max_ts_per_ep"],
              save_state=False, update_mode="fused")
    pol = ppo.policies["agent"]
    assert pol.actor.use_hip and pol.critic.use_hip
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        sd0 = {k[len(f"init_{tag}."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"init_{tag}.")}
        missing, unexpected = net.load_state_dict(sd0, strict=False)
        assert not missing and not unexpected, (tag, missing, unexpected)
    tol = dict(rtol=1e-5, atol=1e-5)
    sd = ppo.status_dict["agent"]
    ep = 0
    stat_dev = 0.0
    for it in range(c["iterations"]):
        sl = slice(it * T, (it + 1) * T)
        ppo.replay_raw_actions = torch.from_numpy(agent_major(g["step_raw_actions"][sl]).reshape(T, E, 1)).to(DEV)
        ds = ppo.rollout()
        pre = f"it{it}_ds_"
        np.testing.assert_array_equal(ds.observations.cpu().numpy(), g[pre + "observations"])
        np.testing.assert_allclose(ds.log_probs.cpu().numpy().reshape(-1), g[pre + "log_probs"].reshape(-1), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), g[pre + "rewards_to_go"], **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), g[pre + "advantages"], **tol)
        for k in ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell"):
            np.testing.assert_allclose(getattr(ds, k)[torch.arange(E * T, device=DEV)].cpu().numpy(), g[pre + k], err_msg=k, **tol)
        pol.train()
        for e in range(c["epochs"]):
            ppo._ppo_batch_train(FixedPermLoader(pol.dataset, B, g["epoch_perms"][ep] - (S - 1)), "agent")
            got = np.array([sd["actor loss"], sd["critic loss"], sd["kl avg"], sd["weighted entropy"]], dtype=np.float64)
            want = np.asarray(g["epoch_stats"][ep], dtype=np.float64)
            stat_dev = max(stat_dev, float(np.max(np.abs(got - want) / (0.1 + np.abs(want)))))
            ep += 1
        pol.clear_dataset()
    print(f"{name}: stat_dev {stat_dev:.3e}")
    assert stat_dev <= STAT_DEV, f"epoch statistics: {stat_dev:.3e} > {STAT_DEV:.0e}"
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        got = np.concatenate([p.detach().cpu().numpy().reshape(-1) for k, p in net.named_parameters()])
        want = np.concatenate([g[f"final_{tag}.{k}"].reshape(-1) for k, p in net.named_parameters()])
        d = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{name}: {tag} weight_max {d:.3e}")
        assert d <= WEIGHT_MAX, f"{tag} final weights: max |dw| {d:.3e} > {WEIGHT_MAX:.0e}"
