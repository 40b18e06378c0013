"""
-m gpu: a two-layer LSTM policy under PPO(update_mode="fused") with the opt-in `fused_lstm_layers`: one learn iteration on
the cart-pole LSTM shape (H 32, F 16, S 5) runs forward_logits and the mini-batch loop on K18's two-layer launches, never
nn.LSTM, and K21 / K22 launch nothing; the first mini-batch's gradient of every parameter tensor matches float64 under
the project's rule (oracle.k12_oracle.deviations), with the same policy on the nn.LSTM route from the same state as the
float32 leg; without the opt-in the constructor refuses as before.

Worst deviation / bound of the mini-batch gradients (one run on the MI355X): 0.025 of the bound (actor.weight_hh_l0); the nn.LSTM route lay within 2.1e-6 of float64 at a largest gradient of 9.9
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import k12_oracle as ko

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _ppo(layers=2, E=4, T=16, B=8):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    space, sp = Discrete(2), Box(-np.inf, np.inf, (4,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, 4, space, T, DEV, reward="uniform", seed=13, term_prob=0.1)
    kw = dict(sequence_length=5, lstm_hidden_size=32, num_lstm_layers=layers, ff_hidden_size=16)
    return PPO(env_gen, {"p": (None, sp, sp, space, dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
               device=DEV, random_seed=1, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
               batch_size=B, epochs_per_iter=1, max_ts_per_ep=7, save_state=False, update_mode="fused")


def test_two_layer_policy_learns_on_k18(monkeypatch):
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.ppo import PermutationLoader
    calls = {"lstm2_forward": 0, "lstm2_backward": 0, "lstm_policy_step": 0, "lstm_forward": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(K, name, counted)
    monkeypatch.setattr(torch.nn.LSTM, "forward", lambda *a, **k: pytest.fail("nn.LSTM.forward was called under update_mode='fused'"))
    monkeypatch.setattr(PPOPolicy, "fused_lstm_layers", True)
    before = FusedLstmUpdate.launches
    ppo = _ppo()
    pol = ppo.policies["p"]
    assert pol.actor.use_hip and pol.critic.use_hip
    assert pol.lstm_step_unsupported_reason().startswith("2 LSTM layers: K21 covers one")
    w0 = pol.policy_params.clone()
    ppo.rollout()
    assert tuple(pol.buffer.hidden["actor_hidden"].shape[2:]) == (2, 32) and pol.buffer.hidden["actor_hidden"].abs().sum() > 0
    assert tuple(pol.actor.hidden_state[0].shape) == (2, 4, 32)
    pol.train()
    ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator), "p")
    assert calls["lstm2_forward"] > 0 and calls["lstm2_backward"] > 0
    assert calls["lstm_policy_step"] == 0 and calls["lstm_forward"] == 0 and FusedLstmUpdate.launches == before
    assert torch.isfinite(pol.policy_params).all() and not torch.equal(w0, pol.policy_params)
    for k in ("actor loss", "critic loss", "kl avg"):
        assert np.isfinite(ppo.status_dict["p"][k]), k


def _float64_grads(pol, mb, up):
    """The mini-batch gradient of every parameter tensor, actor then critic, as one vector: plain nn.LSTM(I, H, 2),
    LayerNorm and Linear layers in float64 on the CPU holding the policy's parameters, started from the mini-batch's
    stored states, a restated Categorical head, and the loss kernel's d log-prob / d entropy / d value (`up`)."""
    out = []
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        H = net.lstm_hidden_size
        mods = [m.double() for m in [nn.LSTM(net.in_size, H, 2), nn.LayerNorm(H)] + [nn.Linear(i, o) for i, o in net.ff_layers.layer_dims()]]
        params = [p for m in mods for p in m.parameters()]
        with torch.no_grad():
            for p, v in zip(params, net._hip_params()):
                p.copy_(v.detach().cpu())
        x = mb["obs" if tag == "actor" else "critic_obs"].cpu().double().transpose(0, 1)
        state = tuple(mb[f"{tag}_{k}"].cpu().double().transpose(0, 1).contiguous() for k in ("hidden", "cell"))
        z = net.activation(mods[1](mods[0](x, state)[1][0][-1]))
        for lin in mods[2:-1]:
            z = net.activation(lin(z))
        z = mods[-1](z)
        if tag == "actor":
            logp = torch.log_softmax(z, -1)
            lp = logp.gather(1, mb["raw_actions"].cpu().long().reshape(-1, 1)).reshape(-1)
            torch.autograd.backward([lp, -(logp.exp() * logp).sum(-1)], [up[0].cpu().double().reshape(-1), up[1].cpu().double().reshape(-1)])
        else:
            z.reshape(-1).backward(up[2].cpu().double().reshape(-1))
        out += [p.grad.reshape(-1).numpy() for p in params]
    return np.concatenate(out)


def test_first_minibatch_gradients_match_float64_and_the_nn_lstm_route(monkeypatch):
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.ppo import PermutationLoader
    monkeypatch.setattr(PPOPolicy, "fused_lstm_layers", True)
    ups = []
    def loss(*a, _f=K.ppo_loss_fwd_bwd, **k):
        ups.append(_f(*a, **k)[1:])
        return _f(*a, **k)
    monkeypatch.setattr(K, "ppo_loss_fwd_bwd", loss)
    ppo = _ppo()
    pol = ppo.policies["p"]
    ppo.rollout()
    ppo.normalize_values = False                           # (its running statistics would move between the two routes)
    pol.train()
    ds = pol.dataset
    perm = PermutationLoader(ds, ppo.batch_size, ppo.loader_generator).epoch_permutation()[:ppo.batch_size].contiguous()
    mb = {k: v.clone() for k, v in ds.gather_sequences(perm).items()}
    assert tuple(mb["actor_hidden"].shape[1:]) == (2, 32) and mb["actor_hidden"].abs().sum() > 0
    tables = {k: t.clone() for k, t in ds.buffer.hidden.items()}

    def minibatch(use_hip):
        for k, v in tables.items():                        # the step before wrote its final states back
            ds.buffer.hidden[k].copy_(v)
        pol.actor.use_hip = pol.critic.use_hip = use_hip
        ppo._minibatch_step("p", ds, perm, None, torch.zeros(9, dtype=torch.float64, device=DEV))
        return np.concatenate([net.flat_grads[o:o + p.numel()].double().cpu().numpy()
                               for net in (pol.actor, pol.critic) for p in net._hip_params()
                               for o in [(p.data_ptr() - net.flat_params.data_ptr()) // 4]])

    got = minibatch(True)
    want32 = minibatch(False)                              # the same policy on nn.LSTM, from the same state
    want64 = _float64_grads(pol, mb, ups[0])
    names = [f"{tag}.{n}" for tag, net in (("actor", pol.actor), ("critic", pol.critic))
             for n in [n for n, _ in net.lstm.named_parameters()] + ["ln_w", "ln_b"] + [f"ff{i}" for i in range(2 * len(net.ff_layers.layer_dims()))]]
    shapes = [tuple(p.shape) for net in (pol.actor, pol.critic) for p in net._hip_params()]
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
    rows = [("", n, int(o), s) for n, o, s in zip(names, offs, shapes)]
    worst = max(ko.deviations(got, want64, want32, rows), key=lambda d: d[1])
    print(f"first mini-batch gradients: worst deviation / bound {worst[1]:.3f} ({worst[0]}); nn.LSTM route against float64 "
          f"max |diff| {np.abs(want32 - want64).max():.3g} of max |gradient| {np.abs(want64).max():.3g}")
    bad = ko.failures(got, want64, want32, rows)
    assert not bad, "; ".join(bad[:6])


def test_without_the_opt_in_two_layers_are_refused():
    with pytest.raises(NotImplementedError, match="2 LSTM layers"):
        _ppo()
