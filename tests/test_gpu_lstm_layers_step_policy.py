"""
-m gpu: a two-layer LSTM policy (H 32, ff 16) on the cart-pole env, E = 20, T = 6, max_ts_per_ep = 3 and every fourth pole
started 0.2 rad over with 0.5 rad/s (it falls at the first step whatever the action: upright poles need eight steps, so
without this no env terminates in six; episodes are cut and terminate inside the rollout), under PPO(update_mode="fused") with `fused_lstm_layers`: with `fused_lstm_layers_step` on, the rollout runs
on the one-launch two-layer step and its buffer matches the buffer of the same seed with the opt-in off (forward_logits
on K18 + torch operators), per tensor.  Bound: both routes are float32 restatements of one float64 computation, each
held to 1e-5 |x| + 1e-5 max|x| of it by the project's rule, so their difference is held to twice that.  An env whose
sampled action differs between the routes (a near tie at a CDF edge) is left out from that step on, at most
mat_step_cases.cap(E) envs.  The hidden rows of terminated envs are zero; test_policy runs on the one-launch step; with the
opt-in off the route and the verbose hint are today's plus the attribute's name.

Worst deviation / bound (one run on the MI355X): 0.000 in every tensor -- the two routes wrote equal values, and no env
took a different action.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from mat_step_cases import cap  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, T = 20, 6


def _env():
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv

    class Tilted(BatchedCartPoleEnv):
        def reset(self):
            super().reset()
            self.state[::4, 2:] = torch.tensor([0.2, 0.5], device=self.device)
            return self.state, self.state
    return Tilted(E, DEV, seed=0)


def _ppo(monkeypatch, step_opt_in):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.spaces import Discrete
    monkeypatch.setattr(PPOPolicy, "fused_lstm_layers", True)
    monkeypatch.setattr(PPOPolicy, "fused_lstm_layers_step", step_opt_in)
    sp = _env().observation_space
    kw = dict(sequence_length=3, lstm_hidden_size=32, num_lstm_layers=2, ff_hidden_size=16)
    return PPO(_env, {"p": (None, sp, sp, Discrete(2), dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
               device=DEV, random_seed=3, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
               batch_size=E * (T - 2), epochs_per_iter=1, max_ts_per_ep=3, save_state=False, update_mode="fused")


def _rollout(monkeypatch, step_opt_in):
    from ppo_and_friends_amd import kernels as K
    calls = {"lstm_policy_step": 0, "lstm_critic_next": 0, "lstm_policy_infer": 0, "lstm2_forward": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(K, name, counted)
    ppo = _ppo(monkeypatch, step_opt_in)
    ppo.rollout()
    buf = ppo.policies["p"].buffer
    out = {k: getattr(buf, k).double().cpu().numpy().reshape(T, E, -1) for k in ("actions", "log_probs", "values", "boot_value")}
    out.update({k: v.double().cpu().numpy().reshape(T, E, -1) for k, v in buf.hidden.items()})
    out["end_kind"] = buf.end_kind.cpu().numpy().reshape(-1, E)[:T]
    return ppo, out, calls


def test_rollout_buffer_matches_the_route_without_the_opt_in(monkeypatch):
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.testing import test_policy as run_test_policy
    ppo, on, calls = _rollout(monkeypatch, True)
    pol = ppo.policies["p"]
    assert pol.lstm_step_unsupported_reason() == "" and isinstance(pol._lstm_step_args(E)["args"], _lib.Lstm2PolicyStepArgs)
    assert calls["lstm_policy_step"] == T and calls["lstm2_forward"] == 0, calls
    assert tuple(pol.actor.hidden_state[0].shape) == (2, E, 32) and pol.actor.hidden_state[0].is_contiguous()
    info = run_test_policy(ppo, 4, deterministic=True, max_steps=400)
    assert calls["lstm_policy_infer"] > 0 and info["num_test_runs"] == 4 and np.isfinite(info["p"]["avg_score"])
    _, off, calls_off = _rollout(monkeypatch, False)
    assert calls_off["lstm_policy_step"] == 0 and calls_off["lstm2_forward"] >= 2 * T, calls_off
    # an env whose sampled action differs (a near tie) is left out from that step on
    differs = (on["actions"] != off["actions"]).any(-1)
    kept = ~(np.cumsum(differs, 0) > 0)
    assert (~kept[-1]).sum() <= cap(E), f"{(~kept[-1]).sum()} envs took different actions"
    assert np.array_equal(on["end_kind"][kept], off["end_kind"][kept])
    assert (on["end_kind"][:-1] == 2).any(), "no episode was cut inside the rollout"
    worst = {}
    for k in ("log_probs", "values", "boot_value", "actor_hidden", "actor_cell", "critic_hidden", "critic_cell"):
        a, b = on[k][kept], off[k][kept]
        bound = 2.0 * (1e-5 * np.abs(b) + 1e-5 * np.abs(off[k]).max())
        worst[k] = float(np.max(np.abs(a - b) / np.maximum(bound, 1e-300)))
    print("worst deviation / bound per tensor: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    # the stored rows of the envs that terminated at a step are zero (an episode cut at max_ts_per_ep keeps its rows, as
    # store_hidden_states keeps them), the others are not
    ended = on["end_kind"] == 1
    assert ended[0, ::4].all() and 5 <= ended.sum() < ended.size // 2, "the tilted poles did not terminate at step 0"
    for k in ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell"):
        assert not on[k][ended].any() and np.abs(on[k][~ended]).sum(-1).all(), k


def test_without_the_step_opt_in_the_route_and_message_are_todays(monkeypatch):
    ppo, _, calls = _rollout(monkeypatch, False)
    pol = ppo.policies["p"]
    why = pol.lstm_step_unsupported_reason()
    assert why == "2 LSTM layers: K21 covers one; forward_logits on K18 steps the policy"
    assert "fused_lstm_layers_step" in pol.lstm_step_hint() and calls["lstm_policy_step"] == 0
