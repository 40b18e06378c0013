"""
-m gpu: tests/test_gpu_lstm_layers_step_policy.py's set-up (tilted cart-poles, E 20, T 6, episodes cut at 3) and rules
(bound, envs left out at a near tie) for a 256-wide LSTM policy under `fused_lstm_wide`: with `fused_lstm_wide_step` the
rollout and one evaluation run on csrc/lstm_wide_step.hip and the buffer matches the route without it, per tensor (measured
on the MI355X: 0.000 of the bound in every tensor); without it route and message are today's.
"""
import numpy as np
import pytest

from test_gpu_lstm_layers_step_policy import DEV, E, T, _env, cap

pytestmark = pytest.mark.gpu


def _rollout(monkeypatch, step_opt_in):
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.spaces import Discrete
    calls = {"lstm_policy_step": 0, "lstm_critic_next": 0, "lstm_policy_infer": 0, "lstm_forward": 0}
    for name in calls:
        def counted(*a, _f=getattr(K, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(K, name, counted)
    monkeypatch.setattr(PPOPolicy, "fused_lstm_wide", True)
    monkeypatch.setattr(PPOPolicy, "fused_lstm_wide_step", step_opt_in)
    sp = _env().observation_space
    kw = dict(sequence_length=3, lstm_hidden_size=256, ff_hidden_size=16)
    ppo = PPO(_env, {"p": (None, sp, sp, Discrete(2), dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
              device=DEV, random_seed=3, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=E * (T - 2), epochs_per_iter=1, max_ts_per_ep=3, save_state=False, update_mode="fused")
    ppo.rollout()
    buf = ppo.policies["p"].buffer
    out = {k: getattr(buf, k).double().cpu().numpy().reshape(T, E, -1) for k in ("actions", "log_probs", "values", "boot_value")}
    out.update({k: v.double().cpu().numpy().reshape(T, E, -1) for k, v in buf.hidden.items()})
    out["end_kind"] = buf.end_kind.cpu().numpy().reshape(-1, E)[:T]
    return ppo, out, calls


def test_rollout_buffer_matches_the_route_without_the_step_opt_in(monkeypatch):
    from ppo_and_friends_amd.testing import test_policy as run_test_policy
    ppo, on, calls = _rollout(monkeypatch, True)
    pol = ppo.policies["p"]
    assert pol.lstm_step_unsupported_reason() == "" and pol.lstm_step_hint() == ""
    assert calls["lstm_policy_step"] == T and calls["lstm_forward"] == 0, calls
    info = run_test_policy(ppo, 4, deterministic=True, max_steps=400)
    assert calls["lstm_policy_infer"] > 0 and info["num_test_runs"] == 4 and np.isfinite(info["p"]["avg_score"])
    _, off, calls_off = _rollout(monkeypatch, False)
    assert calls_off["lstm_policy_step"] == 0 and calls_off["lstm_forward"] >= 2 * T, calls_off
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
    # the stored rows of the envs that terminated at a step are zero, the others are not
    ended = on["end_kind"] == 1
    assert ended[0, ::4].all() and 5 <= ended.sum() < ended.size // 2, "the tilted poles did not terminate at step 0"
    for k in ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell"):
        assert not on[k][ended].any() and np.abs(on[k][~ended]).sum(-1).all(), k


def test_without_the_step_opt_in_the_route_and_message_are_todays(monkeypatch):
    ppo, _, calls = _rollout(monkeypatch, False)
    pol = ppo.policies["p"]
    assert pol.lstm_step_unsupported_reason() == "LSTM hidden size 256: K21 covers 32, 64, 128; forward_logits on K18 steps the policy"
    assert "fused_lstm_wide_step" in pol.lstm_step_hint() and calls["lstm_policy_step"] == 0
