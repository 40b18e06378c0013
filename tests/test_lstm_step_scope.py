"""
Host logic of K21's coverage, without a GPU and without a launch: which LSTM policies PPO.rollout and
get_inference_actions take to ppoaf_lstm_policy_step (PPOPolicy.lstm_step_unsupported_reason), and that the two older
questions -- K6's (fused_step_unsupported_reason) and K19's (inference_unsupported_reason) -- keep their answers.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn


@pytest.fixture(scope="module", autouse=True)
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)


def _ppo(space=None, mode="fused", actor=None, critic=None, obs_dim=4):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.spaces import Box, Discrete
    space = Discrete(2) if space is None else space
    env_gen = lambda: SyntheticFixedLengthEnv(4, obs_dim, space, 40, "cpu", term_prob=0.2)
    sp = Box(-np.inf, np.inf, (obs_dim,), np.float32)
    pargs = dict(ac_network=LSTMNetwork, actor_kw_args=dict(actor or {}), critic_kw_args=dict(critic or actor or {}))
    return PPO(env_gen, {"p": (None, sp, sp, space, pargs)}, device="cpu", envs_per_proc=4, ts_per_rollout=8,
               normalize_obs=False, normalize_rewards=False, update_mode=mode, save_state=False)


def _as_if_on_device(ppo):
    """The coverage question is host arithmetic on shapes and layouts: nothing is launched.  On a device PPO would have
    put the networks of a "fused" LSTM policy on K18 (ppo.py: `use_hip`); the host-built policy is given the same."""
    pol = ppo.policies["p"]
    pol.device = torch.device("cuda", 0)
    if ppo.update_mode == "fused":
        pol.actor.use_hip = pol.critic.use_hip = True
    return pol


def _reason(**kw):
    return _as_if_on_device(_ppo(**kw)).lstm_step_unsupported_reason()


CART_POLE = dict(lstm_hidden_size=32, ff_hidden_size=16, activation=nn.LeakyReLU())     # baselines/gymnasium/cart_pole_lstm.py


def test_covered_shapes():
    from ppo_and_friends_amd.spaces import Box
    assert _reason(actor=CART_POLE) == ""
    assert _reason(space=Box(-1.0, 1.0, (6,), np.float32), obs_dim=17) == ""           # the reference defaults: H 128, ff 128
    # the feed-forward head may differ between the two networks; the LSTM width may not
    assert _reason(actor=dict(lstm_hidden_size=64, ff_hidden_size=16), critic=dict(lstm_hidden_size=64, ff_hidden_size=128,
                                                                                  ff_hidden_depth=2)) == ""


def test_the_policy_lives_on_the_host():
    assert "lives on cpu" in _ppo(actor=CART_POLE).policies["p"].lstm_step_unsupported_reason()


@pytest.mark.parametrize("kw,needles", [
    (dict(actor=dict(lstm_hidden_size=32), critic=dict(lstm_hidden_size=64)), ("hidden sizes differ", "32", "64")),
    (dict(actor=dict(num_lstm_layers=2)), ("2 LSTM layers",)),
    (dict(actor=dict(lstm_hidden_size=48)), ("48",)),
    (dict(space="box9"), ("output width 9",)),
    (dict(mode="torch", actor=CART_POLE), ("update_mode='torch'",)),
    (dict(mode="auto", actor=CART_POLE), ("use_hip", "auto")),
])
def test_refusals_name_their_cause(kw, needles):
    from ppo_and_friends_amd.spaces import Box
    if kw.get("space") == "box9":
        kw = dict(kw, space=Box(-1.0, 1.0, (9,), np.float32))
    why = _reason(**kw)
    assert why != ""
    for n in needles:
        assert n in why, why


def test_the_attribute_switches_the_route_off_and_on():
    pol = _as_if_on_device(_ppo(actor=CART_POLE))
    assert pol.fused_lstm_step is True and pol.lstm_step_unsupported_reason() == ""
    pol.fused_lstm_step = False
    assert "fused_lstm_step" in pol.lstm_step_unsupported_reason()
    pol.fused_lstm_step = True
    assert pol.lstm_step_unsupported_reason() == ""


def test_an_mlp_policy_is_not_k21s():
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    sp = Box(-np.inf, np.inf, (4,), np.float32)
    ppo = PPO(lambda: SyntheticFixedLengthEnv(4, 4, Discrete(2), 40, "cpu"), {"p": (None, sp, sp, Discrete(2), {})},
              device="cpu", envs_per_proc=4, ts_per_rollout=8, save_state=False)
    assert "not an LSTM policy" in ppo.policies["p"].lstm_step_unsupported_reason()


def test_k6_and_k19_keep_their_answers_for_a_covered_policy():
    pol = _as_if_on_device(_ppo(actor=CART_POLE))
    assert pol.lstm_step_unsupported_reason() == ""
    assert "LSTM" in pol.fused_step_unsupported_reason()
    assert "LSTM" in pol.inference_unsupported_reason()


def test_the_library_check_is_part_of_the_answer(monkeypatch):
    """What ppoaf_lstm_policy_step_check refuses is refused by the policy, in the library's words."""
    from ppo_and_friends_amd import kernels as K
    pol = _as_if_on_device(_ppo(actor=CART_POLE))
    monkeypatch.setattr(K, "lstm_policy_step_refusal", lambda a: "lstm_policy_step: refused for the test")
    assert pol.lstm_step_unsupported_reason() == "lstm_policy_step: refused for the test"
