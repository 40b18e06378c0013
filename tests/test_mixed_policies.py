"""
Multi-policy runs with MATPolicy teams and ICM members, on a CPU device (the torch path; no GPU needed).

What needs no launch: the refusal of LSTM members and of a single replay tensor.  Sampling, log-probs and attention
are HIP kernels on every path, so the rollouts themselves are in tests/test_gpu_mixed_policies.py.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)


def test_a_single_replay_tensor_is_refused_for_several_policies():
    import mixed_policies as M
    ppo, specs, _ = M.mixed_run("ppo+mat", CPU, "torch")
    ppo.replay_raw_actions = torch.zeros(M.T, M.E, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="dict"):
        ppo.rollout()


def test_an_lstm_member_is_refused_by_name():
    import mixed_policies as M
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    specs = M.SPECS
    env_gen = lambda: SyntheticMixedAgentsEnv(M.E, specs, M.T, CPU, reward="uniform", seed=33)
    lstm = dict(ac_network=LSTMNetwork, actor_kw_args=dict(lstm_hidden_size=32), critic_kw_args=dict(lstm_hidden_size=32))
    settings = {"adversary": (None, M.box(8), M.box(8), specs[0][2], lstm),
                "team": (M.MATPolicy, M.box(10), M.box(10), specs[1][2], {})}
    ppo = M.make_ppo(env_gen, settings, lambda a: "adversary" if a.startswith("adversary") else "team", CPU, "torch")
    with pytest.raises(NotImplementedError, match="LSTM") as err:
        ppo.rollout()
    assert "adversary" in str(err.value) and "ICM" not in str(err.value) and "feed-forward" not in str(err.value)
