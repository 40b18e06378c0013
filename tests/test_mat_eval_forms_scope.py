"""
The opt-in `MATPolicy.fused_mat_eval_forms` (no GPU): off, K20 refuses a Box team and a 71-wide Discrete team in the words it
always had; on, both answers are ""; flipping the attribute asks again; a (3, 18, 5) Discrete policy answers the same either
way.  The policies live on the CPU: a stand-in device type and update_mode let the question past its first two answers.
"""
import types

import numpy as np
import pytest
import torch

BOX_OFF = "K20 covers Discrete actions: the evaluation of a Box team keeps the module decode"
WIDE_OFF = "observations 71 wide: the K20 evaluation step takes up to 64 (K15 and K16 take these)"
HINT = "; MATPolicy.fused_mat_eval_forms = True would take it on the one-launch step"


@pytest.mark.parametrize("kind,O,off", [("box", 18, BOX_OFF), ("wide", 71, WIDE_OFF), ("c5", 18, "")])
def test_off_the_refusals_are_todays_and_on_both_forms_are_taken(kind, O, off):
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.fused_update import mat_eval_hint
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.spaces import Box, Discrete
    cpu, space = torch.device("cpu"), Box(-0.5, 2.0, (5,), np.float32) if kind == "box" else Discrete(5)
    env_gen = lambda: SyntheticFixedLengthEnv(4, O, space, 8, cpu, reward="uniform", seed=41, num_agents=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    pol = PPO(env_gen, {"mat": (MATPolicy, sp, sp, space, {})}, device=cpu, random_seed=6, normalize_obs=False, normalize_rewards=False,
              envs_per_proc=4, ts_per_rollout=32, batch_size=8, use_graphs=False, update_mode="torch").policies["mat"]
    pol.device, pol.update_mode = types.SimpleNamespace(type="cuda"), "auto"      # the stand-in
    pol.fused_mat_eval_forms = True                                      # (a Box team that K16 refuses: in K16's words, either way)
    assert kind != "box" or pol.inference_unsupported_reason() == "the fused MAT update covers Discrete actions"
    del pol.fused_mat_eval_forms
    pol.fused_mat_box_actions = True
    assert pol.inference_unsupported_reason() == off and mat_eval_hint(pol, off) == (HINT if off else "")
    assert "fused_mat_eval_forms" not in vars(pol)                       # (asking wrote nothing)
    pol.fused_mat_eval_forms = True                                      # flipping it asks again
    assert pol.inference_unsupported_reason() == "" and mat_eval_hint(pol, "") == ""
    pol.fused_mat_eval_forms = False
    assert pol.inference_unsupported_reason() == off
