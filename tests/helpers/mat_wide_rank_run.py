"""Child process of test_gpu_mat_wide_obs.py::test_multi_rank_rehearsal_matches_single_rank: one PPO iteration of a
MATPolicy with 71-wide observations under update_mode="fused" (K16 rollout, K15 update); with PPOAF_REHEARSE_MULTI_RANK=1
the one rank takes the N > 1 path.  Writes the final parameters and the epoch statistics to the .npz named on the command
line."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ppo_and_friends_amd.utils import mpi_utils  # noqa: E402
from ppo_and_friends_amd.ppo import PPO  # noqa: E402
from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv  # noqa: E402
from ppo_and_friends_amd.policies.mat_policy import MATPolicy  # noqa: E402
from ppo_and_friends_amd.spaces import Box, Discrete  # noqa: E402

mpi_utils.init_process_group_from_env()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
A, O, NA, E, T, B = 3, 71, 5, 8, 12, 20
env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
sp = Box(-np.inf, np.inf, (O,), np.float32)
ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=dev, random_seed=6, normalize_obs=False,
          normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode="fused",
          save_state=False)
pol, sd = ppo.policies["mat"], ppo.status_dict["mat"]
assert pol.fused_step_unsupported_reason() == ""
ppo.rollout()
ppo.train_on_rollout()
upd = ppo._fused_updater("mat", B)
np.savez(sys.argv[1], params=pol.policy_params.detach().cpu().numpy(), multi=np.array(bool(upd.multi)),
         stats=np.array([sd["actor loss"], sd["critic loss"], sd["kl avg"], sd["weighted entropy"]], dtype=np.float64))
print("done", flush=True)
