"""Child process of test_gpu_action_heads.py::test_multi_rank_rehearsal_matches_single_rank: one PPO iteration of a
MultiDiscrete policy under update_mode="fused" (K6+K7 rollout, K12 update); with PPOAF_REHEARSE_MULTI_RANK=1 the one rank
takes the N > 1 path.  Writes the final parameters and the epoch statistics to the .npz named on the command line."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ppo_and_friends_amd.utils import mpi_utils  # noqa: E402
from ppo_and_friends_amd.ppo import PPO  # noqa: E402
from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv  # noqa: E402
from ppo_and_friends_amd.spaces import Box, MultiDiscrete  # noqa: E402

mpi_utils.init_process_group_from_env()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
E, T, B, O = 16, 32, 64, 6
space = MultiDiscrete([3, 2, 2])
env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=11, term_prob=0.05)
sp = Box(-np.inf, np.inf, (O,), np.float32)
ppo = PPO(env_gen, {"p": (None, sp, sp, space, {})}, device=dev, random_seed=4, normalize_obs=False,
          normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2,
          update_mode="fused", save_state=False)
ppo.rollout()
ppo.train_on_rollout()
pol, sd = ppo.policies["p"], ppo.status_dict["p"]
upd = ppo._fused_updater("p", B)
np.savez(sys.argv[1], params=pol.policy_params.detach().cpu().numpy(), multi=np.array(bool(upd.multi)),
         stats=np.array([sd["actor loss"], sd["critic loss"], sd["kl avg"], sd["weighted entropy"]], dtype=np.float64))
print("done", flush=True)
