"""Child process of tests/test_gpu_wide_ranks.py::test_c_loop_equals_the_python_loop: tests/helpers/rccl_fallback_run.py for a
(256, 512) policy with PPOPolicy.fused_wide_ranks -- one rank takes the N > 1 path (PPOAF_REHEARSE_MULTI_RANK=1, RCCL
all-reduce exchange) for two iterations, the split-wgrad chain from ppoaf_ppo_update_chain_allreduce (PPOAF_TEST_RCCL_LOOP=c)
or from the Python loop (=python), and prints a digest of the result."""
import hashlib, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ppo_and_friends_amd.utils import mpi_utils
from ppo_and_friends_amd.ppo import PPO
from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
from ppo_and_friends_amd.spaces import Box, Discrete
from ppo_and_friends_amd import fused_update

# (test-side knob of this helper, not a switch of the package: which of the two fallback loops issues the launches)
fused_update.FusedPolicyUpdate.rccl_loop = os.environ.get("PPOAF_TEST_RCCL_LOOP", "c")
PPOPolicy.fused_wide_ranks = True
mpi_utils.init_process_group_from_env()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
E, T, B, O = 8, 16, 24, 8                                    # 5 full mini-batches and a tail of 8 per epoch
sp = Box(-np.inf, np.inf, (O,), np.float32)
env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(4), T, dev, reward="uniform", seed=11, term_prob=0.05)
pargs = dict(actor_kw_args=dict(hidden_size=256, hidden_depth=2), critic_kw_args=dict(hidden_size=512, hidden_depth=2))
ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(4), pargs)}, device=dev, random_seed=4, normalize_obs=False,
          normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode="fused",
          save_state=False)
for _ in range(2):
    ppo.rollout(); ppo.train_on_rollout()
pol = ppo.policies["p"]
h = hashlib.sha256()
for t in (pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq):
    h.update(t.detach().cpu().numpy().tobytes())
upd, = [f for f in ppo._fused.values() if f is not None]
used_c = fused_update.FusedPolicyUpdate._rccl_comm_cache not in ("unset", None)
print("RESULT " + json.dumps({"digest": h.hexdigest(), "c_loop": bool(used_c), "wide": bool(upd.wide), "split": bool(upd.split),
                              "multi": bool(upd.multi), "peer_exchange": upd.xchg is not None, "description": upd.description(),
                              "critic_loss": float(ppo.status_dict["p"]["critic loss"]),
                              "steps": int(pol.policy_step_counts[0].item())}), flush=True)
