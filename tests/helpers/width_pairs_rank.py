"""
One rank of tests/test_gpu_k12_width_pairs.py's two-process runs (spawned by that test, never collected): the `wide_tail`
shape of tests/test_gpu_two_ranks.py with a 64-wide actor of depth 1 beside a 256-wide critic of depth 2 -- three agents share
the policy, the critic sees the concatenated observations -- for one iteration of two epochs under update_mode="fused" on
N = 2 ranks that share the one GPU (collectives over gloo).  The result goes to <dir>/<mode>_rank<r>.pt.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

WIDTHS, DEPTHS, SEED = (64, 256), (1, 2), 11


def rank_main(rank, world, port, out_dir, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0", PPOAF_GRAD_EXCHANGE=mode,
                      PPOAF_SHARE_DEVICE="1")          # one GPU for both ranks
    import torch.distributed as dist
    from ppo_and_friends_amd.utils import mpi_utils
    mpi_utils.init_process_group_from_env(backend="gloo")
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, O, NA, B, A = 8, 32, 18, 5, 32, 3
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=79, rank=rank,
                                              num_agents=A, critic_view="policy")
    sp, csp = Box(-np.inf, np.inf, (O,), np.float32), Box(-np.inf, np.inf, (A * O,), np.float32)
    settings = {"p": (None, sp, csp, Discrete(NA), dict(actor_kw_args=dict(hidden_size=WIDTHS[0], hidden_depth=DEPTHS[0]),
                                                         critic_kw_args=dict(hidden_size=WIDTHS[1], hidden_depth=DEPTHS[1])))}
    ppo = PPO(env_gen, settings, device=dev, random_seed=SEED, normalize_obs=False, normalize_rewards=False,
              envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode="fused")
    pol = ppo.policies["p"]
    assert pol.fused_step_unsupported_reason() == ""
    w0 = pol.policy_params.detach().cpu().clone()
    ppo.rollout()
    ppo.train_on_rollout()
    torch.cuda.synchronize()
    fused = [f for f in getattr(ppo, "_fused", {}).values() if f is not None]
    res = dict(peer_exchange=[getattr(f, "xchg", None) is not None for f in fused],
               split=[bool(getattr(f, "split", False)) for f in fused],
               tail=[f.tail_reason() == "" for f in fused], pairs=[f.pairs_reason() == "" for f in fused],
               stats={k: float(v) for k, v in ppo.status_dict["p"].items()
                      if isinstance(v, (int, float)) and not isinstance(v, bool)},
               w0=w0, w=pol.policy_params.detach().cpu().clone(), obs=ppo.env.obs_table.cpu().clone())
    torch.save(res, os.path.join(out_dir, f"{mode}_rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
