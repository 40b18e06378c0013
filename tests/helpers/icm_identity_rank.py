"""
One rank of tests/test_gpu_icm_identity.py's two-process run (started by that test, never collected): one ICM epoch of the
blind-maze form (identity encoder, O 2, models of width 128) through K14's identity chain on N = 2 ranks -- fused_adam = 0,
the gradient bucket summed over the ranks, then the flat Adam step -- and the same epoch with update_mode="torch"; the
buckets go to <dir>/rank<r>.pt.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(out_dir):
    rank = int(os.environ["RANK"])
    import torch.distributed as dist
    from ppo_and_friends_amd.utils import mpi_utils
    mpi_utils.init_process_group_from_env(backend="gloo")
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    envs, T, B, O, NA = 12, 16, 40, 2, 5
    icm_kw = dict(encoded_obs_dim=0, inverse_hidden_size=128, forward_hidden_size=128)
    res = {}
    for mode in ("fused", "torch"):
        env_gen = lambda: SyntheticFixedLengthEnv(envs, O, Discrete(NA), T, dev, reward="uniform", seed=500, rank=rank)
        sp = Box(-np.inf, np.inf, (O,), np.float32)
        ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(enable_icm=True, icm_kw_args=icm_kw))}, device=dev, random_seed=11,
                  normalize_obs=False, normalize_rewards=False, envs_per_proc=envs, ts_per_rollout=T, batch_size=B, epochs_per_iter=1,
                  update_mode=mode)
        pol = ppo.policies["p"]
        tag = "" if mode == "fused" else "_torch"
        # (the host-side orthogonal init's last bits depend on the intra-op thread count at that moment -- see
        # tests/helpers/initial_weights.py --, so the second leg starts from the first leg's buckets, not from its own draw)
        if mode == "fused":
            start = pol.policy_params.detach().clone(), pol.icm_model.flat_params.detach().clone()
        else:
            with torch.no_grad():
                pol.policy_params.copy_(start[0]); pol.icm_model.flat_params.copy_(start[1])
        res["w0" + tag] = pol.icm_model.flat_params.detach().cpu().clone()       # after the rank-0 broadcast
        upd = ppo._fused_icm_updater("p")
        assert (upd is not None) == (mode == "fused")
        ppo.rollout()
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        ppo._icm_batch_train(loader, "p")
        torch.cuda.synchronize()
        res["w" + tag] = pol.icm_model.flat_params.detach().cpu().clone()
        res["loss" + tag] = float(ppo.status_dict["p"]["icm loss"])
        res["actions" + tag] = pol.buffer.actions.cpu().clone()
        if mode == "fused":
            res.update(identity=bool(upd.topo.get("identity")), exp_avg=pol.icm_optim.exp_avg.detach().cpu().clone(),
                       exp_avg_sq=pol.icm_optim.exp_avg_sq.detach().cpu().clone(), obs=ppo.env.obs_table.cpu().clone())
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
