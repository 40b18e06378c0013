"""
One rank of tests/test_gpu_lstm_update.py's two-process run (started by that test, never collected): a rollout and two
update epochs of an LSTM policy on N = 2 ranks through K22 (FusedLstmUpdate: the gradient exchange between the wgrad and
the Adam launch), then the same from the same starting weights through the mini-batch loop (fused_lstm_update = False);
what the test compares goes to <dir>/rank<r>.pt.
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
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    from ppo_and_friends_amd.ppo import PPO, PermutationLoader
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, B, O, NA, S = 6, 20, 16, 5, 3, 4
    kw = dict(sequence_length=S, lstm_hidden_size=32, ff_hidden_size=16)
    res = {}
    for leg in ("k22", "loop"):
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=13, term_prob=0.05, rank=rank)
        sp = Box(-np.inf, np.inf, (O,), np.float32)
        ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), dict(ac_network=LSTMNetwork, actor_kw_args=dict(kw),
                                                                 critic_kw_args=dict(kw)))},
                  device=dev, random_seed=3, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
                  batch_size=B, epochs_per_iter=2, max_ts_per_ep=7, save_state=False, update_mode="fused")
        pol = ppo.policies["p"]
        if leg == "k22":
            start = pol.policy_params.detach().clone()
        else:
            pol.fused_lstm_update = False
            with torch.no_grad():
                pol.policy_params.copy_(start)
        upd = ppo._fused_updater("p", B)
        assert isinstance(upd, FusedLstmUpdate) == (leg == "k22")
        res["w0_" + leg] = pol.policy_params.detach().cpu().clone()
        ppo.rollout()
        pol.train()
        launches = FusedLstmUpdate.launches
        for _ in range(2):
            ppo._ppo_batch_train(PermutationLoader(pol.dataset, B, ppo.loader_generator), "p")
        torch.cuda.synchronize()
        sd = ppo.status_dict["p"]
        res.update({"w_" + leg: pol.policy_params.detach().cpu().clone(),
                    "exp_avg_" + leg: pol.policy_exp_avg.detach().cpu().clone(),
                    "exp_avg_sq_" + leg: pol.policy_exp_avg_sq.detach().cpu().clone(),
                    "steps_" + leg: pol.policy_step_counts.cpu().clone(),
                    "actions_" + leg: pol.buffer.actions.cpu().clone(),
                    "stats_" + leg: [float(sd[k]) for k in ("actor loss", "critic loss")]})
        if leg == "k22":
            res.update(launches=FusedLstmUpdate.launches - launches, n_done=upd.n_done, obs=ppo.env.obs_table.cpu().clone(),
                       exchange="peer" if upd.xchg is not None else "allreduce")
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
