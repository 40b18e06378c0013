#!/usr/bin/env python3
"""
Golden vectors for a MULTI-POLICY run (fixture g14_mixed_mat), recorded from the *unmodified* reference with the recipe
and the table-driven environment of make_golden_update.py: three agents, agent0 on a PPOPolicy and {agent1, agent2} on a
MATPolicy team (ppo.py:329-345,710-858: `policy_mapping_fn`), Discrete actions, two iterations of the reference's own PPO
object -- rollout, per-policy datasets, the shuffles of both policies' loaders in the order the one generator serves
them, epoch statistics, final weights, status.  envs_per_proc = 1 as for g12_c5_mat (quirk Q13: the reference's
autoregressive rollout only broadcasts for E = 1).

Usage:  PYTHONHASHSEED=0 python tests/golden/make_golden_mixed.py
"""
import copy
import os
import sys
import tempfile

sys.dont_write_bytecode = True
if os.environ.get("PYTHONHASHSEED") != "0":
    # PPOPolicy.register_agent orders a policy's agents through a set of strings (policies/ppo_policy.py:375-376)
    raise SystemExit("run with PYTHONHASHSEED=0 so that regenerating the fixture reproduces it bit for bit")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
import make_golden_update as U  # noqa: E402

SEED, E, T, A, O, NA, B, EPOCHS, ITERATIONS = 141, 1, 16, 3, 6, 3, 8, 2, 2
TEAM = ("agent1", "agent2")


def main():
    from gymnasium.spaces import Discrete
    from torch.utils.data import DataLoader
    from ppo_and_friends.ppo import PPO
    from ppo_and_friends.networks.ppo_networks.feed_forward import FeedForwardNetwork
    from ppo_and_friends.policies.mat_policy import MATPolicy
    import ppo_and_friends.networks.actor_critic.multi_agent_transformer as mat

    TableEnv = U.table_env_class()
    tables = U.make_tables(SEED, T, E, A, O, "uniform", 0.0)
    pmap = lambda agent_id: "team" if agent_id in TEAM else "solo"
    space = Discrete(NA)
    env_generator = lambda: TableEnv(tables, 0, space, A, critic_view="local", policy_mapping_fn=pmap)
    template = env_generator()
    sp = template.observation_space["agent0"]
    narrow = dict(hidden_size=32)                  # (keeps the fixture small: the weights are most of it)
    settings = {"solo": (None, sp, sp, space, dict(ac_network=FeedForwardNetwork, actor_kw_args=narrow, critic_kw_args=dict(narrow))),
                "team": (MATPolicy, sp, sp, space, dict(ac_network=mat.MATActorCritic, mat_kw_args={"embedding size": 64}))}
    state_dir = tempfile.mkdtemp(prefix="ppoaf_golden_state_")
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    ppo = PPO(env_generator=env_generator, policy_settings=settings, policy_mapping_fn=pmap, device="cpu", random_seed=SEED,
              envs_per_proc=E, max_ts_per_ep=200, batch_size=B, ts_per_rollout=T, epochs_per_iter=EPOCHS, normalize_obs=False,
              normalize_rewards=False, state_path=state_dir, save_train_scores=False, save_ep_scores=False,
              save_avg_ep_len=False, save_running_time=False, save_bs_info=False, checkpoint_every=10 ** 9)
    out = {"cfg_names": np.array(["seed", "E", "T", "A", "O", "NA", "batch_size", "epochs", "iterations"]),
           "cfg": np.array([SEED, E, T, A, O, NA, B, EPOCHS, ITERATIONS], dtype=np.int64),
           "policy_ids": np.array(list(ppo.policies))}
    out["obs_table"], out["reward_table"], out["term_table"] = tables
    for pid, pol in ppo.policies.items():
        out[f"{pid}_agent_ids"] = np.array(list(pol.agent_ids))
        for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
            for k, v in U._flat_state(net).items():
                out[f"{pid}_init_{tag}.{k}"] = v

    rec = {"steps": [], "epochs": [], "datasets": {pid: [] for pid in ppo.policies}, "slot_orders": [], "status": []}
    orig_actions = ppo.get_rollout_actions

    def rec_actions(obs):
        raw, act, lp = orig_actions(obs)
        rec["steps"].append(dict(raw={a: np.array(raw[a]).copy() for a in raw}, act={a: np.array(act[a]).copy() for a in act},
                                 logp={a: lp[a].detach().numpy().copy() for a in lp}))
        return raw, act, lp
    ppo.get_rollout_actions = rec_actions

    team = ppo.policies["team"]
    orig_shuffle = team.shuffle_agent_ids

    def rec_shuffle():
        orig_shuffle()
        rec["slot_orders"].append(np.array([str(a) for a in team.agent_ids]))
    team.shuffle_agent_ids = rec_shuffle

    def hook_finalize(pid, pol):
        orig = pol.finalize_dataset

        def finalize():
            orig()
            ds = pol.dataset
            d = dict(observations=ds.observations, critic_observations=ds.critic_observations, actions=ds.actions,
                     raw_actions=ds.raw_actions, advantages=ds.advantages, log_probs=ds.log_probs,
                     rewards_to_go=ds.rewards_to_go, values=ds.values)
            rec["datasets"][pid].append({k: v.detach().cpu().numpy().copy() for k, v in d.items()})
        pol.finalize_dataset = finalize
    for pid, pol in ppo.policies.items():
        hook_finalize(pid, pol)

    orig_train = ppo._ppo_batch_train

    def rec_train(data_loader, policy_id):
        state = torch.get_rng_state()
        probe = DataLoader(data_loader.dataset, batch_size=data_loader.batch_size, shuffle=True)
        perm = torch.cat([b[12] for b in probe]).numpy().copy()
        torch.set_rng_state(state)
        orig_train(data_loader, policy_id)
        sd = ppo.status_dict[policy_id]
        rec["epochs"].append(dict(policy=policy_id, perm=perm, stats=np.array(
            [sd["actor loss"], sd["critic loss"], sd["kl avg"], sd["weighted entropy"]], dtype=np.float64)))
    ppo._ppo_batch_train = rec_train

    orig_rollout = ppo.rollout

    def rec_rollout():
        orig_rollout()
        rec["status"].append(copy.deepcopy(ppo.status_dict))
    ppo.rollout = rec_rollout

    ppo.learn(E * T * ITERATIONS)

    agents = [f"agent{a}" for a in range(A)]
    stack = lambda key: np.stack([np.stack([s[key][a] for a in agents], 1) for s in rec["steps"]])     # [steps, E, A, ...]
    out["step_raw_actions"], out["step_actions"], out["step_log_probs"] = stack("raw"), stack("act"), stack("logp")
    out["team_slot_orders"] = np.stack(rec["slot_orders"])                      # [rollouts, 2] agent ids, slot by slot
    for pid in ppo.policies:
        for i, d in enumerate(rec["datasets"][pid]):
            for k, v in d.items():
                out[f"{pid}_it{i}_ds_{k}"] = v
        eps = [e for e in rec["epochs"] if e["policy"] == pid]
        out[f"{pid}_epoch_perms"] = np.stack([e["perm"] for e in eps])
        out[f"{pid}_epoch_stats"] = np.stack([e["stats"] for e in eps])
        pol = ppo.policies[pid]
        for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
            for k, v in U._flat_state(net).items():
                out[f"{pid}_final_{tag}.{k}"] = v
        keys = ["score avg", "natural score avg", "top score", "top natural reward"]
        out[f"{pid}_rollout_status"] = np.array([[float(s[pid][k]) for k in keys] for s in rec["status"]])
    out["epoch_order"] = np.array([e["policy"] for e in rec["epochs"]])         # whose loader drew, draw by draw
    out["rollout_status_keys"] = np.array(["score avg", "natural score avg", "top score", "top natural reward"])
    gkeys = ["total episodes", "longest episode", "shortest episode", "average episode", "timesteps"]
    out["global_status_keys"] = np.array(gkeys)
    out["global_status"] = np.array([[float(s["global status"][k]) for k in gkeys] for s in rec["status"]])
    import shutil
    shutil.rmtree(state_dir, ignore_errors=True)
    path = os.path.join(HERE, "g14_mixed_mat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    scratch = ref_import.make_scratch()
    try:
        main()
    finally:
        ref_import.drop_scratch(scratch)
