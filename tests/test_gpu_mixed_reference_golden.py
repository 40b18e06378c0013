"""
-m gpu: a multi-policy run against the UNMODIFIED reference (fixture tests/golden/g14_mixed_mat.npz, recorded by
tests/golden/make_golden_mixed.py): three agents, agent0 on a PPOPolicy and {agent1, agent2} on a MATPolicy team,
Discrete(3), two iterations of the reference's own PPO object.  The product replays it on the torch path through
`PPO.rollout` (the recorded raw actions as a dict per policy, the team's recorded shuffles) and `_ppo_batch_train` with
the recorded shuffles of both loaders: per-policy datasets, epoch statistics, final weights, rollout and global status.

Quantities behind optimiser steps are bounded as in tests/test_gpu_reference_golden.py: MARGIN x the deviation measured
on an MI355X (tests/golden/measured_deviations_mixed.json; rerecord with PPOAF_RECORD_MIXED_DEVIATIONS=<file>), at least
the float32 resolution floor.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 4.0                                        # the margin of tests/test_gpu_reference_golden.py
_MEASURED_FILE = os.path.join(HERE, "golden", "measured_deviations_mixed.json")
try:
    with open(_MEASURED_FILE) as _fh:
        MEASURED = json.load(_fh)
except OSError:
    MEASURED = {}
_RECORDED = {}


def _bound(case, key, value, floor):
    rec = os.environ.get("PPOAF_RECORD_MIXED_DEVIATIONS")
    if rec:
        slot = _RECORDED.setdefault(case, {})
        slot[key] = max(float(value), slot.get(key, 0.0))
        with open(rec, "w") as fh:
            json.dump(_RECORDED, fh, indent=1, sort_keys=True)
        return
    assert case in MEASURED and key in MEASURED[case], f"no measured deviation for {case} / {key}"
    limit = max(MARGIN * MEASURED[case][key], floor)
    assert value <= limit, f"{case} {key}: {value:.3e} > {limit:.3e} (= max({MARGIN} x measured {MEASURED[case][key]:.3e}, {floor:.0e}))"


class FixedPermLoader:
    """The loader surface PPO._ppo_batch_train reads, replaying one recorded shuffle."""

    def __init__(self, dataset, batch_size, perm):
        self.dataset, self.batch_size = dataset, int(batch_size)
        self._perm = torch.as_tensor(np.asarray(perm, dtype=np.int64), device=dataset.device)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def epoch_permutation(self):
        return self._perm

    def prefetch(self):
        pass


def test_product_reproduces_the_reference_mixed_iterations(golden):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.spaces import Box, Discrete
    g = golden("g14_mixed_mat")
    c = dict(zip([str(x) for x in g["cfg_names"]], [int(x) for x in g["cfg"]]))
    E, T, A, O, NA, B = c["E"], c["T"], c["A"], c["O"], c["NA"], c["batch_size"]
    dev = torch.device("cuda", 0)
    agents = [f"agent{a}" for a in range(A)]
    assert [str(p) for p in g["policy_ids"]] == ["solo", "team"] and not g["term_table"].any()
    assert [str(p) for p in g["epoch_order"]] == (["solo"] * c["epochs"] + ["team"] * c["epochs"]) * c["iterations"]

    class FixtureEnv(SyntheticMixedAgentsEnv):
        def __init__(self):
            super().__init__(E, [(a, O, Discrete(NA)) for a in agents], T, dev)
            self.obs_table = {a: torch.from_numpy(np.ascontiguousarray(g["obs_table"][:, :, i])).to(dev) for i, a in enumerate(agents)}
            self.reward_table = {a: torch.from_numpy(np.ascontiguousarray(g["reward_table"][:, :, i])).to(dev)
                                 for i, a in enumerate(agents)}

    sp = Box(-np.inf, np.inf, (O,), np.float32)
    narrow = dict(hidden_size=32)
    settings = {"solo": (None, sp, sp, Discrete(NA), dict(actor_kw_args=narrow, critic_kw_args=dict(narrow))),
                "team": (MATPolicy, sp, sp, Discrete(NA), {})}
    team_ids = [str(a) for a in g["team_agent_ids"]]
    ppo = PPO(FixtureEnv, settings, policy_mapping_fn=lambda a: "team" if a in team_ids else "solo", device=dev,
              random_seed=c["seed"], normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=B, epochs_per_iter=c["epochs"], max_ts_per_ep=200, update_mode="torch", save_state=False)
    solo, team = ppo.policies["solo"], ppo.policies["team"]
    assert [str(a) for a in solo.agent_ids] == [str(a) for a in g["solo_agent_ids"]] == ["agent0"]
    for tag, net in (("actor", solo.actor), ("critic", solo.critic)):
        sd = {k[len(f"solo_init_{tag}."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"solo_init_{tag}.")}
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and not [m for m in missing if "dist_m" not in m], (tag, missing, unexpected)
    sd0 = {"actor." + k[len("team_init_actor."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("team_init_actor.")}
    sd0.update({"critic." + k[len("team_init_critic."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("team_init_critic.")})
    missing, unexpected = team.actor_critic.load_state_dict(sd0, strict=False)
    assert not [m for m in missing if "mask" not in m] and not [u for u in unexpected if "mask" not in u], (missing, unexpected)
    # the reference's agent orders: the one the team had after finalize, then one recorded shuffle per rollout
    team.agent_ids = np.array(team_ids)
    orders = iter(g["team_slot_orders"])

    def recorded_shuffle():
        team.agent_ids = np.array([str(a) for a in next(orders)])
    team.shuffle_agent_ids = recorded_shuffle

    tol = dict(rtol=1e-5, atol=1e-5)
    raw = g["step_raw_actions"]                                            # [steps, E, A, .]
    ep = {"solo": 0, "team": 0}
    keys = [str(k) for k in g["rollout_status_keys"]]
    gkeys = [str(k) for k in g["global_status_keys"]]
    for it in range(c["iterations"]):
        sl = slice(it * T, (it + 1) * T)
        order = [agents.index(str(a)) for a in g["team_slot_orders"][it]]
        ppo.replay_raw_actions = {
            "solo": torch.from_numpy(np.ascontiguousarray(raw[sl][:, :, 0]).reshape(T, E, -1)).to(dev),
            "team": torch.from_numpy(np.ascontiguousarray(raw[sl][:, :, order])).to(dev)}
        datasets = ppo.rollout()
        assert [team._env_agent_index[a] + 1 for a in team.agent_ids] == order      # (agent0 is the solo policy's)
        for pid, ds in datasets.items():
            pre = f"{pid}_it{it}_ds_"
            shaped = lambda x, k: x.cpu().numpy().reshape(g[pre + k].shape)
            np.testing.assert_array_equal(shaped(ds.observations, "observations"), g[pre + "observations"])
            np.testing.assert_array_equal(shaped(ds.critic_observations, "critic_observations"), g[pre + "critic_observations"])
            np.testing.assert_array_equal(shaped(ds.actions, "actions"), g[pre + "actions"])
            idx = torch.arange(len(ds), device=dev)
            np.testing.assert_allclose(shaped(ds.values[idx], "values"), g[pre + "values"], **tol)
            np.testing.assert_allclose(shaped(ds.log_probs, "log_probs"), g[pre + "log_probs"], **tol)
            np.testing.assert_allclose(shaped(ds.rewards_to_go, "rewards_to_go"), g[pre + "rewards_to_go"], rtol=1e-5, atol=2e-5)
            np.testing.assert_allclose(shaped(ds.advantages, "advantages"), g[pre + "advantages"], rtol=1e-5, atol=2e-5)
            got = [float(ppo.status_dict[pid][k]) for k in keys]
            np.testing.assert_allclose(got, g[f"{pid}_rollout_status"][it], rtol=1e-5, atol=1e-5, err_msg=f"{pid} {keys}")
        gs = ppo.status_dict["global status"]
        np.testing.assert_allclose([float(gs[k]) for k in gkeys], g["global_status"][it], rtol=0, atol=0, err_msg=str(gkeys))
        for pid, pol in ppo.policies.items():
            pol.train()
            sd = ppo.status_dict[pid]
            for _ in range(c["epochs"]):
                ppo._ppo_batch_train(FixedPermLoader(pol.dataset, B, g[f"{pid}_epoch_perms"][ep[pid]]), pid)
                got = np.array([sd["actor loss"], sd["critic loss"], sd["kl avg"], sd["weighted entropy"]], dtype=np.float64)
                want = g[f"{pid}_epoch_stats"][ep[pid]]
                _bound(f"g14_mixed_mat/torch/{pid}", "stat_dev", float(np.max(np.abs(got - want) / (0.1 + np.abs(want)))), 2e-6)
                ep[pid] += 1
            pol.clear_dataset()

    def check_weights(case, tag, named, prefix, final):
        got = np.concatenate([p.detach().cpu().numpy().reshape(-1) for _, p in named])
        want = np.concatenate([final[prefix + k].reshape(-1) for k, _ in named])
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        _bound(case, f"{tag}_weight_max", float(d.max()), 2e-6)
        _bound(case, f"{tag}_weight_share", float(np.mean(d > 2e-5)), 1e-4)
    for tag, net in (("actor", solo.actor), ("critic", solo.critic)):
        check_weights("g14_mixed_mat/torch/solo", tag, list(net.named_parameters()), f"solo_final_{tag}.", g)
    final = {"actor." + k[len("team_final_actor."):]: g[k] for k in g.files if k.startswith("team_final_actor.")}
    final.update({"critic." + k[len("team_final_critic."):]: g[k] for k in g.files if k.startswith("team_final_critic.")})
    check_weights("g14_mixed_mat/torch/team", "actor_critic", list(team.actor_critic.named_parameters()), "", final)
