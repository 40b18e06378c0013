"""
The restriction property of tests/helpers/mixed_policies.py extended to LSTM members (`PPO.lstm_members = True`): a
member of the mixed run logs, and then learns, bit for bit what it logs and learns ALONE on the env restricted to its
agents -- every buffer field, the four hidden-state rows, the networks' states after the rollout, advantages,
rewards-to-go, weights and Adam moments after train_on_rollout, status entries and episode counts.

Shapes are the existing helper's (E = 10, so a 16-row tile of a two-agent member straddles its blocks; T = 16, B = 32,
max_ts_per_ep = 7 and term_prob > 0, so terminal and cut ends both occur); LSTM width 32 (64 for the second LSTM member),
ff_hidden_size 16, sequence_length 4; observations 8 and 10 wide.
"""
import torch

import mixed_policies as M
from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv, SyntheticMixedAgentsEnv
from ppo_and_friends_amd.networks.lstm import LSTMNetwork
from ppo_and_friends_amd.policies.mat_policy import MATPolicy
from ppo_and_friends_amd.spaces import Discrete

E, T, B = M.E, M.T, M.B
HIDDEN_KEYS = ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell")
TENSOR_OBS = 8                       # the agent-major tensor env: three agents that share shapes, split 1 + 2


def lstm(width=32, **more):
    net = dict(sequence_length=4, lstm_hidden_size=width, ff_hidden_size=16)
    return dict(ac_network=LSTMNetwork, actor_kw_args=dict(net), critic_kw_args=dict(net), **more)


def cases():
    """name -> (agent specs or None for the tensor env, {policy_id: (class, agent-id prefix, policy args)})."""
    return {
        "lstm+mat": (M.SPECS, {"adversary": (None, "adversary", lstm()), "team": (MATPolicy, "agent", {})}),
        # the LSTM policy owns the non-adjacent agents {0, 2}
        "lstm02+ff": (M.SPLIT_SPECS, {"adversary": (None, "adversary", {}), "pair": (None, "agent", lstm())}),
        "lstm32+lstm64": (M.SPECS, {"adversary": (None, "adversary", lstm(32)), "pair": (None, "agent", lstm(64))}),
        "tensor lstm+ff": (None, {"solo": (None, "agent0", lstm()), "pair": (None, ("agent1", "agent2"), {})}),
        "lstm_icm+mat": (M.SPECS, {"adversary": (None, "adversary", lstm(enable_icm=True)), "team": (MATPolicy, "agent", {})}),
    }


def _owns(prefix, agent_id):
    return agent_id in prefix if isinstance(prefix, tuple) else agent_id.startswith(prefix)


def opt_in(prepare=None):
    def prep(ppo):
        ppo.lstm_members = True                     # on the instance, before the first rollout
        if prepare is not None:
            prepare(ppo)
    return prep


def hidden_snapshot(pol):
    out = {k: pol.buffer.hidden[k].detach().cpu().clone() for k in HIDDEN_KEYS}
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        out[tag + "_state"] = torch.stack([x.detach().cpu().clone() for x in net.hidden_state])
    return out


def capture_hidden(ppo, sink):
    """The hidden rows right after ppo.rollout() (the update writes its windows' states back into them)."""
    inner = ppo.rollout

    def rollout():
        out = inner()
        sink.update({pid: hidden_snapshot(pol) for pid, pol in ppo.policies.items() if pol.using_lstm})
        return out
    ppo.rollout = rollout


def mixed_run(name, dev, mode, prepare=None, term_prob=0.05, **kw):
    specs, members = cases()[name]
    if specs is None:
        space = Discrete(5)
        env_gen = lambda: SyntheticFixedLengthEnv(E, TENSOR_OBS, space, T, dev, reward="uniform", seed=33, term_prob=term_prob,
                                                  num_agents=3)
        specs = [(f"agent{a}", TENSOR_OBS, space) for a in range(3)]
    else:
        env_gen = lambda: SyntheticMixedAgentsEnv(E, specs, T, dev, reward="uniform", seed=33, term_prob=term_prob)
    dims = {a: (o, sp) for a, o, sp in specs}
    settings = {}
    for pid, (cls, prefix, pargs) in members.items():
        o, sp = next(v for a, v in dims.items() if _owns(prefix, a))
        settings[pid] = (cls, M.box(o), M.box(o), sp, dict(pargs))
    mapping = lambda a: next(pid for pid, (_, prefix, _) in members.items() if _owns(prefix, a))
    ppo = M.make_ppo(env_gen, settings, mapping, dev, mode, **kw)
    opt_in(prepare)(ppo)
    return ppo, specs, members


class RestrictedTensorEnv(SyntheticFixedLengthEnv):
    """The agents at positions `index` of an agent-major SyntheticFixedLengthEnv as an env of their own: the same tables."""

    def __init__(self, full, index, device):
        super().__init__(full.num_envs, full.obs_dim, full.action_space, full.horizon, device, reward="uniform", term_prob=0.5,
                         num_agents=len(index))
        A, n, Ev = full.num_agents, len(index), full.num_envs
        take = lambda x: x.reshape((x.shape[0], A, Ev) + tuple(x.shape[2:]))[:, index].reshape((x.shape[0], n * Ev) + tuple(x.shape[2:])).clone()
        self.agent_ids = [full.agent_ids[i] for i in index]
        self.obs_table = self.critic_obs_table = take(full.obs_table)
        self.reward_table = take(full.reward_table)
        self.term_table = take(full.term_table)


def run_alone(mixed_ppo, rec, pid, members, dev, mode, prepare=None, **kw):
    """The member `pid` alone on its restriction of the mixed env, fed what `M.run_mixed` recorded for it -> M.run_alone's
    record plus `hidden`."""
    cls, prefix, pargs = members[pid]
    mixed_env = M.raw_env(mixed_ppo.env)
    agents = [a for a in mixed_env.agent_ids if _owns(prefix, a)]
    if isinstance(mixed_env, SyntheticMixedAgentsEnv):
        env_gen = lambda: M.RestrictedEnv(mixed_env, agents, dev)
        o, space = mixed_env.observation_space[agents[0]].shape[0], mixed_env.action_space[agents[0]]
    else:
        index = [mixed_env.agent_ids.index(a) for a in agents]
        env_gen = lambda: RestrictedTensorEnv(mixed_env, index, dev)
        o, space = mixed_env.obs_dim, mixed_env.action_space
    ppo = M.make_ppo(env_gen, {pid: (cls, M.box(o), M.box(o), space, dict(pargs))}, None, dev, mode, **kw)
    if prepare is not None:
        prepare(ppo)
    pol = ppo.policies[pid]
    with torch.no_grad():
        for k, v in M.weights(pol).items():
            v.copy_(rec["start"][pid][k])
    if pol.agent_grouping:
        (idxs, ids), log = rec["shuffles"][pid]
        pol.agent_idxs, pol.agent_ids = idxs.copy(), ids.copy()
        feed = iter(log)

        def shuffle():
            pol.agent_idxs, pol.agent_ids = (x.copy() for x in next(feed))
        pol.shuffle_agent_ids = shuffle
    ppo.replay_raw_actions = mixed_ppo.replay_raw_actions[pid]
    hidden = {}
    capture_hidden(ppo, hidden)
    ppo.rollout()
    snap = M.snapshot(ppo, pid)
    ppo.loader_generator.set_state(rec["gen_state"][pid])
    ppo.train_on_rollout()
    return dict(snap=snap, hidden=hidden.get(pid), end={k: v.detach().cpu().clone() for k, v in M.weights(pol).items()},
                status=dict(ppo.status_dict[pid]), global_status=dict(ppo.status_dict["global status"]), ppo=ppo)


def run_case(name, dev, mode, prepare=None, **kw):
    """The mixed run of `name` -> (ppo, specs, members, record with `hidden` per LSTM member)."""
    ppo, specs, members = mixed_run(name, dev, mode, prepare, **kw)
    hidden = {}
    capture_hidden(ppo, hidden)
    rec = M.run_mixed(ppo, specs)
    rec["hidden"] = hidden
    return ppo, specs, members, rec


def same_tensors(got, want, what):
    assert set(got) == set(want), what
    for k, w in want.items():
        g = got[k]
        assert (g is None) == (w is None), f"{what} {k}"
        if w is not None:
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), f"{what} {k}"


def assert_member_equals_alone(name, dev, mode, prepare=None, **kw):
    """The restriction property for every member of the case `name`; returns the mixed run's ppo and record."""
    ppo, specs, members, rec = run_case(name, dev, mode, prepare, **kw)
    for pid, pol in ppo.policies.items():
        alone = run_alone(ppo, rec, pid, members, dev, mode, prepare, **kw)
        same_tensors(rec["snaps"][pid], alone["snap"], f"{name} {pid}")
        assert pol.using_lstm == (alone["hidden"] is not None)
        if pol.using_lstm:
            same_tensors(rec["hidden"][pid], alone["hidden"], f"{name} {pid} hidden")
            assert all(rec["hidden"][pid][k].abs().max() > 0 for k in HIDDEN_KEYS)
        same_tensors(rec["end"][pid], alone["end"], f"{name} {pid} after train_on_rollout")
        assert set(rec["status"][pid]) == set(alone["status"]), f"{name} {pid} status keys"
        for k, want in alone["status"].items():
            assert M.same_entry(rec["status"][pid][k], want), f"{name} {pid} status[{k!r}]: {rec['status'][pid][k]} != {want}"
        assert rec["global_status"]["total episodes"] == alone["global_status"]["total episodes"], f"{name} {pid}"
        # the path the member took alone is the one it took in the mixed run
        alone_pol = alone["ppo"].policies[pid]
        assert (getattr(pol, "_lstm_step_state", None) is None) == (getattr(alone_pol, "_lstm_step_state", None) is None)
    assert rec["global_status"]["timesteps"] == E * T
    # terminal and cut ends both occur before the last row
    kinds = next(iter(rec["snaps"].values()))["end_kind"][:-1]
    assert (kinds == 1).any() and (kinds == 2).any()
    return ppo, rec
