"""
Shared by tests/test_mixed_policies.py and tests/test_gpu_mixed_policies.py (torch path and fused path): the
restriction property of a multi-policy run.  The synthetic envs are table-driven, so a member's data does not depend on
the other members' actions: a member of a mixed run must log, and then learn, exactly what it logs and learns ALONE in
`PPO.rollout` on an env restricted to its agents with the same tables, the same replayed raw actions, the same agent
permutations and the same mini-batch shuffles.
"""
import numpy as np
import torch

from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv, SyntheticMixedAgentsEnv
from ppo_and_friends_amd.policies.mat_policy import MATPolicy
from ppo_and_friends_amd.spaces import Box, Discrete

E, T, B = 10, 16, 32
# the mixed shape of tests/test_gpu_end_to_end.py (mpe_simple_adversary's dims)
SPECS = [("adversary_0", 8, Discrete(5)), ("agent_0", 10, Discrete(3)), ("agent_1", 10, Discrete(3))]
# the team is agents {0, 2} of the env
SPLIT_SPECS = [("agent_0", 10, Discrete(3)), ("adversary_0", 8, Discrete(5)), ("agent_1", 10, Discrete(3))]
TWO_TEAMS = [("red_0", 8, Discrete(5)), ("red_1", 8, Discrete(5)), ("blue_0", 10, Discrete(3)), ("blue_1", 10, Discrete(3)),
             ("blue_2", 10, Discrete(3))]
ICM = dict(enable_icm=True)
BUFFER_FIELDS = ("observations", "critic_observations", "next_observations", "actions", "raw_actions", "log_probs", "values",
                 "rewards", "end_kind", "boot_value", "boot_reward", "boot_stats")


def box(n):
    return Box(-np.inf, np.inf, (n,), np.float32)


def member_sets():
    """name -> (agent specs, {policy_id: (class, agent-id prefix, policy args)})."""
    adv = lambda **k: (None, "adversary", dict(k))
    team = lambda **k: (MATPolicy, "agent", dict(k))
    return {
        "ppo+mat": (SPECS, {"adversary": adv(), "team": team()}),
        "ppo+mat split": (SPLIT_SPECS, {"adversary": adv(), "team": team()}),
        "ppo_icm+mat": (SPECS, {"adversary": adv(**ICM), "team": team()}),
        "ppo+mat_icm": (SPECS, {"adversary": adv(), "team": team(enable_icm=True, agent_shared_icm=False)}),
        "ppo+mat_shared_icm": (SPECS, {"adversary": adv(), "team": team(enable_icm=True, agent_shared_icm=True)}),
        # a member whose shapes the fused step does not cover (mpe_simple_tag's 256 / 512 MAPPO critic) beside a fused team
        "ppo_wide+mat": (SPECS, {"adversary": adv(actor_kw_args=dict(hidden_size=256), critic_kw_args=dict(hidden_size=512)),
                                 "team": team()}),
        "mat+mat": (TWO_TEAMS, {"red": (MATPolicy, "red", {}), "blue": (MATPolicy, "blue", dict(lr=1e-3))}),
    }


class RestrictedEnv(SyntheticFixedLengthEnv):
    """The agents `agents` of a SyntheticMixedAgentsEnv as an env of their own: the same tables, agent-major."""

    def __init__(self, mixed, agents, device):
        spec = mixed.observation_space[agents[0]]
        super().__init__(mixed.num_envs, spec.shape[0], mixed.action_space[agents[0]], mixed.horizon, device, reward="uniform",
                         term_prob=0.5, num_agents=len(agents))
        self.agent_ids = list(agents)
        self.obs_table = self.critic_obs_table = torch.cat([mixed.obs_table[a] for a in agents], 1).clone()
        self.reward_table = torch.cat([mixed.reward_table[a] for a in agents], 1).clone()
        self.term_table = mixed.term_table.repeat(1, len(agents)).clone()


def raw_env(env):
    while not hasattr(env, "obs_table"):
        env = env.env
    return env


def make_ppo(env_gen, settings, mapping, dev, mode, **kw):
    from ppo_and_friends_amd.ppo import PPO
    args = dict(device=dev, random_seed=8, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
                batch_size=B, epochs_per_iter=2, update_mode=mode, save_state=False, max_ts_per_ep=7, ext_reward_weight=0.37)
    args.update(kw)
    return PPO(env_gen, settings, policy_mapping_fn=mapping, **args)


def settings_of(specs, members):
    dims = {a: (o, sp) for a, o, sp in specs}
    out = {}
    for pid, (cls, prefix, pargs) in members.items():
        o, sp = next(v for a, v in dims.items() if a.startswith(prefix))
        out[pid] = (cls, box(o), box(o), sp, dict(pargs))
    return out


def mixed_run(name, dev, mode, prepare=None, term_prob=0.05, **kw):
    specs, members = member_sets()[name]
    env_gen = lambda: SyntheticMixedAgentsEnv(E, specs, T, dev, reward="uniform", seed=33, term_prob=term_prob)
    mapping = lambda a: next(pid for pid, (_, prefix, _) in members.items() if a.startswith(prefix))
    ppo = make_ppo(env_gen, settings_of(specs, members), mapping, dev, mode, **kw)
    if prepare is not None:
        prepare(ppo)
    return ppo, specs, members


def weights(pol):
    """The parameter buckets and Adam moments of a policy."""
    if pol.agent_grouping:
        opt = pol.actor_critic_optim
        out = dict(params=pol.actor_critic.flat_params, m=opt.exp_avg, v=opt.exp_avg_sq)
    else:
        out = dict(params=pol.policy_params, m=pol.policy_exp_avg, v=pol.policy_exp_avg_sq)
    if pol.enable_icm:
        out.update(icm=pol.icm_model.flat_params, icm_m=pol.icm_optim.exp_avg, icm_v=pol.icm_optim.exp_avg_sq)
    return out


def replay_actions(ppo, specs, seed=5):
    """Recorded raw actions per member, in its buffer layout: [T, n*E, 1] (PPO) / [T, E, n, 1] (MAT)."""
    g = torch.Generator().manual_seed(seed)
    n_act = {a: sp.n for a, _, sp in specs}
    out = {}
    for pid, pol in ppo.policies.items():
        n, na = len(pol.agent_ids), n_act[pol.agent_ids[0]]
        shape = (T, E, n, 1) if pol.agent_grouping else (T, n * E, 1)
        out[pid] = torch.randint(0, na, shape, generator=g).to(ppo.device)
    return out


def snapshot(ppo, pid):
    """Everything the rollout left for one policy, as host copies."""
    pol = ppo.policies[pid]
    out = {k: None if getattr(pol.buffer, k, None) is None else getattr(pol.buffer, k).detach().cpu().clone()
           for k in BUFFER_FIELDS}
    out["advantages"] = pol.dataset.advantages.detach().cpu().clone()
    out["rewards_to_go"] = pol.dataset.rewards_to_go.detach().cpu().clone()
    return out


def record_shuffles(pol):
    """Keeps (agent_idxs, agent_ids) after every shuffle_agent_ids of `pol`; returns the list and the state before."""
    before = (pol.agent_idxs.copy(), pol.agent_ids.copy())
    log, inner = [], pol.shuffle_agent_ids

    def shuffle():
        inner()
        log.append((pol.agent_idxs.copy(), pol.agent_ids.copy()))
    pol.shuffle_agent_ids = shuffle
    return before, log


def run_mixed(ppo, specs):
    """rollout + train_on_rollout of the mixed run -> per policy: snapshot, shuffles, generator state at its epochs, result."""
    ppo.replay_raw_actions = replay_actions(ppo, specs)
    start = {pid: {k: v.detach().clone() for k, v in weights(pol).items()} for pid, pol in ppo.policies.items()}
    shuffles = {pid: record_shuffles(pol) for pid, pol in ppo.policies.items() if pol.agent_grouping}
    ppo.rollout()
    snaps = {pid: snapshot(ppo, pid) for pid in ppo.policies}
    gen_state = {}

    def stream_position():
        """Where the shuffle stream stands for the next loader: a permutation drawn ahead by the previous member's last
        epoch is either handed on or put back, so the position is the one before that draw."""
        c = ppo._perm_cache
        if c.get("perm") is not None and c.get("state_before") is not None:
            return c["state_before"].clone()
        return ppo.loader_generator.get_state()
    for pid, pol in ppo.policies.items():
        inner = pol.train
        pol.train = lambda _pid=pid, _f=inner: (gen_state.__setitem__(_pid, stream_position()), _f())[1]
    ppo.train_on_rollout()
    return dict(start=start, shuffles=shuffles, snaps=snaps, gen_state=gen_state,
                end={pid: {k: v.detach().cpu().clone() for k, v in weights(pol).items()} for pid, pol in ppo.policies.items()},
                status={pid: dict(ppo.status_dict[pid]) for pid in ppo.policies},
                global_status=dict(ppo.status_dict["global status"]))


def run_alone(mixed_ppo, rec, pid, members, dev, mode, prepare=None, **kw):
    """The member `pid` alone on its restriction of the mixed env, fed what `run_mixed` recorded for it."""
    cls, prefix, pargs = members[pid]
    mixed_env = raw_env(mixed_ppo.env)
    agents = [a for a in mixed_env.agent_ids if a.startswith(prefix)]
    env_gen = lambda: RestrictedEnv(mixed_env, agents, dev)
    o = mixed_env.observation_space[agents[0]].shape[0]
    ppo = make_ppo(env_gen, {pid: (cls, box(o), box(o), mixed_env.action_space[agents[0]], dict(pargs))}, None, dev, mode, **kw)
    if prepare is not None:
        prepare(ppo)
    pol = ppo.policies[pid]
    with torch.no_grad():
        for k, v in weights(pol).items():
            v.copy_(rec["start"][pid][k])
    if pol.agent_grouping:
        (idxs, ids), log = rec["shuffles"][pid]
        pol.agent_idxs, pol.agent_ids = idxs.copy(), ids.copy()
        feed = iter(log)

        def shuffle():
            pol.agent_idxs, pol.agent_ids = (x.copy() for x in next(feed))
        pol.shuffle_agent_ids = shuffle
    ppo.replay_raw_actions = mixed_ppo.replay_raw_actions[pid]
    ppo.rollout()
    snap = snapshot(ppo, pid)
    ppo.loader_generator.set_state(rec["gen_state"][pid])
    ppo.train_on_rollout()
    return dict(snap=snap, end={k: v.detach().cpu().clone() for k, v in weights(pol).items()},
                status=dict(ppo.status_dict[pid]), global_status=dict(ppo.status_dict["global status"]))


def same_entry(a, b):
    """Two status entries (numbers, tuples of numbers, strings, tensors), bit for bit."""
    if isinstance(a, str) or isinstance(b, str):
        return a == b
    to_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    a, b = to_np(a), to_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_member_equals_alone(name, dev, mode, prepare=None, **kw):
    """The restriction property for every member of the set `name`; returns the mixed run's record."""
    ppo, specs, members = mixed_run(name, dev, mode, prepare, **kw)
    rec = run_mixed(ppo, specs)
    for pid in ppo.policies:
        alone = run_alone(ppo, rec, pid, members, dev, mode, prepare, **kw)
        for k, want in alone["snap"].items():
            got = rec["snaps"][pid][k]
            assert (got is None) == (want is None), f"{name} {pid} {k}"
            if want is not None:
                assert got.shape == want.shape and torch.equal(got, want), f"{name} {pid} {k}"
        for k, want in alone["end"].items():
            assert torch.equal(rec["end"][pid][k], want), f"{name} {pid} {k} after train_on_rollout"
        assert set(rec["status"][pid]) == set(alone["status"]), f"{name} {pid} status keys"
        for k, want in alone["status"].items():
            assert same_entry(rec["status"][pid][k], want), f"{name} {pid} status[{k!r}]: {rec['status'][pid][k]} != {want}"
        assert rec["global_status"]["total episodes"] == alone["global_status"]["total episodes"], f"{name} {pid}"
    assert rec["global_status"]["timesteps"] == E * T
    return ppo, rec


# ---- what the package issues between two env.step calls --------------------------------------------------------------
# operators that only make another view of a tensor's memory: no launch, no copy
PURE_VIEWS = ("aten.select.int", "aten.view.default", "aten._unsafe_view.default", "aten.reshape.default", "aten.unbind.int",
              "aten.alias.default", "aten.slice.Tensor", "aten.detach.default")


def ops_between_env_steps(ppo, run=None):
    """One rollout under a TorchDispatchMode that is suspended inside env.step -> per pair of consecutive env.step calls
    the names of the torch operators that touched a device tensor (what follows step t and what prepares step t + 1)."""
    from torch.utils._python_dispatch import TorchDispatchMode, _disable_current_modes
    log = []

    class DeviceOps(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            flat = list(args) + list((kwargs or {}).values()) + (list(out) if isinstance(out, (tuple, list)) else [out])
            flat = [y for x in flat for y in (x if isinstance(x, (tuple, list)) else [x])]
            if any(torch.is_tensor(x) and x.is_cuda for x in flat):
                log.append(str(func))
            return out
    env = raw_env(ppo.env)
    inner = env.step

    def step(action):
        log.append("env.step")
        with _disable_current_modes():
            return inner(action)
    env.step = step
    try:
        with DeviceOps():
            (run or ppo.rollout)()
    finally:
        env.step = inner
    marks = [i for i, x in enumerate(log) if x == "env.step"]
    return [log[a + 1:b] for a, b in zip(marks[:-1], marks[1:])]


def launching(ops):
    """The operators of one segment that are not pure views."""
    return [o for o in ops if o not in PURE_VIEWS]
