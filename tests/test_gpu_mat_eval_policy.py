"""
-m gpu: evaluation of multi-agent policies through the host path -- `testing.test_policy` on a MATPolicy drives ONE K20
launch (`ppoaf_mat_policy_infer`) and ONE `ppoaf_eval_scores_step_books` launch per env step, reads the host only for
`remaining`, leaves the training state alone, and its result is the numpy restatement
(tests/helpers/eval_restatement.py) of the traced env; `PPO.get_inference_actions` on the env's agent-major tensor
against the regroup -> module decode -> un-group route it replaces; the module path where K20 does not cover the policy;
and shared-MLP / two-policy envs through the books.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _box(n):
    from ppo_and_friends_amd.spaces import Box
    return Box(-np.inf, np.inf, (n,), np.float32)


def _traced(env_cls):
    """env class -> the same env recording (reward, terminated, truncated) of every step: what the harness is fed."""
    class Traced(env_cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            if torch.is_tensor(getattr(self, "term_table", None)):
                self.term_table[-1] = True                   # every row finishes once per horizon
            self.trace = []

        def step(self, action):
            out = super().step(action)
            self.trace.append((out[2], out[3], out[4]))
            return out
    return Traced


def _trace_arrays(env, E, agent_ids):
    raw = env
    while not hasattr(raw, "trace"):
        raw = raw.env
    if isinstance(raw.trace[0][0], dict):
        score = {a: np.stack([r[a].cpu().numpy() for r, _, _ in raw.trace]) for a in agent_ids}
        done = np.stack([(t[agent_ids[0]] | u[agent_ids[0]]).cpu().numpy() for _, t, u in raw.trace])
        return score, done
    A = len(agent_ids)
    rew = np.stack([r.cpu().numpy().reshape(A, E) for r, _, _ in raw.trace])
    done = np.stack([(t | u).cpu().numpy().reshape(-1)[:E] for _, t, u in raw.trace])
    return {a: rew[:, i] for i, a in enumerate(agent_ids)}, done


def _raw(env):
    while not hasattr(env, "trace"):
        env = env.env
    return env


def _mat_ppo(E=9, A=3, O=18, NA=5, expanded=False, mode="auto", horizon=40, seed=1, shuffled=True, ts=16, **kw):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.spaces import Discrete
    cls = _traced(SyntheticFixedLengthEnv)
    env_gen = lambda: cls(E, O, Discrete(NA), horizon, DEV, reward="uniform", seed=5, term_prob=0.08, num_agents=A,
                          critic_view="policy" if expanded else "local")
    fk = dict(normalize_obs=False, normalize_rewards=False)
    fk.update(kw)
    ppo = PPO(env_gen, {"agent": (MATPolicy, _box(O), _box(O * A if expanded else O), Discrete(NA), {})}, device=DEV,
              random_seed=seed, envs_per_proc=E, ts_per_rollout=ts, batch_size=16, save_state=False, update_mode=mode, **fk)
    pol = ppo.policies["agent"]
    assert pol.expanded_actor_space == expanded
    if shuffled:
        np.random.seed(12)
        while np.array_equal(pol.agent_slot_order(), np.arange(A)):
            pol.shuffle_agent_ids()
    return ppo, pol


class _Counters:
    """Counts K20 launches, module forwards and bookkeeping calls; from the first bookkeeping step on a host
    synchronisation raises, except inside `remaining` / `results`."""

    def __init__(self, pol, monkeypatch, guard_syncs=True):
        from ppo_and_friends_amd import kernels as K
        self.k20, self.modules, self.single, self.books, self.reads = [], [], [], [], []
        infer = K.mat_policy_infer
        monkeypatch.setattr(K, "mat_policy_infer", lambda a: (self.k20.append(a.mode), infer(a))[1])
        for net in (pol.actor, pol.critic):
            inner = net.forward
            monkeypatch.setattr(net, "forward", lambda *a, _f=inner, **k: (self.modules.append(1), _f(*a, **k))[1])
        step1, stepb = K.EvalScores.step, K.EvalScoreBooks.step
        remaining, results = K.EvalScoreBooks.remaining, K.EvalScoreBooks.results
        mode = torch.cuda.set_sync_debug_mode

        def books_step(this, score, done):
            if guard_syncs:
                mode("error")
            self.books.append(1)
            return stepb(this, score, done)

        def books_remaining(this, book=0):
            mode("default")
            try:
                self.reads.append(len(self.books))
                return remaining(this, book)
            finally:
                if guard_syncs:
                    mode("error")

        def books_results(this, book=None):
            mode("default")
            return results(this, book)
        monkeypatch.setattr(K.EvalScores, "step", lambda this, s, d: (self.single.append(1), step1(this, s, d))[1])
        monkeypatch.setattr(K.EvalScoreBooks, "step", books_step)
        monkeypatch.setattr(K.EvalScoreBooks, "remaining", books_remaining)
        monkeypatch.setattr(K.EvalScoreBooks, "results", books_results)


# ------------------------------------------------------------------------------------------------- test_policy on K20
@pytest.mark.parametrize("expanded", [False, True])
@pytest.mark.parametrize("deterministic", [True, False])
def test_mat_evaluation_is_one_k20_and_one_books_launch_per_step(deterministic, expanded, monkeypatch):
    import eval_restatement as R
    from ppo_and_friends_amd.testing import test_policy
    E, A, N, every = 9, 3, 20, 5
    ppo, pol = _mat_ppo(E=E, A=A, O=8 if expanded else 18, expanded=expanded)
    assert pol.inference_unsupported_reason() == "" and not np.array_equal(pol.agent_slot_order(), np.arange(A))
    rng = pol.actor.distribution.rng
    before = (rng.seed, rng.offset)
    eval_offset = pol.eval_rng().offset
    cnt = _Counters(pol, monkeypatch)
    try:
        info = test_policy(ppo, N, deterministic=deterministic, check_every=every, max_steps=4000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    agents = list(ppo.env.agent_ids)
    score, done = _trace_arrays(ppo.env, E, agents)
    steps = len(done)
    assert info == R.score_info(score, done, {a: "agent" for a in agents}, N)
    assert cnt.k20 == [1 if deterministic else 0] * steps                   # one K20 launch per env step
    assert not cnt.modules and not cnt.single                               # no module forward, no per-agent launch
    assert len(cnt.books) == steps
    assert cnt.reads == list(range(every, steps + 1, every))                # the only host reads
    assert (rng.seed, rng.offset) == before
    assert pol.eval_rng().offset - eval_offset == (0 if deterministic else steps * E * A)


def _training_state(ppo, pol):
    opt = pol.actor_critic_optim
    out = {"params": pol.policy_params, "optim.exp_avg": opt.exp_avg, "optim.exp_avg_sq": opt.exp_avg_sq,
           "optim.step": opt.step_count, "optim.lr": opt.lr}
    for key, vn in ppo.value_normalizers.items():
        out[f"vn.{key}"] = torch.stack([vn.running_stats.mean_t.double().reshape(-1)[0], vn.running_stats.var_t.double().reshape(-1)[0]])
    for w in ppo._filter_stack(ppo.env):
        for key in ("stats", "critic_stats", "state"):
            for i, t in enumerate(getattr(w, "_cfg", {}).get(key, ())):
                out[f"{type(w).__name__}.{key}.{i}"] = t
    rng = pol.actor.distribution.rng
    out["rng"] = torch.tensor([rng.seed % (1 << 62), rng.offset])
    out["training"] = torch.tensor([int(pol.actor_critic.training)])
    return {k: v.detach().clone().cpu() for k, v in out.items()}


def test_mat_evaluation_leaves_the_training_state_untouched(monkeypatch):
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Discrete
    from ppo_and_friends_amd.testing import test_policy
    E, A = 8, 3
    ppo, pol = _mat_ppo(E=E, A=A, ts=32, shuffled=False, normalize_obs=True, normalize_rewards=True, obs_clip=(-10.0, 10.0),
                        reward_clip=(-10.0, 10.0))
    ppo.learn(2 * 32)                                        # optimiser state and filter statistics that are not the initial ones
    assert pol.inference_unsupported_reason() == ""
    pol.train()
    before = _training_state(ppo, pol)
    assert int(before["optim.step"]) > 0 and before["optim.exp_avg"].abs().sum() > 0 and any(".stats." in k for k in before)
    ev = ppo.make_eval_env(lambda: _traced(SyntheticFixedLengthEnv)(10, 18, Discrete(5), 30, DEV, reward="uniform", seed=6,
                                                                    term_prob=0.1, num_agents=A))
    cnt = _Counters(pol, monkeypatch, guard_syncs=False)
    for deterministic in (False, True):
        info = test_policy(ppo, 30, deterministic=deterministic, env=ev, check_every=10, max_steps=4000)
        assert info["num_test_runs"] == 30 and info["total_time_steps"] >= 30
    after = _training_state(ppo, pol)
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert cnt.k20 and not cnt.modules and pol.eval_rng().offset > 0


# ------------------------------------------------------------------------------------------- where K20 does not apply
@pytest.mark.parametrize("case", ["torch_mode", "nine_actions"])
def test_uncovered_policies_decode_on_the_modules(case, monkeypatch):
    import eval_restatement as R
    from ppo_and_friends_amd.testing import test_policy
    E, N = 7, 15
    ppo, pol = _mat_ppo(E=E, mode="torch" if case == "torch_mode" else "auto", NA=9 if case == "nine_actions" else 5)
    why = pol.inference_unsupported_reason()
    assert why and (("torch" in why) if case == "torch_mode" else ("actions 9" in why))
    cnt = _Counters(pol, monkeypatch, guard_syncs=False)
    for deterministic in (True, False):
        _raw(ppo.env).trace = []
        info = test_policy(ppo, N, deterministic=deterministic, check_every=5, max_steps=4000)
        agents = list(ppo.env.agent_ids)
        score, done = _trace_arrays(ppo.env, E, agents)
        assert info == R.score_info(score, done, {a: "agent" for a in agents}, N)
    assert not cnt.k20 and cnt.modules and not cnt.single and cnt.books        # the books serve every multi-agent env


# ----------------------------------------------------------------------------- PPO.get_inference_actions, agent-major
@pytest.mark.parametrize("expanded", [False, True])
def test_agent_major_inference_is_the_regrouping_route(expanded):
    import mat_float64 as M
    E, A, NA = 2048, 3, 5
    O = 8 if expanded else 18
    ppo, pol = _mat_ppo(E=E, A=A, O=O, NA=NA, expanded=expanded)
    cO = O * A if expanded else O
    order_np = pol.agent_slot_order()
    assert pol.inference_unsupported_reason() == "" and not np.array_equal(order_np, np.arange(A))
    gen = torch.Generator(device=DEV).manual_seed(8)
    critic_obs = torch.randn(A * E, cO, device=DEV, generator=gen) * 2.0
    obs = critic_obs[:, :O].contiguous() if expanded else critic_obs
    got = ppo.get_inference_actions(obs, True, critic_obs=critic_obs if expanded else None).clone()
    assert got.shape == (A * E, 1) and got.dtype == torch.int64
    # the route this replaces: regroup by slot order, decode on the network modules, un-group
    order = torch.as_tensor(order_np, device=DEV)
    grouped = critic_obs.reshape(A, E, cO)[order].transpose(0, 1).contiguous()
    with torch.no_grad():
        enc, _ = pol.critic(grouped)
        a = pol._get_autoregressive_actions_without_exploration(enc)                     # [E, A, 1]
    want = a.transpose(0, 1)[torch.argsort(order)].reshape(A * E, 1)
    # decisions the float64 forward flags as near ties (and the later slots of their env) may differ, no others
    _, logits = M.float64_logits_decode(pol.actor_critic.state_dict(), cO, NA, A, grouped.cpu().numpy())
    keep = torch.from_numpy(M.compared_slots(logits)).to(DEV)                           # [E, A], slot order
    keep_major = keep.transpose(0, 1)[torch.argsort(order)].reshape(A * E, 1)
    differ = got != want
    print(f"\nexpanded={expanded}: {int(differ.sum())} of {A * E} decisions differ from the module route, "
          f"{int((~keep).sum())} flagged by the float64 forward")
    assert float((~keep).float().mean()) <= 0.005
    assert not (differ & keep_major).any()
    assert len(torch.unique(got)) > 1
    # grouped input through the policy's own method: the same decisions
    g2 = pol.get_inference_actions(grouped, True)
    assert torch.equal(g2.transpose(0, 1)[torch.argsort(order)].reshape(A * E, 1), got)


# ------------------------------------------------------------------------------------ MLP policies through the books
def test_three_agents_sharing_an_mlp_policy_through_the_books(monkeypatch):
    import torch.nn as nn
    import eval_restatement as R
    from initial_weights import float64_orthogonal_init
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Discrete
    from ppo_and_friends_amd.testing import test_policy
    E, N, O, A = 12, 40, 18, 3
    cls = _traced(SyntheticFixedLengthEnv)
    env_gen = lambda: cls(E, O, Discrete(5), 48, DEV, reward="uniform", seed=77, term_prob=0.06, num_agents=A, critic_view="policy")
    net = dict(hidden_size=128, hidden_depth=3, activation=nn.ReLU())
    with float64_orthogonal_init():
        ppo = PPO(env_gen, {"p": (None, _box(O), _box(O * A), Discrete(5), dict(actor_kw_args=dict(net), critic_kw_args=dict(net)))},
                  device=DEV, random_seed=3, envs_per_proc=E, ts_per_rollout=16, batch_size=64, save_state=False,
                  normalize_obs=False, normalize_rewards=False)
    cnt = _Counters(ppo.policies["p"], monkeypatch)
    try:
        info = test_policy(ppo, N, deterministic=True, check_every=10, max_steps=4000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    agents = list(ppo.env.agent_ids)
    score, done = _trace_arrays(ppo.env, E, agents)
    assert info == R.score_info(score, done, {a: "p" for a in agents}, N)
    assert len(cnt.books) == len(done) and not cnt.single
    assert info["p"]["avg_score"] == pytest.approx(sum(info[a]["avg_score"] for a in agents), rel=1e-12)


def test_two_policies_in_a_dict_env_through_the_books(monkeypatch):
    import eval_restatement as R
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    from ppo_and_friends_amd.testing import test_policy
    E, N = 10, 25
    specs = [("adversary_0", 8, Discrete(5)), ("agent_0", 10, Box(-1.0, 1.0, (2,), np.float32)),
             ("agent_1", 10, Box(-1.0, 1.0, (2,), np.float32))]
    cls = _traced(SyntheticMixedAgentsEnv)
    env_gen = lambda: cls(E, specs, 40, DEV, reward="uniform", seed=33, term_prob=0.07)
    settings = {"adversary": (None, _box(8), _box(8), Discrete(5), {}),
                "team": (None, _box(10), _box(10), Box(-1.0, 1.0, (2,), np.float32), {})}
    mapping = lambda a: "adversary" if a.startswith("adversary") else "team"
    ppo = PPO(env_gen, settings, policy_mapping_fn=mapping, device=DEV, random_seed=8, normalize_obs=False,
              normalize_rewards=False, envs_per_proc=E, ts_per_rollout=16, batch_size=32, save_state=False)
    cnt = _Counters(ppo.policies["team"], monkeypatch, guard_syncs=False)
    agents = [a for a, _, _ in specs]
    for deterministic in (True, False):
        _raw(ppo.env).trace = []
        cnt.books.clear()
        info = test_policy(ppo, N, deterministic=deterministic, check_every=7, max_steps=4000)
        score, done = _trace_arrays(ppo.env, E, agents)
        assert info == R.score_info(score, done, {a: mapping(a) for a in agents}, N)
        assert len(cnt.books) == len(done) and not cnt.single
        assert set(info) == {"num_test_runs", "total_time_steps", *agents, "adversary", "team"}
