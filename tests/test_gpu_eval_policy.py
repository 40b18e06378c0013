"""
-m gpu: ppo_and_friends_amd.testing.test_policy end to end -- the harness's result against the numpy restatement
(tests/helpers/eval_restatement.py) fed with the (score, done) trace of the same run; the fused evaluation step (K19)
against the torch path PER STEP ON THE SAME OBSERVATIONS (one flipped near-tie action changes an env's whole remaining
trajectory, so final scores are not compared); agent-shared and two-policy envs, MAT, LSTM, MultiDiscrete / MultiBinary;
no side effects on a training run; host reads; and the learning check the reference ships (CartPole reaches 200).

Near-tie rule as in tests/test_gpu_eval_kernels.py: a row may differ from the float64 forward's greedy action only when
its top two float64 logits are closer than the sum of their bounds 1e-5 |z| + 1e-5 max|z|; the share of such rows is
asserted to stay <= 0.5 % over all rows of all steps.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _box(n):
    from ppo_and_friends_amd.spaces import Box
    return Box(-np.inf, np.inf, (n,), np.float32)


def _logits64(pol, obs):
    """The actor's outputs in float64 numpy from its Linear layers (plain FeedForwardNetwork actors)."""
    lin = [m for m in pol.actor.sequential_net.modules() if isinstance(m, nn.Linear)]
    act = pol.actor.activation
    h = obs.detach().cpu().numpy().astype(np.float64)
    for l, m in enumerate(lin):
        h = h @ m.weight.detach().cpu().numpy().astype(np.float64).T + m.bias.detach().cpu().numpy().astype(np.float64)
        if l + 1 < len(lin):
            if isinstance(act, nn.Tanh):
                h = np.tanh(h)
            else:
                h = np.where(h > 0, h, (0.01 if isinstance(act, nn.LeakyReLU) else 0.0) * h)
    return h


def _greedy_and_near(z, kind, nvec=()):
    tol = 1e-5 * np.abs(z) + 1e-5 * np.abs(z).max()
    if kind == "bernoulli":
        return (z >= 0).astype(np.float32), (np.abs(z) < tol).any(1)
    acts, near, o = [], np.zeros(len(z), bool), 0
    for n in (nvec or (z.shape[1],)):
        s, t = z[:, o:o + n], tol[:, o:o + n]
        acts.append(np.argmax(s, 1))
        if n > 1:
            order = np.argsort(-s, axis=1, kind="stable")
            r = np.arange(len(s))
            near |= (s[r, order[:, 0]] - s[r, order[:, 1]]) < (t[r, order[:, 0]] + t[r, order[:, 1]])
        o += n
    a = np.stack(acts, 1)
    return (a if nvec else a[:, 0]), near


class _Log:
    """Records what goes through a policy's get_inference_actions."""

    def __init__(self, pol, monkeypatch):
        self.obs, self.actions = [], []
        inner = pol.get_inference_actions

        def logged(obs, deterministic):
            a = inner(obs, deterministic)
            self.obs.append(obs.clone()); self.actions.append(a.clone())
            return a
        monkeypatch.setattr(pol, "get_inference_actions", logged)


def _traced(env_cls):
    """env class -> the same env recording (score, done) of every step: what the harness is fed."""
    class Traced(env_cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            if torch.is_tensor(getattr(self, "term_table", None)):
                self.term_table[-1] = True                   # table-driven envs: every row finishes once per horizon

        def step(self, action):
            out = super().step(action)
            self.trace.append((out[2], out[3], out[4]))
            return out

        def reset(self):
            if not hasattr(self, "trace"):
                self.trace = []
            return super().reset()
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


def _cartpole_ppo(E=50, mode="auto", seed=4, max_steps=200, **kw):
    from initial_weights import float64_orthogonal_init
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv
    from ppo_and_friends_amd.spaces import Discrete
    cls = _traced(BatchedCartPoleEnv)
    env_gen = lambda: cls(E, DEV, seed=11, max_episode_steps=max_steps)
    probe = BatchedCartPoleEnv(1, DEV)
    net = dict(hidden_size=128, hidden_depth=3, activation=nn.ReLU())
    with float64_orthogonal_init():
        return PPO(env_gen, {"p": (None, probe.observation_space, probe.observation_space, Discrete(2),
                                   dict(actor_kw_args=dict(net), critic_kw_args=dict(net)))},
                   device=DEV, random_seed=seed, envs_per_proc=E, ts_per_rollout=32, batch_size=64, update_mode=mode,
                   save_state=False, **kw)


# --------------------------------------------------------------------------------------------------------------- 9 (a)
@pytest.mark.parametrize("deterministic", [True, False])
def test_cartpole_result_is_the_restatement_of_its_own_trace(deterministic, monkeypatch):
    import eval_restatement as R
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.testing import test_policy
    E, N = 50, 130
    ppo = _cartpole_ppo(E)
    pol = ppo.policies["p"]
    assert pol.inference_unsupported_reason() == ""
    log = _Log(pol, monkeypatch)
    launches = []
    inner = K.policy_infer
    monkeypatch.setattr(K, "policy_infer", lambda a: (launches.append(a.mode), inner(a))[1])
    rng = pol.actor.distribution.rng
    before = (rng.seed, rng.offset)
    info = test_policy(ppo, N, deterministic=deterministic, check_every=25, max_steps=4000)
    score, done = _trace_arrays(ppo.env, E, ["agent0"])
    assert info == R.score_info(score, done, {"agent0": "p"}, N)
    assert info["num_test_runs"] == N and 8.0 <= info["p"]["low_score"] <= info["p"]["avg_score"] <= info["p"]["high_score"] <= 200.0
    assert len(launches) == len(done) and set(launches) == {1 if deterministic else 0}      # K19 drove every step
    assert (rng.seed, rng.offset) == before                                                   # the rollout's stream did not move
    assert pol.eval_rng().offset == (0 if deterministic else E * len(done))
    if not deterministic:
        assert len({tuple(a.cpu().numpy().tolist()) for a in log.actions[:8]}) > 1
        return
    # the torch path's greedy action beside the fused one, on the same observations
    obs, act = torch.cat(log.obs), torch.cat([a.reshape(-1) for a in log.actions]).cpu().numpy()
    with torch.no_grad():
        torch_act = pol.actor.distribution.refine_prediction(pol.actor.forward_logits(obs)).cpu().numpy()
    want, near = _greedy_and_near(_logits64(pol, obs), "categorical")
    print(f"\n{near.sum()} of {len(near)} rows near a tie; fused != torch on {(act != torch_act).sum()} rows")
    assert near.mean() <= 0.005
    assert not ((act != torch_act) & ~near).any() and not ((act != want) & ~near).any()


# --------------------------------------------------------------------------------------------------------------- 9 (b)
def _synthetic_ppo(space, O=18, agents=1, E=12, horizon=48, hidden=128, critic_hidden=None, depth=3, mode="auto", term=0.06,
                   filters=False, seed=3, act=nn.ReLU, T=16, B=64):
    from initial_weights import float64_orthogonal_init
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    cls = _traced(SyntheticFixedLengthEnv)
    view = "policy" if agents > 1 else "local"
    env_gen = lambda: cls(E, O, space, horizon, DEV, reward="uniform", seed=77, term_prob=term, num_agents=agents, critic_view=view)
    net = dict(hidden_size=hidden, hidden_depth=depth, activation=act())
    pargs = dict(actor_kw_args=dict(net), critic_kw_args=dict(net, hidden_size=critic_hidden or hidden))
    fk = dict(normalize_obs=True, normalize_rewards=True, obs_clip=(-10.0, 10.0), reward_clip=(-10.0, 10.0)) if filters else \
        dict(normalize_obs=False, normalize_rewards=False)
    with float64_orthogonal_init():
        return PPO(env_gen, {"p": (None, _box(O), _box(O * agents), space, pargs)}, device=DEV, random_seed=seed, envs_per_proc=E,
                   ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode=mode, save_state=False, **fk)


def test_three_agents_sharing_a_policy_c4_shape():
    import eval_restatement as R
    from ppo_and_friends_amd.spaces import Discrete
    from ppo_and_friends_amd.testing import test_policy
    E, N = 12, 40
    ppo = _synthetic_ppo(Discrete(5), O=18, agents=3, E=E, hidden=128, critic_hidden=256)
    assert ppo.policies["p"].inference_unsupported_reason() == ""
    info = test_policy(ppo, N, deterministic=True, check_every=10, verbose=True, max_steps=4000)
    agents = list(ppo.env.agent_ids)
    score, done = _trace_arrays(ppo.env, E, agents)
    assert info == R.score_info(score, done, {a: "p" for a in agents}, N)
    # the policy's episode score is the sum of its three agents': not an agent's own low / high
    assert info["p"]["avg_score"] == pytest.approx(sum(info[a]["avg_score"] for a in agents), rel=1e-12)


def test_two_policies_in_a_dict_env():
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
    assert all(p.inference_unsupported_reason() == "" for p in ppo.policies.values())
    for deterministic in (True, False):
        ppo.env.trace = []
        info = test_policy(ppo, N, deterministic=deterministic, check_every=7, max_steps=4000)
        agents = [a for a, _, _ in specs]
        score, done = _trace_arrays(ppo.env, E, agents)
        assert info == R.score_info(score, done, {a: mapping(a) for a in agents}, N)
        assert info["agent_1"]["policy"] == "team" and set(info) == {"num_test_runs", "total_time_steps", *agents, "adversary", "team"}


# --------------------------------------------------------------------------------------------------------------- 9 (c)
def test_mat_deterministic_decode_is_the_per_agent_loop(golden):
    import torch.nn.functional as F
    import eval_restatement as R
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.spaces import Discrete
    from ppo_and_friends_amd.testing import test_policy
    g = golden("g12_c5_mat")
    E, A, O, NA = 9, 3, 18, 5
    cls = _traced(SyntheticFixedLengthEnv)
    env_gen = lambda: cls(E, O, Discrete(NA), 40, DEV, reward="uniform", seed=5, term_prob=0.08, num_agents=A)
    ppo = PPO(env_gen, {"agent": (MATPolicy, _box(O), _box(O), Discrete(NA), {})}, device=DEV, random_seed=1,
              normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=16, batch_size=16, save_state=False)
    pol = ppo.policies["agent"]
    sd0 = {"actor." + k[len("init_actor."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init_actor.")}
    sd0.update({"critic." + k[len("init_critic."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init_critic.")})
    missing, unexpected = pol.actor_critic.load_state_dict(sd0, strict=False)
    assert not [m for m in missing if "mask" not in m] and not [u for u in unexpected if "mask" not in u]
    obs = torch.randn(E, A, O, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * 2.0
    got = pol.get_inference_actions(obs, True)
    with torch.no_grad():                                   # mat_policy.py:521-585 with the network modules
        enc, _ = pol.critic(obs)
        block = torch.zeros(E, A, NA + 1, device=DEV)
        block[:, 0, 0] = 1
        want = torch.zeros(E, A, 1, dtype=torch.int64, device=DEV)
        for i in range(A):
            a = pol.actor(block, enc)[:, i, :].argmax(-1)
            want[:, i, 0] = a
            if i + 1 < A:
                block[:, i + 1, 1:] = F.one_hot(a, NA).float()
    assert got.shape == (E, A, 1) and torch.equal(got, want) and len(torch.unique(got)) > 1
    with pytest.raises(ValueError, match="grouped"):
        pol.get_inference_actions(obs[0], True)
    # numpy in the reference's [A, E, O] -> numpy [A, E, .]
    np.testing.assert_array_equal(pol.get_inference_actions(obs.transpose(0, 1).cpu().numpy(), True), want.transpose(0, 1).cpu().numpy())
    rng = pol.actor.distribution.rng
    before = (rng.seed, rng.offset)
    for deterministic in (True, False):
        ppo.env.trace = []
        info = test_policy(ppo, 20, deterministic=deterministic, check_every=5, max_steps=4000)
        agents = list(ppo.env.agent_ids)
        score, done = _trace_arrays(ppo.env, E, agents)
        assert info == R.score_info(score, done, {a: "agent" for a in agents}, 20)
    assert (rng.seed, rng.offset) == before and pol.eval_rng().offset > 0


# --------------------------------------------------------------------------------------------------------------- 9 (d)
@pytest.mark.parametrize("mode", ["fused", "auto"])
def test_lstm_state_is_reset_once_carried_and_put_back(mode, monkeypatch):
    import eval_restatement as R
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Discrete
    from ppo_and_friends_amd.testing import test_policy
    E, O = 8, 5
    cls = _traced(SyntheticFixedLengthEnv)
    env_gen = lambda: cls(E, O, Discrete(3), 24, DEV, reward="uniform", seed=13, term_prob=0.1)
    kw = dict(sequence_length=4, lstm_hidden_size=32, ff_hidden_size=32)
    ppo = PPO(env_gen, {"p": (None, _box(O), _box(O), Discrete(3), dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
              device=DEV, random_seed=1, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=24,
              batch_size=16, max_ts_per_ep=7, save_state=False, update_mode=mode)
    pol = ppo.policies["p"]
    assert pol.actor.use_hip == (mode == "fused") and "LSTM" in pol.inference_unsupported_reason()
    ppo.rollout()                                            # leaves a training-time hidden state behind
    kept = {n: net.hidden_state for n, net in (("actor", pol.actor), ("critic", pol.critic))}
    kept_values = {n: tuple(t.clone() for t in s) for n, s in kept.items()}
    log = _Log(pol, monkeypatch)
    ppo.env.trace = []
    info = test_policy(ppo, 30, deterministic=True, check_every=4, max_steps=4000)
    score, done = _trace_arrays(ppo.env, E, ["agent0"])
    assert info == R.score_info(score, done, {"agent0": "p"}, 30)
    assert done[:len(log.obs) - 1].any()                     # episodes ended inside the run
    for n, net in (("actor", pol.actor), ("critic", pol.critic)):
        assert net.hidden_state is kept[n] and all(torch.equal(a, b) for a, b in zip(net.hidden_state, kept_values[n]))
    # the loop over forward_logits: zero state once, then carried over every step, episode ends included
    pol.actor.reset_hidden_state(batch_size=E, device=DEV)
    with torch.no_grad():
        for t, (o, a) in enumerate(zip(log.obs, log.actions)):
            assert torch.equal(pol.actor.forward_logits(o).argmax(-1).reshape(-1), a.reshape(-1)), t
    pol.actor.hidden_state = kept["actor"]


# --------------------------------------------------------------------------------------------------------------- 9 (e)
@pytest.mark.parametrize("head", [("md", (3, 2, 3)), ("mb", 6)])
def test_multidiscrete_and_multibinary_under_fused(head, monkeypatch):
    import eval_restatement as R
    from ppo_and_friends_amd.spaces import MultiBinary, MultiDiscrete
    from ppo_and_friends_amd.testing import test_policy
    space = MultiDiscrete(list(head[1])) if head[0] == "md" else MultiBinary(head[1])
    E = 20
    assert _synthetic_ppo(space, O=9, E=E, hidden=64, depth=2).policies["p"].inference_unsupported_reason() != ""    # "auto": torch
    ppo = _synthetic_ppo(space, O=9, E=E, hidden=64, depth=2, mode="fused")
    pol = ppo.policies["p"]
    assert pol.inference_unsupported_reason() == ""
    log = _Log(pol, monkeypatch)
    info = test_policy(ppo, 33, deterministic=True, check_every=6, max_steps=4000)
    score, done = _trace_arrays(ppo.env, E, ["agent0"])
    assert info == R.score_info(score, done, {"agent0": "p"}, 33)
    obs, act = torch.cat(log.obs), torch.cat(log.actions).cpu().numpy()
    want, near = _greedy_and_near(_logits64(pol, obs), "bernoulli" if head[0] == "mb" else "multi", head[1] if head[0] == "md" else ())
    assert act.shape == want.shape and near.mean() <= 0.005
    np.testing.assert_array_equal(act[~near], want[~near])
    with torch.no_grad():
        torch_act = pol.actor.distribution.refine_prediction(pol.actor.forward_logits(obs)).cpu().numpy()
    np.testing.assert_array_equal(act[~near], torch_act[~near])
    ppo.env.trace = []
    info = test_policy(ppo, 12, deterministic=False, check_every=6, max_steps=4000)
    score, done = _trace_arrays(ppo.env, E, ["agent0"])
    assert info == R.score_info(score, done, {"agent0": "p"}, 12)


# ------------------------------------------------------------------------------------------------------------------ 10
def _training_state(ppo):
    pol = ppo.policies["p"]
    out = {"params": pol.policy_params, "m": pol.policy_exp_avg, "v": pol.policy_exp_avg_sq, "steps": pol.policy_step_counts,
           "lr": pol.policy_lr}
    vs = ppo.value_normalizers["p"].running_stats
    out["vn"] = torch.stack([vs.mean_t.double().reshape(-1)[0], vs.var_t.double().reshape(-1)[0]])
    for w in ppo._filter_stack(ppo.env):
        for key in ("stats", "critic_stats", "state"):
            for i, t in enumerate(getattr(w, "_cfg", {}).get(key, ())):
                out[f"{type(w).__name__}.{key}.{i}"] = t
    rng = pol.actor.distribution.rng
    out["rng"] = torch.tensor([rng.seed % (1 << 62), rng.offset])
    return {k: v.detach().clone().cpu() for k, v in out.items()}


@pytest.mark.parametrize("config", ["c2", "c3_filters"])
def test_evaluation_leaves_the_training_run_untouched(config):
    """rollout -> test_policy(env = an evaluation env of its own, sampled) -> train_on_rollout -> rollout, against the
    same sequence without the evaluation: bitwise the same parameters, optimiser state, normaliser statistics and
    second-rollout actions."""
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    from ppo_and_friends_amd.testing import test_policy
    runs = {}
    for evaluate in (False, True):
        if config == "c2":
            ppo = _cartpole_ppo(E=64, seed=6)
            eval_gen = lambda: BatchedCartPoleEnv(24, DEV, seed=99, max_episode_steps=60)
        else:
            space = Box(-1.0, 1.0, (6,), np.float32)
            ppo = _synthetic_ppo(space, O=17, E=16, hidden=256, depth=3, filters=True, act=nn.Tanh, T=32, B=128)
            eval_gen = lambda: SyntheticFixedLengthEnv(10, 17, space, 30, DEV, reward="uniform", seed=5, term_prob=0.1)
        assert ppo.policies["p"].inference_unsupported_reason() == ""
        ppo.rollout()
        if evaluate:
            before = _training_state(ppo)
            ev = ppo.make_eval_env(eval_gen)
            info = test_policy(ppo, 30, deterministic=False, env=ev, check_every=10, max_steps=4000)
            assert info["num_test_runs"] == 30 and info["total_time_steps"] >= 30
            after = _training_state(ppo)
            assert sorted(before) == sorted(after) and all(torch.equal(before[k], after[k]) for k in before)
            assert ppo.policies["p"].eval_rng().offset > 0
        ppo.train_on_rollout()
        ppo.rollout()
        st = _training_state(ppo)
        st["actions2"] = ppo.policies["p"].buffer.actions.detach().clone().cpu()
        st["obs2"] = ppo.policies["p"].buffer.observations.detach().clone().cpu()
        runs[evaluate] = st
    assert len(runs[True]) > (12 if config == "c3_filters" else 8)
    for k in runs[False]:
        assert torch.equal(runs[False][k], runs[True][k]), k


# ------------------------------------------------------------------------------------------------------------------ 12
def test_the_loop_reads_the_host_only_for_remaining(monkeypatch):
    """Every env step of the loop is enqueued without a host synchronisation (torch's sync debug mode raises on one);
    the only reads are `remaining`, every check_every steps, through the one method that does them."""
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.testing import test_policy
    ppo = _cartpole_ppo(E=32, max_steps=40)
    reads, steps = [], []
    remaining, step, results = K.EvalScores.remaining, K.EvalScores.step, K.EvalScores.results

    def counted_remaining(self):
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(len(steps))
            return remaining(self)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    def counted_step(self, score, done):
        torch.cuda.set_sync_debug_mode("error")            # from the first step on
        steps.append(1)
        return step(self, score, done)

    def final_results(self):
        torch.cuda.set_sync_debug_mode("default")
        return results(self)

    monkeypatch.setattr(K.EvalScores, "remaining", counted_remaining)
    monkeypatch.setattr(K.EvalScores, "step", counted_step)
    monkeypatch.setattr(K.EvalScores, "results", final_results)
    try:
        info = test_policy(ppo, 64, deterministic=True, check_every=40, max_steps=4000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # every row owes two episodes of at most 40 steps: done within 80 steps, i.e. at most two reads, at steps 40 and 80
    assert reads == list(range(40, len(steps) + 1, 40)) and len(steps) in (40, 80)
    assert info["total_time_steps"] <= 80 * 32 and info["num_test_runs"] == 64
    with pytest.raises(RuntimeError):                       # the guard itself works: a read inside the loop raises
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(3, device=DEV).sum().item()
        finally:
            torch.cuda.set_sync_debug_mode("default")


# ------------------------------------------------------------------------------------------------------------------ 11
def test_cartpole_reaches_200_under_fused(tmp_path):
    """
    The reference's learning check (test/tests/train/test_gymnasium.py:3-49): train CartPole for 70 000 timesteps, then
    test the best policy for 10 runs, deterministically; the high score must reach 200 with max_episode_steps = 200.
    Runner settings as baselines/gymnasium/cart_pole.py (LeakyReLU, lr 2e-3, batch 256, max_ts_per_ep 32, observation /
    reward normalisers, +-10 clips), update_mode="fused", seed fixed.
    """
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv
    from ppo_and_friends_amd.spaces import Discrete
    from ppo_and_friends_amd.testing import test_policy
    E = 16
    env_gen = lambda: BatchedCartPoleEnv(E, DEV, seed=0, max_episode_steps=200)
    probe = env_gen()
    act = dict(activation=nn.LeakyReLU())
    ppo = PPO(env_gen, {"p": (None, probe.observation_space, probe.observation_space, Discrete(2),
                              dict(lr=2e-3, actor_kw_args=act, critic_kw_args=dict(act)))},
              device=DEV, random_seed=2, envs_per_proc=E, ts_per_rollout=256, max_ts_per_ep=32, batch_size=256,
              obs_clip=(-10.0, 10.0), reward_clip=(-10.0, 10.0), normalize_obs=True, normalize_rewards=True,
              update_mode="fused", state_path=str(tmp_path), save_state=True, checkpoint_every=10 ** 9)
    assert ppo.policies["p"].inference_unsupported_reason() == ""
    while ppo.status_dict["global status"]["timesteps"] < 70000:
        ppo.learn(E * 256)
    ppo.load(str(tmp_path), "p_best")                        # --policy_tag single_agent_best
    info = test_policy(ppo, 10, deterministic=True, save_test_scores=True, max_steps=4000)
    print(f"\nCartPole after 70 000 timesteps under 'fused': {info['p']}")
    assert os.path.exists(os.path.join(str(tmp_path), "test-scores.yaml"))
    assert info["p"]["high_score"] >= 200.0
