"""
test_policy -- the reference's second verb (`ppoaf test`: testing.py:8-175) for batched device environments.

The reference plays `num_test_runs` episodes one after the other in one env.  Here the env holds E environments that
play in parallel, and taking "the first N episodes to finish" would take the SHORTEST ones -- a bias for every env
whose return grows with its length (CartPole).  So every env row owes a quota, N // E + (e < N % E) episodes, and the
score bookkeeping (ppoaf_eval_scores_step, csrc/policy_infer.hip) enforces it on the device: per step the package's own
share is the filter stack, one launch per policy for the actions -- K19 (ppoaf_policy_infer: actor forward -> env action)
for an MLP policy, K20 (ppoaf_mat_policy_infer: encoder + A decoder passes -> env actions, straight from and into the
env's agent-major tensors) for a multi-agent transformer -- and one bookkeeping launch: ppoaf_eval_scores_step with one
agent, ppoaf_eval_scores_step_books with several (every agent's book and every shared policy's book together).  The host
reads one int32 (`remaining`) every `check_every` steps and nothing else.  With E = 1 this is the reference's loop.
"""
import os

import numpy as np
import torch

from . import kernels as K
from .utils.mpi_utils import rank_print


def _yaml_scalar(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        if v != v:
            return ".nan"
        if v in (float("inf"), float("-inf")):
            return ".inf" if v > 0 else "-.inf"
        r = repr(v)
        if "e" in r and "." not in r:                     # YAML 1.1 floats need the dot: 1e-05 -> 1.0e-05
            m, e = r.split("e")
            r = f"{m}.0e{e}"
        return r
    s = str(v)
    return "'" + s.replace("'", "''") + "'"               # always quoted: an agent called "1" or "no" stays a string


def dump_score_info(score_info, path):
    """score_info -> `path` as YAML: through `yaml` when importable (what the reference does, testing.py:159-162), else
    a two-level block mapping written by hand that yaml.safe_load reads identically."""
    try:
        import yaml
    except ImportError:
        yaml = None
    with open(path, "w") as fh:
        if yaml is not None:
            yaml.dump(score_info, fh, default_flow_style=False)
            return
        for key in sorted(score_info, key=str):
            val = score_info[key]
            if isinstance(val, dict):
                fh.write(f"{_yaml_scalar(key)}:\n")
                for k in sorted(val, key=str):
                    fh.write(f"  {_yaml_scalar(k)}: {_yaml_scalar(val[k])}\n")
            else:
                fh.write(f"{_yaml_scalar(key)}: {_yaml_scalar(val)}\n")


def _reduce(rows, num_test_runs):
    """Per-row results (numpy, row order) -> (low, high, avg, steps) in float64; rows that owed nothing are skipped."""
    lo, hi, total, steps = np.inf, -np.inf, np.float64(0.0), 0
    for e in range(len(rows["count"])):
        if rows["count"][e] == 0:
            continue
        lo, hi = min(lo, float(rows["min"][e])), max(hi, float(rows["max"][e]))
        total = total + np.float64(rows["sum"][e])
        steps += int(rows["steps"][e])
    return float(lo), float(hi), float(total / num_test_runs) if num_test_runs else 0.0, steps


class _HostScores:
    """The bookkeeping of ppoaf_eval_scores_step for a policy that lives on the CPU (no kernel there): the same rule,
    written with torch ops."""

    def __init__(self, E, num_test_runs, device):
        q = torch.full((E,), num_test_runs // E, dtype=torch.int64)
        q[:num_test_runs % E] += 1
        self.quota = q.to(device)
        z = lambda dt: torch.zeros(E, dtype=dt, device=device)
        self.run_score, self.run_len, self.count, self.sum, self.steps = z(torch.float64), z(torch.int64), z(torch.int64), \
            z(torch.float64), z(torch.int64)
        self.min = torch.full((E,), float("inf"), dtype=torch.float64, device=device)
        self.max = torch.full((E,), float("-inf"), dtype=torch.float64, device=device)

    def step(self, score, done):
        live = self.count < self.quota
        self.run_score = torch.where(live, self.run_score + score.double(), self.run_score)
        self.run_len = torch.where(live, self.run_len + 1, self.run_len)
        fin = live & done.bool()
        self.count = self.count + fin
        self.sum = torch.where(fin, self.sum + self.run_score, self.sum)
        self.min = torch.where(fin, torch.minimum(self.min, self.run_score), self.min)
        self.max = torch.where(fin, torch.maximum(self.max, self.run_score), self.max)
        self.steps = torch.where(fin, self.steps + self.run_len, self.steps)
        self.run_score = torch.where(fin, torch.zeros_like(self.run_score), self.run_score)
        self.run_len = torch.where(fin, torch.zeros_like(self.run_len), self.run_len)

    def remaining(self):
        return int((self.quota - self.count).sum().item())

    def results(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("count", "sum", "min", "max", "steps")}


def _lstm_networks(ppo):
    return [net for pol in ppo.policies.values() if pol.using_lstm for net in (pol.actor, pol.critic)]


def test_policy(ppo, num_test_runs, deterministic=False, save_test_scores=False, verbose=False, env=None,
                check_every=None, max_steps=None, **kw_args):
    """
    testing.py:8-175.  -> score_info: `num_test_runs`, `total_time_steps`, per agent `low_score / high_score /
    avg_score / policy`, per policy `low_score / high_score / avg_score` (testing.py:114-157), printed as the
    reference prints it and written to `<state_path>/test-scores.yaml` when `save_test_scores`.

    env: the env to play in (default ppo.env); a caller that evaluates during training passes one from
    ppo.make_eval_env().  check_every: env steps between two host reads of `remaining` (default: the env's
    max_episode_steps if it has one, else 16); surplus steps change no result, the quotas are enforced on the device.
    max_steps: bound on the loop (RuntimeError beyond it).  The reference's render / GIF arguments are accepted through
    **kw_args and ignored (no renderer here).

    Filter statistics, value normalisers, parameters, optimiser state and the training random streams are left as they
    were; the filters' `update` switches, the policies' train / eval mode and the LSTM networks' hidden state are restored
    on the way out, also when the loop raises.
    """
    env = ppo.env if env is None else env
    N = int(num_test_runs)
    if N < 1:
        raise ValueError(f"num_test_runs={num_test_runs}: at least one test run")
    E = int(env.get_batch_size())
    agent_ids = list(getattr(env, "agent_ids", ["agent0"]))
    A = len(agent_ids)
    device = ppo.device
    if check_every is None:
        check_every = int(getattr(env, "max_episode_steps", 0) or 16)
    check_every = max(1, int(check_every))
    policy_of = {a: ppo.policy_mapping_fn(a) for a in agent_ids}
    policy_agents = {p: [a for a in agent_ids if policy_of[a] == p] for p in ppo.policies}
    # a policy with one agent scores what its agent scores; with several, its episode score is the float64 sum of
    # their scores added agent by agent within a step (testing.py:93-98): one bookkeeping call per agent, the episode
    # closing with the last one
    shared = [p for p, mine in policy_agents.items() if len(mine) > 1]
    books = None
    if device.type == "cuda" and A > 1:
        # every agent's book and every shared policy's book in ONE launch per env step
        masks = [1 << i for i in range(A)] + [sum(1 << agent_ids.index(a) for a in policy_agents[p]) for p in shared]
        books = K.EvalScoreBooks(E, N, device, A, masks)
    else:
        make = (lambda: K.EvalScores(E, N, device)) if device.type == "cuda" else (lambda: _HostScores(E, N, device))
        agent_scores = {a: make() for a in agent_ids}
        policy_scores = {p: make() for p in shared}
        never = torch.zeros(E, dtype=torch.bool, device=device)

    if verbose:
        for p, pol in ppo.policies.items():
            why = pol.inference_unsupported_reason() if policy_agents[p] and hasattr(pol, "inference_unsupported_reason") else ""
            if why:
                rank_print("Policy {}: the network modules decode its actions, not the one-launch step: {}".format(p, why))

    # ---- state to put back
    stack = list(ppo._filter_stack(env))
    switches = [(w, w._cfg["update"], w.update_stats) for w in stack if hasattr(w, "update_stats")]
    modes = {p: bool(getattr(pol, "actor_critic", pol.actor).training) for p, pol in ppo.policies.items()}
    hidden = [(net, net.hidden_state) for net in _lstm_networks(ppo)]
    steps = 0
    try:
        for w, _, _ in switches:                          # statistics frozen
            w._cfg["update"] = False
            w.update_stats = False
        for pol in ppo.policies.values():
            pol.eval()
        for pol in ppo.policies.values():
            if pol.using_lstm:
                # once, before the first step (what lstm.py:114 does when the batch size changes); then carried across
                # episode ends, as the reference's test_policy never resets it
                for net in (pol.actor, pol.critic):
                    net.reset_hidden_state(batch_size=E * len(pol.agent_ids), device=device)
        obs, critic_obs = ppo.apply_policy_reset_constraints(*env.reset())
        remaining = N
        while remaining > 0:
            if max_steps is not None and steps >= int(max_steps):
                raise RuntimeError(f"test_policy: {remaining} of {N} test runs still unfinished after {steps} env steps "
                                   f"(max_steps={max_steps})")
            actions = ppo.get_inference_actions(obs, deterministic, critic_obs=critic_obs, env=env)
            obs, critic_obs, reward, terminated, truncated, _ = ppo.apply_policy_step_constraints(*env.step(actions))
            score = ppo._natural_reward(env, reward)      # testing.py:88-91
            steps += 1
            if isinstance(score, dict):                   # the agents of an env end together
                done = (terminated[agent_ids[0]] | truncated[agent_ids[0]]).contiguous()
            else:
                done = (terminated | truncated).reshape(-1)[:E].contiguous()
                score = score.reshape(A, E)
            if books is not None:
                if isinstance(score, dict):
                    score = torch.stack([score[a].reshape(E) for a in agent_ids])
                books.step(score.to(torch.float32).contiguous(), done)
            else:
                for i, a in enumerate(agent_ids):
                    s = (score[a] if isinstance(score, dict) else score[i]).to(torch.float32).contiguous()
                    agent_scores[a].step(s, done)
                    mine = policy_agents[policy_of[a]]
                    if len(mine) > 1:
                        policy_scores[policy_of[a]].step(s, done if a == mine[-1] else never)
            if steps % check_every == 0:
                remaining = books.remaining() if books is not None else agent_scores[agent_ids[0]].remaining()
    finally:
        for w, upd, flag in switches:
            w._cfg["update"] = upd
            w.update_stats = flag
        for p, pol in ppo.policies.items():
            pol.train() if modes[p] else pol.eval()
        for net, state in hidden:
            net.hidden_state = state

    score_info = {"num_test_runs": N}
    if books is not None:
        per_book = books.results()
        rows = {a: per_book[i] for i, a in enumerate(agent_ids)}
        policy_rows = {p: per_book[A + j] for j, p in enumerate(shared)}
    else:
        rows = {a: agent_scores[a].results() for a in agent_ids}
        policy_rows = {p: policy_scores[p].results() for p in shared}
    score_info["total_time_steps"] = _reduce(rows[agent_ids[0]], N)[3]
    for a in agent_ids:
        lo, hi, avg, _ = _reduce(rows[a], N)
        score_info[a] = {"low_score": lo, "high_score": hi, "avg_score": avg, "policy": str(policy_of[a])}
    for p, mine in policy_agents.items():
        if not mine:
            continue
        lo, hi, avg, _ = _reduce(policy_rows[p] if len(mine) > 1 else rows[mine[0]], N)
        score_info[p] = {"low_score": lo, "high_score": hi, "avg_score": avg}

    num_steps = score_info["total_time_steps"]
    if verbose:                                           # testing.py:123-141
        for a in agent_ids:
            rank_print("\nAgent {}:".format(a))
            rank_print("    Policy: {}".format(policy_of[a]))
            rank_print("    Ran env {} times.".format(N))
            rank_print("    Ran {} total time steps.".format(num_steps))
            rank_print("    Ran {} time steps on average.".format(num_steps / N))
            rank_print("    Lowest score: {}".format(score_info[a]["low_score"]))
            rank_print("    Highest score: {}".format(score_info[a]["high_score"]))
            rank_print("    Average score: {}".format(score_info[a]["avg_score"]))
    else:
        for p in ppo.policies:
            if p not in score_info:
                continue
            rank_print("\nPolicy {}:".format(p))
            rank_print("    Ran env {} times.".format(N))
            rank_print("    Ran {} total time steps.".format(num_steps))
            rank_print("    Ran {} time steps on average.".format(num_steps / N))
            rank_print("    Lowest score: {}".format(score_info[p]["low_score"]))
            rank_print("    Highest score: {}".format(score_info[p]["high_score"]))
            rank_print("    Average score: {}".format(score_info[p]["avg_score"]))
    if save_test_scores:
        os.makedirs(ppo.state_path, exist_ok=True)
        dump_score_info(score_info, os.path.join(ppo.state_path, "test-scores.yaml"))
    return score_info


test_policy.__test__ = False          # (pytest: a library function, not a test)
