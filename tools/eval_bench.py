"""
Evaluation env-steps/s of `ppo_and_friends_amd.testing.test_policy` at three shapes, two legs in one process, alternated:

  shapes  c2  BatchedCartPoleEnv, E = 4096, actor 4 -> 128^3 -> 2 (Discrete(2)), observation / reward normalisers
          c3  SyntheticFixedLengthEnv, E = 4096, actor 17 -> 256^3 -> 6 (Box(6), C3's actor shape), no filters
          c5  SyntheticFixedLengthEnv, E = 4096, O = 18, Discrete(5), 3 agents, MATPolicy defaults (C5's shape), no
              filters; only with --shape c5 ("both" stays c2 + c3)
          lstm  BatchedCartPoleEnv, E = 4096, LSTM actor / critic of the reference's cart_pole_lstm baseline (4
              observations, Discrete(2), LSTM 32, feed-forward 16, LeakyReLU), update_mode="fused"; only with --shape
              lstm.  Also times PPO.rollout (T = --rollout-steps per env) with the K21 step on and off.
  legs    a   this package: test_policy (K19 `ppoaf_policy_infer` + `ppoaf_eval_scores_step` per step, one host read
              of `remaining` every check_every steps)
          b   the baseline: the same loop written only with what the package had before K19 -- the torch forward of
              PPOPolicy.get_inference_actions (actor.forward_logits + refine_prediction) and torch ops for the
              scores, same quotas, same host read
              c5: the path evaluation took before K20 on the same object -- `inference_unsupported_reason` forced
              non-empty, so PPO.get_inference_actions regroups and the network modules decode, and one
              `ppoaf_eval_scores_step` launch per agent and one more per agent for the policy's book
              lstm: leg a is K21 (`ppoaf_lstm_policy_step`, INFER), leg b the same test_policy with
              `pol.fused_lstm_step = False`: forward_logits on K18 + torch ops, the route before K21

Both legs play the same number of test runs from the same env seed; env-steps/s = E x loop steps / wall time, printed as
median and spread (min .. max) over `--repeats`, then one JSON line.  `--leg a|b --shape c2|c3 --repeats 1` under
`rocprofv3 --kernel-trace --stats` gives the launches per evaluation step of one leg (the loop steps are printed).

    python tools/eval_bench.py [--shape both|c2|c3|c5|lstm] [--leg both|a|b] [--envs 4096] [--runs-per-env 2] [--repeats 5]
                               [--rollout-steps 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)


def count_steps(ppo):
    """Counts the raw env's steps (the loop steps of either leg) in ppo.loop_steps[0]."""
    raw = ppo.env
    while hasattr(raw, "env"):
        raw = raw.env
    ppo.loop_steps = [0]
    inner = raw.step

    def step(action):
        ppo.loop_steps[0] += 1
        return inner(action)
    raw.step = step


def make(shape, E, T=32):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    if shape == "c2":
        env_gen = lambda: BatchedCartPoleEnv(E, DEV, seed=0, max_episode_steps=200)
        probe = BatchedCartPoleEnv(1, DEV)
        net = dict(hidden_size=128, hidden_depth=3, activation=nn.ReLU())
        settings = {"p": (None, probe.observation_space, probe.observation_space, Discrete(2),
                          dict(actor_kw_args=dict(net), critic_kw_args=dict(net)))}
        ppo = PPO(env_gen, settings, device=DEV, random_seed=1, envs_per_proc=E, ts_per_rollout=32, save_state=False)
    elif shape == "lstm":
        from ppo_and_friends_amd.networks.lstm import LSTMNetwork
        env_gen = lambda: BatchedCartPoleEnv(E, DEV, seed=0, max_episode_steps=200)
        probe = BatchedCartPoleEnv(1, DEV)
        net = dict(lstm_hidden_size=32, ff_hidden_size=16, activation=nn.LeakyReLU())
        settings = {"p": (None, probe.observation_space, probe.observation_space, Discrete(2),
                          dict(ac_network=LSTMNetwork, actor_kw_args=dict(net), critic_kw_args=dict(net)))}
        ppo = PPO(env_gen, settings, device=DEV, random_seed=1, envs_per_proc=E, ts_per_rollout=T, max_ts_per_ep=200,
                  save_state=False, update_mode="fused")
    elif shape == "c5":
        from ppo_and_friends_amd.policies.mat_policy import MATPolicy

        def env_gen():
            env = SyntheticFixedLengthEnv(E, 18, Discrete(5), 64, DEV, reward="uniform", seed=1234, term_prob=0.02, num_agents=3)
            env.term_table[-1] = True                 # every row finishes at least once per 64 steps
            return env
        sp = Box(-np.inf, np.inf, (18,), np.float32)
        ppo = PPO(env_gen, {"p": (MATPolicy, sp, sp, Discrete(5), {})}, device=DEV, random_seed=1, envs_per_proc=E,
                  ts_per_rollout=32, normalize_obs=False, normalize_rewards=False, save_state=False)
    else:
        space = Box(-1.0, 1.0, (6,), np.float32)

        def env_gen():
            env = SyntheticFixedLengthEnv(E, 17, space, 64, DEV, reward="uniform", seed=1234, term_prob=0.02)
            env.term_table[-1] = True                 # every row finishes at least once per 64 steps
            return env
        sp = Box(-np.inf, np.inf, (17,), np.float32)
        net = dict(hidden_size=256, hidden_depth=3, activation=nn.Tanh())
        settings = {"p": (None, sp, sp, space, dict(actor_kw_args=dict(net), critic_kw_args=dict(net)))}
        ppo = PPO(env_gen, settings, device=DEV, random_seed=1, envs_per_proc=E, ts_per_rollout=32, normalize_obs=False,
                  normalize_rewards=False, save_state=False)
    ppo.rollout()                                     # filter statistics that are not the identity
    count_steps(ppo)
    return ppo


def leg_a(ppo, N, check_every):
    from ppo_and_friends_amd.testing import test_policy
    return test_policy(ppo, N, deterministic=True, check_every=check_every)


def leg_b(ppo, N, check_every):
    """The evaluation loop with the torch forward and torch bookkeeping (no K19, no scores kernel)."""
    env, pol = ppo.env, ppo.policies["p"]
    E = env.get_batch_size()
    quota = torch.full((E,), N // E, dtype=torch.int64, device=DEV)
    quota[:N % E] += 1
    z = lambda dt: torch.zeros(E, dtype=dt, device=DEV)
    run_score, run_len, count, total, steps = z(torch.float64), z(torch.int64), z(torch.int64), z(torch.float64), z(torch.int64)
    lo = torch.full((E,), float("inf"), dtype=torch.float64, device=DEV)
    hi = torch.full((E,), float("-inf"), dtype=torch.float64, device=DEV)
    stack = [w for w in ppo._filter_stack(env) if hasattr(w, "update_stats")]
    saved = [w._cfg["update"] for w in stack]
    for w in stack:
        w._cfg["update"] = False
    pol.eval()
    try:
        obs, _ = env.reset()
        t, remaining = 0, N
        while remaining > 0:
            with torch.no_grad():                     # PPOPolicy.get_inference_actions as it was: torch forward + refine
                action = pol.actor.distribution.refine_prediction(pol.actor.forward_logits(obs))
            obs, _, reward, terminated, truncated, _ = env.step(action)
            score = ppo._natural_reward(env, reward)
            done = terminated | truncated
            live = count < quota
            run_score = torch.where(live, run_score + score.double(), run_score)
            run_len = torch.where(live, run_len + 1, run_len)
            fin = live & done
            count = count + fin
            total = torch.where(fin, total + run_score, total)
            lo = torch.where(fin, torch.minimum(lo, run_score), lo)
            hi = torch.where(fin, torch.maximum(hi, run_score), hi)
            steps = torch.where(fin, steps + run_len, steps)
            run_score = torch.where(fin, torch.zeros_like(run_score), run_score)
            run_len = torch.where(fin, torch.zeros_like(run_len), run_len)
            t += 1
            if t % check_every == 0:
                remaining = int((quota - count).sum().item())
    finally:
        for w, u in zip(stack, saved):
            w._cfg["update"] = u
    return {"num_test_runs": N, "total_time_steps": int(steps.sum().item()),
            "p": {"low_score": float(lo.min().item()), "high_score": float(hi.max().item()),
                  "avg_score": float(total.sum().item() / N)}}


def leg_b_mat(ppo, N, check_every):
    """test_policy as it ran before K20 and the books: module decode behind PPO.get_inference_actions' regrouping, and the
    per-agent chain of ppoaf_eval_scores_step launches (agent books + the shared policy's book)."""
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.testing import _reduce
    env, pol = ppo.env, ppo.policies["p"]
    E, agent_ids = env.get_batch_size(), list(env.agent_ids)
    A = len(agent_ids)
    agent_scores = [K.EvalScores(E, N, DEV) for _ in agent_ids]
    policy_scores = K.EvalScores(E, N, DEV)
    never = torch.zeros(E, dtype=torch.bool, device=DEV)
    training = pol.actor_critic.training
    pol.inference_unsupported_reason = lambda: "eval_bench leg b: the module decode"
    pol.eval()
    try:
        obs, critic_obs = ppo.apply_policy_reset_constraints(*env.reset())
        t, remaining = 0, N
        while remaining > 0:
            actions = ppo.get_inference_actions(obs, True, critic_obs=critic_obs, env=env)
            obs, critic_obs, reward, terminated, truncated, _ = ppo.apply_policy_step_constraints(*env.step(actions))
            score = ppo._natural_reward(env, reward).reshape(A, E)
            done = (terminated | truncated).reshape(-1)[:E].contiguous()
            for i in range(A):
                s = score[i].to(torch.float32).contiguous()
                agent_scores[i].step(s, done)
                policy_scores.step(s, done if i == A - 1 else never)
            t += 1
            if t % check_every == 0:
                remaining = agent_scores[0].remaining()
    finally:
        del pol.inference_unsupported_reason
        pol.train() if training else pol.eval()
    lo, hi, avg, steps = _reduce(policy_scores.results(), N)
    return {"num_test_runs": N, "total_time_steps": _reduce(agent_scores[0].results(), N)[3],
            "p": {"low_score": lo, "high_score": hi, "avg_score": avg}}


def leg_b_lstm(ppo, N, check_every):
    """test_policy with the K21 step switched off: the route an LSTM policy's evaluation took before K21."""
    pol = ppo.policies["p"]
    pol.fused_lstm_step = False
    try:
        return leg_a(ppo, N, check_every)
    finally:
        pol.fused_lstm_step = True


def rollout_seconds(ppo, fused):
    """Wall time of one PPO.rollout with the K21 step on or off (synchronised before and after)."""
    pol = ppo.policies["p"]
    pol.fused_lstm_step = fused
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ppo.rollout()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    finally:
        pol.fused_lstm_step = True
        pol.clear_dataset()


def time_rollouts(ppo, result, legs, repeats, warmup):
    """Rollout seconds per leg (a: K21, b: the attribute off), alternated; median and min .. max."""
    for name in legs:
        for _ in range(warmup):
            rollout_seconds(ppo, name == "a")
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for name in legs:
            times[name].append(rollout_seconds(ppo, name == "a"))
    T = ppo.ts_per_rollout // ppo.envs_per_proc
    for name in legs:
        t = np.array(times[name])
        result[f"lstm_rollout_{name}_seconds"] = float(np.median(t))
        result[f"lstm_rollout_{name}_spread"] = [float(t.min()), float(t.max())]
        print(f"lstm rollout leg {name}: seconds median {np.median(t):.4f}  spread {t.min():.4f} .. {t.max():.4f}"
              f"  (T {T} x E {ppo.envs_per_proc})", flush=True)
    if len(legs) == 2:
        result["lstm_rollout_b_over_a"] = result["lstm_rollout_b_seconds"] / result["lstm_rollout_a_seconds"]


def timed(fn, ppo, N, check_every):
    ppo.loop_steps[0] = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = fn(ppo, N, check_every)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ppo.loop_steps[0], info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["both", "c2", "c3", "c5", "lstm"])
    ap.add_argument("--leg", default="both", choices=["both", "a", "b"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--runs-per-env", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rollout-steps", type=int, default=128, help="--shape lstm: env steps per env of the timed rollouts (0: skip them)")
    args = ap.parse_args()
    from ppo_and_friends_amd import testing
    testing.rank_print = lambda *a, **k: None        # the score report is not what is timed
    shapes = ["c2", "c3"] if args.shape == "both" else [args.shape]
    legs = {"a": leg_a, "b": leg_b}
    legs = legs if args.leg == "both" else {args.leg: legs[args.leg]}
    E, N = args.envs, args.envs * args.runs_per_env
    result = {"envs": E, "num_test_runs": N}
    for shape in shapes:
        ppo = make(shape, E, max(1, args.rollout_steps) if shape == "lstm" else 32)
        check_every = 50 if shape in ("c2", "lstm") else 64
        if shape == "lstm":
            assert ppo.policies["p"].lstm_step_unsupported_reason() == "", ppo.policies["p"].lstm_step_unsupported_reason()
            if "b" in legs:
                legs = dict(legs, b=leg_b_lstm)
            if args.rollout_steps > 0:
                time_rollouts(ppo, result, legs, args.repeats, args.warmup)
        elif "a" in legs:
            assert ppo.policies["p"].inference_unsupported_reason() == "", ppo.policies["p"].inference_unsupported_reason()
        if shape == "c5" and "b" in legs:
            legs = dict(legs, b=leg_b_mat)
        for name, fn in legs.items():
            for _ in range(args.warmup):
                timed(fn, ppo, N, check_every)
        times = {k: [] for k in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():             # alternating: drifts of clock / neighbours hit both legs alike
                dt, steps, info = timed(fn, ppo, N, check_every)
                times[name].append((dt, steps))
                result[f"{shape}_{name}_avg_score"] = info["p"]["avg_score"]
        for name in legs:
            sps = np.array([E * s / dt for dt, s in times[name]])
            result[f"{shape}_{name}_env_steps_per_s"] = float(np.median(sps))
            result[f"{shape}_{name}_spread"] = [float(sps.min()), float(sps.max())]
            result[f"{shape}_{name}_loop_steps"] = [s for _, s in times[name]]
            print(f"{shape} leg {name}: env-steps/s median {np.median(sps):12.0f}  spread {sps.min():12.0f} .. {sps.max():12.0f}"
                  f"  (loop steps {times[name][0][1]}, {np.median([dt for dt, _ in times[name]]) * 1e3:.1f} ms)", flush=True)
        if len(legs) == 2:
            result[f"{shape}_a_over_b"] = result[f"{shape}_a_env_steps_per_s"] / result[f"{shape}_b_env_steps_per_s"]
        del ppo
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
