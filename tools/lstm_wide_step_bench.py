"""
The one-launch step of a 256-wide LSTM policy (opt-in `fused_lstm_wide_step`, csrc/lstm_wide_step.hip) measured on the GPU
against the same policy with the opt-in off (forward_logits on K18 + torch operators), both under update_mode="fused"
with `fused_lstm_wide`, on BatchedCartPoleEnv at H 256 / ff 128: a rollout of `--steps` steps x `--envs` envs (all of
PPO.rollout) and evaluation (test_policy, deterministic) in env-steps/s.  Both legs live in one process, are warmed up
once each and then alternate `--repeats` times; wall time between two device synchronisations; reported are median and
range per leg, whether the opt-in leg won every alternation, and the device launches per env step of one more rollout /
evaluation of each leg (torch.profiler).

    python tools/lstm_wide_step_bench.py [--envs 256] [--steps 128] [--repeats 5] [--out profiles/lstm_wide_step.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lstm_layers_step_bench import device_launches, timed  # noqa: E402  (one copy of the clock and the launch count)


def make(step_opt_in, envs, steps):
    import torch
    from ppo_and_friends_amd import testing
    from ppo_and_friends_amd.environments.cartpole import BatchedCartPoleEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.spaces import Discrete
    testing.rank_print = lambda *a, **k: None
    dev = torch.device("cuda", 0)
    PPOPolicy.fused_lstm_wide, PPOPolicy.fused_lstm_wide_step = True, step_opt_in
    env_gen = lambda: BatchedCartPoleEnv(envs, dev, seed=0)
    sp = env_gen().observation_space
    kw = dict(sequence_length=10, lstm_hidden_size=256, ff_hidden_size=128)
    ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(2), dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
              device=dev, random_seed=1, envs_per_proc=envs, ts_per_rollout=steps, batch_size=256, epochs_per_iter=1,
              max_ts_per_ep=64, save_state=False, update_mode="fused")
    pol = ppo.policies["p"]
    pol.fused_lstm_wide_step = step_opt_in                     # (the instance keeps its leg whatever the class says later)
    assert (pol.lstm_step_unsupported_reason() == "") == step_opt_in
    return ppo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--eval-steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from ppo_and_friends_amd.testing import test_policy
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    legs = {"on": make(True, args.envs, args.steps), "off": make(False, args.envs, args.steps)}
    loop = args.eval_steps

    def eval_run(ppo):
        try:                                                   # more runs than the loop can finish: max_steps ends it
            return test_policy(ppo, 1000 * args.envs, deterministic=True, check_every=loop, max_steps=loop)
        except RuntimeError as exc:                            # the loop bound is the measurement's length
            if "max_steps" not in str(exc):
                raise
            return None
    say(f"H 256 ff 128: rollout {args.steps} steps x {args.envs} envs; evaluation {loop} loop steps x {args.envs} envs")
    for ppo in legs.values():
        ppo.rollout()
        eval_run(ppo)
    roll, ev = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, ppo in legs.items():
            roll[k].append(timed(ppo.rollout)[0])
        for k, ppo in legs.items():
            ev[k].append(loop * args.envs / timed(lambda: eval_run(ppo))[0])
    counts = {k: (device_launches(ppo.rollout), device_launches(lambda: eval_run(ppo))) for k, ppo in legs.items()}
    per = lambda n, d: "n/a" if n is None else f"{n / d:.1f}"
    for k in legs:
        r, e = np.asarray(roll[k]) * 1e3, np.asarray(ev[k])
        say(f"  opt-in {k:3s}: rollout ms median {np.median(r):.2f}  range {r.min():.2f} .. {r.max():.2f}  "
            f"launches per env step {per(counts[k][0], args.steps)}")
        say(f"              evaluation env-steps/s median {np.median(e):.0f}  range {e.min():.0f} .. {e.max():.0f}  "
            f"launches per loop step {per(counts[k][1], loop)}")
    wins_r = sum(a < b for a, b in zip(roll["on"], roll["off"]))
    wins_e = sum(a > b for a, b in zip(ev["on"], ev["off"]))
    say(f"  off / on (medians): rollout {np.median(roll['off']) / np.median(roll['on']):.2f}x, evaluation "
        f"{np.median(ev['on']) / np.median(ev['off']):.2f}x; the opt-in leg was faster in {wins_r} (rollout) and {wins_e} "
        f"(evaluation) of {args.repeats} alternations")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
