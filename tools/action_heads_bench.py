"""
One PPO iteration (rollout + `--epochs` update epochs at batch 256, hipGraph replay) at C2's shape -- 4096 envs x 128
steps, 4 observations, 128^3 ReLU actor and critic -- with a MultiDiscrete([3, 3, 2]) or a MultiBinary(4) action head,
timed on the torch-ROCm path (update_mode="auto") against the fused kernels (update_mode="fused": K6+K7 rollout steps
and the K12 update with the heads of csrc/action_heads.hpp).

Both paths are warmed up, then timed alternately `--repeats` times each in this one process; env-steps/s are printed as
median and spread (min .. max) per head and path, then one JSON line.

    python tools/action_heads_bench.py [--head multi_discrete|multi_binary|both] [--mode both|auto|fused] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS = {"multi_discrete": [3, 3, 2], "multi_binary": 4}


def make_ppo(head, mode, E, T, epochs, seed=1):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, MultiBinary, MultiDiscrete
    dev = torch.device("cuda", 0)
    space = MultiDiscrete(HEADS[head]) if head == "multi_discrete" else MultiBinary(HEADS[head])
    env_gen = lambda: SyntheticFixedLengthEnv(E, 4, space, T, dev, reward="ones", seed=1234)
    sp = Box(-np.inf, np.inf, (4,), np.float32)
    return PPO(env_gen, {"p": (None, sp, sp, space, {})}, device=dev, random_seed=seed, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=256, epochs_per_iter=epochs,
               save_state=False, update_mode=mode)


def iteration(ppo):
    """Wall seconds of one rollout + epochs_per_iter update epochs (synchronised at both ends)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo.rollout()
    ppo.train_on_rollout()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default="both", choices=["both", *HEADS])
    ap.add_argument("--mode", default="both", choices=["both", "auto", "fused"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128, help="env steps per rollout (E x T transitions)")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    heads = list(HEADS) if args.head == "both" else [args.head]
    modes = ["auto", "fused"] if args.mode == "both" else [args.mode]
    n = args.envs * args.steps
    result = {"transitions_per_iteration": n, "epochs": args.epochs, "batch_size": 256}
    for head in heads:
        ppos = {m: make_ppo(head, m, args.envs, args.steps, args.epochs) for m in modes}
        for m in modes:                              # the path each mode takes, as the JSON line reports it
            pol = ppos[m].policies["p"]
            result[f"{head}_{m}_rollout"] = "K6+K7" if pol.fused_step_unsupported_reason() == "" else "torch"
            result[f"{head}_{m}_update"] = "K12" if ppos[m]._fused_updater("p", 256) is not None else "torch"
            for _ in range(args.warmup):
                iteration(ppos[m])
        times = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m in modes:                          # alternating: drifts of clock / neighbours hit both paths alike
                times[m].append(iteration(ppos[m]))
        for m in modes:
            sps = np.array([n / t for t in times[m]])
            print(f"{head:15s} {m:6s} env-steps/s median {np.median(sps):10.0f}  spread {sps.min():10.0f} .. "
                  f"{sps.max():10.0f}  (iteration {np.median(times[m]):.3f} s)", flush=True)
            result[f"{head}_{m}_env_steps_per_s"] = float(np.median(sps))
            result[f"{head}_{m}_spread"] = [float(sps.min()), float(sps.max())]
        if len(modes) == 2:
            result[f"{head}_fused_over_auto"] = result[f"{head}_fused_env_steps_per_s"] / result[f"{head}_auto_env_steps_per_s"]
        del ppos
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
