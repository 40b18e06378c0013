"""
One PPO iteration of an LSTM policy (rollout + `--epochs` update epochs at batch 256 on a synthetic environment), timed
with nn.LSTM / MIOpen (update_mode="auto") against K18 (update_mode="fused"), at two shapes:

  cart_pole_lstm : 4 observations, Discrete(2), LSTM 32, ff 16, sequence 5, LeakyReLU
  defaults       : 17 observations, Box(6), LSTM 128, ff 128, sequence 10, ReLU (the reference's LSTMNetwork defaults)

Both paths are warmed up, then timed alternately `--repeats` times each in this one process; env-steps/s are printed
as median and spread (min .. max) per path and shape, then one JSON line.

    python tools/lstm_bench.py [--shape cart_pole_lstm|defaults|both] [--mode both|auto|fused] [--repeats 3]
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

SHAPES = {
    "cart_pole_lstm": dict(O=4, action="discrete", n=2, H=32, F=16, S=5, act="leaky"),
    "defaults": dict(O=17, action="box", n=6, H=128, F=128, S=10, act="relu"),
}


def make_ppo(shape, mode, E, T, epochs, seed=0):
    import torch.nn as nn
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    space = Discrete(c["n"]) if c["action"] == "discrete" else Box(-1.0, 1.0, (c["n"],), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, c["O"], space, T, dev, reward="uniform", seed=11, term_prob=0.02)
    sp = Box(-np.inf, np.inf, (c["O"],), np.float32)
    act = nn.LeakyReLU() if c["act"] == "leaky" else nn.ReLU()
    kw = dict(sequence_length=c["S"], lstm_hidden_size=c["H"], ff_hidden_size=c["F"], activation=act)
    return PPO(env_gen, {"p": (None, sp, sp, space, dict(ac_network=LSTMNetwork, actor_kw_args=dict(kw),
                                                       critic_kw_args=dict(kw)))},
               device=dev, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E,
               ts_per_rollout=T, batch_size=256, epochs_per_iter=epochs, max_ts_per_ep=64, save_state=False,
               update_mode=mode)


def iteration(ppo):
    """Wall seconds of one rollout + epochs_per_iter update epochs (synchronised at both ends)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol = ppo.policies["p"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo.rollout()
    pol.train()
    for _ in range(ppo.epochs_per_iter):
        ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator, ppo._perm_cache), "p")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pol.clear_dataset()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["both", *SHAPES])
    ap.add_argument("--mode", default="both", choices=["both", "auto", "fused"])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128, help="env steps per rollout (E x T transitions)")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    shapes = list(SHAPES) if args.shape == "both" else [args.shape]
    modes = ["auto", "fused"] if args.mode == "both" else [args.mode]
    n = args.envs * args.steps
    result = {"transitions_per_iteration": n, "epochs": args.epochs, "batch_size": 256}
    for shape in shapes:
        ppos = {m: make_ppo(shape, m, args.envs, args.steps, args.epochs) for m in modes}
        for m in modes:
            for _ in range(args.warmup):
                iteration(ppos[m])
        times = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m in modes:                          # alternating: drifts of clock / neighbours hit both paths alike
                times[m].append(iteration(ppos[m]))
        for m in modes:
            sps = np.array([n / t for t in times[m]])
            name = "miopen" if m == "auto" else "hip"
            print(f"{shape:15s} {name:6s} env-steps/s median {np.median(sps):10.0f}  spread {sps.min():10.0f} .. "
                  f"{sps.max():10.0f}  (iteration {np.median(times[m]):.3f} s)", flush=True)
            result[f"{shape}_{name}_env_steps_per_s"] = float(np.median(sps))
            result[f"{shape}_{name}_spread"] = [float(sps.min()), float(sps.max())]
        if len(modes) == 2:
            result[f"{shape}_hip_over_miopen"] = result[f"{shape}_hip_env_steps_per_s"] / result[f"{shape}_miopen_env_steps_per_s"]
        del ppos
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
