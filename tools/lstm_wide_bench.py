"""
256-wide LSTM networks (opt-in `fused_lstm_wide`, csrc/lstm_wide.hip) measured on the GPU:

  1. one update epoch and one rollout of a one-layer LSTM policy with H 256, ff 128, S 10 under update_mode="fused" with
     the opt-in on (forward_logits and the mini-batch loop on K18's 256-wide kernels) against the same policy under "auto"
     (nn.LSTM / MIOpen).  The two legs alternate `--repeats` times in one process after one warm-up each; reported are
     median and range, and whether the HIP leg won every alternation.
  2. the 256-wide forward kernel alone at S 16, N 256 against the H 128 kernel at the same shape (in 4 -> H -> ff 64 ->
     2 outputs, no stash), median of `--launches` launches timed with events.

    python tools/lstm_wide_bench.py [--envs 256] [--steps 128] [--batch 256] [--repeats 5] [--out profiles/lstm_wide.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(mode, H, F, S, envs, steps, batch):
    import torch
    from ppo_and_friends_amd import testing
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.spaces import Box, Discrete
    testing.rank_print = lambda *a, **k: None
    dev = torch.device("cuda", 0)
    space, sp = Discrete(2), Box(-np.inf, np.inf, (4,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(envs, 4, space, steps, dev, reward="uniform", seed=13, term_prob=0.02)
    kw = dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=F)
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
              device=dev, random_seed=1, normalize_obs=False, normalize_rewards=False, envs_per_proc=envs,
              ts_per_rollout=steps, batch_size=batch, epochs_per_iter=1, max_ts_per_ep=steps, save_state=False, update_mode=mode)
    pol = ppo.policies["p"]
    assert pol.actor.use_hip == (mode == "fused")
    return ppo, pol


def rollout(ppo, pol):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo.rollout()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def epoch(ppo, pol):
    import torch
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator), "p")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def policy_legs(say, args, H, F, S):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    PPOPolicy.fused_lstm_wide = True
    legs = {"hip": make("fused", H, F, S, args.envs, args.steps, args.batch), "torch": make("auto", H, F, S, args.envs, args.steps, args.batch)}
    say(f"one layer, H {H} ff {F} S {S}: {args.envs} envs x {args.steps} steps, batch {args.batch}")
    for what, run in (("rollout", rollout), ("epoch", epoch)):
        for leg in legs.values():
            run(*leg)
        t = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, leg in legs.items():
                t[k].append(run(*leg))
        for k in legs:
            x = np.asarray(t[k])
            say(f"  {what:7s} {k:5s}: seconds median {np.median(x):.4f}  range {x.min():.4f} .. {x.max():.4f}")
        wins = sum(a < b for a, b in zip(t["hip"], t["torch"]))
        say(f"  {what:7s} torch / hip (medians) {np.median(t['torch']) / np.median(t['hip']):.2f}x; the HIP leg was faster in "
            f"{wins} of {args.repeats} alternations")


def forward_kernels(say, args):
    import torch
    from ppo_and_friends_amd import kernels as K
    dev = torch.device("cuda", 0)
    N, S, I, F, O = 256, 16, 4, 64, 2
    say(f"forward kernel alone, N {N} S {S} in {I} ff {F} out {O}, no stash, median of {args.launches} launches (us)")
    med = {}
    for H in (128, 256):
        g = torch.Generator().manual_seed(H)
        x = torch.rand(N, S, I, generator=g).to(dev)
        bucket = torch.zeros(4, device=dev)
        n = K.lstm_sizes(K.lstm_desc(I, H, F, 1, O, K.ACT_TANH, N, S, bucket))[1]
        bucket = (0.2 * torch.rand(n, generator=g) - 0.1).to(dev)
        desc = K.lstm_desc(I, H, F, 1, O, K.ACT_TANH, N, S, bucket)
        h0 = (torch.rand(N, H, generator=g) - 0.5).to(dev)
        for _ in range(10):
            K.lstm_forward(desc, x, h0, h0, False)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
        for a, b in ev:
            a.record()
            K.lstm_forward(desc, x, h0, h0, False)
            b.record()
        torch.cuda.synchronize()
        med[H] = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
    say(f"  H 128 {med[128]:7.1f}   H 256 {med[256]:7.1f}   ratio {med[256] / med[128]:.2f} (4x the recurrent multiply-adds)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    forward_kernels(say, args)
    policy_legs(say, args, 256, 128, 10)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
