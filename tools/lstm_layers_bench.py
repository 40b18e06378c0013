"""
Two stacked LSTM layers (opt-in `fused_lstm_layers`, csrc/lstm_stacked.hip) measured on the GPU:

  1. one update epoch of a two-layer LSTM policy under update_mode="fused" with the opt-in on (the mini-batch loop on
     K18's two-layer kernels) against the same policy under "auto" (nn.LSTM / MIOpen), at the cart-pole LSTM shape (H 32,
     ff 16, S 10) and at the reference defaults (H 128, ff 128, S 10).  The two legs alternate `--repeats` times in one
     process after one warm-up epoch each; reported are median and range, and whether the HIP leg won every alternation.
  2. the two-layer forward kernel alone at S 16, N 256 per H against the one-layer forward kernel at the same shape
     (in 4 -> H -> ff 64 -> 2 outputs, no stash), median of `--launches` launches timed with events.

    python tools/lstm_layers_bench.py [--envs 256] [--steps 128] [--batch 256] [--repeats 5] [--out profiles/lstm_layers.txt]
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
    kw = dict(sequence_length=S, lstm_hidden_size=H, num_lstm_layers=2, ff_hidden_size=F)
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
              device=dev, random_seed=1, normalize_obs=False, normalize_rewards=False, envs_per_proc=envs,
              ts_per_rollout=steps, batch_size=batch, epochs_per_iter=1, max_ts_per_ep=steps, save_state=False, update_mode=mode)
    pol = ppo.policies["p"]
    assert pol.actor.use_hip == (mode == "fused")
    ppo.rollout()
    pol.train()
    torch.cuda.synchronize()
    return ppo, pol


def epoch(ppo, pol):
    import torch
    from ppo_and_friends_amd.ppo import PermutationLoader
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator), "p")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def epochs(say, args, H, F, S):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    PPOPolicy.fused_lstm_layers = True
    legs = {"hip": make("fused", H, F, S, args.envs, args.steps, args.batch), "torch": make("auto", H, F, S, args.envs, args.steps, args.batch)}
    n_mb = (len(legs["hip"][1].dataset) + args.batch - 1) // args.batch
    say(f"epoch, two layers, H {H} ff {F} S {S}: {args.envs} envs x {args.steps} steps, batch {args.batch}, {n_mb} mini-batches")
    for leg in legs.values():
        epoch(*leg)
    t = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, leg in legs.items():
            t[k].append(epoch(*leg))
    for k in legs:
        x = np.asarray(t[k])
        say(f"  {k:5s}: epoch seconds median {np.median(x):.4f}  range {x.min():.4f} .. {x.max():.4f}  "
            f"({np.median(x) / n_mb * 1e6:.0f} us per mini-batch)")
    wins = sum(a < b for a, b in zip(t["hip"], t["torch"]))
    say(f"  torch / hip (medians) {np.median(t['torch']) / np.median(t['hip']):.2f}x; the HIP leg was faster in {wins} of {args.repeats} alternations")


def forward_kernels(say, args):
    import torch
    from ppo_and_friends_amd import kernels as K
    dev = torch.device("cuda", 0)
    N, S, I, F, O = 256, 16, 4, 64, 2
    say(f"forward kernel alone, N {N} S {S} in {I} ff {F} out {O}, no stash, median of {args.launches} launches (us)")
    for H in (32, 64, 128):
        g = torch.Generator().manual_seed(H)
        x = torch.rand(N, S, I, generator=g).to(dev)
        med = {}
        for layers in (1, 2):
            desc_of, sizes, fwd = (K.lstm_desc, K.lstm_sizes, K.lstm_forward) if layers == 1 else (K.lstm2_desc, K.lstm2_sizes, K.lstm2_forward)
            bucket = torch.zeros(4, device=dev)
            n = sizes(desc_of(I, H, F, 1, O, K.ACT_TANH, N, S, bucket))[1]
            bucket = (0.2 * torch.rand(n, generator=g) - 0.1).to(dev)
            desc = desc_of(I, H, F, 1, O, K.ACT_TANH, N, S, bucket)
            h0 = (torch.rand(*((N, H) if layers == 1 else (2, N, H)), generator=g) - 0.5).to(dev)
            for _ in range(10):
                fwd(desc, x, h0, h0, False)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
            for a, b in ev:
                a.record()
                fwd(desc, x, h0, h0, False)
                b.record()
            torch.cuda.synchronize()
            med[layers] = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
        say(f"  H {H:3d}: one layer {med[1]:7.1f}   two layers {med[2]:7.1f}   ratio {med[2] / med[1]:.2f}")


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
    epochs(say, args, 32, 16, 10)
    epochs(say, args, 128, 128, 10)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
