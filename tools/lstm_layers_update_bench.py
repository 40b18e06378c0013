"""
The update epoch of a two-layer LSTM policy measured on the GPU: K22 for two stacked layers (opt-in
`fused_lstm_layers_update`, csrc/lstm_stacked_update.hip, four cursor-driven launches per mini-batch replayed from
hipGraphs) against the same policy with the opt-in off (the mini-batch loop on K18's two-layer kernels), at the two
shapes of tools/lstm_layers_bench.py: H 32 / ff 16 / S 10 and H 128 / ff 128 / S 10.  The two legs alternate `--repeats`
times in one process after two warm-up epochs each (the first eager, which also counts the driver's launches per
mini-batch; the second captures the graphs); reported are median and range, and whether the fused leg won every
alternation.

    python tools/lstm_layers_update_bench.py [--envs 256] [--steps 128] [--batch 256] [--repeats 5]
                                             [--out profiles/lstm_layers_update.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(fused, H, F, S, envs, steps, batch):
    import torch
    from ppo_and_friends_amd import testing
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.spaces import Box, Discrete
    testing.rank_print = lambda *a, **k: None
    PPOPolicy.fused_lstm_layers, PPOPolicy.fused_lstm_layers_update = True, fused
    dev = torch.device("cuda", 0)
    space, sp = Discrete(2), Box(-np.inf, np.inf, (4,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(envs, 4, space, steps, dev, reward="uniform", seed=13, term_prob=0.02)
    kw = dict(sequence_length=S, lstm_hidden_size=H, num_lstm_layers=2, ff_hidden_size=F)
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(ac_network=LSTMNetwork, actor_kw_args=kw, critic_kw_args=kw))},
              device=dev, random_seed=1, normalize_obs=False, normalize_rewards=False, envs_per_proc=envs,
              ts_per_rollout=steps, batch_size=batch, epochs_per_iter=1, max_ts_per_ep=steps, save_state=False,
              update_mode="fused", use_graphs=False)
    pol = ppo.policies["p"]
    pol.fused_lstm_layers_update = fused                       # (the class attribute goes back and forth between the legs)
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
    from ppo_and_friends_amd.fused_update import FusedLstm2Update, FusedLstmUpdate
    legs = {"fused": make(True, H, F, S, args.envs, args.steps, args.batch), "loop": make(False, H, F, S, args.envs, args.steps, args.batch)}
    n_mb = (len(legs["fused"][1].dataset) + args.batch - 1) // args.batch
    say(f"update epoch, two layers, H {H} ff {F} S {S}: {args.envs} envs x {args.steps} steps, batch {args.batch}, {n_mb} mini-batches")
    before = FusedLstmUpdate.launches
    for leg in legs.values():
        epoch(*leg)                                            # eager
    ppo = legs["fused"][0]
    assert isinstance(ppo._fused_updater("p", args.batch), FusedLstm2Update) and legs["loop"][0]._fused_updater("p", args.batch) is None
    say(f"  fused: {(FusedLstmUpdate.launches - before) / n_mb:.2f} launches per mini-batch (the driver's counter over one eager epoch)")
    ppo.use_graphs = True
    for leg in legs.values():
        epoch(*leg)                                            # captures
    t = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, leg in legs.items():
            t[k].append(epoch(*leg))
    for k in legs:
        x = np.asarray(t[k])
        say(f"  {k:5s}: epoch seconds median {np.median(x):.4f}  range {x.min():.4f} .. {x.max():.4f}  "
            f"({np.median(x) / n_mb * 1e6:.0f} us per mini-batch)")
    wins = sum(a < b for a, b in zip(t["fused"], t["loop"]))
    say(f"  loop / fused (medians) {np.median(t['loop']) / np.median(t['fused']):.2f}x; the fused leg was faster in {wins} of {args.repeats} alternations")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    epochs(say, args, 32, 16, 10)
    epochs(say, args, 128, 128, 10)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
