"""
One rollout and one update epoch of an MLP policy at `lunar_lander`'s dimensions -- 8 observations, Discrete(4), 64-wide
actor and 256-wide critic of depth 3, 4096 envs x 128 steps, batch 256 (2048 mini-batches per epoch, hipGraph replay) -- on
the fused kernels (update_mode="fused": K6+K7 rollout steps, K12 update on the pair <64, 256>: the critic's row tiles on
workgroup pairs, the fused tail) against the torch-ROCm path (update_mode="torch": what "auto" ran for this width pair
before the pair was instantiated).  A 128 / 256 policy at the same dimensions runs on the fused path beside them: the
critic's row pairs set fwd_bwd's time in both, so the narrower actor should cost nothing.

All legs are warmed up, then timed alternately `--repeats` times each in this one process, each timing between two device
synchronisations; seconds are printed as median and spread (min .. max) per leg, then one JSON line.

    python tools/width_pairs_bench.py [--repeats 5] [--envs 4096] [--steps 128]

--widths A C times another pair instead, at `bipedal_walker_hardcore`'s dimensions (24 observations, Box(4), depth 3): the
policy under update_mode="fused" against the same policy under update_mode="torch", by the same protocol.  `--widths 256 512`
is the wide pair (K12 ends in the wgrad and Adam launches there: profiles/wide_critic.txt).

--obs-dim N (with --widths) times the pair at the RAM baselines' dimensions instead: N observations, Discrete(4), depth 3
(--action discrete:N | box:N and --activation relu | leaky_relu | tanh for another head and activation; --wide-heads sets
PPOPolicy.fused_wide_heads, which the pair needs above 8 actor outputs: profiles/wide_heads.txt).
--wide-inputs sets PPOPolicy.fused_wide_inputs, which a wide pair needs above 64 inputs, and --batch the mini-batch size:

    python tools/width_pairs_bench.py --widths 256 512 --obs-dim 128 --wide-inputs --batch 128

is `breakout_ram` / `mario_bros_ram` at --hist_size 1 (128 RAM bytes, batch 128: 4096 mini-batches per epoch;
profiles/wide_inputs.txt).  --wide-shapes sets PPOPolicy.fused_wide_shapes instead (in_dim <= 512, mini-batches <= 1024):

    python tools/width_pairs_bench.py --widths 256 512 --obs-dim 256 --wide-shapes --batch 128
    python tools/width_pairs_bench.py --widths 256 512 --obs-dim 142 --wide-shapes --batch 1000

are `breakout_ram` at the reference's default --hist_size 2 and the critic of `robot_warehouse`'s MAPPO members at their
default batch (profiles/wide_shapes.txt).
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

LEGS = {"64x256_fused": ((64, 256), "fused"), "64x256_torch": ((64, 256), "torch"), "128x256_fused": ((128, 256), "fused")}
BATCH = 256


ACTIVATIONS = {"relu": "ReLU", "leaky_relu": "LeakyReLU", "tanh": "Tanh"}


def action_space(spec):
    """--action discrete:N | box:N -> the space (Box bounds -0.4 .. 0.4 on every dimension, humanoid's)."""
    from ppo_and_friends_amd.spaces import Box, Discrete
    kind, _, n = spec.partition(":")
    if kind not in ("discrete", "box") or not n.isdigit() or int(n) < 1:
        raise ValueError(f"--action {spec!r}: expected discrete:N or box:N")
    return Discrete(int(n)) if kind == "discrete" else Box(-0.4, 0.4, (int(n),), np.float32)


def make_ppo(widths, mode, E, T, seed=1, walker=False, obs_dim=None, action="discrete:4", activation="relu"):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    O, space = (24, Box(-1.0, 1.0, (4,), np.float32)) if walker else (8, Discrete(4))
    if obs_dim is not None:
        O, space = obs_dim, action_space(action)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="ones", seed=1234)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    act = lambda: getattr(torch.nn, ACTIVATIONS[activation])()
    pargs = dict(actor_kw_args=dict(hidden_size=widths[0], hidden_depth=3, activation=act()),
                 critic_kw_args=dict(hidden_size=widths[1], hidden_depth=3, activation=act()))
    return PPO(env_gen, {"p": (None, sp, sp, space, pargs)}, device=dev, random_seed=seed, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=BATCH, epochs_per_iter=1,
               save_state=False, update_mode=mode)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def rollout_and_epoch(ppo):
    """(seconds of one rollout, seconds of one update epoch on it)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol = ppo.policies["p"]
    t_roll = timed(ppo.rollout)
    pol.train()
    loader = PermutationLoader(pol.dataset, BATCH, ppo.loader_generator)
    t_epoch = timed(lambda: ppo._ppo_batch_train(loader, "p"))
    return t_roll, t_epoch


def main():
    global BATCH
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128, help="env steps per rollout (E x T transitions)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--widths", type=int, nargs=2, metavar=("ACTOR", "CRITIC"), default=None,
                    help="this pair, fused against torch, at bipedal_walker_hardcore's dimensions (default: the 64 / 256 legs)")
    ap.add_argument("--obs-dim", type=int, default=None, help="with --widths: this many observations and Discrete(4) actions")
    ap.add_argument("--wide-inputs", action="store_true", help="PPOPolicy.fused_wide_inputs = True (a wide pair above 64 inputs)")
    ap.add_argument("--wide-shapes", action="store_true",
                    help="PPOPolicy.fused_wide_shapes = True (a wide pair above 128 inputs or above 512 rows per mini-batch)")
    ap.add_argument("--wide-heads", action="store_true",
                    help="PPOPolicy.fused_wide_heads = True (a wide pair's actor with 9 .. 24 outputs, Discrete or Box)")
    ap.add_argument("--wide-ranks", action="store_true",
                    help="PPOPolicy.fused_wide_ranks = True (a wide pair on N > 1 ranks, under a launcher: profiles/wide_ranks.txt)")
    ap.add_argument("--action", default="discrete:4", help="with --obs-dim: discrete:N or box:N (default discrete:4)")
    ap.add_argument("--activation", choices=sorted(ACTIVATIONS), default="relu")
    ap.add_argument("--batch", type=int, default=BATCH, help="mini-batch size")
    args = ap.parse_args()
    if args.obs_dim is not None and not args.widths:
        ap.error("--obs-dim goes with --widths")
    BATCH = args.batch
    if args.wide_inputs:
        from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
        PPOPolicy.fused_wide_inputs = True
    if args.wide_shapes:
        from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
        PPOPolicy.fused_wide_shapes = True
    if args.wide_heads:
        from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
        PPOPolicy.fused_wide_heads = True
    if args.wide_ranks:
        from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
        PPOPolicy.fused_wide_ranks = True
    # under a launcher, or PPOAF_REHEARSE_MULTI_RANK=1 (one rank on the N > 1 path): the process group (no-op otherwise)
    from ppo_and_friends_amd.utils import mpi_utils
    mpi_utils.init_process_group_from_env()
    legs, pair = LEGS, "64x256"
    if args.widths:
        pair = f"{args.widths[0]}x{args.widths[1]}"
        legs = {f"{pair}_{m}": (tuple(args.widths), m) for m in ("fused", "torch")}
    n = args.envs * args.steps
    result = {"transitions": n, "batch_size": BATCH, "minibatches_per_epoch": (n + BATCH - 1) // BATCH, "repeats": args.repeats}
    if args.obs_dim is not None:
        result.update(obs_dim=args.obs_dim, wide_inputs=bool(args.wide_inputs))
        if args.wide_shapes:
            result.update(wide_shapes=True)
        if args.wide_heads or args.action != "discrete:4" or args.activation != "relu":
            result.update(wide_heads=bool(args.wide_heads), action=args.action, activation=args.activation)
    ppos = {k: make_ppo(w, m, args.envs, args.steps, walker=bool(args.widths), obs_dim=args.obs_dim, action=args.action,
                        activation=args.activation) for k, (w, m) in legs.items()}
    for k, ppo in ppos.items():                      # the path each leg takes, as the JSON line reports it
        pol = ppo.policies["p"]
        fused = ppo._fused_updater("p", BATCH)
        step_on = ppo.update_mode != "torch" and pol.fused_step_unsupported_reason() == ""
        result[f"{k}_rollout_path"] = "K6+K7" if step_on else "torch"
        result[f"{k}_update_path"] = "torch" if fused is None else \
            "K12" + (", row pairs" if fused.pairs_reason() == "" else "") + (", fused tail" if fused.tail_reason() == "" else "") \
            + (", N > 1 path" if fused.multi else "")
        for _ in range(args.warmup):
            rollout_and_epoch(ppo)
    times = {k: [] for k in ppos}
    for _ in range(args.repeats):
        for k, ppo in ppos.items():                  # alternating: drifts of clock / neighbours hit all legs alike
            times[k].append(rollout_and_epoch(ppo))
    for k in ppos:
        for j, what in enumerate(("rollout", "epoch")):
            t = np.array([x[j] for x in times[k]])
            path = result[k + ("_rollout_path" if what == "rollout" else "_update_path")]
            print(f"{k:14s} {what:8s} median {np.median(t) * 1e3:9.2f} ms  spread {t.min() * 1e3:9.2f} .. {t.max() * 1e3:9.2f} ms"
                  f"   ({path})", flush=True)
            result[f"{k}_{what}_s"] = float(np.median(t))
            result[f"{k}_{what}_spread_s"] = [float(t.min()), float(t.max())]
    for what in ("rollout", "epoch"):
        result[f"{pair}_{what}_torch_over_fused"] = result[f"{pair}_torch_{what}_s"] / result[f"{pair}_fused_{what}_s"]
    if args.widths:
        nb = result["minibatches_per_epoch"]
        result[f"{pair}_fused_us_per_minibatch"] = result[f"{pair}_fused_epoch_s"] / nb * 1e6
        result[f"{pair}_torch_us_per_minibatch"] = result[f"{pair}_torch_epoch_s"] / nb * 1e6
        # the pair's reason to exist: the fused epoch's median below the fastest of the torch path's runs
        result[f"{pair}_fused_median_below_fastest_torch"] = bool(
            result[f"{pair}_fused_epoch_s"] < result[f"{pair}_torch_epoch_spread_s"][0])
        # ... and leg against leg inside each alternation
        for j, what in enumerate(("rollout", "epoch")):
            result[f"{pair}_fused_{what}_faster_in_every_alternation"] = bool(
                all(f[j] < t[j] for f, t in zip(times[f"{pair}_fused"], times[f"{pair}_torch"])))
    else:
        result["epoch_64x256_over_128x256"] = result["64x256_fused_epoch_s"] / result["128x256_fused_epoch_s"]
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
