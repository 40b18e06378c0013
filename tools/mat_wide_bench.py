"""
Rollout and update epoch of a MATPolicy whose per-agent observations are wider than 32 -- 3 agents, Discrete(5), 1024 envs x
128 steps, mini-batches of 256: the C5 dims of bench.py apart from the observation width, at O = 71 (robot_warehouse's
flattened default) and O = 128 (the kernels' limit) -- on K16 / K15 with the chunked observation front end
(csrc/mat_update.hip: mat_obs_encoder_wide; update_mode="fused") against update_mode="torch", which is what ran these
widths before.

Both legs live in one process; after a warm-up pass of each they are ALTERNATED `--repeats` times: the rollout =
PPO.rollout() (wall clock around a device synchronisation: env steps, the policy step, GAE), the epoch =
PPO._ppo_batch_train over 512 mini-batches (device events, shuffle draw included).  Prints, per width, the median and the
range (min .. max) of rollout ms, epoch ms and us per mini-batch of both legs, every alternation in which the fused leg was
not the faster one, the device launches per env step of one more rollout of each leg (torch.profiler; "n/a" where the
profiler gives no device events), and one JSON line.

    python tools/mat_wide_bench.py [--obs 71 128] [--envs 1024] [--steps 128] [--batch 256] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
A, NA = 3, 5


def make(mode, O, E, T, B):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.spaces import Box, Discrete
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, DEV, reward="uniform", seed=5, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    return PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=DEV, random_seed=4, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1, update_mode=mode,
               save_state=False)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def device_launches(fn):
    """Device kernel launches during fn(), or None when the profiler records none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA")
                and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())
        return n or None
    except Exception as exc:                                   # noqa: BLE001 -- a figure of the report, not of the run
        print(f"(launch count unavailable: {type(exc).__name__}: {exc})")
        return None


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def run_width(O, args):
    from ppo_and_friends_amd.ppo import PermutationLoader
    legs = {}
    for mode in ("fused", "torch"):
        ppo = make(mode, O, args.envs, args.steps, args.batch)
        pol = ppo.policies["mat"]
        upd = ppo._fused_updater("mat", args.batch)
        if mode == "fused":
            assert upd is not None and pol.fused_step_unsupported_reason() == "", pol.fused_step_unsupported_reason()
        else:
            assert upd is None
        ppo.rollout()                                          # warm-up: allocations, the first launches
        loader = PermutationLoader(pol.dataset, args.batch, ppo.loader_generator)
        pol.train()
        ppo._ppo_batch_train(loader, "mat")                    # warm-up: graph capture
        legs[mode] = dict(ppo=ppo, pol=pol, loader=loader, rollout=[], epoch=[])
    n_mb = -(-args.envs * args.steps // args.batch)
    for _ in range(args.repeats):
        for mode in ("fused", "torch"):
            leg = legs[mode]
            leg["rollout"].append(wall_ms(leg["ppo"].rollout))
            leg["pol"].train()
            leg["epoch"].append(event_ms(lambda leg=leg: leg["ppo"]._ppo_batch_train(leg["loader"], "mat")))
    out = dict(shape=dict(agents=A, O=O, actions=f"Discrete({NA})", envs=args.envs, steps=args.steps, batch=args.batch,
                          minibatches=n_mb))
    print(f"--- O = {O}: {A} agents, Discrete({NA}), {args.envs} envs x {args.steps} steps, batch {args.batch} ({n_mb} mini-batches), "
          f"{args.repeats} alternations")
    for mode, leg in legs.items():
        launches = device_launches(leg["ppo"].rollout)
        per_step = None if launches is None else launches / args.steps
        ro, ep = spread(leg["rollout"]), spread(leg["epoch"])
        out[mode] = dict(rollout_ms=ro, epoch_ms=ep, us_per_minibatch={k: 1e3 * v / n_mb for k, v in ep.items()},
                         launches_per_env_step=per_step)
        print(f"{mode:5s}: rollout {ro['median']:9.2f} ms ({ro['min']:.2f} .. {ro['max']:.2f}); epoch {ep['median']:9.2f} ms "
              f"({ep['min']:.2f} .. {ep['max']:.2f}) = {1e3 * ep['median'] / n_mb:8.2f} us per mini-batch "
              f"({1e3 * ep['min'] / n_mb:.2f} .. {1e3 * ep['max'] / n_mb:.2f}); launches per env step "
              f"{'n/a' if per_step is None else f'{per_step:.1f}'}")
    slower = [(i, what) for what in ("rollout", "epoch") for i in range(args.repeats)
              if legs["fused"][what][i] >= legs["torch"][what][i]]
    out["alternations_fused_not_faster"] = slower
    out["rollout_speedup"] = out["torch"]["rollout_ms"]["median"] / out["fused"]["rollout_ms"]["median"]
    out["epoch_speedup"] = out["torch"]["epoch_ms"]["median"] / out["fused"]["epoch_ms"]["median"]
    print(f"fused against torch: rollout x{out['rollout_speedup']:.2f}, epoch x{out['epoch_speedup']:.2f}; alternations in which "
          f"fused was not faster: {slower if slower else 'none'}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, nargs="+", default=[71, 128])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    results = [run_width(O, args) for O in args.obs]
    print(json.dumps(results))


if __name__ == "__main__":
    main()
