"""
One ICM epoch and the per-env-step intrinsic reward at the reference baselines' ICM shape -- encoder 17 -> 128^3 -> 9,
inverse / forward model width 32, Box(6) actions, 4096 envs x 128 steps, mini-batches of 256 -- on K14's chain for ICMs with
widths of their own (csrc/icm_update_shapes.hip, update_mode="fused") against update_mode="torch", which is what ran this
shape before that chain existed.  Two more cases, each against the torch path that ran them until K14 covered them:

  --identity   the abmarl_blind_large_maze form: identity encoder (encoded_obs_dim = 0) on the agent's position (O 2),
               inverse / forward model width 128, Discrete(5) actions (csrc/icm_update_shapes.hip with enc_hidden = 0)
  --agents A   an agent-grouped MATPolicy of A agents (O 18, Discrete(5): the C5 dims of bench.py at A = 3) with the default
               ICM (one width, 128): one ICM sample per (row, agent) pair, so a mini-batch of `--batch` grouped rows is
               `--batch` x A ICM rows; `--envs` defaults to 1024 here, as C5's.  Combine with --identity for the identity ICM.
  --agents A --shared   the same policy with agent_shared_icm: ONE ICM per env over the group's A x 18 observation columns,
               actions MultiDiscrete([5] * A), one ICM row per grouped row.  Both legs run update_mode="fused"; the "fused" leg
               sets the opt-in PPOPolicy.fused_shared_icm (K14's shapes chain, n_action_slices = A), the "torch" leg leaves it
               off, which keeps the ICM epoch and MATPolicy.get_agent_shared_intrinsic_rewards on the torch path.  Combines
               with --identity.
  --action discrete:N | box:N   another action space for the single-agent cases (the syntax of tools/width_pairs_bench.py;
               Box bounds -1 .. 1), --obs-dim O another observation width.  Above 8 classes or dimensions the ICM needs
  --wide-actions   both legs run update_mode="auto" (the policy's own 18-output actor is not the subject and stays where it
               is); the "fused" leg sets the opt-in PPOPolicy.fused_wide_icm_actions (K14's shapes chain, the 32-column
               action form), the "torch" leg leaves it off, which keeps the ICM epoch and the reward on the torch path.
               mario_bros_ram's ICM: --wide-actions --action discrete:18 --obs-dim 256 --batch 128.

Both legs live in one process on the same rollout shape; after a warm-up pass of each they are ALTERNATED `--repeats`
times and timed with device events: the epoch = PPO._icm_batch_train over 2048 mini-batches (shuffle draw included), the
reward = PPOPolicy.get_intrinsic_reward on the 4096-row env batch (mean of `--reward-calls` back-to-back calls).  Prints the
median and the spread (min .. max) of both, the launches per mini-batch of the fused chain, and one JSON line.

    python tools/icm_shapes_bench.py [--identity] [--agents A [--shared]] [--action discrete:N|box:N] [--obs-dim O] [--wide-actions]
                                     [--envs 4096] [--steps 128] [--batch 256] [--repeats 5] [--reward-calls 50]
                                     [--allow-torch-path]

--allow-torch-path: do not insist that the "fused" leg has a fused updater -- for running this tool on a commit whose K14
does not cover the case yet (both legs then time the torch path, which is what that commit runs).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
BASELINE_KW = dict(encoded_obs_dim=9, encoder_hidden_size=128, inverse_hidden_size=32, forward_hidden_size=32)
IDENTITY_KW = dict(encoded_obs_dim=0, inverse_hidden_size=128, forward_hidden_size=128)


def action_space(spec):
    """--action discrete:N | box:N -> the space (Box bounds -1 .. 1 on every dimension)."""
    from ppo_and_friends_amd.spaces import Box, Discrete
    kind, _, n = spec.partition(":")
    if kind not in ("discrete", "box") or not n.isdigit() or int(n) < 1:
        raise ValueError(f"--action {spec!r}: expected discrete:N or box:N")
    return Discrete(int(n)) if kind == "discrete" else Box(-1.0, 1.0, (int(n),), np.float32)


def case_of(args):
    """-> (O, action space, agents, ICM keyword arguments) of the case the flags select."""
    from ppo_and_friends_amd.spaces import Box, Discrete
    if args.agents > 1:
        return 18, Discrete(5), args.agents, (dict(IDENTITY_KW) if args.identity else {})
    O, space, kw = (2, Discrete(5), IDENTITY_KW) if args.identity else (17, Box(-1.0, 1.0, (6,), np.float32), BASELINE_KW)
    return args.obs_dim or O, action_space(args.action) if args.action else space, 1, dict(kw)


def make(mode, E, T, B, case, shared=False, wide_actions=False):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    O, space, A, icm_kw = case
    cls = None
    if A > 1:
        from ppo_and_friends_amd.policies.mat_policy import MATPolicy
        cls = MATPolicy
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, DEV, reward="uniform", seed=5, num_agents=A)
    else:
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, DEV, reward="uniform", seed=5, term_prob=0.05)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    kw = dict(enable_icm=True, icm_kw_args=icm_kw)
    if shared:
        kw["agent_shared_icm"] = True
    ppo = PPO(env_gen, {"p": (cls, sp, sp, space, kw)}, device=DEV, random_seed=4,
              normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1,
              update_mode="fused" if shared else "auto" if wide_actions else mode)
    if shared and mode == "fused":
        ppo.policies["p"].fused_shared_icm = True              # the opt-in, before the first rollout
    if wide_actions and mode == "fused":
        ppo.policies["p"].fused_wide_icm_actions = True        # likewise
    ppo.rollout()
    return ppo


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--identity", action="store_true")
    ap.add_argument("--agents", type=int, default=1)
    ap.add_argument("--shared", action="store_true")
    ap.add_argument("--allow-torch-path", action="store_true")
    ap.add_argument("--action", default=None, help="discrete:N or box:N (single-agent cases)")
    ap.add_argument("--obs-dim", type=int, default=None, help="observation width (single-agent cases)")
    ap.add_argument("--wide-actions", action="store_true", help="the fused leg sets PPOPolicy.fused_wide_icm_actions")
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reward-calls", type=int, default=50)
    args = ap.parse_args()
    if args.shared and args.agents < 2:
        ap.error("--shared needs --agents A with A >= 2")
    if args.agents > 1 and (args.action or args.obs_dim or args.wide_actions):
        ap.error("--action, --obs-dim and --wide-actions are for the single-agent cases")
    if args.wide_actions:
        # (at 8 or fewer the opt-in changes nothing: both legs would run the fused chain and there is nothing to compare)
        try:
            width = action_space(args.action or "")
        except ValueError:
            ap.error("--wide-actions needs --action discrete:N or box:N with N in 9..24")
        width = width.n if hasattr(width, "n") else width.shape[0]
        if not 9 <= width <= 24:
            ap.error(f"--wide-actions needs an action width in 9..24 (--action {args.action}: {width})")
    if args.envs is None:
        args.envs = 1024 if args.agents > 1 else 4096
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    case = case_of(args)
    O, space, A, icm_kw = case
    legs, path = {}, {}
    for mode in ("fused", "torch"):
        ppo = make(mode, args.envs, args.steps, args.batch, case, args.shared, args.wide_actions)
        pol = ppo.policies["p"]
        upd = ppo._fused_icm_updater("p")
        path[mode] = "torch" if upd is None else "K14"
        if mode == "fused" and not args.allow_torch_path:
            assert upd is not None, FusedIcmUpdate.unsupported_reason(pol)
            assert bool(upd.topo.get("identity")) == args.identity, upd.topo
            assert not args.shared or upd.topo.get("n_action_slices") == A, upd.topo
            assert not args.wide_actions or upd.topo.get("general"), upd.topo
        elif mode == "torch":
            assert upd is None, "the torch leg got a fused ICM updater: there is no torch path to compare against at this shape"
        loader = PermutationLoader(pol.dataset, args.batch, ppo.loader_generator)
        buf = pol.buffer
        rows = args.envs * A                                     # the env batch of one step: one row per (env, agent)
        o1, o2 = buf.observations[0].reshape(rows, -1), buf.next_observations[0].reshape(rows, -1)
        act = buf.actions[0].reshape(rows, -1)
        if args.shared:                                          # the environment's agent-major batches [A E, .]
            major = lambda x: x.reshape(args.envs, A, -1).transpose(0, 1).reshape(rows, -1).contiguous()
            o1, o2, act = major(o1), major(o2), major(act)

        def epoch(ppo=ppo, loader=loader):
            ppo._icm_batch_train(loader, "p")

        def reward(pol=pol, o1=o1, o2=o2, act=act, n=args.reward_calls):
            call = pol.get_agent_shared_intrinsic_rewards if args.shared else pol.get_intrinsic_reward
            for _ in range(n):
                call(o1, o2, act)
        legs[mode] = dict(epoch=epoch, reward=reward, ms=[], us=[], upd=upd)
    n_mb = -(-args.envs * args.steps // args.batch)
    for leg in legs.values():                                  # warm-up pass: graph capture, allocations, autotuning
        leg["epoch"](); leg["reward"]()
    calls = PPOPolicy.fused_icm_reward_calls
    topo = {} if legs["fused"]["upd"] is None else legs["fused"]["upd"].topo
    for _ in range(max(5, args.repeats)):
        for mode in ("fused", "torch"):
            leg = legs[mode]
            leg["ms"].append(timed(leg["epoch"]))
            leg["us"].append(1e3 * timed(leg["reward"]) / args.reward_calls)
    if not args.allow_torch_path:
        assert PPOPolicy.fused_icm_reward_calls - calls == max(5, args.repeats) * args.reward_calls, "the fused leg's rewards took the torch path"
    # launches per mini-batch: [encoder forward,] the models (one launch per model when their widths differ) [, encoder
    # backward], weight gradients; the one-width chain fuses its first three into one launch where it can
    if not topo:
        launches = None
    elif topo.get("general"):
        launches = (1 if topo["inv_hidden"] == topo["fwd_hidden"] else 2) + (1 if topo.get("identity") else 3)
    else:
        launches = 2 if legs["fused"]["upd"].fuse_reason() == "" else 4
    out = dict(shape=dict(O=O, actions=f"Discrete({space.n})" if hasattr(space, "n") else f"Box({space.shape[0]})", agents=A, envs=args.envs, steps=args.steps, batch=args.batch,
                          shared_icm=args.shared, wide_actions=args.wide_actions, icm_rows_per_minibatch=args.batch * (1 if args.shared else A), minibatches=n_mb,
                          **icm_kw),
               path=path, fused_launches_per_minibatch=launches)
    for mode, leg in legs.items():
        ms, us = leg["ms"], leg["us"]
        out[mode] = dict(epoch_ms_median=statistics.median(ms), epoch_ms_min=min(ms), epoch_ms_max=max(ms),
                         us_per_minibatch=1e3 * statistics.median(ms) / n_mb,
                         reward_us_median=statistics.median(us), reward_us_min=min(us), reward_us_max=max(us))
        print(f"{mode:5s} ({path[mode]}): ICM epoch {statistics.median(ms):9.2f} ms ({min(ms):.2f} .. {max(ms):.2f}) = "
              f"{1e3 * statistics.median(ms) / n_mb:7.2f} us per mini-batch; reward call {statistics.median(us):8.1f} us "
              f"({min(us):.1f} .. {max(us):.1f})")
    out["epoch_speedup"] = out["torch"]["epoch_ms_median"] / out["fused"]["epoch_ms_median"]
    out["reward_speedup"] = out["torch"]["reward_us_median"] / out["fused"]["reward_us_median"]
    print(f"fused chain: {out['fused_launches_per_minibatch']} launches per mini-batch; epoch x{out['epoch_speedup']:.2f}, "
          f"reward x{out['reward_speedup']:.2f} against the torch path")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
