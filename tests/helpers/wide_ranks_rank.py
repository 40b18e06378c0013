"""
One rank of tests/test_gpu_wide_ranks.py's multi-process runs (spawned by that test, never collected): a (256, 512) policy of
depth 2 under update_mode="fused" with PPOPolicy.fused_wide_ranks on N ranks that share the one GPU (collectives over gloo).
A run is described by a scenario dict:

  mode        PPOAF_GRAD_EXCHANGE ("auto" | "rccl": the pair takes the all-reduce route under either)
  refusal     first build the PPO with the attribute off and keep what it raises
  train       None, or dict(E, T, O, B, normalize_values, identical, shapes, drop): one iteration of two epochs (identical:
              every rank gets rank 0's env and random streams and no clip; w0_from: the run whose initial weights are taken;
              drop: after it drop_peer_exchange("test") on every driver and a second iteration)
  members     None, or dict(E, T, B, normalize_values): one iteration of a multi-policy run with two wide members (MEMBERS)
  grads       [(name, case of test_gpu_k12_gradients, opt-ins)]: ONE steered mini-batch per rank (different rows on each),
              gradient_only, then the all-reduce, against the float64 oracle of every rank's rows

The result goes to <dir>/<name>_rank<r>.pt.  world == 1 runs the same without a process group (the single-rank fused run).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 11


def _settings(O, space, identical):
    from ppo_and_friends_amd.spaces import Box
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=256, hidden_depth=2), critic_kw_args=dict(hidden_size=512, hidden_depth=2))
    if identical:
        pargs["gradient_clip"] = None
    return {"p": (None, sp, sp, space, pargs)}


def _build(rank, t, verbose=False):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Discrete
    dev = torch.device("cuda", 0)
    space = Discrete(4)
    env_rank = 0 if t.get("identical") else rank
    env_gen = lambda: SyntheticFixedLengthEnv(t["E"], t["O"], space, t["T"], dev, reward="uniform", seed=500, rank=env_rank)
    return PPO(env_gen, _settings(t["O"], space, t.get("identical")), device=dev, random_seed=SEED, normalize_obs=False,
               normalize_rewards=False, normalize_values=t["normalize_values"], envs_per_proc=t["E"], ts_per_rollout=t["T"],
               batch_size=t["B"], epochs_per_iter=2, update_mode="fused", save_state=False, verbose=verbose)


def _train(rank, world, t, sc, out_dir):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.utils import mpi_utils
    res = {}
    PPOPolicy.fused_wide_shapes = bool(t.get("shapes"))
    if sc.get("refusal"):
        PPOPolicy.fused_wide_ranks = False
        try:
            _build(rank, t, verbose=True)
            res["refusal"] = ""
        except NotImplementedError as exc:
            res["refusal"] = str(exc)
    PPOPolicy.fused_wide_ranks = True
    ppo = _build(rank, t)
    pol = ppo.policies["p"]
    if t.get("identical"):
        # rank 0's random streams on every rank: shuffles, action draws (the env is rank 0's already)
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        ppo.loader_generator.manual_seed(SEED)
        pol.actor.distribution.rng.seed = SEED
    if t.get("w0_from"):
        # the starting point of the run named there (a job of another rank count draws its initial weights with another
        # number of host threads, and so not to the last bit alike)
        w0 = torch.load(os.path.join(out_dir, t["w0_from"] + "_rank0.pt"), weights_only=False)["train"]["w0"]
        pol.policy_params.copy_(w0.to(pol.device))
    # the all-reduce route's collective, counted where the driver calls it
    bucket, calls = pol.policy_grads.numel(), [0]
    inner = mpi_utils.allreduce_sum_

    def counted(x):
        calls[0] += int(x.numel() == bucket)
        return inner(x)

    mpi_utils.allreduce_sum_ = counted
    res["w0"] = pol.policy_params.detach().cpu().clone()
    descriptions, exchanged = [], []
    for it in range(2 if t.get("drop") else 1):
        ppo.rollout()
        if it == 0:
            res["obs"] = ppo.env.obs_table.cpu().clone()
        ppo.train_on_rollout()
        torch.cuda.synchronize()
        upd, = [f for f in ppo._fused.values() if f is not None]
        descriptions.append(upd.description())
        exchanged.append(None if upd.xchg is None else upd.xchg.status()[0])
        res[f"w_{it}"] = pol.policy_params.detach().cpu().clone()
        if t.get("drop") and it == 0:
            for f in ppo._fused.values():
                if f is not None:
                    f.drop_peer_exchange("test")                      # on the host, every rank: nothing happens on the device
    mpi_utils.allreduce_sum_ = inner
    vs = ppo.value_normalizers["p"].running_stats if t["normalize_values"] else None
    n = t["E"] * t["T"]
    res.update(w=pol.policy_params.detach().cpu().clone(), exp_avg=pol.policy_exp_avg.detach().cpu().clone(),
               exp_avg_sq=pol.policy_exp_avg_sq.detach().cpu().clone(), steps=pol.policy_step_counts.cpu().clone(),
               vn=None if vs is None else torch.from_numpy(np.array([vs.mean, vs.variance, vs.count], dtype=np.float64)),
               stats={k: float(v) for k, v in ppo.status_dict["p"].items() if isinstance(v, (int, float)) and not isinstance(v, bool)},
               descriptions=descriptions, exchanged=exchanged, allreduce_calls=calls[0], graphs=sorted(upd._graphs),
               split=bool(upd.split), tail=upd.tail_reason(), multi=bool(upd.multi), world=upd.world,
               minibatches_per_epoch=n // t["B"] + int(n % t["B"] >= 2), passes=t["B"] > 512,
               guard=ppo._guard_replicas() if world > 1 else True,
               healed=bool(ppo.status_dict["global status"].get("peer exchange disabled", False)))
    return res


MEMBERS = [("adv_0", 8, 5), ("good_0", 10, 3), ("good_1", 10, 3)]      # (agent, observations, classes): mpe_simple_tag's shape


def _train_members(rank, world, t):
    """One iteration of a multi-policy run with TWO wide members -- "adv" (one agent) and "good" (two agents share it) --:
    -> {policy: what _train returns for its one policy}."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.spaces import Box, Discrete
    from ppo_and_friends_amd.utils import mpi_utils
    PPOPolicy.fused_wide_ranks = True
    dev = torch.device("cuda", 0)
    specs = [(a, o, Discrete(n)) for a, o, n in MEMBERS]
    env_gen = lambda: SyntheticMixedAgentsEnv(t["E"], specs, t["T"], dev, reward="uniform", seed=500, rank=rank)
    pargs = dict(actor_kw_args=dict(hidden_size=256, hidden_depth=2), critic_kw_args=dict(hidden_size=512, hidden_depth=2))
    box = lambda o: Box(-np.inf, np.inf, (o,), np.float32)
    settings = {"adv": (None, box(8), box(8), Discrete(5), dict(pargs)), "good": (None, box(10), box(10), Discrete(3), dict(pargs))}
    ppo = PPO(env_gen, settings, policy_mapping_fn=lambda agent: agent.split("_")[0], device=dev, random_seed=SEED,
              normalize_obs=False, normalize_rewards=False, normalize_values=t["normalize_values"], envs_per_proc=t["E"],
              ts_per_rollout=t["T"], batch_size=t["B"], epochs_per_iter=2, update_mode="fused", save_state=False)
    calls, inner = {}, mpi_utils.allreduce_sum_

    def counted(x):
        calls[x.numel()] = calls.get(x.numel(), 0) + 1
        return inner(x)

    mpi_utils.allreduce_sum_ = counted
    w0 = {pid: pol.policy_params.detach().cpu().clone() for pid, pol in ppo.policies.items()}
    ppo.rollout()
    ppo.train_on_rollout()
    torch.cuda.synchronize()
    mpi_utils.allreduce_sum_ = inner
    guard = ppo._guard_replicas()
    healed = bool(ppo.status_dict["global status"].get("peer exchange disabled", False))
    out = {}
    for pid, pol in ppo.policies.items():
        upd, = [f for k, f in ppo._fused.items() if f is not None and k[0] == pid]
        vs = ppo.value_normalizers[pid].running_stats
        n = t["E"] * t["T"] * sum(a.startswith(pid) for a, _, _ in MEMBERS)
        out[pid] = dict(
            w0=w0[pid], w=pol.policy_params.detach().cpu().clone(), exp_avg=pol.policy_exp_avg.detach().cpu().clone(),
            exp_avg_sq=pol.policy_exp_avg_sq.detach().cpu().clone(), steps=pol.policy_step_counts.cpu().clone(),
            vn=torch.from_numpy(np.array([vs.mean, vs.variance, vs.count], dtype=np.float64)),
            stats={k: float(v) for k, v in ppo.status_dict[pid].items() if isinstance(v, (int, float)) and not isinstance(v, bool)},
            descriptions=[upd.description()], exchanged=[None if upd.xchg is None else upd.xchg.status()[0]],
            allreduce_calls=calls.get(pol.policy_grads.numel(), 0), graphs=sorted(upd._graphs), split=bool(upd.split),
            tail=upd.tail_reason(), multi=bool(upd.multi), world=upd.world, bucket=pol.policy_grads.numel(),
            minibatches_per_epoch=n // t["B"] + int(n % t["B"] >= 2), guard=guard, healed=healed,
            fused_step=pol.fused_step_unsupported_reason())
    return out


def _bounds(r64, r32, tables):
    """The per-tensor bound of tests/test_gpu_k12_gradients.py (oracle/k12_oracle.deviations) for one rank's rows, per element."""
    out = np.zeros_like(r64)
    for _, _, off, shape in tables:
        sl = slice(off, off + int(np.prod(shape)))
        a, b = r64[sl], r32[sl]
        out[sl] = np.maximum(1e-5 * np.abs(a) + 1e-5 * float(np.abs(a).max()), 4.0 * float(np.abs(b - a).max()))
    return out


def _grad(rank, world, name, c, flags, mode):
    import torch.distributed as dist
    import test_gpu_k12_gradients as g12
    from oracle import k12_oracle as ko
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.utils import mpi_utils

    class RankSteered(g12.Steered):
        """The steered mini-batch of ONE rank; the value normaliser takes the records of every rank's rows, in rank order."""
        records = None

        def _ref(self, dtype):
            if self.c["norm_values"] and self.records is None:
                r = np.asarray(self.mb.rewards_to_go, dtype=np.float64).reshape(-1)
                every = [None] * world
                dist.all_gather_object(every, (len(r), float(r.mean()), float(((r - r.mean()) ** 2).sum())))
                self.records = every
            return ko.minibatch(self.params, self.actor, self.critic, self.head, self.slices, self.mb, self.consts, self.vn,
                                records=self.records, dtype=dtype)

    for f in ("fused_wide_inputs", "fused_wide_shapes", "fused_wide_heads"):
        setattr(PPOPolicy, f, f in flags)
    PPOPolicy.fused_wide_ranks = True
    s = RankSteered(dict(c, seed=c["seed"] + 1000 * rank))           # (another seed: other rows on every rank)
    pol, B = s.pol, c["B"]
    upd = FusedPolicyUpdate(s.ppo, "p")
    assert upd.wide and upd.split and upd.world == world and upd.xchg is None       # (no K17 route for this pair)
    upd.begin_epoch(s.perm)
    args = upd._args_for(B)
    steps = pol.policy_step_counts.clone()
    upd.gradient_only(args)
    torch.cuda.synchronize()
    pol.policy_step_counts.copy_(steps)
    local = pol.policy_grads.detach().double().cpu().numpy()
    pad = g12._padding(s.tables, local.size)
    res = dict(name=name, description=upd.description(), passes=B > 512, xld=(args.row_pairs, upd.wide_bits))
    res["local_failures"] = ko.failures(local, s.r64["grads"], s.r32["grads"], s.tables) \
        + ko.failures(upd.totals[:8].cpu().numpy(), s.r64["totals"], s.r32["totals"], g12.TOTALS)
    res["local_padding_written"] = bool(local[pad].any())
    g = pol.policy_grads
    mpi_utils.allreduce_sum_(g)                             # the route's exchange, as FusedPolicyUpdate._one issues it
    torch.cuda.synchronize()
    got = g.detach().double().cpu().numpy()
    every = [None] * world
    dist.all_gather_object(every, (s.r64["grads"], _bounds(s.r64["grads"], s.r32["grads"], s.tables), s.r32["grads"]))
    scale = float(args.grad_scale)
    want = sum(e[0] for e in every) * scale
    bound = sum(e[1] for e in every) * scale              # each rank's bound for its rows, added
    err = np.abs(got * scale - want)
    inside = ~pad
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    res.update(grad_scale=scale, elements=int(inside.sum()), padding=int(pad.sum()), bucket=int(got.size),
               padding_written=bool(got[pad].any()), finite=bool(np.isfinite(got).all()),
               worst=float(frac[inside].max()), worst_at=int(np.argmax(np.where(inside, frac, -1.0))),
               outside=int((frac[inside] > 1.0).sum()), differs_from_local=bool((got != local).any()))
    # ---- one WHOLE mini-batch on the route (fwd_bwd, wgrad, all-reduce, Adam's norm pass + Adam) from a preset optimiser
    # state with the clip active, against float64: clip + Adam (oracle/k12_oracle.clip_adam) of the ranks' summed float64
    # gradient times grad_scale.  State and bound as tests/test_gpu_k12_gradients.run_case has them for one rank; the float32
    # twin of the reference sums the ranks' float32 gradients.
    g64, g32 = sum(e[0] for e in every) * scale, sum(e[2] for e in every) * scale
    rng = np.random.default_rng(c["seed"] + 1)             # (the case's seed: the same state on every rank)
    rms = np.sqrt(np.mean(g64 * g64)) + 1e-12
    m0 = np.where(pad, 0.0, 0.5 * g64 + rng.normal(0, 0.1 * rms, g64.size)).astype(np.float32)
    v0 = np.where(pad, 0.0, g64 * g64 * rng.uniform(0.5, 2.0, g64.size) + (0.1 * rms) ** 2).astype(np.float32)
    steps0, na = (6, 9), upd.actor_desc.size
    norms = [np.sqrt((g64[:na] ** 2).sum()), np.sqrt((g64[na:] ** 2).sum())]
    mn = float(np.float32(0.25 * min(norms)))              # both networks clipped
    pol.gradient_clip = mn
    pol.policy_exp_avg.copy_(torch.from_numpy(m0)); pol.policy_exp_avg_sq.copy_(torch.from_numpy(v0))
    pol.policy_step_counts.copy_(torch.tensor(steps0))
    upd.begin_epoch(s.perm)
    upd._one(upd._args_for(B))
    torch.cuda.synchronize()
    lr = float(pol.policy_lr[0])
    want = ko.clip_adam(s.params, g64, m0, v0, steps0, lr, mn, na)
    want32 = ko.clip_adam(s.params, g32, m0, v0, steps0, lr, mn, na, dtype=torch.float32)
    got_p, got_m, got_v = (t.detach().double().cpu().numpy() for t in (pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq))
    res["step_failures"] = ["step " + x for x in ko.failures(got_p - s.params, want[0] - s.params, want32[0] - s.params, s.tables)] \
        + ["m " + x for x in ko.failures(got_m, want[1], want32[1], s.tables)] \
        + ["v " + x for x in ko.failures(got_v, want[2], want32[2], s.tables)]
    res["step_worst"] = max(d[1] for x, a, b in ((got_p - s.params, want[0] - s.params, want32[0] - s.params), (got_m, want[1], want32[1]),
                                                 (got_v, want[2], want32[2])) for d in ko.deviations(x, a, b, s.tables))
    res["steps_after"] = pol.policy_step_counts.cpu().tolist()
    res["clip_coefficients"] = [min(mn / (n + 1e-6), 1.0) for n in norms]
    for f in ("fused_wide_inputs", "fused_wide_shapes", "fused_wide_heads"):
        setattr(PPOPolicy, f, False)
    return res


def rank_main(rank, world, port, out_dir, name, sc):
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0", PPOAF_GRAD_EXCHANGE=sc["mode"], PPOAF_SHARE_DEVICE="1")
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
        import torch.distributed as dist
        from ppo_and_friends_amd.utils import mpi_utils
        mpi_utils.init_process_group_from_env(backend="gloo")
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    FusedPolicyUpdate.graph_chunk = 2                  # (one rank: 5 full mini-batches = a warm-up chunk, a replay, an eager one)
    res = {}
    if sc.get("train"):
        res["train"] = _train(rank, world, sc["train"], sc, out_dir)
    if sc.get("members"):
        res["members"] = _train_members(rank, world, sc["members"])
    res["grads"] = [_grad(rank, world, n, c, flags, sc["mode"]) for n, c, flags in sc.get("grads", ())]
    torch.save(res, os.path.join(out_dir, f"{name}_rank{rank}.pt"))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
