"""
TEST INFRASTRUCTURE (see oracle/__init__.py) -- whole update EPOCHS of K12 (csrc/ppo_update.hip under
fused_update.FusedPolicyUpdate) restated on torch-CPU in a chosen dtype: a thin loop over pieces that are already pinned,
mini-batch after mini-batch, each from the state the one before it left.  Nothing here restates a network:

  one mini-batch (forward, loss, backward, normaliser)   <- k12_oracle.minibatch
  clip + Adam per network                                <- k12_oracle.clip_adam

What the loop itself restates of the reference:

  mini-batch k is rows perm[k B : (k + 1) B] of the epoch's shuffle, the last one shorter    ppo.py:2181-2184, :2292
  a tail of >= 2 rows is a mini-batch of its own size: advantage moments, loss means and the normaliser's batch
      are taken over the tail's rows                                                         ppo.py:2299-2303, :2325-2333
  a tail of ONE row is integrated into the value normaliser and otherwise skipped (quirk Q9) ppo.py:2299-2306
  the critic's outputs of the rows a mini-batch held go back into the dataset's `values`;
      rows of a skipped tail keep theirs                                                      ppo.py:2340
  both optimisers step once per mini-batch that ran                                           ppo.py:2444
  the epoch's totals are sums over the mini-batches that ran, the count beside them           ppo.py:2438-2485

PINNED by fixture g12_c2_cut (4 mini-batches of 64 rows and a tail of 8): the float32 chain reproduces the first epoch of
cpu_ppo_loop.CpuPPO.train_epoch, mini-batch by mini-batch (tests/test_epoch_oracle.py).  tests/test_gpu_epoch_float64.py
compares the fused driver's epochs with the float64 chain.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import k12_oracle as ko

N_TOTALS = 9                   # the eight of k12_oracle.SC_NAMES, summed over the mini-batches that ran, and their count
KINK_REL, RATIO_GAP, HUBER_GAP = 1e-4, 1e-4, 1e-3     # clearances of a step's rows from the branch edges


class K12Chain(NamedTuple):
    """What an epoch of K12 holds fixed."""
    actor: ko.Net
    critic: ko.Net
    head: str
    slices: tuple
    consts: ko.Consts
    B: int
    lr: float
    max_norm: float


class State(NamedTuple):
    """What an epoch starts from and leaves: the bucket, Adam's moments over it, its step counters (actor, critic), the
    value normaliser (mean, variance, count) and the dataset's `values` column."""
    params: np.ndarray
    m: np.ndarray
    v: np.ndarray
    steps: tuple
    vn: tuple
    values: np.ndarray


def _record(r):
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    return [(len(r), r.mean(), ((r - r.mean()) ** 2).sum())]


def _clearances(chain, params, mb, r, na):
    """Of one float64 step: the rows closer to a branch edge than float32 can be trusted to resolve, and which branches the
    step reached."""
    c = chain.consts
    kink = ko.kinked_rows(chain.actor, params[:na], mb.obs, KINK_REL) | \
        ko.kinked_rows(chain.critic, params[na:], mb.critic_obs, KINK_REL)
    ratio = np.exp(r["logp"] - np.asarray(mb.old_log_probs, dtype=np.float64).reshape(-1))
    lo, hi = 1.0 - c.surr_clip, 1.0 + c.surr_clip
    near_ratio = (np.abs(ratio - lo) < RATIO_GAP) | (np.abs(ratio - hi) < RATIO_GAP)
    d = np.abs(r["values"] - r["rtg"])
    near_huber = (np.abs(d - c.huber_delta) < HUBER_GAP) if c.use_huber else np.zeros(len(d), dtype=bool)
    g = r["grads"]
    norms = (float(np.sqrt((g[:na] ** 2).sum())), float(np.sqrt((g[na:] ** 2).sum())))
    return dict(kink=kink, ratio=near_ratio, huber=near_huber, norms=norms,
                ratio_below=bool((ratio < lo).any()), ratio_inside=bool(((ratio > lo) & (ratio < hi)).any()),
                ratio_above=bool((ratio > hi).any()), huber_linear=bool(c.use_huber and (d > c.huber_delta).any()))


def k12_epochs(chain, data, perms, state, dtype=torch.float64, clearances=False, *, frozen_step=False, stale_vn=False,
               swap_minibatches=False, tail_mean_over_B=False, tail_record_of_full_batch=False, totals_over_n_full=False,
               q9_dropped=False):
    """
    len(perms) epochs of K12 over the dataset `data` (a k12_oracle.Minibatch of all N rows, in the order the shuffles
    index), from `state` -> per epoch dict(state: State after it; totals [9] as end_epoch() returns them; n_done: the
    mini-batches that ran; steps: per mini-batch that ran dict(rows: its dataset rows, totals [8], grads, and with
    `clearances` the float64 step's distances from the branch edges and its gate_args)).
    The keywords behind `*` plant errors for the sharpness test (tests/test_epoch_oracle.py) and are never set otherwise:
      frozen_step               Adam's bias correction keeps the step counters the chain started from
      stale_vn                  mini-batch k integrates its record into the normaliser state mini-batch k - 2 left
      swap_minibatches          mini-batches 1 and 2 of the first epoch change places
      tail_mean_over_B          the tail's loss means (and with them its gradients) are divided by B
      tail_record_of_full_batch the tail's normaliser record is taken over the epoch's last B rows
      totals_over_n_full        the totals leave the tail mini-batch out
      q9_dropped                a one-row tail does not reach the normaliser
    """
    B, c = chain.B, chain.consts
    _, na = ko.tensor_table(chain.actor, chain.head == "gaussian")
    params, m, v = (np.asarray(x, dtype=np.float64).copy() for x in (state.params, state.m, state.v))
    steps, steps0 = [int(s) for s in state.steps], [int(s) for s in state.steps]
    vn, values = tuple(float(x) for x in state.vn), np.asarray(state.values, dtype=np.float64).copy()
    fields = [np.asarray(x) for x in data]
    out = []
    for e, perm in enumerate(perms):
        perm = np.asarray(perm, dtype=np.int64)
        N = len(perm)
        n_full, tail = N // B, N % B
        batches = [perm[k * B:(k + 1) * B] for k in range(n_full)] + ([perm[n_full * B:]] if tail else [])
        if swap_minibatches and e == 0:
            batches[1], batches[2] = batches[2], batches[1]
        totals, info, n_done = np.zeros(N_TOTALS), [], 0
        history = [vn]                                 # the normaliser state each mini-batch of the epoch started from
        for k, rows in enumerate(batches):
            is_tail = k == n_full
            mb = ko.Minibatch(*[x[rows] for x in fields])
            records = _record(mb.rewards_to_go)
            if is_tail and tail_record_of_full_batch:
                records = _record(fields[5][perm[N - B:]])
            vn_in = history[max(k - 1, 0)] if stale_vn else vn
            if len(rows) == 1:                         # Q9: the normaliser sees the row, nothing else does
                if c.normalize_values and not q9_dropped:
                    _, vn = ko.normalised_rtg(mb.rewards_to_go, vn_in, records, dtype)
                continue
            r = ko.minibatch(params, chain.actor, chain.critic, chain.head, chain.slices, mb, c, vn_in, records, dtype=dtype)
            step = dict(rows=rows, totals=r["totals"], grads=r["grads"])
            if clearances:
                step.update(_clearances(chain, params, mb, r, na), gate_args=r["gate_args"],
                            raw_actions=np.asarray(mb.raw_actions))
            info.append(step)
            if c.normalize_values:
                vn = r["vn"]
            history.append(vn)
            values[rows] = r["values"]
            grads, t8 = r["grads"], r["totals"].copy()
            if is_tail and tail_mean_over_B:
                grads = grads * (len(rows) / B)
                t8[:5] *= len(rows) / B
            if not (is_tail and totals_over_n_full):
                totals[:8] += t8
                totals[8] += 1.0
            params, m, v = ko.clip_adam(params, grads, m, v, steps0 if frozen_step else steps, chain.lr, chain.max_norm, na,
                                        dtype=dtype)
            steps = [s + 1 for s in steps]
            n_done += 1
        out.append(dict(state=State(params.copy(), m.copy(), v.copy(), tuple(steps), vn, values.copy()), totals=totals,
                        n_done=n_done, steps=info))
    return out


PLANTS = ("frozen_step", "stale_vn", "swap_minibatches", "tail_mean_over_B", "tail_record_of_full_batch",
          "totals_over_n_full", "q9_dropped")


def compared(chain, start, epoch):
    """The tensors of one epoch that the rule of k12_oracle.deviations is applied to -> {name: (array, tables or None)}:
    the parameter step over the epoch, m and v per parameter tensor; the normaliser's mean and variance; the nine totals
    and the whole `values` column, each as one tensor."""
    tables, _ = ko.bucket_tables(chain.actor, chain.critic, chain.head)
    s = epoch["state"]
    one = lambda name, n: [("", name, 0, (n,))]
    return {"step": (s.params - np.asarray(start.params, dtype=np.float64), tables), "m": (s.m, tables), "v": (s.v, tables),
            "normaliser": (np.array(s.vn[:2]), [("", "mean", 0, (1,)), ("", "variance", 1, (1,))]),
            "totals": (epoch["totals"], one("totals", N_TOTALS)), "values": (s.values, one("values", len(s.values)))}
