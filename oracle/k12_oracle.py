"""
TEST INFRASTRUCTURE (see oracle/__init__.py) -- ONE mini-batch of K12 (csrc/ppo_update.hip) restated on torch-CPU in a
chosen dtype (float64 for the reference, float32 for the floor of what f32 arithmetic can reach): forward, loss,
backward, and the per-network clip + Adam of the step that follows.

PINNED by the g12_* fixtures: float64 reproduces the first mini-batch's losses and raw gradients of every feed-forward
fixture (tests/test_k12_oracle.py).  Built from the pinned pieces:

  networks                <- cpu_ppo_loop.make_mlp                     networks/utils.py:120-191
  categorical / tanh-Gaussian heads <- ppo_loss_oracle                 networks/distributions.py:199-269, :441-694
  MultiDiscrete / MultiBinary heads  (torch.distributions, like the product's networks/distributions.py; fixture g16)
                                                                       networks/distributions.py:134-196, :272-438
  value normaliser        <- running_stats_oracle.RunningMeanStd       utils/stats.py:73-94, misc.py:106-111
  surrogate / entropy / KL / critic loss                               ppo.py:2325-2419
  clip + Adam             <- clip_grad_norm_ + torch.optim.Adam         policies/ppo_policy.py:1032-1055

Layouts are K12's (include/ppoaf_hip.h ppoaf_mlp_desc_t, csrc/ppo_update.hip fill_net): per Linear the weight
[out, in] row-major, then the bias, each padded to 4 floats; the Gaussian head's log_std follows the actor's last
bias (padded to 4); the critic's segment follows the actor's.  Padding stays zero in the gradient bucket.
"""
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import cpu_ppo_loop
from . import ppo_loss_oracle as lo
from .running_stats_oracle import RunningMeanStd

HEADS = ("categorical", "gaussian", "multi_categorical", "bernoulli")          # K.HEAD_* order
ACTIVATIONS = ("relu", "leaky_relu", "tanh")                                     # K.ACT_* order
SC_NAMES = ("surr", "actor", "critic", "entropy", "kl", "adv_mean", "adv_std", "bad")   # K.SC_* order


class Net(NamedTuple):
    in_dim: int
    hidden: int
    depth: int            # hidden layers; depth + 1 Linear layers
    out_dim: int
    activation: str


def _pad4(n):
    return (n + 3) // 4 * 4


def tensor_table(net, log_std=False):
    """[(name, offset, shape)] of one network's segment in K12's layout, and the segment's size."""
    out, off = [], 0
    for l in range(net.depth + 1):
        i = net.in_dim if l == 0 else net.hidden
        o = net.out_dim if l == net.depth else net.hidden
        out.append((f"{l}.weight", off, (o, i)))
        off += _pad4(o * i)
        out.append((f"{l}.bias", off, (o,)))
        off += _pad4(o)
    if log_std:
        out.append(("log_std", off, (net.out_dim,)))
        off += _pad4(net.out_dim)
    return out, off


def bucket_tables(actor, critic, head):
    """[(tag, name, offset, shape)] over the whole bucket, and its size."""
    ta, na = tensor_table(actor, head == "gaussian")
    tc, nc = tensor_table(critic)
    return [("actor", n, o, s) for n, o, s in ta] + [("critic", n, na + o, s) for n, o, s in tc], na + nc


def _activation(name):
    return {"relu": nn.ReLU(), "leaky_relu": nn.LeakyReLU(0.01), "tanh": nn.Tanh()}[name]


def _module(net, seg, dtype):
    """cpu_ppo_loop.make_mlp holding the segment's weights, in `dtype`."""
    m = cpu_ppo_loop.make_mlp(net.in_dim, net.out_dim, net.hidden, net.depth, activation=_activation(net.activation))
    m = m.to(dtype)
    lin = [x for x in m.modules() if isinstance(x, nn.Linear)]
    table, _ = tensor_table(net)
    with torch.no_grad():
        for (name, off, shape), p in zip(table, [p for x in lin for p in (x.weight, x.bias)]):
            p.copy_(torch.as_tensor(seg[off:off + int(np.prod(shape))].reshape(shape), dtype=dtype))
    return m, lin


def pre_activations(net, seg, x, dtype=torch.float64):
    """The hidden layers' pre-activations of rows x ([rows, in_dim]) -> list of [rows, hidden] arrays (kink checks)."""
    m, lin = _module(net, seg, dtype)
    act = _activation(net.activation)
    h, out = torch.as_tensor(np.asarray(x), dtype=dtype), []
    with torch.no_grad():
        for layer in lin[:-1]:
            z = layer(h)
            out.append(z.numpy())
            h = act(z)
    return out


def _head_terms(head, out, log_std, actions, slices, min_std, entropy_slice_scale):
    """(log-prob, entropy) per row of the actor output."""
    if head == "categorical":
        logp, ent, _ = lo.categorical_logp_entropy(out, actions.long().reshape(-1))
        return logp, ent
    if head == "gaussian":                                 # entropy := -log_prob of the mean (distributions.py:694)
        return (lo.gaussian_tanh_logp(out, log_std, actions, min_std),
                -lo.gaussian_tanh_logp(out, log_std, out, min_std))
    if head == "multi_categorical":                        # one Categorical per slice, summed (:272-438)
        lps, ents, start = [], [], 0
        a = actions.long().reshape(out.shape[0], -1)
        for d, n in enumerate(slices):
            dist = torch.distributions.Categorical(probs=torch.softmax(out[:, start:start + n], dim=-1))
            lps.append(dist.log_prob(a[:, d]))
            ents.append(dist.entropy() * entropy_slice_scale.get(d, 1.0))
            start += n
        return torch.stack(lps, -1).sum(-1), torch.stack(ents, -1).sum(-1)
    dist = torch.distributions.Bernoulli(probs=torch.sigmoid(out), validate_args=False)     # (:134-196)
    return dist.log_prob(actions.reshape(out.shape).to(out.dtype)).sum(-1), dist.entropy().sum(-1)


def normalised_rtg(rtg, vn_state, records, dtype=torch.float64):
    """The value normaliser after this mini-batch's records (one (n, mean, M2) per rank, merged), and the normalised
    rewards-to-go (ppo.py:2299-2303 with the rank-gathered data of utils/stats.py:47-50)."""
    rs = RunningMeanStd()
    rs.mean, rs.variance, rs.count = np.float64(vn_state[0]), np.float64(vn_state[1]), float(vn_state[2])
    n = mean = M2 = 0.0
    for rn, rm, rq in records:                          # Chan merge of the ranks' records
        if rn <= 0:
            continue
        d = rm - mean
        tot = n + rn
        mean += d * rn / tot
        M2 += rq + d * d * n * rn / tot
        n = tot
    rs.integrate(np.float64(mean), np.float64(M2 / n), n)
    r = torch.as_tensor(np.asarray(rtg), dtype=dtype)
    m, v = torch.tensor(rs.mean, dtype=dtype), torch.tensor(rs.variance, dtype=dtype)
    return (r - m) / torch.sqrt(v + 1e-8), (float(rs.mean), float(rs.variance), float(rs.count))


def losses(logp, old_logp, adv, ent, values, rtg, normalize_adv=True, surr_clip=0.2, entropy_weight=0.01,
           kl_loss_weight=0.0, use_huber=False, huber_delta=10.0, adv_std_ddof=1, clip_wrong_side=False):
    """
    (actor loss, critic loss, the eight totals) of ppo.py:2325-2419 as K12 reports them (csrc/ppo_loss.hip: the entropy
    mean is reported whatever its weight; adv mean / std are 0 / 1 without normalisation).
    adv_std_ddof / clip_wrong_side: planted errors of the sharpness tests (tests/test_k12_oracle.py), never set otherwise.
    """
    a, mean, std = adv, torch.zeros((), dtype=adv.dtype), torch.ones((), dtype=adv.dtype)
    if normalize_adv:                                   # :2325-2333 (torch.std: Bessel-corrected)
        mean, std = adv.mean(), adv.std(correction=adv_std_ddof)
        a = (adv - mean) / (std + 1e-8)
    ratios = torch.exp(logp - old_logp)                 # :2352
    surr1 = ratios * a
    surr2 = torch.clamp(ratios, 1 - surr_clip, 1 + surr_clip) * a
    surr = (-(torch.max(surr1, surr2) if clip_wrong_side else torch.min(surr1, surr2))).mean()   # :2392
    kl = (old_logp - logp).mean()                       # :2358 (a python float there: no gradient)
    actor = surr
    if entropy_weight != 0.0:                           # :2395-2398
        actor = actor - entropy_weight * ent.mean()
    if kl_loss_weight > 0.0:                            # :2403-2405
        actor = actor + kl_loss_weight * kl.detach()
    d = values - rtg
    if use_huber:                                       # :2416-2419 (nn.HuberLoss(delta))
        critic = torch.where(d.abs() < huber_delta, 0.5 * d * d, huber_delta * (d.abs() - 0.5 * huber_delta)).mean()
    else:
        critic = (d * d).mean()
    bad = bool(torch.isnan(ratios).any() or torch.isinf(ratios).any())
    totals = [surr.item(), actor.item(), critic.item(), ent.mean().item(), kl.item(), mean.item(), std.item(), float(bad)]
    return actor, critic, np.array(totals, dtype=np.float64)


class Minibatch(NamedTuple):
    obs: np.ndarray            # [B, actor in_dim]
    critic_obs: np.ndarray     # [B, critic in_dim]
    raw_actions: np.ndarray    # [B] class / [B, D] Gaussian pre-tanh, slice classes or bits
    old_log_probs: np.ndarray  # [B]
    advantages: np.ndarray     # [B]
    rewards_to_go: np.ndarray  # [B]


class Consts(NamedTuple):
    normalize_adv: bool = True
    normalize_values: bool = True
    use_huber: bool = False
    huber_delta: float = 10.0
    surr_clip: float = 0.2
    entropy_weight: float = 0.01
    kl_loss_weight: float = 0.0
    min_std: float = 0.01


def minibatch(params, actor, critic, head, slices, mb, consts, vn_state=(0.0, 1.0, 1e-4), records=None,
              dtype=torch.float64, adv_std_ddof=1, clip_wrong_side=False, entropy_slice_scale=None):
    """
    One K12 mini-batch from the flat parameter bucket `params` -> dict(totals [8], grads [bucket size] in K12's layout,
    padding zero; values [B] (critic outputs); vn (the normaliser state after the records)).  `records`: this
    mini-batch's (n, mean, M2) per rank (default: the mini-batch's own rewards-to-go).  The remaining keywords plant
    errors for the sharpness tests only.
    """
    params = np.asarray(params, dtype=np.float64)
    _, na = tensor_table(actor, head == "gaussian")
    am, alin = _module(actor, params[:na], dtype)
    cm, clin = _module(critic, params[na:], dtype)
    aparams = [p for x in alin for p in (x.weight, x.bias)]
    log_std = None
    if head == "gaussian":
        t, _ = tensor_table(actor, True)
        off = t[-1][1]
        log_std = nn.Parameter(torch.as_tensor(params[off:off + actor.out_dim], dtype=dtype))
        aparams.append(log_std)
    cparams = [p for x in clin for p in (x.weight, x.bias)]
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    out = am(T(mb.obs))
    values = cm(T(mb.critic_obs)).reshape(-1)
    logp, ent = _head_terms(head, out, log_std, T(mb.raw_actions), slices, consts.min_std, entropy_slice_scale or {})
    rtg = T(mb.rewards_to_go).reshape(-1)
    vn = None
    if consts.normalize_values:
        r = np.asarray(mb.rewards_to_go, dtype=np.float64).reshape(-1)
        if records is None:
            records = [(len(r), r.mean(), ((r - r.mean()) ** 2).sum())]
        rtg, vn = normalised_rtg(mb.rewards_to_go, vn_state, records, dtype)
        rtg = rtg.reshape(-1)
    a_loss, c_loss, totals = losses(logp.reshape(-1), T(mb.old_log_probs).reshape(-1), T(mb.advantages).reshape(-1),
                                    ent.reshape(-1), values, rtg, consts.normalize_adv, consts.surr_clip,
                                    consts.entropy_weight, consts.kl_loss_weight, consts.use_huber, consts.huber_delta,
                                    adv_std_ddof, clip_wrong_side)
    ga = torch.autograd.grad(a_loss, aparams)
    gc = torch.autograd.grad(c_loss, cparams)
    tables, size = bucket_tables(actor, critic, head)
    grads = np.zeros(size, dtype=np.float64)
    for (tag, name, off, shape), g in zip(tables, list(ga) + list(gc)):
        grads[off:off + g.numel()] = g.detach().double().numpy().reshape(-1)
    return dict(totals=totals, grads=grads, values=values.detach().double().numpy(), rtg=rtg.detach().double().numpy(),
                logp=logp.detach().double().numpy().reshape(-1), vn=vn)


def kinked_rows(net, seg, x, rel=1e-4):
    """Rows of x with a ReLU / LeakyReLU pre-activation within rel x its row's scale (max |z| of that layer) of zero:
    there float32 may take the other side of the kink.  Tanh has none."""
    bad = np.zeros(len(x), dtype=bool)
    if net.activation == "tanh":
        return bad
    for z in pre_activations(net, seg, x):
        bad |= (np.abs(z) < rel * np.abs(z).max(axis=1, keepdims=True)).any(axis=1)
    return bad


def steered_old_log_probs(logp64, rng, surr_clip=0.2, lo=0.5, hi=1.6, gap=1e-3):
    """float32 old log-probs whose ratios exp(logp - old) spread over [lo, hi] with none within `gap` of 1 -/+ surr_clip
    (a ratio drawn too close is drawn again)."""
    old = np.empty(len(logp64), dtype=np.float32)
    for i, lp in enumerate(np.asarray(logp64, dtype=np.float64)):
        while True:
            o = np.float32(lp - np.log(rng.uniform(lo, hi)))
            r = np.exp(lp - np.float64(o))
            if abs(r - (1 - surr_clip)) >= gap and abs(r - (1 + surr_clip)) >= gap:
                break
        old[i] = o
    return old


def clip_adam(params, grads, exp_avg, exp_avg_sq, step, lr, max_norm, n_actor, beta1=0.9, beta2=0.999, eps=1e-5,
              dtype=torch.float64):
    """
    One optimiser step of both networks from a NON-zero state: Adam's step counter `step` ((actor, critic), before the
    step), exp_avg / exp_avg_sq over the bucket.  Each network is clipped by its own norm with the coefficient
    min(max_norm / (norm + 1e-6), 1) (nn.utils.clip_grad_norm_), then torch.optim.Adam's update (ppo_policy.py:1032-1055).
    -> (params, exp_avg, exp_avg_sq) after the step.
    """
    T = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dtype)
    p, g, m, v = T(params), T(grads), T(exp_avg), T(exp_avg_sq)
    outs = []
    for w, sl in enumerate((slice(0, n_actor), slice(n_actor, p.numel()))):
        gw = g[sl]
        if max_norm:
            norm = torch.sqrt((gw * gw).sum())
            gw = gw * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        t = int(step[w]) + 1
        mw = beta1 * m[sl] + (1 - beta1) * gw
        vw = beta2 * v[sl] + (1 - beta2) * gw * gw
        bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
        pw = p[sl] - (lr / bc1) * (mw / (torch.sqrt(vw) / np.sqrt(bc2) + eps))
        outs.append((pw, mw, vw))
    return tuple(torch.cat([o[k] for o in outs]).double().numpy() for k in range(3))


def deviations(got, want64, want32, tables):
    """
    Per parameter tensor (and per total): the worst |got - want64| against its bound
    1e-5 |want64| + 1e-5 max|want64 over the tensor|, raised to 4 max|want32 - want64| where float32 arithmetic itself
    cannot do better.  -> [(tensor, worst fraction of the bound, floor used)]; a fraction > 1 is a failure.
    `tables`: [(tag, name, offset, shape)] (bucket_tables), or None for a vector compared element by element.
    """
    got, w64, w32 = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want64, want32))
    if tables is None:
        tables = [("", SC_NAMES[i] if len(w64) == 8 else str(i), i, (1,)) for i in range(len(w64))]
    out = []
    for tag, name, off, shape in tables:
        sl = slice(off, off + int(np.prod(shape)))
        g, a, b = got[sl], w64[sl], w32[sl]
        floor = 4.0 * float(np.abs(b - a).max())
        bound = np.maximum(1e-5 * np.abs(a) + 1e-5 * float(np.abs(a).max()), floor)
        err = np.abs(g - a)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        if not np.all(np.isfinite(g)):
            frac = np.full_like(frac, np.inf)
        out.append((f"{tag}.{name}" if tag else name, float(frac.max()), floor))
    return out


def failures(got, want64, want32, tables):
    """The tensors of `deviations` outside their bound, as readable lines (empty: accepted)."""
    return [f"{n}: {f:.3g} x bound (float32 floor {fl:.3g})" for n, f, fl in deviations(got, want64, want32, tables)
            if not f <= 1.0]
