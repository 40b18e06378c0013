"""
TEST INFRASTRUCTURE (see oracle/__init__.py) -- ONE mini-batch of K12 (csrc/ppo_update.hip) restated on torch-CPU in a
chosen dtype (float64 for the reference, float32 for the floor of what f32 arithmetic can reach): forward, loss,
backward, and the per-network clip + Adam of the step that follows.

PINNED by the g12_* fixtures: float64 reproduces the first mini-batch's losses and raw gradients of every feed-forward
fixture (tests/test_k12_oracle.py).  Built from the pinned pieces:

  networks                <- cpu_ppo_loop.make_mlp                     networks/utils.py:120-191
  tanh-Gaussian head      <- ppo_loss_oracle                           networks/distributions.py:441-694
  Categorical / MultiDiscrete / MultiBinary heads: torch.distributions' text written out, probs_to_logits' clamp at
                          float32's eps in EVERY dtype -- the constant of the reference (a float32 program) and of the
                          kernels; held to torch.distributions in float32 by tests/test_head_gates_oracle.py (fixture g16)
                                                                       networks/distributions.py:134-269, :272-438
  value normaliser        <- running_stats_oracle.RunningMeanStd       utils/stats.py:73-94, misc.py:106-111
  surrogate / entropy / KL / critic loss                               ppo.py:2325-2419
  clip + Adam             <- clip_grad_norm_ + torch.optim.Adam         policies/ppo_policy.py:1032-1055

Layouts are K12's (include/ppoaf_hip.h ppoaf_mlp_desc_t, csrc/ppo_update.hip fill_net): per Linear the weight
[out, in] row-major, then the bias, each padded to 4 floats; the Gaussian head's log_std follows the actor's last
bias (padded to 4); the critic's segment follows the actor's.  Padding stays zero in the gradient bucket.
"""
import math
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


EPS32 = float(np.finfo(np.float32).eps)   # probs_to_logits' clamp in the reference (a float32 program) and in the kernels


class GatePlants(NamedTuple):
    """Errors planted in the heads' gradient gates by the sharpness tests (tests/test_head_gates_oracle.py), never set
    otherwise.  Each leaves the forward values alone and lets gradient through where the clean text passes none."""
    gate_open: bool = False                # the discrete clamp to [eps32, 1 - eps32] passes gradient everywhere
    gate_on_chosen_only: bool = False      # the entropy term's gate is dropped, the chosen class's gate is kept
    density_clamp_open: bool = False       # clamp(Normal.log_prob, -100, 100) passes gradient outside
    tanh_clamp_open: bool = False          # the entropy's clamp(1 - tanh(mean)^2, 1e-6) passes gradient below
    floor_open: bool = False               # max(softplus(log_std), min_std) passes gradient to log_std below the floor
    softplus_no_identity: bool = False     # d softplus = sigmoid(log_std) above 20 in place of 1


class _Through(torch.autograd.Function):
    """forward: `y` (the clamped / floored value of x); backward: the gradient handed to x as it is (an open gate)."""

    @staticmethod
    def forward(ctx, x, y):
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _SoftplusSigmoid(torch.autograd.Function):
    """softplus whose derivative is sigmoid(x) on the identity branch (x > 20) as well."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return nn.functional.softplus(x)

    @staticmethod
    def backward(ctx, g):
        return g * torch.sigmoid(ctx.saved_tensors[0])


def _clamp(x, lo, hi, through=False):
    y = torch.clamp(x, lo, hi)
    return _Through.apply(x, y.detach()) if through else y


def _categorical_terms(z, a, plants, note):
    """Categorical(probs=softmax(z)) written out (torch.distributions: probs / probs.sum, probs_to_logits' clamp, log)
    with the clamp at float32's eps in every dtype -> (log-prob [rows], entropy [rows])."""
    p = torch.softmax(z, dim=-1)
    n = p / p.sum(-1, keepdim=True)
    note(n)
    l = torch.log(_clamp(n, EPS32, 1.0 - EPS32, plants.gate_open))
    le = torch.log(_clamp(n, EPS32, 1.0 - EPS32, True)) if plants.gate_on_chosen_only else l
    return l.gather(-1, a.reshape(-1, 1)).squeeze(-1), -(n * le).sum(-1)


def _bernoulli_terms(z, a, plants, note):
    """Bernoulli(probs=sigmoid(z)) written out (probs_to_logits(is_binary=True), log_prob and entropy as binary cross
    entropies with logits; the entropy's target p carries gradient) with the clamp at float32's eps in every dtype."""
    bce = nn.functional.binary_cross_entropy_with_logits
    p = torch.sigmoid(z)
    note(p)
    q = _clamp(p, EPS32, 1.0 - EPS32, plants.gate_open)
    l = torch.log(q) - torch.log1p(-q)
    le = l
    if plants.gate_on_chosen_only:
        qe = _clamp(p, EPS32, 1.0 - EPS32, True)
        le = torch.log(qe) - torch.log1p(-qe)
    return -bce(l, a, reduction="none").sum(-1), bce(le, p, reduction="none").sum(-1)


def _gaussian_planted(mean, log_std, x, min_std, plants, tanh_open):
    """ppo_loss_oracle.gaussian_tanh_logp with a place for each planted gate error."""
    sp = _SoftplusSigmoid.apply(log_std) if plants.softplus_no_identity else nn.functional.softplus(log_std)
    std = torch.max(sp, torch.tensor([min_std], dtype=torch.float32))
    if plants.floor_open:
        std = _Through.apply(sp, std.detach())
    nlp = torch.distributions.Normal(mean, std).log_prob(x)
    nlp = _clamp(nlp, -100, 100, plants.density_clamp_open).sum(dim=-1)
    s_log = torch.log(torch.clamp(1.0 - torch.pow(torch.tanh(x), 2), 1e-6, None))
    if tanh_open:       # the clamped value with the gradient of log(1 - tanh(x)^2) = 2 (log 2 - x - softplus(-2 x)): -2 tanh(x)
        f = 2.0 * (math.log(2.0) - x - nn.functional.softplus(-2.0 * x))
        s_log = s_log.detach() + (f - f.detach())
    return nlp - s_log.sum(dim=-1)


def _head_terms(head, out, log_std, actions, slices, min_std, entropy_slice_scale, plants=GatePlants(), gate_args=None):
    """(log-prob, entropy) per row of the actor output.  The discrete heads are torch.distributions' text written out, so
    that the clamp of probs_to_logits stands at float32's eps in every dtype (tests/test_head_gates_oracle.py holds the
    text to torch.distributions).  gate_args: a dict that receives the arguments of the heads' gradient gates, in the run's
    dtype -- n [rows, classes] (renormalised probabilities; MultiBinary: p), or density / tanh_prime [rows, D] and
    softplus / log_std [D]."""
    args = {} if gate_args is None else gate_args
    note = lambda n: args.setdefault("n", []).append(n.detach())
    if head == "categorical":
        logp, ent = _categorical_terms(out, actions.long().reshape(-1), plants, note)
    elif head == "gaussian":                               # entropy := -log_prob of the mean (distributions.py:694)
        if any(plants):
            logp = _gaussian_planted(out, log_std, actions, min_std, plants, False)
            ent = -_gaussian_planted(out, log_std, out, min_std, plants, plants.tanh_clamp_open)
        else:
            logp = lo.gaussian_tanh_logp(out, log_std, actions, min_std)
            ent = -lo.gaussian_tanh_logp(out, log_std, out, min_std)
        with torch.no_grad():
            sp = nn.functional.softplus(log_std)
            args["softplus"], args["log_std"] = sp, log_std.detach()
            args["density"] = lo.gaussian_dist(out, log_std, min_std).log_prob(actions)
            args["tanh_prime"] = 1.0 - torch.pow(torch.tanh(out), 2)
    elif head == "multi_categorical":                      # one Categorical per slice, summed (:272-438)
        lps, ents, start = [], [], 0
        a = actions.long().reshape(out.shape[0], -1)
        for d, n in enumerate(slices):
            lp, en = _categorical_terms(out[:, start:start + n], a[:, d], plants, note)
            lps.append(lp)
            ents.append(en * entropy_slice_scale.get(d, 1.0))
            start += n
        logp, ent = torch.stack(lps, -1).sum(-1), torch.stack(ents, -1).sum(-1)
    else:                                                  # MultiBinary: independent Bernoullis (:134-196)
        logp, ent = _bernoulli_terms(out, actions.reshape(out.shape).to(out.dtype), plants, note)
    if "n" in args:
        args["n"] = torch.cat(args["n"], dim=-1)
    return logp, ent


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
              dtype=torch.float64, adv_std_ddof=1, clip_wrong_side=False, entropy_slice_scale=None, *,
              gate_plants=GatePlants()):
    """
    One K12 mini-batch from the flat parameter bucket `params` -> dict(totals [8], grads [bucket size] in K12's layout,
    padding zero; values [B] (critic outputs); vn (the normaliser state after the records); gate_args: the arguments of
    the head's gradient gates in the run's dtype, see _head_terms).  `records`: this mini-batch's (n, mean, M2) per rank
    (default: the mini-batch's own rewards-to-go).  The remaining keywords plant errors for the sharpness tests only.
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
    gate_args = {}
    logp, ent = _head_terms(head, out, log_std, T(mb.raw_actions), slices, consts.min_std, entropy_slice_scale or {},
                            gate_plants, gate_args)
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
                logp=logp.detach().double().numpy().reshape(-1), vn=vn,
                gate_args={k: v.double().numpy() for k, v in gate_args.items()})


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
