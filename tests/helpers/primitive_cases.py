"""
The standalone kernels K2-K11 (csrc/ppo_loss.hip, gather.hip, moments.hip, ppo_update.hip: minibatch_moments,
distributions.hip, icm.hip, mat_attention.hip, adam.hip) restated in a chosen dtype, and the cases
tests/test_gpu_primitives_float64.py runs them at.  One function per operation: the float64 run is the reference, the
float32 run of the same text the floor of the bound (eval_kernels.k12_bound).  tests/test_primitives_oracle.py holds the
restatements to oracle/ppo_loss_oracle.py, torch.optim.Adam and fixture g8 and asserts, on the reference alone, every
condition a case relies on.

Constants the reference takes from float32 are those float32 values in the float64 run too (c32): Categorical's eps32
clamp, the literals 1e-8 / 1e-6 / 1e-5, min_std, the learning rate; softplus' threshold 20, Huber's delta 10 and the +-100
clamp are exact in both.

Float64 outputs (the (n, mean, M2) records, `count`, the squared gradient norm) have a derived bound, f64_sum_bound: two
float64 sums of the same n terms in different orders each lie within (n - 1) u sum|term| of the exact sum (u = 2^-53,
first order: no partial sum exceeds sum|term|), so within 2 n 2^-53 sum|term| of each other, n 2^-53 sum|term| for
terms of one sign (M2, the norm, data whose mean dominates its spread), whose partial sums grow linearly.  The bound is 8 times the latter:
M2's terms are (x - mean)^2 with a mean that itself carries such an error d, which moves M2 by 2 d sum(x - mean) + n d^2,
zero to first order; the factor covers it and the rounding of the terms themselves.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(os.path.dirname(_HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import eval_kernels as ek  # noqa: E402
import head_draws as hd  # noqa: E402
import philox  # noqa: E402
from oracle import k12_oracle as ko  # noqa: E402
from oracle.running_stats_oracle import RunningMeanStd  # noqa: E402

F32 = np.float32
EPS32 = hd.EPS32
HALF_LOG_2PI = 0.91893853320467274178
SEED, OFFSET = 0x1234_5678_9ABC, 2 ** 32 - 7          # a seed above 32 bits; the low counter word wraps in the launch


def c32(x):
    """The value of a float32 literal, as a python float."""
    return float(np.float32(x))


def _td(dtype):
    return dtype if isinstance(dtype, torch.dtype) else {np.float64: torch.float64, np.float32: torch.float32}[dtype]


def _T(x, dtype):
    return torch.tensor(np.asarray(x, np.float64), dtype=_td(dtype))


def _np(t):
    return t.detach().double().numpy()


# ------------------------------------------------------------------------------------------------------------ bounds
def frac(got, x64, x32):
    """Worst |got - x64| over eval_kernels.k12_bound(x64, x32) of one tensor (inf for a non-finite `got`; where the
    bound is zero the value must be exact)."""
    got, x64 = np.asarray(got, np.float64).reshape(-1), np.asarray(x64, np.float64).reshape(-1)
    if got.size == 0:
        return 0.0
    return frac_abs(got, x64, ek.k12_bound(x64, np.asarray(x32, np.float64).reshape(-1)))


def frac_abs(got, want, bound):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64).reshape(-1), want.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(f.max()) if f.size else 0.0


def f64_sum_bound(n, abs_sum):
    """8 n 2^-53 sum|term| (the module docstring derives it)."""
    return 8.0 * n * 2.0 ** -53 * np.asarray(abs_sum, np.float64)


# ------------------------------------------------------------------------------------------------------------ K2 + K3
LOSS_DEFAULTS = dict(normalize=True, clip=0.2, ent_w=0.01, kl=0.0, huber=False, delta=10.0, adv_mean=0.0, entropy=True,
                     ratio_one=False, null=None, bad=None, seed=11)
LOSS_CASES = [dict(name=f"B{B}", B=B, huber=B in (63, 1024, 3000), seed=B) for B in (2, 63, 64, 65, 1023, 1024, 1025, 3000)] + [
    dict(name="B1_raw", B=1, normalize=False, huber=True),
    dict(name="adv_1e3", B=65, adv_mean=1e3),
    dict(name="no_entropy_kl", B=64, ent_w=0.0, entropy=False, kl=0.3, huber=True),
    dict(name="clip0_ratio_one", B=12, clip=0.0, ratio_one=True),
    dict(name="null_d_logp", B=65, null="d_logp"),
    dict(name="null_d_entropy", B=65, null="d_entropy", huber=True),
    dict(name="null_d_values", B=65, null="d_values"),
    dict(name="inf_ratio", B=65, bad="inf"),
    dict(name="nan_logp", B=65, bad="nan"),
]
INSIDE, BELOW, ABOVE, EDGE_LO, EDGE_HI, ONE = range(6)


def loss_case(c):
    return {**LOSS_DEFAULTS, **c}


def loss_inputs(c):
    """float32 streams of one mini-batch.  Row i is steered to ratio class i % 3 (inside the clip, below 1 - clip, above
    1 + clip) with the sign of its advantage (i // 3) % 2; rows 6 / 7 (B >= 8) sit on the lower / upper clip edge, within
    the device's expf rounding of it, with the sign of advantage for which loss and gradient are continuous across the
    edge; ratio_one: every ratio is exactly 1 (old == cur), which with clip 0 is both edges at once.  |value - rtg|: rows
    0 / 1 are 15 above / below (Huber's linear side), rows 2 / 3 exactly +10 / -10, the rest N(0, 3)."""
    c = loss_case(c)
    B, rng = c["B"], np.random.default_rng(c["seed"])
    i = np.arange(B)
    cur = (-np.abs(rng.standard_normal(B)) - 0.1).astype(F32)
    cls, sign = i % 3, np.where((i // 3) % 2 == 0, 1.0, -1.0)
    target = np.where(cls == INSIDE, rng.uniform(0.85, 1.15, B), np.where(cls == BELOW, rng.uniform(0.5, 0.75, B), rng.uniform(1.25, 1.6, B)))
    z = sign * (0.2 + np.abs(rng.standard_normal(B)))
    if B >= 8:
        cls[6], cls[7], z[6], z[7] = EDGE_LO, EDGE_HI, 2.0, -2.0
        target[6], target[7] = float(F32(1) - F32(c["clip"])), float(F32(1) + F32(c["clip"]))
    old = (cur.astype(np.float64) - np.log(target)).astype(F32)
    if c["ratio_one"]:
        cls[:], old = ONE, cur.copy()
    adv = (c["adv_mean"] + z).astype(F32)
    rtg = (2.0 * rng.standard_normal(B)).astype(F32)
    diff = 3.0 * rng.standard_normal(B)
    diff[:2] = (15.0, -15.0)[:min(B, 2)]
    values = (rtg + diff).astype(F32)
    for r, v in ((2, 10.0), (3, -10.0)):
        if B > r:
            rtg[r], values[r] = 0.0, v
    ent = rng.uniform(0.2, 1.5, B).astype(F32) if c["entropy"] else None
    if c["bad"] == "inf":
        cur[1], old[1] = 0.0, -200.0
    if c["bad"] == "nan":
        cur[1] = np.nan
    return dict(cur=cur, old=old, adv=adv, ent=ent, values=values, rtg=rtg, cls=cls)


def loss_ref(inp, c, dtype, **planted):
    """oracle/k12_oracle.losses in `dtype` with autograd: dict(scalars [8], d_logp, d_entropy, d_values).  planted: that
    function's planted errors, for the sharpness test only."""
    c = loss_case(c)
    lp, val = _T(inp["cur"], dtype).requires_grad_(), _T(inp["values"], dtype).requires_grad_()
    ent = _T(np.zeros(c["B"]) if inp["ent"] is None else inp["ent"], dtype).requires_grad_()
    actor, critic, totals = ko.losses(lp, _T(inp["old"], dtype), _T(inp["adv"], dtype), ent, val, _T(inp["rtg"], dtype),
                                      c["normalize"], c["clip"], c["ent_w"], c["kl"], c["huber"], c["delta"], **planted)
    (actor + critic).backward()
    g = lambda t: np.zeros(c["B"]) if t.grad is None else _np(t.grad)
    return dict(scalars=totals, d_logp=g(lp), d_entropy=g(ent), d_values=g(val))


def loss_rows(inp, c):
    """What the float64 reference makes of the rows: (ratio, normalised advantage, |value - rtg|)."""
    c = loss_case(c)
    adv = inp["adv"].astype(np.float64)
    if c["normalize"]:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    return np.exp(inp["cur"].astype(np.float64) - inp["old"]), adv, np.abs(inp["values"].astype(np.float64) - inp["rtg"])


# ------------------------------------------------------------------------------------------------------------ K4
def gather_ref(src, dst0, perm, row_map, n_rows):
    """dst[b] = src[row_map[perm[b]]]; a perm entry outside [0, n_rows) leaves its row as it was."""
    dst = dst0.copy()
    for b, r in enumerate(perm):
        if 0 <= r < n_rows:
            dst[b] = src[row_map[r] if row_map is not None else r]
    return dst


def scatter_ref(src, dst0, perm, row_map, n_rows):
    dst = dst0.copy()
    for b, r in enumerate(perm):
        if 0 <= r < n_rows:
            dst[row_map[r] if row_map is not None else r] = src[b]
    return dst


# ------------------------------------------------------------------------------------------------------------ K5
MOMENT_SHAPES = [(1, 1), (63, 2), (64, 17), (65, 1), (1025, 17), (5000, 2), (3, 1025), (1025, 1)]      # (n, W)


def moments_data(n, W, seed=5):
    return (1e4 + np.random.default_rng(seed + n + W).standard_normal((n, W))).astype(F32)


def moments_ref(x):
    """(record [1 + 2 W] float64: n, the column means, the columns' M2; its bound per entry, f64_sum_bound)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mean = x.mean(0)
    M2 = ((x - mean) ** 2).sum(0)
    rec = np.concatenate([[float(n)], mean, M2])
    bound = np.concatenate([[0.0], f64_sum_bound(n, np.abs(x).sum(0)) / n, f64_sum_bound(n, M2)])
    return rec, bound


def minibatch_moments_ref(data, perm, row_map, B):
    """[ceil(n / B), 3] records of data[row_map[perm]] per mini-batch, and their bounds."""
    rows = np.asarray(perm) if row_map is None else np.asarray(row_map)[perm]
    x = np.asarray(data, np.float64)[rows]
    recs, bounds = [], []
    for k in range(0, len(x), B):
        r, b = moments_ref(x[k:k + B, None])
        recs.append(r); bounds.append(b)
    return np.array(recs), np.array(bounds)


INTEGRATE_CASES = [dict(name="R1", R=1, W=1, empty=(), count=1e-4), dict(name="R3_one_empty", R=3, W=5, empty=(1,), count=1e-4),
                   dict(name="R4_one_empty_W300", R=4, W=300, empty=(0,), count=1e7), dict(name="all_empty", R=3, W=5, empty=(0, 1, 2), count=1e7),
                   dict(name="R4_W300_fresh", R=4, W=300, empty=(3,), count=1e-4)]


def integrate_inputs(c):
    rng = np.random.default_rng(c["R"] * 100 + c["W"])
    W = c["W"]
    recs = np.zeros((c["R"], 1 + 2 * W))
    for r in range(c["R"]):
        n = 0 if r in c["empty"] else int(rng.integers(3, 400))
        recs[r, 0] = n
        recs[r, 1:1 + W] = 3.0 * rng.standard_normal(W) + r               # an empty record's moments are junk to be skipped
        recs[r, 1 + W:] = rng.uniform(0.5, 2.0, W) * max(n, 1)
    fresh = c["count"] < 1.0
    mean = np.zeros(W, F32) if fresh else rng.standard_normal(W).astype(F32)
    var = np.ones(W, F32) if fresh else rng.uniform(0.5, 2.0, W).astype(F32)
    return recs, mean, var, float(c["count"])


def integrate_ref(recs, mean, var, count, dtype):
    """Chan's merge of the records in float64 (they are float64), then oracle/running_stats_oracle's integrate step on a
    state held in `dtype` -> (mean, var, count).  No record with n > 0: the state as it was."""
    W = len(mean)
    n, m, M2 = 0.0, np.zeros(W), np.zeros(W)
    for r in recs:
        if r[0] <= 0:
            continue
        d, tot = r[1:1 + W] - m, n + r[0]
        m = m + d * (r[0] / tot)
        M2 = M2 + r[1 + W:] + d * d * n * r[0] / tot
        n = tot
    rs = RunningMeanStd()
    rs.mean, rs.variance, rs.count = mean.astype(dtype), var.astype(dtype), float(count)
    if n > 0:
        rs.integrate(m.astype(dtype), (M2 / n).astype(dtype), float(n))
    return np.asarray(rs.mean), np.asarray(rs.variance), rs.count


NORMALIZE_CASES = [dict(name="W1", n=1000, W=1, clip=None), dict(name="W5_clip", n=333, W=5, clip=(-1.5, 2.0)),
                   dict(name="grid_stride", n=105000, W=5, clip=None), dict(name="W1_clip", n=257, W=1, clip=(-1.0, 0.5)),
                   dict(name="W5_var0", n=64, W=5, clip=None, var0=True)]


def normalize_inputs(c):
    rng = np.random.default_rng(c["n"] + c["W"])
    mean = (2.0 * rng.standard_normal(c["W"])).astype(F32)
    var = rng.uniform(0.3, 4.0, c["W"]).astype(F32)
    if c.get("var0"):
        var[0] = 0.0
    x = (mean + 2.0 * rng.standard_normal((c["n"], c["W"]))).astype(F32)
    return x, mean, var


def normalize_ref(x, mean, var, clip, dtype, eps=1e-8):
    y = (x.astype(dtype) - mean.astype(dtype)) / np.sqrt(var.astype(dtype) + dtype(c32(eps)))
    return y if clip is None else np.clip(y, dtype(clip[0]), dtype(clip[1]))


def denormalize_ref(x, mean, var, dtype, eps=1e-8):
    return mean.astype(dtype) + x.astype(dtype) * np.sqrt(var.astype(dtype) + dtype(c32(eps)))


MB_MOMENT_CASES = [(1, 3, False), (255, 510, True), (255, 509, False), (255, 256, False), (256, 767, True), (256, 512, False), (256, 257, True),
                   (257, 258, True), (257, 770, False), (257, 514, True)]                # (B, n_perm, row_map given)


# ------------------------------------------------------------------------------------------------------------ K6 categorical
CAT_EVAL_SHAPES = [(1, 257), (2, 1), (2, 256), (17, 255), (63, 256), (64, 257), (64, 1)]       # (K, n)
ORDINARY, HOT, EQUAL, SHIFTED = 0, 1, 2, 3


def categorical_inputs(K, n, seed=3):
    """Rows by i % 5: ordinary N(0, 2) logits (0 and 4), one logit 40 above the rest, all equal, a common offset of 1e4.
    Actions: class 0, class K - 1 and a random class in turn; a HOT row's action is its hot class or the class after it."""
    rng = np.random.default_rng(seed + 1000 * K + n)
    kind = np.arange(n) % 5 % 4
    z = 2.0 * rng.standard_normal((n, K))
    hot = rng.integers(0, K, n)
    for i in range(n):
        if kind[i] == HOT:
            z[i] *= 0.25
            z[i, hot[i]] += 40.0
        elif kind[i] == EQUAL:
            z[i] = 0.7
        elif kind[i] == SHIFTED:
            z[i] = 1e4 + z[i] * 0.5
    a = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, K - 1, rng.integers(0, K, n)))
    a = np.where(kind == HOT, (hot + (np.arange(n) // 5) % 2) % K, a)
    gl, ge = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    return dict(z=z.astype(F32), a=a.astype(np.int64), kind=kind, hot=hot, d_logp=gl, d_ent=ge)


def categorical_eval_ref(z, a, d_logp, d_ent, dtype):
    """softmax -> p, n = p / sum p, l = log(clamp(n, eps32, 1 - eps32)); logp = l_a, entropy -sum n l;
    d_logits = d(sum d_logp logp + sum d_ent entropy) / dz by autograd (a weight None: zero).  p is what the forward
    kernel stores as probs."""
    zt = _T(z, dtype).requires_grad_()
    e = torch.exp(zt - zt.max(1, keepdim=True).values.detach())
    p = e / e.sum(1, keepdim=True)
    nrm = p / p.sum(1, keepdim=True)
    l = torch.log(torch.clamp(nrm, EPS32, 1.0 - EPS32))
    logp = l[torch.arange(len(a)), torch.as_tensor(a)]
    ent = -(nrm * l).sum(1)
    w = lambda g: _T(np.zeros(len(a)) if g is None else g, dtype)
    (w(d_logp) * logp + w(d_ent) * ent).sum().backward()
    return dict(logp=_np(logp), ent=_np(ent), probs=_np(p), n=_np(nrm), d_logits=_np(zt.grad))


CAT_SAMPLE_CASES = [dict(K=1, n=300, scale=1.0, seed=0), dict(K=2, n=1, scale=1.0, seed=0), dict(K=5, n=300, scale=1.0, seed=0),
                    dict(K=64, n=300, scale=0.3, seed=0), dict(K=64, n=1, scale=0.3, seed=0), dict(K=2, n=300, scale=1.0, seed=0)]


def categorical_sample_logits(c):
    return (c["scale"] * np.random.default_rng(77 + c["seed"] + 10 * c["K"] + c["n"]).standard_normal((c["n"], c["K"]))).astype(F32)


def categorical_sample_ref(z, dtype, seed=SEED, offset=OFFSET):
    """head_draws' inverse-CDF draw at counters offset + row -> dict(a, gap, probs, logp)."""
    a, gap, p, s = hd.categorical_draw(z, seed, philox.counters_u64(offset, np.arange(len(z))), dtype)
    return dict(a=a, gap=gap, probs=p.astype(np.float64), logp=hd.categorical_logp(p, s, a, dtype).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------ K6 Gaussian
GAUSS_EVAL_SHAPES = [(1, 2049, 0), (4, 1, 2), (5, 1023, 0), (17, 1024, 0), (64, 1025, 0), (4, 1, 1)]      # (D, n, row shift)
MIN_STD = 0.01
PLAIN, X12, X60, MEAN9 = 0, 1, 2, 3


def gaussian_inputs(D, n, shift=0, seed=9):
    """log_std: -8 at d % 4 == 0 (softplus below min_std: the floor, no gradient), 25 at d % 4 == 1 (softplus' identity
    branch), U(-1.5, 0.5) elsewhere.  Rows by (i + shift) % 7: 1 has x = 12 in the last dimension (1 - tanh^2 < 1e-6),
    2 has x = 60 in dimension 0 under the floored std (the normal log-density below -100), 3 has mean = 9 in the last
    dimension (the entropy's tanh clamp)."""
    rng = np.random.default_rng(seed + 100 * D + n)
    log_std = rng.uniform(-1.5, 0.5, D)
    log_std[0::4], log_std[1::4] = -8.0, 25.0
    log_std = log_std.astype(F32)
    sd = hd.gauss_std(log_std, c32(MIN_STD), np.float64)
    mean = rng.standard_normal((n, D))
    kind = (np.arange(n) + shift) % 7
    kind = np.where(kind > 3, PLAIN, kind)
    mean[kind == MEAN9, D - 1] = 9.0
    x = mean + sd * rng.standard_normal((n, D))
    x[kind == X12, D - 1] = 12.0
    x[kind == X60, 0] = 60.0
    gl, ge = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    return dict(mean=mean.astype(F32), log_std=log_std, x=x.astype(F32), kind=kind, d_logp=gl, d_ent=ge)


def gaussian_terms(mean, log_std, x, dtype, min_std=MIN_STD):
    """The per-dimension pieces, torch tensors in `dtype` (mean and log_std leaves that require grad)."""
    m, ls, xx = _T(mean, dtype).requires_grad_(), _T(log_std, dtype).requires_grad_(), _T(x, dtype)
    sp = F.softplus(ls)                                                   # beta 1, threshold 20
    sd = torch.max(sp, torch.tensor(c32(min_std), dtype=_td(dtype)))
    zz = xx - m
    l = -(zz * zz) / (2.0 * sd * sd) - torch.log(sd) - c32(HALF_LOG_2PI)
    l0 = -torch.log(sd) - c32(HALF_LOG_2PI)
    return dict(m=m, ls=ls, x=xx, sp=sp, sd=sd, l=l, l0=l0, tx=1.0 - torch.tanh(xx) ** 2, tm=1.0 - torch.tanh(m) ** 2)


def gaussian_eval_ref(mean, log_std, x, d_logp, d_ent, dtype, min_std=MIN_STD):
    """logp = sum_d clamp(log N(x; mean, sd), +-100) - sum_d log(max(1 - tanh(x)^2, 1e-6)), entropy = -(that at x = mean);
    d_mean / d_log_std of sum d_logp logp + sum d_ent entropy by autograd (a weight None: zero)."""
    t = gaussian_terms(mean, log_std, x, dtype, min_std)
    logp = torch.clamp(t["l"], -100.0, 100.0).sum(1) - torch.log(torch.clamp(t["tx"], min=c32(1e-6))).sum(1)
    ent = (torch.log(torch.clamp(t["tm"], min=c32(1e-6))) - torch.clamp(t["l0"], -100.0, 100.0)).sum(1)
    n = len(mean)
    w = lambda g: _T(np.zeros(n) if g is None else g, dtype)
    (w(d_logp) * logp + w(d_ent) * ent).sum().backward()
    return dict(logp=_np(logp), ent=_np(ent), d_mean=_np(t["m"].grad), d_log_std=_np(t["ls"].grad))


GAUSS_SAMPLE_CASES = [(1, 257, False), (3, 1, True), (4, 257, True), (5, 1, False), (8, 257, False), (9, 257, True), (64, 257, True),
                      (64, 1, False)]                                    # (D, n, per-dimension bounds)


def gaussian_sample_inputs(D, n, bounded, seed=21):
    rng = np.random.default_rng(seed + 10 * D + n)
    mean = (0.5 * rng.standard_normal((n, D))).astype(F32)
    log_std = rng.uniform(-1.5, 0.0, D).astype(F32)
    bounds = (rng.uniform(-3.0, -0.5, D).astype(F32), rng.uniform(0.5, 4.0, D).astype(F32)) if bounded else None
    return mean, log_std, bounds


def gaussian_sample_ref(mean, log_std, bounds, dtype, seed=SEED, offset=OFFSET, min_std=MIN_STD):
    n, D = mean.shape
    z = hd.gauss_normals(seed, philox.counters_u64(offset, np.arange(n)), D, dtype)
    sd = hd.gauss_std(log_std, c32(min_std), dtype)
    m = mean.astype(dtype)
    raw = m + sd * z
    act, logp = hd.squashed_gaussian(m, sd, raw, bounds, dtype)
    return dict(raw=raw.astype(np.float64), action=act.astype(np.float64), logp=logp.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------ K8
ICM_SHAPES = [(1, 1), (3, 2), (4, 63), (5, 64), (1025, 65), (3, 128), (5, 200), (1025, 128), (2625, 200)]       # (n, D)
ICM_SCALE, ICM_G = 0.7, 3.0


def icm_inputs(n, D):
    rng = np.random.default_rng(n * 7 + D)
    return rng.standard_normal((n, D)).astype(F32), rng.standard_normal((n, D)).astype(F32)


def icm_ref(pred, enc2, dtype, scale=ICM_SCALE, g=ICM_G):
    n, D = pred.shape
    d = pred.astype(dtype) - enc2.astype(dtype)
    rowsum = (d * d).sum(1)
    d_pred = d * (dtype(g) * (dtype(1.0) / (dtype(n) * dtype(D))))
    return dict(rowsum=rowsum, intr=dtype(c32(scale)) * dtype(0.5) * rowsum, f_loss=dtype(0.5) * rowsum.sum() / dtype(n * D),
                d_pred=d_pred, d_enc2=-d_pred)


# ------------------------------------------------------------------------------------------------------------ K9
def attention_cases():
    """Every L in 1..16 with a partial last tile (where a tile holds more than one sequence) and 1, 2 or 3 idle waves in the
    last workgroup; D over 16 / 64 / 128, 1024 twice; masked for odd L; one saturated case (q, k scaled by 8)."""
    out = []
    for L in range(1, 17):
        per, idle = 16 // L, 1 + L % 3
        tiles = 8 - idle
        n_seq = (tiles - 1) * per + max(1, per - 1)
        out.append(dict(L=L, n_seq=n_seq, D=(16, 64, 128)[L % 3], masked=bool(L % 2), scale=1.0))
    out += [dict(L=3, n_seq=6, D=1024, masked=True, scale=1.0), dict(L=16, n_seq=2, D=1024, masked=False, scale=1.0),
            dict(L=5, n_seq=7, D=64, masked=True, scale=8.0), dict(L=7, n_seq=1, D=16, masked=True, scale=1.0)]
    return out


def attention_name(c):
    return f"L{c['L']}_n{c['n_seq']}_D{c['D']}_{'masked' if c['masked'] else 'full'}" + ("_x8" if c["scale"] != 1.0 else "")


def attention_inputs(c):
    rng = np.random.default_rng(c["L"] * 1000 + c["n_seq"] + c["D"])
    shape = (c["n_seq"], c["L"], c["D"])
    q, k, v, dy = (rng.standard_normal(shape).astype(F32) for _ in range(4))
    return (q * F32(c["scale"])), (k * F32(c["scale"])), v, dy


def attention_ref(q, k, v, dy, masked, dtype):
    """networks/attention.py:94-103 with autograd: dict(y, probs (zeros at masked entries), dq, dk, dv)."""
    qt, kt, vt = (_T(t, dtype).requires_grad_() for t in (q, k, v))
    L, D = q.shape[-2], q.shape[-1]
    att = (qt @ kt.transpose(-2, -1)) * (1.0 / np.sqrt(D))
    if masked:
        att = att.masked_fill(torch.tril(torch.ones(L, L)) == 0, float("-inf"))
    probs = torch.softmax(att, dim=-1)
    y = probs @ vt
    (y * _T(dy, dtype)).sum().backward()
    return dict(y=_np(y), probs=_np(probs), dq=_np(qt.grad), dk=_np(kt.grad), dv=_np(vt.grad))


# ------------------------------------------------------------------------------------------------------------ K11
LR, ADAM_EPS, BETA1, BETA2 = c32(3e-4), c32(1e-5), 0.9, 0.999
CLIP_ON, CLIP_OFF, CLIP_NONE = "active", "inactive", "max_norm<=0"
ADAM_CASES = [dict(n=n, step=(0, 6, 100000)[i % 3], clip=(CLIP_ON, CLIP_OFF, CLIP_NONE)[(i // 2) % 3], scale=(1.0, 0.125)[i % 2],
                   norm_out=i % 4 != 3) for i, n in enumerate((1, 2, 3, 4, 5, 1023, 1024, 1025, 65 * 1024 + 3, 2048 * 256 + 5))]
PRENORMED_PARTIALS = (0, 1, 64, 65, 200)


def adam_inputs(n, step, seed=31):
    """Parameters, gradients and a preset non-zero Adam state on the gradient's scale."""
    rng = np.random.default_rng(seed + n + step)
    p = (0.1 * rng.standard_normal(n)).astype(F32)
    g = (0.05 * rng.standard_normal(n)).astype(F32)
    m = (0.02 * rng.standard_normal(n)).astype(F32)
    v = (0.0025 * rng.uniform(0.2, 2.0, n)).astype(F32)
    return p, g, m, v


def adam_max_norm(clip, g, scale):
    """max_norm that makes the clip active / inactive by a wide margin, or switches it off."""
    norm = float(np.sqrt(((np.asarray(g, np.float64) * scale) ** 2).sum()))
    return {CLIP_ON: 0.37 * norm, CLIP_OFF: 2.5 * norm + 1.0, CLIP_NONE: 0.0}[clip]


def adam_ref(p, g, m, v, t, max_norm, scale, dtype, sq=None, lr=LR, eps=ADAM_EPS):
    """One step with the counter already at t: gradients times `scale`, clipped by min(max_norm / (norm + 1e-6), 1) where
    max_norm > 0 (norm = sqrt(sq), sq given or the scaled gradients' own), then torch.optim.Adam's update.
    -> dict(norm, sq, p, m, v) as float64 arrays."""
    pt, gt, mt, vt = (_T(a, dtype) for a in (p, g, m, v))
    gs = gt * scale
    sqt = (gs * gs).sum() if sq is None else torch.tensor(float(sq), dtype=_td(dtype))
    norm = torch.sqrt(sqt)
    if max_norm > 0:
        gs = gs * torch.clamp(max_norm / (norm + c32(1e-6)), max=1.0)
    mw = BETA1 * mt + (1 - BETA1) * gs
    vw = BETA2 * vt + (1 - BETA2) * gs * gs
    bc1, bc2 = 1 - BETA1 ** t, 1 - BETA2 ** t
    pw = pt - (lr / bc1) * (mw / (torch.sqrt(vw) / np.sqrt(bc2) + eps))
    return dict(norm=float(norm), sq=float(sqt), p=_np(pw), m=_np(mw), v=_np(vw))
