"""
Steering that CLOSES the gradient gates of the fused update kernels' action heads (no device): the 0 / 1 factors by which
the hand-derived backwards restate "autograd passes no gradient through a clamp" --

  floor / ceil   n >= eps32 / n <= 1 - eps32 per class (Categorical, every MultiDiscrete slice; MultiBinary: per bit's p)
  chosen         the same two at the chosen class: a closed one takes the row's surrogate gradient away
  density        Normal.log_prob in [-100, 100] per Gaussian dimension
  tanh           1 - tanh(mean)^2 >= 1e-6 per Gaussian dimension (the entropy's clamp)
  std_floor      softplus(log_std) > min_std per dimension
  identity       log_std <= 20 per dimension (above: softplus's identity branch)

-- in csrc/ppo_update_dev.hpp (ppo_head_rows), csrc/action_heads.hpp (mcat_entropy_grad, bern_entropy_grad),
csrc/ppo_update_rowtile_heads.hpp, csrc/mat_update.hip and csrc/distributions.hip.

steer_model works on the flat parameter bucket through a Model (where the last Linear and log_std lie, the actor's float64
forward, how a row's inputs are drawn and scaled); steer is the Model of a feed-forward pair of ko.Nets (K12).  K22 and K15
put a LayerNorm between the inputs and the head, so scaling a row's input does not move its confidence: their steerings
(lstm_update_cases.Steering._steer_gates, mat_update_cases.Steering._gates) pick among drawn candidates instead, with this
module's last-layer steering, planting, census and near-gate rule.
  discrete heads   the actor's last weight and bias x a factor that brings the float64 logits to a root mean square of
                   1.5 x saturate over rows of unit scale; the rows' observations are N(0, 1) x ROW_SCALES in turn, so
                   that confident and unconfident rows stand side by side.  Actions are planted by row index: the top
                   class; the largest class below eps32 (kind c: log-prob log eps32, no surrogate gradient); an in-range
                   class that is not the top one; a uniform draw.  MultiDiscrete turns the rule by one per slice (rows of
                   mixed kinds), MultiBinary plants bit (row + d) % 2.
                   TUNED rows (1, 5, 9 ..): a chosen class far below eps32 hides a wrong gate as well as a closed one
                   does (an open gate lets n / eps32 of the row's surrogate gradient through).  Their observation's scale
                   is found by bisection so that the first Categorical's second class -- the chosen one -- stands at
                   TUNED x eps32 (MultiBinary: the most confident bit at TUNED x eps32 from 0 or 1, its bit planted against
                   it), and force_surrogate puts their ratio inside the clip with an advantage of +-2.
  Gaussian head    log_std[d] = -8 where d % 4 == 0 (sd = min_std), 25 where d % 4 == 1, the policy's own elsewhere.  In a
                   floored dimension x = mu64 +- 0.05 (mean gradient of order 0.05 / min_std^2) in the rows with
                   (row + d / 4) % 2 == 0 and mu64 +- U(0.2, 0.3) (density below -100) in the others: a row then has closed
                   and open dimensions.  A floored dimension's output row is scaled down until its means have a root
                   mean square of FLOORED_RMS at most: float32's own error in mu enters the mean gradient as
                   d mu / min_std^2, and means of order 1 (1e-7 off in any float32 evaluation) would spend the whole
                   bound -- 1e-5 of a gradient of 0.05 / min_std^2 -- on that rounding alone, whatever the gates do.
                   Elsewhere x = mu64 + min(sd, 1.5) N(0, 1).  One output row of the last layer
                   (tanh_dim) is scaled to a standard deviation of TANH_SPREAD over the rows and given the bias that
                   lifts the share TANH_SHARE of them above TANH_TOP: |mu| > 7.26 there, nearly all on one side, so that
                   their entropy terms add up in the bias's gradient.
KINDS of a (row, slice): a  no class outside [eps32, 1 - eps32];  b  a class other than the chosen one below eps32;
c  the chosen class below eps32;  d  a class above 1 - eps32.  (c before d before b where several hold.)  MultiBinary:
low0 / low1 / high0 / high1 -- p < eps32 or p > 1 - eps32 with the bit.

NEAR-GATE RULE (ko.kinked_rows applied to gates): a row whose gate argument float32 could put on the other side gets new
inputs from default_rng((seed, round)), at most 50 rounds:
  * n <= 1 - eps32 is decided by n's rounding onto float32's grid (spacing eps32 / 2 below 1): (1 - n64) / eps32 in [0.5, 2];
    the same for MultiBinary's p (float32's sigmoid reaches 1 near z = 16.6, float64 crosses 1 - eps32 at 15.94);
  * 1 - tanh(mu)^2 is a difference of float32 numbers next to 1 (steps of 1.2e-7 around the threshold 1e-6):
    (1 - tanh^2) / 1e-6 in [0.5, 2];
  * every other gate within 1e-3 relative of its threshold: n / eps32, |l| / 100, softplus(log_std) / min_std.
The rule is checked, not trusted: census() of the float32 reference must equal that of the float64 one entry for entry
(same_census), wherever the steering is used.

OUT OF SCOPE: exact ties (softplus == min_std with dmax = 0.5, an argument exactly on a bound: not reachable from a
float64 comparison); the pass0 gate (sd < e^-101 or > e^99: unreachable with min_std > 0 in float32); the NaN / Inf flag
(tests/test_gpu_recovery.py).
"""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from oracle import k12_oracle as ko

EPS32 = ko.EPS32
ROW_SCALES = (1.0, 1.0, 0.1, 0.5)   # of the discrete heads' observations by row % 4; rows 1, 5, 9 .. are tuned from theirs
TUNED = 0.2                      # a tuned row's probability just past the gate, in units of eps32
# the scaled Gaussian output: its standard deviation over the rows; the share of rows its bias lifts above TANH_TOP (past the
# gate and past the near-gate band, which ends at |mu| = 7.6)
TANH_SPREAD, TANH_SHARE, TANH_TOP = 4.5, 0.3, 7.9
FLOORED_RMS = 0.01               # of the means of a floored Gaussian dimension (the policies' initial output gain)
# the gates a case of each head names: both sides hold at least MIN_ENTRIES entries
NAMED = {"categorical": ("floor", "ceil", "chosen"), "multi_categorical": ("floor", "ceil", "chosen"),
         "bernoulli": ("floor", "ceil"), "gaussian": ("density", "tanh")}
MIN_ENTRIES = 2


def named_gates(head, out_dim):
    """std_floor / identity have two dimensions on the closed side from 6 dimensions on (0, 4 and 1, 5)."""
    return NAMED[head] + (("std_floor", "identity") if head == "gaussian" and out_dim >= 6 else ())


class Model(NamedTuple):
    weight: tuple                 # (offset, shape) of the actor's last Linear in the bucket
    bias: tuple
    log_std: Optional[int]        # offset, Gaussian head
    out_dim: int
    forward: Callable             # (params, inputs) -> float64 actor output [B, out_dim]
    draw: Callable                # (generator, row indices) -> unit-scale inputs of these rows (dict of float64 arrays)
    scaled: Callable              # (unit inputs, row scales [B]) -> the inputs as the kernel reads them (float32)
    kinked: Callable              # (params, inputs) -> bool [B]


class Gated(NamedTuple):
    params: np.ndarray            # the steered bucket (float32-exact float64)
    inputs: dict
    actions: np.ndarray           # raw actions, float32: [B] / [B, slices] / [B, bits] / [B, D]
    tanh_dim: Optional[int]
    forced: np.ndarray            # rows whose ratio and advantage are set by hand (force_surrogate): the tuned rows


def _span(params, span):
    off, shape = span
    return slice(off, off + int(np.prod(shape)))


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def slice_table(head, slices, out_dim):
    """[(start, n)] of the head's Categoricals over the actor's outputs."""
    if head == "categorical":
        return [(0, out_dim)]
    out, start = [], 0
    for n in slices:
        out.append((start, n))
        start += n
    return out


def probabilities(head, slices, out):
    """float64 renormalised probabilities of the logits [B, out_dim] (MultiBinary: sigmoid), as the oracle forms them."""
    t = torch.as_tensor(out, dtype=torch.float64)
    if head == "bernoulli":
        return torch.sigmoid(t).numpy()
    ps = []
    for start, n in slice_table(head, slices, out.shape[1]):
        p = torch.softmax(t[:, start:start + n], dim=-1)
        ps.append((p / p.sum(-1, keepdim=True)).numpy())
    return np.concatenate(ps, axis=1)


def near_discrete(n):
    """[B] rows with a class (bit) that float32 could put on the other side of a gate (module docstring)."""
    lo = np.abs(n / EPS32 - 1.0) < 1e-3
    r = (1.0 - n) / EPS32
    return (lo | ((r >= 0.5) & (r <= 2.0))).any(axis=1)


def near_gaussian(args, min_std):
    """([B] rows near the density or the tanh gate, whether a dimension is near the floor or the identity threshold)."""
    l, tp = np.abs(args["density"]), args["tanh_prime"] / 1e-6
    rows = (np.abs(l / 100.0 - 1.0) < 1e-3).any(axis=1) | ((tp >= 0.5) & (tp <= 2.0)).any(axis=1)
    dims = (np.abs(args["softplus"] / min_std - 1.0) < 1e-3) | (np.abs(args["log_std"] / 20.0 - 1.0) < 1e-3)
    return rows, bool(dims.any())


def near_rows(head, args, min_std=0.01):
    """[B] rows the near-gate rule would draw again, from a reference's gate_args."""
    if head == "gaussian":
        rows, dims = near_gaussian(args, min_std)
        return rows | dims
    return near_discrete(args["n"])


def census(head, slices, args, actions, min_std=0.01):
    """{gate: bool array, True where the gate is OPEN (gradient passes)} from a reference's gate_args (either dtype) and the
    mini-batch's raw actions.  Discrete heads add "kind": the kind of each (row, slice) -- MultiBinary: of each (row, bit),
    "" where p is in range."""
    if head == "gaussian":
        return dict(density=np.abs(args["density"]) <= 100.0, tanh=args["tanh_prime"] >= 1e-6,
                    std_floor=args["softplus"] > min_std, identity=args["log_std"] <= 20.0)
    n = args["n"]
    B = len(n)
    lo, hi = n >= EPS32, n <= 1.0 - EPS32
    out = dict(floor=lo, ceil=hi)
    if head == "bernoulli":
        bit = np.asarray(actions).reshape(B, -1) > 0.5
        kind = np.full(n.shape, "", dtype=object)
        kind[~lo & ~bit], kind[~lo & bit], kind[~hi & ~bit], kind[~hi & bit] = "low0", "low1", "high0", "high1"
        out["kind"] = kind
        return out
    a = np.asarray(actions).astype(np.int64).reshape(B, -1)
    table = slice_table(head, slices, n.shape[1])
    chosen, kind = np.zeros((B, len(table)), dtype=bool), np.full((B, len(table)), "a", dtype=object)
    for j, (start, k) in enumerate(table):
        l, h = lo[:, start:start + k], hi[:, start:start + k]
        c = np.clip(a[:, j], 0, k - 1)
        rows = np.arange(B)
        chosen[:, j] = l[rows, c] & h[rows, c]
        kind[(~l).any(1), j] = "b"
        kind[(~h).any(1), j] = "d"
        kind[~l[rows, c], j] = "c"
    out["chosen"], out["kind"] = chosen, kind
    return out


def counts(cen):
    """{gate: (entries on the open side, on the closed side)}, {kind: entries}."""
    gates = {g: (int(v.sum()), int((~v).sum())) for g, v in cen.items() if g != "kind"}
    kinds = {}
    if "kind" in cen:
        for k in cen["kind"].reshape(-1):
            if k:
                kinds[k] = kinds.get(k, 0) + 1
    return gates, kinds


def same_census(a, b):
    """The gates (and kinds) whose entries differ between two censuses (empty: equal entry for entry)."""
    return [g for g in a if a[g].shape != b[g].shape or not np.array_equal(a[g], b[g])]


def census_failures(head, slices, out_dim, r64, r32, actions, min_std=0.01):
    """What the steering promises, checked on the two references of the steered mini-batch -> readable lines (empty: kept):
    both sides of every named gate hold MIN_ENTRIES entries, every kind is there, float32 reports float64's census, and no
    row is left near a gate."""
    c64 = census(head, slices, r64["gate_args"], actions, min_std)
    c32 = census(head, slices, r32["gate_args"], actions, min_std)
    gates, kinds = counts(c64)
    bad = [f"gate {g}: {gates[g][0]} open / {gates[g][1]} closed entries" for g in named_gates(head, out_dim)
           if min(gates[g]) < MIN_ENTRIES]
    if head == "gaussian":
        mixed = (~c64["density"]).any(1) & c64["density"].any(1)
        if mixed.sum() < MIN_ENTRIES:
            bad.append("no rows with closed and open density gates side by side")
        gates_1 = {g: gates[g] for g in ("std_floor", "identity")}
        bad += [f"gate {g}: no dimension on one side {v}" for g, v in gates_1.items() if min(v) < 1 and out_dim >= 2]
    elif head == "bernoulli":
        bad += [f"kind {k}: {kinds.get(k, 0)} entries" for k in ("low0", "low1", "high0", "high1")
                if kinds.get(k, 0) < MIN_ENTRIES]
        if (c64["kind"] == "").sum() < MIN_ENTRIES:
            bad.append("no bits in range")
    else:
        need = MIN_ENTRIES if head == "categorical" else 1
        # (two classes: the other class below eps32 IS the chosen one above 1 - eps32 -- kind b is kind d)
        want = "acd" if head == "categorical" and out_dim == 2 else "abcd"
        bad += [f"kind {k}: {kinds.get(k, 0)} (row, slice) entries" for k in want if kinds.get(k, 0) < need]
        if head == "multi_categorical" and not any(len(set(row)) > 1 for row in c64["kind"]):
            bad.append("no row whose slices are of different kinds")
    diff = same_census(c64, c32)
    if diff:
        bad.append("float32 census differs from float64 in " + ", ".join(diff))
    left = int(near_rows(head, r64["gate_args"], min_std).sum())
    if left:
        bad.append(f"{left} rows left near a gate")
    return bad


def describe(head, slices, r64, actions, min_std=0.01):
    gates, kinds = counts(census(head, slices, r64["gate_args"], actions, min_std))
    return "  ".join(f"{g} {o}/{c}" for g, (o, c) in gates.items()) + "  kinds " + \
        " ".join(f"{k}:{v}" for k, v in sorted(kinds.items()))


# ------------------------------------------------------------------------------------------------------------ planting
def _plant_classes(n_row, rule, rng):
    """One Categorical's chosen class under `rule` (module docstring)."""
    k = len(n_row)
    top = int(np.argmax(n_row))
    below = [i for i in range(k) if n_row[i] < EPS32]
    inside = [i for i in range(k) if EPS32 <= n_row[i] <= 1.0 - EPS32 and i != top]
    if rule == 0:
        return top
    if rule == 1 and below:
        return max(below, key=lambda i: n_row[i])
    if rule == 2 and inside:
        return max(inside, key=lambda i: n_row[i])
    return int(rng.integers(0, k))


def plant_discrete(head, slices, out, n, rng):
    """Raw actions (float32) of the discrete heads from the float64 logits and probabilities [B, out_dim]."""
    B = len(n)
    if head == "bernoulli":
        a = ((np.arange(B)[:, None] + np.arange(n.shape[1])[None, :]) % 2).astype(np.float32)
        for i in range(1, B, 4):                      # a tuned row: the bit against its most confident logit
            d = int(np.argmax(np.abs(out[i])))
            a[i, d] = 1.0 if out[i, d] < 0 else 0.0
        return a
    table = slice_table(head, slices, n.shape[1])
    a = np.zeros((B, len(table)), dtype=np.float32)
    for i in range(B):
        for j, (start, k) in enumerate(table):
            a[i, j] = _plant_classes(n[i, start:start + k], (i + j) % 4, rng)
    return a[:, 0] if head == "categorical" else a


def tuning_margin(head, slices, out):
    """[B] > 0 while a row is less confident than its tuned rows should be: the first Categorical's second class at
    TUNED x eps32 (its top class is then above 1 - eps32), MultiBinary's most confident bit at TUNED x eps32 from 0 or 1."""
    if head == "bernoulli":
        return (-np.log(TUNED * EPS32)) - np.abs(out).max(axis=1)
    start, k = slice_table(head, slices, out.shape[1])[0]
    n = probabilities("categorical", (), out[:, start:start + k])
    second = np.sort(n, axis=1)[:, -2] if k > 1 else n[:, 0]
    return np.log(np.maximum(second, 1e-300) / (TUNED * EPS32))


def plant_gaussian(mu, log_std, min_std, rng, tanh_dim):
    """Raw actions (float32) of the Gaussian head from the float64 means mu [B, D].  The scaled dimension's actions stay
    within |x| <= 3: between 4 and 7.3 the log-prob's own log(1 - tanh(x)^2) is a difference of float32 numbers next to 1
    and carries per cent of noise into the ratio, which would raise every float32 floor.  An entry whose density lands
    within 5e-3 of -100 is moved by 0.3 sd."""
    B, D = mu.shape
    sd = np.maximum(np.logaddexp(0.0, log_std), np.float64(np.float32(min_std)))
    x = mu + np.minimum(sd, 1.5)[None, :] * rng.normal(0, 1, (B, D))
    x[:, tanh_dim] = np.clip(x[:, tanh_dim], -3.0, 3.0)
    for d in range(0, D, 4):
        sign = np.where(rng.random(B) < 0.5, -1.0, 1.0)
        far = (np.arange(B) + d // 4) % 2 == 1
        x[:, d] = mu[:, d] + sign * np.where(far, rng.uniform(0.2, 0.3, B), 0.05)
    x = x.astype(np.float32)
    for _ in range(8):
        l = -(x - mu) ** 2 / (2.0 * sd * sd) - np.log(sd) - 0.5 * np.log(2.0 * np.pi)
        close = np.abs(np.abs(l) / 100.0 - 1.0) < 5e-3
        if not close.any():
            break
        x = np.where(close, x + np.sign(x - mu) * 0.3 * sd, x).astype(np.float32)
    return x


FORCED = ((1.05, -2.0), (0.9, 2.0))      # (ratio, advantage): inside the clip, so that the row's surrogate carries gradient


def force_surrogate(old, adv, logp64, rows):
    """The old log-probs and advantages with the rows `rows` set to FORCED in turn (float32): a tuned row's closed gate is
    then the only thing between its surrogate gradient and the bucket."""
    old, adv = np.array(old, dtype=np.float32), np.array(adv, dtype=np.float32)
    for k, i in enumerate(rows):
        ratio, a = FORCED[k % 2]
        old[i], adv[i] = np.float32(logp64[i] - np.log(ratio)), np.float32(a)
    return old, adv


def tanh_dim_of(D):
    """The dimension whose output row is scaled past the tanh gate: the last one that keeps the policy's own log_std, or
    the last identity-branch one, or 0."""
    for want in ((2, 3), (1,), (0,)):
        ds = [d for d in range(D) if d % 4 in want]
        if ds:
            return ds[-1]


def steer_last_layer(params, weight, bias, log_std, out_dim, head, forward, rms):
    """The bucket with the actor's last Linear ((offset, shape) weight / bias) steered -- discrete heads: x the factor that
    brings forward(params) [rows, out_dim] to the root mean square rms; Gaussian: log_std (offset) set by dimension, the
    output row tanh_dim at TANH_SPREAD with TANH_SHARE of the rows above TANH_TOP -- float32-exact -> (params, tanh_dim)."""
    params = np.array(params, dtype=np.float64)
    w, b = _span(params, weight), _span(params, bias)
    tanh_dim = None
    if head == "gaussian":
        d = np.arange(out_dim)
        ls = slice(log_std, log_std + out_dim)
        params[ls] = np.where(d % 4 == 0, -8.0, np.where(d % 4 == 1, 25.0, params[ls]))
        tanh_dim = tanh_dim_of(out_dim)
        params[bias[0] + tanh_dim] = 0.0
        width = weight[1][1]
        mu = forward(params)
        for k in range(0, out_dim, 4):     # a floored dimension's mean at 0.01 (FLOORED_RMS): see the module docstring
            g = min(1.0, FLOORED_RMS / np.sqrt((mu[:, k] ** 2).mean()))
            params[weight[0] + k * width:weight[0] + (k + 1) * width] *= g
            params[bias[0] + k] *= g
        mu = mu[:, tanh_dim]
        g = TANH_SPREAD / mu.std()
        params[weight[0] + tanh_dim * width:weight[0] + (tanh_dim + 1) * width] *= g
        params[bias[0] + tanh_dim] = TANH_TOP - np.quantile(g * mu, 1.0 - TANH_SHARE)
    else:
        g = rms / np.sqrt((forward(params) ** 2).mean())
        params[w] *= g
        params[b] *= g
    params[w], params[b] = _f32(params[w]), _f32(params[b])
    return params, tanh_dim


def _tune(params, model, head, slices, unit, t, rows):
    """Bisection of the row scales t[rows] on (0.02, 1.5) to tuning_margin == 0; a row without a crossing keeps its scale."""
    if not len(rows):
        return t
    lo, hi = t.copy(), t.copy()
    lo[rows], hi[rows] = 0.02, 1.5
    f = lambda tt: tuning_margin(head, slices, model.forward(params, model.scaled(unit, tt)))
    ok = np.zeros(len(t), dtype=bool)
    ok[rows] = (f(lo)[rows] > 0) & (f(hi)[rows] < 0)
    for _ in range(40):
        mid = np.sqrt(lo * hi)
        up = f(mid) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return np.where(ok, np.sqrt(lo * hi), t)


def steer_model(params, model, head, slices, B, rng, seed, saturate=20.0, min_std=0.01):
    """-> Gated: the steered bucket, the rows' inputs and the planted raw actions (module docstring).  `rng` draws the
    inputs and the actions; redrawn rows come from default_rng((seed, round))."""
    rows = np.arange(B)
    unit = model.draw(rng, rows)
    tuned = rows[1::4] if head != "gaussian" else rows[:0]
    t = np.array([ROW_SCALES[i % 4] for i in rows]) if head != "gaussian" else np.ones(B)
    params, tanh_dim = steer_last_layer(params, model.weight, model.bias, model.log_std, model.out_dim, head,
                                        lambda p: model.forward(p, model.scaled(unit, np.ones(B))), 1.5 * saturate)
    if head == "gaussian":
        ls = slice(model.log_std, model.log_std + model.out_dim)
    fresh = tuned
    for rnd in range(50):
        t = _tune(params, model, head, slices, unit, t, fresh)
        inputs = model.scaled(unit, t)
        out = model.forward(params, inputs)
        if head == "gaussian":
            tp = (1.0 - np.tanh(out) ** 2) / 1e-6
            near = ((tp >= 0.5) & (tp <= 2.0)).any(axis=1)
        else:
            near = near_discrete(probabilities(head, slices, out))
        bad = near | model.kinked(params, inputs)
        if not bad.any():
            break
        new = model.draw(np.random.default_rng((seed, rnd)), rows[bad])
        for k, v in new.items():
            unit[k][bad] = v
        fresh = np.intersect1d(tuned, rows[bad])
        t[fresh] = ROW_SCALES[1]
    else:
        raise AssertionError("rows near a gate (or a kink) left after 50 redraws")
    if head == "gaussian":
        actions = plant_gaussian(out, params[ls], min_std, rng, tanh_dim)
    else:
        actions = plant_discrete(head, slices, out, probabilities(head, slices, out), rng)
    return Gated(params, inputs, actions, tanh_dim, tuned)


# ------------------------------------------------------------------------------------------------- K12: a feed-forward pair
def actor_output(actor, seg, obs, dtype=torch.float64):
    m, _ = ko._module(actor, np.asarray(seg, dtype=np.float64), dtype)
    with torch.no_grad():
        return m(torch.as_tensor(np.asarray(obs), dtype=dtype)).double().numpy()


def feed_forward_model(actor, critic, head):
    """The Model of K12's bucket (ko.bucket_tables): inputs are obs [B, actor in_dim], scaled row by row, and cobs
    [B, critic in_dim]."""
    table, na = ko.tensor_table(actor, head == "gaussian")
    spans = {name: (off, shape) for name, off, shape in table}

    def draw(g, idx):
        return dict(obs=g.normal(0, 1, (len(idx), actor.in_dim)), cobs=g.normal(0, 1, (len(idx), critic.in_dim)))

    def scaled(unit, t):
        return dict(obs=(unit["obs"] * t[:, None]).astype(np.float32), cobs=unit["cobs"].astype(np.float32))

    def kinked(params, inputs):
        return ko.kinked_rows(actor, params[:na], inputs["obs"]) | ko.kinked_rows(critic, params[na:], inputs["cobs"])

    return Model(spans[f"{actor.depth}.weight"], spans[f"{actor.depth}.bias"],
                 spans["log_std"][0] if head == "gaussian" else None, actor.out_dim,
                 lambda params, inputs: actor_output(actor, params[:na], inputs["obs"]), draw, scaled, kinked)


def steer(params, actor, critic, head, slices, B, rng, seed, saturate=20.0, min_std=0.01):
    """steer_model on K12's flat bucket of the two ko.Nets."""
    return steer_model(params, feed_forward_model(actor, critic, head), head, slices, B, rng, seed, saturate, min_std)


def draw_bucket(actor, critic, head, rng, last_gain=0.01):
    """A bucket on the scale of the policies' initial weights for CPU tests: N(0, 1 / fan_in) x sqrt(2) hidden weights, the
    actor's last weight x last_gain, zero biases, log_std 0 (float32-exact)."""
    tables, size = ko.bucket_tables(actor, critic, head)
    p = np.zeros(size)
    for tag, name, off, shape in tables:
        if len(shape) == 2:
            gain = last_gain if (tag == "actor" and name == f"{actor.depth}.weight") else np.sqrt(2.0)
            p[off:off + int(np.prod(shape))] = rng.normal(0, gain / np.sqrt(shape[1]), int(np.prod(shape)))
    return _f32(p)


# ------------------------------------------------------------------------------------------------------- the K12 cases
def k12_case(O, ha, hc, depth, B, head, act, seed, ent=0.01, **kw):
    """Keywords of test_gpu_k12_gradients.case (which adds the defaults) for a gates case."""
    return dict(O=O, ha=ha, hc=hc, depth=depth, B=B, head=head, act=act, seed=seed, ent=ent, gates=True, **kw)


K12_CASES = {
    # both class slots of a lane quad, a ragged tile
    "cat8_64": k12_case(8, 64, 64, 2, 33, ("categorical", 8), "tanh", 901),
    # csrc/ppo_update_narrow.hip
    "cat5_narrow": k12_case(12, 32, 256, 2, 17, ("categorical", 5), "relu", 902),
    # mcat_entropy_grad, rows of mixed kinds
    "mcat_323": k12_case(8, 64, 64, 2, 33, ("multi_categorical", (3, 2, 3)), "leaky_relu", 903),
    # bern_entropy_grad in csrc/ppo_update_wide.hip
    "bern6_wide_critic": k12_case(11, 256, 512, 2, 33, ("bernoulli", 6), "tanh", 904),
    # every Gaussian gate: floored dimensions 0 and 4, identity dimensions 1 and 5
    "gau8_64": k12_case(8, 64, 64, 2, 33, ("gaussian", 8), "relu", 905, ent=0.01),
    # the row-pair build
    "gau3_rowpair": k12_case(20, 256, 256, 2, 48, ("gaussian", 3), "tanh", 906),
}
# csrc/ppo_update_rowtile_heads.hpp (fused_wide_heads): six classes per lane, a fifth action-word group
K12_HEADS_CASES = {
    "cat24_heads": k12_case(24, 256, 512, 2, 33, ("categorical", 24), "relu", 907),
    "gau17_heads": k12_case(24, 256, 512, 2, 33, ("gaussian", 17), "tanh", 908),
}
# the lean kernel (csrc/ppo_update_lean.hip): depth 3, Categorical(2) / Gaussian(2)
K12_LEAN_CASES = {
    "lean_cat2": k12_case(4, 64, 64, 3, 48, ("categorical", 2), "relu", 909),
    "lean_gau2": k12_case(17, 32, 32, 3, 17, ("gaussian", 2), "leaky_relu", 910),
}
ALL_K12_CASES = {**K12_CASES, **K12_HEADS_CASES, **K12_LEAN_CASES}
VN = (0.3, 0.25, 5000.0)


def head_of(c):
    head = c["head"][0]
    slices = tuple(c["head"][1]) if head == "multi_categorical" else ()
    out_dim = sum(slices) if slices else c["head"][1]
    return head, slices, out_dim


class CpuCase:
    """A K12 gates case on weights drawn on the CPU (draw_bucket) with the loss inputs of
    test_gpu_k12_gradients.Steered: the steered mini-batch and its float64 / float32 references."""

    def __init__(self, c):
        self.c, B = c, c["B"]
        self.head, self.slices, out_dim = head_of(c)
        self.actor = ko.Net(c["O"], c["ha"], c["depth"], out_dim, c["act"])
        self.critic = ko.Net(c["O"] * (2 if c.get("wide_critic") else 1), c["hc"], c["depth"], 1, c["act"])
        self.tables, _ = ko.bucket_tables(self.actor, self.critic, self.head)
        rng = np.random.default_rng(c["seed"])
        g = steer(draw_bucket(self.actor, self.critic, self.head, rng), self.actor, self.critic, self.head, self.slices,
                  B, rng, c["seed"])
        self.params, self.actions = g.params, g.actions
        rtg = (0.3 + 0.5 * rng.normal(0, 1, B)).astype(np.float32)
        rtg[:max(1, B // 50)] = np.float32(0.3 + 0.5 * 20.0)
        adv = rng.normal(0.2, 1.0, B).astype(np.float32)
        self.consts = ko.Consts(True, True, True, 10.0, 0.2, c["ent"], 0.0, 0.01)
        mb = ko.Minibatch(g.inputs["obs"], g.inputs["cobs"], g.actions, np.zeros(B, np.float32), adv, rtg)
        logp = self.reference(torch.float64, mb)["logp"]
        old, adv = force_surrogate(ko.steered_old_log_probs(logp, rng, 0.2), adv, logp, g.forced)
        self.mb = mb._replace(old_log_probs=old, advantages=adv)
        self.r64, self.r32 = self.reference(torch.float64), self.reference(torch.float32)

    def reference(self, dtype, mb=None, **plants):
        return ko.minibatch(self.params, self.actor, self.critic, self.head, self.slices, mb or self.mb, self.consts, VN,
                            dtype=dtype, gate_plants=ko.GatePlants(**plants))

    def census_failures(self):
        return census_failures(self.head, self.slices, self.actor.out_dim, self.r64, self.r32, self.actions)
