"""
The one-lane-per-row heads of csrc/action_heads.hpp (cat_step_row / gauss_step_row, cat_infer_row / gauss_infer_row: K6,
K19 and K21 share them) restated in numpy in a chosen dtype, on tests/helpers/philox.py (held to the published known
answers by tests/test_philox.py).  Row e of a launch has the Philox counter offset + e (philox.counters_u64).

Categorical: p = softmax(z) (the row maximum subtracted, normalised), s = sum p; u = u32_to_unit(word x of
Philox(seed, counter, stream 0)); the action is the first k with u s < cum_k (cum the running sum of p), out_dim - 1 when
there is none; the log-prob log(clip(p_a / s, eps32, 1 - eps32)).  `gap` is min_k |u s - cum_k|, the distance to the
nearest CDF edge.
Gaussian: dimensions 4 q .. 4 q + 3 take the two Box-Muller pairs of block (seed, counter, stream q); raw = mean + sd z,
sd = max(softplus(log_std), min_std); action tanh(raw), rescaled ((a + 1) / 2) (hi - lo) + lo with bounds; log-prob
sum_d clip(log N(raw; mean, sd), -100, 100) - sum_d log(max(1 - a^2, 1e-6)).

Near-tie rule: a logit's bound is 1e-5 |z| + 1e-5 max|z| over the case's float64 logits (logit_bound).  A sampled row
whose u s lies within 2 max_k bound_k + 1e-6 of a CDF edge (softmax is 1-Lipschitz in the max norm, so an edge moves by
at most twice the largest logit error), a greedy row whose top two logits are closer than the sum of their bounds, may be
left out of an action comparison.

MultiDiscrete (mcat_probs / mcat_sample / mcat_pick / mcat_logp): per slice j of `slices` the softmax of the slice's
logits (the slice maximum subtracted, normalised) -> p, s its sum; u = u32_to_unit(word x of Philox(seed,
offset + j E + e, stream 0)); the class is the first k of the slice with u s < cum_k, the slice's last class when there is
none; a forced index is clamped into its slice; the log-prob sum_j log(clip(p / s, eps32, 1 - eps32)) -- a slice of one
class gives log(1 - eps32), not 0.  A slice is near a tie by near_cdf_edge's rule on its own gap, a row when any slice is.
MultiBinary (bern_uniform / bern_logp): bit d = u_d < sigmoid(z_d), u_d from word d % 4 of Philox(seed, counter_e,
stream d / 4); forced bits are taken as given; the log-prob -sum_d BCEWithLogits(logit(clip(sigmoid z_d, eps32,
1 - eps32)), a_d).  A bit is near a tie when |u_d - sigmoid(z_d)| is within the logit's bound / 4 (sigmoid is
1/4-Lipschitz) + 1e-6.
"""
import numpy as np

import philox

EPS32 = float(np.finfo(np.float32).eps)


def logit_bound(z64):
    z64 = np.asarray(z64, np.float64)
    return 1e-5 * np.abs(z64) + 1e-5 * np.abs(z64).max()


def categorical_probs(z, dtype):
    """-> (p [E, out_dim], s [E] its sum, cum [E, out_dim] its running sum), all in `dtype`."""
    z = np.asarray(z, dtype)
    p = np.exp(z - z.max(1, keepdims=True))
    p = p / p.sum(1, keepdims=True)
    return p, p.sum(1), np.cumsum(p, 1)


def categorical_draw(z, seed, counters, dtype, stream=0, word=0, edge_before_mass=False):
    """The inverse-CDF draw of every row -> (action [E], gap [E] to the nearest CDF edge, p, s).  stream / word: which
    Philox block and which of its four words (the kernels: 0, 0).  edge_before_mass: a planted error -- class k is tested
    against the running sum before its own mass is added, which draws the class after the right one."""
    p, s, cum = categorical_probs(z, dtype)
    out_dim = p.shape[1]
    w = philox.philox4x32_10(seed, counters, stream)[word]
    us = philox.u32_to_unit(w).astype(dtype) * s
    edges = cum - p if edge_before_mass else cum
    a = np.minimum((us[:, None] >= edges).sum(1), out_dim - 1)         # edges never decrease: the first k with us < edge_k
    gap = np.abs(us[:, None].astype(np.float64) - cum.astype(np.float64)).min(1)
    return a.astype(np.int64), gap, p, s


def categorical_logp(p, s, a, dtype, clamp=True):
    q = p[np.arange(len(p)), a] / s
    return np.log(np.clip(q, dtype(EPS32), dtype(1.0) - dtype(EPS32)) if clamp else q)


def near_cdf_edge(z64, gap):
    """bool [E]: the rows whose draw lies within the logits' bound of a CDF edge."""
    return np.asarray(gap) < 2.0 * logit_bound(z64).max(1) + 1e-6


def greedy(head, z, slices=(), dtype=np.float64):
    """(greedy action of the logits in `dtype`, rows that may be left out by the near-tie rule).  categorical: the
    argmax, the lowest index on an exact tie; multi_categorical: one per slice; bernoulli: z >= 0 (a bit's |z| against its
    own bound)."""
    z = np.asarray(z, dtype)
    tol = logit_bound(z)
    if head == "bernoulli":
        return (z >= 0).astype(np.float32), (np.abs(z) < tol).any(1)
    acts, near, o = [], np.zeros(len(z), bool), 0
    for n in (slices or (z.shape[1],)):
        zs, t = z[:, o:o + n], tol[:, o:o + n]
        order = np.argsort(-zs, axis=1, kind="stable")
        acts.append(np.argmax(zs, axis=1))
        if n > 1:
            r = np.arange(len(zs))
            i0, i1 = order[:, 0], order[:, 1]
            near |= (zs[r, i0] - zs[r, i1]) < (t[r, i0] + t[r, i1])
        o += n
    a = np.stack(acts, 1)
    return (a if slices else a[:, 0]), near


def gauss_normals(seed, counters, out_dim, dtype, q1_reuses_q0=False):
    """gauss_normals4 of csrc/action_heads.hpp in `dtype`: dimensions 4 q .. 4 q + 3 from the block (seed, counter, q) --
    x an open-0 word and y an angle word give the cos and the sin output, z and w the second pair.  q1_reuses_q0: a
    planted error."""
    z = np.zeros((len(counters), 4 * ((out_dim + 3) // 4)), dtype)
    two_pi = dtype(6.28318530717958647692)
    for q in range((out_dim + 3) // 4):
        w = philox.philox4x32_10(seed, counters, 0 if q1_reuses_q0 else q)
        for pair in (0, 1):
            r = np.sqrt(dtype(-2.0) * np.log(philox.u32_to_unit_open0(w[2 * pair]).astype(dtype)))
            ang = two_pi * philox.u32_to_unit(w[2 * pair + 1]).astype(dtype)
            z[:, 4 * q + 2 * pair], z[:, 4 * q + 2 * pair + 1] = r * np.cos(ang), r * np.sin(ang)
    return z[:, :out_dim]


def gauss_std(log_std, min_std, dtype):
    return np.maximum(np.log1p(np.exp(np.asarray(log_std).astype(dtype))), dtype(min_std))


def unit_to_bounds(a, bounds, dtype):
    """tanh(x) in [-1, 1] -> [lo, hi] (bounds None: the unit box)."""
    if bounds is None:
        return a
    lo, hi = (np.asarray(v).astype(dtype) for v in bounds)
    return ((a + dtype(1.0)) / dtype(2.0)) * (hi - lo) + lo


def squashed_gaussian(mean, sd, raw, bounds, dtype):
    """The raw action's (env action, log-prob) under the tanh-squashed N(mean, sd): 1 - a^2 clamped at 1e-6, every
    dimension's normal log-density at +-100."""
    a = np.tanh(raw)
    slog = np.log(np.maximum(dtype(1.0) - a * a, dtype(1e-6))).sum(1)
    zz = raw - mean
    l = -(zz * zz) / (dtype(2.0) * sd * sd) - np.log(sd) - dtype(0.91893853320467274178)
    return unit_to_bounds(a, bounds, dtype), np.clip(l, dtype(-100.0), dtype(100.0)).sum(1) - slog


def slice_starts(slices):
    return np.concatenate([[0], np.cumsum(slices)[:-1]]).astype(int)


def multi_categorical_probs(z, slices, dtype):
    """-> (p [E, out_dim]: every slice's normalised softmax, s [E, D]: every slice's sum of p), in `dtype`."""
    z = np.asarray(z, dtype)
    p, s = np.zeros_like(z), np.zeros((len(z), len(slices)), dtype)
    for j, (o, n) in enumerate(zip(slice_starts(slices), slices)):
        q = np.exp(z[:, o:o + n] - z[:, o:o + n].max(1, keepdims=True))
        q = q / q.sum(1, keepdims=True)
        p[:, o:o + n], s[:, j] = q, q.sum(1)
    return p, s


def multi_categorical_draw(z, slices, seed, offset, E, dtype, row_shift=0, counter_row_major=False, share_uniform=False,
                           edge_before_mass=False):
    """One inverse-CDF draw per slice -> (action [E, D]: the class's index in its slice, gap [E, D] to the slice's nearest
    CDF edge, p, s).  Slice j of row e draws at counter offset + j E + e + row_shift.  Planted errors: counter_row_major
    (offset + e D + j), share_uniform (every slice of a row takes slice 0's uniform), edge_before_mass (class k tested
    against the running sum before its own mass)."""
    p, s = multi_categorical_probs(z, slices, dtype)
    rows, D = np.arange(len(p)), len(slices)
    a, gap = np.zeros((len(p), D), np.int64), np.zeros((len(p), D))
    for j, (o, n) in enumerate(zip(slice_starts(slices), slices)):
        jj = 0 if share_uniform else j
        index = rows * D + jj if counter_row_major else jj * E + rows
        w = philox.philox4x32_10(seed, philox.counters_u64(offset, index + row_shift), 0)[0]
        us = philox.u32_to_unit(w).astype(dtype) * s[:, j]
        cum = np.cumsum(p[:, o:o + n], 1)
        edges = cum - p[:, o:o + n] if edge_before_mass else cum
        a[:, j] = np.minimum((us[:, None] >= edges).sum(1), n - 1)
        gap[:, j] = np.abs(us[:, None].astype(np.float64) - cum.astype(np.float64)).min(1)
    return a, gap, p, s


def multi_categorical_pick(forced, slices):
    """mcat_pick: every forced index clamped into its slice."""
    f = np.asarray(forced, np.int64).reshape(-1, len(slices))
    return np.clip(f, 0, np.asarray(slices, np.int64)[None, :] - 1)


def multi_categorical_logp(p, s, a, slices, dtype, eps=EPS32, clamp=True, one_is_zero=False):
    """sum_j log(clip(p_a / s, eps, 1 - eps)).  Planted errors: clamp=False; one_is_zero (a slice of one class adds 0)."""
    rows, lp = np.arange(len(p)), np.zeros(len(p), dtype)
    for j, (o, n) in enumerate(zip(slice_starts(slices), slices)):
        if one_is_zero and n == 1:
            continue
        q = p[rows, o + a[:, j]] / s[:, j]
        lp = lp + np.log(np.clip(q, dtype(eps), dtype(1.0) - dtype(eps)) if clamp else q)
    return lp


def near_slice_edge(z64, gap):
    """bool [E, D]: the slices whose draw lies within the logits' bound of a CDF edge (near_cdf_edge's rule per slice)."""
    return np.asarray(gap) < (2.0 * logit_bound(z64).max(1) + 1e-6)[:, None]


def sigmoid(z, dtype):
    z = np.asarray(z, dtype)
    return dtype(1.0) / (dtype(1.0) + np.exp(-z))


def bernoulli_draw(z, seed, counters, dtype, words_reversed=False, block0_again=False):
    """-> (bits [E, n] float32, gap [E, n] = |u_d - sigmoid(z_d)|, p = sigmoid(z)).  counters: [E], or [E, n] (one per
    bit -- the planted counter offset + e n + d).  Planted errors: words_reversed (word 3 - d % 4), block0_again (bits
    4 .. 7 from stream 0 again)."""
    p = sigmoid(z, dtype)
    E, n = p.shape
    counters = np.asarray(counters, np.uint64)
    counters = np.broadcast_to(counters[:, None] if counters.ndim == 1 else counters, (E, n))
    u = np.zeros((E, n))
    for d in range(n):
        w = philox.philox4x32_10(seed, np.ascontiguousarray(counters[:, d]), 0 if block0_again else d // 4)
        u[:, d] = philox.u32_to_unit(w[3 - d % 4 if words_reversed else d % 4])
    bits = (u.astype(dtype) < p).astype(np.float32)
    return bits, np.abs(u - p.astype(np.float64)), p


def bernoulli_logp(z, a, dtype, eps=EPS32, clamp=True):
    """-sum_d BCEWithLogits(l_d, a_d), l = log q - log1p(-q), q = clip(sigmoid z, eps, 1 - eps) (torch's Bernoulli(probs)),
    BCEWithLogits(l, t) = (1 - t) l - log sigmoid(l).  clamp=False: a planted error."""
    p = sigmoid(z, dtype)
    q = np.clip(p, dtype(eps), dtype(1.0) - dtype(eps)) if clamp else p
    with np.errstate(divide="ignore"):
        l = np.log(q) - np.log1p(-q)
    a = np.asarray(a).astype(dtype)
    bce = (dtype(1.0) - a) * l - (np.minimum(l, dtype(0.0)) - np.log1p(np.exp(-np.abs(l))))
    return -bce.sum(1)


def near_bernoulli_edge(z64, gap):
    """bool [E, n]: the bits whose uniform lies within the logit's bound, carried through sigmoid, of the probability."""
    return np.asarray(gap) < 0.25 * logit_bound(z64) + 1e-6
