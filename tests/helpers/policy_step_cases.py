"""
ONE launch of K6+K7 (csrc/policy_step.hip: ppoaf_policy_step / ppoaf_policy_step_blocks) restated in numpy in a chosen
dtype, and the cases of tests/test_gpu_policy_step_float64.py built on it (no device): tests/test_policy_step_oracle.py
shows with the same cases that every planted error is caught by one of them and that the float32 restatement stays inside
every bound and cap.

The step, restated (launch_reference; step_reference(case, dtype) is a case's sampled launch), from two eval_kernels.Net
in one bucket (per Linear the weight [out, in], then the bias, each padded to 4 floats; log_std behind the actor's layers):
  * the actor's MLP on `obs`, the critic's on `critic_obs` (an in_dim, a width and a depth of its own);
  * the value: the critic's output v, or mean + v sqrt(var + 1e-8) (normalize_values);
  * the head on the actor's outputs (tests/helpers/head_draws.py), sampled or forced:
      Categorical    row e at Philox counter offset + e: the inverse-CDF draw, or the forced class clamped into
                     [0, out_dim - 1]; log(clip(p_a / s, eps32, 1 - eps32));
      Gaussian       raw = mean + sd z (Box-Muller pairs of block q = d / 4 at counter offset + e), sd =
                     max(softplus(log_std), min_std), or the forced raw action; tanh, the rescale to per-dimension bounds,
                     the squashed log-prob (1 - a^2 clamped at 1e-6, every dimension's density at +-100);
      MultiDiscrete  slice j of row e at counter offset + j E + e, one inverse-CDF draw per slice, or the forced indices
                     clamped into their slices; the slices' clamped log-probs summed;
      MultiBinary    bit d = u_d < sigmoid(z_d), u_d word d % 4 of block (seed, offset + e, stream d / 4), or the forced
                     bits as given; Bernoulli(probs = sigmoid z)'s log-prob, the probability clamped to [eps32, 1 - eps32];
  * raw_action_out == action_out for the three discrete heads; the two observation copies are the inputs.
min_std is the float32 the launch is handed (0.01f), in every dtype.

NEAR TIES: head_draws.near_cdf_edge (Categorical), near_slice_edge (any slice of the row), near_bernoulli_edge (any bit
of the row); at most mat_step_cases.cap(E) rows of a case's sampled launch may be near a tie, and never all rows unless
E = 1 -- a condition of the case, met by the choice of its seed (tests/test_policy_step_oracle.py), not a measurement.
Gaussian outputs, values and the forced launch leave nothing out.

A case's steering: both networks drawn by eval_kernels.Net (weights N(0, 1) / sqrt(fan-in), biases 0.1 N(0, 1), log_std
U(-1.5, 0)); observations N(0, 1) rounded to float32, a row whose ReLU / LeakyReLU pre-activation lies within 1e-4 of its
row's scale of zero (oracle.k12_oracle.kinked_rows) drawn again; the actor's output layer then scaled so that the
float64 logits have a root mean square of 1.5 (the default initialisation's head gain leaves every distribution near
uniform) -- times `saturate` where some class probabilities shall fall below float32's eps; `floor`: log_std = -8 on one
dimension (softplus = 3.4e-4 < min_std); `pm20`: bits 0 and 1 of a MultiBinary head at logits +20 / -20 whatever the
row; value statistics (0.3, 0.25) on every other case; bounds lo_d = -1 - d / 2, hi_d = 2 + d / 4.
The forced launch replays the float64 draw with
  Categorical / MultiDiscrete  one index below 0 and one at or above its slice's classes (clamped); saturated cases: the
                               rarest class wherever it lies safely below eps32 (log eps32 by the clamp);
  Gaussian                     |raw| in 3.8 .. 4.2 in the first rows, one row at |raw| = 9 (1 - a^2 below its clamp), on a
                               `floor` case one row 20 sd from the mean on the floored dimension (density below -100);
  MultiBinary                  a quarter of the bits flipped; `pm20`: rows that log the bit the +-20 logit excludes.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import k12_oracle as ko

import eval_kernels as ek
import head_draws as hd
import philox
from mat_step_cases import cap, k12_bound, worst  # noqa: F401  (the project's bound rule and cap, one copy)

EPS32 = hd.EPS32
VN = (0.3, 0.25)
MIN_STD = float(np.float32(0.01))
CAT, GAU, MCAT, BERN = "categorical", "gaussian", "multi_categorical", "bernoulli"
DISCRETE = (CAT, MCAT, BERN)
WIDTH_PAIRS = ((32, 32), (64, 64), (128, 128), (256, 256), (128, 256), (64, 128), (64, 256), (32, 256), (32, 64), (256, 512))
LDS_LIMIT = 160 * 1024


class Planted(NamedTuple):
    """Errors planted by the sharpness tests (tests/test_policy_step_oracle.py), never set otherwise."""
    tile_minus_4: bool = False            # tile g >= 4 reads the rows of tile g - 4
    counter_plus_one: bool = False        # row e draws at offset + e + 1
    mcat_counter_row_major: bool = False  # slice j of row e draws at offset + e D + j
    mcat_share_uniform: bool = False      # every slice of a row takes slice 0's uniform
    mcat_vector_index: bool = False       # the action reported as the class's index in the whole output vector
    mcat_one_is_zero: bool = False        # a slice of one class adds 0 to the log-prob
    mcat_edge_before_mass: bool = False   # the CDF edge taken before the class's mass
    bern_words_reversed: bool = False     # bit d from word 3 - d % 4
    bern_counter_per_bit: bool = False    # bit d of row e at counter offset + e n + d
    bern_block0_again: bool = False       # bits 4 .. 7 from block 0 again
    logp_no_clamp: bool = False           # no [eps32, 1 - eps32] clamp in the three discrete log-probs
    no_min_std: bool = False              # sd = softplus(log_std), no floor
    bounds_swapped: bool = False          # lo and hi swapped
    denorm_var: bool = False              # mean + v var in place of mean + v sqrt(var + 1e-8)
    critic_reads_actor_obs: bool = False  # the critic's rows read from the actor's observation tensor
    copy_shifted: bool = False            # the observation copies shifted by one row
    forced_no_clamp: bool = False         # a forced class outside its slice written as it came


def lds_floats(in_dim, hidden, depth):
    """mlp_rows_forward_lds_floats (csrc/mlp_device.hpp) of one network."""
    hs, inp = hidden + 4, 16 * ((in_dim + 15) // 16) + 4
    return (depth + 1) * hidden + 8 * hidden + 16 * inp + 2 * 16 * hs + 16 * 16


def lds_bytes(actor, critic):
    """step_lds_bytes (csrc/policy_step.hip): the larger network's need, rounded up to 16 bytes."""
    worst_ = max(4 * lds_floats(n.in_dim, n.hidden, n.depth) for n in (actor, critic))
    return (worst_ + 15) // 16 * 16


def ko_net(net):
    return ko.Net(net.in_dim, net.hidden, net.depth, net.out_dim, net.act)


def bounds_of(out_dim):
    d = np.arange(out_dim)
    return (-1.0 - 0.5 * d).astype(np.float32), (2.0 + 0.25 * d).astype(np.float32)


def launch_reference(actor, critic, head, slices, obs, cobs, seed, offset, forced=None, vn=None, bounds=None,
                     dtype=np.float64, planted=Planted(), eps=EPS32):
    """One launch -> dict of numpy arrays computed in `dtype`: logits [E, out_dim] (Gaussian: the means); raw / action
    (what raw_action_out / action_out hold: Categorical [E] int64, MultiDiscrete [E, D] int64, MultiBinary [E, n] and
    Gaussian [E, out_dim] float64); drawn (the draw, also where a forced action overrides it); gap (Categorical [E],
    MultiDiscrete [E, D], MultiBinary [E, n]: to the nearest edge); probs (the discrete heads); logp [E]; value [E] and
    value_raw [E] (the critic's own output); obs_copy / cobs_copy.  eps: the log-prob clamp of the MultiDiscrete and
    MultiBinary heads (float32's, as the kernel's; float64's for the comparison with torch.distributions)."""
    pl = planted
    obs, cobs = np.asarray(obs, np.float32), np.asarray(cobs, np.float32)
    E, O = len(obs), actor.out_dim
    rows = np.arange(E)
    src = rows.copy()
    if pl.tile_minus_4:
        src[64:] -= 64
    z = actor.forward(obs[src], dtype)
    cin = np.resize(obs.reshape(-1), (E, critic.in_dim)) if pl.critic_reads_actor_obs else cobs   # (at the critic's stride)
    v = critic.forward(cin[src], dtype)[:, 0]
    r = dict(logits=z.astype(np.float64), value_raw=v.astype(np.float64))
    if vn is not None:
        mean, var = dtype(vn[0]), dtype(vn[1])
        v = mean + v * (var if pl.denorm_var else np.sqrt(var + dtype(1e-8)))
    r["value"] = v.astype(np.float64)
    shift = np.roll if pl.copy_shifted else (lambda x, *_: x)
    r["obs_copy"], r["cobs_copy"] = shift(obs, 1, 0), shift(cobs, 1, 0)
    plus = 1 if pl.counter_plus_one else 0
    counters = philox.counters_u64(offset, rows + plus)
    clamp = not pl.logp_no_clamp
    if head == CAT:
        a, gap, p, s = hd.categorical_draw(z, seed, counters, dtype)
        r["drawn"], r["gap"], r["probs"] = a, gap, p.astype(np.float64)
        written = a
        if forced is not None:
            written = np.asarray(forced, np.int64).reshape(E)
            a = np.clip(written, 0, O - 1)
            if not pl.forced_no_clamp:
                written = a
        r["raw"] = r["action"] = written
        r["logp"] = hd.categorical_logp(p, s, a, dtype, clamp).astype(np.float64)
    elif head == MCAT:
        a, gap, p, s = hd.multi_categorical_draw(z, slices, seed, offset, E, dtype, plus, pl.mcat_counter_row_major,
                                                 pl.mcat_share_uniform, pl.mcat_edge_before_mass)
        r["drawn"], r["gap"], r["probs"] = a, gap, p.astype(np.float64)
        written = a
        if forced is not None:
            written = np.asarray(forced, np.int64).reshape(E, len(slices))
            a = hd.multi_categorical_pick(written, slices)
            if not pl.forced_no_clamp:
                written = a
        if pl.mcat_vector_index:
            written = written + hd.slice_starts(slices)[None, :]
        r["raw"] = r["action"] = written
        r["logp"] = hd.multi_categorical_logp(p, s, a, slices, dtype, eps, clamp, pl.mcat_one_is_zero).astype(np.float64)
    elif head == BERN:
        if pl.bern_counter_per_bit:
            counters = philox.counters_u64(offset, rows[:, None] * O + np.arange(O)[None, :] + plus)
        a, gap, p = hd.bernoulli_draw(z, seed, counters, dtype, pl.bern_words_reversed, pl.bern_block0_again)
        r["drawn"], r["gap"], r["probs"] = a.astype(np.float64), gap, p.astype(np.float64)
        if forced is not None:
            a = np.asarray(forced, np.float32).reshape(E, O)
        r["raw"] = r["action"] = a.astype(np.float64)
        with np.errstate(invalid="ignore"):
            r["logp"] = hd.bernoulli_logp(z, a, dtype, eps, clamp).astype(np.float64)
    else:
        sd = hd.gauss_std(actor.log_std, 0.0 if pl.no_min_std else MIN_STD, dtype)
        drawn = z + sd * hd.gauss_normals(seed, counters, O, dtype)
        raw = drawn if forced is None else np.asarray(forced, np.float32).reshape(E, O).astype(dtype)
        box = bounds if (bounds is None or not pl.bounds_swapped) else (bounds[1], bounds[0])
        act, logp = hd.squashed_gaussian(z, sd, raw, box, dtype)
        r["drawn"], r["gap"], r["sd"] = drawn.astype(np.float64), np.zeros(E), sd.astype(np.float64)
        r["raw"], r["action"], r["logp"] = raw.astype(np.float64), act.astype(np.float64), logp.astype(np.float64)
    return r


def near_rows(head, r64):
    """bool [E]: the rows of a sampled float64 launch that lie near a tie."""
    z, gap = r64["logits"], r64["gap"]
    if head == CAT:
        return hd.near_cdf_edge(z, gap)
    if head == MCAT:
        return hd.near_slice_edge(z, gap).any(1)
    if head == BERN:
        return hd.near_bernoulli_edge(z, gap).any(1)
    return np.zeros(len(z), bool)


# ------------------------------------------------------------------------------------------------------------ cases
def case(E, pair, Ia, Ic, Da, Dc, act, head, seed, slices=(), bounds=False, offset=None, saturate=0.0, floor=False,
         pm20=False, copies=True):
    kind, O = head
    assert kind != MCAT or sum(slices) == O
    return dict(E=E, Ha=pair[0], Hc=pair[1], Ia=Ia, Ic=Ic, Da=Da, Dc=Dc, act=act, head=kind, O=O, slices=tuple(slices),
                seed=seed, bounds=bounds, offset=977 * seed + (seed << 33) if offset is None else offset, saturate=saturate,
                floor=floor, pm20=pm20, copies=copies)


WRAP = 2 ** 32 - 7                        # the counter's low word wraps inside the launch
CASES = {
    # ---- Categorical
    "cat2_e1_32x32": case(1, (32, 32), 1, 1, 1, 1, "relu", (CAT, 2), 1),                               # every lower limit
    "cat5_e17_wrap_64x64": case(17, (64, 64), 17, 34, 2, 2, "tanh", (CAT, 5), 2, offset=WRAP),
    "cat8_e65_64x64": case(65, (64, 64), 16, 48, 3, 3, "leaky_relu", (CAT, 8), 3),                     # tile 4: second group
    "cat5_sat_e16_128x128": case(16, (128, 128), 15, 15, 2, 2, "relu", (CAT, 5), 4, saturate=10.0),
    "cat8_e129_32x256": case(129, (32, 256), 33, 65, 1, 3, "tanh", (CAT, 8), 5),                       # tile 8: third group
    "cat2_lds_in376_256x256": case(15, (256, 256), 376, 376, 2, 2, "relu", (CAT, 2), 6),               # > 64 KB of LDS
    # ---- Gaussian
    "gau1_e16_64x128": case(16, (64, 128), 64, 64, 2, 2, "tanh", (GAU, 1), 7, copies=False),
    "gau3_floor_e15_128x256": case(15, (128, 256), 16, 32, 2, 1, "leaky_relu", (GAU, 3), 8, bounds=True, floor=True),
    "gau4_e63_wrap_32x64": case(63, (32, 64), 15, 45, 4, 4, "relu", (GAU, 4), 9, bounds=True, offset=WRAP),
    "gau5_e129_128x256": case(129, (128, 256), 65, 17, 1, 2, "tanh", (GAU, 5), 10),                    # a second Philox block
    "gau8_e65_256x512": case(65, (256, 512), 33, 66, 2, 2, "leaky_relu", (GAU, 8), 11, bounds=True),
    "gau4_depth7_e17_64x256": case(17, (64, 256), 1, 3, 7, 7, "tanh", (GAU, 4), 12),
    # ---- MultiDiscrete
    "md32_e15_32x32": case(15, (32, 32), 16, 16, 1, 1, "relu", (MCAT, 5), 13, slices=(3, 2), copies=False),
    "md2222_e17_wrap_64x128": case(17, (64, 128), 17, 51, 3, 2, "tanh", (MCAT, 8), 14, slices=(2, 2, 2, 2), offset=WRAP),
    "md17_e129_32x64": case(129, (32, 64), 33, 33, 2, 2, "leaky_relu", (MCAT, 8), 15, slices=(1, 7)),
    "md8_sat_e16_256x256": case(16, (256, 256), 15, 30, 1, 1, "tanh", (MCAT, 8), 16, slices=(8,), saturate=10.0),
    "md1x8_e63_128x128": case(63, (128, 128), 64, 64, 2, 2, "relu", (MCAT, 8), 17, slices=(1,) * 8),
    "md44_e16_wrap_between_64x256": case(16, (64, 256), 65, 65, 4, 4, "leaky_relu", (MCAT, 8), 18, slices=(4, 4),
                                         offset=2 ** 32 - 16),                                         # slice 1 starts at the wrap
    # ---- MultiBinary
    "mb1_e15_32x256": case(15, (32, 256), 15, 15, 2, 2, "relu", (BERN, 1), 19),
    "mb4_e63_64x64": case(63, (64, 64), 33, 99, 1, 1, "leaky_relu", (BERN, 4), 20),
    "mb5_e17_wrap_256x256": case(17, (256, 256), 16, 16, 3, 3, "tanh", (BERN, 5), 21, offset=WRAP),
    "mb8_e65_64x128": case(65, (64, 128), 17, 34, 2, 2, "relu", (BERN, 8), 22),
    "mb8_pm20_e16_32x64": case(16, (32, 64), 64, 128, 2, 2, "tanh", (BERN, 8), 23, pm20=True),
    "mb5_lds_limit_e15_256x512": case(15, (256, 512), 33, 1000, 2, 6, "tanh", (BERN, 5), 24),          # 1280 B under 160 KB
}
for _i, _c in enumerate(CASES.values()):
    _c["norm_values"] = bool(_i & 1)

BLOCK_CASES = ("cat8_e65_64x64", "gau5_e129_128x256", "md17_e129_32x64", "mb8_e65_64x128", "gau8_e65_256x512",
               "cat8_e129_32x256")
BLOCK_SHAPES = {65: (13, 5), 129: (43, 3)}            # E -> (rows per block, blocks)
# a critic refused on the host: 768 B over the limit
OVER_LDS = dict(pair=(256, 512), Ia=16, Ic=993, Da=1, Dc=7)
LAUNCHES = ("sampled", "forced")


def draw_nets(c, rng):
    actor = ek.Net(rng, c["Ia"], c["Ha"], c["Da"], c["O"], c["act"], log_std=c["head"] == GAU)
    critic = ek.Net(rng, c["Ic"], c["Hc"], c["Dc"], 1, c["act"])
    return actor, critic


def draw_observations(actor, critic, E, rng):
    """N(0, 1) rows rounded to float32; a row with a pre-activation at a ReLU / LeakyReLU kink is drawn again."""
    obs = rng.normal(0, 1, (E, actor.in_dim)).astype(np.float32)
    cobs = rng.normal(0, 1, (E, critic.in_dim)).astype(np.float32)
    for _ in range(200):
        bad = ko.kinked_rows(ko_net(actor), actor.flat(), obs) | ko.kinked_rows(ko_net(critic), critic.flat(), cobs)
        if not bad.any():
            return obs, cobs
        obs[bad] = rng.normal(0, 1, (int(bad.sum()), actor.in_dim)).astype(np.float32)
        cobs[bad] = rng.normal(0, 1, (int(bad.sum()), critic.in_dim)).astype(np.float32)
    raise AssertionError("observations without a kinked row were not found")


def steer(actor, obs, rms=1.5, saturate=0.0, floor=False, pm20=False):
    """The actor's output layer scaled so that the float64 outputs of `obs` have the root mean square `rms`."""
    z = actor.forward(obs)
    g = rms / np.sqrt((z * z).mean()) * (saturate or 1.0)
    W, b = actor.layers[-1]
    W, b = (W.astype(np.float64) * g).astype(np.float32), (b.astype(np.float64) * g).astype(np.float32)
    if pm20:
        W[:2], b[:2] = 0.0, (20.0, -20.0)
    actor.layers[-1] = (W, b)
    if floor:
        actor.log_std[actor.out_dim - 1] = -8.0


class Steering:
    """A case's inputs and the float64 / float32 references of its launches (self.ref[launch] = (r64, r32))."""

    def __init__(self, c):
        self.c = c
        E, O = c["E"], c["O"]
        self.head, self.slices = c["head"], c["slices"]
        rng = np.random.default_rng(c["seed"])
        self.actor, self.critic = draw_nets(c, rng)
        self.obs, self.cobs = draw_observations(self.actor, self.critic, E, rng)
        steer(self.actor, self.obs, saturate=c["saturate"], floor=c["floor"], pm20=c["pm20"])
        self.seed, self.offset = 0x1234ABCD5678 + c["seed"], c["offset"]
        self.vn = VN if c["norm_values"] else None
        self.bounds = bounds_of(O) if c["bounds"] else None
        r64 = self.reference("sampled", np.float64)
        self.near = dict(sampled=near_rows(self.head, r64), forced=np.zeros(E, bool))
        self.forced, self.marked = self._forced(r64, rng)
        self.ref = {}
        for launch in LAUNCHES:
            self.ref[launch] = (r64 if launch == "sampled" else self.reference(launch, np.float64),
                                self.reference(launch, np.float32))

    def _forced(self, r64, rng):
        """-> (the forced raw actions, {regime: bool [E] rows (Categorical, Gaussian) or [E, .] entries in it})."""
        c, E, O, head = self.c, self.c["E"], self.c["O"], self.head
        marked = {}
        if head in (CAT, MCAT):
            f = r64["drawn"].copy().reshape(E, -1)
            n_last = O if head == CAT else self.slices[-1]
            o_last = O - n_last
            f[-1, -1] = n_last + 2
            if E > 1:
                f[0, 0] = -3
            if c["saturate"]:
                # the last slice's rarest class wherever it lies safely below eps32 (the two clamped entries stay)
                p = r64["probs"][:, o_last:]
                rare = p.min(1) < 0.5 * EPS32
                rare[[0, -1]] = False
                f[rare, -1] = p.argmin(1)[rare]
                marked["saturated"] = rare
            return (f.reshape(E) if head == CAT else f), marked
        if head == GAU:
            f = r64["drawn"].astype(np.float32)
            k = max(1, E // 8)
            f[:k] = (np.where(f[:k] < 0, -1.0, 1.0) * rng.uniform(3.8, 4.2, f[:k].shape)).astype(np.float32)
            f[k] = np.where(f[k] < 0, -9.0, 9.0)
            marked["tanh_clamped"] = np.arange(E) == k
            if c["floor"]:
                f[k + 1, O - 1] = np.float32(r64["logits"][k + 1, O - 1] + 0.2)
                marked["density_clamped"] = np.arange(E) == k + 1
            return f, marked
        f = r64["drawn"].astype(np.float32)
        flip = rng.random(f.shape) < 0.25
        if c["pm20"]:
            flip[:, :2] = False
            flip[0, 0] = flip[1, 1] = flip[2, 0] = flip[2, 1] = True     # the bit its +-20 logit excludes
            marked["excluded_bit"] = flip & (np.arange(O)[None, :] < 2)
        return np.where(flip, 1.0 - f, f).astype(np.float32), marked

    def reference(self, launch, dtype, eps=EPS32, **planted):
        forced = self.forced if launch == "forced" else None
        return launch_reference(self.actor, self.critic, self.head, self.slices, self.obs, self.cobs, self.seed, self.offset,
                                forced, self.vn, self.bounds, dtype, Planted(**planted), eps)

    def params(self):
        """The bucket: the actor's segment (log_std last), then the critic's."""
        return np.concatenate([self.actor.flat(), self.critic.flat()])

    def left_out(self, launch):
        return int(self.near[launch].sum())


@functools.lru_cache(maxsize=None)
def steering(name):
    return Steering(CASES[name])


def step_reference(case, dtype=np.float64):
    """The sampled launch of a case (a name of CASES, or a case dict) restated in `dtype`."""
    s = steering(case) if isinstance(case, str) else Steering(case)
    return s.reference("sampled", dtype)


def _exact(got, want):
    """0 when bitwise the wanted values (float32 / int64 values held in float64), inf otherwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return 0.0 if got.shape == want.shape and np.array_equal(got, want) else float("inf")


def judge(s, got, launch):
    """A launch's outputs (raw, action, logp, value, obs_copy, cobs_copy; the copies may be missing) -- or a planted
    reference's dict -- under the GPU test's rules -> (number of compared rows whose action differs, {tensor: worst
    deviation / bound; inf where a tensor that must be exact is not}).
      sampled   discrete heads: action equal on the kept rows, raw == action on every row; Gaussian: raw and action by
                bound on every row; logp by bound on the kept rows; value by bound on every row; the copies exact;
      forced    every row compared; raw exact: the forced tensor, the discrete indices clamped."""
    r64, r32 = s.ref[launch]
    kept = ~s.near[launch]
    fr, wrong = {}, 0
    cmp = lambda k, mask=None: fr.__setitem__(k, worst(got[k], r64[k], r32[k], mask))
    if s.head in DISCRETE:
        ga, gr, wa = (np.asarray(x).reshape(len(kept), -1) for x in (got["action"], got["raw"], r64["action"]))
        wrong = int(((ga != wa).any(1) & kept).sum()) + int((gr != ga).any(1).sum())
    else:
        if launch == "forced":
            fr["raw"] = _exact(got["raw"], r64["raw"])
        else:
            cmp("raw")
        cmp("action")
    cmp("logp", kept)
    cmp("value")
    for k in ("obs_copy", "cobs_copy"):
        if got.get(k) is not None:
            fr[k] = _exact(got[k], r64[k])
    return wrong, fr
