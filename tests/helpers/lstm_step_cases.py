"""
ONE launch of K21 (csrc/lstm_policy_step.hip) restated on torch-CPU in a chosen dtype, and the cases of
tests/test_gpu_lstm_step_float64.py built on it (no device): tests/test_lstm_step_oracle.py shows with the same cases that
every planted error is caught by one of them and that the float32 restatement stays inside every bound and cap.

The step, restated (step_reference), from a parameter bucket in K18's layout (oracle.lstm_update_oracle.bucket_tables):
  * each network once: (out, h', c') = _Module.forward(x[:, None, :], h, c) of oracle/lstm_update_oracle.py -- one LSTM
    step (gate order i, f, g, o; b_ih + b_hh), LayerNorm(eps 1e-5) of the NEW h, activation, the feed-forward layers;
    the actor on the observations, the critic on the critic observations, each from its own (h, c);
  * the value: the critic's output as it is, or mean + v sqrt(var + 1e-8) (normalize_values);
  * the head on the actor's output, row e at Philox counter offset + e (tests/helpers/head_draws.py): the Categorical
    inverse-CDF draw -- or the forced class clamped into [0, out_dim - 1] -- with log(clip(p_a / s, eps32, 1 - eps32)),
    or the Gaussian raw = mean + sd z (Box-Muller pairs of block q = d / 4) -- or the forced raw action --, tanh, the
    rescale to the bounds and the squashed log-prob;
  * the state the launch leaves: (h', c') of both networks, in place and again in the step's four stored rows.
next_reference: CRITIC_NEXT -- V(next critic observation), the critic's (h', c') kept only when `commit` is set, the four
stored rows of the terminated rows zeroed.  INFER is the actor's half of the step: its env action is the draw's
(sampled) or argmax z / tanh(mean) rescaled (greedy).

NEAR TIES: head_draws.near_cdf_edge for a sampled Categorical row, head_draws.greedy's mask for a greedy one; at most
mat_step_cases.cap(E) rows of a case and launch may be near a tie -- a condition of the case, met by the choice of its
seed (tests/test_lstm_step_oracle.py), not a measurement.  Gaussian outputs, values and states leave nothing out.

A case's steering: the bucket drawn as lstm_update_cases.draw_params draws it (logits of O(1), non-zero biases, an affine
LayerNorm, log_std ~ N(0, 0.3); small_h: output-gate biases of -2.5 + -2.5, LayerNorm rows of variance ~1e-4), observations
N(0, 1) -- three of them, for a chain of three steps --, states 0.5 N(0, 1), all rounded to float32; value statistics
(0.3, 0.25) on every other case; bounds (-2, 3) where the case says so.  `saturate`: the actor's last Linear multiplied
so that some class probabilities fall below float32's eps -- the forced launch then logs such classes (log eps32 by the
clamp).  The forced launch replays the float64 draw with one class below 0 and one at or above out_dim (Categorical) or
with |raw| in 3.8 .. 4.2 in the first rows (Gaussian).
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

from oracle import lstm_update_oracle as lo

import head_draws as hd
import philox
from mat_step_cases import cap, k12_bound, worst  # noqa: F401  (the project's bound rule and cap, one copy)

EPS32 = hd.EPS32
VN = (0.3, 0.25)
BOUNDS = (-2.0, 3.0)
MIN_STD = 0.01
STATES = ("actor_h", "actor_c", "critic_h", "critic_c")
STORED = tuple("stored_" + k for k in STATES)
CAT, GAU = "categorical", "gaussian"


class Planted(NamedTuple):
    """Errors planted by the sharpness tests (tests/test_lstm_step_oracle.py), never set otherwise."""
    counter_plus_one: bool = False        # row e draws at offset + e + 1
    counter_tile_local: bool = False      # row e draws at offset + e % 16
    cat_stream_1: bool = False            # the Categorical draw from Philox stream 1
    cat_word_y: bool = False              # the Categorical draw from word y of the block
    gauss_q1_reuses_q0: bool = False      # dimensions 4 .. 7 from block q = 0 again
    cdf_edge_before_mass: bool = False    # the class after the right one at every CDF edge
    gate_order: bool = False              # the gate blocks read as i, g, f, o
    drop_b_hh: bool = False
    ln_eps_1e6: bool = False
    head_reads_old_h: bool = False        # LayerNorm of the h the step started from
    stored_swapped: bool = False          # the stored hidden and cell rows swapped
    critic_reads_actor_obs: bool = False  # the critic's rows read from the actor's observation tensor
    denorm_var: bool = False              # mean + v var in place of mean + v sqrt(var + 1e-8)
    no_rescale: bool = False              # the env action left in the unit box
    forced_no_clamp: bool = False         # a forced class outside [0, out_dim - 1] written as it came
    tile_minus_4: bool = False            # tile g >= 4 reads the rows of tile g - 4
    ignore_commit: bool = False           # CRITIC_NEXT keeps the critic's stepped state whatever `commit` says
    terminated_shifted: bool = False      # row n zeroed for the byte of row n - 1


def _np(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def _segment(net, seg, pl):
    """The network's segment as a planted kernel would read it."""
    seg = np.array(seg, dtype=np.float64)
    H = net.hidden
    for name, off, shape in lo.tensor_table(net)[0]:
        n = int(np.prod(shape))
        if pl.gate_order and name in ("w_ih", "w_hh", "b_ih", "b_hh"):
            t = seg[off:off + n].reshape((4, H) + tuple(shape[1:])).copy()
            t[[1, 2]] = t[[2, 1]]
            seg[off:off + n] = t.reshape(-1)
        if pl.drop_b_hh and name == "b_hh":
            seg[off:off + n] = 0.0
    return seg


def net_step(net, seg, x, h0, c0, dtype, pl=Planted()):
    """One step of one network -> (out [E, out_dim], h' [E, H], c' [E, H]) as torch tensors of `dtype`."""
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    x, h0, c0 = np.asarray(x), np.asarray(h0), np.asarray(c0)
    if pl.tile_minus_4:
        src = np.arange(len(x))
        src[64:] -= 64
        x, h0, c0 = x[src], h0[src], c0[src]
    m = lo._Module(net, _segment(net, seg, pl), dtype, 1e-6 if pl.ln_eps_1e6 else 1e-5)
    with torch.no_grad():
        out, h, c, _ = m(T(x)[:, None, :], T(h0), T(c0))
        if pl.head_reads_old_h:
            y = m.act(m.layer_norm(T(h0)))
            for layer in m.ff[:-1]:
                y = m.act(layer(y))
            out = m.ff[-1](y)
    return out, h, c


def _values(out, vn, dtype, pl):
    v = out[:, 0]
    raw = v.double().numpy().copy()
    if vn is not None:
        mean, var = (torch.tensor(s, dtype=dtype) for s in vn)
        v = mean + v * (var if pl.denorm_var else torch.sqrt(var + torch.tensor(1e-8, dtype=dtype)))
    return v.double().numpy().copy(), raw


def _critic_obs(obs, cobs, critic, pl):
    if not pl.critic_reads_actor_obs:
        return cobs
    return np.resize(np.asarray(obs).reshape(-1), (len(cobs), critic.in_dim))     # the actor's tensor at the critic's stride


def step_reference(params, actor, critic, head, obs, cobs, state, seed, offset, forced=None, vn=None, bounds=None,
                   dtype=torch.float64, planted=Planted()):
    """One STEP launch -> dict of float64 numpy computed in `dtype`: actor_h / actor_c / critic_h / critic_c [E, H] (the
    states it leaves) and stored_* (the step's four rows); logits [E, out_dim] (Gaussian: the means); actions (Categorical
    [E] int64: the draw, or the forced class clamped; Gaussian [E, out_dim]: the raw action, drawn or forced); drawn (the
    draw, also where a forced action overrides it); gap [E] (Categorical: to the nearest CDF edge); raw (what raw_action_out
    holds: == actions); env_action (action_out: the class, or tanh(raw) rescaled); logp [E]; values [E] and values_raw [E]
    (the critic's own output); greedy (INFER's deterministic env action: argmax z, or tanh(mean) rescaled)."""
    pl, npdt = planted, _np(dtype)
    na = lo.tensor_table(actor, head == GAU)[1]
    params = np.asarray(params, np.float64)
    E, O = len(obs), actor.out_dim
    out, ah, ac = net_step(actor, params[:na], obs, state[0], state[1], dtype, pl)
    val, ch, cc = net_step(critic, params[na:], _critic_obs(obs, cobs, critic, pl), state[2], state[3], dtype, pl)
    n64 = lambda t: t.double().numpy().copy()
    r = dict(zip(STATES, (n64(ah), n64(ac), n64(ch), n64(cc))))
    for k in STATES:
        r["stored_" + k] = r[k]
    if pl.stored_swapped:
        for w in ("actor", "critic"):
            r[f"stored_{w}_h"], r[f"stored_{w}_c"] = r[f"{w}_c"], r[f"{w}_h"]
    r["values"], r["values_raw"] = _values(val, vn, dtype, pl)
    z = out.numpy().astype(npdt)
    r["logits"] = z.astype(np.float64)
    rows = np.arange(E)
    index = rows % 16 if pl.counter_tile_local else rows + 1 if pl.counter_plus_one else rows
    counters = philox.counters_u64(offset, index)
    box = None if (bounds is None or pl.no_rescale) else tuple(np.full(O, b, np.float32) for b in bounds)
    if head == CAT:
        a, gap, p, s = hd.categorical_draw(z, seed, counters, npdt, 1 if pl.cat_stream_1 else 0, 1 if pl.cat_word_y else 0,
                                           pl.cdf_edge_before_mass)
        r["drawn"], r["gap"] = a, gap
        written = a
        if forced is not None:
            written = np.asarray(forced, np.int64).reshape(E)
            a = np.clip(written, 0, O - 1)
            if not pl.forced_no_clamp:
                written = a
        r["actions"] = r["raw"] = r["env_action"] = written
        r["logp"] = hd.categorical_logp(p, s, a, npdt).astype(np.float64)
        r["probs"] = p.astype(np.float64)
        r["greedy"] = hd.greedy(CAT, z, dtype=npdt)[0]
    else:
        at = lo.tensor_table(actor, True)[0][-1][1]                            # log_std: behind the actor's last bias
        log_std = params[at:at + O]
        sd = hd.gauss_std(log_std, MIN_STD, npdt)
        drawn = z + sd * hd.gauss_normals(seed, counters, O, npdt, pl.gauss_q1_reuses_q0)
        raw = drawn if forced is None else np.asarray(forced).reshape(E, O).astype(npdt)
        act, logp = hd.squashed_gaussian(z, sd, raw, box, npdt)
        r["drawn"], r["gap"] = drawn.astype(np.float64), np.zeros(E)
        r["actions"] = r["raw"] = raw.astype(np.float64)
        r["env_action"], r["logp"] = act.astype(np.float64), logp.astype(np.float64)
        r["greedy"] = hd.unit_to_bounds(np.tanh(z), box, npdt).astype(np.float64)
    return r


def next_reference(params, actor, critic, head, cobs, state, commit, terminated, stored, vn=None, dtype=torch.float64,
                   planted=Planted()):
    """One CRITIC_NEXT launch -> dict(values [E] (boot_value_out), critic_h / critic_c (stepped when `commit`, else as they
    were), actor_h / actor_c (as they were), stored_* (the terminated rows zeroed)), float64 numpy."""
    pl = planted
    na = lo.tensor_table(actor, head == GAU)[1]
    val, ch, cc = net_step(critic, np.asarray(params, np.float64)[na:], cobs, state[2], state[3], dtype, pl)
    keep = bool(commit) or pl.ignore_commit
    r = dict(actor_h=np.asarray(state[0], np.float64), actor_c=np.asarray(state[1], np.float64),
             critic_h=ch.double().numpy().copy() if keep else np.asarray(state[2], np.float64),
             critic_c=cc.double().numpy().copy() if keep else np.asarray(state[3], np.float64))
    r["values"], r["values_raw"] = _values(val, vn, dtype, pl)
    r.update(masked_rows(stored, terminated, pl))
    return r


def masked_rows(stored, terminated, planted=Planted()):
    """The four stored rows after the zeroing (MASK, and the tail of CRITIC_NEXT)."""
    term = np.asarray(terminated, bool)
    if planted.terminated_shifted:
        term = np.concatenate([[False], term[:-1]])
    out = {}
    for k, t in zip(STORED, stored):
        t = np.array(t, np.float64)
        t[term] = 0.0
        out[k] = t
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def case(E, H, Fa, Fc, Da, Dc, Ia, Ic, act, head, seed, bounds=False, offset=None, small_h=False, saturate=0.0):
    return dict(E=E, H=H, Fa=Fa, Fc=Fc, Da=Da, Dc=Dc, Ia=Ia, Ic=Ic, act=act, head=head, seed=seed, bounds=bounds,
                offset=977 * seed + (seed << 33) if offset is None else offset, small_h=small_h, saturate=saturate)


CASES = {
    # E 1 .. 33: one tile short, full, one row over, two tiles and one row; in_dim at the 16-column chunk edges
    "e1_cat2": case(1, 32, 16, 32, 1, 1, 1, 15, "relu", (CAT, 2), 1),
    "e15_cat3": case(15, 64, 32, 16, 2, 1, 15, 16, "tanh", (CAT, 3), 2),
    "e16_gau1": case(16, 32, 64, 128, 1, 2, 16, 17, "leaky_relu", (GAU, 1), 3),
    "e17_wrap_cat8": case(17, 128, 128, 64, 2, 2, 17, 1, "relu", (CAT, 8), 4, offset=2 ** 32 - 5),   # the low word wraps
    "e33_gau4_bounds": case(33, 64, 16, 64, 1, 1, 255, 256, "tanh", (GAU, 4), 5, bounds=True),
    "e33_gau5": case(33, 32, 32, 128, 2, 1, 256, 255, "leaky_relu", (GAU, 5), 6),                    # a second Philox block
    # E > 64: tile 4 alone in the second group of eight workgroups; tile 8, third group, one live row
    "e65_h128_cat3": case(65, 128, 64, 32, 1, 2, 9, 12, "relu", (CAT, 3), 7),
    "e65_in256_gau8_bounds": case(65, 32, 16, 32, 1, 1, 256, 17, "tanh", (GAU, 8), 8, bounds=True),
    "e129_h128_gau5_bounds": case(129, 128, 32, 16, 2, 1, 5, 7, "leaky_relu", (GAU, 5), 9, bounds=True),
    "e129_in256_cat8": case(129, 64, 128, 16, 1, 2, 256, 255, "relu", (CAT, 8), 10),
    # a LayerNorm row of small variance; probabilities below float32's eps
    "small_h_cat3": case(17, 32, 16, 32, 1, 1, 6, 9, "relu", (CAT, 3), 11, small_h=True),
    "sat_cat5": case(16, 32, 32, 16, 1, 1, 7, 5, "tanh", (CAT, 5), 12, saturate=10.0),
    # the remaining heads, widths and depths
    "e17_gau8": case(17, 64, 64, 32, 2, 2, 3, 3, "relu", (GAU, 8), 13),
    "e16_gau1_bounds": case(16, 128, 16, 128, 1, 1, 1, 256, "tanh", (GAU, 1), 14, bounds=True),
    "e15_gau4": case(15, 32, 128, 64, 2, 1, 17, 15, "leaky_relu", (GAU, 4), 15),
    "e1_gau5_bounds": case(1, 64, 32, 64, 1, 2, 15, 1, "relu", (GAU, 5), 16, bounds=True),
    "e33_h128_cat2": case(33, 128, 16, 32, 2, 2, 16, 255, "leaky_relu", (CAT, 2), 17),
    "e17_cat3": case(17, 64, 64, 16, 1, 1, 16, 16, "leaky_relu", (CAT, 3), 18),
}
for _i, _c in enumerate(CASES.values()):
    _c["norm_values"] = bool(_i & 1)


def nets(c):
    return (lo.Net(c["Ia"], c["H"], c["Fa"], c["Da"], c["head"][1], c["act"]),
            lo.Net(c["Ic"], c["H"], c["Fc"], c["Dc"], 1, c["act"]))


def draw_params(actor, critic, head, rng, small_h=False):
    """lstm_update_cases.draw_params for two networks of shapes of their own."""
    tables, size = lo.bucket_tables(actor, critic, head)
    H = actor.hidden
    p = np.zeros(size)
    for tag, name, off, shape in tables:
        n = int(np.prod(shape))
        if name in ("w_ih", "w_hh") or name.endswith(".weight"):
            v = rng.normal(0.0, (0.8 if name.startswith("w_") else 1.2) / np.sqrt(shape[1]), n)
        elif name == "ln_w":
            v = 1.0 + rng.normal(0.0, 0.1, n)
        elif name == "log_std":
            v = rng.normal(0.0, 0.3, n)
        else:
            v = rng.normal(0.0, 0.1, n)
            if small_h and name in ("b_ih", "b_hh"):
                v[3 * H:] -= 2.5
        p[off:off + n] = v
    return p.astype(np.float32).astype(np.float64)


LAUNCHES = ("sampled", "forced", "chain", "next0", "next1", "greedy", "infer_sampled")


class Steering:
    """A case's inputs and the float64 / float32 references of its launches (self.ref[launch] = (r64, r32))."""

    def __init__(self, c):
        self.c = c
        E, H = c["E"], c["H"]
        self.head, O = c["head"]
        self.actor, self.critic = nets(c)
        self.tables, self.size = lo.bucket_tables(self.actor, self.critic, self.head)
        self.na = lo.tensor_table(self.actor, self.head == GAU)[1]
        rng = np.random.default_rng(c["seed"])
        self.params = draw_params(self.actor, self.critic, self.head, rng, c["small_h"])
        if c["saturate"]:
            for tag, name, off, shape in self.tables:
                if tag == "actor" and name in (f"ff{c['Da']}.weight", f"ff{c['Da']}.bias"):
                    n = int(np.prod(shape))
                    self.params[off:off + n] = (self.params[off:off + n] * c["saturate"]).astype(np.float32)
        f32 = lambda x: np.asarray(x, dtype=np.float32)
        self.obs = f32(rng.normal(0, 1, (3, E, c["Ia"])))                    # the chain's three steps; [0]: every other launch
        self.cobs = f32(rng.normal(0, 1, (3, E, c["Ic"])))
        self.state = tuple(f32(0.5 * rng.normal(0, 1, (E, H))) for _ in range(4))
        self.stored0 = tuple(f32(rng.normal(0, 1, (E, H))) for _ in range(4))
        self.seed, self.offset = 0x1234ABCD5678 + c["seed"], c["offset"]
        self.vn = VN if c["norm_values"] else None
        self.bounds = BOUNDS if c["bounds"] else None
        # terminated: row 0, the last live row, a row of tile >= 4 where there is one, and about a quarter of the rest
        self.terminated = rng.random(E) < 0.25
        self.terminated[[0, E - 1]] = True
        if E > 70:
            self.terminated[70] = True
        if E > 2:
            self.terminated[1] = False                                        # (a shifted mask shows at once)
        self.ref = {}
        r64 = self.reference("sampled", torch.float64)
        # the forced launch
        if self.head == CAT:
            f = r64["actions"].copy()
            f[-1] = O + 2
            if E > 1:
                f[0] = -3
            self.saturated = np.zeros(E, bool)
            if c["saturate"]:
                # the rarest class wherever it lies safely below eps32 (the two clamped entries stay)
                rare = r64["probs"].min(1) < 0.5 * EPS32
                rare[[0, -1]] = False
                f[rare] = r64["probs"].argmin(1)[rare]
                self.saturated = rare
        else:
            f = f32(r64["drawn"])
            k = max(1, E // 8)
            f[:k] = f32(np.where(f[:k] < 0, -1.0, 1.0) * rng.uniform(3.8, 4.2, f[:k].shape))
        self.forced = f
        for launch in LAUNCHES:
            self.ref[launch] = (r64 if launch == "sampled" else self.reference(launch, torch.float64),
                                self.reference(launch, torch.float32))
        # near ties, per launch that draws or picks a class
        none = np.zeros(E, bool)
        self.near = {l: none for l in LAUNCHES}
        if self.head == CAT:
            z = self.ref["sampled"][0]
            self.near["sampled"] = self.near["infer_sampled"] = hd.near_cdf_edge(z["logits"], z["gap"])
            self.near["greedy"] = hd.greedy(CAT, z["logits"])[1]
            z = self.ref["chain"][0]
            self.near["chain"] = hd.near_cdf_edge(z["logits"], z["gap"])

    def chain_offset(self, t):
        return (self.offset + t * self.c["E"]) & 0xFFFFFFFFFFFFFFFF

    def reference(self, launch, dtype, **planted):
        """The launch's outputs and the state it leaves (see judge for what each launch is held to)."""
        pl = Planted(**planted)
        step = lambda t, state, forced=None: step_reference(
            self.params, self.actor, self.critic, self.head, self.obs[t], self.cobs[t], state, self.seed, self.chain_offset(t),
            forced, self.vn, self.bounds, dtype, pl)
        if launch in ("sampled", "infer_sampled"):
            return step(0, self.state)
        if launch == "greedy":
            r = step(0, self.state)
            r["env_action"] = r["greedy"]                                     # what INFER writes in its deterministic mode
            return r
        if launch == "forced":
            return step(0, self.state, self.forced)
        if launch == "chain":
            state = self.state
            for t in range(3):
                r = step(t, state)
                # the next launch reads what this one left in the float32 state tensors
                state = tuple(r[k] if dtype == torch.float64 else r[k].astype(np.float32) for k in STATES)
            return r
        assert launch in ("next0", "next1"), launch
        return next_reference(self.params, self.actor, self.critic, self.head, self.cobs[1], self.state, launch == "next1",
                              self.terminated, self.stored0, self.vn, dtype, pl)

    def left_out(self, launch):
        return int(self.near[launch].sum())


@functools.lru_cache(maxsize=None)
def steering(name):
    return Steering(CASES[name])


def _exact(got, want):
    """0 when bitwise the wanted values (float32 values held in float64), inf otherwise."""
    return 0.0 if np.array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64)) else float("inf")


def judge(s, got, launch):
    """A launch's outputs -- or a planted reference's dict -- under the GPU test's rules -> (number of compared rows whose
    action differs, {tensor: worst deviation / bound; inf where a tensor that must be exact is not}).
      sampled / chain   actions (Categorical: equal on the kept rows; Gaussian: raw and env action by bound), logp (kept
                        rows), values, the four states and the four stored rows by bound;
      forced            the same on every row;
      next0 / next1     values by bound; the critic's state exact (0) or by bound (1); the actor's state exact; the four
                        stored rows exact (the terminated rows zero, every other row as before);
      greedy / infer_sampled   the env action (Categorical: equal on the kept rows; Gaussian: by bound), the actor's state
                        by bound."""
    r64, r32 = s.ref[launch]
    kept = ~s.near[launch]
    cat = s.head == CAT
    fr, wrong = {}, 0
    cmp = lambda k, kg=None, mask=None: fr.__setitem__(kg or k, worst(got[kg or k], r64[k], r32[k], mask))
    if launch in ("next0", "next1"):
        cmp("values")
        for k in ("critic_h", "critic_c"):
            if launch == "next1":
                cmp(k)
            else:
                fr[k] = _exact(got[k], r64[k])
        for k in ("actor_h", "actor_c") + STORED:
            fr[k] = _exact(got[k], r64[k])
        return wrong, fr
    if launch in ("greedy", "infer_sampled"):
        if cat:
            wrong = int(((np.asarray(got["env_action"]) != r64["env_action"]) & kept).sum())
        else:
            cmp("env_action")
        cmp("actor_h"), cmp("actor_c")
        return wrong, fr
    if cat:
        wrong = int(((np.asarray(got["actions"]) != r64["actions"]) & kept).sum())
        wrong += int((np.asarray(got["raw"]) != np.asarray(got["actions"])).sum())
        wrong += int((np.asarray(got["env_action"]) != np.asarray(got["actions"])).sum())
    else:
        cmp("raw"), cmp("env_action")
    cmp("logp", mask=kept)
    cmp("values")
    for k in STATES + STORED:
        cmp(k)
    return wrong, fr
