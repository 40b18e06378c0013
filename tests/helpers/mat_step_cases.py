"""
ONE rollout step of K16 (csrc/mat_update.hip, mat_policy_step_body) restated on torch-CPU in a chosen dtype, and the cases
of tests/test_gpu_mat_step_float64.py built on it (no device): tests/test_mat_step_oracle.py shows with the same cases that
every planted error is caught by one of them and that the float32 restatement stays inside every bound and cap.  Shapes
are written (A, O, NA, E): agents, observation width, actions, envs (E A tokens; floor(16 / A) envs per 16-row tile).

The step, restated (step_reference), from oracle.mat_update_oracle.network holding a parameter bucket:
  * the encoder once: the values v [E, A], written as they are or as mean + v sqrt(var + 1e-8) (normalize_values);
  * A decoder passes over the token block [E, A, NA + 1], which starts with the start token of agent 0; pass i decides
    slot i from its logits z: p = softmax(z), s = sum p,
        u = u32_to_unit(word x of Philox(seed, offset + e A + i, stream 0)),
    the action is the first k with u s < cum_k (cum the running sum of p), NA - 1 if there is none -- or the forced action
    clamped into [0, NA - 1] --, its log-prob log(clip(p_a / s, eps32, 1 - eps32)), and its one-hot goes into slot i + 1;
  * per token the gap min_k |u s - cum_k| to the nearest edge of the CDF.

NEAR TIES (kept_tokens): a logit's bound is 1e-5 |z| + 1e-5 max|z| over the case's float64 logits; a token whose gap is
below 2 max_k bound + 1e-6 is a near tie (softmax is 1-Lipschitz in the max norm, so a CDF edge moves by at most twice the
largest logit error); an env is left out from its first near tie on, since a flipped action changes every later token
of it.  At most 5 % of a case's envs -- at most 2 where it has fewer than 40 -- may have a near tie (cap): a condition of
the case, met by the choice of its seed (tests/test_mat_step_oracle.py), not a measurement.

A case's steering: the bucket from mat_update_cases.draw_params (logits of O(1); the default initialisation's head gain
of 0.01 leaves every distribution uniform whatever the decoder does), observations N(0, 1) rounded to float32, a fixed
seed and offset (one offset's low word wraps inside the launch), value statistics (0.3, 0.25) on every other case.
`saturate`: the head's last linear multiplied so that some class probabilities fall below float32's eps -- the forced
launch then logs such classes (log eps32 by the clamp).
"""
import functools

import numpy as np
import torch

from oracle import mat_update_oracle as mu

import mat_update_cases as uc
import philox

EPS32 = mu.EPS32
VN = uc.VN[:2]                            # (mean, var) of the value normaliser


def step_reference(params, A, O, NA, obs, seed, offset, forced=None, vn=None, dtype=torch.float64, planted=mu.Planted()):
    """-> dict(logits [E, A, NA] of the slot each pass decided, probs (not renormalised), actions [E, A] (drawn, or the
    forced ones clamped), drawn [E, A] (the draw, also where a forced action overrides it), logp [E, A], values [E, A],
    gap [E, A]), everything float64 numpy computed in `dtype`."""
    pl = planted
    net = mu.network(A, O, NA, params, dtype, pl)
    x = torch.as_tensor(np.asarray(obs), dtype=dtype).reshape(-1, A, O)
    E = x.shape[0]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    logits, probs = np.zeros((E, A, NA)), np.zeros((E, A, NA))
    actions, logp, gap = np.zeros((E, A), np.int64), np.zeros((E, A)), np.zeros((E, A))
    drawn = np.zeros((E, A), np.int64)
    env = np.arange(E)
    with torch.no_grad():
        enc, v = net.critic(x)
        v = v.squeeze(-1)
        if vn is not None:
            mean, var = (torch.tensor(s, dtype=dtype) for s in vn)
            v = mean + v * (var if pl.denorm_var else torch.sqrt(var + torch.tensor(1e-8, dtype=dtype)))
        block = torch.zeros(E, A, NA + 1, dtype=dtype)
        if not pl.no_start_token:
            block[:, 0, 0] = 1
        z_all = None
        for i in range(A):
            if z_all is None or not pl.stale_logits:
                h = net.actor.ln(net.actor.action_encoder(block))
                for b in net.actor.blocks:
                    h = b(h, enc)
                z_all = net.actor.head(h)
            z = z_all[:, i, :]
            p = torch.softmax(z, dim=-1)
            s = p.sum(-1)
            cum = torch.cumsum(p, dim=-1).numpy()
            index = i * E + env if pl.counter_slot_major else env if pl.counter_no_slot else env * A + i
            word = philox.philox4x32_10(seed, philox.counters_u64(offset, index), 0)[1 if pl.philox_word_y else 0]
            us = philox.u32_to_unit(word).astype(npdt) * s.numpy()
            a = np.minimum((us[:, None] >= cum).sum(-1), NA - 1)         # cum never decreases: the first k with us < cum_k
            drawn[:, i] = a
            gap[:, i] = np.abs(us[:, None].astype(np.float64) - cum.astype(np.float64)).min(-1)
            if forced is not None:
                a = np.clip(np.asarray(forced).reshape(E, A)[:, i], 0, NA - 1)
            q = p[torch.arange(E), torch.as_tensor(a)] / s
            lp = torch.log(q if pl.logp_no_clamp else q.clamp(EPS32, 1.0 - EPS32))
            logits[:, i], probs[:, i], actions[:, i], logp[:, i] = z.numpy(), p.numpy(), a, lp.numpy()
            slot = i if pl.onehot_shift else i + 1
            if slot < A:
                block[torch.arange(E), slot, 1 + torch.as_tensor(a)] = 1
    return dict(logits=logits, probs=probs, actions=actions, logp=logp, values=v.double().numpy().copy(), gap=gap, drawn=drawn)


def near_ties(logits64, gap64):
    """bool [E, A]: the tokens whose draw lies within the logits' bound of a CDF edge."""
    z = np.abs(np.asarray(logits64, np.float64))
    bound = 1e-5 * z + 1e-5 * z.max()
    return np.asarray(gap64) < 2.0 * bound.max(-1) + 1e-6


def kept_tokens(logits64, gap64):
    """bool [E, A]: True before the env's first near tie."""
    return np.cumsum(near_ties(logits64, gap64), axis=1) == 0


def cap(E):
    """How many envs of a case may have a near tie."""
    return 2 if E < 40 else int(0.05 * E)


def case(A, O, NA, E, seed, offset=None, own_obs=0, saturate=0.0):
    """own_obs: the width of the actor's own observations (0: it sees the critic's)."""
    return dict(A=A, O=O, NA=NA, E=E, seed=seed, offset=977 * seed + (seed << 33) if offset is None else offset,
                own_obs=own_obs, saturate=saturate)


def _drawn():
    """Six seeded draws over the kernel's whole range, the same six in every run."""
    rng = np.random.default_rng(20250321)
    out = {}
    for i in range(6):
        A, O, NA, E = int(rng.integers(1, 17)), int(rng.integers(1, 129)), int(rng.integers(1, 9)), int(rng.integers(1, 66))
        out[f"draw{i}_{A}_{O}_{NA}_{E}"] = case(A, O, NA, E, 800 + i)
    return out


CASES = {
    "c5_3_18_5_4": case(3, 18, 5, 4, 1),                                    # the C5 topology: one env short of a tile
    "c5_3_18_5_5": case(3, 18, 5, 5, 2),                                    # one full tile, its dead row
    "c5_3_18_5_21": case(3, 18, 5, 21, 3, offset=2 ** 32 - 5, own_obs=7),   # four tiles and one env; the counter's low word wraps
    "min_1_1_1_1": case(1, 1, 1, 1, 4),                                     # every lower limit at once
    "lds_1_32_8_17": case(1, 32, 8, 17, 5),                                 # last width staged whole; one-token sequences
    "mask_16_33_8_3": case(16, 33, 8, 3, 6),                                # the mask fills the tile; first wide width
    "dead_7_64_2_5": case(7, 64, 2, 5, 7),                                  # two dead rows
    "chunk_5_65_4_7": case(5, 65, 4, 7, 8),
    "chunk_3_97_5_11": case(3, 97, 5, 11, 9, own_obs=40),
    "chunk_2_128_8_9": case(2, 128, 8, 9, 10),
    "chunk_16_128_8_2": case(16, 128, 8, 2, 11),
    "sat_3_18_5_16": case(3, 18, 5, 16, 12, saturate=8.0),                  # probabilities below float32's eps
    **_drawn(),
}
for _i, _c in enumerate(CASES.values()):
    _c["norm_values"] = bool(_i & 1)


class Steering:
    """A case's inputs and its float64 / float32 references of the sampled and of the forced launch."""

    def __init__(self, c):
        self.c = c
        A, O, NA, E = self.shape = (c["A"], c["O"], c["NA"], c["E"])
        self.table, self.size = mu.bucket_table(A, O, NA)
        rng = np.random.default_rng(c["seed"])
        self.params = uc.draw_params(A, O, NA, rng)
        if c["saturate"]:
            for _, name, off, shape in self.table:
                if name in ("actor.head.3.weight", "actor.head.3.bias"):
                    n = int(np.prod(shape))
                    self.params[off:off + n] = (self.params[off:off + n] * c["saturate"]).astype(np.float32)
        self.obs = rng.normal(0, 1, (E, A, O)).astype(np.float32)
        self.actor_obs = rng.normal(0, 1, (E, A, c["own_obs"])).astype(np.float32) if c["own_obs"] else None
        self.seed, self.offset = 0x1234ABCD5678 + c["seed"], c["offset"]
        self.vn = VN if c["norm_values"] else None
        self.r64, self.r32 = self.reference(torch.float64), self.reference(torch.float32)
        self.kept = kept_tokens(self.r64["logits"], self.r64["gap"])
        # the forced launch: the float64 actions, one entry below 0 and one at or above NA (one token: the latter only)
        f = self.r64["actions"].copy()
        f[-1, -1] = NA + 2
        if f.size > 1:
            f[0, 0] = -3
        self.n_saturated = 0
        if c["saturate"]:
            # the last agent's rarest class wherever it lies safely below eps32 (no later token is conditioned on it)
            p = self.reference(torch.float64, forced=f)["probs"][:, -1]
            rare = p.min(-1) < 0.5 * EPS32
            rare[[0, -1]] = False                                           # (the two clamped entries stay)
            f[rare, -1] = p.argmin(-1)[rare]
            self.saturated = np.zeros((E, A), bool)
            self.saturated[rare, -1] = True
            self.n_saturated = int(rare.sum())
        self.forced = f
        self.f64, self.f32 = self.reference(torch.float64, forced=f), self.reference(torch.float32, forced=f)

    def reference(self, dtype, forced=None, **planted):
        A, O, NA, _ = self.shape
        return step_reference(self.params, A, O, NA, self.obs, self.seed, self.offset, forced, self.vn, dtype, mu.Planted(**planted))

    def left_out(self):
        """The envs with a near tie."""
        return int((~self.kept).any(1).sum())


@functools.lru_cache(maxsize=None)
def steering(name):
    return Steering(CASES[name])


def k12_bound(x64, x32):
    """eval_kernels.k12_bound: per element 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64|."""
    x64 = np.asarray(x64, np.float64)
    tol = 1e-5 * np.abs(x64) + 1e-5 * np.abs(x64).max()
    return np.maximum(tol, 4.0 * np.abs(np.asarray(x32, np.float64) - x64).max())


def worst(got, x64, x32, mask=None):
    """The worst |got - x64| / bound over the compared elements (0 when none is compared)."""
    got, x64, x32 = (np.asarray(t, np.float64) for t in (got, x64, x32))
    if mask is not None:
        got, x64, x32 = got[mask], x64[mask], x32[mask]
    if x64.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    bound = k12_bound(x64, x32)
    err = np.abs(got - x64)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


def judge(s, got, forced=False):
    """A launch's (actions, logp, values) -- or a planted reference's dict -- under the GPU test's rules ->
    (number of compared tokens whose action differs, {tensor: worst deviation / bound}).  Sampled launch: actions and
    log-probs on the kept tokens; forced launch: on all.  The values depend on no draw: all of them, always."""
    r64, r32 = (s.f64, s.f32) if forced else (s.r64, s.r32)
    mask = np.ones_like(s.kept) if forced else s.kept
    wrong = int(((np.asarray(got["actions"]) != r64["actions"]) & mask).sum())
    return wrong, dict(logp=worst(got["logp"], r64["logp"], r32["logp"], mask), values=worst(got["values"], r64["values"], r32["values"]))
