"""
The cases of tests/test_gpu_mat_update_float64.py and their steering, built on the CPU from the shapes and a seed (no
device): tests/test_mat_update_oracle.py uses the same cases to show that every planted error is caught by one of them and
that every case meets its conditions by construction.  Shapes are written (A, O, NA, B): agents, observation width,
actions, envs per mini-batch (B A token rows; floor(16 / A) envs per 16-row tile, the other 16 % A rows dead).

A case's steering (everything float32-exact):
  * the parameter bucket overwritten: weights N(0, 1 / fan_in) x 1.2 (with 64-wide LayerNorm'd inputs the key and query
    linears then give scores of O(1) spread), every bias 0.3 N(0, 1), every LayerNorm gain 1 + U(-0.3, 0.3) with a bias
    0.3 N(0, 1) -- the default initialisation (gains of 0.01, zero biases, identity LayerNorms) leaves the attention cores
    with uniform softmaxes and gradients 1e-9 of the bucket's largest (see test_default_initialisation_hides_...);
  * observations N(0, 1), raw actions uniform, advantages N(0.2, 1), rewards-to-go 0.3 + sd N(0, 1) clipped to 3 sd, one
    token in 50 (at least one) 25 sd away: Huber's linear branch (delta 10 on the normalised scale);
  * the value normaliser at (0.3, 0.25, 5000) (normalize_values) and this mini-batch's (n, mean, M2) record, with a
    synthetic second rank's record for n_ranks = 2;
  * old log-probs from ko.steered_old_log_probs; the first tokens are then set by hand: (ratio 1.45, advantage +2) and
    (0.65, -2) clipped, (1.05, -2) and (0.9, +2) not -- as many of the four as the mini-batch has tokens for (two at least:
    one clipped with a positive advantage, one unclipped with a negative one);
  * a preset optimiser state: step 6, m and v on the gradient's scale; clip thresholds 0.25 x and 4 x the float64 norm;
  * `second`: mini-batch 1 of max(2, B // 2) envs -- a tail shorter than batch_stride -- steered under the float64
    prediction of the parameters mini-batch 0 leaves.
GELU has no kink: no token is ever left out of a comparison.

ANALYTICALLY ZERO tensors (zero_tensors): exactly zero in exact arithmetic, and required to be exactly zero on the GPU
  * A = 1: attention over one token -- the softmax has one column, its backward p (dp - p dp) is 0: every key_net.* and
    query_net.* of the three attentions;
  * NA = 1: one action -- the log-prob and the entropy are constants: every actor.* tensor (the critic's tensors keep the
    critic loss).
float64 autograd gives exactly 0.0 for these.  ZERO IN EXACT ARITHMETIC, ROUND-OFF IN FLOATING POINT (round_off_zero; at most
1e-12 of the bucket's largest entry in float64), judged on the scale of a neighbouring tensor:
  * the three key_net.bias tensors in EVERY case (a constant added to every key shifts each score row by a constant, which
    softmax ignores): on the scale of the same attention's query_net.bias (KEY_BIAS);
  * O = 1: LayerNorm over one column returns its bias, so the gain critic.obs_encoder.0.weight has no gradient -- but
    torch's layer_norm backward leaves 1e-13 in float64 and 1e-7 in float32: on the scale of critic.obs_encoder.0.bias.
The cases these rules touch: min_1_1_1_2 (A = 1, O = 1 and NA = 1: every actor.* tensor and the critic's key / query linears
exactly zero, the observation LayerNorm's gain round-off), lds_1_32_8_17 and draw5_1_66_6_31 (A = 1), draw2_1_109_1_7
(A = 1 and NA = 1), draw3_3_3_1_30 (NA = 1); tests/test_mat_update_oracle.py holds the rules to what the float64 oracle gives.
"""
import numpy as np
import torch

from oracle import k12_oracle as ko
from oracle import mat_update_oracle as mu

import head_gates as hg

VN = (0.3, 0.25, 5000.0)
STEP0 = 6
LR = float(np.float32(3e-4))
SECOND_RECORD = (37.0, 0.1, 9.0)          # the synthetic second rank's (n, mean, M2)
ATTENTIONS = ("actor.blocks.0.attn1", "actor.blocks.0.attn2", "critic.blocks.0.attn")
KEY_BIAS = {f"{a}.key_net.bias": f"{a}.query_net.bias" for a in ATTENTIONS}
ROW_MODES = ("map", "order", "offset", "tail")


def case(A, O, NA, B, seed, norm_values=True, n_ranks=1, norm_adv=True, huber=True, kl=0.0, ent=0.01, rows="map", second=False,
         saturate=0.0):
    """rows: how the GPU test addresses the mini-batch (perm o row_map on buffer rows; per-epoch tables from cursor 1; the
    same by mb_offset 1; a tail mini-batch behind two full ones).  second: mini-batch 1 is launched right after.
    saturate: the head's last linear multiplied by it (tests/helpers/mat_step_cases.py) and actions planted so that the
    clamp's gradient gate is closed in part of the tokens (Steering._gates, tests/helpers/head_gates.py)."""
    return dict(A=A, O=O, NA=NA, B=B, seed=seed, norm_values=norm_values, n_ranks=n_ranks, norm_adv=norm_adv, huber=huber,
                kl=kl, ent=ent, rows=rows, second=second, saturate=saturate)


def _drawn():
    """Six seeded draws over the kernel's whole range, the same six in every run."""
    rng = np.random.default_rng(20240615)
    out = {}
    for i in range(6):
        A, O, NA, B = int(rng.integers(1, 17)), int(rng.integers(1, 129)), int(rng.integers(1, 9)), int(rng.integers(2, 41))
        out[f"draw{i}_{A}_{O}_{NA}_{B}"] = case(A, O, NA, B, 700 + i, norm_values=bool(i & 1), norm_adv=i != 2, huber=i != 3,
                                                kl=0.5 if i == 4 else 0.0, ent=0.0 if i == 5 else 0.01,
                                                n_ranks=2 if i == 1 else 1, rows=ROW_MODES[i % 4])
    return out


CASES = {
    "c5_3_18_5_32": case(3, 18, 5, 32, 1, second=True),                              # the C5 topology
    "min_1_1_1_2": case(1, 1, 1, 2, 2, rows="order"),                               # every lower limit at once
    "lds_1_32_8_17": case(1, 32, 8, 17, 3, rows="offset", n_ranks=2),               # last width staged whole; a tile of one sequence
    "mask_16_33_8_3": case(16, 33, 8, 3, 4, rows="tail", huber=False, second=True),  # the mask fills the tile; first chunked width
    "dead_7_64_2_5": case(7, 64, 2, 5, 5, rows="map", kl=0.5, second=True),          # 2 sequences + 2 dead rows; half-filled last tile
    "chunk_5_65_4_7": case(5, 65, 4, 7, 6, rows="order", norm_adv=False),
    "chunk_6_96_3_5": case(6, 96, 3, 5, 7, rows="offset", norm_values=False),
    "chunk_3_97_5_11": case(3, 97, 5, 11, 8, rows="tail", ent=0.0),
    "chunk_2_128_8_9": case(2, 128, 8, 9, 9, rows="map", huber=False, kl=0.5),
    "chunk_16_128_8_2": case(16, 128, 8, 2, 10, rows="order", norm_values=False, norm_adv=False),
    "tiles64_16_7_4_64": case(16, 7, 4, 64, 11, rows="offset"),                      # the last count in one trip of the wgrad tile
    "tiles65_16_7_4_65": case(16, 7, 4, 65, 12, rows="tail", n_ranks=2),             # the first that takes a second trip
    **_drawn(),
}


# tests/test_gpu_head_gates.py: K15's own head with the clamp's gate closed
GATES_CASES = {
    "k15_3_18_8_11": case(3, 18, 8, 11, 961, saturate=8.0),
    "k15_16_7_5_3": case(16, 7, 5, 3, 942, saturate=8.0, rows="order"),
}


def zero_tensors(A, O, NA, names):
    """The analytically zero tensors of a shape that float64 autograd gives as exactly 0.0 (module docstring)."""
    return {n for n in names if (NA == 1 and n.startswith("actor.")) or (A == 1 and (".key_net." in n or ".query_net." in n))}


def round_off_zero(A, O, NA, names):
    """{tensor zero in exact arithmetic but round-off in floating point: the tensor whose scale it is judged on}."""
    out = dict(KEY_BIAS)
    if O == 1:
        out["critic.obs_encoder.0.weight"] = "critic.obs_encoder.0.bias"
    exact = zero_tensors(A, O, NA, names)
    return {n: ref for n, ref in out.items() if n not in exact}


def draw_params(A, O, NA, rng):
    table, size = mu.bucket_table(A, O, NA)
    p = np.zeros(size)
    for _, name, off, shape in table:
        n = int(np.prod(shape))
        if len(shape) == 2:
            v = rng.normal(0.0, 1.2 / np.sqrt(shape[1]), n)
        elif name.endswith(".weight"):                    # a LayerNorm's gain
            v = 1.0 + rng.uniform(-0.3, 0.3, n)
        else:                                             # a bias, of a linear or of a LayerNorm: never zero
            v = 0.3 * rng.normal(0.0, 1.0, n)
            v = np.where(np.abs(v) < 1e-3, 1e-3, v)
        p[off:off + n] = v
    return p.astype(np.float32).astype(np.float64)


FORCED = ((1.45, 2.0), (1.05, -2.0), (0.65, -2.0), (0.9, 2.0))      # (ratio, advantage): clipped, not, clipped, not


class Steering:
    """The steered mini-batch(es) of a case and their float64 / float32 references."""

    def __init__(self, c):
        self.c = c
        A, O, NA, B = self.shape = (c["A"], c["O"], c["NA"], c["B"])
        self.table, self.size = mu.bucket_table(A, O, NA)
        self.names = [n for _, n, _, _ in self.table]
        self.pad = np.ones(self.size, dtype=bool)
        for _, _, off, shape in self.table:
            self.pad[off:off + int(np.prod(shape))] = False
        rng = np.random.default_rng(c["seed"])
        self.params = draw_params(A, O, NA, rng)
        self.gated = None
        self.consts = ko.Consts(c["norm_adv"], c["norm_values"], c["huber"], 10.0, 0.2, c["ent"], c["kl"], 0.01)
        self.vn = VN if c["norm_values"] else (0.0, 1.0, 1e-4)
        if c["saturate"]:
            self._gates()
        self.mb = self.draw(B, rng, self.params, self.vn)
        self.records = self.records_of(self.mb)
        self.r64 = self.reference(torch.float64)
        self.r32 = self.reference(torch.float32)
        g = self.r64["grads"]
        rng2 = np.random.default_rng(c["seed"] + 1)
        rms = np.sqrt(np.mean(g * g)) + 1e-12
        f32 = lambda x: np.asarray(x, dtype=np.float32)
        self.m0 = f32(np.where(self.pad, 0.0, 0.5 * g + rng2.normal(0, 0.1 * rms, g.size)))
        self.v0 = f32(np.where(self.pad, 0.0, g * g * rng2.uniform(0.5, 2.0, g.size) + (0.1 * rms) ** 2))
        norm = float(np.sqrt((g * g).sum()))
        self.max_norms = [float(np.float32(0.25 * norm)), float(np.float32(4.0 * norm))]
        self.mb1 = None
        if c["second"]:
            p1 = mu.clip_adam(self.params, g, self.m0, self.v0, STEP0, LR, self.max_norms[-1])[0]
            vn1 = self.r64["vn"] if c["norm_values"] else self.vn
            self.mb1 = self.draw(max(2, B // 2), rng, p1.astype(np.float32).astype(np.float64), vn1)

    def draw(self, B, rng, params, vn):
        """One steered mini-batch of B envs under `params` and the normaliser state `vn`."""
        c, (A, O, NA, _) = self.c, self.shape
        f32 = lambda x: np.asarray(x, dtype=np.float32)
        n = B * A
        obs = f32(rng.normal(0, 1, (B, A, O)))
        act = rng.integers(0, NA, (B, A)).astype(np.int64)
        if self.gated is not None:
            obs, act = self.gated
        adv = f32(rng.normal(0.2, 1.0, n))
        sd = 0.5 if c["norm_values"] else 1.0
        rtg = 0.3 + sd * np.clip(rng.normal(0, 1, n), -3.0, 3.0)
        far = rng.permutation(n)[:max(1, n // 50)]
        rtg[far] = 0.3 + sd * 25.0 * np.where(rng.random(len(far)) < 0.5, -1.0, 1.0)
        rtg = f32(rtg)
        k = min(len(FORCED), n)
        adv[:k] = f32([a for _, a in FORCED[:k]])
        mb = mu.Minibatch(obs, act, np.zeros((B, A), np.float32), adv.reshape(B, A), rtg.reshape(B, A))
        logp = mu.minibatch(params, A, O, NA, mb, self.consts, vn, self.records_of(mb))["logp"].reshape(-1)
        old = ko.steered_old_log_probs(logp, rng, self.consts.surr_clip)
        old[:k] = f32(logp[:k] - np.log([r for r, _ in FORCED[:k]]))
        if self.gated is not None:             # tokens whose closed gate would carry a visible surrogate gradient: inside the clip
            chosen = np.take_along_axis(self.probs_of(params, obs, act), act[..., None], -1).reshape(-1) / hg.EPS32
            self.visible = np.array([i for i in np.flatnonzero((chosen > 0.01) & (chosen < 0.9)) if i >= k], dtype=np.int64)
            old, adv = hg.force_surrogate(old, adv, logp, self.visible)
            mb = mb._replace(advantages=adv.reshape(B, A))
        return mb._replace(old_log_probs=old.reshape(B, A))

    def probs_of(self, params, obs, act):
        """float64 renormalised probabilities [B, A, NA] of the tokens under the given actions."""
        A, O, NA, _ = self.shape
        net = mu.network(A, O, NA, params)
        with torch.no_grad():
            _, p = net(torch.as_tensor(obs, dtype=torch.float64), mu.action_block(act, A, NA))
        return (p / p.sum(-1, keepdim=True)).numpy()

    def logits_of(self, params, obs, act):
        """float64 outputs of the head's last linear [B, A, NA]."""
        A, O, NA, _ = self.shape
        net = mu.network(A, O, NA, params)
        got = []
        hook = net.actor.head[3].register_forward_hook(lambda m, i, o: got.append(o.detach().numpy()))
        with torch.no_grad():
            net(torch.as_tensor(obs, dtype=torch.float64), mu.action_block(act, A, NA))
        hook.remove()
        return got[0]

    def _gates(self):
        """The gates steering on the B A tokens.  A LayerNorm stands before everything, so a token's confidence cannot be
        tuned by scaling its observation, and one factor on the head's last linear leaves every token equally confident.
        Its rows are therefore scaled apart: classes 1 .. to a root mean square of saturate / 4 over the tokens (among
        themselves in range), class 0 to a standard deviation of 2 saturate against them, its bias set so that it is centred on them -- far above them in some tokens
        (kind d), far below in others (b, c), among them in the rest (a).  Observations come from generator
        (seed, 500 + round) and actions are planted agent by agent (an agent's probabilities depend on the agents before
        it) by hg's row rule, until the tokens hold every kind, none is near a gate, and two chosen classes lie at
        0.01 .. 0.9 eps32 (their surrogate gradient is what an open gate would let through)."""
        c, (A, O, NA, B) = self.c, self.shape
        spans = {name: (off, shape) for _, name, off, shape in self.table}
        (wo, (_, width)), (bo, _) = spans["actor.head.3.weight"], spans["actor.head.3.bias"]
        g = np.random.default_rng((c["seed"], 499))
        z = self.logits_of(self.params, np.asarray(g.normal(0, 1, (64, A, O)), dtype=np.float32), g.integers(0, NA, (64, A)))
        z = z.reshape(-1, NA)
        rest = z[:, 1:].mean(axis=1)
        f = np.full(NA, 0.25 * c["saturate"] / np.sqrt(((z[:, 1:] - rest[:, None]) ** 2).mean()))
        f[0] = 2.0 * c["saturate"] / (z[:, 0] - rest).std()
        for k in range(NA):
            self.params[wo + k * width:wo + (k + 1) * width] *= f[k]
            self.params[bo + k] *= f[k]
        self.params[bo] -= (f[0] * z[:, 0] - f[1] * rest).mean()          # class 0 centred on the others over the tokens
        self.params = self.params.astype(np.float32).astype(np.float64)
        for r in range(200):
            g = np.random.default_rng((c["seed"], 500 + r))
            obs = np.asarray(g.normal(0, 1, (B, A, O)), dtype=np.float32)
            act = np.zeros((B, A), dtype=np.int64)
            for i in range(A):
                n = self.probs_of(self.params, obs, act)
                for b in range(B):
                    act[b, i] = hg._plant_classes(n[b, i], (b * A + i) % 4, g)
            n = self.probs_of(self.params, obs, act).reshape(-1, NA)
            kinds = hg.counts(hg.census("categorical", (), dict(n=n), act.reshape(-1)))[1]
            chosen = n[np.arange(B * A), act.reshape(-1)] / hg.EPS32
            if not hg.near_discrete(n).any() and all(kinds.get(k, 0) >= hg.MIN_ENTRIES for k in "abcd") \
                    and ((chosen > 0.01) & (chosen < 0.9))[4:].sum() >= 2:
                self.gated, self.rounds = (obs, act), r
                return
        raise AssertionError("no draw of the observations holds every kind of token away from the gates")

    def gates_failures(self):
        """hg.census_failures of the steered tokens (rows = tokens) on the two references."""
        NA = self.shape[2]
        as_args = lambda r: dict(gate_args=dict(n=r["probs"].reshape(-1, NA)))
        return hg.census_failures("categorical", (), NA, as_args(self.r64), as_args(self.r32), self.mb.raw_actions.reshape(-1))

    def records_of(self, mb):
        """The mini-batch's (n, mean, M2) per rank."""
        return [mu.own_record(mb.rewards_to_go)] + ([SECOND_RECORD] if self.c["n_ranks"] == 2 else [])

    def reference(self, dtype, mb=None, params=None, vn=None, **planted):
        A, O, NA, _ = self.shape
        mb = self.mb if mb is None else mb
        return mu.minibatch(self.params if params is None else params, A, O, NA, mb, self.consts,
                            self.vn if vn is None else vn, self.records_of(mb), dtype, mu.Planted(**planted))

    def zero(self):
        return zero_tensors(*self.shape[:3], self.names)

    def round_off(self):
        return round_off_zero(*self.shape[:3], self.names)

    def judge(self, got, r64=None, r32=None):
        """judge_gradient of a gradient bucket against the case's references (or those of another mini-batch)."""
        return judge_gradient(got, (r64 or self.r64)["grads"], (r32 or self.r32)["grads"], self.table, self.zero(), self.round_off())


def judge_gradient(got, r64, r32, table, zero, round_off):
    """
    The gradient bucket per tensor under ko.deviations -> [(tensor, fraction of the bound, floor)].  Two kinds of tensor
    have no scale of their own.  An analytically zero tensor (`zero`: float64 gives exactly 0.0) must be exactly zero.  A
    tensor of `round_off` -- zero in exact arithmetic, round-off in float64: each key_net.bias, judged on the scale of the
    same attention's query_net.bias -- is held to |x - x64| <= 1e-5 max|g64 of the partner tensor|, raised to
    4 max|x32 - x64| of the tensor itself.
    """
    got = np.asarray(got, dtype=np.float64)
    spans = {n: slice(o, o + int(np.prod(s))) for _, n, o, s in table}
    out = []
    for name, frac, floor in ko.deviations(got, r64, r32, table):
        sl = spans[name]
        if name in zero:
            assert not r64[sl].any(), f"{name}: listed as analytically zero, float64 gives {np.abs(r64[sl]).max():.3g}"
            frac = 0.0 if not got[sl].any() else np.inf
        elif name in round_off:
            bound = max(1e-5 * float(np.abs(r64[spans[round_off[name]]]).max()), floor)
            err = float(np.abs(got[sl] - r64[sl]).max())
            frac = err / bound if bound > 0 else (np.inf if err > 0 else 0.0)
            if not np.all(np.isfinite(got[sl])):
                frac = np.inf
        out.append((name, float(frac), floor))
    return out
