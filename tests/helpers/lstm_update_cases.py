"""
The cases of tests/test_gpu_lstm_update_float64.py and their steering, built on the CPU from the network shapes and a seed
(no device): tests/test_lstm_update_oracle.py uses the same cases to show that every planted error is caught by one of
them and that every case finds B un-kinked items.

Everything lives in DATASET-POSITION space: N = T x 4 envs x agents positions, item p is the window of positions
[p, p + S - 1], every non-observation field of an item is the one of its last position.  The GPU test writes the tables
into the rollout buffer through the dataset's row map.

A case's steering:
  * parameters drawn from the seed (non-zero biases, an affine LayerNorm), float32-exact;
  * observations and critic observations N(0, 1), the four hidden tables 0.5 N(0, 1);
  * terminal bytes drawn (generator (seed, 1000 + round)) until the items hold every kind of window: the first byte at
    step 0, at step S - 2, at step S - 1 (no effect on observations), two bytes in one window, no byte;
  * kinks: an item with a ReLU / LeakyReLU argument within 1e-4 x its row's scale of zero (float64, lo.kinked_items) gets
    new hidden rows at its last position -- read by that item alone -- from generator (seed, round), up to 50 rounds;
  * the first B items of the permutation: max(1, B // 16) un-kinked items of each kind (as many kinds as B holds), the rest
    un-kinked items in drawn order;
  * Gaussian raw actions with |x| near 4 in the first max(1, B // 8) rows, advantages of both signs, rewards-to-go of one
    row in 50 (at least one) on Huber's linear branch, the value normaliser at (0.3, 0.25, 5000), old log-probs from
    ko.steered_old_log_probs;
  * a preset optimiser state: steps (6, 9), m and v on the gradient's scale;
  * the items behind the first B are mini-batch 1: a few items of mini-batch 0 again (their stored states are the ones
    mini-batch 0 wrote back), then unused ones, un-kinked under the float64 prediction of the state mini-batch 0 leaves.
"""
import numpy as np
import torch

from oracle import k12_oracle as ko
from oracle import lstm_update_oracle as lo

import head_gates as hg

E = 4                           # envs of every case
VN = (0.3, 0.25, 5000.0)
STEPS0 = (6, 9)
LR = 3e-4                       # the policies' default (the GPU test checks it)
KINDS = ("first byte at step 0", "first byte at step S-2", "only byte at step S-1", "two bytes", "no byte")


def case(I=5, H=32, F=16, depth=1, S=4, B=16, head=("categorical", 3), act="relu", agents=1, norm_adv=True,
         norm_values=True, huber=True, kl=0.0, ent=0.01, clip=True, second=False, small_h=False, seed=0, gates=False):
    """agents = 2: two agents per env, the critic sees both observations (in_dim 2 I).  clip = False: gradient_clip None.
    second: mini-batch 1 is run and checked as well.  small_h: output-gate biases of -2.5 + -2.5, so that the LayerNorm
    sees rows of variance ~1e-4 (its eps matters there).  gates: the head's gradient gates are closed in part of the
    mini-batch (Steering._steer_gates, tests/helpers/head_gates.py)."""
    return dict(I=I, H=H, F=F, depth=depth, S=S, B=B, head=head, act=act, agents=agents, norm_adv=norm_adv,
                norm_values=norm_values, huber=huber, kl=kl, ent=ent, clip=clip, second=second, small_h=small_h, seed=seed,
                gates=gates)


CAT, GAU = "categorical", "gaussian"
CASES = {
    # in_dim edges: the forward pads to 16-column chunks; 255 / 256 at the smallest and at the LDS-maximum shape
    **{f"in{I}": case(I=I, H=H, F=F, depth=d, S=S, B=20, head=h, act=a, seed=I) for I, H, F, d, S, h, a in (
        (1, 32, 16, 1, 4, (CAT, 2), "relu"), (3, 64, 32, 2, 3, (GAU, 2), "tanh"), (15, 32, 16, 2, 5, (CAT, 3), "leaky_relu"),
        (16, 64, 16, 1, 4, (GAU, 1), "relu"), (17, 32, 128, 1, 3, (CAT, 8), "tanh"),
        (255, 32, 16, 1, 4, (GAU, 3), "leaky_relu"), (256, 32, 16, 2, 3, (CAT, 4), "relu"))},
    "in255_max": case(I=255, H=128, F=128, depth=2, S=16, B=20, head=(CAT, 5), act="relu", seed=1255),
    "in256_max": case(I=256, H=128, F=128, depth=2, S=16, B=20, head=(GAU, 8), act="leaky_relu", seed=1256),
    "unequal_in": case(I=7, H=64, F=32, depth=2, S=4, B=24, head=(GAU, 2), act="relu", agents=2, seed=77),
    # H x F
    **{f"h{H}_f{F}": case(I=6, H=H, F=F, depth=d, S=3, B=24, head=h, act=a, seed=H + F) for H, F, d, h, a in (
        (32, 16, 2, (GAU, 2), "relu"), (32, 128, 1, (CAT, 3), "leaky_relu"), (64, 16, 1, (CAT, 5), "tanh"),
        (64, 128, 2, (GAU, 4), "relu"), (128, 16, 2, (CAT, 2), "leaky_relu"), (128, 128, 1, (GAU, 3), "tanh"),
        (64, 32, 2, (CAT, 6), "leaky_relu"), (128, 64, 1, (GAU, 5), "relu"))},
    # S
    "S1": case(S=1, B=24, H=64, F=32, depth=2, head=(GAU, 2), act="leaky_relu", seed=201),
    "S2": case(S=2, B=24, H=32, F=16, depth=1, head=(CAT, 3), act="relu", second=True, seed=202),
    "S15": case(S=15, B=20, H=64, F=16, depth=2, head=(CAT, 4), act="tanh", seed=215),
    "S16": case(S=16, B=20, H=32, F=32, depth=1, head=(GAU, 2), act="relu", seed=216),
    # out_dim
    "cat2": case(head=(CAT, 2), act="tanh", H=64, F=16, depth=2, B=20, seed=302),
    "cat8": case(head=(CAT, 8), act="relu", H=32, F=32, depth=1, B=20, seed=308),
    "gau1": case(head=(GAU, 1), act="leaky_relu", H=32, F=16, depth=2, B=20, seed=311),
    "gau2": case(head=(GAU, 2), act="relu", H=64, F=32, depth=1, B=20, seed=312),
    "gau8": case(head=(GAU, 8), act="tanh", H=32, F=64, depth=2, B=20, seed=318),
    # B: ragged tiles, one to seventeen tiles per network, the weight-gradient reduction K = B S across 16, 64 and 256
    **{f"B{B}": case(I=9, H=H, F=F, depth=d, S=S, B=B, head=h, act=a, second=sec, seed=400 + B)
       for B, S, H, F, d, h, a, sec in (
        (2, 4, 32, 16, 1, (CAT, 3), "relu", False), (5, 3, 64, 32, 2, (GAU, 2), "relu", False),
        (15, 4, 32, 16, 1, (CAT, 2), "leaky_relu", False), (16, 4, 64, 16, 2, (GAU, 3), "tanh", False),
        (17, 15, 32, 32, 1, (CAT, 4), "relu", True), (31, 2, 64, 64, 1, (GAU, 1), "leaky_relu", False),
        (33, 2, 32, 16, 2, (CAT, 5), "relu", False), (80, 4, 128, 32, 1, (GAU, 2), "relu", True),
        (257, 3, 32, 16, 1, (CAT, 3), "tanh", False))},
    # loss switches
    "no_norm_adv": case(norm_adv=False, head=(GAU, 2), H=64, F=32, depth=2, B=24, seed=91),
    "no_norm_values": case(norm_values=False, head=(CAT, 3), act="leaky_relu", B=24, seed=92),
    "mse_kl_no_entropy": case(huber=False, kl=0.3, ent=0.0, head=(GAU, 3), act="tanh", H=64, F=16, B=24, seed=93),
    "no_gradient_clip": case(clip=False, head=(CAT, 4), H=32, F=32, depth=2, B=24, seed=94),
    # a LayerNorm row of small variance
    "ln_small_variance": case(small_h=True, head=(CAT, 3), H=32, F=16, depth=1, S=3, B=24, seed=95),
}
# tests/test_gpu_head_gates.py: ppo_head_loss inside K22 with gates closed
GATES_CASES = {
    "k22_cat8": case(I=5, H=32, F=16, depth=1, S=4, B=20, head=(CAT, 8), act="relu", seed=921, gates=True),
    "k22_gau4": case(I=5, H=32, F=16, depth=1, S=4, B=20, head=(GAU, 4), act="tanh", seed=922, gates=True),
}
GATES_RMS = 10.0               # of the steered logits: unconfident rows (kind a) and confident ones among the candidates
GATES_CANDIDATES = 1024


def geometry(c):
    """(T, positions N, items) of a case: 4 envs, the smallest T with at least B + 8 items."""
    cols = E * c["agents"]
    T = -(-(c["B"] + 8 + c["S"] - 1) // cols)
    N = T * cols
    return T, N, N - (c["S"] - 1)


def nets(c):
    kind, n = c["head"]
    actor = lo.Net(c["I"], c["H"], c["F"], c["depth"], n, c["act"])
    critic = lo.Net(c["I"] * c["agents"], c["H"], c["F"], c["depth"], 1, c["act"])
    return actor, critic


def draw_params(c, rng):
    actor, critic = nets(c)
    tables, size = lo.bucket_tables(actor, critic, c["head"][0])
    H = c["H"]
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
            if c["small_h"] and name in ("b_ih", "b_hh"):
                v[3 * H:] -= 2.5
        p[off:off + n] = v
    return p.astype(np.float32).astype(np.float64)


def window_kinds(term, S, items):
    """[items, 5] bool: which of KINDS each item's window is."""
    w = np.stack([term[s:s + items] for s in range(S)], 1).astype(np.int64)
    count = w.sum(1)
    first = np.where(count > 0, w.argmax(1), -1)
    return np.stack([first == 0, first == S - 2, (first == S - 1) & (count == 1), count >= 2, count == 0], 1)


class Steering:
    """The steered tables of a case, its first mini-batch and that mini-batch's float64 / float32 references."""

    def __init__(self, c):
        self.c, B, S, H, seed = c, c["B"], c["S"], c["H"], c["seed"]
        self.T, self.N, self.items = geometry(c)
        N, items = self.N, self.items
        self.head = c["head"][0]
        self.actor, self.critic = nets(c)
        self.tables, self.size = lo.bucket_tables(self.actor, self.critic, self.head)
        self.na = lo.tensor_table(self.actor, self.head == "gaussian")[1]
        rng = np.random.default_rng(seed)
        self.params = draw_params(c, rng)
        f32 = lambda x: np.asarray(x, dtype=np.float32)
        self.obs = f32(rng.normal(0, 1, (N, self.actor.in_dim)))
        self.cobs = f32(rng.normal(0, 1, (N, self.critic.in_dim)))
        self.hidden = {k: f32(0.5 * rng.normal(0, 1, (N, H))) for k in ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell")}
        O = self.actor.out_dim
        if self.head == "gaussian":
            self.raw_actions = f32(rng.normal(0, 1.5, (N, O)))
        else:
            self.raw_actions = rng.integers(0, O, (N, 1)).astype(np.int64)
        self.advantages = f32(rng.normal(0.2, 1.0, N))
        sd = 0.5 if c["norm_values"] else 1.0
        self.rewards_to_go = f32(0.3 + sd * rng.normal(0, 1, N))
        self.log_probs = np.zeros(N, np.float32)
        self.vn = VN if c["norm_values"] else (0.0, 1.0, 1e-4)
        self.consts = ko.Consts(c["norm_adv"], c["norm_values"], c["huber"], 10.0, 0.2, c["ent"], c["kl"], 0.01)
        # ---- terminal bytes: every kind of window among the items
        self.need = max(1, B // 16)
        self.term = np.zeros(N, dtype=bool)
        self.kinds = np.zeros((items, 5), dtype=bool)
        self.kinds[:, 4] = True
        if S > 1:
            for r in range(400):
                g = np.random.default_rng((seed, 1000 + r))
                term = g.random(N) < 1.0 / (S + 1)
                kinds = window_kinds(term, S, items)
                if (kinds.sum(0) >= self.need + (r < 200)).all():        # (one to spare for the kinks, if a draw has it)
                    break
            else:
                raise AssertionError("no draw of the terminal bytes holds every kind of window")
            self.term, self.kinds = term, kinds
        # ---- kinks: new hidden rows for kinked items
        all_items = np.arange(items)
        for r in range(51):
            ka, kc = self.kinked(all_items, self.params, self.hidden)
            if r == 50 or not (ka.any() or kc.any()):
                break
            g = np.random.default_rng((seed, r))
            last = all_items + S - 1
            for k, bad in (("actor_hidden", ka), ("actor_cell", ka), ("critic_hidden", kc), ("critic_cell", kc)):
                self.hidden[k][last[bad]] = f32(0.5 * g.normal(0, 1, (int(bad.sum()), H)))
        self.unkinked = ~(ka | kc)
        # ---- the first B items: every kind, then un-kinked items in drawn order
        order = rng.permutation(items)
        order = order[self.unkinked[order]]
        chosen = []
        if S > 1:
            for k in range(5):
                of_kind = [i for i in order if self.kinds[i, k] and i not in chosen]
                chosen += of_kind[:max(0, min(self.need, B - len(chosen)))]
        chosen += [i for i in order if i not in chosen][:B - len(chosen)]
        self.budget = len(order)                         # un-kinked candidates
        if len(chosen) < B:
            raise AssertionError(f"kink budget: {len(order)} un-kinked items of {items}, {B} needed")
        chosen = np.asarray(chosen, dtype=np.int64)[rng.permutation(B)]
        self.chosen, last = chosen, chosen + S - 1
        self.forced = np.zeros(0, dtype=np.int64)
        if c["gates"]:
            self._steer_gates(rng)
        elif self.head == "gaussian":
            k = max(1, B // 8)
            a = self.raw_actions[last[:k]]
            self.raw_actions[last[:k]] = f32(np.where(a < 0, -1.0, 1.0) * rng.uniform(3.8, 4.2, a.shape))
        k = max(1, B // 50)
        self.rewards_to_go[last[:k]] = f32(0.3 + sd * 20.0 * np.where(rng.random(k) < 0.5, -1.0, 1.0))
        logp = lo.minibatch(self.params, self.actor, self.critic, self.head, self.minibatch_of(chosen), self.consts, self.vn)["logp"]
        self.log_probs[last] = ko.steered_old_log_probs(logp, rng, self.consts.surr_clip)
        # (small B: the last two rows on either side of the clip for certain, with advantages of either sign)
        self.log_probs[last[-2:]] = np.float32(logp[-2:] - np.log([0.65, 1.45]))
        self.advantages[last[-2:]] = np.abs(self.advantages[last[-2:]]) * np.float32([1.0, -1.0])
        if len(self.forced):                  # the tuned rows' surrogate inside the clip
            self.log_probs[last], self.advantages[last] = hg.force_surrogate(self.log_probs[last], self.advantages[last], logp,
                                                                              self.forced)
        self.mb =self.minibatch_of(chosen)
        self.r64 = self.reference(torch.float64)
        self.r32 = self.reference(torch.float32)
        self.gates_failures = None
        if c["gates"]:
            self.gates_failures = hg.census_failures(self.head, (), O, self.r64, self.r32, self.mb.raw_actions)
            self.census = hg.describe(self.head, (), self.r64, self.mb.raw_actions)
        # ---- preset optimiser state on the gradient's scale, the two clip thresholds
        g = self.r64["grads"]
        self.pad = np.ones(self.size, dtype=bool)
        for _, _, off, shape in self.tables:
            self.pad[off:off + int(np.prod(shape))] = False
        rng2 = np.random.default_rng(seed + 1)
        rms = np.sqrt(np.mean(g * g)) + 1e-12
        self.m0 = f32(np.where(self.pad, 0.0, 0.5 * g + rng2.normal(0, 0.1 * rms, g.size)))
        self.v0 = f32(np.where(self.pad, 0.0, g * g * rng2.uniform(0.5, 2.0, g.size) + (0.1 * rms) ** 2))
        norms = [np.sqrt((g[:self.na] ** 2).sum()), np.sqrt((g[self.na:] ** 2).sum())]
        self.max_norms = [float(np.float32(0.25 * min(norms))), float(np.float32(4.0 * max(norms)))] if c["clip"] else [None]
        # ---- mini-batch 1
        self.perm = np.concatenate([chosen, np.setdiff1d(order, chosen), np.setdiff1d(all_items, order)])
        self.second = None
        if c["second"]:
            self._steer_second(rng)

    # ------------------------------------------------------------------------------------------------------------------
    def windows(self, items, hidden=None):
        """(actor windows, critic windows, terminal bytes, the four states at the last and at the first position)."""
        hidden = self.hidden if hidden is None else hidden
        pos = np.asarray(items)[:, None] + np.arange(self.c["S"])[None, :]
        keys = ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell")
        return (self.obs[pos], self.cobs[pos], self.term[pos], tuple(hidden[k][pos[:, -1]] for k in keys),
                tuple(hidden[k][pos[:, 0]] for k in keys))

    def minibatch_of(self, items, hidden=None):
        obs, cobs, term, last_states, first_states = self.windows(items, hidden)
        last = np.asarray(items) + self.c["S"] - 1
        raw = self.raw_actions[last]
        return lo.Minibatch(obs, cobs, term, *last_states, raw if self.head == "gaussian" else raw.reshape(-1),
                            self.log_probs[last], self.advantages[last], self.rewards_to_go[last], first_states)

    def kinked(self, items, params, hidden):
        obs, cobs, term, (ah, ac, ch, cc), _ = self.windows(items, hidden)
        masked = np.where(lo.window_mask(term)[:, :, None], np.float32(0.0), obs)
        return (lo.kinked_items(self.actor, params[:self.na], masked, ah, ac),
                lo.kinked_items(self.critic, params[self.na:], cobs, ch, cc))

    def reference(self, dtype, mb=None, params=None, vn=None, **planted):
        return lo.minibatch(self.params if params is None else params, self.actor, self.critic, self.head,
                            self.mb if mb is None else mb, self.consts, self.vn if vn is None else vn, dtype=dtype, **planted)

    def _steer_gates(self, rng):
        """The gates steering of tests/helpers/head_gates.py on the chosen items.  A LayerNorm stands before the head, so a
        row's confidence cannot be tuned by scaling its inputs: each item's (h, c) at its last position -- read by that item
        alone -- is picked among GATES_CANDIDATES draws (h = 0.9 tanh N(0, 1), c = 1.5 N(0, 1): wider than the other rows', so
        that the logits move) of generator (seed, 3000 + row) as the first un-kinked one, not near
        a gate, of the kind the row's index asks for (row % 4: a top class above 1 - eps32; a second class at 0.05 .. 0.45
        eps32, the tuned row; no class out of range; any)."""
        c, S, H, seed, head = self.c, self.c["S"], self.c["H"], self.c["seed"], self.head
        table, na = lo.tensor_table(self.actor, head == "gaussian")
        spans = {name: (off, shape) for name, off, shape in table}
        weight, bias = spans[f"ff{self.actor.ff_depth}.weight"], spans[f"ff{self.actor.ff_depth}.bias"]
        f32 = lambda x: np.asarray(x, dtype=np.float32)
        T = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
        chosen, last = self.chosen, self.chosen + S - 1
        obs, _, term, _, _ = self.windows(chosen)
        masked = np.where(lo.window_mask(term)[:, :, None], np.float32(0.0), obs)

        def forward(params, inputs):
            with torch.no_grad():
                return lo._Module(self.actor, params[:na], torch.float64)(T(inputs["obs"]), T(inputs["h"]), T(inputs["c"]))[0].numpy()

        inputs = dict(obs=masked, h=self.hidden["actor_hidden"][last], c=self.hidden["actor_cell"][last])
        self.params, tanh_dim = hg.steer_last_layer(self.params, weight, bias, spans["log_std"][0] if head == "gaussian" else None,
                                                    self.actor.out_dim, head, lambda p: forward(p, inputs), GATES_RMS)
        K = GATES_CANDIDATES
        outs = np.zeros((len(chosen), self.actor.out_dim))
        for i in range(len(chosen)):
            g = np.random.default_rng((seed, 3000 + i))
            cand = dict(obs=np.repeat(masked[i:i + 1], K, axis=0), h=f32(0.9 * np.tanh(g.normal(0, 1, (K, H)))), c=f32(1.5 * g.normal(0, 1, (K, H))))
            out = forward(self.params, cand)
            ok = ~lo.kinked_items(self.actor, self.params[:na], cand["obs"], cand["h"], cand["c"])
            if head == "gaussian":
                tp = (1.0 - np.tanh(out) ** 2) / 1e-6
                ok &= ~((tp >= 0.5) & (tp <= 2.0)).any(axis=1)
                want = ok
            else:
                n = hg.probabilities(head, (), out)
                ok &= ~hg.near_discrete(n)
                srt = np.sort(n, axis=1)
                gap = (1.0 - srt[:, -1]) / hg.EPS32
                want = ok & [gap < 0.5, (srt[:, -2] / hg.EPS32 > 0.05) & (srt[:, -2] / hg.EPS32 < 0.45) & (gap < 0.5),
                             (srt[:, 0] > hg.EPS32) & (gap > 2.0), ok][i % 4]
            k = int(np.argmax(want)) if want.any() else int(np.argmax(ok))
            assert ok[k], "no candidate state without a kink and away from the gates"
            self.hidden["actor_hidden"][last[i]], self.hidden["actor_cell"][last[i]] = cand["h"][k], cand["c"][k]
            outs[i] = out[k]
        if head == "gaussian":
            ls = spans["log_std"][0]
            self.raw_actions[last] = hg.plant_gaussian(outs, self.params[ls:ls + self.actor.out_dim], self.consts.min_std, rng, tanh_dim)
        else:
            self.raw_actions[last] = hg.plant_discrete(head, (), outs, hg.probabilities(head, (), outs), rng).reshape(-1, 1)
            self.forced = np.arange(len(chosen))[1::4]

    def _steer_second(self, rng):
        """Mini-batch 1 = perm[B : B + L], L = min(items - B, B): three items of mini-batch 0 again, then unused ones;
        chosen un-kinked and given old log-probs under the float64 prediction of what mini-batch 0 leaves behind."""
        c, B, S = self.c, self.c["B"], self.c["S"]
        L = min(self.items - B, B)
        p1 = ko.clip_adam(self.params, self.r64["grads"], self.m0, self.v0, STEPS0, LR, self.max_norms[-1] or 0.0, self.na)[0]
        p1 = p1.astype(np.float32).astype(np.float64)
        hidden = {k: v.copy() for k, v in self.hidden.items()}
        last0 = self.chosen + S - 1
        for k, r in (("actor_hidden", "actor_h"), ("actor_cell", "actor_c"), ("critic_hidden", "critic_h"), ("critic_cell", "critic_c")):
            hidden[k][last0] = self.r64[r].astype(np.float32)
        cand = np.concatenate([self.chosen[:B // 2][::-1], self.perm[B:]])           # (items of mini-batch 0 first)
        ka, kc = self.kinked(cand, p1, hidden)
        ok = cand[~(ka | kc)]
        again = [i for i in ok if i in set(self.chosen.tolist())][:min(3, L - 1)]
        fresh = [i for i in ok if i not in set(self.chosen.tolist())][:L - len(again)]
        assert again and len(again) + len(fresh) == L, "mini-batch 1: not enough un-kinked items"
        mb1 = np.asarray(again + fresh, dtype=np.int64)[rng.permutation(L)]
        rest = np.setdiff1d(self.perm[B:], mb1)
        self.perm = np.concatenate([self.chosen, mb1, rest])[:self.items]
        vn1 = self.r64["vn"] if c["norm_values"] else self.vn
        new = np.asarray([i for i in mb1 if i in set(fresh)], dtype=np.int64)
        if len(new):
            logp = lo.minibatch(p1, self.actor, self.critic, self.head, self.minibatch_of(new, hidden), self.consts, vn1)["logp"]
            self.log_probs[new + S - 1] = ko.steered_old_log_probs(logp, rng, self.consts.surr_clip)
        self.second = mb1
