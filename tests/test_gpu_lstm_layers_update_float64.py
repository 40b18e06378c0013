"""
-m gpu: ONE mini-batch of K22 for two stacked LSTM layers (csrc/lstm_stacked_update.hip, fused_update.FusedLstm2Update)
against a float64 reference written here -- nn.LSTM(I, H, 2) -> LayerNorm -> activation -> Linear head, around it the
oracle's own window mask, head terms, normalised rewards-to-go, losses and clip + Adam -- at the shape edges of the
kernels: H 32 / 64 / 128, S 1 (fill and drain only) .. 16, B 2 .. 33 (ragged and several tiles), in_dim 1 / 17 / 256,
depth, F, both heads, the loss switches, the three activations.

Each case builds a two-layer PPO (4 envs, the smallest T with B + 8 items), runs one rollout and overwrites from a CPU
seed: the parameter bucket (non-zero biases, affine LayerNorm), both observation tables, the four [rows, 2, H] hidden
tables, the terminal bytes (the first items of the permutation hold a window with a byte at step 0, one at S - 2, one
only at S - 1, one with none: asserted wherever S > 1 and B >= 4; B 2 holds the first and a clean one), and at every
position raw actions, advantages, rewards-to-go and old log-probs (ratios on both sides of the clip); the value
normaliser starts at (0.3, 0.25, 5000).  Then
  a. gradient_only: the gradient bucket per tensor (padding zero), the eight totals folded from the loss partials, the
     values and both layers' written-back (h, c) at the mini-batch's rows, every other row bitwise unchanged;
  b. _one from a preset optimiser state (steps (6, 9), m and v on the gradient's scale), clip at 0.25 x the smaller norm:
     parameter step, m, v, counters, cursor, normaliser slot 1;
  c. (`second`) _one on mini-batch 1 right after, a partial tile that holds items of mini-batch 0 again: the reference
     starts from the state the GPU left;
  d. (`epoch`) a whole epoch of three mini-batches (partial tail) through PPO._ppo_batch_train with use_graphs=True and
     graphs of one mini-batch: parameters, m, v against the float64 chain; four launches per eager mini-batch.
Bound per tensor: |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| (ko.deviations); no element is left
out.  relu / leaky_relu cases: the seed was chosen on the CPU so that no activation argument of the float64 reference
lies within 1e-4 of its row's scale of zero, which the test asserts before it compares.

Worst deviation / bound per case, one run of this file on the MI355X:
  h128_s16_b33_in256     0.272  gradient: actor.bias_hh_l1
  h128_s1_b2_gau8        0.259  clip step: critic.weight_hh_l0
  h128_s2_b16_mse        0.258  clip step: actor.weight_hh_l1
  h128_s5_b17            0.263  clip step: critic.weight_hh_l0
  h32_epoch              0.649  epoch v: critic.bias_ih_l1
  h32_s16_b33_leaky      0.256  clip step: critic.weight_hh_l1
  h32_s1_b17_in1         0.256  clip step: critic.bias_ih_l0
  h32_s2_b2_relu         0.250  clip step: actor.weight_ih_l0
  h32_s5_b16             0.250  clip step: actor.weight_ih_l0
  h64_s16_b16_in256      0.349  gradient: actor.bias_ih_l1
  h64_s2_b33_d2          0.259  clip step: critic.weight_ih_l1
  h64_s5_b17_gau8        0.276  second gradient: actor.weight_ih_l0
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import k12_oracle as ko
from oracle import lstm_update_oracle as lo

pytestmark = pytest.mark.gpu

E, VN, STEPS0, LR = 4, (0.3, 0.25, 5000.0), (6, 9), 3e-4
ACTS = {"relu": nn.ReLU, "leaky_relu": nn.LeakyReLU, "tanh": nn.Tanh}
TABLES = ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell")
CAT, GAU = "categorical", "gaussian"


def case(H=32, S=5, B=16, I=5, depth=1, F=16, head=(CAT, 3), act="tanh", huber=True, norm_adv=True, norm_values=True,
         second=False, epoch=False, seed=0):
    return dict(H=H, S=S, B=B, I=I, depth=depth, F=F, head=head, act=act, huber=huber, norm_adv=norm_adv,
                norm_values=norm_values, second=second, epoch=epoch, seed=seed)


CASES = {
    "h32_s5_b16": case(second=True, seed=1),
    "h32_s1_b17_in1": case(S=1, B=17, I=1, head=(CAT, 2), huber=False, seed=2),
    "h32_s2_b2_relu": case(S=2, B=2, F=16, head=(GAU, 1), act="relu", seed=3),
    "h32_s16_b33_leaky": case(S=16, B=33, I=17, depth=2, F=16, head=(CAT, 8), act="leaky_relu", norm_adv=False, seed=364),
    "h64_s5_b17_gau8": case(H=64, B=17, I=17, F=128, head=(GAU, 8), second=True, seed=5),
    "h64_s2_b33_d2": case(H=64, S=2, B=33, depth=2, F=16, head=(CAT, 2), norm_values=False, seed=6),
    "h64_s16_b16_in256": case(H=64, S=16, I=256, F=128, depth=2, head=(GAU, 1), huber=False, seed=7),
    "h128_s5_b17": case(H=128, B=17, F=128, head=(CAT, 8), seed=8),
    "h128_s1_b2_gau8": case(H=128, S=1, B=2, I=17, depth=2, F=16, head=(GAU, 8), norm_adv=False, seed=9),
    "h128_s16_b33_in256": case(H=128, S=16, B=33, I=256, depth=2, F=128, head=(GAU, 1), norm_values=False, seed=10),
    "h128_s2_b16_mse": case(H=128, S=2, I=1, F=128, head=(CAT, 2), huber=False, seed=11),
    "h32_epoch": case(B=16, epoch=True, seed=12),
}


def _check(name, what, got, want64, want32, tables):
    tensor, frac, _ = max(ko.deviations(got, want64, want32, tables), key=lambda d: d[1])
    print(f"{name:22s} {what:28s} {frac:.3f} ({tensor})")      # (-s: the docstring's figures)
    bad = ko.failures(got, want64, want32, tables)
    assert not bad, f"{name} / {what}: " + "; ".join(bad[:6])


def _vec(what, n):
    return [("", what, 0, (int(n),))]


def _layout(c):
    """[(tag, name, offset, shape)] of the policy's bucket (module order, each tensor padded to 4 floats, log_std behind the
    actor), its size and the actor's part: what the test asserts of the policy it builds."""
    H, I, F, D, (head, O) = c["H"], c["I"], c["F"], c["depth"], c["head"]
    rows, off = [], 0
    for tag, out in (("actor", O), ("critic", 1)):
        shapes = [(f"{w}_l{l}", (4 * H, (I if l == 0 else H) if w == "weight_ih" else H) if w[0] == "w" else (4 * H,))
                  for l in range(2) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        shapes += [("layer_norm.weight", (H,)), ("layer_norm.bias", (H,))]
        for l in range(D + 1):
            i, o = (H if l == 0 else F), (out if l == D else F)
            shapes += [(f"ff{l}.weight", (o, i)), (f"ff{l}.bias", (o,))]
        if tag == "actor" and head == GAU:
            shapes.append(("log_std", (O,)))
        for name, shape in shapes:
            rows.append((tag, name, off, shape))
            off += (int(np.prod(shape)) + 3) // 4 * 4
        if tag == "actor":
            na = off
    return dict(tables=rows, size=off, na=na)


class _Net(nn.Module):
    """nn.LSTM(I, H, 2) -> LayerNorm -> activation -> Linear head holding the given tensors, in `dtype`."""

    def __init__(self, shapes, values, act, dtype):
        super().__init__()
        H, I = shapes[1][1], shapes[0][1]
        dims = [(s[1], s[0]) for s in shapes[10::2]]
        self.mods = nn.ModuleList([nn.LSTM(I, H, 2), nn.LayerNorm(H)] + [nn.Linear(i, o) for i, o in dims]).to(dtype)
        self.act = ACTS[act]()
        with torch.no_grad():
            for p, v in zip(self.mods.parameters(), values):
                p.copy_(torch.as_tensor(v, dtype=dtype).reshape(p.shape))

    def forward(self, x, h0, c0):
        """x [B, S, I], h0 / c0 [B, 2, H] -> (out, h_n [B, 2, H], c_n, the activations' arguments)."""
        _, (hn, cn) = self.mods[0](x.transpose(0, 1), (h0.transpose(0, 1).contiguous(), c0.transpose(0, 1).contiguous()))
        z = self.mods[1](hn[-1])
        pre = [z]
        for lin in self.mods[2:-1]:
            z = lin(self.act(z))
            pre.append(z)
        return self.mods[-1](self.act(z)), hn.transpose(0, 1), cn.transpose(0, 1), pre


def _reference(c, lay, params, tabs, items, vn, dtype):
    """One mini-batch over dataset-position tables `tabs` from the flat bucket `params`: lo.minibatch's text around _Net."""
    S, head = c["S"], c["head"][0]
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    seg = lambda rows: [params[o:o + int(np.prod(s))] for _, _, o, s in rows]
    arows, crows = [t for t in lay["tables"] if t[0] == "actor"], [t for t in lay["tables"] if t[0] == "critic"]
    nets = [r for r in arows if r[1] != "log_std"]
    am, cm = _Net([r[3] for r in nets], seg(nets), c["act"], dtype), _Net([r[3] for r in crows], seg(crows), c["act"], dtype)
    aparams, log_std = list(am.mods.parameters()), None
    if head == GAU:
        log_std = nn.Parameter(T(seg([arows[-1]])[0]))
        aparams.append(log_std)
    pos = np.asarray(items)[:, None] + np.arange(S)[None, :]
    last = pos[:, -1]
    mask = torch.as_tensor(lo.window_mask(tabs["term"][pos]))
    out, ah, ac, apre = am(T(tabs["obs"][pos]).masked_fill(mask.unsqueeze(-1), 0.0), T(tabs["actor_hidden"][last]), T(tabs["actor_cell"][last]))
    val, ch, cc, cpre = cm(T(tabs["cobs"][pos]), T(tabs["critic_hidden"][last]), T(tabs["critic_cell"][last]))
    raw = tabs["raw_actions"][last]
    logp, ent = ko._head_terms(head, out, log_std, T(raw if head == GAU else raw.reshape(-1)), (), 0.01, {})
    r = np.asarray(tabs["rewards_to_go"][last], dtype=np.float64)
    rtg, vn1 = T(r), None
    if c["norm_values"]:
        rtg, vn1 = ko.normalised_rtg(r, vn, [(len(r), r.mean(), ((r - r.mean()) ** 2).sum())], dtype)
    a_loss, c_loss, totals = ko.losses(logp.reshape(-1), T(tabs["log_probs"][last]), T(tabs["advantages"][last]), ent.reshape(-1),
                                       val.reshape(-1), rtg.reshape(-1), c["norm_adv"], 0.2, 0.01, 0.0, c["huber"], 10.0)
    grads = np.zeros(lay["size"])
    for (_, _, off, _), g in zip(lay["tables"], torch.autograd.grad(a_loss, aparams) + torch.autograd.grad(c_loss, list(cm.mods.parameters()))):
        grads[off:off + g.numel()] = g.double().numpy().reshape(-1)
    n64 = lambda t: t.detach().double().numpy()
    margin = min(float((p.detach().abs().min(1).values / p.detach().abs().max(1).values).min()) for p in apre + cpre)
    return dict(totals=totals, grads=grads, values=n64(val).reshape(-1), logp=n64(logp).reshape(-1), vn=vn1, margin=margin,
                actor_hidden=n64(ah), actor_cell=n64(ac), critic_hidden=n64(ch), critic_cell=n64(cc))


def _steer(c, lay, N):
    """The case's tables in dataset-position order and its permutation, from the CPU seed alone."""
    S, B, H, (head, O) = c["S"], c["B"], c["H"], c["head"]
    rng = np.random.default_rng(c["seed"])
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    p = np.zeros(lay["size"])
    for _, name, off, shape in lay["tables"]:
        n = int(np.prod(shape))
        sd = 0.9 / np.sqrt(shape[1]) if len(shape) == 2 else 0.3 if name == "log_std" else 0.1
        p[off:off + n] = rng.normal(0.0, sd, n) + (1.0 if name == "layer_norm.weight" else 0.0)
    items = N - (S - 1)
    t = dict(obs=f32(rng.normal(0, 1, (N, c["I"]))), cobs=f32(rng.normal(0, 1, (N, c["I"]))), term=np.zeros(N, dtype=bool),
             advantages=f32(rng.normal(0.2, 1.0, N)), rewards_to_go=f32(0.3 + 0.5 * rng.normal(0, 1, N)), log_probs=np.zeros(N, np.float32),
             raw_actions=f32(rng.normal(0, 1.5, (N, O))) if head == GAU else rng.integers(0, O, (N, 1)).astype(np.int64),
             **{k: f32(0.5 * rng.normal(0, 1, (N, 2, H))) for k in TABLES})
    # ONE byte, at position `at`, gives a window of every kind: item at (byte at step 0), at - (S - 2) (byte at S - 2),
    # at - (S - 1) (only at S - 1); then one window with none, and whatever the draw brings (bytes at the steps between)
    special = []
    if S > 1:
        at = max(S - 1, items // 2)
        t["term"][at] = True
        special = list(dict.fromkeys((at, at - (S - 2), at - (S - 1))))[:B - 1]
    rest = [i for i in rng.permutation(items) if i not in special]
    clean = [i for i in rest if not t["term"][i:i + S].any()][:1]
    first = special + clean + [i for i in rest if i not in clean][:B - len(special) - 1]
    others = [i for i in rest if i not in first]
    if c["second"]:                                              # mini-batch 1 (the items behind B) holds two of mini-batch 0 again
        others = first[-2:] + others[:-2]
    perm = np.asarray(first + others, dtype=np.int64)
    t["rewards_to_go"][perm[0] + S - 1] = np.float32(0.3 + 12.0)             # (normalised: Huber's linear branch)
    logp = _reference(c, lay, f32(p).astype(np.float64), t, np.arange(items), VN, torch.float64)["logp"]
    t["log_probs"][S - 1:] = ko.steered_old_log_probs(logp, rng, 0.2)
    t["log_probs"][perm[:2] + S - 1] = f32(logp[perm[:2]] - np.log([0.65, 1.45]))
    t["advantages"][perm[:2] + S - 1] = np.abs(t["advantages"][perm[:2] + S - 1]) * f32([1.0, -1.0])
    return f32(p).astype(np.float64), t, perm


def _items(c):
    return E * -(-((2 * c["B"] + 4 if c["epoch"] else c["B"] + 8) + c["S"] - 1) // E)


class Steered:
    def __init__(self, c, monkeypatch):
        from ppo_and_friends_amd.ppo import PPO
        from ppo_and_friends_amd.networks.lstm import LSTMNetwork
        from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
        from ppo_and_friends_amd.fused_update import FusedLstm2Update, FusedLstmUpdate
        from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
        from ppo_and_friends_amd.spaces import Box, Discrete
        monkeypatch.setattr(PPOPolicy, "fused_lstm_layers", True)
        monkeypatch.setattr(PPOPolicy, "fused_lstm_layers_update", True)
        dev = torch.device("cuda", 0)
        S, B, H, I, (head, O) = c["S"], c["B"], c["H"], c["I"], c["head"]
        T = _items(c) // E
        space, sp = (Discrete(O) if head == CAT else Box(-1.0, 1.0, (O,), np.float32)), Box(-np.inf, np.inf, (I,), np.float32)
        kw = dict(sequence_length=S, lstm_hidden_size=H, num_lstm_layers=2, ff_hidden_size=c["F"], ff_hidden_depth=c["depth"])
        pargs = dict(ac_network=LSTMNetwork, actor_kw_args=dict(kw, activation=ACTS[c["act"]]()),
                     critic_kw_args=dict(kw, activation=ACTS[c["act"]]()), use_huber_loss=c["huber"])
        env_gen = lambda: SyntheticFixedLengthEnv(E, I, space, T, dev, reward="uniform", seed=13, term_prob=0.05)
        self.ppo = ppo = PPO(env_gen, {"p": (None, sp, sp, space, pargs)}, device=dev, random_seed=1, normalize_obs=False,
                             normalize_rewards=False, normalize_adv=c["norm_adv"], normalize_values=c["norm_values"],
                             envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1, max_ts_per_ep=7, save_state=False,
                             update_mode="fused", use_graphs=c["epoch"])
        pol = self.pol = ppo.policies["p"]
        assert FusedLstmUpdate.unsupported_reason(pol, B) == ""
        ppo.rollout()
        pol.train()
        buf, ds = pol.buffer, pol.dataset
        self.N = N = buf.num_transitions
        self.lay = lay = _layout(c)
        base = pol.policy_params.data_ptr()
        mods = pol.actor._hip_params() + ([pol.actor.distribution.log_std] if head == GAU else []) + pol.critic._hip_params()
        assert [((p.data_ptr() - base) // 4, tuple(p.shape)) for p in mods] == [(o, tuple(sh)) for _, _, o, sh in lay["tables"]]
        assert lay["size"] == pol.policy_params.numel() and lay["na"] == pol.actor.bucket_size()
        self.pad = np.ones(lay["size"], dtype=bool)
        for _, _, off, shape in lay["tables"]:
            self.pad[off:off + int(np.prod(shape))] = False
        self.params, self.t, perm = _steer(c, lay, N)
        assert float(pol.policy_lr[0]) == np.float32(LR) and len(ds) == N - (S - 1)
        self.upd = ppo._fused_updater("p", B)
        assert isinstance(self.upd, FusedLstm2Update)
        self.rows = ds.row_map.long()
        flat = self._flat = lambda x: x.view((N,) + tuple(x.shape[2:]))
        dt = lambda x, like: torch.as_tensor(x).to(device=dev, dtype=like.dtype)
        with torch.no_grad():
            pol.policy_params.copy_(dt(self.params, pol.policy_params))
        for field, k in (("observations", "obs"), ("critic_observations", "cobs"), ("raw_actions", "raw_actions"),
                         ("advantages", "advantages"), ("rewards_to_go", "rewards_to_go"), ("log_probs", "log_probs")):
            x = getattr(buf, field)
            flat(x)[self.rows] = dt(self.t[k], x).reshape((N,) + tuple(x.shape[2:]))
        for k in TABLES:
            assert tuple(flat(buf.hidden[k]).shape) == (N, 2, H)
            flat(buf.hidden[k])[self.rows] = dt(self.t[k], buf.hidden[k])
        if S > 1:
            ds.terminal_positions.copy_(dt(self.t["term"], ds.terminal_positions))
        if c["norm_values"]:
            rs = ppo.value_normalizers["p"].running_stats
            rs.mean_t.fill_(VN[0]); rs.var_t.fill_(VN[1]); rs.count_t.fill_(VN[2])
        self.vn = VN if c["norm_values"] else (0.0, 1.0, 1e-4)
        self.perm = torch.as_tensor(perm, dtype=torch.int64, device=dev)
        self.keep = dict({k: buf.hidden[k].clone() for k in TABLES}, values=buf.values.clone())

    def tables_now(self):
        """The reference's tables with the hidden states the GPU holds now."""
        return dict(self.t, **{k: self._flat(self.pol.buffer.hidden[k])[self.rows].cpu().numpy() for k in TABLES})

    def state(self):
        pol = self.pol
        return [x.detach().double().cpu().numpy() for x in (pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq)]

    def check_written(self, name, tag, items, r64, r32, before):
        pol, N = self.pol, self.N
        rows = self.rows[torch.as_tensor(np.asarray(items) + self.ppo.policies["p"].actor.sequence_length - 1, device=self.rows.device)]
        other = torch.ones(N, dtype=torch.bool, device=rows.device)
        other[rows] = False
        for k in TABLES + ("values",):
            x = pol.buffer.values if k == "values" else pol.buffer.hidden[k]
            x, b = x.view(N, -1), before[k].view(N, -1)
            _check(name, f"{tag} {k}", x[rows].cpu().numpy(), r64[k], r32[k], _vec(k, r64[k].size))
            assert torch.equal(x[other], b[other]), f"{tag}: {k} rows outside the mini-batch changed"

    def check_step(self, name, tag, r64, r32, p0, m0, v0, steps0, max_norm):
        na = self.lay["na"]
        grads = self.pol.policy_grads.detach().double().cpu().numpy()
        assert not grads[self.pad].any(), f"{name} / {tag}: padding of the gradient bucket written"
        _check(name, f"{tag} gradient", grads, r64["grads"], r32["grads"], self.lay["tables"])
        want = ko.clip_adam(p0, r64["grads"], m0, v0, steps0, LR, max_norm, na)
        want32 = ko.clip_adam(p0, r32["grads"], m0, v0, steps0, LR, max_norm, na, dtype=torch.float32)
        p, m, v = self.state()
        for what, g, w, w32 in (("step", p - p0, want[0] - p0, want32[0] - p0), ("m", m, want[1], want32[1]), ("v", v, want[2], want32[2])):
            _check(name, f"{tag} {what}", g, w, w32, self.lay["tables"])
        assert (self.pol.policy_step_counts.cpu().numpy() == np.array(steps0) + 1).all(), f"{name} / {tag}: step counters"


def _fold(upd, c, B):
    n_wg = (B + 15) // 16
    lp = upd.loss_partials.view(-1)[:2 * n_wg * 8].view(2, n_wg, 8).double().cpu().numpy()
    surr, ent, kl, crit = lp[0, :, 0].sum() / B, lp[0, :, 3].sum() / B, lp[0, :, 4].sum() / B, lp[1, :, 2].sum() / B
    return [surr, surr - 0.01 * ent, crit, ent, kl, lp[0, 0, 5], lp[0, 0, 6], float(lp[0, :, 7].sum() > 0)]


def _epoch(name, c, st):
    """d. three mini-batches through the public path against the float64 chain of the same three."""
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol, ppo, B, S = st.pol, st.ppo, c["B"], c["S"]
    items = st.N - (S - 1)
    assert items // B == 2 and items % B >= 2
    st.upd.graph_chunk = 1                                       # mini-batch 0 is warm-up + capture, mini-batch 1 a replay
    chain = {}
    for dtype in (torch.float64, torch.float32):
        (p, m, v), tabs, vn, steps = st.state(), st.tables_now(), st.vn, tuple(int(x) for x in pol.policy_step_counts.cpu())
        for k in range(3):
            mb = st.perm.cpu().numpy()[k * B:(k + 1) * B]
            r = _reference(c, st.lay, p, tabs, mb, vn, dtype)
            p, m, v = ko.clip_adam(p, r["grads"], m, v, steps, LR, float(pol.gradient_clip), st.lay["na"], dtype=dtype)
            for t in TABLES:
                tabs[t] = tabs[t].copy()
                tabs[t][mb + S - 1] = r[t].astype(np.float32)
            vn, steps = (r["vn"] if c["norm_values"] else vn), tuple(x + 1 for x in steps)
        chain[dtype] = (p, m, v)
    before = FusedLstmUpdate.launches
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator, {"n": items, "perm": st.perm.cpu()})
    ppo._ppo_batch_train(loader, "p")
    torch.cuda.synchronize()
    assert FusedLstmUpdate.launches - before == 4 * 3            # warm-up, capture pass and the tail; the replay counts none
    for what, g, w, w32 in zip(("params", "m", "v"), st.state(), chain[torch.float64], chain[torch.float32]):
        _check(name, f"epoch {what}", g, w, w32, st.lay["tables"])
    assert (pol.policy_step_counts.cpu().numpy() == 3).all() and int(st.upd.cursor.item()) == 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_stacked_update_minibatch_against_float64(name, monkeypatch):
    c = CASES[name]
    st = Steered(c, monkeypatch)
    pol, upd, B, S = st.pol, st.upd, c["B"], c["S"]
    chosen = st.perm.cpu().numpy()[:B]
    if S > 1 and B >= 4:                                         # the four kinds of window are among the first B items
        w = st.t["term"][chosen[:, None] + np.arange(S)]
        kinds = (w[:, 0], w[:, S - 2], w[:, S - 1] & ~w[:, :S - 1].any(1), ~w.any(1))
        assert all(k.any() for k in kinds), f"{name}: windows with a byte at 0 / S-2 / only S-1 / none: {[int(k.sum()) for k in kinds]}"
    if c["epoch"]:
        return _epoch(name, c, st)
    r64, r32 = (_reference(c, st.lay, st.params, st.t, chosen, st.vn, d) for d in (torch.float64, torch.float32))
    if c["act"] != "tanh":
        assert r64["margin"] > 1e-4, f"an activation argument at {r64['margin']:.2e} of its row's scale: choose another seed"
    ratio = np.exp(r64["logp"] - st.t["log_probs"][chosen + S - 1])
    assert (ratio < 0.8).any() and (ratio > 1.2).any(), "ratios on both sides of the clip"
    # ---- a. the gradient of one mini-batch
    upd.begin_epoch(st.perm)
    upd.gradient_only(upd._args_for(B))
    torch.cuda.synchronize()
    grads = pol.policy_grads.detach().double().cpu().numpy()
    assert not grads[st.pad].any(), f"{name}: padding of the gradient bucket written"
    _check(name, "gradient", grads, r64["grads"], r32["grads"], st.lay["tables"])
    _check(name, "totals", _fold(upd, c, B), r64["totals"], r32["totals"], [("", "totals", 0, (8,))])
    st.check_written(name, "gradient_only", chosen, r64, r32, st.keep)
    assert int(upd.cursor.item()) == 0
    # ---- b. one full mini-batch from a non-zero optimiser state with the clip active
    g, na = r64["grads"], st.lay["na"]
    rng = np.random.default_rng(c["seed"] + 1)
    rms = np.sqrt(np.mean(g * g)) + 1e-12
    m0 = np.where(st.pad, 0.0, 0.5 * g + rng.normal(0, 0.1 * rms, g.size)).astype(np.float32)
    v0 = np.where(st.pad, 0.0, g * g * rng.uniform(0.5, 2.0, g.size) + (0.1 * rms) ** 2).astype(np.float32)
    max_norm = float(np.float32(0.25 * min(np.sqrt((g[:na] ** 2).sum()), np.sqrt((g[na:] ** 2).sum()))))
    pol.gradient_clip = max_norm
    for k in TABLES:
        pol.buffer.hidden[k].copy_(st.keep[k])
    pol.buffer.values.copy_(st.keep["values"])
    pol.policy_exp_avg.copy_(torch.from_numpy(m0)); pol.policy_exp_avg_sq.copy_(torch.from_numpy(v0))
    pol.policy_step_counts.copy_(torch.tensor(STEPS0))
    upd.begin_epoch(st.perm)
    upd._one(upd._args_for(B))
    torch.cuda.synchronize()
    st.check_step(name, "clip", r64, r32, st.params, m0, v0, STEPS0, max_norm)
    tot = upd.totals.cpu().numpy()
    _check(name, "clip totals", tot[:8], r64["totals"], r32["totals"], [("", "totals", 0, (8,))])
    assert tot[8] == 1.0 and int(upd.cursor.item()) == 1, f"{name}: mini-batch count / cursor"
    if c["norm_values"]:
        _check(name, "normaliser", [float(upd.vn_mean[1]), float(upd.vn_var[1]), float(upd.vn_count[1])], r64["vn"], r32["vn"], None)
    st.check_written(name, "_one", chosen, r64, r32, st.keep)
    # ---- c. mini-batch 1 right after, a partial tile: the other normaliser slot, states that mini-batch 0 wrote back
    if c["second"]:
        mb1 = st.perm.cpu().numpy()[B:]                          # (its records are those of the whole remainder)
        L = len(mb1)
        assert 2 <= L < 16 and set(mb1.tolist()) & set(chosen.tolist())
        (p1, m1, v1), tabs = st.state(), st.tables_now()
        before1 = dict({k: pol.buffer.hidden[k].clone() for k in TABLES}, values=pol.buffer.values.clone())
        vn1 = (float(upd.vn_mean[1]), float(upd.vn_var[1]), float(upd.vn_count[1])) if c["norm_values"] else st.vn
        q64, q32 = (_reference(c, st.lay, p1, tabs, mb1, vn1, d) for d in (torch.float64, torch.float32))
        upd._one(upd._args_for(L))
        torch.cuda.synchronize()
        st.check_step(name, "second", q64, q32, p1, m1, v1, tuple(x + 1 for x in STEPS0), max_norm)
        assert int(upd.cursor.item()) == 2 and upd.totals.cpu().numpy()[8] == 2.0
        if c["norm_values"]:
            _check(name, "second normaliser", [float(upd.vn_mean[0]), float(upd.vn_var[0]), float(upd.vn_count[0])], q64["vn"], q32["vn"], None)
        st.check_written(name, "second", mb1, q64, q32, before1)
