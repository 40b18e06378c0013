"""
ONE K14 mini-batch (csrc/icm_update.hip, csrc/icm_update_shapes.hip) in float64: the reference, the bound and the cases
shared by tests/test_gpu_icm_float64.py (the kernels against it) and tests/test_icm_float64_oracle.py (the float32 oracle
against it, planted errors against it; no GPU).

The reference is autograd on oracle/icm_oracle.ICM in `.double()` -- pinned by g10_icm / g12_* / g17 -- in the forms the
sibling helpers build: the identity encoder (icm_identity.oracle_icm) and MultiDiscrete actions (ICM(nvec=...),
icm_shared.oracle_shared_icm).  A case is built on the CPU from its shapes and a seed: orthogonal weights as the reference
initialises them, biases N(0, 0.1) (zero biases would hide a bias-gradient or a bias-add error of the hidden layers behind
ReLU's symmetric halves), observations N(0, 1), every action class present, continuous actions over [-1, 1] with some at
the bounds.  Rows with a ReLU / LeakyReLU pre-activation within 1e-4 x the row's scale of zero are drawn again.

Bound (oracle/k12_oracle.deviations, the project's rule): per tensor |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to
4 max|x32 - x64| where the same oracle in float32 on the CPU cannot do better.  A tensor that is identically zero in
float64 (icm_beta 0 / 1) therefore has the bound 0: exactly zero, and finite.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import cpu_ppo_loop, icm_oracle
from oracle import k12_oracle as ko

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icm_identity import oracle_icm  # noqa: E402
from icm_shared import oracle_shared_icm  # noqa: E402

ACTIVATIONS = ("relu", "leaky_relu", "tanh")
ROW_MODES = ("perm", "tail", "order", "agents")
REWARD_SCALE = 0.01
LOSS = [("", "loss", 0, (1,))]


# ------------------------------------------------------------------------------------------------------------ cases
def case(chain, O, B, widths, depths=(2, 2), action=("discrete", 3), act="relu", beta=0.2, rows="perm", seed=0):
    """chain "one_width": widths = H.  "shapes": widths = (E, D, Mi, Mf).  "identity": widths = (Mi, Mf).
    action: ("discrete", classes) | ("continuous", dims) | ("multi", (slices, classes)).
    rows (how the harness addresses the mini-batch's rows):
      perm    a random perm over n_rows > B and a random injective row_map, cursor 0
      tail    the same with cursor 2, batch_stride = B + 7: a tail of B rows behind two full mini-batches
      order   inputs_in_batch_order 1, perm = row_map = NULL, cursor 1, batch_stride = B + 3 (grouped / shared tables)
      agents  the same with B = 3 n and batch_stride = B (the (row, agent) samples of a MAT policy of three agents)"""
    assert chain in ("one_width", "shapes", "identity") and act in ACTIVATIONS and rows in ROW_MODES
    assert rows != "agents" or B % 3 == 0
    return dict(chain=chain, O=O, B=B, widths=widths, depths=tuple(depths), action=action, act=act, beta=beta, rows=rows,
                seed=seed)


def action_dims(c):
    """(inverse-model outputs = forward-model action columns, discrete?, nvec or None)."""
    kind, n = c["action"]
    if kind == "multi":
        k, classes = n
        return k * classes, True, [classes] * k
    return n, kind == "discrete", None


def label(c):
    """The chain as the report names it: MultiDiscrete slices are forms of their own."""
    return c["chain"] + ("_md" if c["action"][0] == "multi" else "")


_ACTIONS = [("discrete", 2), ("continuous", 1), ("discrete", 3), ("continuous", 2), ("discrete", 8), ("continuous", 6),
            ("continuous", 8)]
_DEPTHS = [(i, f) for i in (1, 2, 3) for f in (1, 2, 3)]
_MULTI = [(2, 2), (8, 2), (2, 8), (4, 4), (5, 3), (3, 5)]


def _cases():
    out = {}
    rot = lambda seq, i: seq[i % len(seq)]
    fit = lambda B, rows: B + (-B) % 3 if rows == "agents" else B          # "agents": the next multiple of three
    # ---- one-width chain.  obs_dim edges (the input tile is padded to 16 columns); H alternates
    for i, (O, B) in enumerate(zip((1, 15, 16, 17, 63, 64, 65, 128, 376, 1024), (17, 33, 31, 18, 17, 33, 21, 48, 17, 19))):
        out[f"ow_in{O}"] = case("one_width", O, B, 64 if i % 2 == 0 else 128, action=rot(_ACTIONS, i), act=rot(ACTIVATIONS, i),
                                beta=(0.2, 0.8)[i % 2], rows=rot(ROW_MODES, i), seed=100 + O)
    # batch edges: ragged tiles, the encoder jobs' second operand trip above 256, the single launch up to 512 (H 128)
    modes = dict(zip((1, 2, 15, 16, 17, 31, 33, 255, 256, 257, 512, 513, 528),
                     ("perm", "tail", "agents", "order", "tail", "perm", "agents", "order", "perm", "tail", "order", "agents",
                      "perm")))
    for i, (B, rows) in enumerate(modes.items()):
        out[f"ow_B{B}"] = case("one_width", 6, B, 64 if B in (2, 15, 16, 31) else 128, action=rot(_ACTIONS, i + 3),
                               act=rot(ACTIVATIONS, i + 1), beta=(0.8, 0.2)[i % 2], rows=rows, seed=200 + B)
    for i, d in enumerate(_DEPTHS):
        rows = rot(ROW_MODES, i + 1)
        out[f"ow_d{d[0]}{d[1]}"] = case("one_width", 5, fit((19, 35)[i % 2], rows), 64, depths=d, action=rot(_ACTIONS, i + 1),
                                        act=rot(ACTIVATIONS, i + 2), beta=(0.2, 0.8)[i % 2], rows=rows, seed=300 + i)
    out["ow_beta0"] = case("one_width", 7, 21, 128, action=("discrete", 3), beta=0.0, rows="perm", seed=401)
    out["ow_beta1"] = case("one_width", 7, 21, 64, action=("continuous", 2), act="tanh", beta=1.0, rows="order", seed=402)
    # ---- shapes chain.  (E, Mi, Mf): the six orders of (32, 64, 128) hold every unequal ordered pair in every pair of
    # roles; four more with equal neighbours.  D edges ride on them
    triples = [(32, 64, 128), (64, 128, 32), (128, 32, 64), (32, 128, 64), (64, 32, 128), (128, 64, 32), (32, 32, 32),
               (64, 64, 128), (128, 32, 32), (128, 128, 64)]
    for i, (D, (E, Mi, Mf)) in enumerate(zip((1, 15, 16, 17, 31, 32, 33, 64, 127, 128), triples)):
        rows = rot(ROW_MODES, i)
        out[f"sh_D{D}"] = case("shapes", 9, fit((17, 33, 21)[i % 3], rows), (E, D, Mi, Mf), action=rot(_ACTIONS, i + 2),
                               act=rot(ACTIVATIONS, i), beta=(0.2, 0.8)[i % 2], rows=rows, seed=500 + D)
    for i, (B, O) in enumerate(((1, 1), (17, 17), (33, 65), (257, 376), (528, 6))):
        out[f"sh_B{B}_in{O}"] = case("shapes", O, B, rot(triples, i + 1)[:1] + (9,) + rot(triples, i + 1)[1:],
                                     action=rot(_ACTIONS, i), act=rot(ACTIVATIONS, i + 1), beta=(0.8, 0.2)[i % 2],
                                     rows=("perm", "tail", "agents", "tail", "agents")[i], seed=600 + B)
    for i, (k, n) in enumerate(_MULTI):
        E, Mi, Mf = rot(triples, i + 3)
        out[f"sh_md{k}x{n}"] = case("shapes", 10, (21, 33)[i % 2], (E, (9, 16, 40)[i % 3], Mi, Mf), action=("multi", (k, n)),
                                    act=rot(ACTIVATIONS, i), beta=(0.2, 0.8)[i % 2], rows=rot(ROW_MODES, i + 2), seed=700 + i)
    for i, d in enumerate(_DEPTHS):
        rows, widths = rot(ROW_MODES, i + 3), (64, 12, (32, 64, 128)[i % 3], (64, 128, 32)[i % 3])
        out[f"sh_d{d[0]}{d[1]}"] = case("shapes", 5, fit((19, 35)[i % 2], rows), widths, depths=d, action=rot(_ACTIONS, i),
                                        act=rot(ACTIVATIONS, i + 1), beta=(0.8, 0.2)[i % 2], rows=rows, seed=800 + i)
    out["sh_beta0"] = case("shapes", 7, 21, (64, 20, 32, 64), action=("continuous", 3), beta=0.0, rows="tail", seed=901)
    out["sh_beta1"] = case("shapes", 7, 21, (32, 20, 64, 32), action=("discrete", 4), act="leaky_relu", beta=1.0, rows="agents",
                           seed=902)
    # ---- identity form: Mi != Mf, depths 1 and 3, every action kind, B 17 and 257
    pairs = [(32, 64), (64, 128), (128, 32), (64, 32), (32, 128), (128, 64)]
    kinds = [("discrete", 3), ("continuous", 2), ("multi", (2, 2)), ("discrete", 8), ("continuous", 8), ("multi", (5, 3)),
             ("multi", (2, 8)), ("discrete", 2)]
    for i, O in enumerate((1, 2, 15, 16, 17, 64, 127, 128)):
        rows = rot(ROW_MODES, i)
        B = (17, 257)[i % 2] if rows != "agents" else (18, 258)[i % 2]
        out[f"id_in{O}"] = case("identity", O, B, rot(pairs, i), depths=((1, 3), (3, 1), (1, 1), (3, 3))[i % 4],
                                action=kinds[i], act=rot(ACTIVATIONS, i), beta=(0.2, 0.8)[i % 2], rows=rows, seed=1000 + O)
    out["id_beta0"] = case("identity", 11, 17, (64, 32), action=("multi", (4, 4)), beta=0.0, rows="order", seed=1101)
    out["id_beta1"] = case("identity", 11, 17, (32, 64), action=("continuous", 1), act="tanh", beta=1.0, rows="perm", seed=1102)
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------------- the oracle
def build_oracle(c):
    """oracle/icm_oracle.ICM of the case in float32: the reference's initialisation under the case's seed, then biases
    N(0, 0.1)."""
    A, discrete, nvec = action_dims(c)
    d_inv, d_fwd = c["depths"]
    O, act = c["O"], c["act"]
    torch.manual_seed(c["seed"])
    if c["chain"] == "identity":
        Mi, Mf = c["widths"]
        if nvec is None:
            m = oracle_icm(O, A, discrete, Mi, Mf, d_inv, d_fwd, activation=act)
        else:
            m = oracle_shared_icm(O, nvec, dict(identity=True, Mi=Mi, Mf=Mf, d_inv=d_inv, d_fwd=d_fwd, activation=act))
    else:
        E, D, Mi, Mf = (c["widths"],) * 4 if c["chain"] == "one_width" else c["widths"]
        m = icm_oracle.ICM(O, A, discrete, reward_scale=REWARD_SCALE, enc=D, hidden=Mi, enc_hidden=E, inv_depth=d_inv,
                           fwd_depth=d_fwd, nvec=nvec, activation=act)
        if Mf != Mi:                               # a forward model of its own width, as icm_identity.oracle_icm builds it
            m.forward_model.sequential_net = cpu_ppo_loop.make_mlp(D + A, D, Mf, d_fwd, out_gain=1.0,
                                                                   activation=icm_oracle.activation_module(act))
    assert m.reward_scale == REWARD_SCALE
    gen = torch.Generator().manual_seed(c["seed"] + 7)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    return m


def tables(model):
    """[(tag, name, offset, shape)] of the flat bucket -- the parameters in module order, each padded to 4 floats, what
    fused_update._icm_bucket_marks checks of the package's ICM -- and the bucket's size."""
    out, off = [], 0
    for name, p in model.named_parameters():
        out.append(("", name, off, tuple(p.shape)))
        off += (p.numel() + 3) // 4 * 4
    return out, off


def padding(table, size):
    used = np.zeros(size, dtype=bool)
    for _, _, off, shape in table:
        used[off:off + int(np.prod(shape))] = True
    return ~used


def _actions_tensor(c, act):
    return torch.as_tensor(act) if action_dims(c)[1] else None


def _hidden_linears(model):
    """The Linear layers whose output goes through the activation: enc_1..3 and all but the last of each model."""
    out = []
    if not isinstance(model.obs_encoder, nn.Identity):
        out += [model.obs_encoder.enc_1, model.obs_encoder.enc_2, model.obs_encoder.enc_3]
    for net in (model.inv_model.sequential_net, model.forward_model.sequential_net):
        out += [m for m in net.modules() if isinstance(m, nn.Linear)][:-1]
    return out


def kinked_rows(model64, obs1, obs2, act, rel=1e-4):
    """bool per row: a hidden pre-activation (both encoder streams, inverse model, forward model) within rel x its row's
    scale (max |z| of that layer) of zero in float64 -- ko.kinked_rows' rule.  Tanh has none."""
    bad = np.zeros(len(obs1), dtype=bool)
    if model64.activation == "tanh":
        return bad
    seen = []
    hooks = [m.register_forward_hook(lambda _m, _i, z: seen.append(z.detach().numpy())) for m in _hidden_linears(model64)]
    try:
        with torch.no_grad():
            a = torch.as_tensor(act)
            model64(torch.as_tensor(obs1, dtype=torch.float64), torch.as_tensor(obs2, dtype=torch.float64),
                    a if a.dtype == torch.int64 else a.double())
    finally:
        for h in hooks:
            h.remove()
    for z in seen:
        bad |= (np.abs(z) < rel * np.abs(z).max(axis=1, keepdims=True)).any(axis=1)
    return bad


def inputs(c, model64):
    """(obs1, obs2 float32 [B, O]; actions int64 [B, 1] / [B, slices] or float32 [B, dims]) of the case, un-kinked."""
    B, O, seed = c["B"], c["O"], c["seed"]
    rng = np.random.default_rng(seed)
    obs1 = rng.normal(0, 1, (B, O)).astype(np.float32)
    obs2 = rng.normal(0, 1, (B, O)).astype(np.float32)
    kind, n = c["action"]
    if kind == "continuous":
        act = rng.uniform(-1, 1, (B, n)).astype(np.float32)
        k = max(1, B // 8)
        act[:k] = np.where(rng.random((k, n)) < 0.5, -1.0, 1.0)
    else:
        slices, classes = n if kind == "multi" else (1, n)
        act = rng.integers(0, classes, (B, slices)).astype(np.int64)
        for j in range(slices):                                      # every class of every slice occurs (B permitting)
            first = rng.permutation(classes)[:B]
            act[:len(first), j] = first
    for r in range(50):
        bad = kinked_rows(model64, obs1, obs2, act)
        if not bad.any():
            break
        g = np.random.default_rng((seed, r))
        obs1[bad] = g.normal(0, 1, (int(bad.sum()), O))
        obs2[bad] = g.normal(0, 1, (int(bad.sum()), O))
    else:
        pytest.fail("kinked rows left after 50 redraws")
    return obs1, obs2, act


def reference(model, obs1, obs2, act, beta, dtype, keep=None, second_stream=True):
    """One mini-batch of `model` in `dtype` -> dict(loss = (1 - beta) f + beta inv; grads: every parameter gradient in the
    flat bucket order (padding zero); reward [B] = reward_scale / 2 x sum f).
    Planted errors (tests/test_icm_float64_oracle.py only): keep = a bool per row, the rows that enter the sums (the means
    still divide by B); second_stream = False takes the next-observation stream out of the encoder's weight gradients."""
    m = copy.deepcopy(model).to(dtype)
    table, size = tables(m)
    o1, o2, a = (torch.as_tensor(np.asarray(x)) for x in (obs1, obs2, act))
    scale = 1.0
    if keep is not None:
        keep = torch.as_tensor(np.asarray(keep, dtype=bool))
        scale = float(keep.sum()) / len(keep)
        o1, o2, a = o1[keep], o2[keep], a[keep]
    if not second_stream:
        enc, calls = m.obs_encoder, [0]
        inner = enc.forward

        def forward(x):
            calls[0] += 1
            y = inner(x)
            return y.detach() if calls[0] == 2 else y
        enc.forward = forward
    intr, inv, f = m(o1.to(dtype), o2.to(dtype), a if a.dtype == torch.int64 else a.to(dtype))
    loss = scale * ((1.0 - beta) * f + beta * inv)
    params = list(m.parameters())
    got = torch.autograd.grad(loss, params, allow_unused=True)
    grads = np.zeros(size, dtype=np.float64)
    for (_, _, off, shape), g in zip(table, got):
        if g is not None:
            grads[off:off + g.numel()] = g.detach().double().numpy().reshape(-1)
    return dict(loss=np.array([float(loss.detach())]), grads=grads, reward=intr.detach().double().numpy().reshape(-1))


def flat_params(model):
    table, size = tables(model)
    out = np.zeros(size, dtype=np.float64)
    for (_, _, off, _), p in zip(table, model.parameters()):
        out[off:off + p.numel()] = p.detach().double().numpy().reshape(-1)
    return out


def adam(params, grads, m0, v0, step0, lr, betas=(0.9, 0.999), eps=1e-5, dtype=torch.float64):
    """The ICM's optimiser step (ppo.py:2559-2562: torch.optim.Adam(lr, eps=1e-5), no clipping) from a non-zero state,
    step0 steps taken before: oracle/k12_oracle.clip_adam with the clip off and the whole bucket as one network.
    -> (params, exp_avg, exp_avg_sq) after the step, float64 arrays."""
    return ko.clip_adam(params, grads, m0, v0, (step0, step0), lr, 0.0, len(params), beta1=betas[0], beta2=betas[1], eps=eps,
                        dtype=dtype)


def preset_state(c, g64, pad):
    """(m0, v0) float32 on the gradient's scale, drawn as tests/test_gpu_k12_gradients.run_case draws them; padding zero."""
    rng = np.random.default_rng(c["seed"] + 1)
    rms = np.sqrt(np.mean(g64 * g64)) + 1e-12
    m0 = np.where(pad, 0.0, 0.5 * g64 + rng.normal(0, 0.1 * rms, g64.size)).astype(np.float32)
    v0 = np.where(pad, 0.0, g64 * g64 * rng.uniform(0.5, 2.0, g64.size) + (0.1 * rms) ** 2).astype(np.float32)
    return m0, v0


def judge(got, want64, want32, table):
    """-> (worst deviation / bound, its tensor, the tensors outside their bound as readable lines)."""
    devs = ko.deviations(got, want64, want32, table)
    name, frac, _ = max(devs, key=lambda d: d[1])
    return frac, name, ko.failures(got, want64, want32, table)


class Built:
    """A case with everything the CPU can say about it: the oracle, the inputs, the float64 / float32 references."""

    def __init__(self, c):
        self.c = c
        self.model = build_oracle(c)
        self.obs1, self.obs2, self.act = inputs(c, copy.deepcopy(self.model).double())
        self.beta = float(np.float32(c["beta"]))             # what the kernel receives
        self.table, self.size = tables(self.model)
        self.pad = padding(self.table, self.size)
        self.params = flat_params(self.model)
        self.r64 = self.ref(torch.float64)
        self.r32 = self.ref(torch.float32)

    def ref(self, dtype, **planted):
        return reference(self.model, self.obs1, self.obs2, self.act, self.beta, dtype, **planted)
