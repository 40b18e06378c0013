"""
-m gpu: ONE mini-batch through K12's lean fwd_bwd kernel (csrc/ppo_update_lean.hip: the row-tile body compiled for one
activation and one head, chosen once per launch on the host) at the edges of its shapes: H = 32 / 64 / 128 and the 64/128
pair, B = 17 (a ragged last tile with one live row) / 48 / 256, in_dim 4 / 17, ReLU / LeakyReLU / tanh and a categorical(2) /
gaussian(2) head, rotated so that each activation and each head meets each H and all six (activation, head) kernels run.

Lean cases, on the gradient bucket, the eight totals and the values written back to the rollout buffer:
  (i)   ppoaf_ppo_update_fwd_bwd_form says 1 for the launch's arguments (and 0 once they carry a row_map);
  (ii)  bitwise equal to the general kernel in the same library on the same rows (reached with an identity `row_map` in the
        launch's arguments: a condition of the host's choice);
  (iii) against the float64 reference (oracle/k12_oracle.py) with the bound rule of tests/test_gpu_k12_gradients.py:
        |x - x64| <= 1e-5 |x64| + 1e-5 max|x64| per tensor, raised to 4 max|x32 - x64| where float32 cannot do better;
  (iv)  five repeated launches give the same bits;
  (v)   values outside the mini-batch's rows are unchanged.
General cases -- a MultiDiscrete head, an actor / critic pair with different activations, depth 2: the export says 0 and the
launch computes what it did before the lean kernel existed (both flavours of the general body agree bitwise, identity
`row_map` again).
The steering of the inputs (both clip branches, Huber's linear branch, no ReLU kinks) is test_gpu_k12_gradients.Steered.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_k12_gradients as g12
from oracle import k12_oracle as ko

pytestmark = pytest.mark.gpu

# (actor H, critic H) x B, with in_dim, activation and head per case
LEAN = {f"h{ha}x{hc}_b{B}": g12.case(O=O, ha=ha, hc=hc, depth=3, B=B, head=(kind, 2), act=act, seed=ha + hc + B)
        for ha, hc, B, O, act, kind in (
            (32, 32, 17, 4, "relu", "categorical"), (32, 32, 48, 17, "leaky_relu", "gaussian"), (32, 32, 256, 4, "tanh", "gaussian"),
            (64, 64, 17, 17, "leaky_relu", "categorical"), (64, 64, 48, 4, "tanh", "categorical"), (64, 64, 256, 17, "relu", "gaussian"),
            (128, 128, 17, 4, "tanh", "gaussian"), (128, 128, 48, 17, "relu", "categorical"), (128, 128, 256, 4, "leaky_relu", "categorical"),
            (64, 128, 17, 17, "relu", "gaussian"), (64, 128, 48, 4, "leaky_relu", "gaussian"), (64, 128, 256, 17, "tanh", "categorical"))}

GENERAL = {
    "multi_discrete": (g12.case(O=4, ha=64, depth=3, B=48, head=("multi_categorical", (3, 2)), act="relu", seed=301), None),
    # (the critic's activation code is changed in the launch's arguments: a policy builds both networks with one)
    "mixed_activations": (g12.case(O=17, ha=128, depth=3, B=48, head=("categorical", 2), act="relu", seed=302), "tanh"),
    "depth_2": (g12.case(O=4, ha=64, hc=128, depth=2, B=48, head=("gaussian", 2), act="tanh", seed=303), None),
}
ACT_CODES = {"relu": 0, "leaky_relu": 1, "tanh": 2}
NAMES = ("gradient bucket", "totals", "values")


def test_cases_cover_the_edges():
    cs = list(LEAN.values())
    assert {(c["ha"], c["hc"]) for c in cs} == {(32, 32), (64, 64), (128, 128), (64, 128)}
    assert {(c["act"], c["head"][0]) for c in cs} == {(a, h) for a in g12.ACTS for h in ("categorical", "gaussian")}
    for pair in {(c["ha"], c["hc"]) for c in cs}:
        mine = [c for c in cs if (c["ha"], c["hc"]) == pair]
        assert {c["B"] for c in mine} == {17, 48, 256} and {c["O"] for c in mine} == {4, 17}
        assert {c["act"] for c in mine} == set(g12.ACTS) and {c["head"][0] for c in mine} == {"categorical", "gaussian"}


def _form(args):
    from ppo_and_friends_amd import _lib
    lib, f = _lib.load(), C.c_int32(-1)
    assert lib.ppoaf_ppo_update_fwd_bwd_form(C.byref(args), C.byref(f)) == 0, lib.ppoaf_last_error()
    return f.value


def _launch(s, upd, B, identity_map, want_form, critic_act=None):
    """One gradient_only launch of the first mini-batch from a fresh epoch -> (gradient bucket, totals, values)."""
    pol = s.pol
    upd.begin_epoch(s.perm)
    args = upd._args_for(B)
    assert args.inputs_in_batch_order == 1 and not args.row_map and args.split_workspace
    steps = pol.policy_step_counts.clone()
    pol.buffer.values.copy_(s.values0)
    act0 = args.critic.activation
    args.row_map = identity_map.data_ptr() if identity_map is not None else None
    if critic_act is not None:
        args.critic.activation = ACT_CODES[critic_act]
    try:
        assert _form(args) == want_form
        upd.gradient_only(args)
        torch.cuda.synchronize()
    finally:
        args.row_map = None
        args.critic.activation = act0
    pol.policy_step_counts.copy_(steps)
    return (pol.policy_grads.detach().clone(), upd.totals[:8].detach().clone(), pol.buffer.values.detach().clone())


def _setup(c):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    s = g12.Steered(c)
    s.values0 = s.pol.buffer.values.detach().clone()
    upd = FusedPolicyUpdate(s.ppo, "p")
    assert (upd.actor_desc.depth, upd.critic_desc.depth) == (c["depth"], c["depth"])
    assert (upd.actor_desc.hidden, upd.critic_desc.hidden) == (c["ha"], c["hc"])
    identity = torch.arange(s.pol.buffer.num_transitions, dtype=torch.int32, device=s.pol.device)
    return s, upd, identity


@pytest.mark.parametrize("name", sorted(LEAN))
def test_lean_kernel(name):
    run_lean(name, LEAN[name])


def run_lean(name, c):
    """Checks (i) .. (v) of the module docstring on one lean case -> the worst deviation / bound against float64."""
    s, upd, identity = _setup(c)
    B = c["B"]
    lean = [_launch(s, upd, B, None, 1) for _ in range(5)]              # (i) inside: the export says "lean"
    general = _launch(s, upd, B, identity, 0)
    # (iv) the same bits from five launches
    for rep in lean[1:]:
        for n, a, b in zip(NAMES, lean[0], rep):
            assert torch.equal(a, b), f"{name}: {n} differs between repeated launches"
    # (ii) the general kernel on the same rows
    for n, a, b in zip(NAMES, lean[0], general):
        assert torch.equal(a, b), f"{name}: {n}: the lean kernel differs from the general kernel " \
                                  f"(max |difference| {(a.double() - b.double()).abs().max().item():.3g})"
    # (iii) float64
    grads, totals, values = (t.double().cpu().numpy() for t in lean[0])
    rows = s.rows.cpu().numpy()
    vals = values.reshape(-1)[rows]
    one = lambda what, n: [("", what, 0, (n,))]
    worst_of_all = (0.0, "")
    for what, got, key, tab in (("gradient", grads, "grads", s.tables), ("totals", totals, "totals", g12.TOTALS),
                                ("values", vals, "values", one("values", B))):
        w64, w32 = np.asarray(s.r64[key]).reshape(-1), np.asarray(s.r32[key]).reshape(-1)
        worst = max(ko.deviations(got, w64, w32, tab), key=lambda d: d[1])
        print(f"{name}: {what}: worst {worst[1]:.3f} x bound at {worst[0]}")
        worst_of_all = max(worst_of_all, (worst[1], f"{what}: {worst[0]}"))
        bad = ko.failures(got, w64, w32, tab)
        assert not bad, f"{name} / {what}: " + "; ".join(bad[:6])
    # (v) the other rows' values
    other = np.ones(values.size, dtype=bool)
    other[rows] = False
    assert np.array_equal(values.reshape(-1)[other], s.values0.double().cpu().numpy().reshape(-1)[other]), \
        f"{name}: values outside the mini-batch's rows changed"
    return worst_of_all


@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_kernel_keeps_the_other_cases(name):
    c, critic_act = GENERAL[name]
    s, upd, identity = _setup(c)
    tables = _launch(s, upd, c["B"], None, 0, critic_act)
    plain = _launch(s, upd, c["B"], identity, 0, critic_act)
    for n, a, b in zip(NAMES, tables, plain):
        assert torch.equal(a, b), f"{name}: {n} differs between the general body's two flavours"
    assert torch.isfinite(tables[0]).all() and tables[0].abs().max() > 0
