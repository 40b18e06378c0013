"""
No GPU: the float64 check of K14's wide-action form (tests/helpers/icm_wide_actions_cases.py, used by
tests/test_gpu_icm_wide_actions_float64.py) asks nothing the reference itself cannot give, and has teeth where a kernel
written for 8 or 16 action columns would go wrong at 9 .. 24:

  * the float32 oracle, judged by the harness's bound against float64, passes for every case;
  * every Discrete case draws every class, so the columns past 8 and past 16 carry one-hots and labels;
  * planted errors are rejected: the classes from 8 (and from 16) on left out of the inverse loss, out of the forward
    model's one-hot / action columns, out of the inverse output layer's weight gradient, and out of its backward pass.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import icm_float64 as H  # noqa: E402
import icm_wide_actions_cases as W  # noqa: E402

_BUILT = {}


def built(name):
    """The case with its references, computed once and left unchanged."""
    if name not in _BUILT:
        _BUILT[name] = H.Built(W.CASES[name])
    return _BUILT[name]


def test_the_cases_cover_what_they_claim():
    cs = W.CASES
    for chain in ("shapes", "identity"):
        got = {c["action"] for c in cs.values() if c["chain"] == chain and c["B"] == 33}
        assert {(k, A) for k in W.KINDS for A in W.WIDE_WIDTHS} <= got, chain
    assert all(8 < H.action_dims(c)[0] <= 24 for c in cs.values())
    assert {c["B"] for c in cs.values()} >= {17, 33, 257}
    assert {c["rows"] for c in cs.values()} == set(H.ROW_MODES) and {c["act"] for c in cs.values()} == set(H.ACTIVATIONS)
    assert {c["depths"] for c in cs.values()} >= {(1, 3), (3, 1)}
    assert {c["widths"][1] for c in cs.values() if c["chain"] == "shapes"} >= {9, 16, 17}
    inv_fwd = {c["widths"][-2:] for c in cs.values()}
    assert any(a < b for a, b in inv_fwd) and any(a > b for a, b in inv_fwd) and any(a == b for a, b in inv_fwd)
    assert {c["beta"] for c in cs.values()} >= {0.0, 1.0}
    m = cs["sh_mario"]
    assert (m["O"], m["widths"], m["depths"], m["action"], m["B"]) == (256, (128, 9, 32, 32), (2, 2), ("discrete", 18), 33)


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_float32_oracle_is_inside_the_bound(name):
    b = built(name)
    A, discrete, _ = H.action_dims(b.c)
    if discrete:
        assert len(np.unique(b.act)) == min(A, b.c["B"]), "every class occurs (B permitting)"
    for what, table in (("grads", b.table), ("loss", H.LOSS), ("reward", [("", "reward", 0, (b.c["B"],))])):
        assert np.isfinite(b.r64[what]).all()
        frac, where, bad = H.judge(b.r32[what], b.r64[what], b.r64[what], table)      # the plain 1e-5 + 1e-5 bound
        assert not bad, (what, where, frac, bad)
        assert not H.judge(b.r32[what], b.r64[what], b.r32[what], table)[2]           # and with the floor, as the GPU file judges
    assert not b.r64["grads"][b.pad].any()
    m0, v0 = H.preset_state(b.c, b.r64["grads"], b.pad)
    lr = float(np.float32(3e-4))
    want = H.adam(b.params, b.r64["grads"], m0, v0, 6, lr)
    want32 = H.adam(b.params, b.r32["grads"], m0, v0, 6, lr, dtype=torch.float32)
    for k, what in ((1, "m"), (2, "v")):
        assert not H.judge(want32[k], want[k], want[k], b.table)[2], what


# --------------------------------------------------------------------------------------------------- planted errors
def _linears(net):
    return [m for m in net.sequential_net.modules() if isinstance(m, nn.Linear)]


def _planted(b, what, cut):
    """The float64 reference of a kernel that handles action columns [0, cut) only in one place:
      loss      the inverse head sees `cut` outputs (Discrete: the softmax runs over them; Box: the MSE's sum does)
      one_hot   the forward model's layer 0 reads zeros in its action columns from `cut` on
      dgrad     d(out) columns from `cut` on do not reach the inverse model's hidden layers (its own wgrad has them)
      wgrad     the inverse output layer's weight and bias gradient rows from `cut` on stay zero"""
    m = copy.deepcopy(b.model)
    A, discrete, _ = H.action_dims(b.c)
    last = _linears(m.inv_model)[-1]
    first = _linears(m.forward_model)[0]
    keep = torch.arange(A) < cut
    if what == "loss":
        if discrete:
            last.register_forward_hook(lambda _m, _i, out: out.masked_fill(~keep, float("-inf")))
        else:
            def hook(_m, _i, out):
                out.register_hook(lambda g: g * keep.to(g.dtype))
            last.register_forward_hook(hook)
    elif what == "one_hot":
        D = first.in_features - A
        first.register_forward_pre_hook(lambda _m, args: (torch.cat((args[0][:, :D + cut], torch.zeros_like(args[0][:, D + cut:])), 1),))
    elif what == "dgrad":
        def hook(mod, args, out):
            # the same values, with the columns from `cut` on detached from the input: their gradient reaches W and b only
            return torch.where(keep, out, nn.functional.linear(args[0].detach(), mod.weight, mod.bias))
        last.register_forward_hook(hook)
    r = H.reference(m, b.obs1, b.obs2, b.act, b.beta, torch.float64)
    if what == "wgrad":
        r = H.reference(b.model, b.obs1, b.obs2, b.act, b.beta, torch.float64)
        names = [n for n, _ in b.model.named_parameters()]
        lw = [t for t in b.table if t[1].startswith("inv_model")][-2:]
        assert [t[1].rsplit(".", 1)[1] for t in lw] == ["weight", "bias"] and lw[0][3][0] == A and names
        (_, _, woff, (_, M)), (_, _, boff, _) = lw
        r["grads"][woff + cut * M:woff + A * M] = 0.0
        r["grads"][boff + cut:boff + A] = 0.0
    return r


def _rejected(b, r, what="grads"):
    table = b.table if what == "grads" else H.LOSS
    return bool(H.judge(r[what], b.r64[what], b.r32[what], table)[2])


PLANT_CASES = ["sh_disc9", "sh_cont9", "id_disc16", "id_cont16", "sh_disc17", "id_cont17", "sh_cont24", "id_disc24", "sh_mario",
               "sh_default128_box17", "id_B17"]


@pytest.mark.parametrize("what", ["loss", "one_hot", "dgrad", "wgrad"])
@pytest.mark.parametrize("name", PLANT_CASES)
def test_columns_left_out_are_rejected(name, what):
    """A kernel that runs one of its loops over 8 (or, above 16, over 16) action columns only does not pass."""
    b = built(name)
    A = H.action_dims(b.c)[0]
    for cut in [c for c in (8, 16) if c < A]:
        r = _planted(b, what, cut)
        assert np.isfinite(r["grads"]).all()
        assert _rejected(b, r), (name, what, cut)
        # (the gradients are what rejects: CrossEntropyLoss on probabilities stays close to log A whatever the logits, and
        # Box is planted in the gradient of the sum, so the loss value says little here)
        if what == "one_hot":                    # the rollout-time reward reads the same tile
            assert H.judge(r["reward"], b.r64["reward"], b.r32["reward"], [("", "reward", 0, (b.c["B"],))])[2], (name, cut)


def test_the_unplanted_reference_is_accepted():
    b = built("sh_mario")
    r = H.reference(copy.deepcopy(b.model), b.obs1, b.obs2, b.act, b.beta, torch.float64)
    assert not _rejected(b, r) and not _rejected(b, r, "loss")
