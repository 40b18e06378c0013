"""
-m gpu: the middle of K12's row-tile body hands work from wave to wave through LDS -- the head's row part leaves d loss /
d out and each row's loss terms there; dz_last, the output layer's gradients, the block's loss partials and the critic's
values are formed behind barriers by other waves.  A missing barrier there shows as a result that changes from launch to
launch, so:

  * repeatability: `gradient_only` on the same mini-batch from the same state, 20 times -- the gradient bucket, the eight
    totals and buffer.values are bitwise the same every time.  B = 17 (one full tile, one tile with a single live row and 15
    dead ones); three 128-wide hidden layers and two 64-wide ones; Discrete(2), Discrete(5) (classes q + 4), Box(8)
    (dlog_std, all 8 action words), MultiDiscrete of eight slices; the value normaliser on; forms chain, slabs, row_tiles
    of tests/test_gpu_k12_gradients.py (whose float64 comparison covers the values themselves).
  * write-back: after one full mini-batch, rows of buffer.values outside the mini-batch keep their bits and the
    mini-batch's rows hold the critic's forward on the pre-step parameters (float64 reference; that module's rule: 1e-5
    relative plus 1e-5 of the tensor's maximum).
"""
import numpy as np
import pytest
import torch

import test_gpu_k12_gradients as g12

pytestmark = pytest.mark.gpu

REPEATS = 20
FORMS = {k: g12.FORMS[k] for k in ("chain", "slabs", "row_tiles")}
HEADS = {"discrete2": ("categorical", 2), "discrete5": ("categorical", 5), "box8": ("gaussian", 8),
         "multidiscrete8": ("multi_categorical", (1,) * 8)}
NETS = {"128x3": dict(ha=128, depth=3), "64x2": dict(ha=64, depth=2)}


def _steered(head, net, seed):
    return g12.Steered(g12.case(O=8, B=17, head=HEADS[head], act="tanh", norm_values=True, seed=seed, **NETS[net]))


def _updater(s, form, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    env, pairs = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(FusedPolicyUpdate, "row_pairs", pairs)
    return FusedPolicyUpdate(s.ppo, "p")


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("head", sorted(HEADS))
def test_gradient_only_repeats_bitwise(head, net, monkeypatch):
    s = _steered(head, net, seed=300 + len(head) + len(net))
    pol, B = s.pol, s.c["B"]
    values0 = pol.buffer.values.clone()
    for form in FORMS:
        with monkeypatch.context() as mp:
            upd = _updater(s, form, mp)
            upd.begin_epoch(s.perm)
            args = upd._args_for(B)
            steps = pol.policy_step_counts.clone()
            first = None
            for i in range(REPEATS):
                upd.totals.zero_()
                pol.buffer.values.copy_(values0)
                upd.gradient_only(args)
                torch.cuda.synchronize()
                pol.policy_step_counts.copy_(steps)
                got = (pol.policy_grads.clone(), upd.totals[:8].clone(), pol.buffer.values.clone())
                if first is None:
                    first = got
                    assert torch.isfinite(got[0]).all() and got[0].abs().max() > 0
                    continue
                for name, a, b in zip(("gradient bucket", "totals", "buffer.values"), first, got):
                    # bit patterns, so that a NaN or a signed zero cannot hide a difference
                    same = torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                       b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))
                    assert same, f"{form}: {name} of launch {i} differs from launch 0 in {(a != b).sum().item()} places"
    pol.buffer.values.copy_(values0)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_values_write_back(form, monkeypatch):
    s = _steered("discrete5", "128x3", seed=411)
    pol, B = s.pol, s.c["B"]
    upd = _updater(s, form, monkeypatch)
    flat = s.flat(pol.buffer.values).view(-1)
    # a pattern no forward pass produces, so that a row the launch skips or writes twice shows
    flat.copy_(torch.linspace(-3.0, 3.0, flat.numel(), device=flat.device))
    before = flat.clone()
    upd.begin_epoch(s.perm)
    upd._one(upd._args_for(B))
    torch.cuda.synchronize()
    upd._check_persistent()
    after = flat.clone()
    inside = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    inside[s.rows] = True
    assert int(inside.sum()) == B
    assert torch.equal(after[~inside].view(torch.int32), before[~inside].view(torch.int32)), "a row outside the mini-batch changed"
    want = np.asarray(s.r64["values"], dtype=np.float64).reshape(-1)
    got = after[s.rows].double().cpu().numpy()
    bound = 1e-5 * np.abs(want) + 1e-5 * np.abs(want).max()
    err = np.abs(got - want)
    print(f"{form}: worst |v - v64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"{form}: rows {np.nonzero(err > bound)[0].tolist()} of the mini-batch"
