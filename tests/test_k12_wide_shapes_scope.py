"""
CPU tests of the second opt-in of the wide width pair (256, 512) of K6+K7 and K12: in_dim <= 512 per network, as far as each
row-tile body's LDS goes, and B <= 1024 (the bit PPOAF_SPLIT_WIDE_SHAPES = 4 of ppoaf_ppo_update_args_t.row_pairs, which
implies PPOAF_SPLIT_WIDE_INPUTS; PPOPolicy.fused_wide_shapes; csrc/ppo_update_dev.hpp: split_xld; the weight-gradient
launch's passes: csrc/ppo_update_split.hip).  Host checks only: nothing is launched.

  * with the bit and both networks at one depth the accepted in_dim are exactly 1 .. min(512, LDS_TABLE[256][depth - 1]); a
    refusal the LDS decides names LDS; beside an actor of depth min(depth, 3) and 40 inputs the critic takes 512 inputs at
    every depth 1 .. 7;
  * in_dim 513 and B 1025 are refused by name; without the bit the refusals of 129 inputs, B 513 and 65 inputs are the words
    the library says today (captured from the same calls), an ordinary pair keeps its own refusal, row_pairs = 8 is refused;
  * the split workspace is the ws_layout formula with a layer-0 panel stride of 64 / 128 / 256 / 512 floats, the wgrad
    launch's workgroups are the job formula;
  * FusedPolicyUpdate.unsupported_reason follows PPOPolicy.fused_wide_shapes, which no update_mode sets.
"""
import ctypes as C

import pytest

from test_k12_oracle import LDS_TABLE, _desc
from test_k12_wide_critic_scope import _ppo, _seg_len
from test_k12_wide_inputs_scope import _wide_layout_args
from test_k12_width_pairs_scope import _layout_args, _ws_bytes

ROW_PAIRS, WIDE_INPUTS, WIDE_SHAPES = 1, 2, 4


def _check(in_a, in_c, ha, hc, actor_depth, critic_depth, bits, B=64):
    """ppoaf_ppo_update_check for a pair with an in_dim and a depth per network (host only: no pointer of args is read)."""
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    a = _lib.PpoUpdateArgs()
    a.actor = _desc(in_a, ha, actor_depth, 2, 0)
    a.critic = _desc(in_c, hc, critic_depth, 1, a.actor.size)
    a.bucket_total = a.actor.size + a.critic.size
    a.head_kind, a.B, a.batch_stride = 0, B, B
    a.row_pairs = bits
    rc = lib.ppoaf_ppo_update_check(C.byref(a))
    return rc == 0, lib.ppoaf_last_error().decode() if rc else ""


def _shapes_layout_args(in_a, in_c, depth, B, bits, ha=256, hc=512):
    """test_k12_wide_inputs_scope._wide_layout_args with the option bits as given."""
    a = _wide_layout_args(in_a, in_c, depth, B, 0, ha, hc)
    a.row_pairs = bits
    return a


def _ws_refusal(a):
    from ppo_and_friends_amd import _lib
    lib, n = _lib.load(), C.c_int64(0)
    assert lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(n)) != 0
    return lib.ppoaf_last_error().decode()


def test_the_opt_in_is_the_third_bit_of_row_pairs_and_the_struct_keeps_its_layout():
    import os
    import re
    from ppo_and_friends_amd import _lib
    assert (_lib.SPLIT_ROW_PAIRS, _lib.SPLIT_WIDE_INPUTS, _lib.SPLIT_WIDE_SHAPES) == (ROW_PAIRS, WIDE_INPUTS, WIDE_SHAPES)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ppoaf_hip.h")) as fh:
        src = fh.read()
    assert re.search(r"#define\s+PPOAF_SPLIT_WIDE_SHAPES\s+4\b", src)
    assert [f[0] for f in _lib.PpoUpdateArgs._fields_][-1] == "action_slices"
    assert _lib.ABI_VERSION == 7 and _lib.load().ppoaf_abi_version() == 7


@pytest.mark.parametrize("depth", range(1, 8))
def test_accepted_inputs_are_the_lds_table_up_to_512(depth):
    """Both networks at one depth: the 256-wide actor's LDS decides below 512 (depth 3: 432, depth 4: 160, deeper: nothing)."""
    limit = min(512, LDS_TABLE[256][depth - 1])
    ok = [d for d in range(1, 520) if _check(d, d, 256, 512, depth, depth, WIDE_SHAPES)[0]]
    assert ok == list(range(1, limit + 1)), (depth, limit, ok[-1:] or None)
    ok_, why = _check(limit + 1, limit + 1, 256, 512, depth, depth, WIDE_SHAPES)
    assert not ok_
    if limit < 512:
        assert "LDS" in why, why
    else:
        assert "wide pair" in why and "in_dim <= 512" in why and "513" in why, why
    # the bit implies the other one, and beside it changes nothing
    if limit:
        assert _check(limit, limit, 256, 512, depth, depth, WIDE_SHAPES | WIDE_INPUTS)[0]


def test_depth_3_takes_432_inputs_and_refuses_433_for_lds():
    assert _check(432, 432, 256, 512, 3, 3, WIDE_SHAPES)[0]
    ok, why = _check(433, 433, 256, 512, 3, 3, WIDE_SHAPES)
    assert not ok and "LDS" in why, why


def test_the_critic_takes_512_inputs_at_every_depth():
    for depth in range(1, 8):
        ok, why = _check(40, 512, 256, 512, min(depth, 3), depth, WIDE_SHAPES)
        assert ok, (depth, why)


def test_513_inputs_and_1025_rows_are_refused_by_name():
    for in_a, in_c in ((513, 513), (40, 513), (513, 40)):
        ok, why = _check(in_a, in_c, 256, 512, 1, 1, WIDE_SHAPES)
        assert not ok and "wide pair" in why and "in_dim <= 512" in why and "513" in why and "LDS" not in why, why
    ok, why = _check(8, 512, 256, 512, 3, 3, WIDE_SHAPES, B=1025)
    assert not ok and "wide pair" in why and "B <= 1024" in why and "1025" in why, why
    assert _check(8, 512, 256, 512, 3, 3, WIDE_SHAPES, B=1024)[0]
    # the layout query says the same
    why = _ws_refusal(_shapes_layout_args(8, 512, 3, 1025, WIDE_SHAPES))
    assert "wide pair" in why and "B <= 1024" in why and "1025" in why, why
    why = _ws_refusal(_shapes_layout_args(513, 40, 2, 64, WIDE_SHAPES))
    assert "wide pair" in why and "in_dim <= 512" in why and "513" in why, why


def test_without_the_bit_every_refusal_is_todays():
    """The words are captured from the same library calls, whose literals tests/test_k12_wide_inputs_scope.py and
    tests/test_k12_wide_critic_scope.py pin; nothing here may mention the new limits."""
    said = {
        "129 inputs": _check(129, 129, 256, 512, 3, 3, WIDE_INPUTS),
        "B 513": _check(8, 128, 256, 512, 3, 3, WIDE_INPUTS, B=513),
        "65 inputs": _check(65, 65, 256, 512, 3, 3, 0),
        "B 513, no bit": _check(8, 8, 256, 512, 3, 3, 0, B=513),
    }
    for what, (ok, why) in said.items():
        assert not ok and "wide pair" in why and "1024" not in why and "WIDE_SHAPES" not in why, (what, why)
    assert "PPOAF_SPLIT_WIDE_INPUTS in_dim <= 128 and B <= 512 (got in_dim 129 / 129, B 64)" in said["129 inputs"][1]
    assert "PPOAF_SPLIT_WIDE_INPUTS in_dim <= 128 and B <= 512 (got in_dim 8 / 128, B 513)" in said["B 513"][1]
    assert "in_dim <= 64 and B <= 512 (got in_dim 65 / 65, B 64)" in said["65 inputs"][1]
    assert "WIDE_INPUTS" not in said["65 inputs"][1] and "WIDE_INPUTS" not in said["B 513, no bit"][1]
    # the layout query: the same words as the check's, with and without the older bit
    for (in_dim, B, bits), what in (((129, 64, WIDE_INPUTS), "129 inputs"), ((65, 64, 0), "65 inputs")):
        assert _ws_refusal(_shapes_layout_args(in_dim, in_dim, 3, B, bits)) == said[what][1]
    # all three are accepted with the bit
    assert _check(129, 129, 256, 512, 3, 3, WIDE_SHAPES)[0]
    assert _check(8, 128, 256, 512, 3, 3, WIDE_SHAPES, B=513)[0]
    assert _check(65, 65, 256, 512, 3, 3, WIDE_SHAPES)[0]


def test_an_ordinary_pair_keeps_its_split_limit_whatever_the_bit_says():
    """(256, 256) with a split workspace: the layout query's refusal of 65 inputs and of B 513, word for word with and
    without the bit."""
    for in_dim, B, got in ((65, 256, "65 / 65, 256"), (8, 513, "8 / 8, 513"), (300, 1024, "300 / 300, 1024")):
        said = [_ws_refusal(_shapes_layout_args(in_dim, in_dim, 3, B, bits, 256, 256)) for bits in (0, WIDE_INPUTS, WIDE_SHAPES)]
        assert f"the split-wgrad chain covers in_dim <= 64 and B <= 512 (got {got})" in said[0], said[0]
        assert said[0] == said[1] == said[2]
    # (wider inputs run that pair's slab chain, which the check accepts either way)
    assert _check(65, 65, 256, 256, 3, 3, 0)[0] and _check(65, 65, 256, 256, 3, 3, WIDE_SHAPES)[0]
    # the row pairs of an ordinary pair answer as before beside the new bit
    p = _layout_args(64, 256, 3, ROW_PAIRS | WIDE_SHAPES)
    assert _ws_bytes(p) == _ws_bytes(_layout_args(64, 256, 3, 1)) > _ws_bytes(_layout_args(64, 256, 3, 0))


def test_bit_8_is_refused():
    """make_update_dev's unknown-bits check, through the wgrad entry point: refused by the host check, ahead of any launch
    (the pointers are placeholders nothing reads)."""
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    a = _shapes_layout_args(8, 8, 3, 64, 8)
    a.split_workspace, a.split_workspace_bytes = 0x10000, 1 << 40
    assert lib.ppoaf_ppo_update_wgrad(C.byref(a), None) != 0
    why = lib.ppoaf_last_error().decode()
    assert "row_pairs=8" in why and "4 wide shapes" in why, why
    a.row_pairs = 8 | WIDE_SHAPES
    assert lib.ppoaf_ppo_update_wgrad(C.byref(a), None) != 0 and "row_pairs=12" in lib.ppoaf_last_error().decode()


@pytest.mark.parametrize("in_dim,xld", [(64, 64), (65, 128), (129, 256), (257, 512)])
@pytest.mark.parametrize("B", [17, 512, 513, 1024])
def test_split_workspace_is_the_panel_layout(in_dim, xld, B):
    """csrc/ppo_update_dev.hpp: ws_layout -- per network hbuf and dbuf ([depth][Bp][H]), the output partials
    ([ceil(B / 16)][seg]) and xbuf ([Bp][xld]), each rounded up to 256 bytes; xld per network, so a narrow actor keeps 64."""
    Bp = (B + 63) // 64 * 64
    take = lambda floats: (floats * 4 + 255) // 256 * 256
    for depth in (1, 2):
        for in_a, xa in ((in_dim, xld), (40, 64)):
            want = 0
            for H, out_dim, x in ((256, 5, xa), (512, 1, xld)):
                want += 2 * take(depth * Bp * H) + take((B + 15) // 16 * _seg_len(0, H, depth, out_dim)) + take(Bp * x)
            assert _ws_bytes(_shapes_layout_args(in_a, in_dim, depth, B, WIDE_SHAPES)) == want, (depth, in_a)
            if in_dim <= 128 and B <= 512:       # inside the older bit's limits the new one changes no byte
                assert _ws_bytes(_shapes_layout_args(in_a, in_dim, depth, B, WIDE_INPUTS)) == want


def test_weight_gradient_workgroups_are_the_job_formula():
    from ppo_and_friends_amd import _lib
    jobs = lambda h, d, i: (d - 1) * (h // 16) * ((h // 16 + 1) // 2) + (h // 16) * (((i + 15) // 16 + 1) // 2) + 1
    for in_dim in (129, 256, 512):
        for depth in (1, 2):
            for B in (256, 1024):
                a = _shapes_layout_args(in_dim, in_dim, depth, B, WIDE_SHAPES)
                blocks = _lib.load().ppoaf_ppo_update_split_blocks(C.byref(a))
                assert blocks == 8 * ((jobs(256, depth, in_dim) + jobs(512, depth, in_dim) + 7) // 8), (in_dim, depth, B)
    # 129 inputs: nine tiles, five layer-0 pieces per 16 output rows; 512: 32 tiles, 16 pieces
    assert jobs(256, 1, 129) - 1 == 16 * 5 and jobs(512, 1, 512) - 1 == 32 * 16


# ---------------------------------------------------------------------------------------------------- the host's answers
PAIR = "wide pair (actor 256, critic 512)"


def _todays_in_dim_reason(O, with_inputs):
    """FusedPolicyUpdate.unsupported_reason of the parent commit for a 256 / 512 policy of O > 64 inputs (the texts
    tests/test_k12_wide_inputs_scope.py pins piece by piece)."""
    if not with_inputs:
        hint = "; PPOPolicy.fused_wide_inputs = True takes in_dim <= 128" if O <= 128 else ""
        return f"{PAIR}: in_dim {O} / {O} > 64 (the split-wgrad chain's panels cover in_dim <= 64){hint}"
    return "" if O <= 128 else (f"{PAIR}: in_dim {O} / {O} > 128 (with fused_wide_inputs the split-wgrad chain's panels "
                                "cover in_dim <= 128)")


def test_update_mode_leaves_the_attribute_alone():
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    assert PPOPolicy.fused_wide_shapes is False
    for mode in ("fused", "auto", "torch"):
        pol = _ppo(mode).policies["p"]
        assert pol.fused_wide_shapes is False and "fused_wide_shapes" not in vars(pol), mode
        assert pol.fused_wide_inputs is False


def test_unsupported_reason_follows_the_attribute(monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedOptIns, FusedPolicyUpdate, panel_stride
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    reason = FusedPolicyUpdate.unsupported_reason
    pols = {O: _ppo("fused", O=O).policies["p"] for O in (128, 129, 256, 433, 513)}
    # both attributes off, then fused_wide_inputs alone: today's texts
    for O, pol in pols.items():
        assert reason(pol, 64) == _todays_in_dim_reason(O, False), O
        assert "fused_wide_shapes" not in reason(pol, 64)
    batch_today = lambda B: f"{PAIR}: batch size {B} > 512 (the split-wgrad chain covers batch sizes <= 512)"
    small = _ppo("fused", O=8).policies["p"]
    for B in (513, 1000, 1024, 1025):
        assert reason(small, B) == batch_today(B), B
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_inputs", True)
        assert FusedOptIns.of(small).wide_inputs and not FusedOptIns.of(small).wide_shapes
        for O, pol in pols.items():
            assert reason(pol, 64) == _todays_in_dim_reason(O, True), O
        for B in (513, 1000, 1024, 1025):
            assert reason(pols[128], B) == batch_today(B), B
    # the new attribute, alone: it implies the other
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_shapes", True)
        assert FusedOptIns.of(small).wide_shapes and FusedOptIns.of(small).wide_inputs and PPOPolicy.fused_wide_inputs is False
        for O in (128, 129, 256):
            assert reason(pols[O], 64) == "", (O, reason(pols[O], 64))
            assert reason(pols[O], 1024) == "", O
            assert pols[O].fused_step_unsupported_reason() == "", O
        why = reason(pols[433], 64)                           # depth 3: the 256-wide actor's LDS, in the library's words
        assert "LDS" in why and "160 KiB" in why, why
        why = reason(pols[513], 64)
        assert PAIR in why and "in_dim 513 / 513 > 512" in why and "in_dim <= 512" in why and "fused_wide_shapes" in why, why
        for B in (513, 1000, 1024):
            assert reason(small, B) == "", B
        why = reason(small, 1025)
        assert PAIR in why and "batch size 1025 > 1024" in why and "batch sizes <= 1024" in why and "fused_wide_shapes" in why, why
        # the attribute does not take the pair by itself: fused_wide_critic does (update_mode="fused")
        auto = _ppo("auto", O=256).policies["p"]
        assert "not one of the instantiated widths" in reason(auto, 64)
    assert reason(pols[129], 64) == _todays_in_dim_reason(129, False)
    assert [panel_stride(i) for i in (1, 64, 65, 128, 129, 256, 257, 512)] == [64, 64, 128, 128, 256, 256, 512, 512]


def test_the_attribute_is_part_of_the_inference_reasons_key():
    """PPOPolicy.inference_unsupported_reason keeps its answer per (parameters, opt-ins): flipping the attribute asks again."""
    import torch
    pol = _ppo("fused", O=256).policies["p"]
    pol.device = torch.device("cuda", 0)                   # (only compared: the question is host-side)
    assert pol.inference_unsupported_reason() == _todays_in_dim_reason(256, False)
    pol.fused_wide_shapes = True
    assert pol.fused_step_unsupported_reason() == ""
    assert pol.inference_unsupported_reason() == ""
