"""
CPU tests of the opt-in that takes the wide width pair (256, 512) of K6+K7 and K12 to 65 .. 128 inputs per network
(the bit PPOAF_SPLIT_WIDE_INPUTS of ppoaf_ppo_update_args_t.row_pairs, called wide_inputs below; PPOPolicy.fused_wide_inputs;
csrc/ppo_update_dev.hpp: split_xld, WsDev::xld).  The opt-in is an option bit of an existing field, not a field appended
behind the slice table: tests/test_action_heads_scope.py pins the end of the ctypes struct.

  * with wide_inputs = 1 ppoaf_ppo_update_check accepts the pair at in_dim 65, 80 and 128 for every critic depth 1 .. 7 beside
    an actor of depth min(depth, 3); with both networks at one depth the actor's LDS decides, by the table of
    tests/test_k12_oracle.py (LDS_TABLE[256]: depth 4 holds in_dim 160, depth 5 .. 7 nothing), and a refusal names LDS;
  * it refuses in_dim 129 by name; an ordinary pair with a split workspace keeps its in_dim <= 64 refusal whatever the flag
    says, and with wide_inputs = 0 the wide pair keeps today's words;
  * the split workspace is the ws_layout formula with a layer-0 panel of Bp x 128 floats for a network above 64 inputs and
    Bp x 64 for one at or below, per network; the wgrad launch's workgroups are the job formula;
  * FusedPolicyUpdate.unsupported_reason follows PPOPolicy.fused_wide_inputs, which no update_mode sets.
"""
import ctypes as C

import pytest

from test_k12_oracle import LDS_TABLE, _desc
from test_k12_wide_critic_scope import _ppo, _seg_len
from test_k12_width_pairs_scope import _layout_args, _ws_bytes

TODAY_C = "in_dim <= 64 and B <= 512"
TODAY_PY = "> 64 (the split-wgrad chain's panels cover in_dim <= 64)"


def _check(in_a, in_c, ha, hc, actor_depth, critic_depth, wide_inputs, B=64):
    """ppoaf_ppo_update_check for a pair with an in_dim and a depth per network (host only: no pointer of args is read)."""
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    a = _lib.PpoUpdateArgs()
    a.actor = _desc(in_a, ha, actor_depth, 2, 0)
    a.critic = _desc(in_c, hc, critic_depth, 1, a.actor.size)
    a.bucket_total = a.actor.size + a.critic.size
    a.head_kind, a.B, a.batch_stride = 0, B, B
    a.row_pairs = _lib.SPLIT_WIDE_INPUTS * wide_inputs
    rc = lib.ppoaf_ppo_update_check(C.byref(a))
    return rc == 0, lib.ppoaf_last_error().decode() if rc else ""


def _wide_layout_args(in_a, in_c, depth, B, wide_inputs, ha=256, hc=512):
    """test_k12_width_pairs_scope._layout_args with the networks' in_dims replaced (sizes and the critic's offset follow)."""
    a = _layout_args(ha, hc, depth, 0, B=B, stride=B, actor_depth=depth)
    pad4 = lambda x: (x + 3) // 4 * 4
    for d, in_dim in ((a.actor, in_a), (a.critic, in_c)):
        d.size += pad4(in_dim * d.hidden) - pad4(d.in_dim * d.hidden)
        d.in_dim = in_dim
    a.critic.offset = a.actor.size
    a.bucket_total = a.actor.size + a.critic.size
    a.row_pairs |= _lib_bits()[1] * wide_inputs
    return a


def _lib_bits():
    from ppo_and_friends_amd import _lib
    return _lib.SPLIT_ROW_PAIRS, _lib.SPLIT_WIDE_INPUTS


def test_the_opt_in_is_a_bit_of_row_pairs_and_the_struct_keeps_its_layout():
    import os
    import re
    from ppo_and_friends_amd import _lib
    assert _lib_bits() == (1, 2)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ppoaf_hip.h")) as fh:
        src = fh.read()
    for name, bit in (("PPOAF_SPLIT_ROW_PAIRS", 1), ("PPOAF_SPLIT_WIDE_INPUTS", 2)):
        assert re.search(rf"#define\s+{name}\s+{bit}\b", src), name
    assert [f[0] for f in _lib.PpoUpdateArgs._fields_][-1] == "action_slices"
    assert _lib.ABI_VERSION == 7 and _lib.load().ppoaf_abi_version() == 7
    # both options at once: the wide pair runs no row pairs, and the record region is not counted
    a = _wide_layout_args(128, 128, 3, 256, 1)
    a.row_pairs |= _lib.SPLIT_ROW_PAIRS
    n = C.c_int64(7)
    assert _lib.load().ppoaf_ppo_update_row_pairs_error_offset(C.byref(a), C.byref(n)) == 0 and n.value == -1
    # the row pairs of an ordinary pair answer as before beside the other bit
    p = _layout_args(64, 256, 3, _lib.SPLIT_ROW_PAIRS | _lib.SPLIT_WIDE_INPUTS)
    assert _ws_bytes(p) == _ws_bytes(_layout_args(64, 256, 3, 1)) > _ws_bytes(_layout_args(64, 256, 3, 0))


@pytest.mark.parametrize("in_dim", [65, 80, 128])
def test_the_wide_pair_is_accepted_up_to_128_inputs(in_dim):
    for depth in range(1, 8):
        ok, why = _check(in_dim, in_dim, 256, 512, min(depth, 3), depth, 1)
        assert ok, (depth, in_dim, why)
        # both networks at this depth: the actor's LDS decides, as for (256, 256)
        ok, why = _check(in_dim, in_dim, 256, 512, depth, depth, 1)
        assert ok == (in_dim <= LDS_TABLE[256][depth - 1]), (depth, in_dim, why)
        if not ok:
            assert "LDS" in why, why


def test_both_networks_at_depth_4_answer_as_the_lds_table_says():
    """What the check says at depth 4 / 4 (the deepest actor the row-tile body holds) and one deeper: the answer of
    LDS_TABLE[256], nothing computed here; a refusal is the LDS one."""
    for in_dim in (64, 65, 80, 128):
        for depth in (4, 5):
            ok, why = _check(in_dim, in_dim, 256, 512, depth, depth, 1)
            print(f"in_dim {in_dim} depth {depth}/{depth}: {'accepted' if ok else why}")
            assert ok == (in_dim <= LDS_TABLE[256][depth - 1]), (in_dim, depth, why)
            assert ok or "LDS" in why, why


def test_129_inputs_are_refused_by_name():
    for in_a, in_c in ((129, 129), (40, 129), (129, 40)):
        ok, why = _check(in_a, in_c, 256, 512, 3, 3, 1)
        assert not ok and "wide pair" in why and "in_dim <= 128" in why and "129" in why, why
    ok, why = _check(8, 128, 256, 512, 3, 3, 1, B=513)
    assert not ok and "wide pair" in why and "B <= 512" in why and "513" in why, why
    assert _check(128, 128, 256, 512, 3, 3, 1, B=512)[0]


def test_without_the_flag_65_inputs_keep_todays_refusal():
    ok, why = _check(65, 65, 256, 512, 3, 3, 0)
    assert not ok and "wide pair" in why and TODAY_C in why and "65" in why and "128" not in why, why
    assert _check(64, 64, 256, 512, 3, 3, 0)[0] and _check(64, 64, 256, 512, 3, 3, 1)[0]


def test_an_ordinary_pair_keeps_its_split_limit_whatever_the_flag_says():
    """(256, 256) with a split workspace at in_dim 65: the layout query's refusal, word for word with and without the flag
    (wider inputs run that pair's slab chain, which the check accepts either way)."""
    from ppo_and_friends_amd import _lib
    lib, said = _lib.load(), []
    for flag in (0, 1):
        a, n = _wide_layout_args(65, 65, 3, 256, flag, 256, 256), C.c_int64(0)
        assert lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(n)) != 0
        said.append(lib.ppoaf_last_error().decode())
        assert "the split-wgrad chain covers in_dim <= 64 and B <= 512 (got 65 / 65, 256)" in said[-1], said[-1]
        assert _check(65, 65, 256, 256, 3, 3, flag)[0]
    assert said[0] == said[1]
    # ... and the wide pair's own layout query without the flag
    a, n = _wide_layout_args(65, 65, 3, 256, 0), C.c_int64(0)
    assert lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(n)) != 0
    assert "wide pair" in lib.ppoaf_last_error().decode() and TODAY_C in lib.ppoaf_last_error().decode()


@pytest.mark.parametrize("in_a,in_c", [(65, 65), (128, 128), (40, 80), (80, 40), (64, 128), (18, 54)])
@pytest.mark.parametrize("depth,B", [(3, 256), (1, 17), (7, 512)])
def test_split_workspace_is_the_panel_layout(in_a, in_c, depth, B):
    """csrc/ppo_update_dev.hpp: ws_layout -- per network hbuf and dbuf ([depth][Bp][H]), the output partials and xbuf, whose row
    stride is 128 floats for a network with more than 64 inputs and 64 otherwise."""
    Bp = (B + 63) // 64 * 64
    take = lambda floats: (floats * 4 + 255) // 256 * 256
    want = 0
    for H, out_dim, in_dim in ((256, 5, in_a), (512, 1, in_c)):
        want += 2 * take(depth * Bp * H) + take((B + 15) // 16 * _seg_len(0, H, depth, out_dim))
        want += take(Bp * (128 if in_dim > 64 else 64))
    assert _ws_bytes(_wide_layout_args(in_a, in_c, depth, B, 1)) == want
    if max(in_a, in_c) <= 64:           # the flag changes nothing where it is not needed
        assert _ws_bytes(_wide_layout_args(in_a, in_c, depth, B, 0)) == want


def test_weight_gradient_workgroups_are_the_job_formula():
    from ppo_and_friends_amd import _lib
    jobs = lambda h, d, i: (d - 1) * (h // 16) * ((h // 16 + 1) // 2) + (h // 16) * (((i + 15) // 16 + 1) // 2) + 1
    for in_dim in (65, 128):
        for depth in (1, 3):
            a = _wide_layout_args(in_dim, in_dim, depth, 256, 1)
            blocks = _lib.load().ppoaf_ppo_update_split_blocks(C.byref(a))
            assert blocks == 8 * ((jobs(256, depth, in_dim) + jobs(512, depth, in_dim) + 7) // 8), (in_dim, depth)
    # 65 inputs: five tiles, three layer-0 pieces per 16 output rows; 128: eight tiles, four pieces
    assert jobs(256, 1, 65) - 1 == 16 * 3 and jobs(512, 1, 128) - 1 == 32 * 4


# ---------------------------------------------------------------------------------------------------- the host's answers
def test_update_mode_leaves_the_attribute_alone():
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    assert PPOPolicy.fused_wide_inputs is False
    for mode in ("fused", "auto", "torch"):
        pol = _ppo(mode).policies["p"]
        assert pol.fused_wide_inputs is False and "fused_wide_inputs" not in vars(pol), mode


def test_unsupported_reason_follows_the_attribute(monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    pols = {O: _ppo("fused", O=O).policies["p"] for O in (64, 65, 128, 129)}
    for O in (65, 128):
        why = FusedPolicyUpdate.unsupported_reason(pols[O], 64)
        assert "wide pair" in why and f"in_dim {O} / {O} > 64" in why and TODAY_PY in why, why
        assert "fused_wide_inputs" in why, why
        assert pols[O].fused_step_unsupported_reason() == why
    why = FusedPolicyUpdate.unsupported_reason(pols[129], 64)
    assert f"in_dim 129 / 129 > 64" in why and TODAY_PY in why and "fused_wide_inputs" not in why, why
    monkeypatch.setattr(PPOPolicy, "fused_wide_inputs", True)
    for O in (64, 65, 128):
        assert FusedPolicyUpdate.unsupported_reason(pols[O], 64) == "", O
        assert FusedPolicyUpdate.unsupported_reason(pols[O], 512) == "", O
        assert pols[O].fused_step_unsupported_reason() == ""
    why = FusedPolicyUpdate.unsupported_reason(pols[129], 64)
    assert "wide pair" in why and "in_dim 129 / 129 > 128" in why and "in_dim <= 128" in why, why
    why = FusedPolicyUpdate.unsupported_reason(pols[128], 513)
    assert "wide pair" in why and "batch size 513 > 512" in why, why
    # the attribute does not take the pair by itself: fused_wide_critic does (update_mode="fused")
    auto = _ppo("auto", O=128).policies["p"]
    assert "512" in FusedPolicyUpdate.unsupported_reason(auto, 64) and "not one of the instantiated widths" in \
        FusedPolicyUpdate.unsupported_reason(auto, 64)
    monkeypatch.setattr(PPOPolicy, "fused_wide_inputs", False)
    assert TODAY_PY in FusedPolicyUpdate.unsupported_reason(pols[65], 64)


def test_the_flag_is_part_of_the_inference_reasons_key():
    """PPOPolicy.inference_unsupported_reason keeps its answer per (parameters, opt-ins): flipping the flag asks again."""
    import torch
    pol = _ppo("fused", O=80).policies["p"]
    pol.device = torch.device("cuda", 0)                   # (only compared: the question is host-side)
    assert "fused_wide_inputs" in pol.inference_unsupported_reason()
    pol.fused_wide_inputs = True
    assert pol.inference_unsupported_reason() == ""
