"""
CPU tests of the wide heads of the wide width pair (256, 512): a 256-wide actor with 9 .. 24 outputs under a Categorical or
tanh-Gaussian head on K6+K7, K12 and K19, behind PPOPolicy.fused_wide_heads (fused_update.WIDE_HEAD_MAX;
csrc/policy_wide_heads.hip, csrc/ppo_update_wide_heads.hip).  Host checks only: nothing is launched.

  * the host's answers: with the attribute off, Box(17) and Discrete(18) at 256 / 512 are refused in the words of the parent
    commit ("actor: output width 17 > 8"), under "fused" and under "auto"; with it on, humanoid's and mario_bros_ram's shapes
    and out_dim 9 and 24 are taken; out_dim 25, MultiDiscrete summing to 9, MultiBinary(9) and Box(9) at (256, 256) and
    (64, 256) are refused with a reason that names the limit; "auto" keeps the torch path; no update_mode sets the attribute;
  * the library, host-only calls: both baseline shapes are accepted by ppoaf_ppo_update_check, ppoaf_policy_step and
    ppoaf_policy_infer; one input over the LDS edge of depth 3 (432, as for the narrow heads) is refused with "LDS" and the
    byte count of the restated carve; the split workspace for out_dim 17 is the ws_layout formula; for out_dim 5 every size
    is what it is without the attribute (the library has no such switch: it accepts by shape).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import k12_oracle as ko

from test_k12_wide_critic_scope import _seg_len
from test_k12_width_pairs_scope import _layout_args, _ws_bytes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wide_heads_cases as wh  # noqa: E402

WIDE_SHAPES = 4
CAT, GAU, MCAT, BERN = 0, 1, 2, 3
TODAY = {17: "actor: output width 17 > 8", 18: "actor: output width 18 > 8"}       # (FusedPolicyUpdate.unsupported_reason of the parent)


# ---------------------------------------------------------------------------------------------------- the host's answers
def _ppo(mode, space, O=8, B=64, ha=256, hc=512, depth=3, act=None, verbose=False):
    from torch import nn
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    dev = torch.device("cpu")
    env_gen = lambda: SyntheticFixedLengthEnv(4, O, space, 8, dev, reward="uniform", seed=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    kw = dict(hidden_depth=depth, activation=(act or nn.ReLU)())
    pargs = dict(actor_kw_args=dict(kw, hidden_size=ha), critic_kw_args=dict(kw, hidden_size=hc))
    return PPO(env_gen, {"p": (None, sp, sp, space, pargs)}, device=dev, random_seed=1, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=4, ts_per_rollout=8, batch_size=B, epochs_per_iter=1,
               save_state=False, update_mode=mode, verbose=verbose)


def _spaces():
    from ppo_and_friends_amd.spaces import Box, Discrete, MultiBinary, MultiDiscrete
    box = lambda n: Box(-0.4, 0.4, (n,), np.float32)
    return box, Discrete, MultiDiscrete, MultiBinary


@pytest.fixture
def on(monkeypatch):
    """Both opt-ins, for the class (376 and 256 inputs need fused_wide_shapes)."""
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)


def _reason(pol, B):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    return FusedPolicyUpdate.unsupported_reason(pol, B)


def test_no_update_mode_sets_the_attribute():
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd import fused_update
    box, Discrete, _, _ = _spaces()
    assert PPOPolicy.fused_wide_heads is False and fused_update.WIDE_HEAD_MAX == 24
    for mode in ("fused", "auto", "torch"):
        pol = _ppo(mode, Discrete(18)).policies["p"]
        assert pol.fused_wide_heads is False and "fused_wide_heads" not in vars(pol), mode


def test_attribute_off_the_refusals_are_todays(monkeypatch):
    from torch import nn
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    box, Discrete, _, _ = _spaces()
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    for mode in ("fused", "auto"):
        hum = _ppo(mode, box(17), O=376, B=512, act=nn.Tanh).policies["p"]
        mario = _ppo(mode, Discrete(18), O=256, B=128, act=nn.LeakyReLU).policies["p"]
        assert _reason(hum, 512) == TODAY[17] and hum.fused_step_unsupported_reason() == TODAY[17], mode
        assert _reason(mario, 128) == TODAY[18] and mario.fused_step_unsupported_reason() == TODAY[18], mode
        # what `verbose` adds: the attribute would take both (under "auto" together with update_mode="fused")
        assert FusedPolicyUpdate.wide_heads_would_take(hum, 512) and FusedPolicyUpdate.wide_heads_would_take(mario, 128)
        assert "fused_wide_heads" not in vars(hum) and hum.fused_wide_critic is (mode == "fused")
    # a False set by hand on the policy under a class attribute of True survives the question
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)
    hum.fused_wide_heads = False
    assert FusedPolicyUpdate.wide_heads_would_take(hum, 512) and vars(hum)["fused_wide_heads"] is False
    assert _reason(hum, 512) == TODAY[17]
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", False)
    # ... and would not take what it does not cover
    assert not FusedPolicyUpdate.wide_heads_would_take(_ppo("fused", box(25)).policies["p"], 64)
    assert not FusedPolicyUpdate.wide_heads_would_take(_ppo("fused", box(9), hc=256).policies["p"], 64)


def test_attribute_on_the_baseline_shapes_are_taken(on):
    from torch import nn
    box, Discrete, _, _ = _spaces()
    hum = _ppo("fused", box(17), O=376, B=512, act=nn.Tanh).policies["p"]
    mario = _ppo("fused", Discrete(18), O=256, B=128, act=nn.LeakyReLU).policies["p"]
    for pol, B in ((hum, 512), (mario, 128)):
        assert _reason(pol, B) == "", _reason(pol, B)
        assert pol.fused_step_unsupported_reason() == ""
    for space in (box(9), box(24), Discrete(9), Discrete(24)):
        assert _reason(_ppo("fused", space).policies["p"], 64) == "", space
    # one input over the depth-3 LDS edge: the library's words
    why = _reason(_ppo("fused", box(17), O=433).policies["p"], 64)
    assert "LDS" in why and str(wh.rowtile_lds_bytes(433, 3, 17)) in why, why
    # "auto" keeps the torch path: the attribute does not take the pair by itself
    auto = _ppo("auto", box(17), O=376, B=512).policies["p"]
    assert _reason(auto, 512) == TODAY[17]


def test_attribute_on_refusals_name_the_limit(on):
    box, Discrete, MultiDiscrete, MultiBinary = _spaces()
    why = _reason(_ppo("fused", box(25)).policies["p"], 64)
    assert why == "actor: output width 25 > 24", why
    why = _reason(_ppo("fused", Discrete(25)).policies["p"], 64)
    assert why == "actor: output width 25 > 24", why
    why = _reason(_ppo("fused", MultiDiscrete([4, 5])).policies["p"], 64)
    assert "MultiDiscrete([4, 5])" in why and "8 classes in all" in why, why
    why = _reason(_ppo("fused", MultiBinary(9)).policies["p"], 64)
    assert "MultiBinary(9)" in why and "1 .. 8 bits" in why, why
    for ha, hc in ((256, 256), (64, 256)):
        why = _reason(_ppo("fused", box(9), ha=ha, hc=hc).policies["p"], 64)
        assert f"(actor {ha}, critic {hc})" in why and "output width 9 > 8" in why and "(256, 512) only" in why, why
    # out_dim <= 8: nothing asks about the attribute
    assert _reason(_ppo("fused", box(4)).policies["p"], 64) == "" and _reason(_ppo("fused", box(4), hc=256).policies["p"], 64) == ""


def test_the_attribute_is_part_of_the_inference_reasons_key(monkeypatch):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    _, Discrete, _, _ = _spaces()
    pol = _ppo("fused", Discrete(18)).policies["p"]
    pol.device = torch.device("cuda", 0)                   # (only compared: the question is host-side)
    assert pol.inference_unsupported_reason() == TODAY[18]
    pol.fused_wide_heads = True
    assert pol.inference_unsupported_reason() == ""


# ---------------------------------------------------------------------------------------------------- the library
def _desc(in_dim, hidden, depth, out_dim, offset, log_std=False):
    from ppo_and_friends_amd import _lib
    _, size = ko.tensor_table(ko.Net(in_dim, hidden, depth, out_dim, "relu"))
    ls = -1
    if log_std:
        ls, size = size, size + (out_dim + 3) // 4 * 4
    return _lib.MlpDesc(in_dim=in_dim, hidden=hidden, depth=depth, out_dim=out_dim, activation=0, offset=offset, size=size,
                        log_std_offset=ls)


def _update_args(in_dim, ha, hc, depth, out_dim, head, B=64, bits=WIDE_SHAPES):
    from ppo_and_friends_amd import _lib
    a = _lib.PpoUpdateArgs()
    a.actor = _desc(in_dim, ha, depth, out_dim, 0, head == GAU)
    a.critic = _desc(in_dim, hc, depth, 1, a.actor.size)
    a.bucket_total = a.actor.size + a.critic.size
    a.head_kind, a.B, a.batch_stride, a.row_pairs = head, B, B, bits
    if head == MCAT:
        a.n_action_slices, a.action_slices[0], a.action_slices[1] = 2, 4, out_dim - 4
    return a


def _ws_args(in_dim, depth, out_dim, head, B, bits):
    """The layout entry points' args (test_k12_width_pairs_scope._layout_args: placeholder pointers nothing reads) with this
    file's descriptors."""
    a, q = _layout_args(256, 512, depth, 0, B=B, stride=B, actor_depth=depth), _update_args(in_dim, 256, 512, depth, out_dim, head, B, bits)
    a.actor, a.critic, a.bucket_total, a.head_kind, a.row_pairs = q.actor, q.critic, q.bucket_total, head, bits
    return a


def _check(*args, **kw):
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    rc = lib.ppoaf_ppo_update_check(C.byref(_update_args(*args, **kw)))
    return rc == 0, lib.ppoaf_last_error().decode() if rc else ""


def _step(in_dim, ha, hc, depth, out_dim, head, E=0):
    """ppoaf_policy_step on the host: E = 0 launches nothing; E > 0 with placeholder pointers is for calls the checks refuse."""
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    a = _lib.PolicyStepArgs()
    a.actor = _desc(in_dim, ha, depth, out_dim, 0, head == GAU)
    a.critic = _desc(in_dim, hc, depth, 1, a.actor.size)
    a.head_kind, a.E = head, E
    rc = lib.ppoaf_policy_step(C.byref(a), None)
    return rc == 0, lib.ppoaf_last_error().decode() if rc else ""


def _infer(in_dim, ha, depth, out_dim, head):
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    a = _lib.PolicyInferArgs()
    a.actor = _desc(in_dim, ha, depth, out_dim, 0, head == GAU)
    a.head_kind, a.E, a.mode = head, 0, 1
    a.params = a.obs = a.action_out = 0x10000              # (never read: E = 0 launches nothing)
    rc = lib.ppoaf_policy_infer(C.byref(a), None)
    return rc == 0, lib.ppoaf_last_error().decode() if rc else ""


def test_library_accepts_the_baseline_shapes():
    for in_dim, out_dim, head, B in ((376, 17, GAU, 512), (256, 18, CAT, 128), (128, 18, CAT, 128), (8, 9, GAU, 64), (8, 24, CAT, 64)):
        assert _check(in_dim, 256, 512, 3, out_dim, head, B=B) == (True, ""), (in_dim, out_dim)
        assert _step(in_dim, 256, 512, 3, out_dim, head) == (True, ""), (in_dim, out_dim)
        assert _infer(in_dim, 256, 3, out_dim, head) == (True, ""), (in_dim, out_dim)


def test_library_refuses_one_step_over_the_lds_edge_with_the_byte_count():
    """The wide-head tile adds no byte to the actor's carve: the edges are the narrow heads' (depth 3: 432 inputs, depth 4: 160)."""
    for depth, edge in ((3, 432), (4, 160)):
        for out_dim, head in ((17, GAU), (18, CAT), (24, GAU)):
            assert _check(edge, 256, 512, depth, out_dim, head)[0], (depth, out_dim)
            ok, why = _check(edge + 1, 256, 512, depth, out_dim, head)
            need = wh.rowtile_lds_bytes(edge + 1, depth, out_dim)
            assert not ok and "LDS" in why and f"needs {need} B" in why and need > wh.LDS_LIMIT, why
            assert need == wh.rowtile_lds_bytes(edge + 1, depth, 5)
    assert wh.rowtile_lds_bytes(376, 3, 17) == 160064 and wh.rowtile_lds_bytes(8, 1, 9) > wh.rowtile_lds_bytes(8, 1, 8)


def test_library_refusals_say_what_would_be_taken():
    ok, why = _check(8, 256, 512, 1, 25, CAT)
    assert not ok and "out_dim=25" in why and "[1,24]" in why, why
    for head in (MCAT, BERN):
        ok, why = _check(8, 256, 512, 1, 9, head)
        assert not ok and "out_dim=9" in why and f"head_kind={head}" in why and "[1,8]" in why and "Categorical" in why, why
    ok, why = _check(8, 256, 256, 1, 9, GAU)
    assert not ok and "out_dim=9" in why and "(actor 256, critic 256)" in why and "(actor 256, critic 512)" in why, why
    assert _step(8, 256, 256, 1, 9, GAU)[1].startswith("policy_step: actor out_dim=9 at hidden widths (actor 256, critic 256)")
    # every other network keeps today's words
    for ha, hc in ((64, 64), (64, 256), (128, 128)):
        assert _check(8, ha, hc, 1, 9, CAT) == (False, "actor: out_dim=9 out of [1,8]")
        assert _step(8, ha, hc, 1, 9, CAT) == (False, "actor: out_dim=9 out of [1,8]")
    assert _infer(8, 64, 1, 9, CAT) == (False, "actor: out_dim=9 out of [1,8]")
    assert _infer(8, 256, 1, 9, BERN)[1].startswith("policy_infer: actor out_dim=9 with head_kind=3")


def test_split_workspace_for_17_outputs_is_the_panel_layout():
    Bp, take = 512, lambda floats: (floats * 4 + 255) // 256 * 256
    B, depth, in_dim, xld = 512, 3, 376, 512
    want = 0
    for H, out_dim, log_std in ((256, 17, 20), (512, 1, 0)):
        want += 2 * take(depth * Bp * H) + take((B + 15) // 16 * (_seg_len(0, H, depth, out_dim) + log_std)) + take(Bp * xld)
    assert _ws_bytes(_ws_args(in_dim, depth, 17, GAU, B, WIDE_SHAPES)) == want


def test_out_dim_5_sizes_do_not_know_the_feature():
    """The library accepts by shape: for out_dim 5 nothing it answers depends on an opt-in of the host."""
    from ppo_and_friends_amd import _lib
    a = _ws_args(40, 3, 5, CAT, 96, 0)
    take = lambda floats: (floats * 4 + 255) // 256 * 256
    want = sum(2 * take(3 * 128 * H) + take(6 * _seg_len(0, H, 3, o)) + take(128 * 64) for H, o in ((256, 5), (512, 1)))
    assert _ws_bytes(a) == want
    assert _lib.load().ppoaf_ppo_update_split_blocks(C.byref(a)) > 0
    assert wh.step_lds_floats(40, 256, 3, 5) == wh.cases.lds_floats(40, 256, 3)
    assert wh.rowtile_lds_bytes(40, 3, 5) == (208 + 4 * 256 + 8 * 256 + 16 * 52 + 5 * 16 * 260 + 512) * 4 + 36864
