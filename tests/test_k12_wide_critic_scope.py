"""
CPU tests of the wide width pair (256, 512) of K6+K7 and K12 (csrc/ppo_update_dev.hpp: PPOAF_WIDTH_PAIRS_WIDE; the critic's
row-tile body: csrc/ppo_update_rowtile_wide.hpp), which runs the three-launch form of the split-wgrad chain only:

  * ppoaf_ppo_update_check accepts the pair for in_dim 1, 17 and 64 at every critic depth 1 .. 7.  The actor's tiles run the
    row-tile body the 256-wide pairs run, whose LDS holds depth + 2 planes and ends at depth 4 (test_k12_oracle.LDS_TABLE):
    with BOTH networks at depth 5 .. 7 the pair is refused for the actor's LDS, as (256, 256) is -- asserted here too;
  * it refuses in_dim 65 and B 513 by name, and (512, 512), (128, 512), (512, 256) with "not instantiated"; every pair of
    {32, 64, 128, 256}^2 answers as before;
  * the split workspace is the ws_layout formula, no row pairs run, the wgrad launch's workgroups are the job formula;
  * FusedPolicyUpdate.unsupported_reason takes the pair only for a policy with `fused_wide_critic`, which
    PPO(update_mode="fused") sets and PPO(update_mode="auto") does not, and names what it refuses.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_k12_oracle import LDS_TABLE, _desc, _query
from test_k12_width_pairs_scope import PAIRS, WIDTHS, _err_off, _layout_args, _ws_bytes

TODAY = "critic: hidden width 512 is not one of the instantiated widths (32, 64, 128, 256)"


def _query2(in_dim, ha, hc, actor_depth, critic_depth, B=64):
    """test_k12_oracle._query with a depth per network."""
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    a = _lib.PpoUpdateArgs()
    a.actor = _desc(in_dim, ha, actor_depth, 2, 0)
    a.critic = _desc(in_dim, hc, critic_depth, 1, a.actor.size)
    a.bucket_total = a.actor.size + a.critic.size
    a.head_kind, a.B, a.batch_stride = 0, B, B
    rc = lib.ppoaf_ppo_update_check(C.byref(a))
    return rc == 0, lib.ppoaf_last_error().decode() if rc else ""


def test_the_wide_pair_is_accepted_at_every_critic_depth():
    for depth in range(1, 8):
        for in_dim in (1, 17, 64):
            ok, why = _query2(in_dim, 256, 512, min(depth, 3), depth)
            assert ok, (depth, in_dim, why)
            ok, why = _query(in_dim, 256, 512, depth)                 # both networks at this depth: the actor's LDS decides
            assert ok == (in_dim <= LDS_TABLE[256][depth - 1]), (depth, in_dim, why)
            if not ok:
                assert "LDS" in why, why


def test_the_split_chains_limits_are_refused_by_name():
    ok, why = _query(65, 256, 512, 3)
    assert not ok and "wide pair" in why and "in_dim <= 64" in why and "65" in why, why
    ok, why = _query(8, 256, 512, 3, B=513)
    assert not ok and "wide pair" in why and "B <= 512" in why and "513" in why, why
    assert _query(64, 256, 512, 3, B=512)[0]


@pytest.mark.parametrize("ha,hc", [(512, 512), (128, 512), (512, 256)])
def test_other_512_wide_combinations_are_not_instantiated(ha, hc):
    for depth in (1, 3, 7):
        ok, why = _query(8, ha, hc, depth)
        assert not ok and "not instantiated" in why, (depth, why)


def test_the_narrower_pairs_answer_as_before():
    for ha in WIDTHS:
        for hc in WIDTHS:
            ok, why = _query(8, ha, hc, 2)
            assert ok == ((ha, hc) in PAIRS), (ha, hc, why)
            if not ok:
                assert "not instantiated" in why, (ha, hc, why)


def _seg_len(in_dim, H, depth, out_dim):
    pad4 = lambda x: (x + 3) // 4 * 4
    return pad4(out_dim * H) + pad4(out_dim)


@pytest.mark.parametrize("depth,B", [(3, 256), (1, 17), (7, 512)])
def test_split_workspace_is_the_panel_layout(depth, B):
    """csrc/ppo_update_dev.hpp: ws_layout -- per network hbuf and dbuf ([depth][Bp][H]), the output partials and xbuf."""
    Bp = (B + 63) // 64 * 64
    take = lambda floats: (floats * 4 + 255) // 256 * 256
    want = 0
    for H, out_dim in ((256, 5), (512, 1)):
        want += 2 * take(depth * Bp * H) + take((B + 15) // 16 * _seg_len(0, H, depth, out_dim)) + take(Bp * 64)
    assert _ws_bytes(_layout_args(256, 512, depth, 0, B=B, stride=B, actor_depth=depth)) == want


def test_no_row_pairs_for_the_wide_pair():
    for depth in (1, 3, 5):
        assert _err_off(_layout_args(256, 512, depth, 1)) == -1
        assert _err_off(_layout_args(256, 512, depth, 0)) == -1


def test_weight_gradient_workgroups_are_the_job_formula():
    from ppo_and_friends_amd import _lib
    jobs = lambda h, d, i: (d - 1) * (h // 16) * ((h // 16 + 1) // 2) + (h // 16) * (((i + 15) // 16 + 1) // 2) + 1
    blocks = {}
    for depth in (1, 3):
        a = _layout_args(256, 512, depth, 0, actor_depth=depth)
        blocks[depth] = _lib.load().ppoaf_ppo_update_split_blocks(C.byref(a))
        assert blocks[depth] == 8 * ((jobs(256, depth, 18) + jobs(512, depth, 54) + 7) // 8)
    assert blocks[3] > 512 and 0 < blocks[1] <= 512


# ---------------------------------------------------------------------------------------------------- the host's answers
def _ppo(mode, O=8, B=64):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cpu")
    env_gen = lambda: SyntheticFixedLengthEnv(4, O, Discrete(3), 8, dev, reward="uniform", seed=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=256), critic_kw_args=dict(hidden_size=512))
    return PPO(env_gen, {"p": (None, sp, sp, Discrete(3), pargs)}, device=dev, random_seed=1, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=4, ts_per_rollout=8, batch_size=B, epochs_per_iter=1,
               save_state=False, update_mode=mode)


def test_update_mode_sets_the_attribute():
    assert _ppo("fused").policies["p"].fused_wide_critic is True
    assert _ppo("auto").policies["p"].fused_wide_critic is False
    assert _ppo("torch").policies["p"].fused_wide_critic is False


def test_unsupported_reason_follows_the_attribute():
    from ppo_and_friends_amd.fused_update import WIDE_WIDTH_PAIRS, WIDTH_PAIRS, FusedPolicyUpdate
    assert WIDE_WIDTH_PAIRS == ((256, 512),) and not set(WIDE_WIDTH_PAIRS) & set(WIDTH_PAIRS)
    pol = _ppo("auto").policies["p"]
    assert FusedPolicyUpdate.unsupported_reason(pol, 64) == TODAY
    assert pol.fused_step_unsupported_reason() == TODAY
    assert FusedPolicyUpdate.fused_mode_would_take(pol, 64) and pol.fused_wide_critic is False
    pol.fused_wide_critic = True
    assert FusedPolicyUpdate.unsupported_reason(pol, 64) == ""
    assert pol.fused_step_unsupported_reason() == ""
    assert not FusedPolicyUpdate.fused_mode_would_take(pol, 64)


def test_unsupported_reason_names_the_limits(monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    from ppo_and_friends_amd.utils import mpi_utils
    pol = _ppo("fused").policies["p"]
    assert FusedPolicyUpdate.unsupported_reason(pol, 512) == ""
    why = FusedPolicyUpdate.unsupported_reason(pol, 513)
    assert "wide pair" in why and "batch size 513 > 512" in why, why
    why = FusedPolicyUpdate.unsupported_reason(_ppo("fused", O=65).policies["p"], 64)
    assert "wide pair" in why and "in_dim 65 / 65 > 64" in why, why
    assert FusedPolicyUpdate.unsupported_reason(_ppo("fused", O=64).policies["p"], 64) == ""
    with monkeypatch.context() as mp:
        mp.setenv("PPOAF_SPLIT_WGRAD", "0")
        why = FusedPolicyUpdate.unsupported_reason(pol, 64)
        assert "PPOAF_SPLIT_WGRAD=0" in why and "the wide pair has no slab form" in why, why
    with monkeypatch.context() as mp:
        mp.setattr(mpi_utils, "get_num_procs", lambda: 2)
        why = FusedPolicyUpdate.unsupported_reason(pol, 64)
        assert "single rank only for now" in why, why
    # with the attribute off none of these is looked at: today's text
    pol.fused_wide_critic = False
    assert FusedPolicyUpdate.unsupported_reason(pol, 513) == TODAY
