"""
CPU tests of the width pairs K6+K7 and K12 are instantiated for (csrc/ppo_update_dev.hpp: PPOAF_WIDTH_PAIRS), the narrow-actor
pairs (64, 256), (32, 256) and (32, 64) among them:

  * ppoaf_ppo_update_check accepts exactly the nine listed pairs of {32, 64, 128, 256}^2 and refuses the other seven by name;
  * for the three narrow-actor pairs the row-tile body's LDS limit is the wider network's, at every depth;
  * the row pairs' record region and error word follow the critic alone: a pair-eligible critic beside a 64-wide actor has
    them, a 64-wide critic or a critic of depth 1 or 5 does not;
  * FusedPolicyUpdate.unsupported_reason takes actor 64 / critic 256 and still refuses actor 256 / critic 64.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_k12_oracle import LDS_TABLE, _query

WIDTHS = (32, 64, 128, 256)
PAIRS = ((32, 32), (64, 64), (128, 128), (256, 256), (128, 256), (64, 128), (64, 256), (32, 256), (32, 64))
NEW_PAIRS = ((64, 256), (32, 256), (32, 64))


def test_exactly_the_nine_pairs_are_accepted():
    for ha in WIDTHS:
        for hc in WIDTHS:
            ok, why = _query(8, ha, hc, 2)
            if (ha, hc) in PAIRS:
                assert ok, (ha, hc, why)
            else:
                assert not ok and "not instantiated" in why, (ha, hc, why)


def test_host_list_is_the_library_list():
    from ppo_and_friends_amd import fused_update
    assert sorted(fused_update.WIDTH_PAIRS) == sorted(PAIRS)


@pytest.mark.parametrize("ha,hc", NEW_PAIRS)
def test_lds_limit_is_the_wider_networks(ha, hc):
    for depth in range(1, 8):
        lim = LDS_TABLE[256][depth - 1] if hc == 256 else 1024
        for in_dim in (1, 17, 64, 376, 1024):
            ok, why = _query(in_dim, ha, hc, depth)
            assert ok == (in_dim <= lim), (ha, hc, depth, in_dim, why)
            if not ok:
                assert "LDS" in why, (ha, hc, depth, in_dim, why)


def _layout_args(ha, hc, critic_depth, pairs, B=256, stride=256, actor_depth=3):
    """Args of the layout entry points, as tests/test_abi.py builds them (no pointer is dereferenced)."""
    from ppo_and_friends_amd import _lib

    def desc(in_dim, hidden, depth, out_dim, offset):
        size, pad4 = 0, lambda x: (x + 3) // 4 * 4
        for l in range(depth + 1):
            i = in_dim if l == 0 else hidden
            o = out_dim if l == depth else hidden
            size += pad4(i * o) + pad4(o)
        return _lib.MlpDesc(in_dim=in_dim, hidden=hidden, depth=depth, out_dim=out_dim, activation=0, offset=offset,
                            size=size, log_std_offset=-1)

    a = _lib.PpoUpdateArgs()
    a.actor = desc(18, ha, actor_depth, 5, 0)
    a.critic = desc(54, hc, critic_depth, 1, a.actor.size)
    a.bucket_total = a.actor.size + a.critic.size
    for f in ("params", "grads", "exp_avg", "exp_avg_sq", "slabs", "step_counts", "lr", "norm_scratch", "obs", "critic_obs",
              "raw_actions", "advantages", "old_log_probs", "rewards_to_go", "values", "perm", "cursor", "vn_mean", "vn_var",
              "vn_count", "loss_partials", "totals"):
        setattr(a, f, 0x10000)
    a.head_kind, a.n_rows, a.B, a.batch_stride, a.n_ranks = 0, 4096, B, stride, 1
    a.beta1, a.beta2, a.adam_eps, a.grad_scale = 0.9, 0.999, 1e-5, 1.0
    a.row_pairs = pairs
    return a


def _ws_bytes(a):
    from ppo_and_friends_amd import _lib
    lib, n = _lib.load(), C.c_int64(0)
    assert lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(n)) == 0, lib.ppoaf_last_error()
    return n.value


def _err_off(a):
    from ppo_and_friends_amd import _lib
    lib, n = _lib.load(), C.c_int64(7)
    assert lib.ppoaf_ppo_update_row_pairs_error_offset(C.byref(a), C.byref(n)) == 0, lib.ppoaf_last_error()
    return n.value


def test_row_pair_region_beside_a_narrow_actor():
    plain, paired = _ws_bytes(_layout_args(64, 256, 3, 0)), _ws_bytes(_layout_args(64, 256, 3, 1))
    assert paired - plain == 256 + 3 * 32 * 2 * 16384
    assert _err_off(_layout_args(64, 256, 3, 1)) == plain
    assert _err_off(_layout_args(64, 256, 3, 1, B=64, stride=256)) == plain       # a tail mini-batch: same place
    assert _err_off(_layout_args(64, 256, 3, 0)) == -1                            # row_pairs off
    assert _err_off(_layout_args(32, 256, 2, 1)) == _ws_bytes(_layout_args(32, 256, 2, 0))
    assert _err_off(_layout_args(32, 64, 3, 1)) == -1
    assert _err_off(_layout_args(64, 256, 1, 1)) == -1 and _err_off(_layout_args(64, 256, 5, 1)) == -1


def test_weight_gradient_workgroups_fit_a_polling_wave():
    """64/256 at depth 3 (the lunar_lander shape): the fused tail's records fit one polling wave (512)."""
    from ppo_and_friends_amd import _lib
    a = _layout_args(64, 256, 3, 0)
    blocks = _lib.load().ppoaf_ppo_update_split_blocks(C.byref(a))
    jobs = lambda h, d, i: (d - 1) * (h // 16) * ((h // 16 + 1) // 2) + (h // 16) * (((i + 15) // 16 + 1) // 2) + 1
    assert blocks == 8 * ((jobs(64, 3, 18) + jobs(256, 3, 54) + 7) // 8)
    assert 0 < blocks <= 512


def _policy(ha, hc):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev, O = torch.device("cpu"), 8
    env_gen = lambda: SyntheticFixedLengthEnv(4, O, Discrete(3), 8, dev, reward="uniform", seed=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=ha, hidden_depth=2), critic_kw_args=dict(hidden_size=hc, hidden_depth=2))
    return PPO(env_gen, {"p": (None, sp, sp, Discrete(3), pargs)}, device=dev, random_seed=1, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=4, ts_per_rollout=8, batch_size=64, epochs_per_iter=1,
               save_state=False, update_mode="auto").policies["p"]


@pytest.mark.parametrize("ha,hc", NEW_PAIRS)
def test_unsupported_reason_takes_the_narrow_actor_pairs(ha, hc):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    pol = _policy(ha, hc)
    assert FusedPolicyUpdate.unsupported_reason(pol, 64) == ""
    assert pol.fused_step_unsupported_reason() == ""


def test_unsupported_reason_still_refuses_a_narrower_critic():
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    why = FusedPolicyUpdate.unsupported_reason(_policy(256, 64), 64)
    assert "not an instantiated pair" in why, why
