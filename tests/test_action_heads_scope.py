"""
CPU tests of the scope of the MultiDiscrete / MultiBinary heads on the fused kernels (csrc/action_heads.hpp): which
action spaces FusedPolicyUpdate.unsupported_reason accepts, only for policies built with update_mode="fused", the C-ABI
fields that carry the slice table, and the library's validation of them.  No kernel is launched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ppo_and_friends_amd import _lib
from ppo_and_friends_amd import kernels as K
from ppo_and_friends_amd.fused_update import FusedPolicyUpdate, action_head
from ppo_and_friends_amd.spaces import Box, Discrete, MultiBinary, MultiDiscrete


def _ppo(space, mode, O=5):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    dev = torch.device("cpu")
    env_gen = lambda: SyntheticFixedLengthEnv(4, O, space, 8, dev, reward="uniform", seed=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    return PPO(env_gen, {"p": (None, sp, sp, space, {})}, device=dev, random_seed=1, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=4, ts_per_rollout=8, batch_size=16, epochs_per_iter=1,
               save_state=False, update_mode=mode)


@pytest.mark.parametrize("nvec", [[3, 4], [2, 2, 2, 2], [8], [1, 3], [1] * 8, [3, 3, 2]])
def test_covered_multi_discrete_spaces(nvec):
    pol = _ppo(MultiDiscrete(nvec), "fused").policies["p"]
    assert pol.fused_action_heads
    assert action_head(pol) == (K.HEAD_MULTI_CATEGORICAL, tuple(nvec), "")
    assert FusedPolicyUpdate.unsupported_reason(pol, 16) == ""
    assert pol.fused_step_unsupported_reason() == ""


@pytest.mark.parametrize("n", [1, 4, 8])
def test_covered_multi_binary_spaces(n):
    pol = _ppo(MultiBinary(n), "fused").policies["p"]
    assert action_head(pol) == (K.HEAD_BERNOULLI, (), "")
    assert FusedPolicyUpdate.unsupported_reason(pol, 16) == ""


@pytest.mark.parametrize("space,needle", [(MultiDiscrete([5, 4]), "MultiDiscrete([5, 4])"),
                                          (MultiDiscrete([1] * 9), "1 .. 8 slices"),
                                          (MultiDiscrete([9]), "8 classes in all"),
                                          (MultiBinary(9), "MultiBinary(9)")])
def test_larger_spaces_keep_a_reason(space, needle):
    pol = _ppo(space, "fused").policies["p"]
    why = FusedPolicyUpdate.unsupported_reason(pol, 16)
    assert needle in why, why
    assert pol.fused_step_unsupported_reason() == why


@pytest.mark.parametrize("space", [MultiDiscrete([3, 3, 2]), MultiBinary(5)])
@pytest.mark.parametrize("mode", ["auto", "torch"])
def test_only_fused_mode_takes_the_new_heads(space, mode):
    """"auto" keeps the torch-ROCm path for these heads (for now): the reason says so, and the flag is off."""
    pol = _ppo(space, mode).policies["p"]
    assert not pol.fused_action_heads
    assert "update_mode='fused'" in FusedPolicyUpdate.unsupported_reason(pol, 16)
    pol.fused_action_heads = True
    assert FusedPolicyUpdate.unsupported_reason(pol, 16) == ""


@pytest.mark.parametrize("mode", ["auto", "fused"])
def test_discrete_and_box_do_not_depend_on_the_flag(mode):
    for space, head in ((Discrete(3), K.HEAD_CATEGORICAL), (Box(-1.0, 1.0, (2,), np.float32), K.HEAD_GAUSSIAN)):
        pol = _ppo(space, mode).policies["p"]
        assert action_head(pol)[0] == head and FusedPolicyUpdate.unsupported_reason(pol, 16) == ""


def test_slice_table_is_appended_to_both_arg_structs():
    """Every existing field keeps its offset: the slice table comes after row_pairs / critic_obs_copy_out."""
    for cls, last in ((_lib.PpoUpdateArgs, "row_pairs"), (_lib.PolicyStepArgs, "critic_obs_copy_out")):
        names = [f[0] for f in cls._fields_]
        assert names[-3:] == [last, "n_action_slices", "action_slices"], names[-3:]
        end = getattr(cls, last).offset + getattr(cls, last).size
        assert cls.n_action_slices.offset == end
        assert cls.action_slices.offset == end + 4 and cls.action_slices.size == 32
    assert _lib.ABI_VERSION == 7
    assert (K.HEAD_CATEGORICAL, K.HEAD_GAUSSIAN, K.HEAD_MULTI_CATEGORICAL, K.HEAD_BERNOULLI) == (0, 1, 2, 3)


def _mlp(in_dim, hidden, depth, out_dim, offset):
    size, pad4 = 0, lambda x: (x + 3) // 4 * 4
    for l in range(depth + 1):
        i = in_dim if l == 0 else hidden
        o = out_dim if l == depth else hidden
        size += pad4(i * o) + pad4(o)
    return _lib.MlpDesc(in_dim=in_dim, hidden=hidden, depth=depth, out_dim=out_dim, activation=0, offset=offset,
                        size=size, log_std_offset=-1)


def _update_args(head, out_dim, slices):
    a = _lib.PpoUpdateArgs()
    a.actor = _mlp(4, 128, 3, out_dim, 0)
    a.critic = _mlp(4, 128, 3, 1, a.actor.size)
    a.bucket_total = a.actor.size + a.critic.size
    for f in ("params", "grads", "exp_avg", "exp_avg_sq", "slabs", "step_counts", "lr", "norm_scratch", "obs", "critic_obs",
              "raw_actions", "advantages", "old_log_probs", "rewards_to_go", "values", "perm", "cursor", "vn_mean", "vn_var",
              "vn_count", "loss_partials", "totals"):
        setattr(a, f, 0x10000)                        # never dereferenced by the host-side entry point below
    a.head_kind, a.n_rows, a.B, a.batch_stride, a.n_ranks = head, 4096, 256, 256, 1
    a.n_action_slices = len(slices)
    for j, k in enumerate(slices):
        a.action_slices[j] = k
    return a


@pytest.mark.parametrize("head,out_dim,slices,needle", [
    (K.HEAD_MULTI_CATEGORICAL, 7, [3, 4], None),
    (K.HEAD_BERNOULLI, 5, [], None),
    (K.HEAD_MULTI_CATEGORICAL, 7, [3, 3], "sum to 6, the actor has 7"),
    (K.HEAD_MULTI_CATEGORICAL, 4, [4, 0], "action_slices[1]=0"),
    (K.HEAD_MULTI_CATEGORICAL, 4, [], "n_action_slices=0"),
    (4, 4, [], "head_kind=4"),
])
def test_the_library_validates_the_head_fields(head, out_dim, slices, needle):
    lib = _lib.load()
    a = _update_args(head, out_dim, slices)
    n = C.c_int64(0)
    rc = lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(n))
    if needle is None:
        assert rc == 0, lib.ppoaf_last_error()
    else:
        assert rc != 0 and needle in lib.ppoaf_last_error().decode()


def test_the_new_heads_refuse_a_log_std():
    lib = _lib.load()
    a = _update_args(K.HEAD_BERNOULLI, 4, [])
    a.actor.log_std_offset = a.actor.size
    a.actor.size += 4
    a.critic.offset = a.actor.size
    a.bucket_total = a.actor.size + a.critic.size
    assert lib.ppoaf_ppo_update_split_workspace_bytes(C.byref(a), C.byref(C.c_int64(0))) != 0
    assert "log_std" in lib.ppoaf_last_error().decode()
