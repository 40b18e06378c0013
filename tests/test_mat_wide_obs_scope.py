"""
CPU tests of the MAT kernels' observation-width scope (no GPU, no launch): `fused_update._describe_mat` takes per-agent
observations up to 128 wide and its bucket is the padded-size table of csrc/mat_update.hip (mat_offset_table, read back
from the library's own refusal text); `ppoaf_mat_policy_step` (K16) and `ppoaf_mat_update_fwd_bwd` (K15) refuse
obs_dim = 129 by size and get past the size check at 128; K20's bound of 64 is named by
`MATPolicy.inference_unsupported_reason`.
"""
import ctypes as C
import os
import re
import sys
import types

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

A, NA = 3, 5


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def mat_sizes(O, NA, D=64):
    """MATActorCritic's parameter tensors in module order."""
    sizes = [D * (NA + 1)] + [D] * 8 + [D * D, D] * 8 + [D * D, D] * 2 + [D * D, D, D, D, NA * D, NA]
    sizes += [O, O, D * O, D] + [D] * 6 + [D * D, D] * 4 + [D * D, D] * 2 + [D * D, D, D, D, D, 1]
    assert len(sizes) == 63
    return sizes


def padded_total(O, NA):
    return sum((s + 3) // 4 * 4 for s in mat_sizes(O, NA))


def _describe(O):
    import mat_float64 as M
    from ppo_and_friends_amd.fused_update import _describe_mat
    ac = M.make_network(O, NA, A, 11)
    return _describe_mat(types.SimpleNamespace(actor_critic=ac, action_dtype="discrete"))


def test_the_padded_size_table_at_the_old_limit():
    assert padded_total(32, 5) == 78988


@pytest.mark.parametrize("O", [33, 64, 65, 71, 128])
def test_describe_mat_accepts_wide_observations(O):
    topo, why = _describe(O)
    assert topo is not None and why == "", why
    assert topo["obs_dim"] == O and topo["num_agents"] == A and topo["num_actions"] == NA
    assert topo["bucket_total"] == padded_total(O, NA)
    offs, off = [], 0
    for s in mat_sizes(O, NA):
        offs.append(off)
        off += (s + 3) // 4 * 4
    assert topo["offsets"] == offs


def test_describe_mat_refuses_129_and_names_the_bound():
    topo, why = _describe(129)
    assert topo is None and "obs 129" in why and "128" in why and "32" not in why


def _update_args(built, O, **over):
    a = built.MatUpdateArgs()
    a.obs_dim, a.num_agents, a.num_actions, a.embedding = O, A, NA, 64
    off = 0
    for i, s in enumerate(mat_sizes(O, NA)):
        a.offsets[i] = off
        off += (s + 3) // 4 * 4
    a.bucket_total = off
    for f in ("params", "grads", "slabs", "critic_obs", "raw_actions", "advantages", "old_log_probs", "rewards_to_go", "values",
              "perm", "cursor", "vn_mean", "vn_var", "vn_count", "loss_partials", "totals"):
        setattr(a, f, 0x10000)                           # never dereferenced: every call below is refused on the host
    a.B, a.batch_stride, a.n_rows, a.n_ranks = 16, 16, 64, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _step_args(built, O, **over):
    a = built.MatStepArgs()
    a.obs_dim, a.num_agents, a.num_actions, a.embedding, a.actor_obs_dim = O, A, NA, 64, O
    a.params = a.critic_obs = a.action_out = a.logp_out = a.value_out = 0x10000
    a.E = 8
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_k15_refuses_129_by_size_and_passes_the_size_check_at_128(built):
    lib = built.load()
    assert lib.ppoaf_mat_update_fwd_bwd(C.byref(_update_args(built, 129)), None) == -1
    msg = lib.ppoaf_last_error().decode()
    assert "obs_dim=129" in msg and "128" in msg, msg
    # at 128 the size check passes: the call is refused by a later one (B = 0), still on the host
    assert lib.ppoaf_mat_update_fwd_bwd(C.byref(_update_args(built, 128, B=0)), None) == -1
    msg = lib.ppoaf_last_error().decode()
    assert "B=0" in msg and "obs_dim" not in msg, msg


@pytest.mark.parametrize("O", [32, 33, 71, 128])
def test_k15s_own_table_is_the_python_table(built, O):
    """A wrong bucket_total is refused with the total the library's table gives."""
    lib = built.load()
    assert lib.ppoaf_mat_update_fwd_bwd(C.byref(_update_args(built, O, bucket_total=4)), None) == -1
    m = re.search(r"the topology needs (\d+)", lib.ppoaf_last_error().decode())
    assert m and int(m.group(1)) == padded_total(O, NA), lib.ppoaf_last_error()


def test_k16_refuses_129_by_size_and_passes_the_size_check_at_128(built):
    lib = built.load()
    assert lib.ppoaf_mat_policy_step(C.byref(_step_args(built, 129)), None) == -1
    msg = lib.ppoaf_last_error().decode()
    assert "sizes" in msg and "obs 129" in msg and "128" in msg, msg
    assert lib.ppoaf_mat_policy_step(C.byref(_step_args(built, 128, E=0)), None) == -1
    msg = lib.ppoaf_last_error().decode()
    assert "E=0" in msg and "sizes" not in msg, msg


@pytest.mark.parametrize("O,covered", [(64, True), (65, False), (128, False)])
def test_inference_reason_names_k20s_bound(O, covered):
    """MATPolicy.inference_unsupported_reason on a stand-in for a device policy (no device here): K15 / K16 take the width,
    K20 stops at 64 and says so."""
    import torch
    import mat_float64 as M
    from ppo_and_friends_amd.fused_update import _describe_mat
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    ac = M.make_network(O, NA, A, 11)
    pol = types.SimpleNamespace(device=torch.device("cuda", 0), update_mode="auto", policy_params=ac.flat_params, actor_critic=ac,
                                action_dtype="discrete", critic=ac.critic)
    pol.fused_step_unsupported_reason = lambda: _describe_mat(pol)[1]
    why = MATPolicy.inference_unsupported_reason(pol)
    assert pol.fused_step_unsupported_reason() == ""
    if covered:
        assert why == ""
    else:
        assert f"observations {O} wide" in why and "64" in why
