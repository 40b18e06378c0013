"""
CPU tests of the agent-shared ICM (MultiDiscrete over the group, ppo.py:2520-2538) on K14's shapes chain: what
`describe_icm_chain(..., multi_discrete=True)` describes and refuses, that without the keyword nothing changed, the C
boundary (`n_action_slices` in the place of the spare field, the host-only check and its messages) and the opt-in
`PPOPolicy.fused_shared_icm` as `FusedIcmUpdate.unsupported_reason` reads it.  Nothing is launched.
"""
import ctypes as C

import numpy as np
import pytest
import torch



def make_icm(kind, NA, O, E, D, Mi, Mf, d_inv=2, d_fwd=2, space=None, activation=None):
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, Discrete
    if space is None:
        space = Discrete(NA) if kind == "d" else Box(-1.0, 1.0, (NA,), np.float32)
    icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (O,), np.float32), action_space=space, encoded_obs_dim=D,
              encoder_hidden_size=E, inverse_hidden_size=Mi, forward_hidden_size=Mf, inverse_hidden_depth=d_inv,
              forward_hidden_depth=d_fwd, activation=activation)
    return icm.flatten_parameters_()                     # the bucket as PPOPolicy.finalize lays it out


def hand_walk(O, E, D, Mi, Mf, A, Ain, d_inv, d_fwd):
    """Offsets of the three networks in a bucket of (weight, bias) pairs in module order, each padded to 4 floats."""
    pad4 = lambda n: (n + 3) // 4 * 4
    lin = lambda i, o: pad4(i * o) + pad4(o)
    enc = lin(O, E) + 2 * lin(E, E) + lin(E, D)
    inv = lin(2 * D, Mi) + (d_inv - 1) * lin(Mi, Mi) + lin(Mi, A)
    fwd = lin(D + Ain, Mf) + (d_fwd - 1) * lin(Mf, Mf) + lin(Mf, D)
    return 0, enc, enc + inv, enc + inv + fwd


def _describe(icm, **kw):
    from ppo_and_friends_amd.fused_update import describe_icm_chain
    return describe_icm_chain(icm, icm.action_dtype, **kw)


def _shared_icm(nvec, O=54, E=128, D=128, Mi=128, Mf=128):
    from ppo_and_friends_amd.spaces import MultiDiscrete
    return make_icm("d", sum(nvec), O, E, D, Mi, Mf, space=MultiDiscrete(list(nvec)))


# (nvec, O, E, D, Mi, Mf): the default ICM over 3 x Discrete(5), the identity form, the baselines' D 9 / M 32 form
FORMS = [([5, 5, 5], 54, 128, 128, 128, 128), ([5, 5, 5], 54, 0, 0, 32, 64), ([8, 8], 36, 128, 9, 32, 32)]


@pytest.mark.parametrize("form", FORMS, ids=["default", "identity", "D9-M32"])
def test_equal_class_counts_are_described_on_the_shapes_chain(form):
    nvec, O, E, D, Mi, Mf = form
    topo, why = _describe(_shared_icm(nvec, O, E or 128, D, Mi, Mf), multi_discrete=True)
    assert topo is not None and why == "", why
    ident = D == 0
    Dk = O if ident else D
    want = dict(general=True, obs_dim=O, enc_hidden=0 if ident else E, enc_dim=Dk, inv_hidden=Mi, fwd_hidden=Mf, discrete=1,
                n_action_slices=len(nvec), action_dim=sum(nvec), fwd_action_dim=sum(nvec), depth_inv=2, depth_fwd=2, activation=0)
    assert {k: topo[k] for k in want} == want
    assert "hidden" not in topo and bool(topo.get("identity")) == ident
    if ident:
        pad4 = lambda n: (n + 3) // 4 * 4
        lin = lambda i, o: pad4(i * o) + pad4(o)
        inv = lin(2 * O, Mi) + lin(Mi, Mi) + lin(Mi, sum(nvec))
        fwd = lin(O + sum(nvec), Mf) + lin(Mf, Mf) + lin(Mf, O)
        marks = (0, 0, inv, inv + fwd)
    else:
        marks = hand_walk(O, E, D, Mi, Mf, sum(nvec), sum(nvec), 2, 2)
    assert (topo["enc_offset"], topo["inv_offset"], topo["fwd_offset"], topo["bucket_total"]) == marks
    # the C side agrees with the description
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.csrc import build
    from ppo_and_friends_amd.fused_update import icm_topology_args
    build.build(verbose=False)
    a = icm_topology_args(topo)
    assert a.n_action_slices == len(nvec)
    assert _lib.load().ppoaf_icm_shapes_check(C.byref(a)) == 0, _lib.load().ppoaf_last_error()


def test_refusals_name_their_cause():
    for nvec, needles in (([3, 5], ("class counts",)), ([5, 5, 5, 5], ("20", "16")), ([2] * 9, ("9 slices",)), ([1, 1], ("class count of 1",))):
        topo, why = _describe(_shared_icm(nvec), multi_discrete=True)
        assert topo is None and all(n in why for n in needles), (nvec, why)
        topo, why = _describe(_shared_icm(nvec, D=0, Mi=32, Mf=32), multi_discrete=True)
        assert topo is None and all(n in why for n in needles), (nvec, why)
    # the rules of the describers hold as they are: a width that is not instantiated, the identity form's O <= 128
    topo, why = _describe(_shared_icm([5, 5, 5], Mi=48), multi_discrete=True)
    assert topo is None and "(48, 128)" in why
    topo, why = _describe(_shared_icm([5, 5, 5], O=3 * 43, D=0, Mi=32, Mf=32), multi_discrete=True)
    assert topo is None and "129" in why and "128" in why


def test_without_the_keyword_nothing_changed():
    from ppo_and_friends_amd.fused_update import _describe_icm, describe_icm_chain
    for icm in (_shared_icm([5, 5, 5]), _shared_icm([5, 5, 5], D=0, Mi=32, Mf=32), _shared_icm([8, 8], 36, 128, 9, 32, 32)):
        for got in (describe_icm_chain(icm, "multi-discrete"), describe_icm_chain(icm, "multi-discrete", multi_discrete=False)):
            assert got[0] is None and "multi-discrete" in got[1], got
    assert describe_icm_chain(_shared_icm([5, 5, 5], D=0, Mi=32, Mf=32), "multi-discrete") == \
        (None, "multi-discrete actions are not covered by the fused ICM update")
    # Discrete / Box descriptions do not depend on the keyword, and carry no slices
    for shape in (("d", 3, 6, 128, 9, 32, 32), ("c", 2, 7, 64, 64, 64, 64), ("d", 5, 18, 128, 0, 32, 32)):
        icm = make_icm(*shape)
        plain = describe_icm_chain(icm, icm.action_dtype)
        assert plain[0] is not None and plain == describe_icm_chain(icm, icm.action_dtype, multi_discrete=True)
        assert "n_action_slices" not in plain[0]


def _args(**over):
    """A valid k = 3 / 15-class topology on the D 9 / M 32 form (layout by hand_walk), with fields replaced."""
    from ppo_and_friends_amd import _lib
    f = dict(obs_dim=54, enc_hidden=128, enc_dim=9, inv_hidden=32, fwd_hidden=32, action_dim=15, fwd_action_dim=15, depth_inv=2,
             depth_fwd=2, activation=0, discrete=1, n_action_slices=3)
    f.update(over)
    marks = hand_walk(f["obs_dim"], f["enc_hidden"], f["enc_dim"], f["inv_hidden"], f["fwd_hidden"], f["action_dim"],
                      f["fwd_action_dim"], 2, 2)
    a = _lib.IcmShapesArgs()
    for k, v in f.items():
        setattr(a, k, v)
    a.enc_offset, a.inv_offset, a.fwd_offset, a.bucket_total = marks
    return a


def test_the_host_check_takes_slices_and_refuses_with_the_field_and_the_value():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    lib = _lib.load()
    for k, A in ((3, 15), (2, 16), (8, 16), (2, 4)):
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(n_action_slices=k, action_dim=A, fwd_action_dim=A))) == 0, \
            (k, A, lib.ppoaf_last_error())
    refused = ((dict(discrete=0), ("discrete=0", "n_action_slices=3")),
               (dict(fwd_action_dim=12), ("action_dim=15", "fwd_action_dim=12")),
               (dict(action_dim=16, fwd_action_dim=16), ("action_dim=16", "multiple of n_action_slices=3")),
               (dict(n_action_slices=4, action_dim=4, fwd_action_dim=4), ("action_dim=4", "n_action_slices=4", "fewer than 2")),
               (dict(n_action_slices=9, action_dim=18, fwd_action_dim=18), ("n_action_slices=9", "at most 8")),
               (dict(n_action_slices=2, action_dim=18, fwd_action_dim=18), ("action_dim=18", "[1,16]")))
    for over, needles in refused:
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(**over))) != 0, over
        msg = lib.ppoaf_last_error().decode()
        assert all(n in msg for n in needles), (over, msg)
    # without slices the limit and its words are what they were
    for k in (0, 1):
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(n_action_slices=k))) != 0
        assert "action_dim=15 fwd_action_dim=15 must be in [1,8]" in lib.ppoaf_last_error().decode()
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(n_action_slices=k, action_dim=5, fwd_action_dim=5))) == 0


def test_the_field_sits_in_the_spare_word_and_the_struct_keeps_its_size():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.fused_update import icm_topology_args
    S = _lib.IcmShapesArgs
    assert C.sizeof(S) == 280
    assert S.n_action_slices.offset == S.inputs_in_batch_order.offset + 4 == S.workspace.offset - 4
    assert not hasattr(S, "_pad")
    a = icm_topology_args(dict(general=True, identity=True, n_action_slices=3, action_dim=15))
    assert isinstance(a, S) and (a.n_action_slices, a.action_dim) == (3, 15)
    assert icm_topology_args(dict(general=True, action_dim=5)).n_action_slices == 0


def _cpu_policy(NA, A, **icm_kw):
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cpu")
    E, T, O = 4, 6, 18
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), dict(enable_icm=True, agent_shared_icm=True, icm_kw_args=icm_kw))},
              device=dev, random_seed=6, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=8, epochs_per_iter=1, update_mode="torch", use_graphs=False)
    return ppo.policies["mat"]


def test_the_opt_in_is_what_opens_the_gate():
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    assert PPOPolicy.fused_shared_icm is False
    pol = _cpu_policy(5, 3)
    assert pol.icm_model.action_dtype == "multi-discrete" and pol.action_dtype == "discrete"
    why = FusedIcmUpdate.unsupported_reason(pol, 8)
    assert why == ("agent_shared_icm: one ICM over the MultiDiscrete action space of the whole group (ppo.py:2520-2538) "
                   "is not covered, torch path")
    pol.fused_shared_icm = True
    assert FusedIcmUpdate.unsupported_reason(pol, 8) == ""
    assert FusedIcmUpdate._agents(pol) == 1
    wide = _cpu_policy(9, 2)
    assert "MultiDiscrete" in FusedIcmUpdate.unsupported_reason(wide, 8)
    wide.fused_shared_icm = True
    why = FusedIcmUpdate.unsupported_reason(wide, 8)
    assert "18" in why and "16" in why, why
