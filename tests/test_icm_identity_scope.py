"""
CPU tests of K14's identity-encoder form (ICM(encoded_obs_dim = 0); csrc/icm_update_shapes.hip with enc_hidden = 0) and of
the agent-grouped ICM rows: which ICMs `_describe_icm_identity` and `describe_icm_chain` send to the kernels, that
`_describe_icm` answers what it did, the host-only layout check, the struct size, the smaller workspace, and which grouped
policies `FusedIcmUpdate.unsupported_reason` covers.  Nothing is launched.
"""
import ctypes as C

import numpy as np
import pytest
import torch.nn as nn

# (kind, NA, O, Mi, Mf, d_inv, d_fwd): the blind-maze form, one column, one past a column tile with two model widths
IDENTITY = [("d", 5, 2, 128, 128, 2, 2), ("c", 1, 1, 32, 32, 2, 2), ("d", 3, 17, 64, 32, 3, 1)]


def make_icm(kind, NA, O, Mi, Mf, d_inv=2, d_fwd=2, space=None, activation=None, D=0, E=128):
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, Discrete
    if space is None:
        space = Discrete(NA) if kind == "d" else Box(-1.0, 1.0, (NA,), np.float32)
    icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (O,), np.float32), action_space=space, encoded_obs_dim=D,
              encoder_hidden_size=E, inverse_hidden_size=Mi, forward_hidden_size=Mf, inverse_hidden_depth=d_inv,
              forward_hidden_depth=d_fwd, activation=activation)
    return icm.flatten_parameters_()                     # the bucket as PPOPolicy.finalize lays it out


def hand_walk(O, Mi, Mf, A, Ain, d_inv, d_fwd):
    """Offsets of the two models in a bucket of (weight, bias) pairs in module order, each padded to 4 floats."""
    pad4 = lambda n: (n + 3) // 4 * 4
    lin = lambda i, o: pad4(i * o) + pad4(o)
    inv = lin(2 * O, Mi) + (d_inv - 1) * lin(Mi, Mi) + lin(Mi, A)
    fwd = lin(O + Ain, Mf) + (d_fwd - 1) * lin(Mf, Mf) + lin(Mf, O)
    return 0, 0, inv, inv + fwd


def _lib_built():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("shape", IDENTITY)
def test_identity_shapes_are_described_with_hand_walked_offsets(shape):
    from ppo_and_friends_amd.fused_update import _describe_icm_identity, describe_icm_chain
    kind, NA, O, Mi, Mf, d_inv, d_fwd = shape
    icm = make_icm(*shape)
    assert isinstance(icm.obs_encoder, nn.Identity)
    topo, why = _describe_icm_identity(icm, icm.action_dtype)
    assert topo is not None and why == "", why
    assert topo["general"] is True and topo["identity"] is True
    want = dict(obs_dim=O, enc_hidden=0, enc_dim=O, inv_hidden=Mi, fwd_hidden=Mf, action_dim=NA, fwd_action_dim=NA,
                depth_inv=d_inv, depth_fwd=d_fwd, activation=0, discrete=int(kind == "d"))
    assert {k: topo[k] for k in want} == want
    marks = hand_walk(O, Mi, Mf, NA, NA, d_inv, d_fwd)
    assert (topo["enc_offset"], topo["inv_offset"], topo["fwd_offset"], topo["bucket_total"]) == marks
    assert topo["bucket_total"] == icm.flat_params.numel()
    assert describe_icm_chain(icm, icm.action_dtype) == (topo, "")


def test_describe_icm_still_refuses_the_identity_encoder_and_the_dispatcher_names_the_matching_cause(monkeypatch):
    from ppo_and_friends_amd.fused_update import _describe_icm, _describe_icm_identity, describe_icm_chain
    from ppo_and_friends_amd.spaces import MultiDiscrete
    icm = make_icm("d", 3, 6, 32, 32)
    topo, why = _describe_icm(icm, icm.action_dtype)
    assert topo is None and "identity encoder" in why and "not covered" in why
    # the dispatcher: one-width, widths of their own, identity -- each ICM reaches the chain that is its own
    assert describe_icm_chain(make_icm("d", 3, 6, 64, 64, D=64, E=64), "discrete")[0].get("hidden") == 64
    general = describe_icm_chain(make_icm("d", 3, 6, 32, 32, D=9), "discrete")[0]
    assert general["general"] and not general.get("identity") and general["enc_hidden"] == 128
    # refusals carry the reason of the describer that matches the encoder type
    wide = make_icm("c", 2, 129, 32, 32)
    topo, why = describe_icm_chain(wide, wide.action_dtype)
    assert topo is None and "129" in why and "128" in why, why
    assert _describe_icm_identity(wide, wide.action_dtype) == (None, why)
    topo, why = describe_icm_chain(make_icm("d", 3, 6, 16, 32), "discrete")
    assert topo is None and "(16, 32)" in why
    md = make_icm("d", 3, 6, 32, 32, space=MultiDiscrete([3, 3]))
    topo, why = describe_icm_chain(md, md.action_dtype)
    assert topo is None and "multi-discrete" in why
    topo, why = describe_icm_chain(make_icm("d", 3, 6, 32, 32, activation=nn.Sigmoid()), "discrete")
    assert topo is None and "activation" in why
    topo, why = describe_icm_chain(make_icm("d", 3, 6, 48, 32, D=9, E=48), "discrete")      # an encoder: the shapes describer's reason
    assert topo is None and "encoder width 48" in why
    topo, why = _describe_icm_identity(make_icm("d", 3, 6, 32, 32, D=9), "discrete")
    assert topo is None and "not an identity encoder" in why
    monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "0")                  # no slab form, as for the other general shapes
    topo, why = describe_icm_chain(icm, icm.action_dtype)
    assert topo is None and "PPOAF_SPLIT_WGRAD=0" in why


def test_check_accepts_the_identity_form_and_names_what_it_refuses():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.fused_update import _describe_icm_identity, icm_topology_args
    lib = _lib_built()
    assert C.sizeof(_lib.IcmShapesArgs) == 280
    err = lambda: lib.ppoaf_last_error().decode()
    for shape in IDENTITY:
        icm = make_icm(*shape)
        topo, _ = _describe_icm_identity(icm, icm.action_dtype)
        assert lib.ppoaf_icm_shapes_check(C.byref(icm_topology_args(topo))) == 0, err()
    icm = make_icm("d", 3, 17, 64, 32, 3, 1)                       # O = 17 and A = 3: two biases carry a pad
    topo, _ = _describe_icm_identity(icm, icm.action_dtype)
    b = icm_topology_args(topo)
    b.enc_dim = 16
    assert lib.ppoaf_icm_shapes_check(C.byref(b)) != 0
    assert "enc_hidden=0" in err() and "enc_dim=16" in err() and "obs_dim=17" in err(), err()
    b = icm_topology_args(topo)
    b.obs_dim = b.enc_dim = 129
    assert lib.ppoaf_icm_shapes_check(C.byref(b)) != 0
    assert "enc_hidden=0" in err() and "obs_dim=129" in err() and "128" in err(), err()
    for field, step in (("inv_offset", 4), ("inv_offset", -3), ("fwd_offset", -1), ("bucket_total", -3), ("enc_offset", 4)):
        b = icm_topology_args(topo)
        setattr(b, field, getattr(b, field) + step)                # (an encoder of size 0: enc_offset == inv_offset)
        assert lib.ppoaf_icm_shapes_check(C.byref(b)) != 0, field
        assert "bucket layout" in err() and str(getattr(b, field)) in err(), err()
    # the messages of the forms that were there stay word for word
    b = icm_topology_args(topo)
    b.enc_hidden = 48
    assert lib.ppoaf_icm_shapes_check(C.byref(b)) != 0 and "enc_hidden=48 is not an instantiated width" in err()


def test_workspace_of_the_identity_form_is_smaller_than_behind_an_encoder():
    from ppo_and_friends_amd.fused_update import _describe_icm_identity, describe_icm_chain, icm_scratch_floats, icm_topology_args
    lib = _lib_built()
    for kind, NA, O, Mi, Mf, d_inv, d_fwd in IDENTITY:
        need = []
        for D in (0, O):                                           # identity | encoder of width 32 with an encoding of O
            icm = make_icm(kind, NA, O, Mi, Mf, d_inv, d_fwd, D=D, E=32)
            topo, why = (_describe_icm_identity if D == 0 else describe_icm_chain)(icm, icm.action_dtype)
            assert topo is not None and topo["general"], why
            a = icm_topology_args(topo)
            a.B = 40
            n = C.c_int64(0)
            assert lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(n)) == 0, lib.ppoaf_last_error()
            need.append((n.value, icm_scratch_floats(topo, 40)))
        (ident, (act_i, denc_i)), (enc, (act_e, denc_e)) = need
        assert ident > 0 and ident % 256 == 0 and ident < enc
        pad16 = (O + 15) // 16 * 16
        assert act_i == 2 * 48 * pad16 and act_i < act_e and 0 < denc_i <= 4 < denc_e


def _grouped_policy(shared, **icm_kw):
    import torch
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cpu")
    A, E, T, O, NA = 3, 4, 6, 18, 5
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), dict(enable_icm=True, agent_shared_icm=shared, icm_kw_args=icm_kw))},
              device=dev, random_seed=6, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=8, epochs_per_iter=1)
    return ppo, ppo.policies["mat"]


def test_grouped_policies_are_covered_unless_the_icm_is_agent_shared():
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    ppo, pol = _grouped_policy(False)
    assert pol.agent_grouping and not pol.agent_shared_icm
    assert FusedIcmUpdate.unsupported_reason(pol) == ""
    assert FusedIcmUpdate.unsupported_reason(pol, 8) == "" and FusedIcmUpdate._agents(pol) == 3
    assert FusedIcmUpdate.unsupported_reason(pol, 21845) == ""                       # 65535 (row, agent) samples
    why = FusedIcmUpdate.unsupported_reason(pol, 21846)
    assert "21846" in why and "65536" in why
    assert ppo._overlapped_epochs("mat") is False
    _, pol = _grouped_policy(False, encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=32)   # robot_warehouse's default
    assert FusedIcmUpdate.unsupported_reason(pol) == ""
    _, pol = _grouped_policy(True)
    why = FusedIcmUpdate.unsupported_reason(pol)
    assert "agent_shared_icm" in why and "MultiDiscrete" in why and "group" in why


def test_a_dropped_loader_gives_back_the_draw_it_made_ahead():
    """The fused ICM epoch draws the next shuffle ahead (PermutationLoader.prefetch), now for grouped policies too.  A loader
    with a cache of its own that goes away with that draw unconsumed must leave the generator where the reference's stream
    is: the next loader on the generator receives exactly that draw.  A shared cache (PPO.train_on_rollout's) keeps it."""
    import torch
    from ppo_and_friends_amd.ppo import PermutationLoader

    class Rows:
        device = torch.device("cpu")

        def __len__(self):
            return 10

    want = PermutationLoader(Rows(), 4, torch.Generator().manual_seed(3))
    want = [want.epoch_permutation().clone() for _ in range(3)]
    g = torch.Generator().manual_seed(3)
    loader = PermutationLoader(Rows(), 4, g)
    got = [loader.epoch_permutation().clone()]
    loader.prefetch()
    got.append(loader.epoch_permutation().clone())
    loader.prefetch()                                              # drawn ahead, never consumed by this loader
    loader = PermutationLoader(Rows(), 4, g)
    got.append(loader.epoch_permutation().clone())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    shared, g = {}, torch.Generator().manual_seed(3)
    loader = PermutationLoader(Rows(), 4, g, shared)
    assert torch.equal(loader.epoch_permutation(), want[0])
    loader.prefetch()
    state = g.get_state()
    del loader
    assert torch.equal(g.get_state(), state) and shared["perm"] is not None
    assert torch.equal(PermutationLoader(Rows(), 4, g, shared).epoch_permutation(), want[1])
