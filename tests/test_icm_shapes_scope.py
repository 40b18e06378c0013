"""
CPU tests of K14's chain for ICMs with widths of their own (csrc/icm_update_shapes.hip): which ICMs `_describe_icm` sends
to it, what it still refuses and why, that the one-width description is what it was, and the C boundary (header, ctypes
table, struct size, the host-only layout check).  Nothing is launched.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppoaf_hip.h")
SOURCE = os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "icm_update_shapes.hip")
SYMBOLS = ("ppoaf_icm_shapes_check", "ppoaf_icm_shapes_workspace_bytes", "ppoaf_icm_shapes_fwd_bwd", "ppoaf_icm_shapes_wgrad",
           "ppoaf_icm_shapes_intrinsic_reward")

# the shapes of tests/test_gpu_icm_shapes.py's oracle cases: (kind, NA, O, E, D, Mi, Mf, d_inv, d_fwd)
GENERAL = [("d", 3, 6, 128, 9, 32, 32, 2, 2), ("c", 1, 2, 128, 2, 32, 32, 2, 2), ("d", 5, 18, 64, 17, 64, 32, 3, 1),
           ("c", 6, 17, 128, 16, 128, 128, 2, 2), ("c", 2, 3, 32, 128, 32, 32, 2, 2), ("d", 3, 6, 64, 9, 32, 32, 2, 2)]


def make_icm(kind, NA, O, E, D, Mi, Mf, d_inv=2, d_fwd=2, space=None, activation=None):
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, Discrete
    if space is None:
        space = Discrete(NA) if kind == "d" else Box(-1.0, 1.0, (NA,), np.float32)
    icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (O,), np.float32), action_space=space, encoded_obs_dim=D,
              encoder_hidden_size=E, inverse_hidden_size=Mi, forward_hidden_size=Mf, inverse_hidden_depth=d_inv,
              forward_hidden_depth=d_fwd, activation=activation)
    return icm.flatten_parameters_()                     # the bucket as PPOPolicy.finalize lays it out


def describe(icm):
    from ppo_and_friends_amd.fused_update import _describe_icm
    return _describe_icm(icm, icm.action_dtype)


def hand_walk(O, E, D, Mi, Mf, A, Ain, d_inv, d_fwd):
    """Offsets of the three networks in a bucket of (weight, bias) pairs in module order, each padded to 4 floats."""
    pad4 = lambda n: (n + 3) // 4 * 4
    lin = lambda i, o: pad4(i * o) + pad4(o)
    enc = lin(O, E) + 2 * lin(E, E) + lin(E, D)
    inv = lin(2 * D, Mi) + (d_inv - 1) * lin(Mi, Mi) + lin(Mi, A)
    fwd = lin(D + Ain, Mf) + (d_fwd - 1) * lin(Mf, Mf) + lin(Mf, D)
    return 0, enc, enc + inv, enc + inv + fwd


@pytest.mark.parametrize("shape", GENERAL)
def test_general_shapes_are_described_with_hand_walked_offsets(shape):
    kind, NA, O, E, D, Mi, Mf, d_inv, d_fwd = shape
    topo, why = describe(make_icm(*shape))
    assert topo is not None and why == "", why
    assert topo["general"] is True
    want = dict(obs_dim=O, enc_hidden=E, enc_dim=D, inv_hidden=Mi, fwd_hidden=Mf, action_dim=NA, fwd_action_dim=NA,
                depth_inv=d_inv, depth_fwd=d_fwd, activation=0, discrete=int(kind == "d"))
    assert {k: topo[k] for k in want} == want
    marks = hand_walk(O, E, D, Mi, Mf, NA, NA, d_inv, d_fwd)
    assert (topo["enc_offset"], topo["inv_offset"], topo["fwd_offset"], topo["bucket_total"]) == marks


def test_refusals_name_their_cause(monkeypatch):
    from ppo_and_friends_amd.spaces import MultiDiscrete
    for shape, needle in ((("d", 3, 6, 48, 9, 32, 32), "encoder width 48"), (("d", 3, 6, 128, 9, 16, 32), "(16, 32)"),
                          (("d", 3, 6, 128, 9, 32, 16), "(32, 16)"), (("c", 2, 6, 128, 129, 32, 32), "encoded dim 129")):
        topo, why = describe(make_icm(*shape))
        assert topo is None and needle in why, (shape, why)
    topo, why = describe(make_icm("d", 3, 6, 128, 0, 32, 32))
    assert topo is None and "identity encoder" in why and "not covered" in why
    topo, why = describe(make_icm("d", 3, 6, 128, 9, 32, 32, space=MultiDiscrete([3, 3])))
    assert topo is None and "multi-discrete" in why
    topo, why = describe(make_icm("d", 3, 6, 128, 9, 32, 32, activation=nn.Sigmoid()))
    assert topo is None and "activation" in why
    monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "0")       # the general chain has no slab form; the one-width chain has
    topo, why = describe(make_icm("d", 3, 6, 128, 9, 32, 32))
    assert topo is None and "PPOAF_SPLIT_WGRAD=0" in why
    assert describe(make_icm("d", 3, 6, 64, 64, 64, 64))[0] is not None


@pytest.mark.parametrize("H", [64, 128])
def test_one_width_shapes_keep_their_description(H):
    O, NA = 7, 3
    topo, why = describe(make_icm("d", NA, O, H, H, H, H, 3, 1))
    assert why == ""
    pad4 = lambda n: (n + 3) // 4 * 4
    enc = H * O + H + 3 * (H * H + H)
    inv = 2 * H * H + H + 2 * (H * H + H) + NA * H + pad4(NA)
    fwd = H * (H + NA) + H + H * H + H
    assert topo == dict(obs_dim=O, hidden=H, action_dim=NA, fwd_action_dim=NA, depth_inv=3, depth_fwd=1, activation=0,
                        discrete=1, enc_offset=0, inv_offset=enc, fwd_offset=enc + inv, bucket_total=enc + inv + fwd)


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bint\s+(ppoaf_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_ctypes_table_and_struct_size_agree():
    from ppo_and_friends_amd import _lib
    d = _declared()
    for name in SYMBOLS:
        assert name in d, f"include/ppoaf_hip.h does not declare {name}"
        assert len(_lib.SIGNATURES[name][1]) == d[name], name
    asserted = re.search(r"static_assert\(sizeof\(ppoaf_icm_shapes_args_t\) == (\d+)", open(SOURCE).read())
    assert asserted and C.sizeof(_lib.IcmShapesArgs) == int(asserted.group(1))
    for field, off in re.findall(r"PPOAF_LAYOUT\(ppoaf_icm_shapes_args_t, (\w+), (\d+)\);", open(SOURCE).read()):
        assert getattr(_lib.IcmShapesArgs, field).offset == int(off), field
    text = open(HEADER).read()
    head = text[:text.index("} ppoaf_icm_shapes_args_t;")]
    block = head[head.rindex("/* ----"):]                            # the section comment the declarations sit under
    for cite in ("ppo.py:2487-2567", "icm.py:227-430", "encoders.py:9-56", "ppo_policy.py:954-1007"):
        assert cite in block, cite


def test_check_rejects_a_layout_off_by_one_pad_without_a_device():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.csrc import build
    from ppo_and_friends_amd.fused_update import icm_topology_args
    build.build(verbose=False)
    lib = _lib.load()
    topo, _ = describe(make_icm("d", 3, 6, 128, 9, 32, 32))        # D = 9 and A = 3: two biases carry a pad
    a = icm_topology_args(topo)
    assert lib.ppoaf_icm_shapes_check(C.byref(a)) == 0, lib.ppoaf_last_error()
    for field, step in (("inv_offset", -3), ("fwd_offset", -1), ("bucket_total", -3), ("bucket_total", 4)):
        b = icm_topology_args(topo)
        setattr(b, field, getattr(b, field) + step)                # what an unpadded bias of 9 (or 3) floats would give
        assert lib.ppoaf_icm_shapes_check(C.byref(b)) != 0, field
        assert "bucket layout" in lib.ppoaf_last_error().decode()
    b = icm_topology_args(topo)
    b.enc_hidden = 48
    assert lib.ppoaf_icm_shapes_check(C.byref(b)) != 0 and "enc_hidden=48" in lib.ppoaf_last_error().decode()
    need = C.c_int64(0)
    a.B = 40
    assert lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)) == 0 and need.value > 0 and need.value % 256 == 0
