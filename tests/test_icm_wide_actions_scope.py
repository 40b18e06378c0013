"""
CPU tests of the wide-action form of K14's shapes chain (Discrete / Box ICM actions of 9 .. 24 classes or dimensions): the
opt-in `PPOPolicy.fused_wide_icm_actions`, what the describers take and refuse with and without it, the library's option bit
PPOAF_ICM_WIDE_ACTIONS in `n_action_slices` (the host-only check and its messages, the workspace), and that an ICM with
action widths <= 8 is described, checked and sized exactly as without the opt-in.  Nothing is launched.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_icm_shared_scope import hand_walk, make_icm

REFUSAL = "action widths ({0}, {0}) must be in [1, 8]"
# (O, E, D, Mi, Mf; D 0 = the identity encoder): mario_bros_ram's ICM, widths of its own, the default one-width ICM, the identity form
FORMS = {"mario": (256, 128, 9, 32, 32), "own": (10, 64, 17, 32, 128), "default128": (20, 128, 128, 128, 128), "identity": (12, 128, 0, 64, 32)}


def _load():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    return _lib.load()


def _describe(icm, **kw):
    from ppo_and_friends_amd.fused_update import describe_icm_chain
    return describe_icm_chain(icm, icm.action_dtype, **kw)


def test_the_attribute_defaults_to_false_and_no_update_mode_sets_it():
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    assert PPOPolicy.fused_wide_icm_actions is False and MATPolicy.fused_wide_icm_actions is False
    for mode in ("auto", "fused", "torch"):
        pol = _cpu_policy(18, update_mode=mode)
        assert "fused_wide_icm_actions" not in vars(pol) and pol.fused_wide_icm_actions is False


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", ["d", "c"])
def test_without_the_opt_in_the_refusals_keep_their_words(form, kind):
    from ppo_and_friends_amd.fused_update import _describe_icm_identity, _describe_icm_shapes
    for A in (9, 17, 18, 24, 25):
        icm = make_icm(kind, A, *FORMS[form])
        for got in (_describe(icm), _describe(icm, wide_actions=False), _describe(icm, multi_discrete=True)):
            assert got == (None, REFUSAL.format(A)), got
        one = _describe_icm_identity if form == "identity" else _describe_icm_shapes
        assert one(icm, icm.action_dtype) == (None, REFUSAL.format(A))


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", ["d", "c"])
def test_with_it_nine_to_twenty_four_are_described_and_the_library_agrees(form, kind):
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.fused_update import WIDE_HEAD_MAX, icm_scratch_floats, icm_topology_args
    assert WIDE_HEAD_MAX == 24 and _lib.ICM_WIDE_ACTIONS == 0x100
    lib = _load()
    O, E, D, Mi, Mf = FORMS[form]
    ident = D == 0
    for A in (9, 16, 17, 18, 24):
        icm = make_icm(kind, A, O, E, D, Mi, Mf)
        topo, why = _describe(icm, wide_actions=True)
        assert topo is not None and why == "", why
        want = dict(general=True, obs_dim=O, enc_hidden=0 if ident else E, enc_dim=O if ident else D, inv_hidden=Mi, fwd_hidden=Mf,
                    discrete=int(kind == "d"), n_action_slices=_lib.ICM_WIDE_ACTIONS, action_dim=A, fwd_action_dim=A, depth_inv=2,
                    depth_fwd=2, activation=0)
        assert {k: topo[k] for k in want} == want
        assert "hidden" not in topo and bool(topo.get("identity")) == ident        # (the one-width chain is not the one)
        if not ident:
            assert (topo["enc_offset"], topo["inv_offset"], topo["fwd_offset"], topo["bucket_total"]) == hand_walk(O, E, D, Mi, Mf, A, A, 2, 2)
        a = icm_topology_args(topo)
        assert a.n_action_slices == 0x100 and lib.ppoaf_icm_shapes_check(C.byref(a)) == 0, lib.ppoaf_last_error()
        # the scratch does not depend on the action width: the action panels live in the workspace
        narrow, _ = _describe(make_icm(kind, 5, O, E, D, Mi, Mf), wide_actions=True)
        if narrow.get("general"):
            assert icm_scratch_floats(topo, 100) == icm_scratch_floats(narrow, 100)
    topo, why = _describe(make_icm(kind, 25, O, E, D, Mi, Mf), wide_actions=True)
    assert topo is None and why == "action widths (25, 25) must be in [1, 24]"


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", ["d", "c"])
def test_up_to_eight_the_opt_in_changes_nothing(form, kind):
    for A in (1, 2, 5, 8):
        if kind == "d" and A == 1:
            continue
        icm = make_icm(kind, A, *FORMS[form])
        plain = _describe(icm)
        assert plain[0] is not None and plain == _describe(icm, wide_actions=True)
        assert "n_action_slices" not in plain[0]
    # the default ICM stays on the one-width chain
    if form == "default128":
        assert "hidden" in _describe(make_icm(kind, 5, *FORMS[form]), wide_actions=True)[0]


def test_other_refusals_are_the_describers_own():
    for kw, needle in ((dict(Mi=48), "(48, 32)"), (dict(E=96), "encoder width 96"), (dict(D=130), "encoded dim 130")):
        f = dict(O=10, E=64, D=17, Mi=32, Mf=32)
        f.update(kw)
        icm = make_icm("d", 18, f["O"], f["E"], f["D"], f["Mi"], f["Mf"])
        topo, why = _describe(icm, wide_actions=True)
        assert topo is None and needle in why, why
    # MultiDiscrete keeps its limits with the opt-in: it is not what the flag is about
    from ppo_and_friends_amd.spaces import MultiDiscrete
    md = make_icm("d", 18, 10, 64, 17, 32, 32, space=MultiDiscrete([9, 9]))
    assert _describe(md, wide_actions=True) == (None, "multi-discrete actions are not covered by the fused ICM update")
    topo, why = _describe(md, multi_discrete=True, wide_actions=True)
    assert topo is None and "18" in why and "16" in why


def test_split_wgrad_off_refuses_as_the_chain_does(monkeypatch):
    monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "0")
    for form in ("mario", "identity", "default128"):
        topo, why = _describe(make_icm("d", 18, *FORMS[form]), wide_actions=True)
        assert topo is None and why == "PPOAF_SPLIT_WGRAD=0: the chain for these ICM shapes has no slab form"


# ------------------------------------------------------------------------------------------------------ the library
def _args(bit=True, **over):
    """mario_bros_ram's topology (layout by hand_walk), with fields replaced."""
    from ppo_and_friends_amd import _lib
    f = dict(obs_dim=256, enc_hidden=128, enc_dim=9, inv_hidden=32, fwd_hidden=32, action_dim=18, fwd_action_dim=18, depth_inv=2,
             depth_fwd=2, activation=0, discrete=1, n_action_slices=_lib.ICM_WIDE_ACTIONS if bit else 0)
    f.update(over)
    marks = hand_walk(f["obs_dim"], f["enc_hidden"], f["enc_dim"], f["inv_hidden"], f["fwd_hidden"], f["action_dim"],
                      f["fwd_action_dim"], 2, 2)
    if f["enc_hidden"] == 0:                             # identity encoder: an encoder of size 0
        marks = (0, 0, marks[2] - marks[1], marks[3] - marks[1])
    a = _lib.IcmShapesArgs()
    for k, v in f.items():
        setattr(a, k, v)
    a.enc_offset, a.inv_offset, a.fwd_offset, a.bucket_total = marks
    return a


def test_the_host_check_takes_the_bit_and_refuses_with_the_field_and_the_value():
    lib = _load()
    W = 0x100
    for A in (1, 5, 8, 9, 16, 17, 24):
        for discrete in (1, 0):
            for k in (W, W | 1):
                a = _args(action_dim=A, fwd_action_dim=A, discrete=discrete, n_action_slices=k)
                assert lib.ppoaf_icm_shapes_check(C.byref(a)) == 0, (A, discrete, k, lib.ppoaf_last_error())
    assert lib.ppoaf_icm_shapes_check(C.byref(_args(action_dim=17, fwd_action_dim=5, discrete=0))) == 0      # Box: each in [1,24]
    refused = ((dict(action_dim=25, fwd_action_dim=25), ("action_dim=25", "[1,24]")),
               (dict(action_dim=25, fwd_action_dim=25, discrete=0), ("action_dim=25", "[1,24]")),
               (dict(action_dim=17, fwd_action_dim=25, discrete=0), ("fwd_action_dim=25", "[1,24]")),
               (dict(action_dim=0, fwd_action_dim=18), ("action_dim=0", "[1,24]")),
               (dict(action_dim=18, fwd_action_dim=17), ("discrete=1", "action_dim=18", "fwd_action_dim=17")),
               (dict(n_action_slices=W | 2), ("action_dim=18", "[1,16]", "n_action_slices=2")),
               (dict(n_action_slices=W | 9, action_dim=18, fwd_action_dim=18), ("n_action_slices=9", "at most 8")))
    for over, needles in refused:
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(**over))) != 0, over
        msg = lib.ppoaf_last_error().decode()
        assert all(n in msg for n in needles), (over, msg)
    # an option bit this library does not know is refused, not ignored -- with or without slices
    for word in (0x300, 0x500, 0x10100, 0x302, 0x40000100):
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(n_action_slices=word, action_dim=16, fwd_action_dim=16))) != 0, hex(word)
        msg = lib.ppoaf_last_error().decode()
        assert f"n_action_slices={hex(word)}" in msg and "PPOAF_ICM_WIDE_ACTIONS" in msg, msg
    # with slices the bit changes nothing: MultiDiscrete keeps k <= 8 and 16 classes
    for k, A in ((3, 15), (2, 16), (8, 16)):
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(n_action_slices=W | k, action_dim=A, fwd_action_dim=A))) == 0
    # without the bit every answer is what it was
    for k in (0, 1):
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(bit=False, n_action_slices=k, action_dim=15, fwd_action_dim=15))) != 0
        assert "action_dim=15 fwd_action_dim=15 must be in [1,8]" in lib.ppoaf_last_error().decode()
        assert lib.ppoaf_icm_shapes_check(C.byref(_args(bit=False, n_action_slices=k, action_dim=5, fwd_action_dim=5))) == 0
    assert lib.ppoaf_icm_shapes_check(C.byref(_args(bit=False, n_action_slices=2))) != 0
    assert "action_dim=18 must be in [1,16] with n_action_slices=2" in lib.ppoaf_last_error().decode()


def test_the_struct_keeps_its_size_and_the_bit_rides_in_the_slice_word():
    from ppo_and_friends_amd import _lib
    S = _lib.IcmShapesArgs
    assert C.sizeof(S) == 280 and S.n_action_slices.offset == 260 and S.workspace.offset == 264
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ppoaf_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+PPOAF_ICM_WIDE_ACTIONS\s+0x100\b", header)


def _ws(a, B):
    lib = _load()
    a.B = B
    need = C.c_int64(-1)
    assert lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)) == 0, lib.ppoaf_last_error()
    return int(need.value)


def test_the_workspace_grows_for_wide_launches_only():
    pad = lambda n: (n + 255) // 256 * 256
    for B in (1, 33, 128, 1000):
        bpad = (B + 15) // 16 * 16
        for ident in (False, True):
            shape = dict(obs_dim=40, enc_hidden=0, enc_dim=40) if ident else {}
            for A in (1, 5, 8):
                for discrete in (0, 1):
                    kw = dict(action_dim=A, fwd_action_dim=A, discrete=discrete, **shape)
                    assert _ws(_args(bit=True, **kw), B) == _ws(_args(bit=False, **kw), B)
            narrow = _ws(_args(bit=False, action_dim=8, fwd_action_dim=8, **shape), B)
            for A in (9, 18, 24):
                # the two action panels oI / aF: [Bpad][16] -> [Bpad][32], each rounded up to 256 bytes
                assert _ws(_args(action_dim=A, fwd_action_dim=A, **shape), B) == narrow + 2 * (pad(bpad * 128) - pad(bpad * 64))
            # Box with one side above 8 is a wide launch as well
            assert _ws(_args(action_dim=4, fwd_action_dim=12, discrete=0, **shape), B) == _ws(_args(action_dim=12, fwd_action_dim=12, **shape), B)


def _llvm_tool(name):
    """llvm-objdump / llvm-readelf of the toolchain that built the library: beside the compiler hipcc drives (`hipconfig -l`,
    hipcc's own InstalledDir), beside hipcc itself, or on PATH.  Not found = a failure: this is the only check of its kind."""
    from ppo_and_friends_amd.csrc import build
    hipcc = shutil.which(build.HIPCC) or build.HIPCC
    dirs = []
    for cmd in ([os.path.join(os.path.dirname(hipcc), "hipconfig"), "-l"], ["hipconfig", "-l"]):
        try:
            dirs.append(subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.strip())
        except (OSError, subprocess.CalledProcessError):
            pass
    try:
        version = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout
        dirs += re.findall(r"InstalledDir:\s*(\S+)", version)
    except (OSError, subprocess.CalledProcessError):
        pass
    real = os.path.dirname(os.path.realpath(hipcc))
    dirs += [real, os.path.join(os.path.dirname(real), "llvm", "bin"), os.path.join(os.path.dirname(real), "lib", "llvm", "bin")]
    for d in dirs:
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    found = shutil.which(name)
    assert found, f"{name} not found beside {hipcc} (looked in {dirs}) nor on PATH"
    return found


def test_the_wide_kernels_have_no_private_segment(tmp_path):
    """The per-class arrays of the wide head stay in registers: .private_segment_fixed_size is 0 for every kernel of the
    shapes chain, the 32-column instantiations included (read from the code object's metadata)."""
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    objdump, readelf = _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    lib = shutil.copy(build.LIB, str(tmp_path / "lib.so"))
    subprocess.run([objdump, "--offloading", lib], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL)
    seen = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if build.ARCH not in f:
            continue
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
            name = re.search(r"\.name:\s*(\S+)", blk)
            private = re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk)
            if name and private and "icm_sh_" in name.group(1):
                seen[name.group(1)] = int(private.group(1))
    wide_models = [k for k in seen if "icm_sh_models_kernelILi" in k and "ELi32E" in k]
    wide_reward = [k for k in seen if "icm_sh_reward_kernelILi" in k and "ELi32E" in k]
    assert len(wide_models) == 3 and len(wide_reward) == 3, sorted(seen)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}


# ------------------------------------------------------------------------------------------------------- the policy
def _cpu_policy(NA, kind="d", update_mode="torch", policy=None, **icm_kw):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cpu")
    E, T, O = 4, 6, 10
    space = Discrete(NA) if kind == "d" else Box(-1.0, 1.0, (NA,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=41)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"p": (policy, sp, sp, space, dict(enable_icm=True, icm_kw_args=icm_kw))},
              device=dev, random_seed=6, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=8, epochs_per_iter=1, update_mode=update_mode, use_graphs=False)
    return ppo.policies["p"]


MARIO_KW = dict(encoded_obs_dim=9, encoder_hidden_size=128, inverse_hidden_size=32, forward_hidden_size=32)


@pytest.mark.parametrize("kind,NA", [("d", 18), ("c", 17)])
@pytest.mark.parametrize("icm_kw", [MARIO_KW, {}, dict(encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=64)],
                         ids=["mario", "default128", "identity"])
def test_the_opt_in_is_what_opens_the_gate(kind, NA, icm_kw):
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    pol = _cpu_policy(NA, kind, **icm_kw)
    assert FusedIcmUpdate.unsupported_reason(pol, 8) == REFUSAL.format(NA)
    assert FusedIcmUpdate.wide_actions_would_take(pol, 8) is True          # what `verbose` adds to the refusal
    pol.fused_wide_icm_actions = True
    assert FusedIcmUpdate.unsupported_reason(pol, 8) == ""
    assert FusedIcmUpdate.wide_actions_would_take(pol, 8) is False
    pol.fused_wide_icm_actions = False
    assert FusedIcmUpdate.unsupported_reason(pol, 8) == REFUSAL.format(NA)
    # what the flag cannot mend is not advertised
    wider = _cpu_policy(25 if kind == "d" else 30, kind, **icm_kw)
    assert FusedIcmUpdate.unsupported_reason(wider, 8) and FusedIcmUpdate.wide_actions_would_take(wider, 8) is False
    narrow = _cpu_policy(5, kind, **icm_kw)
    assert FusedIcmUpdate.unsupported_reason(narrow, 8) == "" and FusedIcmUpdate.wide_actions_would_take(narrow, 8) is False
