"""
CPU tests of K21's entry points at the C boundary (no GPU, no launch): header <-> SIGNATURES <-> library for
ppoaf_lstm_policy_step / ppoaf_lstm_policy_step_check, the argument-struct layout (ctypes against the static_assert list
in csrc/lstm_policy_step.hip), the ABI version, and the validation errors of the host-only check.
"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppoaf_hip.h")
SOURCE = os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "lstm_policy_step.hip")
ENTRY_POINTS = {"ppoaf_lstm_policy_step": 2, "ppoaf_lstm_policy_step_check": 1}
STEP, CRITIC_NEXT, INFER, MASK = 0, 1, 2, 3
PTR = 0x10000                                        # never dereferenced: nothing here launches


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def test_header_signatures_and_library_agree(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = built.load()
    for name, want in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/ppoaf_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = built.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args == want
        assert hasattr(lib, name)
    assert lib.ppoaf_abi_version() == 7 and built.ABI_VERSION == 7
    for k, v in (("STEP", STEP), ("CRITIC_NEXT", CRITIC_NEXT), ("INFER", INFER), ("MASK", MASK)):
        assert re.search(r"#define\s+PPOAF_LSTM_" + k + r"\s+" + str(v) + r"\b", src), k
    from ppo_and_friends_amd import kernels as K
    assert (K.LSTM_STEP, K.LSTM_CRITIC_NEXT, K.LSTM_INFER, K.LSTM_MASK) == (STEP, CRITIC_NEXT, INFER, MASK)


def test_entry_points_cite_the_reference_lines():
    src = open(HEADER).read()
    pos = src.index("int ppoaf_lstm_policy_step(")
    block = src[src.rfind("/* ---", 0, pos):pos]
    for needle in ("ppo_policy.py:729-794", "ppo_policy.py:593-627", "ppo.py:1863-1881", "networks/ppo_networks/lstm.py:103-127"):
        assert needle in block, needle


def test_struct_layout_matches_the_static_asserts(built):
    struct, cls = "ppoaf_lstm_policy_step_args_t", built.LstmPolicyStepArgs
    text = open(SOURCE).read()
    listed = re.findall(r"PPOAF_LAYOUT\(" + struct + r",\s*(\w+),\s*(\d+)\)", text)
    fields = [f for f, _ in cls._fields_]
    # `actor, critic` share one declaration and one static_assert each
    assert [f for f, _ in listed] == fields, "every field, in order"
    for field, off in listed:
        assert getattr(cls, field).offset == int(off), field
    size = re.search(r"static_assert\(sizeof\(" + struct + r"\)\s*==\s*(\d+)", text)
    assert size and C.sizeof(cls) == int(size.group(1))
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)).group(1)
    names = [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\**\s+", "", decl.strip()).split(",")]
    assert names == fields


def _desc(built, hidden=64, ff=32, depth=1, in_dim=5, out_dim=3):
    return built.LstmDesc(in_dim=in_dim, hidden=hidden, ff_hidden=ff, ff_depth=depth, out_dim=out_dim, activation=0,
                          rows=32, steps=1, params=PTR)


STEP_OUTPUTS = ("raw_action_out", "action_out", "logp_out", "value_out", "actor_hidden_out", "actor_cell_out",
                "critic_hidden_out", "critic_cell_out")


def _args(built, mode=STEP, **over):
    a = built.LstmPolicyStepArgs()
    a.actor, a.critic = _desc(built), _desc(built, ff=16, depth=2, in_dim=9, out_dim=1)
    a.E, a.head_kind, a.mode, a.infer_mode = 32, 0, mode, 1
    for f in ("obs", "critic_obs", "actor_h", "actor_c", "critic_h", "critic_c", "commit", "boot_value_out") + STEP_OUTPUTS:
        setattr(a, f, PTR)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _refused(built, a, needle):
    lib = built.load()
    assert lib.ppoaf_lstm_policy_step_check(None if a is None else C.byref(a)) != 0
    msg = lib.ppoaf_last_error().decode()
    assert needle in msg, msg
    # the launching entry point runs the same check first
    assert lib.ppoaf_lstm_policy_step(None if a is None else C.byref(a), None) != 0
    assert needle in lib.ppoaf_last_error().decode()


@pytest.mark.parametrize("mode", [STEP, CRITIC_NEXT, INFER, MASK])
def test_a_covered_descriptor_is_accepted(built, mode):
    a = _args(built, mode, terminated=PTR)
    assert built.load().ppoaf_lstm_policy_step_check(C.byref(a)) == 0, built.load().ppoaf_last_error()
    for hidden in (32, 64, 128):                         # ff width and depth may differ between the networks
        a.actor, a.critic = _desc(built, hidden=hidden, ff=128, depth=2), _desc(built, hidden=hidden, ff=16, out_dim=1)
        assert built.load().ppoaf_lstm_policy_step_check(C.byref(a)) == 0, built.load().ppoaf_last_error()


def test_null_args(built):
    _refused(built, None, "null args")


def test_shapes_outside_the_coverage(built):
    a = _args(built)
    a.critic = _desc(built, hidden=128, out_dim=1)
    _refused(built, a, "hidden sizes differ (actor 64, critic 128)")
    a = _args(built)
    a.actor = a.critic = _desc(built, hidden=48)
    _refused(built, a, "hidden 48")
    a = _args(built)
    a.actor = _desc(built, out_dim=9)
    _refused(built, a, "out_dim 9")
    a = _args(built)
    a.critic = _desc(built, out_dim=2)
    _refused(built, a, "critic out_dim must be 1")
    a = _args(built)
    a.actor = _desc(built, in_dim=257)
    _refused(built, a, "in_dim 257")


@pytest.mark.parametrize("mode", [4, -1])
def test_unknown_mode(built, mode):
    _refused(built, _args(built, mode), f"mode={mode}")


@pytest.mark.parametrize("missing", STEP_OUTPUTS)
def test_a_step_without_its_output_rows(built, missing):
    _refused(built, _args(built, STEP, **{missing: None}), "STEP needs the row-t outputs")


@pytest.mark.parametrize("mode,over,needle", [
    (STEP, dict(actor_h=None), "STEP: null observation / state pointer"),
    (STEP, dict(critic_obs=None), "STEP: null observation / state pointer"),
    (STEP, dict(head_kind=2), "head_kind=2"),
    (STEP, dict(head_kind=1), "log_std"),
    (STEP, dict(act_lo=PTR), "both action bounds"),
    (STEP, dict(normalize_values=1), "normaliser state missing"),
    (STEP, dict(E=-1), "negative E"),
    (CRITIC_NEXT, dict(commit=None), "CRITIC_NEXT"),
    (CRITIC_NEXT, dict(boot_value_out=None), "CRITIC_NEXT"),
    (CRITIC_NEXT, dict(terminated=PTR, critic_cell_out=None), "terminated given without"),
    (INFER, dict(action_out=None), "INFER"),
    (INFER, dict(infer_mode=2), "infer_mode=2"),
    (MASK, dict(), "MASK needs terminated"),
])
def test_refusals_of_each_mode(built, mode, over, needle):
    _refused(built, _args(built, mode, **over), needle)


def test_no_rows_is_accepted_and_launches_nothing(built):
    lib = built.load()
    for mode in (STEP, CRITIC_NEXT, INFER):
        a = _args(built, mode, E=0)
        assert lib.ppoaf_lstm_policy_step_check(C.byref(a)) == 0
        assert lib.ppoaf_lstm_policy_step(C.byref(a), None) == 0      # (there is no device here: a launch would fail)


def test_wrappers_refuse_host_tensors(built):
    import torch
    from ppo_and_friends_amd import kernels as K
    a = _args(built, E=4)
    z = torch.zeros(4, 64)
    with pytest.raises(built.PpoafError, match="device tensor"):
        K.lstm_critic_next(a, torch.zeros(4, 9), (z, z), torch.zeros(4), torch.zeros(1, dtype=torch.bool))
    with pytest.raises(built.PpoafError, match="device tensor"):
        K.lstm_policy_infer(a, torch.zeros(4, 5), (z, z), torch.zeros(4, dtype=torch.int64), True)
