"""
CPU tests of the evaluation entry points at the C boundary (no GPU, no launch): header <-> SIGNATURES <-> library for
ppoaf_policy_infer / ppoaf_eval_scores_step, the argument-struct layouts (ctypes against the static_assert list in
csrc/policy_infer.hip), the ABI version, and the validation errors.
"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppoaf_hip.h")
SOURCE = os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "policy_infer.hip")
ENTRY_POINTS = ("ppoaf_policy_infer", "ppoaf_eval_scores_step")


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def test_header_signatures_and_library_agree(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = built.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/ppoaf_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = built.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args == 2
        assert hasattr(lib, name)
    assert lib.ppoaf_abi_version() == 7 and built.ABI_VERSION == 7
    assert "#define PPOAF_ABI_VERSION" not in src or re.search(r"#define\s+PPOAF_ABI_VERSION\s+7\b", src)


def test_entry_points_cite_the_reference_lines():
    src = open(HEADER).read()
    for needle in ("ppo_policy.py:796-889", "ppo.py:896-1028", "testing.py:59-112", "distributions.py:177-196",
                   ":404-436", ":580-581,611-631"):
        assert needle in src, needle
    for name in ENTRY_POINTS:
        pos = src.index(f"int {name}(")
        comment = src.rfind("/*", 0, pos)
        assert re.search(r"[\w/]+\.py:\d+", src[comment:pos]) or re.search(r"[\w/]+\.py:\d+", src[src.rfind("/* ---", 0, pos):pos])


@pytest.mark.parametrize("struct,ctype", [("ppoaf_policy_infer_args_t", "PolicyInferArgs"),
                                          ("ppoaf_eval_scores_args_t", "EvalScoresArgs")])
def test_struct_layout_matches_the_static_asserts(built, struct, ctype):
    text = open(SOURCE).read()
    cls = getattr(built, ctype)
    listed = re.findall(r"PPOAF_LAYOUT\(" + struct + r",\s*(\w+),\s*(\d+)\)", text)
    assert [f for f, _ in listed] == [f for f, _ in cls._fields_], "every field, in order"
    for field, off in listed:
        assert getattr(cls, field).offset == int(off), field
    size = re.search(r"static_assert\(sizeof\(" + struct + r"\)\s*==\s*(\d+)", text)
    assert size and C.sizeof(cls) == int(size.group(1))
    # and the header declares the fields in the same order
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)).group(1)
    names = [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\**\s+", "", decl.strip()).split(",")]
    assert names == [f for f, _ in cls._fields_]


def _desc(built, hidden=64, log_std=False, out_dim=3):
    pad4 = lambda x: (x + 3) // 4 * 4
    size = pad4(5 * hidden) + hidden + pad4(hidden * hidden) + hidden + pad4(out_dim * hidden) + pad4(out_dim)
    d = built.MlpDesc(in_dim=5, hidden=hidden, depth=2, out_dim=out_dim, activation=0, offset=0, size=size, log_std_offset=-1)
    if log_std:
        d.log_std_offset = size
        d.size = size + pad4(out_dim)
    return d


def _infer_args(built, **over):
    a = built.PolicyInferArgs()
    a.actor = _desc(built)
    a.params = a.obs = a.action_out = 0x10000           # never dereferenced: every case below is refused on the host
    a.E, a.head_kind, a.mode = 32, 0, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over,needle", [
    (dict(mode=2), "mode=2"), (dict(mode=-1), "mode=-1"), (dict(head_kind=4), "head_kind=4"), (dict(head_kind=-1), "head_kind"),
    (dict(params=None), "null pointer"), (dict(obs=None), "null pointer"), (dict(action_out=None), "null pointer"),
    (dict(E=-1), "negative E"), (dict(act_lo=0x10000), "both action bounds"),
    (dict(head_kind=1), "log_std"), (dict(head_kind=2, n_action_slices=0), "n_action_slices"),
    (dict(head_kind=2, n_action_slices=2), "action_slices"),
])
def test_policy_infer_refuses_on_the_host(built, over, needle):
    lib = built.load()
    a = _infer_args(built, **over)
    assert lib.ppoaf_policy_infer(C.byref(a), None) == -1
    assert needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error()


def test_policy_infer_refuses_shapes_outside_k6s(built):
    lib = built.load()
    a = _infer_args(built)
    a.actor = _desc(built, hidden=48)
    assert lib.ppoaf_policy_infer(C.byref(a), None) == -1 and "not instantiated" in lib.ppoaf_last_error().decode()
    a.actor = _desc(built, out_dim=9)
    assert lib.ppoaf_policy_infer(C.byref(a), None) == -1 and "out_dim" in lib.ppoaf_last_error().decode()
    assert lib.ppoaf_policy_infer(None, None) == -1 and "null args" in lib.ppoaf_last_error().decode()
    a = _infer_args(built, E=0)                          # nothing to do: accepted without a launch
    assert lib.ppoaf_policy_infer(C.byref(a), None) == 0


def test_eval_scores_step_refuses_on_the_host(built):
    lib = built.load()
    fields = [f for f, _ in built.EvalScoresArgs._fields_ if f != "E"]
    for missing in fields:
        a = built.EvalScoresArgs()
        for f in fields:
            setattr(a, f, None if f == missing else 0x10000)
        a.E = 8
        assert lib.ppoaf_eval_scores_step(C.byref(a), None) == -1, missing
        assert "null pointer" in lib.ppoaf_last_error().decode()
    a = built.EvalScoresArgs()
    a.E = -3
    assert lib.ppoaf_eval_scores_step(C.byref(a), None) == -1 and "E=-3" in lib.ppoaf_last_error().decode()
    assert lib.ppoaf_eval_scores_step(None, None) == -1


def test_wrappers_refuse_host_tensors(built):
    import torch
    from ppo_and_friends_amd import kernels as K
    a = built.EvalScoresArgs()
    a.E = 4
    with pytest.raises(built.PpoafError):
        K.eval_scores_step(a, torch.zeros(4), torch.zeros(4, dtype=torch.bool))
    with pytest.raises(built.PpoafError, match="float32"):
        K.eval_scores_step(a, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.bool))
