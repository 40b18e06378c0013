"""
CPU tests of K22's entry points at the C boundary (no GPU, no launch): header <-> SIGNATURES <-> library for the five
ppoaf_lstm_update_* symbols, the argument-struct layout (ctypes against the static_assert list in csrc/lstm_update.hip
and the header's field order) and the ABI version, which additive entry points leave alone.
"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppoaf_hip.h")
SOURCE = os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "lstm_update.hip")
ENTRY_POINTS = {"ppoaf_lstm_update_check": 2, "ppoaf_lstm_update_workspace_floats": 2, "ppoaf_lstm_update_fwd_bwd": 2,
                "ppoaf_lstm_update_wgrad": 2, "ppoaf_lstm_update_adam": 3}


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def test_the_five_symbols_are_declared_bound_and_exported(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = built.load()
    for name, want in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/ppoaf_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = built.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args == want, name
        assert hasattr(lib, name)
    from ppo_and_friends_amd import kernels as K
    for wrapper in ("lstm_update_refusal", "lstm_update_sizes", "lstm_update_fwd_bwd", "lstm_update_wgrad", "lstm_update_adam"):
        assert callable(getattr(K, wrapper))


def test_the_abi_version_stays_7(built):
    assert built.load().ppoaf_abi_version() == 7 and built.ABI_VERSION == 7
    assert re.search(r"#define\s+PPOAF_ABI_VERSION\s+7\b", open(HEADER).read())


def test_the_source_is_part_of_the_build():
    from ppo_and_friends_amd.csrc import build
    assert "lstm_update.hip" in build.sources()
    assert any(h.endswith("lstm_device.hpp") for h in build.headers())


def test_struct_layout_matches_the_header_and_the_static_asserts(built):
    struct, cls = "ppoaf_lstm_update_args_t", built.LstmUpdateArgs
    text = open(SOURCE).read()
    listed = re.findall(r"PPOAF_LAYOUT\(" + struct + r",\s*(\w+),\s*(\d+)\)", text)
    fields = [f for f, _ in cls._fields_]
    assert [f for f, _ in listed] == fields, "every field, in order"
    for field, off in listed:
        assert getattr(cls, field).offset == int(off), field
    size = re.search(r"static_assert\(sizeof\(" + struct + r"\)\s*==\s*(\d+)", text)
    assert size and C.sizeof(cls) == int(size.group(1))
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)).group(1)
    names = [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\**\s+", "", decl.strip()).split(",")]
    assert names == fields


def test_the_entry_points_cite_the_reference_lines():
    src = open(HEADER).read()
    pos = src.index("int ppoaf_lstm_update_check(")
    block = src[src.rfind("/* ---", 0, pos):pos]
    for needle in ("ppo.py:2292-2469", "ppo.py:2312-2319,2450-2466", "policies/ppo_policy.py:1037-1042"):
        assert needle in block, needle
