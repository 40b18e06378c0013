"""K12's lean fwd_bwd kernel (csrc/ppo_update_lean.hip) on the compiled instruction stream (tools/prologue_isa.py; no GPU:
hipcc cross-compiles).  The kernel is the row-tile body of `fwd_bwd_kernel<8,8,true>` compiled for one activation and one
head, per-epoch-tables flavour only; checked on `fwd_bwd_lean_kernel<8,8,0,0>` (128/128, ReLU, Categorical: the benchmark's):
  * no scratch memory, and no more vector registers than the general kernel in the same build;
  * what was decided at run time is gone from the text: no `v_exp_f32` (tanh) between a hidden forward layer's start and the
    end of its epilogue, a head row part of fewer than 1 000 instructions (no Gaussian / MultiDiscrete arm; the general
    kernel's is about 9 000 over both networks), and fewer than half the general kernel's instructions overall;
  * what tests/test_k12_prologue_isa.py, test_k12_middle_isa.py and test_k12_hidden_isa.py pin on the general kernel holds
    here, read with the same tool functions: at most 2 scalar waits ahead of the first vector-memory instruction; behind the
    first hidden-set load the prologue waits with vmcnt(16 / 17 / 18) only, never for a set; the head's row part and the
    window before the hidden backward are closed, store nothing to global memory, use no ds_(b)permute and no barrier; no
    vector load between a layer's last MFMA and its epilogue writes; the dgrad sets are requested at the 32 + 32 / 64 / 64
    sites, once per wave.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prologue_isa as isa  # noqa: E402

pytestmark = pytest.mark.skipif(not isa.have_hipcc(), reason="hipcc not installed")

LEAN = "fwd_bwd_lean_kernel<8,8,0,0>"                        # <HTA, HTC, PPOAF_ACT_RELU, PPOAF_HEAD_CATEGORICAL>
GENERAL = "fwd_bwd_kernel<8,8,true>"


@pytest.fixture(scope="module")
def lean(tmp_path_factory):
    assert isa.unit_of(LEAN) == "ppo_update_lean.hip" and isa.unit_of(GENERAL) == "ppo_update.hip"
    asm = isa.compile_unit(isa.unit_of(LEAN), str(tmp_path_factory.mktemp("isa_lean")))
    return asm, isa.kernel_text(asm, LEAN)


@pytest.fixture(scope="module")
def general(tmp_path_factory):
    asm = isa.compile_unit(isa.unit_of(GENERAL), str(tmp_path_factory.mktemp("isa_lean_general")))
    return asm, isa.kernel_text(asm, GENERAL)


def test_no_scratch_and_no_more_registers_than_the_general_kernel(lean, general):
    assert isa.kernel_resource(lean[0], LEAN, "ScratchSize") == 0
    v, vg = (isa.kernel_resource(a, k, "TotalNumVgprs") for a, k in ((lean[0], LEAN), (general[0], GENERAL)))
    print("vector registers: lean", v, "general", vg)
    assert v <= vg


def test_fewer_than_half_the_general_kernels_instructions(lean, general):
    n, ng = isa.instruction_count(lean[1]), isa.instruction_count(general[1])
    print("instructions: lean", n, "general", ng)
    assert 2 * n < ng


def test_hidden_forward_layers_hold_no_tanh(lean):
    layers = isa.marked_windows(lean[1], isa.MARK_LAYER)
    assert len(layers) == 4 and all(w["closed"] for w in layers)           # two layers per network
    for w in layers:
        assert any(op.startswith("v_mfma") for op, _ in w["ins"])
        assert not [op for op, _ in w["ins"] if op.startswith("v_exp_f32")]


def test_head_row_part_holds_one_head(lean):
    rows = isa.marked_windows(lean[1], isa.MARK_HEAD_ROWS)
    assert len(rows) == 2 and all(w["closed"] for w in rows)               # actor and critic
    print("head row part, instructions per network:", [len(w["ins"]) for w in rows])
    for w in rows:
        assert 0 < len(w["ins"]) < 1000


def test_prologue_as_the_general_kernels(lean):
    r = isa.fwd_bwd_report(lean[1])
    assert r["scalar_waits"] <= 2, r["scalar_wait_list"]
    assert r["bodies"] == 2 and r["set_loads_at_barrier"] == [16]
    assert r["waits_after_first_set"] and {n for n, _ in r["waits_after_first_set"]} <= {16, 17, 18}, r["waits_after_first_set"]
    assert r["draining"] == [], r["draining"]


def test_middle_as_the_general_kernels(lean):
    for part, m in isa.middle_report(lean[1]).items():
        assert m["windows"] == 2 and m["closed"], (part, m)
        assert m["instructions"] > 0 and m["lds_writes"] > 0, (part, m)
        assert m["global_stores"] == [] and m["barriers"] == 0, (part, m)
    assert isa.middle_report(lean[1])["middle"]["permutes"] == []


def test_hidden_layers_as_the_general_kernels(lean):
    r = isa.hidden_report(lean[1])
    assert len(r) == 2
    for i, h in enumerate(r):
        assert h["layers"] >= 1 and all(n > 0 for n in h["layer_mfmas"]), h
        assert all(not late for late in h["late_loads"]), (i, h["late_loads"])
        assert h["dgrad_loads"] == [32, 32, 64, 64, 0], (i, h["dgrad_loads"])
