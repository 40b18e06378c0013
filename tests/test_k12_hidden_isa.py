"""The hidden forward layers of K12's row-tile body on the compiled instruction stream (tools/prologue_isa.py; no GPU: hipcc
cross-compiles): where the two dgrad weight sets are requested.

In `fwd_bwd_kernel<8,8,true>` (the benchmark's kernel; per-epoch-tables flavour of the body, which marks the places with
comment lines, one set per network):
  * between a hidden forward layer's last MFMA and the LDS writes of its epilogue (the activations the next layer's barrier
    waits for) there is no vector-memory load: a wave issues in order, and 32 value-by-value loads per wave in front of the
    epilogue held the layer's barrier up (profiles/hidden_phase_stamps_C2.txt).  Parent commit: 32 per layer;
  * from the start of hidden layer 1 to the start of the hidden backward every wave asks for its two dgrad sets exactly
    once: 64 single-dword loads per network on its way -- nothing dropped, nothing doubled.  Three sets of waves ask at
    three places, so the text of a network holds 3 x 64, counted per phase.  (This kernel fetches the sets as
    `global_load_dword`, not through a buffer resource; the head's row part in between is left out of the count: its loads
    are no weight sets.);
  * the kernel uses no scratch memory.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prologue_isa as isa  # noqa: E402

pytestmark = pytest.mark.skipif(not isa.have_hipcc(), reason="hipcc not installed")

KERNEL = "fwd_bwd_kernel<8,8,true>"


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    asm = isa.compile_unit("ppo_update.hip", str(tmp_path_factory.mktemp("isa_hidden")))
    r = isa.hidden_report(isa.kernel_text(asm, KERNEL))
    for i, h in enumerate(r):
        print("network", i, h)
    return asm, r


def test_both_networks_and_both_layers_are_found(compiled):
    _, r = compiled
    assert len(r) == 2                                        # actor and critic
    for h in r:
        assert h["layers"] >= 1 and all(n > 0 for n in h["layer_mfmas"]), h


def test_no_vector_load_between_last_mfma_and_epilogue_writes(compiled):
    _, r = compiled
    for i, h in enumerate(r):
        assert all(not late for late in h["late_loads"]), (i, h["late_loads"])


def test_dgrad_sets_are_requested_exactly_once(compiled):
    """Per barrier-delimited phase [hidden layer 1, hidden layer 2, output layer, head, output backward].  The three request
    sites belong to disjoint sets of waves (the source's conditions on the wave number): wave 0 asks for W_2's set through
    the loop of layer 1 and for W_1's through the loop of layer 2, waves 4-7 for both ahead of the output layer, waves 1-3
    for both ahead of the head's barrier -- 64 loads on every wave's way, and no fourth site."""
    _, r = compiled
    for i, h in enumerate(r):
        assert h["dgrad_loads"] == [32, 32, 64, 64, 0], (i, h["dgrad_loads"])


def test_no_scratch(compiled):
    asm, _ = compiled
    assert isa.kernel_scratch_bytes(asm, KERNEL) == 0
