"""The middle of K12's row-tile body on the compiled instruction stream (tools/prologue_isa.py; no GPU: hipcc
cross-compiles): what the hidden backward waits for carries nothing else.

In `fwd_bwd_kernel<8,8,true>` (the benchmark's kernel; per-epoch-tables flavour of the body, which marks the places with
comment lines, one set per network):
  * the head's row part -- everything up to d loss / d out in LDS -- stores nothing to global memory (the block's loss
    partials and the critic's values leave later, on waves that are not on the path);
  * the window from the barrier that ends the head phase to the barrier that releases the hidden backward holds no store
    to global memory and no `ds_bpermute` (dz_last on all eight waves, LDS to LDS), and no barrier of its own.
Parent commit: the head stored 8 partials and the critic's values and handed its row results over with four `ds_bpermute`
ahead of its barrier; the window stored dW_out, db_out and the log_std sums.
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
def report(tmp_path_factory):
    asm = isa.compile_unit("ppo_update.hip", str(tmp_path_factory.mktemp("isa_middle")))
    r = isa.middle_report(isa.kernel_text(asm, KERNEL))
    for name, m in r.items():
        print(name, {k: v for k, v in m.items()})
    return r


@pytest.mark.parametrize("part", ["head_rows", "middle"])
def test_marked_parts_are_found_whole(report, part):
    m = report[part]
    assert m["windows"] == 2                                  # actor and critic
    assert m["closed"], "a path leaves the marked part without passing its end marker"
    assert m["instructions"] > 0 and m["lds_writes"] > 0      # sDOut / dz_last are written inside


def test_head_row_part_stores_nothing_to_global_memory(report):
    assert report["head_rows"]["global_stores"] == []
    assert report["head_rows"]["barriers"] == 0


def test_window_before_the_hidden_backward_is_lds_only(report):
    m = report["middle"]
    assert m["global_stores"] == [], m["global_stores"]
    assert m["permutes"] == [], m["permutes"]
    assert m["barriers"] == 0
