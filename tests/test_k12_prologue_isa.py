"""What K12's two C2 kernels do before their first useful loads go out, asserted on the compiled instruction stream
(tools/prologue_isa.py; no GPU: hipcc cross-compiles).  Each translation unit is compiled once per module.

Bounds (the issue's): the fused tail executes no `s_waitcnt vmcnt` ahead of the first operand load of a tile job
(parent: 3 -- `seq`, `step_counts`, and one where the operand requests wait for the optimiser state); fwd_bwd <8,8,true>
executes at most 2 `s_waitcnt lgkmcnt(0)` ahead of its first vector-memory instruction (parent: 9 in the text, 6 on the
shortest path), and in the per-epoch-tables flavour of the row-tile body no `vmcnt(N)` between the first hidden-set load
and the S0 barrier has N below the number of set loads issued (parent: `vmcnt(0)` right behind the index load).

This commit: tail 0 and 0; fwd_bwd 2 scalar waits (the argument batch, then the cursor's trip); 16 set loads in flight at
S0, the waits behind them vmcnt(16), (17), (18).
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prologue_isa as isa  # noqa: E402

pytestmark = pytest.mark.skipif(not isa.have_hipcc(), reason="hipcc not installed")


@pytest.fixture(scope="module")
def tail_asm(tmp_path_factory):
    return isa.compile_unit("ppo_update_tail.hip", str(tmp_path_factory.mktemp("isa_tail")))


@pytest.fixture(scope="module")
def fwd_bwd_asm(tmp_path_factory):
    return isa.compile_unit("ppo_update.hip", str(tmp_path_factory.mktemp("isa_fwd_bwd")))


@pytest.mark.parametrize("kernel", ["wgrad_adam_kernel<128,128,false>", "wgrad_adam_kernel<128,128,true>"])
def test_tail_requests_operands_before_any_vector_wait(tail_asm, kernel):
    ins = isa.kernel_text(tail_asm, kernel)
    n, waits = isa.tail_waits_before_operands(ins)
    print(kernel, "vmcnt waits before the first operand load:", n, waits)
    assert n == 0, waits


def test_fwd_bwd_scalar_waits_before_first_vector_memory_instruction(fwd_bwd_asm):
    ins = isa.kernel_text(fwd_bwd_asm, "fwd_bwd_kernel<8,8,true>")
    n, waits = isa.scalar_waits_before_vmem(ins)
    print("s_waitcnt lgkmcnt(0) before the first vector-memory instruction:", n)
    assert n <= 2, waits


def test_fwd_bwd_no_wait_for_a_hidden_set_before_s0(fwd_bwd_asm):
    r = isa.fwd_bwd_report(isa.kernel_text(fwd_bwd_asm, "fwd_bwd_kernel<8,8,true>"))
    print("bodies", r["bodies"], "set loads at S0", r["set_loads_at_barrier"], "waits behind the first set load",
          r["waits_after_first_set"])
    assert r["bodies"] == 2                                  # actor and critic
    assert r["set_loads_at_barrier"] == [16]                  # W_1 and W_2 of this wave's tile, all in flight at S0
    assert r["waits_after_first_set"], "the row lanes and the bias copy wait for SOMETHING before S0"
    assert r["draining"] == [], r["draining"]
