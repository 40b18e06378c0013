"""
-m gpu: the value normaliser's state after ONE mini-batch with hand-made per-rank records, on K12 (the row-tile body's
TABLES flavour: a 32-wide critic of depth 3, one 16-row tile), K15 (mat_update) and K22 (lstm_update), each at its test
suite's smallest shape.  The drivers are the package's own; only n_ranks and the record table of the launch's arguments
are replaced, so that one process reaches what otherwise takes three ranks: the row-tile body merges ranks beyond the two
records it requests ahead of its weight sets in a loop of its own (n_ranks > 2), which no single-GPU test reached.

n_ranks = 1, 2 and 3 over the same three records.  The second is EMPTY (n = 0) and carries values that would wreck the
result if it were merged; the means of the other two lie four orders of magnitude apart and their sums cancel, so merging
them in the other order gives another float32 mean (asserted below, on the CPU).

The state the launch writes to the other slot must equal, BITWISE for mean and variance and exactly for the count, a Chan
merge of the records in rank order followed by the reference's integrate (utils/stats.py:73-94) in the kernels' number
formats: records, merge and counts float64, batch mean / variance and the state float32.
oracle/running_stats_oracle.py has no merge of records -- it integrates one (mean, variance, n) batch -- and leaves the
mixed float32 / float64 products to numpy's promotion rules, which round `delta * (n / count)` in float32 where the kernels
round it in float64.  So `expected` below is the same arithmetic in numpy with every cast written out, and
test_expected_state_on_the_cpu (no GPU) holds it to exact arithmetic and to the oracle.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle.running_stats_oracle import RunningMeanStd

STATE = (0.3, 0.25, 5000.0)                                   # mean, variance (float32), count (float64) before the mini-batch
# (n, mean, M2) of ranks 0, 1, 2: the live records' sums cancel to 222 / 513037, the empty one would wreck everything
RECORDS = ((37.0, 513.0e9 + 6.0, 5.0e4), (0.0, 7.0e8, 3.0e30), (513000.0, -37.0e6, 0.75))
f32, f64 = np.float32, np.float64


def merged(records):
    """Chan merge in rank order, float64 -> (n, mean, M2)."""
    n, bm, M2 = f64(0.0), f64(0.0), f64(0.0)
    for nb, mean, m2 in np.asarray(records, dtype=f64):
        if nb <= 0.0:
            continue
        d, nn = mean - bm, n + nb
        bm = bm + d * (nb / nn)
        M2 = M2 + (m2 + d * d * n * nb / nn)
        n = nn
    return n, bm, M2


def expected(records, state=STATE):
    """-> (mean float32, variance float32, count float64)."""
    m, v, cnt = f32(state[0]), f32(state[1]), f64(state[2])
    n, bm, M2 = merged(records)
    if n > 0.0:
        batch_mean, batch_var = f32(bm), f32(M2 / n)
        delta = f32(batch_mean - m)
        new_count = cnt + n
        new_mean = f32(f64(m) + f64(delta) * (n / new_count))
        m_2 = f64(v) * cnt + f64(batch_var) * n + f64(f32(delta * delta)) * cnt * n / (cnt + n)
        m, v, cnt = new_mean, f32(m_2 / (cnt + n)), new_count
    return m, v, cnt


def test_expected_state_on_the_cpu():
    """What the GPU test compares against, held to exact arithmetic and to the oracle (no GPU): the merge gives the pooled
    moments of the live records (rationals; each merge step rounds a few times at the scale of the largest mean), the
    integrate step is the oracle's within float32 rounding (module docstring: fewer than eight roundings of positive terms,
    1e-6), the empty record changes nothing, and the order of the merge shows in the result."""
    for R in (1, 2, 3):
        live = [tuple(Fraction(x) for x in r) for r in RECORDS[:R] if r[0] > 0]
        N = sum(r[0] for r in live)
        mean = sum(r[0] * r[1] for r in live) / N
        M2 = sum(r[2] + r[0] * (r[1] - mean) ** 2 for r in live)
        n, bm, m2 = merged(RECORDS[:R])
        assert n == N
        assert abs(Fraction(float(bm)) - mean) <= 4 * Fraction(float(np.spacing(max(abs(r[1]) for r in RECORDS[:R] if r[0] > 0))))
        assert abs(Fraction(float(m2)) - M2) <= Fraction(1, 10 ** 12) * M2
        rs = RunningMeanStd()
        rs.mean, rs.variance, rs.count = f32(STATE[0]), f32(STATE[1]), STATE[2]
        rs.integrate(f32(bm), f32(m2 / n), float(n))
        m, v, cnt = expected(RECORDS[:R])
        assert abs(float(m) - float(rs.mean)) <= 1e-6 * abs(float(rs.mean))
        assert abs(float(v) - float(rs.variance)) <= 1e-6 * abs(float(rs.variance))
        assert cnt == rs.count == STATE[2] + float(n)
    assert [x.tobytes() for x in expected(RECORDS[:2])] == [x.tobytes() for x in expected(RECORDS[:1])]
    assert expected(RECORDS)[0].tobytes() != expected(RECORDS[::-1])[0].tobytes(), "the merge order does not show"


@functools.lru_cache(maxsize=None)
def _driver(kernel):
    """-> (the kernel's fused driver after a rollout, mini-batch size): the suites' own builders at their smallest shapes."""
    if kernel == "k12":
        from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
        import test_gpu_k12_gradients as t
        B = 16
        ppo = t._ppo(t.case(O=8, ha=32, depth=3, B=B))
        ppo.rollout()
        ppo.policies["p"].train()
        return FusedPolicyUpdate(ppo, "p"), B
    if kernel == "k15":
        import test_gpu_mat_update_float64 as t
        B = 2
        ppo = t._ppo(2, 3, 2, B)
        pid = "mat"
    else:
        import test_gpu_lstm_update_float64 as t
        c = t.cases.case()
        B = c["B"]
        ppo = t._ppo(c)
        pid = "p"
    ppo.rollout()
    ppo.policies[pid].train()
    return ppo._fused_updater(pid, B), B


@pytest.mark.gpu
@pytest.mark.parametrize("n_ranks", [1, 2, 3])
@pytest.mark.parametrize("kernel", ["k12", "k15", "k22"])
def test_state_after_one_minibatch(kernel, n_ranks):
    upd, B = _driver(kernel)
    dev = upd.pol.device
    g = torch.Generator().manual_seed(5)
    upd.begin_epoch(torch.randperm(len(upd.pol.dataset), generator=g).to(dev))
    args = upd._args_for(B)
    a = type(args).from_buffer_copy(args)
    assert a.normalize_values == 1 and a.n_ranks == 1 and int(upd.cursor.item()) == 0
    if kernel == "k12":
        assert upd.critic_desc.hidden == 32 and upd.critic_desc.depth == 3 and a.inputs_in_batch_order == 1    # the TABLES flavour
    # mini-batch 0 reads slot 0 and its n_ranks records, and writes slot 1
    rec = torch.tensor(RECORDS[:n_ranks], dtype=torch.float64, device=dev).contiguous()
    a.n_ranks, a.vn_records = n_ranks, rec.data_ptr()
    upd.vn_mean[0], upd.vn_var[0], upd.vn_count[0] = STATE
    upd.vn_mean[1], upd.vn_var[1], upd.vn_count[1] = float("nan"), float("nan"), float("nan")
    upd._one(a)
    torch.cuda.synchronize()
    why = upd._bounded_wait_failure()
    assert not why, why
    got = (upd.vn_mean[1].cpu().numpy(), upd.vn_var[1].cpu().numpy(), upd.vn_count[1].cpu().numpy())
    want = expected(RECORDS[:n_ranks])
    print(f"{kernel} n_ranks={n_ranks}: got {[float(x) for x in got]} want {[float(x) for x in want]}")
    assert (upd.vn_mean[0].item(), upd.vn_var[0].item(), upd.vn_count[0].item()) == (float(f32(STATE[0])), STATE[1], STATE[2])
    assert got[0].tobytes() == want[0].tobytes(), f"mean {got[0]!r}, expected {want[0]!r}"
    assert got[1].tobytes() == want[1].tobytes(), f"variance {got[1]!r}, expected {want[1]!r}"
    assert got[2] == want[2], f"count {got[2]!r}, expected {want[2]!r}"
