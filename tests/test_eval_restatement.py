"""
The evaluation's quota rule and score bookkeeping as restated in tests/helpers/eval_restatement.py (what the
ppoaf_eval_scores_step kernel and ppo_and_friends_amd/testing.py are held to on the GPU), pinned by hand-computed
cases and by the sequential loop of the reference's testing.py:59-112 written out beside it.  (The reference's own
testing.py does not import here -- it needs `moviepy` for its GIF writer -- so no fixture is recorded from it.)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import eval_restatement as R        # noqa: E402


@pytest.mark.parametrize("N", [0, 1, 5, 16, 17, 100, 4097])
@pytest.mark.parametrize("E", [1, 2, 7, 16, 4096])
def test_quotas_sum_to_n_and_differ_by_at_most_one(N, E):
    q = R.quotas(N, E)
    assert q.shape == (E,) and q.dtype == np.int32
    assert int(q.sum()) == N and int(q.max()) - int(q.min()) <= 1
    assert (np.diff(q) <= 0).all()                          # the first N % E rows owe the extra one
    assert q[0] == N // E + (1 if N % E else 0)


def test_hand_computed_trace():
    """Three rows, N = 4 -> quotas (2, 1, 1).
    row 0: scores 1, 2 | 3 | 4 ...: episodes (1 + 2) = 3 over 2 steps, then 3 over 1 step; its third episode is not owed.
    row 1: 0.5, 0.25, 0.125 done at t = 2 -> 0.875 over 3 steps; nothing after.
    row 2: never done inside the trace: running pair (-5, 5 steps), no result."""
    score = np.array([[1, 0.5, -1], [2, 0.25, -1], [3, 0.125, -1], [4, 9, -1], [5, 9, -1]], np.float32)
    done = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0], [1, 1, 0]], bool)
    r = R.replay(score, done, R.quotas(4, 3))
    np.testing.assert_array_equal(r["count"], [2, 1, 0])
    np.testing.assert_array_equal(r["sum"], [6.0, 0.875, 0.0])
    np.testing.assert_array_equal(r["min"], [3.0, 0.875, np.inf])
    np.testing.assert_array_equal(r["max"], [3.0, 0.875, -np.inf])
    np.testing.assert_array_equal(r["steps"], [3, 3, 0])
    np.testing.assert_array_equal(r["remaining_after"], [4, 3, 1, 1, 1])
    np.testing.assert_array_equal(r["run_score"], [0.0, 0.0, -5.0])
    np.testing.assert_array_equal(r["run_len"], [0, 0, 5])
    assert r["remaining"] == 1
    assert R.reduce_rows(r, 4) == (0.875, 3.0, 6.875 / 4, 6)


def test_one_row_is_the_reference_sequential_loop():
    """E = 1: row 0 owes all N episodes and the restatement is testing.py:59-112 -- the loop written out as the
    reference writes it (running total over all steps, per-episode min / max from +-max_int).  Scores are float32
    values of bounded dynamic range, for which float64 sums are exact in either association."""
    rng = np.random.default_rng(5)
    T, N = 400, 23
    score = np.round(rng.standard_normal(T) * 8.0, 3).astype(np.float32)
    done = rng.random(T) < 0.08
    done[-1] = True
    N = min(N, int(done.sum()))
    lo, hi, avg, steps = R.sequential_reference_loop(score, done, N)
    r = R.replay(score[:, None], done[:, None], R.quotas(N, 1))
    assert r["count"][0] == N and r["remaining"] == 0
    assert R.reduce_rows(r, N) == (lo, hi, avg, steps)
    info = R.score_info({"agent0": score[:, None]}, done[:, None], {"agent0": "p"}, N)
    assert info == {"num_test_runs": N, "total_time_steps": steps,
                    "agent0": {"low_score": lo, "high_score": hi, "avg_score": avg, "policy": "p"},
                    "p": {"low_score": lo, "high_score": hi, "avg_score": avg}}


def test_steps_after_remaining_is_zero_change_nothing():
    rng = np.random.default_rng(9)
    T, E, N = 300, 6, 20
    score = rng.standard_normal((T, E)).astype(np.float32)
    done = rng.random((T, E)) < 0.1
    full = R.replay(score, done, R.quotas(N, E))
    assert full["remaining"] == 0
    t_end = int(np.argmax(full["remaining_after"] == 0)) + 1
    assert t_end < T - 50
    cut = R.replay(score[:t_end], done[:t_end], R.quotas(N, E))
    for k in ("count", "sum", "min", "max", "steps", "run_score", "run_len"):
        assert cut[k].tobytes() == full[k].tobytes(), k
    # and the shortest-episode bias the quotas avoid: the first N finishers are shorter on average than the quota's
    order = sorted((t, e) for t in range(T) for e in range(E) if done[t, e])[:N]
    starts = {}
    lens = []
    for t, e in sorted((t, e) for t in range(T) for e in range(E) if done[t, e]):
        lens.append(((t, e), t - starts.get(e, -1)))
        starts[e] = t
    first_n = np.mean([l for k, l in lens if k in set(order)])
    assert first_n <= full["steps"].sum() / N


def test_reduction_to_policy_and_agent_scores():
    """Two agents of one policy and one agent of another, E = 2, N = 3 (quotas 2, 1); a policy's episode score is the sum
    of its agents' (testing.py:93-98), its low / high the extremes of those sums -- not of the agents' own extremes."""
    done = np.array([[0, 0], [1, 0], [0, 1], [1, 0], [0, 0]], bool)
    a0 = np.array([[1, 1], [1, 1], [5, 1], [5, 1], [0, 0]], np.float32)        # env 0: 2, 10 ; env 1: 3
    a1 = np.array([[4, 0], [4, 0], [-1, 0], [-1, 2], [0, 0]], np.float32)      # env 0: 8, -2 ; env 1: 0
    b0 = np.array([[0.5, 2], [0.5, 2], [0.5, 2], [0.5, 2], [7, 7]], np.float32)  # env 0: 1, 1 ; env 1: 6
    info = R.score_info({"a0": a0, "a1": a1, "b0": b0}, done, {"a0": "team", "a1": "team", "b0": "solo"}, 3)
    assert info["num_test_runs"] == 3 and info["total_time_steps"] == 2 + 2 + 3
    assert info["a0"] == {"low_score": 2.0, "high_score": 10.0, "avg_score": 5.0, "policy": "team"}
    assert info["a1"] == {"low_score": -2.0, "high_score": 8.0, "avg_score": 2.0, "policy": "team"}
    assert info["b0"] == {"low_score": 1.0, "high_score": 6.0, "avg_score": 8.0 / 3, "policy": "solo"}
    assert info["team"] == {"low_score": 3.0, "high_score": 10.0, "avg_score": 7.0}       # 10, 8 ; 3
    assert info["solo"] == {"low_score": 1.0, "high_score": 6.0, "avg_score": 8.0 / 3}
