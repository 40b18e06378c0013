"""
-m gpu: the evaluation kernels (csrc/policy_infer.hip) on their own, each against something other than themselves:
  * K19 in sample mode against K6 (ppoaf_policy_step): the same action, bit for bit, for equal (obs, params, seed, offset);
  * K19 in deterministic mode against the float64 forward on the CPU (tests/helpers/eval_kernels.py) -- the Gaussian head
    by the bound rule tests/test_gpu_k12_gradients.py states for K12, the discrete heads by their argmax with the
    near-tie rule below --, against planted exact ties, and against the `*_refined` arrays fixture g16 recorded from the
    reference's distribution classes;
  * ppoaf_eval_scores_step against the numpy restatement (tests/helpers/eval_restatement.py), bit for bit;
  * K6's own Categorical and Gaussian draws (cat_step_row / gauss_step_row of csrc/action_heads.hpp, which K21 and K19's
    sample mode share) against the restated heads of tests/helpers/head_draws.py (on the Philox of tests/helpers/philox.py)
    fed with the float64 forward (section 9).
    Measured on the MI355X, worst deviation / bound: Categorical, no row left out in any of the four cases, logp <= 0.007,
    value <= 0.011; Gaussian (out_dim 1, 4, 5, 6, with and without bounds) raw <= 0.024, action <= 0.027, logp <= 0.100,
    value <= 0.013 -- the device's logf and sincosf stay well inside the rule at these arguments.

Near-tie rule (discrete heads): a logit's bound is 1e-5 |z| + 1e-5 max|z| over the case's float64 logits, so two logits
are told apart when their float64 gap is at least the sum of their bounds (at most 4e-5 max|z|).  A row may be left out
of the comparison only when the top two logits of it (of one of its slices; a bit: |z| against its own bound) are closer
than that; the share of rows left out is asserted to stay <= 0.5 %.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_draws as hd  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE, GREEDY = 0, 1
BOUNDS3 = (np.array([-1.0, -2.0, 0.0], np.float32), np.array([1.0, 2.0, 5.0], np.float32))     # g12_gauss_bounds's


def _bounds(n):
    return tuple(np.resize(b, n) for b in BOUNDS3)


def _obs(seed, E, O, dev="cuda"):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((E, O)).astype(np.float32)).to(dev)


def _head_args(head, rng_int):
    """(out_dim, slices) for a head from one fuzz integer."""
    if head == "multi_categorical":
        nvec, k = [], rng_int
        while sum(nvec) < 8 and len(nvec) < 8:
            n = 1 + k % 4
            k //= 4
            if sum(nvec) + n > 8:
                break
            nvec.append(n)
        nvec = nvec or [2]
        return sum(nvec), tuple(nvec)
    return 1 + rng_int % 8, ()


# ---------------------------------------------------------------------------------------------- 5: sampled mode is K6
WIDTHS = [(32, 32), (64, 64), (128, 128), (256, 256), (128, 256), (64, 128)]


@pytest.mark.parametrize("head", ["categorical", "gaussian", "multi_categorical", "bernoulli"])
@pytest.mark.parametrize("widths", WIDTHS)
def test_sampled_action_is_k6s(head, widths):
    from eval_kernels import Policy
    for i, (E, O, depth) in enumerate(((1, 4, 3), (16, 17, 1), (37, 70, 2), (4096 + 5, 18, 3))):
        out_dim, slices = _head_args(head, 977 * (i + 1) + widths[0])
        bounds = _bounds(out_dim) if head == "gaussian" and i % 2 else None
        pol = Policy(100 + i, O, widths[0], depth, out_dim, head, act=("relu", "tanh", "leaky_relu")[i % 3], slices=slices,
                     bounds=bounds, critic_hidden=widths[1])
        obs = _obs(i, E, O)
        seed, offset = 0x1234ABCD5678 + i, 1000003 * i
        want = pol.step_k6(obs, seed, offset)
        got = pol.infer(obs, SAMPLE, seed, offset)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want), (head, widths, E, O, depth)
        if E >= 37:          # another offset draws other actions (the comparison above is not one of two constants)
            assert not torch.equal(pol.infer(obs, SAMPLE, seed, offset + 7919), want)


def test_sampled_action_is_k6s_fuzz():
    """Derandomised fuzz of (E, in_dim, depth, out_dim / slices, bounds, width, activation, head)."""
    from hypothesis import HealthCheck, given, settings, strategies as st
    from eval_kernels import Policy

    @settings(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(head=st.sampled_from(["categorical", "gaussian", "multi_categorical", "bernoulli"]),
           E=st.one_of(st.integers(1, 50), st.sampled_from([1, 15, 16, 17, 255, 257, 1000])), O=st.integers(1, 130),
           depth=st.integers(1, 4), k=st.integers(0, 10 ** 6), hidden=st.sampled_from([32, 64, 128, 256]),
           act=st.sampled_from(["relu", "leaky_relu", "tanh"]), bounded=st.booleans(), seed=st.integers(0, 2 ** 40))
    def run(head, E, O, depth, k, hidden, act, bounded, seed):
        out_dim, slices = _head_args(head, k)
        pol = Policy(k, O, hidden, depth, out_dim, head, act=act, slices=slices,
                     bounds=_bounds(out_dim) if head == "gaussian" and bounded else None)
        obs = _obs(k + 1, E, O)
        assert torch.equal(pol.infer(obs, SAMPLE, seed, k), pol.step_k6(obs, seed, k)), (head, E, O, depth, hidden)

    run()


# ------------------------------------------------------------------------------------------ 6: deterministic Gaussian
GAUSS_CASES = {
    "c2_unit": dict(O=4, hidden=128, depth=3, D=2, act="relu", bounded=False),
    "c3_bounds": dict(O=17, hidden=256, depth=3, D=6, act="tanh", bounded=True),
    "wide_in_bounds": dict(O=376, hidden=64, depth=2, D=8, act="leaky_relu", bounded=True),
    "small_unit": dict(O=7, hidden=32, depth=2, D=3, act="relu", bounded=False),
    "one_dim_bounds": dict(O=18, hidden=128, depth=1, D=1, act="tanh", bounded=True),
}


@pytest.mark.parametrize("case", sorted(GAUSS_CASES))
def test_deterministic_gaussian_against_float64(case):
    from eval_kernels import Policy, k12_bound
    c = GAUSS_CASES[case]
    E = 1000 + 3
    pol = Policy(11, c["O"], c["hidden"], c["depth"], c["D"], "gaussian", act=c["act"],
                 bounds=_bounds(c["D"]) if c["bounded"] else None)
    obs = _obs(5, E, c["O"])
    x = obs.cpu().numpy()
    # means steered to |mean| up to 4
    W, b = pol.actor.layers[-1]
    g = 4.0 / np.abs(pol.actor.forward(x)).max()
    pol.actor.layers[-1] = ((W * g).astype(np.float32), (b * g).astype(np.float32))
    pol.set_actor()

    def restate(dt):
        a = np.tanh(pol.actor.forward(x.astype(dt), dt))
        if c["bounded"]:
            lo, hi = (v.astype(dt) for v in _bounds(c["D"]))
            a = ((a + dt(1.0)) / dt(2.0)) * (hi - lo) + lo
        return a

    a64, a32 = restate(np.float64), restate(np.float32)
    assert 3.9 < np.abs(pol.actor.forward(x)).max() <= 4.1
    got = pol.infer(obs, GREEDY).cpu().numpy().astype(np.float64)
    frac = np.abs(got - a64) / k12_bound(a64, a32)
    print(f"\n{case}: worst deviation / bound = {frac.max():.3f}")
    assert np.isfinite(got).all() and frac.max() <= 1.0, (case, frac.max())


# ------------------------------------------------------------------------------------- 7: deterministic discrete heads
SHAPES = {"c2": (4, 128, 3, 2), "c4": (18, 128, 3, 5), "c3w": (17, 256, 3, 8), "wide_in": (376, 64, 2, 6)}
SLICES = {2: (2,), 5: (3, 2), 8: (2, 2, 2, 2), 6: (1, 2, 3)}


@pytest.mark.parametrize("gain", [0.01, 1.0])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("head", ["categorical", "multi_categorical", "bernoulli"])
def test_deterministic_discrete_against_float64(head, shape, gain):
    from eval_kernels import Policy
    O, hidden, depth, out_dim = SHAPES[shape]
    E = 4096
    slices = SLICES[out_dim] if head == "multi_categorical" else ()
    pol = Policy(21, O, hidden, depth, out_dim, head, act="relu", slices=slices, out_gain=gain)
    obs = _obs(9, E, O)
    want, near = hd.greedy(head, pol.actor.forward(obs.cpu().numpy()), slices)
    got = pol.infer(obs, GREEDY).cpu().numpy()
    share = near.mean()
    print(f"\n{head} {shape} gain {gain}: {near.sum()} of {E} rows near a tie ({100 * share:.3f} %)")
    assert share <= 0.005
    np.testing.assert_array_equal(got[~near], want[~near])


@pytest.mark.parametrize("head", ["categorical", "multi_categorical"])
def test_exact_ties_give_the_lowest_index(head):
    from eval_kernels import Policy
    slices = (3, 2, 3) if head == "multi_categorical" else ()
    pol = Policy(3, 9, 64, 2, 8, head, slices=slices)
    obs = _obs(2, 50, 9)
    W, b = pol.actor.layers[-1]
    # every output equal: rows and biases copied from output 0
    pol.actor.layers[-1] = (np.repeat(W[:1], 8, 0), np.repeat(b[:1], 8))
    pol.set_actor()
    got = pol.infer(obs, GREEDY).cpu().numpy()
    assert (got == 0).all()
    # outputs 1 and 2 (and 6 and 7) tie above the rest: far below, outputs 0, 3, 4, 5
    W2, b2 = np.repeat(W[:1], 8, 0), np.repeat(b[:1], 8).copy()
    b2[[0, 3, 4, 5]] -= 100.0
    pol.actor.layers[-1] = (W2, b2)
    pol.set_actor()
    got = pol.infer(obs, GREEDY).cpu().numpy()
    if head == "categorical":
        assert (got == 1).all()
    else:
        # slices [0,3) -> class 1; [3,5): outputs 3, 4 tie (both lowered) -> class 0; [5,8): 5 lowered, 6 and 7 tie -> 1
        np.testing.assert_array_equal(got, np.tile([1, 0, 1], (50, 1)))


@pytest.mark.parametrize("tag", ["md34", "md2222", "md13", "mb1", "mb4", "mb8"])
def test_greedy_action_of_given_logits_is_the_reference_refinement(golden, tag):
    """Output weights zeroed, bias = a row of g16's logits (saturated rows included): K19's greedy action is that row of
    `*_refined`, which the fixture recorded from the reference's distribution classes."""
    from eval_kernels import Policy
    g = golden("g16_action_heads")
    logits, refined = g[f"{tag}_logits"], g[f"{tag}_refined"]
    md = tag.startswith("md")
    slices = tuple(int(n) for n in g[f"{tag}_nvec"]) if md else ()
    pol = Policy(4, 6, 32, 1, logits.shape[1], "multi_categorical" if md else "bernoulli", slices=slices)
    obs = _obs(3, 19, 6)
    W, _ = pol.actor.layers[-1]
    for r in range(logits.shape[0]):
        pol.actor.layers[-1] = (np.zeros_like(W), logits[r].astype(np.float32))
        pol.set_actor()
        got = pol.infer(obs, GREEDY).cpu().numpy()
        np.testing.assert_array_equal(got, np.tile(refined[r], (19, 1)), err_msg=f"{tag} row {r}")


def test_validation_refuses_before_any_launch():
    from eval_kernels import Policy
    from ppo_and_friends_amd import _lib, kernels as K
    pol = Policy(1, 5, 64, 2, 3, "categorical")
    obs = _obs(1, 20, 5)
    a, out = pol.infer_args(obs, GREEDY)
    for field, value, needle in (("mode", 2, "mode"), ("head_kind", 9, "head_kind"), ("obs", None, "null pointer"),
                                 ("action_out", None, "null pointer")):
        b = _lib.PolicyInferArgs.from_buffer_copy(a)
        setattr(b, field, value)
        with pytest.raises(_lib.PpoafError, match=needle):
            K.policy_infer(b)
    torch.cuda.synchronize()
    assert (out == -7).all()                     # nothing was launched
    K.policy_infer(a)
    assert (out >= 0).all() and (out < 3).all()


# ------------------------------------------------------------------------------------------------ 8: the scores kernel
def _run_scores(score, done, quota):
    from ppo_and_friends_amd import kernels as K
    T, E = score.shape
    st = K.EvalScores(E, int(quota.sum()), "cuda", quota=torch.from_numpy(quota))
    ds, dd = torch.from_numpy(score).cuda(), torch.from_numpy(done).cuda()
    after = []
    for t in range(T):
        st.step(ds[t], dd[t])
        after.append(st.remaining_t.clone())
    res = st.results()
    res["remaining"] = st.remaining()
    res["remaining_after"] = torch.cat(after).cpu().numpy()
    res["run_score"], res["run_len"] = st.run_score.cpu().numpy(), st.run_len.cpu().numpy()
    return res


SCORE_CASES = {
    "n_not_multiple_of_e": dict(T=120, E=37, N=100, p=0.08),
    "n_below_e": dict(T=60, E=300, N=7, p=0.1),
    "all_finish_in_one_step": dict(T=9, E=64, N=128, p=None),
    "rows_that_never_finish": dict(T=50, E=40, N=80, p=0.1, never=(3, 17, 39)),
    "quota_zero_and_mixed": dict(T=80, E=20, N=None, p=0.15, quota=[0, 5, 1, 0, 2, 3, 0, 0, 9, 1] * 2),
    "one_row": dict(T=200, E=1, N=11, p=0.07),
    "wide": dict(T=30, E=5000, N=7001, p=0.2),
}


@pytest.mark.parametrize("case", sorted(SCORE_CASES))
def test_scores_kernel_is_the_restatement_bit_for_bit(case):
    import eval_restatement as R
    c = SCORE_CASES[case]
    rng = np.random.default_rng(len(case))
    T, E = c["T"], c["E"]
    score = (rng.standard_normal((T, E)) * 3.0).astype(np.float32)
    if c["p"] is None:
        done = np.zeros((T, E), bool)
        done[[3, 7]] = True
    else:
        done = rng.random((T, E)) < c["p"]
    for e in c.get("never", ()):
        done[:, e] = False
    quota = np.asarray(c["quota"], np.int32) if "quota" in c else R.quotas(c["N"], E)
    want = R.replay(score, done, quota)
    got = _run_scores(score, done, quota)
    for k in ("count", "steps", "run_len", "remaining_after"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("sum", "min", "max", "run_score"):
        assert got[k].tobytes() == want[k].tobytes(), k                # float64, bit for bit (inf included)
    assert got["remaining"] == want["remaining"]
    if "never" in c:
        assert got["remaining"] > 0


# ------------------------------------------------------------------- 9: K6's draws against the restated Philox block
def _k6(pol, obs, seed, offset):
    raw, act, logp, val = pol.step_k6(obs, seed, offset, full=True)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), act.cpu().numpy(), logp.double().cpu().numpy(), val.double().cpu().numpy()


def _judge(what, got, x64, x32, mask=None):
    from eval_kernels import k12_bound
    got, x64, x32 = (np.asarray(t, np.float64) for t in (got, x64, x32))
    if mask is not None:
        got, x64, x32 = got[mask], x64[mask], x32[mask]
    frac = (np.abs(got - x64) / k12_bound(x64, x32)).max()
    print(f"  {what}: worst deviation / bound = {frac:.3f}")
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)


@pytest.mark.parametrize("E", [15, 33])
@pytest.mark.parametrize("out_dim", [2, 8])
def test_k6_categorical_draw_against_the_restated_philox(out_dim, E):
    """Row e draws word x of Philox(seed, offset + e, stream 0); the action is the first k with u s < cum_k over the
    softmax of the float64 logits (s its sum), the log-prob log(clip(p_a / s, eps32, 1 - eps32)).  Near-tie rule: a
    logit's bound is 1e-5 |z| + 1e-5 max|z|; a row whose u s lies within 2 max_k bound + 1e-6 of a CDF edge is left out
    (at most 2 rows per case, asserted).  The counter's low word wraps inside the launch."""
    import philox
    from eval_kernels import Policy
    O = 18
    pol = Policy(40 + out_dim + E, O, 64, 2, out_dim, "categorical", act="tanh", out_gain=1.0, critic_hidden=64)
    obs = _obs(out_dim * 100 + E, E, O)
    x = obs.cpu().numpy()
    seed, offset = 0x1234ABCD5678 + E, 2 ** 32 - 7
    counters = philox.counters_u64(offset, np.arange(E))

    def restate(dt):
        z = pol.actor.forward(x.astype(dt), dt)
        a, gap, p, s = hd.categorical_draw(z, seed, counters, dt)
        return z, a, gap, p, s

    z64, a64, gap, p64, s64 = restate(np.float64)
    _, a32, _, p32, s32 = restate(np.float32)
    near = hd.near_cdf_edge(z64, gap)
    assert near.sum() <= 2, f"{near.sum()} rows of {E} near a CDF edge"
    raw, act, logp, val = _k6(pol, obs, seed, offset)
    print(f"\ncategorical out_dim {out_dim} E {E}: {near.sum()} rows left out, classes drawn {np.unique(act).tolist()}")
    assert np.array_equal(raw, act)
    assert np.array_equal(a32[~near], a64[~near]), "the float32 restatement decodes a kept row differently"
    np.testing.assert_array_equal(act[~near], a64[~near])
    assert len(np.unique(a64)) > 1
    _judge("logp", logp, hd.categorical_logp(p64, s64, a64, np.float64), hd.categorical_logp(p32, s32, a64, np.float32), ~near)
    _judge("value", val, pol.critic.forward(x)[:, 0], pol.critic.forward(x.astype(np.float32), np.float32)[:, 0])


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("out_dim", [1, 4, 5, 6])
def test_k6_gaussian_draw_against_the_restated_philox(out_dim, bounded):
    """raw = mean + sd z with z the Box-Muller pairs of the row's Philox blocks (seed, offset + e, q = d / 4), sd =
    max(softplus(log_std), min_std); action tanh(raw) (scaled to the bounds); the squashed Gaussian's log-prob.  raw,
    action, log-prob and value by the bound rule, in float64 with the float32 restatement as the floor; no row is left
    out (the map is continuous)."""
    import philox
    from eval_kernels import Policy
    O, E = 17, 33
    pol = Policy(60 + out_dim, O, 64, 2, out_dim, "gaussian", act="tanh", bounds=_bounds(out_dim) if bounded else None,
                 out_gain=1.0, critic_hidden=64)
    obs = _obs(7 + out_dim, E, O)
    x = obs.cpu().numpy()
    seed, offset = 0x1234ABCD5678 + out_dim, 2 ** 32 - 9 if bounded else 977 * out_dim
    counters = philox.counters_u64(offset, np.arange(E))

    def restate(dt):
        mean = pol.actor.forward(x.astype(dt), dt)
        sd = hd.gauss_std(pol.actor.log_std, pol.min_std, dt)
        raw = mean + sd * hd.gauss_normals(seed, counters, out_dim, dt)
        act, logp = hd.squashed_gaussian(mean, sd, raw, _bounds(out_dim) if bounded else None, dt)
        return raw, act, logp

    r64, r32 = restate(np.float64), restate(np.float32)
    assert r32[0].dtype == np.float32 and r32[2].dtype == np.float32
    raw, act, logp, val = _k6(pol, obs, seed, offset)
    print(f"\ngaussian out_dim {out_dim} bounded {bounded}: max |raw| {np.abs(r64[0]).max():.3g}")
    for what, got, x64, x32 in (("raw", raw, r64[0], r32[0]), ("action", act, r64[1], r32[1]), ("logp", logp, r64[2], r32[2])):
        _judge(what, got, x64, x32)
    _judge("value", val, pol.critic.forward(x)[:, 0], pol.critic.forward(x.astype(np.float32), np.float32)[:, 0])
