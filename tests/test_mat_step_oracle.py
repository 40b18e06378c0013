"""
CPU tests of the restated K16 rollout step (tests/helpers/mat_step_cases.py) that tests/test_gpu_mat_step_float64.py
compares the kernels with:

  * pinning: teacher-forced on its own actions, the step's log-probs and values are those of the float64 K15 mini-batch
    reference (oracle/mat_update_oracle.minibatch, itself pinned to fixture g12_c5_mat) for the same bucket; the draw is the
    inverse CDF of the probabilities it returns, from the Philox word the docstring names;
  * the conditions of every case, met by construction: the float32 restatement alone decodes every kept token as float64
    does, stays inside every bound, and the near ties stay within the cap; logits of O(1); the saturated case has forced
    tokens below float32's eps; the clamped forced entries are there;
  * sharpness: each planted error changes a kept action or pushes a tensor outside its bound in at least one case.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import k12_oracle as ko
from oracle import mat_update_oracle as mu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mat_step_cases as cases  # noqa: E402
import philox  # noqa: E402


# ---------------------------------------------------------------------------------------------------- pinning
@pytest.mark.parametrize("name", ["c5_3_18_5_21", "mask_16_33_8_3", "lds_1_32_8_17", "sat_3_18_5_16"])
def test_teacher_forced_step_is_the_minibatch_reference(name):
    s = cases.steering(name)
    A, O, NA, E = s.shape
    r = s.reference(torch.float64)                                          # (the values as the critic gives them)
    raw = cases.step_reference(s.params, A, O, NA, s.obs, s.seed, s.offset, forced=r["actions"])
    zeros = np.zeros((E, A), np.float32)
    mb = mu.Minibatch(s.obs, r["actions"], zeros, zeros + 1.0, zeros)
    m = mu.minibatch(s.params, A, O, NA, mb, ko.Consts(False, False, True, 10.0, 0.2, 0.01, 0.0, 0.01))
    np.testing.assert_allclose(raw["logp"], m["logp"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(raw["values"], m["values"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(raw["probs"] / raw["probs"].sum(-1, keepdims=True), m["probs"], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(raw["actions"], r["actions"])
    np.testing.assert_allclose(raw["logp"], r["logp"], rtol=1e-12, atol=1e-13)  # forcing the drawn actions changes nothing
    if s.vn is not None:
        np.testing.assert_allclose(r["values"], s.vn[0] + raw["values"] * np.sqrt(s.vn[1] + 1e-8), rtol=1e-12)


def test_the_draw_is_the_inverse_cdf_at_the_named_counter():
    """Token (e, i) of c5_3_18_5_21 from the probabilities the reference returns, the counter written out by hand (its low
    word wraps inside the launch: offset 2^32 - 5)."""
    s = cases.steering("c5_3_18_5_21")
    A, O, NA, E = s.shape
    assert s.offset == 2 ** 32 - 5
    for e, i in ((0, 0), (1, 2), (2, 0), (20, 2)):
        c = s.offset + e * A + i
        x = int(philox.philox4x32_10_words((c & 0xffffffff, c >> 32, 0, 0), (s.seed & 0xffffffff, s.seed >> 32))[0])
        u = (x >> 8) / 2.0 ** 24
        p = s.r64["probs"][e, i]
        k = int(np.searchsorted(np.cumsum(p), u * p.sum(), side="right"))
        assert s.r64["actions"][e, i] == min(k, NA - 1)
    assert (s.offset + 1 * A + 2) >> 32 == 1 and s.offset >> 32 == 0


# ---------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_meets_its_conditions_by_construction(name):
    s = cases.steering(name)
    c, (A, O, NA, E) = s.c, s.shape
    assert E <= 65 and s.obs.shape == (E, A, O)
    left = s.left_out()
    print(f"{name}: {left} of {E} envs with a near tie (cap {cases.cap(E)}), max|z| {np.abs(s.r64['logits']).max():.3g}, "
          f"float32 logits within {np.abs(s.r32['logits'] - s.r64['logits'])[s.kept].max() if s.kept.any() else 0.0:.3g}")
    assert left <= cases.cap(E), f"{left} envs of {E} with a near tie"
    assert left < E, "no env of the case is compared to its end"
    # the float32 restatement alone: every kept action float64's, every tensor inside its bound, both launches
    for forced in (False, True):
        wrong, fracs = cases.judge(s, s.f32 if forced else s.r32, forced)
        assert wrong == 0 and max(fracs.values()) <= 1.0, (forced, wrong, fracs)
        wrong, fracs = cases.judge(s, s.f64 if forced else s.r64, forced)
        assert wrong == 0 and max(fracs.values()) == 0.0
    # logits of O(1) and above: no distribution of the case is the uniform one of the default head gain
    if NA > 1:
        spread = s.r64["logits"].max(-1) - s.r64["logits"].min(-1)
        assert 0.3 < spread.mean() and np.abs(s.r64["logits"]).max() < (40.0 if c["saturate"] else 12.0), spread.mean()
        if E * A >= 12:
            assert len(np.unique(s.r64["actions"])) > 1
    else:
        assert not s.r64["actions"].any() and np.allclose(s.r64["logp"], np.log(1.0 - cases.EPS32), rtol=1e-12)
    # the forced launch: an entry at or above NA, one below 0 (more than one token), clamped by the reference
    f = s.forced
    assert f[-1, -1] >= NA and s.f64["actions"][-1, -1] == NA - 1
    assert f.size == 1 or (f[0, 0] < 0 and s.f64["actions"][0, 0] == 0)
    inside = (f >= 0) & (f < NA)
    assert np.array_equal(s.f64["actions"][inside], f[inside])
    if c["saturate"]:
        assert s.n_saturated >= 2
        assert np.allclose(s.f64["logp"][s.saturated], np.log(cases.EPS32), rtol=1e-12)
        assert np.array_equal(s.f32["logp"][s.saturated], s.f64["logp"][s.saturated].astype(np.float32).astype(np.float64)) or \
            np.allclose(s.f32["logp"][s.saturated], np.log(cases.EPS32), rtol=1e-6)
    else:
        assert s.r64["probs"].min() > 10 * cases.EPS32 or NA == 1
    assert (s.vn is not None) == c["norm_values"]


def test_the_cases_cover_what_the_gpu_test_needs():
    cs = cases.CASES
    assert sum(c["norm_values"] for c in cs.values()) >= 6 and sum(not c["norm_values"] for c in cs.values()) >= 6
    assert sum(1 for c in cs.values() if c["own_obs"] and c["own_obs"] != c["O"]) >= 2
    assert any((c["offset"] & 0xffffffff) + c["E"] * c["A"] > 2 ** 32 for c in cs.values())
    assert sum(1 for c in cs.values() if c["saturate"]) == 1
    per_tile = 16 // 3
    assert {c["E"] for c in cs.values() if (c["A"], c["O"], c["NA"]) == (3, 18, 5) and not c["saturate"]} == {per_tile - 1, per_tile, 4 * per_tile + 1}
    for shape in ((1, 1, 1, 1), (1, 32, 8, 17), (16, 33, 8, 3), (7, 64, 2, 5), (5, 65, 4, 7), (3, 97, 5, 11), (2, 128, 8, 9), (16, 128, 8, 2)):
        assert any((c["A"], c["O"], c["NA"], c["E"]) == shape for c in cs.values()), shape
    assert sum(1 for n in cs if n.startswith("draw")) == 6


# ---------------------------------------------------------------------------------------------------- sharpness
PLANTED = {
    "the one-hot shifted by one agent": dict(onehot_shift=True),
    "no start token": dict(no_start_token=True),
    "attn2 unmasked": dict(attn2_unmasked=True),
    "the counter as offset + slot E + env": dict(counter_slot_major=True),
    "the counter without the slot": dict(counter_no_slot=True),
    "Philox word y instead of x": dict(philox_word_y=True),
    "every agent's draw taken from pass 0's logits": dict(stale_logits=True),
    "values denormalised with var instead of sqrt(var + 1e-8)": dict(denorm_var=True),
    "the log-prob without the clamp": dict(logp_no_clamp=True),
}


def _caught(s, planted):
    """What of a planted float64 step the GPU test's rules refuse in this case ('' when they accept all of it)."""
    out = []
    for forced in (False, True):
        r = s.reference(torch.float64, forced=s.forced if forced else None, **planted)
        wrong, fracs = cases.judge(s, r, forced)
        tag = "forced" if forced else "sampled"
        out += [f"{tag}: {wrong} kept actions"] if wrong else []
        out += [f"{tag}: {k} {v:.3g} x bound" for k, v in fracs.items() if not v <= 1.0]
    return "; ".join(out)


@pytest.mark.parametrize("error", list(PLANTED))
def test_a_case_catches_every_planted_error(error):
    names = ["sat_3_18_5_16"] if "clamp" in error else list(cases.CASES)
    caught = {n: w for n in names for w in [_caught(cases.steering(n), PLANTED[error])] if w}
    print(f"{error}: caught by {len(caught)} of {len(names)} cases")
    for n, w in list(caught.items())[:4]:
        print(f"    {n}: {w}")
    assert caught, f"planted error accepted by every case: {error}"
