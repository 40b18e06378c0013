"""
CPU tests of the restated K21 launch (tests/helpers/lstm_step_cases.py) that tests/test_gpu_lstm_step_float64.py compares
the kernels with:

  * pinning: with the forced action, the step's log-probs, the critic's own outputs and the states it leaves are those of
    the float64 K22 mini-batch reference (oracle/lstm_update_oracle.minibatch, itself pinned to the g12_lstm_* fixtures)
    for the same rows as windows of S = 1; three chained steps leave the (h, c) of one S = 3 forward; the draw is the
    inverse CDF of the probabilities the step returns, from the Philox word at the counter the docstring names;
  * the conditions of every case, met by construction: the near ties of the sampled, the greedy and the chain's third
    launch stay within the cap, the float32 restatement alone stays inside every bound of every launch, a Categorical
    case of twelve rows or more draws more than one class, the forced entries are there;
  * coverage: the shapes the GPU test needs are among the cases (E > 64, a second Philox block, a wrapping offset, ...);
  * sharpness: each planted error changes a kept action or pushes a tensor outside its bound in a named case.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import lstm_update_oracle as lo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_step_cases as cases  # noqa: E402
import philox  # noqa: E402

CAT, GAU = cases.CAT, cases.GAU


# ---------------------------------------------------------------------------------------------------- pinning
@pytest.mark.parametrize("name", ["e15_cat3", "e33_gau4_bounds", "small_h_cat3", "e129_h128_gau5_bounds", "e17_wrap_cat8"])
def test_forced_step_is_the_minibatch_reference_at_s1(name):
    s = cases.steering(name)
    E = s.c["E"]
    f64 = s.ref["forced"][0]
    zeros = np.zeros(E, np.float32)
    mb = lo.Minibatch(s.obs[0][:, None, :], s.cobs[0][:, None, :], np.zeros((E, 1), bool), *s.state, f64["actions"],
                      zeros, zeros + 1.0, zeros)
    m = lo.minibatch(s.params, s.actor, s.critic, s.head, mb, lo.Consts(False, False, True, 10.0, 0.2, 0.01, 0.0, cases.MIN_STD))
    np.testing.assert_allclose(f64["logp"], m["logp"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f64["values_raw"], m["values"], rtol=1e-12, atol=1e-13)
    for k in cases.STATES:
        np.testing.assert_allclose(f64[k], m[k], rtol=1e-12, atol=1e-14)
    if s.vn is not None:
        np.testing.assert_allclose(f64["values"], s.vn[0] + m["values"] * np.sqrt(s.vn[1] + 1e-8), rtol=1e-12)
    else:
        np.testing.assert_array_equal(f64["values"], f64["values_raw"])


@pytest.mark.parametrize("name", ["e16_gau1", "e17_wrap_cat8", "e65_in256_gau8_bounds"])
def test_three_chained_steps_are_one_window_of_three(name):
    s = cases.steering(name)
    chain = s.ref["chain"][0]
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    for tag, net, seg, x, (h0, c0) in (("actor", s.actor, s.params[:s.na], s.obs, s.state[:2]),
                                       ("critic", s.critic, s.params[s.na:], s.cobs, s.state[2:])):
        with torch.no_grad():
            out, h, c, _ = lo._Module(net, seg, torch.float64)(T(x).transpose(0, 1), T(h0), T(c0))
        np.testing.assert_allclose(chain[tag + "_h"], h.numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(chain[tag + "_c"], c.numpy(), rtol=1e-12, atol=1e-14)
        if tag == "actor":
            np.testing.assert_allclose(chain["logits"], out.numpy(), rtol=1e-12, atol=1e-13)
        else:
            np.testing.assert_allclose(chain["values_raw"], out.numpy()[:, 0], rtol=1e-12, atol=1e-13)


def test_the_draw_is_the_inverse_cdf_at_the_named_counter():
    """Rows of e17_wrap_cat8 from the probabilities the reference returns, the counter written out by hand (its low word
    wraps inside the launch: offset 2^32 - 5); the chain's third launch draws at offset + 2 E + e."""
    s = cases.steering("e17_wrap_cat8")
    E, O = s.c["E"], s.c["head"][1]
    assert s.offset == 2 ** 32 - 5
    for launch, base in (("sampled", s.offset), ("chain", s.offset + 2 * E)):
        r = s.ref[launch][0]
        for e in (0, 4, 5, 16):
            c = base + e
            x = int(philox.philox4x32_10_words((c & 0xffffffff, c >> 32, 0, 0), (s.seed & 0xffffffff, s.seed >> 32))[0])
            u = (x >> 8) / 2.0 ** 24
            p = r["probs"][e]
            k = int(np.searchsorted(np.cumsum(p), u * p.sum(), side="right"))
            assert r["actions"][e] == min(k, O - 1), (launch, e)
    assert (s.offset + 5) >> 32 == 1 and (s.offset + 4) >> 32 == 0


def test_the_gaussian_draw_is_the_box_muller_pair_at_the_named_counter():
    """Dimension d of row e of e33_gau5: block (seed, offset + e, stream d / 4), words (x, y) for d % 4 < 2 and (z, w)
    above, the cos output for an even d and the sin output for an odd one."""
    s = cases.steering("e33_gau5")
    r = s.ref["sampled"][0]
    at = lo.tensor_table(s.actor, True)[0][-1][1]
    sd = np.maximum(np.log1p(np.exp(s.params[at:at + 5])), cases.MIN_STD)
    for e, d in ((0, 0), (7, 1), (16, 2), (17, 3), (32, 4)):
        c = s.offset + e
        w = philox.philox4x32_10_words((c & 0xffffffff, c >> 32, d // 4, 0), (s.seed & 0xffffffff, s.seed >> 32))
        pair = (d % 4) // 2
        rad = np.sqrt(-2.0 * np.log(((int(w[2 * pair]) >> 8) + 1) / 2.0 ** 24))
        ang = 2.0 * np.pi * ((int(w[2 * pair + 1]) >> 8) / 2.0 ** 24)
        z = rad * (np.cos(ang) if d % 2 == 0 else np.sin(ang))
        np.testing.assert_allclose(r["raw"][e, d], r["logits"][e, d] + sd[d] * z, rtol=1e-12, atol=1e-13)


# ---------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_meets_its_conditions_by_construction(name):
    s = cases.steering(name)
    c, E, (head, O) = s.c, s.c["E"], s.c["head"]
    r64 = s.ref["sampled"][0]
    for launch in ("sampled", "greedy", "chain"):
        left = s.left_out(launch)
        print(f"{name} {launch}: {left} of {E} rows near a tie (cap {cases.cap(E)})")
        assert left <= cases.cap(E) and (left < E or E == 1), f"{launch}: {left} rows of {E} near a tie"
        assert E > 1 or left == 0
    # the float32 restatement alone: every kept action float64's, every tensor inside its bound, every launch
    for launch in cases.LAUNCHES:
        wrong, fracs = cases.judge(s, s.ref[launch][1], launch)
        assert wrong == 0 and max(fracs.values()) <= 1.0, (launch, wrong, fracs)
        wrong, fracs = cases.judge(s, s.ref[launch][0], launch)
        assert wrong == 0 and max(fracs.values()) == 0.0, (launch, wrong, fracs)
    z = r64["logits"]
    if head == CAT:
        spread = z.max(1) - z.min(1)
        assert np.abs(z).max() < (60.0 if c["saturate"] else 12.0)
        if E >= 12:                                           # (a mean over a row or two says nothing)
            assert 0.3 < spread.mean(), spread.mean()
            assert len(np.unique(r64["actions"])) > 1 and len(np.unique(r64["greedy"])) > 1
        # the forced launch: an entry at or above out_dim, one below 0 (more than one row), clamped by the reference
        f, f64 = s.forced, s.ref["forced"][0]
        assert f[-1] >= O and f64["actions"][-1] == O - 1
        assert E == 1 or (f[0] < 0 and f64["actions"][0] == 0)
        inside = (f >= 0) & (f < O)
        assert np.array_equal(f64["actions"][inside], f[inside])
        if c["saturate"]:
            assert s.saturated.sum() >= 2
            assert np.allclose(f64["logp"][s.saturated], np.log(cases.EPS32), rtol=1e-12)
            assert np.allclose(s.ref["forced"][1]["logp"][s.saturated], np.log(cases.EPS32), rtol=1e-6)
        else:
            assert r64["probs"].min() > 10 * cases.EPS32 and not s.saturated.any()
    else:
        k = max(1, E // 8)
        a = np.abs(s.forced[:k])
        assert (a >= 3.8 - 1e-6).all() and (a <= 4.2 + 1e-6).all()
        assert np.array_equal(s.ref["forced"][0]["raw"], s.forced.astype(np.float64))
        assert np.abs(z).max() < 12.0 and np.abs(r64["raw"]).max() > 0.5
    if c["small_h"]:
        assert min(r64["actor_h"].var(1).min(), r64["critic_h"].var(1).min()) < 1e-3   # the LayerNorm's eps matters
    assert (s.vn is not None) == c["norm_values"] and (s.bounds is not None) == c["bounds"]
    # terminated: row 0, the last live row, a row of tile >= 4 where there is one -- and not every row
    assert s.terminated[0] and s.terminated[E - 1] and (E <= 70 or s.terminated[64:].sum() >= 2)
    assert E <= 2 or not s.terminated.all()


def test_the_cases_cover_what_the_gpu_test_needs():
    cs = cases.CASES
    assert 16 <= len(cs) <= 24
    col = lambda k: {c[k] for c in cs.values()}
    assert col("E") == {1, 15, 16, 17, 33, 65, 129}
    assert col("H") == {32, 64, 128} and col("Fa") | col("Fc") == {16, 32, 64, 128}
    assert all(c["Fa"] != c["Fc"] for c in cs.values())
    assert col("Da") == col("Dc") == {1, 2} and any(c["Da"] != c["Dc"] for c in cs.values())
    assert col("Ia") | col("Ic") >= {1, 15, 16, 17, 255, 256}
    assert sum(c["Ia"] != c["Ic"] for c in cs.values()) > len(cs) // 2
    assert col("act") == {"relu", "leaky_relu", "tanh"}
    assert {c["head"][1] for c in cs.values() if c["head"][0] == CAT} >= {2, 3, 8}
    gau = [c for c in cs.values() if c["head"][0] == GAU]
    assert {c["head"][1] for c in gau} == {1, 4, 5, 8}
    assert {c["head"][1] >= 5 for c in gau if c["bounds"]} == {True, False} == {c["head"][1] >= 5 for c in gau if not c["bounds"]}
    assert sum(c["norm_values"] for c in cs.values()) >= 6 and sum(not c["norm_values"] for c in cs.values()) >= 6
    # E > 64: tile 4 alone in the second group (65), tile 8 in the third (129); at H = 128 or I = 256, both heads
    big = [c for c in cs.values() if c["E"] > 64]
    assert {c["E"] for c in big} == {65, 129} and all(c["H"] == 128 or 256 in (c["Ia"], c["Ic"]) for c in big)
    assert any(c["H"] == 128 for c in big) and any(c["Ia"] == 256 for c in big)
    assert {c["head"][0] for c in big} == {CAT, GAU}
    assert sum(c["small_h"] for c in cs.values()) == 1 and sum(bool(c["saturate"]) for c in cs.values()) == 1
    assert any(c["E"] >= 17 and c["offset"] == 2 ** 32 - 5 for c in cs.values())


# ---------------------------------------------------------------------------------------------------- sharpness
# error -> (the planted field, the case named to catch it)
PLANTED = {
    "the counter is offset + e + 1": ("counter_plus_one", "e15_cat3"),
    "the counter is the tile-local row": ("counter_tile_local", "e17_wrap_cat8"),
    "the Categorical draw from Philox stream 1": ("cat_stream_1", "e15_cat3"),
    "the Categorical draw from word y": ("cat_word_y", "e17_cat3"),
    "Gaussian block q = 1 reuses q = 0": ("gauss_q1_reuses_q0", "e33_gau5"),
    "the class after the right one at the CDF edge": ("cdf_edge_before_mass", "e15_cat3"),
    "the gate order is i, g, f, o": ("gate_order", "e16_gau1"),
    "b_hh is dropped": ("drop_b_hh", "e16_gau1"),
    "LayerNorm eps is 1e-6": ("ln_eps_1e6", "small_h_cat3"),
    "the head reads the old h": ("head_reads_old_h", "e15_gau4"),
    "stored h and c are swapped": ("stored_swapped", "e1_cat2"),
    "the critic reads the actor's observations": ("critic_reads_actor_obs", "e15_cat3"),
    "the value denormalised with var": ("denorm_var", "e15_cat3"),
    "the bounds rescale is dropped": ("no_rescale", "e33_gau4_bounds"),
    "a forced action is not clamped": ("forced_no_clamp", "e15_cat3"),
    "tile g >= 4 reads the rows of tile g - 4": ("tile_minus_4", "e65_h128_cat3"),
    "commit is ignored": ("ignore_commit", "e17_cat3"),
    "the terminated mask is shifted by one row": ("terminated_shifted", "e129_in256_cat8"),
}


def _caught(s, field):
    """What of a planted float64 launch the GPU test's rules refuse in this case ('' when they accept all of it)."""
    out = []
    for launch in cases.LAUNCHES:
        wrong, fracs = cases.judge(s, s.reference(launch, torch.float64, **{field: True}), launch)
        out += [f"{launch}: {wrong} kept actions"] if wrong else []
        out += [f"{launch}: {k} {v:.3g} x bound" for k, v in fracs.items() if not v <= 1.0]
    return "; ".join(out)


@pytest.mark.parametrize("error", list(PLANTED))
def test_a_named_case_catches_every_planted_error(error):
    field, named = PLANTED[error]
    assert set(cases.Planted._fields) == {f for f, _ in PLANTED.values()}
    what = _caught(cases.steering(named), field)
    print(f"{error}: {named}: {what[:300]}")
    assert what, f"planted error accepted by {named}: {error}"


def test_every_case_beyond_four_tiles_catches_the_tile_mapping_error():
    """The E > 64 cases, and only they, refuse a launch whose tile g >= 4 reads the rows of tile g - 4."""
    for name, c in cases.CASES.items():
        what = _caught(cases.steering(name), "tile_minus_4")
        assert bool(what) == (c["E"] > 64), (name, what)
        if what:
            print(f"{name}: {what[:200]}")
