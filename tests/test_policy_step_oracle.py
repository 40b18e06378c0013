"""
CPU tests of the restated K6+K7 launch (tests/helpers/policy_step_cases.py, the heads of tests/helpers/head_draws.py) that
tests/test_gpu_policy_step_float64.py compares the kernels with:

  * pinning: every case's forced launch in float64 has the log-probs and values of oracle/k12_oracle.py (_module +
    _head_terms, themselves pinned to the g12_* / g16 fixtures) on the same bucket and actions; the MultiDiscrete and
    MultiBinary log-probs are torch.distributions'; the draws are the inverse CDF / the bit test of the probabilities
    the step returns, from the Philox word at the counter the docstrings name, written out by hand.  (torch clamps a
    float64 probability at float64's eps, the kernel a float32 one at float32's: the comparison runs the restatement
    with eps = float64's for the MultiDiscrete and MultiBinary heads and without its clamp for the Categorical one, and
    shows that float32's clamp moves exactly the terms outside [eps32, 1 - eps32], to log(eps32) / log(1 - eps32).)
  * the conditions of every case, met by construction: the near ties of the sampled launch stay within the cap, the
    float32 restatement alone stays inside every bound of every launch, a sampled discrete case draws more than one class
    per slice and bit, the saturated, floored and clamped rows a case claims are there;
  * coverage: the shapes, heads and switches the GPU test needs are among the cases;
  * sharpness: each planted error changes a kept action or pushes a tensor outside its bound in a named case; the
    tile-mapping error fails exactly the E > 64 cases, the second-block error exactly the MultiBinary cases of more than
    four bits;
  * the bucket layout of the helper is oracle.k12_oracle.bucket_tables'.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import k12_oracle as ko

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import policy_step_cases as cases  # noqa: E402
import head_draws as hd  # noqa: E402
import philox  # noqa: E402

CAT, GAU, MCAT, BERN = cases.CAT, cases.GAU, cases.MCAT, cases.BERN
EPS32, EPS64 = cases.EPS32, float(np.finfo(np.float64).eps)
BY_HEAD = {h: [n for n, c in cases.CASES.items() if c["head"] == h] for h in (CAT, GAU, MCAT, BERN)}


def _words(seed, counter, stream):
    return [int(w) for w in philox.philox4x32_10_words((counter & 0xffffffff, counter >> 32, stream, 0),
                                                       (seed & 0xffffffff, seed >> 32))]


# ---------------------------------------------------------------------------------------------------- pinning
@pytest.mark.parametrize("name", list(cases.CASES))
def test_forced_launch_is_the_k12_oracle(name):
    s = cases.steering(name)
    f64 = s.reference("forced", np.float64)              # (the clamp at eps32, as the K12 oracle holds it in every dtype)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        out = ko._module(cases.ko_net(s.actor), s.actor.flat().astype(np.float64), torch.float64)[0](T(s.obs))
        val = ko._module(cases.ko_net(s.critic), s.critic.flat().astype(np.float64), torch.float64)[0](T(s.cobs))
        log_std = T(s.actor.log_std) if s.head == GAU else None
        actions = T(f64["raw"] if s.head in (GAU, BERN) else
                    np.clip(s.forced, 0, s.c["O"] - 1) if s.head == CAT else hd.multi_categorical_pick(s.forced, s.slices))
        logp, _ = ko._head_terms(s.head, out, log_std, actions, s.slices, cases.MIN_STD, {})
    np.testing.assert_allclose(f64["logits"], out.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(f64["value_raw"], val.numpy()[:, 0], rtol=1e-12, atol=1e-13)
    if s.vn is not None:
        np.testing.assert_allclose(f64["value"], s.vn[0] + val.numpy()[:, 0] * np.sqrt(s.vn[1] + 1e-8), rtol=1e-12)
    else:
        np.testing.assert_array_equal(f64["value"], f64["value_raw"])
    rows = np.ones(s.c["E"], bool)
    mine = f64["logp"]
    if s.head == CAT:
        # the K12 oracle clamps at eps32 in every dtype, as the kernel and this restatement do: every row compares below, the
        # clamped ones included.  The restatement's clamp moves exactly the classes outside [eps32, 1 - eps32] -- to
        # log(eps32) / log(1 - eps32)
        q = f64["probs"][np.arange(s.c["E"]), f64["action"]] / f64["probs"].sum(1)
        unclamped = s.reference("forced", np.float64, logp_no_clamp=True)["logp"]
        inside = (q >= EPS32) & (q <= 1.0 - EPS32)
        assert (q >= EPS64).sum() >= max(1, s.c["E"] // 2) and inside.any()
        np.testing.assert_array_equal(f64["logp"][inside], unclamped[inside])
        np.testing.assert_allclose(f64["logp"][q < EPS32], np.log(EPS32), rtol=1e-12)
        np.testing.assert_allclose(f64["logp"][q > 1.0 - EPS32], np.log1p(-EPS32), rtol=1e-12)
    np.testing.assert_allclose(mine[rows], logp.numpy().reshape(-1)[rows], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", BY_HEAD[MCAT] + BY_HEAD[BERN])
def test_multi_discrete_and_multi_binary_log_probs_are_torch_distributions(name):
    s = cases.steering(name)
    for launch in cases.LAUNCHES:
        r = s.reference(launch, np.float64, eps=EPS64)
        z = torch.as_tensor(r["logits"])
        if s.head == MCAT:
            want, o = 0.0, 0
            a = hd.multi_categorical_pick(r["action"], s.slices)
            for j, n in enumerate(s.slices):
                d = torch.distributions.Categorical(probs=torch.softmax(z[:, o:o + n], dim=-1))
                want, o = want + d.log_prob(torch.as_tensor(a[:, j])), o + n
        else:
            d = torch.distributions.Bernoulli(probs=torch.sigmoid(z), validate_args=False)
            want = d.log_prob(torch.as_tensor(r["action"])).sum(-1)
        np.testing.assert_allclose(r["logp"], want.numpy(), rtol=1e-12, atol=1e-12)
        # float32's clamp moves nothing but the terms it clamps
        r32c = s.ref[launch][0]["logp"]
        p = r["probs"]
        clamped = ((p < EPS32) | (p > 1.0 - EPS32)).any(1)
        np.testing.assert_allclose(r32c[~clamped], r["logp"][~clamped], rtol=1e-12, atol=1e-12)


def test_the_multi_discrete_draw_is_the_inverse_cdf_at_the_named_counter():
    """Slice j of row e of md44_e16_wrap_between_64x256 draws word x of block (seed, offset + j E + e, stream 0): at
    offset 2^32 - 16 and E = 16 slice 0 ends on the last counter below the wrap and slice 1 starts on 2^32."""
    s = cases.steering("md44_e16_wrap_between_64x256")
    E = s.c["E"]
    assert s.offset + E == 2 ** 32 and s.slices == (4, 4)
    r = s.ref["sampled"][0]
    for e, j in ((0, 0), (15, 0), (0, 1), (7, 1), (15, 1)):
        c = s.offset + j * E + e
        assert (c >> 32) == j
        u = (_words(s.seed, c, 0)[0] >> 8) / 2.0 ** 24
        p = r["probs"][e, 4 * j:4 * j + 4]
        k = int(np.searchsorted(np.cumsum(p), u * p.sum(), side="right"))
        assert r["action"][e, j] == min(k, 3), (e, j)
    # md2222_e17_wrap: the wrap lies inside slice 0 (row 7)
    s = cases.steering("md2222_e17_wrap_64x128")
    assert (s.offset + 6) >> 32 == 0 and (s.offset + 7) >> 32 == 1


def test_the_multi_binary_draw_is_the_bit_test_at_the_named_counter():
    """Bit d of row e of mb8_e65_64x128: u from word d % 4 of block (seed, offset + e, stream d / 4), the bit u < sigmoid z."""
    s = cases.steering("mb8_e65_64x128")
    r = s.ref["sampled"][0]
    for e, d in ((0, 0), (3, 3), (16, 4), (64, 5), (33, 7)):
        u = (_words(s.seed, s.offset + e, d // 4)[d % 4] >> 8) / 2.0 ** 24
        assert r["action"][e, d] == float(u < 1.0 / (1.0 + np.exp(-r["logits"][e, d]))), (e, d)
        assert abs(abs(u - r["probs"][e, d]) - r["gap"][e, d]) < 1e-15


# ---------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_meets_its_conditions_by_construction(name):
    s = cases.steering(name)
    c, E, O, head = s.c, s.c["E"], s.c["O"], s.head
    r64, f64 = s.ref["sampled"][0], s.ref["forced"][0]
    left = s.left_out("sampled")
    print(f"{name}: {left} of {E} rows near a tie (cap {cases.cap(E)})")
    assert left <= cases.cap(E) and (left < E or E == 1) and s.left_out("forced") == 0
    # the float32 restatement alone: every kept action float64's, every tensor inside its bound; float64 against itself: 0
    for launch in cases.LAUNCHES:
        wrong, fracs = cases.judge(s, s.ref[launch][1], launch)
        print(f"{name} {launch}: float32 restatement " + ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
        assert wrong == 0 and max(fracs.values()) <= 1.0, (launch, wrong, fracs)
        wrong, fracs = cases.judge(s, s.ref[launch][0], launch)
        assert wrong == 0 and max(fracs.values()) == 0.0, (launch, wrong, fracs)
    # no observation row at a kink; the lds need the case is there for
    assert not ko.kinked_rows(cases.ko_net(s.actor), s.actor.flat(), s.obs).any()
    assert not ko.kinked_rows(cases.ko_net(s.critic), s.critic.flat(), s.cobs).any()
    assert cases.lds_bytes(s.actor, s.critic) <= cases.LDS_LIMIT
    z = r64["logits"]
    steered = z[:, 2:] if c["pm20"] else z
    assert 1.0 <= np.sqrt((steered ** 2).mean()) <= (20.0 if c["saturate"] else 2.0)
    assert np.abs(steered).max() < (60.0 if c["saturate"] else 12.0)
    assert (s.vn is not None) == c["norm_values"] and (s.bounds is not None) == c["bounds"]
    if head in (CAT, MCAT):
        slices = s.slices or (O,)
        drawn, f = r64["drawn"].reshape(E, -1), np.asarray(s.forced).reshape(E, -1)
        if E >= 12:
            for j, n in enumerate(slices):
                assert n == 1 or len(np.unique(drawn[:, j])) > 1, f"slice {j} draws one class"
        # the forced launch: an index at or above its slice's classes, one below 0, clamped by the reference
        assert f[-1, -1] >= slices[-1] and f64["action"].reshape(E, -1)[-1, -1] == slices[-1] - 1
        assert E == 1 or (f[0, 0] < 0 and f64["action"].reshape(E, -1)[0, 0] == 0)
        inside = (f >= 0) & (f < np.asarray(slices)[None, :])
        assert np.array_equal(f64["action"].reshape(E, -1)[inside], f[inside])
        if c["saturate"]:
            sat = s.marked["saturated"]
            assert sat.sum() >= 2 and len(slices) == 1                               # (one slice: no other term)
            assert np.allclose(f64["logp"][sat], np.log(EPS32), rtol=1e-12)
            assert np.allclose(s.ref["forced"][1]["logp"][sat], np.log(EPS32), rtol=1e-6)
        elif 1 not in slices:
            assert r64["probs"].min() > 10 * EPS32 and not s.marked
    elif head == BERN:
        if E >= 12:
            bits = r64["drawn"][:, 2:] if c["pm20"] else r64["drawn"]
            assert all(len(np.unique(bits[:, d])) > 1 for d in range(bits.shape[1])), "a bit never changes"
        assert np.array_equal(f64["raw"], s.forced.astype(np.float64)) and (s.forced != r64["drawn"]).any()
        if c["pm20"]:
            assert (z[:, 0] == 20.0).all() and (z[:, 1] == -20.0).all()
            assert (r64["drawn"][:, 0] == 1.0).all() and (r64["drawn"][:, 1] == 0.0).all()
            ex = s.marked["excluded_bit"]
            assert ex.sum() == 4 and (s.forced[ex[:, 0], 0] == 0.0).all() and (s.forced[ex[:, 1], 1] == 1.0).all()
            # float32's sigmoid(20) is 1: the clamp's log(eps32) per excluded bit, not -20
            moved = f64["logp"] - s.reference("forced", np.float64, logp_no_clamp=True)["logp"]
            assert np.allclose(moved[ex.any(1)] / ex.sum(1)[ex.any(1)], np.log(EPS32) + 20.0, atol=1e-6)
    else:
        k = max(1, E // 8)
        a = np.abs(s.forced[:k])
        assert (a >= 3.8 - 1e-6).all() and (a <= 4.2 + 1e-6).all() and (np.abs(s.forced[k]) == 9.0).all()
        assert np.array_equal(f64["raw"], s.forced.astype(np.float64))
        assert s.marked["tanh_clamped"][k] and (1.0 - np.tanh(9.0) ** 2) < 1e-6
        assert np.abs(r64["raw"]).max() > 0.5 and len(np.unique(np.sign(r64["raw"]))) > 1
        floored = hd.gauss_std(s.actor.log_std, 0.0, np.float64) < cases.MIN_STD
        assert floored.any() == c["floor"]
        if c["floor"]:
            d, row = O - 1, int(np.flatnonzero(s.marked["density_clamped"])[0])
            assert floored[d] and floored.sum() == 1 and r64["sd"][d] == cases.MIN_STD
            assert abs(s.forced[row, d] - z[row, d]) > 15 * cases.MIN_STD
            # that dimension's density is the clamp's -100: the log-prob moves when the clamp's row is forced elsewhere
            zz = (s.forced[row, d] - z[row, d]) / cases.MIN_STD
            assert -0.5 * zz * zz - np.log(cases.MIN_STD) - 0.9189385332 < -100.0
        if c["bounds"]:
            lo, hi = s.bounds
            assert len(np.unique(hi - lo)) == O or O == 1
            assert (r64["action"] >= lo).all() and (r64["action"] <= hi).all()


def test_the_cases_cover_what_the_gpu_test_needs():
    cs = cases.CASES
    assert 20 <= len(cs) <= 26
    col = lambda k, h=None: {c[k] for c in cs.values() if h is None or c["head"] == h}
    assert all(len(BY_HEAD[h]) >= 5 for h in BY_HEAD)
    assert {(c["Ha"], c["Hc"]) for c in cs.values()} == set(cases.WIDTH_PAIRS)
    assert col("E") == {1, 15, 16, 17, 63, 65, 129}
    for E in (65, 129):
        assert len({(c["Ha"], c["Hc"]) for c in cs.values() if c["E"] == E}) >= 2
    assert {c["head"] for c in cs.values() if c["E"] > 64} == set(BY_HEAD)
    assert col("Ia") >= {1, 15, 16, 17, 33, 64, 65} and col("Ia") | col("Ic") >= {1, 15, 16, 17, 33, 64, 65}
    assert any(c["Ic"] == 2 * c["Ia"] for c in cs.values()) and any(c["Ic"] == 3 * c["Ia"] for c in cs.values())
    lds = {n: cases.lds_bytes(cases.steering(n).actor, cases.steering(n).critic) for n in cs}
    assert lds["cat2_lds_in376_256x256"] > 64 * 1024 and cs["cat2_lds_in376_256x256"]["Ha"] == 256
    near = lds["mb5_lds_limit_e15_256x512"]
    assert cases.LDS_LIMIT - 4096 <= near <= cases.LDS_LIMIT and cs["mb5_lds_limit_e15_256x512"]["Hc"] == 512
    o = cases.OVER_LDS
    over = 4 * cases.lds_floats(o["Ic"], o["pair"][1], o["Dc"])
    assert cases.LDS_LIMIT < over <= cases.LDS_LIMIT + 1024
    assert col("Da") | col("Dc") >= {1, 2, 3, 4, 7} and any(c["Da"] == 1 and c["Dc"] == 3 for c in cs.values())
    assert col("act") == {"relu", "leaky_relu", "tanh"}
    assert col("O", CAT) == {2, 5, 8} and col("O", GAU) == {1, 3, 4, 5, 8} and col("O", BERN) == {1, 4, 5, 8}
    assert col("slices", MCAT) == {(3, 2), (2, 2, 2, 2), (1, 7), (8,), (1,) * 8, (4, 4)}
    assert {c["bounds"] for c in cs.values() if c["head"] == GAU} == {True, False}
    assert sum(c["floor"] for c in cs.values()) == 1 and sum(c["pm20"] for c in cs.values()) == 1
    assert {c["head"] for c in cs.values() if c["saturate"]} == {CAT, MCAT}
    assert {c["head"] for c in cs.values() if c["offset"] == cases.WRAP and c["E"] > 7} == set(BY_HEAD)
    assert any(c["head"] == MCAT and c["offset"] + c["E"] == 2 ** 32 for c in cs.values())
    assert any(c["offset"] >> 32 and (0x1234ABCD5678 + c["seed"]) >> 32 for c in cs.values())
    norm = [c["norm_values"] for c in cs.values()]
    assert norm[::2] == [False] * len(norm[::2]) and norm[1::2] == [True] * len(norm[1::2])
    assert sum(not c["copies"] for c in cs.values()) == 2
    # the block form: each head, 256/512 and 32/256, E a product of rows not a multiple of 16
    blk = [cs[n] for n in cases.BLOCK_CASES]
    assert len(blk) == 6 and {c["head"] for c in blk} == set(BY_HEAD)
    assert {(256, 512), (32, 256)} <= {(c["Ha"], c["Hc"]) for c in blk}
    for c in blk:
        rows, n = cases.BLOCK_SHAPES[c["E"]]
        assert rows * n == c["E"] and rows % 16 and n <= 16


# ---------------------------------------------------------------------------------------------------- sharpness
# error -> (the planted field, the case named to catch it)
PLANTED = {
    "tile g >= 4 reads the rows of tile g - 4": ("tile_minus_4", "cat8_e65_64x64"),
    "the counter is offset + e + 1": ("counter_plus_one", "cat5_e17_wrap_64x64"),
    "the MultiDiscrete counter is offset + e D + j": ("mcat_counter_row_major", "md2222_e17_wrap_64x128"),
    "every slice takes slice 0's uniform": ("mcat_share_uniform", "md44_e16_wrap_between_64x256"),
    "the MultiDiscrete action is the index in the whole vector": ("mcat_vector_index", "md32_e15_32x32"),
    "a slice of one class adds 0 to the log-prob": ("mcat_one_is_zero", "md1x8_e63_128x128"),
    "the MultiDiscrete CDF edge before the class's mass": ("mcat_edge_before_mass", "md17_e129_32x64"),
    "the Bernoulli words reversed": ("bern_words_reversed", "mb4_e63_64x64"),
    "the Bernoulli counter is offset + e n + d": ("bern_counter_per_bit", "mb5_e17_wrap_256x256"),
    "bits 4 to 7 from block 0 again": ("bern_block0_again", "mb8_e65_64x128"),
    "no log-prob clamp (Categorical)": ("logp_no_clamp", "cat5_sat_e16_128x128"),
    "no log-prob clamp (MultiDiscrete)": ("logp_no_clamp", "md8_sat_e16_256x256"),
    "no log-prob clamp (MultiBinary)": ("logp_no_clamp", "mb8_pm20_e16_32x64"),
    "no min_std floor": ("no_min_std", "gau3_floor_e15_128x256"),
    "lo and hi swapped": ("bounds_swapped", "gau4_e63_wrap_32x64"),
    "the value denormalised with var": ("denorm_var", "cat5_e17_wrap_64x64"),
    "the critic reads the actor's observations": ("critic_reads_actor_obs", "gau1_e16_64x128"),
    "the observation copy shifted by one row": ("copy_shifted", "mb1_e15_32x256"),
    "a forced class is not clamped (Categorical)": ("forced_no_clamp", "cat2_e1_32x32"),
    "a forced class is not clamped (MultiDiscrete)": ("forced_no_clamp", "md32_e15_32x32"),
}


def _caught(s, field):
    """What of a planted float64 launch the GPU test's rules refuse in this case ('' when they accept all of it)."""
    out = []
    for launch in cases.LAUNCHES:
        wrong, fracs = cases.judge(s, s.reference(launch, np.float64, **{field: True}), launch)
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


# the cases an error cannot show in: everything else must refuse it or be another head's
_APPLIES = {
    "tile_minus_4": lambda c: c["E"] > 64,
    "bern_block0_again": lambda c: c["head"] == BERN and c["O"] > 4,
    "denorm_var": lambda c: c["norm_values"],
    "critic_reads_actor_obs": lambda c: True,
    "copy_shifted": lambda c: c["E"] > 1,
    "forced_no_clamp": lambda c: c["head"] in (CAT, MCAT),
    "bounds_swapped": lambda c: c["bounds"],
    "no_min_std": lambda c: c["floor"],
    "mcat_vector_index": lambda c: c["head"] == MCAT and len(c["slices"]) > 1,
}


@pytest.mark.parametrize("field", list(_APPLIES))
def test_these_errors_fail_exactly_the_cases_they_can_show_in(field):
    """Tile g >= 4 reading the rows of tile g - 4 fails the E > 64 cases and no other; bits 4 .. 7 drawn from block 0
    again fail the MultiBinary cases of more than four bits and no other; likewise the errors whose reach is a switch of
    the case: the wrong denormalisation (normalize_values), the critic on the actor's rows (every case), a shifted copy
    (more than one row), an unclamped forced index (Categorical, MultiDiscrete), swapped bounds, no min_std floor, the
    whole-vector index (MultiDiscrete of more than one slice)."""
    for name, c in cases.CASES.items():
        what = _caught(cases.steering(name), field)
        assert bool(what) == _APPLIES[field](c), (name, what)
        if what:
            print(f"{name}: {what[:200]}")


def test_no_planted_error_fails_a_case_of_another_head():
    """An error of one head leaves the other heads' cases as they are (the float64 launch, bitwise)."""
    own = {"mcat": MCAT, "bern": BERN, "no_min_std": GAU, "bounds_swapped": GAU}
    for field in cases.Planted._fields:
        head = next((h for k, h in own.items() if field.startswith(k)), None)
        if head is None:
            continue
        for name, c in cases.CASES.items():
            if c["head"] != head and not (field == "bounds_swapped" and not c["bounds"]):
                assert not _caught(cases.steering(name), field), (field, name)
    for name in BY_HEAD[GAU]:
        if not cases.CASES[name]["bounds"]:
            assert not _caught(cases.steering(name), "bounds_swapped"), name
        if not cases.CASES[name]["floor"]:
            assert not _caught(cases.steering(name), "no_min_std"), name


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("name", ["cat8_e129_32x256", "gau3_floor_e15_128x256", "md17_e129_32x64", "mb5_lds_limit_e15_256x512"])
def test_the_bucket_layout_is_the_k12_oracles(name):
    s = cases.steering(name)
    tables, size = ko.bucket_tables(cases.ko_net(s.actor), cases.ko_net(s.critic), s.head)
    bucket = s.params()
    assert bucket.size == size and s.actor.size() == ko.tensor_table(cases.ko_net(s.actor), s.head == GAU)[1]
    want = {"actor": s.actor, "critic": s.critic}
    used = np.zeros(size, bool)
    for tag, tname, off, shape in tables:
        n = int(np.prod(shape))
        got = bucket[off:off + n].reshape(shape)
        if tname == "log_std":
            ref = want[tag].log_std
        else:
            l, kind = tname.split(".")
            ref = want[tag].layers[int(l)][0 if kind == "weight" else 1]
        assert np.array_equal(got, ref), (tag, tname)
        used[off:off + n] = True
    assert not bucket[~used].any()                                   # the padding
