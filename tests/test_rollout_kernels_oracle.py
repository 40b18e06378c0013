"""
No GPU: tests/helpers/rollout_cases.py (the references of tests/test_gpu_rollout_kernels_float64.py) held to what is already
pinned -- K1 to oracle/episode_info_oracle.py (end_episode, rollout_to_dataset), the C oracle and fixtures g1 / g2, K13 to
oracle/filter_oracle.py, K23 to the torch statements of tests/test_gpu_rollout_finish.py -- and every condition a case
relies on asserted on the reference alone: the steered ends lie where their case says (chunk and tile positions walked
from T and the instantiation's constants), every clip range clips some ending rewards and leaves some, the batch variances
are positive where claimed, the float64 bounds are tight and the float32 floors small.  The K1 bound is shown to hold
between two float64 evaluation orders of the same case, so it is a property of the arithmetic, not of the kernel.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rollout_cases as R  # noqa: E402
from oracle import episode_info_oracle as eo  # noqa: E402
from oracle import filter_oracle as fo  # noqa: E402

F32 = np.float32
SMALL = [c for c in R.TMAJOR_CASES if c["E"] <= 17]
DENSE = [c for c in R.TMAJOR_CASES if c["dense"]] + [R.MISALIGNED_CASE]
_name = lambda c: c["name"]


def _ref(c, inp):
    return R.gae_tmajor_ref(inp["rew"], inp["val"], inp["bv"], inp["br"], inp["ek"], c["gamma"], c["lambd"], c["clip"], c["use_gae"])


def _dense_tables(c, inp):
    """The fixed-length form as the dense tables the oracles take."""
    if c["dense"]:
        return inp["bv"], inp["br"], inp["ek"]
    T, E = c["T"], c["E"]
    bv, br, ekd = np.zeros((T, E), F32), np.zeros((T, E), F32), np.zeros((T, E), np.int8)
    bv[-1], br[-1], ekd[-1] = inp["bv"], inp["br"], 2
    return bv, br, ekd


def _f64_part(ref, k):
    """The bound without its float32 output rounding: what two float64 evaluations may differ by."""
    return ref[k + "_bound"] - R.U23 * np.abs(ref[k]) + 1e-300


# ============================================================================================================== K1
@pytest.mark.parametrize("c", SMALL, ids=_name)
def test_k1_restatement_is_the_episode_oracle(c):
    inp = R.tmajor_inputs(c)
    ref = _ref(c, inp)
    bv, br, ekd = _dense_tables(c, inp)
    d = eo.rollout_to_dataset(inp["rew"], inp["val"], bv, br, ekd, c["gamma"], c["lambd"], c["clip"], c["use_gae"])
    ft, fe = d["flat_t"], d["flat_e"]
    assert len(ft) == c["T"] * c["E"]
    for k in ("adv", "rtg"):
        assert R.frac_abs(d[k], ref[k][ft, fe], ref[k + "_bound"][ft, fe]) <= 1.0
    # before the dataset's float32 cast: the oracle's float64 values, segment by segment
    for e, t0, t1, kind in d["segs"][:40]:
        a, g = eo.end_episode(inp["rew"][t0:t1 + 1, e], inp["val"][t0:t1 + 1, e], 0.0 if kind == 1 else float(bv[t1, e]),
                              0.0 if kind == 1 else float(br[t1, e]), c["gamma"], c["lambd"], c["clip"], c["use_gae"])
        assert R.frac_abs(a, ref["adv"][t0:t1 + 1, e], _f64_part(ref, "adv")[t0:t1 + 1, e]) <= 1.0
        assert R.frac_abs(g, ref["rtg"][t0:t1 + 1, e], _f64_part(ref, "rtg")[t0:t1 + 1, e]) <= 1.0


@pytest.mark.parametrize("name", ["chunk32_E8193_T129_dense", "chunk32_E8223_T9_fixed", "chunk16_E8191_T257_dense", "chunk16_E8191_T5_fixed"])
def test_k1_restatement_is_the_c_oracle(name):
    from oracle import c_oracle
    c = next(c for c in R.TMAJOR_CASES if c["name"] == name)
    inp = R.tmajor_inputs(c)
    ref = _ref(c, inp)
    bv, br, ekd = _dense_tables(c, inp)
    adv, rtg = c_oracle.gae_rtg_tmajor(inp["rew"], inp["val"], bv, br, ekd, c["gamma"], c["lambd"], c["clip"], c["use_gae"])
    assert R.frac_abs(adv, ref["adv"], ref["adv_bound"]) <= 1.0 and R.frac_abs(rtg, ref["rtg"], ref["rtg_bound"]) <= 1.0


def test_k1_restatement_against_golden_g1(golden):
    """Every recorded end_episode case as a one-column fixed-length rollout: the oracle on the same float32 rewards to the
    float64 bound, and the reference's own outputs where its rewards are exact in float32."""
    g = golden("g1_end_episode")
    exact = 0
    for i in range(int(g["n_cases"][0])):
        p = g[f"c{i}_params"]
        gamma, lambd, use_gae, clip = float(p[0]), float(p[1]), bool(p[2]), None if np.isnan(p[3]) else (float(p[3]), float(p[4]))
        rew, val = g[f"c{i}_rewards"].astype(F32), g[f"c{i}_values"].astype(F32)
        ev, er = np.array([p[5]], F32), np.array([p[6]], F32)
        ref = R.gae_tmajor_ref(rew[:, None], val[:, None], ev, er, None, gamma, lambd, clip, use_gae)
        a, r = eo.end_episode(rew, val, float(ev[0]), float(er[0]), gamma, lambd, clip, use_gae)
        assert R.frac_abs(a, ref["adv"][:, 0], _f64_part(ref, "adv")[:, 0]) <= 1.0, i
        assert R.frac_abs(r, ref["rtg"][:, 0], _f64_part(ref, "rtg")[:, 0]) <= 1.0, i
        if (g[f"c{i}_rewards"] == 1.0).all():
            exact += 1
            assert R.frac_abs(g[f"c{i}_rtg_f64"].astype(F32), ref["rtg"][:, 0], ref["rtg_bound"][:, 0]) <= 1.0, i
            if use_gae:
                assert R.frac_abs(g[f"c{i}_adv"].astype(F32), ref["adv"][:, 0], ref["adv_bound"][:, 0]) <= 1.0, i
    assert exact > 0


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_k1_restatement_against_golden_g2(golden, tag):
    g = golden("g2_dataset")
    rew, val, boot, ekd = (g[f"{tag}_in_{k}"] for k in ("rewards", "values", "boot_v", "end_kind"))
    ref = R.gae_tmajor_ref(rew.astype(F32), val.astype(F32), boot.astype(F32), boot.astype(F32), ekd, 0.99, 0.95, (-100.0, 100.0), True)
    d = eo.rollout_to_dataset(rew.astype(F32), val, boot, boot, ekd)
    ft, fe = d["flat_t"], d["flat_e"]
    # the fixture ran on float64 rewards: 1e-5, as the GPU test of the same fixture
    np.testing.assert_allclose(ref["adv"][ft, fe], g[tag + "_adv"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ref["rtg"][ft, fe], g[tag + "_rtg"], rtol=1e-5, atol=1e-5)
    assert R.frac_abs(d["adv"], ref["adv"][ft, fe], ref["adv_bound"][ft, fe]) <= 1.0


@pytest.mark.parametrize("c", R.TRAJ_CASES, ids=_name)
def test_k1_trajectory_cases(c):
    inp = R.traj_inputs(c)
    ref = R.gae_traj_ref(inp, c)
    n, lens, start = len(inp["lens"]), inp["lens"], inp["start"]
    assert inp["used"].sum() == lens.sum() and not inp["used"][:R.TRAJ_GAP].any() and not inp["used"][-R.TRAJ_GAP:].any()
    assert n == 1 or (np.diff(start) < 0).any(), "the start table is in address order"
    assert np.isnan(ref["adv"][~inp["used"]]).all() and np.isfinite(ref["adv"][inp["used"]]).all()
    for i in range(n):
        a, r = eo.end_episode(inp["rew"][start[i]:start[i] + lens[i]], inp["val"][start[i]:start[i] + lens[i]], float(inp["ev"][i]),
                              float(inp["er"][i]), c["gamma"], c["lambd"], c["clip"], c["use_gae"])
        sl = slice(start[i], start[i] + lens[i])
        assert R.frac_abs(a, ref["adv"][sl], _f64_part(ref, "adv")[sl]) <= 1.0 and R.frac_abs(r, ref["rtg"][sl], _f64_part(ref, "rtg")[sl]) <= 1.0
    if c["clip"] is not None and n > 1:
        er = inp["er"][lens > 0]
        assert ((er < c["clip"][0]) | (er > c["clip"][1])).any()


def test_k1_trajectory_cases_cover_the_issue():
    lens = {L for c in R.TRAJ_CASES for L in c["lens"]}
    assert lens == {0, 1, 63, 64, 65, 128, 129, 1000} and {len(c["lens"]) for c in R.TRAJ_CASES} == {1, 3, 4, 5, 9}
    for c in R.TRAJ_CASES:
        if 0 in c["lens"]:
            assert 0 < c["lens"].index(0) < len(c["lens"]) - 1
    assert any(not c["rtg"] and c["use_gae"] for c in R.TRAJ_CASES) and all(c["rtg"] or c["use_gae"] for c in R.TRAJ_CASES)
    assert any(not c["use_gae"] for c in R.TRAJ_CASES)


def test_k1_cases_cover_the_launch_forms():
    for inst, d in R.INST.items():
        cases = [c for c in R.TMAJOR_CASES if c["inst"] == inst]
        assert {c["E"] for c in cases} == set(d["E"]) and {c["T"] for c in cases} == set(d["T"]), inst
        assert {c["dense"] for c in cases} == {True, False}, inst
        assert all(R.instantiation(c["E"]) == inst for c in cases)
        pairs = {(c["gamma"], c["lambd"]) for c in cases}
        assert (pairs == set(R.GAMMA_LAMBDA) if inst.startswith("chunk") else len(pairs) >= 2) and {c["use_gae"] for c in cases} == {True, False}, inst
        assert {c["clip"] for c in cases} == set(R.CLIPS), inst
        if d["tile"]:
            assert any(c["T"] > d["tile"] for c in cases) and d["tile"] % d["chunk"] == 0
    assert {(c["gamma"], c["lambd"]) for c in R.TMAJOR_CASES} == set(R.GAMMA_LAMBDA)
    assert {c["density"] for c in DENSE} == set(R.DENSITIES)
    m = R.MISALIGNED_CASE
    assert m["E"] == 2 ** 20 and m["T"] == 3 and R.instantiation(m["E"]) == "stream4" and R.instantiation(m["E"], False) == "stream1"
    assert sorted(R.MISALIGNED) == sorted([("rewards", 4), ("values", 4), ("adv_out", 4), ("rtg_out", 4), ("end_kind", 1), ("end_kind", 4)])
    assert R.INST["chunk16"]["tile"] == 8 * (64 // 16) * 4 and R.INST["chunk32"]["tile"] == 8 * (64 // 32) * 8


@pytest.mark.parametrize("c", DENSE, ids=_name)
def test_k1_steered_ends_lie_where_the_case_says(c):
    """The chunk and tile positions come from walking T with the instantiation's constants (rollout_cases.chunk_edges), not
    from the arithmetic that placed the ends."""
    inst, T, E = R.INST[c["inst"]], c["T"], c["E"]
    ekd = R.tmajor_inputs(c)["ek"]
    edges = R.chunk_edges(T, inst["chunk"], inst["tile"])
    pats = R.column_patterns(c)
    cols = inst["cols"]
    assert 0 in pats and E - 1 in pats and all(0 <= col < E for col in pats)
    if E > cols:
        assert {col % cols for col in pats} >= {0, cols - 1}, "a workgroup's first and last column"
    assert (ekd[-1] != 0).all() and set(np.unique(ekd)) <= {0, 1, 2}
    for col, pat in pats.items():
        inner = ekd[:-1, col] != 0                                       # the last row is closed in any case
        if pat in ("chunk_first", "chunk_last", "tile_first", "tile_last"):
            here = edges[pat][:-1]
            if pat.startswith("tile") and not inst["tile"]:
                assert not inner.any()
                continue
            assert (inner <= here).all(), f"{pat}: an end off its edge in column {col}"
            if pat == "chunk_first":
                assert inner.any() == (T > inst["chunk"] or (T == inst["chunk"] and T > 1))
            if pat == "chunk_last":
                assert inner.any() == (T > inst["chunk"])
            if pat == "tile_first":
                assert inner.any() == (T > inst["tile"] or (T == inst["tile"]))
            if pat == "tile_last":
                assert inner.any() == (T > inst["tile"])
        elif pat == "consecutive":
            assert inner.sum() == (2 if T >= 3 else 0) and (T < 3 or np.diff(np.flatnonzero(inner)).tolist() == [1])
        elif pat == "every":
            assert inner.all()
        elif pat == "none":
            assert not inner.any()
        elif pat == "alternating":
            assert inner.all() and (T < 2 or (np.abs(np.diff(ekd[:-1, col].astype(int))) == 1).all())


def test_k1_every_pattern_meets_every_column_kind():
    for inst, d in R.INST.items():
        seen = set()
        for c in (c for c in DENSE if c["inst"] == inst and c["T"] >= 3):
            for col, pat in R.column_patterns(c).items():
                kinds = {"zero"} if col == 0 else set()
                if col % d["cols"] == 0 and col:
                    kinds.add("first")
                if col % d["cols"] == d["cols"] - 1:
                    kinds.add("last")
                if col == c["E"] - 1 and c["E"] % d["cols"]:
                    kinds.add("ragged")
                seen |= {(pat, k) for k in kinds}
        pats = [p for p in R.PATTERNS if d["tile"] or not p.startswith("tile")]
        want = {(p, k) for p in pats for k in ("zero", "first", "last", "ragged")}
        if inst in ("chunk16", "chunk32"):
            assert seen >= want, (inst, sorted(want - seen))
        else:                                   # the few large cases: every pattern, and every kind of column
            assert {p for p, _ in seen} >= set(pats) and {k for _, k in seen} == {"zero", "first", "last", "ragged"}, inst


@pytest.mark.parametrize("c", [c for c in R.TMAJOR_CASES + [R.MISALIGNED_CASE] if c["clip"] and c["E"] >= 15], ids=_name)
def test_k1_clip_ranges_bite_and_spare(c):
    inp = R.tmajor_inputs(c)
    lo, hi = c["clip"]
    er = inp["br"][inp["ek"] == 2] if c["dense"] else inp["br"]
    assert ((er < lo) | (er > hi)).any() and ((er > lo) & (er < hi)).any() and (er.size < 1000 or np.abs(er).max() > 100)
    if c["dense"] and c["T"] >= 3 and c["E"] >= 8191:
        assert (inp["ek"] == 1).any() and (lo <= 0.0 <= hi or R.clip32(np.zeros(1, F32), c["clip"])[0] == F32(lo))


@pytest.mark.parametrize("name", ["chunk16_E17_T257_dense", "chunk16_E16_T129_dense", "chunk16_E15_T128_dense", "chunk16_E17_T127_fixed",
                                  "chunk16_E17_T5_dense", "chunk16_E16_T257_fixed"])
@pytest.mark.parametrize("inst", ["chunk16", "chunk32", "stream1"])
def test_k1_bound_holds_between_two_float64_evaluation_orders(name, inst):
    c = next(c for c in R.TMAJOR_CASES if c["name"] == name)
    inp = R.tmajor_inputs(c)
    ref = R.gae_tmajor_ref(inp["rew"], inp["val"], inp["bv"], inp["br"], inp["ek"], c["gamma"], c["lambd"], c["clip"], True)
    adv, rtg = R.gae_tmajor_composed(inp["rew"], inp["val"], inp["bv"], inp["br"], inp["ek"], c["gamma"], c["lambd"], c["clip"],
                                     R.INST[inst]["chunk"], R.INST[inst]["tile"])
    fa, fr = R.frac_abs(adv, ref["adv"], _f64_part(ref, "adv")), R.frac_abs(rtg, ref["rtg"], _f64_part(ref, "rtg"))
    print(f"{name} in the order of {inst}: adv {fa:.3f}, rtg {fr:.3f} of the float64 part of the bound")
    assert fa <= 1.0 and fr <= 1.0
    # and the bound is no licence: the float64 part is far below the float32 rounding it is added to
    assert (_f64_part(ref, "adv") <= 1e-3 * R.U23 * np.abs(ref["adv"]).max()).all()


def test_k1_bound_notices_a_wrong_chain():
    """gamma in the place of gamma * lambda, or an unclipped terminal seed, lies far outside the bound."""
    c = dict(next(c for c in R.TMAJOR_CASES if c["name"] == "chunk16_E17_T129_dense"), gamma=0.99, lambd=0.95, clip=(-0.5, 0.5), use_gae=True)
    inp = R.tmajor_inputs(c)
    ref = _ref(c, inp)
    wrong = R.gae_tmajor_ref(inp["rew"], inp["val"], inp["bv"], inp["br"], inp["ek"], c["gamma"], 1.0, c["clip"], True)
    assert c["lambd"] != 1.0 and R.frac_abs(wrong["adv"].astype(F32), ref["adv"], ref["adv_bound"]) > 100
    c2 = dict(c, clip=(0.25, 2.0))
    a, b = _ref(c2, inp), R.gae_tmajor_ref(inp["rew"], inp["val"], inp["bv"], np.where(inp["ek"] == 1, F32(0.25), inp["br"]), np.where(
        inp["ek"] == 1, 2, inp["ek"]).astype(np.int8), c["gamma"], c["lambd"], (0.25, 2.0), False)
    assert R.frac_abs(a["rtg"], b["rtg"], a["rtg_bound"]) <= 1.0, "a terminal end seeds rtg with clip(0)"


# ============================================================================================================== K13
@pytest.mark.parametrize("c", R.K13_CASES, ids=_name)
def test_k13_case_conditions(c):
    cc, steps = R.k13_case(c), R.k13_inputs(c)
    r64, r32 = R.k13_reference(c, np.float64), R.k13_reference(c, np.float32)
    G, W, n = cc["G"], cc["W"], cc["n"]
    for k, (ranks, o64, o32) in enumerate(zip(steps, r64, r32)):
        for s in "oc":
            if s not in cc["streams"]:
                continue
            if n >= 2:                                                    # a positive batch variance in every column
                assert (R.obs_records(ranks[0][s], G)[1] > 0).all()
            tensors = [(o64[s], o32[s])] + ([(o64[s + "_state"][j], o32[s + "_state"][j]) for j in (0, 1)] if cc["normalize"] else [])
            for x64, x32 in tensors:                                      # the float32 floor tests something
                assert 4.0 * np.abs(x32.astype(np.float64) - x64).max() <= 1e-3 * np.abs(x64).max(), (k, s)
            assert np.isfinite(o64[s]).all() and (cc["clip"] is None or (o64[s].min() >= cc["clip"][0] and o64[s].max() <= cc["clip"][1]))
            if cc["clip"] is not None and cc["clip"][0] < cc["clip"][1] and n >= 64:
                assert (o64[s] == cc["clip"][0]).any() and (o64[s] == cc["clip"][1]).any() and ((o64[s] > cc["clip"][0]) & (o64[s] < cc["clip"][1])).any()
        if "r" in cc["streams"]:
            assert 4.0 * np.abs(o32["r"].astype(np.float64) - o64["r"]).max() <= 1e-3 * np.abs(o64["r"]).max(), k
            if cc["normalize"]:
                st = o64["r_state"]
                scale = np.sqrt(st["var"] + st["mean"] ** 2)
                assert (st["var"] > 0).all() and (st["b_var"] < 1e-9 * st["var"]).all() and (st["b_mean"] < 1e-9 * scale).all(), (k, st["b_var"] / st["var"])
                assert (st["b_rr"] <= 1e-9 * np.maximum(np.abs(st["rr"]), 1e-6)).all()
    if cc["normalize"] and "r" in cc["streams"]:
        assert (r64[-1]["r_state"]["rr"] == 0.0).any() and (r64[-1]["r_state"]["rr"] != 0.0).any()
    if cc["data"] == "far" and cc["normalize"]:
        for s in (s for s in "oc" if s in cc["streams"]):
            assert (np.abs(r64[-1][s + "_state"][0]) > 900).all()
    if cc["data"] == "tiny":
        for s in (s for s in "oc" if s in cc["streams"]):
            v = r64[-1][s + "_state"][1]
            assert ((R.K13_EPS / (v + R.K13_EPS)) > 1e-4).all(), "eps does not matter to this case"
    if cc["frozen"]:
        for s in cc["frozen"]:
            key = s + "_state"
            a, b = (r64[0][key], r64[-1][key])
            same = all(np.array_equal(a[j], b[j]) for j in ((0, 1, 2) if s in "oc" else ("mean", "var", "count")))
            assert same, "a frozen stream's statistics moved"


def test_k13_cases_cover_the_issue():
    cs = [R.k13_case(c) for c in R.K13_CASES]
    assert {c["n"] for c in cs} >= {1, 2, 63, 64, 65, 255, 256, 257, 1000} and {c["G"] for c in cs} == {1, 3} and {c["W"] for c in cs} == {1, 17}
    assert {c["streams"] for c in cs} >= {"ocr", "r", "c", "or"} and {c["gamma"] for c in cs} == {0.97, 1.0} and {c["done2"] for c in cs} == {True, False}
    assert {c["data"] for c in cs} == {"std", "far", "tiny"} and any(c["reward"] == "far" for c in cs)
    assert any(c["frozen"] and c["frozen"] != c["streams"] for c in cs) and any(not c["normalize"] for c in cs)
    assert any(c["clip"] and c["clip"][0] == c["clip"][1] for c in cs) and all(c["steps"] == 3 for c in cs)
    r3 = [c for c in cs if len(c["ranks"]) == 3]
    assert any(len(set(c["ranks"])) == 3 and "r" not in c["streams"] for c in r3) and any(0 in c["ranks"] and "r" in c["streams"] for c in r3)
    assert all(len({nr for nr in c["ranks"] if nr}) == 1 for c in r3 if "r" in c["streams"]), "the reward stream has equal n per rank"


def test_k13_restatement_is_the_filter_oracle():
    """A short single-rank stream of all three filters against FilteredEnvOracle (its moments are float32: to float32
    rounding), the reward state against its float64 state tightly; and three ranks against reward_filter_ranks."""
    c = dict(name="short", n=5, G=2, W=3, clip=(-1.2, 1.2), rclip=(-0.8, 0.8))
    steps = R.k13_inputs(c)
    mine = R.k13_reference(c, np.float32)
    env = fo.FilteredEnvOracle(2, 5, 3, 3, obs_clip=(-1.2, 1.2), reward_clip=(-0.8, 0.8), gamma=0.97)
    for ranks, o in zip(steps, mine):
        r = ranks[0]
        obs, cobs, rew = env.filter_step(r["o"], r["c"], r["r"], r["term"], r["trunc"])
        for got, want in ((o["o"], obs), (o["c"], cobs), (o["r"], rew)):
            np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(o["o_state"][0], np.stack([s.mean for s in env.obs_norm.stats]), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(o["c_state"][1], np.stack([s.variance for s in env.cobs_norm.stats]), rtol=1e-5, atol=1e-6)
        st = o["r_state"]
        np.testing.assert_allclose(st["mean"], [float(s.mean) for s in env.rew_norm.stats], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(st["var"], [float(s.variance) for s in env.rew_norm.stats], rtol=1e-12)
        np.testing.assert_allclose(st["count"], [s.count for s in env.rew_norm.stats], rtol=1e-15)
        np.testing.assert_allclose(st["rr"], np.stack(env.rew_norm.running_reward), rtol=1e-15)
    # three ranks with rows
    G, n = 2, 4
    rng = np.random.default_rng(0)
    oracles = [fo.RewardNormalizerOracle(G, n, gamma=0.9) for _ in range(3)]
    ref = R.RewardStreamRef(G, n, 3, 0.9, np.float64)
    for _ in range(3):
        rews = [rng.standard_normal(G * n).astype(F32) + 3 for _ in range(3)]
        dones = [rng.random(G * n) < 0.3 for _ in range(3)]
        want = fo.reward_filter_ranks(oracles, rews, dones)
        got = ref.step(rews, dones, True, True, None)
        np.testing.assert_allclose(got, want[0], rtol=1e-6)
        np.testing.assert_allclose(ref.var, [float(s.variance) for s in oracles[0].stats], rtol=1e-12)
        np.testing.assert_allclose(ref.rr[1], np.stack(oracles[1].running_reward), rtol=1e-15)


def test_k13_the_pooled_identity_the_kernel_uses_lies_inside_the_bound():
    """The kernel's one merge of the n * n_all pooled values, in float64 on the host, against the sequential procedure: the
    identity holds to the derived bound, and a weight off by one does not."""
    for name in ("n255_G3_W17_far", "R3_equal_n", "n1000_G3_reward_only"):
        c = next(c for c in R.K13_CASES if c["name"] == name)
        cc, ranks = R.k13_case(c), R.k13_inputs(c)[0]
        st = R.k13_reference(c, np.float64)[0]["r_state"]
        G, n = cc["G"], cc["n"]
        rew = np.stack([r["r"].astype(np.float64).reshape(G, n) for r in ranks if r is not None])
        for off, inside in ((0, True), (1, False)):
            i = np.arange(n)
            s1 = ((n - i - off) * rew).sum((0, 2))                       # old = 0, m = 0 at the first step
            s2 = ((n - i - off) * rew * rew).sum((0, 2))
            cnt = 1e-4 + float(n) * n * len(rew)
            mean, var = s1 / cnt, (1e-4 * 1.0 + s2 - s1 * s1 / cnt) / cnt
            ok = (np.abs(mean - st["mean"]) <= st["b_mean"]).all() and (np.abs(var - st["var"]) <= st["b_var"]).all()
            assert ok == inside, (name, off)


# ============================================================================================================== K23
def test_k23_restatement_is_the_torch_statements(monkeypatch):
    import test_gpu_rollout_finish as trf
    monkeypatch.setattr(trf, "DEV", torch.device("cpu"))
    for layout, (A, members) in trf.LAYOUTS.items():
        for E, w, with_intr in ((17, 0.37, True), (5, 1.0, True), (17, 0.37, False)):
            g = torch.Generator().manual_seed(E)
            term, trunc = trf._flags(E, g)
            rnd = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
            rew = [{a: rnd(E) for a in range(A)} for _ in range(trf.T)]
            nat = [{a: rnd(E) for a in range(A)} for _ in range(trf.T)]
            intr = [rnd(trf.T, len(agents) * E) if with_intr and m != 0 else None for m, (_, agents, _) in enumerate(members)]
            want, want_ts, _ = trf._torch_reference(members, E, w, rew, nat, intr, term, trunc)
            mem = [(len(agents), kind == "mat") for kind, agents, _ in members]
            orders = [order for _, _, order in members]
            c = dict(E=E, w=w, write_ends=True, truncated=True)
            outs = [dict(reward=np.zeros(n * E, F32), natural=np.zeros(n * E, F32), end_kind=np.zeros(E if grouped else n * E, np.int8)) for n, grouped in mem]
            ep_ts = np.zeros(E, np.int32)
            for t in range(trf.T):
                step = dict(term=term[t].numpy(), trunc=trunc[t].numpy(), last=t == trf.T - 1, members=[
                    dict(reward=np.stack([rew[t][a].numpy() for a in agents]), natural=np.stack([nat[t][a].numpy() for a in agents]),
                         natural_given=np.ones(len(agents), bool), intrinsic=None if intr[m] is None else intr[m][t].numpy())
                    for m, (_, agents, _) in enumerate(members)])
                ep_ts, outs = R.finish_ref(c, step, ep_ts, outs, mem, orders, trf.MAX_TS)
                for m, o in enumerate(outs):
                    assert np.array_equal(o["reward"].view(np.uint32), want[m]["rewards"][t].numpy().view(np.uint32)), (layout, t, m)
                    assert np.array_equal(o["natural"], want[m]["natural"][t].numpy()) and np.array_equal(o["end_kind"], want[m]["end_kind"][t].numpy())
            assert np.array_equal(ep_ts, want_ts.numpy())


@pytest.mark.parametrize("c", R.FINISH_CASES, ids=_name)
def test_k23_case_conditions(c):
    E, steps = c["E"], R.finish_inputs(c)
    ts, outs = (np.arange(E) % R.FINISH_MAX_TS).astype(np.int32), R.finish_blank_outs(c)
    kinds, fma_differs = set(), 0
    for step in steps:
        ts, outs = R.finish_ref(c, step, ts, outs)
        for m, ((n, grouped), mem, o) in enumerate(zip(R.FINISH_MEMBERS, step["members"], outs)):
            assert not (o["reward"] == F32(-777.0)).any() and (o["natural"] is None or not (o["natural"] == F32(-777.0)).any())
            kinds |= set(np.unique(o["end_kind"]).tolist())
            if mem["intrinsic"] is not None and not grouped and c["w"] != 1.0:
                fused = (mem["reward"].astype(np.float64).reshape(-1) * float(F32(c["w"])) + mem["intrinsic"]).astype(F32)
                fma_differs += int((fused != o["reward"]).sum())
    assert kinds == ({0, 1, 2} if c["write_ends"] else {-7})
    if c["intrinsic"] and c["w"] != 1.0:
        assert fma_differs > 100, "one fused rounding would pass for two"
    assert c["w"] == 1.0 or float(F32(c["w"])) != c["w"]


def test_k23_cases_cover_the_issue():
    assert {c["E"] for c in R.FINISH_CASES} == {255, 256, 257, 513} and len(R.FINISH_MEMBERS) == 8
    assert max(n for n, _ in R.FINISH_MEMBERS) == 16 and any(g and n > 1 for n, g in R.FINISH_MEMBERS)
    for m, (n, grouped) in enumerate(R.FINISH_MEMBERS):
        if grouped and n > 1:
            p = R.finish_slot_agent(m, n)
            assert sorted(p) == list(range(n)) and (p != np.arange(n)).any()
    assert any(c["natural"] == "some" for c in R.FINISH_CASES) and any(not c["truncated"] for c in R.FINISH_CASES)
    assert any(not c["write_ends"] for c in R.FINISH_CASES) and {c["w"] for c in R.FINISH_CASES} == {1.0, 0.37}
