"""
No GPU: tests/helpers/primitive_cases.py (the float64 references of tests/test_gpu_primitives_float64.py) held to what is
already pinned -- oracle/ppo_loss_oracle.py (golden fixtures g8 / g12), oracle/running_stats_oracle.py (g4),
`_attention_ref` of tests/test_gpu_kernels.py, torch.optim.Adam + clip_grad_norm_ -- on every case the GPU file runs, and
every condition such a case relies on asserted on the reference alone: the rows meant to take a branch take it in float64,
and no other row lies within float32 rounding of a branch edge.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_draws as hd  # noqa: E402
import primitive_cases as P  # noqa: E402
from oracle import k12_oracle as ko  # noqa: E402
from oracle import ppo_loss_oracle as plo  # noqa: E402
from oracle import running_stats_oracle as rso  # noqa: E402

F32 = np.float32


def close32(got, want, what, rel=1e-5, scale=3e-6):
    """Agreement to float32 rounding: |got - want| <= rel |want| + scale max|want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = rel * np.abs(want) + scale * (np.abs(want).max() if want.size else 0.0) + 1e-30
    assert got.shape == want.shape and (np.abs(got - want) <= tol).all(), \
        f"{what}: worst {np.abs(got - want).max():.3g} against {tol.reshape(-1)[np.abs(got - want).argmax()]:.3g}"


# ------------------------------------------------------------------------------------------------------------ K2 + K3
FINITE_LOSS = [c for c in P.LOSS_CASES if not c.get("bad")]


@pytest.mark.parametrize("c", FINITE_LOSS, ids=lambda c: c["name"])
def test_loss_restatement_is_the_pinned_oracle(c):
    cc, inp = P.loss_case(c), P.loss_inputs(c)
    r = P.loss_ref(inp, c, np.float32)
    t = {k: torch.tensor(inp[k], requires_grad=k in ("cur", "values")) for k in ("cur", "old", "adv", "values", "rtg")}
    ent = torch.tensor(np.zeros(cc["B"], F32) if inp["ent"] is None else inp["ent"], requires_grad=True)
    o = plo.ppo_minibatch_losses(t["cur"], t["old"], t["adv"], ent, t["values"], t["rtg"], cc["normalize"], cc["clip"],
                                 cc["ent_w"], cc["kl"], cc["huber"])
    (o["actor_loss"] + o["critic_loss"]).backward()
    want = [o["surr"], o["actor"], o["critic"], o["entropy"], o["kl"], o["adv_mean"] or 0.0, 1.0 if o["adv_std"] is None else o["adv_std"]]
    if cc["ent_w"] == 0.0:
        want[3] = r["scalars"][3]                                         # the kernel reports the mean whatever its weight
    close32(r["scalars"][:7], want, "scalars")
    assert r["scalars"][7] == 0.0 and not o["bad"]
    close32(r["d_logp"], t["cur"].grad.numpy(), "d_logp")
    close32(r["d_values"], t["values"].grad.numpy(), "d_values")
    close32(r["d_entropy"], np.zeros(cc["B"]) if ent.grad is None else ent.grad.numpy(), "d_entropy")


@pytest.mark.parametrize("c", P.LOSS_CASES, ids=lambda c: c["name"])
def test_loss_cases_take_their_branches(c):
    cc, inp = P.loss_case(c), P.loss_inputs(c)
    B, cls = cc["B"], inp["cls"]
    if cc["bad"]:
        with np.errstate(over="ignore", invalid="ignore"):
            r32 = np.exp(inp["cur"] - inp["old"])
        bad = ~np.isfinite(r32)
        assert bad.sum() == 1 and (np.isinf(r32[1]) if cc["bad"] == "inf" else np.isnan(r32[1]))
        return
    ratio, a, ad = P.loss_rows(inp, c)
    lo, hi = float(F32(1) - F32(cc["clip"])), float(F32(1) + F32(cc["clip"]))
    assert np.abs(a).min() > 1e-3, "an advantage whose sign float32 could change"
    if cc["ratio_one"]:
        assert (ratio == 1.0).all() and lo == 1.0 and hi == 1.0 and (a > 0).any() and (a < 0).any()
    else:
        gap = 1e-3
        assert ((ratio[cls == P.INSIDE] > lo + gap) & (ratio[cls == P.INSIDE] < hi - gap)).all()
        assert (ratio[cls == P.BELOW] < lo - gap).all() and (ratio[cls == P.ABOVE] > hi + gap).all()
        if B >= 8:           # the placed rows: on the edge to the device's expf rounding, loss and gradient continuous across it
            assert abs(ratio[6] - lo) < 1e-6 and a[6] > 0 and abs(ratio[7] - hi) < 1e-6 and a[7] < 0
        if B >= 63:
            for k in (P.INSIDE, P.BELOW, P.ABOVE):
                assert ((cls == k) & (a > 0)).any() and ((cls == k) & (a < 0)).any(), "a ratio class lacks a sign of advantage"
    if cc["adv_mean"]:
        assert inp["adv"].mean() > 999.0 and 0.5 < inp["adv"].astype(np.float64).std() < 2.0
    d = inp["values"].astype(np.float64) - inp["rtg"]
    placed = np.zeros(B, bool)
    placed[2:4] = True
    assert (d[2:4] == np.array([10.0, -10.0])[:max(0, min(B, 4) - 2)]).all()
    assert (np.abs(ad[~placed] - 10.0) > 1e-3).all(), "|value - rtg| within float32 rounding of Huber's delta"
    if B >= 2:
        assert d[0] > 10.0 and d[1] < -10.0
    if B >= 63:
        assert (ad < 10.0).sum() > B // 2


# ------------------------------------------------------------------------------------------------------------ K4
def test_gather_and_scatter_restatements():
    src = np.arange(12, dtype=np.int64).reshape(6, 2)
    dst0 = np.full((4, 2), -7, np.int64)
    perm, row_map = np.array([5, -1, 4, 0]), np.array([3, 2, 1, 0, 5], np.int32)
    got = P.gather_ref(src, dst0, perm, row_map, 5)
    assert got.tolist() == [[-7, -7], [-7, -7], [10, 11], [6, 7]]
    assert P.gather_ref(src, dst0, perm, None, 6).tolist() == [[10, 11], [-7, -7], [8, 9], [0, 1]]
    s = P.scatter_ref(np.array([1.0, 2.0, 3.0, 4.0]), np.zeros(6), perm, row_map, 5)
    assert s.tolist() == [0.0, 0.0, 0.0, 4.0, 0.0, 3.0]


# ------------------------------------------------------------------------------------------------------------ K5
@pytest.mark.parametrize("n,W", P.MOMENT_SHAPES)
def test_moments_restatement(n, W):
    x = P.moments_data(n, W)
    rec, bound = P.moments_ref(x)
    x64 = x.astype(np.float64)
    assert rec[0] == n and rec.shape == bound.shape == (1 + 2 * W,)
    np.testing.assert_allclose(rec[1:1 + W], np.mean(x64, 0), rtol=1e-14)
    np.testing.assert_allclose(rec[1 + W:] / n, np.var(x64, 0), rtol=1e-9, atol=1e-20)
    assert (bound[1:1 + W] < 1e-11 * rec[1:1 + W]).all() and (bound[1 + W:] <= 1e-9 * np.maximum(rec[1 + W:], 1e-300)).all()
    assert 9990 < x.min() and x.max() < 10010


def test_moment_shapes_cover_the_edges():
    ns, Ws = {n for n, _ in P.MOMENT_SHAPES}, {W for _, W in P.MOMENT_SHAPES}
    assert {1, 63, 64, 65, 1025, 5000} <= ns and {1, 2, 17, 1025} <= Ws
    rems = {(B, n % B) for B, n, _ in P.MB_MOMENT_CASES}
    for B in (255, 256, 257):
        assert {(B, 0), (B, 1), (B, B - 1)} <= rems
    assert (1, 0) in rems and {m for _, _, m in P.MB_MOMENT_CASES} == {True, False}


@pytest.mark.parametrize("c", P.INTEGRATE_CASES, ids=lambda c: c["name"])
def test_integrate_restatement_is_the_pinned_oracle(c):
    """The records of raw groups, merged and integrated in float32, against RunningMeanStd.update on the groups' data."""
    rng = np.random.default_rng(3)
    W = c["W"]
    _, mean, var, count = P.integrate_inputs(c)
    groups = [np.zeros((0, W), F32) if r in c["empty"] else (1.5 * rng.standard_normal((int(rng.integers(3, 60)), W)) + r).astype(F32)
              for r in range(c["R"])]
    recs = np.array([np.concatenate([[0.0], np.full(2 * W, 123.0)]) if len(g) == 0 else P.moments_ref(g)[0] for g in groups])
    m32, v32, n32 = P.integrate_ref(recs, mean, var, count, np.float32)
    m64, v64, n64 = P.integrate_ref(recs, mean, var, count, np.float64)
    if len(c["empty"]) == c["R"]:
        assert np.array_equal(m32, mean) and np.array_equal(v32, var) and n32 == n64 == count
        return
    rs = rso.RunningMeanStd((W,))
    rs.mean, rs.variance, rs.count = mean.copy(), var.copy(), count
    rs.update(None, gathered=[g for g in groups if len(g)])
    close32(m32, rs.mean, "mean"); close32(v32, rs.variance, "variance")
    close32(m64, rs.mean, "mean, float64"); close32(v64, rs.variance, "variance, float64")
    assert n32 == n64 == rs.count and m32.dtype == np.float32 and m64.dtype == np.float64


def test_integrate_cases_cover_the_edges():
    assert {c["R"] for c in P.INTEGRATE_CASES} >= {1, 3, 4} and any(c["W"] == 300 for c in P.INTEGRATE_CASES)
    assert {c["count"] for c in P.INTEGRATE_CASES} == {1e-4, 1e7}
    for c in P.INTEGRATE_CASES:
        recs = P.integrate_inputs(c)[0]
        assert sorted(np.flatnonzero(recs[:, 0] == 0)) == sorted(c["empty"])
    assert any(len(c["empty"]) == 1 and c["R"] in (3, 4) for c in P.INTEGRATE_CASES)
    assert any(len(c["empty"]) == c["R"] for c in P.INTEGRATE_CASES)


@pytest.mark.parametrize("c", P.NORMALIZE_CASES, ids=lambda c: c["name"])
def test_normalize_restatement_is_the_pinned_oracle(c):
    x, mean, var = P.normalize_inputs(c)
    y32, y64 = P.normalize_ref(x, mean, var, None, np.float32), P.normalize_ref(x, mean, var, c["clip"], np.float64)
    close32(y32, rso.normalize(x, mean, var), "normalize", scale=0.0)
    close32(P.denormalize_ref(x, mean, var, np.float32), rso.denormalize(x, mean, var), "denormalize", scale=0.0)
    if c["clip"]:
        raw = P.normalize_ref(x, mean, var, None, np.float64)
        lo, hi = c["clip"]
        assert (raw < lo).any() and (raw > hi).any() and ((raw > lo) & (raw < hi)).any()
        assert (np.minimum(np.abs(raw - lo), np.abs(raw - hi)) > 1e-5 * np.abs(raw)).all(), "a value within rounding of a clip edge"
        assert y64.min() == lo and y64.max() == hi
    assert (var[0] == 0.0) == bool(c.get("var0"))


def test_normalize_cases_cover_the_edges():
    assert {c["W"] for c in P.NORMALIZE_CASES} == {1, 5}
    assert any(c["n"] * c["W"] > 2048 * 256 for c in P.NORMALIZE_CASES)
    for W in (1, 5):
        assert {bool(c["clip"]) for c in P.NORMALIZE_CASES if c["W"] == W} == {True, False}


# ------------------------------------------------------------------------------------------------------------ K6 categorical
@pytest.mark.parametrize("K,n", P.CAT_EVAL_SHAPES)
def test_categorical_restatement_is_the_pinned_oracle(K, n):
    i = P.categorical_inputs(K, n)
    r = P.categorical_eval_ref(i["z"], i["a"], i["d_logp"], i["d_ent"], np.float32)
    z = torch.tensor(i["z"], requires_grad=True)
    lp, ent, probs = plo.categorical_logp_entropy(z, torch.tensor(i["a"]))
    (torch.tensor(i["d_logp"]) * lp + torch.tensor(i["d_ent"]) * ent).sum().backward()
    close32(r["probs"], probs.detach().numpy(), "probs", scale=1e-7)
    close32(r["logp"], lp.detach().numpy(), "logp"); close32(r["ent"], ent.detach().numpy(), "entropy")
    close32(r["d_logits"], z.grad.numpy(), "d_logits")


@pytest.mark.parametrize("K,n", P.CAT_EVAL_SHAPES)
def test_categorical_cases_take_their_branches(K, n):
    i = P.categorical_inputs(K, n)
    r = P.categorical_eval_ref(i["z"], i["a"], i["d_logp"], i["d_ent"], np.float64)
    nrm, kind, rows = r["n"], i["kind"], np.arange(n)
    lo, hi = P.EPS32, 1.0 - P.EPS32
    assert (np.abs(nrm - lo) > 1e-3 * lo).all() and (np.abs(nrm - hi) > 0.5 * P.EPS32).all(), "a probability on a clamp edge"
    hot = kind == P.HOT
    if K > 1 and hot.any():
        assert (nrm[hot, i["hot"][hot]] > hi).all(), "the hot class is not clamped from above"
        others = np.ones((n, K), bool)
        others[rows, i["hot"]] = False
        assert (nrm[hot][others[hot]] < lo).all(), "the other classes are not clamped from below"
        at_hot = i["a"][hot] == i["hot"][hot]
        assert at_hot.any() and (n < 10 or (~at_hot).any())
        only_logp = P.categorical_eval_ref(i["z"], i["a"], i["d_logp"], None, np.float64)["d_logits"]
        assert (only_logp[hot] == 0.0).all(), "a clamped log-prob has a gradient"
    if K == 1:
        assert (nrm == 1.0).all() and (r["d_logits"] == 0.0).all()
    eq = kind == P.EQUAL
    assert np.allclose(nrm[eq], 1.0 / K, rtol=1e-15) and (i["z"][kind == P.SHIFTED] > 9990).all()
    if n >= 255:
        assert (i["a"] == 0).any() and (i["a"] == K - 1).any() and set(np.unique(kind)) == {0, 1, 2, 3}
    assert i["a"].min() >= 0 and i["a"].max() < K


@pytest.mark.parametrize("tag", ["c2", "c5", "c17"])
def test_categorical_restatement_reproduces_g8(golden, tag):
    g = golden("g8_distributions")
    z, a = g[f"{tag}_logits"], g[f"{tag}_actions"].reshape(-1)
    n = len(a)
    lp = P.categorical_eval_ref(z, a, np.ones(n), None, np.float32)
    en = P.categorical_eval_ref(z, a, None, np.ones(n), np.float32)
    np.testing.assert_allclose(lp["probs"], g[f"{tag}_probs"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(lp["logp"], g[f"{tag}_log_probs"].reshape(-1), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(lp["ent"], g[f"{tag}_entropy"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(lp["d_logits"], g[f"{tag}_dlogp_dlogits"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(en["d_logits"], g[f"{tag}_dent_dlogits"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("c", P.CAT_SAMPLE_CASES, ids=lambda c: f"K{c['K']}_n{c['n']}")
def test_categorical_sample_cases(c):
    z = P.categorical_sample_logits(c)
    r64, r32 = P.categorical_sample_ref(z, np.float64), P.categorical_sample_ref(z, np.float32)
    near = hd.near_cdf_edge(z.astype(np.float64), r64["gap"])
    assert near.sum() <= 2, f"{near.sum()} rows near a CDF edge: take another seed"
    assert np.array_equal(r64["a"][~near], r32["a"][~near]), "float32 and float64 decode a kept row differently"
    if c["K"] > 1 and c["n"] > 1:
        assert len(np.unique(r64["a"])) > 1
    assert r64["a"].min() >= 0 and r64["a"].max() < c["K"]
    lp, _, _ = plo.categorical_logp_entropy(torch.tensor(z), torch.tensor(r32["a"]))
    close32(r32["logp"], lp.numpy(), "logp of the drawn class")


def test_sampler_counters_wrap_inside_the_launch():
    assert P.SEED >> 32 and P.OFFSET < 2 ** 32 <= P.OFFSET + 256
    assert {c["K"] for c in P.CAT_SAMPLE_CASES} == {1, 2, 5, 64} and {c["n"] for c in P.CAT_SAMPLE_CASES} == {1, 300}
    assert {D for D, _, _ in P.GAUSS_SAMPLE_CASES} == {1, 3, 4, 5, 8, 9, 64} and {n for _, n, _ in P.GAUSS_SAMPLE_CASES} == {1, 257}
    assert {b for _, _, b in P.GAUSS_SAMPLE_CASES} == {True, False}


# ------------------------------------------------------------------------------------------------------------ K6 Gaussian
@pytest.mark.parametrize("D,n,shift", P.GAUSS_EVAL_SHAPES)
def test_gaussian_restatement_is_the_pinned_oracle(D, n, shift):
    i = P.gaussian_inputs(D, n, shift)
    r = P.gaussian_eval_ref(i["mean"], i["log_std"], i["x"], i["d_logp"], i["d_ent"], np.float32)
    mean, ls, x = torch.tensor(i["mean"], requires_grad=True), torch.tensor(i["log_std"], requires_grad=True), torch.tensor(i["x"])
    lp = plo.gaussian_tanh_logp(mean, ls, x)
    ent = -plo.gaussian_tanh_logp(mean, ls, mean)
    (torch.tensor(i["d_logp"]) * lp + torch.tensor(i["d_ent"]) * ent).sum().backward()
    close32(r["logp"], lp.detach().numpy(), "logp"); close32(r["ent"], ent.detach().numpy(), "entropy")
    close32(r["d_mean"], mean.grad.numpy(), "d_mean")
    close32(r["d_log_std"], ls.grad.numpy(), "d_log_std", scale=1e-5)      # a float32 sum of n cancelling terms, two orders


@pytest.mark.parametrize("D,n,shift", P.GAUSS_EVAL_SHAPES)
def test_gaussian_cases_take_their_branches(D, n, shift):
    i = P.gaussian_inputs(D, n, shift)
    t = {k: v.detach().numpy() for k, v in P.gaussian_terms(i["mean"], i["log_std"], i["x"], np.float64).items()}
    ms, kind, ls = P.c32(P.MIN_STD), i["kind"], i["log_std"]
    floored, ident = ls == -8.0, ls == 25.0
    assert floored[0] and (t["sp"][floored] < 0.1 * ms).all() and (t["sd"][floored] == ms).all()
    assert (t["sp"][~floored] > 10 * ms).all() and (np.abs(ls - 20.0) > 1.0).all(), "a std near the floor, a log_std near the threshold"
    assert D < 2 or (ident[1] and (t["sp"][ident] == 25.0).all())
    assert (np.abs(np.abs(t["l"]) - 100.0) > 1e-2).all() and (np.abs(t["l0"]) < 99.0).all(), "a log-density on the +-100 clamp"
    assert (np.abs(t["tm"] - 1e-6) > 1e-3 * 1e-6).all(), "1 - tanh(mean)^2 on its clamp edge"
    assert (t["tx"][kind == P.X12, D - 1] < 1e-7).all() and (t["l"][kind == P.X60, 0] < -1000.0).all()
    assert (t["tm"][kind == P.MEAN9, D - 1] < 1e-7).all() and (t["tm"][kind != P.MEAN9] > 1e-5).all()
    if n >= 7:
        assert set(np.unique(kind)) == {0, 1, 2, 3}
    else:
        assert kind[0] == (P.X60 if shift == 2 else P.X12)
    r = P.gaussian_eval_ref(i["mean"], i["log_std"], i["x"], i["d_logp"], i["d_ent"], np.float64)
    assert (r["d_log_std"][floored] == 0.0).all() and (r["d_log_std"][~floored] != 0.0).all()
    assert np.allclose(r["d_mean"][kind == P.X60, 0], -i["d_ent"][kind == P.X60] * 2 * np.tanh(i["mean"].astype(np.float64)[kind == P.X60, 0]),
                       rtol=1e-9, atol=0.0), \
        "the clamped log-density has a gradient"


def test_gaussian_shapes_cover_the_edges():
    assert {D for D, _, _ in P.GAUSS_EVAL_SHAPES} == {1, 4, 5, 17, 64} and {n for _, n, _ in P.GAUSS_EVAL_SHAPES} == {1, 1023, 1024, 1025, 2049}


@pytest.mark.parametrize("tag", ["unit", "bounds"])
def test_gaussian_restatement_reproduces_g8(golden, tag):
    g = golden("g8_distributions")
    mean, ls, raw = (g[f"g_{tag}_{k}"] for k in ("mean", "log_std", "raw"))
    n = len(mean)
    lp = P.gaussian_eval_ref(mean, ls, raw, np.ones(n), None, np.float32)
    en = P.gaussian_eval_ref(mean, ls, raw, None, np.ones(n), np.float32)
    np.testing.assert_allclose(lp["logp"], g[f"g_{tag}_log_probs"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(lp["ent"], g[f"g_{tag}_entropy"], rtol=1e-6, atol=1e-6)
    for got, key in ((lp["d_mean"], "dlogp_dmean"), (lp["d_log_std"], "dlogp_dlogstd"), (en["d_mean"], "dent_dmean"),
                     (en["d_log_std"], "dent_dlogstd")):
        np.testing.assert_allclose(got, g[f"g_{tag}_{key}"], rtol=1e-5, atol=1e-6, err_msg=key)
    np.testing.assert_allclose(hd.gauss_std(ls, P.c32(P.MIN_STD), np.float32), g[f"g_{tag}_std"], rtol=1e-6)
    act, _ = hd.squashed_gaussian(mean, hd.gauss_std(ls, P.c32(P.MIN_STD), np.float32), raw, (g[f"g_{tag}_low"], g[f"g_{tag}_high"]), np.float32)
    np.testing.assert_allclose(act, g[f"g_{tag}_refined_sample"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("D,n,bounded", P.GAUSS_SAMPLE_CASES)
def test_gaussian_sample_restatement_is_the_pinned_oracle(D, n, bounded):
    mean, ls, bounds = P.gaussian_sample_inputs(D, n, bounded)
    r32, r64 = P.gaussian_sample_ref(mean, ls, bounds, np.float32), P.gaussian_sample_ref(mean, ls, bounds, np.float64)
    raw = torch.tensor(r32["raw"].astype(F32))
    close32(r32["logp"], plo.gaussian_tanh_logp(torch.tensor(mean), torch.tensor(ls), raw).numpy(), "logp of the drawn action")
    lo, hi = bounds if bounded else (-1.0, 1.0)
    close32(r32["action"], plo.gaussian_refine(raw, lo, hi).numpy(), "action")
    close32(r32["raw"], r64["raw"], "raw", scale=1e-5)
    assert np.isfinite(r64["logp"]).all() and (np.abs(r64["raw"]) < 7.0).all(), "a draw that reaches the tanh clamp"
    if n > 1:
        z = (r64["raw"] - mean) / hd.gauss_std(ls, P.c32(P.MIN_STD), np.float64)
        assert abs(z.mean()) < 0.2 and 0.8 < z.std() < 1.2 and len(np.unique(z)) == z.size, "the draws are not distinct unit normals"


# ------------------------------------------------------------------------------------------------------------ K8
@pytest.mark.parametrize("n,D", P.ICM_SHAPES)
def test_icm_restatement(n, D):
    pred, enc2 = P.icm_inputs(n, D)
    r = P.icm_ref(pred, enc2, np.float32)
    p, e = torch.tensor(pred, requires_grad=True), torch.tensor(enc2, requires_grad=True)
    elem = torch.nn.MSELoss(reduction="none")(p, e)
    f_loss = 0.5 * elem.mean()
    (P.ICM_G * f_loss).backward()
    close32(r["intr"], ((P.ICM_SCALE / 2.0) * elem.sum(-1)).detach().numpy(), "intrinsic reward")
    close32(r["f_loss"], f_loss.item(), "f_loss")
    close32(r["d_pred"], p.grad.numpy(), "d_pred"); close32(r["d_enc2"], e.grad.numpy(), "d_enc2")


def test_icm_shapes_cover_the_edges():
    assert {n for n, _ in P.ICM_SHAPES} >= {1, 3, 4, 5, 1025} and {D for _, D in P.ICM_SHAPES} >= {1, 2, 63, 64, 65, 128, 200}
    assert sum(n * D > 2048 * 256 for n, D in P.ICM_SHAPES) == 1


# ------------------------------------------------------------------------------------------------------------ K9
@pytest.mark.parametrize("c", P.attention_cases(), ids=P.attention_name)
def test_attention_restatement_is_the_pinned_reference(c):
    import test_gpu_kernels as tgk
    q, k, v, dy = P.attention_inputs(c)
    r = P.attention_ref(q, k, v, dy, c["masked"], np.float32)
    qt, kt, vt = (torch.tensor(t, requires_grad=True) for t in (q, k, v))
    y = tgk._attention_ref(qt, kt, vt, c["masked"])
    (y * torch.tensor(dy)).sum().backward()
    close32(r["y"], y.detach().numpy(), "y")
    for name, t in (("dq", qt), ("dk", kt), ("dv", vt)):
        close32(r[name], t.grad.numpy(), name)
    r64 = P.attention_ref(q, k, v, dy, c["masked"], np.float64)
    np.testing.assert_allclose(r64["probs"].sum(-1), 1.0, rtol=1e-12)
    if c["masked"]:
        L = c["L"]
        assert (r64["probs"][:, np.triu_indices(L, 1)[0], np.triu_indices(L, 1)[1]] == 0.0).all() and (r64["probs"][:, 0, 0] == 1.0).all()
    if c["scale"] != 1.0:
        assert (r64["probs"].max(-1) > 0.999).mean() > 0.5, "the scaled case does not saturate the softmax"


def test_attention_cases_cover_the_tiles():
    cs = P.attention_cases()
    assert {c["L"] for c in cs} == set(range(1, 17)) and {c["D"] for c in cs} == {16, 64, 128, 1024}
    idle = set()
    for c in cs[:16]:
        per = 16 // c["L"]
        tiles = -(-c["n_seq"] // per)
        assert tiles > 4 and (per == 1 or c["n_seq"] % per), "no second workgroup, or a full last tile"
        idle.add(4 - tiles % 4)
    assert idle == {1, 2, 3}
    assert {c["masked"] for c in cs} == {True, False} and any(c["scale"] == 8.0 and c["masked"] for c in cs)


# ------------------------------------------------------------------------------------------------------------ K11
@pytest.mark.parametrize("c", P.ADAM_CASES, ids=lambda c: f"n{c['n']}")
def test_adam_restatement_is_torch_adam(c):
    p, g, m, v = P.adam_inputs(c["n"], c["step"])
    max_norm, t = P.adam_max_norm(c["clip"], g, c["scale"]), c["step"] + 1
    r64 = P.adam_ref(p, g, m, v, t, max_norm, c["scale"], np.float64)
    r32 = P.adam_ref(p, g, m, v, t, max_norm, c["scale"], np.float32)
    D = lambda a: torch.tensor(a.astype(np.float64))
    w = torch.nn.Parameter(D(p))
    opt = torch.optim.Adam([w], lr=P.LR, betas=(P.BETA1, P.BETA2), eps=P.ADAM_EPS)
    opt.state[w] = dict(step=torch.tensor(float(c["step"])), exp_avg=D(m), exp_avg_sq=D(v))
    w.grad = D(g) * c["scale"]
    norm = float(torch.nn.utils.clip_grad_norm_([w], max_norm)) if max_norm > 0 else float(w.grad.norm())
    opt.step()
    np.testing.assert_allclose(r64["norm"], norm, rtol=1e-13)
    np.testing.assert_allclose(r64["p"], w.detach().numpy(), rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(r64["m"], opt.state[w]["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(r64["v"], opt.state[w]["exp_avg_sq"].numpy(), rtol=1e-12)
    kp, km, kv = ko.clip_adam(p, g.astype(np.float64) * c["scale"], m, v, (c["step"], c["step"]), P.LR, max_norm, c["n"], eps=P.ADAM_EPS)
    np.testing.assert_allclose(r64["p"], kp, rtol=1e-9, atol=1e-13); np.testing.assert_allclose(r64["v"], kv, rtol=1e-9)
    close32(r32["p"] - p, r64["p"] - p, "step, float32", scale=1e-3)        # |p| / |step|: the step sits in p's last bits
    close32(r32["m"], r64["m"], "m, float32"); close32(r32["v"], r64["v"], "v, float32")
    have = np.sqrt(((g.astype(np.float64) * c["scale"]) ** 2).sum())
    assert {P.CLIP_ON: 0 < max_norm < 0.5 * have, P.CLIP_OFF: max_norm > 2 * have, P.CLIP_NONE: max_norm <= 0}[c["clip"]]


def test_adam_cases_cover_the_edges():
    ns = [c["n"] for c in P.ADAM_CASES]
    assert ns == [1, 2, 3, 4, 5, 1023, 1024, 1025, 65 * 1024 + 3, 2048 * 256 + 5]
    assert (ns[-2] // 4 + 255) // 256 > 64 and (ns[-1] + 255) // 256 > 2048 and {n & 3 for n in ns} == {0, 1, 2, 3}
    assert {c["step"] for c in P.ADAM_CASES} == {0, 6, 100000} and {c["clip"] for c in P.ADAM_CASES} == {P.CLIP_ON, P.CLIP_OFF, P.CLIP_NONE}
    assert {c["scale"] for c in P.ADAM_CASES} == {1.0, 0.125} and {c["norm_out"] for c in P.ADAM_CASES} == {True, False}
    assert P.PRENORMED_PARTIALS == (0, 1, 64, 65, 200)
    sq = 3.7
    r = P.adam_ref(*P.adam_inputs(5, 6), 7, 0.5, 1.0, np.float64, sq=sq)
    assert r["sq"] == sq and r["norm"] == np.sqrt(sq)


# ------------------------------------------------------------------------------------------------------------ sharpness
def test_bounds_reject_planted_errors():
    """The float32 restatement lies inside every bound by construction; the same restatement with one small error planted
    lies outside: Bessel's correction dropped, the clip taken on the wrong side, Philox block 0 again for dimensions 4..7,
    the class tested against the running sum before its own mass, the n & 3 tail dropped from the squared norm."""
    c = next(c for c in P.LOSS_CASES if c["name"] == "B65")
    inp = P.loss_inputs(c)
    r64, r32 = P.loss_ref(inp, c, np.float64), P.loss_ref(inp, c, np.float32)
    assert P.frac(r32["d_logp"], r64["d_logp"], r32["d_logp"]) <= 0.25
    for planted in (dict(adv_std_ddof=0), dict(clip_wrong_side=True)):
        assert P.frac(P.loss_ref(inp, c, np.float32, **planted)["d_logp"], r64["d_logp"], r32["d_logp"]) > 1.0, planted
    mean, ls, _ = P.gaussian_sample_inputs(5, 257, False)
    g64, g32 = P.gaussian_sample_ref(mean, ls, None, np.float64), P.gaussian_sample_ref(mean, ls, None, np.float32)
    z = hd.gauss_normals(P.SEED, P.philox.counters_u64(P.OFFSET, np.arange(257)), 5, np.float32, q1_reuses_q0=True)
    raw = mean + hd.gauss_std(ls, P.c32(P.MIN_STD), np.float32) * z
    assert P.frac(raw[:, :4], g64["raw"][:, :4], g32["raw"][:, :4]) <= 1.0 < P.frac(raw, g64["raw"], g32["raw"])
    sc = next(c for c in P.CAT_SAMPLE_CASES if c["K"] == 5)
    zs = P.categorical_sample_logits(sc)
    a = hd.categorical_draw(zs, P.SEED, P.philox.counters_u64(P.OFFSET, np.arange(len(zs))), np.float32, edge_before_mass=True)[0]
    assert (a != P.categorical_sample_ref(zs, np.float64)["a"]).sum() > 2
    for n in (1, 3, 1025, 65 * 1024 + 3):
        g = P.adam_inputs(n, 0)[1].astype(np.float64)
        sq = (g * g).sum()
        assert abs((g[:n - (n & 3)] ** 2).sum() - sq) > P.f64_sum_bound(n, sq), n
