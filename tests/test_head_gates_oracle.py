"""
No GPU: what tests/test_gpu_head_gates.py rests on.

  1. The discrete heads restated in oracle/k12_oracle.py (_categorical_terms, _bernoulli_terms: torch.distributions' text
     with probs_to_logits' clamp at float32's eps in every dtype) against torch.distributions itself: in float32 -- where
     the two clamps coincide -- on saturated and unsaturated logits, log-prob, entropy and their autograd gradients with
     respect to the logits, per element to 4 ulp of the tensor's largest entry (ULP4; both texts call the same torch
     primitives in the same order, and in fact agree bitwise); a row whose chosen class (bit) lies outside [eps32, 1 - eps32]
     has a log-prob gradient of exactly zero in both.  In float64 on unsaturated logits, where no clamp is reached, old and new
     text agree to 1e-12 relative.
  2. The steering of every GPU case on weights drawn on the CPU for the case's shapes: at least two entries on each side of
     every gate the case names, every kind of row, the float32 census equal to the float64 one, no row left near a gate.
  3. Sharpness: each plant of ko.GatePlants (mat_update_oracle.Planted for K15) run in float32 as "the kernel" and judged
     with ko.deviations against the clean float64 / float32 runs must exceed the bound by MARGIN = 2.5 x in every case that
     names its gate (the clean float32 run reaches 0.25 of the bound at most: the floor is 4 max|x32 - x64|).  The table is
     printed at the module's end.
  4. Two plants NO case can show, and why (test_plants_float32_cannot_show):
       gate_on_chosen_only   the entropy's gate alone.  With the gate dropped, class k's term of d entropy / d n changes by
                             n_k / clamp(n_k): at most 1 where n_k < eps32 or n_k > 1 - eps32, and the softmax backward
                             multiplies it by n_k < eps32, or by 1 - n_k < eps32.  A logit's gradient moves by less than
                             eps32 x entropy_weight / B, against a bound of 1e-5 of the tensor's largest entry, which the
                             unsaturated rows (kind a, which the steering must hold) keep at entropy_weight / B and more.
       softplus_no_identity  sigmoid(x) rounds to exactly 1.0f from x = 17; above 20 "1" and "sigmoid(log_std)" are the same
                             float32 number (1 - sigmoid(25) = 1.4e-11 in float64).
     For these the test asserts what holds: the planted float32 run stays INSIDE the bound in every case.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import k12_oracle as ko

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_gates as hg  # noqa: E402
import lstm_update_cases  # noqa: E402
import mat_update_cases  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
ULP4 = 4.0 * EPS32
MARGIN = 2.5
TABLE = {}                     # (plant, case) -> deviation / bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nsharpness: plant x case -> deviation / bound of the planted float32 run (clean float32: <= 0.25)\n" +
          "\n".join(f"{p:22s} {c:20s} {v:12.3g}" for (p, c), v in sorted(TABLE.items())))


# ------------------------------------------------------------------------------- 1. the restated heads and torch.distributions
def _logits(kind, rows, n, dtype, saturated, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 1.5, (rows, n))
    if saturated:                          # rows of scale 1.5 .. 45: classes below eps32, tops above 1 - eps32, and neither
        z *= np.array([1.0, 4.0, 12.0, 30.0])[np.arange(rows) % 4][:, None]
    return torch.tensor(z, dtype=dtype)


def _old_terms(kind, z, a, slices):
    """(log-prob, entropy) as oracle/k12_oracle.py formed them before: torch.distributions in the run's dtype."""
    if kind == "bernoulli":
        d = torch.distributions.Bernoulli(probs=torch.sigmoid(z), validate_args=False)
        return d.log_prob(a.to(z.dtype)).sum(-1), d.entropy().sum(-1)
    lps, ents, start = [], [], 0
    for j, n in enumerate(slices):
        d = torch.distributions.Categorical(probs=torch.softmax(z[:, start:start + n], dim=-1))
        lps.append(d.log_prob(a[:, j].long()))
        ents.append(d.entropy())
        start += n
    return torch.stack(lps, -1).sum(-1), torch.stack(ents, -1).sum(-1)


def _both(kind, slices, dtype, saturated, seed):
    """{text: (logp, ent, d logp.sum / dz, d ent.sum / dz)} of the old and the new text, the actions, the probabilities."""
    rows, n = 64, sum(slices)
    z0 = _logits(kind, rows, n, dtype, saturated, seed)
    rng = np.random.default_rng(seed + 1)
    p = hg.probabilities(kind, slices if kind == "multi_categorical" else (), z0.double().numpy())
    if kind == "bernoulli":
        a = torch.tensor(rng.integers(0, 2, (rows, n)))
    else:                                  # every other row: the least likely class of each slice
        a = np.stack([rng.integers(0, k, rows) for k in slices], 1)
        start = 0
        for j, k in enumerate(slices):
            a[::2, j] = np.argmin(p[::2, start:start + k], axis=1)
            start += k
        a = torch.tensor(a)
    out = {}
    for text in ("old", "new"):
        z = z0.clone().requires_grad_(True)
        if text == "old":
            lp, en = _old_terms(kind, z, a, slices)
        else:
            acts = a.to(dtype) if kind != "categorical" else a[:, 0].to(dtype)
            lp, en = ko._head_terms(kind, z, None, acts, slices if kind == "multi_categorical" else (), 0.01, {})
        glp, = torch.autograd.grad(lp.sum(), z, retain_graph=True)
        gen, = torch.autograd.grad(en.sum(), z)
        out[text] = tuple(t.detach().double().numpy() for t in (lp, en, glp, gen))
    return out, a.numpy(), p


HEADS = {"categorical": (6,), "multi_categorical": (3, 2, 3), "bernoulli": (5,)}


@pytest.mark.parametrize("saturated", [False, True])
@pytest.mark.parametrize("kind", sorted(HEADS))
def test_restated_heads_are_torch_distributions_in_float32(kind, saturated):
    out, a, p = _both(kind, HEADS[kind], torch.float32, saturated, 11)
    for name, old, new in zip(("log-prob", "entropy", "d log-prob / dz", "d entropy / dz"), out["old"], out["new"]):
        assert np.all(np.isfinite(old)) and np.all(np.isfinite(new))
        err, scale = np.abs(new - old).max(), np.abs(old).max()
        print(f"{kind} saturated={saturated} {name}: max |new - old| {err:.3g} of max {scale:.3g}")
        assert err <= ULP4 * scale, f"{name}: {err:.3g} > 4 ulp of {scale:.3g}"
    if saturated:                          # a closed gate at the chosen class (bit): no gradient from the log-prob, exactly
        inside = (p >= EPS32) & (p <= 1.0 - EPS32)
        r = (1.0 - p) / EPS32              # (float32 rounds p onto 1 - eps32 or 1 here: the near-gate rule's band)
        settled = ~((r >= 0.5) & (r <= 2.0))
        if kind == "bernoulli":
            closed = ~inside & settled
        else:
            closed, start = np.ones(len(p), dtype=bool), 0
            for j, k in enumerate(HEADS[kind]):                     # every slice's chosen class closed: the whole row is zero
                closed &= ~inside[np.arange(len(p)), start + a[:, j]]
                start += k
            closed &= settled.all(axis=1)
        assert closed.sum() >= 2 and (~closed).sum() >= 2
        for text in ("old", "new"):
            assert not out[text][2][closed].any(), f"{text}: log-prob gradient through a closed gate"
            assert out[text][2][~closed].any()


@pytest.mark.parametrize("kind", sorted(HEADS))
def test_restated_heads_keep_the_float64_values_on_unsaturated_logits(kind):
    out, _, p = _both(kind, HEADS[kind], torch.float64, False, 12)
    assert p.min() > 1e3 * EPS32 and p.max() < 1.0 - 1e3 * EPS32
    for name, old, new in zip(("log-prob", "entropy", "d log-prob / dz", "d entropy / dz"), out["old"], out["new"]):
        assert np.abs(new - old).max() <= 1e-12 * np.abs(old).max(), name


def test_float64_clamp_stands_at_float32_eps():
    """What the restatement is for: at a saturated class the float64 reference answers log eps32, as float32 does."""
    z = torch.tensor([[0.0, -40.0, 1.0]], dtype=torch.float64)
    lp, _ = ko._head_terms("categorical", z, None, torch.tensor([1.0], dtype=torch.float64), (), 0.01, {})
    assert abs(lp.item() - np.log(EPS32)) < 1e-12
    lp, _ = ko._head_terms("bernoulli", torch.tensor([[-40.0]], dtype=torch.float64), None,
                           torch.tensor([[1.0]], dtype=torch.float64), (), 0.01, {})
    assert abs(lp.item() - np.log(EPS32)) < 1e-6


# ---------------------------------------------------------------------------------------------- 2. the steering of every GPU case
@functools.lru_cache(maxsize=None)
def k12(name):
    return hg.CpuCase(hg.ALL_K12_CASES[name])


@pytest.mark.parametrize("name", sorted(hg.ALL_K12_CASES))
def test_k12_steering_closes_every_named_gate(name):
    s = k12(name)
    print(name, hg.describe(s.head, s.slices, s.r64, s.actions))
    assert s.census_failures() == []
    ratio = np.exp(s.r64["logp"] - s.mb.old_log_probs)
    assert (ratio < 0.8).any() and (ratio > 1.2).any() and ((ratio > 0.8) & (ratio < 1.2)).any()
    clean = max(f for _, f, _ in ko.deviations(s.r32["grads"], s.r64["grads"], s.r32["grads"], s.tables))
    assert clean <= 0.25 + 1e-12


# ---------------------------------------------------------------------------------------------------------------- 3. sharpness
DISCRETE_PLANTS = ("gate_open",)
GAUSSIAN_PLANTS = ("density_clamp_open", "tanh_clamp_open", "floor_open")
INVISIBLE = {"categorical": "gate_on_chosen_only", "multi_categorical": "gate_on_chosen_only",
             "bernoulli": "gate_on_chosen_only", "gaussian": "softplus_no_identity"}


def _plants_of(head):
    return GAUSSIAN_PLANTS if head == "gaussian" else DISCRETE_PLANTS


def _planted_fraction(s, tables, plant):
    r = s.reference(torch.float32, **{plant: True})
    assert np.array_equal(r["totals"], s.r32["totals"]), "a gate plant changes no forward value"
    return max(f for _, f, _ in ko.deviations(r["grads"], s.r64["grads"], s.r32["grads"], tables))


K12_SHARPNESS = [(p, n) for n, c in sorted(hg.ALL_K12_CASES.items()) for p in _plants_of(c["head"][0])]


@pytest.mark.parametrize("plant,name", K12_SHARPNESS)
def test_k12_planted_gate_misses_the_bound(plant, name):
    s = k12(name)
    TABLE[(plant, name)] = frac = _planted_fraction(s, s.tables, plant)
    assert frac >= MARGIN, f"{plant} in {name}: {frac:.3g} x the bound"


@pytest.mark.parametrize("name", sorted(hg.ALL_K12_CASES))
def test_plants_float32_cannot_show(name):
    s = k12(name)
    plant = INVISIBLE[s.head]
    TABLE[(plant + " (invisible)", name)] = frac = _planted_fraction(s, s.tables, plant)
    assert frac <= 1.0
    if plant == "softplus_no_identity":    # bitwise the clean run
        assert np.array_equal(s.reference(torch.float32, **{plant: True})["grads"], s.r32["grads"])
        assert torch.sigmoid(torch.tensor(20.0)).item() == 1.0


# ----------------------------------------------------------------------------------------------------------- K22 and K15
@functools.lru_cache(maxsize=None)
def k22(name):
    return lstm_update_cases.Steering(lstm_update_cases.GATES_CASES[name])


@functools.lru_cache(maxsize=None)
def k15(name):
    return mat_update_cases.Steering(mat_update_cases.GATES_CASES[name])


@pytest.mark.parametrize("name", sorted(lstm_update_cases.GATES_CASES))
def test_k22_steering_closes_every_named_gate(name):
    s = k22(name)
    print(name, s.census)
    assert s.gates_failures == []
    assert max(f for _, f, _ in ko.deviations(s.r32["grads"], s.r64["grads"], s.r32["grads"], s.tables)) <= 0.25 + 1e-12


@pytest.mark.parametrize("name", sorted(mat_update_cases.GATES_CASES))
def test_k15_steering_closes_the_gate(name):
    s = k15(name)
    assert s.gates_failures() == []
    assert len(s.visible) >= 2
    assert max(f for _, f, _ in s.judge(s.r32["grads"])) <= 0.25 + 1e-12


def _k22_fraction(s, plant):
    r = s.reference(torch.float32, gate_plants=ko.GatePlants(**{plant: True}))
    assert np.array_equal(r["totals"], s.r32["totals"])
    return max(f for _, f, _ in ko.deviations(r["grads"], s.r64["grads"], s.r32["grads"], s.tables))


def _k15_fraction(s, plant):
    r = s.reference(torch.float32, **{plant: True})
    assert np.array_equal(r["totals"], s.r32["totals"])
    return max(f for _, f, _ in s.judge(r["grads"]))


K22_SHARPNESS = [(p, n) for n, c in sorted(lstm_update_cases.GATES_CASES.items()) for p in _plants_of(c["head"][0])]


@pytest.mark.parametrize("plant,name", K22_SHARPNESS)
def test_k22_planted_gate_misses_the_bound(plant, name):
    TABLE[(plant, name)] = frac = _k22_fraction(k22(name), plant)
    assert frac >= MARGIN, f"{plant} in {name}: {frac:.3g} x the bound"


@pytest.mark.parametrize("name", sorted(mat_update_cases.GATES_CASES))
def test_k15_planted_gate_misses_the_bound(name):
    TABLE[("gate_open", name)] = frac = _k15_fraction(k15(name), "gate_open")
    assert frac >= MARGIN, f"gate_open in {name}: {frac:.3g} x the bound"


@pytest.mark.parametrize("name", sorted(lstm_update_cases.GATES_CASES) + sorted(mat_update_cases.GATES_CASES))
def test_plants_float32_cannot_show_k22_k15(name):
    if name in mat_update_cases.GATES_CASES:
        plant, frac = "gate_on_chosen_only", _k15_fraction(k15(name), "gate_on_chosen_only")
    else:
        plant = INVISIBLE[k22(name).head]
        frac = _k22_fraction(k22(name), plant)
    TABLE[(plant + " (invisible)", name)] = frac
    assert frac <= 1.0
