"""
CPU tests of the yardstick of the wide heads, where nobody has used it yet: the float64 restatement of one K6+K7 launch
(tests/helpers/policy_step_cases.py: launch_reference, tests/helpers/head_draws.py) at 18 and 24 classes and at 17 and 24
dimensions, against torch on the CPU in float64 --

  * log-prob: torch.distributions.Categorical(probs = softmax) and the tanh-squashed Normal of the reference
    (networks/distributions.py:441-694: the density per dimension clamped at +-100, 1 - a^2 clamped at 1e-6);
  * entropy: oracle.k12_oracle.minibatch (the reference of tests/test_gpu_k12_gradients.py) at these widths -- its log-prob is
    the launch restatement's, its entropy total Categorical(probs).entropy() and, for the Gaussian head, the reference's
    -log_prob of the mean;
  * refine_prediction: the package's own CategoricalDistribution / GaussianDistribution on CPU tensors (argmax with the
    lowest index on a tie; tanh(mean) rescaled to the bounds) against head_draws.greedy / unit_to_bounds.

The package's log-prob and entropy functions are device kernels (K8, K9) and have no CPU form: torch.distributions stands in
for them here, and tests/test_gpu_wide_heads_step.py compares the kernels themselves.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wide_heads_cases as wh  # noqa: E402

cases = wh.cases
hd = cases.hd


@pytest.mark.parametrize("name", ["cat18_e33_d3_in376", "cat24_sat_e17_d3_in8"])
def test_categorical_restatement_against_torch(name):
    s = wh.steering(name)
    for launch in cases.LAUNCHES:
        r = s.ref[launch][0]
        z = torch.from_numpy(r["logits"])
        assert z.shape[1] in (18, 24)
        p = torch.softmax(z, 1)
        a = torch.from_numpy(np.clip(np.asarray(r["action"]), 0, z.shape[1] - 1))
        eps = float(np.finfo(np.float32).eps)
        want = torch.log(torch.clamp(p / p.sum(1, keepdim=True), eps, 1 - eps)).gather(1, a[:, None])[:, 0]
        np.testing.assert_allclose(r["logp"], want.numpy(), rtol=1e-12, atol=1e-12)
        # where no class is clamped the log-prob is torch.distributions'
        free = (p.min(1).values > 2 * eps).numpy()
        dist = torch.distributions.Categorical(probs=p)
        np.testing.assert_allclose(r["logp"][free], dist.log_prob(a).numpy()[free], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(r["probs"], p.numpy(), rtol=1e-12, atol=1e-300)
    # the draw is a class of the row and the gap is the distance to a CDF edge
    r = s.ref["sampled"][0]
    assert r["drawn"].min() >= 0 and r["drawn"].max() < r["logits"].shape[1] and (r["gap"] >= 0).all()


@pytest.mark.parametrize("name", ["gau17_e33_d3_in376", "gau24_floor_e17_d3_in8"])
def test_gaussian_restatement_against_torch(name):
    s = wh.steering(name)
    O = s.c["O"]
    assert O in (17, 24) and s.bounds is not None
    for launch in cases.LAUNCHES:
        r = s.ref[launch][0]
        mean, raw = torch.from_numpy(r["logits"]), torch.from_numpy(r["raw"])
        sd = torch.clamp(torch.nn.functional.softplus(torch.from_numpy(s.actor.log_std.astype(np.float64))), min=cases.MIN_STD)
        np.testing.assert_allclose(r["sd"], sd.numpy(), rtol=1e-12)
        lp = torch.clamp(torch.distributions.Normal(mean, sd).log_prob(raw), -100.0, 100.0).sum(1)
        a = torch.tanh(raw)
        lp = lp - torch.log(torch.clamp(1 - a * a, min=1e-6)).sum(1)
        np.testing.assert_allclose(r["logp"], lp.numpy(), rtol=1e-10, atol=1e-10)
        lo, hi = (torch.from_numpy(b.astype(np.float64)) for b in s.bounds)
        np.testing.assert_allclose(r["action"], (((a + 1) / 2) * (hi - lo) + lo).numpy(), rtol=1e-12, atol=1e-12)
    if s.c["pm04"]:
        assert np.abs(s.ref["sampled"][0]["action"]).max() <= 0.4 + 1e-12
    # five Philox blocks per row at 17 dimensions, six at 24: the normals of dimension d come from block d // 4
    counters = cases.philox.counters_u64(s.offset, np.arange(s.c["E"]))
    n = hd.gauss_normals(s.seed, counters, O, np.float64)
    n4 = hd.gauss_normals(s.seed, counters, 4, np.float64)
    assert n.shape == (s.c["E"], O) and np.array_equal(n[:, :4], n4)
    assert len(np.unique(np.round(n, 12))) == n.size          # no block drawn twice


def _cat24():
    """24 classes without saturation (cat24_sat_e17_d3_in8 puts classes below eps32, where the clamp bends the entropy)."""
    c = wh.case(17, 8, 3, "tanh", (wh.CAT, 24), 33)
    c["norm_values"] = False
    return cases.Steering(c)


@pytest.mark.parametrize("name", ["cat18_e33_d3_in376", "cat24", "gau17_e33_d3_in376", "gau24_floor_e17_d3_in8"])
def test_k12_reference_logp_and_entropy_at_these_widths(name):
    """oracle.k12_oracle.minibatch -- the reference of tests/test_gpu_k12_gradients.py -- on a case's networks and its sampled
    launch as the mini-batch: its log-prob is the K6+K7 restatement's, its entropy total is torch's own (Categorical(probs)
    .entropy(); Gaussian: the reference's -log_prob of the mean, written out from Normal and the tanh correction), and with
    old log-probs = its log-probs the KL total is zero."""
    from oracle import k12_oracle as ko
    s = _cat24() if name == "cat24" else wh.steering(name)
    r = s.ref["sampled"][0]
    E, O = s.c["E"], s.c["O"]
    rng = np.random.default_rng(7)
    mb = ko.Minibatch(s.obs, s.cobs, r["raw"] if s.head == wh.GAU else r["action"], r["logp"], rng.normal(0, 1, E),
                      rng.normal(0, 1, E))
    consts = ko.Consts(min_std=cases.MIN_STD)
    out = ko.minibatch(s.params(), cases.ko_net(s.actor), cases.ko_net(s.critic), s.head, (), mb, consts)
    np.testing.assert_allclose(out["logp"], r["logp"], rtol=1e-9, atol=1e-9)
    z = torch.from_numpy(r["logits"])
    if s.head == wh.CAT:
        assert z.shape[1] == O and O in (18, 24)
        ent = torch.distributions.Categorical(probs=torch.softmax(z, 1)).entropy()
    else:
        assert O in (17, 24)
        sd = torch.from_numpy(r["sd"])
        lp_mean = torch.clamp(torch.distributions.Normal(z, sd).log_prob(z), -100.0, 100.0).sum(1)
        t = torch.tanh(z)
        ent = -(lp_mean - torch.log(torch.clamp(1 - t * t, min=1e-6)).sum(1))
    totals = dict(zip(ko.SC_NAMES, out["totals"]))
    np.testing.assert_allclose(totals["entropy"], float(ent.mean()), rtol=1e-9, atol=1e-12)
    assert abs(totals["kl"]) < 1e-9
    assert np.isfinite(out["grads"]).all() and np.abs(out["grads"]).max() > 0


def test_refine_prediction_of_the_packages_distributions_on_the_cpu():
    from ppo_and_friends_amd.networks.distributions import CategoricalDistribution, GaussianDistribution
    rng = np.random.default_rng(5)
    for O in (18, 24):
        z = rng.normal(0, 1.5, (40, O))
        z[:, 20 % O] = z[:, 3]                                 # an exact tie in every row
        z[:8, 3] = z[:8, 20 % O] = 9.0                         # ... that wins in the first rows
        want, _ = hd.greedy("categorical", z)
        got = CategoricalDistribution().refine_prediction(torch.from_numpy(z)).numpy()
        assert np.array_equal(got, want) and (got[:8] == min(3, 20 % O)).all()
    for O in (17, 24):
        mean = rng.normal(0, 2.0, (40, O))
        dist = GaussianDistribution(O, distribution_min=-0.4, distribution_max=0.4)
        got = dist.refine_prediction(torch.from_numpy(mean)).numpy()
        bounds = (np.full(O, -0.4, np.float32), np.full(O, 0.4, np.float32))
        np.testing.assert_allclose(got, hd.unit_to_bounds(np.tanh(mean), bounds, np.float64), rtol=1e-6, atol=1e-7)
