"""
CPU tests of the chain oracle (oracle/epoch_oracle.py) that tests/test_gpu_epoch_float64.py compares whole fused update
epochs with, and of that test's cases (tests/helpers/epoch_cases.py):

  * PIN: the chain in float32 reproduces the first epoch of the pinned port (cpu_ppo_loop.CpuPPO.train_epoch) on fixture
    g12_c2_cut -- four mini-batches of 64 rows and a tail of 8, from the fixture's initial weights with Adam's state zero:
    every mini-batch's losses and raw gradients, the weights, the normaliser, the `values` column and the epoch's
    statistics, within the tolerances tests/test_oracle_update_golden.py holds that port to; and the statistics the
    reference itself recorded for that epoch;
  * CONDITIONS on every case, on the reference alone: (a) the float32 chain stays within 2.5 x 2e-5 max|x64| of the float64
    chain in every compared tensor, so the raised bound is at most 10 x the unraised rule; (b) the chain reaches what it is
    meant to reach -- a clipped and an unclipped optimiser step per network, ratios on both sides of both clip edges, a row
    on Huber's linear branch -- and no row is left near a branch edge;
  * SHARPNESS: every planted error of the chain exceeds the bound of the GPU test by at least 2.5 x in every case that
    claims to reject it, and every planted error is claimed by some case.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ppo_loop
from oracle import epoch_oracle as eo
from oracle import k12_oracle as ko

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import epoch_cases as ec  # noqa: E402
import test_k12_oracle as tko  # noqa: E402
import test_oracle_update_golden as tug  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ pin
def _unpadded(tables, x, tag):
    return np.concatenate([x[o:o + int(np.prod(s))] for t, _, o, s in tables if t == tag])


def test_float32_chain_reproduces_the_first_epoch_of_the_pinned_port(golden):
    name = "g12_c2_cut"
    g = golden(name)
    c = tug._cfg(g)
    c["name"] = name
    B, N = c["batch_size"], len(g["it0_ds_observations"])
    assert N // B == 4 and N % B == 8                                      # four mini-batches and a tail
    perm = np.asarray(g["epoch_perms"][0])
    # ---- the pinned port on the fixture's dataset, shuffle and initial weights
    cpu = tug.build_cpu_port(g, c)
    ds = object.__new__(cpu_ppo_loop._ListDataset)
    T = lambda k, dtype=torch.float32: torch.tensor(np.asarray(g["it0_ds_" + k]), dtype=dtype)
    ds.observations, ds.next_observations = T("observations"), T("next_observations")
    ds.critic_observations = T("critic_observations")
    ds.actions, ds.raw_actions = T("actions", torch.long), T("raw_actions", torch.long)
    ds.rewards_to_go, ds.advantages, ds.values = T("rewards_to_go"), T("advantages"), T("values")
    ds.log_probs = T("log_probs").reshape(-1, 1)
    ds.empty = np.zeros(N).astype(np.uint8)
    cpu.dataset, cpu.trace = ds, []
    stats = cpu.train_epoch(perm=perm)
    # ---- the chain in float32
    act = tko.FIXTURES[name]
    actor, sa = tko._fixture_net(g, "init_actor", act)
    critic, sc = tko._fixture_net(g, "init_critic", act)
    params = np.concatenate([sa, sc])
    chain = eo.K12Chain(actor, critic, "categorical", (), ko.Consts(), B, 3e-4, 0.5)
    data = ko.Minibatch(*[np.asarray(g["it0_ds_" + k]) for k in ("observations", "critic_observations", "raw_actions",
                                                                  "log_probs", "advantages", "rewards_to_go")])
    zero = np.zeros_like(params)
    start = eo.State(params, zero, zero, (0, 0), (0.0, 1.0, 1e-4), np.asarray(g["it0_ds_values"]))
    ep = eo.k12_epochs(chain, data, [perm], start, dtype=torch.float32)[0]
    tables, _ = ko.bucket_tables(actor, critic, "categorical")
    # every mini-batch, the tail included: losses and raw gradients
    assert ep["n_done"] == len(ep["steps"]) == len(cpu.trace) == 5 and len(ep["steps"][-1]["rows"]) == 8
    for k, (s, m) in enumerate(zip(ep["steps"], cpu.trace)):
        np.testing.assert_array_equal(s["rows"], perm[k * B:(k + 1) * B])
        np.testing.assert_allclose(s["totals"][1:3], [m["actor"], m["critic"]], rtol=1e-5, atol=1e-7, err_msg=f"mini-batch {k}")
        np.testing.assert_allclose(s["totals"][3:7], [m["entropy"], m["kl"], m["adv_mean"], m["adv_std"]], rtol=1e-5, atol=1e-7)
        for tag in ("actor", "critic"):
            np.testing.assert_allclose(_unpadded(tables, s["grads"], tag), m[tag + "_grad"], rtol=1e-5, atol=1e-7,
                                       err_msg=f"mini-batch {k} {tag}")
    # the state the epoch leaves
    st = ep["state"]
    np.testing.assert_allclose(_unpadded(tables, st.params, "actor"), tug._flat(cpu.actor), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(_unpadded(tables, st.params, "critic"), tug._flat(cpu.critic), rtol=1e-5, atol=1e-7)
    for tag, opt, net in (("actor", cpu.actor_optim, cpu.actor), ("critic", cpu.critic_optim, cpu.critic)):
        for key, mine in (("exp_avg", st.m), ("exp_avg_sq", st.v)):
            want = torch.cat([opt.state[p][key].reshape(-1) for p in net.parameters()]).numpy()
            np.testing.assert_allclose(_unpadded(tables, mine, tag), want, rtol=1e-5, atol=1e-7 * np.abs(want).max(), err_msg=key)
        assert {int(opt.state[p]["step"]) for p in net.parameters()} == {5}
    assert st.steps == (5, 5)
    vs = cpu.value_stats
    np.testing.assert_allclose(st.vn, [vs.mean, vs.variance, vs.count], rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(st.values, ds.values.numpy(), rtol=1e-5, atol=1e-6)
    # the epoch's statistics: the port's, and what the reference recorded (actor loss, critic loss, kl avg, weighted entropy)
    t = ep["totals"]
    assert t[8] == 5.0
    mine = np.array([t[0] / t[8], t[2] / t[8], t[4] / t[8], t[3] * 0.01 / t[8]])
    np.testing.assert_allclose(mine, [stats["actor loss"], stats["critic loss"], stats["kl avg"], stats["weighted entropy"]],
                               rtol=5e-6, atol=1e-6)
    np.testing.assert_allclose(mine, g["epoch_stats"][0], rtol=5e-6, atol=1e-6)


def test_a_one_row_tail_reaches_the_normaliser_and_nothing_else():
    """Q9 in the chain against the pinned running statistics: N = 2 B + 1."""
    from oracle.running_stats_oracle import RunningMeanStd
    s = ec.built("three_launches")
    B, perm = s.c["B"], s.perms[0]
    assert len(perm) % B == 1
    ep = s.e64[0]
    assert ep["n_done"] == len(perm) // B and ep["totals"][8] == ep["n_done"]
    rs = RunningMeanStd()
    rs.mean, rs.variance, rs.count = np.float64(ec.VN[0]), np.float64(ec.VN[1]), ec.VN[2]
    rtg = s.rtg().astype(np.float64)
    for k in range(len(perm) // B + 1):
        rs.update(rtg[perm[k * B:(k + 1) * B]])
    np.testing.assert_allclose(ep["state"].vn, [rs.mean, rs.variance, rs.count], rtol=1e-10)
    last = perm[-1]
    assert ep["state"].values[last] == np.float64(s.values0[last])         # the skipped row keeps its value
    assert ep["state"].steps == tuple(x + ep["n_done"] for x in ec.STEPS0)


# ----------------------------------------------------------------------------------------------------------- conditions
def test_cases_cover_the_mechanics():
    cs = list(ec.K12_CASES.values())
    assert {c["form"] for c in cs} == {"chain", "three_launches", "slabs", "row_tiles"}
    assert {c["graphs"] for c in cs if c["form"] == "chain" and c["ha"] == 64} == {True, False}
    assert {(c["ha"], c["hc"]) for c in cs} >= {(64, 64), (256, 256), (32, 256), (256, 512), (128, 128)}
    assert {c["head"][0] for c in cs} == set(ko.HEADS) and {c["act"] for c in cs} == set(ko.ACTIVATIONS)
    assert {c["tail"] if c["tail"] < 3 else c["tail"] - c["B"] for c in cs} == {0, 1, 2, -1}
    assert any(not c["norm_values"] for c in cs) and any(not c["norm_adv"] for c in cs)
    assert any(not c["huber"] and c["kl"] > 0 and c["ent"] == 0 for c in cs)
    assert any(c["lean"] == 1 and c["depth"] == 3 and c["ha"] == 128 and c["head"] == ("categorical", 2) for c in cs)
    for c in cs:
        assert 16 <= c["B"] <= 48 and 5 <= c["n_full"] <= 7 and c["chunk"] in (2, 3)
        # a warm-up chunk and at least one replay in the first epoch
        assert c["n_full"] >= 2 * c["chunk"]
    # an eager remainder behind the replays somewhere, and none somewhere
    assert {c["n_full"] % c["chunk"] > 0 for c in cs} == {True, False}
    claimed = {p for c in ec.CASES.values() for p in c["plants"]}
    assert claimed == set(eo.PLANTS), set(eo.PLANTS) - claimed


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_case_conditions(name):
    s = ec.built(name)
    assert not s.problems, f"{name} (seeds tried: {s.tried}): " + "; ".join(s.problems)
    # (a) the float32 floor under its cap, tensor by tensor
    worst = max(s.floor, key=s.floor.get)
    assert s.floor[worst] <= 1.0, f"{worst}: float32 floor at {s.floor[worst]:.3g} of its cap"
    # (b) the branches, and no row left near an edge
    assert not s.branch_problems(s.e64)
    bad, _, closed = s.near(s.e64)
    assert not bad.any() and not closed
    for e, ep in enumerate(s.e64):
        assert ep["n_done"] == s.c["n_full"] + (s.c["tail"] >= 2)
    # the comparison accepts both clean chains
    ask = lambda eps: [d for d in s.deviations(eps) if not d[3] <= 1.0]
    assert not ask(s.e64) and not ask(s.e32)


# ------------------------------------------------------------------------------------------------------------ sharpness
@pytest.mark.parametrize("name,plant", [(n, p) for n in sorted(ec.CASES) for p in ec.CASES[n]["plants"]])
def test_comparison_rejects_the_planted_error(name, plant):
    s = ec.built(name)
    devs = s.deviations(s.run(**{plant: True}))
    e, what, tensor, frac = max(devs, key=lambda d: d[3])
    assert frac >= ec.MARGIN, f"{plant} in {name}: at most {frac:.3g} x the bound (epoch {e} {what} {tensor})"
