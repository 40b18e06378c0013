"""
CPU tests of the float64 K15 mini-batch reference (oracle/mat_update_oracle.py) that tests/test_gpu_mat_update_float64.py
compares the kernels with:

  * pinning: on the first mini-batch of the pinned CPU port (oracle/mat_oracle.CpuMATPPO, itself tied to fixture
    g12_c5_mat by tests/test_oracle_update_golden.py) the reference gives the trace's losses, its actor gradients and the
    critic's total gradient recomputed as test_gpu_mat_wide_obs.py::test_first_minibatch_gradient_matches_the_oracle does;
    the bucket's offsets are the package's (_describe_mat); the hand-written attention backward is autograd's;
  * sharpness: each planted error (mu.Planted) pushes a gradient tensor of at least one GPU-test case outside the bound
    of ko.deviations;
  * the gap, recorded: at the default initialisation, under the rule of the only per-mini-batch gradient test K15 had
    (rtol 1e-5, atol 1e-5 x the bucket's max|g|), the attention errors stay inside the bound;
  * the conditions of every GPU-test case (tests/helpers/mat_update_cases.py), met by construction: no token excluded.
"""
import copy
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from oracle import k12_oracle as ko
from oracle import mat_oracle
from oracle import mat_update_oracle as mu
from oracle import ppo_loss_oracle as plo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mat_update_cases as cases  # noqa: E402


@functools.lru_cache(maxsize=None)
def steering(name):
    return cases.Steering(cases.CASES[name])


def _cfg(g):
    return dict(zip([str(x) for x in g["cfg_names"]], [int(x) for x in g["cfg"]]))


def _bucket(named, grads, table, size):
    out = np.zeros(size)
    at = {n: (o, s) for _, n, o, s in table}
    for (name, p), g in zip(named, grads):
        off, shape = at[name]
        assert tuple(p.shape) == tuple(shape)
        out[off:off + g.numel()] = g.detach().double().numpy().reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------- pinning
def test_float64_reference_reproduces_the_first_minibatch_of_the_pinned_port(golden):
    g = golden("g12_c5_mat")
    c = _cfg(g)
    T, A, O, NA, B = c["T"], c["A"], c["O"], 5, c["batch_size"]
    cpu = mat_oracle.CpuMATPPO(O, NA, A, batch_size=B, seed=0)
    sd = {"actor." + k[len("init_actor."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init_actor.")}
    sd.update({"critic." + k[len("init_critic."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init_critic.")})
    cpu.ac.load_state_dict(sd)
    order = g["slot_orders"][0]
    prev = np.array([int(a[len("agent"):]) for a in g["agent_ids"]])
    cpu.rollout(g["obs_table"][:, :, order], g["reward_table"][:, :, order], g["step_actions"][:T][:, :, order],
                dataset_slot_of=np.argsort(order)[prev])
    perm = g["epoch_perms"][0]
    table, size = mu.bucket_table(A, O, NA)
    named = list(cpu.ac.named_parameters())
    params = _bucket(named, [p for _, p in named], table, size)
    vn0 = (cpu.value_stats.mean, cpu.value_stats.variance, cpu.value_stats.count)
    # ---- the port's own first mini-batch: the trace, and the critic's TOTAL gradient through a copy (float32)
    twin = copy.deepcopy(cpu)
    cpu.trace = []
    cpu.train_epoch(perm)
    tr = cpu.trace[0]
    obs, actions, adv, logp_old, rtg, _ = next(iter(DataLoader(twin.dataset, batch_size=B, sampler=[int(i) for i in perm])))
    mb = mu.Minibatch(obs.numpy(), actions.numpy(), logp_old.numpy(), adv.numpy(), rtg.numpy())
    twin.value_stats.update(rtg.flatten().numpy())
    mean = torch.tensor(twin.value_stats.mean, dtype=torch.float32)
    var = torch.tensor(twin.value_stats.variance, dtype=torch.float32)
    rtg_n = ((rtg.flatten() - mean) / torch.sqrt(var + torch.tensor([1e-8]))).reshape(rtg.shape)
    values, cur_lp, entropy = twin.evaluate(obs, actions)
    r = plo.ppo_minibatch_losses(cur_lp, logp_old, adv, entropy, values, rtg_n, True, twin.surr_clip, twin.entropy_weight, use_huber=True)
    cnamed = [(n, p) for n, p in twin.ac.named_parameters() if n.startswith("critic.")]
    anamed = [(n, p) for n, p in twin.ac.named_parameters() if n.startswith("actor.")]
    share = torch.cat([x.reshape(-1) for x in torch.autograd.grad(r["critic_loss"], [p for _, p in cnamed], retain_graph=True)]).numpy()
    np.testing.assert_allclose(share, tr["critic_grad"], rtol=1e-6, atol=1e-7 * np.abs(tr["critic_grad"]).max(),
                               err_msg="the recomputed mini-batch is not the trace's")
    total_c = torch.autograd.grad(r["actor_loss"] + r["critic_loss"], [p for _, p in cnamed])
    # ---- the new oracle on the same mini-batch
    consts = ko.Consts(True, True, True, 10.0, cpu.surr_clip, cpu.entropy_weight, 0.0)
    r64 = mu.minibatch(params, A, O, NA, mb, consts, vn0)
    r32 = mu.minibatch(params, A, O, NA, mb, consts, vn0, dtype=torch.float32)
    split = lambda flat, nm: [torch.from_numpy(x).reshape(p.shape) for x, (_, p) in
                              zip(np.split(flat, np.cumsum([p.numel() for _, p in nm])[:-1]), nm)]
    trace_actor = _bucket(anamed, split(tr["actor_grad"], anamed), table, size)
    trace_critic = _bucket(cnamed, split(tr["critic_grad"], cnamed), table, size)
    total = trace_actor + _bucket(cnamed, total_c, table, size)
    for what, got, key in (("actor gradients of the trace", trace_actor, "actor_grads"),
                           ("critic-loss share of the trace", trace_critic, "critic_grads"), ("the bucket", total, "grads")):
        bad = ko.failures(got, r64[key], r32[key], table)
        assert not bad, f"{what}: " + "; ".join(bad[:6])
    bad = ko.failures([tr["actor"], tr["critic"], r["surr"], r["kl"]], r64["totals"][[1, 2, 0, 4]], r32["totals"][[1, 2, 0, 4]],
                      [("", "losses", 0, (4,))])
    assert not bad, "; ".join(bad)
    bad = ko.failures(values.detach().numpy(), r64["values"], r32["values"], [("", "values", 0, (B * A,))])
    assert not bad, "; ".join(bad)
    # (the port takes the mini-batch's mean and variance in float32, the oracle from a float64 record)
    np.testing.assert_allclose(r64["vn"], [twin.value_stats.mean, twin.value_stats.variance, twin.value_stats.count], rtol=1e-6)


@pytest.mark.parametrize("shape", [(3, 18, 5), (1, 1, 1), (16, 128, 8), (7, 33, 2)])
def test_bucket_table_is_the_layout_the_driver_describes(shape):
    """The oracle's offsets against fused_update._describe_mat on the package's network (the table K15 checks again)."""
    import mat_float64 as M
    from ppo_and_friends_amd.fused_update import _describe_mat
    A, O, NA = shape
    ac = M.make_network(O, NA, A, 3)
    topo, why = _describe_mat(types.SimpleNamespace(actor_critic=ac, action_dtype="discrete"))
    assert why == "", why
    table, size = mu.bucket_table(A, O, NA)
    assert size == topo["bucket_total"] and [o for _, _, o, _ in table] == list(topo["offsets"])
    assert [(n, tuple(p.shape)) for n, p in ac.named_parameters()] == [(n, s) for _, n, _, s in table]


def test_the_written_out_attention_backward_is_autograds():
    s = steering("dead_7_64_2_5")
    g = s.reference(torch.float64, manual_core=True)["grads"]
    np.testing.assert_allclose(g, s.r64["grads"], rtol=1e-10, atol=1e-13 * np.abs(s.r64["grads"]).max())


@pytest.mark.parametrize("max_norm", [0.3, 50.0])
def test_one_clip_and_one_adam_over_the_bucket_are_torchs(max_norm):
    """mu.clip_adam from a non-zero state (step 6) against nn.utils.clip_grad_norm_ + torch.optim.Adam on ONE parameter that
    holds the whole bucket (mat_policy.py:677-699), clip active and inactive."""
    rng = np.random.default_rng(5)
    n = 203
    p0, g, m0, v0 = rng.normal(0, 1, n), rng.normal(0, 0.3, n), rng.normal(0, 0.1, n), rng.uniform(0.01, 0.2, n)
    w = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([w], lr=cases.LR, eps=1e-5)
    opt.state[w] = dict(step=torch.tensor(6.0), exp_avg=torch.tensor(m0), exp_avg_sq=torch.tensor(v0))
    w.grad = torch.tensor(g)
    norm = float(torch.nn.utils.clip_grad_norm_([w], max_norm))
    opt.step()
    p, m, v, got_norm = mu.clip_adam(p0, g, m0, v0, 6, cases.LR, max_norm)
    assert (norm > max_norm) == (max_norm < 1.0)
    np.testing.assert_allclose(got_norm, norm, rtol=1e-12)
    np.testing.assert_allclose(p - p0, w.detach().numpy() - p0, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(m, opt.state[w]["exp_avg"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(v, opt.state[w]["exp_avg_sq"].numpy(), rtol=1e-12)
    assert int(opt.state[w]["step"]) == 7


# ---------------------------------------------------------------------------------------------------- sharpness
PLANTED = {
    "the softmax backward loses its row-sum term": dict(softmax_no_rowsum=True),
    "the 1/sqrt(64) scale is missing in the backward only": dict(bwd_no_scale=True),
    "the causal mask is missing in attn2": dict(attn2_unmasked=True),
    "dK is taken from the unmasked probabilities": dict(dk_unmasked=True),
    "the action one-hot is shifted by one agent": dict(onehot_shift=True),
    "the start token is missing": dict(no_start_token=True),
    "LayerNorm eps 1e-6": dict(ln_eps=1e-6),
    "a LayerNorm gain applied before the normalisation": dict(ln_gain_first=True),
    "tanh-GELU instead of erf-GELU": dict(tanh_gelu=True),
    "the biased advantage std": dict(adv_std_ddof=0),
    "the loss mean over 16-row tiles instead of B A tokens": dict(tile_mean=True),
}
# accepted by the bucket-wide rule at the default initialisation (test_default_initialisation_hides_...).  Of the four
# attention errors the missing causal mask of attn2 is NOT among them: it changes the forward pass, and its 1.6e-5 on the
# attention's value / projection gradients is 8 x that rule's atol
HIDDEN_AT_DEFAULT = [e for e in PLANTED if "softmax" in e or "scale" in e or "dK" in e or "eps" in e]


def _outside(s, planted):
    """The tensors of the planted float64 gradient outside the GPU test's bound for the case."""
    g = s.reference(torch.float64, **planted)["grads"]
    return [n for n, f, _ in s.judge(g) if not f <= 1.0]


@pytest.mark.parametrize("error", list(PLANTED))
def test_a_gpu_test_case_catches_every_planted_error(error):
    """float64-correct against float64-planted under the GPU test's own judgement (judge_gradient: ko.deviations with the
    float32 floor), over every case; the cases that catch it are printed."""
    caught = []
    for name in cases.CASES:
        s = steering(name)
        assert not _outside(s, {}) and not [n for n, f, _ in s.judge(s.r32["grads"]) if not f <= 1.0], "the references themselves must pass"
        if _outside(s, PLANTED[error]):
            caught.append(name)
    print(f"{error}: caught by {len(caught)} of {len(cases.CASES)} cases" + (f" ({', '.join(caught)})" if len(caught) < 8 else ""))
    assert caught, f"planted error accepted by every case: {error}"


# ---------------------------------------------------------------------------------------------------- the gap, recorded
def test_default_initialisation_hides_the_attention_errors_from_the_bucket_wide_rule():
    """Why the cases overwrite the weights.  (A, O, NA) = (3, 18, 5), B = 32, the network's default initialisation
    (orthogonal gains of 0.01 on every attention linear, zero biases, identity LayerNorms), one random mini-batch, Huber:
    under rtol 1e-5, atol 1e-5 x the bucket's max|g| -- the rule of test_first_minibatch_gradient_matches_the_oracle --
    the errors of HIDDEN_AT_DEFAULT are ACCEPTED (three of the four attention errors and the LayerNorm eps; the missing
    mask of attn2 is caught there), and more than 25 of the 63 tensors lie below 1e-3 of the bucket's largest entry.
    (Which of the other planted errors that rule accepts there is printed, not asserted.)"""
    A, O, NA, B = 3, 18, 5, 32
    torch.manual_seed(0)
    net = mat_oracle.MATActorCritic(O, NA, A)
    table, size = mu.bucket_table(A, O, NA)
    named = list(net.named_parameters())
    params = _bucket(named, [p for _, p in named], table, size)
    rng = np.random.default_rng(0)
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    mb = mu.Minibatch(f32(rng.normal(0, 1, (B, A, O))), rng.integers(0, NA, (B, A)), np.zeros((B, A), np.float32),
                      f32(rng.normal(0, 1, (B, A))), f32(rng.normal(0, 1, (B, A))))
    consts = ko.Consts(True, True, True, 10.0, 0.2, 0.01, 0.0)
    logp = mu.minibatch(params, A, O, NA, mb, consts)["logp"].reshape(-1)
    mb = mb._replace(old_log_probs=ko.steered_old_log_probs(logp, rng).reshape(B, A))
    g64 = mu.minibatch(params, A, O, NA, mb, consts)["grads"]
    scale = np.abs(g64).max()
    small = [n for _, n, o, sh in table if np.abs(g64[o:o + int(np.prod(sh))]).max() < 1e-3 * scale]
    print(f"default initialisation: {len(small)} of {len(table)} tensors below 1e-3 of the bucket's max|g| {scale:.3g}")
    assert len(small) >= 25
    verdict = {}
    for error, kw in PLANTED.items():
        g = mu.minibatch(params, A, O, NA, mb, consts, planted=mu.Planted(**kw))["grads"]
        verdict[error] = bool(np.abs(g - g64).max() > 0) and np.allclose(g, g64, rtol=1e-5, atol=1e-5 * scale)
        print(f"  {error}: {'ACCEPTED' if verdict[error] else 'caught'} by the bucket-wide rule (max |dg| {np.abs(g - g64).max():.3g})")
    assert [e for e in HIDDEN_AT_DEFAULT if not verdict[e]] == []


# ---------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_meets_its_conditions_by_construction(name):
    s = steering(name)
    c, (A, O, NA, B) = s.c, s.shape
    g, zero = s.r64["grads"], s.zero()
    scale = np.abs(g).max()
    assert not g[s.pad].any()
    # every tensor on the bucket's scale, but the analytically zero ones -- which are what the float64 oracle says
    round_off = s.round_off()
    assert set(cases.KEY_BIAS) <= set(round_off) | zero and not set(round_off) & zero
    for _, n, o, sh in s.table:
        m = np.abs(g[o:o + int(np.prod(sh))]).max()
        if n in zero:
            assert m == 0.0, f"{n}: listed as exactly zero, float64 gives {m:.3g}"
        elif n in round_off:
            assert m <= 1e-12 * scale, f"{n}: {m / scale:.3g} of the bucket's max (zero in exact arithmetic)"
        else:
            assert m >= 1e-4 * scale, f"{n}: max|g| {m / scale:.3g} of the bucket's largest entry"
    # parameters: every bias non-zero, every LayerNorm affine
    for _, n, o, sh in s.table:
        v = s.params[o:o + int(np.prod(sh))]
        assert (v != 0).all() and (len(sh) == 2 or n.endswith(".bias") or (np.abs(v - 1.0) <= 0.3 + 1e-6).all()), n
        assert len(sh) == 2 or n.endswith(".bias") or np.abs(v - 1.0).max() > 0.0 or v.size == 0, n
    # the surrogate's clip: no ratio near an edge, clipped and unclipped tokens, both signs of the advantage
    for mb, r64 in ((s.mb, s.r64),) + (((s.mb1, None),) if s.mb1 is not None else ()):
        if r64 is None:
            p1 = mu.clip_adam(s.params, g, s.m0, s.v0, cases.STEP0, cases.LR, s.max_norms[-1])[0].astype(np.float32).astype(np.float64)
            r64 = s.reference(torch.float64, mb=mb, params=p1, vn=s.r64["vn"] if c["norm_values"] else s.vn)
        ratio = np.exp(r64["logp"] - mb.old_log_probs).reshape(-1)
        assert np.abs(ratio - 0.8).min() >= 1e-3 and np.abs(ratio - 1.2).min() >= 1e-3
        a = np.float64(mb.advantages).reshape(-1)
        if c["norm_adv"]:
            a = (a - a.mean()) / (a.std(ddof=1) + 1e-8)
        clipped = ((ratio > 1.2) & (a > 0)) | ((ratio < 0.8) & (a < 0))
        assert clipped.any() and (~clipped).any(), "clipped and unclipped tokens"
        assert (a > 0).any() and (a < 0).any(), "both signs of the advantage"
        d = np.abs(r64["values"] - r64["rtg"]).reshape(-1)
        assert np.abs(d - 10.0).min() > 1e-3, "no |v - rtg| near Huber's delta"
        assert (d > 10.0).any() and (d < 10.0).any(), "both branches of the Huber loss"
        # the clamp K15 restates (float32 eps, stated in the oracle): out of reach wherever there is a choice
        if NA > 1:
            assert r64["probs"].min() > 1e-5 and r64["probs"].max() < 1.0 - 1e-5
        else:
            assert (r64["probs"] == 1.0).all() and np.allclose(r64["logp"], np.log(1.0 - mu.EPS32), rtol=1e-12)
        # no kink anywhere (GELU, tanh-free heads): the share of the mini-batch left out of a comparison is zero
        assert mb.obs.shape[:2] == mb.raw_actions.shape == mb.old_log_probs.shape == r64["values"].shape
    assert len(s.mb.obs) == B and (s.mb1 is None or 2 <= len(s.mb1.obs) < B or B == 2)
    # the key and query linears give scores of O(1) spread: no softmax of the case is the uniform one of the default weights
    if A > 1:
        net = mu.network(A, O, NA, s.params)
        kept = {}
        for n, m in net.named_modules():
            if n.endswith("key_net") or n.endswith("query_net"):
                m.register_forward_hook(lambda mod, args, out, n=n: kept.__setitem__(n, out.detach()))
        net(torch.as_tensor(s.mb.obs, dtype=torch.float64), mu.action_block(s.mb.raw_actions, A, NA))
        for att in cases.ATTENTIONS:
            scores = kept[att + ".query_net"] @ kept[att + ".key_net"].transpose(-2, -1) / 8.0
            assert 0.3 < float(scores.std()) < 5.0, f"{att}: scores of spread {float(scores.std()):.3g}"
    assert s.max_norms[0] < np.sqrt((g * g).sum()) < s.max_norms[1]
