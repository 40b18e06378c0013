"""
CPU tests of the float64 K22 mini-batch reference (oracle/lstm_update_oracle.py) that tests/test_gpu_lstm_update_float64.py
compares the kernels with:

  * pinning: on the first mini-batch of the pinned CPU port (oracle/lstm_oracle.CpuLSTMPPO, itself tied to fixtures
    g12_lstm_term / g12_lstm_cut by tests/test_oracle_update_golden.py) the reference gives the port's per-tensor
    gradients, losses and final (h, c); a Gaussian-head, Tanh, depth-2 network against one assembled from torch.nn;
  * sharpness: each planted error (actor rows zeroed from the terminal position on, critic rows zeroed as well, (h0, c0)
    from the window's first position, the b_hh gradient dropped, LayerNorm eps 1e-6, the biased advantage std) pushes a
    gradient tensor of at least one GPU-test case outside the bound of ko.deviations;
  * kink budget: every GPU-test case finds its B un-kinked items, with every kind of terminal window among them.
"""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import k12_oracle as ko
from oracle import lstm_oracle
from oracle import lstm_update_oracle as lo
from oracle import ppo_loss_oracle as plo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_update_cases as cases  # noqa: E402


@functools.lru_cache(maxsize=None)
def steering(name):
    return cases.Steering(cases.CASES[name])


def _cfg(g):
    return dict(zip([str(x) for x in g["cfg_names"]], [int(x) for x in g["cfg"]]))


def _bucket(actor_params, critic_params, tables, size):
    out = np.zeros(size)
    for (_, _, off, shape), p in zip(tables, list(actor_params) + list(critic_params)):
        assert tuple(p.shape) == tuple(shape)
        out[off:off + p.numel()] = p.detach().double().numpy().reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------- pinning
@pytest.mark.parametrize("name,S,n_act", [("g12_lstm_term", 4, 2), ("g12_lstm_cut", 3, 3)])
def test_float64_reference_reproduces_the_first_minibatch_of_the_pinned_port(golden, name, S, n_act):
    g = golden(name)
    c = _cfg(g)
    T, B = c["T"], c["batch_size"]
    cpu = lstm_oracle.CpuLSTMPPO(c["O"], n_act, sequence_length=S, lstm_hidden=32, ff_hidden=32, batch_size=B, seed=0,
                                 rtg_accum="float32")
    for net, tag in ((cpu.actor, "init_actor."), (cpu.critic, "init_critic.")):
        net.load_state_dict({k[len(tag):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag)})
    term = g["term_table"]
    ds = cpu.rollout(g["obs_table"][:, :, 0], g["reward_table"][:, :, 0], g["step_actions"][:T, :, 0],
                     term_table=term if term.any() else None, max_ts_per_ep=c["max_ts_per_ep"])
    # ---- the port's own first mini-batch: float32 autograd through copies of its networks (train_epoch's steps)
    batch = next(iter(cpu._loader(g["epoch_perms"][0] - (S - 1))))
    critic_obs, obs, raw_actions, advantages, log_probs, rewards_tg, a_h, c_h, a_c, c_c, idxs = batch
    actor, critic = copy.deepcopy(cpu.actor), copy.deepcopy(cpu.critic)
    rtg_n = cpu._norm_update(rewards_tg.flatten()).reshape(rewards_tg.shape)
    actor.hidden_state = (torch.transpose(a_h, 0, 1).contiguous(), torch.transpose(a_c, 0, 1).contiguous())
    critic.hidden_state = (torch.transpose(c_h, 0, 1).contiguous(), torch.transpose(c_c, 0, 1).contiguous())
    values = critic(critic_obs).squeeze()
    dist = torch.distributions.Categorical(torch.softmax(actor(obs), dim=-1))
    cur_lp = torch.unsqueeze(dist.log_prob(raw_actions.flatten()), dim=-1)
    r = plo.ppo_minibatch_losses(cur_lp, log_probs, advantages, dist.entropy(), values, rtg_n, cpu.normalize_adv,
                                 cpu.surr_clip, cpu.entropy_weight)
    ga = torch.autograd.grad(r["actor_loss"], list(actor.parameters()))
    gc = torch.autograd.grad(r["critic_loss"], list(critic.parameters()))
    # ---- the same mini-batch for the new oracle: unmasked windows + terminal bytes, states of the last position
    na_net = lo.Net(c["O"], 32, 32, 1, n_act, "relu")
    nc_net = lo.Net(c["O"], 32, 32, 1, 1, "relu")
    tables, size = lo.bucket_tables(na_net, nc_net, "categorical")
    params = _bucket(cpu.actor.parameters(), cpu.critic.parameters(), tables, size)
    term_pos = np.zeros(len(ds.observations), dtype=bool)
    cur = 0
    for ep in ds.episodes:
        cur += ep.length
        term_pos[cur - 1] = ep.terminal
    last = idxs.numpy()
    pos = (last - (S - 1))[:, None] + np.arange(S)[None, :]
    st = lambda t: t[last][:, 0].numpy()
    mb = lo.Minibatch(ds.observations.numpy()[pos], ds.critic_observations.numpy()[pos], term_pos[pos], st(ds.actor_hidden),
                      st(ds.actor_cell), st(ds.critic_hidden), st(ds.critic_cell), ds.raw_actions.numpy()[last].reshape(-1),
                      ds.log_probs.numpy()[last].reshape(-1), ds.advantages.numpy()[last], ds.rewards_to_go.numpy()[last])
    assert np.array_equal(np.where(lo.window_mask(mb.terminal)[:, :, None], 0.0, mb.obs), obs.numpy()), "window masks"
    if name == "g12_lstm_term":
        assert lo.window_mask(mb.terminal).any(), "the fixture's first mini-batch holds a masked window"
    consts = ko.Consts(cpu.normalize_adv, cpu.normalize_values, False, 10.0, cpu.surr_clip, cpu.entropy_weight, 0.0)
    r64 = lo.minibatch(params, na_net, nc_net, "categorical", mb, consts)
    r32 = lo.minibatch(params, na_net, nc_net, "categorical", mb, consts, dtype=torch.float32)
    bad = ko.failures(_bucket(ga, gc, tables, size), r64["grads"], r32["grads"], tables)
    assert not bad, "; ".join(bad)
    pick = [0, 1, 2, 4]                                   # surrogate, actor loss, critic loss, KL
    bad = ko.failures([r["surr"], r["actor"], r["critic"], r["kl"]], r64["totals"][pick], r32["totals"][pick],
                      [("", "losses", 0, (4,))])
    assert not bad, "; ".join(bad)
    for key, got in (("actor_h", actor.hidden_state[0]), ("actor_c", actor.hidden_state[1]),
                     ("critic_h", critic.hidden_state[0]), ("critic_c", critic.hidden_state[1])):
        bad = ko.failures(got[0].detach().numpy(), r64[key], r32[key], [("", key, 0, (r64[key].size,))])
        assert not bad, "; ".join(bad)
    bad = ko.failures(values.detach().numpy(), r64["values"], r32["values"], [("", "values", 0, (len(last),))])
    assert not bad, "; ".join(bad)


def test_gaussian_tanh_depth2_against_a_network_of_torch_modules():
    """The bucket layout, the Gaussian head with log_std behind the actor's last bias, Tanh and two hidden layers, with
    unequal actor / critic widths: against nn.LSTM / LayerNorm / Linear assembled here, in float64."""
    s = cases.Steering(cases.case(I=6, H=32, F=16, depth=2, S=4, B=12, head=("gaussian", 3), act="tanh", agents=2, seed=5))
    tab = {(t, n): (o, sh) for t, n, o, sh in s.tables}
    P = lambda tag, name: torch.tensor(s.params[tab[tag, name][0]:tab[tag, name][0] + int(np.prod(tab[tag, name][1]))]
                                       .reshape(tab[tag, name][1]), dtype=torch.float64, requires_grad=True)
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    mb = s.mb
    mask = torch.as_tensor(lo.window_mask(mb.terminal))
    assert mask.any()

    def run(tag, net, x, h0, c0):
        lstm, ln = nn.LSTM(net.in_dim, net.hidden, 1).double(), nn.LayerNorm(net.hidden).double()
        ps = {n: P(tag, n) for (t, n) in tab if t == tag}
        w = [ps["w_ih"], ps["w_hh"], ps["b_ih"], ps["b_hh"]]
        _, (h, cc) = torch.func.functional_call(lstm, dict(zip(["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"], w)),
                                                (x.transpose(0, 1), (T(h0)[None], T(c0)[None])))
        y = torch.tanh(nn.functional.layer_norm(h[-1], (net.hidden,), ps["ln_w"], ps["ln_b"], 1e-5))
        for l in range(3):
            y = nn.functional.linear(y, ps[f"ff{l}.weight"], ps[f"ff{l}.bias"])
            y = torch.tanh(y) if l < 2 else y
        return y, h[-1], cc[-1], ps

    mean, ah, ac, pa = run("actor", s.actor, T(mb.obs).masked_fill(mask[:, :, None], 0.0), mb.actor_h0, mb.actor_c0)
    val, ch, cc, pc = run("critic", s.critic, T(mb.critic_obs), mb.critic_h0, mb.critic_c0)
    lp = plo.gaussian_tanh_logp(mean, pa["log_std"], T(mb.raw_actions))
    ent = -plo.gaussian_tanh_logp(mean, pa["log_std"], mean)
    rtg, _ = ko.normalised_rtg(mb.rewards_to_go, s.vn, [(12, np.float64(mb.rewards_to_go).mean(),
                                                         ((np.float64(mb.rewards_to_go) - np.float64(mb.rewards_to_go).mean()) ** 2).sum())])
    r = plo.ppo_minibatch_losses(lp, T(mb.old_log_probs), T(mb.advantages), ent, val.reshape(-1), rtg, True, use_huber=True)
    names_a = [n for t, n, _, _ in s.tables if t == "actor"]
    names_c = [n for t, n, _, _ in s.tables if t == "critic"]
    ga = torch.autograd.grad(r["actor_loss"], [pa[n] for n in names_a])
    gc = torch.autograd.grad(r["critic_loss"], [pc[n] for n in names_c])
    got = _bucket(ga, gc, s.tables, s.size)
    bad = ko.failures(got, s.r64["grads"], s.r32["grads"], s.tables)
    assert not bad, "; ".join(bad)
    np.testing.assert_allclose(got, s.r64["grads"], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose([r["actor"], r["critic"]], s.r64["totals"][1:3], rtol=1e-12)
    for key, t in (("actor_h", ah), ("actor_c", ac), ("critic_h", ch), ("critic_c", cc)):
        np.testing.assert_allclose(t.detach().numpy(), s.r64[key], rtol=1e-12, atol=1e-15)
    assert not s.r64["grads"][s.pad].any() and all(np.abs(s.r64["grads"][o:o + int(np.prod(sh))]).max() > 0 for _, _, o, sh in s.tables)


# ---------------------------------------------------------------------------------------------------- sharpness
PLANTED = {
    "actor rows zeroed from the terminal position on": dict(mask_from_terminal=True),
    "critic rows zeroed as well": dict(mask_critic=True),
    "(h0, c0) from the window's first position": dict(states_from_first=True),
    "b_hh gradient dropped": dict(drop_b_hh_grad=True),
    "LayerNorm eps 1e-6": dict(ln_eps=1e-6),
    "biased advantage std": dict(adv_std_ddof=0),
}
@pytest.mark.parametrize("error", sorted(PLANTED))
def test_a_gpu_test_case_catches_every_planted_error(error):
    """float64-correct against float64-planted with the float32 floor, over every case; the cases that catch it are printed
    (S = 1 cases have no window to mask and no first position; LayerNorm's eps shows where a row's variance is small)."""
    caught = []
    for name in sorted(cases.CASES):
        s = steering(name)
        assert not ko.failures(s.r32["grads"], s.r64["grads"], s.r32["grads"], s.tables), "the float32 reference itself must pass"
        if ko.failures(s.reference(torch.float64, **PLANTED[error])["grads"], s.r64["grads"], s.r32["grads"], s.tables):
            caught.append(name)
    print(f"{error}: caught by {len(caught)} of {len(cases.CASES)} cases" + (f" ({', '.join(caught)})" if len(caught) < 6 else ""))
    assert caught, f"planted error accepted by every case: {error}"


# ---------------------------------------------------------------------------------------------------- kink budget
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_finds_its_unkinked_items_and_window_kinds(name):
    s = steering(name)                                      # (raises when fewer than B un-kinked items are found)
    c, B, S = s.c, s.c["B"], s.c["S"]
    assert s.items >= B + 8 and len(s.chosen) == B == len(set(s.chosen.tolist())) and s.budget >= B
    ka, kc = s.kinked(s.chosen, s.params, s.hidden)
    assert not (ka.any() or kc.any())
    if S > 1:
        have = s.kinds[s.chosen].sum(0)
        want = [min(s.need, max(0, B - k * s.need)) for k in range(5)]
        assert (have >= want).all(), dict(zip(cases.KINDS, have))
    ratio = np.exp(s.r64["logp"] - s.mb.old_log_probs)
    assert (ratio < 0.8).any() and (ratio > 1.2).any() and (B < 16 or ((ratio > 0.8) & (ratio < 1.2)).any())
    assert (s.mb.advantages > 0).any() and (s.mb.advantages < 0).any()
    if c["huber"]:
        d = np.abs(s.r64["values"] - s.r64["rtg"])
        assert (d > 10.0).any() and np.abs(d - 10.0).min() > 1e-3
    if s.head == "gaussian":
        assert (np.abs(s.mb.raw_actions) > 3.8).any()
    if c["second"]:
        assert set(s.second.tolist()) & set(s.chosen.tolist()) and len(s.second) == min(s.items - B, B)
        assert np.array_equal(s.perm[:B], s.chosen) and np.array_equal(s.perm[B:B + len(s.second)], s.second)
    assert len(s.perm) == s.items and s.perm.min() >= 0 and s.perm.max() < s.items
