"""
TEST INFRASTRUCTURE (see oracle/__init__.py) -- ONE mini-batch of K22 (csrc/lstm_update.hip) restated on torch-CPU in a
chosen dtype (float64 for the reference, float32 for the floor of what f32 arithmetic can reach): window masks, the
hidden-state hand-over, forward, loss, backward.  The clip + Adam of the step that follows is k12_oracle.clip_adam.

PINNED by the g12_lstm_* fixtures through oracle/lstm_oracle.CpuLSTMPPO (tests/test_lstm_update_oracle.py: float64
reproduces the first mini-batch's losses, raw gradients and final states of the pinned port).  Built from the pinned
pieces:

  network                 nn.LSTM(in, H, 1) -> LayerNorm(H) -> activation -> 1 or 2 hidden Linear + activation -> Linear
                          <- lstm_oracle.LSTMNet                         networks/ppo_networks/lstm.py:13-127
  window masks            <- lstm_oracle.SequenceDataset                 utils/episode_info.py:775-809, :976-987
  hidden-state hand-over  (h0, c0) of the window's LAST position         ppo.py:2312-2319, write-back :2450-2466
  heads, value normaliser, losses, comparison rule <- k12_oracle         (_head_terms, normalised_rtg, losses, deviations)

Layout is K18's (csrc/lstm_device.hpp layout_of): w_ih [4H, in], w_hh [4H, H], b_ih, b_hh (gate order i, f, g, o),
LayerNorm weight and bias, then weight [out, in] and bias per Linear, each tensor padded to 4 floats; the Gaussian head's
log_std follows the actor's last bias (padded to 4); the critic's segment follows the actor's.  Padding stays zero in the
gradient bucket.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import k12_oracle as ko

Consts = ko.Consts
SC_NAMES = ko.SC_NAMES


class Net(NamedTuple):
    in_dim: int
    hidden: int           # H of the LSTM and of the LayerNorm
    ff_hidden: int        # F of the feed-forward head
    ff_depth: int         # hidden Linear layers (1 or 2); ff_depth + 1 Linear layers
    out_dim: int
    activation: str


def _pad4(n):
    return (n + 3) // 4 * 4


def tensor_table(net, log_std=False):
    """[(name, offset, shape)] of one network's segment in K18's layout, and the segment's size."""
    H, I, F, D, O = net.hidden, net.in_dim, net.ff_hidden, net.ff_depth, net.out_dim
    shapes = [("w_ih", (4 * H, I)), ("w_hh", (4 * H, H)), ("b_ih", (4 * H,)), ("b_hh", (4 * H,)), ("ln_w", (H,)), ("ln_b", (H,))]
    for l in range(D + 1):
        i, o = (H if l == 0 else F), (O if l == D else F)
        shapes += [(f"ff{l}.weight", (o, i)), (f"ff{l}.bias", (o,))]
    if log_std:
        shapes.append(("log_std", (O,)))
    out, off = [], 0
    for name, shape in shapes:
        out.append((name, off, shape))
        off += _pad4(int(np.prod(shape)))
    return out, off


def bucket_tables(actor, critic, head):
    """[(tag, name, offset, shape)] over the whole bucket, and its size."""
    ta, na = tensor_table(actor, head == "gaussian")
    tc, nc = tensor_table(critic)
    return [("actor", n, o, s) for n, o, s in ta] + [("critic", n, na + o, s) for n, o, s in tc], na + nc


class _Module(nn.Module):
    """The network holding one segment's weights."""

    def __init__(self, net, seg, dtype, ln_eps=1e-5):
        super().__init__()
        self.net = net
        self.lstm = nn.LSTM(net.in_dim, net.hidden, 1)
        self.layer_norm = nn.LayerNorm(net.hidden, eps=ln_eps)
        dims = [net.hidden] + [net.ff_hidden] * net.ff_depth + [net.out_dim]
        self.ff = nn.ModuleList([nn.Linear(i, o) for i, o in zip(dims[:-1], dims[1:])])
        self.act = ko._activation(net.activation)
        self.to(dtype)
        table, _ = tensor_table(net)
        with torch.no_grad():
            for (name, off, shape), p in zip(table, self.ordered()):
                p.copy_(torch.as_tensor(np.asarray(seg[off:off + int(np.prod(shape))]).reshape(shape), dtype=dtype))

    def ordered(self):
        """The parameters in the layout's order."""
        l = self.lstm
        return [l.weight_ih_l0, l.weight_hh_l0, l.bias_ih_l0, l.bias_hh_l0, self.layer_norm.weight, self.layer_norm.bias] + \
               [p for x in self.ff for p in (x.weight, x.bias)]

    def forward(self, x, h0, c0):
        """x [B, S, in], h0 / c0 [B, H] -> (output [B, out], final h, final c, the activations' arguments)."""
        _, (h, c) = self.lstm(torch.transpose(x, 0, 1), (h0.unsqueeze(0), c0.unsqueeze(0)))     # lstm.py:103-113
        z = self.layer_norm(h[-1])                                                              # :115-121
        pre = [z]
        y = self.act(z)
        for layer in self.ff[:-1]:
            z = layer(y)
            pre.append(z)
            y = self.act(z)
        return self.ff[-1](y), h[-1], c[-1], pre


class Minibatch(NamedTuple):
    obs: np.ndarray            # [B, S, actor in_dim]   the windows as stored: the oracle applies the mask
    critic_obs: np.ndarray     # [B, S, critic in_dim]
    terminal: np.ndarray       # [B, S] bytes: the window's position is the last transition of a terminated episode
    actor_h0: np.ndarray       # [B, H] each: the states stored at the window's LAST position
    actor_c0: np.ndarray
    critic_h0: np.ndarray
    critic_c0: np.ndarray
    raw_actions: np.ndarray    # [B] class / [B, D] Gaussian pre-tanh      (this and the fields below: last position)
    old_log_probs: np.ndarray  # [B]
    advantages: np.ndarray     # [B]
    rewards_to_go: np.ndarray  # [B]
    first_states: Optional[tuple] = None    # the four states at the window's FIRST position: read by a planted error only


def window_mask(terminal, from_terminal=False):
    """[B, S] True where the actor's observation is zeroed: strictly after the window's first terminal byte
    (episode_info.py:791-809).  from_terminal: the planted error that zeroes the terminal position as well."""
    t = np.asarray(terminal).astype(np.int64)
    seen = np.cumsum(t, axis=1)
    return (seen > 0) if from_terminal else ((seen - t) > 0)


def _inputs(mb, dtype, mask_from_terminal, mask_critic, states_from_first):
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    mask = torch.as_tensor(window_mask(mb.terminal, mask_from_terminal))
    obs = T(mb.obs).masked_fill(mask.unsqueeze(-1), 0.0)                                   # :976-978
    cobs = T(mb.critic_obs)
    if mask_critic:
        cobs = cobs.masked_fill(mask.unsqueeze(-1), 0.0)
    st = mb.first_states if states_from_first else (mb.actor_h0, mb.actor_c0, mb.critic_h0, mb.critic_c0)
    return obs, cobs, [T(s) for s in st]


def minibatch(params, actor, critic, head, mb, consts, vn_state=(0.0, 1.0, 1e-4), records=None, dtype=torch.float64,
              mask_from_terminal=False, mask_critic=False, states_from_first=False, drop_b_hh_grad=False, ln_eps=1e-5,
              adv_std_ddof=1, *, gate_plants=ko.GatePlants()):
    """
    One K22 mini-batch from the flat parameter bucket `params` -> dict(totals [8] (ko.SC_NAMES), grads [bucket size] in
    K18's layout, padding zero; values [B] (critic outputs), rtg [B] (normalised), logp [B]; actor_h / actor_c / critic_h /
    critic_c [B, H]: the final states, written back at the last position; vn: the normaliser state after the records;
    gate_args: the arguments of the head's gradient gates, ko._head_terms).
    `records`: this mini-batch's (n, mean, M2) per rank (default: the mini-batch's own rewards-to-go).
    mask_from_terminal, mask_critic, states_from_first, drop_b_hh_grad, ln_eps, adv_std_ddof: planted errors of the
    sharpness tests (tests/test_lstm_update_oracle.py), never set otherwise; gate_plants: those of
    tests/test_head_gates_oracle.py.
    """
    params = np.asarray(params, dtype=np.float64)
    ta, na = tensor_table(actor, head == "gaussian")
    am = _Module(actor, params[:na], dtype, ln_eps)
    cm = _Module(critic, params[na:], dtype, ln_eps)
    aparams, cparams = am.ordered(), cm.ordered()
    log_std = None
    if head == "gaussian":
        off = ta[-1][1]
        log_std = nn.Parameter(torch.as_tensor(params[off:off + actor.out_dim], dtype=dtype))
        aparams = aparams + [log_std]
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    obs, cobs, (ah0, ac0, ch0, cc0) = _inputs(mb, dtype, mask_from_terminal, mask_critic, states_from_first)
    out, ah, ac, _ = am(obs, ah0, ac0)
    val, ch, cc, _ = cm(cobs, ch0, cc0)
    values = val.reshape(-1)
    gate_args = {}
    logp, ent = ko._head_terms(head, out, log_std, T(mb.raw_actions), (), consts.min_std, {}, gate_plants, gate_args)
    rtg = T(mb.rewards_to_go).reshape(-1)
    vn = None
    if consts.normalize_values:
        r = np.asarray(mb.rewards_to_go, dtype=np.float64).reshape(-1)
        if records is None:
            records = [(len(r), r.mean(), ((r - r.mean()) ** 2).sum())]
        rtg, vn = ko.normalised_rtg(mb.rewards_to_go, vn_state, records, dtype)
        rtg = rtg.reshape(-1)
    a_loss, c_loss, totals = ko.losses(logp.reshape(-1), T(mb.old_log_probs).reshape(-1), T(mb.advantages).reshape(-1),
                                       ent.reshape(-1), values, rtg, consts.normalize_adv, consts.surr_clip,
                                       consts.entropy_weight, consts.kl_loss_weight, consts.use_huber, consts.huber_delta,
                                       adv_std_ddof)
    ga = torch.autograd.grad(a_loss, aparams)
    gc = torch.autograd.grad(c_loss, cparams)
    tables, size = bucket_tables(actor, critic, head)
    grads = np.zeros(size, dtype=np.float64)
    for (tag, name, off, shape), g in zip(tables, list(ga) + list(gc)):
        if not (drop_b_hh_grad and name == "b_hh"):
            grads[off:off + g.numel()] = g.detach().double().numpy().reshape(-1)
    n64 = lambda t: t.detach().double().numpy()
    return dict(totals=totals, grads=grads, values=n64(values), rtg=n64(rtg), logp=n64(logp).reshape(-1),
                actor_h=n64(ah), actor_c=n64(ac), critic_h=n64(ch), critic_c=n64(cc), vn=vn,
                gate_args={k: n64(v) for k, v in gate_args.items()})


def pre_activations(net, seg, x, h0, c0, dtype=torch.float64):
    """The arguments of every activation -- the LayerNorm output and the hidden Linear layers' pre-activations -- of the
    items (x [B, S, in] as the network sees it, mask applied) -> list of [B, .] arrays."""
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    with torch.no_grad():
        return [z.numpy() for z in _Module(net, np.asarray(seg, dtype=np.float64), dtype)(T(x), T(h0), T(c0))[3]]


def kinked_items(net, seg, x, h0, c0, rel=1e-4):
    """Items with a ReLU / LeakyReLU argument within rel x its row's scale (max |z| of that layer) of zero: there float32
    may take the other side of the kink (the rule of ko.kinked_rows).  Tanh has none."""
    bad = np.zeros(len(x), dtype=bool)
    if net.activation == "tanh":
        return bad
    for z in pre_activations(net, seg, x, h0, c0):
        bad |= (np.abs(z) < rel * np.abs(z).max(axis=1, keepdims=True)).any(axis=1)
    return bad
