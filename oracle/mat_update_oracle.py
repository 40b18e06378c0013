"""
TEST INFRASTRUCTURE (see oracle/__init__.py) -- ONE mini-batch of K15 (csrc/mat_update.hip) restated on torch-CPU in a
chosen dtype (float64 for the reference, float32 for the floor of what f32 arithmetic can reach): token block, forward,
loss, backward of actor_loss + critic_loss over the one shared bucket, and the ONE clip + Adam of the step that follows.

PINNED by fixture g12_c5_mat through oracle/mat_oracle.CpuMATPPO (tests/test_mat_update_oracle.py: float64 reproduces the
first mini-batch's losses, actor gradients and recomputed critic gradients of the pinned port).  Built from the pinned
pieces:

  network                 <- mat_oracle.MATActorCritic (under .to(dtype))          networks/attention.py:13-257
  token block             <- mat_oracle.CpuMATPPO.action_block                      policies/mat_policy.py:308-344, :399-403
  Categorical of the actor's probabilities: renormalised, clamped to [eps, 1 - eps] before the log (torch's
                          probs_to_logits) with float32's eps IN EVERY DTYPE -- the clamp K15 restates
                          (csrc/mat_update.hip clamp_prob_u); it passes no gradient outside the bounds
  value normaliser        <- k12_oracle.normalised_rtg ((n, mean, M2) records, one per rank)
  advantage normalisation over the mini-batch's B A values, surrogate / entropy / KL / MSE-or-Huber <- k12_oracle.losses
  clip + Adam             <- k12_oracle.clip_adam with ONE network owning the whole bucket (mat_policy.py:677-699)

Layout is K15's (include/ppoaf_hip.h ppoaf_mat_update_args_t): the 63 tensors of MATActorCritic in module order, each
padded to 4 floats; rows are [n, A, .].  Padding stays zero in the gradient bucket.
"""
import functools
import math
import types
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import k12_oracle as ko
from . import mat_oracle as mo

Consts = ko.Consts
SC_NAMES = ko.SC_NAMES
EPS32 = float(np.finfo(np.float32).eps)


class Planted(NamedTuple):
    """Errors planted by the sharpness tests (tests/test_mat_update_oracle.py), never set otherwise.  manual_core runs the
    hand-written attention backward with no error in it (it must then agree with autograd)."""
    manual_core: bool = False
    softmax_no_rowsum: bool = False      # the softmax backward loses its row-sum term
    bwd_no_scale: bool = False           # the 1/sqrt(64) scale is missing in the backward only
    attn2_unmasked: bool = False         # the causal mask is missing in attn2
    dk_unmasked: bool = False            # dK is taken from the unmasked probabilities
    onehot_shift: bool = False           # the action one-hot is shifted by one agent (agent i sees its own action)
    no_start_token: bool = False
    ln_eps: float = 1e-5
    ln_gain_first: bool = False          # a LayerNorm gain applied before the normalisation
    tanh_gelu: bool = False
    adv_std_ddof: int = 1                # 0: the biased advantage std
    tile_mean: bool = False              # the loss mean over 16-row tiles (dead rows counted) instead of B A tokens
    # the rollout step K16 only (tests/helpers/mat_step_cases.py, tests/test_mat_step_oracle.py)
    counter_slot_major: bool = False     # the Philox counter as offset + slot E + env
    counter_no_slot: bool = False        # the Philox counter as offset + env: one draw shared by an env's agents
    philox_word_y: bool = False          # the draw from word y of the block
    stale_logits: bool = False           # every agent's draw taken from pass 0's logits
    denorm_var: bool = False             # values denormalised with var instead of sqrt(var + 1e-8)
    logp_no_clamp: bool = False          # the log-prob without the clamp to [eps, 1 - eps]
    # the clamp's gradient gate in K15's backward (tests/test_head_gates_oracle.py)
    gate_open: bool = False              # the clamp passes gradient everywhere
    gate_on_chosen_only: bool = False    # the entropy term's gate is dropped, the chosen class's gate is kept


def _pad4(n):
    return (n + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def bucket_table(A, O, NA):
    """([(tag '', name, offset, shape)] over the 63 tensors in module order, the bucket's size)."""
    out, off = [], 0
    for name, p in mo.MATActorCritic(O, NA, A).named_parameters():
        out.append(("", name, off, tuple(p.shape)))
        off += _pad4(p.numel())
    return out, off


class _Core(torch.autograd.Function):
    """softmax(mask(q k^T / sqrt(D))) v with the backward written out, so that the planted errors have a place."""

    @staticmethod
    def forward(ctx, q, k, v, mask, pl):
        scale = 1.0 / math.sqrt(k.size(-1))
        s = (q @ k.transpose(-2, -1)) * scale
        p = F.softmax(s if mask is None else s.masked_fill(~mask, float("-inf")), dim=-1)
        ctx.save_for_backward(q, k, v, p, F.softmax(s, dim=-1))
        ctx.pl, ctx.scale = pl, scale
        return p @ v

    @staticmethod
    def backward(ctx, dy):
        q, k, v, p, p_unmasked = ctx.saved_tensors
        pl = ctx.pl
        dp = dy @ v.transpose(-2, -1)

        def ds_of(pp):
            return pp * dp if pl.softmax_no_rowsum else pp * (dp - (pp * dp).sum(-1, keepdim=True))
        ds = ds_of(p)
        sc = 1.0 if pl.bwd_no_scale else ctx.scale
        dq = (ds @ k) * sc
        dk = (ds_of(p_unmasked) if pl.dk_unmasked else ds).transpose(-2, -1) @ q * sc
        return dq, dk, p.transpose(-2, -1) @ dy, None, None


def _attention_forward(pl):
    def forward(self, key, value, query):                 # mat_oracle.SelfAttention.forward with one head
        assert self.num_heads == 1
        L = query.size(1)
        mask = (self.mask[0, 0, :L, :L] != 0) if self.masked else None
        return self.proj(_Core.apply(self.query_net(query), self.key_net(key), self.value_net(value), mask, pl))
    return forward


def network(A, O, NA, params, dtype=torch.float64, planted=Planted()):
    """mat_oracle.MATActorCritic holding the bucket's weights in `dtype` (planted errors applied to this copy)."""
    net = mo.MATActorCritic(O, NA, A).to(dtype)
    table, _ = bucket_table(A, O, NA)
    params = np.asarray(params, dtype=np.float64)
    with torch.no_grad():
        for (_, name, off, shape), (pname, p) in zip(table, net.named_parameters()):
            assert name == pname
            p.copy_(torch.as_tensor(params[off:off + int(np.prod(shape))].reshape(shape), dtype=dtype))
    pl = planted
    for m in net.modules():
        if isinstance(m, nn.LayerNorm):
            m.eps = pl.ln_eps
            if pl.ln_gain_first:
                m.forward = (lambda x, m=m: F.layer_norm(x * m.weight, m.normalized_shape, None, None, m.eps) + m.bias)
        elif isinstance(m, nn.GELU) and pl.tanh_gelu:
            m.approximate = "tanh"
        elif isinstance(m, mo.SelfAttention) and (pl.manual_core or pl.softmax_no_rowsum or pl.bwd_no_scale or pl.dk_unmasked):
            m.forward = types.MethodType(_attention_forward(pl), m)
    if pl.attn2_unmasked:
        net.actor.blocks[0].attn2.masked = False
    return net


def action_block(actions, A, NA, dtype=torch.float64, planted=Planted()):
    """CpuMATPPO.action_block: the start token and the one-hot of the previous agents' actions, [B, A, NA + 1]."""
    a = torch.as_tensor(np.asarray(actions)).long().reshape(-1, A)
    if planted.onehot_shift:
        a = torch.roll(a, -1, dims=1)
    blk = mo.CpuMATPPO.action_block(types.SimpleNamespace(A=A, n_actions=NA), a).to(dtype)
    if planted.no_start_token:
        blk[:, 0, 0] = 0
    return blk


class Minibatch(NamedTuple):
    obs: np.ndarray            # [B, A, O]
    raw_actions: np.ndarray    # [B, A] classes
    old_log_probs: np.ndarray  # [B, A]
    advantages: np.ndarray     # [B, A]
    rewards_to_go: np.ndarray  # [B, A]


def own_record(x):
    """The (n, mean, M2) record of a table's values, as the driver forms it in float64."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return (len(x), x.mean(), ((x - x.mean()) ** 2).sum())


def minibatch(params, A, O, NA, mb, consts, vn_state=(0.0, 1.0, 1e-4), records=None, dtype=torch.float64, planted=Planted()):
    """
    One K15 mini-batch from the flat parameter bucket -> dict(totals [8] (ko.SC_NAMES; totals[9]'s ninth entry is the
    mini-batch count), grads [bucket size]: d (actor_loss + critic_loss) / d every tensor, padding zero; values [B, A]
    (the critic's outputs, written back as they are), rtg [B, A] (normalised), logp [B, A], probs [B, A, NA] (renormalised),
    vn (the normaliser state after the records); actor_grads / critic_grads: d actor_loss / d actor and d critic_loss /
    d critic as CpuMATPPO's trace holds them).  `records`: this mini-batch's (n, mean, M2) per rank (default: its own).
    """
    net = network(A, O, NA, params, dtype, planted)
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    B = len(mb.obs)
    actions = torch.as_tensor(np.asarray(mb.raw_actions)).long().reshape(B, A)
    values, probs = net(T(mb.obs).reshape(B, A, O), action_block(actions, A, NA, dtype, planted))
    n = probs / probs.sum(-1, keepdim=True)               # Categorical(probs=...): renormalised, clamped, log
    l = torch.log(ko._clamp(n, EPS32, 1.0 - EPS32, planted.gate_open))
    le = torch.log(ko._clamp(n, EPS32, 1.0 - EPS32, True)) if planted.gate_on_chosen_only else l
    logp = l.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    ent = -(n * le).sum(-1)
    values = values.squeeze(-1)
    rtg, vn = T(mb.rewards_to_go).reshape(B, A), None
    if consts.normalize_values:
        if records is None:
            records = [own_record(mb.rewards_to_go)]
        rtg, vn = ko.normalised_rtg(np.asarray(mb.rewards_to_go).reshape(-1), vn_state, records, dtype)
        rtg = rtg.reshape(B, A)
    a_loss, c_loss, totals = ko.losses(logp.reshape(-1), T(mb.old_log_probs).reshape(-1), T(mb.advantages).reshape(-1),
                                       ent.reshape(-1), values.reshape(-1), rtg.reshape(-1), consts.normalize_adv,
                                       consts.surr_clip, consts.entropy_weight, consts.kl_loss_weight, consts.use_huber,
                                       consts.huber_delta, planted.adv_std_ddof)
    if planted.tile_mean:
        per_tile = 16 // A
        f = (B * A) / (16.0 * ((B + per_tile - 1) // per_tile))
        a_loss, c_loss = a_loss * f, c_loss * f
    table, size = bucket_table(A, O, NA)
    ps = list(net.parameters())
    n64 = lambda t: t.detach().double().numpy()

    def bucket(loss, only=""):
        g = torch.autograd.grad(loss, ps, retain_graph=True, allow_unused=True)
        out = np.zeros(size, dtype=np.float64)
        for (_, name, off, shape), x in zip(table, g):
            if x is not None and name.startswith(only):
                out[off:off + x.numel()] = n64(x).reshape(-1)
        return out
    return dict(totals=totals, grads=bucket(a_loss + c_loss), actor_grads=bucket(a_loss, "actor."),
                critic_grads=bucket(c_loss, "critic."), values=n64(values), rtg=n64(rtg), logp=n64(logp), probs=n64(n), vn=vn)


def clip_adam(params, grads, exp_avg, exp_avg_sq, step, lr, max_norm, dtype=torch.float64):
    """One clip over the whole bucket and one Adam (ko.clip_adam with one network owning everything) from Adam's step
    counter `step` (before the step) -> (params, exp_avg, exp_avg_sq, the gradient's norm before the clip)."""
    p, m, v = ko.clip_adam(params, grads, exp_avg, exp_avg_sq, (step, step), lr, max_norm, len(np.asarray(params)), dtype=dtype)
    g = torch.as_tensor(np.asarray(grads, dtype=np.float64), dtype=dtype)
    return p, m, v, float(torch.sqrt((g * g).sum()))
