"""
-m gpu: ONE K15 mini-batch (csrc/mat_update.hip, fused_update.FusedMatUpdate) against the float64 reference
(oracle/mat_update_oracle.py, pinned to fixture g12_c5_mat by tests/test_mat_update_oracle.py) at the shape edges where the
kernel changes behaviour (tests/helpers/mat_update_cases.py: A 1 .. 16 with every dead-row count, obs_dim 1 .. 128 across
the LDS / chunk edges, 1 .. 8 actions, 1 .. 65 row tiles, the loss switches, six seeded draws), with the WEIGHTS OVERWRITTEN
so that every tensor's gradient is on the scale of the others -- at the default initialisation the attention cores get
gradients 1e-9 of the bucket's largest, and a bucket-wide atol accepts a wrong softmax backward, dq / dk or scale
(tests/test_mat_update_oracle.py::test_default_initialisation_hides_the_attention_errors_from_the_bucket_wide_rule).

Each case: a PPO with a MATPolicy on SyntheticFixedLengthEnv, one rollout, the parameter bucket overwritten, begin_epoch;
the args are the driver's (fused._args_for), with the tables, the row addressing, the records and the loss switches of
the case written into a copy (A = 1, which MATPolicy does not take but the kernel does: the package's network and args
filled as the driver fills them), and the library's entry points launched directly:
  tail   ppoaf_mat_update_fwd_bwd -> ppoaf_mat_update_wgrad_adam                   (the default chain)
  three  ... fwd_bwd -> ppoaf_mat_update_reduce (fuse_norm) -> ppoaf_adam_step_prenormed
  slab   the same three launches with split_workspace NULL
(the narrow kernel for O <= 32 and the wide one above are selected by the shapes).  The mini-batch's rows are addressed as
the driver does -- perm o row_map (non-identity) on buffer rows; per-epoch tables in batch order from cursor 1; the same by
mb_offset 1 with the cursor at 0 and cursor_advance 2; a tail mini-batch shorter than batch_stride behind two full ones --
and every table row, every record that is not the mini-batch's holds NaN, so a row taken from the wrong place shows.
  1. gradient only (fwd_bwd -> reduce; the split and the slab form): the gradient bucket, filled with NaN before, per
     tensor, padding exactly zero; totals[9]; the values of the mini-batch's rows, every other row bitwise unchanged; the
     cursor advanced by cursor_advance; the parameters bitwise unchanged;
  2. the step from a preset optimiser state (step 6, m and v on the gradient's scale), clip active (0.25 x the float64
     norm) and inactive (4 x): gradient bucket, parameter step, m, v, step count, grad norm, the normaliser slot written;
  3. (three cases) mini-batch 1 right after mini-batch 0, the reference started from the state the GPU left: the
     normaliser's other slot, the step counter, a mini-batch shorter than batch_stride.
Bound per tensor: |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| (the same reference in float32 on
the CPU) where float32 itself cannot do better (ko.deviations); totals is one tensor of the rule.  Tensors without a scale
of their own (cases.judge_gradient): a tensor that float64 gives as exactly zero (one agent, one action) must be exactly
zero; each key_net.bias -- zero in exact arithmetic, since a constant added to every key shifts a score row by a constant,
round-off in float64 -- is judged on the scale of the same attention's query_net.bias: 1e-5 max|g64| of that tensor, raised
to the float32 floor (and the observation LayerNorm's gain at O = 1 likewise on the scale of that LayerNorm's bias).
The slabs are zeroed before every launch, as the driver allocates them: the split and the slab form lay them out
differently and neither writes a tensor's padding.

Worst deviation / bound per case and form, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import functools
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import k12_oracle as ko
from oracle import mat_update_oracle as mu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mat_float64 as M  # noqa: E402
import mat_update_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}                     # (case, form) -> (worst fraction of the bound, where)
TOTALS = [("", "totals", 0, (8,))]
BETAS, EPS = (0.9, 0.999), 1e-5
E, T = 2, 4                    # the rollout that gives the driver a dataset (the case's tables are the test's own)
SENTINEL = 7.0                 # what the actions of rows outside the mini-batch hold (clamped by the kernel: never read)

MEASURED = """
worst deviation / bound per case and form (one run of the whole GPU suite: 1003 passed, 1 skipped in 231 s; this file alone 7 s)
  c5_3_18_5_32         slab   0.255  no clip step: actor.blocks.0.attn2.key_net.weight
  c5_3_18_5_32         tail   0.257  second step: critic.blocks.0.mlp.2.weight
  c5_3_18_5_32         three  0.255  no clip step: actor.blocks.0.attn2.key_net.weight
  chunk_16_128_8_2     slab   0.253  no clip step: critic.obs_encoder.1.weight
  chunk_16_128_8_2     tail   0.253  no clip step: critic.obs_encoder.1.weight
  chunk_16_128_8_2     three  0.253  no clip step: critic.obs_encoder.1.weight
  chunk_2_128_8_9      slab   0.259  clip step: actor.head.3.weight
  chunk_2_128_8_9      tail   0.259  clip step: actor.head.3.weight
  chunk_2_128_8_9      three  0.259  clip step: actor.head.3.weight
  chunk_3_97_5_11      slab   0.257  clip step: critic.blocks.0.mlp.2.weight
  chunk_3_97_5_11      tail   0.257  clip step: critic.blocks.0.mlp.2.weight
  chunk_3_97_5_11      three  0.257  clip step: critic.blocks.0.mlp.2.weight
  chunk_5_65_4_7       slab   0.257  clip step: critic.blocks.0.attn.proj.weight
  chunk_5_65_4_7       tail   0.257  clip step: critic.blocks.0.attn.proj.weight
  chunk_5_65_4_7       three  0.257  clip step: critic.blocks.0.attn.proj.weight
  chunk_6_96_3_5       slab   0.257  no clip step: actor.blocks.0.attn2.key_net.weight
  chunk_6_96_3_5       tail   0.257  no clip step: actor.blocks.0.attn2.key_net.weight
  chunk_6_96_3_5       three  0.257  no clip step: actor.blocks.0.attn2.key_net.weight
  dead_7_64_2_5        slab   0.259  no clip step: actor.blocks.0.attn1.key_net.weight
  dead_7_64_2_5        tail   0.259  no clip step: actor.blocks.0.attn1.key_net.weight
  dead_7_64_2_5        three  0.259  no clip step: actor.blocks.0.attn1.key_net.weight
  draw0_12_15_7_20     slab   0.259  no clip step: actor.blocks.0.attn2.query_net.weight
  draw0_12_15_7_20     tail   0.259  no clip step: actor.blocks.0.attn2.query_net.weight
  draw0_12_15_7_20     three  0.259  no clip step: actor.blocks.0.attn2.query_net.weight
  draw1_2_75_3_11      slab   0.263  clip step: actor.blocks.0.attn1.proj.bias
  draw1_2_75_3_11      tail   0.263  clip step: actor.blocks.0.attn1.proj.bias
  draw1_2_75_3_11      three  0.263  clip step: actor.blocks.0.attn1.proj.bias
  draw2_1_109_1_7      slab   0.259  clip step: actor.blocks.0.attn2.query_net.weight
  draw2_1_109_1_7      tail   0.259  clip step: actor.blocks.0.attn2.query_net.weight
  draw2_1_109_1_7      three  0.259  clip step: actor.blocks.0.attn2.query_net.weight
  draw3_3_3_1_30       slab   0.258  clip step: actor.blocks.0.attn2.query_net.weight
  draw3_3_3_1_30       tail   0.258  clip step: actor.blocks.0.attn2.query_net.weight
  draw3_3_3_1_30       three  0.258  clip step: actor.blocks.0.attn2.query_net.weight
  draw4_14_104_6_9     slab   0.256  no clip step: actor.blocks.0.attn1.value_net.weight
  draw4_14_104_6_9     tail   0.256  no clip step: actor.blocks.0.attn1.value_net.weight
  draw4_14_104_6_9     three  0.256  no clip step: actor.blocks.0.attn1.value_net.weight
  draw5_1_66_6_31      slab   0.648  gradient: critic.head.2.bias
  draw5_1_66_6_31      tail   0.648  gradient: critic.head.2.bias
  draw5_1_66_6_31      three  0.648  clip gradient: critic.head.2.bias
  lds_1_32_8_17        slab   0.258  clip step: actor.blocks.0.attn2.query_net.weight
  lds_1_32_8_17        tail   0.258  clip step: actor.blocks.0.attn2.query_net.weight
  lds_1_32_8_17        three  0.258  clip step: actor.blocks.0.attn2.query_net.weight
  mask_16_33_8_3       slab   0.264  no clip step: actor.blocks.0.attn2.key_net.weight
  mask_16_33_8_3       tail   0.264  no clip step: actor.blocks.0.attn2.key_net.weight
  mask_16_33_8_3       three  0.264  no clip step: actor.blocks.0.attn2.key_net.weight
  min_1_1_1_2          slab   0.255  clip step: critic.blocks.0.attn.query_net.weight
  min_1_1_1_2          tail   0.255  clip step: critic.blocks.0.attn.query_net.weight
  min_1_1_1_2          three  0.255  clip step: critic.blocks.0.attn.query_net.weight
  tiles64_16_7_4_64    slab   0.256  no clip step: actor.blocks.0.attn2.query_net.weight
  tiles64_16_7_4_64    tail   0.256  no clip step: actor.blocks.0.attn2.query_net.weight
  tiles64_16_7_4_64    three  0.256  no clip step: actor.blocks.0.attn2.query_net.weight
  tiles65_16_7_4_65    slab   0.268  clip step: actor.blocks.0.mlp.0.weight
  tiles65_16_7_4_65    tail   0.268  clip step: actor.blocks.0.mlp.0.weight
  tiles65_16_7_4_65    three  0.268  clip step: actor.blocks.0.mlp.0.weight
(a parameter step's ~0.25: the float32 rounding of p - p0, which the float32 reference on the CPU rounds the same way)
"""


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{c:24s} {f:6s} {v[0]:.3f}  {v[1]}" for (c, f), v in sorted(WORST.items())]
    print("\nworst deviation / bound per case and form:\n" + "\n".join(lines))
    out = os.environ.get("PPOAF_K15_REPORT")
    if out:
        with open(out, "w") as fh:
            json.dump({f"{c}/{f}": v for (c, f), v in sorted(WORST.items())}, fh, indent=1)


@functools.lru_cache(maxsize=None)
def steering(name):
    """The case's tables and its float64 / float32 references: built once per case, not once per form."""
    return cases.Steering({**cases.CASES, **cases.GATES_CASES}[name])


def _note(key, what, devs):
    tensor, frac, _ = max(devs, key=lambda d: d[1])
    if frac > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (frac, f"{what}: {tensor}")
    bad = [f"{n}: {f:.3g} x bound (float32 floor {fl:.3g})" for n, f, fl in devs if not f <= 1.0]
    assert not bad, f"{key[0]} / {key[1]} / {what}: " + "; ".join(bad[:6])


def _check(key, what, got, want64, want32, tables):
    _note(key, what, ko.deviations(got, want64, want32, tables))


def _one_tensor(what, n):
    return [("", what, 0, (n,))]


def _ppo(A, O, NA, B):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    return PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=dev, random_seed=6, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=1, update_mode="fused",
               use_graphs=False)


def _placement(c, B):
    """Where the mini-batches sit: mini-batch index mb0 = cursor + mb_offset for the case's own, mb0 + 1 for the second
    launch.  perm ranges over n_rows dataset rows, row_map sends them to n_buf buffer rows (both non-identity)."""
    cursor, offset, stride, in_order, advance = {"map": (0, 0, B, 0, 1), "tail": (2, 0, B + 7, 0, 1), "order": (1, 0, B + 3, 1, 1),
                                                 "offset": (0, 1, B, 1, 2)}[c["rows"]]
    rng = np.random.default_rng(c["seed"] + 2)
    mb0 = cursor + offset
    n_rows = (mb0 + 2) * stride + 3
    n_buf = n_rows + 4
    perm = rng.permutation(n_rows).astype(np.int64)
    row_map = rng.permutation(n_buf)[:n_rows].astype(np.int32)
    assert not np.array_equal(perm, np.arange(n_rows)) and not np.array_equal(row_map, np.arange(n_rows))
    return dict(cursor=cursor, offset=offset, stride=stride, in_order=in_order, advance=advance, mb0=mb0, n_mb=mb0 + 2,
                n_rows=n_rows, n_buf=n_buf, perm=perm, row_map=row_map)


class Device:
    """The case on the device: the policy's bucket holding the case's weights, the test's own tables, the driver's args."""

    def __init__(self, name):
        from ppo_and_friends_amd import _lib, kernels as K
        from ppo_and_friends_amd.fused_update import FusedMatUpdate, _describe_mat
        from ppo_and_friends_amd.fused_update import FusedEpoch
        self.wait_seconds = FusedEpoch.tail_wait_seconds
        self.name, self.s = name, steering(name)
        s, c = self.s, self.s.c
        A, O, NA, B = s.shape
        if c["saturate"]:
            assert s.gates_failures() == [], "gates steering: " + "; ".join(s.gates_failures())
        self.lib, self.K, self._lib = _lib.load(), K, _lib
        dev = self.dev = torch.device("cuda", 0)
        n_wg = (B + 16 // A - 1) // (16 // A)
        if A >= 2:
            self.ppo = ppo = _ppo(A, O, NA, B)
            pol = ppo.policies["mat"]
            assert FusedMatUpdate.unsupported_reason(pol, B) == ""
            ppo.rollout()
            pol.train()
            fused = self.fused = ppo._fused_updater("mat", B)
            assert isinstance(fused, FusedMatUpdate) and fused.split and fused.tail_reason() == "", fused.tail_reason()
            assert fused.n_wg == n_wg and tuple(pol.actor_critic_optim.betas) == BETAS and pol.actor_critic_optim.eps == EPS
            ac, owner, self.slabs = pol.actor_critic, pol, fused.slabs
        else:
            # MATPolicy takes two agents or more (one agent is an ordinary PPOPolicy), so no driver exists for A = 1, which
            # the kernel accepts: the package's network alone, the args filled as FusedMatUpdate._make_args fills them
            ac = M.make_network(O, NA, A, c["seed"], dev)
            owner = types.SimpleNamespace(actor_critic=ac, action_dtype="discrete")
        self.ac = ac
        # the bucket is laid out as the oracle's table says (module order, each tensor padded to 4 floats)
        topo, why = _describe_mat(owner)
        assert why == "" and topo["bucket_total"] == s.size == ac.flat_params.numel() == ac.flat_grads.numel()
        base = ac.flat_params.data_ptr()
        for (_, tname, off, shape), (pname, p), o in zip(s.table, ac.named_parameters(), topo["offsets"]):
            assert tname == pname and (p.data_ptr() - base) // 4 == off == o and tuple(p.shape) == tuple(shape), tname
        self.p0 = torch.as_tensor(s.params, dtype=torch.float32, device=dev)
        with torch.no_grad():
            ac.flat_params.copy_(self.p0)
        if A >= 2:
            fused.begin_epoch(torch.randperm(len(pol.dataset), device=dev))
            a = self.a = _lib.MatUpdateArgs.from_buffer_copy(fused._args_for(B))
        else:
            a = self.a = _lib.MatUpdateArgs()
            a.obs_dim, a.num_agents, a.num_actions, a.embedding, a.bucket_total = O, A, NA, 64, s.size
            for i, o in enumerate(topo["offsets"]):
                a.offsets[i] = o
            self.slabs = torch.zeros(n_wg, s.size, device=dev)
            a.params, a.grads, a.slabs, a.fuse_norm = ac.flat_params.data_ptr(), ac.flat_grads.data_ptr(), self.slabs.data_ptr(), 1
        assert (a.obs_dim, a.num_agents, a.num_actions, a.bucket_total) == (O, A, NA, s.size)
        assert a.params == ac.flat_params.data_ptr() and a.grads == ac.flat_grads.data_ptr() and a.fuse_norm == 1
        self.loss_partials = torch.zeros(n_wg, 8, device=dev)
        self.lr = torch.full((1,), cases.LR, device=dev)
        self.ctl = None                                          # the fused tail's control block: zeroed once, then kept
        a.loss_partials = self.loss_partials.data_ptr()
        # ---- the test's own tables: NaN wherever no mini-batch has a row
        pl = self.pl = _placement(c, B)
        n_tab = pl["n_rows"] if pl["in_order"] else pl["n_buf"]
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32)
        tab = dict(obs=nan(n_tab, A, O), act=torch.full((n_tab, A), int(SENTINEL), dtype=torch.int64), adv=nan(n_tab, A),
                   old=nan(n_tab, A), rtg=nan(n_tab, A))
        vn_rec = torch.full((pl["n_mb"], c["n_ranks"], 3), float("nan"), dtype=torch.float64)
        adv_rec = torch.full((pl["n_mb"], 3), float("nan"), dtype=torch.float64)
        self.rows = {}
        for k, mb in enumerate([s.mb] + ([s.mb1] if s.mb1 is not None else [])):
            n = len(mb.obs)
            pos = (pl["mb0"] + k) * pl["stride"] + np.arange(n)
            buf = pl["row_map"][pl["perm"][pos]].astype(np.int64)
            self.rows[k] = torch.as_tensor(buf, device=dev)
            at = torch.as_tensor(pos if pl["in_order"] else buf)
            for key, x in (("obs", mb.obs), ("act", mb.raw_actions), ("adv", mb.advantages), ("old", mb.old_log_probs), ("rtg", mb.rewards_to_go)):
                tab[key][at] = torch.as_tensor(np.asarray(x)).to(tab[key].dtype)
            vn_rec[pl["mb0"] + k] = torch.as_tensor(np.asarray(s.records_of(mb), dtype=np.float64))
            adv_rec[pl["mb0"] + k] = torch.as_tensor(np.asarray(mu.own_record(mb.advantages), dtype=np.float64))
        g = torch.Generator().manual_seed(c["seed"])
        k = self.keep = {key: x.to(dev).contiguous() for key, x in tab.items()}
        k.update(vn_rec=vn_rec.to(dev), adv_rec=adv_rec.to(dev), perm=torch.as_tensor(pl["perm"]).to(dev),
                 row_map=torch.as_tensor(pl["row_map"]).to(dev), values0=torch.randn(pl["n_buf"], A, generator=g).to(dev),
                 cursor=torch.zeros(1, dtype=torch.int64, device=dev), totals=torch.zeros(9, dtype=torch.float64, device=dev),
                 scratch=torch.zeros(4096, dtype=torch.float64, device=dev), m=torch.zeros(s.size, device=dev),
                 v=torch.zeros(s.size, device=dev), step=torch.zeros(1, dtype=torch.int64, device=dev),
                 gnorm=torch.zeros(1, device=dev), vn_mean=torch.zeros(2, device=dev), vn_var=torch.zeros(2, device=dev),
                 vn_count=torch.zeros(2, dtype=torch.float64, device=dev))
        k["values"] = k["values0"].clone()
        a.critic_obs, a.raw_actions, a.advantages = k["obs"].data_ptr(), k["act"].data_ptr(), k["adv"].data_ptr()
        a.old_log_probs, a.rewards_to_go, a.values = k["old"].data_ptr(), k["rtg"].data_ptr(), k["values"].data_ptr()
        a.perm, a.row_map, a.n_rows = k["perm"].data_ptr(), k["row_map"].data_ptr(), pl["n_rows"]
        a.inputs_in_batch_order = pl["in_order"]
        a.cursor, a.B, a.batch_stride = k["cursor"].data_ptr(), B, pl["stride"]
        a.mb_offset, a.cursor_advance = pl["offset"], pl["advance"]
        a.normalize_values, a.n_ranks = int(c["norm_values"]), c["n_ranks"]
        a.normalize_adv, a.use_huber = int(c["norm_adv"]), int(c["huber"])
        a.vn_mean, a.vn_var, a.vn_count = k["vn_mean"].data_ptr(), k["vn_var"].data_ptr(), k["vn_count"].data_ptr()
        a.vn_records, a.adv_records = k["vn_rec"].data_ptr(), k["adv_rec"].data_ptr()
        a.surr_clip, a.entropy_weight, a.kl_loss_weight, a.huber_delta = 0.2, c["ent"], c["kl"], 10.0
        a.totals, a.norm_scratch, a.step_count = k["totals"].data_ptr(), k["scratch"].data_ptr(), k["step"].data_ptr()
        if A == 1:                                               # (sized with every other field in place: the call validates them)
            need = C.c_int64(0)
            _lib.check(self.lib.ppoaf_mat_update_split_workspace_bytes(C.byref(a), C.byref(need)), "mat_update_split_workspace_bytes")
            self.split_space = torch.zeros(int(need.value), dtype=torch.uint8, device=dev)
            a.split_workspace, a.split_workspace_bytes = self.split_space.data_ptr(), self.split_space.numel()
        self.ws = (a.split_workspace, a.split_workspace_bytes)
        assert self.ws[0] and self.ws[0] % 256 == 0

    # ------------------------------------------------------------------------------------------------------------------
    def reset(self):
        """The case's starting state: parameters, a NaN gradient bucket, the preset optimiser state, cursor, normaliser."""
        s, k, pl = self.s, self.keep, self.pl
        with torch.no_grad():
            self.ac.flat_params.copy_(self.p0)
            self.ac.flat_grads.fill_(float("nan"))               # every gradient element must be written
        k["m"].copy_(torch.from_numpy(s.m0)); k["v"].copy_(torch.from_numpy(s.v0))
        k["step"].fill_(cases.STEP0)
        k["cursor"].fill_(pl["cursor"])
        k["totals"].zero_(); k["scratch"].zero_(); k["gnorm"].fill_(float("nan"))
        k["values"].copy_(k["values0"])
        k["vn_mean"].fill_(s.vn[0]); k["vn_var"].fill_(s.vn[1]); k["vn_count"].fill_(s.vn[2])
        self.loss_partials.zero_()
        self.slabs.zero_()             # as the driver allocates them: the two forms lay them out differently, neither writes padding
        self.a.B, self.a.mb_offset, self.a.cursor_advance = s.shape[3], pl["offset"], pl["advance"]

    def _form(self, form):
        a = self.a
        a.fuse_norm = 1
        a.split_workspace, a.split_workspace_bytes = (None, 0) if form == "slab" else self.ws

    def gradient_only(self, form):
        a, st = self.a, self.K.stream()
        self._form(form)
        assert 0 < int(self.lib.ppoaf_mat_update_norm_partials(C.byref(a))) <= self.keep["scratch"].numel() - 2
        self._lib.check(self.lib.ppoaf_mat_update_fwd_bwd(C.byref(a), st), "mat_update_fwd_bwd")
        self._lib.check(self.lib.ppoaf_mat_update_reduce(C.byref(a), st), "mat_update_reduce")
        torch.cuda.synchronize()

    def step(self, form, max_norm):
        a, k, st = self.a, self.keep, self.K.stream()
        self._form(form)
        self._lib.check(self.lib.ppoaf_mat_update_fwd_bwd(C.byref(a), st), "mat_update_fwd_bwd")
        if form == "tail":
            if self.ctl is None:
                need = C.c_int64(0)
                self._lib.check(self.lib.ppoaf_mat_update_tail_ctl_bytes(C.byref(a), C.byref(need)), "mat_update_tail_ctl_bytes")
                self.ctl = torch.zeros((int(need.value) + 63) // 64 * 16, dtype=torch.int32, device=self.dev)
            self._lib.check(self.lib.ppoaf_mat_update_wgrad_adam(
                C.byref(a), self.ctl.data_ptr(), k["m"].data_ptr(), k["v"].data_ptr(), self.lr.data_ptr(), BETAS[0], BETAS[1],
                EPS, 1.0, max_norm, k["gnorm"].data_ptr(), self.wait_seconds, st), "mat_update_wgrad_adam")
            torch.cuda.synchronize()
            assert int(self.ctl[2].item()) == 0, "the fused tail: a wait for the other workgroups ran out of time"
            return
        self._lib.check(self.lib.ppoaf_mat_update_reduce(C.byref(a), st), "mat_update_reduce")
        n = int(self.lib.ppoaf_mat_update_norm_partials(C.byref(a)))
        assert 0 < n <= k["scratch"].numel() - 2
        self._lib.check(self.lib.ppoaf_adam_step_prenormed(
            self.ac.flat_params.data_ptr(), self.ac.flat_grads.data_ptr(), k["m"].data_ptr(), k["v"].data_ptr(), self.s.size,
            k["step"].data_ptr(), self.lr.data_ptr(), BETAS[0], BETAS[1], EPS, 1.0, max_norm, k["scratch"].data_ptr(), n,
            k["gnorm"].data_ptr(), st), "adam_step_prenormed")
        torch.cuda.synchronize()

    def state(self):
        k = self.keep
        return [t.detach().double().cpu().numpy() for t in (self.ac.flat_grads, self.ac.flat_params, k["m"], k["v"])]


def _check_gradient(key, what, d, grads, r64, r32):
    s = d.s
    assert not grads[s.pad].any(), f"{key}: {what}: padding of the gradient bucket is not exactly zero"
    _note(key, what, cases.judge_gradient(grads, r64["grads"], r32["grads"], s.table, s.zero(), s.round_off()))


def _check_launch(key, what, d, which, r64, r32, mb_index, advanced_to, n_done, totals0=None):
    """What every launch leaves besides the bucket: totals[9], the values of the mini-batch's rows (every other row bitwise
    unchanged), the cursor, and -- normalize_values -- the normaliser slot the mini-batch writes."""
    s, k = d.s, d.keep
    tot = k["totals"].cpu().numpy() - (0.0 if totals0 is None else totals0)
    _check(key, f"{what} totals", tot[:8], r64["totals"], r32["totals"], TOTALS)
    assert k["totals"][8].item() == float(n_done), f"{key}: {what}: mini-batch count {k['totals'][8].item()}"
    rows = d.rows[which]
    n = r64["values"].size
    _check(key, f"{what} values", k["values"][rows].cpu().numpy(), r64["values"], r32["values"], _one_tensor("values", n))
    other = torch.ones(d.pl["n_buf"], dtype=torch.bool, device=d.dev)
    for w in range(which + 1):
        other[d.rows[w]] = False
    assert torch.equal(k["values"][other], k["values0"][other]), f"{key}: {what}: values outside the mini-batch's rows changed"
    assert int(k["cursor"].item()) == advanced_to, f"{key}: {what}: cursor {int(k['cursor'].item())}, expected {advanced_to}"
    if s.c["norm_values"]:
        slot = (mb_index & 1) ^ 1
        vn = [float(k["vn_mean"][slot]), float(k["vn_var"][slot]), float(k["vn_count"][slot])]
        _check(key, f"{what} normaliser", vn, r64["vn"], r32["vn"], None)


def _check_step(key, what, d, r64, r32, p0, m0, v0, step0, max_norm):
    s, k = d.s, d.keep
    grads, params, m, v = d.state()
    want = mu.clip_adam(p0, r64["grads"], m0, v0, step0, cases.LR, max_norm)
    want32 = mu.clip_adam(p0, r32["grads"], m0, v0, step0, cases.LR, max_norm, dtype=torch.float32)
    _check_gradient(key, f"{what} gradient", d, grads, r64, r32)
    _check(key, f"{what} step", params - p0, want[0] - p0, want32[0] - p0, s.table)
    _check(key, f"{what} m", m, want[1], want32[1], s.table)
    _check(key, f"{what} v", v, want[2], want32[2], s.table)
    for name, got, start in (("parameters", params, p0), ("m", m, m0), ("v", v, v0)):
        assert np.array_equal(got[s.pad], np.asarray(start, dtype=np.float64)[s.pad]), f"{key}: {what}: padding of {name} written"
    assert int(k["step"].item()) == step0 + 1, f"{key}: {what}: step count {int(k['step'].item())}"
    _check(key, f"{what} grad norm", [float(k["gnorm"].item())], [want[3]], [want32[3]], _one_tensor("grad norm", 1))


def run_case(name):
    d = Device(name)
    s, pl = d.s, d.pl
    p0 = d.p0.double().cpu().numpy()
    assert np.array_equal(p0, s.params)
    forms = ("three", "slab", "tail")          # (every form on every case: the file takes a few seconds; the default chain last)
    for form in forms:
        key = (name, form)
        # ---- 1. the gradient of one mini-batch ("three" launches what "tail" launches here: the split form once)
        if form != "three":
            d.reset()
            d.gradient_only(form)
            grads, params, _, _ = d.state()
            _check_gradient(key, "gradient", d, grads, s.r64, s.r32)
            _check_launch(key, "gradient only", d, 0, s.r64, s.r32, pl["mb0"], pl["cursor"] + pl["advance"], 1)
            assert np.array_equal(params, p0), f"{key}: parameters changed by the gradient-only launches"
        # ---- 2. one full step from a non-zero optimiser state, clip active / inactive
        for tag, max_norm in zip(("clip", "no clip"), s.max_norms):
            d.reset()
            d.step(form, max_norm)
            _check_step(key, tag, d, s.r64, s.r32, p0, s.m0, s.v0, cases.STEP0, max_norm)
            _check_launch(key, tag, d, 0, s.r64, s.r32, pl["mb0"], pl["cursor"] + pl["advance"], 1)
    # ---- 3. mini-batch 1 right after (the default chain, from the state the no-clip step above left)
    if s.mb1 is not None:
        key, k = (name, "tail"), d.keep
        _, p1, m1, v1 = d.state()
        slot = (pl["mb0"] & 1) ^ 1
        vn1 = (float(k["vn_mean"][slot]), float(k["vn_var"][slot]), float(k["vn_count"][slot])) if s.c["norm_values"] else s.vn
        r64 = s.reference(torch.float64, mb=s.mb1, params=p1, vn=vn1)
        r32 = s.reference(torch.float32, mb=s.mb1, params=p1, vn=vn1)
        tot0 = k["totals"].cpu().numpy().copy()
        with torch.no_grad():
            d.ac.flat_grads.fill_(float("nan"))
        d.a.B, d.a.mb_offset, d.a.cursor_advance = len(s.mb1.obs), 0, 1
        assert d.a.B < d.a.batch_stride or s.shape[3] == 2
        d.step("tail", s.max_norms[1])
        _check_step(key, "second", d, r64, r32, p1, m1, v1, cases.STEP0 + 1, s.max_norms[1])
        _check_launch(key, "second", d, 1, r64, r32, pl["mb0"] + 1, pl["cursor"] + pl["advance"] + 1, 2, tot0)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_k15_minibatch_against_float64(name):
    run_case(name)
