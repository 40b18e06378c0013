"""
-m gpu: ONE launch of K6+K7 (csrc/policy_step.hip: ppoaf_policy_step and its block form, every width pair of
PPOAF_WIDTH_PAIRS, the four heads of csrc/action_heads.hpp) against its restatement in float64
(tests/helpers/policy_step_cases.py: eval_kernels.Net, the heads of tests/helpers/head_draws.py on the Philox of
tests/helpers/philox.py), at the shape edges of the kernel and with the actor's output layer STEERED for logits of
O(1) .. O(3) (at the default initialisation every distribution is near uniform).  What the restatement states and no
other test does: the tile-to-workgroup mapping beyond four tiles (E = 65 and 129), a critic with an in_dim, a width and a
depth of its own, the value's denormalisation, the min_std floor, per-dimension bounds, the clamps of the four log-probs,
which Philox counter, block and word a row, a slice and a bit draw from, and that the draw is the inverse CDF / the bit
test / the Box-Muller pair of the float64 distribution.  tests/test_policy_step_oracle.py shows on the CPU that each of
these, planted as an error, is caught by a named case, and that every case meets its conditions.

Each case: ppoaf_policy_step launched directly on one bucket holding the case's parameters.  Every output tensor has
PAD rows in front of and behind its E rows holding a sentinel that must stay; the inputs, the bucket, the bounds and the
normaliser state must come back bitwise as they went in; the launch with NULL observation-copy pointers must give
bitwise the other outputs of the launch with them.
  sampled      actions float64's on the kept rows (near-tie rules of head_draws; the cap on rows left out is a condition
               of the cases), raw == action for the discrete heads; logp (kept rows), values, Gaussian raw and action
               by the bound rule; the observation copies bitwise the inputs;
  forced       the float64 draw replayed with indices outside their slices (clamped), |raw| ~ 4, |raw| = 9 and a row
               20 sd off a floored dimension (Gaussian), flipped bits (MultiBinary): raw_action_out bitwise the forced
               tensor (the indices clamped), every row's logp by bound -- the saturated cases log log(eps32);
  block form   six cases of E = 65 as 13 x 5 and E = 129 as 43 x 3 row blocks, not ascending in memory: every output
               bitwise the plain form's, the env's action blocks hold the action rows;
  refusals     made on the host, nothing launched: LDS just over 160 KB, out_dim 9, an nvec that does not sum to out_dim,
               one action bound without the other; E = 0 is accepted and writes nothing.
Bound per tensor (eval_kernels.k12_bound): |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| of the same
restatement in float32.
And once per head through the policy (PPO.rollout, update_mode="fused"): see test_counters_through_the_policy.

Worst deviation / bound and rows left out per case and launch, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import eval_kernels as ek  # noqa: E402
import policy_step_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

CAT, GAU, MCAT, BERN = cases.CAT, cases.GAU, cases.MCAT, cases.BERN
PAD = 4                        # sentinel rows in front of and behind every output tensor
I_SENT, F_SENT = -77, -12345.0
OUTPUTS = ("raw", "act", "logp", "value", "obs_copy", "cobs_copy")
WORST = {}                     # (case, launch) -> (rows left out, {tensor: deviation / bound})

MEASURED = """
per case and launch: rows left out by the near-tie rule / worst deviation over bound (the tensor it belongs to)
(this file alone: 63 passed in 4.3 s; tests/test_gpu_lstm_step_float64.py: 42 passed in 4.5 s)
  cat2_e1_32x32                    sampled 0/0.012 value | forced 0/0.012 value
  cat2_lds_in376_256x256           sampled 0/0.042 logp | forced 0/0.031 logp
  cat5_e17_wrap_64x64              sampled 0/0.018 value | forced 0/0.018 value
  cat5_sat_e16_128x128             sampled 1/0.048 logp | forced 0/0.015 logp
  cat8_e129_32x256                 sampled 0/0.026 value | forced 0/0.026 value
  cat8_e65_64x64                   sampled 1/0.023 value | forced 0/0.023 value
  gau1_e16_64x128                  sampled 0/0.034 logp | forced 0/0.045 logp
  gau3_floor_e15_128x256           sampled 0/0.151 logp | forced 0/0.032 logp
  gau4_depth7_e17_64x256           sampled 0/0.250 logp | forced 0/0.023 logp
  gau4_e63_wrap_32x64              sampled 0/0.263 logp | forced 0/0.107 logp
  gau5_e129_128x256                sampled 0/0.177 logp | forced 0/0.056 logp
  gau8_e65_256x512                 sampled 0/0.130 logp | forced 0/0.041 logp
  mb1_e15_32x256                   sampled 0/0.011 value | forced 0/0.011 value
  mb4_e63_64x64                    sampled 0/0.019 value | forced 0/0.019 value
  mb5_e17_wrap_256x256             sampled 0/0.029 value | forced 0/0.029 value
  mb5_lds_limit_e15_256x512        sampled 0/0.026 value | forced 0/0.026 value
  mb8_e65_64x128                   sampled 0/0.019 value | forced 0/0.019 value
  mb8_pm20_e16_32x64               sampled 0/0.013 value | forced 0/0.013 value
  md17_e129_32x64                  sampled 0/0.018 value | forced 0/0.018 value
  md1x8_e63_128x128                sampled 0/0.018 value | forced 0/0.018 value
  md2222_e17_wrap_64x128           sampled 0/0.019 value | forced 0/0.019 value
  md32_e15_32x32                   sampled 0/0.011 value | forced 0/0.011 value
  md44_e16_wrap_between_64x256     sampled 0/0.016 value | forced 0/0.016 value
  md8_sat_e16_256x256              sampled 0/0.053 logp | forced 0/0.012 value
  policy_bernoulli                 rollout 0/0.008 logp
  policy_categorical               rollout 0/0.007 value
  policy_gaussian                  rollout 0/0.107 logp
  policy_multi_categorical         rollout 0/0.010 logp
worst, categorical: logp 0.048 (cat5_sat_e16_128x128 sampled), value 0.026 (cat8_e129_32x256 sampled)
worst, gaussian: action 0.096 (gau8_e65_256x512 sampled), logp 0.263 (gau4_e63_wrap_32x64 sampled), raw 0.029 (gau8_e65_256x512 sampled), value 0.031 (gau4_e63_wrap_32x64 sampled)
worst, multi_categorical: logp 0.053 (md8_sat_e16_256x256 sampled), value 0.019 (md2222_e17_wrap_64x128 sampled)
worst, bernoulli: logp 0.016 (mb5_e17_wrap_256x256 sampled), value 0.029 (mb5_e17_wrap_256x256 sampled)
rows left out: 2
(the two rows left out -- one of cat5_sat_e16_128x128, one of cat8_e65_64x64 -- are the float64 reference's own near ties;
the block form is bitwise the plain form at E = 65 and E = 129, sampled and forced; the observation copies are bitwise the
inputs; no kernel or host bug was found)
"""


def _report_lines():
    """One line per case: per launch the rows left out and the worst deviation / bound with its tensor; then the worst
    per head and tensor over all cases."""
    lines, per = [], {}
    for c in sorted({c for c, _ in WORST}):
        parts = []
        head = cases.CASES[c]["head"] if c in cases.CASES else c.replace("policy_", "")
        for (cc, l), (left, fr) in WORST.items():
            if cc != c:
                continue
            k = max(fr, key=fr.get)
            parts.append(f"{l} {left}/{fr[k]:.3f} {k}")
            for t, v in fr.items():
                if t.endswith("_copy"):                                # (exact or inf: nothing to rank)
                    continue
                if v > per.get((head, t), (-1.0, ""))[0]:
                    per[(head, t)] = (v, f"{c} {l}")
        lines.append(f"  {c:32s} " + " | ".join(parts))
    for head in (CAT, GAU, MCAT, BERN):
        lines.append(f"worst, {head}: " + ", ".join(f"{t} {v:.3f} ({w})" for (h, t), (v, w) in sorted(per.items()) if h == head))
    lines.append(f"rows left out: {sum(left for left, _ in WORST.values())}")
    return lines


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = _report_lines()
    print("\nrows left out / worst deviation over bound (its tensor) per case and launch:\n" + "\n".join(lines))
    out = os.environ.get("PPOAF_K6_REPORT")
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _bits(x):
    return x.contiguous().view(torch.uint8)


class Device:
    """The case on the device: eval_kernels.Policy holding the case's networks in one bucket, and the launches."""

    def __init__(self, name):
        from ppo_and_friends_amd import _lib, kernels as K
        self.name, self.s = name, cases.steering(name)
        s, c = self.s, self.s.c
        self._lib, self.lib, self.K = _lib, _lib.load(), K
        dev = self.dev = torch.device("cuda", 0)
        self.E, self.O, self.head = c["E"], c["O"], s.head
        self.pol = ek.Policy(0, c["Ia"], c["Ha"], c["Da"], self.O, s.head, c["act"], s.slices, s.bounds,
                             nets=(s.actor, s.critic))
        assert self.pol.params.numel() == s.params().size
        assert np.array_equal(self.pol.params.cpu().numpy(), s.params())
        self.obs = torch.from_numpy(s.obs).to(dev).contiguous()
        self.cobs = torch.from_numpy(s.cobs).to(dev).contiguous()
        self.vn = None
        if s.vn is not None:
            self.vn = tuple(torch.tensor([x], dtype=torch.float32, device=dev) for x in s.vn)
        self.adt = torch.float32 if s.head in (GAU, BERN) else torch.int64
        self.aw = {CAT: 1, MCAT: len(s.slices)}.get(s.head, self.O)

    def outputs(self):
        """name -> [PAD + E + PAD, w] tensor of sentinels."""
        n, dev = self.E + 2 * PAD, self.dev
        floats = lambda w: torch.full((n, w), F_SENT, dtype=torch.float32, device=dev)
        acts = lambda: torch.full((n, self.aw), I_SENT, device=dev).to(self.adt)
        return dict(raw=acts(), act=acts(), logp=floats(1), value=floats(1), obs_copy=floats(self.s.c["Ia"]),
                    cobs_copy=floats(self.s.c["Ic"]))

    def args(self, T, forced=None, copies=True, keep=None):
        """The launch's argument block over the output tensors T (`keep`: tensors that must outlive the launch)."""
        s = self.s
        a = self.pol.step_args(self.obs, s.seed, s.offset, self.cobs)
        if self.vn is not None:
            a.normalize_values, a.vn_mean, a.vn_var = 1, self.vn[0].data_ptr(), self.vn[1].data_ptr()
        first = lambda k: T[k][PAD:].data_ptr()
        a.raw_action_out, a.action_out, a.logp_out, a.value_out = first("raw"), first("act"), first("logp"), first("value")
        if copies:
            a.obs_copy_out, a.critic_obs_copy_out = first("obs_copy"), first("cobs_copy")
        if forced is not None:
            f = torch.as_tensor(np.asarray(forced)).to(self.dev).to(self.adt).reshape(self.E, self.aw).contiguous()
            keep.append(f)
            a.forced_raw_action = f.data_ptr()
        return a

    def inputs(self, keep):
        t = dict(obs=self.obs, cobs=self.cobs, params=self.pol.params)
        if self.vn is not None:
            t.update(vn_mean=self.vn[0], vn_var=self.vn[1])
        if self.pol.bounds is not None:
            t.update(lo=self.pol.bounds[0], hi=self.pol.bounds[1])
        t.update({f"forced{i}": k for i, k in enumerate(keep)})
        return t

    def launch(self, forced=None, copies=True, table=None):
        """One launch -> dict of the outputs' E rows (the copies None without their pointers).  Checked here: the
        sentinels around every output, the copy tensors untouched without their pointers, every input bitwise as it went
        in.  table: a filled _lib.StepBlocks -- the block form."""
        T, keep = self.outputs(), []
        a = self.args(T, forced, copies, keep)
        ins = self.inputs(keep)
        before = {k: v.clone() for k, v in ins.items()}
        sentinels = {k: v.clone() for k, v in T.items()}
        if table is None:
            self.K.policy_step(a)
        else:
            a.obs = a.critic_obs = None
            self.K.policy_step_blocks(a, table)
        torch.cuda.synchronize()
        E, what = self.E, f"{self.name}{' (block form)' if table is not None else ''}"
        for k, v in T.items():
            sent = sentinels[k]
            assert torch.equal(_bits(v[:PAD]), _bits(sent[:PAD])), f"{what}: {k} written in front of its rows"
            assert torch.equal(_bits(v[PAD + E:]), _bits(sent[PAD + E:])), f"{what}: {k} written past its {E} rows"
            if not copies and k in ("obs_copy", "cobs_copy"):
                assert torch.equal(_bits(v), _bits(sent)), f"{what}: {k} written without its pointer"
        for k, v in ins.items():
            assert torch.equal(_bits(v), _bits(before[k])), f"{what}: the launch changed its input {k}"
        res = {k: v[PAD:PAD + E] for k, v in T.items()}
        if not copies:
            res["obs_copy"] = res["cobs_copy"] = None
        return res

    def got(self, res):
        """A launch's tensors as the dict policy_step_cases.judge takes."""
        n64 = lambda t: None if t is None else t.double().cpu().numpy()
        g = dict(logp=n64(res["logp"])[:, 0], value=n64(res["value"])[:, 0], obs_copy=n64(res["obs_copy"]),
                 cobs_copy=n64(res["cobs_copy"]))
        if self.adt == torch.float32:
            g["raw"], g["action"] = n64(res["raw"]), n64(res["act"])
        else:
            shape = (self.E,) if self.head == CAT else (self.E, self.aw)
            g["raw"], g["action"] = res["raw"].cpu().numpy().reshape(shape), res["act"].cpu().numpy().reshape(shape)
        return g

    def judged(self, g, launch):
        """The launch under policy_step_cases.judge: recorded, printed, asserted."""
        s = self.s
        wrong, fracs = cases.judge(s, g, launch)
        left = s.left_out(launch)
        WORST[(self.name, launch)] = (left, fracs)
        print(f"{self.name} {launch}: {left} of {self.E} rows left out, {wrong} actions differ, " +
              ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
        assert left <= cases.cap(self.E) and (left < self.E or self.E == 1)
        assert wrong == 0, f"{self.name} {launch}: {wrong} compared actions are not the float64 reference's"
        bad = {k: v for k, v in fracs.items() if not v <= 1.0}
        assert not bad, f"{self.name} {launch}: " + ", ".join(f"{k} {v:.3g} x bound" for k, v in bad.items())

    def both(self, forced=None):
        """The launch with the observation copies and the one without: the other outputs bitwise the same, the copies
        bitwise the inputs -> the launch the case asks for."""
        full, bare = self.launch(forced), self.launch(forced, copies=False)
        for k in ("raw", "act", "logp", "value"):
            assert torch.equal(_bits(full[k]), _bits(bare[k])), f"{self.name}: {k} differs without the copy pointers"
        assert torch.equal(_bits(full["obs_copy"]), _bits(self.obs)), f"{self.name}: obs_copy_out is not the input"
        assert torch.equal(_bits(full["cobs_copy"]), _bits(self.cobs)), f"{self.name}: critic_obs_copy_out is not the input"
        res = full if self.s.c["copies"] else bare
        if self.head in cases.DISCRETE:
            assert torch.equal(_bits(res["raw"]), _bits(res["act"])), f"{self.name}: raw_action_out is not action_out"
        return res


@pytest.mark.parametrize("name", list(cases.CASES))
def test_k6_sampled_launch_against_float64(name):
    d = Device(name)
    res = d.both()
    d.judged(d.got(res), "sampled")
    if d.head in (CAT, MCAT):
        top = torch.tensor(d.s.slices or (d.O,), device=d.dev)
        assert int(res["act"].min()) >= 0 and bool((res["act"] < top).all())
    elif d.head == BERN:
        assert set(np.unique(res["act"].cpu().numpy()).tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_k6_forced_launch_against_float64(name):
    d = Device(name)
    s = d.s
    res = d.both(s.forced)
    g = d.got(res)
    d.judged(g, "forced")
    f64, f32 = s.ref["forced"]
    if d.head == CAT:
        assert np.array_equal(g["raw"], np.clip(s.forced, 0, d.O - 1))
    elif d.head == MCAT:
        assert np.array_equal(g["raw"], cases.hd.multi_categorical_pick(s.forced, s.slices))
    else:
        assert np.array_equal(res["raw"].cpu().numpy(), np.asarray(s.forced, np.float32).reshape(d.E, d.O))   # bitwise
    bound = cases.k12_bound(f64["logp"], f32["logp"])
    if s.c["saturate"]:
        # forced classes below float32's eps: the clamp's log(eps32), within the tensor's bound
        sat = s.marked["saturated"]
        assert sat.sum() >= 2
        assert (np.abs(g["logp"][sat] - np.log(cases.EPS32)) <= bound[sat]).all(), g["logp"][sat]
    for regime, rows in s.marked.items():
        rows = rows if rows.ndim == 1 else rows.any(1)
        assert rows.any() and (np.abs(g["logp"] - f64["logp"])[rows] <= bound[rows]).all(), regime


def _scattered(n_blocks, rows, width, fill, dtype=torch.float32, dev="cuda"):
    """n_blocks contiguous [rows, width] views of one arena filled with `fill`, in an order that is not ascending in
    memory, 16-element gaps between them -> (blocks in table order, arena)."""
    stride = (rows * width + 16 + 3) // 4 * 4                # (every base 16-byte aligned)
    arena = torch.full((n_blocks * stride,), fill, dtype=dtype, device=dev)
    order = [(2 * b + 1) % n_blocks for b in range(n_blocks)]
    assert sorted(order) == list(range(n_blocks)) and order != sorted(order)
    return [arena[o * stride:o * stride + rows * width].view(rows, width) for o in order], arena


@pytest.mark.parametrize("name", cases.BLOCK_CASES)
def test_block_form_is_the_plain_form(name):
    d = Device(name)
    s, E = d.s, d.E
    rows, n_blocks = cases.BLOCK_SHAPES[E]
    assert rows % 16 and rows * n_blocks == E
    obs_b, _ = _scattered(n_blocks, rows, s.c["Ia"], 7.0)
    cobs_b, _ = _scattered(n_blocks, rows, s.c["Ic"], 7.0)
    for b in range(n_blocks):
        obs_b[b].copy_(d.obs[b * rows:(b + 1) * rows])
        cobs_b[b].copy_(d.cobs[b * rows:(b + 1) * rows])
    env_b, env_arena = _scattered(n_blocks, rows, d.aw, 7, d.adt)
    tb = d._lib.StepBlocks()
    tb.n_blocks, tb.rows_per_block = n_blocks, rows
    for b in range(n_blocks):
        tb.obs[b], tb.critic_obs[b], tb.env_action[b] = obs_b[b].data_ptr(), cobs_b[b].data_ptr(), env_b[b].data_ptr()
    for forced in (None, s.forced):
        want, got = d.launch(forced), d.launch(forced, table=tb)
        for k in OUTPUTS:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{name}: block form, {k} is not bitwise the plain form's"
        assert torch.equal(torch.cat(env_b, 0), want["act"]), f"{name}: the env's action blocks"
        for b in env_b:
            b.fill_(7)
        assert bool((env_arena == 7).all()), f"{name}: written between the env's action blocks"


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(d, change, message):
    """The launch of a valid case after `change(args)`: an error whose text holds `message`, no output written."""
    T, keep = d.outputs(), []
    a = d.args(T, None, True, keep)
    change(a)
    before = {k: v.clone() for k, v in T.items()}
    rc = d.lib.ppoaf_policy_step(C.byref(a), d.K.stream())
    text = d.lib.ppoaf_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    assert rc != 0 and message in text, (rc, text)
    for k, v in T.items():
        assert torch.equal(_bits(v), _bits(before[k])), f"refused launch wrote {k}"
    return text


def test_host_refuses_a_network_just_over_the_lds_limit():
    from ppo_and_friends_amd import _lib
    o = cases.OVER_LDS
    d = Device("gau8_e65_256x512")
    rng = np.random.default_rng(5)
    actor = ek.Net(rng, o["Ia"], o["pair"][0], o["Da"], d.O, "tanh", log_std=True)
    critic = ek.Net(rng, o["Ic"], o["pair"][1], o["Dc"], 1, "tanh")
    need = cases.lds_bytes(actor, critic)
    assert cases.LDS_LIMIT < need <= cases.LDS_LIMIT + 1024
    bucket = torch.from_numpy(np.concatenate([actor.flat(), critic.flat()])).to(d.dev)
    obs = torch.zeros(d.E, o["Ia"], device=d.dev)
    cobs = torch.zeros(d.E, o["Ic"], device=d.dev)

    def change(a):
        a.actor, a.critic = actor.desc(_lib, 0), critic.desc(_lib, actor.size())
        a.params, a.obs, a.critic_obs = bucket.data_ptr(), obs.data_ptr(), cobs.data_ptr()
        a.obs_copy_out = a.critic_obs_copy_out = None
    text = _refused(d, change, "LDS")
    assert str(need) in text, text


def test_host_refuses_out_dim_9():
    d = Device("cat8_e65_64x64")
    _refused(d, lambda a: setattr(a.actor, "out_dim", 9), "out_dim=9")


def test_host_refuses_an_nvec_that_does_not_sum_to_out_dim():
    d = Device("md32_e15_32x32")

    def change(a):
        a.action_slices[0], a.action_slices[1] = 3, 3
    _refused(d, change, "sum to 6")


def test_host_refuses_one_action_bound_without_the_other():
    d = Device("gau8_e65_256x512")
    _refused(d, lambda a: setattr(a, "act_hi", None), "both action bounds or neither")
    _refused(d, lambda a: setattr(a, "act_lo", None), "both action bounds or neither")


def test_no_env_is_accepted_and_writes_nothing():
    d = Device("mb4_e63_64x64")
    T, keep = d.outputs(), []
    a = d.args(T, None, True, keep)
    a.E = 0
    before = {k: v.clone() for k, v in T.items()}
    assert d.lib.ppoaf_policy_step(C.byref(a), d.K.stream()) == 0
    torch.cuda.synchronize()
    for k, v in T.items():
        assert torch.equal(_bits(v), _bits(before[k])), f"E = 0 wrote {k}"


# ---------------------------------------------------------------------------------------------------- the policy
POLICY_HEADS = {CAT: (CAT, 5, ()), GAU: (GAU, 3, ()), MCAT: (MCAT, 5, (3, 2)), BERN: (BERN, 5, ())}


@pytest.mark.parametrize("head", list(POLICY_HEADS))
def test_counters_through_the_policy(head):
    """PPO.rollout (update_mode="fused": K6+K7 steps it) at E = 6, T = 2, 32 / 64 wide, the bucket overwritten with a drawn,
    steered actor and critic (its layout held to the helper's by the descriptors the policy hands the kernel): the
    generator's offset advances by exactly T E (Categorical, Gaussian), T E D (MultiDiscrete) or T E n (MultiBinary);
    every kept buffered raw action of both steps is the restated draw at the offset the generator handed that step, from
    the float64 forward of the buffered observations; buffered log-probs, values and env actions are within bound."""
    import torch.nn as nn
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.fused_update import _describe
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete, MultiBinary, MultiDiscrete
    E, T, I = 6, 2, 7
    kind, O, slices = POLICY_HEADS[head]
    gauss = kind == GAU
    dev = torch.device("cuda", 0)
    bounds = cases.bounds_of(O) if gauss else None
    space = {CAT: lambda: Discrete(O), GAU: lambda: Box(bounds[0], bounds[1], (O,), np.float32),
             MCAT: lambda: MultiDiscrete(list(slices)), BERN: lambda: MultiBinary(O)}[kind]()
    env_gen = lambda: SyntheticFixedLengthEnv(E, I, space, T + 5, dev, reward="uniform", seed=13, term_prob=0.0)
    sp = Box(-np.inf, np.inf, (I,), np.float32)
    kw = lambda H: dict(hidden_size=H, hidden_depth=2, activation=nn.Tanh())
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(actor_kw_args=kw(32), critic_kw_args=kw(64)))}, device=dev,
              random_seed=6, normalize_obs=False, normalize_rewards=False, normalize_values=True, envs_per_proc=E,
              ts_per_rollout=T, batch_size=E * T, epochs_per_iter=1, max_ts_per_ep=T + 50, save_state=False,
              update_mode="fused")
    pol = ppo.policies["p"]
    assert pol.fused_step_unsupported_reason() == ""
    rng = np.random.default_rng(77)
    actor = ek.Net(rng, I, 32, 2, O, "tanh", log_std=gauss)
    critic = ek.Net(rng, I, 64, 2, 1, "tanh")
    cases.steer(actor, rng.normal(0, 1, (64, I)).astype(np.float32))
    from ppo_and_friends_amd import _lib
    da, _ = _describe(pol.actor, pol.policy_params, gauss)
    dc, _ = _describe(pol.critic, pol.policy_params, False)
    fields = lambda m: [(f, getattr(m, f)) for f, _ in _lib.MlpDesc._fields_ if f != "_pad"]
    assert fields(da) == fields(actor.desc(_lib, 0)) and fields(dc) == fields(critic.desc(_lib, actor.size()))
    bucket = np.concatenate([actor.flat(), critic.flat()])
    assert pol.policy_params.numel() == bucket.size
    with torch.no_grad():
        pol.policy_params.copy_(torch.from_numpy(bucket).to(dev))
    rs = ppo.value_normalizers["p"].running_stats
    rs.mean_t.fill_(cases.VN[0]); rs.var_t.fill_(cases.VN[1])
    gen = pol.actor.distribution.rng
    seed, off0 = gen.seed, gen.offset
    steps, inner = [], pol.rollout_step

    def logged(t, *a, **k):
        steps.append((t, gen.offset))
        return inner(t, *a, **k)
    pol.rollout_step = logged
    ppo.rollout()
    per_row = {MCAT: len(slices), BERN: O}.get(kind, 1)
    assert [t for t, _ in steps] == list(range(T)), "K6+K7 did not step the rollout"
    assert [o for _, o in steps] == [off0 + t * E * per_row for t in range(T)]
    assert gen.offset == off0 + T * E * per_row
    buf = pol.buffer
    obs = buf.observations.cpu().numpy().reshape(T, E, I)
    cobs = buf.critic_observations.cpu().numpy().reshape(T, E, I)
    raw = buf.raw_actions.cpu().numpy().reshape(T, E, -1)
    act = buf.actions.cpu().numpy().reshape(T, E, -1)
    logp = buf.log_probs.double().cpu().numpy().reshape(T, E)
    values = buf.values.double().cpu().numpy().reshape(T, E)
    compared, report = 0, {}
    for t in range(T):
        off = off0 + t * E * per_row
        r64, r32 = (cases.launch_reference(actor, critic, kind, slices, obs[t], cobs[t], seed, off,
                                           raw[t] if gauss or kind == BERN else raw[t].astype(np.int64), cases.VN, bounds, dt)
                    for dt in (np.float64, np.float32))
        fr = dict(logp=cases.worst(logp[t], r64["logp"], r32["logp"]), value=cases.worst(values[t], r64["value"], r32["value"]))
        if gauss:
            # the buffered raw action is the draw at its counter; the env action its squashed, rescaled image
            fr["raw"] = cases.worst(raw[t], r64["drawn"], r32["drawn"])
            fr["action"] = cases.worst(act[t], r64["action"], r32["action"])
            compared += E
        else:
            kept = ~cases.near_rows(kind, r64)
            assert (~kept).sum() <= cases.cap(E)
            wrong = (r64["drawn"].reshape(E, -1) != raw[t]).any(1) & kept
            assert not wrong.any(), f"step {t}: {int(wrong.sum())} buffered actions are not the draw at their counter"
            assert np.array_equal(act[t], raw[t])
            compared += int(kept.sum())
        report = {k: max(v, report.get(k, 0.0)) for k, v in fr.items()}
        print(f"step {t}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
        assert max(fr.values()) <= 1.0, (t, fr)
    WORST[(f"policy_{head}", "rollout")] = (T * E - compared, report)
    assert compared >= T * E - 2 * T and len(np.unique(raw.reshape(T * E, -1), axis=0)) > 1
