"""
-m gpu: ONE launch of K21 (csrc/lstm_policy_step.hip: the tensor-form and the block-form kernel, H = 32 / 64 / 128) against
its restatement in float64 (tests/helpers/lstm_step_cases.py: the network of oracle/lstm_update_oracle.py, the heads of
tests/helpers/head_draws.py on the Philox of tests/helpers/philox.py), at the shape edges of the kernel and with the
WEIGHTS DRAWN for logits of O(1) (at the default initialisation the head's gain leaves every distribution near uniform).
What the restatement states and no other test does: K21's own instantiation lstm_rows_forward<H, true> (the state stepped
in place, its second copies in the step's stored rows, the device `commit` byte), the four modes, the XCD-grouped tile
mapping beyond four tiles (E = 65 and 129), the heads fed from the rows in LDS, the value's denormalisation, which Philox
counter a row draws from (offset + e, a rollout's step t at off0 + t E + e) and that the draw is the inverse CDF / the
Box-Muller pair of the float64 distribution.  tests/test_lstm_step_oracle.py shows on the CPU that each of these, planted
as an error, is caught by a named case, and that every case meets its conditions.

Each case: ppoaf_lstm_policy_step launched directly on one bucket holding the case's parameters (actor, log_std, critic
at the offsets of lstm_update_oracle.bucket_tables, the segment sizes those of kernels.lstm_sizes).  Every output and
state tensor has 16 rows more than E holding a sentinel that must stay; every tensor a mode does not own must come back
bitwise as it went in.
  STEP sampled   actions float64's on the kept rows (near-tie rule of head_draws; the cap on rows left out is a condition of
                 the cases), raw == action (Categorical); logp (kept rows), values, the four states, Gaussian raw and env
                 action per tensor by the bound rule; the four stored rows bitwise the in-place states; the observation
                 copies bitwise the inputs;
  STEP forced    the float64 draw replayed with one class below 0 and one at or above out_dim (clamped), or |raw| ~ 4 in
                 the first rows (Gaussian); every row compared; the saturated case logs log(eps32);
  chain          three STEP launches on the same state tensors, fresh observations, offset += E: the third launch against
                 the float64 chain, the float32 chain as the floor;
  CRITIC_NEXT    commit 0, then 1: boot values; the critic's state bitwise unchanged / within bound; the actor's state
                 bitwise unchanged; exactly the terminated rows (row 0, the last live row, a row of tile >= 4) of the four
                 stored tensors zero;
  INFER          greedy and sampled: the env action (float64 argmax on the kept rows / the draw / tanh(mean) rescaled by
                 bound); the actor's state stepped, everything else untouched;
  MASK           the zeroing alone;
  block form     E = 65 as 13 x 5 and E = 129 as 43 x 3 row blocks, not ascending in memory: STEP and CRITIC_NEXT bitwise the
                 tensor form, the env's action blocks hold the action rows.
Bound per tensor (eval_kernels.k12_bound): |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| of the same
restatement in float32.
And once through the policy (PPO.rollout, an LSTM PPOPolicy, update_mode="fused"): see test_counters_through_the_policy.

Worst deviation / bound and rows left out per case and launch, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import lstm_update_oracle as lo

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_step_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

STEP, CRITIC_NEXT, INFER, MASK = 0, 1, 2, 3
SAMPLE, GREEDY = 0, 1
ACTS = {"relu": 0, "leaky_relu": 1, "tanh": 2}
PAD = 16                       # rows past the end of every output and state tensor
I_SENT, F_SENT = -77, -12345.0
WORST = {}                     # (case, launch) -> (rows left out, {tensor: deviation / bound})
STATE_KEYS, STORED_KEYS = cases.STATES, cases.STORED
OWNED = {STEP: {"raw", "act", "logp", "value", "obs_copy", "cobs_copy"} | set(STATE_KEYS) | set(STORED_KEYS),
         CRITIC_NEXT: {"boot", "critic_h", "critic_c"} | set(STORED_KEYS),
         INFER: {"act", "actor_h", "actor_c"},
         MASK: set(STORED_KEYS)}

MEASURED = """
per case and launch: rows left out by the near-tie rule / worst deviation over bound (the tensor it belongs to)
(this file alone: 42 passed in 4.5 s; tests/test_gpu_mat_step_float64.py: 20 passed in 5.5 s)
  e129_h128_gau5_bounds  sampled 0/0.172 logp | forced 0/0.092 logp | chain 0/0.107 logp | next0 0/0.021 values | next1 0/0.021 values | greedy 0/0.030 env_action | infer_sampled 0/0.041 env_action
  e129_in256_cat8        sampled 0/0.054 actor_h | forced 0/0.054 actor_h | chain 0/0.053 actor_h | next0 0/0.029 values | next1 0/0.044 critic_h | greedy 0/0.054 actor_h | infer_sampled 0/0.054 actor_h
  e15_cat3               sampled 0/0.014 values | forced 0/0.014 values | chain 0/0.014 critic_h | next0 0/0.006 values | next1 0/0.011 critic_c | greedy 0/0.011 actor_h | infer_sampled 0/0.011 actor_h
  e15_gau4               sampled 0/0.060 logp | forced 0/0.037 logp | chain 0/0.153 logp | next0 0/0.038 values | next1 0/0.038 values | greedy 0/0.044 env_action | infer_sampled 0/0.051 env_action
  e16_gau1               sampled 0/0.044 logp | forced 0/0.100 logp | chain 0/0.037 logp | next0 0/0.038 values | next1 0/0.038 values | greedy 0/0.025 env_action | infer_sampled 0/0.026 env_action
  e16_gau1_bounds        sampled 0/0.044 logp | forced 0/0.262 logp | chain 0/0.045 critic_h | next0 0/0.033 values | next1 0/0.033 values | greedy 0/0.023 env_action | infer_sampled 0/0.017 actor_h
  e17_cat3               sampled 0/0.016 actor_h | forced 0/0.016 actor_h | chain 0/0.013 actor_h | next0 0/0.010 values | next1 0/0.010 values | greedy 0/0.016 actor_h | infer_sampled 0/0.016 actor_h
  e17_gau8               sampled 0/0.029 values | forced 0/0.045 logp | chain 0/0.031 env_action | next0 0/0.014 values | next1 0/0.014 values | greedy 0/0.029 env_action | infer_sampled 0/0.029 env_action
  e17_wrap_cat8          sampled 0/0.035 values | forced 0/0.035 values | chain 0/0.058 values | next0 0/0.019 values | next1 0/0.019 values | greedy 0/0.015 actor_h | infer_sampled 0/0.015 actor_h
  e1_cat2                sampled 0/0.012 values | forced 0/0.012 values | chain 0/0.026 values | next0 0/0.001 values | next1 0/0.008 critic_h | greedy 0/0.005 actor_h | infer_sampled 0/0.005 actor_h
  e1_gau5_bounds         sampled 0/0.038 values | forced 0/0.133 logp | chain 0/0.038 values | next0 0/0.034 values | next1 0/0.034 values | greedy 0/0.009 env_action | infer_sampled 0/0.009 env_action
  e33_gau4_bounds        sampled 0/0.055 actor_h | forced 0/0.063 logp | chain 0/0.056 critic_h | next0 0/0.020 values | next1 0/0.034 critic_h | greedy 0/0.055 actor_h | infer_sampled 0/0.055 actor_h
  e33_gau5               sampled 0/0.066 env_action | forced 0/0.077 logp | chain 0/0.062 env_action | next0 0/0.066 values | next1 0/0.066 values | greedy 0/0.056 env_action | infer_sampled 0/0.066 env_action
  e33_h128_cat2          sampled 0/0.059 critic_h | forced 0/0.059 critic_h | chain 0/0.042 critic_h | next0 0/0.020 values | next1 0/0.036 critic_h | greedy 0/0.013 actor_h | infer_sampled 0/0.013 actor_h
  e65_h128_cat3          sampled 0/0.024 values | forced 0/0.024 values | chain 0/0.032 values | next0 0/0.035 values | next1 0/0.035 values | greedy 0/0.019 actor_h | infer_sampled 0/0.019 actor_h
  e65_in256_gau8_bounds  sampled 0/0.247 logp | forced 0/0.099 logp | chain 0/0.059 logp | next0 0/0.008 values | next1 0/0.009 critic_h | greedy 0/0.050 env_action | infer_sampled 0/0.049 actor_h
  policy_categorical     rollout 0/0.042 values
  policy_gaussian_bounds rollout 0/0.063 logp
  sat_cat5               sampled 0/0.038 logp | forced 0/0.017 values | chain 0/0.048 logp | next0 0/0.015 values | next1 0/0.015 values | greedy 0/0.007 actor_h | infer_sampled 0/0.007 actor_h
  small_h_cat3           sampled 0/0.043 values | forced 0/0.043 values | chain 0/0.026 critic_h | next0 0/0.027 values | next1 0/0.027 values | greedy 0/0.016 actor_h | infer_sampled 0/0.016 actor_h
worst per tensor: actor_c 0.040 (e33_gau4_bounds sampled), actor_h 0.055 (e33_gau4_bounds sampled), critic_c 0.048 (e33_gau4_bounds chain), critic_h 0.059 (e33_h128_cat2 sampled), env_action 0.066 (e33_gau5 sampled), logp 0.262 (e16_gau1_bounds forced), raw 0.035 (e33_gau5 sampled), values 0.066 (e33_gau5 next0)
(no row of any case and launch lies near a tie with these seeds; the block form is bitwise the tensor form at E = 65 and
E = 129, STEP sampled and forced and CRITIC_NEXT at commit 0 and 1; no kernel or host bug was found)
"""


def _report_lines():
    """One line per case: per launch the rows left out and the worst deviation / bound with its tensor; then the worst
    per tensor over all cases."""
    lines, per_tensor = [], {}
    for c in sorted({c for c, _ in WORST}):
        parts = []
        for (cc, l), (left, fr) in WORST.items():
            if cc != c:
                continue
            k = max(fr, key=fr.get)
            parts.append(f"{l} {left}/{fr[k]:.3f} {k}")
            for t, v in fr.items():
                t = t.replace("stored_", "")
                if v > per_tensor.get(t, (-1.0, ""))[0]:
                    per_tensor[t] = (v, f"{c} {l}")
        lines.append(f"  {c:22s} " + " | ".join(parts))
    lines.append("worst per tensor: " + ", ".join(f"{t} {v:.3f} ({w})" for t, (v, w) in sorted(per_tensor.items())))
    return lines


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = _report_lines()
    print("\nrows left out / worst deviation over bound (its tensor) per case and launch:\n" + "\n".join(lines))
    out = os.environ.get("PPOAF_K21_REPORT")
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _padded(rows, dev):
    """[E, w] float32 numpy -> [E + PAD, w] device tensor, the sentinel behind the rows."""
    t = torch.full((rows.shape[0] + PAD,) + tuple(rows.shape[1:]), F_SENT, dtype=torch.float32, device=dev)
    t[:rows.shape[0]] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
    return t


class Device:
    """The case on the device: one bucket holding the case's parameters, the descriptors over it, the launches."""

    def __init__(self, name):
        from ppo_and_friends_amd import _lib, kernels as K
        self.name, self.s = name, cases.steering(name)
        s, c = self.s, self.s.c
        self._lib, self.lib, self.K = _lib, _lib.load(), K
        dev = self.dev = torch.device("cuda", 0)
        self.E, self.H, self.O = c["E"], c["H"], c["head"][1]
        self.gauss = s.head == cases.GAU
        self.bucket = torch.as_tensor(s.params, dtype=torch.float32).to(dev)
        assert self.bucket.numel() == s.size
        mk = lambda n, seg: K.lstm_desc(n.in_dim, n.hidden, n.ff_hidden, n.ff_depth, n.out_dim, ACTS[n.activation], self.E, 1, seg)
        self.desc = dict(actor=mk(s.actor, self.bucket), critic=mk(s.critic, self.bucket[s.na:]))
        # the bucket's offsets: the oracle's tables, the segment sizes the library's own
        n_actor, n_critic = K.lstm_sizes(self.desc["actor"])[1], K.lstm_sizes(self.desc["critic"])[1]
        assert n_actor == lo.tensor_table(s.actor)[1] and n_critic == lo.tensor_table(s.critic)[1]
        assert s.na == n_actor + (lo._pad4(self.O) if self.gauss else 0) and s.size == s.na + n_critic
        first_critic = [o for tag, _, o, _ in s.tables if tag == "critic"][0]
        assert first_critic == s.na and s.na % 4 == 0
        self.log_std = None
        if self.gauss:
            tag, nm, at, _ = [t for t in s.tables if t[0] == "actor"][-1]
            assert nm == "log_std" and at == n_actor
            self.log_std = self.bucket[at:at + self.O]
        self.lo = self.hi = None
        if s.bounds is not None:
            self.lo = torch.full((self.O,), s.bounds[0], device=dev)
            self.hi = torch.full((self.O,), s.bounds[1], device=dev)
        self.vn = None
        if s.vn is not None:
            self.vn = (torch.tensor([s.vn[0]], dtype=torch.float32, device=dev), torch.tensor([s.vn[1]], dtype=torch.float32, device=dev))
        self.obs = [torch.from_numpy(s.obs[t]).to(dev).contiguous() for t in range(3)]
        self.cobs = [torch.from_numpy(s.cobs[t]).to(dev).contiguous() for t in range(3)]
        self.adt, self.aw = (torch.float32, self.O) if self.gauss else (torch.int64, 1)

    def fresh_state(self):
        return [_padded(t, self.dev) for t in self.s.state]

    def launch(self, mode, t=0, state=None, forced=None, commit=None, terminated=None, stored=None, infer_mode=SAMPLE,
               table=None):
        """One launch -> dict of device tensors (their first E rows; `state` holds the padded state tensors for a next
        launch).  Checked here: the sentinels past row E, and that every tensor the mode does not own is bitwise as it
        went in.  table: a filled _lib.LstmStepBlocks -- the block form (`terminated` then holds one byte per env)."""
        s, _lib, dev, E, H = self.s, self._lib, self.dev, self.E, self.H
        n = E + PAD
        a = _lib.LstmPolicyStepArgs()
        a.actor, a.critic = self.desc["actor"], self.desc["critic"]
        a.E, a.head_kind, a.mode, a.min_std, a.infer_mode = E, int(self.gauss), mode, cases.MIN_STD, infer_mode
        if self.gauss:
            a.log_std = self.log_std.data_ptr()
        if self.lo is not None:
            a.act_lo, a.act_hi = self.lo.data_ptr(), self.hi.data_ptr()
        a.seed, a.offset = s.seed, s.chain_offset(t)
        if self.vn is not None:
            a.normalize_values, a.vn_mean, a.vn_var = 1, self.vn[0].data_ptr(), self.vn[1].data_ptr()
        floats = lambda *w: torch.full((n,) + w, F_SENT, dtype=torch.float32, device=dev)
        acts = lambda: torch.full((n, self.aw), I_SENT, device=dev).to(self.adt)
        state = self.fresh_state() if state is None else state
        stored_t = [floats(H) for _ in range(4)] if stored is None else [_padded(x, dev) for x in stored]
        T = dict(raw=acts(), act=acts(), logp=floats(), value=floats(), boot=floats(), obs_copy=floats(s.c["Ia"]),
                 cobs_copy=floats(s.c["Ic"]))
        T.update(zip(STATE_KEYS, state))
        T.update(zip(STORED_KEYS, stored_t))
        before = {k: v.clone() for k, v in T.items()}
        if table is None:
            a.obs, a.critic_obs = self.obs[t].data_ptr(), self.cobs[t].data_ptr()
        for f, k in (("actor_h", "actor_h"), ("actor_c", "actor_c"), ("critic_h", "critic_h"), ("critic_c", "critic_c"),
                     ("actor_hidden_out", "stored_actor_h"), ("actor_cell_out", "stored_actor_c"),
                     ("critic_hidden_out", "stored_critic_h"), ("critic_cell_out", "stored_critic_c"),
                     ("raw_action_out", "raw"), ("action_out", "act"), ("logp_out", "logp"), ("value_out", "value"),
                     ("obs_copy_out", "obs_copy"), ("critic_obs_copy_out", "cobs_copy"), ("boot_value_out", "boot")):
            setattr(a, f, T[k].data_ptr())
        keep = []
        if forced is not None:
            f = torch.as_tensor(np.asarray(forced)).to(dev).to(self.adt).reshape(E, self.aw).contiguous()
            keep.append(f)
            a.forced_raw_action = f.data_ptr()
        if commit is not None:
            flag = torch.full((1,), int(commit), dtype=torch.uint8, device=dev)
            keep.append(flag)
            a.commit = flag.data_ptr()
        if terminated is not None:
            tm = torch.as_tensor(np.asarray(terminated, bool)).to(dev).contiguous()
            keep.append(tm)
            a.terminated = tm.data_ptr()
        if table is None:
            _lib.check(self.lib.ppoaf_lstm_policy_step(C.byref(a), self.K.stream()), "lstm_policy_step")
        else:
            _lib.check(self.lib.ppoaf_lstm_policy_step_blocks(C.byref(a), C.byref(table), self.K.stream()), "lstm_policy_step_blocks")
        torch.cuda.synchronize()
        what = f"{self.name} mode {mode}{' (block form)' if table is not None else ''}"
        for k, v in T.items():
            assert torch.equal(_bits(v[E:]), _bits(before[k][E:])), f"{what}: {k} written past its {E} rows"
            if k not in OWNED[mode]:
                assert torch.equal(_bits(v), _bits(before[k])), f"{what}: {k} is not this mode's to write"
        res = {k: v[:E] for k, v in T.items()}
        res["state"] = state
        return res

    # ---- a launch's tensors as the dict lstm_step_cases.judge takes
    def got(self, res, value="value"):
        n64 = lambda t: t.double().cpu().numpy()
        g = {k: n64(res[k]) for k in STATE_KEYS + STORED_KEYS}
        g["values"], g["logp"] = n64(res[value]), n64(res["logp"])
        if self.gauss:
            g["raw"], g["env_action"] = n64(res["raw"]), n64(res["act"])
            g["actions"] = g["raw"]
        else:
            g["raw"], g["env_action"] = res["raw"].cpu().numpy().reshape(-1), res["act"].cpu().numpy().reshape(-1)
            g["actions"] = g["env_action"]
        return g

    def judged(self, g, launch):
        """The launch under lstm_step_cases.judge: recorded, printed, asserted."""
        s = self.s
        wrong, fracs = cases.judge(s, g, launch)
        left = s.left_out(launch)
        WORST[(self.name, launch)] = (left, fracs)
        print(f"{self.name} {launch}: {left} of {self.E} rows left out, {wrong} actions differ, " +
              ", ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
        assert left <= cases.cap(self.E)
        assert wrong == 0, f"{self.name} {launch}: {wrong} compared actions are not the float64 reference's"
        bad = {k: v for k, v in fracs.items() if not v <= 1.0}
        assert not bad, f"{self.name} {launch}: " + ", ".join(f"{k} {v:.3g} x bound" for k, v in bad.items())


def _step_checks(d, res, t, what):
    """What every STEP launch owes beside the judged tensors."""
    for k in STATE_KEYS:
        assert torch.equal(_bits(res["stored_" + k]), _bits(res[k])), f"{what}: stored {k} is not the in-place state"
    assert torch.equal(_bits(res["obs_copy"]), _bits(d.obs[t])), f"{what}: obs_copy_out is not the input"
    assert torch.equal(_bits(res["cobs_copy"]), _bits(d.cobs[t])), f"{what}: critic_obs_copy_out is not the input"
    if not d.gauss:
        assert torch.equal(res["raw"], res["act"]), f"{what}: raw_action_out is not action_out"
        assert int(res["act"].min()) >= 0 and int(res["act"].max()) < d.O


@pytest.mark.parametrize("name", list(cases.CASES))
def test_k21_step_against_float64(name):
    d = Device(name)
    s, E, O = d.s, d.E, d.O
    # ---- sampled
    res = d.launch(STEP)
    _step_checks(d, res, 0, f"{name} sampled")
    d.judged(d.got(res), "sampled")
    # ---- forced
    res = d.launch(STEP, forced=s.forced)
    _step_checks(d, res, 0, f"{name} forced")
    g = d.got(res)
    d.judged(g, "forced")
    if d.gauss:
        assert np.array_equal(g["raw"], s.forced.astype(np.float64))
    else:
        assert np.array_equal(g["actions"], np.clip(s.forced, 0, O - 1))
    if s.c["saturate"]:
        # forced classes below float32's eps: the clamp's log(eps32), within the tensor's bound
        assert s.saturated.sum() >= 2
        f64, f32 = s.ref["forced"]
        bound = cases.k12_bound(f64["logp"], f32["logp"])[s.saturated]
        assert (np.abs(g["logp"][s.saturated] - np.log(cases.EPS32)) <= bound).all(), g["logp"][s.saturated]
    # ---- chain: three launches on the same state tensors
    state = d.fresh_state()
    for t in range(3):
        res = d.launch(STEP, t=t, state=state)
        _step_checks(d, res, t, f"{name} chain step {t}")
    d.judged(d.got(res), "chain")


@pytest.mark.parametrize("name", list(cases.CASES))
def test_k21_critic_next_infer_and_mask_against_float64(name):
    d = Device(name)
    s, E = d.s, d.E
    state0 = d.fresh_state()
    term = torch.as_tensor(s.terminated).to(d.dev)
    # ---- CRITIC_NEXT, commit 0 then 1 (the launch reads the next critic observation: the chain's second)
    for commit in (0, 1):
        res = d.launch(CRITIC_NEXT, t=1, commit=commit, terminated=s.terminated, stored=s.stored0)
        g = d.got(res, value="boot")
        d.judged(g, f"next{commit}")
        for k, k0 in zip(STATE_KEYS, state0):
            same = torch.equal(_bits(res[k]), _bits(k0[:E]))
            assert same == (commit == 0 or k.startswith("actor")), f"{name} commit {commit}: {k}"
        for k, before in zip(STORED_KEYS, s.stored0):
            rows = res[k]
            assert not rows[term].any(), f"{name}: {k}: a terminated row is not zero"
            assert torch.equal(_bits(rows[~term]), _bits(torch.from_numpy(before).to(d.dev)[~term])), f"{name}: {k}: a live row changed"
    # ---- MASK: the zeroing alone
    res = d.launch(MASK, terminated=s.terminated, stored=s.stored0)
    want = cases.masked_rows(s.stored0, s.terminated)
    for k in STORED_KEYS:
        assert np.array_equal(res[k].double().cpu().numpy(), want[k]), f"{name} MASK: {k}"
    # ---- INFER, greedy and sampled
    for launch, mode in (("greedy", GREEDY), ("infer_sampled", SAMPLE)):
        res = d.launch(INFER, infer_mode=mode)
        g = d.got(res)
        d.judged(g, launch)
        assert not torch.equal(_bits(res["actor_h"]), _bits(state0[0][:E])), f"{name} {launch}: the actor was not stepped"


def _scattered(n_blocks, rows, width, fill, dtype=torch.float32, dev="cuda"):
    """n_blocks contiguous [rows, width] views of one arena filled with `fill`, in an order that is not ascending in
    memory, 16-element gaps between them -> (blocks in table order, arena)."""
    stride = rows * width + 16
    arena = torch.full((n_blocks * stride,), fill, dtype=dtype, device=dev)
    order = [(2 * b + 1) % n_blocks for b in range(n_blocks)]
    assert sorted(order) == list(range(n_blocks)) and order != sorted(order)
    return [arena[o * stride:o * stride + rows * width].view(rows, width) for o in order], arena


@pytest.mark.parametrize("name", [n for n, c in cases.CASES.items() if c["E"] > 64])
def test_block_form_beyond_four_tiles_is_the_tensor_form(name):
    d = Device(name)
    s, E = d.s, d.E
    rows, n_blocks = {65: (13, 5), 129: (43, 3)}[E]
    obs_b, _ = _scattered(n_blocks, rows, s.c["Ia"], 7.0)
    cobs_b, _ = _scattered(n_blocks, rows, s.c["Ic"], 7.0)
    for b in range(n_blocks):
        obs_b[b].copy_(d.obs[0][b * rows:(b + 1) * rows])
        cobs_b[b].copy_(d.cobs[0][b * rows:(b + 1) * rows])
    env_b, env_arena = _scattered(n_blocks, rows, d.aw, 7, d.adt)
    tb = d._lib.LstmStepBlocks()
    tb.n_blocks, tb.rows_per_block = n_blocks, rows
    for b in range(n_blocks):
        tb.obs[b], tb.critic_obs[b], tb.env_action[b] = obs_b[b].data_ptr(), cobs_b[b].data_ptr(), env_b[b].data_ptr()
    keys = ("raw", "act", "logp", "value", "obs_copy", "cobs_copy") + STATE_KEYS + STORED_KEYS
    for forced in (None, s.forced):
        want, got = d.launch(STEP, forced=forced), d.launch(STEP, forced=forced, table=tb)
        for k in keys:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{name}: block form, {k} is not bitwise the tensor form's"
        assert torch.equal(torch.cat(env_b, 0), want["act"]), f"{name}: the env's action blocks"
        for b in env_b:
            b.fill_(7)
        assert bool((env_arena == 7).all()), f"{name}: written between the env's action blocks"
    # CRITIC_NEXT: one byte per env serves each of its blocks' rows
    term_env = s.terminated[:rows].copy()
    term_env[rows - 1] = True
    for b in range(n_blocks):
        tb.obs[b], tb.env_action[b] = None, None
    for commit in (0, 1):
        want = d.launch(CRITIC_NEXT, commit=commit, terminated=np.tile(term_env, n_blocks), stored=s.stored0)
        got = d.launch(CRITIC_NEXT, commit=commit, terminated=term_env, stored=s.stored0, table=tb)
        for k in ("boot", "critic_h", "critic_c") + STORED_KEYS:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{name}: block form CRITIC_NEXT, commit {commit}: {k}"
        assert float(want["stored_actor_h"][E - 1].abs().max()) == 0.0 and torch.isfinite(want["boot"]).all()


@pytest.mark.parametrize("head", ["categorical", "gaussian_bounds"])
def test_counters_through_the_policy(head):
    """PPO.rollout on an LSTM PPOPolicy (update_mode="fused": K21 steps it) at E = 6, T = 4, H = 32, no episode ending
    inside the rollout, the bucket overwritten with drawn parameters (its layout held to bucket_tables by data_ptr): the
    generator's offset advances by exactly T E; every kept buffered action is the restated draw at counter
    off0 + t E + e from the float64 recurrence over the buffered observations, starting at the state the networks held
    before step 0; buffered log-probs and values are within bound.  The buffered hidden rows at step t are the (h, c) the
    networks hold AFTER step t's forward -- the state the launch leaves (lstm_rows_forward<H, true> writes its final h and
    c to hn_row / cn_row; the reference clones hidden_state after the step's forward passes, ppo_policy.py:598-604) --
    not the state step t started from."""
    import torch.nn as nn
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    E, T, H, I, S = 6, 4, 32, 5, 3
    gauss = head != "categorical"
    O, Fa, Fc = (4, 16, 32) if gauss else (3, 32, 16)
    dev = torch.device("cuda", 0)
    space = Box(cases.BOUNDS[0], cases.BOUNDS[1], (O,), np.float32) if gauss else Discrete(O)
    env_gen = lambda: SyntheticFixedLengthEnv(E, I, space, T + 5, dev, reward="uniform", seed=13, term_prob=0.0)
    sp = Box(-np.inf, np.inf, (I,), np.float32)
    kw = lambda F: dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=F, ff_hidden_depth=1, activation=nn.Tanh())
    ppo = PPO(env_gen, {"p": (None, sp, sp, space, dict(ac_network=LSTMNetwork, actor_kw_args=kw(Fa), critic_kw_args=kw(Fc)))},
              device=dev, random_seed=6, normalize_obs=False, normalize_rewards=False, normalize_values=gauss, envs_per_proc=E,
              ts_per_rollout=T, batch_size=E * (T - S + 1), epochs_per_iter=1, max_ts_per_ep=T + 50, save_state=False,
              update_mode="fused")
    pol = ppo.policies["p"]
    assert pol.lstm_step_unsupported_reason() == ""
    actor, critic = lo.Net(I, H, Fa, 1, O, "tanh"), lo.Net(I, H, Fc, 1, 1, "tanh")
    kind = cases.GAU if gauss else cases.CAT
    tables, size = lo.bucket_tables(actor, critic, kind)
    params = cases.draw_params(actor, critic, kind, np.random.default_rng(77))
    assert pol.policy_params.numel() == size
    base = pol.policy_params.data_ptr()
    mods = pol.actor._hip_params() + ([pol.actor.distribution.log_std] if gauss else []) + pol.critic._hip_params()
    assert [((p.data_ptr() - base) // 4, tuple(p.shape)) for p in mods] == [(o, tuple(sh)) for _, _, o, sh in tables]
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(params, dtype=torch.float32, device=dev))
    vn = None
    if gauss:
        rs = ppo.value_normalizers["p"].running_stats
        rs.mean_t.fill_(cases.VN[0]); rs.var_t.fill_(cases.VN[1])
        vn = cases.VN
    rng = pol.actor.distribution.rng
    seed, off0 = rng.seed, rng.offset
    first, inner = [], pol.lstm_rollout_step

    def logged(t, *a, **k):
        if not first:                                        # the state the networks hold before step 0
            for net in (pol.actor, pol.critic):              # (the policy's own rule: reset when the batch size changes)
                if net.hidden_state is None or net.hidden_state[0].shape[1] != E:
                    net.reset_hidden_state(batch_size=E, device=dev)
            first.append([x.detach().clone().reshape(E, H).cpu().numpy() for x in list(pol.actor.hidden_state) + list(pol.critic.hidden_state)])
        first.append(t)
        return inner(t, *a, **k)
    pol.lstm_rollout_step = logged
    ppo.rollout()
    assert first[1:] == list(range(T)), "K21 did not step the rollout"
    assert rng.offset == off0 + T * E
    buf = pol.buffer
    obs = buf.observations.cpu().numpy().reshape(T, E, I)
    cobs = buf.critic_observations.cpu().numpy().reshape(T, E, I)
    assert not (buf.end_kind[:-1].cpu().numpy() != 0).any(), "an episode ended inside the rollout"
    raw = buf.raw_actions.cpu().numpy().reshape(T, E, -1)
    act = buf.actions.cpu().numpy().reshape(T, E, -1)
    logp = buf.log_probs.double().cpu().numpy().reshape(T, E)
    values = buf.values.double().cpu().numpy().reshape(T, E)
    hidden = {k: buf.hidden[b].double().cpu().numpy().reshape(T, E, H) for k, b in
              zip(STATE_KEYS, ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell"))}
    s64, s32 = tuple(first[0]), tuple(first[0])
    compared, report = 0, {}
    for t in range(T):
        forced = raw[t] if gauss else raw[t].reshape(E)
        r64, r32 = (cases.step_reference(params, actor, critic, kind, obs[t], cobs[t], st, seed, off0 + t * E, forced, vn,
                                         cases.BOUNDS if gauss else None, dt)
                    for dt, st in ((torch.float64, s64), (torch.float32, s32)))
        s64 = tuple(r64[k] for k in STATE_KEYS)
        s32 = tuple(r32[k].astype(np.float32) for k in STATE_KEYS)
        fr = dict(logp=cases.worst(logp[t], r64["logp"], r32["logp"]), values=cases.worst(values[t], r64["values"], r32["values"]))
        for k in STATE_KEYS:
            fr[k] = cases.worst(hidden[k][t], r64[k], r32[k])
        if gauss:
            # the buffered raw action is the draw at its counter; the env action its squashed, rescaled image
            fr["raw"] = cases.worst(raw[t], r64["drawn"], r32["drawn"])
            fr["env_action"] = cases.worst(act[t], r64["env_action"], r32["env_action"])
            compared += E
        else:
            kept = ~cases.hd.near_cdf_edge(r64["logits"], r64["gap"])
            assert (~kept).sum() <= cases.cap(E)
            wrong = (r64["drawn"] != raw[t].reshape(E)) & kept
            assert not wrong.any(), f"step {t}: {int(wrong.sum())} buffered actions are not the draw at their counter"
            assert np.array_equal(act[t], raw[t])
            compared += int(kept.sum())
        report = {k: max(v, report.get(k, 0.0)) for k, v in fr.items()}
        print(f"step {t}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
        assert max(fr.values()) <= 1.0, (t, fr)
    WORST[(f"policy_{head}", "rollout")] = (T * E - compared, report)
    assert compared >= T * E - 2 * T and (gauss or len(np.unique(raw)) > 1)
