"""
-m gpu: the rollout-side kernels K1 (GAE and rewards-to-go, csrc/gae.hip), K13 (environment filters, csrc/env_filters.hip)
and K23 (rollout finish, csrc/rollout_finish.hip), each launch in isolation against the restatements of tests/helpers/
rollout_cases.py (held to the pinned oracles and to their own case conditions by tests/test_rollout_kernels_oracle.py).

K1, time-major: each of the four kernel instantiations the host chooses among -- chunked <16, 8, 4> and <32, 8, 8>,
streaming <1, 8, 256> and <4, 1, 1024> -- with E on its workgroup and lane edges and T on its chunk and tile edges, the
dense and the fixed-length form, episode ends steered onto the first / last step of a lane chunk and of a tile on the first
/ last column of a workgroup, and E = 2^20 with one array at a time off its 16-byte boundary (the <1, 8, 256> fallback).
K1, trajectory form: lengths around the 64-lane chunk, a zero length in the middle of the table, a start table out of
address order with sentinel gaps, rtg_out NULL, the entry point's refusals.  Bound per element: 2^-23 |x64| plus the float64
reordering bound of its chain (rollout_cases derives it); no element is left out.

K13: three consecutive steps from the initial state through kernels.obs_filter / reward_filter / env_filter_moments /
env_filter_apply, n over the 256-thread column walk's edges, stream subsets, data far from zero and with a spread near eps,
frozen statistics, clip only, one to three rank records.  float32 outputs and state: eval_kernels.k12_bound with the float32
run of the same text as the floor; the float64 reward state against quirk Q3's own sequential procedure with the propagated
bound of the pooled sums.

K23: 8 members, one of 16 blocks, grouped members with shuffled slot orders, E across the 256-thread workgroup, bit for bit
against numpy float32.

Every output lies in a NaN- / sentinel-filled buffer with a frame of 4 elements on either side that must stay as it was.

Worst deviation / bound per kernel and form, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rollout_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
worst deviation / bound per kernel and form (one run of this file: 185 tests in 12 s; no element or row left out)
  gae_rtg_tmajor chunk16 dense              0.500  chunk16_E8191_T129_dense: adv
  gae_rtg_tmajor chunk16 fixed              0.500  chunk16_E8191_T127_fixed: rtg
  gae_rtg_tmajor chunk32 dense              0.500  chunk32_E8193_T257_dense: rtg
  gae_rtg_tmajor chunk32 fixed              0.500  chunk32_E8223_T8_fixed: adv
  gae_rtg_tmajor stream1 dense              0.500  stream1_E1048578_T1_dense: rtg
  gae_rtg_tmajor stream1 dense misaligned   0.500  misaligned_rewards+4: adv
  gae_rtg_tmajor stream1 fixed              0.500  stream1_E1048577_T7_fixed: adv
  gae_rtg_tmajor stream4 dense              0.500  stream4_E1048576_T5_dense: adv
  gae_rtg_tmajor stream4 fixed              0.500  stream4_E1048580_T2_fixed: adv
  gae_rtg_traj                              0.496  n9_zero_mid: rtg
  gae_rtg_traj rtg_out NULL                 0.487  n3_zero_mid: adv
  env_filters R1                            0.372  n2_G3_W17_far: step 2 o out
  env_filters R3                            0.250  R3_unequal_n_obs: step 0 o out
  env_filters clip only                     0.000  bit for bit
  rollout_finish_rows                       0.000  bit for bit
(K1's 0.5 is the output's own float32 rounding, half an ulp against a bound of one: the float64 chains agree far inside
their part of the bound.  K13's 0.25 is a tensor whose bound is its float32 floor and whose error is the float32
restatement's own.)

Sharpness, on arithmetic variants of the library built aside and never kept: gamma for gamma * lambda in pass 1 of the
chunked kernel fails 21 of the chunk16 / chunk32 cases (T >= 127: the map's slope only meets a carry across waves), the
swapped arguments of one then(run, mk) 56 of them; clip_reward dropped at terminal ends of the streaming kernel fails the
three dense streaming cases whose clip range excludes zero; the weight n - i - 1 for n - i in K13's reward moments fails
every case with an updating reward stream; fmaf(r, w, intrinsic) in K23 fails E255 and E513.  The K1 tests of
tests/test_gpu_kernels.py at E >= 8192 (its streaming cases) pass under the first variant: none launches <32, 8, 8>.
"""

WORST = {}                     # kernel and form -> (worst fraction of its bound, where)
PAD, SENT = 4, -7
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    from ppo_and_friends_amd import kernels
    assert torch.cuda.is_available(), "GPU tests need a device"
    kernels._lib.load()
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst deviation / bound per kernel and form:\n" + "\n".join(f"  {k:36s} {v[0]:.3f}  {v[1]}" for k, v in sorted(WORST.items())))


def dev(a, shift=0):
    """The array on the device; shift: that many elements off the start of its allocation."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    if not shift:
        return t.cuda().contiguous()
    buf = torch.zeros(t.numel() + shift, dtype=t.dtype, device="cuda")
    view = buf[shift:].view(t.shape)
    view.copy_(t)
    return view


def host(t):
    return t.detach().cpu().numpy()


class Framed:
    """A device buffer filled with NaN (floats) or SENT (integers): `.t` the tensor a kernel is given, PAD elements of
    frame on either side (PAD floats are 16 bytes: `.t` keeps the allocation's alignment unless `shift` elements are added)."""

    def __init__(self, shape, dtype=torch.float32, init=None, shift=0):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.n, self.lo = int(np.prod(shape)), PAD + shift
        fill = float("nan") if dtype.is_floating_point else SENT
        self.full = torch.full((self.n + 2 * PAD + shift,), fill, dtype=dtype, device="cuda")
        self.t = self.full[self.lo:self.lo + self.n].view(shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).to(dtype).view(shape))

    def _blank(self, x):
        return torch.isnan(x) if x.dtype.is_floating_point else x == SENT

    def frame_ok(self):
        return bool(self._blank(self.full[:self.lo]).all() and self._blank(self.full[self.lo + self.n:]).all())

    def untouched(self):
        return bool(self._blank(self.full).all())

    def np(self):
        return host(self.t)


class Judge:
    """Collects one test's figures, prints the worst, then asserts (so a failing run still shows every figure)."""

    def __init__(self, kernel, case):
        self.kernel, self.case, self.worst, self.bad = kernel, case, (0.0, "-"), []

    def _add(self, what, f):
        if f > self.worst[0]:
            self.worst = (f, what)
        if not f <= 1.0:
            self.bad.append(f"{what}: {f:.3g} x bound")

    def tensor(self, what, got, x64, x32):
        self._add(what, R.frac(got, x64, x32))

    def absolute(self, what, got, want, bound):
        self._add(what, R.frac_abs(got, want, bound))

    def exact(self, what, ok):
        if not ok:
            self.bad.append(f"{what}: not exact")

    def frames(self, **bufs):
        for name, b in bufs.items():
            self.exact(f"frame of {name}", b.frame_ok())

    def done(self):
        print(f"{self.kernel} {self.case}: worst deviation / bound {self.worst[0]:.3f} ({self.worst[1]})")
        if self.worst[0] > WORST.get(self.kernel, (-1.0, ""))[0]:
            WORST[self.kernel] = (self.worst[0], f"{self.case}: {self.worst[1]}")
        assert not self.bad, f"{self.kernel} {self.case}: " + "; ".join(self.bad[:8])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F32 else a.dtype)


# ============================================================================================================== K1
_REFS = {}


def _run_tmajor(K, c, shifted=None):
    """One launch of case c; shifted = (array, bytes): that array lies so many bytes off its 16-byte boundary."""
    inp = R.tmajor_inputs(c)
    T, E = c["T"], c["E"]
    sh = lambda name: shifted[1] // (1 if name == "end_kind" else 4) if shifted and shifted[0] == name else 0      # in elements
    rew, val = dev(inp["rew"], sh("rewards")), dev(inp["val"], sh("values"))
    bv, br = dev(inp["bv"]), dev(inp["br"])
    ekd = dev(inp["ek"], sh("end_kind")) if c["dense"] else None
    adv, rtg = Framed((T, E), shift=sh("adv_out")), Framed((T, E), shift=sh("rtg_out"))
    arrays = dict(rewards=rew, values=val, adv_out=adv.t, rtg_out=rtg.t, **({"end_kind": ekd} if c["dense"] else {}))
    for name, t in arrays.items():                      # the alignment the case claims, hence the instantiation it runs
        want = sh(name) * t.element_size() % 16
        assert t.data_ptr() % 16 == want, f"{name} lies {t.data_ptr() % 16} bytes off a 16-byte boundary, the case says {want}"
    assert R.instantiation(E, shifted is None) == c["inst"]
    K.gae_rtg_tmajor(rew, val, bv, br, ekd, c["gamma"], c["lambd"], c["clip"], c["use_gae"], adv_out=adv.t, rtg_out=rtg.t)
    torch.cuda.synchronize()
    if c["name"] not in _REFS:                           # the misaligned launches share one case and its reference
        _REFS.clear()
        _REFS[c["name"]] = R.gae_tmajor_ref(inp["rew"], inp["val"], inp["bv"], inp["br"], inp["ek"], c["gamma"], c["lambd"], c["clip"], c["use_gae"])
    ref = _REFS[c["name"]]
    J = Judge(f"gae_rtg_tmajor {c['inst']} {'dense' if c['dense'] else 'fixed'}" + (" misaligned" if shifted else ""),
              c["name"] + (f"_{shifted[0]}+{shifted[1]}" if shifted else ""))
    J.absolute("adv", adv.np(), ref["adv"], ref["adv_bound"])
    J.absolute("rtg", rtg.np(), ref["rtg"], ref["rtg_bound"])
    J.frames(adv=adv, rtg=rtg)
    J.exact("the inputs are only read", np.array_equal(host(rew), inp["rew"]) and np.array_equal(host(val), inp["val"]))
    J.done()


@pytest.mark.parametrize("c", R.TMAJOR_CASES, ids=lambda c: c["name"])
def test_gae_tmajor(K, c):
    _run_tmajor(K, c)


@pytest.mark.parametrize("shifted", R.MISALIGNED, ids=lambda s: f"{s[0]}+{s[1]}")
def test_gae_tmajor_misaligned_arrays_take_the_one_column_kernel(K, shifted):
    _run_tmajor(K, R.MISALIGNED_CASE, shifted)


@pytest.mark.parametrize("c", R.TRAJ_CASES, ids=lambda c: c["name"])
def test_gae_traj(K, c):
    inp = R.traj_inputs(c)
    ref = R.gae_traj_ref(inp, c)
    adv, rtg = Framed(inp["N"]), Framed(inp["N"])
    K.gae_rtg_traj(dev(inp["rew"]), dev(inp["val"]), dev(inp["ev"]), dev(inp["er"]), dev(inp["start"]), dev(inp["lens"]), c["gamma"],
                   c["lambd"], c["clip"], c["use_gae"], adv_out=adv.t, rtg_out=rtg.t if c["rtg"] else None, compute_rtg=c["rtg"])
    torch.cuda.synchronize()
    used = inp["used"]
    J = Judge("gae_rtg_traj" + ("" if c["rtg"] else " rtg_out NULL"), c["name"])
    J.absolute("adv", adv.np()[used], ref["adv"][used], ref["adv_bound"][used])
    J.exact("adv: the gaps between the trajectories", np.isnan(adv.np()[~used]).all())
    if c["rtg"]:
        J.absolute("rtg", rtg.np()[used], ref["rtg"][used], ref["rtg_bound"][used])
        J.exact("rtg: the gaps between the trajectories", np.isnan(rtg.np()[~used]).all())
    else:
        J.exact("rtg_out was not given", rtg.untouched())
    J.frames(adv=adv, rtg=rtg)
    J.done()


@pytest.mark.parametrize("what,needle", [("no_rtg_without_gae", "rtg_out required"), ("negative_n_traj", "negative n_traj"),
                                         ("null_rewards", "null pointer"), ("null_adv_out", "null pointer"), ("null_traj_len", "null pointer")])
def test_gae_traj_refusals_write_nothing(K, what, needle):
    c = R.TRAJ_CASES[2]
    inp = R.traj_inputs(c)
    adv, rtg = Framed(inp["N"]), Framed(inp["N"])
    t = dict(rew=dev(inp["rew"]), val=dev(inp["val"]), ev=dev(inp["ev"]), er=dev(inp["er"]), start=dev(inp["start"]), lens=dev(inp["lens"]))
    p = {k: K.ptr(v) for k, v in t.items()}
    p.update(adv=K.ptr(adv.t), rtg=K.ptr(rtg.t), n=len(inp["lens"]), use_gae=1)
    p.update(dict(no_rtg_without_gae=dict(rtg=None, use_gae=0), negative_n_traj=dict(n=-1), null_rewards=dict(rew=None),
                  null_adv_out=dict(adv=None), null_traj_len=dict(lens=None))[what])
    lib = K._lib.load()
    rc = lib.ppoaf_gae_rtg_traj(p["rew"], p["val"], p["ev"], p["er"], p["start"], p["lens"], p["n"], 0.99, 0.95, 0, 0.0, 0.0, p["use_gae"],
                                p["adv"], p["rtg"], K.stream())
    torch.cuda.synchronize()
    assert rc != 0 and needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error().decode()
    assert adv.untouched() and rtg.untouched()


# ============================================================================================================== K13
class _RankState:
    """The device state of one rank: float32 statistics per observation stream, the float64 reward state."""

    def __init__(self, G, W, n, streams):
        self.obs = {s: (Framed(G * W, init=np.zeros(G * W)), Framed(G * W, init=np.ones(G * W)),
                        Framed(G * W, torch.float64, init=np.full(G * W, 1e-4))) for s in "oc" if s in streams}
        self.rew = (Framed(G * n, torch.float64, init=np.zeros(G * n)), Framed(G, torch.float64, init=np.zeros(G)),
                    Framed(G, torch.float64, init=np.ones(G)), Framed(G, torch.float64, init=np.full(G, 1e-4))) if "r" in streams else None

    def buffers(self):
        out = {f"{s}_{k}": b for s, st in self.obs.items() for k, b in zip(("mean", "var", "count"), st)}
        if self.rew:
            out.update({f"r_{k}": b for k, b in zip(("rr", "mean", "var", "count"), self.rew)})
        return out


def _filters(K, cc, rank, st, step, outs):
    """The three filter structs of one rank for one step (None: the stream is absent); the tensors they point at are kept
    alive in `keep`."""
    G, W = cc["G"], cc["W"]
    n = rank["o"].shape[0] // G
    keep, f = [], dict(o=None, c=None, r=None)
    for s in "oc":
        if s in cc["streams"]:
            x = dev(rank[s])
            keep.append(x)
            f[s] = K.obs_filter(x, outs[s].t, G, n, stats=tuple(b.t for b in st.obs[s]) if cc["normalize"] else None,
                                update=not (s in cc["frozen"] and step > 0), clip=cc["clip"], eps=R.K13_EPS)
    if "r" in cc["streams"]:
        rew, term, trunc = dev(rank["r"]), dev(rank["term"]), dev(rank["trunc"]) if cc["done2"] else None
        keep += [rew, term, trunc]
        f["r"] = K.reward_filter(rew, term, trunc, outs["r"].t, G, n, state=tuple(b.t for b in st.rew) if cc["normalize"] else None,
                                 update=not ("r" in cc["frozen"] and step > 0), clip=cc["rclip"], gamma=cc["gamma"], eps=R.K13_EPS)
    return f, keep


@pytest.mark.parametrize("c", R.K13_CASES, ids=lambda c: c["name"])
def test_env_filters(K, c):
    cc, steps = R.k13_case(c), R.k13_inputs(c)
    r64, r32 = R.k13_reference(c, np.float64), R.k13_reference(c, np.float32)
    G, W, n, streams = cc["G"], cc["W"], cc["n"], cc["streams"]
    n_ranks = len(cc["ranks"])
    live = [i for i, nr in enumerate(cc["ranks"]) if nr > 0]
    state = {i: _RankState(G, W, cc["ranks"][i], streams) for i in live}
    rec_len = K.env_filter_record_len(G, W if "o" in streams else 0, W if "c" in streams else 0, "r" in streams)
    J = Judge("env_filters " + ("clip only" if not cc["normalize"] else f"R{n_ranks}"), c["name"])
    for k, ranks in enumerate(steps):
        updating = cc["normalize"] and any(not (s in cc["frozen"] and k > 0) for s in streams)
        outs, filt, keep = {}, {}, []
        records = Framed((n_ranks, rec_len), torch.float64, init=np.zeros((n_ranks, rec_len)))
        for i in live:
            rows = G * cc["ranks"][i]
            outs[i] = {s: Framed((rows, W) if s in "oc" else rows) for s in streams}
            filt[i], kp = _filters(K, cc, ranks[i], state[i], k, outs[i])
            keep.append(kp)
            if updating:
                rec = Framed(rec_len, torch.float64)
                K.env_filter_moments(filt[i]["o"], filt[i]["c"], filt[i]["r"], G, cc["ranks"][i], rec.t)
                torch.cuda.synchronize()
                J.frames(record=rec)
                # what a frozen stream leaves unwritten is never read; zeros stand in for it in the gathered buffer
                records.t[i] = torch.nan_to_num(rec.t, nan=0.0)
                if i == 0:
                    _judge_record(J, cc, k, rec.np(), ranks[0])
        for i in live:
            K.env_filter_apply(filt[i]["o"], filt[i]["c"], filt[i]["r"], G, cc["ranks"][i], records.t if updating else None)
        torch.cuda.synchronize()
        o64, o32 = r64[k], r32[k]
        for s in "oc":
            if s not in streams:
                continue
            J.tensor(f"step {k} {s} out", outs[0][s].np(), o64[s], o32[s])
            if cc["normalize"]:
                mean, var, count = state[0].obs[s]
                J.tensor(f"step {k} {s} mean", mean.np(), o64[s + "_state"][0].reshape(-1), o32[s + "_state"][0].reshape(-1))
                J.tensor(f"step {k} {s} var", var.np(), o64[s + "_state"][1].reshape(-1), o32[s + "_state"][1].reshape(-1))
                cnt = np.repeat(o64[s + "_state"][2], W)
                J.absolute(f"step {k} {s} count", count.np(), cnt, R.f64_sum_bound(n_ranks + 1, cnt))
        if "r" in streams:
            J.tensor(f"step {k} reward out", outs[0]["r"].np(), o64["r"], o32["r"])
            if cc["normalize"]:
                rr, mean, var, count = state[0].rew
                st = o64["r_state"]
                J.absolute(f"step {k} reward mean", mean.np(), st["mean"], st["b_mean"])
                J.absolute(f"step {k} reward var", var.np(), st["var"], st["b_var"])
                J.absolute(f"step {k} reward count", count.np(), st["count"], 2.0 ** -50 * st["count"])
                J.absolute(f"step {k} running reward", rr.np(), st["rr"].reshape(-1), st["b_rr"].reshape(-1))
        for i in live:
            J.frames(**{f"rank {i} {s} out": b for s, b in outs[i].items()}, **{f"rank {i} {name}": b for name, b in state[i].buffers().items()})
            if i and cc["normalize"]:            # the ranks share the records, so they hold the same statistics bit for bit
                same = {name: b for name, b in state[i].buffers().items() if name != "r_rr"}
                J.exact(f"step {k}: rank {i} holds rank 0's statistics", all(torch.equal(b.t, state[0].buffers()[name].t) for name, b in same.items()))
        J.frames(records=records)
    J.done()


def _judge_record(J, cc, k, rec, rank0):
    """Rank 0's record of the moments launch: n, and the observation streams' (mean, M2) against float64."""
    G, W, n = cc["G"], cc["W"], cc["n"]
    J.exact(f"step {k} record n", rec[0] == n)
    off = 1
    for s in "oc":
        if s not in cc["streams"]:
            continue
        if not (s in cc["frozen"] and k > 0):
            mean, M2 = R.obs_records(rank0[s], G)
            S = np.abs(rank0[s].astype(np.float64)).reshape(G, n, W).sum(1)
            J.absolute(f"step {k} {s} record mean", rec[off:off + G * W], mean.reshape(-1), R.f64_sum_bound(n, S).reshape(-1) / n)
            J.absolute(f"step {k} {s} record M2", rec[off + G * W:off + 2 * G * W], M2.reshape(-1), R.f64_sum_bound(n, M2).reshape(-1))
        off += 2 * G * W


K13_REFUSALS = [("W0", "bad W"), ("null_stats", "null stats"), ("clip_lo_above_hi", "clip range"), ("reward_clip_lo_above_hi", "clip range"),
                ("reward_null_state", "null state"), ("G0", "G=0"), ("n0", "n=0"), ("nothing", "nothing to filter"),
                ("no_records", "needs R >= 1"), ("R0", "needs R >= 1"), ("null_record", "null record")]


@pytest.mark.parametrize("what,needle", K13_REFUSALS, ids=[w for w, _ in K13_REFUSALS])
def test_env_filter_refusals_leave_outputs_and_state(K, what, needle):
    cc = R.k13_case(dict(name="refusal", n=65, G=3, W=17))
    rank = R.k13_inputs(cc)[0][0]
    G, n = cc["G"], cc["n"]
    st = _RankState(G, cc["W"], n, "ocr")
    before = {name: b.np().copy() for name, b in st.buffers().items()}
    outs = {s: Framed((G * n, cc["W"]) if s in "oc" else G * n) for s in "ocr"}
    f, keep = _filters(K, cc, rank, st, 0, outs)
    rec = Framed(K.env_filter_record_len(G, cc["W"], cc["W"], True), torch.float64)
    lib, ref = K._lib.load(), lambda s: None if s is None else C.byref(s)
    gathered = dev(np.zeros(rec.n))
    records, n_rec = K.ptr(gathered), 1
    if what == "W0":
        f["o"].W = 0
    elif what == "null_stats":
        f["c"].var = None
    elif what == "clip_lo_above_hi":
        f["o"].has_clip, f["o"].clip_lo, f["o"].clip_hi = 1, 0.5, 0.25
    elif what == "reward_clip_lo_above_hi":
        f["r"].has_clip, f["r"].clip_lo, f["r"].clip_hi = 1, 0.5, 0.25
    elif what == "reward_null_state":
        f["r"].running_reward = None
    elif what == "G0":
        G = 0
    elif what == "n0":
        n = 0
    elif what == "nothing":
        f = dict(o=None, c=None, r=None)
    elif what == "no_records":
        records = None
    elif what == "R0":
        n_rec = 0
    rcs = []
    if what not in ("no_records", "R0"):
        rcs.append(lib.ppoaf_env_filter_moments(ref(f["o"]), ref(f["c"]), ref(f["r"]), G, n, None if what == "null_record" else K.ptr(rec.t), K.stream()))
        assert needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error().decode()
    if what != "null_record":
        rcs.append(lib.ppoaf_env_filter_apply(ref(f["o"]), ref(f["c"]), ref(f["r"]), G, n, records, n_rec, K.stream()))
        assert needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error().decode()
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs) and rec.untouched() and all(b.untouched() for b in outs.values())
    assert all(np.array_equal(b.np(), before[name]) and b.frame_ok() for name, b in st.buffers().items())


# ============================================================================================================== K23
@pytest.mark.parametrize("c", R.FINISH_CASES, ids=lambda c: c["name"])
def test_rollout_finish_rows(K, c):
    lib_mod = K._lib
    assert len(R.FINISH_MEMBERS) == lib_mod.FINISH_MAX_MEMBERS and max(n for n, _ in R.FINISH_MEMBERS) == lib_mod.ROW_BLOCKS_MAX
    E, steps = c["E"], R.finish_inputs(c)
    want = R.finish_blank_outs(c)
    # where no ends are written, ep_ts and the end_kind rows hold values of their own that must stay
    ts0 = (np.arange(E) % R.FINISH_MAX_TS).astype(np.int32)
    ep_ts = Framed(E, torch.int32, init=ts0)
    bufs = [{k: None if v is None else Framed(v.size, torch.float32 if v.dtype == F32 else torch.int8, init=v) for k, v in o.items()} for o in want]
    want_ts = ts0
    J = Judge("rollout_finish_rows", c["name"])
    for t, step in enumerate(steps):
        a = lib_mod.RolloutFinishArgs()
        a.n_members, a.E, a.max_ts_per_ep, a.ext_reward_weight = len(R.FINISH_MEMBERS), E, R.FINISH_MAX_TS, c["w"]
        a.write_ends, a.last_step = int(c["write_ends"]), int(step["last"])
        term, trunc = dev(step["term"]), dev(step["trunc"])
        a.terminated, a.truncated, a.ep_ts = term.data_ptr(), trunc.data_ptr() if c["truncated"] else None, ep_ts.t.data_ptr()
        keep = []
        for m, ((n, grouped), mem) in enumerate(zip(R.FINISH_MEMBERS, step["members"])):
            M = a.members[m]
            M.n_blocks, M.grouped = n, int(grouped)
            for s, b in enumerate(R.finish_slot_agent(m, n) if grouped else range(n)):
                M.slot_agent[s] = int(b)
            rew, nat = dev(mem["reward"]), dev(mem["natural"])
            intr = None if mem["intrinsic"] is None else dev(mem["intrinsic"])
            keep += [rew, nat, intr]
            for b in range(n):
                M.reward[b] = rew.data_ptr() + 4 * E * b
                M.natural[b] = nat.data_ptr() + 4 * E * b if mem["natural_given"][b] else None
            M.intrinsic = None if intr is None else intr.data_ptr()
            M.reward_out, M.end_kind_out = bufs[m]["reward"].t.data_ptr(), bufs[m]["end_kind"].t.data_ptr()
            M.natural_out = None if bufs[m]["natural"] is None else bufs[m]["natural"].t.data_ptr()
        K.rollout_finish_rows(a)
        torch.cuda.synchronize()
        want_ts, want = R.finish_ref(c, step, want_ts, want)
        J.exact(f"step {t} ep_ts", np.array_equal(ep_ts.np(), want_ts))
        for m, (o, w) in enumerate(zip(bufs, want)):
            for k, b in o.items():
                if b is not None:
                    J.exact(f"step {t} member {m} {k}", np.array_equal(bits(b.np()), bits(w[k])))
                    J.frames(**{f"member {m} {k}": b})
        J.exact(f"step {t}: the inputs are only read", all(np.array_equal(host(x), y) for x, y in ((term, step["term"]), (trunc, step["trunc"]))))
    J.frames(ep_ts=ep_ts)
    if not c["write_ends"]:
        J.exact("no ends written: ep_ts and the end_kind rows stay", np.array_equal(ep_ts.np(), ts0) and all(b["end_kind"].untouched() for b in bufs))
    J.done()
