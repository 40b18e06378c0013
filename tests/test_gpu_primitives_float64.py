"""
-m gpu: the standalone kernels K2-K11 -- what a run executes wherever a policy lies outside the fused chains, and the other
side of every "fused equals torch path" test -- each ONE launch in isolation against float64 (tests/helpers/
primitive_cases.py, held to the pinned oracles and to its own branch conditions by tests/test_primitives_oracle.py) at the
smallest shapes that reach every branch and every loop edge: the thread-count thresholds of the one-workgroup kernels, the
grid caps (2048 x 256 threads, 64 norm partials, 1024 column workgroups), the declared limits K = 64, D = 64, L = 1..16 and
D = 1024, NULL optional pointers, and Philox counters whose low word wraps inside the launch.

Bounds.  float32 outputs: per tensor |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| of the same
restatement in float32 (eval_kernels.k12_bound); the five loss scalars are one tensor.  float64 outputs (moment records,
count, the squared norm): primitive_cases.f64_sum_bound, derived there.  Integer and copied outputs: bit for bit.  Every
output lies in a NaN- / sentinel-filled buffer with a frame of 4 elements on either side that must stay as it was.
A sampled class is compared outside the rows head_draws.near_cdf_edge names (at most 2 per case).

Through ppo_and_friends_amd.kernels where its wrapper takes the output buffers; through the C ABI (ctypes) where the wrapper
allocates them, for NULL optional pointers and for ppoaf_adam_step_prenormed.

Worst deviation / bound per kernel, measured on the MI355X: see MEASURED below.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_draws as hd  # noqa: E402
import primitive_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED = """
worst deviation / bound per kernel (one run of this file; no sampled row fell under the near-edge rule)
  ppo_loss_fwd_bwd             0.250  adv_1e3: d_logp
  minibatch_gather             0.000  bit for bit
  scatter_rows_f32             0.000  bit for bit
  batch_moments                0.082  n3_W1025: record
  running_moments_integrate    0.004  R4_W300_fresh: mean
  normalize / denormalize      0.006  W5_var0: normalize
  minibatch_moments            0.001  B257_n770_direct: records
  categorical_eval             0.029  K64_n257: ent
  categorical_sample           0.013  K64_n300: probs
  gaussian_tanh_eval           0.250  D64_n1025: logp
  gaussian_tanh_sample         0.240  D64_n1_unit: logp
  icm_forward_loss             0.007  n1025_D65: intr
  mat_attention                0.098  L16_n2_D1024_full: y
  clip_adam_step               0.260  n524293: parameter step
  adam_step_prenormed          0.255  0_partials: parameter step
(0.25 is a tensor whose bound is its float32 floor and whose error is the float32 restatement's own)
"""

WORST = {}                     # kernel -> (worst fraction of its bound, where)
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
    print("\nworst deviation / bound per kernel:\n" + "\n".join(f"  {k:28s} {v[0]:.3f}  {v[1]}" for k, v in sorted(WORST.items())))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous()


def host(t):
    return t.detach().cpu().numpy()


class Framed:
    """A device buffer filled with NaN (floats) or SENT (integers): `.t` the tensor a kernel is given, PAD elements of
    frame on either side."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.n = int(np.prod(shape))
        fill = float("nan") if dtype.is_floating_point else SENT
        self.full = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device="cuda")
        self.t = self.full[PAD:PAD + self.n].view(shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).to(dtype).view(shape))

    def _blank(self, x):
        return torch.isnan(x) if x.dtype.is_floating_point else x == SENT

    def frame_ok(self):
        return bool(self._blank(self.full[:PAD]).all() and self._blank(self.full[PAD + self.n:]).all())

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
        self._add(what, P.frac(got, x64, x32))

    def absolute(self, what, got, want, bound):
        self._add(what, P.frac_abs(got, want, bound))

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


def call(K, name, *args):
    K.check(getattr(K._lib.load(), name)(*args, K.stream()), name)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ K2 + K3
@pytest.mark.parametrize("c", P.LOSS_CASES, ids=lambda c: c["name"])
def test_ppo_loss_fwd_bwd(K, c):
    cc, inp = P.loss_case(c), P.loss_inputs(c)
    B = cc["B"]
    d = {k: dev(inp[k]) for k in ("cur", "old", "adv", "values", "rtg")}
    ent = None if inp["ent"] is None else dev(inp["ent"])
    sc = Framed(8)
    out = {k: Framed(B) for k in ("d_logp", "d_entropy", "d_values")}
    if cc["null"] is None:
        K.ppo_loss_fwd_bwd(d["cur"], d["old"], d["adv"], ent, d["values"], d["rtg"], cc["normalize"], cc["clip"], cc["ent_w"], cc["kl"],
                           cc["huber"], cc["delta"], scalars=sc.t, d_logp=out["d_logp"].t, d_entropy=out["d_entropy"].t,
                           d_values=out["d_values"].t)
        torch.cuda.synchronize()
    else:
        o = [None if k == cc["null"] else K.ptr(out[k].t) for k in ("d_logp", "d_entropy", "d_values")]
        call(K, "ppoaf_ppo_loss_fwd_bwd", K.ptr(d["cur"]), K.ptr(d["old"]), K.ptr(d["adv"]), K.ptr(ent), K.ptr(d["values"]), K.ptr(d["rtg"]),
             B, int(cc["normalize"]), cc["clip"], cc["ent_w"], cc["kl"], int(cc["huber"]), cc["delta"], K.ptr(sc.t), *o)
    J = Judge("ppo_loss_fwd_bwd", c["name"])
    J.frames(scalars=sc, **out)
    s = sc.np().astype(np.float64)
    if cc["bad"]:
        J.exact("the non-finite flag", s[7] == 1.0)
        return J.done()
    r64, r32 = P.loss_ref(inp, c, np.float64), P.loss_ref(inp, c, np.float32)
    J.tensor("loss scalars", s[:5], r64["scalars"][:5], r32["scalars"][:5])
    J.tensor("adv mean", s[5:6], r64["scalars"][5:6], r32["scalars"][5:6])
    J.tensor("adv std", s[6:7], r64["scalars"][6:7], r32["scalars"][6:7])
    J.exact("the non-finite flag", s[7] == 0.0)
    for k, b in out.items():
        if k == cc["null"]:
            J.exact(f"{k} was not given", b.untouched())
        else:
            J.tensor(k, b.np(), r64[k], r32[k])
    J.done()


# ------------------------------------------------------------------------------------------------------------ K4
_F, _I64, _I32 = torch.float32, torch.int64, torch.int32
EIGHT = [(_F, 1), (_I64, 1), (_F, 54), (_F, 1000), (_I32, 3), (_F, 7), (_I64, 2), (_F, 2)]
GATHER_CASES = [dict(name="one_field", fields=[(_F, 1)], B=5, n_rows=9, row_map=False),
                dict(name="one_field_mapped", fields=[(_I64, 1)], B=300, n_rows=40, row_map=True),
                dict(name="eight_fields_grid_stride", fields=EIGHT, B=500, n_rows=600, row_map=True),
                dict(name="eight_fields_no_map", fields=EIGHT, B=37, n_rows=50, row_map=False)]


def _bytes(t):
    return host(t.contiguous().view(torch.uint8)).reshape(-1)


@pytest.mark.parametrize("c", GATHER_CASES, ids=lambda c: c["name"])
def test_minibatch_gather(K, c):
    rng = np.random.default_rng(len(c["fields"]) + c["B"])
    B, n_rows = c["B"], c["n_rows"]
    n_table = n_rows + 40 if c["row_map"] else n_rows
    row_map = rng.permutation(n_table)[:n_rows].astype(np.int32) if c["row_map"] else None
    perm = rng.integers(0, n_rows, B).astype(np.int64)
    perm[[1, B // 2, B - 1]] = (-1, n_rows, n_rows + 5)
    words = sum(w * (2 if dt == _I64 else 1) for dt, w in c["fields"])
    assert (B * words > 2048 * 256) == (c["name"] == "eight_fields_grid_stride") and (row_map is None or row_map.max() < n_table)
    pairs, want = [], []
    for dt, w in c["fields"]:
        src = rng.standard_normal((n_table, w)).astype(F32) if dt == _F else rng.integers(-2 ** 31, 2 ** 31 - 1, (n_table, w))
        src = dev(src).to(dt)
        dst = Framed((B, w), dt)
        pairs.append((src, dst))
        want.append(P.gather_ref(host(src), dst.np(), perm, row_map, n_rows))
    K.minibatch_gather([(s, d.t) for s, d in pairs], dev(perm), None if row_map is None else dev(row_map))
    torch.cuda.synchronize()
    J = Judge("minibatch_gather", c["name"])
    for i, ((src, dst), w) in enumerate(zip(pairs, want)):
        J.exact(f"field {i}", np.array_equal(_bytes(dst.t), np.ascontiguousarray(w).view(np.uint8).reshape(-1)))
        J.exact(f"field {i}: rows of perm entries outside the table", dst._blank(dst.t[[1, B // 2, B - 1]]).all().item())
        J.frames(**{f"field {i}": dst})
    J.done()


@pytest.mark.parametrize("mapped", [False, True])
def test_scatter_rows(K, mapped):
    rng = np.random.default_rng(4 + mapped)
    B, n_rows = 257, 280
    n_table = 300 if mapped else n_rows
    row_map = rng.permutation(n_table)[:n_rows].astype(np.int32) if mapped else None
    perm = rng.permutation(n_rows)[:B].astype(np.int64)
    perm[[0, 100, 256]] = (n_rows, -3, 2 ** 40)
    src = rng.standard_normal(B).astype(F32)
    dst = Framed(n_table)
    want = P.scatter_ref(src, dst.np(), perm, row_map, n_rows)
    K.scatter_rows_f32(dev(src), dev(perm), dst.t, None if row_map is None else dev(row_map))
    torch.cuda.synchronize()
    J = Judge("scatter_rows_f32", "mapped" if mapped else "direct")
    J.exact("rows", np.array_equal(dst.np().view(np.uint32), want.view(np.uint32)))
    J.exact("rows written", int(np.isfinite(dst.np()).sum()) == B - 3)
    J.frames(dst=dst)
    J.done()


# ------------------------------------------------------------------------------------------------------------ K5
@pytest.mark.parametrize("n,W", P.MOMENT_SHAPES)
def test_batch_moments(K, n, W):
    x = P.moments_data(n, W)
    out = Framed(1 + 2 * W, torch.float64)
    K.batch_moments(dev(x), W, out=out.t)
    torch.cuda.synchronize()
    rec, bound = P.moments_ref(x)
    J = Judge("batch_moments", f"n{n}_W{W}")
    J.exact("n", out.np()[0] == n)
    J.absolute("record", out.np(), rec, bound)
    J.frames(record=out)
    J.done()


@pytest.mark.parametrize("c", P.INTEGRATE_CASES, ids=lambda c: c["name"])
def test_running_moments_integrate(K, c):
    recs, mean, var, count = P.integrate_inputs(c)
    m, v, n = Framed(c["W"], init=mean), Framed(c["W"], init=var), Framed(1, torch.float64, init=np.array([count]))
    K.running_moments_integrate(dev(recs), m.t, v.t, n.t)
    torch.cuda.synchronize()
    J = Judge("running_moments_integrate", c["name"])
    J.frames(mean=m, var=v, count=n)
    if len(c["empty"]) == c["R"]:
        J.exact("an all-empty merge leaves the state", np.array_equal(m.np(), mean) and np.array_equal(v.np(), var) and n.np()[0] == count)
        return J.done()
    (m64, v64, n64), (m32, v32, _) = P.integrate_ref(recs, mean, var, count, np.float64), P.integrate_ref(recs, mean, var, count, np.float32)
    J.tensor("mean", m.np(), m64, m32)
    J.tensor("var", v.np(), v64, v32)
    J.absolute("count", n.np(), [n64], P.f64_sum_bound(c["R"] + 1, n64))
    J.done()


@pytest.mark.parametrize("c", P.NORMALIZE_CASES, ids=lambda c: c["name"])
def test_normalize_denormalize(K, c):
    x, mean, var = P.normalize_inputs(c)
    y, z = Framed(x.shape), Framed(x.shape)
    K.normalize(dev(x), dev(mean), dev(var), 1e-8, c["clip"], out=y.t)
    K.denormalize(dev(x), dev(mean), dev(var), 1e-8, out=z.t)
    torch.cuda.synchronize()
    J = Judge("normalize / denormalize", c["name"])
    J.tensor("normalize", y.np(), P.normalize_ref(x, mean, var, c["clip"], np.float64), P.normalize_ref(x, mean, var, c["clip"], np.float32))
    J.tensor("denormalize", z.np(), P.denormalize_ref(x, mean, var, np.float64), P.denormalize_ref(x, mean, var, np.float32))
    J.frames(normalize=y, denormalize=z)
    J.done()


@pytest.mark.parametrize("B,n,mapped", P.MB_MOMENT_CASES)
def test_minibatch_moments(K, B, n, mapped):
    rng = np.random.default_rng(B + n)
    n_table = n + 13
    data = (3.0 + 2.0 * rng.standard_normal(n_table)).astype(F32)
    row_map = rng.permutation(n_table)[:n + 5].astype(np.int32) if mapped else None
    perm = rng.permutation(n).astype(np.int64)
    nb = -(-n // B)
    out = Framed((nb, 3), torch.float64)
    K.minibatch_moments(dev(data), dev(perm), None if row_map is None else dev(row_map), B, out=out.t)
    torch.cuda.synchronize()
    rec, bound = P.minibatch_moments_ref(data, perm, row_map, B)
    J = Judge("minibatch_moments", f"B{B}_n{n}_{'mapped' if mapped else 'direct'}")
    J.exact("n of every record, the ragged one included", np.array_equal(out.np()[:, 0], rec[:, 0]) and rec[-1, 0] == n - (nb - 1) * B)
    J.absolute("records", out.np(), rec, bound)
    J.frames(records=out)
    J.done()


# ------------------------------------------------------------------------------------------------------------ K6 categorical
@pytest.mark.parametrize("Kc,n", P.CAT_EVAL_SHAPES)
def test_categorical_eval_fwd_bwd(K, Kc, n):
    i = P.categorical_inputs(Kc, n)
    z, a = dev(i["z"]), dev(i["a"])
    logp, ent, probs = Framed(n), Framed(n), Framed((n, Kc))
    call(K, "ppoaf_categorical_eval_fwd", K.ptr(z), K.ptr(a), n, Kc, K.ptr(logp.t), K.ptr(ent.t), K.ptr(probs.t))
    logp2, ent2 = Framed(n), Framed(n)
    call(K, "ppoaf_categorical_eval_fwd", K.ptr(z), K.ptr(a), n, Kc, K.ptr(logp2.t), K.ptr(ent2.t), None)
    J = Judge("categorical_eval", f"K{Kc}_n{n}")
    ref = lambda gl, ge, dt: P.categorical_eval_ref(i["z"], i["a"], gl, ge, dt)
    r64, r32 = ref(i["d_logp"], i["d_ent"], np.float64), ref(i["d_logp"], i["d_ent"], np.float32)
    for what, b in (("logp", logp), ("ent", ent), ("probs", probs)):
        J.tensor(what, b.np(), r64[what], r32[what])
    J.exact("probs_out NULL changes nothing", torch.equal(logp.t, logp2.t) and torch.equal(ent.t, ent2.t))
    J.frames(logp=logp, ent=ent, probs=probs, logp2=logp2, ent2=ent2)
    for what, gl, ge in (("d_logp and d_entropy", i["d_logp"], i["d_ent"]), ("d_logp only", i["d_logp"], None), ("d_entropy only", None, i["d_ent"])):
        dz, gl_t, ge_t = Framed((n, Kc)), None if gl is None else dev(gl), None if ge is None else dev(ge)
        call(K, "ppoaf_categorical_eval_bwd", K.ptr(probs.t), K.ptr(a), K.ptr(gl_t), K.ptr(ge_t), n, Kc, K.ptr(dz.t))
        J.tensor(f"d_logits, {what}", dz.np(), ref(gl, ge, np.float64)["d_logits"], ref(gl, ge, np.float32)["d_logits"])
        J.frames(d_logits=dz)
    J.done()


@pytest.mark.parametrize("c", P.CAT_SAMPLE_CASES, ids=lambda c: f"K{c['K']}_n{c['n']}")
def test_categorical_sample(K, c):
    z = P.categorical_sample_logits(c)
    n, Kc = z.shape
    a, logp, probs = Framed(n, torch.int64), Framed(n), Framed((n, Kc))
    K.categorical_sample(dev(z), P.SEED, P.OFFSET, action_out=a.t, logp_out=logp.t, probs_out=probs.t)
    torch.cuda.synchronize()
    r64, r32 = P.categorical_sample_ref(z, np.float64), P.categorical_sample_ref(z, np.float32)
    keep = ~hd.near_cdf_edge(z.astype(np.float64), r64["gap"])
    J = Judge("categorical_sample", f"K{Kc}_n{n}")
    print(f"categorical_sample K{Kc}_n{n}: {int((~keep).sum())} rows left out by the near-edge rule")
    J.exact("classes", np.array_equal(a.np()[keep], r64["a"][keep]))
    J.exact("classes in range", a.np().min() >= 0 and a.np().max() < Kc)
    J.tensor("logp", logp.np()[keep], r64["logp"][keep], r32["logp"][keep])
    J.tensor("probs", probs.np(), r64["probs"], r32["probs"])
    J.frames(action=a, logp=logp, probs=probs)
    J.done()


# ------------------------------------------------------------------------------------------------------------ K6 Gaussian
@pytest.mark.parametrize("D,n,shift", P.GAUSS_EVAL_SHAPES)
def test_gaussian_eval_fwd_bwd(K, D, n, shift):
    i = P.gaussian_inputs(D, n, shift)
    mean, ls, x = dev(i["mean"]), dev(i["log_std"]), dev(i["x"])
    logp, ent = Framed(n), Framed(n)
    call(K, "ppoaf_gaussian_tanh_eval_fwd", K.ptr(mean), K.ptr(ls), K.ptr(x), n, D, P.MIN_STD, K.ptr(logp.t), K.ptr(ent.t))
    J = Judge("gaussian_tanh_eval", f"D{D}_n{n}" + (f"_shift{shift}" if shift else ""))
    ref = lambda gl, ge, dt: P.gaussian_eval_ref(i["mean"], i["log_std"], i["x"], gl, ge, dt)
    r64, r32 = ref(None, None, np.float64), ref(None, None, np.float32)
    J.tensor("logp", logp.np(), r64["logp"], r32["logp"])
    J.tensor("ent", ent.np(), r64["ent"], r32["ent"])
    J.frames(logp=logp, ent=ent)
    for what, gl, ge in (("d_logp and d_entropy", i["d_logp"], i["d_ent"]), ("d_logp only", i["d_logp"], None), ("d_entropy only", None, i["d_ent"])):
        dm, dls, gl_t, ge_t = Framed((n, D)), Framed(D), None if gl is None else dev(gl), None if ge is None else dev(ge)
        call(K, "ppoaf_gaussian_tanh_eval_bwd", K.ptr(mean), K.ptr(ls), K.ptr(x), K.ptr(gl_t), K.ptr(ge_t), n, D, P.MIN_STD, K.ptr(dm.t),
             K.ptr(dls.t))
        g64, g32 = ref(gl, ge, np.float64), ref(gl, ge, np.float32)
        J.tensor(f"d_mean, {what}", dm.np(), g64["d_mean"], g32["d_mean"])
        J.tensor(f"d_log_std, {what}", dls.np(), g64["d_log_std"], g32["d_log_std"])
        J.exact(f"d_log_std under the floored std, {what}", (dls.np()[i["log_std"] == -8.0] == 0.0).all())
        J.frames(d_mean=dm, d_log_std=dls)
    J.done()


@pytest.mark.parametrize("D", [1, 64])
def test_gaussian_eval_bwd_without_rows_stores_zeros(K, D):
    dls = Framed(D)
    call(K, "ppoaf_gaussian_tanh_eval_bwd", None, None, None, None, None, 0, D, P.MIN_STD, None, K.ptr(dls.t))
    J = Judge("gaussian_tanh_eval", f"D{D}_n0")
    J.exact("d_log_std", (dls.np() == 0.0).all())
    J.frames(d_log_std=dls)
    J.done()


@pytest.mark.parametrize("D,n,bounded", P.GAUSS_SAMPLE_CASES)
def test_gaussian_tanh_sample(K, D, n, bounded):
    mean, ls, bounds = P.gaussian_sample_inputs(D, n, bounded)
    raw, act, logp = Framed((n, D)), Framed((n, D)), Framed(n)
    lo, hi = (dev(bounds[0]), dev(bounds[1])) if bounded else (None, None)
    mean_t, ls_t = dev(mean), dev(ls)
    call(K, "ppoaf_gaussian_tanh_sample", K.ptr(mean_t), K.ptr(ls_t), n, D, P.MIN_STD, K.ptr(lo), K.ptr(hi), P.SEED, P.OFFSET,
         K.ptr(raw.t), K.ptr(act.t), K.ptr(logp.t))
    r64, r32 = P.gaussian_sample_ref(mean, ls, bounds, np.float64), P.gaussian_sample_ref(mean, ls, bounds, np.float32)
    J = Judge("gaussian_tanh_sample", f"D{D}_n{n}_{'bounds' if bounded else 'unit'}")
    for what, b in (("raw", raw), ("action", act), ("logp", logp)):
        J.tensor(what, b.np(), r64[what], r32[what])
    J.frames(raw=raw, action=act, logp=logp)
    J.done()


# ------------------------------------------------------------------------------------------------------------ K8
@pytest.mark.parametrize("n,D", P.ICM_SHAPES)
def test_icm_forward_loss_fwd_bwd(K, n, D):
    pred, enc2 = P.icm_inputs(n, D)
    p, e, g = dev(pred), dev(enc2), dev(np.array([P.ICM_G], F32))
    r64, r32 = P.icm_ref(pred, enc2, np.float64), P.icm_ref(pred, enc2, np.float32)
    J = Judge("icm_forward_loss", f"n{n}_D{D}")
    for null in (None, "intr", "f_loss"):
        out = dict(rowsum=Framed(n), intr=Framed(n), f_loss=Framed(1))
        call(K, "ppoaf_icm_forward_loss_fwd", K.ptr(p), K.ptr(e), n, D, P.ICM_SCALE, K.ptr(out["rowsum"].t),
             *(None if k == null else K.ptr(out[k].t) for k in ("intr", "f_loss")))
        for k, b in out.items():
            if k == null:
                J.exact(f"{k} was not given", b.untouched())
            else:
                J.tensor(f"{k} ({null} NULL)", b.np(), r64[k], r32[k])
        J.frames(**out)
    for null in (None, "d_enc2"):
        out = dict(d_pred=Framed((n, D)), d_enc2=Framed((n, D)))
        call(K, "ppoaf_icm_forward_loss_bwd", K.ptr(p), K.ptr(e), n, D, K.ptr(g), K.ptr(out["d_pred"].t),
             None if null else K.ptr(out["d_enc2"].t))
        for k, b in out.items():
            if k == null:
                J.exact(f"{k} was not given", b.untouched())
            else:
                J.tensor(f"{k} ({null} NULL)", b.np(), r64[k], r32[k])
        J.frames(**out)
    J.done()


# ------------------------------------------------------------------------------------------------------------ K9
@pytest.mark.parametrize("c", P.attention_cases(), ids=P.attention_name)
def test_mat_attention_fwd_bwd(K, c):
    q, k, v, dy = P.attention_inputs(c)
    n_seq, L, D = q.shape
    dq_, dk_, dv_, dy_ = dev(q), dev(k), dev(v), dev(dy)
    y, probs = Framed(q.shape), Framed((n_seq, L, L))
    call(K, "ppoaf_mat_attention_fwd", K.ptr(dq_), K.ptr(dk_), K.ptr(dv_), n_seq, L, D, int(c["masked"]), K.ptr(y.t), K.ptr(probs.t))
    grads = dict(dq=Framed(q.shape), dk=Framed(q.shape), dv=Framed(q.shape))
    call(K, "ppoaf_mat_attention_bwd", K.ptr(dq_), K.ptr(dk_), K.ptr(dv_), K.ptr(probs.t), K.ptr(dy_), n_seq, L, D,
         *(K.ptr(grads[g].t) for g in ("dq", "dk", "dv")))
    r64, r32 = P.attention_ref(q, k, v, dy, c["masked"], np.float64), P.attention_ref(q, k, v, dy, c["masked"], np.float32)
    J = Judge("mat_attention", P.attention_name(c))
    for what, b in dict(y=y, probs=probs, **grads).items():
        J.tensor(what, b.np(), r64[what], r32[what])
        J.frames(**{what: b})
    if c["masked"]:
        iu = np.triu_indices(L, 1)
        J.exact("masked probabilities are zeros", (probs.np()[:, iu[0], iu[1]] == 0.0).all() and (probs.np()[:, 0, 0] == 1.0).all())
    J.done()


# ------------------------------------------------------------------------------------------------------------ K11
def _adam_state(p, g, m, v, step):
    return dict(p=Framed(len(p), init=p), g=Framed(len(g), init=g), m=Framed(len(m), init=m), v=Framed(len(v), init=v),
                step=Framed(1, torch.int64, init=np.array([step], np.int64)))


def _adam_judge(J, s, p, g, r64, r32):
    J.tensor("parameter step", s["p"].np().astype(np.float64) - p, r64["p"] - p, r32["p"] - p)
    J.tensor("m", s["m"].np(), r64["m"], r32["m"])
    J.tensor("v", s["v"].np(), r64["v"], r32["v"])
    J.exact("the gradients are only read", np.array_equal(s["g"].np(), g))
    J.frames(**s)


@pytest.mark.parametrize("c", P.ADAM_CASES, ids=lambda c: f"n{c['n']}_step{c['step']}_{c['clip']}")
def test_clip_adam_step(K, c):
    n = c["n"]
    p, g, m, v = P.adam_inputs(n, c["step"])
    max_norm = P.adam_max_norm(c["clip"], g, c["scale"])
    s = _adam_state(p, g, m, v, c["step"])
    scratch, norm = Framed(K.NORM_SCRATCH_DOUBLES, torch.float64), Framed(1)
    K.clip_adam_step(s["p"].t, s["g"].t, s["m"].t, s["v"].t, s["step"].t, dev(np.array([P.LR], F32)), scratch.t, P.BETA1, P.BETA2, 1e-5,
                     c["scale"], max_norm, norm.t if c["norm_out"] else None)
    torch.cuda.synchronize()
    r64, r32 = (P.adam_ref(p, g, m, v, c["step"] + 1, max_norm, c["scale"], dt) for dt in (np.float64, np.float32))
    J = Judge("clip_adam_step", f"n{n}")
    _adam_judge(J, s, p, g, r64, r32)
    J.exact("step counter", int(s["step"].np()[0]) == c["step"] + 1)
    J.absolute("scratch[0], the squared norm", scratch.np()[:1], [r64["sq"]], P.f64_sum_bound(n, r64["sq"]))
    if c["norm_out"]:
        J.tensor("norm", norm.np(), [r64["norm"]], [r32["norm"]])
    else:
        J.exact("grad_norm_out was not given", norm.untouched())
    J.frames(scratch=scratch, norm=norm)
    J.done()


@pytest.mark.parametrize("k", P.PRENORMED_PARTIALS)
def test_adam_step_prenormed(K, k):
    """The squared norm handed over is four times the gradients' own, so a kernel that took its own would show."""
    n, t = 1025, 7
    p, g, m, v = P.adam_inputs(n, t)
    rng = np.random.default_rng(k)
    sq_own = float((g.astype(np.float64) ** 2).sum())
    parts = 4.0 * sq_own * rng.dirichlet(np.ones(max(k, 1)))
    sq = math.fsum(parts) if k else 4.0 * sq_own
    max_norm = 0.37 * math.sqrt(sq)
    s = _adam_state(p, g, m, v, t)
    scratch, norm = Framed(2 + max(k, 64), torch.float64), Framed(1)
    if k:
        scratch.t[2:2 + k] = dev(parts)
    else:
        scratch.t[0] = sq
    lr = dev(np.array([P.LR], F32))
    call(K, "ppoaf_adam_step_prenormed", K.ptr(s["p"].t), K.ptr(s["g"].t), K.ptr(s["m"].t), K.ptr(s["v"].t), n, K.ptr(s["step"].t),
         K.ptr(lr), P.BETA1, P.BETA2, 1e-5, 1.0, max_norm, K.ptr(scratch.t), k, K.ptr(norm.t))
    r64, r32 = (P.adam_ref(p, g, m, v, t, max_norm, 1.0, dt, sq=sq) for dt in (np.float64, np.float32))
    J = Judge("adam_step_prenormed", f"{k}_partials")
    _adam_judge(J, s, p, g, r64, r32)
    J.exact("step counter is only read", int(s["step"].np()[0]) == t)
    J.absolute("scratch[0], the squared norm", scratch.np()[:1], [sq], P.f64_sum_bound(max(k, 1), sq) if k else 0.0)
    J.tensor("norm", norm.np(), [r64["norm"]], [r32["norm"]])
    J.exact("the partials are only read", k == 0 or np.array_equal(scratch.np()[2:2 + k], parts))
    J.frames(scratch=scratch, norm=norm)
    J.done()
