"""
-m gpu: ONE K14 mini-batch against float64 autograd of the oracle (tests/helpers/icm_float64.py, pinned to g10_icm / g12_* /
g17 and checked without a GPU by tests/test_icm_float64_oracle.py) at the shape edges where kernels go wrong, through the C
ABI, on every form of K14:

  one_width  csrc/icm_update.hip, H 64 / 128: the split-wgrad chain as one launch (fuse_kernels 1, where
             ppoaf_icm_update_fuses_kernels says so) and as three, and the slab chain (split_workspace NULL)
  shapes     csrc/icm_update_shapes.hip: widths of its own (E, D, Mi, Mf), Discrete / Box / MultiDiscrete slices
  identity   the same file with an identity encoder

each with xcd_half 0 and 2 (the confined grid deals the tiles differently and leaves idle workgroups).  The rows of the
mini-batch are addressed in the four ways the drivers use (icm_float64.case: perm o row_map, a tail behind two full
mini-batches, tables in batch order from cursor 1, the same with B = 3 n); every table row that is not the mini-batch's
holds NaN, so a row taken from the wrong place shows.  Per form
  1. fused_adam 0: the gradient bucket (filled with NaN before: every element must be written), totals[0] (the loss),
     totals[1] == 1, cursor + 1, parameters bitwise unchanged;
  2. fused_adam 1 from a preset state (step 6, m and v on the gradient's scale): the parameter step, m, v, step 7, the
     bucket's padding unchanged in all three;
and once per case the rollout-time reward of the same rows.
Bound per tensor: |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| (the same oracle in float32 on the
CPU) where float32 itself cannot do better (oracle/k12_oracle.deviations); a tensor that is identically zero in float64
(icm_beta 0 / 1) must be exactly zero.

Worst deviation / bound per chain and form, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import icm_float64 as H  # noqa: E402

pytestmark = pytest.mark.gpu

ACTS = {"relu": nn.ReLU, "leaky_relu": nn.LeakyReLU, "tanh": nn.Tanh}
WORST = {}                     # (chain, form) -> (worst fraction of the bound, where)
LR, STEP0, BETAS, EPS = float(np.float32(3e-4)), 6, (0.9, 0.999), 1e-5

MEASURED = """
worst deviation / bound per chain and form (one run of the whole GPU suite; xcd_half 0 and 2 measured the same)
  one_width    split, one launch                          0.280  ow_in17 step: obs_encoder.enc_3.bias
  one_width    split, three launches                      0.445  fuzz_one_width_1 step: inv_model.sequential_net.3.bias
  one_width    split, three launches (fuse_kernels=1)     0.445  fuzz_one_width_1 step: inv_model.sequential_net.3.bias
  one_width    slabs                                      0.445  fuzz_one_width_1 step: inv_model.sequential_net.3.bias
  one_width    reward                                     0.020  ow_fuse_edge_in384 reward
  shapes       split                                      0.289  fuzz_shapes_2 gradient: inv_model.sequential_net.0.weight
  shapes       reward                                     0.064  fuzz_shapes_2 reward
  shapes_md    split                                      0.262  sh_md8x2 step: forward_model.sequential_net.3.bias
  shapes_md    reward                                     0.015  fuzz_shapes_4 reward
  identity     split                                      0.298  id_in2 step: inv_model.sequential_net.3.bias
  identity     reward                                     0.013  id_in128 reward
  identity_md  split                                      0.258  id_beta0 step: forward_model.sequential_net.3.bias
  identity_md  reward                                     0.009  fuzz_identity_4 reward
(the file run alone draws other hypothesis examples: 0.534 for shapes / split there, the inverse head's bias gradient)
"""


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{c:12s} {f:28s} {v[0]:.3f}  {v[1]}" for (c, f), v in sorted(WORST.items())]
    print("\nworst deviation / bound per chain and form:\n" + "\n".join(lines))
    out = os.environ.get("PPOAF_K14_REPORT")
    if out:
        with open(out, "w") as fh:
            json.dump({f"{c}/{f}": v for (c, f), v in sorted(WORST.items())}, fh, indent=1)


def _check(key, case_name, what, got, want64, want32, table):
    frac, where, bad = H.judge(got, want64, want32, table)
    if frac > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (frac, f"{case_name} {what}: {where}")
    assert not bad, f"{case_name} {key[1]} / {what}: " + "; ".join(bad[:6])


# ------------------------------------------------------------------------------------------------------ the harness
def _package_icm(c, dev):
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, Discrete, MultiDiscrete
    kind, n = c["action"]
    space = {"discrete": lambda: Discrete(n), "continuous": lambda: Box(-1.0, 1.0, (n,), np.float32),
             "multi": lambda: MultiDiscrete([n[1]] * n[0])}[kind]()
    if c["chain"] == "identity":
        E, D, (Mi, Mf) = 128, 0, c["widths"]
    else:
        E, D, Mi, Mf = (c["widths"],) * 4 if c["chain"] == "one_width" else c["widths"]
    icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (c["O"],), np.float32), action_space=space,
              activation=ACTS[c["act"]](), encoded_obs_dim=D, encoder_hidden_size=E, inverse_hidden_size=Mi,
              inverse_hidden_depth=c["depths"][0], forward_hidden_size=Mf, forward_hidden_depth=c["depths"][1])
    return icm.to(dev)


def _placement(c):
    """Where the B rows of the mini-batch sit: dict(n_table, n_rows, perm, row_map, cursor, stride, in_order, rows) with
    rows[s] the table row of the mini-batch's row s (icm_rows, csrc/icm_update_dev.hpp)."""
    B, mode = c["B"], c["rows"]
    rng = np.random.default_rng(c["seed"] + 2)
    if mode in ("perm", "tail"):
        cursor, stride = (0, B) if mode == "perm" else (2, B + 7)
        n_rows = (cursor + 1) * stride + 9
        n_table = n_rows + 5
        perm = rng.permutation(n_rows).astype(np.int64)
        row_map = rng.permutation(n_table)[:n_rows].astype(np.int32)
        rows = row_map[perm[cursor * stride:cursor * stride + B]].astype(np.int64)
        assert not np.array_equal(perm, np.arange(n_rows)) or n_rows < 3
        return dict(n_table=n_table, n_rows=n_rows, perm=perm, row_map=row_map, cursor=cursor, stride=stride, in_order=0, rows=rows)
    stride = B + 3 if mode == "order" else B
    return dict(n_table=2 * stride + 1, n_rows=2 * stride + 1, perm=None, row_map=None, cursor=1, stride=stride, in_order=1,
                rows=stride + np.arange(B, dtype=np.int64))


class Device:
    """The case on the device: the package's ICM holding the oracle's weights, the tables, the args of its chain."""

    def __init__(self, b):
        from ppo_and_friends_amd import _lib
        from ppo_and_friends_amd.fused_update import describe_icm_chain, icm_scratch_floats, icm_topology_args
        self.b, c = b, b.c
        self.lib = _lib.load()
        dev = self.dev = torch.device("cuda", 0)
        icm = self.icm = _package_icm(c, dev)
        icm.load_state_dict({k: v.detach().clone() for k, v in b.model.state_dict().items()})
        multi = c["action"][0] == "multi"
        topo, why = describe_icm_chain(icm, icm.action_dtype, multi_discrete=multi)
        assert why == "" and topo is not None, why
        chain = "identity" if topo.get("identity") else "shapes" if topo.get("general") else "one_width"
        assert chain == c["chain"], (chain, c["chain"])
        assert topo.get("n_action_slices", 0) == (c["action"][1][0] if multi else 0)
        self.topo, self.general = topo, bool(topo.get("general"))
        # the bucket is laid out as the reference lays its gradients
        base = icm.flat_params.data_ptr()
        assert topo["bucket_total"] == b.size == icm.flat_params.numel()
        for (_, name, off, shape), (pname, p) in zip(b.table, icm.named_parameters()):
            assert name == pname and (p.data_ptr() - base) // 4 == off and tuple(p.shape) == shape, name
        assert np.array_equal(icm.flat_params.detach().cpu().double().numpy()[~b.pad], b.params[~b.pad])
        self.p0 = icm.flat_params.detach().clone()
        # ---- tables: NaN wherever the mini-batch has no row
        pl = self.pl = _placement(c)
        B, O = c["B"], c["O"]
        rows = torch.as_tensor(pl["rows"])
        obs1, obs2 = (torch.full((pl["n_table"], O), float("nan")) for _ in range(2))
        obs1[rows], obs2[rows] = torch.as_tensor(b.obs1), torch.as_tensor(b.obs2)
        act = torch.as_tensor(b.act)
        if act.dtype == torch.int64:
            table_act = torch.zeros((pl["n_table"],) + tuple(act.shape[1:]), dtype=torch.int64)
        else:
            table_act = torch.full((pl["n_table"], act.shape[1]), float("nan"))
        table_act[rows] = act
        if c["action"][0] == "discrete":
            table_act, act = table_act.reshape(-1), act.reshape(-1)              # int64 [n_rows]
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
        nT, total = (B + 15) // 16, b.size
        n_act, n_denc = icm_scratch_floats(topo, B)
        k = self.keep = dict(
            act=z(n_act), denc=z(n_denc), m=z(total), v=z(total), step=z(1, torch.int64), lr=torch.full((1,), LR, device=dev),
            cursor=z(1, torch.int64), parts=z(2 * (nT + 1)), totals=z(2, torch.float64),
            obs1=obs1.to(dev).contiguous(), obs2=obs2.to(dev).contiguous(), actions=table_act.to(dev).contiguous(),
            perm=None if pl["perm"] is None else torch.as_tensor(pl["perm"]).to(dev),
            row_map=None if pl["row_map"] is None else torch.as_tensor(pl["row_map"]).to(dev),
            # the reward entry point takes the rows themselves
            r_obs1=torch.as_tensor(b.obs1).to(dev).contiguous(), r_obs2=torch.as_tensor(b.obs2).to(dev).contiguous(),
            r_actions=act.to(dev).contiguous())
        a = self.args = icm_topology_args(topo)
        a.params, a.grads = icm.flat_params.data_ptr(), icm.flat_grads.data_ptr()
        a.exp_avg, a.exp_avg_sq, a.step_count, a.lr = (k[x].data_ptr() for x in ("m", "v", "step", "lr"))
        a.beta1, a.beta2, a.adam_eps, a.grad_scale = BETAS[0], BETAS[1], EPS, 1.0
        a.obs, a.next_obs, a.actions = k["obs1"].data_ptr(), k["obs2"].data_ptr(), k["actions"].data_ptr()
        a.perm = None if k["perm"] is None else k["perm"].data_ptr()
        a.row_map = None if k["row_map"] is None else k["row_map"].data_ptr()
        a.n_rows, a.inputs_in_batch_order = pl["n_rows"], pl["in_order"]
        a.cursor, a.B, a.batch_stride = k["cursor"].data_ptr(), B, pl["stride"]
        a.icm_beta, a.fused_adam = b.beta, 0
        a.act_scratch, a.denc_scratch = k["act"].data_ptr(), k["denc"].data_ptr()
        a.loss_partials, a.totals = k["parts"].data_ptr(), k["totals"].data_ptr()
        if self.general:
            need = C.c_int64(0)
            _lib.check(self.lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)), "icm_shapes_workspace_bytes")
            k["ws"] = z(int(need.value), torch.uint8)
            a.workspace, a.workspace_bytes = k["ws"].data_ptr(), k["ws"].numel()
        else:
            k["slabs"] = z((2 * nT, total))
            a.slabs = k["slabs"].data_ptr()
            a.split_workspace, a.split_workspace_bytes, a.fuse_kernels = None, 0, 0

    def forms(self):
        """[(form, set-up of the args)]: the shapes chain has one; the one-width chain three."""
        if self.general:
            return [("split", lambda: None)]
        return [("split fuse_kernels=1", lambda: self._split(1)), ("split fuse_kernels=0", lambda: self._split(0)),
                ("slabs", lambda: self._split(None))]

    def _split(self, fuse):
        from ppo_and_friends_amd import _lib
        a, k = self.args, self.keep
        a.split_workspace, a.split_workspace_bytes, a.fuse_kernels = None, 0, 0
        if fuse is None:
            return
        a.fuse_kernels = fuse
        need = C.c_int64(0)
        _lib.check(self.lib.ppoaf_icm_update_split_workspace_bytes(C.byref(a), C.byref(need)), "icm_update_split_workspace_bytes")
        k["ws"] = torch.zeros(int(need.value), dtype=torch.uint8, device=self.dev)
        a.split_workspace, a.split_workspace_bytes = k["ws"].data_ptr(), k["ws"].numel()

    def fuses(self):
        return (not self.general) and self.lib.ppoaf_icm_update_fuses_kernels(C.byref(self.args)) == 1

    def launch(self, fused_adam, m0=None, v0=None):
        """One mini-batch from the case's starting state -> (grads, params, m, v) as float64 arrays."""
        from ppo_and_friends_amd import _lib, kernels as K
        from ppo_and_friends_amd.fused_update import FusedIcmUpdate
        a, k, icm = self.args, self.keep, self.icm
        with torch.no_grad():
            icm.flat_params.copy_(self.p0)
            icm.flat_grads.fill_(float("nan"))                   # every gradient element must be written
        k["m"].zero_() if m0 is None else k["m"].copy_(torch.from_numpy(m0))
        k["v"].zero_() if v0 is None else k["v"].copy_(torch.from_numpy(v0))
        k["step"].fill_(STEP0 if fused_adam else 0)
        k["cursor"].fill_(self.pl["cursor"])
        for name in ("totals", "parts", "act", "denc", "ws", "slabs"):
            if name in k:
                k[name].zero_()                                  # (the single launch's records are tagged with the cursor)
        a.fused_adam = fused_adam
        st = K.stream()
        if self.general:
            _lib.check(self.lib.ppoaf_icm_shapes_fwd_bwd(C.byref(a), st), "icm_shapes_fwd_bwd")
            _lib.check(self.lib.ppoaf_icm_shapes_wgrad(C.byref(a), st), "icm_shapes_wgrad")
        else:
            single = self.fuses()
            _lib.check(self.lib.ppoaf_icm_update_fwd_bwd(C.byref(a), st), "icm_update_fwd_bwd")
            _lib.check(self.lib.ppoaf_icm_update_reduce(C.byref(a), st), "icm_update_reduce")
            if single:                                           # a bounded wait that ran out: reported, no second try
                torch.cuda.synchronize()
                if int(k["ws"][:4].view(torch.int32).item()) != 0:
                    raise _lib.PpoafError(FusedIcmUpdate._FUSED_FAILURE)
        torch.cuda.synchronize()
        return [t.detach().double().cpu().numpy() for t in (icm.flat_grads, icm.flat_params, k["m"], k["v"])]

    def reward(self):
        from ppo_and_friends_amd import _lib, kernels as K
        from ppo_and_friends_amd.fused_update import icm_topology_args
        B, k = self.b.c["B"], self.keep
        r = icm_topology_args(self.topo)
        r.params, r.act_scratch = self.icm.flat_params.data_ptr(), k["act"].data_ptr()
        r.obs, r.next_obs, r.actions = k["r_obs1"].data_ptr(), k["r_obs2"].data_ptr(), k["r_actions"].data_ptr()
        r.B, r.batch_stride, r.n_rows, r.fused_adam = B, B, B, 0
        out = torch.full((B,), float("nan"), device=self.dev)
        entry = "ppoaf_icm_shapes_intrinsic_reward" if self.general else "ppoaf_icm_intrinsic_reward"   # PPOPolicy._fused_intrinsic_reward
        with torch.no_grad():
            self.icm.flat_params.copy_(self.p0)
        _lib.check(getattr(self.lib, entry)(C.byref(r), H.REWARD_SCALE / 2.0, out.data_ptr(), K.stream()), entry)
        torch.cuda.synchronize()
        return out.double().cpu().numpy()


def run_case(name, c, expect_single_launch=None):
    """expect_single_launch: None = what the shapes promise (H 128, at most 512 rows, an observation the LDS has room for:
    asserted for obs_dim <= 128); True / False = asserted as given."""
    b = H.Built(c)
    d = Device(b)
    chain, B = H.label(c), c["B"]
    m0, v0 = H.preset_state(c, b.r64["grads"], b.pad)
    want = H.adam(b.params, b.r64["grads"], m0, v0, STEP0, LR, BETAS, EPS)
    want32 = H.adam(b.params, b.r32["grads"], m0, v0, STEP0, LR, BETAS, EPS, dtype=torch.float32)
    p0 = d.p0.double().cpu().numpy()
    for form, setup in d.forms():
        setup()
        if form == "split fuse_kernels=1":
            single = d.fuses()
            if expect_single_launch is not None:
                assert single == expect_single_launch, (name, single)
            elif c["widths"] == 64 or B > 512:
                assert not single, name
            elif c["O"] <= 128:
                assert single, name
            form = "split, one launch" if single else "split, three launches (fuse_kernels=1)"
        elif form == "split fuse_kernels=0":
            assert not d.fuses()
            form = "split, three launches"
        for half in (0, 2):
            d.args.xcd_half = half
            key = (chain, f"{form}, xcd_half {half}")
            # ---- 1. the gradient of the mini-batch
            grads, params, _, _ = d.launch(0)
            k = d.keep
            _check(key, name, "gradient", grads, b.r64["grads"], b.r32["grads"], b.table)
            _check(key, name, "loss", [float(k["totals"][0])], b.r64["loss"], b.r32["loss"], H.LOSS)
            assert float(k["totals"][1]) == 1.0 and int(k["cursor"].item()) == d.pl["cursor"] + 1 and int(k["step"].item()) == 0
            assert np.array_equal(params, p0), f"{name} {key[1]}: parameters changed without fused_adam"
            # ---- 2. one full step from a non-zero optimiser state
            _, params, m, v = d.launch(1, m0, v0)
            _check(key, name, "step", params - b.params, want[0] - b.params, want32[0] - b.params, b.table)
            _check(key, name, "m", m, want[1], want32[1], b.table)
            _check(key, name, "v", v, want[2], want32[2], b.table)
            assert int(k["step"].item()) == STEP0 + 1 and int(k["cursor"].item()) == d.pl["cursor"] + 1
            assert float(k["totals"][1]) == 1.0
            for what, got, start in (("params", params, p0), ("m", m, m0), ("v", v, v0)):
                assert np.array_equal(got[b.pad], np.asarray(start, dtype=np.float64)[b.pad]), f"{name} {key[1]}: padding of {what} written"
    # ---- 3. the rollout-time reward of the same rows
    _check((chain, "reward"), name, "reward", d.reward(), b.r64["reward"], b.r32["reward"], [("", "reward", 0, (B,))])


# ------------------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("name", sorted(H.CASES))
def test_k14_minibatch_against_float64(name):
    run_case(name, H.CASES[name])


def test_one_width_at_the_edge_of_the_single_launch():
    """H 128: the largest obs_dim for which ppoaf_icm_update_fuses_kernels still answers 1 (the three phases' LDS beside the
    input tile), and the next one -- found by asking, with the arguments of a real mini-batch."""
    def fuses(O):
        b = H.Built(H.case("one_width", O, 18, 128, seed=1200))
        d = Device(b)
        d._split(1)
        return d.fuses()
    lo, hi = 1, 1024
    assert fuses(lo), "the single launch is not taken at obs_dim 1"
    if fuses(hi):
        pytest.fail("ppoaf_icm_update_fuses_kernels answers 1 up to obs_dim 1024: there is no edge to test")
    while hi - lo > 1:                                             # the LDS need grows with ceil(obs_dim / 16)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fuses(mid) else (lo, mid)
    print(f"single launch up to obs_dim {lo}")
    run_case(f"ow_fuse_edge_in{lo}", H.case("one_width", lo, 18, 128, action=("discrete", 3), act="leaky_relu", rows="tail", seed=1201), True)
    run_case(f"ow_fuse_edge_in{hi}", H.case("one_width", hi, 18, 128, action=("continuous", 2), rows="agents", seed=1202), False)


# ------------------------------------------------------------------------------------------------------------- fuzz
def _fuzz(chain):
    from hypothesis import HealthCheck, given, settings, strategies as st
    count = [0]

    @settings(max_examples=12, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(O=st.integers(1, 200), B=st.integers(1, 528), H1=st.sampled_from([64, 128]),
           w=st.tuples(*[st.sampled_from([32, 64, 128])] * 3), D=st.integers(1, 128), d_inv=st.integers(1, 3),
           d_fwd=st.integers(1, 3), kind=st.sampled_from(["discrete", "continuous", "multi"]), n=st.integers(1, 8),
           md=st.sampled_from(H._MULTI), act=st.sampled_from(H.ACTIVATIONS), beta=st.sampled_from([0.2, 0.8]),
           rows=st.sampled_from(H.ROW_MODES), seed=st.integers(0, 1000))
    def run(O, B, H1, w, D, d_inv, d_fwd, kind, n, md, act, beta, rows, seed):
        if chain == "one_width" and kind == "multi":
            kind = "discrete"
        action = ("multi", md) if kind == "multi" else (kind, max(n, 2) if kind == "discrete" else n)
        if rows == "agents":
            B += (-B) % 3
        if chain == "one_width":
            widths = H1
        elif chain == "identity":
            O, widths = min(O, 128), (w[1], w[2])
        else:
            widths = (w[0], D, w[1], w[2])
            if kind != "multi" and len({w[0], D, w[1], w[2]}) == 1 and D in (64, 128):
                widths = (w[0], D - 1, w[1], w[2])                  # (all four equal is the one-width chain's)
        count[0] += 1
        run_case(f"fuzz_{chain}_{count[0]}", H.case(chain, O, B, widths, (d_inv, d_fwd), action, act, beta, rows, 2000 + seed))

    run()


@pytest.mark.parametrize("chain", ["one_width", "shapes", "identity"])
def test_k14_minibatch_fuzz(chain):
    """Derandomised draws over the same space: obs_dim, widths, depths, B, actions, activation, icm_beta, row addressing."""
    _fuzz(chain)
