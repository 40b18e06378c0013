"""
-m gpu: ONE K14 mini-batch of the wide-action form (csrc/icm_update_shapes.hip: icm_sh_models_kernel<., 32>,
icm_sh_reward_kernel<., 32>, the [Bpad][32] action panels of the weight-gradient launch; Discrete / Box ICM actions of
9 .. 24 classes or dimensions, PPOAF_ICM_WIDE_ACTIONS) against float64 autograd of the oracle, through the C ABI, on the
shapes chain and the identity form.  Cases: tests/helpers/icm_wide_actions_cases.py (checked without a GPU, with planted
errors, by tests/test_icm_wide_actions_oracle.py).  Row addressing, NaN-filled tables, launches and the checks are
tests/test_gpu_icm_float64.py's (run_case over a Device described with the opt-in): per case and xcd_half 0 / 2
  1. fused_adam 0: the gradient bucket (prefilled with NaN, padding zero), the loss, cursor + 1, parameters unchanged;
  2. fused_adam 1 from H.preset_state: the parameter step, both moments, step + 1, the padding untouched;
and once per case the rollout-time reward of the same rows, written into a frame of sentinels that must stay untouched.
Bound per tensor (oracle/k12_oracle.deviations): |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| where
the float32 oracle on the CPU cannot do better; no row is left out (the helper redraws kinked rows).

Worst deviation / bound, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import icm_float64 as H  # noqa: E402
import icm_wide_actions_cases as W  # noqa: E402
import test_gpu_icm_float64 as T  # noqa: E402

pytestmark = pytest.mark.gpu

PlainDevice = T.Device         # (the tests below run T.run_case over WideDevice)
WORST = {}

MEASURED = """
worst deviation / bound per chain and form (one run of this file on the MI355X; xcd_half 0 and 2 measured the same)
  shapes       split        0.303  sh_disc17 step: inv_model.sequential_net.3.bias
  shapes       reward       0.034  sh_mario reward
  identity     split        0.270  id_disc24 step: forward_model.sequential_net.0.bias
  identity     reward       0.012  id_disc24 reward
"""


PAD = 64                       # sentinel floats in front of and behind the reward's B outputs
SENTINEL = -12345.678


class WideDevice(T.Device):
    """T.Device for a case described under `wide_actions` (the opt-in PPOPolicy.fused_wide_icm_actions).  It builds its own
    topology, tables and arguments the way the parent's constructor does -- that one describes without the opt-in and asserts
    a slice word of 0 -- and inherits the launches; the reward is taken inside a frame of sentinels."""

    def __init__(self, b):
        from ppo_and_friends_amd import _lib
        from ppo_and_friends_amd.fused_update import describe_icm_chain, icm_scratch_floats, icm_topology_args
        self.b, c = b, b.c
        self.lib = _lib.load()
        dev = self.dev = torch.device("cuda", 0)
        icm = self.icm = T._package_icm(c, dev)
        icm.load_state_dict({k: v.detach().clone() for k, v in b.model.state_dict().items()})
        assert c["action"][0] in ("discrete", "continuous") and H.action_dims(c)[0] > 8
        assert describe_icm_chain(icm, icm.action_dtype)[0] is None                 # refused without the opt-in
        topo, why = describe_icm_chain(icm, icm.action_dtype, wide_actions=True)
        assert why == "" and topo is not None, why
        assert topo.get("general") and ("identity" if topo.get("identity") else "shapes") == c["chain"]
        assert topo["n_action_slices"] == _lib.ICM_WIDE_ACTIONS
        self.topo, self.general = topo, True
        # the bucket is laid out as the reference lays its gradients
        base = icm.flat_params.data_ptr()
        assert topo["bucket_total"] == b.size == icm.flat_params.numel()
        for (_, name, off, shape), (pname, p) in zip(b.table, icm.named_parameters()):
            assert name == pname and (p.data_ptr() - base) // 4 == off and tuple(p.shape) == shape, name
        assert np.array_equal(icm.flat_params.detach().cpu().double().numpy()[~b.pad], b.params[~b.pad])
        self.p0 = icm.flat_params.detach().clone()
        # ---- tables: NaN wherever the mini-batch has no row
        pl = self.pl = T._placement(c)
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
            act=z(n_act), denc=z(n_denc), m=z(total), v=z(total), step=z(1, torch.int64), lr=torch.full((1,), T.LR, device=dev),
            cursor=z(1, torch.int64), parts=z(2 * (nT + 1)), totals=z(2, torch.float64),
            obs1=obs1.to(dev).contiguous(), obs2=obs2.to(dev).contiguous(), actions=table_act.to(dev).contiguous(),
            perm=None if pl["perm"] is None else torch.as_tensor(pl["perm"]).to(dev),
            row_map=None if pl["row_map"] is None else torch.as_tensor(pl["row_map"]).to(dev),
            r_obs1=torch.as_tensor(b.obs1).to(dev).contiguous(), r_obs2=torch.as_tensor(b.obs2).to(dev).contiguous(),
            r_actions=act.to(dev).contiguous())
        a = self.args = icm_topology_args(topo)
        assert a.n_action_slices == _lib.ICM_WIDE_ACTIONS
        a.params, a.grads = icm.flat_params.data_ptr(), icm.flat_grads.data_ptr()
        a.exp_avg, a.exp_avg_sq, a.step_count, a.lr = (k[x].data_ptr() for x in ("m", "v", "step", "lr"))
        a.beta1, a.beta2, a.adam_eps, a.grad_scale = T.BETAS[0], T.BETAS[1], T.EPS, 1.0
        a.obs, a.next_obs, a.actions = k["obs1"].data_ptr(), k["obs2"].data_ptr(), k["actions"].data_ptr()
        a.perm = None if k["perm"] is None else k["perm"].data_ptr()
        a.row_map = None if k["row_map"] is None else k["row_map"].data_ptr()
        a.n_rows, a.inputs_in_batch_order = pl["n_rows"], pl["in_order"]
        a.cursor, a.B, a.batch_stride = k["cursor"].data_ptr(), B, pl["stride"]
        a.icm_beta, a.fused_adam = b.beta, 0
        a.act_scratch, a.denc_scratch = k["act"].data_ptr(), k["denc"].data_ptr()
        a.loss_partials, a.totals = k["parts"].data_ptr(), k["totals"].data_ptr()
        need = C.c_int64(0)
        _lib.check(self.lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)), "icm_shapes_workspace_bytes")
        k["ws"] = z(int(need.value), torch.uint8)
        a.workspace, a.workspace_bytes = k["ws"].data_ptr(), k["ws"].numel()

    def reward(self):
        """The rollout-time reward of the case's B rows, written into the middle of [PAD + B + PAD] floats: the sentinels in
        front and behind must stay bit for bit (a ragged last tile must not write past row B)."""
        from ppo_and_friends_amd import _lib, kernels as K
        from ppo_and_friends_amd.fused_update import icm_topology_args
        B, k = self.b.c["B"], self.keep
        r = icm_topology_args(self.topo)
        r.params, r.act_scratch = self.icm.flat_params.data_ptr(), k["act"].data_ptr()
        r.obs, r.next_obs, r.actions = k["r_obs1"].data_ptr(), k["r_obs2"].data_ptr(), k["r_actions"].data_ptr()
        r.B, r.batch_stride, r.n_rows, r.fused_adam = B, B, B, 0
        frame = torch.full((PAD + B + PAD,), SENTINEL, device=self.dev)
        frame[PAD:PAD + B] = float("nan")                          # every reward must be written
        before = frame.clone()
        with torch.no_grad():
            self.icm.flat_params.copy_(self.p0)
        _lib.check(self.lib.ppoaf_icm_shapes_intrinsic_reward(C.byref(r), H.REWARD_SCALE / 2.0, frame[PAD:].data_ptr(), K.stream()),
                   "icm_shapes_intrinsic_reward")
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32)
        assert torch.equal(bits(frame[:PAD]), bits(before[:PAD])), "the reward kernel wrote in front of its rows"
        assert torch.equal(bits(frame[PAD + B:]), bits(before[PAD + B:])), f"the reward kernel wrote past its {B} rows"
        return frame[PAD:PAD + B].double().cpu().numpy()


@pytest.fixture(autouse=True)
def _wide_harness(monkeypatch):
    monkeypatch.setattr(T, "Device", WideDevice)
    monkeypatch.setattr(T, "WORST", WORST)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{c:12s} {f:28s} {v[0]:.3f}  {v[1]}" for (c, f), v in sorted(WORST.items())]
    print("\nwide ICM actions: worst deviation / bound per chain and form:\n" + "\n".join(lines))


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_wide_action_minibatch_against_float64(name):
    T.run_case(name, W.CASES[name])


def test_a_narrow_launch_with_the_bit_is_bitwise_the_launch_without_it():
    """A <= 8 with PPOAF_ICM_WIDE_ACTIONS set runs the kernels it runs without it: gradients, step and reward bit for bit,
    and the same workspace."""
    from ppo_and_friends_amd import _lib
    for name in ("sh_D17", "id_in17"):
        b = H.Built(H.CASES[name])
        assert H.action_dims(b.c)[0] <= 8 and b.c["action"][0] != "multi"
        m0, v0 = H.preset_state(b.c, b.r64["grads"], b.pad)
        outs = []
        for bit in (0, _lib.ICM_WIDE_ACTIONS):
            d = PlainDevice(b)
            d.args.n_action_slices = bit
            d.topo = dict(d.topo, n_action_slices=bit)           # (reward() builds its arguments from the topology)
            need = C.c_int64(0)
            _lib.check(d.lib.ppoaf_icm_shapes_workspace_bytes(C.byref(d.args), C.byref(need)), "icm_shapes_workspace_bytes")
            assert int(need.value) == d.keep["ws"].numel()
            outs.append(d.launch(0) + d.launch(1, m0, v0) + [d.reward()])
        assert np.isfinite(outs[0][0][~b.pad]).all() and not np.array_equal(outs[0][1], outs[0][5])      # a gradient; a step was taken
        for x, y in zip(*outs):
            assert np.array_equal(x, y, equal_nan=True)          # (the gradient bucket's padding keeps its NaN prefill)
