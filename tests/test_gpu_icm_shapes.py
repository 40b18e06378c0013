"""
-m gpu: K14's chain for ICMs whose encoder, encoding and models have widths of their own (csrc/icm_update_shapes.hip) --
the shapes every reference baseline with an ICM configures (E 128, D 9 or 2, M 32 or 128).  Against the fixtures recorded
from the unmodified reference (g10_icm), against the torch-CPU oracle over whole epochs, against this package's torch path
(rollout rewards, fuzzed shapes and activations), bitwise from run to run and beside the overlapped PPO chain, and on two
ranks.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ppo_loop

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# kind, NA, O, E (encoder width), D (encoding), Mi, Mf, envs, T, B
CASES = [
    dict(kind="d", NA=3, O=6, E=128, D=9, Mi=32, Mf=32, envs=12, T=16, B=40),        # baseline shape; 4 full mini-batches + a tail of 32
    dict(kind="c", NA=1, O=2, E=128, D=2, Mi=32, Mf=32, envs=8, T=8, B=16),          # mountain_car
    dict(kind="d", NA=5, O=18, E=64, D=17, Mi=64, Mf=32, envs=8, T=12, B=32, d_inv=3, d_fwd=1),   # D one past a column tile; Mi != Mf
    dict(kind="c", NA=6, O=17, E=128, D=16, Mi=128, Mf=128, envs=12, T=16, B=64),    # abmarl_maze form; D exactly one tile
    dict(kind="c", NA=2, O=3, E=32, D=128, Mi=32, Mf=32, envs=16, T=64, B=16, graphs=True),   # 64 mini-batches: two graph chunks; D > E
    # 33 row tiles: the wgrad tile's operand loop takes a third trip on the encoder jobs (66 chunks over both streams); tail of 32
    dict(kind="d", NA=3, O=6, E=64, D=9, Mi=32, Mf=32, envs=34, T=32, B=528),
]


def _space(c):
    from ppo_and_friends_amd.spaces import Box, Discrete
    return Discrete(c["NA"]) if c["kind"] == "d" else Box(-1.0, 1.0, (c["NA"],), np.float32)


def _icm_kw(c, **more):
    return dict(encoded_obs_dim=c["D"], encoder_hidden_size=c["E"], inverse_hidden_size=c["Mi"], forward_hidden_size=c["Mf"],
                inverse_hidden_depth=c.get("d_inv", 2), forward_hidden_depth=c.get("d_fwd", 2), **more)


def _make_ppo(c, mode="fused", seed=4, epochs=1, **icm_more):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    dev = torch.device("cuda", 0)
    space, O = _space(c), c["O"]
    env_gen = lambda: SyntheticFixedLengthEnv(c["envs"], O, space, c["T"], dev, reward="uniform", seed=5, term_prob=0.05)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    return PPO(env_gen, {"p": (None, sp, sp, space, dict(enable_icm=True, icm_kw_args=_icm_kw(c, **icm_more)))}, device=dev,
               random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=c["envs"], ts_per_rollout=c["T"],
               batch_size=c["B"], epochs_per_iter=epochs, update_mode=mode, use_graphs=c.get("graphs", False))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's own numbers through the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["cont", "disc"])
def test_reference_fixture_g10_through_the_kernels(golden, tag):
    """
    g10_icm (ICM.forward and every parameter gradient of the unmodified reference, icm.py:22-430) through ONE mini-batch of
    B = 40 rows (two full row tiles + one of 8 rows) of fwd_bwd + wgrad, fused_adam = 0, icm_beta = 0.8, identity perm, and
    through the reward entry point.  Tolerances: those of test_icm_module_matches_reference_golden_g10 (the torch path on
    the same fixture).
    """
    from ppo_and_friends_amd import _lib, kernels as K
    from ppo_and_friends_amd.fused_update import _describe_icm, icm_scratch_floats, icm_topology_args
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, Discrete
    g = golden("g10_icm")
    dev = torch.device("cuda", 0)
    if tag == "disc":
        icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (6,), np.float32), action_space=Discrete(3), encoded_obs_dim=32,
                  encoder_hidden_size=32, inverse_hidden_size=32, forward_hidden_size=32)
    else:
        icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (17,), np.float32), action_space=Box(-1.0, 1.0, (6,), np.float32),
                  encoded_obs_dim=32, encoder_hidden_size=64, inverse_hidden_size=32, forward_hidden_size=32,
                  inverse_hidden_depth=3, forward_hidden_depth=1)
    icm.to(dev)
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}_p_")}
    missing, unexpected = icm.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    topo, why = _describe_icm(icm, icm.action_dtype)
    assert why == "" and topo["general"], why
    obs1 = torch.from_numpy(g[f"{tag}_obs1"]).to(dev).reshape(40, -1).contiguous()
    obs2 = torch.from_numpy(g[f"{tag}_obs2"]).to(dev).reshape(40, -1).contiguous()
    act = torch.from_numpy(g[f"{tag}_actions"]).to(dev)
    act = (act.reshape(40).long() if tag == "disc" else act.reshape(40, -1).float()).contiguous()
    B, nT, total = 40, 3, topo["bucket_total"]
    lib = _lib.load()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
    n_act, n_denc = icm_scratch_floats(topo, B)
    keep = dict(act=z(n_act), denc=z(n_denc), m=z(total), v=z(total), step=z(1, torch.int64), lr=z(1), cursor=z(1, torch.int64),
                perm=torch.arange(B, dtype=torch.int64, device=dev), parts=z(2 * (nT + 1)), totals=z(2, torch.float64))
    a = icm_topology_args(topo)
    a.params, a.grads = icm.flat_params.data_ptr(), icm.flat_grads.data_ptr()
    a.exp_avg, a.exp_avg_sq, a.step_count, a.lr = (keep[k].data_ptr() for k in ("m", "v", "step", "lr"))
    a.beta1, a.beta2, a.adam_eps, a.grad_scale = 0.9, 0.999, 1e-5, 1.0
    a.obs, a.next_obs, a.actions = obs1.data_ptr(), obs2.data_ptr(), act.data_ptr()
    a.perm, a.row_map, a.n_rows, a.inputs_in_batch_order = keep["perm"].data_ptr(), None, B, 0
    a.cursor, a.B, a.batch_stride = keep["cursor"].data_ptr(), B, B
    a.icm_beta, a.fused_adam = 0.8, 0
    a.act_scratch, a.denc_scratch = keep["act"].data_ptr(), keep["denc"].data_ptr()
    a.loss_partials, a.totals = keep["parts"].data_ptr(), keep["totals"].data_ptr()
    need = C.c_int64(0)
    _lib.check(lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)), "workspace_bytes")
    ws = z(need.value, torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    icm.flat_grads.fill_(float("nan"))                      # every gradient element must be written
    before = icm.flat_params.clone()
    _lib.check(lib.ppoaf_icm_shapes_fwd_bwd(C.byref(a), K.stream()), "fwd_bwd")
    _lib.check(lib.ppoaf_icm_shapes_wgrad(C.byref(a), K.stream()), "wgrad")
    torch.cuda.synchronize()
    assert torch.equal(icm.flat_params, before) and int(keep["cursor"].item()) == 1 and float(keep["totals"][1]) == 1.0
    got_loss, want_loss = float(keep["totals"][0]), float(g[f"{tag}_losses"][2])
    print(f"{tag}: loss {got_loss!r} against {want_loss!r} (rel {abs(got_loss - want_loss) / abs(want_loss):.2e})")
    np.testing.assert_allclose(got_loss, want_loss, rtol=1e-5)
    params = dict(icm.named_parameters())
    worst = 0.0
    for k in (str(n) for n in g[f"{tag}_names"]):
        want = g[f"{tag}_g_{k}"]
        got = params[k].grad.detach().cpu().numpy()
        scale = max(np.abs(want).max(), 1e-6)
        worst = max(worst, float(np.abs(got - want).max() / scale))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * scale, err_msg=k)
    print(f"{tag}: worst gradient deviation {worst:.2e} of the parameter's largest gradient")
    # rollout-time reward: the encoder, then the forward model alone
    r = icm_topology_args(topo)
    r.params, r.act_scratch = a.params, a.act_scratch
    r.obs, r.next_obs, r.actions = a.obs, a.next_obs, a.actions
    r.B, r.batch_stride, r.n_rows, r.fused_adam = B, B, B, 0
    out = torch.full((B,), float("nan"), device=dev)
    _lib.check(lib.ppoaf_icm_shapes_intrinsic_reward(C.byref(r), float(icm.reward_scale) / 2.0, out.data_ptr(), K.stream()), "reward")
    np.testing.assert_allclose(out.cpu().numpy(), g[f"{tag}_intr"].reshape(-1), rtol=1e-5, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole epochs against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['kind']}-O{c['O']}-E{c['E']}-D{c['D']}-M{c['Mi']}.{c['Mf']}-B{c['B']}")
def test_fused_icm_update_of_general_shapes_matches_oracle(case):
    """K14's general chain against the torch-CPU ICM of oracle/icm_oracle.py trained on the same mini-batches: two epochs, the
    tolerances of test_fused_icm_update_matches_oracle."""
    from oracle import icm_oracle
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    dev = torch.device("cuda", 0)
    c = dict(d_inv=2, d_fwd=2); c.update(case)
    envs, T, O, NA, B, D = c["envs"], c["T"], c["O"], c["NA"], c["B"], c["D"]
    ppo = _make_ppo(case)
    pol = ppo.policies["p"]
    assert FusedIcmUpdate.unsupported_reason(pol) == ""
    ref = icm_oracle.ICM(O, NA, discrete=c["kind"] == "d", enc=D, hidden=c["Mi"], enc_hidden=c["E"], inv_depth=c["d_inv"],
                         fwd_depth=c["d_fwd"])
    if c["Mf"] != c["Mi"]:
        ref.forward_model.sequential_net = cpu_ppo_loop.make_mlp(D + NA, D, c["Mf"], c["d_fwd"], out_gain=1.0)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    opt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-5)
    ppo.rollout()
    buf = pol.buffer
    N = envs * T
    rm = buf.row_map.cpu().long()
    flat = lambda t: t.reshape((N,) + tuple(t.shape[2:])).cpu()[rm]
    obs, nxt, act = flat(buf.observations), flat(buf.next_observations), flat(buf.actions)
    fused = FusedIcmUpdate(ppo, "p")
    assert fused.topo["general"] and fused.fuse_reason() != ""
    g = torch.Generator().manual_seed(9)
    for epoch in range(2):
        perm = torch.randperm(N, generator=g)
        fused.begin_epoch(perm.to(dev))
        fused.run_epoch()
        assert fused._epoch_snapshot is None                 # no bounded waits in this chain: nothing to restart from
        t = fused.end_epoch()
        tot, cnt = 0.0, 0
        for o in range(0, N, B):
            idx = perm[o:o + B]
            _, inv_loss, f_loss = ref(obs[idx], nxt[idx], act[idx])
            loss = (1.0 - pol.icm_beta) * f_loss + pol.icm_beta * inv_loss
            opt.zero_grad(); loss.backward(); opt.step()
            tot += float(loss); cnt += 1
        assert t[1] == cnt
        np.testing.assert_allclose(t[0] / cnt, tot / cnt, rtol=2e-5, err_msg=f"icm loss, epoch {epoch}")
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=1e-4, atol=2e-5)
    assert int(pol.icm_optim.step_count.item()) == 2 * cnt


# ---------------------------------------------------------------------------------------------------------------------
# 3. rollout-time reward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=["baseline", "D17-Mi64-Mf32"])
def test_rollout_reward_takes_the_two_launch_path(case):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    dev = torch.device("cuda", 0)
    pol = _make_ppo(case).policies["p"]
    n, O, NA = 37, case["O"], case["NA"]                       # two row tiles + one of 5 rows
    gen = torch.Generator().manual_seed(3)
    o1, o2 = torch.randn(n, O, generator=gen).to(dev), torch.randn(n, O, generator=gen).to(dev)
    act = torch.randint(0, NA, (n, 1), generator=gen).to(dev) if case["kind"] == "d" else torch.rand(n, NA, generator=gen).to(dev) * 2 - 1
    calls = PPOPolicy.fused_icm_reward_calls
    pol.fused_icm_reward = True
    fused = pol.get_intrinsic_reward(o1, o2, act)
    assert PPOPolicy.fused_icm_reward_calls == calls + 1 and pol.fused_icm_reward, "the fused path was not the one taken"
    pol.fused_icm_reward = False
    plain = pol.get_intrinsic_reward(o1, o2, act)
    assert PPOPolicy.fused_icm_reward_calls == calls + 1
    assert fused.shape == plain.shape == (n,)
    np.testing.assert_allclose(fused.cpu().numpy(), plain.cpu().numpy(), rtol=3e-5, atol=3e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 4. fuzz against the torch path
# ---------------------------------------------------------------------------------------------------------------------
def test_general_icm_shapes_fuzz_against_the_torch_path():
    """Randomised shapes (hypothesis, derandomised) against this package's torch-ROCm path on the same rollout and shuffles:
    the body and tolerances of the `icm` half of test_fused_mat_and_icm_paths_fuzz_against_the_torch_paths; the three
    activations are drawn here."""
    import torch.nn as nn
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.ppo import PermutationLoader
    widths = st.sampled_from([32, 64, 128])

    @settings(max_examples=10, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(kind=st.sampled_from(["d", "c"]), NA=st.integers(2, 8), O=st.integers(1, 60), E=widths, D=st.integers(1, 128), Mi=widths,
           Mf=widths, d_inv=st.integers(1, 3), d_fwd=st.integers(1, 3), envs=st.integers(1, 10), T=st.integers(2, 20),
           B=st.integers(2, 70), act=st.sampled_from(["relu", "leaky", "tanh"]))
    def icm(kind, NA, O, E, D, Mi, Mf, d_inv, d_fwd, envs, T, B, act):
        if E == D == Mi == Mf and E != 32:
            return                                             # (the one-width chain's: fuzzed in test_gpu_end_to_end.py)
        c = dict(kind=kind, NA=NA, O=O, E=E, D=D, Mi=Mi, Mf=Mf, d_inv=d_inv, d_fwd=d_fwd, envs=envs, T=T, B=B)
        res = []
        for mode in ("fused", "torch"):
            activation = {"relu": nn.ReLU(), "leaky": nn.LeakyReLU(), "tanh": nn.Tanh()}[act]
            ppo = _make_ppo(c, mode, activation=activation)
            pol = ppo.policies["p"]
            upd = ppo._fused_icm_updater("p")
            assert (upd is not None) == (mode == "fused")
            assert upd is None or upd.topo["general"]
            ppo.rollout()
            loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
            ppo._icm_batch_train(loader, "p")
            res.append((pol.icm_model.flat_params.detach().cpu().numpy().copy(), pol.buffer.rewards.cpu().numpy().copy(),
                        ppo.status_dict["p"]["icm loss"]))
        (w0, r0, l0), (w1, r1, l1) = res
        np.testing.assert_allclose(r0, r1, rtol=3e-5, atol=3e-6)                 # rollout-time intrinsic rewards
        np.testing.assert_allclose(l0, l1, rtol=5e-5)
        np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)

    icm()


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism and overlap
# ---------------------------------------------------------------------------------------------------------------------
def test_one_epoch_is_bitwise_reproducible():
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    dev = torch.device("cuda", 0)
    c = CASES[0]
    ppo = _make_ppo(c)
    pol = ppo.policies["p"]
    ppo.rollout()
    fused = FusedIcmUpdate(ppo, "p")
    opt = pol.icm_optim
    state = [pol.icm_model.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_count]
    start = [t.clone() for t in state]
    perm = torch.randperm(c["envs"] * c["T"], generator=torch.Generator().manual_seed(1)).to(dev)
    runs = []
    for _ in range(2):
        for t, k in zip(state, start):
            t.copy_(k)
        fused.begin_epoch(perm)
        fused.run_epoch()
        totals = fused.end_epoch()
        runs.append([t.clone() for t in state] + [pol.icm_model.flat_grads.clone(), torch.as_tensor(totals)])
    assert not torch.equal(runs[0][0], start[0])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_overlapped_with_the_ppo_chain_is_bitwise_the_epochs_in_turn(monkeypatch):
    """train_on_rollout: the ICM chain on XCDs 4-7 beside the PPO chain on XCDs 0-3 (two streams) against PPOAF_OVERLAP_ICM=0."""
    res = []
    for overlap in ("1", "0"):
        monkeypatch.setenv("PPOAF_OVERLAP_ICM", overlap)
        ppo = _make_ppo(CASES[0], epochs=2)
        assert ppo._fused_updater("p", CASES[0]["B"]) is not None and ppo._fused_icm_updater("p").topo["general"]
        ppo.rollout()
        ppo.train_on_rollout()
        torch.cuda.synchronize()
        assert getattr(ppo._fused_icm_updater("p"), "xcd_half", 0) == (2 if overlap == "1" else 0)
        res.append((ppo.policies["p"].icm_model.flat_params.clone(), ppo.policies["p"].icm_optim.exp_avg.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_stay_identical_and_match_the_torch_path(tmp_path):
    """Two processes on the one GPU (tests/helpers/icm_shapes_rank.py, collectives over gloo as in tests/test_gpu_two_ranks.py), each under
    its own time limit: one ICM epoch of the baseline shape with update_mode "fused", then the same with "torch"."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PPOAF_GRAD_EXCHANGE="rccl")
    env.pop("PPOAF_BACKEND", None)
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "helpers", "icm_shapes_rank.py"), str(tmp_path)],
                              cwd=os.path.dirname(HERE), env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(outs)[-4000:]      # (nothing further is started after a failure)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(2))
    assert r0["general"] and r1["general"]
    assert not torch.equal(r0["obs"], r1["obs"]), "each rank rolls out its own envs"
    for k in ("w0", "w", "exp_avg", "exp_avg_sq"):
        assert torch.equal(r0[k], r1[k]), f"{k}: the ranks' ICM buckets differ"
    assert not torch.equal(r0["w"], r0["w0"])
    assert torch.equal(r0["w0"], r0["w0_torch"]) and torch.equal(r0["actions"], r0["actions_torch"]), "the two legs' starting points"
    np.testing.assert_allclose(r0["loss"], r0["loss_torch"], rtol=5e-5)
    np.testing.assert_allclose(r0["w"].numpy(), r0["w_torch"].numpy(), rtol=2e-4, atol=3e-5)
