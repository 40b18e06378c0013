"""
-m gpu: K14's identity-encoder form (ICM(encoded_obs_dim = 0): csrc/icm_update_shapes.hip with enc_hidden = 0) -- what
abmarl_blind_maze / abmarl_blind_large_maze configure (O 2, models of width 128) and robot_warehouse's default (models of
width 32).  Test for test what tests/test_gpu_icm_shapes.py asks of the chain behind an encoder: against the fixture
recorded from the unmodified reference (g17_icm_identity), against the torch-CPU oracle over whole epochs, against this
package's torch path (rollout rewards, fuzzed shapes and activations), bitwise from run to run, and on two ranks.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

# kind, NA, O, Mi, Mf, envs, T, B
CASES = [
    dict(kind="d", NA=5, O=2, Mi=128, Mf=128, envs=12, T=16, B=40),                 # the blind-maze form; 4 full mini-batches + a tail of 32
    dict(kind="c", NA=1, O=1, Mi=32, Mf=32, envs=8, T=8, B=16),                     # one column
    dict(kind="d", NA=3, O=17, Mi=64, Mf=32, envs=8, T=12, B=32, d_inv=3, d_fwd=1),  # one past a column tile; two model launches
    dict(kind="c", NA=6, O=16, Mi=128, Mf=128, envs=12, T=16, B=64),                # exactly one column tile
    dict(kind="c", NA=2, O=128, Mi=32, Mf=32, envs=16, T=64, B=16, graphs=True),    # 64 mini-batches: two graph chunks; the widest O
    dict(kind="d", NA=3, O=6, Mi=32, Mf=32, envs=34, T=32, B=528),                  # 33 row tiles; tail of 32
]


def _space(c):
    from ppo_and_friends_amd.spaces import Box, Discrete
    return Discrete(c["NA"]) if c["kind"] == "d" else Box(-1.0, 1.0, (c["NA"],), np.float32)


def _icm_kw(c, **more):
    return dict(encoded_obs_dim=0, inverse_hidden_size=c["Mi"], forward_hidden_size=c["Mf"], inverse_hidden_depth=c.get("d_inv", 2),
                forward_hidden_depth=c.get("d_fwd", 2), **more)


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
def test_reference_fixture_g17_through_the_kernels(golden, tag):
    """
    g17_icm_identity (ICM.forward and every parameter gradient of the unmodified reference built with encoded_obs_dim = 0)
    through ONE mini-batch of B = 40 rows (two full row tiles + one of 8 rows) of fwd_bwd + wgrad, fused_adam = 0,
    icm_beta = 0.8, identity perm, denc_scratch = NULL, and through the reward entry point.  Tolerances: those of
    test_reference_fixture_g10_through_the_kernels.
    """
    from ppo_and_friends_amd import _lib, kernels as K
    from ppo_and_friends_amd.fused_update import describe_icm_chain, icm_scratch_floats, icm_topology_args
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, Discrete
    g = golden("g17_icm_identity")
    dev = torch.device("cuda", 0)
    if tag == "disc":
        icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (2,), np.float32), action_space=Discrete(5), encoded_obs_dim=0,
                  inverse_hidden_size=32, forward_hidden_size=32)
    else:
        icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (17,), np.float32), action_space=Box(-1.0, 1.0, (6,), np.float32),
                  encoded_obs_dim=0, inverse_hidden_size=64, forward_hidden_size=32, inverse_hidden_depth=3, forward_hidden_depth=1)
    icm.to(dev)
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}_p_")}
    missing, unexpected = icm.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    topo, why = describe_icm_chain(icm, icm.action_dtype)
    assert why == "" and topo["general"] and topo["identity"], why
    obs1 = torch.from_numpy(g[f"{tag}_obs1"]).to(dev).reshape(40, -1).contiguous()
    obs2 = torch.from_numpy(g[f"{tag}_obs2"]).to(dev).reshape(40, -1).contiguous()
    act = torch.from_numpy(g[f"{tag}_actions"]).to(dev)
    act = (act.reshape(40).long() if tag == "disc" else act.reshape(40, -1).float()).contiguous()
    B, nT, total = 40, 3, topo["bucket_total"]
    lib = _lib.load()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
    n_act, _ = icm_scratch_floats(topo, B)
    assert n_act == 2 * 48 * (16 if tag == "disc" else 32)
    keep = dict(act=z(n_act), m=z(total), v=z(total), step=z(1, torch.int64), lr=z(1), cursor=z(1, torch.int64),
                perm=torch.arange(B, dtype=torch.int64, device=dev), parts=z(2 * (nT + 1)), totals=z(2, torch.float64))
    a = icm_topology_args(topo)
    a.params, a.grads = icm.flat_params.data_ptr(), icm.flat_grads.data_ptr()
    a.exp_avg, a.exp_avg_sq, a.step_count, a.lr = (keep[k].data_ptr() for k in ("m", "v", "step", "lr"))
    a.beta1, a.beta2, a.adam_eps, a.grad_scale = 0.9, 0.999, 1e-5, 1.0
    a.obs, a.next_obs, a.actions = obs1.data_ptr(), obs2.data_ptr(), act.data_ptr()
    a.perm, a.row_map, a.n_rows, a.inputs_in_batch_order = keep["perm"].data_ptr(), None, B, 0
    a.cursor, a.B, a.batch_stride = keep["cursor"].data_ptr(), B, B
    a.icm_beta, a.fused_adam = 0.8, 0
    a.act_scratch, a.denc_scratch = keep["act"].data_ptr(), None          # no d(enc): observations take no gradient
    a.loss_partials, a.totals = keep["parts"].data_ptr(), keep["totals"].data_ptr()
    need = C.c_int64(0)
    _lib.check(lib.ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)), "workspace_bytes")
    ws = z(need.value, torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    icm.flat_grads.fill_(float("nan"))                      # every gradient element must be written
    before = icm.flat_params.clone()
    _lib.check(lib.ppoaf_icm_shapes_fwd_bwd(C.byref(a), K.stream()), "fwd_bwd (denc_scratch = NULL)")
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
    # rollout-time reward: the forward model alone on the observation rows, one launch
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
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['kind']}-O{c['O']}-M{c['Mi']}.{c['Mf']}-B{c['B']}")
def test_fused_icm_update_of_identity_encoders_matches_oracle(case):
    """K14's identity chain against the torch-CPU ICM of oracle/icm_oracle.py with its encoder replaced by nn.Identity()
    (tests/helpers/icm_identity.py) trained on the same mini-batches: two epochs, the tolerances of
    test_fused_icm_update_of_general_shapes_matches_oracle."""
    from icm_identity import oracle_icm
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    dev = torch.device("cuda", 0)
    c = dict(d_inv=2, d_fwd=2); c.update(case)
    envs, T, O, NA, B = c["envs"], c["T"], c["O"], c["NA"], c["B"]
    ppo = _make_ppo(case)
    pol = ppo.policies["p"]
    assert FusedIcmUpdate.unsupported_reason(pol) == ""
    ref = oracle_icm(O, NA, c["kind"] == "d", c["Mi"], c["Mf"], c["d_inv"], c["d_fwd"])
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    opt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-5)
    ppo.rollout()
    buf = pol.buffer
    N = envs * T
    rm = buf.row_map.cpu().long()
    flat = lambda t: t.reshape((N,) + tuple(t.shape[2:])).cpu()[rm]
    obs, nxt, act = flat(buf.observations), flat(buf.next_observations), flat(buf.actions)
    fused = FusedIcmUpdate(ppo, "p")
    assert fused.topo["general"] and fused.topo["identity"] and fused.fuse_reason() != ""
    assert fused._c_loop(None, 1) is False
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
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=["blind-maze", "O17-Mi64-Mf32"])
def test_rollout_reward_takes_the_one_launch_path(case):
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
    assert pol._icm_reward_state["entry"] == "ppoaf_icm_shapes_intrinsic_reward" and pol._icm_reward_state["args"].enc_hidden == 0
    pol.fused_icm_reward = False
    plain = pol.get_intrinsic_reward(o1, o2, act)
    assert PPOPolicy.fused_icm_reward_calls == calls + 1
    assert fused.shape == plain.shape == (n,)
    np.testing.assert_allclose(fused.cpu().numpy(), plain.cpu().numpy(), rtol=3e-5, atol=3e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 4. fuzz against the torch path
# ---------------------------------------------------------------------------------------------------------------------
def test_identity_icm_shapes_fuzz_against_the_torch_path():
    """Randomised shapes (hypothesis, derandomised) against this package's torch-ROCm path on the same rollout and shuffles:
    the body and tolerances of test_general_icm_shapes_fuzz_against_the_torch_path; O over the whole covered range."""
    import torch.nn as nn
    from hypothesis import given, settings, strategies as st, HealthCheck
    from ppo_and_friends_amd.ppo import PermutationLoader
    widths = st.sampled_from([32, 64, 128])

    @settings(max_examples=10, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(kind=st.sampled_from(["d", "c"]), NA=st.integers(2, 8), O=st.integers(1, 128), Mi=widths, Mf=widths, d_inv=st.integers(1, 3),
           d_fwd=st.integers(1, 3), envs=st.integers(1, 10), T=st.integers(2, 20), B=st.integers(2, 70),
           act=st.sampled_from(["relu", "leaky", "tanh"]))
    def icm(kind, NA, O, Mi, Mf, d_inv, d_fwd, envs, T, B, act):
        c = dict(kind=kind, NA=NA, O=O, Mi=Mi, Mf=Mf, d_inv=d_inv, d_fwd=d_fwd, envs=envs, T=T, B=B)
        res = []
        for mode in ("fused", "torch"):
            activation = {"relu": nn.ReLU(), "leaky": nn.LeakyReLU(), "tanh": nn.Tanh()}[act]
            ppo = _make_ppo(c, mode, activation=activation)
            pol = ppo.policies["p"]
            upd = ppo._fused_icm_updater("p")
            assert (upd is not None) == (mode == "fused")
            assert upd is None or upd.topo["identity"]
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
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_one_epoch_is_bitwise_reproducible():
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    dev = torch.device("cuda", 0)
    c = CASES[0]
    ppo = _make_ppo(c)
    pol = ppo.policies["p"]
    ppo.rollout()
    fused = FusedIcmUpdate(ppo, "p")
    assert fused.topo["identity"]
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


# ---------------------------------------------------------------------------------------------------------------------
# 6. two ranks
# ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_stay_identical_and_match_the_torch_path(tmp_path):
    """Two processes on the one GPU (tests/helpers/icm_identity_rank.py, collectives over gloo as in tests/test_gpu_two_ranks.py),
    each under its own time limit: one ICM epoch of the blind-maze form with update_mode "fused", then the same with "torch"."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PPOAF_GRAD_EXCHANGE="rccl")
    env.pop("PPOAF_BACKEND", None)
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "helpers", "icm_identity_rank.py"), str(tmp_path)],
                              cwd=os.path.dirname(HERE), env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(outs)[-4000:]      # (nothing further is started after a failure)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(2))
    assert r0["identity"] and r1["identity"]
    assert not torch.equal(r0["obs"], r1["obs"]), "each rank rolls out its own envs"
    for k in ("w0", "w", "exp_avg", "exp_avg_sq"):
        assert torch.equal(r0[k], r1[k]), f"{k}: the ranks' ICM buckets differ"
    assert not torch.equal(r0["w"], r0["w0"])
    assert torch.equal(r0["w0"], r0["w0_torch"]) and torch.equal(r0["actions"], r0["actions_torch"]), "the two legs' starting points"
    np.testing.assert_allclose(r0["loss"], r0["loss_torch"], rtol=5e-5)
    np.testing.assert_allclose(r0["w"].numpy(), r0["w_torch"].numpy(), rtol=2e-4, atol=3e-5)
