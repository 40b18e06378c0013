"""
-m gpu: the agent-shared ICM of an agent-grouped (MAT) policy on K14's shapes chain, behind the opt-in
`PPOPolicy.fused_shared_icm` -- one ICM sample per grouped row over the group's concatenated observations, actions
MultiDiscrete([n] * agents) (ppo.py:2520-2538, "case 2"; icm.py:76-77, 198-211, 400-412).  E 8, T 12, seed 6; shapes

    a  A 3, Discrete(5): 15 classes, the default ICM (128s); B 16 and 5 (a partial row tile, an epoch tail of one row)
    b  A 2, Discrete(8): 16 classes, D 9 / M 32 behind an encoder of 128
    c  A 8, Discrete(2): 16 classes in eight slices, identity encoder over 8 x 8 = 64 columns, Mi 32 / Mf 64
    d  A 2, Discrete(2): 4 classes, identity encoder over 36 columns, M 32; B 5

The opt-in is set right after PPO(...) and before the first rollout.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

E, T, SEED = 8, 12, 6
# agents, classes per agent, per-agent observation width, icm_kw_args, the oracle's form (tests/helpers/icm_shared.py)
SHAPES = {
    "a": dict(A=3, NA=5, O=18, icm={}, ref={}),
    "b": dict(A=2, NA=8, O=18, icm=dict(encoded_obs_dim=9, encoder_hidden_size=128, inverse_hidden_size=32, forward_hidden_size=32),
              ref=dict(enc=9, hidden=32, enc_hidden=128)),
    "c": dict(A=8, NA=2, O=8, icm=dict(encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=64),
              ref=dict(identity=True, Mi=32, Mf=64)),
    "d": dict(A=2, NA=2, O=18, icm=dict(encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=32),
              ref=dict(identity=True, Mi=32, Mf=32)),
}
CASES = [("a", 16), ("a", 5), ("b", 16), ("c", 16), ("d", 5)]


def _make_ppo(shape, B, mode="fused", opt_in=True, use_graphs=False):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    env_gen = lambda: SyntheticFixedLengthEnv(E, c["O"], Discrete(c["NA"]), T, dev, reward="uniform", seed=41, num_agents=c["A"])
    sp = Box(-np.inf, np.inf, (c["O"],), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(c["NA"]),
                                dict(enable_icm=True, agent_shared_icm=True, icm_kw_args=dict(c["icm"])))},
              device=dev, random_seed=SEED, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
              batch_size=B, epochs_per_iter=1, update_mode=mode, use_graphs=use_graphs)
    if opt_in:
        ppo.policies["mat"].fused_shared_icm = True
    return ppo


def _check_updater(ppo, shape, B):
    c = SHAPES[shape]
    upd = ppo._fused_icm_updater("mat")
    assert upd is not None, "the shared ICM's epoch stayed on the torch path"
    assert upd.topo["general"] is True and upd.topo["n_action_slices"] == c["A"] and upd.A == 1 and upd.shared
    assert upd.topo["action_dim"] == upd.topo["fwd_action_dim"] == c["A"] * c["NA"] and upd.topo["obs_dim"] == c["A"] * c["O"]
    assert bool(upd.topo.get("identity")) == bool(c["ref"].get("identity"))
    if upd.tables is not None:
        args = upd._args_for(B)
        assert (args.B, args.batch_stride, args.n_rows, args.inputs_in_batch_order) == (B, B, E * T, 1)
        assert args.n_action_slices == c["A"] and not args.perm and not args.row_map
    assert ppo._overlapped_epochs("mat") is False
    return upd


# ---------------------------------------------------------------------------------------------------------------------
# 1. the path
# ---------------------------------------------------------------------------------------------------------------------
def test_the_opt_in_takes_the_fused_path_for_the_epoch_and_the_reward():
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    B = 16
    ppo = _make_ppo("a", B)
    pol = ppo.policies["mat"]
    _check_updater(ppo, "a", B)
    calls = PPOPolicy.fused_icm_reward_calls
    ppo.rollout()
    assert PPOPolicy.fused_icm_reward_calls == calls + T, "the rollout's intrinsic rewards did not come from K14"
    upd = _check_updater(ppo, "a", B)
    upd.begin_epoch(PermutationLoader(pol.dataset, B, ppo.loader_generator).epoch_permutation())
    _check_updater(ppo, "a", B)
    args = upd._args_for(B)
    assert (args.B, args.batch_stride, args.n_rows, args.inputs_in_batch_order) == (B, B, E * T, 1)
    assert tuple(upd.tables["obs"].shape) == (E * T, 3 * 18) and tuple(upd.tables["actions"].shape) == (E * T, 3)
    assert upd.tables["actions"].dtype == torch.int64
    # without the opt-in, in the same process: the torch path, as before
    plain = _make_ppo("a", B, opt_in=False)
    assert plain._fused_icm_updater("mat") is None
    calls = PPOPolicy.fused_icm_reward_calls
    plain.rollout()
    assert PPOPolicy.fused_icm_reward_calls == calls


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the torch path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", CASES, ids=[f"{s}-B{b}" for s, b in CASES])
def test_shared_icm_epoch_fused_against_the_torch_path(shape, B):
    """As test_grouped_icm_epoch_fused_against_the_torch_path (tests/test_gpu_icm_grouped.py): both modes on the same rollout
    (the torch rollout) and the same shuffles; its tolerances."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    res, start = [], None
    for mode in ("fused", "torch"):
        ppo = _make_ppo(shape, B, mode, opt_in=(mode == "fused"))
        pol = ppo.policies["mat"]
        if start is None:
            start = pol.policy_params.detach().clone(), pol.icm_model.flat_params.detach().clone()
        with torch.no_grad():
            pol.policy_params.copy_(start[0]); pol.icm_model.flat_params.copy_(start[1])
        if mode == "fused":
            _check_updater(ppo, shape, B)
        else:
            assert ppo._fused_icm_updater("mat") is None
        pol.fused_step_unsupported_reason = lambda: "torch rollout forced by the test"
        calls = PPOPolicy.fused_icm_reward_calls
        ppo.rollout()
        assert PPOPolicy.fused_icm_reward_calls == calls + (T if mode == "fused" else 0)
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._icm_batch_train(loader, "mat")
        if mode == "fused":
            upd = _check_updater(ppo, shape, B)
            assert (upd.n_full, upd.tail, upd.n_done) == (E * T // B, E * T % B, -(-E * T // B))
        res.append((pol.icm_model.flat_params.detach().cpu().numpy().copy(), pol.buffer.rewards.cpu().numpy().copy(),
                    ppo.status_dict["mat"]["icm loss"], pol.buffer.actions.cpu().numpy().copy()))
    (w0, r0, l0, a0), (w1, r1, l1, a1) = res
    np.testing.assert_array_equal(a0, a1)
    print(f"{shape} B={B}: icm loss {l0!r} against {l1!r}; worst reward deviation {np.abs(r0 - r1).max():.2e}; "
          f"worst weight deviation {np.abs(w0 - w1).max():.2e}")
    np.testing.assert_allclose(r0, r1, rtol=3e-5, atol=3e-6)                 # rollout-time intrinsic rewards
    np.testing.assert_allclose(l0, l1, rtol=5e-5)
    np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the oracle, over a reshuffle of the agents
# ---------------------------------------------------------------------------------------------------------------------
def test_shared_icm_two_iterations_match_the_cpu_port():
    """The structure and tolerances of test_mat_policy_with_icm_matches_cpu_port[fused-shared] (tests/test_gpu_end_to_end.py)
    with the ICM half on K14: the second iteration runs after the policy reshuffled its agents, so agent_idxs and the
    dataset's slot order both differ from the first."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from oracle import mat_oracle
    c, B = SHAPES["a"], 16
    A, O, NA = c["A"], c["O"], c["NA"]
    ppo = _make_ppo("a", B, use_graphs=True)
    pol = ppo.policies["mat"]
    cpu = mat_oracle.CpuMATPPO(O, NA, A, batch_size=B, seed=SEED, enable_icm=True, agent_shared_icm=True)
    cpu.ac.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor_critic.state_dict().items()}, strict=False)
    cpu.icm.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(SEED)
    tol = dict(rtol=3e-5, atol=3e-5)
    orders = []
    for it in range(2):
        calls = PPOPolicy.fused_icm_reward_calls
        ds = ppo.rollout()
        assert PPOPolicy.fused_icm_reward_calls == calls + T
        env, buf = ppo.env, pol.buffer
        order = pol.agent_slot_order()
        obs_t = env.obs_table.view(T + 1, A, E, O)[:, order].transpose(1, 2).cpu().numpy()       # [T+1,E,A,O]
        rew_t = env.reward_table.view(T, A, E)[:, order].transpose(1, 2).cpu().numpy()
        ism_before = cpu.intrinsic_score_avg
        k = np.argsort(order)[pol._dataset_slot_order]                 # quirk Q14: dataset slot j <- rollout slot k[j]
        ref = cpu.rollout(obs_t, rew_t, buf.actions[..., 0].cpu().numpy()[:, :, np.argsort(k)], slot_order=order,
                          dataset_slot_of=k)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rtg.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.adv.numpy(), **tol)
        np.testing.assert_array_equal(ds.next_observations.cpu().numpy(), ref.next_obs.numpy())
        np.testing.assert_allclose(ppo.status_dict["mat"]["intrinsic score avg"], cpu.intrinsic_score_avg, rtol=1e-4)
        assert it == 0 or ism_before != 0.0
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._ppo_batch_train(loader, "mat")
        r = cpu.train_epoch()
        for name in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["mat"][name], r[name], rtol=5e-5, atol=5e-6, err_msg=name)
        ppo._icm_batch_train(loader, "mat")
        _check_updater(ppo, "a", B)
        icm_loss = cpu.icm_train_epoch(agent_idxs=pol.agent_idxs)
        print(f"iteration {it}: agent_idxs {list(pol.agent_idxs)}, slot order {list(order)}; icm loss "
              f"{ppo.status_dict['mat']['icm loss']!r} against {icm_loss!r}")
        np.testing.assert_allclose(ppo.status_dict["mat"]["icm loss"], icm_loss, rtol=5e-5)
        orders.append((list(pol.agent_idxs), list(order)))
        pol.clear_dataset()
    assert orders[0] != orders[1], "the agents were not reshuffled between the iterations: the test shows nothing"
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in cpu.icm.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=3e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 6. the C ABI on random rows
# ---------------------------------------------------------------------------------------------------------------------
def _abi_case(shape, B, seed=11):
    """The project's ICM of `shape` on the device, its oracle twin with the same weights, random rows, and the args of one
    mini-batch (identity perm, fused_adam 0) with everything they point to."""
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.fused_update import describe_icm_chain, icm_scratch_floats, icm_topology_args
    from ppo_and_friends_amd.networks.icm import ICM
    from ppo_and_friends_amd.spaces import Box, MultiDiscrete
    from icm_shared import oracle_shared_icm
    c = SHAPES[shape]
    dev = torch.device("cuda", 0)
    nvec, Ow = [c["NA"]] * c["A"], c["A"] * c["O"]
    torch.manual_seed(seed)
    icm = ICM(name="icm", obs_space=Box(-np.inf, np.inf, (Ow,), np.float32), action_space=MultiDiscrete(nvec), **c["icm"])
    icm.to(dev)
    ref = oracle_shared_icm(Ow, nvec, c["ref"])
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in icm.state_dict().items()})
    topo, why = describe_icm_chain(icm, icm.action_dtype, multi_discrete=True)
    assert why == "" and topo["general"] and topo["n_action_slices"] == c["A"], why
    gen = torch.Generator().manual_seed(seed)
    obs1, obs2 = torch.randn(B, Ow, generator=gen), torch.randn(B, Ow, generator=gen)
    act = torch.randint(0, c["NA"], (B, c["A"]), generator=gen)
    nT, total = (B + 15) // 16, topo["bucket_total"]
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
    n_act, n_denc = icm_scratch_floats(topo, B)
    keep = dict(act=z(n_act), denc=z(n_denc), m=z(total), v=z(total), step=z(1, torch.int64), lr=z(1), cursor=z(1, torch.int64),
                perm=torch.arange(B, dtype=torch.int64, device=dev), parts=z(2 * (nT + 1)), totals=z(2, torch.float64),
                obs1=obs1.to(dev).contiguous(), obs2=obs2.to(dev).contiguous(), actions=act.to(dev).contiguous())
    a = icm_topology_args(topo)
    a.params, a.grads = icm.flat_params.data_ptr(), icm.flat_grads.data_ptr()
    a.exp_avg, a.exp_avg_sq, a.step_count, a.lr = (keep[k].data_ptr() for k in ("m", "v", "step", "lr"))
    a.beta1, a.beta2, a.adam_eps, a.grad_scale = 0.9, 0.999, 1e-5, 1.0
    a.obs, a.next_obs, a.actions = keep["obs1"].data_ptr(), keep["obs2"].data_ptr(), keep["actions"].data_ptr()
    a.perm, a.row_map, a.n_rows, a.inputs_in_batch_order = keep["perm"].data_ptr(), None, B, 0
    a.cursor, a.B, a.batch_stride = keep["cursor"].data_ptr(), B, B
    a.icm_beta, a.fused_adam = 0.2, 0
    a.act_scratch, a.denc_scratch = keep["act"].data_ptr(), keep["denc"].data_ptr()
    a.loss_partials, a.totals = keep["parts"].data_ptr(), keep["totals"].data_ptr()
    need = C.c_int64(0)
    _lib.check(_lib.load().ppoaf_icm_shapes_workspace_bytes(C.byref(a), C.byref(need)), "workspace_bytes")
    keep["ws"] = z(need.value, torch.uint8)
    a.workspace, a.workspace_bytes = keep["ws"].data_ptr(), keep["ws"].numel()
    return icm, ref, topo, a, keep, (obs1, obs2, act)


@pytest.mark.parametrize("shape", ["b", "c"])
def test_one_minibatch_gradient_against_float64(shape):
    """fwd_bwd + wgrad (fused_adam 0) on B = 21 random rows (a partial last tile) against autograd in float64 on
    oracle/icm_oracle.ICM(nvec=...).  Bound, per tensor: 4 x the deviation of the SAME oracle in float32 on the CPU from that
    float64 result -- the margin the project gives MFMA K-order sums against a differently ordered float32 reference
    (tests/test_gpu_reference_golden.py).  The loss in `totals` has the same bound, 4 x the float32 oracle's deviation.  Only
    in the degenerate case that the float32 oracle's loss equals the float64 one (a deviation of 0, a bound that nothing
    but the same number meets) is the bound 4 float32 ulps of the loss instead; the test prints which bound was in force."""
    import copy
    from ppo_and_friends_amd import _lib, kernels as K
    B, beta = 21, 0.2
    icm, ref, topo, a, keep, (obs1, obs2, act) = _abi_case(shape, B)
    lib = _lib.load()
    icm.flat_grads.fill_(float("nan"))                      # every gradient element must be written
    before = icm.flat_params.clone()
    _lib.check(lib.ppoaf_icm_shapes_fwd_bwd(C.byref(a), K.stream()), "fwd_bwd")
    _lib.check(lib.ppoaf_icm_shapes_wgrad(C.byref(a), K.stream()), "wgrad")
    torch.cuda.synchronize()
    assert torch.equal(icm.flat_params, before) and int(keep["cursor"].item()) == 1 and float(keep["totals"][1]) == 1.0

    def run(model, dt):
        model.zero_grad()
        _, inv, f = model(obs1.to(dt), obs2.to(dt), act)
        loss = (1.0 - beta) * f + beta * inv
        loss.backward()
        return float(loss.detach()), {k: p.grad.detach().double().numpy().copy() for k, p in model.named_parameters()}

    l64, g64 = run(copy.deepcopy(ref).double(), torch.float64)
    l32, g32 = run(ref, torch.float32)
    got_loss = float(keep["totals"][0])
    print(f"{shape}: loss kernel {got_loss!r} float32 oracle {l32!r} float64 {l64!r}: deviations {abs(got_loss - l64):.3e} against {abs(l32 - l64):.3e}")
    got = {k: p.grad.detach().cpu().double().numpy() for k, p in icm.named_parameters()}
    assert sorted(got) == sorted(g64)
    failures = []
    for k in g64:
        assert np.isfinite(got[k]).all(), k
        dev_k, dev_32 = np.abs(got[k] - g64[k]).max(), np.abs(g32[k] - g64[k]).max()
        print(f"{shape}: {k:44s} max |g| {np.abs(g64[k]).max():.3e}  kernel {dev_k:.3e}  float32 oracle {dev_32:.3e}  ratio {dev_k / max(dev_32, 1e-300):.2f}")
        if not dev_k <= 4.0 * dev_32:
            failures.append((k, dev_k, dev_32))
    assert not failures, failures
    loss_bound = 4.0 * abs(l32 - l64)
    if l32 == l64:                                          # degenerate: the float32 oracle hit the float64 value itself
        loss_bound = 4.0 * 2.0 ** -23 * abs(l64)
    print(f"{shape}: loss bound in force {loss_bound:.3e} ({'4 float32 ulps: the oracle deviates by 0' if l32 == l64 else '4 x the float32 oracle deviation'})")
    assert abs(got_loss - l64) <= loss_bound, (got_loss, l32, l64)


@pytest.mark.parametrize("shape", ["b", "c"])
def test_out_of_range_classes_are_clamped_not_followed(shape):
    """A reward call with one class set to n + 3 and one to -1 gives, bitwise, what the call with them clamped to n - 1 and
    0 gives: per slice the Discrete behaviour, nothing is read beyond the slice's columns of the weight row."""
    from ppo_and_friends_amd import _lib, kernels as K
    from ppo_and_friends_amd.fused_update import icm_topology_args
    B = 21
    c = SHAPES[shape]
    icm, ref, topo, a, keep, (obs1, obs2, act) = _abi_case(shape, B)
    lib = _lib.load()
    dev = keep["obs1"].device

    def reward(actions):
        actions = actions.to(dev).contiguous()
        r = icm_topology_args(topo)
        r.params, r.act_scratch = a.params, a.act_scratch
        r.obs, r.next_obs, r.actions = a.obs, a.next_obs, actions.data_ptr()
        r.B, r.batch_stride, r.n_rows, r.fused_adam = B, B, B, 0
        out = torch.full((B,), float("nan"), device=dev)
        _lib.check(lib.ppoaf_icm_shapes_intrinsic_reward(C.byref(r), 0.005, out.data_ptr(), K.stream()), "reward")
        torch.cuda.synchronize()
        return out.cpu()

    wild, tame = act.clone(), act.clone()
    wild[3, 0], tame[3, 0] = c["NA"] + 3, c["NA"] - 1
    wild[17, c["A"] - 1], tame[17, c["A"] - 1] = -1, 0
    got, want = reward(wild), reward(tame)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    plain = reward(act)
    changed = (plain != want).nonzero().reshape(-1).tolist()
    assert set(changed) <= {3, 17}
    with torch.no_grad():
        intr, _, _ = ref(obs1, obs2, tame)
    np.testing.assert_allclose(want.numpy(), intr.numpy(), rtol=3e-5, atol=3e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 5. replay
# ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bitwise_the_eager_launches(monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    B = 16
    monkeypatch.setattr(FusedIcmUpdate, "graph_chunk", 2)          # 6 mini-batches: a warm-up chunk, then two replays
    ppo = _make_ppo("a", B)
    pol = ppo.policies["mat"]
    ppo.rollout()
    upd = _check_updater(ppo, "a", B)
    opt = pol.icm_optim
    state = [pol.icm_model.flat_params, opt.exp_avg, opt.exp_avg_sq, opt.step_count]
    start = [t.clone() for t in state]
    perm = torch.randperm(E * T, generator=torch.Generator().manual_seed(1)).to(pol.device)
    runs = []
    for graphs in (True, False):
        for t, k in zip(state, start):
            t.copy_(k)
        ppo.use_graphs = graphs
        upd.begin_epoch(perm)
        upd.run_epoch()
        totals = upd.end_epoch()
        runs.append([t.clone() for t in state] + [torch.as_tensor(totals)])
        assert upd.n_done == 6
    assert len(upd._graphs) == 1, "no graph was captured: the comparison shows nothing"
    assert not torch.equal(runs[0][0], start[0])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
