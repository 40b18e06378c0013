"""
-m gpu: MATPolicy with per-agent observations 33..128 wide on the fused kernels -- K16 (rollout step), K15 (mini-batch
update) and, up to 64, K20 (evaluation step).  Wider than 32 the observation rows are not staged in LDS: the observation
LayerNorm and the encoder's first linear stream them through two 32-column chunk tiles, and K15's backward rebuilds the
chunks from global memory (csrc/mat_update.hip: mat_obs_encoder_wide).  Shapes are written (agents, obs, actions).

  1. rollout and two epochs against oracle.mat_oracle.CpuMATPPO, built as and held to the bounds of
     test_gpu_end_to_end.py::test_mat_policy_rollout_and_update_match_cpu_port;
  2. the first mini-batch's gradient bucket against the oracle's raw gradients;
  3. the forms at (3, 71, 5): fused tail / three launches, slab form, graphs on / off;
  4. K20 at 33..64 (helpers of test_gpu_mat_infer.py restated), the module decode above 64;
  5. MAT + identity-encoder ICM at (3, 71, 5): K16, K15 and K14 in one iteration, against the torch paths;
  6. the multi-rank rehearsal at (3, 71, 5).
"""
import copy
import ctypes as C
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E, T, SEED = 8, 12, 6


def _ppo(shape, B, mode="fused", epochs=2, icm=None, **kw):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    A, O, NA = shape
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, DEV, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    pk = {} if icm is None else dict(enable_icm=True, agent_shared_icm=False, icm_kw_args=dict(icm))
    return PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), pk)}, device=DEV, random_seed=SEED, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=epochs,
               update_mode=mode, **kw)


def _count_rollout_steps(pol):
    """-> list that receives one entry per K16 launch of the policy's rollout."""
    calls, inner = [], pol.rollout_step
    pol.rollout_step = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    return calls


def _oracle_for(pol, shape, B):
    """The CPU port with the policy's (initial) weights and the run's shuffle seed."""
    from oracle import mat_oracle
    A, O, NA = shape
    cpu = mat_oracle.CpuMATPPO(O, NA, A, batch_size=B, seed=SEED)
    cpu.ac.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor_critic.state_dict().items()}, strict=False)
    cpu.loader_generator = torch.Generator().manual_seed(SEED)
    return cpu


def _replay_on_oracle(cpu, ppo, pol, shape):
    """The recorded rollout on the CPU port (quirk Q14 included) -> its dataset."""
    A, O, NA = shape
    env, buf = ppo.env, pol.buffer
    order = pol.agent_slot_order()
    obs_t = env.obs_table.view(T + 1, A, E, O)[:, order].transpose(1, 2).cpu().numpy()       # [T+1,E,A,O]
    rew_t = env.reward_table.view(T, A, E)[:, order].transpose(1, 2).cpu().numpy()
    k = np.argsort(order)[pol._dataset_slot_order]                     # quirk Q14: dataset slot j <- rollout slot k[j]
    return cpu.rollout(obs_t, rew_t, buf.actions[..., 0].cpu().numpy()[:, :, np.argsort(k)], dataset_slot_of=k)


# ------------------------------------------------------------------------------- 1. rollout and two epochs, CPU port
#   (3, 33, 5) first wide width, a chunk of one column; (5, 100, 4) 3 sequences per tile and one dead row;
#   (16, 128, 8) every limit at once; B = 20: a tail mini-batch and a partly filled tile
ORACLE_CASES = [((3, 33, 5), 32), ((3, 71, 5), 32), ((3, 71, 5), 20), ((3, 128, 5), 32), ((5, 100, 4), 32), ((16, 128, 8), 32)]


@pytest.mark.parametrize("shape,B", ORACLE_CASES, ids=[f"{s[0]}-{s[1]}-{s[2]}-B{b}" for s, b in ORACLE_CASES])
def test_wide_mat_rollout_and_update_match_cpu_port(shape, B):
    from ppo_and_friends_amd.ppo import PermutationLoader
    A, O, NA = shape
    ppo = _ppo(shape, B)
    pol = ppo.policies["mat"]
    assert ppo._fused_updater("mat", B) is not None
    assert pol.agent_grouping and pol.fused_step_unsupported_reason() == ""
    steps = _count_rollout_steps(pol)
    cpu = _oracle_for(pol, shape, B)
    ds = ppo.rollout()
    assert len(steps) == T, "K16 did not step the rollout"
    assert len(ds) == E * T and ds.observations.shape == (E * T, A, O)
    ref = _replay_on_oracle(cpu, ppo, pol, shape)
    tol = dict(rtol=2e-5, atol=2e-5)
    np.testing.assert_array_equal(ds.observations.cpu().numpy(), ref.obs.numpy())
    got = dict(log_probs=ds.log_probs.cpu().numpy(), values=ds.values[torch.arange(E * T)].cpu().numpy(),
               rewards_to_go=ds.rewards_to_go.cpu().numpy(), advantages=ds.advantages.cpu().numpy())
    want = dict(log_probs=ref.logp.numpy(), values=ref.values.numpy(), rewards_to_go=ref.rtg.numpy(), advantages=ref.adv.numpy())
    for k in got:
        print(f"{shape} B={B} rollout {k}: max |d| {np.abs(got[k] - want[k]).max():.3e} (max |x| {np.abs(want[k]).max():.3e})")
    for k in got:
        np.testing.assert_allclose(got[k], want[k], err_msg=k, **tol)
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    pol.train()
    for ep in range(2):
        ppo._ppo_batch_train(loader, "mat")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            print(f"{shape} B={B} epoch {ep} {k}: {ppo.status_dict['mat'][k]!r} against {r[k]!r}")
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            np.testing.assert_allclose(ppo.status_dict["mat"][k], r[k], rtol=5e-5, atol=5e-6, err_msg=k)
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.actor_critic.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in cpu.ac.parameters()]).numpy()
    print(f"{shape} B={B} final weights: max |d| {np.abs(w - w_ref).max():.3e}")
    np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=3e-5)


# ------------------------------------------------------------------------------- 2. first mini-batch gradient
@pytest.mark.parametrize("shape", [(3, 71, 5), (3, 128, 5)], ids=["3-71-5", "3-128-5"])
def test_first_minibatch_gradient_matches_the_oracle(shape):
    """
    One ppoaf_mat_update_fwd_bwd + ppoaf_mat_update_reduce, no optimiser step, against the raw gradients of
    CpuMATPPO.train_epoch(perm)'s trace: rtol 1e-5, atol 1e-5 max|g|.  The trace holds d actor_loss / d actor and
    d critic_loss / d critic; the bucket holds d (actor_loss + critic_loss) / d (actor, critic) -- the decoder's queries
    read the encoder's output, so the critic's tensors, the observation encoder's among them, also receive the actor
    loss.  The actor's tensors are compared with the trace as it is.  For the critic's, the same mini-batch is taken
    through the oracle's own evaluate and loss once more on a copy: its critic-loss share must be the trace's, and its
    total is the reference.  The atol here is on the BUCKET's scale, and at the default initialisation half of the tensors
    lie orders of magnitude below it: tests/test_gpu_mat_update_float64.py judges every tensor of one K15 mini-batch on its
    own scale, against float64, with the weights overwritten.
    """
    from torch.utils.data import DataLoader
    from oracle import ppo_loss_oracle as lo
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    A, O, NA = shape
    B = 32
    ppo = _ppo(shape, B)
    pol = ppo.policies["mat"]
    cpu = _oracle_for(pol, shape, B)
    ppo.rollout()
    _replay_on_oracle(cpu, ppo, pol, shape)
    pol.train()
    perm = torch.randperm(E * T, generator=torch.Generator().manual_seed(3))
    fused = ppo._fused_updater("mat", B)
    assert fused is not None
    fused.begin_epoch(perm.to(DEV))
    args, lib, st = fused._args_for(B), _lib.load(), K.stream()
    _lib.check(lib.ppoaf_mat_update_fwd_bwd(C.byref(args), st), "mat fwd_bwd")
    _lib.check(lib.ppoaf_mat_update_reduce(C.byref(args), st), "mat reduce")
    torch.cuda.synchronize()
    base = pol.actor_critic.flat_params.data_ptr()
    piece = lambda p: pol.actor_critic.flat_grads[(p.data_ptr() - base) // 4:(p.data_ptr() - base) // 4 + p.numel()].cpu().numpy()

    twin = copy.deepcopy(cpu)
    cpu.trace = []
    cpu.train_epoch(perm.tolist())
    tr = cpu.trace[0]
    obs, actions, adv, logp_old, rtg, _ = next(iter(DataLoader(twin.dataset, batch_size=B, sampler=[int(i) for i in perm])))
    twin.value_stats.update(rtg.flatten().numpy())
    mean = torch.tensor(twin.value_stats.mean, dtype=torch.float32)
    var = torch.tensor(twin.value_stats.variance, dtype=torch.float32)
    rtg = ((rtg.flatten() - mean) / torch.sqrt(var + torch.tensor([1e-8]))).reshape(rtg.shape)
    values, cur_lp, entropy = twin.evaluate(obs, actions)
    r = lo.ppo_minibatch_losses(cur_lp, logp_old, adv, entropy, values, rtg, True, twin.surr_clip, twin.entropy_weight, use_huber=True)
    cparams = list(twin.ac.critic.parameters())
    share = torch.cat([x.reshape(-1) for x in torch.autograd.grad(r["critic_loss"], cparams, retain_graph=True)]).numpy()
    np.testing.assert_allclose(share, tr["critic_grad"], rtol=1e-6, atol=1e-7 * np.abs(tr["critic_grad"]).max(),
                               err_msg="the recomputed mini-batch is not the trace's")
    total_c = torch.autograd.grad(r["actor_loss"] + r["critic_loss"], cparams)

    want = np.concatenate([tr["actor_grad"]] + [x.reshape(-1).numpy() for x in total_c])
    got = np.concatenate([piece(p) for net in (pol.actor, pol.critic) for p in net.parameters()])
    scale = np.abs(want).max()
    report, own = [], []
    for (name, p), w in zip(pol.critic.named_parameters(), total_c):
        if name.startswith("obs_encoder."):                      # the only gradients the chunked backward writes
            d = np.abs(piece(p) - w.reshape(-1).numpy()).max()
            report.append(f"{name}: max |d| {d:.3e}, max |g| {float(w.abs().max()):.3e}")
            own.append((name, piece(p), w.reshape(-1).numpy()))
    print(f"{shape}: bucket max |d| {np.abs(got - want).max():.3e} against max |g| {scale:.3e}; " + "; ".join(report))
    assert len(report) == 4
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5 * scale, err_msg="; ".join(report))
    # these four are ~300 x smaller than the bucket's largest entry: the same rule at each tensor's own scale
    for name, g_got, g_want in own:
        np.testing.assert_allclose(g_got, g_want, rtol=1e-5, atol=1e-5 * np.abs(g_want).max(), err_msg=name)


# ------------------------------------------------------------------------------- 3. the forms at (3, 71, 5)
def test_forms_of_the_update_at_71_wide(monkeypatch):
    """One epoch (N = 96, B = 20: four full mini-batches and a tail of 16), as
    test_mat_update_with_more_row_tiles_than_one_operand_batch: (b) fused tail against the three-launch chain, bitwise;
    (c) the slab form against the chain, that test's bounds; and graphs on against off, bitwise."""
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.ppo import PermutationLoader
    shape, B = (3, 71, 5), 20
    n_mb = (E * T + B - 1) // B

    def first_minibatch(split):
        monkeypatch.setenv("PPOAF_SPLIT_WGRAD", split)
        ppo = _ppo(shape, B, epochs=1, use_graphs=False)
        pol = ppo.policies["mat"]
        ppo.rollout()
        pol.train()
        fused = ppo._fused_updater("mat", B)
        assert fused.split == (split == "1")
        perm = torch.randperm(len(pol.dataset), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        fused.begin_epoch(perm)
        args, lib, st = fused._args_for(B), _lib.load(), K.stream()
        _lib.check(lib.ppoaf_mat_update_fwd_bwd(C.byref(args), st), "mat fwd_bwd")
        _lib.check(lib.ppoaf_mat_update_reduce(C.byref(args), st), "mat reduce")
        torch.cuda.synchronize()
        return pol.actor_critic.flat_grads.clone(), fused.totals.clone(), pol.buffer.actions.clone()

    def epoch(split="1", tail="1", graphs=False):
        monkeypatch.setenv("PPOAF_SPLIT_WGRAD", split)
        monkeypatch.setenv("PPOAF_FUSED_TAIL", tail)
        ppo = _ppo(shape, B, epochs=1, use_graphs=graphs)
        pol = ppo.policies["mat"]
        ppo.rollout()
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._ppo_batch_train(loader, "mat")
        torch.cuda.synchronize()
        sd = ppo.status_dict["mat"]
        opt = pol.actor_critic_optim
        fused = ppo._fused_updater("mat", B)
        assert fused is not None and int(opt.step_count.item()) == n_mb
        assert fused.split == (split == "1") and (fused.tail_reason() == "") == (split == "1" and tail == "1"), fused.tail_reason()
        return dict(w=pol.actor_critic.flat_params.detach().clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                    g=pol.actor_critic.flat_grads.clone(), actions=pol.buffer.actions.clone(),
                    status=[sd[k] for k in ("actor loss", "critic loss", "kl avg", "weighted entropy")])

    chain, three, slabs, graphed = epoch(), epoch(tail="0"), epoch(split="0", tail="0"), epoch(graphs=True)
    for r in (three, slabs, graphed):
        assert torch.equal(r["actions"], chain["actions"])
    for k, what in (("w", "parameters"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("g", "gradient bucket of the last mini-batch")):
        assert torch.equal(chain[k], three[k]), f"tail / three launches: {what} differ, max |d| {float((chain[k] - three[k]).abs().max()):.3e}"
    for k, what in (("w", "parameters"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        assert torch.equal(chain[k], graphed[k]), f"graphs on / off: {what} differ, max |d| {float((chain[k] - graphed[k]).abs().max()):.3e}"
    assert chain["status"] == graphed["status"]
    (g1, t1, a1), (g0, t0, a0) = first_minibatch("1"), first_minibatch("0")
    assert torch.equal(a1, a0)
    scale, d = float(g0.abs().max()), float((g1 - g0).abs().max())
    print(f"slab form against the chain: max |dg| {d:.3e} against max |g| {scale:.3e}")
    assert d <= 1e-5 * scale, f"max |dg| {d:.3e} against max |g| {scale:.3e}"
    np.testing.assert_allclose(t1.cpu().numpy(), t0.cpu().numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(chain["status"], slabs["status"], rtol=2e-4, atol=1e-4)


# ------------------------------------------------------------------------------- 4. K20 up to 64 wide
K20_SHAPES = [(3, 33, 5), (3, 64, 5), (16, 64, 8)]
NET_SEED, OBS_SEED = 11, 111


def _network(A, O, NA):
    import mat_float64 as M
    from ppo_and_friends_amd.fused_update import _describe_mat
    ac = M.make_network(O, NA, A, NET_SEED, DEV)
    topo, why = _describe_mat(types.SimpleNamespace(actor_critic=ac, action_dtype="discrete"))
    assert topo is not None, why
    return ac, topo


def _fill(a, topo, ac):
    a.obs_dim, a.num_agents, a.num_actions, a.embedding = topo["obs_dim"], topo["num_agents"], topo["num_actions"], 64
    for i, o in enumerate(topo["offsets"]):
        a.offsets[i] = o
    a.params = ac.flat_params.data_ptr()


def _k16_actions(ac, topo, obs, seed, offset):
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    n, A, O = obs.shape
    a = _lib.MatStepArgs()
    _fill(a, topo, ac)
    a.actor_obs_dim, a.normalize_values, a.E = O, 0, n
    obs = obs.contiguous()
    a.critic_obs = obs.data_ptr()
    a.seed, a.offset = seed, offset
    act = torch.full((n, A), -1, dtype=torch.int64, device=DEV)
    logp, val = torch.zeros(n, A, device=DEV), torch.zeros(n, A, device=DEV)
    a.action_out, a.logp_out, a.value_out = act.data_ptr(), logp.data_ptr(), val.data_ptr()
    _lib.check(_lib.load().ppoaf_mat_policy_step(C.byref(a), K.stream()), "mat_policy_step")
    return act


def _k20_actions(ac, topo, obs, mode, seed=0, offset=0):
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    A, O = topo["num_agents"], topo["obs_dim"]
    n = obs.numel() // (A * O)
    a = _lib.MatInferArgs()
    _fill(a, topo, ac)
    obs = obs.contiguous()
    a.obs, a.E, a.mode, a.seed, a.offset = obs.data_ptr(), n, mode, seed, offset
    for i in range(A):
        a.slot_agent[i] = i
    a.obs_env_stride, a.obs_agent_stride, a.act_env_stride, a.act_agent_stride = A, 1, A, 1
    act = torch.full((n, A), -1, dtype=torch.int64, device=DEV)
    a.action_out = act.data_ptr()
    K.mat_policy_infer(a)
    return act


def _obs(n, A, O, seed):
    return torch.from_numpy((2 * np.random.default_rng(seed).standard_normal((n, A, O))).astype(np.float32)).to(DEV)


def _batch_sizes(A):
    per_tile = 16 // A
    return sorted(e for e in {1, per_tile - 1, 4 * per_tile, 4 * per_tile + 1, 4096} if e >= 1)


@pytest.mark.parametrize("shape", K20_SHAPES)
def test_k20_sampled_actions_are_k16s(shape):
    A, O, NA = shape
    ac, topo = _network(A, O, NA)
    for n in _batch_sizes(A):
        obs = _obs(n, A, O, seed=n)
        seed, offset = 0x1234ABCD5678 + n, 977 * n
        want = _k16_actions(ac, topo, obs, seed, offset)
        got = _k20_actions(ac, topo, obs, 0, seed, offset)
        assert int(want.min()) >= 0 and int(want.max()) < NA
        assert torch.equal(got, want), (shape, n, int((got != want).sum()))
        if n >= 16:
            assert len(torch.unique(got)) > 1


@pytest.mark.parametrize("shape", K20_SHAPES)
def test_k20_deterministic_against_float64(shape):
    """E = 1024, torch seed 11, obs seed 111: the float64 forward alone leaves out 0 of 3 072, 3 of 3 072 and 5 of
    16 384 decisions at these shapes (near-tie rule of tests/helpers/mat_float64.py); at most 0.25 % may be left out."""
    import mat_float64 as M
    A, O, NA = shape
    ac, topo = _network(A, O, NA)
    obs = _obs(1024, A, O, OBS_SEED)
    got = _k20_actions(ac, topo, obs, 1).cpu().numpy()
    want, logits = M.float64_logits_decode(ac.state_dict(), O, NA, A, obs.cpu().numpy())
    keep = M.compared_slots(logits)
    wrong = (got != want) & keep
    print(f"\n{shape}: {(~keep).sum()} of {keep.size} decisions left out, {(got != want).sum()} differ from float64, "
          f"{wrong.sum()} of them compared; classes {np.unique(got).tolist()}")
    assert (~keep).mean() <= 0.0025
    assert not wrong.any()
    assert len(np.unique(got)) > 1


def _eval_ppo(O, monkeypatch):
    """MATPolicy (3 agents, Discrete(5)) under "auto" in an env whose rows end; counters of K20 launches and module forwards."""
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.spaces import Box, Discrete
    steps = []

    class Counted(SyntheticFixedLengthEnv):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.term_table[-1] = True                     # every row finishes once per horizon

        def step(self, action):
            steps.append(1)
            return super().step(action)

    env_gen = lambda: Counted(9, O, Discrete(5), 40, DEV, reward="uniform", seed=5, term_prob=0.08, num_agents=3)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"agent": (MATPolicy, sp, sp, Discrete(5), {})}, device=DEV, random_seed=1, envs_per_proc=9,
              ts_per_rollout=16, batch_size=16, save_state=False, update_mode="auto", normalize_obs=False, normalize_rewards=False)
    pol = ppo.policies["agent"]
    k20, modules = [], []
    infer = K.mat_policy_infer
    monkeypatch.setattr(K, "mat_policy_infer", lambda a: (k20.append(a.mode), infer(a))[1])
    for net in (pol.actor, pol.critic):
        inner = net.forward
        monkeypatch.setattr(net, "forward", lambda *a, _f=inner, **k: (modules.append(1), _f(*a, **k))[1])
    return ppo, pol, steps, k20, modules


def test_evaluation_of_a_64_wide_policy_is_one_k20_launch_per_step(monkeypatch):
    from ppo_and_friends_amd.testing import test_policy
    ppo, pol, steps, k20, modules = _eval_ppo(64, monkeypatch)
    assert pol.fused_step_unsupported_reason() == "" and pol.inference_unsupported_reason() == ""
    info = test_policy(ppo, 20, deterministic=True, check_every=5, max_steps=4000)
    assert info["num_test_runs"] == 20 and len(steps) > 0
    assert k20 == [1] * len(steps) and not modules


def test_evaluation_of_a_71_wide_policy_decodes_on_the_modules_and_says_why(monkeypatch, capfd):
    from ppo_and_friends_amd.testing import test_policy
    ppo, pol, steps, k20, modules = _eval_ppo(71, monkeypatch)
    assert pol.fused_step_unsupported_reason() == ""                    # K16 and K15 take it
    why = pol.inference_unsupported_reason()
    assert "observations 71 wide" in why and "64" in why
    info = test_policy(ppo, 20, deterministic=True, check_every=5, max_steps=4000, verbose=True)
    assert info["num_test_runs"] == 20 and len(steps) > 0
    assert not k20 and modules
    assert why in capfd.readouterr().out


# ------------------------------------------------------------------------------- 5. MAT + identity-encoder ICM
def test_wide_mat_with_identity_icm_against_the_torch_paths():
    """(3, 71, 5) with an identity-encoder ICM of model width 32 (robot_warehouse's baseline shape): K16 steps the
    rollout, K15 runs the policy epoch and K14 the ICM epoch of one iteration; then both epochs against
    update_mode="torch" on identical rollouts, within the bounds of test_fused_mat_and_icm_paths_fuzz_against_the_torch_paths
    (its K16 check, teacher-forced on the kernel's own actions, included)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    shape, B = (3, 71, 5), 20
    A, O, NA = shape
    icm = dict(encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=32)

    def iteration(ppo, pol):
        ppo.rollout()
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._ppo_batch_train(loader, "mat")
        ppo._icm_batch_train(loader, "mat")
        torch.cuda.synchronize()

    # all three kernels in one iteration
    ppo = _ppo(shape, B, epochs=1, icm=icm, use_graphs=False)
    pol = ppo.policies["mat"]
    assert pol.fused_step_unsupported_reason() == "" and ppo._fused_updater("mat", B) is not None
    upd = ppo._fused_icm_updater("mat")
    assert upd is not None and upd.topo.get("identity")
    steps = _count_rollout_steps(pol)
    iteration(ppo, pol)
    assert len(steps) == T
    assert int(pol.actor_critic_optim.step_count.item()) == -(-E * T // B) == int(pol.icm_optim.step_count.item())
    assert torch.isfinite(pol.policy_params).all() and torch.isfinite(pol.icm_model.flat_params).all()

    # K16 against the modules, teacher-forced on its own actions
    ppo = _ppo(shape, B, epochs=1, icm=icm, use_graphs=False)
    pol = ppo.policies["mat"]
    ppo.rollout()
    buf = pol.buffer
    flat = lambda x: x.reshape((T * E,) + tuple(x.shape[2:]))
    k = torch.as_tensor(np.argsort(np.argsort(pol.agent_slot_order())[pol._dataset_slot_order]), device=DEV)
    ro = lambda x: flat(x).index_select(1, k)
    with torch.no_grad():
        v, lp, _ = pol.evaluate(ro(buf.critic_observations), ro(buf.observations), ro(buf.raw_actions))
    np.testing.assert_allclose(ro(buf.log_probs).cpu().numpy(), lp.reshape(T * E, A).cpu().numpy(), rtol=3e-5, atol=3e-5)
    vn = ppo.value_normalizers["mat"]
    np.testing.assert_allclose(ro(buf.values).cpu().numpy(), vn.denormalize(v.reshape(T * E, A)).cpu().numpy(), rtol=3e-5, atol=3e-5)

    # K15 and K14 against the torch epochs on identical (torch-sampled) rollouts
    res = []
    for mode in ("fused", "torch"):
        ppo = _ppo(shape, B, mode=mode, epochs=1, icm=icm, use_graphs=False)
        pol = ppo.policies["mat"]
        assert (ppo._fused_updater("mat", B) is not None) == (mode == "fused")
        assert (ppo._fused_icm_updater("mat") is not None) == (mode == "fused")
        pol.fused_step_unsupported_reason = lambda: "torch rollout forced by the test"
        iteration(ppo, pol)
        sd = ppo.status_dict["mat"]
        res.append(dict(w=pol.actor_critic.flat_params.detach().cpu().numpy().copy(), a=pol.buffer.actions.cpu().numpy().copy(),
                        s=[sd[k] for k in ("actor loss", "critic loss", "kl avg", "weighted entropy")],
                        iw=pol.icm_model.flat_params.detach().cpu().numpy().copy(), r=pol.buffer.rewards.cpu().numpy().copy(),
                        il=sd["icm loss"]))
    f, t = res
    np.testing.assert_array_equal(f["a"], t["a"])
    np.testing.assert_allclose(f["r"], t["r"], rtol=3e-5, atol=3e-6)
    np.testing.assert_allclose(f["s"], t["s"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(f["w"], t["w"], rtol=2e-4, atol=3e-5)
    np.testing.assert_allclose(f["il"], t["il"], rtol=5e-5)
    np.testing.assert_allclose(f["iw"], t["iw"], rtol=2e-4, atol=3e-5)


# ------------------------------------------------------------------------------- 6. multi-rank rehearsal
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_multi_rank_rehearsal_matches_single_rank(tmp_path):
    """One rank through the N > 1 path (PPOAF_REHEARSE_MULTI_RANK=1: process group, per-mini-batch gradient exchange sized by
    the 71-wide bucket, record all-gathers) in a child process, against the single-rank path in another; the bounds of
    test_gpu_action_heads.py::test_multi_rank_rehearsal_matches_single_rank."""
    outs = {}
    for tag, rehearse in (("single", "0"), ("rehearsal", "1")):
        env = dict(os.environ, PPOAF_REHEARSE_MULTI_RANK=rehearse, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PPOAF_BACKEND"):
            env.pop(k, None)
        out = str(tmp_path / f"{tag}.npz")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "mat_wide_rank_run.py"), out],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[tag] = np.load(out)
    s, r = outs["single"], outs["rehearsal"]
    assert bool(r["multi"]) and not bool(s["multi"])
    np.testing.assert_allclose(r["stats"], s["stats"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(r["params"], s["params"], rtol=1e-4, atol=2e-5)
