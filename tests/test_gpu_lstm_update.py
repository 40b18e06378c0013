"""
K22 (csrc/lstm_update.hip, fused_update.FusedLstmUpdate): the fused mini-batch update epoch of LSTM policies against the
mini-batch loop it replaces (`pol.fused_lstm_update = False`), the CPU port of the reference's LSTM flow, torch autograd
through the K18 modules, itself (graph replay against eager launches, seeded reruns) and a second rank.

Setup of every case (the configuration of test_gpu_lstm_hip.py's _lstm_ppo): 5 observations, 6 envs x 20 steps = 120
rows, episodes cut after 7 steps and terminated with probability 0.05-0.08, so terminal positions fall inside windows.
At S = 4 that is 117 items: B = 16 gives 7 full mini-batches and a tail of 5 (a partial row tile), B = 29 gives 4 full
and a tail of 1 -- the mini-batch that is not launched but whose record still reaches the value normaliser.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HERE = os.path.dirname(os.path.abspath(__file__))
E, T, O = 6, 20, 5
TABLES = ("actor_hidden", "actor_cell", "critic_hidden", "critic_cell")

# action, H, F, depth, S, B: the three kernel widths (H = 128: W_hh re-read every step, the LDS maximum with F 128, depth 2,
# S 16), both heads, S = 1 (no windows), the partial tile and the skipped size-1 tail
CASES = [
    ("discrete", 32, 16, 1, 4, 16),
    ("continuous", 32, 16, 1, 4, 29),
    ("continuous", 64, 32, 2, 1, 16),
    ("discrete", 128, 128, 2, 16, 16),
]


def _ppo(action="discrete", H=32, F=16, depth=1, S=4, B=16, seed=1, term_prob=0.05, use_graphs=True, mode="fused", max_ts=7):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    act_space = Discrete(3) if action == "discrete" else Box(-1.0, 1.0, (2,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, act_space, T, DEV, reward="uniform", seed=13, term_prob=term_prob)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    kw = dict(sequence_length=S, lstm_hidden_size=H, ff_hidden_size=F, ff_hidden_depth=depth)
    return PPO(env_gen, {"p": (None, sp, sp, act_space, dict(ac_network=LSTMNetwork, actor_kw_args=dict(kw), critic_kw_args=dict(kw)))},
               device=DEV, random_seed=seed, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
               batch_size=B, epochs_per_iter=2, max_ts_per_ep=max_ts, save_state=False, update_mode=mode, use_graphs=use_graphs)


def _epochs(ppo, n=2):
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol = ppo.policies["p"]
    pol.train()
    stats = []
    for _ in range(n):
        ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator), "p")
        sd = ppo.status_dict["p"]
        stats.append([float(sd[k]) for k in ("actor loss", "critic loss", "kl avg", "weighted entropy")])
    torch.cuda.synchronize()
    return np.asarray(stats)


def _state(ppo):
    """What an update epoch leaves behind: weights, optimiser state, hidden tables, values, the value normaliser."""
    pol = ppo.policies["p"]
    rs = ppo.value_normalizers["p"].running_stats
    out = dict(params=pol.policy_params, exp_avg=pol.policy_exp_avg, exp_avg_sq=pol.policy_exp_avg_sq,
               steps=pol.policy_step_counts, values=pol.buffer.values, vn_mean=rs.mean_t, vn_var=rs.var_t, vn_count=rs.count_t)
    out.update({k: pol.buffer.hidden[k] for k in TABLES})
    return {k: v.detach().clone() for k, v in out.items()}


def _run(loop, case, epochs=2, start=None, **kw):
    action, H, F, depth, S, B = case
    ppo = _ppo(action, H, F, depth, S, B, **kw)
    pol = ppo.policies["p"]
    if loop:
        pol.fused_lstm_update = False
    if start is not None:
        with torch.no_grad():
            pol.policy_params.copy_(start)
    w0 = pol.policy_params.detach().clone()
    ppo.rollout()
    stats = _epochs(ppo, epochs)
    return ppo, w0, stats


# ----------------------------------------------------------------------------------------------------------------------
# 1. the driver is there and the loop is not used
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("action,B,n_full,tail,n_done", [("discrete", 16, 7, 5, 8), ("continuous", 29, 4, 1, 4)])
def test_the_driver_runs_the_epoch_and_the_loop_is_not_used(monkeypatch, action, B, n_full, tail, n_done):
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    from ppo_and_friends_amd.ppo import PPO

    def refuse(*a, **k):
        raise AssertionError("the mini-batch loop / autograd ran under K22")
    ppo = _ppo(action, B=B, use_graphs=False)
    pol = ppo.policies["p"]
    upd = ppo._fused_updater("p", B)
    assert isinstance(upd, FusedLstmUpdate)
    monkeypatch.setattr(PPO, "_minibatch_step", refuse)
    monkeypatch.setattr(torch.autograd, "backward", refuse)
    w0 = pol.policy_params.clone()
    ppo.rollout()
    assert len(pol.dataset) == 117
    before = FusedLstmUpdate.launches
    stats = _epochs(ppo, 2)
    assert (upd.n_full, upd.tail, upd.n_done) == (n_full, tail, n_done)
    launches = FusedLstmUpdate.launches - before
    assert launches == 3 * 2 * n_done and launches <= 4 * 2 * n_done          # eager launches: every one is counted
    assert np.isfinite(stats).all() and torch.isfinite(pol.policy_params).all() and not torch.equal(w0, pol.policy_params)
    assert pol.policy_step_counts.tolist() == [2 * n_done, 2 * n_done]
    # every item's record reached the value normaliser, the skipped size-1 mini-batch's included (quirk Q9)
    rs = ppo.value_normalizers["p"].running_stats
    np.testing.assert_allclose(float(rs.count_t.item()), 1e-4 + 2 * 117, rtol=1e-12)
    monkeypatch.undo()
    pol.fused_lstm_update = False
    assert ppo._fused_updater("p", B) is None
    pol.fused_lstm_update = True
    assert ppo._fused_updater("p", B) is upd


# ----------------------------------------------------------------------------------------------------------------------
# 2. K22 against the loop
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_two_epochs_match_the_minibatch_loop(case):
    """Two PPO objects from one seed, the second on the loop: identical rollouts (K21), then two epochs each -- the second
    epoch reads the states and values the first wrote back.  Tolerances: the project's own for a fused-against-unfused
    epoch (test_grouped_icm_epoch_fused_against_the_torch_path): losses rtol 5e-5, weights and tables rtol 2e-4, atol 3e-5."""
    a, w0, stats_a = _run(False, case)
    b, w0_b, stats_b = _run(True, case, start=w0)
    assert torch.equal(w0, w0_b)
    pa, pb = a.policies["p"], b.policies["p"]
    assert torch.equal(pa.buffer.actions, pb.buffer.actions) and torch.equal(pa.buffer.log_probs, pb.buffer.log_probs)
    sa, sb = _state(a), _state(b)
    print(f"{case}: stats K22 {stats_a.tolist()} loop {stats_b.tolist()}")
    for k in sa:
        d = float((sa[k].double() - sb[k].double()).abs().max())
        print(f"{case}: {k} max |K22 - loop| {d:.3e} (max |loop| {float(sb[k].double().abs().max()):.3e})")
    assert not torch.equal(sa["params"], w0)
    assert torch.equal(sa["steps"], sb["steps"])
    np.testing.assert_allclose(stats_a[:, :2], stats_b[:, :2], rtol=5e-5, err_msg="actor / critic loss per epoch")
    # KL and entropy averages are differences / sums of log-probs of magnitude ~1 (3 classes, 2 Gaussian dimensions): their
    # f32 rounding (6e-8 per operation, a few operations per row) does not shrink with the statistic itself
    np.testing.assert_allclose(stats_a[:, 2:], stats_b[:, 2:], rtol=5e-5, atol=1e-6, err_msg="kl avg / weighted entropy per epoch")
    for k in ("params", "exp_avg", "exp_avg_sq", "values", "vn_mean", "vn_var", "vn_count") + TABLES:
        np.testing.assert_allclose(sa[k].cpu().numpy(), sb[k].cpu().numpy(), rtol=2e-4, atol=3e-5, err_msg=k)


# ----------------------------------------------------------------------------------------------------------------------
# 3. K22 against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _against_the_cpu_port(loop, S, max_ts, term_prob, H):
    """test_gpu_lstm_hip.py's test_fused_lstm_policy_matches_the_cpu_port, on K22 or on the loop -> worst weight deviation."""
    from oracle import lstm_oracle
    from ppo_and_friends_amd.ppo import PermutationLoader
    NA, B, seed = 3, 16, 2
    ppo = _ppo("discrete", H, H, 1, S, B, seed=seed, term_prob=term_prob, max_ts=max_ts)
    ppo.epochs_per_iter = 1
    pol = ppo.policies["p"]
    pol.fused_lstm_update = not loop
    assert pol.actor.use_hip and (ppo._fused_updater("p", B) is not None) == (not loop)
    cpu = lstm_oracle.CpuLSTMPPO(O, NA, sequence_length=S, lstm_hidden=H, ff_hidden=H, batch_size=B, seed=seed)
    cpu.actor.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor.state_dict().items()})
    cpu.critic.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.critic.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    flat = lambda net: torch.cat([p.detach().cpu().reshape(-1) for p in net.parameters()]).numpy()
    for it in range(2):
        ds = ppo.rollout()
        env = ppo.env
        term = None if env.term_table is None else env.term_table.cpu().numpy()
        ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(), pol.buffer.actions[..., 0].cpu().numpy(),
                          term, max_ts_per_ep=max_ts)
        tol = dict(rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(ds.log_probs.cpu().numpy(), ref.log_probs.numpy().reshape(-1), **tol)
        np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
        np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(), **tol)
        np.testing.assert_allclose(ds.critic_cell[torch.arange(E * T)].cpu().numpy(), ref.critic_cell.numpy(), **tol)
        pol.train()
        ppo._ppo_batch_train(PermutationLoader(pol.dataset, B, ppo.loader_generator, ppo._perm_cache), "p")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg"):
            np.testing.assert_allclose(ppo.status_dict["p"][k], r[k], rtol=1e-4, atol=1e-5, err_msg=f"{k} it={it}")
        np.testing.assert_allclose(ds.actor_hidden[torch.arange(E * T)].cpu().numpy(), ref.actor_hidden.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(flat(pol.actor), flat(cpu.actor), rtol=2e-4, atol=5e-5)
    np.testing.assert_allclose(flat(pol.critic), flat(cpu.critic), rtol=2e-4, atol=5e-5)
    return max(float(np.abs(flat(pol.actor) - flat(cpu.actor)).max()), float(np.abs(flat(pol.critic) - flat(cpu.critic)).max()))


@pytest.mark.parametrize("S,max_ts,term_prob,H", [(4, 7, 0.05, 32), (10, 200, 0.08, 128)])
def test_k22_matches_the_cpu_port_as_closely_as_the_loop(S, max_ts, term_prob, H):
    """Two iterations against oracle/lstm_oracle.CpuLSTMPPO with the tolerances of the loop's own test; K22's worst weight
    deviation is at most twice the loop's (two f32 chains that differ in summation order may differ by that; a wrong term
    will not)."""
    k22 = _against_the_cpu_port(False, S, max_ts, term_prob, H)
    loop = _against_the_cpu_port(True, S, max_ts, term_prob, H)
    print(f"S {S} H {H}: worst weight deviation from the CPU port: K22 {k22:.3e}, loop {loop:.3e}")
    assert k22 <= 2.0 * loop, (k22, loop)


# ----------------------------------------------------------------------------------------------------------------------
# 4. replay equals eager, reruns are bitwise
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=lambda c: "-".join(map(str, c)))
def test_graph_replay_equals_eager_launches_and_reruns_are_bitwise(case, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    monkeypatch.setattr(FusedLstmUpdate, "graph_chunk", 2)
    runs = []
    for use_graphs in (True, False, True):
        ppo, w0, stats = _run(False, case, use_graphs=use_graphs)
        upd = ppo._fused_updater("p", case[5])
        assert bool(upd._graphs) == use_graphs, "7 full mini-batches in chunks of 2: captured and replayed"
        runs.append((_state(ppo), stats, w0))
    assert torch.equal(runs[0][2], runs[1][2])
    for other, what in ((1, "graph replay against eager launches"), (2, "two seeded runs")):
        for k, v in runs[0][0].items():
            assert torch.equal(v, runs[other][0][k]), f"{what}: {k}"
        assert np.array_equal(runs[0][1], runs[other][1]), what


# ----------------------------------------------------------------------------------------------------------------------
# 5. the gradient of one mini-batch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("action", ["discrete", "continuous"])
@pytest.mark.parametrize("rows", [16, 5])
def test_one_minibatch_gradient_matches_autograd_through_the_k18_modules(action, rows):
    """fwd_bwd + wgrad (gradient_only) against torch autograd over PPO._minibatch_step on the same mini-batch (K18 modules,
    distribution and loss kernels), per tensor at test_network_matches_torch_cpu's gradient tolerance: 1e-5 x max |g|.
    rows = 16: the first mini-batch (a full tile); rows = 5: the epoch's tail (mini-batch 7, a partial tile)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    B = 16
    ppo = _ppo(action, 64, 32, 2, 4, B, use_graphs=False)
    pol = ppo.policies["p"]
    ppo.rollout()
    pol.train()
    upd = ppo._fused_updater("p", B)
    perm = PermutationLoader(pol.dataset, B, ppo.loader_generator).epoch_permutation()
    upd.begin_epoch(perm)
    mb = 0 if rows == B else upd.n_full
    assert rows == B or upd.tail == rows
    upd.cursor.fill_(mb)
    for t in (upd.vn_mean, upd.vn_var, upd.vn_count):
        t[1] = t[0]                                                    # (mini-batch 7 reads slot 1)
    keep = {k: v.clone() for k, v in pol.buffer.hidden.items()}
    values = pol.buffer.values.clone()
    upd.gradient_only(upd._args_for(rows))
    torch.cuda.synchronize()
    got = pol.policy_grads.clone()
    tables = {k: v.clone() for k, v in pol.buffer.hidden.items()}
    values_k22 = pol.buffer.values.clone()
    for k, v in keep.items():
        pol.buffer.hidden[k].copy_(v)
    pol.buffer.values.copy_(values)
    totals = torch.zeros(9, dtype=torch.float64, device=DEV)
    ppo._minibatch_step("p", pol.dataset, perm[mb * B:mb * B + rows].contiguous(), upd.records[mb].reshape(1, 3), totals)
    torch.cuda.synchronize()
    want = pol.policy_grads.clone()
    assert float(want.abs().max()) > 0
    base = pol.policy_grads.data_ptr()
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        for name, p in net.named_parameters():
            off = (p.grad.data_ptr() - base) // 4
            g, w = got[off:off + p.numel()].cpu().numpy(), want[off:off + p.numel()].cpu().numpy()
            scale = float(np.abs(w).max())
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-5 * scale + 1e-12, err_msg=f"{tag}.{name} (max |g| {scale:.3e})")
    # what fwd_bwd wrote back on the way: the final states and the values of the mini-batch's last positions
    for k in TABLES:
        np.testing.assert_allclose(tables[k].cpu().numpy(), pol.buffer.hidden[k].cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg=k)
        assert not torch.equal(tables[k], keep[k])
    np.testing.assert_allclose(values_k22.cpu().numpy(), pol.buffer.values.cpu().numpy(), rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------------------------------------------------
# 6. the optimiser state is shared with the loop and with checkpoints
# ----------------------------------------------------------------------------------------------------------------------
def test_optimiser_state_is_shared_with_the_loop_and_checkpoints(tmp_path):
    ppo = _ppo("discrete", 32, 32, 1, 4, 16)
    pol = ppo.policies["p"]
    ppo.rollout()
    _epochs(ppo, 1)
    assert pol.policy_step_counts.tolist() == [8, 8]
    m_after_k22 = pol.policy_exp_avg.clone()
    pol.fused_lstm_update = False
    assert ppo._fused_updater("p", 16) is None
    stats = _epochs(ppo, 1)
    assert pol.policy_step_counts.tolist() == [16, 16], "the loop continues K22's step counts"
    assert np.isfinite(stats).all() and torch.isfinite(pol.policy_params).all()
    assert not torch.equal(m_after_k22, pol.policy_exp_avg)
    pol.save(str(tmp_path))
    pol_a = _ppo("discrete", 32, 32, 1, 4, 16, seed=5, mode="auto").policies["p"]
    assert not pol_a.actor.use_hip
    pol_a.load(str(tmp_path))
    assert pol_a.policy_step_counts.tolist() == [16, 16]
    assert torch.equal(pol_a.policy_exp_avg, pol.policy_exp_avg) and torch.equal(pol_a.policy_exp_avg_sq, pol.policy_exp_avg_sq)
    x = torch.randn(40, 4, O, device=DEV)
    for tag in ("actor", "critic"):
        net_f, net_a = getattr(pol, tag), getattr(pol_a, tag)
        assert list(net_f.state_dict().keys()) == list(net_a.state_dict().keys())
        with torch.no_grad():
            net_f.reset_hidden_state(40, DEV)
            net_a.reset_hidden_state(40, DEV)
            y_f, y_a = net_f.forward_logits(x), net_a.forward_logits(x)
        np.testing.assert_allclose(y_f.cpu().numpy(), y_a.cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg=tag)


# ----------------------------------------------------------------------------------------------------------------------
# 7. two ranks on one GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["peer", "rccl"])
def test_two_ranks_stay_identical_and_match_the_loop(tmp_path, mode):
    """Two fresh processes on the one GPU (tests/helpers/lstm_update_rank.py, collectives over gloo), each under its own time
    limit: K22 with the K17 peer exchange / with the all-reduce fallback between wgrad and Adam, then the loop on two ranks."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PPOAF_GRAD_EXCHANGE=mode, PPOAF_SHARE_DEVICE="1", PPOAF_BACKEND="gloo")
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.join(HERE, "helpers", "lstm_update_rank.py"), str(tmp_path)],
                              cwd=os.path.dirname(HERE), env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(outs)[-4000:]      # (nothing further is started after a failure)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(2))
    assert r0["exchange"] == r1["exchange"] == ("peer" if mode == "peer" else "allreduce")
    assert r0["n_done"] == 8 and r0["launches"] == 4 * 2 * 8, "fwd_bwd, wgrad, the exchange / norm pass, adam"
    assert not torch.equal(r0["obs"], r1["obs"]), "each rank rolls out its own envs"
    for leg in ("k22", "loop"):
        for k in ("w0_", "w_", "exp_avg_", "exp_avg_sq_", "steps_"):
            assert torch.equal(r0[k + leg], r1[k + leg]), f"{k}{leg}: the replicas differ"
    assert r0["steps_k22"].tolist() == [16, 16] and not torch.equal(r0["w_k22"], r0["w0_k22"])
    assert torch.equal(r0["w0_k22"], r0["w0_loop"]) and torch.equal(r0["actions_k22"], r0["actions_loop"]), "the legs' starting points"
    print(f"{mode}: stats K22 {r0['stats_k22']} loop {r0['stats_loop']}, max |dw| {float((r0['w_k22'] - r0['w_loop']).abs().max()):.3e}")
    np.testing.assert_allclose(r0["stats_k22"], r0["stats_loop"], rtol=5e-5)
    for k in ("w_", "exp_avg_", "exp_avg_sq_"):
        np.testing.assert_allclose(r0[k + "k22"].numpy(), r0[k + "loop"].numpy(), rtol=2e-4, atol=3e-5, err_msg=k)
