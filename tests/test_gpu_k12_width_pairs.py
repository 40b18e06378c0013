"""
-m gpu: the narrow-actor width pairs (64, 256), (32, 256) and (32, 64) of K6+K7 and K12 (csrc/ppo_update_narrow.hip and the
pair list of csrc/ppo_update_dev.hpp), on every path a policy of these widths takes:

  * one mini-batch against float64 on all four forms of K12 (the cases and the bound of tests/test_gpu_k12_gradients.py);
  * the critic's row tiles on workgroup pairs, beside one workgroup per actor tile, bitwise against one workgroup per tile
    (the procedure of tests/test_gpu_row_pairs.py), and the fused tail bitwise against the wgrad + Adam launches;
  * a whole iteration against the CPU port under "fused" and "auto", and the rollout buffer's values and log-probs (K6+K7)
    against the policy's networks in float64;
  * the PPO chain confined to half of the XCDs beside the ICM chain, bitwise against the two epochs in turn;
  * two ranks on the one device, the peer exchange inside the fused tail against the all-reduce loop.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import cpu_ppo_loop
from oracle import k12_oracle as ko

import test_gpu_k12_gradients as g12
import test_gpu_row_pairs as rp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import width_pairs_rank  # noqa: E402

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- one mini-batch
K12_CASES = {
    "w64x256": g12.case(O=11, ha=64, hc=256, depth=2, B=96, wide_critic=True, head=("gaussian", 3), act="relu", seed=320),
    "w32x256": g12.case(O=7, ha=32, hc=256, depth=3, B=40, head=("categorical", 5), act="tanh", seed=288),     # ragged last tile
    "w32x64": g12.case(O=16, ha=32, hc=64, depth=1, B=17, head=("bernoulli", 3), act="leaky_relu", seed=96),
    # critic depth 1: not pair-eligible, the plain <4,16> kernel inside the default chain
    "w64x256_d1": g12.case(O=9, ha=64, hc=256, depth=1, B=33, head=("multi_categorical", (2, 3)), seed=321),
    "w64x256_d4_in160": g12.case(O=160, ha=64, hc=256, depth=4, B=64, seed=322),           # the LDS edge of a 256-wide network
    "w32x256_in65_B513": g12.case(O=65, ha=32, hc=256, depth=2, B=513, seed=289),          # past the split chain: slabs by fallback
    "w64x256_no_norm": g12.case(ha=64, hc=256, norm_adv=False, norm_values=False, huber=False, kl=0.3, seed=323),
}


@pytest.mark.parametrize("name", sorted(K12_CASES))
def test_k12_minibatch_against_float64(name, monkeypatch):
    g12.run_case(K12_CASES[name], monkeypatch)


# ---------------------------------------------------------------------------------------------------- row pairs
PAIR_CASES = {
    "w64x256_ragged": dict(widths=(64, 256), depth=3, O=18, A=3, cont=False, B=200, act="relu"),       # 13 tiles + a tail mini-batch
    "w32x256_wide_input": dict(widths=(32, 256), depth=2, O=20, A=3, cont=True, B=96, act="tanh"),     # critic in_dim 60: not staged
}


def _same(got, ref, what):
    for i, name in enumerate(("parameters", "exp_avg", "exp_avg_sq", "values")):
        assert torch.equal(got[i], ref[i]), f"{what}: {name} differ, max |d| {float((got[i] - ref[i]).abs().max()):.3e}"
    assert got[4] == ref[4] and got[5] == ref[5], (what, got[4], ref[4])


@pytest.mark.parametrize("case", sorted(PAIR_CASES))
def test_row_pairs_beside_a_narrow_actor_are_bitwise_one_workgroup_per_tile(case, monkeypatch):
    monkeypatch.setattr(rp, "CASES", dict(rp.CASES, **PAIR_CASES))
    ref = rp._run(case, False, monkeypatch, graphs=False)        # (_run asserts pairs_reason() and the growth of pair_launches)
    paired = {}
    for graphs in (False, True):
        paired[graphs] = rp._run(case, True, monkeypatch, graphs=graphs)
        _same(paired[graphs], ref, f"{case} graphs={graphs}")
    if case == "w64x256_ragged":
        monkeypatch.setenv("PPOAF_FUSED_TAIL", "0")
        _same(rp._run(case, True, monkeypatch, graphs=False), paired[False], f"{case} PPOAF_FUSED_TAIL=0")


# ---------------------------------------------------------------------------------------------------- a whole iteration
def _f64_rule(got, want64, want32, name):
    bad = ko.failures(np.asarray(got, np.float64).reshape(-1), np.asarray(want64, np.float64).reshape(-1),
                      np.asarray(want32, np.float64).reshape(-1), [("", name, 0, (int(np.asarray(got).size),))])
    assert not bad, "; ".join(bad[:6])


def _buffer_against_float64(ppo, name, widths):
    """values and log_probs of the rollout buffer (K6+K7) against the policy's networks on the buffer's observations and raw
    actions, in float64 (and in float32 on the CPU, for the bound)."""
    pol = ppo.policies[name]
    buf = pol.buffer
    N = buf.num_transitions
    flat = lambda x: x.view((N,) + tuple(x.shape[2:])).detach().cpu()
    obs, cobs, raw = flat(buf.observations), flat(buf.critic_observations), flat(buf.raw_actions)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    gauss = hasattr(pol.actor.distribution, "log_std")
    rs = ppo.value_normalizers[name].running_stats if ppo.normalize_values else None
    out = {}
    for dt in (torch.float64, torch.float32):
        actor = cpu_ppo_loop.make_mlp(obs.shape[1], pol.actor.out_size, widths[0], 3).to(dt)
        critic = cpu_ppo_loop.make_mlp(cobs.shape[1], 1, widths[1], 3).to(dt)
        actor.load_state_dict(strip(pol.actor.state_dict()))
        critic.load_state_dict(strip(pol.critic.state_dict()))
        with torch.no_grad():
            z, v = actor(obs.to(dt)), critic(cobs.to(dt)).reshape(-1)
            if rs is not None:
                v = rs.mean_t.cpu().to(dt) + v * torch.sqrt(rs.var_t.cpu().to(dt) + 1e-8)
            if gauss:
                x = raw.to(dt)
                sd = torch.clamp(torch.nn.functional.softplus(pol.actor.distribution.log_std.detach().cpu().to(dt)),
                                 min=pol.actor.distribution.min_std)
                lp = torch.clamp(-(x - z) ** 2 / (2 * sd * sd) - torch.log(sd) - 0.5 * np.log(2 * np.pi), -100.0, 100.0).sum(-1)
                lp = lp - torch.log(torch.clamp(1 - torch.tanh(x) ** 2, min=1e-6)).sum(-1)
            else:
                p = torch.softmax(z, -1)
                p = torch.clamp(p / p.sum(-1, keepdim=True), float(np.finfo(np.float32).eps), 1 - float(np.finfo(np.float32).eps))
                lp = torch.log(p).gather(1, raw.long().reshape(-1, 1)).reshape(-1)
        out[dt] = (v.double().numpy(), lp.double().numpy())
    _f64_rule(flat(buf.values).numpy(), out[torch.float64][0], out[torch.float32][0], "values")
    _f64_rule(flat(buf.log_probs).numpy(), out[torch.float64][1], out[torch.float32][1], "log_probs")


def _team_ppo(widths, space, E, update_mode):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    dev = torch.device("cuda", 0)
    A, T, O, B, seed = 3, 10, 18, 48, 4
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, space, T, dev, reward="uniform", seed=21,
                                              num_agents=A, critic_view="policy", term_prob=0.05)
    sp, csp = Box(-np.inf, np.inf, (O,), np.float32), Box(-np.inf, np.inf, (A * O,), np.float32)
    pargs = dict(actor_kw_args=dict(hidden_size=widths[0]), critic_kw_args=dict(hidden_size=widths[1]))
    return PPO(env_gen, {"team": (None, sp, csp, space, pargs)}, device=dev, random_seed=seed, normalize_obs=False,
               normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2,
               update_mode=update_mode)


@pytest.mark.parametrize("update_mode", ["fused", "auto"])
def test_mappo_shared_policy_three_agents_actor_64_critic_256(update_mode):
    """tests/test_gpu_end_to_end.py::test_mappo_shared_policy_three_agents with a 64-wide actor: its shape, its assertions, its
    tolerances (the same networks one width apart)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    from ppo_and_friends_amd.spaces import Discrete
    A, E, T, O, NA, B, seed = 3, 6, 10, 18, 5, 48, 4
    ppo = _team_ppo((64, 256), Discrete(NA), E, update_mode)
    pol = ppo.policies["team"]
    assert pol.fused_step_unsupported_reason() == ""
    assert ppo._fused_updater("team", B) is not None, "a 64 / 256 policy trains on the fused path"
    cpu = cpu_ppo_loop.CpuPPO(O, NA, hidden=64, batch_size=B, seed=seed, critic_obs_dim=A * O, critic_hidden=256)
    strip = lambda sd: {k.replace("sequential_net.", ""): v.detach().cpu().clone() for k, v in sd.items()
                        if k.startswith("sequential_net.")}
    cpu.actor.load_state_dict(strip(pol.actor.state_dict()))
    cpu.critic.load_state_dict(strip(pol.critic.state_dict()))
    cpu.loader_generator = torch.Generator().manual_seed(seed)
    ds = ppo.rollout()
    env = ppo.env
    assert len(ds) == A * E * T
    _buffer_against_float64(ppo, "team", (64, 256))                  # K6+K7 at <4,16>
    ref = cpu.rollout(env.obs_table.cpu().numpy(), env.reward_table.cpu().numpy(),
                      actions=pol.buffer.actions[..., 0].cpu().numpy(),
                      term_table=env.term_table.cpu().numpy(),
                      critic_obs_table=env.critic_obs_table.cpu().numpy())
    tol = dict(rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(ds.critic_observations.cpu().numpy(), ref.critic_observations.numpy())
    np.testing.assert_allclose(ds.advantages.cpu().numpy(), ref.advantages.numpy(), **tol)
    np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rewards_to_go.numpy(), **tol)
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    pol.train()
    flat_params = lambda net: torch.cat([p.detach().cpu().reshape(-1) for p in net.parameters()]).numpy()
    for _ in range(2):
        ppo._ppo_batch_train(loader, "team")
        r = cpu.train_epoch()
        for k in ("actor loss", "critic loss", "kl avg", "weighted entropy"):
            np.testing.assert_allclose(ppo.status_dict["team"][k], r[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(flat_params(pol.critic), flat_params(cpu.critic), rtol=1e-4, atol=2e-5)


def test_rollout_buffer_actor_32_critic_64_fewer_rows_than_a_tile():
    """K6+K7 at <2,4>: Box(2), 3 agents x 5 envs = 15 rows per step."""
    from ppo_and_friends_amd.spaces import Box
    ppo = _team_ppo((32, 64), Box(-1.0, 1.0, (2,), np.float32), 5, "fused")
    assert ppo.policies["team"].fused_step_unsupported_reason() == ""
    ppo.rollout()
    _buffer_against_float64(ppo, "team", (32, 64))


# ---------------------------------------------------------------------------------------------------- beside the ICM chain
def test_confined_beside_the_icm_chain_is_bitwise_the_epochs_in_turn(monkeypatch):
    """The abmarl_blind_large_maze form: a 64 / 256 policy with an identity-encoder ICM (O 2, M 128).  The PPO chain on XCDs 0-3
    beside the ICM chain on XCDs 4-7 (two streams) against PPOAF_OVERLAP_ICM=0."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    E, T, B, O, NA = 8, 16, 32, 2, 5
    icm_kw = dict(encoded_obs_dim=0, inverse_hidden_size=128, forward_hidden_size=128, inverse_hidden_depth=2,
                  forward_hidden_depth=2)
    pargs = dict(enable_icm=True, icm_kw_args=icm_kw, actor_kw_args=dict(hidden_size=64), critic_kw_args=dict(hidden_size=256))
    res = []
    for overlap in ("1", "0"):
        monkeypatch.setenv("PPOAF_OVERLAP_ICM", overlap)
        env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=5, term_prob=0.05)
        sp = Box(-np.inf, np.inf, (O,), np.float32)
        ppo = PPO(env_gen, {"p": (None, sp, sp, Discrete(NA), pargs)}, device=dev, random_seed=4, normalize_obs=False,
                  normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=B, epochs_per_iter=2, update_mode="fused")
        pol = ppo.policies["p"]
        assert ppo._fused_updater("p", B) is not None and ppo._fused_icm_updater("p") is not None
        ppo.rollout()
        ppo.train_on_rollout()
        torch.cuda.synchronize()
        assert getattr(ppo._fused_updater("p", B), "xcd_half", 0) == (1 if overlap == "1" else 0), "the PPO chain's XCD half"
        assert getattr(ppo._fused_icm_updater("p"), "xcd_half", 0) == (2 if overlap == "1" else 0)
        res.append((pol.policy_params.detach().clone(), pol.policy_exp_avg.detach().clone(),
                    pol.icm_model.flat_params.detach().clone(), pol.icm_optim.exp_avg.detach().clone()))
    for a, b, what in zip(res[0], res[1], ("policy parameters", "policy exp_avg", "ICM parameters", "ICM exp_avg")):
        assert torch.equal(a, b), f"{what}: overlapped and in turn differ, max |d| {float((a - b).abs().max()):.3e}"


# ---------------------------------------------------------------------------------------------------- two ranks
RANK_TIME_LIMIT = 150.0          # seconds per two-process run, as the suite's other rank helpers get


def _spawn_two_ranks(out_dir, mode):
    s = __import__("socket").socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.spawn(width_pairs_rank.rank_main, args=(2, port, out_dir, mode), nprocs=2, join=False)
    deadline = time.monotonic() + RANK_TIME_LIMIT
    while not ctx.join(timeout=1.0):                    # (raises when a rank failed; the other one is ended with it)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"{mode}: the two ranks did not finish within {RANK_TIME_LIMIT:.0f} s")
    return [torch.load(os.path.join(out_dir, f"{mode}_rank{r}.pt")) for r in range(2)]


def test_two_ranks_peer_exchange_equals_allreduce_path(tmp_path):
    """tests/test_gpu_two_ranks.py::test_peer_exchange_equals_allreduce_path[wide_tail] with a 64-wide actor: its assertions."""
    runs = {}
    for mode in ("peer", "rccl"):
        r0, r1 = runs[mode] = _spawn_two_ranks(str(tmp_path), mode)
        assert r0["peer_exchange"] and all(x == (mode == "peer") for x in r0["peer_exchange"]), r0["peer_exchange"]
        assert torch.equal(r0["w0"], r1["w0"]) and torch.equal(r0["w"], r1["w"]), f"{mode}: replicas identical"
        assert not torch.equal(r0["w"], r0["w0"]) and not torch.equal(r0["obs"], r1["obs"])
        # with K17 the 256-wide critic runs the split-wgrad chain on row pairs and the fused tail with the exchange inside; the
        # all-reduce loop keeps slabs
        assert r0["split"] == [mode == "peer"] and r0["pairs"] == [mode == "peer"], (r0["split"], r0["pairs"])
        assert r0["tail"] == [mode == "peer"], r0["tail"]
    a, b = runs["peer"][0], runs["rccl"][0]
    wtol = dict(rtol=1e-4, atol=2e-5)           # (the split-wgrad chain against the slab chain: the same sums in another association)
    torch.testing.assert_close(a["w"], b["w"], **wtol)
    for k in a["stats"]:
        np.testing.assert_allclose(a["stats"][k], b["stats"][k], err_msg=k, **wtol)
