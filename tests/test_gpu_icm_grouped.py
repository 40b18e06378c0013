"""
-m gpu: the ICM epoch of agent-grouped (MAT) policies on K14 -- one ICM sample per (row, agent) pair (ppo.py:2540-2545,
"case 3"): FusedIcmUpdate drives either chain with B = n A rows read from the epoch's [N, A, .] tables as [N A, .].
MATPolicy with A 3, E 8, T 12, O 18, Discrete(5) and three ICMs: the default (one-width 128), the baselines' shape behind
an encoder (E 128, D 9, M 32) and the identity form (M 32, robot_warehouse's default); batch sizes 16 and 5 -- the latter
gives 15 ICM rows (a partial row tile) and an epoch tail of one grouped row.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

A, E, T, O, NA, SEED = 3, 8, 12, 18, 5, 6
ICMS = {
    "default": {},
    "baseline": dict(encoded_obs_dim=9, encoder_hidden_size=128, inverse_hidden_size=32, forward_hidden_size=32),
    "identity": dict(encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=32),
}
CASES = [(name, B) for name in ICMS for B in (16, 5)]


def _make_ppo(icm, B, mode="fused", shared=False, verbose=False):
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    dev = torch.device("cuda", 0)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    return PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), dict(enable_icm=True, agent_shared_icm=shared, icm_kw_args=dict(ICMS[icm])))},
               device=dev, random_seed=SEED, normalize_obs=False, normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T,
               batch_size=B, epochs_per_iter=1, update_mode=mode, use_graphs=False, verbose=verbose)


def _oracle_icm(icm):
    from oracle import icm_oracle
    from icm_identity import oracle_icm
    if icm == "default":
        return icm_oracle.ICM(O, NA, discrete=True)
    if icm == "baseline":
        return icm_oracle.ICM(O, NA, discrete=True, enc=9, hidden=32, enc_hidden=128)
    return oracle_icm(O, NA, True, 32, 32)


def _check_updater(ppo, icm, B):
    upd = ppo._fused_icm_updater("mat")
    assert upd is not None, "the grouped policy's ICM epoch stayed on the torch path"
    assert upd.A == A and bool(upd.topo.get("general")) == (icm != "default") and bool(upd.topo.get("identity")) == (icm == "identity")
    args = upd._args_for(B) if upd.tables is not None else None
    if args is not None:
        assert (args.B, args.batch_stride, args.n_rows, args.inputs_in_batch_order) == (B * A, B * A, E * T * A, 1)
    assert ppo._overlapped_epochs("mat") is False
    return upd


@pytest.mark.parametrize("icm,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_grouped_icm_epoch_fused_against_the_torch_path(icm, B):
    """The structure and tolerances of the `icm` half of test_fused_mat_and_icm_paths_fuzz_against_the_torch_paths: both
    modes on the same rollout (the torch rollout, whose draws the one-launch sampler's differ from) and the same shuffles."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    res, start = [], None
    for mode in ("fused", "torch"):
        ppo = _make_ppo(icm, B, mode)
        pol = ppo.policies["mat"]
        if start is None:
            start = pol.policy_params.detach().clone(), pol.icm_model.flat_params.detach().clone()
        with torch.no_grad():
            pol.policy_params.copy_(start[0]); pol.icm_model.flat_params.copy_(start[1])
        if mode == "fused":
            _check_updater(ppo, icm, B)
        else:
            assert ppo._fused_icm_updater("mat") is None
        pol.fused_step_unsupported_reason = lambda: "torch rollout forced by the test"
        ppo.rollout()
        loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
        pol.train()
        ppo._icm_batch_train(loader, "mat")
        if mode == "fused":
            upd = _check_updater(ppo, icm, B)
            assert (upd.n_full, upd.tail, upd.n_done) == (E * T // B, E * T % B, -(-E * T // B))
        res.append((pol.icm_model.flat_params.detach().cpu().numpy().copy(), pol.buffer.rewards.cpu().numpy().copy(),
                    ppo.status_dict["mat"]["icm loss"], pol.buffer.actions.cpu().numpy().copy()))
    (w0, r0, l0, a0), (w1, r1, l1, a1) = res
    np.testing.assert_array_equal(a0, a1)
    np.testing.assert_allclose(r0, r1, rtol=3e-5, atol=3e-6)                 # rollout-time intrinsic rewards
    print(f"{icm} B={B}: icm loss {l0!r} against {l1!r}; worst weight deviation {np.abs(w0 - w1).max():.2e}")
    np.testing.assert_allclose(l0, l1, rtol=5e-5)
    np.testing.assert_allclose(w0, w1, rtol=2e-4, atol=3e-5)


@pytest.mark.parametrize("icm,B", CASES, ids=[f"{n}-B{b}" for n, b in CASES])
def test_grouped_icm_epoch_fused_against_the_oracle(icm, B):
    """Against oracle/mat_oracle.CpuMATPPO.icm_train_epoch on the recorded rollout, as test_mat_policy_with_icm_matches_cpu_port
    does (its tolerances), with the oracle's ICM built to the shape under test."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    from oracle import mat_oracle
    ppo = _make_ppo(icm, B)
    pol = ppo.policies["mat"]
    _check_updater(ppo, icm, B)
    cpu = mat_oracle.CpuMATPPO(O, NA, A, batch_size=B, seed=SEED, enable_icm=True, agent_shared_icm=False)
    cpu.icm = _oracle_icm(icm)
    cpu.icm_optim = torch.optim.Adam(cpu.icm.parameters(), lr=3e-4, eps=1e-5)
    cpu.ac.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.actor_critic.state_dict().items()}, strict=False)
    cpu.icm.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    cpu.loader_generator = torch.Generator().manual_seed(SEED)
    ds = ppo.rollout()
    env, buf = ppo.env, pol.buffer
    order = pol.agent_slot_order()
    obs_t = env.obs_table.view(T + 1, A, E, O)[:, order].transpose(1, 2).cpu().numpy()       # [T+1,E,A,O]
    rew_t = env.reward_table.view(T, A, E)[:, order].transpose(1, 2).cpu().numpy()
    k = np.argsort(order)[pol._dataset_slot_order]                 # quirk Q14: dataset slot j <- rollout slot k[j]
    ref = cpu.rollout(obs_t, rew_t, buf.actions[..., 0].cpu().numpy()[:, :, np.argsort(k)], slot_order=order, dataset_slot_of=k)
    np.testing.assert_array_equal(ds.next_observations.cpu().numpy(), ref.next_obs.numpy())
    np.testing.assert_allclose(ds.rewards_to_go.cpu().numpy(), ref.rtg.numpy(), rtol=3e-5, atol=3e-5)
    loader = PermutationLoader(pol.dataset, B, ppo.loader_generator)
    pol.train()
    ppo._icm_batch_train(loader, "mat")
    icm_loss = cpu.icm_train_epoch(agent_idxs=pol.agent_idxs)
    print(f"{icm} B={B}: icm loss {ppo.status_dict['mat']['icm loss']!r} against {icm_loss!r}")
    np.testing.assert_allclose(ppo.status_dict["mat"]["icm loss"], icm_loss, rtol=5e-5)
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in cpu.icm.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=3e-5)
    upd = _check_updater(ppo, icm, B)
    assert int(pol.icm_optim.step_count.item()) == upd.n_done == -(-E * T // B)


def test_agent_shared_icm_keeps_the_torch_path_and_says_why(capfd):
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    ppo = _make_ppo("default", 16, shared=True, verbose=True)
    assert ppo._fused_icm_updater("mat") is None
    out = capfd.readouterr()
    text = out.out + out.err
    assert "torch ICM update path" in text and "agent_shared_icm" in text and "MultiDiscrete" in text, text[-2000:]
    assert FusedIcmUpdate.unsupported_reason(ppo.policies["mat"], 16) != ""
    assert ppo._overlapped_epochs("mat") is False
