"""
-m gpu: ICMs over Discrete(18) and Box(17) actions -- mario_bros_ram's widths (E 128, D 9, M 32 / 32) and the default ICM
(128 everywhere) -- with the opt-in `PPOPolicy.fused_wide_icm_actions`, through PPO on SyntheticFixedLengthEnv (8 envs,
T 12, B 32): the update epoch runs on FusedIcmUpdate over the shapes chain's wide-action form, the rollout-time reward on
its reward kernel.  Against this package's torch path (rollout rewards), against oracle/icm_oracle.py over two epochs on the
same mini-batches (the tolerances of tests/test_gpu_icm_shapes.py for the same comparisons), bitwise from run to run; a
Discrete(5) ICM is bitwise what it is without the opt-in, and without it the Discrete(18) ICM is on the torch path with
the reason it had.
"""
import numpy as np
import pytest
import torch

import test_gpu_icm_shapes as S

pytestmark = pytest.mark.gpu

MARIO = dict(E=128, D=9, Mi=32, Mf=32)
DEFAULT = dict(E=128, D=128, Mi=128, Mf=128)
CASES = [dict(kind="d", NA=18, O=20, envs=8, T=12, B=32, **MARIO), dict(kind="c", NA=17, O=20, envs=8, T=12, B=32, **MARIO),
         dict(kind="d", NA=18, O=20, envs=8, T=12, B=32, **DEFAULT), dict(kind="c", NA=17, O=20, envs=8, T=12, B=32, **DEFAULT)]
IDS = ["disc18-mario", "box17-mario", "disc18-default128", "box17-default128"]


def _ppo(case, wide=True, mode="auto", **kw):
    """update_mode "auto": the policy's own 18-output actor is not this file's subject (it stays where it is today)."""
    ppo = S._make_ppo(case, mode, **kw)
    if wide:
        ppo.policies["p"].fused_wide_icm_actions = True          # by hand, before the first rollout
    return ppo


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_epochs_match_the_oracle_and_the_reward_kernel_runs(case):
    from oracle import icm_oracle
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    dev = torch.device("cuda", 0)
    envs, T, O, NA, B, D = (case[k] for k in ("envs", "T", "O", "NA", "B", "D"))
    ppo = _ppo(case)
    pol = ppo.policies["p"]
    assert FusedIcmUpdate.unsupported_reason(pol, B) == ""
    ref = icm_oracle.ICM(O, NA, discrete=case["kind"] == "d", enc=D, hidden=case["Mi"], enc_hidden=case["E"], inv_depth=2, fwd_depth=2)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.icm_model.state_dict().items()})
    opt = torch.optim.Adam(ref.parameters(), lr=3e-4, eps=1e-5)
    calls = PPOPolicy.fused_icm_reward_calls
    ppo.rollout()
    assert PPOPolicy.fused_icm_reward_calls >= calls + T and pol.fused_icm_reward, "the rollout rewards did not come from K14"
    fused = ppo._fused_icm_updater("p")
    assert isinstance(fused, FusedIcmUpdate) and fused.topo["general"] and fused.topo["n_action_slices"] == _lib.ICM_WIDE_ACTIONS
    buf = pol.buffer
    N = envs * T
    rm = buf.row_map.cpu().long()
    flat = lambda t: t.reshape((N,) + tuple(t.shape[2:])).cpu()[rm]
    obs, nxt, act = flat(buf.observations), flat(buf.next_observations), flat(buf.actions)
    g = torch.Generator().manual_seed(9)
    for epoch in range(2):
        perm = torch.randperm(N, generator=g)
        fused.begin_epoch(perm.to(dev))
        fused.run_epoch()
        t = fused.end_epoch()
        tot, cnt = 0.0, 0
        for o in range(0, N, B):
            idx = perm[o:o + B]
            _, inv_loss, f_loss = ref(obs[idx], nxt[idx], act[idx])
            loss = (1.0 - pol.icm_beta) * f_loss + pol.icm_beta * inv_loss
            opt.zero_grad(); loss.backward(); opt.step()
            tot += float(loss.detach()); cnt += 1
        assert t[1] == cnt
        np.testing.assert_allclose(t[0] / cnt, tot / cnt, rtol=2e-5, err_msg=f"icm loss, epoch {epoch}")
    w = torch.cat([p.detach().cpu().reshape(-1) for p in pol.icm_model.parameters()]).numpy()
    w_ref = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).numpy()
    np.testing.assert_allclose(w, w_ref, rtol=1e-4, atol=2e-5)
    assert int(pol.icm_optim.step_count.item()) == 2 * cnt


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rollout_rewards_match_the_torch_path(case):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    dev = torch.device("cuda", 0)
    pol = _ppo(case).policies["p"]
    n, O, NA = 37, case["O"], case["NA"]                       # two row tiles + one of 5 rows
    gen = torch.Generator().manual_seed(3)
    o1, o2 = torch.randn(n, O, generator=gen).to(dev), torch.randn(n, O, generator=gen).to(dev)
    if case["kind"] == "d":
        act = torch.randint(0, NA, (n, 1), generator=gen)
        act[:NA, 0] = torch.arange(NA)                         # every class
        act = act.to(dev)
    else:
        act = torch.rand(n, NA, generator=gen).to(dev) * 2 - 1
    calls = PPOPolicy.fused_icm_reward_calls
    pol.fused_icm_reward = True
    fused = pol.get_intrinsic_reward(o1, o2, act)
    assert PPOPolicy.fused_icm_reward_calls == calls + 1 and pol.fused_icm_reward, "the fused path was not the one taken"
    pol.fused_icm_reward = False
    plain = pol.get_intrinsic_reward(o1, o2, act)
    assert PPOPolicy.fused_icm_reward_calls == calls + 1
    assert fused.shape == plain.shape == (n,)
    np.testing.assert_allclose(fused.cpu().numpy(), plain.cpu().numpy(), rtol=3e-5, atol=3e-6)


def _one_iteration(case, wide):
    """Rollout (rewards) + one ICM epoch through PPO's own loop -> (rewards, parameters, moments, loss, the updater)."""
    from ppo_and_friends_amd.ppo import PermutationLoader
    ppo = _ppo(case, wide)
    pol = ppo.policies["p"]
    ppo.rollout()
    ppo._icm_batch_train(PermutationLoader(pol.dataset, case["B"], ppo.loader_generator), "p")
    torch.cuda.synchronize()
    opt = pol.icm_optim
    return ([pol.buffer.rewards.clone(), pol.icm_model.flat_params.detach().clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(),
             torch.as_tensor(ppo.status_dict["p"]["icm loss"])], ppo._fused_icm_updater("p"))


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_bitwise_from_run_to_run(case):
    (a, upd), (b, _) = _one_iteration(case, True), _one_iteration(case, True)
    assert upd is not None and upd.topo["general"]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("widths", [MARIO, DEFAULT], ids=["mario", "default128"])
def test_a_discrete_5_icm_is_bitwise_what_it_is_without_the_opt_in(widths):
    case = dict(kind="d", NA=5, O=20, envs=8, T=12, B=32, **widths)
    (on, upd_on), (off, upd_off) = _one_iteration(case, True), _one_iteration(case, False)
    assert upd_on is not None and upd_off is not None and upd_on.topo == upd_off.topo and "n_action_slices" not in upd_on.topo
    for x, y in zip(on, off):
        assert torch.equal(x, y)


def test_without_the_opt_in_the_icm_is_on_the_torch_path_with_its_reason(capsys):
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    ppo = _ppo(CASES[0], wide=False)
    pol = ppo.policies["p"]
    assert pol.fused_wide_icm_actions is False
    assert FusedIcmUpdate.unsupported_reason(pol, 32) == "action widths (18, 18) must be in [1, 8]"
    calls = PPOPolicy.fused_icm_reward_calls
    ppo.rollout()
    assert PPOPolicy.fused_icm_reward_calls == calls and not pol.fused_icm_reward
    ppo.verbose = True
    capsys.readouterr()
    assert ppo._fused_icm_updater("p") is None
    said = capsys.readouterr().out
    assert "torch ICM update path (action widths (18, 18) must be in [1, 8])" in said
    assert "PPOPolicy.fused_wide_icm_actions = True would take it on the fused kernels" in said
