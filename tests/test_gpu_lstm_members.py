"""
LSTM members of multi-policy runs (`PPO.lstm_members = True`) on the GPU.

The restriction property (tests/helpers/lstm_members.py): every member of the mixed run logs and then learns bit for bit
what it does alone on the env restricted to its agents.  Under update_mode="fused" each case runs with the block form of
K21 (the default), with `PPO.step_row_blocks = False` (K21 on gathered rows) and with `PPO.finish_rows = False` (the torch
statements instead of K23, so the `cut` flag of the LSTM critic's extra step is formed the other way); the three agree
bit for bit with each other as well.  Launch counters and the policies' launch state show that K21 and K22 really ran.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FUSED_CASES = ["lstm+mat", "lstm02+ff", "lstm32+lstm64", "tensor lstm+ff"]
VARIANTS = {"blocks": {}, "gathered": dict(step_row_blocks=False), "torch_finish": dict(finish_rows=False)}
_RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)


def _switches(flags):
    def prepare(ppo):
        for k, v in flags.items():
            setattr(ppo, k, v)
    return prepare


def _lstm_ids(ppo):
    return [pid for pid, pol in ppo.policies.items() if pol.using_lstm]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", FUSED_CASES)
def test_every_member_equals_itself_alone_fused(name, variant):
    import lstm_members as L
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    before = FusedLstmUpdate.launches
    ppo, rec = L.assert_member_equals_alone(name, DEV, "fused", _switches(VARIANTS[variant]))
    _RECORDS[(name, variant)] = rec
    assert FusedLstmUpdate.launches > before, "K22 did not run"
    for pid in _lstm_ids(ppo):
        pol = ppo.policies[pid]
        assert pol.lstm_step_unsupported_reason() == "" and getattr(pol, "_lstm_step_state", None) is not None, "K21 did not run"
        # the block form ran exactly where it is switched on
        assert (getattr(pol, "_lstm_blocks_table", None) is not None) == (variant != "gathered"), (pid, variant)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_the_three_step_forms_agree_bitwise(name):
    import lstm_members as L
    recs = [_RECORDS.get((name, v)) for v in sorted(VARIANTS)]
    if any(r is None for r in recs):                       # run alone: compute what the test above would have left
        recs = [L.run_case(name, DEV, "fused", _switches(VARIANTS[v]))[3] for v in sorted(VARIANTS)]
    first = recs[0]
    for other in recs[1:]:
        for pid in first["snaps"]:
            L.same_tensors(other["snaps"][pid], first["snaps"][pid], f"{name} {pid}")
            L.same_tensors(other["end"][pid], first["end"][pid], f"{name} {pid} weights")
        for pid in first["hidden"]:
            L.same_tensors(other["hidden"][pid], first["hidden"][pid], f"{name} {pid} hidden")


def test_the_lstm_member_on_the_torch_route_auto():
    """update_mode="auto": the LSTM member keeps nn.LSTM and the pending / write_step / store_hidden_states route."""
    import lstm_members as L
    ppo, _ = L.assert_member_equals_alone("lstm02+ff", DEV, "auto")
    pol = ppo.policies["pair"]
    assert "use_hip is not set" in pol.lstm_step_unsupported_reason() and getattr(pol, "_lstm_step_state", None) is None


def test_an_lstm_member_with_an_icm_keeps_its_torch_route_under_fused():
    import lstm_members as L
    ppo, rec = L.assert_member_equals_alone("lstm_icm+mat", DEV, "fused")
    pol = ppo.policies["adversary"]
    assert "ICM" in pol.lstm_step_unsupported_reason() and getattr(pol, "_lstm_step_state", None) is None
    assert rec["snaps"]["adversary"]["next_observations"] is not None


def test_the_opt_in_off_still_refuses():
    import lstm_members as L
    ppo, _, _ = L.mixed_run("lstm+mat", DEV, "fused")
    ppo.lstm_members = False
    with pytest.raises(NotImplementedError, match="LSTM policies are not supported"):
        ppo.rollout()


def test_lstm_inside_a_mat_policy_stays_refused():
    import lstm_members as L
    import mixed_policies as M
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.ppo import PPO
    env_gen = lambda: SyntheticMixedAgentsEnv(M.E, M.SPECS, M.T, DEV, reward="uniform", seed=33)
    settings = {"adversary": (None, M.box(8), M.box(8), M.SPECS[0][2], {}),
                "team": (M.MATPolicy, M.box(10), M.box(10), M.SPECS[1][2], L.lstm())}
    assert PPO.lstm_members is False
    with pytest.raises(Exception, match="(?i)lstm"):
        ppo = M.make_ppo(env_gen, settings, lambda a: "adversary" if a.startswith("adversary") else "team", DEV, "fused")
        ppo.lstm_members = True
        ppo.rollout()


def test_verbose_names_the_step_form(capsys):
    import lstm_members as L
    for flags, needle in (({}, "LSTM policy adversary steps on K21 on the env's row blocks"),
                          (dict(step_row_blocks=False), "LSTM policy adversary steps on K21 on gathered rows")):
        ppo, _, _ = L.mixed_run("lstm+mat", DEV, "fused", _switches(flags), verbose=True)
        ppo.rollout()
        assert needle in capsys.readouterr().out
    ppo, _, _ = L.mixed_run("lstm_icm+mat", DEV, "fused", verbose=True)
    ppo.rollout()
    out = capsys.readouterr().out
    assert "LSTM policy adversary steps on the torch route (" in out and "ICM" in out


def test_no_gather_and_no_index_put_between_env_steps():
    """{LSTM, MAT} on the block forms: between two env.step calls the only torch operators that are not pure views are
    the four that form the device flag `cut` from the end_kind row K23 wrote (eq, any, any of `truncated`, or) -- no cat /
    index gather of the LSTM member's observations, no index_put of its actions."""
    import lstm_members as L
    import mixed_policies as M
    ppo, _, _ = L.mixed_run("lstm+mat", DEV, "fused")
    ppo.rollout()                                           # buffers, tables and launch arguments exist
    segments = M.ops_between_env_steps(ppo)
    assert len(segments) == M.T - 1
    # cut = (end_kind[t] == 2).any() | truncated.any(): the flag of the LSTM critic's extra step, kept on the device
    cut_flag = ["aten.eq.Scalar", "aten.any.default", "aten.any.default", "aten.bitwise_or.Tensor"]
    allowed = set(cut_flag)
    print("between two env steps:", M.launching(segments[0]))
    for t, ops in enumerate(segments):
        assert M.launching(ops) == cut_flag, f"after env step {t}: {M.launching(ops)}"
    # the same run with the gathers has them: the enumeration sees what it should
    ppo, _, _ = L.mixed_run("lstm+mat", DEV, "fused", _switches(dict(step_row_blocks=False)))
    ppo.rollout()
    seen = {o for ops in M.ops_between_env_steps(ppo) for o in M.launching(ops)}
    assert seen - allowed, seen


def test_evaluation_scores_equal_the_member_alone():
    """test_policy on {LSTM, MAT}: the LSTM member's scores are those it gets alone on its restricted env, and the
    training hidden states are left as they were found.  term_prob = 0.3: every env of the seeded table terminates
    within its 16 steps, so each of the six quotas is met (at 0.05 three of the first six envs never end and the
    evaluation would not either); max_steps turns any such loop into an error."""
    import lstm_members as L
    import mixed_policies as M
    from ppo_and_friends_amd.testing import test_policy as run_test_policy
    ppo, specs, members, rec = L.run_case("lstm+mat", DEV, "fused", term_prob=0.3)
    assert M.raw_env(ppo.env).term_table.any(0).all()
    pol = ppo.policies["adversary"]
    kept = [(net, net.hidden_state, tuple(x.clone() for x in net.hidden_state)) for net in (pol.actor, pol.critic)]
    mixed = run_test_policy(ppo, 6, deterministic=True, max_steps=400)
    for net, state, values in kept:
        assert net.hidden_state is state and all(torch.equal(a, b) for a, b in zip(net.hidden_state, values))
    alone = L.run_alone(ppo, rec, "adversary", members, DEV, "fused")["ppo"]
    with torch.no_grad():                                   # the weights the mixed run evaluated with
        for k, v in M.weights(alone.policies["adversary"]).items():
            v.copy_(M.weights(pol)[k])
    want = run_test_policy(alone, 6, deterministic=True, max_steps=400)
    assert mixed["adversary_0"] == want["adversary_0"], (mixed["adversary_0"], want["adversary_0"])
    assert mixed["adversary"] == want["adversary"]
    assert mixed["num_test_runs"] == want["num_test_runs"] == 6
