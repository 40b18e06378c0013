"""
-m gpu: multi-policy runs with MATPolicy teams and ICM members.

The restriction property (tests/helpers/mixed_policies.py): each member of a mixed run logs and learns bitwise what it
does alone in `PPO.rollout` on an env restricted to its agents -- rollout buffer, bootstrap tables, advantages,
rewards-to-go, parameters, Adam moments, status entries and the episode count -- on the torch path and on the fused
path.  Also the dense end table an ICM member forces on every member, `get_inference_actions` for a grouped
member of a multi-policy env, and `test_policy` on a mixed env with a MAT member against the numpy restatement.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SETS = ["ppo+mat", "ppo+mat split", "ppo_icm+mat", "ppo+mat_icm", "ppo+mat_shared_icm", "mat+mat"]


def _prepare(ppo):
    """Under `fused` an agent-shared ICM runs on K14 (the opt-in of a single-policy run)."""
    for pol in ppo.policies.values():
        if pol.enable_icm and getattr(pol, "agent_shared_icm", False):
            pol.fused_shared_icm = True


@pytest.mark.parametrize("mode", ["torch", "fused"])
@pytest.mark.parametrize("name", SETS)
def test_every_member_of_a_mixed_run_equals_the_member_alone(name, mode):
    import mixed_policies as M
    ppo, rec = M.assert_member_equals_alone(name, DEV, mode, _prepare if mode == "fused" else None)
    # the ends of the tables occur: terminal ends, ends at max_ts_per_ep and the last row
    kinds = {pid: s["end_kind"] for pid, s in rec["snaps"].items()}
    for pid, ek in kinds.items():
        assert set(ek.unique().tolist()) == {0, 1, 2}, pid
        assert tuple(ek.shape) == ((M.T, M.E) if ppo.policies[pid].agent_grouping else (M.T, M.E * len(ppo.policies[pid].agent_ids)))
    for pid, pol in ppo.policies.items():
        assert (rec["snaps"][pid]["next_observations"] is not None) == bool(pol.enable_icm)
        assert (rec["snaps"][pid]["boot_stats"] is not None) == bool(pol.enable_icm)


def test_a_torch_path_member_beside_a_fused_team():
    """Under "auto" the 256 / 512 adversary steps and learns on the torch path, the MAT team on K16 / K15, in one run; each
    equals itself alone."""
    import mixed_policies as M
    ppo, rec = M.assert_member_equals_alone("ppo_wide+mat", DEV, "auto")
    assert ppo.policies["adversary"].fused_step_unsupported_reason() != ""
    assert ppo.policies["team"].fused_step_unsupported_reason() == ""


def test_an_icm_member_turns_the_dense_end_table_on_for_every_member():
    """No terminations and episodes longer than the rollout: only the ICM makes the ends dense, and for both members."""
    import mixed_policies as M
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    specs, members = M.member_sets()["ppo_icm+mat"]
    env_gen = lambda: SyntheticMixedAgentsEnv(M.E, specs, M.T, DEV, reward="uniform", seed=33)
    mapping = lambda a: "adversary" if a.startswith("adversary") else "team"
    for icm in (True, False):
        m = dict(members) if icm else M.member_sets()["ppo+mat"][1]
        ppo = M.make_ppo(env_gen, M.settings_of(specs, m), mapping, DEV, "torch", max_ts_per_ep=200)
        ppo.rollout()
        for pol in ppo.policies.values():
            assert pol.buffer.fixed_length == (not icm)
            assert bool((pol.buffer.end_kind[-1] == 2).all())


@pytest.mark.parametrize("name", ["ppo+mat", "ppo+mat split"])
def test_inference_actions_hand_a_grouped_member_its_slot_order(name):
    """The dict env's per-agent actions of the team are the MAT decode of [E, A, .] in the team's slot order."""
    import mixed_policies as M
    ppo, specs, _ = M.mixed_run(name, DEV, "torch")
    team = ppo.policies["team"]
    np.random.seed(3)
    while np.array_equal(team.agent_slot_order(), np.arange(2)):
        team.shuffle_agent_ids()
    obs, cobs = ppo.env.reset()
    acts = ppo.get_inference_actions(obs, True, critic_obs=cobs)
    assert set(acts) == {a for a, _, _ in specs}
    grouped = torch.stack([obs[a] for a in team.agent_ids], 1)                 # slot order
    want = team.get_inference_actions(grouped, True)
    for s, a in enumerate(team.agent_ids):
        assert torch.equal(acts[a].reshape(M.E, -1), want[:, s].reshape(M.E, -1)), a
    want_adv = ppo.policies["adversary"].get_inference_actions(obs["adversary_0"], True)
    assert torch.equal(acts["adversary_0"], want_adv)


@pytest.mark.parametrize("specs_name", ["ppo+mat", "ppo+mat split"])
def test_test_policy_on_a_mixed_env_with_a_mat_member_equals_the_restatement(specs_name):
    """`test_policy` over the dict env: the MAT team decodes in its slot order, deterministic and sampled; the scores
    are the numpy restatement's of the traced env (as test_two_policies_in_a_dict_env_through_the_books)."""
    import eval_restatement as R
    import mixed_policies as M
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.testing import test_policy
    specs, members = M.member_sets()[specs_name]
    N = 25

    class Traced(SyntheticMixedAgentsEnv):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.term_table[-1] = True                       # every row finishes once per horizon
            self.trace = []

        def step(self, action):
            out = super().step(action)
            self.trace.append((out[2], out[3], out[4]))
            return out
    env_gen = lambda: Traced(M.E, specs, 40, DEV, reward="uniform", seed=33, term_prob=0.07)
    mapping = lambda a: "adversary" if a.startswith("adversary") else "team"
    ppo = M.make_ppo(env_gen, M.settings_of(specs, members), mapping, DEV, "auto")
    team = ppo.policies["team"]
    np.random.seed(3)
    while np.array_equal(team.agent_slot_order(), np.arange(2)):
        team.shuffle_agent_ids()
    raw = M.raw_env(ppo.env)
    agents = [a for a, _, _ in specs]
    for deterministic in (True, False):
        raw.trace = []
        info = test_policy(ppo, N, deterministic=deterministic, check_every=7, max_steps=4000)
        score = {a: np.stack([r[a].cpu().numpy() for r, _, _ in raw.trace]) for a in agents}
        done = np.stack([(t[agents[0]] | u[agents[0]]).cpu().numpy() for _, t, u in raw.trace])
        assert info == R.score_info(score, done, {a: mapping(a) for a in agents}, N)
        assert set(info) == {"num_test_runs", "total_time_steps", *agents, "adversary", "team"}


@pytest.mark.parametrize("name", ["ppo+mat", "ppo+mat_shared_icm"])
def test_library_calls_per_env_step_of_a_fused_mixed_rollout(name, monkeypatch):
    """Between two env.step calls the fused mixed rollout makes exactly one library step call per member (K6+K7's block
    form for the PPOPolicy, K16's for the MATPolicy) and ONE finish call (K23) for all of them; with `finish_rows` and
    `step_row_blocks` off, the gathered K6+K7 and regrouped K16 steps and no finish call."""
    import mixed_policies as M
    from ppo_and_friends_amd import _lib, kernels as K
    ppo, specs, _ = M.mixed_run(name, DEV, "fused", _prepare)
    calls = []
    lib = _lib.load()

    class Counting:
        def __getattr__(self, fn):
            inner = getattr(lib, fn)
            if fn in ("ppoaf_policy_step", "ppoaf_policy_step_blocks", "ppoaf_mat_policy_step", "ppoaf_mat_policy_step_blocks",
                      "ppoaf_rollout_finish_rows"):
                return lambda *a: (calls.append(fn), inner(*a))[1]
            return inner
    monkeypatch.setattr(_lib, "load", lambda: Counting())
    raw = M.raw_env(ppo.env)
    inner_step = raw.step
    raw.step = lambda action: (calls.append("env.step"), inner_step(action))[1]
    ppo.rollout()
    per_step = ["ppoaf_policy_step_blocks", "ppoaf_mat_policy_step_blocks", "env.step", "ppoaf_rollout_finish_rows"]
    assert calls == per_step * M.T
    calls.clear()
    monkeypatch.setattr(type(ppo), "finish_rows", False)
    monkeypatch.setattr(type(ppo), "step_row_blocks", False)
    ppo.rollout()
    assert calls == ["ppoaf_policy_step", "ppoaf_mat_policy_step", "env.step"] * M.T


@pytest.mark.parametrize("name", ["ppo+mat_icm", "ppo_icm+mat", "ppo+mat fixed-length"])
def test_the_block_routes_against_the_torch_operators_they_replace(name):
    """The attributes that keep the gather path: the same fused mixed rollout with `finish_rows` and `step_row_blocks` on
    and off, bitwise.  `fixed-length`: no terminations and episodes longer than the rollout, so no end is written before
    the last row (K23 without end tables against the torch statements that skip theirs)."""
    import mixed_policies as M
    name, _, fixed_length = name.partition(" fixed-length")
    kw = dict(term_prob=0.0, max_ts_per_ep=200) if fixed_length else {}
    snaps = []
    for on in (True, False):
        ppo, specs, _ = M.mixed_run(name, DEV, "fused", _prepare, **kw)
        ppo.finish_rows = ppo.step_row_blocks = on
        ppo.replay_raw_actions = M.replay_actions(ppo, specs)
        np.random.seed(11)
        ppo.rollout()
        snaps.append({pid: M.snapshot(ppo, pid) for pid in ppo.policies})
    for pid in snaps[0]:
        for k, want in snaps[1][pid].items():
            got = snaps[0][pid][k]
            assert (got is None) == (want is None) and (want is None or torch.equal(got, want)), f"{pid} {k}"


# what an agent-shared ICM on K14 adds between two env.step calls, besides its own library launches: the joins of the team's
# previous / next observation and action rows into one ICM row per env, the spread of the shared reward over the agents
# into the buffer's [E, A] layout, and the next-observation rows the ICM update reads
ICM_OPERATORS = (
    ["aten.cat.default"]                                                      # the team's next observation rows, agent-major
    + ["aten.transpose.int", "aten.clone.default"] * 3                        # joined per env: previous obs, next obs, actions
    + ["aten.empty.memory_format"]                                            # the reward row K14 writes
    + ["aten.repeat.default"]                                                 # one shared reward per env -> each of its agents
    + ["aten.index.Tensor", "aten.transpose.int", "aten.clone.default", "aten.copy_.default"]   # -> [E, A] slot order, kept
    + ["aten.cat.default", "aten.index.Tensor", "aten.transpose.int", "aten.clone.default",
       "aten.copy_.default"]                                                  # next observations -> buffer, [E, A] slot order
    + ["aten.cat.default", "aten.cat.default"])                               # before the next step: previous obs and actions


def test_no_torch_operator_between_env_steps_of_a_fused_ppo_mat_rollout():
    """{PPO, MAT} on the block routes: between two env.step calls the package issues its three library launches and NO
    torch operator on a device tensor (pure views aside: they launch and copy nothing)."""
    import mixed_policies as M
    ppo, specs, _ = M.mixed_run("ppo+mat", DEV, "fused", _prepare)
    ppo.rollout()                                                        # buffers and launch arguments exist
    segments = M.ops_between_env_steps(ppo)
    assert len(segments) == M.T - 1
    for t, ops in enumerate(segments):
        assert M.launching(ops) == [], f"after env step {t}: {M.launching(ops)}"
    # the comparison path does issue them: the count is not vacuous
    ppo.finish_rows = ppo.step_row_blocks = False
    assert all(len(M.launching(ops)) > 10 for ops in M.ops_between_env_steps(ppo))


def test_operators_between_env_steps_with_an_agent_shared_icm():
    """{PPO, MAT + agent_shared_icm on K14}: the PPO member and the step / finish launches add nothing; what remains is the
    enumerated list of the ICM reward's own operators, the same after every env step."""
    import mixed_policies as M
    ppo, specs, _ = M.mixed_run("ppo+mat_shared_icm", DEV, "fused", _prepare)
    ppo.rollout()
    segments = [M.launching(ops) for ops in M.ops_between_env_steps(ppo)]
    assert all(ops == segments[0] for ops in segments)
    assert segments[0] == ICM_OPERATORS
