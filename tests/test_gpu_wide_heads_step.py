"""
-m gpu: K6+K7 and K19 for the wide heads of the wide width pair (256, 512) -- 9 .. 24 actor outputs, Categorical and
tanh-Gaussian (csrc/policy_wide_heads.hip) -- one launch against float64 and the restated Philox draws, judged by
policy_step_cases.judge with its per-element bounds and its near-tie rule, through the Device of
tests/test_gpu_policy_step_float64.py (sentinels around every output, inputs unchanged, the launch with and without the
observation copies).  The cases: tests/helpers/wide_heads_cases.py.

Near ties: with these seeds the float64 reference alone leaves out no row of any sampled case (computed without a device; the
cap is mat_step_cases.cap(E) = 2 at these E).  Measured on one MI355X (23 passed in 3.9 s), worst deviation over bound:
logp 0.245 (gau24_floor_e17_d3_in8 sampled), action 0.105 (gau16_e17_d3_in8 sampled), raw 0.037, value 0.129; Categorical
logp 0.060 (cat24_sat_e17_d3_in8 sampled); no compared action differs; the block form at E 32 is bitwise the plain form.

The block form: E 32 as two aligned blocks, bitwise the plain form; a misaligned base refused by the library by name; and in
PPO.rollout a wide-head member whose block leaves the 16-byte boundary at step 1 -- it falls back to gathered rows, `verbose`
says why once, and the rollout is bitwise the run without row blocks.

K19: the deterministic action against head_draws.greedy with an exact tie planted between classes 3 and 20 (the lower index
wins), and the sampled action bitwise K6's action_out for equal (obs, params, seed, offset).
"""
import numpy as np
import pytest
import torch

import test_gpu_policy_step_float64 as k6
import wide_heads_cases as wh

cases, ek = k6.cases, k6.ek
pytestmark = pytest.mark.gpu


class Device(k6.Device):
    """k6.Device on a case of wide_heads_cases."""

    def __init__(self, name):
        from ppo_and_friends_amd import _lib, kernels as K
        self.name, self.s = name, wh.steering(name)
        s, c = self.s, self.s.c
        self._lib, self.lib, self.K = _lib, _lib.load(), K
        dev = self.dev = torch.device("cuda", 0)
        self.E, self.O, self.head = c["E"], c["O"], s.head
        self.pol = ek.Policy(0, c["Ia"], c["Ha"], c["Da"], self.O, s.head, c["act"], s.slices, s.bounds, nets=(s.actor, s.critic))
        assert np.array_equal(self.pol.params.cpu().numpy(), s.params())
        self.obs = torch.from_numpy(s.obs).to(dev).contiguous()
        self.cobs = torch.from_numpy(s.cobs).to(dev).contiguous()
        self.vn = None
        if s.vn is not None:
            self.vn = tuple(torch.tensor([x], dtype=torch.float32, device=dev) for x in s.vn)
        self.adt = torch.float32 if s.head == wh.GAU else torch.int64
        self.aw = 1 if s.head == wh.CAT else self.O


@pytest.mark.parametrize("name", list(wh.CASES))
def test_k6_sampled_launch_against_float64(name):
    d = Device(name)
    res = d.both()
    d.judged(d.got(res), "sampled")
    if d.head == wh.CAT:
        assert int(res["act"].min()) >= 0 and int(res["act"].max()) < d.O


@pytest.mark.parametrize("name", list(wh.CASES))
def test_k6_forced_launch_against_float64(name):
    d = Device(name)
    s = d.s
    res = d.both(s.forced)
    g = d.got(res)
    d.judged(g, "forced")
    f64, f32 = s.ref["forced"]
    if d.head == wh.CAT:
        assert np.array_equal(g["raw"], np.clip(s.forced, 0, d.O - 1))
    else:
        assert np.array_equal(res["raw"].cpu().numpy(), np.asarray(s.forced, np.float32).reshape(d.E, d.O))   # bitwise
    bound = cases.k12_bound(f64["logp"], f32["logp"])
    for regime, rows in s.marked.items():
        rows = rows if rows.ndim == 1 else rows.any(1)
        if regime == "saturated" and not rows.any():
            continue
        assert rows.any() and (np.abs(g["logp"] - f64["logp"])[rows] <= bound[rows]).all(), regime


def _table(d, n_blocks, rows, shift=0):
    """The block table of a launch: the case's rows as n_blocks blocks of `rows` rows, each in a tensor of its own (shift: the
    first observation block starts `shift` floats into its tensor)."""
    tb = d._lib.StepBlocks()
    tb.n_blocks, tb.rows_per_block = n_blocks, rows
    keep, acts = [], []
    for b in range(n_blocks):
        o = torch.zeros(rows * d.s.c["Ia"] + 4, device=d.dev)
        off = shift if b == 0 else 0
        o[off:off + rows * d.s.c["Ia"]] = d.obs[b * rows:(b + 1) * rows].reshape(-1)
        co = d.cobs[b * rows:(b + 1) * rows].clone().contiguous()
        ea = torch.full((rows, d.aw), -5.0, device=d.dev).to(d.adt)
        keep += [o, co]
        acts.append(ea)
        tb.obs[b], tb.critic_obs[b], tb.env_action[b] = o.data_ptr() + 4 * off, co.data_ptr(), ea.data_ptr()
    return tb, keep, acts


def test_block_form_is_the_plain_form_and_fills_the_env_action_blocks():
    """E 32 as 2 blocks of 16 rows of Box(17): every output bitwise the plain launch's, each block's env action tensor the 17
    floats of its rows' action_out."""
    d = Device("block")
    plain = d.launch()
    tb, keep, acts = _table(d, 2, 16)
    blk = d.launch(table=tb)
    for k in k6.OUTPUTS:
        assert torch.equal(k6._bits(blk[k]), k6._bits(plain[k])), k
    for b, ea in enumerate(acts):
        assert ea.shape == (16, 17) and torch.equal(k6._bits(ea), k6._bits(plain["act"][16 * b:16 * (b + 1)])), b
    d.judged(d.got(blk), "sampled")


def test_a_misaligned_block_is_refused_by_name():
    """The library refuses a block base that is not 16-byte aligned before it launches anything (the policy's own check,
    step_blocks_unsupported_reason, says the same words to `verbose` and the member gathers its rows with torch operators)."""
    d = Device("block")
    tb, keep, acts = _table(d, 2, 16, shift=1)
    T, hold = d.outputs(), []
    a = d.args(T, None, True, hold)
    a.obs = a.critic_obs = None
    with pytest.raises(d._lib.PpoafError, match="16-byte aligned"):
        d.K.policy_step_blocks(a, tb)
    torch.cuda.synchronize()


def _member_run(blocks, verbose=False):
    """A two-policy run (tests/helpers/mixed_policies.py: make_ppo) whose member `team` is a 256 / 512 Box(17) policy of two
    agents at 86 observations and 5 envs: the env hands each agent's rows as step t of a [T + 1, 5, 86] table, 1720 bytes per
    step, so the member's observation blocks start on a 16-byte boundary at even steps only."""
    import mixed_policies as mp
    from ppo_and_friends_amd.environments.synthetic import SyntheticMixedAgentsEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    E, T = 5, 8
    space = Box(-0.4, 0.4, (17,), np.float32)
    specs = [("solo_0", 8, Discrete(3)), ("team_0", 86, space), ("team_1", 86, space)]
    env_gen = lambda: SyntheticMixedAgentsEnv(E, specs, T, "cuda", reward="uniform", seed=33, term_prob=0.05)
    wide = dict(actor_kw_args=dict(hidden_size=256), critic_kw_args=dict(hidden_size=512))
    settings = {"solo": (None, mp.box(8), mp.box(8), Discrete(3), {}), "team": (None, mp.box(86), mp.box(86), space, wide)}
    ppo = mp.make_ppo(env_gen, settings, lambda a: a.split("_")[0], torch.device("cuda", 0), "fused", envs_per_proc=E,
                      ts_per_rollout=T, batch_size=16, verbose=verbose)
    ppo.step_row_blocks = blocks
    return ppo, mp


def test_a_member_with_a_misaligned_block_falls_back_and_verbose_says_so(monkeypatch, capsys):
    """PPO.rollout with a wide-head member: step 0 runs the block form (ppoaf_policy_step_blocks' wide-head kernel), at step 1
    the member's observation block lies 8 bytes off a 16-byte boundary, PPOPolicy.step_blocks_unsupported_reason says so, the
    member gathers its rows with torch operators from there on and `verbose` prints the reason once; the rollout's buffer
    and dataset are bitwise those of the run with step_row_blocks off (the plain form at every step)."""
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)
    calls = {"blocks": [], "plain": []}
    inner_b, inner_p = K.policy_step_blocks, K.policy_step
    monkeypatch.setattr(K, "policy_step_blocks", lambda a, tb: (calls["blocks"].append(int(a.actor.out_dim)), inner_b(a, tb))[1])
    monkeypatch.setattr(K, "policy_step", lambda a: (calls["plain"].append(int(a.actor.out_dim)), inner_p(a))[1])
    ppo, mp = _member_run(True, verbose=True)
    team = ppo.policies["team"]
    assert team.fused_step_unsupported_reason() == ""
    capsys.readouterr()
    ppo.rollout()
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    said = "rollout: policy team gathers its rows with torch operators (observation block 0 does not start on a 16-byte boundary)"
    assert out.count(said) == 1, out
    assert "policy solo gathers" not in out
    # the member: one block-form launch (step 0), then the plain form on gathered rows; the other member: blocks throughout
    assert calls["blocks"].count(17) == 1 and calls["plain"].count(17) == 7, calls
    assert calls["blocks"].count(3) == 8 and calls["plain"].count(3) == 0, calls
    with_blocks = mp.snapshot(ppo, "team")
    calls["blocks"].clear(); calls["plain"].clear()
    ref, _ = _member_run(False)
    ref.rollout()
    torch.cuda.synchronize()
    assert calls["blocks"] == [] and calls["plain"].count(17) == 8
    plain = mp.snapshot(ref, "team")
    for k, v in plain.items():
        assert (v is None) == (with_blocks[k] is None), k
        if v is not None:
            assert torch.equal(k6._bits(with_blocks[k]), k6._bits(v)), k
    assert with_blocks["actions"].shape[-1] == 17


# ---------------------------------------------------------------------------------------------------- K19
def _policy(head, O, seed, E=33, in_dim=8, depth=3, bounds=None):
    pol = ek.Policy(seed, in_dim, 256, depth, O, head, "tanh", bounds=bounds, out_gain=4.0, critic_hidden=512)
    obs = torch.from_numpy(np.random.default_rng(seed).normal(0, 1, (E, in_dim)).astype(np.float32)).cuda()
    return pol, obs


@pytest.mark.parametrize("O", [9, 18, 24])
def test_k19_greedy_is_the_argmax_with_the_lowest_index_on_a_tie(O):
    from ppo_and_friends_amd import kernels as K
    pol, obs = _policy("categorical", O, 50 + O)
    if O > 20:
        # classes 3 and 20 share one output row and one bias: an exact tie in every row, above every other class in some
        W, b = pol.actor.layers[-1]
        W[20], b[20] = W[3], b[3]
        W[3] *= 3.0
        W[20] *= 3.0
        pol.set_actor()
    got = pol.infer(obs, K.INFER_DETERMINISTIC).cpu().numpy()
    z = pol.actor.forward(obs.cpu().numpy())
    want, near = cases.hd.greedy("categorical", z)
    if O > 20:
        # (exact in every dtype and on the device: both classes are the same sum) the tie's rows are compared, not left out
        assert np.array_equal(z[:, 3], z[:, 20])
        tied = z.argmax(1) == 3
        assert tied.sum() >= 2, "the planted tie must win some rows"
        assert (got[tied] == 3).all() and not (got == 20).any()
        third = np.sort(np.delete(z, 20, axis=1), axis=1)
        near = np.where(tied, third[:, -1] - third[:, -2] < 2 * cases.hd.logit_bound(z).max(1), near)
    assert near.sum() <= cases.cap(len(z))
    assert np.array_equal(got[~near], want[~near])


@pytest.mark.parametrize("head,O", [("categorical", 18), ("categorical", 24), ("gaussian", 17), ("gaussian", 24)])
def test_k19_sampled_is_bitwise_k6s_action_and_greedy_gaussian_is_the_mean(head, O):
    from ppo_and_friends_amd import kernels as K
    bounds = (np.full(O, -0.4, np.float32), np.full(O, 0.4, np.float32)) if head == "gaussian" else None
    pol, obs = _policy(head, O, 70 + O, bounds=bounds)
    seed, offset = 0xABCDEF12345, 2 ** 32 - 9
    k6_act = pol.step_k6(obs, seed, offset)
    k19 = pol.infer(obs, K.INFER_SAMPLE, seed, offset)
    assert torch.equal(k6._bits(k19), k6._bits(k6_act))
    if head == "gaussian":
        z = pol.actor.forward(obs.cpu().numpy())
        want = cases.hd.unit_to_bounds(np.tanh(z), bounds, np.float64)
        want32 = cases.hd.unit_to_bounds(np.tanh(pol.actor.forward(obs.cpu().numpy(), np.float32)), bounds, np.float32)
        got = pol.infer(obs, K.INFER_DETERMINISTIC).double().cpu().numpy()
        assert (np.abs(got - want) <= cases.k12_bound(want, want32)).all()
