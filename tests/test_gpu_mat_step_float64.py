"""
-m gpu: ONE K16 rollout step (csrc/mat_update.hip, mat_policy_step_body: the narrow, the wide and the two block-form
kernels) against its restatement in float64 (tests/helpers/mat_step_cases.py: the network of oracle/mat_update_oracle.py,
the Philox draw of tests/helpers/philox.py, which tests/test_philox.py holds to the published known answers), at the shape
edges of the kernel and with the WEIGHTS OVERWRITTEN (mat_update_cases.draw_params: logits of O(1) -- at the default
initialisation the head's gain of 0.01 leaves every distribution uniform, and the log-probs near -log NA whatever the
decoder does).  What the restatement states and no other test does: which Philox counter a token draws from
(offset + env A + slot, stream 0, word x), that the draw is the inverse CDF of the decoder's probabilities, and that
agent i + 1 is conditioned on the action agent i just drew.  tests/test_mat_step_oracle.py shows on the CPU that each of
these, planted as an error, is caught by a case, and that every case meets its conditions.

Each case: the library's entry points launched directly (ppoaf_mat_policy_step, ppoaf_mat_policy_step_blocks) on the
package's network holding the case's bucket (offsets: fused_update._describe_mat, required to be the oracle's table):
  sampled   the draw; forced   the float64 reference's actions replayed, one entry below 0 and one at or above NA (clamped),
            on the saturated case also classes whose probability lies below float32's eps (log eps32 by the clamp);
  block     both again through the row-block table -- a non-identity slot_agent permutation, per-agent observation
            tensors, the env's action blocks filled -- required to be bitwise the plain form's outputs;
normalize_values on every other case ((0.3, 0.25)); two cases with actor observations of their own width.
  * actions: the float64 reference's on every kept token (near-tie rule of mat_step_cases: an env is left out from its first
    draw within 2 max_k bound_k + 1e-6 of a CDF edge on; the cap on such envs is a condition of the cases);
  * logp_out (kept tokens; forced launch: all) and value_out (all) per tensor: |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|,
    raised to 4 max|x32 - x64| of the same restatement in float32 (eval_kernels.k12_bound);
  * raw_action_out == action_out; critic_obs_copy_out and obs_copy_out bitwise the inputs;
  * every output is allocated with 16 tokens more (one env more per action block) holding a sentinel: untouched.
And once through the policy (MATPolicy.rollout_step under PPO.rollout): the counter advances by T E A, and every buffered
action is the restated draw at counter off0 + t E A + e A + slot from the float64 logits teacher-forced on the buffer.

Worst deviation / bound and envs left out per case, measured on the MI355X: see MEASURED below.
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import mat_update_oracle as mu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mat_float64 as M  # noqa: E402
import mat_step_cases as cases  # noqa: E402
import mat_update_cases as uc  # noqa: E402
import philox  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}                     # (case, launch) -> (kept tokens, envs left out, logp / bound, values / bound)
PAD = 16                       # tokens past the end of every output
I_SENT, F_SENT = -77, -12345.0

MEASURED = """
worst deviation / bound per case and launch, tokens compared and envs left out by the near-tie rule
(this file alone: 20 passed in 5.5 s)
  c5_3_18_5_21           forced   kept   63 tokens, 0 envs left out, logp 0.016  values 0.041
  c5_3_18_5_21           sampled  kept   63 tokens, 0 envs left out, logp 0.016  values 0.041
  c5_3_18_5_4            forced   kept   12 tokens, 0 envs left out, logp 0.026  values 0.085
  c5_3_18_5_4            sampled  kept   12 tokens, 0 envs left out, logp 0.045  values 0.085
  c5_3_18_5_5            forced   kept   15 tokens, 0 envs left out, logp 0.015  values 0.015
  c5_3_18_5_5            sampled  kept   15 tokens, 0 envs left out, logp 0.010  values 0.015
  chunk_16_128_8_2       forced   kept   32 tokens, 0 envs left out, logp 0.008  values 0.037
  chunk_16_128_8_2       sampled  kept   32 tokens, 0 envs left out, logp 0.010  values 0.037
  chunk_2_128_8_9        forced   kept   18 tokens, 0 envs left out, logp 0.017  values 0.022
  chunk_2_128_8_9        sampled  kept   18 tokens, 0 envs left out, logp 0.017  values 0.022
  chunk_3_97_5_11        forced   kept   33 tokens, 0 envs left out, logp 0.012  values 0.034
  chunk_3_97_5_11        sampled  kept   33 tokens, 0 envs left out, logp 0.012  values 0.034
  chunk_5_65_4_7         forced   kept   35 tokens, 0 envs left out, logp 0.012  values 0.036
  chunk_5_65_4_7         sampled  kept   32 tokens, 1 envs left out, logp 0.012  values 0.036
  dead_7_64_2_5          forced   kept   35 tokens, 0 envs left out, logp 0.036  values 0.028
  dead_7_64_2_5          sampled  kept   35 tokens, 0 envs left out, logp 0.020  values 0.028
  draw0_10_29_4_62       forced   kept  620 tokens, 0 envs left out, logp 0.021  values 0.037
  draw0_10_29_4_62       sampled  kept  620 tokens, 0 envs left out, logp 0.023  values 0.037
  draw1_10_86_7_37       forced   kept  370 tokens, 0 envs left out, logp 0.027  values 0.050
  draw1_10_86_7_37       sampled  kept  370 tokens, 0 envs left out, logp 0.030  values 0.050
  draw2_5_20_3_20        forced   kept  100 tokens, 0 envs left out, logp 0.034  values 0.043
  draw2_5_20_3_20        sampled  kept  100 tokens, 0 envs left out, logp 0.034  values 0.043
  draw3_7_103_8_25       forced   kept  175 tokens, 0 envs left out, logp 0.027  values 0.039
  draw3_7_103_8_25       sampled  kept  168 tokens, 1 envs left out, logp 0.027  values 0.039
  draw4_11_114_4_57      forced   kept  627 tokens, 0 envs left out, logp 0.035  values 0.028
  draw4_11_114_4_57      sampled  kept  627 tokens, 0 envs left out, logp 0.028  values 0.028
  draw5_1_103_3_53       forced   kept   53 tokens, 0 envs left out, logp 0.019  values 0.051
  draw5_1_103_3_53       sampled  kept   53 tokens, 0 envs left out, logp 0.019  values 0.051
  lds_1_32_8_17          forced   kept   17 tokens, 0 envs left out, logp 0.006  values 0.013
  lds_1_32_8_17          sampled  kept   17 tokens, 0 envs left out, logp 0.006  values 0.013
  mask_16_33_8_3         forced   kept   48 tokens, 0 envs left out, logp 0.015  values 0.018
  mask_16_33_8_3         sampled  kept   48 tokens, 0 envs left out, logp 0.015  values 0.018
  min_1_1_1_1            forced   kept    1 tokens, 0 envs left out, logp 0.003  values 0.001
  min_1_1_1_1            sampled  kept    1 tokens, 0 envs left out, logp 0.003  values 0.001
  sat_3_18_5_16          forced   kept   48 tokens, 0 envs left out, logp 0.035  values 0.019
  sat_3_18_5_16          sampled  kept   48 tokens, 0 envs left out, logp 0.049  values 0.019
(the block form is bitwise the plain form in every case, sampled and forced)
through the policy: 18 of 18 actions compared in each of the 4 steps, logp 0.021 .. 0.028 x bound
"""


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"  {c:22s} {l:8s} kept {v[0]:4d} tokens, {v[1]} envs left out, logp {v[2]:.3f}  values {v[3]:.3f}"
             for (c, l), v in sorted(WORST.items())]
    print("\nworst deviation / bound per case and launch:\n" + "\n".join(lines))
    out = os.environ.get("PPOAF_K16_REPORT")
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _bits(x):
    return x.contiguous().view(torch.int32)


class Device:
    """The case on the device: the package's network holding the case's bucket, its inputs, the launches."""

    def __init__(self, name):
        from ppo_and_friends_amd import _lib, kernels as K
        from ppo_and_friends_amd.fused_update import _describe_mat
        self.name, self.s = name, cases.steering(name)
        s, c = self.s, self.s.c
        A, O, NA, E = s.shape
        self._lib, self.lib, self.K = _lib, _lib.load(), K
        dev = self.dev = torch.device("cuda", 0)
        # MATPolicy takes two agents or more; the kernel takes one: the package's network alone for every case
        ac = self.ac = M.make_network(O, NA, A, c["seed"], dev)
        topo, why = _describe_mat(types.SimpleNamespace(actor_critic=ac, action_dtype="discrete"))
        assert why == "" and topo["bucket_total"] == s.size == ac.flat_params.numel()
        assert list(topo["offsets"]) == [o for _, _, o, _ in s.table], "the driver's offsets are not the oracle's table"
        assert (topo["obs_dim"], topo["num_agents"], topo["num_actions"]) == (O, A, NA)
        self.topo = topo
        with torch.no_grad():
            ac.flat_params.copy_(torch.as_tensor(s.params, dtype=torch.float32, device=dev))
        self.obs = torch.from_numpy(s.obs).to(dev).contiguous()
        self.Oa = c["own_obs"] or O
        self.actor_obs = torch.from_numpy(s.actor_obs).to(dev).contiguous() if c["own_obs"] else None
        self.vn = None
        if s.vn is not None:
            self.vn = (torch.tensor([s.vn[0]], dtype=torch.float32, device=dev), torch.tensor([s.vn[1]], dtype=torch.float32, device=dev))
        # the block form's table: slot s of env e reads row e of block slot_agent[s]
        rng = np.random.default_rng(c["seed"] + 50)
        self.slot_agent = rng.permutation(A)
        while A > 1 and np.array_equal(self.slot_agent, np.arange(A)):
            self.slot_agent = rng.permutation(A)
        self.obs_blocks, self.actor_blocks = [None] * A, [None] * A
        for slot, b in enumerate(self.slot_agent):
            self.obs_blocks[b] = self.obs[:, slot].contiguous()
            if self.actor_obs is not None:
                self.actor_blocks[b] = self.actor_obs[:, slot].contiguous()

    def launch(self, forced=None, blocks=False):
        """One launch -> dict of the outputs' first E A tokens (device tensors); the sentinels past them are checked here."""
        s, _lib = self.s, self._lib
        A, O, NA, E = s.shape
        n, dev, Oa = E * A, self.dev, self.Oa
        a = _lib.MatStepArgs()
        a.obs_dim, a.num_agents, a.num_actions, a.embedding = O, A, NA, 64
        for i, o in enumerate(self.topo["offsets"]):
            a.offsets[i] = o
        a.params = self.ac.flat_params.data_ptr()
        a.actor_obs_dim, a.E, a.seed, a.offset = Oa, E, s.seed, s.offset
        a.normalize_values = int(self.vn is not None)
        if self.vn is not None:
            a.vn_mean, a.vn_var = self.vn[0].data_ptr(), self.vn[1].data_ptr()
        ints = lambda m: torch.full((m,), I_SENT, dtype=torch.int64, device=dev)
        floats = lambda m: torch.full((m,), F_SENT, dtype=torch.float32, device=dev)
        out = dict(actions=ints(n + PAD), raw=ints(n + PAD), logp=floats(n + PAD), values=floats(n + PAD),
                   critic_copy=floats((n + PAD) * O), obs_copy=floats((n + PAD) * Oa))
        a.action_out, a.raw_action_out = out["actions"].data_ptr(), out["raw"].data_ptr()
        a.logp_out, a.value_out = out["logp"].data_ptr(), out["values"].data_ptr()
        a.critic_obs_copy_out, a.obs_copy_out = out["critic_copy"].data_ptr(), out["obs_copy"].data_ptr()
        f = None
        if forced is not None:
            f = torch.as_tensor(np.asarray(forced, dtype=np.int64).reshape(-1)).to(dev).contiguous()
            a.forced_action = f.data_ptr()
        env_actions = None
        if blocks:
            tb = _lib.MatStepBlocks()
            tb.n_blocks = A
            env_actions = [ints(E + 1) for _ in range(A)]
            for slot, b in enumerate(self.slot_agent):
                tb.slot_agent[slot] = int(b)
            for b in range(A):
                tb.critic_obs[b], tb.env_action[b] = self.obs_blocks[b].data_ptr(), env_actions[b].data_ptr()
                tb.actor_obs[b] = None if self.actor_obs is None else self.actor_blocks[b].data_ptr()
            _lib.check(self.lib.ppoaf_mat_policy_step_blocks(C.byref(a), C.byref(tb), self.K.stream()), "mat_policy_step_blocks")
        else:
            a.critic_obs = self.obs.data_ptr()
            a.actor_obs = None if self.actor_obs is None else self.actor_obs.data_ptr()
            _lib.check(self.lib.ppoaf_mat_policy_step(C.byref(a), self.K.stream()), "mat_policy_step")
        torch.cuda.synchronize()
        what = f"{self.name} ({'block' if blocks else 'plain'} form, {'forced' if f is not None else 'sampled'})"
        res = {}
        for k, width in (("actions", 1), ("raw", 1), ("logp", 1), ("values", 1), ("critic_copy", O), ("obs_copy", Oa)):
            t = out[k]
            sent = I_SENT if t.dtype == torch.int64 else F_SENT
            assert bool((t[n * width:] == sent).all()), f"{what}: {k} written past its {n} tokens"
            res[k] = t[:n * width]
        if blocks:
            for b, t in enumerate(env_actions):
                assert int(t[E]) == I_SENT, f"{what}: env action block {b} written past its {E} envs"
            res["env_actions"] = torch.stack([env_actions[b][:E] for b in self.slot_agent], 1)        # [E, A] in slot order
        # copies
        assert torch.equal(res["raw"], res["actions"]), f"{what}: raw_action_out is not action_out"
        assert torch.equal(_bits(res["critic_copy"]), _bits(self.obs.reshape(-1))), f"{what}: critic_obs_copy_out is not the input"
        src = self.obs if self.actor_obs is None else self.actor_obs
        assert torch.equal(_bits(res["obs_copy"]), _bits(src.reshape(-1))), f"{what}: obs_copy_out is not the actor's observations"
        return res

    def judged(self, res, forced):
        """The launch under mat_step_cases.judge: recorded, printed, asserted."""
        s = self.s
        A, O, NA, E = s.shape
        got = dict(actions=res["actions"].cpu().numpy().reshape(E, A), logp=res["logp"].double().cpu().numpy().reshape(E, A),
                   values=res["values"].double().cpu().numpy().reshape(E, A))
        assert got["actions"].min() >= 0 and got["actions"].max() < NA
        wrong, fracs = cases.judge(s, got, forced)
        kept = E * A if forced else int(s.kept.sum())
        left = 0 if forced else s.left_out()
        launch = "forced" if forced else "sampled"
        WORST[(self.name, launch)] = (kept, left, fracs["logp"], fracs["values"])
        print(f"{self.name} {launch}: {kept} of {E * A} tokens compared, {left} envs left out, {wrong} actions differ, "
              f"logp {fracs['logp']:.3f} x bound, values {fracs['values']:.3f} x bound")
        assert wrong == 0, f"{self.name} {launch}: {wrong} compared actions are not the float64 reference's"
        bad = {k: v for k, v in fracs.items() if not v <= 1.0}
        assert not bad, f"{self.name} {launch}: " + ", ".join(f"{k} {v:.3g} x bound" for k, v in bad.items())
        return got


@pytest.mark.parametrize("name", list(cases.CASES))
def test_k16_step_against_float64(name):
    d = Device(name)
    s = d.s
    A, O, NA, E = s.shape
    assert s.left_out() <= cases.cap(E)
    sampled = d.launch()
    d.judged(sampled, forced=False)
    forced = d.launch(forced=s.forced)
    got = d.judged(forced, forced=True)
    clamped = np.clip(s.forced, 0, NA - 1)
    assert np.array_equal(got["actions"], clamped)
    if s.c["saturate"]:
        # forced classes below float32's eps: the clamp's log(eps32), within the tensor's bound
        assert s.n_saturated >= 2
        bound = cases.k12_bound(s.f64["logp"], s.f32["logp"])[s.saturated]
        assert (np.abs(got["logp"][s.saturated] - np.log(cases.EPS32)) <= bound).all(), got["logp"][s.saturated]
    # ---- the block form: bitwise the plain form
    for plain, f in ((sampled, None), (forced, s.forced)):
        blk = d.launch(forced=f, blocks=True)
        tag = f"{name}: block form, {'sampled' if f is None else 'forced'}"
        assert torch.equal(blk["actions"], plain["actions"]), f"{tag}: actions differ from the plain form's"
        for k in ("logp", "values"):
            assert torch.equal(_bits(blk[k]), _bits(plain[k])), f"{tag}: {k} is not bitwise the plain form's"
        assert torch.equal(blk["env_actions"].reshape(-1), plain["actions"]), f"{tag}: the env's action blocks"
    assert A == 1 or not np.array_equal(d.slot_agent, np.arange(A))


def test_block_form_cases_cover_the_kernels():
    """The block form runs on every case: among them a wide one, one with 16 agents and one with one agent."""
    shapes = [(c["A"], c["O"]) for c in cases.CASES.values()]
    assert any(o > 32 for _, o in shapes) and any(a == 16 for a, _ in shapes) and any(a == 1 for a, _ in shapes)
    assert len(shapes) >= 4


def test_counters_through_the_policy():
    """MATPolicy.rollout_step under PPO.rollout at (3, 18, 5), E = 6, T = 4, the bucket overwritten: the generator's offset
    advances by exactly T E A, and every buffered action is the inverse-CDF draw at counter off0 + t E A + e A + slot
    (the buffer's slot order) from the float64 logits teacher-forced on the buffer's observations and actions."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box, Discrete
    A, O, NA, E, T = 3, 18, 5, 6, 4
    dev = torch.device("cuda", 0)
    env_gen = lambda: SyntheticFixedLengthEnv(E, O, Discrete(NA), T, dev, reward="uniform", seed=41, num_agents=A)
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"mat": (MATPolicy, sp, sp, Discrete(NA), {})}, device=dev, random_seed=6, normalize_obs=False,
              normalize_rewards=False, envs_per_proc=E, ts_per_rollout=T, batch_size=E * T, epochs_per_iter=1, update_mode="fused",
              use_graphs=False)
    pol = ppo.policies["mat"]
    assert pol.fused_step_unsupported_reason() == ""
    params = uc.draw_params(A, O, NA, np.random.default_rng(77))
    table, size = mu.bucket_table(A, O, NA)
    assert pol.actor_critic.flat_params.numel() == size
    base = pol.actor_critic.flat_params.data_ptr()
    for (_, tname, off, shape), (pname, p) in zip(table, pol.actor_critic.named_parameters()):
        assert tname == pname and (p.data_ptr() - base) // 4 == off and tuple(p.shape) == tuple(shape), tname
    with torch.no_grad():
        pol.actor_critic.flat_params.copy_(torch.as_tensor(params, dtype=torch.float32, device=dev))
    rng = pol.actor.distribution.rng
    seed, off0 = rng.seed, rng.offset
    launches, inner = [], pol.rollout_step
    pol.rollout_step = lambda *a, **k: (launches.append(1), inner(*a, **k))[1]
    ppo.rollout()
    assert len(launches) == T, "K16 did not step the rollout"
    assert rng.offset == off0 + T * E * A
    buf = pol.buffer
    # the rollout's slot order: finalize_dataset has put the buffer's agent axis into the dataset's order (quirk Q14);
    # rollout slot s is dataset slot k[s]
    k = np.argsort(np.argsort(pol.agent_slot_order())[pol._dataset_slot_order])
    actions = buf.actions.cpu().numpy().reshape(T, E, A)[:, :, k]
    obs = buf.critic_observations.cpu().numpy().reshape(T, E, A, O)[:, :, k]
    assert np.array_equal(buf.raw_actions.cpu().numpy().reshape(T, E, A)[:, :, k], actions)
    logp = buf.log_probs.double().cpu().numpy().reshape(T, E, A)[:, :, k]
    compared = 0
    for t in range(T):
        r64, r32 = (cases.step_reference(params, A, O, NA, obs[t], seed, off0 + t * E * A, forced=actions[t], dtype=dt)
                    for dt in (torch.float64, torch.float32))
        kept = cases.kept_tokens(r64["logits"], r64["gap"])
        assert (~kept).any(1).sum() <= cases.cap(E)
        wrong = (r64["drawn"] != actions[t]) & kept
        assert not wrong.any(), f"step {t}: {int(wrong.sum())} buffered actions are not the draw at their counter"
        frac = cases.worst(logp[t], r64["logp"], r32["logp"])
        print(f"step {t}: {int(kept.sum())} of {E * A} actions compared, logp {frac:.3f} x bound")
        assert frac <= 1.0
        compared += int(kept.sum())
    assert compared >= T * E * A - 2 * A * T and len(np.unique(actions)) > 1
