"""
-m gpu: K20 behind `MATPolicy.fused_mat_eval_forms` -- ppoaf_mat_box_policy_infer (Box teams) and ppoaf_mat_policy_infer_wide
(Discrete, observations 65 .. 128 wide), at E = 16 // A and one more (a partial tile, two workgroups).
Box, sampled: bitwise ppoaf_mat_box_policy_step's action_out.  Box, deterministic: the package's MATActorCritic on the CPU in
float64 with the attention written out (network, weights and attention of tests/test_gpu_mat_box_float64.py), decoded greedily
with agent i + 1 fed the kernel's own action of agent i.  Bound: that file's rule for K16's mean, 1e-6 |mean64| + 1e-6, raised
to 4 x the float32-on-CPU deviation; through the refinement (tanh: slope <= 1) times (hi - lo) / 2; plus the float32 rounding
of the output, that file's 8 x 2^-24 (hi - lo + |lo|) (the unit box: 8 x 2^-24).
Discrete, wide: sampled bitwise ppoaf_mat_policy_step's; deterministic against tests/helpers/mat_float64.py under the near-tie
rule and cap of tests/test_gpu_mat_infer.py.  WIDE_SEED = 11, obs seed 111, E = 512: the float64 decode alone leaves out 0 of
1 536, 0 of 8 192 and 0 of 1 024 decisions at (3, 71, 5), (16, 65, 5), (2, 128, 8) (checked on the CPU).

MEASURED (one run on the MI355X, this file 4 s): Box, deterministic, worst deviation / bound over both E, bounds / unit box:
  A1 O1 NA1 0.128 / 0.178   A3 O18 NA5 0.402 / 0.614   A16 O33 NA8 0.467 / 0.466   A5 O65 NA1 0.306 / 0.226
  A2 O128 NA8 0.467 / 0.704.  Discrete, wide: 0 decisions left out, 0 compared ones differ, at all three shapes.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import test_gpu_mat_box_float64 as B
import test_gpu_mat_infer as I

pytestmark = pytest.mark.gpu
DEV = I.DEV
BOX_SHAPES = [(1, 1, 1), (3, 18, 5), (16, 33, 8), (5, 65, 1), (2, 128, 8)]
WIDE_SHAPES = [(3, 71, 5), (16, 65, 5), (2, 128, 8)]
WIDE_SEED = 11
SEED, OFFSET = 0x1234567, 2 ** 33 + 5


def _box_network(A, O, NA):
    from ppo_and_friends_amd.fused_update import _describe_mat
    ac = B._network(A, O, NA)
    w = B._weights(ac, "")
    ac.to(DEV)
    with torch.no_grad():
        for n, p in ac.named_parameters():
            p.copy_(torch.as_tensor(w[n], dtype=torch.float32))
    topo, why = _describe_mat(types.SimpleNamespace(actor_critic=ac, action_dtype="continuous", fused_mat_box_actions=True))
    assert why == ""
    return ac, w, topo


def _bounds(NA, spread):
    """Device (lo, hi) from (-0.5, 2.0); spread: a bound of its own for every dimension."""
    lo, hi = np.linspace(B.LO, B.LO + 0.3 * spread, NA), np.linspace(B.HI, B.HI + spread, NA)
    return torch.as_tensor(lo, dtype=torch.float32, device=DEV), torch.as_tensor(hi, dtype=torch.float32, device=DEV)


def box_actions(ac, topo, obs, bounds, seed=0, offset=0, mode=None, order=None):
    """mode None: ppoaf_mat_box_policy_step's action_out on grouped obs [E, A, O]; else ppoaf_mat_box_policy_infer, grouped
    -> [E, A, NA] or, with `order`, agent-major obs [A * E, O] in that slot order -> [A * E, NA]."""
    from ppo_and_friends_amd import _lib, kernels as K
    A, O, NA = topo["num_agents"], topo["obs_dim"], topo["num_actions"]
    E = obs.numel() // (A * O)
    box = (_lib.MatBoxStepArgs if mode is None else _lib.MatBoxInferArgs)()
    a = box.mat
    I._fill(a, topo, ac)
    box.enc_bias_offset, box.log_std_offset, box.min_std = topo["enc_bias_offset"], topo["log_std_offset"], B.MIN_STD
    box.act_lo, box.act_hi = (None, None) if bounds is None else (bounds[0].data_ptr(), bounds[1].data_ptr())
    act = torch.full((E, A, NA) if order is None else (A * E, NA), float("nan"), device=DEV)
    a.E, a.seed, a.offset, box.action_out = E, seed, offset, act.data_ptr()
    if mode is None:
        raw, lp, val = (torch.zeros(E, A, NA, device=DEV) for _ in range(3))
        a.actor_obs_dim, a.critic_obs, a.actor_obs = O, obs.data_ptr(), obs.data_ptr()
        box.raw_action_out, a.logp_out, a.value_out = raw.data_ptr(), lp.data_ptr(), val.data_ptr()
        _lib.check(_lib.load().ppoaf_mat_box_policy_step(C.byref(box), K.stream()), "mat_box_policy_step")
    else:
        a.obs, a.mode = obs.data_ptr(), mode
        for i, k in enumerate(range(A) if order is None else order):
            a.slot_agent[i] = int(k)
        a.obs_env_stride, a.obs_agent_stride = a.act_env_stride, a.act_agent_stride = (A, 1) if order is None else (1, E)
        K.mat_box_policy_infer(box)
    return act


@pytest.fixture
def k20_wide(monkeypatch):
    """tests/test_gpu_mat_infer.py's k20_actions through the wide entry point."""
    from ppo_and_friends_amd import kernels as K
    monkeypatch.setattr(K, "mat_policy_infer", K.mat_policy_infer_wide)
    return I.k20_actions


@pytest.mark.parametrize("shape", BOX_SHAPES)
def test_box_sampled_is_k16_and_deterministic_is_float64(shape, monkeypatch):
    from ppo_and_friends_amd.networks import attention
    monkeypatch.setattr(attention._AttentionCore, "apply", staticmethod(B._plain_attention))
    A, O, NA = shape
    ac, w, topo = _box_network(A, O, NA)
    for E, unit_box in [(e, u) for e in (16 // A, 16 // A + 1) for u in (False, True)]:
        obs = I._obs(E, A, O, seed=7 + E)
        bounds = None if unit_box else _bounds(NA, 1.0)
        want = box_actions(ac, topo, obs, bounds, SEED + E, OFFSET)
        got = box_actions(ac, topo, obs, bounds, SEED + E, OFFSET, mode=0)
        assert torch.isfinite(want).all() and torch.equal(got, want), (shape, E, unit_box, int((got != want).sum()))
        assert not torch.equal(got, box_actions(ac, topo, obs, bounds, SEED + E, OFFSET + E * A, mode=0))      # the counter counts
        # deterministic: bounds (-0.5, 2.0) or the unit box; the counter is not read
        lo, hi = (-1.0, 1.0) if unit_box else (B.LO, B.HI)
        bounds = None if unit_box else _bounds(NA, 0.0)
        got = box_actions(ac, topo, obs, bounds, 1, 2, mode=1)
        assert torch.equal(got, box_actions(ac, topo, obs, bounds, 99, 10 ** 12, mode=1))
        got, mean = got.cpu().numpy(), {}
        for dtype in (torch.float64, torch.float32):
            net = B._network(A, O, NA, w, dtype)
            with torch.no_grad():
                enc, _ = net.critic(obs.cpu().to(dtype))
                block, rows = torch.zeros(E, A, NA, dtype=dtype), []
                for i in range(A):
                    rows.append(net.actor(block, enc)[:, i])
                    if i + 1 < A:
                        block[:, i + 1] = torch.as_tensor(got[:, i], dtype=dtype)      # the kernel's own action
            mean[dtype] = torch.stack(rows, 1).double().numpy()
        m64 = mean[torch.float64]
        b_mean = np.maximum(1e-6 * np.abs(m64) + 1e-6, 4 * np.abs(mean[torch.float32] - m64))
        bound = b_mean * (hi - lo) / 2 + 8 * 2.0 ** -24 * (1.0 if unit_box else hi - lo + abs(lo))
        frac = float((np.abs(got - (lo + (np.tanh(m64) + 1.0) / 2.0 * (hi - lo))) / bound).max())
        print(f"\nK20 Box A{A} O{O} NA{NA} E{E} {'unit box' if unit_box else 'bounds'}: worst {frac:.3f} x bound")
        assert frac <= 1.0 and (O == 1 or np.ptp(got) > 0) and got.min() >= lo and got.max() <= hi


@pytest.mark.parametrize("form", ["box", "wide"])
def test_agent_major_layout_is_the_grouped_result_permuted(form, k20_wide):
    A, O, order, E = 3, 18 if form == "box" else 71, [2, 0, 1], 6
    if form == "box":
        ac, _, topo = _box_network(A, O, 5)
        run = lambda obs, mode, order=None: box_actions(ac, topo, obs, _bounds(5, 1.0), 9, 31, mode, order)
    else:
        ac, topo = I._network(A, O, 5, WIDE_SEED)
        run = lambda obs, mode, order=None: k20_wide(ac, topo, obs, mode, 9, 31, order).unsqueeze(-1)
    order_t = torch.as_tensor(order, device=DEV)
    grouped = I._obs(E, A, O, seed=46)
    major = torch.empty(A, E, O, device=DEV)
    major[order_t] = grouped.transpose(0, 1)                                    # env agent order[s] sits in slot s
    for mode in (1, 0):
        got = run(major.reshape(A * E, O), mode, order).reshape(A, E, -1)
        assert torch.equal(got[order_t].transpose(0, 1), run(grouped, mode)), (form, mode)


@pytest.mark.parametrize("shape", WIDE_SHAPES)
def test_wide_discrete_sampled_is_k16_and_deterministic_is_float64(shape, k20_wide):
    import mat_float64 as M
    A, O, NA = shape
    ac, topo = I._network(A, O, NA, WIDE_SEED)
    for E in (16 // A, 16 // A + 1):
        obs = I._obs(E, A, O, seed=E)
        want = I.k16_actions(ac, topo, obs, SEED + E, 977 * E)
        assert int(want.min()) >= 0 and torch.equal(k20_wide(ac, topo, obs, 0, SEED + E, 977 * E), want), (shape, E)
    obs = I._obs(512, A, O, seed=100 + WIDE_SEED)
    got = k20_wide(ac, topo, obs, 1, 1, 2)
    assert torch.equal(got, k20_wide(ac, topo, obs, 1, 99, 10 ** 12))                  # the counter is not read
    want, logits = M.float64_logits_decode(ac.state_dict(), O, NA, A, obs.cpu().numpy())
    keep, got = M.compared_slots(logits), got.cpu().numpy()
    print(f"\n{shape}: {(~keep).sum()} of {keep.size} decisions left out, {((got != want) & keep).sum()} compared ones differ")
    assert (~keep).mean() <= 0.005 and not ((got != want) & keep).any() and len(np.unique(got)) > 1


@pytest.mark.parametrize("form,on", [("box", True), ("box", False), ("wide", True), ("wide", False)])
def test_evaluation_through_the_policy_is_one_k20_launch_per_step(form, on, monkeypatch):
    """On: test_policy issues one launch of the form's entry point per env step and no module forward.  Off: what it always did."""
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv as Env
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.spaces import Box, Discrete
    from ppo_and_friends_amd.testing import test_policy as run_test_policy
    O, space = (18, Box(B.LO, B.HI, (5,), np.float32)) if form == "box" else (71, Discrete(5))
    steps, launches, modules = [], {}, []
    monkeypatch.setattr(Env, "step", lambda self, a, _f=Env.step: (steps.append(1), _f(self, a))[1])

    def env_gen():
        env = Env(9, O, space, 40, DEV, reward="uniform", seed=5, term_prob=0.08, num_agents=3)
        env.term_table[-1] = True                          # every row finishes once per horizon
        return env
    sp = Box(-np.inf, np.inf, (O,), np.float32)
    ppo = PPO(env_gen, {"agent": (MATPolicy, sp, sp, space, {})}, device=DEV, random_seed=1, envs_per_proc=9, ts_per_rollout=16,
              batch_size=16, save_state=False, update_mode="auto", normalize_obs=False, normalize_rewards=False)
    pol = ppo.policies["agent"]
    pol.fused_mat_box_actions, pol.fused_mat_eval_forms = True, on
    for name in ("mat_policy_infer", "mat_policy_infer_wide", "mat_box_policy_infer"):
        monkeypatch.setattr(K, name, lambda a, _n=name, _f=getattr(K, name): (launches.setdefault(_n, []).append(1), _f(a))[1])
    for net in (pol.actor, pol.critic):
        monkeypatch.setattr(net, "forward", lambda *a, _f=net.forward, **k: (modules.append(1), _f(*a, **k))[1])
    info = run_test_policy(ppo, 20, deterministic=True, check_every=5, max_steps=4000)
    assert info["num_test_runs"] == 20 and len(steps) > 0
    want = {"mat_box_policy_infer" if form == "box" else "mat_policy_infer_wide": [1] * len(steps)} if on else {}
    assert launches == want and bool(modules) != on
