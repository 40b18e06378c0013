"""
-m gpu: the fused update kernels with the action heads' GRADIENT GATES CLOSED in part of the mini-batch, against float64.

Each hand-derived backward of a head restates "autograd passes no gradient through a clamp" as 0 / 1 factors (in_range, pass,
pass_t, dmax, dsp).  On initial weights and N(0, 1) observations every one of them reads 1; here the policy's own bucket is
steered (tests/helpers/head_gates.py: the actor's last layer scaled, log_std set to -8 / 25 by dimension, observations and
actions planted) until the mini-batch holds entries on both sides of every gate, none of them where float32 could take the
other side.  The census of the float64 reference -- and that the float32 reference reports the same one, entry for entry
-- is asserted in every case (Steered / the helpers' Steering); tests/test_head_gates_oracle.py shows on the CPU that a
wrong gate planted in the float32 reference then misses the bound by far more than 2.5 x.

Per case ONE mini-batch: the gradient bucket, the eight totals (entropy and KL see the clamps), the step, m and v with the
clip on and off, padding unwritten -- the checks and the bound rule of the sibling files, untouched:

  case               runs through                                 copy of the gates reached
  cat8_64            g12.run_case, all four FORMS                 ppo_head_rows' Categorical arm (csrc/ppo_update_dev.hpp): both
                                                                  class slots of a lane quad, a ragged tile
  cat5_narrow        g12.run_case                                 the same text compiled into csrc/ppo_update_narrow.hip (32/256)
  mcat_323           g12.run_case                                 mcat_entropy_grad (csrc/action_heads.hpp), rows of mixed kinds
  bern6_wide_critic  wc.run_wide                                  bern_entropy_grad in csrc/ppo_update_wide.hip (256/512)
  gau8_64            g12.run_case                                 every Gaussian gate: floored dimensions 0 and 4, identity
                                                                  dimensions 1 and 5, the tanh gate in dimension 7
  gau3_rowpair       g12.run_case                                 the row-pair build (256/256, csrc/ppo_update_rowpair.hpp)
  cat24_heads,       wc.run_wide under fused_wide_heads           csrc/ppo_update_rowtile_heads.hpp: six classes per lane, a fifth
  gau17_heads                                                     action-word group
  lean_cat2,         test_gpu_k12_lean.run_lean                   csrc/ppo_update_lean.hip: the export says 1; bitwise the general
  lean_gau2                                                       kernel; within the bound of float64
  K22 cat8 / gau4    the launcher and checks of                   ppo_head_loss in csrc/lstm_update.hip (H 32, S 4, B 20)
                     tests/test_gpu_lstm_update_float64.py
  K15 3x8 / 16x5     Device + judge_gradient of                   K15's own head (csrc/mat_update.hip)
                     tests/test_gpu_mat_update_float64.py

NOT SHOWN BY ANY CASE, because float32 cannot show them (tests/test_head_gates_oracle.py holds both to that): the gate on the
ENTROPY term of the discrete heads (dropping it moves a logit's gradient by less than eps32 x the entropy weight) and the
identity branch of softplus' derivative (sigmoid(x) == 1.0f for x > 17).  Exact ties, pass0 and the NaN / Inf flag: see the
helper's docstring.
"""
import os
import sys

import pytest

import test_gpu_k12_gradients as g12
import test_gpu_k12_lean as lean
import test_gpu_k12_wide_critic as wc
import test_gpu_lstm_update_float64 as k22
import test_gpu_mat_update_float64 as k15

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_gates as hg  # noqa: E402
import lstm_update_cases  # noqa: E402
import mat_update_cases  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}                     # (kernel copy, head) -> (worst fraction of the bound, where)
CENSUS = {}                    # case -> the census of its float64 reference

MEASURED = """
On one MI355X (14 passed in 7.90s; open / closed entries per gate of the policies' real weights, then worst deviation / bound):
census (open/closed entries per gate, kinds):
bern6_wide_critic    floor 165/33  ceil 171/27  kinds high0:16 high1:11 low0:11 low1:22
cat24_heads          floor 271/521  ceil 787/5  chosen 15/18  kinds a:8 b:7 c:16 d:2
cat5_narrow          floor 47/38  ceil 79/6  chosen 8/9  kinds a:6 b:2 c:7 d:2
cat8_64              floor 122/142  ceil 259/5  chosen 16/17  kinds a:6 b:10 c:14 d:3
gau17_heads          density 475/86  tanh 552/9  std_floor 12/5  identity 13/4  kinds
gau3_rowpair         density 110/34  tanh 129/15  std_floor 2/1  identity 2/1  kinds
gau8_64              density 227/37  tanh 253/11  std_floor 6/2  identity 6/2  kinds
k15_16_7_5_3         floor 180/60  ceil 230/10  chosen 31/17  kinds a:24 b:7 c:14 d:3
k15_3_18_8_11        floor 216/48  ceil 260/4  chosen 25/8  kinds a:18 b:7 c:5 d:3
k22_cat8             floor 99/61  ceil 156/4  chosen 12/8  kinds a:2 b:10 c:6 d:2
k22_gau4             density 62/18  tanh 71/9  std_floor 3/1  identity 3/1  kinds
lean_cat2            floor 70/26  ceil 70/26  chosen 22/26  kinds a:22 c:13 d:13
lean_gau2            density 26/8  tanh 29/5  std_floor 1/1  identity 1/1  kinds
mcat_323             floor 170/94  ceil 210/54  chosen 41/58  kinds a:35 b:6 c:37 d:21
worst deviation / bound per kernel copy and head:
K15            categorical        0.565  k15_16_7_5_3 / slab / gradient: critic.blocks.0.mlp.2.bias
K22            categorical        0.398  gradient: actor.ff1.bias
K22            gaussian           0.359  gradient: actor.w_hh
general        categorical        0.390  cat8_64 / slabs / no clip step: actor.0.bias
general        gaussian           0.785  gau8_64 / chain / no clip step: actor.1.bias
general        multi_categorical  0.334  mcat_323 / chain / clip step: actor.0.bias
lean           categorical        0.162  lean_cat2 / gradient: actor.1.weight
lean           gaussian           0.249  lean_gau2 / gradient: actor.2.bias
narrow         categorical        0.331  cat5_narrow / chain / clip step: critic.2.bias
row pairs      gaussian           0.492  gau3_rowpair / chain / no clip step: actor.0.bias
wide           bernoulli          0.330  bern6_wide_critic / wide / clip step: critic.2.bias
wide heads     categorical        0.335  cat24_heads / wide / clip step: actor.1.bias
wide heads     gaussian           0.628  gau17_heads / wide / gradient: actor.0.weight
"""


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ncensus (open/closed entries per gate, kinds):\n" + "\n".join(f"{k:20s} {v}" for k, v in sorted(CENSUS.items())))
    print("worst deviation / bound per kernel copy and head:\n" +
          "\n".join(f"{c:14s} {h:18s} {v[0]:.3f}  {v[1]}" for (c, h), v in sorted(WORST.items())))


def _note(copy, head, frac, where):
    if frac > WORST.get((copy, head), (-1.0, ""))[0]:
        WORST[(copy, head)] = (float(frac), where)


def _through_g12(copy, name, c, run):
    """Run a sibling file's case runner and move what it noted in g12.WORST under this module's (copy, head)."""
    seen = []
    inner = g12.Steered

    class Noting(inner):
        def __init__(self, case):
            super().__init__(case)
            assert case["gates"] and self.census, "the gates steering did not run"
            seen.append(self.census)

    keep = dict(g12.WORST)
    g12.WORST.clear()
    g12.Steered = Noting
    try:
        run(c)
        for (form, head), (frac, where) in g12.WORST.items():
            _note(copy, head, frac, f"{name} / {form} / {where}")
    finally:
        g12.Steered = inner
        g12.WORST.clear()
        g12.WORST.update(keep)
    assert seen, "the case never built its steering"
    CENSUS[name] = seen[0]


COPIES = {"cat8_64": "general", "cat5_narrow": "narrow", "mcat_323": "general", "bern6_wide_critic": "wide",
          "gau8_64": "general", "gau3_rowpair": "row pairs"}


@pytest.mark.parametrize("name", sorted(hg.K12_CASES))
def test_k12_gates(name, monkeypatch):
    c = g12.case(**hg.K12_CASES[name])
    if c["hc"] == 512:
        _through_g12(COPIES[name], name, c, wc.run_wide)
    else:
        _through_g12(COPIES[name], name, c, lambda case: g12.run_case(case, monkeypatch))


@pytest.mark.parametrize("name", sorted(hg.K12_HEADS_CASES))
def test_k12_wide_heads_gates(name, monkeypatch):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)
    _through_g12("wide heads", name, g12.case(**hg.K12_HEADS_CASES[name]), wc.run_wide)


@pytest.mark.parametrize("name", sorted(hg.K12_LEAN_CASES))
def test_k12_lean_gates(name):
    c = g12.case(**hg.K12_LEAN_CASES[name])
    out = []
    _through_g12("lean", name, c, lambda case: out.append(lean.run_lean(name, case)))
    _note("lean", c["head"][0], out[0][0], f"{name} / {out[0][1]}")


@pytest.mark.parametrize("name", sorted(lstm_update_cases.GATES_CASES))
def test_k22_gates(name):
    """The launcher and every check of tests/test_gpu_lstm_update_float64.py (its Steered asserts the census)."""
    c = lstm_update_cases.GATES_CASES[name]
    assert c["gates"]
    inner, seen = k22.Steered, []

    class Noting(inner):
        def __init__(self, case):
            super().__init__(case)
            seen.append(self.s.census)

    k22.WORST.pop(name, None)
    k22.Steered = Noting
    try:
        k22.run_case(name, c)
    finally:
        k22.Steered = inner
        if name in k22.WORST:
            _note("K22", c["head"][0], *k22.WORST.pop(name))
    CENSUS[name] = seen[0]


@pytest.mark.parametrize("name", sorted(mat_update_cases.GATES_CASES))
def test_k15_gates(name):
    """Device, the three forms and judge_gradient of tests/test_gpu_mat_update_float64.py (its Device asserts the census)."""
    assert mat_update_cases.GATES_CASES[name]["saturate"]
    try:
        k15.run_case(name)
    finally:
        for key in [k for k in k15.WORST if k[0] == name]:
            frac, where = k15.WORST.pop(key)
            _note("K15", "categorical", frac, f"{name} / {key[1]} / {where}")
    s = k15.steering(name)
    NA = s.shape[2]
    CENSUS[name] = hg.describe("categorical", (), dict(gate_args=dict(n=s.r64["probs"].reshape(-1, NA))),
                               s.mb.raw_actions.reshape(-1))
