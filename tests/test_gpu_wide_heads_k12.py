"""
-m gpu: K12 for the wide heads of the wide width pair (256, 512) -- a 256-wide actor with 9 .. 24 outputs under a Categorical
or tanh-Gaussian head, behind PPOPolicy.fused_wide_heads (csrc/ppo_update_rowtile_heads.hpp, csrc/ppo_update_wide_heads.hip).

One mini-batch against float64 per tensor (tests/test_gpu_k12_wide_critic.py: run_wide, with the steering, the weight
overwrite, the reference and the per-tensor bound of tests/test_gpu_k12_gradients.py) at the smallest shapes at which each new
piece can go wrong:

  d1_B2_in8       gaussian 9     depth 1: no hidden backward ever touches the plane that holds output rows 8 .. 23; fewer rows
                                 than lanes; 8 inputs: the region behind the input rows at its floor of 768 floats
  d3_B17_in376    gaussian 17    tanh: humanoid's tile (the LDS edge of depth 3 is 432 inputs as for the narrow heads), a block
                                 with one live row and fifteen dead ones; a fifth action word group with one live word
  d3_B128_in256   categorical 18 leaky_relu: mario_bros_ram
  d2_B96_in40     categorical 24 the cap: every lane of a row's four holds six live classes
  d3_B64_in24     gaussian 24    entropy_weight 0.01: every d / d log_std term live, the log_std segment exactly 24 slots
  d4_B33_in160    categorical 9  the LDS edge of depth 4; class 8 alone in its lane's second slot

Class indices out of range are clamped as for the narrow heads (the steering plants them).

Measured on one MI355X (7 passed in 5.0 s), worst deviation over bound per tensor: 0.502 over the Gaussian cases (actor.1.bias
of the step without clip, d1_B2_in8), 0.342 over the Categorical cases (actor.4.weight of the step without clip, d4_B33_in160).
"""
import pytest
import torch

import test_gpu_k12_gradients as g12
import test_gpu_k12_wide_critic as wc

pytestmark = pytest.mark.gpu
WIDE = dict(ha=256, hc=512)


@pytest.fixture
def wide_heads(monkeypatch):
    """Both opt-ins, for the class, before any PPO of the test is built (376 and 256 inputs need fused_wide_shapes)."""
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_shapes", True)
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)


K12_CASES = {
    "d1_B2_in8": g12.case(O=8, depth=1, B=2, head=("gaussian", 9), act="relu", seed=811, **WIDE),
    "d3_B17_in376": g12.case(O=376, depth=3, B=17, head=("gaussian", 17), act="tanh", seed=812, **WIDE),
    "d3_B128_in256": g12.case(O=256, depth=3, B=128, head=("categorical", 18), act="leaky_relu", seed=813, **WIDE),
    "d2_B96_in40": g12.case(O=40, depth=2, B=96, head=("categorical", 24), act="relu", seed=814, **WIDE),
    "d3_B64_in24": g12.case(O=24, depth=3, B=64, head=("gaussian", 24), act="tanh", ent=0.01, seed=815, **WIDE),
    "d4_B33_in160": g12.case(O=160, depth=4, B=33, head=("categorical", 9), act="relu", seed=816, **WIDE),
}


@pytest.mark.parametrize("name", sorted(K12_CASES))
def test_k12_minibatch_against_float64(name, wide_heads):
    c = K12_CASES[name]
    wc.run_wide(c)


def test_the_updater_says_which_heads_it_runs(wide_heads):
    """description(): the line `verbose` prints names the actor's outputs and the attribute."""
    ppo = g12._ppo(K12_CASES["d2_B96_in40"])
    fused = ppo._fused_updater("p", 96)
    assert fused is not None and fused.wide and fused.split and fused.actor_desc.out_dim == 24
    assert "24 actor outputs (fused_wide_heads)" in fused.description(), fused.description()
    torch.cuda.synchronize()
