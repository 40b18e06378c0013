"""
What the wide heads of the wide width pair (256, 512) -- a 256-wide actor with 9 .. 24 outputs, Categorical or tanh-Gaussian;
csrc/policy_wide_heads.hip, csrc/ppo_update_rowtile_heads.hpp -- need restated beside tests/helpers/policy_step_cases.py:
the LDS formulas of the 24-wide carves and the K6+K7 cases of tests/test_gpu_wide_heads_step.py (no device).
"""
import functools

import numpy as np

import policy_step_cases as cases

CAT, GAU = cases.CAT, cases.GAU
PAIR = (256, 512)
WIDE_OUT = 24
LDS_LIMIT = 160 * 1024


def step_lds_floats(in_dim, hidden, depth, out_dim):
    """mlp_rows_forward_lds_floats (csrc/mlp_device.hpp): more than 8 outputs take the 24-wide carve -- sWout [24, H] and
    sOut [16][24] -- where policy_step_cases.lds_floats restates 8 * hidden and 16 * 16."""
    if out_dim <= 8:
        return cases.lds_floats(in_dim, hidden, depth)
    hs, inp = hidden + 4, 16 * ((in_dim + 15) // 16) + 4
    return (depth + 1) * hidden + WIDE_OUT * hidden + 16 * inp + 2 * 16 * hs + 16 * WIDE_OUT


def rowtile_lds_bytes(in_dim, depth, out_dim, hidden=256):
    """fwd_bwd's dynamic LDS for the actor's row tile (csrc/ppo_update.hip: fwd_bwd_lds_bytes): rowtile_lds_floats, or for more
    than 8 outputs rowtile_heads_lds_floats (csrc/ppo_update_dev.hpp) -- the same terms with a floor of 2 x 16 x 24 floats
    under the input rows -- rounded up to 16 bytes, plus the eight waves' line slots."""
    hs, inp = hidden + 4, 16 * ((in_dim + 15) // 16) + 4
    x = 16 * inp if out_dim <= 8 else max(16 * inp, 2 * 16 * WIDE_OUT)
    floats = 208 + (depth + 1) * hidden + 8 * hidden + x + depth * 16 * hs + 2 * 16 * hs + 2 * 16 * 16
    return (floats * 4 + 15) // 16 * 16 + 8 * 2 * 16 * 36 * 4


def case(E, Ia, depth, act, head, seed, bounds=False, **kw):
    """policy_step_cases.case at the wide pair, the critic on 8 inputs at the actor's depth.  bounds "pm04": -0.4 / +0.4 on
    every dimension (humanoid's distribution_min / max) in place of the module's per-dimension bounds."""
    c = cases.case(E, PAIR, Ia, 8, depth, depth, act, head, seed, bounds=bool(bounds), **kw)
    c["pm04"] = bounds == "pm04"
    return c


# one combination per new piece (E in {1, 15, 17, 33}, depth 1 and 3, 8 and 376 inputs, bounds, saturate, floor)
CASES = {
    "cat9_e1_d1_in8": case(1, 8, 1, "relu", (CAT, 9), 31),                              # the first wide head; one row
    "cat18_e33_d3_in376": case(33, 376, 3, "leaky_relu", (CAT, 18), 32),                # mario_bros_ram's head, a third tile
    "cat24_sat_e17_d3_in8": case(17, 8, 3, "tanh", (CAT, 24), 33, saturate=10.0),       # the cap; classes below eps32
    "gau9_e15_d1_in8": case(15, 8, 1, "relu", (GAU, 9), 34, bounds=True),               # a third Philox block with one component
    "gau16_e17_d3_in8": case(17, 8, 3, "tanh", (GAU, 16), 35),                          # a full fourth Philox block
    "gau17_e33_d3_in376": case(33, 376, 3, "tanh", (GAU, 17), 36, bounds="pm04"),       # humanoid: a fifth block, one component
    "gau24_floor_e17_d3_in8": case(17, 8, 3, "leaky_relu", (GAU, 24), 37, bounds=True, floor=True),   # the cap
}
for _i, _c in enumerate(CASES.values()):
    _c["norm_values"] = bool(_i & 1)
BLOCK_CASE = case(32, 8, 3, "relu", (GAU, 17), 38, bounds="pm04")                       # the block form: 2 blocks of 16 rows
BLOCK_CASE["norm_values"] = False


@functools.lru_cache(maxsize=None)
def steering(name):
    """policy_step_cases.Steering of a case of this module (its bounds rule replaced for a "pm04" case)."""
    c = BLOCK_CASE if name == "block" else CASES[name]
    if not c["pm04"]:
        return cases.Steering(c)
    keep = cases.bounds_of
    cases.bounds_of = lambda out_dim: (np.full(out_dim, -0.4, np.float32), np.full(out_dim, 0.4, np.float32))
    try:
        return cases.Steering(c)
    finally:
        cases.bounds_of = keep
