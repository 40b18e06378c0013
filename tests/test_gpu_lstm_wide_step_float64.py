"""
-m gpu: ONE launch of K21 at LSTM hidden size 256 (csrc/lstm_wide_step.hip, 32-row tiles) against float64: the test bodies,
launch plumbing and judge of tests/test_gpu_lstm_step_float64.py as they stand (every launch of lstm_step_cases.LAUNCHES and
MASK; bound k12_bound, sentinels, bitwise rules: see there), run over this kernel's shape edges -- 1 / 17 / 32 / 33 rows, tile
4 alone in the second group of eight workgroups (E 129), tile 8 in the third with one live row (E 257), in_dim at the chunk
edges and at 256, F 16 .. 128.  Then: the states after STEP are bitwise ppoaf_lstm_forward's at S = 1, and the block form is
bitwise the tensor form (E = 65 as 13 x 5, E = 129 as 43 x 3 blocks).  `cases.steering` is a lookup by name into the
helper's own table; pytest's monkeypatch points it at CASES below for the length of a test.

Measured on the MI355X, worst deviation / bound over all launches per case (no row left out anywhere): w_e1_cat2 0.093
values, w_e17_gau1_bounds 0.236 logp (forced), w_e32_wrap_cat8 0.063 critic_h, w_e33_gau5 0.098 critic_h (chain),
w_e65_cat3 0.048 critic_h, w_e129_gau8_bounds 0.093 logp (forced), w_e257_cat5 0.067 actor_h, w_small_h_cat3 0.150 values.
"""
import functools

import pytest
import torch

import test_gpu_lstm_step_float64 as k21
from test_gpu_lstm_step_float64 import _bits, cases

pytestmark = pytest.mark.gpu
CAT, GAU = cases.CAT, cases.GAU
CASES = {
    "w_e1_cat2": cases.case(1, 256, 16, 128, 1, 2, 1, 15, "relu", (CAT, 2), 101),
    "w_e17_gau1_bounds": cases.case(17, 256, 128, 16, 2, 1, 17, 1, "tanh", (GAU, 1), 102, bounds=True),
    "w_e32_wrap_cat8": cases.case(32, 256, 64, 32, 1, 1, 16, 256, "leaky_relu", (CAT, 8), 103, offset=2 ** 32 - 5),
    "w_e33_gau5": cases.case(33, 256, 32, 64, 2, 2, 256, 255, "relu", (GAU, 5), 104),
    "w_e65_cat3": cases.case(65, 256, 16, 128, 1, 2, 9, 12, "tanh", (CAT, 3), 105),
    "w_e129_gau8_bounds": cases.case(129, 256, 128, 16, 1, 2, 5, 7, "leaky_relu", (GAU, 8), 106, bounds=True),
    "w_e257_cat5": cases.case(257, 256, 32, 32, 1, 1, 255, 17, "relu", (CAT, 5), 107),
    "w_small_h_cat3": cases.case(17, 256, 16, 32, 1, 1, 6, 9, "relu", (CAT, 3), 108, small_h=True),
}
for _i, _c in enumerate(CASES.values()):
    _c["norm_values"] = bool(_i & 1)
_steering = functools.lru_cache(maxsize=None)(lambda name: cases.Steering(CASES[name]))


@pytest.fixture(autouse=True)
def _wide_cases(monkeypatch):
    monkeypatch.setattr(cases, "steering", _steering)


@pytest.mark.parametrize("name", list(CASES))
def test_k21_wide_launches_against_float64(name):
    k21.test_k21_step_against_float64(name)
    k21.test_k21_critic_next_infer_and_mask_against_float64(name)


@pytest.mark.parametrize("name", list(CASES))
def test_stepped_states_are_bitwise_k18s_at_one_step(name):
    d = k21.Device(name)
    res, state = d.launch(k21.STEP), d.fresh_state()
    for i, (net, x) in enumerate((("actor", d.obs[0]), ("critic", d.cobs[0]))):
        h0, c0 = state[2 * i][:d.E].contiguous(), state[2 * i + 1][:d.E].contiguous()
        _, hn, cn = d.K.lstm_forward(d.desc[net], x.view(d.E, 1, -1), h0, c0, stash=False)
        torch.cuda.synchronize()
        assert torch.equal(_bits(res[f"{net}_h"]), _bits(hn)), f"{name}: {net} h is not ppoaf_lstm_forward's"
        assert torch.equal(_bits(res[f"{net}_c"]), _bits(cn)), f"{name}: {net} c is not ppoaf_lstm_forward's"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["E"] in (65, 129)])
def test_wide_block_form_is_the_tensor_form(name):
    k21.test_block_form_beyond_four_tiles_is_the_tensor_form(name)
