"""
CPU tests of K18's coverage at LSTM hidden size 256 (csrc/lstm_wide.hip): taken with the policy's opt-in `fused_lstm_wide`
only, one layer only, on K18 alone (K21 and K22 say why they do not take it).  No kernel is launched.
"""
from types import SimpleNamespace

import pytest

from ppo_and_friends_amd import kernels as K
from ppo_and_friends_amd.fused_update import FusedLstm, FusedLstmUpdate
from ppo_and_friends_amd.networks.distributions import CategoricalDistribution
from ppo_and_friends_amd.networks.lstm import LSTMNetwork
from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy

REFUSAL = "actor: LSTM hidden size 256 is not one of 32, 64, 128"


def _policy(wide, H=256, layers=1, **flags):
    kw = dict(sequence_length=10, lstm_hidden_size=H, ff_hidden_size=128, num_lstm_layers=layers)
    actor, critic = LSTMNetwork(4, 2, name="actor", **kw), LSTMNetwork(4, 1, name="critic", **kw)
    actor.distribution = CategoricalDistribution()
    for net in (actor, critic):
        net.flatten_parameters_("cpu")
    return SimpleNamespace(using_lstm=True, agent_grouping=False, actor=actor, critic=critic, fused_lstm_wide=wide, **flags)


def test_the_opt_in_is_off_by_default():
    assert PPOPolicy.fused_lstm_wide is False


@pytest.mark.parametrize("wide", [False, True])
def test_256_is_taken_with_the_opt_in_only(wide):
    pol = _policy(wide)
    assert FusedLstm.unsupported_reason(pol) == ("" if wide else REFUSAL)
    assert FusedLstm.unsupported_reason(pol, lstm_wide=True) == ""
    assert FusedLstm.unsupported_reason(pol, lstm_wide=False) == REFUSAL
    assert ("fused_lstm_wide = True would take it on K18" in FusedLstm.layers_hint(pol)) == (not wide)
    assert pol.actor.hip_unsupported_reason() == REFUSAL[len("actor: "):]


@pytest.mark.parametrize("wide", [False, True])
def test_other_widths_and_two_layers_at_256_stay_refused(wide):
    assert "hidden size 96 is not one of 32, 64, 128" in FusedLstm.unsupported_reason(_policy(wide, H=96))
    assert FusedLstm.wide_hint(_policy(wide, H=96)) == ""
    assert FusedLstm.unsupported_reason(_policy(wide, H=128)) == ""
    assert "2 LSTM layers (K18 covers one)" in FusedLstm.unsupported_reason(_policy(wide, layers=2))
    why = FusedLstm.unsupported_reason(_policy(wide, layers=2, fused_lstm_layers=True))
    assert ("the stacked kernels cover 32, 64, 128" if wide else "hidden size 256 is not one of 32, 64, 128") in why
    assert FusedLstm.layers_hint(_policy(wide, layers=2)) == ""


def test_k21_and_k22_say_why_they_leave_the_wide_policy_to_k18():
    pol = _policy(True)
    assert FusedLstmUpdate.unsupported_reason(pol, 8).startswith("LSTM hidden size 256: K22 covers 32, 64, 128")
    assert PPOPolicy._lstm_step_scope(pol).startswith("LSTM hidden size 256: K21 covers 32, 64, 128")


def test_the_library_takes_256_on_the_one_layer_entry_points_alone():
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    shape = dict(in_dim=4, ff_hidden=128, ff_depth=1, out_dim=2, activation=K.ACT_RELU, rows=33, steps=10, params=0x10000)
    n, size = K.lstm_sizes(_lib.LstmDesc(hidden=256, **shape))
    assert size == 4 * 256 * (4 + 256 + 2) + 2 * 256 + 128 * 256 + 128 + 2 * 128 + 4 and n > 2 * 33 * 10 * 4 * 256
    with pytest.raises(Exception, match="hidden 96 not in"):
        K.lstm_sizes(_lib.LstmDesc(hidden=96, **shape))
    two = _lib.Lstm2Desc(hidden=256, state_row_stride=256, state_layer_stride=33 * 256, **shape)
    assert "hidden 256 not in {32, 64, 128}" in K.lstm2_refusal(two)
