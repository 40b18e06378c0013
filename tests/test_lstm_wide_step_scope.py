"""
CPU tests (no launch) of K21 at LSTM hidden size 256 (csrc/lstm_wide_step.hip): the opt-in `fused_lstm_wide_step`, honoured
only beside `fused_lstm_wide`, what `_lstm_step_scope` and the verbose hint answer with and without it, and what the
library's host checks take and refuse at that width.  The two-layer entry points and K22 keep refusing 256.
"""
import ctypes as C
import types

import pytest
import torch

from ppo_and_friends_amd import kernels as K
from ppo_and_friends_amd.fused_update import FusedLstmUpdate
from ppo_and_friends_amd.networks.distributions import CategoricalDistribution
from ppo_and_friends_amd.networks.lstm import LSTMNetwork
from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy

TODAY = "LSTM hidden size 256: K21 covers 32, 64, 128; forward_logits on K18 steps the policy"
HINT = "; PPOPolicy.fused_lstm_wide_step = True would step it in one launch (K21 at 256)"


@pytest.fixture(scope="module", autouse=True)
def _library():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)


def _policy(**flags):
    kw = dict(sequence_length=10, lstm_hidden_size=256, ff_hidden_size=128)
    actor, critic = LSTMNetwork(4, 2, name="actor", **kw), LSTMNetwork(4, 1, name="critic", **kw)
    actor.distribution = CategoricalDistribution()
    for net in (actor, critic):
        net.flatten_parameters_(torch.device("cpu"))
        net.use_hip = True
    pol = types.SimpleNamespace(using_lstm=True, agent_grouping=False, actor=actor, critic=critic, enable_icm=False,
                                policy_params=actor.flat_params, **flags)
    pol.lstm_step_unsupported_reason = lambda: PPOPolicy._lstm_step_scope(pol)
    return pol


@pytest.mark.parametrize("wide,step", [(False, False), (True, False), (False, True), (True, True)])
def test_scope_and_hint_per_flag_pair(wide, step):
    assert PPOPolicy.fused_lstm_wide_step is False
    pol = _policy(fused_lstm_wide=wide, fused_lstm_wide_step=step)
    why = PPOPolicy._lstm_step_scope(pol)
    if wide and step:
        assert why == ""
    elif wide:
        assert why == TODAY
    else:                                                     # K18 itself does not take the width
        assert why == "actor: LSTM hidden size 256 is not one of 32, 64, 128"
    assert PPOPolicy.lstm_step_hint(pol) == (HINT if wide and not step else "")
    assert PPOPolicy._lstm_step_scope(_policy()) == "actor: LSTM hidden size 256 is not one of 32, 64, 128"


def _args(mode, hidden=256):
    from ppo_and_friends_amd import _lib
    a = _lib.LstmPolicyStepArgs()
    for d in (a.actor, a.critic):
        d.in_dim, d.hidden, d.ff_hidden, d.ff_depth, d.out_dim, d.activation = 5, hidden, 16, 1, 1, 0
        d.rows, d.steps, d.params = 4, 1, 0x10000
    a.actor.out_dim, a.E, a.mode = 3, 4, mode
    for f in ("obs", "critic_obs", "actor_h", "actor_c", "critic_h", "critic_c", "raw_action_out", "action_out", "logp_out",
              "value_out", "actor_hidden_out", "actor_cell_out", "critic_hidden_out", "critic_cell_out", "commit", "terminated",
              "boot_value_out"):
        setattr(a, f, 0x10000)
    return a


def _table():
    from ppo_and_friends_amd import _lib
    tb = _lib.LstmStepBlocks()
    tb.n_blocks, tb.rows_per_block = 2, 2
    for b in range(2):
        tb.obs[b] = tb.critic_obs[b] = tb.env_action[b] = 0x10000
    return tb


@pytest.mark.parametrize("mode", range(4))
def test_the_library_takes_256_in_every_mode(mode):
    assert K.lstm_policy_step_refusal(_args(mode)) == ""
    why = K.lstm_policy_step_blocks_refusal(_args(mode), _table())
    assert why == "" if mode < 2 else "INFER and MASK have no block form" in why, why


@pytest.mark.parametrize("needle,fields", [
    ("hidden 48 not in {32, 64, 128}", dict(actor__hidden=48, critic__hidden=48)),
    ("LSTM hidden sizes differ (actor 256, critic 128)", dict(critic__hidden=128)),
    ("in_dim 257 not in [1, 256]", dict(actor__in_dim=257)),
    ("critic out_dim must be 1", dict(critic__out_dim=2))])
def test_both_forms_keep_their_refusals(needle, fields):
    a = _args(0)
    for k, v in fields.items():
        obj, _, f = k.rpartition("__")
        setattr(getattr(a, obj), f, v)
    assert needle in K.lstm_policy_step_refusal(a)
    assert needle in K.lstm_policy_step_blocks_refusal(a, _table())


def test_no_row_launches_nothing_and_the_other_kernels_keep_refusing_256():
    from ppo_and_friends_amd import _lib
    a = _args(0)
    a.E = 0
    assert _lib.load().ppoaf_lstm_policy_step(C.byref(a), None) == 0
    shape = dict(in_dim=4, ff_hidden=128, ff_depth=1, out_dim=2, activation=K.ACT_RELU, rows=33, steps=10, params=0x10000)
    two = _lib.Lstm2Desc(hidden=256, state_row_stride=256, state_layer_stride=33 * 256, **shape)
    assert "hidden 256 not in {32, 64, 128}" in K.lstm2_refusal(two)
    pol = _policy(fused_lstm_wide=True, fused_lstm_wide_step=True)
    assert FusedLstmUpdate.unsupported_reason(pol, 8).startswith("LSTM hidden size 256: K22 covers 32, 64, 128")
