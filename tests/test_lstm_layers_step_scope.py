"""
CPU tests (no launch) of K21 for two stacked LSTM layers: the opt-in `fused_lstm_layers_step` and what `_lstm_step_scope`
answers with it, ppoaf_lstm2_policy_step_args_t against _lib.Lstm2PolicyStepArgs, and the host check's refusals.
"""
import ctypes as C
import os
import re
import types

import pytest
import torch

from ppo_and_friends_amd.networks.distributions import CategoricalDistribution
from ppo_and_friends_amd.networks.lstm import LSTMNetwork
from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(layers=(2, 2), widths=(32, 32), step=True, icm=False):
    nets = [LSTMNetwork(5, out, sequence_length=5, lstm_hidden_size=h, num_lstm_layers=n, ff_hidden_size=16, name=tag)
            for tag, out, n, h in (("actor", 3, layers[0], widths[0]), ("critic", 1, layers[1], widths[1]))]
    for net in nets:
        net.flatten_parameters_(torch.device("cpu"))
        net.use_hip = True
    nets[0].distribution = CategoricalDistribution()
    return types.SimpleNamespace(using_lstm=True, agent_grouping=False, actor=nets[0], critic=nets[1], fused_lstm_layers=True,
                                 fused_lstm_layers_step=step, enable_icm=icm, policy_params=nets[0].flat_params)


@pytest.mark.parametrize("kw,needle", [(dict(), ""), (dict(step=False), "2 LSTM layers: K21 covers one"),
                                       (dict(layers=(1, 2)), "layer counts differ (actor 1, critic 2)"),
                                       (dict(layers=(3, 3)), "3 LSTM layers (K18 covers one or two)"),
                                       (dict(widths=(32, 64)), "LSTM hidden sizes differ (actor 32, critic 64)"),
                                       (dict(icm=True), "ICM policies keep today's route")])
def test_scope_with_the_opt_in(kw, needle):
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    assert PPOPolicy.fused_lstm_layers_step is False
    why = PPOPolicy._lstm_step_scope(_policy(**kw))
    assert why == "" if not needle else needle in why, why


def _args(mode=2):
    from ppo_and_friends_amd import _lib
    a = _lib.Lstm2PolicyStepArgs()
    for d in (a.actor, a.critic):
        d.in_dim, d.hidden, d.ff_hidden, d.ff_depth, d.out_dim, d.activation = 5, 32, 16, 1, 1, 0
        d.rows, d.steps, d.params, d.state_row_stride, d.state_layer_stride = 4, 1, 0x10000, 32, 4 * 32
    a.actor.out_dim, a.E, a.mode, a.stored_row_stride, a.stored_layer_stride = 3, 4, mode, 64, 32
    for f in ("obs", "critic_obs", "actor_h", "actor_c", "critic_h", "critic_c", "raw_action_out", "action_out", "logp_out",
              "value_out", "actor_hidden_out", "actor_cell_out", "critic_hidden_out", "critic_cell_out", "commit", "terminated",
              "boot_value_out"):
        setattr(a, f, 0x10000)
    return a


def test_layout_and_host_refusals():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib, kernels as K
    text = open(os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "lstm_stacked_step.hip")).read()
    listed = re.findall(r"PPOAF_LAYOUT\(ppoaf_lstm2_policy_step_args_t,\s*(\w+),\s*(\d+)\)", text)
    assert [f for f, _ in listed] == [f for f, _ in _lib.Lstm2PolicyStepArgs._fields_]
    for field, off in listed:
        assert getattr(_lib.Lstm2PolicyStepArgs, field).offset == int(off), field
    assert C.sizeof(_lib.Lstm2PolicyStepArgs) == 440
    for mode in range(4):
        assert K.lstm_policy_step_refusal(_args(mode)) == "", mode

    def refused(needle, mode=0, blocks=None, **fields):
        a = _args(mode)
        for k, v in fields.items():
            obj, _, f = k.rpartition("__")
            setattr(getattr(a, obj) if obj else a, f, v)
        why = K.lstm_policy_step_refusal(a) if blocks is None else K.lstm_policy_step_blocks_refusal(a, blocks)
        assert why.startswith("lstm2_policy_step") and needle in why, why

    refused("state strides", actor__state_layer_stride=48)
    refused("state strides", critic__state_layer_stride=5 * 32)              # [2, E, H] of another E
    refused("stored strides", stored_row_stride=32)
    refused("mode=4", mode=4)
    refused("STEP: null observation / state pointer", actor_c=None)
    refused("STEP needs the row-t outputs", critic_cell_out=None)
    refused("CRITIC_NEXT: null", mode=1, commit=None)
    refused("INFER: null", mode=2, action_out=None)
    refused("MASK needs terminated", mode=3, terminated=None)
    refused("LSTM hidden sizes differ (actor 32, critic 64)", critic__hidden=64, critic__state_row_stride=64,
            critic__state_layer_stride=4 * 64)
    tb = _lib.LstmStepBlocks()
    tb.n_blocks, tb.rows_per_block = 2, 2
    for b in range(2):
        tb.obs[b] = tb.critic_obs[b] = tb.env_action[b] = 0x10000
    assert K.lstm_policy_step_blocks_refusal(_args(0), tb) == ""
    refused("INFER and MASK have no block form", mode=2, blocks=tb)
    tb.n_blocks = 17
    refused("n_blocks=17 not in [1, 16]", blocks=tb)
    tb.n_blocks = 0
    refused("n_blocks=0 not in [1, 16]", blocks=tb)
