"""
CPU tests (no launch) of the scope of two-layer LSTM policies under the opt-in `fused_lstm_layers` (K18 takes 2 / 2 layers;
K21, K22 and other stacks refuse), of the two-layer bucket-layout check and of ppoaf_lstm2_desc_t against _lib.Lstm2Desc.
"""
import ctypes as C
import os
import re
import types

import pytest
import torch

from ppo_and_friends_amd.fused_update import FusedLstm, FusedLstmUpdate
from ppo_and_friends_amd.networks.distributions import CategoricalDistribution
from ppo_and_friends_amd.networks.lstm import LSTMNetwork
from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(layers=(2, 2), opt_in=True):
    nets = [LSTMNetwork(5, out, sequence_length=5, lstm_hidden_size=32, num_lstm_layers=n, ff_hidden_size=16, name=tag)
            for tag, out, n in (("actor", 3, layers[0]), ("critic", 1, layers[1]))]
    nets[0].distribution = CategoricalDistribution()
    return types.SimpleNamespace(using_lstm=True, agent_grouping=False, actor=nets[0], critic=nets[1],
                                 fused_lstm_layers=opt_in, enable_icm=False)


def test_two_layers_are_taken_with_the_opt_in_only():
    assert FusedLstm.unsupported_reason(_policy()) == ""
    assert FusedLstm.unsupported_reason(_policy(opt_in=False)) == "actor: 2 LSTM layers (K18 covers one)"
    assert "fused_lstm_layers" in FusedLstm.layers_hint(_policy(opt_in=False))
    assert FusedLstm.layers_hint(_policy()) == "" and FusedLstm.layers_hint(_policy((3, 3), opt_in=False)) == ""
    assert PPOPolicy.fused_lstm_layers is False


@pytest.mark.parametrize("layers,needle", [((1, 2), "layer counts differ (actor 1, critic 2)"), ((2, 1), "layer counts differ"),
                                           ((3, 3), "3 LSTM layers (K18 covers one or two)")])
def test_other_stacks_are_refused(layers, needle):
    assert needle in FusedLstm.unsupported_reason(_policy(layers))


def test_k21_and_k22_refuse_two_layers_with_their_own_reason():
    pol = _policy()
    why = FusedLstmUpdate.unsupported_reason(pol, 32)
    assert why.startswith("2 LSTM layers: K22 covers one")
    why = PPOPolicy._lstm_step_scope(pol)
    assert why.startswith("2 LSTM layers: K21 covers one")


def test_layout_check_catches_a_reallocated_second_layer_weight():
    net = LSTMNetwork(5, 3, sequence_length=5, lstm_hidden_size=32, num_lstm_layers=2, ff_hidden_size=16, name="net")
    net.flatten_parameters_(torch.device("cpu"))
    assert net._hip_scope(max_layers=2) == ""
    net.lstm.weight_ih_l1.data = net.lstm.weight_ih_l1.data.clone()
    assert net._hip_scope(max_layers=2) == "parameter layout differs from the kernel's"


def test_descriptor_layout_and_host_check():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib, kernels as K
    text = open(os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "lstm_stacked.hip")).read()
    listed = re.findall(r"PPOAF_LAYOUT\(ppoaf_lstm2_desc_t,\s*(\w+),\s*(\d+)\)", text)
    assert [f for f, _ in listed] == [f for f, _ in _lib.Lstm2Desc._fields_]
    for field, off in listed:
        assert getattr(_lib.Lstm2Desc, field).offset == int(off), field
    assert C.sizeof(_lib.Lstm2Desc) == 88 and C.sizeof(_lib.LstmDesc) == 72
    d = _lib.Lstm2Desc(in_dim=5, hidden=32, ff_hidden=16, ff_depth=1, out_dim=3, activation=0, rows=4, steps=5, params=0x10000,
                       state_row_stride=32, state_layer_stride=128)
    assert K.lstm2_refusal(d) == ""
    d.state_row_stride, d.state_layer_stride = 64, 32                   # [rows, 2, H]
    assert K.lstm2_refusal(d) == ""
    d.state_layer_stride = 48
    assert "state strides" in K.lstm2_refusal(d)
    d.state_layer_stride, d.hidden = 32, 48
    assert "hidden 48 not in {32, 64, 128}" in K.lstm2_refusal(d)
    d.hidden, d.steps = 32, 17
    assert "steps 17 not in [1, 16]" in K.lstm2_refusal(d)
    d.steps = 5
    assert "workspace holds 0 floats" in K.lstm2_refusal(d, need_workspace=True)
