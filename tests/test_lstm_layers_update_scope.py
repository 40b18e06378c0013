"""
CPU tests (no launch) of the scope of K22 for two stacked LSTM layers (csrc/lstm_stacked_update.hip) under the opt-in
`fused_lstm_layers_update`, of its sizes call and of ppoaf_lstm2_update_args_t against _lib.Lstm2UpdateArgs.
"""
import types

import pytest

from ppo_and_friends_amd.fused_update import FusedLstmUpdate, _describe_lstm_update
from ppo_and_friends_amd.networks.distributions import CategoricalDistribution
from ppo_and_friends_amd.networks.lstm import LSTMNetwork
from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
from ppo_and_friends_amd.utils import mpi_utils


def _policy(update=True, layers_opt=True, H=(32, 32), S=(5, 5)):
    nets = [LSTMNetwork(5, out, sequence_length=s, lstm_hidden_size=h, num_lstm_layers=2, ff_hidden_size=16, name=tag)
            for tag, out, h, s in (("actor", 3, H[0], S[0]), ("critic", 1, H[1], S[1]))]
    nets[0].distribution = CategoricalDistribution()
    return types.SimpleNamespace(using_lstm=True, agent_grouping=False, actor=nets[0], critic=nets[1], enable_icm=False,
                                 fused_lstm_layers=layers_opt, fused_lstm_layers_update=update)


@pytest.fixture(scope="module", autouse=True)
def _library():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)


def test_opt_in_off_keeps_the_refusal_and_on_takes_the_policy():
    parent = "2 LSTM layers: K22 covers one; the mini-batch loop on K18 trains it"
    assert PPOPolicy.fused_lstm_layers_update is False
    assert FusedLstmUpdate.unsupported_reason(_policy(update=False), 32) == parent
    assert FusedLstmUpdate.unsupported_reason(_policy(layers_opt=False), 32) == "actor: 2 LSTM layers (K18 covers one)"
    assert FusedLstmUpdate.unsupported_reason(_policy(), 32) == ""


@pytest.mark.parametrize("kw,B,needle", [(dict(H=(32, 64)), 32, "LSTM hidden sizes differ (actor 32, critic 64)"),
                                         (dict(S=(5, 4)), 32, "sequence lengths differ (actor 5, critic 4)"),
                                         (dict(), 1, "batch size < 2")])
def test_each_refusal_has_its_own_words(kw, B, needle):
    assert needle in FusedLstmUpdate.unsupported_reason(_policy(**kw), B)


def test_more_than_one_rank_keeps_the_loop(monkeypatch):
    monkeypatch.setattr(mpi_utils, "get_num_procs", lambda: 2)
    monkeypatch.setattr(mpi_utils, "distributed_path", lambda: True)        # what FusedEpoch.multi reads
    why = FusedLstmUpdate.unsupported_reason(_policy(), 32)
    assert "2 LSTM layers on the multi-rank path (2 ranks)" in why and "mini-batch loop" in why


@pytest.mark.parametrize("H", [32, 64, 128])
def test_sizes_and_the_last_field_of_the_argument_struct(H):
    from ppo_and_friends_amd import kernels as K
    a = _describe_lstm_update(_policy(H=(H, H)), 33, layers=2)
    na = 4 * H * 5 + 3 * 4 * H * H + 16 * H + 2 * H + 16 * H + 16 + 3 * 16 + 4        # the actor's two-layer bucket, padded
    nc = na - (3 * 16 + 4) + 16 + 4
    a.bucket_total, a.actor_size = na + nc, na
    floats, doubles, lds = K.lstm_update_sizes(a)
    assert floats > 0 and doubles > 2 and 0 < lds <= 160 * 1024
    # every pointer set (never followed), sizes as the library's layout has them: only the workspace is one float short
    d = _describe_lstm_update(_policy(H=(H, H)), 33, layers=2)
    d.actor.state_row_stride = 0
    assert "state strides" in K.lstm_update_refusal(d)
    for name, kind in a._fields_[2:]:
        if kind.__name__ == "c_void_p":
            setattr(a, name, 0x100000)
    a.log_std_offset = -1
    a.actor.params = a.actor.grads = a.params
    a.critic.params = a.critic.grads = a.params + 4 * na
    a.n_rows, a.n_items, a.n_ranks = 64, 60, 1
    a.workspace_floats = floats - 1
    why = K.lstm_update_refusal(a, pointers=True)
    assert f"workspace holds {floats - 1} floats, {floats} needed" in why, why
    a.workspace_floats = floats
    assert K.lstm_update_refusal(a, pointers=True) == ""
