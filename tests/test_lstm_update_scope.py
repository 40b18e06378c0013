"""
Host logic of K22's coverage (csrc/lstm_update.hip), without a GPU and without a launch: which LSTM policies
FusedLstmUpdate takes, the reason it gives for the others, and what the library's own host-only check refuses.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch.nn as nn


@pytest.fixture(scope="module", autouse=True)
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)


def _net(obs, n_out, name, H=32, F=16, S=5, act=None, layers=1, depth=1):
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    return LSTMNetwork(obs, n_out, name=name, sequence_length=S, lstm_hidden_size=H, ff_hidden_size=F, ff_hidden_depth=depth,
                       num_lstm_layers=layers, activation=act if act is not None else nn.ReLU())


def _policy(obs=4, n_out=2, gaussian=False, critic=None, **kw):
    from ppo_and_friends_amd.networks.distributions import CategoricalDistribution, GaussianDistribution
    actor = _net(obs, n_out, "actor", **kw)
    critic = _net(obs, 1, "critic", **dict(kw, **(critic or {})))
    actor.distribution = GaussianDistribution(n_out) if gaussian else CategoricalDistribution()
    for net in (actor, critic):
        net.flatten_parameters_("cpu")
    return SimpleNamespace(using_lstm=True, agent_grouping=False, actor=actor, critic=critic)


def _reason(B=256, **kw):
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    return FusedLstmUpdate.unsupported_reason(_policy(**kw), B)


def test_the_two_baseline_shapes_are_covered():
    # cart_pole_lstm: 4 observations, Discrete(2), H 32, ff 16, S 5, LeakyReLU
    assert _reason(obs=4, n_out=2, H=32, F=16, S=5, act=nn.LeakyReLU()) == ""
    # the reference's LSTMNetwork defaults: H 128, ff 128, S 10, ReLU; a Box(6) action
    assert _reason(obs=17, n_out=6, gaussian=True, H=128, F=128, S=10) == ""
    # the LDS maximum: H 128, S 16, F 128, depth 2; the feed-forward heads may differ between the networks
    assert _reason(obs=256, n_out=8, H=128, F=128, S=16, depth=2, critic=dict(F=16, depth=1)) == ""
    assert _reason(B=2) == ""


@pytest.mark.parametrize("kw,needle", [
    (dict(layers=2), "2 LSTM layers"),
    (dict(H=96), "hidden size 96"),
    (dict(S=32), "sequence length 32"),
    (dict(n_out=9), "output width 9"),
    (dict(F=48), "feed-forward width 48"),
    (dict(depth=3), "1 or 2 hidden layers"),
    (dict(obs=300), "input width 300"),
    (dict(act=nn.ELU()), "activation"),
    (dict(B=1), "batch size < 2"),
])
def test_uncovered_shapes_give_a_reason_naming_them(kw, needle):
    why = _reason(**kw)
    assert needle in why, why


def test_unequal_hidden_sizes_say_so():
    why = _reason(H=32, critic=dict(H=64))
    assert "hidden sizes differ" in why and "actor 32" in why and "critic 64" in why, why
    assert "sequence lengths differ" in _reason(S=4, critic=dict(S=5))


def test_the_library_check_is_part_of_the_answer(monkeypatch):
    from ppo_and_friends_amd import kernels as K
    monkeypatch.setattr(K, "lstm_update_refusal", lambda a, pointers=False: "lstm_update: refused for the test")
    assert _reason() == "lstm_update: refused for the test"


def test_the_policy_switch_exists_and_defaults_to_on():
    import numpy as np
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.spaces import Box, Discrete
    sp = Box(-np.inf, np.inf, (4,), np.float32)
    ppo = PPO(lambda: SyntheticFixedLengthEnv(4, 4, Discrete(2), 40, "cpu"),
              {"p": (None, sp, sp, Discrete(2), dict(ac_network=LSTMNetwork))}, device="cpu", envs_per_proc=4,
              ts_per_rollout=8, update_mode="fused", save_state=False)
    assert ppo.policies["p"].fused_lstm_update is True
    assert ppo._fused_updater("p", 4) is None            # a host policy: no fused driver at all


# ---- ppoaf_lstm_update_check: every bad field is refused with a message naming it (host only: PTR is never followed)
PTR = 0x10000


def _args(**over):
    from ppo_and_friends_amd import _lib
    a = _lib.LstmUpdateArgs()
    H, I, F, O, S, B = 64, 5, 32, 3, 4, 32
    pad4 = lambda n: (n + 3) // 4 * 4
    size = lambda i, o: (pad4(4 * H * i) + pad4(4 * H * H) + 2 * pad4(4 * H) + 2 * pad4(H) + pad4(F * H) + pad4(F)
                         + pad4(o * F) + pad4(o))
    na, nc = size(I, O), size(I, 1)
    for d, o in ((a.actor, O), (a.critic, 1)):
        d.in_dim, d.hidden, d.ff_hidden, d.ff_depth, d.out_dim, d.activation, d.rows, d.steps = I, H, F, 1, o, 0, B, S
    a.params = a.grads = a.exp_avg = a.exp_avg_sq = PTR
    a.actor.params = a.actor.grads = PTR
    a.critic.params = a.critic.grads = PTR + 4 * na
    a.bucket_total, a.actor_size, a.log_std_offset = na + nc, na, -1
    a.B = a.batch_stride = B
    a.n_rows, a.n_items, a.n_ranks = 120, 117, 1
    for f in ("step_counts", "lr", "norm_scratch", "obs", "critic_obs", "terminal", "perm", "row_map", "raw_actions",
              "advantages", "old_log_probs", "rewards_to_go", "values", "actor_hidden", "actor_cell", "critic_hidden",
              "critic_cell", "cursor", "vn_mean", "vn_var", "vn_count", "vn_records", "adv_records", "loss_partials",
              "totals", "workspace"):
        setattr(a, f, PTR)
    a.workspace_floats = a.norm_scratch_doubles = 1 << 30
    for k, v in over.items():
        obj, _, field = k.rpartition("__")
        setattr(getattr(a, obj) if obj else a, field, v)
    return a


def _check(a, pointers=True):
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    rc = lib.ppoaf_lstm_update_check(None if a is None else C.byref(a), 1 if pointers else 0)
    return rc, lib.ppoaf_last_error().decode()


def test_a_complete_argument_block_is_accepted():
    rc, msg = _check(_args())
    assert rc == 0, msg
    rc, msg = _check(_args(normalize_values=1, normalize_adv=1, use_huber=1))
    assert rc == 0, msg


@pytest.mark.parametrize("over,needle", [
    (dict(actor__hidden=48), "actor: hidden 48"),
    (dict(critic__hidden=128), "hidden sizes differ (actor 64, critic 128)"),
    (dict(actor__ff_hidden=48), "actor: ff_hidden 48"),
    (dict(critic__ff_depth=3), "critic: ff_depth 3"),
    (dict(actor__in_dim=257), "actor: in_dim 257"),
    (dict(actor__out_dim=9), "actor: out_dim 9"),
    (dict(critic__out_dim=2), "critic out_dim must be 1"),
    (dict(actor__steps=17, critic__steps=17), "steps 17"),
    (dict(critic__steps=5), "steps differ"),
    (dict(actor__activation=7), "activation 7"),
    (dict(head_kind=2), "head_kind=2"),
    (dict(B=1), "B=1"),
    (dict(batch_stride=16), "batch_stride=16"),
])
def test_bad_shapes_are_refused_by_name(over, needle):
    for pointers in (False, True):
        rc, msg = _check(_args(**over), pointers)
        assert rc != 0 and needle in msg, msg


@pytest.mark.parametrize("over,needle", [
    (dict(exp_avg=None), "exp_avg"),
    (dict(log_std_offset=0), "log_std_offset=0"),
    (dict(head_kind=1), "log_std_offset=-1"),
    (dict(actor_size=8), "actor_size=8"),
    (dict(bucket_total=8), "bucket_total=8"),
    (dict(critic__params=PTR), "critic.params"),
    (dict(actor__grads=PTR + 16), "actor.grads"),
    (dict(lr=None), "lr"),
    (dict(row_map=None), "row_map"),
    (dict(terminal=None), "terminal is NULL with steps > 1"),
    (dict(n_rows=2), "n_rows=2"),
    (dict(n_items=118), "n_items=118"),
    (dict(values=None), "values"),
    (dict(critic_cell=None), "hidden-state table"),
    (dict(cursor=None), "cursor"),
    (dict(normalize_values=1, vn_records=None), "vn_records missing"),
    (dict(normalize_adv=1, adv_records=None), "adv_records missing"),
    (dict(workspace_floats=16), "workspace holds 16 floats"),
])
def test_bad_pointers_and_sizes_are_refused_by_name(over, needle):
    rc, msg = _check(_args(**over))
    assert rc != 0 and needle in msg, msg
    from ppo_and_friends_amd import _lib
    lib = _lib.load()
    for entry in (lib.ppoaf_lstm_update_fwd_bwd, lib.ppoaf_lstm_update_wgrad):      # the launching entry points check first
        assert entry(C.byref(_args(**over)), None) != 0
        assert needle in lib.ppoaf_last_error().decode()


def test_null_args_and_the_sizes_query():
    rc, msg = _check(None)
    assert rc != 0 and "null args" in msg
    from ppo_and_friends_amd import kernels as K
    floats, doubles, lds = K.lstm_update_sizes(_args())
    assert floats > 0 and doubles > 2
    # forward (x and h buffers) + backward (two dgates buffers) + the head's arrays fit a workgroup's LDS at the widest shape
    assert lds < 160 * 1024
    _, _, lds128 = K.lstm_update_sizes(_args(actor__hidden=128, critic__hidden=128, actor__ff_hidden=128, actor__ff_depth=2,
                                             actor__steps=16, critic__steps=16))
    assert lds < lds128 <= 160 * 1024
    assert lds128 >= 4 * 2 * 16 * (4 * 128 + 4)
