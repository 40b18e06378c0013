"""
CPU tests of the block form of K21 at the C boundary (no GPU, no launch): header <-> SIGNATURES <-> library for
ppoaf_lstm_policy_step_blocks / ppoaf_lstm_policy_step_blocks_check, the table's layout (ctypes against the static_assert
list in csrc/lstm_policy_step.hip), the ABI version, the refusals of the host-only check by value and by name, and the
opt-in's default.
"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppoaf_hip.h")
SOURCE = os.path.join(ROOT, "ppo_and_friends_amd", "csrc", "lstm_policy_step.hip")
ENTRY_POINTS = {"ppoaf_lstm_policy_step_blocks": 3, "ppoaf_lstm_policy_step_blocks_check": 2}
STEP, CRITIC_NEXT, INFER, MASK = 0, 1, 2, 3
PTR = 0x10000                                        # never dereferenced: nothing here launches
INVALID = -1                                         # PPOAF_E_INVALID (a failed launch is PPOAF_E_LAUNCH, -2)


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def test_header_signatures_and_library_agree(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = built.load()
    for name, want in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/ppoaf_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = built.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args == want
        assert hasattr(lib, name)
    assert lib.ppoaf_abi_version() == 7 and built.ABI_VERSION == 7


def test_every_header_function_has_its_ctypes_signature(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ppoaf_\w+)\s*\(", src))
    assert set(ENTRY_POINTS) <= declared
    assert declared <= set(built.SIGNATURES), declared - set(built.SIGNATURES)


def test_table_layout_matches_the_static_asserts(built):
    struct, cls = "ppoaf_lstm_step_blocks_t", built.LstmStepBlocks
    text = open(SOURCE).read()
    listed = re.findall(r"PPOAF_LAYOUT\(" + struct + r",\s*(\w+),\s*(\d+)\)", text)
    fields = [f for f, _ in cls._fields_]
    assert [f for f, _ in listed] == fields, "every field, in order"
    for field, off in listed:
        assert getattr(cls, field).offset == int(off), field
    size = re.search(r"static_assert\(sizeof\(" + struct + r"\)\s*==\s*(\d+)", text)
    assert size and C.sizeof(cls) == int(size.group(1))
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)).group(1)
    names = [re.sub(r"\[\w+\]", "", n.strip().lstrip("*")) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\**\s+", "", decl.strip()).split(",")]
    assert names == fields
    m = re.search(r"#define\s+PPOAF_ROW_BLOCKS_MAX\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == built.ROW_BLOCKS_MAX == len(cls().obs)


def test_the_existing_argument_struct_keeps_its_size(built):
    assert C.sizeof(built.LstmPolicyStepArgs) == 392


def _desc(built, hidden=32, ff=16, depth=1, in_dim=8, out_dim=5):
    return built.LstmDesc(in_dim=in_dim, hidden=hidden, ff_hidden=ff, ff_depth=depth, out_dim=out_dim, activation=0,
                          rows=30, steps=1, params=PTR)


def _args(built, mode=STEP, E=30, **over):
    a = built.LstmPolicyStepArgs()
    a.actor, a.critic = _desc(built), _desc(built, in_dim=10, out_dim=1)
    a.E, a.head_kind, a.mode, a.infer_mode = E, 0, mode, 1
    # obs / critic_obs stay NULL: the block form does not read them
    for f in ("actor_h", "actor_c", "critic_h", "critic_c", "commit", "boot_value_out", "raw_action_out", "action_out", "logp_out",
              "value_out", "actor_hidden_out", "actor_cell_out", "critic_hidden_out", "critic_cell_out"):
        setattr(a, f, PTR)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _table(built, n_blocks=3, rows=10, **over):
    t = built.LstmStepBlocks()
    t.n_blocks, t.rows_per_block = n_blocks, rows
    for b in range(max(0, min(n_blocks, built.ROW_BLOCKS_MAX))):
        t.obs[b], t.critic_obs[b], t.env_action[b] = PTR + 64 * b, 2 * PTR + 64 * b, 3 * PTR + 64 * b
    for k, (b, v) in over.items():
        getattr(t, k)[b] = v
    return t


def _refused(built, a, t, needle):
    lib = built.load()
    ref = lambda x: None if x is None else C.byref(x)
    assert lib.ppoaf_lstm_policy_step_blocks_check(ref(a), ref(t)) == INVALID
    msg = lib.ppoaf_last_error().decode()
    assert needle in msg, msg
    # the launching entry point runs the same check before any launch (there is no device here: a launch would fail
    # with another code and another message)
    assert lib.ppoaf_lstm_policy_step_blocks(ref(a), ref(t), None) == INVALID
    assert needle in lib.ppoaf_last_error().decode()


@pytest.mark.parametrize("mode", [STEP, CRITIC_NEXT])
@pytest.mark.parametrize("n_blocks,rows", [(3, 10), (2, 16), (16, 1), (3, 5), (1, 30)])
def test_a_covered_table_is_accepted(built, mode, n_blocks, rows):
    a, t = _args(built, mode, E=n_blocks * rows, terminated=PTR if mode == CRITIC_NEXT else None), _table(built, n_blocks, rows)
    assert built.load().ppoaf_lstm_policy_step_blocks_check(C.byref(a), C.byref(t)) == 0, built.load().ppoaf_last_error()


def test_critic_next_reads_the_critic_blocks_only(built):
    a, t = _args(built, CRITIC_NEXT), _table(built)
    for b in range(3):
        t.obs[b] = t.env_action[b] = None
    assert built.load().ppoaf_lstm_policy_step_blocks_check(C.byref(a), C.byref(t)) == 0, built.load().ppoaf_last_error()


def test_null_args(built):
    _refused(built, None, _table(built), "null args")
    _refused(built, _args(built), None, "null args")


@pytest.mark.parametrize("n_blocks", [0, 17, -1])
def test_block_count_outside_the_table(built, n_blocks):
    _refused(built, _args(built, E=n_blocks * 10), _table(built, n_blocks), f"n_blocks={n_blocks} not in [1, 16]")


def test_rows_that_do_not_fill_the_blocks(built):
    _refused(built, _args(built, E=31), _table(built), "E=31 is not n_blocks=3 x rows_per_block=10")
    _refused(built, _args(built, E=30), _table(built, 2, 10), "E=30 is not n_blocks=2 x rows_per_block=10")
    _refused(built, _args(built, E=-30), _table(built, 3, -10), "rows_per_block=-10 must be >= 0")


@pytest.mark.parametrize("mode,field,block", [(STEP, "obs", 0), (STEP, "critic_obs", 2), (STEP, "env_action", 1),
                                              (CRITIC_NEXT, "critic_obs", 1)])
def test_a_null_base(built, mode, field, block):
    _refused(built, _args(built, mode), _table(built, **{field: (block, None)}), f"block {block}: ")


@pytest.mark.parametrize("mode,head,field,base", [
    (STEP, 0, "obs", PTR + 2), (STEP, 0, "critic_obs", PTR + 1), (CRITIC_NEXT, 0, "critic_obs", PTR + 2),
    (STEP, 0, "env_action", PTR + 4),                     # int64 actions: 8 bytes
    (STEP, 1, "env_action", PTR + 2),                     # float32 actions: 4 bytes
])
def test_a_misaligned_base(built, mode, head, field, base):
    a = _args(built, mode, head_kind=head, log_std=PTR)
    _refused(built, a, _table(built, **{field: (1, base)}), "block 1: ")
    assert "not aligned" in built.load().ppoaf_last_error().decode()


def test_float_actions_need_four_bytes_only(built):
    a, t = _args(built, STEP, head_kind=1, log_std=PTR), _table(built, env_action=(1, PTR + 4))
    assert built.load().ppoaf_lstm_policy_step_blocks_check(C.byref(a), C.byref(t)) == 0, built.load().ppoaf_last_error()


@pytest.mark.parametrize("mode", [INFER, MASK, 4])
def test_modes_without_a_block_form(built, mode):
    _refused(built, _args(built, mode, terminated=PTR), _table(built), f"mode={mode}")


def test_what_the_tensor_form_refuses_is_refused_too(built):
    _refused(built, _args(built, STEP, actor_h=None), _table(built), "STEP: null observation / state pointer")
    _refused(built, _args(built, STEP, logp_out=None), _table(built), "STEP needs the row-t outputs")
    _refused(built, _args(built, CRITIC_NEXT, commit=None), _table(built), "CRITIC_NEXT")
    a = _args(built)
    a.critic = _desc(built, hidden=64, in_dim=10, out_dim=1)
    _refused(built, a, _table(built), "hidden sizes differ (actor 32, critic 64)")


@pytest.mark.parametrize("mode", [STEP, CRITIC_NEXT])
def test_no_rows_is_accepted_and_launches_nothing(built, mode):
    lib = built.load()
    a, t = _args(built, mode, E=0), _table(built, 3, 0)
    assert lib.ppoaf_lstm_policy_step_blocks_check(C.byref(a), C.byref(t)) == 0, lib.ppoaf_last_error()
    assert lib.ppoaf_lstm_policy_step_blocks(C.byref(a), C.byref(t), None) == 0      # (no device here: a launch would fail)


def test_the_opt_in_is_off_by_default():
    from ppo_and_friends_amd.ppo import PPO
    assert PPO.lstm_members is False
    assert PPO.step_row_blocks is True and PPO.finish_rows is True


def test_the_policy_names_what_its_table_cannot_take():
    """lstm_step_blocks_unsupported_reason, on host tensors: every answer is a refusal, by name."""
    import numpy as np
    import torch
    from ppo_and_friends_amd.networks.lstm import LSTMNetwork
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    assert callable(getattr(PPOPolicy, "lstm_step_blocks_unsupported_reason", None))
    from ppo_and_friends_amd.policies.utils import generate_policy
    from ppo_and_friends_amd.spaces import Box, Discrete
    box = Box(-np.inf, np.inf, (8,), np.float32)
    pol = generate_policy(policy_name="p", policy_class=None, actor_observation_space=box, critic_observation_space=box,
                          action_space=Discrete(5), test_mode=False, envs_per_proc=4, random_seed=1, ac_network=LSTMNetwork,
                          actor_kw_args=dict(lstm_hidden_size=32), critic_kw_args=dict(lstm_hidden_size=32))
    for a in ("a0", "a1"):
        pol.register_agent(a)
    pol.finalize({}, torch.device("cpu"))
    pol.initialize_dataset()
    pol.initialize_episodes(4, None, ts_per_rollout=8)
    obs = [torch.zeros(4, 8) for _ in range(2)]
    act = [torch.zeros(4, dtype=torch.int64) for _ in range(2)]
    why = pol.lstm_step_blocks_unsupported_reason(obs, obs, act)
    assert "observation block 0 is not a contiguous" in why and "device tensor of 4 x 8" in why
    assert "row blocks, a table holds 1 .. 16" in pol.lstm_step_blocks_unsupported_reason([], [], [])
    assert "do not pair" in pol.lstm_step_blocks_unsupported_reason(obs[:1], obs, act)
    assert "do not pair" in pol.lstm_step_blocks_unsupported_reason(None, obs + obs[:1], None)
