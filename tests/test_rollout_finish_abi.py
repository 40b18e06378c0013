"""
Host checks of ppoaf_rollout_finish_rows (K23) and of the block table of ppoaf_policy_step_blocks, without a GPU: every
refusal is decided before the launch, and E == 0 returns 0 without one.  The pointers are never dereferenced on the host,
so made-up addresses do.
"""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from ppo_and_friends_amd.csrc import build
    from ppo_and_friends_amd import _lib
    build.build(verbose=False)
    return _lib.load()


def _args(E=4, n_members=2, n_blocks=(1, 2), grouped=(0, 1), base=0x10000):
    from ppo_and_friends_amd import _lib
    a = _lib.RolloutFinishArgs()
    a.n_members, a.write_ends, a.last_step, a.max_ts_per_ep, a.ext_reward_weight, a.E = n_members, 1, 0, 7, 1.0, E
    a.terminated, a.truncated, a.ep_ts = base, base + 64, base + 128
    p = base + 1024
    for m, nb, g in zip(a.members, n_blocks, grouped):
        m.n_blocks, m.grouped = nb, g
        for b in range(min(nb, _lib.ROW_BLOCKS_MAX)):
            m.slot_agent[b] = b
            m.reward[b] = p
            p += 64
        m.reward_out, m.natural_out, m.end_kind_out = p, p + 64, p + 128
        p += 256
    return a


def _refused(lib, a, needle):
    from ppo_and_friends_amd import _lib
    rc = lib.ppoaf_rollout_finish_rows(C.byref(a), None)
    assert rc != 0
    msg = lib.ppoaf_last_error().decode()
    assert needle in msg, msg
    with pytest.raises(_lib.PpoafError, match="rollout_finish_rows"):
        _lib.check(rc, "rollout_finish_rows")


def test_the_abi_version_and_the_older_entry_points_stay(lib):
    from ppo_and_friends_amd import _lib
    assert lib.ppoaf_abi_version() == 7 == _lib.ABI_VERSION
    assert C.sizeof(_lib.RolloutFinishArgs) < 4096                      # travels by value in the kernel arguments


def test_no_env_is_no_launch(lib):
    assert lib.ppoaf_rollout_finish_rows(C.byref(_args(E=0)), None) == 0


def test_a_negative_env_count_is_refused(lib):
    _refused(lib, _args(E=-1), "E=-1")


def test_a_misaligned_block_is_refused(lib):
    a = _args()
    a.members[1].reward[1] = a.members[1].reward[1] + 2
    _refused(lib, a, "member 1: reward block 1")
    a = _args()
    a.members[0].reward[0] = None
    _refused(lib, a, "member 0: reward block 0")


def test_seventeen_blocks_and_none_are_refused(lib):
    _refused(lib, _args(n_blocks=(17, 2)), "n_blocks=17")
    _refused(lib, _args(n_blocks=(1, 0)), "n_blocks=0")


def test_nine_members_are_refused(lib):
    _refused(lib, _args(n_members=9), "n_members=9")
    _refused(lib, _args(n_members=0), "n_members=0")


def test_a_slot_outside_the_table_is_refused(lib):
    a = _args()
    a.members[1].slot_agent[1] = 2
    _refused(lib, a, "slot_agent[1]=2 is outside the table of 2 blocks")
    a = _args()
    a.members[1].slot_agent[0] = -1
    _refused(lib, a, "slot_agent[0]=-1")
    a = _args()
    a.members[1].slot_agent[1] = 0
    _refused(lib, a, "twice")


def test_ends_need_their_tables(lib):
    a = _args()
    a.terminated = None
    _refused(lib, a, "write_ends needs terminated and ep_ts")
    a = _args()
    a.members[0].end_kind_out = None
    _refused(lib, a, "write_ends without end_kind_out")


def _step_blocks(n_blocks=2, rows=4, base=0x20000):
    from ppo_and_friends_amd import _lib
    a, t = _lib.PolicyStepArgs(), _lib.StepBlocks()
    a.E = n_blocks * rows
    t.n_blocks, t.rows_per_block = n_blocks, rows
    for b in range(min(n_blocks, _lib.ROW_BLOCKS_MAX)):
        t.obs[b], t.critic_obs[b], t.env_action[b] = base + 256 * b, base + 0x1000 + 256 * b, base + 0x2000 + 256 * b
    return a, t


def _step_refused(lib, a, t, needle):
    assert lib.ppoaf_policy_step_blocks(C.byref(a), C.byref(t), None) != 0
    msg = lib.ppoaf_last_error().decode()
    assert needle in msg, msg


def test_step_blocks_refuses_a_bad_table_before_anything_else(lib):
    a, t = _step_blocks(n_blocks=17)
    _step_refused(lib, a, t, "n_blocks=17")
    a, t = _step_blocks(n_blocks=0)
    _step_refused(lib, a, t, "n_blocks=0")
    a, t = _step_blocks()
    t.obs[1] = t.obs[1] + 4
    _step_refused(lib, a, t, "block 1: a base is null or not 16-byte aligned")
    a, t = _step_blocks()
    t.env_action[0] = None
    _step_refused(lib, a, t, "block 0: a base is null or not 16-byte aligned")
    a, t = _step_blocks()
    a.E = 9
    _step_refused(lib, a, t, "E=9 is not n_blocks=2 x rows_per_block=4")
    a, t = _step_blocks(rows=-1)
    _step_refused(lib, a, t, "rows_per_block=-1")


def test_step_blocks_without_an_env_is_no_launch(lib):
    a, t = _step_blocks(rows=0)
    assert a.E == 0
    assert lib.ppoaf_policy_step_blocks(C.byref(a), C.byref(t), None) == 0
    a, t = _step_blocks(rows=0)
    t.obs[0] = t.obs[0] + 4                       # the table is still checked
    _step_refused(lib, a, t, "block 0: a base is null or not 16-byte aligned")


def test_the_ctypes_mirrors_have_the_layout_the_library_asserts():
    """The offsets the library pins with static_asserts (csrc/rollout_finish.hip, policy_step.hip, mat_update.hip)."""
    from ppo_and_friends_amd import _lib
    off = lambda cls: {n: getattr(cls, n).offset for n, _ in cls._fields_}
    assert C.sizeof(_lib.FinishMember) == 360 and off(_lib.FinishMember) == dict(
        n_blocks=0, grouped=4, slot_agent=8, reward=72, natural=200, intrinsic=328, reward_out=336, natural_out=344, end_kind_out=352)
    assert C.sizeof(_lib.RolloutFinishArgs) == 2936 and off(_lib.RolloutFinishArgs) == dict(
        n_members=0, write_ends=4, last_step=8, max_ts_per_ep=12, ext_reward_weight=16, E=24, terminated=32, truncated=40,
        ep_ts=48, members=56)
    assert C.sizeof(_lib.StepBlocks) == 400 and off(_lib.StepBlocks) == dict(
        n_blocks=0, rows_per_block=8, obs=16, critic_obs=144, env_action=272)
    assert C.sizeof(_lib.MatStepBlocks) == 456 and off(_lib.MatStepBlocks) == dict(
        n_blocks=0, slot_agent=4, critic_obs=72, actor_obs=200, env_action=328)


def test_mat_step_blocks_refuses_a_bad_table_before_anything_else(lib):
    from ppo_and_friends_amd import _lib

    def table(n=3, agents=3):
        a, t = _lib.MatStepArgs(), _lib.MatStepBlocks()
        a.num_agents, a.E, t.n_blocks = agents, 4, n
        for b in range(min(n, _lib.ROW_BLOCKS_MAX)):
            t.slot_agent[b] = b
            t.critic_obs[b], t.env_action[b] = 0x30000 + 256 * b, 0x40000 + 256 * b
        return a, t

    def refused(a, t, needle):
        assert lib.ppoaf_mat_policy_step_blocks(C.byref(a), C.byref(t), None) != 0
        msg = lib.ppoaf_last_error().decode()
        assert needle in msg, msg
    refused(*table(n=17, agents=17), "n_blocks=17")
    refused(*table(n=2), "n_blocks=2, the policy has 3 agents")
    a, t = table()
    t.slot_agent[2] = 3
    refused(a, t, "slot_agent[2]=3 is outside the table of 3 blocks")
    a, t = table()
    t.slot_agent[2] = 1
    refused(a, t, "twice")
    a, t = table()
    t.critic_obs[1] = t.critic_obs[1] + 8
    refused(a, t, "block 1: a base is null or not 16-byte aligned")
    a, t = table()
    a.E = 0
    assert lib.ppoaf_mat_policy_step_blocks(C.byref(a), C.byref(t), None) == 0          # no env: no launch
