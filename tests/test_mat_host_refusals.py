"""
CPU tests of what the MAT update (K15) and step (K16) entry points refuse and accept on the host, Discrete and Box form
(no GPU, no launch: every pointer is a fake address that is never dereferenced).  One case per host check that a caller can
reach before a launch, named by the number or field in its message; and, for valid argument sets, the sizes the update's
query entry points return, as literals.
"""
import ctypes as C

import numpy as np
import pytest

P = 0x10000                                               # 256-byte aligned, never dereferenced
SHAPES = [(3, 5, 2, 7), (16, 33, 8, 1)]                   # (agents, obs, actions, B)
UPDATE_POINTERS = ("params", "grads", "slabs", "critic_obs", "advantages", "old_log_probs", "rewards_to_go", "values", "perm",
                   "cursor", "vn_mean", "vn_var", "vn_count", "loss_partials", "totals")


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def mat_offsets(O, NA, D=64):
    """Offset table of MATActorCritic's parameters in module order, every tensor padded to 4 floats; [63] is the total."""
    sizes = [D * (NA + 1)] + [D] * 8 + [D * D, D] * 8 + [D * D, D] * 2 + [D * D, D, D, D, NA * D, NA]
    sizes += [O, O, D * O, D] + [D] * 6 + [D * D, D] * 4 + [D * D, D] * 2 + [D * D, D, D, D, D, 1]
    return np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])]).astype(np.int64)


def _topology(a, box, L, O, NA, shift):
    """sizes and the 63 offsets into `a`; box: its two offsets; shift: {index: floats} moves one offset"""
    a.num_agents, a.obs_dim, a.num_actions, a.embedding = L, O, NA, 64
    offs = mat_offsets(max(O, 0), max(NA, 0))
    lead = (NA + 3) // 4 * 4 if box is not None else 0   # the Box bucket opens with log_std
    for i in range(63):
        a.offsets[i] = int(offs[i]) + lead + shift.get(i, 0)
    if box is not None:
        box.enc_bias_offset, box.log_std_offset = lead + 64 * NA, 0
    return int(offs[63]) + lead


def _set(a, box, over):
    for k, v in over.items():
        if k.startswith("box_"):
            setattr(box, k[4:], v)
        else:
            setattr(a, k, v)


def update_args(built, box=False, L=3, O=5, NA=2, B=7, split=True, shift=None, **over):
    full = built.MatBoxUpdateArgs() if box else None
    a = full.mat if box else built.MatUpdateArgs()
    a.bucket_total = _topology(a, full, L, O, NA, shift or {})
    for f in UPDATE_POINTERS:
        setattr(a, f, P)
    if box:
        full.raw_actions, full.min_std = P, 0.0
    else:
        a.raw_actions = P
    a.B, a.batch_stride, a.n_rows, a.n_ranks = B, B, B * L, 1
    if split:
        a.split_workspace, a.split_workspace_bytes = P, 1 << 40
    _set(a, full, over)
    return full if box else a


def step_args(built, box=False, L=3, O=5, NA=2, E=7, shift=None, **over):
    full = built.MatBoxStepArgs() if box else None
    a = full.mat if box else built.MatStepArgs()
    _topology(a, full, L, O, NA, shift or {})
    a.actor_obs_dim, a.E = O, E
    a.params = a.critic_obs = a.logp_out = a.value_out = P
    if box:
        full.action_out = full.raw_action_out = P
    else:
        a.action_out = P
    _set(a, full, over)
    return full if box else a


def blocks(built, box=False, n=3, **over):
    t = (built.MatBoxStepBlocks if box else built.MatStepBlocks)()
    t.n_blocks = n
    for b in range(min(max(n, 0), 16)):
        t.slot_agent[b], t.critic_obs[b], t.env_action[b] = b, P, P
    for k, v in over.items():
        if isinstance(v, dict):
            for i, x in v.items():
                getattr(t, k)[i] = x
        else:
            setattr(t, k, v)
    return t


def refused(lib, rc, needle):
    assert rc == -1
    assert needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error()


# ---- K15 -------------------------------------------------------------------------------------------------------------
UPDATE_BOTH = [
    (dict(embedding=32), "embedding=32"),
    (dict(L=0), "num_agents=0"), (dict(L=17), "num_agents=17"),
    (dict(O=0), "obs_dim=0"), (dict(O=129), "obs_dim=129"),
    (dict(NA=0), "num_actions=0"), (dict(NA=9), "num_actions=9"),
    (dict(B=0), "B=0"), (dict(batch_stride=6), "stride=6"),
    *[({f: None}, "null pointer") for f in UPDATE_POINTERS],
    (dict(normalize_values=1), "vn_records"), (dict(normalize_values=1, vn_records=P, n_ranks=0), "vn_records"),
    (dict(normalize_adv=1), "adv_records"),
    (dict(params=P + 8), "16-byte"), (dict(grads=P + 4), "16-byte"), (dict(slabs=P + 8), "16-byte"),
    (dict(bucket_total=4), "bucket_total=4"),
    (dict(shift={40: 4}), "parameter 40 sits at"), (dict(shift={0: 4}), "parameter 0 sits at"),
    (dict(shift={62: -4}), "parameter 62 sits at"),
    (dict(mb_offset=-1), "mb_offset=-1"), (dict(cursor_advance=-2), "cursor_advance=-2"),
    (dict(fuse_norm=1), "norm_scratch"), (dict(fuse_norm=1, norm_scratch=P), "step_count"),
    (dict(split_workspace=P + 16), "256-byte"), (dict(split_workspace_bytes=16), "split_workspace of 16 B"),
]
UPDATE_DISCRETE = [(dict(raw_actions=None), "null pointer")]
UPDATE_BOX = [
    (dict(box_raw_actions=None), "null pointer"), (dict(raw_actions=P), "null pointer"),
    (dict(box_enc_bias_offset=4), "4 / 0"), (dict(box_log_std_offset=8), "132 / 8"),
    (dict(box_min_std=-0.5), "min_std=-0.5"),
    (dict(split=False), "split_workspace"),
]


@pytest.mark.parametrize("over,needle", UPDATE_BOTH + UPDATE_DISCRETE)
def test_update_fwd_bwd_refuses(built, over, needle):
    lib = built.load()
    refused(lib, lib.ppoaf_mat_update_fwd_bwd(C.byref(update_args(built, **over)), None), needle)


@pytest.mark.parametrize("over,needle", UPDATE_BOTH + UPDATE_BOX)
def test_box_update_fwd_bwd_refuses(built, over, needle):
    lib = built.load()
    refused(lib, lib.ppoaf_mat_box_update_fwd_bwd(C.byref(update_args(built, box=True, **over)), None), needle)


def test_update_null_args(built):
    lib = built.load()
    refused(lib, lib.ppoaf_mat_update_fwd_bwd(None, None), "null args")
    refused(lib, lib.ppoaf_mat_box_update_fwd_bwd(None, None), "null args")


# ---- K16 -------------------------------------------------------------------------------------------------------------
STEP_BOTH = [
    (dict(embedding=128), "embedding=128"),
    (dict(O=0), "obs 0"), (dict(O=129), "obs 129"), (dict(NA=0), "actions 0"), (dict(NA=9), "actions 9"),
    (dict(actor_obs_dim=0), "agents 3, obs 5, actions 2"),
    (dict(params=None), "null pointer"), (dict(logp_out=None), "null pointer"), (dict(value_out=None), "null pointer"),
    (dict(normalize_values=1), "normaliser"), (dict(normalize_values=1, vn_mean=P), "normaliser"),
    (dict(params=P + 4), "16-byte"),
    (dict(L=16, E=1 << 40), "too many envs"),
]
STEP_PLAIN = [(dict(L=0), "agents 0"), (dict(L=17), "agents 17"), (dict(E=0), "E=0"), (dict(E=-1), "E=-1"),
              (dict(critic_obs=None), "null pointer")]
STEP_DISCRETE = [(dict(action_out=None), "null pointer")]
STEP_BOX = [
    (dict(box_action_out=None), "null pointer"), (dict(box_raw_action_out=None), "null pointer"),
    (dict(action_out=P), "int64"), (dict(raw_action_out=P), "int64"), (dict(forced_action=P), "int64"),
    (dict(box_act_lo=P), "bounds"), (dict(box_act_hi=P), "bounds"),
    (dict(box_min_std=-0.5), "min_std=-0.5"),
    (dict(shift={40: 4}), "parameter 40 sits at"), (dict(shift={0: -4}), "parameter 0 sits at"),
    (dict(box_enc_bias_offset=4), "4 / 0"), (dict(box_log_std_offset=8), "132 / 8"),
]
BLOCKS_TABLE = [
    (dict(n=0), "n_blocks=0"), (dict(n=17), "n_blocks=17"), (dict(n=2), "n_blocks=2"),
    (dict(slot_agent={1: 5}), "slot_agent[1]=5"), (dict(slot_agent={2: -1}), "slot_agent[2]=-1"),
    (dict(slot_agent={1: 0}), "block 0 twice"),
    (dict(critic_obs={1: None}), "block 1"), (dict(env_action={2: None}), "block 2"), (dict(critic_obs={0: P + 8}), "block 0"),
    (dict(actor_obs={1: P + 4}), "block 1"), (dict(actor_obs={1: P}), "block 1"), (dict(env_action={0: P + 8}), "block 0"),
]


@pytest.mark.parametrize("over,needle", STEP_BOTH + STEP_PLAIN + STEP_DISCRETE)
def test_policy_step_refuses(built, over, needle):
    lib = built.load()
    refused(lib, lib.ppoaf_mat_policy_step(C.byref(step_args(built, **over)), None), needle)


@pytest.mark.parametrize("over,needle", STEP_BOTH + STEP_PLAIN + STEP_BOX)
def test_box_policy_step_refuses(built, over, needle):
    lib = built.load()
    refused(lib, lib.ppoaf_mat_box_policy_step(C.byref(step_args(built, box=True, **over)), None), needle)


@pytest.mark.parametrize("box", [False, True])
def test_policy_step_blocks_refuses(built, box):
    lib = built.load()
    fn = lib.ppoaf_mat_box_policy_step_blocks if box else lib.ppoaf_mat_policy_step_blocks
    call = lambda a, t: fn(C.byref(a), C.byref(t), None)
    for over, needle in BLOCKS_TABLE:
        refused(lib, call(step_args(built, box=box), blocks(built, box, **over)), needle)
    refused(lib, call(step_args(built, box=box, E=-1), blocks(built, box)), "E=-1")
    refused(lib, call(step_args(built, box=box, L=17), blocks(built, box)), "17 agents")
    refused(lib, call(step_args(built, box=box, L=0), blocks(built, box)), "0 agents")
    # behind the table's checks the block form runs the plain form's (without the observation pointers of the args)
    for over, needle in STEP_BOTH + (STEP_BOX if box else STEP_DISCRETE):
        refused(lib, call(step_args(built, box=box, **over), blocks(built, box, n=over.get("L", 3))), needle)
    a = step_args(built, box=box, critic_obs=None, actor_obs=None, E=0)
    assert call(a, blocks(built, box)) == 0              # nothing to do: accepted without a launch
    refused(lib, fn(None, C.byref(blocks(built, box)), None), "null args")
    refused(lib, fn(C.byref(step_args(built, box=box)), None, None), "null args")


def test_policy_step_null_args(built):
    lib = built.load()
    refused(lib, lib.ppoaf_mat_policy_step(None, None), "null args")
    refused(lib, lib.ppoaf_mat_box_policy_step(None, None), "null args")


# ---- the accepted path that needs no device -----------------------------------------------------------------------------
# (box, agents, obs, actions, B) -> [split_workspace_bytes, tail_ctl_bytes, norm_partials on the split-wgrad chain,
# norm_partials without a split workspace (the Box form has no such chain: refused, -1)]
SIZES = {
    (False, 3, 5, 2, 7): [245760, 2688, 152, 76],
    (False, 16, 33, 8, 1): [122880, 2848, 162, 78],
    (True, 3, 5, 2, 7): [245760, 2688, 152, -1],
    (True, 16, 33, 8, 1): [122880, 2848, 162, -1],
}


@pytest.mark.parametrize("box,L,O,NA,B", sorted(SIZES))
def test_update_sizes_are_the_recorded_ones(built, box, L, O, NA, B):
    lib = built.load()
    fn = lambda name: getattr(lib, ("ppoaf_mat_box_update_" if box else "ppoaf_mat_update_") + name)
    args = lambda **kw: update_args(built, box=box, L=L, O=O, NA=NA, B=B, **kw)
    ws, ws2, ctl = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    assert fn("split_workspace_bytes")(C.byref(args(split=False)), C.byref(ws)) == 0
    exact = args(split_workspace_bytes=ws.value)          # the least workspace is accepted, one byte less is not
    assert fn("split_workspace_bytes")(C.byref(exact), C.byref(ws2)) == 0 and ws2.value == ws.value
    assert fn("tail_ctl_bytes")(C.byref(exact), C.byref(ctl)) == 0
    got = [ws.value, ctl.value, fn("norm_partials")(C.byref(exact)), fn("norm_partials")(C.byref(args(split=False)))]
    assert got == SIZES[(box, L, O, NA, B)]
    assert fn("norm_partials")(C.byref(args(split_workspace_bytes=ws.value - 1))) == -1
    refused(lib, fn("tail_ctl_bytes")(C.byref(args(split=False)), C.byref(ctl)), "split_workspace")
    refused(lib, fn("tail_ctl_bytes")(None, C.byref(ctl)), "null argument")
    refused(lib, fn("split_workspace_bytes")(C.byref(exact), None), "null argument")


@pytest.mark.parametrize("box", [False, True])
@pytest.mark.parametrize("L,O,NA,B", SHAPES)
def test_policy_step_blocks_accepts_an_empty_batch(built, box, L, O, NA, B):
    lib = built.load()
    fn = lib.ppoaf_mat_box_policy_step_blocks if box else lib.ppoaf_mat_policy_step_blocks
    a = step_args(built, box=box, L=L, O=O, NA=NA, E=0)
    assert fn(C.byref(a), C.byref(blocks(built, box, n=L)), None) == 0
