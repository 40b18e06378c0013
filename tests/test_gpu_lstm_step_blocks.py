"""
The block form of K21 (ppoaf_lstm_policy_step_blocks) against the tensor form (ppoaf_lstm_policy_step) on the gathered
rows, through the C ABI: same buckets, same states, same seed / offset -> every output bit for bit, and the env-action
blocks hold the action rows.

Shapes: rows_per_block x blocks = 10 x 3 (a 16-row tile straddles two blocks), 16 x 2 (tiles and blocks coincide), 1 x 16 (one
tile over sixteen blocks), 5 x 3 (a tile over three blocks, the last tile -- here the only one -- partial).  The blocks
are handed in an order that is not ascending in memory, with gaps between them that hold a canary.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEP, CRITIC_NEXT = 0, 1
I_ACTOR, I_CRITIC = 8, 10
SHAPES = {"10x3": (10, 3), "16x2": (16, 2), "1x16": (1, 16), "5x3": (5, 3)}
# head: (head_kind, out_dim, bounds)
HEADS = {"categorical": (0, 5, None), "gaussian": (1, 2, None), "gaussian_bounds": (1, 3, (-2.0, 3.0))}


@pytest.fixture(scope="module")
def lib():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def _rand(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


def _scattered(g, n_blocks, rows, width, dtype=torch.float32):
    """n_blocks contiguous [rows, width] views of one arena filled with 7, in an order that is not ascending in memory,
    16-element gaps between them; returns (blocks in table order, arena)."""
    stride = rows * width + 16
    arena = torch.full((n_blocks * stride,), 7, dtype=dtype, device=DEV)
    order = {2: [1, 0], 3: [2, 0, 1]}.get(n_blocks) or [(5 * b + 2) % n_blocks for b in range(n_blocks)]
    assert sorted(order) == list(range(n_blocks)) and (n_blocks == 1 or order != sorted(order))
    blocks = [arena[o * stride:o * stride + rows * width].view(rows, width) for o in order]
    return blocks, arena


class Problem:
    """One policy's buckets and one step's inputs for E = rows * n_blocks rows."""

    def __init__(self, lib, H, head, rows, n_blocks, seed=3):
        from ppo_and_friends_amd import kernels as K
        self.lib, self.H, self.rows, self.n_blocks, self.E = lib, H, rows, n_blocks, rows * n_blocks
        self.kind, self.O, self.bounds = HEADS[head]
        g = torch.Generator().manual_seed(seed)
        E = self.E
        self.desc, self.params = {}, {}
        for tag, I, F, depth, O in (("actor", I_ACTOR, 16, 1, self.O), ("critic", I_CRITIC, 32, 2, 1)):
            d = K.lstm_desc(I, H, F, depth, O, 0, E, 1, torch.zeros(4, device=DEV))
            _, floats = K.lstm_sizes(d)
            self.params[tag] = _rand(g, floats, scale=0.2)
            self.desc[tag] = K.lstm_desc(I, H, F, depth, O, 0, E, 1, self.params[tag])
        self.obs_blocks, self.obs_arena = _scattered(g, n_blocks, rows, I_ACTOR)
        self.cobs_blocks, self.cobs_arena = _scattered(g, n_blocks, rows, I_CRITIC)
        for b in self.obs_blocks + self.cobs_blocks:
            b.copy_(_rand(g, *b.shape))
        self.state0 = [_rand(g, E, H, scale=0.5) for _ in range(4)]              # actor h, c, critic h, c
        self.log_std = _rand(g, self.O, scale=0.3)
        self.lo = self.hi = None
        if self.bounds is not None:
            self.lo = torch.full((self.O,), self.bounds[0], device=DEV)
            self.hi = torch.full((self.O,), self.bounds[1], device=DEV)
        gauss = self.kind == 1
        self.adt, self.aw = (torch.float32, self.O) if gauss else (torch.int64, 1)
        forced = torch.randint(0, self.O, (E, 1), generator=g) if not gauss else torch.randn(E, self.O, generator=g)
        self.forced = forced.to(DEV).to(self.adt).contiguous()
        self.vn = (torch.full((1,), 0.7, device=DEV), torch.full((1,), 2.5, device=DEV))
        self.terminated_env = (torch.rand(rows, generator=g) < 0.4).to(DEV)
        self.terminated_env[0] = True
        self.stored0 = [_rand(g, E, H) for _ in range(4)]

    def args(self, mode, out, forced=False, commit=None, terminated=None):
        a = self.lib.LstmPolicyStepArgs()
        a.actor, a.critic = self.desc["actor"], self.desc["critic"]
        a.E, a.head_kind, a.mode, a.min_std = self.E, self.kind, mode, 0.01
        a.log_std = self.log_std.data_ptr()
        if self.lo is not None:
            a.act_lo, a.act_hi = self.lo.data_ptr(), self.hi.data_ptr()
        a.seed, a.offset = 1234, 96
        a.normalize_values, a.vn_mean, a.vn_var = 1, self.vn[0].data_ptr(), self.vn[1].data_ptr()
        for f, t in zip(("actor_h", "actor_c", "critic_h", "critic_c"), out["state"]):
            setattr(a, f, t.data_ptr())
        for f, t in zip(("actor_hidden_out", "actor_cell_out", "critic_hidden_out", "critic_cell_out"), out["stored"]):
            setattr(a, f, t.data_ptr())
        a.raw_action_out, a.action_out = out["raw"].data_ptr(), out["act"].data_ptr()
        a.logp_out, a.value_out = out["logp"].data_ptr(), out["value"].data_ptr()
        a.obs_copy_out, a.critic_obs_copy_out = out["obs_copy"].data_ptr(), out["cobs_copy"].data_ptr()
        a.boot_value_out = out["boot"].data_ptr()
        a.forced_raw_action = self.forced.data_ptr() if forced else None
        a.commit = None if commit is None else commit.data_ptr()
        a.terminated = None if terminated is None else terminated.data_ptr()
        return a

    def outputs(self, stored_from=None):
        E, H = self.E, self.H
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        return dict(state=[s.clone() for s in self.state0],
                    stored=[s.clone() for s in stored_from] if stored_from is not None else [nan(E, H) for _ in range(4)],
                    raw=torch.full((E, self.aw), -9, device=DEV).to(self.adt), act=torch.full((E, self.aw), -9, device=DEV).to(self.adt),
                    logp=nan(E), value=nan(E), obs_copy=nan(E, I_ACTOR), cobs_copy=nan(E, I_CRITIC), boot=nan(E))

    def table(self, env_action=None):
        t = self.lib.LstmStepBlocks()
        t.n_blocks, t.rows_per_block = self.n_blocks, self.rows
        for b in range(self.n_blocks):
            t.obs[b], t.critic_obs[b] = self.obs_blocks[b].data_ptr(), self.cobs_blocks[b].data_ptr()
            t.env_action[b] = None if env_action is None else env_action[b].data_ptr()
        return t


def _launch(lib, a, table=None):
    from ppo_and_friends_amd import kernels as K
    L = lib.load()
    rc = L.ppoaf_lstm_policy_step(C.byref(a), K.stream()) if table is None else \
        L.ppoaf_lstm_policy_step_blocks(C.byref(a), C.byref(table), K.stream())
    assert rc == 0, L.ppoaf_last_error().decode()
    torch.cuda.synchronize()


def _same(got, want, what):
    """Bit for bit (NaN fill included: what one form leaves untouched the other leaves untouched)."""
    for k in want:
        pairs = zip(got[k], want[k]) if isinstance(want[k], list) else [(got[k], want[k])]
        for i, (g, w) in enumerate(pairs):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, i)
            assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), (what, k, i)


@pytest.mark.parametrize("forced", [False, True], ids=["sampled", "forced"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("head", sorted(HEADS))
@pytest.mark.parametrize("H", [32, 64, 128])
def test_step_equals_the_tensor_form_on_gathered_rows(lib, H, head, shape, forced):
    rows, n_blocks = SHAPES[shape]
    p = Problem(lib, H, head, rows, n_blocks)
    obs, cobs = torch.cat(p.obs_blocks, 0).contiguous(), torch.cat(p.cobs_blocks, 0).contiguous()
    want = p.outputs()
    a = p.args(STEP, want, forced)
    a.obs, a.critic_obs = obs.data_ptr(), cobs.data_ptr()
    _launch(lib, a)
    got = p.outputs()
    env_blocks, env_arena = _scattered(torch.Generator().manual_seed(1), n_blocks, rows, p.aw, p.adt)
    arena_before = env_arena.clone()
    a = p.args(STEP, got, forced)                                  # obs / critic_obs stay NULL: they are not read
    _launch(lib, a, p.table(env_blocks))
    _same(got, want, f"H={H} {head} {shape}")
    # the tensor form wrote something everywhere it should (so equality is not NaN == NaN)
    assert torch.isfinite(want["logp"]).all() and torch.isfinite(want["value"]).all()
    assert all(torch.isfinite(s).all() for s in want["stored"] + want["state"])
    assert torch.equal(want["obs_copy"], obs) and torch.equal(want["cobs_copy"], cobs)
    assert not torch.equal(want["state"][0], p.state0[0])
    if forced:
        assert torch.equal(want["raw"], p.forced)
    # the env's action blocks hold the action rows, and nothing between the blocks was written
    assert torch.equal(torch.cat(env_blocks, 0), want["act"])
    for b in env_blocks:
        b.fill_(7)
    assert torch.equal(env_arena, torch.full_like(arena_before, 7))


@pytest.mark.parametrize("commit", [0, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("H", [32, 64, 128])
def test_critic_next_equals_the_tensor_form_on_gathered_rows(lib, H, shape, commit):
    rows, n_blocks = SHAPES[shape]
    p = Problem(lib, H, "categorical", rows, n_blocks)
    cobs = torch.cat(p.cobs_blocks, 0).contiguous()
    flag = torch.full((1,), commit, dtype=torch.uint8, device=DEV)
    term_rows = p.terminated_env.repeat(n_blocks).contiguous()     # the tensor form: one flag per row
    want = p.outputs(p.stored0)
    a = p.args(CRITIC_NEXT, want, commit=flag, terminated=term_rows)
    a.critic_obs = cobs.data_ptr()
    _launch(lib, a)
    got = p.outputs(p.stored0)
    a = p.args(CRITIC_NEXT, got, commit=flag, terminated=p.terminated_env)     # the block form: one flag per env
    t = p.table()
    for b in range(n_blocks):
        t.obs[b] = None                                            # CRITIC_NEXT reads the critic's blocks only
    _launch(lib, a, t)
    _same(got, want, f"H={H} {shape} commit={commit}")
    assert torch.isfinite(want["boot"]).all()
    assert torch.equal(want["state"][2], p.state0[2]) == (commit == 0)
    assert torch.equal(want["state"][0], p.state0[0])               # the actor is not stepped
    for s, s0 in zip(want["stored"], p.stored0):
        assert not s[term_rows].any() and torch.equal(s[~term_rows], s0[~term_rows])


def test_the_policy_wrappers_run_the_block_form(lib):
    """kernels.lstm_policy_step / lstm_critic_next with `blocks` reach the same entry point (one shape)."""
    from ppo_and_friends_amd import kernels as K
    p = Problem(lib, 32, "categorical", 10, 3)
    obs, cobs = torch.cat(p.obs_blocks, 0).contiguous(), torch.cat(p.cobs_blocks, 0).contiguous()
    want, got = p.outputs(), p.outputs()
    a = p.args(STEP, want)
    a.obs, a.critic_obs = obs.data_ptr(), cobs.data_ptr()
    _launch(lib, a)
    env_blocks = [torch.zeros(10, dtype=torch.int64, device=DEV) for _ in range(3)]
    a = p.args(STEP, got)
    K.lstm_policy_step(a, None, None, got["state"][:2], got["state"][2:], got["raw"], got["act"], got["logp"], got["value"],
                       got["stored"], got["obs_copy"], got["cobs_copy"], blocks=p.table(env_blocks))
    torch.cuda.synchronize()
    _same(got, want, "wrapper")
    assert torch.equal(torch.cat(env_blocks, 0), want["act"].reshape(-1))
    assert K.lstm_policy_step_blocks_refusal(a, p.table(env_blocks)) == ""
    bad = p.table(env_blocks)
    bad.n_blocks = 2
    assert "E=30 is not n_blocks=2" in K.lstm_policy_step_blocks_refusal(a, bad)
