"""
-m gpu: K20 `ppoaf_mat_policy_infer` and `ppoaf_eval_scores_step_books` at the kernel level.

  * sampled mode is K16: for equal (obs, params, seed, offset) in grouped layout the actions are bitwise
    ppoaf_mat_policy_step's action_out, at g12_c5_mat's shape and the shape edges, for E around the tile boundaries
    (this is also what catches an aliasing mistake in the forward-only LDS carve);
  * layouts: agent-major input with a non-identity slot order gives the grouped result, permuted, in both modes;
  * deterministic mode against the float64 greedy decode of oracle.mat_oracle (tests/helpers/mat_float64.py) under the
    near-tie rule of tests/test_gpu_eval_kernels.py; exact ties take class 0;
  * the books against the chain of ppoaf_eval_scores_step calls they replace and against the numpy restatement, bit
    for bit after every step.
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

C5 = (3, 18, 5)                                              # (agents, obs, actions) of g12_c5_mat
EDGES = [(2, 18, 5), (5, 18, 5), (16, 18, 5), (3, 18, 1), (3, 18, 8), (3, 1, 5), (3, 32, 5)]
EDGE_SEED = 11          # torch seed of the edge shapes' initialisation: the float64 forward alone leaves out at most
#                         0.25 % of the decisions of any of them (41 of 16 384 at 16 agents; checked on the CPU)


def _topology(ac):
    from ppo_and_friends_amd.fused_update import _describe_mat
    topo, why = _describe_mat(types.SimpleNamespace(actor_critic=ac, action_dtype="discrete"))
    assert topo is not None, why
    return topo


def _network(A, O, NA, seed=EDGE_SEED):
    import mat_float64 as M
    ac = M.make_network(O, NA, A, seed, DEV)
    return ac, _topology(ac)


def _c5_network(golden, head_scale=1.0):
    ac, topo = _network(*C5)
    g = golden("g12_c5_mat")
    sd = {"actor." + k[len("init_actor."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init_actor.")}
    sd.update({"critic." + k[len("init_critic."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init_critic.")})
    missing, unexpected = ac.load_state_dict(sd, strict=False)
    assert not [m for m in missing if "mask" not in m] and not [u for u in unexpected if "mask" not in u]
    with torch.no_grad():
        ac.actor.head[3].weight.mul_(head_scale)
    return ac, topo


def _fill(a, topo, ac):
    a.obs_dim, a.num_agents, a.num_actions, a.embedding = topo["obs_dim"], topo["num_agents"], topo["num_actions"], 64
    for i, o in enumerate(topo["offsets"]):
        a.offsets[i] = o
    a.params = ac.flat_params.data_ptr()


def k16_actions(ac, topo, obs, seed, offset):
    """ppoaf_mat_policy_step on grouped obs [E, A, O] -> action_out [E, A]."""
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    E, A, O = obs.shape
    a = _lib.MatStepArgs()
    _fill(a, topo, ac)
    a.actor_obs_dim, a.normalize_values, a.E = O, 0, E
    obs = obs.contiguous()
    a.critic_obs = obs.data_ptr()
    a.seed, a.offset = seed, offset
    act = torch.full((E, A), -1, dtype=torch.int64, device=DEV)
    logp, val = torch.zeros(E, A, device=DEV), torch.zeros(E, A, device=DEV)
    a.action_out, a.logp_out, a.value_out = act.data_ptr(), logp.data_ptr(), val.data_ptr()
    _lib.check(_lib.load().ppoaf_mat_policy_step(C.byref(a), K.stream()), "mat_policy_step")
    return act


def k20_actions(ac, topo, obs, mode, seed=0, offset=0, order=None):
    """ppoaf_mat_policy_infer.  order None: grouped obs [E, A, O] -> [E, A]; else agent-major obs [A * E, O] with that
    slot order -> [A * E]."""
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    A, O = topo["num_agents"], topo["obs_dim"]
    E = obs.numel() // (A * O)
    a = _lib.MatInferArgs()
    _fill(a, topo, ac)
    obs = obs.contiguous()
    a.obs, a.E, a.mode, a.seed, a.offset = obs.data_ptr(), E, mode, seed, offset
    for i, k in enumerate(range(A) if order is None else order):
        a.slot_agent[i] = int(k)
    a.obs_env_stride, a.obs_agent_stride = (A, 1) if order is None else (1, E)
    a.act_env_stride, a.act_agent_stride = a.obs_env_stride, a.obs_agent_stride
    act = torch.full((E, A) if order is None else (A * E,), -1, dtype=torch.int64, device=DEV)
    a.action_out = act.data_ptr()
    K.mat_policy_infer(a)
    return act


def _obs(E, A, O, seed=3):
    return torch.from_numpy((2 * np.random.default_rng(seed).standard_normal((E, A, O))).astype(np.float32)).to(DEV)


def _batch_sizes(A):
    per_tile = 16 // A
    sizes = {1, per_tile - 1, 4 * per_tile, 4 * per_tile + 1, 4096}
    return sorted(e for e in sizes if e >= 1)


# ------------------------------------------------------------------------------------------------------------- sampled
@pytest.mark.parametrize("shape", [C5] + EDGES)
def test_sampled_actions_are_k16s(shape):
    A, O, NA = shape
    ac, topo = _network(A, O, NA)
    for E in _batch_sizes(A):
        obs = _obs(E, A, O, seed=E)
        seed, offset = 0x1234ABCD5678 + E, 977 * E
        want = k16_actions(ac, topo, obs, seed, offset)
        got = k20_actions(ac, topo, obs, 0, seed, offset)
        assert int(want.min()) >= 0 and int(want.max()) < NA
        assert torch.equal(got, want), (shape, E, int((got != want).sum()))
        if NA > 1 and E >= 16:
            assert len(torch.unique(got)) > 1
    # the draw depends on the counter: another offset, other actions (and K16's again)
    if NA > 1:
        obs = _obs(256, A, O)
        a0, a1 = k20_actions(ac, topo, obs, 0, 5, 0), k20_actions(ac, topo, obs, 0, 5, 256 * A)
        assert not torch.equal(a0, a1) and torch.equal(a1, k16_actions(ac, topo, obs, 5, 256 * A))


# ------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("shape,order", [(C5, [2, 0, 1]), ((5, 18, 5), [4, 2, 0, 3, 1]),
                                         ((16, 18, 5), [3, 15, 0, 9, 1, 12, 6, 14, 2, 8, 5, 11, 7, 13, 4, 10])])
def test_agent_major_layout_is_the_grouped_result_permuted(shape, order):
    A, O, NA = shape
    ac, topo = _network(A, O, NA)
    order_t = torch.as_tensor(order, device=DEV)
    for E in (1, 7, 333):
        grouped = _obs(E, A, O, seed=40 + E)                                    # [E, A, O], slot order
        major = torch.empty(A, E, O, device=DEV)
        major[order_t] = grouped.transpose(0, 1)                                # env agent order[s] sits in slot s
        for mode in (1, 0):
            want = k20_actions(ac, topo, grouped, mode, 9, 31)                  # [E, A]
            got = k20_actions(ac, topo, major.reshape(A * E, O), mode, 9, 31, order=order).reshape(A, E)
            assert torch.equal(got[order_t].transpose(0, 1), want), (shape, E, mode)
            assert int(got.min()) >= 0


# ------------------------------------------------------------------------------------------------------- deterministic
def _check_against_float64(ac, topo, obs, label):
    import mat_float64 as M
    A, O, NA = topo["num_agents"], topo["obs_dim"], topo["num_actions"]
    got = k20_actions(ac, topo, obs, 1).cpu().numpy()
    want, logits = M.float64_logits_decode(ac.state_dict(), O, NA, A, obs.cpu().numpy())
    keep = M.compared_slots(logits)
    wrong = (got != want) & keep
    print(f"\n{label}: {(~keep).sum()} of {keep.size} decisions left out ({100 * (~keep).mean():.3f} %), "
          f"{(got != want).sum()} differ from float64, {wrong.sum()} of them compared; classes {np.unique(got).tolist()}")
    if wrong.any():
        e, s = np.argwhere(wrong)[0]
        z = np.sort(logits[s, e])[::-1]
        print(f"  first: env {e} slot {s}: K20 {got[e, s]}, float64 {want[e, s]}, top-two gap {z[0] - z[1]:.3e}")
    assert (~keep).mean() <= 0.005
    assert not wrong.any()
    if NA > 1:
        assert len(np.unique(got)) > 1
    else:
        assert not got.any()
    return got


@pytest.mark.parametrize("head_scale", [1.0, 100.0])
def test_deterministic_c5_against_float64(golden, head_scale):
    """g12_c5_mat initial weights, obs = 2 * default_rng(3).standard_normal((4096, 3, 18)): the float64 forward leaves
    out 9 of 12 288 decisions (0.073 %), as is and with the head's last layer x 100; all five classes occur."""
    ac, topo = _c5_network(golden, head_scale)
    got = _check_against_float64(ac, topo, _obs(4096, *C5[:2]), f"c5 head x {head_scale:g}")
    assert sorted(np.unique(got).tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("shape", EDGES)
def test_deterministic_edges_against_float64(shape):
    A, O, NA = shape
    ac, topo = _network(A, O, NA)
    _check_against_float64(ac, topo, _obs(1024, A, O, seed=100 + EDGE_SEED), f"{shape}")


@pytest.mark.parametrize("shape", [C5, (16, 18, 8), (2, 1, 5)])
def test_exact_ties_take_class_zero(shape):
    A, O, NA = shape
    ac, topo = _network(A, O, NA)
    with torch.no_grad():
        ac.actor.head[3].weight.zero_()
        ac.actor.head[3].bias.fill_(0.25)
    for E in (5, 1000):
        grouped = k20_actions(ac, topo, _obs(E, A, O), 1)
        assert grouped.shape == (E, A) and not grouped.any()
    # (the modes differ: the same logits sampled are not all class 0)
    assert k20_actions(ac, topo, _obs(1000, A, O), 0, 3, 0).any()


def test_deterministic_mode_does_not_read_the_counter():
    ac, topo = _network(*C5)
    obs = _obs(500, *C5[:2])
    assert torch.equal(k20_actions(ac, topo, obs, 1, 1, 2), k20_actions(ac, topo, obs, 1, 99, 10 ** 12))


# --------------------------------------------------------------------------------------------------------------- books
@pytest.mark.parametrize("A,masks,E", [
    (3, [1, 2, 4, 7], 300),                                  # three agents and the policy they share
    (2, [1, 2, 3], 256),
    (16, [1 << 15, 0xFFFF, 3, 1], 257),                      # masks with 1, 2 and 16 agents
    (5, [1, 2, 4, 8, 16, 0b10101, 0b01010], 1000),           # two policies splitting the agents
])
def test_books_are_the_chain_of_single_calls(A, masks, E):
    import eval_restatement as R
    from ppo_and_friends_amd import kernels as K
    T = 50
    rng = np.random.default_rng(17 * A + E)
    quota = rng.integers(0, 4, E).astype(np.int32)           # rows that owe nothing included
    quota[:3] = (0, 1, 3)
    score = (3 * rng.standard_normal((T, A, E))).astype(np.float32)
    done = rng.random((T, E)) < 0.15
    done[6::7] = True                                        # all-done steps
    N = int(quota.sum())
    books = K.EvalScoreBooks(E, N, DEV, A, masks, quota=torch.from_numpy(quota))
    chains = [K.EvalScores(E, N, DEV, quota=torch.from_numpy(quota)) for _ in masks]
    never = torch.zeros(E, dtype=torch.bool, device=DEV)
    fields = ("run_score", "run_len", "count", "sum", "min", "max", "steps")
    for t in range(T):
        s_t, d_t = torch.from_numpy(score[t]).to(DEV), torch.from_numpy(done[t]).to(DEV)
        books.step(s_t, d_t)
        for b, m in enumerate(masks):
            mine = [a for a in range(A) if (m >> a) & 1]
            for a in mine:                                   # what testing.py did per agent (and per agent of a policy)
                chains[b].step(s_t[a].contiguous(), d_t if a == mine[-1] else never)
            for f in fields:
                assert torch.equal(getattr(books, f)[b], getattr(chains[b], f)), (t, b, f)
            assert int(books.remaining_t[b]) == int(chains[b].remaining_t[0]) == books.remaining(b)
    per_book = books.results()
    for b, m in enumerate(masks):
        mine = [a for a in range(A) if (m >> a) & 1]
        sc = score[:, mine, :].reshape(T * len(mine), E)
        dn = np.stack([np.zeros((T, E), bool)] * (len(mine) - 1) + [done], 1).reshape(T * len(mine), E)
        want = R.replay(sc, dn, quota)
        for f in ("count", "sum", "min", "max", "steps"):
            np.testing.assert_array_equal(per_book[b][f], want[f], err_msg=f"book {b} {f}")
            np.testing.assert_array_equal(books.results(b)[f], chains[b].results()[f])
        np.testing.assert_array_equal(books.run_score[b].cpu().numpy(), want["run_score"])
        np.testing.assert_array_equal(books.run_len[b].cpu().numpy(), want["run_len"])
        assert books.remaining(b) == want["remaining"]
    assert (quota == 0).any() and (per_book[0]["count"][quota == 0] == 0).all()
