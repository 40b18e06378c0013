"""
CPU tests of the multi-agent evaluation entry points at the C boundary (no GPU, no launch): header <-> SIGNATURES <->
library for ppoaf_mat_policy_infer (K20) / ppoaf_eval_scores_step_books, the argument-struct layouts (ctypes against the
static_assert lists in csrc/mat_update.hip and csrc/policy_infer.hip), the ABI version, every host refusal, and
MATPolicy.inference_unsupported_reason() on a CPU policy.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppoaf_hip.h")
CSRC = os.path.join(ROOT, "ppo_and_friends_amd", "csrc")
ENTRY_POINTS = {"ppoaf_mat_policy_infer": ("mat_update.hip", "ppoaf_mat_infer_args_t", "MatInferArgs"),
                "ppoaf_eval_scores_step_books": ("policy_infer.hip", "ppoaf_eval_books_args_t", "EvalBooksArgs")}


@pytest.fixture(scope="module")
def built():
    from ppo_and_friends_amd.csrc import build
    build.build(verbose=False)
    from ppo_and_friends_amd import _lib
    return _lib


def test_header_signatures_and_library_agree(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = built.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/ppoaf_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = built.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args == 2
        assert hasattr(lib, name)
    assert lib.ppoaf_abi_version() == 7 and built.ABI_VERSION == 7
    assert re.search(r"#define\s+PPOAF_ABI_VERSION\s+7\b", src)


def test_entry_points_are_declared_under_cited_comments():
    src = open(HEADER).read()
    want = {"ppoaf_mat_policy_infer": ("mat_policy.py:521-585", "mat_policy.py:701-790", "testing.py:8-175"),
            "ppoaf_eval_scores_step_books": ("testing.py:59-112",)}
    for name, needles in want.items():
        pos = src.index(f"int {name}(")
        comment = src[src.rfind("/*", 0, src.rfind("typedef struct", 0, pos)):pos]
        for needle in needles:
            assert needle in comment, (name, needle)


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_struct_layout_matches_the_static_asserts(built, name):
    source, struct, ctype = ENTRY_POINTS[name]
    text = open(os.path.join(CSRC, source)).read()
    cls = getattr(built, ctype)
    listed = re.findall(r"PPOAF_LAYOUT\(" + struct + r",\s*(\w+),\s*(\d+)\)", text)
    assert [f for f, _ in listed] == [f for f, _ in cls._fields_], "every field, in order"
    for field, off in listed:
        assert getattr(cls, field).offset == int(off), field
    size = re.search(r"static_assert\(sizeof\(" + struct + r"\)\s*==\s*(\d+)", text)
    assert size and C.sizeof(cls) == int(size.group(1))
    # and the header declares the fields in the same order
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct, re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)).group(1)
    names = [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\**\s+", "", decl.strip()).split(",")]
    assert names == [f for f, _ in cls._fields_]


def mat_offsets(O, NA, D=64):
    """Offset table of MATActorCritic's parameters in module order, every tensor padded to 4 floats."""
    sizes = [D * (NA + 1)] + [D] * 8 + [D * D, D] * 8 + [D * D, D] * 2 + [D * D, D, D, D, NA * D, NA]
    sizes += [O, O, D * O, D] + [D] * 6 + [D * D, D] * 4 + [D * D, D] * 2 + [D * D, D, D, D, D, 1]
    assert len(sizes) == 63
    return np.concatenate([[0], np.cumsum([(s + 3) // 4 * 4 for s in sizes])]).astype(np.int64)


def _infer_args(built, **over):
    a = built.MatInferArgs()
    a.obs_dim, a.num_agents, a.num_actions, a.embedding = 18, 3, 5, 64
    sizes = {k: over.pop(k) for k in ("obs_dim", "num_agents", "num_actions") if k in over}
    for k, v in sizes.items():
        setattr(a, k, v)
    if 1 <= a.obs_dim <= 64 and 1 <= a.num_actions <= 8:
        for i, o in enumerate(mat_offsets(a.obs_dim, a.num_actions)[:63]):
            a.offsets[i] = int(o)
    a.params = a.obs = a.action_out = 0x10000              # never dereferenced: every case below is refused on the host
    a.E, a.mode = 32, 1
    a.obs_env_stride, a.obs_agent_stride, a.act_env_stride, a.act_agent_stride = 3, 1, 3, 1
    for i in range(a.num_agents if 1 <= a.num_agents <= 16 else 0):
        a.slot_agent[i] = i
    for k, v in over.items():
        if k == "slot_agent":
            for i, s in enumerate(v):
                a.slot_agent[i] = s
        elif k == "offset_shift":
            a.offsets[v] += 4
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("over,needle", [
    (dict(params=None), "null pointer"), (dict(obs=None), "null pointer"), (dict(action_out=None), "null pointer"),
    (dict(embedding=32), "embedding=32"), (dict(embedding=128), "embedding=128"),
    (dict(num_agents=0), "sizes"), (dict(num_agents=17), "sizes"), (dict(obs_dim=0), "sizes"), (dict(obs_dim=65), "sizes"),
    (dict(num_actions=0), "sizes"), (dict(num_actions=9), "sizes"),
    (dict(mode=2), "mode=2"), (dict(mode=-1), "mode=-1"), (dict(E=-1), "negative E"),
    (dict(slot_agent=[0, 0, 1]), "not a permutation"), (dict(slot_agent=[0, 1, 3]), "not a permutation"),
    (dict(slot_agent=[-1, 1, 2]), "not a permutation"),
    (dict(params=0x10008), "16-byte aligned"),
    (dict(obs_env_stride=0), "strides"), (dict(obs_agent_stride=-1), "strides"), (dict(act_env_stride=0), "strides"),
    (dict(act_agent_stride=0), "strides"),
    (dict(offset_shift=40), "parameter 40 sits at"),
])
def test_mat_policy_infer_refuses_on_the_host(built, over, needle):
    lib = built.load()
    a = _infer_args(built, **over)
    assert lib.ppoaf_mat_policy_infer(C.byref(a), None) == -1
    assert needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error()


def test_mat_policy_infer_null_args_and_empty_batch(built):
    lib = built.load()
    assert lib.ppoaf_mat_policy_infer(None, None) == -1 and "null args" in lib.ppoaf_last_error().decode()
    for order in ([0, 1, 2], [2, 0, 1]):
        a = _infer_args(built, E=0, slot_agent=order)    # nothing to do: accepted without a launch (no device here)
        assert lib.ppoaf_mat_policy_infer(C.byref(a), None) == 0
    a = _infer_args(built, E=0, num_agents=16, obs_dim=32, num_actions=8)
    assert lib.ppoaf_mat_policy_infer(C.byref(a), None) == 0


def _books_args(built, **over):
    a = built.EvalBooksArgs()
    for f, _ in built.EvalBooksArgs._fields_:
        if f not in ("E", "num_agents", "n_books", "book_mask"):
            setattr(a, f, 0x10000)
    a.E, a.num_agents, a.n_books = 8, 3, 4
    for b, m in enumerate([1, 2, 4, 7]):
        a.book_mask[b] = m
    for k, v in over.items():
        if k == "masks":
            for b, m in enumerate(v):
                a.book_mask[b] = m
        else:
            setattr(a, k, v)
    return a


def test_eval_scores_step_books_refuses_on_the_host(built):
    lib = built.load()
    pointers = [f for f, _ in built.EvalBooksArgs._fields_ if f not in ("E", "num_agents", "n_books", "book_mask")]
    assert len(pointers) == 11
    for missing in pointers:
        a = _books_args(built, **{missing: None})
        assert lib.ppoaf_eval_scores_step_books(C.byref(a), None) == -1, missing
        assert "null pointer" in lib.ppoaf_last_error().decode()
    for over, needle in [(dict(E=-3), "E=-3"), (dict(num_agents=0), "num_agents=0"), (dict(num_agents=17), "num_agents=17"),
                         (dict(n_books=0), "n_books=0"), (dict(n_books=33), "n_books=33"),
                         (dict(masks=[1, 2, 4, 0]), "book_mask[3]"), (dict(masks=[1, 8, 4, 7]), "book_mask[1]"),
                         (dict(masks=[-1, 2, 4, 7]), "book_mask[0]")]:
        a = _books_args(built, **over)
        assert lib.ppoaf_eval_scores_step_books(C.byref(a), None) == -1, over
        assert needle in lib.ppoaf_last_error().decode(), lib.ppoaf_last_error()
    assert lib.ppoaf_eval_scores_step_books(None, None) == -1 and "null args" in lib.ppoaf_last_error().decode()
    assert lib.ppoaf_eval_scores_step_books(C.byref(_books_args(built, E=0)), None) == 0
    a = _books_args(built, num_agents=16, n_books=1, masks=[0xFFFF], E=0)
    assert lib.ppoaf_eval_scores_step_books(C.byref(a), None) == 0


def test_book_wrapper_refuses_host_tensors_and_bad_masks(built):
    import torch
    from ppo_and_friends_amd import kernels as K
    with pytest.raises(built.PpoafError, match="mask"):
        K.EvalScoreBooks(4, 8, "cpu", 2, [1, 4])
    with pytest.raises(built.PpoafError, match="16 agents"):
        K.EvalScoreBooks(4, 8, "cpu", 17, [1])
    with pytest.raises(built.PpoafError):                  # CPU state: no CPU fallback exists
        K.EvalScoreBooks(4, 8, "cpu", 2, [1, 2, 3])


def test_offset_table_is_the_modules_layout():
    """The table the refusal tests send is the one a real MATActorCritic has (so the accepted E == 0 case is a real one)."""
    from ppo_and_friends_amd.networks.multi_agent_transformer import MATActorCritic
    from ppo_and_friends_amd.spaces import Box, Discrete
    ac = MATActorCritic(name="actor_critic", obs_space=Box(-np.inf, np.inf, (18,), np.float32), action_space=Discrete(5),
                        num_agents=3, test_mode=False, seed=1)
    ac.to("cpu")                                           # builds the flat bucket
    base, offs = ac.flat_params.data_ptr(), []
    for _, p in ac.named_parameters():
        offs.append((p.data_ptr() - base) // 4)
    want = mat_offsets(18, 5)
    assert offs == want[:63].tolist() and ac.flat_params.numel() == int(want[63])


def test_a_cpu_mat_policy_names_the_device():
    import torch
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.policies.mat_policy import MATPolicy
    from ppo_and_friends_amd.spaces import Box, Discrete
    cpu = torch.device("cpu")
    box = Box(-np.inf, np.inf, (6,), np.float32)
    env_gen = lambda: SyntheticFixedLengthEnv(4, 6, Discrete(3), 8, cpu, reward="uniform", seed=5, num_agents=2)
    ppo = PPO(env_gen, {"agent": (MATPolicy, box, box, Discrete(3), {})}, device=cpu, random_seed=1, normalize_obs=False,
              normalize_rewards=False, envs_per_proc=4, ts_per_rollout=8, batch_size=8, save_state=False)
    why = ppo.policies["agent"].inference_unsupported_reason()
    assert why and "cpu" in why and "HIP device" in why
