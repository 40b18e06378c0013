"""
CPU tests of the wide width pair (256, 512) on N > 1 ranks (PPOPolicy.fused_wide_ranks): what FusedPolicyUpdate.unsupported_reason
answers with mpi_utils.get_num_procs patched to 2 and 3.  Host checks only: nothing is launched.

  * attribute off: the parent's refusal, word for word;
  * attribute on (with fused_wide_critic): "" at 64 inputs, with fused_wide_inputs at 65, with fused_wide_shapes at B 513, with
    fused_wide_heads at 17 outputs; each of those without its own opt-in keeps the words it has on one rank;
  * PPOAF_SPLIT_WGRAD=0 still refuses; no update_mode sets the attribute; `wide_ranks_would_take` is what verbose asks;
  * on one rank the attribute changes no answer (a table of shapes, some pinned to the parent's literal texts).
"""
import numpy as np
import pytest

from test_k12_wide_critic_scope import TODAY, _ppo
from test_wide_heads_scope import _ppo as _ppo_space

PAIR = "wide pair (actor 256, critic 512)"
RANKS_TODAY = PAIR + ": single rank only for now ({n} ranks)"


def _reason(pol, B):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    return FusedPolicyUpdate.unsupported_reason(pol, B)


@pytest.fixture(scope="module")
def pols():
    """Policies built on one rank (the constructor is not the subject): 8, 64, 65 inputs; Box(17) and Discrete(18) heads."""
    from ppo_and_friends_amd.spaces import Box, Discrete
    p = {O: _ppo("fused", O=O).policies["p"] for O in (8, 64, 65, 129)}
    p["box17"] = _ppo_space("fused", Box(-0.4, 0.4, (17,), np.float32)).policies["p"]
    p["disc18"] = _ppo_space("fused", Discrete(18)).policies["p"]
    p["auto"] = _ppo("auto").policies["p"]
    return p


@pytest.fixture(params=[2, 3])
def ranks(request, monkeypatch):
    from ppo_and_friends_amd.utils import mpi_utils
    monkeypatch.setattr(mpi_utils, "get_num_procs", lambda: request.param)
    return request.param


def test_no_update_mode_sets_the_attribute():
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    assert PPOPolicy.fused_wide_ranks is False
    for mode in ("fused", "auto", "torch"):
        pol = _ppo(mode).policies["p"]
        assert pol.fused_wide_ranks is False and "fused_wide_ranks" not in vars(pol), mode


def test_attribute_off_the_refusal_is_todays(pols, ranks):
    for key, B in ((8, 64), (64, 512), (8, 2)):
        assert _reason(pols[key], B) == RANKS_TODAY.format(n=ranks), key
    assert pols[8].fused_step_unsupported_reason() == RANKS_TODAY.format(n=ranks)
    # what is refused ahead of the rank count on one rank is refused so here
    assert "in_dim 65 / 65 > 64" in _reason(pols[65], 64)
    assert "batch size 513 > 512" in _reason(pols[8], 513)
    assert _reason(pols["box17"], 64) == "actor: output width 17 > 8"
    assert _reason(pols["auto"], 64) == TODAY


def test_attribute_on_takes_the_pair_at_every_shape_of_one_rank(pols, ranks, monkeypatch):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_ranks", True)
    for B in (2, 32, 512):
        assert _reason(pols[64], B) == "", B
    assert pols[64].fused_step_unsupported_reason() == ""
    # each further shape needs its own opt-in, in the words of one rank
    assert "in_dim 65 / 65 > 64" in _reason(pols[65], 64) and "fused_wide_inputs = True" in _reason(pols[65], 64)
    assert "batch size 513 > 512" in _reason(pols[8], 513)
    assert _reason(pols["box17"], 64) == "actor: output width 17 > 8"
    assert _reason(pols["disc18"], 64) == "actor: output width 18 > 8"
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_inputs", True)
        assert _reason(pols[65], 64) == "" and pols[65].fused_step_unsupported_reason() == ""
        assert "in_dim 129 / 129 > 128" in _reason(pols[129], 64)
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_shapes", True)
        assert _reason(pols[8], 513) == "" and _reason(pols[129], 1024) == ""
        assert "batch size 1025 > 1024" in _reason(pols[8], 1025)
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_heads", True)
        assert _reason(pols["box17"], 64) == "" and _reason(pols["disc18"], 64) == ""
        assert pols["box17"].fused_step_unsupported_reason() == ""
    # the attribute does not take the pair by itself: fused_wide_critic does
    assert _reason(pols["auto"], 64) == TODAY


def test_no_slab_form_on_any_rank_count(pols, ranks, monkeypatch):
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_ranks", True)
    monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "0")
    why = _reason(pols[8], 64)
    assert why == f"{PAIR}: PPOAF_SPLIT_WGRAD=0, and the wide pair has no slab form", why


def test_verbose_is_told_that_the_attribute_would_take_the_policy(pols, ranks, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    would = FusedPolicyUpdate.wide_ranks_would_take
    assert would(pols[8], 64) and would(pols[64], 512)
    assert "fused_wide_ranks" not in vars(pols[8]) and pols[8].fused_wide_critic is True
    assert would(pols["auto"], 64) and pols["auto"].fused_wide_critic is False          # ("auto": together with update_mode="fused")
    assert not would(pols[65], 64) and not would(pols["box17"], 64) and not would(pols[8], 513)    # (other opt-ins are missing)
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_inputs", True)
        assert would(pols[65], 64)
    # a False set by hand on the policy under a class attribute of True survives the question
    with monkeypatch.context() as mp:
        mp.setattr(PPOPolicy, "fused_wide_ranks", True)
        assert not would(pols[8], 64)                          # (on: nothing to hint at)
        mp.setitem(vars(pols[8]), "fused_wide_ranks", False)
        assert would(pols[8], 64) and vars(pols[8])["fused_wide_ranks"] is False
        assert _reason(pols[8], 64) == RANKS_TODAY.format(n=ranks)


def test_auto_prints_the_hint_under_verbose(capsys, monkeypatch):
    """The clause `verbose` appends where "auto" keeps the torch path (PPO._fused_updater; where "fused" raises it is
    tests/test_gpu_wide_ranks.py's).  The PPO is built on the CPU and on one rank; its device is only compared afterwards."""
    import torch
    from ppo_and_friends_amd.utils import mpi_utils
    hint = "; update_mode='fused' with PPOPolicy.fused_wide_ranks = True would take it on the fused kernels"
    said = {}
    for ranks in (1, 2):
        ppo = _ppo("auto")
        ppo.verbose = True
        ppo.device = torch.device("cuda", 0)
        with monkeypatch.context() as mp:
            mp.setattr(mpi_utils, "get_num_procs", lambda: ranks)
            assert ppo._fused_updater("p", 64) is None
        said[ranks] = capsys.readouterr().out
    assert f"policy p: torch update path ({TODAY}); update_mode='fused' would take it on the fused kernels" in said[1]
    assert "fused_wide_ranks" not in said[1]
    assert f"policy p: torch update path ({TODAY}){hint}" in said[2], said[2]


def test_on_one_rank_the_attribute_changes_nothing(pols, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    table = [(k, B) for k in pols for B in (2, 64, 512, 513, 1025)]
    opt_ins = ((), ("fused_wide_inputs",), ("fused_wide_shapes",), ("fused_wide_heads",), ("fused_wide_shapes", "fused_wide_heads"))
    for flags in opt_ins:
        with monkeypatch.context() as mp:
            for f in flags:
                mp.setattr(PPOPolicy, f, True)
            off = [_reason(pols[k], B) for k, B in table]
            mp.setattr(PPOPolicy, "fused_wide_ranks", True)
            assert [_reason(pols[k], B) for k, B in table] == off, flags
            assert not any(FusedPolicyUpdate.wide_ranks_would_take(pols[k], B) for k, B in table)
    # ... and with no opt-in they are the parent's: the texts tests/test_k12_wide_critic_scope.py and its neighbours pin
    monkeypatch.setattr(PPOPolicy, "fused_wide_ranks", True)
    assert _reason(pols[8], 64) == "" and _reason(pols[64], 512) == ""
    assert _reason(pols[8], 513) == f"{PAIR}: batch size 513 > 512 (the split-wgrad chain covers batch sizes <= 512)"
    assert _reason(pols[65], 64) == (f"{PAIR}: in_dim 65 / 65 > 64 (the split-wgrad chain's panels cover in_dim <= 64); "
                                     "PPOPolicy.fused_wide_inputs = True takes in_dim <= 128")
    assert _reason(pols[129], 64) == f"{PAIR}: in_dim 129 / 129 > 64 (the split-wgrad chain's panels cover in_dim <= 64)"
    assert _reason(pols["box17"], 64) == "actor: output width 17 > 8"
    assert _reason(pols["auto"], 64) == TODAY


@pytest.mark.parametrize("ranks", [2, 3])
def test_the_attribute_is_part_of_the_inference_reasons_key(ranks, monkeypatch):
    import torch
    from ppo_and_friends_amd.utils import mpi_utils
    # (the policy is built on one rank, as every policy here: PPO's constructor divides torch's host threads by the rank count,
    #  for the rest of the process)
    pol = _ppo("fused").policies["p"]
    monkeypatch.setattr(mpi_utils, "get_num_procs", lambda: ranks)
    pol.device = torch.device("cuda", 0)                   # (only compared: the question is host-side)
    assert pol.inference_unsupported_reason() == RANKS_TODAY.format(n=ranks)
    pol.fused_wide_ranks = True
    assert pol.inference_unsupported_reason() == ""
