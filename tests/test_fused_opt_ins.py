"""
CPU tests of the host code that decides which fused kernels a policy runs on (fused_update.FusedOptIns, describe_policy,
describe_policy_icm, the `*_would_take` questions and opt_in_hint).  Nothing is launched.

  * purity: no scope question writes to the policy it asks about, or to PPOPolicy -- on one and on two ranks, with an opt-in
    absent from the instance, and with a False set by hand under a class attribute of True;
  * reading: FusedOptIns.of sees class-level and instance-level attributes, lets `fused_wide_shapes` imply
    `fused_wide_inputs`, and is all False for an object with none of the attributes;
  * one description: the descriptors FusedPolicyUpdate.unsupported_reason hands the library's check, those in rollout_step's
    args and those in _infer_step's args are describe_policy's, field for field, and so is the head;
  * hint precedence: the clause `verbose` appends under "auto" and under "fused", on one and on two ranks.
"""
import numpy as np
import pytest
import torch

from test_icm_wide_actions_scope import _cpu_policy as _icm_policy
from test_wide_heads_scope import _ppo

FLAGS = ("action_heads", "wide_critic", "wide_inputs", "wide_shapes", "wide_heads", "wide_ranks", "shared_icm", "wide_icm_actions")
BATCHES = (64, 513)
FUSED_MODE = "; update_mode='fused' would take it on the fused kernels"
HEADS = "; PPOPolicy.fused_wide_heads = True would take it on the fused kernels"
RANKS = "; PPOPolicy.fused_wide_ranks = True would take it on the fused kernels"
AUTO_HEADS = "; update_mode='fused' with PPOPolicy.fused_wide_heads = True would take it on the fused kernels"
AUTO_RANKS = "; update_mode='fused' with PPOPolicy.fused_wide_ranks = True would take it on the fused kernels"


@pytest.fixture(scope="module")
def pols():
    """4-wide observations; 64/64 and the 256/512 pair; Discrete(2), Discrete(18), Box(17), MultiDiscrete; a 65-wide observation;
    an identity-encoder ICM over Discrete(18).  Built once, only read."""
    from ppo_and_friends_amd.spaces import Box, Discrete, MultiDiscrete
    box17 = Box(-0.4, 0.4, (17,), np.float32)
    p = {"narrow": _ppo("auto", Discrete(2), O=4, ha=64, hc=64),
         "wide_auto": _ppo("auto", Discrete(2), O=4), "wide_fused": _ppo("fused", Discrete(2), O=4),
         "d18_auto": _ppo("auto", Discrete(18), O=4), "d18_fused": _ppo("fused", Discrete(18), O=4),
         "box17_fused": _ppo("fused", box17, O=4), "md_fused": _ppo("fused", MultiDiscrete([3, 2, 3]), O=4, ha=64, hc=64),
         "o65_fused": _ppo("fused", Discrete(2), O=65), "d18_o65_auto": _ppo("auto", Discrete(18), O=65),
         "d18_o65_fused": _ppo("fused", Discrete(18), O=65)}
    p = {k: v.policies["p"] for k, v in p.items()}
    p["icm18"] = _icm_policy(18, encoded_obs_dim=0, inverse_hidden_size=32, forward_hidden_size=64)
    return p


@pytest.fixture(params=[1, 2])
def ranks(request, monkeypatch):
    from ppo_and_friends_amd.utils import mpi_utils
    monkeypatch.setattr(mpi_utils, "get_num_procs", lambda: request.param)
    return request.param


# ------------------------------------------------------------------------------------------------------------ purity
def _ask_everything(pol):
    from ppo_and_friends_amd import fused_update as fu
    F, I = fu.FusedPolicyUpdate, fu.FusedIcmUpdate
    answers = []
    for B in BATCHES:
        answers += [F.unsupported_reason(pol, B), F.fused_mode_would_take(pol, B), F.wide_heads_would_take(pol, B),
                    F.wide_ranks_would_take(pol, B), I.unsupported_reason(pol, B), I.wide_actions_would_take(pol, B),
                    fu.opt_in_hint(pol, B, "auto"), fu.opt_in_hint(pol, B, "fused")]
    answers.append(fu.describe_policy(pol)[1])
    if pol.enable_icm:
        answers.append(fu.describe_policy_icm(pol)[1])
    return answers


def _class_state():
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    return {f: vars(PPOPolicy).get("fused_" + f, "absent") for f in FLAGS}


def test_no_question_writes_to_the_policy_or_the_class(pols, ranks):
    for name, pol in pols.items():
        before, cls_before = dict(vars(pol)), _class_state()
        answers = _ask_everything(pol)
        after = dict(vars(pol))
        assert list(after) == list(before) and all(after[k] is before[k] for k in before), name
        assert _class_state() == cls_before, name
        assert answers == _ask_everything(pol), name             # (and asking twice gives the same answers)
    # the questions were not all trivially refused: each of these is a hypothetical that is answered with yes
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate, FusedPolicyUpdate as F
    assert F.wide_heads_would_take(pols["d18_fused"], 64) == (ranks == 1)
    assert F.fused_mode_would_take(pols["wide_auto"], 64) == (ranks == 1)
    assert F.wide_ranks_would_take(pols["wide_fused"], 64) == (ranks == 2)
    assert FusedIcmUpdate.wide_actions_would_take(pols["icm18"], 64) is True


def test_an_absent_and_a_hand_set_instance_attribute_survive(pols, ranks, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate as F
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    pol = pols["d18_fused"]
    for flag in ("fused_wide_heads", "fused_wide_ranks", "fused_wide_inputs", "fused_wide_shapes", "fused_wide_icm_actions"):
        assert flag not in vars(pol)
    _ask_everything(pol)
    for flag in ("fused_wide_heads", "fused_wide_ranks", "fused_wide_inputs", "fused_wide_shapes", "fused_wide_icm_actions"):
        assert flag not in vars(pol), flag
    # a False set by hand under a class attribute of True: read as False, left as it is
    monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)
    monkeypatch.setattr(PPOPolicy, "fused_wide_ranks", True)
    assert F.unsupported_reason(pol, 64) == "" and not F.wide_heads_would_take(pol, 64)
    monkeypatch.setitem(vars(pol), "fused_wide_heads", False)
    assert F.unsupported_reason(pol, 64) == "actor: output width 18 > 8"
    assert F.wide_heads_would_take(pol, 64)
    _ask_everything(pol)
    assert vars(pol)["fused_wide_heads"] is False and "fused_wide_ranks" not in vars(pol)
    assert PPOPolicy.fused_wide_heads is True and PPOPolicy.fused_wide_ranks is True


# ----------------------------------------------------------------------------------------------------------- reading
def test_opt_ins_are_read_from_the_class_and_from_the_instance(pols, monkeypatch):
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.fused_update import WIDE_HEAD_MAX, FusedOptIns
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    assert FusedOptIns._fields == FLAGS
    none = FusedOptIns(*[False] * len(FLAGS))
    assert FusedOptIns() == none and FusedOptIns.of(object()) == none and FusedOptIns.of(pols["wide_auto"]) == none
    assert FusedOptIns.of(pols["wide_fused"]) == none._replace(action_heads=True, wide_critic=True)
    assert all(type(v) is bool for v in FusedOptIns.of(pols["wide_fused"]))
    pol = pols["wide_auto"]
    for flag in FLAGS[2:]:
        want = none._replace(**{flag: True})
        if flag == "wide_shapes":
            want = want._replace(wide_inputs=True)               # (it implies the other; the class attribute stays as it is)
        with monkeypatch.context() as mp:
            mp.setattr(PPOPolicy, "fused_" + flag, True)         # class-level
            assert FusedOptIns.of(pol) == want, flag
            mp.setitem(vars(pol), "fused_" + flag, False)        # an instance False under a class True
            assert FusedOptIns.of(pol) == none, flag
        with monkeypatch.context() as mp:
            mp.setitem(vars(pol), "fused_" + flag, True)         # instance-level
            assert FusedOptIns.of(pol) == want and getattr(PPOPolicy, "fused_" + flag) is False, flag
        assert FusedOptIns.of(pol) == none and "fused_" + flag not in vars(pol)
    # the value's own answers: the wide pair's option bits and the actor's output limit
    assert (none.wide_bits, none._replace(wide_inputs=True).wide_bits) == (0, _lib.SPLIT_WIDE_INPUTS)
    assert none._replace(wide_inputs=True, wide_shapes=True).wide_bits == _lib.SPLIT_WIDE_SHAPES
    both = none._replace(wide_heads=True, wide_critic=True)
    assert [both.actor_out_limit(h) for h in (K.HEAD_CATEGORICAL, K.HEAD_GAUSSIAN, K.HEAD_MULTI_CATEGORICAL, K.HEAD_BERNOULLI)] \
        == [WIDE_HEAD_MAX, WIDE_HEAD_MAX, 8, 8]
    assert none._replace(wide_heads=True).actor_out_limit(K.HEAD_CATEGORICAL) == 8
    assert none._replace(wide_critic=True).actor_out_limit(K.HEAD_GAUSSIAN) == 8


def test_the_inference_reasons_key_is_the_value(pols, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedOptIns
    pol = _ppo("fused", pols["d18_fused"].action_space, O=4).policies["p"]
    pol.device = torch.device("cuda", 0)                       # (only compared: the question is host-side)
    assert pol.inference_unsupported_reason() == "actor: output width 18 > 8"
    assert pol._infer_reason[0] == (pol.policy_params.data_ptr(), FusedOptIns.of(pol))
    pol.fused_wide_heads = True
    assert pol.inference_unsupported_reason() == "" and pol._infer_reason[0][1].wide_heads is True


# --------------------------------------------------------------------------------------------------- one description
def _fields(desc):
    return {name: getattr(desc, name) for name, _ in type(desc)._fields_}


@pytest.mark.parametrize("name,heads", [("narrow", False), ("wide_fused", False), ("md_fused", False), ("d18_fused", True),
                                        ("box17_fused", True)])
def test_every_consumer_takes_the_descriptors_of_describe_policy(pols, name, heads, monkeypatch):
    """A policy of its own, shaped like pols[name]: the two step sites keep their args on the policy."""
    from ppo_and_friends_amd import _lib
    from ppo_and_friends_amd import kernels as K
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate, describe_policy
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    from ppo_and_friends_amd.spaces import Box
    space, narrow = pols[name].action_space, name in ("narrow", "md_fused")
    ppo = _ppo("auto" if name == "narrow" else "fused", space, O=4, **(dict(ha=64, hc=64) if narrow else {}))
    pol = ppo.policies["p"]
    if heads:
        assert describe_policy(pol) == (None, f"actor: output width {pol.actor.layer_dims()[-1][1]} > 8")
        monkeypatch.setattr(PPOPolicy, "fused_wide_heads", True)
    desc, why = describe_policy(pol)
    assert why == "" and desc.wide == (not narrow)
    assert (desc.actor.hidden, desc.critic.hidden, desc.actor.in_dim, desc.critic.out_dim) == \
        ((64, 64, 4, 1) if not desc.wide else (256, 512, 4, 1))
    assert desc.actor.out_dim == pol.actor.layer_dims()[-1][1] and (desc.actor.log_std_offset >= 0) == isinstance(space, Box)
    want_head = dict(head_kind=desc.head, n_action_slices=len(desc.slices),
                     action_slices=[desc.slices[j] if j < len(desc.slices) else 0 for j in range(8)])
    head_of = lambda a: dict(head_kind=a.head_kind, n_action_slices=a.n_action_slices, action_slices=list(a.action_slices))
    # what the update's scope question hands the library
    lib, asked = _lib.load(), []
    real = lib.ppoaf_ppo_update_check

    def check(ref):
        q = ref._obj
        asked.append((_fields(q.actor), _fields(q.critic), head_of(q), q.bucket_total))
        return real(ref)
    monkeypatch.setattr(lib, "ppoaf_ppo_update_check", check)
    assert FusedPolicyUpdate.unsupported_reason(pol, 64) == ""
    assert asked == [(_fields(desc.actor), _fields(desc.critic), want_head, desc.actor.size + desc.critic.size)]
    # the rollout step's and the inference step's args: built in full before the host refuses the CPU tensors
    pol.initialize_dataset()
    pol.initialize_episodes(4, ppo.status_dict, ts_per_rollout=8)
    obs = torch.zeros(4, 4)
    with pytest.raises(_lib.PpoafError, match="device tensor"):
        pol.rollout_step(0, obs, obs)
    with pytest.raises(_lib.PpoafError, match="obs must hold"):
        pol._infer_step(obs, True)
    step, infer = pol._step_args, pol._infer_state["args"]
    assert _fields(step.actor) == _fields(desc.actor) and _fields(step.critic) == _fields(desc.critic)
    assert _fields(infer.actor) == _fields(desc.actor)
    lo, hi = pol.actor.distribution.bound_tensors() if desc.head == K.HEAD_GAUSSIAN else (None, None)
    for a in (step, infer):
        assert head_of(a) == want_head
        assert a.min_std == np.float32(getattr(pol.actor.distribution, "min_std", 0.01))
        assert (a.act_lo, a.act_hi) == (None if lo is None else lo.data_ptr(), None if hi is None else hi.data_ptr())
        assert a.params == pol.policy_params.data_ptr() and a.E == 4
    assert step.critic.offset == step.actor.size and isinstance(step, _lib.PolicyStepArgs) and isinstance(infer, _lib.PolicyInferArgs)


def test_describe_policy_refuses_in_the_order_of_the_scope_question(pols):
    from ppo_and_friends_amd.fused_update import FusedOptIns, FusedPolicyUpdate, describe_policy
    for name, pol in pols.items():
        if name == "icm18":
            continue
        for opt in (None, FusedOptIns.of(pol)._replace(wide_critic=True), FusedOptIns.of(pol)._replace(wide_critic=True, wide_heads=True)):
            desc, why = describe_policy(pol, opt)
            assert (desc is None) == (why != ""), name
            if why:                                              # what describe_policy refuses, the scope question refuses so
                assert FusedPolicyUpdate.unsupported_reason(pol, 64, opt) == why, name
    assert describe_policy(pols["wide_auto"])[1] == "critic: hidden width 512 is not one of the instantiated widths (32, 64, 128, 256)"
    assert describe_policy(pols["d18_auto"])[1] == "actor: output width 18 > 8"          # (the actor is asked first)


def test_the_policys_icm_chain_is_described_once(pols):
    from ppo_and_friends_amd.fused_update import FusedIcmUpdate, FusedOptIns, describe_icm_chain, describe_policy_icm
    pol = pols["icm18"]
    refusal = "action widths (18, 18) must be in [1, 8]"
    assert describe_policy_icm(pol) == (None, refusal) and FusedIcmUpdate.unsupported_reason(pol, 8) == refusal
    on = FusedOptIns.of(pol)._replace(wide_icm_actions=True)
    topo, why = describe_policy_icm(pol, on)
    assert why == "" and topo["identity"] is True and topo["action_dim"] == 18 and FusedIcmUpdate.unsupported_reason(pol, 8, on) == ""
    assert (topo, why) == describe_icm_chain(pol.icm_model, pol.action_dtype, wide_actions=True)
    assert "fused_wide_icm_actions" not in vars(pol)


# ---------------------------------------------------------------------------------------------------- hint precedence
#  (policy, update_mode, fused_wide_ranks on the class) -> the clause on one rank, on two ranks.  The questions behind it:
#  fused mode = "taken with fused_wide_critic on"; heads / ranks = "taken with that opt-in AND fused_wide_critic on".  So under
#  "auto" a wide pair on two ranks misses fused mode and ranks, which is what the ranks clause of "auto" names; Discrete(18)
#  there misses heads and ranks -- two opt-ins of PPOPolicy at once -- and gets no clause.  None: the policy is covered, so
#  nothing is refused and the clause is not asked for.
HINTS = [
    ("wide_auto", "auto", False, FUSED_MODE, AUTO_RANKS),        # missing only fused mode / (two ranks) only ranks beside it
    ("wide_auto", "auto", True, FUSED_MODE, FUSED_MODE),         # ... fused mode comes first although the heads question says yes too
    ("wide_fused", "auto", False, None, AUTO_RANKS),             # fused_wide_critic set by hand: covered / missing only ranks
    ("d18_auto", "auto", False, AUTO_HEADS, ""),                 # missing only heads / heads and ranks: no clause
    ("d18_auto", "auto", True, AUTO_HEADS, AUTO_HEADS),
    ("d18_o65_auto", "auto", False, "", ""),                     # heads and inputs
    ("d18_o65_auto", "auto", True, "", ""),
    ("narrow", "auto", False, None, None),
    ("wide_fused", "fused", False, None, RANKS),                 # covered / missing only ranks
    ("wide_fused", "fused", True, None, None),
    ("d18_fused", "fused", False, HEADS, ""),                    # missing only heads / heads and ranks
    ("d18_fused", "fused", True, HEADS, HEADS),
    ("box17_fused", "fused", False, HEADS, ""),
    ("o65_fused", "fused", False, "", ""),                       # inputs: the refusal itself names that opt-in
    ("d18_o65_fused", "fused", False, "", ""),                   # heads and inputs
    ("d18_o65_fused", "fused", True, "", ""),
]


@pytest.mark.parametrize("name,mode,ranks_on,one,two", HINTS)
def test_hint_precedence(pols, name, mode, ranks_on, one, two, ranks, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedPolicyUpdate as F, opt_in_hint
    from ppo_and_friends_amd.policies.ppo_policy import PPOPolicy
    monkeypatch.setattr(PPOPolicy, "fused_wide_ranks", ranks_on)
    pol, want = pols[name], one if ranks == 1 else two
    if want is None:
        assert F.unsupported_reason(pol, 64) == ""
        return
    got = opt_in_hint(pol, 64, mode)
    assert F.unsupported_reason(pol, 64) != "" and got == want, (got, F.unsupported_reason(pol, 64))
    # the clause is the first question that says yes, in the order of its mode
    order = [(F.wide_heads_would_take, HEADS if mode == "fused" else AUTO_HEADS), (F.wide_ranks_would_take, RANKS if mode == "fused" else AUTO_RANKS)]
    if mode == "auto":
        order.insert(0, (F.fused_mode_would_take, FUSED_MODE))
    assert got == next((text for would, text in order if would(pol, 64)), "")


def test_auto_prints_the_hint_under_verbose_only(capsys):
    """PPO._fused_updater under "auto" (where "fused" raises with it, a device is needed: tests/test_gpu_wide_ranks.py)."""
    from ppo_and_friends_amd.spaces import Discrete
    ppo = _ppo("auto", Discrete(18), O=4)
    ppo.verbose, ppo.device = True, torch.device("cuda", 0)     # (the device is only compared)
    assert ppo._fused_updater("p", 64) is None
    assert f"policy p: torch update path (actor: output width 18 > 8){AUTO_HEADS}" in capsys.readouterr().out
    ppo.verbose = False
    ppo._fused.clear()
    assert ppo._fused_updater("p", 64) is None and "would take" not in capsys.readouterr().out
