"""
The epoch protocol of the fused drivers (fused_update.FusedEpoch) on fabricated state, no GPU: how a bounded in-kernel
wait that ran out is recovered from, voted on across ranks, and how the drivers read their environment switches.
"""
import types

import pytest
import torch

from ppo_and_friends_amd import fused_update
from ppo_and_friends_amd.fused_update import FusedIcmUpdate, FusedMatUpdate, FusedPolicyUpdate


@pytest.fixture(autouse=True)
def _host_stream(monkeypatch):
    """end_epoch synchronises the current stream before it reads the error words: nothing to wait for here."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(synchronize=lambda: None))


def _k12(state):
    """A single-rank K12 driver after an epoch whose launches took both bounded-wait forms (no error yet)."""
    upd = FusedPolicyUpdate.__new__(FusedPolicyUpdate)
    upd.__dict__.update(multi=False, world=1, ppo=types.SimpleNamespace(normalize_values=False), n_full=3, tail=0, n_done=3,
                        cursor=torch.full((1,), 3, dtype=torch.int64), totals=torch.ones(9, dtype=torch.float64),
                        _split_space=torch.zeros(64, dtype=torch.uint8), _pair_region=16, _pairs_used=True,
                        _tail_ctl=torch.zeros(16, dtype=torch.int32), _tail_used=True, _graphs={"x": 1}, _args={"sig": 3})
    upd._split_space[20:].fill_(7)                       # the pairs' records of the failed pass, tagged 1 .. n
    upd._epoch_state = lambda: [state]
    upd.pairs_reason = lambda: "" if not getattr(upd, "_pairs_disabled", "") else "off"
    upd.tail_reason = lambda: "" if not getattr(upd, "_tail_disabled", "") else "off"
    upd._epoch_snapshot = [state.clone()]
    return upd


def test_recovery_restart_zeroes_every_tagged_record_region():
    """Defect 1: a fused-tail failure with row pairs still on.  The redo must not find the failed pass's pair records (they
    carry matching tags), and K14's exchange records start over the same way."""
    state = torch.zeros(4)
    upd = _k12(state)
    upd._tail_ctl[2] = 1                                 # TailCtl.error
    seen = []

    def launch():
        seen.append((upd._split_space.clone(), int(upd.cursor.item()), float(upd.totals.sum()), upd.n_done))
        upd.n_done = 3
    upd._launch_epoch = launch
    upd.end_epoch()
    assert len(seen) == 1 and upd.pairs_reason() == "" and "ran out of time" in upd.tail_reason() + upd._tail_disabled
    region, cursor, totals, n_done = seen[0]
    assert not region.any() and cursor == 0 and totals == 0.0 and n_done == 0

    icm = FusedIcmUpdate.__new__(FusedIcmUpdate)
    icm.__dict__.update(multi=False, cursor=torch.ones(1, dtype=torch.int64), totals=torch.ones(2, dtype=torch.float64),
                        _split_space=torch.full((FusedIcmUpdate._REC_BYTES + 64,), 5, dtype=torch.uint8), _split_fused_layout=1,
                        _fused_used=True, _graphs={}, _args={"sig": 0}, _epoch_snapshot=[state.clone()])
    icm._epoch_state = lambda: [state]
    icm._split_space[:4].view(torch.int32).fill_(1)
    records = []
    icm._launch_epoch = lambda: records.append(icm._split_space[:FusedIcmUpdate._REC_BYTES].clone())
    icm.end_epoch()
    assert len(records) == 1 and not records[0].any() and icm._split_space[FusedIcmUpdate._REC_BYTES:].eq(5).all()
    assert "ran out of time" in icm._fuse_disabled


def test_failed_redo_restores_the_original_snapshot_again(monkeypatch):
    """Defect 2: a failure inside the redo is checked before anything leaves the epoch: the ORIGINAL starting state comes back
    a second time, with the next form off as well, and only a clean pass reaches the normaliser and the totals."""
    state = torch.arange(4, dtype=torch.float32)
    upd = _k12(state)
    upd._tail_ctl[2] = 1
    events, starts = [], []

    def launch():
        starts.append(state.clone())
        state.add_(100.0)                                # the pass trains
        if len(starts) == 1:                             # ... and its row pairs fail this time
            upd._split_space[16:20].view(torch.int32).fill_(1)
            upd._pairs_used = True
        events.append("launch")
    upd._launch_epoch = launch
    upd._publish = lambda: events.append("publish")
    monkeypatch.setattr(fused_update, "_reduce_totals", lambda u, t: events.append("totals"))
    upd.end_epoch()
    assert events == ["launch", "launch", "publish", "totals"]
    assert all(torch.equal(s, torch.arange(4, dtype=torch.float32)) for s in starts)
    assert upd._tail_disabled and upd._pairs_disabled and not upd._graphs


def test_snapshot_for_an_epoch_of_only_a_tail_minibatch():
    """Defect 3: no full mini-batch, but the tail one takes the fused tail: the epoch still starts from a snapshot."""
    state = torch.zeros(4)
    upd = _k12(state)
    upd.n_full, upd.tail, upd._epoch_snapshot, upd.B = 0, 5, None, 8
    upd._args[8] = object()
    upd.pairs_reason = lambda: "off"
    upd._launch_epoch = lambda: None
    upd.run_epoch()
    assert upd._epoch_snapshot is not None


def test_icm_failure_joins_the_ranks_vote(monkeypatch):
    """Defect 4: on N > 1 ranks a failed icm_fused_kernel launch is voted on with the totals, so every rank heals together
    instead of one rank raising while the others wait in the all-reduce."""
    healed, sent = [], []
    icm = FusedIcmUpdate.__new__(FusedIcmUpdate)
    icm.__dict__.update(multi=True, xchg=None, _fused_used=True, _split_space=torch.zeros(64, dtype=torch.uint8),
                        _graphs={}, _args={"sig": 0}, ppo=types.SimpleNamespace(_heal_replicas=healed.append))
    icm._split_space[:4].view(torch.int32).fill_(1)
    monkeypatch.setattr(fused_update.mpi_utils, "allreduce_sum_", lambda t: sent.append(t.clone()) or t)
    out = fused_update._reduce_totals(icm, torch.tensor([3.0, 2.0], dtype=torch.float64))
    assert sent[0][-1] == 1.0 and len(out) == 2 and healed and icm._fuse_disabled


def test_invalid_split_wgrad_switch_raises_in_every_driver(monkeypatch):
    monkeypatch.setenv("PPOAF_SPLIT_WGRAD", "yes")
    desc = types.SimpleNamespace(in_dim=4, hidden=64, depth=2, out_dim=1, size=8)
    monkeypatch.setattr(fused_update, "_describe", lambda *a: (desc, ""))
    monkeypatch.setattr(fused_update, "_describe_icm", lambda *a: (dict(hidden=64, bucket_total=8), ""))
    monkeypatch.setattr(fused_update, "_describe_mat", lambda *a: (dict(num_agents=2, bucket_total=8), ""))
    pol = types.SimpleNamespace(device=torch.device("cpu"), actor=types.SimpleNamespace(distribution=None), critic=None,
                                policy_params=torch.zeros(8), icm_model=types.SimpleNamespace(flat_grads=torch.zeros(8)),
                                action_dtype="discrete")
    ppo = types.SimpleNamespace(policies={"p": pol}, batch_size=4)
    for driver in (FusedPolicyUpdate, FusedIcmUpdate, FusedMatUpdate):
        with pytest.raises(ValueError, match="PPOAF_SPLIT_WGRAD='yes'"):
            driver(ppo, "p")
