"""
-m gpu: TWO whole update epochs of K12 through the package's own driver (FusedPolicyUpdate.begin_epoch / run_epoch /
end_epoch) against the float64 chain oracle (oracle/epoch_oracle.py: k12_oracle.minibatch -> clip_adam, mini-batch after
mini-batch; pinned to cpu_ppo_loop.CpuPPO.train_epoch on fixture g12_c2_cut by tests/test_epoch_oracle.py).  What an epoch
has and a single mini-batch has not: the device cursor and the offsets baked into a captured chunk, the graph_chunk schedule
(warm-up, capture, replay, eager remainder), the tail mini-batch with arguments of its own, the one-row tail that only
feeds the normaliser (Q9), the normaliser's two slots, the per-mini-batch records, Adam's counters and bias correction
advancing on the device, the launch tag carried from one fused tail to the next, the totals, `values` written back for
every row, and a second epoch that restarts the cursor and reuses graphs and argument blocks.

The cases and their steering are tests/helpers/epoch_cases.py (built on the CPU from shapes and a seed; the conditions on
them are asserted by tests/test_epoch_oracle.py).  After one rollout the test overwrites the bucket, all N dataset rows, the
normaliser, and the optimiser state (steps (6, 9), m and v on the gradient's scale), shrinks the driver's graph_chunk to 2
or 3, and runs two epochs with different shuffles.

After EACH epoch, per tensor |x - x64| <= 1e-5 |x64| + 1e-5 max|x64|, raised to 4 max|x32 - x64| of the float32 chain
(ko.deviations): the parameter step over the epoch, m and v per parameter tensor; the normaliser's mean and variance as
published; the nine totals as one tensor; all of buffer.values.  Exact: the step counters, the normaliser's count, n_done,
the cursor, the padding of params / m / v, and `values` of the rows no mini-batch held.

A failure names the case, its form, the epoch and the tensors; `chain_eager` is `chain_graphs` without graphs, so the two
together say whether the eager launches of the same case pass.

MEASURED (worst deviation / bound per driver and form, one MI355X; every case passed, no bug found):
  k12 chain           0.742  lean_128 epoch 1 step: critic.3.weight
  k12 chain eager     0.680  chain_eager epoch 0 step: actor.1.bias
  k12 row_tiles       0.494  row_tiles epoch 0 step: critic.0.bias
  k12 slabs           0.476  slabs epoch 1 step: actor.2.bias
  k12 three_launches  0.525  three_launches epoch 0 step: actor.2.bias
K22, K15 and K14 have no chain yet.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import epoch_cases as ec  # noqa: E402
import test_gpu_k12_gradients as g12  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}                     # (driver, form) -> (worst fraction of the bound, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{d:5s} {f:15s} {v[0]:.3f}  {v[1]}" for (d, f), v in sorted(WORST.items())]
    print("\nworst deviation / bound per driver and form:\n" + "\n".join(lines))
    out = os.environ.get("PPOAF_EPOCH_REPORT")
    if out:
        with open(out, "w") as fh:
            json.dump({f"{d}/{f}": v for (d, f), v in sorted(WORST.items())}, fh, indent=1)


def _ppo(s):
    """test_gpu_k12_gradients._ppo with the case's geometry: the dataset is exactly the case's N rows."""
    from ppo_and_friends_amd.ppo import PPO
    from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
    from ppo_and_friends_amd.spaces import Box
    c, dev = s.c, torch.device("cuda", 0)
    agents, T, E = c["agents"], s.T, s.E
    space = g12._space(c["head"])
    env_gen = lambda: SyntheticFixedLengthEnv(E, c["O"], space, T, dev, reward="uniform", seed=77, num_agents=agents,
                                              critic_view="policy" if agents > 1 else "local")
    sp, csp = Box(-np.inf, np.inf, (c["O"],), np.float32), Box(-np.inf, np.inf, (c["O"] * agents,), np.float32)
    kw = dict(hidden_size=c["ha"], hidden_depth=c["depth"], activation=g12.ACTS[c["act"]]())
    pargs = dict(actor_kw_args=kw, critic_kw_args=dict(kw, hidden_size=c["hc"]), use_huber_loss=c["huber"],
                 entropy_weight=c["ent"], kl_loss_weight=c["kl"], lr=c["lr"], gradient_clip=s.max_norm)
    return PPO(env_gen, {"p": (None, sp, csp, space, pargs)}, device=dev, random_seed=3, normalize_obs=False,
               normalize_rewards=False, normalize_adv=c["norm_adv"], normalize_values=c["norm_values"], envs_per_proc=E,
               ts_per_rollout=T, batch_size=c["B"], epochs_per_iter=2, use_graphs=c["graphs"], update_mode="fused",
               save_state=False)


def _form(args):
    from ppo_and_friends_amd import _lib
    lib, f = _lib.load(), C.c_int32(-1)
    assert lib.ppoaf_ppo_update_fwd_bwd_form(C.byref(args), C.byref(f)) == 0, lib.ppoaf_last_error()
    return f.value


def run_k12(name, monkeypatch):
    from ppo_and_friends_amd.fused_update import FusedEpoch, FusedPolicyUpdate
    s = ec.built(name)
    c, B, N = s.c, s.c["B"], s.N
    assert not s.problems, "; ".join(s.problems)
    env, pairs = g12.FORMS[c["form"]]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(FusedPolicyUpdate, "row_pairs", pairs)
    monkeypatch.setattr(FusedPolicyUpdate, "graph_chunk", c["chunk"])
    ppo = _ppo(s)
    assert FusedPolicyUpdate.unsupported_reason(ppo.policies["p"], B) == ""
    ppo.rollout()
    pol = ppo.policies["p"]
    pol.train()
    buf, dev = pol.buffer, pol.device
    assert len(pol.dataset) == N and pol.policy_params.numel() == s.size
    assert float(pol.policy_lr[0]) == c["lr"] and float(np.float32(pol.gradient_clip)) == s.max_norm
    rows = buf.row_map[torch.arange(N, device=dev)].long()                  # dataset position -> buffer row
    assert rows.unique().numel() == N
    flat = lambda x: x.view((buf.num_transitions,) + tuple(x.shape[2:]))

    def put(field, x):
        t = flat(getattr(buf, field))
        t[rows] = torch.as_tensor(np.asarray(x)).to(device=dev, dtype=t.dtype).reshape((N,) + tuple(t.shape[1:]))

    dt = lambda x, like: torch.as_tensor(np.asarray(x)).to(device=dev, dtype=like.dtype)
    # ---- everything the epochs read, overwritten: the bucket, all N rows, the normaliser, the optimiser state
    with torch.no_grad():
        pol.policy_params.copy_(dt(s.params, pol.policy_params))
        pol.policy_exp_avg.copy_(dt(s.m0, pol.policy_exp_avg))
        pol.policy_exp_avg_sq.copy_(dt(s.v0, pol.policy_exp_avg_sq))
        pol.policy_step_counts.copy_(dt(ec.STEPS0, pol.policy_step_counts))
    data = s.data()
    for field, x in (("observations", data.obs), ("critic_observations", data.critic_obs), ("raw_actions", data.raw_actions),
                     ("advantages", data.advantages), ("rewards_to_go", data.rewards_to_go), ("log_probs", data.old_log_probs),
                     ("values", s.values0)):
        put(field, x)
    rs = None
    if c["norm_values"]:
        rs = ppo.value_normalizers["p"].running_stats
        rs.mean_t.fill_(s.vn[0]); rs.var_t.fill_(s.vn[1]); rs.count_t.fill_(s.vn[2])
    upd = FusedPolicyUpdate(ppo, "p")
    assert upd.split == (c["form"] != "slabs")
    assert (upd.tail_reason() == "") == (c["form"] in ("chain", "row_tiles") and c["hc"] != 512), upd.tail_reason()
    # ---- two epochs
    got, values_before = [], flat(buf.values).clone()
    launches = FusedEpoch.tail_launches
    for e, perm in enumerate(s.perms):
        want = s.e64[e]
        upd.begin_epoch(torch.as_tensor(perm, dtype=torch.int64, device=dev))
        if e == 0 and c["lean"]:
            assert _form(upd._args_for(B)) == c["lean"]
        upd.run_epoch()
        totals = upd.end_epoch()
        torch.cuda.synchronize()
        where = f"{name} ({c['form']}, graphs {c['graphs']}) epoch {e}"
        # ---- exact
        assert upd.n_done == want["n_done"] and int(upd.cursor.item()) == want["n_done"], where
        assert tuple(pol.policy_step_counts.cpu().tolist()) == want["state"].steps, where
        assert totals[8] == want["totals"][8], where
        if rs is not None:
            assert float(rs.count_t.item()) == want["state"].vn[2], where
        bucket = [t.detach().double().cpu().numpy() for t in (pol.policy_params, pol.policy_exp_avg, pol.policy_exp_avg_sq)]
        for t, what in zip(bucket, ("params", "m", "v")):
            assert not t[s.pad].any(), f"{where}: padding of {what} written"
        values = flat(buf.values)
        touched = torch.zeros(buf.num_transitions, dtype=torch.bool, device=dev)
        ran = np.concatenate([st["rows"] for st in want["steps"]])
        touched[rows[torch.as_tensor(ran, device=dev)]] = True
        assert torch.equal(values[~touched], values_before[~touched]), f"{where}: values outside the mini-batches' rows changed"
        values_before = values.clone()
        vn = (float(rs.mean_t.item()), float(rs.var_t.item()), float(rs.count_t.item())) if rs is not None else s.vn
        got.append(dict(state=ec.eo.State(bucket[0], bucket[1], bucket[2], want["state"].steps, vn,
                                          values[rows].detach().double().cpu().numpy()), totals=np.asarray(totals)))
        # ---- against the float64 chain
        devs = [d for d in s.deviations(got) if d[0] == e]
        _, what, tensor, frac = max(devs, key=lambda d: d[3])
        key = ("k12", c["form"] + ("" if c["graphs"] else " eager"))
        if frac > WORST.get(key, (-1.0, ""))[0]:
            WORST[key] = (frac, f"{name} epoch {e} {what}: {tensor}")
        bad = [f"{w} {t}: {f:.3g} x bound" for _, w, t, f in devs if not f <= 1.0]
        assert not bad, f"{where}: " + "; ".join(bad[:8])
    if c["graphs"]:
        assert list(upd._graphs) == [c["chunk"]], "the chunk was not captured"
    if upd.tail_reason() == "":
        assert FusedEpoch.tail_launches > launches, "the fused tail did not run"


@pytest.mark.parametrize("name", sorted(ec.K12_CASES))
def test_k12_epochs_against_float64(name, monkeypatch):
    run_k12(name, monkeypatch)
