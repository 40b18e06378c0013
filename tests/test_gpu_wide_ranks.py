"""
-m gpu: the wide width pair (256, 512) on N > 1 ranks (PPOPolicy.fused_wide_ranks).  Fresh rank processes share the one GPU
(collectives over gloo, PPOAF_SHARE_DEVICE=1; tests/helpers/wide_ranks_rank.py).  The pair takes the all-reduce route -- fwd_bwd,
wgrad, all-reduce, Adam with its norm pass -- whatever PPOAF_GRAD_EXCHANGE asks for: it has no K17 route (FusedPolicyUpdate.__init__
says why), so no test here starts one.  Shapes: E 8, T 16, O 8, Discrete(4), depth 2, B 24 over 128 rows (5 full mini-batches of
two row tiles and a tail of 8), two epochs; the steered mini-batches have B 32.

  * replicas: two ranks with their own envs under PPOAF_GRAD_EXCHANGE = auto and = rccl: parameters, Adam moments, value
    normaliser bitwise identical on both ranks, the two runs bitwise equal, description() names the route that ran;
    with the attribute off PPO(update_mode="fused") raises what it raised, with it on the run trains;
  * identical data on both ranks, no clip: g + g times 1/2 is g, so both ranks end bit for bit where the single-rank run,
    started from the same weights, ends;
  * one steered mini-batch per rank (other rows on each) against float64: the gradient bucket after the all-reduce against the
    sum of the ranks' float64 gradients, times grad_scale, every element; bound per tensor = each rank's bound of
    tests/test_gpu_k12_gradients.py for its rows, added; then the whole mini-batch from a preset optimiser state with the clip
    active: step, m and v against float64 clip + Adam of that sum (that test's state and bound).  Box(17) with fused_wide_heads, 65 inputs with fused_wide_inputs;
  * three ranks (1/3 is no power of two); B 528 with fused_wide_shapes: the passes kernel feeds the all-reduce;
  * ppoaf_ppo_update_chain_allreduce on the split form bitwise against the Python loop; the slab form as it was;
  * a multi-policy run with two wide members (mpe_simple_tag's shape): per member the same assertions;
  * drop_peer_exchange("test") between two iterations leaves the pair on its split-wgrad chain, replicas stay identical.
"""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_gpu_k12_gradients as g12

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import wide_ranks_rank  # noqa: E402

pytestmark = pytest.mark.gpu

RANK_TIME_LIMIT = 150.0          # seconds per multi-process run, as the suite's other rank helpers get
TRAIN = dict(E=8, T=16, O=8, B=24, normalize_values=True)
SAME = dict(TRAIN, normalize_values=False, identical=True)
# the steered mini-batches: B 32 = two row tiles; value normaliser on (the records of R ranks are merged), Huber, both clip
# branches -- the steering of tests/test_gpu_k12_gradients.py
BASE = g12.case(O=8, ha=256, hc=512, depth=2, B=32, head=("categorical", 4), act="relu", seed=600)
HEADS = g12.case(O=8, ha=256, hc=512, depth=2, B=32, head=("gaussian", 17), act="tanh", seed=617)
INPUTS = g12.case(O=65, ha=256, hc=512, depth=2, B=32, head=("categorical", 4), act="leaky_relu", seed=665)
B528 = g12.case(O=8, ha=256, hc=512, depth=2, B=528, head=("categorical", 4), act="relu", seed=628)
GRADS = [("base", BASE, ()), ("heads", HEADS, ("fused_wide_heads",)), ("inputs", INPUTS, ("fused_wide_inputs",))]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _spawn(out_dir, name, world, sc):
    """`world` fresh processes under one time limit; the first rank that fails ends the run (and the test)."""
    ctx = mp.spawn(wide_ranks_rank.rank_main, args=(world, _free_port(), out_dir, name, sc), nprocs=world, join=False)
    deadline = time.monotonic() + RANK_TIME_LIMIT
    while not ctx.join(timeout=1.0):                    # (raises when a rank failed; the others are ended with it)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"{name}: the {world} ranks did not finish within {RANK_TIME_LIMIT:.0f} s")
    return [torch.load(os.path.join(out_dir, f"{name}_rank{r}.pt"), weights_only=False) for r in range(world)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every multi-process run once, started on demand, shared by the tests; after a run that failed no other is started."""
    out, done = str(tmp_path_factory.mktemp("wide_ranks")), {}
    scenarios = {
        "auto": (2, dict(mode="auto", train=TRAIN, grads=GRADS)),
        "rccl": (2, dict(mode="rccl", train=TRAIN)),
        "same_two": (2, dict(mode="auto", train=dict(SAME, w0_from="same_single"))),
        "same_single": (1, dict(mode="auto", train=SAME)),
        "three": (3, dict(mode="auto", train=TRAIN, grads=GRADS[:1])),
        "rows528": (2, dict(mode="auto", train=dict(TRAIN, T=80, B=528, shapes=True), grads=[("b528", B528, ("fused_wide_shapes",))])),
        "members": (2, dict(mode="auto", members=TRAIN)),
        "drop": (2, dict(mode="auto", refusal=True, train=dict(TRAIN, drop=True))),
    }

    def get(name):
        if name not in done:
            if None in done.values():                   # a rank failed or ran out of time: no further process is started
                pytest.fail(f"not starting {name!r}: the run {[k for k, v in done.items() if v is None][0]!r} failed")
            done[name] = None
            world, sc = scenarios[name]
            done[name] = _spawn(out, name, world, sc)
        if done[name] is None:
            pytest.fail(f"the run {name!r} failed in an earlier test")
        return done[name]
    return get


def _replicas_identical(ranks, what):
    t0 = ranks[0]["train"]
    for r in ranks[1:]:
        t = r["train"]
        assert torch.equal(t0["w0"], t["w0"]), f"{what}: rank-0 broadcast of the policy bucket"
        for k in ("w", "exp_avg", "exp_avg_sq", "steps"):
            assert torch.equal(t0[k], t[k]), f"{what}: {k} differs between ranks, max |d| {float((t0[k] - t[k]).abs().max()):.3e}"
        assert t0["stats"] == t["stats"], what
        if t0["vn"] is not None:
            assert torch.equal(t0["vn"], t["vn"]), what
    for r in ranks:
        t = r["train"]
        assert not torch.equal(t["w"], t["w0"]) and torch.isfinite(t["w"]).all(), f"{what}: the run trained"
        assert t["guard"] is True and t["healed"] is False, f"{what}: _guard_replicas found the replicas apart"
        assert t["multi"] and t["world"] == len(ranks) and t["split"] and "wide pair" in t["tail"], what


def _route_ran(t, iterations=1):
    """description() names the all-reduce route, and its collective ran once per mini-batch; no K17 object, no graph."""
    n = 2 * t["minibatches_per_epoch"] * iterations
    for d in t["descriptions"]:
        assert "split-wgrad chain, wgrad and Adam launches" in d and f"N > 1 ({t['world']} ranks): all-reduce route" in d, d
        assert "no K17 route" in d and "K17 route --" not in d and "slab chain" not in d, d
    assert t["exchanged"] == [None] * iterations and t["graphs"] == [] and t["allreduce_calls"] == n, (t["exchanged"], t["allreduce_calls"])


# ---------------------------------------------------------------------------------------------------- replicas
@pytest.mark.parametrize("name", ["auto", "rccl"])
def test_replicas_stay_identical(runs, name):
    ranks = runs(name)
    _replicas_identical(ranks, name)
    assert not torch.equal(ranks[0]["train"]["obs"], ranks[1]["train"]["obs"]), "each rank rolls out its own envs"
    for r in ranks:
        _route_ran(r["train"])
    assert ranks[0]["train"]["minibatches_per_epoch"] == 6


def test_whatever_exchange_is_asked_for_the_same_route_runs(runs):
    """PPOAF_GRAD_EXCHANGE = auto and = rccl reach the one route this pair has: what this shows is that `auto` opens no peer
    exchange for it (no other code path runs, so the two trainings are the same bits) and that the route is deterministic
    from one job to the next."""
    a, b = runs("auto")[0]["train"], runs("rccl")[0]["train"]
    for k in ("w0", "w", "exp_avg", "exp_avg_sq", "steps", "vn"):
        assert torch.equal(a[k], b[k]), f"{k}: max |d| {float((a[k] - b[k]).abs().max()):.3e}"
    assert a["stats"] == b["stats"]


def test_identical_data_ends_where_one_rank_ends(runs):
    single, = runs("same_single")
    ranks = runs("same_two")
    _replicas_identical(ranks, "identical data")
    assert torch.equal(ranks[0]["train"]["obs"], ranks[1]["train"]["obs"]) and torch.equal(single["train"]["obs"], ranks[0]["train"]["obs"])
    assert not single["train"]["multi"] and single["train"]["descriptions"][0].count("N > 1") == 0
    for r in ranks:
        _route_ran(r["train"])
        for k in ("w0", "w", "exp_avg", "exp_avg_sq", "steps"):
            a, b = single["train"][k], r["train"][k]
            assert torch.equal(a, b), f"{k} is not the single-rank run's, max |d| {float((a - b).abs().max()):.3e}"


# ---------------------------------------------------------------------------------------------------- one mini-batch
def _gradient_case_holds(ranks, name, world):
    for r in ranks:
        g, = [x for x in r["grads"] if x["name"] == name]
        where = f"{name}, {world} ranks: "
        print(f"{where}worst |sum - float64 sum| / bound {g['worst']:.3f} at {g['worst_at']}; {g['description']}")
        assert g["grad_scale"] == float(np.float32(1.0 / world)) and g["bucket"] == g["elements"] + g["padding"], where
        assert "all-reduce route" in g["description"], g["description"]
        assert not g["local_failures"], where + "this rank's own gradient: " + "; ".join(g["local_failures"][:6])
        assert not g["local_padding_written"] and not g["padding_written"], where + "padding of the gradient bucket written"
        assert g["finite"] and g["differs_from_local"], where
        assert g["outside"] == 0 and g["worst"] <= 1.0, where + f"{g['outside']} elements outside the bound, worst {g['worst']:.3g} x"
        # the whole mini-batch with the clip active (coefficient 0.25 on the network with the smaller norm): Adam's norm pass at
        # grad_scale 1 / R, the parameter step and both moments against float64
        print(f"{where}clipped step, m, v: worst {g['step_worst']:.3f} of the bound; coefficients {g['clip_coefficients']}")
        assert not g["step_failures"], where + "clip + Adam after the all-reduce: " + "; ".join(g["step_failures"][:6])
        assert g["steps_after"] == [7, 10] and max(g["clip_coefficients"]) < 1.0, where
    assert len({(g["worst"], g["worst_at"]) for r in ranks for g in r["grads"] if g["name"] == name}) == 1, "every rank holds the same sum"


@pytest.mark.parametrize("name", ["base", "heads", "inputs"])
def test_exchanged_gradient_against_float64(runs, name):
    _gradient_case_holds(runs("auto"), name, 2)


def test_three_ranks(runs):
    ranks = runs("three")
    _replicas_identical(ranks, "three ranks")
    for r in ranks:
        _route_ran(r["train"])
    _gradient_case_holds(ranks, "base", 3)


def test_more_than_512_rows_feed_the_all_reduce(runs):
    ranks = runs("rows528")
    _replicas_identical(ranks, "B 528")
    for r in ranks:
        t = r["train"]
        assert t["passes"] and t["minibatches_per_epoch"] == 2 and "fused_wide_shapes" in t["descriptions"][0]
        _route_ran(t)
        assert r["grads"][0]["passes"]
    _gradient_case_holds(ranks, "b528", 2)


# ---------------------------------------------------------------------------------------------------- around it
def test_fused_mode_refuses_without_the_attribute_and_trains_with_it(runs):
    for r in runs("drop"):
        why = r["train"]["refusal"]
        assert why.startswith("update_mode='fused' but policy p: wide pair (actor 256, critic 512): single rank only for now (2 ranks)"), why
        assert why.endswith("; PPOPolicy.fused_wide_ranks = True would take it on the fused kernels"), why      # (verbose)
        assert not torch.equal(r["train"]["w"], r["train"]["w0"])


def test_dropping_the_peer_exchange_leaves_the_split_chain(runs):
    """PPO._heal_replicas calls drop_peer_exchange on every driver, a wide pair's included.  That driver holds no exchange, so
    nothing is closed here; what the call still does is ask _split_wanted again and drop the split workspace and the args.
    Shown: the pair stays on the split-wgrad chain (no slab chain exists for it), the workspace is laid out anew, and the next
    iteration trains on the all-reduce route with replicas bitwise identical."""
    ranks = runs("drop")
    _replicas_identical(ranks, "after drop_peer_exchange")
    for r in ranks:
        t = r["train"]
        _route_ran(t, iterations=2)
        assert not torch.equal(t["w_0"], t["w_1"]) and torch.equal(t["w_1"], t["w"])
    assert torch.equal(ranks[0]["train"]["w_0"], ranks[1]["train"]["w_0"])


def test_two_wide_members_in_one_run(runs):
    """mpe_simple_tag's shape under MAPPO: two 256/512 policies in one PPO, one of them shared by two agents, on two ranks.  Each
    has a driver of its own (its split workspace, its norm partials re-laid out), both go through the one all-reduce loop."""
    ranks = runs("members")
    assert sorted(ranks[0]["members"]) == ["adv", "good"]
    assert ranks[0]["members"]["adv"]["bucket"] != ranks[0]["members"]["good"]["bucket"]        # (so the counts are per policy)
    for pid, per_epoch in (("adv", 6), ("good", 11)):
        view = [{"train": r["members"][pid]} for r in ranks]
        _replicas_identical(view, f"member {pid}")
        for v in view:
            assert v["train"]["fused_step"] == "" and v["train"]["minibatches_per_epoch"] == per_epoch, pid
            _route_ran(v["train"])                          # one all-reduce of this policy's bucket per mini-batch: 2 x per_epoch


def _fallback(helper, loop, **env):
    e = dict(os.environ, PPOAF_REHEARSE_MULTI_RANK="1", PPOAF_GRAD_EXCHANGE="rccl", PPOAF_TEST_RCCL_LOOP=loop, MASTER_ADDR="127.0.0.1",
             MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PPOAF_BACKEND"):
        e.pop(k, None)
    root = os.path.dirname(HERE)
    p = subprocess.run([sys.executable, os.path.join(HERE, "helpers", helper)], cwd=root, env=e, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_c_loop_equals_the_python_loop():
    """ppoaf_ppo_update_chain_allreduce with a split workspace (fwd_bwd, wgrad, RCCL all-reduce, Adam's norm pass + Adam) against
    FusedPolicyUpdate._one's all-reduce route: the same launches in the same order, bitwise equal parameters and moments.  For a
    slab pair the C loop stays bitwise what the Python loop -- code this feature does not touch -- computes
    (tests/helpers/rccl_fallback_run.py, unchanged)."""
    outs = {loop: _fallback("wide_ranks_fallback_run.py", loop) for loop in ("c", "python")}
    assert outs["c"]["c_loop"] is True and outs["python"]["c_loop"] is False
    for o in outs.values():
        assert o["wide"] and o["split"] and o["multi"] and not o["peer_exchange"] and "all-reduce route" in o["description"], o
        assert o["steps"] == 2 * 2 * 6                            # iterations x epochs x (5 full mini-batches + the tail)
    assert outs["c"]["digest"] == outs["python"]["digest"], outs
    slabs = {loop: _fallback("rccl_fallback_run.py", loop, PPOAF_FALLBACK_KIND="ppo") for loop in ("c", "python")}
    assert slabs["c"]["c_loop"] is True and slabs["python"]["c_loop"] is False
    assert slabs["c"]["digest"] == slabs["python"]["digest"] and slabs["c"]["steps"] == 2 * 2 * (16 * 32 // 64), slabs
