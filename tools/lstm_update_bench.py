"""
One update epoch of an LSTM policy with K22 (FusedLstmUpdate, csrc/lstm_update.hip) against the mini-batch loop it replaces
(`pol.fused_lstm_update = False`), at tools/eval_bench.py's `lstm` shape: the reference's cart_pole_lstm networks (4
observations, Discrete(2), H 32, ff 16, S 10, LeakyReLU), E = 4096 envs x T = 128 steps, batch 256.  ONLY this shape is timed.

    python tools/lstm_update_bench.py [--envs 4096] [--steps 128] [--batch 256] [--repeats 5] [--out profiles/lstm_update.txt]

One rollout, then the two legs alternate in one process (a K22 epoch, a loop epoch, ...) on the same dataset; an epoch is
PPO._ppo_batch_train plus a device synchronisation.  Reported: median and spread (min .. max) of `--repeats` alternations
after one warm-up epoch per leg (K22's captures its hipGraphs), the ratio, whether K22's slowest epoch beat the loop's
fastest, and K22's launches per mini-batch from the driver's own counter (eager launches, `use_graphs` off, in a second PPO
object).

Launches per mini-batch of the loop, and the time per launch of both, come from a kernel trace of one leg per run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lstm_update_bench.py --trace-leg loop|k22
    python tools/lstm_update_bench.py --parse 'OUT/**/*_kernel_trace.csv' --minibatches N        # N as the traced run printed it

The traced run warms the leg up, then runs ONE epoch between two launches of a marker kernel that nothing else in a
one-agent run uses (eval_scores_books_kernel on one row), eagerly (`use_graphs` off: a graph replay is one trace entry per
node either way, but the loop never replays).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARKER = "eval_scores_books_kernel"


def make(envs, steps, batch, use_graphs=True):
    import torch
    import eval_bench as B
    from ppo_and_friends_amd import testing
    testing.rank_print = lambda *a, **k: None
    ppo = B.make("lstm", envs, steps)
    ppo.batch_size = batch
    ppo.use_graphs = ppo.use_graphs and use_graphs
    pol = ppo.policies["p"]
    ppo.rollout()
    pol.train()
    torch.cuda.synchronize()
    return ppo, pol


def epoch(ppo, pol, k22):
    import torch
    from ppo_and_friends_amd.ppo import PermutationLoader
    pol.fused_lstm_update = bool(k22)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo._ppo_batch_train(PermutationLoader(pol.dataset, ppo.batch_size, ppo.loader_generator), "p")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(args):
    from ppo_and_friends_amd.fused_update import FusedLstmUpdate
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ppo, pol = make(args.envs, args.steps, args.batch)
    upd = ppo._fused_updater("p", args.batch)
    assert isinstance(upd, FusedLstmUpdate), FusedLstmUpdate.unsupported_reason(pol, args.batch)
    n_items = len(pol.dataset)
    n_mb = (n_items + args.batch - 1) // args.batch
    say(f"shape: cart_pole_lstm networks (H {pol.actor.lstm_hidden_size}, ff {pol.actor.ff_layers.layer_dims()[0][1]}, "
        f"S {pol.actor.sequence_length}), {args.envs} envs x {args.steps} steps = {n_items} items, batch {args.batch}: "
        f"{n_mb} mini-batches per epoch; graphs {'on' if ppo.use_graphs else 'off'}; only this shape was timed")
    for k22 in (True, False):
        epoch(ppo, pol, k22)                               # warm-up: allocations, K22's graph capture
    t = {True: [], False: []}
    for _ in range(args.repeats):
        for k22 in (True, False):
            t[k22].append(epoch(ppo, pol, k22))
    result = dict(envs=args.envs, steps=args.steps, batch=args.batch, minibatches=n_mb, repeats=args.repeats)
    for k22, name in ((True, "k22"), (False, "loop")):
        x = np.asarray(t[k22])
        result[f"{name}_epoch_seconds"] = float(np.median(x))
        result[f"{name}_epoch_spread"] = [float(x.min()), float(x.max())]
        say(f"{name:4s}: epoch seconds median {np.median(x):.4f}  spread {x.min():.4f} .. {x.max():.4f}  "
            f"({np.median(x) / n_mb * 1e6:.1f} us per mini-batch)")
    result["loop_over_k22"] = result["loop_epoch_seconds"] / result["k22_epoch_seconds"]
    result["k22_slowest_below_loop_fastest"] = bool(max(t[True]) < min(t[False]))
    say(f"loop / K22 (medians): {result['loop_over_k22']:.2f}x; K22's slowest epoch {max(t[True]):.4f} s "
        f"{'<' if result['k22_slowest_below_loop_fastest'] else '>='} the loop's fastest {min(t[False]):.4f} s")
    # launches per mini-batch from the driver's own counter: eager launches (a replayed graph's are not counted)
    ppo2, pol2 = make(min(args.envs, 256), min(args.steps, 32), args.batch, use_graphs=False)
    before = FusedLstmUpdate.launches
    epoch(ppo2, pol2, True)
    done = ppo2._fused_updater("p", args.batch).n_done
    result["k22_launches_per_minibatch"] = (FusedLstmUpdate.launches - before) / done
    say(f"K22 launches per mini-batch (driver counter, {done} mini-batches): {result['k22_launches_per_minibatch']:.2f}")
    say(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def trace_leg(args):
    import torch
    import eval_bench as B
    from ppo_and_friends_amd import kernels as K
    k22 = args.trace_leg == "k22"
    ppo, pol = make(args.envs, args.steps, args.batch, use_graphs=False)
    books = K.EvalScoreBooks(1, 1, B.DEV, 2, [1, 2])
    score, done = torch.zeros(2, 1, device=B.DEV), torch.zeros(1, dtype=torch.bool, device=B.DEV)
    mark = lambda: books.step(score, done)
    epoch(ppo, pol, k22)                                   # warm-up of this leg
    mark()
    epoch(ppo, pol, k22)
    mark()
    torch.cuda.synchronize()
    n_items = len(pol.dataset)
    print(f"leg={args.trace_leg} minibatches={(n_items + args.batch - 1) // args.batch}", flush=True)


def parse(paths, n_mb):
    rows = []
    for pattern in paths:
        for path in glob.glob(pattern, recursive=True):
            with open(path, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[2]]
    assert len(marks) == 2, f"{len(marks)} marker launches in the trace (2 expected)"
    body = rows[marks[0] + 1:marks[1]]
    print(f"{len(body)} launches over {n_mb} mini-batches = {len(body) / n_mb:.2f} per mini-batch "
          f"(the epoch's own launches -- table gather, moment records -- included); kernel time "
          f"{sum(e - s for s, e, _ in body) / n_mb / 1e3:.1f} us per mini-batch")
    count = {}
    for s, e, n in body:
        c = count.setdefault(n[:100], [0, 0])
        c[0] += 1
        c[1] += e - s
    print("  per mini-batch   avg us   kernel")
    for key, (c, ns) in sorted(count.items(), key=lambda kv: -kv[1][1])[:16]:
        print(f"    {c / n_mb:10.2f}  {ns / c / 1e3:8.2f}   {key}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--trace-leg", default=None, choices=["k22", "loop"], help="one warm-up epoch and one marked epoch of this leg")
    ap.add_argument("--parse", nargs="+", default=None, help="kernel trace CSV files (globs) of one leg")
    ap.add_argument("--minibatches", type=int, default=None, help="--parse: mini-batches of the traced epoch")
    args = ap.parse_args()
    if args.parse:
        parse(args.parse, args.minibatches)
    elif args.trace_leg:
        trace_leg(args)
    else:
        bench(args)


if __name__ == "__main__":
    main()
