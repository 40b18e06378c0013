"""
Launches per env step of an LSTM policy's rollout and evaluation, with the K21 step on or off, from a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lstm_step_trace.py --fused 1   # one leg per run
    python tools/lstm_step_trace.py --parse OUT/**/*_kernel_trace.csv --steps ROLLOUT_STEPS,EVAL_STEPS

The first form builds tools/eval_bench.py's `lstm` shape (cart_pole_lstm networks, E = 4096, T = 128), warms both verbs
up, then runs ONE rollout and ONE test_policy, each between two launches of a marker kernel that nothing else in a
one-agent run uses (the package's own eval_scores_books_kernel on one row), and prints the env steps of both.  The
second form counts the dispatches between the markers of such a trace and divides by the steps: launches per env step,
everything included (the env's own torch ops and the filter stack are the same in both legs), and the kernels that make
them up.
"""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARKER = "eval_scores_books_kernel"


def run(fused, envs, steps, runs_per_env):
    import torch
    import eval_bench as B
    from ppo_and_friends_amd import testing
    testing.rank_print = lambda *a, **k: None
    ppo = B.make("lstm", envs, steps)
    pol = ppo.policies["p"]
    pol.fused_lstm_step = bool(fused)
    assert (pol.lstm_step_unsupported_reason() == "") == bool(fused)
    from ppo_and_friends_amd import kernels as K
    books = K.EvalScoreBooks(1, 1, B.DEV, 2, [1, 2])
    score, done = torch.zeros(2, 1, device=B.DEV), torch.zeros(1, dtype=torch.bool, device=B.DEV)
    mark = lambda: books.step(score, done)
    N = envs * runs_per_env
    ppo.rollout()                                          # warm-up of this leg: allocations, first-use compilations
    testing.test_policy(ppo, N, deterministic=True, check_every=50)
    torch.cuda.synchronize()
    mark(); ppo.rollout(); mark()
    ppo.loop_steps[0] = 0
    mark(); testing.test_policy(ppo, N, deterministic=True, check_every=50); mark()
    torch.cuda.synchronize()
    print(f"fused={int(bool(fused))} rollout_steps={steps} eval_steps={ppo.loop_steps[0]}", flush=True)


def parse(paths, steps):
    rows = []
    for pattern in paths:
        for path in glob.glob(pattern, recursive=True):
            with open(path, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, (_, n) in enumerate(rows) if MARKER in n]
    assert len(marks) == 4, f"{len(marks)} marker launches in the trace (4 expected)"
    for what, (a, b), n_steps in zip(("rollout", "evaluation"), ((marks[0], marks[1]), (marks[2], marks[3])), steps):
        names = [n for _, n in rows[a + 1:b]]
        print(f"{what}: {len(names)} launches over {n_steps} env steps = {len(names) / n_steps:.2f} per env step")
        count = {}
        for n in names:
            key = n[:110]
            count[key] = count.get(key, 0) + 1
        for key, c in sorted(count.items(), key=lambda kv: -kv[1])[:14]:
            print(f"    {c / n_steps:7.2f}  {key}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rollout-steps", type=int, default=128)
    ap.add_argument("--runs-per-env", type=int, default=1)
    ap.add_argument("--parse", nargs="+", default=None, help="kernel trace CSV files (globs) of one leg")
    ap.add_argument("--steps", default=None, help="--parse: ROLLOUT_STEPS,EVAL_STEPS as the traced run printed them")
    args = ap.parse_args()
    if args.parse:
        parse(args.parse, [int(x) for x in args.steps.split(",")])
    else:
        run(args.fused, args.envs, args.rollout_steps, args.runs_per_env)


if __name__ == "__main__":
    main()
