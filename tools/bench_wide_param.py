"""A [Q, N] evidence column on a parametric network vs what a caller could do
without it, alternated in one process.

Two arms, every window pair in the same job:

* ``wide``    ONE ``infer`` with the parent's N per-query values as a [Q, N]
              column (the parametric wide plan: k_param_query's ``!M1`` form
              averaging over N x N combos in one launch);
* ``slices``  what a caller could do before when a single factor reads the
              column: N ``infer_raw`` calls on the N [Q, 1] slices (each
              averages the free parent's N points), their mean and one division
              by the batch max in torch.  (The mean over the wide axis commutes
              with the product because no other factor reads that column.)

Plans: LinearRegression and NeuralNetwork (hidden [16], tanh) on
``helpers.mixed_dag_data`` columns (unit-scaled; 6 nodes: a 3-node observed
chain, two feeders of its last node and the target below both feeders), one
parent of the target wide and the other free, N_max = 16, 131 072 queries.
Before timing, at the timed size, the two arms must agree (rtol 1e-4 on the
entries above 1e-30 of the batch max).  Then R repetitions of K calls of each
arm in turn, each window between device events after a warm-up of both arms;
one JSON line per estimator with each arm's mean and spread (min / max over
the windows) of us per call and the wide plan's ``cbn_plan_param_info``.
``--out FILE`` also writes the lines there.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from continuousbayesiannetwork_amd import BayesianNetwork, _native  # noqa: E402
from helpers import make_bn, mixed_dag_data, param_config, sample_evidence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--est", choices=["lr", "nn", "both"], default="both")
    ap.add_argument("--queries", type=int, default=131072)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=8, help="alternated windows per arm")
    ap.add_argument("--out", metavar="FILE", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, Q = 16, a.queries
    data, cols, _ = mixed_dag_data(20_000, 7, n=6, unit=True)
    chain, (wide, free), target = cols[:3], cols[3:5], cols[5]
    edges = [(chain[0], chain[1]), (chain[1], chain[2]), (chain[2], wide), (chain[2], free), (wide, target),
             (free, target)]
    ests = [("linear_regression", None), ("neural_network", {"hidden_dims": [16], "activation": "tanh"})]
    ests = ests[:1] if a.est == "lr" else ests[1:] if a.est == "nn" else ests
    lines = []
    for est, model in ests:
        torch.manual_seed(0)
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev, estimator=est,
                     config=param_config(est, n_epochs=30, model=model))
        batches = []
        for s in range(2):
            ev = {k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, chain, Q, s).items()}
            w = torch.tensor(np.random.default_rng(100 + s).uniform(-0.3, 1.3, (Q, N)).astype(np.float32), device=dev)
            sl = [dict(ev, **{wide: w[:, i:i + 1].contiguous()}) for i in range(N)]  # (sliced outside the windows)
            batches.append((dict(ev, **{wide: w}), sl))

        def run_wide(b):
            return bn.infer(target, b[0], N_max=N)[0]

        def run_slices(b):
            acc = None
            for e in b[1]:
                rows = bn.engine.infer_raw(target, e, N)[0]
                acc = rows.clone() if acc is None else acc.add_(rows)
            acc /= N
            return acc.div_(acc.max())

        arms = dict(wide=run_wide, slices=run_slices)
        worst = 0.0
        for b in batches:  # results first, at the timed size
            x, y = run_wide(b), run_slices(b)
            torch.cuda.synchronize()
            big = y >= 1e-30
            rel = ((x - y).abs()[big] / y[big]).max()
            worst = max(worst, float(rel))
            if not torch.isfinite(x).all() or not rel <= 1e-4:
                sys.exit(f"bench_wide_param: the arms differ ({est}: max relative difference {float(rel):.3e})")
        for _ in range(2):
            for b in batches:
                for fn in arms.values():
                    fn(b)
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.reps):
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.calls):
                    fn(batches[i % 2])
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        info = _native.param_info(bn.engine.serving_plan(target, batches[0][0], N).handle)
        out = dict(workload=f"{est} {model or ''}: chain of 3 observed nodes, target with one wide and one free parent, "
                            f"N_max={N}", queries=Q, calls_per_window=a.calls, windows=a.reps,
                   max_relative_difference_of_the_arms=worst,
                   wide_plan={k: info[k] for k in ("generic", "nc", "n_chunks", "hmax", "mode", "tab", "m1", "parts")})
        for k, v in times.items():
            out[k] = dict(us_per_call_mean=round(float(np.mean(v)), 1), us_min=round(min(v), 1), us_max=round(max(v), 1))
        out["wide_over_slices"] = round(out["wide"]["us_per_call_mean"] / out["slices"]["us_per_call_mean"], 3)
        lines.append(out)
        print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
