"""predict vs infer + argmax + gather, alternated in one process.

Arm A is what a caller can do without ``predict``: ``infer``, ``torch.argmax``
over each row and ``torch.gather`` of the domain value (benchmarking_df's
lines, bayesian_network.py:329-373, without the ``.cpu()``).  Arm B is
``BayesianNetwork.predict``.  Default: BASELINE configs[1] (20-node chain,
d = 32, 65 536 queries); ``--config 2|3|4`` runs configs[2] (ALARM-like X35,
262 144 queries), configs[3] (50-node mixed DAG, LinearRegression, 131 072
queries) or configs[4] (10 x 10 grid, d = 64, peaked CPDs, 65 536 queries) at
their benchmarked sizes.

Before timing, at the timed size: B's index must equal ``argmax`` of A's rows
on every decided row (tests/predict_ref.decided on A's rows).  Then R
repetitions of (K calls of A, K calls of B), each window between device
events after a warm-up of both arms; the JSON line holds each arm's mean and
spread (min / max over the windows) of us per call, the algorithmic bytes per
query of each arm (4 B per evidence value read; written: 4 N B for A's row,
12 B for B's three outputs) and the plan flags.  ``--out FILE`` also writes
it there.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from continuousbayesiannetwork_amd import BayesianNetwork  # noqa: E402
from helpers import (alarm_like_data, chain_data, grid_data, make_bn, mixed_dag_data, param_config,  # noqa: E402
                     sample_evidence)
from predict_ref import decided  # noqa: E402


def workload(config, dev):
    """(bn, target, N, queries, data, cols, description)"""
    if config == 1:
        data, cols, edges = chain_data(20, 32, 200_000, 3, stay=0.8)
        return make_bn(BayesianNetwork, edges, cols, data, device=dev), "X19", 32, 65536, data, cols, "20-node chain d=32"
    if config == 2:
        data, cols, edges = alarm_like_data(200_000, 5)
        return make_bn(BayesianNetwork, edges, cols, data, device=dev), "X35", 8, 262144, data, cols, "ALARM-like 37 nodes d=8"
    if config == 3:
        data, cols, edges = mixed_dag_data(50_000, 7, unit=True)
        torch.manual_seed(0)
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev, estimator="linear_regression",
                     config=param_config("linear_regression", n_epochs=50))
        return bn, cols[-1], 16, 131072, data, cols, "mixed DAG 50 nodes, LinearRegression"
    data, cols, edges = grid_data(400_000, 3, side=10, d=64, keep=0.995, noise=0)
    return make_bn(BayesianNetwork, edges, cols, data, device=dev), cols[-1], 64, 65536, data, cols, "grid 10x10 d=64 (peaked)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=[1, 2, 3, 4], default=1)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=10, help="alternated (A, B) window pairs")
    ap.add_argument("--queries", type=int, default=None)
    ap.add_argument("--out", metavar="FILE", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bn, target, N, Q, data, cols, what = workload(a.config, dev)
    Q = a.queries or Q
    names = [c for c in cols if c != target]
    batches = [{k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, names, Q, s).items()}
               for s in range(4)]

    def arm_a(ev):
        probs, domain = bn.infer(target, ev, N_max=N)
        idx = torch.argmax(probs, dim=1, keepdim=True)
        return torch.gather(domain.expand(probs.shape[0], -1), dim=1, index=idx).squeeze(1), idx.squeeze(1), probs

    def arm_b(ev):
        return bn.predict(target, ev, N_max=N, return_index=True)

    # results first, at the timed size: B's index == argmax of A's rows on every decided row
    random.seed(0)
    checked = []
    for ev in batches:
        va, ia, probs = arm_a(ev)
        vb, ib = arm_b(ev)
        torch.cuda.synchronize()
        dec = torch.tensor(decided(probs.cpu().numpy()), device=dev)
        if not torch.equal(ia[dec], ib.long()[dec]) or not torch.equal(va[dec], vb[dec]):
            sys.exit("bench_predict: predict differs from argmax(infer) on decided rows")
        checked.append(round(float(dec.float().mean()), 4))
    for _ in range(3):  # warm-up of both arms on every batch
        for ev in batches:
            arm_a(ev)
            arm_b(ev)
    torch.cuda.synchronize()
    times = {"A": [], "B": []}
    for _ in range(a.reps):
        for name, fn in (("A", arm_a), ("B", arm_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.calls):
                fn(batches[i % 4])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    out = dict(workload=f"configs[{a.config}]: {what}, N_max={N}, evidence on {len(names)} nodes", queries=Q,
               calls_per_window=a.calls, windows=a.reps, decided_share=checked,
               plan_flags=bn.engine.predict_flags(target, batches[0].keys(), N),
               bytes_per_query=dict(A=4 * len(names) + 4 * N, B=4 * len(names) + 12))
    for k, v in times.items():
        out[k] = dict(us_per_call_mean=round(float(np.mean(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                      queries_per_s=round(Q / (float(np.mean(v)) * 1e-6), 1))
    out["B_over_A"] = round(out["B"]["us_per_call_mean"] / out["A"]["us_per_call_mean"], 3)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
