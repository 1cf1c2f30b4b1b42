"""quantile vs the composition it replaces, alternated in one process.

Three arms, every window triple in the same job:

* ``quantile``     ``BayesianNetwork.quantile`` with 3 probabilities (the
                   median and a 95 % interval): one launch, Q x 3 values stored;
* ``composition``  what a caller does without it: ``engine.posterior(rows=True)``,
                   then ``torch.cumsum``, ``torch.searchsorted`` and a gather
                   over the stored [Q, N] tensor;
* ``expect``       ``BayesianNetwork.expect(moments=True)``: the floor for a
                   launch that stores no rows (the distance of ``quantile`` from
                   it is the cost of the scan and the searches).

Workloads: tools/bench_predict.py's (BASELINE configs[1] by default,
``--config 2|3|4``).  Before timing, at the timed size: ``quantile``'s values
must equal the composition's on at least 90 % of the entries of rows with mass
>= 1e-30 (the two scan in different float32 associations, and searchsorted on a
cdf with flat segments may return a column of probability 0, which ``quantile``
never does; the share is reported).  Then R repetitions of K calls of each arm
in turn, each window between device events after a warm-up of all arms; the
JSON line holds each arm's mean and spread (min / max over the windows) of us
per call, the plan flags and the algorithmic bytes per query (4 B per evidence
value read; written: 8 B per probability for ``quantile``'s index and value
plus 4 B of mass).  ``--out FILE`` also writes it there.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from helpers import sample_evidence  # noqa: E402
from bench_predict import workload  # noqa: E402

PROBS = (0.025, 0.5, 0.975)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=[1, 2, 3, 4], default=1)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=10, help="alternated windows per arm")
    ap.add_argument("--queries", type=int, default=None)
    ap.add_argument("--out", metavar="FILE", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bn, target, N, Q, data, cols, what = workload(a.config, dev)
    Q = a.queries or Q
    names = [c for c in cols if c != target]
    batches = [{k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, names, Q, s).items()}
               for s in range(4)]
    probs = torch.tensor(PROBS, device=dev)

    def quantile(ev):
        return bn.quantile(target, ev, probs=probs, N_max=N)

    def composition(ev):
        pdf, mass, _, _, dom = bn.engine.posterior_domain(target, ev, N)
        cdf = torch.cumsum(pdf, 1)
        idx = torch.searchsorted(cdf, probs.expand(cdf.shape[0], -1).contiguous()).clamp_max(N - 1)
        return dom.reshape(-1, N)[0][idx], mass

    def expect(ev):
        return bn.expect(target, ev, N_max=N, moments=True)

    arms = dict(quantile=quantile, composition=composition, expect=expect)

    # results first, at the timed size
    random.seed(0)
    agree = []
    for ev in batches:
        got = quantile(ev)
        ref, mass = composition(ev)
        torch.cuda.synchronize()
        big = mass >= 1e-30
        agree.append(float((got[big] == ref[big]).float().mean()))
        if agree[-1] < 0.9:
            sys.exit(f"bench_quantile: quantile equals the cumsum / searchsorted composition on only {agree[-1]:.4f} "
                     "of the entries")
    for _ in range(3):  # warm-up of every arm on every batch
        for ev in batches:
            for fn in arms.values():
                fn(ev)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.calls):
                fn(batches[i % 4])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    out = dict(workload=f"configs[{a.config}]: {what}, N_max={N}, evidence on {len(names)} nodes", queries=Q,
               probabilities=list(PROBS), calls_per_window=a.calls, windows=a.reps,
               share_of_entries_equal_to_composition=[round(x, 5) for x in agree],
               plan_flags=bn.engine.predict_flags(target, batches[0].keys(), N),
               bytes_per_query=dict(quantile=4 * len(names) + 8 * len(PROBS) + 4,
                                    composition=4 * len(names) + 3 * 2 * 4 * N))
    for k, v in times.items():
        out[k] = dict(us_per_call_mean=round(float(np.mean(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                      queries_per_s=round(Q / (float(np.mean(v)) * 1e-6), 1))
    out["quantile_over_composition"] = round(out["quantile"]["us_per_call_mean"] / out["composition"]["us_per_call_mean"], 3)
    out["quantile_minus_expect_us"] = round(out["quantile"]["us_per_call_mean"] - out["expect"]["us_per_call_mean"], 2)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
