"""posterior / expect vs infer + torch reductions, alternated in one process.

Five arms, every window pair in the same job:

* ``infer``          ``BayesianNetwork.infer`` alone (the yardstick);
* ``infer_norm``     what a caller does without ``posterior``: ``infer`` then
                     ``pdf / pdf.sum(1, keepdim=True)``;
* ``posterior``      ``BayesianNetwork.posterior``;
* ``infer_moments``  what a caller does without ``expect``: ``infer`` then the
                     torch reductions (row sum, weighted mean, centred variance)
                     over the stored [Q, N] tensor;
* ``expect``         ``BayesianNetwork.expect(moments=True)``.

Workloads: tools/bench_predict.py's (BASELINE configs[1] by default,
``--config 2|3|4``).  Before timing, at the timed size: ``posterior`` must agree
with ``infer_norm`` and ``expect``'s mean with ``infer_moments``' on every row of mass
>= 1e-30 (rtol 1e-4, on the entries that are not subnormal quotients in either
arm: on configs[1] ``infer``'s raw / batch max underflows for 0.07 % of them);
the variance's largest distance from a float64 evaluation of ``infer``'s rows is
reported beside the float32 torch arm's.
Then R repetitions of K calls of each arm in turn, each window between device
events after a warm-up of all arms; the JSON line holds each arm's mean and
spread (min / max over the windows) of us per call, the plan flags and the
algorithmic bytes per query (4 B per evidence value read; written: 4 N B for
``posterior``'s row, 12 B for ``expect``'s three outputs).  ``--out FILE`` also
writes it there.
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

    def infer(ev):
        return bn.infer(target, ev, N_max=N)

    def infer_norm(ev):
        pdf, _ = bn.infer(target, ev, N_max=N)
        return pdf / pdf.sum(1, keepdim=True)

    def posterior(ev):
        return bn.posterior(target, ev, N_max=N)[0]

    def infer_moments(ev):
        pdf, dom = bn.infer(target, ev, N_max=N)
        mass = pdf.sum(1)
        mean = (pdf * dom).sum(1) / mass
        var = (pdf * (dom - mean[:, None]) ** 2).sum(1) / mass
        return mean, var, mass

    def expect(ev):
        return bn.expect(target, ev, N_max=N, moments=True)

    arms = dict(infer=infer, infer_norm=infer_norm, posterior=posterior, infer_moments=infer_moments, expect=expect)

    # results first, at the timed size
    random.seed(0)
    checked, var_check = [], []
    for ev in batches:
        ref, got = infer_norm(ev), posterior(ev)
        rmean, rvar, _ = infer_moments(ev)
        mean, var, mass = expect(ev)
        torch.cuda.synchronize()
        big = mass >= 1e-30
        # entries that are subnormal in either arm (infer's raw / batch max underflows where posterior's
        # raw / row sum does not) carry no relative accuracy: compared where both quotients are >= 1e-34
        pdf, _ = infer(ev)
        norm = (pdf >= 1e-34) & (got >= 1e-34)
        got, ref = torch.where(norm, got, 0), torch.where(norm, ref, 0)
        ok = dict(pdf=torch.allclose(got[big], ref[big], rtol=1e-4, atol=0),
                  mean=torch.allclose(mean[big], rmean[big], rtol=1e-4, atol=1e-4 * float(rmean[big].abs().max())))
        if not all(ok.values()):
            sys.exit(f"bench_posterior: posterior / expect differ from the torch reductions of infer's rows: {ok}")
        # the variance against a float64 evaluation of infer's rows, reported (the float32 torch arm is the other figure)
        p64, d64 = pdf.double(), bn.infer(target, ev, N_max=N)[1].double()
        m64 = (p64 * d64).sum(1) / p64.sum(1)
        v64 = (p64 * (d64 - m64[:, None]) ** 2).sum(1) / p64.sum(1)
        var_check.append(dict(max_abs_err_vs_f64=float((var.double() - v64).abs()[big].max()),
                              max_abs_err_torch_f32_vs_f64=float((rvar.double() - v64).abs()[big].max()),
                              largest_var=float(v64[big].abs().max())))
        checked.append(round(float(big.float().mean()), 4))
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
               calls_per_window=a.calls, windows=a.reps, share_of_rows_compared=checked, var_check=var_check[0],
               plan_flags=bn.engine.predict_flags(target, batches[0].keys(), N),
               bytes_per_query=dict(posterior=4 * len(names) + 4 * N, expect=4 * len(names) + 12))
    for k, v in times.items():
        out[k] = dict(us_per_call_mean=round(float(np.mean(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                      queries_per_s=round(Q / (float(np.mean(v)) * 1e-6), 1))
    out["posterior_over_infer"] = round(out["posterior"]["us_per_call_mean"] / out["infer"]["us_per_call_mean"], 3)
    out["posterior_over_infer_norm"] = round(out["posterior"]["us_per_call_mean"] / out["infer_norm"]["us_per_call_mean"], 3)
    out["expect_over_infer_moments"] = round(out["expect"]["us_per_call_mean"] / out["infer_moments"]["us_per_call_mean"], 3)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
