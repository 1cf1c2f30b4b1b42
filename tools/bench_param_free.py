"""us per ``infer`` call of free-parent parametric plans (k_param_query's
``!M1`` forms, no wide input), for one source tree.

    python tools/bench_param_free.py <tree root>

A/B of two builds: run it for the other tree (a clean export of that commit,
built beside this one) and for this tree in turn, as alternated process pairs.
Plans: three cases of tests/param_matrix.py (linear, one hidden layer, two
hidden layers, each with one unobserved parent) at 131 072 queries; per plan 5
warm-up calls, then 5 windows of 20 calls between device events.  Prints one
JSON line: per plan the mean, min and max of the windows' us per call."""
import json
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import param_matrix as pm  # noqa: E402
from continuousbayesiannetwork_amd import BayesianNetwork  # noqa: E402
from helpers import make_bn, param_config  # noqa: E402
from test_gpu_param import load_fixture_params  # noqa: E402

dev = torch.device("cuda:0")
Q = 131072
out = {"tree": root}
for cid in ("lin_free-mode1-N20", "h1_free-mode2-N16-w7relu", "h32_free-8x8-mode2-N16"):
    case = pm.BY_ID[cid]
    data, cols, edges, target, _, params = pm.network(case)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=dev, estimator=case.est,
                 config=param_config(case.est, n_epochs=1, model=case.model))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        load_fixture_params(bn, {"meta": {"estimator": case.est}, "params": params}, tmp, dev)
    ev = {k: torch.tensor(v, device=dev) for k, v in pm.evidence(case, Q).items()}
    for _ in range(5):
        bn.infer(target, ev, N_max=case.N)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            bn.infer(target, ev, N_max=case.N)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / 20)
    out[cid] = dict(us_mean=round(float(np.mean(ts)), 1), us_min=round(min(ts), 1), us_max=round(max(ts), 1))
print(json.dumps(out), flush=True)
