"""Golden vectors for [Q, N] evidence columns on PARAMETRIC networks, produced
by running the REFERENCE itself (run where the reference checkout is present):

    python tests/golden/make_golden_param_wide.py

A node whose evidence keys are not all of its parents reads each evidence
column through ``.expand(-1, N)`` (node.py:246-248): a column of width N_max is
N per-query values of that parent, paired by the meshgrid with the free
parents' sample points (node.py:258-261, :335-375); the factor is the mean
over all combos (bayesian_network.py:292).  Nothing there depends on the
estimator type.

Every case runs on the ``mixed_multi`` network of make_golden_param.py (A, B ->
C; A -> D; C, D -> E) with target E and C given as a [Q, N] column whose values
are drawn uniformly from the column's range widened by 30 % on each side.  A
and D have 3 levels, so N = 4 or 5 also redraws their sample domains
(``random`` is seeded per case before each reference call).  Each fixture
stores the data, the evidence, the reference's ``pdf`` / ``domain``, the
unnormalised rows (``raw``, make_golden_param.raw_rows) and every node's fitted
parameters in ``golden_io.load_param_golden``'s format.  No reference source
is copied.
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_param import _load_reference, _params, make_data, raw_rows, sample_evidence  # noqa: E402

WIDE = "C"
CASES = [
    dict(name="wide_lr_c", est="linear_regression", data=("multi", 400, 61), ev=["C"], Q=20, N=5, seed=2),
    # A is read strictly by D ([Q, 1] copy) and expanded by C
    dict(name="wide_lr_c_a", est="linear_regression", data=("multi", 400, 62), ev=["C", "A"], Q=16, N=4, seed=4),
    dict(name="wide_nn16_tanh_c_a", est="neural_network", data=("multi", 400, 63), ev=["C", "A"], Q=12, N=4, seed=6,
         unit=True, model={"hidden_dims": [16], "activation": "tanh"}),
    dict(name="wide_nn8x6_relu_c", est="neural_network", data=("multi", 400, 64), ev=["C"], Q=14, N=4, seed=8,
         unit=True, model={"hidden_dims": [8, 6], "activation": "relu"}),
    dict(name="wide_logreg_c_a", est="logistic_regression", data=("multi", 400, 65), ev=["C", "A"], Q=18, N=4, seed=10,
         unit=True),
    # case 1's network, fit and evidence with one NaN, one +inf and one -inf entry in three rows
    dict(name="wide_lr_c_special", est="linear_regression", data=("multi", 400, 61), ev=["C"], Q=20, N=5, seed=2,
         like=0, special=True),
]
# (row, position in the row) -> value
SPECIAL = {(3, 1): np.nan, (9, 4): np.inf, (15, 0): -np.inf}


def wide_column(data, cols, Q, N, seed):
    """[Q, N] values uniform in the column's range widened by 30 % on each side."""
    c = data[:, cols.index(WIDE)]
    lo, hi = float(c.min()), float(c.max())
    span = hi - lo
    rng = np.random.default_rng(seed)
    return rng.uniform(lo - 0.3 * span, hi + 0.3 * span, (Q, N)).astype(np.float32)


def main():
    import networkx as nx
    import pandas as pd
    import torch

    BayesianNetwork = _load_reference()
    manifest = []
    for i, c in enumerate(CASES):
        k = c.get("like", i)  # the special case repeats case 1's fit and draws
        torch.manual_seed(3000 + k)
        data, cols, edges = make_data(c["data"], c.get("unit", False))
        dag = nx.DiGraph()
        dag.add_nodes_from(cols)
        dag.add_edges_from(edges)
        df = pd.DataFrame(data, columns=cols)
        cfg = {"estimator_name": c["est"], "optimizer": {"name": "Adam", "params": {"lr": 0.05}},
               "train": {"n_epochs": 40}}
        if "model" in c:
            cfg["model"] = c["model"]
        bn = BayesianNetwork(dag, df, cfg, {"inference_obj": "exact"}, device="cpu")
        ev = sample_evidence(data, cols, c["ev"], c["Q"], seed=400 + k)
        ev[WIDE] = wide_column(data, cols, c["Q"], c["N"], seed=500 + k)
        if c.get("special"):
            for (r, a), v in SPECIAL.items():
                ev[WIDE][r, a] = v
        ev_t = {k2: torch.tensor(v) for k2, v in ev.items()}
        random.seed(c["seed"])
        p, d = bn.infer("E", ev_t, N_max=c["N"])
        random.seed(c["seed"])
        raw = raw_rows(bn, "E", ev_t, c["N"])
        pdf = p.numpy().astype(np.float32)
        assert np.array_equal((torch.tensor(raw) / torch.tensor(raw).max()).numpy(), pdf, equal_nan=True), c["name"]
        if not c.get("special"):
            assert np.isfinite(raw).all() and raw.min() > raw.max() * 1e-6, c["name"]
        out = dict(data=data, pdf=pdf, domain=d.numpy().astype(np.float32), raw=raw)
        meta_params = {}
        for n in cols:
            layers, ls = _params(bn.nodes_obj[n].estimator)
            for li, (W, b) in enumerate(layers):
                out[f"W_{n}_{li}"] = W
                out[f"b_{n}_{li}"] = b
            meta_params[n] = dict(n_layers=len(layers), log_scale=ls)
        for k2, v in ev.items():
            out["ev_" + k2] = v
        out["meta"] = np.array(json.dumps(dict(
            name=c["name"], estimator=c["est"], model=c.get("model", {}), columns=cols, edges=edges, target="E",
            evidence=list(ev.keys()), wide=[WIDE], N_max=c["N"], seed=c["seed"], unit=c.get("unit", False),
            special=[[r, a] for r, a in SPECIAL] if c.get("special") else [], params=meta_params)))
        np.savez_compressed(os.path.join(HERE, c["name"] + ".npz"), **out)
        manifest.append(c["name"])
        print(c["name"], pdf.shape, float(np.nanmin(raw) / np.nanmax(raw)), flush=True)
    with open(os.path.join(HERE, "MANIFEST_param_wide.json"), "w") as f:
        json.dump(dict(generator="tests/golden/make_golden_param_wide.py",
                       reference="Giovannibriglia/ContinuousBayesianNetwork",
                       cases=manifest), f, indent=1)


if __name__ == "__main__":
    main()
