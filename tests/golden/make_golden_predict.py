"""Golden predictions by running the REFERENCE itself (CPU), as make_golden.py.

    python tests/golden/make_golden_predict.py

A 6-node chain with d = 16 (tests/helpers.chain_data, stay = 0.8), 512
evidence rows over every node but the target, N_max = 16.  The three lines
``BayesianNetwork.benchmarking_df`` (cbn/base/bayesian_network.py:329-373)
applies to every ``infer`` result are done here -- ``argmax`` over each row of
the pdf, ``gather`` of the domain value at that index -- because
``benchmarking_df`` itself hard-codes ``.to("cuda")``.  Stored in
``predict_chain.npz``: the seeded data parameters (the data is regenerated from
them), the evidence, the arg-max indices and the gathered domain values.  No
reference source is copied.
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

PARAMS = dict(n=6, d=16, S=60000, seed=8, stay=0.8, target="X5", Q=512, ev_seed=41, N_max=16)


def main():
    import networkx as nx
    import pandas as pd
    import torch

    from helpers import chain_data, sample_evidence
    from make_golden import _load_reference

    BayesianNetwork = _load_reference()
    p = PARAMS
    data, cols, edges = chain_data(p["n"], p["d"], p["S"], p["seed"], stay=p["stay"])
    dag = nx.DiGraph()
    dag.add_nodes_from(cols)
    dag.add_edges_from(edges)
    bn = BayesianNetwork(dag, pd.DataFrame(data, columns=cols), {"estimator_name": "brute_force"},
                         {"inference_obj": "exact"}, device="cpu")
    names = [c for c in cols if c != p["target"]]
    ev = sample_evidence(data, cols, names, p["Q"], p["ev_seed"])
    random.seed(0)
    probs, domain = bn.infer(p["target"], {k: torch.tensor(v) for k, v in ev.items()}, N_max=p["N_max"])
    # benchmarking_df's own lines (bayesian_network.py:329-373)
    idx = torch.argmax(probs, dim=1, keepdim=True)
    pred = torch.gather(domain, dim=1, index=idx).squeeze(1)
    out = dict(index=idx.squeeze(1).numpy().astype(np.int32), value=pred.numpy().astype(np.float32),
               meta=np.array(json.dumps(dict(PARAMS, evidence=names))))
    for k, v in ev.items():
        out["ev_" + k] = v
    np.savez_compressed(os.path.join(HERE, "predict_chain.npz"), **out)
    print("predict_chain", probs.shape, np.bincount(out["index"], minlength=p["N_max"]))


if __name__ == "__main__":
    main()
