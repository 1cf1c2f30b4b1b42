"""Parametric estimators (LinearRegression / LogisticRegression /
NeuralNetwork) on the HIP path vs the reference (golden vectors, same fitted
parameters loaded through ``load_model``) and vs the CPU oracle.

Tolerance (tests/parity.py): rtol 1e-5 (north star, fp32) on every entry of
the max-normalised pdfs plus the subnormal-rounding floor n_factors * 2^-149 *
peak / (the oracle's unnormalised batch max), never above the former atol
1e-7; single densities (get_prob): rtol 1e-5 plus one subnormal step.  The
kernels evaluate exp / tanh / erf with the device math library and sum the
free-parent means in their own order, so results differ from torch's CPU
kernels in the last ulps; NaN patterns (the reference's overflowing logistic
density) must match exactly, and there the unnormalised rows are compared too.
"""
import os
import random

import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, Node
from continuousbayesiannetwork_amd.parameter_learning import LinearRegression, NeuralNetwork
from golden_io import load_param_golden, oracle_estimators, param_golden_names
from helpers import make_bn, mixed_dag_data, param_config, sample_evidence
from oracle.ref_infer import OracleBN, OracleNode, OracleParametric
from parity import (assert_factor_close, assert_golden_close, assert_marginals_close, engine_raw_rows, n_factors,
                    oracle_raw, oracle_reference, peak as oracle_peak)

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def _t(ev, dev):
    return {k: torch.tensor(v, device=dev) for k, v in ev.items()}


def _state(est_name, layers, log_scale, dev):
    """The reference's save_model dict for these parameters (linear_regression.py:117-124,
    logistIc_regression.py:125-132, neural_network.py:149-156)."""
    ls = torch.tensor(log_scale, dtype=torch.float32, device=dev)
    if est_name == "neural_network":
        sd = {}
        for i, (W, b) in enumerate(layers):
            sd[f"{2 * i}.weight"] = torch.tensor(W, device=dev)
            sd[f"{2 * i}.bias"] = torch.tensor(b, device=dev)
        return {"nn_state_dict": sd, "log_scale": ls}
    sd = {"weight": torch.tensor(layers[0][0], device=dev), "bias": torch.tensor(layers[0][1], device=dev)}
    key = "log_sigma" if est_name == "linear_regression" else "log_scale"
    return {"linear_state_dict": sd, key: ls}


def load_fixture_params(bn, g, tmp_path, dev):
    """Every node's estimator gets the reference's fitted parameters via Node.load_node."""
    m = g["meta"]
    for n, (layers, ls) in g["params"].items():
        path = os.path.join(str(tmp_path), f"{n}.pt")
        torch.save(_state(m["estimator"], layers, ls, dev), path)
        bn.nodes_obj[n].load_node(path)


def _fixture_bn(g, gpu, tmp_path):
    m = g["meta"]
    cfg = param_config(m["estimator"], n_epochs=1, model=m["model"] or None)
    bn = make_bn(BayesianNetwork, m["edges"], m["columns"], g["data"], device=gpu, estimator=m["estimator"],
                 config=cfg)
    load_fixture_params(bn, g, tmp_path, gpu)
    return bn


@pytest.mark.parametrize("name", param_golden_names())
def test_parametric_infer_matches_reference_golden(name, gpu, tmp_path):
    g = load_param_golden(name)
    m = g["meta"]
    bn = _fixture_bn(g, gpu, tmp_path)
    ev = _t({k: g["evidence"][k] for k in m["evidence"]}, gpu)
    random.seed(m["seed"])
    pdf, dom = bn.infer(m["target"], ev, N_max=m["N_max"])
    assert pdf.device.type == "cuda"
    np.testing.assert_array_equal(dom.cpu().numpy(), g["domain"])
    assert_golden_close(pdf.cpu().numpy(), name, param=True, got_raw=engine_raw_rows(bn, name, ev, param=True))
    # cached plan (or a redraw of the padded domains) gives the same rows
    random.seed(m["seed"])
    pdf2, _ = bn.infer(m["target"], ev, N_max=m["N_max"])
    np.testing.assert_array_equal(pdf2.cpu().numpy(), pdf.cpu().numpy())


def _oracle_from_bn(bn, edges, cols, data, est_name, act=None):
    """OracleBN carrying the parameters the framework fitted (training is not
    the accelerated path; inference parity is checked on the same model)."""
    fam = "gauss" if est_name == "linear_regression" else "logistic"
    ests = {}
    for n in cols:
        e = bn.nodes_obj[n].estimator
        lins = e._linears()
        layers = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in lins]
        ests[n] = OracleParametric(fam, layers, float(e._log_scale().detach().cpu()), act=act,
                                   root_bias_only=est_name == "linear_regression")
    return OracleBN(edges, cols, data, estimators=ests)


@pytest.mark.parametrize("est,model,evn,N", [
    ("linear_regression", None, "all", 16),
    ("linear_regression", None, "sparse", 8),
    ("neural_network", {"hidden_dims": [16], "activation": "tanh"}, "all", 16),
    ("neural_network", {"hidden_dims": [32], "activation": "tanh"}, "all", 12),
    ("logistic_regression", None, "sparse", 6),
    # beyond the register-resident kernels (generic kernel, activations in LDS)
    ("neural_network", {"hidden_dims": [64, 64], "activation": "tanh"}, "all", 16),
    ("neural_network", {"hidden_dims": [8, 8, 8, 8, 8, 8], "activation": "relu"}, "sparse", 8),
    # one hidden layer wider than 32 units: the streamed fast kernel
    ("neural_network", {"hidden_dims": [48], "activation": "sigmoid"}, "all", 12),
])
def test_mixed_dag_matches_oracle(est, model, evn, N, gpu):
    """configs[3]-shaped network (mixed continuous / 20-level discrete columns,
    in-degree <= 3), 12 nodes here so the oracle stays fast."""
    unit = est != "linear_regression"
    data, cols, edges = mixed_dag_data(3000, 4, n=12, unit=unit)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator=est,
                 config=param_config(est, n_epochs=25, model=model))
    act = (model or {}).get("activation")
    ora = _oracle_from_bn(bn, edges, cols, data, est, act)
    target = cols[-1]
    names = [c for c in cols if c != target] if evn == "all" else [cols[-2], cols[5], cols[2]]
    ev = sample_evidence(data, cols, names, 700, 3)
    random.seed(4)
    ref, rdom, kw = oracle_reference(ora, target, ev, N)
    random.seed(4)
    pdf, dom = bn.infer(target, _t(ev, gpu), N_max=N)
    np.testing.assert_array_equal(dom.cpu().numpy(), rdom)
    assert_marginals_close(pdf.cpu().numpy(), ref, **kw)


def test_estimator_get_prob_matches_oracle(gpu):
    """_get_prob of all three estimators (query rows, query=None roots) vs the oracle."""
    rng = np.random.default_rng(1)
    for est, model, act in [("linear_regression", None, None), ("logistic_regression", None, None),
                            ("neural_network", {"hidden_dims": [8, 5], "activation": "gelu"}, "gelu")]:
        from continuousbayesiannetwork_amd.parameter_learning import ESTIMATORS

        e = ESTIMATORS[est](param_config(est, n_epochs=5, model=model), device=gpu)
        x = rng.uniform(0, 1, (3, 400)).astype(np.float32)
        y = (0.3 * x[0] + 0.5 * x[1] - 0.2 * x[2]).astype(np.float32)
        e.fit(torch.tensor(y, device=gpu), torch.tensor(x, device=gpu))
        lins = e._linears()
        layers = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in lins]
        fam = "gauss" if est == "linear_regression" else "logistic"
        o = OracleParametric(fam, layers, float(e._log_scale().detach().cpu()), act=act,
                             root_bias_only=est == "linear_regression")
        pts = rng.uniform(-1, 2, (64, 9)).astype(np.float32)
        q = rng.uniform(0, 1, (64, 3, 1)).astype(np.float32)
        got = e.get_prob(torch.tensor(pts, device=gpu), torch.tensor(q, device=gpu)).cpu().numpy()
        assert_factor_close(got, o.get_prob(pts, q))
    # root (query=None): LinearRegression uses its bias, the logistic models a ones input
    lr = LinearRegression(param_config("linear_regression", n_epochs=5), device=gpu)
    lr.fit(torch.tensor(y, device=gpu))
    o = OracleParametric("gauss", [(lr.linear_model.weight.detach().cpu().numpy(),
                                    lr.linear_model.bias.detach().cpu().numpy())], 0.0, root_bias_only=True)
    assert_factor_close(lr.get_prob(torch.tensor(pts, device=gpu)).cpu().numpy(), o.get_prob(pts))
    nn_ = NeuralNetwork(param_config("neural_network", n_epochs=5, model={"hidden_dims": [16]}), device=gpu)
    nn_.fit(torch.tensor(y, device=gpu))
    o = OracleParametric("logistic", [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy())
                                      for l in nn_._linears()], 0.0, act="tanh")
    assert_factor_close(nn_.get_prob(torch.tensor(pts, device=gpu)).cpu().numpy(), o.get_prob(pts))


def test_node_get_prob_parametric_matches_oracle(gpu):
    """Node.get_prob with a parametric estimator: free-parent grid, partial and full evidence."""
    g = load_param_golden("lr_multi_partial")
    m = g["meta"]
    data, cols = g["data"], m["columns"]
    parents = ["C", "D"]
    layers, ls = g["params"]["E"]
    on = OracleNode("E", parents, OracleParametric("gauss", layers, ls, root_bias_only=True))
    on.fit(data[:, cols.index("E")], np.stack([data[:, cols.index(p)] for p in parents]))
    nd = Node("E", "linear_regression", param_config("linear_regression", n_epochs=1), parents, device=gpu)
    nd.fit(torch.tensor(data[:, cols.index("E")], device=gpu),
           torch.tensor(np.stack([data[:, cols.index(p)] for p in parents]), device=gpu))
    est = nd.estimator
    est.linear_model.weight.data = torch.tensor(layers[0][0], device=gpu)
    est.linear_model.bias.data = torch.tensor(layers[0][1], device=gpu)
    est.log_sigma.data = torch.tensor(ls, device=gpu)
    est._invalidate()
    ev = sample_evidence(data, cols, ["C", "D"], 11, 3)
    for q in [{}, {"C": ev["C"]}, {"C": ev["C"], "D": ev["D"]}]:
        for N in (2, 3, 5):
            random.seed(1)
            ref, rdom = on.get_prob(dict(q), N)
            random.seed(1)
            pdf, dom, _ = nd.get_prob({k: torch.tensor(v, device=gpu) for k, v in q.items()}, N)
            assert tuple(pdf.shape) == ref.shape
            assert_factor_close(pdf.cpu().numpy(), ref)  # single densities


@pytest.mark.parametrize("Q,shards", [(1001, 2), (131072, 8), (5, 3)])
def test_parametric_raw_sharded_equals_single_call(Q, shards, gpu):
    """Sharded step on a parametric plan (raw launch per shard, MAX of the words,
    in-place scale) == the single-process infer, bit for bit."""
    from continuousbayesiannetwork_amd.distributed import shard_evidence, sharded_infer

    data, cols, edges = mixed_dag_data(4000, 6, n=16)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=10))
    names = cols[:-1]
    ev = _t(sample_evidence(data, cols, names, Q, 11), gpu)
    full, _ = bn.infer(cols[-1], ev, N_max=16)
    full = full.clone()
    rows, bits, scales = [], [], []
    for r in range(shards):
        res = bn.engine.infer_raw(cols[-1], shard_evidence(ev, shards, r), 16)
        assert res is not None
        o, _, b, sc = res
        rows.append(o)
        bits.append(b.clone())
        scales.append(sc)
    m = torch.stack(bits).max(0).values
    for o, sc in zip(rows, scales):
        sc(o, m)
    np.testing.assert_array_equal(torch.cat(rows).cpu().numpy(), full.cpu().numpy())
    one, _ = sharded_infer(bn, cols[-1], ev, N_max=16)
    np.testing.assert_array_equal(one.cpu().numpy(), full.cpu().numpy())


@pytest.mark.parametrize("name", ["lr_mixed50_config3_full", "nn_mixed50_config3_full"])
def test_config3_full_share_matches_reference(name, gpu, tmp_path):
    """BASELINE configs[3] at one GPU's share of the 1 M-query batch (131 072
    queries, 50-node mixed DAG, LinearRegression / NeuralNetwork [16] tanh, the
    reference fixtures' fitted parameters): a 4 097-row slice (every 32nd row +
    the batch argmax row) of the reference's output over the WHOLE batch,
    normalised by its max (tests/golden/make_golden_full_param.py), at rtol 1e-5."""
    import hashlib
    import json

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    meta = json.loads(str(z["meta"]))
    g = load_param_golden(meta["base"])
    m = g["meta"]
    bn = _fixture_bn(g, gpu, tmp_path)
    names = [c for c in m["columns"] if c != m["target"]]
    ev = sample_evidence(g["data"], m["columns"], names, meta["Q"], meta["ev_seed"])
    h = hashlib.sha256()
    for k in sorted(ev):
        h.update(np.ascontiguousarray(ev[k]).tobytes())
    assert h.hexdigest() == meta["evidence_sha256"]
    random.seed(0)
    pdf, dom = bn.infer(m["target"], _t(ev, gpu), N_max=m["N_max"])
    p = pdf.cpu().numpy()
    np.testing.assert_array_equal(dom.cpu().numpy(), z["domain"])
    assert float(p[meta["argmax_row"]].max()) == 1.0 and float(np.nanmax(p)) == 1.0
    # the batch max M of the unnormalised products: the oracle (the fixture's
    # parameters) on the reference's argmax row alone
    ora = OracleBN(m["edges"], m["columns"], g["data"], estimators=oracle_estimators(g))
    r = meta["argmax_row"]
    _, mx = oracle_raw(ora, m["target"], {k: v[r:r + 1] for k, v in ev.items()}, m["N_max"])
    assert_marginals_close(p[z["rows"]], z["pdf"], raw_max=mx, n_factors=n_factors(ora, m["target"]),
                           peak=oracle_peak(ora, m["target"]))


@pytest.mark.parametrize("est,model", [("linear_regression", None),
                                       ("neural_network", {"hidden_dims": [16], "activation": "tanh"})])
def test_config3_full_size_properties(est, model, gpu):
    """configs[3] shape at one GPU's share of the batch (50 nodes, 131 072
    queries, evidence on the 49 non-target nodes, GPU-trained parameters): max
    exactly 1, duplicated evidence rows identical, a sample of rows plus the
    batch argmax row matches the oracle on the same parameters at rtol 1e-5."""
    # unit-scaled columns: with raw 0..19 levels and the reference's fixed
    # sigma = 1 (log_sigma is not in its optimizer, linear_regression.py:53),
    # the 50-factor product underflows to 0 in every column and 0 / 0 = NaN
    data, cols, edges = mixed_dag_data(20000, 7, unit=True)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator=est,
                 config=param_config(est, n_epochs=20, model=model))
    names = cols[:-1]
    Q = 131072
    ev = sample_evidence(data, cols, names, Q, 8)
    for k in ev:
        ev[k][1] = ev[k][0]
    pdf, _ = bn.infer(cols[-1], _t(ev, gpu), N_max=16)
    p = pdf.cpu().numpy()
    assert p.shape == (Q, 16) and p.max() == 1.0
    assert (p > 0).mean() > 0.99
    np.testing.assert_array_equal(p[0], p[1])
    ora = _oracle_from_bn(bn, edges, cols, data, est, (model or {}).get("activation"))
    rstar = int(np.argmax(p.max(1)))
    sub = np.append(np.arange(0, Q, Q // 61)[:60], rstar)  # + the argmax row: one normaliser for both
    ref, _, kw = oracle_reference(ora, cols[-1], {k: v[sub] for k, v in ev.items()}, 16)
    assert ref[-1].max() == 1.0
    assert_marginals_close(p[sub], ref, **kw)


def _set_linear(est, W, b, log_scale, gpu):
    est.linear_model.weight.data = torch.tensor(W, dtype=torch.float32, device=gpu)
    est.linear_model.bias.data = torch.tensor(b, dtype=torch.float32, device=gpu)
    getattr(est, "log_sigma", None) is not None and setattr(est.log_sigma, "data",
                                                            torch.tensor(log_scale, device=gpu))
    getattr(est, "log_scale", None) is not None and setattr(est.log_scale, "data",
                                                            torch.tensor(log_scale, device=gpu))
    est._invalidate()


def test_density_accuracy_full_range(gpu):
    """The kernels' exp (split x*log2e + v_exp_f32) and Newton-refined divisions
    vs float64 over the whole fp32 range of the two densities: <= 4 ulp where
    the float64 value is a normal fp32; subnormal results (< 2^-126, kept as
    the reference keeps them) within 2 subnormal steps (2^-148) plus 4 ulp of
    the float64 value; overflow gives the reference's NaN (logistic: inf / inf)."""
    from continuousbayesiannetwork_amd.parameter_learning import LogisticRegression

    tiny = np.float32(2.0 ** -126)
    x = np.linspace(-14.6, 14.6, 200001, dtype=np.float32)
    q = np.zeros((x.size, 1, 1), np.float32)
    lr = LinearRegression(param_config("linear_regression", n_epochs=1), device=gpu)
    lr.fit(torch.tensor(x[:100], device=gpu), torch.tensor(x[None, :100], device=gpu))
    for ls in (0.0, -0.7, 1.3):  # sigma = 1 (unit path) and scaled
        _set_linear(lr, [[0.0]], [0.0], ls, gpu)
        got = lr.get_prob(torch.tensor(x[:, None], device=gpu), torch.tensor(q, device=gpu)).cpu().numpy()[:, 0]
        # sigma / norm exactly as the estimator computes them (torch CPU float32,
        # linear_regression.py:91-95): d pdf / pdf = t^2 per unit relative change of t
        sig_t = torch.exp(torch.tensor(ls, dtype=torch.float32))
        sig = np.float32(sig_t.item())
        norm = np.float32((1 / (sig_t * torch.sqrt(torch.tensor(2 * torch.pi)))).item())
        t = (x / sig).astype(np.float32)
        ideal = (np.float64(norm) * np.exp(np.float64(np.float32(-0.5) * (t * t)))).astype(np.float32)
        normal = ideal >= tiny
        ulp = np.abs(got[normal].astype(np.float64) - ideal[normal]) / np.spacing(ideal[normal])
        assert ulp.max() <= 4, (ls, ulp.max())
        sub = ~normal & (ideal > 0)
        assert ls != 0.0 or sub.sum() > 1000
        assert (np.abs(got[sub].astype(np.float64) - ideal[sub]) <= 2.0 ** -148 + 4 * 2.0 ** -23 * ideal[sub]).all()
    lg = LogisticRegression(param_config("logistic_regression", n_epochs=1), device=gpu)
    lg.fit(torch.tensor(np.zeros(100, np.float32), device=gpu), torch.tensor(x[None, :100], device=gpu))
    d = np.linspace(-95.0, 95.0, 200001, dtype=np.float32)
    for ls in (0.0, 0.4):
        _set_linear(lg, [[0.0]], [0.0], ls, gpu)
        got = lg.get_prob(torch.tensor(d[:, None], device=gpu), torch.tensor(q, device=gpu)).cpu().numpy()[:, 0]
        s = np.float32(torch.exp(torch.tensor(ls, dtype=torch.float32)).item())
        dd = (d / s).astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            e32 = np.exp(-dd)  # the reference's float32 path decides inf / NaN
            u = (np.float32(1) + e32).astype(np.float32)
            ref32 = (e32 / (s * u * u)).astype(np.float32)
            e = np.exp(-np.float64(dd))
            ideal = (e / (np.float64(s) * (1 + e) ** 2)).astype(np.float32)
        nan = np.isnan(ref32)
        np.testing.assert_array_equal(np.isnan(got), nan)
        zero = ~nan & (ref32 == 0)
        assert np.all(got[zero] == 0)
        normal = ~nan & ~zero & (ideal >= tiny)  # zero: the reference's (1 + e)^2 overflowed
        ulp = np.abs(got[normal].astype(np.float64) - ideal[normal]) / np.spacing(ideal[normal])
        assert ulp.max() <= 4, (ls, ulp.max())
        sub = ~nan & ~zero & (ideal < tiny) & (ideal > 0)
        assert (np.abs(got[sub].astype(np.float64) - ideal[sub]) <= 2.0 ** -148 + 4 * 2.0 ** -23 * ideal[sub]).all()


@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
def test_activation_accuracy(act, gpu):
    """The kernels' tanh (two-branch: odd polynomial below 0.625, else
    1 - 2 / (1 + e^2|x|)) and sigmoid (split exp + Newton-refined reciprocal)
    vs float64,
    through cbn_param_eval of mu = act(x) (one hidden unit, W = 1, b = 0) and a
    Gaussian at the point 0: pdf = exp(-0.5 (mu / s)^2), so mu = s sqrt(-2 ln
    pdf) recovers mu to ~1 ulp when s puts (mu / s)^2 in [36, 150] (one call
    per binade of mu).  Bound: 8 ulp of the float64 activation."""
    import ctypes

    from continuousbayesiannetwork_amd import _native

    lib = _native.load()
    x = np.concatenate([np.linspace(-9, 9, 400001), np.logspace(-7, 0.5, 20001), -np.logspace(-7, 0.5, 20001)])
    x = x.astype(np.float32)
    x64 = x.astype(np.float64)
    ref = np.tanh(x64) if act == "tanh" else 1 / (1 + np.exp(-x64))
    keep = ref != 0
    x, ref = x[keep], ref[keep]
    code = _native.CBN_ACT[act]
    w = torch.tensor([1.0, 0.0, 1.0, 0.0], device=gpu)
    worst = 0.0
    binade = np.floor(np.log2(np.abs(ref)))
    for b in np.unique(binade):
        sel = binade == b
        s = np.float32(2.0 ** b / 6)  # (mu / s)^2 in [36, 144)
        m = _native.ParamModel()
        m.family, m.n_layers, m.act = _native.CBN_FAMILY_GAUSS, 2, code
        m.width[0], m.width[1], m.width[2] = 1, 1, 1
        m.weights, m.scale, m.norm = w.data_ptr(), float(s), 1.0
        q = torch.tensor(x[sel][:, None], device=gpu)
        pts = torch.zeros((q.shape[0], 1), device=gpu)
        out = torch.empty_like(pts)
        _native.check(lib.cbn_param_eval(ctypes.byref(m), _native.ptr(pts), q.shape[0], 1, _native.ptr(q), 0,
                                         _native.ptr(out), _native.stream_ptr(gpu)), "cbn_param_eval")
        pdf = out.cpu().numpy()[:, 0].astype(np.float64)
        mu = np.float64(s) * np.sqrt(-2 * np.log(pdf))
        r = ref[sel]
        ulp = np.abs(mu - np.abs(r)) / np.spacing(np.abs(r).astype(np.float32))
        worst = max(worst, float(ulp.max()))
    assert worst <= 8, worst


def test_parametric_sharded_stepper_equals_infer(gpu):
    """The pipelined stepper on a parametric plan (raw launch of the
    parametric query kernel, grouped exchange, batched scale) == infer on each
    batch bit for bit; float64 evidence (rejected by the native checks) falls
    back to the serial sharded path with the same result."""
    from continuousbayesiannetwork_amd.distributed import ShardedStepper

    data, cols, edges = mixed_dag_data(4000, 6, n=16)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=10))
    names = cols[:-1]
    batches = [_t(sample_evidence(data, cols, names, 3000 + 517 * i, 40 + i), gpu) for i in range(5)]
    ref = [bn.infer(cols[-1], b, N_max=16)[0].clone() for b in batches]
    st = ShardedStepper(bn, cols[-1], 16, exchange_every=3, force_exchange=True)
    got = [st.step(b)[0] for b in batches]
    st.wait()
    torch.cuda.synchronize()
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g.cpu().numpy(), r.cpu().numpy())
    b64 = {k: v.double() for k, v in batches[1].items()}
    g64, _ = st.step(b64)
    st.wait()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g64.cpu().numpy(), ref[1].cpu().numpy())
    st.close()


@pytest.mark.parametrize("observed", [10, 8])
def test_ten_parent_parametric_node(observed, gpu):
    """A LinearRegression node with 10 parents (beyond the fixed input array):
    every parent observed, and 2 free parents (N^2 combos)."""
    rng = np.random.default_rng(5)
    S = 4000
    R = np.round(rng.normal(0, 1, (S, 10)), 2)
    Y = np.round(R @ rng.uniform(-0.5, 0.5, 10) + rng.normal(0, 0.5, S), 2)
    data = np.concatenate([R, Y[:, None]], 1).astype(np.float32)
    cols = [f"R{i}" for i in range(10)] + ["Y"]
    edges = [(f"R{i}", "Y") for i in range(10)]
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=20))
    ora = _oracle_from_bn(bn, edges, cols, data, "linear_regression")
    N = 16 if observed == 10 else 4
    ev = sample_evidence(data, cols, cols[:observed], 300, 6)
    random.seed(2)
    ref, rdom, kw = oracle_reference(ora, "Y", ev, N)
    random.seed(2)
    pdf, dom = bn.infer("Y", _t(ev, gpu), N_max=N)
    np.testing.assert_array_equal(dom.cpu().numpy(), rdom)
    assert_marginals_close(pdf.cpu().numpy(), ref, **kw)


def test_subnormal_densities_in_infer(gpu):
    """Factors whose densities fall below 2^-126 inside a full infer (a sharp
    LinearRegression, sigma = 0.03): the unnormalised products agree with the
    oracle's float32 ones to rtol 1e-5 plus eight subnormal steps (2^-146: a
    subnormal density carries its few-ulp error as an absolute one, and the
    product rounds it once more), and the
    normalised marginals to the north-star tolerance."""
    rng = np.random.default_rng(9)
    S = 3000
    x0 = np.round(rng.normal(0, 1, S), 2)
    x1 = np.round(x0 + rng.normal(0, 0.03, S), 2)
    data = np.stack([x0, x1], 1).astype(np.float32)
    cols, edges = ["X0", "X1"], [("X0", "X1")]
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=5))
    _set_linear(bn.nodes_obj["X1"].estimator, [[1.0]], [0.0], float(np.log(0.03)), gpu)
    ora = _oracle_from_bn(bn, edges, cols, data, "linear_regression")
    ev = {"X0": (x0[rng.integers(0, S, 4000)] + rng.uniform(-0.2, 0.2, 4000)).astype(np.float32)[:, None]}
    rows, _, words, scale = bn.engine.infer_raw("X1", _t(ev, gpu), 16)
    raw = rows.cpu().numpy().copy()
    ref_raw, _ = ora.infer_raw("X1", ev, 16)
    tiny = 2.0 ** -126
    sub = (ref_raw > 0) & (ref_raw < tiny)
    assert sub.sum() > 100  # the case is exercised
    np.testing.assert_allclose(raw, ref_raw, rtol=RTOL, atol=2.0 ** -146)
    scale(rows, words)
    assert_marginals_close(rows.cpu().numpy(), ref_raw / ref_raw.max(), raw_max=float(ref_raw.max()),
                           n_factors=n_factors(ora, "X1"), peak=oracle_peak(ora, "X1"))


# ---------------------------------------------------------------------------
# Order guard of the factor split (round 6).  The M1 linear kernels multiply
# the factors in 4 contiguous ranges from 1 and then multiply the ranges
# together; the reference keeps ONE running product (bayesian_network.py:269,
# :293).  Where a range's own product under- or overflows while the running
# product does not (or the reverse), the orders give different numbers; the
# kernel then recomputes that wave in the reference's order (cbn_param.hip,
# FSplit).  24-node LinearRegression chain, N = 16 = every node's domain
# {0.0, 0.1, ..., 1.5}: the plan splits its 24 factors [0, 7) [7, 13) [13, 19)
# [19, 24) (the host's cost balance: root 1, each query factor 242).
_GUARD_N = 24
_GUARD_DOM = (np.arange(16) * 0.1).astype(np.float32)


def _guard_chain(gpu, sigmas):
    rng = np.random.default_rng(61)
    cols = [f"X{i}" for i in range(_GUARD_N)]
    edges = [(cols[i], cols[i + 1]) for i in range(_GUARD_N - 1)]
    data = _GUARD_DOM[rng.integers(0, 16, (2000, _GUARD_N))]
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=1))
    _set_linear(bn.nodes_obj["X0"].estimator, [[0.0]], [0.7], 0.0, gpu)
    for i in range(1, _GUARD_N):  # mu = the parent's evidence
        _set_linear(bn.nodes_obj[cols[i]].estimator, [[1.0]], [0.0], float(np.log(sigmas[i])), gpu)
    ora = _oracle_from_bn(bn, edges, cols, data, "linear_regression")
    return bn, ora, cols


def _guard_evidence(cols, Q, offsets):
    """Evidence of X0..X22: X_{i-1} = s_7 + offsets[i] (query-dependent rows of offsets)."""
    ev = {}
    for i in range(1, _GUARD_N):
        ev[cols[i - 1]] = (_GUARD_DOM[7] + offsets[i]).astype(np.float32)[:, None]
    return ev


def _guard_check(bn, ora, ev, gpu):
    rows, _, words, scale = bn.engine.infer_raw(cols_target := f"X{_GUARD_N - 1}", _t(ev, gpu), 16)
    raw = rows.cpu().numpy().copy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ref_raw, _ = ora.infer_raw(cols_target, ev, 16)
        ref = ref_raw / ref_raw.max()
    np.testing.assert_array_equal(np.isnan(raw), np.isnan(ref_raw))
    np.testing.assert_array_equal(np.isinf(raw), np.isinf(ref_raw))
    fin = np.isfinite(ref_raw)
    np.testing.assert_allclose(raw[fin], ref_raw[fin], rtol=RTOL, atol=2.0 ** -146)
    scale(rows, words)
    out = rows.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(out), np.isnan(ref))
    # the overflow case is NaN by design (inf / inf; every finite row is x / inf
    # = 0): NaN positions and the unnormalised rows; the other two are finite
    kw = dict(raw_max=float(ref_raw.max()), n_factors=n_factors(ora, cols_target), peak=oracle_peak(ora, cols_target))
    if np.isnan(ref).any():
        kw.update(nan="match", got_raw=raw, ref_raw=ref_raw)
    assert_marginals_close(out, ref, **kw)
    pdf, _ = bn.infer(cols_target, _t(ev, gpu), N_max=16)  # the fused / two-pass path too
    assert_marginals_close(pdf.cpu().numpy(), ref, **kw)
    return ref_raw


def test_split_order_guard_range_underflow(gpu):
    """Part 0's six sharp factors (sigma 1e-4, evidence at the mean: 3989 each)
    lift the running product to ~1e21; part 1's six factors sit 7.2-7.4 sigma
    off (~1e-8 each): that range's product alone (~1e-48) flushes to 0, the
    reference's running product (~1e-27) stays normal.  Unguarded, the split
    returned 0 for every row's only nonzero column."""
    sig = [1.0] + [1e-4] * 12 + [1.0] * (_GUARD_N - 13)
    bn, ora, cols = _guard_chain(gpu, sig)
    Q = 4096
    rng = np.random.default_rng(5)
    off = np.zeros((_GUARD_N, Q), np.float32)
    off[7:13] = rng.uniform(7.2e-4, 7.4e-4, (6, Q)).astype(np.float32)  # parts 1's factors X7..X12
    ref_raw = _guard_check(bn, ora, _guard_evidence(cols, Q, off), gpu)
    P1 = np.prod([3989.4 * np.exp(-0.5 * (off[i] / 1e-4) ** 2) for i in range(7, 13)], axis=0)
    assert (P1 < 2.0 ** -149).all() and (ref_raw[:, 7] > 2.0 ** -120).all()  # the case is exercised


def test_split_order_guard_running_overflow(gpu):
    """The mirror: the reference's running product overflows inside part 1
    (1e21 x 3989^5 > FLT_MAX) and stays inf -- its max is inf, so those rows
    normalise to NaN and every finite row to 0 -- while part 1's own range
    (3989^5 x 1e-11) and the split's product stay finite.  Half the queries
    overflow; the other half keep part 1 far off its mean (finite rows)."""
    sig = [1.0] + [1e-4] * 12 + [1.0] * (_GUARD_N - 13)
    bn, ora, cols = _guard_chain(gpu, sig)
    Q = 2048
    off = np.zeros((_GUARD_N, Q), np.float32)
    off[12] = 8.0e-4  # X12 (last of part 1): 3989 e^-32
    off[8:12, Q // 2:] = 6.0e-4  # the finite half: X8..X11 at 6 sigma
    ref_raw = _guard_check(bn, ora, _guard_evidence(cols, Q, off), gpu)
    assert np.isinf(ref_raw[: Q // 2, 7]).all() and np.isfinite(ref_raw[Q // 2:]).all()


def test_split_order_guard_quiet_case(gpu):
    """Every range and every running product normal (parts 1.. near their
    means): the split's products are kept, and agree with the reference's
    order to the north-star tolerance on every row."""
    sig = [1.0] + [0.05] * 12 + [1.0] * (_GUARD_N - 13)
    bn, ora, cols = _guard_chain(gpu, sig)
    Q = 4096
    rng = np.random.default_rng(8)
    off = rng.uniform(-0.02, 0.02, (_GUARD_N, Q)).astype(np.float32)
    ref_raw = _guard_check(bn, ora, _guard_evidence(cols, Q, off), gpu)
    assert (ref_raw[:, 7] > 2.0 ** -100).all()


# ---------------------------------------------------------------------------
# Special evidence values through the parametric kernels.  The reference's
# densities are plain float arithmetic: a NaN parent value gives a NaN mean and
# a NaN row, +-inf gives a zero Gaussian (exp(-inf)) and NaN or 0 for the
# logistic density, and out_pdf.max() (bayesian_network.py:296) spreads one NaN
# over the whole batch.  The oracle is pinned to the reference on these inputs
# by tests/golden/activation_special.npz and special_param_*.npz; here the
# kernels are compared with it on the same parameters: NaN / inf positions of
# the UNnormalised rows equal, finite values at rtol 1e-5, every untouched row
# bit-identical to the same row of the clean batch.
SPECIAL_ROWS = ((50, np.nan), (100, np.inf), (150, -np.inf))


def _special_param_check(bn, ora, target, ev, clean, N, gpu, expect_nan=True):
    from continuousbayesiannetwork_amd import _native

    eng = bn.engine
    res = eng.infer_raw(target, _t(ev, gpu), N)
    assert res is not None
    raw, words = res[0].cpu().numpy().copy(), res[2].clone()
    out = res[3](res[0], words).cpu().numpy().copy()
    flags = [_native.load().cbn_plan_flags(p.handle) for p in eng._plans.values()]
    assert flags and all(f & _native.CBN_PLAN_PARAMETRIC for f in flags)
    raw_clean = eng.infer_raw(target, _t(clean, gpu), N)[0].cpu().numpy().copy()
    with np.errstate(all="ignore"):
        ref_raw, _ = ora.infer_raw(target, ev, N)
        ref = (ref_raw / ref_raw.max()).astype(np.float32)
    kw = dict(raw_max=float(ref_raw.max()), n_factors=n_factors(ora, target), peak=oracle_peak(ora, target))
    assert bool(np.isnan(ref_raw).any()) == expect_nan
    if expect_nan:
        assert np.isnan(ref).all()  # one NaN row: the batch max, and so every entry
        assert_marginals_close(out, ref, nan="match", got_raw=raw, ref_raw=ref_raw, **kw)
        assert np.isnan(out).all()
    else:
        assert np.isfinite(raw).all()
        assert_marginals_close(out, ref, **kw)
    pdf, _ = bn.infer(target, _t(ev, gpu), N_max=N)  # the fused / two-pass path
    np.testing.assert_array_equal(np.isnan(pdf.cpu().numpy()), np.isnan(ref))
    touched = np.zeros(raw.shape[0], bool)
    for k in ev:
        touched |= ~((ev[k] == clean[k]).all(1))  # (NaN != NaN: a NaN row counts as touched)
    assert 0 < touched.sum() <= 16
    np.testing.assert_array_equal(raw[~touched].view(np.uint32), raw_clean[~touched].view(np.uint32))
    assert np.isfinite(raw_clean).all() and (raw_clean > 0).any(1).mean() > 0.9
    return raw, ref_raw


# [16]: the pair-packed one-hidden-layer form; [7]: an odd width (a padding unit
# in the last pair, 0 x inf there must not reach mu); [8, 8]: the multi-layer
# register form; [33, 4]: beyond the register-resident kernels (k_param_query_gen)
@pytest.mark.parametrize("hidden", [[16], [7], [8, 8], [33, 4]], ids=["h16", "h7", "h8x8", "h33x4"])
@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "leakyrelu", "gelu", "elu"])
def test_special_evidence_through_activations(act, hidden, gpu):
    data, cols, edges = mixed_dag_data(1500, 4, n=6, unit=True)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="neural_network",
                 config=param_config("neural_network", n_epochs=5, model={"hidden_dims": hidden, "activation": act}))
    ora = _oracle_from_bn(bn, edges, cols, data, "neural_network", act)
    clean = sample_evidence(data, cols, cols[:-1], 256, 3)
    ev = {k: v.copy() for k, v in clean.items()}
    for r, v in SPECIAL_ROWS:
        ev[cols[-2]][r, 0] = v  # X4 -> X5 (the backbone edge): the target's own factor reads it
    raw, ref_raw = _special_param_check(bn, ora, cols[-1], ev, clean, 8, gpu)
    assert np.isnan(ref_raw[50]).all() and np.isnan(raw[50]).all()


@pytest.mark.parametrize("k,n_obs", [(1, 1), (3, 3), (4, 4), (5, 5), (2, 1), (3, 1)])
def test_special_evidence_linear_regression_parents(k, n_obs, gpu):
    """A LinearRegression node with k parents (1, 3, 4: the zero-padded
    4-input weights and the column table's null pointers; 5: beyond them), one
    parent special and the others finite; n_obs < k: free parents beside the
    observed special one (the per-combo inputs).  +-inf evidence: the Gaussian
    is exactly 0 (exp(-inf)) and the rest of the batch stays finite."""
    rng = np.random.default_rng(40 + k)
    S, Q, N = 3000, 256, 8
    R = np.round(rng.normal(0, 1, (S, k)), 2)
    Y = np.round(R @ rng.uniform(0.3, 0.8, k) + rng.normal(0, 0.5, S), 2)
    data = np.concatenate([R, Y[:, None]], 1).astype(np.float32)
    cols = [f"R{i}" for i in range(k)] + ["Y"]
    edges = [(f"R{i}", "Y") for i in range(k)]
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=20))
    ora = _oracle_from_bn(bn, edges, cols, data, "linear_regression")
    assert (bn.nodes_obj["Y"].estimator.linear_model.weight.detach().cpu().numpy() != 0).all()  # (w x inf = +-inf)
    clean = sample_evidence(data, cols, cols[:n_obs], Q, 6)
    inf_only = {c: v.copy() for c, v in clean.items()}
    for i in range(n_obs):  # each observed parent in turn
        inf_only[cols[i]][100 + i, 0] = np.inf
        inf_only[cols[i]][150 + i, 0] = -np.inf
    raw, ref_raw = _special_param_check(bn, ora, "Y", inf_only, clean, N, gpu, expect_nan=False)
    hit = [100 + i for i in range(n_obs)] + [150 + i for i in range(n_obs)]
    assert (raw[hit] == 0).all() and (ref_raw[hit] == 0).all()
    ev = {c: v.copy() for c, v in inf_only.items()}
    for i in range(n_obs):
        ev[cols[i]][50 + i, 0] = np.nan if i % 2 == 0 else np.copysign(np.float32(np.nan), np.float32(-1))
    raw, ref_raw = _special_param_check(bn, ora, "Y", ev, clean, N, gpu)
    assert np.isnan(raw[50:50 + n_obs]).all() and (raw[hit] == 0).all()


def test_split_order_guard_nan_row(gpu):
    """The 4-part split with its order guard (the quiet case's chain): one
    query's evidence is NaN.  That row is NaN; the guard decides per row, so
    every other row's unnormalised values are those of the clean batch."""
    sig = [1.0] + [0.05] * 12 + [1.0] * (_GUARD_N - 13)
    bn, ora, cols = _guard_chain(gpu, sig)
    Q = 512
    rng = np.random.default_rng(8)
    off = rng.uniform(-0.02, 0.02, (_GUARD_N, Q)).astype(np.float32)
    clean = _guard_evidence(cols, Q, off)
    for col, row, v in ((cols[10], 77, np.nan), (cols[3], 300, np.copysign(np.float32(np.nan), np.float32(-1)))):
        ev = {k: a.copy() for k, a in clean.items()}
        ev[col][row, 0] = v
        raw, ref_raw = _special_param_check(bn, ora, cols[-1], ev, clean, 16, gpu)
        assert np.isnan(raw[row]).all() and np.isfinite(np.delete(raw, row, 0)).all()


@pytest.mark.parametrize("negative", [False, True], ids=["nan", "negative_nan"])
def test_sharded_raw_path_with_a_nan_row(negative, gpu):
    """sharded_infer's raw path, one rank over 3 ragged shards, the NaN row in
    the middle shard: the NaN max word wins the MAX over the shards' int32
    words (a NaN with its sign bit set included) and reaches the scale, so
    every shard's rows are NaN, as the single call's are."""
    from continuousbayesiannetwork_amd.distributed import shard_evidence, sharded_infer

    data, cols, edges = mixed_dag_data(4000, 6, n=16)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator="linear_regression",
                 config=param_config("linear_regression", n_epochs=10))
    Q = 1001
    ev = sample_evidence(data, cols, cols[:-1], Q, 11)
    ev[cols[-2]][500, 0] = np.copysign(np.float32(np.nan), np.float32(-1)) if negative else np.nan
    evt = _t(ev, gpu)
    full = bn.infer(cols[-1], evt, N_max=16)[0].clone()
    assert torch.isnan(full).all()
    rows, bits, scales = [], [], []
    for r in range(3):
        o, _, b, sc = bn.engine.infer_raw(cols[-1], shard_evidence(evt, 3, r), 16)
        rows.append(o.clone())
        bits.append(b.clone())
        scales.append(sc)
    assert [o.shape[0] for o in rows] != [Q // 3] * 3 and sum(o.shape[0] for o in rows) == Q
    assert torch.isfinite(rows[0]).all() and torch.isfinite(rows[2]).all() and torch.isnan(rows[1]).any()
    m = torch.stack(bits).max(0).values  # the all-reduce's MAX over int32 words
    for o, sc in zip(rows, scales):
        sc(o, m)
        assert torch.isnan(o).all()
    np.testing.assert_array_equal(torch.cat(rows).cpu().numpy(), full.cpu().numpy())  # (NaN == NaN here)
    one, _ = sharded_infer(bn, cols[-1], evt, N_max=16)
    np.testing.assert_array_equal(one.cpu().numpy(), full.cpu().numpy())
