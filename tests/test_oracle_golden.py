"""The CPU oracle (oracle/ref_infer.py) against vectors produced by running the
reference itself (tests/golden/make_golden.py).  Tolerance: the oracle and the
reference sum the parent-axis means in different orders, so rtol 1e-5 (the
north-star fp32 bar) on every entry, plus the subnormal-rounding floor of
tests/parity.py scaled by the oracle's own unnormalised batch max."""
import random

import numpy as np
import pytest

from golden_io import golden_error, golden_names, load_golden, load_param_golden, oracle_estimators, param_golden_names
from oracle.ref_infer import OracleBN
from parity import MIN_CHECKED_ROWS, assert_marginals_close, golden_scale, n_factors, oracle_raw


def _infer_keeping_raw(bn, target, ev, N):
    """``bn.infer`` (the oracle's own division by the batch max), plus the
    unnormalised rows that same call divided: one oracle pass."""
    kept, inner = {}, bn.infer_raw

    def run(*a):
        out, dom = inner(*a)
        kept["raw"] = out
        return out, dom

    bn.infer_raw = run
    with np.errstate(invalid="ignore", over="ignore"):  # the NaN fixtures: 0 / 0, inf / inf
        pdf, dom = bn.infer(target, ev, N)
    return pdf, dom, kept["raw"]


def _check_golden(name, param, pdf, ref, raw, ref_raw=None):
    """The oracle's marginals vs the reference's through the helper, and the
    committed raw max (tests/golden/oracle_raw_max.json) vs the oracle's run."""
    mx, nf, pk = golden_scale(name, param)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(np.float32(mx), raw.max())  # NaN == NaN here
    if np.isnan(ref).any():
        # NaN by design (0 / 0: every product of the batch is 0; the logistic
        # density's inf / inf; or a NaN / inf evidence value).  The older
        # reference fixtures hold no unnormalised rows, so the oracle's own
        # stand on both sides: what this adds to the NaN positions is the cause
        # -- a batch max of 0, inf or NaN.  The special-evidence fixtures hold
        # the reference's rows (``ref_raw``): NaN / inf positions equal, the
        # finite rows at rtol
        assert np.isnan(ref).all() and not (raw.max() > 0 and np.isfinite(raw.max()))
        assert_marginals_close(pdf, ref, raw_max=mx, n_factors=nf, peak=pk, nan="match", got_raw=raw,
                               ref_raw=raw if ref_raw is None else ref_raw)
    else:
        assert_marginals_close(pdf, ref, raw_max=mx, n_factors=nf, peak=pk,
                               min_checked_rows=MIN_CHECKED_ROWS.get(name, 0.5))


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_reference_golden(name):
    g = load_golden(name)
    m = g["meta"]
    bn = OracleBN(m["edges"], m["columns"], g["data"])
    random.seed(m["seed"])
    ev = None if m["evidence_none"] else {k: g["evidence"][k] for k in m["evidence"]}
    if m["error"]:
        exc, msg = golden_error(m)
        with pytest.raises(exc) as info:
            if ev is None:
                ev.items()
            bn.infer(m["target"], ev, m["N_max"])
        if exc is RuntimeError:  # the evidence-width errors: the reference's message too
            assert str(info.value) == msg
        return
    pdf, dom, raw = _infer_keeping_raw(bn, m["target"], ev, m["N_max"])
    assert pdf.shape == g["pdf"].shape
    np.testing.assert_array_equal(dom, g["domain"])
    _check_golden(name, False, pdf, g["pdf"], raw)
    assert (pdf[g["pdf"] == 0] == 0).all()  # what the reference zeroed (an unmatched evidence value) is exactly 0


def test_golden_manifest_covers_config0():
    """BASELINE configs[0]: 5-node chain, d=4, 1024 queries on the reference CPU path."""
    g = load_golden("chain5_d4_q1024_parent")
    assert g["pdf"].shape == (1024, 4)
    assert len(g["meta"]["columns"]) == 5


@pytest.mark.parametrize("name", param_golden_names())
def test_oracle_parametric_matches_reference_golden(name):
    """LinearRegression / LogisticRegression / NeuralNetwork networks: the
    oracle, given the reference's fitted parameters, reproduces the reference's
    infer output (NaN where the reference's logistic density overflows)."""
    g = load_param_golden(name)
    m = g["meta"]
    bn = OracleBN(m["edges"], m["columns"], g["data"], estimators=oracle_estimators(g))
    random.seed(m["seed"])
    ev = {k: g["evidence"][k] for k in m["evidence"]}
    pdf, dom, raw = _infer_keeping_raw(bn, m["target"], ev, m["N_max"])
    assert pdf.shape == g["pdf"].shape
    np.testing.assert_array_equal(dom, g["domain"])
    _check_golden(name, True, pdf, g["pdf"], raw, g.get("raw"))
    if "raw" in g:  # the case is exercised: NaN rows beside finite, nonzero ones
        assert np.isnan(g["raw"][5]).all() and (np.isfinite(g["raw"]).all(1) & (g["raw"] > 0).any(1)).sum() >= 16


ACTIVATIONS = ["relu", "tanh", "sigmoid", "leakyrelu", "gelu", "elu"]


@pytest.mark.parametrize("act", ACTIVATIONS)
def test_oracle_activation_matches_reference_on_special_values(act):
    """``_act`` vs the reference's own torch modules (tests/golden/
    make_golden_activation.py) at NaN of both signs, +-inf, +-0, subnormals,
    +-2^-126, 0.625 and its float neighbours, 88.7, 104, 1e30, FLT_MAX: NaN
    positions, inf positions and zeros WITH their sign exactly; every other
    value at this file's rtol 1e-5 plus one subnormal step (a single value,
    parity.assert_factor_close)."""
    import os

    from oracle.ref_infer import _act
    from parity import assert_factor_close

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activation_special.npz"))
    x, ref = z["x"], z["y_" + act]
    assert x.size == 24 and np.isnan(x[:2]).all() and np.signbit(x[1]) and np.isinf(x[-2:]).all()
    assert sorted(k[2:] for k in z.files if k.startswith("y_")) == sorted(ACTIVATIONS)
    with np.errstate(all="ignore"):
        got = _act(act, x.copy())
    assert got.dtype == np.float32
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf), ("zero", lambda a: a == 0)):
        assert np.array_equal(f(got), f(ref)), f"{act}: {name} positions differ at x = {x[f(got) != f(ref)]}"
    zero = ref == 0
    assert np.array_equal(np.signbit(got[zero]), np.signbit(ref[zero])), \
        f"{act}: signs of zero differ at x = {x[zero][np.signbit(got[zero]) != np.signbit(ref[zero])]}"
    fin = np.isfinite(ref) & ~zero
    assert fin.sum() >= 8
    assert_factor_close(got[fin], ref[fin])


def _full(name):
    import json
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
    return z["rows"], z["pdf"], z["domain"], json.loads(str(z["meta"]))


@pytest.mark.parametrize("name,gen", [("chain20_d32_bench65536", "chain"), ("alarm37_d8_bench262144", "alarm")])
def test_oracle_matches_full_batch_golden(name, gen):
    """The full-batch reference goldens (tests/golden/make_golden_full.py): the
    oracle on a few rows plus the batch argmax row (so it normalises by the same
    max as the reference's whole-batch call) reproduces those rows."""
    from helpers import alarm_like_data, chain_data, sample_evidence

    rows, ref, rdom, m = _full(name)
    if gen == "chain":
        data, cols, edges = chain_data(20, 32, 200_000, 3, stay=0.8)
    else:
        data, cols, edges = alarm_like_data(200_000, 5)
    ev = sample_evidence(data, cols, [c for c in cols if c != m["target"]], m["Q"], m["ev_seed"])
    pick = np.array([0, 1, 2, 3, 5, 8, 13, 21, int(np.searchsorted(rows, m["argmax_row"]))])
    sub = rows[pick]
    bn = OracleBN(edges, cols, data)
    pdf, dom = bn.infer(m["target"], {k: v[sub] for k, v in ev.items()}, m["N_max"])
    assert (rdom == rdom[:1]).all()  # one sample domain per query row
    np.testing.assert_array_equal(dom, np.broadcast_to(rdom[:1], dom.shape))
    assert pdf[-1].max() == 1.0
    # the batch max M: the oracle's unnormalised argmax row alone (one row)
    _, mx = oracle_raw(bn, m["target"], {k: v[rows[pick[-1:]]] for k, v in ev.items()}, m["N_max"])
    assert_marginals_close(pdf, ref[pick], raw_max=mx, n_factors=n_factors(bn, m["target"]))


def test_grid_oracle_fixture_matches_reference_run():
    """BASELINE configs[4]'s plan (10 x 10 grid, d = N = 64, 100 factors): the
    oracle fixture (tests/golden/make_grid_oracle.py, 64 queries) against the
    reference's own infer on the same 64 queries (make_golden_full.py
    grid10_d64_peaked_ref64), at the north-star tolerance; same domain."""
    import os

    rows, ref, rdom, m = _full("grid10_d64_peaked_ref64")
    assert m["Q"] == 64 and list(rows) == list(range(64)) and m["N_max"] == 64
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid10_d64_peaked_oracle.npz"))
    assert (rdom == rdom[:1]).all() and (z["domain"] == rdom[:1]).all()
    assert np.isfinite(ref).all() and ref.max() == 1.0
    # the oracle fixture holds normalised rows only; every factor is <= 1, so
    # 1 bounds the unnormalised max from above: a floor of 100 subnormal steps,
    # tighter than the one the true max would give.  29 of the 64 queries have
    # a nonzero row (peaked CPDs: the rest meet an unseen parent combination)
    assert_marginals_close(z["pdf"], ref, raw_max=1.0, n_factors=100, min_checked_rows=0.45)


def test_free_parent_grid_fixtures_regenerate_their_inputs():
    """The free-parent grid fixtures' data and evidence come back bit for bit
    from the committed generators (tests/helpers.py grid_rows_data /
    grid_rows_evidence / grid_data), so the GPU tests rebuild exactly the
    reference's inputs; their outputs are finite and non-degenerate."""
    import json
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from make_golden_full import CASES, digest, make_case

    for name in ("grid10_d64_dense_ref", "grid10_d64_rows_ref", "grid10_d64_rows_x99_ref"):
        z = np.load(os.path.join(here, "golden", name + ".npz"))
        meta = json.loads(str(z["meta"]))
        data, cols, edges, ev = make_case(CASES[name])
        assert digest([data]) == meta["data_sha256"], name
        assert digest([ev[k] for k in sorted(ev)]) == meta["evidence_sha256"], name
        assert sorted(ev) == meta["evidence_columns"]
        assert all((int(k[1:]) // 10) % 2 == 0 for k in ev)  # even grid rows only
        pdf = z["pdf"]
        assert np.isfinite(pdf).all() and pdf.max() == 1.0
        if name == "grid10_d64_dense_ref":
            assert (pdf > 0).mean() >= 0.2
