"""[Q, N] evidence columns on parametric networks, without a GPU.

* The CPU oracle reproduces the reference-run fixtures of
  tests/golden/make_golden_param_wide.py (``param_wide_cases.assert_wide_golden``:
  ``parity.assert_marginals_close`` at the project's tolerance, scaled by the
  reference's own unnormalised batch max, which each of these fixtures holds);
  for the fixture with a NaN, a +inf and a -inf entry: NaN positions and the
  unnormalised rows.
* ``CBN_INPUT_WIDE`` in include/cbn_amd.h and in ``_native`` agree.
* ``InferenceEngine.check_columns`` returns the wide set {C} for the fixtures'
  evidence, and raises the reference's message for a width-N column on a parent
  that a node reads strictly (its evidence keys equal its parents).
* Every case of tests/test_gpu_param_wide.py's kernel matrix can be checked by
  the oracle alone: finite rows, a normal batch max, every compared row holding
  an entry the relative tolerance governs (as tests/test_param_matrix_cases.py).
"""
import os
import random
import re

import numpy as np
import pytest
import torch

import param_wide_cases as pw
from continuousbayesiannetwork_amd import BayesianNetwork, _native
from continuousbayesiannetwork_amd.inference.engine import InferenceEngine, Plan, build_factor_specs, relevant_observed
from golden_io import load_param_golden
from helpers import make_bn
from parity import FLT_MIN, coverage, oracle_raw, oracle_reference

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cbn_amd.h")


def test_manifest_lists_the_six_cases():
    names = pw.wide_golden_names()
    assert len(names) == 6 and len(set(names)) == 6
    for name in names:
        g = load_param_golden(name)
        m = g["meta"]
        N = m["N_max"]
        assert m["target"] == "E" and m["wide"] == ["C"] and 12 <= g["pdf"].shape[0] <= 24
        assert g["evidence"]["C"].shape == (g["pdf"].shape[0], N) and g["raw"].shape == g["pdf"].shape
        assert all(v.shape[1] == 1 for k, v in g["evidence"].items() if k != "C")
        assert os.path.getsize(os.path.join(pw.GOLDEN_DIR, name + ".npz")) < 16 * 1024


@pytest.mark.parametrize("name", pw.wide_golden_names())
def test_oracle_reproduces_the_reference(name):
    g = load_param_golden(name)
    m = g["meta"]
    ora = pw.golden_oracle(g)
    ev = {k: g["evidence"][k] for k in m["evidence"]}
    raw, _ = oracle_raw(ora, m["target"], ev, m["N_max"], seed=m["seed"])
    random.seed(m["seed"])
    with np.errstate(all="ignore"):
        pdf, dom = ora.infer(m["target"], ev, m["N_max"])
    np.testing.assert_array_equal(dom, g["domain"])
    if m["special"]:
        rows = sorted({r for r, _ in m["special"]})
        assert len(rows) == 3 and not np.isfinite(g["evidence"]["C"][rows]).all(1).any()
        clean = np.delete(np.arange(raw.shape[0]), rows)
        assert np.isfinite(g["raw"][clean]).all() and np.isnan(g["raw"][rows]).any()
        assert np.array_equal(np.isnan(raw), np.isnan(g["raw"]))
        assert np.isnan(g["pdf"]).all()  # the batch max is NaN (bayesian_network.py:296)
    else:
        assert np.isfinite(g["raw"]).all()
        np.testing.assert_allclose(raw, g["raw"], rtol=1e-5, atol=0)
    pw.assert_wide_golden(pdf, g, got_raw=raw)


def test_wide_slot_encoding_agrees_with_the_header():
    text = open(HEADER).read()
    m = re.search(r"#define\s+CBN_INPUT_WIDE\(slot\)\s+\((-?\d+)\s*-\s*\(slot\)\)", text)
    assert m, "CBN_INPUT_WIDE(slot) not found in include/cbn_amd.h"
    base = int(m.group(1))
    assert base == -16 == _native.CBN_INPUT_WIDE_BASE
    for slot in (0, 1, 7, _native.CBN_MAX_EVIDENCE - 1):
        assert _native.CBN_INPUT_WIDE(slot) == base - slot <= -16
    assert _native.CBN_INPUT_FREE == -1 and _native.CBN_INPUT_ONE == -2
    assert re.search(r"#define\s+CBN_AMD_ABI_VERSION\s+6\b", text) and _native.ABI_VERSION == 6


def _host_plan(g, target, ev, N):
    m = g["meta"]
    bn = make_bn(BayesianNetwork, m["edges"], m["columns"], g["data"], device="cpu")
    order = bn.get_ancestors(bn.initial_dag, target) + [target]
    obs = relevant_observed(bn, order, ev.keys())
    random.seed(m["seed"])
    order, specs, tdom, det = build_factor_specs(bn, target, obs, N)
    return Plan(target, N, order, specs, sorted(obs), tdom, True, det)


@pytest.mark.parametrize("name", pw.wide_golden_names())
def test_check_columns_returns_the_wide_set(name):
    g = load_param_golden(name)
    m = g["meta"]
    ev = {k: torch.tensor(g["evidence"][k]) for k in m["evidence"]}
    plan = _host_plan(g, m["target"], ev, m["N_max"])
    assert InferenceEngine.check_columns(plan, ev) == {"C"}
    assert InferenceEngine.check_columns(plan, {k: v[:, :1] for k, v in ev.items()}) == set()


def test_width_n_column_on_a_strict_parent_raises_the_reference_message():
    g = load_param_golden("wide_lr_c_a")
    N = g["meta"]["N_max"]
    a = np.repeat(g["evidence"]["A"], N, 1)  # A as [Q, N]: D reads it strictly (its evidence keys == its parents)
    with pytest.raises(RuntimeError) as want:
        pw.golden_oracle(g).infer_raw("D", {"A": a}, N)
    plan = _host_plan(g, "D", {"A": torch.tensor(a)}, N)
    with pytest.raises(RuntimeError) as got:
        InferenceEngine.check_columns(plan, {"A": torch.tensor(a)})
    assert str(got.value) == str(want.value) and f"({N})" in str(got.value)
    # and below E, where C expands the same column: D's strict read raises first or last, but raises
    ev = {"C": torch.tensor(g["evidence"]["C"]), "A": torch.tensor(a)}
    with pytest.raises(RuntimeError) as got:
        InferenceEngine.check_columns(_host_plan(g, "E", ev, N), ev)
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("case", pw.CASES, ids=lambda c: c.id)
def test_case_is_checkable_by_the_oracle(case):
    _, _, _, target, _, wide, _ = pw.network(case)
    ev = {k: v[:case.rows] for k, v in pw.evidence(case, pw.SMALL).items()}
    for w in wide:
        assert ev[w].shape == (case.rows, case.N) and ev[w].min() >= -0.3 and ev[w].max() <= 1.3
    random.seed(0)
    with np.errstate(all="ignore"):
        ref, dom, kw = oracle_reference(pw.oracle(case), target, ev, case.N)
    assert ref.shape == (case.rows, case.N) and dom.shape[-1] == case.N
    assert np.isfinite(ref).all()
    assert FLT_MIN <= kw["raw_max"] < np.inf
    (entries, rows_share), _ = coverage(ref, **kw)
    print(f"{case.id}: raw max {kw['raw_max']:.3e}, rtol governs {entries:.3f} of the entries, {rows_share:.3f} of the rows")
    assert rows_share == 1.0


def test_case_table_reaches_every_family():
    inst = {(c.info["generic"], c.info["nc"], c.info["hmax"], c.info["mode"], c.info["tab"]) for c in pw.CASES}
    want = {(0, 8, 0, m, 1) for m in range(4)}                         # linear, MODE 0-3
    want |= {(0, nc, 1, m, 1) for nc in (8, 16, 32) for m in (2, 3)}   # one hidden layer
    want |= {(0, 8, 32, 2, 1), (0, 32, 32, 3, 1)}                      # deep LDS scratch
    want |= {(0, 16, 32, 4, 0), (1, 16, 0, 4, 0)}                      # switch (slot mode), generic
    assert want <= inst, want - inst
    assert all(c.info["m1"] == 0 for c in pw.CASES)
    assert any(c.split for c in pw.CASES) and all(c.n >= 7 for c in pw.CASES if c.split)
