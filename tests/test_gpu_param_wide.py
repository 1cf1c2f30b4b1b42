"""[Q, N] evidence columns on parametric networks, on the GPU.

A node whose evidence keys are not all of its parents reads an evidence column
of width N_max as N per-query values of that parent (node.py:246-248); they
are axes of the combo mean like the free parents' sample points.  The engine
runs such calls on a parametric wide plan (``InferenceEngine._wide_plan``:
CBN_INPUT_WIDE inputs of ``cbn_param_factor``), through ``k_param_query``'s
``!M1`` forms and ``k_param_query_gen``.

1. The reference-run fixtures (tests/golden/make_golden_param_wide.py):
   ``infer`` and a repeat call against ``pdf``, ``infer_raw`` against ``raw``,
   ``sharded_infer`` without a process group bit-equal to ``infer``; the
   fixture with a NaN, a +inf and a -inf entry by NaN positions and raw rows,
   its other rows bit-equal to the call with those entries made finite.  Their
   sample domains are redrawn (N above A's and D's 3 levels): the plans are
   rebuilt per call and leave no plan alive.
2. Every kernel family that can take a wide factor (tests/param_wide_cases.py)
   against the oracle: the wide plan's ``cbn_plan_param_info`` first, then a
   257-row batch -- normalised and raw rows on the first rows and the arg-max
   row, prefixes of 1, 63, 64 and 65 rows and a row-shuffled batch bit-equal to
   the same rows of the 257-row launch (a lane-indexed or mis-strided column
   read shows there), ``infer`` == raw + scale.
3. A constant wide column against the [Q, 1] call with the same values (both
   against the oracle; not bit-equal, M differs).
4. ``predict`` / ``posterior`` / ``quantile`` on a wide call against the
   references applied to that call's ``infer_raw`` rows (the criteria of the
   existing reduction tests' fallback plans).
5. What stays declined: ``ShardedStepper`` with a wide column
   (NotImplementedError); a wide column on a strictly read parent
   (the reference's RuntimeError), after which the plan still serves [Q, 1].
"""
import random

import numpy as np
import pytest
import torch

import param_wide_cases as pw
from continuousbayesiannetwork_amd import BayesianNetwork, _native
from golden_io import load_param_golden
from helpers import make_bn, param_config
from parity import assert_marginals_close, oracle_raw, oracle_reference
from predict_ref import check_exact
from test_gpu_param import load_fixture_params

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def _t(ev, dev):
    return {k: torch.tensor(v, device=dev) for k, v in ev.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------- 1. reference fixtures -----
def _fixture_bn(g, gpu, tmp_path):
    m = g["meta"]
    bn = make_bn(BayesianNetwork, m["edges"], m["columns"], g["data"], device=gpu, estimator=m["estimator"],
                 config=param_config(m["estimator"], n_epochs=1, model=m["model"] or None))
    load_fixture_params(bn, g, tmp_path, gpu)
    return bn


def _raw_rows(bn, m, ev, gpu):
    """The call's unnormalised rows as ``sharded_infer`` gets them: the call's
    plan with its draws made, then the raw launch -- ``infer_raw`` on a kept
    plan's fast path, ``raw_wide_call`` on a plan rebuilt per call, which is
    destroyed after the call with its wide plan."""
    eng = bn.engine
    random.seed(m["seed"])
    plan, fp = eng.call_plan(m["target"], ev, m["N_max"])
    try:
        if fp is None:
            res = eng.raw_wide_call(plan, ev, None)
            assert res is not None and len(plan.wide_children) == 1
        else:
            res = eng.infer_raw(m["target"], ev, m["N_max"], fp=fp)
            assert res is not None
        torch.cuda.synchronize()
        return res[0].cpu().numpy().copy()
    finally:
        if not plan.deterministic and not plan.reusable:
            torch.cuda.current_stream().synchronize()
            plan.destroy()
            assert plan.handle is None and not plan.wide_children


@pytest.mark.parametrize("name", pw.wide_golden_names())
def test_reference_fixture(name, gpu, tmp_path):
    from continuousbayesiannetwork_amd.distributed import sharded_infer

    g = load_param_golden(name)
    m = g["meta"]
    N = m["N_max"]
    bn = _fixture_bn(g, gpu, tmp_path)
    ev = _t({k: g["evidence"][k] for k in m["evidence"]}, gpu)
    random.seed(m["seed"])
    pdf, dom = bn.infer(m["target"], ev, N_max=N)
    np.testing.assert_array_equal(dom.cpu().numpy(), g["domain"])
    pdf = pdf.cpu().numpy().copy()
    raw = _raw_rows(bn, m, ev, gpu)
    pw.assert_wide_golden(pdf, g, got_raw=raw)
    fin = np.isfinite(g["raw"])
    assert np.array_equal(np.isfinite(raw), fin)
    np.testing.assert_allclose(raw[fin], g["raw"][fin], rtol=RTOL, atol=0)
    # a repeat call, and sharded_infer without a process group: the same bits
    random.seed(m["seed"])
    again = bn.infer(m["target"], ev, N_max=N)[0].cpu().numpy()
    np.testing.assert_array_equal(_bits(again), _bits(pdf))
    random.seed(m["seed"])
    sh = sharded_infer(bn, m["target"], ev, N_max=N)[0].cpu().numpy()
    np.testing.assert_array_equal(_bits(sh), _bits(pdf))
    # redrawn domains: every plan of these calls was rebuilt per call and destroyed with its wide plan
    eng = bn.engine
    assert not eng._wide_plans and not eng._plans and not eng._fast
    if m["special"]:
        rows = sorted({r for r, _ in m["special"]})
        clean = np.delete(np.arange(raw.shape[0]), rows)
        assert np.isnan(pdf).all() and np.isfinite(raw[clean]).all()
        evf = {k: v.clone() for k, v in ev.items()}
        for r, a in m["special"]:
            evf["C"][r, a] = 0.25
        rawf = _raw_rows(bn, m, evf, gpu)
        assert np.isfinite(rawf).all()
        np.testing.assert_array_equal(_bits(rawf[clean]), _bits(raw[clean]))


# ------------------------------------------------- 2. kernel families --------
def _bn(case, gpu, tmp_path):
    data, cols, edges, _, _, _, params = pw.network(case)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator=case.est,
                 config=param_config(case.est, n_epochs=1, model=case.model))
    load_fixture_params(bn, {"meta": {"estimator": case.est}, "params": params}, tmp_path, gpu)
    return bn


def _raw(bn, target, evt, N):
    """(raw rows, scaled rows) of one raw launch + scale, as host copies."""
    res = bn.engine.infer_raw(target, evt, N)
    assert res is not None
    raw = res[0].cpu().numpy().copy()
    out = res[3](res[0], res[2]).cpu().numpy().copy()
    return raw, out


def _sub(rows, rstar):
    """``rows`` row indices of a batch: its first rows, the last one its arg-max row."""
    return np.array([r for r in range(rows) if r != rstar][:rows - 1] + [rstar])


def _against_oracle(ora, target, ev, sub, pdf, raw, N):
    """Rows ``sub`` (the last one the batch's arg-max row) against the oracle."""
    evs = {k: v[sub] for k, v in ev.items()}
    random.seed(0)
    with np.errstate(all="ignore"):
        ref, _, kw = oracle_reference(ora, target, evs, N, norm_row=-1)
        ref_raw, _ = oracle_raw(ora, target, evs, N)
    assert_marginals_close(pdf[sub], ref, **kw)
    np.testing.assert_allclose(raw[sub], ref_raw, rtol=RTOL, atol=kw["n_factors"] * 2.0 ** -149 * kw["peak"])


@pytest.mark.parametrize("case", pw.CASES, ids=lambda c: c.id)
def test_wide_kernel_case(case, gpu, tmp_path):
    target = pw.network(case)[3]
    N = case.N
    bn = _bn(case, gpu, tmp_path)
    ev = pw.evidence(case, pw.SMALL)
    evt = _t(ev, gpu)
    # the plan that serves the call
    wp = bn.engine.serving_plan(target, evt, N)
    assert wp is not bn.engine.call_plan(target, evt, N)[0]
    assert _native.load().cbn_plan_flags(wp.handle) & _native.CBN_PLAN_PARAMETRIC
    info = _native.param_info(wp.handle)
    assert {k: info[k] for k in case.info} == case.info, (case.id, info)
    assert 0 <= info["lds_bytes"] <= info["lds_limit"]
    bounds = _native.param_split(wp.handle)
    nf = len(wp.factors)
    assert len(bounds) == info["parts"] + 1 and bounds[0] == 0 and bounds[-1] == nf == case.n
    if case.split:  # the target's wide factor (the last one) runs in a part >= 1, the other wide factor in part 0
        assert info["parts"] > 1 and 0 < bounds[1] <= nf - 1 and nf - 2 < bounds[1], bounds

    raw, out = _raw(bn, target, evt, N)
    pdf = bn.infer(target, evt, N_max=N)[0].cpu().numpy().copy()
    assert pdf.shape == (pw.SMALL, N)
    np.testing.assert_array_equal(_bits(pdf), _bits(out))
    rstar = int(np.argmax(raw.max(1)))
    assert np.isfinite(raw).all() and pdf[rstar].max() == 1.0
    _against_oracle(pw.oracle(case), target, ev, _sub(case.rows, rstar), pdf, raw, N)

    for Q in (65, 64, 63, 1):
        evq = {k: v[:Q].contiguous() for k, v in evt.items()}
        rq, oq = _raw(bn, target, evq, N)
        np.testing.assert_array_equal(_bits(rq), _bits(raw[:Q]))
        pq = bn.infer(target, evq, N_max=N)[0].cpu().numpy()
        np.testing.assert_array_equal(_bits(pq), _bits(oq))
        assert oq.max() == 1.0
    perm = np.random.default_rng(7).permutation(pw.SMALL)
    rp, _ = _raw(bn, target, {k: v[torch.tensor(perm, device=gpu)].contiguous() for k, v in evt.items()}, N)
    np.testing.assert_array_equal(_bits(rp), _bits(raw[perm]))
    assert len(bn.engine._wide_plans) == 1  # one cached wide plan served every call


# ------------------------------------------------- 3. constant wide column ---
@pytest.mark.parametrize("cid", ["lin-mode1-N12", "h1-mode2-N16-w16relu"])
def test_constant_wide_column_matches_the_narrow_call(cid, gpu, tmp_path):
    case = pw.BY_ID[cid]
    _, _, _, target, _, wide, _ = pw.network(case)
    N, Q = case.N, 65
    bn = _bn(case, gpu, tmp_path)
    ev = pw.evidence(case, Q)
    narrow = dict(ev)
    narrow[wide[0]] = ev[wide[0]][:, :1].copy()
    const = dict(ev)
    const[wide[0]] = np.repeat(narrow[wide[0]], N, 1)
    ora = pw.oracle(case)
    got = {}
    for tag, e in (("narrow", narrow), ("const", const)):
        raw, out = _raw(bn, target, _t(e, gpu), N)
        rstar = int(np.argmax(raw.max(1)))
        _against_oracle(ora, target, e, _sub(case.rows, rstar), out, raw, N)
        got[tag] = raw
    # two evaluations of one quantity, each within rtol of its oracle
    np.testing.assert_allclose(got["const"], got["narrow"], rtol=2 * RTOL, atol=0)


# ------------------------------------------------- 4. reductions -------------
@pytest.mark.parametrize("cid", ["lin-mode0-N12", "h1-mode2-N16-w16relu"])
def test_reductions_on_a_wide_call(cid, gpu, tmp_path):
    from test_gpu_moments import check_case as check_moments
    from test_gpu_quantile import check_case as check_quantile

    case = pw.BY_ID[cid]
    target = pw.network(case)[3]
    N = case.N
    bn = _bn(case, gpu, tmp_path)
    evt = _t(pw.evidence(case, 300), gpu)
    index, value, row_max, had_raw = check_exact(bn, target, evt, N)
    assert had_raw and (row_max > 0).all()
    out = check_moments(bn, target, evt, N)
    assert out[5] and (out[1] > 0).all()
    q = check_quantile(bn, target, evt, N)
    assert q[5] == 0.0 and (q[2] > 0).all()
    wf = [int(_native.load().cbn_plan_flags(wp.handle)) for _, wp in bn.engine._wide_plans.values()]
    assert len(wf) == 1 and wf[0] & _native.CBN_PLAN_PARAMETRIC, wf


# ------------------------------------------------- 5. declines stay ----------
def test_sharded_stepper_declines_wide_columns(gpu, tmp_path):
    from continuousbayesiannetwork_amd.distributed import ShardedStepper

    case = pw.BY_ID["lin-mode0-N8"]
    target = pw.network(case)[3]
    bn = _bn(case, gpu, tmp_path)
    evt = _t(pw.evidence(case, 64), gpu)
    st = ShardedStepper(bn, target, case.N)
    try:
        with pytest.raises(NotImplementedError):
            st.step(evt)
    finally:
        st.close()


def test_strict_parent_wide_column_raises_and_the_plan_lives_on(gpu, tmp_path):
    case = pw.BY_ID["lin-mode0-N8"]
    _, cols, _, target, _, wide, _ = pw.network(case)
    N, Q = case.N, 65
    bn = _bn(case, gpu, tmp_path)
    ev = pw.evidence(case, Q)
    narrow = dict(ev)
    narrow[wide[0]] = ev[wide[0]][:, :1].copy()
    bad = dict(ev)
    bad[cols[1]] = np.repeat(ev[cols[1]], N, 1)  # X1 is read strictly by X2
    ora = pw.oracle(case)
    with pytest.raises(RuntimeError) as want:
        ora.infer_raw(target, bad, N)
    for call in (lambda e: bn.infer(target, e, N_max=N), lambda e: bn.engine.infer_raw(target, e, N),
                 lambda e: bn.engine.predict(target, e, N)):
        with pytest.raises(RuntimeError) as got:
            call(_t(bad, gpu))
        assert str(got.value) == str(want.value)
    for e in (narrow, ev):  # the [Q, 1] call and the wide call still match the oracle
        raw, out = _raw(bn, target, _t(e, gpu), N)
        rstar = int(np.argmax(raw.max(1)))
        _against_oracle(ora, target, e, _sub(33, rstar), out, raw, N)
