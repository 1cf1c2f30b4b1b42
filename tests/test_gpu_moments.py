"""``posterior`` / ``expect`` (per-query normalised marginal and its moments)
on the GPU.

Every case goes through ``check_case``:

(i)   exactly: ``pdf == rows / mass[:, None]`` computed in torch, bit for bit
      outside NaN and with equal NaN positions, where ``rows`` are the same
      plan's ``engine.infer_raw`` rows; ``|pdf.sum(1) - 1| <= 2 N u`` on rows
      of positive mass; ``expect``'s mass / mean / var equal ``posterior``'s
      bit for bit.  Plans with no raw launch (generic table plans, redrawn
      domains) are compared with the float64 normalisation of ``infer``'s rows
      at ``(N + 4) u`` relative (one rounding in each of infer's and the
      posterior's quotient, ``(N - 1) u`` in the mass, first order; the rest is
      slack for the higher-order terms);
(ii)  own rows: ``moments_ref.assert_moments`` against ``infer_raw``'s rows
      (summation error only), where the plan has them;
(iii) against the CPU oracle's rows (<= 257 rows; <= 64 at N = 64).

``cbn_plan_flags`` tells which kernel served each case: CBN_PLAN_MOMENTS is
asserted set for the plans whose query kernel reduces the row itself and clear
for the ``k_row_moments`` fallbacks.  The networks are those of
tests/test_gpu_predict.py.
"""
import ctypes
import random

import numpy as np
import pandas as pd
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from helpers import chain_data, grid_data, make_bn, sample_evidence, special_batch
from moments_ref import MIN_SHARE, U, assert_moments, mean_tolerance, moments_f64
from oracle.ref_infer import OracleBN
from test_gpu_predict import _fallback_case, _flags, _t

pytestmark = pytest.mark.gpu

FAST, LDS, STAGED = _native.CBN_PLAN_FAST, _native.CBN_PLAN_LDS, _native.CBN_PLAN_STAGED
DIRECT, COLS, SLOTS = _native.CBN_PLAN_DIRECT, _native.CBN_PLAN_COLS, _native.CBN_PLAN_SLOTS
MOMENTS = _native.CBN_PLAN_MOMENTS


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Equal NaN positions, equal bits elsewhere."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def check_case(bn, target, evt, N, seed=None, min_share=MIN_SHARE):
    """Checks (i) and (ii) of the module docstring.  ``evt``: device evidence
    columns; ``seed``: Python's ``random`` before each call (redrawn domains);
    ``min_share``: check (ii)'s refusal threshold (lifted where the test says why).
    Returns numpy (pdf, mass, mean, var, domain) and whether the plan had raw
    rows to compare with."""
    eng = bn.engine
    random.seed(seed)
    pdf, dom = bn.posterior(target, evt, N_max=N)
    random.seed(seed)
    pdf2, mass, mean, var = eng.posterior(target, evt, N)
    assert all(t.dtype == torch.float32 for t in (pdf, mass, mean, var))
    Q = mass.shape[0]
    assert pdf.shape == (Q, N) and mean.shape == var.shape == (Q,) and dom.shape[-1] == N
    assert same_bits(pdf, pdf2)
    random.seed(seed)
    emean, evar, emass = bn.expect(target, evt, N_max=N, moments=True)
    assert same_bits(emass, mass) and same_bits(emean, mean) and same_bits(evar, var)
    random.seed(seed)
    assert same_bits(bn.expect(target, evt, N_max=N), mean)
    random.seed(seed)
    res = eng.infer_raw(target, evt, N)
    points = dom.reshape(-1, N)[0].cpu().numpy()
    if res is not None:
        rows = res[0]
        assert same_bits(pdf, rows / mass[:, None])
        assert_moments(mass.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), rows.cpu().numpy(), points,
                       own=True, min_share=min_share)
    else:
        random.seed(seed)
        rows, _ = bn.infer(target, evt, N_max=N)
        r64 = rows.double()
        ref = r64 / r64.sum(1, keepdim=True)
        ok = mass > 0
        assert ok.float().mean() >= 0.9
        err = (pdf.double() - ref).abs()[ok]
        assert (err <= (N + 4) * U * ref[ok]).all(), float((err / ref[ok].clamp_min(1e-300)).max())
    pos = mass > 0
    assert ((pdf.double().sum(1) - 1).abs()[pos] <= 2 * N * U).all()
    assert torch.isnan(pdf[mass == 0]).all()
    return (pdf.cpu().numpy(), mass.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), dom.cpu().numpy(),
            res is not None)


def check_oracle(out, ora, target, ev, N, seed=None, rows=None):
    """Check (iii) on the rows ``rows`` (default: all)."""
    sub = slice(None) if rows is None else rows
    random.seed(seed)
    with np.errstate(all="ignore"):
        raw, dom = ora.infer_raw(target, {k: v[sub] for k, v in ev.items()}, N)
    np.testing.assert_array_equal(out[4].reshape(-1, N)[0], dom.reshape(-1, N)[0])
    return assert_moments(out[1][sub], out[2][sub], out[3][sub], raw, dom, own=False)


# ------------------------------------------------------------------ staged --
@pytest.fixture(scope="module")
def staged(gpu):
    """The 6-node d = 32 chain (k_query_staged) and the oracle's rows of its 257-row batch."""
    data, cols, edges = chain_data(6, 32, 60000, 8, stay=0.8)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    names = [c for c in cols if c != "X5"]
    ev = sample_evidence(data, cols, names, 257, 40)
    ora = OracleBN(edges, cols, data)
    raw, dom = ora.infer_raw("X5", ev, 32)
    raw.setflags(write=False)
    return dict(bn=bn, data=data, cols=cols, edges=edges, names=names, ev=ev, ora=ora, raw=raw, dom=dom)


@pytest.mark.parametrize("Q", [1, 3, 15, 16, 17, 255, 256, 257, 4097])
def test_staged_chain(Q, staged, gpu):
    s = staged
    bn = s["bn"]
    ev = sample_evidence(s["data"], s["cols"], s["names"], Q, 40)  # (a prefix property: the same rows as the 257 batch)
    out = check_case(bn, "X5", _t(ev, gpu), 32)
    assert out[5]
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | STAGED | MOMENTS) == FAST | STAGED | MOMENTS, f
    n = min(Q, 257)
    sub = {k: v[:n] for k, v in ev.items()}
    raw = s["raw"][:n] if all(np.array_equal(sub[k], s["ev"][k][:n]) for k in sub) else s["ora"].infer_raw("X5", sub, 32)[0]
    assert_moments(out[1][:n], out[2][:n], out[3][:n], raw, s["dom"], own=False)


def test_staged_chain_more_than_one_round_per_block(staged, gpu):
    """131 073 queries: beyond one round per block of the raw-style grid, so the
    double-buffered evidence staging runs, with a single query in the last
    round.  Checks (i) and (ii)."""
    s = staged
    ev = sample_evidence(s["data"], s["cols"], s["names"], 131073, 41)
    out = check_case(s["bn"], "X5", _t(ev, gpu), 32)
    assert out[5] and (out[1] > 0).all()


# -------------------------------------------------------------- lane sweep --
@pytest.mark.parametrize("N", [4, 8, 12, 16, 20, 24, 64])
def test_lane_count_sweep(N, gpu):
    """Short chains over N levels, 65 queries (a ragged last wave): N / 4 or
    N / 8 lanes per query where that divides 64 (k_query_cols; k_query_fast at
    N = 64); N = 12, 20, 24 run the generic kernel and the row fallback."""
    data, cols, edges = chain_data(5, N, 30000, 20 + N, stay=0.8)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    Q = 65 if N < 64 else 64
    ev = sample_evidence(data, cols, cols[:-1], Q, 9)
    out = check_case(bn, cols[-1], _t(ev, gpu), N)
    f = _flags(bn)
    assert len(f) == 1
    if N in (12, 20, 24):
        assert not f[0] & (FAST | MOMENTS) and not out[5], f
    elif N == 64:
        assert f[0] & (FAST | LDS | MOMENTS) == FAST | LDS | MOMENTS and not f[0] & (COLS | SLOTS | STAGED), f
    else:
        assert f[0] & (FAST | COLS | MOMENTS) == FAST | COLS | MOMENTS, f
    assert check_oracle(out, OracleBN(edges, cols, data), cols[-1], ev, N) == 1.0


# ------------------------------------------------------------------- slots --
def test_slots_plan(gpu):
    """The 100-node construction of tests/test_gpu_predict.py (k_query_slots:
    100 factors, global tables, 4 lanes per query), 3 000 queries: checks (i)
    and (ii) on every row.  Its masses are around 1e-33, below the helper's
    1e-30, so (ii) compares the masses alone here (its refusal is lifted:
    ``min_share=0``) and the oracle comparison would be refused: means,
    variances and the oracle are checked on
    ``test_slots_plan_against_the_oracle``'s network."""
    rng = np.random.default_rng(17)
    S, d, n = 20000, 32, 100
    pm = np.full(d, 0.03 / 30)
    pm[0] = pm[1] = 0.485
    X = np.zeros((S, n), np.int64)
    X[:, 0] = rng.choice(d, S, p=pm)
    for i in range(1, n):
        src = (X[:, i - 1] + X[:, i - 2]) % d if i in (12, 22, 32) else X[:, i - 1]
        draw = rng.choice(d, S, p=pm)
        X[:, i] = np.where(rng.random(S) < 0.04, src, draw)
    data = X.astype(np.float32)
    cols = [f"X{i}" for i in range(n)]
    edges = [(cols[i - 1], cols[i]) for i in range(1, n)] + [(cols[i - 2], cols[i]) for i in (12, 22, 32)]
    ev = sample_evidence(data, cols, ["X10", "X11", "X20", "X21", "X30", "X31", "X98"], 3000, 4)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    out = check_case(bn, "X99", _t(ev, gpu), 32, min_share=0.0)
    assert out[5] and (out[1] > 0).mean() > 0.9  # (some sampled rows have no support)
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | SLOTS | MOMENTS) == FAST | SLOTS | MOMENTS and not f[0] & LDS, f


def test_slots_plan_against_the_oracle(gpu):
    """k_query_slots at 8 lanes per query (3 x 3 grid, d = 64, peaked CPDs;
    3 % of the compared rows are all zero, the others have mass >= 1e-30)."""
    data, cols, edges = grid_data(100000, 7, side=3, d=64, keep=0.995, noise=0)
    ev = sample_evidence(data, cols, cols[:-1], 1001, 5)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    out = check_case(bn, "X8", _t(ev, gpu), 64)
    assert out[5]
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | SLOTS | MOMENTS) == FAST | SLOTS | MOMENTS and not f[0] & LDS, f
    assert check_oracle(out, OracleBN(edges, cols, data), "X8", ev, 64, rows=np.arange(0, 1001, 24)) >= 0.9


# --------------------------------------------------------------- fallbacks --
@pytest.mark.parametrize("name", ["generic5", "generic7", "forced_direct", "hashed", "wide", "linear_regression",
                                  "neural_network16"])
def test_fallback_plans(name, gpu, tmp_path):
    """Plans without the epilogue: their stored rows through k_row_moments
    (N = 5, 7: its scalar path).  Q = 300 and Q = 1."""
    bn, ora, target, ev, N, want, forbid, seed = _fallback_case(name, gpu, tmp_path)
    forbid = (forbid & ~_native.CBN_PLAN_ARGMAX) | (MOMENTS if forbid & _native.CBN_PLAN_ARGMAX else 0)
    if name == "hashed":
        # the 16 points drawn of X3's ~25 values leave 44 % of the sampled rows without support (mass 0): the
        # batch is the rows of oracle mass >= 1e-30 and eight of the others, so that the helper's 90 % rule holds
        random.seed(seed)
        m = ora.infer_raw(target, ev, N)[0].sum(1)
        keep = np.sort(np.concatenate([np.flatnonzero(m >= 1e-30), np.flatnonzero(m < 1e-30)[:8]]))
        assert keep.size >= 150 and (m[keep] == 0).sum() == 8
        ev = {k: v[keep] for k, v in ev.items()}
    out = check_case(bn, target, _t(ev, gpu), N, seed)
    f = _flags(bn)
    assert all(x & want == want and not x & forbid for x in f), f
    if name == "wide":  # the [Q, N] column runs on the wide direct plan
        wf = [int(_native.load().cbn_plan_flags(wp.handle)) for _, wp in bn.engine._wide_plans.values()]
        assert len(wf) == 1 and wf[0] & DIRECT and not wf[0] & MOMENTS, wf
    check_oracle(out, ora, target, ev, N, seed, rows=slice(0, 257))
    i = int(np.argmax(out[1] > 0))  # the first row with support, alone
    one = {k: v[i:i + 1] for k, v in ev.items()}
    out1 = check_case(bn, target, _t(one, gpu), N, seed)
    for a, b in zip(out1[:4], out[:4]):
        np.testing.assert_array_equal(a, b[i:i + 1])


@pytest.mark.parametrize("n_cols", [1, 4, 5, 7, 12, 20, 24, 32, 260, 1024])
@pytest.mark.parametrize("normalize", [0, 1])
def test_row_moments_kernel(n_cols, normalize, gpu):
    """cbn_row_moments on stored rows of every lane split (one lane per row;
    1 .. 64 lanes; 260 and 1 024 columns: more than one piece per lane), 1 001
    rows, some of mass 0: check (ii), the in-place division, and that a row's
    outputs do not depend on its position."""
    rng = np.random.default_rng(n_cols)
    raw = (rng.random((1001, n_cols)) ** 4 * 1e-9).astype(np.float32)
    raw[rng.random(raw.shape) < (0.3 if n_cols >= 8 else 0.02)] = 0
    raw[5] = raw[700] = 0
    raw[1000] = raw[0]
    s = np.sort(rng.normal(50, 20, n_cols)).astype(np.float32)
    rows, tv = torch.tensor(raw, device=gpu), torch.tensor(s, device=gpu)
    mass, mean, var = (torch.empty(1001, device=gpu) for _ in range(3))
    with torch.cuda.device(gpu):
        _native.check(_native.load().cbn_row_moments(_native.ptr(rows), 1001, n_cols, _native.ptr(tv), normalize,
                                                     _native.ptr(mass), _native.ptr(mean), _native.ptr(var),
                                                     _native.stream_ptr(gpu)), "cbn_row_moments")
    assert_moments(mass.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), raw, s, own=True)
    ref = torch.tensor(raw, device=gpu)
    assert same_bits(rows, ref / mass[:, None] if normalize else ref)
    for t in (mass, mean, var):
        assert same_bits(t[1000:], t[:1])
    # mass alone (no sample points)
    m2 = torch.empty(1001, device=gpu)
    with torch.cuda.device(gpu):
        _native.check(_native.load().cbn_row_moments(_native.ptr(ref), 1001, n_cols, None, 0, _native.ptr(m2), None, None,
                                                     _native.stream_ptr(gpu)), "cbn_row_moments")
    assert same_bits(m2, mass)
    assert _native.load().cbn_row_moments(_native.ptr(ref), 1001, n_cols, None, 0, _native.ptr(m2), _native.ptr(mean),
                                          None, _native.stream_ptr(gpu)) == _native.CBN_E_ARG


# ------------------------------------------------------------ independence --
def _independence(bn, data, cols, names, target, N, gpu):
    base = sample_evidence(data, cols, names, 1, 123)
    got, masses = [], []
    for Q in (1, 257, 4097):
        ev = sample_evidence(data, cols, names, Q, 77 + Q)
        pos = sorted({p for p in (0, 1, 127, 128, Q - 1) if p < Q})
        for k in names:
            ev[k][pos, 0] = base[k][0, 0]
        pdf, mass, mean, var = bn.engine.posterior(target, _t(ev, gpu), N)
        _, mass2, mean2, var2 = bn.engine.posterior(target, _t(ev, gpu), N, rows=False)
        masses += [float(mass[p]) for p in pos]
        for p in pos:
            got.append(torch.cat([bits(pdf[p]), bits(mass[p:p + 1]), bits(mean[p:p + 1]), bits(var[p:p + 1])]))
            got.append(torch.cat([bits(pdf[p]), bits(mass2[p:p + 1]), bits(mean2[p:p + 1]), bits(var2[p:p + 1])]))
    assert len(got) == 2 * (1 + 5 + 5)
    assert min(masses) > 0
    for g in got[1:]:
        assert torch.equal(g, got[0])


def test_a_row_does_not_depend_on_its_batch_staged(staged, gpu):
    """Positions 0 / 128 are even query slots of the N = 32 layout, 1 / 127 odd
    ones (the lane's two column blocks swap)."""
    s = staged
    _independence(s["bn"], s["data"], s["cols"], s["names"], "X5", 32, gpu)


@pytest.mark.parametrize("N", [16, 20, 64])
def test_a_row_does_not_depend_on_its_batch(N, gpu):
    """k_query_cols (two lanes per query), the generic fallback, k_query_fast (eight lanes)."""
    data, cols, edges = chain_data(5, N, 30000, 20 + N, stay=0.8)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    _independence(bn, data, cols, cols[:-1], cols[-1], N, gpu)


# ---------------------------------------------------------- special values --
def test_special_evidence_on_the_staged_chain(staged, gpu):
    s = staged
    bn, names = s["bn"], s["names"]
    Q = 4 * len(names) * 20 + 21
    doms = {c: np.unique(s["data"][:, s["cols"].index(c)]) for c in names}
    clean = sample_evidence(s["data"], s["cols"], names, Q, 5)
    ev, rows = special_batch(clean, doms)
    out = check_case(bn, "X5", _t(ev, gpu), 32, min_share=0.0)  # (about half of the rows are off-domain: mass 0)
    ref = check_case(bn, "X5", _t(clean, gpu), 32)
    off = np.array([r[0] for r in rows if not r[4]])
    assert off.size >= 17 * len(names)
    # off-domain, NaN, +-inf: an all-zero row -> mass 0, everything else NaN (0 / 0)
    assert (out[1][off] == 0).all() and np.isnan(out[0][off]).all() and np.isnan(out[2][off]).all() \
        and np.isnan(out[3][off]).all()
    for c in names:  # -0.0 equals +0.0 (same base row)
        r_neg, r_pos = (next(r[0] for r in rows if r[1] == c and r[2] == k) for k in (4, 5))
        assert np.signbit(ev[c][r_neg, 0]) and out[1][r_neg] == out[1][r_pos] > 0
        for a in out[:4]:
            np.testing.assert_array_equal(a[r_neg], a[r_pos])
    untouched = np.ones(Q, bool)
    untouched[[r[0] for r in rows]] = False
    assert (ref[1] > 0).all()
    for a, b in zip(out[:4], ref[:4]):
        np.testing.assert_array_equal(a[untouched], b[untouched])
    sub = np.arange(1, min(Q, 257), 2)  # (the odd rows hold the special values: mostly mass 0, compared exactly)
    with np.errstate(all="ignore"):
        raw, dom = s["ora"].infer_raw("X5", {k: v[sub] for k, v in ev.items()}, 32)
    assert_moments(out[1][sub], out[2][sub], out[3][sub], raw, dom, own=False, min_share=0.0)


def test_nan_parent_value_on_the_linear_regression_network(gpu, tmp_path):
    """A NaN parent value: that row is NaN throughout; no other row changes
    (there is no batch maximum to spread it)."""
    bn, ora, target, ev, N, _, _, seed = _fallback_case("linear_regression", gpu, tmp_path)
    bad = {k: v.copy() for k, v in ev.items()}
    parent = sorted(p for p, c in bn.initial_dag.edges if c == target)[0]
    bad[parent][7, 0] = np.nan
    random.seed(seed)
    out = [t.cpu().numpy() for t in bn.engine.posterior(target, _t(bad, gpu), N)]
    ref = check_case(bn, target, _t(ev, gpu), N, seed)
    assert np.isnan(out[1][7]) and np.isnan(out[2][7]) and np.isnan(out[3][7]) and np.isnan(out[0][7]).all()
    keep = np.arange(300) != 7
    assert not np.isnan(out[1][keep]).any()
    for a, b in zip(out[:4], ref[:4]):
        np.testing.assert_array_equal(a[keep], b[keep])
    random.seed(seed)
    e = [t.cpu().numpy() for t in bn.expect(target, _t(bad, gpu), N_max=N, moments=True)]
    np.testing.assert_array_equal(e[0], out[2])
    np.testing.assert_array_equal(e[1], out[3])
    np.testing.assert_array_equal(e[2], out[1])


# ---------------------------------------------------------- redrawn domain --
@pytest.mark.parametrize("force_direct", [False, True])
def test_redrawn_domain(force_direct, gpu):
    """N_max = 7 above the cardinality 4: the sample domains are drawn per
    call; ``mean`` and ``var`` use THIS call's draw."""
    data, cols, edges = chain_data(6, 4, 4000, 21)
    ora = OracleBN(edges, cols, data)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    bn.engine.force_direct = force_direct
    ev = sample_evidence(data, cols, ["X4", "X2"], 200, 6)
    doms, means = [], []
    for seed in (1, 2, 3, 2):
        out = check_case(bn, "X5", _t(ev, gpu), 7, seed)
        check_oracle(out, ora, "X5", ev, 7, seed)
        doms.append(out[4].copy())
        means.append(out[2].copy())
    assert not np.array_equal(doms[0], doms[1]) and np.array_equal(doms[1], doms[3])
    np.testing.assert_array_equal(means[1], means[3])  # (NaN on the rows without support, in both)
    assert len(bn.engine._plans) == 1
    f = _flags(bn)
    assert not force_direct or (f[0] & DIRECT and not f[0] & MOMENTS), f


# ------------------------------------------------------------------ errors --
def test_errors_are_infers_and_precede_any_launch(gpu):
    data, cols, edges = chain_data(6, 4, 4000, 5, stay=0.8)
    ev = sample_evidence(data, cols, ["X4", "X2"], 300, 3)
    two = dict(ev, X4=np.concatenate([ev["X4"], ev["X4"]], 1))
    short = dict(ev, X2=ev["X2"][:299])
    for bad in (two, short, None):
        got = []
        for fn in ("infer", "posterior", "expect"):
            bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
            with pytest.raises((RuntimeError, AssertionError, AttributeError)) as info:
                getattr(bn, fn)("X5", None if bad is None else _t(bad, gpu), N_max=4)
            got.append((type(info.value), str(info.value)))
            assert all(not p.tables_built for p in bn.engine._plans.values())  # nothing was launched
        assert got[0] == got[1] == got[2], got
    # ... and on a cached plan (the native host path declines, the general path raises)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    bn.engine.posterior("X5", _t(ev, gpu), 4)
    with pytest.raises(RuntimeError, match="expanded size"):
        bn.engine.posterior("X5", _t(two, gpu), 4)
    # conversions: float64 columns on the host give the float32 device result
    for rows in (True, False):
        a = bn.engine.posterior("X5", _t(ev, gpu), 4, rows=rows)
        b = bn.engine.posterior("X5", {k: torch.tensor(v, dtype=torch.float64) for k, v in ev.items()}, 4, rows=rows)
        assert (a[0] is None) == (not rows) and (b[0] is None) == (not rows)
        for x, y in zip(a[1 - rows:], b[1 - rows:]):
            assert torch.equal(x, y)
    # the C entry point: mean / var without the sample points, no output, no queries (all refused before a launch)
    lib, plan = _native.load(), next(iter(bn.engine._plans.values()))
    m = torch.empty(4, device=gpu)
    col = torch.zeros(4, 1, device=gpu)
    ptrs = (ctypes.c_void_p * 2)(col.data_ptr(), col.data_ptr())
    E = _native.CBN_E_ARG
    assert lib.cbn_plan_run_moments(plan.handle, 4, ptrs, 2, None, None, _native.ptr(m), _native.ptr(m), None, None, 0, None) == E
    assert lib.cbn_plan_run_moments(plan.handle, 4, ptrs, 2, None, None, None, None, None, None, 0, None) == E
    assert lib.cbn_plan_run_moments(plan.handle, 0, ptrs, 2, None, None, _native.ptr(m), None, None, None, 0, None) == E


def test_no_evidence_rows(gpu):
    """n_queries = 1 without evidence rows (evidence = {}): one posterior."""
    data, cols, edges = chain_data(5, 4, 3000, 3)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    pdf, mass, mean, var = bn.engine.posterior("X4", {}, 4)
    assert pdf.shape == (1, 4) and mass.shape == (1,)
    raw, dom = OracleBN(edges, cols, data).infer_raw("X4", None, 4)
    assert_moments(mass.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy(), raw, dom, own=False)
    np.testing.assert_allclose(pdf.cpu().numpy(), moments_f64(raw, dom)[3], rtol=3e-5)
    p2, d2 = bn.posterior("X4", {}, N_max=4)
    assert torch.equal(p2, pdf) and d2.shape == (1, 4)
    assert torch.equal(bn.expect("X4", {}, N_max=4), mean)


# --------------------------------------------------------------- expect_df --
def test_expect_df_equals_per_batch_expect(gpu):
    data, cols, edges = chain_data(5, 16, 20000, 14, stay=0.8)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    df = pd.DataFrame(data[:300], columns=cols)  # batch 128: two full batches and one of 44
    got = bn.expect_df(df, "X4", batch_size=128, N_max=16)
    assert isinstance(got, np.ndarray) and got.shape == (300,) and got.dtype == np.float64
    ref = []
    for n in range(0, 300, 128):
        ev = {c: torch.tensor(data[n:min(n + 128, 300), [i]], device=gpu) for i, c in enumerate(cols) if c != "X4"}
        ref.append(bn.expect("X4", ev, N_max=16).cpu().numpy())
    np.testing.assert_array_equal(got, np.concatenate(ref).astype(np.float64))
    assert np.isfinite(got).all()
    assert bn.expect_df(df[:0], "X4").shape == (0,)


# ---------------------------------------------------------- point-mass row --
@pytest.mark.parametrize("d", [8, 32])
def test_point_mass_rows(d, gpu):
    """X0 -> X1 -> X2 with X_i = X_{i-1} always: the row of X1 = a has one
    nonzero column, a (k_query_cols at d = 8, k_query_staged at d = 32, where a
    runs over every lane and both column blocks).  The mean is that sample
    point to tm and the variance at most tm^2."""
    data, cols, edges = chain_data(3, d, 4000, 2, stay=1.0)
    data = data + np.float32(100.0)  # sample points 100 .. 100 + d - 1: a mean error would show in the variance
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    a = np.tile(np.arange(d, dtype=np.float32) + 100, 3)[:, None]
    ev = {"X0": a.copy(), "X1": a.copy()}
    pdf, mass, mean, var, dom, _ = check_case(bn, "X2", _t(ev, gpu), d)
    assert MOMENTS & _flags(bn)[0]
    assert ((pdf > 0).sum(1) == 1).all() and (pdf.argmax(1) == a[:, 0] - 100).all()
    onehot = (np.arange(d)[None, :] == (a - 100)).astype(np.float64)
    tm = mean_tolerance(onehot, dom, own=True)
    assert (np.abs(mean.astype(np.float64) - a[:, 0]) <= tm).all() and (var >= 0).all() and (var <= tm ** 2).all()


# ----------------------------------------------------------------- timeout --
def test_pending_timeout_is_reported_once(staged, gpu):
    s = staged
    bn = s["bn"]
    evt = _t(s["ev"], gpu)
    a = bn.engine.posterior("X5", evt, 32)
    plan = next(iter(bn.engine._plans.values()))
    _native.check(_native.load().cbn_debug_flag_timeout(plan.handle), "flag")
    with pytest.raises(_native.NativeError, match="timed out"):
        bn.engine.posterior("X5", evt, 32)
    b = bn.engine.posterior("X5", evt, 32)  # reported once, then cleared
    for x, y in zip(a, b):
        assert torch.equal(x, y)
