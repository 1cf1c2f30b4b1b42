"""``predict`` (per-query arg-max of the marginal) on the GPU.

Every case is checked two ways:

(i)  exactly, against the parent's kernels: ``index == torch.argmax(rows, 1)``
     and ``row_max == rows.max(1).values`` bit for bit on EVERY row, where
     ``rows`` are the same plan's ``engine.infer_raw`` rows.  Plans without a
     raw launch (generic table plans, redrawn domains) are compared with
     ``infer``'s rows instead, on decided rows (tests/predict_ref.py);
(ii) against the CPU oracle through ``predict_ref.assert_predictions``
     (<= 257 rows; <= 64 at N = 64, where the oracle is slow).

``cbn_plan_flags`` tells which kernel served each case: CBN_PLAN_ARGMAX is
asserted set for the plans whose query kernel reduces the row itself and clear
for the ``k_row_argmax`` fallbacks.  Inputs other than the three chains that
tests/test_predict_host.py checks were checked on the CPU to have >= 90 %
decided rows (assert_predictions refuses less).
"""
import json
import os
import random

import numpy as np
import pandas as pd
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from golden_io import load_param_golden, oracle_estimators
from helpers import chain_data, continuous_data, make_bn, param_config, sample_evidence, special_batch
from oracle.ref_infer import OracleBN
from parity import n_factors, peak
from predict_ref import assert_predictions, check_exact, decided, raw_argmax
from test_gpu_param import load_fixture_params

pytestmark = pytest.mark.gpu

FAST, LDS, PAIRED, STAGED = _native.CBN_PLAN_FAST, _native.CBN_PLAN_LDS, _native.CBN_PLAN_PAIRED, _native.CBN_PLAN_STAGED
DIRECT, COLS, SLOTS, PARAM = (_native.CBN_PLAN_DIRECT, _native.CBN_PLAN_COLS, _native.CBN_PLAN_SLOTS,
                              _native.CBN_PLAN_PARAMETRIC)
ARGMAX = _native.CBN_PLAN_ARGMAX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_chain.npz")


def _t(ev, dev):
    return {k: torch.tensor(v, device=dev) for k, v in ev.items()}


def _flags(bn):
    lib = _native.load()
    return [int(lib.cbn_plan_flags(p.handle)) for p in bn.engine._plans.values()]


def check_oracle(out, ora, target, ev, N, seed=None):
    """Check (ii)."""
    random.seed(seed)
    with np.errstate(all="ignore"):
        raw, dom = ora.infer_raw(target, ev, N)
    return assert_predictions(out[0], out[1], out[2], raw, dom, n_factors=n_factors(ora, target),
                              peak=peak(ora, target))


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
    out = check_exact(bn, "X5", _t(ev, gpu), 32)
    assert out[3]
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | STAGED | ARGMAX) == FAST | STAGED | ARGMAX, f
    n = min(Q, 257)
    sub = {k: v[:n] for k, v in ev.items()}
    raw = s["raw"][:n] if all(np.array_equal(sub[k], s["ev"][k][:n]) for k in sub) else s["ora"].infer_raw("X5", sub, 32)[0]
    assert_predictions(out[0][:n], out[1][:n], out[2][:n], raw, s["dom"], n_factors=6)


def test_staged_chain_more_than_one_round_per_block(staged, gpu):
    """131 073 queries: beyond one round per block of the raw-style grid, so the
    double-buffered evidence staging runs, with a single query in the last
    round.  Check (i) only."""
    s = staged
    ev = sample_evidence(s["data"], s["cols"], s["names"], 131073, 41)
    out = check_exact(s["bn"], "X5", _t(ev, gpu), 32)
    assert out[3] and len(np.unique(out[0])) == 32


# -------------------------------------------------------------------- ties --
TIES = {8: [(3, 4), (0, 7), (1, 2), (6, 7), (0, 4), (2, 5)],
        # N = 32, lane l of a quad holds columns 4 l .. 4 l + 3 and 16 + 4 l .. 16 + 4 l + 3 (which of the
        # two sits in the first registers depends on the query slot's parity): pairs that straddle two
        # lanes, the two blocks of one lane, and both at once
        32: [(3, 4), (2, 18), (15, 16), (7, 28), (0, 31), (17, 19)]}


def tie_data(N):
    """A -> T, both over N levels (N_max = N draws nothing): for A = a the two
    columns TIES[N][a % 6] have the same count (40, the row's maximum), every
    other column a smaller one."""
    rows = []
    for a in range(N):
        c1, c2 = TIES[N][a % 6]
        for t in range(N):
            cnt = 40 if t in (c1, c2) else 1 + (t * 7 + a * 3) % 23
            rows += [(a, t)] * cnt
    rng = np.random.default_rng(3)
    data = np.array(rows, np.float32)[rng.permutation(len(rows))]
    return data, ["A", "T"], [("A", "T")]


@pytest.mark.parametrize("N", [8, 32])
def test_ties_go_to_the_lowest_column(N, gpu):
    """Exact ties across register blocks, lanes and (N = 32) the clo / chi
    blocks of odd and even query slots.  The oracle check is replaced by the
    construction's own answer: tied rows are undecided by definition."""
    data, cols, edges = tie_data(N)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    rng = np.random.default_rng(5)
    a = rng.integers(0, N, (257, 1)).astype(np.float32)
    a[:12, 0] = np.repeat(np.arange(6), 2)  # every A in an even and an odd slot
    out = check_exact(bn, "T", _t({"A": a}, gpu), N)
    assert out[3]
    f = _flags(bn)
    want = FAST | STAGED | ARGMAX if N == 32 else FAST | COLS | ARGMAX
    assert len(f) == 1 and f[0] & want == want, f
    np.testing.assert_array_equal(out[0], [TIES[N][int(x) % 6][0] for x in a[:, 0]])
    raw, dom = OracleBN(edges, cols, data).infer_raw("T", {"A": a}, N)
    for q in range(257):
        c1, c2 = TIES[N][int(a[q, 0]) % 6]
        assert raw[q, c1] == raw[q, c2] == raw[q].max()
    np.testing.assert_array_equal(out[1], dom.reshape(-1, N)[0][out[0]])
    np.testing.assert_allclose(out[2], raw.max(1), rtol=1e-5)


# -------------------------------------------------------------- lane sweep --
@pytest.mark.parametrize("N", [4, 8, 12, 16, 20, 24, 64])
def test_lane_count_sweep(N, gpu):
    """Short chains over N levels, 65 queries (a ragged last wave).  The fast
    path takes N / 4 or N / 8 lanes per query only when that divides 64: N =
    12, 20, 24 (3, 5, 6 lanes) run the generic kernel and the row fallback."""
    data, cols, edges = chain_data(5, N, 30000, 20 + N, stay=0.8)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    Q = 65 if N < 64 else 64
    ev = sample_evidence(data, cols, cols[:-1], Q, 9)
    out = check_exact(bn, cols[-1], _t(ev, gpu), N)
    f = _flags(bn)
    assert len(f) == 1
    if N in (12, 20, 24):
        assert not f[0] & (FAST | ARGMAX) and not out[3], f
    elif N == 64:
        assert f[0] & (FAST | LDS | ARGMAX) == FAST | LDS | ARGMAX and not f[0] & (COLS | SLOTS | STAGED), f
    else:
        assert f[0] & (FAST | COLS | ARGMAX) == FAST | COLS | ARGMAX, f
    check_oracle(out, OracleBN(edges, cols, data), cols[-1], ev, N)


# ------------------------------------------------------------------- slots --
def test_slots_plan(gpu):
    """The 100-node construction of tests/test_gpu_api.py (k_query_slots: 100
    factors, global tables, 4 lanes per query), 3 000 queries.  Check (i) on
    every row.  The oracle (every 97th row) cannot decide this construction: by
    design each row has two near-equal maxima (levels 0 and 1, 0.485 each) and
    tops around 1e-34, below the rule's 1e-30 -- 0 of the 31 rows are decided --
    so the helper's refusal is lifted here (``min_decided=0``) and its other
    assertions hold on every row: the chosen column's oracle value is within
    1e-4 of the top, row_max within rtol 1e-5 + 100 subnormal steps,
    value == domain[index]."""
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
    names = ["X10", "X11", "X20", "X21", "X30", "X31", "X98"]
    ev = sample_evidence(data, cols, names, 3000, 4)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    out = check_exact(bn, "X99", _t(ev, gpu), 32)
    assert out[3]
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | SLOTS | ARGMAX) == FAST | SLOTS | ARGMAX and not f[0] & LDS, f
    sub = np.arange(0, 3000, 97)
    random.seed(0)
    ora = OracleBN(edges, cols, data)
    raw, dom = ora.infer_raw("X99", {k: v[sub] for k, v in ev.items()}, 32)
    assert not decided(raw).any()
    assert_predictions(out[0][sub], out[1][sub], out[2][sub], raw, dom, n_factors=100, min_decided=0.0)


def test_slots_plan_with_decided_rows(gpu):
    """k_query_slots at 8 lanes per query (3 x 3 grid, d = 64, peaked CPDs;
    checked on the CPU: every compared row decided, 3 % of them all zero), so
    the slots epilogue also meets the oracle under the helper's 90 % rule."""
    from helpers import grid_data

    data, cols, edges = grid_data(100000, 7, side=3, d=64, keep=0.995, noise=0)
    ev = sample_evidence(data, cols, cols[:-1], 1001, 5)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    out = check_exact(bn, "X8", _t(ev, gpu), 64)
    assert out[3]
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | SLOTS | ARGMAX) == FAST | SLOTS | ARGMAX and not f[0] & LDS, f
    sub = np.arange(0, 1001, 24)
    ora = OracleBN(edges, cols, data)
    raw, dom = ora.infer_raw("X8", {k: v[sub] for k, v in ev.items()}, 64)
    assert decided(raw).all()
    assert_predictions(out[0][sub], out[1][sub], out[2][sub], raw, dom, n_factors=n_factors(ora, "X8"))


# --------------------------------------------------------------- fallbacks --
def _multi_net(S=20000, seed=9, d=4):
    """A, B -> C; A -> D; C, D -> E over d levels (multi_widthN_partial's shape)."""
    rng = np.random.default_rng(seed)
    A, B = rng.integers(0, d, S), rng.integers(0, d, S)
    C = (A + B + rng.integers(0, 2, S)) % d
    D = (A + rng.choice(3, S, p=[0.7, 0.2, 0.1])) % d
    E = (C + D + rng.choice(3, S, p=[0.8, 0.15, 0.05])) % d
    data = np.stack([A, B, C, D, E], 1).astype(np.float32)
    return data, ["A", "B", "C", "D", "E"], [("A", "C"), ("B", "C"), ("C", "E"), ("D", "E"), ("A", "D")]


def _fallback_case(name, gpu, tmp_path):
    """(bn, oracle, target, evidence, N, flags wanted, flags forbidden, seed)"""
    if name in ("generic5", "generic7"):
        d = int(name[-1])
        data, cols, edges = chain_data(5, d, 8000, 11, stay=0.7)
        ev = sample_evidence(data, cols, cols[:-1], 300, 5)
        return make_bn(BayesianNetwork, edges, cols, data, device=gpu), OracleBN(edges, cols, data), cols[-1], ev, d, 0, \
            FAST | DIRECT | ARGMAX, None
    if name == "forced_direct":
        data, cols, edges = chain_data(5, 16, 20000, 14, stay=0.8)
        bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
        bn.engine.force_direct = True
        return bn, OracleBN(edges, cols, data), "X4", sample_evidence(data, cols, cols[:-1], 300, 5), 16, DIRECT, ARGMAX, None
    if name == "hashed":
        data, cols, edges = continuous_data(8000, 35)
        return make_bn(BayesianNetwork, edges, cols, data, device=gpu), OracleBN(edges, cols, data), "X3", \
            sample_evidence(data, cols, ["X0", "X1", "X2"], 300, 5), 16, DIRECT, ARGMAX, 7
    if name == "wide":
        data, cols, edges = _multi_net()
        rng = np.random.default_rng(31)  # each query's four values of C: one level, the first entry redrawn
        cw = np.repeat(rng.integers(0, 4, (300, 1)), 4, 1).astype(np.float32)
        cw[:, 0] = rng.integers(0, 4, 300)
        return make_bn(BayesianNetwork, edges, cols, data, device=gpu), OracleBN(edges, cols, data), "E", {"C": cw}, 4, 0, \
            0, None
    fixture = {"linear_regression": "lr_chain5_all", "neural_network16": "nn_multi_leakyrelu"}[name]
    g = load_param_golden(fixture)
    m = g["meta"]
    cfg = param_config(m["estimator"], n_epochs=1, model=m["model"] or None)
    bn = make_bn(BayesianNetwork, m["edges"], m["columns"], g["data"], device=gpu, estimator=m["estimator"], config=cfg)
    load_fixture_params(bn, g, tmp_path, gpu)
    ora = OracleBN(m["edges"], m["columns"], g["data"], estimators=oracle_estimators(g))
    ev = sample_evidence(g["data"], m["columns"], m["evidence"], 300, 77)
    return bn, ora, m["target"], ev, m["N_max"], PARAM, ARGMAX, m["seed"]


@pytest.mark.parametrize("name", ["generic5", "generic7", "forced_direct", "hashed", "wide", "linear_regression",
                                  "neural_network16"])
def test_fallback_plans(name, gpu, tmp_path):
    """Plans without the epilogue: their stored rows through k_row_argmax
    (N = 5, 7: its scalar path).  Q = 300 and Q = 1."""
    bn, ora, target, ev, N, want, forbid, seed = _fallback_case(name, gpu, tmp_path)
    out = check_exact(bn, target, _t(ev, gpu), N, seed)
    f = _flags(bn)
    assert all(x & want == want and not x & forbid for x in f), f
    if name == "wide":  # the [Q, N] column runs on the wide direct plan
        wf = [int(_native.load().cbn_plan_flags(wp.handle)) for _, wp in bn.engine._wide_plans.values()]
        assert len(wf) == 1 and wf[0] & DIRECT and not wf[0] & ARGMAX, wf
    check_oracle(out, ora, target, ev, N, seed)
    one = {k: v[:1] for k, v in ev.items()}
    out1 = check_exact(bn, target, _t(one, gpu), N, seed)
    np.testing.assert_array_equal(out1[0], out[0][:1])
    np.testing.assert_array_equal(out1[2], out[2][:1])


# ---------------------------------------------------------- special values --
def test_special_evidence_on_the_staged_chain(staged, gpu):
    s = staged
    bn, names = s["bn"], s["names"]
    Q = 4 * len(names) * 20 + 21
    doms = {c: np.unique(s["data"][:, s["cols"].index(c)]) for c in names}
    clean = sample_evidence(s["data"], s["cols"], names, Q, 5)
    ev, rows = special_batch(clean, doms)
    out = check_exact(bn, "X5", _t(ev, gpu), 32)
    ref = check_exact(bn, "X5", _t(clean, gpu), 32)
    off = np.array([r[0] for r in rows if not r[4]])
    assert off.size >= 17 * len(names)
    assert (out[0][off] == 0).all() and (out[2][off] == 0).all()  # off-domain, NaN, +-inf: an all-zero row
    for c in names:  # -0.0 equals +0.0 (same base row)
        r_neg, r_pos = (next(r[0] for r in rows if r[1] == c and r[2] == k) for k in (4, 5))
        assert np.signbit(ev[c][r_neg, 0]) and out[0][r_neg] == out[0][r_pos] and out[2][r_neg] == out[2][r_pos] > 0
    untouched = np.ones(Q, bool)
    untouched[[r[0] for r in rows]] = False
    for a, b in zip(out[:3], ref[:3]):
        np.testing.assert_array_equal(a[untouched], b[untouched])
    sub = np.arange(min(Q, 257))
    assert_predictions(out[0][sub], out[1][sub], out[2][sub], s["ora"].infer_raw("X5", {k: v[sub] for k, v in ev.items()}, 32)[0],
                       s["dom"], n_factors=6)


def test_nan_parent_value_on_the_linear_regression_network(gpu, tmp_path):
    """A NaN parent value: that row's first NaN column and a NaN row_max; no
    other row changes (there is no global max to spread it)."""
    bn, ora, target, ev, N, _, _, seed = _fallback_case("linear_regression", gpu, tmp_path)
    bad = {k: v.copy() for k, v in ev.items()}
    parent = sorted(p for p, c in bn.initial_dag.edges if c == target)[0]
    bad[parent][7, 0] = np.nan
    out = check_exact(bn, target, _t(bad, gpu), N, seed)
    ref = check_exact(bn, target, _t(ev, gpu), N, seed)
    random.seed(seed)
    with np.errstate(all="ignore"):
        raw, _ = ora.infer_raw(target, bad, N)
    assert np.isnan(raw[7]).any() and np.isnan(out[2][7])
    assert out[0][7] == raw_argmax(raw[7:8])[0] == int(np.flatnonzero(np.isnan(raw[7]))[0])
    keep = np.arange(300) != 7
    for a, b in zip(out[:3], ref[:3]):
        np.testing.assert_array_equal(a[keep], b[keep])


# ---------------------------------------------------------- redrawn domain --
@pytest.mark.parametrize("force_direct", [False, True])
def test_redrawn_domain(force_direct, gpu):
    """N_max = 7 above the cardinality 4: the sample domains are drawn per
    call; ``value`` comes from THIS call's draw."""
    data, cols, edges = chain_data(6, 4, 4000, 21)
    ora = OracleBN(edges, cols, data)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    bn.engine.force_direct = force_direct
    ev = sample_evidence(data, cols, ["X4", "X2"], 200, 6)
    doms = []
    for seed in (1, 2, 3, 2):
        random.seed(seed)
        raw, dom = ora.infer_raw("X5", ev, 7)
        random.seed(seed)
        index, value, row_max = bn.engine.predict("X5", _t(ev, gpu), 7)
        assert_predictions(index.cpu().numpy(), value.cpu().numpy(), row_max.cpu().numpy(), raw, dom, n_factors=6)
        doms.append(dom.copy())
    assert not np.array_equal(doms[0], doms[1]) and np.array_equal(doms[1], doms[3])
    assert len(bn.engine._plans) == 1


# ------------------------------------------------------------------ errors --
def test_errors_are_infers_and_precede_any_launch(gpu):
    data, cols, edges = chain_data(6, 4, 4000, 5, stay=0.8)
    ev = sample_evidence(data, cols, ["X4", "X2"], 300, 3)
    two = dict(ev, X4=np.concatenate([ev["X4"], ev["X4"]], 1))
    short = dict(ev, X2=ev["X2"][:299])
    for bad in (two, short, None):
        got = []
        for fn in ("infer", "predict"):
            bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
            with pytest.raises((RuntimeError, AssertionError, AttributeError)) as info:
                getattr(bn.engine, fn)("X5", None if bad is None else _t(bad, gpu), 4)
            got.append((type(info.value), str(info.value)))
            assert all(not p.tables_built for p in bn.engine._plans.values())  # nothing was launched
        assert got[0] == got[1], got
    # ... and on a cached plan (the native host path declines, the general path raises)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    bn.engine.predict("X5", _t(ev, gpu), 4)
    with pytest.raises(RuntimeError, match="expanded size"):
        bn.engine.predict("X5", _t(two, gpu), 4)
    # conversions: float64 columns on the host give the float32 device result
    a = bn.engine.predict("X5", _t(ev, gpu), 4)
    b = bn.engine.predict("X5", {k: torch.tensor(v, dtype=torch.float64) for k, v in ev.items()}, 4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_no_evidence_rows(gpu):
    """n_queries = 1 without evidence rows (evidence = {}): one prediction."""
    data, cols, edges = chain_data(5, 4, 3000, 3)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    index, value, row_max = bn.engine.predict("X4", {}, 4)
    raw, dom = OracleBN(edges, cols, data).infer_raw("X4", None, 4)
    assert_predictions(index.cpu().numpy(), value.cpu().numpy(), row_max.cpu().numpy(), raw, dom, n_factors=5)
    from continuousbayesiannetwork_amd.inference import VariableElimination

    v, i = VariableElimination({}, bn=bn).map_query("X4", {}, N_max=4)
    assert torch.equal(i, index) and torch.equal(v, value)


# -------------------------------------------------------------- predict_df --
def test_predict_df_equals_benchmarking_df_and_the_reference(gpu):
    g = np.load(GOLDEN)
    m = json.loads(str(g["meta"]))
    data, cols, edges = chain_data(m["n"], m["d"], m["S"], m["seed"], stay=m["stay"])
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    ora = OracleBN(edges, cols, data)
    # 1 000 rows, batch 128: seven full batches and one of 104
    df = pd.DataFrame(data[:1000], columns=cols)
    got = bn.predict_df(df, m["target"], batch_size=128, N_max=16)
    ref = bn.benchmarking_df(df, m["target"], batch_size=128)
    assert isinstance(got, np.ndarray) and got.shape == ref.shape == (1000,) and got.dtype == ref.dtype
    raw, _ = ora.infer_raw(m["target"], {c: data[:1000, [i]] for i, c in enumerate(cols) if c != m["target"]}, 16)
    dec = decided(raw)
    assert dec.mean() >= 0.9
    np.testing.assert_array_equal(got[dec], ref[dec])
    # the reference's own arg-max on the fixture's rows
    ev = {k: g["ev_" + k] for k in m["evidence"]}
    fdf = pd.DataFrame({**{k: v[:, 0] for k, v in ev.items()}, m["target"]: np.zeros(m["Q"], np.float32)})[cols]
    fgot = bn.predict_df(fdf, m["target"], batch_size=128, N_max=m["N_max"])
    fdec = decided(ora.infer_raw(m["target"], ev, m["N_max"])[0])
    assert fdec.mean() >= 0.9
    np.testing.assert_array_equal(fgot[fdec], g["value"][fdec].astype(np.float64))
    value, index = bn.predict(m["target"], _t(ev, gpu), N_max=m["N_max"], return_index=True)
    np.testing.assert_array_equal(index.cpu().numpy()[fdec], g["index"][fdec])
    np.testing.assert_array_equal(value.cpu().numpy(), fgot.astype(np.float32))


# ----------------------------------------------------------------- timeout --
def test_pending_timeout_is_reported_once(staged, gpu):
    s = staged
    bn = s["bn"]
    evt = _t(s["ev"], gpu)
    a = bn.engine.predict("X5", evt, 32)
    plan = next(iter(bn.engine._plans.values()))
    _native.check(_native.load().cbn_debug_flag_timeout(plan.handle), "flag")
    with pytest.raises(_native.NativeError, match="timed out"):
        bn.engine.predict("X5", evt, 32)
    b = bn.engine.predict("X5", evt, 32)  # reported once, then cleared
    for x, y in zip(a, b):
        assert torch.equal(x, y)
