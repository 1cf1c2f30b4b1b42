"""``quantile`` / ``interval`` / ``sample`` (per-query inverse cdf of the
marginal) on the GPU.

Every case goes through ``check_case``:

(i)   ``index`` against the SAME plan's ``engine.infer_raw`` rows with
      ``quantile_ref.assert_quantile`` at ``extra = 0`` -- or, where the plan has
      no raw launch (generic table plans, redrawn domains), against ``infer``'s
      rows at ``extra = 2 u`` (the quantile is scale-invariant) -- for the
      shared list [0, 0.025, 0.25, 0.5, 0.75, 0.975, 1] AND the per-row decided
      midpoints of the cdf steps (``quantile_ref.midpoint_probs``: they hit
      every column, which is what catches a scan in register order), in one
      comparison; the midpoints go in per-row [Q, <= 16] calls, so plans with
      the in-kernel scan serve them in the query kernel; their NaN fillers must
      come back as -1 / NaN;
(ii)  ``value == domain[index]`` bit for bit (NaN where index is -1); ``mass``
      within ``2 N u`` of the raw rows' float64 sum; ``index`` non-decreasing
      along the sorted list; the [P]-shared and the [Q, P]-broadcast call agree
      bit for bit; ``interval`` equals the two quantiles;
(iii) position invariance: the same rows in a shuffled order, and with one more
      row appended, give the same bits.

``cbn_plan_flags`` tells which kernel served each case: CBN_PLAN_QUANTILE is
asserted set for the plans whose query kernel scans the row itself and clear
for the ``k_row_quantile`` fallbacks.  The networks are those of
tests/test_gpu_predict.py.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from helpers import chain_data, grid_data, make_bn, sample_evidence, special_batch
from oracle.ref_infer import OracleBN
from quantile_ref import U, assert_quantile, midpoint_probs
from test_gpu_predict import _fallback_case, _flags, _t

pytestmark = pytest.mark.gpu

FAST, LDS, STAGED = _native.CBN_PLAN_FAST, _native.CBN_PLAN_LDS, _native.CBN_PLAN_STAGED
DIRECT, COLS, SLOTS = _native.CBN_PLAN_DIRECT, _native.CBN_PLAN_COLS, _native.CBN_PLAN_SLOTS
QUANTILE, PMAX = _native.CBN_PLAN_QUANTILE, _native.CBN_MAX_QUANTILES
FIXED = [0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Equal NaN positions, equal bits elsewhere."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def run_probs(bn, target, evt, N, probs, seed=None):
    """engine.quantile at probs [Q, P] (any P) in per-row calls of <= 16
    columns: (index, value) as numpy [Q, P]."""
    idx, val = [], []
    for c in range(0, probs.shape[1], PMAX):
        random.seed(seed)
        i, v, _ = bn.engine.quantile(target, evt, N, probs[:, c:c + PMAX].contiguous())
        idx.append(i)
        val.append(v)
    return torch.cat(idx, 1), torch.cat(val, 1)


def reference_rows(bn, target, evt, N, seed=None):
    """(rows float64 numpy, extra, own): the plan's own raw rows, else infer's."""
    random.seed(seed)
    res = bn.engine.infer_raw(target, evt, N)
    if res is not None:
        return res[0].double().cpu().numpy(), 0.0, True
    random.seed(seed)
    rows, _ = bn.infer(target, evt, N_max=N)
    return rows.double().cpu().numpy(), 2 * U, False


def check_case(bn, target, evt, N, seed=None, invariance=True):
    """Checks (i) - (iii) of the module docstring.  ``evt``: device evidence
    columns; ``seed``: Python's ``random`` before each call (redrawn domains).
    Returns numpy (index [Q, 7], value [Q, 7], mass [Q], domain points [N],
    reference rows, extra)."""
    eng = bn.engine
    random.seed(seed)
    index, value, mass = eng.quantile(target, evt, N, FIXED)
    Q = mass.shape[0]
    assert index.dtype == torch.int32 and value.dtype == mass.dtype == torch.float32
    assert index.shape == value.shape == (Q, len(FIXED))
    rows, extra, own = reference_rows(bn, target, evt, N, seed)
    assert rows.shape == (Q, N)
    random.seed(seed)
    _, dom = bn.infer(target, evt, N_max=N)
    points = dom.reshape(-1, N)[0]
    # (i)
    dev = index.device
    mp = midpoint_probs(rows, extra)
    mi, mv = run_probs(bn, target, evt, N, torch.tensor(mp, device=dev), seed)
    all_idx, all_val = torch.cat([index, mi], 1), torch.cat([value, mv], 1)
    probs = np.concatenate([np.broadcast_to(np.float32(FIXED), (Q, len(FIXED))), mp], 1)
    assert_quantile(all_idx.cpu().numpy(), rows, probs, extra)
    # (ii)
    want = torch.where(all_idx >= 0, points[all_idx.clamp_min(0).long()], torch.full_like(all_val, float("nan")))
    assert same_bits(all_val, want)
    m64 = rows.sum(1)
    if own:
        assert (np.abs(mass.double().cpu().numpy() - m64) <= 2 * N * U * m64).all()
    pos = torch.tensor(m64 > 0, device=dev)
    assert (index[pos][:, 1:] >= index[pos][:, :-1]).all() and (index[~pos] == -1).all()
    random.seed(seed)
    bi, bv, bm = eng.quantile(target, evt, N, torch.tensor(FIXED, device=dev).expand(Q, -1).contiguous())
    assert torch.equal(bi, index) and same_bits(bv, value) and same_bits(bm, mass)
    random.seed(seed)
    v2, i2 = bn.quantile(target, evt, probs=FIXED, N_max=N, return_index=True)
    assert torch.equal(i2, index) and same_bits(v2, value)
    random.seed(seed)
    lo, hi = bn.interval(target, evt, level=0.95, N_max=N)
    assert same_bits(lo, value[:, 1]) and same_bits(hi, value[:, 5])
    # (iii)
    if invariance and Q >= 1 and all(v.shape[0] == Q for v in evt.values()):
        perm = torch.randperm(Q, generator=torch.Generator().manual_seed(Q)).to(dev)
        random.seed(seed)
        pi, pv, pm = eng.quantile(target, {k: v[perm].contiguous() for k, v in evt.items()}, N, FIXED)
        assert torch.equal(pi, index[perm]) and same_bits(pv, value[perm]) and same_bits(pm, mass[perm])
        random.seed(seed)
        more = {k: torch.cat([v, v[:1]]) for k, v in evt.items()}
        ai, av, am = eng.quantile(target, more, N, FIXED)
        assert torch.equal(ai[:Q], index) and same_bits(av[:Q], value) and same_bits(am[:Q], mass)
        assert torch.equal(ai[Q], index[0]) and same_bits(am[Q:], mass[:1])
    return index.cpu().numpy(), value.cpu().numpy(), mass.cpu().numpy(), points.cpu().numpy(), rows, extra


def check_oracle(out, ora, target, ev, N, seed=None, rows=None):
    """``index`` of the shared list against the CPU oracle's rows (``extra =
    1e-5``) on the rows ``rows`` (default: all); refused like any comparison
    that decides too little."""
    sub = slice(None) if rows is None else rows
    random.seed(seed)
    with np.errstate(all="ignore"):
        raw, dom = ora.infer_raw(target, {k: v[sub] for k, v in ev.items()}, N)
    np.testing.assert_array_equal(out[3], dom.reshape(-1, N)[0])
    return assert_quantile(out[0][sub][:, 1:6], raw, FIXED[1:6], 1e-5)  # (p = 0 and 1: compared on the plan's own rows)


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


def _full_batch(s, gpu):
    """check_case on the fixture's 257 rows (once), and its midpoint results."""
    if "full" not in s:
        evt = _t(s["ev"], gpu)
        out = check_case(s["bn"], "X5", evt, 32)
        mp = midpoint_probs(out[4])
        s["full"] = (out, mp, *run_probs(s["bn"], "X5", evt, 32, torch.tensor(mp, device=gpu)))
    return s["full"]


@pytest.mark.parametrize("Q", [1, 2, 3, 16, 17, 257])
def test_staged_chain(Q, staged, gpu):
    """Q >= 2 has an odd query slot, where the lane's upper columns sit in its
    first register block.  The 257-row batch goes through check_case and the
    oracle; a shorter batch is its first Q rows and must reproduce their bits
    (one to three rows alone decide too few entries at p = 1 for the helper,
    which would refuse them; through the equality they are checked all the
    same)."""
    s = staged
    bn = s["bn"]
    out, mp, mi, mv = _full_batch(s, gpu)
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | STAGED | QUANTILE) == FAST | STAGED | QUANTILE, f
    assert out[5] == 0.0
    if Q == 257:
        # the oracle's rows: the list and the midpoints decided at extra = 1e-5, in one comparison
        raw = s["raw"]
        omp = midpoint_probs(raw, 1e-5)
        oi, _ = run_probs(bn, "X5", _t(s["ev"], gpu), 32, torch.tensor(omp, device=gpu))
        probs = np.concatenate([np.broadcast_to(np.float32(FIXED), (Q, 7)), omp], 1)
        assert_quantile(np.concatenate([out[0], oi.cpu().numpy()], 1), raw, probs, 1e-5)
        np.testing.assert_array_equal(out[3], s["dom"].reshape(-1, 32)[0])
        return
    evt = _t({k: v[:Q] for k, v in s["ev"].items()}, gpu)
    index, value, mass = bn.engine.quantile("X5", evt, 32, FIXED)
    np.testing.assert_array_equal(index.cpu().numpy(), out[0][:Q])
    np.testing.assert_array_equal(value.cpu().numpy(), out[1][:Q])
    np.testing.assert_array_equal(mass.cpu().numpy(), out[2][:Q])
    qi, qv = run_probs(bn, "X5", evt, 32, torch.tensor(mp[:Q], device=gpu))
    assert torch.equal(qi, mi[:Q]) and same_bits(qv, mv[:Q])
    bi, bv, bm = bn.engine.quantile("X5", evt, 32, torch.tensor(FIXED, device=gpu).expand(Q, -1).contiguous())
    assert torch.equal(bi, index) and same_bits(bv, value) and same_bits(bm, mass)


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
        assert not f[0] & (FAST | QUANTILE) and out[5] > 0, f
    elif N == 64:
        assert f[0] & (FAST | LDS | QUANTILE) == FAST | LDS | QUANTILE and not f[0] & (COLS | SLOTS | STAGED), f
    else:
        assert f[0] & (FAST | COLS | QUANTILE) == FAST | COLS | QUANTILE, f
    check_oracle(out, OracleBN(edges, cols, data), cols[-1], ev, N)


# ----------------------------------------------------------- n_probs split --
def test_probability_counts_on_the_staged_chain(staged, gpu):
    """P = 1 and 16 run in the query kernel (no scratch), P = 17 stores rows
    and runs k_row_quantile.  The two routes scan in different associations, so
    they must agree wherever the reference decides the entry (and each passes
    the helper on its own)."""
    s = staged
    bn, evt = s["bn"], _t(s["ev"], gpu)
    lib = _native.load()
    rows, extra, own = reference_rows(bn, "X5", evt, 32)
    assert own
    plan = next(iter(bn.engine._plans.values()))
    assert [int(lib.cbn_plan_quantile_scratch(plan.handle, 257, P)) for P in (1, 16, 17)] == [0, 0, 257 * 32]
    mp = midpoint_probs(rows)
    order = np.argsort(np.isnan(mp), axis=1, kind="stable")  # the decided midpoints first
    mp = np.take_along_axis(mp, order, 1)
    p17 = np.concatenate([np.broadcast_to(np.float32(FIXED), (257, 7)), mp[:, :10]], 1)
    got = {}
    for P in (1, 16, 17):
        i, v, m = bn.engine.quantile("X5", evt, 32, torch.tensor(p17[:, :P].copy(), device=gpu))
        assert i.shape == (257, P)
        got[P] = (i.cpu().numpy(), v, m)
    decided = assert_quantile(got[17][0], rows, p17)
    assert_quantile(got[16][0], rows, p17[:, :16])
    np.testing.assert_array_equal(got[1][0], got[16][0][:, :1])
    d16 = decided[:, :16]
    np.testing.assert_array_equal(got[17][0][:, :16][d16], got[16][0][d16])
    ok = np.abs(got[17][2].double().cpu().numpy() - rows.sum(1)) <= 2 * 32 * U * rows.sum(1)
    assert ok.all()
    # a shared list longer than 16
    many = np.linspace(0.0, 1.0, 41).astype(np.float32)
    i, _, _ = bn.engine.quantile("X5", evt, 32, many)
    assert i.shape == (257, 41) and (np.diff(i.cpu().numpy(), axis=1) >= 0).all()
    assert_quantile(i.cpu().numpy(), rows, many)


# ------------------------------------------------------------------- slots --
def test_slots_plan(gpu):
    """k_query_slots at 8 lanes per query (3 x 3 grid, d = 64, peaked CPDs):
    the __shfl_up ladder."""
    data, cols, edges = grid_data(100000, 7, side=3, d=64, keep=0.995, noise=0)
    ev = sample_evidence(data, cols, cols[:-1], 301, 5)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    out = check_case(bn, "X8", _t(ev, gpu), 64)
    f = _flags(bn)
    assert len(f) == 1 and f[0] & (FAST | SLOTS | QUANTILE) == FAST | SLOTS | QUANTILE and not f[0] & LDS, f
    assert out[5] == 0.0 and (out[2] > 0).mean() > 0.9


# --------------------------------------------------------------- fallbacks --
@pytest.mark.parametrize("name", ["generic5", "generic7", "forced_direct", "hashed", "wide", "linear_regression",
                                  "neural_network16"])
def test_fallback_plans(name, gpu, tmp_path):
    """Plans without the epilogue: their stored rows through k_row_quantile
    (N = 5, 7: its scalar loads).  Q = 300 and Q = 1."""
    bn, ora, target, ev, N, want, forbid, seed = _fallback_case(name, gpu, tmp_path)
    forbid = (forbid & ~_native.CBN_PLAN_ARGMAX) | (QUANTILE if forbid & _native.CBN_PLAN_ARGMAX else 0)
    if name == "hashed":
        # the 16 points drawn of X3's ~25 values leave 44 % of the sampled rows without support (mass 0): keep the
        # rows of oracle mass >= 1e-30 and eight of the others (tests/test_gpu_moments.py's batch)
        random.seed(seed)
        m = ora.infer_raw(target, ev, N)[0].sum(1)
        keep = np.sort(np.concatenate([np.flatnonzero(m >= 1e-30), np.flatnonzero(m < 1e-30)[:8]]))
        ev = {k: v[keep] for k, v in ev.items()}
    out = check_case(bn, target, _t(ev, gpu), N, seed)
    f = _flags(bn)
    assert all(x & want == want and not x & forbid for x in f), f
    if name == "wide":  # the [Q, N] column runs on the wide direct plan
        wf = [int(_native.load().cbn_plan_flags(wp.handle)) for _, wp in bn.engine._wide_plans.values()]
        assert len(wf) == 1 and wf[0] & DIRECT and not wf[0] & QUANTILE, wf
    i = int(np.argmax(out[2] > 0))  # the first row with support, alone
    one = {k: v[i:i + 1] for k, v in ev.items()}
    random.seed(seed)
    i1, v1, m1 = bn.engine.quantile(target, _t(one, gpu), N, FIXED)
    np.testing.assert_array_equal(i1.cpu().numpy(), out[0][i:i + 1])
    np.testing.assert_array_equal(m1.cpu().numpy(), out[2][i:i + 1])
    if name == "forced_direct":  # against the table plan of the same network: the same index wherever it is decided
        tb, _, _, _, _, _, _, _ = _fallback_case(name, gpu, tmp_path)
        tb.engine.force_direct = False
        tout = check_case(tb, target, _t(ev, gpu), N, seed, invariance=False)
        assert _flags(tb)[0] & QUANTILE
        probs = np.float32(FIXED[:6] + [0.1, 0.4, 0.6, 0.9])
        a, _, _ = bn.engine.quantile(target, _t(ev, gpu), N, probs)
        b, _, _ = tb.engine.quantile(target, _t(ev, gpu), N, probs)
        decided = assert_quantile(b.cpu().numpy(), tout[4], probs, tout[5])
        np.testing.assert_array_equal(a.cpu().numpy()[decided], b.cpu().numpy()[decided])


def _row_quantile(rows, tv, probs, gpu, stride=None):
    """cbn_row_quantile on device tensors (probs: numpy or tensor, [P] or [Q, P]; made C-contiguous here: numpy
    concatenates a one-column slice in Fortran order, and the C ABI takes row-major arrays)."""
    probs = torch.as_tensor(np.ascontiguousarray(probs) if isinstance(probs, np.ndarray) else probs).to(gpu).contiguous()
    n_rows, n_cols = rows.shape
    P = probs.shape[-1]
    index = torch.empty((n_rows, P), dtype=torch.int32, device=gpu)
    value, mass = torch.empty((n_rows, P), device=gpu), torch.empty(n_rows, device=gpu)
    if stride is None:
        stride = P if probs.dim() == 2 else 0
    with torch.cuda.device(gpu):
        _native.check(_native.load().cbn_row_quantile(_native.ptr(rows), n_rows, n_cols, _native.ptr(tv), _native.ptr(probs),
                                                      P, stride, _native.ptr(index), _native.ptr(value),
                                                      _native.ptr(mass), _native.stream_ptr(gpu)), "cbn_row_quantile")
    return index, value, mass


def row_case(n_cols):
    """(rows [501, n_cols], sample points [n_cols]) of test_row_quantile_kernel: rows 5 and 400 (and some more
    below 8 columns) of mass 0, row 500 a copy of row 0.  Above 64 columns, where a flat row would leave the
    shared list within delta of a cdf step too often for the helper, the first, the last and about eight more
    columns carry the mass (x 1e5)."""
    rng = np.random.default_rng(n_cols)
    raw = (rng.random((501, n_cols)) ** 2 * 1e-9 + 1e-10).astype(np.float32)
    raw[rng.random(raw.shape) < (0.3 if n_cols >= 8 else 0.05)] = 0
    if n_cols > 64:
        big = rng.random(raw.shape) < 8 / n_cols
        big[:, 0] = big[:, -1] = True
        raw = np.where(big, np.maximum(raw, np.float32(1e-10)) * np.float32(1e5), raw).astype(np.float32)
    raw[5] = raw[400] = 0
    raw[500] = raw[0]
    return raw, np.sort(rng.normal(50, 20, n_cols)).astype(np.float32)


ROW_COLS = [1, 3, 4, 5, 7, 12, 32, 33, 255, 260, 1024]


@pytest.mark.parametrize("n_cols", ROW_COLS)
def test_row_quantile_kernel(n_cols, gpu):
    """cbn_row_quantile on stored rows of every lane split (1 .. 64 lanes per
    row; n_cols not a multiple of 4: scalar loads; 260 and 1 024 columns: more
    than one tile per row, so the carry and the rescan run), 501 rows, some of
    mass 0: every column's decided midpoint and the shared list; a row's
    outputs do not depend on its position; P = 1 .. 23."""
    raw, s = row_case(n_cols)
    rows, tv = torch.tensor(raw, device=gpu), torch.tensor(s, device=gpu)
    mp = midpoint_probs(raw)
    assert n_cols > 64 or (~np.isnan(mp)).any(0).all()
    probs = np.concatenate([np.broadcast_to(np.float32(FIXED), (501, 7)), mp[:, :16]], 1)
    index, value, mass = _row_quantile(rows, tv, probs, gpu)
    assert_quantile(index.cpu().numpy(), raw, probs)
    want = torch.where(index >= 0, tv[index.clamp_min(0).long()], torch.full_like(value, float("nan")))
    assert same_bits(value, want)
    m64 = raw.astype(np.float64).sum(1)
    assert (np.abs(mass.double().cpu().numpy() - m64) <= 2 * n_cols * U * m64).all()
    assert torch.equal(index[500], index[0]) and same_bits(mass[500:], mass[:1])
    if n_cols > 16:  # the midpoints of the other columns, 16 at a time
        for c in range(16, min(n_cols, 80), 16):
            pc = np.concatenate([np.broadcast_to(np.float32(FIXED), (501, 7)), mp[:, c:c + 16]], 1)
            i2, _, _ = _row_quantile(rows, tv, pc, gpu)
            assert_quantile(i2.cpu().numpy(), raw, pc)
    # one shared list, and the same list as rows of a wider array (probs_stride > P)
    shared = torch.tensor(FIXED, device=gpu)
    i3, v3, m3 = _row_quantile(rows, tv, shared, gpu)
    assert torch.equal(i3, index[:, :7]) and same_bits(m3, mass)
    wide = torch.full((501, 9), 0.5, device=gpu)
    wide[:, :7] = shared
    assert wide.is_contiguous()
    i4, v4, _ = _row_quantile(rows, tv, wide, gpu, stride=9)
    assert i4.shape == (501, 9)
    i5 = torch.empty((501, 7), dtype=torch.int32, device=gpu)
    with torch.cuda.device(gpu):
        _native.check(_native.load().cbn_row_quantile(_native.ptr(rows), 501, n_cols, None, _native.ptr(wide), 7, 9,
                                                      _native.ptr(i5), None, None, _native.stream_ptr(gpu)), "row")
    assert torch.equal(i5, index[:, :7])


def test_row_quantile_kernel_special_values(gpu):
    """Rows with NaN, inf, -0.0 and an all-zero row, and a bad p among the
    probabilities: index -1 / value NaN for the whole row where the mass is not
    a finite positive number, for the bad entry alone elsewhere; a -0.0 entry
    is a column of probability 0."""
    nan, inf = float("nan"), float("inf")
    raw = np.array([[1.0, 2.0, 0.0, 1.0, 0.0],
                    [1.0, nan, 0.0, 1.0, 0.0],
                    [1.0, inf, 0.0, 1.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0, 0.0],
                    [-0.0, 2.0, -0.0, 2.0, -0.0],
                    [0.0, 0.0, 0.0, 0.0, 3.0]], np.float32)
    p = np.array([0.0, 0.5, nan, 1.0, 1.5, -0.25, 0.8], np.float32)
    tv = torch.arange(5, device=gpu, dtype=torch.float32) + 10
    index, value, mass = _row_quantile(torch.tensor(raw, device=gpu), tv, p, gpu)
    index, value, mass = index.cpu().numpy(), value.cpu().numpy(), mass.cpu().numpy()
    np.testing.assert_array_equal(index[0], [0, 1, -1, 3, -1, -1, 3])
    np.testing.assert_array_equal(index[4], [1, 1, -1, 3, -1, -1, 3])
    np.testing.assert_array_equal(index[5], [4, 4, -1, 4, -1, -1, 4])
    assert (index[1:4] == -1).all()
    assert np.isnan(mass[1]) and np.isinf(mass[2]) and mass[3] == 0 and mass[0] == 4 and mass[4] == 4
    np.testing.assert_array_equal(np.isnan(value), index < 0)
    np.testing.assert_array_equal(value[index >= 0], 10.0 + index[index >= 0])


# ---------------------------------------------------------- special values --
def test_off_domain_evidence_on_the_staged_chain(staged, gpu):
    s = staged
    bn, names = s["bn"], s["names"]
    Q = 4 * len(names) * 20 + 21
    doms = {c: np.unique(s["data"][:, s["cols"].index(c)]) for c in names}
    clean = sample_evidence(s["data"], s["cols"], names, Q, 5)
    ev, rows = special_batch(clean, doms)
    out = check_case(bn, "X5", _t(ev, gpu), 32)
    ref = check_case(bn, "X5", _t(clean, gpu), 32, invariance=False)
    off = np.array([r[0] for r in rows if not r[4]])
    assert off.size >= 17 * len(names)
    # off-domain, NaN, +-inf evidence: an all-zero row -> mass 0, index -1, value NaN for every p
    assert (out[2][off] == 0).all() and (out[0][off] == -1).all() and np.isnan(out[1][off]).all()
    untouched = np.ones(Q, bool)
    untouched[[r[0] for r in rows]] = False
    assert (ref[2] > 0).all() and (ref[0] >= 0).all()
    for a, b in zip(out[:3], ref[:3]):
        np.testing.assert_array_equal(a[untouched], b[untouched])


# ---------------------------------------------------------- redrawn domain --
@pytest.mark.parametrize("force_direct", [False, True])
def test_redrawn_domain(force_direct, gpu):
    """N_max = 7 above the cardinality 4: the sample domains are drawn per
    call; ``value`` uses THIS call's draw."""
    data, cols, edges = chain_data(6, 4, 4000, 21)
    ora = OracleBN(edges, cols, data)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    bn.engine.force_direct = force_direct
    ev = sample_evidence(data, cols, ["X4", "X2"], 200, 6)
    doms, vals = [], []
    for seed in (1, 2, 3, 2):
        out = check_case(bn, "X5", _t(ev, gpu), 7, seed)
        random.seed(seed)
        _, dom = ora.infer_raw("X5", ev, 7)
        np.testing.assert_array_equal(out[3], dom.reshape(-1, 7)[0])
        doms.append(out[3].copy())
        vals.append(out[1].copy())
    assert not np.array_equal(doms[0], doms[1]) and np.array_equal(doms[1], doms[3])
    np.testing.assert_array_equal(vals[1], vals[3])  # (NaN on the rows without support, in both)
    assert len(bn.engine._plans) == 1
    f = _flags(bn)
    assert not force_direct or (f[0] & DIRECT and not f[0] & QUANTILE), f


# ------------------------------------------------------------------ errors --
def test_errors_are_infers_and_precede_any_launch(gpu):
    data, cols, edges = chain_data(6, 4, 4000, 5, stay=0.8)
    ev = sample_evidence(data, cols, ["X4", "X2"], 300, 3)
    two = dict(ev, X4=np.concatenate([ev["X4"], ev["X4"]], 1))
    short = dict(ev, X2=ev["X2"][:299])
    for bad in (two, short, None):
        got = []
        for fn in ("infer", "quantile", "interval", "sample"):
            bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
            with pytest.raises((RuntimeError, AssertionError, AttributeError)) as info:
                getattr(bn, fn)("X5", None if bad is None else _t(bad, gpu), N_max=4)
            got.append((type(info.value), str(info.value)))
            assert all(not p.tables_built for p in bn.engine._plans.values())  # nothing was launched
        assert got[0] == got[1] == got[2] == got[3], got
    # ... and on a cached plan (the native host path declines, the general path raises)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    a = bn.engine.quantile("X5", _t(ev, gpu), 4, FIXED)
    with pytest.raises(RuntimeError, match="expanded size"):
        bn.engine.quantile("X5", _t(two, gpu), 4, FIXED)
    # host probabilities are range-checked before anything else runs; per-query rows must match the batch
    for bad in ([0.5, 1.5], [float("nan")], torch.tensor([-0.5])):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            bn.engine.quantile("X5", _t(ev, gpu), 4, bad)
    with pytest.raises(ValueError, match="rows for 300 queries"):
        bn.engine.quantile("X5", _t(ev, gpu), 4, torch.full((299, 2), 0.5, device=gpu))
    with pytest.raises(ValueError, match="level"):
        bn.interval("X5", _t(ev, gpu), level=1.5, N_max=4)
    with pytest.raises(ValueError, match="n_samples"):
        bn.sample("X5", _t(ev, gpu), n_samples=0, N_max=4)
    # a device tensor is not checked: the bad entry alone is -1 / NaN
    i, v, _ = bn.engine.quantile("X5", _t(ev, gpu), 4, torch.tensor([0.5, 1.5, float("nan")], device=gpu))
    assert torch.equal(i[:, 0], a[0][:, 3]) and (i[:, 1:] == -1).all() and torch.isnan(v[:, 1:]).all()
    # conversions: float64 columns on the host give the float32 device result
    b = bn.engine.quantile("X5", {k: torch.tensor(v, dtype=torch.float64) for k, v in ev.items()}, 4, FIXED)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the C entry point: refused before a launch
    lib, plan = _native.load(), next(iter(bn.engine._plans.values()))
    idx = torch.empty((4, 3), dtype=torch.int32, device=gpu)
    pr = torch.full((4, 3), 0.5, device=gpu)
    col = torch.zeros(4, 1, device=gpu)
    ptrs = (ctypes.c_void_p * 2)(col.data_ptr(), col.data_ptr())
    E, h, ip, pp = _native.CBN_E_ARG, plan.handle, _native.ptr(idx), _native.ptr(pr)
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, None, 3, 0, ip, None, None, None, 0, None) == E  # no probs
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, pp, 3, 0, None, None, None, None, 0, None) == E  # no index
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, pp, 0, 0, ip, None, None, None, 0, None) == E    # n_probs < 1
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, pp, 3, 2, ip, None, None, None, 0, None) == E    # stride < P
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, pp, 3, -3, ip, None, None, None, 0, None) == E
    assert lib.cbn_plan_run_quantile(h, 0, ptrs, 2, None, pp, 3, 3, ip, None, None, None, 0, None) == E    # no queries
    # more probabilities than the kernel serves, without scratch
    assert lib.cbn_plan_quantile_scratch(h, 4, 17) == 4 * 4
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, pp, 17, 0, ip, None, None, None, 0, None) == E
    # ... and with scratch that is not 16-B aligned
    sc = torch.empty(4 * 4 + 4, device=gpu)
    assert sc.data_ptr() % 16 == 0
    assert lib.cbn_plan_run_quantile(h, 4, ptrs, 2, None, pp, 17, 0, ip, None, None, ctypes.c_void_p(sc.data_ptr() + 4), 0,
                                     None) == E
    assert b"aligned" in lib.cbn_last_error()


def test_a_rejected_first_call_leaves_the_plan_unbuilt(gpu):
    """A [Q', P] tensor with the wrong row count as the FIRST call on a new
    network: the ValueError precedes everything that marks the plan's tables as
    built, so the following good call builds them and matches a fresh network."""
    data, cols, edges = chain_data(6, 4, 4000, 5, stay=0.8)
    ev = _t(sample_evidence(data, cols, ["X4", "X2"], 300, 3), gpu)
    for call in ("quantile", "sample"):
        bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
        with pytest.raises(ValueError, match="rows for 300 queries"):
            bn.engine.quantile("X5", ev, 4, torch.full((299, 2), 0.5, device=gpu))
        plans = list(bn.engine._plans.values())
        assert len(plans) == 1 and not plans[0].tables_built
        fresh = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
        if call == "quantile":
            got, want = bn.engine.quantile("X5", ev, 4, FIXED), fresh.engine.quantile("X5", ev, 4, FIXED)
        else:
            g = lambda: torch.Generator(device=gpu).manual_seed(3)  # noqa: E731
            got = bn.sample("X5", ev, n_samples=5, N_max=4, generator=g(), return_index=True)
            want = fresh.sample("X5", ev, n_samples=5, N_max=4, generator=g(), return_index=True)
        assert plans[0].tables_built
        for x, y in zip(got, want):
            assert same_bits(x.float(), y.float())
        assert (got[0] >= 0).all() if call == "quantile" else (got[1] >= 0).all()
        a, b = bn.infer("X5", ev, N_max=4), fresh.infer("X5", ev, N_max=4)
        assert torch.equal(a[0], b[0]) and float(a[0].max()) == 1.0


def test_no_evidence_rows(gpu):
    """n_queries = 1 without evidence rows (evidence = {}): one row of quantiles."""
    data, cols, edges = chain_data(5, 4, 3000, 3)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    index, value, mass = bn.engine.quantile("X4", {}, 4, FIXED)
    assert index.shape == (1, 7) and mass.shape == (1,)
    raw, dom = OracleBN(edges, cols, data).infer_raw("X4", None, 4)
    assert_quantile(index.cpu().numpy(), raw, FIXED, 1e-5)
    assert torch.equal(bn.quantile("X4", {}, FIXED, N_max=4), value)
    assert bn.sample("X4", {}, n_samples=5, N_max=4, generator=torch.Generator(device=gpu).manual_seed(1)).shape == (1, 5)


# ------------------------------------------------------------------ sample --
def test_sample(staged, gpu):
    s = staged
    bn = s["bn"]
    evt = _t({k: v[:3] for k, v in s["ev"].items()}, gpu)
    g = lambda seed: torch.Generator(device=gpu).manual_seed(seed)  # noqa: E731
    # reproducible, and exactly quantile at the same draw -- also beyond CBN_MAX_QUANTILES (the row-kernel route)
    for n in (1, 16, 50):
        a, ai = bn.sample("X5", evt, n_samples=n, N_max=32, generator=g(7), return_index=True)
        b = bn.sample("X5", evt, n_samples=n, N_max=32, generator=g(7))
        assert a.shape == ai.shape == (3, n) and same_bits(a, b)
        u = torch.rand((3, n), device=gpu, dtype=torch.float32, generator=g(7))
        qi, qv, _ = bn.engine.quantile("X5", evt, 32, u)
        assert torch.equal(qi, ai) and same_bits(qv, a)
    assert not torch.equal(bn.sample("X5", evt, n_samples=50, N_max=32, generator=g(8)), a)
    # 4 096 draws per row against posterior's p_j: |freq_j - p_j| <= 5 sqrt(p_j (1 - p_j) / n) + 1 / n (five
    # standard deviations of a binomial share plus one count; deterministic under the fixed seed)
    n = 4096
    v, i = bn.sample("X5", evt, n_samples=n, N_max=32, generator=g(11), return_index=True)
    pdf, dom = bn.posterior("X5", evt, N_max=32)
    p = pdf.double().cpu().numpy()
    assert (i >= 0).all() and same_bits(v, dom.reshape(-1, 32)[0][i.long()])
    freq = np.stack([np.bincount(r, minlength=32) for r in i.cpu().numpy()]) / n
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1 / n).all()
    assert (freq[p == 0] == 0).all()  # no zero-probability column is ever drawn
    # without a generator: the default one
    assert bn.sample("X5", evt, n_samples=4, N_max=32).shape == (3, 4)


# ----------------------------------------------------------------- timeout --
def test_pending_timeout_is_reported_once(staged, gpu):
    s = staged
    bn = s["bn"]
    evt = _t(s["ev"], gpu)
    a = bn.engine.quantile("X5", evt, 32, FIXED)
    plan = next(iter(bn.engine._plans.values()))
    _native.check(_native.load().cbn_debug_flag_timeout(plan.handle), "flag")
    with pytest.raises(_native.NativeError, match="timed out"):
        bn.engine.quantile("X5", evt, 32, FIXED)
    b = bn.engine.quantile("X5", evt, 32, FIXED)  # reported once, then cleared
    for x, y in zip(a, b):
        assert torch.equal(x, y)
