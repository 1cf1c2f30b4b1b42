"""Every path of a plan gives the same rows, for every fast-path kernel family.

The four fast-path query kernels (``k_query_staged``, ``k_query_fast``,
``k_query_cols``, ``k_query_slots``) are each compiled in five modes (max,
write, fused, raw, arg-max) and share one set of mode epilogues
(csrc/cbn_infer.hip: ``batch_max``, ``round_epilogue``, ``publish_block_max``,
``fused_block_max``).  Which kernel a plan reaches is decided by the planner
(csrc/cbn_table_plan.h; DESIGN.md, "Table plans: one host planner, one
selection"); every family below asserts its ``cbn_plan_flags`` so a plan
cannot silently land elsewhere:

staged        5-node N = 32 chain, all evidence
paired        25-node N = 32 chain, all evidence: one past the staged kernel's
              LDS gate (tests/test_gpu_staged_shapes.py), the paired k_query_fast
fast_lds      5-node d = 64 chain, N = 64: 8 lanes per query with the tables in
              LDS -- too many lanes for k_query_cols, no global tables for
              k_query_slots: the plain k_query_fast
fast_global   66-node d = 16 chain whose node X12 has three observed parents
              (a 256 KiB table: the image is beyond LDS), N = 16: 2 lanes per
              query (not k_query_slots) and more than 64 factors (not
              k_query_cols): k_query_fast gathering from global memory
many_factors  the 100-node N = 32 network of tests/test_gpu_api.py's
              test_global_table_plan_with_many_factors_and_few_slots_takes_a_fast_kernel
              (global tables, 4 lanes per query: k_query_slots takes it)
cols_lds      8-node N = 8 chain: k_query_cols, tables in LDS
cols_global   the k = 3, d = 16, N = 16 star of tests/test_gpu_parity.py's
              test_many_observed_parents_generic_and_global_paths: k_query_cols
              over a global table
slots         the d = 32, side 5 grid of test_slots_plan_lane_counts_rounds_and_survivors:
              k_query_slots.  (VPL 2 only: a slots plan needs > 2 lanes per
              query, so N / 4 is a power of two >= 4 and the plan always takes
              8 columns per lane; no shape reaches the VPL 1 instantiation.)

Batch sizes, from ``engine.fused_capacity`` (``cap``) of the family's plan:
1, 257, cap // 2 + 1 (cols and slots plans: the fused launch then holds two
rounds of products per lane across the barrier), cap, and cap + 1 (the first
batch that falls to raw + scale).  Per family and size, on one seeded batch:

* the default ``infer``, ``infer`` with ``engine.fused = False`` (max pass +
  write pass) and ``infer_raw`` followed by its scale give the same rows bit
  for bit, each into a buffer of NaNs (a row that a launch fails to store
  cannot pass on what an earlier call left in recycled memory);
* ``predict`` equals the arg-max / max of the raw rows bit for bit
  (``predict_ref.check_exact``).

At the smallest size the row is also compared with the CPU oracle through
``parity.assert_marginals_close`` with ``oracle_reference``'s own keywords
(the one query has a nonzero product, below; the helper refuses an all-zero
reference), and at 257 the first 32 rows plus the batch's arg-max row
(the same normaliser on both sides) are.

The size-1 case first runs the cap + 1 batch through every path of the same
plan: the larger grid leaves its per-block max words behind, and the one-block
launches that follow must zero them (``publish_block_max``), or the raw + scale
and two-launch rows are divided by the larger batch's max.  Its one query is
the batch's first whose product is nonzero and below the larger batch's max,
so the case cannot pass vacuously.
"""
import random

import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from helpers import chain_data, grid_data, make_bn, sample_evidence, skewed_chain
from oracle.ref_infer import OracleBN
from parity import assert_marginals_close, oracle_reference
from predict_ref import check_exact

pytestmark = pytest.mark.gpu

FAST, LDS, PAIRED, STAGED = _native.CBN_PLAN_FAST, _native.CBN_PLAN_LDS, _native.CBN_PLAN_PAIRED, _native.CBN_PLAN_STAGED
FUSED, ARGMAX, VPL2 = _native.CBN_PLAN_FUSED, _native.CBN_PLAN_ARGMAX, _native.CBN_PLAN_VPL2
COLS, SLOTS = _native.CBN_PLAN_COLS, _native.CBN_PLAN_SLOTS
EV_SEED = 11
SMALL = 257
ORACLE_ROWS = 32  # of the 257-row batch (the oracle takes up to 50 ms per row of the grid)


def _t(ev, dev):
    return {k: torch.tensor(v, device=dev) for k, v in ev.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _chain(n, d, S, seed, stay):
    data, cols, edges = chain_data(n, d, S, seed, stay=stay)
    return data, cols, edges, cols[-1], cols[:-1]


def _skewed(n):
    data, cols, edges = skewed_chain(n, 32, 40000, 8, stay=0.5, hot=5, p_hot=0.9)
    return data, cols, edges, cols[-1], cols[:-1]


def _fast_global():
    """A d = 16 chain of 66 nodes as ``helpers.skewed_chain`` draws it (a factor's
    column j is P(node = v_j | its evidence), so only a "hot" level that most
    nodes take keeps a 66-factor product inside fp32's range); X12 also depends
    on X10 and X9: 4 096 rows of 16 floats, 256 KiB."""
    rng = np.random.default_rng(23)
    S, d, n, hot = 60000, 16, 66, 5

    def fresh():
        return np.where(rng.random(S) < 0.9, hot, rng.integers(0, d, S))

    X = np.zeros((S, n), np.int64)
    X[:, 0] = fresh()
    for i in range(1, n):
        src = np.where(X[:, i - 2] == X[:, i - 3], X[:, i - 1], X[:, i - 2]) if i == 12 else X[:, i - 1]
        X[:, i] = np.where(rng.random(S) < 0.5, src, fresh())
    assert all(np.unique(X[:, i]).size == d for i in range(n))
    cols = [f"X{i}" for i in range(n)]
    edges = [(cols[i - 1], cols[i]) for i in range(1, n)] + [("X10", "X12"), ("X9", "X12")]
    return X.astype(np.float32), cols, edges, cols[-1], cols[:-1]


def _many_factors():
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
    cols = [f"X{i}" for i in range(n)]
    edges = [(cols[i - 1], cols[i]) for i in range(1, n)] + [(cols[i - 2], cols[i]) for i in (12, 22, 32)]
    return X.astype(np.float32), cols, edges, "X99", ["X10", "X11", "X20", "X21", "X30", "X31", "X98"]


def _star():
    k, d = 3, 16
    rng = np.random.default_rng(k * 10 + d)
    P = rng.integers(0, d, (40000, k))
    C = (P.sum(1) + rng.integers(0, 3, 40000)) % d
    cols = [f"P{i}" for i in range(k)] + ["C"]
    return np.concatenate([P, C[:, None]], 1).astype(np.float32), cols, [(f"P{i}", "C") for i in range(k)], "C", cols[:-1]


def _grid():
    data, cols, edges = grid_data(100000, 7, side=5, d=32, keep=0.995, noise=0)
    return data, cols, edges, cols[-1], cols[:-1]


# family -> (builder, N, flags wanted, flags forbidden, fused launch holds two rounds)
FAMILIES = {
    "staged": (lambda: _skewed(5), 32, FAST | LDS | PAIRED | STAGED | FUSED | ARGMAX, COLS | SLOTS, False),
    "paired": (lambda: _skewed(25), 32, FAST | LDS | PAIRED | FUSED | ARGMAX, STAGED | COLS | SLOTS, False),
    "fast_lds": (lambda: _chain(5, 64, 60000, 16, 0.8), 64, FAST | LDS | FUSED | ARGMAX,
                 PAIRED | STAGED | COLS | SLOTS, False),
    "fast_global": (_fast_global, 16, FAST | FUSED | ARGMAX, LDS | PAIRED | STAGED | COLS | SLOTS, False),
    "many_factors": (_many_factors, 32, FAST | SLOTS | VPL2 | FUSED | ARGMAX, LDS | PAIRED | STAGED | COLS, True),
    "cols_lds": (lambda: _chain(8, 8, 5000, 4, 0.7), 8, FAST | LDS | COLS | FUSED | ARGMAX, PAIRED | STAGED | SLOTS, True),
    "cols_global": (_star, 16, FAST | COLS | FUSED | ARGMAX, LDS | PAIRED | STAGED | SLOTS, True),
    "slots": (_grid, 32, FAST | SLOTS | VPL2 | FUSED | ARGMAX, LDS | PAIRED | STAGED | COLS, True),
}
SIZES = ["cap+1", "1", "257", "half", "cap"]
# cap // 2 + 1 where the fused launch then holds a second round of products (cols and slots plans)
CASES = [(f, s) for f in FAMILIES for s in SIZES if s != "half" or FAMILIES[f][4]]


class Net:
    """One family's network on the GPU with its plan made, the plan's fused
    capacity, and one seeded evidence batch of cap + 1 rows on the device (the
    smaller batches are its prefixes)."""

    def __init__(self, family, gpu):
        build, self.N, self.want, self.forbid, self.two_rounds = FAMILIES[family]
        self.data, self.cols, self.edges, self.target, self.names = build()
        self.bn = make_bn(BayesianNetwork, self.edges, self.cols, self.data, device=gpu)
        eng = self.bn.engine
        self.small = sample_evidence(self.data, self.cols, self.names, SMALL, EV_SEED)
        self.bn.infer(self.target, _t(self.small, gpu), N_max=self.N)
        self.cap = eng.fused_capacity(self.target, self.names, self.N)
        assert self.cap > 2 * SMALL, self.cap
        ev = sample_evidence(self.data, self.cols, self.names, self.cap + 1, EV_SEED)
        assert all(np.array_equal(ev[k][:SMALL], self.small[k]) for k in ev)
        self.ev = _t(ev, gpu)
        self.ora = None

    def flags(self):
        plans = list(self.bn.engine._plans.values())
        assert len(plans) == 1, list(self.bn.engine._plans)
        return int(_native.load().cbn_plan_flags(plans[0].handle))

    def batch(self, q, first=0):
        return {k: v[first:first + q].contiguous() for k, v in self.ev.items()}

    def oracle(self, rows, norm_row=None):
        """``parity.oracle_reference`` on the given rows of the batch."""
        if self.ora is None:
            self.ora = OracleBN(self.edges, self.cols, self.data)
        random.seed(0)
        return oracle_reference(self.ora, self.target,
                                {k: v[rows] for k, v in self.small.items()}, self.N, norm_row=norm_row)


def all_paths(net, q, first=0):
    """The rows of queries [first, first + q) by the default path; asserts that
    the two-launch path, raw + scale and predict agree with them bit for bit.
    Returns (rows, the unnormalised row maxima)."""
    bn, eng, target, N = net.bn, net.bn.engine, net.target, net.N
    evt = net.batch(q, first)
    def nan_rows():  # a row a launch does not store stays NaN (never equal to anything)
        return torch.full((q, N), float("nan"), device=net.bn.device)

    eng.fused = True
    p = eng.infer(target, evt, N, out=nan_rows())[0]
    flags = net.flags()
    assert flags & net.want == net.want and not flags & net.forbid, f"plan flags {flags:#x}"
    assert p.shape == (q, N)
    eng.fused = False
    try:
        p2 = eng.infer(target, evt, N, out=nan_rows())[0]
    finally:
        eng.fused = True
    assert not torch.isnan(p).any()
    np.testing.assert_array_equal(_bits(p2).cpu().numpy(), _bits(p).cpu().numpy())
    res = eng.infer_raw(target, evt, N, out=nan_rows())
    assert res is not None
    row_max = res[0].max(1).values.cpu().numpy()
    scaled = res[3](res[0], res[2].clone())
    np.testing.assert_array_equal(_bits(scaled).cpu().numpy(), _bits(p).cpu().numpy())
    assert check_exact(bn, target, evt, N)[3]
    assert net.flags() == flags
    return p, row_max


@pytest.fixture(scope="module")
def nets(gpu):
    """Each family's network, built once for its sizes."""
    cache = {}

    def get(family):
        if family not in cache:
            cache.clear()  # one family's batch on the device at a time
            cache[family] = Net(family, gpu)
        return cache[family]

    yield get
    cache.clear()


@pytest.mark.parametrize("family,size", CASES)
def test_all_paths_agree(family, size, nets, gpu):
    net = nets(family)
    cap = net.cap
    q = {"cap+1": cap + 1, "1": 1, "257": SMALL, "half": cap // 2 + 1, "cap": cap}[size]
    if size == "1":
        _, big = all_paths(net, cap + 1)  # leaves cap + 1's per-block max words behind
        # the one query: the first whose product is nonzero and below the larger batch's
        # max, so stale words would change its rows
        r = int(np.flatnonzero((big[:SMALL] > 0) & (big[:SMALL] < big.max()))[0])
        p, one = all_paths(net, 1, first=r)
        assert 0 < one[0] < big.max()
        ref, _, kw = net.oracle(np.arange(r, r + 1))
        assert_marginals_close(p.cpu().numpy(), ref, **kw)
        return
    p, _ = all_paths(net, q)
    if size == "257":
        # ORACLE_ROWS rows and the batch's arg-max row, which carries the batch's normaliser
        p = p.cpu().numpy()
        sub = np.append(np.arange(ORACLE_ROWS), int(np.argmax(p.max(1))))
        ref, _, kw = net.oracle(sub, norm_row=-1)
        assert ref[-1].max() == 1.0 and ref.max() == 1.0  # the same normaliser on both sides
        assert_marginals_close(p[sub], ref, **kw)
