"""The LDS image fill (``lds_dma_copy``) at its edges, through every kernel that calls it.

The copy moves the plan's image (tables, zero / ones rows, domains, records)
to LDS in 1 KiB chunks: each wave takes a contiguous run of chunks, the runs
are rotated by ``blockIdx % nchunk`` and walked as two wrap-free segments in
groups of four chunks (immediate offsets 0 / 1 / 2 / 3 KiB), and only the
copy's last, partial chunk is lane-masked.  A chunk that lands in the wrong
place, or not at all, shows only if a query READS it, so the evidence here is
built to reach the whole image (``base_evidence``):

* queries 1 mod 8 observe ``(i // 8 + k) mod d`` on evidence column k: every
  row of every one-parent table is read (asserted on the host);
* queries 3 mod 8 observe uniform in-domain values, and column k observes
  ``d + 0.5`` on one of them: the zero rows;
* the other queries are rows of the training data (products that are not
  zero: the comparison with the oracle needs them -- a factor's column j is
  P(node = point j | its evidence), so along a chain of many factors only
  evidence that mostly repeats keeps a product above fp32's range);
* every staged plan here has offset slots past its last factor: the ones rows.

A batch of Q queries repeats a base batch of ``B`` = 257 rows (query i = base
row i mod B), so the oracle runs once per network on B rows and the grids can
be large: at least nchunk + 1 blocks of 256 queries, so that some block starts
its rotation at the last chunk and some at chunk 0 (asserted from
``cbn_plan_table_bytes``), plus Q = 1, 255, 256, 257.

Staged plans (N = 32): d = 32 all-evidence chains of 2 .. 6 nodes -- 10, 10,
18, 18 and 26 chunks, all 2 mod 4: a pair of 32-row tables is 8 chunks --
three chains whose leading nodes are free (one-row tables of 256 B: 19, 20 and
29 chunks), and a 14-node chain (60 chunks: the waves' runs are 4 chunks
long, a whole group with all four immediates; the shorter images only reach
the groups of two and one).  Together the image sizes are asserted to
cover every chunk count mod 4 and a partial last chunk
(``test_staged_images_cover_the_copy_edges``).  The other callers: a 25-node
chain (the paired ``k_query_fast``), an N = 16 chain (``k_query_cols``), a
3 x 3 grid (``k_query_slots``, global tables: the small tables and the slot
records are two small copies of arbitrary size), and a global-table plan each
of ``k_query_cols`` and ``k_query_fast`` (small tables + records).  The kernel
is confirmed by ``cbn_plan_flags``.

Per case and size: the fused launch into a NaN-filled buffer against
``OracleBN`` through ``parity.assert_marginals_close`` with the helper's own
keywords; fused == two-pass == raw launch + scale, bit for bit, each into its
own NaN-filled buffer; ``predict`` == arg-max / max of the raw rows
(``predict_ref.check_exact``).
"""
import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from helpers import chain_data, grid_data, make_bn, sample_evidence, skewed_chain
from oracle.ref_infer import OracleBN
from parity import assert_marginals_close, n_factors
from predict_ref import check_exact

pytestmark = pytest.mark.gpu

FAST, LDS, PAIRED, STAGED = _native.CBN_PLAN_FAST, _native.CBN_PLAN_LDS, _native.CBN_PLAN_PAIRED, _native.CBN_PLAN_STAGED
COLS, SLOTS = _native.CBN_PLAN_COLS, _native.CBN_PLAN_SLOTS
B = 257          # base batch (rows the oracle computes)
CHUNK = 1024     # bytes one LDS-DMA wave-instruction moves
BLOCK_Q = 256    # queries per block of a fused N = 32 launch
EV_SEED = 91
SMALL = [1, 255, 256, 257]


def _chain(n, d):
    data, cols, edges = chain_data(n, d, 40000, 30 + n, stay=0.8)  # a dense CPT: no transition has probability 0
    return data, cols, edges, cols[-1], cols[:-1]


def _tail(n, free):
    """An n-node chain whose first ``free`` nodes are not observed: free + 1
    leading one-row tables (the merged prefix) in front of the 32-row ones,
    256 B each -- image sizes between those of the all-evidence chains.
    ``helpers.skewed_chain`` keeps the free nodes' factors inside fp32 range."""
    data, cols, edges = skewed_chain(n, 32, 40000, 8, stay=0.5, hot=5, p_hot=0.9)
    return data, cols, edges, cols[-1], cols[free:-1]


def _grid3():
    data, cols, edges = grid_data(60000, 7, side=3, d=32, keep=0.995, noise=0)
    return data, cols, edges, cols[-1], cols[:-1]


def _cols_global():
    """A d = 16 chain whose node X6 also depends on X4 and X3: that table has
    4 096 rows of 16 floats (256 KiB, more than the LDS), so the plan keeps its
    tables in global memory and copies only the small ones and the records."""
    rng = np.random.default_rng(23)
    S, d, n = 60000, 16, 10
    X = np.zeros((S, n), np.int64)
    X[:, 0] = rng.integers(0, d, S)
    for i in range(1, n):
        src = np.where(X[:, i - 2] == X[:, i - 3], X[:, i - 1], X[:, i - 2]) if i == 6 else X[:, i - 1]
        X[:, i] = np.where(rng.random(S) < 0.8, src, rng.integers(0, d, S))
    cols = [f"X{i}" for i in range(n)]
    edges = [(cols[i - 1], cols[i]) for i in range(1, n)] + [("X4", "X6"), ("X3", "X6")]
    return X.astype(np.float32), cols, edges, cols[-1], cols[:-1]


def _fast_global():
    """The same with 66 nodes (more factors than ``k_query_cols`` takes: the
    global-table ``k_query_fast``), drawn as ``helpers.skewed_chain`` does: only
    a "hot" level that most nodes take keeps a 66-factor product inside fp32's
    range.  X12 also depends on X10 and X9."""
    rng = np.random.default_rng(23)
    S, d, n, hot = 60000, 16, 66, 5

    def fresh():
        return np.where(rng.random(S) < 0.9, hot, rng.integers(0, d, S))

    X = np.zeros((S, n), np.int64)
    X[:, 0] = fresh()
    for i in range(1, n):
        src = np.where(X[:, i - 2] == X[:, i - 3], X[:, i - 1], X[:, i - 2]) if i == 12 else X[:, i - 1]
        X[:, i] = np.where(rng.random(S) < 0.5, src, fresh())
    cols = [f"X{i}" for i in range(n)]
    edges = [(cols[i - 1], cols[i]) for i in range(1, n)] + [("X10", "X12"), ("X9", "X12")]
    return X.astype(np.float32), cols, edges, cols[-1], cols[:-1]


# name -> (builder, N, flags wanted, flags forbidden, large batch, base rows)
CASES = {
    **{f"staged_{n}": (lambda n=n: _chain(n, 32), 32, FAST | LDS | PAIRED | STAGED, COLS | SLOTS, None, B)
       for n in (2, 3, 4, 5, 6, 14)},
    # 19, 20 and 29 chunks (the all-evidence chains: 10, 10, 18, 18, 26 and 60)
    **{f"staged_tail_{n}": (lambda n=n, p=p: _tail(n, p), 32, FAST | LDS | PAIRED | STAGED, COLS | SLOTS, None, B)
       for n, p in ((7, 3), (12, 7), (14, 7))},
    "paired_25": (lambda: _chain(25, 32), 32, FAST | LDS | PAIRED, STAGED | COLS | SLOTS, None, B),
    "cols_16": (lambda: _chain(8, 16), 16, FAST | LDS | COLS, STAGED | SLOTS, 20001, B),
    "slots_grid3": (_grid3, 32, FAST | SLOTS, LDS | STAGED | COLS, 8193, B),
    "cols_global": (_cols_global, 16, FAST | COLS, LDS | STAGED | SLOTS, 20001, B),
    "fast_global": (_fast_global, 16, FAST, LDS | STAGED | COLS | SLOTS, 20001, B),
}
STAGED_CASES = [c for c in CASES if c.startswith("staged_")]


def _bits(t):
    return t.contiguous().view(torch.int32)


def base_evidence(data, cols, names, d, nb=B):
    """The nb base queries (module docstring)."""
    ev = sample_evidence(data, cols, names, nb, EV_SEED)
    rng = np.random.default_rng(EV_SEED + 1)
    i = np.arange(nb)
    rot, rnd = i % 8 == 1, i % 8 == 3
    for k, nm in enumerate(names):
        v = ev[nm][:, 0]
        v[rot] = (i[rot] // 8 + k) % d
        v[rnd] = rng.integers(0, d, int(rnd.sum()))
        v[(8 * k + 3) % (nb - nb % 8)] = d + 0.5  # outside the domain (and no integer): a zero row
        assert set(v[rot].astype(int)) == set(range(d)), nm  # every row of a one-parent table is read
    return ev


class Net:
    def __init__(self, name, gpu):
        build, self.N, self.want, self.forbid, self.big, self.nb = CASES[name]
        self.data, self.cols, self.edges, self.target, self.names = build()
        d = int(self.data.max()) + 1
        assert d == self.N and all(np.unique(self.data[:, c]).size == d for c in range(self.data.shape[1]))
        self.bn = make_bn(BayesianNetwork, self.edges, self.cols, self.data, device=gpu)
        self.ora = OracleBN(self.edges, self.cols, self.data)
        self.ev = base_evidence(self.data, self.cols, self.names, d, self.nb)
        self.raw, self.dom = self.ora.infer_raw(self.target, self.ev, self.N)
        self.raw.setflags(write=False)
        self.nf = n_factors(self.ora, self.target)
        # off-domain evidence gives all-zero rows, the data's own rows do not
        assert (self.raw.max(1) == 0).any() and (self.raw.max(1) > 0).mean() > 0.6

    def batch(self, q, gpu):
        idx = np.arange(q) % self.nb
        evt = {k: torch.tensor(v[idx], device=gpu) for k, v in self.ev.items()}
        mx = self.raw[:min(q, self.nb)].max()
        ref = (self.raw / mx).astype(np.float32)[idx]
        return evt, ref, self.dom[idx] if self.dom.shape[0] == self.nb else self.dom, dict(
            raw_max=float(mx), peak=1.0, n_factors=self.nf)

    def plan(self):
        plans = list(self.bn.engine._plans.values())
        assert len(plans) == 1, list(self.bn.engine._plans)
        lib = _native.load()
        return int(lib.cbn_plan_flags(plans[0].handle)), int(lib.cbn_plan_table_bytes(plans[0].handle))


@pytest.fixture(scope="module")
def nets(gpu):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Net(name, gpu)
        return cache[name]

    yield get
    cache.clear()


def nan_rows(q, n, gpu):
    return torch.full((q, n), float("nan"), dtype=torch.float32, device=gpu)


def check(net, q, gpu):
    eng, target, N = net.bn.engine, net.target, net.N
    evt, ref, rdom, kw = net.batch(q, gpu)
    eng.fused = True
    out = nan_rows(q, N, gpu)
    pdf, dom = eng.infer(target, evt, N, out)
    assert pdf.data_ptr() == out.data_ptr() and not torch.isnan(out).any()
    flags, nbytes = net.plan()
    print(f"plan flags {flags:#x}, image {nbytes} B = {-(-nbytes // CHUNK)} chunks, last chunk {nbytes % CHUNK} B, Q {q}")
    assert flags & net.want == net.want and not flags & net.forbid, f"plan flags {flags:#x}"
    # 1. the oracle
    np.testing.assert_array_equal(dom.cpu().numpy(), rdom)
    assert_marginals_close(pdf.cpu().numpy(), ref, **kw)
    # 2. fused == two-pass == raw launch + scale
    out_raw = nan_rows(q, N, gpu)
    res = eng.infer_raw(target, evt, N, out_raw)
    assert res is not None and res[0].data_ptr() == out_raw.data_ptr() and not torch.isnan(out_raw).any()
    scaled = res[3](res[0], res[2].clone())
    assert torch.equal(_bits(scaled), _bits(pdf))
    eng.fused = False
    try:
        out2 = nan_rows(q, N, gpu)
        p2, _ = eng.infer(target, evt, N, out2)
        assert p2.data_ptr() == out2.data_ptr() and not torch.isnan(out2).any()
    finally:
        eng.fused = True
    assert torch.equal(_bits(p2), _bits(pdf))
    # 3. predict == arg-max / max of the raw rows
    assert check_exact(net.bn, target, evt, N)[3]
    assert net.plan()[0] == flags
    return nbytes


@pytest.mark.parametrize("q", SMALL + ["wrap"])
@pytest.mark.parametrize("name", STAGED_CASES)
def test_staged_image(name, q, nets, gpu):
    net = nets(name)
    if q == "wrap":  # nchunk + 1 blocks and a ragged one: every rotation start, the wrap at chunk 0 included
        check(net, 1, gpu)
        nchunk = -(-net.plan()[1] // CHUNK)
        q = BLOCK_Q * (nchunk + 1) + 77
        assert q <= 65536
    check(net, q, gpu)


def test_staged_images_cover_the_copy_edges(nets, gpu):
    """The staged cases' images, in chunks: residues 1, 2 and 3 mod 4 (the
    groups' remainders), a partial last chunk (the masked tail), and an image
    of fewer chunks than the block has waves."""
    sizes = {}
    for name in STAGED_CASES:
        net = nets(name)
        check(net, 1, gpu)
        sizes[name] = net.plan()[1]
    chunks = {n: -(-b // CHUNK) for n, b in sizes.items()}
    print("image bytes", sizes, "chunks", chunks)
    assert {c % 4 for c in chunks.values()} == {0, 1, 2, 3}, chunks
    assert any(b % CHUNK for b in sizes.values()), sizes
    assert all(b % 16 == 0 for b in sizes.values()), sizes
    assert min(chunks.values()) < 16, chunks


@pytest.mark.parametrize("q", [257, "big"])
@pytest.mark.parametrize("name", [c for c in CASES if c not in STAGED_CASES])
def test_other_callers(name, q, nets, gpu):
    net = nets(name)
    if q == "big":
        if net.big is None:  # an LDS image: nchunk + 1 blocks, as the staged cases
            check(net, 1, gpu)
            q = BLOCK_Q * (-(-net.plan()[1] // CHUNK) + 1) + 77
            assert q <= 65536
        else:
            q = net.big
    check(net, q, gpu)
