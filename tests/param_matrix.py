"""The cases of tests/test_gpu_param_matrix.py: networks, explicit parameters,
evidence and the ``cbn_param_info`` each case must report.

Shared with tests/test_param_matrix_cases.py, which shows on the CPU that the
oracle alone can check every case (finite rows, a normal batch max, every
compared row holding an entry the relative tolerance governs).

Networks: ``helpers.mixed_dag_data(unit=True)`` columns, every second node a
128-level one and the others continuous, so every domain holds >= 64 values
and ``N_max`` up to 64 subsamples it without random padding (the plan is
deterministic and cached).  Parameters are drawn, not trained: weights uniform
in +-0.6 / sqrt(max(1, fan_in / 4)), biases in +-0.2, ``log_scale`` 0 ("unit"),
log 0.5 ("half") or alternating by node ("mixed").

Shapes: ``dag`` (the drawn edges, in-degree <= 3), ``dag2`` (X{i-1} and X{i-2}
-> X{i}), ``chain`` (in-degree 1) and ``wide5`` (a dag2 whose last node has
its five predecessors as parents).  Parameters are given, so the data need
not follow the edges.
Evidence: ``all`` (every node but the target), ``free`` (all but one mid node:
its children's factors take the mean over its N sample points) and ``leaf``
(the target's backbone parent alone: every other factor is query-independent).
"""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from helpers import mixed_dag_data, sample_evidence

EV_SEED = 23
SMALL = 257
ORACLE_ROWS = 33  # rows a case with free parents sends through the oracle (N^(parents + 1) values per row and factor)
FAMILY = {"linear_regression": "gauss", "logistic_regression": "logistic", "neural_network": "logistic"}
COMB_BYTES_PER_COL = 8 * 64 * 4  # the split's combine buffer: one NC x 64 tile per wave of an 8-wave block
DEEP_BYTES = 2 * 32 * 512 * 4    # LDS scratch of a network with >= 2 hidden layers (register-resident kernels)
INCOL_BYTES = 8 * 16             # slot-mode column table, per factor


@dataclass(frozen=True)
class Case:
    id: str
    est: str
    scales: str  # unit | half | mixed
    n: int       # nodes = factors of the product
    N: int
    shape: str = "dag"
    ev: str = "all"
    hidden: Optional[Tuple[int, ...]] = None
    act: Optional[str] = None
    info: dict = field(default_factory=dict, compare=False, hash=False)  # expected cbn_param_info fields

    @property
    def all_evidence(self):
        return self.ev == "all"

    @property
    def model(self):
        return {"hidden_dims": list(self.hidden), "activation": self.act} if self.hidden else None


def _lds(nc, parts, tab, n, deep):
    b = (0 if tab else n * INCOL_BYTES) + (DEEP_BYTES if deep else 0)
    return (b + 15) // 16 * 16 + (COMB_BYTES_PER_COL * nc if parts > 1 else 0)


def _info(nc, N, hmax, mode, tab, m1, parts, n, deep=False, generic=0):
    d = dict(generic=generic, nc=nc, n_chunks=-(-N // nc), hmax=hmax, mode=mode, tab=tab, m1=m1, parts=parts,
             block_threads=256 if generic else 512)
    if not generic:
        d["lds_bytes"] = _lds(nc, parts, tab, n, deep)
    return d


LIN_MODES = (("linear_regression", "unit", 0), ("linear_regression", "half", 1),
             ("logistic_regression", "unit", 2), ("logistic_regression", "half", 3))
NN_MODES = (("unit", 2), ("half", 3))
# one-hidden-layer plans: (N, width, activation).  tanh / relu: the templated
# mlp1p_nin; gelu: the mlp1p_rt switch; 7: a padding unit in the last pair; 48: streamed
H1_SHAPES = ((8, 16, "tanh"), (16, 7, "relu"), (20, 48, "gelu"), (32, 16, "relu"), (40, 7, "gelu"), (64, 48, "tanh"))


def _nc_mlp(N):
    return 8 if N <= 8 else 16 if N <= 16 else 32


def _build_cases():
    out = []

    def add(id, est, scales, n, N, info, **kw):
        out.append(Case(id=id, est=est, scales=scales, n=n, N=N, info=info, **kw))

    # linear, every parent observed: <8 | 16, 0, MODE, TAB, M1>
    for est, sc, mode in LIN_MODES:
        for N in (7, 8, 12, 16, 20, 33, 40):
            for n in ((7, 8) if N in (20, 40) else (8,)):
                nc = 16 if N >= 16 else 8
                parts = 4 if N >= 16 and n >= 8 else 2
                add(f"lin_m1-mode{mode}-N{N}-f{n}", est, sc, n, N, _info(nc, N, 0, mode, 1, 1, parts, n))
    for est, sc, mode in (LIN_MODES[0], LIN_MODES[3]):  # two factors: the split's second range is empty
        for N in (8, 20):
            add(f"lin_m1-mode{mode}-N{N}-f2", est, sc, 2, N, _info(16 if N >= 16 else 8, N, 0, mode, 1, 1, 2, 2),
                shape="chain")
    # linear, one unobserved parent: <8, 0, MODE, TAB, false>, 2 parts
    for est, sc, mode in LIN_MODES:
        for N in (8, 12, 20):
            add(f"lin_free-mode{mode}-N{N}", est, sc, 6, N, _info(8, N, 0, mode, 1, 0, 2, 6), shape="dag2", ev="free")
    # one hidden layer: <8 | 16 | 32, 1, 2 | 3, TAB, M1 | false>
    for sc, mode in NN_MODES:
        for N, w, act in H1_SHAPES:
            add(f"h1_m1-mode{mode}-N{N}-w{w}{act}", "neural_network", sc, 9, N,
                _info(_nc_mlp(N), N, 1, mode, 1, 1, 4, 9), hidden=(w,), act=act)
            if N <= 40:  # (the oracle's free-parent grid at N = 64 is beyond a test's memory)
                add(f"h1_free-mode{mode}-N{N}-w{w}{act}", "neural_network", sc, 6, N,
                    _info(_nc_mlp(N), N, 1, mode, 1, 0, 2, 6), shape="dag2", ev="free", hidden=(w,), act=act)
        add(f"h1_m1-mode{mode}-N16-w16tanh-f7", "neural_network", sc, 7, 16, _info(16, 16, 1, mode, 1, 1, 2, 7),
            hidden=(16,), act="tanh")  # fewer than 8 factors: 2 parts
    # two hidden layers: <8 | 16 | 32, 32, 2 | 3, TAB, false>; the 128 KiB scratch leaves
    # room for the combine buffer at NC = 8 only, so N > 8 runs one part
    for hidden, act in (((8, 8), "tanh"), ((32, 32), "relu")):
        for sc, mode in NN_MODES:
            for N in (8, 16, 20, 40):
                for ev in ("all", "free"):
                    add(f"h32_{ev}-{hidden[0]}x{hidden[1]}-mode{mode}-N{N}", "neural_network", sc, 6, N,
                        _info(_nc_mlp(N), N, 32, mode, 1, 0, 2 if N <= 8 else 1, 6, deep=True),
                        shape="dag2", ev=ev, hidden=hidden, act=act)
    # the per-factor-switch kernel <16, 32, 4, false, false> (column table in LDS)
    for N in (12, 40):
        add(f"switch_mixed-logreg-N{N}", "logistic_regression", "mixed", 6, N, _info(16, N, 32, 4, 0, 0, 2, 6),
            shape="dag2")
        add(f"switch_mixed-8x8-N{N}", "neural_network", "mixed", 6, N, _info(16, N, 32, 4, 0, 0, 1, 6, deep=True),
            shape="dag2", hidden=(8, 8), act="tanh")
        add(f"switch_wide5-logreg-N{N}", "logistic_regression", "unit", 7, N, _info(16, N, 32, 4, 0, 0, 2, 7),
            shape="wide5")
        add(f"switch_wide5-8x8-N{N}", "neural_network", "unit", 7, N, _info(16, N, 32, 4, 0, 0, 1, 7, deep=True),
            shape="wide5", hidden=(8, 8), act="tanh")
    add("switch_mixed-16-N40", "neural_network", "mixed", 6, 40, _info(16, 40, 32, 4, 0, 0, 2, 6), shape="dag2",
        hidden=(16,), act="tanh")
    # beyond the register-resident kernels: k_param_query_gen, 16-column chunks
    for sc, mode in NN_MODES:
        for N in (20, 40):
            add(f"generic-33x4-mode{mode}-N{N}", "neural_network", sc, 6, N,
                _info(16, N, 0, 4, 0, 0, 1, 6, generic=1), shape="dag2", hidden=(33, 4), act="tanh")
    # query-independent factors (k_param_const<0 | 1 | 32>): only the target's factor reads evidence
    for N in (40, 64):
        add(f"const-lr-N{N}", "linear_regression", "unit", 6, N, _info(16, N, 0, 0, 1, 1, 2, 6), shape="chain", ev="leaf")
        add(f"const-16-N{N}", "neural_network", "unit", 6, N, _info(32, N, 1, 2, 1, 1, 2, 6), shape="chain", ev="leaf",
            hidden=(16,), act="tanh")
        add(f"const-8x8-N{N}", "neural_network", "half", 6, N, _info(32, N, 32, 3, 1, 0, 1, 6, deep=True),
            shape="chain", ev="leaf", hidden=(8, 8), act="tanh")
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# Grid-stride batches (more wave tasks than the grid holds): one plan per kernel family
GRID_CASES = [
    # (4-part plans hold two query groups per block: an odd chunk count, so that the task count
    # can be odd and the last trip has an idle group)
    Case("grid-lin16-4parts", "linear_regression", "unit", 8, 40, info=_info(16, 40, 0, 0, 1, 1, 4, 8)),
    Case("grid-lin_free-2parts", "logistic_regression", "half", 6, 20, shape="dag2", ev="free",
         info=_info(8, 20, 0, 3, 1, 0, 2, 6)),
    Case("grid-h1_m1-nc32-4parts", "neural_network", "unit", 9, 20, hidden=(16,), act="tanh",
         info=_info(32, 20, 1, 2, 1, 1, 4, 9)),
    Case("grid-h1_free", "neural_network", "half", 6, 40, shape="dag2", ev="free", hidden=(7,), act="relu",
         info=_info(32, 40, 1, 3, 1, 0, 2, 6)),
    Case("grid-h32", "neural_network", "unit", 6, 40, shape="dag2", hidden=(8, 8), act="tanh",
         info=_info(32, 40, 32, 2, 1, 0, 1, 6, deep=True)),
    Case("grid-generic", "neural_network", "unit", 6, 40, shape="dag2", hidden=(33, 4), act="tanh",
         info=_info(16, 40, 0, 4, 0, 0, 1, 6, generic=1)),
]
# Cross-instantiation equalities under the CBN_PARAM_* diagnostic switches (tests/diag_child.py)
DIAG_CASES = {
    "lin": Case("diag-lin", "linear_regression", "half", 8, 40, info=_info(16, 40, 0, 1, 1, 1, 4, 8)),
    "h1": Case("diag-h1", "neural_network", "half", 9, 40, hidden=(16,), act="tanh",
               info=_info(32, 40, 1, 3, 1, 1, 4, 9)),
}
ALL_CASES = CASES + GRID_CASES + list(DIAG_CASES.values())


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % 100003


@functools.lru_cache(maxsize=None)
def network(case):
    """(data, columns, edges, target, evidence names, params) of a case;
    params = {node: ([(W, b), ...], log_scale)}.  Read-only, shared."""
    mp = {"dag": 3, "dag2": 2, "wide5": 2, "chain": 1}[case.shape]
    data, cols, edges = mixed_dag_data(1500, 5, n=case.n, max_parents=mp, card=128, unit=True)
    if mp == 2:  # every node past X1 has exactly its two predecessors as parents (the drawn edges vary)
        edges = [(cols[i - 1], cols[i]) for i in range(1, case.n)] + [(cols[i - 2], cols[i]) for i in range(2, case.n)]
    if case.shape == "wide5":
        t = cols[-1]
        edges = edges + [(p, t) for p in cols[-6:-1] if (p, t) not in edges]
        assert sum(1 for _, b in edges if b == t) == 5
    assert all(np.unique(data[:, i]).size >= 64 for i in range(case.n)), "a column with fewer than 64 values"
    data.setflags(write=False)
    target = cols[-1]
    if case.ev == "all":
        names = cols[:-1]
    elif case.ev == "free":
        # the free node: one with a child that has a second, observed parent -- that child's factor is
        # the mean over the free parent's N points per query (a child whose only parent is free
        # would be query-independent, and the plan an M1 one)
        indeg = {c: sum(1 for _, b in edges if b == c) for c in cols}
        free = [a for a, b in edges if indeg[b] == 2 and a != cols[0]]
        assert free, "no node with a two-parent child"
        names = [c for c in cols[:-1] if c != free[0]]
    else:
        names = [cols[-2]]
    rng = np.random.default_rng(_seed(case))
    params = {}
    for i, c in enumerate(cols):
        n_in = max(1, sum(1 for _, b in edges if b == c))  # a root's model has one input
        widths = [n_in, *(case.hidden or ()), 1]
        layers = []
        for a, b in zip(widths[:-1], widths[1:]):
            s = 0.6 / math.sqrt(max(1.0, a / 4))
            layers.append((rng.uniform(-s, s, (b, a)).astype(np.float32), rng.uniform(-0.2, 0.2, b).astype(np.float32)))
        ls = {"unit": 0.0, "half": float(np.log(0.5)), "mixed": 0.0 if i % 2 else float(np.log(0.5))}[case.scales]
        params[c] = (layers, ls)
    return data, cols, edges, target, names, params


def oracle(case):
    from oracle.ref_infer import OracleBN, OracleParametric

    data, cols, edges, _, _, params = network(case)
    ests = {c: OracleParametric(FAMILY[case.est], layers, ls, act=case.act,
                                root_bias_only=case.est == "linear_regression") for c, (layers, ls) in params.items()}
    return OracleBN(edges, cols, data, estimators=ests)


def evidence(case, Q, seed=EV_SEED):
    data, cols, _, _, names, _ = network(case)
    return sample_evidence(data, cols, names, Q, seed)


def oracle_rows(case):
    """Rows of the 257-row batch the oracle can take: all of them when every
    parent is observed, else the first ORACLE_ROWS."""
    return SMALL if case.all_evidence else ORACLE_ROWS
