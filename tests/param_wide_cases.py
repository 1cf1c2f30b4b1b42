"""The cases of tests/test_gpu_param_wide.py: parametric networks whose target
reads a [Q, N] evidence column (N per-query values of an observed parent), the
explicit parameters, the evidence and the ``cbn_param_info`` each wide plan
must report.  Shared with tests/test_param_wide_host.py, which shows on the CPU
that the oracle alone can check every case.

Networks (built as tests/param_matrix.py builds its own: ``mixed_dag_data``
columns with >= 64 values each, so N <= 33 subsamples every domain without
random padding and the plans are deterministic; parameters drawn with
param_matrix's bounds, never trained):

    X0 -> X1 -> X2           a short chain, every node observed ([Q, 1])
    X2 -> P_i                one "feeder" per role in ``roles``
    P_* -> T                 the target reads every feeder

A feeder's role: ``w`` observed through a [Q, N] column (wide), ``f``
unobserved (free: its N sample points), ``e`` observed through a [Q, 1] column
that T -- whose evidence keys are not all of its parents -- expands like the
wide one.  Each feeder's own factor has its one parent observed (strict), so
only T reads the wide columns.  ``split``: one more observed node H with the
first wide and the first free feeder as parents, itself a parent of T: two
factors of N^2 combos, the second one in part 1 of the two-part factor split.

Wide values are uniform in the column's [0, 1] range widened by 30 % on each
side, as in the reference-run fixtures (tests/golden/make_golden_param_wide.py).
"""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

import param_matrix as pm
from helpers import mixed_dag_data, sample_evidence

from golden_io import GOLDEN_DIR, oracle_estimators
from parity import assert_marginals_close, n_factors, peak

SMALL = 257
EV_SEED = 29
CHAIN = 3


# ------------------------------------------------ reference-run fixtures -----
def wide_golden_names():
    import json
    import os

    with open(os.path.join(GOLDEN_DIR, "MANIFEST_param_wide.json")) as f:
        return json.load(f)["cases"]


def golden_oracle(g):
    from oracle.ref_infer import OracleBN

    m = g["meta"]
    return OracleBN(m["edges"], m["columns"], g["data"], estimators=oracle_estimators(g))


def assert_wide_golden(got, g, got_raw=None):
    """``got`` vs the fixture's reference pdf at the tolerance of
    ``parity.assert_golden_close`` (the same helper and keywords).  The floor's
    ``raw_max`` is the reference's own unnormalised batch max: these fixtures
    hold their ``raw`` rows.  The fixture that is NaN in every entry compares
    NaN positions and the unnormalised rows (``got_raw``) with the reference's."""
    ora = golden_oracle(g)
    t = g["meta"]["target"]
    with np.errstate(invalid="ignore"):
        kw = dict(raw_max=float(g["raw"].max()), n_factors=n_factors(ora, t), peak=peak(ora, t))
    if np.isnan(g["pdf"]).any():
        assert got_raw is not None, "a NaN fixture needs the unnormalised rows"
        assert_marginals_close(got, g["pdf"], nan="match", got_raw=got_raw, ref_raw=g["raw"], **kw)
    else:
        assert_marginals_close(got, g["pdf"], **kw)


# ------------------------------------------------- kernel-matrix cases -------


@dataclass(frozen=True)
class WCase:
    id: str
    est: str
    scales: str  # unit | half | mixed
    N: int
    roles: Tuple[str, ...] = ("w", "f")
    split: bool = False
    hidden: Optional[Tuple[int, ...]] = None
    act: Optional[str] = None
    rows: int = 33  # rows sent through the oracle (N^(parents of T + 1) values per row)
    info: dict = field(default_factory=dict, compare=False, hash=False)  # expected cbn_param_info fields

    @property
    def model(self):
        return {"hidden_dims": list(self.hidden), "activation": self.act} if self.hidden else None

    @property
    def n(self):
        return CHAIN + len(self.roles) + (1 if self.split else 0) + 1


def _info(nc, N, hmax, mode, tab, parts, generic=0):
    return dict(generic=generic, nc=nc, n_chunks=-(-N // nc), hmax=hmax, mode=mode, tab=tab, m1=0, parts=parts)


def _build_cases():
    out = []

    def add(id, est, scales, N, info, **kw):
        out.append(WCase(id=id, est=est, scales=scales, N=N, info=info, **kw))

    # linear models: <8, 0, MODE, TAB, false>
    for est, sc, mode in pm.LIN_MODES:
        for N in (8, 12, 20):
            add(f"lin-mode{mode}-N{N}", est, sc, N, _info(8, N, 0, mode, 1, 2), rows=65 if N <= 12 else 33)
    # one hidden layer, widths 16 and 7 (a padding unit in the last pair): NC 8 / 16 / 32, N = 33: two chunks
    for i, (N, w, act) in enumerate(((8, 16, "tanh"), (8, 7, "relu"), (16, 16, "relu"), (16, 7, "tanh"),
                                     (20, 16, "tanh"), (20, 7, "relu"), (33, 16, "relu"), (33, 7, "tanh"))):
        sc, mode = pm.NN_MODES[i % 2]
        add(f"h1-mode{mode}-N{N}-w{w}{act}", "neural_network", sc, N, _info(pm._nc_mlp(N), N, 1, mode, 1, 2),
            hidden=(w,), act=act, rows=65 if N <= 8 else 33)
    # two hidden layers: the deep LDS scratch (one part beyond NC = 8)
    add("h32-8x8-mode2-N8", "neural_network", "unit", 8, _info(8, 8, 32, 2, 1, 2), hidden=(8, 8), act="tanh", rows=65)
    add("h32-8x8-mode3-N20", "neural_network", "half", 20, _info(32, 20, 32, 3, 1, 1), hidden=(8, 8), act="tanh")
    # the per-factor switch <16, 32, 4>, column table in LDS (slot mode): mixed scales, a 5-input factor
    add("switch-mixed-logreg-N12", "logistic_regression", "mixed", 12, _info(16, 12, 32, 4, 0, 2), rows=65)
    add("switch-5in-logreg-N12", "logistic_regression", "unit", 12, _info(16, 12, 32, 4, 0, 2),
        roles=("e", "w", "f", "e", "e"), rows=9)
    # beyond the register-resident kernels: k_param_query_gen
    add("generic-33x4-N20", "neural_network", "unit", 20, _info(16, 20, 0, 4, 0, 1, generic=1), hidden=(33, 4),
        act="tanh")
    # shapes of the wide factor, on a linear and a one-hidden-layer plan
    for tag, est, sc, mode, hmax, kw in (("lr", "linear_regression", "half", 1, 0, {}),
                                         ("nn16", "neural_network", "unit", 2, 1, dict(hidden=(16,), act="tanh"))):
        nc = (lambda N: 8) if hmax == 0 else pm._nc_mlp
        add(f"shape-fw-{tag}-N12", est, sc, 12, _info(nc(12), 12, hmax, mode, 1, 2), roles=("f", "w"), **kw)
        add(f"shape-wwf-{tag}-N8", est, sc, 8, _info(nc(8), 8, hmax, mode, 1, 2), roles=("w", "w", "f"), **kw)
        add(f"shape-wff-{tag}-N5", est, sc, 5, _info(nc(5), 5, hmax, mode, 1, 2), roles=("w", "f", "f"), rows=65, **kw)
        add(f"shape-wef-{tag}-N12", est, sc, 12, _info(nc(12), 12, hmax, mode, 1, 2), roles=("w", "e", "f"), **kw)
        add(f"shape-split-{tag}-N8", est, sc, 8, _info(nc(8), 8, hmax, mode, 1, 2), split=True, rows=65, **kw)
    return out


CASES = _build_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


@functools.lru_cache(maxsize=None)
def network(case):
    """(data, columns, edges, target, [Q, 1] evidence names, wide names, params);
    params = {node: ([(W, b), ...], log_scale)}.  Read-only, shared."""
    n = case.n
    data, cols, _ = mixed_dag_data(1500, 5, n=n, max_parents=1, card=128, unit=True)
    assert all(np.unique(data[:, i]).size >= 64 for i in range(n)), "a column with fewer than 64 values"
    data.setflags(write=False)
    edges = [(cols[i - 1], cols[i]) for i in range(1, CHAIN)]
    feeders = cols[CHAIN:CHAIN + len(case.roles)]
    target = cols[-1]
    edges += [(cols[CHAIN - 1], p) for p in feeders] + [(p, target) for p in feeders]
    narrow = list(cols[:CHAIN]) + [p for p, r in zip(feeders, case.roles) if r == "e"]
    wide = [p for p, r in zip(feeders, case.roles) if r == "w"]
    if case.split:
        h = cols[-2]
        free = [p for p, r in zip(feeders, case.roles) if r == "f"]
        edges += [(wide[0], h), (free[0], h), (h, target)]
        narrow.append(h)
    rng = np.random.default_rng(pm._seed(case))
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
    return data, cols, edges, target, narrow, wide, params


def oracle(case):
    from oracle.ref_infer import OracleBN, OracleParametric

    data, cols, edges, _, _, _, params = network(case)
    ests = {c: OracleParametric(pm.FAMILY[case.est], layers, ls, act=case.act,
                                root_bias_only=case.est == "linear_regression") for c, (layers, ls) in params.items()}
    return OracleBN(edges, cols, data, estimators=ests)


def wide_values(Q, N, seed):
    """[Q, N] values uniform in [0, 1] widened by 30 % on each side."""
    return np.random.default_rng(seed).uniform(-0.3, 1.3, (Q, N)).astype(np.float32)


def evidence(case, Q, seed=EV_SEED):
    data, cols, _, _, narrow, wide, _ = network(case)
    ev = sample_evidence(data, cols, narrow, Q, seed)
    for i, w in enumerate(wide):
        ev[w] = wide_values(Q, case.N, seed * 100 + i)
    return ev
