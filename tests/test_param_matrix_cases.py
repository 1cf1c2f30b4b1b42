"""Every case of tests/test_gpu_param_matrix.py can be checked by the CPU
oracle alone (no GPU).

``parity.assert_marginals_close`` refuses a comparison in which fewer than
half of the rows hold an entry the relative tolerance governs.  The matrix'
cases are built so that the question never arises: per case, on the rows the
GPU test sends through the oracle (the 257-row batch, or its first 33 rows
where a factor has a free parent), the oracle's rows are finite, their
unnormalised batch max is a normal positive float and EVERY row holds a
governed entry (``parity.coverage``: share of rows 1.0).  A case that cannot
meet this gets other inputs, never a smaller share.
"""
import random

import numpy as np
import pytest

import param_matrix as pm
from parity import FLT_MIN, coverage, oracle_reference


def test_case_table_is_complete_and_distinct():
    ids = [c.id for c in pm.ALL_CASES]
    assert len(set(ids)) == len(ids)
    # every instantiation the table claims: (nc, hmax, mode, tab, m1) of the non-generic cases
    inst = {(c.info["nc"], c.info["hmax"], c.info["mode"], c.info["tab"], c.info["m1"])
            for c in pm.ALL_CASES if not c.info["generic"]}
    want = {(nc, 0, m, 1, 1) for nc in (8, 16) for m in range(4)} | {(8, 0, m, 1, 0) for m in range(4)}
    want |= {(nc, 1, m, 1, m1) for nc in (8, 16, 32) for m in (2, 3) for m1 in (0, 1)}
    want |= {(nc, 32, m, 1, 0) for nc in (8, 16, 32) for m in (2, 3)} | {(16, 32, 4, 0, 0)}
    assert inst == want and len(want) == 31
    assert any(c.info["generic"] for c in pm.CASES)
    for c in pm.ALL_CASES:  # the LDS request the table expects fits what a launch may ask for
        assert c.info["generic"] or c.info["lds_bytes"] <= 160 * 1024 - 256, c.id


@pytest.mark.parametrize("case", pm.ALL_CASES, ids=lambda c: c.id)
def test_case_is_checkable_by_the_oracle(case):
    _, _, _, target, _, _ = pm.network(case)
    rows = pm.oracle_rows(case)
    ev = {k: v[:rows] for k, v in pm.evidence(case, pm.SMALL).items()}
    random.seed(0)
    with np.errstate(all="ignore"):
        ref, dom, kw = oracle_reference(pm.oracle(case), target, ev, case.N)
    assert ref.shape == (rows, case.N) and dom.shape[-1] == case.N
    assert np.isfinite(ref).all()
    assert FLT_MIN <= kw["raw_max"] < np.inf
    (entries, rows_share), _ = coverage(ref, **kw)
    print(f"{case.id}: raw max {kw['raw_max']:.3e}, rtol governs {entries:.3f} of the entries, {rows_share:.3f} of the rows")
    assert rows_share == 1.0
