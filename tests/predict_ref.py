"""Reference semantics and the comparison of ``predict`` (helper, not a test).

``predict`` returns, per query row, the first index of the maximum of the
UNNORMALISED product row (the row ``OracleBN.infer_raw`` computes), the
target's sample point there and the maximum itself.  ``raw_argmax`` is that
definition in numpy; ``assert_predictions`` compares a GPU result with the
oracle's rows:

* a row is DECIDED when it is all zero, or its top entry is >= 1e-30 and every
  other entry is < (1 - 1e-4) * top.  1e-4 is ten times the project's rtol
  1e-5 bar (tests/parity.py), so a GPU row within that bar of the oracle's
  cannot flip a decided row: on decided rows the index must be equal;
* on the other rows the chosen column's reference value must be
  >= (1 - 1e-4) * top;
* ``row_max`` is within rtol 1e-5 of the oracle's row max plus the parity
  module's subnormal-rounding floor (n_factors * 2^-149);
* ``value == domain[index]`` exactly;
* the helper REFUSES a comparison in which fewer than 90 % of the rows are
  decided (it would check little).

``check_exact`` is the GPU tests' other check: ``predict`` against the same
plan's ``infer_raw`` rows, bit for bit (tests/test_gpu_predict.py,
tests/test_gpu_staged_shapes.py).
"""
import numpy as np

from parity import SUB

MARGIN = 1e-4
MIN_TOP = 1e-30
MIN_DECIDED = 0.9


def raw_argmax(raw):
    """First index of each row's maximum with torch.argmax's rules: ties to the
    lowest column, a NaN greater than every number (the first NaN wins),
    -0.0 == +0.0, an all-zero row gives 0."""
    raw = np.atleast_2d(np.asarray(raw))
    nan = np.isnan(raw)
    # -inf < every number < +inf < NaN; np.argmax returns the first maximum and compares -0.0 == +0.0
    key = np.where(nan, np.inf, raw.astype(np.float64))
    idx = np.argmax(key, axis=1)
    first_nan = np.argmax(nan, axis=1)
    return np.where(nan.any(1), first_nan, idx).astype(np.int64)


def decided(raw):
    """Boolean per row (module docstring)."""
    raw = np.atleast_2d(np.asarray(raw, np.float64))
    fin = np.isfinite(raw).all(1)
    safe = np.where(fin[:, None], raw, 0.0)
    zero = (safe == 0).all(1)
    if raw.shape[1] == 1:
        return fin & (zero | (safe[:, 0] >= MIN_TOP))
    two = np.sort(safe, axis=1)[:, -2:]  # (the runner-up, the top): a tie makes them equal
    return fin & (zero | ((two[:, 1] >= MIN_TOP) & (two[:, 0] < (1 - MARGIN) * two[:, 1])))


def check_exact(bn, target, evt, N, seed=None):
    """``engine.predict`` against the same plan's own rows, exactly: ``index ==
    torch.argmax(rows, 1)`` and ``row_max == rows.max(1).values`` bit for bit on
    EVERY row, where ``rows`` are ``engine.infer_raw``'s.  Plans without a raw
    launch (generic table plans, redrawn domains) are compared with ``infer``'s
    rows instead, on decided rows.  ``evt``: device evidence columns; ``seed``:
    Python's ``random`` before each call (redrawn domains).  Returns (index,
    value, row_max) as numpy plus whether the plan had raw rows to compare
    with."""
    import random

    import torch

    def bits(t):
        return t.contiguous().view(torch.int32)

    eng = bn.engine
    random.seed(seed)
    index, value, row_max = eng.predict(target, evt, N)
    assert index.dtype == torch.int32 and value.dtype == torch.float32 and row_max.dtype == torch.float32
    random.seed(seed)
    res = eng.infer_raw(target, evt, N)
    if res is not None:
        rows = res[0]
        assert torch.equal(index.long(), torch.argmax(rows, 1))
        mx = rows.max(1).values
        nan = torch.isnan(mx)
        assert torch.equal(torch.isnan(row_max), nan)
        assert torch.equal(bits(row_max)[~nan], bits(mx)[~nan])
    else:
        random.seed(seed)
        rows, _ = bn.infer(target, evt, N_max=N)
        dec = torch.tensor(decided(rows.cpu().numpy()), device=rows.device)
        assert dec.float().mean() >= 0.9
        assert torch.equal(index.long()[dec], torch.argmax(rows, 1)[dec])
    return index.cpu().numpy(), value.cpu().numpy(), row_max.cpu().numpy(), res is not None


def assert_predictions(index, value, row_max, raw_ref, domain, n_factors=1, peak=1.0, min_decided=MIN_DECIDED):
    """GPU ``(index, value, row_max)`` against the oracle's unnormalised rows
    ``raw_ref`` [Q, N] and the target's sample points ``domain`` [N] or [1, N]
    (module docstring; ``n_factors`` / ``peak``: the subnormal floor's terms,
    tests/parity.py).  Returns the share of decided rows."""
    index = np.asarray(index).astype(np.int64).reshape(-1)
    value = np.asarray(value).reshape(-1)
    row_max = np.asarray(row_max, np.float64).reshape(-1)
    raw_ref = np.atleast_2d(np.asarray(raw_ref, np.float64))
    domain = np.asarray(domain)
    domain = domain.reshape(-1, domain.shape[-1])[0]
    Q, N = raw_ref.shape
    if Q == 0:
        raise AssertionError("vacuous comparison: no rows")
    assert index.shape == (Q,) and value.shape == (Q,) and row_max.shape == (Q,), (index.shape, value.shape, Q)
    if not np.isfinite(raw_ref).all():
        raise AssertionError("assert_predictions compares finite reference rows")
    dec = decided(raw_ref)
    share = float(dec.mean())
    if share < min_decided:
        raise AssertionError(f"vacuous comparison: only {share:.1%} of the {Q} rows are decided (< {min_decided:.0%})")
    assert ((index >= 0) & (index < N)).all(), "index out of range"
    ref_idx = raw_argmax(raw_ref)
    bad = np.flatnonzero(dec & (index != ref_idx))
    assert bad.size == 0, (f"{bad.size} decided rows differ; first at row {bad[0]}: got {index[bad[0]]}, "
                           f"ref {ref_idx[bad[0]]}, row {raw_ref[bad[0]]}")
    top = raw_ref.max(1)
    chosen = raw_ref[np.arange(Q), index]
    und = np.flatnonzero(~dec & ~(chosen >= (1 - MARGIN) * top))
    assert und.size == 0, (f"{und.size} undecided rows chose a column below (1 - {MARGIN}) of the top; first at row "
                           f"{und[0]}: column {index[und[0]]} = {chosen[und[0]]}, top {top[und[0]]}")
    tol = 1e-5 * np.abs(top) + n_factors * SUB * float(peak)
    err = np.abs(row_max - top)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"row_max: row {worst} got {row_max[worst]!r}, ref {top[worst]!r}"
    np.testing.assert_array_equal(value, domain[index])
    return share
