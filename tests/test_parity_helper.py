"""tests/parity.py's comparison against the one it replaces.

On the oracle's output for two reference goldens (a 20-factor BruteForce
chain, a neural-network estimator network) the mutations below all PASS the
former ``assert_allclose(rtol=1e-5, atol=1e-7)`` on max-normalised marginals
and are all rejected by ``assert_marginals_close``; the unmutated output
passes both."""
import numpy as np
import pytest

from golden_io import load_golden, load_param_golden
from parity import (OLD_ATOL, OLD_RTOL, assert_factor_close, assert_marginals_close, coverage, golden_raw,
                    golden_scale, tolerance)

CASES = [("chain20_d32_config1", False), ("nn_multi_all", True)]


def _old(got, ref):
    np.testing.assert_allclose(got, ref, rtol=OLD_RTOL, atol=OLD_ATOL)


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    name, param = request.param
    raw = golden_raw(name, param)
    mx, nf, pk = golden_scale(name, param)
    pdf = (raw / raw.max()).astype(np.float32)
    pdf.setflags(write=False)
    ref = (load_param_golden(name) if param else load_golden(name))["pdf"]
    return pdf, ref, dict(raw_max=mx, n_factors=nf, peak=pk)


def test_unmutated_oracle_output_passes(case):
    pdf, ref, kw = case
    _old(pdf, ref)
    assert_marginals_close(pdf, ref, **kw)
    (ne, nr), (oe, orow) = coverage(ref, **kw)
    assert nr > 0.95 and nr > orow + 0.5 and ne > oe  # most rows were not compared before


def test_rows_below_1e7_set_to_zero(case):
    """(a) every row whose max is below 1e-7 written as +0."""
    pdf, ref, kw = case
    got = pdf.copy()
    dead = pdf.max(1) < 1e-7
    assert dead.mean() > 0.5 and (pdf[dead] > 0).any()
    got[dead] = 0
    _old(got, ref)
    with pytest.raises(AssertionError, match="marginals: .* beyond tolerance"):
        assert_marginals_close(got, ref, **kw)


def test_small_entries_off_by_a_thousandth(case):
    """(b) every entry in (1e-30, 1e-7) multiplied by 1.001."""
    pdf, ref, kw = case
    got = pdf.copy()
    small = (pdf > 1e-30) & (pdf < 1e-7)
    assert small.sum() > 10
    got[small] *= np.float32(1.001)
    _old(got, ref)
    with pytest.raises(AssertionError, match="relative error 1.0"):
        assert_marginals_close(got, ref, **kw)


def test_zero_entry_given_a_value(case):
    """(c) one entry that is 0 in ``ref`` written as 1e-12."""
    pdf, ref, kw = case
    got = pdf.copy()
    idx = np.unravel_index(int(np.argmin(ref)), ref.shape)
    assert ref[idx] == 0
    got[idx] = 1e-12
    _old(got, ref)
    with pytest.raises(AssertionError, match=f"worst at \\({idx[0]}, {idx[1]}\\)"):
        assert_marginals_close(got, ref, **kw)


def test_all_nan_against_all_nan_is_refused(case):
    """(d) NaN == NaN for assert_allclose (equal_nan defaults to True)."""
    pdf, ref, kw = case
    nan = np.full_like(ref, np.nan)
    _old(nan, nan)
    with pytest.raises(AssertionError, match="non-finite"):
        assert_marginals_close(nan, nan, **kw)
    with pytest.raises(AssertionError, match="needs got_raw and ref_raw"):
        assert_marginals_close(nan, nan, nan="match", **kw)


def test_all_zero_reference_is_refused(case):
    """(e)"""
    pdf, ref, kw = case
    zero = np.zeros_like(ref)
    _old(zero, zero)
    with pytest.raises(AssertionError, match="all-zero reference"):
        assert_marginals_close(zero, zero, **kw)


def test_too_few_checked_rows_is_refused_unless_stated(case):
    pdf, ref, kw = case
    half = ref.copy()
    half[: (2 * ref.shape[0]) // 3] = 0
    with pytest.raises(AssertionError, match="vacuous comparison: only 0.3"):
        assert_marginals_close(half, half, **kw)
    assert_marginals_close(half, half, min_checked_rows=0.3, **kw)


def test_never_looser_than_the_former_tolerance(case):
    pdf, ref, kw = case
    assert (tolerance(ref, **kw) <= OLD_RTOL * np.abs(ref.astype(np.float64)) + OLD_ATOL).all()
    for mx in (1e-45, 1e-30, 1.0, 1e30):
        assert (tolerance(ref, mx, 100, peak=1e40) <= OLD_RTOL * np.abs(ref.astype(np.float64)) + OLD_ATOL).all()


def test_nan_match_compares_positions_and_raw_rows():
    """nan="match": NaN positions and the unnormalised rows' values, inf and
    NaN positions all have to agree."""
    raw = np.array([[1e-30, 2e-30, 0.0], [np.inf, 3e-20, 1e-10]], np.float32)
    with np.errstate(invalid="ignore"):
        ref = raw / raw.max()  # [[0, 0, 0], [NaN, 0, 0]]
    kw = dict(raw_max=np.inf, n_factors=4, nan="match")
    assert_marginals_close(ref, ref, got_raw=raw, ref_raw=raw, **kw)
    bad = raw.copy()
    bad[0, 1] = 2.001e-30
    with pytest.raises(AssertionError, match="unnormalised rows: 1 of 6"):
        assert_marginals_close(ref, ref, got_raw=bad, ref_raw=raw, **kw)
    bad = raw.copy()
    bad[1, 0] = 1e38  # finite where the reference overflowed
    with pytest.raises(AssertionError, match="inf positions"):
        assert_marginals_close(ref, ref, got_raw=bad, ref_raw=raw, **kw)
    got = ref.copy()
    got[1, 0] = 0.0
    with pytest.raises(AssertionError, match="NaN positions differ"):
        assert_marginals_close(got, ref, got_raw=raw, ref_raw=raw, **kw)


def test_factor_comparison_has_no_1e7_floor():
    ref = np.array([0.25, 1e-20, 0.0], np.float32)
    assert_factor_close(ref, ref)
    got = ref.copy()
    got[1] = 1.001e-20
    with pytest.raises(AssertionError):
        assert_factor_close(got, ref)
    got = ref.copy()
    got[2] = 1e-30
    with pytest.raises(AssertionError):
        assert_factor_close(got, ref)
