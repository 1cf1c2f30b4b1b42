"""Reference semantics and the comparison of ``posterior`` / ``expect``
(helper, not a test).

Per query row, with ``raw`` the UNNORMALISED product row and ``s`` the
target's sample points: ``mass = sum_j raw_j``, ``pdf_j = raw_j / mass``,
``mean = (sum_j raw_j s_j) / mass``, ``var = (sum_j raw_j (s_j - mean)^2) /
mass``.  ``moments_f64`` is that definition in float64; ``assert_moments``
compares a GPU result with it.

The bounds are derived, not measured.  ``u = 2^-24`` (float32 unit roundoff),
``N`` the row length, ``A = sum_j p_j |s_j| / sum_j p_j``.  A float32 sum of N
non-negative terms in any order is within ``(N - 1) u`` (relative, first
order) of the exact sum; the factor 2 in each bound covers the higher-order
terms and the final division.

* against the SAME plan's own float32 raw rows (``own=True``: only the
  summation error counts)::

      |mass - ref| <= 2 N u ref
      |mean - ref| <= 2 (2 N + 2) u A                     =: tm
      |var  - ref| <= 2 (2 N + 8) u ref + tm^2

  (the mean's numerator carries a product rounding per term, and numerator and
  mass each a summation error; a mean error d changes the centred second
  moment by exactly d^2 -- the cross term sum_j p_j (s_j - mean) vanishes --
  and (s_j - mean)^2 adds three roundings per term);

* against the oracle's rows (``own=False``), which agree with the GPU's to
  rtol 1e-5 per entry (tests/parity.py): ``1e-5 ref`` more on the mass,
  ``2e-5 A`` more in ``tm``, ``2e-5 ref`` more on the variance.

``mean`` and ``var`` are compared on rows with ``mass >= 1e-30`` only (below,
the rows' own entries are subnormal and carry no relative accuracy); on rows of
mass 0 the NaN positions must match exactly (mass 0; pdf, mean, var NaN).  The
helper REFUSES a comparison in which fewer than 90 % of the rows have ``mass >=
1e-30`` (it would check little).
"""
import numpy as np

U = 2.0 ** -24
MIN_MASS = 1e-30
MIN_SHARE = 0.9


def moments_f64(raw, points):
    """(mass [Q], mean [Q], var [Q], pdf [Q, N]) in float64 from rows [Q, N]
    and the sample points [N] or [1, N]; 0 / 0 = NaN on rows of mass 0."""
    raw = np.atleast_2d(np.asarray(raw, np.float64))
    s = np.asarray(points, np.float64)
    s = s.reshape(-1, s.shape[-1])[0]
    assert s.shape == (raw.shape[1],), (s.shape, raw.shape)
    with np.errstate(all="ignore"):
        mass = raw.sum(1)
        pdf = raw / mass[:, None]
        mean = (raw * s).sum(1) / mass
        var = (raw * (s - mean[:, None]) ** 2).sum(1) / mass
    return mass, mean, var, pdf


def abs_mean(raw, points):
    """A = sum_j p_j |s_j| / sum_j p_j per row (float64)."""
    raw = np.atleast_2d(np.asarray(raw, np.float64))
    s = np.asarray(points, np.float64)
    s = np.abs(s.reshape(-1, s.shape[-1])[0])
    with np.errstate(all="ignore"):
        return (raw * s).sum(1) / raw.sum(1)


def mean_tolerance(raw, points, own):
    """tm per row (module docstring)."""
    N = np.atleast_2d(raw).shape[1]
    return (2 * (2 * N + 2) * U + (0.0 if own else 2e-5)) * abs_mean(raw, points)


def assert_moments(mass, mean, var, raw_ref, points, own, min_share=MIN_SHARE):
    """GPU ``(mass, mean, var)`` [Q] against the reference rows ``raw_ref`` [Q,
    N] (finite, >= 0) and the sample points (module docstring).  ``own``: the
    rows are the same plan's float32 raw rows, else the oracle's.  Returns the
    share of rows with mass >= 1e-30."""
    raw_ref = np.atleast_2d(np.asarray(raw_ref, np.float64))
    Q, N = raw_ref.shape
    if Q == 0:
        raise AssertionError("vacuous comparison: no rows")
    mass, mean, var = (np.asarray(x, np.float64).reshape(-1) for x in (mass, mean, var))
    assert mass.shape == mean.shape == var.shape == (Q,), (mass.shape, mean.shape, var.shape, Q)
    if not (np.isfinite(raw_ref).all() and (raw_ref >= 0).all()):
        raise AssertionError("assert_moments compares finite non-negative reference rows")
    rm, rmean, rvar, _ = moments_f64(raw_ref, points)
    big = rm >= MIN_MASS
    share = float(big.mean())
    if share < min_share:
        raise AssertionError(f"vacuous comparison: only {share:.1%} of the {Q} rows have mass >= {MIN_MASS} "
                             f"(< {min_share:.0%})")
    extra = 0.0 if own else 1.0
    err = np.abs(mass - rm)
    tol = (2 * N * U + extra * 1e-5) * rm
    worst = int(np.argmax(err - tol))
    assert (err[rm > 0] <= tol[rm > 0]).all(), f"mass: row {worst} got {mass[worst]!r}, ref {rm[worst]!r}"
    zero = rm == 0
    if own:  # the same rows: exactly the rows of mass 0 are 0 / NaN / NaN
        assert ((mass == 0) == zero).all(), "mass == 0 rows differ"
    assert (mass[zero] == 0).all(), "a row of reference mass 0 has mass != 0"
    assert np.isnan(mean[zero]).all() and np.isnan(var[zero]).all(), "mass == 0 rows: mean / var must be NaN"
    assert not np.isnan(mean[big]).any() and not np.isnan(var[big]).any(), "NaN in a row with mass >= 1e-30"
    tm = mean_tolerance(raw_ref, points, own)
    err = np.abs(mean - rmean)[big]
    if big.any():
        worst = int(np.argmax(err - tm[big]))
        assert (err <= tm[big]).all(), (f"mean: row {np.flatnonzero(big)[worst]} got {mean[big][worst]!r}, "
                                        f"ref {rmean[big][worst]!r}, tol {tm[big][worst]!r}")
        tv = (2 * (2 * N + 8) * U + extra * 2e-5) * rvar[big] + tm[big] ** 2
        err = np.abs(var - rvar)[big]
        worst = int(np.argmax(err - tv))
        assert (err <= tv).all(), (f"var: row {np.flatnonzero(big)[worst]} got {var[big][worst]!r}, "
                                   f"ref {rvar[big][worst]!r}, tol {tv[worst]!r}")
    return share
