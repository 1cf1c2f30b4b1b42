"""One comparison for max-normalised marginals, over their whole dynamic range.

``BayesianNetwork.infer`` divides the factor products by ONE max over the
whole batch (bayesian_network.py:296), and the products here have 18-100
factors, so almost every entry of a batch lies far below 1.  A fixed absolute
tolerance (the former ``atol=1e-7``) accepts any value, zero included, for
every entry below it.  The reference's values carry full fp32 relative
precision down to where the UNnormalised product goes subnormal, so the
per-entry tolerance here is

    rtol * |ref|  +  min(1e-7, n_factors * 2^-149 * peak / raw_max)

* ``raw_max``: the batch max of the unnormalised products -- read from the
  oracle's ``infer_raw`` (or a fixture's own ``raw`` rows), NEVER from the code
  under test.  An upper bound of it gives a tighter check, a lower bound a
  looser one.
* ``n_factors * 2^-149 * peak``: the subnormal-rounding bound of DESIGN.md
  ("order guard"): every product that rounds in the subnormal range errs by at
  most half a subnormal step, and is then multiplied by at most the remaining
  factors, ``peak = prod_f max(1, peak_f)`` (1 for BruteForce: every factor is
  a probability or a mean of probabilities; a Gaussian's norm 1/(s sqrt(2 pi))
  or a logistic density's 1/(4 s) for the parametric estimators).
* the ``min`` with 1e-7 keeps the helper at least as tight as the former
  ``assert_allclose(rtol=1e-5, atol=1e-7)`` at every entry.

The helper RAISES on comparisons that would check nothing: a non-finite
``ref`` (unless ``nan="match"``), a ``ref`` whose max is not positive, and a
``ref`` in which fewer than ``min_checked_rows`` of the rows hold an entry that
the relative term governs (tolerance below 1e-3 of the entry).
"""
import functools
import random

import numpy as np

OLD_RTOL, OLD_ATOL = 1e-5, 1e-7  # the former comparison; the helper is never looser
SUB = 2.0 ** -149  # the smallest fp32 subnormal
FLT_MIN = 2.0 ** -126
CHECKED = 1e-3  # an entry is "really checked" when its tolerance is below this share of it


def tolerance(ref, raw_max, n_factors, peak=1.0, rtol=1e-5):
    """Per-entry tolerance (module docstring), float64, shape of ``ref``."""
    raw_max = float(raw_max)
    if raw_max == np.inf:  # every finite product normalises to exactly 0
        floor = 0.0
    elif not raw_max > 0:  # 0 / 0 (nan="match" only): no finite entry is left to compare
        floor = OLD_ATOL
    else:
        floor = min(OLD_ATOL, float(n_factors) * SUB * float(peak) / raw_max)
    return rtol * np.abs(np.asarray(ref, np.float64)) + floor


def coverage(ref, raw_max, n_factors, peak=1.0, rtol=1e-5):
    """(share of entries, share of rows) the relative term governs under this
    helper, and the same two shares under the former rtol 1e-5 / atol 1e-7."""
    ref = np.atleast_2d(np.asarray(ref, np.float64))
    fin = np.isfinite(ref)
    a = np.where(fin, np.abs(ref), 0.0)
    new = fin & (tolerance(a, raw_max, n_factors, peak, rtol) < CHECKED * a)
    old = fin & (OLD_RTOL * a + OLD_ATOL < CHECKED * a)
    return (float(new.mean()), float(new.any(1).mean())), (float(old.mean()), float(old.any(1).mean()))


def _worst(got, ref, tol, what):
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        bad = ~(err <= tol)
        if not bad.any():
            return None
        over = np.where(bad, err / np.where(tol > 0, tol, SUB), -1.0)
        idx = np.unravel_index(int(np.argmax(over)), over.shape)
        rel = err[idx] / abs(ref[idx]) if ref[idx] != 0 else np.inf
    return (f"{what}: {int(bad.sum())} of {bad.size} entries beyond tolerance; worst at {tuple(int(i) for i in idx)}: "
            f"got {got[idx]!r}, ref {ref[idx]!r}, relative error {rel:.3e}, tolerance {tol[idx]:.3e}")


def assert_marginals_close(got, ref, *, raw_max, n_factors, peak=1.0, rtol=1e-5, nan="forbid",
                           min_checked_rows=0.5, got_raw=None, ref_raw=None):
    """``got`` vs ``ref`` ([Q, N] max-normalised marginals) at the module's
    tolerance.  ``nan="match"`` (fixtures whose reference output is NaN by
    design): NaN positions must be equal, and the caller passes the
    unnormalised rows of both sides (``got_raw``, ``ref_raw``), compared at
    ``rtol`` and atol ``n_factors * 2^-149 * peak`` with inf / NaN positions
    equal -- so the NaN is shown to arise for the reference's reason (0 / 0 or
    inf / inf) and the finite entries to carry values; the guards against
    vacuous comparisons then rest on those rows."""
    assert nan in ("forbid", "match")
    got = np.atleast_2d(np.asarray(got, np.float64))
    ref = np.atleast_2d(np.asarray(ref, np.float64))
    if got.shape != ref.shape:
        raise AssertionError(f"shapes differ: got {got.shape}, ref {ref.shape}")
    if ref.size == 0:
        raise AssertionError("vacuous comparison: ref is empty")
    fin = np.isfinite(ref)
    if nan == "forbid":
        if not fin.all():
            raise AssertionError(f"vacuous comparison: ref has {int((~fin).sum())} non-finite entries of {ref.size} "
                                 "(nan=\"forbid\")")
        if not ref.max() > 0:
            raise AssertionError("vacuous comparison: ref.max() <= 0 (an all-zero reference)")
        if not (np.isfinite(raw_max) and raw_max > 0):
            raise AssertionError(f"raw_max = {raw_max!r}: the oracle's unnormalised batch max must be finite and > 0")
    else:
        if got_raw is None or ref_raw is None:
            raise AssertionError("nan=\"match\" needs got_raw and ref_raw (the unnormalised rows of both sides)")
        if np.isinf(ref).any():
            raise AssertionError("ref holds inf: a max-normalised marginal is finite or NaN")
        graw = np.atleast_2d(np.asarray(got_raw, np.float64))
        rraw = np.atleast_2d(np.asarray(ref_raw, np.float64))
        if graw.shape != ref.shape or rraw.shape != ref.shape:
            raise AssertionError(f"raw shapes {graw.shape}, {rraw.shape} differ from {ref.shape}")
        for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            if not np.array_equal(f(graw), f(rraw)):
                raise AssertionError(f"{name} positions of the unnormalised rows differ: "
                                     f"got {int(f(graw).sum())}, ref {int(f(rraw).sum())}")
        rfin = np.isfinite(rraw)
        rtol_raw = rtol * np.abs(np.where(rfin, rraw, 0.0)) + n_factors * SUB * float(peak)
        msg = _worst(np.where(rfin, graw, 0.0), np.where(rfin, rraw, 0.0), rtol_raw, "unnormalised rows")
        if msg:
            raise AssertionError(msg)
        if not np.array_equal(np.isnan(got), np.isnan(ref)):
            raise AssertionError(f"NaN positions differ: got {int(np.isnan(got).sum())}, ref {int(np.isnan(ref).sum())} "
                                 f"of {ref.size}")
    a = np.where(fin, ref, 0.0)
    tol = tolerance(a, raw_max, n_factors, peak, rtol)
    governed = fin & (tol < CHECKED * np.abs(a))
    if nan == "forbid":
        share = float(governed.any(1).mean())
        if share < min_checked_rows:
            raise AssertionError(f"vacuous comparison: only {share:.3f} of ref's {ref.shape[0]} rows hold an entry the "
                                 f"relative term governs (min_checked_rows={min_checked_rows})")
    old = fin & (OLD_RTOL * np.abs(a) + OLD_ATOL < CHECKED * np.abs(a))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - a)[governed] / np.abs(a)[governed]
    # one line per comparison (pytest shows it with -rA): coverage at a glance
    print(f"parity: {ref.shape[0]} rows, rtol governs {governed.mean():.3f} of the entries / "
          f"{governed.any(1).mean():.3f} of the rows (rtol 1e-5, atol 1e-7: {old.mean():.3f} / {old.any(1).mean():.3f}); "
          f"worst relative error on them {rel.max() if rel.size else 0.0:.2e}")
    msg = _worst(np.where(fin, got, 0.0), a, tol, "marginals")
    if msg:
        raise AssertionError(f"{msg}; rtol governs {governed.mean():.3f} of the entries, "
                             f"{governed.any(1).mean():.3f} of the rows")


def assert_factor_close(got, ref, n_terms=1, rtol=1e-5):
    """A single factor's values (``get_prob``: a probability, a density, or a
    sum / mean of ``n_terms`` of them -- not a normalised product): rtol plus
    one subnormal step per summed term."""
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=SUB * n_terms)


def n_factors(ora, target):
    """Factors in ``target``'s product: its ancestors and itself."""
    return len(ora.ancestors(target)) + 1


def peak(ora, target):
    """prod_f max(1, peak_f) over ``target``'s factors, from the ORACLE's
    parameters: a Gaussian's norm 1 / (s sqrt(2 pi)), a logistic density's
    1 / (4 s); 1 for BruteForce factors."""
    import torch

    from oracle.ref_infer import OracleParametric

    p = 1.0
    for n in ora.ancestors(target) + [target]:
        est = ora.nodes[n].est
        if isinstance(est, OracleParametric):
            s = float(torch.exp(torch.tensor(est.log_scale, dtype=torch.float32)).item())
            pf = 1.0 / (s * np.sqrt(2 * np.pi)) if est.family == "gauss" else 1.0 / (4.0 * s)
            p *= max(1.0, pf)
    return p


def oracle_raw(ora, target, ev, N, seed=None):
    """(raw rows, raw max) of the oracle; Python's ``random`` state (the
    oversampled domains' draws) is left as found."""
    state = random.getstate()
    try:
        if seed is not None:
            random.seed(seed)
        with np.errstate(all="ignore"):
            raw, _ = ora.infer_raw(target, ev, N)
    finally:
        random.setstate(state)
    with np.errstate(invalid="ignore"):
        return raw, float(raw.max())


def oracle_reference(ora, target, ev, N, norm_row=None):
    """One oracle pass (Python's ``random`` is consumed as ``ora.infer`` would):
    (max-normalised marginals, sample domain, the helper's keyword arguments
    ``raw_max`` / ``n_factors`` / ``peak`` read from that same pass).
    ``norm_row``: normalise by that row's max (a sample of a larger batch
    whose argmax row it is) instead of the max of all the rows."""
    raw, dom = ora.infer_raw(target, ev, N)
    mx = raw.max() if norm_row is None else raw[norm_row].max()
    ref = (raw / mx).astype(np.float32)
    return ref, dom, dict(raw_max=float(mx), n_factors=n_factors(ora, target), peak=peak(ora, target))


def _golden_oracle(name, param):
    from golden_io import load_golden, load_param_golden, oracle_estimators
    from oracle.ref_infer import OracleBN

    g = load_param_golden(name) if param else load_golden(name)
    m = g["meta"]
    return g, OracleBN(m["edges"], m["columns"], g["data"], estimators=oracle_estimators(g) if param else None)


@functools.lru_cache(maxsize=None)
def golden_raw(name, param=False):
    """The oracle's unnormalised rows for a reference golden that ran without
    error, computed once per session and shared (read-only).  Up to 25 s of
    CPU for a few fixtures: the GPU tests call it for the NaN fixtures only
    and take every other fixture's raw max from ``golden_scale``."""
    g, ora = _golden_oracle(name, param)
    m = g["meta"]
    ev = None if m.get("evidence_none") else {k: g["evidence"][k] for k in m["evidence"]}
    raw, _ = oracle_raw(ora, m["target"], ev, m["N_max"], seed=m["seed"])
    raw.setflags(write=False)
    return raw


# all-zero rows by construction (off-domain evidence, sparse high-cardinality
# CPDs): the share of rows with an entry the relative term governs, measured on
# the fixture itself (rows with a nonzero entry: 0.406, 0.396, 0.575), less a hair
MIN_CHECKED_ROWS = {"hicard40_all": 0.40, "cont4_all": 0.39}


@functools.lru_cache(maxsize=None)
def golden_scale(name, param=False):
    """(raw_max, n_factors, peak) of a reference golden without running the
    oracle: the raw max is the oracle's, recorded in
    tests/golden/oracle_raw_max.json (tests/golden/make_oracle_raw_max.py) and
    pinned to the oracle's own run by tests/test_oracle_golden.py."""
    import json
    import os

    from golden_io import GOLDEN_DIR

    g, ora = _golden_oracle(name, param)
    with open(os.path.join(GOLDEN_DIR, "oracle_raw_max.json")) as f:
        mx = float.fromhex(json.load(f)[name])
    t = g["meta"]["target"]
    return mx, n_factors(ora, t), peak(ora, t)


def engine_raw_rows(bn, name, ev, param=False):
    """The engine's unnormalised rows (``engine.infer_raw``: the raw launch)
    for a golden that is NaN by design, drawn with the fixture's seed; None
    for every other golden (their normalised rows carry the values)."""
    from golden_io import load_golden, load_param_golden

    g = load_param_golden(name) if param else load_golden(name)
    if not np.isnan(g["pdf"]).any():
        return None
    import torch

    m = g["meta"]
    eng = bn.engine
    random.seed(m["seed"])
    # as sharded_infer takes it: the call's plan with its sample-domain draws
    # made (N_max above a domain's size: redrawn per call), then the raw launch
    plan, fp = eng.call_plan(m["target"], ev, m["N_max"])
    try:
        if fp is None:  # a plan rebuilt per call (redrawn parametric plans): its own fast path, for this call
            from continuousbayesiannetwork_amd import _native
            from continuousbayesiannetwork_amd.inference.engine import _FastPath

            fp = _FastPath(plan, _native.require_gpu(bn.device), next(iter(ev)))
        res = eng.infer_raw(m["target"], ev, m["N_max"], fp=fp)
        assert res is not None, f"{name}: the plan takes no raw launch"
        return res[0].cpu().numpy()
    finally:
        if not plan.deterministic and not plan.reusable:  # a plan rebuilt per call
            torch.cuda.current_stream().synchronize()
            plan.destroy()


def assert_golden_close(got, name, param=False, got_raw=None, **kw):
    """``got`` vs the reference golden ``name``'s pdf through the helper; the
    fixtures that are NaN in every entry compare NaN positions and the
    unnormalised rows (``got_raw``) with the oracle's."""
    from golden_io import load_golden, load_param_golden

    g = load_param_golden(name) if param else load_golden(name)
    ref = g["pdf"]
    mx, nf, pk = golden_scale(name, param)
    if np.isnan(ref).any():
        assert got_raw is not None, f"{name}: a NaN fixture needs the unnormalised rows"
        # (the reference's own unnormalised rows where the fixture holds them, else the oracle's)
        assert_marginals_close(got, ref, raw_max=mx, n_factors=nf, peak=pk, nan="match", got_raw=got_raw,
                               ref_raw=g["raw"] if "raw" in g else golden_raw(name, param), **kw)
    else:
        kw.setdefault("min_checked_rows", MIN_CHECKED_ROWS.get(name, 0.5))
        assert_marginals_close(got, ref, raw_max=mx, n_factors=nf, peak=pk, **kw)
