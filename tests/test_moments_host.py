"""Host-side checks of ``posterior`` / ``expect`` that need no GPU: the C ABI's
argument validation, the native host path's rejections, the public signatures,
the ``moments_ref`` helper itself, and that the oracle inputs of
tests/test_gpu_moments.py meet the helper's 90 % rule."""
import inspect
import os
import random

import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from continuousbayesiannetwork_amd.inference.engine import InferenceEngine
from helpers import chain_data, sample_evidence
from moments_ref import MIN_MASS, U, assert_moments, mean_tolerance, moments_f64
from oracle.ref_infer import OracleBN


def test_c_abi_rejects_null_arguments():
    lib = _native.load()
    # (every pointer below is NULL: nothing can be dereferenced, no device is touched)
    assert lib.cbn_row_moments(None, 4, 8, None, 0, None, None, None, None) == _native.CBN_E_ARG
    assert lib.cbn_row_moments(None, -1, 8, None, 0, None, None, None, None) == _native.CBN_E_ARG
    assert lib.cbn_row_moments(None, 4, 0, None, 1, None, None, None, None) == _native.CBN_E_ARG
    assert lib.cbn_plan_run_moments(None, 4, None, 0, None, None, None, None, None, None, 0, None) == _native.CBN_E_ARG
    assert b"null plan" in lib.cbn_last_error()
    assert lib.cbn_plan_moments_scratch(None, 4) == 0


def test_flag_value_and_abi_version():
    assert _native.CBN_PLAN_MOMENTS == 2048
    assert _native.load().cbn_abi_version() == 6 == _native.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cbn_amd.h")).read()
    assert "#define CBN_PLAN_MOMENTS 2048" in header


def test_run_moments_returns_none_for_what_it_cannot_take():
    host = _native.load_host()
    cpu = {"A": torch.zeros(4, 1), "B": torch.zeros(4, 1)}
    slots = ("A", "B")
    # CPU tensors, a missing key, an empty column: None before any library call (fn = plan = 0)
    for rows in (True, False):
        assert host.run_moments(0, 0, cpu, slots, "A", 0, 8, True, 0, rows, 0, 0) is None
        assert host.run_moments(0, 0, {"A": cpu["A"]}, slots, "A", 0, 8, True, 0, rows, 0, 0) is None
        assert host.run_moments(0, 0, {"A": torch.zeros(0, 1), "B": torch.zeros(0, 1)}, slots, "A", 0, 8, True, 0, rows,
                                0, 0) is None


def test_public_signatures():
    p = inspect.signature(InferenceEngine.posterior).parameters
    assert list(p) == ["self", "target", "evidence", "N_max", "rows"] and p["rows"].default is True
    p = inspect.signature(BayesianNetwork.posterior).parameters
    assert list(p) == ["self", "target_node", "evidence", "N_max"]
    assert (p["evidence"].default, p["N_max"].default) == (None, 16)
    p = inspect.signature(BayesianNetwork.expect).parameters
    assert list(p) == ["self", "target_node", "evidence", "N_max", "moments"]
    assert (p["evidence"].default, p["N_max"].default, p["moments"].default) == (None, 16, False)
    p = inspect.signature(BayesianNetwork.expect_df).parameters
    assert list(p) == ["self", "data", "target_feature", "batch_size", "N_max"]
    assert (p["batch_size"].default, p["N_max"].default) == (128, 16)


def test_moments_f64():
    s = np.array([1.0, 2.0, 4.0, 8.0])
    raw = np.array([[1.0, 1.0, 0.0, 2.0], [0.0, 0.0, 3.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    with np.errstate(all="ignore"):
        mass, mean, var, pdf = moments_f64(raw, s[None, :])
    np.testing.assert_array_equal(mass, [4.0, 3.0, 0.0])
    np.testing.assert_array_equal(mean[:2], [19.0 / 4, 4.0])
    np.testing.assert_allclose(var[:2], [(3.75 ** 2 + 2.75 ** 2 + 2 * 3.25 ** 2) / 4, 0.0], rtol=1e-15)
    np.testing.assert_array_equal(pdf[0], [0.25, 0.25, 0.0, 0.5])
    assert np.isnan(mean[2]) and np.isnan(var[2]) and np.isnan(pdf[2]).all()


def _case(Q=40, N=16, seed=0):
    rng = np.random.default_rng(seed)
    raw = rng.random((Q, N)).astype(np.float32) * np.float32(1e-6)
    s = np.sort(rng.normal(0, 3, N)).astype(np.float32)
    return raw, s


def test_assert_moments_accepts_float32_sums_and_rejects_errors_beyond_the_bounds():
    raw, s = _case()
    N = raw.shape[1]
    # a float32 evaluation in another order than numpy's float64: inside the own-row bounds
    m32 = raw[:, ::-1].sum(1, dtype=np.float32)
    mean32 = (raw * s).sum(1, dtype=np.float32) / m32
    var32 = (raw * (s - mean32[:, None]) ** 2).sum(1, dtype=np.float32) / m32
    assert assert_moments(m32, mean32, var32, raw, s, own=True) == 1.0
    assert assert_moments(m32, mean32, var32, raw, s, own=False) == 1.0
    mass, mean, var, _ = moments_f64(raw, s)
    tm = mean_tolerance(raw, s, own=True)
    with pytest.raises(AssertionError, match="mass"):
        assert_moments(mass * (1 + 3 * N * U), mean, var, raw, s, own=True)
    assert_moments(mass * (1 + 3 * N * U), mean, var, raw, s, own=False)  # (inside the oracle bound's 1e-5)
    with pytest.raises(AssertionError, match="mass"):
        assert_moments(mass * (1 + 2e-5), mean, var, raw, s, own=False)
    with pytest.raises(AssertionError, match="mean"):
        assert_moments(mass, mean + 1.5 * tm, var, raw, s, own=True)
    assert_moments(mass, mean + 0.9 * tm, var, raw, s, own=True)
    with pytest.raises(AssertionError, match="var"):
        assert_moments(mass, mean, var * (1 + 3 * (2 * N + 8) * U) + 2 * tm ** 2, raw, s, own=True)
    with pytest.raises(AssertionError, match="var"):
        assert_moments(mass, mean, var * (1 + 5e-5), raw, s, own=False)
    # the naive E[s^2] - mean^2 in float32 on a narrow peak far from 0 is what the variance bound excludes
    far = (s + np.float32(1000.0)).astype(np.float32)
    peak = np.zeros((20, N), np.float32)
    peak[:, 3], peak[:, 4] = 0.5, 0.5
    pm = peak.sum(1, dtype=np.float32)
    pmean = (peak * far).sum(1, dtype=np.float32) / pm
    naive = (peak * far * far).sum(1, dtype=np.float32) / pm - pmean * pmean
    with pytest.raises(AssertionError, match="var"):
        assert_moments(pm, pmean, naive, peak, far, own=True)
    centred = (peak * (far - pmean[:, None]) ** 2).sum(1, dtype=np.float32) / pm
    assert_moments(pm, pmean, centred, peak, far, own=True)


def test_assert_moments_zero_mass_rows_and_the_refusal():
    raw, s = _case(Q=40)
    raw[5] = 0
    raw[7] = np.float32(1e-33)  # mass < 1e-30: mass compared, mean / var not
    with np.errstate(all="ignore"):
        mass, mean, var, _ = moments_f64(raw, s)
    assert np.isnan(mean[5]) and mass[7] < MIN_MASS
    share = assert_moments(mass, mean, var, raw, s, own=True)
    assert share == 38 / 40
    junk = mean.copy()
    junk[7] += 1.0
    assert_moments(mass, junk, var, raw, s, own=True)
    bad = mean.copy()
    bad[5] = 0.0  # a number where the reference has NaN
    with pytest.raises(AssertionError, match="NaN"):
        assert_moments(mass, bad, var, raw, s, own=True)
    bad = mean.copy()
    bad[3] = np.nan  # NaN where the reference has a number
    with pytest.raises(AssertionError, match="NaN"):
        assert_moments(mass, bad, var, raw, s, own=True)
    bad = mass.copy()
    bad[5] = 1e-40
    with pytest.raises(AssertionError, match="mass"):
        assert_moments(bad, mean, var, raw, s, own=True)
    # fewer than 90 % of the rows at mass >= 1e-30: refused
    raw[10:14] = 0
    with np.errstate(all="ignore"):
        mass, mean, var, _ = moments_f64(raw, s)
    with pytest.raises(AssertionError, match="vacuous"):
        assert_moments(mass, mean, var, raw, s, own=True)
    with pytest.raises(AssertionError, match="vacuous"):
        assert_moments(mass[:0], mean[:0], var[:0], raw[:0], s, own=True)
    with pytest.raises(AssertionError, match="finite"):
        assert_moments(mass, mean, var, np.where(raw == 0, np.nan, raw), s, own=True)


@pytest.mark.parametrize("n,d,S,seed,Q,ev_seed", [(6, 32, 60000, 8, 257, 40)] + [
    (5, N, 30000, 20 + N, 65 if N < 64 else 64, 9) for N in (4, 8, 12, 16, 20, 24, 64)])
def test_oracle_inputs_of_the_gpu_tests_meet_the_mass_rule(n, d, S, seed, Q, ev_seed):
    """The chains tests/test_gpu_moments.py compares through the oracle: at
    least 90 % of the rows have mass >= 1e-30 (here: all of them), so
    assert_moments does not refuse them, and the means are spread over the
    domain (a constant mean would check little)."""
    data, cols, edges = chain_data(n, d, S, seed, stay=0.8)
    ev = sample_evidence(data, cols, cols[:-1], Q, ev_seed)
    random.seed(0)
    raw, dom = OracleBN(edges, cols, data).infer_raw(cols[-1], ev, d)
    mass, mean, var, _ = moments_f64(raw, dom)
    assert (mass >= MIN_MASS).all()
    assert assert_moments(mass, mean, var, raw, dom, own=False) == 1.0
    if Q > 1:
        assert mean.max() - mean.min() > 0.25 * (d - 1) and (var > 0).all()
