"""Host-side checks of ``quantile`` / ``interval`` / ``sample`` that need no
GPU: the C ABI's argument validation, the native host path's rejections, the
public signatures, the ``quantile_ref`` helper itself, and that the oracle
inputs of tests/test_gpu_quantile.py meet the helper's 90 % rule."""
import inspect
import os
import random

import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from continuousbayesiannetwork_amd.inference.engine import InferenceEngine
from helpers import chain_data, sample_evidence
from oracle.ref_infer import OracleBN
from quantile_ref import U, acceptable, assert_quantile, decided_share, midpoint_probs, quantile_f64

FIXED = [0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0]  # (tests/test_gpu_quantile.py's shared probabilities)


def test_c_abi_rejects_null_and_bad_arguments():
    lib = _native.load()
    E = _native.CBN_E_ARG
    # (8 stands for any non-NULL address: every call fails its argument checks before a pointer is
    # dereferenced or a device is touched)
    assert lib.cbn_plan_run_quantile(None, 4, None, 0, None, 8, 1, 0, 8, None, None, None, 0, None) == E
    assert b"null plan" in lib.cbn_last_error()
    assert lib.cbn_row_quantile(None, 4, 8, None, 8, 1, 0, 8, None, None, None) == E   # null rows
    assert lib.cbn_row_quantile(8, 4, 8, None, None, 1, 0, 8, None, None, None) == E   # null probs
    assert lib.cbn_row_quantile(8, 4, 8, None, 8, 1, 0, None, None, None, None) == E   # null index
    assert lib.cbn_row_quantile(8, 4, 8, None, 8, 0, 0, 8, None, None, None) == E      # n_probs < 1
    assert lib.cbn_row_quantile(8, 4, 8, None, 8, 3, 2, 8, None, None, None) == E      # 0 < probs_stride < n_probs
    assert lib.cbn_row_quantile(8, 4, 8, None, 8, 3, -1, 8, None, None, None) == E
    assert lib.cbn_row_quantile(8, 4, 0, None, 8, 1, 0, 8, None, None, None) == E      # n_cols < 1
    assert lib.cbn_row_quantile(8, -1, 8, None, 8, 1, 0, 8, None, None, None) == E
    assert lib.cbn_row_quantile(None, 0, 8, None, 8, 1, 0, 8, None, None, None) == 0   # no rows: nothing to do
    assert lib.cbn_plan_quantile_scratch(None, 4, 1) == 0
    assert lib.cbn_plan_quantile_scratch(None, 4, 17) == 0


def test_flag_values_and_abi_version():
    assert _native.CBN_PLAN_QUANTILE == 4096 and _native.CBN_MAX_QUANTILES == 16
    assert _native.load().cbn_abi_version() == 6 == _native.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cbn_amd.h")).read()
    assert "#define CBN_PLAN_QUANTILE 4096" in header and "#define CBN_MAX_QUANTILES 16" in header


def test_run_quantile_returns_none_for_what_it_cannot_take():
    host = _native.load_host()
    cpu = {"A": torch.zeros(4, 1), "B": torch.zeros(4, 1)}
    slots = ("A", "B")
    probs = torch.tensor([0.5])
    # CPU tensors, a missing key, an empty column: None before any library call (fn = plan = 0)
    assert host.run_quantile(0, 0, cpu, slots, "A", 0, True, 0, probs, 0, 0) is None
    assert host.run_quantile(0, 0, {"A": cpu["A"]}, slots, "A", 0, True, 0, probs, 0, 0) is None
    assert host.run_quantile(0, 0, {"A": torch.zeros(0, 1), "B": torch.zeros(0, 1)}, slots, "A", 0, True, 0, probs, 0,
                             0) is None


def test_public_signatures():
    p = inspect.signature(InferenceEngine.quantile).parameters
    assert list(p) == ["self", "target", "evidence", "N_max", "probs"]
    p = inspect.signature(BayesianNetwork.quantile).parameters
    assert list(p) == ["self", "target_node", "evidence", "probs", "N_max", "return_index"]
    assert (p["evidence"].default, p["probs"].default, p["N_max"].default, p["return_index"].default) == \
        (None, (0.5,), 16, False)
    p = inspect.signature(BayesianNetwork.interval).parameters
    assert list(p) == ["self", "target_node", "evidence", "level", "N_max"]
    assert (p["evidence"].default, p["level"].default, p["N_max"].default) == (None, 0.95, 16)
    p = inspect.signature(BayesianNetwork.sample).parameters
    assert list(p) == ["self", "target_node", "evidence", "n_samples", "N_max", "generator", "return_index"]
    assert (p["evidence"].default, p["n_samples"].default, p["N_max"].default, p["generator"].default,
            p["return_index"].default) == (None, 1, 16, None, False)
    assert "quantile" in _native.load_host().run_quantile.__name__


def test_host_probabilities_are_range_checked():
    dev = torch.device("cpu")
    for bad in ([0.5, 1.5], [-0.1], [float("nan")], torch.tensor([[0.2, 2.0]]), torch.tensor([0.5, float("nan")])):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            InferenceEngine._probs(bad, dev)
    with pytest.raises(ValueError, match="probs must be"):
        InferenceEngine._probs(torch.zeros(2, 2, 2), dev)
    with pytest.raises(ValueError, match="probs must be"):
        InferenceEngine._probs([], dev)
    t = InferenceEngine._probs((0.0, 0.5, 1.0), dev)
    assert t.dtype is torch.float32 and t.shape == (3,) and t.is_contiguous()
    t = InferenceEngine._probs(torch.tensor([[0.25, 0.5]], dtype=torch.float64), dev)
    assert t.dtype is torch.float32 and t.shape == (1, 2)
    assert InferenceEngine._probs(0.5, dev).shape == (1,)


# ------------------------------------------------------------- the helper --
def test_quantile_f64_on_hand_made_rows():
    raw = np.array([[0.0, 1.0, 0.0, 1.0, 2.0, 0.0],    # leading / trailing zeros, a flat cdf segment at column 2
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],    # mass 0
                    [4.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    p = [0.0, 0.25, 0.25 + 1e-9, 0.5, 0.5 + 1e-9, 1.0, float("nan"), 1.5, -0.5]
    idx, mass = quantile_f64(raw, p)
    np.testing.assert_array_equal(mass, [4.0, 0.0, 4.0])
    # p = 0: the first supported column; p on a boundary: that column; just above: the next SUPPORTED one
    np.testing.assert_array_equal(idx[0], [1, 1, 3, 3, 4, 4, -1, -1, -1])
    np.testing.assert_array_equal(idx[1], [-1] * 9)
    np.testing.assert_array_equal(idx[2], [0, 0, 0, 0, 0, 0, -1, -1, -1])
    # per-row probabilities
    idx2, _ = quantile_f64(raw, np.array([[0.9], [0.9], [0.9]]))
    np.testing.assert_array_equal(idx2[:, 0], [4, -1, 0])


def test_acceptable_sets_and_assert_quantile():
    N = 6
    raw = np.array([[0.0, 1.0, 0.0, 1.0, 2.0, 0.0]] * 12)
    p = np.array([0.0, 0.1, 0.25, 0.3, 0.5, 0.6, 0.9, 1.0, 0.2, 0.4, 0.7, 0.8])
    acc = acceptable(raw, p)
    # on a boundary (p = 0.25, 0.5) both neighbours of positive probability are acceptable, never a zero column
    np.testing.assert_array_equal(np.flatnonzero(acc[0, 2]), [1, 3])
    np.testing.assert_array_equal(np.flatnonzero(acc[0, 4]), [3, 4])
    for k, want in ((0, 1), (1, 1), (3, 3), (5, 4), (6, 4), (7, 4)):
        np.testing.assert_array_equal(np.flatnonzero(acc[0, k]), [want])
    assert decided_share(raw, p) == 10 / 12
    exact, _ = quantile_f64(raw, p)
    with pytest.raises(AssertionError, match="vacuous"):
        assert_quantile(exact, raw, p)  # (10 of 12 decided: below 90 %)
    p = np.array([0.0, 0.1, 0.3, 0.6, 0.9, 1.0, 0.2, 0.4, 0.7, 0.8, 0.25])
    exact, _ = quantile_f64(raw[:1], p)
    decided = assert_quantile(exact, raw[:1], p)
    assert decided.sum() == 10 and not decided[0, 10]
    other = exact.copy()
    other[0, 10] = 3  # the other side of the boundary
    assert_quantile(other, raw[:1], p)
    for col in (0, 2, 4, 5):  # zero-probability columns and a column beyond the step
        wrong = exact.copy()
        wrong[0, 10] = col
        with pytest.raises(AssertionError, match="not acceptable"):
            assert_quantile(wrong, raw[:1], p)
    wrong = exact.copy()
    wrong[0, 2] = 4  # p = 0.3 -> column 3, decided
    with pytest.raises(AssertionError, match="not acceptable"):
        assert_quantile(wrong, raw[:1], p)
    wrong = exact.copy()
    wrong[0, 0] = -1
    with pytest.raises(AssertionError, match="out of range"):
        assert_quantile(wrong, raw[:1], p)
    # delta scales with extra: 0.2501 is decided at extra = 0 and not at extra = 1e-3
    assert acceptable(raw[:1], [0.2501]).sum() == 1 and acceptable(raw[:1], [0.2501], extra=1e-3).sum() == 2
    assert 4 * N * U * 4.0 < 1e-4  # (the delta of these rows is far below the margins used above)


def test_assert_quantile_mass_zero_rows_and_bad_p():
    raw = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    p = [0.1, 0.6, float("nan"), 2.0]
    exact, _ = quantile_f64(raw, p)
    np.testing.assert_array_equal(exact, [[0, 1, -1, -1], [-1] * 4, [1, 1, -1, -1]])
    assert_quantile(exact, raw, p)
    for q, k in ((1, 0), (0, 2), (2, 3)):
        wrong = exact.copy()
        wrong[q, k] = 1  # a column where -1 is due
        with pytest.raises(AssertionError, match="not -1"):
            assert_quantile(wrong, raw, p)
    with pytest.raises(AssertionError, match="vacuous"):
        assert_quantile(exact[1:2], raw[1:2], p)
    with pytest.raises(AssertionError, match="finite"):
        assert_quantile(exact, np.where(raw == 0, np.nan, raw), p)


def test_midpoint_probs_are_decided_by_construction():
    rng = np.random.default_rng(3)
    raw = (rng.random((50, 32)) ** 6).astype(np.float32)
    raw[rng.random(raw.shape) < 0.3] = 0
    raw[7] = 0
    for extra in (0.0, 1e-5):
        mp = midpoint_probs(raw, extra)
        assert mp.dtype == np.float32 and mp.shape == raw.shape
        idx, _ = quantile_f64(raw, mp)
        given = ~np.isnan(mp)
        assert given.sum() > 0.5 * (raw > 0).sum() and not given[7].any() and not given[raw == 0].any()
        want = np.broadcast_to(np.arange(32), raw.shape)
        np.testing.assert_array_equal(idx[given], want[given])
        assert (idx[~given] == -1).all()
        assert (acceptable(raw, mp, extra).sum(2) == 1)[given].all()
        assert decided_share(raw, mp, extra) == 1.0
    assert (~np.isnan(midpoint_probs(raw, 1e-5))).sum() < (~np.isnan(midpoint_probs(raw))).sum()


def _all_probs(raw, extra=0.0):
    return np.concatenate([np.broadcast_to(np.float32(FIXED), (raw.shape[0], 7)), midpoint_probs(raw, extra)], 1)


def test_a_float32_scan_in_any_association_is_accepted_and_a_register_order_scan_is_not():
    rng = np.random.default_rng(5)
    raw = (rng.random((300, 32)) ** 3 * 1e-7).astype(np.float32)
    raw[rng.random(raw.shape) < 0.2] = 0
    probs = _all_probs(raw)

    def scan32(rows, order):
        """index by the rule from a float32 sequential scan over the columns taken in `order`"""
        c = np.zeros(rows.shape, np.float32)
        run = np.zeros(rows.shape[0], np.float32)
        for j in order:
            run = (run + rows[:, j]).astype(np.float32)
            c[:, j] = run
        t = (probs * run[:, None]).astype(np.float32)
        with np.errstate(invalid="ignore"):
            ok = (rows > 0)[:, None, :] & (c[:, None, :] >= t[:, :, None])
        first = np.where(ok.any(2), ok.argmax(2), -1)
        last = 31 - (rows > 0)[:, ::-1].argmax(1)
        return np.where(np.isnan(probs), -1, np.where(first >= 0, first, last[:, None]))

    assert_quantile(scan32(raw, range(32)), raw, probs)
    # the paired layouts' register order: the lane's two blocks swapped (columns 16.. before 0..15)
    swapped = scan32(raw, list(range(16, 32)) + list(range(16)))
    with pytest.raises(AssertionError, match="not acceptable"):
        assert_quantile(swapped, raw, probs)


@pytest.mark.parametrize("n,d,S,seed,Q,ev_seed", [(6, 32, 60000, 8, 257, 40)] + [
    (5, N, 30000, 20 + N, 65 if N < 64 else 64, 9) for N in (4, 8, 12, 16, 20, 24, 64)])
def test_oracle_inputs_of_the_gpu_tests_meet_the_decided_rule(n, d, S, seed, Q, ev_seed):
    """The chains tests/test_gpu_quantile.py checks, with its probabilities (the
    shared list and the per-row decided midpoints, in one comparison): at
    least 90 % of the entries have exactly one acceptable index at each
    ``extra`` the tests use, so assert_quantile does not refuse them; every
    column is the decided midpoint of some row; the medians are spread over
    the domain."""
    data, cols, edges = chain_data(n, d, S, seed, stay=0.8)
    ev = sample_evidence(data, cols, cols[:-1], Q, ev_seed)
    random.seed(0)
    raw, _ = OracleBN(edges, cols, data).infer_raw(cols[-1], ev, d)
    assert (raw.sum(1) > 0).all()
    for extra in (0.0, 2 * U, 1e-5):
        probs = _all_probs(raw, extra)
        assert decided_share(raw, probs, extra) >= 0.9
        # the list's own floor (quantile_ref's docstring): all but p = 1 pass the cap without the midpoints
        assert decided_share(raw, FIXED[:6], extra) >= 0.9
        idx, _ = quantile_f64(raw, probs)
        assert_quantile(idx, raw, probs, extra)
    assert (~np.isnan(midpoint_probs(raw))).any(0).all()
    idx, _ = quantile_f64(raw, FIXED)
    assert (np.diff(idx, axis=1) >= 0).all()
    if Q > 1:
        assert len(np.unique(idx[:, 3])) >= min(d, 4)


def test_row_kernel_inputs_of_the_gpu_test_meet_the_decided_rule():
    """test_row_quantile_kernel's hand-made rows, with each set of probabilities it compares."""
    import test_gpu_quantile as T

    for n_cols in T.ROW_COLS:
        raw, _ = T.row_case(n_cols)
        mp = midpoint_probs(raw)
        for c in range(0, min(n_cols, 80), 16):
            probs = np.concatenate([np.broadcast_to(np.float32(FIXED), (501, 7)), mp[:, c:c + 16]], 1)
            assert decided_share(raw, probs) >= 0.9, (n_cols, c)
