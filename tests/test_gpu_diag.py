"""Diagnostic kernel-selection switches stay out of the serving path
(VERDICT r04 weak 7): they count only when libcbn_amd.so is loaded with
CBN_DIAG=1.  Each case runs tests/diag_child.py in a child process started
with the environment under test (one child at a time)."""
import json
import os
import subprocess
import sys

import pytest

from continuousbayesiannetwork_amd import _native

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _child(mode: str, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("CBN_")}
    e.update(env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "diag_child.py"), mode], env=e, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_no_staged_ignored_without_cbn_diag(gpu):
    """CBN_NO_STAGED=1 alone leaves the configs[1] plan on k_query_staged;
    with CBN_DIAG=1 it takes effect and the override is listed on stderr."""
    base, _ = _child("flags")
    stray, err = _child("flags", CBN_NO_STAGED="1")
    assert stray["diag"] == 0 and "diagnostic override" not in err
    assert stray["flags"] == base["flags"] and all(f & _native.CBN_PLAN_STAGED for f in base["flags"])
    diag, err = _child("flags", CBN_DIAG="1", CBN_NO_STAGED="1")
    assert diag["diag"] == 1 and "diagnostic override CBN_NO_STAGED=1" in err
    assert not any(f & _native.CBN_PLAN_STAGED for f in diag["flags"])


def test_generic_kernel_equals_fast_kernel(gpu):
    """The generic parametric kernel (CBN_PARAM_GENERIC, under CBN_DIAG=1)
    runs the fast kernels' operations in the same order: bit-identical rows
    on an NN [16] network with free parents (moved here from
    test_gpu_param.py: the switch is read at plan creation, the gate at load)."""
    res, _ = _child("generic", CBN_DIAG="1")
    assert res["diag"] == 1 and res["equal"] and res["finite"] > 0


def test_grid_bench_batch_slots_equals_fast_kernel(gpu):
    """configs[4] at its benchmarked size (tools/bench_grid.py's headline
    batch: 100 factors, L = 8, 65 536 queries -- k_query_slots' fused
    two-round launch with a 3-chunk phase-B survivor chain) == k_query_fast
    (CBN_NO_SLOTS=1 under CBN_DIAG=1) bit for bit."""
    res, _ = _child("gridfull", CBN_DIAG="1")
    assert res["diag"] == 1 and res["equal"] and res["nonzero_rows"] > 1000
    assert res["flags"][0] & _native.CBN_PLAN_SLOTS and not res["flags"][1] & _native.CBN_PLAN_SLOTS


def test_grid_coalesced_index_phase_equals_per_lane(gpu, tmp_path):
    """k_query_slots' coalesced index phase (round 6: 16-B evidence loads per
    (slot, 4 queries), taken by launches of >= 3 block rounds) == the per-lane
    index phase (CBN_SLOTS_NO_COAL=1 under CBN_DIAG=1) bit for bit on a
    200 003-query grid batch (the raw launch + scale path, ragged last
    round), and == the same batch through 4-B-offset column views (the
    coalesced phase declines unaligned columns); 42 rows vs the oracle."""
    import random

    import numpy as np

    from helpers import grid_data, sample_evidence
    from oracle.ref_infer import OracleBN

    outp = str(tmp_path / "rows.npy")
    res, _ = _child("gridcoal", CBN_DIAG="1", CBN_CHILD_OUT=outp)
    assert res["diag"] == 1 and res["equal"] and res["equal_unaligned"] and res["nonzero_rows"] > 1000
    assert all(f & _native.CBN_PLAN_SLOTS for f in res["flags"])
    data, cols, edges = grid_data(100000, 7, side=5, d=64, keep=0.995, noise=0)
    target, names = cols[-1], cols[:-1]
    ev = sample_evidence(data, cols, names, 200003, 3)
    rows = np.asarray(res["rows"])
    random.seed(0)
    from parity import assert_marginals_close, oracle_reference

    ref, _, kw = oracle_reference(OracleBN(edges, cols, data), target, {k: v[rows] for k, v in ev.items()}, 64)
    got = np.load(outp)
    assert_marginals_close(got / got.max(), ref, **kw)


def test_special_evidence_through_coalesced_index_phase(gpu, tmp_path):
    """Special evidence values (NaN, +-inf, -0.0, ... tests/helpers.py
    special_batch) through k_query_slots' coalesced index phase -- 16-B
    evidence loads, two int16 indices packed per word -- forced at 1 001
    queries (not a multiple of 4: the tail masking) by CBN_SLOTS_COAL=1 under
    CBN_DIAG=1: bit for bit the per-lane phase's rows (normalised and raw),
    for dense and for sorted non-integer domains; every row whose special
    value == no domain entry is exactly zero, and -0.0 rows equal +0.0 rows."""
    import numpy as np

    from helpers import grid_data, sample_evidence, special_batch

    outp = str(tmp_path / "rows.npz")
    res, _ = _child("coalspecial", CBN_DIAG="1", CBN_CHILD_OUT=outp)  # (the child sets CBN_SLOTS_COAL per launch)
    assert res["diag"] == 1
    assert res["equal"] == [True, True] and res["equal_raw"] == [True, True]
    assert len(res["flags"]) == 2 and all(f & _native.CBN_PLAN_SLOTS for f in res["flags"])
    base, cols, edges = grid_data(100000, 7, side=3, d=64, keep=0.995, noise=0)
    z = np.load(outp)
    for tag in ("dense", "levels"):
        data = base if tag == "dense" else ((np.arange(64) - 2) * 0.25).astype(np.float32)[base.astype(np.int64)]
        doms = {c: np.unique(data[:, cols.index(c)]) for c in cols[:-1]}
        ev, rows = special_batch(sample_evidence(data, cols, cols[:-1], 1001, 5), doms)
        p = z[tag]
        off = [r[0] for r in rows if not r[4]]
        assert p.shape == (1001, 64) and p.max() == 1.0 and len(off) >= 17 * 8 and (p[off] == 0).all()
        for c in cols[:-1]:
            r_neg, r_pos = (next(r[0] for r in rows if r[1] == c and r[2] == k) for k in (4, 5))
            np.testing.assert_array_equal(p[r_neg].view(np.uint32), p[r_pos].view(np.uint32))
        assert any((p[r[0]] > 0).any() for r in rows if r[4])


def _info(nc, hmax, mode, m1, parts, N=40):
    return {"nc": nc, "n_chunks": -(-N // nc), "hmax": hmax, "mode": mode, "m1": m1, "parts": parts}


def test_linear_param_rows_do_not_depend_on_chunk_width_or_m1_form(gpu):
    """One LinearRegression plan (sigma = 0.5, 8 factors, N = 40, all
    evidence; tests/param_matrix.py) under CBN_DIAG=1: the 16-column kernel
    and the 8-column one (CBN_PARAM_LIN8) give bit-identical raw rows at 4
    parts, and at 2 parts (CBN_PARAM_PARTS=2) so do both and the
    M1 = false kernel (CBN_PARAM_NO_M1) -- a column's arithmetic does not
    depend on its chunk, and lin4's zero-padded fma chain is model_mu<0>'s
    (cbn_param.hip: fma(0, 0, s) == s), with mul_row_t behind both.  A linear
    plan has no 32-column instantiation, and CBN_PARAM_NC does not reach it.
    Rows are not compared across `parts`: the product's association differs
    by design."""
    res, _ = _child("paramlin", CBN_DIAG="1")
    assert res["diag"] == 1
    assert res["infos"] == [_info(16, 0, 1, 1, 4), _info(8, 0, 1, 1, 4),
                            _info(16, 0, 1, 1, 2), _info(8, 0, 1, 1, 2), _info(8, 0, 1, 0, 2)]
    assert res["equal"] == [True] * 5 and res["finite"] == [True] * 5


def test_mlp_param_rows_do_not_depend_on_chunk_width_or_m1_form(gpu):
    """One NN [16] tanh plan (scale 0.5, 9 factors, N = 40, all evidence)
    under CBN_DIAG=1: CBN_PARAM_NC = 32, 16 and 8 (2, 3 and 5 chunks) give
    bit-identical raw rows at the plan's 4 parts; at 2 parts the M1 kernel,
    the M1 = false one (CBN_PARAM_NO_M1: both evaluate the pair-packed
    mlp1p forms and mul_row_t) and the latter at 16 columns do too."""
    res, _ = _child("paramh1", CBN_DIAG="1")
    assert res["diag"] == 1
    assert res["infos"] == [_info(32, 1, 3, 1, 4), _info(16, 1, 3, 1, 4), _info(8, 1, 3, 1, 4),
                            _info(32, 1, 3, 1, 2), _info(32, 1, 3, 0, 2), _info(16, 1, 3, 0, 2)]
    assert res["equal"] == [True] * 6 and res["finite"] == [True] * 6
