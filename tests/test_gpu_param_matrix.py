"""Every instantiation of the parametric query kernels, at the smallest shapes
that reach it, against the CPU oracle.

``cbn_plan_create_param`` and ``param_select`` (csrc/cbn_param.hip) choose one
of 31 instantiations of ``k_param_query<NC, HMAX, MODE, TAB, M1>``, or
``k_param_query_gen``, and the launch shape.  ``cbn_plan_param_info`` reports
that choice from the selection the launch itself uses; every case below first
asserts it (and ``lds_bytes <= lds_limit``), so a plan cannot land elsewhere
silently.  The cases (tests/param_matrix.py: networks with explicit, seeded
parameters loaded through ``Node.load_node``; nothing is trained):

lin_m1        LinearRegression (MODE 0 sigma = 1, 1 sigma = 0.5) and
              LogisticRegression (MODE 2, 3), all evidence, 7 / 8 factors:
              <8, 0, MODE, M1> at N = 7 (N % 4 != 0: scalar stores), 8 and 12
              (ragged second chunk); <16, 0, MODE, M1> ("lin16") at N = 16, 20
              (4 ragged columns with N % 4 == 0: the scalar row store of a
              short last chunk), 33 and 40 (3 chunks, 8 ragged); 2 parts below
              8 factors or below N = 16, else 4; a 2-factor plan whose split
              has an empty second range
lin_free      the same families with one unobserved parent, N = 8, 12, 20:
              <8, 0, MODE, M1 = false>, 2 parts
h1_m1/h1_free one hidden layer (MODE 2, 3), all evidence (9 factors: 4 parts;
              7 factors: 2) and one free parent (2 parts): NC 8 at N = 8, 16 at
              16, 32 at 20 (one ragged chunk), 32 (full chunk: vector stores),
              40 (two chunks) and 64; widths 16, 7 (a padding unit in the last
              pair) and 48 (streamed); tanh and relu (the templated mlp1p_nin)
              and gelu (mlp1p_rt)
h32_all/_free two hidden layers [8, 8] tanh and [32, 32] relu (MODE 2, 3) at
              N = 8 (NC 8, 2 parts), 16, 20 and 40 (NC 16 / 32: ONE part -- the
              128 KiB scratch plus the split's combine buffer is more LDS than
              a launch may request; before the plan-time fix these plans failed
              at their first call)
switch_*      <16, 32, 4, TAB = false>: plans mixing log_scale 0 and log 0.5
              (LogisticRegression, NN [16], NN [8, 8]) and plans with a
              5-input factor (LogisticRegression, NN [8, 8]), N = 12 and 40
generic       NN [33, 4] (k_param_query_gen, 16-column chunks), N = 20 and 40
const         evidence on the target's parent alone at N = 40 and 64: every
              other factor is built once by k_param_const<0 | 1 | 32>, and the
              query kernel reads those padded rows in its last chunk

No instantiation is unreachable: tests/test_param_matrix_cases.py asserts that
the table's (NC, HMAX, MODE, TAB, M1) tuples are exactly the 31 the dispatch
holds.

Per case, one seeded 257-row batch: ``infer`` and ``infer_raw`` + scale agree
bit for bit; the normalised rows match the oracle through
``parity.assert_marginals_close`` with ``oracle_reference``'s own keywords, the
unnormalised ones at rtol 1e-5 + n_factors * 2^-149 * peak (cases with a free
parent: the first 32 rows and the batch's arg-max row, one normaliser for both
sides -- the oracle holds N^(parents + 1) values per row and factor).  Then the
prefixes Q = 65, 64, 63 and a single row: raw rows bit-equal to the same rows
of the 257-row launch (a row's bits never depend on its wave-mates: lanes past
Q read row Q - 1 and store nothing), and ``infer`` == ``infer_raw`` + scale.
The single row follows a 257-row launch on both routes, so the words of the
blocks it does not run are stale and must be zeroed; it is the first row whose
max is nonzero and below the batch max, so a stale word would show as a row
max below 1.

Grid-stride batches (``test_grid_stride_*``): for one plan per kernel family
the batch size is computed from ``cbn_param_info`` so that the wave tasks
exceed ``max_blocks`` x groups per block (some block makes a second trip of
the loop that holds the combine step's block barriers), Q % 64 != 0 and the
task count is no multiple of the groups per block (idle waves in the last
trip).  The first and last 128 rows, 64 sampled rows and the arg-max row are
bit-equal to the same rows run as a small batch, and 33 of them match the
oracle.
"""
import random

import numpy as np
import pytest
import torch

import param_matrix as pm
from continuousbayesiannetwork_amd import BayesianNetwork, _native
from helpers import make_bn, param_config
from parity import assert_marginals_close, oracle_raw, oracle_reference
from test_gpu_param import load_fixture_params

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def _t(ev, dev):
    return {k: torch.tensor(v, device=dev) for k, v in ev.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bn(case, gpu, tmp_path):
    data, cols, edges, _, _, params = pm.network(case)
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu, estimator=case.est,
                 config=param_config(case.est, n_epochs=1, model=case.model))
    load_fixture_params(bn, {"meta": {"estimator": case.est}, "params": params}, tmp_path, gpu)
    return bn


def _plan_info(bn, case, evt, gpu):
    """The case's plan reaches the kernel the table says, with an LDS request that fits."""
    target = pm.network(case)[3]
    plan, _ = bn.engine.call_plan(target, evt, case.N)
    assert _native.load().cbn_plan_flags(plan.handle) & _native.CBN_PLAN_PARAMETRIC
    info = _native.param_info(plan.handle)
    got = {k: info[k] for k in case.info}
    assert got == case.info, (case.id, info)
    assert 0 <= info["lds_bytes"] <= info["lds_limit"] == 160 * 1024 - 256, info
    assert info["max_blocks"] == min(4 * torch.cuda.get_device_properties(gpu).multi_processor_count, 1024)
    return info


def _raw(bn, target, evt, N):
    """(raw rows, scaled rows) of one raw launch + scale, as host copies."""
    res = bn.engine.infer_raw(target, evt, N)
    assert res is not None
    raw = res[0].cpu().numpy().copy()
    out = res[3](res[0], res[2]).cpu().numpy().copy()
    return raw, out


def _against_oracle(case, ev, sub, pdf, raw):
    """Rows ``sub`` of the batch (the last one the batch's arg-max row when
    ``sub`` is not the whole batch) against the oracle: normalised and raw."""
    target = pm.network(case)[3]
    ora = pm.oracle(case)
    evs = {k: v[sub] for k, v in ev.items()}
    whole = len(sub) == pdf.shape[0]
    random.seed(0)
    ref, _, kw = oracle_reference(ora, target, evs, case.N, norm_row=None if whole else -1)
    assert_marginals_close(pdf[sub], ref, **kw)
    ref_raw, _ = oracle_raw(ora, target, evs, case.N)
    np.testing.assert_allclose(raw[sub], ref_raw, rtol=RTOL, atol=kw["n_factors"] * 2.0 ** -149 * kw["peak"])


@pytest.mark.parametrize("case", pm.CASES, ids=lambda c: c.id)
def test_param_kernel_case(case, gpu, tmp_path):
    target = pm.network(case)[3]
    N = case.N
    bn = _bn(case, gpu, tmp_path)
    ev = pm.evidence(case, pm.SMALL)
    evt = _t(ev, gpu)
    _plan_info(bn, case, evt, gpu)

    raw, out = _raw(bn, target, evt, N)
    pdf, dom = bn.infer(target, evt, N_max=N)
    pdf = pdf.cpu().numpy().copy()
    assert pdf.shape == (pm.SMALL, N) and dom.shape[-1] == N
    np.testing.assert_array_equal(_bits(pdf), _bits(out))
    rowmax = raw.max(1)
    rstar = int(np.argmax(rowmax))
    assert np.isfinite(raw).all() and pdf[rstar].max() == 1.0
    sub = np.arange(pm.SMALL) if case.all_evidence else np.append(np.arange(pm.ORACLE_ROWS - 1), rstar)
    _against_oracle(case, ev, sub, pdf, raw)

    for Q in (65, 64, 63):
        evq = {k: v[:Q] for k, v in evt.items()}
        rq, oq = _raw(bn, target, evq, N)
        np.testing.assert_array_equal(_bits(rq), _bits(raw[:Q]))
        pq = bn.infer(target, evq, N_max=N)[0].cpu().numpy()
        np.testing.assert_array_equal(_bits(pq), _bits(oq))
        assert oq.max() == 1.0

    # one row after the 257-row launch, on both routes (each has its own max words)
    cand = np.flatnonzero((rowmax > 0) & (rowmax < rowmax.max()))
    assert cand.size, "no row below the batch max"
    r = int(cand[0])
    ev1 = {k: v[r:r + 1] for k, v in evt.items()}
    _raw(bn, target, evt, N)
    r1, o1 = _raw(bn, target, ev1, N)
    np.testing.assert_array_equal(_bits(r1), _bits(raw[r:r + 1]))
    assert o1.max() == 1.0
    bn.infer(target, evt, N_max=N)
    p1 = bn.infer(target, ev1, N_max=N)[0].cpu().numpy()
    np.testing.assert_array_equal(_bits(p1), _bits(o1))


def _grid_stride_rows(info):
    """A batch size whose wave tasks exceed what the grid holds in one trip."""
    L = info["n_chunks"]
    if info["generic"]:  # one thread per (chunk, query): tasks = Q * L
        T = info["block_threads"]
        Q = info["max_blocks"] * T // L + 2 * 64 + 37
        while Q % 64 == 0 or (Q * L) % T == 0:
            Q += 1
        assert Q * L > info["max_blocks"] * T
        return Q
    gpb = info["block_threads"] // 64 // info["parts"]  # query groups per block
    QW = info["max_blocks"] * gpb // L + 2
    QW += next(d for d in range(gpb) if (L * (QW + d)) % gpb != 0)  # (the grid cases' chunk counts allow it)
    Q = QW * 64 - 27
    assert L * -(-Q // 64) > info["max_blocks"] * gpb and Q % 64 != 0 and (L * QW) % gpb != 0
    return Q


@pytest.mark.parametrize("case", pm.GRID_CASES, ids=lambda c: c.id)
def test_grid_stride_batch(case, gpu, tmp_path):
    target = pm.network(case)[3]
    N = case.N
    bn = _bn(case, gpu, tmp_path)
    info = _plan_info(bn, case, _t(pm.evidence(case, 8), gpu), gpu)
    Q = _grid_stride_rows(info)
    assert Q * N * 4 < 64 << 20, Q  # a few MB to a few tens of MB
    ev = pm.evidence(case, Q, seed=pm.EV_SEED + 1)
    evt = _t(ev, gpu)
    res = bn.engine.infer_raw(target, evt, N)
    assert res is not None
    rows = res[0]
    rstar = int(torch.argmax(rows.max(1).values))
    rng = np.random.default_rng(3)
    pick = np.unique(np.concatenate([np.arange(128), np.arange(Q - 128, Q), rng.integers(128, Q - 128, 64), [rstar]]))
    idx = torch.tensor(pick, device=gpu)
    raw = rows[idx].cpu().numpy().copy()
    assert np.isfinite(raw).all() and bool(torch.isfinite(rows).all())
    pdf = res[3](rows, res[2])[idx].cpu().numpy().copy()
    assert pdf.max() == 1.0
    full = bn.infer(target, evt, N_max=N)[0][idx].cpu().numpy()
    np.testing.assert_array_equal(_bits(full), _bits(pdf))
    # the same rows as a small batch
    small = {k: v[pick] for k, v in ev.items()}
    rs, _ = _raw(bn, target, _t(small, gpu), N)
    np.testing.assert_array_equal(_bits(rs), _bits(raw))
    # 32 of them and the arg-max row through the oracle
    at = int(np.flatnonzero(pick == rstar)[0])
    sub = np.append(rng.choice(np.delete(np.arange(pick.size), at), pm.ORACLE_ROWS - 1, replace=False), at)
    _against_oracle(case, small, sub, pdf, raw)
