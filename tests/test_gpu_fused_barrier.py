"""The fused launch's grid barrier (slot_barrier_max: every block publishes
{epoch, block max} in its own slot, wave 0 of every block polls all slots,
lane i owning slots i, i + 64, ...) at the grid sizes where lane ownership
changes (1, 2, 64, 65, 255 and 256 blocks), with the global max in the first
and in the last block, across calls that leave slots of larger earlier grids
at old epochs, and in the other kernels that call it.

Reference for every case: the two-launch path (``engine.fused = False``: max
pass, write pass, no grid barrier) bit for bit, and for the staged plan the CPU
oracle on a sample of rows through tests/parity.py.
"""
import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from helpers import chain_data, make_bn, sample_evidence
from oracle.ref_infer import OracleBN
from parity import assert_marginals_close, n_factors, oracle_raw

pytestmark = pytest.mark.gpu

TARGET, N = "X5", 32
QMAX = 65536
# One block holds 256 queries and the fused grid is ceil(Q / 256) blocks: grids
# of 1, 1, 1, 2, 64, 65, 255, 255, 256 and 256 blocks.  At 255 blocks lane 63
# owns three slots and every other lane four (65 279: the last block one query
# short; 65 280: full); 65 281 is 256 blocks with a single query in the last.
QS = [1, 255, 256, 257, 16384, 16385, 65279, 65280, 65281, 65536]
BLOCKS = {1: 1, 255: 1, 256: 1, 257: 2, 16384: 64, 16385: 65, 65279: 255, 65280: 255, 65281: 256, 65536: 256}
SAMPLE = 257


def _t(ev, dev, Q=None):
    return {k: torch.tensor(v[:Q], device=dev) for k, v in ev.items()}


class _Chain:
    """6-node chain, d = N = 32 (a staged plan), three evidence pools of 65 536
    rows and the oracle's unnormalised rows of pool 0's first 257 rows."""

    def __init__(self, dev):
        self.data, self.cols, self.edges = chain_data(6, 32, 60000, 8, stay=0.8)
        self.names = [c for c in self.cols if c != TARGET]
        self.bn = make_bn(BayesianNetwork, self.edges, self.cols, self.data, device=dev)
        self.pools = [sample_evidence(self.data, self.cols, self.names, QMAX, 40 + i) for i in range(3)]
        self.ora = OracleBN(self.edges, self.cols, self.data)
        self.raw, _ = oracle_raw(self.ora, TARGET, {k: v[:SAMPLE] for k, v in self.pools[0].items()}, N)
        self.raw.setflags(write=False)
        self.dev = dev

    def run(self, ev, fused):
        """(rows as numpy, plan flags) of one infer on the given path."""
        self.bn.engine.fused = fused
        try:
            pdf, _ = self.bn.infer(TARGET, ev, N_max=N)
            out = pdf.clone()
            torch.cuda.synchronize()
            self.bn.engine.check_status()
        finally:
            self.bn.engine.fused = True
        fp = self.bn.engine._fast[(TARGET, tuple(ev.keys()), N)]
        return out.cpu().numpy(), _native.load().cbn_plan_flags(fp.plan.handle)


@pytest.fixture(scope="module")
def chain(gpu):
    return _Chain(gpu)


@pytest.mark.parametrize("Q", QS)
def test_staged_fused_grid_edges(Q, chain):
    """Fused == two-launch bit for bit at every lane-ownership edge of the
    grid; a sample of 257 rows plus the batch's arg-max row matches the oracle
    (normalised by that row's max); the global-max row, made unique and moved
    to query 0 and then to query Q - 1, has max exactly 1.0."""
    ev_np = {k: v[:Q] for k, v in chain.pools[0].items()}
    ev = _t(ev_np, chain.dev)
    two, flags = chain.run(ev, fused=False)
    one, flags = chain.run(ev, fused=True)
    assert flags & _native.CBN_PLAN_STAGED
    assert chain.bn.engine.fused_capacity(TARGET, chain.names, N) >= QMAX
    assert BLOCKS[Q] == (Q + 255) // 256  # the grid this case is about (launch_fused_v: ceil(Q / 256))
    np.testing.assert_array_equal(one, two)
    assert one.max() == 1.0

    # the oracle: pool 0's first rows (computed once) + this batch's arg-max row
    rstar = int(np.argmax(one.max(1)))
    ns = min(Q, SAMPLE)
    star, mx = oracle_raw(chain.ora, TARGET, {k: v[rstar:rstar + 1] for k, v in ev_np.items()}, N)
    ref = (np.concatenate([chain.raw[:ns], star]) / mx).astype(np.float32)
    assert ref.max() == 1.0 and ref[-1].max() == 1.0  # the GPU's arg-max row is the oracle's too
    sub = np.append(np.arange(ns), rstar)
    assert_marginals_close(one[sub], ref, raw_max=mx, n_factors=n_factors(chain.ora, TARGET))

    # one row alone holds the global max (every other row at the max takes the
    # evidence of a row below it), first as query 0, then as query Q - 1
    top = np.flatnonzero(one.max(1) == 1.0)
    below = np.flatnonzero(one.max(1) < 1.0)
    for pos in sorted({0, Q - 1}):
        e = {k: v.copy() for k, v in ev_np.items()}
        for k in e:
            if below.size:
                e[k][top[1:]] = e[k][below[0]]
            e[k][[pos, rstar]] = e[k][[rstar, pos]]
        evp = _t(e, chain.dev)
        got, _ = chain.run(evp, fused=True)
        assert got[pos].max() == 1.0 and got.max() == 1.0
        want, _ = chain.run(evp, fused=False)
        np.testing.assert_array_equal(got, want)


def test_staged_fused_stale_epochs(chain):
    """One plan, consecutive fused calls: three with different evidence, then
    shrinking and growing grids (65 536 -> 257 -> 16 385 -> 1 -> 65 536
    queries), so that the slots of the larger earlier grids carry old epochs.
    Every call equals the two-launch path."""
    seq = [(QMAX, 0), (QMAX, 1), (QMAX, 2), (QMAX, 0), (257, 1), (16385, 2), (1, 0), (QMAX, 1)]
    evs = {(Q, i): _t(chain.pools[i], chain.dev, Q) for Q, i in set(seq)}
    want = {key: chain.run(ev, fused=False)[0] for key, ev in evs.items()}
    got = [chain.run(evs[key], fused=True)[0] for key in seq]  # the fused calls, back to back
    for key, g in zip(seq, got):
        np.testing.assert_array_equal(g, want[key], err_msg=f"Q = {key[0]}, pool {key[1]}")


def _other_plan_case(gpu, n, d, want_flag):
    """Fused == two-launch on a chain whose plan runs another fused kernel, at
    a batch of 65 blocks (64 full ones + one query): the block capacity, 16
    waves x 64 / L queries, is read off the plan's fused capacity."""
    data, cols, edges = chain_data(n, d, 60000, 8, stay=0.8)
    target = cols[-1]
    names = cols[:-1]
    bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
    bn.infer(target, _t(sample_evidence(data, cols, names, 8, 1), gpu), N_max=d)  # plans
    fp = bn.engine._fast[(target, tuple(names), d)]
    flags = _native.load().cbn_plan_flags(fp.plan.handle)
    assert flags & _native.CBN_PLAN_FAST and flags & _native.CBN_PLAN_FUSED and not flags & _native.CBN_PLAN_STAGED
    assert (flags & (_native.CBN_PLAN_COLS | _native.CBN_PLAN_SLOTS)) == want_flag
    # capacity = #CUs blocks x 16 waves x 64 / L queries (x 2 rounds for cols / slots plans)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    rounds = 2 if want_flag else 1
    cap = bn.engine.fused_capacity(target, names, d)
    per_block = cap // (min(cus, 1024) * rounds)
    L = d // (8 if flags & _native.CBN_PLAN_VPL2 else 4)
    assert per_block == 16 * 64 // L
    Q = 64 * per_block + 1
    assert Q <= cap and (Q + per_block - 1) // per_block == 65
    ev = _t(sample_evidence(data, cols, names, Q, 2), gpu)
    bn.engine.fused = False
    a = bn.infer(target, ev, N_max=d)[0].clone()
    bn.engine.fused = True
    b = bn.infer(target, ev, N_max=d)[0].clone()
    torch.cuda.synchronize()
    bn.engine.check_status()
    np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert float(b.max()) == 1.0


def test_cols_plan_fused_65_blocks(gpu):
    """k_query_cols (N = 16 chain: 2 lanes per query)."""
    _other_plan_case(gpu, 20, 16, _native.CBN_PLAN_COLS)


def test_fast_plan_fused_65_blocks(gpu):
    """k_query_fast's fused mode (N = 64 chain in LDS: 8 lanes per query,
    neither the staged N = 32 layout nor a column-staged plan)."""
    _other_plan_case(gpu, 5, 64, 0)
