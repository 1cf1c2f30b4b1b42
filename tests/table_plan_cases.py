"""Synthetic table plans for the planner census (tools/plan_census.py,
tests/test_table_plan.py, tests/test_gpu_table_plan.py).

A case is ``Case(name, N, factors, env)``: ``factors`` is one
``(node_card, [(parent_card, evidence_slot or -1), ...])`` per factor, in plan
order -- integers only, the shape ``engine.py`` hands to ``cbn_plan_create``
for a network (one factor per node in topological order; a root is SCALAR, a
node with an observed parent QUERY, else SHARED) -- and ``env`` the diagnostic
switches (with ``CBN_DIAG=1``) the case is created under.  ``descriptors()``
turns the integers into ``cbn_factor_desc`` with caller-supplied pointers.

Every value of the planner's kernel enum and both sides of every gate in
``csrc/cbn_table_plan.h`` is reached; the comment on each case says which.
"""
import ctypes
from collections import namedtuple

Case = namedtuple("Case", "name N factors env")


def network(n, card, parents, observed):
    """Factors of an n-node network: ``parents(i)`` lists node i's parents,
    ``observed`` the evidence nodes (slots in ascending node order)."""
    slot = {v: s for s, v in enumerate(sorted(observed))}
    return [(card, [(card, slot.get(p, -1)) for p in parents(i)]) for i in range(n)]


def chain(n, d, observed=None, extra=None):
    """X0 -> X1 -> ... ; ``extra`` maps a node to further parents."""
    observed = range(n - 1) if observed is None else observed
    extra = extra or {}
    return network(n, d, lambda i: ([i - 1] if i else []) + list(extra.get(i, [])), observed)


def grid(side, d):
    """side x side lattice, node (r, c) has parents (r-1, c) and (r, c-1); all but the last node observed."""
    def parents(i):
        r, c = divmod(i, side)
        return ([i - side] if r else []) + ([i - 1] if c else [])
    return network(side * side, d, parents, range(side * side - 1))


def star(k, d):
    """k observed roots feeding one node."""
    return network(k + 1, d, lambda i: list(range(k)) if i == k else [], range(k))


HOUSE = [7 + f for f in range(32) if f % 4 in (2, 3)]  # tests/test_gpu_staged_shapes.py, case A
GATE = [7 + f for f in range(33) if f % 4 in (0, 3)]   # ... case F
# ALARM-shaped (in-degree <= 4, d = 8, two 4096-row tables); 36 factors: with 37 and one lane per query
# (N = 8) k_query_fast's offset buffer alone is 160 KiB
ALARM = chain(36, 8, extra={20: [18, 17, 16], 30: [28, 27, 26], 12: [10], 33: [5]})
BENCH = chain(20, 32)
GRID5 = grid(5, 32)

CASES = [
    # k_query_cols, tables in LDS: one lane per query (N = 4: VPL 1; N = 8: VPL 2)
    Case("config0_chain5_d4", 4, chain(5, 4), {}),
    Case("chain8_d8", 8, chain(8, 8), {}),
    # k_query_staged: the benchmark's plan
    Case("bench_chain20_d32", 32, BENCH, {}),
    # the staged kernel's LDS gate: the last staged chain, the first paired k_query_fast
    Case("chain24_d32", 32, chain(24, 32), {}),
    Case("chain25_d32", 32, chain(25, 32), {}),
    # the 128-entry pointer table gate (nf = 32 staged / 33 paired fast), prefix at its cap of 8
    Case("house40_nf32", 32, chain(40, 32, HOUSE), {}),
    Case("gate41_nf33", 32, chain(41, 32, GATE), {}),
    # evidence on one late node: prefix 8, un-merged 1-row factors behind it
    Case("tail12_x10", 32, chain(12, 32, [10]), {}),
    Case("tail6_x4", 32, chain(6, 32, [4]), {}),  # prefix = n_factors - 1
    # 1, 7, 8 and 9 leading one-row factors
    *[Case(f"prefix{k}_chain12", 32, chain(12, 32, range(k - 1, 11)), {}) for k in (1, 7, 8, 9)],
    # the paired layout's 3/4-of-LDS gate: 30 nodes fill it exactly, 31 and 33 nodes exceed it
    # (padded rows, an image too large to stage: k_query_slots over a padded layout)
    Case("chain30_d32", 32, chain(30, 32), {}),
    Case("chain31_d32", 32, chain(31, 32), {}),
    Case("chain33_d32", 32, chain(33, 32), {}),
    # plain k_query_fast, tables in LDS (8 lanes per query)
    Case("chain5_d64", 64, chain(5, 64), {}),
    # k_query_fast over global tables with the large pointer table (66 factors: above k_query_cols' 64)
    Case("chain66_d16_obs3", 16, chain(66, 16, extra={40: [38, 37]}), {}),
    # k_query_cols over a global table
    Case("star3_d16", 16, star(3, 16), {}),
    # k_query_cols, two large tables in L2 and the small ones split into LDS
    Case("alarm36_d8", 8, ALARM, {}),
    # k_query_slots
    Case("chain100_d32", 32, chain(100, 32), {}),
    Case("grid5_d32", 32, GRID5, {}),
    Case("grid10_d64", 64, grid(10, 64), {}),  # the small-table budget beside k_query_slots' buffers
    # generic: vec = 1
    Case("chain5_d3_n3", 3, chain(5, 3), {}),
    Case("chain5_d6_n6", 6, chain(5, 6), {}),
    # generic: five observed parents (above kFastObs), 105 factors (above kFastPtrs / 4)
    Case("star5_d4", 16, star(5, 4), {}),
    Case("chain105_d4", 4, chain(105, 4), {}),
    # free parents (SHARED factors), tables in LDS
    Case("chain6_d8_free", 8, chain(6, 8, [4]), {}),
    # the fast kernel's side buffers beyond LDS (one lane per query, 40 factors): generic, in LDS / global
    Case("chain32_d4", 4, chain(32, 4), {}),
    Case("chain40_d4", 4, chain(40, 4), {}),
    Case("alarm37_d8_n8", 8, chain(37, 8, extra={20: [18, 17, 16], 30: [28, 27, 26]}), {}),
    # a slot of more than 32 767 values: k_query_cols (N = 4) and k_query_slots (N = 32) decline
    Case("chain3_d40000_n4", 4, chain(3, 40000), {}),
    Case("chain3_d40000_n32", 32, chain(3, 40000), {}),
    # one case per diagnostic switch, on a plan it changes
    Case("bench_fast_vpl1", 32, BENCH, {"CBN_FAST_VPL": "1"}),
    Case("alarm_fast_vpl1", 8, ALARM, {"CBN_FAST_VPL": "1"}),
    Case("bench_no_paired", 32, BENCH, {"CBN_NO_PAIRED": "1"}),
    Case("tail12_no_prefix", 32, chain(12, 32, [10]), {"CBN_NO_PREFIX": "1"}),
    Case("alarm_no_lds_split", 8, ALARM, {"CBN_NO_LDS_SPLIT": "1"}),
    Case("grid5_no_slots", 32, GRID5, {"CBN_NO_SLOTS": "1"}),
    Case("bench_no_staged", 32, BENCH, {"CBN_NO_STAGED": "1"}),
    Case("config0_no_cols", 4, chain(5, 4), {"CBN_NO_COLS": "1"}),
    Case("bench_no_fused", 32, BENCH, {"CBN_NO_FUSED": "1"}),
    Case("grid5_slots_bpc1", 32, GRID5, {"CBN_SLOTS_BPC": "1"}),
    Case("grid5_slots_bpc2", 32, GRID5, {"CBN_SLOTS_BPC": "2"}),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def slot_cards(case):
    """card of every evidence slot, in slot order."""
    cards = {}
    for _, parents in case.factors:
        for card, slot in parents:
            if slot >= 0:
                cards[slot] = card
    return [cards[s] for s in range(len(cards))]


def descriptors(case, factor_desc, ptr=16, domain_ptr=None):
    """``cbn_factor_desc[]`` of a case.  ``ptr`` stands for every CPD and
    sample-index pointer (plan creation never reads them); ``domain_ptr(slot)``
    gives the slots' domains, which ``cbn_plan_create`` does read."""
    descs = (factor_desc * len(case.factors))()
    for d, (node_card, parents) in zip(descs, case.factors):
        d.kind = 0 if not parents else (2 if any(s >= 0 for _, s in parents) else 1)
        d.n_parents = len(parents)
        d.node_card = node_card
        d.cpd = d.node_sample_idx = ptr
        d.parent_sample_idx = ptr if parents else None
        for i, (card, slot) in enumerate(parents):
            d.parent_card[i] = card
            d.parent_ev_slot[i] = slot
            if slot >= 0:
                d.parent_domain[i] = domain_ptr(slot) if domain_ptr else ptr
    return descs


def factor_desc_type():
    """``cbn_factor_desc`` for callers that load a library without the package's binding."""
    class FactorDesc(ctypes.Structure):
        _fields_ = [("kind", ctypes.c_int32), ("n_parents", ctypes.c_int32), ("node_card", ctypes.c_int32),
                    ("parent_card", ctypes.c_int32 * 8), ("parent_ev_slot", ctypes.c_int32 * 8),
                    ("cpd", ctypes.c_void_p), ("node_sample_idx", ctypes.c_void_p),
                    ("parent_sample_idx", ctypes.c_void_p), ("parent_domain", ctypes.c_void_p * 8)]
    return FactorDesc
