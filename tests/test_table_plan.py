"""The table planner (csrc/cbn_table_plan.h) decides what the recorded census says.

tests/data/table_plan_census.json holds, for every case of
tests/table_plan_cases.py, what ``cbn_plan_create`` of the commit before the
planner existed reported on an MI355X (256 CUs): ``cbn_plan_flags``,
``cbn_plan_table_bytes``, ``cbn_plan_uses_lds``, ``cbn_plan_max_words`` and
``cbn_plan_fused_capacity`` (tools/plan_census.py wrote it).  Here
``cbn_table_plan_info`` -- the planner alone, no device -- is asked for the
same cases at ``n_cu = 256`` under the case's diagnostic switches and must
give the same values: flags without CBN_PLAN_FUSED (the occupancy query at plan
creation decides that bit), and the fused capacity wherever the record's is
nonzero.

The switches count only in a process started with CBN_DIAG=1, so one child
(``tools/plan_census.py --info``) computes every case; the tests share its
output.  No GPU is needed.
"""
import json
import os
import subprocess
import sys

import pytest

import table_plan_cases as tpc
from continuousbayesiannetwork_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "data", "table_plan_census.json")
KERNELS = set(_native.TABLE_KERNELS)


def load_fixture():
    with open(FIXTURE) as fh:
        return {r["name"]: r for r in json.load(fh)}


def run_census(*args):
    """{case name: record} of one tools/plan_census.py child started with CBN_DIAG=1."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CBN_")}
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "tools", "plan_census.py"), *args],
                       env={**env, "CBN_DIAG": "1"}, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return {r["name"]: r for r in map(json.loads, p.stdout.strip().splitlines())}


@pytest.fixture(scope="module")
def infos():
    return run_census("--info", "--n-cu", "256")


def test_fixture_covers_the_case_list():
    fx = load_fixture()
    assert len(tpc.CASES) >= 40
    assert sorted(fx) == sorted(c.name for c in tpc.CASES)
    for c in tpc.CASES:  # the record is of these very descriptors
        r = fx[c.name]
        assert (r["N"], r["env"], r["n_cu"]) == (c.N, c.env, 256), c.name
        assert r["factors"] == json.loads(json.dumps(c.factors)), c.name


def test_every_case_is_planned(infos):
    """Every case's descriptors are accepted, and every kernel is some case's."""
    assert sorted(infos) == sorted(c.name for c in tpc.CASES)
    assert {r["info"]["kernel"] for r in infos.values()} == KERNELS


@pytest.mark.parametrize("name", [c.name for c in tpc.CASES])
def test_planner_matches_the_recorded_plan(name, infos):
    want, got = load_fixture()[name], infos[name]["info"]
    assert got["flags"] == want["flags"] & ~_native.CBN_PLAN_FUSED
    assert got["table_bytes"] == want["table_bytes"]
    assert got["uses_lds"] == want["uses_lds"]
    assert got["max_words"] == want["max_words"]
    if want["fused_capacity"]:
        assert got["fused_capacity"] == want["fused_capacity"]
    assert got["fused_candidate"] or not want["flags"] & _native.CBN_PLAN_FUSED


def test_switches_count_only_under_cbn_diag():
    """In this process (no CBN_DIAG) a switch in the environment changes nothing."""
    case = tpc.BY_NAME["bench_chain20_d32"]
    descs = tpc.descriptors(case, _native.FactorDesc)
    base = _native.table_plan_info(descs, len(case.factors), case.N, 256)
    assert _native.TABLE_KERNELS[base["kernel"]] == "staged"
    if not _native.load().cbn_diag_enabled():
        os.environ["CBN_NO_STAGED"] = "1"
        try:
            assert _native.table_plan_info(descs, len(case.factors), case.N, 256) == base
        finally:
            del os.environ["CBN_NO_STAGED"]
    # the CU count only scales the grid's bounds
    half = _native.table_plan_info(descs, len(case.factors), case.N, 128)
    assert half["max_slots"] == base["max_slots"] // 2 and half["fused_capacity"] == base["fused_capacity"] // 2
    assert {k: v for k, v in half.items() if k not in ("max_slots", "fused_capacity")} == \
        {k: v for k, v in base.items() if k not in ("max_slots", "fused_capacity")}
