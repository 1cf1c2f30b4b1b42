"""``cbn_plan_create`` builds the plan the planner describes, on this device.

For every case of tests/table_plan_cases.py one child process
(``tools/plan_census.py --both``, started with CBN_DIAG=1 for the cases'
switches) creates the plan -- no query is launched -- and asks
``cbn_table_plan_info`` with the device's CU count.  Per case:

* the plan's ``cbn_plan_flags`` (without CBN_PLAN_FUSED), table bytes, uses-LDS,
  max words and fused capacity equal the planner's; a plan without
  CBN_PLAN_FUSED has capacity 0;
* on a 256-CU device the five values equal the record of the commit before the
  planner existed (tests/data/table_plan_census.json, tests/test_table_plan.py);
* CBN_PLAN_FUSED is set exactly where that commit set it (the occupancy query
  depends on the kernel's registers and LDS, not on the CU count).
"""
import pytest

import table_plan_cases as tpc
from continuousbayesiannetwork_amd import _native
from test_table_plan import load_fixture, run_census

pytestmark = pytest.mark.gpu
FUSED = _native.CBN_PLAN_FUSED


@pytest.fixture(scope="module")
def census(gpu):
    return run_census("--both")


def test_every_case_made_a_plan(census):
    assert sorted(census) == sorted(c.name for c in tpc.CASES)


@pytest.mark.parametrize("name", [c.name for c in tpc.CASES])
def test_plan_is_what_the_planner_says(name, census):
    rec, want = census[name], load_fixture()[name]
    plan, info = rec["plan"], rec["info"]
    assert plan["flags"] & ~FUSED == info["flags"]
    assert (plan["table_bytes"], plan["uses_lds"], plan["max_words"]) == \
        (info["table_bytes"], info["uses_lds"], info["max_words"])
    assert plan["fused_capacity"] == (info["fused_capacity"] if plan["flags"] & FUSED else 0)
    assert plan["flags"] & FUSED == want["flags"] & FUSED
    if rec["n_cu"] == 256:
        assert plan == {k: want[k] for k in plan}
