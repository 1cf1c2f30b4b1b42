"""What ``predict``, ``posterior`` and ``quantile`` share above the kernels
(``InferenceEngine._reduce``), pinned for every operation on every route a plan
can take to its raw rows:

  (1) a rejected call leaves no trace: it raises what ``infer`` raises on that
      evidence, marks no table as built, and the next valid call returns the
      bits a fresh engine returns;
  (2) a plan the call owns (``call_plan`` hands it over without a fast path, as
      it does a plan rebuilt per call) is destroyed, on success and on a raise;
  (3) the native hot path (contiguous float32 device columns) and the general
      path (float64 host columns, converted) return the same bits.

Operations: predict; posterior with and without rows; quantile with 3 and with
17 shared probabilities (17: beyond CBN_MAX_QUANTILES, the scratch route of a
fast plan) and with a [Q, 3] tensor.  Routes: the staged all-evidence N = 32
chain (the reductions run in the query kernel), a generic table plan, a forced
direct plan, a parametric plan (the linear-regression network) and a [Q, N]
evidence column (the wide direct plan).  Q = 4 throughout.

``predict``'s ``value`` keeps the plan's ``target_domain`` dtype when that is
not float32; no builder here yields such a plan (``BayesianNetwork.fit`` stores
every column as float32), so that is not pinned here.
"""
import random

import numpy as np
import pytest
import torch

from continuousbayesiannetwork_amd import BayesianNetwork, _native
from continuousbayesiannetwork_amd.inference.engine import InferenceEngine
from helpers import chain_data, make_bn, sample_evidence
from test_gpu_predict import _fallback_case

pytestmark = pytest.mark.gpu

Q = 4
P3 = (0.1, 0.5, 0.9)
P17 = tuple(np.linspace(0.02, 0.98, 17).tolist())
ROUTES = {"native": None, "generic": "generic5", "forced_direct": "forced_direct", "parametric": "linear_regression",
          "wide": "wide"}


def _probs_q3(dev):
    return torch.tensor(np.random.default_rng(3).uniform(0.05, 0.95, (Q, 3)), dtype=torch.float32, device=dev)


OPS = {
    "predict": lambda e, t, ev, N, dev: e.predict(t, ev, N),
    "posterior_rows": lambda e, t, ev, N, dev: e.posterior(t, ev, N, rows=True),
    "posterior_no_rows": lambda e, t, ev, N, dev: e.posterior(t, ev, N, rows=False),
    "quantile_3": lambda e, t, ev, N, dev: e.quantile(t, ev, N, P3),
    "quantile_17": lambda e, t, ev, N, dev: e.quantile(t, ev, N, P17),
    "quantile_q3": lambda e, t, ev, N, dev: e.quantile(t, ev, N, _probs_q3(dev)),
}


class Case:
    """One route: the fitted network, a valid batch of Q rows and the same
    batch with one evidence column of shape [Q, 2]."""

    def __init__(self, route, gpu, tmp):
        self.route, self.dev = route, gpu
        if route == "native":
            data, cols, edges = chain_data(6, 32, 60000, 8, stay=0.8)
            self.bn = make_bn(BayesianNetwork, edges, cols, data, device=gpu)
            self.target, self.N, self.seed = "X5", 32, None
            ev = sample_evidence(data, cols, [c for c in cols if c != "X5"], Q, 40)
        else:
            self.bn, _, self.target, ev, self.N, _, _, self.seed = _fallback_case(ROUTES[route], gpu, tmp)
        self.force_direct = self.bn.engine.force_direct
        self.ev = {k: np.ascontiguousarray(v[:Q]) for k, v in ev.items()}
        k = next(iter(self.ev))
        self.bad = dict(self.ev, **{k: np.ascontiguousarray(np.concatenate([self.ev[k], self.ev[k]], 1)[:, :2])})

    def engine(self):
        """A fresh engine on the fitted network: no plan, no fast path."""
        e = InferenceEngine(self.bn)
        e.force_direct = self.force_direct
        return e

    def dev_ev(self, ev=None):
        return {k: torch.tensor(v, device=self.dev) for k, v in (self.ev if ev is None else ev).items()}

    def run(self, op, eng, ev=None):
        random.seed(self.seed)
        return OPS[op](eng, self.target, self.dev_ev() if ev is None else ev, self.N, self.dev)


@pytest.fixture(scope="module", params=list(ROUTES))
def case(request, gpu, tmp_path_factory):
    return Case(request.param, gpu, tmp_path_factory.mktemp(request.param))


def assert_same(a, b):
    """Bit-identical outputs (None where the other is None)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
            continue
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _rejects(case, op, eng, ev):
    with pytest.raises(Exception) as info:
        case.run(op, eng, ev)
    return type(info.value), str(info.value)


@pytest.mark.parametrize("op", list(OPS))
def test_a_rejected_call_leaves_no_trace(op, case):
    with pytest.raises(Exception) as info:
        random.seed(case.seed)
        case.engine().infer(case.target, case.dev_ev(case.bad), case.N)
    eng = case.engine()
    assert _rejects(case, op, eng, case.dev_ev(case.bad)) == (type(info.value), str(info.value))
    assert all(not p.tables_built for p in eng._plans.values())  # nothing was launched
    if op.startswith("quantile"):
        # one row of probabilities too many: raised before the general path marks the tables as built
        with pytest.raises(ValueError, match=f"{Q + 1} rows for {Q} queries"):
            random.seed(case.seed)
            eng.quantile(case.target, case.dev_ev(), case.N, torch.full((Q + 1, 3), 0.5, device=case.dev))
        assert all(not p.tables_built for p in eng._plans.values())
    assert_same(case.run(op, eng), case.run(op, case.engine()))


def _own_plans(eng):
    """Make every call of ``eng`` own its plan: ``call_plan`` forgets the plan
    it made and hands it over without a fast path, which is its contract for a
    plan rebuilt per call (the caller destroys it).  Returns the plans made."""
    made, call_plan = [], eng.call_plan

    def owned(target, evidence, N_max):
        plan, _ = call_plan(target, evidence, N_max)
        eng._fast.clear()
        eng._plans.clear()
        made.append(plan)
        return plan, None

    eng.call_plan = owned
    return made


@pytest.mark.parametrize("op", list(OPS))
def test_an_owned_plan_is_destroyed_on_success_and_on_raise(op, case):
    eng = case.engine()
    made = _own_plans(eng)
    out = case.run(op, eng)
    assert len(made) == 1 and made[0].handle is None and made[0].keep == []
    _rejects(case, op, eng, case.dev_ev(case.bad))
    assert len(made) == 2 and made[1] is not made[0] and made[1].handle is None
    if op.startswith("quantile"):
        with pytest.raises(ValueError, match="rows for"):
            eng.quantile(case.target, case.dev_ev(), case.N, torch.full((Q + 1, 3), 0.5, device=case.dev))
        assert len(made) == 3 and made[2].handle is None
    assert_same(out, case.run(op, case.engine()))  # ... and the owned plan gave the cached plan's bits


@pytest.mark.parametrize("op", list(OPS))
def test_fast_and_general_paths_agree(op, case):
    eng = case.engine()
    general, calls = eng._general_call, []
    eng._general_call = lambda *a: calls.append(1) or general(*a)
    fast = case.run(op, eng)
    # the route is the one this case is named for
    lib = _native.load()
    flags = [int(lib.cbn_plan_flags(p.handle)) for p in eng._plans.values()]
    native = _native.CBN_PLAN_ARGMAX | _native.CBN_PLAN_MOMENTS | _native.CBN_PLAN_QUANTILE
    want = {"native": _native.CBN_PLAN_STAGED | native, "forced_direct": _native.CBN_PLAN_DIRECT,
            "parametric": _native.CBN_PLAN_PARAMETRIC}.get(case.route, 0)
    # (a generic plan is none of these; a [Q, N] column leaves its base plan, of any kind, aside)
    forbid = {"native": 0, "wide": 0, "generic": native | _native.CBN_PLAN_FAST | _native.CBN_PLAN_DIRECT |
              _native.CBN_PLAN_PARAMETRIC}.get(case.route, native)
    assert len(flags) == 1 and flags[0] & want == want and not flags[0] & forbid, flags
    assert len(eng._wide_plans) == (case.route == "wide")
    # float32 device columns took the hot path wherever the plan is cached and its columns are [Q, 1]
    assert len(calls) == (0 if eng._fast and case.route != "wide" else 1)
    n = len(calls)
    slow = case.run(op, eng, {k: torch.tensor(v, dtype=torch.float64) for k, v in case.ev.items()})
    assert len(calls) == n + 1
    assert_same(fast, slow)
