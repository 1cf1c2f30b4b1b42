"""Child process of tests/test_gpu_diag.py and tests/test_native_abi.py.

Diagnostic kernel-selection switches (CBN_NO_STAGED, CBN_PARAM_GENERIC, ...)
count only when libcbn_amd.so is loaded with CBN_DIAG=1 (cbn_diag_enabled,
include/cbn_amd.h), so a test that toggles them needs a process started with
the environment it is testing.  Prints one JSON line.

    python tests/diag_child.py enabled   # no GPU: cbn_diag_enabled()
    python tests/diag_child.py flags     # configs[1]-shaped plan's cbn_plan_flags
    python tests/diag_child.py generic   # NN [16] rows: fast kernel vs CBN_PARAM_GENERIC
    python tests/diag_child.py gridfull  # configs[4] bench batch: k_query_slots vs k_query_fast (CBN_NO_SLOTS)
    python tests/diag_child.py gridcoal  # k_query_slots' coalesced index phase vs the per-lane one (CBN_SLOTS_NO_COAL)
    python tests/diag_child.py coalspecial  # special evidence values: coalesced index phase (CBN_SLOTS_COAL) vs per-lane
    python tests/diag_child.py paramlin  # linear parametric plan: 16- vs 8-column chunks, M1 vs CBN_PARAM_NO_M1
    python tests/diag_child.py paramh1   # NN [16] plan: CBN_PARAM_NC 8 / 16 / 32, M1 vs CBN_PARAM_NO_M1
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(mode: str):
    from continuousbayesiannetwork_amd import _native

    lib = _native.load()
    res = {"diag": int(lib.cbn_diag_enabled())}
    if mode == "enabled":
        print(json.dumps(res))
        return
    import numpy as np
    import torch

    from continuousbayesiannetwork_amd import BayesianNetwork
    from helpers import chain_data, make_bn, mixed_dag_data, param_config, sample_evidence

    dev = torch.device("cuda:0")
    if mode == "flags":
        # BASELINE configs[1]'s plan shape: 20-node chain, d = 32, evidence on X0..X18, N = 32
        data, cols, edges = chain_data(20, 32, 20000, 21, stay=0.8)
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev)
        ev = {k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, cols[:19], 1024, 5).items()}
        bn.infer("X19", ev, N_max=32)
        res["flags"] = [int(lib.cbn_plan_flags(p.handle)) for p in bn.engine._plans.values()]
    elif mode == "generic":
        data, cols, edges = mixed_dag_data(3000, 4, n=12, unit=True)
        model = {"hidden_dims": [16], "activation": "tanh"}
        names = [cols[-2], cols[5], cols[2]]
        ev = {k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, names, 500, 3).items()}
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev, estimator="neural_network",
                     config=param_config("neural_network", n_epochs=10, model=model))
        os.environ["CBN_PARAM_PARTS"] = "1"  # one factor range per wave: the generic kernel's product order
        outs, flags = [], []
        for generic in (False, True):
            if generic:  # read at plan creation: drop the cached plan
                os.environ["CBN_PARAM_GENERIC"] = "1"
                bn.engine.invalidate()
            random.seed(4)
            outs.append(bn.infer(cols[-1], ev, N_max=8)[0].cpu().numpy())
        res["equal"] = bool(np.array_equal(outs[0], outs[1], equal_nan=True))
        res["finite"] = int(np.isfinite(outs[0]).sum())
    elif mode == "gridfull":
        # tools/bench_grid.py's headline batch (BASELINE configs[4], 65 536 queries)
        from helpers import grid_data

        data, cols, edges = grid_data(400_000, 3, side=10, d=64, keep=0.995, noise=0)
        target, names = cols[-1], cols[:-1]
        ev = {k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, names, 65536, 0).items()}
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev)
        outs, flags = [], []
        for no_slots in (False, True):
            if no_slots:  # read at plan creation: drop the cached plan
                os.environ["CBN_NO_SLOTS"] = "1"
                bn.engine.invalidate()
            outs.append(bn.infer(target, ev, N_max=64)[0].cpu().numpy())
            flags += [int(lib.cbn_plan_flags(p.handle)) for p in bn.engine._plans.values()]
        res["flags"] = flags
        res["equal"] = bool(np.array_equal(outs[0], outs[1], equal_nan=True))
        res["nonzero_rows"] = int((outs[0] > 0).any(1).sum())
    elif mode == "gridcoal":
        # >= 3 block rounds (the raw launch + scale path): coalesced index phase
        # vs the per-lane loads, ragged batch, and a column view that is not
        # 16-B aligned (the coalesced phase declines it)
        from helpers import grid_data

        data, cols, edges = grid_data(100000, 7, side=5, d=64, keep=0.995, noise=0)
        target, names = cols[-1], cols[:-1]
        ev = {k: torch.tensor(v, device=dev) for k, v in sample_evidence(data, cols, names, 200003, 3).items()}
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev)
        outs = []
        for no_coal in (False, True):
            os.environ["CBN_SLOTS_NO_COAL"] = "1" if no_coal else "0"
            if not no_coal:
                os.environ.pop("CBN_SLOTS_NO_COAL")
            outs.append(bn.infer(target, ev, N_max=64)[0].cpu().numpy())
        off = {k: torch.cat([torch.zeros((1, 1), device=dev), v])[1:] for k, v in ev.items()}  # 4-B offset views
        outs.append(bn.infer(target, off, N_max=64)[0].cpu().numpy())
        res["flags"] = [int(lib.cbn_plan_flags(p.handle)) for p in bn.engine._plans.values()]
        res["equal"] = bool(np.array_equal(outs[0], outs[1], equal_nan=True))
        res["equal_unaligned"] = bool(np.array_equal(outs[0], outs[2], equal_nan=True))
        res["nonzero_rows"] = int((outs[0] > 0).any(1).sum())
        rows = np.append(np.arange(0, 200003, 5003)[:40], [200002, int(np.argmax(outs[0].max(1)))])
        np.save(os.environ["CBN_CHILD_OUT"], outs[0][rows])
        res["rows"] = rows.tolist()
    elif mode == "coalspecial":
        # special evidence values (helpers.special_batch) through k_query_slots'
        # coalesced index phase, forced at a small ragged batch (Q % 4 != 0: the
        # c4 + e < nv masking) by CBN_SLOTS_COAL=1, vs the per-lane phase:
        # dense domains and sorted non-integer ones; rows -> CBN_CHILD_OUT
        from helpers import grid_data, special_batch

        base, cols, edges = grid_data(100000, 7, side=3, d=64, keep=0.995, noise=0)
        target, names, Q = cols[-1], cols[:-1], 1001
        res["flags"], res["equal"], res["equal_raw"], keep = [], [], [], {}
        for tag in ("dense", "levels"):
            data = base if tag == "dense" else ((np.arange(64) - 2) * 0.25).astype(np.float32)[base.astype(np.int64)]
            doms = {c: np.unique(data[:, cols.index(c)]) for c in names}
            ev_np, _ = special_batch(sample_evidence(data, cols, names, Q, 5), doms)
            ev = {k: torch.tensor(v, device=dev) for k, v in ev_np.items()}
            bn = make_bn(BayesianNetwork, edges, cols, data, device=dev)
            outs, raws = [], []
            for coal in (False, True):  # read per launch
                os.environ.pop("CBN_SLOTS_COAL", None)
                if coal:
                    os.environ["CBN_SLOTS_COAL"] = "1"
                outs.append(bn.infer(target, ev, N_max=64)[0].cpu().numpy().copy())
                raws.append(bn.engine.infer_raw(target, ev, 64)[0].cpu().numpy().copy())
            res["flags"] += [int(lib.cbn_plan_flags(p.handle)) for p in bn.engine._plans.values()]
            res["equal"].append(bool(np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))))
            res["equal_raw"].append(bool(np.array_equal(raws[0].view(np.uint32), raws[1].view(np.uint32))))
            keep[tag] = outs[1]
        np.savez(os.environ["CBN_CHILD_OUT"], **keep)
    elif mode in ("paramlin", "paramh1"):
        # one parametric plan (tests/param_matrix.py DIAG_CASES, N = 40, all
        # evidence) under the CBN_PARAM_* switches: per setting the plan is
        # rebuilt (CBN_PARAM_NC / NO_M1 are read at plan creation, LIN8 /
        # PARTS per call), its cbn_plan_param_info recorded and its raw rows
        # compared bit for bit with the first setting of its group -- within
        # a group the factor split (parts) is the same, across groups it is
        # not, and the association of the product differs by design
        import tempfile

        import param_matrix as pm
        from test_gpu_param import load_fixture_params

        case = pm.DIAG_CASES[mode[5:]]
        data, cols, edges, target, _, params = pm.network(case)
        bn = make_bn(BayesianNetwork, edges, cols, data, device=dev, estimator=case.est,
                     config=param_config(case.est, n_epochs=1, model=case.model))
        with tempfile.TemporaryDirectory() as tmp:
            load_fixture_params(bn, {"meta": {"estimator": case.est}, "params": params}, tmp, dev)
        ev = {k: torch.tensor(v, device=dev) for k, v in pm.evidence(case, pm.SMALL).items()}
        if mode == "paramlin":  # (a linear plan launches 8 or 16 columns whatever CBN_PARAM_NC says: LIN8 picks 8)
            groups = [[{}, {"CBN_PARAM_LIN8": "1"}],
                      [{"CBN_PARAM_PARTS": "2"}, {"CBN_PARAM_PARTS": "2", "CBN_PARAM_LIN8": "1"},
                       {"CBN_PARAM_PARTS": "2", "CBN_PARAM_NO_M1": "1"}]]
        else:
            groups = [[{"CBN_PARAM_NC": "32"}, {"CBN_PARAM_NC": "16"}, {"CBN_PARAM_NC": "8"}],
                      [{"CBN_PARAM_PARTS": "2"}, {"CBN_PARAM_PARTS": "2", "CBN_PARAM_NO_M1": "1"},
                       {"CBN_PARAM_PARTS": "2", "CBN_PARAM_NO_M1": "1", "CBN_PARAM_NC": "16"}]]
        res["infos"], res["equal"], res["finite"] = [], [], []
        names = ("CBN_PARAM_NC", "CBN_PARAM_NO_M1", "CBN_PARAM_LIN8", "CBN_PARAM_PARTS")
        for group in groups:
            first = None
            for env in group:
                for n in names:
                    os.environ.pop(n, None)
                os.environ.update(env)
                bn.engine.invalidate()
                plan, _ = bn.engine.call_plan(target, ev, case.N)
                info = _native.param_info(plan.handle)
                raw = bn.engine.infer_raw(target, ev, case.N)[0].cpu().numpy().copy()
                first = raw if first is None else first
                res["infos"].append({k: info[k] for k in ("nc", "n_chunks", "hmax", "mode", "m1", "parts")})
                res["equal"].append(bool(np.array_equal(raw.view(np.uint32), first.view(np.uint32))))
                res["finite"].append(bool(np.isfinite(raw).all() and (raw > 0).any(1).all()))
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
