"""Census of table plans: what cbn_plan_create decides for every case of
tests/table_plan_cases.py, one JSON line per case.

    python tools/plan_census.py [--lib LIB] [--cases a,b] [--out FILE]
        creates each plan (no query is launched) and prints its descriptors'
        integers, the device's CU count, cbn_plan_flags, cbn_plan_table_bytes,
        cbn_plan_uses_lds, cbn_plan_max_words and cbn_plan_fused_capacity.
        Uses only entry points every ABI has: --lib may name a library built
        from another commit (tools/build_variant.sh), to compare line by line.
    python tools/plan_census.py --info [--n-cu 256]
        the same five values from cbn_table_plan_info (ABI 6): no GPU needed.
    python tools/plan_census.py --both
        both, with the device's CU count ("plan" and "info" per case).
    python tools/plan_census.py --launch [--lib LIB]
        per case with a fast-path plan, at 1 query and at fused capacity + 1:
        cbn_plan_run fused, CBN_RUN_TWO_PASS, CBN_RUN_RAW + cbn_scale and
        cbn_plan_run_argmax over zeroed tables -- for a kernel trace, which
        shows each launch's instantiation, grid and LDS request.
    python tools/plan_census.py --compare-traces A_kernel_trace.csv B_kernel_trace.csv [--out-prefix P]
        the two traces' sequences of (kernel, grid, workgroup, LDS) must be
        equal; writes those four columns of each to P_a.csv / P_b.csv.
    python tools/plan_census.py --create-loop 200 --cases bench_chain20_d32
        seconds per cbn_plan_create + cbn_plan_destroy.

The diagnostic switches of a case are set in this process's environment before
its plan is made (the library reads them per plan under CBN_DIAG=1); without
CBN_DIAG=1 the tool runs itself in a child process that has it.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCHES = ("CBN_FAST_VPL", "CBN_NO_PAIRED", "CBN_NO_PREFIX", "CBN_NO_LDS_SPLIT", "CBN_NO_SLOTS", "CBN_NO_STAGED",
            "CBN_NO_COLS", "CBN_NO_FUSED", "CBN_SLOTS_BPC")
RUN_TWO_PASS, RUN_RAW = 4, 8
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


def load(path):
    """The library with the signatures the census needs (present in every ABI)."""
    import torch  # noqa: F401  (maps the HIP runtime the library links)

    if path is None:
        from continuousbayesiannetwork_amd import _native

        _native.load()  # (its stamp check: this tree's build)
        path = _native.LIB_PATH
    lib = ctypes.CDLL(path)
    for name, res, args in (
            ("cbn_plan_create", ctypes.c_int, [vp, i32, i32, ctypes.POINTER(vp)]),
            ("cbn_plan_destroy", ctypes.c_int, [vp]), ("cbn_plan_flags", i32, [vp]),
            ("cbn_plan_table_bytes", i64, [vp]), ("cbn_plan_uses_lds", ctypes.c_int, [vp]),
            ("cbn_plan_max_words", i32, [vp]), ("cbn_plan_fused_capacity", i64, [vp]),
            ("cbn_last_error", ctypes.c_char_p, []),
            ("cbn_plan_run", ctypes.c_int, [vp, i64, vp, i32, vp, vp, i32, vp]),
            ("cbn_scale", ctypes.c_int, [vp, i64, vp, i32, vp]),
            ("cbn_plan_run_argmax", ctypes.c_int, [vp, i64, vp, i32, vp, vp, vp, vp, vp, i32, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def set_switches(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


class Device:
    """Device buffers of a case: the slots' domains (dense 0..card-1 on even
    slots, sorted non-integer levels on odd ones) and one dummy for the rest."""

    def __init__(self):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.dummy = torch.zeros(64, device=self.dev)
        self.n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count
        self.doms = {}

    def domain(self, card, slot):
        key = (card, slot & 1)
        if key not in self.doms:
            a = self.torch.arange(card, dtype=self.torch.float32, device=self.dev)
            self.doms[key] = (a - 2) * 0.25 if slot & 1 else a
        return self.doms[key]


def create(lib, case, device, tpc):
    cards = tpc.slot_cards(case)
    descs = tpc.descriptors(case, tpc.factor_desc_type(), device.dummy.data_ptr(),
                            lambda s: device.domain(cards[s], s).data_ptr())
    handle = vp()
    rc = lib.cbn_plan_create(ctypes.cast(descs, vp), len(case.factors), case.N, ctypes.byref(handle))
    if rc:
        raise RuntimeError(f"{case.name}: cbn_plan_create rc={rc}: {lib.cbn_last_error().decode()}")
    device.torch.cuda.synchronize()
    return handle


def plan_values(lib, h):
    return {"flags": int(lib.cbn_plan_flags(h)), "table_bytes": int(lib.cbn_plan_table_bytes(h)),
            "uses_lds": int(lib.cbn_plan_uses_lds(h)), "max_words": int(lib.cbn_plan_max_words(h)),
            "fused_capacity": int(lib.cbn_plan_fused_capacity(h))}


def info_values(case, n_cu, tpc):
    from continuousbayesiannetwork_amd import _native

    descs = tpc.descriptors(case, _native.FactorDesc)
    i = _native.table_plan_info(descs, len(case.factors), case.N, n_cu)
    return {"flags": i["flags"], "table_bytes": i["table_bytes"], "uses_lds": 1 if i["flags"] & _native.CBN_PLAN_LDS else 0,
            "max_words": i["max_slots"], "fused_capacity": i["fused_capacity"],
            "kernel": _native.TABLE_KERNELS[i["kernel"]],
            **{k: i[k] for k in ("vpl", "lanes", "row_stride", "prefix", "lds_tab_floats", "lds_bytes",
                                 "blocks_per_cu", "fused_candidate")}}


def launch(lib, case, h, device, tpc):
    """The four call paths at 1 query and at fused capacity + 1 (tables left zero: the rows are NaN, the launches real)."""
    torch = device.torch
    cards = tpc.slot_cards(case)
    ns, cap = len(cards), int(lib.cbn_plan_fused_capacity(h))
    if not lib.cbn_plan_max_words(h):
        return  # generic plan: no raw launch, no fused launch
    words = torch.zeros(1024, dtype=torch.int32, device=device.dev)
    stream = vp(torch.cuda.current_stream(device.dev).cuda_stream)
    for Q in (1, cap + 1):
        g = torch.Generator().manual_seed(Q)
        cols = [device.domain(c, s)[torch.randint(0, c, (Q,), generator=g).to(device.dev)].contiguous()
                for s, c in enumerate(cards)]
        ev = (vp * max(ns, 1))(*[c.data_ptr() for c in cols])
        out = torch.empty((Q, case.N), device=device.dev)
        idx = torch.empty(Q, dtype=torch.int32, device=device.dev)
        val, rmax = torch.empty(Q, device=device.dev), torch.empty(Q, device=device.dev)
        run = lambda flags: lib.cbn_plan_run(h, Q, ev, ns, words.data_ptr(), out.data_ptr(), flags, stream)  # noqa: E731
        rcs = [run(0), run(RUN_TWO_PASS), run(RUN_RAW),
               lib.cbn_scale(out.data_ptr(), Q * case.N, words.data_ptr(), lib.cbn_plan_max_words(h), stream),
               lib.cbn_plan_run_argmax(h, Q, ev, ns, None, idx.data_ptr(), val.data_ptr(), rmax.data_ptr(), None, 0, stream)]
        torch.cuda.synchronize()
        if any(rcs):
            raise RuntimeError(f"{case.name} Q={Q}: rc {rcs}: {lib.cbn_last_error().decode()}")


def compare_traces(a, b, prefix):
    import csv

    seqs = []
    for path, tag in ((a, "a"), (b, "b")):
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        seq = [(r["Kernel_Name"], "x".join(r[f"Grid_Size_{d}"] for d in "XYZ"),
                "x".join(r[f"Workgroup_Size_{d}"] for d in "XYZ"), r["LDS_Block_Size"]) for r in rows]
        seqs.append(seq)
        if prefix:
            with open(f"{prefix}_{tag}.csv", "w", newline="") as fh:
                w = csv.writer(fh)
                w.writerow(["kernel", "grid", "workgroup", "lds_block_size"])
                w.writerows(seq)
    diff = [i for i, (x, y) in enumerate(zip(*seqs)) if x != y]
    ours = sum(1 for r in seqs[0] if "k_query" in r[0])
    print(json.dumps({"launches_a": len(seqs[0]), "launches_b": len(seqs[1]), "query_kernel_launches_a": ours,
                      "distinct_query_kernels_a": len({r[0] for r in seqs[0] if "k_query" in r[0]}),
                      "first_difference": diff[:1], "equal": seqs[0] == seqs[1]}))
    for i in diff[:5]:
        print(seqs[0][i], "!=", seqs[1][i])
    return 0 if seqs[0] == seqs[1] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare-traces", nargs=2)
    ap.add_argument("--out-prefix")
    ap.add_argument("--lib")
    ap.add_argument("--cases")
    ap.add_argument("--out")
    ap.add_argument("--info", action="store_true")
    ap.add_argument("--both", action="store_true")
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--n-cu", type=int, default=256)
    ap.add_argument("--create-loop", type=int, default=0)
    a = ap.parse_args()
    if a.compare_traces:
        return compare_traces(*a.compare_traces, a.out_prefix)
    if os.environ.get("CBN_DIAG") != "1":
        return subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:]],
                              env={**os.environ, "CBN_DIAG": "1"}).returncode
    import table_plan_cases as tpc

    cases = [tpc.BY_NAME[n] for n in a.cases.split(",")] if a.cases else tpc.CASES
    out = open(a.out, "w") if a.out else sys.stdout
    gpu = not a.info
    lib = load(a.lib) if gpu else None
    device = Device() if gpu else None
    for case in cases:
        set_switches(case.env)
        rec = {"name": case.name, "N": case.N, "env": case.env, "factors": case.factors}
        if a.info or a.both:
            rec["info"] = info_values(case, device.n_cu if gpu else a.n_cu, tpc)
            rec["n_cu"] = device.n_cu if gpu else a.n_cu
        if gpu:
            h = create(lib, case, device, tpc)
            rec["n_cu"] = device.n_cu
            if a.both:
                rec["plan"] = plan_values(lib, h)
            elif a.launch:
                launch(lib, case, h, device, tpc)
                rec = {"name": case.name, "launched": bool(lib.cbn_plan_max_words(h))}
            elif a.create_loop:
                lib.cbn_plan_destroy(h)
                t0 = time.perf_counter()
                for _ in range(a.create_loop):
                    h = create(lib, case, device, tpc)
                    lib.cbn_plan_destroy(h)
                rec = {"name": case.name, "create_destroy_us": (time.perf_counter() - t0) / a.create_loop * 1e6}
                h = None
            else:
                rec.update(plan_values(lib, h))
            if h:
                lib.cbn_plan_destroy(h)
        print(json.dumps(rec), file=out, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
