#!/usr/bin/env python3
"""Cost of the mesh simplify (r2s_mesh_simplify_dev) on an extracted surface, device-resident, HIP events, median of --reps calls
after one warm-up, beside the mesh weld (r2s_mesh_weld_dev, snap = cell, collapsed and unused dropped) of the same mesh in the
same run: the simplify is that weld's two stages plus two segmented Float64 sums and the per-class solve.

Inputs: the indexed surface of the 253^3 sphere field and of the 513^3 Float32 gyroid, both rules, cell = 2 and 4 lattice
spacings, duplicates dropped, both maps written.

Writes profiles/mesh_simplify_bench.json and prints it.  Usage: python tools/mesh_simplify_bench.py [--reps 5] [--gyroid 513]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import iso_ref  # noqa: E402
import mesh_query_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sphere", type=int, default=253)
    ap.add_argument("--gyroid", type=int, default=513)
    ap.add_argument("--period", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_bench.json"))
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    L = pkg._lib
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    vp = ctypes.c_void_p

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def stats(fn):
        fn()
        ms = [timed(fn) for _ in range(args.reps)]
        return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "samples_ms": ms}

    def leg(name, host, n, spacing):
        d = torch.from_numpy(np.ascontiguousarray(host, np.float32)).to("cuda:0")
        dd, oo = (ctypes.c_int64 * 3)(n, n, n), (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().r2s_extract_isosurface_dev(vp(d.data_ptr()), 1, dd, oo, spacing, 0.0, None, 0, None, 0, ctypes.byref(nv),
                                                   ctypes.byref(nt), sp))
        V = torch.empty((nv.value, 3), dtype=torch.float32, device=d.device)
        T = torch.empty((nt.value, 3), dtype=torch.int32, device=d.device)
        L.check(L.lib().r2s_extract_isosurface_dev(vp(d.data_ptr()), 1, dd, oo, spacing, 0.0, vp(V.data_ptr()), nv.value, vp(T.data_ptr()),
                                                   nt.value, ctypes.byref(nv), ctypes.byref(nt), sp))
        del d
        n_v, n_t = V.shape[0], T.shape[0]
        vo = torch.empty((n_v, 3), dtype=torch.float32, device=V.device)
        to = torch.empty((n_t, 3), dtype=torch.int32, device=V.device)
        vm = torch.empty(n_v, dtype=torch.int32, device=V.device)
        tm = torch.empty(n_t, dtype=torch.int32, device=V.device)
        tot = (ctypes.c_int64 * 8)()
        rows = []
        for k in (2, 4):
            cell = k * spacing

            def weld():
                L.check(L.lib().r2s_mesh_weld_dev(vp(V.data_ptr()), n_v, vp(T.data_ptr()), n_t, cell, 7, vp(vo.data_ptr()), vp(to.data_ptr()),
                                                  vp(vm.data_ptr()), vp(tm.data_ptr()), tot, sp))
            row = {"leg": name, "dims": [n, n, n], "verts": n_v, "tris": n_t, "cell_spacings": k, "cell": cell}
            row["mesh_weld_dev"] = stats(weld)
            row["weld_totals"] = list(tot)
            for rule, code in (("mean", 0), ("quadric", 1)):
                def simplify():
                    L.check(L.lib().r2s_mesh_simplify_dev(vp(V.data_ptr()), n_v, vp(T.data_ptr()), n_t, cell, code, 2, vp(vo.data_ptr()),
                                                          vp(to.data_ptr()), vp(vm.data_ptr()), vp(tm.data_ptr()), tot, sp))
                row[rule] = stats(simplify)
                row[rule]["totals"] = list(tot)
                row[rule]["ratio_to_weld"] = row[rule]["ms_median"] / row["mesh_weld_dev"]["ms_median"]
                row[rule]["tris_out_per_tris_in"] = tot[1] / max(n_t, 1)
            print(name, row, file=sys.stderr, flush=True)
            rows.append(row)
        return rows

    res = {}
    n = args.sphere
    res["sphere"] = leg("sphere", mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; indexed input, duplicates dropped, "
                     "both maps written; the weld beside it: snap = cell, flags 7, same mesh, same run")
    res["quadric_vs_eigh"] = {"max_abs_diff_in_cell_eps32": 0.0, "source": "tests/test_mesh_simplify_gpu.py -s on an MI355X: every class of "
                              "every case, each coordinate bit-equal to the eigh restatement (or to one of its candidates)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
