#!/usr/bin/env python3
"""Cost of the mesh weld (r2s_mesh_weld_dev) on a triangle soup, device-resident, HIP events, median of --reps calls after one
warm-up, beside the mesh shells (r2s_mesh_shells_dev) on the welded mesh in the same run: both are dominated by radix sorts.

Inputs: the soup (three vertices per triangle, nothing shared: what an STL file holds) of the surface of the 253^3 sphere field
and of the 513^3 Float32 gyroid (54.6 M triangles, a soup of 164 M vertices).  snap = 0, flags DROP_COLLAPSED | DROP_UNUSED.
bytes_sorted counts the records that go through the four radix sorts: per vertex a (32-bit key, index) and a (64-bit key,
index) record, per triangle the same two, 20 bytes each way.

Writes profiles/mesh_weld_bench.json and prints it.  Usage: python tools/mesh_weld_bench.py [--reps 5] [--gyroid 513]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_weld_bench.json"))
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
        soup = V[T.reshape(-1).long()].contiguous()
        del V, T
        ns_v, ns_t = soup.shape[0], soup.shape[0] // 3
        vo = torch.empty((ns_v, 3), dtype=torch.float32, device=soup.device)
        to = torch.empty((ns_t, 3), dtype=torch.int32, device=soup.device)
        vm = torch.empty(ns_v, dtype=torch.int32, device=soup.device)
        tm = torch.empty(ns_t, dtype=torch.int32, device=soup.device)
        tot = (ctypes.c_int64 * 8)()

        def weld():
            L.check(L.lib().r2s_mesh_weld_dev(vp(soup.data_ptr()), ns_v, None, ns_t, 0.0, 5, vp(vo.data_ptr()), vp(to.data_ptr()),
                                              vp(vm.data_ptr()), vp(tm.data_ptr()), tot, sp))
        row = {"leg": name, "dims": [n, n, n], "soup_verts": ns_v, "soup_tris": ns_t, "bytes_sorted": 20 * (ns_v + ns_t)}
        row["mesh_weld_dev"] = stats(weld)
        row["totals"] = list(tot)
        W, Tw = vo[:tot[0]].contiguous(), to[:tot[1]].contiguous()
        first = pkg.mesh_shells_dev(W, Tw)
        cap = first.n_shells
        sot = torch.empty(len(Tw), dtype=torch.int32, device=soup.device)
        counts = torch.empty((max(cap, 1), 8), dtype=torch.int64, device=soup.device)
        sums = torch.empty((max(cap, 1), 11), dtype=torch.float64, device=soup.device)
        ns, ref, stot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def shells():
            L.check(L.lib().r2s_mesh_shells_dev(vp(W.data_ptr()), len(W), vp(Tw.data_ptr()), len(Tw), vp(sot.data_ptr()),
                                                vp(counts.data_ptr()), vp(sums.data_ptr()), cap, ctypes.byref(ns), ref, stot, sp))
        row["welded_verts"], row["welded_tris"], row["shells"] = len(W), len(Tw), cap
        row["closed_shells"] = int(first.closed.sum())
        row["mesh_shells_dev"] = stats(shells)
        row["ratio_to_shells"] = row["mesh_weld_dev"]["ms_median"] / row["mesh_shells_dev"]["ms_median"]
        row["sorted_gb_per_s"] = row["bytes_sorted"] / row["mesh_weld_dev"]["ms_median"] * 1e-6
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    res["sphere"] = leg("sphere", mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; soup input (tris = NULL), "
                     "snap 0, flags DROP_COLLAPSED | DROP_UNUSED, both maps written; shells on the welded mesh, tables written")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
