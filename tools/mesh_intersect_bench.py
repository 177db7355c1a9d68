#!/usr/bin/env python3
"""Cost of the self-intersection check (r2s_mesh_index_intersections_dev), device-resident, HIP events, median of --reps calls
after one warm-up, beside the index build (r2s_mesh_index_build_dev) on the same mesh in the same run: the check walks the tree
the build makes, once for the counts and once more for the pair list when there are pairs.

Cases: (a) the surface of the 253^3 sphere field: clean, 0 pairs expected; (b) the surface of the 513^3 Float32 gyroid;
(c) the sphere plus a copy translated by half a radius: a real intersection curve.  Per case: milliseconds with the pair list
written and for the counts alone, candidate pairs, intersecting pairs, and the ratio to the build.  No time is fixed in advance.

Writes profiles/mesh_intersect_bench.json and prints it.  Usage: python tools/mesh_intersect_bench.py [--reps 5] [--gyroid 513]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_intersect_bench.json"))
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

    def extract(host, n, spacing):
        d = torch.from_numpy(np.ascontiguousarray(host, np.float32)).to("cuda:0")
        dd, oo = (ctypes.c_int64 * 3)(n, n, n), (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().r2s_extract_isosurface_dev(vp(d.data_ptr()), 1, dd, oo, spacing, 0.0, None, 0, None, 0, ctypes.byref(nv),
                                                   ctypes.byref(nt), sp))
        V = torch.empty((nv.value, 3), dtype=torch.float32, device=d.device)
        T = torch.empty((nt.value, 3), dtype=torch.int32, device=d.device)
        L.check(L.lib().r2s_extract_isosurface_dev(vp(d.data_ptr()), 1, dd, oo, spacing, 0.0, vp(V.data_ptr()), nv.value, vp(T.data_ptr()),
                                                   nt.value, ctypes.byref(nv), ctypes.byref(nt), sp))
        return V, T

    def leg(name, V, T, dims):
        handles = []

        def build():
            h = ctypes.c_void_p()
            L.check(L.lib().r2s_mesh_index_build_dev(vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), sp, ctypes.byref(h)))
            handles.append(h)
            while len(handles) > 1:
                L.lib().r2s_mesh_index_destroy(handles.pop(0))
        row = {"leg": name, "dims": dims, "verts": len(V), "tris": len(T)}
        row["mesh_index_build_dev"] = stats(build)
        h = handles[0]
        info = (ctypes.c_int64 * 4)()
        L.check(L.lib().r2s_mesh_index_info(h, info))
        row["tree_depth"] = int(info[2])
        tot = (ctypes.c_int64 * 8)()
        hits = torch.empty(len(T), dtype=torch.int32, device=T.device)
        L.check(L.lib().r2s_mesh_index_intersections_dev(h, vp(hits.data_ptr()), None, 0, tot, sp))
        cap = max(int(tot[0]), 1)
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=T.device)

        def check(capacity):
            def run():
                L.check(L.lib().r2s_mesh_index_intersections_dev(h, vp(hits.data_ptr()), vp(pairs.data_ptr()) if capacity else None,
                                                                 capacity, tot, sp))
            return run
        row["intersections_dev_counts_only"] = stats(check(0))
        row["intersections_dev_with_pairs"] = stats(check(cap))
        row["totals"] = list(tot)
        row["candidate_pairs"], row["intersecting_pairs"] = int(tot[2]), int(tot[0])
        row["first_pairs"] = pairs[:min(int(tot[0]), 4)].cpu().tolist()
        row["ratio_to_build"] = row["intersections_dev_with_pairs"]["ms_median"] / row["mesh_index_build_dev"]["ms_median"]
        L.lib().r2s_mesh_index_destroy(h)
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    radius = 0.4 * (n - 1)
    V, T = extract(mesh_query_cases.sphere_field(n, radius, np.float32), n, 2.0 / (n - 1))
    res["sphere"] = leg("sphere", V, T, [n, n, n])
    shift = torch.tensor([0.48, 0.6, 0.64], dtype=torch.float32, device=V.device) * (0.5 * radius * 2.0 / (n - 1))
    V2, T2 = torch.cat([V, V + shift]).contiguous(), torch.cat([T, T + len(V)]).contiguous()
    res["two_spheres"] = leg("two_spheres", V2, T2, [n, n, n])
    del V, T, V2, T2
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    V, T = extract(iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["gyroid"] = leg("gyroid", V, T, [n, n, n])
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; the index is built once per "
                     "timed build and kept for the check; hits_of_tri written; 'with_pairs': capacity = the number of pairs (the "
                     "counting and the listing traversal, the sort); 'counts_only': capacity 0 (one traversal); lanes take triangles "
                     "in index order")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
