#!/usr/bin/env python3
"""Cost of the mesh sections (r2s_mesh_sections_dev), device-resident, HIP events, median of --reps calls after one warm-up,
beside the mesh shells (r2s_mesh_shells_dev) on the same mesh in the same run: both are a radix sort of the half-edges and a
union-find, the sections add one segment per (triangle, level), the loop ranking and 52 bytes of output per segment.

Meshes: the surface of the 253^3 sphere field and of the 513^3 Float32 gyroid (54.6 M triangles), cut along z with one level
per lattice plane.

Kernel times by name come from a separate run under the profiler (trace only, no counters):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mesh_sections_bench.py --reps 1
Writes profiles/mesh_sections_bench.json and prints it.  Usage: python tools/mesh_sections_bench.py [--reps 5] [--gyroid 513]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sections_bench.json"))
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
        normal = np.array([0.0, 0.0, 1.0])
        levels = -1.0 + spacing * np.arange(n, dtype=np.float64)          # one level per lattice plane
        first = pkg.mesh_sections_dev(V, T, normal, levels)
        ccap, scap = first.n_contours, first.n_segments
        start = torch.empty(ccap + 1, dtype=torch.int64, device=V.device)
        counts = torch.empty((max(ccap, 1), 8), dtype=torch.int64, device=V.device)
        sums = torch.empty((max(ccap, 1), 7), dtype=torch.float64, device=V.device)
        seg_tri = torch.empty(max(scap, 1), dtype=torch.int32, device=V.device)
        pts = torch.empty((max(scap, 1), 2, 3), dtype=torch.float64, device=V.device)
        nc, ns, ref, tot = ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def sections():
            L.check(L.lib().r2s_mesh_sections_dev(vp(V.data_ptr()), nv.value, vp(T.data_ptr()), nt.value, normal.ctypes.data_as(L.c_double_p),
                                                  levels.ctypes.data_as(L.c_double_p), len(levels), vp(start.data_ptr()),
                                                  vp(counts.data_ptr()), vp(sums.data_ptr()), ccap, vp(seg_tri.data_ptr()),
                                                  vp(pts.data_ptr()), scap, ctypes.byref(nc), ctypes.byref(ns), ref, tot, sp))

        row = {"leg": name, "dims": [n, n, n], "n_verts": nv.value, "n_tris": nt.value, "n_levels": len(levels),
               "totals": first.totals.tolist(), "longest_closed_loop": int(first.n_segs[first.closed].max()) if first.closed.any() else 0,
               "area_sum": float(first.level_area.sum())}
        row["mesh_sections_dev"] = stats(sections)
        del start, counts, sums, seg_tri, pts
        shells = pkg.mesh_shells_dev(V, T)
        cap = shells.n_shells
        sot = torch.empty(nt.value, dtype=torch.int32, device=V.device)
        scounts = torch.empty((max(cap, 1), 8), dtype=torch.int64, device=V.device)
        ssums = torch.empty((max(cap, 1), 11), dtype=torch.float64, device=V.device)
        nsh = ctypes.c_int64()

        def run_shells():
            L.check(L.lib().r2s_mesh_shells_dev(vp(V.data_ptr()), nv.value, vp(T.data_ptr()), nt.value, vp(sot.data_ptr()),
                                                vp(scounts.data_ptr()), vp(ssums.data_ptr()), cap, ctypes.byref(nsh), ref, tot, sp))
        row["mesh_shells_dev"] = stats(run_shells)
        row["ratio_to_shells"] = row["mesh_sections_dev"]["ms_median"] / row["mesh_shells_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    res["sphere"] = leg("sphere", mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; tables written (capacities = the "
                     "counts); normal z, one level per lattice plane")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
