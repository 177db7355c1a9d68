#!/usr/bin/env python3
"""Cost of the mesh holes (r2s_mesh_holes_dev), device-resident, tables written, HIP events, median of --reps whole calls after
one warm-up, beside the mesh shells (r2s_mesh_shells_dev) on the same mesh in the same run: both sort the half-edges once; the
holes then work on the boundary half-edges only (a second sort of their ends by vertex, a union-find, pointer jumping over the
closed rims, a third sort into output order), where the shells work on all triangles.

Inputs: the surface of the 253^3 sphere field with 1 000 isolated triangles deleted (1 000 closed rims of 3 edges), report only
and filled; the 513^3 Float32 gyroid as extracted, report only: its rims lie at the lattice border, and the longest closed one
sets the number of jumping rounds.  No time is fixed in advance: the yardstick is the shells' time, the ratio is reported.

Writes profiles/mesh_holes_bench.json and prints it.  Usage: python tools/mesh_holes_bench.py [--reps 5] [--gyroid 513]"""
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
import mesh_holes_cases  # noqa: E402
import mesh_query_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sphere", type=int, default=253)
    ap.add_argument("--gyroid", type=int, default=513)
    ap.add_argument("--period", type=int, default=24)
    ap.add_argument("--deleted", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_holes_bench.json"))
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

    def leg(name, V, T, dims, fills):
        first = pkg.mesh_holes_dev(V, T, fill=-1 if True in fills else None)
        nr, nb = first.n_rims, len(first.rim_edge)
        nvo, nto = (len(first.verts), len(first.tris)) if first.verts is not None else (0, 0)
        longest = int(first.n_edges[first.closed].max(initial=0))
        del first
        rcap, ecap = max(nr, 1), max(nb, 1)
        dev = T.device
        start = torch.empty(rcap + 1, dtype=torch.int64, device=dev)
        counts = torch.empty((rcap, 8), dtype=torch.int64, device=dev)
        sums = torch.empty((rcap, 7), dtype=torch.float64, device=dev)
        edge = torch.empty(ecap, dtype=torch.int32, device=dev)
        to = torch.empty((max(nto, 1), 3), dtype=torch.int32, device=dev)
        vo = torch.empty((max(nvo, 1), 3), dtype=torch.float32, device=dev)
        sc = [ctypes.c_int64() for _ in range(4)]
        ref, tot = (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def holes(fill):
            def run():
                L.check(L.lib().r2s_mesh_holes_dev(vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), -1, vp(start.data_ptr()),
                                                   vp(counts.data_ptr()), vp(sums.data_ptr()), rcap, vp(edge.data_ptr()), ecap,
                                                   vp(to.data_ptr()) if fill else None, vp(vo.data_ptr()) if fill else None,
                                                   nvo if fill else 0, nto if fill else 0, *[ctypes.byref(x) for x in sc], ref, tot, sp))
            return run
        row = {"leg": name, "dims": dims, "verts": len(V), "tris": len(T), "longest_closed_rim": longest}
        for fill in fills:
            key = "mesh_holes_dev_fill" if fill else "mesh_holes_dev"
            row[key] = stats(holes(fill))
            row["totals_fill" if fill else "totals"] = list(tot)
        row["n_rims"], row["n_edges"], row["n_verts_out"], row["n_tris_out"] = (x.value for x in sc)
        del start, counts, sums, edge, to, vo
        shells0 = pkg.mesh_shells_dev(V, T)
        scap = max(shells0.n_shells, 1)
        del shells0
        sot = torch.empty(len(T), dtype=torch.int32, device=dev)
        scounts = torch.empty((scap, 8), dtype=torch.int64, device=dev)
        ssums = torch.empty((scap, 11), dtype=torch.float64, device=dev)
        ns, sref, stot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def shells():
            L.check(L.lib().r2s_mesh_shells_dev(vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), vp(sot.data_ptr()),
                                                vp(scounts.data_ptr()), vp(ssums.data_ptr()), scap, ctypes.byref(ns), sref, stot, sp))
        row["mesh_shells_dev"] = stats(shells)
        row["shells_totals"] = list(stot)
        for fill in fills:
            key = "mesh_holes_dev_fill" if fill else "mesh_holes_dev"
            row["ratio_to_shells" + key[len("mesh_holes_dev"):]] = row[key]["ms_median"] / row["mesh_shells_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    V, T = extract(mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    T = torch.from_numpy(mesh_holes_cases._delete_isolated(T.cpu().numpy(), args.deleted, 0, 9)).to(V.device)
    res["sphere_holes"] = leg("sphere_holes", V, T, [n, n, n], (False, True))
    del V, T
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    V, T = extract(iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["gyroid"] = leg("gyroid", V, T, [n, n, n], (False,))
    del V, T
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} whole calls after one warm-up call; rim_start, rim_edge, the "
                     "records and the sums written, with and without the fill; shells on the same mesh, tables written")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
