#!/usr/bin/env python3
"""Cost of the mesh fans (r2s_mesh_fans_dev), device-resident, HIP events, median of --reps calls after one warm-up, with and
without the split, beside the mesh shells (r2s_mesh_shells_dev) on the same mesh in the same run: both sort the half-edges once
and run one union pass; the fans work on a union-find of the 3 n_tris corners and sort the fans by vertex where the shells sort
the triangles by shell.

Inputs: the surface of the 253^3 sphere field and of the 513^3 Float32 gyroid (54.6 M triangles), each as extracted (every vertex
has one fan), and the gyroid welded with snap = 0, which is where pinched vertices occur.  No time is fixed in advance: the
yardstick is the shells' time, the ratio is reported.

Writes profiles/mesh_fans_bench.json and prints it.  Usage: python tools/mesh_fans_bench.py [--reps 5] [--gyroid 513]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_fans_bench.json"))
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
        first = pkg.mesh_fans_dev(V, T)
        nf, nvo = first.n_fans, first.n_verts_out
        del first
        fcap, vcap = max(nf, 1), max(nvo, 1)
        foc = torch.empty((len(T), 3), dtype=torch.int32, device=T.device)
        fov = torch.empty(len(V), dtype=torch.int32, device=T.device)
        counts = torch.empty((fcap, 8), dtype=torch.int64, device=T.device)
        to = torch.empty_like(T)
        vo = torch.empty((vcap, 3), dtype=torch.float32, device=T.device)
        vof = torch.empty(vcap, dtype=torch.int32, device=T.device)
        n, nv_out, tot = ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_int64 * 8)()

        def fans(split):
            def run():
                L.check(L.lib().r2s_mesh_fans_dev(vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), vp(foc.data_ptr()), vp(fov.data_ptr()),
                                                  vp(counts.data_ptr()), fcap, vp(to.data_ptr()) if split else None,
                                                  vp(vo.data_ptr()) if split else None, vp(vof.data_ptr()) if split else None,
                                                  vcap if split else 0, ctypes.byref(n), ctypes.byref(nv_out), tot, sp))
            return run
        row = {"leg": name, "dims": dims, "verts": len(V), "tris": len(T)}
        row["mesh_fans_dev"] = stats(fans(False))
        row["mesh_fans_dev_split"] = stats(fans(True))
        row["totals"] = list(tot)
        row["n_fans"], row["n_verts_out"] = n.value, nv_out.value
        row["split_is_a_copy_of_the_triangles"] = bool(torch.equal(to, T))
        del foc, fov, counts, to, vo, vof
        shells0 = pkg.mesh_shells_dev(V, T)
        scap = max(shells0.n_shells, 1)
        del shells0
        sot = torch.empty(len(T), dtype=torch.int32, device=T.device)
        scounts = torch.empty((scap, 8), dtype=torch.int64, device=T.device)
        sums = torch.empty((scap, 11), dtype=torch.float64, device=T.device)
        ns, sref, stot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def shells():
            L.check(L.lib().r2s_mesh_shells_dev(vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), vp(sot.data_ptr()),
                                                vp(scounts.data_ptr()), vp(sums.data_ptr()), scap, ctypes.byref(ns), sref, stot, sp))
        row["mesh_shells_dev"] = stats(shells)
        row["shells_totals"] = list(stot)
        for k in ("mesh_fans_dev", "mesh_fans_dev_split"):
            row["ratio_to_shells" + k[len("mesh_fans_dev"):]] = row[k]["ms_median"] / row["mesh_shells_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    V, T = extract(mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    res["sphere"] = leg("sphere", V, T, [n, n, n])
    del V, T
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    V, T = extract(iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["gyroid"] = leg("gyroid", V, T, [n, n, n])
    pkg._lib.lib().r2s_release_cache()
    w = pkg.mesh_weld_dev(V, T, snap=0.0)
    del V, T
    WV, WT = w.verts.contiguous(), w.tris.contiguous()
    weld_totals = [int(x) for x in w.totals]
    del w
    pkg._lib.lib().r2s_release_cache()
    res["gyroid_welded"] = leg("gyroid_welded", WV, WT, [n, n, n])
    res["gyroid_welded"]["weld_totals"] = weld_totals
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; fan_of_corner, fans_of_vert and the "
                     "records written, with and without the split; shells on the same mesh, tables written")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
