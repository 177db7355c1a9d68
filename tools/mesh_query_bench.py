#!/usr/bin/env python3
"""Cost of the mesh index (r2s_mesh_index_*), device-resident, HIP events, median of --reps calls after one warm-up:

(a) build time and device bytes for the surface of the fitted sphere's Float32 fine field and of the 513^3 Float32 gyroid (the
    two legs of tools/redistance_bench.py);
(b) r2s_mesh_index_lattice_dev on both lattices, beside r2s_redistance_dev at bands of 2 and 16 cells in the same run (that
    call also extracts the surface; its own phases are listed so that the tile kernel can be compared alone);
(c) 10^7 uniformly random Float32 points in the gyroid's box;
(d) the vertices of the smoothed sphere surface against the raw surface (what surface_deviation runs).

Kernel times by name come from a separate run under the profiler (trace only, no counters):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mesh_query_bench.py --reps 1
Writes profiles/mesh_query_bench.json and prints it.  Usage: python tools/mesh_query_bench.py [--reps 5] [--gyroid 513]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gyroid", type=int, default=513)
    ap.add_argument("--period", type=int, default=24)
    ap.add_argument("--bands", type=float, nargs="+", default=[2, 16])
    ap.add_argument("--sphere-grid", type=int, default=120)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_query_bench.json"))
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    L = pkg._lib
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)

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

    def leg(name, host, dims, origin, spacing):
        d = torch.from_numpy(host).to("cuda:0")
        lat = (dims, origin, spacing)
        dd, oo = (ctypes.c_int64 * 3)(*dims), (ctypes.c_double * 3)(*origin)
        # the surface on the device, through the lattice form of the C ABI
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        f32 = int(host.dtype == np.float32)
        L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0, None, 0, None, 0,
                                                   ctypes.byref(nv), ctypes.byref(nt), sp))
        V = torch.empty((nv.value, 3), dtype=torch.float32, device=d.device)
        T = torch.empty((nt.value, 3), dtype=torch.int32, device=d.device)
        L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0, ctypes.c_void_p(V.data_ptr()),
                                                   nv.value, ctypes.c_void_p(T.data_ptr()), nt.value, ctypes.byref(nv), ctypes.byref(nt), sp))
        row = {"leg": name, "dims": list(dims), "dtype": str(host.dtype), "n_verts": nv.value, "n_tris": nt.value}
        row["build"] = stats(lambda: pkg.MeshIndex(V, T).close())
        ix = pkg.MeshIndex(V, T)
        row["index"] = ix.info()
        out = torch.empty(dims[::-1], dtype=torch.float32, device=d.device)

        def lattice():
            L.check(L.lib().r2s_mesh_index_lattice_dev(ix._handle(), dd, oo, spacing, 1, ctypes.c_void_p(out.data_ptr()), None, sp))
        row["lattice_query"] = stats(lattice)
        row["redistance_full_dev"] = stats(lambda: pkg.redistance_full_dev(d.view(dims[::-1]), lat))
        row["banded"] = []
        for cells in args.bands:
            def run():
                L.check(L.lib().r2s_redistance_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0, cells * spacing,
                                                   ctypes.c_void_p(out.data_ptr()), sp))
            r = stats(run)
            r.update(band_cells=cells, **{k: v for k, v in pkg.last_distance_stats().items() if k.startswith("ms_") or k == "pairs"})
            row["banded"].append(r)
        print(name, row, file=sys.stderr, flush=True)
        return row, ix, V, T

    res = {}
    d = np.load(os.path.join(ROOT, "tests", "golden", "sphere.npz"))
    X, IEN, rho = d["X"], d["IEN"].astype(np.int64), d["rho"]
    grid = pkg.Grid(X.min(0), X.max(0), args.sphere_grid, 3)
    fine, _, _, raw = pkg.rho2sdf("bench", X, IEN, rho, options=pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine"), sdf_grid=grid)
    res["sphere_fine"], ix_s, Vs, Ts = leg("sphere_fine", np.ascontiguousarray(fine).ravel(), fine.shape[::-1], tuple(grid.AABB_min),
                                           grid.cell_size / 2)
    # (d) the vertices of the smoothed surface against the raw surface
    Vr, Tr = pkg.extract_isosurface(raw, grid, None)
    with pkg.MeshIndex(Vr, Tr) as ix_r:
        res["smoothed_vertices_against_raw_surface"] = dict(stats(lambda: ix_r.distance_dev(Vs)), n_points=int(Vs.shape[0]),
                                                            n_tris=int(len(Tr)), max=float(ix_r.distance_dev(Vs).max()))
    ix_s.close()
    del Vs, Ts
    n = args.gyroid
    res["gyroid"], ix_g, Vg, Tg = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1))
    # (c) random points in the gyroid's box
    P = torch.rand((args.points, 3), dtype=torch.float32, device="cuda:0") * 2.0 - 1.0
    res["random_points"] = dict(stats(lambda: ix_g.distance_dev(P, dtype=torch.float32)), n_points=args.points, n_tris=int(Tg.shape[0]))
    ix_g.close()
    res["method"] = f"HIP events on the call's stream, median of {args.reps} after one warm-up call; Float32 outputs"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
