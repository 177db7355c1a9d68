#!/usr/bin/env python3
"""Cost of the ray query of the mesh index (r2s_mesh_index_raycast_dev), device-resident, HIP events, median of --reps calls
after one warm-up, on the two meshes of tools/mesh_query_bench.py (the surface of the fitted sphere's Float32 fine field and of
the 513^3 Float32 gyroid):

(a) --rays random rays from inside the mesh box (uniform origins, normally distributed directions);
(b) --rays rays from a plane along one axis (origins on a square lattice below the box, direction +z: a coherent depth image);
(c) the thickness of every vertex (surface_thickness_dev with a given index; the normals are part of the call).
Each figure stands beside the nearest-point query (r2s_mesh_index_query_dev) of the same number of points from the same run.

Kernel times by name come from a separate run under the profiler (trace only, no counters):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ray_bench.py --reps 1
Writes profiles/ray_bench.json and prints it.  Usage: python tools/ray_bench.py [--reps 5] [--gyroid 513] [--rays 10000000]"""
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
    ap.add_argument("--sphere-grid", type=int, default=120)
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_bench.json"))
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    L = pkg._lib
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    dev = torch.device("cuda:0")

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

    def surface(host, dims, origin, spacing):
        d = torch.from_numpy(host).to(dev)
        dd, oo = (ctypes.c_int64 * 3)(*dims), (ctypes.c_double * 3)(*origin)
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        f32 = int(host.dtype == np.float32)
        L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0, None, 0, None, 0,
                                                   ctypes.byref(nv), ctypes.byref(nt), sp))
        V = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        T = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0, ctypes.c_void_p(V.data_ptr()),
                                                   nv.value, ctypes.c_void_p(T.data_ptr()), nt.value, ctypes.byref(nv), ctypes.byref(nt), sp))
        return V, T

    def leg(name, host, dims, origin, spacing):
        V, T = surface(host, dims, origin, spacing)
        lo, hi = V.min(dim=0).values, V.max(dim=0).values
        row = {"leg": name, "dims": list(dims), "n_verts": int(V.shape[0]), "n_tris": int(T.shape[0]), "n_rays": args.rays}
        with pkg.MeshIndex(V, T) as ix:
            row["index"] = ix.info()
            n = args.rays
            gen = torch.Generator(device=dev).manual_seed(1)
            o = lo + (hi - lo) * torch.rand((n, 3), dtype=torch.float32, device=dev, generator=gen)
            d = torch.randn((n, 3), dtype=torch.float32, device=dev, generator=gen)
            t = ix.raycast_dev(o, d, dtype=torch.float32)
            row["random_rays"] = dict(stats(lambda: ix.raycast_dev(o, d, dtype=torch.float32)), hit_fraction=float(torch.isfinite(t).float().mean()))
            row["random_rays"]["nearest_point_same_count"] = stats(lambda: ix.distance_dev(o, dtype=torch.float32))
            side = int(np.ceil(np.sqrt(n)))
            u = torch.linspace(0.0, 1.0, side, dtype=torch.float32, device=dev)
            gy, gx = torch.meshgrid(u, u, indexing="ij")
            po = torch.stack([lo[0] + (hi[0] - lo[0]) * gx.reshape(-1), lo[1] + (hi[1] - lo[1]) * gy.reshape(-1),
                              torch.full((side * side,), float(lo[2] - 0.5 * (hi[2] - lo[2])), dtype=torch.float32, device=dev)], dim=1)[:n].contiguous()
            pd = torch.zeros_like(po)
            pd[:, 2] = 1.0
            t = ix.raycast_dev(po, pd, dtype=torch.float32)
            row["depth_image"] = dict(stats(lambda: ix.raycast_dev(po, pd, dtype=torch.float32)), hit_fraction=float(torch.isfinite(t).float().mean()))
            row["depth_image"]["nearest_point_same_count"] = stats(lambda: ix.distance_dev(po, dtype=torch.float32))
            del o, d, po, pd, t
            skip = 0.5 * spacing
            th = pkg.surface_thickness_dev(V, T, skip=skip, index=ix)[0]
            fin = torch.isfinite(th)
            row["thickness"] = dict(stats(lambda: pkg.surface_thickness_dev(V, T, skip=skip, index=ix)), n_points=int(V.shape[0]),
                                    finite_fraction=float(fin.float().mean()), median=float(th[fin].median()) if bool(fin.any()) else None)
            nrm = torch.randn((V.shape[0], 3), dtype=torch.float64, device=dev)
            row["thickness"]["rays_alone_given_normals"] = stats(lambda: pkg.surface_thickness_dev(V, T, nrm, skip=skip, index=ix))
            row["thickness"]["nearest_point_same_count"] = stats(lambda: ix.distance_dev(V, dtype=torch.float32))
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    d = np.load(os.path.join(ROOT, "tests", "golden", "sphere.npz"))
    X, IEN, rho = d["X"], d["IEN"].astype(np.int64), d["rho"]
    grid = pkg.Grid(X.min(0), X.max(0), args.sphere_grid, 3)
    fine, _, _, _ = pkg.rho2sdf("bench", X, IEN, rho, options=pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine"), sdf_grid=grid)
    res["sphere_fine"] = leg("sphere_fine", np.ascontiguousarray(fine).ravel(), fine.shape[::-1], tuple(grid.AABB_min), grid.cell_size / 2)
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1))
    res["method"] = f"HIP events on the call's stream, median of {args.reps} after one warm-up call; Float32 rays and outputs"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
