#!/usr/bin/env python3
"""Cost of the iso-surface extraction, timed with HIP events on the call's stream after warm-up (median of --reps):

* r2s_extract_isosurface_dev (count + scan + emit, the field already on the device) on a 513^3 Float32 gyroid and on
  the Float64 raw field of bench.py's NS workload (synthetic.hex_mesh, threshold 0.5, as tools/components_bench.py);
  bytes moved against the one-read floor of the field, and the share of 8 TB/s that one read at the measured time is;
* ms_total of r2s_rho2sdf with extract_surface off and on (bench.py's rho2sdf leg, alternated);
* the numpy reference of the vertices (tests/iso_ref.py) on the same fields, for the CPU comparison.

Prints one JSON line.  Usage: python tools/surface_bench.py [--reps 10] [--grid 512] [--gyroid 513]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import iso_ref  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--mesh", type=int, default=46)
    ap.add_argument("--gyroid", type=int, default=513)
    ap.add_argument("--period", type=int, default=24)
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    from rho2sdf_jl_amd import synthetic
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

    def leg(name, host, dims, origin, spacing):
        d = torch.from_numpy(host).to("cuda:0")
        dd = (ctypes.c_int64 * 3)(*dims)
        oo = (ctypes.c_double * 3)(*origin)
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        f32 = int(host.dtype == np.float32)
        L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0, None, 0, None, 0,
                                                   ctypes.byref(nv), ctypes.byref(nt), sp))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device="cuda:0")
        tris = torch.empty((nt.value, 3), dtype=torch.int32, device="cuda:0")

        def run():
            L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(d.data_ptr()), f32, dd, oo, spacing, 0.0,
                                                       ctypes.c_void_p(verts.data_ptr()), nv.value, ctypes.c_void_p(tris.data_ptr()),
                                                       nt.value, ctypes.byref(nv), ctypes.byref(nt), sp))
        run()
        run()
        ms = [timed(run) for _ in range(args.reps)]
        med = float(np.median(ms))
        field = host.nbytes
        out = 12 * nv.value + 12 * nt.value
        t0 = time.perf_counter()
        ref, _ = iso_ref.vertices(host, dims, origin, spacing, 0.0)
        ms_numpy = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(ref.view(np.uint32), verts.cpu().numpy().view(np.uint32)))
        del d, verts, tris
        torch.cuda.empty_cache()
        return {"leg": name, "dims": list(dims), "dtype": str(host.dtype), "ms_median": med, "ms_min": float(np.min(ms)),
                "n_verts": nv.value, "n_tris": nt.value,
                # the field is read twice (count, emit) plus the output; floor = one read of the field
                "bytes_moved_model": 2 * field + out, "bytes_one_read_floor": field,
                "floor_over_measured": field / (med * 1e-3) / HBM_PEAK, "moved_rate_TBps": (2 * field + out) / (med * 1e-3) / 1e12,
                "ms_numpy_vertices_cpu": ms_numpy, "vertices_match_numpy": same, "samples_ms": ms}

    out = {}
    n = args.gyroid
    out["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1))

    # the NS workload's raw field (threshold 0.5), as tools/components_bench.py
    X, IEN, rho_n = synthetic.hex_mesh(args.mesh)
    grid = pkg.Grid(X.min(0), X.max(0), synthetic.grid_n_max_for_points(args.grid), 3)
    rho_e = np.ascontiguousarray(rho_n[IEN - 1].mean(axis=1))
    mesh = pkg.Mesh(X, IEN)
    o = L.R2SOptions()
    L.lib().r2s_default_options(ctypes.byref(o))
    o.threshold_density = 0.5
    o.skip_rbf = 1
    raw = np.empty(grid.ngp)
    L.check(L.lib().r2s_rho2sdf(mesh.X.ctypes.data_as(L.c_double_p), mesh.nnp, mesh.IEN.ctypes.data_as(L.c_int64_p), mesh.nel,
                                rho_e.ctypes.data_as(L.c_double_p), ctypes.byref(o), ctypes.byref(grid.c), None,
                                raw.ctypes.data_as(L.c_double_p), None, None, None))
    out["ns_raw"] = leg("ns_raw", raw, grid.dims, tuple(grid.AABB_min), grid.cell_size)
    del raw

    opts = pkg.Rho2sdfOptions(threshold_density=0.5)
    for s in (False, True):
        pkg.rho2sdf("bench", X, IEN, rho_e, options=opts, sdf_grid=grid, surface=s)
    tot_off, tot_on, nt_in_call = [], [], 0
    for _ in range(max(3, args.reps // 2)):
        for s, acc in ((False, tot_off), (True, tot_on)):
            info = {}
            pkg.rho2sdf("bench", X, IEN, rho_e, options=opts, sdf_grid=grid, info=info, surface=s)
            acc.append(info["ms_total"])
            if s:
                nt_in_call = len(info["surface"][1])
    med = lambda v: float(np.median(v))  # noqa: E731
    out["rho2sdf"] = {"ms_total_surface_off": med(tot_off), "ms_total_surface_on": med(tot_on),
                      "ms_added": med(tot_on) - med(tot_off), "n_tris": nt_in_call, "samples_off": tot_off, "samples_on": tot_on}
    out["workload"] = f"NS: synthetic jittered HEX8 {args.mesh}^3, grid {grid.dims}; gyroid {n}^3 period {args.period}"
    print(json.dumps(out))
    L.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
