#!/usr/bin/env python3
"""Cost of redistancing (r2s_redistance_dev, the field already on the device), per band of 2, 4, 8 and 16 cells:

* the 513^3 Float32 gyroid of tools/surface_bench.py, and the Float32 fine field of a fitted sphere (rho2sdf on the sphere
  fixture, rbf_grid fine);
* whole call with HIP events on the call's stream, median of --reps after a warm-up; the phases from the library's own events
  (r2s_last_distance_stats: surface extraction, binning = count + scan + list fills, tile kernel; the +-band fill of tiles
  without triangles happens inside the tile kernel and has no time of its own);
* tile/triangle pairs, pairs per second of tile-kernel time, the one-read-one-write HBM floor of the field beside each figure,
  and an UPPER bound of the share of the 78.6 TFLOP/s FP64 peak: pairs x 512 voxels x FLOP_PER_PAIR over the tile-kernel
  time - the per-wave cull skips triangles that are counted here, so the true share is lower.

Kernel times by name come from a separate run under the profiler (no counters):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/redistance_bench.py --reps 1 --bands 4
Writes profiles/redistance_bench.json and prints it.  Usage: python tools/redistance_bench.py [--reps 10] [--gyroid 513]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import iso_ref  # noqa: E402

HBM_PEAK = 8.0e12
FP64_PEAK = 78.6e12
FLOP_PER_PAIR = 80   # one voxel against one triangle: 3 clamped segments (17 each), 2 differences (6), 3 edge functions (16), plane (7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gyroid", type=int, default=513)
    ap.add_argument("--period", type=int, default=24)
    ap.add_argument("--bands", type=float, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--sphere-grid", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redistance_bench.json"))
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    st = torch.cuda.current_stream()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def leg(name, host, dims, origin, spacing):
        import ctypes
        L = pkg._lib
        d = torch.from_numpy(host).to("cuda:0")
        out = torch.empty_like(d)
        dd, oo = (ctypes.c_int64 * 3)(*dims), (ctypes.c_double * 3)(*origin)
        sp = ctypes.c_void_p(st.cuda_stream)
        rows = []
        for cells in args.bands:
            band = cells * spacing

            def run():
                L.check(L.lib().r2s_redistance_dev(ctypes.c_void_p(d.data_ptr()), int(host.dtype == np.float32), dd, oo, spacing, 0.0,
                                                   band, ctypes.c_void_p(out.data_ptr()), sp))
            run()
            ms, phases = [], []
            for _ in range(args.reps):
                ms.append(timed(run))
                phases.append(pkg.last_distance_stats())
            med = lambda k: float(np.median([p[k] for p in phases]))  # noqa: E731
            s = phases[-1]
            tile_ms = med("ms_tile_kernel")
            floor_ms = 2 * host.nbytes / HBM_PEAK * 1e3
            rows.append({"band_cells": cells, "ms_call_median": float(np.median(ms)), "ms_call_min": float(np.min(ms)),
                         "ms_extract": med("ms_extract"), "ms_binning": med("ms_binning"), "ms_tile_kernel": tile_ms,
                         "pairs": s["pairs"], "batches": s["batches"], "n_tris": s["n_tris"], "n_tiles": s["n_tiles"],
                         "n_active_tiles": s["n_active_tiles"],
                         "pairs_per_s_of_tile_kernel": s["pairs"] / (tile_ms * 1e-3) if tile_ms > 0 else None,
                         "ms_hbm_floor_one_read_one_write": floor_ms,
                         "fp64_share_upper_bound": s["pairs"] * 512 * FLOP_PER_PAIR / (tile_ms * 1e-3) / FP64_PEAK if tile_ms > 0 else None,
                         "in_band_fraction": float((out.abs() < band).float().mean()), "samples_ms": ms})
            print(name, rows[-1], file=sys.stderr, flush=True)
        del d, out
        torch.cuda.empty_cache()
        return {"leg": name, "dims": list(dims), "dtype": str(host.dtype), "bands": rows}

    res = {}
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), (n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1))
    d = np.load(os.path.join(ROOT, "tests", "golden", "sphere.npz"))
    X, IEN, rho = d["X"], d["IEN"].astype(np.int64), d["rho"]
    grid = pkg.Grid(X.min(0), X.max(0), args.sphere_grid, 3)
    fine = pkg.rho2sdf("bench", X, IEN, rho, options=pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine"), sdf_grid=grid)[0]
    dims = fine.shape[::-1]
    res["sphere_fine"] = leg("sphere_fine", np.ascontiguousarray(fine).ravel(), dims, tuple(grid.AABB_min), grid.cell_size / 2)
    res["method"] = (f"HIP events, median of {args.reps} after one warm-up call per band; phases from the library's events; "
                     f"FLOP model {FLOP_PER_PAIR} per voxel-triangle pair, culled pairs included (upper bound)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
