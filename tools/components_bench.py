#!/usr/bin/env python3
"""Cost of the component table at 512^3 on the NS workload (bench.py), timed with HIP events on the call's stream:

* r2s_analyze_components_dev (labelling + table) against r2s_remove_artifacts_dev at ratio 0 (the same labelling, the
  largest-component kernel and a flip pass that flips nothing) on the raw field;
* ms_artifacts of r2s_rho2sdf with analyze_components on against off (bench.py's rho2sdf leg; alternated).

Prints one JSON line.  Usage: python tools/components_bench.py [--reps 10] [--grid 512]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--mesh", type=int, default=46)
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    from rho2sdf_jl_amd import synthetic
    L = pkg._lib
    X, IEN, rho_n = synthetic.hex_mesh(args.mesh)
    grid = pkg.Grid(X.min(0), X.max(0), synthetic.grid_n_max_for_points(args.grid), 3)
    rho_e = np.ascontiguousarray(rho_n[IEN - 1].mean(axis=1))
    mesh = pkg.Mesh(X, IEN)

    # the raw field of the rho2sdf leg (threshold 0.5), kept on the device
    o = L.R2SOptions()
    L.lib().r2s_default_options(ctypes.byref(o))
    o.threshold_density = 0.5
    o.skip_rbf = 1
    raw = np.empty(grid.ngp)
    L.check(L.lib().r2s_rho2sdf(mesh.X.ctypes.data_as(L.c_double_p), mesh.nnp, mesh.IEN.ctypes.data_as(L.c_int64_p), mesh.nel,
                                rho_e.ctypes.data_as(L.c_double_p), ctypes.byref(o), ctypes.byref(grid.c), None,
                                raw.ctypes.data_as(L.c_double_p), None, None, None))
    d_raw = torch.from_numpy(raw).to("cuda:0")
    d_work = torch.empty_like(d_raw)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    n = ctypes.c_int64()
    flipped = ctypes.c_int64()

    def analyze():
        L.check(L.lib().r2s_analyze_components_dev(ctypes.c_void_p(d_raw.data_ptr()), ctypes.byref(grid.c), 0.0, sp, None, None,
                                                   0, ctypes.byref(n)))

    def remove():
        L.check(L.lib().r2s_remove_artifacts_dev(ctypes.c_void_p(d_work.data_ptr()), ctypes.byref(grid.c), 0.0, 0.0, sp,
                                                 ctypes.byref(flipped)))

    def timed(fn, before=None):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    copy = lambda: d_work.copy_(d_raw)   # noqa: E731  (outside the timed window)
    analyze(); timed(remove, copy)       # warm-up: work buffers, code objects
    t_an, t_rm = [], []
    for _ in range(args.reps):
        t_an.append(timed(analyze))
        t_rm.append(timed(remove, copy))

    opts_off = pkg.Rho2sdfOptions(threshold_density=0.5)
    opts_on = pkg.Rho2sdfOptions(threshold_density=0.5, export_analysis=True)
    for op in (opts_off, opts_on):
        pkg.rho2sdf("bench", X, IEN, rho_e, options=op, sdf_grid=grid)
    art_off, art_on = [], []
    for _ in range(max(3, args.reps // 2)):
        for op, out in ((opts_off, art_off), (opts_on, art_on)):
            info = {}
            pkg.rho2sdf("bench", X, IEN, rho_e, options=op, sdf_grid=grid, info=info)
            out.append(info["ms_artifacts"])
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps({
        "workload": f"NS: synthetic jittered HEX8 {args.mesh}^3, grid {grid.dims}", "components": n.value,
        "ms_analyze_dev": med(t_an), "ms_remove_dev_ratio0": med(t_rm),
        "ms_artifacts_flag_off": med(art_off), "ms_artifacts_flag_on": med(art_on),
        "ms_artifacts_added": med(art_on) - med(art_off),
        "samples": {"analyze": t_an, "remove": t_rm, "artifacts_off": art_off, "artifacts_on": art_on}}))
    L.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
