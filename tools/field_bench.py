#!/usr/bin/env python
"""Timings of the point evaluator (r2s_rbf_field), device-resident, medians of repeated launches after a warm-up; writes
profiles/field_bench.json.

At the NS workload's coarse lattice (513^3 nodes, kernel threshold 1e-3, a gyroid as weights through
r2s_rbf_field_from_weights - the evaluator's cost does not depend on their values):
  a   the 513^3 lattice points (the field's own Float32 axes) in lattice order, value only; its yardstick is the library's
      neighbour-by-neighbour lattice evaluation rbf_apply_kernel (R2S_RBF_APPLY=fly) on the same lattice: `--cases fly`
      runs it (approximation mode, smooth = 1: its two evaluations are 513^3 targets over the 513^3 lattice each)
  c   10^7 uniformly random points, value; cg: the same with the gradient; ch: with gradient and Hessian, timed beside the
      gradient mode in the same run (ratio recorded)
On a fitted field (sphere fixture, N_max 160, fit + smooth = 2 + extract_isosurface):
  b   value + gradient at the surface's vertices;  d: their projection (8 steps at most, tol 1e-4 cell)
  bk  curvature at the surface's vertices, timed beside the gradient mode in the same run (ratio recorded)

Kernel times: run one case under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/field_bench.py --cases X --no-json` (a run of its own per case: tracing slows the host, and a and c share a kernel
name), then `--merge X=DIR ...` adds the per-launch kernel times of those traces to the JSON.

    python tools/field_bench.py [--cases a,c,cg,ch,b,d,bk] [--update] [--reps 7] [--merge a=DIR fly=DIR ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def _median_ms(fn, reps, torch):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def _kernel_rows(d):
    """rows of every *kernel_stats.csv under d whose kernel is the evaluator's or the lattice evaluation's"""
    import csv
    import glob
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if "rbf_field_kernel" in r["Name"] or "rbf_apply_kernel" in r["Name"]:
                    name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
                    rows.append({"kernel": name.split("(")[0], "calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) * 1e-6,
                                 "min_ms": float(r["MinNs"]) * 1e-6, "max_ms": float(r["MaxNs"]) * 1e-6})
    return rows


def _coarse_axis(lo, hi, n):
    a, b = float(np.float32(lo)), float(np.float32(hi))
    x = (a + np.arange(n, dtype=np.float64) * (b - a) / (n - 1)).astype(np.float32)
    x[-1] = np.float32(hi)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="a,c,cg,ch,b,d,bk")
    ap.add_argument("--no-json", action="store_true", help="do not write the result file (runs under the profiler)")
    ap.add_argument("--merge", nargs="*", default=None, metavar="CASE=DIR", help="add the kernel times of rocprofv3 output directories")
    ap.add_argument("--update", action="store_true", help="add this run's cases and ratios to the existing result file instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_bench.json"))
    a = ap.parse_args()
    if a.merge is not None:
        with open(a.out) as fh:
            res = json.load(fh)
        res["kernel_trace"] = {k: _kernel_rows(d) for k, d in (m.split("=", 1) for m in a.merge)}
        kt = res["kernel_trace"]
        # (the traces of a and c also hold the small launch that counts the taps: a full launch is the row's max_ms)
        if kt.get("a") and kt.get("fly"):
            res["lattice_order_over_fly_kernel_time"] = max(r["max_ms"] for r in kt["a"]) / kt["fly"][0]["avg_ms"]
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res))
        return
    cases = set(a.cases.split(","))
    pkg = graft.load_built()
    import torch
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    n = a.n
    grid = pkg.Grid([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], n, 0)
    nx, ny, nz = grid.dims
    ax = [np.arange(d, dtype=np.float32) * np.float32(2 * np.pi * 3 / n) for d in (nx, ny, nz)]
    res = {"lattice": [nx, ny, nz], "threshold": 1e-3, "reps": a.reps, "cases": {}}

    def record(name, npts, taps_per_point, ms, **extra):
        med, lo, hi = ms
        res["cases"][name] = dict(points=int(npts), ms_median=med, ms_min=lo, ms_max=hi, points_per_s=npts / (med * 1e-3),
                                  taps_per_s=npts * taps_per_point / (med * 1e-3), **extra)
        print(name, json.dumps(res["cases"][name]), flush=True)

    if cases & {"a", "c", "cg", "ch", "fly"}:
        w = (np.sin(ax[0])[None, None, :] * np.cos(ax[1])[None, :, None] + np.sin(ax[1])[None, :, None] * np.cos(ax[2])[:, None, None]
             + np.sin(ax[2])[:, None, None] * np.cos(ax[0])[None, None, :]).astype(np.float32) * np.float32(0.18)
    if "fly" in cases:
        os.environ["R2S_RBF_APPLY"] = "fly"
        for _ in range(3):
            pkg.RBFs_smoothing(w.astype(np.float64).ravel(), grid, False, 1, 0.5, 1e-3, device=0)
        del os.environ["R2S_RBF_APPLY"]
    if cases & {"a", "c", "cg", "ch"}:
        with pkg.RbfField(w, grid, 0.0, 1e-3, device=0) as f:
            amin, amax = grid.AABB_min, grid.AABB_max
            cx, cy, cz = [torch.tensor(_coarse_axis(amin[k], amax[k], d), device=dev) for k, d in enumerate((nx, ny, nz))]
            taps = None
            if "a" in cases:
                Z, Y, X = torch.meshgrid(cz, cy, cx, indexing="ij")
                lat = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], dim=1).contiguous()
                del X, Y, Z
                taps = f.eval_dev(lat[:: max(1, lat.shape[0] // 100000)].contiguous(), taps=True)[1].abs().float().mean().item()
                record("a_lattice_value", lat.shape[0], taps, _median_ms(lambda: f.eval_dev(lat), a.reps, torch))
                del lat
            if cases & {"c", "cg", "ch"}:
                torch.manual_seed(1)
                rnd = torch.rand((10_000_000, 3), device=dev, dtype=torch.float32)
                taps = f.eval_dev(rnd[:100000].contiguous(), taps=True)[1].abs().float().mean().item()
                if "c" in cases:
                    record("c_random_value", rnd.shape[0], taps, _median_ms(lambda: f.eval_dev(rnd), a.reps, torch))
                if "cg" in cases:
                    record("c_random_value_grad", rnd.shape[0], taps, _median_ms(lambda: f.eval_dev(rnd, grad=True), a.reps, torch))
                if "ch" in cases:
                    grad_ms = _median_ms(lambda: f.eval_dev(rnd, grad=True), a.reps, torch)
                    record("c_random_hessian", rnd.shape[0], taps, _median_ms(lambda: f.hessian_dev(rnd), a.reps, torch),
                           grad_ms_same_run=grad_ms[0])
                    res["ratio_hessian_to_grad_random"] = res["cases"]["c_random_hessian"]["ms_median"] / grad_ms[0]
                del rnd
    if cases & {"b", "d", "bk"}:
        d = np.load(os.path.join(ROOT, "tests", "golden", "sphere.npz"))
        X, IEN, rho = d["X"], d["IEN"].astype(np.int64), d["rho"]
        mesh = pkg.Mesh(X, IEN)
        sg = pkg.Grid(X.min(0), X.max(0), 160, 3)
        sdf = pkg.sdf_fused(mesh, sg, pkg.DenseInNodes(mesh, rho, device=0), 0.5, device=0)
        vd, vf = pkg.calculate_mesh_volume(mesh, rho, device=0)
        fine = pkg.RBFs_smoothing(sdf, sg, True, 2, vd * vf, 1e-3, device=0)
        verts = torch.tensor(pkg.extract_isosurface(fine, sg, 2, device=0)[0], device=dev)
        with pkg.fit_rbf_field(sdf, sg, True, vd * vf, 1e-3, device=0) as f:
            taps = f.eval_dev(verts, taps=True)[1].abs().float().mean().item()
            extra = {"lattice": list(sg.dims)}
            if "b" in cases:
                record("b_surface_value_grad", verts.shape[0], taps, _median_ms(lambda: f.eval_dev(verts, grad=True), a.reps, torch), **extra)
            if "d" in cases:
                _, status, _, iters = f.project_dev(verts, 8)
                torch.cuda.synchronize()
                extra.update(status0_share=float((status == 0).float().mean().item()), mean_steps=float(iters.float().mean().item()))
                record("d_surface_project", verts.shape[0], taps * (1.0 + extra["mean_steps"]),
                       _median_ms(lambda: f.project_dev(verts, 8), a.reps, torch), **extra)
            if "bk" in cases:
                grad_ms = _median_ms(lambda: f.eval_dev(verts, grad=True), a.reps, torch)
                record("b_surface_curvature", verts.shape[0], taps, _median_ms(lambda: f.curvature_dev(verts), a.reps, torch),
                       grad_ms_same_run=grad_ms[0], **{"lattice": list(sg.dims)})
                res["ratio_curvature_to_grad_surface"] = res["cases"]["b_surface_curvature"]["ms_median"] / grad_ms[0]
    c = res["cases"]
    if "a_lattice_value" in c and "c_random_value" in c:
        res["ratio_random_to_lattice_per_point"] = (c["c_random_value"]["ms_median"] / c["c_random_value"]["points"]) / (
            c["a_lattice_value"]["ms_median"] / c["a_lattice_value"]["points"])
    if a.update and os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
        old["cases"].update(res["cases"])
        old.update({k: v for k, v in res.items() if k.startswith("ratio_")})
        res = old
    if not a.no_json:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
