#!/usr/bin/env python3
"""Cost of the winding number and the signed distance (r2s_mesh_index_winding_dev / _winding_lattice_dev / _signed_lattice_dev),
device-resident, HIP events, median of --reps calls after one warm-up, beside the distance query of the same points in the same
run (r2s_mesh_index_query_dev / _lattice_dev).

Meshes: the surface of the 253^3 sphere field and of the 513^3 Float32 gyroid (open at the lattice border: crossings and times
only, no inside claim).  Per mesh: --points random points through `winding` and through `distance`; the whole lattice through the
row kernels, through the per-point kernel on the same lattice points (4x4x4 blocks, R2S_WINDING_ROWS=0; and as an explicit array
through `winding`), and through `lattice` (the distance); `signed_lattice` as a whole, both ways.  No time is fixed in advance.

Writes profiles/mesh_winding_bench.json (after every leg) and prints it.  Usage: python tools/mesh_winding_bench.py [--reps 5]"""
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
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--ray", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding_bench.json"))
    args = ap.parse_args()
    pkg = graft.load_built()
    import torch
    L = pkg._lib
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    vp = ctypes.c_void_p
    res = {}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

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

    def leg(name, V, T, n, closed):
        h = 2.0 / (n - 1)
        lat = ((n, n, n), (-1.0, -1.0, -1.0), h)
        row = {"leg": name, "dims": [n, n, n], "verts": len(V), "tris": len(T), "ray": args.ray, "closed": closed}
        res[name] = row
        with pkg.MeshIndex(V, T) as ix:
            row["tree_depth"] = ix.info()["depth"]
            g = torch.Generator(device="cuda").manual_seed(1)
            P = (torch.rand((args.points, 3), generator=g, device="cuda", dtype=torch.float64) * 2.0 - 1.0).contiguous()
            row["points"] = args.points
            row["winding_dev"] = stats(lambda: ix.winding_dev(P, args.ray, want_crossings=True))
            row["distance_dev"] = stats(lambda: ix.distance_dev(P))
            w, c = ix.winding_dev(P, args.ray, want_crossings=True)
            row["points_mean_crossings"] = float(c.double().mean())
            if closed:
                row["points_inside_fraction"] = float((w > 0).double().mean())
            del P, w, c
            save()
            os.environ.pop("R2S_WINDING_ROWS", None)                  # the row kernels (the default)
            row["winding_lattice_dev_rows"] = stats(lambda: ix.winding_lattice_dev(lat, ray=args.ray, want_crossings=True))
            row["signed_lattice_dev_rows"] = stats(lambda: ix.signed_lattice_dev(lat, ray=args.ray))
            lw, lc = ix.winding_lattice_dev(lat, ray=args.ray, want_crossings=True)
            sr = ix.signed_lattice_dev(lat, ray=args.ray)
            os.environ["R2S_WINDING_ROWS"] = "0"                      # the per-point kernel on 4x4x4 blocks
            row["winding_lattice_dev_points"] = stats(lambda: ix.winding_lattice_dev(lat, ray=args.ray, want_crossings=True))
            row["signed_lattice_dev_points"] = stats(lambda: ix.signed_lattice_dev(lat, ray=args.ray))
            bw, bc = ix.winding_lattice_dev(lat, ray=args.ray, want_crossings=True)
            sb = ix.signed_lattice_dev(lat, ray=args.ray)
            os.environ.pop("R2S_WINDING_ROWS")
            row["rows_equal_blocks"] = bool(torch.equal(lw, bw) and torch.equal(lc, bc) and torch.equal(sr, sb))
            del bw, bc, sr, sb
            row["lattice_dev"] = stats(lambda: ix.lattice_dev(lat))
            row["rows_over_points"] = row["winding_lattice_dev_rows"]["ms_median"] / row["winding_lattice_dev_points"]["ms_median"]
            save()
            ax = -1.0 + h * torch.arange(n, device="cuda", dtype=torch.float64)
            Q = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij")[::-1], dim=-1).reshape(-1, 3).contiguous()   # x fastest
            row["winding_dev_on_lattice_points"] = stats(lambda: ix.winding_dev(Q, args.ray, want_crossings=True))
            pw, pc = ix.winding_dev(Q, args.ray, want_crossings=True)
            row["lattice_equals_points"] = bool(torch.equal(lw.ravel(), pw) and torch.equal(lc.ravel(), pc))
            row["lattice_mean_crossings"] = float(lc.double().mean())
            if closed:
                row["lattice_inside_fraction"] = float((lw > 0).double().mean())
            row["winding_lattice_over_lattice"] = row["winding_lattice_dev_rows"]["ms_median"] / row["lattice_dev"]["ms_median"]
            row["winding_over_distance_points"] = row["winding_dev"]["ms_median"] / row["distance_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        save()

    n = args.sphere
    V, T = extract(mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    leg("sphere", V, T, n, True)
    del V, T
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    V, T = extract(iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    leg("gyroid", V, T, n, False)
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; outputs allocated inside the timed "
                     "call (torch caching allocator); winding and crossings both written; points: uniform in the lattice's box, "
                     "float64; 'rows': the row kernels (one traversal per row, bisection, prefix sum), the default; 'points': R2S_WINDING_ROWS=0, the "
                     "per-point kernel on 4x4x4 blocks of the same lattice")
    save()
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
