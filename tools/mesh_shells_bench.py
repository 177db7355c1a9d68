#!/usr/bin/env python3
"""Cost of the mesh shells (r2s_mesh_shells_dev), device-resident, HIP events, median of --reps calls after one warm-up, beside
the mesh-index build (r2s_mesh_index_build_dev) on the same mesh in the same run: both are dominated by radix sorts.

Meshes: the surface of the 253^3 sphere field (one shell), of the 513^3 Float32 gyroid (one shell of 54.6 M triangles: the
long-chain extreme) and of a 257^3 noise field (about 10^6 small shells: the many-segments extreme).

Kernel times by name come from a separate run under the profiler (trace only, no counters):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mesh_shells_bench.py --reps 1
Writes profiles/mesh_shells_bench.json and prints it.  Usage: python tools/mesh_shells_bench.py [--reps 5] [--gyroid 513]"""
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
    ap.add_argument("--noise", type=int, default=257)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_shells_bench.json"))
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
        first = pkg.mesh_shells_dev(V, T)
        cap = first.n_shells
        sot = torch.empty(nt.value, dtype=torch.int32, device=V.device)
        counts = torch.empty((max(cap, 1), 8), dtype=torch.int64, device=V.device)
        sums = torch.empty((max(cap, 1), 11), dtype=torch.float64, device=V.device)
        ns, ref, tot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def shells():
            L.check(L.lib().r2s_mesh_shells_dev(vp(V.data_ptr()), nv.value, vp(T.data_ptr()), nt.value, vp(sot.data_ptr()),
                                                vp(counts.data_ptr()), vp(sums.data_ptr()), cap, ctypes.byref(ns), ref, tot, sp))
        row = {"leg": name, "dims": [n, n, n], "n_verts": nv.value, "n_tris": nt.value, "totals": first.totals.tolist(),
               "closed_shells": int(first.closed.sum()), "voids": int(first.is_void.sum()),
               "largest_shell_tris": int(first.n_tris.max()) if cap else 0, "volume": float(first.volume.sum())}
        row["mesh_shells_dev"] = stats(shells)
        row["mesh_index_build_dev"] = stats(lambda: pkg.MeshIndex(V, T).close())
        row["ratio_to_build"] = row["mesh_shells_dev"]["ms_median"] / row["mesh_index_build_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    res["sphere"] = leg("sphere", mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    n = args.noise
    f = (np.random.default_rng(7).normal(size=(n, n, n)) - 0.9).astype(np.float32)
    res["noise"] = leg("noise", f.ravel(), n, 2.0 / (n - 1))
    res["method"] = f"HIP events on the call's stream, median of {args.reps} after one warm-up call; tables written (capacity = n_shells)"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
