#!/usr/bin/env python3
"""Cost of the mesh nesting (r2s_mesh_nesting_dev), device-resident, HIP events, median of --reps calls after one warm-up, records
and pair list written, with R2S_NESTING_REWIND, beside the mesh shells (r2s_mesh_shells_dev) and the index build
(r2s_mesh_index_build_dev) of the same mesh in the same run.  The nesting is timed twice: with index = NULL (it builds and drops
a tree) and against the built index.

Inputs: the surface of the 257^3 noise field of tools/mesh_shells_bench.py (about 1.47 M shells: one lane per patch, the
many-queries extreme) and of a 253^3 hollow sphere (two patches: two lanes, the cost of everything around the traversal).  No
time is fixed in advance: what is measured is recorded.

Writes profiles/mesh_nesting_bench.json and prints it.  Usage: python tools/mesh_nesting_bench.py [--reps 5] [--noise 257]"""
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


def hollow_field(n):
    """a ball of radius 0.4 (n - 1) with a concentric hollow of half that radius, lattice units"""
    g = np.arange(n, dtype=np.float32) - np.float32((n - 1) / 2)
    d = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    r = np.float32(0.4 * (n - 1))
    return np.minimum(r - d, d - np.float32(0.5) * r).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--noise", type=int, default=257)
    ap.add_argument("--sphere", type=int, default=253)
    ap.add_argument("--ray", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_nesting_bench.json"))
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
        first = pkg.mesh_nesting_dev(V, T, ray=args.ray)
        cap, pcap = max(first.n_patches, 1), max(len(first.pairs), 1)
        crossings = int(first.counts[:, 6].sum())
        del first
        out = torch.empty_like(T)
        pot = torch.empty(len(T), dtype=torch.int32, device=T.device)
        counts = torch.empty((cap, 8), dtype=torch.int64, device=T.device)
        pairs = torch.empty(pcap, dtype=torch.int64, device=T.device)
        npt, npr, tot = ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_int64 * 8)()

        def nesting(handle):
            def run():
                L.check(L.lib().r2s_mesh_nesting_dev(handle, vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), args.ray, L.NESTING_REWIND,
                                                     vp(out.data_ptr()), vp(pot.data_ptr()), vp(counts.data_ptr()), cap, vp(pairs.data_ptr()),
                                                     pcap, ctypes.byref(npt), ctypes.byref(npr), tot, sp))
            return run
        row = {"leg": name, "dims": [n, n, n], "verts": len(V), "tris": len(T), "ray": args.ray, "crossings": crossings}
        row["mesh_nesting_dev"] = stats(nesting(None))
        row["totals"] = list(tot)
        row["pairs"] = npr.value
        keep = (out.clone(), counts.clone(), pairs.clone())

        handles = []

        def build():
            while handles:
                L.lib().r2s_mesh_index_destroy(handles.pop())
            h = ctypes.c_void_p()
            L.check(L.lib().r2s_mesh_index_build_dev(vp(V.data_ptr()), len(V), vp(T.data_ptr()), len(T), sp, ctypes.byref(h)))
            handles.append(h)
        row["mesh_index_build_dev"] = stats(build)
        row["mesh_nesting_dev_with_index"] = stats(nesting(handles[-1]))
        row["equal_with_index"] = bool(torch.equal(out, keep[0]) and torch.equal(counts, keep[1]) and torch.equal(pairs, keep[2]))
        for h in handles:
            L.lib().r2s_mesh_index_destroy(h)
        del keep
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
        row["shells"] = ns.value
        row["ratio_to_shells"] = row["mesh_nesting_dev"]["ms_median"] / row["mesh_shells_dev"]["ms_median"]
        row["ratio_to_index_build"] = row["mesh_nesting_dev"]["ms_median"] / row["mesh_index_build_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.noise
    f = (np.random.default_rng(7).normal(size=(n, n, n)) - 0.9).astype(np.float32)
    res["noise"] = leg("noise", f.ravel(), n, 2.0 / (n - 1))
    del f
    pkg._lib.lib().r2s_release_cache()
    n = args.sphere
    res["hollow_sphere"] = leg("hollow_sphere", hollow_field(n).ravel(), n, 2.0 / (n - 1))
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; R2S_NESTING_REWIND, triangles, patch "
                     "labels, records and the pair list written; with index = NULL (a tree is built and dropped) and against a built "
                     "index; shells (tables written) and the index build on the same mesh in the same run")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
