#!/usr/bin/env python3
"""Cost of the mesh orient (r2s_mesh_orient_dev), device-resident, HIP events, median of --reps calls after one warm-up, tables
written, beside the mesh shells (r2s_mesh_shells_dev) on the same mesh in the same run: both sort the half-edges once and the
triangles once, the orient works on a union-find of twice the nodes and passes over the edge runs three times.

Inputs: the surface of the 253^3 sphere field and of the 513^3 Float32 gyroid (54.6 M triangles), with a seeded random 30 % of
the triangles pre-flipped (corners 1 and 2 swapped).  Both rules are timed; the flipped count of the majority rule must equal the
number of pre-flipped triangles.  No time is fixed in advance: the yardstick is the shells' time, the ratio is reported.

Writes profiles/mesh_orient_bench.json and prints it.  Usage: python tools/mesh_orient_bench.py [--reps 5] [--gyroid 513]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_orient_bench.json"))
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
        gen = torch.Generator(device="cpu").manual_seed(30)
        pick = (torch.rand(len(T), generator=gen) < 0.3).to(T.device)
        S = torch.where(pick[:, None], T[:, [0, 2, 1]], T).contiguous()      # the pre-flipped mesh
        n_pre = int(pick.sum())
        del pick
        out = torch.empty_like(S)
        flip = torch.empty(len(S), dtype=torch.int32, device=S.device)
        pot = torch.empty(len(S), dtype=torch.int32, device=S.device)
        first = pkg.mesh_orient_dev(V, S)
        cap = max(first.n_patches, 1)
        counts = torch.empty((cap, 8), dtype=torch.int64, device=S.device)
        vol = torch.empty(cap, dtype=torch.float64, device=S.device)
        npt, ref, tot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def orient(flags):
            def run():
                L.check(L.lib().r2s_mesh_orient_dev(vp(V.data_ptr()), len(V), vp(S.data_ptr()), len(S), flags, vp(out.data_ptr()),
                                                    vp(flip.data_ptr()), vp(pot.data_ptr()), vp(counts.data_ptr()), vp(vol.data_ptr()),
                                                    cap, ctypes.byref(npt), ref, tot, sp))
            return run
        row = {"leg": name, "dims": [n, n, n], "verts": len(V), "tris": len(S), "pre_flipped": n_pre}
        row["mesh_orient_dev_majority"] = stats(orient(0))
        row["totals_majority"] = list(tot)
        row["restored_majority"] = bool(torch.equal(out, T))
        row["mesh_orient_dev_outward"] = stats(orient(1))
        row["totals_outward"] = list(tot)
        row["volumes_outward"] = vol[:min(npt.value, 4)].cpu().tolist()
        del first
        shells0 = pkg.mesh_shells_dev(V, out)
        scap = max(shells0.n_shells, 1)
        sot = torch.empty(len(S), dtype=torch.int32, device=S.device)
        scounts = torch.empty((scap, 8), dtype=torch.int64, device=S.device)
        sums = torch.empty((scap, 11), dtype=torch.float64, device=S.device)
        ns, sref, stot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()

        def shells():
            L.check(L.lib().r2s_mesh_shells_dev(vp(V.data_ptr()), len(V), vp(S.data_ptr()), len(S), vp(sot.data_ptr()),
                                                vp(scounts.data_ptr()), vp(sums.data_ptr()), scap, ctypes.byref(ns), sref, stot, sp))
        row["mesh_shells_dev"] = stats(shells)
        row["shells_totals_input"] = list(stot)
        row["shells_flipped_edges_output"] = int(shells0.totals[5])
        for rule in ("majority", "outward"):
            row[f"ratio_to_shells_{rule}"] = row[f"mesh_orient_dev_{rule}"]["ms_median"] / row["mesh_shells_dev"]["ms_median"]
        print(name, row, file=sys.stderr, flush=True)
        return row

    res = {}
    n = args.sphere
    res["sphere"] = leg("sphere", mesh_query_cases.sphere_field(n, 0.4 * (n - 1), np.float32), n, 2.0 / (n - 1))
    pkg._lib.lib().r2s_release_cache()
    n = args.gyroid
    res["gyroid"] = leg("gyroid", iso_ref.gyroid(n, args.period).ravel(), n, 2.0 / (n - 1))
    res["method"] = (f"HIP events on the call's stream, median of {args.reps} after one warm-up call; a seeded random 30 % of the "
                     "triangles pre-flipped; triangles, flips, patch labels and tables written; shells on the same pre-flipped mesh, "
                     "tables written")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    pkg._lib.lib().r2s_release_cache()


if __name__ == "__main__":
    main()
