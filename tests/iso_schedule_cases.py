"""Cases, knob sets and the child process of tests/test_iso_schedule_gpu.py: the persistent HEX8 projection kernels
(iso_project_hex_pl_kernel, iso_straggler_kernel, iso_sweep_kernel) under forced schedules.

The launch rule of iso_project_hex() gives almost every wavefront one group of one chunk at test sizes, so the
multi-fetch loop, groups that span items, slot reuse and the straggler kernel's refill run in the other parity tests by
accident of timing or not at all.  The environment switches below (read once per process: one child process per set) bring the
machine down to a few wavefronts on grids the oracle finishes in seconds.  Every answer depends on its own (voxel,
element) pair only, so every set must give the oracle's field bit for bit and the baseline's projection points and
hand-over counts exactly.

Run as a script this file is the child: it loads the built library, runs every call of the named cases against the
oracle results in an .npz written by the parent, and writes its counters and projection points for the parent.
"""
import json
import os
import sys
import time

import numpy as np

RHO_T = 0.5
BF = 1.1

# environment of every knob set (the baseline set is empty); cases: which ones the child of a set runs
HEX_CASES = ("one_item", "distorted", "tiny_items", "slab")
KNOB_SETS = {
    "baseline": ({}, HEX_CASES + ("tet",)),
    "one_wave": ({"R2S_ISO_RESIDENT": "1"}, HEX_CASES),                       # one wavefront walks every chunk; default group rule
    "few_odd": ({"R2S_ISO_RESIDENT": "3", "R2S_ISO_GROUP": "5"}, HEX_CASES),  # group no power of two, partial last group
    "few_single": ({"R2S_ISO_RESIDENT": "2", "R2S_ISO_GROUP": "1"}, HEX_CASES),   # one fetch per chunk
    "one_fetch": ({"R2S_ISO_RESIDENT": "7", "R2S_ISO_GROUP": "1000000"}, HEX_CASES),   # the first fetch takes everything
    "strag_one": ({"R2S_STRAG_WAVES": "1"}, HEX_CASES),                       # quota 64, dozens of refills per lane
    "strag_two_overflow": ({"R2S_ISO_RESIDENT": "2", "R2S_STRAG_WAVES": "2", "R2S_ISO_STRAGGLER_CAP": "64"}, HEX_CASES),
    "wps1": ({"R2S_ISO_WPS": "1"}, HEX_CASES),
    "wps2": ({"R2S_ISO_WPS": "2"}, HEX_CASES),
    "wps3": ({"R2S_ISO_WPS": "3"}, HEX_CASES),
    "no_early_iso": ({"R2S_NO_EARLY_ISO": "1"}, HEX_CASES),                   # the non-early launch sites
    "no_overlap": ({"R2S_NO_OVERLAP": "1"}, HEX_CASES),
    "tet_cpw1": ({"R2S_ISO_CPW": "1"}, ("tet",)),                             # chunks-per-wave loop of iso_project_kernel
    "tet_cpw3": ({"R2S_ISO_CPW": "3"}, ("tet",)),
    "tet_cpw1000000": ({"R2S_ISO_CPW": "1000000"}, ("tet",)),
}
# switches a child must not inherit from the caller's environment
SCHEDULE_VARS = ("R2S_ISO_RESIDENT", "R2S_ISO_GROUP", "R2S_ISO_WPS", "R2S_ISO_FREE", "R2S_ISO_CPW", "R2S_ISO_STRAGGLER_CAP",
                 "R2S_STRAG_WAVES", "R2S_STRAG_WPC", "R2S_NO_EARLY_ISO", "R2S_NO_OVERLAP", "R2S_NO_SPECULATION")
SLAB_RUNS = {"planes": dict(k_begin=4, k_end=13), "layers": dict(zstride=2, zphase=1)}


def build_case(name):
    """-> (X, IEN, rho_n, N_max of the grid).  `slab` is the distorted mesh (its oracle field is shared)."""
    from rho2sdf_jl_amd import synthetic
    if name == "one_item":
        from test_oracle_drift import one_hex
        X, IEN, rn = one_hex()
        return X, IEN, rn, 20
    if name in ("distorted", "slab"):
        X, IEN, _ = synthetic.hex_mesh(7, jitter=.30, seed=20240502)
        rn = np.clip(np.random.default_rng(1).normal(0.5, 0.35, len(X)), 0, 1)
        return X, IEN, rn, synthetic.grid_n_max_for_points(48)
    if name == "tiny_items":
        X, IEN, rn = synthetic.hex_mesh(20)
        return X, IEN, rn, synthetic.grid_n_max_for_points(24)
    if name == "tet":
        X, IT, rn = synthetic.tet_mesh(6)
        return X, IT, rn, synthetic.grid_n_max_for_points(48)
    raise KeyError(name)


def oracle_case(name):
    """the case whose oracle field `name` is compared against"""
    return "distorted" if name == "slab" else name


def item_chunks(X, IEN, g, bf=BF):
    """64-voxel chunks of the lattice box of every element as item_build_kernel sizes it, from box arithmetic alone:
    the mini-AABB cell range of the element's bounding box widened by bf cells (Grid.jl:130-145), as lattice indices
    trimmed to the points whose cell lies in the range.  `g`: a grid with amin, amax, N, cell."""
    lo_x = X[IEN - 1].min(1)
    hi_x = X[IEN - 1].max(1)
    vol = np.ones(len(IEN), np.int64)
    delta = bf * g.cell
    for ax in range(3):
        N, amin, amax = int(g.N[ax]), g.amin[ax], g.amax[ax]
        cell = lambda x: np.floor(N * (x - amin) / (amax - amin))
        imin = np.maximum(cell(lo_x[:, ax] - delta), 0).astype(np.int64)
        imax = np.minimum(cell(hi_x[:, ax] + delta), N).astype(np.int64)
        a = imin.copy()
        b = np.minimum(imax + 1, N)
        a += cell(amin + g.cell * a) < imin
        b -= cell(amin + g.cell * b) > imax
        vol *= np.maximum(b - a + 1, 0)
    return (vol + 63) // 64, vol


def slab_planes(which, nz):
    """global Z planes of the local planes of a SLAB_RUNS entry (-1: padding behind the last plane)"""
    kw = SLAB_RUNS[which]
    if "k_begin" in kw:
        return np.arange(kw["k_begin"], kw["k_end"])
    G, r = kw["zstride"], kw["zphase"]
    layers = (nz + 3) // 4
    owned = (layers - r + G - 1) // G if layers > r else 0
    p = np.arange(4 * owned)
    k = 4 * ((p // 4) * G + r) + p % 4
    return np.where(k < nz, k, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------
def _xp_check(label, xp, oxp, sent, X):
    real = ~sent
    atol = 1e-9 * max(1.0, np.abs(X).max())        # the bar of test_parity_gpu._compare
    err = np.abs(xp[real] - oxp[real]).max() if real.any() else 0.0
    assert err <= atol, f"{label}: projection points off by {err}"
    assert not xp[sent].any(), f"{label}: projection point on a sentinel voxel"


def _same(label, got, want, exact=True, cell=1.0):
    """HEX8: equal to the oracle bit for bit on every voxel.  TET4 (exact=False): the bar of test_parity_gpu._compare -
    sentinel set and sign identical, magnitudes within 1e-6 relative (absolute against the cell size near zero)"""
    if exact:
        assert np.array_equal(got, want), f"{label}: {int((got != want).sum())} of {want.size} voxels differ from the oracle"
        return
    real = np.abs(want) < 1e9
    assert np.array_equal(np.abs(got) < 1e9, real), f"{label}: sentinel set differs"
    assert np.array_equal(np.sign(got), np.sign(want)), f"{label}: sign differs"
    err = np.abs(got[real] - want[real])
    bad = (err > 1e-6 * np.maximum(np.abs(want[real]), 1e-300)) & (err > 1e-12 * cell)
    assert not bad.any(), f"{label}: {int(bad.sum())} values beyond 1e-6"


def _keep(st):
    return {k: int(st[k]) for k in ("n_items", "n_iso_chunks", "n_iso_straggler", "n_iso_fail")}


def run_case(pkg, name, ref, out):
    """every call of one case; asserts against the oracle arrays in `ref`, returns the counters of every call"""
    import torch
    X, IEN, rn, nmax = build_case(name)
    oc = oracle_case(name)
    odist, osign, oxp = ref[oc + "_dist"], ref[oc + "_sign"], ref[oc + "_xp"]
    want = odist * osign
    sent = odist == 1e10
    pg = pkg.Grid(X.min(0), X.max(0), nmax, 3)
    nx, ny, nz = pg.dims
    dev = torch.device("cuda:0")
    dX, dI, dR = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, IEN, rn))
    stats = {}
    if name == "slab":
        plan = pkg.DevicePlan(0)
        for which, kw in SLAB_RUNS.items():
            planes = slab_planes(which, nz)
            ok = planes >= 0
            w = want.reshape(nz, ny, nx)[planes[ok]]
            for call in ("first", "repeat"):     # waiting regime, then speculated sizes (early launch)
                buf = torch.empty(len(planes) * ny * nx, dtype=torch.float64, device=dev)
                stats[f"{which}_{call}"] = _keep(plan.run(dX, dI, dR, RHO_T, pg, sdf=buf, **kw))
                _same(f"{name} {which} {call}", buf.cpu().numpy().reshape(len(planes), ny, nx)[ok], w)
        plan.close()
        return stats
    hex8 = IEN.shape[1] == 8
    cell = pg.cell_size
    # (a) fused field: first call (waiting), second call of the same plan (speculated), a fresh plan
    plan = pkg.DevicePlan(0)
    fields = []
    for call in ("first", "repeat"):
        buf = torch.empty(pg.ngp, dtype=torch.float64, device=dev)
        stats[call] = _keep(plan.run(dX, dI, dR, RHO_T, pg, sdf=buf))
        fields.append(buf.cpu().numpy())
        _same(f"{name} sdf {call}", fields[-1], want, hex8, cell)
    fresh = pkg.DevicePlan(0)
    buf = torch.empty(pg.ngp, dtype=torch.float64, device=dev)
    stats["fresh"] = _keep(fresh.run(dX, dI, dR, RHO_T, pg, sdf=buf))
    fields.append(buf.cpu().numpy())
    _same(f"{name} sdf fresh", fields[-1], want, hex8, cell)
    fresh.close()
    assert np.array_equal(fields[0], fields[1]) and np.array_equal(fields[0], fields[2]), f"{name}: the three calls differ"
    out[name + "_sdf"] = fields[0]
    # (b) distance, sign and projection points in one call (never launched early; res_xp in all three kernels)
    d, s = (torch.empty(pg.ngp, dtype=torch.float64, device=dev) for _ in range(2))
    xp = torch.empty((pg.ngp, 3), dtype=torch.float64, device=dev)
    stats["xp"] = _keep(plan.run(dX, dI, dR, RHO_T, pg, dist=d, sign=s, xp=xp))
    plan.close()
    xp = xp.cpu().numpy()
    _same(f"{name} dist", d.cpu().numpy(), odist, hex8, cell)
    _same(f"{name} sign", s.cpu().numpy(), osign)
    _xp_check(f"{name} run", xp, oxp, sent, X)
    out[name + "_xp"] = xp
    # (c) the host entry point
    st = {}
    hd, hxp = pkg.evalDistances(pkg.Mesh(X, IEN), pg, rn, RHO_T, band_factor=BF, stats=st)
    stats["host"] = _keep(st)
    _same(f"{name} evalDistances", hd, odist, hex8, cell)
    _xp_check(f"{name} evalDistances", hxp, oxp, sent, X)
    assert np.array_equal(hxp, xp), f"{name}: host and device entry points give different projection points"
    if hex8:
        n_fail, n_solves = int(ref[oc + "_n_iso_fail"]), int(ref[oc + "_n_iso_solves"])
        for call, c in stats.items():
            assert c["n_iso_fail"] == n_fail, (name, call, c, n_fail)
            assert n_fail <= c["n_iso_straggler"] <= n_solves, (name, call, c, n_fail, n_solves)
    return stats


def main(argv):
    ref_path, out_prefix, cases = argv[0], argv[1], argv[2].split(",")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as graft
    t0 = time.perf_counter()
    pkg = graft.load_built()
    ref = np.load(ref_path)
    stats, arrays, secs = {}, {}, {}
    for name in cases:
        t1 = time.perf_counter()
        stats[name] = run_case(pkg, name, ref, arrays)
        secs[name] = round(time.perf_counter() - t1, 2)
    np.savez(out_prefix + ".npz", **arrays)
    with open(out_prefix + ".json", "w") as f:
        json.dump({"stats": stats, "seconds": secs, "total_seconds": round(time.perf_counter() - t0, 2)}, f)


if __name__ == "__main__":
    main(sys.argv[1:])
