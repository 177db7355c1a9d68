"""The code paths that only production-sized calls take, each against a plain reference of the same operation:

* connected components with more roots than the list of roots holds (ccl_roots_max_kernel, r2s_post.hip): at the
  boundary of R2S_CCL_ROOTS_CAP and with more than 2^22 components and no knob, against oracle.remove_artifacts;
* the early delivery of the fine field of r2s_rho2sdf (nfine >= 2^22: the field without its level shift lands chunk by
  chunk in pinned memory, host threads add the shift), against the same call with R2S_FINE_EARLY=0 and the oracle;
* the streaming stores of the sparse download of r2s_sdf (nx % 4 == 0 and a 32-byte-aligned output), against the
  device path.

Switches that are read once per process run in child processes (one at a time: the parent and one child have the
GPU open); the children write what they computed under tmp_path and the parent compares.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu
TESTS = os.path.join(ROOT, "tests")


def _bits(a):
    """the bit patterns of a float array (0.0 and -0.0 differ, NaN equals itself)"""
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _at(alloc, n, dtype, mod, rem):
    """n values of `dtype` from `alloc` (np.empty / host_array) starting at an address that is `rem` modulo `mod`"""
    dtype = np.dtype(dtype)
    raw = alloc(n * dtype.itemsize + 2 * mod, np.uint8)
    off = (rem - raw.ctypes.data) % mod
    a = raw[off:off + n * dtype.itemsize].view(dtype)
    assert a.ctypes.data % mod == rem
    return a


def _pageable(n, dtype=np.float64):
    return np.empty(n, dtype)


def _run_child(func, args, env, timeout):
    """run `func(*args)` of this module in a fresh interpreter; returns its stdout"""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_large_paths_gpu as t; t.%s(*%r)"
            % (ROOT, TESTS, func, tuple(args)))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{func}{tuple(args)} exited with {r.returncode}:\n{r.stdout}\n{r.stderr}"
    return r.stdout


# ---- A. connected components: the list of roots full, overflowing, and overflowing its allocation ------------------

def _isolated_and_block(dims, lattice, b0, b1, edge, rng):
    """-1 everywhere, +1 on the voxels of `lattice` (none of them 6-neighbours of another), one solid +1 block
    [b0, b1)^3 and a -1 moat one voxel wide around it; `edge` values replace random lattice voxels outside the moat.
    Returns the field (z, y, x) and the mask of the isolated lattice voxels."""
    nx, ny, nz = dims
    k, j, i = np.ogrid[:nz, :ny, :nx]
    iso = np.broadcast_to(lattice(i, j, k), (nz, ny, nx)).copy()
    iso[b0 - 1:b1 + 1, b0 - 1:b1 + 1, b0 - 1:b1 + 1] = False
    f = np.where(iso, 1.0, -1.0)
    f[b0:b1, b0:b1, b0:b1] = 1.0
    f[b0 + 2, b0 + 2, b0 + 2] = 0.0                       # inside the block: interior at threshold 0
    f[b0 + 3, b0 + 2, b0 + 2] = -0.0
    where = np.flatnonzero(iso)
    pick = rng.choice(where, sum(n for _, n in edge), replace=False)
    at = 0
    for v, n in edge:
        f.reshape(-1)[pick[at:at + n]] = v
        at += n
    odd = np.flatnonzero(~iso & (f < 0))                  # exterior whatever the threshold: NaN >= thr is false
    f.reshape(-1)[rng.choice(odd, 50, replace=False)] = np.nan
    return f, iso


def _components(f, iso, threshold):
    """the number of components by construction: every isolated lattice voxel at or above the threshold, and the block"""
    return int(np.count_nonzero(f[iso] >= threshold)) + 1


@pytest.mark.parametrize("threshold", [0.0, 0.5])
def test_remove_artifacts_at_the_root_list_capacity(pkg, oracle, monkeypatch, threshold):
    """C components known by construction: R2S_CCL_ROOTS_CAP = C fills the list of roots exactly (the list path),
    C - 1 makes it overflow by one (the sweeps over all counters).  Both must flip what the oracle flips, to the bit
    (0.0 and -0.0 are interior at threshold 0 and come back as -0.0, NaN is exterior), at a ratio that flips every
    isolated voxel and one that flips none."""
    rng = np.random.default_rng(41)
    lo, hi = np.zeros(3), np.ones(3)
    pg, og = pkg.Grid(lo, hi, 27, 1), oracle.grid_make(lo, hi, 27, 1)
    assert pg.dims == (30, 30, 30)
    f, iso = _isolated_and_block(pg.dims, lambda i, j, k: (i % 2 == 0) & (j % 2 == 0) & (k % 2 == 0), 4, 12,
                                 [(0.0, 30), (-0.0, 30), (np.nan, 30), (0.5, 30), (0.25, 30)], rng)
    C = _components(f, iso, threshold)
    assert 2000 < C < 4000
    sdf = f.reshape(-1)
    for cap in (C, C - 1):
        monkeypatch.setenv("R2S_CCL_ROOTS_CAP", str(cap))
        pkg._lib.lib().r2s_release_cache()                # a fresh list: no roots left over from an earlier call
        for ratio, flips in ((0.001, 0), (0.01, C - 1)):  # min size round(ratio * 512) = 1 / 5
            a, b = sdf.copy(), sdf.copy()
            na = pkg.remove_sdf_artifacts(a, pg, threshold=threshold, min_component_ratio=ratio)
            nb = oracle.remove_artifacts(b, og, threshold, ratio)
            assert na == nb == flips, (cap, ratio, na, nb, flips)
            assert np.array_equal(_bits(a), _bits(b)), (cap, ratio, int((_bits(a) != _bits(b)).sum()))


def test_remove_artifacts_more_components_than_the_root_list(pkg, oracle, monkeypatch):
    """a checkerboard of isolated voxels on 205^3 and one 40^3 block: more than 2^22 components, more than the list
    of roots holds without any knob (the sweeps take over; nothing may read past the list)"""
    monkeypatch.delenv("R2S_CCL_ROOTS_CAP", raising=False)
    rng = np.random.default_rng(43)
    lo, hi = np.zeros(3), np.ones(3)
    pg, og = pkg.Grid(lo, hi, 202, 1), oracle.grid_make(lo, hi, 202, 1)
    assert pg.dims == (205, 205, 205)
    f, iso = _isolated_and_block(pg.dims, lambda i, j, k: (i + j + k) % 2 == 0, 10, 50,
                                 [(0.0, 1000), (-0.0, 1000), (np.nan, 1000)], rng)
    C = _components(f, iso, 0.0)
    assert C == int(iso.sum()) - 1000 + 1 and C > (1 << 22)
    sdf = f.reshape(-1)
    del f, iso
    for ratio, flips in ((1e-5, 0), (0.01, C - 1)):      # min size 1 / 640 against the block's 64000
        a, b = sdf.copy(), sdf.copy()
        na = pkg.remove_sdf_artifacts(a, pg, min_component_ratio=ratio)
        nb = oracle.remove_artifacts(b, og, 0.0, ratio)
        assert na == nb == flips, (ratio, na, nb, flips)
        assert np.array_equal(_bits(a), _bits(b)), (ratio, int((_bits(a) != _bits(b)).sum()))


# ---- B. the early delivery of the fine field of r2s_rho2sdf --------------------------------------------------------

# beam_vfrac_04 on manual grids: name -> (N_max, rbf_grid, rbf_interp).  The fine grids have 2 N + 1 points per axis,
# so their Z extents are odd: the four chunks the field is delivered in have unequal sizes.
BEAM = {
    "big": (250, "fine", True),        # 257 x 91 x 24 coarse (561 k), 513 x 181 x 47 fine (4.36 M)
    "bigger": (270, "fine", True),     # 5.50 M fine: the session's landing zone grows
    "small": (240, "fine", True),      # 3.84 M fine: below 2^22, not early
    "big_approx": (250, "fine", False),
    "same": (532, "same", True),       # 539 x 185 x 43 = 4.29 M >= 162^3, one fine point per coarse point
}
# the early child's calls in order: (label, case, kind of fine_out / dists_out)
EARLY_CALLS = [
    ("pinned", "big", "pinned"),
    ("pageable", "big", "pageable"),
    ("pageable+4", "big", "pageable+4"),
    ("pinned+4", "big", "pinned+4"),
    ("bigger", "bigger", "pageable"),
    ("small", "small", "pageable"),
    ("big_again", "big", "pageable"),
    ("big_approx", "big_approx", "pageable"),
    ("same_pinned", "same", "pinned"),
    ("same_pageable+4", "same", "pageable+4"),
]


def _beam_grid(pkg, X, N):
    return pkg.Grid(X.min(0), X.max(0), N, 3)


def _beam_outputs(pkg, kind, nfine, ngp):
    """fine_out (Float32) / dists_out (Float64): pinned or pageable, 64-byte aligned or one value off"""
    alloc = pkg.host_array if kind.startswith("pinned") else _pageable
    if kind.endswith("+4"):
        return _at(alloc, nfine, np.float32, 16, 4), _at(alloc, ngp, np.float64, 32, 8)
    return _at(alloc, nfine, np.float32, 64, 0), _at(alloc, ngp, np.float64, 64, 0)


def _early_child(out_dir, early):
    """early == 0: every case once, with R2S_FINE_EARLY=0; else EARLY_CALLS in one process"""
    import __graft_entry__ as graft
    pkg = graft.load_built()
    X, IEN, rho = load_fixture("beam_vfrac_04")
    calls = EARLY_CALLS if early else [(name, name, "pageable") for name in BEAM]
    report = {}
    for label, case, kind in calls:
        N, rbf_grid, interp = BEAM[case]
        pg = _beam_grid(pkg, X, N)
        nfine = int(np.prod([int(n) * (2 if rbf_grid == "fine" else 1) + 1 for n in pg.N]))
        fine_out, dists_out = _beam_outputs(pkg, kind, nfine, pg.ngp)
        fine_out[:] = 7.0 if early else np.nan            # nothing stale may pass, and the twins are filled differently
        dists_out[:] = 7.0 if early else np.nan
        opts = pkg.Rho2sdfOptions(threshold_density=0.518555, rbf_interp=interp, rbf_grid=rbf_grid)
        info = {}
        fine, _, _, dists = pkg.rho2sdf("beam", X, IEN, rho, options=opts, sdf_grid=pg, info=info,
                                        fine_out=fine_out, dists_out=dists_out)
        assert np.shares_memory(fine, fine_out) and dists is dists_out
        np.save(os.path.join(out_dir, f"{label}_fine.npy"), fine.reshape(-1))
        np.save(os.path.join(out_dir, f"{label}_dists.npy"), dists)
        report[label] = {"case": case, "nfine": nfine, "level_shift": info["level_shift"], "cg_iters": info["cg_iters"],
                         "n_flipped": info["n_flipped"], "fine_addr": fine_out.ctypes.data % 64,
                         "pinned": kind.startswith("pinned")}
    with open(os.path.join(out_dir, "report.json"), "w") as fh:
        json.dump(report, fh)


def test_rho2sdf_early_fine_field(pkg, oracle, tmp_path):
    """r2s_rho2sdf with more than 2^22 fine points: the field arrives without its level shift before the level is known
    and host threads add it.  Into pinned and pageable arrays, 16-byte aligned and one value off (the alignment
    prologue, the scalar tail, the in-place add on the caller's own pinned array), through a session whose landing
    zone grows, with a call below 2^22 in between and on a :same grid: every result equals the same call with
    R2S_FINE_EARLY=0 bit for bit, and the approximation leg equals the oracle at the approximation tolerance."""
    import threading
    env = {k: v for k, v in os.environ.items() if k not in ("R2S_FINE_EARLY", "R2S_FINE_CHUNKS")}
    X, IEN, rho = load_fixture("beam_vfrac_04")
    ref_oracle = {}

    def run_oracle():                                     # the CPU reference while the children use the GPU
        N = BEAM["big_approx"][0]
        og = oracle.grid_make(X.min(0), X.max(0), N, 3)
        orn = oracle.dense_in_nodes(X, IEN, rho)
        d, _, _ = oracle.eval_distances(X, IEN, orn, 0.518555, og, 1.1, want_xp=False)
        ref = d * oracle.sign_detection(X, IEN, orn, 0.518555, og)
        oracle.remove_artifacts(ref, og)
        vd, vf = oracle.mesh_volume(X, IEN, rho)
        ref_oracle["dists"] = ref.copy()
        ref_oracle["fine"], ref_oracle["th"], _, ref_oracle["lsf"] = oracle.rbf_smoothing(ref, og, False, 2, vd * vf)

    th_oracle = threading.Thread(target=run_oracle)
    th_oracle.start()
    try:
        dirs = {}
        for early in (0, 1):
            d = tmp_path / f"early{early}"
            d.mkdir()
            _run_child("_early_child", (str(d), early), env if early else dict(env, R2S_FINE_EARLY="0"), timeout=180)
            dirs[early] = d
    finally:
        th_oracle.join()
    rep0 = json.loads((dirs[0] / "report.json").read_text())
    rep1 = json.loads((dirs[1] / "report.json").read_text())
    assert rep1["pageable+4"]["fine_addr"] % 16 == 4 and rep1["pinned+4"]["fine_addr"] % 16 == 4
    for label, case, kind in EARLY_CALLS:
        r0, r1 = rep0[case], rep1[label]
        assert (r1["nfine"] >= (1 << 22)) == (case != "small")
        assert (r1["level_shift"], r1["cg_iters"], r1["n_flipped"]) == (r0["level_shift"], r0["cg_iters"], r0["n_flipped"]), label
        for what in ("fine", "dists"):
            a = np.load(dirs[1] / f"{label}_{what}.npy")
            b = np.load(dirs[0] / f"{case}_{what}.npy")
            assert not np.isnan(b).any(), f"{case}: the R2S_FINE_EARLY=0 call left {what} values unwritten"
            diff = int((_bits(a) != _bits(b)).sum())
            assert diff == 0, f"{label} ({case}, {kind}): {diff} values of {what} differ from the R2S_FINE_EARLY=0 call"
    # the large-grid result is right, not only self-consistent (tolerances of test_rbf_smoothing's approximation leg)
    fine = np.load(dirs[1] / "big_approx_fine.npy")
    dists = np.load(dirs[1] / "big_approx_dists.npy")
    ref, ofine, oth, olsf = ref_oracle["dists"], ref_oracle["fine"].reshape(-1), ref_oracle["th"], ref_oracle["lsf"]
    real = np.abs(ref) < 1e9
    assert np.array_equal(_bits(dists[~real]), _bits(ref[~real]))
    assert np.allclose(dists[real], ref[real], rtol=1e-6, atol=1e-12)
    scale = np.abs(olsf).max()
    th = np.float32(rep1["big_approx"]["level_shift"])
    assert abs(th - oth) <= 1e-3 * scale
    err = np.abs((fine - th) - (ofine - np.float32(oth))).max()
    assert err <= 2e-6 * scale, err / scale


# ---- C. the streaming stores of the sparse download -----------------------------------------------------------------

def _nt_grids(pkg):
    """(label, mesh, grid): 172^3, and 184 x 147 x 159 (nx % 4 == 0; partial tiles in y and z), HEX8 and TET4"""
    from rho2sdf_jl_amd import synthetic
    out = []
    for tets in (False, True):
        X, IEN, rn = (synthetic.tet_mesh if tets else synthetic.hex_mesh)(9)
        pad = np.array([0.4, 0.1, 0.2])
        grids = {"cube": pkg.Grid(X.min(0), X.max(0), synthetic.grid_n_max_for_points(172), 3),
                 "box": pkg.Grid(X.min(0) - pad, X.max(0) + pad, 177, 3)}
        for name, pg in grids.items():
            out.append((f"{name}_{'tet4' if tets else 'hex8'}", (X, IEN, rn), pg))
    return out


NT_OUTPUTS = {   # kind -> (allocator, address modulo 32)
    "pinned": ("pinned", 0),
    "pageable32": ("pageable", 0),
    "pageable32+8": ("pageable", 8),
}


def _nt_child(ref_dir, report_path):
    """every grid x output kind, twice in a row, against the device results the parent saved"""
    import __graft_entry__ as graft
    pkg = graft.load_built()
    report = {}
    for label, (X, IEN, rn), pg in _nt_grids(pkg):
        want = np.load(os.path.join(ref_dir, label + ".npy"), mmap_mode="r")
        mesh = pkg.Mesh(X, IEN)
        for kind, (alloc, rem) in NT_OUTPUTS.items():
            out = _at(pkg.host_array if alloc == "pinned" else _pageable, pg.ngp, np.float64, 32, rem)
            for rep in range(2):
                out[:] = 7.0                              # nothing of the previous call may survive
                got = pkg.sdf_fused(mesh, pg, rn, 0.5, out=out)
                assert got is out
                report[f"{label}/{kind}/{rep}"] = int((_bits(got) != _bits(np.asarray(want))).sum())
    with open(report_path, "w") as fh:
        json.dump(report, fh)


@pytest.fixture(scope="module")
def nt_reference(pkg, tmp_path_factory):
    """DevicePlan.run(..., sdf=...) of every grid of _nt_grids, saved for the children"""
    import torch
    d = tmp_path_factory.mktemp("nt_ref")
    dev = torch.device("cuda:0")
    plan = pkg.DevicePlan(0)
    for label, (X, IEN, rn), pg in _nt_grids(pkg):
        nx, ny, nz = pg.dims
        assert pg.ngp > (1 << 22) and nx % 4 == 0, (label, pg.dims)     # else the streaming stores are off
        dX, dI, dR = (torch.from_numpy(a).to(dev) for a in (X, IEN, rn))
        want = torch.empty(pg.ngp, dtype=torch.float64, device=dev)
        plan.run(dX, dI, dR, 0.5, pg, sdf=want)
        want = want.cpu().numpy()
        assert (np.abs(want) < 1e9).sum() > 10000 and (want == 1.0e10).any() and (want == -1.0e10).any()
        np.save(d / (label + ".npy"), want)
    plan.close()
    assert {pg.dims for _, _, pg in _nt_grids(pkg)} == {(172, 172, 172), (184, 147, 159)}
    return d


@pytest.mark.parametrize("knobs", [{}, {"R2S_HOST_NT": "1"}, {"R2S_HOST_NT": "0"},
                                   {"R2S_HOST_NT": "1", "R2S_HOST_MASKSKIP": "0"}],
                         ids=["default", "nt1", "nt0", "nt1-maskskip0"])
def test_host_pointer_sparse_download_streaming_stores(pkg, nt_reference, tmp_path, knobs):
    """r2s_sdf's sparse download with nx % 4 == 0: into a 32-byte-aligned output the band tiles go down by streaming
    stores, x-neighbouring tiles as pairs of half lines, and the rows of the sign-only tiles too (pinned outputs by
    default, pageable ones with R2S_HOST_NT=1); 8 bytes off, or with R2S_HOST_NT=0, the plain stores.  Bit-equal to
    the device path on a cube and on a box with partial tiles, HEX8 and TET4, twice in a row."""
    env = {k: v for k, v in os.environ.items() if k not in ("R2S_HOST_NT", "R2S_HOST_MASKSKIP", "R2S_HOST_SPARSE")}
    env.update(knobs)
    report_path = tmp_path / "report.json"
    _run_child("_nt_child", (str(nt_reference), str(report_path)), env, timeout=180)
    report = json.loads(report_path.read_text())
    assert len(report) == 4 * len(NT_OUTPUTS) * 2
    bad = {k: v for k, v in report.items() if v}
    assert not bad, f"voxels that differ from the device path: {bad}"
