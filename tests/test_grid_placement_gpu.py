"""The raw signed-distance path on grids that are not the mesh's own box, and on meshes in other units at other positions.

Every other raw-SDF test builds Grid(X.min(0), X.max(0), n, 3) or the automatic grid on a mesh of unit-sized elements next to
the origin.  Here (cases: tests/grid_placement_cases.py; the reference conditions are proven by
tests/test_grid_placement_cpu.py on the oracle alone):

1. parity with the oracle (test_parity_gpu._compare, unchanged) on windows that zoom into the mesh, hang over a corner, miss
   it, contain it, are two planes thin, move the 4x4x4 tile origin through the residues mod 4, or lie 2^30 away;
2. without the oracle: every entry point on a window is bit-equal to the crop of the same call on the full grid - the
   coordinates are the same doubles and the element order is unchanged, so a difference is a dependence on tile alignment or
   a candidate lost at a window edge;
3. DevicePlan.run on a window in three Z slabs (one of them past the mesh where the window allows it), and a second call of
   the same shapes on another window (the speculated-sizes path) against a fresh plan;
4. r2s_rho2sdf on a window, one and three (oversubscribed) devices;
5. the sparse host download on a grid that cuts the mesh, at the size where it switches on, against the device path and
   the dense download;
6. parity with the oracle on the scaled, shifted and anisotropically scaled mesh; HEX8 at scales 2^-10 and 2^10 also
   bit-equal to the unscaled GPU result after unscaling.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_placement_cases as C
from conftest import ROOT
from test_parity_gpu import _compare

pytestmark = pytest.mark.gpu
KINDS = ("hex8", "tet4")
ENTRY_POINTS = ("dist", "xp", "sign", "sdf")


def _entry_points(pkg, X, IEN, rn, pg, stats=None):
    """evalDistances, Sign_Detection and sdf_fused on grid pg -> dict of (nz, ny, nx[, 3]) arrays"""
    nx, ny, nz = pg.dims
    mesh = pkg.Mesh(X, IEN)
    st = [{}, {}, {}]
    dist, xp = pkg.evalDistances(mesh, pg, rn, C.RHO_T, band_factor=C.BAND_FACTOR, stats=st[0])
    sign = pkg.Sign_Detection(mesh, pg, rn, C.RHO_T, stats=st[1])
    sdf = pkg.sdf_fused(mesh, pg, rn, C.RHO_T, band_factor=C.BAND_FACTOR, stats=st[2])
    if stats is not None:
        stats.extend(st)
    return {"dist": dist.reshape(nz, ny, nx), "xp": xp.reshape(nz, ny, nx, 3), "sign": sign.reshape(nz, ny, nx),
            "sdf": sdf.reshape(nz, ny, nx)}


@pytest.fixture(scope="module")
def gpu_full(pkg):
    """the three entry points on the full 39^3 grid, once per element type, read-only"""
    out = {}
    for kind in KINDS:
        X, IEN, rn = C.mesh(kind)
        out[kind] = _entry_points(pkg, X, IEN, rn, C.full_grid(pkg.Grid))
        for a in out[kind].values():
            a.setflags(write=False)
    return out


SENTINEL = {"dist": 1.0e10, "sign": -1.0, "sdf": -1.0e10, "xp": 0.0}


# ---- 1. parity on the window ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(C.WINDOWS))
def test_window_parity_with_the_oracle(pkg, oracle, kind, name):
    X, IEN, rn = C.mesh(kind)
    pg, og = C.window_grid(pkg.Grid, name), C.window_grid(oracle.grid_make, name)
    assert pg.dims == og.dims
    _compare(pkg, oracle, X, IEN, rn, C.RHO_T, pg, og, C.BAND_FACTOR, f"window {name} {kind}")
    if name in C.EMPTY_WINDOWS:
        # the mesh has work items, every one of them with an empty box on this grid: nothing may be launched over an empty
        # list, and the outputs are the sentinel everywhere
        stats = []
        got = _entry_points(pkg, X, IEN, rn, pg, stats)
        for key in ENTRY_POINTS:
            assert np.all(got[key] == SENTINEL[key]), (name, kind, key)
        assert not np.signbit(got["xp"]).any()
        for st in stats:
            assert st["n_active_tiles"] == 0 and st["n_active_sign_tiles"] == 0 and st["n_any_tiles"] == 0, (name, kind, st)
            assert st["n_band_entries"] == 0 and st["n_sign_entries"] == 0 and st["n_iso_chunks"] == 0, (name, kind, st)


# ---- 2. window == crop of the full grid, no oracle --------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(C.WINDOWS))
def test_window_equals_crop_of_the_full_grid(pkg, gpu_full, kind, name):
    """(`superset` the other way round: the full grid is the crop of the window - the same comparison of the overlap)"""
    X, IEN, rn = C.mesh(kind)
    got = _entry_points(pkg, X, IEN, rn, C.window_grid(pkg.Grid, name))
    ov = C.overlap(name)
    outside = np.ones(C.dims3(name), dtype=bool)
    bad = {}
    if ov is not None:
        outside[ov[0]] = False
        for key in ENTRY_POINTS:
            ne = C.bits(got[key][ov[0]]) != C.bits(gpu_full[kind][key][ov[1]])
            if ne.any():
                where = np.argwhere(ne.any(axis=-1) if key == "xp" else ne)
                bad[key] = (len(where), where[:5].tolist())
    assert not bad, f"{name} {kind}: (voxels that differ from the crop, first window indices z y x) {bad}"
    for key in ENTRY_POINTS:
        assert np.all(got[key][outside] == SENTINEL[key]), (name, kind, key)
    print(f"{name} {kind}: {int((~outside).sum())} shared voxels bit-equal in dist, xp, sign, sdf; "
          f"{int(outside.sum())} voxels off the full grid all sentinel")


# ---- 3. the plan API on a window -------------------------------------------------------------------------------------

PLAN_CASES = {   # window -> (Z slab bounds, index of the slab that holds no mesh or None, the second window of the same shape)
    "corner-out": ((0, 6, 11, 17), 2, ((27, 26, -8), (16, 16, 16))),   # planes 11.. lie at z >= 1.375, the mesh ends at 1
    "align1": ((0, 5, 11, 16), None, C.WINDOWS["align2"]),              # (an interior window: every plane cuts the mesh)
}
PLAN_MODES = (("sdf",), ("dist", "sign", "sdf", "xp"))


def _plan_run(torch, plan, dev_mesh, pg, names, k0=0, k1=None):
    nx, ny, nz = pg.dims
    k1 = nz if k1 is None else k1
    out = {n: torch.full(((k1 - k0) * ny * nx * (3 if n == "xp" else 1),), 7.0, dtype=torch.float64, device=dev_mesh[0].device)
           for n in names}
    st = plan.run(*dev_mesh, C.RHO_T, pg, k_begin=k0, k_end=k1, band_factor=C.BAND_FACTOR, **out)
    torch.cuda.synchronize()
    return out, st


def _same_bits(torch, a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("names", PLAN_MODES, ids=["sdf", "all"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_slabs_and_speculated_sizes_on_a_window(pkg, gpu_full, name, kind, names):
    import torch
    bounds, empty, other = PLAN_CASES[name]
    X, IEN, rn = C.mesh(kind)
    dev = torch.device("cuda:0")
    dev_mesh = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, IEN, rn))
    pg = C.window_grid(pkg.Grid, name)
    nx, ny, nz = pg.dims
    assert bounds[0] == 0 and bounds[-1] == nz
    plan = pkg.DevicePlan(0)
    one, _ = _plan_run(torch, plan, dev_mesh, pg, names)
    # the plan equals the host entry points (which test 2 ties to the full grid)
    ov = C.overlap(name)
    sdf = one["sdf"].cpu().numpy().reshape(nz, ny, nx)
    assert np.array_equal(C.bits(sdf[ov[0]]), C.bits(gpu_full[kind]["sdf"][ov[1]]))
    pieces = {n: [] for n in names}
    for s, (k0, k1) in enumerate(zip(bounds[:-1], bounds[1:])):
        out, st = _plan_run(torch, plan, dev_mesh, pg, names, k0, k1)
        if s == empty:
            assert st["n_any_tiles"] == 0 and st["n_active_tiles"] == 0, st
            for n in names:
                assert bool((out[n] == SENTINEL[n]).all()), (name, kind, n)
        for n in names:
            pieces[n].append(out[n])
    for n in names:
        assert _same_bits(torch, torch.cat(pieces[n]), one[n]), f"{name} {kind}: {n} in 3 slabs differs from one call"
    # the same shapes again, then on another window: sizes remembered from the first, data behind them changed
    again, _ = _plan_run(torch, plan, dev_mesh, pg, names)
    pg2 = C.window_grid_at(pkg.Grid, *other)
    assert pg2.dims == pg.dims
    second, _ = _plan_run(torch, plan, dev_mesh, pg2, names)
    plan.close()
    fresh = pkg.DevicePlan(0)
    want, _ = _plan_run(torch, fresh, dev_mesh, pg2, names)
    fresh.close()
    for n in names:
        assert _same_bits(torch, again[n], one[n]), (name, kind, n)
        assert _same_bits(torch, second[n], want[n]), f"{name} {kind}: {n} on the second window differs from a fresh plan's"
    assert bool((want["sdf"] != -1.0e10).any())


# ---- 4. the whole call on a window ------------------------------------------------------------------------------------

def _rho2sdf_raw(pkg, X, IEN, rho, grid, n_gpus):
    """r2s_rho2sdf through the C ABI with skip_rbf: (raw field, field after artifact removal, nodal densities, rho_t)"""
    L = pkg._lib
    mesh = pkg.Mesh(X, IEN)
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    o = L.R2SOptions()
    L.lib().r2s_default_options(ctypes.byref(o))
    o.threshold_density = C.RHO_T
    o.band_factor = C.BAND_FACTOR
    o.elem_type = mesh.element_type
    o.skip_rbf = 1
    o.n_gpus = int(n_gpus)
    raw, dists, rho_n = np.empty(grid.ngp), np.empty(grid.ngp), np.empty(mesh.nnp)
    ri = L.R2SRunInfo()
    L.check(L.lib().r2s_rho2sdf(mesh.X.ctypes.data_as(L.c_double_p), mesh.nnp, mesh.IEN.ctypes.data_as(L.c_int64_p),
                                mesh.nel, rho.ctypes.data_as(L.c_double_p), ctypes.byref(o), ctypes.byref(grid.c),
                                rho_n.ctypes.data_as(L.c_double_p), raw.ctypes.data_as(L.c_double_p),
                                dists.ctypes.data_as(L.c_double_p), None, ctypes.byref(ri)))
    return raw, dists, rho_n, ri.rho_t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["interior", "corner-out"])
def test_whole_call_on_a_window(pkg, monkeypatch, name, kind):
    X, IEN, rn = C.mesh(kind)
    rho = rn[IEN - 1].mean(axis=1)                       # element densities; the call makes its own nodal ones
    pg = C.window_grid(pkg.Grid, name)
    monkeypatch.setenv("R2S_MULTI_OVERSUBSCRIBE", "1")
    res = {G: _rho2sdf_raw(pkg, X, IEN, rho, pg, G) for G in (1, 3)}
    pkg._lib.lib().r2s_release_cache()
    for G, (raw, dists, rho_n, rho_t) in res.items():
        assert rho_t == C.RHO_T
        want = pkg.sdf_fused(pkg.Mesh(X, IEN), pg, rho_n, rho_t, band_factor=C.BAND_FACTOR)
        assert np.array_equal(C.bits(raw), C.bits(want)), f"{name} {kind} n_gpus {G}: {int((C.bits(raw) != C.bits(want)).sum())} voxels"
        assert (np.abs(want) < 1e9).any()
    assert np.array_equal(C.bits(res[1][2]), C.bits(res[3][2]))
    assert np.array_equal(C.bits(res[1][1]), C.bits(res[3][1])), f"{name} {kind}: sdf_dists differs between 1 and 3 devices"


# ---- 5. the sparse host download on a grid that cuts the mesh --------------------------------------------------------

SPARSE_BOX = (np.array([-1.0, -1.0, -1.0]), np.array([0.75, 1.0, 1.0]), 168, 0)   # [-1, 1]^3 minus an eighth in X, no margin


def _dense_child(path):
    """sdf_fused on the sparse-download grid, in a process started with R2S_HOST_SPARSE=0 (read once per process)"""
    import __graft_entry__ as graft
    pkg = graft.load_built()
    assert os.environ["R2S_HOST_SPARSE"] == "0"
    X, IEN, rn = C.mesh("hex8")
    np.save(path, pkg.sdf_fused(pkg.Mesh(X, IEN), pkg.Grid(*SPARSE_BOX), rn, C.RHO_T, band_factor=C.BAND_FACTOR))


def test_sparse_host_download_on_a_grid_that_cuts_the_mesh(pkg, tmp_path):
    """148 x 169 x 169 = 4 227 028 voxels, the first size of this box at or above the 2^22 voxels from which r2s_sdf brings
    only the non-sentinel tiles down (167 cells: 4 177 152, dense).  The grid has no margin and ends at x = 0.75: band and
    sign-only tiles lie on five of its faces."""
    import torch
    assert os.environ.get("R2S_HOST_SPARSE") is None, "this test compares the default (sparse) download with the dense one"
    pg = pkg.Grid(*SPARSE_BOX)
    nx, ny, nz = pg.dims
    assert (nx, ny, nz) == (148, 169, 169) and pg.ngp >= 1 << 22 > 148 * 168 * 168
    X, IEN, rn = C.mesh("hex8")
    st = {}
    got = pkg.sdf_fused(pkg.Mesh(X, IEN), pg, rn, C.RHO_T, band_factor=C.BAND_FACTOR, stats=st)
    assert st["n_active_tiles"] > 0
    print(f"sparse download: {st['n_active_tiles']} band tiles, {st['n_sign_only_tiles']} sign-only tiles of {st['n_tiles']}")
    dev = torch.device("cuda:0")
    dev_mesh = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, IEN, rn))
    plan = pkg.DevicePlan(0)
    want = torch.empty(pg.ngp, dtype=torch.float64, device=dev)
    plan.run(*dev_mesh, C.RHO_T, pg, band_factor=C.BAND_FACTOR, sdf=want)
    want = want.cpu().numpy()
    plan.close()
    assert (np.abs(want) < 1e9).sum() > 100000 and (want == -1.0e10).any()
    assert np.abs(want.reshape(nz, ny, nx)[:, :, -1]).min() < 1e9       # the band reaches the cut face
    assert np.array_equal(C.bits(got), C.bits(want)), f"{int((C.bits(got) != C.bits(want)).sum())} voxels differ from the device path"
    path = str(tmp_path / "dense.npy")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_grid_placement_gpu as t; t._dense_child(%r)" % (
        ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, R2S_HOST_SPARSE="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    dense = np.load(path)
    assert np.array_equal(C.bits(got), C.bits(dense)), f"{int((C.bits(got) != C.bits(dense)).sum())} voxels differ from the dense download"


# ---- 6. units and position -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tname", list(C.TRANSFORMS))
def test_transformed_mesh_parity_with_the_oracle(pkg, oracle, gpu_full, tname, kind):
    """_compare prints the bit-equal count and the largest relative difference of every transform"""
    X, IEN, rn, lo, hi = C.transformed(kind, tname)
    pg = pkg.Grid(lo, hi, C.FULL_N_MAX, C.FULL_MARGIN)
    og = oracle.grid_make(lo, hi, C.FULL_N_MAX, C.FULL_MARGIN)
    assert pg.dims == og.dims
    _compare(pkg, oracle, X, IEN, rn, C.RHO_T, pg, og, C.BAND_FACTOR, f"transform {tname} {kind}")
    if kind == "hex8" and tname in C.EXACT_SCALES:
        # the oracle is exactly equivariant here (tests/test_grid_placement_cpu.py), so the kernels have to be
        sc = C.TRANSFORMS[tname][0]
        assert pg.dims == C.FULL_DIMS
        got, ref = _entry_points(pkg, X, IEN, rn, pg), gpu_full[kind]
        real = ref["dist"] < 1e9
        assert np.array_equal(got["dist"] < 1e9, real)
        assert np.array_equal(C.bits(got["sign"]), C.bits(ref["sign"]))
        for key in ("dist", "sdf"):
            assert np.array_equal(C.bits(got[key][~real]), C.bits(ref[key][~real])), (tname, key)      # +-1e10 does not scale
            ne = C.bits(got[key][real] / sc) != C.bits(ref[key][real])
            assert not ne.any(), f"{tname}: {int(ne.sum())} of {int(real.sum())} {key} values differ after unscaling"
        assert np.array_equal(C.bits(got["xp"] / sc), C.bits(ref["xp"])), tname
        print(f"transform {tname} hex8: {int(real.sum())} band voxels bit-equal to the unscaled GPU run after unscaling")
