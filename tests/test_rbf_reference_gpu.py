"""RBF smoothing on the GPU against the float64 restatement of RBFs4Smoothing.jl (rbf_ref64).

Every result here is compared with rbf_ref64, never only with another kernel: the restatement shares none of the
product's stencils, tables, coordinate arrays or CG driver.  The per-voxel bound is rbf_ref64.bound (m Float32 roundings
of the accumulator plus the distance / exp() term); each test prints the largest fraction of it that it observed."""
import ctypes
import math

import numpy as np
import pytest

import rbf_ref64 as ref
from conftest import load_fixture

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-8)


def _grid(pkg, dims, dyadic=True):
    dims = np.array(dims)
    if dyadic:   # (dyadic numbers: the cell count of `Grid` comes out exact)
        lo, h = np.array([0.375, -0.25, 0.125]), 0.125
    else:
        lo, h = np.array([0.013, -0.2, 0.07]), 0.1037
    g = pkg.Grid(lo, lo + h * (dims - 1.0), int(dims.max()) - 1, 0)
    assert g.dims == tuple(int(d) for d in dims)
    return g


def _geom(g, smooth):
    amin, amax, N = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N]
    return ref.coarse_axes(amin, amax, N), ref.fine_axes(amin, amax, N, smooth), float(g.c.cell_size)


def _set_modes(monkeypatch, mode):
    for name in ("R2S_RBF_MATVEC", "R2S_RBF_APPLY"):
        if mode == "default":
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, mode)


def _fraction(err, b, ok):
    sel = ok & (b > 0)
    assert (err[ok & (b == 0)] == 0).all()
    return float((err[sel] / b[sel]).max()) if sel.any() else 0.0


def _check_coarse(lsf, e, thr, ok=None):
    ok = (e["tie_d2"] < 0) if ok is None else ok
    err, b = np.abs(lsf.astype(np.float64) - e["val"]), ref.bound(e, thr)
    assert (err[ok] <= b[ok]).all(), ("lsf", float((err - b)[ok].max()), int((err[ok] > b[ok]).sum()))
    return _fraction(err, b, ok)


def _check_fine(fine, th, e, thr, ok=None):
    ok = (e["tie_d2"] < 0) if ok is None else ok
    want = (e["val"] + float(th)).astype(np.float32).astype(np.float64)
    err, b = np.abs(fine.astype(np.float64) - want), ref.fine_bound(e, th, thr)
    assert (err[ok] <= b[ok]).all(), ("fine", float((err - b)[ok].max()), int((err[ok] > b[ok]).sum()))
    return _fraction(err, b, ok)


def _check_level(oracle, lsf, th, edge, target, note):
    """the level shift: th in [-max lsf, -min lsf], and |V(lsf + th) - target| <= 1e-4 + 1e-5 target (+ Float32 sums) unless the 40-step
    bisection ran out - then no Float32 shift next to th reaches the tolerance either: the target volume lies between
    the volumes a few ulp to either side"""
    assert -float(lsf.max()) <= th <= -float(lsf.min()), note
    # (+ the spread of two Float32 sums of the cell volumes in different orders: the bisection saw its own sum)
    tol = 1e-4 + 1e-5 * target + 2.0 ** -24 * math.sqrt(lsf.size) * target
    v = oracle.volume_from_sdf(lsf + np.float32(th), edge)
    if abs(v - target) <= tol:
        return
    # after 40 halvings the bracket is range * 2^-40 wide (or a few ulp of th, where Float32 stops halving it); a
    # volume that jumps inside it (whole uniform regions switch at once) cannot be bisected to the tolerance
    delta = np.float32((float(lsf.max()) - float(lsf.min())) * 2.0 ** -39)
    lo, hi = np.float32(th) - delta, np.float32(th) + delta
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    vl, vh = oracle.volume_from_sdf(lsf + lo, edge), oracle.volume_from_sdf(lsf + hi, edge)
    assert min(vl, vh) - tol <= target <= max(vl, vh) + tol, (note, v, vl, vh, target)


# ---- impulse responses -----------------------------------------------------------------------------------------------

IMPULSE_DIMS = (9, 8, 9)


def _spikes(dims):
    nx, ny, nz = dims
    return [(4, 4, 4), (0, 0, 0), (nx - 1, 0, 4), (1, ny - 2, 4), (nx - 2, 3, 5)]   # interior, corner, edge, face, far x


@pytest.mark.parametrize("smooth", [1, 2, 3, 4])
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_rbf_impulse_responses(pkg, thr, smooth):
    """approximation mode with one weight of 1: the output is the stencil itself, so an extra or a missing tap shows even
    at 1e-8, where one tap is ~1e-7 of the field.  Coarse LSF and fine - th, at five spike positions"""
    g = _grid(pkg, IMPULSE_DIMS)
    nx, ny, nz = g.dims
    caxes, taxes, sigma = _geom(g, smooth)
    spikes = _spikes(g.dims)
    W = np.zeros((len(spikes), nz, ny, nx), dtype=np.float32)
    for b, (i, j, k) in enumerate(spikes):
        W[b, k, j, i] = 1.0
    ec = ref.evaluate(W, caxes, caxes, 1, sigma, thr)
    ef = ref.evaluate(W, caxes, taxes, smooth, sigma, thr)
    worst = 0.0
    for b, sp in enumerate(spikes):
        info = {}
        fine = pkg.RBFs_smoothing(W[b].astype(np.float64).ravel(), g, False, smooth, 2.0 * sigma ** 3, thr, info=info)
        for coarse, got, e, s in ((True, info["lsf"], ec, 1), (False, fine, ef, smooth)):
            # A tie at the cap matters only where it involves the spike.  On this dyadic lattice equal lattice distances
            # are equal Float32 distances: the reference leaves their order open, the product documents (d^2, dz, dy, dx)
            # and the restatement follows it - so the tied targets are compared too, against that order
            one = dict(val=e["val"][b], S=e["S"][b], m=e["m"], tie_d2=e["tie_d2"])
            ok = np.ones(got.shape, dtype=bool)
            if coarse:
                worst = max(worst, _check_coarse(got, one, thr, ok))
            else:
                worst = max(worst, _check_fine(got, info["th"], one, thr, ok))
    print(f"impulse thr={thr} smooth={smooth}: largest fraction of the bound {worst:.3g}")


# ---- realistic fields ------------------------------------------------------------------------------------------------

def _banded_spheres(g, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = g.dims
    ax = [g.AABB_min[a] + g.cell_size * np.arange(n) for a, n in enumerate((nx, ny, nz))]
    c = [0.45 * (a[0] + a[-1]) for a in ax]
    r = np.sqrt((ax[0][None, None, :] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2 + (ax[2][:, None, None] - c[2]) ** 2)
    sdf = 0.3 * g.cell_size * max(g.dims) - r + 0.01 * g.cell_size * rng.normal(size=r.shape)
    sdf = np.where(np.abs(sdf) < 4 * g.cell_size, sdf, np.sign(sdf) * 1e10).ravel()
    sdf[rng.random(sdf.size) < 0.03] = -1e10
    # the inside fraction of the lattice points times the volume of the cells: a volume the cells can hold
    return sdf, max(float((sdf > 0).mean()), 0.01) * (nx - 1) * (ny - 1) * (nz - 1) * g.cell_size ** 3


FIELD_CASES = [((4, 3, 5), 1), ((61, 7, 5), 1), ((5, 67, 3), 1), ((130, 9, 8), 1), ((311, 6, 6), 1), ((64, 64, 5), 1),
               ((261, 41, 37), 1), ((40, 23, 17), 2), ((21, 30, 13), 3), ((131, 9, 70), 2), ((12, 11, 15), 4)]


def _modes(smooth):
    return ("default", "fly", "lut") if smooth == 1 else ("default", "fly")


def _run_field(pkg, oracle, monkeypatch, g, sdf, target, smooth, thr, note):
    caxes, taxes, sigma = _geom(g, smooth)
    nx, ny, nz = g.dims
    w = ref.process_vector(sdf).reshape(nz, ny, nx)
    ec = ref.evaluate(w, caxes, caxes, 1, sigma, thr)
    ef = ref.evaluate(w, caxes, taxes, smooth, sigma, thr)
    worst = 0.0
    edge = float(caxes[0][1] - caxes[0][0])
    for mode in _modes(smooth):
        _set_modes(monkeypatch, mode)
        info = {}
        fine = pkg.RBFs_smoothing(sdf, g, False, smooth, target, thr, info=info)
        worst = max(worst, _check_coarse(info["lsf"], ec, thr), _check_fine(fine, info["th"], ef, thr))
        _check_level(oracle, info["lsf"], info["th"], edge, target, (note, mode))
    _set_modes(monkeypatch, "default")
    return worst


@pytest.mark.parametrize("dims,smooth", FIELD_CASES)
def test_rbf_fields_against_float64(pkg, oracle, monkeypatch, dims, smooth):
    """banded synthetic spheres with sentinels on the lattices of the kernel tests (the row walk, table and fine-table
    instantiations are the code under test), approximation mode, under every form of the evaluation"""
    g = _grid(pkg, dims)
    sdf, target = _banded_spheres(g, sum(dims) + smooth)
    worst = _run_field(pkg, oracle, monkeypatch, g, sdf, target, smooth, 1e-3, dims)
    if max(dims) <= 70:   # the capped evaluation on a few of them
        worst = max(worst, _run_field(pkg, oracle, monkeypatch, g, sdf, target, smooth, 1e-5, dims))
    print(f"field {dims}/{smooth}: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()


def _beam_raw_sdf(oracle):
    X, IEN, rho = load_fixture("beam_vfrac_04")
    rn = oracle.dense_in_nodes(X, IEN, rho)
    g, _ = oracle.auto_grid(X, IEN)
    d, _, _ = oracle.eval_distances(X, IEN, rn, 0.518555, g, 1.1, want_xp=False)
    sdf = d * oracle.sign_detection(X, IEN, rn, 0.518555, g)
    oracle.remove_artifacts(sdf, g)
    vd, vf = oracle.mesh_volume(X, IEN, rho)
    return X, IEN, sdf, vd * vf


def test_rbf_beam_against_float64(pkg, oracle, monkeypatch):
    """the beam's raw SDF on its own (non-dyadic) grid, :same and :fine, at the default threshold and where the knn cap
    binds"""
    X, IEN, sdf, target = _beam_raw_sdf(oracle)
    g = pkg.noninteractive_sdf_grid_setup(pkg.Mesh(X, IEN))
    worst = 0.0
    for smooth, thr in ((1, 1e-3), (2, 1e-3), (2, 1e-4), (1, 1e-5)):
        worst = max(worst, _run_field(pkg, oracle, monkeypatch, g, sdf, target, smooth, thr, ("beam", smooth, thr)))
    print(f"beam: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()


# ---- process_vector --------------------------------------------------------------------------------------------------

def test_rbf_process_vector_edges(pkg):
    """approximation mode is linear in the processed input, so the sentinel rule shows exactly: +-1e10 and
    1e10 (1 +- 3e-4) become +-max, 1e10 (1 + 4e-4) stays, 5e9 stays and is no candidate for the maximum, -0.0 stays"""
    g = _grid(pkg, (9, 8, 7))
    nx, ny, nz = g.dims
    caxes, taxes, sigma = _geom(g, 1)
    rng = np.random.default_rng(3)
    sdf = rng.uniform(-0.4, 0.7, nx * ny * nz)
    specials = [1e10, -1e10, 1e10 * (1 + 3e-4), -1e10 * (1 - 3e-4), 1e10 * (1 + 4e-4), 5e9, -0.0]
    pos = rng.choice(sdf.size, len(specials), replace=False)
    sdf[pos] = specials
    w = ref.process_vector(sdf)
    mx = np.float32(np.abs(sdf[np.abs(sdf) < 1e9]).max())
    assert w[pos[0]] == mx and w[pos[1]] == -mx and w[pos[2]] == mx and w[pos[3]] == -mx
    assert w[pos[4]] == np.float32(1e10 * (1 + 4e-4)) and w[pos[5]] == np.float32(5e9) and w[pos[6]] == 0.0
    worst = 0.0
    for field in (sdf, np.where(np.arange(sdf.size) == 17, 0.25, 1e10)):   # and a field with a single real value
        info = {}
        fine = pkg.RBFs_smoothing(field, g, False, 1, sigma ** 3, 1e-3, info=info)
        e = ref.evaluate(ref.process_vector(field).reshape(nz, ny, nx), caxes, caxes, 1, sigma, 1e-3)
        worst = max(worst, _check_coarse(info["lsf"], e, 1e-3))
        ef = ref.evaluate(ref.process_vector(field).reshape(nz, ny, nx), caxes, taxes, 1, sigma, 1e-3)
        worst = max(worst, _check_fine(fine, info["th"], ef, 1e-3))
    print(f"process_vector: largest fraction of the bound {worst:.3g}")
    sent = np.full(sdf.size, -1e10)
    with pytest.raises(pkg._lib.R2SError):
        pkg.RBFs_smoothing(sent, g, False, 1, 1.0)
    import torch
    d = torch.tensor(sent, dtype=torch.float64, device="cuda:0")
    out = torch.empty(sdf.size, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(pkg._lib.R2SError):
        _smooth_dev(pkg, d, g, False, 1, 1e-3, 1.0, out)


def test_rbf_kernel_threshold_limit(pkg):
    """thresholds below R2S_RBF_MIN_KERNEL_THRESHOLD (1e-10) need stencils beyond the kernels' 512 entries: an error"""
    g = _grid(pkg, (6, 5, 4))
    sdf = np.linspace(-1.0, 1.0, 6 * 5 * 4)
    for thr in (9e-11, 0.0, 1.0):
        with pytest.raises(pkg._lib.R2SError):
            pkg.RBFs_smoothing(sdf, g, False, 2, 1.0, thr)
    assert np.isfinite(pkg.RBFs_smoothing(sdf, g, False, 4, 0.05, 1e-10)).all()


# ---- interpolation mode ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thr", [0.1, 1e-2, 1e-3, 1e-4])
@pytest.mark.parametrize("dims,smooth", [((40, 23, 17), 2), ((21, 30, 13), 3), ((61, 7, 5), 1), ((12, 11, 15), 4)])
def test_rbf_interpolation_residual(pkg, dims, smooth, thr):
    """CG of compute_rbf_weights: the evaluation of the weights at the lattice (pinned by the impulse and field tests)
    reproduces the processed input, ||lsf - b|| <= 2 sqrt(eps(Float32)) ||b||, unless the iteration count reached n; on
    these dyadic refined grids the fine field at the coarse nodes, minus th, equals lsf"""
    g = _grid(pkg, dims)
    sdf, target = _banded_spheres(g, 7 * sum(dims))
    b = ref.process_vector(sdf).astype(np.float64)
    info = {}
    fine = pkg.RBFs_smoothing(sdf, g, True, smooth, target, thr, info=info)
    lsf = info["lsf"].astype(np.float64).ravel()
    n = sdf.size
    rel = np.linalg.norm(lsf - b) / np.linalg.norm(b)
    assert info["cg_iterations"] >= n or rel <= 2 * float(ref.RTOL32), (rel, info["cg_iterations"])
    at = fine[::smooth, ::smooth, ::smooth].astype(np.float64) - float(info["th"])
    lsf3 = info["lsf"].astype(np.float64)
    assert at.shape == lsf3.shape
    tol = 2.0 ** -23 * (np.abs(lsf3) + abs(float(info["th"])))
    assert (np.abs(at - lsf3) <= tol).all(), float(np.abs(at - lsf3).max())
    print(f"interpolation {dims}/{smooth} thr={thr}: residual {rel:.3g} of ||b||, {info['cg_iterations']} iterations")
    pkg._lib.lib().r2s_release_cache()


# ---- device-pointer entry and the slab-distributed path -----------------------------------------------------------------

def _smooth_dev(pkg, d_sdf, g, interp, smooth, thr, target, d_out):
    L = pkg._lib
    th, its = ctypes.c_float(), ctypes.c_int32()
    L.check(L.lib().r2s_rbf_smooth_dev(ctypes.c_void_p(d_sdf.data_ptr()), ctypes.byref(g.c), int(interp), int(smooth),
                                       float(thr), float(target), ctypes.c_void_p(d_out.data_ptr()), ctypes.byref(th),
                                       ctypes.byref(its), None))
    return th.value, its.value


@pytest.mark.parametrize("interp,smooth,thr", [(False, 2, 1e-3), (True, 1, 1e-3), (False, 3, 1e-5)])
def test_rbf_smooth_dev_matches_host_entry(pkg, interp, smooth, thr):
    """r2s_rbf_smooth_dev on torch tensors: bit for bit the host entry's result"""
    import torch
    g = _grid(pkg, (40, 23, 17))
    sdf, target = _banded_spheres(g, 11)
    info = {}
    want = pkg.RBFs_smoothing(sdf, g, interp, smooth, target, thr, info=info)
    d = torch.tensor(sdf, dtype=torch.float64, device="cuda:0")
    out = torch.full((want.size,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    th, its = _smooth_dev(pkg, d, g, interp, smooth, thr, target, out)
    got = out.cpu().numpy().reshape(want.shape)
    assert th == info["th"] and its == info["cg_iterations"]
    assert np.array_equal(got, want)
    pkg._lib.lib().r2s_release_cache()


def test_rbf_slabs_capped_threshold(pkg, oracle, monkeypatch):
    """r2s_rho2sdf at rbf_kernel_threshold 1e-5 (knn cap binding): 3 slab devices (R2S_MULTI_OVERSUBSCRIBE) equal one
    device bit for bit, and the one-device fine field matches the float64 restatement on the call's own sdf_dists"""
    monkeypatch.setenv("R2S_MULTI_OVERSUBSCRIBE", "1")
    X, IEN, rho = load_fixture("beam_vfrac_04")
    pg = pkg.noninteractive_sdf_grid_setup(pkg.Mesh(X, IEN))
    thr = 1e-5
    opts = pkg.Rho2sdfOptions(threshold_density=0.518555, rbf_interp=False, rbf_grid="fine", rbf_kernel_threshold=thr)
    ia, ib = {}, {}
    a = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=pg, info=ia)
    b = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=pg, n_gpus=3, info=ib)
    assert ia["level_shift"] == ib["level_shift"]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[0], b[0])
    caxes, taxes, sigma = _geom(pg, 2)
    nx, ny, nz = pg.dims
    w = ref.process_vector(a[3]).reshape(nz, ny, nx)
    ef = ref.evaluate(w, caxes, taxes, 2, sigma, thr)
    worst = _check_fine(a[0], ia["level_shift"], ef, thr)
    print(f"slabs at 1e-5: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()
