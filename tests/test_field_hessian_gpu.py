"""Hessian and curvature of the smoothed level-set on the GPU against the float64 restatement (field_hess_ref64).

Lattice: 9 x 8 x 7 cells, non-dyadic aabb_min and cell_size, random Float32 weights, th != 0.  Per threshold (1e-1 small
support, 1e-3 production, 1e-5 cap and ranking wherever the support is not cut by a face, 1e-9 workgroup shrunk to 128 threads) 3 013 =
16 * 188 + 5 points: random inside, random up to 3 cells outside, every lattice node, NaN / inf / far rows.

    |H_ab - ref.H_ab| <= (6 ln(1/thr) + 12) 2^-24 S_ab + 2^-23 |H_ab| + slack (4 R^2 + 2) / sigma^2     (hess_bound)

Curvature is checked against the header's formulas applied to the library's own Float32 g and H (bounds in
test_curvature_follows_its_own_inputs), against the sphere of a single Gaussian, and end to end on the fitted sphere.
"""
import ctypes
import math

import numpy as np
import pytest

import field_hess_ref64 as FH
import rbf_ref64 as R64
from conftest import load_fixture

pytestmark = pytest.mark.gpu

LO, H = np.array([0.013, -0.2, 0.07]), 0.1037
DIMS = (10, 9, 8)                                  # nodes of the 9 x 8 x 7-cell lattice
THRESHOLDS = (1e-1, 1e-3, 1e-5, 1e-9)
TH = np.float32(0.3712)
_CACHE = {}


def _grid(pkg, dims=DIMS):
    dims = np.array(dims)
    g = pkg.Grid(LO, LO + H * (dims - 1.0), int(dims.max()) - 1, 0)
    assert g.dims == tuple(int(d) for d in dims)
    return g


def _ref_field(g, w, thr, th):
    return FH.HessField(w, np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N], float(g.c.cell_size), thr, th)


def _points(g, rng):
    amin, amax, N = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N]
    tx, ty, tz = R64.coarse_axes(amin, amax, N)
    Z, Y, X = np.meshgrid(tz, ty, tx, indexing="ij")
    lattice = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    inside = amin + rng.random((1700, 3)) * (amax - amin)
    wide = amin - 3.0 * H + rng.random((8 * 588, 3)) * (amax - amin + 6.0 * H)
    wide = wide[((wide < amin) | (wide > amax)).any(1)][:588]
    special = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [1e30, 0.0, 0.0], [amax[0] + 40 * H, 0.5, 0.5]])
    pts = np.vstack([inside, wide, lattice, special]).astype(np.float32)
    assert len(pts) == 3013 and len(pts) % 16 == 5
    return pts


def _case(pkg, thr):
    """weights, points, the restatement (computed once per threshold) and the library's outputs"""
    if thr in _CACHE:
        return _CACHE[thr]
    g = _grid(pkg)
    rng = np.random.default_rng(int(-math.log10(thr)) + 40)
    w = rng.standard_normal((DIMS[2], DIMS[1], DIMS[0])).astype(np.float32)
    pts = _points(g, rng)
    fld = _ref_field(g, w, thr, TH)
    ref = fld.hessian(pts)
    for v in ref.values():
        v.setflags(write=False)
    with pkg.RbfField(w, g, TH, thr, device=0) as f:
        val, grad, hess, taps = f.eval(pts, grad=True, hess=True, taps=True)
        ev, eg, et = f.eval(pts, grad=True, taps=True)
        curv = np.stack(f.curvature(pts), axis=1)
    _CACHE[thr] = dict(g=g, w=w, pts=pts, fld=fld, ref=ref, val=val, grad=grad, hess=hess, taps=taps, ev=ev, eg=eg, et=et, curv=curv)
    return _CACHE[thr]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_hessian_against_the_restatement(pkg, thr):
    """every finite point within hess_bound, component by component (tied points at the cap included: the restatement
    follows the index rule); value, gradient and taps of the Hessian call are r2s_rbf_field_eval's bits"""
    c = _case(pkg, thr)
    ref, fld, hess = c["ref"], c["fld"], c["hess"]
    assert np.array_equal(_bits(c["val"]), _bits(c["ev"])) and np.array_equal(_bits(c["grad"]), _bits(c["eg"]))
    assert np.array_equal(c["taps"], c["et"])
    fin = np.isfinite(ref["val"])
    assert int((~fin).sum()) == 3 and np.isnan(hess[~fin]).all() and (c["taps"][~fin] == 0).all()
    assert np.isfinite(hess[fin]).all()
    assert c["val"][-1] == TH and (c["grad"][-1] == 0).all() and (hess[-1] == 0).all() and c["taps"][-1] == 0    # no node in reach
    assert c["val"][-2] == TH and (hess[-2] == 0).all()
    hb = fld.hess_bound(ref)
    err = np.abs(hess.astype(np.float64) - ref["H"])
    zero = fin[:, None] & (hb == 0)
    assert (err[zero] == 0).all()
    sel = fin[:, None] & (hb > 0)
    frac = err[sel] / hb[sel]
    capped = ref["capped"]
    print(f"FIELD_HESS thr {thr:g}: {len(c['pts'])} points, cap binds at {100 * capped.mean():.1f} %, ties at the cap "
          f"{int((capped & ref['tie']).sum())}, largest fraction of hess_bound {frac.max():.3f}")
    assert (frac <= 1.0).all(), (int((frac > 1.0).sum()), float(frac.max()))
    sure = fin & (ref["slack"] == 0)
    assert np.array_equal(np.abs(c["taps"][sure]), ref["m"][sure]) and np.array_equal(c["taps"][sure] < 0, capped[sure])
    if thr >= 1e-3:
        assert not capped.any()
    if thr <= 1e-5:   # the ranking path is exercised (and, above, reported by taps < 0 exactly where the restatement caps)
        assert capped[:1700].any() and capped[-725:-5].any() and (capped & ref["tie"]).any()


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_curvature_follows_its_own_inputs(pkg, thr):
    """c = curvature(g32, H32) of the library's returned gradient and Hessian:
        |mean  - c.mean | <= 2^-23 |mean|  + 2^-44 |H|_F / |g|
        |gauss - c.gauss| <= 2^-23 |gauss| + 2^-44 |H|_F^2 / g2
        |k     - c.k    | <= 2^-23 |k|     + 2^-20 |H|_F / |g|        (k1 and k2)
    one Float32 rounding + the Float64 round-off of the cancelling numerators; the square root of the discriminant
    amplifies that round-off near umbilic points (sqrt(2^-44) = 2^-22 of |H|_F / |g|, with the count of operations on top),
    hence the third.  Also k1 >= k2, k1 + k2 = 2 mean to 2^-22 max(|k1|, |k2|), NaN exactly where g2 is 0 or not finite."""
    c = _case(pkg, thr)
    curv = c["curv"].astype(np.float64)
    r = FH.curvature(c["grad"], c["hess"])
    g2 = r["g2"]
    defined = (g2 > 0) & np.isfinite(g2)
    assert np.array_equal(np.isnan(curv).all(1), ~defined) and np.array_equal(np.isnan(curv).any(1), ~defined)
    assert int((~defined).sum()) >= 5                                                  # the special rows at least
    d = defined
    gn, hn = np.sqrt(g2[d]), r["hnorm"][d]
    mean, gauss, k1, k2 = curv[d].T
    bm = 2.0 ** -23 * np.abs(mean) + 2.0 ** -44 * hn / gn
    bg = 2.0 ** -23 * np.abs(gauss) + 2.0 ** -44 * hn * hn / g2[d]
    bk1 = 2.0 ** -23 * np.abs(k1) + 2.0 ** -20 * hn / gn
    bk2 = 2.0 ** -23 * np.abs(k2) + 2.0 ** -20 * hn / gn
    fr = [np.abs(mean - r["mean"][d]) / bm, np.abs(gauss - r["gauss"][d]) / bg, np.abs(k1 - r["k1"][d]) / bk1,
          np.abs(k2 - r["k2"][d]) / bk2]
    print(f"FIELD_CURV thr {thr:g}: {int(d.sum())} defined of {len(curv)}; largest fractions of the bounds: mean {fr[0].max():.3f}, "
          f"gauss {fr[1].max():.3f}, k1 {fr[2].max():.3f}, k2 {fr[3].max():.3f}")
    for name, f in zip(("mean", "gauss", "k1", "k2"), fr):
        assert (f <= 1.0).all(), (name, int((f > 1.0).sum()), float(f.max()))
    assert (k1 >= k2).all()
    assert (np.abs(k1 + k2 - 2.0 * mean) <= 2.0 ** -22 * np.maximum(np.abs(k1), np.abs(k2))).all()


def test_known_answer_single_node(pkg):
    """one non-zero weight, threshold 1e-3, 64 points on a sphere of 0.7 cell around the node: mean r = gauss r^2 = k1 r =
    k2 r = 1 (r = |d| of the Float32 differences).  Allowed: the first-order propagation of grad_bound and hess_bound through
    the formulas - sum_i |dQ/dx_i| bound_i over the 9 inputs, the partial derivatives by central differences of the
    restatement's curvature64 - doubled for the second-order term, plus the Float32 rounding of the result.  mean and gauss
    are smooth in the inputs.  k = mean +- sqrt(disc) is not at an umbilic point (disc = 0): there
    |dk| <= |dmean| + sqrt(|ddisc|) with |ddisc| <= 2 |mean| |dmean| + |dgauss| + |dmean|^2, which is what is allowed."""
    g = _grid(pkg)
    w = np.zeros((DIMS[2], DIMS[1], DIMS[0]), np.float32)
    node = (3, 4, 5)
    w[node] = np.float32(0.83)
    fld = _ref_field(g, w, 1e-3, TH)
    cen = np.array([fld.axes[0][node[2]], fld.axes[1][node[1]], fld.axes[2][node[0]]], np.float32)
    rng = np.random.default_rng(50)
    v = rng.standard_normal((64, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    p = (cen.astype(np.float64) + 0.7 * H * v).astype(np.float32)
    r = np.linalg.norm((p - cen).astype(np.float64), axis=1)
    ref = fld.hessian(p)
    x = np.hstack([ref["grad"], ref["H"]])                                             # (64, 9)
    bx = np.hstack([fld.grad_bound(ref), fld.hess_bound(ref)])
    c0 = FH.curvature64(x[:, :3], x[:, 3:])
    dm, dg = np.zeros(64), np.zeros(64)
    for i in range(9):
        e = np.zeros_like(x)
        e[:, i] = 1e-6 * np.maximum(np.abs(x[:, i]), np.abs(x).max(1) * 1e-3)
        hi, lo = FH.curvature64((x + e)[:, :3], (x + e)[:, 3:]), FH.curvature64((x - e)[:, :3], (x - e)[:, 3:])
        dm += np.abs(hi["mean"] - lo["mean"]) / (2.0 * e[:, i]) * bx[:, i]
        dg += np.abs(hi["gauss"] - lo["gauss"]) / (2.0 * e[:, i]) * bx[:, i]
    dm, dg = 2.0 * dm, 2.0 * dg
    dk = dm + np.sqrt(2.0 / r * dm + dg + dm * dm)
    am = dm * r + 2.0 ** -23
    ag = dg * r * r + 2.0 ** -23
    ak = dk * r + 2.0 ** -23
    # the restatement alone first
    assert (np.abs(c0["mean"] * r - 1.0) <= am).all() and (np.abs(c0["gauss"] * r * r - 1.0) <= ag).all()
    assert (np.abs(c0["k1"] * r - 1.0) <= ak).all() and (np.abs(c0["k2"] * r - 1.0) <= ak).all()
    assert am.max() < 1e-4 and ak.max() < 2e-2                                         # the comparison means something
    with pkg.RbfField(w, g, TH, 1e-3, device=0) as f:
        mean, gauss, k1, k2 = (a.astype(np.float64) for a in f.curvature(p))
    fr = [np.abs(mean * r - 1.0) / am, np.abs(gauss * r * r - 1.0) / ag, np.abs(k1 * r - 1.0) / ak, np.abs(k2 * r - 1.0) / ak]
    print(f"FIELD_CURV single node: largest fractions of the propagated bound: mean {fr[0].max():.3f}, gauss {fr[1].max():.3f}, "
          f"k1 {fr[2].max():.3f}, k2 {fr[3].max():.3f} (allowed: mean {am.max():.2e}, k {ak.max():.2e} relative)")
    for f_ in fr:
        assert (f_ <= 1.0).all(), float(f_.max())


def test_host_and_device_variants_order_and_guards(pkg):
    """_dev = host bit for bit; a permutation of the points permutes the bits; n = 1 and n = 17 write nothing beyond n"""
    import torch
    lib = pkg._lib.lib()
    torch.cuda.set_device(0)
    for thr in (1e-3, 1e-9):
        c = _case(pkg, thr)
        pts = c["pts"]
        with pkg.RbfField(c["w"], c["g"], TH, thr, device=0) as f:
            t = torch.tensor(pts, device="cuda:0")
            dv, dg, dh, dt = f.hessian_dev(t, taps=True)
            dc = f.curvature_dev(t)
            torch.cuda.synchronize()
            for a, b in ((c["val"], dv), (c["grad"], dg), (c["hess"], dh), (c["curv"], dc)):
                assert np.array_equal(_bits(a), _bits(b.cpu().numpy()))
            assert np.array_equal(c["taps"], dt.cpu().numpy())
            rng = np.random.default_rng(4)
            perm = rng.permutation(len(pts))
            inv = np.argsort(perm)
            q = np.ascontiguousarray(pts[perm])
            v2, g2, h2, t2 = f.eval(q, grad=True, hess=True, taps=True)
            assert np.array_equal(_bits(v2[inv]), _bits(c["val"])) and np.array_equal(_bits(g2[inv]), _bits(c["grad"]))
            assert np.array_equal(_bits(h2[inv]), _bits(c["hess"])) and np.array_equal(t2[inv], c["taps"])
            assert np.array_equal(_bits(np.stack(f.curvature(q), axis=1)[inv]), _bits(c["curv"]))
            # gradient and Hessian handed out by the curvature call are the Hessian call's
            n = len(pts)
            cg, ch, cc = np.empty((n, 3), np.float32), np.empty((n, 6), np.float32), np.empty((n, 4), np.float32)
            fp = lambda a: a.ctypes.data_as(pkg._lib.c_float_p)   # noqa: E731
            pkg._lib.check(lib.r2s_rbf_field_curvature(f._handle(), fp(pts), n, fp(cc), fp(cg), fp(ch)))
            assert np.array_equal(_bits(cg), _bits(c["grad"])) and np.array_equal(_bits(ch), _bits(c["hess"]))
            assert np.array_equal(_bits(cc), _bits(c["curv"]))
            assert f.eval(np.zeros((0, 3), np.float32), hess=True)[2].shape == (0, 6) and f.curvature_dev(t[:0]).shape == (0, 4)
            # guard words behind n results
            GUARD = 0x5A5A5A5A
            for n in (1, 17):
                bufs = {k: torch.full((n * m + 64,), GUARD, dtype=torch.int32, device="cuda:0") for k, m in
                        (("val", 1), ("grad", 3), ("hess", 6), ("taps", 1), ("curv", 4), ("cgrad", 3), ("chess", 6))}
                ptr = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
                tp = t[:n].contiguous()
                pkg._lib.check(lib.r2s_rbf_field_hessian_dev(f._handle(), ptr(tp), n, ptr(bufs["val"]), ptr(bufs["grad"]), ptr(bufs["hess"]),
                                                             ptr(bufs["taps"]), None))
                pkg._lib.check(lib.r2s_rbf_field_curvature_dev(f._handle(), ptr(tp), n, ptr(bufs["curv"]), ptr(bufs["cgrad"]),
                                                               ptr(bufs["chess"]), None))
                torch.cuda.synchronize()
                for k, m in (("val", 1), ("grad", 3), ("hess", 6), ("taps", 1), ("curv", 4), ("cgrad", 3), ("chess", 6)):
                    b = bufs[k].cpu().numpy()
                    assert (b[n * m:] == GUARD).all(), (k, n)
                assert np.array_equal(bufs["hess"].cpu().numpy()[:6 * n].view(np.uint32), _bits(c["hess"][:n]).ravel())
                assert np.array_equal(bufs["curv"].cpu().numpy()[:4 * n].view(np.uint32), _bits(c["curv"][:n]).ravel())
                assert np.array_equal(bufs["taps"].cpu().numpy()[:n], c["taps"][:n])
            assert lib.r2s_rbf_field_curvature_dev(f._handle(), ptr(tp), 1, None, None, None, None) == -1   # curv is required


def test_surface_curvature_end_to_end(pkg):
    """fit on the sphere fixture, extract, refine; on the vertices that reached the level (status 0, all others are the
    < 3 % of tests/test_field_gpu.py): positive median mean curvature, no undefined vertex, and the median of min_radius
    inside the spread - the 25 % to 75 % quantiles - of the min_radius the float64 restatement gives on those vertices"""
    X, IEN, rho = load_fixture("sphere")
    mesh = pkg.Mesh(X, IEN)
    grid = pkg.Grid(X.min(0), X.max(0), 14, 3)
    sdf = pkg.sdf_fused(mesh, grid, pkg.DenseInNodes(mesh, rho, device=0), 0.5, device=0)
    vd, vf = pkg.calculate_mesh_volume(mesh, rho, device=0)
    fine = pkg.RBFs_smoothing(sdf, grid, True, 2, vd * vf, 1e-3, device=0)
    verts, _ = pkg.extract_isosurface(fine, grid, 2, device=0)
    with pkg.fit_rbf_field(sdf, grid, True, vd * vf, 1e-3, device=0) as f:
        w, th = f.weights, f.level_shift
        p, _, status = pkg.refine_surface(f, verts)
        on = status == 0
        assert on.mean() > 0.97
        out = pkg.surface_curvature(f, p[on])
    assert set(out) == {"mean", "gauss", "k1", "k2", "min_radius", "n_undefined", "min_radius_p01", "min_radius_p50"}
    assert out["n_undefined"] == 0 and np.isfinite(out["min_radius"]).all()
    assert np.median(out["mean"]) > 0
    fld = _ref_field(grid, w, 1e-3, th)
    ref = fld.hessian(p[on])
    rc = FH.curvature64(ref["grad"], ref["H"])
    rad = 1.0 / np.maximum(np.abs(rc["k1"]), np.abs(rc["k2"]))
    lo, hi = np.quantile(rad, [0.25, 0.75])
    med = float(np.median(out["min_radius"]))
    print(f"surface_curvature: {int(on.sum())} of {len(on)} vertices; median mean curvature {np.median(out['mean']):.4f}, min_radius median "
          f"{med:.4f} (restatement: median {np.median(rad):.4f}, quartiles {lo:.4f} .. {hi:.4f}), p01 {out['min_radius_p01']:.4f}; "
          f"sphere radius {0.5 * float((X.max(0) - X.min(0)).max()):.3f}")
    assert lo <= med <= hi
    assert out["min_radius_p50"] == med and out["min_radius_p01"] <= med
    assert np.array_equal(out["min_radius"], 1.0 / np.maximum(np.abs(out["k1"]), np.abs(out["k2"])).astype(np.float64))
