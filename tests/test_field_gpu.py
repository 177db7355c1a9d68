"""The point evaluator of the smoothed level-set on the GPU against its float64 restatement (field_ref64).

Every comparison is against field_ref64, which shares no code with the library.  Bounds (Field.value_bound / grad_bound):

    |val  - ref.val |     <= (m + 6 ln(1/thr) + 8) 2^-24 S   + 2^-23 (|ref.val| + |th|) + slack
    |grad_a - ref.grad_a| <= (6 ln(1/thr) + 12)   2^-24 S_a + 2^-23 |ref.grad_a|       + slack 2 R / sigma

No point is left out.  Where the knn cap binds and the 124th / 125th distances are equal the reference's own result is not
unique; the library documents the (distance, linear node index) rule and the restatement follows it, so those points
(most lattice points at 1e-5, hardly any random point) are compared too, against that rule; their number is printed.
Each test prints the largest fraction of its bound that it observed.

Projection (test_projection_follows_the_restatement): the restatement runs the header's step rule from the same start
with its own Float32 values; its figures (vertices on the level, steps, distance moved, border vertices) are written into
PROJECTION_REF and asserted.  Two correct evaluators may stop one step apart where some |f| of the trajectory lies within
the value bound of tol ("border" vertices; their number is one of the asserted figures).  Every other vertex must have the
restatement's status, step count and end point.  A border vertex must be at most one step apart, with a status such a
stop can give, and its end point must lie on the restatement's trajectory at the kernel's step count.  Every status-0
vertex must satisfy |ref.val(p)| <= tol + value bound at the point the KERNEL returned.
Distance allowed between the end points: the sum over the steps of the one-step bound.  One step p - f g / |g|^2 changes by
at most |df| / |g| + 3 |f| |dg| / |g|^2 for evaluation differences df, dg within the value / gradient bounds, plus one
Float32 rounding of p.  A position difference e that enters a step is not amplified to first order: its component along g
changes f by g.e, which the step takes out again, and its tangential part is carried over (the change of direction
contributes |f| |H| |e| / |g|^2, second order next to e where |f| <= tol-sized or the step is the first).  The test asserts
the restatement's largest allowed distance as one of its own figures (2.7e-3 / 1.8e-2 cell) and a median below 1e-3 cell,
so the comparison cannot become empty.
"""
import ctypes
import math

import numpy as np
import pytest

import field_ref64 as F
import rbf_ref64 as R64
from conftest import load_fixture

pytestmark = pytest.mark.gpu

LO, H = np.array([0.013, -0.2, 0.07]), 0.1037
THRESHOLDS = (0.1, 1e-2, 1e-3, 1e-4, 1e-5)


def _grid(pkg, dims):
    dims = np.array(dims)
    g = pkg.Grid(LO, LO + H * (dims - 1.0), int(dims.max()) - 1, 0)
    assert g.dims == tuple(int(d) for d in dims)
    return g


def _ref_field(g, w, thr, th):
    return F.Field(w, np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N], float(g.c.cell_size), thr, th)


def _lattice_points(axes):
    tx, ty, tz = axes
    Z, Y, X = np.meshgrid(tz, ty, tx, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1).astype(np.float32)


def _random_points(g, rng, n_in, n_out):
    amin, amax = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:])
    h = float(g.c.cell_size)
    inside = amin + rng.random((n_in, 3)) * (amax - amin)
    wide = amin - 3.0 * h + rng.random((4 * n_out, 3)) * (amax - amin + 6.0 * h)
    wide = wide[((wide < amin) | (wide > amax)).any(1)][:n_out]
    return np.vstack([inside, wide]).astype(np.float32)


def _compare(fld, ref, val, grad, taps, label, check_taps=True):
    """-> largest fraction of the bounds; asserts every point"""
    fin = np.isfinite(ref["val"])
    ok = fin
    assert np.isnan(val[~fin]).all() and (grad is None or np.isnan(grad[~fin]).all())
    vb = fld.value_bound(ref)
    err = np.abs(val.astype(np.float64) - ref["val"])
    assert (err[ok] <= vb[ok]).all(), (label, "value", int((err[ok] > vb[ok]).sum()), float((err[ok] / np.maximum(vb[ok], 1e-300)).max()))
    worst = float((err[ok] / np.maximum(vb[ok], 1e-300)).max()) if ok.any() else 0.0
    if grad is not None:
        gb = fld.grad_bound(ref)
        gerr = np.abs(grad.astype(np.float64) - ref["grad"])
        zero = ok[:, None] & (gb == 0)
        assert (gerr[zero] == 0).all(), (label, "gradient where the bound is 0")
        sel = ok[:, None] & (gb > 0)
        assert (gerr[sel] <= gb[sel]).all(), (label, "gradient", int((gerr[sel] > gb[sel]).sum()), float((gerr[sel] / gb[sel]).max()))
        worst = max(worst, float((gerr[sel] / gb[sel]).max()) if sel.any() else 0.0)
    if taps is not None:
        assert (taps[~fin] == 0).all()
        if check_taps:
            sure = fin & (ref["slack"] == 0)          # (a node at the very edge of the support may count either way)
            assert np.array_equal(np.abs(taps[sure]), ref["m"][sure]), label
            assert np.array_equal(taps[sure] < 0, ref["capped"][sure]), label
    return worst


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_from_weights_against_the_restatement(pkg, thr):
    """random weights on the non-dyadic lattice: 20 000 points inside the box, 2 000 within three cells outside it, the
    lattice points themselves, NaN / inf rows, a far point; value, gradient and taps"""
    g = _grid(pkg, (20, 17, 22))
    rng = np.random.default_rng(int(-math.log10(thr)) + 11)
    nx, ny, nz = g.dims
    w = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    th = np.float32(0.3712)
    amin, amax, N = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:]), [int(n) for n in g.c.N]
    special = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [1e30, 0.0, 0.0], [amax[0] + 40 * H, 0.5, 0.5]], np.float32)
    pts = np.vstack([_random_points(g, rng, 20000, 2000), _lattice_points(R64.coarse_axes(amin, amax, N)), special])
    fld = _ref_field(g, w, thr, th)
    ref = fld.evaluate(pts)
    with pkg.RbfField(w, g, th, thr, device=0) as f:
        val, grad, taps = f.eval(pts, grad=True, taps=True)
        only = f.eval(pts)
        assert np.array_equal(f.weights, w) and f.level_shift == th
    assert np.array_equal(val.view(np.uint32), only.view(np.uint32))                   # value-only launch: the same numbers
    worst = _compare(fld, ref, val, grad, taps, f"thr {thr}")
    assert val[-1] == th and (grad[-1] == 0).all() and taps[-1] == 0                   # no node in reach
    assert val[-2] == th and (grad[-2] == 0).all()
    capped = float(ref["capped"].mean())
    print(f"thr {thr}: {len(pts)} points, cap binds at {100 * capped:.2f} %, ties at the cap (compared by the index rule) {int((ref['capped'] & ref['tie']).sum())}, "
          f"largest fraction of the bound {worst:.3f}")
    if thr >= 1e-3:
        assert capped == 0.0
    if thr == 1e-5:
        assert ref["capped"][:20000].mean() > 0.5                                      # the slow path is exercised


def _mesh_case(pkg, name, nmax):
    X, IEN, rho = load_fixture(name)
    mesh = pkg.Mesh(X, IEN)
    grid = pkg.Grid(X.min(0), X.max(0), nmax, 3)
    rho_n = pkg.DenseInNodes(mesh, rho, device=0)
    sdf = pkg.sdf_fused(mesh, grid, rho_n, 0.5, device=0)
    Vd, Vf = pkg.calculate_mesh_volume(mesh, rho, device=0)
    return X, grid, sdf, Vd * Vf


def test_fit_is_the_smoothing_stage(pkg):
    """fit on the sphere fixture: the level shift and CG count of r2s_rbf_smooth bit for bit, a from_weights round trip, and
    eval at the smooth = 2 lattice against the stage's own output within the sum of both bounds"""
    X, grid, sdf, target = _mesh_case(pkg, "sphere", 14)
    info = {}
    fine = pkg.RBFs_smoothing(sdf, grid, True, 2, target, 1e-3, device=0, info=info)
    amin, amax, N = np.array(grid.c.aabb_min[:]), np.array(grid.c.aabb_max[:]), [int(n) for n in grid.c.N]
    pts = _lattice_points(R64.fine_axes(amin, amax, N, 2))
    with pkg.fit_rbf_field(sdf, grid, True, target, 1e-3, device=0) as f:
        assert np.float32(info["th"]) == f.level_shift and info["cg_iterations"] == f.cg_iterations and f.cg_iterations > 0
        w, th = f.weights, f.level_shift
        val, grad = f.eval(pts, grad=True)
        pkg._lib.lib().r2s_release_cache()                                            # live fields survive it
        again = f.eval(pts)
        with pkg.RbfField(w, grid, th, 1e-3, device=0) as f2:
            assert np.array_equal(f2.weights.view(np.uint32), w.view(np.uint32)) and f2.level_shift == th
            v2, g2 = f2.eval(pts, grad=True)
    assert np.array_equal(val.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(val.view(np.uint32), v2.view(np.uint32)) and np.array_equal(grad.view(np.uint32), g2.view(np.uint32))
    fld = _ref_field(grid, w, 1e-3, th)
    ref = fld.evaluate(pts)
    worst = _compare(fld, ref, val, grad, None, "sphere fit")
    # the stage's own bound (rbf_ref64.fine_bound) from the same taps
    stage = ((ref["m"] + 6.0 * math.log(1e3) + 8.0) * 2.0 ** -24 * ref["S"]
             + 2.0 ** -23 * (np.abs(ref["val"] - float(th)) + abs(float(th))))
    both = fld.value_bound(ref) + stage
    err = np.abs(val.astype(np.float64) - fine.ravel().astype(np.float64))
    assert (err <= both).all(), (int((err > both).sum()), float((err / both).max()))
    print(f"sphere fit: th {float(th):.6g}, {f.cg_iterations} CG steps; eval vs restatement {worst:.3f} of the bound, "
          f"eval vs the stage's fine field {float((err / both).max()):.3f} of both bounds")


def test_host_and_device_variants_and_point_order(pkg):
    """host and _dev entry points give the same bits; a permutation of the points permutes the results"""
    import torch
    g = _grid(pkg, (20, 17, 22))
    rng = np.random.default_rng(3)
    nx, ny, nz = g.dims
    w = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    pts = _random_points(g, rng, 30000, 3000)
    pts[17] = np.nan
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)   # noqa: E731
    for thr in (1e-3, 1e-5):
        with pkg.RbfField(w, g, -0.11, thr, device=0) as f:
            torch.cuda.set_device(0)
            val, grad, taps = f.eval(pts, grad=True, taps=True)
            nrm = f.normals(pts)
            tol = np.float32(1e-3)
            pp, st, rs, its = f.project(pts, 6, tol)
            t = torch.tensor(pts, device="cuda:0")
            dv, dg, dt = f.eval_dev(t, grad=True, taps=True)
            dn = f.normals_dev(t)
            dp, ds, dr, di = f.project_dev(t, 6, tol)
            torch.cuda.synchronize()
            assert np.array_equal(bits(t.cpu().numpy()), bits(pts))                        # project_dev works on a copy
            for a, b in ((val, dv), (grad, dg), (nrm, dn), (pp, dp), (rs, dr)):
                assert np.array_equal(bits(a), bits(b.cpu().numpy()))
            assert np.array_equal(taps, dt.cpu().numpy()) and np.array_equal(st, ds.cpu().numpy()) and np.array_equal(its, di.cpu().numpy())
            perm = rng.permutation(len(pts))
            inv = np.argsort(perm)
            q = np.ascontiguousarray(pts[perm])
            v2, g2, t2 = f.eval(q, grad=True, taps=True)
            assert np.array_equal(bits(v2[inv]), bits(val)) and np.array_equal(bits(g2[inv]), bits(grad)) and np.array_equal(t2[inv], taps)
            assert np.array_equal(bits(f.normals(q)[inv]), bits(nrm))
            p3, s3, r3, i3 = f.project(q, 6, tol)
            assert np.array_equal(bits(p3[inv]), bits(pp)) and np.array_equal(s3[inv], st) and np.array_equal(i3[inv], its)
            assert np.array_equal(bits(r3[inv]), bits(rs))
            # n = 0 touches nothing; a shorter array (another launch shape) gives the same leading results
            assert f.eval(np.zeros((0, 3), np.float32)).shape == (0,)
            assert np.array_equal(bits(f.eval(pts[:1001])), bits(val[:1001]))
            assert st[17] == 3 and its[17] == 0 and np.isnan(rs[17]) and (nrm[17] == 0).all()


def test_normals(pkg):
    """unit length to 2^-22 where defined; equal to -ref.grad / |ref.grad| within the gradient bound through the
    normalisation: |dn| <= 2 |dg| / |g| (first order: |dg| / |g|; doubled for the second order) + 2^-22 of rounding"""
    g = _grid(pkg, (20, 17, 22))
    rng = np.random.default_rng(9)
    nx, ny, nz = g.dims
    w = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    pts = _random_points(g, rng, 20000, 2000)
    fld = _ref_field(g, w, 1e-3, 0.2)
    ref = fld.evaluate(pts)
    with pkg.RbfField(w, g, 0.2, 1e-3, device=0) as f:
        nrm = f.normals(pts)
        grad = f.eval(pts, grad=True)[1]
    assert np.array_equal(nrm.view(np.uint32), fld.normals(grad).view(np.uint32))        # the header's rule on the kernel's own gradient
    ln = np.sqrt((nrm.astype(np.float64) ** 2).sum(1))
    defined = ln > 0
    assert np.abs(ln[defined] - 1.0).max() <= 2.0 ** -22
    gn = np.sqrt((ref["grad"] ** 2).sum(1))
    gb = np.sqrt((fld.grad_bound(ref) ** 2).sum(1)) + 2.0 ** -23 * gn
    sel = defined & (gn > 0)
    want = -ref["grad"][sel] / gn[sel][:, None]
    nb = 2.0 * gb[sel] / gn[sel] + 2.0 ** -22
    err = np.sqrt(((nrm[sel].astype(np.float64) - want) ** 2).sum(1))
    assert (err <= nb).all(), (int((err > nb).sum()), float((err / nb).max()))
    assert ((gn[~defined] <= gb[~defined])).all()                                     # undefined only where the gradient vanishes
    print(f"normals: {int(defined.sum())} of {len(pts)} defined, largest fraction of the bound {float((err / nb).max()):.3f}")


# The restatement's own numbers for the projection of the extracted smooth = 2 surface (max_iter = 8, tol = 1e-4
# cell_size), taken from field_ref64.Field.project on the weights of the fit: vertices, vertices that reach the level
# (status 0) / hit the iteration cap (1) / meet a vanishing gradient (2), steps in total and at most, border vertices,
# distance moved in fine cells (median, max), and the largest end-point distance the restatement's bounds allow along any
# trajectory (the measured 2.61e-3 / 1.77e-2 cells, rounded up; the large ones belong to vertices that pass places where |g|
# is small, which the one-step bound has in its denominator).  Deterministic numpy on deterministic weights: asserted.
PROJECTION_REF = {
    "sphere": dict(nmax=14, verts=3072, status0=2988, status1=84, status2=0, steps=3852, max_steps=8, border=42,
                   moved_median=0.005784591535551172, moved_max=0.0939988943108061, allowed_max_cells=2.7e-3),
    "chapadlo": dict(nmax=30, verts=6500, status0=6383, status1=117, status2=0, steps=11084, max_steps=8, border=263,
                     moved_median=0.027160078044332726, moved_max=0.7690009701313234, allowed_max_cells=1.8e-2),
}


def _projection_case(pkg, name):
    X, grid, sdf, target = _mesh_case(pkg, name, PROJECTION_REF[name]["nmax"])
    h = float(grid.c.cell_size)
    tol = np.float32(1e-4 * h)
    fine = pkg.RBFs_smoothing(sdf, grid, True, 2, target, 1e-3, device=0)
    verts, tris = pkg.extract_isosurface(fine, grid, 2, device=0)
    with pkg.fit_rbf_field(sdf, grid, True, target, 1e-3, device=0) as f:
        w, th = f.weights, f.level_shift
        out = f.project(verts, 8, tol)
        refined = pkg.refine_surface(f, verts)
        nrm = f.normals(out[0])
    fld = _ref_field(grid, w, 1e-3, th)
    ref = fld.project(verts, 8, tol)
    moved = np.sqrt(((ref["points"].astype(np.float64) - verts.astype(np.float64)) ** 2).sum(1)) / (h / 2.0)
    got = dict(verts=len(verts), status0=int((ref["status"] == 0).sum()), status1=int((ref["status"] == 1).sum()),
               status2=int((ref["status"] == 2).sum()), steps=int(ref["iters"].sum()), max_steps=int(ref["iters"].max()),
               border=int(ref["border"].sum()), moved_median=float(np.median(moved)), moved_max=float(moved.max()))
    return X, grid, h, tol, verts, out, refined, nrm, fld, ref, got


@pytest.mark.parametrize("name", ["sphere", "chapadlo"])
def test_projection_follows_the_restatement(pkg, name):
    """vertices of extract_isosurface on the smooth = 2 field, projected with max_iter = 8, tol = 1e-4 cell_size: the
    restatement's figures equal PROJECTION_REF, and the kernel follows the restatement vertex by vertex (module docstring)"""
    X, grid, h, tol, verts, (p, status, resid, iters), (rp, rn, rs), nrm, fld, ref, got = _projection_case(pkg, name)
    print(f"{name}: restatement {got}")
    want = {k: v for k, v in PROJECTION_REF[name].items() if k != "nmax"}
    for k in ("verts", "status0", "status1", "status2", "steps", "max_steps", "border"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["moved_median"] == pytest.approx(want["moved_median"], rel=1e-6)
    assert got["moved_max"] == pytest.approx(want["moved_max"], rel=1e-6)
    assert np.array_equal(rp.view(np.uint32), p.view(np.uint32)) and np.array_equal(rs, status)
    assert np.array_equal(rn.view(np.uint32), nrm.view(np.uint32))
    n = len(verts)
    idx = np.arange(n)
    border = ref["border"]
    plain = ~border
    # every vertex that is not a border case: the restatement's status, step count and end point
    assert np.array_equal(status[plain], ref["status"][plain]), int((status[plain] != ref["status"][plain]).sum())
    assert np.array_equal(iters[plain], ref["iters"][plain]), int((iters[plain] != ref["iters"][plain]).sum())
    assert int((status[plain] == 0).sum()) == int((ref["status"][plain] == 0).sum())
    # border vertices: one step apart at most, a status that such a stop can give, and the end point on the restatement's
    # trajectory (which reaches one step beyond its own stop) at the kernel's step count
    di = iters.astype(np.int64) - ref["iters"]
    assert (np.abs(di[border]) <= 1).all(), int((np.abs(di[border]) > 1).sum())
    same = border & (di == 0)
    # (same step count: the same status, or 0 against 1 at the iteration cap, where the last |f| decides)
    assert ((status[same] == ref["status"][same])
            | ((iters[same] == 8) & np.isin(status[same], (0, 1)) & np.isin(ref["status"][same], (0, 1)))).all()
    early, late = border & (di == -1), border & (di == 1)
    assert (status[early] == 0).all()                                   # stopped where the restatement went on: only by |f| <= tol
    assert (ref["status"][late] == 0).all()                             # went on where the restatement stopped by |f| <= tol
    assert ((status[late] == 0) | ((status[late] == 1) & (iters[late] == 8))).all()
    k = np.clip(iters, 0, 9)
    assert ref["trail_ok"][k, idx].all()
    end = ref["trail"][k, idx].astype(np.float64)
    dist = np.sqrt(((p.astype(np.float64) - end) ** 2).sum(1))
    allowed = ref["trail_err"][k, idx] + 2.0 ** -22 * np.abs(end).max(1)
    # the comparison means something: the allowed distance is the restatement's own figure, far below a cell, and below
    # 1e-3 cell for most vertices
    assert float(ref["trail_err"].max() / h) <= want["allowed_max_cells"] and allowed.max() / h <= 1.01 * want["allowed_max_cells"]
    assert np.median(allowed) <= 1e-3 * h, float(np.median(allowed) / h)
    assert (dist <= allowed).all(), (int((dist > allowed).sum()), float((dist / allowed).max()))
    # independently of the trajectory: the returned points lie on the zero level of the restatement
    at = fld.evaluate(p)
    conv = status == 0
    vb = fld.value_bound(at)
    assert (np.abs(at["val"][conv]) <= float(tol) + vb[conv]).all()
    assert (np.abs(resid[conv].astype(np.float64) - np.abs(at["val"][conv])) <= vb[conv]).all()
    # the kernel's count of vertices on the level: the restatement's, give or take the border vertices that differ
    differ = int((status[border] != ref["status"][border]).sum())
    assert abs(int(conv.sum()) - want["status0"]) <= differ <= want["border"]
    kmoved = np.sqrt(((p.astype(np.float64) - verts.astype(np.float64)) ** 2).sum(1)) / (h / 2.0)
    line = (f"{name}: kernel status 0 for {int(conv.sum())} of {n} (restatement {want['status0']}), moved median {np.median(kmoved):.4f} "
            f"max {kmoved.max():.4f} fine cells; border vertices {want['border']}, of which {int((di != 0).sum())} a step apart and "
            f"{differ} with another status; end points within {float((dist / allowed).max()):.3f} of the allowed distance "
            f"(largest allowed {float(allowed.max() / h):.2e} cells)")
    if name == "sphere":
        # angle between the normals and the radial direction (reported: the smoothed surface is close to a sphere)
        rad = p.astype(np.float64) - 0.5 * (X.min(0) + X.max(0))
        rad /= np.linalg.norm(rad, axis=1)[:, None]
        ang = np.degrees(np.arccos(np.clip((nrm.astype(np.float64) * rad).sum(1), -1.0, 1.0)))
        line += f"; angle to radial median {np.median(ang):.2f} max {ang.max():.2f} deg"
        assert (np.linalg.norm(nrm, axis=1) > 0).all()
    print(line)


def test_production_sized_call(pkg):
    """2^22 points in one call, checked on a 1-in-64 sample"""
    g = _grid(pkg, (40, 37, 43))
    rng = np.random.default_rng(21)
    nx, ny, nz = g.dims
    w = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    n = 1 << 22
    amin, amax = np.array(g.c.aabb_min[:]), np.array(g.c.aabb_max[:])
    pts = (amin - H + rng.random((n, 3)) * (amax - amin + 2.0 * H)).astype(np.float32)
    with pkg.RbfField(w, g, 0.05, 1e-3, device=0) as f:
        val, grad, taps = f.eval(pts, grad=True, taps=True)
    sel = np.arange(37, n, 64)
    fld = _ref_field(g, w, 1e-3, 0.05)
    ref = fld.evaluate(pts[sel])
    worst = _compare(fld, ref, val[sel], grad[sel], taps[sel], "2^22 points")
    assert np.isfinite(val).all() and np.isfinite(grad).all() and (taps >= 0).all() and int(taps.max()) <= 124
    print(f"2^22 points: {len(sel)} checked, largest fraction of the bound {worst:.3f}")
