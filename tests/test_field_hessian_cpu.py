"""The yardstick of the Hessian / curvature evaluation, without a GPU: the float64 restatement field_hess_ref64 against
central differences of its own float64 gradient, against 50-digit mpmath and against the curvature of a sphere (the level sets of a
single Gaussian), and the argument errors of the r2s_rbf_field_hessian / _curvature entry points."""
import ctypes
import os

import numpy as np
import pytest

import field_hess_ref64 as FH
import field_ref64 as F
from conftest import ROOT

LO, H = np.array([0.013, -0.2, 0.07]), 0.1037   # the non-dyadic lattice of the RBF tests
DIMS = (10, 9, 8)                                  # nodes of a 9 x 8 x 7-cell lattice


def _field(w, thr, th=0.0, dims=DIMS):
    dims = np.array(dims)
    return FH.HessField(w, LO, LO + H * (dims - 1.0), [int(d) - 1 for d in dims], H, thr, th)


def _weights(rng, dims=DIMS):
    return rng.standard_normal((dims[2], dims[1], dims[0])).astype(np.float32)


def test_hessian_is_the_derivative_of_the_gradient():
    """cutoff off: the restatement's Hessian against central differences of its own float64 gradient, step 1e-4 cell, 200
    random points of the 9 x 8 x 7-cell lattice with random weights, to 1e-6 max|H|.  (Step error h^2 f^(4) / 6 ~ 1e-8
    relative, round-off 2^-53 / 1e-4 ~ 1e-12.)  With the cutoff off the restatement works in float64 throughout
    (field_hess_ref64.hessian): a gradient whose distances are rounded to Float32 carries 2^-24-sized steps, which a
    difference over 2e-4 cell turns into ~1e-3 of the derivative.  The box of a point follows its cell and a node entering
    it adds exp(-B^2) ~ 1e-7: the random points are drawn at least 1e-3 cell inside their cells, so that the three
    evaluations of a difference sum the same nodes (as tests/test_field_cpu.py does for the gradient)."""
    rng = np.random.default_rng(31)
    fld = _field(_weights(rng), 1e-3, th=0.25)
    amin, amax = LO, LO + H * (np.array(DIMS) - 1.0)
    q = np.zeros((0, 3))
    while len(q) < 200:
        x = amin + rng.random((200, 3)) * (amax - amin)
        t = (x - amin) / H
        q = np.vstack([q, x[(np.abs(t - np.round(t)) > 1e-3).all(1)]])[:200]
    step = 1e-4 * H
    ref = fld.hessian(q, cutoff=False)
    assert (ref["m"] > 100).all() and np.isfinite(ref["H"]).all()
    num = np.zeros((200, 3, 3))
    for b in range(3):
        e = np.zeros(3)
        e[b] = step
        hi, lo = fld.hessian(q + e, cutoff=False), fld.hessian(q - e, cutoff=False)
        assert np.array_equal(hi["m"], ref["m"]) and np.array_equal(lo["m"], ref["m"])
        num[:, :, b] = (hi["grad"] - lo["grad"]) / (2.0 * step)
    tol = 1e-6 * np.abs(ref["H"]).max()
    worst = max(max(np.abs(num[:, a, b] - ref["H"][:, k]).max(), np.abs(num[:, b, a] - ref["H"][:, k]).max())
                for k, (a, b) in enumerate(FH.PAIRS))
    print(f"central differences: largest difference {worst:.3e}, allowed {tol:.3e}, max|H| {np.abs(ref['H']).max():.4g}")
    assert worst <= tol, (worst, tol)


def test_float32_steps_stay_within_their_rounding():
    """the same closed forms fed with Field._chunk's Float32 differences and distances (what cutoff=True uses) against the
    float64 ones on the same nodes, cutoff off so that no node is at an edge: k_j differs by <= 6 u^2 2^-24 relative with
    u^2 <= 3 (B + 2)^2 = 108 in this box, each Float32 difference d_a by 2^-24: (6 * 108 + 16) 2^-24 S_ab.  Value and
    gradient of the Float32 path are Field.evaluate's own, bit for bit."""
    rng = np.random.default_rng(35)
    fld = _field(_weights(rng), 1e-3, th=0.25)
    amin, amax = LO, LO + H * (np.array(DIMS) - 1.0)
    p = (amin - H + rng.random((300, 3)) * (amax - amin + 2.0 * H)).astype(np.float32)
    f64 = fld.hessian(p, cutoff=False)
    f32 = fld.hessian(p, cutoff=False, float64_steps=False)
    assert fld.B == 4 and np.array_equal(f64["m"], f32["m"])
    bound = (6.0 * 108.0 + 16.0) * 2.0 ** -24 * f64["Sab"]
    err = np.abs(f32["H"] - f64["H"])
    assert (err <= bound).all(), float((err / bound).max())
    assert (err > 0).any() and (bound < 1e-3 * np.abs(f64["H"]).max()).all()
    base = fld.evaluate(p, cutoff=False)
    assert np.array_equal(base["val"], f32["val"]) and np.array_equal(base["grad"], f32["grad"])
    on = fld.hessian(p)                                                                # cutoff on: Field.evaluate's too
    base = fld.evaluate(p)
    assert np.array_equal(base["val"], on["val"]) and np.array_equal(base["grad"], on["grad"]) and np.array_equal(base["m"], on["m"])


@pytest.mark.parametrize("thr", [1e-3, 1e-5])
def test_hessian_against_mpmath(thr):
    """the same sum over the same nodes in 50 digits: the float64 restatement is within 2^-48 S_ab (20 points; at 1e-5
    the cap binds on them).  mpmath repeats the sum, not the choice of nodes: it takes the nodes whose Float32 distance is
    among those the restatement counted (the m smallest by (distance, index)) and checks that count"""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(32)
    w = _weights(rng)
    fld = _field(w, thr, th=-0.1)
    amin, amax = LO, LO + H * (np.array(DIMS) - 1.0)
    p = (amin + rng.random((20, 3)) * (amax - amin)).astype(np.float32)
    ref = fld.hessian(p)
    assert (ref["capped"].any() and ref["capped"][0]) if thr == 1e-5 else not ref["capped"].any()
    ax = fld.axes
    sig = mp.mpf(fld.sigma)
    for i in range(len(p)):
        dx = (p[i, 0] - ax[0]).astype(np.float32)
        dy = (p[i, 1] - ax[1]).astype(np.float32)
        dz = (p[i, 2] - ax[2]).astype(np.float32)
        dist = np.sqrt((dx * dx)[None, None, :] + (dy * dy)[None, :, None] + (dz * dz)[:, None, None]).astype(np.float32)
        assert dist.dtype == np.float32
        order = np.argsort(dist.ravel(), kind="stable")
        inside = int((dist <= fld.maxd).sum())
        m = min(inside, F.KNN)
        assert m == ref["m"][i]
        Hm = [mp.mpf(0)] * 6
        for j in order[:m]:
            kz, ky, kx = np.unravel_index(j, dist.shape)
            d = (mp.mpf(float(dx[kx])), mp.mpf(float(dy[ky])), mp.mpf(float(dz[kz])))
            u = mp.mpf(float(dist[kz, ky, kx])) / sig
            wk = mp.mpf(float(w[kz, ky, kx])) * mp.exp(-(u * u))
            for k, (a, b) in enumerate(FH.PAIRS):
                Hm[k] += wk * (4 * d[a] * d[b] / sig ** 4 - (2 / sig ** 2 if a == b else 0))
        err = np.array([abs(float(mp.mpf(float(ref["H"][i, k])) - Hm[k])) for k in range(6)])
        assert (err <= 2.0 ** -48 * ref["Sab"][i]).all(), (i, err / ref["Sab"][i])


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_single_node_field_has_the_curvature_of_a_sphere(sign):
    """all weights 0 but one: the level sets are spheres around that node.  With g = -2 w k d / sigma^2 and
    H = w k (4 d d^T / sigma^4 - 2 I / sigma^2) the formulas give mean = 1 / |d|, gauss = 1 / |d|^2, k1 = k2 = 1 / |d| for
    w > 0 whatever k is, |d| being the norm of the Float32 differences the evaluation uses; w < 0 flips the normal: mean
    and k change sign, gauss does not.  50 points at 0.3 - 1.5 cells, 1e-9 relative."""
    rng = np.random.default_rng(33)
    w = np.zeros((DIMS[2], DIMS[1], DIMS[0]), np.float32)
    node = (3, 4, 5)                                                                   # (k, j, i)
    w[node] = np.float32(sign * 0.83)
    fld = _field(w, 1e-3, th=0.4)
    c = np.array([fld.axes[0][node[2]], fld.axes[1][node[1]], fld.axes[2][node[0]]], np.float32)
    v = rng.standard_normal((50, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    p = (c.astype(np.float64) + v * (rng.uniform(0.3, 1.5, 50) * H)[:, None]).astype(np.float32)
    r = np.linalg.norm((p - c).astype(np.float64), axis=1)                             # p - c in Float32, as evaluated
    assert (p - c).dtype == np.float32 and (r > 0.29 * H).all() and (r < 1.51 * H).all()
    ref = fld.hessian(p)
    assert (ref["m"] > 0).all()
    cv = FH.curvature64(ref["grad"], ref["H"])
    assert np.abs(cv["mean"] * r - sign).max() <= 1e-9
    assert np.abs(cv["gauss"] * r * r - 1.0).max() <= 1e-9
    # every point is umbilic: k1 = k2 needs the discriminant's numerator beyond float64 (field_hess_ref64.curvature64)
    assert np.abs(cv["k1"] * r - sign).max() <= 1e-9 and np.abs(cv["k2"] * r - sign).max() <= 1e-9
    assert (cv["k1"] >= cv["k2"]).all()
    # curvature() is the same on the Float32-rounded inputs, to their rounding
    c32 = FH.curvature(ref["grad"].astype(np.float32), ref["H"].astype(np.float32))
    assert np.abs(c32["mean"] * r - sign).max() <= 1e-5
    # undefined where the gradient vanishes or is not finite
    bad = FH.curvature(np.array([[0, 0, 0], [np.nan, 1, 1], [np.inf, 0, 0], [1, 0, 0]], np.float32), np.ones((4, 6), np.float32))
    assert np.isnan(bad["mean"][:3]).all() and np.isnan(bad["k1"][:3]).all() and np.isfinite(bad["mean"][3])


def test_restatement_special_points_and_bound():
    rng = np.random.default_rng(34)
    fld = _field(_weights(rng), 1e-3, th=-0.5)
    far = LO + H * (np.array(DIMS) + 50.0)
    p = np.vstack([[LO + 2.2 * H], [[np.nan, 0, 0]], [[0, np.inf, 0]], [far]]).astype(np.float32)
    r = fld.hessian(p)
    assert np.isfinite(r["H"][0]).all() and np.isnan(r["H"][1:3]).all()
    assert (r["H"][3] == 0).all() and r["val"][3] == -0.5 and r["m"][3] == 0
    b = fld.hess_bound(r)
    assert b.shape == (4, 6) and (b[0] > 0).all() and (b[0] < 1e-4 * np.abs(r["H"][0]).max()).all() and (b[3] == 0).all()
    assert FH.HESS_C <= 16


def test_argument_errors_before_any_device_work(pkg):
    """what r2s_rbf_field_eval / _normals answer to the same mistakes (tests/test_field_cpu.py)"""
    lib, L = pkg._lib.lib(), pkg._lib
    ARG = -1
    p = np.zeros((4, 3), np.float32)
    pp = p.ctypes.data_as(L.c_float_p)
    assert lib.r2s_rbf_field_eval(None, pp, 4, pp, None, None) == ARG
    assert lib.r2s_rbf_field_hessian(None, pp, 4, pp, None, None, None) == ARG
    assert lib.r2s_rbf_field_hessian(None, pp, 4, None, None, None, None) == ARG
    assert lib.r2s_rbf_field_hessian(None, None, 0, None, None, None, None) == ARG
    assert lib.r2s_rbf_field_hessian_dev(None, None, 0, None, None, None, None, None) == ARG
    assert lib.r2s_rbf_field_curvature(None, pp, 4, pp, None, None) == ARG
    assert lib.r2s_rbf_field_curvature(None, pp, 4, None, None, None) == ARG
    assert lib.r2s_rbf_field_curvature_dev(None, None, 4, None, None, None, None) == ARG


def test_bindings_match_the_header():
    """the four entry points in the header, the ctypes table and the Julia binding: same parameter counts; the _dev variant
    is the host variant + the stream"""
    import test_field_cpu as T
    names = ("r2s_rbf_field_hessian", "r2s_rbf_field_curvature")
    from importlib.util import module_from_spec, spec_from_file_location
    spec = spec_from_file_location("_r2s_lib_only_hess", os.path.join(ROOT, "rho2sdf.jl_amd", "_lib.py"))
    Lm = module_from_spec(spec)
    spec.loader.exec_module(Lm)
    table = {n: a for n, _, a in Lm.SYMBOLS}
    for name in names:
        assert T._c_params(name + "_dev") == T._c_params(name) + ["void *"]
        for nm in (name, name + "_dev"):
            c, calls = T._c_params(nm), T._julia_ccalls(nm)
            assert calls, f"{nm}: no ccall in the Julia binding"
            for types in calls:
                assert len(types) == len(c), (nm, types, c)
                for jt, ct in zip(types, c):
                    assert jt in T.C_TO_JULIA[ct], (nm, jt, ct)
            assert len(table[nm]) == len(c), nm


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_no_field(pkg):
    """without a device no field can be made, so the new entry points are reachable with a NULL field only: the same
    R2S_ERR_ARG as r2s_rbf_field_eval, and no crash"""
    lib, L = pkg._lib.lib(), pkg._lib
    p = np.zeros((2, 3), np.float32)
    pp = p.ctypes.data_as(L.c_float_p)
    out = np.zeros((2, 6), np.float32)
    op = out.ctypes.data_as(L.c_float_p)
    assert lib.r2s_rbf_field_eval(None, pp, 2, op, None, None) == lib.r2s_rbf_field_hessian(None, pp, 2, op, None, op, None) == -1
    assert lib.r2s_rbf_field_curvature(None, pp, 2, op, None, None) == -1
    with pytest.raises(L.R2SError, match="no HIP device|CPU fallback"):
        pkg.RbfField(np.ones(125, np.float32), pkg.Grid(LO, LO + H * 4.0, 4, 0))
