"""No GPU: pins the float64 restatement of the mesh distance (tests/mesh_dist_ref64.py) that tests/test_redistance_gpu.py
compares the kernels with - against the closed-form distance to a box, against mpmath at 50 digits on a hand-made set of
awkward triangles (this is where the bound constant K is measured), and its block-culled lattice form against the plain
brute force.  Also the CPU side of the binding: refusals that need no device, and no CPU fallback."""
import ctypes
import os

import numpy as np
import pytest

import mesh_dist_ref64 as M


def test_box_against_closed_form():
    lo, hi = (-0.75, 0.5, 1.0), (1.25, 2.0, 1.5)
    verts, tris = M.box_mesh(lo, hi)
    assert tris.shape == (12, 3)
    rng = np.random.default_rng(3)
    P = rng.uniform(-2.0, 3.5, size=(4000, 3))                       # inside and outside
    g = [np.array([lo[a], hi[a], 0.5 * (lo[a] + hi[a]), lo[a] - 0.5, hi[a] + 0.25]) for a in range(3)]
    Z, Y, X = np.meshgrid(g[2], g[1], g[0], indexing="ij")           # on faces, edges and corners, and beside them
    P = np.concatenate([P, np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)])
    d, idx = M.distance_brute(verts, tris, P)
    want = M.box_distance(P, lo, hi)
    L = max(np.abs(P).max(), 2.0)
    assert np.abs(d - want).max() <= M.K / 4 * M.EPS * L, np.abs(d - want).max() / (M.EPS * L)
    on = want == 0.0
    assert on.sum() >= 26 and (d[on] == 0.0).all()
    assert ((idx >= 0) & (idx < 12)).all()
    assert np.array_equal(M.distance_to_given(verts, tris, P, idx), d)


def hand_made_set():
    """(verts float32, tris int32, points float64): slivers of aspect 1e-7, exactly degenerate triangles, duplicate vertices,
    vertices on the points of a lattice with a non-dyadic origin"""
    rng = np.random.default_rng(11)
    origin, h = np.array([0.1, -0.7, 1.3]), 0.3
    V, T = [], []

    def tri(a, b, c):
        T.append([len(V), len(V) + 1, len(V) + 2])
        V.extend([a, b, c])

    for _ in range(40):                                              # ordinary
        c = rng.uniform(-1, 3, 3)
        tri(c + rng.normal(size=3) * 0.4, c + rng.normal(size=3) * 0.4, c + rng.normal(size=3) * 0.4)
    for _ in range(40):                                              # needles and caps of aspect 1e-7
        a = rng.uniform(-1, 1, 3) * 1e-3
        e = rng.normal(size=3)
        e /= np.linalg.norm(e)
        s = np.cross(e, rng.normal(size=3))
        s /= np.linalg.norm(s)
        t = rng.choice([0.0, 0.5, 1.0])
        tri(a, a + e, a + t * e + 1e-7 * s)
    for _ in range(20):                                              # exactly degenerate: collinear, two equal, all equal
        a = np.float32(rng.uniform(-1, 2, 3)).astype(np.float64)
        e = np.array([0.25, -0.5, 0.125])
        tri(a, a + e, a + 2 * e)
        tri(a, a, a + e)
        tri(a, a, a)
    for _ in range(30):                                              # vertices on lattice points
        i = rng.integers(0, 8, size=(3, 3))
        tri(*(origin + h * i.astype(np.float64)))
    V = np.array(V, np.float32)
    T = np.array(T, np.int32)
    T = np.concatenate([T, T[:5]])                                   # duplicate triangles
    # points: lattice points (some coincide with vertices), points close to the slivers' planes and long edges, random ones
    I = rng.integers(0, 8, size=(1500, 3)).astype(np.float64)
    P = [origin + h * I, rng.uniform(-1.5, 3.5, size=(1500, 3))]
    Vd = V.astype(np.float64)
    for t in T[40:80]:
        a, b, c = Vd[t]
        u = rng.uniform(0, 1, size=(25, 1))
        w = rng.uniform(0, 1, size=(25, 1))
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        P.append(a + u * (b - a) + w * (1 - u) * (c - a) + rng.choice([0.0, 1e-9, 1e-3, 0.3], size=(25, 1)) * n)
    return V, T, np.concatenate(P)


def test_restatement_against_mpmath():
    V, T, P = hand_made_set()
    rng = np.random.default_rng(5)
    n = 4000
    pi, ti = rng.integers(0, len(P), n), rng.integers(0, len(T), n)
    # every sliver with the points made for it
    pi[:1000] = 3000 + np.arange(1000)
    ti[:1000] = 40 + np.arange(1000) // 25
    d = M.distance_to_given(V, T, P[pi], ti)
    assert np.isfinite(d).all()
    L = max(np.abs(P).max(), float(np.abs(V).max()))
    Vd = V.astype(np.float64)
    worst = 0.0
    for k in range(n):
        a, b, c = Vd[T[ti[k]]]
        worst = max(worst, abs(float(M.pair_mp(P[pi[k]], a, b, c) - d[k])) / (M.EPS * L))
    print(f"REDIST K measured ratio {worst:.3f} (L = {L:.3f}); K = {M.K:g}")
    assert worst <= M.K / 4, worst
    assert worst <= M.MEASURED_RATIO * 1.0001, "the docstring's measured ratio is out of date"


def test_lattice_form_equals_brute_force():
    rng = np.random.default_rng(2)
    dims, origin, h = (11, 7, 9), (0.1, -0.3, 0.7), 0.3
    V = rng.uniform(0, 3, size=(90, 3)).astype(np.float32)
    T = rng.integers(0, 90, size=(60, 3)).astype(np.int32)
    P = M.lattice_points(dims, origin, h)
    d, idx = M.distance_brute(V, T, P)
    for band in (0.2, 0.7, 50.0):
        db, ib, raw, _ = M.lattice_distance(V, T, dims, origin, h, band, block=4)
        far = ~(d < band)
        assert np.array_equal(db, np.where(far, band, d))
        assert np.array_equal(ib, np.where(far, -1, idx))
        assert np.array_equal(raw[~far], d[~far])
    d0, i0, _, _ = M.lattice_distance(V, T[:0], dims, origin, h, 0.5)
    assert (d0 == 0.5).all() and (i0 == -1).all()


def _call(pkg, verts, tris, dims, origin, spacing, band, nv=None):
    L = pkg._lib
    verts, tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32)
    out = np.full(int(np.prod(dims)), -7.0)
    rc = L.lib().r2s_mesh_distance(verts.ctypes.data_as(L.c_float_p), len(verts) if nv is None else nv,
                                   tris.ctypes.data_as(L.c_int32_p), len(tris), (ctypes.c_int64 * 3)(*dims),
                                   (ctypes.c_double * 3)(*origin), spacing, band, 0, -1, out.ctypes.data_as(ctypes.c_void_p), None)
    return rc, out


def test_refusals_need_no_device(pkg):
    """argument errors come before any device work: the same codes with and without a GPU"""
    V, T = M.box_mesh((0, 0, 0), (1, 1, 1))
    ARG = -1
    bad = [dict(dims=(1, 4, 4)), dict(spacing=0.0), dict(spacing=np.inf), dict(band=0.0), dict(band=-1.0), dict(band=np.nan),
           dict(origin=(0.0, np.nan, 0.0))]
    for kw in bad:
        a = dict(dims=(4, 4, 4), origin=(0.0, 0.0, 0.0), spacing=0.5, band=1.0)
        a.update(kw)
        rc, out = _call(pkg, V, T, **a)
        assert rc == ARG and (out == -7.0).all(), kw
    T2 = T.copy()
    T2[7, 1] = 8                                                     # == n_verts
    rc, out = _call(pkg, V, T2, (4, 4, 4), (0.0, 0.0, 0.0), 0.5, 1.0)
    assert rc == ARG and (out == -7.0).all() and b"index" in pkg._lib.lib().r2s_last_error()
    V2 = V.copy()
    V2[3, 2] = np.inf
    rc, out = _call(pkg, V2, T, (4, 4, 4), (0.0, 0.0, 0.0), 0.5, 1.0)
    assert rc == ARG and (out == -7.0).all()
    f = np.zeros(64, np.float32)
    L = pkg._lib
    rc = L.lib().r2s_redistance(f.ctypes.data_as(ctypes.c_void_p), 1, (ctypes.c_int64 * 3)(4, 4, 4), (ctypes.c_double * 3)(0, 0, 0),
                                0.5, float("nan"), 1.0, -1, f.ctypes.data_as(ctypes.c_void_p))
    assert rc == ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = M.box_mesh((0, 0, 0), (1, 1, 1))
    rc, out = _call(pkg, V, T, (4, 4, 4), (0.0, 0.0, 0.0), 0.5, 1.0)
    assert rc == -2 and (out == -7.0).all()                          # R2S_ERR_NO_DEVICE
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.redistance(np.zeros((4, 4, 4), np.float32), pkg.Grid([0, 0, 0], [1, 1, 1], 3, 0), band=1.0)
