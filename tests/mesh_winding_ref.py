"""The winding number of include/rho2sdf_hip.h (r2s_mesh_index_winding) restated in numpy, to the letter: a loop over ALL triangles,
vectorised over the points, float64 with every operation rounded on its own (numpy has no fused multiply-add).  And the same pair
test in exact rational arithmetic, to measure the documented limit: a computed edge function that is 0 where the exact one is not
sends the tie rule against the truth.

winding_ref(V, T, P, ray) -> (winding, crossings), int32.
exact_disagreements(V, T, P, ray) -> (pairs examined exactly, pairs whose computed verdict differs from the exact one)."""
from fractions import Fraction

import numpy as np

RAYS = range(6)
POSITIVE, NONZERO, ODD = 0, 1, 2


def frame(ray):
    """step 1: kx, ky, kz, Sz"""
    kz = ray % 3
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    if ray >= 3:
        kx, ky = ky, kx
    return kx, ky, kz, (1.0 if ray < 3 else -1.0)


def _tie(px, py, qx, qy):
    """step 4 for f == 0: the sign of Qy - Py, else of Px - Qx (the vertices' own coordinates: exact differences)"""
    if qy != py:
        return 1 if qy > py else -1
    return 1 if px > qx else (-1 if px < qx else 0)


def _esign(f, px, py, qx, qy):
    return np.where(f == 0.0, _tie(px, py, qx, qy), np.where(f > 0.0, 1, -1)).astype(np.int64)


def _own_box(a, b, c, P, finite, ray):
    """step 6, first half: the points whose ray may meet the triangle's own float32 box (float32 values in float64: exact)"""
    kx, ky, kz, _ = frame(ray)
    lo, hi = np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))
    ahead = hi[kz] >= P[:, kz] if ray < 3 else lo[kz] <= P[:, kz]
    return finite & (lo[kx] <= P[:, kx]) & (P[:, kx] <= hi[kx]) & (lo[ky] <= P[:, ky]) & (P[:, ky] <= hi[ky]) & ahead


def _pair(a, b, c, o, ray):
    """steps 2 to 6 for the points o (m, 3) against one triangle -> (crossing (m,) bool, side (m,) int, U, V, W, the Sz-scaled
    A[kz], B[kz], C[kz])"""
    kx, ky, kz, Sz = frame(ray)
    Ax, Ay, Bx, By, Cx, Cy = a[kx] - o[:, kx], a[ky] - o[:, ky], b[kx] - o[:, kx], b[ky] - o[:, ky], c[kx] - o[:, kx], c[ky] - o[:, ky]
    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
    su = _esign(U, b[kx], b[ky], c[kx], c[ky])
    sv = _esign(V, c[kx], c[ky], a[kx], a[ky])
    sw = _esign(W, a[kx], a[ky], b[kx], b[ky])
    cross = (su == sv) & (su == sw) & (su != 0)
    det = (U + V) + W
    Az, Bz, Cz = Sz * (a[kz] - o[:, kz]), Sz * (b[kz] - o[:, kz]), Sz * (c[kz] - o[:, kz])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((U * Az + V * Bz) + W * Cz) / det
    cross &= (det != 0.0) & (t > 0.0)
    return cross, su, (U, V, W), (Az, Bz, Cz), (su, sv, sw)


def _inputs(V, T, P):
    V = np.asarray(V)
    assert V.dtype == np.float32
    P = np.asarray(P)
    assert P.dtype in (np.float32, np.float64)
    return V.astype(np.float64).reshape(-1, 3), np.asarray(T).reshape(-1, 3), P.astype(np.float64).reshape(-1, 3)


def winding_ref(V, T, P, ray):
    V, T, P = _inputs(V, T, P)
    n = len(P)
    wn, nc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    finite = np.isfinite(P).all(axis=1)
    for ia, ib, ic in T:
        if ia == ib or ib == ic or ia == ic:       # a collapsed triangle takes part in nothing
            continue
        a, b, c = V[ia], V[ib], V[ic]
        idx = np.nonzero(_own_box(a, b, c, P, finite, ray))[0]
        if idx.size == 0:
            continue
        cross, side = _pair(a, b, c, P[idx], ray)[:2]
        wn[idx] -= np.where(cross, side, 0).astype(np.int32)
        nc[idx] += cross.astype(np.int32)
    nc[~finite] = -1
    return wn, nc


def inside(wn, nc, rule):
    return (wn > 0, wn != 0, (nc > 0) & (nc % 2 == 1))[rule]


# ---- the exact pair test -------------------------------------------------------------------------------------------------

def _exact_pair(a, b, c, o, ray):
    """the effective signs and the crossing verdict of one pair with U, V, W, t exact (Fractions of the float64 inputs)"""
    kx, ky, kz, Sz = frame(ray)
    F = Fraction
    fa, fb, fc, fo = [F(float(x)) for x in a], [F(float(x)) for x in b], [F(float(x)) for x in c], [F(float(x)) for x in o]
    Ax, Ay, Bx, By, Cx, Cy = fa[kx] - fo[kx], fa[ky] - fo[ky], fb[kx] - fo[kx], fb[ky] - fo[ky], fc[kx] - fo[kx], fc[ky] - fo[ky]
    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax

    def es(f, p, q):
        return (1 if f > 0 else -1) if f != 0 else _tie(p[kx], p[ky], q[kx], q[ky])
    s = (es(U, fb, fc), es(V, fc, fa), es(W, fa, fb))
    cross = s[0] == s[1] == s[2] != 0
    if cross:
        det = U + V + W
        cross = det != 0 and (U * (fa[kz] - fo[kz]) + V * (fb[kz] - fo[kz]) + W * (fc[kz] - fo[kz])) * int(Sz) / det > 0
    return s, cross


def exact_disagreements(V, T, P, ray):
    """Over every (point, triangle) pair that passes the own-box condition: does a computed effective sign, or the computed
    crossing verdict, differ from the exact one?  A pair is examined exactly unless a static filter proves its computed verdict:
    with u = 2^-53 each of U, V, W carries an absolute error below 5 u (|l| + |r|) of its two products (three roundings per
    product, one for the difference), so |f| > 2^-49 (|l| + |r|) fixes its sign; three such signs that differ settle "no crossing";
    three equal ones with the whole triangle strictly ahead of (or behind) the point settle t > 0 (or t < 0), every term of the
    numerator and det then having one sign.  -> (pairs examined exactly, disagreements)"""
    V, T, P = _inputs(V, T, P)
    kx, ky, kz, Sz = frame(ray)
    finite = np.isfinite(P).all(axis=1)
    examined = bad = 0
    for ia, ib, ic in T:
        if ia == ib or ib == ic or ia == ic:
            continue
        a, b, c = V[ia], V[ib], V[ic]
        idx = np.nonzero(_own_box(a, b, c, P, finite, ray))[0]
        if idx.size == 0:
            continue
        o = P[idx]
        cross, _, (U, Vv, W), (Az, Bz, Cz), signs = _pair(a, b, c, o, ray)
        Ax, Ay, Bx, By, Cx, Cy = a[kx] - o[:, kx], a[ky] - o[:, ky], b[kx] - o[:, kx], b[ky] - o[:, ky], c[kx] - o[:, kx], c[ky] - o[:, ky]
        tol = 2.0 ** -49
        sure = (np.abs(U) > tol * (np.abs(Cx * By) + np.abs(Cy * Bx))) & (np.abs(Vv) > tol * (np.abs(Ax * Cy) + np.abs(Ay * Cx))) & \
            (np.abs(W) > tol * (np.abs(Bx * Ay) + np.abs(By * Ax)))
        same = (signs[0] == signs[1]) & (signs[0] == signs[2])
        one_side = ((Az > 0) & (Bz > 0) & (Cz > 0)) | ((Az < 0) & (Bz < 0) & (Cz < 0))
        proven = sure & (~same | one_side)
        for j in np.nonzero(~proven)[0]:
            s, x = _exact_pair(a, b, c, o[j], ray)
            examined += 1
            if s != (signs[0][j], signs[1][j], signs[2][j]) or x != bool(cross[j]):
                bad += 1
    return examined, bad


def predicate_along_row(a, b, c, base, h, n, ray):
    """step 6's per-point conditions (box ahead, det != 0, t > 0) for the n points base + h * i * e_kz, i = 0 .. n - 1, of one
    triangle whose projected conditions the row shares -> (n,) bool.  Monotone in i: what a row kernel would bisect."""
    a, b, c = [np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c)]
    kx, ky, kz, Sz = frame(ray)
    o = np.repeat(np.asarray(base, np.float64)[None, :], n, axis=0)
    o[:, kz] = base[kz] + h * np.arange(n, dtype=np.float64)
    lo, hi = np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))
    ahead = hi[kz] >= o[:, kz] if ray < 3 else lo[kz] <= o[:, kz]
    _, _, (U, V, W), (Az, Bz, Cz), _ = _pair(a, b, c, o, ray)
    det = (U + V) + W
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((U * Az + V * Bz) + W * Cz) / det
    return ahead & (det != 0.0) & (t > 0.0)
