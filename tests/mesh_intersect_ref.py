"""numpy restatement of the self-intersection definition of include/rho2sdf_hip.h (r2s_mesh_index_intersections), brute force over
all pairs s < t, for tests/test_mesh_intersect_*.py, and the same question in exact arithmetic (fractions.Fraction).

Definition (the header has the full text): a candidate pair is two non-collapsed triangles s < t whose closed float32 boxes
overlap; sharing two or three vertex indices it is skipped as adjacent, sharing one index v only the edges opposite v are tested
(two segment tests), else all six edges; the segment test is the ray pair test of tests/ray_ref64.py::_pairs (same step order,
every operation rounded on its own) with o = p, d = q - p, a hit being not mixed, det != 0 and 0 <= t <= 1."""
from fractions import Fraction

import numpy as np


def _frames(d):
    """ray_ref64._frames: kz the axis of the largest |d| (lowest on ties), kx, ky the next two, swapped for d[kz] < 0"""
    ad = np.abs(d)
    kz = np.zeros(len(d), np.int64)
    big = ad[:, 0].copy()
    for k in (1, 2):
        up = ad[:, k] > big
        kz[up] = k
        big[up] = ad[up, k]
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = d[np.arange(len(d)), kz] < 0.0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    return kx, ky, kz


def segment_hits(p, q, a, b, c):
    """row i: does the segment p[i] -> q[i] hit the triangle a[i] b[i] c[i]?  (m, 3) float64 each -> (m,) bool; the steps of
    ray_ref64._pairs, one segment against one triangle per row"""
    m = len(p)
    if m == 0:
        return np.zeros(0, bool)
    r = np.arange(m)
    d = q - p
    zero = (d == 0.0).all(axis=1)
    kx, ky, kz = _frames(d)
    with np.errstate(all="ignore"):
        dz = d[r, kz]
        Sx, Sy, Sz = d[r, kx] / dz, d[r, ky] / dz, 1.0 / dz
        sh = []
        for v in (a, b, c):
            z = v[r, kz] - p[r, kz]
            x = (v[r, kx] - p[r, kx]) - Sx * z
            y = (v[r, ky] - p[r, ky]) - Sy * z
            sh.append((x, y, z))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sh
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        det = (U + V) + W
        t = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det
        mixed = ((U < 0.0) | (V < 0.0) | (W < 0.0)) & ((U > 0.0) | (V > 0.0) | (W > 0.0))
        return ~zero & ~mixed & (det != 0.0) & (t >= 0.0) & (t <= 1.0)


def collapsed(T):
    return (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 0] == T[:, 2])


def candidates(verts, tris, chunk=512):
    """-> (S, Tt) int64 arrays of the candidate pairs, ascending by (s, t): s < t, both non-collapsed, closed float32 boxes
    overlapping on all three axes"""
    V = np.asarray(verts, np.float32).reshape(-1, 3)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(T)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    P = V[T]                                              # (n, 3 corners, 3 axes) float32
    lo, hi = P.min(axis=1), P.max(axis=1)
    ok = ~collapsed(T)
    S, Tt = [], []
    for s0 in range(0, n, chunk):
        s1 = min(s0 + chunk, n)
        ov = ((lo[s0:s1, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[s0:s1, None, :])).all(axis=2)
        ov &= ok[s0:s1, None] & ok[None, :]
        ov &= np.arange(s0, s1)[:, None] < np.arange(n)[None, :]
        i, j = np.nonzero(ov)
        S.append(i + s0)
        Tt.append(j)
    return np.concatenate(S), np.concatenate(Tt)


def tests_of(T, S, Tt):
    """the segment tests of the candidate pairs -> (shared (m,), mask (m, 6) bool): mask[:, c] = edge c of s against t,
    mask[:, 3 + c] = edge c of t against s; edge c runs from corner c to corner (c + 1) % 3"""
    eq = T[S][:, :, None] == T[Tt][:, None, :]            # (m, corner of s, corner of t)
    in_t, in_s = eq.any(axis=2), eq.any(axis=1)
    shared = in_t.sum(axis=1)
    mask = np.zeros((len(S), 6), bool)
    mask[shared == 0] = True
    one = np.nonzero(shared == 1)[0]
    a, b = in_t[one].argmax(axis=1), in_s[one].argmax(axis=1)
    mask[one, (a + 1) % 3] = True                         # the edge opposite corner a is edge (a + 1) % 3
    mask[one, 3 + (b + 1) % 3] = True
    return shared, mask


def intersections(verts, tris):
    """-> (pairs (n, 2) int32 ascending by (s, t), hits_of_tri (nt,) int32, totals (8,) int64): the definition over all pairs"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    S, Tt = candidates(verts, T)
    shared, mask = tests_of(T, S, Tt)
    hit = np.zeros(len(S), bool)
    for k in range(6):
        own, c = k < 3, k % 3
        rows = np.nonzero(mask[:, k] & ~hit)[0]
        E, O = (S, Tt)[0 if own else 1][rows], (Tt, S)[0 if own else 1][rows]
        hit[rows] = segment_hits(v[T[E, c]], v[T[E, (c + 1) % 3]], v[T[O, 0]], v[T[O, 1]], v[T[O, 2]])
    pairs = np.stack([S[hit], Tt[hit]], axis=1).astype(np.int32).reshape(-1, 2)
    hits = np.bincount(pairs.ravel(), minlength=len(T)).astype(np.int32)
    totals = np.array([len(pairs), int((hits > 0).sum()), len(S), int((shared >= 2).sum()), int((shared == 1).sum()),
                       int(collapsed(T).sum()), 0, 0], np.int64)
    return pairs, hits, totals


# ---- the same question in exact arithmetic ------------------------------------------------------------------------------------

MARGIN = Fraction(1, 2 ** 40)


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _parallel_exact(p, q, a, b, c, n, nn, dd):
    """a segment exactly parallel to the triangle's plane: False when it stays strictly clear with the margin (off the plane, or in
    the plane and separated from the triangle by one of the triangle's edge lines or by its own line), else None (coplanar
    overlap or contact is out of scope: the definition never reports it and no verdict is asked of it)"""
    size2 = max(dd, _dot(_sub(b, a), _sub(b, a)), _dot(_sub(c, b), _sub(c, b)), _dot(_sub(a, c), _sub(a, c)))
    h = _dot(n, _sub(p, a))
    if h != 0:
        return False if h * h >= MARGIN * MARGIN * nn * size2 else None
    k = max(range(3), key=lambda i: abs(n[i]))            # the plane's coordinates: drop the axis of the largest |n|
    i, j = (k + 1) % 3, (k + 2) % 3
    tri, seg = [(v[i], v[j]) for v in (a, b, c)], [(v[i], v[j]) for v in (p, q)]
    lines = [(tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]), (seg[0], seg[1])]
    for (u, w) in lines:
        m = (-(w[1] - u[1]), w[0] - u[0])                 # a normal of the line u w
        pt, ps = [m[0] * v[0] + m[1] * v[1] for v in tri], [m[0] * v[0] + m[1] * v[1] for v in seg]
        gap = max(min(ps) - max(pt), min(pt) - max(ps))
        if gap > 0 and gap * gap >= MARGIN * MARGIN * (m[0] * m[0] + m[1] * m[1]) * size2:
            return False
    return None


def segment_exact(p, q, a, b, c):
    """the segment p -> q against the triangle a b c over Fractions -> True (it properly crosses the open triangle), False (it
    stays strictly clear of it) or None (not decided with the margin 2^-40).  With |det| = |n.d| at least 2^-40 |n| |d|:
    True needs 2^-40 <= t <= 1 - 2^-40 and every barycentric coordinate of the crossing point >= 2^-40; False needs t beyond
    an end of [0, 1] by 2^-40, or a barycentric coordinate <= -2^-40 (the line meets the plane decidedly outside the
    triangle, whatever t); anything nearer than the margin to an end, an edge or the plane is None.  A segment exactly
    parallel to the plane: _parallel_exact."""
    d, n = _sub(q, p), _cross(_sub(b, a), _sub(c, a))
    nd, nn, dd = _dot(n, d), _dot(n, n), _dot(d, d)
    if nn == 0 or dd == 0:
        return None                                       # a degenerate triangle or segment
    if nd == 0:
        return _parallel_exact(p, q, a, b, c, n, nn, dd)
    if nd * nd < MARGIN * MARGIN * nn * dd:
        return None                                       # nearly parallel to the plane
    t = _dot(n, _sub(a, p)) / nd
    if t <= -MARGIN or t >= 1 + MARGIN:
        return False
    x = [p[k] + t * d[k] for k in range(3)]
    bary = [_dot(n, _cross(_sub(c, b), _sub(x, b))) / nn, _dot(n, _cross(_sub(a, c), _sub(x, c))) / nn,
            _dot(n, _cross(_sub(b, a), _sub(x, a))) / nn]
    if any(w <= -MARGIN for w in bary):
        return False                                      # the line meets the plane decidedly outside the triangle, whatever t
    if MARGIN <= t <= 1 - MARGIN and all(w >= MARGIN for w in bary):
        return True
    return None


def pairs_exact(verts, tris):
    """the candidate pairs classified over Fractions -> (S, Tt, verdict): verdict True when a segment test of the pair is a
    decided crossing, False when all of them are decided clear, None otherwise; adjacent pairs are left out"""
    V = np.asarray(verts, np.float32).reshape(-1, 3)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    F = [[Fraction(float(x)) for x in row] for row in V]
    S, Tt = candidates(verts, T)
    shared, mask = tests_of(T, S, Tt)
    keep = shared < 2
    out = []
    for s, t, m in zip(S[keep], Tt[keep], mask[keep]):
        verdict = False
        for k in np.nonzero(m)[0]:
            e, o = (s, t) if k < 3 else (t, s)
            c = k % 3
            r = segment_exact(F[T[e, c]], F[T[e, (c + 1) % 3]], F[T[o, 0]], F[T[o, 1]], F[T[o, 2]])
            if r:
                verdict = True
                break
            if r is None:
                verdict = None
        out.append(verdict)
    return S[keep], Tt[keep], out
