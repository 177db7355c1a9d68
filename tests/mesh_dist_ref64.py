"""float64 restatement of the mesh distance of include/rho2sdf_hip.h (r2s_mesh_distance / r2s_redistance), and the same
per-pair routine in mpmath at 50 digits, for tests/test_redistance_*.py.

Definition: lattice point p = origin + spacing * (i, j, k) in float64 (x fastest); vertices are float32 widened to float64;
the distance to a triangle (a, b, c) is the minimum of the distances to the segments a-b, a-c, b-c (foot-point parameter
clamped to [0, 1], a zero-length segment is a point) and of the plane distance |n.(p-a)| / |n|, the latter counted only
when n = (b-a) x (c-a) is non-zero and the three edge functions are >= 0.  d(p) is the minimum over the triangles, the
result min(d, band), the index the smallest one that attains the minimum (-1 where the result is band).

The float64 form works on squared distances with per-triangle reciprocals and in-plane edge normals n x e (the edge function
((b-a) x (p-a)).n equals (p-a).(n x (b-a))) and takes one square root at the end; `pair_mp` evaluates the definition as
written, with divisions and cross products per pair.

Bound constant K (tests/test_redistance_cpu.py::test_restatement_against_mpmath measures it): with L the largest absolute
lattice or vertex coordinate of a case, the largest |ref64 - mp| / (2^-52 L) seen on the hand-made set (slivers of aspect
1e-7, exactly degenerate triangles, duplicate vertices, vertices on lattice points with a non-dyadic origin; 4000 pairs)
is MEASURED_RATIO below; K = 4 x that, rounded up to a power of two and at least 8.  The factor 4 leaves room for an
equivalent formula with other roundings in the kernel.  The CPU test asserts that the restatement stays within K / 4.
"""
import numpy as np

MEASURED_RATIO = 0.9   # largest |ref64 - mp| / (2^-52 L) on the hand-made set (printed by the CPU test as "REDIST K ...")
K = 8.0                # 4 x MEASURED_RATIO rounded up to a power of two, at least 8
EPS = 2.0 ** -52


def bound(ref, L, out_dtype):
    """|out - ref| allowed: one rounding to the output type + K 2^-52 L"""
    u = 2.0 ** -24 if np.dtype(out_dtype) == np.float32 else 2.0 ** -53
    return u * np.abs(ref) + K * EPS * L


def coord_scale(verts, dims, origin, spacing):
    """L: the largest absolute lattice or vertex coordinate"""
    o = np.asarray(origin, np.float64)
    far = o + float(spacing) * (np.asarray(dims, np.float64) - 1.0)
    L = max(np.abs(o).max(), np.abs(far).max())
    if len(verts):
        L = max(L, float(np.abs(np.asarray(verts, np.float64)).max()))
    return float(L)


def lattice_axes(dims, origin, spacing):
    return [np.float64(origin[a]) + np.float64(spacing) * np.arange(dims[a], dtype=np.float64) for a in range(3)]


def lattice_points(dims, origin, spacing):
    """(nx*ny*nz, 3) float64, x fastest"""
    x, y, z = lattice_axes(dims, origin, spacing)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; numpy has no fma)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dop(a, b, c, d):
    """a * b - c * d to about one ulp (the kernel uses Kahan's fma form)"""
    p, ep = _two_prod(a, b)
    q, eq = _two_prod(c, d)
    return (p - q) + (ep - eq)


def _cross_exact(a, b):
    """the normal of a sliver must keep its direction: plain products tilt the plane by 2^-53 / aspect"""
    return (_dop(a[1], b[2], a[2], b[1]), _dop(a[2], b[0], a[0], b[2]), _dop(a[0], b[1], a[1], b[0]))


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _inv(e):
    with np.errstate(divide="ignore", over="ignore"):
        r = np.where(e > 0.0, 1.0 / np.where(e > 0.0, e, 1.0), 0.0)
    return np.where(np.isfinite(r), r, 0.0)


class Records:
    """per-triangle data, every field a tuple of three (nt,) arrays or one (nt,) array"""

    def __init__(self, verts, tris):
        v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
        t = np.asarray(tris, np.int64).reshape(-1, 3)
        a, b, c = (tuple(v[t[:, k], i] for i in range(3)) for k in range(3))
        self.a, self.b = a, b
        self.ab, self.ac, self.bc = _sub(b, a), _sub(c, a), _sub(c, b)
        self.n = _cross_exact(self.ab, self.ac)
        self.mab, self.mac, self.mbc = _cross(self.n, self.ab), _cross(self.n, self.ac), _cross(self.n, self.bc)
        self.iab, self.iac, self.ibc = _inv(_dot(self.ab, self.ab)), _inv(_dot(self.ac, self.ac)), _inv(_dot(self.bc, self.bc))
        self.inn = _inv(_dot(self.n, self.n))
        self.lo = np.minimum(np.minimum(v[t[:, 0]], v[t[:, 1]]), v[t[:, 2]]) if len(t) else np.zeros((0, 3))
        self.hi = np.maximum(np.maximum(v[t[:, 0]], v[t[:, 1]]), v[t[:, 2]]) if len(t) else np.zeros((0, 3))
        self.nt = len(t)

    def take(self, sel):
        r = object.__new__(Records)
        for k, val in self.__dict__.items():
            if isinstance(val, tuple):
                setattr(r, k, tuple(x[sel] for x in val))
            elif isinstance(val, np.ndarray):
                setattr(r, k, val[sel])
        r.nt = len(r.inn)
        return r


def _seg_d2(w, e, inv):
    t = _dot(w, e) * inv
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    q = (w[0] - t * e[0], w[1] - t * e[1], w[2] - t * e[2])
    return _dot(q, q)


def pair_d2(P, R):
    """squared distances of the points P (m, 3) to the triangles of R: (m, nt); see pair_d2_each for point i against triangle i"""
    p = tuple(P[:, i][:, None] for i in range(3))
    return _pair_d2(p, R, lambda x: x[None, :])


def pair_d2_each(P, R):
    """point i against triangle i: (m,)"""
    return _pair_d2(tuple(P[:, i] for i in range(3)), R, lambda x: x)


def _pair_d2(p, R, sh):
    g = lambda v: tuple(sh(x) for x in v)   # noqa: E731
    ap, bp = _sub(p, g(R.a)), _sub(p, g(R.b))
    d2 = _seg_d2(ap, g(R.ab), sh(R.iab))
    d2 = np.minimum(d2, _seg_d2(ap, g(R.ac), sh(R.iac)))
    d2 = np.minimum(d2, _seg_d2(bp, g(R.bc), sh(R.ibc)))
    inn = sh(R.inn)
    inside = (inn > 0.0) & (_dot(ap, g(R.mab)) >= 0.0) & (_dot(bp, g(R.mbc)) >= 0.0) & (-_dot(ap, g(R.mac)) >= 0.0)
    s = _dot(g(R.n), ap)
    dp = s * s * inn
    return np.where(inside & (dp < d2), dp, d2)


def distance_brute(verts, tris, points, chunk=2048):
    """-> (d (m,), index (m,)) over ALL triangles, no culling; index -1 and d inf without triangles"""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    R = Records(verts, tris)
    best = np.full(len(P), np.inf)
    idx = np.full(len(P), -1, np.int64)
    step = max(1, int(4_000_000 // max(len(P), 1)))
    for t0 in range(0, R.nt, min(chunk, step)):
        sel = np.arange(t0, min(R.nt, t0 + min(chunk, step)))
        d2 = pair_d2(P, R.take(sel))
        j = d2.argmin(axis=1)            # (first = smallest index among equals)
        m = d2[np.arange(len(P)), j]
        better = m < best                # (strict: earlier chunks keep ties)
        best[better] = m[better]
        idx[better] = sel[j[better]]
    return np.sqrt(best), idx


def distance_to_given(verts, tris, points, tri_index):
    """distance of point i to triangle tri_index[i]"""
    R = Records(verts, tris).take(np.asarray(tri_index, np.int64))
    return np.sqrt(pair_d2_each(np.asarray(points, np.float64).reshape(-1, 3), R))


def lattice_distance(verts, tris, dims, origin, spacing, band, block=4):
    """-> (min(d, band), index (-1 where band), d, second) on every lattice point (x fastest): the same minimum as
    distance_brute, with the triangles of each block of voxels pre-selected by AABB (box-to-box distance <= band * (1 + 1e-9)
    + 1e-9 L: a triangle left out is farther than the band from every voxel of the block).  d is the unclamped minimum and
    second the second smallest per-triangle distance, both over the pre-selected triangles only (inf without): exact where
    they are below the band"""
    nx, ny, nz = (int(n) for n in dims)
    ax = lattice_axes(dims, origin, spacing)
    R = Records(verts, tris)
    L = coord_scale(verts, dims, origin, spacing)
    r = band * (1.0 + 1e-9) + 1e-9 * L
    out = np.full((nz, ny, nx), np.inf)
    idx = np.full((nz, ny, nx), -1, np.int64)
    sec = np.full((nz, ny, nx), np.inf)
    for z0 in range(0, nz, block):
        zs = slice(z0, min(nz, z0 + block))
        gz = np.maximum(0.0, np.maximum(R.lo[:, 2] - ax[2][zs][-1], ax[2][zs][0] - R.hi[:, 2]))
        selz = np.nonzero(gz <= r)[0]
        for y0 in range(0, ny, block):
            ys = slice(y0, min(ny, y0 + block))
            gy = np.maximum(0.0, np.maximum(R.lo[selz, 1] - ax[1][ys][-1], ax[1][ys][0] - R.hi[selz, 1]))
            keep = gy * gy + gz[selz] ** 2 <= r * r
            sely, gyz = selz[keep], (gy * gy + gz[selz] ** 2)[keep]
            for x0 in range(0, nx, block):
                xs = slice(x0, min(nx, x0 + block))
                gx = np.maximum(0.0, np.maximum(R.lo[sely, 0] - ax[0][xs][-1], ax[0][xs][0] - R.hi[sely, 0]))
                sel = sely[gx * gx + gyz <= r * r]
                if len(sel) == 0:
                    continue
                Z, Y, X = np.meshgrid(ax[2][zs], ax[1][ys], ax[0][xs], indexing="ij")
                P = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
                d2 = pair_d2(P, R.take(sel))
                j = d2.argmin(axis=1)
                out[zs, ys, xs] = d2[np.arange(len(P)), j].reshape(Z.shape)
                idx[zs, ys, xs] = sel[j].reshape(Z.shape)
                if len(sel) > 1:
                    sec[zs, ys, xs] = np.partition(d2, 1, axis=1)[:, 1].reshape(Z.shape)
    raw = np.sqrt(out).ravel()
    idx = idx.ravel()
    far = ~(raw < band)
    d = np.where(far, band, raw)
    idx[far] = -1
    return d, idx, raw, np.sqrt(sec).ravel()


def box_mesh(lo, hi):
    """the 12 triangles of an axis-aligned box, outward normals: (verts (8, 3) float32, tris (12, 3) int32)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = [f for a, b, c, d in q for f in ((a, b, c), (a, c, d))]
    return v, np.array(t, np.int32)


def box_distance(points, lo, hi):
    """closed form: distance to the SURFACE of the box [lo, hi]"""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = np.sqrt((np.maximum(0.0, np.maximum(lo - P, P - hi)) ** 2).sum(axis=1))
    inside = ((P >= lo) & (P <= hi)).all(axis=1)
    return np.where(inside, np.minimum(P - lo, hi - P).min(axis=1), out)


def pair_mp(p, a, b, c, digits=50):
    """the definition as written, in mpmath: distance of point p to triangle (a, b, c) (sequences of 3 floats)"""
    import mpmath as mp
    mp.mp.dps = digits
    f = lambda v: [mp.mpf(float(x)) for x in v]   # noqa: E731
    p, a, b, c = f(p), f(a), f(b), f(c)
    sub = lambda u, v: [u[i] - v[i] for i in range(3)]   # noqa: E731
    dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]   # noqa: E731
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]   # noqa: E731

    def seg(u, v):
        e, w = sub(v, u), sub(p, u)
        ee = dot(e, e)
        t = dot(w, e) / ee if ee > 0 else mp.mpf(0)
        t = min(max(t, mp.mpf(0)), mp.mpf(1))
        q = [w[i] - t * e[i] for i in range(3)]
        return mp.sqrt(dot(q, q))

    d = min(seg(a, b), seg(a, c), seg(b, c))
    n = cross(sub(b, a), sub(c, a))
    nn = dot(n, n)
    if nn > 0:
        e0 = dot(cross(sub(b, a), sub(p, a)), n)
        e1 = dot(cross(sub(c, b), sub(p, b)), n)
        e2 = dot(cross(sub(a, c), sub(p, c)), n)
        if e0 >= 0 and e1 >= 0 and e2 >= 0:
            d = min(d, abs(dot(n, sub(p, a))) / mp.sqrt(nn))
    return d
