"""float64 restatement of the ray query of include/rho2sdf_hip.h (r2s_mesh_index_raycast) in plain numpy operations, brute
force over all triangles, and the same pair test in mpmath at 50 digits in exact geometry (no shear rounding), for
tests/test_ray_*.py.

Definition (the header has the full text): the watertight pair test of Woop, Benthin and Wald (2013) in float64, every
operation rounded on its own; a pair is a hit only if its t also lies in the ray's parameter interval through the triangle's
float32 box inflated by m = 2^-40 max(|o|, absmax of the vertices), intersected with [t_min, t_max]; the result is the
lexicographic minimum of (t, triangle index) over the accepted pairs, side = the sign of det.

MEASURED_RATIO (tests/test_ray_cpu.py::test_restatement_against_mpmath prints it as "RAY K ..."): the largest
|t_ref - t_mp| |d| / (2^-52 L) over the decidable pairs of that test, L the largest absolute coordinate of the case.
GRAZING_COS: the largest |cos| of the incidence angle at which a pair that exact geometry accepts was lost to the in-box
condition on that set (0.0: no such pair; GRAZING_FLATTEST is the flattest incidence the set holds)."""
import numpy as np

MEASURED_RATIO = 283.5      # (a far origin at 10^3 box sizes, near the silhouette)
GRAZING_COS = 0.0           # no decidable pair of the set was lost
GRAZING_FLATTEST = 1.1e-11  # the flattest decided hit of the set
EPS = 2.0 ** -52
INF = np.inf


def _frames(d):
    """-> (kx, ky, kz) per ray: kz the axis of the largest |d| (lowest on ties), kx, ky the next two, swapped for d[kz] < 0"""
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


def bad_rays(o, d):
    return ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0.0).any(axis=1))


def slab(blo, bhi, o, d, inv, m, t_min, t_max):
    """parameter intervals of rays (n, 3) through the boxes (nt, 3) inflated by m (n,) -> lo, hi (n, nt)"""
    lo = np.full((len(o), len(blo)), float(t_min))
    hi = np.full((len(o), len(blo)), float(t_max))
    for k in range(3):
        l = blo[None, :, k] - m[:, None]
        h = bhi[None, :, k] + m[:, None]
        ok = o[:, k, None]
        t1, t2 = (l - ok) * inv[:, k, None], (h - ok) * inv[:, k, None]
        nz = (d[:, k] != 0.0)[:, None]
        inside = (l <= ok) & (ok <= h)
        lo = np.where(nz, np.fmax(lo, np.fmin(t1, t2)), np.where(inside, lo, INF))
        hi = np.where(nz, np.fmin(hi, np.fmax(t1, t2)), np.where(inside, hi, -INF))
    return lo, hi


def _pairs(Vt, o, d, kx, ky, kz):
    """rays of ONE frame (kx, ky, kz scalars) against the triangles Vt (nt, 3 corners, 3 axes) -> U, V, W, det, t (n, nt)"""
    dz = d[:, kz]
    Sx, Sy, Sz = (d[:, kx] / dz)[:, None], (d[:, ky] / dz)[:, None], (1.0 / dz)[:, None]
    sh = []
    for c in range(3):
        z = Vt[None, :, c, kz] - o[:, kz, None]
        x = (Vt[None, :, c, kx] - o[:, kx, None]) - Sx * z
        y = (Vt[None, :, c, ky] - o[:, ky, None]) - Sy * z
        sh.append((x, y, z))
    (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sh
    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
    det = (U + V) + W
    t = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det
    return U, V, W, det, t


def pair_table(verts, tris, origins, dirs, t_min=0.0, t_max=INF):
    """every ray against every triangle -> (accepted (n, nt) bool, t (n, nt), det (n, nt)); bad rays accept nothing"""
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    return _pair_table_with_absmax(verts, T, o, d, t_min, t_max, float(np.abs(v[T]).max()) if len(T) else 0.0)


def raycast_brute(verts, tris, origins, dirs, t_min=0.0, t_max=INF, budget=1_500_000):
    """-> (t (n,) float64, tri (n,) int32, side (n,) int8): the definition over ALL triangles, in chunks of triangles"""
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    n, nt = len(o), len(T)
    best, idx, side = np.full(n, INF), np.full(n, -1, np.int32), np.zeros(n, np.int8)
    step = max(1, budget // max(n, 1))
    rows = np.arange(n)
    absmax_all = float(np.abs(np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)[T]).max()) if nt else 0.0
    for t0 in range(0, nt, step):
        sel = T[t0:t0 + step]
        acc, t, det = _pair_table_with_absmax(verts, sel, o, d, t_min, t_max, absmax_all)
        tm = np.where(acc, t, INF)
        m = tm.min(axis=1)
        j = (acc & (t == m[:, None])).argmax(axis=1)         # the first accepted index that attains the minimum
        hit = acc[rows, j]
        better = hit & ((idx < 0) | (t[rows, j] < best))     # (strict: earlier chunks hold the smaller indices)
        best[better] = t[rows, j][better]
        idx[better] = (t0 + j[better]).astype(np.int32)
        side[better] = np.where(det[rows, j][better] > 0.0, 1, -1).astype(np.int8)
    best = best + 0.0                                        # (-0 -> +0, as the header says)
    best[bad_rays(o, d)] = np.nan
    return best, idx, side


def _pair_table_with_absmax(verts, tris, o, d, t_min, t_max, absmax):
    """pair_table for a chunk of the triangles with the margin of the whole mesh"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    n, nt = len(o), len(T)
    acc, tt, dd = np.zeros((n, nt), bool), np.full((n, nt), np.nan), np.zeros((n, nt))
    good = np.nonzero(~bad_rays(o, d))[0]
    if nt == 0 or len(good) == 0:
        return acc, tt, dd
    Vt = v[T]
    blo, bhi = Vt.min(axis=1), Vt.max(axis=1)
    og, dg = o[good], d[good]
    with np.errstate(all="ignore"):
        inv = np.where(dg != 0.0, 1.0 / np.where(dg != 0.0, dg, 1.0), 0.0)
        m = np.ldexp(np.maximum(np.abs(og).max(axis=1), absmax), -40)
        lo, hi = slab(blo, bhi, og, dg, inv, m, t_min, t_max)
        kx, ky, kz = _frames(dg)
        for fx, fy, fz in sorted({(int(a), int(b), int(c)) for a, b, c in zip(kx, ky, kz)}):
            s = np.nonzero((kx == fx) & (ky == fy) & (kz == fz))[0]
            U, V, W, det, t = _pairs(Vt, og[s], dg[s], fx, fy, fz)
            mixed = ((U < 0.0) | (V < 0.0) | (W < 0.0)) & ((U > 0.0) | (V > 0.0) | (W > 0.0))
            a = ~mixed & (det != 0.0) & (t >= lo[s]) & (t <= hi[s])
            acc[good[s]], tt[good[s]], dd[good[s]] = a, t, det
    return acc, tt, dd


def pair_mp(o, d, a, b, c, digits=50):
    """the pair test in exact geometry (mpmath, `digits` digits, the sheared frame of the definition without its roundings)
    -> dict(hit (edge rule and det != 0, no window), t, edges (U, V, W scaled by 1 / R^2), cos (of the incidence angle),
    R (the largest |vertex - origin| component))"""
    import mpmath as mp
    mp.mp.dps = digits
    f = lambda v: [mp.mpf(float(x)) for x in v]   # noqa: E731
    o, d, a, b, c = f(o), f(d), f(a), f(b), f(c)
    kz = max(range(3), key=lambda k: (abs(d[k]), -k))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    if d[kz] < 0:
        kx, ky = ky, kx
    Sx, Sy, Sz = d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
    P = [[p[k] - o[k] for k in range(3)] for p in (a, b, c)]
    (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = [(p[kx] - Sx * p[kz], p[ky] - Sy * p[kz], p[kz]) for p in P]
    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
    det = U + V + W
    mixed = min(U, V, W) < 0 and max(U, V, W) > 0
    hit = (not mixed) and det != 0
    t = (U * Sz * Az + V * Sz * Bz + W * Sz * Cz) / det if det != 0 else mp.nan
    ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
    nn, dn = mp.sqrt(sum(x * x for x in n)), mp.sqrt(sum(x * x for x in d))
    cos = abs(sum(n[k] * d[k] for k in range(3))) / (nn * dn) if nn > 0 else mp.mpf(0)
    R = max(abs(x) for p in P for x in p)
    s = R * R if R > 0 else mp.mpf(1)
    return dict(hit=hit, t=t, edges=(U / s, V / s, W / s), det=det, cos=cos, R=R, dnorm=dn)
