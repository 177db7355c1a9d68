"""A float64 restatement of RBF smoothing, written from the reference's RBFs4Smoothing.jl (helper of the tests).

What it pins, and how:
- process_vector (:15-22) in Float32 with `isapprox` semantics (rtol = sqrt(eps(Float32)), atol = 0).
- create_grid (:36-46): every node of the Float32 `range` is computed in Float64 and rounded once;
  create_smooth_grid (:60-74): a Float32 step from the x axis, `xmin + (i - 1) * dx` in Float32 on every axis.
- rbf_interpolation_kdtree (:219-248): knn(kdtree, p, 124) then `dist <= max_distance`.  The candidates are the
  in-bounds coarse nodes of a box of +-(ceil(R) + 1) cells around the target, ordered by (lattice distance^2, dz, dy,
  dx) - the reference leaves the order of equal distances open; this is the product's documented tie order.  The first
  124 of them are kept, then those within the support.  Distances are Float32 as in the reference; the kernel values
  and the sum are Float64.  Per target the result carries the number of taps m, S = sum |w k| (the scale of the
  Float32 accumulation error) and the lattice distance^2 of a tie between the 124th and the 125th node inside the
  support (-1 where there is none): where such a tie exists, the reference's result is not unique.
- compute_sparse_kernel_matrix (:142-176): Float32 entries `> threshold`, no cap.

Every evaluation asserts its precondition: no candidate distance lies within 1e-5 (relative) of max_distance, so that
the rounding of Float32 distances cannot change which nodes take part.

Arrays are (z, y, x) with x fastest, like the library's.
"""
import math

import numpy as np

KNN = 124
RTOL32 = np.float32(math.sqrt(float(np.finfo(np.float32).eps)))   # sqrt(eps(Float32))
SENTINEL = np.float32(1.0e10)


def process_vector(vec):
    """Float32.(vec); values isapprox 1f10 in magnitude -> sign * (largest |value| below 1f9)"""
    v = np.asarray(vec, dtype=np.float64).astype(np.float32)
    a = np.abs(v)
    real = a[a < np.float32(1.0e9)]
    if real.size == 0:
        raise ValueError("every value is a sentinel")   # `maximum` of an empty collection throws
    mx = real.max()
    with np.errstate(invalid="ignore"):
        near = np.isfinite(a) & (np.abs(a - SENTINEL) <= RTOL32 * np.maximum(a, SENTINEL))
    return np.where(near, np.sign(v) * mx, v).astype(np.float32)


def coarse_axis(lo, hi, n):
    """one axis of create_grid: range(Float32(lo), Float32(hi), length=n)"""
    a, b = float(np.float32(lo)), float(np.float32(hi))
    x = np.array([a + i * (b - a) / (n - 1) for i in range(n)], dtype=np.float64).astype(np.float32)
    x[-1] = np.float32(hi)
    return x


def fine_axes(aabb_min, aabb_max, N, smooth):
    """create_smooth_grid: three Float32 axes with the step of the x axis"""
    f = [int(n) * smooth + 1 for n in N]
    xmin, xmax = np.float32(aabb_min[0]), np.float32(aabb_max[0])
    dx = (xmax - xmin) / np.float32(f[0] - 1)
    return [np.float32(aabb_min[a]) + np.arange(f[a], dtype=np.float32) * dx for a in range(3)]


def coarse_axes(aabb_min, aabb_max, N):
    return [coarse_axis(aabb_min[a], aabb_max[a], int(N[a]) + 1) for a in range(3)]


def max_distance(sigma, thr):
    return np.float32(math.sqrt(-math.log(thr) * sigma * sigma))


def _class_offsets(s, frac, R):
    """box offsets of a target with sub-index frac, in (lattice d^2, dz, dy, dx) order; offsets beyond 1.05 R cannot
    lie in the support nor precede a node that does, and are left out"""
    B = math.ceil(R) + 1
    r = np.arange(-B, B + 1)
    dz, dy, dx = [a.ravel() for a in np.meshgrid(r, r, r, indexing="ij")]
    d2 = (dx * s - frac[0]) ** 2 + (dy * s - frac[1]) ** 2 + (dz * s - frac[2]) ** 2
    keep = d2 <= 1.05 * R * R * s * s
    order = np.lexsort((dx[keep], dy[keep], dz[keep], d2[keep]))
    return d2[keep][order], dz[keep][order], dy[keep][order], dx[keep][order]


def evaluate(w, caxes, taxes, s, sigma, thr):
    """rbf_interpolation_kdtree(targets, coarse grid, w, kernel) -> dict(val, m, S, tie_d2), arrays (tz, ty, tx).
    Target (i, j, k) lies at coarse index (i, j, k) / s: base node (i // s, ...) plus sub-index (i % s, ...).
    w may carry a leading batch axis (several weight fields at once); val and S then carry it too."""
    w = np.asarray(w, dtype=np.float32)
    if w.ndim == 4:
        return _evaluate(w, caxes, taxes, s, sigma, thr)
    r = _evaluate(w[None], caxes, taxes, s, sigma, thr)
    return dict(val=r["val"][0], m=r["m"], S=r["S"][0], tie_d2=r["tie_d2"])


def _evaluate(w, caxes, taxes, s, sigma, thr):
    cx, cy, cz = caxes
    tx, ty, tz = taxes
    nb, nz, ny, nx = w.shape
    assert (nx, ny, nz) == (cx.size, cy.size, cz.size)
    R = math.sqrt(-math.log(thr))
    maxd = max_distance(sigma, thr)
    shape = (tz.size, ty.size, tx.size)
    val = np.zeros((nb,) + shape)
    S = np.zeros((nb,) + shape)
    m = np.zeros(shape, dtype=np.int32)
    tie = np.full(shape, -1, dtype=np.int64)
    w64 = w.astype(np.float64)
    for fz in range(s):
        for fy in range(s):
            for fx in range(s):
                ti, tj, tk = np.arange(fx, tx.size, s), np.arange(fy, ty.size, s), np.arange(fz, tz.size, s)
                if not (ti.size and tj.size and tk.size):
                    continue
                bi, bj, bk = ti // s, tj // s, tk // s
                sub = (slice(fz, None, s), slice(fy, None, s), slice(fx, None, s))
                cshape = (tk.size, tj.size, ti.size)
                rank = np.zeros(cshape, dtype=np.int32)
                v, a, mm = np.zeros((nb,) + cshape), np.zeros((nb,) + cshape), np.zeros(cshape, dtype=np.int32)
                d2_at = {KNN: np.full(cshape, -1, dtype=np.int64), KNN + 1: np.full(cshape, -1, dtype=np.int64)}
                in_at = np.zeros(cshape, dtype=bool)
                for d2, dz, dy, dx in zip(*_class_offsets(s, (fx, fy, fz), R)):
                    ci, cj, ck = bi + dx, bj + dy, bk + dz
                    oi, oj, ok = (ci >= 0) & (ci < nx), (cj >= 0) & (cj < ny), (ck >= 0) & (ck < nz)
                    if not (oi.any() and oj.any() and ok.any()):
                        continue
                    inb = ok[:, None, None] & oj[None, :, None] & oi[None, None, :]
                    rank += inb
                    ci, cj, ck = np.clip(ci, 0, nx - 1), np.clip(cj, 0, ny - 1), np.clip(ck, 0, nz - 1)
                    ex, ey, ez = tx[ti] - cx[ci], ty[tj] - cy[cj], tz[tk] - cz[ck]   # Float32 differences
                    dist = np.sqrt((ex * ex)[None, None, :] + (ey * ey)[None, :, None] + (ez * ez)[:, None, None])
                    assert dist.dtype == np.float32
                    near = inb & (np.abs(dist.astype(np.float64) - float(maxd)) <= 1e-5 * float(maxd))
                    assert not near.any(), "precondition: a candidate distance lies within 1e-5 of max_distance"
                    inside = inb & (dist <= maxd)
                    for r in (KNN, KNN + 1):
                        hit = inb & (rank == r)
                        d2_at[r][hit] = d2
                        if r == KNN:
                            in_at |= hit & inside
                    take = inside & (rank <= KNN)
                    u = dist.astype(np.float64) / sigma
                    c = w64[(slice(None),) + np.ix_(ck, cj, ci)] * np.exp(-(u * u))[None]
                    v += np.where(take[None], c, 0.0)
                    a += np.where(take[None], np.abs(c), 0.0)
                    mm += take
                val[(slice(None),) + sub], S[(slice(None),) + sub], m[sub] = v, a, mm
                tie[sub] = np.where(in_at & (d2_at[KNN] == d2_at[KNN + 1]), d2_at[KNN], -1)
    return dict(val=val, m=m, S=S, tie_d2=tie)


def kernel_matrix(caxes, sigma, thr):
    """compute_sparse_kernel_matrix on the coarse lattice: scipy CSR, Float32 entries > thr (no cap)"""
    import scipy.sparse as sp
    cx, cy, cz = caxes
    nx, ny, nz = cx.size, cy.size, cz.size
    n = nx * ny * nz
    rr = int(math.floor(math.sqrt(-math.log(thr) * 1.05))) + 1
    idx = np.arange(n).reshape(nz, ny, nx)
    rows, cols, vals = [], [], []
    for dz in range(-rr, rr + 1):
        for dy in range(-rr, rr + 1):
            for dx in range(-rr, rr + 1):
                k0, k1 = max(0, -dz), min(nz, nz - dz)
                j0, j1 = max(0, -dy), min(ny, ny - dy)
                i0, i1 = max(0, -dx), min(nx, nx - dx)
                if k1 <= k0 or j1 <= j0 or i1 <= i0:
                    continue
                ex = cx[i0:i1] - cx[i0 + dx:i1 + dx]
                ey = cy[j0:j1] - cy[j0 + dy:j1 + dy]
                ez = cz[k0:k1] - cz[k0 + dz:k1 + dz]
                r = np.sqrt((ex * ex)[None, None, :] + (ey * ey)[None, :, None] + (ez * ez)[:, None, None])
                u = r.astype(np.float64) / sigma
                k = np.exp(-(u * u))
                k32 = np.where(k > thr, k, 0.0).astype(np.float32)
                keep = k32 > thr
                if not keep.any():
                    continue
                rows.append(idx[k0:k1, j0:j1, i0:i1][keep])
                cols.append(idx[k0 + dz:k1 + dz, j0 + dy:j1 + dy, i0 + dx:i1 + dx][keep])
                vals.append(k32[keep])
    return sp.csr_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(n, n))


def bound(ref, thr):
    """|kernel - ref| allowed per target: m Float32 roundings of the accumulator (each <= 2^-24 S) plus the change of
    exp(-u^2) that the rounding of a Float32 distance and a different exp() can cause"""
    return (ref["m"] + 6.0 * math.log(1.0 / thr) + 8.0) * 2.0 ** -24 * ref["S"]


def fine_bound(ref, th, thr):
    """the same for the output field `fine + th` (one more Float32 rounding of the sum)"""
    return bound(ref, thr) + 2.0 ** -23 * (np.abs(ref["val"]) + abs(float(th)))
