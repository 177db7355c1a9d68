"""A float64 restatement of calculate_volume_from_sdf (CalcVolumeFromSDF.jl:26-125) and of the volume-preserving level
bisection of RBFs_smoothing (RBFs4Smoothing.jl:265-300, 359), helper of the tests.

What it pins, and how:
- The Gauss table is numpy's leggauss rounded to Float32 (`Float32.(...)`, :43-44); xi = (gp + 1) / 2, elvol = edge^3
  (left to right) and jac = elvol / 8 are Float32; the weight of point (iq, jq, kq) is gw[iq] * gw[jq] * gw[kq] * jac in
  Float32, left to right.  These are the very numbers the kernels add.
- Every decision is taken in Float32 exactly as the kernels take it (they are built without contraction): corners
  c = v - shift; a cell is outside if max(c) < iso, full if min(c) >= iso (min(c) = fl(min(v) - shift): the rounding of
  a subtraction is monotonic), else cut, and a Gauss point of a cut cell counts if the seven-lerp chain
  `a * (1 - x) + b * x` (x along x, then y, then z) is >= iso.  So the set of counted terms is the kernels' set.
- Only the order of the additions differs: here the sum is Float64.  Every term is >= 0, so the kernels' Float32 sum
  is within gamma(d) * V of V, gamma(d) = d u / (1 - d u), u = 2^-24, where d is the longest chain of Float32
  additions any one term passes through (volume_rowwave_kernel, volume_narrow_kernel, sum_f32_kernel in r2s_post.hip):
    * the Gauss points of a cut cell, per lane: order <= 9 takes the tensor form, lane e adds the n points of column e
      (and of e + 64 when n^2 > 64) -> n * ceil(n^2 / 64) <= 18 additions; order >= 10 takes one point after the other,
      point p to lane p mod 64 -> ceil(n^3 / 64) additions (512 at order 32);
    * the butterfly of the lanes' parts of a cut cell: 6;
    * the butterfly of a segment's 64 cell values (cfull64 / volume_cfull_kernel for a full segment: the same 6): 6;
    * the segments of a row, in x order (rowwave or narrow): nseg = ceil((nx - 1) / 64);
    * sum_f32_kernel: ceil(nrows / 1024) per thread, then a tree of 10.
  d = points + 22 + nseg + ceil(nrows / 1024); one more covers the Float64 sum here.  V = 0 has bound 0: no term
  means the exact 0.
- The bisection replays rbf_smooth_host (r2s_post.hip) step by step on the coarse LSF: lo, hi = min, max of the field,
  th = (lo + hi) / 2 in Float32, V(th) at order 9 with iso 0, eps = |target - V|, stop when eps <= 1e-4 or after
  40 levels, return -th.  A decision taken from V_ref is the product's too when V_ref is farther than the bound from
  the number it is compared with; each step says whether that holds.

Arrays are (z, y, x) with x fastest, like the library's.  NaN is not defined here.
"""
import numpy as np

U = 2.0 ** -24
F1, F2, F8 = np.float32(1), np.float32(2), np.float32(8)
TOL = 1.0e-4      # the bisection's stop tolerance (RBFs4Smoothing.jl:291)
MAX_LEVELS = 40


def tables(order, edge):
    """(xi, weights (kq, jq, iq), elvol) in Float32, as the kernels form them"""
    gp, gw = np.polynomial.legendre.leggauss(order)
    gp, gw = gp.astype(np.float32), gw.astype(np.float32)
    xi = (gp + F1) / F2
    e = np.float32(edge)
    elvol = e * e * e
    jac = elvol / F8
    w = ((gw[None, None, :] * gw[None, :, None]) * gw[:, None, None]) * jac
    return xi, w, elvol


def chain_length(order, nx, ny, nz):
    """d: the longest chain of Float32 additions a term passes through in the kernels (see the module docstring)"""
    n = order
    pts = n * -(-n * n // 64) if n <= 9 else -(-n ** 3 // 64)
    nseg = -(-(nx - 1) // 64)
    nrows = (ny - 1) * (nz - 1)
    return pts + 6 + 6 + nseg + -(-nrows // 1024) + 10


def _extrema(v):
    """the smallest / largest of the 8 corners of every cell, (nz-1, ny-1, nx-1)"""
    mn, mx = np.minimum(v[:, :, :-1], v[:, :, 1:]), np.maximum(v[:, :, :-1], v[:, :, 1:])
    mn, mx = np.minimum(mn[:, :-1], mn[:, 1:]), np.maximum(mx[:, :-1], mx[:, 1:])
    return np.minimum(mn[:-1], mn[1:]), np.maximum(mx[:-1], mx[1:])


def _cut_sum(v, k, j, i, shift, iso, xi, w):
    """the Float64 sum of the weights of the counted Gauss points of the cut cells (k, j, i)"""
    n = xi.size
    om = F1 - xi
    w64 = w.astype(np.float64).reshape(-1)
    iso = np.float32(iso)
    total = 0.0
    step = max(1, (1 << 21) // (n ** 3))
    for s in range(0, k.size, step):
        kk, jj, ii = k[s:s + step], j[s:s + step], i[s:s + step]

        def corner(dz, dy, dx):
            return (v[kk + dz, jj + dy, ii + dx] - shift)[:, None]
        # along x (n): c00 (y0 z0), c01 (y0 z1), c10 (y1 z0), c11 (y1 z1)
        c00 = corner(0, 0, 0) * om + corner(0, 0, 1) * xi
        c01 = corner(1, 0, 0) * om + corner(1, 0, 1) * xi
        c10 = corner(0, 1, 0) * om + corner(0, 1, 1) * xi
        c11 = corner(1, 1, 0) * om + corner(1, 1, 1) * xi
        # along y (jq, iq), then z (kq, jq, iq)
        c0 = c00[:, None, :] * om[:, None] + c10[:, None, :] * xi[:, None]
        c1 = c01[:, None, :] * om[:, None] + c11[:, None, :] * xi[:, None]
        p = c0[:, None] * om[:, None, None] + c1[:, None] * xi[:, None, None]
        assert p.dtype == np.float32
        total += float(((p >= iso).reshape(p.shape[0], -1).astype(np.float64) @ w64).sum())
    return total


def classify(values, shift=0.0, iso=0.0, zchunk=64):
    """(number of full cells, (k, j, i) of the cut cells) of {v - shift >= iso}"""
    v = np.asarray(values)
    assert v.dtype == np.float32 and v.ndim == 3 and min(v.shape) >= 2
    shift, iso = np.float32(shift), np.float32(iso)
    nfull, cut = 0, []
    for k0 in range(0, v.shape[0] - 1, zchunk):
        mn, mx = _extrema(v[k0:k0 + zchunk + 1])
        full = (mn - shift) >= iso
        c = ~full & ~((mx - shift) < iso)
        nfull += int(np.count_nonzero(full))
        kk, jj, ii = np.nonzero(c)
        cut.append((kk + k0, jj, ii))
    return nfull, tuple(np.concatenate([c[a] for c in cut]) for a in range(3))


def volume(values, edge, iso=0.0, order=9, shift=0.0):
    """(V_ref, bound): the volume of {v - shift >= iso} on the lattice of Float32 `values` (nz, ny, nx) with spacing
    `edge`, and the largest distance the kernels' Float32 sum may lie from it"""
    v = np.asarray(values)
    nz, ny, nx = v.shape
    xi, w, elvol = tables(order, edge)
    shift = np.float32(shift)
    nfull, (k, j, i) = classify(v, shift, iso)
    V = nfull * float(elvol) + _cut_sum(v, k, j, i, shift, iso, xi, w)
    d = chain_length(order, nx, ny, nz) + 1
    return V, d * U / (1.0 - d * U) * V


def coarse_edge(cx):
    """edge of the bisection: sqrt((cx[1] - cx[0])^2) in Float32 from the coarse x axis (rbf_smooth_host)"""
    d = np.float32(cx[1]) - np.float32(cx[0])
    return np.sqrt(np.float32(d * d))


def bisect(lsf, edge, target):
    """replay of the level bisection on the coarse LSF: (-th, steps); each step is a dict with the level th, the bracket
    (lo, hi) it was taken in, V_ref, bound, and whether the branch and the stop check are decided beyond the bound"""
    v = np.asarray(lsf)
    assert v.dtype == np.float32
    lo, hi = v.min(), v.max()
    eps, th, steps = 1.0, np.float32(0), []
    while len(steps) < MAX_LEVELS and eps > TOL:
        th = (lo + hi) / F2
        V, b = volume(v, edge, iso=0.0, order=9, shift=th)
        eps = abs(target - V)
        steps.append(dict(th=th, lo=lo, hi=hi, V=V, bound=b, branch_ok=eps > b, stop_ok=abs(eps - TOL) > b))
        if V > target:
            lo = th
        else:
            hi = th
    assert th.dtype == np.float32
    return -th, steps


def first_ambiguous(steps):
    """index of the first step whose branch or stop check the bound cannot decide (None: all decided)"""
    for s, st in enumerate(steps):
        if not (st["branch_ok"] and st["stop_ok"]):
            return s
    return None


def serial_bound(nterms, V):
    """the bound of a serial Float32 sum of `nterms` terms >= 0 with total V (the oracle's order)"""
    return nterms * U / (1.0 - nterms * U) * V

