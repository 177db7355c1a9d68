"""A float64 restatement of the second derivatives of the smoothed level-set and of the curvature of its level sets (helper of
the tests), on top of field_ref64.Field; it shares no code with the library.

    H_ab(p) = sum_j w_j k_j (4 d_a d_b / sigma^4 - 2 delta_ab / sigma^2),   d = p - x_j,  k_j = exp(-(|d| / sigma)^2)

- which nodes take part (candidates, Float32 distance, support test, knn cap with the (distance, node index) rule, ties) is
  decided by Field._chunk and by nothing else: hessian() runs Field._chunk itself and reads the arrays it worked with
  (`take`, the Float32 differences `d`, the contributions `c = w k` of the nodes taken) from its frame when it returns, so
  there is no second copy of those rules that could drift.  The value and gradient _chunk returns are handed on unchanged.
- cutoff=False is the smooth function for differentiation: the same nodes and closed forms in float64 throughout (hessian()).
- H in Float64 from the same Float32 differences the gradient uses; S_ab = sum |w k| (4 |d_a d_b| / sigma^4 +
  2 delta_ab / sigma^2): the sum of the magnitudes of what is added.  Components in the order xx, yy, zz, xy, xz, yz.
- non-finite point: NaN.  No node in reach: H = 0.

hess_bound, derived like Field.grad_bound.  An implementation that follows the header forms the same Float32 differences
d_a exactly, sums in Float64 (its round-off, ~m 2^-53 S_ab, is far below one unit of the constant) and rounds each
component to Float32 once (2^-24 |H_ab|, stated as 2^-23).  What differs between two correct implementations is k_j alone:
the Float32 distance and another exp() change exp(-u^2) by <= 6 ln(1/thr) 2^-24 relative, with the same allowance of 12
units of 2^-24 for the exp and the products that grad_bound makes; every term of H_ab carries k_j once, so the sum of
magnitudes S_ab multiplies it.  A node at the very edge of the support (slack = thr sum |w|) may take part or not; it adds
at most thr |w| (4 R^2 + 2) / sigma^2 to any component (|d_a d_b| <= R^2 sigma^2).  Hence

    hess_bound = (6 ln(1/thr) + 12) 2^-24 S_ab + 2^-23 |H_ab| + slack (4 R^2 + 2) / sigma^2

curvature(g32, H32): the header's formulas in numpy float64 on Float32 gradients and Hessians (the discriminant's
cancelling numerator in double-double, see curvature64).
"""
import math
import sys

import numpy as np

from field_ref64 import Field

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # xx, yy, zz, xy, xz, yz
HESS_C = 12.0


def _chunk_with_locals(fld, p, cutoff):
    """Field._chunk(p, cutoff) and the local variables it held when it returned"""
    code = Field._chunk.__code__
    seen = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is code:
            seen.update(frame.f_locals)

    old = sys.getprofile()
    sys.setprofile(prof)
    try:
        out = fld._chunk(p, cutoff)
    finally:
        sys.setprofile(old)
    assert {"take", "d", "c", "ac", "n", "idx", "wv"} <= set(seen), "Field._chunk no longer has the arrays the Hessian is built from"
    return out, seen


def _sums(fld, c, ac, d):
    """H and S_ab (n, 6) and the gradient (n, 3) from the contributions c = w k (0 where a node does not take part),
    ac = |c| and the per-axis differences d, all (n, K) / (n, K, K, K) float64 in _chunk's (n, z, y, x) layout: the one
    place where the closed forms are written down, whichever arithmetic produced c and d"""
    n = len(c)
    db = (d[0][:, None, None, :], d[1][:, None, :, None], d[2][:, :, None, None])
    s2 = fld.sigma * fld.sigma
    sv, sa = c.reshape(n, -1).sum(1), ac.reshape(n, -1).sum(1)
    H, S = np.zeros((n, 6)), np.zeros((n, 6))
    for k, (a, b) in enumerate(PAIRS):
        dd = db[a] * db[b]
        H[:, k] = 4.0 / (s2 * s2) * (c * dd).reshape(n, -1).sum(1)
        S[:, k] = 4.0 / (s2 * s2) * (ac * np.abs(dd)).reshape(n, -1).sum(1)
        if a == b:
            H[:, k] -= 2.0 / s2 * sv
            S[:, k] += 2.0 / s2 * sa
    grad = np.stack([-2.0 / s2 * (c * db[a]).reshape(n, -1).sum(1) for a in range(3)], axis=1)
    return H, S, grad, sv


def _hess_chunk(fld, p, cutoff, float64_steps):
    out, loc = _chunk_with_locals(fld, p.astype(np.float32), cutoff)
    n, take, c, ac = loc["n"], loc["take"], loc["c"], loc["ac"]
    assert np.array_equal(take.reshape(n, -1).sum(1), out["m"]) and not c[~take].any()
    assert all(x.dtype == np.float32 for x in loc["d"])
    out = dict(out)
    if not float64_steps:
        H, S, grad, _ = _sums(fld, c, ac, [x.astype(np.float64) for x in loc["d"]])
        assert np.array_equal(grad, out["grad"])                                       # _chunk's own gradient, bit for bit
    else:
        # the nodes _chunk took, but differences, distance and exp from the float64 point: no Float32 step anywhere
        d = [p[:, a].astype(np.float64)[:, None] - fld.axes[a].astype(np.float64)[loc["idx"][a]] for a in range(3)]
        r2 = (d[0] * d[0])[:, None, None, :] + (d[1] * d[1])[:, None, :, None] + (d[2] * d[2])[:, :, None, None]
        c = np.where(take, loc["wv"] * np.exp(-r2 / (fld.sigma * fld.sigma)), 0.0)
        H, S, grad, sv = _sums(fld, c, np.abs(c), d)
        out["grad"], out["val"] = grad, sv + float(fld.th)
    out["H"], out["Sab"] = H, S
    return out


def hessian(fld, points, cutoff=True, chunk=None, float64_steps=None):
    """-> Field.evaluate's dict (val, grad, m, S, Sa, slack, capped, tie) + H (n, 6) and Sab (n, 6), float64.
    cutoff=True: the evaluation the header describes, with Field._chunk's Float32 differences and distances; val and grad
    are Field.evaluate's.
    cutoff=False (float64_steps defaults to True): the smooth function, there to be differentiated.  Field._chunk still
    names the nodes (every in-bounds candidate of the box of the Float32-rounded point), but points may be float64 and the
    differences, the distance and exp are formed in float64, and val / grad come from the same float64 terms as H.  A
    function whose distances are rounded to Float32 cannot be differenced over 1e-4 cell: the 2^-24 of k_j divided by the
    step is ~1e-3 of the derivative.  float64_steps=False keeps _chunk's Float32 steps with the cutoff off."""
    float64_steps = (not cutoff) if float64_steps is None else float64_steps
    assert not (cutoff and float64_steps), "the support test is defined on the Float32 distance"
    p = np.asarray(points, dtype=np.float64 if float64_steps else np.float32).reshape(-1, 3)
    n = len(p)
    out = dict(val=np.full(n, np.nan), grad=np.full((n, 3), np.nan), m=np.zeros(n, np.int32), S=np.zeros(n), Sa=np.zeros((n, 3)),
               slack=np.zeros(n), capped=np.zeros(n, bool), tie=np.zeros(n, bool), H=np.full((n, 6), np.nan), Sab=np.zeros((n, 6)))
    K = 2 * fld.B + 2
    chunk = chunk or max(1, (1 << 21) // K ** 3)
    fin = np.flatnonzero(np.isfinite(p).all(1))
    for s in range(0, len(fin), chunk):
        ids = fin[s:s + chunk]
        r = _hess_chunk(fld, p[ids], cutoff, float64_steps)
        for k, v in r.items():
            out[k][ids] = v
    return out


class HessField(Field):
    """field_ref64.Field with hessian(points, cutoff=True) and hess_bound(ref)"""

    def hessian(self, points, cutoff=True, chunk=None, float64_steps=None):
        return hessian(self, points, cutoff, chunk, float64_steps)

    def hess_bound(self, ref):
        return hess_bound(self, ref)


def hess_bound(fld, ref):
    """(n, 6), module docstring"""
    s2 = fld.sigma * fld.sigma
    return ((6.0 * math.log(1.0 / fld.thr) + HESS_C) * 2.0 ** -24 * ref["Sab"] + 2.0 ** -23 * np.abs(ref["H"])
            + (ref["slack"] * (4.0 * fld.R * fld.R + 2.0) / s2)[:, None])


def curvature(g32, H32):
    """the header's formulas on Float32 gradients (n, 3) and Hessians (n, 6) -> dict(mean, gauss, k1, k2, g2, hnorm) in
    float64; NaN where g2 is 0 or not finite.  hnorm is the Frobenius norm of the full symmetric matrix."""
    g = np.asarray(g32, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    h = np.asarray(H32, dtype=np.float32).astype(np.float64).reshape(-1, 6)
    return curvature64(g, h)


class _DD:
    """a + b, a - b, a * b on unevaluated sums hi + lo of two float64 arrays (Dekker / Knuth error-free transformations):
    about 100 significant bits, enough to form the discriminant below without the cancellation of its float64 evaluation"""

    def __init__(self, hi, lo=None):
        self.hi = np.asarray(hi, dtype=np.float64)
        self.lo = np.zeros_like(self.hi) if lo is None else lo

    @staticmethod
    def _two_sum(a, b):
        s = a + b
        bb = s - a
        return s, (a - (s - bb)) + (b - bb)

    @staticmethod
    def _split(a):
        c = 134217729.0 * a
        hi = c - (c - a)
        return hi, a - hi

    def __add__(self, o):
        s, e = self._two_sum(self.hi, o.hi)
        e = e + (self.lo + o.lo)
        hi = s + e
        return _DD(hi, e - (hi - s))

    def __neg__(self):
        return _DD(-self.hi, -self.lo)

    def __sub__(self, o):
        return self + (-o)

    def __mul__(self, o):
        p = self.hi * o.hi
        ah, al = self._split(self.hi)
        bh, bl = self._split(o.hi)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        e = e + (self.hi * o.lo + self.lo * o.hi)
        hi = p + e
        return _DD(hi, e - (hi - p))


def _forms(gx, gy, gz, hxx, hyy, hzz, hxy, hxz, hyz):
    """g2, A = g2 tr(H) - g^T H g, B = g^T adj(H) g, with whatever arithmetic the arguments bring"""
    g2 = gx * gx + gy * gy + gz * gz
    ghg = gx * (hxx * gx + hxy * gy + hxz * gz) + gy * (hxy * gx + hyy * gy + hyz * gz) + gz * (hxz * gx + hyz * gy + hzz * gz)
    axx, ayy, azz = hyy * hzz - hyz * hyz, hxx * hzz - hxz * hxz, hxx * hyy - hxy * hxy
    axy, axz, ayz = hxz * hyz - hxy * hzz, hxy * hyz - hxz * hyy, hxy * hxz - hxx * hyz
    gag = gx * (axx * gx + axy * gy + axz * gz) + gy * (axy * gx + ayy * gy + ayz * gz) + gz * (axz * gx + ayz * gy + azz * gz)
    return g2, g2 * (hxx + hyy + hzz) - ghg, gag


def curvature64(g, h):
    """the same formulas on float64 arrays as they are.  mean and gauss are evaluated in float64 as written.  The
    discriminant mean^2 - gauss = (A^2 - 4 g2 B) / (4 g2^3) vanishes at umbilic points, where its float64 evaluation keeps
    only round-off and the square root would turn 1e-16 into 1e-8: its numerator is formed in double-double, so k1 and k2
    are as exact as mean and gauss are"""
    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    h = np.asarray(h, dtype=np.float64).reshape(-1, 6)
    cols = list(g.T) + list(h.T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g2, A, B = _forms(*cols)
        ok = (g2 > 0) & np.isfinite(g2)
        mean = -A / (2.0 * g2 * np.sqrt(g2))
        gauss = B / (g2 * g2)
        dg2, dA, dB = _forms(*[_DD(c) for c in cols])
        four = _DD(np.full(len(g), 4.0))
        num = dA * dA - four * dg2 * dB
        root = np.sqrt(np.maximum(num.hi + num.lo, 0.0) / (4.0 * g2 * g2 * g2))
        k1, k2 = mean + root, mean - root
        hxx, hyy, hzz, hxy, hxz, hyz = h.T
        hnorm = np.sqrt(hxx * hxx + hyy * hyy + hzz * hzz + 2.0 * (hxy * hxy + hxz * hxz + hyz * hyz))
    nan = np.full(len(g), np.nan)
    return dict(mean=np.where(ok, mean, nan), gauss=np.where(ok, gauss, nan), k1=np.where(ok, k1, nan), k2=np.where(ok, k2, nan),
                g2=g2, hnorm=hnorm)
