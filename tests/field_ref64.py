"""A float64 restatement of the point evaluation of the smoothed level-set (helper of the tests), written from the
reference's RBFs4Smoothing.jl (:219-248, :366) and the evaluation rules in include/rho2sdf_hip.h; it shares no code with
the library.

    f(p) = th + sum_j w_j exp(-(|p - x_j| / sigma)^2)

- geometry: rbf_ref64.coarse_axes (Float32 `range` of create_grid), sigma = cell_size, rbf_ref64.max_distance.
- candidates of a point: the in-bounds coarse nodes of a box of ceil(R) + 1 cells to either side of the point's cell
  (nodes cell - B .. cell + 1 + B per axis), R = sqrt(-ln thr); the cell is floor((p - aabb_min) / cell_size) in double.
  The box reaches at least two cells beyond the support, so the lookup never decides membership.
- dist = sqrt((dx*dx + dy*dy) + dz*dz) in Float32, every operation rounded separately; a node takes part when
  dist <= max_distance.
- knn cap: more than 124 such nodes -> the 124 smallest by (dist, linear node index); `tie` marks points where the 124th
  and 125th distances are equal: the reference's own result is not unique there, the index rule is the library's
  documented choice.
- value and gradient in Float64; per point also m, S = sum |w k|, S_a = sum |w k| 2 |p_a - x_a| / sigma^2 and
  slack = thr * sum |w_j| over in-bounds candidates whose Float32 distance lies within 1e-5 (relative) of max_distance:
  such a node may fall on either side in another implementation's arithmetic, so it widens the bound.
- cutoff=False: every in-bounds candidate of the box takes part (no support test, no cap): a smooth function, used to
  check the gradient against central differences.
- non-finite point: val and grad NaN, m 0.  No node in reach: val th, grad 0.

project() restates the projection of the header step for step, with Float32 value / gradient / coordinates.
"""
import math

import numpy as np

import rbf_ref64 as R64

KNN = 124


class Field:
    def __init__(self, w, aabb_min, aabb_max, N, cell_size, thr, th=0.0):
        self.N = [int(n) for n in N]
        self.nx, self.ny, self.nz = [n + 1 for n in self.N]
        self.w = np.asarray(w, dtype=np.float32).reshape(self.nz, self.ny, self.nx).astype(np.float64)
        self.amin = np.asarray(aabb_min, dtype=np.float64)
        self.h = float(cell_size)
        self.sigma = float(cell_size)
        self.thr = float(thr)
        self.th = np.float32(th)
        self.axes = R64.coarse_axes(aabb_min, aabb_max, self.N)
        self.maxd = R64.max_distance(self.sigma, self.thr)
        self.R = math.sqrt(-math.log(self.thr))
        self.B = math.ceil(self.R) + 1

    def evaluate(self, points, cutoff=True, chunk=None):
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        out = dict(val=np.full(n, np.nan), grad=np.full((n, 3), np.nan), m=np.zeros(n, np.int32), S=np.zeros(n),
                   Sa=np.zeros((n, 3)), slack=np.zeros(n), capped=np.zeros(n, bool), tie=np.zeros(n, bool))
        K = 2 * self.B + 2
        chunk = chunk or max(1, (1 << 21) // K ** 3)
        fin = np.flatnonzero(np.isfinite(p).all(1))
        for s in range(0, len(fin), chunk):
            ids = fin[s:s + chunk]
            r = self._chunk(p[ids], cutoff)
            for k, v in r.items():
                out[k][ids] = v
        return out

    def _chunk(self, p, cutoff):
        n = len(p)
        offs = np.arange(-self.B, self.B + 2)
        K = offs.size
        dims = (self.nx, self.ny, self.nz)
        d, inb, idx = [], [], []
        for a in range(3):
            cell = np.floor((p[:, a].astype(np.float64) - self.amin[a]) / self.h)
            cell = np.clip(cell, -4.0 * K, dims[a] + 4.0 * K).astype(np.int64)   # (far points: an empty box either way)
            ia = cell[:, None] + offs[None, :]
            ok = (ia >= 0) & (ia < dims[a])
            ia = np.clip(ia, 0, dims[a] - 1)
            da = p[:, a][:, None] - self.axes[a][ia]
            assert da.dtype == np.float32
            d.append(da), inb.append(ok), idx.append(ia)
        with np.errstate(over="ignore"):   # (a point at 1e30: the Float32 squares overflow to inf, as in any Float32 evaluation)
            sq = [x * x for x in d]
            dist = np.sqrt((sq[0][:, None, None, :] + sq[1][:, None, :, None]) + sq[2][:, :, None, None])
        assert dist.dtype == np.float32
        ok = inb[2][:, :, None, None] & inb[1][:, None, :, None] & inb[0][:, None, None, :]
        lin = (idx[2][:, :, None, None] * self.ny + idx[1][:, None, :, None]) * self.nx + idx[0][:, None, None, :]
        wv = self.w.ravel()[lin]
        maxd = float(self.maxd)
        d64 = dist.astype(np.float64)
        capped = np.zeros(n, bool)
        tie = np.zeros(n, bool)
        if cutoff:
            take = ok & (dist <= self.maxd)
            cnt = take.reshape(n, -1).sum(1)
            capped = cnt > KNN
            if capped.any():
                c = np.flatnonzero(capped)
                # the flat (z, y, x) order of one box is the order of the linear node index: a stable sort by distance
                # breaks equal distances by it
                dm = np.where(take[c], dist[c], np.float32(np.inf)).reshape(len(c), -1)
                order = np.argsort(dm, axis=1, kind="stable")
                srt = np.take_along_axis(dm, order, axis=1)
                tie[c] = srt[:, KNN - 1] == srt[:, KNN]
                keep = np.zeros(dm.shape, bool)
                np.put_along_axis(keep, order[:, :KNN], True, axis=1)
                take[c] = keep.reshape(take[c].shape)
            near = ok & (np.abs(d64 - maxd) <= 1e-5 * maxd)
            slack = self.thr * np.where(near, np.abs(wv), 0.0).reshape(n, -1).sum(1)
        else:
            take = ok
            slack = np.zeros(n)
        u = d64 / self.sigma
        c = np.where(take, wv * np.exp(-(u * u)), 0.0)
        ac = np.abs(c)
        val = c.reshape(n, -1).sum(1)
        S = ac.reshape(n, -1).sum(1)
        gs = -2.0 / (self.sigma * self.sigma)
        d64a = [x.astype(np.float64) for x in d]
        grad = np.stack([gs * (c * d64a[0][:, None, None, :]).reshape(n, -1).sum(1),
                         gs * (c * d64a[1][:, None, :, None]).reshape(n, -1).sum(1),
                         gs * (c * d64a[2][:, :, None, None]).reshape(n, -1).sum(1)], axis=1)
        Sa = np.stack([-gs * (ac * np.abs(d64a[0])[:, None, None, :]).reshape(n, -1).sum(1),
                       -gs * (ac * np.abs(d64a[1])[:, None, :, None]).reshape(n, -1).sum(1),
                       -gs * (ac * np.abs(d64a[2])[:, :, None, None]).reshape(n, -1).sum(1)], axis=1)
        return dict(val=val + float(self.th), grad=grad, m=take.reshape(n, -1).sum(1).astype(np.int32), S=S, Sa=Sa,
                    slack=slack, capped=capped, tie=tie)

    # ---- bounds (derived like rbf_ref64.bound) -------------------------------------------------------------------
    def value_bound(self, ref):
        """m roundings of a Float32 accumulator are allowed (the reference's own sum), the rounding of the Float32
        distances and another exp() change exp(-u^2) by <= 6 ln(1/thr) 2^-24 relative; one rounding of the sum and one
        of `+ th`; nodes at the edge of the support may fall on either side (slack)"""
        return ((ref["m"] + 6.0 * math.log(1.0 / self.thr) + 8.0) * 2.0 ** -24 * ref["S"]
                + 2.0 ** -23 * (np.abs(ref["val"]) + abs(float(self.th))) + ref["slack"])

    def grad_bound(self, ref):
        """per component: Float64 sums rounded once (no accumulator term); an edge node contributes at most
        thr |w| 2 R / sigma"""
        return ((6.0 * math.log(1.0 / self.thr) + 12.0) * 2.0 ** -24 * ref["Sa"] + 2.0 ** -23 * np.abs(ref["grad"])
                + (ref["slack"] * 2.0 * self.R / self.sigma)[:, None])

    # ---- Float32 outputs of one evaluation, as the header states them ------------------------------------------------
    def eval32(self, points):
        r = self.evaluate(points)
        with np.errstate(invalid="ignore"):
            val = ((r["val"] - float(self.th)).astype(np.float32) + self.th).astype(np.float32)
        return val, r["grad"].astype(np.float32), r

    def normals(self, grad32):
        g = np.asarray(grad32, dtype=np.float32).astype(np.float64)
        g2 = (g * g).sum(1)
        ok = (g2 > 0) & np.isfinite(g2)
        out = np.zeros(g.shape, np.float32)
        out[ok] = (-g[ok] / np.sqrt(g2[ok])[:, None]).astype(np.float32)
        return out

    def project(self, points, max_iter, tol):
        """-> dict(points, status, iters, resid, err, border, trail, trail_err, trail_ok).
        err: the distance allowed between another correct evaluator's returned point and this one's: the sum over the steps
        of the one-step bound (see tests/test_field_gpu.py).
        border: some evaluation of the trajectory had | |f| - tol | within the value bound, so another correct evaluator
        may stop one step earlier or later.  For those the trajectory itself is returned: trail[k] = the point after k
        steps, with trail_err[k], valid where trail_ok[k]; it reaches one step BEYOND a status-0 stop (the step the
        other evaluator would take)."""
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3).copy()
        n = len(p)
        tol = np.float32(tol)
        cell = float(np.float32(self.h))
        status = np.full(n, 3, np.int32)
        iters = np.zeros(n, np.int32)
        resid = np.full(n, np.nan, np.float32)
        err = np.zeros(n)
        border = np.zeros(n, bool)
        trail = np.repeat(p[None], max_iter + 2, axis=0)
        trail_err = np.zeros((max_iter + 2, n))
        trail_ok = np.zeros((max_iter + 2, n), bool)
        live = np.flatnonzero(np.isfinite(p).all(1))
        trail_ok[0, live] = True
        it = 0
        while live.size:
            val, g, r = self.eval32(p[live])
            vb, gb = self.value_bound(r), self.grad_bound(r)
            resid[live] = np.abs(val)
            border[live] |= np.abs(np.abs(val).astype(np.float64) - float(tol)) <= vb
            g64 = g.astype(np.float64)
            g2 = (g64 * g64).sum(1)
            done = np.abs(val) <= tol
            status[live[done]] = 0
            rest = ~done
            if it >= max_iter:
                status[live[rest]] = 1
            good = (g2 > 0) & np.isfinite(g2)
            if it < max_iter:
                status[live[rest & ~good]] = 2
            # the step of every point with a usable gradient: taken by those that go on, kept as the trail's extra entry
            # for those that have just stopped
            f64 = val.astype(np.float64)
            g2s = np.where(good, g2, 1.0)
            s = f64 / g2s
            gn = np.sqrt(g2s)
            ln = np.abs(f64) / gn
            s = np.where(ln > cell, s * (cell / np.maximum(ln, 1e-300)), s)
            step_err = vb / gn + 3.0 * np.abs(f64) * np.sqrt((gb ** 2).sum(1)) / g2s + 2.0 ** -22 * np.abs(p[live]).max(1)
            nxt = (p[live].astype(np.float64) - s[:, None] * g64).astype(np.float32)
            trail[it + 1, live[good]] = nxt[good]
            trail_err[it + 1, live[good]] = err[live[good]] + step_err[good]
            trail_ok[it + 1, live[good]] = True
            if it >= max_iter:
                break
            go = rest & good
            ids = live[go]
            err[ids] = err[ids] + step_err[go]
            p[ids] = nxt[go]
            iters[ids] += 1
            live = ids
            it += 1
        return dict(points=p, status=status, iters=iters, resid=resid, err=err, border=border, trail=trail, trail_err=trail_err,
                    trail_ok=trail_ok)
