"""Sign_Detection restated in plain numpy float64, from the reference's Julia alone
(src/SignedDistances/SignDetection.jl:6-81 for HEX8, :128-147 for TET4; Grid.jl:10-35, :81-93).

Test infrastructure only.  It shares no code with the product or with the C oracle and is written for clarity:
every candidate pair (voxel, element) is inverse-mapped, then the reference's ordered walk is replayed.

HEX8.  The reference's find_local_coordinates minimises |x(xi) - x|^2 over the box |xi| <= 1.1 (LBFGS from nine
starts).  Where the inverse map has a root in that box the minimiser is that root; elsewhere it sits on the box
boundary with max|xi| = 1.1, which the walk's `max|xi| < 1.01` rejects.  So the restatement solves x(xi) = x by a
float64 Newton from the element centre, falls back to the eight other starts where that fails, iterates to a residual
of 1e-14 of the element size, and treats a pair without a root in the box as rejected (max|xi| = 1.1).

The candidate test `min <= x <= max` (SignDetection.jl:30) compares stored coordinates with grid_coord(i) =
AABB_min + cell * i; it involves no arithmetic of this file's and is taken as exact, so it has no margin.

Besides the signs it returns a per-voxel *decision margin*: how far the closest comparison that the outcome hangs on
is from flipping.  A voxel is *decidable* when the margin exceeds DECIDABLE = 1e-9: five orders above the round-off of
this file's own arithmetic, seven below the spacing of lattice points in xi on the grids of tests/sign_cases.py.
"""
import numpy as np

DECIDABLE = 1e-9

_S = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1],
               [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)    # hex8_shape.jl:28-35
_STARTS = np.array([[-.5, -.5, -.5], [.5, -.5, -.5], [.5, .5, -.5], [-.5, .5, -.5],
                    [-.5, -.5, .5], [.5, -.5, .5], [.5, .5, .5], [-.5, .5, .5]])     # FindLocalCoordinates.jl:27-37


# ---------------------------------------------------------------------------------------
# grid (Grid.jl)
# ---------------------------------------------------------------------------------------
class Grid64:
    def __init__(self, amin, amax, n_max, margin=3):
        amin, amax = np.asarray(amin, np.float64), np.asarray(amax, np.float64)
        self.cell = float(np.max(amax - amin) / n_max)
        self.amin = amin - margin * self.cell
        hi = amax + margin * self.cell
        self.N = np.ceil((hi - self.amin) / self.cell).astype(np.int64)
        self.amax = self.amin + self.N * self.cell
        self.dims = tuple(int(n) + 1 for n in self.N)
        self.ngp = int(np.prod(self.N + 1))

    def coord(self, axis, i):
        """grid_coord(i): AABB_min + cell_size * i, in this order (Grid.jl:87)"""
        return self.amin[axis] + self.cell * np.asarray(i, np.float64)

    def points(self):
        """(ngp, 3), x fastest (Grid.jl:84-90)"""
        ax = [self.coord(a, np.arange(self.dims[a])) for a in range(3)]
        Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


# ---------------------------------------------------------------------------------------
# HEX8
# ---------------------------------------------------------------------------------------
def hex8_shape(xi):
    """(n, 3) -> N (n, 8)"""
    return 0.125 * np.prod(1.0 + _S[None, :, :] * xi[:, None, :], axis=2)


def _hex8_dshape(xi):
    """(n, 3) -> dN/dxi (n, 8, 3)"""
    f = 1.0 + _S[None, :, :] * xi[:, None, :]
    d = np.empty(f.shape)
    d[:, :, 0] = _S[None, :, 0] * f[:, :, 1] * f[:, :, 2]
    d[:, :, 1] = _S[None, :, 1] * f[:, :, 0] * f[:, :, 2]
    d[:, :, 2] = _S[None, :, 2] * f[:, :, 0] * f[:, :, 1]
    return 0.125 * d


def _newton(Xe, x, xi0, tol, iters=30):
    """float64 Newton for x(xi) = x, all pairs at once; -> xi, converged"""
    xi = xi0.copy()
    ok = np.zeros(len(x), bool)
    live = np.ones(len(x), bool)
    for _ in range(iters):
        idx = np.nonzero(live)[0]
        if len(idx) == 0:
            break
        N = hex8_shape(xi[idx])
        R = np.einsum("nk,nkd->nd", N, Xe[idx]) - x[idx]
        res = np.linalg.norm(R, axis=1)
        conv = res <= tol[idx]
        ok[idx[conv]] = True
        live[idx[conv]] = False
        idx, R = idx[~conv], R[~conv]
        if len(idx) == 0:
            break
        J = np.einsum("nkd,nke->nde", Xe[idx], _hex8_dshape(xi[idx]))        # dx_d / dxi_e
        det = np.linalg.det(J)
        bad = ~(np.abs(det) > 1e-300) | ~np.isfinite(det)
        live[idx[bad]] = False
        idx, R, J = idx[~bad], R[~bad], J[~bad]
        step = np.linalg.solve(J, R[:, :, None])[:, :, 0]
        xi[idx] -= step
        far = np.abs(xi[idx]).max(axis=1) > 50.0                              # left for good: no root near the box
        live[idx[far]] = False
    return xi, ok


def hex8_inverse_map(Xe, x):
    """Xe (n, 8, 3), x (n, 3) -> xi (n, 3), found (n,).  `found`: a root with max|xi| <= 1.1 exists."""
    # coordinates relative to the element's first node: the differences are exact or nearly so, and the residual of
    # 1e-14 of the element size stays reachable for a mesh far from the origin
    x = x - Xe[:, 0, :]
    Xe = Xe - Xe[:, :1, :]
    size = np.linalg.norm(Xe.max(axis=1) - Xe.min(axis=1), axis=1)
    tol = 1e-14 * size
    xi, ok = _newton(Xe, x, np.zeros_like(x), tol)
    found = ok & (np.abs(xi).max(axis=1) <= 1.1)
    for s in _STARTS:                                                          # multi-start fallback
        todo = np.nonzero(~found)[0]
        if len(todo) == 0:
            break
        xi2, ok2 = _newton(Xe[todo], x[todo], np.broadcast_to(s, (len(todo), 3)).copy(), tol[todo])
        good = ok2 & (np.abs(xi2).max(axis=1) <= 1.1)
        xi[todo[good]] = xi2[good]
        found[todo[good]] = True
    return xi, found


def _candidate_pairs(lo, hi, pts, dims, amin, cell, slack=0.0):
    """all (voxel, element) with lo - slack <= x <= hi + slack, sorted by voxel, then by element (the walk's order).
    The index ranges are only a generous pre-selection; the float comparison with the point decides."""
    nx, ny, nz = dims
    vox, els = [], []
    for e in range(len(lo)):
        r = []
        for a, n in ((0, nx), (1, ny), (2, nz)):
            i0 = int(np.clip(np.floor((lo[e, a] - slack - amin[a]) / cell) - 1, 0, n))
            i1 = int(np.clip(np.ceil((hi[e, a] + slack - amin[a]) / cell) + 2, 0, n))
            r.append(np.arange(i0, i1))
        if min(len(q) for q in r) == 0:
            continue
        v = (r[2][:, None, None] * ny + r[1][None, :, None]) * nx + r[0][None, None, :]
        v = v.ravel()
        p = pts[v]
        inside = np.all(lo[e] - slack <= p, axis=1) & np.all(p <= hi[e] + slack, axis=1)
        vox.append(v[inside])
        els.append(np.full(int(inside.sum()), e, np.int64))
    if not vox:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    vox, els = np.concatenate(vox), np.concatenate(els)
    order = np.lexsort((els, vox))
    return vox[order], els[order]


def sign_hex8(X, IEN, rho_n, rho_t, grid):
    """-> dict: sign (ngp,), margin (ngp,), winner (ngp,; 0-based element whose acceptance came last, -1 none),
    winner_mx (ngp,; its max|xi|), pair_vox / pair_el / pair_mx / pair_xi (every candidate pair), n_cand (ngp,)"""
    X = np.asarray(X, np.float64)
    I0 = np.asarray(IEN, np.int64) - 1
    rho_n = np.asarray(rho_n, np.float64)
    pts = grid.points()
    ngp = len(pts)
    Xe_all = X[I0]                                                             # (nel, 8, 3)
    lo, hi = Xe_all.min(axis=1), Xe_all.max(axis=1)
    pv, pe = _candidate_pairs(lo, hi, pts, grid.dims, grid.amin, grid.cell)
    xi, found = hex8_inverse_map(Xe_all[pe], pts[pv])
    mx = np.where(found, np.abs(xi).max(axis=1), 1.1)
    rho = np.einsum("nk,nk->n", hex8_shape(np.where(found[:, None], xi, 0.0)), rho_n[I0[pe]])
    scale = max(1.0, abs(rho_t))

    n_cand = np.bincount(pv, minlength=ngp)
    start = np.concatenate([[0], np.cumsum(n_cand)])[:-1]
    rank = np.arange(len(pv)) - start[pv]
    # SignDetection.jl:36: no candidates, or every nodal density of every candidate below rho_t
    rmax_v = np.full(ngp, -np.inf)
    np.maximum.at(rmax_v, pv, rho_n[I0[pe]].max(axis=1))
    skipped = (n_cand == 0) | (rmax_v < rho_t)

    # the ordered walk (SignDetection.jl:41-70), one candidate rank at a time, every voxel at once
    sign = -np.ones(ngp)
    max_local = np.full(ngp, 10.0)
    done = np.zeros(ngp, bool)
    winner = np.full(ngp, -1, np.int64)
    winner_mx = np.full(ngp, np.nan)
    for r in range(int(n_cand.max()) if ngp and len(pv) else 0):
        sel = np.nonzero(rank == r)[0]
        v = pv[sel]
        take = ~done[v] & (mx[sel] < 1.01) & (max_local[v] > mx[sel])
        sel, v = sel[take], v[take]
        pos = rho[sel] >= rho_t
        sign[v[pos]] = 1.0
        winner[v], winner_mx[v] = pe[sel], mx[sel]
        deep = mx[sel] < 0.95
        done[v[deep]] = True
        max_local[v[~deep]] = mx[sel][~deep]
    walk_sign = sign.copy()
    sign[skipped] = -1.0

    # ---- decision margin ----
    margin = np.full(ngp, np.inf)
    np.minimum.at(margin, pv, np.abs(mx - 1.01))
    inb = mx < 1.01
    np.minimum.at(margin, pv[inb], np.abs(rho[inb] - rho_t) / scale)
    # the order-dependent comparisons (max_local > max|xi|, max|xi| < 0.95) matter only where the candidates inside the
    # 1.01 box disagree about rho >= rho_t; where they agree every walk gives that answer
    n_in = np.bincount(pv[inb], minlength=ngp)
    n_pos = np.bincount(pv[inb], weights=(rho[inb] >= rho_t).astype(np.float64), minlength=ngp)
    mixed = (n_pos > 0) & (n_pos < n_in)
    if mixed.any():
        sel = np.nonzero(inb & mixed[pv])[0]
        np.minimum.at(margin, pv[sel], np.abs(mx[sel] - 0.95))
        order = np.lexsort((mx[sel], pv[sel]))
        sv, sm = pv[sel][order], mx[sel][order]
        same = sv[1:] == sv[:-1]
        np.minimum.at(margin, sv[1:][same], (sm[1:] - sm[:-1])[same])
    # the early `continue`: it decides only where the walk would have answered +1
    skip_gap = np.abs(rmax_v - rho_t) / scale
    flips = (n_cand > 0) & (walk_sign > 0)
    margin = np.where(flips & skipped, skip_gap, np.where(flips, np.minimum(margin, skip_gap), margin))
    return dict(sign=sign, margin=margin, winner=winner, winner_mx=winner_mx, n_cand=n_cand,
                pair_vox=pv, pair_el=pe, pair_mx=mx, pair_xi=xi, pair_rho=rho)


# ---------------------------------------------------------------------------------------
# TET4
# ---------------------------------------------------------------------------------------
def sign_tet4(X, IEN, rho_n, rho_t, grid, tol=1e-10):
    """SignDetection.jl:127-150: +1 where some tetrahedron that holds the point (is_point_in_tetrahedron, tolerance
    1e-10) has valid barycentric coordinates (all >= 0, sum <= 1.0) and an interpolated density >= rho_t.
    The cell -> tetrahedra table of the reference lists a superset of the tetrahedra whose box holds the point, and
    the answer does not depend on their order, so the candidates here are those boxes.

    `sum(lambda) <= 1.0` compares a sum that equals 1 up to rounding; it is evaluated in the reference's order
    (lambda_1 = 1 - (l2 + l3 + l4), then ((l1 + l2) + l3) + l4) and a voxel whose sign changes when that one test is
    dropped has margin 0."""
    X = np.asarray(X, np.float64)
    I0 = np.asarray(IEN, np.int64) - 1
    rho_n = np.asarray(rho_n, np.float64)
    pts = grid.points()
    ngp = len(pts)
    Xe_all = X[I0]                                                             # (nel, 4, 3)
    lo, hi = Xe_all.min(axis=1), Xe_all.max(axis=1)
    pv, pe = _candidate_pairs(lo, hi, pts, grid.dims, grid.amin, grid.cell, slack=tol)
    Xe, x = Xe_all[pe], pts[pv]
    n = len(pv)
    # is_point_in_tetrahedron: T = [v1 v2 v3 v4; 1 1 1 1], lambda = T \ [x; 1]
    T = np.ones((n, 4, 4))
    T[:, :3, :] = np.transpose(Xe, (0, 2, 1))
    b = np.ones((n, 4))
    b[:, :3] = x
    det = np.linalg.det(T) if n else np.zeros(0)
    good = np.abs(det) > 0
    lam4 = np.full((n, 4), 10.0)
    if good.any():
        lam4[good] = np.linalg.solve(T[good], b[good][:, :, None])[:, :, 0]
    m_in = np.minimum((lam4 + tol).min(axis=1), (1.0 + tol - lam4).min(axis=1))         # >= 0: inside
    # find_local_coordinates(TET4): A = [x2-x1 x3-x1 x4-x1], l234 = A \ (x - x1)
    A = np.transpose(Xe[:, 1:, :] - Xe[:, :1, :], (0, 2, 1))
    l234 = np.full((n, 3), 10.0)
    if good.any():
        l234[good] = np.linalg.solve(A[good], (x - Xe[:, 0, :])[good][:, :, None])[:, :, 0]
    l1 = 1.0 - ((l234[:, 0] + l234[:, 1]) + l234[:, 2])
    lam = np.concatenate([l1[:, None], l234], axis=1)
    m_valid = lam.min(axis=1)                                                            # >= 0: valid
    s4 = ((lam[:, 0] + lam[:, 1]) + lam[:, 2]) + lam[:, 3]
    sum_ok = s4 <= 1.0
    N4 = 1.0 - ((lam[:, 0] + lam[:, 1]) + lam[:, 2])                                     # ShapeFunctions.jl:21
    rho = (lam[:, 0] * rho_n[I0[pe, 0]] + lam[:, 1] * rho_n[I0[pe, 1]] + lam[:, 2] * rho_n[I0[pe, 2]]
           + N4 * rho_n[I0[pe, 3]])
    scale = max(1.0, abs(rho_t))
    m_rho = (rho - rho_t) / scale                                                        # >= 0: solid
    m_all = np.minimum(np.minimum(m_in, m_valid), m_rho)                                 # >= 0: this pair says +1
    geo_ok = (m_in >= 0) & (m_valid >= 0)
    says = geo_ok & (rho >= rho_t)
    sign = -np.ones(ngp)
    sign[pv[says & sum_ok]] = 1.0
    nosum = -np.ones(ngp)
    nosum[pv[says]] = 1.0
    # margin: the surest +1 pair where there is one, else the least sure -1 pair
    best_pos = np.full(ngp, -np.inf)
    np.maximum.at(best_pos, pv, m_all)
    margin = np.where(best_pos >= 0, best_pos, -best_pos)
    margin[np.bincount(pv, minlength=ngp) == 0] = np.inf
    margin[sign != nosum] = 0.0
    return dict(sign=sign, margin=margin, n_cand=np.bincount(pv, minlength=ngp), pair_vox=pv, pair_el=pe,
                pair_lam=lam, pair_rho=rho, pair_m=m_all, pair_sum_ok=sum_ok)


def sign_ref(X, IEN, rho_n, rho_t, grid):
    return (sign_hex8 if np.asarray(IEN).shape[1] == 8 else sign_tet4)(X, IEN, rho_n, rho_t, grid)
