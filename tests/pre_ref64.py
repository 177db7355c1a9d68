"""A float64 restatement of the mesh pre-stage (helper of the tests), written from the reference's Julia:
calculate_mesh_volume (src/MeshGrid/MeshVolume.jl), DenseInNodes (NodalDensities.jl), calculate_isocontour_volume and
find_threshold_for_volume (Isocontour_volume.jl), nodeToElementConnectivity (MeshInformations.jl:69-77).  It shares no
code with the library or with the C oracle: Gauss points come from numpy's leggauss, the eigen-decomposition of A'A from
numpy.linalg.eigh (LAPACK, as `eigen` in Julia), batched over (n, 4, 4).

Arguments: X (nnp, 3) float64, IEN (nel, 8 | 4) 1-based int64, densities float64.

Every function returns, beside its result, an a-priori round-off bound for it (forward error analysis with absolute
values) that holds for ANY correct float64 evaluation of the same formulas, whatever the order of its sums:

- volume of one Gauss point: w |det J|.  An entry of J = xe dN is a sum of 8 (4) products, its error is a multiple of
  eps Jabs[r][c], Jabs = |xe| |dN|; to first order det J moves by sum_rc dJ[r][c] |cof[r][c]|, with the cofactors formed
  from |J|.  So the unit of a point is  w sum_rc Jabs[r][c] cofabs[r][c]  (>= 3 w perm|J| >= 3 w |det J|, which covers the
  roundings of the determinant itself), the unit U of a volume the sum over its points, and
      bound = K_VOL eps U + n eps V_abs
  where the second term allows any other order of the n additions (V_abs = the sum of the terms, all >= 0).
- a Gauss point of a cut element counts when v = N . rho_e >= thr: a discontinuous decision.  A point with
  |v - thr| <= K_PT eps (sum |N_a rho_a| + |thr|) may fall on either side; its weight is reported (`flagged`) and widens
  the bound.  TET4 (the library's own extension, documented in r2s_pre.hip: the classification of
  Isocontour_volume.jl:35-49 with the collapsed-cube rule of MeshVolume.jl:87-113 and the point test
  N = [xi, eta, zeta, 1 - xi - eta - zeta]) likewise.
- nodal density of a node with 4+ elements: DN = p' f(M) A'b with p = [1; x_i], M = A'A and f(M) the sum of
  phi_k phi_k' / lambda_k over the kept eigenpairs (NodalDensities.jl:159-179).  M and A'b are sums of cnt products, known to
  cnt eps trace(M) (Frobenius) and cnt eps |A|'|b|.  To first order f moves by dM / lambda_first^2 inside the kept block
  (which turns A'b into x: dM |x| / lambda_first) and by dM / (gap lambda_first) between a kept and a dropped pair,
  gap = lambda_first_kept - lambda_last_dropped.  So, with cond_kept = trace(M) / lambda_first in front,
      unit = |p| cnt (trace(M) (|x| / min(lambda_first, gap) + |c_dropped| / (gap lambda_first)) + | |A|'|b| | / lambda_first)
      bound = K_LSQ eps unit        (2-norms; c_dropped = the part of phi' A'b that the reduction drops).
  This is eps times the kept condition number times |p| |x|, the Cauchy-Schwarz majorant of the sum of |p_r x_r|: LAPACK's
  eigenvectors are accurate norm-wise, not component by component, and with the sum of |p_r x_r| itself the float64
  reference misses its exact self by a factor 2e3 on the (1, 1e-3, 1e3) meshes, where single components of x are tiny.
  The `mean(b)` leg: (cnt + 1) eps mean|b|.
  A node with 2 or 3 elements (FilterForNodalDensity): the weights 1 - L_j / Lmax lose |x| / L digits to the cancellation
  in x_i - c_e:  bound = K_FLT eps (1 + max(|x_i| + |c_e|) / min L) sum_j |rho_j w_j| / sum_j w_j.
  One element: the value itself, bound 0.  No element: 0.0, as `zeros` leaves it (:96).
- LamReduction (:192-218) decides on lambda ratios against 1e7 and 3e3.  An eigenvalue of the float64 A'A is only known
  to K_EIG eps cnt trace(A'A); a node one of whose decisive ratios lies within that (relative) distance of its
  threshold is `undecidable`: either leg is a correct float64 answer, so such nodes are left out of comparisons.

The constants are not guessed.  The same restatement runs in mpmath at 50 digits (`*_mp` below) on samples of every
mesh family the tests use (tests/test_pre_reference_cpu.py); the largest observed |float64 - exact| / (eps unit) were
    K_VOL: 0.57 (1.58 on coarser 6^3 / 4^3 meshes of the same families)    K_PT: 2.98    K_LSQ: 0.98 (1.19)
    K_FLT: 0.92 (1.28)    K_EIG: 1.82    mean(b) leg, no constant: 0.23 of its bound
and each constant is the smallest power of two that leaves a factor 4 over its ratio: 8, 16, 8, 8, 8.
"""
import math

import numpy as np

EPS = 2.0 ** -53
K_VOL = 8.0
K_PT = 16.0
K_LSQ = 8.0
K_FLT = 8.0
K_EIG = 8.0
T1, T2 = 1.0e7, 3.0e3          # LamReduction, NodalDensities.jl:194-195

# HEX8 corner signs (hex8_shape.jl:28-35): N_a = (1 + sx xi)(1 + sy eta)(1 + sz zeta) / 8
_S = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], float)
# TET4: N = [xi, eta, zeta, 1 - xi - eta - zeta] (ShapeFunctions.jl:50-72)
_DN_TET = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-1.0, -1.0, -1.0]])


def gauss(n):
    return np.polynomial.legendre.leggauss(n)


def hex_tables(n):
    """N (g, 8), dN (g, 8, 3), w (g) of the n^3 rule, point g = i + n (j + n k) as `for k, j, i` runs"""
    gp, gw = gauss(n)
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    xi = np.stack([gp[i.ravel()], gp[j.ravel()], gp[k.ravel()]], axis=1)
    f = 1.0 + _S[None, :, :] * xi[:, None, :]                       # (g, 8, 3)
    N = 0.125 * f[:, :, 0] * f[:, :, 1] * f[:, :, 2]
    dN = np.stack([0.125 * _S[None, :, 0] * f[:, :, 1] * f[:, :, 2],
                   0.125 * _S[None, :, 1] * f[:, :, 0] * f[:, :, 2],
                   0.125 * _S[None, :, 2] * f[:, :, 0] * f[:, :, 1]], axis=2)
    w = gw[i.ravel()] * gw[j.ravel()] * gw[k.ravel()]
    return N, dN, w


def tet_tables(n):
    """N (g, 4), w (g) of the collapsed n^3 rule (MeshVolume.jl:87-113); w carries the reference's
    jacobian_transform (1 - xi)^2 (1 - xi - eta) / 8 (:110), one factor (1 - xi) more than the map's Jacobian"""
    gp, gw = gauss(n)
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    xi = (gp[i.ravel()] + 1.0) / 2.0
    eta = (gp[j.ravel()] + 1.0) / 2.0 * (1.0 - xi)
    zeta = (gp[k.ravel()] + 1.0) / 2.0 * (1.0 - xi - eta)
    inside = ~((xi < 0) | (eta < 0) | (zeta < 0) | (xi + eta + zeta > 1.0))      # :99
    jt = (1.0 - xi) ** 2 * (1.0 - xi - eta) / 8.0
    w = gw[i.ravel()] * gw[j.ravel()] * gw[k.ravel()] * jt * inside
    N = np.stack([xi, eta, zeta, 1.0 - xi - eta - zeta], axis=1)
    return N, w


def _det_and_unit(J, Jabs):
    """det J and sum_rc Jabs[r][c] cofabs[r][c] over the last two axes"""
    a = np.abs(J)
    det = (J[..., 0, 0] * (J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1])
           - J[..., 0, 1] * (J[..., 1, 0] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 0])
           + J[..., 0, 2] * (J[..., 1, 0] * J[..., 2, 1] - J[..., 1, 1] * J[..., 2, 0]))
    unit = 0.0
    for r in range(3):
        r1, r2 = (r + 1) % 3, (r + 2) % 3
        for c in range(3):
            c1, c2 = (c + 1) % 3, (c + 2) % 3
            unit = unit + Jabs[..., r, c] * (a[..., r1, c1] * a[..., r2, c2] + a[..., r1, c2] * a[..., r2, c1])
    return det, unit


def _hex_points(Xe, dN):
    """|det J| and its unit at every point: Xe (m, 8, 3), dN (g, 8, 3) -> (m, g) each"""
    m, g = len(Xe), len(dN)
    D = dN.transpose(1, 0, 2).reshape(8, g * 3)
    Xt = Xe.transpose(0, 2, 1).reshape(m * 3, 8)
    J = (Xt @ D).reshape(m, 3, g, 3).transpose(0, 2, 1, 3)
    Jabs = (np.abs(Xt) @ np.abs(D)).reshape(m, 3, g, 3).transpose(0, 2, 1, 3)
    det, unit = _det_and_unit(J, Jabs)
    return np.abs(det), unit


def _tet_det(Xe):
    """|det J| and unit of the constant TET4 Jacobian: Xe (m, 4, 3) -> (m), (m)"""
    J = np.einsum("mar,ac->mrc", Xe, _DN_TET)
    Jabs = np.einsum("mar,ac->mrc", np.abs(Xe), np.abs(_DN_TET))
    det, unit = _det_and_unit(J, Jabs)
    return np.abs(det), unit


def element_volumes(X, IEN, chunk=20000):
    """calculate_element_volume with the 3^3 rule (MeshVolume.jl:45-117) -> (vol (nel), unit (nel))"""
    X = np.asarray(X, float)
    I0 = np.asarray(IEN) - 1
    nel, nen = I0.shape
    vol, unit = np.empty(nel), np.empty(nel)
    if nen == 8:
        _, dN, w = hex_tables(3)
        for s in range(0, nel, chunk):
            d, u = _hex_points(X[I0[s:s + chunk]], dN)
            vol[s:s + chunk] = d @ w
            unit[s:s + chunk] = u @ w
    else:
        _, w = tet_tables(3)
        d, u = _tet_det(X[I0])
        vol[:] = (d[:, None] * w[None, :]).sum(1)
        unit[:] = u * w.sum()
    return vol, unit


def mesh_volume(X, IEN, rho):
    """calculate_mesh_volume (MeshVolume.jl:4-42) -> dict(V_domain, V_frac, bound_domain, bound_frac, vol)"""
    rho = np.asarray(rho, float)
    vol, unit = element_volumes(X, IEN)
    nen = np.asarray(IEN).shape[1]
    n = vol.size * 27
    vd, vt = math.fsum(vol), math.fsum(vol * rho)
    bd = K_VOL * EPS * math.fsum(unit) + n * EPS * vd
    bt = K_VOL * EPS * math.fsum(unit * np.abs(rho)) + (n + 1) * EPS * math.fsum(vol * np.abs(rho))
    vf = vt / vd                                                      # :41
    bf = (bt + abs(vf) * bd) / vd + 2 * EPS * abs(vf)
    return dict(V_domain=vd, V_frac=vf, bound_domain=bd, bound_frac=bf, vol=vol, nen=nen)


# ---- DenseInNodes -------------------------------------------------------------------------------------------------------
def node_elements(IEN, nnp):
    """nodeToElementConnectivity (MeshInformations.jl:69-77): CSR (ptr, elements), each node's elements ascending"""
    I0 = np.asarray(IEN) - 1
    nen = I0.shape[1]
    flat = I0.ravel()
    order = np.argsort(flat, kind="stable")                           # (element-major input: ascending elements per node)
    ptr = np.zeros(nnp + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=nnp), out=ptr[1:])
    return ptr, order // nen


def centroids(X, IEN):
    """GeometricCentre (NodalDensities.jl:71-80): the mean of the element's nodes"""
    return np.asarray(X, float)[np.asarray(IEN) - 1].mean(axis=1)


LEG_NONE, LEG_ONE, LEG_FILTER, LEG_LSQ = 0, 1, 2, 3


def _norm2(v):
    """row-wise 2-norm that does not underflow on densities of 1e-250 (the fixtures hold such values)"""
    m = np.abs(v).max(1)
    m = np.where(m > 0, m, 1.0)
    return m * np.sqrt(((v / m[:, None]) ** 2).sum(1))


def lam_reduction(lam):
    """LamReduction (:192-218) on ascending eigenvalues (n, 4) -> (kept (n): 4, 3, 2, 1 eigenvalues or 0 = the `else`
    leg that makes the caller take mean(b), e1, e2, e3)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        e1 = np.abs(lam[:, 3] / lam[:, 0])
        e2 = np.abs(lam[:, 3] / lam[:, 1])
        e3 = np.abs(lam[:, 3] / lam[:, 2])
    kept = np.zeros(len(lam), np.int32)
    a = (T1 > e1) & (T2 > e2)
    b = (T1 < e1) & (T2 > e2)
    c = (T1 < e1) & (T2 < e2)
    kept[a] = 4
    kept[b] = 3
    kept[c & (T2 > e3)] = 2
    kept[c & ~(T2 > e3)] = 1
    return kept, e1, e2, e3


def dense_in_nodes(X, IEN, rho):
    """DenseInNodes (NodalDensities.jl:89-108) -> dict(rho_n, bound, count, leg, e1, e2, e3, kept, cond, undecidable)"""
    X = np.asarray(X, float)
    rho = np.asarray(rho, float)
    nnp = len(X)
    ptr, els = node_elements(IEN, nnp)
    C = centroids(X, IEN)
    cnt = np.diff(ptr)
    out = dict(rho_n=np.zeros(nnp), bound=np.zeros(nnp), count=cnt, leg=np.zeros(nnp, np.int32),
               e1=np.full(nnp, np.nan), e2=np.full(nnp, np.nan), e3=np.full(nnp, np.nan), kept=np.full(nnp, -1, np.int32),
               cond=np.full(nnp, np.nan), lam=np.full((nnp, 4), np.nan), undecidable=np.zeros(nnp, bool), margin=np.full(nnp, np.inf))
    for c in np.unique(cnt):
        nodes = np.flatnonzero(cnt == c)
        if c == 0:
            continue
        E = els[ptr[nodes][:, None] + np.arange(c)[None, :]]          # (m, c)
        b = rho[E]
        if c == 1:
            out["rho_n"][nodes] = b[:, 0]                             # :99-100
            out["leg"][nodes] = LEG_ONE
        elif c < 4:                                                   # FilterForNodalDensity (:117-136)
            d = X[nodes][:, None, :] - C[E]
            L = np.sqrt((d * d).sum(2))
            Lmax = L.max(1) * 1.2
            w = 1.0 - L / Lmax[:, None]
            den = w.sum(1)
            out["rho_n"][nodes] = (b * w).sum(1) / den
            mag = (np.abs(X[nodes]).sum(1)[:, None] + np.abs(C[E]).sum(2)).max(1)
            out["bound"][nodes] = K_FLT * EPS * (1.0 + mag / L.min(1)) * (np.abs(b) * w).sum(1) / den
            out["leg"][nodes] = LEG_FILTER
        else:                                                         # NodalDensityLeastSquares (:145-183)
            A = np.concatenate([np.ones((len(nodes), c, 1)), C[E]], axis=2)
            M = np.einsum("mjr,mjs->mrs", A, A)
            Atb = np.einsum("mjr,mj->mr", A, b)
            lam, phi = np.linalg.eigh(M)                              # ascending, eigenvectors in columns
            kept, e1, e2, e3 = lam_reduction(lam)
            poz = 4 - kept                                            # 0-based first kept column
            b1 = np.einsum("mrc,mr->mc", phi, Atb)
            keepmask = np.arange(4)[None, :] >= poz[:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                x2 = np.where(keepmask, b1 / lam, 0.0)
            x = np.einsum("mrc,mc->mr", phi, x2)
            p = np.concatenate([np.ones((len(nodes), 1)), X[nodes]], axis=1)
            val = (p * x).sum(1)
            idx = np.arange(len(nodes))
            first = lam[idx, np.minimum(poz, 3)]
            dropped = np.where(poz > 0, lam[idx, np.maximum(poz - 1, 0)], -np.inf)
            c_drop = _norm2(np.where(keepmask, 0.0, b1))
            Atb_abs = np.einsum("mjr,mj->mr", np.abs(A), np.abs(b))
            nrm = _norm2
            with np.errstate(divide="ignore", invalid="ignore"):
                cond = np.abs(lam[:, 3] / first)
                gap = first - dropped
                unit = nrm(p) * c * (np.trace(M, axis1=1, axis2=2) * (nrm(x) / np.minimum(first, gap)
                                                                        + np.where(poz > 0, c_drop / (gap * first), 0.0))
                                     + nrm(Atb_abs) / first)
                bound = K_LSQ * EPS * unit
            mean = kept == 0                                          # :166-167
            val[mean] = b[mean].mean(1)
            bound[mean] = (c + 1) * EPS * np.abs(b[mean]).mean(1)
            cond[mean] = 1.0
            # how far (relative) each decisive ratio is from its threshold, against how well lambda is known
            dl = K_EIG * EPS * c * np.trace(M, axis1=1, axis2=2)
            with np.errstate(divide="ignore", invalid="ignore"):
                m1 = np.abs(e1 / T1 - 1.0) - dl / np.abs(lam[:, 0])
                m2 = np.abs(e2 / T2 - 1.0) - dl / np.abs(lam[:, 1])
                m3 = np.abs(e3 / T2 - 1.0) - dl / np.abs(lam[:, 2])
            m3 = np.where((T1 < e1) & (T2 < e2) | (m1 <= 0) | (m2 <= 0), m3, np.inf)   # e3 decides in the third leg only
            margin = np.minimum(np.minimum(m1, m2), m3)
            margin = np.where(np.isnan(margin), -np.inf, margin)
            out["rho_n"][nodes] = val
            out["bound"][nodes] = bound
            out["leg"][nodes] = LEG_LSQ
            out["kept"][nodes] = kept
            out["cond"][nodes] = cond
            out["lam"][nodes] = lam
            out["e1"][nodes], out["e2"][nodes], out["e3"][nodes] = e1, e2, e3
            out["margin"][nodes] = margin
            out["undecidable"][nodes] = margin <= 0
    # below the normal range the eps model ends: a subnormal result is known to the subnormal spacing times the
    # amplification of the solve (<= 1e7), far inside the smallest normal number
    out["bound"][cnt > 1] += np.finfo(float).tiny
    return out


# ---- calculate_isocontour_volume ----------------------------------------------------------------------------------------
def isocontour_volume(X, IEN, rho_n, thr, chunk=64):
    """calculate_isocontour_volume (Isocontour_volume.jl:1-75) and its TET4 counterpart ->
    dict(volume, bound, flagged, n_skip, n_whole, n_cut)"""
    X = np.asarray(X, float)
    rho_n = np.asarray(rho_n, float)
    I0 = np.asarray(IEN) - 1
    nen = I0.shape[1]
    re = rho_n[I0]
    mn, mx = re.min(1), re.max(1)
    skip = mx < thr                                                   # :35
    whole = ~skip & (mn >= thr)                                       # :41
    cut = ~skip & ~whole
    vol3, unit3 = element_volumes(X, IEN[whole]) if whole.any() else (np.zeros(0), np.zeros(0))
    terms, units, flagged = [vol3], [unit3], 0.0
    n = 27 * int(whole.sum()) + 3375 * int(cut.sum())
    ids = np.flatnonzero(cut)
    if nen == 8:
        N, dN, w = hex_tables(15)
    else:
        N, w = tet_tables(15)
    aN = np.abs(N)
    for s in range(0, len(ids), chunk):
        e = ids[s:s + chunk]
        v = re[e] @ N.T                                               # (m, g)   :60
        slack = K_PT * EPS * (np.abs(re[e]) @ aN.T + abs(thr))
        take = ~(v < thr)                                             # :61
        if nen == 8:
            d, u = _hex_points(X[I0[e]], dN)
        else:
            d, u = _tet_det(X[I0[e]])
            d, u = d[:, None], u[:, None]
        t = d * w[None, :]
        flagged += float((t * (np.abs(v - thr) <= slack)).sum())
        terms.append((t * take).sum(1))
        units.append((u * w[None, :] * take).sum(1))
    V = math.fsum(np.concatenate(terms))
    U = math.fsum(np.concatenate(units))
    return dict(volume=V, bound=K_VOL * EPS * U + n * EPS * V + flagged, flagged=flagged, n_skip=int(skip.sum()),
                n_whole=int(whole.sum()), n_cut=int(cut.sum()))


# ---- find_threshold_for_volume -------------------------------------------------------------------------------------------
class OutOfRange(ValueError):
    pass


def find_threshold(X, IEN, rho_n, target, tol=1e-4, maxit=60):
    """find_threshold_for_volume (Isocontour_volume.jl:77-154) -> dict(rho_t, iters, steps, decidable, vmin, vmax, ...).
    steps: per evaluation (thr, volume, bound, margin): margin = the smallest distance, in volume, between a number a
    decision compares and the number it is compared with (v against target; |v - target| against tol * target and
    against the best error so far).  decidable: every margin exceeds its bound, so any evaluation within the bound
    takes the same decisions and returns the same threshold after the same number of iterations."""
    lo, hi = 0.0, 1.0
    rmin = isocontour_volume(X, IEN, rho_n, hi)                       # :89
    rmax = isocontour_volume(X, IEN, rho_n, lo)                       # :90
    vmin, vmax = rmin["volume"], rmax["volume"]
    range_margin = min(abs(target - vmax) - rmax["bound"], abs(target - vmin) - rmin["bound"])
    res = dict(vmin=vmin, vmax=vmax, bound_min=rmin["bound"], bound_max=rmax["bound"], range_margin=range_margin, steps=[])
    if target > vmax or target < vmin:                                # :93-95
        raise OutOfRange(f"Requested volume {target} is outside the possible range [{vmin}, {vmax}]", res)
    it, best, best_err = 0, 0.0, math.inf
    decidable = range_margin > 0
    while it < maxit:                                                 # :106
        thr = (lo + hi) / 2
        r = isocontour_volume(X, IEN, rho_n, thr)
        v = r["volume"]
        err = abs(v - target) / target                               # :114
        dist = abs(v - target)
        margin = min(dist, abs(dist - tol * target), abs(dist - best_err * target) if math.isfinite(best_err) else math.inf)
        res["steps"].append(dict(thr=thr, volume=v, bound=r["bound"], margin=margin, flagged=r["flagged"]))
        decidable = decidable and margin > 2.0 * r["bound"]
        if err < best_err:                                            # :121-124
            best, best_err = thr, err
        if err < tol:                                                 # :127
            break
        if v > target:                                                # :132-136
            lo = thr
        else:
            hi = thr
        it += 1
    res.update(rho_t=best, iters=it, decidable=decidable)
    return res


# ---- the same in mpmath (50 digits), on samples: where the constants come from ------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def element_volume_mp(Xe):
    """one element's 3^3 volume from its float64 coordinates, everything else exact to 50 digits"""
    mp = _mp()
    nen = len(Xe)
    gp, gw = _gauss_mp(3)
    Xm = [[mp.mpf(float(v)) for v in row] for row in Xe]
    tot = mp.mpf(0)
    for k in range(3):
        for j in range(3):
            for i in range(3):
                if nen == 8:
                    xi = (gp[i], gp[j], gp[k])
                    dN = _hex_dn_mp(xi)
                    wt = gw[i] * gw[j] * gw[k]
                else:
                    a = (gp[i] + 1) / 2
                    b = (gp[j] + 1) / 2 * (1 - a)
                    dN = [[mp.mpf(v) for v in row] for row in _DN_TET.tolist()]
                    wt = gw[i] * gw[j] * gw[k] * (1 - a) ** 2 * (1 - a - b) / 8
                J = mp.matrix(3, 3)
                for r in range(3):
                    for c in range(3):
                        J[r, c] = sum(Xm[a_][r] * dN[a_][c] for a_ in range(nen))
                tot += wt * abs(mp.det(J))
    return tot


_GAUSS_MP = {}


def _gauss_mp(n):
    """Gauss-Legendre nodes and weights to 50 digits: Newton on P_n from numpy's nodes"""
    if n not in _GAUSS_MP:
        mp = _mp()
        xs, ws = [], []
        for x0 in gauss(n)[0]:
            x = mp.mpf(float(x0))
            for _ in range(6):
                p0, p1 = mp.mpf(1), x
                for k in range(2, n + 1):
                    p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
                dp = n * (x * p1 - p0) / (x * x - 1)
                x = x - p1 / dp
            p0, p1 = mp.mpf(1), x
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            dp = n * (x * p1 - p0) / (x * x - 1)
            xs.append(x)
            ws.append(2 / ((1 - x * x) * dp * dp))
        _GAUSS_MP[n] = (xs, ws)
    return _GAUSS_MP[n]


def _hex_dn_mp(xi):
    mp = _mp()
    out = []
    for a in range(8):
        f = [1 + mp.mpf(_S[a, c]) * xi[c] for c in range(3)]
        out.append([mp.mpf(_S[a, 0]) * f[1] * f[2] / 8, mp.mpf(_S[a, 1]) * f[0] * f[2] / 8, mp.mpf(_S[a, 2]) * f[0] * f[1] / 8])
    return out


def hex_point_value_mp(re, g, n=15):
    """N . rho_e at point g of the n^3 HEX8 rule, exact"""
    mp = _mp()
    gp, _ = _gauss_mp(n)
    xi = (gp[g % n], gp[(g // n) % n], gp[g // (n * n)])
    tot = mp.mpf(0)
    for a in range(8):
        tot += (1 + mp.mpf(_S[a, 0]) * xi[0]) * (1 + mp.mpf(_S[a, 1]) * xi[1]) * (1 + mp.mpf(_S[a, 2]) * xi[2]) / 8 * mp.mpf(float(re[a]))
    return tot


def nodal_density_mp(X, IEN, rho, node, ptr, els, kept):
    """one node's density, exact from the float64 inputs; `kept` (the float64 reference's LamReduction decision) selects
    the eigenvalues for a 4+ node.  -> (value, ascending eigenvalues or None)"""
    mp = _mp()
    E = els[ptr[node]:ptr[node + 1]]
    nen = IEN.shape[1]
    Cm = [[sum(mp.mpf(float(X[n - 1, i])) for n in IEN[e]) / nen for i in range(3)] for e in E]
    b = [mp.mpf(float(rho[e])) for e in E]
    x = [mp.mpf(float(v)) for v in X[node]]
    c = len(E)
    if c == 0:
        return mp.mpf(0), None
    if c == 1:
        return b[0], None
    if c < 4:
        L = [mp.sqrt(sum((x[i] - Cm[j][i]) ** 2 for i in range(3))) for j in range(c)]
        Lmax = max(L) * mp.mpf(1.2)
        w = [1 - Lj / Lmax for Lj in L]
        return sum(bj * wj for bj, wj in zip(b, w)) / sum(w), None
    A = mp.matrix(c, 4)
    for j in range(c):
        A[j, 0] = 1
        for i in range(3):
            A[j, i + 1] = Cm[j][i]
    M = A.T * A
    lam, phi = mp.eigsy(M)
    order = sorted(range(4), key=lambda i: lam[i])
    lam_s = [lam[i] for i in order]
    if kept == 0:
        return sum(b) / c, lam_s
    Atb = A.T * mp.matrix(b)
    p = [mp.mpf(1)] + x
    val = mp.mpf(0)
    for i in order[4 - kept:]:
        coef = sum(phi[r, i] * Atb[r] for r in range(4)) / lam[i]
        val += coef * sum(p[r] * phi[r, i] for r in range(4))
    return val, lam_s
