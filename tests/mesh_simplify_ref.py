"""r2s_mesh_simplify (include/rho2sdf_hip.h) restated in numpy / Python, for tests/test_mesh_simplify_cpu.py and _gpu.py.

Cells are a dict from the tuple floor(float64(v) / cell) to its members; the Float64 sums are taken in the header's order through
tests/segsum_ref.py (one IEEE addition at a time, no fused operation); the per-class solve uses numpy.linalg.eigh (LAPACK), on
purpose NOT the library's Jacobi.  On every case it is given, simplify_ref asserts

  the summation bound   |sum - exact| <= (n + K) 2^-53 T per class and column, with n the items of the class, T the sum of the
      absolute terms and `exact` the Fraction sum of the same Float64 terms.  Derivation: any order of n - 1 additions has
      |error| <= gamma(n - 1) T, gamma(k) = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability, 4.2), and
      gamma(n - 1) <= n u as long as n (n - 1) u <= 1, i.e. n < 9e7.  So K = 0 holds for the sums; K = 2 is used everywhere so
      that the same bound also covers one rounding in each term (sum of u |term| = u T) and the division by the count.

and records which classes decided with a margin: no eigenvalue ratio lambda / lambda_max within a factor 2 of the 1e-3 truncation
threshold, no pull-back factor within 1e-9 of 1, and no step component within a factor 2 of the 2^-40 cell below which an axis is
not pulled back.  Classes without a margin are `undecidable` for a comparison with the one result; for them `candidates` lists
the result of EVERY decision the class could take (each eigenvalue without a margin kept or dropped, the pull-back flag set or
not), the definition's own first, so that an implementation can still be compared: it has to agree with one of them."""
from fractions import Fraction

import numpy as np

import segsum_ref

K = 2
U = 2.0 ** -53
MEAN, QUADRIC = "mean", "quadric"
TRUNCATION = 1e-3
TINY_STEP = 2.0 ** -40                                    # in cells: a step component below this is not pulled back


def cells_of(verts, cell):
    """(nv, 3) int64 cell indices: float64(v) / cell, then floor (-0.0 folds onto 0)"""
    q = np.floor(np.asarray(verts, np.float32).astype(np.float64) / float(cell))
    if not np.isfinite(q).all() or (q < -2.0 ** 31).any() or (q >= 2.0 ** 31).any():
        raise ValueError("cell is too fine for the extent of the mesh")
    return q.astype(np.int64)


def ref_point(verts):
    v = np.asarray(verts, np.float32)
    return 0.5 * (v.min(0).astype(np.float64) + v.max(0).astype(np.float64)) if len(v) else np.zeros(3)


def quadric_terms(verts, tris, t, ref):
    """the ten Float64 terms of triangles t in the header's operation order -> (len(t), 10)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    a = v[tris[t, 0]] - ref
    e1 = (v[tris[t, 1]] - ref) - a
    e2 = (v[tris[t, 2]] - ref) - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = (n0 * a[:, 0] + n1 * a[:, 1]) + n2 * a[:, 2]
    return np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, d * n0, d * n1, d * n2, d * d], 1)


def _check_sums(terms, starts, sums):
    """the summation bound of the module docstring; -> (T (n, k), bound (n, k))"""
    n = len(starts) - 1
    T = np.add.reduceat(np.abs(terms), starts[:-1], axis=0) if n else np.zeros((0, terms.shape[1]))
    count = np.diff(starts)[:, None]
    bound = (count + K) * U * T
    for s in range(n):
        for q in range(terms.shape[1]):
            exact = sum((Fraction(float(x)) for x in terms[starts[s]:starts[s + 1], q]), Fraction(0))
            assert abs(Fraction(float(sums[s, q])) - exact) <= Fraction(float(bound[s, q])), (s, q)
    return T, bound


def _quadric_value(S, b, c, p):
    Sp = [(S[k][0] * p[0] + S[k][1] * p[1]) + S[k][2] * p[2] for k in range(3)]
    quadratic = (p[0] * Sp[0] + p[1] * Sp[1]) + p[2] * Sp[2]
    linear = (b[0] * p[0] + b[1] * p[1]) + b[2] * p[2]
    return (quadratic - 2.0 * linear) + c


def simplify_ref(verts, tris, cell, rule=QUADRIC, drop_duplicates=True, check=True):
    """-> dict: verts, tris, vert_map, tri_map, members, error, solved, totals as the library defines them, and for the tests
    cells (n_out, 3), ref, mean (n_out, 3 Float64 about ref), mean_T / mean_bound (the summation bound of the mean per
    coordinate, before the division), undecidable (n_out,) bool, candidates (per class a list of (solved, float32 point): one entry
    where the class has a margin), items_max"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    nv, nt = len(v), len(t)
    cell = float(cell)
    assert cell > 0.0 and np.isfinite(cell) and rule in (MEAN, QUADRIC)
    assert nt == 0 or (t.min() >= 0 and t.max() < nv)
    q = cells_of(v, cell)
    input_ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2]) if nt else np.zeros(0, bool)
    member = np.zeros(nv, bool)
    member[t[input_ok].ravel()] = True
    members_of = {}                                        # cell tuple -> ascending member list
    for i in np.nonzero(member)[0]:
        members_of.setdefault(tuple(q[i]), []).append(int(i))
    # triangles through the classes (a class is named by its cell tuple here)
    seen, orientations = set(), {}
    keep = np.zeros(nt, bool)
    n_collapsed = n_dup = 0
    for k in range(nt):
        c = [tuple(q[i]) for i in t[k]]
        if c[0] == c[1] or c[1] == c[2] or c[0] == c[2]:
            n_collapsed += 1                               # (an input-collapsed triangle has two equal cells too)
            continue
        r = min(range(3), key=lambda j: c[j])
        key = (c[r], c[(r + 1) % 3], c[(r + 2) % 3])
        dup = key in seen
        seen.add(key)
        n_dup += dup
        orientations.setdefault(frozenset(c), set()).add(key)
        keep[k] = not (dup and drop_duplicates)
    n_opposite = sum(len(o) == 2 for o in orientations.values())
    used = {tuple(q[i]) for i in t[keep].ravel()}
    order = sorted(used, key=lambda c: members_of[c][0])   # first-occurrence order of the first member
    number = {c: n for n, c in enumerate(order)}
    n_out = len(order)
    vert_map = np.array([number.get(tuple(q[i]), -1) if member[i] else -1 for i in range(nv)], np.int32).reshape(nv)
    tri_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    tris_out = vert_map[t[keep]].reshape(-1, 3).astype(np.int32)
    totals = np.array([n_out, int(keep.sum()), int(member.sum()) - n_out, n_collapsed, n_dup, n_opposite, nv - int(member.sum()), 0], np.int64)
    out = dict(verts=np.zeros((0, 3), np.float32), tris=tris_out, vert_map=vert_map, tri_map=tri_map, members=np.zeros(0, np.int64),
               error=np.zeros(0), solved=np.zeros(0, np.int32), totals=totals, cells=np.zeros((0, 3), np.int64), ref=ref_point(v),
               mean=np.zeros((0, 3)), mean_T=np.zeros((0, 3)), mean_bound=np.zeros((0, 3)), undecidable=np.zeros(0, bool), candidates=[], items_max=0)
    if n_out == 0:
        return out
    ref = out["ref"]
    # the mean: items = members, ascending inside a class
    vitems = np.concatenate([members_of[c] for c in order])
    vstarts = np.concatenate([[0], np.cumsum([len(members_of[c]) for c in order])])
    vterms = v[vitems].astype(np.float64) - ref
    vsums = segsum_ref.segsum(vterms, vstarts)
    count = np.diff(vstarts)
    # the quadric: items = (class, triangle), one per distinct output class of a non-collapsed input triangle
    pairs = []
    for k in np.nonzero(input_ok)[0]:
        f = []
        for i in t[k]:
            if vert_map[i] >= 0 and vert_map[i] not in f:
                f.append(int(vert_map[i]))
        pairs += [(c, int(k)) for c in f]
    pairs.sort()                                           # (by class, then triangle: no pair occurs twice)
    qclass = np.array([p[0] for p in pairs], np.int64)
    qtri = np.array([p[1] for p in pairs], np.int64)
    qstarts = np.searchsorted(qclass, np.arange(n_out + 1))
    assert (np.diff(qstarts) > 0).all()
    qterms = quadric_terms(v, t, qtri, ref)
    qsums = segsum_ref.segsum(qterms, qstarts)
    if check:
        mean_T, mean_bound = _check_sums(vterms, vstarts, vsums)
        _check_sums(qterms, qstarts, qsums)
    else:
        mean_T = np.add.reduceat(np.abs(vterms), vstarts[:-1], axis=0)
        mean_bound = (count[:, None] + K) * U * mean_T
    cells = np.array(order, np.int64)
    lo = cells * cell - ref
    hi = (cells + 1.0) * cell - ref
    mean = vsums / count[:, None]
    x = mean.copy()
    solved = np.zeros(n_out, np.int32)
    undecidable = np.zeros(n_out, bool)
    candidates = [None] * n_out
    pulled_total = 0
    for c in range(n_out):
        Q = qsums[c]
        S = np.array([[Q[0], Q[1], Q[2]], [Q[1], Q[3], Q[4]], [Q[2], Q[4], Q[5]]])
        b = Q[6:9]
        m = mean[c]
        candidates[c] = [(0, (m + ref).astype(np.float32))]
        if rule == QUADRIC:
            w, V = np.linalg.eigh(S)
            wmax = w.max()
            if wmax > 0.0:
                g = b - S @ m
                ratio = w / wmax
                marginal = (ratio > 0.5 * TRUNCATION) & (ratio < 2.0 * TRUNCATION)
                first = ~(w < TRUNCATION * wmax)
                # the definition's decision first, then every other decision of the eigenvalues without a margin
                keeps = [first] + [k for k in (np.where(marginal, np.array(bits), first) for bits in np.ndindex(2, 2, 2))
                                   if not np.array_equal(k, first)]
                seen = []
                for kept in keeps:
                    if any(np.array_equal(kept, k) for k in seen):
                        continue
                    seen.append(kept)
                    step = np.zeros(3)
                    for e in np.nonzero(kept)[0]:
                        step = step + (V[:, e] @ g) / w[e] * V[:, e]
                    s, close = np.inf, False
                    for k in range(3):                     # (an axis the step does not really move along constrains nothing)
                        if step[k] > TINY_STEP * cell:
                            s = min(s, (hi[c, k] - m[k]) / step[k])
                        elif step[k] < -TINY_STEP * cell:
                            s = min(s, (lo[c, k] - m[k]) / step[k])
                        close |= bool(0.5 * TINY_STEP * cell < abs(step[k]) < 2.0 * TINY_STEP * cell)
                    s = max(s, 0.0)
                    close |= bool(abs(s - 1.0) <= 1e-9)
                    found = []
                    for pulled in ([s < 1.0] if not close else [s < 1.0, not s < 1.0]):
                        xc = m + min(s, 1.0) * step if pulled else m + step
                        found.append((int(kept.sum()) + (4 if pulled else 0), xc))
                    if kept is first:
                        undecidable[c] = bool(marginal.any()) or close
                        solved[c], x[c] = found[0]
                        pulled_total += solved[c] >= 4
                        candidates[c] = []
                    candidates[c] += [(code, (xc + ref).astype(np.float32)) for code, xc in found]
    verts_out = (x + ref).astype(np.float32)
    p = verts_out.astype(np.float64) - ref
    error = np.array([_quadric_value([[Q[0], Q[1], Q[2]], [Q[1], Q[3], Q[4]], [Q[2], Q[4], Q[5]]], Q[6:9], Q[9], p[c])
                      for c, Q in enumerate(qsums)])
    totals[7] = pulled_total
    out.update(verts=verts_out, members=count.astype(np.int64), error=error, solved=solved, cells=cells, mean=mean, mean_T=mean_T,
               mean_bound=mean_bound, undecidable=undecidable, candidates=candidates, items_max=int(max(count.max(), np.diff(qstarts).max())), quad=qsums)
    return out


# ---- exact and brute-force helpers of the tests -------------------------------------------------------------------------------
def exact_quadric(verts, tris, vert_map):
    """per output class the exact quadric (S 3x3, b, c as Fractions, with n and d from the float32 coordinates, no reference
    point) over the same (class, triangle) items -> function E(class, point as 3 floats) -> Fraction"""
    v = np.asarray(verts, np.float32)
    planes = {}
    for k, tri in enumerate(np.asarray(tris)):
        if tri[0] == tri[1] or tri[1] == tri[2] or tri[0] == tri[2]:
            continue
        A, B, C = ([Fraction(float(x)) for x in v[i]] for i in tri)
        e1 = [B[j] - A[j] for j in range(3)]
        e2 = [C[j] - A[j] for j in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        d = n[0] * A[0] + n[1] * A[1] + n[2] * A[2]
        for c in {int(vert_map[i]) for i in tri if vert_map[i] >= 0}:
            planes.setdefault(c, []).append((n, d))

    def E(c, point):
        P = [Fraction(float(x)) for x in point]
        return sum(((n[0] * P[0] + n[1] * P[1] + n[2] * P[2] - d) ** 2 for n, d in planes[c]), Fraction(0))

    def trace(c):
        return sum((n[0] ** 2 + n[1] ** 2 + n[2] ** 2 for n, _ in planes[c]), Fraction(0))

    E.trace = trace
    return E


def point_triangle_distance(p, a, b, c):
    """brute-force distance from point p to triangle abc (Ericson, Real-Time Collision Detection 5.1.5), float64"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return np.linalg.norm(ap)
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return np.linalg.norm(bp)
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return np.linalg.norm(ap - d1 / (d1 - d3) * ab)
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return np.linalg.norm(cp)
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return np.linalg.norm(ap - d2 / (d2 - d6) * ac)
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        return np.linalg.norm(p - (b + w * (c - b)))
    den = 1.0 / (va + vb + vc)
    return np.linalg.norm(p - (a + ab * (vb * den) + ac * (vc * den)))


def distance_to_mesh(points, verts, tris):
    """brute force: the distance of every point to the nearest triangle"""
    V = np.asarray(verts, np.float64)
    return np.array([min(point_triangle_distance(p, *V[tri]) for tri in tris) for p in points])
