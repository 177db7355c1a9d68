"""Plain-Python restatement of the mesh holes (include/rho2sdf_hip.h, r2s_mesh_holes) for tests/test_mesh_holes_*.py.  It shares
no code and no method with the library: a dictionary from undirected edge to its half-edges, a dictionary from vertex to the
boundary ends at it, a breadth-first walk over the boundary half-edges for the rims and a walk along the successors for the
order of a closed rim.  The Float64 sums are computed twice: in numpy float64 in the header's operation order, summed one term
at a time in output order, and exactly in Fractions.  On every mesh that passes through it asserts

    |float64 sum - exact sum| <= bound = (n_edges + K) * 2^-53 * T

(T = the sum of the absolute values of the term's monomials in A = from - r and B = to - r, K = the roundings on the longest
chain of the term, counted as tests/mesh_sections_ref64.py counts them), and that a closed rim is one cycle of distinct vertices
with n_edges == n_nodes >= 3.
    A = from - r, B = to - r                     1
    D = B - A                                    2
    length = sqrt((D*D + D*D) + D*D)             D*D: 2*2 + 1 = 5, two sums: 7, sqrt halves and adds one: 4.5 -> K = 5
    A x B = A*B - A*B                            1 + 1 + 1 (product) + 1 (difference) = 4
    A                                            1
The exact length is irrational: it is taken as the Fraction of a square root computed with 60 digits (an error of 1e-60
relative, far below 2^-53), the other six sums are exact."""
from collections import deque
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

from mesh_shells_ref64 import ref_point

K = np.array([5, 4, 4, 4, 1, 1, 1], np.float64)
NAMES = ("length", "AxB_x", "AxB_y", "AxB_z", "A_x", "A_y", "A_z")
worst_vertex_fraction = 0.0   # the largest fraction of the added-vertex bound any mesh has used (vertex_bound below)


def _sqrt(q):
    with localcontext() as ctx:
        ctx.prec = 60
        return Fraction((Decimal(q.numerator) / Decimal(q.denominator)).sqrt())


def terms(frm, to, r):
    """-> (terms (m, 7) float64 in the header's order, T (m, 7)) of the half-edges frm -> to (m, 3) float64"""
    A, B = frm - r, to - r
    D = B - A
    x, y, z = 0, 1, 2
    out = np.empty((len(frm), 7))
    out[:, 0] = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
    out[:, 1] = A[:, y] * B[:, z] - A[:, z] * B[:, y]
    out[:, 2] = A[:, z] * B[:, x] - A[:, x] * B[:, z]
    out[:, 3] = A[:, x] * B[:, y] - A[:, y] * B[:, x]
    out[:, 4:7] = A
    a, b = np.abs(A), np.abs(B)
    T = np.empty_like(out)
    T[:, 0] = np.sqrt(((a + b) ** 2).sum(-1))
    T[:, 1] = a[:, y] * b[:, z] + a[:, z] * b[:, y]
    T[:, 2] = a[:, z] * b[:, x] + a[:, x] * b[:, z]
    T[:, 3] = a[:, x] * b[:, y] + a[:, y] * b[:, x]
    T[:, 4:7] = a
    return out, T


def exact_terms(frm, to, r):
    """the seven terms of one half-edge as Fractions (frm, to, r: sequences of floats)"""
    A = [Fraction(float(p)) - Fraction(float(q)) for p, q in zip(frm, r)]
    B = [Fraction(float(p)) - Fraction(float(q)) for p, q in zip(to, r)]
    D = [b - a for a, b in zip(A, B)]
    return [_sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]), A[1] * B[2] - A[2] * B[1], A[2] * B[0] - A[0] * B[2],
            A[0] * B[1] - A[1] * B[0], A[0], A[1], A[2]]


def bound(n_edges, T):
    return (np.asarray(n_edges, np.float64)[:, None] + K[None, :]) * 2.0 ** -53 * T


def vertex_bound(c, sum_bound, n_edges):
    """the bound of an added vertex against the exact mean c (Fractions, per axis): the float32 rounding of c (2^-24 |c| plus one
    denormal step), the sum's bound divided by n_edges, the two double roundings (2^-52 |c|)"""
    c = np.array([abs(float(q)) for q in c])
    return 2.0 ** -24 * c + 2.0 ** -149 + np.asarray(sum_bound) / n_edges + 2.0 ** -52 * c


def holes(verts, tris, fill=None):
    """the restated result: a dict with rim_start, rim_edge, counts (n, 8), totals, ref_point, sums / exact (as float) / T /
    bound (all (n, 7)), exact_sums (Fractions) and, with fill = max_edges, verts, tris and exact_added (the exact means of the
    added vertices, Fractions) and added_bound"""
    global worst_vertex_fraction
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    nv, nt = len(v), len(t)
    T = t.tolist()
    ok = [len(set(tri)) == 3 for tri in T]
    r = ref_point(verts)
    edges = {}                                        # (min, max) -> [half-edge id]
    for ti, tri in enumerate(T):
        if ok[ti]:
            for c in range(3):
                u, w = tri[c], tri[(c + 1) % 3]
                edges.setdefault((min(u, w), max(u, w)), []).append(3 * ti + c)
    boundary = sorted(g[0] for g in edges.values() if len(g) == 1)
    frm = {h: T[h // 3][h % 3] for h in boundary}
    to = {h: T[h // 3][(h % 3 + 1) % 3] for h in boundary}
    ends = {}                                         # vertex -> [(half-edge, kind)], kind 0 outgoing, 1 incoming
    for h in boundary:
        ends.setdefault(frm[h], []).append((h, 0))
        ends.setdefault(to[h], []).append((h, 1))

    def node_class(vert):
        e = ends[vert]
        if len(e) == 1:
            return 1
        if len(e) >= 3:
            return 3
        return 0 if e[0][1] != e[1][1] else 2

    succ = {}
    for vert, e in ends.items():
        if node_class(vert) == 0:
            (h0, k0), (h1, _) = e
            inc, out = (h0, h1) if k0 == 1 else (h1, h0)
            succ[inc] = out
    seen, rims = set(), []                            # rims in ascending smallest half-edge: boundary is ascending
    for h0 in boundary:
        if h0 in seen:
            continue
        seen.add(h0)
        comp, queue = [], deque([h0])
        while queue:
            h = queue.popleft()
            comp.append(h)
            for vert in (frm[h], to[h]):
                for h2, _ in ends[vert]:
                    if h2 not in seen:
                        seen.add(h2)
                        queue.append(h2)
        rims.append(sorted(comp))
    n = len(rims)
    counts = np.zeros((n, 8), np.int64)
    order = []
    for c, comp in enumerate(rims):
        nodes = sorted({frm[h] for h in comp} | {to[h] for h in comp})
        cls = [node_class(x) for x in nodes]
        counts[c, :6] = [comp[0], len(comp), len(nodes), cls.count(1), cls.count(2), cls.count(3)]
        closed = cls.count(0) == len(cls)
        counts[c, 6], counts[c, 7] = int(closed), -1
        if closed:
            walk, h = [], comp[0]
            for _ in range(len(comp)):
                walk.append(h)
                h = succ[h]
            # one simple cycle of distinct vertices
            assert h == comp[0] and sorted(walk) == comp and len(comp) == len(nodes) >= 3, c
            assert len({frm[q] for q in walk}) == len(walk)
            order += walk
        else:
            order += comp
    start = np.concatenate([[0], np.cumsum(counts[:, 1])]).astype(np.int64) if n else np.zeros(1, np.int64)
    m = len(order)
    F = v[[frm[h] for h in order]] if m else np.zeros((0, 3))
    G = v[[to[h] for h in order]] if m else np.zeros((0, 3))
    x, Tt = terms(F, G, r)
    sums, Ts = np.zeros((n, 7)), np.zeros((n, 7))
    exact = []
    for c in range(n):
        lo, hi = int(start[c]), int(start[c + 1])
        sums[c] = np.cumsum(x[lo:hi], axis=0)[-1]     # (a cumulative sum adds one term at a time)
        Ts[c] = Tt[lo:hi].sum(0)
        ex = [Fraction(0)] * 7
        for p in range(lo, hi):
            ex = [a + b for a, b in zip(ex, exact_terms(F[p], G[p], r))]
        exact.append(ex)
    bnd = bound(counts[:, 1], Ts)
    exact_f = np.array([[float(q) for q in ex] for ex in exact]).reshape(n, 7)
    for c in range(n):
        for q in range(7):
            assert abs(Fraction(float(sums[c, q])) - exact[c][q]) <= Fraction(float(bnd[c, q])), (c, NAMES[q])
    closed = counts[:, 6] == 1
    nodes_total = len(ends)
    irregular = int(counts[:, 3:6].sum())
    out = dict(rim_start=start, rim_edge=np.array(order, np.int32), counts=counts, ref_point=r, sums=sums, exact=exact_f,
               exact_sums=exact, T=Ts, bound=bnd)
    filled = added_t = 0
    if fill is not None:
        V2, T2, exact_added, added_bound = [v32], [t.astype(np.int32)], [], []
        for c in range(n):
            ne = int(counts[c, 1])
            if not closed[c] or fill == 0 or (fill > 0 and ne > fill):
                continue
            filled += 1
            walk = order[int(start[c]):int(start[c + 1])]
            if ne == 3:
                a, b, cc = frm[walk[0]], to[walk[0]], to[walk[1]]
                assert frm[walk[1]] == b and frm[walk[2]] == cc and to[walk[2]] == a
                T2.append(np.array([[b, a, cc]], np.int32))
                counts[c, 6] = 2
                added_t += 1
                continue
            w = nv + len(exact_added)
            mean = [Fraction(float(r[k])) + exact[c][4 + k] / ne for k in range(3)]
            got = np.array([np.float32(r[k] + sums[c, 4 + k] / ne) for k in range(3)], np.float32)
            vb = vertex_bound(mean, bnd[c, 4:7], ne)
            for k in range(3):
                err = abs(Fraction(float(got[k])) - mean[k])
                assert err <= Fraction(float(vb[k])), (c, k)
                worst_vertex_fraction = max(worst_vertex_fraction, float(err) / vb[k])
            exact_added.append(mean)
            added_bound.append(vb)
            V2.append(got[None, :])
            T2.append(np.array([[to[h], frm[h], w] for h in walk], np.int32))
            counts[c, 6], counts[c, 7] = 3, w
            added_t += ne
        out.update(verts=np.concatenate(V2), tris=np.concatenate(T2), exact_added=exact_added,
                   added_bound=np.array(added_bound).reshape(-1, 3))
    out["totals"] = np.array([n, len(boundary), nt - sum(ok), nodes_total, irregular, int(closed.sum()), filled, added_t], np.int64)
    return out
