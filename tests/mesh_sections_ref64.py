"""Float64 restatement of the mesh sections (include/rho2sdf_hip.h, r2s_mesh_sections) for tests/test_mesh_sections_*.py:
heights in numpy in the header's operation order, segments and nodes in plain Python, nodes grouped by a dict keyed
(level, min, max), a dictionary union-find, loops walked along the successors, the terms in numpy in the header's order,
summed sequentially in output order.  Beside every Float64 sum it returns T, the sum over the contour's segments of the
absolute values of the term's monomials in A = from - r and B = to - r, and the bound of the header:

    bound(c) = (n_segs(c) + K) * 2^-53 * T(c)

K = the roundings on the longest chain of the term, a product counting the chains of both factors (to first order the
computed term is the sum of its monomials, each times (1 + d)^K with |d| <= 2^-53; n_segs more for the additions of any
summation order).  The points are the data here: their own roundings are the same bits for every summation order.
    A = from - r, B = to - r                     1
    D = B - A                                    2
    length = sqrt((D*D + D*D) + D*D)             D*D: 2*2 + 1 = 5, two sums: 7, sqrt halves and adds one: 4.5 -> K = 5
    C = A*B - A*B                                1 + 1 + 1 (product) + 1 (difference) = 4
    w = (n*C + n*C) + n*C                        4 + 1 (product; n is exact) + 2 (sums) = 7
    moment = w * (A + B)                         A + B: 2; 7 + 2 + 1 = 10"""
import numpy as np

from mesh_shells_ref64 import ref_point

K = np.array([5, 4, 4, 4, 10, 10, 10], np.float64)
NAMES = ("length", "C_x", "C_y", "C_z", "m_x", "m_y", "m_z")


def heights(verts, normal):
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    n = np.asarray(normal, np.float64)
    return (n[0] * v[:, 0] + n[1] * v[:, 1]) + n[2] * v[:, 2]


def node_point(v, h, i, j, c):
    """the point of node (level value c, edge {i, j}) from the smaller index"""
    i, j = (i, j) if i < j else (j, i)
    t = (c - h[i]) / (h[j] - h[i])
    assert 0.0 <= t <= 1.0
    return v[i] + t * (v[j] - v[i])


def terms(pts, r, normal):
    """-> (terms (m, 7), T (m, 7)) of the segments pts (m, 2, 3) in the header's order, and the absolute monomial sums"""
    n = np.asarray(normal, np.float64)
    A, B = pts[:, 0] - r, pts[:, 1] - r
    D = B - A
    x, y, z = 0, 1, 2
    C = np.stack([A[:, y] * B[:, z] - A[:, z] * B[:, y], A[:, z] * B[:, x] - A[:, x] * B[:, z], A[:, x] * B[:, y] - A[:, y] * B[:, x]], -1)
    w = (n[0] * C[:, 0] + n[1] * C[:, 1]) + n[2] * C[:, 2]
    out = np.empty((len(pts), 7))
    out[:, 0] = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
    out[:, 1:4] = C
    out[:, 4:7] = w[:, None] * (A + B)
    a, b = np.abs(A), np.abs(B)
    Tc = np.stack([a[:, y] * b[:, z] + a[:, z] * b[:, y], a[:, z] * b[:, x] + a[:, x] * b[:, z], a[:, x] * b[:, y] + a[:, y] * b[:, x]], -1)
    T = np.empty_like(out)
    T[:, 0] = np.sqrt(((a + b) ** 2).sum(-1))
    T[:, 1:4] = Tc
    T[:, 4:7] = (Tc @ np.abs(n))[:, None] * (a + b)
    return out, T


def sections(verts, tris, normal, levels):
    """the restated result: a dict with contour_start, seg_tri, seg_id, seg_points, counts, totals, ref_point, sums, T, bound
    (all (n, 7)) and terms (per output position)"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    lev = np.asarray(levels, np.float64).reshape(-1)
    h = heights(verts, normal)
    r = ref_point(verts)
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    seg_tri, seg_level, ends = [], [], []          # per segment id: triangle, level, (from edge, to edge)
    nodes = {}                                     # (level, i, j) -> [(segment, kind)], kind 0 = outgoing (from), 1 = incoming (to)
    for ti in np.nonzero(ok)[0].tolist():
        i = [int(q) for q in t[ti]]
        hh = [h[q] for q in i]
        first = int(np.searchsorted(lev, min(hh), side="right"))      # the levels <= hmin: all three vertices above
        end = int(np.searchsorted(lev, max(hh), side="right"))
        for k in range(first, end):
            above = [x >= lev[k] for x in hh]
            s = len(seg_tri)
            fr = to = None
            for c in range(3):
                u, w = c, (c + 1) % 3
                if above[u] != above[w]:
                    e = (min(i[u], i[w]), max(i[u], i[w]))
                    nodes.setdefault((k,) + e, []).append((s, 0 if above[u] else 1))
                    if above[u]:
                        assert fr is None
                        fr = e
                    else:
                        assert to is None
                        to = e
            assert fr is not None and to is not None
            seg_tri.append(ti)
            seg_level.append(k)
            ends.append((fr, to))
    m = len(seg_tri)
    parent = {s: s for s in range(m)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    succ = {}
    for members in nodes.values():
        for (a, _), (b, _) in zip(members, members[1:]):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(s) for s in range(m)], np.int64)
    roots = sorted({int(x) for x in root}, key=lambda x: (seg_level[x], x))
    number = {x: c for c, x in enumerate(roots)}
    contour = np.array([number[int(x)] for x in root], np.int64)
    n = len(roots)
    counts = np.zeros((n, 8), np.int64)
    counts[:, 0] = [seg_level[x] for x in roots]
    counts[:, 1] = roots
    counts[:, 2] = np.bincount(contour, minlength=n)
    for members in nodes.values():
        c = contour[members[0][0]]
        counts[c, 3] += 1
        if len(members) == 1:
            counts[c, 4] += 1
        elif len(members) == 2 and members[0][1] == members[1][1]:
            counts[c, 5] += 1
        elif len(members) == 2:
            out, inc = (members[0][0], members[1][0]) if members[0][1] == 0 else (members[1][0], members[0][0])
            succ[inc] = out
        else:
            counts[c, 6] += 1
    closed = (counts[:, 4] == 0) & (counts[:, 5] == 0) & (counts[:, 6] == 0)
    order = []
    by_contour = [[] for _ in range(n)]
    for s in range(m):
        by_contour[contour[s]].append(s)
    for c in range(n):
        if closed[c]:
            walk, s = [], int(counts[c, 1])
            for _ in range(int(counts[c, 2])):
                walk.append(s)
                s = succ[s]
            assert s == counts[c, 1] and sorted(walk) == by_contour[c]      # one simple cycle
            order += walk
        else:
            order += by_contour[c]
    start = np.concatenate([[0], np.cumsum(counts[:, 2])]).astype(np.int64) if n else np.zeros(1, np.int64)
    pts = np.empty((m, 2, 3))
    for p, s in enumerate(order):
        k = seg_level[s]
        pts[p, 0] = node_point(v, h, *ends[s][0], lev[k])
        pts[p, 1] = node_point(v, h, *ends[s][1], lev[k])
    x, T = terms(pts, r, normal)
    sums, Ts = np.zeros((n, 7)), np.zeros((n, 7))
    for c in range(n):
        sums[c] = np.cumsum(x[start[c]:start[c + 1]], axis=0)[-1]          # (a cumulative sum adds one term at a time)
        Ts[c] = T[start[c]:start[c + 1]].sum(0)
    totals = np.array([n, m, int((~ok).sum())] + counts[:, 3:7].sum(0).tolist() + [int(closed.sum())], np.int64)
    return dict(contour_start=start, seg_tri=np.array(seg_tri, np.int32)[order] if m else np.zeros(0, np.int32),
                seg_id=np.array(order, np.int64), seg_points=pts, counts=counts, totals=totals, ref_point=r, sums=sums, T=Ts,
                bound=bound(counts[:, 2], Ts), terms=x, closed=closed, levels=lev, normal=np.asarray(normal, np.float64))


def bound(n_segs, T):
    return (np.asarray(n_segs, np.float64)[:, None] + K[None, :]) * 2.0 ** -53 * T
