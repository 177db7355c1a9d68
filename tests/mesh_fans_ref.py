"""Plain-Python restatement of the mesh fans (include/rho2sdf_hip.h, r2s_mesh_fans) for tests/test_mesh_fans_*.py.  It shares no
code and no method with the library: a dictionary from undirected edge to its half-edges, a breadth-first walk over the corners of
every vertex, the fans numbered by sorting (vertex, first_corner), the records counted from Python sets, the split by the
header's rule.  The invariants the header states for closed and open fans are asserted here on every mesh that passes through."""
from collections import deque

import numpy as np


def fans(verts, tris, split=True):
    """-> dict(fan_of_corner (nt, 3) int32, fans_of_vert (nv,) int32, counts (n, 8) int64, totals (8,) int64, n_added and, with
    split, verts (nv_out, 3) float32, tris (nt, 3) int32, vert_of (nv_out,) int32)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    nv, nt = len(v), len(t)
    T = t.tolist()
    ok = [len(set(tri)) == 3 for tri in T]
    edges = {}                                        # (min, max) -> [(triangle, direction)]
    for ti, tri in enumerate(T):
        if ok[ti]:
            for c in range(3):
                u, w = tri[c], tri[(c + 1) % 3]
                edges.setdefault((min(u, w), max(u, w)), []).append((ti, u > w))
    at = {}                                           # vertex -> its corners, ascending
    for ti, tri in enumerate(T):
        if ok[ti]:
            for c in range(3):
                at.setdefault(tri[c], []).append(3 * ti + c)
    corner_of = lambda ti, vert: 3 * ti + T[ti].index(vert)   # noqa: E731

    def edges_of(k):
        ti, c = divmod(k, 3)
        a, b, p = T[ti][c], T[ti][(c + 1) % 3], T[ti][(c + 2) % 3]
        return (min(a, b), max(a, b)), (min(a, p), max(a, p))

    found = []                                        # (vertex, first_corner, sorted corners)
    for vert, corners in at.items():
        seen = set()
        for k0 in corners:
            if k0 in seen:
                continue
            seen.add(k0)
            comp, queue = [], deque([k0])
            while queue:
                k = queue.popleft()
                comp.append(k)
                for e in edges_of(k):
                    for ti, _ in edges[e]:
                        k2 = corner_of(ti, vert)
                        if k2 not in seen:
                            seen.add(k2)
                            queue.append(k2)
            found.append((vert, min(comp), sorted(comp)))
    found.sort(key=lambda f: (f[0], f[1]))
    n = len(found)
    foc = np.full(3 * nt, -1, np.int32)
    fov = np.zeros(nv, np.int32)
    counts = np.zeros((n, 8), np.int64)
    for f, (vert, first, comp) in enumerate(found):
        foc[comp] = f
        fov[vert] += 1
        es = set()
        for k in comp:
            es.update(edges_of(k))
        nb = sum(1 for e in es if len(edges[e]) == 1)
        nf = sum(1 for e in es if len(edges[e]) == 2 and edges[e][0][1] == edges[e][1][1])
        nm = sum(1 for e in es if len(edges[e]) >= 3)
        cls = 2 if nm else (1 if nb else 0)
        counts[f] = [vert, first, len(comp), len(es), nb, nf, nm, cls]
        # the invariants of the header: a closed fan is a single cycle, an open fan a single path
        if cls == 0:
            assert len(es) == len(comp), (vert, first)
        elif cls == 1:
            assert nb == 2 and len(es) == len(comp) + 1, (vert, first)
    used = int((fov > 0).sum())
    totals = np.array([n, nt, nt - sum(ok), used, nv - used, int((fov >= 2).sum()), int((counts[:, 7] == 2).sum()),
                       int((counts[:, 7] == 1).sum())], np.int64)
    out = dict(fan_of_corner=foc.reshape(-1, 3), fans_of_vert=fov, counts=counts, totals=totals, n_added=n - used)
    if split:
        index_of, vert_of = np.empty(n, np.int64), list(range(nv))
        for f, (vert, _, _) in enumerate(found):
            if f == 0 or found[f - 1][0] != vert:
                index_of[f] = vert
            else:
                index_of[f] = len(vert_of)
                vert_of.append(vert)
        flat = t.reshape(-1).copy()
        has = foc >= 0
        flat[has] = index_of[foc[has]]
        vert_of = np.array(vert_of, np.int32)
        assert len(vert_of) == nv + n - used
        out.update(verts=v[vert_of], tris=flat.reshape(-1, 3).astype(np.int32), vert_of=vert_of)
    return out
