"""numpy restatement of the mesh weld (include/rho2sdf_hip.h, r2s_mesh_weld) for tests/test_mesh_weld_*.py.  It shares no code
with the library: classes come from np.unique on the canonicalised key triples, the representative of a class is its smallest
index, everything after that is plain integer code on Python tuples and sets."""
import numpy as np

DROP_COLLAPSED, DROP_DUPLICATES, DROP_UNUSED = 1, 2, 4


class SnapTooFine(ValueError):
    pass


def keys(verts, snap):
    """(n, 3) integer key triples: equal rows <=> the same vertex"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    if snap == 0:
        k = v.copy()
        k[k == 0] = np.float32(0.0)                 # -0.0 == +0.0: both become +0.0
        return k.view(np.uint32).astype(np.int64)   # equal float32 values (no NaN here) have equal bits after that
    with np.errstate(over="ignore"):
        q = np.floor(v.astype(np.float64) / np.float64(snap))   # one division in double, then floor
    if not (np.isfinite(q).all() and (q >= -2.0 ** 31).all() and (q < 2.0 ** 31).all()):
        raise SnapTooFine("snap is too fine for the extent")
    return q.astype(np.int64)


def canonical(tri):
    """the rotation of (a, b, c) that starts with the smallest index"""
    a, b, c = tri
    m = min(a, b, c)
    return (a, b, c) if a == m else ((b, c, a) if b == m else (c, a, b))


def weld(verts, tris=None, snap=0.0, flags=DROP_COLLAPSED | DROP_UNUSED):
    """-> dict(verts, tris, vert_map, tri_map, totals, rep): rep[j] is the input index of output vertex j"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    nv = len(v)
    if tris is None:
        assert nv % 3 == 0
        T = np.arange(nv, dtype=np.int64).reshape(-1, 3)
    else:
        T = np.asarray(tris, np.int64).reshape(-1, 3)
    nt = len(T)
    if nv:
        _, inv = np.unique(keys(v, snap), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        ncls = int(inv.max()) + 1
        first = np.full(ncls, nv, np.int64)
        np.minimum.at(first, inv, np.arange(nv))                 # the smallest index of every class
        number = np.empty(ncls, np.int64)
        number[np.argsort(first)] = np.arange(ncls)              # classes numbered by ascending representative
        class_of, rep = number[inv], np.sort(first)
    else:
        ncls, class_of, rep = 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    R = [tuple(int(class_of[i]) for i in t) for t in T]
    collapsed = [len(set(r)) < 3 for r in R]
    seen, dup, orient = set(), [False] * nt, {}
    for t, r in enumerate(R):
        if collapsed[t]:
            continue
        c = canonical(r)
        dup[t] = c in seen
        seen.add(c)
        orient.setdefault(tuple(sorted(r)), set()).add(c)
    opposite = sum(1 for s in orient.values() if len(s) == 2)
    keep = [not (collapsed[t] and flags & DROP_COLLAPSED) and not (dup[t] and flags & DROP_DUPLICATES) for t in range(nt)]
    used = np.zeros(ncls, bool)
    for t in range(nt):
        if keep[t]:
            used[list(R[t])] = True
    if flags & DROP_UNUSED:
        final = np.where(used, np.cumsum(used) - 1, -1)
        kept = np.nonzero(used)[0]
    else:
        final, kept = np.arange(ncls), np.arange(ncls)
    tri_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32) if nt else np.zeros(0, np.int32)
    tris_out = np.array([[final[c] for c in R[t]] for t in range(nt) if keep[t]], np.int32).reshape(-1, 3)
    totals = np.array([len(kept), int(sum(keep)), nv - ncls, int(sum(collapsed)), int(sum(dup)), opposite,
                       int(ncls - used.sum()), 0], np.int64)
    return dict(verts=v[rep[kept]], tris=tris_out, vert_map=final[class_of].astype(np.int32), tri_map=tri_map, totals=totals,
                rep=rep[kept])
