"""Restatement of the mesh nesting (include/rho2sdf_hip.h, r2s_mesh_nesting) for tests/test_mesh_nesting_*.py, to the letter and
independent of the library's method: the patches and the closed flag come from tests/mesh_orient_ref.py, the pair test from
tests/mesh_winding_ref.py (_own_box, _pair); the crossings are a loop over ALL triangles of closed patches against the samples of
all patches, counted in a dict; containment is "odd", the depth a count and the parent a plain max.  No tree, no sort."""
import numpy as np

import mesh_orient_ref as O
import mesh_winding_ref as W

REWIND = 1
CLOSED, REVERSED, IRREGULAR = 1, 2, 4


def patches(verts, tris):
    """what does not depend on the ray -> dict: tris (nt, 3), patch_of_tri (nt,), first, n_tris (n,), closed (n,) bool, samples
    (n, 3) float64"""
    a = O.analyse(verts, tris)
    V = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    first = a["first"]
    samples = V[a["tris"][first, 0]] if len(first) else np.zeros((0, 3))
    return dict(tris=a["tris"], patch_of_tri=a["patch_of_tri"], first=first, n_tris=a["n_tris"],
                closed=(a["boundary"] == 0) & (a["nonmanifold"] == 0), samples=samples, verts=V, ok=a["ok"])


def nesting(verts, tris, ray=2, flags=0, pre=None):
    """-> dict: patch_of_tri (nt,) int32, counts (n, 8) int64, pairs (m,) int64 ascending, totals (8,) int64, tris (nt, 3) int32
    (the rewound triangles with REWIND, else None), cross {(P, Q): count}"""
    p = pre or patches(verts, tris)
    V, T, pot, closed, S = p["verts"], p["tris"], p["patch_of_tri"], p["closed"], p["samples"]
    n = len(p["first"])
    finite = np.ones(n, bool)
    cross = {}
    for t, (ia, ib, ic) in enumerate(T):
        Q = pot[t]
        if Q < 0 or not closed[Q]:                     # collapsed triangles and open patches take part in nothing
            continue
        a, b, c = V[ia], V[ib], V[ic]
        idx = np.nonzero(W._own_box(a, b, c, S, finite, ray))[0]
        idx = idx[idx != Q]                            # nor do the triangles of the query itself
        if idx.size == 0:
            continue
        hit = W._pair(a, b, c, S[idx], ray)[0]
        for P in idx[hit].tolist():
            cross[(P, int(Q))] = cross.get((P, int(Q)), 0) + 1
    containers = [[] for _ in range(n)]
    for (P, Q), k in cross.items():
        if k % 2 == 1:
            containers[P].append(Q)
    depth = np.array([len(c) for c in containers], np.int64).reshape(n)
    parent = np.full(n, -1, np.int64)
    for P in range(n):
        if containers[P]:
            parent[P] = max(containers[P], key=lambda Q: (depth[Q], -Q))   # the largest depth, among equals the smallest number
    irregular = np.array([depth[P] > 0 and depth[parent[P]] != depth[P] - 1 for P in range(n)], bool).reshape(n)
    pairs = np.array(sorted((P << 32) | Q for P in range(n) for Q in containers[P]), np.int64).reshape(-1)
    assert depth.sum() == len(pairs)
    rev = closed & (depth % 2 == 1) & bool(flags & REWIND)
    counts = np.zeros((n, 8), np.int64)
    counts[:, 0], counts[:, 1] = p["first"], p["n_tris"]
    counts[:, 2] = CLOSED * closed + REVERSED * rev + IRREGULAR * irregular
    counts[:, 3], counts[:, 4] = parent, depth
    counts[:, 5] = np.bincount(parent[parent >= 0], minlength=n)
    for (P, Q), k in cross.items():
        counts[P, 6] += k
    out = None
    if flags & REWIND:
        out = T.astype(np.int32)
        sel = (pot >= 0) & np.concatenate([rev, [False]])[pot]
        out[sel] = out[sel][:, [0, 2, 1]]
    totals = np.array([n, len(T), int((~p["ok"]).sum()), int(closed.sum()), len(pairs), int(depth.max()) if n else 0,
                       int(irregular.sum()), int(p["n_tris"][rev].sum())], np.int64)
    return dict(patch_of_tri=pot.astype(np.int32), counts=counts, pairs=pairs, totals=totals, tris=out, cross=cross)
