"""Restatement of the mesh orient (include/rho2sdf_hip.h, r2s_mesh_orient) for tests/test_mesh_orient_*.py, independent of the
library's method: the edge groups in a Python dict, the patches and the relative parity by a breadth-first walk from each
patch's smallest triangle over the groups of exactly two (a visited neighbour whose parity contradicts the walk makes the patch
non-orientable) - no union-find, no doubled graph.  The tentative volume V is the sequential float64 sum, in ascending triangle
index, of the volume terms of tests/mesh_shells_ref64.py, negated where rel = 1.  Beside V comes the shells' bound

    bound(p) = (n_tris(p) + 9) * 2^-53 * T(p)

(T the sum of the absolute values of the term's monomials, 9 the roundings on the term's longest chain), so that a caller can
see whether a decision by the sign of V is decidable: |V| is either exactly 0 or above the bound."""
from collections import deque

import numpy as np

import mesh_shells_ref64 as M

OUTWARD = 1
CLOSED, NONORIENTABLE, BY_VOLUME = 1, 2, 4


def analyse(verts, tris):
    """everything that does not depend on the flags -> dict: ok (nt,) bool, patch_of_tri, rel (nt,), first (n,), nonorientable
    (n,) bool, n_tris, n1, boundary, nonmanifold, flipped_in (n,), groups (the dict), V, T, bound (n,), ref_point"""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    nt = len(t)
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    groups = {}
    for ti in np.nonzero(ok)[0].tolist():
        for c in range(3):
            u, w = int(t[ti, c]), int(t[ti, (c + 1) % 3])
            groups.setdefault((min(u, w), max(u, w)), []).append((ti, u > w))
    partners = [[] for _ in range(nt)]                     # (neighbour, the two half-edges run in the same direction)
    for members in groups.values():
        if len(members) == 2:
            (a, da), (b, db) = members
            partners[a].append((b, da == db))
            partners[b].append((a, da == db))
    patch = np.full(nt, -1, np.int32)
    rel = np.zeros(nt, np.int32)
    first, nonor = [], []
    for f in range(nt):                                    # ascending: a new patch starts at its smallest triangle
        if not ok[f] or patch[f] >= 0:
            continue
        p = len(first)
        first.append(f)
        nonor.append(False)
        patch[f] = p
        queue = deque([f])
        while queue:
            a = queue.popleft()
            for b, same in partners[a]:
                want = rel[a] ^ int(same)
                if patch[b] < 0:
                    patch[b], rel[b] = p, want
                    queue.append(b)
                elif rel[b] != want:
                    nonor[p] = True
    n = len(first)
    nonor = np.array(nonor, bool).reshape(n)
    rel[(patch >= 0) & np.concatenate([nonor, [False]])[patch]] = 0   # no parity is defined there
    boundary, nonmanifold, flipped_in = (np.zeros(n, np.int64) for _ in range(3))
    for members in groups.values():
        if len(members) == 1:
            boundary[patch[members[0][0]]] += 1
        elif len(members) == 2:
            flipped_in[patch[members[0][0]]] += members[0][1] == members[1][1]
        else:
            for ti, _ in members:
                nonmanifold[patch[ti]] += 1
    r = M.ref_point(verts)
    x, T = M.terms(verts, t, r) if nt else (np.zeros((0, 11)), np.zeros((0, 11)))
    sign = 1.0 - 2.0 * rel
    V, Ts = np.zeros(n), np.zeros(n)
    order = np.argsort(patch, kind="stable")
    order = order[patch[order] >= 0]
    n_tris = np.bincount(patch[ok], minlength=n).astype(np.int64)
    ends = np.cumsum(n_tris)
    for p in range(n):
        idx = order[ends[p] - n_tris[p]:ends[p]]           # ascending triangle index
        V[p] = np.cumsum(sign[idx] * x[idx, 1])[-1]        # (a cumulative sum adds one term at a time)
        Ts[p] = T[idx, 1].sum()
    n1 = np.bincount(patch[ok], weights=rel[ok], minlength=n).astype(np.int64)
    return dict(ok=ok, patch_of_tri=patch, rel=rel, first=np.array(first, np.int64).reshape(n), nonorientable=nonor, n_tris=n_tris,
                n1=n1, boundary=boundary, nonmanifold=nonmanifold, flipped_in=flipped_in, groups=groups, V=V, T=Ts,
                bound=(n_tris + 9.0) * 2.0 ** -53 * Ts, ref_point=r, tris=t)


def decide(a, flags):
    """the restated result under `flags` -> dict: tris, flip, patch_of_tri, counts (n, 8), volume (n,), totals (8,), ref_point,
    g (n,), bound (n,)"""
    n = len(a["first"])
    closed = (a["boundary"] == 0) & (a["nonmanifold"] == 0)
    orientable = ~a["nonorientable"]
    by_volume = orientable & closed & (a["V"] != 0) & bool(flags & OUTWARD)
    n0 = a["n_tris"] - a["n1"]
    g = np.where(by_volume, a["V"] < 0, a["n1"] > n0) & orientable
    patch, ok = a["patch_of_tri"], a["ok"]
    flip = np.zeros(len(patch), np.int32)
    flip[ok] = a["rel"][ok] ^ g[patch[ok]]
    flip[ok] *= orientable[patch[ok]]
    out = a["tris"].astype(np.int32)
    sel = flip == 1
    out[sel] = out[sel][:, [0, 2, 1]]
    counts = np.zeros((n, 8), np.int64)
    counts[:, 0], counts[:, 1] = a["first"], a["n_tris"]
    counts[:, 2] = np.bincount(patch[ok], weights=flip[ok], minlength=n).astype(np.int64)
    counts[:, 3] = CLOSED * closed + NONORIENTABLE * a["nonorientable"] + BY_VOLUME * by_volume
    counts[:, 4], counts[:, 5], counts[:, 6] = a["boundary"], a["nonmanifold"], a["flipped_in"]
    remaining = 0
    for members in a["groups"].values():
        if len(members) == 2:
            (ta, da), (tb, db) = members
            remaining += (bool(da) ^ bool(flip[ta])) == (bool(db) ^ bool(flip[tb]))
    totals = np.array([n, len(patch), int((~ok).sum()), int(flip.sum()), int(a["nonorientable"].sum()), int(closed.sum()),
                       int(by_volume.sum()), int(remaining)], np.int64)
    return dict(tris=out, flip=flip, patch_of_tri=patch, counts=counts, volume=np.where(g, -a["V"], a["V"]), totals=totals,
                ref_point=a["ref_point"], g=g, bound=a["bound"])


def orient(verts, tris, flags=0):
    return decide(analyse(verts, tris), flags)
