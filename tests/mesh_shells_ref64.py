"""Float64 restatement of the mesh shells (include/rho2sdf_hip.h, r2s_mesh_shells) for tests/test_mesh_shells_*.py: edges
grouped by a dict, union-find in Python, the terms in numpy in the header's operation order, summed sequentially in ascending
triangle order.  Beside every Float64 sum it returns T, the sum over the shell's triangles of the absolute values of the
term's monomials in A, B, C, and the bound of the header:

    bound(s) = (n_tris(s) + K) * 2^-53 * T(s)

K = the roundings on the longest chain of the term, a product counting the chains of both factors (to first order the
computed term is the sum of its monomials, each times (1 + d)^K with |d| <= 2^-53; n_tris more for the additions of any
summation order):
    A = a - r                                    1     (likewise B, C)
    S = (A + B) + C                              3
    E = B - A, F = C - A                         2
    N = E*F - E*F                                2 + 2 + 1 (product) + 1 (difference) = 6 as a product, 4 on one chain
    area = 0.5 * sqrt((N*N + N*N) + N*N)         N*N: 2*4 + 1 = 9, two sums: 11, sqrt halves and adds one: 6.5 -> K = 8
    det = (A*(B*C - B*C) + A*(..)) + A*(..)      B*C: 3, difference: 4, times A: 6, two sums: 8 -> volume = det / 6: K = 9
    first = (det * S) / 24                       8 + 3 + 1 + 1 = 13
    Q = ((A*A + B*B) + C*C) + S*S                A*A: 3, three sums: 6; S*S: 7, last sum: 8
    second = (det * Q) / 120                     8 + 8 + 1 + 1 = 18"""
import numpy as np

K = np.array([8, 9, 13, 13, 13, 18, 18, 18, 18, 18, 18], np.float64)
NAMES = ("area", "volume", "m_x", "m_y", "m_z", "m_xx", "m_yy", "m_zz", "m_xy", "m_xz", "m_yz")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def ref_point(verts):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    if len(v) == 0:
        return np.zeros(3)
    return 0.5 * (v.min(0).astype(np.float64) + v.max(0).astype(np.float64))


def terms(verts, tris, r):
    """-> (terms (nt, 11), T (nt, 11)): every triangle's terms in the header's order, and the absolute monomial sums"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(tris).reshape(-1, 3)
    A, B, C = v[t[:, 0]] - r, v[t[:, 1]] - r, v[t[:, 2]] - r
    S = (A + B) + C
    E, F = B - A, C - A
    x, y, z = 0, 1, 2
    N = np.stack([E[:, y] * F[:, z] - E[:, z] * F[:, y], E[:, z] * F[:, x] - E[:, x] * F[:, z], E[:, x] * F[:, y] - E[:, y] * F[:, x]], -1)
    out = np.empty((len(t), 11))
    out[:, 0] = 0.5 * np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    det = (A[:, x] * (B[:, y] * C[:, z] - B[:, z] * C[:, y]) + A[:, y] * (B[:, z] * C[:, x] - B[:, x] * C[:, z])) \
        + A[:, z] * (B[:, x] * C[:, y] - B[:, y] * C[:, x])
    out[:, 1] = det / 6.0
    for i in range(3):
        out[:, 2 + i] = (det * S[:, i]) / 24.0
    for q, (i, j) in enumerate(PAIRS):
        out[:, 5 + q] = (det * (((A[:, i] * A[:, j] + B[:, i] * B[:, j]) + C[:, i] * C[:, j]) + S[:, i] * S[:, j])) / 120.0
    a, b, c = np.abs(A), np.abs(B), np.abs(C)
    s = a + b + c
    e, f = a + b, a + c
    M = np.stack([e[:, y] * f[:, z] + e[:, z] * f[:, y], e[:, z] * f[:, x] + e[:, x] * f[:, z], e[:, x] * f[:, y] + e[:, y] * f[:, x]], -1)
    T = np.empty_like(out)
    T[:, 0] = 0.5 * np.sqrt((M * M).sum(-1))
    D = a[:, x] * (b[:, y] * c[:, z] + b[:, z] * c[:, y]) + a[:, y] * (b[:, z] * c[:, x] + b[:, x] * c[:, z]) \
        + a[:, z] * (b[:, x] * c[:, y] + b[:, y] * c[:, x])
    T[:, 1] = D / 6.0
    for i in range(3):
        T[:, 2 + i] = D * s[:, i] / 24.0
    for q, (i, j) in enumerate(PAIRS):
        T[:, 5 + q] = D * (a[:, i] * a[:, j] + b[:, i] * b[:, j] + c[:, i] * c[:, j] + s[:, i] * s[:, j]) / 120.0
    return out, T


def topology(tris):
    """-> (shell_of_tri (nt,) int32, counts (n, 8) int64, totals (8,) int64 with [7] = referenced vertices)"""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    nt = len(t)
    ok = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    parent = list(range(nt))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    groups = {}
    for ti in np.nonzero(ok)[0].tolist():
        for c in range(3):
            u, w = int(t[ti, c]), int(t[ti, (c + 1) % 3])
            groups.setdefault((min(u, w) << 32) | max(u, w), []).append((ti, u > w))
    for members in groups.values():
        for (a, _), (b, _) in zip(members, members[1:]):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) if ok[i] else -1 for i in range(nt)], np.int64)
    roots = np.unique(root[ok])                                 # ascending smallest triangle index
    number = {int(r): k for k, r in enumerate(roots)}
    shell = np.array([number[int(r)] if r >= 0 else -1 for r in root], np.int32)
    n = len(roots)
    counts = np.zeros((n, 8), np.int64)
    counts[:, 0] = roots
    counts[:, 1] = np.bincount(shell[ok], minlength=n)
    for s in range(n) if n < 64 else ():
        counts[s, 2] = len(np.unique(t[shell == s]))
    if n >= 64:
        sv = np.unique(np.stack([np.repeat(shell[ok], 3), t[ok].ravel()], -1), axis=0)
        counts[:, 2] = np.bincount(sv[:, 0], minlength=n)
    for members in groups.values():
        s = shell[members[0][0]]
        counts[s, 3] += 1
        if len(members) == 1:
            counts[s, 4] += 1
        elif len(members) == 2:
            counts[s, 5] += members[0][1] == members[1][1]
        else:
            counts[s, 6] += 1
    totals = np.array([n, nt, int((~ok).sum())] + counts[:, 3:7].sum(0).tolist() + [len(np.unique(t[ok]))], np.int64)
    return shell, counts, totals


def shells(verts, tris):
    """the restated result: a dict with shell_of_tri, counts, totals, ref_point, sums, T and bound (all (n, 11))"""
    shell, counts, totals = topology(tris)
    r = ref_point(verts)
    x, T = terms(verts, tris, r)
    n = len(counts)
    sums, Ts = np.zeros((n, 11)), np.zeros((n, 11))
    order = np.argsort(shell, kind="stable")
    order = order[shell[order] >= 0]
    ends = np.cumsum(counts[:, 1])
    for s in range(n):
        idx = order[ends[s] - counts[s, 1]:ends[s]]            # ascending triangle index
        sums[s] = np.cumsum(x[idx], axis=0)[-1]                # (a cumulative sum adds one term at a time)
        Ts[s] = T[idx].sum(0)
    return dict(shell_of_tri=shell, counts=counts, totals=totals, ref_point=r, sums=sums, T=Ts, bound=bound(counts[:, 1], Ts),
                terms=x)


def bound(n_tris, T):
    return (np.asarray(n_tris, np.float64)[:, None] + K[None, :]) * 2.0 ** -53 * T
