"""numpy restatement of the iso-surface's vertex definition (include/rho2sdf_hip.h, r2s_extract_isosurface) and the
table-independent checks of its triangles, for tests/test_isosurface_*.py.

Vertices: one per lattice edge whose endpoints differ in interiority (f >= iso, NaN exterior), at
t = (iso - f0) / (f1 - f0) in float64 (0.5 when an endpoint is not finite), coordinate a = origin[a] + h*(i_a + t), the
others origin[b] + h*i_b, rounded to float32 once, in ascending edge key 3*p + a."""
import numpy as np


def vertices(values, dims, origin, spacing, iso):
    """-> (verts (n, 3) float32, keys (n,) int64)"""
    nx, ny, nz = dims
    f = np.asarray(values).reshape(nz, ny, nx).astype(np.float64)   # (float32 -> float64 is exact)
    inside = f >= iso
    keys, coords = [], []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[2 - a], hi[2 - a] = slice(0, -1), slice(1, None)
        cr = inside[tuple(lo)] != inside[tuple(hi)]
        k, j, i = np.nonzero(cr)
        f0, f1 = f[tuple(lo)][cr], f[tuple(hi)][cr]
        with np.errstate(all="ignore"):
            t = (iso - f0) / (f1 - f0)
        t[~(np.isfinite(f0) & np.isfinite(f1))] = 0.5
        ijk = [i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)]
        c = np.empty((len(i), 3))
        for b in range(3):
            c[:, b] = origin[b] + spacing * ((ijk[b] + t) if b == a else ijk[b])
        keys.append(3 * (i.astype(np.int64) + nx * (j.astype(np.int64) + ny * k.astype(np.int64))) + a)
        coords.append(c)
    keys, coords = np.concatenate(keys), np.concatenate(coords)
    o = np.argsort(keys, kind="stable")
    return coords[o].astype(np.float32), keys[o]


def cube_bounds(keys, tris, dims):
    """per triangle and axis, the range [lo, hi] of cube coordinates whose cube holds all three vertices' edges"""
    nx, ny, nz = dims
    k = keys[tris]                                  # (nt, 3)
    a, p = k % 3, k // 3
    pos = np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], -1)   # (nt, 3 vertices, 3 axes)
    axis = np.arange(3)[None, None, :]
    lo = np.where(a[..., None] == axis, pos, pos - 1).max(axis=1)
    hi = pos.min(axis=1)
    return lo, hi


def check_cube_locality(keys, tris, dims):
    """every triangle's three edges lie on one cube, and triangles are sorted by that cube's index"""
    nx, ny, nz = dims
    lo, hi = cube_bounds(keys, tris, dims)
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, np.array([nx - 2, ny - 2, nz - 2]))
    assert (lo <= hi).all(), "a triangle's vertices do not lie on one cube"
    lin = lambda c: c[:, 0] + (nx - 1) * (c[:, 1] + (ny - 1) * c[:, 2])   # noqa: E731
    clo, chi = lin(lo), lin(hi)
    assert (np.maximum.accumulate(clo)[:-1] <= chi[1:]).all(), "triangles are not ordered by cube"


def directed_edges(tris, nv):
    t = tris.astype(np.int64)
    return np.concatenate([t[:, 0] * nv + t[:, 1], t[:, 1] * nv + t[:, 2], t[:, 2] * nv + t[:, 0]])


def unpaired_edges(tris, nv):
    """(directed edges that occur more than once, directed edges whose reverse is missing)"""
    e = directed_edges(tris, nv)
    u, c = np.unique(e, return_counts=True)
    rev = (u % nv) * nv + u // nv
    return u[c > 1], u[~np.isin(rev, u)]


def euler(tris, nv):
    e = directed_edges(tris, nv)
    a, b = e // nv, e % nv
    und = np.unique(np.minimum(a, b) * nv + np.maximum(a, b))
    used = np.unique(tris)
    return len(used) - len(und) + len(tris)


def signed_volume(verts, tris):
    v = verts.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def on_boundary_face(keys, edges, nv, dims):
    """whether each directed edge (u*nv + v) joins two vertices on one face of the lattice's bounding box"""
    nx, ny, nz = dims
    n = np.array(dims)
    out = np.zeros(len(edges), bool)
    pts = []
    for w in (edges // nv, edges % nv):
        k = keys[w]
        p, a = k // 3, k % 3
        pts.append((np.stack([p % nx, (p // nx) % ny, p // (nx * ny)], -1), a))
    (p0, a0), (p1, a1) = pts
    for b in range(3):
        for side in (0, n[b] - 1):
            out |= (a0 != b) & (a1 != b) & (p0[:, b] == side) & (p1[:, b] == side)
    return out


def gyroid(n, period):
    """float32 gyroid sin x cos y + sin y cos z + sin z cos x on an n^3 lattice, `period` points per 2 pi"""
    s = (2 * np.pi / period) * np.arange(n, dtype=np.float64)
    sn, cs = np.sin(s).astype(np.float32), np.cos(s).astype(np.float32)
    f = np.broadcast_to(sn[None, None, :] * cs[None, :, None], (n, n, n)).copy()
    f += sn[None, :, None] * cs[:, None, None]
    f += sn[:, None, None] * cs[None, None, :]
    return f
