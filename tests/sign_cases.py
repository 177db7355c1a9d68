"""Named inputs that put lattice points on the decision boundaries of the sign pass.

Every case is at most 48^3 grid points.  A case carries
  kind        "generic": tests/sign_ref64.py is the comparator on every voxel and no voxel may be undecidable;
              "knife":   the oracle is the comparator bit for bit, the restatement on the decidable voxels only
  cap         the largest share of undecidable voxels it may have (0 for generic cases)
  check       name -> smallest count that its self-check must reach (see self_check)
The literals (`cap`, `check`) were obtained on the CPU from tests/sign_ref64.py alone, by running
`python tests/sign_cases.py`, which prints for every case the undecidable share and the self-check counts; each cap is
the printed share rounded up, each check bound is what the case exists for (the issue's figure), not the printed count.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sign_ref64 as R  # noqa: E402

SCHLAFLI = np.array([[0, 1, 2, 6], [0, 5, 1, 6], [0, 2, 3, 6], [0, 3, 7, 6], [0, 4, 5, 6], [0, 7, 4, 6]])
_FACES = np.array([[0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [3, 0, 4, 7]])


class Case:
    def __init__(self, name, X, IEN, rho_n, rho_t, grid_args, kind, cap=0.0, check=None, extra=None):
        self.name, self.kind, self.cap, self.check = name, kind, cap, dict(check or {})
        self.X = np.ascontiguousarray(X, np.float64)
        self.IEN = np.ascontiguousarray(IEN, np.int64)
        self.rho_n = np.ascontiguousarray(rho_n, np.float64)
        self.rho_t = float(rho_t)
        self.grid_args = grid_args                 # (AABB_min, AABB_max, N_max, margin) of Grid(...)
        self.extra = dict(extra or {})             # what a self-check needs to know about the construction
        self._ref = None

    def grid64(self):
        return R.Grid64(*self.grid_args)

    def ref(self):
        """the restatement's answer, computed once and shared (do not modify)"""
        if self._ref is None:
            self._ref = R.sign_ref(self.X, self.IEN, self.rho_n, self.rho_t, self.grid64())
        return self._ref

    def undecidable(self):
        return ~(self.ref()["margin"] > R.DECIDABLE)


# ---------------------------------------------------------------------------------------
# mesh builders (node numbering x fastest, reference HEX8 node order, 1-based IEN)
# ---------------------------------------------------------------------------------------
def tensor_mesh(ax, ay, az):
    nx, ny, nz = len(ax), len(ay), len(az)
    Z, Y, Xc = np.meshgrid(az, ay, ax, indexing="ij")
    X = np.stack([Xc.ravel(), Y.ravel(), Z.ravel()], axis=1)
    k, j, i = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    base = (k * ny * nx + j * nx + i).ravel()
    off = np.array([0, 1, nx + 1, nx, nx * ny, nx * ny + 1, nx * ny + nx + 1, nx * ny + nx])
    return X, (base[:, None] + off[None, :] + 1).astype(np.int64)


def jitter_interior(X, shape, amount, seed):
    """move the nodes that are not on the outside of an (nz, ny, nx) node block by U(-amount, amount)"""
    nz, ny, nx = shape
    inner = np.zeros(shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    return X + np.random.default_rng(seed).uniform(-amount, amount, X.shape) * inner.ravel()[:, None]


def to_tets(IEN):
    return np.ascontiguousarray(IEN[:, SCHLAFLI].reshape(-1, 4))


def _twist(X, deg_per_z, z0, shear=0.0, taper=0.0):
    """rotate each node about the z axis by deg_per_z * (z - z0); optionally shear x by z*y and shrink with height"""
    a = np.deg2rad(deg_per_z) * (X[:, 2] - z0)
    s = 1.0 - taper * (X[:, 2] - z0)
    x, y = X[:, 0] * s, X[:, 1] * s
    out = np.stack([np.cos(a) * x - np.sin(a) * y, np.sin(a) * x + np.cos(a) * y, X[:, 2]], axis=1)
    if shear:
        out[:, 0] += shear * out[:, 2] * out[:, 1]
        out[:, 2] += 0.5 * shear * out[:, 0] * out[:, 1]           # top and bottom faces leave their planes too
    return out


def _smooth_rho(X, k=(1.3, 0.9, 1.7), ph=0.4):
    return 0.5 + 0.45 * np.sin(k[0] * X[:, 0] + ph) * np.cos(k[1] * X[:, 1] - ph) + 0.3 * np.sin(k[2] * X[:, 2])


def _window(centre, half, npts):
    """grid_args of a cubic grid of `npts` points per axis centred on `centre` (margin 0)"""
    c = np.asarray(centre, np.float64)
    return (c - half, c + half, npts - 1, 0)


# ---------------------------------------------------------------------------------------
# generic cases
# ---------------------------------------------------------------------------------------
def _twisted():
    out = []
    # single hex of edge 2, top face rotated against the bottom face; 44 cells across its box, which is 2.66 to 2.82
    # wide, so 32 lattice points or more along an element edge (grid at most 47^3)
    for deg in (25.0, 40.0):
        X, IEN = tensor_mesh([-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0])
        X = _twist(X, deg / 2.0, -1.0)
        out.append(Case(f"twisted_single_{int(deg)}", X, IEN, _smooth_rho(X), 0.5, (X.min(0), X.max(0), 44, 1), "generic",
                        check=dict(shell=50, nonplanar=20)))
    # the same with shear and taper: all six faces far from planar
    X, IEN = tensor_mesh([-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0])
    X = _twist(X, 16.0, -1.0, shear=0.35, taper=0.15)
    out.append(Case("twisted_single_shear_taper", X, IEN, _smooth_rho(X), 0.5, (X.min(0), X.max(0), 44, 1), "generic",
                    check=dict(shell=50, nonplanar=20)))
    # 2x2x2 block, each element twisted by 30 degrees (and a sheared, tapered twin); the grid is a window of 1.4
    # elements (47 points, 33 across an element) on the middle of one side of the block, so that it holds outer
    # faces, an outer edge-free patch of four elements and the shells between neighbours
    for name, kw in (("twisted_block_30", {}), ("twisted_block_shear_taper", dict(shear=0.3, taper=0.1))):
        ax = np.array([-1.0, 0.0, 1.0])
        X, IEN = tensor_mesh(ax, ax, ax)
        X = _twist(X, 30.0, -1.0, **kw)
        mid = X[(1 * 3 + 1) * 3 + 2]                          # node (i, j, k) = (2, 1, 1): middle of the +x side
        out.append(Case(name, X, IEN, _smooth_rho(X), 0.5, _window(mid, 0.7, 47), "generic",
                        check=dict(shell=50, nonplanar=20)))
    return out


def _box_edges():
    """Block meshes whose element bounds are lattice coordinates: every node is AABB_min + cell * (integer), computed
    as the grid computes it.  The elements are 6 cells wide and the node planes lie at lattice indices
    -9, -3, ..., 33 of a 25-point grid (indices 0..24): two layers stick out on each of the six sides and the outermost
    layer lies wholly outside.  cell = 0.7 / 24 is no power of two, and the far variants sit at (1e3, -2e3, 512.3),
    where (b - AABB_min) / cell rounds: `on_lattice_rounded_off` counts the bounds b == grid_coord(i) for which ceil or
    floor of that quotient is not i (5, 12 and 9 bounds in the three variants)."""
    out = []
    idx = np.arange(-9, 40, 6)                                # 9 node planes, 8 elements per axis, 512 elements
    for name, shift, nz_cells in (("box_edges_origin", (0.0, 0.0, 0.0), 24),
                                  ("box_edges_far", (1e3, -2e3, 512.3), 24),
                                  ("box_edges_thin_z", (1e3, -2e3, 512.3), 1)):
        lo = np.array([0.1, -0.7, 0.3]) + np.array(shift)
        c = 0.7 / 24
        hi = lo + c * np.array([24, 24, nz_cells])
        args = (lo, hi, 24, 0)
        g = R.Grid64(*args)
        zidx = idx if nz_cells > 1 else np.array([-3, 0, 1, 4])          # bounds on both lattice planes of the thin grid
        X, IEN = tensor_mesh(g.coord(0, idx), g.coord(1, idx), g.coord(2, zidx))
        u = (X - g.amin) / (24 * g.cell)
        rho = 0.5 + 0.45 * np.sin(5.0 * u[:, 0] + 0.3) * np.cos(4.0 * u[:, 1]) + 0.2 * np.sin(3.0 * u[:, 2] + 1.0)
        out.append(Case(name, X, IEN, rho, 0.5, args, "generic", check=dict(on_lattice=1, on_lattice_rounded_off=1)))
    # In the blocks above every face on a lattice plane inside the grid is shared, so a point dropped from one box is
    # picked up by the neighbour.  The `outer` blocks end inside the grid: 3^3 elements with node planes at lattice
    # indices 3, 9, 15, 21 (`zero`: 9, 11, 13, 15), every outer node above rho_t (the 8 inner nodes below), so each lattice point on an outer
    # face is +1 through exactly the boxes that end there.  `exact`: the outer planes are grid_coord(3) and
    # grid_coord(21); the point on the plane belongs to the box (`min <= x <= max`).  `inset`: the outer planes are
    # one ulp inside those coordinates; the lattice point is outside every box and stays -1, though (b - AABB_min) / cell
    # rounds to the integer.  `outset`: one ulp outside; the point is inside by an ulp.
    # `zero`: a grid around the origin with the outer planes at indices 9 and 15, close to coordinate 0: there a bound
    # is much smaller than its distance to AABB_min, one ulp of it vanishes in (b - AABB_min) / cell, and ceil / floor
    # of an inset bound give the lattice index of a point that lies outside the box.
    for place, lo0, shift, idx in (("origin", (0.1, -0.7, 0.3), (0.0, 0.0, 0.0), np.array([3, 9, 15, 21])),
                                   ("far", (0.1, -0.7, 0.3), (1e3, -2e3, 512.3), np.array([3, 9, 15, 21])),
                                   ("zero", (-0.35, -0.28, -0.4), (0.0, 0.0, 0.0), np.array([9, 11, 13, 15]))):
        lo = np.array(lo0) + np.array(shift)
        n_face = int((idx[-1] - idx[0] + 1) ** 3 - (idx[-1] - idx[0] - 1) ** 3)      # 1946 (19^3 - 17^3) or 218
        args = (lo, lo + (0.7 / 24) * 24, 24, 0)
        g = R.Grid64(*args)
        for kind, step in (("exact", 0.0), ("inset", 1.0), ("outset", -1.0)):
            axes = []
            for a in range(3):
                v = g.coord(a, idx)
                if step:
                    v[0], v[-1] = np.nextafter(v[0], step * np.inf), np.nextafter(v[-1], -step * np.inf)
                axes.append(v)
            X, IEN = tensor_mesh(*axes)
            inner = np.zeros((4, 4, 4), bool)
            inner[1:3, 1:3, 1:3] = True
            u = (X - g.amin) / (24 * g.cell)
            rho = np.where(inner.ravel(), 0.2, 0.7 + 0.2 * np.sin(5.0 * u[:, 0] + 0.3) * np.cos(4.0 * u[:, 1] + 3.0 * u[:, 2]))
            out.append(Case(f"box_edges_outer_{place}_{kind}", X, IEN, rho, 0.5, args, "generic",
                            check={"outer_face_points": n_face, ("outer_face_negative" if kind == "inset" else "outer_face_positive"): n_face},
                            extra=dict(lo=int(idx[0]), hi=int(idx[-1]))))
    return out


def _long_lists():
    out = []
    # (a) 10^3 jittered elements of 0.4 cell (10 per 4-cell tile edge) centred on the second tile of a 12^3 grid, the
    # block rotated out of the axes so that the elements' boxes overlap: about a quarter of the boxes hold a lattice
    # point, and the tile's list is longer than 64
    ax = 0.4 * (np.arange(11) - 5.0)
    X, IEN = tensor_mesh(ax, ax, ax)
    X = jitter_interior(X, (11, 11, 11), 0.06, 7)
    a, b = np.deg2rad(35.0), np.deg2rad(25.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    X = X @ (Rx @ Rz).T + 1.53
    rho =0.5 + 0.4 * np.sin(1.1 * X[:, 0]) * np.cos(0.9 * X[:, 1]) + 0.3 * np.sin(1.3 * X[:, 2] + 0.5)
    out.append(Case("long_lists_fine", X, IEN, rho, 0.5, (np.full(3, -4.0), np.full(3, 7.0), 11, 0), "generic",
                    check=dict(longest_list=65)))
    # (b) tensor mesh with spacings large, small, large, small, large (6.3 and 0.8 cells) on each axis: 125 elements of
    # mixed size inside one tile's list - 8 whose box holds one point (small^3), 36 of 6 or 7 points, 54 of 36 to 49
    # and 27 of more than 200 (large^3).  In element order (x fastest) large and small alternate: 1-point elements
    # stand between 6-7-point ones, 216-point elements between 36-49-point ones.  The two leftmost element columns
    # (50 elements, 40 %) lie wholly below rho_t
    w = np.array([6.3, 0.8, 6.3, 0.8, 6.3])
    ax = 1.35 + np.concatenate([[0.0], np.cumsum(w)])
    X, IEN = tensor_mesh(ax, ax, ax)
    rho = 0.5 + 0.4 * np.sin(0.45 * X[:, 1] + 0.2) * np.cos(0.4 * X[:, 2]) + 0.02 * X[:, 0]
    rho = np.where(X[:, 0] < ax[2] + 1e-9, np.minimum(rho, 0.5) - 0.2, rho)
    out.append(Case("long_lists_alternating", X, IEN, rho, 0.5, (np.zeros(3), np.full(3, 23.0), 23, 0), "generic",
                    check=dict(small_boxes=1, large_boxes=1, below=1)))
    return out


# ---------------------------------------------------------------------------------------
# knife-edge cases
# ---------------------------------------------------------------------------------------
def _aligned():
    """4x4x4 block on [-1, 1]^3, lattice of 8 cells per element (cell 1/16): every coordinate is exact in binary and
    lattice points sit on nodes, edges and faces.  Nodal densities alternate 0 / 1; rho_t = 0.45 is crossed inside every
    element and is no dyadic rational, so no lattice point has rho == rho_t."""
    ax = np.linspace(-1.0, 1.0, 5)
    X, IEN = tensor_mesh(ax, ax, ax)
    ijk = np.rint((X + 1.0) * 2.0).astype(np.int64)
    rho = (ijk.sum(axis=1) % 2).astype(np.float64)
    args = (X.min(0), X.max(0), 32, 3)
    return [Case("aligned_hex8", X, IEN, rho, 0.45, args, "knife", cap=0.0, check=dict(ties=100)),
            # on a tet face one barycentric coordinate is 0 and `lambda >= 0` hangs on its rounding: those voxels
            # are undecidable by construction unless every tetrahedron around them is clearly below rho_t
            Case("aligned_tet4", X, to_tets(IEN), rho, 0.45, args, "knife", cap=CAPS["aligned_tet4"], check=dict(on_face=100))]


def _threshold_ties():
    out = []
    ax = np.linspace(-1.0, 1.0, 4)
    X, IEN = tensor_mesh(ax, ax, ax)
    X = jitter_interior(X, (4, 4, 4), 0.1, 11)
    args = (X.min(0), X.max(0), 12, 2)                       # 17^3 points
    for rt in (0.5, 1e-3, 5.0):
        vals = [("eq", rt), ("up1", np.nextafter(rt, np.inf)), ("dn1", np.nextafter(rt, -np.inf)),
                ("p05", rt * (1 + 0.5e-9)), ("m05", rt * (1 - 0.5e-9)), ("p2", rt * (1 + 2e-9)), ("m2", rt * (1 - 2e-9))]
        for tag, v in vals:
            name = f"threshold_hex8_rt{rt:g}_{tag}"
            out.append(Case(name, X, IEN, np.full(len(X), v), rt, args, "knife", cap=CAPS[name]))
        for tag, f in (("m05", 0.5), ("m2", 2.0)):
            v = rt - f * 1e-12 * (abs(rt) + 1.0)
            name = f"threshold_tet4_rt{rt:g}_{tag}"
            out.append(Case(name, X, to_tets(IEN), np.full(len(X), v), rt, args, "knife", cap=CAPS[name]))
    return out


def _margin_mixed():
    """6x6x6 jittered block.  Element columns i = 0, 1 have every node at or above rho_t + d with the minimum exactly
    there (the shortcut's side), columns i = 4, 5 every node at or below rho_t - d, columns 2, 3 cross rho_t; shortcut
    and Newton elements share faces."""
    out = []
    ax = np.linspace(-1.0, 1.0, 7)
    for tag, d in (("05", 0.5e-9), ("2", 2e-9)):
        X, IEN = tensor_mesh(ax, ax, ax)
        X = jitter_interior(X, (7, 7, 7), 0.04, 13)
        rng = np.random.default_rng(17)
        i = np.tile(np.arange(7), 49)
        u = rng.uniform(0.0, 1.0, len(X))
        pick = rng.uniform(0.0, 1.0, len(X)) < 0.5
        rho = np.where(i <= 2, np.where(pick, 0.5 + d, 0.5 + d + 0.4 * u),
                       np.where(i >= 4, np.where(pick, 0.5 - d, 0.5 - d - 0.4 * u), 0.1 + 0.8 * u))
        out.append(Case(f"margin_mixed_{tag}", X, IEN, rho, 0.5, (X.min(0), X.max(0), 33, 3), "knife",
                        cap=CAPS["margin_mixed_" + tag], check=dict(above=1, below=1, crossing=1)))
    return out


# Largest undecidable share of each knife-edge case, one literal per case.  Obtained on the CPU from tests/sign_ref64.py
# alone (`python tests/sign_cases.py` prints the shares); each literal is the printed share of that case, rounded up.
_INTERIOR = 0.448                # printed 0.447181 = 13^3 / 17^3: every lattice point inside the 3x3x3 block
CAPS = {
    "aligned_tet4": 0.215,       # printed 0.214535: the lattice points on tet faces with a tetrahedron at or above rho_t
    "threshold_hex8_rt0.5_eq": _INTERIOR, "threshold_hex8_rt0.5_up1": _INTERIOR, "threshold_hex8_rt0.5_dn1": _INTERIOR,
    "threshold_hex8_rt0.5_p05": _INTERIOR, "threshold_hex8_rt0.5_m05": _INTERIOR, "threshold_hex8_rt0.5_p2": _INTERIOR,
    # rho_t - v = 1e-9 here and max(1, |rho_t|) = 1: the margin of an interior voxel is 1e-9 up to the round-off of
    # sum(N_k) v, and which side of DECIDABLE it falls on differs from voxel to voxel (printed 0.154692; another
    # summation order moves single voxels, which the second digit leaves room for)
    "threshold_hex8_rt0.5_m2": 0.16,
    "threshold_tet4_rt0.5_m05": _INTERIOR, "threshold_tet4_rt0.5_m2": _INTERIOR,
    "threshold_hex8_rt0.001_eq": _INTERIOR, "threshold_hex8_rt0.001_up1": _INTERIOR, "threshold_hex8_rt0.001_dn1": _INTERIOR,
    "threshold_hex8_rt0.001_p05": _INTERIOR, "threshold_hex8_rt0.001_m05": _INTERIOR, "threshold_hex8_rt0.001_p2": _INTERIOR,
    "threshold_hex8_rt0.001_m2": _INTERIOR,
    "threshold_tet4_rt0.001_m05": _INTERIOR, "threshold_tet4_rt0.001_m2": _INTERIOR,
    "threshold_hex8_rt5_eq": _INTERIOR, "threshold_hex8_rt5_up1": _INTERIOR, "threshold_hex8_rt5_dn1": _INTERIOR,
    "threshold_hex8_rt5_p05": _INTERIOR, "threshold_hex8_rt5_m05": _INTERIOR,
    "threshold_hex8_rt5_p2": 0.0,     # printed 0: |v - rho_t| / max(1, |rho_t|) = 2e-9
    "threshold_hex8_rt5_m2": 0.0,     # printed 0
    "threshold_tet4_rt5_m05": _INTERIOR, "threshold_tet4_rt5_m2": _INTERIOR,
    "margin_mixed_05": 0.0083,   # printed 0.008219: points where rho is within 1e-9 of rho_t, around the nodes at rho_t +- 0.5e-9
    "margin_mixed_2": 0.0,       # printed 0
}


def all_cases():
    return _twisted() + _box_edges() + _long_lists() + _aligned() + _threshold_ties() + _margin_mixed()


_CACHE = {}


def cases():
    """name -> Case, built once per process"""
    if not _CACHE:
        for c in all_cases():
            _CACHE[c.name] = c
    return _CACHE


def case_names():
    return list(cases().keys())


# ---------------------------------------------------------------------------------------
# self-checks: does the case reach what it exists for?  -> dict of counts, compared with case.check
# ---------------------------------------------------------------------------------------
def tile_list_lengths(case):
    """for every 4x4x4-voxel tile: the number of elements whose box holds a lattice point of the tile"""
    g = case.grid64()
    ref = case.ref()
    nx, ny, nz = g.dims
    v = ref["pair_vox"]
    i, j, k = v % nx, (v // nx) % ny, v // (nx * ny)
    tx, ty = (nx + 3) // 4, (ny + 3) // 4
    tile = ((k // 4) * ty + j // 4) * tx + i // 4
    pairs = np.unique(np.stack([tile, ref["pair_el"]], axis=1), axis=0)
    return np.bincount(pairs[:, 0])


def self_check(case):
    ref, g = case.ref(), case.grid64()
    out = {}
    want = case.check
    I0 = case.IEN - 1
    if "shell" in want:
        out["shell"] = int(((ref["winner_mx"] > 1.0) & (ref["winner_mx"] < 1.01)).sum())
    if "nonplanar" in want:
        # voxels inside the 1.01 box of an element that lie outside the plane through three nodes of one of its faces
        pts = g.points()
        sel = ref["pair_mx"] < 1.01
        pv, pe = ref["pair_vox"][sel], ref["pair_el"][sel]
        Xe = case.X[I0[pe]]
        lost = np.zeros(len(pv), bool)
        for f in _FACES:
            a, b, c = Xe[:, f[0]], Xe[:, f[1]], Xe[:, f[2]]
            nrm = np.cross(b - a, c - a)
            nrm *= np.sign(np.einsum("nd,nd->n", nrm, a - Xe.mean(axis=1)))[:, None]     # outward
            lost |= np.einsum("nd,nd->n", nrm, pts[pv] - a) > 0
        out["nonplanar"] = int(len(np.unique(pv[lost])))
    if "on_lattice" in want:
        # bounds b == grid_coord(i) for which ceil / floor of (b - amin) / cell is not i
        n_on = n_off = 0
        for a in range(3):
            lat = g.coord(a, np.arange(g.dims[a]))
            for b in np.unique(case.X[:, a]):
                hit = np.nonzero(lat == b)[0]
                if len(hit):
                    n_on += 1
                    q = (b - g.amin[a]) / g.cell
                    n_off += int(np.ceil(q) != hit[0] or np.floor(q) != hit[0])
        out["on_lattice"] = n_on
        out["on_lattice_rounded_off"] = n_off
    if "outer_face_points" in want:
        # lattice points on the six lattice planes that bound the block, within the block's extent
        lo_i, hi_i = case.extra["lo"], case.extra["hi"]
        nx, ny, nz = g.dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
        on = np.all((ijk >= lo_i) & (ijk <= hi_i), axis=1) & np.any((ijk == lo_i) | (ijk == hi_i), axis=1)
        out["outer_face_points"] = int(on.sum())
        out["outer_face_positive"] = int((ref["sign"][on] > 0).sum())
        out["outer_face_negative"] = int((ref["sign"][on] < 0).sum())
    if "longest_list" in want:
        out["longest_list"] = int(tile_list_lengths(case).max())
    if "small_boxes" in want:
        per_el = np.bincount(ref["pair_el"], minlength=len(case.IEN))
        out["small_boxes"] = int(((per_el >= 1) & (per_el <= 3)).sum())
        out["large_boxes"] = int((per_el > 200).sum())
        out["below"] = int((case.rho_n[I0].max(axis=1) < case.rho_t).sum())
    if "ties" in want:
        # voxels with two or more candidates at the same max|xi| <= 1: points on shared faces, edges and nodes
        sel = ref["pair_mx"] <= 1.0
        key = np.stack([ref["pair_vox"][sel].astype(np.float64), ref["pair_mx"][sel]], axis=1)
        _, cnt = np.unique(key, axis=0, return_counts=True)
        out["ties"] = int((cnt > 1).sum())
    if "on_face" in want:
        on = np.any(ref["pair_lam"] == 0.0, axis=1) & (ref["pair_lam"].min(axis=1) >= 0)
        out["on_face"] = int(len(np.unique(ref["pair_vox"][on])))
    if "above" in want:
        r = case.rho_n[I0]
        out["above"] = int((r.min(axis=1) > case.rho_t).sum())
        out["below"] = int((r.max(axis=1) < case.rho_t).sum())
        out["crossing"] = int(((r.min(axis=1) < case.rho_t) & (r.max(axis=1) > case.rho_t)).sum())
    return out


if __name__ == "__main__":
    import time
    for name, c in cases().items():
        t = time.time()
        und = c.undecidable()
        print(f"{name:36s} {c.kind:8s} ngp {c.grid64().ngp:7d} nel {len(c.IEN):5d} undecidable {int(und.sum()):6d} "
              f"share {und.mean():.6f} +1: {int((c.ref()['sign'] > 0).sum()):6d} checks {self_check(c)} {time.time() - t:.1f}s")
