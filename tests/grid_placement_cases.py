"""The mesh, the windows and the transforms of the grid-placement tests (CPU and GPU files share them; no GPU here).

One mesh, synthetic.hex_mesh(6, jitter=0.3, seed=7) with every coordinate rounded to a multiple of 2^-20 (dyadic shifts and
power-of-two scalings are then exact), as HEX8 and split into TET4; nodal densities clip(N(0.5, 0.35), 0, 1), rho_t = 0.5,
band factor 1.1.

The FULL grid is Grid([-1]*3, [1]*3, 32, 3): 39^3 points, cell exactly 1/16.  A WINDOW is an offset and an extent in cells
of that lattice: grid_make(amin_full + off * cell, that + ext * cell, max(ext), 0).  Every number involved is a small
multiple of 2^-4, so every lattice point of a window is the same double as the point off + (i, j, k) of the full lattice,
and a result on the window can be compared bit for bit with a crop of the result on the full grid.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

RHO_T = 0.5
BAND_FACTOR = 1.1
CELL = 1.0 / 16.0
FULL_BOX = (np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0]))
FULL_N_MAX, FULL_MARGIN = 32, 3
FULL_DIMS = (39, 39, 39)
AMIN_FULL = np.array([-1.0 - 3 * CELL] * 3)

# name -> (offset, extent) in cells of the full lattice
WINDOWS = {
    "interior": ((11, 7, 19), (16, 12, 9)),            # inside the mesh: every voxel is a band voxel
    "corner-out": ((-5, -4, 30), (16, 16, 16)),        # hangs over one corner of the full grid
    "outside": ((60, 3, 3), (8, 8, 8)),                # misses the mesh: all sentinel
    "superset": ((-9, -2, -13), (64, 50, 60)),         # the full grid lies inside it
    "thin": ((9, 10, 17), (16, 16, 1)),                # two planes
    "far": ((2 ** 34, 5, 5), (8, 8, 8)),               # 2^30 length units away: lattice indices of the mesh beyond int32
    "farneg": ((-2 ** 34, 5, 5), (8, 8, 8)),
}
for _r in range(4):   # the tile origin at different residues mod 4 on every axis
    WINDOWS[f"align{_r}"] = ((8 + _r, 8 + (2 * _r + 1) % 4, 8 + (3 * _r + 2) % 4), (13, 14, 15))
EMPTY_WINDOWS = ("outside", "far", "farneg")

# name -> (scale per axis, shift); the grid is rebuilt as Grid(lo, hi, 32, 3) on the transformed [-1, 1]^3 box
TRANSFORMS = {
    "scale2^-10": (2.0 ** -10, 0.0),
    "scale2^10": (2.0 ** 10, 0.0),
    "scale1e-3": (1e-3, 0.0),
    "scale1e3": (1e3, 0.0),
    "shift64": (1.0, 64.0),
    "shift4096": (1.0, 4096.0),
    "shift2^20": (1.0, 2.0 ** 20),
    "aniso": (np.array([1.0, 0.25, 3.0]), 0.0),
}
EXACT_SCALES = ("scale2^-10", "scale2^10")   # HEX8: the oracle is exactly equivariant under these


def _syn():
    graft.load_package()
    from rho2sdf_jl_amd import synthetic
    return synthetic


_MESH = {}


def mesh(kind):
    """kind 'hex8' / 'tet4' -> (X, IEN, rho_n); built once, returned read-only"""
    if not _MESH:
        syn = _syn()
        X, IH, _ = syn.hex_mesh(6, jitter=0.3, seed=7)
        X = np.ascontiguousarray(np.round(X * 2.0 ** 20) / 2.0 ** 20)
        rn = np.clip(np.random.default_rng(1).normal(0.5, 0.35, len(X)), 0.0, 1.0)
        IT = syn.hex_to_tets(IH)
        for a in (X, IH, IT, rn):
            a.setflags(write=False)
        _MESH["hex8"] = (X, IH, rn)
        _MESH["tet4"] = (X, IT, rn)
    return _MESH[kind]


def full_grid(make):
    """`make` is oracle.grid_make or pkg.Grid (same arguments)"""
    return make(FULL_BOX[0], FULL_BOX[1], FULL_N_MAX, FULL_MARGIN)


def _grid_fields(g):
    """(N, cell) of an oracle grid or a package grid"""
    if hasattr(g, "c"):
        return tuple(int(n) for n in g.c.N), float(g.c.cell_size)
    return tuple(int(n) for n in g.N), float(g.cell)


def window_grid_at(make, off, ext):
    """the grid of the window (offset, extent), with the guarantees the bit-exact crops rest on"""
    lo = AMIN_FULL + np.array(off, dtype=np.float64) * CELL
    hi = lo + np.array(ext, dtype=np.float64) * CELL
    g = make(lo, hi, max(ext), 0)
    N, cell = _grid_fields(g)
    assert cell == CELL and N == tuple(ext), (off, ext, cell, N)
    return g


def window_grid(make, name):
    return window_grid_at(make, *WINDOWS[name])


def overlap(name):
    """the part of window `name` that lies on the full lattice: (slices into the window's (nz, ny, nx) array, slices into
    the full grid's), or None when they share no point"""
    off, ext = WINDOWS[name]
    win, full = [], []
    for ax in range(3):
        a, b = max(off[ax], 0), min(off[ax] + ext[ax], FULL_DIMS[ax] - 1)      # full-lattice indices, inclusive
        if a > b:
            return None
        win.append(slice(a - off[ax], b - off[ax] + 1))
        full.append(slice(a, b + 1))
    return tuple(win[::-1]), tuple(full[::-1])                                  # arrays are (z, y, x)


def dims3(name):
    """(nz, ny, nx) of window `name`"""
    return tuple(e + 1 for e in WINDOWS[name][1][::-1])


def transformed(kind, tname):
    """-> (X', IEN, rho_n, lo', hi'): the mesh and the [-1, 1]^3 box under transform `tname`"""
    X, IEN, rn = mesh(kind)
    sc, sh = TRANSFORMS[tname]
    return np.ascontiguousarray(X * sc + sh), IEN, rn, FULL_BOX[0] * sc + sh, FULL_BOX[1] * sc + sh


def bits(a):
    """the bit patterns of a float64 array (0.0 and -0.0 differ, NaN equals itself)"""
    return np.ascontiguousarray(a).view(np.uint64)
