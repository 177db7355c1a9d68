"""The SDF volume on the GPU against the float64 restatement of CalcVolumeFromSDF.jl (vol_ref64), standalone
(r2s_volume_from_sdf) and inside the level bisection of RBFs_smoothing (segment extrema, narrowed row lists).

The kernels take every point decision as the restatement does, so the only difference is the order of a sum of
non-negative Float32 terms: |V_gpu - V_ref| <= vol_ref64's bound, and exactly 0 where every term is a multiple of a power
of two that no partial sum can round.  The bounded tests print the largest fraction of the bound they observed, the
bisection how many of its replays were decided at every level."""
import numpy as np
import pytest

import rbf_ref64
import vol_ref64 as ref

pytestmark = pytest.mark.gpu


def _check(pkg, v, edge, iso=0.0, order=9):
    V, b = ref.volume(v, edge, iso=iso, order=order)
    got = pkg.calculate_volume_from_sdf(v, edge, iso_threshold=iso, detailed_quad_order=order)
    assert abs(got - V) <= b, (v.shape, edge, iso, order, got, V, b)
    return abs(got - V) / b if b > 0 else 0.0


def _waves(dims, seed, amp=1.0, offset=0.0):
    """Float32 (nz, ny, nx): waves of a few cells along every axis, so that cut cells lie in every segment and row"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.2, 0.9, 3)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij", sparse=True)
    f = np.sin(a[0] * x + 0.3) + np.cos(a[1] * y - 0.5 * z) * np.sin(a[2] * z + 0.1 * y) - 0.2
    return (amp * f + offset).astype(np.float32)


# ---- shapes ----------------------------------------------------------------------------------------------------------

SHAPES = [(70, 23, 41), (23, 41, 70), (41, 70, 23),          # one anisotropic field in its three orientations
          (2, 17, 9), (64, 9, 5), (65, 3, 7), (66, 7, 3), (129, 5, 4), (130, 4, 5),   # nx - 1 = 1, 63, 64, 65, 128, 129
          (37, 2, 11), (29, 13, 2), (40, 2, 2),                                      # ny = 2, nz = 2
          (4097, 3, 3), (4098, 3, 3), (4162, 3, 3),                                  # > 64 segments per row
          (3, 259, 256), (3, 300, 300)]                                              # rows past the first grid-stride pass


def test_volume_shapes(pkg):
    worst = 0.0
    base = _waves((70, 23, 41), 1)
    for dims in SHAPES:
        if dims == (23, 41, 70):
            v = np.ascontiguousarray(base.transpose(2, 0, 1))       # x, y, z of the base field along z, x, y
        elif dims == (41, 70, 23):
            v = np.ascontiguousarray(base.transpose(1, 2, 0))       # ... along y, z, x
        else:
            v = _waves(dims, sum(dims))
        assert v.shape == dims[::-1]
        for order in (9, 2):
            worst = max(worst, _check(pkg, v, 0.03125, order=order))
    print(f"shapes: largest fraction of the bound {worst:.3g}")


# ---- exact cases: marked cells in chosen places ------------------------------------------------------------------------

def _marked(dims, cells, iso, blocks=(), corner=None):
    """background iso - 4; the 8 corners of every marked cell (i, j, k) and of every block of cells ((i0, i1), (j0, j1),
    (k0, k1)) set to `corner` (default iso): the marked cells are full (their minimum is iso), their neighbours are
    cut cells whose Gauss points all lie below iso"""
    nx, ny, nz = dims
    v = np.full((nz, ny, nx), np.float32(iso) - np.float32(4), dtype=np.float32)
    c = np.float32(iso) if corner is None else corner
    for i, j, k in cells:
        v[k:k + 2, j:j + 2, i:i + 2] = c
    for (i0, i1), (j0, j1), (k0, k1) in blocks:
        v[k0:k1 + 1, j0:j1 + 1, i0:i1 + 1] = c
    return v


def _row(dims, row):
    return row % (dims[1] - 1), row // (dims[1] - 1)


EXACT = [
    # the first, a middle, the last cell of a row; the 65th segment; the partial last segment (one cell)
    ((4162, 3, 3), [(0, 0, 0), (2000, 1, 0), (4160, 0, 1), (4096, 1, 1), (4159, 1, 1)]),
    ((4098, 3, 3), [(4096, 0, 0), (4032, 1, 1), (4031, 0, 1)]),
    # rows 0, 65 535, 65 536 and the last of 89 401: the second grid-stride pass
    ((3, 300, 300), [(0,) + _row((3, 300, 300), r) for r in (0, 65535, 65536, 70000)] + [(1, 298, 298)]),
    # ny != nz, a partial last segment of one cell, rows past 65 536
    ((130, 260, 300), [(128, 258, 298), (0, 258, 298), (64, 0, 252), (127, 100, 260), (128, 0, 0)]),
    ((130, 300, 260), [(128, 298, 258), (0, 298, 258), (64, 0, 220), (127, 259, 1)]),
]


@pytest.mark.parametrize("dims,cells", EXACT)
def test_volume_marked_cells_exact(pkg, dims, cells):
    """V = (number of marked cells) edge^3 exactly, at every quadrature form: the marked cells are full (minimum ==
    iso), the cut cells around them add nothing; edge a power of two and far fewer than 2^24 cells, so no partial sum
    rounds.  Also with -0.0 corners at iso 0"""
    for iso, corner in ((0.25, None), (0.0, np.float32(-0.0)), (-3.5, None)):
        v = _marked(dims, cells, iso, corner=corner)
        for order, edge in ((9, 0.0625), (17, 4.0), (1, 2.0 ** -10)):
            V, _ = ref.volume(v, edge, iso=iso, order=order)
            assert V == len(cells) * edge ** 3, (V, len(cells))
            got = pkg.calculate_volume_from_sdf(v, edge, iso_threshold=iso, detailed_quad_order=order)
            assert got == V, (dims, iso, order, got, V)


def test_volume_513_cubed_exact(pkg):
    """the coarse lattice the bisection sees at bench size: one full block of 200^3 cells (< 2^24), marked cells in the
    last rows (the fourth grid-stride pass), the rest empty"""
    dims = (513, 513, 513)
    cells = [(511, 511, 511), (0, 511, 511), (300, 510, 511), (448, 255, 400), (511, 0, 300)]
    v = _marked(dims, cells, 0.5, blocks=[((20, 220), (100, 300), (30, 230))])
    edge = 2.0 ** -9
    V = (len(cells) + 200 ** 3) * edge ** 3
    assert ref.volume(v, edge, iso=0.5, order=2)[0] == V   # (the restatement once: the cut cells add nothing at any order)
    for order in (2, 9):
        got = pkg.calculate_volume_from_sdf(v, edge, iso_threshold=0.5, detailed_quad_order=order)
        assert got == V, (order, got, V, (got - V) / edge ** 3)


@pytest.mark.parametrize("dims,cells", EXACT)
def test_volume_sparse_cut_cells(pkg, dims, cells):
    """the same places with cut cells instead of full ones: a tiny V, so the bound is a small fraction of one cell and
    a lost, doubled or misplaced cell fails"""
    rng = np.random.default_rng(len(cells))
    v = _marked(dims, cells, 0.0, corner=np.float32(0.0))
    for i, j, k in cells:   # the corners of each marked cell: random, on both sides of iso
        v[k:k + 2, j:j + 2, i:i + 2] = rng.uniform(-1.0, 1.0, (2, 2, 2)).astype(np.float32)
        v[k, j, i] = np.float32(0.75)
    worst = 0.0
    for order in (9, 20):
        V, b = ref.volume(v, 0.125, order=order)
        assert V > 0 and b < 1e-3 * 0.125 ** 3
        worst = max(worst, _check(pkg, v, 0.125, order=order))
    print(f"sparse cut cells {dims}: largest fraction of the bound {worst:.3g}")


# ---- quadrature forms and values -----------------------------------------------------------------------------------

def test_volume_quadrature_orders(pkg):
    """the tensor form (order <= 9) and the point-per-lane form (order >= 10) against the restatement; order 0 and 33
    are argument errors"""
    v = _waves((40, 9, 13), 3)
    worst = 0.0
    for order in (1, 2, 3, 8, 9, 10, 16, 17, 20, 32):
        worst = max(worst, _check(pkg, v, 0.0625, iso=0.1, order=order))
    for order in (0, 33):
        with pytest.raises(pkg._lib.R2SError, match="error -1"):
            pkg.calculate_volume_from_sdf(v, 0.0625, detailed_quad_order=order)
    print(f"orders: largest fraction of the bound {worst:.3g}")


def test_volume_values(pkg):
    """iso != 0, all-negative and mixed-sign fields, -0.0 values, edges of 1e-3 and 1e3"""
    worst = 0.0
    dims = (70, 23, 41)
    mixed = _waves(dims, 7)
    neg = _waves(dims, 8, amp=0.5, offset=-3.0)
    zeros = mixed.copy()
    zeros[np.abs(zeros) < 0.15] = np.float32(-0.0)
    zeros[::3, ::2] = np.where(zeros[::3, ::2] == 0, np.float32(0.0), zeros[::3, ::2])
    for v, iso in ((mixed, 0.0), (mixed, 0.37), (mixed, -0.61), (neg, -3.2), (neg, -2.5), (zeros, 0.0)):
        for edge in (1e-3, 1.0, 1e3):
            worst = max(worst, _check(pkg, v, edge, iso=iso))
    print(f"values: largest fraction of the bound {worst:.3g}")


# ---- the level bisection of RBFs_smoothing -----------------------------------------------------------------------------

BISECT = [((150, 40, 33), 2.0 ** -6, (0.1, 0.37, 0.5, 0.8)),
          ((20, 300, 260), 2.0 ** -7, (0.1, 0.5, 0.8))]
MIN_UNAMBIGUOUS = 11   # of 14 (7 targets x 2 smooth values)


def _layers(g, seed):
    """a coarse SDF whose level sets are wavy sheets across z: the cut cells of every level lie in a band of rows, the
    other rows are settled by the narrowing"""
    nx, ny, nz = g.dims
    h = g.cell_size
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij", sparse=True)
    f = (0.6 * nz - z) + 2.5 * np.sin(0.21 * x + 0.4) * np.cos(0.13 * y) + 0.3 * rng.normal(size=(nz, ny, nx))
    return (h * f).astype(np.float64).ravel()


def test_level_bisection_replay(pkg):
    """RBFs_smoothing's level shift against a replay of its bisection on the LSF it returns: wherever every branch and
    the stop check are decided beyond the bound, th is the replay's bit for bit; elsewhere th lies in the bracket of the
    first undecided level.  :same and a refined smooth; rows with several segments and more than 65 536 rows"""
    decided, total = 0, 0
    for dims, h, fractions in BISECT:
        lo = np.array([0.375, -0.25, 0.125])
        g = pkg.Grid(lo, lo + h * (np.array(dims) - 1.0), max(dims) - 1, 0)
        assert g.dims == dims and g.cell_size == h
        cx = rbf_ref64.coarse_axes(g.AABB_min, g.AABB_max, g.N)[0]
        edge = ref.coarse_edge(cx)
        assert edge == np.float32(h)
        sdf = _layers(g, sum(dims))
        domain = float(np.prod(np.array(dims) - 1)) * h ** 3
        replays = {}
        for smooth in (1, 2):
            for frac in fractions:
                target = frac * domain
                info = {}
                pkg.RBFs_smoothing(sdf, g, False, smooth, target, info=info)
                lsf = info["lsf"]
                key = (lsf.tobytes(), target)
                if key not in replays:
                    replays[key] = ref.bisect(lsf, edge, target)
                th, steps = replays[key]
                got = np.float32(info["th"])
                s = ref.first_ambiguous(steps)
                total += 1
                if s is None:
                    decided += 1
                    assert got == th, (dims, smooth, frac, got, th, len(steps))
                else:
                    st = steps[s]
                    assert st["lo"] <= -got <= st["hi"], (dims, smooth, frac, got, st)
                    print(f"bisection {dims}/{smooth} target {frac}: level {s} of {len(steps)} undecided "
                          f"(|V - target| {abs(st['V'] - target):.3g}, bound {st['bound']:.3g})")
    pkg._lib.lib().r2s_release_cache()
    print(f"bisection: {decided} of {total} replays decided at every level")
    assert decided >= MIN_UNAMBIGUOUS, (decided, total)
