"""CPU checks around the SDF volume: the product's Gauss-Legendre table, the float64 restatement (vol_ref64) against the
oracle's serial Float32 sum, and the argument errors r2s_volume_from_sdf returns before it touches a device."""
import ctypes

import numpy as np
import pytest

import vol_ref64 as ref

R2S_ERR_ARG = -1


def test_product_gauss_tables_match_leggauss(pkg):
    """r2s_internal_gauss_legendre (the table every volume kernel rounds to Float32) against numpy's leggauss, for every
    order the volume accepts: within a few ulp in Float64 and the same numbers after rounding to Float32"""
    f = ctypes.CDLL(pkg._lib.LIB_PATH).r2s_internal_gauss_legendre
    f.restype = None
    for n in range(1, 33):
        x, w = np.full(n, np.nan), np.full(n, np.nan)
        f(ctypes.c_int(n), x.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p))
        xr, wr = np.polynomial.legendre.leggauss(n)
        assert np.abs(x - xr).max() <= 2.5e-16 and np.abs(w - wr).max() <= 4e-15, n
        assert np.array_equal(x.astype(np.float32), xr.astype(np.float32)), n
        assert np.array_equal(w.astype(np.float32), wr.astype(np.float32)), n


def _field(dims, seed, scale=0.05, offset=0.0):
    """a bumpy ball with noise: full, outside and cut cells on a small lattice"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r = np.sqrt((x - 0.45 * nx) ** 2 + (y - 0.4 * ny) ** 2 + (z - 0.55 * nz) ** 2)
    return ((0.3 * max(dims) - r + 0.3 * rng.normal(size=r.shape)) * scale + offset).astype(np.float32)


@pytest.mark.parametrize("dims", [(17, 9, 13), (30, 12, 7), (5, 40, 6), (2, 11, 9)])
@pytest.mark.parametrize("order", [1, 2, 3, 9, 10, 17, 32])
def test_reference_matches_oracle(oracle, dims, order):
    """the restatement against the oracle's serial Float32 sum (CalcVolumeFromSDF.jl's loop order) on fields with cut
    cells; iso != 0, an all-negative field, -0.0 corners and two edge scales included.  The oracle's own error is at
    most (cells + points per cell) Float32 additions deep"""
    nx, ny, nz = dims
    nterms = (nx - 1) * (ny - 1) * (nz - 1) + order ** 3
    worst = 0.0
    f = _field(dims, sum(dims) + order)
    neg = _field(dims, order, offset=-2.0)
    zer = f.copy()
    zer[::2] = np.where(zer[::2] > 0, np.float32(-0.0), zer[::2])
    for v, edge, iso in ((f, 0.0625, 0.0), (f, 0.0625, 0.013), (f, 1e-3, -0.02), (neg, 1e3, -2.1), (zer, 0.5, 0.0)):
        V, b = ref.volume(v, edge, iso=iso, order=order)
        ov = oracle.volume_from_sdf(v, edge, iso=iso, order=order)
        sb = ref.serial_bound(nterms, V) + b
        assert V > 0 and abs(ov - V) <= sb, (edge, iso, V, ov, sb)
        worst = max(worst, abs(ov - V) / sb)
    print(f"{dims} order {order}: largest fraction of the oracle's bound {worst:.3g}")


def test_reference_counts_every_cell_once():
    """no cut cell: a field of one value is all full or all outside, with the iso value itself counting as inside"""
    v = np.full((5, 4, 7), np.float32(0.25))
    assert ref.volume(v, 0.5, iso=0.25)[0] == 4 * 3 * 6 * 0.125
    assert ref.volume(v, 0.5, iso=np.nextafter(np.float32(0.25), np.float32(1)))[0] == 0.0
    assert ref.volume(v, 0.5, iso=0.0, shift=0.25)[0] == 4 * 3 * 6 * 0.125
    nfull, cut = ref.classify(v, shift=0.25, iso=1e-30)
    assert nfull == 0 and cut[0].size == 0


def test_volume_from_sdf_argument_errors(pkg):
    """rejected before any device work (so also without a GPU): null pointers and a lattice without cells"""
    L = pkg._lib.lib()
    a = np.zeros(27, dtype=np.float32)
    p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    v = ctypes.c_float(123.0)
    assert L.r2s_volume_from_sdf(None, 3, 3, 3, 1.0, 0.0, 9, 0, ctypes.byref(v)) == R2S_ERR_ARG
    assert L.r2s_volume_from_sdf(p, 3, 3, 3, 1.0, 0.0, 9, 0, None) == R2S_ERR_ARG
    for dims in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (0, 3, 3), (3, 3, -2)):
        assert L.r2s_volume_from_sdf(p, *dims, 1.0, 0.0, 9, 0, ctypes.byref(v)) == R2S_ERR_ARG, dims
    assert v.value == 123.0
