"""The per-voxel gather (sdf_tiles_kernel) against the CPU oracle, bit for bit, on the inputs where its list entries decide.

The list sort writes, per (tile, list entry), the storage chunk of the tile inside the entry's result array and a 12-bit
mask (4 bits per axis: which voxel planes of the tile pass the entry's range test); the gather only broadcasts these words
and tests three bits.  A wrong bit or chunk shows as a voxel that takes a candidate it must not see, misses one, or reads
another tile's results - every such voxel differs from the oracle in `dist`, `sign`, `sdf` or `xp`.  No tolerance: the
kernels keep the oracle's operation order, and the gather computes no double itself.

Cases (all small: the largest grid has 46^3 points):
  partial tiles    no grid dimension is a multiple of 4: the last tile of every axis has voxels off the grid
  long lists       a mesh finer than the grid: lists beyond the 64 entries one batch of the list walk fetches
  large elements   item / element boxes that span many tiles: the chunk index inside the box matters
  Z slabs          planes [k_begin, k_end) and interleaved tile layers (zstride 2 and 3, every zphase), stitched
  true_min         the order-independent rules of the same walks
  TET4             the band walk with boundary triangles, the sign walk that keeps evaluating its candidates itself
  far mesh         a mesh (and grid) thousands of cells away from the origin
"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIELDS = ("dist", "sign", "sdf", "xp")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _oracle_fields(oracle, X, IEN, rn, rt, og, true_min=False):
    with (oracle.true_min() if true_min else contextlib.nullcontext()):
        d, xp, _ = oracle.eval_distances(X, IEN, rn, rt, og, 1.1)
        s = oracle.sign_detection(X, IEN, rn, rt, og)
    return {"dist": d, "sign": s, "sdf": d * s, "xp": xp}


def _assert_bits(got, ref, label):
    bad = {}
    for key in FIELDS:
        g, r = np.asarray(got[key]).reshape(np.asarray(ref[key]).shape), ref[key]
        ne = _bits(g) != _bits(r)
        if ne.any():
            where = np.argwhere(ne.any(axis=-1) if key == "xp" else ne)
            bad[key] = (len(where), where[:5].ravel().tolist())
    assert not bad, f"{label}: voxels that differ from the oracle (count, first flat indices) {bad}"


def _check(pkg, oracle, X, IEN, rn, rt, pg, og, label, true_min=False):
    """the three host entry points (distance-only, sign-only and fused instantiations of the gather) == oracle;
    returns the work counts of the fused call"""
    assert pg.dims == og.dims
    mesh = pkg.Mesh(X, IEN)
    st = {}
    dist, xp = pkg.evalDistances(mesh, pg, rn, rt, true_min=true_min)
    sign = pkg.Sign_Detection(mesh, pg, rn, rt, true_min=true_min)
    sdf = pkg.sdf_fused(mesh, pg, rn, rt, true_min=true_min, stats=st)
    ref = _oracle_fields(oracle, X, IEN, rn, rt, og, true_min)
    _assert_bits({"dist": dist, "sign": sign, "sdf": sdf, "xp": xp}, ref, label)
    real = ref["dist"] < 1e9
    assert real.sum() > 100 and (ref["sign"] > 0).sum() > 100, f"{label}: the case has lost its band or its inside"
    print(f"{label}: grid {pg.dims}, {int(real.sum())} band voxels, {int((ref['sign'] > 0).sum())} inside, "
          f"band entries {st['n_band_entries']} in {st['n_active_tiles']} tiles, "
          f"sign entries {st['n_sign_entries']} in {st['n_active_sign_tiles']} tiles: dist, sign, sdf, xp bit-equal")
    return st


def _grids(pkg, oracle, X, n_max):
    return pkg.Grid(X.min(0), X.max(0), n_max, 3), oracle.grid_make(X.min(0), X.max(0), n_max, 3)


def test_partial_tiles(pkg, oracle):
    """the 4^3-element jittered hex mesh, squeezed per axis so that the three grid dimensions leave the residues
    1, 2 and 3 mod 4: upper mask bits and `valid` in the last tile of every axis"""
    from rho2sdf_jl_amd import synthetic
    X, IEN, rn = synthetic.hex_mesh(4)
    X = X * np.array([1.0, 0.875, 0.84375])
    pg, og = _grids(pkg, oracle, X, 22)
    assert sorted(d % 4 for d in pg.dims) == [1, 2, 3], pg.dims
    _check(pkg, oracle, X, IEN, rn, 0.5, pg, og, "partial tiles")


def test_long_lists(pkg, oracle):
    """20^3 elements on a 24^3 grid (the construction of test_parity_gpu.test_mesh_finer_than_grid): the mean list
    length, hence the longest, is beyond the 64 entries of one batch - in the band lists and in the sign lists"""
    from rho2sdf_jl_amd import synthetic
    X, IEN, rn = synthetic.hex_mesh(20)
    pg, og = _grids(pkg, oracle, X, synthetic.grid_n_max_for_points(24))
    st = _check(pkg, oracle, X, IEN, rn, 0.5, pg, og, "long lists")
    assert st["n_band_entries"] > 64 * st["n_active_tiles"] > 0, st
    assert st["n_sign_entries"] > 64 * st["n_active_sign_tiles"] > 0, st


def test_large_elements(pkg, oracle):
    """8 elements on a 46^3 grid: every item box and every element box spans about 6^3 tiles, so the chunk of a tile
    inside the box takes every value of a three-axis index"""
    from rho2sdf_jl_amd import synthetic
    X, IEN, _ = synthetic.hex_mesh(2, jitter=0.1)
    rn = np.clip(1.2 - np.linalg.norm(X, axis=1), 0.0, 1.0)
    pg, og = _grids(pkg, oracle, X, synthetic.grid_n_max_for_points(45))
    st = _check(pkg, oracle, X, IEN, rn, 0.5, pg, og, "large elements")
    assert st["n_sign_entries"] >= 8 * 100, st   # an element is listed in > 100 tiles


@pytest.fixture(scope="module")
def slab_case(pkg, oracle):
    """mesh, grids and the oracle's fields for the slab runs, computed once, read-only"""
    from rho2sdf_jl_amd import synthetic
    X, IEN, rn = synthetic.hex_mesh(6, jitter=0.3, seed=20240503)
    X = X * np.array([1.0, 0.90625, 1.0])
    pg, og = _grids(pkg, oracle, X, 24)
    ref = _oracle_fields(oracle, X, IEN, rn, 0.5, og)
    for a in ref.values():
        a.setflags(write=False)
    return X, IEN, rn, pg, ref


def _plan_fields(torch, plan, dev_mesh, pg, names, planes, **kw):
    nx, ny, _ = pg.dims
    out = {n: torch.full((planes * ny * nx * (3 if n == "xp" else 1),), 7.0, dtype=torch.float64, device=dev_mesh[0].device)
           for n in names}
    plan.run(*dev_mesh, 0.5, pg, **kw, **out)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().reshape((planes, ny, nx, 3) if n == "xp" else (planes, ny, nx)) for n, t in out.items()}


@pytest.mark.parametrize("names", [("sdf",), FIELDS], ids=["sdf", "all_outputs"])
def test_z_slabs(pkg, oracle, slab_case, names):
    """the plan API in one slab, in three slabs of planes whose bounds are no multiples of 4, and in the interleaved
    tile layers of 2 and 3 ranks with every phase: each stitched field == the oracle's.  (`sdf` alone takes the lean /
    sign-only instantiations and, from the second call of a shape on, the early projection; all outputs take the
    general instantiation with projection points.)"""
    import torch
    from rho2sdf_jl_amd import slabs
    X, IEN, rn, pg, ref = slab_case
    nx, ny, nz = pg.dims
    assert nz % 4 != 0 and nz > 24
    dev = torch.device("cuda:0")
    dev_mesh = tuple(torch.from_numpy(a).to(dev) for a in (X, IEN, rn))
    want = {n: ref[n].reshape((nz, ny, nx, 3) if n == "xp" else (nz, ny, nx)) for n in names}
    plan = pkg.DevicePlan(0)
    try:
        for rep in range(2):   # the second run of a shape goes by the sizes the first one left
            one = _plan_fields(torch, plan, dev_mesh, pg, names, nz)
            for n in names:
                assert np.array_equal(_bits(one[n]), _bits(want[n])), f"one slab, run {rep}: {n} differs from the oracle"
        bounds = (0, 5, 14, nz)
        pieces = [_plan_fields(torch, plan, dev_mesh, pg, names, b - a, k_begin=a, k_end=b) for a, b in zip(bounds[:-1], bounds[1:])]
        for n in names:
            got = np.concatenate([p[n] for p in pieces])
            assert np.array_equal(_bits(got), _bits(want[n])), f"planes {bounds}: {n} differs from the oracle"
        for world in (2, 3):
            got = {n: np.full_like(want[n], 7.0) for n in names}
            for r in range(world):
                owned, _ = slabs.interleaved_layers(nz, world, r)
                part = _plan_fields(torch, plan, dev_mesh, pg, names, 4 * owned, zstride=world, zphase=r)
                for layer in range(owned):
                    k = 4 * (layer * world + r)
                    m = min(4, nz - k)
                    for n in names:
                        got[n][k:k + m] = part[n][4 * layer:4 * layer + m]
            for n in names:
                assert np.array_equal(_bits(got[n]), _bits(want[n])), f"zstride {world}: {n} differs from the oracle"
    finally:
        plan.close()


def _solid_boundary(synthetic):
    """radial density on a 6^3 cube, rho_t = 0.05: solid elements with boundary faces and iso elements with
    validated boundary triangles - band lists that mix triangles and iso items"""
    X, IH, rn = synthetic.radial_cube(6, 6.0)
    return X, IH, rn, 0.05


@pytest.mark.parametrize("true_min", [False, True], ids=["ordered", "true_min"])
def test_hex8_with_triangles(pkg, oracle, true_min):
    from rho2sdf_jl_amd import synthetic
    X, IH, rn, rt = _solid_boundary(synthetic)
    pg, og = _grids(pkg, oracle, X, 23)
    assert all(d % 4 for d in pg.dims)
    _check(pkg, oracle, X, IH, rn, rt, pg, og, f"hex8 solid boundary true_min={true_min}", true_min)


def test_true_min_distorted_hexes(pkg, oracle):
    """strongly distorted elements with random densities: several elements hold a voxel within the 1 % zone, ties
    between candidates - the order-independent rules of both walks"""
    from rho2sdf_jl_amd import synthetic
    X, IEN, _ = synthetic.hex_mesh(5, jitter=0.3, seed=20240502)
    rn = np.clip(np.random.default_rng(1).normal(0.5, 0.35, len(X)), 0, 1)
    pg, og = _grids(pkg, oracle, X, 23)
    _check(pkg, oracle, X, IEN, rn, 0.5, pg, og, "distorted hexes true_min", True)


@pytest.mark.parametrize("true_min", [False, True], ids=["ordered", "true_min"])
def test_tet4(pkg, oracle, true_min):
    from rho2sdf_jl_amd import synthetic
    X, IH, rn, rt = _solid_boundary(synthetic)
    pg, og = _grids(pkg, oracle, X, 23)
    _check(pkg, oracle, X, synthetic.hex_to_tets(IH), rn, rt, pg, og, f"tet4 solid boundary true_min={true_min}", true_min)


def test_far_mesh(pkg, oracle):
    """the mesh of the partial-tile case thousands of its own lengths away from the origin, another distance per axis:
    the masks are computed from the same coordinates and cell indices as the oracle's tests, wherever the grid lies"""
    from rho2sdf_jl_amd import synthetic
    X, IEN, rn = synthetic.hex_mesh(4)
    X = X * np.array([1.0, 0.875, 0.84375]) + np.array([4096.0, -1024.0, 2.0 ** 20])
    pg, og = _grids(pkg, oracle, X, 22)
    assert all(d % 4 for d in pg.dims)
    _check(pkg, oracle, X, IEN, rn, 0.5, pg, og, "far mesh")
