"""analyze_sdf_components (reference src/SignedDistances/SdfArtifactRemoval.jl:256-311) on the GPU: the standalone
entry points r2s_analyze_components(_dev) / r2s_last_components and the table r2s_rho2sdf keeps with
analyze_components, against scipy.ndimage.label (6-connectivity) as an independent reference."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

from conftest import block_mesh, load_fixture
from test_large_paths_gpu import _isolated_and_block

pytestmark = pytest.mark.gpu


def _expected(sdf, dims, threshold):
    """(roots, sizes) of the components of {sdf >= threshold}: 0-based first voxel (x fastest), in root order"""
    nx, ny, nz = dims
    lab, _ = ndimage.label(np.asarray(sdf).reshape(nz, ny, nx) >= threshold)   # (generate_binary_structure(3, 1))
    flat = lab.ravel()
    ids, first = np.unique(flat, return_index=True)
    keep = ids > 0
    roots, sizes = first[keep].astype(np.int64), np.bincount(flat)[ids[keep]].astype(np.int64)
    o = np.argsort(roots)
    return roots[o], sizes[o]


def _table(pkg, sdf, grid, threshold=0.0, capacity=None):
    """r2s_analyze_components -> (n, roots, sizes) with room for `capacity` entries (None: the full count)"""
    lib = pkg._lib.lib()
    n = ctypes.c_int64(-1)
    if capacity is None:
        pkg._lib.check(lib.r2s_analyze_components(sdf.ctypes.data_as(pkg._lib.c_double_p), ctypes.byref(grid.c),
                                                  float(threshold), -1, None, None, 0, ctypes.byref(n)))
        capacity = n.value
    roots, sizes = np.full(capacity, -7, np.int64), np.full(capacity, -7, np.int64)
    pkg._lib.check(lib.r2s_analyze_components(sdf.ctypes.data_as(pkg._lib.c_double_p), ctypes.byref(grid.c),
                                              float(threshold), -1, _i(roots), _i(sizes), capacity, ctypes.byref(n)))
    return n.value, roots, sizes


def _last(pkg):
    lib = pkg._lib.lib()
    n = ctypes.c_int64(-1)
    pkg._lib.check(lib.r2s_last_components(None, None, 0, ctypes.byref(n)))
    roots, sizes = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
    pkg._lib.check(lib.r2s_last_components(_i(roots), _i(sizes), n.value, ctypes.byref(n)))
    return roots, sizes


def _i(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _assert_table(pkg, sdf, grid, threshold, label=""):
    before = sdf.tobytes()
    n, roots, sizes = _table(pkg, sdf, grid, threshold)
    assert sdf.tobytes() == before, f"{label}: the field was modified"
    er, es = _expected(sdf, grid.dims, threshold)
    assert n == len(er), (label, n, len(er))
    assert np.array_equal(roots, er), label
    assert np.array_equal(sizes, es), label
    return roots, sizes


def _chapadlo(pkg, oracle):
    """the chapadlo raw SDF with 400 interior specks (test_stages_gpu.py::test_remove_artifacts)"""
    X, IEN, rho = load_fixture("chapadlo")
    rn = oracle.dense_in_nodes(X, IEN, rho)
    og, _ = oracle.auto_grid(X, IEN)
    d, _, _ = oracle.eval_distances(X, IEN, rn, 0.5, og, 1.1, want_xp=False)
    sdf = d * oracle.sign_detection(X, IEN, rn, 0.5, og)
    pg = pkg.noninteractive_sdf_grid_setup(pkg.Mesh(X, IEN))
    rng = np.random.default_rng(5)
    idx = rng.choice(sdf.size, 400, replace=False)
    sdf[idx] = np.abs(sdf[idx])
    return sdf, pg


def _noisy(pkg):
    """the noisy field of test_stages_gpu.py::test_remove_artifacts_many_components"""
    rng = np.random.default_rng(23)
    pg = pkg.Grid(np.zeros(3), np.array([2.0, 1.3, 0.9]), 70, 1)
    nx, ny, nz = pg.dims
    f = rng.normal(size=(nz, ny, nx))
    for ax in range(3):
        f = f + np.roll(f, 1, axis=ax)
    return (f - 0.8).ravel(), pg


def test_reference_field(pkg, oracle):
    sdf, pg = _chapadlo(pkg, oracle)
    for thr in (0.0, 0.3, -0.2):
        roots, sizes = _assert_table(pkg, sdf, pg, thr, f"chapadlo threshold {thr}")
        assert len(roots) > 1
        d = pkg.analyze_sdf_components(sdf, pg, threshold=thr)
        assert list(d.keys()) == (roots + 1).tolist() and list(d.values()) == sizes.tolist()


def test_noisy_field_with_a_short_root_list(pkg, monkeypatch):
    sdf, pg = _noisy(pkg)
    monkeypatch.delenv("R2S_CCL_ROOTS_CAP", raising=False)
    full = _assert_table(pkg, sdf, pg, 0.0, "noisy")
    assert len(full[0]) > 16                               # more roots than the capped list holds
    monkeypatch.setenv("R2S_CCL_ROOTS_CAP", "16")
    pkg._lib.lib().r2s_release_cache()
    capped = _assert_table(pkg, sdf, pg, 0.0, "noisy, 16 roots listed")
    assert all(np.array_equal(a, b) for a, b in zip(full, capped))
    monkeypatch.delenv("R2S_CCL_ROOTS_CAP")
    pkg._lib.lib().r2s_release_cache()


def test_more_components_than_the_root_list(pkg, monkeypatch):
    """205^3 checkerboard + block (test_large_paths_gpu.py): more than 2^22 components, +-0 and NaN voxels"""
    monkeypatch.delenv("R2S_CCL_ROOTS_CAP", raising=False)
    rng = np.random.default_rng(43)
    pg = pkg.Grid(np.zeros(3), np.ones(3), 202, 1)
    assert pg.dims == (205, 205, 205)
    f, iso = _isolated_and_block(pg.dims, lambda i, j, k: (i + j + k) % 2 == 0, 10, 50,
                                 [(0.0, 1000), (-0.0, 1000), (np.nan, 1000)], rng)
    sdf = f.reshape(-1)
    roots, sizes = _assert_table(pkg, sdf, pg, 0.0, "checkerboard")
    assert len(roots) > (1 << 22) and sizes.max() == 40 ** 3


def test_edge_cases(pkg):
    lib = pkg._lib.lib()
    pg = pkg.Grid(np.zeros(3), np.array([1.0, 0.8, 0.6]), 20, 1)
    out = -np.ones(pg.ngp)
    n, _, _ = _table(pkg, out, pg)
    assert n == 0 and pkg.analyze_sdf_components(out, pg) == {}
    inside = np.ones(pg.ngp)
    n, roots, sizes = _table(pkg, inside, pg)
    assert n == 1 and roots.tolist() == [0] and sizes.tolist() == [pg.ngp]
    sdf, pg = _noisy(pkg)
    n, roots, sizes = _table(pkg, sdf, pg)
    for cap in (0, n - 1):
        m, r, s = _table(pkg, sdf, pg, capacity=cap)
        assert m == n and np.array_equal(r, roots[:cap]) and np.array_equal(s, sizes[:cap])
    z = ctypes.c_int64(-1)
    p = sdf.ctypes.data_as(pkg._lib.c_double_p)
    buf = np.empty(4, np.int64)
    assert lib.r2s_analyze_components(p, ctypes.byref(pg.c), 0.0, -1, None, None, 4, ctypes.byref(z)) == -1
    assert lib.r2s_analyze_components(p, ctypes.byref(pg.c), 0.0, -1, _i(buf), None, 4, ctypes.byref(z)) == -1
    assert lib.r2s_last_components(None, _i(buf), 4, ctypes.byref(z)) == -1
    with pytest.raises(pkg._lib.R2SError, match="doesn't match grid points"):
        pkg.analyze_sdf_components(np.zeros(7), pg)


def test_device_variant(pkg):
    import torch
    sdf, pg = _noisy(pkg)
    _, roots, sizes = _table(pkg, sdf, pg)
    d = torch.from_numpy(sdf).to("cuda:0")
    before = d.clone()
    lib = pkg._lib.lib()
    n = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pkg._lib.check(lib.r2s_analyze_components_dev(ctypes.c_void_p(d.data_ptr()), ctypes.byref(pg.c), 0.0, stream, None,
                                                  None, 0, ctypes.byref(n)))
    assert n.value == len(roots)
    r2, s2 = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
    pkg._lib.check(lib.r2s_analyze_components_dev(ctypes.c_void_p(d.data_ptr()), ctypes.byref(pg.c), 0.0, stream, _i(r2),
                                                  _i(s2), n.value, ctypes.byref(n)))
    torch.cuda.synchronize()
    assert np.array_equal(r2, roots) and np.array_equal(s2, sizes)
    assert torch.equal(d, before)
    lr, ls = _last(pkg)
    assert np.array_equal(lr, roots) and np.array_equal(ls, sizes)


@pytest.mark.parametrize("field", ["chapadlo", "noisy"])
def test_agrees_with_removal(pkg, oracle, field):
    sdf, pg = _chapadlo(pkg, oracle) if field == "chapadlo" else _noisy(pkg)
    _, roots, sizes = _table(pkg, sdf, pg)
    big = int(np.argmax(sizes))                            # the first root of maximal size is kept
    for ratio in (0.01, 0.5):
        min_size = max(1, round(ratio * int(sizes[big])))  # (Python's round: ties to even, like Julia's)
        small = sizes < min_size
        small[big] = False
        a = sdf.copy()
        assert pkg.remove_sdf_artifacts(a, pg, min_component_ratio=ratio) == int(sizes[small].sum()), (field, ratio)


def _raw_field(pkg, X, IEN, rho, opts, grid):
    """the raw field of r2s_rho2sdf (api.rho2sdf passes no sdf_raw_out): the same call through the C ABI, one device"""
    L = pkg._lib
    mesh = pkg.Mesh(X, IEN)
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    o = L.R2SOptions()
    L.lib().r2s_default_options(ctypes.byref(o))
    if opts.threshold_density is not None:
        o.threshold_density = float(opts.threshold_density)
    o.elem_type = mesh.element_type
    o.rbf_interp = int(bool(opts.rbf_interp))
    o.artifact_min_component_ratio = float(opts.artifact_min_component_ratio)
    o.skip_rbf = 1
    raw, dists = np.empty(grid.ngp), np.empty(grid.ngp)
    L.check(L.lib().r2s_rho2sdf(mesh.X.ctypes.data_as(L.c_double_p), mesh.nnp, mesh.IEN.ctypes.data_as(L.c_int64_p),
                                mesh.nel, rho.ctypes.data_as(L.c_double_p), ctypes.byref(o), ctypes.byref(grid.c), None,
                                raw.ctypes.data_as(L.c_double_p), dists.ctypes.data_as(L.c_double_p), None, None))
    return raw


def _in_call_inputs(pkg, which):
    if which == "beam":                                    # config 2
        X, IEN, rho = load_fixture("beam_vfrac_03")
        opts = dict(sdf_grid_setup="automatic", rbf_interp=False)
        grid = pkg.noninteractive_sdf_grid_setup(pkg.Mesh(X, IEN))
    else:                                                  # random densities: components across slab interfaces
        X, IEN = block_mesh((14, 10, 24))
        rho = np.random.default_rng(29).uniform(0.0, 1.0, len(IEN))
        opts = dict(threshold_density=0.62, rbf_interp=True, artifact_min_component_ratio=0.05)
        grid = pkg.Grid(X.min(0), X.max(0), 40, 2)
    return X, IEN, rho, opts, grid


@pytest.mark.parametrize("which", ["beam", "block"])
def test_in_call_analysis(pkg, monkeypatch, which):
    X, IEN, rho, opts, grid = _in_call_inputs(pkg, which)
    raw = _raw_field(pkg, X, IEN, rho, pkg.Rho2sdfOptions(**opts), grid)
    want = pkg.analyze_sdf_components(raw, grid)
    assert len(want) >= (50 if which == "block" else 1)
    monkeypatch.setenv("R2S_MULTI_OVERSUBSCRIBE", "1")
    for G in (1, 2, 3, 8):
        on, off = {}, {}
        a = pkg.rho2sdf("t", X, IEN, rho, options=pkg.Rho2sdfOptions(export_analysis=True, **opts), sdf_grid=grid,
                        n_gpus=G, info=on)
        b = pkg.rho2sdf("t", X, IEN, rho, options=pkg.Rho2sdfOptions(**opts), sdf_grid=grid, n_gpus=G, info=off)
        assert on["components_before"] == want, (which, G)
        assert list(on["components_before"]) == sorted(want), (which, G)
        assert "components_before" not in off
        assert on["n_flipped"] == off["n_flipped"], (which, G)
        assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), (which, G, "sdf_dists")
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (which, G, "fine_sdf")
    pkg._lib.lib().r2s_release_cache()
