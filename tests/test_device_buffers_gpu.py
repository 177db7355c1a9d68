"""Device buffers free themselves (DevBuf in csrc/r2s_common.hpp): r2s_live_device_bytes() counts what the library's own
buffers hold, so that a leak shows as a counter that does not come back - the free memory the runtime reports is shared with
other processes and says nothing.  Every case: release the caches, read the counter, make the calls, release the caches, and
the counter is where it was.  A: calls that succeed, B: calls rejected after they have allocated (host-side argument checks
only), C: the handles."""
import gc
import re

import numpy as np
import pytest

import mesh_shells_cases as S
from conftest import load_fixture

pytestmark = pytest.mark.gpu

LATTICE = ((9, 9, 9), (-0.5, -0.5, -0.5), 0.375)   # 9^3 points around the cube of side 2


def _live(pkg):
    return int(pkg._lib.lib().r2s_live_device_bytes())


class _Frame:
    """with _Frame(pkg) as f: ... - the caches are released before and after, and the counter must return to f.L0"""

    def __init__(self, pkg):
        self.pkg = pkg

    def __enter__(self):
        self.pkg._lib.lib().r2s_release_cache()
        self.L0 = _live(self.pkg)
        return self

    def __exit__(self, et, ev, tb):
        self.pkg._lib.lib().r2s_release_cache()
        if et is None:
            assert _live(self.pkg) == self.L0, (_live(self.pkg), self.L0)


@pytest.fixture(scope="module")
def sphere(pkg):
    """the sphere fixture on 6 cells per axis (4 across the mesh, a margin of 1) with everything the stages need, computed once"""
    X, IEN, rho = load_fixture("sphere")
    mesh = pkg.Mesh(X, IEN)
    grid = pkg.Grid(X.min(0), X.max(0), 4, 1)
    assert grid.N.max() <= 6
    rho_n = pkg.DenseInNodes(mesh, rho)
    vd, vf = pkg.calculate_mesh_volume(mesh, rho)
    sdf = pkg.sdf_fused(mesh, grid, rho_n, 0.5, band_factor=2.5)
    return dict(X=X, IEN=IEN, rho=rho, mesh=mesh, grid=grid, rho_n=rho_n, target=vd * vf, sdf=sdf)


def _bits(x):
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, _bits(x[k])) for k in sorted(x))
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    return np.asarray(x).tobytes() if isinstance(x, (float, np.floating)) else x


# ---- A: calls that succeed ----------------------------------------------------------------------------------------------------
def _pre(pkg, s):
    m = s["mesh"]
    return (pkg.calculate_mesh_volume(m, s["rho"]), pkg.DenseInNodes(m, s["rho"]),
            pkg.find_threshold_for_volume(m, s["rho_n"], s["target"]), pkg.calculate_isocontour_volume(m, s["rho_n"], 0.5))


def _post(pkg, s):
    fine = pkg.RBFs_smoothing(s["sdf"], s["grid"], True, 1, s["target"])
    return (pkg.calculate_volume_from_sdf(fine, s["grid"].cell_size), pkg.remove_sdf_artifacts(s["sdf"].copy(), s["grid"]),
            pkg.analyze_sdf_components(s["sdf"], s["grid"]))


def _rbf(pkg, s):
    return tuple(pkg.RBFs_smoothing(s["sdf"], s["grid"], interp, 1, s["target"]) for interp in (True, False))


def _fused(pkg, s):
    return pkg.sdf_fused(s["mesh"], s["grid"], s["rho_n"], 0.5, band_factor=2.5)


def _mesh_calls(pkg, s):
    V, T = S.case("cube_with_void")
    fine = pkg.RBFs_smoothing(s["sdf"], s["grid"], True, 1, s["target"])
    return (pkg.extract_isosurface(fine, s["grid"], 1), pkg.mesh_distance(V, T, LATTICE, 1.0, want_index=True),
            pkg.mesh_signed_distance(V, T, LATTICE))


def _rho2sdf(pkg, s, n_gpus=1):
    opts = pkg.Rho2sdfOptions(threshold_density=0.5, rbf_grid="fine")
    out = pkg.rho2sdf("t", s["X"], s["IEN"], s["rho"], options=opts, sdf_grid=s["grid"], n_gpus=n_gpus)
    return out[0], out[3]


@pytest.mark.parametrize("family", [_pre, _post, _rbf, _fused, _mesh_calls, _rho2sdf], ids=lambda f: f.__name__.strip("_"))
def test_successful_calls_return_what_they_took(pkg, sphere, family):
    with _Frame(pkg) as f:
        first = _bits(family(pkg, sphere))
        assert _live(pkg) >= f.L0
        assert _bits(family(pkg, sphere)) == first          # (the second call runs on whatever the first one cached)


def test_slab_paths_return_what_they_took(pkg, sphere, monkeypatch):
    """rho2sdf over two devices: the slab smoothing and the slab artifact removal.  With one visible device the two logical
    devices share it (R2S_MULTI_OVERSUBSCRIBE)."""
    import torch
    if torch.cuda.device_count() < 2:
        monkeypatch.setenv("R2S_MULTI_OVERSUBSCRIBE", "1")
    with _Frame(pkg):
        one = _bits(_rho2sdf(pkg, sphere))
        assert _bits(_rho2sdf(pkg, sphere, n_gpus=2)) == one


# ---- B: calls rejected after they have allocated ----------------------------------------------------------------------------------
def _bad_threshold(pkg, s, bad):
    return pkg.find_threshold_for_volume(s["mesh"], s["rho_n"], 1e6 if bad else s["target"])


def _bad_ien(pkg, s, bad):
    IEN = s["IEN"].copy()
    if bad:
        IEN[len(IEN) // 2, 3] = len(s["X"]) + 1
    return pkg.calculate_mesh_volume(pkg.Mesh(s["X"], IEN), s["rho"])


def _bad_field(pkg, s, bad):
    return pkg.RBFs_smoothing(np.full(s["grid"].ngp, -1.0e10) if bad else s["sdf"], s["grid"], True, 1, s["target"])


def _bad_triangle(pkg, s, bad):
    V, T = S.case("cube_with_void")
    T = T.copy()
    if bad:
        T[7, 1] = len(V)
    return pkg.mesh_signed_distance(V, T, LATTICE)


NUM = r"[-+0-9.e]+"
REJECTED = [
    (_bad_threshold, rf"rho2sdf_hip error -1: Requested volume 1000000 is outside the possible range \[{NUM}, {NUM}\]"),
    (_bad_ien, r"rho2sdf_hip error -1: IEN contains node ids outside 1\.\.nnp"),
    (_bad_field, r"rho2sdf_hip error -1: every SDF value is a sentinel: nothing to smooth"),
    (_bad_triangle, r"rho2sdf_hip error -1: mesh_signed_distance: triangle 7 has vertex index 16 outside \[0, 16\)"),
]


@pytest.mark.parametrize("call,text", REJECTED, ids=[c.__name__.strip("_") for c, _ in REJECTED])
def test_rejected_calls_return_what_they_took(pkg, sphere, call, text):
    with _Frame(pkg) as f:
        before = _bits(call(pkg, sphere, False))
        pkg._lib.lib().r2s_release_cache()
        assert _live(pkg) == f.L0
        with pytest.raises(pkg._lib.R2SError) as e:
            call(pkg, sphere, True)
        assert re.fullmatch(text, str(e.value)), str(e.value)
        pkg._lib.lib().r2s_release_cache()
        assert _live(pkg) == f.L0, (call.__name__, _live(pkg) - f.L0)
        assert _bits(call(pkg, sphere, False)) == before


# ---- C: handles -----------------------------------------------------------------------------------------------------------------
def test_handles_hold_memory_until_they_are_freed(pkg, sphere):
    import torch
    V, T = S.case("cube_with_void")
    pts = np.array([[1.0, 1.0, 1.0], [3.0, 0.5, 0.25]], np.float32)
    with _Frame(pkg) as f:
        ix = pkg.MeshIndex(V, T)                              # close()
        assert _live(pkg) > f.L0
        d = ix.distance(pts)
        pkg._lib.lib().r2s_release_cache()                   # (live handles survive it)
        assert _live(pkg) > f.L0 and np.array_equal(ix.distance(pts), d)
        ix.close()
        pkg._lib.lib().r2s_release_cache()
        assert _live(pkg) == f.L0

        with pkg.MeshIndex(V, T):                             # the context manager
            assert _live(pkg) > f.L0
        pkg._lib.lib().r2s_release_cache()
        assert _live(pkg) == f.L0

        field = pkg.fit_rbf_field(sphere["sdf"], sphere["grid"], True, sphere["target"])   # del + gc.collect()
        pkg._lib.lib().r2s_release_cache()
        assert _live(pkg) > f.L0
        del field
        gc.collect()
        assert _live(pkg) == f.L0

        # a plan allocates on its first run, not when it is created
        plan = pkg.DevicePlan(0)
        assert _live(pkg) == f.L0
        dev = torch.device("cuda:0")
        out = torch.empty(sphere["grid"].ngp, dtype=torch.float64, device=dev)
        plan.run(torch.from_numpy(sphere["X"]).to(dev), torch.from_numpy(sphere["IEN"]).to(dev),
                 torch.from_numpy(sphere["rho_n"]).to(dev), 0.5, sphere["grid"], band_factor=2.5, sdf=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), sphere["sdf"])
        assert _live(pkg) > f.L0
        plan.close()
        assert _live(pkg) == f.L0
