"""r2s_release_cache() against the eleven per-device work caches (PerDevice in r2s_internal.hpp): shells, sections, weld, orient,
fans, holes, intersections, nesting, the distance calls, the component labelling and the device extraction.  Every family is
called once, the cache is released, and every family is called again on fresh buffers: the same bits.  r2s_live_device_bytes()
grows with the calls and is back at its value from before them after the release (include/rho2sdf_hip.h)."""
import gc

import numpy as np
import pytest

import mesh_holes_cases as CH
import mesh_sections_cases as CX
import mesh_shells_cases as S

pytestmark = pytest.mark.gpu


def _flat(x, name="", out=None):
    """every array and scalar of a result, by name, as (dtype, shape, bytes)"""
    out = {} if out is None else out
    if x is None or isinstance(x, (bool, int, float, str)):
        out[name] = x
    elif isinstance(x, np.ndarray) or np.isscalar(x):
        a = np.ascontiguousarray(x)
        out[name] = (str(a.dtype), a.shape, a.tobytes())
    elif isinstance(x, dict):
        for k in sorted(x):
            _flat(x[k], f"{name}[{k}]", out)
    elif isinstance(x, (list, tuple)):
        for k, v in enumerate(x):
            _flat(v, f"{name}[{k}]", out)
    else:
        for k, v in sorted(vars(x).items()):
            _flat(v, f"{name}.{k}", out)
    return out


def _families(pkg):
    V, T = S.case("cube_with_void")
    Vh, Th = CH.case("tube_and_cube")
    Vx, Tx, normal, levels = CX.case("cube_with_void")
    grid = pkg.Grid(np.zeros(3), np.ones(3), 6, 1)
    n = [int(k) + 1 for k in grid.c.N]
    c = np.indices(n[::-1]).reshape(3, -1).T / (np.array(n[::-1]) - 1.0)
    sdf = 0.3 - np.linalg.norm(c - 0.5, axis=1) + np.where((c < 0.1).all(1), 1.0, 0.0)   # a ball and a corner blob

    def extracted():
        import torch
        return [x.cpu().numpy() for x in pkg.extract_isosurface_dev(torch.from_numpy(sdf).cuda(), grid)]

    return {
        "shells": lambda: pkg.mesh_shells(V, T),
        "sections": lambda: pkg.mesh_sections(Vx, Tx, normal, levels),
        "weld": lambda: pkg.mesh_weld(V[T].reshape(-1, 3)),
        "orient": lambda: pkg.mesh_orient(V, T, outward=True),
        "fans": lambda: pkg.mesh_fans(V, T, split=True),
        "holes": lambda: pkg.mesh_holes(Vh, Th, fill=-1),
        "intersect": lambda: pkg.mesh_intersections(V, T),
        "distance": lambda: pkg.mesh_distance(V, T, ((9, 9, 9), (-0.5, -0.5, -0.5), 0.375), 1.0, want_index=True),
        "components": lambda: pkg.analyze_sdf_components(sdf, grid),
        "nesting": lambda: pkg.mesh_nesting(V, T, rewind=True),
        "extraction": extracted,
    }


def test_every_family_gives_the_same_bits_after_release_cache(pkg):
    calls = _families(pkg)
    live = pkg._lib.lib().r2s_live_device_bytes
    gc.collect()                                             # (no handle of an earlier test is freed in between)
    pkg._lib.lib().r2s_release_cache()
    b0 = live()
    before = {k: _flat(f()) for k, f in calls.items()}
    assert len(before["components"]) == 2 and before["shells"][".totals"] is not None
    assert len(before["extraction"]["[1]"][2]) > 0 and before["nesting"][".totals"] is not None
    assert live() > b0
    pkg._lib.lib().r2s_release_cache()
    assert live() == b0
    for k, f in calls.items():
        assert _flat(f()) == before[k], k
    pkg._lib.lib().r2s_release_cache()                       # released twice in a row: nothing left to free
    pkg._lib.lib().r2s_release_cache()
    assert live() == b0
    assert _flat(calls["shells"]()) == before["shells"]
