"""The self-intersection entry points on the GPU (include/rho2sdf_hip.h, r2s_mesh_index_intersections) against the numpy
restatement of tests/mesh_intersect_ref.py on the named cases of tests/mesh_intersect_cases.py: pairs, hits_of_tri and totals are
EQUAL, from the host, the device and the index variants; the capacity protocol; refusals; the index is left as it was."""
import ctypes
import os

import numpy as np
import pytest

import mesh_intersect_cases as C

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _equal(label, got, want):
    pairs, hits, tot = want
    gp = got.pairs if isinstance(got.pairs, np.ndarray) else got.pairs.cpu().numpy()
    gh = got.hits_of_tri if isinstance(got.hits_of_tri, np.ndarray) else got.hits_of_tri.cpu().numpy()
    assert np.array_equal(got.totals, tot), (label, got.totals, tot)
    assert gp.dtype == np.int32 and gp.shape == pairs.shape and np.array_equal(gp, pairs), label
    assert gh.dtype == np.int32 and np.array_equal(gh, hits), label
    assert len(got) == tot[0]
    tris = got.tris if isinstance(got.tris, np.ndarray) else got.tris.cpu().numpy()
    assert np.array_equal(tris, np.nonzero(hits)[0]), label


@pytest.mark.parametrize("name", C.ALL)
def test_cases_all_entry_points(pkg, name):
    V, T = C.case(name)
    want = C.expected(name)
    _equal(f"{name} host", pkg.mesh_intersections(V, T, device=0), want)
    _equal(f"{name} host again", pkg.mesh_intersections(V, T, device=0), want)
    dV, dT = _dev(V), _dev(T)
    _equal(f"{name} dev", pkg.mesh_intersections_dev(dV, dT), want)
    _equal(f"{name} dev with room", pkg.mesh_intersections_dev(dV, dT, capacity=int(want[2][0]) + 3), want)
    with pkg.MeshIndex(V, T, device=0) as ix:
        _equal(f"{name} index", ix.self_intersections(), want)
        _equal(f"{name} index dev", ix.self_intersections_dev(), want)
        counts = ix.self_intersections(want_pairs=False)
        assert counts.pairs is None and np.array_equal(counts.totals, want[2]) and np.array_equal(counts.hits_of_tri, want[1])
    with pkg.MeshIndex(dV, dT) as ix:
        _equal(f"{name} index of a device mesh", ix.self_intersections_dev(), want)


@pytest.mark.parametrize("variant", ["index", "mesh"])
def test_capacity_protocol(pkg, variant):
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("random200")
    pairs, hits, tot = C.expected("random200")
    n = int(tot[0])
    dV, dT = _dev(V), _dev(T)
    ix = pkg.MeshIndex(V, T, device=0) if variant == "index" else None

    def host(hits_out, pairs_out, cap, totals):
        ip = lambda a: a.ctypes.data_as(L.c_int32_p) if a is not None else None   # noqa: E731
        pt = totals.ctypes.data_as(L.c_int64_p)
        if ix:
            return lib.r2s_mesh_index_intersections(ix._handle(), ip(hits_out), ip(pairs_out), cap, pt)
        return lib.r2s_mesh_intersections(V.ctypes.data_as(L.c_float_p), len(V), T.ctypes.data_as(L.c_int32_p), len(T), 0, ip(hits_out),
                                          ip(pairs_out), cap, pt)

    def dev(hits_out, pairs_out, cap, totals):
        p = lambda t: vp(t.data_ptr()) if t is not None else None   # noqa: E731
        pt = totals.ctypes.data_as(L.c_int64_p)
        st = vp(torch.cuda.current_stream().cuda_stream)
        if ix:
            return lib.r2s_mesh_index_intersections_dev(ix._handle(), p(hits_out), p(pairs_out), cap, pt, st)
        return lib.r2s_mesh_intersections_dev(p(dV), len(V), p(dT), len(T), p(hits_out), p(pairs_out), cap, pt, st)

    try:
        for cap in (0, n - 1, n, n + 3):
            room = max(cap, n) + 5
            h, p, t = np.full(len(T), -7, np.int32), np.full((room, 2), -7, np.int32), np.full(8, -7, np.int64)
            assert host(h, p if cap else None, cap, t) == 0
            assert np.array_equal(t, tot) and np.array_equal(h, hits)
            written = n if cap >= n else 0
            assert np.array_equal(p[:written], pairs[:written]) and (p[written:] == -7).all(), cap
            dh, dp, t = _dev(np.full(len(T), -7, np.int32)), _dev(np.full((room, 2), -7, np.int32)), np.full(8, -7, np.int64)
            assert dev(dh, dp if cap else None, cap, t) == 0
            p = dp.cpu().numpy()
            assert np.array_equal(t, tot) and np.array_equal(dh.cpu().numpy(), hits)
            assert np.array_equal(p[:written], pairs[:written]) and (p[written:] == -7).all(), cap
        t = np.full(8, -7, np.int64)
        assert host(None, None, 0, t) == 0 and np.array_equal(t, tot)             # hits_of_tri may be NULL
        t = np.full(8, -7, np.int64)
        assert dev(None, None, 0, t) == 0 and np.array_equal(t, tot)
    finally:
        if ix:
            ix.close()


def test_index_is_unchanged(pkg):
    """distance and ray queries give their previous answers after self_intersections, and the intersections repeat"""
    V, T = C.case("two_spheres")
    rng = np.random.default_rng(3)
    lo, hi = V.min(axis=0), V.max(axis=0)
    pts = rng.uniform(lo - 0.5, hi + 0.5, size=(500, 3))
    o, d = rng.uniform(lo - 0.5, hi + 0.5, size=(500, 3)), rng.normal(size=(500, 3))
    with pkg.MeshIndex(V, T, device=0) as ix:
        info = ix.info()
        d0, i0 = ix.distance(pts, want_index=True)
        r0 = ix.raycast(o, d, want_index=True, want_side=True)
        a = ix.self_intersections()
        assert ix.info() == info
        d1, i1 = ix.distance(pts, want_index=True)
        r1 = ix.raycast(o, d, want_index=True, want_side=True)
        b = ix.self_intersections()
    assert np.array_equal(d0, d1) and np.array_equal(i0, i1)
    assert all(np.array_equal(x, y) for x, y in zip(r0, r1))
    _equal("two_spheres through the index", a, C.expected("two_spheres"))
    _equal("two_spheres again", b, C.expected("two_spheres"))


def test_argument_errors_leave_outputs_untouched(pkg):
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("random64")
    n = len(T)
    h, p, t = np.full(n, -7, np.int32), np.full((64, 2), -7, np.int32), np.full(8, -7, np.int64)
    ph, pp, pt = h.ctypes.data_as(L.c_int32_p), p.ctypes.data_as(L.c_int32_p), t.ctypes.data_as(L.c_int64_p)
    pv, ptr = V.ctypes.data_as(L.c_float_p), T.ctypes.data_as(L.c_int32_p)
    bad_index = T.copy()
    bad_index[5, 1] = len(V)
    bad_vert = V.copy()
    bad_vert[7, 2] = np.nan
    with pkg.MeshIndex(V, T, device=0) as ix:
        calls = [
            lambda: lib.r2s_mesh_index_intersections(None, ph, pp, 64, pt),
            lambda: lib.r2s_mesh_index_intersections(ix._handle(), ph, pp, 64, None),
            lambda: lib.r2s_mesh_index_intersections(ix._handle(), ph, pp, -1, pt),
            lambda: lib.r2s_mesh_index_intersections(ix._handle(), ph, None, 64, pt),
            lambda: lib.r2s_mesh_intersections(None, len(V), ptr, n, 0, ph, pp, 64, pt),
            lambda: lib.r2s_mesh_intersections(pv, len(V), None, n, 0, ph, pp, 64, pt),
            lambda: lib.r2s_mesh_intersections(pv, -1, ptr, n, 0, ph, pp, 64, pt),
            lambda: lib.r2s_mesh_intersections(pv, len(V), ptr, -1, 0, ph, pp, 64, pt),
            lambda: lib.r2s_mesh_intersections(pv, len(V), ptr, n, 0, ph, pp, 64, None),
            lambda: lib.r2s_mesh_intersections(pv, len(V), bad_index.ctypes.data_as(L.c_int32_p), n, 0, ph, pp, 64, pt),
            lambda: lib.r2s_mesh_intersections(bad_vert.ctypes.data_as(L.c_float_p), len(V), ptr, n, 0, ph, pp, 64, pt),
        ]
        for k, call in enumerate(calls):
            assert call() == -1, k
        assert (h == -7).all() and (p == -7).all() and (t == -7).all()
        dh, dp = _dev(h), _dev(p)
        st = vp(torch.cuda.current_stream().cuda_stream)
        dV, dB = _dev(V), _dev(bad_index)
        dev_calls = [
            lambda: lib.r2s_mesh_index_intersections_dev(None, vp(dh.data_ptr()), vp(dp.data_ptr()), 64, pt, st),
            lambda: lib.r2s_mesh_index_intersections_dev(ix._handle(), vp(dh.data_ptr()), vp(dp.data_ptr()), 64, None, st),
            lambda: lib.r2s_mesh_index_intersections_dev(ix._handle(), vp(dh.data_ptr()), None, 64, pt, st),
            lambda: lib.r2s_mesh_intersections_dev(vp(dV.data_ptr()), len(V), vp(dB.data_ptr()), n, vp(dh.data_ptr()), vp(dp.data_ptr()), 64,
                                                   pt, st),
            lambda: lib.r2s_mesh_intersections_dev(vp(dV.data_ptr()), len(V), None, n, vp(dh.data_ptr()), vp(dp.data_ptr()), 64, pt, st),
        ]
        for k, call in enumerate(dev_calls):
            assert call() == -1, k
        torch.cuda.synchronize()
        assert (dh.cpu().numpy() == -7).all() and (dp.cpu().numpy() == -7).all() and (t == -7).all()
        if torch.cuda.device_count() > 1:                  # the index lives on device 0
            with torch.cuda.device(1):
                d1h = torch.full((n,), -7, dtype=torch.int32, device="cuda:1")
                assert lib.r2s_mesh_index_intersections_dev(ix._handle(), vp(d1h.data_ptr()), None, 0, pt,
                                                            vp(torch.cuda.current_stream().cuda_stream)) == -1
                assert (d1h.cpu().numpy() == -7).all() and (t == -7).all()


def test_import_stl_check_intersections(pkg, tmp_path):
    V, T = C.case("two_cubes")
    path = pkg.export_stl(os.path.join(str(tmp_path), "two_cubes"), V, T)
    v, t, res = pkg.import_stl(path, check_intersections=True)
    plain = pkg.import_stl(path)
    assert len(plain) == 2 and np.array_equal(plain[0], v) and np.array_equal(plain[1], t)
    # the weld keeps the triangle order of the file and merges only equal points: the pairs are those of the case
    assert len(t) == len(T) and np.array_equal(v[t], V[T])
    pairs, hits, tot = C.expected("two_cubes")
    assert np.array_equal(res.pairs, pairs) and np.array_equal(res.hits_of_tri, hits) and np.array_equal(res.totals, tot)
    with pytest.raises(pkg._lib.R2SError):
        pkg.import_stl(path, weld=False, check_intersections=True)
