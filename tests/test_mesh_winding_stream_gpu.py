"""The stream contract of the winding and signed-distance _dev entry points (include/rho2sdf_hip.h, "Streams"), by the method and
with the helpers of tests/test_mesh_intersect_stream_gpu.py (that file's docstring explains them): the call is made on a
non-blocking stream whose input buffers still hold a decoy while a delay and the copy of the real input are queued in front of it
(L), also with a busy null stream (N), and must give the plain call's bits, which differ from the decoy's.  The index entries get
late POINTS (the index is built beforehand: it copies the mesh); r2s_mesh_signed_distance_dev gets a late MESH.  The lattice entries
of an index read no device input: they are checked to run on the caller's stream behind a delay and to equal the plain result."""
import ctypes

import numpy as np
import pytest

import mesh_winding_cases as C
from test_mesh_intersect_stream_gpu import Case, _delay, _dev, _p, _same, _scenario

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
_cases = {}


def _build(pkg):
    if _cases:
        return _cases
    import torch
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("octahedra")
    P = np.ascontiguousarray(C.points("octahedra")[:-3][::7])
    D = np.ascontiguousarray(P[::-1] * 0.5)                                 # the decoy points: other windings, other distances
    n = len(P)
    ix = pkg.MeshIndex(V, T, device=0)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")   # noqa: E731

    def winding(b, outs, st):
        L.check(lib.r2s_mesh_index_winding_dev(ix._handle(), _p(b[0]), 0, n, 4, _p(outs[0]), _p(outs[1]), vp(st.cuda_stream)))
        return ()

    def signed(b, outs, st):
        L.check(lib.r2s_mesh_index_signed_dev(ix._handle(), _p(b[0]), 0, n, 0, 1, 0, _p(outs[0]), _p(outs[1]), vp(st.cuda_stream)))
        return ()

    dims, origin, h = C.lattice("octahedra")
    cd, co = (ctypes.c_int64 * 3)(*dims), (ctypes.c_double * 3)(*origin)
    nlat = int(np.prod(dims))
    DV = (V * np.float32(0.75)).astype(np.float32)                          # the decoy mesh: the same triangles, scaled

    def mesh_signed(b, outs, st):
        L.check(lib.r2s_mesh_signed_distance_dev(_p(b[0]), len(V), _p(b[1]), len(T), cd, co, h, 0, 2, 0, _p(outs[0]), vp(st.cuda_stream)))
        return ()

    _cases["winding"] = Case("r2s_mesh_index_winding_dev", [_dev(P)], [_dev(D)], lambda: [e(n, torch.int32), e(n, torch.int32)], winding,
                             keep=ix)
    _cases["signed"] = Case("r2s_mesh_index_signed_dev", [_dev(P)], [_dev(D)], lambda: [e(n, torch.float64), e(n, torch.int32)], signed,
                            keep=ix)
    _cases["mesh_signed"] = Case("r2s_mesh_signed_distance_dev", [_dev(V), _dev(T)], [_dev(DV), _dev(T)],
                                 lambda: [e(nlat, torch.float64)], mesh_signed)
    _cases["ix"] = ix
    return _cases


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
@pytest.mark.parametrize("entry", ["winding", "signed", "mesh_signed"])
def test_late_producer(pkg, entry, busy_null):
    _scenario(_build(pkg)[entry], busy_null)


def test_lattice_entries_run_on_the_callers_stream(pkg):
    """winding_lattice_dev and signed_lattice_dev queued behind a delay on a non-blocking stream: not done when the call returns
    (they do not wait), done after the stream is, and equal to the plain results"""
    import torch
    ix = _build(pkg)["ix"]
    lat = C.lattice("octahedra")
    w0, c0 = ix.winding_lattice_dev(lat, ray=1, want_crossings=True)
    s0 = ix.signed_lattice_dev(lat, ray=1)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        _delay(30.0)
        w1, c1 = ix.winding_lattice_dev(lat, ray=1, want_crossings=True, stream=S)
        s1 = ix.signed_lattice_dev(lat, ray=1, stream=S)
        done = torch.cuda.Event()
        done.record(S)
        pending = not done.query()
    S.synchronize()
    assert pending, "the delay had finished before the calls returned - the scenario proves nothing"
    assert _same(w1.cpu().numpy(), w0.cpu().numpy()) and _same(c1.cpu().numpy(), c0.cpu().numpy()) and _same(s1.cpu().numpy(), s0.cpu().numpy())
