"""The mesh nesting on the GPU (r2s_mesh_nesting, r2s_mesh_nesting_dev with and without an index, import_stl(orient="nested"))
against the restatement of tests/mesh_nesting_ref.py on every case of tests/mesh_nesting_cases.py under all six rays:
patch_of_tri, every record, the totals, the sorted pair list and the rewound triangles are EQUAL.  Then repeatability, the
capacity protocol, the index left unchanged, the orient's patches, the composition orient -> nesting -> shells / winding, the
STL import and the stream contract of the _dev entry point (the method and helpers of tests/test_mesh_orient_stream_gpu.py)."""
import ctypes

import numpy as np
import pytest

import mesh_nesting_cases as C
import mesh_nesting_ref as R
from test_mesh_nesting_cpu import ARG, ref
from test_mesh_orient_stream_gpu import Case, _dev as _to_dev, _p, _scenario

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p


def _host(m):
    """a MeshNesting of the _dev call with everything on the host"""
    m.tris = None if m.tris is None else m.tris.cpu().numpy()
    m.patch_of_tri, m.pairs = m.patch_of_tri.cpu().numpy(), m.pairs.cpu().numpy()
    return m


def _dev(pkg, V, T, index=None, **kw):
    import torch
    v, t = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(T)).cuda()
    ix = pkg.MeshIndex(v, t) if index else None
    try:
        return _host(pkg.mesh_nesting_dev(v, t, index=ix, **kw))
    finally:
        if ix is not None:
            ix.close()


def _same(a, b):
    return (np.array_equal(a.tris, b.tris) if a.tris is not None else b.tris is None) and np.array_equal(a.patch_of_tri, b.patch_of_tri) \
        and np.array_equal(a.counts, b.counts) and np.array_equal(a.pairs, b.pairs) and np.array_equal(a.totals, b.totals)


def _check(label, m, r, rewind):
    """a result against the restatement r computed with REWIND (without the flag: no reversed bit, no reversed triangles)"""
    counts, totals = r["counts"].copy(), r["totals"].copy()
    if not rewind:
        counts[:, 2] &= ~np.int64(2)
        totals[7] = 0
    assert np.array_equal(m.patch_of_tri, r["patch_of_tri"]) and m.patch_of_tri.dtype == np.int32, label
    assert np.array_equal(m.counts, counts) and m.counts.dtype == np.int64, label
    assert np.array_equal(m.totals, totals), label
    assert np.array_equal(m.pairs, r["pairs"]) and m.pairs.dtype == np.int64, label
    if rewind:
        assert np.array_equal(m.tris, r["tris"]) and m.tris.dtype == np.int32, label
    else:
        assert m.tris is None, label


@pytest.mark.parametrize("name", C.ALL)
def test_equal_to_the_restatement(pkg, name):
    V, T = C.case(name)
    for ray in range(6):
        r = ref(name, ray, R.REWIND)
        label = f"{name} ray {ray}"
        _check(label + " host", pkg.mesh_nesting(V, T, ray=ray, rewind=True), r, True)
        _check(label + " dev", _dev(pkg, V, T, ray=ray, rewind=True), r, True)
        _check(label + " dev index", _dev(pkg, V, T, index=True, ray=ray, rewind=True, capacity=len(r["counts"]) + 3,
                                          pair_capacity=len(r["pairs"]) + 1), r, True)
    r = ref(name, 2, R.REWIND)
    _check(name + " no rewind", pkg.mesh_nesting(V, T), r, False)
    _check(name + " no rewind dev", _dev(pkg, V, T, index=True), r, False)
    with pkg.MeshIndex(V, T) as ix:                   # host arrays and an index on the current device
        _check(name + " host index", pkg.mesh_nesting(V, T, ray=4, rewind=True, index=ix), ref(name, 4, R.REWIND), True)


def test_repeated_calls_and_fresh_work_buffers_give_the_same_bits(pkg):
    for name in ("scatter257", "noise17", "chain70"):
        V, T = C.case(name)
        a = pkg.mesh_nesting(V, T, ray=1, rewind=True)
        assert _same(a, pkg.mesh_nesting(V, T, ray=1, rewind=True)) and _same(a, _dev(pkg, V, T, ray=1, rewind=True))
        pkg._lib.lib().r2s_release_cache()
        assert _same(a, pkg.mesh_nesting(V, T, ray=1, rewind=True)) and _same(a, _dev(pkg, V, T, index=True, ray=1, rewind=True))


def test_what_the_cases_must_show(pkg):
    n = lambda name, **kw: pkg.mesh_nesting(*C.case(name), **kw)   # noqa: E731
    e = n("empty", rewind=True)
    assert e.n_patches == 0 and e.totals.tolist() == [0] * 8 and e.tris.shape == (0, 3) and len(e.pairs) == 0
    assert n("beside", ray=3).counts[1].tolist() == [12, 12, 1, -1, 0, 0, 2, 0]
    c = n("chain70")
    assert c.totals.tolist() == [70, 840, 0, 70, 2415, 69, 0, 0] and c.parent.tolist() == list(range(-1, 69))
    assert c.voids.tolist() == list(range(1, 70, 2)) and c.bodies.tolist() == list(range(0, 70, 2)) and c.roots.tolist() == [0]
    i = n("interpenetrating")
    assert i.irregular.tolist() == [False, False, True] and i.parent.tolist() == [-1, -1, 0] and i.depth.tolist() == [0, 0, 2]
    assert not n("open_container").closed[0] and n("open_container").totals[4] == 0 and n("open_query").depth.tolist() == [0, 1]
    assert n("ico_around").children(0).tolist() == list(range(1, 41))
    # every triangle collapsed: no patch, the triangles copied
    V, T = C.S.all_collapsed()
    a = pkg.mesh_nesting(V, T, rewind=True)
    assert a.totals.tolist() == [0, 4, 4, 0, 0, 0, 0, 0] and (a.patch_of_tri == -1).all() and np.array_equal(a.tris, T)
    assert _same(a, _dev(pkg, V, T, rewind=True))


def test_patches_are_the_orients(pkg):
    for name in ("collapsed_mixed", "shared_edge", "scatter256", "noise17"):
        V, T = C.case(name)
        for Tx in (T, C.reversed_some(T)):
            o, m = pkg.mesh_orient(V, Tx), pkg.mesh_nesting(V, Tx)
            assert np.array_equal(o.patch_of_tri, m.patch_of_tri) and np.array_equal(o.counts[:, :2], m.counts[:, :2])
            assert np.array_equal(o.closed, m.closed) and o.totals[:3].tolist() == m.totals[:3].tolist() and o.totals[5] == m.totals[3]


def test_dev_capacity_too_small_leaves_the_tables_untouched(pkg):
    import torch
    L = pkg._lib
    V, T = C.case("chain3")
    r = ref("chain3", 2, R.REWIND)
    v, t = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    out = torch.full((len(T), 3), -7, dtype=torch.int32, device="cuda")
    pot = torch.full((len(T),), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((3, 8), -7, dtype=torch.int64, device="cuda")
    pairs = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    n, m, tot = ctypes.c_int64(), ctypes.c_int64(), np.zeros(8, np.int64)

    def call(cap, pcap):
        L.check(L.lib().r2s_mesh_nesting_dev(None, vp(v.data_ptr()), len(V), vp(t.data_ptr()), len(T), 2, 1, vp(out.data_ptr()), vp(pot.data_ptr()),
                                             vp(counts.data_ptr()), cap, vp(pairs.data_ptr()), pcap, ctypes.byref(n), ctypes.byref(m),
                                             tot.ctypes.data_as(L.c_int64_p), None))
        assert n.value == 3 and m.value == 3 and np.array_equal(tot, r["totals"])              # the counts always come back
        assert np.array_equal(out.cpu().numpy(), r["tris"]) and np.array_equal(pot.cpu().numpy(), r["patch_of_tri"])
    for cap, pcap in ((0, 0), (2, 2)):
        call(cap, pcap)
        assert (counts == -7).all() and (pairs == -7).all()
    call(3, 2)                                        # room for the records, a short pair list
    assert np.array_equal(counts.cpu().numpy(), r["counts"]) and (pairs == -7).all()
    counts.fill_(-7)
    call(2, 3)                                        # and the other way round
    assert (counts == -7).all() and np.array_equal(pairs.cpu().numpy(), r["pairs"])
    pkg.mesh_nesting(*C.case("tetrahedron"))          # the thread's last result is the host variant's
    call(3, 3)
    L.check(L.lib().r2s_last_mesh_nesting(None, 0, None, 0, ctypes.byref(n), ctypes.byref(m)))
    assert n.value == 1 and m.value == 0


def test_index_is_used_and_left_unchanged(pkg):
    V, T = C.case("hollow21")
    P = np.random.default_rng(3).uniform(V.min(0) - 0.5, V.max(0) + 0.5, (64, 3))
    with pkg.MeshIndex(V, T) as ix:
        info, d = ix.info(), ix.distance(P, want_index=True)
        m = pkg.mesh_nesting(V, T, rewind=True, index=ix)
        _check("hollow21 index", m, ref("hollow21", 2, R.REWIND), True)
        d2 = ix.distance(P, want_index=True)
        assert ix.info() == info and np.array_equal(d[0].view(np.uint64), d2[0].view(np.uint64)) and np.array_equal(d[1], d2[1])
        # an index of another triangle count is refused before any output is touched
        import torch
        L = pkg._lib
        V2, T2 = C.case("nested2")
        v, t = torch.from_numpy(V2).cuda(), torch.from_numpy(T2).cuda()
        pot = torch.full((len(T2),), -7, dtype=torch.int32, device="cuda")
        n, k, tot = ctypes.c_int64(-7), ctypes.c_int64(-7), np.full(8, -7, np.int64)
        rc = L.lib().r2s_mesh_nesting_dev(ix._handle(), vp(v.data_ptr()), len(V2), vp(t.data_ptr()), len(T2), 2, 0, None, vp(pot.data_ptr()), None, 0,
                                          None, 0, ctypes.byref(n), ctypes.byref(k), tot.ctypes.data_as(L.c_int64_p), None)
        assert rc == ARG and "index" in L.lib().r2s_last_error().decode()
        assert (pot == -7).all() and n.value == -7 and k.value == -7 and (tot == -7).all()


def _scrambled(T, seed):
    """T under a seeded permutation with 30 % of the triangles reversed"""
    rng = np.random.default_rng(seed)
    Ts = np.ascontiguousarray(T[rng.permutation(len(T))])
    sel = rng.random(len(Ts)) < 0.3
    Ts[sel] = Ts[sel][:, ::-1]
    return Ts


@pytest.mark.parametrize("name,void_point,wall_point", [("nested2", (1.5, 2.0, 1.75), (0.5, 0.5, 0.5)),
                                                         ("hollow21", (1.5, 3.0, 2.75), (0.0, 3.0, 2.75))])
def test_composition_with_orient_shells_and_winding(pkg, name, void_point, wall_point):
    V, T = C.case(name)
    Ts = _scrambled(T, 12)
    o = pkg.mesh_orient(V, Ts, outward=True)
    m = pkg.mesh_nesting(V, o.tris, rewind=True)
    assert m.depth.tolist() in ([0, 1], [1, 0]) and m.closed.all() and m.totals[7] == m.n_tris[m.depth == 1].sum()
    s = pkg.mesh_shells(V, m.tris)
    assert s.n_shells == 2 and s.totals[5] == 0
    for p in range(2):                                # positive at even depth, negative at odd depth
        vol = s.volume[s.shell_of_tri[m.first_tri[p]]]
        assert (vol > 0) if m.depth[p] % 2 == 0 else (vol < 0), (p, vol)
    with pkg.MeshIndex(V, m.tris) as ix:
        assert ix.contains(np.array([void_point, wall_point]), rule="positive").tolist() == [False, True]
    with pkg.MeshIndex(V, o.tris) as ix:              # the outward orient alone fills the void: the caveat this tool answers
        assert ix.contains(np.array([void_point]), rule="positive").tolist() == [True]
    # the two steps again return the same triangles
    o2 = pkg.mesh_orient(V, m.tris, outward=True)
    assert np.array_equal(pkg.mesh_nesting(V, o2.tris, rewind=True).tris, m.tris)


def test_import_stl_orient_nested(pkg, tmp_path):
    V, T = C.case("hollow21")
    want = pkg.mesh_nesting(V, pkg.mesh_orient(V, T, outward=True).tris, rewind=True).tris
    sw = pkg.mesh_shells(V, want)
    assert sorted(np.sign(sw.volume).tolist()) == [-1.0, 1.0]
    path = pkg.export_stl(str(tmp_path / "hollow"), V, _scrambled(T, 5))
    Vn, Tn = pkg.import_stl(path, orient="nested")
    Vo, To = pkg.import_stl(path, orient="outward")
    assert np.array_equal(Vn.view(np.uint32), Vo.view(np.uint32)) and np.array_equal(np.sort(Tn, 1), np.sort(To, 1))
    assert (pkg.mesh_shells(Vo, To).volume > 0).all()                                   # outward alone: the void has become a body
    got = pkg.mesh_shells(Vn, Tn)
    assert got.n_shells == 2 and got.closed.all() and got.totals[5] == 0
    # the same mesh as the exported body, oriented: the same two signed volumes and areas
    for a, b in ((np.sort(got.volume), np.sort(sw.volume)), (np.sort(got.area), np.sort(sw.area))):
        assert np.allclose(a, b, rtol=1e-9, atol=0.0)
    with pkg.MeshIndex(Vn, Tn) as ix:
        assert ix.contains(np.array([(1.5, 3.0, 2.75), (0.0, 3.0, 2.75)]), rule="positive").tolist() == [False, True]


# ---- the stream contract of the _dev entry point ------------------------------------------------------------------------------

_cache = {}


def _nesting_case(pkg):
    if "case" not in _cache:
        import torch
        L, lib = pkg._lib, pkg._lib.lib()
        (V, T), (DV, DT) = C.case("siblings"), C.case("chain3")            # the same counts, another forest
        nv, nt = len(V), len(T)
        assert (nv, nt) == (len(DV), len(DT))
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda:0")   # noqa: E731

        def nesting(b, outs, st):
            n, m, tot = ctypes.c_int64(-7), ctypes.c_int64(-7), np.full(8, -7, np.int64)
            L.check(lib.r2s_mesh_nesting_dev(None, _p(b[0]), nv, _p(b[1]), nt, 2, 1, _p(outs[0]), _p(outs[1]), _p(outs[2]), 4, _p(outs[3]), 4,
                                             ctypes.byref(n), ctypes.byref(m), tot.ctypes.data_as(L.c_int64_p), vp(st.cuda_stream)))
            return (n.value, m.value, tot.tobytes())

        _cache["case"] = Case("r2s_mesh_nesting_dev", [_to_dev(V), _to_dev(T)], [_to_dev(DV), _to_dev(DT)],
                              lambda: [e((nt, 3), torch.int32), e(nt, torch.int32), e((4, 8), torch.int64), e(4, torch.int64)], nesting)
    return _cache["case"]


@pytest.mark.parametrize("busy_null", [False, True], ids=["L", "N"])
def test_mesh_nesting_late_producer(pkg, busy_null):
    case = _nesting_case(pkg)
    _scenario(case, busy_null)
    exp = case.expected
    r = ref("siblings", 2, R.REWIND)
    assert exp["real"][1] != exp["decoy"][1] and exp["real"][1][:2] == (3, 2)
    assert np.array_equal(exp["real"][0][0], r["tris"]) and np.array_equal(exp["real"][0][2][:3], r["counts"])
