"""The mesh fans on the GPU (r2s_mesh_fans, r2s_mesh_fans_dev, import_stl(split_vertices=True)) against the restatement of
tests/mesh_fans_ref.py on every case of tests/mesh_fans_cases.py and its variants: fan_of_corner, fans_of_vert, every record, the
totals, the split triangles and vert_of EQUAL, the split vertices bit for bit.  All of it is integer or copied bits: there is no
tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

import mesh_fans_cases as C
from test_mesh_fans_cpu import ARG, TOO_MANY_TRIS, UNSUPPORTED, follows_permutation, ref

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """two results bit for bit"""
    return (np.array_equal(a.fan_of_corner, b.fan_of_corner) and np.array_equal(a.fans_of_vert, b.fans_of_vert)
            and np.array_equal(a.counts, b.counts) and np.array_equal(a.totals, b.totals) and np.array_equal(a.tris, b.tris)
            and np.array_equal(a.vert_of, b.vert_of) and a.verts.shape == b.verts.shape and np.array_equal(_bits(a.verts), _bits(b.verts)))


def _dev(pkg, V, T, capacity=0):
    import torch
    v, t = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(T)).cuda()
    o = pkg.mesh_fans_dev(v, t, split=True, capacity=capacity)
    for k in ("fan_of_corner", "fans_of_vert", "verts", "tris", "vert_of"):
        setattr(o, k, getattr(o, k).cpu().numpy())
    return o


def _check(label, o, r, nv):
    assert np.array_equal(o.fan_of_corner, r["fan_of_corner"]) and o.fan_of_corner.dtype == np.int32, label
    assert np.array_equal(o.fans_of_vert, r["fans_of_vert"]) and o.fans_of_vert.dtype == np.int32, label
    assert np.array_equal(o.counts, r["counts"]) and np.array_equal(o.totals, r["totals"]), label
    assert o.n_fans == len(r["counts"]) and o.n_added == r["n_added"] and o.n_verts_out == nv + r["n_added"], label
    assert np.array_equal(o.tris, r["tris"]) and o.tris.dtype == np.int32 and np.array_equal(o.vert_of, r["vert_of"]), label
    assert o.verts.shape == r["verts"].shape and np.array_equal(_bits(o.verts), _bits(r["verts"])), label


@pytest.mark.parametrize("name,variant", C.variants())
def test_equal_to_the_restatement(pkg, name, variant):
    V, T = C.case(name, variant)
    r = ref(name, variant)
    label = f"{name} {variant}"
    o = pkg.mesh_fans(V, T, split=True)
    _check(label, o, r, len(V))
    print(f"FANS {label}: {len(T)} triangles, {o.n_fans} fans, totals {o.totals.tolist()}")
    # the host variant, the _dev variant (asking for the records, and with room for them) and a second call: bit for bit
    assert _same(o, _dev(pkg, V, T)), label
    assert _same(o, _dev(pkg, V, T, capacity=o.n_fans + 3)), label
    assert _same(o, pkg.mesh_fans(V, T, split=True)), label
    # without the split: the same analysis, no mesh
    p = pkg.mesh_fans(V, T)
    assert p.verts is None and p.tris is None and np.array_equal(p.counts, o.counts) and np.array_equal(p.fan_of_corner, o.fan_of_corner)
    assert np.array_equal(o.pinched, np.nonzero(r["fans_of_vert"] >= 2)[0])
    assert o.vertex_manifold == (r["totals"][5] == 0 and r["totals"][6] == 0)


def test_fresh_work_buffers_give_the_same_bits(pkg):
    V, T = C.case("welded_lattice_touch")
    a = pkg.mesh_fans(V, T, split=True)
    pkg._lib.lib().r2s_release_cache()
    assert _same(a, pkg.mesh_fans(V, T, split=True)) and _same(a, _dev(pkg, V, T))
    _check("after release", a, ref("welded_lattice_touch"), len(V))


@pytest.mark.parametrize("name", ["two_tets_sharing_vertex", "pinched_sphere", "apex300", "cubes_sharing_edge", "collapsed_mixed",
                                  "welded_lattice_touch", "noise24_open"])
def test_shells_of_the_split_mesh_and_idempotence(pkg, name):
    V, T = C.case(name)
    o = pkg.mesh_fans(V, T, split=True)
    a, b = pkg.mesh_shells(V, T), pkg.mesh_shells(o.verts, o.tris)
    assert np.array_equal(a.shell_of_tri, b.shell_of_tri) and np.array_equal(a.counts[:, [0, 1, 3, 4, 5, 6]], b.counts[:, [0, 1, 3, 4, 5, 6]])
    assert np.array_equal(a.totals[:7], b.totals[:7]) and b.totals[7] - a.totals[7] == o.n_added
    assert np.array_equal(a.ref_point.view(np.uint64), b.ref_point.view(np.uint64))
    assert np.array_equal(a.sums.view(np.uint64), b.sums.view(np.uint64))
    shell_of_fan = a.shell_of_tri[o.first_corner // 3]
    assert np.array_equal(b.n_verts, np.bincount(shell_of_fan, minlength=a.n_shells))
    if name == "pinched_sphere":                       # one shell touching itself: the Euler characteristic rises by 1
        assert a.n_shells == 1 and a.closed[0] and (a.euler[0], b.euler[0]) == (1, 2) and b.genus[0] == 0
    again = pkg.mesh_fans(o.verts, o.tris, split=True)
    assert again.fans_of_vert.max() <= 1 and again.n_added == 0 and len(again.pinched) == 0
    assert np.array_equal(again.tris, o.tris) and np.array_equal(_bits(again.verts), _bits(o.verts))
    assert again.totals[6] == o.totals[6]              # complex fans are not repaired


@pytest.mark.parametrize("name", ["cone5000", "tets40", "disk_and_cone"])
def test_permutation_of_the_triangles(pkg, name):
    res = lambda o: dict(fan_of_corner=o.fan_of_corner, counts=o.counts, totals=o.totals, fans_of_vert=o.fans_of_vert)   # noqa: E731
    a, p = pkg.mesh_fans(*C.case(name)), pkg.mesh_fans(*C.case(name, "permuted"))
    assert follows_permutation(res(a), res(p), C.perm_of(name))


def test_import_stl_split_vertices(pkg, tmp_path):
    V, T = C.case("pinched_sphere")
    path = pkg.export_stl(str(tmp_path / "pinched"), V, T)
    Vk, Tk = pkg.import_stl(path)                                                     # the weld brings the pinched vertex back
    kept = pkg.mesh_fans(Vk, Tk)
    assert len(Vk) == 9 and kept.totals[5] == 1 and not kept.vertex_manifold
    for orient in (None, "outward"):
        Vs, Ts = pkg.import_stl(path, split_vertices=True, orient=orient)
        got = pkg.mesh_fans(Vs, Ts)
        assert len(Vs) == 10 and got.vertex_manifold and got.totals[0] == 10 and np.array_equal(_bits(Vs[:9]), _bits(Vk))
        s = pkg.mesh_shells(Vs, Ts)
        assert s.n_shells == 1 and s.closed[0] and s.euler[0] == 2
    with pytest.raises(pkg._lib.R2SError):
        pkg.import_stl(path, split_vertices=True, weld=False)


# ---- refusals and capacities -------------------------------------------------------------------------------------------------

def _raw(pkg, V, T, nv=None, nt=None, dev=False, null=(), vcap=None, fcap=8, alias=None):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs; `null`: the arguments passed as NULL; alias: the output
    that is given the address of the input triangles"""
    import torch
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    vcap = len(v) + 8 if vcap is None else vcap
    n, nvo, tot = ctypes.c_int64(-7), ctypes.c_int64(-7), np.full(8, -7, np.int64)
    tail = [None if "n" in null else ctypes.byref(n), None if "nvo" in null else ctypes.byref(nvo),
            None if "tot" in null else tot.ctypes.data_as(L.c_int64_p)]
    shapes = dict(foc=((len(t), 3), np.int32), fov=((len(v),), np.int32), to=((len(t), 3), np.int32), vo=((len(v) + 8, 3), np.float32),
                  vof=((len(v) + 8,), np.int32), cnt=((8, 8), np.int64))
    if dev:
        arr = dict(verts=torch.from_numpy(v).cuda(), tris=torch.from_numpy(t).cuda())
        for k, (shape, dt) in shapes.items():
            arr[k] = torch.full(shape, -7, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        p = lambda k: None if k in null else ctypes.c_void_p(arr["tris" if k == alias else k].data_ptr())   # noqa: E731
        rc = L.lib().r2s_mesh_fans_dev(p("verts"), nv, p("tris"), nt, p("foc"), p("fov"), p("cnt"), fcap, p("to"), p("vo"), p("vof"), vcap,
                                       *tail, None)
        torch.cuda.synchronize()
        outs = [arr[k].cpu().numpy() for k in shapes]
        t_after = arr["tris"].cpu().numpy()
    else:
        arr = dict(verts=v, tris=t)
        for k, (shape, dt) in shapes.items():
            arr[k] = np.full(shape, -7, dt)
        q = lambda k: arr["tris" if k == alias else k]   # noqa: E731
        ip = lambda k: None if k in null else q(k).ctypes.data_as(L.c_int32_p)   # noqa: E731
        fp = lambda k: None if k in null else q(k).ctypes.data_as(L.c_float_p)   # noqa: E731
        rc = L.lib().r2s_mesh_fans(fp("verts"), nv, ip("tris"), nt, -1, ip("foc"), ip("fov"), ip("to"), fp("vo"), ip("vof"), vcap, *tail)
        outs = [arr[k] for k in shapes if k != "cnt"]
        t_after = t
    clean = all((x == -7).all() for x in outs) and n.value == -7 and nvo.value == -7 and (tot == -7).all()
    return rc, bool(clean) and np.array_equal(t_after, np.ascontiguousarray(T, np.int32).reshape(-1, 3))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_leave_the_outputs_untouched(pkg, dev):
    V, T = C.case("two_tets_sharing_vertex")
    T_big, T_neg, V_nan, V_inf = T.copy(), T.copy(), V.copy(), V.copy()
    T_big[5, 2], T_neg[0, 0], V_nan[3, 1], V_inf[6, 2] = len(V), -1, np.nan, -np.inf
    for Vx, Tx in ((V, T_big), (V, T_neg), (V_nan, T), (V_inf, T)):                 # an out-of-range index, a non-finite vertex
        assert _raw(pkg, Vx, Tx, dev=dev) == (ARG, True)
    for null in (("verts",), ("tris",), ("n",), ("nvo",), ("tot",)):                # NULL arrays with a count, NULL scalar outputs
        assert _raw(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    for null in (("vo",), ("vof",), ("vo", "vof"), ("to",)):                        # tris_out without verts_out / vert_of_out, and back
        assert _raw(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    for alias in ("foc", "to"):                                                      # an output overlapping an input
        assert _raw(pkg, V, T, dev=dev, alias=alias) == (ARG, True), alias
    if dev:
        for kw in (dict(null=("cnt",)), dict(fcap=-1)):                             # NULL records with a capacity, a negative capacity
            assert _raw(pkg, V, T, dev=True, **kw) == (ARG, True), kw
    assert _raw(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _raw(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    assert _raw(pkg, V, T, vcap=-1, dev=dev) == (ARG, True)
    # 3 * n_tris >= 2^31 as a fake count on the tiny buffer: refused before anything is read; n_verts beyond 32 bits likewise
    assert _raw(pkg, V, T, nt=TOO_MANY_TRIS, dev=dev) == (UNSUPPORTED, True)
    assert _raw(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    assert _raw(pkg, V, T, dev=dev)[0] == 0                                          # (and the same call goes through unharmed)


def test_capacities_of_both_tables(pkg):
    import torch
    L = pkg._lib
    V, T = C.case("two_tets_sharing_vertex")                                         # 8 fans, 7 + 1 vertices
    r = ref("two_tets_sharing_vertex")
    v, t = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    full = lambda shape, dt: torch.full(shape, -7, dtype=dt, device="cuda")   # noqa: E731
    foc, fov, cnt = full((8, 3), torch.int32), full((7,), torch.int32), full((9, 8), torch.int64)
    to, vo, vof = full((8, 3), torch.int32), full((9, 3), torch.float32), full((9,), torch.int32)
    n, nvo, tot = ctypes.c_int64(), ctypes.c_int64(), np.zeros(8, np.int64)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731

    def call(fcap, vcap):
        L.check(L.lib().r2s_mesh_fans_dev(vp(v), 7, vp(t), 8, vp(foc), vp(fov), vp(cnt), fcap, vp(to), vp(vo), vp(vof), vcap, ctypes.byref(n),
                                          ctypes.byref(nvo), tot.ctypes.data_as(L.c_int64_p), None))
        assert (n.value, nvo.value) == (8, 8) and tot.tolist() == [8, 8, 0, 7, 0, 1, 0, 0]      # the counts are always returned
        assert np.array_equal(foc.cpu().numpy(), r["fan_of_corner"]) and np.array_equal(fov.cpu().numpy(), r["fans_of_vert"])

    for fcap, vcap in ((0, 0), (7, 7)):                                              # one short each: both tables stay untouched
        call(fcap, vcap)
        assert (cnt == -7).all() and (to == -7).all() and (vo == -7).all() and (vof == -7).all()
    call(8, 7)                                                                       # room for the records only
    assert np.array_equal(cnt.cpu().numpy()[:8], r["counts"]) and (cnt[8:] == -7).all() and (to == -7).all() and (vo == -7).all()
    cnt.fill_(-7)
    call(7, 9)                                                                       # room for the split only
    assert (cnt == -7).all() and np.array_equal(to.cpu().numpy(), r["tris"]) and np.array_equal(vof.cpu().numpy()[:8], r["vert_of"])
    assert np.array_equal(_bits(vo.cpu().numpy()[:8]), _bits(r["verts"])) and (vof[8:] == -7).all() and (vo[8:] == -7).all()
    # the host variant: the split only into room for it; its records are the thread's last result, which _dev leaves alone
    out = np.full((8, 3), -7, np.int32), np.full((9, 3), -7, np.float32), np.full(9, -7, np.int32)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
    for vcap in (7, 8):
        L.check(L.lib().r2s_mesh_fans(V.ctypes.data_as(L.c_float_p), 7, ip(T), 8, -1, None, None, ip(out[0]), out[1].ctypes.data_as(L.c_float_p),
                                      ip(out[2]), vcap, ctypes.byref(n), ctypes.byref(nvo), tot.ctypes.data_as(L.c_int64_p)))
        assert (n.value, nvo.value) == (8, 8)
        if vcap == 7:
            assert all((x == -7).all() for x in out)
    assert np.array_equal(out[0], r["tris"]) and np.array_equal(out[2][:8], r["vert_of"]) and (out[2][8:] == -7).all()
    pkg.mesh_fans(*C.case("bowtie"))
    call(8, 8)
    m, rec = ctypes.c_int64(), np.full((8, 8), -7, np.int64)
    L.check(L.lib().r2s_last_mesh_fans(rec.ctypes.data_as(L.c_int64_p), 2, ctypes.byref(m)))
    assert m.value == 6 and np.array_equal(rec[:2], ref("bowtie")["counts"][:2]) and (rec[2:] == -7).all()


def test_no_triangles_copies_the_vertices(pkg):
    V = C.case("tetrahedron")[0]
    o = pkg.mesh_fans(V, np.zeros((0, 3), np.int32), split=True)
    assert o.n_fans == 0 and o.totals.tolist() == [0, 0, 0, 0, 4, 0, 0, 0] and (o.fans_of_vert == 0).all()
    assert np.array_equal(_bits(o.verts), _bits(V)) and o.vert_of.tolist() == [0, 1, 2, 3] and o.tris.shape == (0, 3)
    d = _dev(pkg, V, np.zeros((0, 3), np.int32))
    assert _same(o, d)
