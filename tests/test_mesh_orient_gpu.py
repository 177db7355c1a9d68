"""The mesh orient on the GPU (r2s_mesh_orient, r2s_mesh_orient_dev, import_stl(orient=...)) against the restatement of
tests/mesh_orient_ref.py on every case of tests/mesh_orient_cases.py, plain and scrambled, with flags 0 and OUTWARD: tris_out,
flip, patch_of_tri, every integer record and the totals exactly, the volume within

    bound(p) = (n_tris(p) + 9) * 2^-53 * T(p)

(tests/test_mesh_orient_cpu.py shows that no volume decision of these cases lies within that bound of zero, so the flips are
decidable).  Each run prints the largest fraction of the bound used as an "ORIENT ..." line."""
import ctypes

import numpy as np
import pytest

import mesh_orient_cases as C
import mesh_orient_ref as R
from test_mesh_orient_cpu import ARG, UNSUPPORTED, analysis

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    """two results bit for bit"""
    return (np.array_equal(np.asarray(a.tris), np.asarray(b.tris)) and np.array_equal(np.asarray(a.flipped), np.asarray(b.flipped))
            and np.array_equal(np.asarray(a.patch_of_tri), np.asarray(b.patch_of_tri)) and np.array_equal(a.counts, b.counts)
            and np.array_equal(_bits(a.volume), _bits(b.volume)) and np.array_equal(a.totals, b.totals)
            and np.array_equal(_bits(a.ref_point), _bits(b.ref_point)))


def _dev(pkg, V, T, outward, capacity=0):
    import torch
    v, t = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(T)).cuda()
    o = pkg.mesh_orient_dev(v, t, outward=outward, capacity=capacity)
    o.tris, o.flipped, o.patch_of_tri = o.tris.cpu().numpy(), o.flipped.cpu().numpy(), o.patch_of_tri.cpu().numpy()
    return o


def _check(label, o, r):
    assert np.array_equal(o.tris, r["tris"]) and o.tris.dtype == np.int32, label
    assert np.array_equal(o.flipped, r["flip"] == 1), label
    assert np.array_equal(o.patch_of_tri, r["patch_of_tri"]), label
    assert np.array_equal(o.counts, r["counts"]), label
    assert np.array_equal(o.totals, r["totals"]), label
    assert np.array_equal(_bits(o.ref_point), _bits(r["ref_point"])), label
    err, b = np.abs(o.volume - r["volume"]), r["bound"]
    frac = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"ORIENT {label}: {len(o.tris)} triangles, {o.n_patches} patches, {int(o.totals[3])} flipped, "
          f"largest fraction of the bound {frac:.4f}")
    assert (err <= b).all(), (label, frac)


@pytest.mark.parametrize("name", C.ALL)
def test_equal_to_the_restatement(pkg, name):
    for scrambled in (False, True):
        V, T = C.case(name, scrambled)
        a = analysis(name, scrambled)
        for flags in (0, R.OUTWARD):
            label = f"{name}{' scrambled' if scrambled else ''} flags {flags}"
            r = R.decide(a, flags)
            o = pkg.mesh_orient(V, T, outward=bool(flags))
            _check(label, o, r)
            # the host variant, the _dev variant (asking for the tables, and with room for them) and a second call: bit for bit
            assert _same(o, _dev(pkg, V, T, bool(flags))), label
            assert _same(o, _dev(pkg, V, T, bool(flags), capacity=o.n_patches + 3)), label
            assert _same(o, pkg.mesh_orient(V, T, outward=bool(flags))), label
            # the flipped edges left in the output are the ones the shells count on the output mesh
            assert o.totals[7] == pkg.mesh_shells(V, o.tris).totals[5], label
            assert np.array_equal(o.closed, (r["counts"][:, 3] & 1) != 0) and np.array_equal(o.by_volume, (r["counts"][:, 3] & 4) != 0)
            assert np.array_equal(o.orientable, ~a["nonorientable"])


def test_fresh_work_buffers_give_the_same_bits(pkg):
    V, T = C.case("nested41", True)
    a = pkg.mesh_orient(V, T, outward=True)
    pkg._lib.lib().r2s_release_cache()
    assert _same(a, pkg.mesh_orient(V, T, outward=True)) and _same(a, _dev(pkg, V, T, True))


def test_what_the_cases_must_show(pkg):
    o = lambda name, outward=False, s=False: pkg.mesh_orient(*C.case(name, s), outward=outward)   # noqa: E731
    e = o("empty")
    assert e.n_patches == 0 and e.totals.tolist() == [0] * 8 and e.tris.shape == (0, 3) and (e.ref_point == 0).all()
    c = o("all_collapsed", True)
    assert c.totals.tolist() == [0, 4, 4, 0, 0, 0, 0, 0] and (c.patch_of_tri == -1).all() and np.array_equal(c.tris, C.case("all_collapsed")[1])
    for name, maj, out in (("tetrahedron", 0, 0), ("tetrahedron_reversed", 0, 4), ("tetrahedron_one_reversed", 1, 1)):
        assert o(name).totals[3] == maj and o(name, True).totals[3] == out, name
    assert o("tetrahedron_reversed", True).volume.tolist() == [36000.0] and o("tetrahedron_reversed").volume.tolist() == [-36000.0]
    # majority leaves the void inward; OUTWARD ignores nesting and turns it into a body (the documented caveat)
    V, T = C.case("cube_with_void")
    m, w = o("cube_with_void"), o("cube_with_void", True)
    assert not m.flipped.any() and m.volume.tolist() == [8.0, -1.0] and not m.by_volume.any()
    assert w.flipped.tolist() == [False] * 12 + [True] * 12 and w.volume.tolist() == [8.0, 1.0] and w.by_volume.all()
    assert pkg.mesh_shells(V, w.tris).is_void.tolist() == [False, False] and pkg.mesh_shells(V, m.tris).is_void.tolist() == [False, True]
    assert np.array_equal(pkg.flip_patches(w.tris, w.patch_of_tri, [1]), T)
    assert o("two_same_direction").flipped.tolist() == [False, True]
    t = o("triangle_twice", True)
    assert t.counts.tolist() == [[0, 2, 1, 1, 0, 0, 3, 0]] and t.volume.tolist() == [0.0] and t.flipped.tolist() == [False, True]
    assert o("three_on_edge").n_patches == 3 and (o("fans40").n_tris == np.arange(1, 41)).all()
    q = o("two_cubes_sharing_edge", True)
    assert q.n_patches == 2 and not q.closed.any() and q.counts[:, 5].tolist() == [2, 2]
    mo = o("moebius", True)
    assert mo.totals[4] == 1 and not mo.orientable[0] and np.array_equal(mo.tris, C.case("moebius")[1]) and not mo.flipped.any()
    assert mo.totals[7] == pkg.mesh_shells(*C.case("moebius")).totals[5] >= 1
    mt = o("moebius_and_tetrahedron", True, True)
    assert mt.orientable.tolist() == [False, True] and mt.by_volume.tolist() == [False, True] and mt.volume[1] > 0
    assert o("ribbon_alternating").counts[0, 1:3].tolist() == [3000, 1500] and o("disjoint").n_patches == 3000
    assert o("torus", True, True).counts[0].tolist()[:2] == [0, 20000]


@pytest.mark.parametrize("name", ["sphere33", "torus", "nested41"])
def test_scrambled_round_trip(pkg, name):
    V, plain = C.case(name)
    _, T = C.case(name, True)
    assert (T != plain).any(1).sum() > 0.25 * len(T)
    assert np.array_equal(pkg.mesh_orient(V, T).tris, plain)                        # majority
    out = pkg.mesh_orient(V, T, outward=True)
    if name == "nested41":                                                           # exactly the negative-volume patches reversed
        ref = pkg.mesh_orient(V, plain)
        assert (np.sign(ref.volume) == [1, -1, 1]).all() and not ref.flipped.any()
        assert np.array_equal(out.tris, pkg.flip_patches(plain, ref.patch_of_tri, ref.volume < 0)) and (out.volume > 0).all()
    else:
        assert np.array_equal(out.tris, plain) and out.volume[0] > 0 and out.by_volume.all()


@pytest.mark.parametrize("name", C.TIE_FREE)
def test_permutation_of_the_triangles(pkg, name):
    for scrambled in (False, True):
        V, T = C.case(name, scrambled)
        (_, Tp), perm = C.S.permuted((V, T), 33)
        for outward in (False, True):
            a, p = pkg.mesh_orient(V, T, outward=outward), pkg.mesh_orient(V, Tp, outward=outward)
            assert np.array_equal(p.flipped, a.flipped[perm]) and np.array_equal(p.tris, a.tris[perm])
            to_a = a.patch_of_tri[perm[p.first_tri]]            # patch k of the permuted mesh is patch to_a[k] of the original
            assert len(np.unique(to_a)) == a.n_patches and np.array_equal(to_a[p.patch_of_tri], a.patch_of_tri[perm])
            assert np.array_equal(p.counts[:, 1:], a.counts[to_a, 1:]) and np.array_equal(p.totals, a.totals)
            b = 2.0 * analysis(name, scrambled)["bound"][to_a]
            assert (np.abs(p.volume - a.volume[to_a]) <= b).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def _raw(pkg, V, T, flags=0, nv=None, nt=None, dev=False, null=()):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs; `null`: the arguments passed as NULL"""
    import torch
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    n, ref, tot = ctypes.c_int64(-7), np.full(3, -7.0), np.full(8, -7, np.int64)
    scal = dict(n=ctypes.byref(n), ref=ref.ctypes.data_as(L.c_double_p), tot=tot.ctypes.data_as(L.c_int64_p))
    tail = [None if k in null else scal[k] for k in ("n", "ref", "tot")]
    if dev:
        vp = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
        dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        full = lambda shape, dt_: torch.full(shape, -7, dtype=dt_, device="cuda")   # noqa: E731
        out, flip, pot = full((len(t), 3), torch.int32), full((len(t),), torch.int32), full((len(t),), torch.int32)
        counts, vol = full((8, 8), torch.int64), full((8,), torch.float64)
        rc = L.lib().r2s_mesh_orient_dev(None if "verts" in null else vp(dv), nv, None if "tris" in null else vp(dt), nt, flags,
                                         None if "out" in null else vp(out), vp(flip), vp(pot), None if "counts" in null else vp(counts),
                                         None if "vol" in null else vp(vol), -1 if "capacity" in null else 8, *tail, None)
        torch.cuda.synchronize()
        arrays = [x.cpu().numpy() for x in (out, flip, pot, counts, vol)]
    else:
        ip = lambda x: x.ctypes.data_as(L.c_int32_p)   # noqa: E731
        out, flip, pot = np.full((len(t), 3), -7, np.int32), np.full(len(t), -7, np.int32), np.full(len(t), -7, np.int32)
        rc = L.lib().r2s_mesh_orient(None if "verts" in null else v.ctypes.data_as(L.c_float_p), nv, None if "tris" in null else ip(t), nt,
                                     flags, -1, None if "out" in null else ip(out), ip(flip), ip(pot), *tail)
        arrays = [out, flip, pot]
    clean = all((x == -7).all() for x in arrays) and n.value == -7 and (ref == -7.0).all() and (tot == -7).all()
    return rc, bool(clean)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_leave_the_outputs_untouched(pkg, dev):
    V, T = C.case("cube_with_void")
    T_big, T_neg, V_nan, V_inf = T.copy(), T.copy(), V.copy(), V.copy()
    T_big[5, 2], T_neg[0, 0], V_nan[3, 1], V_inf[15, 2] = len(V), -1, np.nan, -np.inf
    for Vx, Tx in ((V, T_big), (V, T_neg), (V_nan, T), (V_inf, T)):                 # an out-of-range index, a non-finite vertex
        assert _raw(pkg, Vx, Tx, dev=dev) == (ARG, True)
    for null in (("verts",), ("tris",), ("out",), ("n",), ("ref",), ("tot",)):      # NULL arrays with a count, NULL scalar outputs
        assert _raw(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    if dev:
        for null in (("counts",), ("vol",), ("capacity",)):                         # NULL tables with a capacity, a negative capacity
            assert _raw(pkg, V, T, dev=True, null=null) == (ARG, True), null
    assert _raw(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _raw(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    for flags in (2, 3, -1, 1 << 20):                                                # a bad flag
        assert _raw(pkg, V, T, flags=flags, dev=dev) == (ARG, True), flags
    # n_tris > 2^30 as a fake count on the tiny buffer: refused before anything is read; n_verts beyond 32 bits likewise
    assert _raw(pkg, V, T, nt=2 ** 30 + 1, dev=dev) == (UNSUPPORTED, True)
    assert _raw(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    assert _raw(pkg, V, T, dev=dev)[0] == 0                                          # (and the same call goes through unharmed)


def test_dev_capacity_too_small_leaves_the_tables_untouched(pkg):
    import torch
    L = pkg._lib
    V, T = C.case("cube_with_void")
    v, t = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    out = torch.full((len(T), 3), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")
    vol = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    n, ref, tot = ctypes.c_int64(), np.zeros(3), np.zeros(8, np.int64)
    vp = ctypes.c_void_p
    args = (vp(v.data_ptr()), len(V), vp(t.data_ptr()), len(T), 1, vp(out.data_ptr()), None, None, vp(counts.data_ptr()), vp(vol.data_ptr()))
    tail = (ctypes.byref(n), ref.ctypes.data_as(L.c_double_p), tot.ctypes.data_as(L.c_int64_p), None)
    for cap in (0, 1):
        L.check(L.lib().r2s_mesh_orient_dev(*args, cap, *tail))
        assert n.value == 2 and tot.tolist() == [2, 24, 0, 12, 0, 2, 2, 0] and (ref == 1.0).all()
        assert (counts == -7).all() and (vol == -7.0).all()
        assert np.array_equal(out.cpu().numpy(), C.reverse(T, np.arange(12, 24)))      # the triangles are always written
    L.check(L.lib().r2s_mesh_orient_dev(*args, 2, *tail))
    assert counts.cpu().numpy()[:, :4].tolist() == [[0, 12, 0, 5], [12, 12, 12, 5]] and vol.cpu().numpy().tolist() == [8.0, 1.0]
    m = ctypes.c_int64()
    pkg.mesh_orient(*C.case("tetrahedron"))                                          # the thread's last result is the host variant's
    L.check(L.lib().r2s_mesh_orient_dev(*args, 2, *tail))
    L.check(L.lib().r2s_last_mesh_orient(None, None, 0, ctypes.byref(m)))
    assert m.value == 1


# ---- STL import --------------------------------------------------------------------------------------------------------------

def test_import_stl_orient_outward(pkg, tmp_path):
    V, plain = C.case("sphere33")
    _, T = C.case("sphere33", True)
    path = pkg.export_stl(str(tmp_path / "scrambled"), V, T)
    want = pkg.mesh_shells(V, plain)
    assert want.n_shells == 1 and want.closed[0] and want.volume[0] > 0
    Vk, Tk = pkg.import_stl(path)                                                     # today's behaviour: the windings of the file
    kept = pkg.mesh_shells(Vk, Tk)
    assert kept.totals[5] > 0 and not kept.closed[0]
    Vk2, Tk2 = pkg.import_stl(path, orient=None)
    assert np.array_equal(Vk2.view(np.uint32), Vk.view(np.uint32)) and np.array_equal(Tk2, Tk)
    for orient in ("outward", "majority"):
        Vo, To = pkg.import_stl(path, orient=orient)
        assert np.array_equal(Vo.view(np.uint32), Vk.view(np.uint32)) and np.array_equal(np.sort(To, 1), np.sort(Tk, 1))
        got = pkg.mesh_shells(Vo, To)
        assert got.n_shells == 1 and got.closed[0] and got.totals[5] == 0 and got.volume[0] > 0
        assert got.totals[0:2].tolist() == [1, len(To)] and got.genus[0] == want.genus[0]
        assert abs(got.volume[0] - want.volume[0]) <= 1e-9 * want.volume[0] and abs(got.area[0] - want.area[0]) <= 1e-9 * want.area[0]
    for bad in (dict(orient="inward"), dict(orient="outward", weld=False)):
        with pytest.raises(pkg._lib.R2SError):
            pkg.import_stl(path, **bad)
