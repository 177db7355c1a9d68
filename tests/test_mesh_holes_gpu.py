"""The mesh holes on the GPU (r2s_mesh_holes, r2s_mesh_holes_dev, import_stl(fill_holes=...)) against the restatement of
tests/mesh_holes_ref.py on every case of tests/mesh_holes_cases.py and its variants: rim_start, rim_edge, every integer record,
the totals, the output triangles and all copied vertex bits EQUAL; the Float64 records within the header's bound
(n_edges + K) 2^-53 T of the exact sums; every added vertex within, per axis, 2^-24 |c| + 2^-149 (the float32 rounding of the
exact mean c) + bound / n_edges (the sum) + 2^-52 |c| (the division and the addition in double).  The largest fraction of that
bound the restatement itself uses is 0.915 (printed by tests/test_mesh_holes_cpu.py)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import mesh_holes_cases as C
import mesh_holes_ref as R
from test_mesh_holes_cpu import ARG, TOO_MANY_TRIS, UNSUPPORTED, follows_variant, ref

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same(a, b):
    """two results bit for bit"""
    return (np.array_equal(a.rim_start, b.rim_start) and np.array_equal(a.rim_edge, b.rim_edge) and np.array_equal(a.counts, b.counts)
            and np.array_equal(_bits(a.sums), _bits(b.sums)) and np.array_equal(_bits(a.ref_point), _bits(b.ref_point))
            and np.array_equal(a.totals, b.totals) and np.array_equal(a.tris, b.tris) and a.verts.shape == b.verts.shape
            and np.array_equal(_bits(a.verts), _bits(b.verts)))


def _dev(pkg, V, T, fill=-1, capacity=0, edge_capacity=0):
    import torch
    v, t = torch.from_numpy(np.ascontiguousarray(V)).cuda(), torch.from_numpy(np.ascontiguousarray(T)).cuda()
    o = pkg.mesh_holes_dev(v, t, fill=fill, capacity=capacity, edge_capacity=edge_capacity)
    for k in ("rim_edge", "verts", "tris"):
        if getattr(o, k) is not None:
            setattr(o, k, getattr(o, k).cpu().numpy())
    return o


def _check(label, o, r, nv):
    assert np.array_equal(o.rim_start, r["rim_start"]) and o.rim_start.dtype == np.int64, label
    assert np.array_equal(o.rim_edge, r["rim_edge"]) and o.rim_edge.dtype == np.int32, label
    assert np.array_equal(o.counts, r["counts"]) and np.array_equal(o.totals, r["totals"]), label
    assert np.array_equal(_bits(o.ref_point), _bits(r["ref_point"])), label
    err = np.abs(o.sums - r["exact"])
    for c, q in zip(*np.nonzero(err > 0.5 * r["bound"])):               # (float(exact) is itself rounded: settle close calls exactly)
        assert abs(Fraction(float(o.sums[c, q])) - r["exact_sums"][c][q]) <= Fraction(float(r["bound"][c, q])), (label, c, R.NAMES[q])
    assert np.array_equal(o.tris, r["tris"]) and o.tris.dtype == np.int32, label
    assert o.verts.shape == r["verts"].shape and np.array_equal(_bits(o.verts[:nv]), _bits(r["verts"][:nv])), label
    worst = 0.0
    for k, (mean, vb) in enumerate(zip(r["exact_added"], r["added_bound"])):
        for a in range(3):
            e = abs(Fraction(float(o.verts[nv + k, a])) - mean[a])
            assert e <= Fraction(float(vb[a])), (label, k, a)
            worst = max(worst, float(e) / vb[a])
    return worst


@pytest.mark.parametrize("name,variant", C.variants())
def test_equal_to_the_restatement(pkg, name, variant):
    V, T = C.case(name, variant)
    r = ref(name, variant)
    label = f"{name} {variant}"
    o = pkg.mesh_holes(V, T, fill=-1)
    worst = _check(label, o, r, len(V))
    print(f"HOLES {label}: {len(T)} triangles, totals {o.totals.tolist()}, largest fraction of the added-vertex bound {worst:.3f}")
    # the host variant, the _dev variant (asking for the tables, and with room for them) and a second call: bit for bit
    assert _same(o, _dev(pkg, V, T)), label
    assert _same(o, _dev(pkg, V, T, capacity=o.n_rims + 3, edge_capacity=len(o.rim_edge) + 5)), label
    assert _same(o, pkg.mesh_holes(V, T, fill=-1)), label
    # without the fill: the same analysis, nothing selected, no mesh
    p = pkg.mesh_holes(V, T)
    assert p.verts is None and p.tris is None and np.array_equal(p.rim_edge, o.rim_edge) and np.array_equal(_bits(p.sums), _bits(o.sums))
    assert np.array_equal(p.counts[:, :6], o.counts[:, :6]) and np.array_equal(p.counts[:, 6], np.minimum(o.counts[:, 6], 1))
    assert (p.counts[:, 7] == -1).all() and p.totals[:6].tolist() == o.totals[:6].tolist() and p.totals[6:].tolist() == [0, 0]
    assert p.watertight == (len(r["rim_edge"]) == 0)


@pytest.mark.parametrize("fill", C.FILLS)
def test_max_edges_selects_the_rims(pkg, fill):
    V, T = C.case("tube_and_cube")
    r = ref("tube_and_cube", None, fill)
    o = pkg.mesh_holes(V, T, fill=fill)
    _check(f"tube_and_cube fill={fill}", o, r, len(V))
    assert _same(o, _dev(pkg, V, T, fill=fill))
    assert o.totals[6:].tolist() == {-1: [3, 20], 0: [0, 0], 4: [1, 4], 8: [3, 20]}[fill]


def test_fresh_work_buffers_give_the_same_bits(pkg):
    V, T = C.case("ico_many_holes")
    a = pkg.mesh_holes(V, T, fill=-1)
    pkg._lib.lib().r2s_release_cache()
    assert _same(a, pkg.mesh_holes(V, T, fill=-1)) and _same(a, _dev(pkg, V, T))
    _check("after release", a, ref("ico_many_holes"), len(V))


@pytest.mark.parametrize("name", ["disk257", "disk16385", "tube_and_cube", "ico_many_holes", "gyroid17", "degenerate_mixed"])
@pytest.mark.parametrize("variant", C.VARIANTS[1:])
def test_permuted_triangles_and_rotated_corners(pkg, name, variant):
    a = ref(name)                                     # (bounds, exact means)
    res = lambda o: dict(rim_start=o.rim_start, rim_edge=o.rim_edge, counts=o.counts, totals=o.totals, sums=o.sums, verts=o.verts)   # noqa: E731
    plain, var = pkg.mesh_holes(*C.case(name), fill=-1), pkg.mesh_holes(*C.case(name, variant), fill=-1)
    base = dict(res(plain), bound=a["bound"], added_bound=a["added_bound"])
    assert follows_variant(name, variant, base, res(var))


@pytest.mark.parametrize("name", ["one_triangle", "tet_minus_face", "cube_minus_face", "tube_and_cube", "bowtie", "ico_touching_holes",
                                  "strip_one_reversed", "moebius", "fin", "degenerate_mixed", "disk257", "ico_many_holes", "gyroid17"])
def test_consequences_on_the_output_mesh(pkg, name):
    V, T = C.case(name)
    o = pkg.mesh_holes(V, T, fill=-1)
    nv, nt = len(V), len(T)
    filled_edges = int(o.n_edges[o.filled].sum())
    a, b = pkg.mesh_shells(V, T), pkg.mesh_shells(o.verts, o.tris)
    assert b.totals[4] == a.totals[4] - filled_edges and b.totals[5] == a.totals[5] and b.totals[6] == a.totals[6]
    assert np.array_equal(b.shell_of_tri[:nt], a.shell_of_tri)
    f0, f1 = pkg.mesh_fans(V, T), pkg.mesh_fans(o.verts, o.tris)
    assert np.array_equal(f1.fans_of_vert[:nv], f0.fans_of_vert) and (f1.fans_of_vert[nv:] == 1).all()
    at_w = f1.counts[f1.counts[:, 0] >= nv]
    assert len(at_w) == len(o.verts) - nv and (at_w[:, 7] == 0).all()
    assert sorted(at_w[:, 2].tolist()) == sorted(o.n_edges[o.counts[:, 6] == 3].tolist())
    again = pkg.mesh_holes(o.verts, o.tris, fill=-1)                                  # a second fill adds nothing
    assert again.totals[5:].tolist() == [0, 0, 0] and np.array_equal(again.tris, o.tris) and np.array_equal(_bits(again.verts), _bits(o.verts))
    assert again.n_rims == o.n_rims - o.totals[6]


def test_split_then_fill_closes_touching_holes(pkg):
    """the recipe for a pinched boundary vertex: the branch node blocks the fill, the fans' split makes it regular"""
    for name in ("bowtie", "ico_touching_holes"):
        V, T = C.case(name)
        o = pkg.mesh_holes(V, T, fill=-1)
        assert o.totals[4:].tolist() == [1, 0, 0, 0] and np.array_equal(o.tris, T) and o.counts[0, 5] == 1
        f = pkg.mesh_fans(V, T, split=True)
        h = pkg.mesh_holes(f.verts, f.tris, fill=-1)
        assert h.totals[4] == 0 and h.totals[5] == h.totals[6] == h.n_rims == (2 if name == "bowtie" else 1)
        s = pkg.mesh_shells(h.verts, h.tris)
        assert s.totals[4] == 0 and s.closed.all()


def test_geometry_after_the_fill(pkg):
    V, T = C.case("cube_minus_face")
    o = pkg.mesh_holes(V, T, fill=-1)
    assert o.verts[8].tolist() == [0.5, 0.5, 0.0]                                     # w is the face centre exactly
    s = pkg.mesh_shells(o.verts, o.tris)
    import mesh_shells_ref64 as M
    assert s.n_shells == 1 and s.closed[0] and abs(s.sums[0, 1] - 1.0) <= M.shells(o.verts, o.tris)["bound"][0, 1]
    ix = pkg.MeshIndex(o.verts, o.tris)
    pts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 0.5, -0.25], [0.5, -2.0, 0.5]])
    for ray in range(6):
        assert ix.contains(pts, ray=ray).tolist() == [True, False, False, False], ray
    V, T = C.case("ico_many_holes")
    o = pkg.mesh_holes(V, T, fill=-1)
    assert len(pkg.mesh_intersections(o.verts, o.tris)) == 0
    s = pkg.mesh_shells(o.verts, o.tris)
    assert s.n_shells == 1 and s.closed[0] and s.totals[4] == 0


def test_import_stl_fill_holes(pkg, tmp_path):
    V, T = C.case("cube_minus_face")
    path = pkg.export_stl(str(tmp_path / "open_cube"), V, T)
    Vk, Tk = pkg.import_stl(path)
    assert len(Vk) == 8 and not pkg.mesh_shells(Vk, Tk).closed[0] and pkg.mesh_holes(Vk, Tk).n_edges.tolist() == [4]
    Vf, Tf = pkg.import_stl(path, fill_holes=-1)
    s = pkg.mesh_shells(Vf, Tf)
    assert len(Vf) == 9 and len(Tf) == 14 and s.n_shells == 1 and s.closed[0] and pkg.mesh_holes(Vf, Tf).watertight
    Vn, Tn = pkg.import_stl(path, fill_holes=3)                                       # the rim of 4 is not selected
    assert len(Vn) == 8 and len(Tn) == 10
    with pytest.raises(pkg._lib.R2SError):
        pkg.import_stl(path, fill_holes=-1, weld=False)


# ---- refusals and capacities -------------------------------------------------------------------------------------------------

def _raw(pkg, V, T, nv=None, nt=None, dev=False, null=(), vcap=None, tcap=None, rcap=8, ecap=64, alias=None):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs; `null`: the arguments passed as NULL; alias: the output
    that is given the address of the input triangles"""
    import torch
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    vcap, tcap = len(v) + 8 if vcap is None else vcap, len(t) + 8 if tcap is None else tcap
    sc = [ctypes.c_int64(-7) for _ in range(4)]
    r, tot = np.full(3, -7.0), np.full(8, -7, np.int64)
    tail = [None if f"s{k}" in null else ctypes.byref(sc[k]) for k in range(4)]
    tail += [None if "r" in null else r.ctypes.data_as(L.c_double_p), None if "tot" in null else tot.ctypes.data_as(L.c_int64_p)]
    shapes = dict(start=((9,), np.int64), cnt=((8, 8), np.int64), sums=((8, 7), np.float64), edge=((64,), np.int32),
                  to=((len(t) + 8, 3), np.int32), vo=((len(v) + 8, 3), np.float32))
    if dev:
        arr = dict(verts=torch.from_numpy(v).cuda(), tris=torch.from_numpy(t).cuda())
        for k, (shape, dt) in shapes.items():
            arr[k] = torch.full(shape, -7, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        p = lambda k: None if k in null else ctypes.c_void_p(arr["tris" if k == alias else k].data_ptr())   # noqa: E731
        rc = L.lib().r2s_mesh_holes_dev(p("verts"), nv, p("tris"), nt, -1, p("start"), p("cnt"), p("sums"), rcap, p("edge"), ecap, p("to"),
                                        p("vo"), vcap, tcap, *tail, None)
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
        rc = L.lib().r2s_mesh_holes(fp("verts"), nv, ip("tris"), nt, -1, -1, ip("to"), fp("vo"), vcap, tcap, *tail)
        outs = [arr[k] for k in ("to", "vo")]
        t_after = t
    clean = all((x == -7).all() for x in outs) and all(s.value == -7 for s in sc) and (tot == -7).all() and (r == -7).all()
    return rc, bool(clean) and np.array_equal(t_after, np.ascontiguousarray(T, np.int32).reshape(-1, 3))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_leave_the_outputs_untouched(pkg, dev):
    V, T = C.case("cube_minus_face")
    T_big, T_neg, V_nan, V_inf = T.copy(), T.copy(), V.copy(), V.copy()
    T_big[5, 2], T_neg[0, 0], V_nan[3, 1], V_inf[6, 2] = len(V), -1, np.nan, -np.inf
    for Vx, Tx in ((V, T_big), (V, T_neg), (V_nan, T), (V_inf, T)):                 # an out-of-range index, a non-finite vertex
        assert _raw(pkg, Vx, Tx, dev=dev) == (ARG, True)
    for null in (("verts",), ("tris",), ("s0",), ("s3",), ("r",), ("tot",), ("vo",), ("to",)):
        assert _raw(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    assert _raw(pkg, V, T, dev=dev, alias="to") == (ARG, True)                       # an output overlapping an input
    if dev:
        for kw in (dict(null=("cnt",)), dict(null=("edge",)), dict(rcap=-1), dict(ecap=-1), dict(alias="edge")):
            assert _raw(pkg, V, T, dev=True, **kw) == (ARG, True), kw
    assert _raw(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _raw(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    assert _raw(pkg, V, T, vcap=-1, dev=dev) == (ARG, True) and _raw(pkg, V, T, tcap=-1, dev=dev) == (ARG, True)
    assert _raw(pkg, V, T, nt=TOO_MANY_TRIS, dev=dev) == (UNSUPPORTED, True)
    assert _raw(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    assert _raw(pkg, V, T, dev=dev)[0] == 0                                          # (and the same call goes through unharmed)


def test_capacities_of_every_group(pkg):
    import torch
    L = pkg._lib
    V, T = C.case("tube_and_cube")                                                   # 3 rims, 20 edges, 24 + 3 vertices, 26 + 20 triangles
    r = ref("tube_and_cube")
    nv, nt = len(V), len(T)
    v, t = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    full = lambda shape, dt: torch.full(shape, -7, dtype=dt, device="cuda")   # noqa: E731
    start, cnt, sums, edge = full((5,), torch.int64), full((4, 8), torch.int64), full((4, 7), torch.float64), full((21,), torch.int32)
    to, vo = full((nt + 21, 3), torch.int32), full((nv + 4, 3), torch.float32)
    sc = [ctypes.c_int64() for _ in range(4)]
    rp, tot = np.zeros(3), np.zeros(8, np.int64)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731

    def call(rcap, ecap, vcap, tcap):
        for x in (start, cnt, sums, edge, to, vo):
            x.fill_(-7)
        L.check(L.lib().r2s_mesh_holes_dev(vp(v), nv, vp(t), nt, -1, vp(start), vp(cnt), vp(sums), rcap, vp(edge), ecap, vp(to), vp(vo), vcap,
                                           tcap, *[ctypes.byref(x) for x in sc], rp.ctypes.data_as(L.c_double_p),
                                           tot.ctypes.data_as(L.c_int64_p), None))
        assert [x.value for x in sc] == [3, 20, nv + 3, nt + 20] and tot.tolist() == r["totals"].tolist()   # always returned
        return [bool((x == -7).all()) for x in (start, cnt, sums, edge, vo, to)]

    assert call(2, 19, nv + 2, nt + 19) == [True] * 6                                # one short each: every group keeps its poison
    assert call(3, 19, nv + 2, nt + 19) == [False, False, False, True, True, True]   # room for the rim group only
    assert np.array_equal(cnt.cpu().numpy()[:3], r["counts"]) and (cnt[3:] == -7).all() and (start[4:] == -7).all()
    assert np.array_equal(start.cpu().numpy()[:4], r["rim_start"])
    assert call(2, 20, nv + 2, nt + 19) == [True, True, True, False, True, True]     # the edge group only
    assert np.array_equal(edge.cpu().numpy()[:20], r["rim_edge"]) and (edge[20:] == -7).all()
    assert call(2, 19, nv + 3, nt + 19) == [True, True, True, True, False, True]     # the vertices only
    assert np.array_equal(_bits(vo.cpu().numpy()[:nv]), _bits(V)) and (vo[nv + 3:] == -7).all()
    assert call(2, 19, nv + 2, nt + 20) == [True, True, True, True, True, False]     # the triangles only
    assert np.array_equal(to.cpu().numpy()[:nt + 20], r["tris"]) and (to[nt + 20:] == -7).all()
    # the host variant: each output only into room for it; its tables are the thread's last result, which _dev leaves alone
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
    for vcap, tcap in ((nv + 2, nt + 20), (nv + 3, nt + 19), (nv + 3, nt + 20)):
        out = np.full((nt + 20, 3), -7, np.int32), np.full((nv + 3, 3), -7, np.float32)
        L.check(L.lib().r2s_mesh_holes(V.ctypes.data_as(L.c_float_p), nv, ip(T), nt, -1, -1, ip(out[0]), out[1].ctypes.data_as(L.c_float_p),
                                       vcap, tcap, *[ctypes.byref(x) for x in sc], rp.ctypes.data_as(L.c_double_p),
                                       tot.ctypes.data_as(L.c_int64_p)))
        assert [x.value for x in sc] == [3, 20, nv + 3, nt + 20]
        assert bool((out[0] == -7).all()) == (tcap < nt + 20) and bool((out[1] == -7).all()) == (vcap < nv + 3)
    assert np.array_equal(out[0], r["tris"])
    pkg.mesh_holes(*C.case("bowtie"))
    call(3, 20, nv + 3, nt + 20)
    n, m = ctypes.c_int64(), ctypes.c_int64()
    st, rec, sm, ed = np.full(3, -7, np.int64), np.full((2, 8), -7, np.int64), np.full((2, 7), -7.0), np.full(8, -7, np.int32)
    L.check(L.lib().r2s_last_mesh_holes(st.ctypes.data_as(L.c_int64_p), rec.ctypes.data_as(L.c_int64_p), sm.ctypes.data_as(L.c_double_p), 2,
                                        ip(ed), 4, ctypes.byref(n), ctypes.byref(m)))
    b = ref("bowtie")
    assert (n.value, m.value) == (1, 6) and np.array_equal(rec[:1, :6], b["counts"][:, :6]) and (rec[1:] == -7).all()
    assert st.tolist() == [0, 6, -7] and ed.tolist() == b["rim_edge"][:4].tolist() + [-7] * 4


def test_no_triangles_copies_the_vertices(pkg):
    V = C.case("tetrahedron")[0]
    o = pkg.mesh_holes(V, np.zeros((0, 3), np.int32), fill=-1)
    assert o.n_rims == 0 and o.totals.tolist() == [0] * 8 and o.rim_start.tolist() == [0] and o.watertight
    assert np.array_equal(_bits(o.verts), _bits(V)) and o.tris.shape == (0, 3)
    assert _same(o, _dev(pkg, V, np.zeros((0, 3), np.int32)))
