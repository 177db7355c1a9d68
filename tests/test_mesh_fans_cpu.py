"""Host-side parts of the mesh fans (no GPU): the restatement of tests/mesh_fans_ref.py held to what the header promises on every
case of tests/mesh_fans_cases.py (the numbering, the invariants of closed and open fans, the consequences of the split for the
shells, idempotence, permutations of the triangles); the figures the case descriptions promise; the refusals of r2s_mesh_fans
that come before any device work; the exported symbols and the Julia ccall tuples."""
import ctypes
import os

import numpy as np
import pytest

import mesh_fans_cases as C
import mesh_fans_ref as R
import mesh_shells_ref64 as M
from test_mesh_orient_cpu import C_TO_JULIA, INTEGRATION, JULIA, _c_params, _ccalls

ARG, UNSUPPORTED, NO_DEVICE = -1, -4, -2
TOO_MANY_TRIS = (2 ** 31 - 1) // 3 + 1                  # the smallest n_tris with 3 * n_tris >= 2^31

_ref = {}


def ref(name, variant=None):
    """the restatement of a case (with the split), computed once and left unchanged"""
    if (name, variant) not in _ref:
        _ref[(name, variant)] = R.fans(*C.case(name, variant))
    return _ref[(name, variant)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.mark.parametrize("name,variant", C.variants())
def test_restatement_properties(name, variant):
    V, T = C.case(name, variant)
    r = ref(name, variant)                             # (asserts the invariants of closed and open fans on every fan)
    foc, cnt, tot = r["fan_of_corner"].reshape(-1), r["counts"], r["totals"]
    n = len(cnt)
    collapsed = (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 0] == T[:, 2])
    assert np.array_equal(foc.reshape(-1, 3) < 0, np.repeat(collapsed[:, None], 3, 1))
    # numbered by ascending vertex, then ascending first corner; the first corner is the smallest corner of the fan
    key = cnt[:, 0] * (3 * len(T) + 1) + cnt[:, 1]
    assert (np.diff(key) > 0).all() and np.array_equal(foc[cnt[:, 1]], np.arange(n))
    first = np.full(n, 3 * len(T), np.int64)
    np.minimum.at(first, foc[foc >= 0], np.nonzero(foc >= 0)[0])
    assert np.array_equal(first, cnt[:, 1]) and np.array_equal(T.reshape(-1)[cnt[:, 1]], cnt[:, 0])
    assert np.array_equal(np.bincount(foc[foc >= 0], minlength=n), cnt[:, 2]) and cnt[:, 2].sum() == 3 * (len(T) - collapsed.sum())
    assert np.array_equal(np.bincount(cnt[:, 0], minlength=len(V)), r["fans_of_vert"])
    assert (cnt[:, 4:7].sum(1) <= cnt[:, 3]).all()
    # every edge is counted at both of its ends: the fans' edge columns sum to twice the shells' totals
    _, _, stot = M.topology(T)
    assert (cnt[:, 3:7].sum(0) == 2 * stot[3:7]).all()
    assert tot[3] == stot[7] and tot[3] + tot[4] == len(V) and tot[0] == n and tot[2] == collapsed.sum()
    assert tot[5] == (r["fans_of_vert"] >= 2).sum() and r["n_added"] == n - tot[3]
    # the split: copies, the vertex of every corner is a copy of the input's, nothing else moves
    assert np.array_equal(r["vert_of"][:len(V)], np.arange(len(V))) and len(r["vert_of"]) == len(V) + r["n_added"]
    assert np.array_equal(_bits(r["verts"]), _bits(V[r["vert_of"]])) and np.array_equal(r["vert_of"][r["tris"]], T)
    assert np.array_equal(r["tris"][collapsed], T[collapsed])
    extra = cnt[np.concatenate([[False], cnt[1:, 0] == cnt[:-1, 0]]), 0] if n else cnt[:0, 0]
    assert np.array_equal(r["vert_of"][len(V):], extra)


@pytest.mark.parametrize("name,variant", C.variants())
def test_split_consequences_and_idempotence(name, variant):
    V, T = C.case(name, variant)
    r = ref(name, variant)
    a, b = M.shells(V, T), M.shells(r["verts"], r["tris"])
    assert np.array_equal(a["shell_of_tri"], b["shell_of_tri"])
    assert np.array_equal(a["counts"][:, [0, 1, 3, 4, 5, 6]], b["counts"][:, [0, 1, 3, 4, 5, 6]])
    assert np.array_equal(a["totals"][:7], b["totals"][:7])
    assert np.array_equal(_bits(a["ref_point"]), _bits(b["ref_point"])) and np.array_equal(_bits(a["sums"]), _bits(b["sums"]))
    # the vertex counts grow: the total by n_added; a shell's by the fans it has beyond its distinct vertices (a vertex that two
    # shells share counted in both before the split already), so that afterwards a shell has one vertex per fan
    assert b["totals"][7] - a["totals"][7] == r["n_added"]
    shell_of_fan = a["shell_of_tri"][r["counts"][:, 1] // 3]
    assert np.array_equal(b["counts"][:, 2], np.bincount(shell_of_fan, minlength=len(a["counts"])))
    grow = b["counts"][:, 2] - a["counts"][:, 2]
    assert (grow >= 0).all() and grow.sum() <= r["n_added"]
    again = R.fans(r["verts"], r["tris"])
    assert again["fans_of_vert"].max(initial=0) <= 1 and again["n_added"] == 0 and again["totals"][5] == 0
    assert np.array_equal(again["tris"], r["tris"]) and np.array_equal(_bits(again["verts"]), _bits(r["verts"]))
    assert np.array_equal(again["totals"][[0, 1, 2, 6, 7]], r["totals"][[0, 1, 2, 6, 7]])
    rows = lambda c: sorted(map(tuple, c[:, 2:].tolist()))   # noqa: E731
    assert rows(again["counts"]) == rows(r["counts"])                                 # the fans themselves are the same


def follows_permutation(a, p, perm):
    """p is the result on the triangles perm of the mesh of a: the partition, and the records after mapping first_corner"""
    nt = len(perm)
    corner_in_a = (3 * perm[:, None] + np.arange(3)[None, :]).reshape(-1)       # corner 3k + c of p is corner 3 perm[k] + c of a
    fa, fp = a["fan_of_corner"].reshape(-1), p["fan_of_corner"].reshape(-1)
    to_a = fa[corner_in_a[p["counts"][:, 1]]]                                   # fan k of p is fan to_a[k] of a
    assert len(np.unique(to_a)) == len(a["counts"]) == len(p["counts"])
    has = fp >= 0
    assert np.array_equal(has, fa[corner_in_a] >= 0) and np.array_equal(to_a[fp[has]], fa[corner_in_a][has])
    assert np.array_equal(p["counts"][:, [0, 2, 3, 4, 5, 6, 7]], a["counts"][to_a][:, [0, 2, 3, 4, 5, 6, 7]])
    first = np.full(len(to_a), 3 * nt, np.int64)
    np.minimum.at(first, to_a[fp[has]], corner_in_a[has])
    assert np.array_equal(first, a["counts"][:, 1])                              # first_corner, mapped, is the smallest again
    assert np.array_equal(p["totals"], a["totals"]) and np.array_equal(p["fans_of_vert"], a["fans_of_vert"])
    return True


@pytest.mark.parametrize("name", tuple(C.NEW))
def test_fans_follow_a_permutation_of_the_triangles(name):
    assert follows_permutation(ref(name), ref(name, "permuted"), C.perm_of(name))
    # reversing triangles swaps their corners 1 and 2 and changes the flipped-edge column; the fans and their numbers stay (two
    # fans of one vertex never share a triangle, so their order by smallest corner is their order by smallest triangle)
    a, b = ref(name), ref(name, "reversed")
    rev = (C.case(name)[1] != C.case(name, "reversed")[1]).any(1)
    assert rev.any() or len(rev) < 20
    back = b["fan_of_corner"].copy()
    back[rev] = back[rev][:, [0, 2, 1]]
    assert np.array_equal(a["fan_of_corner"], back) and np.array_equal(a["counts"][:, [0, 2, 3, 4, 6, 7]], b["counts"][:, [0, 2, 3, 4, 6, 7]])
    assert np.array_equal(a["counts"][:, 1] // 3, b["counts"][:, 1] // 3)


def test_restatement_on_the_named_cases():
    """the figures the case descriptions promise"""
    t = lambda name: ref(name)["totals"].tolist()   # noqa: E731
    assert t("empty") == [0] * 8 and t("all_collapsed") == [0, 4, 4, 0, 3, 0, 0, 0]
    assert t("bowtie") == [6, 2, 0, 5, 0, 1, 0, 6]
    assert ref("bowtie")["counts"].tolist()[:2] == [[0, 0, 1, 2, 2, 0, 0, 1], [0, 3, 1, 2, 2, 0, 0, 1]]
    assert ref("bowtie")["tris"].tolist() == [[0, 1, 2], [5, 3, 4]] and ref("bowtie")["vert_of"].tolist() == [0, 1, 2, 3, 4, 0]
    assert t("two_tets_sharing_vertex") == [8, 8, 0, 7, 0, 1, 0, 0]
    assert ref("two_tets_sharing_vertex")["counts"][:2, [0, 2, 3, 7]].tolist() == [[0, 3, 3, 0]] * 2
    assert M.topology(C.case("two_tets_sharing_vertex")[1])[2][0] == 2
    r = ref("pinched_sphere")                         # one shell, one pinched vertex; the Euler characteristic rises by 1
    s0, s1 = M.topology(C.case("pinched_sphere")[1]), M.topology(r["tris"])
    assert s0[2][0] == 1 and s0[2][4:7].tolist() == [0, 0, 0] and r["totals"].tolist() == [10, 16, 0, 9, 0, 1, 0, 0]
    euler = lambda c: int(c[0, 2] - c[0, 3] + c[0, 1])   # noqa: E731
    assert (euler(s0[1]), euler(s1[1])) == (1, 2)
    r = ref("disk_and_cone")
    assert r["fans_of_vert"][0] == 2 and sorted(r["counts"][:2, 7].tolist()) == [0, 1] and r["totals"][5] == 1
    r = ref("cubes_sharing_edge")                     # a complex fan at either end of the non-manifold edge, not split
    assert r["totals"].tolist() == [14, 24, 0, 14, 2, 0, 2, 0] and r["n_added"] == 0 and (r["counts"][[3, 7], 7] == 2).all()
    assert (r["counts"][[3, 7], 6] == 1).all() and np.array_equal(r["tris"], C.case("cubes_sharing_edge")[1])
    r = ref("apex300")
    nv = len(C.case("apex300")[0])
    assert r["fans_of_vert"][0] == 300 and r["n_added"] == 299 and np.array_equal(r["tris"][1:, 0], np.arange(nv, nv + 299))
    assert r["tris"][0, 0] == 0 and (r["vert_of"][nv:] == 0).all()
    r = ref("tets40")
    assert r["fans_of_vert"][0] == 40 and r["totals"].tolist() == [160, 160, 0, 121, 0, 1, 0, 0] and (r["counts"][:, 7] == 0).all()
    r = ref("cone5000")
    assert r["counts"][:2, [0, 2, 3, 7]].tolist() == [[0, 5000, 5000, 0], [1, 5000, 5000, 0]] and r["totals"][5] == 0
    r = ref("unused_vertices")
    assert r["fans_of_vert"].tolist() == [0, 0, 2, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0] and r["tris"].max() == 13
    r = ref("collapsed_mixed")
    assert r["fans_of_vert"][9] == 0 and r["totals"][2] == 5 and r["totals"][4] == 1 and r["totals"][5] == 1
    # the welded iso-surface through lattice points: pinched vertices, no complex fan, and clean edges - the shells see nothing
    V, T = C.case("welded_lattice_touch")
    r = ref("welded_lattice_touch")
    assert r["totals"][5] >= 1 and r["totals"][6] == 0 and M.topology(T)[2][4:7].tolist() == [0, 0, 0]
    V0, T0 = C.extracted("lattice_touch")             # as extracted (unwelded) every vertex has one fan
    assert R.fans(V0, T0, split=False)["totals"][5] == 0 and len(V0) > len(V)


# ---- the library without a device -----------------------------------------------------------------------------------------

def test_symbols_and_exports(pkg):
    lib = pkg._lib.lib()
    for s in ("r2s_mesh_fans", "r2s_last_mesh_fans", "r2s_mesh_fans_dev"):
        assert hasattr(lib, s) and [x[0] for x in pkg._lib.SYMBOLS].count(s) == 1
    for name in ("MeshFans", "mesh_fans", "mesh_fans_dev"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def _call(pkg, V, T, nv=None, nt=None, dev=False, null=(), vcap=None, alias=None, fcap=0):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs (dev: host memory as "device" pointers - every call
    here is refused before anything reads them).  null: the arguments passed as NULL; alias: the output given the address of
    the input triangles"""
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    vcap = len(v) + 8 if vcap is None else vcap
    foc, fov, to = np.full((len(t) + 1, 3), -7, np.int32), np.full(len(v) + 1, -7, np.int32), np.full((len(t) + 1, 3), -7, np.int32)
    vo, vof, cnt = np.full((len(v) + 9, 3), -7.0, np.float32), np.full(len(v) + 9, -7, np.int32), np.full((8, 8), -7, np.int64)
    n, nvo, tot = ctypes.c_int64(-7), ctypes.c_int64(-7), np.full(8, -7, np.int64)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    arr = dict(verts=v, tris=t, foc=foc, fov=fov, to=to, vo=vo, vof=vof, cnt=cnt)
    if alias:
        arr[alias] = t
    tail = [None if "n" in null else ctypes.byref(n), None if "nvo" in null else ctypes.byref(nvo),
            None if "tot" in null else tot.ctypes.data_as(L.c_int64_p)]
    if dev:
        p = lambda k: None if k in null else arr[k].ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        rc = L.lib().r2s_mesh_fans_dev(p("verts"), nv, p("tris"), nt, p("foc"), p("fov"), p("cnt"), fcap, p("to"), p("vo"), p("vof"), vcap,
                                       *tail, None)
    else:
        ip = lambda k: None if k in null else arr[k].ctypes.data_as(L.c_int32_p)   # noqa: E731
        fp = lambda k: None if k in null else arr[k].ctypes.data_as(L.c_float_p)   # noqa: E731
        rc = L.lib().r2s_mesh_fans(fp("verts"), nv, ip("tris"), nt, -1, ip("foc"), ip("fov"), ip("to"), fp("vo"), ip("vof"), vcap, *tail)
    clean = all((x == -7).all() for x in (foc, fov, to, vo, vof, cnt, tot)) and n.value == -7 and nvo.value == -7
    return rc, bool(clean) and np.array_equal(t, np.ascontiguousarray(T, np.int32).reshape(-1, 3))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_before_any_device_work(pkg, dev):
    V, T = C.case("two_tets_sharing_vertex")
    assert _call(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _call(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    for null in (("verts",), ("tris",), ("n",), ("nvo",), ("tot",)):                 # NULL arrays with a count, NULL scalar outputs
        assert _call(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    for null in (("vo",), ("vof",), ("vo", "vof"), ("to",)):                         # tris_out without verts_out / vert_of_out, and back
        assert _call(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    assert "together" in pkg._lib.lib().r2s_last_error().decode()
    assert _call(pkg, V, T, dev=dev, vcap=-1) == (ARG, True)
    for alias in ("foc", "to"):                                                       # an output overlapping an input
        assert _call(pkg, V, T, dev=dev, alias=alias) == (ARG, True), alias
        assert "overlaps" in pkg._lib.lib().r2s_last_error().decode()
    if dev:
        assert _call(pkg, V, T, dev=True, fcap=-1) == (ARG, True) and _call(pkg, V, T, dev=True, fcap=4, null=("cnt",)) == (ARG, True)
    assert _call(pkg, V, T, nt=TOO_MANY_TRIS, dev=dev) == (UNSUPPORTED, True)        # refused before anything is read
    assert "2^31" in pkg._lib.lib().r2s_last_error().decode()
    assert _call(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    lib = pkg._lib.lib()
    n = ctypes.c_int64()
    assert lib.r2s_last_mesh_fans(None, 4, ctypes.byref(n)) == ARG and lib.r2s_last_mesh_fans(None, 0, None) == ARG
    assert lib.r2s_last_mesh_fans(None, -1, ctypes.byref(n)) == ARG


def test_host_mesh_check_comes_before_the_device(pkg):
    V, T = C.case("two_tets_sharing_vertex")
    T2, V2, V3 = T.copy(), V.copy(), V.copy()
    T2[5, 1], V2[3, 2], V3[0, 0] = len(V), np.nan, np.inf
    for v, t in ((V, T2), (V, T - 1), (V2, T), (V3, T)):
        assert _call(pkg, v, t) == (ARG, True)
        msg = pkg._lib.lib().r2s_last_error().decode()
        assert msg.startswith("mesh_fans:") and ("not finite" in msg or "outside" in msg)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = C.case("bowtie")
    assert _call(pkg, V, T) == (NO_DEVICE, True) and _call(pkg, V, T, dev=True) == (NO_DEVICE, True)
    with pytest.raises(pkg._lib.R2SError, match="error -2"):
        pkg.mesh_fans(V, T, split=True)


def test_meshfans_derived_fields(pkg):
    """the host-side fields of the result class, on the restatement's tables"""
    for name in ("bowtie", "cubes_sharing_edge", "welded_lattice_touch", "tetrahedron"):
        r = ref(name)
        f = pkg.MeshFans(r["fan_of_corner"], r["fans_of_vert"], r["counts"], r["totals"], len(C.case(name)[0]), r["verts"], r["tris"],
                         r["vert_of"])
        assert f.n_fans == len(f) == r["totals"][0] and f.n_added == r["n_added"] and f.n_verts_out == len(r["verts"])
        assert np.array_equal(f.pinched, np.nonzero(r["fans_of_vert"] >= 2)[0])
        assert f.closed.sum() + f.open.sum() + f.complex.sum() == f.n_fans and f.complex.sum() == r["totals"][6]
        assert f.vertex_manifold == (name == "tetrahedron")


# ---- the Julia binding and the INTEGRATION snippet against the header -------------------------------------------------------

@pytest.mark.parametrize("path", [JULIA, INTEGRATION], ids=["julia", "integration"])
def test_ccall_type_tuples_match_the_header(path):
    to_julia = dict(C_TO_JULIA, **{"float *": {"Ptr{Float32}", "Ptr{Cvoid}"}})
    src = open(path).read()
    for name in ("r2s_mesh_fans", "r2s_last_mesh_fans", "r2s_mesh_fans_dev"):
        c = _c_params(name)
        calls = _ccalls(src, name)
        if path == INTEGRATION and name != "r2s_mesh_fans":
            continue                                  # (the snippet shows the host call)
        assert calls, f"{name}: no ccall in {os.path.basename(path)}"
        for types in calls:
            assert len(types) == len(c), (name, types, c)
            for jt, ct in zip(types, c):
                assert jt in to_julia[ct], (name, jt, ct)
                if name != "r2s_mesh_fans_dev":
                    assert jt != "Ptr{Cvoid}", (name, jt, ct)   # the host variants use typed pointers
    assert "mesh_fans" in src and "pinched" in src
