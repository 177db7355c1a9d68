"""Host-side parts of the mesh holes (no GPU): the restatement of tests/mesh_holes_ref.py held to hand answers and to what the
header promises on every case of tests/mesh_holes_cases.py (the numbering, the output order, the Float64 sums against exact
Fractions - asserted inside the restatement -, the consequences of the fill for the shells and the fans, idempotence, permuted
triangles and rotated corners); the refusals of r2s_mesh_holes that come before any device work; the exported symbols and the
Julia ccall tuples."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import mesh_fans_ref as F
import mesh_holes_cases as C
import mesh_holes_ref as R
import mesh_shells_ref64 as M
from test_mesh_orient_cpu import C_TO_JULIA, INTEGRATION, JULIA, _c_params, _ccalls

ARG, UNSUPPORTED, NO_DEVICE = -1, -4, -2
TOO_MANY_TRIS = (2 ** 31 - 1) // 3 + 1                  # the smallest n_tris with 3 * n_tris >= 2^31

_ref = {}


def ref(name, variant=None, fill=-1):
    """the restatement of a case under fill = max_edges (None: report only), computed once and left unchanged"""
    key = (name, variant, fill)
    if key not in _ref:
        _ref[key] = R.holes(*C.case(name, variant), fill=fill)
    return _ref[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def ends_of(T, h):
    h = np.asarray(h, np.int64)
    return T.reshape(-1)[h], T.reshape(-1)[3 * (h // 3) + (h % 3 + 1) % 3]


@pytest.mark.parametrize("name,variant", C.variants())
def test_restatement_properties(name, variant):
    V, T = C.case(name, variant)
    r = ref(name, variant)                            # (asserts the sums against Fractions and the cycle of every closed rim)
    cnt, tot, start, edge = r["counts"], r["totals"], r["rim_start"], r["rim_edge"]
    n = len(cnt)
    _, _, stot = M.topology(T)
    assert tot[0] == n and tot[1] == len(edge) == stot[4] == cnt[:, 1].sum() and tot[2] == stot[2]
    assert tot[3] == cnt[:, 2].sum() and tot[4] == cnt[:, 3:6].sum() and tot[5] == (cnt[:, 6] >= 1).sum()
    assert np.array_equal(np.diff(start), cnt[:, 1]) and (np.diff(cnt[:, 0]) > 0).all()
    assert sorted(edge.tolist()) == sorted(set(edge.tolist()))          # every boundary half-edge once
    frm, to = ends_of(T, edge)
    for c in range(n):
        lo, hi = start[c], start[c + 1]
        assert edge[lo] == cnt[c, 0] == edge[lo:hi].min()
        if cnt[c, 6] >= 1:                            # closed: a walk along the successors, back to the start
            assert np.array_equal(to[lo:hi], np.roll(frm[lo:hi], -1)) and cnt[c, 1] == cnt[c, 2] >= 3 and not cnt[c, 3:6].any()
        else:
            assert (np.diff(edge[lo:hi]) > 0).all() and cnt[c, 3:6].any()
    # the fill of every closed rim: copies bit for bit, the caps, the counts
    assert np.array_equal(r["tris"][:len(T)], T) and np.array_equal(_bits(r["verts"][:len(V)]), _bits(V))
    fan = cnt[:, 6] == 3
    assert tot[6] == (cnt[:, 6] >= 2).sum() == tot[5] and tot[7] == len(r["tris"]) - len(T) == cnt[fan, 1].sum() + (cnt[:, 6] == 2).sum()
    assert np.array_equal(cnt[fan, 7], len(V) + np.arange(fan.sum())) and (cnt[~fan, 7] == -1).all()
    assert len(r["verts"]) == len(V) + fan.sum()


@pytest.mark.parametrize("name,variant", C.variants())
def test_fill_consequences_and_idempotence(name, variant):
    V, T = C.case(name, variant)
    r = ref(name, variant)
    nt, filled_edges = len(T), int(r["counts"][r["counts"][:, 6] >= 2, 1].sum())
    s0, c0, t0 = M.topology(T)
    s1, c1, t1 = M.topology(r["tris"])
    assert t1[4] == t0[4] - filled_edges and t1[5] == t0[5] and t1[6] == t0[6]
    assert np.array_equal(s1[:nt], s0)                # the shells of the input triangles, and the caps in those of their rims
    assert np.array_equal(s1[nt:], s0[_tri_of_cap(r, T)])
    f0, f1 = F.fans(V, T, split=False), F.fans(r["verts"], r["tris"], split=False)
    added = r["counts"][r["counts"][:, 6] == 3]
    assert np.array_equal(f1["fans_of_vert"][:len(V)], f0["fans_of_vert"]) and (f1["fans_of_vert"][len(V):] == 1).all()
    w_fans = f1["counts"][np.isin(f1["counts"][:, 0], added[:, 7])]
    assert len(w_fans) == len(added) and (w_fans[:, 7] == 0).all() and sorted(w_fans[:, 2].tolist()) == sorted(added[:, 1].tolist())
    again = R.holes(r["verts"], r["tris"], fill=-1)
    assert again["totals"][6] == 0 and again["totals"][7] == 0 and again["totals"][5] == 0
    assert np.array_equal(again["tris"], r["tris"]) and np.array_equal(_bits(again["verts"]), _bits(r["verts"]))
    assert again["totals"][0] == r["totals"][0] - r["totals"][6]                      # the other rims are untouched
    keep = r["counts"][:, 6] < 2
    assert np.array_equal(again["counts"][:, 1:7], r["counts"][keep][:, 1:7])


def _tri_of_cap(r, T):
    """for every added triangle the input triangle of the boundary half-edge it was made for (the first one, for a rim of 3)"""
    out = []
    for c in np.nonzero(r["counts"][:, 6] >= 2)[0]:
        walk = r["rim_edge"][r["rim_start"][c]:r["rim_start"][c + 1]]
        out += (walk[:1] if r["counts"][c, 6] == 2 else walk).tolist()
    return np.array(out, np.int64) // 3


def follows_variant(name, variant, a, p, factor=2.0):
    """p is the result on a variant of the mesh of a: the partition and every integer once `first` is mapped, closed rims as
    cyclic sequences, sums and added vertices within `factor` times the bound"""
    old = C.old_half_edge(name, variant, p["rim_edge"])
    rim_of_a = np.empty(3 * len(C.case(name)[1]), np.int64)
    rim_of_a[a["rim_edge"]] = np.repeat(np.arange(len(a["counts"])), a["counts"][:, 1])
    n = len(p["counts"])
    assert n == len(a["counts"]) and np.array_equal(p["totals"], a["totals"])
    to_a = rim_of_a[C.old_half_edge(name, variant, p["counts"][:, 0])]
    assert len(np.unique(to_a)) == n
    assert np.array_equal(p["counts"][:, 1:7], a["counts"][to_a][:, 1:7])
    for c in range(n):
        mine = old[p["rim_start"][c]:p["rim_start"][c + 1]]
        theirs = a["rim_edge"][a["rim_start"][to_a[c]]:a["rim_start"][to_a[c] + 1]].astype(np.int64)
        assert theirs.min() == a["counts"][to_a[c], 0]
        if p["counts"][c, 6] >= 1:
            k = int(np.nonzero(mine == theirs[0])[0][0])
            assert np.array_equal(np.roll(mine, -k), theirs)
        else:
            assert sorted(mine.tolist()) == theirs.tolist()
    assert (np.abs(p["sums"] - a["sums"][to_a]) <= factor * a["bound"][to_a]).all()
    if "verts" in a and len(a["added_bound"]):
        nv = len(C.case(name)[0])
        fa, fp = a["counts"][to_a][:, 7], p["counts"][:, 7]
        assert np.array_equal(fa >= 0, fp >= 0)
        va, vp = a["verts"][fa[fa >= 0]].astype(np.float64), p["verts"][fp[fp >= 0]].astype(np.float64)
        assert (np.abs(va - vp) <= factor * a["added_bound"][fa[fa >= 0] - nv]).all()
    return True


@pytest.mark.parametrize("name", C.VARIED)
@pytest.mark.parametrize("variant", C.VARIANTS[1:])
def test_rims_follow_permuted_triangles_and_rotated_corners(name, variant):
    assert follows_variant(name, variant, ref(name), ref(name, variant))


def test_restatement_on_the_named_cases():
    """hand answers"""
    t = lambda name, fill=-1: ref(name, None, fill)["totals"].tolist()   # noqa: E731
    assert t("empty") == [0] * 8 and t("all_collapsed") == [0, 0, 4, 0, 0, 0, 0, 0] and t("tetrahedron") == [0] * 8
    r = ref("one_triangle")                           # its rim of 3 is filled by its reverse
    assert r["rim_edge"].tolist() == [0, 1, 2] and r["counts"].tolist() == [[0, 3, 3, 0, 0, 0, 2, -1]]
    assert r["tris"].tolist() == [[0, 1, 2], [1, 0, 2]] and len(r["verts"]) == 3
    V = C.case("one_triangle")[0].astype(np.float64)  # the reference point is the box centre (0.5, 0.5, 0.25)
    assert r["ref_point"].tolist() == [0.5, 0.5, 0.25]
    per = sum(np.linalg.norm(V[b] - V[a]) for a, b in ((0, 1), (1, 2), (2, 0)))
    assert abs(r["sums"][0, 0] - per) < 1e-15 and r["exact_sums"][0][4:] == [Fraction(-1, 2), Fraction(-1, 2), Fraction(-1, 4)]
    n2 = np.cross(V[1] - V[0], V[2] - V[0])           # sum A x B of a closed rim is twice its vector area
    assert np.allclose(r["sums"][0, 1:4], n2, atol=1e-15)
    r = ref("tet_minus_face")                         # closed again with no new vertex
    assert r["counts"][0, 6] == 2 and len(r["verts"]) == 4 and M.topology(r["tris"])[2][4:7].tolist() == [0, 0, 0]
    for name, centre in (("cube_minus_face", [0.5, 0.5, 0.0]), ("cube_far", None)):
        r = ref(name)
        V, T = C.case(name)
        assert r["totals"].tolist() == [1, 4, 0, 4, 0, 1, 1, 4] and r["counts"][0, 6:].tolist() == [3, 8]
        lo = V.astype(np.float64).min(0)
        side = V.astype(np.float64)[:, 0].max() - lo[0]
        want = np.float32(np.array([lo[0] + side / 2, lo[1] + side / 2, lo[2]]))
        if centre is not None:
            assert r["verts"][8].tolist() == centre   # exactly
        assert np.abs(r["verts"][8] - want).max() <= 2.0 ** -23 * 1000.1
        assert abs(0.5 * np.linalg.norm(r["sums"][0, 1:4]) - side * side) <= 1e-12 and abs(r["sums"][0, 0] - 4 * side) <= 1e-12
        s = M.shells(r["verts"], r["tris"])
        assert s["totals"][4:7].tolist() == [0, 0, 0] and abs(s["sums"][0, 1] - side ** 3) <= s["bound"][0, 1]
    # selection: the tube's two rims of 8 and the cube's rim of 4
    assert t("tube_and_cube", None)[5:] == [3, 0, 0] and t("tube_and_cube", 0)[5:] == [3, 0, 0]
    assert t("tube_and_cube", 4)[5:] == [3, 1, 4] and t("tube_and_cube", 8)[5:] == [3, 3, 20] and t("tube_and_cube", -1)[5:] == [3, 3, 20]
    assert ref("tube_and_cube", None, 4)["counts"][:, 6].tolist() == [1, 1, 3] and ref("tube_and_cube", None, None)["counts"][:, 6].tolist() == [1] * 3
    assert np.array_equal(ref("tube_and_cube", None, 0)["tris"], C.case("tube_and_cube")[1])
    # nodes that block the fill
    for name in ("bowtie", "ico_touching_holes"):
        r = ref(name)
        V, T = C.case(name)
        assert r["counts"][0, 1:].tolist() == [6, 5, 0, 0, 1, 0, -1] and np.array_equal(r["tris"], T)
        f = F.fans(V, T)                              # the fans' split makes the node regular
        r2 = R.holes(f["verts"], f["tris"], fill=-1)
        if name == "bowtie":
            assert r2["counts"][:, 1:7].tolist() == [[3, 3, 0, 0, 0, 2]] * 2
        else:                                         # the two holes have become one hole of 6 edges through both copies
            assert r2["counts"][:, 1:].tolist() == [[6, 6, 0, 0, 0, 3, len(f["verts"])]]
        assert M.topology(r2["tris"])[2][4] == 0
    assert ref("strip_one_reversed")["counts"][0, 3:7].tolist() == [0, 2, 0, 0] and t("strip_one_reversed")[5:] == [0, 0, 0]
    r = ref("moebius")                                # one rim of 18 edges; the seam leaves flipped nodes
    assert r["counts"][0, 1] == 18 and r["counts"][0, 4] == 2 and r["counts"][0, 6] == 0
    assert ref("fin")["counts"][0, 1:7].tolist() == [2, 3, 2, 0, 0, 0]
    assert ref("three_on_edge")["counts"][0, 1:7].tolist() == [6, 5, 0, 0, 2, 0]
    r = ref("degenerate_mixed")
    assert r["totals"].tolist() == [1, 4, 4, 4, 0, 1, 1, 4] and r["counts"][0, 7] == 11 and len(r["tris"]) == 18
    for n in (255, 256, 257, 16385):
        r = ref(f"disk{n}")
        assert r["counts"].tolist() == [[1, n, n, 0, 0, 0, 3, n + 1]] and r["rim_edge"].tolist() == [1 + 3 * ((k) % n) for k in range(n)]
    r = ref("ico_many_holes")
    assert r["totals"].tolist() == [250, 900, 0, 900, 0, 250, 250, 500] and sorted(set(r["counts"][:, 1].tolist())) == [3, 6]
    assert M.topology(r["tris"])[2][[0, 4, 5, 6]].tolist() == [1, 0, 0, 0]
    assert ref("sphere33_holes")["totals"][[0, 5, 6]].tolist() == [40, 40, 40]
    assert ref("gyroid17")["totals"][[0, 1, 5]].tolist() == [4, 369, 4]               # the rims at the lattice border
    print(f"largest fraction of the added-vertex bound used by the restatement: {R.worst_vertex_fraction:.3f}")


# ---- the library without a device -----------------------------------------------------------------------------------------

def test_symbols_and_exports(pkg):
    lib = pkg._lib.lib()
    for s in ("r2s_mesh_holes", "r2s_last_mesh_holes", "r2s_mesh_holes_dev"):
        assert hasattr(lib, s) and [x[0] for x in pkg._lib.SYMBOLS].count(s) == 1
    for name in ("MeshHoles", "mesh_holes", "mesh_holes_dev"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def _call(pkg, V, T, nv=None, nt=None, dev=False, null=(), vcap=None, tcap=None, alias=None, rcap=0, ecap=0):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs (dev: host memory as "device" pointers - every call
    here is refused before anything reads them).  null: the arguments passed as NULL; alias: the output given the address of
    the input triangles"""
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    vcap, tcap = len(v) + 8 if vcap is None else vcap, len(t) + 8 if tcap is None else tcap
    to, vo = np.full((len(t) + 9, 3), -7, np.int32), np.full((len(v) + 9, 3), -7.0, np.float32)
    start, cnt, sums, edge = np.full(9, -7, np.int64), np.full((8, 8), -7, np.int64), np.full((8, 7), -7.0), np.full(64, -7, np.int32)
    sc = [ctypes.c_int64(-7) for _ in range(4)]
    r, tot = np.full(3, -7.0), np.full(8, -7, np.int64)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    arr = dict(verts=v, tris=t, to=to, vo=vo, start=start, cnt=cnt, sums=sums, edge=edge)
    if alias:
        arr[alias] = t
    tail = [None if f"s{k}" in null else ctypes.byref(sc[k]) for k in range(4)]
    tail += [None if "r" in null else r.ctypes.data_as(L.c_double_p), None if "tot" in null else tot.ctypes.data_as(L.c_int64_p)]
    if dev:
        p = lambda k: None if k in null else arr[k].ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        rc = L.lib().r2s_mesh_holes_dev(p("verts"), nv, p("tris"), nt, -1, p("start"), p("cnt"), p("sums"), rcap, p("edge"), ecap, p("to"),
                                        p("vo"), vcap, tcap, *tail, None)
    else:
        ip = lambda k: None if k in null else arr[k].ctypes.data_as(L.c_int32_p)   # noqa: E731
        fp = lambda k: None if k in null else arr[k].ctypes.data_as(L.c_float_p)   # noqa: E731
        rc = L.lib().r2s_mesh_holes(fp("verts"), nv, ip("tris"), nt, -1, -1, ip("to"), fp("vo"), vcap, tcap, *tail)
    clean = all((x == -7).all() for x in (to, vo, start, cnt, sums, edge, r, tot)) and all(s.value == -7 for s in sc)
    return rc, bool(clean) and np.array_equal(t, np.ascontiguousarray(T, np.int32).reshape(-1, 3))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_before_any_device_work(pkg, dev):
    V, T = C.case("cube_minus_face")
    assert _call(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _call(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    for null in (("verts",), ("tris",), ("s0",), ("s1",), ("s2",), ("s3",), ("r",), ("tot",)):   # NULL arrays with a count, NULL scalars
        assert _call(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    for null in (("vo",), ("to",)):                                                   # tris_out without verts_out, and back
        assert _call(pkg, V, T, dev=dev, null=null) == (ARG, True), null
        assert "together" in pkg._lib.lib().r2s_last_error().decode()
    assert _call(pkg, V, T, dev=dev, vcap=-1) == (ARG, True) and _call(pkg, V, T, dev=dev, tcap=-1) == (ARG, True)
    assert _call(pkg, V, T, dev=dev, alias="to") == (ARG, True)                       # an output overlapping an input
    assert "overlaps" in pkg._lib.lib().r2s_last_error().decode()
    if dev:
        assert _call(pkg, V, T, dev=True, rcap=-1) == (ARG, True) and _call(pkg, V, T, dev=True, ecap=-1) == (ARG, True)
        for null in (("start",), ("cnt",), ("sums",)):
            assert _call(pkg, V, T, dev=True, rcap=4, null=null) == (ARG, True)
        assert _call(pkg, V, T, dev=True, ecap=4, null=("edge",)) == (ARG, True)
        assert _call(pkg, V, T, dev=True, ecap=30, alias="edge") == (ARG, True)
        assert "overlaps" in pkg._lib.lib().r2s_last_error().decode()
    assert _call(pkg, V, T, nt=TOO_MANY_TRIS, dev=dev) == (UNSUPPORTED, True)        # refused before anything is read
    assert "2^31" in pkg._lib.lib().r2s_last_error().decode()
    assert _call(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    lib = pkg._lib.lib()
    n, m = ctypes.c_int64(), ctypes.c_int64()
    assert lib.r2s_last_mesh_holes(None, None, None, 4, None, 0, ctypes.byref(n), ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_holes(None, None, None, 0, None, 4, ctypes.byref(n), ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_holes(None, None, None, 0, None, 0, None, ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_holes(None, None, None, -1, None, 0, ctypes.byref(n), ctypes.byref(m)) == ARG


def test_host_mesh_check_comes_before_the_device(pkg):
    V, T = C.case("cube_minus_face")
    T2, V2, V3 = T.copy(), V.copy(), V.copy()
    T2[5, 1], V2[3, 2], V3[0, 0] = len(V), np.nan, np.inf
    for v, t in ((V, T2), (V, T - 1), (V2, T), (V3, T)):
        assert _call(pkg, v, t) == (ARG, True)
        msg = pkg._lib.lib().r2s_last_error().decode()
        assert msg.startswith("mesh_holes:") and ("not finite" in msg or "outside" in msg)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = C.case("bowtie")
    assert _call(pkg, V, T) == (NO_DEVICE, True) and _call(pkg, V, T, dev=True) == (NO_DEVICE, True)
    with pytest.raises(pkg._lib.R2SError, match="error -2"):
        pkg.mesh_holes(V, T, fill=-1)


def test_import_stl_refuses_fill_holes_on_a_soup(pkg, tmp_path):
    with pytest.raises(pkg._lib.R2SError, match="fill_holes needs weld"):
        pkg.import_stl(str(tmp_path / "none.stl"), weld=False, fill_holes=-1)


def test_meshholes_derived_fields(pkg):
    """the host-side fields of the result class, on the restatement's tables"""
    for name in ("cube_minus_face", "tube_and_cube", "bowtie", "tetrahedron"):
        r = ref(name)
        h = pkg.MeshHoles(r["rim_start"], r["rim_edge"], r["counts"], r["sums"], r["ref_point"], r["totals"], r["verts"], r["tris"])
        assert h.n_rims == len(h) == r["totals"][0] and h.closed.sum() == r["totals"][5] and h.filled.sum() == r["totals"][6]
        assert h.watertight == (name == "tetrahedron") and np.array_equal(h.n_edges, r["counts"][:, 1])
    r = ref("cube_minus_face")
    h = pkg.MeshHoles(r["rim_start"], r["rim_edge"], r["counts"], r["sums"], r["ref_point"], r["totals"])
    assert np.allclose(h.area, [1.0]) and np.allclose(h.length, [4.0]) and np.allclose(h.centroid, [[0.5, 0.5, 0.0]])


# ---- the Julia binding against the header --------------------------------------------------------------------------------

def test_ccall_type_tuples_match_the_header():
    to_julia = dict(C_TO_JULIA, **{"float *": {"Ptr{Float32}", "Ptr{Cvoid}"}})
    src = open(JULIA).read()
    for name in ("r2s_mesh_holes", "r2s_last_mesh_holes", "r2s_mesh_holes_dev"):
        c = _c_params(name)
        calls = _ccalls(src, name)
        assert calls, f"{name}: no ccall in {os.path.basename(JULIA)}"
        for types in calls:
            assert len(types) == len(c), (name, types, c)
            for jt, ct in zip(types, c):
                assert jt in to_julia[ct], (name, jt, ct)
                if name != "r2s_mesh_holes_dev":
                    assert jt != "Ptr{Cvoid}", (name, jt, ct)   # the host variants use typed pointers
    assert "mesh_holes_hip" in src and "mesh_holes" in open(INTEGRATION).read()
