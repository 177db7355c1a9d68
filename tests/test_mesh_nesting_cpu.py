"""Host-side parts of the mesh nesting (no GPU): the restatement of tests/mesh_nesting_ref.py held to the forest every constructed
case of tests/mesh_nesting_cases.py carries from its construction, under all six rays, with 30 % of the triangles reversed and
with the triangles permuted; the rounding limit of the tie rule on the samples of every case; the refusals of r2s_mesh_nesting
that come before any device work; the result class; the exported symbols and the Julia ccall tuples.  (The refusal of an index
of another triangle count needs an index, hence a device: tests/test_mesh_nesting_gpu.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_nesting_cases as C
import mesh_nesting_ref as R
import mesh_winding_ref as W
from test_mesh_orient_cpu import C_TO_JULIA, HEADER, INTEGRATION, JULIA, _c_params, _ccalls

ARG, UNSUPPORTED, NO_DEVICE = -1, -4, -2

_pre, _ref = {}, {}


def pre(name):
    if name not in _pre:
        _pre[name] = R.patches(*C.case(name))
    return _pre[name]


def ref(name, ray, flags=0):
    """the restatement of a case, computed once and left unchanged"""
    if (name, ray, flags) not in _ref:
        _ref[(name, ray, flags)] = R.nesting(*C.case(name), ray=ray, flags=flags, pre=pre(name))
    return _ref[(name, ray, flags)]


def expect_counts(e, first, n_tris):
    depth, parent, irregular = C.forest(e["containers"])
    n = len(depth)
    cnt = np.zeros((n, 5), np.int64)
    cnt[:, 0], cnt[:, 1], cnt[:, 2] = first, n_tris, 1 * e["closed"] + 4 * irregular
    cnt[:, 3], cnt[:, 4] = parent, depth
    return cnt, np.bincount(parent[parent >= 0], minlength=n)


def check_against_construction(r, e, T):
    """the restated result r of the triangles T against the expectation e of the construction"""
    pot = e["patch_of_tri"]
    n = len(e["containers"])
    first = np.array([np.nonzero(pot == p)[0].min() for p in range(n)], np.int64).reshape(n)
    assert (np.diff(first) > 0).all()
    cnt, children = expect_counts(e, first, np.bincount(pot[pot >= 0], minlength=n))
    assert np.array_equal(r["patch_of_tri"], pot)
    assert np.array_equal(r["counts"][:, :5], cnt) and np.array_equal(r["counts"][:, 5], children) and (r["counts"][:, 7] == 0).all()
    pairs = sorted((p << 32) | q for p in range(n) for q in e["containers"][p])
    assert r["pairs"].tolist() == pairs
    depth = cnt[:, 4]
    assert r["totals"].tolist() == [n, len(T), int((pot < 0).sum()), int(e["closed"].sum()), len(pairs), int(depth.max()) if n else 0,
                                    int((cnt[:, 2] & 4 != 0).sum()), 0]
    # the sum of the crossings: at least one per container, and of the container's parity
    for p in range(n):
        assert r["counts"][p, 6] == sum(k for (a, _), k in r["cross"].items() if a == p)
    assert all((k % 2 == 1) == (q in e["containers"][p]) for (p, q), k in r["cross"].items())


@pytest.mark.parametrize("name", ("empty",) + tuple(C.BUILT))
def test_restatement_against_construction(name):
    V, T = C.case(name)
    e = C.built(name)
    for ray in W.RAYS:
        check_against_construction(ref(name, ray), e, T)
    # 30 % of the triangles reversed: no winding is read
    Tr = C.reversed_some(T)
    for ray in W.RAYS:
        r = R.nesting(V, Tr, ray=ray)
        check_against_construction(r, e, Tr)
    # the triangles permuted: everything follows, through the renumbering of the patches
    perm = np.random.default_rng(7).permutation(len(T))
    Tp, pot = np.ascontiguousarray(T[perm]), e["patch_of_tri"][perm]
    n = len(e["containers"])
    first = np.array([np.nonzero(pot == p)[0].min() for p in range(n)], np.int64).reshape(n)
    new_of = np.empty(n, np.int64)
    new_of[np.argsort(first)] = np.arange(n)           # old patch number -> new patch number
    ep = dict(patch_of_tri=np.where(pot >= 0, new_of[np.maximum(pot, 0)], -1).astype(np.int32), closed=np.empty(n, bool),
              containers=[None] * n)
    for p in range(n):
        ep["closed"][new_of[p]] = e["closed"][p]
        ep["containers"][new_of[p]] = {int(new_of[q]) for q in e["containers"][p]}
    for ray in (0, 5):
        # (corner 0 of a patch's first triangle moves with the permutation: the forest must not)
        check_against_construction(R.nesting(V, Tp, ray=ray), ep, Tp)


def test_restatement_on_the_named_cases():
    """the figures the case descriptions promise"""
    assert ref("empty", 2)["totals"].tolist() == [0] * 8
    assert ref("one_triangle", 2)["counts"].tolist() == [[0, 1, 0, -1, 0, 0, 0, 0]]
    assert ref("tetrahedron", 2)["counts"].tolist() == [[0, 4, 1, -1, 0, 0, 0, 0]]
    r = ref("beside", 3)                              # the -x ray crosses the neighbour twice
    assert r["cross"] == {(1, 0): 2} and r["counts"][1].tolist() == [12, 12, 1, -1, 0, 0, 2, 0] and r["totals"][4] == 0
    assert ref("chain3", 1)["counts"][:, 3:6].tolist() == [[-1, 0, 1], [0, 1, 1], [1, 2, 0]]
    assert ref("siblings", 4)["counts"][:, 3:6].tolist() == [[-1, 0, 2], [0, 1, 0], [0, 1, 0]]
    assert ref("open_query", 0)["counts"][:, 2:5].tolist() == [[1, -1, 0], [0, 0, 1]]
    assert ref("open_container", 0)["totals"][3:7].tolist() == [1, 0, 0, 0]
    assert ref("shared_edge", 2)["totals"][[0, 3, 4]].tolist() == [3, 1, 0]
    assert ref("collapsed_mixed", 2)["totals"][:5].tolist() == [2, 28, 4, 2, 1]
    r = ref("interpenetrating", 2)
    assert r["counts"][2, 2:6].tolist() == [1 | 4, 0, 2, 0] and r["totals"][4:7].tolist() == [2, 2, 1]
    r = ref("chain70", 0)
    assert r["totals"].tolist() == [70, 840, 0, 70, 69 * 70 // 2, 69, 0, 0] and r["counts"][:, 3].tolist() == list(range(-1, 69))
    for n in (255, 256, 257):
        r = ref(f"scatter{n}", 3)
        assert r["totals"][0] == n + 2 and set(r["counts"][2:, 4].tolist()) == {0, 1, 2} and r["totals"][6] == 0
    assert ref("ico_around", 1)["counts"][0, 5] == 40
    r = ref("hollow21", 2)
    assert r["totals"][[0, 3, 4, 5]].tolist() == [2, 2, 1, 1] and r["pairs"].tolist() == [(1 << 32) | 0]
    for ray in (0, 5):                                # small bodies beside each other: crossings in pairs, nothing nested
        r = ref("noise17", ray)
        assert r["totals"].tolist() == [308, 5116, 0, 308, 0, 0, 0, 0] and r["counts"][:, 6].sum() > 0


@pytest.mark.parametrize("name", ("nested2", "void_island", "collapsed_mixed", "siblings", "hollow21"))
def test_rewind(name):
    V, T = C.case(name)
    plain, r = ref(name, 2), ref(name, 2, R.REWIND)
    assert np.array_equal(r["counts"][:, [0, 1, 3, 4, 5, 6, 7]], plain["counts"][:, [0, 1, 3, 4, 5, 6, 7]]) and plain["tris"] is None
    odd = (r["counts"][:, 2] & 1 != 0) & (r["counts"][:, 4] % 2 == 1)
    assert np.array_equal(r["counts"][:, 2], plain["counts"][:, 2] | 2 * odd) and r["totals"][7] == r["counts"][odd, 1].sum() > 0
    pot = r["patch_of_tri"]
    rev = (pot >= 0) & np.concatenate([odd, [False]])[pot]
    assert np.array_equal(r["tris"][~rev], T[~rev]) and np.array_equal(r["tris"][rev], T[rev][:, [0, 2, 1]])
    # relative to the input: the same patches, samples and forest, so a second pass reverses the same triangles again
    again = R.nesting(V, r["tris"], ray=2, flags=R.REWIND)
    assert np.array_equal(again["tris"], T) and np.array_equal(again["counts"], r["counts"])


@pytest.mark.parametrize("name", C.ALL)
def test_rounding_limit_is_not_met_on_the_samples(name):
    """on the samples of every case no computed effective sign or verdict differs from the exact one: the restatement alone is
    the truth of these cases"""
    V, T = C.case(name)
    S = pre(name)["samples"]
    for ray in W.RAYS:
        assert W.exact_disagreements(V, T, S, ray)[1] == 0, ray


# ---- the library without a device -----------------------------------------------------------------------------------------

def test_symbols_and_exports(pkg):
    lib = pkg._lib.lib()
    for s in ("r2s_mesh_nesting", "r2s_last_mesh_nesting", "r2s_mesh_nesting_dev"):
        assert hasattr(lib, s) and [x[0] for x in pkg._lib.SYMBOLS].count(s) == 1
    for name in ("MeshNesting", "mesh_nesting", "mesh_nesting_dev"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg._lib.NESTING_REWIND == 1 and re.search(r"#define R2S_NESTING_REWIND 1\b", open(HEADER).read())


def _call(pkg, V, T, ray=2, flags=0, nv=None, nt=None, dev=False, null=(), alias=False, cap=0, pcap=0):
    """-> (rc, outputs untouched?) of one raw call with poisoned outputs (dev: host memory as "device" pointers - every call
    here is refused before anything reads them).  null: the arguments passed as NULL; alias: tris_out is the input triangles"""
    L = pkg._lib
    v, t = np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(T, np.int32).reshape(-1, 3)
    keep = t.copy()
    out, pot = np.full((len(t) + 1, 3), -7, np.int32), np.full(len(t) + 1, -7, np.int32)
    cnt, prs = np.full((8, 8), -7, np.int64), np.full(8, -7, np.int64)
    n, m, tot = ctypes.c_int64(-7), ctypes.c_int64(-7), np.full(8, -7, np.int64)
    nv, nt = len(v) if nv is None else nv, len(t) if nt is None else nt
    arr = dict(verts=v, tris=t, out=t if alias else out, pot=pot, cnt=cnt, prs=prs)
    pn, pm = None if "n" in null else ctypes.byref(n), None if "m" in null else ctypes.byref(m)
    ptot = None if "tot" in null else tot.ctypes.data_as(L.c_int64_p)
    if dev:
        p = lambda k: None if k in null else arr[k].ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        rc = L.lib().r2s_mesh_nesting_dev(None, p("verts"), nv, p("tris"), nt, ray, flags, p("out"), p("pot"), p("cnt"), cap, p("prs"), pcap,
                                          pn, pm, ptot, None)
    else:
        ip = lambda k: None if k in null else arr[k].ctypes.data_as(L.c_int32_p)   # noqa: E731
        rc = L.lib().r2s_mesh_nesting(None if "verts" in null else v.ctypes.data_as(L.c_float_p), nv, ip("tris"), nt, ray, flags, -1,
                                      ip("out"), ip("pot"), pn, ptot)
    clean = all((x == -7).all() for x in (out, pot, cnt, prs, tot)) and n.value == -7 and m.value == -7 and np.array_equal(t, keep)
    return rc, bool(clean)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_refusals_before_any_device_work(pkg, dev):
    V, T = C.case("nested2")
    err = lambda: pkg._lib.lib().r2s_last_error().decode()   # noqa: E731
    assert _call(pkg, V, T, nv=-1, dev=dev) == (ARG, True) and _call(pkg, V, T, nt=-1, dev=dev) == (ARG, True)
    for null in (("verts",), ("tris",), ("n",), ("tot",)) + ((("m",),) if dev else ()):   # NULL arrays with a count, NULL scalars
        assert _call(pkg, V, T, dev=dev, null=null) == (ARG, True), null
    for ray in (-1, 6, 1 << 20):
        assert _call(pkg, V, T, ray=ray, dev=dev) == (ARG, True) and "ray" in err()
    for flags in (2, 3, -1, 1 << 20):
        assert _call(pkg, V, T, flags=flags, dev=dev) == (ARG, True) and "flag" in err()
    assert _call(pkg, V, T, flags=1, dev=dev, null=("out",)) == (ARG, True) and "tris_out" in err()   # REWIND without tris_out
    assert _call(pkg, V, T, flags=1, dev=dev, alias=True) == (ARG, True) and "overlaps" in err()
    if dev:
        assert _call(pkg, V, T, dev=True, cap=-1) == (ARG, True) and _call(pkg, V, T, dev=True, pcap=-1) == (ARG, True)
        assert _call(pkg, V, T, dev=True, cap=4, null=("cnt",)) == (ARG, True) and _call(pkg, V, T, dev=True, pcap=4, null=("prs",)) == (ARG, True)
    assert _call(pkg, V, T, nt=2 ** 30 + 1, dev=dev) == (UNSUPPORTED, True) and "2^30" in err()   # refused before anything is read
    assert _call(pkg, V, T, nv=2 ** 31, dev=dev) == (UNSUPPORTED, True)
    lib = pkg._lib.lib()
    n, m = ctypes.c_int64(), ctypes.c_int64()
    assert lib.r2s_last_mesh_nesting(None, 4, None, 0, ctypes.byref(n), ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_nesting(None, 0, None, 4, ctypes.byref(n), ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_nesting(None, -1, None, 0, ctypes.byref(n), ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_nesting(None, 0, None, -1, ctypes.byref(n), ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_nesting(None, 0, None, 0, None, ctypes.byref(m)) == ARG
    assert lib.r2s_last_mesh_nesting(None, 0, None, 0, ctypes.byref(n), None) == ARG


def test_host_mesh_check_comes_before_the_device(pkg):
    V, T = C.case("nested2")
    T2, V2, V3 = T.copy(), V.copy(), V.copy()
    T2[7, 1], V2[3, 2], V3[0, 0] = len(V), np.nan, np.inf
    for v, t in ((V, T2), (V, T - 1), (V2, T), (V3, T)):
        assert _call(pkg, v, t, flags=1) == (ARG, True)
        msg = pkg._lib.lib().r2s_last_error().decode()
        assert msg.startswith("mesh_nesting:") and ("not finite" in msg or "outside" in msg)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = C.case("tetrahedron")
    assert _call(pkg, V, T, flags=1) == (NO_DEVICE, True) and _call(pkg, V, T, flags=1, dev=True) == (NO_DEVICE, True)
    with pytest.raises(pkg._lib.R2SError, match="error -2"):
        pkg.mesh_nesting(V, T)


def test_python_argument_errors(pkg, tmp_path):
    V, T = C.case("tetrahedron")
    for ray in (-1, 6, 2.0, "z", True):
        with pytest.raises(pkg._lib.R2SError, match="ray must be"):
            pkg.mesh_nesting(V, T, ray=ray)
    with pytest.raises(pkg._lib.R2SError, match="orient needs weld"):
        pkg.import_stl(str(tmp_path / "none.stl"), weld=False, orient="nested")
    with pytest.raises(pkg._lib.R2SError, match="orient must be"):
        pkg.import_stl(str(tmp_path / "none.stl"), orient="inward")


def test_meshnesting_derived_fields(pkg):
    """the host-side fields of the result class, on the restatement's tables"""
    r = ref("void_island", 2, R.REWIND)
    m = pkg.MeshNesting(r["tris"], r["patch_of_tri"], r["counts"], r["pairs"], r["totals"])
    assert len(m) == m.n_patches == 3 and m.parent.tolist() == [-1, 0, 1] and m.depth.tolist() == [0, 1, 2]
    assert m.closed.all() and not m.irregular.any() and m.reversed.tolist() == [False, True, False]
    assert m.roots.tolist() == [0] and m.voids.tolist() == [1] and m.bodies.tolist() == [0, 2]
    assert m.children(0).tolist() == [1] and m.children(1).tolist() == [2] and m.children(2).tolist() == []
    assert m.first_tri.tolist() == [0, 12, 24] and m.n_tris.tolist() == [12] * 3 and m.n_children.tolist() == [1, 1, 0]
    r = ref("siblings", 2)
    m = pkg.MeshNesting(None, r["patch_of_tri"], r["counts"], r["pairs"], r["totals"])
    assert m.children(0).tolist() == [1, 2] and m.voids.tolist() == [1, 2] and m.bodies.tolist() == [0] and m.tris is None
    r = ref("open_query", 2)
    m = pkg.MeshNesting(None, r["patch_of_tri"], r["counts"], r["pairs"], r["totals"])
    assert m.voids.tolist() == [] and m.bodies.tolist() == [0] and m.roots.tolist() == [0] and m.depth.tolist() == [0, 1]
    r = ref("interpenetrating", 2)
    m = pkg.MeshNesting(None, r["patch_of_tri"], r["counts"], r["pairs"], r["totals"])
    assert m.irregular.tolist() == [False, False, True] and m.parent.tolist() == [-1, -1, 0] and m.roots.tolist() == [0, 1]


# ---- the Julia binding against the header --------------------------------------------------------------------------------

def test_ccall_type_tuples_match_the_header():
    to_julia = dict(C_TO_JULIA, **{"const r2s_mesh_index *": {"Ptr{Cvoid}"}})
    src = open(JULIA).read()
    for name in ("r2s_mesh_nesting", "r2s_last_mesh_nesting", "r2s_mesh_nesting_dev"):
        c = _c_params(name)
        calls = _ccalls(src, name)
        assert calls, f"{name}: no ccall in {os.path.basename(JULIA)}"
        for types in calls:
            assert len(types) == len(c), (name, types, c)
            for jt, ct in zip(types, c):
                assert jt in to_julia[ct], (name, jt, ct)
                if name != "r2s_mesh_nesting_dev":
                    assert jt != "Ptr{Cvoid}", (name, jt, ct)   # the host variants use typed pointers
    assert "mesh_nesting_hip" in src and "NESTING_REWIND" in src and "mesh_nesting" in open(INTEGRATION).read()
