"""CPU-side checks of the self-intersection feature (include/rho2sdf_hip.h, r2s_mesh_index_intersections): the numpy restatement
(tests/mesh_intersect_ref.py) gives the known answers of the named cases, agrees with exact arithmetic wherever that decides with
a margin, follows a permutation of the triangles, and the library exports the entry points and refuses to run without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import mesh_intersect_cases as C
import mesh_intersect_ref as R

# totals[0..5] of the restatement: intersecting pairs, triangles involved, candidates, adjacent, one shared index, collapsed
KNOWN = {
    "empty": (0, 0, 0, 0, 0, 0), "one_triangle": (0, 0, 0, 0, 0, 0), "two_far": (0, 0, 0, 0, 0, 0),
    "piercing": (1, 2, 1, 0, 0, 0), "boxes_only": (0, 0, 1, 0, 0, 0), "folded_edge_pair": (0, 0, 1, 1, 0, 0),
    "duplicate": (0, 0, 1, 1, 0, 0), "vertex_pair_clear": (0, 0, 1, 0, 1, 0), "vertex_pair_piercing": (1, 2, 1, 0, 1, 0),
    "coplanar_overlap": (0, 0, 1, 0, 0, 0), "t_junction": (1, 2, 1, 0, 0, 0), "with_collapsed": (1, 2, 1, 0, 0, 1),
    "zero_area": (1, 2, 1, 0, 0, 0), "tetrahedron": (0, 0, 6, 6, 0, 0), "cube": (0, 0, 54, 18, 30, 0),
    "tetrahedron_soup": (6, 4, 6, 0, 0, 0), "two_tetrahedra": (3, 4, 16, 12, 0, 0), "two_cubes": (18, 12, 132, 36, 60, 0),
    "random63": (23, 32, 106, 0, 0, 0), "random64": (17, 25, 101, 0, 0, 0), "random65": (11, 18, 99, 0, 0, 0),
    "random200": (157, 145, 1023, 0, 0, 0), "random200_far": (156, 144, 1023, 0, 0, 0), "deep": (10094, 150, 11175, 0, 0, 0),
}


@pytest.mark.parametrize("name", C.ALL)
def test_known_answers(name):
    V, T = C.case(name)
    pairs, hits, tot = C.expected(name)
    assert pairs.dtype == np.int32 and hits.dtype == np.int32 and tot.dtype == np.int64 and tot.shape == (8,)
    assert pairs.shape == (tot[0], 2) and hits.shape == (len(T),) and tot[6] == 0 and tot[7] == 0
    assert (pairs[:, 0] < pairs[:, 1]).all() and hits.sum() == 2 * tot[0] and (hits > 0).sum() == tot[1]
    key = pairs[:, 0].astype(np.int64) * max(len(T), 1) + pairs[:, 1]
    assert (np.diff(key) > 0).all()
    if name in KNOWN:
        assert tuple(int(x) for x in tot[:6]) == KNOWN[name]
    if name == "sphere17":                                 # a closed surface over the lattice: clean, and really a mesh
        assert tot[0] == 0 and tot[5] == 0 and len(T) > 1000 and tot[3] == 3 * len(T) // 2
    if name == "two_spheres":                              # an intersection curve between the two copies, and only there
        n = len(T) // 2
        assert tot[0] > 100 and (pairs[:, 0] < n).all() and (pairs[:, 1] >= n).all()
    if name == "tetrahedron_soup":                         # every neighbour of every triangle
        assert pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    if name == "two_cubes":
        assert (pairs[:, 0] < 12).all() and (pairs[:, 1] >= 12).all()


@pytest.mark.parametrize("name", ["random63", "random64", "random65", "random200", "two_spheres"])
def test_restatement_against_exact_arithmetic(name):
    """Every candidate pair that exact arithmetic decides with the margin 2^-40 (a proper crossing of the open triangle, or
    strictly clear) is classified the same way by the restatement; the pairs left out number at most 0.1 % of the candidates."""
    V, T = C.case(name)
    pairs, _, tot = C.expected(name)
    got = set(map(tuple, pairs.tolist()))
    S, Tt, verdict = R.pairs_exact(V, T)
    assert len(verdict) == tot[2] - tot[3]
    undecided = sum(v is None for v in verdict)
    wrong = [(int(s), int(t), v) for s, t, v in zip(S, Tt, verdict) if v is not None and ((int(s), int(t)) in got) != v]
    print(f"INTERSECT exact {name}: {len(verdict)} pairs tested, {undecided} undecided (cap {tot[2] // 1000}), {len(wrong)} differ")
    assert not wrong, wrong[:10]
    assert 1000 * undecided <= tot[2]
    assert sum(v is True for v in verdict) > 10


def test_permutation():
    V, T = C.case("random200")
    pairs, hits, tot = C.expected("random200")
    perm = np.random.default_rng(5).permutation(len(T))   # new triangle k is the old triangle perm[k]
    p2, h2, t2 = R.intersections(V, T[perm])
    back = np.sort(perm[p2], axis=1)
    back = back[np.lexsort((back[:, 1], back[:, 0]))]
    assert np.array_equal(back, pairs) and np.array_equal(t2, tot)
    assert np.array_equal(h2, hits[perm])


NAMES = ("r2s_mesh_index_intersections", "r2s_mesh_index_intersections_dev", "r2s_mesh_intersections", "r2s_mesh_intersections_dev")


def test_abi_symbols(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    bound = {name for name, _, _ in pkg._lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name) and name in bound
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rho2sdf_hip.h")).read()
    for name in NAMES:
        assert name + "(" in hdr


def test_abi_null_totals(pkg):
    """a NULL totals is R2S_ERR_ARG, with or without a device"""
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("piercing")
    pv, pt = V.ctypes.data_as(L.c_float_p), T.ctypes.data_as(L.c_int32_p)
    assert lib.r2s_mesh_intersections(pv, len(V), pt, len(T), -1, None, None, 0, None) == -1
    assert lib.r2s_mesh_intersections_dev(None, 0, None, 0, None, None, 0, None, None) == -1
    tot = np.full(8, -7, np.int64)
    ptot = tot.ctypes.data_as(L.c_int64_p)
    assert lib.r2s_mesh_index_intersections(None, None, None, 0, ptot) == -1          # a NULL index
    assert lib.r2s_mesh_index_intersections_dev(None, None, None, 0, ptot, None) == -1
    assert lib.r2s_mesh_intersections(pv, len(V), pt, len(T), -1, None, None, -1, ptot) == -1   # a negative capacity
    assert lib.r2s_mesh_intersections(pv, len(V), pt, len(T), -1, None, None, 2, ptot) == -1    # NULL pairs with a capacity
    assert (tot == -7).all()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_abi_no_device(pkg):
    """without a GPU the calls fail loudly with R2S_ERR_NO_DEVICE and touch nothing"""
    L, lib = pkg._lib, pkg._lib.lib()
    V, T = C.case("piercing")
    tot, hits = np.full(8, -7, np.int64), np.full(len(T), -7, np.int32)
    pv, pt, ptot = V.ctypes.data_as(L.c_float_p), T.ctypes.data_as(L.c_int32_p), tot.ctypes.data_as(L.c_int64_p)
    assert lib.r2s_mesh_intersections(pv, len(V), pt, len(T), -1, hits.ctypes.data_as(L.c_int32_p), None, 0, ptot) == -2
    assert lib.r2s_mesh_intersections_dev(ctypes.c_void_p(V.ctypes.data), len(V), ctypes.c_void_p(T.ctypes.data), len(T), None, None, 0,
                                          ptot, None) == -2
    assert (tot == -7).all() and (hits == -7).all()
    with pytest.raises(L.R2SError, match="no HIP device|CPU fallback"):
        pkg.mesh_intersections(V, T)
