"""No GPU: the yardstick of tests/test_mesh_shells_gpu.py and the CPU side of the binding (include/rho2sdf_hip.h,
r2s_mesh_shells).  The restatement (mesh_shells_ref64) is checked against an exact evaluation of the same terms on every case
of mesh_shells_cases, under four summation orders, against its own bound; its partition and counts against iso_ref on the
extracted cases; the library's refusals that need no device return their codes; select_shells on hand-made input."""
import ctypes
import os

import mpmath
import numpy as np
import pytest

import iso_ref as R
import mesh_shells_cases as C
import mesh_shells_ref64 as M

ARG, NO_DEVICE, UNSUPPORTED = -1, -2, -4


def _exact_sums(V, T, r, shell, n):
    """Per shell the exact sums of the header's terms at 50 digits: the coordinates are scaled to integers (float32 and the
    double reference point are dyadic), the polynomial parts are formed exactly in integers, the square root of the area and
    the final quotients in mpmath at 50 digits."""
    mpmath.mp.dps = 50
    vals = [float(x) for x in np.asarray(V, np.float32).ravel()] + [float(x) for x in r]
    sh = max([0] + [d.bit_length() - 1 for d in (x.as_integer_ratio()[1] for x in vals)])
    toint = lambda x: (lambda p, q: p * ((1 << sh) // q))(*float(x).as_integer_ratio())   # noqa: E731
    Vi = np.array([toint(x) for x in np.asarray(V, np.float32).ravel()], dtype=object).reshape(-1, 3)
    ri = np.array([toint(x) for x in r], dtype=object)
    t = np.asarray(T).reshape(-1, 3)
    A, B, Cc = Vi[t[:, 0]] - ri, Vi[t[:, 1]] - ri, Vi[t[:, 2]] - ri
    S = A + B + Cc
    E, F = B - A, Cc - A
    x, y, z = 0, 1, 2
    N2 = (E[:, y] * F[:, z] - E[:, z] * F[:, y]) ** 2 + (E[:, z] * F[:, x] - E[:, x] * F[:, z]) ** 2 + (E[:, x] * F[:, y] - E[:, y] * F[:, x]) ** 2
    det = A[:, x] * (B[:, y] * Cc[:, z] - B[:, z] * Cc[:, y]) + A[:, y] * (B[:, z] * Cc[:, x] - B[:, x] * Cc[:, z]) \
        + A[:, z] * (B[:, x] * Cc[:, y] - B[:, y] * Cc[:, x])
    cols = [det] + [det * S[:, i] for i in range(3)] + [det * (A[:, i] * A[:, j] + B[:, i] * B[:, j] + Cc[:, i] * Cc[:, j] + S[:, i] * S[:, j])
                                                         for i, j in M.PAIRS]
    power = [3, 4, 4, 4, 5, 5, 5, 5, 5, 5]
    div = [6, 24, 24, 24, 120, 120, 120, 120, 120, 120]
    out = [[mpmath.mpf(0)] * 11 for _ in range(n)]
    two = mpmath.mpf(2)
    for s in range(n):
        idx = np.nonzero(shell == s)[0]
        out[s][0] = sum((mpmath.sqrt(mpmath.mpf(int(v))) for v in N2[idx]), mpmath.mpf(0)) / (2 * two ** (2 * sh))
        for q in range(10):
            out[s][1 + q] = mpmath.mpf(int(sum(cols[q][idx].tolist()))) / (div[q] * two ** (power[q] * sh))
    return out


def _pairwise(x):
    x = np.array(x)
    while len(x) > 1:
        if len(x) % 2:
            x = np.concatenate([x, np.zeros((1, x.shape[1]))])
        x = x[0::2] + x[1::2]
    return x[0]


def _orders(x, seed):
    seq = lambda a: np.cumsum(a, axis=0)[-1]   # noqa: E731
    return {"sequential": seq(x), "reversed": seq(x[::-1]), "shuffled": seq(x[np.random.default_rng(seed).permutation(len(x))]),
            "pairwise": _pairwise(x)}


@pytest.mark.parametrize("name", C.ALL)
def test_restatement_within_its_bound_under_four_summation_orders(name):
    V, T = C.case(name)
    r = M.shells(V, T)
    n = len(r["counts"])
    exact = _exact_sums(V, T, r["ref_point"], r["shell_of_tri"], n)
    worst = 0.0
    # the exact sums as unevaluated pairs of doubles: got - hi is exact for a got this close, so the error keeps 30 digits
    hi = np.array([[float(v) for v in row] for row in exact]).reshape(n, 11)
    lo = np.array([[float(v - mpmath.mpf(h)) for v, h in zip(row, hrow)] for row, hrow in zip(exact, hi)]).reshape(n, 11)
    for s in range(n):
        x = r["terms"][r["shell_of_tri"] == s]
        for label, got in _orders(x, 3 + s).items():
            assert label != "sequential" or (got == r["sums"][s]).all()
            err, b = np.abs((got - hi[s]) - lo[s]), r["bound"][s]
            assert (err <= b).all(), (name, s, label, err.tolist(), b.tolist())
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
    print(f"SHELLS yardstick {name}: {len(T)} triangles, {n} shells, largest fraction of the bound {worst:.3f}")


@pytest.mark.parametrize("name", C.EXTRACTED)
def test_restatement_agrees_with_iso_ref_on_the_extracted_cases(name):
    V, T = C.case(name)
    r = M.shells(V, T)
    dup, norev = R.unpaired_edges(T, len(V))
    tot = r["totals"]
    assert tot[2] == 0 and tot[0] == len(r["counts"]) and r["counts"][:, 1].sum() == len(T)
    # a regular edge is the only class in which no direction occurs twice and every direction has its reverse
    assert (len(dup) == 0 and len(norev) == 0) == (tot[4] == 0 and tot[5] == 0 and tot[6] == 0)
    assert tot[6] == 0 and tot[5] == 0 and len(norev) == tot[4]          # the extraction is oriented and manifold
    assert tot[7] - tot[3] + tot[1] == R.euler(T, len(V))
    for s in range(len(r["counts"])):
        Ts = T[r["shell_of_tri"] == s]
        c = r["counts"][s]
        assert c[2] - c[3] + c[1] == R.euler(Ts, len(V))
        assert len(R.unpaired_edges(Ts, len(V))[1]) == c[4]
        assert c[0] == np.nonzero(r["shell_of_tri"] == s)[0][0]
    if name in ("sphere33", "nested41", "noise24_closed"):
        assert tot[4] == 0
        # (a closed surface has the same volume about the origin as about the reference point)
        assert abs(R.signed_volume(V, T) - r["sums"][:, 1].sum()) <= 1e-9 * r["T"][:, 1].sum()
    else:
        assert tot[4] > 0


def test_expected_shapes_of_the_hand_made_cases():
    want = {"empty": 0, "one_triangle": 1, "all_collapsed": 0, "tetrahedron": 1, "cube_with_void": 2, "two_tets_sharing_vertex": 2,
            "three_on_edge": 1, "triangle_twice": 1, "cube_one_reversed": 1, "torus": 1, "ribbon": 1, "ribbon_reversed": 1,
            "ribbon_shuffled": 1, "disjoint": 3000, "fans": 400}
    for name, n in want.items():
        assert M.shells(*C.case(name))["totals"][0] == n, name
    r = M.shells(*C.case("cube_with_void"))
    assert r["sums"][:, 1].tolist() == [8.0, -1.0] and r["sums"][:, 0].tolist() == [24.0, 6.0]
    assert M.shells(*C.case("three_on_edge"))["counts"][0, 3:7].tolist() == [7, 6, 0, 1]
    assert M.shells(*C.case("triangle_twice"))["counts"][0, 3:7].tolist() == [3, 0, 3, 0]
    assert (M.shells(*C.case("fans"))["counts"][:, 1] == np.arange(1, 401)).all()


def test_library_exports_the_symbols(pkg):
    lib = pkg._lib.lib()
    for name in ("r2s_mesh_shells", "r2s_last_mesh_shells", "r2s_mesh_shells_dev"):
        assert getattr(lib, name) is not None
    assert {"mesh_shells", "mesh_shells_dev", "select_shells", "MeshShells"} <= set(pkg.__all__)


def _call(pkg, V, T, nv=None, nt=None, outs=True):
    L = pkg._lib
    V, T = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(T, np.int32)
    sot = np.full(max(len(T), 1), -7, np.int32)
    n, ref, tot = ctypes.c_int64(-7), np.full(3, -7.0), np.full(8, -7, np.int64)
    rc = L.lib().r2s_mesh_shells(V.ctypes.data_as(L.c_float_p) if V.size else None, len(V) if nv is None else nv,
                                 T.ctypes.data_as(L.c_int32_p) if T.size else None, len(T) if nt is None else nt, -1,
                                 sot.ctypes.data_as(L.c_int32_p), ctypes.byref(n) if outs else None, ref.ctypes.data_as(L.c_double_p),
                                 tot.ctypes.data_as(L.c_int64_p))
    untouched = (sot == -7).all() and n.value == -7 and (ref == -7.0).all() and (tot == -7).all()
    return rc, untouched


def test_refusals_need_no_device(pkg):
    V, T = C.cube((0, 0, 0), 1.0)
    for bad in (8, -1):
        T2 = T.copy()
        T2[7, 1] = bad
        assert _call(pkg, V, T2) == (ARG, True)
    for bad in (np.inf, np.nan):
        V2 = V.copy()
        V2[3, 2] = bad
        assert _call(pkg, V2, T) == (ARG, True)
    assert _call(pkg, V, T, nv=-1) == (ARG, True) and _call(pkg, V, T, nt=-1) == (ARG, True)
    assert _call(pkg, V, T, outs=False) == (ARG, True)
    assert _call(pkg, np.zeros((0, 3)), T, nv=8) == (ARG, True)
    assert _call(pkg, V, T, nt=2 ** 30 + 1) == (UNSUPPORTED, True)
    assert _call(pkg, V, T, nv=2 ** 31) == (UNSUPPORTED, True)
    lib = pkg._lib.lib()
    n = ctypes.c_int64()
    assert lib.r2s_last_mesh_shells(None, None, 4, ctypes.byref(n)) == ARG
    assert lib.r2s_last_mesh_shells(None, None, 0, None) == ARG
    assert lib.r2s_mesh_shells_dev(None, 0, None, 0, None, None, None, 0, None, None, None, None) == ARG
    with pytest.raises(pkg._lib.R2SError, match="info"):
        pkg.rho2sdf("t", np.zeros((8, 3)), np.arange(1, 9)[None, :], np.ones(1), shells=True)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback(pkg):
    V, T = C.cube((0, 0, 0), 1.0)
    assert _call(pkg, V, T) == (NO_DEVICE, True)
    assert _call(pkg, V[:0], T[:0]) == (NO_DEVICE, True)
    n, ref, tot = ctypes.c_int64(), (ctypes.c_double * 3)(), (ctypes.c_int64 * 8)()
    assert pkg._lib.lib().r2s_mesh_shells_dev(None, 0, None, 0, None, None, None, 0, ctypes.byref(n), ref, tot, None) == NO_DEVICE
    with pytest.raises(pkg._lib.R2SError, match="no HIP device|CPU fallback"):
        pkg.mesh_shells(V, T)


def test_select_shells_on_hand_made_input(pkg):
    V, T = C.cube_with_void()
    V = np.concatenate([np.full((2, 3), 9.0, np.float32), V])           # two unused vertices in front
    T = np.concatenate([T + 2, [[2, 2, 3]]]).astype(np.int32)           # and a collapsed triangle behind
    r = M.shells(V, T)
    counts, sums = r["counts"], r["sums"]
    s = pkg.MeshShells(counts, sums, r["ref_point"], r["totals"], r["shell_of_tri"])
    assert s.n_shells == 2 and s.closed.all() and s.euler.tolist() == [2, 2] and s.genus.tolist() == [0, 0]
    assert s.is_void.tolist() == [False, True]
    assert np.allclose(s.centroid, 1.0) and np.allclose(s.inertia[0], np.eye(3) * 8.0 * (4 + 4) / 12.0)
    v1, t1 = pkg.select_shells(V, T, s, lambda sh: sh.volume > 0)
    assert v1.shape == (8, 3) and t1.shape == (12, 3) and t1.dtype == T.dtype
    assert (v1[t1] == V[T[:12]]).all()
    v2, t2 = pkg.select_shells(V, T, s, np.array([False, True]))
    assert v2.shape == (8, 3) and (v2[t2] == V[T[12:24]]).all() and t2.min() == 0 and t2.max() == 7
    v3, t3 = pkg.select_shells(V, T, s, [False, False])
    assert len(v3) == 0 and t3.shape == (0, 3)
    with pytest.raises(pkg._lib.R2SError):
        pkg.select_shells(V, T, s, [True])
    # an open shell has no centroid
    o = M.shells(*C.one_triangle())
    o = pkg.MeshShells(o["counts"], o["sums"], o["ref_point"], o["totals"], o["shell_of_tri"])
    assert not o.closed[0] and o.genus[0] == -1 and np.isnan(o.centroid).all() and np.isnan(o.inertia).all()
