"""r2s_mesh_simplify on the GPU against tests/mesh_simplify_ref.py, from the host entry, the _dev entry and a non-default stream.

Measured on an MI355X (`SIMPLIFY` lines, pytest -s): MEAN, every output vertex of every case bit-equal to the restatement, at
most 1.000 of the bound used (the float32 rounding itself); QUADRIC, |x_gpu - x_ref| = 0.000 cell * eps32 on every margined class
of every case.  QUADRIC_TOL is that measured value; the test asserts 4 times it with a floor of one float32 ulp, and checks each
case's value against the a-priori ceiling of a_priori()."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import mesh_simplify_cases as C
import mesh_simplify_ref as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
RULES = (R.MEAN, R.QUADRIC)
# the largest |x_gpu - x_ref| / (cell * eps32) measured over all cases and all classes on an MI355X: 0.0 - every float32
# coordinate equals the eigh restatement's bit for bit (the Float64 results differ far below a float32 ulp).  Asserted times 4,
# with a floor of ONE float32 ulp of the coordinate (|x| / cell in these units): a Float64 difference of any size can flip one
# float32 rounding, and another LAPACK build must not break the suite for that.
QUADRIC_TOL = 0.0
_refs, _gpu = {}, {}


CASES = dict(C.all_cases())                              # the named cases, the permuted half, the recorded extractor meshes
NAMES = list(CASES)
RECORDED = tuple(C.recorded())


def ref(name, rule):
    if (name, rule) not in _refs:
        _refs[name, rule] = R.simplify_ref(*CASES[name], rule, check=False)
    return _refs[name, rule]


def run(pkg, name, rule, mode="host", **kw):
    """one library call -> dict of numpy arrays; mode host / dev / stream (a non-default, non-blocking stream that also carries
    the upload of the inputs)"""
    v, t, cell = CASES[name]
    if mode == "host":
        r = pkg.mesh_simplify(v, t, cell, rule, device=0, **kw)
        f = lambda a: np.asarray(a)
    else:
        import torch
        st = torch.cuda.Stream() if mode == "stream" else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            dv = torch.empty((len(v), 3), dtype=torch.float32, device="cuda:0")
            dt = torch.empty((len(t), 3), dtype=torch.int32, device="cuda:0")
            dv.copy_(torch.from_numpy(v).pin_memory(), non_blocking=True)
            dt.copy_(torch.from_numpy(t).pin_memory(), non_blocking=True)
            r = pkg.mesh_simplify_dev(dv, dt, cell, rule, stream=st, **kw)
            out = [x.clone() for x in (r.verts, r.tris, r.vert_map, r.tri_map)]
        st.synchronize()
        r.verts, r.tris, r.vert_map, r.tri_map = out
        f = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return dict(verts=f(r.verts).reshape(-1, 3), tris=f(r.tris).reshape(-1, 3), vert_map=f(r.vert_map), tri_map=f(r.tri_map),
                members=r.members, error=r.error, solved=r.solved, totals=np.asarray(r.totals), ratio=r.ratio)


def gpu(pkg, name, rule):
    if (name, rule) not in _gpu:
        _gpu[name, rule] = run(pkg, name, rule)
    return _gpu[name, rule]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k]))
               for k in ("verts", "tris", "vert_map", "tri_map", "members", "error", "solved", "totals"))


def partition(labels):
    groups = {}
    for i, c in enumerate(labels):
        groups.setdefault(int(c), []).append(i)
    return sorted(map(tuple, groups.values()))


def test_abi_symbols(pkg):
    names = [s[0] for s in pkg._lib.SYMBOLS]
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for s in ("r2s_mesh_simplify", "r2s_mesh_simplify_dev", "r2s_last_mesh_simplify"):
        assert names.count(s) == 1 and hasattr(lib, s)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", NAMES)
def test_integers(pkg, name, rule):
    """from the host entry, the _dev entry and a non-default stream: the integers equal the restatement, and the three agree bit
    for bit in everything"""
    r = ref(name, rule)
    host = gpu(pkg, name, rule)
    for mode in ("host", "dev", "stream"):
        g = host if mode == "host" else run(pkg, name, rule, mode)
        for k in ("tris", "vert_map", "tri_map", "members"):
            assert g[k].shape == r[k].shape and np.array_equal(g[k], r[k]), (mode, k)
        assert np.array_equal(g["totals"][:7], r["totals"][:7]), mode
        assert len(g["verts"]) == r["totals"][0] and len(g["solved"]) == r["totals"][0] == len(g["error"])
        assert g["totals"][7] == (g["solved"] >= 4).sum()
        if not r["undecidable"].any():                   # (every named case; else a pull-back flag may be either way)
            assert g["totals"][7] == r["totals"][7], mode
        assert same(g, host), mode
    # the partition is the weld's, on the member vertices of classes that survive
    v, t, cell = CASES[name]
    if len(v):
        w = pkg.mesh_weld(v, t, snap=cell, drop_collapsed=False, drop_unused=False, device=0)
        m = host["vert_map"] >= 0
        assert partition(host["vert_map"][m]) == partition(w.vert_map[m])


@pytest.mark.parametrize("name", NAMES)
def test_mean_positions(pkg, name):
    g, r = gpu(pkg, name, R.MEAN), ref(name, R.MEAN)
    v = CASES[name][0]
    if not len(g["verts"]):
        return
    equal = int((bits(g["verts"]) == bits(r["verts"])).all(1).sum())
    worst = 0.0
    for c in range(len(g["verts"])):
        members = np.nonzero(g["vert_map"] == c)[0]
        assert len(members) == g["members"][c]
        for k in range(3):
            exact = sum((Fraction(float(x)) for x in v[members, k]), Fraction(0)) / len(members)
            x = float(g["verts"][c, k])
            bound = r["mean_bound"][c, k] / len(members) + 2.0 ** -53 * abs(x) + 0.5 * float(np.spacing(np.float32(abs(x))))
            used = float(abs(Fraction(x) - exact)) / bound
            worst = max(worst, used)
            assert used <= 1.0, (c, k, used)
    print(f"SIMPLIFY mean {name}: {equal} of {len(g['verts'])} vertices bit-equal to the restatement, {worst:.3f} of the bound used")
    assert np.array_equal(g["solved"], np.zeros(len(g["verts"]), np.int32))


def a_priori(xmax, cell):
    """the ceiling of |x_gpu - x_ref| / (cell * eps32): Jacobi and LAPACK agree on the eigen-system of S to a few ulps of
    lambda_max, taken as 8 * 2^-53 relative; a kept direction has lambda >= 1e-3 lambda_max, so the solve amplifies that by at
    most 1e3; the step is at most the cell diagonal: 8 * 2^-53 * 1e3 * sqrt(3) cell.  Then both sides round once to float32,
    and two roundings of nearby Float64 values differ by at most one float32 ulp of the coordinate, at most eps32 * xmax."""
    return 8 * 2.0 ** -53 * 1e3 * 3 ** 0.5 / EPS32 + xmax / cell


def test_quadric_positions(pkg):
    """every class of every case against the restatement.  A class with a margin has one candidate, the definition's result; a
    class without one has the result of every decision it could take (R.simplify_ref: each eigenvalue without a margin kept or
    dropped, the pull-back flag either way), and the library has to agree with one of them in `solved` AND position - so no class
    is skipped.  The share of classes without a margin is capped at 1 % on the named cases; the recorded extractor meshes cannot
    meet that at any cell (a sphere sampled finer than its curvature has eigenvalue ratios of about (cell / radius)^2 spread
    across the 1e-3 threshold, box faces put optima ON cell faces), which is why they are compared through the candidates."""
    worst, worst_name = 0.0, ""
    for name in NAMES:
        g, r = gpu(pkg, name, R.QUADRIC), ref(name, R.QUADRIC)
        if not len(g["verts"]):
            continue
        v, _, cell = CASES[name]
        und = r["undecidable"]
        if name not in RECORDED:
            assert und.sum() <= 0.01 * len(und), (name, int(und.sum()), len(und))
        m = 0.0
        for c in range(len(g["verts"])):
            cands = [x for code, x in r["candidates"][c] if code == g["solved"][c]]
            assert len(r["candidates"][c]) == 1 or und[c]
            assert cands, (name, c, int(g["solved"][c]), [code for code, _ in r["candidates"][c]])
            x = g["verts"][c].astype(np.float64)
            best = min(cands, key=lambda y: np.abs(x - y.astype(np.float64)).max())
            d = np.abs(x - best.astype(np.float64))
            allowed = np.maximum(4 * QUADRIC_TOL * cell * EPS32, np.spacing(np.abs(best)).astype(np.float64))
            assert (d <= allowed).all(), (name, c, d, allowed)
            m = max(m, float(d.max()) / (cell * EPS32))
        ceiling = a_priori(float(np.abs(r["verts"]).max()), cell)
        print(f"SIMPLIFY quadric {name}: {len(und)} classes, {int(und.sum())} without a margin (compared through their candidates), "
              f"max |x_gpu - x_ref| = {m:.3f} cell * eps32 (a-priori ceiling {ceiling:.3f}), pulled {int(g['totals'][7])}")
        assert m <= ceiling, name
        if m > worst:
            worst, worst_name = m, name
    print(f"SIMPLIFY quadric worst {worst:.3f} cell * eps32 ({worst_name}); measured value recorded: {QUADRIC_TOL}")


def _slack(E, c, point, cell, items_max):
    """how much E may change when `point` moves by the rounding the header allows: one float32 ulp per axis plus the Float64
    solve error 1e3 (n + K) 2^-53 cell: |E(p + e) - E(p)| <= 2 sqrt(E(p) tr(S)) |e| + tr(S) |e|^2 (Cauchy-Schwarz)"""
    e = 3 ** 0.5 * (float(np.spacing(np.float32(np.abs(point).max()))) + 1e3 * (items_max + R.K) * 2.0 ** -53 * cell)
    tr = float(E.trace(c))
    return 2.0 * (float(E(c, point)) * tr) ** 0.5 * e + tr * e * e


@pytest.mark.parametrize("name", NAMES)
def test_quadric_properties(pkg, name):
    """independent of the restatement's solve: E(x) <= E(m) in Fraction, in-cell, and the deviation bound"""
    q, m = gpu(pkg, name, R.QUADRIC), gpu(pkg, name, R.MEAN)
    v, t, cell = CASES[name]
    if not len(q["verts"]):
        return
    r = ref(name, R.QUADRIC)
    E = R.exact_quadric(v, t, q["vert_map"])
    for c in range(len(q["verts"])):                     # (every class, margin or not)
        ex, em = E(c, q["verts"][c]), E(c, m["verts"][c])
        assert float(ex - em) <= _slack(E, c, q["verts"][c], cell, r["items_max"]) + _slack(E, c, m["verts"][c], cell, r["items_max"]), c
    for g in (q, m):
        x = g["verts"].astype(np.float64)
        lo, hi = r["cells"] * cell, (r["cells"] + 1.0) * cell
        ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)   # of the cell's larger face coordinate
        assert (x >= lo - ulp).all() and (x <= hi + ulp).all()
    if len(q["tris"]):
        moved = np.linalg.norm(q["verts"][q["vert_map"][q["vert_map"] >= 0]].astype(np.float64) - v[q["vert_map"] >= 0], axis=1)
        assert moved.max() <= 3 ** 0.5 * cell * (1 + 1e-6)
        pts = v[np.unique(t[q["tri_map"] >= 0])]         # the vertices of the surviving input triangles
        d = pkg.MeshIndex(q["verts"], q["tris"], device=0).distance(pts)
        assert float(np.max(d)) <= 3 ** 0.5 * cell * (1 + 1e-6), name


def test_cube_corners_edges_faces(pkg):
    q, m = gpu(pkg, "cube", R.QUADRIC), gpu(pkg, "cube", R.MEAN)
    v, t, cell = CASES["cube"]
    r = ref("cube", R.QUADRIC)
    lo, hi = v.min(0), v.max(0)
    tol = float(np.spacing(np.float32(np.abs(v).max()))) + 1e3 * (r["items_max"] + R.K) * 2.0 ** -53 * 1.0
    on = (v == lo) | (v == hi)                           # per vertex and axis: on a face of that axis
    gap = 0.0
    for c in range(len(q["verts"])):
        mem = np.nonzero(q["vert_map"] == c)[0]
        # the planes the class touches: axis k is pinned if some member triangle lies in a face of axis k; with this cube every
        # class that holds a vertex on a face of axis k holds triangles of that face
        for k in range(3):
            if on[mem, k].any():
                target = v[mem[on[mem, k]][0], k]
                assert abs(float(q["verts"][c, k]) - float(target)) <= tol, (c, k)
                gap = max(gap, abs(float(m["verts"][c, k]) - float(target)))
    assert gap > 0.05, gap                               # the mean leaves the faces: rule MEAN rounds the cube off


def test_reproducible(pkg):
    """repeated calls and fresh work buffers (host against _dev against a stream: test_integers, on every case)"""
    for name in ("cube", "fan_5000", "icosphere_0.25", "sphere33", "welded_touch_2"):
        for rule in RULES:
            assert same(gpu(pkg, name, rule), run(pkg, name, rule)), (name, rule, "repeat")
    pkg._lib.lib().r2s_release_cache()
    for rule in RULES:
        assert same(gpu(pkg, "fan_5000", rule), run(pkg, "fan_5000", rule)), "fresh work buffers"


def test_capacities(pkg):
    L, lib = pkg._lib, pkg._lib.lib()
    g = run(pkg, "icosphere_0.25", R.QUADRIC)
    n = len(g["verts"])
    for cap in (0, n - 1, n):
        mem, err, sol = np.full(n, -7, np.int64), np.full(n, -7.0), np.full(n, -7, np.int32)
        cnt = ctypes.c_int64(-1)
        L.check(lib.r2s_last_mesh_simplify(mem.ctypes.data_as(L.c_int64_p) if cap else None, err.ctypes.data_as(L.c_double_p) if cap else None,
                                           sol.ctypes.data_as(L.c_int32_p) if cap else None, cap, ctypes.byref(cnt)))
        assert cnt.value == n
        assert np.array_equal(mem[:cap], g["members"][:cap]) and np.array_equal(bits(err[:cap]), bits(g["error"][:cap]))
        assert np.array_equal(sol[:cap], g["solved"][:cap])
        assert (mem[cap:] == -7).all() and (err[cap:] == -7.0).all() and (sol[cap:] == -7).all()
    assert lib.r2s_last_mesh_simplify(None, None, None, 1, ctypes.byref(cnt)) == -1      # (R2S_ERR_ARG: NULL arrays with a capacity)


def test_refusals(pkg):
    L, lib = pkg._lib, pkg._lib.lib()
    v, t, cell = CASES["cube"]
    nv, nt = len(v), len(t)
    fp, ip = lambda a: a.ctypes.data_as(L.c_float_p), lambda a: a.ctypes.data_as(L.c_int32_p)

    def call(v=v, t=t, cell=cell, rule=1, flags=2, tris_null=False):
        vo, to = np.full((nv, 3), -7, np.float32), np.full((nt, 3), -7, np.int32)
        vm, tm, tot = np.full(nv, -7, np.int32), np.full(nt, -7, np.int32), np.full(8, -7, np.int64)
        rc = lib.r2s_mesh_simplify(fp(v), nv, None if tris_null else ip(t), nt, cell, rule, flags, 0, fp(vo), ip(to), ip(vm), ip(tm),
                                   tot.ctypes.data_as(L.c_int64_p))
        untouched = (vo == -7).all() and (to == -7).all() and (vm == -7).all() and (tm == -7).all() and (tot == -7).all()
        return rc, untouched

    assert call() == (0, False)
    bad = t.copy()
    bad[5, 1] = nv
    neg = t.copy()
    neg[0, 0] = -1
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e-12), dict(rule=2),
               dict(rule=-1), dict(flags=1), dict(flags=4), dict(flags=8), dict(tris_null=True), dict(t=bad), dict(t=neg)):
        assert call(**kw) == (-1, True), kw
    import torch
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(bad).cuda()
    with pytest.raises(L.R2SError):
        pkg.mesh_simplify_dev(dv, dt, cell)
    with pytest.raises(L.R2SError):
        pkg.mesh_simplify_dev(dv, torch.from_numpy(t).cuda(), 1e-12)
    with pytest.raises(L.R2SError):
        pkg.mesh_simplify(v, t, cell, "best")


def _boundary_edges(t):
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return int((n == 1).sum())


def test_chain(pkg):
    v, t, cell = CASES["sphere33"]
    assert _boundary_edges(t) == 0
    for rule in RULES:
        g = gpu(pkg, "sphere33", rule)
        sh = pkg.mesh_shells(g["verts"], g["tris"], device=0)
        fans = pkg.mesh_fans(g["verts"], g["tris"], device=0)
        holes = pkg.mesh_holes(g["verts"], g["tris"], device=0)
        x = pkg.mesh_intersections(g["verts"], g["tris"], device=0)
        print(f"SIMPLIFY chain {rule}: {len(t)} -> {len(g['tris'])} triangles (ratio {g['ratio']:.3f}), shells totals {np.asarray(sh.totals).tolist()}, "
              f"fans totals {np.asarray(fans.totals).tolist()}, holes totals {np.asarray(holes.totals).tolist()}, {len(x)} intersecting pairs")
        assert _boundary_edges(g["tris"]) == 0           # clustering opens no hole
        again = pkg.mesh_simplify(g["verts"], g["tris"], cell, rule, device=0)
        assert again.n_tris == len(g["tris"])


def test_entry_points(pkg, tmp_path):
    from conftest import load_fixture
    X, IEN, rho = load_fixture("sphere")
    grid = pkg.Grid(X.min(0), X.max(0), 8, 3)
    opts = pkg.Rho2sdfOptions(threshold_density=0.5)
    a, b = {}, {}
    pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=a, surface=True)
    pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=grid, info=b, surface=True, simplify_cells=2)
    assert 0 < len(b["surface"][1]) < len(a["surface"][1])
    assert b["simplify"].n_tris == len(b["surface"][1]) and b["simplify"].ratio < 1.0
    v, t, cell = CASES["sphere33"]
    path = pkg.export_stl(str(tmp_path / "s"), v, t)
    v0, t0 = pkg.import_stl(path, device=0)
    v1, t1 = pkg.import_stl(path, device=0, simplify=cell)
    want = pkg.mesh_simplify(v0, t0, cell, device=0)
    assert np.array_equal(bits(v1), bits(want.verts)) and np.array_equal(t1, want.tris) and len(t1) < len(t0)
