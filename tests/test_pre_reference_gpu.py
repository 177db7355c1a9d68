"""The pre-stage kernels (r2s_pre.hip: calculate_mesh_volume, DenseInNodes, calculate_isocontour_volume,
find_threshold_for_volume) through the C ABI against tests/pre_ref64.py, the LAPACK / float64 restatement of the
reference's Julia, never against the C oracle.  The kernel is held to the reference's own a-priori round-off bound
(constants measured against mpmath in tests/test_pre_reference_cpu.py); every case prints the largest fraction of the
bound it used, the nodes left out as undecidable and the legs it reached."""
import numpy as np
import pytest

import pre_cases as PC
import pre_ref64 as P

pytestmark = pytest.mark.gpu

NODE_CAP = 1e-3      # at most 0.1 % of a case's nodes may be undecidable
WEIGHT_CAP = 1e-6    # flagged Gauss weight, as a share of the case's volume

SMALL = PC.small_cases()


def _frac(diff, bound):
    """largest |diff| / bound; a zero bound demands the exact value"""
    diff, bound = np.atleast_1d(np.abs(diff)), np.atleast_1d(bound)
    zero = bound == 0
    assert not (zero & (diff != 0)).any(), "a value with bound 0 differs"
    return float((diff[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _check_nodal(pkg, name, X, IEN, rho, repeats=3):
    mesh = pkg.Mesh(X, IEN)
    ref = P.dense_in_nodes(X, IEN, rho)
    got = pkg.DenseInNodes(mesh, rho)
    for _ in range(repeats - 1):   # the scatter's atomics must not reach the answer
        assert np.array_equal(pkg.DenseInNodes(mesh, rho), got)
    undec = ref["undecidable"]
    assert undec.sum() <= NODE_CAP * len(X), (name, int(undec.sum()))
    ok = ~undec
    assert np.isfinite(got[ok]).all()
    frac = _frac((got - ref["rho_n"])[ok], ref["bound"][ok])
    unused = ref["count"] == 0
    assert (got[unused] == 0.0).all()                       # `zeros` (NodalDensities.jl:96) leaves them
    legs = sorted(set(ref["kept"][ref["leg"] == P.LEG_LSQ].tolist()))
    print(f"PRE nodal {name}: nnp {len(X)} fraction of bound {frac:.3g} excluded {int(undec.sum())} "
          f"counts {sorted(set(ref['count'].tolist()))} eigenvalues kept {legs}")
    assert frac < 1.0, (name, frac)
    return ref, got, frac


def _check_volume(pkg, name, X, IEN, rho, repeats=3):
    mesh = pkg.Mesh(X, IEN)
    ref = P.mesh_volume(X, IEN, rho)
    vd, vf = pkg.calculate_mesh_volume(mesh, rho)
    for _ in range(repeats - 1):
        assert pkg.calculate_mesh_volume(mesh, rho) == (vd, vf)
    fd = _frac(vd - ref["V_domain"], ref["bound_domain"])
    ff = _frac(vf - ref["V_frac"], ref["bound_frac"])
    print(f"PRE volume {name}: nel {len(IEN)} V_domain {vd!r} fraction of bound {fd:.3g} V_frac {vf!r} fraction {ff:.3g}")
    assert fd < 1.0 and ff < 1.0, (name, fd, ff)
    return ref, vd, vf


@pytest.mark.parametrize("dens", PC.DENSITIES)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_mesh_volume_and_nodal_densities(pkg, name, dens):
    X, IEN = SMALL[name]()
    rho = PC.density(dens, X, IEN)
    _check_volume(pkg, f"{name}/{dens}", X, IEN, rho)
    _check_nodal(pkg, f"{name}/{dens}", X, IEN, rho)


@pytest.mark.parametrize("name", PC.FIXTURES)
def test_fixtures(pkg, name):
    X, IEN, rho = PC.fixture(name)
    _check_volume(pkg, name, X, IEN, rho)
    ref, got, _ = _check_nodal(pkg, name, X, IEN, rho)
    if name == "sphere":   # reference known answers, HexSphereSdfTest.jl:26-27
        assert abs(got.max() - 1.0000000000000022) <= ref["bound"][np.argmax(got)]
        assert abs(got.mean() - 0.29490556408887564) <= ref["bound"].mean()


def test_million_nodes_scan_carries_across_tiles(pkg):
    """nnp + 1 > 1024 * 1024: scan_sums_kernel runs its loop a second time and hands the carry on; a node list that
    starts at the wrong offset gives a wrong density at that node"""
    X, IEN = PC.big_mesh()
    rho = PC.density("uniform", X, IEN)
    _check_volume(pkg, "hex102", X, IEN, rho, repeats=2)
    ref, got, _ = _check_nodal(pkg, "hex102", X, IEN, rho, repeats=2)
    tile = 1024 * 1024
    assert (ref["count"][tile - 8: tile + 8] > 0).all()     # real nodes on both sides of the first carried tile


def test_every_leg_is_reached():
    """by the reference's own diagnostics over the cases above: node counts 0, 1, 2, 3, 4+ (3, 5, 6, 7 on the mesh with
    holes), and LamReduction keeping 4, 3, 2, 1 eigenvalues or none (mean of b: reached by real meshes, the thin bars,
    where 3e3 < e2 <= e1 < 1e7, so nothing is forced)"""
    counts, kept = set(), set()
    for name in sorted(SMALL):
        X, IEN = SMALL[name]()
        ref = P.dense_in_nodes(X, IEN, PC.density("uniform", X, IEN))
        counts |= set(ref["count"].tolist())
        kept |= set(ref["kept"][ref["leg"] == P.LEG_LSQ].tolist())
    print("PRE legs reached: counts", sorted(counts), "eigenvalues kept", sorted(kept))
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} <= counts and max(counts) > 8
    assert kept == {0, 1, 2, 3, 4}


# ---- iso-volume ---------------------------------------------------------------------------------------------------------
ISO_CASES = ("hex7-j0.3-id", "hex7-j0.3-+30", "tet5-j0.3-id", "tet5-j0.3-aniso", "holes", "hex-nel3", "hex-nel5", "tet-nel1",
             "tet-nel2")


def _nodal_field(X, IEN, kind):
    if kind == "reference":      # what DenseInNodes delivers for a binary design: values leave [0, 1]
        return P.dense_in_nodes(X, IEN, PC.density("binary", X, IEN))["rho_n"]
    c = X.mean(0)
    r = np.linalg.norm((X - c) / np.maximum(np.ptp(X, axis=0), 1e-300), axis=1)
    return np.clip(1.5 - 2.5 * r, 0.0, 1.0)   # exact zeros and ones at many nodes, as a clamped design has


@pytest.mark.parametrize("field", ["reference", "clipped"])
@pytest.mark.parametrize("name", ISO_CASES)
def test_isocontour_volume(pkg, name, field):
    X, IEN = SMALL[name]()
    mesh = pkg.Mesh(X, IEN)
    rn = _nodal_field(X, IEN, field)
    used = np.unique(IEN) - 1
    lo, hi = rn[used].min(), rn[used].max()
    vd, _ = pkg.calculate_mesh_volume(mesh, np.ones(len(IEN)))
    one_node = float(np.sort(rn[used])[len(used) // 2])
    thrs = {"below min": lo - 0.1, "min": lo, "above max": hi + 0.1, "0": 0.0, "1": 1.0, "a nodal value": one_node,
            "mid": 0.5 * (lo + hi)}
    worst = 0.0
    for label, thr in thrs.items():
        ref = P.isocontour_volume(X, IEN, rn, thr)
        v = pkg.calculate_isocontour_volume(mesh, rn, thr)
        for _ in range(2):
            assert pkg.calculate_isocontour_volume(mesh, rn, thr) == v
        assert ref["flagged"] <= WEIGHT_CAP * vd, (name, label, ref["flagged"])
        f = _frac(v - ref["volume"], ref["bound"])
        worst = max(worst, f)
        print(f"PRE iso {name}/{field} thr {label} = {thr!r}: volume {v!r} fraction of bound {f:.3g} flagged {ref['flagged']:.3g} "
              f"skip/whole/cut {ref['n_skip']}/{ref['n_whole']}/{ref['n_cut']}")
        assert f < 1.0, (name, label, f)
        if label in ("below min", "min"):    # find_threshold compares target > vmax without slack
            assert v == vd, (name, label, v, vd)
        if label == "above max":
            assert v == 0.0
    # a constant field equal to the threshold is solid everywhere: min >= thr holds with equality
    for c in (0.0, 0.3, 1.0):
        assert pkg.calculate_isocontour_volume(mesh, np.full(len(X), c), c) == vd, (name, c)
    print(f"PRE iso {name}/{field}: largest fraction of bound {worst:.3g}")


# ---- find_threshold_for_volume ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hex7-j0.3-id", "tet5-j0.3-id", "holes"])
def test_find_threshold(pkg, name):
    X, IEN = SMALL[name]()
    mesh = pkg.Mesh(X, IEN)
    rn = _nodal_field(X, IEN, "clipped")
    memo = {}
    real = P.isocontour_volume

    def cached(X_, IEN_, rn_, thr, **kw):
        if thr not in memo:
            memo[thr] = real(X_, IEN_, rn_, thr, **kw)
        return memo[thr]

    P.isocontour_volume = cached
    try:
        vmin, vmax = cached(X, IEN, rn, 1.0)["volume"], cached(X, IEN, rn, 0.0)["volume"]
        assert 0.0 < vmin < vmax
        target = vmin + 0.37 * (vmax - vmin)
        configs = [("default", target, 1e-4, 60, None), ("best so far", target, 0.0, 7, 7), ("first step", target, 0.5, 60, 0),
                   ("just inside vmax", vmax * (1 - 1e-9), 1e-4, 5, None), ("just inside vmin", vmin * (1 + 1e-9), 1e-4, 5, None)]
        for label, tgt, tol, maxit, want_iters in configs:
            ref = P.find_threshold(X, IEN, rn, tgt, tol, maxit)
            worst = max(s["bound"] / s["margin"] if s["margin"] > 0 else np.inf for s in ref["steps"])
            assert ref["decidable"], (name, label, "pick another target: the reference's own margin is inside the bound", worst)
            info = {}
            rt = pkg.find_threshold_for_volume(mesh, rn, tgt, tol, maxit, info=info)
            for _ in range(2):
                assert pkg.find_threshold_for_volume(mesh, rn, tgt, tol, maxit) == rt
            print(f"PRE threshold {name} {label}: rho_t {rt!r} ({ref['rho_t']!r}) iterations {info['iterations']} ({ref['iters']}) "
                  f"largest bound / margin {worst:.3g}")
            assert rt == ref["rho_t"] and info["iterations"] == ref["iters"], (name, label)
            if want_iters is not None:
                assert info["iterations"] == want_iters
        for label, tgt in (("just outside vmax", vmax * (1 + 1e-9)), ("just outside vmin", vmin * (1 - 1e-9))):
            with pytest.raises(P.OutOfRange):
                P.find_threshold(X, IEN, rn, tgt)
            with pytest.raises(pkg._lib.R2SError, match="outside the possible range"):
                pkg.find_threshold_for_volume(mesh, rn, tgt)
    finally:
        P.isocontour_volume = real


@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_fully_solid_mesh_is_inside_the_range(pkg, kind):
    """V_frac == 1: the target V_domain * 1 must not be refused as "outside the possible range"; volume(thr <= min) and
    V_domain are the same sum.  (HEX8: both come from the same kernel path; TET4: the whole-element path of the iso-volume
    kernel adds its points in the order of the mesh-volume kernel)"""
    X, IEN = SMALL[f"{kind}12-j0.45-id" if kind == "hex" else "tet8-j0.45-id"]()
    mesh = pkg.Mesh(X, IEN)
    vd, vf = pkg.calculate_mesh_volume(mesh, np.ones(len(IEN)))
    assert vf == 1.0
    rn = np.ones(len(X))
    assert pkg.calculate_isocontour_volume(mesh, rn, 0.0) == vd
    info = {}
    rt = pkg.find_threshold_for_volume(mesh, rn, vd * vf, info=info)
    print(f"PRE solid {kind}: V_domain {vd!r} rho_t {rt!r} iterations {info['iterations']}")
    assert 0.0 < rt <= 1.0
