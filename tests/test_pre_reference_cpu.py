"""tests/pre_ref64.py (the LAPACK / float64 restatement of the pre-stage) checked on its own, without a GPU:
known answers, the reference against its 50-digit mpmath self (where the constants of its bounds come from), the caps on
undecidable nodes and flagged Gauss weight for every case the GPU file uses, and the C oracle (the yardstick of the
other GPU tests, cyclic Jacobi instead of LAPACK) against the new reference."""
import mpmath
import numpy as np
import pytest

import pre_cases as PC
import pre_ref64 as P

SMALL = PC.small_cases()
NODE_CAP, WEIGHT_CAP = 1e-3, 1e-6
ISO_CASES = ("hex7-j0.3-id", "hex7-j0.3-+30", "tet5-j0.3-id", "tet5-j0.3-aniso", "holes", "hex-nel3", "hex-nel5", "tet-nel1",
             "tet-nel2")
MP_CASES = ("hex12-j0.15-id", "hex12-j0.45-+30", "hex12-j0.15-+1000", "hex12-j0.45-aniso", "hex12-j0.15-bar", "tet8-j0.45-id",
            "tet8-j0.15-+30", "tet8-j0.45-+1000", "tet8-j0.15-aniso", "tet8-j0.45-bar", "holes")


def _frac(diff, bound):
    diff, bound = np.atleast_1d(np.abs(diff)), np.atleast_1d(bound)
    zero = bound == 0
    assert not (zero & (diff != 0)).any()
    return float((diff[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ---- known answers ------------------------------------------------------------------------------------------------------
def test_sphere_nodal_densities_known_answer():
    X, IEN, rho = PC.fixture("sphere")
    ref = P.dense_in_nodes(X, IEN, rho)
    rn = ref["rho_n"]
    assert not ref["undecidable"].any()
    assert abs(rn.max() - 1.0000000000000022) <= ref["bound"][np.argmax(rn)]      # HexSphereSdfTest.jl:26-27
    assert abs(rn.mean() - 0.29490556408887564) <= ref["bound"].mean()
    assert rn.max() == pytest.approx(1.0000000000000022, rel=1e-10, abs=1e-12)
    assert rn.mean() == pytest.approx(0.29490556408887564, rel=1e-10, abs=1e-12)


def test_beam_threshold_known_answer():
    X, IEN, rho = PC.fixture("beam_vfrac_04")
    mv = P.mesh_volume(X, IEN, rho)
    rn = P.dense_in_nodes(X, IEN, rho)["rho_n"]
    r = P.find_threshold(X, IEN, rn, mv["V_domain"] * mv["V_frac"])
    assert float(f"{r['rho_t']:.6g}") == 0.518555                                   # reference literal, runtests.jl:198
    assert r["decidable"]


def test_exact_volumes_on_the_cube():
    """interior jitter leaves the HEX8 total of [-1, 1]^3 at 8 while det J stays positive at every Gauss point (trilinear
    maps tile the cube; the 3^3 rule is exact for them); the TET4 total is 0.75 * 8 with the reference's (1 - xi)^2
    Jacobian (MeshVolume.jl:110).  At jitter 0.45 some elements fold over and |det J| (MeshVolume.jl:67) adds their
    inverted parts instead of subtracting them: the total can only grow."""
    Xh, Ih = SMALL["hex12-j0.15-id"]()
    Xt, It = SMALL["tet8-j0.15-id"]()
    h = P.mesh_volume(Xh, Ih, np.ones(len(Ih)))
    t = P.mesh_volume(Xt, It, np.ones(len(It)))
    assert abs(h["V_domain"] - 8.0) <= h["bound_domain"] and h["bound_domain"] < 1e-10
    assert abs(t["V_domain"] - 6.0) <= t["bound_domain"] and t["bound_domain"] < 1e-10
    assert h["V_frac"] == 1.0 and t["V_frac"] == 1.0
    Xf, If = SMALL["hex12-j0.45-id"]()
    f = P.mesh_volume(Xf, If, np.ones(len(If)))
    assert f["V_domain"] >= 8.0 - f["bound_domain"]


@pytest.mark.parametrize("name", ["hex12-j0.15-id", "hex12-j0.45-id", "tet8-j0.15-id", "holes"])
def test_linear_density_is_reproduced_where_all_eigenvalues_are_kept(name):
    X, IEN = SMALL[name]()
    g = np.array([0.2, -0.1, 0.15])
    rho = 0.5 + P.centroids(X, IEN) @ g
    ref = P.dense_in_nodes(X, IEN, rho)
    full = (ref["kept"] == 4) & ~ref["undecidable"]
    assert full.sum() > 100
    assert _frac((ref["rho_n"] - (0.5 + X @ g))[full], ref["bound"][full]) < 1.0


# ---- the float64 reference against its exact self: the constants ----------------------------------------------------------
def _mpf(x):
    return mpmath.mpf(float(x))


def test_constants_leave_a_factor_four_over_the_reference_error():
    rng = np.random.default_rng(2024)
    worst = dict(K_VOL=0.0, K_LSQ=0.0, K_FLT=0.0, K_EIG=0.0, K_PT=0.0, mean=0.0)
    for name in MP_CASES:
        X, IEN = SMALL[name]()
        rho = PC.density("uniform", X, IEN)
        ref = P.dense_in_nodes(X, IEN, rho)
        ptr, els = P.node_elements(IEN, len(X))
        pick = np.concatenate([rng.choice(len(X), 24, replace=False), np.flatnonzero((ref["count"] > 1) & (ref["count"] < 4))[:6]])
        for n in pick:
            if ref["undecidable"][n]:
                continue
            val, lam = P.nodal_density_mp(X, IEN, rho, n, ptr, els, int(ref["kept"][n]))
            err = float(abs(_mpf(ref["rho_n"][n]) - val))
            if ref["leg"][n] == P.LEG_LSQ:
                cnt = int(ref["count"][n])
                unit_eig = P.EPS * cnt * float(sum(lam))
                worst["K_EIG"] = max(worst["K_EIG"], max(float(abs(_mpf(a) - b)) for a, b in zip(ref["lam"][n], lam)) / unit_eig)
                if ref["kept"][n] == 0:
                    worst["mean"] = max(worst["mean"], err / ref["bound"][n])
                else:
                    worst["K_LSQ"] = max(worst["K_LSQ"], err / (ref["bound"][n] / P.K_LSQ))
            elif ref["leg"][n] == P.LEG_FILTER:
                worst["K_FLT"] = max(worst["K_FLT"], err / (ref["bound"][n] / P.K_FLT))
            else:
                assert err == 0.0
        vol, unit = P.element_volumes(X, IEN)
        for e in rng.choice(len(IEN), 16, replace=False):
            exact = P.element_volume_mp(X[IEN[e] - 1])
            worst["K_VOL"] = max(worst["K_VOL"], float(abs(_mpf(vol[e]) - exact)) / (P.EPS * unit[e]))
    # the interpolated density of the point test, on random corner values
    N, _, _ = P.hex_tables(15)
    for _ in range(40):
        re = rng.uniform(-0.2, 1.2, 8)
        g = int(rng.integers(0, 3375))
        exact = P.hex_point_value_mp(re, g)
        worst["K_PT"] = max(worst["K_PT"], float(abs(_mpf(N[g] @ re) - exact)) / (P.EPS * float(np.abs(N[g]) @ np.abs(re))))
    print("PRE largest |float64 - exact| in units of the bounds:", {k: round(v, 4) for k, v in worst.items()})
    assert worst["mean"] <= 1.0
    for k in ("K_VOL", "K_LSQ", "K_FLT", "K_EIG", "K_PT"):
        K = getattr(P, k)
        assert 4.0 * worst[k] <= K, (k, worst[k], K)                 # inside its own bound with a factor 4 to spare
        assert np.log2(K) == int(np.log2(K))


# ---- the caps, with the reference alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_cases_stay_inside_the_node_cap(name):
    X, IEN = SMALL[name]()
    for dens in PC.DENSITIES:
        ref = P.dense_in_nodes(X, IEN, PC.density(dens, X, IEN))
        assert ref["undecidable"].sum() <= NODE_CAP * len(X), (name, dens, int(ref["undecidable"].sum()))
        assert np.isfinite(ref["rho_n"][~ref["undecidable"]]).all()


def test_fixtures_stay_inside_the_node_cap():
    for name in PC.FIXTURES:
        X, IEN, rho = PC.fixture(name)
        ref = P.dense_in_nodes(X, IEN, rho)
        print("PRE", name, "undecidable", int(ref["undecidable"].sum()), "of", len(X))
        assert ref["undecidable"].sum() <= NODE_CAP * len(X)


def test_every_leg_is_reached():
    counts, kept = set(), set()
    for name in sorted(SMALL):
        X, IEN = SMALL[name]()
        ref = P.dense_in_nodes(X, IEN, PC.density("uniform", X, IEN))
        counts |= set(ref["count"].tolist())
        kept |= set(ref["kept"][ref["leg"] == P.LEG_LSQ].tolist())
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8} <= counts and max(counts) > 8
    assert kept == {0, 1, 2, 3, 4}       # 0: mean(b), reached by the thin bars


# ---- the C oracle against the new reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL) + list(PC.FIXTURES))
def test_oracle_agrees_with_lapack(oracle, name):
    """the oracle's Jacobi, sort, column convention and LamReduction against LAPACK, inside the reference's bound"""
    if name in PC.FIXTURES:
        X, IEN, rho = PC.fixture(name)
    else:
        X, IEN = SMALL[name]()
        rho = PC.density("uniform", X, IEN)
    ref = P.dense_in_nodes(X, IEN, rho)
    got = oracle.dense_in_nodes(X, IEN, rho)
    ok = ~ref["undecidable"]
    f = _frac((got - ref["rho_n"])[ok], ref["bound"][ok])
    mv = P.mesh_volume(X, IEN, rho)
    vd, vf = (oracle.mesh_volume if IEN.shape[1] == 8 else oracle.mesh_volume_tet4)(X, IEN, rho)
    fv = max(_frac(vd - mv["V_domain"], mv["bound_domain"]), _frac(vf - mv["V_frac"], mv["bound_frac"]))
    print(f"PRE oracle {name}: nodal fraction of bound {f:.3g}, volume {fv:.3g}")
    assert f < 1.0 and fv < 1.0


@pytest.mark.parametrize("name", ISO_CASES)
def test_oracle_iso_volume_and_flagged_weight(oracle, name):
    X, IEN = SMALL[name]()
    vd = P.mesh_volume(X, IEN, np.ones(len(IEN)))["V_domain"]
    for field in ("reference", "clipped"):
        rn = nodal_field(X, IEN, field)
        used = np.unique(IEN) - 1
        lo, hi = rn[used].min(), rn[used].max()
        for thr in (lo - 0.1, lo, hi + 0.1, 0.0, 1.0, float(np.sort(rn[used])[len(used) // 2]), 0.5 * (lo + hi)):
            ref = P.isocontour_volume(X, IEN, rn, thr)
            assert ref["flagged"] <= WEIGHT_CAP * vd, (name, field, thr, ref["flagged"])
            assert _frac(oracle.isocontour_volume(X, IEN, rn, thr) - ref["volume"], ref["bound"]) < 1.0, (name, field, thr)


def nodal_field(X, IEN, kind):
    if kind == "reference":
        return P.dense_in_nodes(X, IEN, PC.density("binary", X, IEN))["rho_n"]
    c = X.mean(0)
    r = np.linalg.norm((X - c) / np.maximum(np.ptp(X, axis=0), 1e-300), axis=1)
    return np.clip(1.5 - 2.5 * r, 0.0, 1.0)


@pytest.mark.parametrize("name", ["hex7-j0.3-id", "tet5-j0.3-id", "holes"])
def test_threshold_targets_are_decidable_and_the_oracle_agrees(oracle, name):
    X, IEN = SMALL[name]()
    rn = nodal_field(X, IEN, "clipped")
    vmin, vmax = P.isocontour_volume(X, IEN, rn, 1.0)["volume"], P.isocontour_volume(X, IEN, rn, 0.0)["volume"]
    assert 0.0 < vmin < vmax
    target = vmin + 0.37 * (vmax - vmin)
    for tgt, tol, maxit in ((target, 1e-4, 60), (target, 0.0, 7), (target, 0.5, 60), (vmax * (1 - 1e-9), 1e-4, 5),
                            (vmin * (1 + 1e-9), 1e-4, 5)):
        r = P.find_threshold(X, IEN, rn, tgt, tol, maxit)
        assert r["decidable"], (name, tgt, tol, maxit)
        assert oracle.find_threshold(X, IEN, rn, tgt, tol, maxit) == (r["rho_t"], r["iters"])
    for tgt in (vmax * (1 + 1e-9), vmin * (1 - 1e-9)):
        with pytest.raises(P.OutOfRange):
            P.find_threshold(X, IEN, rn, tgt)
