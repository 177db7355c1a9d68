"""The sign pass on the inputs where its shortcuts decide (tests/sign_cases.py): the half-space cull on twisted
elements, coord_range on bounds that are lattice coordinates, sign lists longer than 64, ties on shared faces, and
densities within a few margins of rho_t.  The C oracle is the comparator bit for bit; the float64 restatement
(tests/sign_ref64.py) on every voxel whose outcome does not hang on a rounding."""
import numpy as np
import pytest

import sign_cases as C
import sign_ref64 as R
from test_sign_edges_cpu import describe

pytestmark = pytest.mark.gpu

NAMES = C.case_names()
_RUNS = {}


def _run(pkg, oracle, name):
    """every product call of one case, made once and shared by the tests below (do not modify the arrays)"""
    if name in _RUNS:
        return _RUNS[name]
    import torch
    c = C.cases()[name]
    og = oracle.grid_make(*c.grid_args)
    pg = pkg.Grid(*c.grid_args)
    assert list(pg.N) == list(og.N) and pg.cell_size == og.cell and list(pg.AABB_min) == list(og.amin)
    mesh = pkg.Mesh(c.X, c.IEN)
    r = dict(case=c, oracle=oracle.sign_detection(c.X, c.IEN, c.rho_n, c.rho_t, og))
    r["st"], r["st_ni"] = {}, {}
    r["sign"] = pkg.Sign_Detection(mesh, pg, c.rho_n, c.rho_t, stats=r["st"])
    r["sign_ni"] = pkg.Sign_Detection(mesh, pg, c.rho_n, c.rho_t, stats=r["st_ni"], sign_no_inner=True)
    r["sdf"] = pkg.sdf_fused(mesh, pg, c.rho_n, c.rho_t)
    r["sdf_ni"] = pkg.sdf_fused(mesh, pg, c.rho_n, c.rho_t, sign_no_inner=True)
    r["dist"], _ = pkg.evalDistances(mesh, pg, c.rho_n, c.rho_t, want_xp=False)
    # device path: every output at once, twice on one plan, then 2 and 3 Z-slabs
    dev = torch.device("cuda:0")
    dX, dI, dR = (torch.from_numpy(a).to(dev) for a in (c.X, c.IEN, c.rho_n))
    nx, ny, nz = pg.dims
    plan = pkg.DevicePlan(0)

    def call(a=0, b=nz):
        o = {k: torch.empty((b - a) * ny * nx * (3 if k == "xp" else 1), dtype=torch.float64, device=dev)
             for k in ("dist", "sign", "sdf", "xp")}
        plan.run(dX, dI, dR, c.rho_t, pg, k_begin=a, k_end=b, **o)
        return {k: v.cpu().numpy() for k, v in o.items()}
    r["all1"], r["all2"] = call(), call()
    r["slabs"] = {}
    for parts in (2, 3):
        bounds = sorted(set(round(nz * p / parts) for p in range(parts + 1)))
        pieces = [call(a, b) for a, b in zip(bounds[:-1], bounds[1:])]
        r["slabs"][parts] = {k: np.concatenate([p[k] for p in pieces]) for k in ("sign", "sdf", "dist")}
    plan.close()
    _RUNS[name] = r
    return r


def _same(got, want, c, what):
    bad = np.nonzero(got != want)[0]
    msg = ""
    if len(bad):
        msg = f"{c.name}: {what}: {len(bad)} of {len(want)} voxels differ; " + "; ".join(
            describe(c, v) + f" got {got[v]:+.0f} want {want[v]:+.0f}" for v in bad[:4])
        print(msg)
    assert len(bad) == 0, msg


@pytest.mark.parametrize("name", NAMES)
def test_signs_equal_oracle(pkg, oracle, name):
    """default parameters and sign_no_inner, bit for bit"""
    r = _run(pkg, oracle, name)
    assert set(np.unique(r["sign"])) <= {-1.0, 1.0}
    _same(r["sign"], r["oracle"], r["case"], "Sign_Detection vs oracle")
    _same(r["sign_ni"], r["oracle"], r["case"], "Sign_Detection(sign_no_inner) vs oracle")


@pytest.mark.parametrize("name", NAMES)
def test_inner_shortcut_changes_nothing(pkg, oracle, name):
    """every case is a conforming mesh: the shortcut for points deep inside one-sided elements must not show"""
    r = _run(pkg, oracle, name)
    _same(r["sign"], r["sign_ni"], r["case"], "default vs sign_no_inner")
    assert np.array_equal(np.signbit(r["sdf"]), np.signbit(r["sdf_ni"]))


@pytest.mark.parametrize("name", NAMES)
def test_fused_and_all_outputs(pkg, oracle, name):
    r = _run(pkg, oracle, name)
    c, neg = r["case"], r["oracle"] < 0
    _same(np.where(np.signbit(r["sdf"]), -1.0, 1.0), r["oracle"], c, "sign bit of sdf_fused vs oracle")
    _same(np.where(np.signbit(r["sdf_ni"]), -1.0, 1.0), r["oracle"], c, "sign bit of sdf_fused(sign_no_inner) vs oracle")
    a = r["all1"]
    _same(a["sign"], r["oracle"], c, "sign of the all-outputs call vs oracle")
    assert np.array_equal(np.signbit(a["sdf"]), neg)
    # sdf == dist * sign, on the host entry points and inside the all-outputs call
    assert np.array_equal(r["sdf"], r["dist"] * r["sign"])
    assert np.array_equal(a["sdf"], a["dist"] * a["sign"])
    assert np.array_equal(a["dist"], r["dist"]) and np.array_equal(a["sdf"], r["sdf"])


@pytest.mark.parametrize("name", NAMES)
def test_second_call_on_the_plan(pkg, oracle, name):
    """the second call runs with speculated sizes and the early projection launch"""
    r = _run(pkg, oracle, name)
    for k in ("sign", "sdf", "dist", "xp"):
        assert np.array_equal(r["all1"][k], r["all2"][k]), k


@pytest.mark.parametrize("name", NAMES)
def test_slabs_equal_one_call(pkg, oracle, name):
    r = _run(pkg, oracle, name)
    for parts, s in r["slabs"].items():
        _same(s["sign"], r["all1"]["sign"], r["case"], f"{parts} Z-slabs vs one call")
        assert np.array_equal(s["sdf"], r["all1"]["sdf"]) and np.array_equal(s["dist"], r["all1"]["dist"])


@pytest.mark.parametrize("name", NAMES)
def test_signs_equal_restatement_where_decidable(pkg, oracle, name):
    r = _run(pkg, oracle, name)
    c = r["case"]
    ok = ~c.undecidable()
    ref = c.ref()["sign"]
    _same(np.where(ok, r["sign"], ref), ref, c, "Sign_Detection vs float64 restatement")
    _same(np.where(ok, r["sign_ni"], ref), ref, c, "Sign_Detection(sign_no_inner) vs float64 restatement")


@pytest.mark.parametrize("name", NAMES)
def test_sign_pass_did_real_work(pkg, oracle, name):
    """a +1 voxel can only come out of the sign kernels: where the oracle has one, tiles and list entries are non-zero.
    r2s_stats has no longest-list figure, but the longest list is at least the mean one: for long_lists_fine the mean
    itself exceeds 64 (test_sign_edges_cpu.py::test_case_reaches_what_it_exists_for counts the longest on the CPU)."""
    r = _run(pkg, oracle, name)
    print(name, {k: r["st"][k] for k in ("n_sign_entries", "n_active_sign_tiles", "n_tiles")})
    if (r["oracle"] > 0).any():
        for st in (r["st"], r["st_ni"]):
            assert st["n_active_sign_tiles"] > 0 and st["n_sign_entries"] > 0
    if name == "long_lists_fine":
        assert r["st"]["n_sign_entries"] > 64 * r["st"]["n_active_sign_tiles"]
