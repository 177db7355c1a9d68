"""The float64 restatement of Sign_Detection (tests/sign_ref64.py) and the edge cases built on it
(tests/sign_cases.py), checked on the CPU: against the C oracle, against their own self-checks, against an analytic
inside and against the reference's known answers."""
import numpy as np
import pytest

import sign_cases as C
import sign_ref64 as R
from conftest import block_mesh, load_fixture

NAMES = C.case_names()


def _oracle_signs(oracle, c):
    og = oracle.grid_make(*c.grid_args)
    g = c.grid64()
    assert list(og.N) == list(g.N) and og.cell == g.cell and list(og.amin) == list(g.amin), "the two grids differ"
    assert g.ngp <= 48 ** 3
    return oracle.sign_detection(c.X, c.IEN, c.rho_n, c.rho_t, og)


def describe(c, v):
    """margin and winning candidate of voxel v, for a failure message"""
    ref, g = c.ref(), c.grid64()
    nx, ny, _ = g.dims
    sel = ref["pair_vox"] == v
    s = f"voxel {v} (i,j,k)=({v % nx},{(v // nx) % ny},{v // (nx * ny)}) margin {ref['margin'][v]:.3e} ref sign {ref['sign'][v]:+.0f}"
    if "winner" in ref:
        s += f" winner el {ref['winner'][v]} max|xi| {ref['winner_mx'][v]:.17g}"
        s += " candidates " + ", ".join(f"el {e}: {m:.17g} rho-rho_t {r - c.rho_t:.3e}" for e, m, r in
                                        zip(ref["pair_el"][sel], ref["pair_mx"][sel], ref["pair_rho"][sel]))
    else:
        s += " candidates " + ", ".join(f"el {e}: m {m:.3e} rho-rho_t {r - c.rho_t:.3e}" for e, m, r in
                                        zip(ref["pair_el"][sel], ref["pair_m"][sel], ref["pair_rho"][sel]))
    return s


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_oracle_where_decidable(oracle, name):
    c = C.cases()[name]
    s = _oracle_signs(oracle, c)
    assert set(np.unique(s)) <= {-1.0, 1.0}
    ok = ~c.undecidable()
    bad = np.nonzero(ok & (s != c.ref()["sign"]))[0]
    assert len(bad) == 0, f"{len(bad)} decidable voxels differ; first: " + "; ".join(describe(c, v) for v in bad[:3])


@pytest.mark.parametrize("name", NAMES)
def test_undecidable_share_within_cap(name):
    c = C.cases()[name]
    share = float(c.undecidable().mean())
    print(f"{name}: undecidable share {share:.6f} cap {c.cap}")
    assert c.kind == "knife" or c.cap == 0.0
    assert share <= c.cap


@pytest.mark.parametrize("name", [n for n in NAMES if C.cases()[n].check])
def test_case_reaches_what_it_exists_for(name):
    c = C.cases()[name]
    got = C.self_check(c)
    print(f"{name}: {got}")
    for key, least in c.check.items():
        assert got[key] >= least, (key, got[key], least)


def test_long_list_counted_from_the_oracle_grid(oracle):
    """the longest tile list of `long_lists_fine`, counted again without the restatement: the oracle's grid points
    against the elements' boxes, point by point; an element is listed by a 4x4x4 tile when its box holds one of the
    tile's points"""
    c = C.cases()["long_lists_fine"]
    og = oracle.grid_make(*c.grid_args)
    pts = oracle.grid_points(og)
    nx, ny, nz = og.dims
    Xe = c.X[c.IEN - 1]
    lo, hi = Xe.min(axis=1), Xe.max(axis=1)
    inside = np.all((lo[None, :, :] <= pts[:, None, :]) & (pts[:, None, :] <= hi[None, :, :]), axis=2)    # (ngp, nel)
    v = np.arange(len(pts))
    tile = (((v // (nx * ny)) // 4) * ((ny + 3) // 4) + ((v // nx) % ny) // 4) * ((nx + 3) // 4) + (v % nx) // 4
    longest = max(int(inside[tile == t].any(axis=0).sum()) for t in np.unique(tile))
    print("longest tile list", longest)
    assert longest > 64
    assert longest == C.tile_list_lengths(c).max()


def test_axis_aligned_cube_inflated_by_one_percent():
    """one element [-1,1]^3 * h + c: xi = (x - c) / h exactly, so `max|xi| < 1.01` is a cube of half-width 1.01 h"""
    h, ctr = 0.37, np.array([0.11, -0.23, 0.05])
    X, IEN = C.tensor_mesh(*[[ctr[a] - h, ctr[a] + h] for a in range(3)])
    # one lattice plane 0.4 % outside the cube on each side (inside the 1 % shell), the next one 3 % outside
    g = R.Grid64(ctr - 1.004 * h, ctr + 1.004 * h, 41, 2)
    for rho, rt, inside_sign in ((np.ones(8), 0.5, 1.0), (np.zeros(8), 0.5, -1.0)):
        ref = R.sign_hex8(X, IEN, rho, rt, g)
        xi = (g.points() - ctr) / h
        # the walk sees only lattice points inside the element's box, so the shell beyond the faces is never +1:
        # SignDetection.jl:30 picks candidates by `min <= x <= max`
        in_box = np.all((X.min(0) <= g.points()) & (g.points() <= X.max(0)), axis=1)
        want = np.where(in_box & (np.abs(xi).max(axis=1) < 1.01), inside_sign, -1.0)
        assert np.array_equal(ref["sign"], want)
        assert (ref["margin"] > R.DECIDABLE).all()
    # and the inverse map itself, on points out to the box of the reference's optimiser
    rng = np.random.default_rng(5)
    xi = rng.uniform(-1.1, 1.1, (4000, 3))
    got, found = R.hex8_inverse_map(np.broadcast_to(X[IEN[0] - 1], (4000, 8, 3)), ctr + h * xi)
    assert found.all() and np.abs(got - xi).max() < 1e-13
    got, found = R.hex8_inverse_map(np.broadcast_to(X[IEN[0] - 1], (8, 8, 3)), ctr + h * 1.2 * R._S)
    assert not found.any()


def test_twisted_inverse_map_round_trip():
    """x(xi) -> xi on the most distorted element of the cases, over the whole 1.01 box"""
    c = C.cases()["twisted_single_shear_taper"]
    Xe = c.X[c.IEN[0] - 1]
    xi = np.random.default_rng(6).uniform(-1.01, 1.01, (4000, 3))
    x = R.hex8_shape(xi) @ Xe
    got, found = R.hex8_inverse_map(np.broadcast_to(Xe, (4000, 8, 3)), x)
    assert found.all() and np.abs(got - xi).max() < 1e-11


def test_reference_known_answers(oracle):
    """the inputs of tests/test_oracle_golden.py (reference test/HexSphereSdfTest.jl, HexBlockSdfTest.jl).  Sphere: no
    voxel is undecidable and restatement and oracle give the same 365 positive voxels, the count behind the
    reference's mean.  Block: its nodal densities equal rho_t on whole faces, so 220 voxels hang on a rounding; the
    restatement reproduces the oracle on the decidable voxels only, and the two positive counts differ by no more
    than the undecidable ones."""
    X, IEN, rho = load_fixture("sphere")
    rn = oracle.dense_in_nodes(X, IEN, rho)
    Xb, IENb = block_mesh([2, 1, 1])
    rb = np.array([0.0, 0.0, 0.5, 0.5, 0.5, 0.5, 1.0, 1.0, 0.0, 0.0, 0.5, 0.5])
    for (Xm, Im, r, n_max, literal) in ((X, IEN, rn, 10, 365), (Xb, IENb, rb, 20, None)):
        g = R.Grid64(Xm.min(0), Xm.max(0), n_max, 3)
        og = oracle.grid_make(Xm.min(0), Xm.max(0), n_max)
        assert g.ngp == og.ngp
        ref = R.sign_hex8(Xm, Im, r, 0.5, g)
        s = oracle.sign_detection(Xm, Im, r, 0.5, og)
        ok = ref["margin"] > R.DECIDABLE
        assert np.array_equal(ref["sign"][ok], s[ok])
        n_ref, n_orc, n_und = int((ref["sign"] > 0).sum()), int((s > 0).sum()), int((~ok).sum())
        print(f"positive voxels: restatement {n_ref} oracle {n_orc} undecidable {n_und}")
        if literal is not None:
            assert n_und == 0 and n_ref == literal and n_orc == literal
        assert abs(n_ref - n_orc) <= n_und
