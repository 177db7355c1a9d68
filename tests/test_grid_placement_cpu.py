"""The reference conditions that tests/test_grid_placement_gpu.py rests on, proven on the CPU oracle alone, so that the GPU
test never asks the kernels for more than the oracle delivers:

* for every window of grid_placement_cases.WINDOWS and both element types, dist * sign and the projection points of the
  oracle on the window are bit-equal to the crop of its full-grid result; outside the full grid everything is the sentinel
  (-1e10, projection point zero);
* HEX8 only: the oracle at scale 2^-10 and 2^10, divided by the scale, is bit-equal to the unscaled run.

No other equivariance holds, and none is asserted.  Measured on this mesh with the oracle (voxels that differ by more than
1e-6 relative from the untransformed run, distances of exactly 0 included; signs compared exactly):

* HEX8, power-of-two scales 2^-30, 2^-10, 2^10, 2^30: every voxel bit-equal after unscaling;
* TET4, scale 2^10: 773 of 46 656 voxels differ - the TET4 restatement works with absolute tolerances;
* shift 64: 947 HEX8 and 1 597 TET4 voxels differ; shift 4096: 1 HEX8 sign differs; shift 2^20: 618 TET4 signs differ.

Away from the origin many voxels therefore sit on tolerance edges, where a kernel that contracts a multiply-add or reorders
a sum the oracle does not takes a different branch: the GPU file holds the kernels to the oracle on exactly those inputs.
"""
import numpy as np
import pytest

import grid_placement_cases as C

KINDS = ("hex8", "tet4")


def _oracle_fields(oracle, X, IEN, rn, g):
    """(dist * sign, xp, dist) of the oracle on grid g, as (nz, ny, nx[, 3]) arrays"""
    nx, ny, nz = g.dims
    d, xp, _ = oracle.eval_distances(X, IEN, rn, C.RHO_T, g, C.BAND_FACTOR)
    s = oracle.sign_detection(X, IEN, rn, C.RHO_T, g)
    return (d * s).reshape(nz, ny, nx), xp.reshape(nz, ny, nx, 3), d.reshape(nz, ny, nx)


@pytest.fixture(scope="module")
def full(oracle):
    out = {}
    for kind in KINDS:
        X, IEN, rn = C.mesh(kind)
        out[kind] = _oracle_fields(oracle, X, IEN, rn, C.full_grid(oracle.grid_make))
        for a in out[kind]:
            a.setflags(write=False)
    return out


def test_full_grid_and_windows_are_what_the_cases_say(oracle):
    g = C.full_grid(oracle.grid_make)
    assert g.dims == C.FULL_DIMS and g.cell == C.CELL and np.array_equal(np.array(g.amin[:]), C.AMIN_FULL)
    X, _, _ = C.mesh("hex8")
    assert np.array_equal(X * 2.0 ** 20, np.round(X * 2.0 ** 20)) and X.min() == -1.0 and X.max() == 1.0
    pf = oracle.grid_points(g).reshape(39, 39, 39, 3)
    for name in C.WINDOWS:
        w = C.window_grid(oracle.grid_make, name)
        nz, ny, nx = C.dims3(name)
        assert w.dims == (nx, ny, nz)
        ov = C.overlap(name)
        assert (ov is None) == (name in C.EMPTY_WINDOWS)
        if ov is not None:   # the same doubles
            pw = oracle.grid_points(w).reshape(nz, ny, nx, 3)
            assert np.array_equal(C.bits(pw[ov[0]]), C.bits(pf[ov[1]])), name
    residues = {tuple(o % 4 for o in C.WINDOWS[f"align{r}"][0]) for r in range(4)}
    assert residues == {(0, 1, 2), (1, 3, 1), (2, 1, 0), (3, 3, 3)}   # x: all four residues, y: 1 and 3, z: all four


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(C.WINDOWS))
def test_oracle_on_a_window_equals_the_crop_of_the_full_grid(oracle, full, kind, name):
    X, IEN, rn = C.mesh(kind)
    sdf, xp, dist = _oracle_fields(oracle, X, IEN, rn, C.window_grid(oracle.grid_make, name))
    ov = C.overlap(name)
    outside = np.ones(sdf.shape, dtype=bool)
    n_band = 0
    if ov is not None:
        fsdf, fxp, fdist = full[kind]
        neq = int((C.bits(sdf[ov[0]]) != C.bits(fsdf[ov[1]])).sum())
        neq_xp = int((C.bits(xp[ov[0]]) != C.bits(fxp[ov[1]])).any(axis=-1).sum())
        assert neq == 0 and neq_xp == 0, (name, kind, neq, neq_xp)
        outside[ov[0]] = False
        n_band = int((dist[ov[0]] < 1e9).sum())
    assert np.all(sdf[outside] == -1.0e10) and not xp[outside].any(), (name, kind)
    print(f"{name} {kind}: {sdf.size} voxels, {int((~outside).sum())} on the full grid, {n_band} band voxels, neq 0")
    # what the table of the cases promises
    if name == "interior":
        assert n_band == sdf.size == 2210
    if name == "corner-out":
        assert int((~outside).sum()) == 1404
    if name == "superset":
        assert int((~outside).sum()) == 39 ** 3
    if name == "thin":
        assert n_band == sdf.size == 578 and sdf.shape[0] == 2
    if name.startswith("align"):
        assert n_band == sdf.size == 3360
    if name in C.EMPTY_WINDOWS:
        assert outside.all()


@pytest.mark.parametrize("tname", C.EXACT_SCALES)
def test_oracle_hex8_is_equivariant_under_power_of_two_scaling(oracle, full, tname):
    sc = C.TRANSFORMS[tname][0]
    X, IEN, rn, lo, hi = C.transformed("hex8", tname)
    g = oracle.grid_make(lo, hi, C.FULL_N_MAX, C.FULL_MARGIN)
    assert g.dims == C.FULL_DIMS and g.cell == C.CELL * sc
    sdf, xp, dist = _oracle_fields(oracle, X, IEN, rn, g)
    fsdf, fxp, fdist = full["hex8"]
    real = fdist < 1e9
    assert np.array_equal(dist < 1e9, real)
    assert np.array_equal(C.bits(sdf[~real]), C.bits(fsdf[~real]))                 # +-1e10 does not scale
    assert np.array_equal(C.bits(sdf[real] / sc), C.bits(fsdf[real]))
    assert np.array_equal(C.bits(xp / sc), C.bits(fxp))
