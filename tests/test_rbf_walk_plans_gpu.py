"""The row-walk kernels (csrc/r2s_rbf_walk.hpp) at the walk lengths, workgroup widths and table widths of production
lattices, on small ones (rbf_walk_cases.py says how each case gets there).

Every case asserts from r2s_last_rbf_plan that it ran the plan it was chosen for, then compares with the float64
restatement (rbf_ref64): approximation mode (the evaluation, MODE 1) per voxel within rbf_ref64.bound / fine_bound;
interpolation mode (the CG product, MODE 0, and the partial sums of its dot product) by the residual of the weights against
rbf_ref64.kernel_matrix - the bar 2 sqrt(eps(Float32)) ||b|| of test_rbf_interpolation_residual - and bit for bit against
the other forms of the product.  No field here needed another seed to meet that bar."""
import numpy as np
import pytest

import rbf_ref64 as ref
import rbf_walk_cases as C
from conftest import load_fixture
from test_rbf_reference_gpu import _check_fine, _geom

pytestmark = pytest.mark.gpu


def _expect(product=None, evaluation=None, rows=None, nxt=None):
    def check(plan):
        pp, ep = plan["product_plan"], plan["evaluation_plan"]
        if product is not None:
            assert pp["NW"] == product, plan
        if evaluation is not None:
            assert ep["NW"] == evaluation and plan["wa_nv"] == 16, plan
        if rows is not None:
            assert ep["L"] == rows and (product is None or pp["L"] == rows), plan
        if nxt is not None:
            assert pp["nxt"] == nxt, plan
    return check


# ---- A: the rule's own long walks ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,rows,chunks", C.NATURAL)
def test_natural_long_walks_approximation(pkg, monkeypatch, dims, rows, chunks):
    """narrow, deep lattices: the rule picks L = 32 / 16 / 8 itself; one wavefront, full walks and a short last one"""
    C.set_hooks(monkeypatch)
    assert C.chunk_rows(dims[1], rows) == chunks and max(chunks) == rows and chunks[-1] < rows
    worst, _ = C.check_approx(pkg, monkeypatch, C.approx_reference(pkg, dims), dims, _expect(evaluation=1, rows=rows))
    print(f"natural {dims} L={rows} approximation: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()


@pytest.mark.parametrize("dims,rows,chunks", C.NATURAL)
def test_natural_long_walks_interpolation(pkg, monkeypatch, dims, rows, chunks):
    C.set_hooks(monkeypatch)
    rel, d = C.check_interp(pkg, monkeypatch, C.interp_reference(pkg, dims), dims, _expect(product=1, evaluation=1, rows=rows, nxt=1))
    print(f"natural {dims} L={rows} interpolation: residual {rel:.3g} of ||b||, {d['its']} iterations")
    pkg._lib.lib().r2s_release_cache()


# ---- B: forced L on wide lattices ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", C.FORCED_L)
@pytest.mark.parametrize("dims,nw_product,nw_eval,nxt", C.FORCED)
def test_forced_long_walks_approximation(pkg, monkeypatch, dims, nw_product, nw_eval, nxt, rows):
    """R2S_RBF_WALK_L on wide, shallow lattices: long walks in workgroups of several wavefronts"""
    C.set_hooks(monkeypatch, rows=rows)
    chunks = C.chunk_rows(dims[1], rows)
    assert max(chunks) == rows and chunks[-1] < rows
    worst, _ = C.check_approx(pkg, monkeypatch, C.approx_reference(pkg, dims), (dims, rows), _expect(evaluation=nw_eval, rows=rows))
    print(f"forced {dims} L={rows} approximation: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()


@pytest.mark.parametrize("rows", C.FORCED_L)
@pytest.mark.parametrize("dims,nw_product,nw_eval,nxt", C.FORCED)
def test_forced_long_walks_interpolation(pkg, monkeypatch, dims, nw_product, nw_eval, nxt, rows):
    """the DPP product with its halo lanes between wavefronts (nxt = 2: between workgroups) over long walks"""
    C.set_hooks(monkeypatch, rows=rows)
    rel, d = C.check_interp(pkg, monkeypatch, C.interp_reference(pkg, dims), (dims, rows),
                            _expect(product=nw_product, evaluation=nw_eval, rows=rows, nxt=nxt))
    print(f"forced {dims} L={rows} interpolation: residual {rel:.3g} of ||b||, {d['its']} iterations")
    pkg._lib.lib().r2s_release_cache()


def test_walk_length_hook_ignores_other_values(pkg, monkeypatch):
    """R2S_RBF_WALK_L accepts 4, 8, 16, 32; anything else leaves the rule's choice"""
    case = C.approx_reference(pkg, (100, 37, 7))
    C.set_hooks(monkeypatch)
    want = C.smooth_approx(pkg, case)
    assert want[3]["evaluation_plan"] == dict(NW=2, L=4, nxt=1)
    for v in ("5", "64", "0", "-8", "x", ""):
        monkeypatch.setenv("R2S_RBF_WALK_L", v)
        got = C.smooth_approx(pkg, case)
        assert got[3] == want[3], v
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    pkg._lib.lib().r2s_release_cache()


# ---- C: every NW ------------------------------------------------------------------------------------------------------------

def test_every_workgroup_width_approximation(pkg, monkeypatch):
    """the evaluation does not depend on NW: under every forced NW, L = 32, lsf, field and level shift are those of the
    unforced run bit for bit (and that run meets the restatement)"""
    case = C.approx_reference(pkg, C.NW_DIMS)
    C.set_hooks(monkeypatch, rows=32)
    worst, want = C.check_approx(pkg, monkeypatch, case, C.NW_DIMS, _expect(evaluation=8, rows=32))
    seen = set()
    for nw in sorted(set(C.NW_PRODUCT + C.NW_EVAL)):
        C.set_hooks(monkeypatch, rows=32, nw=nw)
        fine, lsf, th, plan = C.smooth_approx(pkg, case)
        ep = plan["evaluation_plan"]
        assert ep["L"] == 32 and ep["NW"] == (nw if nw in C.NW_EVAL else 8) and plan["wa_nv"] == 16, plan
        assert ep["nxt"] == -(-C.NW_DIMS[0] // (64 * ep["NW"])), plan
        seen.add(ep["NW"])
        assert np.array_equal(fine, want[0]) and np.array_equal(lsf, want[1]) and th == want[2], nw
    assert seen == set(C.NW_EVAL)
    print(f"every NW {C.NW_DIMS} approximation: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()


@pytest.mark.parametrize("nw", C.NW_PRODUCT)
def test_every_workgroup_width_interpolation(pkg, monkeypatch, nw):
    """the product under every NW of the DPP form at L = 32: the partial sums of the dot product regroup with NW, so the CG
    results are held to the restatement's residual, not to each other; the other forms follow the regrouped sums bit for bit"""
    C.set_hooks(monkeypatch, rows=32, nw=nw)
    nxt = -(-C.NW_DIMS[0] // (60 * nw))
    rel, d = C.check_interp(pkg, monkeypatch, C.interp_reference(pkg, C.NW_DIMS), (C.NW_DIMS, nw), _expect(product=nw, rows=32, nxt=nxt))
    print(f"NW={nw} {C.NW_DIMS} interpolation: residual {rel:.3g} of ||b||, {d['its']} iterations")
    pkg._lib.lib().r2s_release_cache()


# ---- D: the 64-slot evaluation tables --------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [None, 32])
@pytest.mark.parametrize("dims,lo,which", C.WIDE)
def test_wide_tables_approximation(pkg, monkeypatch, dims, lo, which, rows):
    """axes long enough for more than 15 variants: the evaluation walks with NV = 64 tables (of the output grid, which is
    rounded separately; of the lattice itself, where the product no longer has a table)"""
    C.set_hooks(monkeypatch, rows=rows)

    def expect(plan):
        if which == "fine":
            assert plan["wa_nv_fine"] == 64 and max(plan["variants_fine"]) > 15, plan
        else:
            assert plan["wa_nv"] == 64 and max(plan["variants"]) > 15, plan
        if rows is not None:
            assert plan["evaluation_plan"]["L"] == rows, plan
    worst, _ = C.check_approx(pkg, monkeypatch, C.approx_reference(pkg, dims, lo), (dims, rows), expect)
    if which == "lattice":   # interpolation mode would take the materialised matrix here
        g, sdf, target = C.approx_reference(pkg, dims, lo)[:3]
        with pkg.fit_rbf_field(sdf, g, True, target, C.THR):
            assert pkg.last_rbf_plan()["product"] == "k"
    print(f"wide {dims} ({which}) L={rows} approximation: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()


# ---- E: Z-slabs --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rbf_grid", ["same", "fine"])
def test_slabs_long_walks(pkg, monkeypatch, rbf_grid):
    """r2s_rho2sdf on the beam at L = 32: 3 slab devices (R2S_MULTI_OVERSUBSCRIBE) equal one device bit for bit in
    interpolation mode (the walk over k_begin / k_end with clamped halo planes, its partial sums cut like the one-device
    run's), and the one-device field of an approximation-mode run meets the restatement on the call's own sdf_dists"""
    monkeypatch.setenv("R2S_MULTI_OVERSUBSCRIBE", "1")
    C.set_hooks(monkeypatch, rows=32)
    X, IEN, rho = load_fixture("beam_vfrac_04")
    pg = pkg.noninteractive_sdf_grid_setup(pkg.Mesh(X, IEN))
    smooth = 1 if rbf_grid == "same" else 2
    opts = pkg.Rho2sdfOptions(threshold_density=0.518555, rbf_interp=True, rbf_grid=rbf_grid, rbf_kernel_threshold=C.THR)
    ia, ib = {}, {}
    a = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=pg, info=ia)
    plan = pkg.last_rbf_plan()
    assert plan["product"] == "walk" and plan["evaluation"] == "walk", plan
    assert plan["product_plan"]["L"] == 32 and plan["evaluation_plan"]["L"] == 32, plan
    assert sum(v >= 3 for v in plan["variants"]) >= 2, plan
    b = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=pg, n_gpus=3, info=ib)
    assert 0 < ia["cg_iters"] == ib["cg_iters"] and ia["level_shift"] == ib["level_shift"]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[0], b[0])
    opts = pkg.Rho2sdfOptions(threshold_density=0.518555, rbf_interp=False, rbf_grid=rbf_grid, rbf_kernel_threshold=C.THR)
    ic = {}
    c = pkg.rho2sdf("t", X, IEN, rho, options=opts, sdf_grid=pg, info=ic)
    assert pkg.last_rbf_plan()["evaluation_plan"]["L"] == 32
    caxes, taxes, sigma = _geom(pg, smooth)
    nx, ny, nz = pg.dims
    w = ref.process_vector(c[3]).reshape(nz, ny, nx)
    ef = ref.evaluate(w, caxes, taxes, smooth, sigma, C.THR)
    worst = _check_fine(c[0], ic["level_shift"], ef, C.THR)
    print(f"slabs at L=32, {rbf_grid}: largest fraction of the bound {worst:.3g}")
    pkg._lib.lib().r2s_release_cache()
