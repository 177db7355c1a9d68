"""Cases and helpers of the row-walk plan tests (test_rbf_walk_plans_cpu.py / test_rbf_walk_plans_gpu.py).

rbf_walk_kernel (csrc/r2s_rbf_walk.hpp) walks L rows with an unrolled ring of five steps; rbf_walk_plan picks the
wavefronts per workgroup NW and L from the lattice size, and small lattices get L = 4: the fifth step of the ring, its
wrap, the table staging beyond four steps and most of the NW instantiations only run on production-sized lattices.  The
cases below reach them on small ones - by shape (narrow, deep lattices where the rule itself picks long walks) and through
the test hooks R2S_RBF_WALK_L / R2S_RBF_WALK_NW.  walk_plan() restates the rule so that the CPU test can show which plan a
case was chosen for; the GPU tests assert what r2s_last_rbf_plan reports, not this restatement.
"""
import functools

import numpy as np

import rbf_ref64 as ref
import vol_ref64
from test_rbf_reference_gpu import _banded_spheres, _check_coarse, _check_fine, _geom, _set_modes

THR = 1e-3                       # the walk exists for R = 2, tap_d2 = 7 only: kernel threshold 1e-3
LO, H = (0.013, -0.2, 0.07), 0.1037   # non-dyadic: several Float32 coordinate differences ("variants") per axis
WALK_W = 5                       # steps of the unrolled ring (2 R + 1)

NW_PRODUCT, NW_EVAL = (1, 2, 3, 5, 9), (1, 2, 4, 8)
STAGE_PRODUCT, STAGE_EVAL16, STAGE_EVAL64 = 420, 840, 3360   # 16-byte table chunks a workgroup stages per step


def walk_plan(nx, ny, nz, dpp, stage_chunks=None, nw=None, rows=None):
    """rbf_walk_plan restated -> (NW, L, nchunk, nxt); nw / rows: R2S_RBF_WALK_NW / R2S_RBF_WALK_L"""
    cand, outw = (NW_PRODUCT, 60) if dpp else (NW_EVAL, 64)
    stage_chunks = (STAGE_PRODUCT if dpp else STAGE_EVAL16) if stage_chunks is None else stage_chunks
    best, NW = -1.0, cand[0]
    for c in cand:
        waves = ((nx + outw * c - 1) // (outw * c)) * c
        cost = waves * (1.0 + 0.12 * ((stage_chunks + 64 * c - 1) // (64 * c)))
        if best < 0.0 or cost <= best:
            best, NW = cost, c
    if nw in cand:
        NW = nw
    nxt = (nx + outw * NW - 1) // (outw * NW)
    L = 32
    while L > 4 and nz * ((ny + L - 1) // L) * nxt < 2048:
        L //= 2
    if rows in (4, 8, 16, 32):
        L = rows
    return NW, L, (ny + L - 1) // L, nxt


def chunk_rows(ny, L):
    """rows of the walks of one plane"""
    return [min(L, ny - j0) for j0 in range(0, ny, L)]


# A: the rule's own long walks (dims, L, rows per walk): one wavefront, one workgroup per row, last walks of 5, 6 and 1
# rows - around the ring's five steps
NATURAL = [((5, 69, 1024), 32, [32, 32, 5]), ((5, 38, 700), 16, [16, 16, 6]), ((5, 33, 420), 8, [8, 8, 8, 8, 1])]

# B: forced L on wide, shallow lattices (dims, product NW, evaluation NW, product nxt): long walks with several
# wavefronts, the DPP halo lanes between them and partly filled last wavefronts.  ny = 33, 37, 41, 70 leave last walks
# of 1, 5, 9 and 6 rows at L = 32
FORCED = [((100, 37, 7), 2, 2, 1), ((130, 70, 6), 3, 4, 1), ((261, 41, 7), 5, 8, 1), ((365, 33, 6), 9, 8, 1),
          ((311, 70, 6), 3, 8, 2)]
FORCED_L = (8, 16, 32)

# C: every NW on one lattice at L = 32
NW_DIMS = (261, 41, 7)

# D: the 64-slot evaluation tables (more than 15 variants on an axis): (dims, lo, which table).  The output grid at
# smooth = 1 is rounded separately from the lattice (create_smooth_grid), so its differences against the lattice spread
# earlier than the lattice's own
WIDE = [((2000, 6, 6), (-0.37 * H, -0.2, 0.07), "fine"), ((10000, 5, 5), LO, "lattice")]

# plans of lattices the suite smoothed before these tests, read back (r2s_last_rbf_plan) with both hooks unset:
# dims -> (product NW, L, nxt), (evaluation NW, L, nxt)
SUITE_PLANS = {   # (the one lattice above L = 4: the evaluation of the large-paths `same` case, L = 8)
    (61, 7, 5): ((2, 4, 1), (1, 4, 1)),
    (130, 9, 8): ((3, 4, 1), (4, 4, 1)),
    (311, 6, 6): ((3, 4, 2), (8, 4, 1)),
    (64, 64, 5): ((2, 4, 1), (1, 4, 1)),
    (261, 41, 37): ((5, 4, 1), (8, 4, 1)),
    (539, 185, 43): ((9, 4, 1), (4, 8, 3)),
    (257, 91, 24): ((5, 4, 1), (8, 4, 1)),
}


def grid(pkg, dims, lo=LO):
    dims, lo = np.array(dims), np.array(lo)
    # (Grid rounds the cell counts of the shorter axes up: a hair short of whole cells, whatever dims.max() * H / dims.max() rounds to)
    cells = np.where(dims == dims.max(), dims - 1.0, dims - 1.0 - 1e-6)
    g = pkg.Grid(lo, lo + H * cells, int(dims.max()) - 1, 0)
    assert g.dims == tuple(int(d) for d in dims)
    return g


def set_hooks(monkeypatch, rows=None, nw=None):
    for name, v in (("R2S_RBF_WALK_L", rows), ("R2S_RBF_WALK_NW", nw)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _field(pkg, dims, lo, seed):
    g = grid(pkg, dims, lo)
    sdf, target = _banded_spheres(g, seed)
    return g, sdf, target


@functools.lru_cache(maxsize=None)
def approx_reference(pkg, dims, lo=LO, seed=None):
    """the field of a case and the float64 restatement of its approximation-mode smoothing (computed once, read only)"""
    g, sdf, target = _field(pkg, dims, lo, sum(dims) if seed is None else seed)
    caxes, taxes, sigma = _geom(g, 1)
    nx, ny, nz = g.dims
    w = ref.process_vector(sdf).reshape(nz, ny, nx)
    ec = ref.evaluate(w, caxes, caxes, 1, sigma, THR)
    ef = ref.evaluate(w, caxes, taxes, 1, sigma, THR)
    for a in (sdf, ec["val"], ec["S"], ef["val"], ef["S"]):
        a.setflags(write=False)
    return g, sdf, target, ec, ef, vol_ref64.coarse_edge(caxes[0])


@functools.lru_cache(maxsize=None)
def interp_reference(pkg, dims, lo=LO, seed=None):
    """the field of a case, the float64 kernel matrix of its lattice and the processed right-hand side"""
    g, sdf, target = _field(pkg, dims, lo, 7 * sum(dims) if seed is None else seed)
    caxes, _, sigma = _geom(g, 1)
    K = ref.kernel_matrix(caxes, sigma, THR)
    b = ref.process_vector(sdf).astype(np.float64)
    sdf.setflags(write=False)
    b.setflags(write=False)
    return g, sdf, target, K, b


def smooth_approx(pkg, case):
    """one approximation-mode smoothing under the current switches -> (fine, lsf, th, plan)"""
    g, sdf, target = case[0], case[1], case[2]
    info = {}
    fine = pkg.RBFs_smoothing(sdf, g, False, 1, target, THR, info=info)
    return fine, info["lsf"], info["th"], pkg.last_rbf_plan()


def check_level(lsf, th, edge, target, note):
    """_check_level of test_rbf_reference_gpu with the float64 volume (vol_ref64) in place of the oracle's: the oracle adds
    the cell volumes one after the other in Float32, and on these non-dyadic lattices of 10^5 cells that sum alone is off by
    more than the tolerance (353 k additions of the same Float32 edge^3 round the same way: 7e-4 of the volume on
    (5, 69, 1024)).  th in [-max lsf, -min lsf]; |V(lsf + th) - target| <= 1e-4 + the bound of the kernels' own Float32 sum,
    unless the 40 halvings ran out - then the target lies between the volumes a few ulp of th to either side"""
    assert -float(lsf.max()) <= th <= -float(lsf.min()), note
    level = np.float32(-th)
    V, b = vol_ref64.volume(lsf, edge, shift=level)
    if abs(V - target) <= vol_ref64.TOL + b:
        return
    delta = np.float32((float(lsf.max()) - float(lsf.min())) * 2.0 ** -39)
    lo, hi = level - delta, level + delta
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    (Vl, bl), (Vh, bh) = vol_ref64.volume(lsf, edge, shift=hi), vol_ref64.volume(lsf, edge, shift=lo)
    assert min(Vl, Vh) - max(bl, bh) <= target <= max(Vl, Vh) + max(bl, bh), (note, V, Vl, Vh, target)


def check_approx(pkg, monkeypatch, case, note, expect=None):
    """coarse LSF and fine field against the restatement under the default form (whose plan `expect` inspects) and under
    fly and lut -> (largest fraction of the bound, the default form's outputs)"""
    g, sdf, target, ec, ef, edge = case
    worst, default = 0.0, None
    for mode in ("default", "fly", "lut"):
        _set_modes(monkeypatch, mode)
        fine, lsf, th, plan = smooth_approx(pkg, case)
        if mode == "default":
            default = (fine, lsf, th)
            assert plan["evaluation"] == "walk" and plan["walk_ok"] and not plan["capped"], plan
            assert sum(v >= 3 for v in plan["variants"]) >= 2, plan      # real variants on at least two axes
            if expect is not None:
                expect(plan)
        else:
            assert plan["evaluation"] == mode, plan
        worst = max(worst, _check_coarse(lsf, ec, THR), _check_fine(fine, th, ef, THR))
        check_level(lsf, th, edge, target, (note, mode))
    _set_modes(monkeypatch, "default")
    return worst, default


def solve_interp(pkg, case):
    """interpolation mode under the current switches: the weights (r2s_rbf_field_fit) and the smoothing itself"""
    g, sdf, target = case[0], case[1], case[2]
    with pkg.fit_rbf_field(sdf, g, True, target, THR) as f:
        w, fit = f.weights, (f.cg_iterations, float(f.level_shift))
    info = {}
    fine = pkg.RBFs_smoothing(sdf, g, True, 1, target, THR, info=info)
    return dict(w=np.array(w), fit=fit, its=info["cg_iterations"], th=info["th"], lsf=info["lsf"], fine=fine, plan=pkg.last_rbf_plan())


def residual(case, w):
    """||K w - b|| / ||b|| in float64 with the restatement's matrix"""
    K, b = case[3], case[4]
    return float(np.linalg.norm(K @ w.astype(np.float64).ravel() - b) / np.linalg.norm(b))


def check_interp_run(case, r, note):
    n = case[1].size
    assert r["fit"] == (r["its"], r["th"]), (note, r["fit"], r["its"], r["th"])
    assert 0 < r["its"] < n, (note, r["its"])
    rel = residual(case, r["w"])
    assert rel <= 2 * float(ref.RTOL32), (note, rel, r["its"])
    return rel


def check_interp(pkg, monkeypatch, case, note, expect=None):
    """the product's forms follow the same numbers: weights, iterations, level shift, LSF and field bit-equal between the
    default form (the row walk) and fly / lut; the weights solve the restatement's system -> (residual / ||b||, default run)"""
    monkeypatch.delenv("R2S_RBF_APPLY", raising=False)
    monkeypatch.delenv("R2S_RBF_MATVEC", raising=False)
    d = solve_interp(pkg, case)
    assert d["plan"]["product"] == "walk" and d["plan"]["walk_ok"], d["plan"]
    if expect is not None:
        expect(d["plan"])
    rel = check_interp_run(case, d, note)
    for mode in ("fly", "lut"):
        monkeypatch.setenv("R2S_RBF_MATVEC", mode)
        o = solve_interp(pkg, case)
        assert o["plan"]["product"] == mode, o["plan"]
        assert o["plan"]["product_plan"] == d["plan"]["product_plan"]        # the grouping of the dot product's partial sums
        assert o["fit"] == d["fit"] and o["its"] == d["its"] and o["th"] == d["th"], (note, mode)
        for key in ("w", "lsf", "fine"):
            assert np.array_equal(o[key], d[key]), (note, mode, key)
    monkeypatch.delenv("R2S_RBF_MATVEC", raising=False)
    return rel, d
