"""The plan arithmetic behind the cases of test_rbf_walk_plans_gpu.py, without a GPU: which wavefronts per workgroup, rows
per walk and walks per plane rbf_walk_plan (csrc/r2s_rbf_walk.hpp, restated in rbf_walk_cases.walk_plan) gives each case,
and that the plans of lattices the suite smoothed before stay what the library reported for them."""
import os
import re
import threading

import rbf_walk_cases as C
from conftest import ROOT


def test_natural_cases_take_long_walks_by_the_rule():
    for dims, rows, chunks in C.NATURAL:
        for dpp in (True, False):
            assert C.walk_plan(*dims, dpp) == (1, rows, len(chunks), 1), dims
        assert C.chunk_rows(dims[1], rows) == chunks
        assert chunks[0] == rows > C.WALK_W - 1                   # a full walk passes the ring's last step and wraps
    assert [c[2][-1] for c in C.NATURAL] == [5, 6, 1]             # last walks of W, W + 1 and one row
    assert sorted(c[1] for c in C.NATURAL) == [8, 16, 32]
    for dims, _, _ in C.NATURAL:
        assert dims[0] * dims[1] * dims[2] < 400_000


def test_forced_cases_reach_every_workgroup_width():
    last = {}
    for dims, nw_product, nw_eval, nxt in C.FORCED:
        assert dims[0] * dims[1] * dims[2] <= 131_000
        assert C.walk_plan(*dims, True)[:2] == (nw_product, 4) and C.walk_plan(*dims, True)[3] == nxt   # L = 4 by the rule
        assert C.walk_plan(*dims, False)[:2] == (nw_eval, 4)
        for rows in C.FORCED_L:
            for dpp, nw in ((True, nw_product), (False, nw_eval)):
                p = C.walk_plan(*dims, dpp, rows=rows)
                assert p[:3] == (nw, rows, -(-dims[1] // rows)), (dims, rows)      # nchunk follows the forced L
            ch = C.chunk_rows(dims[1], rows)
            assert sum(ch) == dims[1] and ch[0] == rows and 0 < ch[-1] < rows
        last[dims[1]] = C.chunk_rows(dims[1], 32)[-1]
    assert last == {37: 5, 70: 6, 41: 9, 33: 1}
    assert {c[1] for c in C.FORCED} | {1} == set(C.NW_PRODUCT)       # NW = 1: the natural cases
    assert {c[2] for c in C.FORCED} | {1} == set(C.NW_EVAL)
    assert 65 <= C.FORCED[0][0][0] <= 128                               # the evaluation's NW = 2 lies there only
    assert any(c[3] == 2 for c in C.FORCED)                             # a row in two workgroups: halo lanes across them


def test_forced_widths_on_one_lattice():
    nx, ny, nz = C.NW_DIMS
    assert C.NW_DIMS in [c[0] for c in C.FORCED]
    for nw in C.NW_PRODUCT:
        assert C.walk_plan(nx, ny, nz, True, nw=nw, rows=32) == (nw, 32, 2, -(-nx // (60 * nw)))
        natural = C.walk_plan(nx, ny, nz, False)[0]
        assert C.walk_plan(nx, ny, nz, False, nw=nw, rows=32)[0] == (nw if nw in C.NW_EVAL else natural)
    for nw in C.NW_EVAL:
        assert C.walk_plan(nx, ny, nz, False, nw=nw, rows=32) == (nw, 32, 2, -(-nx // (64 * nw)))


def test_hooks_ignore_other_values():
    for dims in [c[0] for c in C.FORCED] + [c[0] for c in C.NATURAL]:
        for dpp in (True, False):
            want = C.walk_plan(*dims, dpp)
            for rows in (0, 5, 64, -8):
                assert C.walk_plan(*dims, dpp, rows=rows) == want
            for nw in (0, 6, 7, 16):
                assert C.walk_plan(*dims, dpp, nw=nw) == want


def test_suite_plans_are_unchanged():
    """with both hooks unset the rule gives the lattices of the older tests the plans the library reported for them
    (r2s_last_rbf_plan on an MI355X)"""
    for dims, (product, evaluation) in C.SUITE_PLANS.items():
        p, e = C.walk_plan(*dims, True), C.walk_plan(*dims, False)
        assert (p[0], p[1], p[3]) == product and (e[0], e[1], e[3]) == evaluation, dims


def test_wide_cases_stay_small():
    for dims, lo, which in C.WIDE:
        assert dims[0] * dims[1] * dims[2] <= 500_000 and which in ("fine", "lattice")
        for stage in (C.STAGE_EVAL16, C.STAGE_EVAL64):
            assert C.walk_plan(*dims, False, stage)[0] == 8


def test_hooks_are_read_per_call_and_documented():
    src = open(os.path.join(ROOT, "rho2sdf.jl_amd", "csrc", "r2s_rbf_walk.hpp")).read()
    for name in ("R2S_RBF_WALK_NW", "R2S_RBF_WALK_L"):
        lines = [ln for ln in src.splitlines() if f'getenv("{name}")' in ln]
        assert len(lines) == 1 and "static" not in lines[0], name
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "R2S_RBF_WALK_L" in integ and "R2S_RBF_WALK_NW" in integ
    assert re.search(r"void\s+r2s_last_rbf_plan\s*\(\s*int32_t\s+out\[12\]\s*\)\s*;", open(os.path.join(ROOT, "include", "rho2sdf_hip.h")).read())


def test_read_back_before_any_smoothing(pkg):
    """a thread that has smoothed nothing reads zeros"""
    got = {}
    t = threading.Thread(target=lambda: got.update(pkg.last_rbf_plan()))
    t.start()
    t.join()
    assert got["product_plan"] == dict(NW=0, L=0, nxt=0) == got["evaluation_plan"]
    assert got["wa_nv"] == 0 and got["wa_nv_fine"] == 0 and got["variants"] == (0, 0, 0) == got["variants_fine"]
    assert "last_rbf_plan" in pkg.__all__
