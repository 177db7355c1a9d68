"""The Float64 sums of mesh shells, orient, sections and holes against tests/segsum_ref.py, BIT FOR BIT: the per-item terms of
the tools' restatements (tests/mesh_*_ref*.py, numpy float64 in the header's operation order), laid out in the device's output
order, go through the one restatement of the block tree, the slot rule and the combine.  The shapes are the smallest at which the
shared summation code (ms_block_sum, ms_combine_kernel in r2s_mesh_graph.hpp) can go wrong:

    one255 / one256 / one257   one segment that ends before, at and behind the first block edge
    mixed                      segments of 10, 20, 700, 30 and 5 items: several inside one block, one across three blocks with
                               others on either side in the same blocks (the slot block + segment)
    one16385                   65 blocks: the first segment whose combine lanes add two block partials (chunk = 2)
    one32769                   129 blocks: chunk = 3, 43 lanes, the last lane's run is short
    and one case of the tool's own with many small segments, one-item segments among them

A one-item segment shows a term's own bits (no addition touches it), so a column that fails there does not agree with numpy as
a term; every column agreed on the MI355X, the square roots included, and all are asserted."""
import numpy as np
import pytest

import mesh_holes_cases as CH
import mesh_holes_ref as RH
import mesh_orient_cases as CO
import mesh_sections_cases as CX
import mesh_sections_ref64 as RX
import mesh_shells_cases as S
import mesh_shells_ref64 as RS
from segsum_ref import segsum

pytestmark = pytest.mark.gpu

MIXED = (10, 20, 700, 30, 5)
SHAPES = ("one255", "one256", "one257", "mixed", "one16385", "one32769", "own")


def _sizes(shape):
    return MIXED if shape == "mixed" else (int(shape[3:]),)


def _strip(n, alternating=False):
    """exactly n triangles of S.ribbon's strip (every second one reversed: the orient's signs alternate)"""
    V, T = CO.ribbon_alternating(n + 1) if alternating else S.ribbon(n + 1)
    return V, np.ascontiguousarray(T[:n])


def _equal_bits(label, got, want, names):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, label
    same = got.view(np.uint64) == want.view(np.uint64)
    bad = [names[q] for q in range(got.shape[1]) if not same[:, q].all()]
    worst = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if got.size else 0.0
    print(f"SEGSUM {label}: {got.shape[0]} segments, columns that differ in bits: {bad or 'none'}, largest relative difference {worst:.3e}")
    assert not bad, (label, bad)


@pytest.mark.parametrize("shape", SHAPES)
def test_shells_sums_are_the_restated_tree(pkg, shape):
    if shape == "own":
        V, T = S.case("fans")                                # shells of 1 .. 400 triangles, a one-triangle shell first
    elif shape in ("one16385", "one32769"):
        V, T = _strip(_sizes(shape)[0])
    else:
        V, T = S.join(*[_strip(n) for n in _sizes(shape)])
    o = pkg.mesh_shells(V, T)
    if shape != "own":
        assert o.n_tris.tolist() == list(_sizes(shape))
    order = np.argsort(o.shell_of_tri, kind="stable")        # ascending triangle index within a shell
    order = order[o.shell_of_tri[order] >= 0]
    starts = np.concatenate([[0], np.cumsum(o.n_tris)])
    x, _ = RS.terms(V, T, o.ref_point)
    _equal_bits(f"shells {shape}", o.sums, segsum(x[order], starts), RS.NAMES)


@pytest.mark.parametrize("shape", SHAPES)
def test_orient_volume_is_the_restated_tree(pkg, shape):
    if shape == "own":
        V, T = CO.case("fans40", True)
    elif shape in ("one16385", "one32769"):
        V, T = CO.case("ribbon" + shape[3:])
    else:
        V, T = S.join(*[_strip(n, True) for n in _sizes(shape)])
    o = pkg.mesh_orient(V, T)
    if shape != "own":
        assert o.counts[:, 1].tolist() == list(_sizes(shape))
    patch, flipped = np.asarray(o.patch_of_tri), np.asarray(o.flipped)
    order = np.argsort(patch, kind="stable")
    order = order[patch[order] >= 0]
    starts = np.concatenate([[0], np.cumsum(o.counts[:, 1])])
    # the volume as written is the tree over the terms negated where the triangle ends up flipped: the tentative sum negates
    # where rel = 1, a whole-patch flip negates the sum, and negation commutes with every rounding
    x, _ = RS.terms(V, T, o.ref_point)
    signed = np.where(flipped[order], -x[order, 1], x[order, 1])
    _equal_bits(f"orient {shape}", np.asarray(o.volume)[:, None], segsum(signed, starts), ("volume",))


@pytest.mark.parametrize("shape", SHAPES)
def test_sections_sums_are_the_restated_tree(pkg, shape):
    if shape == "own":
        V, T, normal, levels = CX.case("cones")              # loops of 3 .. 1025 segments on two levels
    else:
        V, T = S.join(*[CX.cone(n, (3.0 * k, 0.0)) for k, n in enumerate(_sizes(shape))])
        normal, levels = np.array(CX.Z), np.array([0.25])
    o = pkg.mesh_sections(V, T, normal, levels)
    if shape != "own":
        assert o.n_segs.tolist() == list(_sizes(shape))
    x, _ = RX.terms(np.asarray(o.seg_points).reshape(-1, 2, 3), o.ref_point, normal)
    _equal_bits(f"sections {shape}", o.sums, segsum(x, o.contour_start), RX.NAMES)


@pytest.mark.parametrize("shape", SHAPES)
def test_holes_sums_are_the_restated_tree(pkg, shape):
    if shape == "own":
        V, T = CH.case("ico_many_holes")                     # 250 rims of 3, 5 or 6 edges
    else:
        V, T = S.join(*[CH.disk(n) for n in _sizes(shape)])
    o = pkg.mesh_holes(V, T)
    if shape != "own":
        assert o.n_edges.tolist() == list(_sizes(shape))
    h = np.asarray(o.rim_edge, np.int64)
    t, c = h // 3, h % 3
    v = np.asarray(V, np.float32).astype(np.float64)
    x, _ = RH.terms(v[T[t, c]], v[T[t, (c + 1) % 3]], o.ref_point)
    _equal_bits(f"holes {shape}", o.sums, segsum(x, o.rim_start), RH.NAMES)
