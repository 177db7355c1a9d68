"""The cases of tests/test_iso_schedule_gpu.py have the chunk-per-item shapes they exist for - from box arithmetic alone
(iso_schedule_cases.item_chunks restates the lattice box of item_build_kernel), no GPU needed."""
import numpy as np

import iso_schedule_cases as C


def _chunks(oracle, name):
    X, IEN, rn, nmax = C.build_case(name)
    og = oracle.grid_make(X.min(0), X.max(0), nmax, 3)
    chunks, vol = C.item_chunks(X, IEN, og)
    iso = (rn[IEN - 1].min(1) < C.RHO_T) & (rn[IEN - 1].max(1) > C.RHO_T)   # elements the iso-surface certainly crosses
    assert iso.any()
    return chunks[iso], vol[iso], og


def test_one_item_spans_hundreds_of_chunks(oracle):
    chunks, _, _ = _chunks(oracle, "one_item")
    assert len(chunks) == 1 and chunks[0] >= 100      # every group of up to 8 chunks lies inside the one item


def test_distorted_items_are_about_a_group_long(oracle):
    """6.9 cells per element and the band: boxes of 9-13 lattice points per axis, 11 to 30 chunks - every item takes
    several groups of up to 8 chunks and most groups straddle an item boundary"""
    chunks, _, _ = _chunks(oracle, "distorted")
    assert chunks.min() > 8 and chunks.max() <= 32
    assert (chunks % 8 != 0).mean() > 0.75


def test_tiny_items_are_one_or_two_chunks_each(oracle):
    """an element of about one cell and a 1.1-cell band on each side: 3 to 6 lattice points per axis, 27 to 150 in the
    box - one chunk for more than half of the items, never more than three, fewer than two on average: a group of 8
    chunks spans more items than the kernel has LDS slots (R2S_ISO_SLOTS = 4)"""
    chunks, vol, _ = _chunks(oracle, "tiny_items")
    assert vol.min() >= 27 and chunks.max() <= 3
    assert 2 * (chunks == 1).sum() > len(chunks) > 64 and chunks.sum() < 2 * len(chunks)


def test_slab_planes_of_the_two_runs():
    assert C.slab_planes("planes", 48).tolist() == list(range(4, 13))
    k = C.slab_planes("layers", 48)
    assert k.tolist() == [4 * t + j for t in range(1, 12, 2) for j in range(4)]
    k = C.slab_planes("layers", 46)      # the last tile layer ends behind the grid: padding planes
    assert k[-4:].tolist() == [44, 45, -1, -1]
