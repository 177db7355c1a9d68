"""The segmented Float64 sum of the mesh tools (include/rho2sdf_hip.h; ms_block_sum and ms_combine_kernel in
rho2sdf.jl_amd/csrc/r2s_mesh_graph.hpp), restated once in numpy float64 with no fused operation, for the bit-for-bit tests of
tests/test_mesh_segsum_gpu.py.  Every addition below is one IEEE double addition, in the order the header defines:

  block tree   block b holds the output positions [256 b, 256 b + 256).  Rounds d = 1, 2, 4, .., 128: position j takes the value
               position j + d held BEFORE the round when j + d < 256 and both lie in the same segment.  Afterwards the first
               position of every segment in the block holds the partial of (block b, segment s).
  slot rule    that partial is stored at slot b + s.
  combine      segment s covers the blocks b0 .. b0 + nb - 1.  chunk = ceil(nb / 64), m = ceil(nb / chunk) lanes have a run; lane
               l adds its partials lo = l chunk .. min(lo + chunk, nb) - 1 one at a time in ascending order, starting from the
               first.  Rounds d = 1, 2, .., 32: lane l takes the value lane l + d held before the round while l + d < m.
               Lane 0 holds the sum."""
import numpy as np

BLOCK = 256


def block_partials(terms, starts):
    """-> slots (nblocks + n_segments, k): the partial of (block b, segment s) at slot b + s, NaN where nothing is stored.
    terms (m, k): the per-item term rows in output order; starts (n + 1,): the first position of every segment and m"""
    x = np.ascontiguousarray(terms, np.float64)
    m, k = x.shape
    starts = np.asarray(starts, np.int64)
    n = len(starts) - 1
    assert starts[0] == 0 and starts[-1] == m and (np.diff(starts) > 0).all()
    nblocks = (m + BLOCK - 1) // BLOCK
    key = np.full(nblocks * BLOCK, -1, np.int64)
    key[:m] = np.repeat(np.arange(n), np.diff(starts))
    key = key.reshape(nblocks, BLOCK)
    v = np.zeros((nblocks * BLOCK, k))
    v[:m] = x
    v = v.reshape(nblocks, BLOCK, k)
    active = key >= 0
    d = 1
    while d < BLOCK:
        take = np.zeros_like(active)
        take[:, :BLOCK - d] = active[:, :BLOCK - d] & (key[:, d:] == key[:, :BLOCK - d])
        other = np.zeros_like(v)
        other[:, :BLOCK - d] = v[:, d:]                     # (the values before the round)
        v = np.where(take[:, :, None], v + other, v)
        d *= 2
    head = active.copy()
    head[:, 1:] &= key[:, 1:] != key[:, :-1]
    slots = np.full((nblocks + n, k), np.nan)
    b, j = np.nonzero(head)
    slot = b + key[b, j]
    assert len(np.unique(slot)) == len(slot)
    slots[slot] = v[b, j]
    return slots


def combine(slots, starts):
    """-> sums (n, k) from the slots of block_partials"""
    starts = np.asarray(starts, np.int64)
    n, k = len(starts) - 1, slots.shape[1]
    sums = np.empty((n, k))
    for s in range(n):
        b0 = int(starts[s]) // BLOCK
        nb = (int(starts[s + 1]) - 1) // BLOCK - b0 + 1
        chunk = (nb + 63) // 64
        m = (nb + chunk - 1) // chunk
        lane = np.zeros((64, k))
        for l in range(m):
            lo, hi = l * chunk, min(l * chunk + chunk, nb)
            acc = slots[b0 + lo + s].copy()
            for b in range(lo + 1, hi):
                acc = acc + slots[b0 + b + s]
            lane[l] = acc
        d = 1
        while d < 64:
            takes = np.arange(64) + d < m
            nxt = lane.copy()
            nxt[:64 - d][takes[:64 - d]] = (lane[:64 - d] + lane[d:])[takes[:64 - d]]   # (the values before the round)
            lane = nxt
            d *= 2
        sums[s] = lane[0]
    assert not np.isnan(sums).any()                         # (a NaN would be a slot nothing was stored to)
    return sums


def segsum(terms, starts):
    """the sums (n, k) of the segments [starts[s], starts[s + 1]) of the term rows, in the header's operation order"""
    terms = np.asarray(terms, np.float64)
    if terms.ndim == 1:
        terms = terms[:, None]
    if len(starts) <= 1:
        return np.zeros((0, terms.shape[1]))
    return combine(block_partials(terms, starts), starts)
