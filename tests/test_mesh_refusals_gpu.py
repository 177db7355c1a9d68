"""What the seven mesh topology tools (shells, orient, nesting, fans, holes, sections, weld) leave alone when they turn something
down AFTER the mesh itself has been accepted, for the host-pointer entry and the _dev entry alike: a table or an output mesh whose
capacity is one too small is not written, not even in part (the call still returns 0 and the sizes), a nesting index of another
mesh and a weld snap too fine for the extent are R2S_ERR_ARG with every output untouched, and r2s_last_* writes no row beyond its
capacity.  Every caller-owned array starts filled with a sentinel and is compared bit for bit afterwards.

The mesh is an octahedron with its top corner cut off and left open: 9 vertices, 12 triangles, one shell / patch, one rim of 4
boundary edges (so the fill adds one vertex and four triangles), no pinched vertex (so the split adds none).

Where a call writes other outputs before or beside the one it turns down, the comment at the call says so and nothing is asserted
on them: a short table does not keep shell_of_tri / tris_out / flip / patch_of_tri / fan_of_corner / fans_of_vert from being
written, and in holes the vertices and the triangles of the fill have a capacity each, so one can be written without the other.

Not reached here: the host entries of shells, orient, nesting and sections turn nothing down once the mesh is accepted, so for
them only r2s_last_* with a short capacity is checked; and the refusals of nesting behind its traversal (more than 2^31 - 1
crossings, a tree too deep), the ones that make it stage a device caller's tris_out in a work buffer, need far more than twelve
triangles, so that they leave d_tris_out untouched is not exercised by any test of this size."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG = -1
NV, NT = 9, 12
I64 = ctypes.c_int64


def sentinel(shape, dtype):
    a = np.empty(shape, dtype)
    a.fill(np.nan if a.dtype.kind == "f" else -7)
    return a


def mesh():
    E = [(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0)]
    V = E + [(0, 0, -1)] + [(0.5 * x, 0.5 * y, 0.5) for x, y, _ in E]
    T = []
    for i in range(4):
        j = (i + 1) % 4
        T += [(i, 4, j), (i, j, 5 + j), (i, 5 + j, 5 + i)]
    return np.array(V, np.float32), np.array(T, np.int32)


class Host:
    """caller-owned numpy arrays"""
    name = "host"

    def __init__(self, pkg):
        self.L = pkg._lib
        self.V, self.T = mesh()

    def new(self, shape, dtype):
        return sentinel(shape, dtype)

    def p(self, a):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))

    def get(self, a):
        return a

    def mesh_args(self):
        return self.p(self.V), NV, self.p(self.T), NT


class Dev(Host):
    """caller-owned device tensors, calls on a stream of the caller's"""
    name = "dev"

    def __init__(self, pkg):
        import torch
        super().__init__(pkg)
        self.torch = torch
        self.dV, self.dT = torch.from_numpy(self.V).cuda(), torch.from_numpy(self.T).cuda()
        self.stream = torch.cuda.Stream()
        self.st = ctypes.c_void_p(self.stream.cuda_stream)

    def new(self, shape, dtype):
        return self.torch.from_numpy(sentinel(shape, dtype)).cuda()

    def p(self, a):
        return None if a is None else ctypes.c_void_p(a.data_ptr())

    def get(self, a):
        return a.cpu().numpy()

    def mesh_args(self):
        return self.p(self.dV), NV, self.p(self.dT), NT


def untouched(c, a):
    got = np.ascontiguousarray(c.get(a))
    want = sentinel(got.shape, got.dtype)
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def hp(a):
    return a.ctypes.data_as(ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


@pytest.fixture(scope="module", params=[Host, Dev], ids=["host", "dev"])
def c(request, pkg):
    return request.param(pkg)


def test_shells(c):
    lib = c.L.lib()
    n, ref, tot = I64(), np.zeros(3), np.zeros(8, np.int64)
    sot = c.new(NT, np.int32)
    if c.name == "host":
        assert lib.r2s_mesh_shells(*c.mesh_args(), -1, c.p(sot), ctypes.byref(n), hp(ref), hp(tot)) == 0 and n.value == 1
        counts, sums = c.new((1, 8), np.int64), c.new((1, 11), np.float64)
        assert lib.r2s_last_mesh_shells(hp(counts), hp(sums), 0, ctypes.byref(n)) == 0 and n.value == 1
        assert untouched(c, counts) and untouched(c, sums)
        return
    counts, sums = c.new((1, 8), np.int64), c.new((1, 11), np.float64)
    # shell_capacity 0 of 1: no table row is written (shell_of_tri is)
    assert lib.r2s_mesh_shells_dev(*c.mesh_args(), c.p(sot), c.p(counts), c.p(sums), 0, ctypes.byref(n), hp(ref), hp(tot), c.st) == 0
    assert n.value == 1 and tot[1] == NT and untouched(c, counts) and untouched(c, sums)


def test_orient(c):
    lib = c.L.lib()
    n, ref, tot = I64(), np.zeros(3), np.zeros(8, np.int64)
    out, flip, pot = c.new((NT, 3), np.int32), c.new(NT, np.int32), c.new(NT, np.int32)
    counts, vol = c.new((1, 8), np.int64), c.new(1, np.float64)
    if c.name == "host":
        assert lib.r2s_mesh_orient(*c.mesh_args(), 1, -1, c.p(out), c.p(flip), c.p(pot), ctypes.byref(n), hp(ref), hp(tot)) == 0
        assert n.value == 1 and lib.r2s_last_mesh_orient(hp(counts), hp(vol), 0, ctypes.byref(n)) == 0 and n.value == 1
        assert untouched(c, counts) and untouched(c, vol)
        return
    # patch_capacity 0 of 1: no table row is written (tris_out, flip and patch_of_tri are)
    assert lib.r2s_mesh_orient_dev(*c.mesh_args(), 1, c.p(out), c.p(flip), c.p(pot), c.p(counts), c.p(vol), 0, ctypes.byref(n), hp(ref),
                                   hp(tot), c.st) == 0
    assert n.value == 1 and tot[1] == NT and untouched(c, counts) and untouched(c, vol)


def test_nesting(c, pkg):
    lib = c.L.lib()
    n, m, tot = I64(), I64(), np.zeros(8, np.int64)
    out, pot = c.new((NT, 3), np.int32), c.new(NT, np.int32)
    counts, pairs = c.new((1, 8), np.int64), c.new(4, np.int64)
    if c.name == "host":
        assert lib.r2s_mesh_nesting(*c.mesh_args(), 2, 1, -1, c.p(out), c.p(pot), ctypes.byref(n), hp(tot)) == 0 and n.value == 1
        assert lib.r2s_last_mesh_nesting(hp(counts), 0, hp(pairs), 0, ctypes.byref(n), ctypes.byref(m)) == 0
        assert (n.value, m.value) == (1, 0) and untouched(c, counts) and untouched(c, pairs)
        return
    # an index over another number of triangles: refused before anything is written, the scalars included
    ix = pkg.MeshIndex(c.V, c.T[:NT - 1])
    try:
        n.value = m.value = 77
        assert lib.r2s_mesh_nesting_dev(ix._handle(), *c.mesh_args(), 2, 1, c.p(out), c.p(pot), c.p(counts), 1, c.p(pairs), 4, ctypes.byref(n),
                                        ctypes.byref(m), hp(tot), c.st) == ARG
        assert b"the index holds 11 triangles, the mesh 12" in lib.r2s_last_error()
        assert (n.value, m.value) == (77, 77) and not tot.any()
        assert untouched(c, out) and untouched(c, pot) and untouched(c, counts) and untouched(c, pairs)
    finally:
        ix.close()
    # patch_capacity 0 of 1: no record is written (tris_out and patch_of_tri are); there is no pair
    assert lib.r2s_mesh_nesting_dev(None, *c.mesh_args(), 2, 1, c.p(out), c.p(pot), c.p(counts), 0, c.p(pairs), 4, ctypes.byref(n),
                                    ctypes.byref(m), hp(tot), c.st) == 0
    assert (n.value, m.value) == (1, 0) and tot[1] == NT and untouched(c, counts) and untouched(c, pairs)


def test_fans(c):
    lib = c.L.lib()
    n, nvo, tot = I64(), I64(), np.zeros(8, np.int64)
    foc, fov = c.new((NT, 3), np.int32), c.new(NV, np.int32)
    to, vo, vof = c.new((NT, 3), np.int32), c.new((NV, 3), np.float32), c.new(NV, np.int32)
    counts = c.new((NV, 8), np.int64)
    # vert_capacity one short of the 9 output vertices: nothing of the split is written (fan_of_corner and fans_of_vert are)
    if c.name == "host":
        assert lib.r2s_mesh_fans(*c.mesh_args(), -1, c.p(foc), c.p(fov), c.p(to), c.p(vo), c.p(vof), NV - 1, ctypes.byref(n),
                                 ctypes.byref(nvo), hp(tot)) == 0
        assert (n.value, nvo.value) == (NV, NV) and untouched(c, to) and untouched(c, vo) and untouched(c, vof)
        assert lib.r2s_last_mesh_fans(hp(counts), 3, ctypes.byref(n)) == 0 and n.value == NV
        assert counts[2, 0] == 2 and untouched(c, counts[3:])   # (three records, nothing behind them)
        return
    # and fan_capacity one short of the 9 fans: no record either
    assert lib.r2s_mesh_fans_dev(*c.mesh_args(), c.p(foc), c.p(fov), c.p(counts), NV - 1, c.p(to), c.p(vo), c.p(vof), NV - 1, ctypes.byref(n),
                                 ctypes.byref(nvo), hp(tot), c.st) == 0
    assert (n.value, nvo.value) == (NV, NV) and untouched(c, to) and untouched(c, vo) and untouched(c, vof) and untouched(c, counts)


def test_holes(c):
    lib = c.L.lib()
    nr, nb, nvo, nto = I64(), I64(), I64(), I64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    sizes = [ctypes.byref(x) for x in (nr, nb, nvo, nto)] + [hp(ref), hp(tot)]
    start, counts, sums, edge = c.new(2, np.int64), c.new((1, 8), np.int64), c.new((1, 7), np.float64), c.new(4, np.int32)
    for vcap, tcap in ((NV, NT + 4), (NV + 1, NT + 3)):   # the fill needs 10 vertices and 16 triangles: one of the two is one short
        to, vo = c.new((NT + 4, 3), np.int32), c.new((NV + 1, 3), np.float32)
        if c.name == "host":
            assert lib.r2s_mesh_holes(*c.mesh_args(), -1, -1, c.p(to), c.p(vo), vcap, tcap, *sizes) == 0
        else:
            # rim_capacity 0 of 1 and edge_capacity 3 of 4 as well: no table is written
            assert lib.r2s_mesh_holes_dev(*c.mesh_args(), -1, c.p(start), c.p(counts), c.p(sums), 0, c.p(edge), 3, c.p(to), c.p(vo), vcap,
                                          tcap, *sizes, c.st) == 0
            assert untouched(c, start) and untouched(c, counts) and untouched(c, sums) and untouched(c, edge)
        assert (nr.value, nb.value, nvo.value, nto.value) == (1, 4, NV + 1, NT + 4)
        # (the array with room is written: the two capacities are judged apart)
        assert untouched(c, vo if vcap == NV else to) and not untouched(c, to if vcap == NV else vo)
    if c.name == "host":
        assert lib.r2s_last_mesh_holes(hp(start), hp(counts), hp(sums), 0, hp(edge), 3, ctypes.byref(nr), ctypes.byref(nb)) == 0
        assert (nr.value, nb.value) == (1, 4) and untouched(c, start) and untouched(c, counts) and untouched(c, sums)
        assert not untouched(c, edge[:3]) and untouched(c, edge[3:])


def test_sections(c):
    lib = c.L.lib()
    nc, ns, ref, tot = I64(), I64(), np.zeros(3), np.zeros(8, np.int64)
    nrm, lev = np.array([0.0, 0.0, 1.0]), np.array([-0.5])   # the plane cuts the four lower triangles: one loop of 4 segments
    start, counts, sums = c.new(2, np.int64), c.new((1, 8), np.int64), c.new((1, 7), np.float64)
    seg, pts = c.new(4, np.int32), c.new((4, 6), np.float64)
    if c.name == "host":
        assert lib.r2s_mesh_sections(*c.mesh_args(), hp(nrm), hp(lev), 1, -1, ctypes.byref(nc), ctypes.byref(ns), hp(ref), hp(tot)) == 0
        assert lib.r2s_last_mesh_sections(hp(start), hp(counts), hp(sums), 0, hp(seg), hp(pts), 3, ctypes.byref(nc), ctypes.byref(ns)) == 0
        assert (nc.value, ns.value) == (1, 4) and untouched(c, start) and untouched(c, counts) and untouched(c, sums)
        assert not untouched(c, seg[:3]) and untouched(c, seg[3:]) and untouched(c, pts[3:])
        return
    for ccap, scap in ((0, 4), (1, 3)):   # either capacity one short: none of the five tables is written
        assert lib.r2s_mesh_sections_dev(*c.mesh_args(), hp(nrm), hp(lev), 1, c.p(start), c.p(counts), c.p(sums), ccap, c.p(seg), c.p(pts),
                                         scap, ctypes.byref(nc), ctypes.byref(ns), hp(ref), hp(tot), c.st) == 0
        assert (nc.value, ns.value) == (1, 4)
        assert all(untouched(c, a) for a in (start, counts, sums, seg, pts))


def test_weld(c):
    lib = c.L.lib()
    tot = np.full(8, -7, np.int64)
    vo, to, vm, tm = c.new((NV, 3), np.float32), c.new((NT, 3), np.int32), c.new(NV, np.int32), c.new(NT, np.int32)
    # snap = 2^-40 puts the cell index of the coordinate 1 at 2^40: refused before anything is written, the totals included
    tail = (c.st,) if c.name == "dev" else ()
    head = c.mesh_args() + ((2.0 ** -40, 7) if c.name == "dev" else (2.0 ** -40, 7, -1))
    rc = (lib.r2s_mesh_weld_dev if c.name == "dev" else lib.r2s_mesh_weld)(*head, c.p(vo), c.p(to), c.p(vm), c.p(tm), hp(tot), *tail)
    assert rc == ARG and b"too fine for the extent" in lib.r2s_last_error()
    assert (tot == -7).all() and all(untouched(c, a) for a in (vo, to, vm, tm))
