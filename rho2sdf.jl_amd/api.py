"""Host-side mirror of the reference's Julia interface for the hot path.

Names, argument meaning and error behaviour follow the reference functions
that `rho2sdf()` calls (src/RhoToSDF.jl:148-224); every function is a thin
marshalling layer over the C ABI in include/rho2sdf_hip.h - exactly what the
Julia `ccall` wrapper (julia/Rho2sdfHIP.jl) does.  No numerics happen here.

Array conventions (numpy): X is (nnp, 3) float64 = Julia's 3 x nnp column-major
matrix; IEN is (nel, nen) 1-based = Julia's nen x nel matrix; grid vectors are
flat in the reference's x-fastest order (Grid.jl:84-92).
"""
import ctypes

import numpy as np

from . import _lib as L


class Grid:
    """Grid(AABB_min, AABB_max, N_max, margineCells=3)  - src/MeshGrid/Grid.jl:2-35"""

    def __init__(self, AABB_min, AABB_max, N_max, margineCells=3, _raw=None):
        if _raw is not None:
            self.c = _raw
            return
        self.c = L.R2SGrid()
        a = (ctypes.c_double * 3)(*[float(v) for v in AABB_min])
        b = (ctypes.c_double * 3)(*[float(v) for v in AABB_max])
        L.check(L.lib().r2s_grid_make(a, b, int(N_max), int(margineCells), ctypes.byref(self.c)))

    AABB_min = property(lambda s: np.array(s.c.aabb_min[:]))
    AABB_max = property(lambda s: np.array(s.c.aabb_max[:]))
    N = property(lambda s: np.array(s.c.N[:], dtype=np.int64))
    cell_size = property(lambda s: float(s.c.cell_size))
    ngp = property(lambda s: int(s.c.ngp))
    dims = property(lambda s: tuple(int(n) + 1 for n in s.c.N))


class Mesh:
    """Flat view of `Mesh{T}` (src/MeshGrid/MeshInformations.jl:16-67): X, IEN (1-based)."""

    def __init__(self, X, IEN, element_type=None):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.IEN = np.ascontiguousarray(IEN, dtype=np.int64)
        if self.X.ndim != 2 or self.X.shape[1] != 3:
            raise L.R2SError("X must be (nnp, 3)")
        nen = self.IEN.shape[1]
        if nen not in (8, 4):
            # MeshInformations.jl:58-60
            raise L.R2SError(f"Element connectivity size ({nen}) doesn't match element type nodes")
        self.element_type = {8: L.HEX8, 4: L.TET4}[nen] if element_type is None else element_type
        self.nnp, self.nel, self.nen = len(self.X), len(self.IEN), nen


def getMesh_AABB(X):
    """src/MeshGrid/Grid.jl:73-77"""
    X = np.asarray(X)
    return X.min(axis=0), X.max(axis=0)


def noninteractive_sdf_grid_setup(mesh):
    """src/MeshGrid/Grid_setup.jl:94-108 -> Grid"""
    g = L.R2SGrid()
    med = ctypes.c_double()
    L.check(L.lib().r2s_auto_grid(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, mesh.element_type,
                                  ctypes.byref(g), ctypes.byref(med)))
    return Grid(None, None, None, _raw=g)


def _d(a):
    return a.ctypes.data_as(L.c_double_p)


def _i(a):
    return a.ctypes.data_as(L.c_int64_p)


def _params(mesh, band_factor, device, n_gpus=1, true_min=False, sign_no_inner=False):
    p = L.R2SParams()
    L.lib().r2s_default_params(ctypes.byref(p))
    p.band_factor = float(band_factor)
    p.elem_type = mesh.element_type
    p.device = int(device)
    p.n_gpus = int(n_gpus)
    p.true_min = int(bool(true_min))
    p.sign_no_inner = int(bool(sign_no_inner))
    return p


def host_array(n, dtype=np.float64):
    """numpy array over pinned host memory from r2s_host_alloc (what the Julia wrapper `unsafe_wrap`s its result
    arrays from): device -> host copies into it are plain DMA.  Freed with r2s_host_free when the array dies."""
    import weakref
    dtype = np.dtype(dtype)
    nbytes = int(n) * dtype.itemsize
    ptr = L.lib().r2s_host_alloc(max(nbytes, 1))
    if not ptr:
        raise L.R2SError("r2s_host_alloc failed: " + L.lib().r2s_last_error().decode())
    buf = (ctypes.c_char * max(nbytes, 1)).from_address(ptr)
    a = np.frombuffer(buf, dtype=dtype, count=int(n))
    weakref.finalize(buf, L.lib().r2s_host_free, ctypes.c_void_p(ptr))
    return a


def _out(out, n, dtype=np.float64):
    if out is None:
        return np.empty(n, dtype=dtype)
    if out.dtype != dtype or not out.flags.c_contiguous or out.size != n:
        raise L.R2SError("`out` must be a contiguous %s array of %d values" % (np.dtype(dtype).name, n))
    return out


def _rho(mesh, rho_n):
    r = np.ascontiguousarray(rho_n, dtype=np.float64)
    if r.shape != (mesh.nnp,):
        raise L.R2SError("length of nodal densities does not match number of nodes")
    return r


def evalDistances(mesh, grid, rho_n, rho_t, *, band_factor=1.1, want_xp=True, device=-1, stats=None, n_gpus=1, out=None, true_min=False):
    """evalDistances(mesh, grid, points, rho_n, rho_t) -> (dist, xp)
    src/SignedDistances/sdfOnDensityField.jl:139-486 (`points` is implied by `grid`)."""
    r = _rho(mesh, rho_n)
    dist = _out(out, grid.ngp)
    xp = np.empty((grid.ngp, 3)) if want_xp else None
    st = L.R2SStats()
    p = _params(mesh, band_factor, device, n_gpus, true_min)
    L.check(L.lib().r2s_eval_distances(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, _d(r), float(rho_t),
                                       ctypes.byref(grid.c), ctypes.byref(p), _d(dist),
                                       _d(xp) if want_xp else None, ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return dist, xp


def Sign_Detection(mesh, grid, rho_n, rho_t, *, device=-1, stats=None, n_gpus=1, out=None, true_min=False, sign_no_inner=False):
    """Sign_Detection(mesh, grid, points, rho_n, rho_t) -> signs  (SignDetection.jl:275-283)"""
    r = _rho(mesh, rho_n)
    s = _out(out, grid.ngp)
    st = L.R2SStats()
    p = _params(mesh, 1.1, device, n_gpus, true_min, sign_no_inner)
    L.check(L.lib().r2s_sign_detection(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, _d(r), float(rho_t),
                                       ctypes.byref(grid.c), ctypes.byref(p), _d(s), ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return s


def sdf_fused(mesh, grid, rho_n, rho_t, *, band_factor=1.1, device=-1, stats=None, n_gpus=1, out=None, true_min=False, sign_no_inner=False):
    """`dists .* signs` in one pass (RhoToSDF.jl:169-171).  `out`: result array to fill (e.g. from host_array)."""
    r = _rho(mesh, rho_n)
    out = _out(out, grid.ngp)
    st = L.R2SStats()
    p = _params(mesh, band_factor, device, n_gpus, true_min, sign_no_inner)
    L.check(L.lib().r2s_sdf(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, _d(r), float(rho_t),
                            ctypes.byref(grid.c), ctypes.byref(p), _d(out), ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return out


def _stream(stream):
    """the raw handle of a torch stream (None: the current stream), as the *_dev entry points take it"""
    import torch
    return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def _mesh_tensors(verts, tris):
    import torch
    if verts.dtype != torch.float32 or tris.dtype != torch.int32 or not (verts.is_cuda and tris.is_cuda) \
            or not (verts.is_contiguous() and tris.is_contiguous()):
        raise L.R2SError("verts / tris must be contiguous float32 / int32 device tensors")


def _float_dtype(dtype, xp):
    """`dtype` as the float32 or float64 of `xp` (numpy or torch); None: float64"""
    dtype = xp.float64 if dtype is None else dtype
    dtype = np.dtype(dtype) if xp is np else dtype
    if dtype not in (xp.float32, xp.float64):
        raise L.R2SError("dtype must be float32 or float64")
    return dtype


def _points_nx3(message, *arrays, same_shape=False):
    """R2SError(message) unless every array is (n, 3); a torch tensor must also be float32 / float64, contiguous and on a device"""
    for a in arrays:
        ok = a.ndim == 2 and a.shape[1] == 3 and not (same_shape and a.shape != arrays[0].shape)
        if ok and not isinstance(a, np.ndarray):
            import torch
            ok = a.dtype in (torch.float32, torch.float64) and a.is_contiguous() and a.is_cuda
        if not ok:
            raise L.R2SError(message)


def _dist_outputs(shape, dtype, want_index, device=None):
    """-> (result, dist pointer, index pointer or None) of a distance call: `result` is dist of `dtype`, or (dist, int32 idx)
    with want_index; numpy arrays, or torch tensors on `device`"""
    if device is None:
        dist, idx = np.empty(shape, dtype), np.empty(shape, np.int32) if want_index else None
        ptrs = dist.ctypes.data_as(ctypes.c_void_p), idx.ctypes.data_as(L.c_int32_p) if want_index else None
    else:
        import torch
        dist = torch.empty(shape, dtype=dtype, device=device)
        idx = torch.empty(shape, dtype=torch.int32, device=device) if want_index else None
        ptrs = ctypes.c_void_p(dist.data_ptr()), ctypes.c_void_p(idx.data_ptr()) if want_index else None
    return ((dist, idx) if want_index else dist,) + ptrs


class DevicePlan:
    """Device-resident path (inputs/outputs are torch CUDA tensors = HBM buffers).

    torch is used only as the owner of device memory and streams; the pointers
    go straight into r2s_plan_run_dev().
    """

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        L.check(L.lib().r2s_plan_create(int(device), ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            L.lib().r2s_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, dX, dIEN, d_rho_n, rho_t, grid, *, k_begin=0, k_end=None, band_factor=1.1,
            elem_type=None, dist=None, sign=None, sdf=None, xp=None, stream=None, zstride=1, zphase=0, true_min=False):
        """one pass over planes [k_begin, k_end) (zstride <= 1) or over the interleaved tile layers
        t % zstride == zphase of the whole grid (see r2s_params in include/rho2sdf_hip.h)"""
        import torch
        if elem_type is None:
            elem_type = L.HEX8 if dIEN.shape[1] == 8 else L.TET4
        k_end = int(grid.c.N[2]) + 1 if k_end is None else int(k_end)
        for t, dt in ((dX, torch.float64), (dIEN, torch.int64), (d_rho_n, torch.float64)):
            assert t.is_cuda and t.is_contiguous() and t.dtype == dt
        mode = 0
        ptr = []
        for t, bit in ((dist, L.OUT_DIST), (sign, L.OUT_SIGN), (sdf, L.OUT_SDF), (xp, L.OUT_XP)):
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
                mode |= bit
                ptr.append(ctypes.c_void_p(t.data_ptr()))
            else:
                ptr.append(None)
        p = L.R2SParams()
        L.lib().r2s_default_params(ctypes.byref(p))
        p.band_factor = float(band_factor)
        p.elem_type = int(elem_type)
        p.zstride = int(zstride)
        p.zphase = int(zphase)
        p.true_min = int(bool(true_min))
        st = L.R2SStats()
        s = _stream(stream)
        L.check(L.lib().r2s_plan_run_dev(self._h, ctypes.c_void_p(dX.data_ptr()), dX.shape[0],
                                         ctypes.c_void_p(dIEN.data_ptr()), dIEN.shape[0],
                                         ctypes.c_void_p(d_rho_n.data_ptr()), float(rho_t),
                                         ctypes.byref(grid.c), ctypes.byref(p), int(k_begin), k_end, mode,
                                         ptr[0], ptr[1], ptr[2], ptr[3], s, ctypes.byref(st)))
        return st.as_dict()

    # ---- sparse stitching (see include/rho2sdf_hip.h) ----
    _stream = staticmethod(_stream)

    def pack_tiles(self, local_sdf, payload, ids, stream=None):
        """pack the non-sentinel tiles of the last run's output into payload (n,64) f64 / ids (n,) i32"""
        n = ctypes.c_int64()
        L.check(L.lib().r2s_plan_pack_tiles_dev(self._h, ctypes.c_void_p(local_sdf.data_ptr()),
                                                ctypes.c_void_p(payload.data_ptr()), ctypes.c_void_p(ids.data_ptr()),
                                                int(ids.numel()), ctypes.byref(n), self._stream(stream)))
        return int(n.value)

    @staticmethod
    def unpack_tiles(payload, ids, n, grid, volume, stream=None):
        L.check(L.lib().r2s_unpack_tiles_dev(ctypes.c_void_p(payload.data_ptr()), ctypes.c_void_p(ids.data_ptr()), int(n),
                                             ctypes.byref(grid.c), ctypes.c_void_p(volume.data_ptr()),
                                             DevicePlan._stream(stream)))

    def pack_tiles2(self, local_sdf, payload, ids, masks, mask_ids, stream=None):
        """compressed packing: band tiles -> payload (n,64) f64 / ids i32; sign-only tiles -> masks i64 / mask_ids i32.
        Returns (n_full, n_mask)."""
        nf, nm = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().r2s_plan_pack_tiles2_dev(
            self._h, ctypes.c_void_p(local_sdf.data_ptr()), ctypes.c_void_p(payload.data_ptr()),
            ctypes.c_void_p(ids.data_ptr()), int(ids.numel()), ctypes.c_void_p(masks.data_ptr()),
            ctypes.c_void_p(mask_ids.data_ptr()), int(mask_ids.numel()), ctypes.byref(nf), ctypes.byref(nm),
            self._stream(stream)))
        return int(nf.value), int(nm.value)

    @staticmethod
    def unpack_masks(masks, mask_ids, n, grid, volume, magnitude=1.0e10, stream=None):
        L.check(L.lib().r2s_unpack_masks_dev(ctypes.c_void_p(masks.data_ptr()), ctypes.c_void_p(mask_ids.data_ptr()), int(n),
                                             ctypes.byref(grid.c), float(magnitude), ctypes.c_void_p(volume.data_ptr()),
                                             DevicePlan._stream(stream)))

    @staticmethod
    def unpack_segments(buf, world, seglen, cap_full, cap_mask, grid, volume, magnitude=1.0e10, stream=None):
        """scatter every rank's segment of the exchange buffer in two launches; the tile counts are read from the segment
        headers on the device (see r2s_unpack_segments_dev)"""
        L.check(L.lib().r2s_unpack_segments_dev(ctypes.c_void_p(buf.data_ptr()), int(world), int(seglen), int(cap_full), int(cap_mask),
                                                ctypes.byref(grid.c), float(magnitude), ctypes.c_void_p(volume.data_ptr()),
                                                DevicePlan._stream(stream)))

    @staticmethod
    def fill(t, value, stream=None):
        L.check(L.lib().r2s_fill_dev(ctypes.c_void_p(t.data_ptr()), int(t.numel()), float(value), DevicePlan._stream(stream)))


# ---------------------------------------------------------------------------------------
# pre-stage and post-processing (same thin marshalling; reference citations at each function)
# ---------------------------------------------------------------------------------------
def _f(a):
    return a.ctypes.data_as(L.c_float_p)


def calculate_mesh_volume(mesh, rho, *, device=-1):
    """calculate_mesh_volume(X, IEN, rho, T) -> [V_domain, V_frac]   src/MeshGrid/MeshVolume.jl:4-42"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    vd, vf = ctypes.c_double(), ctypes.c_double()
    L.check(L.lib().r2s_mesh_volume(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, mesh.element_type, _d(rho),
                                    int(device), ctypes.byref(vd), ctypes.byref(vf)))
    return vd.value, vf.value


def DenseInNodes(mesh, rho, *, device=-1):
    """DenseInNodes(mesh, rho) -> rho_n   src/MeshGrid/NodalDensities.jl:89-108"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    if rho.shape != (mesh.nel,):
        raise L.R2SError("length of element densities does not match number of elements")
    out = np.empty(mesh.nnp)
    L.check(L.lib().r2s_dense_in_nodes(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, mesh.element_type, _d(rho),
                                       int(device), _d(out)))
    return out


def find_threshold_for_volume(mesh, rho_n, target_volume, tolerance=1e-4, max_iterations=60, *, device=-1, info=None):
    """find_threshold_for_volume(mesh, nodal_values, tol, maxit); target_volume = V_domain*V_frac
    src/MeshGrid/Isocontour_volume.jl:77-154.  `info` (a dict) receives "iterations", the reference's current_iteration"""
    r = _rho(mesh, rho_n)
    rt = ctypes.c_double()
    it = ctypes.c_int32()
    L.check(L.lib().r2s_find_threshold_et(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, mesh.element_type, _d(r),
                                          float(target_volume), float(tolerance), int(max_iterations), int(device),
                                          ctypes.byref(rt), ctypes.byref(it)))
    if info is not None:
        info["iterations"] = int(it.value)
    return rt.value


def calculate_isocontour_volume(mesh, rho_n, iso_threshold, *, device=-1):
    """calculate_isocontour_volume(mesh, nodal_values, iso_threshold)   src/MeshGrid/Isocontour_volume.jl:1-75
    (TET4: the iso-volume assembled from the reference's TET4 quadrature, see include/rho2sdf_hip.h)"""
    r = _rho(mesh, rho_n)
    v = ctypes.c_double()
    L.check(L.lib().r2s_isocontour_volume(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, mesh.element_type, _d(r),
                                          float(iso_threshold), int(device), ctypes.byref(v)))
    return v.value


def remove_sdf_artifacts(sdf, grid, *, threshold=0.0, min_component_ratio=0.01, device=-1):
    """remove_sdf_artifacts!(sdf, grid; threshold, min_component_ratio) -> nodes flipped (sdf modified in place)
    src/SignedDistances/SdfArtifactRemoval.jl:134-245"""
    if sdf.dtype != np.float64 or not sdf.flags.c_contiguous:
        raise L.R2SError("sdf must be a contiguous float64 array (it is modified in place)")
    if sdf.size != grid.ngp:   # SdfArtifactRemoval.jl:141-143
        raise L.R2SError(f"SDF values length ({sdf.size}) doesn't match grid points ({grid.ngp})")
    n = ctypes.c_int64()
    L.check(L.lib().r2s_remove_artifacts(_d(sdf), ctypes.byref(grid.c), float(threshold), float(min_component_ratio),
                                         int(device), ctypes.byref(n)))
    return int(n.value)


def _components_dict(analyze):
    """the table of one analysis call through the thread's last table: count (capacity 0), then copy -> {root + 1: size}"""
    n = ctypes.c_int64()
    L.check(analyze(None, None, 0, ctypes.byref(n)))
    roots, sizes = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
    if n.value:
        L.check(L.lib().r2s_last_components(_i(roots), _i(sizes), n.value, ctypes.byref(n)))
    return dict(zip((roots + 1).tolist(), sizes.tolist()))


def analyze_sdf_components(sdf, grid, *, threshold=0.0, device=-1):
    """analyze_sdf_components(sdf, grid; threshold) -> Dict{Int,Int}  src/SignedDistances/SdfArtifactRemoval.jl:256-311
    One entry per 6-connected component of {sdf >= threshold} (NaN is never interior), in ascending key order:
    key = the 1-based (Julia) linear index of the component's first voxel, value = its voxel count.  The reference keys
    each component by its union-find root (union by rank, :41-60), which depends on the union order; here the key is
    canonical.  The partition and the sizes are the same.  An all-exterior field gives {}.  sdf is not modified and
    nothing is printed."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float64)
    if sdf.size != grid.ngp:
        raise L.R2SError(f"SDF values length ({sdf.size}) doesn't match grid points ({grid.ngp})")
    return _components_dict(lambda r, s, cap, n: L.lib().r2s_analyze_components(
        _d(sdf), ctypes.byref(grid.c), float(threshold), int(device), r, s, cap, n))


def calculate_volume_from_sdf(fine_sdf, edge, *, iso_threshold=0.0, detailed_quad_order=9, device=-1):
    """calculate_volume_from_sdf(fine_sdf, fine_grid; iso_threshold, detailed_quad_order) -> Float32
    src/SdfSmoothing/CalcVolumeFromSDF.jl:26-125; fine_sdf is (nz, ny, nx) float32, `edge` the grid spacing."""
    a = np.ascontiguousarray(fine_sdf, dtype=np.float32)
    nz, ny, nx = a.shape
    v = ctypes.c_float()
    L.check(L.lib().r2s_volume_from_sdf(_f(a), nx, ny, nz, float(edge), float(iso_threshold), int(detailed_quad_order),
                                        int(device), ctypes.byref(v)))
    return float(v.value)


def RBFs_smoothing(sdf, grid, Is_interpolation, smooth, target_volume, threshold=1e-3, *, device=-1, info=None):
    """RBFs_smoothing(mesh, dist, grid, Is_interpolation, smooth, taskName, threshold) -> fine_sdf
    src/SdfSmoothing/RBFs4Smoothing.jl:321-377 (mesh only contributes V_frac*V_domain = target_volume).
    Returns fine_sdf as (nz', ny', nx') float32; the fine grid is AABB_min + spacing*(i,j,k)."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float64)
    dims = tuple(int(n) * int(smooth) + 1 for n in grid.c.N)
    fine = np.empty(dims[2] * dims[1] * dims[0], dtype=np.float32)
    lsf = np.empty(grid.ngp, dtype=np.float32)
    th = ctypes.c_float()
    its = ctypes.c_int32()
    L.check(L.lib().r2s_rbf_smooth(_d(sdf), ctypes.byref(grid.c), int(bool(Is_interpolation)), int(smooth),
                                   float(threshold), float(target_volume), int(device), _f(fine), ctypes.byref(th),
                                   ctypes.byref(its), _f(lsf)))
    if info is not None:
        info.update(th=float(th.value), cg_iterations=int(its.value), lsf=lsf.reshape(grid.dims[2], grid.dims[1], grid.dims[0]))
    return fine.reshape(dims[2], dims[1], dims[0])


def last_rbf_plan():
    """forms, row-walk plans and tables of the calling thread's last smoothing (r2s_last_rbf_plan), decoded"""
    s = (ctypes.c_int32 * 12)()
    L.lib().r2s_last_rbf_plan(s)
    v = [int(x) for x in s]
    axes = lambda w: tuple((w >> (8 * a)) & 255 for a in range(3))
    return dict(product=(None, "walk", "lut", "k", "fly")[v[0] + 1], evaluation=("walk", "lut", "fly")[v[1]],
                walk_ok=bool(v[2] & 1), capped=bool(v[2] & 2),
                product_plan=dict(NW=v[3], L=v[4], nxt=v[5]), evaluation_plan=dict(NW=v[6], L=v[7], nxt=v[8]),
                wa_nv=v[9] & 255, wa_nv_fine=(v[9] >> 8) & 255, variants=axes(v[10]), variants_fine=axes(v[11]))


def exportSdfToVTI(filename, grid, values, value_label, smooth=None, compress=0):
    """exportSdfToVTI(filename, grid, values, value_label, smooth) - VTK ImageData (.vti)
    src/DataExport/ExportToVTI.jl:22-67: dimensions N(*smooth)+1, origin AABB_min, spacing cell_size(/smooth).
    `values` is float32 or float64, x fastest (any shape).  Returns the path written."""
    a = np.ascontiguousarray(values)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    L.check(L.lib().r2s_export_vti_z(str(filename).encode(), ctypes.byref(grid.c), a.ctypes.data_as(ctypes.c_void_p),
                                     int(a.dtype == np.float32), int(a.size), str(value_label).encode(),
                                     0 if smooth is None else int(smooth), int(compress)))
    filename = str(filename)
    return filename if filename.endswith(".vti") else filename + ".vti"


def _iso_lattice(grid, smooth):
    """(dims, origin, spacing) of the lattice exportSdfToVTI writes for `grid` and `smooth` (None: N+1 points, cell_size)"""
    s = 1 if smooth is None else int(smooth)
    dims = (ctypes.c_int64 * 3)(*[int(n) * s + 1 for n in grid.c.N])
    origin = (ctypes.c_double * 3)(*grid.c.aabb_min)
    spacing = float(grid.cell_size) if smooth is None else float(grid.cell_size) / float(s)
    return dims, origin, spacing


def _last_isosurface():
    """the calling thread's last surface (r2s_last_isosurface): count, then copy"""
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_last_isosurface(None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    verts, tris = np.empty((nv.value, 3), np.float32), np.empty((nt.value, 3), np.int32)
    L.check(L.lib().r2s_last_isosurface(_f(verts), nv.value, tris.ctypes.data_as(L.c_int32_p), nt.value, ctypes.byref(nv),
                                        ctypes.byref(nt)))
    return verts, tris


def extract_isosurface(values, grid, smooth=None, *, iso=0.0, device=-1):
    """The watertight triangle mesh of {values >= iso} (include/rho2sdf_hip.h, r2s_extract_isosurface) -> (verts (nv, 3)
    float32, tris (nt, 3) int32, 0-based).  `values` is the (nz, ny, nx) float32 fine field (smooth = the rbf_grid factor)
    or the float64 `sdf_dists` (smooth=None); the lattice is the one exportSdfToVTI writes for the same grid and smooth, so
    the mesh overlays the .vti.  Vertices lie on the lattice edges that cross the level, in ascending edge order; normals
    (v1-v0)x(v2-v0) point from the interior to the exterior.  No counterpart in the reference, whose only geometry output
    is a Makie contour plot (src/Visualizations/VisualizeIsosurface.jl)."""
    a = np.ascontiguousarray(values)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    dims, origin, spacing = _iso_lattice(grid, smooth)
    if a.size != dims[0] * dims[1] * dims[2]:
        raise L.R2SError(f"values length ({a.size}) doesn't match the lattice {tuple(dims)}")
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_extract_isosurface(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), dims, origin, spacing,
                                           float(iso), int(device), None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
    return _last_isosurface()


def extract_isosurface_dev(t, grid, smooth=None, *, iso=0.0, stream=None):
    """extract_isosurface on a torch tensor on the current device (float32 / float64, contiguous, x fastest) -> (verts, tris)
    as device tensors.  Counts first, then allocates and emits: the kernels run twice."""
    import torch
    if t.dtype not in (torch.float32, torch.float64) or not t.is_contiguous() or not t.is_cuda:
        raise L.R2SError("t must be a contiguous float32 / float64 device tensor")
    dims, origin, spacing = _iso_lattice(grid, smooth)
    if t.numel() != dims[0] * dims[1] * dims[2]:
        raise L.R2SError(f"values length ({t.numel()}) doesn't match the lattice {tuple(dims)}")
    st = _stream(stream)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    f32 = int(t.dtype == torch.float32)
    L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(t.data_ptr()), f32, dims, origin, spacing, float(iso), None, 0, None,
                                               0, ctypes.byref(nv), ctypes.byref(nt), st))
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=t.device)
    tris = torch.empty((nt.value, 3), dtype=torch.int32, device=t.device)
    if nv.value or nt.value:
        L.check(L.lib().r2s_extract_isosurface_dev(ctypes.c_void_p(t.data_ptr()), f32, dims, origin, spacing, float(iso),
                                                   ctypes.c_void_p(verts.data_ptr()), nv.value, ctypes.c_void_p(tris.data_ptr()),
                                                   nt.value, ctypes.byref(nv), ctypes.byref(nt), st))
    return verts, tris


def _dist_lattice(grid_or_lattice, smooth):
    """a Grid (with `smooth`, as _iso_lattice) or an explicit lattice (dims, origin, spacing)"""
    if isinstance(grid_or_lattice, Grid):
        return _iso_lattice(grid_or_lattice, smooth)
    dims, origin, spacing = grid_or_lattice
    return (ctypes.c_int64 * 3)(*[int(n) for n in dims]), (ctypes.c_double * 3)(*[float(x) for x in origin]), float(spacing)


def mesh_distance(verts, tris, grid_or_lattice, band, *, smooth=None, want_index=False, device=-1):
    """The unsigned Euclidean distance from every lattice point to the triangle mesh (verts (nv, 3) float32, tris (nt, 3)
    int32, 0-based), exact within `band` and clamped to it (include/rho2sdf_hip.h, r2s_mesh_distance) -> float64 array
    (nz, ny, nx); want_index=True: also the int32 index of the closest triangle (-1 where the result is `band`).  The lattice
    is that of extract_isosurface for a Grid and `smooth`, or an explicit (dims, origin, spacing)."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
    res, p_dist, p_idx = _dist_outputs((dims[2], dims[1], dims[0]), np.float64, want_index)
    L.check(L.lib().r2s_mesh_distance(_f(v), len(v), t.ctypes.data_as(L.c_int32_p), len(t), dims, origin, spacing, float(band), 0,
                                      int(device), p_dist, p_idx))
    return res


def mesh_distance_dev(verts, tris, grid_or_lattice, band, *, smooth=None, want_index=False, dtype=None, stream=None):
    """mesh_distance on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous) -> a
    device tensor (nz, ny, nx) of `dtype` (float64 by default, or float32)"""
    import torch
    _mesh_tensors(verts, tris)
    dtype = _float_dtype(dtype, torch)
    dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
    res, p_dist, p_idx = _dist_outputs((dims[2], dims[1], dims[0]), dtype, want_index, verts.device)
    L.check(L.lib().r2s_mesh_distance_dev(ctypes.c_void_p(verts.data_ptr()), verts.numel() // 3, ctypes.c_void_p(tris.data_ptr()),
                                          tris.numel() // 3, dims, origin, spacing, float(band), int(dtype == torch.float32),
                                          p_dist, p_idx, _stream(stream)))
    return res


def redistance(values, grid, smooth=None, *, iso=0.0, band, device=-1):
    """The banded signed distance to the iso-surface of `values` (include/rho2sdf_hip.h, r2s_redistance): s * min(d, band)
    with s = +1 where values >= iso and -1 elsewhere, d the exact distance to the mesh extract_isosurface returns for the
    same arguments.  Same conventions as extract_isosurface; the result has the shape (nz, ny, nx) and the type of the
    (float32 / float64) input."""
    a = np.ascontiguousarray(values)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    dims, origin, spacing = _iso_lattice(grid, smooth)
    if a.size != dims[0] * dims[1] * dims[2]:
        raise L.R2SError(f"values length ({a.size}) doesn't match the lattice {tuple(dims)}")
    out = np.empty((dims[2], dims[1], dims[0]), a.dtype)
    L.check(L.lib().r2s_redistance(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), dims, origin, spacing, float(iso),
                                   float(band), int(device), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def redistance_dev(t, grid, smooth=None, *, iso=0.0, band, stream=None):
    """redistance on a torch tensor on the current device (float32 / float64, contiguous, x fastest) -> a device tensor"""
    import torch
    if t.dtype not in (torch.float32, torch.float64) or not t.is_contiguous() or not t.is_cuda:
        raise L.R2SError("t must be a contiguous float32 / float64 device tensor")
    dims, origin, spacing = _iso_lattice(grid, smooth)
    if t.numel() != dims[0] * dims[1] * dims[2]:
        raise L.R2SError(f"values length ({t.numel()}) doesn't match the lattice {tuple(dims)}")
    out = torch.empty((dims[2], dims[1], dims[0]), dtype=t.dtype, device=t.device)
    st = _stream(stream)
    L.check(L.lib().r2s_redistance_dev(ctypes.c_void_p(t.data_ptr()), int(t.dtype == torch.float32), dims, origin, spacing, float(iso),
                                       float(band), ctypes.c_void_p(out.data_ptr()), st))
    return out


def last_distance_stats():
    """phases and counters of the calling thread's last distance call (r2s_last_distance_stats)"""
    s = (ctypes.c_double * 8)()
    L.lib().r2s_last_distance_stats(s)
    keys = ("ms_extract", "ms_binning", "ms_tile_kernel", "pairs", "batches", "n_tris", "n_tiles", "n_active_tiles")
    return dict(zip(keys, [float(x) for x in s]))


_INSIDE_RULES = {"positive": 0, "nonzero": 1, "odd": 2}


def _inside_rule(rule):
    """"positive" / "nonzero" / "odd", or the library's R2S_INSIDE_* integer 0 / 1 / 2 -> that integer"""
    if isinstance(rule, str) and rule in _INSIDE_RULES:
        return _INSIDE_RULES[rule]
    if not isinstance(rule, str) and rule in (0, 1, 2):
        return int(rule)
    raise L.R2SError('rule must be "positive", "nonzero" or "odd" (or 0, 1, 2)')


class MeshIndex:
    """A bounding-volume hierarchy over a triangle mesh on the device (include/rho2sdf_hip.h, r2s_mesh_index): the exact
    distance to the mesh from arbitrary points (`distance`) or from every point of a lattice (`lattice`), without a band.
    verts (nv, 3) float32, tris (nt, 3) int32, 0-based; numpy arrays, or torch tensors on the current device (then `device` is
    ignored).  A context manager; `close()` frees the device memory."""

    def __init__(self, verts, tris, device=-1):
        h = ctypes.c_void_p()
        if type(verts).__module__.startswith("torch"):
            _mesh_tensors(verts, tris)
            L.check(L.lib().r2s_mesh_index_build_dev(ctypes.c_void_p(verts.data_ptr()), verts.numel() // 3,
                                                     ctypes.c_void_p(tris.data_ptr()), tris.numel() // 3, _stream(None), ctypes.byref(h)))
        else:
            v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
            t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
            L.check(L.lib().r2s_mesh_index_build(_f(v), len(v), t.ctypes.data_as(L.c_int32_p), len(t), int(device), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            L.lib().r2s_mesh_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the loader's globals may be gone already
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if not self._h:
            raise L.R2SError("the index is closed")
        return self._h

    def info(self):
        """{n_tris, n_nodes (leaves + internal), depth (internal levels), device_bytes}"""
        out = (ctypes.c_int64 * 4)()
        L.check(L.lib().r2s_mesh_index_info(self._handle(), out))
        return dict(zip(("n_tris", "n_nodes", "depth", "device_bytes"), [int(x) for x in out]))

    def distance(self, points, want_index=False, dtype=np.float64):
        """distance of every point ((n, 3), float32 or float64; other types are converted to float64) to the mesh -> (n,)
        array of `dtype` (float64 or float32); want_index=True: also the int32 index of the closest triangle.  An empty mesh
        gives inf / -1, a non-finite point NaN / -1."""
        p = np.ascontiguousarray(points)
        if p.dtype not in (np.float32, np.float64):
            p = p.astype(np.float64)
        _points_nx3("points must be (n, 3)", p)
        dtype = _float_dtype(dtype, np)
        res, p_dist, p_idx = _dist_outputs(len(p), dtype, want_index)
        L.check(L.lib().r2s_mesh_index_query(self._handle(), p.ctypes.data_as(ctypes.c_void_p), int(p.dtype == np.float32), len(p),
                                             int(dtype == np.float32), p_dist, p_idx))
        return res

    def distance_dev(self, t, want_index=False, dtype=None, stream=None):
        """distance on a torch tensor of points on the index's device ((n, 3) float32 / float64, contiguous) -> device
        tensor(s); enqueued on the current stream (or `stream`)"""
        import torch
        _points_nx3("points must be a contiguous float32 / float64 (n, 3) device tensor", t)
        dtype = _float_dtype(dtype, torch)
        n = t.shape[0]
        res, p_dist, p_idx = _dist_outputs(n, dtype, want_index, t.device)
        if n:
            L.check(L.lib().r2s_mesh_index_query_dev(self._handle(), ctypes.c_void_p(t.data_ptr()), int(t.dtype == torch.float32), n,
                                                     int(dtype == torch.float32), p_dist, p_idx, _stream(stream)))
        return res

    def lattice(self, grid_or_lattice, smooth=None, want_index=False, dtype=np.float64):
        """distance of every lattice point (a Grid with `smooth`, as extract_isosurface, or (dims, origin, spacing)) -> array
        (nz, ny, nx) of `dtype`; want_index=True: also the closest triangle"""
        dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
        dtype = _float_dtype(dtype, np)
        res, p_dist, p_idx = _dist_outputs((dims[2], dims[1], dims[0]), dtype, want_index)
        L.check(L.lib().r2s_mesh_index_lattice(self._handle(), dims, origin, spacing, int(dtype == np.float32), p_dist, p_idx))
        return res

    def lattice_dev(self, grid_or_lattice, smooth=None, want_index=False, dtype=None, stream=None):
        """lattice -> torch tensor(s) on the current device (the index's); enqueued on the current stream (or `stream`)"""
        import torch
        dtype = _float_dtype(dtype, torch)
        dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
        dev = torch.device("cuda", torch.cuda.current_device())
        res, p_dist, p_idx = _dist_outputs((dims[2], dims[1], dims[0]), dtype, want_index, dev)
        L.check(L.lib().r2s_mesh_index_lattice_dev(self._handle(), dims, origin, spacing, int(dtype == torch.float32), p_dist, p_idx,
                                                   _stream(stream)))
        return res

    @staticmethod
    def _window(t_min, t_max):
        t_min, t_max = float(t_min), float(t_max)
        if t_min != t_min or t_max != t_max or t_min > t_max:
            raise L.R2SError("t_min <= t_max is required, neither may be NaN")
        return t_min, t_max

    def raycast(self, origins, directions, t_min=0.0, t_max=float("inf"), want_index=False, want_side=False, dtype=np.float64):
        """first hit of every ray origins[i] + t * directions[i] with t_min <= t <= t_max (include/rho2sdf_hip.h,
        r2s_mesh_index_raycast).  Both arrays (n, 3); both float32, or else both are taken as float64.  Directions are not
        normalised: t is a length only for unit directions.  -> t (n,) of `dtype` (float64 or float32): inf on a miss, NaN for
        a ray with a non-finite entry or a zero direction; want_index=True: also the int32 index of the triangle hit (-1:
        none); want_side=True: also int8 +1 (the ray enters through the front of the winding), -1 (through the back), 0."""
        o, d = np.ascontiguousarray(origins), np.ascontiguousarray(directions)
        if o.dtype != np.float32 or d.dtype != np.float32:
            o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        _points_nx3("origins and directions must both be (n, 3)", o, d, same_shape=True)
        dtype = _float_dtype(dtype, np)
        t_min, t_max = self._window(t_min, t_max)
        n = len(o)
        t = np.empty(n, dtype)
        idx = np.empty(n, np.int32) if want_index else None
        side = np.empty(n, np.int8) if want_side else None
        vp = ctypes.c_void_p
        L.check(L.lib().r2s_mesh_index_raycast(self._handle(), o.ctypes.data_as(vp), d.ctypes.data_as(vp), int(o.dtype == np.float32), n,
                                               t_min, t_max, int(dtype == np.float32), t.ctypes.data_as(vp),
                                               idx.ctypes.data_as(L.c_int32_p) if want_index else None,
                                               side.ctypes.data_as(vp) if want_side else None))
        res = (t,) + ((idx,) if want_index else ()) + ((side,) if want_side else ())
        return res if len(res) > 1 else t

    def raycast_dev(self, origins, directions, t_min=0.0, t_max=float("inf"), want_index=False, want_side=False, dtype=None,
                    stream=None):
        """raycast on torch tensors on the index's device ((n, 3), contiguous, both float32 or both float64) -> device
        tensor(s); enqueued on the current stream (or `stream`)"""
        import torch
        _points_nx3("origins / directions must be contiguous float32 / float64 (n, 3) device tensors", origins, directions)
        if origins.dtype != directions.dtype or origins.shape != directions.shape or origins.device != directions.device:
            raise L.R2SError("origins and directions must agree in type, shape and device")
        dtype = _float_dtype(dtype, torch)
        t_min, t_max = self._window(t_min, t_max)
        n = origins.shape[0]
        t = torch.empty(n, dtype=dtype, device=origins.device)
        idx = torch.empty(n, dtype=torch.int32, device=origins.device) if want_index else None
        side = torch.empty(n, dtype=torch.int8, device=origins.device) if want_side else None
        if n:
            vp = ctypes.c_void_p
            L.check(L.lib().r2s_mesh_index_raycast_dev(self._handle(), vp(origins.data_ptr()), vp(directions.data_ptr()),
                                                       int(origins.dtype == torch.float32), n, t_min, t_max, int(dtype == torch.float32),
                                                       vp(t.data_ptr()), vp(idx.data_ptr()) if want_index else None,
                                                       vp(side.data_ptr()) if want_side else None, _stream(stream)))
        res = (t,) + ((idx,) if want_index else ()) + ((side,) if want_side else ())
        return res if len(res) > 1 else t

    def winding(self, points, ray=2, want_crossings=False):
        """The winding number of every point ((n, 3), float32 or float64; other types are converted to float64) against the mesh
        (include/rho2sdf_hip.h, r2s_mesh_index_winding): minus the signed count of crossings of the axis ray `ray` (0, 1, 2 = +x,
        +y, +z; 3, 4, 5 = -x, -y, -z) -> (n,) int32: +1 inside an outward-wound closed body, 0 outside; want_crossings=True: also
        the int32 number of crossings.  A non-finite point gives 0 / -1, an empty mesh 0 / 0; a point ON the surface gets a
        ray-dependent answer."""
        p = np.ascontiguousarray(points)
        if p.dtype not in (np.float32, np.float64):
            p = p.astype(np.float64)
        _points_nx3("points must be (n, 3)", p)
        w = np.empty(len(p), np.int32)
        c = np.empty(len(p), np.int32) if want_crossings else None
        L.check(L.lib().r2s_mesh_index_winding(self._handle(), p.ctypes.data_as(ctypes.c_void_p), int(p.dtype == np.float32), len(p),
                                               int(ray), w.ctypes.data_as(L.c_int32_p), c.ctypes.data_as(L.c_int32_p) if want_crossings else None))
        return (w, c) if want_crossings else w

    def winding_dev(self, t, ray=2, want_crossings=False, stream=None):
        """winding on a torch tensor of points on the index's device ((n, 3) float32 / float64, contiguous) -> int32 device
        tensor(s); enqueued on the current stream (or `stream`)"""
        import torch
        _points_nx3("points must be a contiguous float32 / float64 (n, 3) device tensor", t)
        n = t.shape[0]
        w = torch.empty(n, dtype=torch.int32, device=t.device)
        c = torch.empty(n, dtype=torch.int32, device=t.device) if want_crossings else None
        if n:
            vp = ctypes.c_void_p
            L.check(L.lib().r2s_mesh_index_winding_dev(self._handle(), vp(t.data_ptr()), int(t.dtype == torch.float32), n, int(ray),
                                                       vp(w.data_ptr()), vp(c.data_ptr()) if want_crossings else None, _stream(stream)))
        return (w, c) if want_crossings else w

    def winding_lattice(self, grid_or_lattice, smooth=None, ray=2, want_crossings=False):
        """winding of every lattice point (a Grid with `smooth`, as extract_isosurface, or (dims, origin, spacing)) -> int32
        array (nz, ny, nx); want_crossings=True: also the number of crossings"""
        dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
        shape = (dims[2], dims[1], dims[0])
        w = np.empty(shape, np.int32)
        c = np.empty(shape, np.int32) if want_crossings else None
        L.check(L.lib().r2s_mesh_index_winding_lattice(self._handle(), dims, origin, spacing, int(ray), w.ctypes.data_as(L.c_int32_p),
                                                       c.ctypes.data_as(L.c_int32_p) if want_crossings else None))
        return (w, c) if want_crossings else w

    def winding_lattice_dev(self, grid_or_lattice, smooth=None, ray=2, want_crossings=False, stream=None):
        """winding_lattice -> int32 torch tensor(s) on the current device (the index's); enqueued on the current stream (or `stream`)"""
        import torch
        dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
        shape, dev = (dims[2], dims[1], dims[0]), torch.device("cuda", torch.cuda.current_device())
        w = torch.empty(shape, dtype=torch.int32, device=dev)
        c = torch.empty(shape, dtype=torch.int32, device=dev) if want_crossings else None
        vp = ctypes.c_void_p
        L.check(L.lib().r2s_mesh_index_winding_lattice_dev(self._handle(), dims, origin, spacing, int(ray), vp(w.data_ptr()),
                                                           vp(c.data_ptr()) if want_crossings else None, _stream(stream)))
        return (w, c) if want_crossings else w

    def contains(self, points, rule="positive", ray=2):
        """is every point inside the mesh? -> (n,) bool.  rule: "positive" (winding > 0), "nonzero" (winding != 0) or "odd" (the
        number of crossings is odd: the rule that survives inconsistent winding).  A non-finite point is outside."""
        rule = _inside_rule(rule)
        w, c = self.winding(points, ray, want_crossings=True)
        return (w > 0, w != 0, (c > 0) & (c % 2 == 1))[rule]

    def signed_distance(self, points, rule="positive", ray=2, want_index=False, dtype=np.float64):
        """The signed distance of every point to the mesh (include/rho2sdf_hip.h, r2s_mesh_index_signed): `distance` of the same
        points with the sign of `contains`: positive inside (in the material), negative outside, a zero is +0.  An empty mesh
        gives -inf, a non-finite point NaN.  want_index as in `distance`."""
        p = np.ascontiguousarray(points)
        if p.dtype not in (np.float32, np.float64):
            p = p.astype(np.float64)
        _points_nx3("points must be (n, 3)", p)
        dtype = _float_dtype(dtype, np)
        res, p_dist, p_idx = _dist_outputs(len(p), dtype, want_index)
        L.check(L.lib().r2s_mesh_index_signed(self._handle(), p.ctypes.data_as(ctypes.c_void_p), int(p.dtype == np.float32), len(p),
                                              _inside_rule(rule), int(ray), int(dtype == np.float32), p_dist, p_idx))
        return res

    def signed_distance_dev(self, t, rule="positive", ray=2, want_index=False, dtype=None, stream=None):
        """signed_distance on a torch tensor of points on the index's device ((n, 3) float32 / float64, contiguous) -> device
        tensor(s); enqueued on the current stream (or `stream`)"""
        import torch
        _points_nx3("points must be a contiguous float32 / float64 (n, 3) device tensor", t)
        dtype = _float_dtype(dtype, torch)
        n = t.shape[0]
        res, p_dist, p_idx = _dist_outputs(n, dtype, want_index, t.device)
        if n:
            L.check(L.lib().r2s_mesh_index_signed_dev(self._handle(), ctypes.c_void_p(t.data_ptr()), int(t.dtype == torch.float32), n,
                                                      _inside_rule(rule), int(ray), int(dtype == torch.float32), p_dist, p_idx,
                                                      _stream(stream)))
        return res

    def signed_lattice(self, grid_or_lattice, smooth=None, rule="positive", ray=2, want_index=False, dtype=np.float64):
        """signed_distance of every lattice point (a Grid with `smooth`, as extract_isosurface, or (dims, origin, spacing)) ->
        array (nz, ny, nx) of `dtype`; want_index=True: also the closest triangle"""
        dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
        dtype = _float_dtype(dtype, np)
        res, p_dist, p_idx = _dist_outputs((dims[2], dims[1], dims[0]), dtype, want_index)
        L.check(L.lib().r2s_mesh_index_signed_lattice(self._handle(), dims, origin, spacing, _inside_rule(rule), int(ray),
                                                      int(dtype == np.float32), p_dist, p_idx))
        return res

    def signed_lattice_dev(self, grid_or_lattice, smooth=None, rule="positive", ray=2, want_index=False, dtype=None, stream=None):
        """signed_lattice -> torch tensor(s) on the current device (the index's); enqueued on the current stream (or `stream`)"""
        import torch
        dtype = _float_dtype(dtype, torch)
        dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
        dev = torch.device("cuda", torch.cuda.current_device())
        res, p_dist, p_idx = _dist_outputs((dims[2], dims[1], dims[0]), dtype, want_index, dev)
        L.check(L.lib().r2s_mesh_index_signed_lattice_dev(self._handle(), dims, origin, spacing, _inside_rule(rule), int(ray),
                                                          int(dtype == torch.float32), p_dist, p_idx, _stream(stream)))
        return res

    def self_intersections(self, want_pairs=True):
        """The pairs of triangles of the indexed mesh that intersect or touch (include/rho2sdf_hip.h,
        r2s_mesh_index_intersections) -> MeshIntersections; want_pairs=False: counts only (`pairs` is None).  The index is not
        changed."""
        h = self._handle()
        nt = self.info()["n_tris"]
        return _intersections_host(nt, want_pairs, lambda hits, pairs, cap, tot: L.lib().r2s_mesh_index_intersections(h, hits, pairs, cap, tot))

    def self_intersections_dev(self, want_pairs=True, stream=None, *, capacity=0):
        """self_intersections with the results on the index's device, which must be current: `hits_of_tri` and `pairs` are torch
        tensors, `totals` a numpy array.  Reads after the work queued on the current stream (or `stream`); synchronous."""
        h = self._handle()
        nt = self.info()["n_tris"]
        return _intersections_dev(nt, want_pairs, capacity, stream,
                                  lambda hits, pairs, cap, tot, st: L.lib().r2s_mesh_index_intersections_dev(h, hits, pairs, cap, tot, st))


class MeshIntersections:
    """The self-intersections of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_index_intersections): `pairs` (n, 2) int32, the
    intersecting or touching pairs (s, t) with s < t, ascending by (s, t) (None when they were not asked for); `hits_of_tri` (nt,)
    int32, the number of pairs each triangle is in; `totals` (8,) int64 (intersecting pairs, triangles involved, candidate pairs,
    candidates skipped as adjacent, candidates sharing exactly one vertex index, collapsed triangles, 0, 0).  len() is the number
    of pairs; `tris` the ascending indices of the triangles involved.  Coplanar overlap is not reported; contact counts, so weld a
    soup first.  numpy arrays, or (from the *_dev calls) torch tensors for pairs and hits_of_tri."""

    def __init__(self, pairs, hits_of_tri, totals):
        self.pairs, self.hits_of_tri, self.totals = pairs, hits_of_tri, totals

    def __len__(self):
        return int(self.totals[0])

    @property
    def tris(self):
        h = self.hits_of_tri
        return np.nonzero(h)[0] if isinstance(h, np.ndarray) else h.nonzero().reshape(-1)


def _intersections_host(nt, want_pairs, call):
    """the two-call capacity protocol of the host entry points: counts first, then the pairs into room for all of them"""
    hits, tot = np.zeros(nt, np.int32), np.zeros(8, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
    L.check(call(ip(hits), None, 0, _i(tot)))
    if not want_pairs:
        return MeshIntersections(None, hits, tot)
    pairs = np.empty((int(tot[0]), 2), np.int32)
    if len(pairs):
        L.check(call(ip(hits), ip(pairs), len(pairs), _i(tot)))
    return MeshIntersections(pairs, hits, tot)


def _intersections_dev(nt, want_pairs, capacity, stream, call):
    import torch
    st = _stream(stream)
    dev = torch.device("cuda", torch.cuda.current_device())
    hits, tot = torch.zeros(nt, dtype=torch.int32, device=dev), np.zeros(8, np.int64)
    vp = ctypes.c_void_p
    cap = int(capacity) if want_pairs else 0
    while True:
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        L.check(call(vp(hits.data_ptr()) if nt else None, vp(pairs.data_ptr()) if cap else None, cap, _i(tot), st))
        if not want_pairs or tot[0] <= cap:
            break
        cap = int(tot[0])
    return MeshIntersections(pairs[:int(tot[0])] if want_pairs else None, hits, tot)


def mesh_intersections(verts, tris, *, device=-1):
    """The self-intersections of a triangle mesh without an index (verts (nv, 3) float32, tris (nt, 3) int32, 0-based) ->
    MeshIntersections: the library builds a tree, uses it and drops it.  With a MeshIndex at hand use its self_intersections()."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    pv, pt = _f(v) if len(v) else None, t.ctypes.data_as(L.c_int32_p) if len(t) else None
    return _intersections_host(len(t), True, lambda hits, pairs, cap, tot: L.lib().r2s_mesh_intersections(
        pv, len(v), pt, len(t), int(device), hits, pairs, cap, tot))


def mesh_intersections_dev(verts, tris, stream=None, *, capacity=0):
    """mesh_intersections on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous); pairs
    and hits_of_tri stay device tensors.  The library writes the pairs only into room for all of them: with more pairs than
    `capacity` the call is made a second time."""
    _mesh_tensors(verts, tris)
    vp = ctypes.c_void_p
    nv, nt = verts.numel() // 3, tris.numel() // 3
    return _intersections_dev(nt, True, capacity, stream, lambda hits, pairs, cap, tot, st: L.lib().r2s_mesh_intersections_dev(
        vp(verts.data_ptr()), nv, vp(tris.data_ptr()), nt, hits, pairs, cap, tot, st))


def mesh_signed_distance(verts, tris, grid_or_lattice, smooth=None, *, rule="positive", ray=2, dtype=np.float64, device=-1):
    """The signed distance from every lattice point to a closed triangle mesh, the sign taken from the mesh alone
    (include/rho2sdf_hip.h, r2s_mesh_signed_distance): MeshIndex(verts, tris).signed_lattice(...) without keeping the index ->
    array (nz, ny, nx) of `dtype` (float64 or float32), positive inside.  The lattice is that of extract_isosurface for a Grid
    and `smooth`, or an explicit (dims, origin, spacing); rule and ray as in MeshIndex.contains.  The mesh should be closed,
    consistently wound outward (mesh_orient(outward=True)) and free of self-intersections (mesh_intersections); with windings
    that cannot be trusted use rule="odd"."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
    dtype = _float_dtype(dtype, np)
    out = np.empty((dims[2], dims[1], dims[0]), dtype)
    L.check(L.lib().r2s_mesh_signed_distance(_f(v), len(v), t.ctypes.data_as(L.c_int32_p), len(t), dims, origin, spacing,
                                             _inside_rule(rule), int(ray), int(dtype == np.float32), int(device),
                                             out.ctypes.data_as(ctypes.c_void_p)))
    return out


def mesh_signed_distance_dev(verts, tris, grid_or_lattice, smooth=None, *, rule="positive", ray=2, dtype=None, stream=None):
    """mesh_signed_distance on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous) -> a
    device tensor (nz, ny, nx) of `dtype` (float64 by default, or float32).  Reads after the work queued on the current stream
    (or `stream`); synchronous."""
    import torch
    _mesh_tensors(verts, tris)
    dtype = _float_dtype(dtype, torch)
    dims, origin, spacing = _dist_lattice(grid_or_lattice, smooth)
    out = torch.empty((dims[2], dims[1], dims[0]), dtype=dtype, device=verts.device)
    L.check(L.lib().r2s_mesh_signed_distance_dev(ctypes.c_void_p(verts.data_ptr()), verts.numel() // 3, ctypes.c_void_p(tris.data_ptr()),
                                                 tris.numel() // 3, dims, origin, spacing, _inside_rule(rule), int(ray),
                                                 int(dtype == torch.float32), ctypes.c_void_p(out.data_ptr()), _stream(stream)))
    return out


class MeshShells:
    """The shells of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_shells): the raw tables and what follows from them.
    Raw: `counts` (n, 8) int64 (first_tri, n_tris, n_verts, n_edges, n_boundary, n_flipped, n_nonmanifold, 0), `sums` (n, 11)
    float64 (area, volume, first moments x y z and second moments xx yy zz xy xz yz about `ref_point`), `ref_point` (3,),
    `totals` (8,) int64 (shells, triangles, collapsed, edges, boundary, flipped, non-manifold, referenced vertices) and
    `shell_of_tri` (-1 for a collapsed triangle; a device tensor from mesh_shells_dev).  Derived, in float64 numpy:
        closed        = (n_boundary == 0) & (n_flipped == 0) & (n_nonmanifold == 0)
        euler         = n_verts - n_edges + n_tris
        genus         = (2 - euler) // 2 for closed shells, else -1
        is_void       = closed & (volume < 0)
        centroid      = ref_point + M1 / volume                         M1 = sums[:, 2:5]
        second_moment = P - volume * d d^T  (n, 3, 3)                   P the symmetric matrix of sums[:, 5:11], d = M1 / volume
        inertia       = trace(second_moment) * identity - second_moment (unit density, about the centroid)
    centroid, second_moment and inertia are NaN unless the shell is closed with a non-zero volume."""

    def __init__(self, counts, sums, ref_point, totals, shell_of_tri):
        self.counts, self.sums, self.ref_point, self.totals, self.shell_of_tri = counts, sums, ref_point, totals, shell_of_tri

    n_shells = property(lambda s: len(s.counts))
    first_tri = property(lambda s: s.counts[:, 0])
    n_tris = property(lambda s: s.counts[:, 1])
    n_verts = property(lambda s: s.counts[:, 2])
    n_edges = property(lambda s: s.counts[:, 3])
    n_boundary = property(lambda s: s.counts[:, 4])
    n_flipped = property(lambda s: s.counts[:, 5])
    n_nonmanifold = property(lambda s: s.counts[:, 6])
    area = property(lambda s: s.sums[:, 0])
    volume = property(lambda s: s.sums[:, 1])
    closed = property(lambda s: (s.n_boundary == 0) & (s.n_flipped == 0) & (s.n_nonmanifold == 0))
    euler = property(lambda s: s.n_verts - s.n_edges + s.n_tris)
    genus = property(lambda s: np.where(s.closed, (2 - s.euler) // 2, -1))
    is_void = property(lambda s: s.closed & (s.volume < 0))

    def __len__(self):
        return len(self.counts)

    def _offset(self):
        """d = M1 / volume, NaN unless closed with a non-zero volume"""
        ok = self.closed & (self.volume != 0)
        v = np.where(ok, self.volume, np.nan)
        return self.sums[:, 2:5] / v[:, None], v

    @property
    def centroid(self):
        return self.ref_point[None, :] + self._offset()[0]

    @property
    def second_moment(self):
        d, v = self._offset()
        q = self.sums[:, 5:11]
        P = np.stack([q[:, [0, 3, 4]], q[:, [3, 1, 5]], q[:, [4, 5, 2]]], axis=1)
        return P - v[:, None, None] * d[:, :, None] * d[:, None, :]

    @property
    def inertia(self):
        c = self.second_moment
        return np.trace(c, axis1=1, axis2=2)[:, None, None] * np.eye(3)[None] - c


def mesh_shells(verts, tris, *, device=-1):
    """The shells of a triangle mesh (verts (nv, 3) float32, tris (nt, 3) int32, 0-based): connected components over shared
    edges, edge classes, and per shell the counts, area, volume and moments -> MeshShells (its docstring has the fields and the
    formulas of the derived ones).  One library call and a copy of the thread's last tables."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    sot = np.empty(len(t), np.int32)
    n = ctypes.c_int64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    L.check(L.lib().r2s_mesh_shells(_f(v) if len(v) else None, len(v), t.ctypes.data_as(L.c_int32_p) if len(t) else None, len(t),
                                    int(device), sot.ctypes.data_as(L.c_int32_p), ctypes.byref(n), _d(ref), _i(tot)))
    counts, sums = np.empty((n.value, 8), np.int64), np.empty((n.value, 11))
    if n.value:
        L.check(L.lib().r2s_last_mesh_shells(_i(counts), _d(sums), n.value, ctypes.byref(n)))
    return MeshShells(counts, sums, ref, tot, sot)


def mesh_shells_dev(verts, tris, stream=None, *, capacity=0):
    """mesh_shells on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous).  The tables
    come back as numpy arrays, shell_of_tri stays a device tensor.  The library writes the tables only into room for all shells:
    with more shells than `capacity` the call is made a second time."""
    import torch
    _mesh_tensors(verts, tris)
    st = _stream(stream)
    nt = tris.numel() // 3
    sot = torch.empty(nt, dtype=torch.int32, device=verts.device)
    n = ctypes.c_int64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    cap = int(capacity)
    while True:
        counts = torch.empty((cap, 8), dtype=torch.int64, device=verts.device)
        sums = torch.empty((cap, 11), dtype=torch.float64, device=verts.device)
        vp = ctypes.c_void_p
        L.check(L.lib().r2s_mesh_shells_dev(vp(verts.data_ptr()), verts.numel() // 3, vp(tris.data_ptr()), nt, vp(sot.data_ptr()),
                                            vp(counts.data_ptr()) if cap else None, vp(sums.data_ptr()) if cap else None, cap,
                                            ctypes.byref(n), _d(ref), _i(tot), st))
        if n.value <= cap:
            break
        cap = n.value
    return MeshShells(counts[:n.value].cpu().numpy(), sums[:n.value].cpu().numpy(), ref, tot, sot)


class MeshWeld:
    """The result of mesh_weld (include/rho2sdf_hip.h, r2s_mesh_weld): `verts` (nv_out, 3) float32, every row an input vertex bit
    for bit, in first-occurrence order; `tris` (nt_out, 3) int32 into them; `vert_map` (nv_in,) and `tri_map` (nt_in,) int32,
    input index -> output index or -1 for what was dropped; `totals` (8,) int64 (output vertices, output triangles, vertices
    merged away, collapsed triangles, same-orientation duplicates, opposite pairs, unreferenced classes, 0).  numpy arrays from
    mesh_weld, device tensors (totals stays numpy) from mesh_weld_dev."""

    def __init__(self, verts, tris, vert_map, tri_map, totals):
        self.verts, self.tris, self.vert_map, self.tri_map, self.totals = verts, tris, vert_map, tri_map, totals

    n_verts = property(lambda s: int(s.totals[0]))
    n_tris = property(lambda s: int(s.totals[1]))
    n_merged = property(lambda s: int(s.totals[2]))
    n_collapsed = property(lambda s: int(s.totals[3]))
    n_duplicates = property(lambda s: int(s.totals[4]))
    n_opposite = property(lambda s: int(s.totals[5]))
    n_unused = property(lambda s: int(s.totals[6]))


def _weld_flags(drop_collapsed, drop_duplicates, drop_unused):
    return (L.WELD_DROP_COLLAPSED if drop_collapsed else 0) | (L.WELD_DROP_DUPLICATES if drop_duplicates else 0) \
        | (L.WELD_DROP_UNUSED if drop_unused else 0)


def mesh_weld(verts, tris=None, *, snap=0.0, drop_collapsed=True, drop_duplicates=False, drop_unused=True, device=-1):
    """Welds the vertices of a triangle mesh that are the same point (verts (nv, 3) float32; tris (nt, 3) int32 0-based, or None
    for a triangle soup: triangle t = vertices 3t, 3t + 1, 3t + 2) -> MeshWeld.  snap = 0: the same iff x, y and z compare equal
    as float32; snap > 0: iff they fall into the same cell floor(v / snap) per axis - grid snapping, NOT a distance tolerance:
    two points closer than snap on either side of a cell face stay apart.  Output vertices are copies of the first input vertex
    of each class, in first-occurrence order; surviving triangles keep their order and corner order.  drop_collapsed drops the
    triangles with two equal indices after the weld, drop_duplicates all but the first of the triangles equal up to a rotation
    of their corners, drop_unused the vertices no surviving triangle references.
    The mesh of extract_isosurface is already topologically closed; welding its exact-iso vertices collapses zero-area triangles
    and can leave non-manifold edges, which mesh_shells reports, and non-manifold (pinched) vertices, which mesh_shells cannot
    see: mesh_fans reports them and mesh_fans(split=True) repairs them.  So the weld is offered, not applied by default."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    if t is None and len(v) % 3:
        raise L.R2SError("a soup (tris=None) needs a multiple of 3 vertices")
    nt = len(v) // 3 if t is None else len(t)
    vo, to = np.empty((len(v), 3), np.float32), np.empty((nt, 3), np.int32)
    vm, tm = np.empty(len(v), np.int32), np.empty(nt, np.int32)
    tot = np.zeros(8, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)
    pad = np.zeros(3, np.int32)   # (a non-NULL pointer for a mesh without triangles: NULL means soup)
    L.check(L.lib().r2s_mesh_weld(_f(v) if len(v) else None, len(v), None if t is None else ip(t if len(t) else pad), nt, float(snap),
                                  _weld_flags(drop_collapsed, drop_duplicates, drop_unused), int(device), _f(vo), ip(to), ip(vm),
                                  ip(tm), _i(tot)))
    return MeshWeld(vo[:tot[0]].copy(), to[:tot[1]].copy(), vm, tm, tot)


def mesh_weld_dev(verts, tris=None, stream=None, *, snap=0.0, drop_collapsed=True, drop_duplicates=False, drop_unused=True):
    """mesh_weld on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3) or None, contiguous).  All four
    arrays of the MeshWeld stay device tensors, verts and tris trimmed to the counts; totals is numpy."""
    import torch
    dev = verts.device
    pad = torch.zeros(3, dtype=torch.int32, device=dev)   # (torch's empty tensors have a NULL pointer; NULL tris means soup)
    _mesh_tensors(verts, pad if tris is None else tris)
    nv = verts.numel() // 3
    if tris is None and nv % 3:
        raise L.R2SError("a soup (tris=None) needs a multiple of 3 vertices")
    nt = nv // 3 if tris is None else tris.numel() // 3
    st = _stream(stream)
    vo, to = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nt, 3), dtype=torch.int32, device=dev)
    vm, tm = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    tot = np.zeros(8, np.int64)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    L.check(L.lib().r2s_mesh_weld_dev(vp(verts), nv, None if tris is None else vp(tris if nt else pad), nt, float(snap),
                                      _weld_flags(drop_collapsed, drop_duplicates, drop_unused), vp(vo), vp(to), vp(vm), vp(tm),
                                      _i(tot), st))
    return MeshWeld(vo[:tot[0]], to[:tot[1]], vm, tm, tot)


class MeshSimplify:
    """The result of mesh_simplify (include/rho2sdf_hip.h, r2s_mesh_simplify): `verts` (nv_out, 3) float32, one computed point per
    cluster, in first-occurrence order of the cluster's first member; `tris` (nt_out, 3) int32 into them; `vert_map` (nv_in,) and
    `tri_map` (nt_in,) int32, input index -> output index or -1; per output vertex `members` (int64, the size of the cluster),
    `error` (float64, the summed squared plane distances, area-weighted, at the vertex) and `solved` (int32: 0 the mean, 1..3 the
    rank the quadric solve kept, + 4 if the point was pulled back to its cell), always numpy; `totals` (8,) int64 (output vertices,
    output triangles, members merged away, collapsed triangles, same-orientation duplicates, opposite pairs, vertices that are no
    member, pulled-back clusters).  numpy arrays from mesh_simplify, device tensors for the first four from mesh_simplify_dev."""

    def __init__(self, verts, tris, vert_map, tri_map, members, error, solved, totals):
        self.verts, self.tris, self.vert_map, self.tri_map = verts, tris, vert_map, tri_map
        self.members, self.error, self.solved, self.totals = members, error, solved, totals

    n_verts = property(lambda s: int(s.totals[0]))
    n_tris = property(lambda s: int(s.totals[1]))
    n_merged = property(lambda s: int(s.totals[2]))
    n_collapsed = property(lambda s: int(s.totals[3]))
    n_duplicates = property(lambda s: int(s.totals[4]))
    n_opposite = property(lambda s: int(s.totals[5]))
    n_unused = property(lambda s: int(s.totals[6]))
    n_pulled = property(lambda s: int(s.totals[7]))

    @property
    def ratio(self):
        """output triangles / input triangles (1.0 for an input without triangles)"""
        return self.n_tris / len(self.tri_map) if len(self.tri_map) else 1.0


_SIMPLIFY_RULES = {"mean": L.SIMPLIFY_MEAN, "quadric": L.SIMPLIFY_QUADRIC}


def _simplify_rule(rule):
    if rule not in _SIMPLIFY_RULES:
        raise L.R2SError('rule must be "mean" or "quadric"')
    return _SIMPLIFY_RULES[rule]


def _last_mesh_simplify():
    """the calling thread's last tables (r2s_last_mesh_simplify): count, then copy"""
    n = ctypes.c_int64(0)
    L.check(L.lib().r2s_last_mesh_simplify(None, None, None, 0, ctypes.byref(n)))
    members, error, solved = np.empty(n.value, np.int64), np.empty(n.value, np.float64), np.empty(n.value, np.int32)
    L.check(L.lib().r2s_last_mesh_simplify(_i(members), _d(error), solved.ctypes.data_as(L.c_int32_p), n.value, ctypes.byref(n)))
    return members, error, solved


def mesh_simplify(verts, tris, cell, rule="quadric", drop_duplicates=True, *, device=-1):
    """Vertex-clustering decimation of an indexed triangle mesh (verts (nv, 3) float32, tris (nt, 3) int32 0-based; weld a soup
    first) -> MeshSimplify.  The vertices are clustered by the cells floor(v / cell) per axis, the cells of mesh_weld(snap=cell);
    every cluster that keeps a triangle becomes one vertex: rule="mean" the Float64 mean of its members, rule="quadric" the point
    of the cell that minimises the summed squared distances to the planes of the triangles around the cluster (Lindstrom), which
    keeps edges and corners where the mean rounds them off.  Triangles with two corners in one cluster are dropped, duplicates
    with drop_duplicates; every vertex moves inside its cell, so the result is within sqrt(3) * cell of the input.
    Clustering does not preserve manifoldness: it can leave non-manifold edges (mesh_shells reports them), pinched vertices
    (mesh_fans reports and splits them), opposite pairs (totals[5]) and self-contact (mesh_intersections).  It opens no hole in a
    consistently oriented closed mesh (or with drop_duplicates=False).
    Not here: edge collapse, boundary or feature constraints, attribute transfer."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    vo, to = np.empty((len(v), 3), np.float32), np.empty((len(t), 3), np.int32)
    vm, tm = np.empty(len(v), np.int32), np.empty(len(t), np.int32)
    tot = np.zeros(8, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)
    pad = np.zeros(3, np.int32)   # (a non-NULL pointer for a mesh without triangles)
    L.check(L.lib().r2s_mesh_simplify(_f(v) if len(v) else None, len(v), ip(t if len(t) else pad), len(t), float(cell), _simplify_rule(rule),
                                      L.WELD_DROP_DUPLICATES if drop_duplicates else 0, int(device), _f(vo), ip(to), ip(vm), ip(tm),
                                      _i(tot)))
    return MeshSimplify(vo[:tot[0]].copy(), to[:tot[1]].copy(), vm, tm, *_last_mesh_simplify(), tot)


def mesh_simplify_dev(verts, tris, cell, rule="quadric", drop_duplicates=True, *, stream=None):
    """mesh_simplify on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous).  verts, tris
    and the two maps of the MeshSimplify stay device tensors, verts and tris trimmed to the counts; the per-vertex tables and
    totals are numpy."""
    import torch
    dev = verts.device
    _mesh_tensors(verts, tris)
    nv, nt = verts.numel() // 3, tris.numel() // 3
    pad = torch.zeros(3, dtype=torch.int32, device=dev)   # (torch's empty tensors have a NULL pointer)
    st = _stream(stream)
    vo, to = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nt, 3), dtype=torch.int32, device=dev)
    vm, tm = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    tot = np.zeros(8, np.int64)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())
    L.check(L.lib().r2s_mesh_simplify_dev(vp(verts), nv, vp(tris if nt else pad), nt, float(cell), _simplify_rule(rule),
                                          L.WELD_DROP_DUPLICATES if drop_duplicates else 0, vp(vo), vp(to), vp(vm), vp(tm), _i(tot), st))
    return MeshSimplify(vo[:tot[0]], to[:tot[1]], vm, tm, *_last_mesh_simplify(), tot)


def select_shells(verts, tris, shells, keep):
    """The triangles of the shells where `keep` is true -> (verts, tris) with the vertices compacted (ascending old index) and the
    indices remapped; the mesh-level counterpart of remove_sdf_artifacts.  `shells` is the MeshShells of (verts, tris); `keep` a
    boolean array with one entry per shell, or a callable on `shells` that returns one, e.g.
    lambda s: s.volume > 0.01 * s.volume.max().  Collapsed triangles (shell -1) are dropped.  Plain array code, no device."""
    v = np.asarray(verts).reshape(-1, 3)
    t = np.asarray(tris).reshape(-1, 3)
    k = np.asarray(keep(shells) if callable(keep) else keep, dtype=bool).reshape(-1)
    sot = shells.shell_of_tri
    sot = np.asarray(sot.cpu() if hasattr(sot, "cpu") else sot)
    if len(k) != shells.n_shells or len(sot) != len(t):
        raise L.R2SError("keep needs one entry per shell, and shells must belong to this mesh")
    sel = t[(sot >= 0) & np.concatenate([k, [False]])[sot]]
    used = np.zeros(len(v), bool)
    used[sel.ravel()] = True
    remap = np.cumsum(used) - 1
    return v[used], remap[sel].astype(t.dtype).reshape(-1, 3)


class MeshOrient:
    """The result of mesh_orient (include/rho2sdf_hip.h, r2s_mesh_orient): `tris` (nt, 3) int32, the input triangles in their
    order with the flipped ones written (i0, i2, i1); `flipped` (nt,) bool; `patch_of_tri` (nt,) int32 (-1 for a collapsed
    triangle); `counts` (n, 8) int64 (first_tri, n_tris, triangles flipped, status bits 1 closed / 2 non-orientable / 4 decided
    by volume, boundary half-edges, non-manifold half-edges, flipped edges of the input, 0); `volume` (n,) float64, the signed
    volume of each patch as written, about `ref_point` (3,); `totals` (8,) int64 (patches, triangles, collapsed, flipped
    triangles, non-orientable, closed, decided by volume, flipped edges left in the output).  numpy arrays from mesh_orient;
    mesh_orient_dev keeps tris, flipped and patch_of_tri on the device."""

    def __init__(self, tris, flipped, patch_of_tri, counts, volume, ref_point, totals):
        self.tris, self.flipped, self.patch_of_tri, self.counts, self.volume = tris, flipped, patch_of_tri, counts, volume
        self.ref_point, self.totals = ref_point, totals

    n_patches = property(lambda s: len(s.counts))
    first_tri = property(lambda s: s.counts[:, 0])
    n_tris = property(lambda s: s.counts[:, 1])
    n_flipped = property(lambda s: s.counts[:, 2])
    closed = property(lambda s: (s.counts[:, 3] & 1) != 0)
    orientable = property(lambda s: (s.counts[:, 3] & 2) == 0)
    by_volume = property(lambda s: (s.counts[:, 3] & 4) != 0)

    def __len__(self):
        return len(self.counts)


def mesh_orient(verts, tris, *, outward=False, device=-1):
    """A consistent winding for a triangle mesh (verts (nv, 3) float32, tris (nt, 3) int32, 0-based) -> MeshOrient.  The mesh falls
    into patches over the edges that exactly two triangles share; inside an orientable patch every triangle gets the winding of
    its neighbours, and the patch as a whole keeps the winding of the MAJORITY of its triangles (a tie: of its first triangle).
    outward=True: a closed patch with a non-zero volume is wound so that its volume is positive instead.  Nesting is ignored:
    outward=True turns an enclosed void into a body (mesh_nesting(rewind=True) on the result reverses the voids again), the majority
    rule leaves a void as most of its triangles say.  Non-orientable patches are copied unchanged and counted; no orientation is
    carried across non-manifold edges; no holes are filled.  One library call and a copy of the thread's last tables."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    out, flip, pot = np.empty((len(t), 3), np.int32), np.empty(len(t), np.int32), np.empty(len(t), np.int32)
    n = ctypes.c_int64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)
    L.check(L.lib().r2s_mesh_orient(_f(v) if len(v) else None, len(v), ip(t) if len(t) else None, len(t),
                                    L.ORIENT_OUTWARD if outward else 0, int(device), ip(out), ip(flip), ip(pot), ctypes.byref(n),
                                    _d(ref), _i(tot)))
    counts, volume = np.empty((n.value, 8), np.int64), np.empty(n.value)
    if n.value:
        L.check(L.lib().r2s_last_mesh_orient(_i(counts), _d(volume), n.value, ctypes.byref(n)))
    return MeshOrient(out, flip != 0, pot, counts, volume, ref, tot)


def mesh_orient_dev(verts, tris, stream=None, *, outward=False, capacity=0):
    """mesh_orient on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous).  The tables
    come back as numpy arrays; tris, flipped and patch_of_tri stay device tensors.  The library writes the tables only into room
    for all patches: with more patches than `capacity` the call is made a second time."""
    import torch
    _mesh_tensors(verts, tris)
    st = _stream(stream)
    dev = verts.device
    nt = tris.numel() // 3
    out = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    flip, pot = torch.empty(nt, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    n = ctypes.c_int64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    cap = int(capacity)
    vp = ctypes.c_void_p
    while True:
        counts = torch.empty((cap, 8), dtype=torch.int64, device=dev)
        volume = torch.empty(cap, dtype=torch.float64, device=dev)
        L.check(L.lib().r2s_mesh_orient_dev(vp(verts.data_ptr()), verts.numel() // 3, vp(tris.data_ptr()), nt,
                                            L.ORIENT_OUTWARD if outward else 0, vp(out.data_ptr()), vp(flip.data_ptr()),
                                            vp(pot.data_ptr()), vp(counts.data_ptr()) if cap else None,
                                            vp(volume.data_ptr()) if cap else None, cap, ctypes.byref(n), _d(ref), _i(tot), st))
        if n.value <= cap:
            break
        cap = n.value
    return MeshOrient(out, flip != 0, pot, counts[:n.value].cpu().numpy(), volume[:n.value].cpu().numpy(), ref, tot)


def flip_patches(tris, patch_of_tri, which):
    """`tris` with the triangles of the chosen patches reversed, (i0, i1, i2) -> (i0, i2, i1), e.g. the voids a user knows about
    after mesh_orient(outward=True).  `patch_of_tri` is MeshOrient.patch_of_tri (shell_of_tri of a MeshShells works the same
    way); `which` a boolean array with one entry per patch, or a list of patch numbers.  Triangles of patch -1 are left alone.
    Plain array code, no device."""
    t = np.array(tris, dtype=np.int32).reshape(-1, 3)
    pot = patch_of_tri
    pot = np.asarray(pot.cpu() if hasattr(pot, "cpu") else pot).reshape(-1)
    if len(pot) != len(t):
        raise L.R2SError("patch_of_tri needs one entry per triangle")
    n = int(pot.max()) + 1 if len(pot) else 0
    w = np.asarray(which)
    if w.dtype == bool:
        if w.shape != (n,):
            raise L.R2SError("a boolean `which` needs one entry per patch")
        sel = w
    else:
        w = w.astype(np.int64).reshape(-1)
        if len(w) and (w.min() < 0 or w.max() >= n):
            raise L.R2SError("`which` names a patch that does not exist")
        sel = np.zeros(n, bool)
        sel[w] = True
    rev = (pot >= 0) & np.concatenate([sel, [False]])[pot]
    t[rev] = t[rev][:, [0, 2, 1]]
    return t


class MeshNesting:
    """The result of mesh_nesting (include/rho2sdf_hip.h, r2s_mesh_nesting): `tris` (nt, 3) int32, with rewind=True the input
    triangles in their order with those of the closed patches at odd depth written (i0, i2, i1), else None; `patch_of_tri` (nt,)
    int32, the patches of mesh_orient (-1 for a collapsed triangle); `counts` (n, 8) int64 (first_tri, n_tris, status bits 1
    closed / 2 reversed in the output / 4 irregular, parent, depth, n_children, the sum of the crossings, 0); `pairs` (m,) int64,
    the (query, container) pairs as (P << 32) | Q, ascending; `totals` (8,) int64 (patches, triangles, collapsed, closed patches,
    containment pairs, largest depth, irregular patches, triangles reversed).  Derived on the host: parent, depth, closed,
    irregular (one entry per patch), roots (the patches without a container), children(p), voids (closed, odd depth) and bodies
    (closed, even depth) as ascending patch numbers.  numpy arrays from mesh_nesting; mesh_nesting_dev keeps tris, patch_of_tri
    and pairs on the device."""

    def __init__(self, tris, patch_of_tri, counts, pairs, totals):
        self.tris, self.patch_of_tri, self.counts, self.pairs, self.totals = tris, patch_of_tri, counts, pairs, totals

    n_patches = property(lambda s: len(s.counts))
    first_tri = property(lambda s: s.counts[:, 0])
    n_tris = property(lambda s: s.counts[:, 1])
    closed = property(lambda s: (s.counts[:, 2] & 1) != 0)
    reversed = property(lambda s: (s.counts[:, 2] & 2) != 0)
    irregular = property(lambda s: (s.counts[:, 2] & 4) != 0)
    parent = property(lambda s: s.counts[:, 3])
    depth = property(lambda s: s.counts[:, 4])
    n_children = property(lambda s: s.counts[:, 5])
    roots = property(lambda s: np.nonzero(s.counts[:, 3] < 0)[0])
    voids = property(lambda s: np.nonzero(s.closed & (s.depth % 2 == 1))[0])
    bodies = property(lambda s: np.nonzero(s.closed & (s.depth % 2 == 0))[0])

    def children(self, p):
        """the patches whose parent is patch p, ascending"""
        return np.nonzero(self.counts[:, 3] == int(p))[0]

    def __len__(self):
        return len(self.counts)


def _nesting_ray(ray):
    if isinstance(ray, bool) or not isinstance(ray, (int, np.integer)) or not 0 <= ray <= 5:
        raise L.R2SError("ray must be 0..5 (+x +y +z -x -y -z)")
    return int(ray)


def mesh_nesting(verts, tris, *, ray=2, rewind=False, index=None, device=-1):
    """Which closed patch of a triangle mesh encloses which patch (verts (nv, 3) float32, tris (nt, 3) int32, 0-based) ->
    MeshNesting.  The patches are those of mesh_orient; no winding is read.  A closed patch Q contains a patch P when the axis ray
    `ray` (0..5: +x +y +z -x -y -z) from P's sample vertex crosses Q an odd number of times, by the exact pair test of
    MeshIndex.winding; the depth of a patch is the number of its containers, its parent the deepest of them.  Closed patches at
    even depth are bodies, at odd depth voids.  rewind=True: `tris` of the result has the voids reversed relative to the input,
    so after mesh_orient(outward=True) bodies are positive and voids negative.  Patches with a boundary or a non-manifold edge
    contain nothing (weld, split and fill first); an irregular patch says that surfaces pass through each other.  index: a
    MeshIndex of the same mesh on the current device, used and left unchanged (the arrays then travel as torch tensors and
    `device` is ignored); None: the library builds a tree, uses it and drops it."""
    ray = _nesting_ray(ray)
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    if index is not None:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        r = mesh_nesting_dev(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), ray=ray, rewind=rewind, index=index)
        return MeshNesting(r.tris.cpu().numpy() if rewind else None, r.patch_of_tri.cpu().numpy(), r.counts, r.pairs.cpu().numpy(), r.totals)
    out, pot = np.empty((len(t), 3), np.int32) if rewind else None, np.empty(len(t), np.int32)
    n, m = ctypes.c_int64(), ctypes.c_int64()
    tot = np.zeros(8, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
    L.check(L.lib().r2s_mesh_nesting(_f(v) if len(v) else None, len(v), ip(t) if len(t) else None, len(t), ray,
                                     L.NESTING_REWIND if rewind else 0, int(device), ip(out) if rewind else None, ip(pot),
                                     ctypes.byref(n), _i(tot)))
    L.check(L.lib().r2s_last_mesh_nesting(None, 0, None, 0, ctypes.byref(n), ctypes.byref(m)))
    counts, pairs = np.empty((n.value, 8), np.int64), np.empty(m.value, np.int64)
    if n.value:
        L.check(L.lib().r2s_last_mesh_nesting(_i(counts), n.value, _i(pairs) if m.value else None, m.value, ctypes.byref(n), ctypes.byref(m)))
    return MeshNesting(out, pot, counts, pairs, tot)


def mesh_nesting_dev(verts, tris, stream=None, *, ray=2, rewind=False, index=None, capacity=0, pair_capacity=0):
    """mesh_nesting on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous).  The records
    and totals come back as numpy arrays; tris (with rewind), patch_of_tri and pairs stay device tensors.  index: a MeshIndex of
    the same mesh on the current device.  The library writes a table only into room for all of it: with more patches than
    `capacity` or more pairs than `pair_capacity` the call is made a second time."""
    import torch
    ray = _nesting_ray(ray)
    _mesh_tensors(verts, tris)
    st = _stream(stream)
    dev = verts.device
    nt = tris.numel() // 3
    out = torch.empty((nt, 3), dtype=torch.int32, device=dev) if rewind else None
    pot = torch.empty(nt, dtype=torch.int32, device=dev)
    n, m = ctypes.c_int64(), ctypes.c_int64()
    tot = np.zeros(8, np.int64)
    cap, pcap = int(capacity), int(pair_capacity)
    vp = ctypes.c_void_p
    h = index._handle() if index is not None else None
    while True:
        counts = torch.empty((cap, 8), dtype=torch.int64, device=dev)
        pairs = torch.empty(pcap, dtype=torch.int64, device=dev)
        L.check(L.lib().r2s_mesh_nesting_dev(h, vp(verts.data_ptr()), verts.numel() // 3, vp(tris.data_ptr()), nt, ray,
                                             L.NESTING_REWIND if rewind else 0, vp(out.data_ptr()) if rewind else None,
                                             vp(pot.data_ptr()), vp(counts.data_ptr()) if cap else None, cap,
                                             vp(pairs.data_ptr()) if pcap else None, pcap, ctypes.byref(n), ctypes.byref(m), _i(tot), st))
        if n.value <= cap and m.value <= pcap:
            break
        cap, pcap = max(cap, n.value), max(pcap, m.value)
    return MeshNesting(out, pot, counts[:n.value].cpu().numpy(), pairs[:m.value], tot)


class MeshFans:
    """The result of mesh_fans (include/rho2sdf_hip.h, r2s_mesh_fans): `fan_of_corner` (nt, 3) int32, the fan of every triangle
    corner (-1 in a collapsed triangle); `fans_of_vert` (nv,) int32 (0 unused, 1 ordinary, >= 2 pinched); `counts` (n, 8) int64
    (vertex, first_corner, n_corners, n_edges, n_boundary, n_flipped, n_nonmanifold, class 0 closed / 1 open / 2 complex);
    `totals` (8,) int64 (fans, triangles, collapsed, used vertices, unused vertices, pinched vertices, complex fans, open
    fans).  With split=True also `verts` (nv_out, 3) float32, `tris` (nt, 3) int32 and `vert_of` (nv_out,) int32 (the source
    vertex of every output vertex), else None.  numpy arrays from mesh_fans; mesh_fans_dev keeps fan_of_corner, fans_of_vert,
    verts, tris and vert_of on the device.  Derived on the host: the masks `closed`, `open`, `complex` per fan, `pinched` (the
    vertex indices with two or more fans) and `vertex_manifold` (no pinched vertex and no complex fan)."""

    def __init__(self, fan_of_corner, fans_of_vert, counts, totals, n_verts_in, verts=None, tris=None, vert_of=None):
        self.fan_of_corner, self.fans_of_vert, self.counts, self.totals = fan_of_corner, fans_of_vert, counts, totals
        self.verts, self.tris, self.vert_of, self._nv = verts, tris, vert_of, int(n_verts_in)

    n_fans = property(lambda s: len(s.counts))
    n_added = property(lambda s: int(s.totals[0] - s.totals[3]))
    n_verts_out = property(lambda s: s._nv + s.n_added)
    vertex = property(lambda s: s.counts[:, 0])
    first_corner = property(lambda s: s.counts[:, 1])
    n_corners = property(lambda s: s.counts[:, 2])
    closed = property(lambda s: s.counts[:, 7] == 0)
    open = property(lambda s: s.counts[:, 7] == 1)
    complex = property(lambda s: s.counts[:, 7] == 2)
    vertex_manifold = property(lambda s: bool(s.totals[5] == 0 and s.totals[6] == 0))

    @property
    def pinched(self):
        v = self.counts[:, 0]
        return np.unique(v[1:][v[1:] == v[:-1]])

    def __len__(self):
        return len(self.counts)


def mesh_fans(verts, tris, *, split=False, device=-1):
    """The fans of a triangle mesh (verts (nv, 3) float32, tris (nt, 3) int32, 0-based) -> MeshFans: the corners of every vertex
    fall into fans, connected over the edges their triangles share at that vertex; a vertex with two or more fans is PINCHED
    (non-manifold although every edge may be regular: two bodies touching in a point, a welded iso-surface through a lattice
    point), which mesh_shells cannot see.  split=True also returns the repaired mesh: the first fan of a vertex keeps its index,
    every further fan gets a copy of the vertex appended behind the input vertices, in fan order; no coordinate, edge or winding
    changes.  Fans on a non-manifold edge (complex) are reported, not repaired.  One library call (a second one when the split
    needs more than a little room) and a copy of the thread's last records."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    foc, fov = np.empty((len(t), 3), np.int32), np.empty(len(v), np.int32)
    n, nvo = ctypes.c_int64(), ctypes.c_int64()
    tot = np.zeros(8, np.int64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)
    cap = len(v) + 1024 if split else 0
    while True:
        to, vo, vof = np.empty((len(t), 3), np.int32), np.empty((max(cap, 1), 3), np.float32), np.empty(max(cap, 1), np.int32)
        L.check(L.lib().r2s_mesh_fans(_f(v) if len(v) else None, len(v), ip(t) if len(t) else None, len(t), int(device), ip(foc), ip(fov),
                                      ip(to) if split else None, _f(vo) if split else None, ip(vof) if split else None, cap,
                                      ctypes.byref(n), ctypes.byref(nvo), _i(tot)))
        if not split or nvo.value <= cap:
            break
        cap = nvo.value
    counts = np.empty((n.value, 8), np.int64)
    if n.value:
        L.check(L.lib().r2s_last_mesh_fans(_i(counts), n.value, ctypes.byref(n)))
    if not split:
        return MeshFans(foc, fov, counts, tot, len(v))
    return MeshFans(foc, fov, counts, tot, len(v), vo[:nvo.value].copy(), to, vof[:nvo.value].copy())


def mesh_fans_dev(verts, tris, stream=None, *, split=False, capacity=0):
    """mesh_fans on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous).  The records come
    back as a numpy array; fan_of_corner, fans_of_vert and, with split=True, verts, tris and vert_of stay device tensors.  The
    library writes the records only into room for all fans and the split only into room for all output vertices: with more fans
    than `capacity`, or a split that needs more than a little room, the call is made a second time."""
    import torch
    _mesh_tensors(verts, tris)
    st = _stream(stream)
    dev = verts.device
    nv, nt = verts.numel() // 3, tris.numel() // 3
    foc, fov = torch.empty((nt, 3), dtype=torch.int32, device=dev), torch.empty(nv, dtype=torch.int32, device=dev)
    n, nvo = ctypes.c_int64(), ctypes.c_int64()
    tot = np.zeros(8, np.int64)
    cap, vcap = int(capacity), (nv + 1024 if split else 0)
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x.numel() else None   # noqa: E731
    while True:
        counts = torch.empty((cap, 8), dtype=torch.int64, device=dev)
        to = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        vo, vof = torch.empty((max(vcap, 1), 3), dtype=torch.float32, device=dev), torch.empty(max(vcap, 1), dtype=torch.int32, device=dev)
        L.check(L.lib().r2s_mesh_fans_dev(vp(verts), nv, vp(tris), nt, vp(foc), vp(fov), vp(counts), cap, vp(to) if split else None,
                                          vp(vo) if split else None, vp(vof) if split else None, vcap, ctypes.byref(n), ctypes.byref(nvo),
                                          _i(tot), st))
        if n.value <= cap and (not split or nvo.value <= vcap):
            break
        cap, vcap = max(cap, n.value), (max(vcap, nvo.value) if split else 0)
    counts = counts[:n.value].cpu().numpy()
    if not split:
        return MeshFans(foc, fov, counts, tot, nv)
    return MeshFans(foc, fov, counts, tot, nv, vo[:nvo.value], to, vof[:nvo.value])


class MeshHoles:
    """The result of mesh_holes (include/rho2sdf_hip.h, r2s_mesh_holes): the RIMS of a mesh, the connected components of its
    boundary half-edges.  `rim_start` (n + 1,) int64, `rim_edge` (m,) int32 (the half-edge id 3 t + c of every output position:
    it runs from tris[t, c] to tris[t, (c + 1) % 3]; a closed rim is listed along its cycle from its smallest half-edge, any
    other rim in ascending id), `counts` (n, 8) int64 (first half-edge, n_edges, n_nodes, open, flipped, branch nodes, status
    0 not closed / 1 closed / 2 filled with one triangle / 3 filled with a fan, added vertex or -1), `sums` (n, 7) float64
    (length, sum A x B, sum A about `ref_point`), `ref_point` (3,), `totals` (8,) int64 (rims, boundary half-edges, collapsed
    triangles, nodes, open + flipped + branch nodes, closed rims, filled rims, added triangles).  With a fill also `verts`
    (nv_out, 3) float32 and `tris` (nt_out, 3) int32, else None.  numpy arrays from mesh_holes; mesh_holes_dev keeps rim_edge,
    verts and tris on the device.  Derived on the host: `closed`, `filled` masks, `length`, `area` (0.5 |sum A x B|, the area of
    a closed rim's vector-area projection), `centroid` (ref_point + sum A / n_edges, the mean of a rim's FROM vertices) and
    `watertight` (no boundary half-edge at all)."""

    def __init__(self, rim_start, rim_edge, counts, sums, ref_point, totals, verts=None, tris=None):
        self.rim_start, self.rim_edge, self.counts, self.sums = rim_start, rim_edge, counts, sums
        self.ref_point, self.totals, self.verts, self.tris = ref_point, totals, verts, tris

    n_rims = property(lambda s: len(s.counts))
    first_edge = property(lambda s: s.counts[:, 0])
    n_edges = property(lambda s: s.counts[:, 1])
    closed = property(lambda s: s.counts[:, 6] >= 1)
    filled = property(lambda s: s.counts[:, 6] >= 2)
    length = property(lambda s: s.sums[:, 0])
    area = property(lambda s: 0.5 * np.sqrt((s.sums[:, 1:4] ** 2).sum(-1)))
    centroid = property(lambda s: s.ref_point[None, :] + s.sums[:, 4:7] / np.maximum(s.counts[:, 1:2], 1))
    watertight = property(lambda s: bool(s.totals[1] == 0))

    def __len__(self):
        return len(self.counts)


def mesh_holes(verts, tris, *, fill=None, device=-1):
    """The rims (boundary loops and chains) of a triangle mesh (verts (nv, 3) float32, tris (nt, 3) int32, 0-based) -> MeshHoles.
    A boundary half-edge is alone on its undirected edge; a rim is a connected component of them, CLOSED when every vertex on
    it has one incoming and one outgoing boundary half-edge (then it is one simple loop: a hole).  fill=None reports only;
    fill=-1 caps every closed rim, fill=k > 0 those of at most k edges, fill=0 none (the mesh is copied): a rim of three gets
    one triangle, a longer one a new vertex at the mean of its vertices and a fan of n_edges triangles, wound against the
    boundary so that every filled edge becomes a regular edge.  Rims that are not closed (a pinched boundary vertex, flipped
    neighbours, a fin) are never filled: weld -> orient -> mesh_fans(split=True) first.  A fan cap of a rim that is far from
    planar or not star-shaped can pass through the surface; mesh_intersections is the check."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    nr, nb, nvo, nto = (ctypes.c_int64() for _ in range(4))
    tot, r = np.zeros(8, np.int64), np.zeros(3, np.float64)
    ip = lambda a: a.ctypes.data_as(L.c_int32_p)   # noqa: E731
    do_fill = fill is not None
    vcap, tcap = (len(v) + 1024, len(t) + 4096) if do_fill else (0, 0)
    while True:
        vo, to = np.empty((max(vcap, 1), 3), np.float32), np.empty((max(tcap, 1), 3), np.int32)
        L.check(L.lib().r2s_mesh_holes(_f(v) if len(v) else None, len(v), ip(t) if len(t) else None, len(t), int(device),
                                       int(fill) if do_fill else 0, ip(to) if do_fill else None, _f(vo) if do_fill else None, vcap, tcap,
                                       ctypes.byref(nr), ctypes.byref(nb), ctypes.byref(nvo), ctypes.byref(nto), _d(r), _i(tot)))
        if not do_fill or (nvo.value <= vcap and nto.value <= tcap):
            break
        vcap, tcap = max(vcap, nvo.value), max(tcap, nto.value)
    start, counts, sums = np.zeros(nr.value + 1, np.int64), np.empty((nr.value, 8), np.int64), np.empty((nr.value, 7), np.float64)
    edge = np.empty(nb.value, np.int32)
    if nr.value:
        L.check(L.lib().r2s_last_mesh_holes(_i(start), _i(counts), _d(sums), nr.value, ip(edge), nb.value, ctypes.byref(nr), ctypes.byref(nb)))
    if not do_fill:
        return MeshHoles(start, edge, counts, sums, r, tot)
    return MeshHoles(start, edge, counts, sums, r, tot, vo[:nvo.value].copy(), to[:nto.value].copy())


def mesh_holes_dev(verts, tris, stream=None, *, fill=None, capacity=0, edge_capacity=0):
    """mesh_holes on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous).  rim_start,
    the records and the sums come back as numpy arrays; rim_edge and, with a fill, verts and tris stay device tensors.  The
    library writes each group only into room for all of it: with more rims than `capacity`, more boundary half-edges than
    `edge_capacity` or a fill that needs more than a little room, the call is made a second time."""
    import torch
    _mesh_tensors(verts, tris)
    st = _stream(stream)
    dev = verts.device
    nv, nt = verts.numel() // 3, tris.numel() // 3
    nr, nb, nvo, nto = (ctypes.c_int64() for _ in range(4))
    tot, r = np.zeros(8, np.int64), np.zeros(3, np.float64)
    do_fill = fill is not None
    cap, ecap = int(capacity), int(edge_capacity)
    vcap, tcap = (nv + 1024, nt + 4096) if do_fill else (0, 0)
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x.numel() else None   # noqa: E731
    while True:
        start = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        counts = torch.empty((cap, 8), dtype=torch.int64, device=dev)
        sums = torch.empty((cap, 7), dtype=torch.float64, device=dev)
        edge = torch.empty(ecap, dtype=torch.int32, device=dev)
        vo = torch.empty((max(vcap, 1), 3), dtype=torch.float32, device=dev)
        to = torch.empty((max(tcap, 1), 3), dtype=torch.int32, device=dev)
        L.check(L.lib().r2s_mesh_holes_dev(vp(verts), nv, vp(tris), nt, int(fill) if do_fill else 0, vp(start) if cap else None, vp(counts),
                                           vp(sums), cap, vp(edge), ecap, vp(to) if do_fill else None, vp(vo) if do_fill else None, vcap,
                                           tcap, ctypes.byref(nr), ctypes.byref(nb), ctypes.byref(nvo), ctypes.byref(nto), _d(r), _i(tot), st))
        if nr.value <= cap and nb.value <= ecap and (not do_fill or (nvo.value <= vcap and nto.value <= tcap)):
            break
        cap, ecap = max(cap, nr.value), max(ecap, nb.value)
        if do_fill:
            vcap, tcap = max(vcap, nvo.value), max(tcap, nto.value)
    out = (start[:nr.value + 1].cpu().numpy(), edge[:nb.value], counts[:nr.value].cpu().numpy(), sums[:nr.value].cpu().numpy(), r, tot)
    if not do_fill:
        return MeshHoles(*out)
    return MeshHoles(*out, vo[:nvo.value], to[:nto.value])


class MeshSections:
    """The plane sections of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_sections): the raw tables and what follows from
    them.  Raw: `normal` (3,), `levels` (n_levels,), `contour_start` (n + 1,) int64, `counts` (n, 8) int64 (level, first segment id,
    n_segs, n_nodes, open, flipped, branch, 0), `sums` (n, 7) float64 (length, the area vector C, the first moments about
    `ref_point`), `ref_point` (3,), `totals` (8,) int64 (contours, segments, collapsed triangles, nodes, open, flipped, branch,
    closed contours), and per output position `seg_tri` (m,) int32 and `seg_points` (m, 2, 3) float64 (from, to); device tensors
    from mesh_sections_dev keep the two segment tables on the device.  Derived per contour, in float64 numpy:
        closed   = (open == 0) & (flipped == 0) & (branch == 0)
        area     = 0.5 * (normal . C) / |normal|, signed: negative for a hole; is_hole = closed & (area < 0)
        length   = sums[:, 0]
        centroid = ref_point + M / (3 * normal . C), moved along the normal onto the plane of its level; NaN unless closed with
                   a non-zero area                                      M = sums[:, 4:7]
    and per level (n_levels,): level_n_contours, level_area (the closed contours, holes subtracting), level_perimeter (all
    contours) and level_centroid (the closed contours together; NaN without area)."""

    def __init__(self, normal, levels, contour_start, counts, sums, ref_point, totals, seg_tri, seg_points):
        self.normal, self.levels = np.asarray(normal, np.float64).reshape(3), np.asarray(levels, np.float64).reshape(-1)
        self.contour_start, self.counts, self.sums, self.ref_point, self.totals = contour_start, counts, sums, ref_point, totals
        self.seg_tri, self.seg_points = seg_tri, seg_points

    n_contours = property(lambda s: len(s.counts))
    n_segments = property(lambda s: int(s.totals[1]))
    level = property(lambda s: s.counts[:, 0])
    first_seg = property(lambda s: s.counts[:, 1])
    n_segs = property(lambda s: s.counts[:, 2])
    n_nodes = property(lambda s: s.counts[:, 3])
    n_open = property(lambda s: s.counts[:, 4])
    n_flipped = property(lambda s: s.counts[:, 5])
    n_branch = property(lambda s: s.counts[:, 6])
    closed = property(lambda s: (s.n_open == 0) & (s.n_flipped == 0) & (s.n_branch == 0))
    length = property(lambda s: s.sums[:, 0])
    area = property(lambda s: 0.5 * (s.sums[:, 1:4] @ s.normal) / np.sqrt(s.normal @ s.normal))
    is_hole = property(lambda s: s.closed & (s.area < 0))

    def __len__(self):
        return len(self.counts)

    def _on_plane(self, W, M, c):
        """ref_point + M / (3 W) moved along the normal to height c (W = normal . sum C; NaN where W is 0)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            g = self.ref_point[None, :] + M / (3.0 * np.where(W != 0, W, np.nan))[:, None]
        return g + ((c - g @ self.normal) / (self.normal @ self.normal))[:, None] * self.normal[None, :]

    @property
    def centroid(self):
        W = np.where(self.closed, self.sums[:, 1:4] @ self.normal, 0.0)
        return self._on_plane(W, self.sums[:, 4:7], self.levels[self.level])

    def _per_level(self, values, mask=None):
        out = np.zeros((len(self.levels),) + values.shape[1:])
        k = self.level if mask is None else self.level[mask]
        np.add.at(out, k, values if mask is None else values[mask])
        return out

    level_n_contours = property(lambda s: np.bincount(s.level, minlength=len(s.levels)))
    level_area = property(lambda s: s._per_level(s.area, s.closed))
    level_perimeter = property(lambda s: s._per_level(s.length))

    @property
    def level_centroid(self):
        W = self._per_level(self.sums[:, 1:4] @ self.normal, self.closed)
        return self._on_plane(W, self._per_level(self.sums[:, 4:7], self.closed), self.levels)

    def loops(self, level):
        """the closed contours of level index `level`, in contour order: a list of (m, 3) float64 arrays, the FROM points of
        the m segments in walking order (the loop closes from the last point back to the first); material is on the left
        seen from the tip of the normal, so outer loops run counter-clockwise and holes clockwise"""
        pts = self.seg_points
        pts = np.asarray(pts.cpu() if hasattr(pts, "cpu") else pts)
        return [pts[self.contour_start[c]:self.contour_start[c + 1], 0].copy()
                for c in np.nonzero((self.level == int(level)) & self.closed)[0]]


def _section_inputs(normal, levels):
    nrm = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1)
    lev = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    if nrm.shape != (3,):
        raise L.R2SError("normal must have three components")
    return nrm, lev


def mesh_sections(verts, tris, normal, levels, *, device=-1):
    """The sections of a triangle mesh (verts (nv, 3) float32, tris (nt, 3) int32, 0-based) with the planes normal . x = levels[k]
    (normal (3,), not normalised; levels ascending): per level the contours, their node classes, lengths, areas and first moments,
    and every segment in output order -> MeshSections (its docstring has the fields and the formulas of the derived ones).  One
    library call and a copy of the thread's last tables."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    nrm, lev = _section_inputs(normal, levels)
    nc, ns = ctypes.c_int64(), ctypes.c_int64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    L.check(L.lib().r2s_mesh_sections(_f(v) if len(v) else None, len(v), t.ctypes.data_as(L.c_int32_p) if len(t) else None, len(t),
                                      _d(nrm), _d(lev) if len(lev) else None, len(lev), int(device), ctypes.byref(nc), ctypes.byref(ns),
                                      _d(ref), _i(tot)))
    start, counts, sums = np.zeros(nc.value + 1, np.int64), np.empty((nc.value, 8), np.int64), np.empty((nc.value, 7))
    seg_tri, pts = np.empty(ns.value, np.int32), np.empty((ns.value, 2, 3))
    if nc.value:
        L.check(L.lib().r2s_last_mesh_sections(_i(start), _i(counts), _d(sums), nc.value, seg_tri.ctypes.data_as(L.c_int32_p), _d(pts),
                                               ns.value, ctypes.byref(nc), ctypes.byref(ns)))
    return MeshSections(nrm, lev, start, counts, sums, ref, tot, seg_tri, pts)


def mesh_sections_dev(verts, tris, normal, levels, stream=None, *, contour_capacity=0, segment_capacity=0):
    """mesh_sections on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous; normal and
    levels are host values).  The contour tables come back as numpy arrays, seg_tri and seg_points stay device tensors.  The
    library writes the tables only into room for all contours and segments: with more of either than the capacities the call
    is made a second time."""
    import torch
    _mesh_tensors(verts, tris)
    nrm, lev = _section_inputs(normal, levels)
    st = _stream(stream)
    nc, ns = ctypes.c_int64(), ctypes.c_int64()
    ref, tot = np.zeros(3), np.zeros(8, np.int64)
    ccap, scap = int(contour_capacity), int(segment_capacity)
    vp = ctypes.c_void_p
    dev = verts.device
    while True:
        start = torch.zeros(ccap + 1, dtype=torch.int64, device=dev)
        counts = torch.empty((ccap, 8), dtype=torch.int64, device=dev)
        sums = torch.empty((ccap, 7), dtype=torch.float64, device=dev)
        seg_tri = torch.empty(scap, dtype=torch.int32, device=dev)
        pts = torch.empty((scap, 2, 3), dtype=torch.float64, device=dev)
        L.check(L.lib().r2s_mesh_sections_dev(
            vp(verts.data_ptr()), verts.numel() // 3, vp(tris.data_ptr()), tris.numel() // 3, _d(nrm), _d(lev) if len(lev) else None,
            len(lev), vp(start.data_ptr()) if ccap else None, vp(counts.data_ptr()) if ccap else None,
            vp(sums.data_ptr()) if ccap else None, ccap, vp(seg_tri.data_ptr()) if scap else None, vp(pts.data_ptr()) if scap else None,
            scap, ctypes.byref(nc), ctypes.byref(ns), _d(ref), _i(tot), st))
        if nc.value <= ccap and ns.value <= scap:
            break
        ccap, scap = max(ccap, nc.value), max(scap, ns.value)
    return MeshSections(nrm, lev, start[:nc.value + 1].cpu().numpy(), counts[:nc.value].cpu().numpy(), sums[:nc.value].cpu().numpy(),
                        ref, tot, seg_tri[:ns.value], pts[:ns.value])


def vertex_normals(verts, tris):
    """area-weighted vertex normals of the winding, float64 (nv, 3), not normalised: the sum of (b-a)x(c-a) over the
    triangles at a vertex, from the float32 vertices widened to float64, added in the order of the triangles (corner 0 of
    every triangle first, then corner 1, then corner 2)"""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    ab, ac = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    fn = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                   ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, t[:, k], fn)
    return n


def _unit(n):
    """n / |n| in float64, |n| = sqrt((x*x + y*y) + z*z); a zero normal stays zero (its ray then answers NaN)"""
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n / np.where(ln > 0.0, ln, 1.0)[:, None]


def _skip(skip):
    skip = float(skip)
    if not (skip >= 0.0) or skip == float("inf"):
        raise L.R2SError("skip must be a finite length >= 0")
    return skip


def surface_thickness(verts, tris, normals=None, *, skip, index=None, device=-1):
    """Wall thickness at every vertex of a surface: the first hit of the ray from the vertex along -normal with t >= skip
    -> (thickness (nv,) float64, hit_tri (nv,) int32, side (nv,) int8) as MeshIndex.raycast returns them.  `normals`
    (nv, 3): any vectors along which to measure, e.g. RbfField.normals(verts); default: vertex_normals(verts, tris).  They
    are normalised in float64, so the thickness is a length.  `skip` is a length of the caller's choosing (typically a
    fraction of the lattice spacing) that steps over the triangles at the vertex itself.  A ray that leaves the mesh gives
    inf / -1 / 0, a vertex with a zero or non-finite normal NaN / -1 / 0.  `index`: a MeshIndex of (verts, tris) to use
    instead of building one."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    skip = _skip(skip)
    n = vertex_normals(v, t) if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    if n.shape != v.shape:
        raise L.R2SError("normals must be (n_verts, 3)")
    d = -_unit(n)
    if index is not None:
        return index.raycast(v.astype(np.float64), d, t_min=skip, want_index=True, want_side=True)
    with MeshIndex(v, t, device=device) as ix:
        return ix.raycast(v.astype(np.float64), d, t_min=skip, want_index=True, want_side=True)


def surface_thickness_dev(verts, tris, normals=None, *, skip, index=None, stream=None):
    """surface_thickness on torch tensors on the current device (verts float32 (nv, 3), tris int32 (nt, 3), contiguous;
    normals float64 or float32 (nv, 3)) -> device tensors (thickness float64, hit_tri int32, side int8).  The default
    normals are summed per vertex in the order of vertex_normals (one conflict-free scatter per incident corner, no
    floating-point atomics), so the result equals surface_thickness."""
    import torch
    _mesh_tensors(verts, tris)
    skip = _skip(skip)
    v = verts.reshape(-1, 3).to(torch.float64)
    nv = v.shape[0]
    if normals is None:
        t = tris.reshape(-1, 3).to(torch.int64)
        ab, ac = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        fn = torch.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                          ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], dim=1)
        n = torch.zeros_like(v)
        if t.numel():
            corner = torch.cat([t[:, 0], t[:, 1], t[:, 2]])
            vs, order = torch.sort(corner, stable=True)
            first = torch.searchsorted(vs, vs)                       # position of the vertex's first corner
            rank = torch.arange(len(vs), device=vs.device) - first
            src = order % t.shape[0]                                 # the triangle of each corner
            for r in range(int(rank.max().item()) + 1):
                sel = rank == r
                n[vs[sel]] = n[vs[sel]] + fn[src[sel]]
    else:
        n = normals.to(torch.float64)
        if n.shape != v.shape or n.device != v.device:
            raise L.R2SError("normals must be (n_verts, 3) on the device of verts")
    ln = torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    d = (-(n / torch.where(ln > 0.0, ln, torch.ones_like(ln))[:, None])).contiguous()
    own = index is None
    ix = MeshIndex(verts, tris) if own else index
    try:
        out = ix.raycast_dev(v.contiguous(), d, t_min=skip, want_index=True, want_side=True, stream=stream)
        if own:
            (torch.cuda.current_stream() if stream is None else stream).synchronize()   # the index goes away below
        return out
    finally:
        if own:
            ix.close()


def redistance_full(values, grid, smooth=None, *, iso=0.0, device=-1):
    """The signed distance to the iso-surface of `values` on the whole lattice (include/rho2sdf_hip.h, r2s_redistance_full):
    s * d with s and the mesh as in redistance and no band; +-inf where the field has no surface.  The result has the shape
    (nz, ny, nx) and the type of the (float32 / float64) input; `grid` is a Grid (with `smooth`) or an explicit (dims, origin,
    spacing), as in mesh_distance."""
    a = np.ascontiguousarray(values)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    dims, origin, spacing = _dist_lattice(grid, smooth)
    if a.size != dims[0] * dims[1] * dims[2]:
        raise L.R2SError(f"values length ({a.size}) doesn't match the lattice {tuple(dims)}")
    out = np.empty((dims[2], dims[1], dims[0]), a.dtype)
    L.check(L.lib().r2s_redistance_full(a.ctypes.data_as(ctypes.c_void_p), int(a.dtype == np.float32), dims, origin, spacing,
                                        float(iso), int(device), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def redistance_full_dev(t, grid, smooth=None, *, iso=0.0, stream=None):
    """redistance_full on a torch tensor on the current device (float32 / float64, contiguous, x fastest) -> a device tensor"""
    import torch
    if t.dtype not in (torch.float32, torch.float64) or not t.is_contiguous() or not t.is_cuda:
        raise L.R2SError("t must be a contiguous float32 / float64 device tensor")
    dims, origin, spacing = _dist_lattice(grid, smooth)
    if t.numel() != dims[0] * dims[1] * dims[2]:
        raise L.R2SError(f"values length ({t.numel()}) doesn't match the lattice {tuple(dims)}")
    out = torch.empty((dims[2], dims[1], dims[0]), dtype=t.dtype, device=t.device)
    st = _stream(stream)
    L.check(L.lib().r2s_redistance_full_dev(ctypes.c_void_p(t.data_ptr()), int(t.dtype == torch.float32), dims, origin, spacing,
                                            float(iso), ctypes.c_void_p(out.data_ptr()), st))
    return out


def _deviation_stats(d):
    if d.size == 0:
        return dict(max=0.0, mean=0.0, rms=0.0, argmax=-1)
    return dict(max=float(d.max()), mean=float(d.mean()), rms=float(np.sqrt(np.mean(d * d))), argmax=int(d.argmax()))


def surface_deviation(verts_a, tris_a, verts_b, tris_b, *, device=-1):
    """How far two surfaces are apart, sampled at their vertices -> {"a_to_b": {max, mean, rms, argmax}, "b_to_a": {...},
    "hausdorff": float}: a_to_b describes the exact distances from the vertices of A to the surface B (argmax = the vertex
    of A that is farthest, -1 without vertices), b_to_a the reverse.  `hausdorff` is the larger of the two maxima; it is
    vertex-sampled, hence a LOWER bound of the true Hausdorff distance of the two surfaces (the farthest point of a triangle
    need not be a vertex).  A surface without triangles is at distance inf."""
    va = np.ascontiguousarray(verts_a, dtype=np.float32).reshape(-1, 3)
    vb = np.ascontiguousarray(verts_b, dtype=np.float32).reshape(-1, 3)
    with MeshIndex(vb, tris_b, device=device) as ib:
        a_to_b = _deviation_stats(ib.distance(va))
    with MeshIndex(va, tris_a, device=device) as ia:
        b_to_a = _deviation_stats(ia.distance(vb))
    return dict(a_to_b=a_to_b, b_to_a=b_to_a, hausdorff=max(a_to_b["max"], b_to_a["max"]))


class RbfField:
    """The smoothed level-set of one RBFs_smoothing as a function (include/rho2sdf_hip.h, r2s_rbf_field): the weights and
    the level shift stay on the device; `eval`, `normals`, `curvature` and `project` take any (n, 3) array of points.  A context manager;
    `close()` frees the device memory.  Build one with fit_rbf_field, or from given weights ((nz, ny, nx) float32)."""

    def __init__(self, weights, grid, level_shift=0.0, threshold=1e-3, *, device=-1, _handle=None):
        self.grid, self.threshold, self.cg_iterations = grid, float(threshold), None
        if _handle is not None:
            self._h = _handle
            return
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.size != grid.ngp:
            raise L.R2SError(f"weights length ({w.size}) doesn't match the grid ({grid.ngp})")
        h = ctypes.c_void_p()
        L.check(L.lib().r2s_rbf_field_from_weights(_f(w), ctypes.byref(grid.c), float(threshold), float(level_shift), int(device),
                                                   ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            L.lib().r2s_rbf_field_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the loader's globals may be gone already
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _handle(self):
        if not self._h:
            raise L.R2SError("the field is closed")
        return self._h

    @property
    def weights(self):
        w = np.empty(self.grid.ngp, dtype=np.float32)
        L.check(L.lib().r2s_rbf_field_weights(self._handle(), _f(w), None))
        return w.reshape(self.grid.dims[2], self.grid.dims[1], self.grid.dims[0])

    @property
    def level_shift(self):
        th = ctypes.c_float()
        L.check(L.lib().r2s_rbf_field_weights(self._handle(), None, ctypes.byref(th)))
        return np.float32(th.value)

    @staticmethod
    def _points(points):
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise L.R2SError("points must be (n, 3)")
        return p

    def eval(self, points, grad=False, hess=False, taps=False):
        """f(points) incl. the level shift -> val (n,) float32; grad=True: (val, grad (n, 3)); hess=True: (val, grad, hess
        (n, 6) = xx, yy, zz, xy, xz, yz), the gradient included; taps=True: the number of nodes that took part is appended
        (negative where the knn cap bound)"""
        p = self._points(points)
        n = len(p)
        grad = grad or hess
        val = np.empty(n, np.float32)
        g = np.empty((n, 3), np.float32) if grad else None
        h = np.empty((n, 6), np.float32) if hess else None
        t = np.empty(n, np.int32) if taps else None
        tp = t.ctypes.data_as(L.c_int32_p) if taps else None
        if hess:
            L.check(L.lib().r2s_rbf_field_hessian(self._handle(), _f(p), n, _f(val), _f(g), _f(h), tp))
        else:
            L.check(L.lib().r2s_rbf_field_eval(self._handle(), _f(p), n, _f(val), _f(g) if grad else None, tp))
        out = (val,) + ((g,) if grad else ()) + ((h,) if hess else ()) + ((t,) if taps else ())
        return out[0] if len(out) == 1 else out

    def curvature(self, points):
        """curvatures of the level set of f through each point, oriented by the outward normal -grad f / |grad f| (a convex
        solid has positive mean curvature) -> (mean, gauss, k1, k2), (n,) float32 each, k1 >= k2; NaN where the gradient
        vanishes or is not finite"""
        p = self._points(points)
        c = np.empty((len(p), 4), np.float32)
        L.check(L.lib().r2s_rbf_field_curvature(self._handle(), _f(p), len(p), _f(c), None, None))
        return tuple(np.ascontiguousarray(c[:, k]) for k in range(4))

    def normals(self, points):
        """outward unit normals -grad f / |grad f| -> (n, 3) float32; (0,0,0) where the gradient vanishes or is not finite"""
        p = self._points(points)
        nv = np.empty((len(p), 3), np.float32)
        L.check(L.lib().r2s_rbf_field_normals(self._handle(), _f(p), len(p), _f(nv)))
        return nv

    def project(self, points, max_iter=8, tol=None):
        """points moved onto {f = 0} along the gradient (header: the step rule) -> (points (n, 3), status (n,) int32, resid
        (n,) float32, iters (n,) int32); tol defaults to 1e-4 * cell_size.  status 0 = converged, 1 = iteration cap,
        2 = vanishing gradient, 3 = non-finite input"""
        p = self._points(points).copy()
        n = len(p)
        tol = np.float32(1e-4 * self.grid.cell_size) if tol is None else np.float32(tol)
        status, resid, iters = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.int32)
        L.check(L.lib().r2s_rbf_field_project(self._handle(), _f(p), n, int(max_iter), float(tol), status.ctypes.data_as(L.c_int32_p),
                                              _f(resid), iters.ctypes.data_as(L.c_int32_p)))
        return p, status, resid, iters

    # ---- torch tensors on the field's device (contiguous float32 (n, 3)); enqueued on the current stream ----
    @staticmethod
    def _dev_points(t):   # (the library checks that the current device is the field's)
        import torch
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.dim() != 2 or t.shape[1] != 3:
            raise L.R2SError("points must be a contiguous float32 (n, 3) device tensor")
        if t.device.index != torch.cuda.current_device():
            raise L.R2SError(f"points live on {t.device}, the current device is cuda:{torch.cuda.current_device()}")
        return ctypes.c_void_p(t.data_ptr()), _stream(None)

    def eval_dev(self, t, grad=False, taps=False):
        import torch
        p, st = self._dev_points(t)
        n = t.shape[0]
        val = torch.empty(n, dtype=torch.float32, device=t.device)
        g = torch.empty((n, 3), dtype=torch.float32, device=t.device) if grad else None
        k = torch.empty(n, dtype=torch.int32, device=t.device) if taps else None
        ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and n else None   # noqa: E731
        L.check(L.lib().r2s_rbf_field_eval_dev(self._handle(), p, n, ptr(val), ptr(g), ptr(k), st))
        out = (val,) + ((g,) if grad else ()) + ((k,) if taps else ())
        return out[0] if len(out) == 1 else out

    def hessian_dev(self, t, taps=False):
        """-> (val (n,), grad (n, 3), hess (n, 6)) float32 tensors; taps=True appends the int32 tap counts"""
        import torch
        p, st = self._dev_points(t)
        n = t.shape[0]
        val = torch.empty(n, dtype=torch.float32, device=t.device)
        g = torch.empty((n, 3), dtype=torch.float32, device=t.device)
        h = torch.empty((n, 6), dtype=torch.float32, device=t.device)
        k = torch.empty(n, dtype=torch.int32, device=t.device) if taps else None
        ptr = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None and n else None   # noqa: E731
        L.check(L.lib().r2s_rbf_field_hessian_dev(self._handle(), p, n, ptr(val), ptr(g), ptr(h), ptr(k), st))
        return (val, g, h) + ((k,) if taps else ())

    def curvature_dev(self, t):
        """-> (n, 4) float32 tensor: mean, gauss, k1, k2"""
        import torch
        p, st = self._dev_points(t)
        n = t.shape[0]
        c = torch.empty((n, 4), dtype=torch.float32, device=t.device)
        if n:
            L.check(L.lib().r2s_rbf_field_curvature_dev(self._handle(), p, n, ctypes.c_void_p(c.data_ptr()), None, None, st))
        return c

    def normals_dev(self, t):
        import torch
        p, st = self._dev_points(t)
        nv = torch.empty_like(t)
        if t.shape[0]:
            L.check(L.lib().r2s_rbf_field_normals_dev(self._handle(), p, t.shape[0], ctypes.c_void_p(nv.data_ptr()), st))
        return nv

    def project_dev(self, t, max_iter=8, tol=None):
        import torch
        out = t.clone()
        p, st = self._dev_points(out)
        n = out.shape[0]
        tol = np.float32(1e-4 * self.grid.cell_size) if tol is None else np.float32(tol)
        status = torch.empty(n, dtype=torch.int32, device=t.device)
        resid = torch.empty(n, dtype=torch.float32, device=t.device)
        iters = torch.empty(n, dtype=torch.int32, device=t.device)
        if n:
            L.check(L.lib().r2s_rbf_field_project_dev(self._handle(), p, n, int(max_iter), float(tol),
                                                      ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(resid.data_ptr()),
                                                      ctypes.c_void_p(iters.data_ptr()), st))
        return out, status, resid, iters


def fit_rbf_field(sdf, grid, Is_interpolation, target_volume, threshold=1e-3, *, device=-1):
    """The function RBFs_smoothing samples: process_vector, the weights and the volume-preserving level shift of
    r2s_rbf_smooth for the same input, kept on the device -> RbfField (`.cg_iterations` is set)"""
    sdf = np.ascontiguousarray(sdf, dtype=np.float64)
    if sdf.size != grid.ngp:
        raise L.R2SError(f"sdf length ({sdf.size}) doesn't match the grid ({grid.ngp})")
    h, th, its = ctypes.c_void_p(), ctypes.c_float(), ctypes.c_int32()
    L.check(L.lib().r2s_rbf_field_fit(_d(sdf), ctypes.byref(grid.c), int(bool(Is_interpolation)), float(threshold),
                                      float(target_volume), int(device), ctypes.byref(h), ctypes.byref(th), ctypes.byref(its)))
    f = RbfField(None, grid, threshold=threshold, _handle=h)
    f.cg_iterations = int(its.value)
    return f


def refine_surface(field, verts, max_iter=8, tol=None):
    """vertices of extract_isosurface moved onto the zero level of the function they sample, with the outward unit normals
    there -> (verts (n, 3) float32, normals (n, 3) float32, status (n,) int32); the triangle list stays valid"""
    p, status, _, _ = field.project(verts, max_iter=max_iter, tol=tol)
    return p, field.normals(p), status


def surface_curvature(field, verts):
    """Curvature of the smoothed surface at given vertices, typically those of refine_surface(field, verts) -> {"mean",
    "gauss", "k1", "k2": (n,) float32 (RbfField.curvature); "min_radius": (n,) float64, 1 / max(|k1|, |k2|), the smallest
    radius of curvature (inf where both are 0, NaN where the curvature is NaN); "n_undefined": vertices with NaN curvature;
    "min_radius_p01", "min_radius_p50": the 1 % and 50 % quantiles of min_radius over its finite entries (NaN without any)}"""
    mean, gauss, k1, k2 = field.curvature(verts)
    kmax = np.maximum(np.abs(k1), np.abs(k2)).astype(np.float64)
    with np.errstate(divide="ignore"):
        radius = 1.0 / kmax
    fin = radius[np.isfinite(radius)]
    p01, p50 = (float(q) for q in np.quantile(fin, [0.01, 0.5])) if fin.size else (float("nan"), float("nan"))
    return dict(mean=mean, gauss=gauss, k1=k1, k2=k2, min_radius=radius, n_undefined=int(np.isnan(mean).sum()),
                min_radius_p01=p01, min_radius_p50=p50)


def export_stl(filename, verts, tris):
    """binary STL of a triangle mesh (verts (nv, 3) float32, tris (nt, 3) 0-based); ".stl" is appended when missing.
    Returns the path written."""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    L.check(L.lib().r2s_export_stl(str(filename).encode(), _f(v), len(v), t.ctypes.data_as(L.c_int32_p), len(t)))
    filename = str(filename)
    return filename if filename.endswith(".stl") else filename + ".stl"


def import_stl(filename, *, weld=True, snap=0.0, device=-1, orient=None, check_intersections=False, split_vertices=False,
               fill_holes=None, simplify=None, simplify_rule="quadric"):
    """The triangles of a binary or ASCII STL file -> (verts (nv, 3) float32, tris (nt, 3) int32).  weld=True (needs the GPU): the
    vertices that are the same point are merged by mesh_weld(soup, snap=snap) with its defaults (collapsed triangles and unused
    vertices dropped), so the mesh tools see shared vertices; weld=False: the soup as the file holds it, 3 nt vertices and
    tris = arange.  Facet normals and attribute bytes are ignored.  orient=None: the windings as the file holds them;
    "majority" or "outward" (needs weld=True): the welded triangles go through mesh_orient(outward=(orient == "outward")), whose
    docstring has the rules and the caveat about enclosed voids; "nested" (needs weld=True): mesh_orient(outward=True) and then
    mesh_nesting(rewind=True), so that closed bodies are positive and the voids enclosed in them negative, alternating with the
    depth of the nesting.  check_intersections=True (needs weld=True): the result is
    (verts, tris, MeshIntersections), the self-intersections of the mesh as returned (mesh_intersections): zero pairs are what
    the shells, the orientation, sections and thickness take for granted.  split_vertices=True (needs weld=True): after the weld,
    and after the orient if one is asked for, the vertices the weld left pinched (two bodies touching in a point) are split by
    mesh_fans(split=True), so that every vertex of the result has a single fan unless it lies on a non-manifold edge.
    fill_holes=k (needs weld=True): after the weld, the orient and the split, the closed rims of the mesh are capped by
    mesh_holes(fill=k): -1 every hole, k > 0 the holes of at most k edges.  The intersections are those of the filled mesh.
    simplify=cell (needs weld=True): directly after the weld, before the orient, the split and the fill, the mesh is decimated by
    mesh_simplify(verts, tris, cell, simplify_rule); what clustering can leave behind (pinched vertices, non-manifold edges) is
    what the later steps and checks are there for.

    From an STL file to the signed-distance volume everything else here produces (the full repair recipe: weld -> simplify
    (optional) -> orient -> split pinched vertices -> fill holes -> check with mesh_shells / mesh_intersections):

        verts, tris, x = import_stl("part.stl", orient="majority", split_vertices=True, fill_holes=-1, check_intersections=True)
        assert len(x) == 0                                        # the surface, caps included, does not pass through itself
        assert mesh_holes(verts, tris).watertight                 # no rim was left open (a fin, a non-manifold edge)
        tris = mesh_orient(verts, tris, outward=True).tris        # every closed shell outward ...
        tris = mesh_nesting(verts, tris, rewind=True).tris        # ... and the enclosed voids inward again, by depth
        grid = Grid(verts.min(0), verts.max(0), 128)              # 128 cells along the longest side, 3 cells of margin
        sdf = mesh_signed_distance(verts, tris, grid)             # (nz, ny, nx), positive inside
        exportSdfToVTI("part_sdf", grid, sdf, "distance")"""
    if orient not in (None, "majority", "outward", "nested"):
        raise L.R2SError('orient must be None, "majority", "outward" or "nested"')
    if orient is not None and not weld:
        raise L.R2SError("orient needs weld=True: a soup has no shared edges to orient across")
    if split_vertices and not weld:
        raise L.R2SError("split_vertices needs weld=True: in a soup no vertex is shared")
    if check_intersections and not weld:
        raise L.R2SError("check_intersections needs weld=True: in a soup every neighbour touches under different indices")
    if fill_holes is not None and not weld:
        raise L.R2SError("fill_holes needs weld=True: in a soup every triangle is a hole of its own")
    if simplify is not None and not weld:
        raise L.R2SError("simplify needs weld=True: clustering works on an indexed mesh")
    m = L.R2SStlMesh()
    L.check(L.lib().r2s_import_stl(str(filename).encode(), ctypes.byref(m)))
    try:
        n = int(m.n_tris)
        soup = np.ctypeslib.as_array(m.verts, shape=(3 * n, 3)).copy() if n else np.empty((0, 3), np.float32)
    finally:
        L.lib().r2s_free_stl_mesh(ctypes.byref(m))
    if not weld:
        return soup, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    w = mesh_weld(soup, None, snap=snap, device=device)
    if simplify is not None:
        w = mesh_simplify(w.verts, w.tris, simplify, simplify_rule, device=device)
    verts = w.verts
    tris = w.tris if orient is None else mesh_orient(verts, w.tris, outward=orient != "majority", device=device).tris
    if orient == "nested":
        tris = mesh_nesting(verts, tris, rewind=True, device=device).tris
    if split_vertices:
        f = mesh_fans(verts, tris, split=True, device=device)
        verts, tris = f.verts, f.tris
    if fill_holes is not None:
        h = mesh_holes(verts, tris, fill=int(fill_holes), device=device)
        verts, tris = h.verts, h.tris
    if check_intersections:
        return verts, tris, mesh_intersections(verts, tris, device=device)
    return verts, tris


def exportToVTU(fileName, X, IEN, VTK_CODE=None, rho=None):
    """exportToVTU(fileName, X, IEN, VTK_CODE, rho) - ASCII UnstructuredGrid of the mesh with optional nodal
    densities (src/DataExport/ExportToVTU.jl:2-99).  X (nnp, 3), IEN (nel, nen) 1-based; VTK_CODE defaults to
    12 (hexahedron) / 10 (tetra) by the number of element nodes, like the reference's callers."""
    mesh = Mesh(X, IEN)
    code = (12 if mesh.nen == 8 else 10) if VTK_CODE is None else int(VTK_CODE)
    r = None
    if rho is not None:
        r = np.ascontiguousarray(rho, dtype=np.float64)
        if r.shape != (mesh.nnp,):
            raise L.R2SError("length of nodal densities does not match number of nodes")
    L.check(L.lib().r2s_export_vtu(str(fileName).encode(), _d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, mesh.nen, code,
                                   _d(r) if r is not None else None))
    return str(fileName)


def import_vtu_mesh(vtu_file, info=None):
    """import_vtu_mesh(vtu_file) -> (X, IEN, rho)   (src/DataImport/VTUImport.jl:22-112)
    X (nnp, 3) Float64, IEN (nel, nen) Int64 1-based, rho (nel,) element densities.  ASCII .vtu only.
    `info` (a dict) receives element_type, n_skipped and the cell-data field the densities came from."""
    m = L.R2SVtuMesh()
    L.check(L.lib().r2s_import_vtu(str(vtu_file).encode(), ctypes.byref(m)))
    try:
        X = np.ctypeslib.as_array(m.X, shape=(m.nnp, 3)).copy()
        IEN = np.ctypeslib.as_array(m.IEN, shape=(m.nel, m.nen)).copy()
        rho = np.ctypeslib.as_array(m.rho, shape=(m.nel,)).copy()
        if info is not None:
            info.update(element_type=int(m.elem_type), n_skipped=int(m.n_skipped),
                        density_field=m.density_field.decode())
    finally:
        L.lib().r2s_free_vtu_mesh(ctypes.byref(m))
    return X, IEN, rho


def MeshInformations(mat_file):
    """MeshInformations(matread(file)) -> (X, IEN, rho)   (src/MeshGrid/MeshInformations.jl:3-12) for MATLAB level-5
    .mat files: X (nnp, 3), IEN (nel, nen) = stored connectivity + 1, rho (nel,)."""
    m = L.R2SVtuMesh()
    L.check(L.lib().r2s_import_mat(str(mat_file).encode(), ctypes.byref(m)))
    try:
        X = np.ctypeslib.as_array(m.X, shape=(m.nnp, 3)).copy()
        IEN = np.ctypeslib.as_array(m.IEN, shape=(m.nel, m.nen)).copy()
        rho = np.ctypeslib.as_array(m.rho, shape=(m.nel,)).copy()
    finally:
        L.lib().r2s_free_vtu_mesh(ctypes.byref(m))
    return X, IEN, rho


def export_sdf_results(fine_sdf, sdf_grid, taskName, smooth, is_interpolation, element_type):
    """export_sdf_results_with_element_type (src/RhoToSDF.jl:249-283), the .vti part: same file name
    `<task>_<HEX8|TET4>_B-<round(cell,4)>_smooth-<s>_<Interpolation|Approximation>.vti`, point array "distance".
    (The two .jld2 dumps are Julia serialisation and stay in the Julia package.)"""
    name = "Interpolation" if is_interpolation else "Approximation"
    ename = "HEX8" if element_type == L.HEX8 else "TET4"
    B = round(float(sdf_grid.cell_size), 4)
    return exportSdfToVTI(f"{taskName}_{ename}_B-{B}_smooth-{smooth}_{name}.vti", sdf_grid, fine_sdf, "distance", smooth)


class Rho2sdfOptions:
    """Rho2sdfOptions (src/RhoToSDF.jl:9-77): same fields, defaults and validation rules; file-export
    switches are accepted and ignored here (file I/O stays in the Julia package)."""

    def __init__(self, threshold_density=None, sdf_grid_setup="manual", export_input_data=False,
                 export_nodal_densities=False, export_raw_sdf=False, rbf_interp=True, rbf_grid="same",
                 remove_artifacts=True, artifact_min_component_ratio=0.01, export_analysis=False,
                 element_type=None, rbf_kernel_threshold=None):
        import warnings
        if threshold_density is not None and not (0.0 <= threshold_density <= 1.0):
            warnings.warn(f"Threshold density {threshold_density} is outside the valid range [0.0, 1.0]. "
                          "Will use automatic calculation instead.")
            threshold_density = None
        if sdf_grid_setup not in ("manual", "automatic"):
            warnings.warn(f"Invalid sdf_grid_setup: {sdf_grid_setup}. Using default manual instead.")
            sdf_grid_setup = "manual"
        if rbf_grid not in ("same", "fine"):
            warnings.warn(f"Invalid rbf_grid: {rbf_grid}. Using default same instead.")
            rbf_grid = "same"
        self.threshold_density = threshold_density
        self.sdf_grid_setup = sdf_grid_setup
        self.rbf_interp = rbf_interp
        self.rbf_grid = rbf_grid
        self.remove_artifacts = remove_artifacts
        self.artifact_min_component_ratio = artifact_min_component_ratio
        self.export_analysis = export_analysis
        self.element_type = element_type
        self.rbf_kernel_threshold = rbf_kernel_threshold   # None: the library's default (1e-3, RBFs4Smoothing.jl:328)


def rho2sdf(taskName, X, IEN, rho, *, options=None, sdf_grid=None, device=-1, export_results=False, n_gpus=1,
            info=None, pinned_results=False, fine_out=None, dists_out=None, surface=False, redistance_cells=None,
            signed_distance=False, deviation=False, thickness=False, shells=False, sections=None, simplify_cells=None,
            simplify_rule="quadric"):
    """rho2sdf(taskName, X, IEN, rho; options) -> (fine_sdf, fine_grid, sdf_grid, sdf_dists)
    src/RhoToSDF.jl:116-242.  ONE call into the library (r2s_rho2sdf): the mesh goes up once, mesh volume ->
    nodal densities -> threshold -> raw SDF -> artifact removal -> RBF smoothing run on HBM-resident data, the two
    result arrays come down once (pinned_results=True: into arrays from r2s_host_alloc - plain DMA, but pinning 1.6 GB
    costs ~0.2 s, so it only pays when the arrays are reused; the default staged path runs within 5 % of it).
    `sdf_grid` replaces the interactive prompt of sdf_grid_setup = :manual (Grid_setup.jl:111-154 is out of scope).
    fine_grid is returned as (origin, spacing, dims) instead of one heap vector per voxel.  export_results=True
    writes the final `.vti` like RhoToSDF.jl:230-238 (the .jld2 dumps stay in the Julia package).  `info` (a dict)
    receives V_domain, V_frac, rho_t, n_flipped, level_shift, cg_iters, per-stage milliseconds and rho_n; with
    options.export_analysis and remove_artifacts also "components_before": analyze_sdf_components of the raw field
    (RhoToSDF.jl:177-179), taken from the labelling the artifact removal runs anyway.
    `fine_out` (Float32, one value per fine grid point) / `dists_out` (Float64, one per sdf_grid point): result arrays
    to fill instead of new ones (e.g. from host_array); fine_sdf is then a view of fine_out.
    surface=True: the library also extracts the iso-0 surface of fine_sdf on the device (r2s_options extract_surface);
    info["surface"] = (verts, tris) as extract_isosurface(fine_sdf, sdf_grid, smooth) returns them (bit-identical), and
    export_results=True also writes it next to the .vti as <same name>.stl.  The return values are unchanged.
    simplify_cells=k (a positive number; needs surface=True): the extracted surface is decimated by mesh_simplify with cell = k
    spacings of the fine lattice and simplify_rule, a further library call after the first; the simplified mesh is then THE
    surface: info["surface"], what thickness / shells / sections read and what the .stl holds; info["simplify"] = the MeshSimplify.
    (deviation=True still measures the surface as extracted, so that it does not include the decimation.)
    redistance_cells=k (a positive number; needs `info`): info["sdf_redistanced"] = redistance(fine_sdf, sdf_grid, smooth,
    band=k * spacing of the fine lattice) - the banded signed distance to the iso-0 surface of fine_sdf, a second library
    call after the first.  None: nothing is called.
    signed_distance=True (needs `info`): info["sdf_distance"] = redistance_full(fine_sdf, sdf_grid, smooth), the signed distance
    to the iso-0 surface of fine_sdf on the whole fine lattice.  deviation=True (needs `info`): info["smoothing_deviation"] =
    surface_deviation of the iso-0 surface of fine_sdf (A) against the iso-0 surface of the raw sdf_dists on the coarse
    lattice (B): how far the smoothing moved the surface.  Both are further library calls after the first; with the defaults
    nothing new is called.
    thickness=True (needs `info`; implies surface=True): info["thickness"] = surface_thickness(*info["surface"], skip=half a
    spacing of the fine lattice) - (thickness, hit_tri, side) at every vertex of the extracted surface, a further library
    call after the first.
    shells=True (needs `info`; implies surface=True): info["shells"] = mesh_shells(*info["surface"]) - the bodies of the exported
    mesh, their topology, volumes and enclosed voids - a further library call after the first.
    sections=(normal, levels) (needs `info`; implies surface=True): info["sections"] = mesh_sections(*info["surface"], normal,
    levels) - the cross-sections of the exported mesh along an axis, a further library call after the first."""
    options = options or Rho2sdfOptions()
    if (signed_distance or deviation) and info is None:
        raise L.R2SError("signed_distance / deviation need an `info` dict for the result")
    if thickness and info is None:
        raise L.R2SError("thickness needs an `info` dict for the result")
    if shells and info is None:
        raise L.R2SError("shells needs an `info` dict for the result")
    if sections is not None and info is None:
        raise L.R2SError("sections needs an `info` dict for the result")
    surface = bool(surface) or bool(thickness) or bool(shells) or sections is not None
    if simplify_cells is not None and not (surface and float(simplify_cells) > 0.0):
        raise L.R2SError("simplify_cells must be a positive number and needs surface=True")
    if redistance_cells is not None and (info is None or not (float(redistance_cells) > 0.0)):
        raise L.R2SError("redistance_cells must be a positive number and needs an `info` dict for the result")
    mesh = Mesh(X, IEN, options.element_type)
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    if rho.shape != (mesh.nel,):
        raise L.R2SError("length of element densities does not match number of elements")
    if sdf_grid is None:
        if options.sdf_grid_setup != "automatic":
            raise L.R2SError("sdf_grid_setup = :manual needs an explicit sdf_grid here")
        sdf_grid = noninteractive_sdf_grid_setup(mesh)                                       # :141-145
    smooth = 1 if options.rbf_grid == "same" else 2                                          # :222
    o = L.R2SOptions()
    L.lib().r2s_default_options(ctypes.byref(o))
    if options.threshold_density is not None:                                                # :151-156
        o.threshold_density = float(options.threshold_density)
    o.elem_type = mesh.element_type
    o.rbf_interp = int(bool(options.rbf_interp))
    o.rbf_smooth = smooth
    o.remove_artifacts = int(bool(options.remove_artifacts))
    o.artifact_min_component_ratio = float(options.artifact_min_component_ratio)
    analysis = info is not None and bool(getattr(options, "export_analysis", False)) and bool(options.remove_artifacts)
    o.analyze_components = int(analysis)
    if getattr(options, "rbf_kernel_threshold", None) is not None:
        o.rbf_kernel_threshold = float(options.rbf_kernel_threshold)
    o.device = int(device)
    o.n_gpus = int(n_gpus)
    o.extract_surface = int(bool(surface))
    dims = tuple(int(nn) * smooth + 1 for nn in sdf_grid.c.N)
    nfine = dims[0] * dims[1] * dims[2]
    alloc = host_array if pinned_results else (lambda n, dt=np.float64: np.empty(n, dtype=dt))
    sdf_dists = alloc(sdf_grid.ngp) if dists_out is None else _out(dists_out, sdf_grid.ngp)
    fine = alloc(nfine, np.float32) if fine_out is None else _out(fine_out, nfine, np.float32)
    rho_n = np.empty(mesh.nnp)
    ri = L.R2SRunInfo()
    L.check(L.lib().r2s_rho2sdf(_d(mesh.X), mesh.nnp, _i(mesh.IEN), mesh.nel, _d(rho), ctypes.byref(o),
                                ctypes.byref(sdf_grid.c), _d(rho_n), None, _d(sdf_dists), _f(fine), ctypes.byref(ri)))
    if info is not None:
        info.update(ri.as_dict())
        info["rho_n"] = rho_n
        if analysis:
            info["components_before"] = _components_dict(lambda r, s, cap, n: L.lib().r2s_last_components(r, s, cap, n))
    mesh_out = _last_isosurface() if surface else None
    extracted = mesh_out                                  # (the smoothing deviation reads the surface as extracted)
    if simplify_cells is not None:
        simplified = mesh_simplify(*mesh_out, float(simplify_cells) * _iso_lattice(sdf_grid, smooth)[2], simplify_rule, device=device)
        mesh_out = (simplified.verts, simplified.tris)
        if info is not None:
            info["simplify"] = simplified
    if info is not None and surface:
        info["surface"] = mesh_out
    fine_sdf = fine.reshape(dims[2], dims[1], dims[0])
    xmin, xmax = np.float32(sdf_grid.AABB_min[0]), np.float32(sdf_grid.AABB_max[0])
    spacing = (xmax - xmin) / np.float32(fine_sdf.shape[2] - 1)
    fine_grid = (sdf_grid.AABB_min.astype(np.float32), float(spacing), fine_sdf.shape[::-1])
    if redistance_cells is not None:
        info["sdf_redistanced"] = redistance(fine_sdf, sdf_grid, smooth, band=float(redistance_cells) * _iso_lattice(sdf_grid, smooth)[2],
                                             device=device)
    if signed_distance:
        info["sdf_distance"] = redistance_full(fine_sdf, sdf_grid, smooth, device=device)
    if deviation:
        smoothed = extracted if surface else extract_isosurface(fine_sdf, sdf_grid, smooth, device=device)
        raw = extract_isosurface(sdf_dists, sdf_grid, None, device=device)
        info["smoothing_deviation"] = surface_deviation(*smoothed, *raw, device=device)
    if thickness:
        info["thickness"] = surface_thickness(*mesh_out, skip=0.5 * _iso_lattice(sdf_grid, smooth)[2], device=device)
    if shells:
        info["shells"] = mesh_shells(*mesh_out, device=device)
    if sections is not None:
        info["sections"] = mesh_sections(*mesh_out, sections[0], sections[1], device=device)
    if export_results:
        vti = export_sdf_results(fine_sdf, sdf_grid, taskName, smooth, options.rbf_interp, mesh.element_type)
        if surface:
            export_stl(vti[:-len(".vti")] + ".stl", *mesh_out)
    return fine_sdf, fine_grid, sdf_grid, sdf_dists
