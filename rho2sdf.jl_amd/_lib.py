"""Loader for the C-ABI shared library (include/rho2sdf_hip.h).

The library is the product; there is no CPU fallback.  If the in-tree
librho2sdf_hip.so is missing or does not load, importing this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("R2S_LIB_OVERRIDE") or os.path.join(_HERE, "librho2sdf_hip.so")  # override: A/B builds

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_float_p = ctypes.POINTER(ctypes.c_float)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
OPT_EXTRACT_SURFACE = 0   # R2S_OPT_EXTRACT_SURFACE


class R2SGrid(ctypes.Structure):
    """mirrors `mutable struct Grid` (reference src/MeshGrid/Grid.jl:2-7)"""
    _fields_ = [("aabb_min", ctypes.c_double * 3), ("aabb_max", ctypes.c_double * 3),
                ("N", ctypes.c_int64 * 3), ("cell_size", ctypes.c_double), ("ngp", ctypes.c_int64)]


class R2SParams(ctypes.Structure):
    _fields_ = [("band_factor", ctypes.c_double), ("elem_type", ctypes.c_int32),
                ("device", ctypes.c_int32), ("zstride", ctypes.c_int32), ("zphase", ctypes.c_int32),
                ("n_gpus", ctypes.c_int32), ("true_min", ctypes.c_int32), ("sign_no_inner", ctypes.c_int32),
                ("reserved_", ctypes.c_int32)]


class R2SOptions(ctypes.Structure):
    """mirrors r2s_options (= Rho2sdfOptions, reference src/RhoToSDF.jl:9-77)"""
    _fields_ = [("threshold_density", ctypes.c_double), ("band_factor", ctypes.c_double),
                ("artifact_min_component_ratio", ctypes.c_double), ("rbf_kernel_threshold", ctypes.c_double),
                ("elem_type", ctypes.c_int32), ("rbf_interp", ctypes.c_int32), ("rbf_smooth", ctypes.c_int32),
                ("remove_artifacts", ctypes.c_int32), ("device", ctypes.c_int32), ("n_gpus", ctypes.c_int32),
                ("skip_rbf", ctypes.c_int32), ("true_min", ctypes.c_int32), ("sign_no_inner", ctypes.c_int32),
                ("analyze_components", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]
    # reserved[R2S_OPT_EXTRACT_SURFACE] (include/rho2sdf_hip.h): keep the iso-0 surface of the fine field
    extract_surface = property(lambda s: s.reserved[OPT_EXTRACT_SURFACE],
                               lambda s, v: s.reserved.__setitem__(OPT_EXTRACT_SURFACE, int(v)))


class R2SRunInfo(ctypes.Structure):
    _fields_ = [("V_domain", ctypes.c_double), ("V_frac", ctypes.c_double), ("rho_t", ctypes.c_double),
                ("n_flipped", ctypes.c_int64), ("level_shift", ctypes.c_float), ("cg_iters", ctypes.c_int32),
                ("threshold_iters", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("ms_upload", ctypes.c_double), ("ms_pre", ctypes.c_double), ("ms_sdf", ctypes.c_double),
                ("ms_sdf_kernels", ctypes.c_double), ("ms_artifacts", ctypes.c_double), ("ms_rbf", ctypes.c_double),
                ("ms_download", ctypes.c_double), ("ms_total", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class R2SStats(ctypes.Structure):
    _fields_ = [("n_solid", ctypes.c_int64), ("n_iso", ctypes.c_int64), ("n_items", ctypes.c_int64),
                ("n_band_entries", ctypes.c_int64), ("n_sign_entries", ctypes.c_int64),
                ("n_tiles", ctypes.c_int64), ("n_active_tiles", ctypes.c_int64),
                ("n_active_sign_tiles", ctypes.c_int64), ("n_iso_chunks", ctypes.c_int64),
                ("n_any_tiles", ctypes.c_int64),
                ("ms_prep", ctypes.c_double), ("ms_bins", ctypes.c_double),
                ("ms_fill", ctypes.c_double), ("ms_main", ctypes.c_double),
                ("ms_gather", ctypes.c_double), ("ms_sign", ctypes.c_double),
                ("n_sign_only_tiles", ctypes.c_int64), ("ms_iso_fast", ctypes.c_double),
                ("n_iso_straggler", ctypes.c_int64), ("n_iso_fail", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class R2SVtuMesh(ctypes.Structure):
    _fields_ = [("nnp", ctypes.c_int64), ("nel", ctypes.c_int64), ("nen", ctypes.c_int32),
                ("elem_type", ctypes.c_int32), ("n_skipped", ctypes.c_int64), ("X", c_double_p),
                ("IEN", c_int64_p), ("rho", c_double_p), ("density_field", ctypes.c_char * 64)]


class R2SStlMesh(ctypes.Structure):
    _fields_ = [("n_tris", ctypes.c_int64), ("verts", c_float_p)]


# every symbol include/rho2sdf_hip.h declares: (name, restype, argtypes)
_P = ctypes.c_void_p
_MESH = [c_double_p, ctypes.c_int64, c_int64_p, ctypes.c_int64]
_COMMON = _MESH + [c_double_p, ctypes.c_double, ctypes.POINTER(R2SGrid), ctypes.POINTER(R2SParams)]
SYMBOLS = [
    ("r2s_version", ctypes.c_int, []),
    ("r2s_last_error", ctypes.c_char_p, []),
    ("r2s_device_count", ctypes.c_int, []),
    ("r2s_default_params", None, [ctypes.POINTER(R2SParams)]),
    ("r2s_grid_make", ctypes.c_int, [c_double_p, c_double_p, ctypes.c_int64, ctypes.c_int64,
                                     ctypes.POINTER(R2SGrid)]),
    ("r2s_auto_grid", ctypes.c_int, _MESH + [ctypes.c_int32, ctypes.POINTER(R2SGrid), c_double_p]),
    ("r2s_eval_distances", ctypes.c_int, _COMMON + [c_double_p, c_double_p, ctypes.POINTER(R2SStats)]),
    ("r2s_sign_detection", ctypes.c_int, _COMMON + [c_double_p, ctypes.POINTER(R2SStats)]),
    ("r2s_sdf", ctypes.c_int, _COMMON + [c_double_p, ctypes.POINTER(R2SStats)]),
    ("r2s_plan_create", ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(_P)]),
    ("r2s_plan_destroy", None, [_P]),
    ("r2s_plan_run_dev", ctypes.c_int,
     [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.c_double, ctypes.POINTER(R2SGrid),
      ctypes.POINTER(R2SParams), ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _P, _P, _P, _P, _P,
      ctypes.POINTER(R2SStats)]),
    ("r2s_plan_pack_tiles_dev", ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, c_int64_p, _P]),
    ("r2s_unpack_tiles_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(R2SGrid), _P, _P]),
    ("r2s_fill_dev", ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_double, _P]),
    ("r2s_plan_pack_tiles2_dev", ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, c_int64_p,
                                                c_int64_p, _P]),
    ("r2s_unpack_masks_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(R2SGrid), ctypes.c_double, _P, _P]),
    ("r2s_unpack_segments_dev", ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.POINTER(R2SGrid), ctypes.c_double, _P, _P]),
    ("r2s_mesh_volume", ctypes.c_int, _MESH + [ctypes.c_int32, c_double_p, ctypes.c_int32, c_double_p, c_double_p]),
    ("r2s_dense_in_nodes", ctypes.c_int, _MESH + [ctypes.c_int32, c_double_p, ctypes.c_int32, c_double_p]),
    ("r2s_find_threshold", ctypes.c_int, _MESH + [c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                                  ctypes.c_int32, c_double_p, ctypes.POINTER(ctypes.c_int32)]),
    ("r2s_find_threshold_et", ctypes.c_int, _MESH + [ctypes.c_int32, c_double_p, ctypes.c_double, ctypes.c_double,
                                                     ctypes.c_int32, ctypes.c_int32, c_double_p,
                                                     ctypes.POINTER(ctypes.c_int32)]),
    ("r2s_isocontour_volume", ctypes.c_int, _MESH + [ctypes.c_int32, c_double_p, ctypes.c_double, ctypes.c_int32,
                                                     c_double_p]),
    ("r2s_default_options", None, [ctypes.POINTER(R2SOptions)]),
    ("r2s_rho2sdf", ctypes.c_int, _MESH + [c_double_p, ctypes.POINTER(R2SOptions), ctypes.POINTER(R2SGrid), c_double_p,
                                           c_double_p, c_double_p, c_float_p, ctypes.POINTER(R2SRunInfo)]),
    ("r2s_last_host_phases", None, [c_double_p]),
    ("r2s_host_alloc", ctypes.c_void_p, [ctypes.c_size_t]),
    ("r2s_host_free", None, [ctypes.c_void_p]),
    ("r2s_remove_artifacts", ctypes.c_int, [c_double_p, ctypes.POINTER(R2SGrid), ctypes.c_double, ctypes.c_double,
                                            ctypes.c_int32, c_int64_p]),
    ("r2s_remove_artifacts_dev", ctypes.c_int, [_P, ctypes.POINTER(R2SGrid), ctypes.c_double, ctypes.c_double, _P,
                                                c_int64_p]),
    ("r2s_analyze_components", ctypes.c_int, [c_double_p, ctypes.POINTER(R2SGrid), ctypes.c_double, ctypes.c_int32,
                                              c_int64_p, c_int64_p, ctypes.c_int64, c_int64_p]),
    ("r2s_analyze_components_dev", ctypes.c_int, [_P, ctypes.POINTER(R2SGrid), ctypes.c_double, _P, c_int64_p, c_int64_p,
                                                  ctypes.c_int64, c_int64_p]),
    ("r2s_last_components", ctypes.c_int, [c_int64_p, c_int64_p, ctypes.c_int64, c_int64_p]),
    ("r2s_volume_from_sdf", ctypes.c_int, [c_float_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_float,
                                           ctypes.c_float, ctypes.c_int32, ctypes.c_int32, c_float_p]),
    ("r2s_rbf_smooth", ctypes.c_int, [c_double_p, ctypes.POINTER(R2SGrid), ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_double, ctypes.c_double, ctypes.c_int32, c_float_p, c_float_p,
                                      ctypes.POINTER(ctypes.c_int32), c_float_p]),
    ("r2s_last_rbf_plan", None, [c_int32_p]),
    ("r2s_release_cache", None, []),
    ("r2s_live_device_bytes", ctypes.c_int64, []),
    ("r2s_export_vtu", ctypes.c_int, [ctypes.c_char_p] + _MESH + [ctypes.c_int32, ctypes.c_int32, c_double_p]),
    ("r2s_import_vtu", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(R2SVtuMesh)]),
    ("r2s_free_vtu_mesh", None, [ctypes.POINTER(R2SVtuMesh)]),
    ("r2s_export_vti", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(R2SGrid), _P, ctypes.c_int32, ctypes.c_int64,
                                      ctypes.c_char_p, ctypes.c_int32]),
    ("r2s_export_vti_z", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(R2SGrid), _P, ctypes.c_int32, ctypes.c_int64,
                                        ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32]),
    ("r2s_import_mat", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(R2SVtuMesh)]),
    ("r2s_rbf_smooth_dev", ctypes.c_int, [_P, ctypes.POINTER(R2SGrid), ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                          ctypes.c_double, _P, c_float_p, ctypes.POINTER(ctypes.c_int32), _P]),
    ("r2s_extract_isosurface", ctypes.c_int, [_P, ctypes.c_int32, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_int32, c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, c_int64_p,
                                              c_int64_p]),
    ("r2s_last_isosurface", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, c_int64_p, c_int64_p]),
    ("r2s_extract_isosurface_dev", ctypes.c_int, [_P, ctypes.c_int32, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                                  _P, ctypes.c_int64, _P, ctypes.c_int64, c_int64_p, c_int64_p, _P]),
    ("r2s_export_stl", ctypes.c_int, [ctypes.c_char_p, c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64]),
    ("r2s_rbf_field_fit", ctypes.c_int, [c_double_p, ctypes.POINTER(R2SGrid), ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int32, ctypes.POINTER(_P), c_float_p, c_int32_p]),
    ("r2s_rbf_field_from_weights", ctypes.c_int, [c_float_p, ctypes.POINTER(R2SGrid), ctypes.c_double, ctypes.c_float,
                                                  ctypes.c_int32, ctypes.POINTER(_P)]),
    ("r2s_rbf_field_weights", ctypes.c_int, [_P, c_float_p, c_float_p]),
    ("r2s_rbf_field_destroy", None, [_P]),
    ("r2s_rbf_field_eval", ctypes.c_int, [_P, c_float_p, ctypes.c_int64, c_float_p, c_float_p, c_int32_p]),
    ("r2s_rbf_field_eval_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P, _P, _P]),
    ("r2s_rbf_field_hessian", ctypes.c_int, [_P, c_float_p, ctypes.c_int64, c_float_p, c_float_p, c_float_p, c_int32_p]),
    ("r2s_rbf_field_hessian_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    ("r2s_rbf_field_curvature", ctypes.c_int, [_P, c_float_p, ctypes.c_int64, c_float_p, c_float_p, c_float_p]),
    ("r2s_rbf_field_curvature_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P, _P, _P]),
    ("r2s_rbf_field_normals", ctypes.c_int, [_P, c_float_p, ctypes.c_int64, c_float_p]),
    ("r2s_rbf_field_normals_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P]),
    ("r2s_rbf_field_project", ctypes.c_int, [_P, c_float_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, c_int32_p,
                                             c_float_p, c_int32_p]),
    ("r2s_rbf_field_project_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, _P, _P, _P, _P]),
    ("r2s_mesh_distance", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, c_int64_p, c_double_p,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _P, c_int32_p]),
    ("r2s_mesh_distance_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, c_int64_p, c_double_p, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_int32, _P, _P, _P]),
    ("r2s_redistance", ctypes.c_int, [_P, ctypes.c_int32, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_int32, _P]),
    ("r2s_redistance_dev", ctypes.c_int, [_P, ctypes.c_int32, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, _P, _P]),
    ("r2s_last_distance_stats", None, [c_double_p]),
    ("r2s_mesh_index_build", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32,
                                            ctypes.POINTER(_P)]),
    ("r2s_mesh_index_build_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, ctypes.POINTER(_P)]),
    ("r2s_mesh_index_destroy", None, [_P]),
    ("r2s_mesh_index_info", ctypes.c_int, [_P, c_int64_p]),
    ("r2s_mesh_index_query", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, _P, c_int32_p]),
    ("r2s_mesh_index_query_dev", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, _P, _P, _P]),
    ("r2s_mesh_index_lattice", ctypes.c_int, [_P, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_int32, _P, c_int32_p]),
    ("r2s_mesh_index_lattice_dev", ctypes.c_int, [_P, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_int32, _P, _P, _P]),
    ("r2s_redistance_full", ctypes.c_int, [_P, ctypes.c_int32, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_int32, _P]),
    ("r2s_redistance_full_dev", ctypes.c_int, [_P, ctypes.c_int32, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_double,
                                               _P, _P]),
    ("r2s_mesh_index_raycast", ctypes.c_int, [_P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_int32, _P, c_int32_p, _P]),
    ("r2s_mesh_index_raycast_dev", ctypes.c_int, [_P, _P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                                  ctypes.c_int32, _P, _P, _P, _P]),
    ("r2s_mesh_index_winding", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, c_int32_p, c_int32_p]),
    ("r2s_mesh_index_winding_dev", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, _P, _P, _P]),
    ("r2s_mesh_index_winding_lattice", ctypes.c_int, [_P, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_int32, c_int32_p, c_int32_p]),
    ("r2s_mesh_index_winding_lattice_dev", ctypes.c_int, [_P, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_int32, _P, _P, _P]),
    ("r2s_mesh_index_signed", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P,
                                             c_int32_p]),
    ("r2s_mesh_index_signed_dev", ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P,
                                                 _P, _P]),
    ("r2s_mesh_index_signed_lattice", ctypes.c_int, [_P, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                                     ctypes.c_int32, _P, c_int32_p]),
    ("r2s_mesh_index_signed_lattice_dev", ctypes.c_int, [_P, c_int64_p, c_double_p, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                                         ctypes.c_int32, _P, _P, _P]),
    ("r2s_mesh_signed_distance", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, c_int64_p, c_double_p, ctypes.c_double,
                                                ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P]),
    ("r2s_mesh_signed_distance_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, c_int64_p, c_double_p, ctypes.c_double,
                                                    ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _P, _P]),
    ("r2s_mesh_shells", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32, c_int32_p, c_int64_p,
                                       c_double_p, c_int64_p]),
    ("r2s_last_mesh_shells", ctypes.c_int, [c_int64_p, c_double_p, ctypes.c_int64, c_int64_p]),
    ("r2s_mesh_shells_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, c_int64_p, c_double_p,
                                           c_int64_p, _P]),
    ("r2s_mesh_sections", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int64,
                                         ctypes.c_int32, c_int64_p, c_int64_p, c_double_p, c_int64_p]),
    ("r2s_last_mesh_sections", ctypes.c_int, [c_int64_p, c_int64_p, c_double_p, ctypes.c_int64, c_int32_p, c_double_p, ctypes.c_int64,
                                              c_int64_p, c_int64_p]),
    ("r2s_mesh_sections_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int64, _P, _P, _P,
                                             ctypes.c_int64, _P, _P, ctypes.c_int64, c_int64_p, c_int64_p, c_double_p, c_int64_p, _P]),
    ("r2s_mesh_weld", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int32,
                                     ctypes.c_int32, c_float_p, c_int32_p, c_int32_p, c_int32_p, c_int64_p]),
    ("r2s_mesh_weld_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, _P, _P, _P, _P,
                                         c_int64_p, _P]),
    ("r2s_mesh_simplify", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_int32, c_float_p, c_int32_p, c_int32_p, c_int32_p, c_int64_p]),
    ("r2s_mesh_simplify_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _P, _P,
                                             _P, _P, c_int64_p, _P]),
    ("r2s_last_mesh_simplify", ctypes.c_int, [c_int64_p, c_double_p, c_int32_p, ctypes.c_int64, c_int64_p]),
    ("r2s_mesh_orient", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, c_int32_p,
                                       c_int32_p, c_int32_p, c_int64_p, c_double_p, c_int64_p]),
    ("r2s_last_mesh_orient", ctypes.c_int, [c_int64_p, c_double_p, ctypes.c_int64, c_int64_p]),
    ("r2s_mesh_orient_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, _P, _P, _P, _P, _P, ctypes.c_int64,
                                           c_int64_p, c_double_p, c_int64_p, _P]),
    ("r2s_mesh_fans", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32, c_int32_p, c_int32_p, c_int32_p,
                                     c_float_p, c_int32_p, ctypes.c_int64, c_int64_p, c_int64_p, c_int64_p]),
    ("r2s_last_mesh_fans", ctypes.c_int, [c_int64_p, ctypes.c_int64, c_int64_p]),
    ("r2s_mesh_fans_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int64,
                                         c_int64_p, c_int64_p, c_int64_p, _P]),
    ("r2s_mesh_holes", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, c_int32_p,
                                      c_float_p, ctypes.c_int64, ctypes.c_int64, c_int64_p, c_int64_p, c_int64_p, c_int64_p, c_double_p,
                                      c_int64_p]),
    ("r2s_last_mesh_holes", ctypes.c_int, [c_int64_p, c_int64_p, c_double_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, c_int64_p,
                                           c_int64_p]),
    ("r2s_mesh_holes_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, ctypes.c_int64, _P,
                                          ctypes.c_int64, _P, _P, ctypes.c_int64, ctypes.c_int64, c_int64_p, c_int64_p, c_int64_p, c_int64_p,
                                          c_double_p, c_int64_p, _P]),
    ("r2s_mesh_index_intersections", ctypes.c_int, [_P, c_int32_p, c_int32_p, ctypes.c_int64, c_int64_p]),
    ("r2s_mesh_index_intersections_dev", ctypes.c_int, [_P, _P, _P, ctypes.c_int64, c_int64_p, _P]),
    ("r2s_mesh_intersections", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32, c_int32_p, c_int32_p,
                                              ctypes.c_int64, c_int64_p]),
    ("r2s_mesh_intersections_dev", ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, c_int64_p, _P]),
    ("r2s_mesh_nesting", ctypes.c_int, [c_float_p, ctypes.c_int64, c_int32_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        c_int32_p, c_int32_p, c_int64_p, c_int64_p]),
    ("r2s_last_mesh_nesting", ctypes.c_int, [c_int64_p, ctypes.c_int64, c_int64_p, ctypes.c_int64, c_int64_p, c_int64_p]),
    ("r2s_mesh_nesting_dev", ctypes.c_int, [_P, _P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _P, _P, _P,
                                            ctypes.c_int64, _P, ctypes.c_int64, c_int64_p, c_int64_p, c_int64_p, _P]),
    ("r2s_import_stl", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(R2SStlMesh)]),
    ("r2s_free_stl_mesh", None, [ctypes.POINTER(R2SStlMesh)]),
]

OUT_DIST, OUT_SIGN, OUT_SDF, OUT_XP = 1, 2, 4, 8
HEX8, TET4 = 0, 1
WELD_DROP_COLLAPSED, WELD_DROP_DUPLICATES, WELD_DROP_UNUSED = 1, 2, 4
SIMPLIFY_MEAN, SIMPLIFY_QUADRIC = 0, 1
ORIENT_OUTWARD = 1
NESTING_REWIND = 1

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same SONAME as
        # /opt/rocm's).  If torch is going to be used for device memory / streams it has to be
        # loaded first so this library binds to the runtime torch already initialised;
        # otherwise two runtimes fight over the device ("No HIP GPUs are available").
        if os.environ.get("R2S_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)          # AttributeError if the symbol is not exported
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class R2SError(RuntimeError):
    pass


def check(rc):
    """C-ABI status -> exception, like the reference's `error(...)` calls."""
    if rc != 0:
        raise R2SError(f"rho2sdf_hip error {rc}: {lib().r2s_last_error().decode()}")
