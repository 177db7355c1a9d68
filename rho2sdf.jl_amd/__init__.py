"""rho2sdf.jl_amd - MI355X-native signed-distance extraction (hot path of Rho2sdf.jl).

The directory name contains a dot, so load it with tests/conftest.py's
`load_package()` (importlib) or `__graft_entry__.load_package()`; it registers
itself as module `rho2sdf_jl_amd`.
"""
from . import _lib
from .api import (DenseInNodes, analyze_sdf_components, DevicePlan, Grid, Mesh, RBFs_smoothing, Rho2sdfOptions, Sign_Detection,
                  calculate_mesh_volume, calculate_volume_from_sdf, evalDistances, find_threshold_for_volume,
                  exportSdfToVTI, exportToVTU, export_sdf_results, getMesh_AABB, import_vtu_mesh, noninteractive_sdf_grid_setup,
                  remove_sdf_artifacts, rho2sdf, sdf_fused, host_array, calculate_isocontour_volume, MeshInformations,
                  extract_isosurface, extract_isosurface_dev, export_stl, RbfField, fit_rbf_field, refine_surface, last_rbf_plan,
                  surface_curvature,
                  mesh_distance, mesh_distance_dev, redistance, redistance_dev, last_distance_stats,
                  MeshIndex, redistance_full, redistance_full_dev, surface_deviation,
                  vertex_normals, surface_thickness, surface_thickness_dev,
                  MeshShells, mesh_shells, mesh_shells_dev, select_shells,
                  MeshSections, mesh_sections, mesh_sections_dev,
                  MeshWeld, mesh_weld, mesh_weld_dev, import_stl, MeshSimplify, mesh_simplify, mesh_simplify_dev,
                  MeshOrient, mesh_orient, mesh_orient_dev, flip_patches,
                  MeshFans, mesh_fans, mesh_fans_dev,
                  MeshHoles, mesh_holes, mesh_holes_dev,
                  MeshIntersections, mesh_intersections, mesh_intersections_dev,
                  MeshNesting, mesh_nesting, mesh_nesting_dev,
                  mesh_signed_distance, mesh_signed_distance_dev)

__all__ = ["DenseInNodes", "analyze_sdf_components", "DevicePlan", "Grid", "Mesh", "RBFs_smoothing", "Rho2sdfOptions", "Sign_Detection",
           "calculate_mesh_volume", "calculate_volume_from_sdf", "evalDistances", "find_threshold_for_volume",
           "exportSdfToVTI", "exportToVTU", "export_sdf_results", "getMesh_AABB", "import_vtu_mesh", "noninteractive_sdf_grid_setup", "remove_sdf_artifacts",
           "rho2sdf", "sdf_fused", "host_array", "calculate_isocontour_volume", "MeshInformations",
           "extract_isosurface", "extract_isosurface_dev", "export_stl", "RbfField", "fit_rbf_field", "refine_surface", "last_rbf_plan",
           "surface_curvature",
           "mesh_distance", "mesh_distance_dev", "redistance", "redistance_dev", "last_distance_stats",
           "MeshIndex", "redistance_full", "redistance_full_dev", "surface_deviation",
           "vertex_normals", "surface_thickness", "surface_thickness_dev",
           "MeshShells", "mesh_shells", "mesh_shells_dev", "select_shells",
           "MeshSections", "mesh_sections", "mesh_sections_dev",
           "MeshWeld", "mesh_weld", "mesh_weld_dev", "import_stl", "MeshSimplify", "mesh_simplify", "mesh_simplify_dev",
           "MeshOrient", "mesh_orient", "mesh_orient_dev", "flip_patches",
           "MeshFans", "mesh_fans", "mesh_fans_dev",
           "MeshHoles", "mesh_holes", "mesh_holes_dev",
           "MeshIntersections", "mesh_intersections", "mesh_intersections_dev",
           "MeshNesting", "mesh_nesting", "mesh_nesting_dev",
           "mesh_signed_distance", "mesh_signed_distance_dev",
           "_lib"]
