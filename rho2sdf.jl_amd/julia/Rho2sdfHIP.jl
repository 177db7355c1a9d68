# Rho2sdfHIP.jl - thin `ccall` layer that re-points Rho2sdf.jl's hot path at
# librho2sdf_hip.so (C ABI: include/rho2sdf_hip.h).
#
# Two levels:
#   * `rho2sdf(taskName, X, IEN, rho; options)` itself (src/RhoToSDF.jl:116-242) is overridden: ONE ccall
#     (r2s_rho2sdf) uploads the mesh once, runs mesh volume -> DenseInNodes -> threshold -> raw SDF -> artifact
#     removal -> RBF smoothing on HBM-resident data and brings `sdf_dists` and `fine_sdf` down once.  `generateGridPoints` (3.2 GB at 512^3, :166) and the projection points `xp` (:169, discarded by the
#     reference) are never materialised.  All file exports stay Julia code and run on the returned arrays.
#   * every function `rho2sdf` and the reference's tests call directly keeps a ccall-backed method with the
#     reference's signature (leaf overrides), for callers that use the stages one by one.
#
# NOTE: there is no Julia toolchain in the build image, so this file is delivered as reviewed
# text; the same ABI is exercised by rho2sdf.jl_amd/api.py (ctypes) in the test-suite.
#
# Usage (in the reference checkout):
#     include("Rho2sdfHIP.jl"); using .Rho2sdfHIP
#     Rho2sdfHIP.enable!("/path/to/librho2sdf_hip.so"; n_gpus = 1)     # overrides the methods below
module Rho2sdfHIP

using Rho2sdf
using Rho2sdf.MeshGrid
using Rho2sdf.SignedDistances
using Rho2sdf.SdfSmoothing
using Rho2sdf.ElementTypes
using Rho2sdf.ShapeFunctions
using Rho2sdf.DataExport

const LIB = Ref{String}("librho2sdf_hip.so")
const SIGN_NO_INNER = Ref(false)      # true: HEX8 sign pass without the inner-region shortcut (overlapping / non-conforming meshes)
const N_GPUS = Ref{Int32}(1)          # devices one call fans out over (single process; r2s_params.n_gpus)

# mirrors r2s_grid / Grid (src/MeshGrid/Grid.jl:2-7)
struct R2SGrid
    aabb_min::NTuple{3,Float64}
    aabb_max::NTuple{3,Float64}
    N::NTuple{3,Int64}
    cell_size::Float64
    ngp::Int64
end
R2SGrid(g::MeshGrid.Grid) = R2SGrid(Tuple(g.AABB_min), Tuple(g.AABB_max), Tuple(g.N), g.cell_size, g.ngp)

struct R2SParams                      # mirrors r2s_params
    band_factor::Float64
    elem_type::Int32
    device::Int32
    zstride::Int32                    # device-pointer plan API only: interleaved tile layers
    zphase::Int32
    n_gpus::Int32                     # host-pointer entry points: devices 0..n_gpus-1 share the call
    true_min::Int32                   # 1 = order-independent semantics (SURVEY 8(f)4); 0 = the reference's
    sign_no_inner::Int32              # 1 = HEX8 sign pass without the inner-region shortcut (overlapping / non-conforming meshes)
    reserved_::Int32
end
etype(::Type{HEX8}) = Int32(0)
etype(::Type{TET4}) = Int32(1)
params(::Type{T}; band_factor = 1.1) where {T} = R2SParams(band_factor, etype(T), -1, 0, 0, N_GPUS[], 0, SIGN_NO_INNER[] ? 1 : 0, 0)

struct R2SOptions                     # mirrors r2s_options (= Rho2sdfOptions, RhoToSDF.jl:9-77)
    threshold_density::Float64        # NaN = nothing
    band_factor::Float64
    artifact_min_component_ratio::Float64
    rbf_kernel_threshold::Float64
    elem_type::Int32
    rbf_interp::Int32
    rbf_smooth::Int32
    remove_artifacts::Int32
    device::Int32
    n_gpus::Int32
    skip_rbf::Int32
    true_min::Int32
    sign_no_inner::Int32
    analyze_components::Int32         # 1 (with remove_artifacts): keep the component table of the removal's labelling
    reserved::NTuple{2,Int32}
end

struct R2SRunInfo                     # mirrors r2s_run_info
    V_domain::Float64; V_frac::Float64; rho_t::Float64
    n_flipped::Int64
    level_shift::Float32; cg_iters::Int32; threshold_iters::Int32; pad::Int32
    ms_upload::Float64; ms_pre::Float64; ms_sdf::Float64; ms_sdf_kernels::Float64
    ms_artifacts::Float64; ms_rbf::Float64; ms_download::Float64; ms_total::Float64
end

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:r2s_last_error, LIB[]), Cstring, ()))
    error("rho2sdf_hip: $msg")          # same behaviour as the reference's error(...)
end

# Result arrays.  Ordinary Julia arrays by default: the library brings results down through pinned staging buffers
# with a multi-threaded copy, within 5 % of a plain DMA (24.9 vs 24.1 ms for 1 GB).  PINNED[] = true allocates them
# with r2s_host_alloc instead (the copy is then one DMA) - pinning 1.6 GB costs ~0.2 s per call, so that only pays
# for callers that keep and reuse the arrays.  The array owns nothing; a finalizer returns the block to the library.
const PINNED = Ref(false)
function pinned(::Type{T}, dims::Int...) where {T}
    PINNED[] || return Array{T}(undef, dims...)
    n = prod(dims)
    p = ccall((:r2s_host_alloc, LIB[]), Ptr{Cvoid}, (Csize_t,), max(n, 1) * sizeof(T))
    p == C_NULL && error("rho2sdf_hip: " * unsafe_string(ccall((:r2s_last_error, LIB[]), Cstring, ())))
    a = unsafe_wrap(Array, Ptr{T}(p), dims; own = false)
    finalizer(_ -> ccall((:r2s_host_free, LIB[]), Cvoid, (Ptr{Cvoid},), p), a)
    return a
end

# fine_grid.  The reference materialises one heap Vector{Float32} per grid point (create_smooth_grid, RBFs4Smoothing.jl:60-74:
# 134 M allocations = several seconds and 10 GB at 512^3) although only fine_grid[2,1,1] - fine_grid[1,1,1] is ever read
# (CalcVolumeFromSDF.jl:37).  LAZY_GRID[] = true returns the same points as an AbstractArray{Vector{Float32},3} over the three
# coordinate vectors instead - element for element equal to the reference's array (same explicit Float32 arithmetic), built
# on demand.  Default false: the reference's own calculate_volume_from_sdf is declared for Array{Vector{Float32},3} and would
# not accept it (the _hip method below does).
const LAZY_GRID = Ref(false)
struct LazyFineGrid <: AbstractArray{Vector{Float32},3}
    x::Vector{Float32}
    y::Vector{Float32}
    z::Vector{Float32}
end
Base.size(g::LazyFineGrid) = (length(g.x), length(g.y), length(g.z))
Base.getindex(g::LazyFineGrid, i::Int, j::Int, k::Int) = Float32[g.x[i], g.y[j], g.z[k]]
Base.IndexStyle(::Type{LazyFineGrid}) = IndexCartesian()
function fine_grid_of(grid::MeshGrid.Grid, smooth::Int)
    LAZY_GRID[] || return SdfSmoothing.create_smooth_grid(grid, smooth)[2]
    nx, ny, nz = (grid.N * smooth) .+ 1                                   # RBFs4Smoothing.jl:61-73, operation for operation
    xmin, ymin, zmin = Float32.(grid.AABB_min)
    xmax = Float32(grid.AABB_max[1])
    dx = (xmax - xmin) / (nx - 1)
    return LazyFineGrid([xmin + (i - 1) * dx for i in 1:nx], [ymin + (j - 1) * dx for j in 1:ny], [zmin + (k - 1) * dx for k in 1:nz])
end

# ---------------------------------------------------------------------------------------------------
# rho2sdf (src/RhoToSDF.jl:116-242): same signature, same return value, same files written
# ---------------------------------------------------------------------------------------------------
function rho2sdf_hip(taskName::String, X::Vector{Vector{Float64}}, IEN::Vector{Vector{Int64}},
                     rho::Vector{Float64}; options::Rho2sdfOptions = Rho2sdfOptions())
    T = options.element_type
    shape_func = coords -> shape_functions(T, coords)
    mesh = Mesh(X, IEN, rho, shape_func; element_type = T)                         # :128 (flat X / IEN for the ccall)
    options.export_input_data && InputDataToVTU(mesh, taskName * "-input_data")    # :137
    sdf_grid = options.sdf_grid_setup == :manual ? interactive_sdf_grid_setup(mesh) :
               noninteractive_sdf_grid_setup(mesh)                                 # :141-145
    smooth = options.rbf_grid == :same ? 1 : 2                                     # :222
    want_raw = options.remove_artifacts && options.export_analysis                 # :177-189 analyses and exports the field before cleanup
    o = R2SOptions(options.threshold_density === nothing ? NaN : Float64(options.threshold_density), 1.1,
                   options.artifact_min_component_ratio, 1e-3, etype(T), Int32(options.rbf_interp), Int32(smooth),
                   Int32(options.remove_artifacts), Int32(-1), N_GPUS[], Int32(0), Int32(0), Int32(SIGN_NO_INNER[] ? 1 : 0),
                   Int32(want_raw), (0, 0))
    ρₙ = Vector{Float64}(undef, mesh.nnp)
    sdf_dists = pinned(Float64, sdf_grid.ngp)
    fine_sdf = pinned(Float32, ((sdf_grid.N .* smooth) .+ 1)...)
    sdf_raw = want_raw ? pinned(Float64, sdf_grid.ngp) : nothing
    info = Ref{R2SRunInfo}()
    check(ccall((:r2s_rho2sdf, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ref{R2SOptions}, Ref{R2SGrid},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float32}, Ref{R2SRunInfo}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, rho, Ref(o), Ref(R2SGrid(sdf_grid)),
                ρₙ, want_raw ? sdf_raw : C_NULL, sdf_dists, fine_sdf, info))
    element_name = string(T.name.name)
    B = round(sdf_grid.cell_size, digits = 4)
    if options.export_nodal_densities                                              # :159-162
        exportToVTU(taskName * "_nodal_densities.vtu", X, IEN, T == HEX8 ? 12 : 10, ρₙ)
    end
    if want_raw                                                                    # :177-206
        # components_before (:178): the table of the labelling the removal ran on the raw field; a local in the
        # reference too (not returned)
        print_components(last_components())
        exportSdfToVTI(taskName * "_SDF_raw_$(element_name)_B-$(B).vti", sdf_grid, sdf_raw, "distance")
        info[].n_flipped > 0 &&
            exportSdfToVTI(taskName * "_SDF_cleaned_$(element_name)_B-$(B).vti", sdf_grid, sdf_dists, "distance")
    end
    if options.export_raw_sdf                                                      # :211-219
        exportSdfToVTI(taskName * "_SDF_$(element_name)_CellSize-" * string(B) * ".vti", sdf_grid, sdf_dists, "distance")
    end
    fine_grid = fine_grid_of(sdf_grid, smooth)                                     # the point list of RBFs4Smoothing.jl:341
    Rho2sdf.export_sdf_results_with_element_type(fine_sdf, fine_grid, sdf_grid, taskName, smooth,
                                                 options.rbf_interp, T)            # :230-238
    return (fine_sdf, fine_grid, sdf_grid, sdf_dists)
end

# ---------------------------------------------------------------------------------------------------
# leaf functions
# ---------------------------------------------------------------------------------------------------
# evalDistances (src/SignedDistances/sdfOnDensityField.jl:139-486).  The reference returns (dist, xp); its only
# caller throws xp away (RhoToSDF.jl:169), and xp is 24 B/voxel of PCIe traffic: it is produced only when
# `want_xp = true` is passed (plot_projection_points_and_lines implies it), otherwise an empty 3 x 0 matrix.
function evalDistances_hip(mesh::Mesh{T}, grid::MeshGrid.Grid, points, ρₙ::Vector{Float64}, ρₜ::Float64;
                           band_factor = 1.1, want_xp::Bool = false, plot_projection_points_and_lines::Bool = false,
                           kwargs...) where {T}
    want_xp |= plot_projection_points_and_lines
    dist = pinned(Float64, grid.ngp)
    xp = want_xp ? pinned(Float64, 3, grid.ngp) : Matrix{Float64}(undef, 3, 0)
    g = Ref(R2SGrid(grid)); p = Ref(params(T; band_factor))
    check(ccall((:r2s_eval_distances, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Float64, Ref{R2SGrid},
                 Ref{R2SParams}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, ρₙ, ρₜ, g, p, dist, want_xp ? xp : C_NULL, C_NULL))
    return dist, xp
end

# Sign_Detection (src/SignedDistances/SignDetection.jl:275-283)
function Sign_Detection_hip(mesh::Mesh{T}, grid::MeshGrid.Grid, points, ρₙ::Vector{Float64}, ρₜ::Float64) where {T}
    signs = pinned(Float64, grid.ngp)
    g = Ref(R2SGrid(grid)); p = Ref(params(T))
    check(ccall((:r2s_sign_detection, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Float64, Ref{R2SGrid},
                 Ref{R2SParams}, Ptr{Float64}, Ptr{Cvoid}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, ρₙ, ρₜ, g, p, signs, C_NULL))
    return signs
end

# fused dists .* signs (src/RhoToSDF.jl:169-171)
function sdf_hip(mesh::Mesh{T}, grid::MeshGrid.Grid, ρₙ::Vector{Float64}, ρₜ::Float64; band_factor = 1.1) where {T}
    sdf = pinned(Float64, grid.ngp)
    g = Ref(R2SGrid(grid)); p = Ref(params(T; band_factor))
    check(ccall((:r2s_sdf, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Float64, Ref{R2SGrid},
                 Ref{R2SParams}, Ptr{Float64}, Ptr{Cvoid}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, ρₙ, ρₜ, g, p, sdf, C_NULL))
    return sdf
end

# calculate_mesh_volume (src/MeshGrid/MeshVolume.jl:4-42) -> [V_domain, V_frac]
function calculate_mesh_volume_hip(X::Matrix{Float64}, IEN::Matrix{Int64}, rho::Vector{Float64}, ::Type{T}) where {T}
    vd = Ref{Float64}(0.0); vf = Ref{Float64}(0.0)
    check(ccall((:r2s_mesh_volume, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Int32, Ref{Float64}, Ref{Float64}),
                X, size(X, 2), IEN, size(IEN, 2), etype(T), rho, Int32(-1), vd, vf))
    return [vd[], vf[]]
end

# DenseInNodes (src/MeshGrid/NodalDensities.jl:89-108)
function DenseInNodes_hip(mesh::Mesh{T}, rho::Vector{Float64}) where {T}
    length(rho) == mesh.nel || error("length of element densities does not match number of elements")
    ρₙ = Vector{Float64}(undef, mesh.nnp)
    check(ccall((:r2s_dense_in_nodes, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Int32, Ptr{Float64}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, etype(T), rho, Int32(-1), ρₙ))
    return ρₙ
end

# find_threshold_for_volume(mesh, nodal_values, tolerance = 1e-4, max_iterations = 60)
# (src/MeshGrid/Isocontour_volume.jl:77-80: positional, like the reference).  TET4 meshes, for which the reference
# has no iso-volume, use the library's TET4 rule (include/rho2sdf_hip.h, r2s_find_threshold_et).
function find_threshold_for_volume_hip(mesh::Mesh{T}, ρₙ::Vector{Float64}, tolerance::Float64 = 1e-4,
                                       max_iterations::Int = 60) where {T}
    ρₜ = Ref{Float64}(0.0); its = Ref{Int32}(0)
    check(ccall((:r2s_find_threshold_et, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Float64, Float64, Int32, Int32,
                 Ref{Float64}, Ref{Int32}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, etype(T), ρₙ, mesh.V_domain * mesh.V_frac, tolerance,
                Int32(max_iterations), Int32(-1), ρₜ, its))
    return ρₜ[]
end

# calculate_isocontour_volume(mesh, nodal_values, iso_threshold) (src/MeshGrid/Isocontour_volume.jl:1-75)
function calculate_isocontour_volume_hip(mesh::Mesh{T}, ρₙ::Vector{Float64}, iso_threshold::Float64) where {T}
    v = Ref{Float64}(0.0)
    check(ccall((:r2s_isocontour_volume, LIB[]), Cint,
                (Ptr{Float64}, Int64, Ptr{Int64}, Int64, Int32, Ptr{Float64}, Float64, Int32, Ref{Float64}),
                mesh.X, mesh.nnp, mesh.IEN, mesh.nel, etype(T), ρₙ, iso_threshold, Int32(-1), v))
    return v[]
end

# remove_sdf_artifacts! (src/SignedDistances/SdfArtifactRemoval.jl:134-245) -> nodes flipped
function remove_sdf_artifacts_hip!(sdf::Vector{Float64}, grid::MeshGrid.Grid; threshold = 0.0,
                                   min_component_ratio = 0.01)
    length(sdf) == grid.ngp || error("SDF values length ($(length(sdf))) doesn't match grid points ($(grid.ngp))")   # :141-143
    n = Ref{Int64}(0)
    check(ccall((:r2s_remove_artifacts, LIB[]), Cint,
                (Ptr{Float64}, Ref{R2SGrid}, Float64, Float64, Int32, Ref{Int64}),
                sdf, Ref(R2SGrid(grid)), threshold, min_component_ratio, Int32(-1), n))
    return n[]
end

# analyze_sdf_components (src/SignedDistances/SdfArtifactRemoval.jl:256-311) -> Dict{Int,Int}, printing the summary of
# :297-308.  Keys are the Julia linear index of each component's FIRST voxel (root + 1): the reference keys a component
# by its union-find root (union by rank, :41-60), which depends on the union order.  Partition and sizes are the same.
# The field is only read.
function analyze_sdf_components_hip(sdf::Vector{Float64}, grid::MeshGrid.Grid; threshold = 0.0)
    length(sdf) == grid.ngp || error("SDF values length ($(length(sdf))) doesn't match grid points ($(grid.ngp))")
    n = Ref{Int64}(0)
    check(ccall((:r2s_analyze_components, LIB[]), Cint,
                (Ptr{Float64}, Ref{R2SGrid}, Float64, Int32, Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}),
                sdf, Ref(R2SGrid(grid)), Float64(threshold), Int32(-1), C_NULL, C_NULL, 0, n))
    comps = last_components()
    print_components(comps)
    return comps
end

# the calling thread's last component table (count first, then copy: no second labelling) as root + 1 => size
function last_components()
    n = Ref{Int64}(0)
    check(ccall((:r2s_last_components, LIB[]), Cint, (Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}), C_NULL, C_NULL, 0, n))
    roots = Vector{Int64}(undef, n[]); sizes = Vector{Int64}(undef, n[])
    n[] > 0 && check(ccall((:r2s_last_components, LIB[]), Cint, (Ptr{Int64}, Ptr{Int64}, Int64, Ref{Int64}),
                           roots, sizes, n[], n))
    return Dict{Int,Int}(r + 1 => s for (r, s) in zip(roots, sizes))
end

function print_components(comps::Dict{Int,Int})                                   # :263-266, :297-308
    if isempty(comps)
        println("No interior nodes found")
        return
    end
    sizes = sort!(collect(values(comps)), rev = true)
    println("Component analysis results:")
    println("  Total components: $(length(sizes))")
    println("  Largest component: $(sizes[1]) nodes")
    if length(sizes) > 1
        println("  Second largest: $(sizes[2]) nodes")
        println("  Smallest component: $(sizes[end]) nodes")
    end
end

# The geometry of a result (no counterpart in the reference, whose only view of it is Makie's contour!(sdf, levels=[0]) in
# src/Visualizations/VisualizeIsosurface.jl): the watertight triangle mesh of {values >= iso} on the lattice
# exportSdfToVTI writes for (grid, smooth) - smooth = nothing: N+1 points, cell_size; so the mesh overlays the .vti.
# values: fine_sdf (Float32) or sdf_dists / the raw field (Float64, N+1 points per axis).  Returns (3 x nv Float32,
# 3 x nt Int32, 1-based); normals (v2-v1)x(v3-v1) point from the interior to the exterior.  Bit-identical to the surface
# r2s_rho2sdf keeps with its extract_surface option (which this binding's rho2sdf_hip leaves off: reserved = (0, 0)).
function extract_isosurface_hip(values::AbstractArray{T}, grid::MeshGrid.Grid, smooth::Union{Int,Nothing} = nothing;
                                iso = 0.0f0) where {T<:Union{Float32,Float64}}
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    length(values) == prod(dims) || error("values length ($(length(values))) doesn't match the lattice $(Tuple(dims))")
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    nv = Ref{Int64}(0); nt = Ref{Int64}(0)
    check(ccall((:r2s_extract_isosurface, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Float64, Float64, Int32, Ptr{Float32}, Int64, Ptr{Int32}, Int64,
                 Ref{Int64}, Ref{Int64}),
                values, Int32(T == Float32), collect(dims), collect(Float64.(grid.AABB_min)), spacing, Float64(iso), Int32(-1),
                C_NULL, 0, C_NULL, 0, nv, nt))
    verts = Matrix{Float32}(undef, 3, nv[]); tris = Matrix{Int32}(undef, 3, nt[])
    check(ccall((:r2s_last_isosurface, LIB[]), Cint, (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Ref{Int64}, Ref{Int64}),
                verts, nv[], tris, nt[], nv, nt))
    tris .+= Int32(1)
    return verts, tris
end

# binary STL of (3 x nv Float32, 3 x nt 1-based) as extract_isosurface_hip returns them; ".stl" appended when missing
function export_stl_hip(filename::AbstractString, verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer})
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    check(ccall((:r2s_export_stl, LIB[]), Cint, (Cstring, Ptr{Float32}, Int64, Ptr{Int32}, Int64),
                filename, Matrix(verts), size(verts, 2), t0, size(t0, 2)))
    return endswith(filename, ".stl") ? String(filename) : filename * ".stl"
end

# Redistancing (no counterpart in the reference): the exact Euclidean distance from every lattice point to a triangle mesh,
# clamped to `band` (include/rho2sdf_hip.h, r2s_mesh_distance).  verts 3 x nv Float32, tris 3 x nt 1-based, as
# extract_isosurface_hip returns them; the lattice is the one of extract_isosurface_hip for (grid, smooth).  Returns the
# Float64 distances (x fastest) and, with want_index, the 1-based index of the closest triangle (0 where the result is band).
function mesh_distance_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}, grid::MeshGrid.Grid, band::Real,
                           smooth::Union{Int,Nothing} = nothing; want_index::Bool = false)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    t0 = Int32.(tris) .- Int32(1)
    dist = Array{Float64,3}(undef, dims...)
    idx = want_index ? Array{Int32,3}(undef, dims...) : nothing
    check(ccall((:r2s_mesh_distance, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Float64}, Float64, Float64, Int32, Int32, Ptr{Cvoid},
                 Ptr{Int32}),
                Matrix(verts), size(verts, 2), t0, size(t0, 2), collect(dims), collect(Float64.(grid.AABB_min)), spacing,
                Float64(band), Int32(0), Int32(-1), dist, want_index ? idx : C_NULL))
    want_index || return dist
    idx .+= Int32(1)
    return dist, idx
end

# The banded signed distance to the iso-surface of `values` (r2s_redistance): s * min(d, band), s = +1 where values >= iso
# and -1 elsewhere, d the exact distance to the mesh extract_isosurface_hip returns for the same arguments; same type and
# shape conventions as extract_isosurface_hip.  redistance_hip(fine_sdf, sdf_grid, smooth; band = k * spacing) turns the
# smoothed field of rho2sdf_hip into a distance function k cells wide.
function redistance_hip(values::AbstractArray{T}, grid::MeshGrid.Grid, smooth::Union{Int,Nothing} = nothing;
                        iso = 0.0, band::Real) where {T<:Union{Float32,Float64}}
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    length(values) == prod(dims) || error("values length ($(length(values))) doesn't match the lattice $(Tuple(dims))")
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    out = Array{T,3}(undef, dims...)
    check(ccall((:r2s_redistance, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Float64, Float64, Float64, Int32, Ptr{Cvoid}),
                values, Int32(T == Float32), collect(dims), collect(Float64.(grid.AABB_min)), spacing, Float64(iso),
                Float64(band), Int32(-1), out))
    return out
end

# Mesh index (no counterpart in the reference): a bounding-volume hierarchy over a triangle mesh on the device and exact
# point-to-mesh distances without a band (include/rho2sdf_hip.h, r2s_mesh_index).  verts 3 x nv Float32, tris 3 x nt 1-based.
# The index owns device memory: close it with destroy!(index) (release!() leaves it alone).
mutable struct MeshIndexHIP
    handle::Ptr{Cvoid}
end

function mesh_index_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:r2s_mesh_index_build, LIB[]), Cint, (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Ptr{Ptr{Cvoid}}),
                Matrix(verts), size(verts, 2), t0, size(t0, 2), Int32(device), h))
    return finalizer(destroy!, MeshIndexHIP(h[]))
end

function destroy!(ix::MeshIndexHIP)
    ix.handle == C_NULL || ccall((:r2s_mesh_index_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), ix.handle)
    ix.handle = C_NULL
    return nothing
end

# (n_tris, nodes, tree depth, device bytes)
function mesh_index_info(ix::MeshIndexHIP)
    out = zeros(Int64, 4)
    check(ccall((:r2s_mesh_index_info, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}), ix.handle, out))
    return (n_tris = out[1], nodes = out[2], depth = out[3], device_bytes = out[4])
end

# distances of the points (3 x n, Float32 or Float64) to the mesh -> Vector{Float64}; want_index: also the 1-based index of the
# closest triangle (0 for an empty mesh or a non-finite point, whose distance is Inf / NaN)
function mesh_index_distance(ix::MeshIndexHIP, points::AbstractMatrix{T}; want_index::Bool = false) where {T<:Union{Float32,Float64}}
    size(points, 1) == 3 || error("points must be 3 x n")
    n = size(points, 2)
    dist = Vector{Float64}(undef, n)
    idx = want_index ? Vector{Int32}(undef, n) : nothing
    check(ccall((:r2s_mesh_index_query, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Cvoid}, Ptr{Int32}),
                ix.handle, Matrix(points), Int32(T == Float32), n, Int32(0), dist, want_index ? idx : C_NULL))
    want_index || return dist
    idx .+= Int32(1)
    return dist, idx
end

# the same on every point of the lattice of extract_isosurface_hip for (grid, smooth) -> Array{Float64,3} (x fastest)
function mesh_index_lattice(ix::MeshIndexHIP, grid::MeshGrid.Grid, smooth::Union{Int,Nothing} = nothing; want_index::Bool = false)
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    dist = Array{Float64,3}(undef, dims...)
    idx = want_index ? Array{Int32,3}(undef, dims...) : nothing
    check(ccall((:r2s_mesh_index_lattice, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Float64, Int32, Ptr{Cvoid}, Ptr{Int32}),
                ix.handle, collect(dims), collect(Float64.(grid.AABB_min)), spacing, Int32(0), dist, want_index ? idx : C_NULL))
    want_index || return dist
    idx .+= Int32(1)
    return dist, idx
end

# first hit of the rays origins + t * dirs (both 3 x n, Float32 or Float64; dirs are not normalised) with t_min <= t <= t_max
# (include/rho2sdf_hip.h, r2s_mesh_index_raycast) -> (t, tri, side): t Vector{Float64} (Inf = miss, NaN = a bad ray), tri the
# 1-based index of the triangle hit (0 = none), side Int8 (+1 the ray enters through the front of the winding, -1 through the
# back, 0 = miss)
function mesh_raycast_hip(ix::MeshIndexHIP, origins::AbstractMatrix{T}, dirs::AbstractMatrix{T}; t_min::Real = 0.0,
                          t_max::Real = Inf) where {T<:Union{Float32,Float64}}
    size(origins, 1) == 3 && size(origins) == size(dirs) || error("origins and dirs must both be 3 x n")
    n = size(origins, 2)
    t = Vector{Float64}(undef, n)
    tri = Vector{Int32}(undef, n)
    side = Vector{Int8}(undef, n)
    check(ccall((:r2s_mesh_index_raycast, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Float64, Float64, Int32, Ptr{Cvoid}, Ptr{Int32}, Ptr{Int8}),
                ix.handle, Matrix(origins), Matrix(dirs), Int32(T == Float32), n, Float64(t_min), Float64(t_max), Int32(0), t, tri, side))
    tri .+= Int32(1)
    return t, tri, side
end

# The shells of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_shells): verts 3 x nv Float32, tris 3 x nt 1-based ->
# (shell_of_tri (1-based shell number, 0 = collapsed triangle), counts 8 x n Int64 with first_tri 1-based, sums 11 x n Float64,
# ref_point, totals)
function mesh_shells_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    shell = Vector{Int32}(undef, size(t0, 2))
    n = Ref{Int64}(0)
    ref = zeros(Float64, 3)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_shells, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                Matrix(verts), size(verts, 2), t0, size(t0, 2), Int32(device), shell, n, ref, totals))
    counts, sums = last_mesh_shells_hip(n[])
    shell .+= Int32(1)
    return (shell_of_tri = shell, counts = counts, sums = sums, ref_point = ref, totals = totals)
end

# the calling thread's last shell tables (r2s_last_mesh_shells): counts 8 x n (first_tri made 1-based), sums 11 x n
function last_mesh_shells_hip(capacity::Integer)
    counts = Matrix{Int64}(undef, 8, capacity)
    sums = Matrix{Float64}(undef, 11, capacity)
    n = Ref{Int64}(0)
    check(ccall((:r2s_last_mesh_shells, LIB[]), Cint, (Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
                capacity == 0 ? C_NULL : counts, capacity == 0 ? C_NULL : sums, Int64(capacity), n))
    counts[1, :] .+= 1
    return counts, sums
end

# the same on device arrays of the current device (raw pointers, e.g. of AMDGPU.jl ROCArrays); the tables are written only when
# shell_capacity holds all shells -> (n_shells, ref_point, totals); indices stay 0-based on the device
function mesh_shells_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer, d_shell_of_tri::Ptr{Cvoid},
                             d_counts::Ptr{Cvoid}, d_sums::Ptr{Cvoid}, shell_capacity::Integer; stream::Ptr{Cvoid} = C_NULL)
    n = Ref{Int64}(0)
    ref = zeros(Float64, 3)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_shells_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64},
                 Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), d_shell_of_tri, d_counts, d_sums, Int64(shell_capacity), n, ref, totals,
                stream))
    return n[], ref, totals
end

# The sections of a triangle mesh with the planes normal . x = levels[k] (include/rho2sdf_hip.h, r2s_mesh_sections): verts
# 3 x nv Float32, tris 3 x nt 1-based, levels ascending -> (contour_start (1-based output positions, n + 1 entries), counts 8 x n
# Int64 with level, first segment and nothing else made 1-based, sums 7 x n Float64, seg_tri (1-based), seg_points 3 x 2 x m
# (from, to), ref_point, totals)
function mesh_sections_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}, normal::AbstractVector{<:Real},
                           levels::AbstractVector{<:Real}; device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 && length(normal) == 3 || error("verts and tris must be 3 x n, normal of length 3")
    t0 = Int32.(tris) .- Int32(1)
    nrm, lev = Vector{Float64}(normal), Vector{Float64}(levels)
    nc, ns = Ref{Int64}(0), Ref{Int64}(0)
    ref = zeros(Float64, 3)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_sections, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
                 Ptr{Int64}),
                Matrix(verts), size(verts, 2), t0, size(t0, 2), nrm, isempty(lev) ? C_NULL : lev, length(lev), Int32(device), nc, ns, ref,
                totals))
    tables = last_mesh_sections_hip(nc[], ns[])
    return (; tables..., ref_point = ref, totals = totals)
end

# the calling thread's last section tables (r2s_last_mesh_sections), indices made 1-based
function last_mesh_sections_hip(contour_capacity::Integer, segment_capacity::Integer)
    start = zeros(Int64, contour_capacity + 1)
    counts = Matrix{Int64}(undef, 8, contour_capacity)
    sums = Matrix{Float64}(undef, 7, contour_capacity)
    seg_tri = Vector{Int32}(undef, segment_capacity)
    pts = Array{Float64,3}(undef, 3, 2, segment_capacity)
    nc, ns = Ref{Int64}(0), Ref{Int64}(0)
    none = contour_capacity == 0
    check(ccall((:r2s_last_mesh_sections, LIB[]), Cint,
                (Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int32}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}),
                none ? C_NULL : start, none ? C_NULL : counts, none ? C_NULL : sums, Int64(contour_capacity),
                segment_capacity == 0 ? C_NULL : seg_tri, segment_capacity == 0 ? C_NULL : pts, Int64(segment_capacity), nc, ns))
    start .+= 1
    counts[1:2, :] .+= 1
    seg_tri .+= Int32(1)
    return (contour_start = start, counts = counts, sums = sums, seg_tri = seg_tri, seg_points = pts)
end

# the same on device arrays of the current device (raw pointers, e.g. of AMDGPU.jl ROCArrays; normal and levels are host
# vectors); the tables are written only when both capacities hold everything -> (n_contours, n_segments, ref_point, totals);
# indices stay 0-based on the device
function mesh_sections_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer,
                               normal::AbstractVector{<:Real}, levels::AbstractVector{<:Real}, d_contour_start::Ptr{Cvoid},
                               d_counts::Ptr{Cvoid}, d_sums::Ptr{Cvoid}, contour_capacity::Integer, d_seg_tri::Ptr{Cvoid},
                               d_seg_points::Ptr{Cvoid}, segment_capacity::Integer; stream::Ptr{Cvoid} = C_NULL)
    nrm, lev = Vector{Float64}(normal), Vector{Float64}(levels)
    nc, ns = Ref{Int64}(0), Ref{Int64}(0)
    ref = zeros(Float64, 3)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_sections_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64,
                 Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), nrm, isempty(lev) ? C_NULL : lev, length(lev), d_contour_start, d_counts,
                d_sums, Int64(contour_capacity), d_seg_tri, d_seg_points, Int64(segment_capacity), nc, ns, ref, totals, stream))
    return nc[], ns[], ref, totals
end

# Welds the vertices of a triangle mesh that are the same point (include/rho2sdf_hip.h, r2s_mesh_weld): verts 3 x nv Float32, tris
# 3 x nt 1-based or `nothing` for a triangle soup (triangle t = columns 3t-2, 3t-1, 3t).  snap = 0: the same iff x, y, z compare
# equal as Float32; snap > 0: iff they fall into the same cell floor(v / snap) per axis - grid snapping, not a distance tolerance.
# -> (verts 3 x nv_out, every column an input vertex bit for bit in first-occurrence order, tris 3 x nt_out 1-based, vert_map and
# tri_map 1-based with 0 for what was dropped, totals).  The mesh of extract_isosurface_hip is closed without welding; welding its
# exact-iso vertices collapses zero-area triangles and can leave non-manifold edges, which mesh_shells_hip reports, and pinched
# vertices, which only mesh_fans_hip reports (and splits): offered, not applied by default.
function mesh_weld_hip(verts::AbstractMatrix{Float32}, tris::Union{Nothing,AbstractMatrix{<:Integer}} = nothing; snap::Real = 0.0,
                       drop_collapsed::Bool = true, drop_duplicates::Bool = false, drop_unused::Bool = true, device::Integer = -1)
    size(verts, 1) == 3 && (tris === nothing ? size(verts, 2) % 3 == 0 : size(tris, 1) == 3) ||
        error("verts and tris must be 3 x n (a soup: a multiple of 3 vertices)")
    nv = size(verts, 2)
    t0 = tris === nothing ? nothing : Int32.(tris) .- Int32(1)
    nt = tris === nothing ? div(nv, 3) : size(t0, 2)
    flags = Int32((drop_collapsed ? 1 : 0) | (drop_duplicates ? 2 : 0) | (drop_unused ? 4 : 0))
    vout = Matrix{Float32}(undef, 3, nv); tout = Matrix{Int32}(undef, 3, nt)
    vmap = Vector{Int32}(undef, nv); tmap = Vector{Int32}(undef, nt)
    totals = zeros(Int64, 8)
    pad = zeros(Int32, 3)                 # a mesh without triangles passes a non-NULL tris: NULL means soup
    check(ccall((:r2s_mesh_weld, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Float64, Int32, Int32, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                 Ptr{Int64}),
                Matrix(verts), nv, t0 === nothing ? C_NULL : (nt == 0 ? pad : t0), nt, Float64(snap), flags, Int32(device), vout, tout,
                vmap, tmap, totals))
    return (verts = vout[:, 1:totals[1]], tris = tout[:, 1:totals[2]] .+ Int32(1), vert_map = vmap .+ Int32(1),
            tri_map = tmap .+ Int32(1), totals = totals)
end

# the same on device arrays of the current device (raw pointers; d_tris == C_NULL: the soup, n_tris = n_verts / 3); the outputs are
# sized to the input counts, the maps may be C_NULL -> totals; indices stay 0-based on the device
function mesh_weld_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer, d_verts_out::Ptr{Cvoid},
                           d_tris_out::Ptr{Cvoid}, d_vert_map::Ptr{Cvoid}, d_tri_map::Ptr{Cvoid}; snap::Real = 0.0,
                           flags::Integer = 5, stream::Ptr{Cvoid} = C_NULL)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_weld_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64},
                 Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), Float64(snap), Int32(flags), d_verts_out, d_tris_out, d_vert_map,
                d_tri_map, totals, stream))
    return totals
end

# Vertex-clustering decimation of an indexed triangle mesh (include/rho2sdf_hip.h, r2s_mesh_simplify): verts 3 x nv Float32, tris
# 3 x nt 1-based, cell > 0.  The clusters are the cells of mesh_weld_hip(snap = cell); rule :mean puts each at the Float64 mean
# of its members, :quadric at the point of the cell that minimises the summed plane quadrics of the triangles around it.
# -> (verts 3 x nv_out, tris 3 x nt_out 1-based, vert_map and tri_map 1-based with 0 for what was dropped, members, error, solved
# per output vertex, totals).  Clustering does not preserve manifoldness: check with mesh_shells_hip / mesh_fans_hip /
# mesh_intersections_hip.  Not here: edge collapse, boundary or feature constraints, attribute transfer.
function mesh_simplify_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}, cell::Real; rule::Symbol = :quadric,
                           drop_duplicates::Bool = true, device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    rule in (:mean, :quadric) || error("rule must be :mean or :quadric")
    nv = size(verts, 2)
    t0 = Int32.(tris) .- Int32(1)
    nt = size(t0, 2)
    vout = Matrix{Float32}(undef, 3, nv); tout = Matrix{Int32}(undef, 3, nt)
    vmap = Vector{Int32}(undef, nv); tmap = Vector{Int32}(undef, nt)
    totals = zeros(Int64, 8)
    pad = zeros(Int32, 3)                 # a mesh without triangles still passes a non-NULL tris
    check(ccall((:r2s_mesh_simplify, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Float64, Int32, Int32, Int32, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                 Ptr{Int64}),
                Matrix(verts), nv, nt == 0 ? pad : t0, nt, Float64(cell), Int32(rule == :mean ? 0 : 1), Int32(drop_duplicates ? 2 : 0),
                Int32(device), vout, tout, vmap, tmap, totals))
    members, err, solved = last_mesh_simplify_hip()
    return (verts = vout[:, 1:totals[1]], tris = tout[:, 1:totals[2]] .+ Int32(1), vert_map = vmap .+ Int32(1),
            tri_map = tmap .+ Int32(1), members = members, error = err, solved = solved, totals = totals)
end

# the per-vertex tables of the calling thread's last mesh_simplify_hip / mesh_simplify_dev_hip -> (members, error, solved)
function last_mesh_simplify_hip()
    n = Ref{Int64}(0)
    check(ccall((:r2s_last_mesh_simplify, LIB[]), Cint, (Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Int64}),
                C_NULL, C_NULL, C_NULL, 0, n))
    members = Vector{Int64}(undef, n[]); err = Vector{Float64}(undef, n[]); solved = Vector{Int32}(undef, n[])
    check(ccall((:r2s_last_mesh_simplify, LIB[]), Cint, (Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Int64}),
                members, err, solved, n[], n))
    return members, err, solved
end

# the same on device arrays of the current device (raw pointers); the outputs are sized to the input counts, the maps may be
# C_NULL -> totals; indices stay 0-based on the device; the tables are read with last_mesh_simplify_hip()
function mesh_simplify_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer, cell::Real,
                               d_verts_out::Ptr{Cvoid}, d_tris_out::Ptr{Cvoid}, d_vert_map::Ptr{Cvoid}, d_tri_map::Ptr{Cvoid};
                               rule::Integer = 1, flags::Integer = 2, stream::Ptr{Cvoid} = C_NULL)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_simplify_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Float64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64},
                 Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), Float64(cell), Int32(rule), Int32(flags), d_verts_out, d_tris_out,
                d_vert_map, d_tri_map, totals, stream))
    return totals
end

mutable struct R2SStlMesh              # mirrors r2s_stl_mesh
    n_tris::Int64
    verts::Ptr{Float32}
end

# A consistent winding for a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_orient): verts 3 x nv Float32, tris 3 x nt 1-based.
# The mesh falls into patches over the edges that exactly two triangles share; inside an orientable patch every triangle gets
# the winding of its neighbours, and the patch as a whole
#     outward = true, the patch closed with a volume V != 0:   is wound so that V > 0 ("decided by volume")
#     otherwise (and always with outward = false):              keeps the winding of the MAJORITY of its triangles, on a tie
#                                                               that of its first triangle
# A flipped triangle (i0, i1, i2) comes back as (i0, i2, i1).  Nesting is ignored: outward = true turns an enclosed void into a
# body, the majority rule leaves a void as most of its triangles say.  Non-orientable patches are copied unchanged and counted;
# no orientation is carried across non-manifold edges; no holes are filled.
# -> (tris 3 x nt 1-based, flipped (Bool), patch_of_tri (1-based patch number, 0 = collapsed triangle), counts 8 x n Int64
# (first_tri 1-based, n_tris, flipped triangles, status bits 1 closed / 2 non-orientable / 4 decided by volume, boundary and
# non-manifold half-edges, flipped edges of the input, 0), volume (n, as written, about ref_point), ref_point, totals)
const ORIENT_OUTWARD = Int32(1)
function mesh_orient_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; outward::Bool = false, device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    nt = size(t0, 2)
    tout = Matrix{Int32}(undef, 3, nt)
    flip = Vector{Int32}(undef, nt); patch = Vector{Int32}(undef, nt)
    n = Ref{Int64}(0)
    ref = zeros(Float64, 3)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_orient, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64},
                 Ptr{Int64}),
                Matrix(verts), size(verts, 2), t0, nt, outward ? ORIENT_OUTWARD : Int32(0), Int32(device), tout, flip, patch, n, ref,
                totals))
    counts, volume = last_mesh_orient_hip(n[])
    return (tris = tout .+ Int32(1), flipped = flip .!= 0, patch_of_tri = patch .+ Int32(1), counts = counts, volume = volume,
            ref_point = ref, totals = totals)
end

# the calling thread's last orient tables (r2s_last_mesh_orient): counts 8 x n (first_tri made 1-based), volume n
function last_mesh_orient_hip(capacity::Integer)
    counts = Matrix{Int64}(undef, 8, capacity)
    volume = Vector{Float64}(undef, capacity)
    n = Ref{Int64}(0)
    check(ccall((:r2s_last_mesh_orient, LIB[]), Cint, (Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
                capacity == 0 ? C_NULL : counts, capacity == 0 ? C_NULL : volume, Int64(capacity), n))
    counts[1, :] .+= 1
    return counts, volume
end

# the same on device arrays of the current device (raw pointers, e.g. of AMDGPU.jl ROCArrays); d_tris_out must not overlap d_tris,
# d_flip and d_patch_of_tri may be C_NULL; the triangles, flips and labels are always written, the tables only when
# patch_capacity holds all patches -> (n_patches, ref_point, totals); indices stay 0-based on the device
function mesh_orient_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer, d_tris_out::Ptr{Cvoid},
                             d_flip::Ptr{Cvoid}, d_patch_of_tri::Ptr{Cvoid}, d_counts::Ptr{Cvoid}, d_volume::Ptr{Cvoid},
                             patch_capacity::Integer; outward::Bool = false, stream::Ptr{Cvoid} = C_NULL)
    n = Ref{Int64}(0)
    ref = zeros(Float64, 3)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_orient_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64,
                 Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), outward ? ORIENT_OUTWARD : Int32(0), d_tris_out, d_flip, d_patch_of_tri,
                d_counts, d_volume, Int64(patch_capacity), n, ref, totals, stream))
    return n[], ref, totals
end

# Which closed patch encloses which (include/rho2sdf_hip.h, r2s_mesh_nesting): verts 3 x nv Float32, tris 3 x nt 1-based.  The
# patches are those of mesh_orient_hip; a closed patch Q contains a patch P when the axis ray `ray` (0..5: +x +y +z -x -y -z) from
# P's sample vertex crosses Q an odd number of times.  depth = the number of containers, parent = the deepest of them; closed
# patches at even depth are bodies, at odd depth voids.  rewind = true: tris comes back with the voids reversed relative to the
# input (after mesh_orient_hip(outward = true): bodies positive, voids negative); otherwise tris is nothing.
# -> (tris 3 x nt 1-based or nothing, patch_of_tri (1-based, 0 = collapsed triangle), counts 8 x n Int64 (first_tri 1-based, n_tris,
# status bits 1 closed / 2 reversed / 4 irregular, parent 1-based (0 = none), depth, n_children, sum of crossings, 0), pairs
# (query, container) 2 x m 1-based, ascending, totals)
const NESTING_REWIND = Int32(1)
function mesh_nesting_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; ray::Integer = 2, rewind::Bool = false,
                          device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    nt = size(t0, 2)
    tout = Matrix{Int32}(undef, 3, rewind ? nt : 0)
    patch = Vector{Int32}(undef, nt)
    n = Ref{Int64}(0)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_nesting, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int64}),
                Matrix(verts), size(verts, 2), t0, nt, Int32(ray), rewind ? NESTING_REWIND : Int32(0), Int32(device),
                rewind ? tout : Ptr{Int32}(C_NULL), patch, n, totals))
    counts, pairs = last_mesh_nesting_hip()
    return (tris = rewind ? tout .+ Int32(1) : nothing, patch_of_tri = patch .+ Int32(1), counts = counts, pairs = pairs, totals = totals)
end

# the calling thread's last nesting tables (r2s_last_mesh_nesting): counts 8 x n (first_tri and parent made 1-based), pairs 2 x m
function last_mesh_nesting_hip()
    n = Ref{Int64}(0); m = Ref{Int64}(0)
    check(ccall((:r2s_last_mesh_nesting, LIB[]), Cint, (Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}),
                Ptr{Int64}(C_NULL), Int64(0), Ptr{Int64}(C_NULL), Int64(0), n, m))
    counts = Matrix{Int64}(undef, 8, n[])
    keys = Vector{Int64}(undef, m[])
    check(ccall((:r2s_last_mesh_nesting, LIB[]), Cint, (Ptr{Int64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}),
                n[] == 0 ? Ptr{Int64}(C_NULL) : pointer(counts), n[], m[] == 0 ? Ptr{Int64}(C_NULL) : pointer(keys), m[], n, m))
    counts[1, :] .+= 1
    counts[4, :] .+= 1
    pairs = Matrix{Int64}(undef, 2, length(keys))
    pairs[1, :] .= (keys .>> 32) .+ 1
    pairs[2, :] .= (keys .& 0xffffffff) .+ 1
    return counts, pairs
end

# the same on device arrays of the current device (raw pointers); index: the handle of a mesh index of the same mesh on that device
# or C_NULL (a tree is built and dropped).  d_tris_out is needed with rewind only and must not overlap d_tris, d_patch_of_tri may be
# C_NULL; the records and the pairs ((P << 32) | Q, 0-based) are written only when their capacity holds all of them
# -> (n_patches, n_pairs, totals); indices stay 0-based on the device
function mesh_nesting_dev_hip(index::Ptr{Cvoid}, d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer,
                              d_tris_out::Ptr{Cvoid}, d_patch_of_tri::Ptr{Cvoid}, d_counts::Ptr{Cvoid}, patch_capacity::Integer,
                              d_pairs::Ptr{Cvoid}, pair_capacity::Integer; ray::Integer = 2, rewind::Bool = false,
                              stream::Ptr{Cvoid} = C_NULL)
    n = Ref{Int64}(0); m = Ref{Int64}(0)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_nesting_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid},
                 Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid}),
                index, d_verts, Int64(n_verts), d_tris, Int64(n_tris), Int32(ray), rewind ? NESTING_REWIND : Int32(0), d_tris_out,
                d_patch_of_tri, d_counts, Int64(patch_capacity), d_pairs, Int64(pair_capacity), n, m, totals, stream))
    return n[], m[], totals
end

# The fans of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_fans): verts 3 x nv Float32, tris 3 x nt 1-based.  The corners of
# every vertex fall into fans, connected over the edges their triangles share at that vertex; a vertex with two or more fans is
# pinched (non-manifold, although every edge may be regular), which mesh_shells_hip cannot see.  split = true also returns the
# repaired mesh: the first fan of a vertex keeps its index, every further fan gets a copy of the vertex appended behind the input
# vertices; fans on a non-manifold edge (complex) are reported, not repaired.
# -> (fan_of_corner 3 x nt (1-based fan number, 0 = collapsed triangle), fans_of_vert (0 unused, 1 ordinary, >= 2 pinched),
# counts 8 x n Int64 (vertex and first_corner 1-based, n_corners, n_edges, boundary, flipped, non-manifold edges, class 0 closed /
# 1 open / 2 complex), totals (fans, triangles, collapsed, used, unused, pinched vertices, complex fans, open fans) and, with
# split, verts 3 x nv_out, tris 3 x nt 1-based, vert_of (1-based source vertex))
function mesh_fans_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; split::Bool = false, device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    nv = size(verts, 2); nt = size(t0, 2)
    foc = Matrix{Int32}(undef, 3, nt); fov = Vector{Int32}(undef, nv)
    n = Ref{Int64}(0); nvo = Ref{Int64}(0)
    totals = zeros(Int64, 8)
    cap = split ? nv + 1024 : 0
    tout = Matrix{Int32}(undef, 3, nt)
    while true
        vout = Matrix{Float32}(undef, 3, max(cap, 1)); vof = Vector{Int32}(undef, max(cap, 1))
        check(ccall((:r2s_mesh_fans, LIB[]), Cint,
                    (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Int64,
                     Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                    Matrix(verts), nv, t0, nt, Int32(device), foc, fov, split ? tout : C_NULL, split ? vout : C_NULL,
                    split ? vof : C_NULL, Int64(cap), n, nvo, totals))
        if !split || nvo[] <= cap
            counts = last_mesh_fans_hip(n[])
            base = (fan_of_corner = foc .+ Int32(1), fans_of_vert = fov, counts = counts, totals = totals)
            return split ? merge(base, (verts = vout[:, 1:nvo[]], tris = tout .+ Int32(1), vert_of = vof[1:nvo[]] .+ Int32(1))) : base
        end
        cap = nvo[]
    end
end

# the calling thread's last fan records (r2s_last_mesh_fans): counts 8 x n (vertex and first_corner made 1-based)
function last_mesh_fans_hip(capacity::Integer)
    counts = Matrix{Int64}(undef, 8, capacity)
    n = Ref{Int64}(0)
    check(ccall((:r2s_last_mesh_fans, LIB[]), Cint, (Ptr{Int64}, Int64, Ptr{Int64}),
                capacity == 0 ? C_NULL : counts, Int64(capacity), n))
    counts[1:2, :] .+= 1
    return counts
end

# the same on device arrays of the current device (raw pointers, e.g. of AMDGPU.jl ROCArrays); d_fan_of_corner and d_fans_of_vert
# may be C_NULL; the records are written only when fan_capacity holds all fans, the split (d_tris_out, d_verts_out, d_vert_of_out:
# all three or C_NULL) only when vert_capacity holds all output vertices -> (n_fans, n_verts_out, totals); indices stay 0-based
function mesh_fans_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer, d_fan_of_corner::Ptr{Cvoid},
                           d_fans_of_vert::Ptr{Cvoid}, d_counts::Ptr{Cvoid}, fan_capacity::Integer, d_tris_out::Ptr{Cvoid} = C_NULL,
                           d_verts_out::Ptr{Cvoid} = C_NULL, d_vert_of_out::Ptr{Cvoid} = C_NULL, vert_capacity::Integer = 0;
                           stream::Ptr{Cvoid} = C_NULL)
    n = Ref{Int64}(0); nvo = Ref{Int64}(0)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_fans_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64,
                 Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), d_fan_of_corner, d_fans_of_vert, d_counts, Int64(fan_capacity), d_tris_out,
                d_verts_out, d_vert_of_out, Int64(vert_capacity), n, nvo, totals, stream))
    return n[], nvo[], totals
end

# The rims (boundary loops and chains) of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_holes): verts 3 x nv Float32, tris
# 3 x nt 1-based.  A rim is a connected component of the boundary half-edges, closed when every vertex on it has one incoming and
# one outgoing boundary half-edge.  fill = nothing reports only; fill = -1 caps every closed rim, fill = k > 0 those of at most k
# edges (a rim of three gets one triangle, a longer one a new vertex at the mean of its vertices and a fan).  Rims that are not
# closed are never filled: weld, orient and split the pinched vertices (mesh_fans_hip) first.
# -> (rim_start (0-based offsets, n + 1), rim_edge (0-based half-edge id 3 (t - 1) + (c - 1) per output position), counts 8 x n
# Int64 (first half-edge 0-based, n_edges, n_nodes, open, flipped, branch nodes, status 0 not closed / 1 closed / 2 one triangle /
# 3 fan, added vertex 1-based or 0), sums 7 x n (length, sum A x B, sum A about ref_point), ref_point, totals (rims, boundary
# half-edges, collapsed, nodes, irregular nodes, closed rims, filled rims, added triangles) and, with a fill, verts 3 x nv_out and
# tris 3 x nt_out 1-based)
function mesh_holes_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; fill::Union{Nothing, Integer} = nothing,
                        device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    t0 = Int32.(tris) .- Int32(1)
    nv = size(verts, 2); nt = size(t0, 2)
    nr = Ref{Int64}(0); nb = Ref{Int64}(0); nvo = Ref{Int64}(0); nto = Ref{Int64}(0)
    r = zeros(Float64, 3); totals = zeros(Int64, 8)
    dofill = fill !== nothing
    vcap = dofill ? nv + 1024 : 0; tcap = dofill ? nt + 4096 : 0
    while true
        vout = Matrix{Float32}(undef, 3, max(vcap, 1)); tout = Matrix{Int32}(undef, 3, max(tcap, 1))
        check(ccall((:r2s_mesh_holes, LIB[]), Cint,
                    (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Int64, Ptr{Int32}, Ptr{Float32}, Int64, Int64, Ptr{Int64}, Ptr{Int64},
                     Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
                    Matrix(verts), nv, t0, nt, Int32(device), Int64(dofill ? fill : 0), dofill ? tout : C_NULL, dofill ? vout : C_NULL,
                    Int64(vcap), Int64(tcap), nr, nb, nvo, nto, r, totals))
        if !dofill || (nvo[] <= vcap && nto[] <= tcap)
            base = merge(last_mesh_holes_hip(nr[], nb[]), (ref_point = r, totals = totals))
            return dofill ? merge(base, (verts = vout[:, 1:nvo[]], tris = tout[:, 1:nto[]] .+ Int32(1))) : base
        end
        vcap = max(vcap, nvo[]); tcap = max(tcap, nto[])
    end
end

# the calling thread's last rim tables (r2s_last_mesh_holes); the added vertex is made 1-based (0: none)
function last_mesh_holes_hip(rim_capacity::Integer, edge_capacity::Integer)
    start = zeros(Int64, rim_capacity + 1); counts = Matrix{Int64}(undef, 8, rim_capacity); sums = Matrix{Float64}(undef, 7, rim_capacity)
    edge = Vector{Int32}(undef, edge_capacity)
    nr = Ref{Int64}(0); nb = Ref{Int64}(0)
    check(ccall((:r2s_last_mesh_holes, LIB[]), Cint, (Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int64}),
                rim_capacity == 0 ? C_NULL : start, rim_capacity == 0 ? C_NULL : counts, rim_capacity == 0 ? C_NULL : sums,
                Int64(rim_capacity), edge_capacity == 0 ? C_NULL : edge, Int64(edge_capacity), nr, nb))
    counts[8, :] .+= 1
    return (rim_start = start, rim_edge = edge, counts = counts, sums = sums)
end

# the same on device arrays of the current device (raw pointers, e.g. of AMDGPU.jl ROCArrays); each group is written only when its
# capacity holds all of it: d_rim_start (rim_capacity + 1), d_counts, d_sums / d_rim_edge / d_verts_out / d_tris_out (both or
# C_NULL: no fill) -> (n_rims, n_edges, n_verts_out, n_tris_out, ref_point, totals); indices stay 0-based
function mesh_holes_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer, max_edges::Integer,
                            d_rim_start::Ptr{Cvoid}, d_counts::Ptr{Cvoid}, d_sums::Ptr{Cvoid}, rim_capacity::Integer,
                            d_rim_edge::Ptr{Cvoid}, edge_capacity::Integer, d_tris_out::Ptr{Cvoid} = C_NULL,
                            d_verts_out::Ptr{Cvoid} = C_NULL, vert_capacity::Integer = 0, tri_capacity::Integer = 0;
                            stream::Ptr{Cvoid} = C_NULL)
    nr = Ref{Int64}(0); nb = Ref{Int64}(0); nvo = Ref{Int64}(0); nto = Ref{Int64}(0)
    r = zeros(Float64, 3); totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_holes_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid},
                 Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), Int64(max_edges), d_rim_start, d_counts, d_sums, Int64(rim_capacity),
                d_rim_edge, Int64(edge_capacity), d_tris_out, d_verts_out, Int64(vert_capacity), Int64(tri_capacity), nr, nb, nvo, nto, r,
                totals, stream))
    return nr[], nb[], nvo[], nto[], r, totals
end

# The self-intersections of a triangle mesh (include/rho2sdf_hip.h, r2s_mesh_index_intersections): the pairs of triangles that
# intersect or touch.  Coplanar overlap is not reported; contact counts (a vertex on a face, equal coordinates under different
# indices), so weld a soup first.  -> (pairs 2 x n Int32, 1-based, s < t, ascending by (s, t); hits_of_tri, the number of pairs
# each triangle is in; totals: intersecting pairs, triangles involved, candidate pairs, candidates skipped as adjacent, candidates
# sharing exactly one vertex index, collapsed triangles, 0, 0).  Two calls: the counts, then the pairs into room for all of them.
function _intersections_two_calls(nt::Integer, call)
    hits = Vector{Int32}(undef, nt)
    totals = zeros(Int64, 8)
    check(call(hits, C_NULL, Int64(0), totals))
    pairs = Matrix{Int32}(undef, 2, totals[1])
    totals[1] == 0 || check(call(hits, pairs, Int64(totals[1]), totals))
    return (pairs = pairs .+ Int32(1), hits_of_tri = hits, totals = totals)
end

# through an index at hand; the index is not changed
function mesh_index_intersections(ix::MeshIndexHIP)
    nt = mesh_index_info(ix).n_tris
    return _intersections_two_calls(nt, (hits, pairs, cap, totals) ->
        ccall((:r2s_mesh_index_intersections, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Int64}),
              ix.handle, hits, pairs, cap, totals))
end

# without an index: verts 3 x nv Float32, tris 3 x nt 1-based; a tree is built, used and dropped
function mesh_intersections_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}; device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    v, t0 = Matrix(verts), Int32.(tris) .- Int32(1)
    return _intersections_two_calls(size(t0, 2), (hits, pairs, cap, totals) ->
        ccall((:r2s_mesh_intersections, LIB[]), Cint,
              (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Int32, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Int64}),
              v, size(v, 2), t0, size(t0, 2), Int32(device), hits, pairs, cap, totals))
end

# the same on device arrays of the current device (raw pointers); d_hits_of_tri may be C_NULL, d_pairs only with pair_capacity 0;
# the pairs are written only when pair_capacity holds all of them -> totals; indices stay 0-based on the device
function mesh_index_intersections_dev(ix::MeshIndexHIP, d_hits_of_tri::Ptr{Cvoid}, d_pairs::Ptr{Cvoid}, pair_capacity::Integer;
                                      stream::Ptr{Cvoid} = C_NULL)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_index_intersections_dev, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}),
                ix.handle, d_hits_of_tri, d_pairs, Int64(pair_capacity), totals, stream))
    return totals
end

function mesh_intersections_dev_hip(d_verts::Ptr{Cvoid}, n_verts::Integer, d_tris::Ptr{Cvoid}, n_tris::Integer,
                                    d_hits_of_tri::Ptr{Cvoid}, d_pairs::Ptr{Cvoid}, pair_capacity::Integer;
                                    stream::Ptr{Cvoid} = C_NULL)
    totals = zeros(Int64, 8)
    check(ccall((:r2s_mesh_intersections_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}),
                d_verts, Int64(n_verts), d_tris, Int64(n_tris), d_hits_of_tri, d_pairs, Int64(pair_capacity), totals, stream))
    return totals
end

# ---- winding number, inside / outside and signed distance from the mesh (include/rho2sdf_hip.h, r2s_mesh_index_winding) ----------
# ray: 0, 1, 2 = +x, +y, +z; 3, 4, 5 = -x, -y, -z.  rule: :positive (winding > 0), :nonzero, :odd (crossings odd).
const _INSIDE_RULES = Dict(:positive => Int32(0), :nonzero => Int32(1), :odd => Int32(2))
_inside_rule(rule::Symbol) = get(() -> error("rule must be :positive, :nonzero or :odd"), _INSIDE_RULES, rule)

# the winding number of the points (3 x n, Float32 or Float64) -> (winding, crossings), Vector{Int32}: +1 inside an outward-wound
# closed body; a non-finite point gives 0 / -1; a point ON the surface gets a ray-dependent answer
function mesh_index_winding(ix::MeshIndexHIP, points::AbstractMatrix{T}; ray::Integer = 2) where {T<:Union{Float32,Float64}}
    size(points, 1) == 3 || error("points must be 3 x n")
    n = size(points, 2)
    winding, crossings = Vector{Int32}(undef, n), Vector{Int32}(undef, n)
    check(ccall((:r2s_mesh_index_winding, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Int32}, Ptr{Int32}),
                ix.handle, Matrix(points), Int32(T == Float32), n, Int32(ray), winding, crossings))
    return winding, crossings
end

# distance of the points with the sign of the inside rule: positive inside (in the material) -> Vector{Float64}
function mesh_index_signed_distance(ix::MeshIndexHIP, points::AbstractMatrix{T}; rule::Symbol = :positive,
                                    ray::Integer = 2) where {T<:Union{Float32,Float64}}
    size(points, 1) == 3 || error("points must be 3 x n")
    n = size(points, 2)
    dist = Vector{Float64}(undef, n)
    check(ccall((:r2s_mesh_index_signed, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Int32}),
                ix.handle, Matrix(points), Int32(T == Float32), n, _inside_rule(rule), Int32(ray), Int32(0), dist, C_NULL))
    return dist
end

# winding and crossings on every point of the lattice of extract_isosurface_hip for (grid, smooth) -> two Array{Int32,3} (x fastest)
function mesh_index_winding_lattice(ix::MeshIndexHIP, grid::MeshGrid.Grid, smooth::Union{Int,Nothing} = nothing; ray::Integer = 2)
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    winding, crossings = Array{Int32,3}(undef, dims...), Array{Int32,3}(undef, dims...)
    check(ccall((:r2s_mesh_index_winding_lattice, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Float64, Int32, Ptr{Int32}, Ptr{Int32}),
                ix.handle, collect(dims), collect(Float64.(grid.AABB_min)), spacing, Int32(ray), winding, crossings))
    return winding, crossings
end

# the signed distance on every point of that lattice -> Array{Float64,3}
function mesh_index_signed_lattice(ix::MeshIndexHIP, grid::MeshGrid.Grid, smooth::Union{Int,Nothing} = nothing;
                                   rule::Symbol = :positive, ray::Integer = 2)
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    dist = Array{Float64,3}(undef, dims...)
    check(ccall((:r2s_mesh_index_signed_lattice, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Float64, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Int32}),
                ix.handle, collect(dims), collect(Float64.(grid.AABB_min)), spacing, _inside_rule(rule), Int32(ray), Int32(0), dist, C_NULL))
    return dist
end

# without an index: verts 3 x nv Float32, tris 3 x nt 1-based; a tree is built, used and dropped.  STL -> .vti:
# import_stl_hip(file; orient = :outward) -> mesh_signed_distance_hip -> the .vti export of the same grid
function mesh_signed_distance_hip(verts::AbstractMatrix{Float32}, tris::AbstractMatrix{<:Integer}, grid::MeshGrid.Grid,
                                  smooth::Union{Int,Nothing} = nothing; rule::Symbol = :positive, ray::Integer = 2, device::Integer = -1)
    size(verts, 1) == 3 && size(tris, 1) == 3 || error("verts and tris must be 3 x n")
    v, t0 = Matrix(verts), Int32.(tris) .- Int32(1)
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    dist = Array{Float64,3}(undef, dims...)
    check(ccall((:r2s_mesh_signed_distance, LIB[]), Cint,
                (Ptr{Float32}, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Float64}, Float64, Int32, Int32, Int32, Int32, Ptr{Cvoid}),
                v, size(v, 2), t0, size(t0, 2), collect(dims), collect(Float64.(grid.AABB_min)), spacing, _inside_rule(rule), Int32(ray),
                Int32(0), Int32(device), dist))
    return dist
end

# the device-pointer forms (raw pointers on the index's device, which must be current; enqueued on `stream`, not waited for)
function mesh_index_winding_dev(ix::MeshIndexHIP, d_points::Ptr{Cvoid}, points_are_float32::Bool, n::Integer, d_winding::Ptr{Cvoid},
                                d_crossings::Ptr{Cvoid}; ray::Integer = 2, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:r2s_mesh_index_winding_dev, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                ix.handle, d_points, Int32(points_are_float32), Int64(n), Int32(ray), d_winding, d_crossings, stream))
end

function mesh_index_signed_dev(ix::MeshIndexHIP, d_points::Ptr{Cvoid}, points_are_float32::Bool, n::Integer, d_dist::Ptr{Cvoid},
                               out_is_float32::Bool; rule::Symbol = :positive, ray::Integer = 2, d_closest_tri::Ptr{Cvoid} = C_NULL,
                               stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:r2s_mesh_index_signed_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                ix.handle, d_points, Int32(points_are_float32), Int64(n), _inside_rule(rule), Int32(ray), Int32(out_is_float32), d_dist,
                d_closest_tri, stream))
end

# The triangles of a binary or ASCII STL file (r2s_import_stl) -> (verts 3 x nv Float32, tris 3 x nt 1-based).  weld = true: the
# equal vertices are merged by mesh_weld_hip(soup; snap); weld = false: the soup as the file holds it, tris = 1:3nt.
# orient = nothing: the windings as the file holds them; :majority or :outward (needs weld = true): the welded triangles go
# through mesh_orient_hip (see there for the rules and the caveat about enclosed voids); :nested: outward, then the enclosed
# voids reversed again by mesh_nesting_hip(rewind = true).  check_intersections = true (needs
# weld = true): -> (verts, tris, mesh_intersections_hip of the mesh as returned).  split_vertices = true (needs weld = true): the
# vertices the weld left pinched are split by mesh_fans_hip(split = true), after the orient if one is asked for.  fill_holes = k
# (needs weld = true): after that the closed rims are capped by mesh_holes_hip(fill = k), -1 every hole, k > 0 those of at most
# k edges; the intersections are those of the filled mesh.
function import_stl_hip(filename::AbstractString; weld::Bool = true, snap::Real = 0.0, device::Integer = -1,
                        orient::Union{Nothing,Symbol} = nothing, check_intersections::Bool = false, split_vertices::Bool = false,
                        fill_holes::Union{Nothing,Integer} = nothing)
    orient === nothing || orient in (:majority, :outward, :nested) || error("orient must be nothing, :majority, :outward or :nested")
    orient === nothing || weld || error("orient needs weld = true")
    !split_vertices || weld || error("split_vertices needs weld = true")
    !check_intersections || weld || error("check_intersections needs weld = true")
    fill_holes === nothing || weld || error("fill_holes needs weld = true")
    m = R2SStlMesh(0, C_NULL)
    check(ccall((:r2s_import_stl, LIB[]), Cint, (Cstring, Ref{R2SStlMesh}), filename, m))
    soup = copy(unsafe_wrap(Array, m.verts, (3, 3 * Int(m.n_tris))))
    ccall((:r2s_free_stl_mesh, LIB[]), Cvoid, (Ref{R2SStlMesh},), m)
    weld || return soup, reshape(Int32.(1:size(soup, 2)), 3, :)
    w = mesh_weld_hip(soup; snap = snap, device = device)
    tris = orient === nothing ? w.tris : mesh_orient_hip(w.verts, w.tris; outward = orient !== :majority, device = device).tris
    orient === :nested && (tris = mesh_nesting_hip(w.verts, tris; rewind = true, device = device).tris)
    verts = w.verts
    if split_vertices
        f = mesh_fans_hip(verts, tris; split = true, device = device)
        verts, tris = f.verts, f.tris
    end
    if fill_holes !== nothing
        h = mesh_holes_hip(verts, tris; fill = fill_holes, device = device)
        verts, tris = h.verts, h.tris
    end
    check_intersections || return verts, tris
    return verts, tris, mesh_intersections_hip(verts, tris; device = device)
end

# The signed distance to the iso-surface of `values` on the whole lattice (r2s_redistance_full): redistance_hip without a band;
# +-Inf where the field has no surface.
function redistance_full_hip(values::AbstractArray{T}, grid::MeshGrid.Grid, smooth::Union{Int,Nothing} = nothing;
                             iso = 0.0) where {T<:Union{Float32,Float64}}
    s = smooth === nothing ? 1 : smooth
    dims = Int64.((grid.N .* s) .+ 1)
    length(values) == prod(dims) || error("values length ($(length(values))) doesn't match the lattice $(Tuple(dims))")
    spacing = smooth === nothing ? Float64(grid.cell_size) : Float64(grid.cell_size) / s
    out = Array{T,3}(undef, dims...)
    check(ccall((:r2s_redistance_full, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Float64, Float64, Int32, Ptr{Cvoid}),
                values, Int32(T == Float32), collect(dims), collect(Float64.(grid.AABB_min)), spacing, Float64(iso), Int32(-1), out))
    return out
end

# calculate_volume_from_sdf (src/SdfSmoothing/CalcVolumeFromSDF.jl:26-125); `grid` is the reference's array of
# per-voxel coordinate vectors - only the spacing is used (:36-39)
function calculate_volume_from_sdf_hip(sdf::Array{Float32,3}, grid::AbstractArray{Vector{Float32},3}; iso_threshold = 0.0f0,
                                       detailed_quad_order = 9)
    @assert size(grid) == size(sdf) "Dimensions of fine_sdf and fine_grid must match"
    d = grid[2, 1, 1] .- grid[1, 1, 1]
    edge = sqrt(sum(d .* d))                                             # norm(edge_vector), :37-38
    v = Ref{Float32}(0.0f0)
    check(ccall((:r2s_volume_from_sdf, LIB[]), Cint,
                (Ptr{Float32}, Int64, Int64, Int64, Float32, Float32, Int32, Int32, Ref{Float32}),
                sdf, size(sdf, 1), size(sdf, 2), size(sdf, 3), edge, Float32(iso_threshold),
                Int32(detailed_quad_order), Int32(-1), v))
    return v[]
end

# RBFs_smoothing (src/SdfSmoothing/RBFs4Smoothing.jl:321-377) -> (fine_sdf::Array{Float32,3}, fine_grid)
function RBFs_smoothing_hip(mesh::Mesh, dist::Vector{Float64}, grid::MeshGrid.Grid, is_interp::Bool,
                            smooth::Int, taskName::String, threshold::Float64 = 1e-3)
    dim = (grid.N .* smooth) .+ 1
    fine_grid = fine_grid_of(grid, smooth)                              # point list only (:341), stays in Julia
    fine = pinned(Float32, dim...)
    check(ccall((:r2s_rbf_smooth, LIB[]), Cint,
                (Ptr{Float64}, Ref{R2SGrid}, Int32, Int32, Float64, Float64, Int32, Ptr{Float32}, Ptr{Float32},
                 Ptr{Int32}, Ptr{Float32}),
                dist, Ref(R2SGrid(grid)), Int32(is_interp), Int32(smooth), threshold,
                mesh.V_frac * mesh.V_domain, Int32(-1), fine, C_NULL, C_NULL, C_NULL))
    return fine, fine_grid
end

# ---- the smoothed level-set as a function (include/rho2sdf_hip.h, r2s_rbf_field) --------------------------------------
# RBFs_smoothing samples f(p) = th + sum_j w_j exp(-(|p - x_j| / sigma)^2) on a lattice; an RbfField keeps w and th on the
# device and evaluates f, its gradient, outward normals and the projection onto {f = 0} at any 3 x n Float32 points.
mutable struct RbfField
    handle::Ptr{Cvoid}
    level_shift::Float32
    cg_iterations::Int32
end

function destroy!(f::RbfField)
    f.handle == C_NULL || ccall((:r2s_rbf_field_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), f.handle)
    f.handle = C_NULL
    return nothing
end

function fit_rbf_field_hip(mesh::Mesh, dist::Vector{Float64}, grid::MeshGrid.Grid, is_interp::Bool, threshold::Float64 = 1e-3)
    h = Ref{Ptr{Cvoid}}(C_NULL); th = Ref{Float32}(0.0f0); its = Ref{Int32}(0)
    check(ccall((:r2s_rbf_field_fit, LIB[]), Cint,
                (Ptr{Float64}, Ref{R2SGrid}, Int32, Float64, Float64, Int32, Ref{Ptr{Cvoid}}, Ref{Float32}, Ref{Int32}),
                dist, Ref(R2SGrid(grid)), Int32(is_interp), threshold, mesh.V_frac * mesh.V_domain, Int32(-1), h, th, its))
    return finalizer(destroy!, RbfField(h[], th[], its[]))
end

function rbf_field_from_weights_hip(weights::Array{Float32}, grid::MeshGrid.Grid, level_shift::Float32 = 0.0f0,
                                    threshold::Float64 = 1e-3)
    length(weights) == grid.ngp || error("weights length ($(length(weights))) doesn't match grid points ($(grid.ngp))")
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:r2s_rbf_field_from_weights, LIB[]), Cint,
                (Ptr{Float32}, Ref{R2SGrid}, Float64, Float32, Int32, Ref{Ptr{Cvoid}}),
                weights, Ref(R2SGrid(grid)), threshold, level_shift, Int32(-1), h))
    return finalizer(destroy!, RbfField(h[], level_shift, Int32(0)))
end

function rbf_field_weights_hip(f::RbfField, grid::MeshGrid.Grid)
    w = Array{Float32,3}(undef, (grid.N .+ 1)...)
    th = Ref{Float32}(0.0f0)
    check(ccall((:r2s_rbf_field_weights, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ref{Float32}), f.handle, w, th))
    return w, th[]
end

# -> (val::Vector{Float32}, grad::Matrix{Float32} 3 x n, taps::Vector{Int32}); taps < 0 where the knn(124) cap bound
function rbf_field_eval_hip(f::RbfField, points::Matrix{Float32})
    size(points, 1) == 3 || error("points must be 3 x n")
    n = size(points, 2)
    val = Vector{Float32}(undef, n); grad = Matrix{Float32}(undef, 3, n); taps = Vector{Int32}(undef, n)
    check(ccall((:r2s_rbf_field_eval, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}),
                f.handle, points, n, val, grad, taps))
    return val, grad, taps
end

# -> (val, grad 3 x n, hess 6 x n = xx, yy, zz, xy, xz, yz per point, taps): the evaluation with its second derivatives
function rbf_field_hessian_hip(f::RbfField, points::Matrix{Float32})
    size(points, 1) == 3 || error("points must be 3 x n")
    n = size(points, 2)
    val = Vector{Float32}(undef, n); grad = Matrix{Float32}(undef, 3, n); hess = Matrix{Float32}(undef, 6, n)
    taps = Vector{Int32}(undef, n)
    check(ccall((:r2s_rbf_field_hessian, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}),
                f.handle, points, n, val, grad, hess, taps))
    return val, grad, hess, taps
end

# -> curv 4 x n = mean, gauss, k1, k2 per point (normal -grad / |grad|: a convex solid has positive mean curvature; NaN where
# the gradient vanishes), with the gradient and Hessian they were formed from
function rbf_field_curvature_hip(f::RbfField, points::Matrix{Float32})
    size(points, 1) == 3 || error("points must be 3 x n")
    n = size(points, 2)
    curv = Matrix{Float32}(undef, 4, n); grad = Matrix{Float32}(undef, 3, n); hess = Matrix{Float32}(undef, 6, n)
    check(ccall((:r2s_rbf_field_curvature, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                f.handle, points, n, curv, grad, hess))
    return curv, grad, hess
end

# device-pointer variants: pointers on the field's device (the current one), enqueued on `stream`, no wait; C_NULL = not wanted
function rbf_field_hessian_dev_hip(f::RbfField, d_points::Ptr{Float32}, n::Integer, d_val::Ptr{Float32}, d_grad::Ptr{Float32},
                                   d_hess::Ptr{Float32}, d_taps::Ptr{Int32}; stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:r2s_rbf_field_hessian_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
                f.handle, d_points, Int64(n), d_val, d_grad, d_hess, d_taps, stream))
end

function rbf_field_curvature_dev_hip(f::RbfField, d_points::Ptr{Float32}, n::Integer, d_curv::Ptr{Float32},
                                     d_grad::Ptr{Float32} = Ptr{Float32}(C_NULL), d_hess::Ptr{Float32} = Ptr{Float32}(C_NULL);
                                     stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:r2s_rbf_field_curvature_dev, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                f.handle, d_points, Int64(n), d_curv, d_grad, d_hess, stream))
end

function rbf_field_normals_hip(f::RbfField, points::Matrix{Float32})
    size(points, 1) == 3 || error("points must be 3 x n")
    normals = similar(points)
    check(ccall((:r2s_rbf_field_normals, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}),
                f.handle, points, size(points, 2), normals))
    return normals
end

# -> (projected points, status, residual |f|, steps); status 0 = converged, 1 = iteration cap, 2 = vanishing gradient,
# 3 = non-finite input
function rbf_field_project_hip(f::RbfField, points::Matrix{Float32}, tol::Float32; max_iter::Integer = 8)
    size(points, 1) == 3 || error("points must be 3 x n")
    p = copy(points); n = size(p, 2)
    status = Vector{Int32}(undef, n); resid = Vector{Float32}(undef, n); iters = Vector{Int32}(undef, n)
    check(ccall((:r2s_rbf_field_project, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Float32}, Int64, Int32, Float32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}),
                f.handle, p, n, Int32(max_iter), tol, status, resid, iters))
    return p, status, resid, iters
end

# vertices of extract_isosurface_hip moved onto the zero level of the function they sample + the unit normals there
function refine_surface_hip(f::RbfField, verts::Matrix{Float32}, grid::MeshGrid.Grid; max_iter::Integer = 8)
    p, status, _, _ = rbf_field_project_hip(f, verts, Float32(1e-4 * grid.cell_size); max_iter = max_iter)
    return p, rbf_field_normals_hip(f, p), status
end

"Replace the reference methods by the HIP-backed ones (method overwrite).  `n_gpus` > 1: every call fans out over
devices 0..n_gpus-1 inside the library (single Julia process, no MPI)."
function enable!(libpath::AbstractString = LIB[]; n_gpus::Integer = 1)
    LIB[] = libpath
    N_GPUS[] = Int32(n_gpus)
    @eval Rho2sdf begin
        rho2sdf(taskName::String, X::Vector{Vector{Float64}}, IEN::Vector{Vector{Int64}}, rho::Vector{Float64};
                options::Rho2sdfOptions = Rho2sdfOptions()) = $(rho2sdf_hip)(taskName, X, IEN, rho; options = options)
    end
    @eval SignedDistances begin
        evalDistances(mesh::Mesh, grid::Grid, points::Matrix, ρₙ::Vector{Float64}, ρₜ::Float64; kw...) =
            $(evalDistances_hip)(mesh, grid, points, ρₙ, ρₜ; want_xp = true, kw...)   # direct callers get the reference's (dist, xp)
        Sign_Detection(mesh::Mesh, grid::Grid, points::Matrix, ρₙ::Vector{Float64}, ρₜ::Float64) =
            $(Sign_Detection_hip)(mesh, grid, points, ρₙ, ρₜ)
        remove_sdf_artifacts!(sdf::Vector{Float64}, grid::Grid; kw...) = $(remove_sdf_artifacts_hip!)(sdf, grid; kw...)
        analyze_sdf_components(sdf_values::Vector{Float64}, grid::Grid; threshold::Float64 = 0.0) =
            $(analyze_sdf_components_hip)(sdf_values, grid; threshold = threshold)
    end
    @eval MeshGrid begin
        DenseInNodes(mesh::Mesh, rho::Vector{Float64}) = $(DenseInNodes_hip)(mesh, rho)
        find_threshold_for_volume(mesh::Mesh, ρₙ::Vector{Float64}, tolerance::Float64 = 1e-4, max_iterations::Int = 60) =
            $(find_threshold_for_volume_hip)(mesh, ρₙ, tolerance, max_iterations)
        calculate_isocontour_volume(mesh::Mesh, ρₙ::Vector{Float64}, iso_threshold::Float64) =
            $(calculate_isocontour_volume_hip)(mesh, ρₙ, iso_threshold)
    end
    @eval SdfSmoothing begin
        RBFs_smoothing(mesh::Mesh, dist::Vector, grid::Grid, is_interp::Bool, smooth::Int, taskName::String,
                       threshold::Float64 = 1e-3) = $(RBFs_smoothing_hip)(mesh, Vector{Float64}(dist), grid, is_interp, smooth, taskName, threshold)
        calculate_volume_from_sdf(sdf::Array{Float32,3}, grid::Array{Vector{Float32},3}; kw...) =
            $(calculate_volume_from_sdf_hip)(sdf, grid; kw...)
    end
    return nothing
end

"Free the device buffers the library keeps between calls (plan, volumes, staging, RBF matrix)."
release!() = ccall((:r2s_release_cache, LIB[]), Cvoid, ())

end # module
