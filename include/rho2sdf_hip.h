/*
 * rho2sdf_hip.h - C ABI of the MI355X-native signed-distance extraction engine.
 *
 * The reference (kopacja/rho2sdf.jl) has no FFI of its own for this path; the
 * drop-in boundary is the set of Julia functions `rho2sdf()` calls
 * (src/RhoToSDF.jl:148-224).  Each entry point below replaces the body of one of
 * them; the Julia-side `ccall` stubs are in INTEGRATION.md and
 * rho2sdf.jl_amd/julia/Rho2sdfHIP.jl.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (streams are void*).
 *   - array layouts are the reference's Julia column-major layouts:
 *       X    3 x nnp  Float64  -> double[nnp][3]
 *       IEN  nen x nel Int64, 1-based -> int64_t[nel][nen]
 *       grid linear index (0-based) = k*(N1+1)*(N2+1) + j*(N1+1) + i   (Grid.jl:84-92)
 *   - return 0 on success, negative on error; r2s_last_error() gives the text
 *     (the Julia wrapper turns it into `error(...)`, as the reference does).
 *   - `*_dev` entry points take DEVICE pointers (resident in HBM) and a HIP
 *     stream handle; the host-pointer entry points allocate/copy internally and
 *     never keep caller pointers after returning.
 *   - the library fails with R2S_ERR_NO_DEVICE when no gfx950 device is usable;
 *     there is no CPU fallback.
 *
 * Streams (every `*_dev` entry point; tests/test_stream_order_gpu.py is the executable form of this paragraph)
 *   - `stream` is a hipStream_t (NULL = the null stream); it may be a non-blocking stream.  Device inputs need only be
 *     ready IN STREAM ORDER: work queued on `stream` before the call (a copy that fills an input, the kernel that
 *     produces it) need not have finished, and nothing need be synchronised with the host.  Outputs are complete in stream
 *     order: work queued on `stream` after the call sees them.
 *   - no work is put on a stream the caller cannot order against.  Where an entry point uses streams of its own, they are
 *     forked from `stream` and joined back into it by events before the call returns (r2s_plan_run_dev: two streams the plan
 *     owns); the one entry point that works on the null stream, r2s_rbf_smooth_dev, waits for `stream` first and for the
 *     whole device before it returns.
 *   - which calls wait.  Enqueue only, return with the work still queued: r2s_fill_dev, r2s_plan_pack_tiles_dev,
 *     r2s_plan_pack_tiles2_dev, r2s_unpack_tiles_dev, r2s_unpack_masks_dev, r2s_unpack_segments_dev, r2s_rbf_field_eval_dev /
 *     _normals_dev / _hessian_dev / _curvature_dev / _project_dev, r2s_mesh_index_query_dev / _lattice_dev / _raycast_dev.
 *     Return only after `stream` has drained (they hand counts to the host, or size their work from counts read back):
 *     r2s_plan_run_dev (every call ends with a wait for `stream`; the first call for a set of shapes also waits twice in
 *     the middle), r2s_remove_artifacts_dev, r2s_analyze_components_dev, r2s_rbf_smooth_dev, r2s_extract_isosurface_dev,
 *     r2s_mesh_distance_dev, r2s_redistance_dev, r2s_redistance_full_dev, r2s_mesh_index_build_dev, r2s_mesh_shells_dev,
 *     r2s_mesh_sections_dev, r2s_mesh_weld_dev, r2s_mesh_simplify_dev, r2s_mesh_orient_dev, r2s_mesh_fans_dev,
 *     r2s_mesh_holes_dev, r2s_mesh_nesting_dev.  A caller should still order its consumers on `stream`, not on that wait.
 *   - sharing.  A plan serves one call at a time: successive calls on one stream need no host wait in between (each call
 *     has drained the stream when it returns), r2s_plan_pack_tiles*_dev read the tile lists of the plan's last run and belong
 *     on that run's stream before the plan's next run; different plans are independent and may be driven on different
 *     streams.  A field (r2s_rbf_field) and a mesh index are only read by their _dev entry points: one object may be used
 *     from several streams and threads at once.  The entry points that keep work buffers per device (removal and component
 *     analysis, smoothing, extraction, redistancing, shells, sections, weld, simplify, orient, fans, holes, intersections, nesting) take a lock
 *     for the length of the call: concurrent calls are safe and run one after the other.  The host-pointer SDF entry points
 *     (r2s_eval_distances, r2s_sign_detection, r2s_sdf, r2s_rho2sdf) lock their device's session in the same way.  Results a
 *     call leaves behind for r2s_last_* and r2s_last_error belong to the calling thread.  tests/test_threads_gpu.py is the
 *     executable form of this item for host threads; r2s_release_cache is the exception (see there).
 *   - devices.  Device pointers and `stream` belong to one device.  r2s_plan_run_dev and r2s_plan_pack_tiles*_dev make the
 *     plan's device current (and leave it current); the _dev entry points of a field or an index refuse a call while
 *     another device than the object's is current (R2S_ERR_ARG, outputs untouched); for every other _dev entry point the
 *     device of the pointers must be the current one - a call with another device current is outside the contract.
 */
#ifndef RHO2SDF_HIP_H
#define RHO2SDF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R2S_VERSION 100 /* 0.1.0 */

#define R2S_OK 0
#define R2S_ERR_ARG (-1)
#define R2S_ERR_NO_DEVICE (-2)
#define R2S_ERR_HIP (-3)
#define R2S_ERR_UNSUPPORTED (-4)
#define R2S_ERR_NOMEM (-5)

#define R2S_HEX8 0
#define R2S_TET4 1

/* mirrors `mutable struct Grid` (src/MeshGrid/Grid.jl:2-7) */
typedef struct {
    double aabb_min[3];
    double aabb_max[3];
    int64_t N[3];      /* cells per axis; grid points per axis = N+1 */
    double cell_size;
    int64_t ngp;
} r2s_grid;

/* constants that are hard-coded in the reference become fields with the same defaults */
typedef struct {
    double band_factor; /* 1.1  : delta = band_factor*cell_size (sdfOnDensityField.jl:158) */
    int32_t elem_type;  /* R2S_HEX8 / R2S_TET4 (Rho2sdfOptions.element_type, RhoToSDF.jl:20) */
    int32_t device;     /* HIP device ordinal, -1 = current device */
    /* multi-GPU Z partition of r2s_plan_run_dev: zstride <= 1 -> contiguous planes [k_begin,k_end);
     * zstride = G > 1 -> this call computes the 4-plane tile layers t with t % G == zphase of the whole
     * grid (k_begin = 0, k_end = N3+1) and stores them consecutively: local plane 4*i+l holds lattice
     * plane 4*(i*G + zphase) + l; the output then has 4*ceil((layers - zphase)/G) planes. */
    int32_t zstride;
    int32_t zphase;
    /* host-pointer entry points (r2s_sdf, r2s_eval_distances, r2s_sign_detection): number of devices the ONE call
     * fans out over (single process, one host thread per device 0..n_gpus-1, interleaved tile layers, every
     * device sends its layers straight to their place in the caller's array); <= 1 = the device named above */
    int32_t n_gpus;
    /* 0 = the reference's single-thread semantics (bit parity with a Julia run); 1 = order-independent "true
     * minimum" (SURVEY 8(f)4): every valid candidate of a boundary triangle takes part in the minimum (no
     * first-improving-edge break, sdfOnDensityField.jl:769-771; no vertex fall-back only after failures, :777),
     * exact ties go to the lexicographically smaller projection point, and the HEX8 sign is +1 when ANY candidate
     * element holding the point (max|xi| < 1.01) has rho >= rho_t (instead of SignDetection.jl:56-69's
     * improving-sequence rule).  dist_true <= dist_ordered everywhere; see DESIGN.md for the measured deviation. */
    int32_t true_min;
    /* HEX8 sign pass: 1 = no inner-region shortcut (every candidate pair runs its inverse map and the ordered walk of
     * SignDetection.jl:41-68) - for OVERLAPPING / non-conforming meshes, where the shortcut's precondition does not hold
     * (see r2s_sign_detection below).  0 = shortcut on.  The environment variable R2S_SIGN_NO_INNER=1 forces it for every
     * call of the process. */
    int32_t sign_no_inner;
    int32_t reserved_;
} r2s_params;

/* per-call counters (optional; pass NULL) */
typedef struct {
    int64_t n_solid;        /* elements with min(rho_e) >= rho_t           */
    int64_t n_iso;          /* elements crossed by the iso-surface         */
    int64_t n_items;        /* band work items (boundary triangles + iso)  */
    int64_t n_band_entries; /* tile->item list entries                     */
    int64_t n_sign_entries; /* tile->element list entries                  */
    int64_t n_tiles;        /* 4x4x4 voxel tiles in the slab               */
    int64_t n_active_tiles; /* tiles that ran the distance kernel          */
    int64_t n_active_sign_tiles; /* tiles that ran the sign kernel         */
    int64_t n_iso_chunks;   /* 64-voxel chunks swept by iso_project_kernel    */
    int64_t n_any_tiles;    /* tiles that can hold non-sentinel voxels (sparse gather) */
    /* HIP-event times of the last call, measured on the call's stream: mesh prep+items,
     * tile bins, sentinel sweep, iso_project_kernel (ms_main), ordered gather
     * (sdf_tiles_kernel<dist>), sign kernel */
    double ms_prep, ms_bins, ms_fill, ms_main, ms_gather, ms_sign;
    int64_t n_sign_only_tiles; /* tiles without band items whose voxels are all +-1e10 (compressed stitching) */
    /* HEX8: iso_project_hex_pl_kernel alone; ms_main also holds iso_straggler_kernel and iso_sweep_kernel */
    double ms_iso_fast;
    /* HEX8 iso-surface projections (one per iso element x band voxel): pairs the fast Newton-SQP lane machine handed to the
     * complete solver, and runs of the complete solver that ended WITHOUT a KKT point (iteration / non-convex-step caps,
     * cycle): their voxel takes the nearest on-surface iterate - the reference likewise uses whatever NLopt returns and
     * only warns on :FAILURE (ComputeCoordsOnIso.jl:79-86).  SURVEY A6: reported, not hidden. */
    int64_t n_iso_straggler, n_iso_fail;
} r2s_stats;

int r2s_version(void);
const char *r2s_last_error(void);
int r2s_device_count(void);
void r2s_default_params(r2s_params *p);

/* Grid(AABB_min, AABB_max, N_max, margineCells)          src/MeshGrid/Grid.jl:10-34 */
int r2s_grid_make(const double xmin[3], const double xmax[3], int64_t n_max, int64_t margin,
                  r2s_grid *out);

/* noninteractive_sdf_grid_setup(mesh)                    src/MeshGrid/Grid_setup.jl:94-108 */
int r2s_auto_grid(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int32_t elem_type,
                  r2s_grid *out, double *median_edge);

/* evalDistances(mesh, grid, points, rho_n, rho_t) -> (dist, xp)
 *                                         src/SignedDistances/sdfOnDensityField.jl:139-486
 * dist_out[ngp] (1e10 = untouched), xp_out[ngp][3] or NULL. */
int r2s_eval_distances(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel,
                       const double *rho_n, double rho_t, const r2s_grid *grid,
                       const r2s_params *params, double *dist_out, double *xp_out, r2s_stats *stats);

/* Sign_Detection(mesh, grid, points, rho_n, rho_t) -> signs in {-1,+1}
 *                                         src/SignedDistances/SignDetection.jl:275-283
 * HEX8 precondition of one shortcut: a lattice point inside the convex inner region of an element whose nodal densities
 * all lie on one side of rho_t gets that element's answer without a Newton solve, which equals the reference's ordered
 * walk (SignDetection.jl:41-68) on a CONFORMING mesh (no other element holds the point with a smaller max|xi|).  On
 * overlapping / non-conforming meshes - where the reference's own result depends on which of the overlapping elements
 * comes first - set the environment variable R2S_SIGN_NO_INNER=1: every candidate pair then runs its inverse map
 * (tests/test_parity_gpu.py::test_overlapping_elements_without_the_inner_region_shortcut). */
int r2s_sign_detection(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel,
                       const double *rho_n, double rho_t, const r2s_grid *grid,
                       const r2s_params *params, double *signs_out, r2s_stats *stats);

/* fused `dists .* signs` (RhoToSDF.jl:169-171) - the path rho2sdf() uses */
int r2s_sdf(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_n,
            double rho_t, const r2s_grid *grid, const r2s_params *params, double *sdf_out,
            r2s_stats *stats);

/* ---- the whole of rho2sdf() in one call ---------------------------------------------
 * rho2sdf(taskName, X, IEN, rho; options)                          src/RhoToSDF.jl:116-242
 * minus the file exports (which stay with the caller): mesh volume (:128) -> DenseInNodes (:148) ->
 * find_threshold_for_volume (:151-156) -> evalDistances / Sign_Detection / product (:169-171) ->
 * remove_sdf_artifacts! (:174-208) -> RBFs_smoothing (:222-224).  The mesh goes up once, every stage
 * runs on HBM-resident data, the results come down once.  Fields mirror Rho2sdfOptions (:9-77). */
typedef struct {
    double threshold_density;            /* NaN = nothing: find_threshold_for_volume (TET4: the TET4 iso-volume) */
    double band_factor;                  /* 1.1 */
    double artifact_min_component_ratio; /* 0.01 */
    double rbf_kernel_threshold;         /* 1e-3 (RBFs4Smoothing.jl:328); [R2S_RBF_MIN_KERNEL_THRESHOLD, 1) */
    int32_t elem_type;                   /* R2S_HEX8 / R2S_TET4 */
    int32_t rbf_interp;                  /* 1 */
    int32_t rbf_smooth;                  /* 1 = rbf_grid :same, 2 = :fine */
    int32_t remove_artifacts;            /* 1 */
    int32_t device;                      /* -1 = current */
    int32_t n_gpus;                      /* > 1: devices 0..n_gpus-1: raw SDF on interleaved tile layers, then components and RBF smoothing
                                            slab-distributed (planes move between devices as peer copies over xGMI; nothing is gathered on one device) */
    int32_t skip_rbf;                    /* 1: stop after artifact removal (fine_sdf_out may be NULL) */
    int32_t true_min;                    /* r2s_params.true_min for the raw SDF */
    int32_t sign_no_inner;               /* r2s_params.sign_no_inner for the raw SDF */
    int32_t analyze_components;          /* 1 (with remove_artifacts): keep the component table of the labelling that artifact
                                            removal computes on the raw field at threshold 0 (analyze_sdf_components before the
                                            cleanup, RhoToSDF.jl:177-179); read it with r2s_last_components.  0 = no change */
    /* reserved[R2S_OPT_EXTRACT_SURFACE] = extract_surface: 1 (needs the smoothing, so not with skip_rbf: R2S_ERR_ARG) keeps the
       iso-0 surface of the returned fine field on the lattice exportSdfToVTI writes (origin aabb_min, spacing
       cell_size / rbf_smooth) as the calling thread's last surface; read it with r2s_last_isosurface.  Bit-identical to
       r2s_extract_isosurface of fine_sdf_out.  0 = no change.  reserved[1] must be 0. */
    int32_t reserved[2];
} r2s_options;
#define R2S_OPT_EXTRACT_SURFACE 0 /* index of the extract_surface flag in r2s_options.reserved */

typedef struct {
    double V_domain, V_frac;             /* calculate_mesh_volume */
    double rho_t;                        /* threshold used */
    int64_t n_flipped;                   /* remove_sdf_artifacts! */
    float level_shift;                   /* LS_Threshold `th` */
    int32_t cg_iters;
    int32_t threshold_iters;
    int32_t pad;
    /* wall-clock milliseconds of the stages of this call */
    double ms_upload, ms_pre, ms_sdf, ms_sdf_kernels, ms_artifacts, ms_rbf, ms_download, ms_total;
} r2s_run_info;

void r2s_default_options(r2s_options *o);

/* grid: from r2s_grid_make / r2s_auto_grid (the caller sizes its result arrays from it).
 * Optional outputs (NULL = not wanted): rho_n_out[nnp] nodal densities, sdf_raw_out[ngp] the field before
 * artifact removal, sdf_dists_out[ngp] the returned `sdf_dists`; fine_sdf_out[prod(N*rbf_smooth+1)] Float32
 * is required unless skip_rbf.  Result arrays from r2s_host_alloc come down by plain DMA. */
int r2s_rho2sdf(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_e,
                const r2s_options *options, const r2s_grid *grid, double *rho_n_out, double *sdf_raw_out,
                double *sdf_dists_out, float *fine_sdf_out, r2s_run_info *info);

/* Pinned host memory for result arrays (the Julia wrapper `unsafe_wrap`s it): device -> host copies into it run
 * at PCIe rate with no staging.  Any other host pointer works too (staged, multi-threaded).  The fused field of
 * r2s_sdf (one device, >= 4 M voxels) does not cross PCIe whole: host threads write the sentinel -1e10 into the caller's
 * array while the device works and only the tiles that can differ from it are transferred (R2S_HOST_SPARSE=0: dense). */
/* Host phases of the calling thread's last host-pointer SDF call on ONE device (r2s_eval_distances / r2s_sign_detection /
 * r2s_sdf), in ms: [0] upload of the mesh, [1] run (launches + the waits of the plan), [2] packing of the non-sentinel tiles
 * and issue of their copies, [3] wait for the host threads' sentinel fill, [4] wait for the copies, [5] scatter into the
 * caller's array (dense download: the whole transfer), [6] the whole call, [7] host threads used.  A diagnostic: where the
 * end-to-end time of a call went (the sparse download's floor is the host's DRAM write bandwidth, not the GPU). */
void r2s_last_host_phases(double out[8]);
void *r2s_host_alloc(size_t bytes);
void r2s_host_free(void *p);

/* ---- device-resident plan API (bench, multi-GPU Z-slabs) ------------------ */
typedef struct r2s_plan r2s_plan;

int r2s_plan_create(int32_t device, r2s_plan **out);
void r2s_plan_destroy(r2s_plan *plan);

/* mode bits for r2s_plan_run_dev */
#define R2S_OUT_DIST 1 /* d_dist[nvox]            */
#define R2S_OUT_SIGN 2 /* d_sign[nvox]            */
#define R2S_OUT_SDF 4  /* d_sdf[nvox] = dist*sign */
#define R2S_OUT_XP 8   /* d_xp[nvox][3]           */

/* One pass of the hot path over the Z-slab of grid planes [k_begin, k_end):
 * all inputs/outputs are device pointers; outputs hold (k_end-k_begin)*(N1+1)*(N2+1)
 * voxels in the reference's x-fastest order.  Work is enqueued on `stream`
 * (hipStream_t as void*, NULL = default stream).  The FIRST call for a set of shapes waits for the stream twice in the
 * middle (item and list sizes are read back); later calls with the same shapes enqueue everything in one go from the
 * sizes of the previous call (a device-side check falls back to the waiting way when they do not hold) and wait once,
 * at the end, with or without `stats`: the speculated sizes are confirmed on the host there.  See "Streams" above. */
int r2s_plan_run_dev(r2s_plan *plan, const double *dX, int64_t nnp, const int64_t *dIEN, int64_t nel,
                     const double *d_rho_n, double rho_t, const r2s_grid *grid,
                     const r2s_params *params, int64_t k_begin, int64_t k_end, int32_t mode,
                     double *d_dist, double *d_sign, double *d_sdf, double *d_xp, void *stream,
                     r2s_stats *stats);

/* ---- sparse stitching of the volume across GPUs (only non-sentinel tiles travel) ---------------
 * After r2s_plan_run_dev with R2S_OUT_SDF on a tile-layer-aligned Z partition (zstride > 1, or k_begin a
 * multiple of 4), pack the 4x4x4 tiles that can differ from the sentinel -1e10: 64 doubles per tile in
 * lane order (x + 4y + 16z) + the tile id in the whole grid's tile numbering.  Receivers pre-fill their
 * volume with the sentinel (r2s_fill_dev) and scatter every rank's tiles (r2s_unpack_tiles_dev). */
int r2s_plan_pack_tiles_dev(r2s_plan *plan, const double *d_local_sdf, double *d_payload, uint32_t *d_ids,
                            int64_t capacity_tiles, int64_t *n_tiles_out, void *stream);
int r2s_unpack_tiles_dev(const double *d_payload, const uint32_t *d_ids, int64_t n_tiles, const r2s_grid *grid,
                         double *d_volume, void *stream);
int r2s_fill_dev(double *d, int64_t n, double value, void *stream);
/* Compressed variant of the same exchange: tiles with band items (r2s_stats.n_active_tiles) travel as 64
 * doubles; tiles that only carry the sign (r2s_stats.n_sign_only_tiles, every voxel +-1e10) travel as one
 * 64-bit mask (bit l set = voxel l of the tile is +1e10) - 12 B instead of 516 B per tile. */
int r2s_plan_pack_tiles2_dev(r2s_plan *plan, const double *d_local_sdf, double *d_payload, uint32_t *d_ids,
                             int64_t capacity_full, uint64_t *d_masks, uint32_t *d_mask_ids, int64_t capacity_mask,
                             int64_t *n_full_out, int64_t *n_mask_out, void *stream);
int r2s_unpack_masks_dev(const uint64_t *d_masks, const uint32_t *d_mask_ids, int64_t n_tiles, const r2s_grid *grid,
                         double magnitude, double *d_volume, void *stream);

/* The whole exchange buffer of the compressed stitching at once: `world` segments of `seglen` doubles, each
 * [n_full, n_mask as two int64 | cap_full x 64 doubles | cap_full ids (uint32, padded to 8 B) | cap_mask masks |
 * cap_mask mask ids (uint32, padded)].  The counts are read from the segment headers on the device (no host round
 * trip, two launches for all ranks); a segment whose counts exceed the capacities is skipped. */
int r2s_unpack_segments_dev(const double *d_buf, int32_t world, int64_t seglen, int64_t cap_full, int64_t cap_mask,
                            const r2s_grid *grid, double magnitude, double *d_volume, void *stream);

/* ---- pre-stage: mesh volume, nodal densities, volume-preserving threshold ------------- */

/* calculate_mesh_volume(X, IEN, rho, HEX8) -> (V_domain, V_frac)     src/MeshGrid/MeshVolume.jl:4-42 */
int r2s_mesh_volume(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int32_t elem_type,
                    const double *rho_e, int32_t device, double *V_domain, double *V_frac);

/* DenseInNodes(mesh, rho) -> rho_n[nnp]                              src/MeshGrid/NodalDensities.jl:89-218 */
int r2s_dense_in_nodes(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int32_t elem_type,
                       const double *rho_e, int32_t device, double *rho_n_out);

/* find_threshold_for_volume(mesh, rho_n, tol=1e-4, maxit=60) with target = V_domain*V_frac
 *                                                                    src/MeshGrid/Isocontour_volume.jl:77-154
 * returns R2S_ERR_ARG ("outside the possible range", :93-95) like the reference's error(). */
int r2s_find_threshold(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_n,
                       double target_volume, double tol, int32_t maxit, int32_t device, double *rho_t_out,
                       int32_t *iters_out);

/* the same bisection for either element type.  TET4 has no iso-volume in the reference
 * (calculate_isocontour_volume hard-codes 8 nodes, Isocontour_volume.jl:27-38): it is assembled
 * from the reference's own pieces - the skip / whole / cut classification of :40-52 with the collapsed-cube
 * rule of MeshVolume.jl:75-117 (3^3 points for whole elements, 15^3 with the point test for cut ones) - so that
 * volume(0) == V_domain of calculate_mesh_volume for TET4. */
int r2s_find_threshold_et(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int32_t elem_type,
                          const double *rho_n, double target_volume, double tol, int32_t maxit, int32_t device,
                          double *rho_t_out, int32_t *iters_out);

/* calculate_isocontour_volume(mesh, nodal_values, iso_threshold)     src/MeshGrid/Isocontour_volume.jl:1-75 */
int r2s_isocontour_volume(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int32_t elem_type,
                          const double *rho_n, double threshold, int32_t device, double *volume_out);

/* ---- post-processing ---------------------------------------------------------------- */

/* remove_sdf_artifacts!(sdf, grid; threshold, min_component_ratio) -> nodes flipped
 *                                                src/SignedDistances/SdfArtifactRemoval.jl:134-245 */
int r2s_remove_artifacts(double *sdf_inout, const r2s_grid *grid, double threshold, double min_ratio,
                         int32_t device, int64_t *n_flipped);
int r2s_remove_artifacts_dev(double *d_sdf, const r2s_grid *grid, double threshold, double min_ratio,
                             void *stream, int64_t *n_flipped);

/* analyze_sdf_components(sdf, grid; threshold)   src/SignedDistances/SdfArtifactRemoval.jl:256-311
 * The 6-connected components of {sdf >= threshold} (NaN is never interior) as a table with one entry per component in
 * ascending root order: roots_out = the component's 0-based x-fastest linear index of its first (= smallest) voxel,
 * sizes_out = its voxel count.  *n_components is always the full count; the first min(capacity, n) entries are
 * written.  roots_out / sizes_out may be NULL only with capacity == 0 (otherwise R2S_ERR_ARG).  sdf is only read.
 * Differences from the reference: it keys each component by its union-find root (union by rank,
 * SdfArtifactRemoval.jl:41-60), which depends on the union order; here the key is canonical, the component's first
 * voxel.  The partition into components and the multiset of sizes are the same.  An all-exterior field gives n = 0
 * (:263-266); nothing is printed.  Grid limits as for removal (ngp < 2^32 - 1).
 * The _dev variant reads a device field on the current device after the work queued on `stream`; its output pointers
 * are host pointers (like n_flipped of r2s_remove_artifacts_dev).  Every call replaces the calling thread's last table. */
int r2s_analyze_components(const double *sdf, const r2s_grid *grid, double threshold, int32_t device,
                           int64_t *roots_out, int64_t *sizes_out, int64_t capacity, int64_t *n_components);
int r2s_analyze_components_dev(const double *d_sdf, const r2s_grid *grid, double threshold, void *stream,
                               int64_t *roots_out, int64_t *sizes_out, int64_t capacity, int64_t *n_components);
/* the calling thread's last component table (from either call above, or from r2s_rho2sdf with analyze_components and
 * remove_artifacts set), same conventions: ask for the count with capacity 0, then copy without labelling again */
int r2s_last_components(int64_t *roots_out, int64_t *sizes_out, int64_t capacity, int64_t *n_components);

/* calculate_volume_from_sdf(sdf::Array{Float32,3}, grid; iso_threshold, detailed_quad_order)
 *                                                src/SdfSmoothing/CalcVolumeFromSDF.jl:26-125
 * sdf is (nx,ny,nz) x-fastest; edge = spacing of the (cubic-cell) grid. */
int r2s_volume_from_sdf(const float *sdf, int64_t nx, int64_t ny, int64_t nz, float edge, float iso,
                        int32_t quad_order, int32_t device, float *vol_out);

/* RBFs_smoothing(mesh, dist, grid, is_interp, smooth, taskName, threshold=1e-3) -> fine_sdf
 *                                                src/SdfSmoothing/RBFs4Smoothing.jl:321-377
 * target_volume = mesh.V_frac*mesh.V_domain; fine_sdf_out has prod(N*smooth+1) Float32 values
 * (x fastest); fine_grid is origin AABB_min + spacing (AABB_max[1]-AABB_min[1])/(N[1]*smooth) and is
 * materialised by the caller.  Optional outputs: level shift `th`, CG iterations, coarse LSF.
 * Every evaluation of the field sums over at most the 124 nearest in-bounds coarse nodes within the support
 * (knn(kdtree, p, 124) at :238, ties by lattice distance^2 then dz, dy, dx); the CG matrix has no such cap.  The cap
 * binds from kernel_threshold 1e-4 on refined grids and from about 1e-5 on the same grid.
 * kernel_threshold must lie in [R2S_RBF_MIN_KERNEL_THRESHOLD, 1): smaller values give neighbour stencils beyond the
 * 512 entries the kernels hold and fail with R2S_ERR_ARG. */
#define R2S_RBF_MIN_KERNEL_THRESHOLD 1e-10
int r2s_rbf_smooth(const double *sdf, const r2s_grid *grid, int32_t is_interp, int32_t smooth,
                   double kernel_threshold, double target_volume, int32_t device, float *fine_sdf_out,
                   float *level_shift_out, int32_t *cg_iters_out, float *lsf_out);

/* device-resident variant (chaining the stages without PCIe): d_sdf (Float64) and d_fine_out (Float32) are
 * device pointers on the current device; waits for `stream` first, synchronous on return. */
int r2s_rbf_smooth_dev(const double *d_sdf, const r2s_grid *grid, int32_t is_interp, int32_t smooth,
                       double kernel_threshold, double target_volume, float *d_fine_out, float *level_shift_out,
                       int32_t *cg_iters_out, void *stream);

/* A diagnostic of the calling thread's last smoothing (r2s_rbf_smooth / _dev, r2s_rbf_field_fit, the smoothing inside
 * r2s_rho2sdf): which kernels it planned and which tables it built.  All zero before the first one.
 *   [0]  form of the CG's product: 0 row walk, 1 table kernels, 2 materialised matrix, 3 on the fly; -1 in approximation mode
 *   [1]  form of the evaluations: 0 row walk, 1 table kernels, 2 on the fly
 *   [2]  bit 0: a row-walk kernel exists for the stencil and the lattice; bit 1: the knn cap can bind
 *   [3..5]  wavefronts per workgroup, rows per walk, workgroups per row of the product's row walk - also the grouping of the
 *           partial sums of dot(u, K u) under every other form; 0 in approximation mode
 *   [6..8]  the same of the row walk that evaluates the weights on the lattice; 0 when it does not run
 *   [9]  variant slots per axis of the row walk's evaluation tables, 16 or 64, 0 = not built: bits 0-7 of the lattice's own
 *        table, bits 8-15 of the table of the separately rounded output grid at smooth = 1
 *   [10] distinct Float32 coordinate differences ("variants") per axis of the lattice: x in bits 0-7, y in bits 8-15, z in
 *        bits 16-23, each the largest count over the stencil's offsets; 0 = more than a table holds, or not formed
 *   [11] the same between the output grid at smooth = 1 and the lattice
 * R2S_RBF_WALK_NW and R2S_RBF_WALK_L (test hooks, read per call) force the wavefronts per workgroup (1, 2, 3, 5, 9 for the
 * product; 1, 2, 4, 8 for the evaluation) and the rows per walk (4, 8, 16, 32); other values are ignored. */
void r2s_last_rbf_plan(int32_t out[12]);

/* ---- the smoothed level-set as a function: value and gradient at arbitrary points ------------------
 * RBFs_smoothing produces f(p) = th + sum_j w_j exp(-(|p - x_j| / sigma)^2) over the coarse lattice nodes x_j
 * (rbf_interpolation_kdtree takes any array of points, RBFs4Smoothing.jl:219-248; `+ th` at :366).  A field object keeps the
 * weights w and the level shift th of one smoothing on its device.  Objects are independent of the library's caches
 * (r2s_release_cache leaves them alone) and of each other; one object may be read by several threads at once.
 *
 * One evaluation, for a point p with Float32 coordinates (geometry as in r2s_rbf_smooth: Float32 axes of create_grid,
 * sigma = cell_size, max_distance = Float32(sqrt(-ln(threshold) sigma^2))):
 *   - a node takes part when it is in bounds and dist = sqrt(dx*dx + dy*dy + dz*dz) <= max_distance, every operation of
 *     it rounded to Float32 separately (dx = p_x - x_j,x ...), as in the lattice evaluations;
 *   - knn cap (:238): when more than 124 nodes take part by that rule, only the 124 smallest by (dist, linear node index)
 *     do.  (Equal distances at the 124th place leave the reference's own result open; the index rule is this library's.)
 *   - value: the sum of w_j exp(-(dist/sigma)^2) in Float64, rounded to Float32 once, then + th in Float32.  The order of
 *     summation is a fixed function of the point and the field: results do not depend on the point's place in the array.
 *   - gradient: sum_j w_j k_j (-2 / sigma^2) (p - x_j) with the same Float32 differences, in Float64, rounded once.
 *   - taps: the number of nodes that took part, negative (-124) when the cap bound.  (INT32_MIN would report that the
 *     evaluator's per-point list overflowed - an internal error, never a property of the input.)
 *   - a non-finite coordinate: value and gradient NaN, taps 0.  No node in reach: value th, gradient 0, taps 0.
 * Normals: with the Float32 gradient g of the evaluation, -g / |g| (|g| and the quotients in Float64, rounded once):
 * the interior is f >= iso as in r2s_extract_isosurface, so this points outward; (0,0,0) where |g| is 0 or not finite.
 * Projection onto {f = 0}, per point, with the Float32 value f and gradient g of the evaluation at the current p:
 *     it = 0
 *     loop: evaluate f, g at p
 *           |f| <= tol            -> status 0, stop
 *           it == max_iter        -> status 1, stop
 *           g2 = gx*gx + gy*gy + gz*gz in Float64; not (g2 > 0) or not finite -> status 2, stop
 *           s = f / g2;  len = |f| / sqrt(g2);  len > Float32(cell_size): s = s * (Float32(cell_size) / len)   (Float64)
 *           p_a = Float32(p_a - s * g_a) for a = x, y, z (Float64, rounded once);  it = it + 1
 * A non-finite input point has status 3 and stays as it is (resid NaN, iters 0).  resid_out = |f| of the last evaluation,
 * iters_out = steps taken; status_out / resid_out / iters_out may each be NULL.
 * Hessian (r2s_rbf_field_hessian): candidates, Float32 distance, support test, knn cap, exp and weights are those of the
 * evaluation with gradient, and value, gradient and taps are its numbers bit for bit.  With the same Float32 differences
 * d = p - x_j and k_j = exp(-(dist/sigma)^2):
 *     H_ab = sum_j w_j k_j (4 d_a d_b / sigma^4 - 2 delta_ab / sigma^2)
 * as H_aa = 4/sigma^4 s_aa - 2/sigma^2 s and H_ab = 4/sigma^4 s_ab, where s_ab = sum_j w_j k_j d_a d_b and s (the value's
 * own sum) are Float64 sums in the evaluation's fixed order; Float64 throughout, each component rounded to Float32 once.
 * hess_out[n][6] = xx, yy, zz, xy, xz, yz.  A non-finite coordinate: value, gradient and Hessian NaN, taps 0.  No node in
 * reach: value th, gradient 0, Hessian 0.
 * Curvature (r2s_rbf_field_curvature) of the level set through p, oriented by the normal n = -g / |g| (a convex solid has
 * positive mean curvature), in Float64 from the Float32 gradient g and Hessian H of the call above:
 *     g2    = gx*gx + gy*gy + gz*gz
 *     mean  = -(g2 (Hxx + Hyy + Hzz) - g^T H g) / (2 g2 sqrt(g2))
 *     gauss = (g^T adj(H) g) / (g2 g2)                    adj(H): the symmetric matrix of cofactors
 *     disc  = max(mean*mean - gauss, 0);  k1 = mean + sqrt(disc);  k2 = mean - sqrt(disc)
 * curv_out[n][4] = mean, gauss, k1, k2, each rounded to Float32 once (k1, k2 are formed from the Float64 mean and gauss).
 * All four are NaN where g2 is 0 or not finite: non-finite points, points with no node in reach, critical points of f.
 * grad_out / hess_out of the curvature call are the g and H it used.
 *
 * Errors: NULL field / points, negative n, max_iter < 0, tol < 0 or NaN, a threshold outside
 * [R2S_RBF_MIN_KERNEL_THRESHOLD, 1), a grid whose aabb_max is not aabb_min + N * cell_size (to 1e-3 of a cell; grids of
 * r2s_grid_make / r2s_auto_grid are): R2S_ERR_ARG before any device work.  n = 0 succeeds and touches nothing.  Lattices of
 * 2^31 nodes or more, or coordinates so large against cell_size that Float32 cannot separate neighbouring nodes (or, at
 * thresholds near 1e-10, that a support outgrows the evaluator's per-point list): R2S_ERR_UNSUPPORTED.  Host variants make the field's device current; the _dev variants take device pointers on the
 * field's device, which must be the current one, enqueue on `stream` and do not wait. */
typedef struct r2s_rbf_field r2s_rbf_field;

/* process_vector + weights (CG, or the values themselves) + level shift: the numbers r2s_rbf_smooth computes for the same
 * input (its own code path, without the output field), kept on the device */
int r2s_rbf_field_fit(const double *sdf, const r2s_grid *grid, int32_t is_interp, double kernel_threshold,
                      double target_volume, int32_t device, r2s_rbf_field **out, float *level_shift_out,
                      int32_t *cg_iters_out);
/* the same object from given numbers: weights[ngp] Float32, x fastest */
int r2s_rbf_field_from_weights(const float *weights, const r2s_grid *grid, double kernel_threshold, float level_shift,
                               int32_t device, r2s_rbf_field **out);
/* either output may be NULL */
int r2s_rbf_field_weights(const r2s_rbf_field *f, float *weights_out, float *level_shift_out);
void r2s_rbf_field_destroy(r2s_rbf_field *f);

/* points[n][3] Float32; val_out[n], grad_out[n][3], taps_out[n] int32: NULL = not wanted */
int r2s_rbf_field_eval(const r2s_rbf_field *f, const float *points, int64_t n, float *val_out, float *grad_out,
                       int32_t *taps_out);
int r2s_rbf_field_eval_dev(const r2s_rbf_field *f, const float *d_points, int64_t n, float *d_val, float *d_grad,
                           int32_t *d_taps, void *stream);
/* normals_out[n][3] */
int r2s_rbf_field_normals(const r2s_rbf_field *f, const float *points, int64_t n, float *normals_out);
int r2s_rbf_field_normals_dev(const r2s_rbf_field *f, const float *d_points, int64_t n, float *d_normals, void *stream);
/* hess_out[n][6] Float32; any output may be NULL (without hess_out this is r2s_rbf_field_eval) */
int r2s_rbf_field_hessian(const r2s_rbf_field *f, const float *points, int64_t n, float *val_out, float *grad_out,
                          float *hess_out, int32_t *taps_out);
int r2s_rbf_field_hessian_dev(const r2s_rbf_field *f, const float *d_points, int64_t n, float *d_val, float *d_grad,
                              float *d_hess, int32_t *d_taps, void *stream);
/* curv_out[n][4] Float32 is required (NULL: R2S_ERR_ARG); grad_out / hess_out may be NULL */
int r2s_rbf_field_curvature(const r2s_rbf_field *f, const float *points, int64_t n, float *curv_out, float *grad_out,
                            float *hess_out);
int r2s_rbf_field_curvature_dev(const r2s_rbf_field *f, const float *d_points, int64_t n, float *d_curv, float *d_grad,
                                float *d_hess, void *stream);
/* points_inout[n][3] are moved in place */
int r2s_rbf_field_project(const r2s_rbf_field *f, float *points_inout, int64_t n, int32_t max_iter, float tol,
                          int32_t *status_out, float *resid_out, int32_t *iters_out);
int r2s_rbf_field_project_dev(const r2s_rbf_field *f, float *d_points_inout, int64_t n, int32_t max_iter, float tol,
                              int32_t *d_status, float *d_resid, int32_t *d_iters, void *stream);

/* ---- iso-surface extraction ---------------------------------------------------------------
 * The reference's only geometry output is a plot (visualize_stable_isosurface, src/Visualizations/VisualizeIsosurface.jl:
 * Makie's contour!(sdf, levels=[0])).  This is the watertight triangle mesh of {f >= iso} on a regular lattice:
 *   - values: dims[0] x dims[1] x dims[2] points, x fastest, Float32 (is_float32 = 1) or Float64; point (i,j,k) sits at
 *     origin + spacing*(i,j,k).  A point is interior when f >= iso; NaN is exterior.
 *   - one vertex on every lattice edge whose endpoints differ in interiority, at t = (iso - f0)/(f1 - f0) in double from
 *     the lower endpoint (t = 0.5 when an endpoint is not finite), rounded to float32 once; vertices in ascending order
 *     of the edge key 3*p + a (p = 0-based x-fastest index of the lower endpoint, a = 0/1/2 for x/y/z).
 *   - triangles (0-based int32 vertex indices) by cube linear index, then in the order of a 256-case face-consistent
 *     table (tools/gen_iso_table.py: ambiguous faces separate the interior corners), at most 5 per cube; normals
 *     (v1-v0)x(v2-v0) point from the interior to the exterior.  Closed where the interior does not touch the lattice
 *     border; there is no capping and coincident vertices (exact-iso points) are not welded here.  The mesh is topologically
 *     closed as it stands; r2s_mesh_weld merges the coincident vertices on request, which collapses the zero-area triangles
 *     between them and can leave non-manifold edges, which r2s_mesh_shells reports, and non-manifold (pinched) vertices, which
 *     the shells cannot see and r2s_mesh_fans reports and splits - so it is offered, not applied.
 *   - >= 2^31 vertices: R2S_ERR_UNSUPPORTED.  Any dim < 2, a non-positive or non-finite spacing or a NaN iso: R2S_ERR_ARG
 *     before any device work.
 * Host variant: *n_verts / *n_tris are always the full counts; the first min(capacity, n) entries are written (verts_out
 * [n][3] float, tris_out [n][3] int32); pointers may be NULL only with capacity 0.  It replaces the calling thread's last
 * surface, which r2s_last_isosurface reads (same two-step pattern as r2s_analyze_components / r2s_last_components). */
int r2s_extract_isosurface(const void *values, int32_t is_float32, const int64_t dims[3], const double origin[3],
                           double spacing, double iso, int32_t device, float *verts_out, int64_t vert_capacity,
                           int32_t *tris_out, int64_t tri_capacity, int64_t *n_verts, int64_t *n_tris);
int r2s_last_isosurface(float *verts_out, int64_t vert_capacity, int32_t *tris_out, int64_t tri_capacity,
                        int64_t *n_verts, int64_t *n_tris);
/* device field and device outputs on the current device, after the work on `stream`; the counts (host pointers) are
 * always returned, the arrays are written only when both capacities hold everything (count with capacity 0, allocate,
 * call again: the kernels run twice).  Synchronous on return.  Does not touch the thread's last surface. */
int r2s_extract_isosurface_dev(const void *d_values, int32_t is_float32, const int64_t dims[3], const double origin[3],
                               double spacing, double iso, float *d_verts, int64_t vert_capacity, int32_t *d_tris,
                               int64_t tri_capacity, int64_t *n_verts, int64_t *n_tris, void *stream);

/* ---- redistancing: exact banded distance to a triangle mesh -----------------------------------
 * Neither field rho2sdf() returns is a distance function away from the surface (the raw field holds distances within
 * band_factor * cell_size only, the smoothed field is an RBF interpolant).  These entry points compute the Euclidean distance
 * from every point of a regular lattice to an indexed triangle mesh, exact within `band`; no counterpart in the reference.
 *   - lattice: dims[0] x dims[1] x dims[2] points, x fastest; point (i,j,k) sits at p = origin + spacing*(i,j,k), computed in
 *     double (one product, one sum per axis) - the lattice of r2s_extract_isosurface.
 *   - vertices: the given float32 values, widened to double; tris: 0-based int32 vertex indices.
 *   - distance to one triangle (a,b,c) = the minimum of four terms: the distances to the segments a-b, a-c and b-c (the
 *     parameter of the foot point clamped to [0,1]; a zero-length segment is a point), and the plane distance
 *     |n.(p-a)| / |n|, counted only when n = (b-a)x(c-a) is non-zero and p projects into the triangle (the three edge
 *     functions ((b-a)x(p-a)).n, ((c-b)x(p-b)).n, ((a-c)x(p-c)).n are all >= 0).  Zero-area triangles and coincident
 *     vertices are ordinary input (the extraction produces them at exact-iso lattice points); the result is never NaN for
 *     finite input.
 *   - d(p) = the minimum over all triangles; dist_out = min(d, band), Float32 (out_is_float32 = 1) or Float64, formed in
 *     Float64 and rounded once.
 *   - closest_tri_out (may be NULL): the smallest triangle index that attains the computed minimum, -1 where the result is
 *     `band`.  With n_tris == 0 every point gets band / -1.
 *   - the result does not depend on the order of the triangles (the index follows a permutation wherever the minimum is
 *     unique); no floating-point atomics are used.
 * r2s_redistance: out = s * min(d, band) in the type of `values`, with s = +1 where f >= iso and -1 elsewhere (NaN included:
 * the interiority rule of the extraction) and d measured to the mesh r2s_extract_isosurface_dev returns for the same
 * arguments.
 * R2S_ERR_ARG before any device work: any dim < 2; a non-finite or non-positive spacing or band; a non-finite origin; a NaN
 * iso; a triangle index outside [0, n_verts) or a non-finite vertex (the host variant checks on the host, the _dev variant
 * with a check kernel whose verdict is read before anything else runs; the outputs are untouched).  Meshes or lattices
 * beyond 32-bit indices: R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.
 * One device only (`device`, -1 = current; the _dev variants: device pointers on the current device, after the work
 * queued on `stream`, synchronous on return); there is no n_gpus here.  The tile lists are built in batches of tile layers
 * so that they stay under a workspace budget of 1 GiB (environment variable R2S_REDIST_WORKSPACE_MB: another budget in
 * MiB; the result does not depend on it); the work buffers are kept per device (r2s_release_cache frees them). */
int r2s_mesh_distance(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, const int64_t dims[3],
                      const double origin[3], double spacing, double band, int32_t out_is_float32, int32_t device,
                      void *dist_out, int32_t *closest_tri_out);
int r2s_mesh_distance_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris,
                          const int64_t dims[3], const double origin[3], double spacing, double band,
                          int32_t out_is_float32, void *d_dist_out, int32_t *d_closest_tri_out, void *stream);
int r2s_redistance(const void *values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing,
                   double iso, double band, int32_t device, void *out);
int r2s_redistance_dev(const void *d_values, int32_t is_float32, const int64_t dims[3], const double origin[3],
                       double spacing, double iso, double band, void *d_out, void *stream);
/* A diagnostic of the calling thread's last call of the four above: [0] ms surface extraction, [1] ms binning (count, scan,
 * list fills), [2] ms tile kernel (HIP events on the call's stream), [3] tile/triangle pairs tested, [4] batches,
 * [5] triangles, [6] 8x8x8 voxel tiles, [7] tiles with a non-empty list. */
void r2s_last_distance_stats(double out[8]);

/* ---- mesh index: exact point-to-mesh distance without a band ------------------------------------
 * A bounding-volume hierarchy over the triangles of a mesh (one triangle per leaf, float32 boxes, built on the device from
 * Morton codes of the triangles' box centres), and nearest-triangle queries against it: from arbitrary points, or from
 * every point of a lattice.  An index owns device copies of verts / tris and the tree; indices are independent of the
 * library's caches (r2s_release_cache leaves them alone) and of each other; one index may be queried by several threads.
 *   - d(p) = the minimum over ALL triangles of the pair distance defined above for r2s_mesh_distance (vertices: float32
 *     widened to double; points: float32 or float64 widened to double, or the lattice p = origin + spacing*(i,j,k) in
 *     double), formed in Float64 and rounded once to the output type.  The tree only skips triangles whose box is farther
 *     than the current minimum by more than a margin of 2^-40 of the largest coordinate, so the numbers are those of a
 *     search over every triangle, and those of r2s_mesh_distance wherever that result is below its band.
 *   - closest_tri_out (may be NULL): the smallest triangle index that attains the computed minimum.
 *   - an empty mesh (n_tris == 0): +inf / -1 for every point.  A point with a non-finite coordinate: NaN / -1.
 *   - the result depends neither on the order of the triangles (the index follows a permutation wherever the minimum is
 *     unique) nor on the order of the points; no floating-point atomics are used.
 * r2s_mesh_index_build: host arrays, `device` (-1 = current).  _build_dev: device arrays on the current device, read after
 * the work queued on `stream`; both are synchronous on return and copy the mesh.  r2s_mesh_index_info: out[0] triangles,
 * [1] nodes (leaves + internal), [2] tree depth (internal levels; the query refuses a tree deeper than its stack of 64
 * entries, which unique 62-bit keys cannot produce), [3] device bytes held.
 * r2s_mesh_index_query: n points [n][3] from host arrays (synchronous); _query_dev: device arrays on the index's device,
 * which must be current; enqueues on `stream` and does not wait.  n == 0 succeeds and touches nothing.
 * r2s_mesh_index_lattice(_dev): the same for the lattice of r2s_mesh_distance (x fastest); a wavefront takes a 4x4x4 block of
 * lattice points.
 * r2s_redistance_full(_dev): out = s * d in the type of `values`, with s and the mesh exactly as in r2s_redistance and no
 * band: +-inf where the field has no surface.  Synchronous on return.
 * R2S_ERR_ARG before any device work: NULL pointers, a negative count, a triangle index outside [0, n_verts) or a non-finite
 * vertex (host variant: on the host; _build_dev: with the check kernel of r2s_mesh_distance_dev), any dim < 2, a non-finite
 * origin, a non-finite or non-positive spacing, a NaN iso; a _dev call on another device than the index's.  Counts beyond
 * 32 bits: R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.  One device only; there is no n_gpus here. */
typedef struct r2s_mesh_index r2s_mesh_index;
int r2s_mesh_index_build(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t device,
                         r2s_mesh_index **out);
int r2s_mesh_index_build_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, void *stream,
                             r2s_mesh_index **out);
void r2s_mesh_index_destroy(r2s_mesh_index *index);
int r2s_mesh_index_info(const r2s_mesh_index *index, int64_t out[4]);
int r2s_mesh_index_query(const r2s_mesh_index *index, const void *points, int32_t points_are_float32, int64_t n,
                         int32_t out_is_float32, void *dist_out, int32_t *closest_tri_out);
int r2s_mesh_index_query_dev(const r2s_mesh_index *index, const void *d_points, int32_t points_are_float32, int64_t n,
                             int32_t out_is_float32, void *d_dist_out, int32_t *d_closest_tri_out, void *stream);
int r2s_mesh_index_lattice(const r2s_mesh_index *index, const int64_t dims[3], const double origin[3], double spacing,
                           int32_t out_is_float32, void *dist_out, int32_t *closest_tri_out);
int r2s_mesh_index_lattice_dev(const r2s_mesh_index *index, const int64_t dims[3], const double origin[3], double spacing,
                               int32_t out_is_float32, void *d_dist_out, int32_t *d_closest_tri_out, void *stream);
int r2s_redistance_full(const void *values, int32_t is_float32, const int64_t dims[3], const double origin[3],
                        double spacing, double iso, int32_t device, void *out);
int r2s_redistance_full_dev(const void *d_values, int32_t is_float32, const int64_t dims[3], const double origin[3],
                            double spacing, double iso, void *d_out, void *stream);

/* ---- mesh index: first-hit ray queries --------------------------------------------------------
 * What does the ray o + t d hit first?  Against the same index (tree, device copies) as the distance queries.
 *   - rays: origin o and direction d, [n][3] each, both float32 (rays_are_float32 = 1) or both float64, widened to double;
 *     d is NOT normalised by the library, so t is a length only for unit directions.  t_min <= t_max are scalars of the
 *     call; t_max may be +inf.  Vertices: the float32 values widened to double.
 *   - pair test (ray, triangle a b c): the watertight formulation of Woop, Benthin and Wald (2013) in Float64; every
 *     product, sum and quotient is rounded on its own (no fma):
 *       1. kz = the axis of the largest |d| (the lowest axis on ties); kx, ky the next two cyclically, swapped when d[kz] < 0;
 *       2. Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz];
 *       3. A = a - o, Ax = A[kx] - Sx*A[kz], Ay = A[ky] - Sy*A[kz]; the same for B and C;
 *       4. U = Cx*By - Cy*Bx, V = Ax*Cy - Ay*Cx, W = Bx*Ay - By*Ax;
 *       5. rejected if one of U, V, W is < 0 and another > 0 (zeros are accepted on both sides of an edge);
 *       6. det = (U + V) + W; rejected if det == 0;
 *       7. t = ((U*(Sz*A[kz]) + V*(Sz*B[kz])) + W*(Sz*C[kz])) / det.
 *     The sheared coordinates of a vertex depend on the ray and that vertex only, so the edge function of a shared edge is
 *     the exact negative in the neighbouring triangle: a ray cannot slip between two triangles that share an edge.
 *   - in-box condition: the pair is a hit only if t_lo <= t <= t_hi, the ray's parameter interval through the triangle's own
 *     float32 bounding box inflated on every side by m = 2^-40 * max(|o_x|, |o_y|, |o_z|, the largest absolute vertex
 *     coordinate), intersected with [t_min, t_max] (both ends inclusive).  Slab arithmetic, the same for a triangle's box
 *     and a node's: start from [t_min, t_max]; for an axis k with d_k != 0, inv_k = 1/d_k (once per ray),
 *     t1 = ((lo_k - m) - o_k)*inv_k, t2 = ((hi_k + m) - o_k)*inv_k, t_lo = max(t_lo, min(t1, t2)), t_hi = min(t_hi,
 *     max(t1, t2)), min / max as IEEE minNum / maxNum (a NaN from 0 * inf sets no bound); for an axis with d_k == 0 no
 *     bound when lo_k - m <= o_k <= hi_k + m, else the interval is empty.  Rounding is monotone, so the interval of a
 *     node contains those of its leaves: skipping a node whose interval is empty or begins after the best t so far never
 *     removes a pair this definition accepts with t <= best.  The tree is exact, the numbers are those of a loop over all
 *     triangles.  The price: a pair whose computed t leaves its box by more than the margin is a miss, possible only at
 *     near-grazing incidence; measured on the mpmath set of tests/test_ray_cpu.py: no decidable pair was lost, down to the
 *     flattest incidence of the set, |cos| = 1.1e-11 (flatter pairs are undecidable: the projected triangle collapses).
 *   - t_out: the minimum accepted t, formed in Float64 and rounded once to Float32 (out_is_float32 = 1) or Float64 (a
 *     zero is returned as +0); +inf on a miss.  tri_out (may be NULL): the smallest triangle index that attains it, -1 on a miss.  side_out (may be NULL,
 *     int8): the sign of det of that triangle: +1 = the ray runs against the winding normal (b-a)x(c-a) and enters through
 *     the front (det > 0), -1 = it runs with the normal (det < 0), 0 on a miss.
 *   - a ray with a non-finite origin or direction, or a zero direction: NaN / -1 / 0.  An empty mesh: +inf / -1 / 0.
 *   - the results depend neither on the order of the triangles (the index follows a permutation wherever the minimum is
 *     unique) nor on the order of the rays; no floating-point atomics are used.  Nothing here counts crossings: the
 *     inside / outside sign of the mesh is the next section's (r2s_mesh_index_winding).
 * r2s_mesh_index_raycast: host arrays, synchronous.  _raycast_dev: device arrays on the index's device, which must be
 * current; enqueues on `stream` and does not wait.  n == 0 succeeds and touches nothing.
 * R2S_ERR_ARG before any device work, outputs untouched: a NULL index or (n > 0) NULL origins / dirs / t_out, a negative n,
 * a NaN t_min or t_max, t_min > t_max, a _dev call on another device than the index's.  n beyond 32 bits:
 * R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE. */
int r2s_mesh_index_raycast(const r2s_mesh_index *index, const void *origins, const void *dirs, int32_t rays_are_float32,
                           int64_t n, double t_min, double t_max, int32_t out_is_float32, void *t_out, int32_t *tri_out,
                           int8_t *side_out);
int r2s_mesh_index_raycast_dev(const r2s_mesh_index *index, const void *d_origins, const void *d_dirs,
                               int32_t rays_are_float32, int64_t n, double t_min, double t_max, int32_t out_is_float32,
                               void *d_t_out, int32_t *d_tri_out, int8_t *d_side_out, void *stream);

/* ---- mesh index: winding number, inside / outside and signed distance ----------------------------
 * Is this point inside the mesh?  The sign that r2s_redistance takes from a field, taken from the mesh alone, against the same
 * index (tree, device copies) as the distance and ray queries; the index is not changed.  The outputs are integers (and the
 * sign of a distance the existing query returns), defined so that a loop over all triangles gives them bit for bit.
 *   - winding(p) = minus the signed count of crossings of an AXIS ray from p (the sum of `side` below, negated).  ray, int32: 0, 1, 2 = +x, +y, +z; 3, 4, 5 = -x, -y, -z.
 *     Only these six: for them the pair test of r2s_mesh_index_raycast needs no shear, and every cull is an exact comparison.
 *   - pair test (point o, triangle a b c), Float64; vertices are the float32 values widened to double, points float32 or
 *     float64 widened to double (or the lattice point, formed as r2s_mesh_index_lattice forms it); every operation rounded on its
 *     own (no fma):
 *       1. kz = ray % 3; kx = (kz+1) % 3, ky = (kz+2) % 3, swapped for ray >= 3; Sz = +1, or -1 for ray >= 3 (steps 1 and 2 of
 *          the ray test with d = +-e_kz, hence Sx = Sy = 0);
 *       2. A = a - o, Ax = A[kx], Ay = A[ky]; the same for B and C;
 *       3. U = Cx*By - Cy*Bx, V = Ax*Cy - Ay*Cx, W = Bx*Ay - By*Ax (the values step 4 of the ray test forms for this ray);
 *       4. the effective sign of an edge function f belongs to the directed projected edge P -> Q: B -> C for U, C -> A for V,
 *          A -> B for W.  +1 if f > 0, -1 if f < 0; if f == 0: the sign of Qy - Py where that is non-zero, else the sign of
 *          Px - Qx, else 0, with P and Q the vertices' own coordinates q[ky], p[ky], p[kx], q[kx] (float32 values: both
 *          differences are exact).  This is the sign f would take with the point moved by (eps, eps^2) in the projected plane.
 *          The two triangles at a shared edge see exact negatives, in f and in the tie, so a ray through an edge or a vertex
 *          is given to exactly one side;
 *       5. the pair is a crossing iff the three effective signs are equal and non-zero; `side` is that sign;
 *       6. and both of: the own-box condition, all exact comparisons: o[kx] and o[ky] lie in the closed [lo, hi] of the
 *          triangle's own float32 box on those axes, and the box reaches ahead: hi[kz] >= o[kz] for ray < 3, lo[kz] <= o[kz]
 *          for ray >= 3; and det = (U+V)+W is non-zero and t = ((U*(Sz*A[kz]) + V*(Sz*B[kz])) + W*(Sz*C[kz])) / det is > 0.
 *          The inequality is strict: A POINT ON THE SURFACE GETS A RAY-DEPENDENT ANSWER.
 *   - crossings(p) = the number of crossings; winding(p) = - (the sum of `side` over them).  An outward-wound closed body gives
 *     +1 inside and 0 outside; an enclosed void, wound inward, brings the inside of the void back to 0.
 *   - a collapsed triangle (two equal vertex INDICES) takes part in nothing.  A point with a non-finite coordinate: winding 0,
 *     crossings -1.  An empty mesh: 0 / 0.
 *   - why the tree is exact: the own-box condition is part of the definition, float32 min / max do not round, so every
 *     ancestor's box contains the leaf's; entering a child iff the same three comparisons hold on the child's box reaches every
 *     pair of the definition.  No margin, no ordering.  The results follow a permutation of the triangles and of the points
 *     exactly; integer accumulators per point, no atomics.
 *   - known limit: a computed f has the sign of the exact f or is 0 (rounding is monotone), never the opposite sign; where a
 *     computed 0 stands for an exact non-zero the tie rule can decide against the truth, and a ray that passes within rounding
 *     of a vertex can then be miscounted.  tests/mesh_winding_ref.py measures this with exact rational arithmetic.
 *   - inside rules: R2S_INSIDE_POSITIVE (winding > 0), R2S_INSIDE_NONZERO (winding != 0), R2S_INSIDE_ODD (crossings odd; the one
 *     that survives inconsistent winding).
 *   - signed distance = s * d: d exactly what r2s_mesh_index_query / _lattice returns for that point (the same kernel, then
 *     signed in place), s = +1 inside, -1 outside: positive in the material, the convention of r2s_redistance.  A zero is
 *     returned as +0; a non-finite point gives NaN; an empty mesh -inf.  closest_tri_out (may be NULL) as in the query.
 * r2s_mesh_index_winding: n points [n][3] from host arrays (synchronous); crossings_out may be NULL.  _winding_dev: device arrays on
 * the index's device, which must be current; enqueues on `stream` and does not wait.  n == 0 succeeds and touches nothing.
 * r2s_mesh_index_winding_lattice(_dev): the same for the lattice of r2s_mesh_index_lattice (x fastest), by rows: all points of a row
 * along the ray's axis share U, V, W, det and the projected comparisons, and "the box reaches ahead and t > 0" is monotone along
 * the row (every step of t is monotone in o[kz]), so one lane traverses the tree once per row, finds each triangle's threshold
 * index by bisection on that very predicate and adds to difference arrays kept in the outputs, which a second kernel sums.  Equal
 * to the per-point results bit for bit; the environment variable R2S_WINDING_ROWS=0 runs the per-point kernel on 4x4x4 blocks
 * of lattice points instead.  r2s_mesh_index_signed(_dev) / _signed_lattice(_dev): the signed distance, same rules.
 * r2s_mesh_signed_distance / _dev: the signed lattice for a mesh without an index (host arrays and `device`, -1 = current; or
 * device arrays on the current device, after the work queued on `stream`): a tree is built, used and dropped; synchronous.
 * R2S_ERR_ARG before any device work, outputs untouched: a NULL index, NULL arrays with a count, a NULL output, a negative count,
 * ray outside 0..5, rule outside 0..2, the lattice and mesh errors of r2s_mesh_index_lattice / r2s_mesh_index_build, a _dev call
 * on another device than the index's.  R2S_ERR_UNSUPPORTED: counts beyond 32 bits, a tree deeper than the traversal stack (64
 * levels).  No GPU: R2S_ERR_NO_DEVICE.  Not here: arbitrary ray directions, the generalized (solid-angle) winding number for
 * open meshes, voting over rays (call three), repair. */
#define R2S_INSIDE_POSITIVE 0
#define R2S_INSIDE_NONZERO 1
#define R2S_INSIDE_ODD 2
int r2s_mesh_index_winding(const r2s_mesh_index *index, const void *points, int32_t points_are_float32, int64_t n, int32_t ray,
                           int32_t *winding_out, int32_t *crossings_out);
int r2s_mesh_index_winding_dev(const r2s_mesh_index *index, const void *d_points, int32_t points_are_float32, int64_t n,
                               int32_t ray, int32_t *d_winding_out, int32_t *d_crossings_out, void *stream);
int r2s_mesh_index_winding_lattice(const r2s_mesh_index *index, const int64_t dims[3], const double origin[3], double spacing,
                                   int32_t ray, int32_t *winding_out, int32_t *crossings_out);
int r2s_mesh_index_winding_lattice_dev(const r2s_mesh_index *index, const int64_t dims[3], const double origin[3],
                                       double spacing, int32_t ray, int32_t *d_winding_out, int32_t *d_crossings_out,
                                       void *stream);
int r2s_mesh_index_signed(const r2s_mesh_index *index, const void *points, int32_t points_are_float32, int64_t n, int32_t rule,
                          int32_t ray, int32_t out_is_float32, void *dist_out, int32_t *closest_tri_out);
int r2s_mesh_index_signed_dev(const r2s_mesh_index *index, const void *d_points, int32_t points_are_float32, int64_t n,
                              int32_t rule, int32_t ray, int32_t out_is_float32, void *d_dist_out, int32_t *d_closest_tri_out,
                              void *stream);
int r2s_mesh_index_signed_lattice(const r2s_mesh_index *index, const int64_t dims[3], const double origin[3], double spacing,
                                  int32_t rule, int32_t ray, int32_t out_is_float32, void *dist_out, int32_t *closest_tri_out);
int r2s_mesh_index_signed_lattice_dev(const r2s_mesh_index *index, const int64_t dims[3], const double origin[3], double spacing,
                                      int32_t rule, int32_t ray, int32_t out_is_float32, void *d_dist_out,
                                      int32_t *d_closest_tri_out, void *stream);
int r2s_mesh_signed_distance(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, const int64_t dims[3],
                             const double origin[3], double spacing, int32_t rule, int32_t ray, int32_t out_is_float32,
                             int32_t device, void *out);
int r2s_mesh_signed_distance_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris,
                                 const int64_t dims[3], const double origin[3], double spacing, int32_t rule, int32_t ray,
                                 int32_t out_is_float32, void *d_out, void *stream);

/* ---- mesh shells: per-shell topology and mass properties ----------------------------------------
 * What a triangle mesh is: its separate bodies (shells), whether each is closed and consistently oriented, and the area,
 * volume and moments of each.  verts float32 [n_verts][3], tris int32 [n_tris][3], 0-based, as everywhere else.
 *   - collapsed triangle: two of its three vertex INDICES are equal.  It takes no part in edges, shells or sums; its
 *     shell_of_tri is -1; it is counted in the totals.  Coincident coordinates under distinct indices are ordinary input.
 *   - half-edge: corner c of triangle t runs from i_c to i_((c+1)%3); its undirected key is (min << 32) | max.
 *   - edge classes: the half-edges of all non-collapsed triangles, grouped by key.  A group of 1: boundary edge; of exactly
 *     2 in opposite directions: regular; of exactly 2 in the same direction: flipped; of 3 or more: non-manifold.
 *   - shell: a connected component of the graph on the non-collapsed triangles in which two triangles are adjacent when
 *     they share an undirected edge of any class (sharing only a vertex does not join them).  Shells are numbered by
 *     ascending smallest triangle index; shell_of_tri[t] is that number.
 *   - integer record of a shell, int64[8]: [0] first_tri (its smallest triangle index), [1] n_tris, [2] n_verts (distinct
 *     vertex indices its triangles reference; a vertex used by two shells counts in both), [3] n_edges (distinct undirected
 *     edges), [4] n_boundary, [5] n_flipped, [6] n_nonmanifold (edges of that class), [7] 0 (reserved).
 *   - totals, int64[8]: [0] shells, [1] triangles (n_tris), [2] collapsed triangles, [3] distinct edges, [4] boundary,
 *     [5] flipped, [6] non-manifold edges, [7] distinct vertex indices referenced by non-collapsed triangles.
 *   - reference point r: per axis 0.5 * (lo + hi) of the float32 coordinates of ALL n_verts given vertices, lo and hi widened
 *     to double, the sum and the product each rounded in double; (0, 0, 0) when n_verts == 0.  Returned in ref_point.
 *   - Float64 record of a shell, double[11]: [0] area, [1] volume, [2..4] first moments x y z about r, [5..10] second moments
 *     xx yy zz xy xz yz about r: the sums over the shell's triangles (a, b, c) of the terms below.  Every product, sum,
 *     quotient and square root is rounded on its own (no fma); parentheses give the order:
 *       A_i = (double)a_i - r_i, likewise B, C (one subtraction each);      S_i = (A_i + B_i) + C_i;
 *       E = B - A, F = C - A;   N_x = E_y*F_z - E_z*F_y, N_y = E_z*F_x - E_x*F_z, N_z = E_x*F_y - E_y*F_x;
 *       area  = 0.5 * sqrt((N_x*N_x + N_y*N_y) + N_z*N_z);
 *       det   = (A_x*(B_y*C_z - B_z*C_y) + A_y*(B_z*C_x - B_x*C_z)) + A_z*(B_x*C_y - B_y*C_x);
 *       volume = det / 6;       first moment i = (det * S_i) / 24;
 *       second moment ij = (det * (((A_i*A_j + B_i*B_j) + C_i*C_j) + S_i*S_j)) / 120.
 *     A closed, outward-oriented shell has a positive volume; a closed shell of negative volume is an enclosed void.
 *   - summation: no floating-point atomics and no library scan or reduction touch the Float64 sums.  The triangles are sorted
 *     by shell number with a stable sort (ascending triangle index within a shell); blocks of 256 consecutive sorted
 *     triangles are summed per shell in a fixed binary tree (round d = 1, 2, .., 128: position p takes position p + d of its
 *     block when both belong to one shell), then the up to 64 equal runs of a shell's consecutive block partials are summed
 *     in ascending block order and those run sums in a fixed binary tree.  The order is a fixed function of the triangle
 *     order of the input: the same input gives the same bits on every call and from both variants.  The sums are NOT
 *     independent of the triangle order: under a permutation of the triangles the partition, every integer and first_tri
 *     follow the permutation exactly, the sums only to within (n_tris + K) * 2^-53 * T, T the sum of the absolute values
 *     of the term's monomials in A, B, C and K the roundings on its longest chain, a product counting the chains of both
 *     factors (area 8, volume 9, first moments 13, second moments 18; counted in tests/mesh_shells_ref64.py).
 * r2s_mesh_shells: host arrays, `device` (-1 = current); shell_of_tri_out [n_tris] may be NULL.  *n_shells, ref_point and
 * totals are always written on success; the two tables become the calling thread's last result, read with
 * r2s_last_mesh_shells: counts_out [capacity][8], sums_out [capacity][11]; *n_shells is always the full count, the first
 * min(capacity, n) records are written; the pointers may be NULL only with capacity == 0.
 * r2s_mesh_shells_dev: device arrays on the current device, read after the work queued on `stream`; d_shell_of_tri [n_tris]
 * (may be NULL), d_counts [shell_capacity][8] and d_sums [shell_capacity][11] are device pointers, n_shells / ref_point /
 * totals host pointers.  The counts are always returned; the tables are written only when shell_capacity >= *n_shells
 * (else they are left untouched: ask with shell_capacity 0, then call again).  Synchronous on return; it does not touch the
 * thread's last result.  Work buffers are kept per device and freed by r2s_release_cache.
 * R2S_ERR_ARG before anything else runs, outputs untouched: NULL arrays with a count, a negative count, NULL n_shells /
 * ref_point / totals, a triangle index outside [0, n_verts) or a non-finite vertex (host variant: on the host; _dev: the
 * check kernel of r2s_mesh_distance_dev).  n_tris > 2^30 or n_verts beyond 32 bits: R2S_ERR_UNSUPPORTED.  No GPU:
 * R2S_ERR_NO_DEVICE.  n_tris == 0 succeeds with 0 shells.  Not here: which shell encloses which
 * (r2s_mesh_nesting), hole filling; for welding see r2s_mesh_weld below, for the repair of flipped triangles r2s_mesh_orient. */
int r2s_mesh_shells(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t device,
                    int32_t *shell_of_tri_out, int64_t *n_shells, double ref_point[3], int64_t totals[8]);
int r2s_last_mesh_shells(int64_t *counts_out, double *sums_out, int64_t capacity, int64_t *n_shells);
int r2s_mesh_shells_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris,
                        int32_t *d_shell_of_tri, int64_t *d_counts, double *d_sums, int64_t shell_capacity,
                        int64_t *n_shells, double ref_point[3], int64_t totals[8], void *stream);

/* ---- mesh sections: plane contours of a triangle mesh -------------------------------------------
 * Cuts the mesh with the planes h = c_k: per level the contours, whether each is closed, and the length, area vector and first
 * moments of each - cross-section properties along an axis, and the closed loops of every layer.  verts float32 [n_verts][3],
 * tris int32 [n_tris][3], 0-based; normal double[3] (host), finite, not all zero, every |component| <= 2^500 (no height can
 * overflow), NOT normalised by the library; levels double [n_levels] (host), finite and strictly ascending.
 *   - height: h(v) = (n_x*x + n_y*y) + n_z*z with x, y, z widened to double; every product and sum is rounded on its own (no
 *     fma).  With normal = (0, 0, 1) this is z exactly.
 *   - side: vertex v is ABOVE level k iff h(v) >= c_k, else BELOW.  No vertex is ever "on" a plane: this is the whole
 *     degeneracy rule.
 *   - collapsed triangle: two equal vertex INDICES; it takes no part and is counted in the totals.
 *   - crossing: a non-collapsed triangle crosses level k iff its vertices are not all on one side, hmin < c_k <= hmax.  The
 *     crossed levels are a contiguous range of k; in each of them exactly two of the triangle's half-edges change side.
 *   - node: a pair (level k, undirected edge {i, j}, i < j) whose ends are on different sides.  Its point is taken from the
 *     smaller index, whichever triangle asks: t = (c_k - h_i) / (h_j - h_i), p_a = X_i,a + t * (X_j,a - X_i,a) per axis in
 *     double, no fma.  The triangles that share the edge get the same bits, and 0 <= t <= 1.
 *   - segment: one per (triangle, crossed level), directed FROM the node on the half-edge that goes above -> below TO the node
 *     on the half-edge that goes below -> above, walking the corners 0 -> 1 -> 2 -> 0.  On a closed, outward-oriented shell
 *     the material is on the left when seen from the tip of `normal`: outer loops run counter-clockwise, holes clockwise.
 *   - segment id: the position in ascending (triangle index, level).  More than 2^31 - 1 segments: R2S_ERR_UNSUPPORTED.
 *   - node classes, over the segment ends at a node (like the shells' edge classes): one outgoing (FROM) and one incoming (TO)
 *     end: regular; one end: open; two ends of the same kind: flipped; three or more: branch.
 *   - contour: a connected component of the segments of one level, two segments being adjacent when they share a node of any
 *     class.  It is CLOSED iff all its nodes are regular; it is then one simple cycle.  Contours are numbered by ascending
 *     (level, smallest segment id).
 *   - output order of the segments: by contour number; inside a closed contour from its smallest segment id along the
 *     successors (the segment whose FROM node is this one's TO node); inside any other contour in ascending segment id (no
 *     walk is promised there).
 *   - tables: contour_start int64 [n_contours + 1] (output positions); per output position seg_tri int32 and seg_points
 *     double [2][3] (from, to); per contour the integer record int64[8]: [0] level k, [1] first segment id, [2] n_segs,
 *     [3] n_nodes, [4] open, [5] flipped, [6] branch nodes, [7] 0 (reserved); and the Float64 record double[7] about the
 *     shells' reference point r (same definition, returned in ref_point): the sums over the contour's segments of the terms
 *       A = from - r, B = to - r (one subtraction each), D = B - A,
 *       C_x = A_y*B_z - A_z*B_y, C_y = A_z*B_x - A_x*B_z, C_z = A_x*B_y - A_y*B_x,   w = (n_x*C_x + n_y*C_y) + n_z*C_z:
 *       [0] length sqrt((D_x*D_x + D_y*D_y) + D_z*D_z), [1..3] C, [4..6] w * (A_a + B_a),
 *     every operation rounded on its own.  Of a closed contour 0.5 * (n . sum C) / |n| is the signed area (negative: a hole)
 *     and r + sum [4..6] / (3 * n . sum C) the centroid up to its offset along the normal.
 *   - totals, int64[8]: [0] contours, [1] segments, [2] collapsed triangles, [3] nodes, [4] open, [5] flipped, [6] branch
 *     nodes, [7] closed contours.
 *   - summation: the shells' scheme on the output order - blocks of 256 consecutive output positions are summed per contour
 *     in a fixed binary tree (round d = 1, 2, .., 128: position p takes position p + d of its block when both belong to one
 *     contour), then the up to 64 equal runs of a contour's consecutive block partials are summed in ascending block order
 *     and those run sums in a fixed binary tree.  No floating-point atomics and no library reduction; the same input gives the
 *     same bits on every call and from both variants.  Under a permutation of the triangles the points and every integer
 *     follow exactly (a closed loop as a cyclic sequence: its head segment may change), the sums to within
 *     (n_segs + K) * 2^-53 * T, T the sum of the absolute values of the term's monomials in A, B and K the roundings on its
 *     longest chain (length 5, C 4, moments 10; counted in tests/mesh_sections_ref64.py).
 * r2s_mesh_sections: host arrays, `device` (-1 = current).  *n_contours, *n_segments, ref_point and totals are always written
 * on success; the tables become the calling thread's last result, read with r2s_last_mesh_sections: contour_start_out
 * [contour_capacity + 1], counts_out [contour_capacity][8], sums_out [contour_capacity][7], seg_tri_out [segment_capacity],
 * seg_points_out [segment_capacity][2][3]; the counts are always the full ones, the first min(capacity, n) records of each
 * group are written (contour_start: one more); pointers of a group may be NULL only with its capacity == 0.
 * r2s_mesh_sections_dev: d_verts / d_tris and the five tables are device pointers on the current device, read after the work
 * queued on `stream`; normal, levels and the scalar outputs are host pointers.  The counts are always returned; the tables
 * are written only when contour_capacity >= *n_contours and segment_capacity >= *n_segments (else all are left untouched:
 * ask with capacities 0, then call again).  Synchronous on return; it does not touch the thread's last result.  Work buffers
 * are kept per device and freed by r2s_release_cache.
 * R2S_ERR_ARG before anything else runs, outputs untouched: as for r2s_mesh_shells (NULL arrays with a count, a negative
 * count, NULL scalar outputs, a triangle index outside [0, n_verts), a non-finite vertex), and a NULL, non-finite, zero or
 * too large normal, NULL levels with a count, non-finite or not strictly ascending levels, NULL tables with a capacity.
 * n_tris or n_levels > 2^30, n_verts beyond 32 bits: R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.  n_levels == 0 or
 * n_tris == 0 succeeds with nothing.  Not here: which loop lies inside which, infill, offsetting. */
int r2s_mesh_sections(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, const double normal[3],
                      const double *levels, int64_t n_levels, int32_t device, int64_t *n_contours, int64_t *n_segments,
                      double ref_point[3], int64_t totals[8]);
int r2s_last_mesh_sections(int64_t *contour_start_out, int64_t *counts_out, double *sums_out, int64_t contour_capacity,
                           int32_t *seg_tri_out, double *seg_points_out, int64_t segment_capacity, int64_t *n_contours,
                           int64_t *n_segments);
int r2s_mesh_sections_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, const double normal[3],
                          const double *levels, int64_t n_levels, int64_t *d_contour_start, int64_t *d_counts, double *d_sums,
                          int64_t contour_capacity, int32_t *d_seg_tri, double *d_seg_points, int64_t segment_capacity,
                          int64_t *n_contours, int64_t *n_segments, double ref_point[3], int64_t totals[8], void *stream);

/* ---- mesh weld: shared vertices for a triangle soup or a mesh with coincident vertices ---------------
 * Every mesh tool above wants an INDEXED mesh: without shared vertices r2s_mesh_shells reports n_tris shells with three boundary
 * edges each and r2s_mesh_sections finds no closed loop.  The weld turns unindexed triangles (what an STL file holds, see
 * r2s_import_stl) or a mesh with coincident vertices into a mesh whose equal points are one vertex.  Integer and copy work only.
 *   - input: verts float32 [n_verts][3]; tris int32 [n_tris][3], 0-based.  tris == NULL means SOUP: triangle t uses the vertices
 *     3t, 3t + 1, 3t + 2 and there are n_verts / 3 triangles; n_verts % 3 != 0 is R2S_ERR_ARG, and the n_tris argument must then be
 *     0 or n_verts / 3.  (A mesh with vertices and no triangle passes a non-NULL tris with n_tris == 0.)
 *   - which vertices are the same, snap == 0: two vertices are the same iff their x, y and z compare equal as float32.  So
 *     -0.0f == +0.0f, and denormals are ordinary values (nothing is flushed).
 *   - which vertices are the same, snap > 0: iff they fall into the same cell q_a = floor((double)v_a / snap) on every axis a: one
 *     division rounded in double, then floor.  This is GRID SNAPPING, NOT A DISTANCE TOLERANCE: two points closer than snap that
 *     lie on either side of a cell face stay apart, and two points of one cell merge although they may be almost snap * sqrt(3)
 *     apart.  Every q_a must lie in [-2^31, 2^31); otherwise R2S_ERR_ARG ("snap is too fine for the extent"), outputs untouched.
 *     A negative or non-finite snap is R2S_ERR_ARG.
 *   - class, representative, output order: a class is a set of vertices that are the same; its representative is the member with
 *     the smallest input index.  The output vertices are the representatives in ascending input index (first-occurrence order).
 *     Their coordinates are COPIED bit for bit - no averaging, no snapping to a cell centre: every output vertex is an input
 *     vertex (of signed zeros the first one's bits are kept).
 *   - vert_map[i]: the output index of vertex i's class, or -1 if the class was dropped as unreferenced (see the flags).
 *   - triangles are remapped through vert_map; the survivors keep their input order and their corner order.  tri_map[t]: the
 *     output index of triangle t, or -1 if it was dropped.
 *   - collapsed triangle: two of its three remapped indices are equal.  Duplicates: non-collapsed triangles that are equal up to
 *     a rotation of their corners (the same orientation); (a,b,c), (b,c,a), (c,a,b) are duplicates of each other, (a,c,b) is not.
 *   - flags, a bit mask: R2S_WELD_DROP_COLLAPSED (1) drops the collapsed triangles; R2S_WELD_DROP_DUPLICATES (2) keeps, of every
 *     set of duplicates, the one with the smallest input index; R2S_WELD_DROP_UNUSED (4) drops the output vertices that no
 *     surviving triangle references, the rest keep their relative order.  Any other bit: R2S_ERR_ARG.
 *   - totals, int64[8]: [0] output vertices, [1] output triangles, [2] n_verts minus the number of classes (vertices merged
 *     away), [3] collapsed triangles after the weld, counted whether or not they are dropped, [4] same-orientation duplicates
 *     (every member of a duplicate set but its first), counted likewise, [5] opposite pairs: classes of non-collapsed triangles on
 *     the same three vertices that contain both orientations, counted once per class and never dropped, [6] classes that no
 *     surviving triangle references, counted whether or not they are dropped, [7] 0.
 * r2s_mesh_weld: host arrays, `device` (-1 = current).  The outputs are sized by the caller to the INPUT counts (verts_out
 * [n_verts][3], tris_out [n_tris][3], vert_map_out [n_verts], tri_map_out [n_tris]; soup: n_tris = n_verts / 3); only the first
 * totals[0] rows of verts_out and totals[1] rows of tris_out are written.  The two maps may be NULL.
 * r2s_mesh_weld_dev: the same with device pointers on the current device, read after the work queued on `stream`; totals is a
 * host pointer.  Synchronous on return.  The outputs must not overlap the inputs.  Work buffers are kept per device and freed
 * by r2s_release_cache.
 * Refused before any output is touched, as by r2s_mesh_shells: R2S_ERR_ARG for NULL arrays with a count (NULL tris excepted: the
 * soup), NULL outputs with a count or NULL totals, a negative count, a triangle index outside [0, n_verts) or a non-finite vertex
 * (host variant: on the host; _dev: the check kernel of r2s_mesh_distance_dev); n_tris > 2^30 or n_verts >= 2^31:
 * R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.  n_verts == 0 or n_tris == 0 succeed.
 * The same input gives the same output on every call and from both variants (no result depends on an atomic's arrival order).
 * Caveat for meshes of r2s_extract_isosurface: they are topologically closed WITHOUT welding; welding their exact-iso vertices
 * collapses the zero-area triangles between them and can leave non-manifold edges, which r2s_mesh_shells reports, and
 * non-manifold vertices, which only r2s_mesh_fans below reports (the shells join triangles over edges and cannot see a vertex
 * whose triangles fall into several fans); weld, then split with r2s_mesh_fans, gives a mesh whose every vertex is manifold.
 * Not here: distance-tolerance welding; hole filling is r2s_mesh_holes, decimation r2s_mesh_simplify below; flipped triangles are
 * re-oriented by r2s_mesh_orient below. */
#define R2S_WELD_DROP_COLLAPSED 1
#define R2S_WELD_DROP_DUPLICATES 2
#define R2S_WELD_DROP_UNUSED 4
int r2s_mesh_weld(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, double snap, int32_t flags,
                  int32_t device, float *verts_out, int32_t *tris_out, int32_t *vert_map_out, int32_t *tri_map_out,
                  int64_t totals[8]);
int r2s_mesh_weld_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, double snap, int32_t flags,
                      float *d_verts_out, int32_t *d_tris_out, int32_t *d_vert_map_out, int32_t *d_tri_map_out,
                      int64_t totals[8], void *stream);

/* ---- mesh simplify: vertex-clustering decimation ------------------------------------------------
 * The extractor makes one vertex per crossed lattice edge; this makes a mesh coarser.  The vertices are clustered by the weld's
 * cells of edge `cell`, every cluster becomes ONE vertex at a computed position, and the triangles are remapped.
 *   - input: an INDEXED mesh, verts float32 [n_verts][3], tris int32 [n_tris][3], 0-based.  tris == NULL is R2S_ERR_ARG: weld a
 *     soup with r2s_mesh_weld(snap = 0) first.  cell must be positive and finite, else R2S_ERR_ARG.
 *   - classes: the cell of a vertex is the weld's, q_a = floor((double)v_a / cell) per axis with the same division, floor and
 *     -0 == +0; the partition of the vertices is by definition that of r2s_mesh_weld(snap = cell).  Every q_a must lie in
 *     [-2^31, 2^31); otherwise R2S_ERR_ARG with the weld's message, outputs untouched.
 *   - members: the vertices that a non-collapsed INPUT triangle references (collapsed: two equal indices).  Other vertices belong to
 *     no class, count in totals[6] and have vert_map -1.
 *   - triangles are remapped through the classes.  Collapsed ones (two corners in one class) are always dropped; flags takes
 *     R2S_WELD_DROP_DUPLICATES with the weld's meaning and no other bit (else R2S_ERR_ARG); opposite pairs (two sheets pressed onto
 *     each other) are counted and never dropped.  Survivors keep their order and corner order; tri_map[t] is the output index or -1.
 *   - output vertices: one per class that a surviving triangle references, numbered in first-occurrence order of the class's first
 *     (smallest-index) member.  A class none of whose triangles survives (a triangle inside one cell) gives no vertex; its members
 *     have vert_map -1 and count in totals[2].
 *   - ref_point: per axis 0.5 * (min + max) of all vertices, as in r2s_mesh_shells.  All sums are Float64 about ref_point and are
 *     the segmented fixed-order sum of r2s_mesh_shells: the items sorted stably by output class, blocks of 256 consecutive items,
 *     the in-block tree, then the block partials of a class in the combine order stated there.  No fma.
 *   - mean: items = the members, ascending index inside a class, each once; terms (double)v_a - ref_a.  m = sum / count.
 *   - quadric: items = (class, triangle) for every non-collapsed input triangle and every DISTINCT output class among its corners
 *     (a triangle with two corners in one class counts once for it), ascending triangle inside a class.  With A, B, C the corners
 *     about ref_point: e1 = B - A, e2 = C - A, n = e1 x e2 (n_x = e1_y e2_z - e1_z e2_y, cyclic), d = (n_x A_x + n_y A_y) + n_z A_z;
 *     the ten terms n_x n_x, n_x n_y, n_x n_z, n_y n_y, n_y n_z, n_z n_z, d n_x, d n_y, d n_z, d d give the symmetric S, b and c of
 *     E(p) = sum (n . p - d)^2 = p^T S p - 2 b . p + c.
 *   - representative, rule R2S_SIMPLIFY_MEAN: m.  Rule R2S_SIMPLIFY_QUADRIC: S is eigen-decomposed by cyclic Jacobi; directions
 *     with lambda < 1e-3 lambda_max are dropped (Lindstrom); x = m + sum over the kept (V_k . (b - S m) / lambda_k) V_k; if x leaves
 *     the closed cell [q cell, (q + 1) cell] it is pulled back along the segment to m: x = m + s (x - m) with the largest s in
 *     [0, 1] that stays inside (an axis along which |x - m| <= 2^-40 cell constrains nothing: a vertex that sits ON a cell face
 *     must not be "pulled back" by the sign of a rounding error); lambda_max <= 0 (only zero-area triangles): m.  E is convex along that segment, so E(x) <= E(m)
 *     up to rounding.  Then ref_point is added and the result is rounded ONCE to float32.
 *   - per output vertex (r2s_last_mesh_simplify): members, the member count; error, E at the float32 representative as computed in
 *     Float64, p^T (S p) - 2 (b . p) + c (under MEAN too: it says what QUADRIC would gain; it may come out slightly negative by
 *     cancellation); solved, 0 = the mean, 1..3 = the rank kept by the quadric solve, + 4 if the point was pulled back.
 *   - totals, int64[8]: [0] output vertices, [1] output triangles, [2] members minus output vertices (merged away), [3] triangles
 *     collapsed by the clustering, [4] same-orientation duplicates, counted whether or not dropped, [5] opposite pairs, [6] input
 *     vertices that are no member, [7] classes whose representative was pulled back to its cell.
 *   - what clustering can break: manifoldness.  It can create non-manifold edges (r2s_mesh_shells reports them), non-manifold
 *     vertices (r2s_mesh_fans reports and splits them), opposite pairs (totals[5]) and self-contact (r2s_mesh_intersections).  It
 *     opens no hole where no triangle is dropped as a duplicate: a closed input gives a result without boundary edges when it
 *     is consistently oriented or R2S_WELD_DROP_DUPLICATES is off (on a closed but inconsistently wound input, dropping a
 *     same-orientation duplicate can leave an edge with one triangle).  Every vertex moves inside its cell, so every point of
 *     a surviving triangle is within sqrt(3) * cell of its image.
 * r2s_mesh_simplify: host arrays, `device` (-1 = current).  Outputs are sized by the caller to the INPUT counts; only the first
 * totals[0] rows of verts_out and totals[1] rows of tris_out are written.  The two maps may be NULL.
 * r2s_mesh_simplify_dev: the same with device pointers on the current device, read after the work queued on `stream`; totals is a
 * host pointer.  Synchronous on return.  The outputs must not overlap the inputs.  Work buffers are kept per device behind a
 * lock and freed by r2s_release_cache.
 * r2s_last_mesh_simplify: the three tables of the calling thread's last successful call of EITHER variant; *n_verts_out is always
 * the full count, the first min(capacity, n) rows are written; the arrays may be NULL only with capacity == 0.
 * Refused before any output is touched, as by r2s_mesh_weld: R2S_ERR_ARG for NULL arrays with a count, NULL tris, NULL outputs
 * with a count or NULL totals, a negative count, a bad cell, rule or flag bit, a triangle index outside [0, n_verts) or a
 * non-finite vertex (checked before any kernel reads through the indices); 3 * n_tris >= 2^31 or n_verts >= 2^31:
 * R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.  n_verts == 0 or n_tris == 0 succeed with nothing.
 * The same input gives the same output bit for bit on every call, from both variants and with fresh work buffers (no result depends
 * on an atomic's arrival order).  Under a permutation of the input the partition and every integer follow up to the renumbering;
 * the positions do not (the order of the additions changes), the bounds above do.
 * Not here: edge collapse, boundary or feature constraints, attribute transfer. */
#define R2S_SIMPLIFY_MEAN 0
#define R2S_SIMPLIFY_QUADRIC 1
int r2s_mesh_simplify(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, double cell, int32_t rule,
                      int32_t flags, int32_t device, float *verts_out, int32_t *tris_out, int32_t *vert_map_out,
                      int32_t *tri_map_out, int64_t totals[8]);
int r2s_mesh_simplify_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, double cell, int32_t rule,
                          int32_t flags, float *d_verts_out, int32_t *d_tris_out, int32_t *d_vert_map_out,
                          int32_t *d_tri_map_out, int64_t totals[8], void *stream);
int r2s_last_mesh_simplify(int64_t *members_out, double *error_out, int32_t *solved_out, int64_t capacity, int64_t *n_verts_out);

/* ---- mesh orient: consistent, outward triangle winding ------------------------------------------
 * STL files from the wild have facets, or whole bodies, wound the wrong way; r2s_mesh_shells reads a shell's volume sign as
 * "body or void", r2s_mesh_sections promises "material on the left" and the ray `side` reads the winding.  The orient finds the
 * orientable patches of a mesh, gives each a consistent winding and chooses that winding by a stated rule.  verts float32
 * [n_verts][3], tris int32 [n_tris][3], 0-based; collapsed triangles, half-edges and edge groups are those of r2s_mesh_shells.
 *   - patch: a connected component of the non-collapsed triangles in which two triangles are adjacent iff they share an
 *     undirected edge whose group has EXACTLY TWO half-edges, regular or flipped.  Boundary edges and non-manifold edges (three
 *     or more half-edges) join nothing: no partner is defined across them, so patches are finer than shells.  Patches are
 *     numbered by ascending smallest triangle index; patch_of_tri[t] is that number, -1 for a collapsed triangle.
 *   - relative parity: f = the patch's smallest triangle.  Along a regular edge two triangles agree, along a flipped edge they
 *     disagree; the patch is ORIENTABLE iff every cycle agrees, and then rel[t] in {0, 1} is unique with rel[f] = 0.
 *   - a NON-ORIENTABLE patch (a Moebius strip, a Klein bottle): its triangles are copied unchanged, its flip flags are 0, it is
 *     counted.
 *   - a patch is CLOSED iff every half-edge of its triangles lies in a group of exactly two; only then is its volume independent
 *     of the reference point.
 *   - tentative volume V: the sum over the patch's triangles of the shells' `volume` term (same reference point r, same
 *     operation order, no fma), negated where rel[t] = 1.  Swapping corners 1 and 2 negates det exactly in that formula, so this
 *     is the volume of the re-wound patch.
 *   - whole-patch flip g of an orientable patch with n1 triangles of rel = 1 and n0 of rel = 0:
 *         flag R2S_ORIENT_OUTWARD set, the patch closed and V != 0:   g = (V < 0); the patch is "decided by volume"
 *         otherwise (and always without the flag), the MAJORITY:      g = (n1 > n0); a tie gives g = 0: the first triangle
 *                                                                     keeps its winding
 *     Any other flag bit: R2S_ERR_ARG.
 *   - output: flip[t] = rel[t] ^ g.  A flipped triangle (i0, i1, i2) is written as (i0, i2, i1): the first corner is kept, the
 *     triangle order is unchanged.  Collapsed triangles are copied.
 *   - integer record of a patch, int64[8]: [0] first_tri, [1] n_tris, [2] triangles flipped in the output, [3] status bits:
 *     1 closed, 2 non-orientable, 4 decided by volume, [4] its half-edges in boundary groups, [5] its half-edges in non-manifold
 *     groups, [6] flipped edges (groups of two in the same direction) inside it IN THE INPUT, [7] 0.
 *   - Float64 of a patch: its signed volume AS WRITTEN about r: g ? -V : V; of a non-orientable patch the plain sum.
 *   - totals, int64[8]: [0] patches, [1] triangles (n_tris), [2] collapsed, [3] flipped triangles, [4] non-orientable patches,
 *     [5] closed patches, [6] patches decided by volume, [7] flipped edges remaining IN THE OUTPUT: 0 unless a patch is
 *     non-orientable; equal to totals[5] of r2s_mesh_shells on the output mesh.
 *   - NOT HERE.  Nesting is ignored: R2S_ORIENT_OUTWARD makes EVERY closed patch a positive body, so an enclosed void becomes a
 *     body (r2s_mesh_nesting with R2S_NESTING_REWIND on the output reverses the enclosed voids again); the majority rule leaves a void as most of its
 *     triangles say.  That is why OUTWARD is opt-in.  No orientation is carried across non-manifold edges.  No hole filling.
 *   - determinism: no result depends on an atomic's arrival order (the union-find hooks the larger root under the smaller, the
 *     counts are integer sums); no floating-point atomic and no library reduction touches V.  V is summed by the shells' scheme:
 *     the triangles sorted by patch with a stable sort, blocks of 256 consecutive sorted triangles per patch in a fixed binary
 *     tree, then the up to 64 equal runs of a patch's block partials in ascending block order and those run sums in a fixed
 *     binary tree - a fixed function of the triangle order, the same bits on every call and from both variants.  Under a
 *     permutation of the triangles everything follows the permutation, with two exceptions: (1) a majority TIE is broken by the
 *     patch's first triangle, which the permutation may change; (2) V changes within the shells' bound (n_tris + 9) * 2^-53 * T
 *     (T the sum of the absolute values of the volume term's monomials), so where |V| is within that bound of zero the sign
 *     OUTWARD reads, or the fall-through of V == 0 to the majority, may change.
 * r2s_mesh_orient: host arrays, `device` (-1 = current).  tris_out [n_tris][3] is required when n_tris > 0 and must not overlap
 * tris; flip_out [n_tris] (0 / 1) and patch_of_tri_out [n_tris] may be NULL.  *n_patches, ref_point and totals are always
 * written on success; the two tables become the calling thread's last result, read with r2s_last_mesh_orient: counts_out
 * [capacity][8], volume_out [capacity]; *n_patches is always the full count, the first min(capacity, n) records are written; the
 * pointers may be NULL only with capacity == 0.
 * r2s_mesh_orient_dev: device arrays on the current device, read after the work queued on `stream`, which is the only stream the
 * call queues on; d_tris_out, d_flip_out (may be NULL), d_patch_of_tri (may be NULL), d_counts [patch_capacity][8] and d_volume
 * [patch_capacity] are device pointers, n_patches / ref_point / totals host pointers.  d_tris_out, the flips and the patch labels
 * are always written; the tables only when patch_capacity >= *n_patches (else they are left untouched: ask with patch_capacity
 * 0, then call again).  Synchronous on return; it does not touch the thread's last result.  Work buffers are kept per device and
 * freed by r2s_release_cache.
 * R2S_ERR_ARG before any output is touched, as by r2s_mesh_shells: NULL arrays with a count, a negative count, NULL tris_out
 * with a count, NULL n_patches / ref_point / totals, NULL tables with a capacity, a bad flag, a triangle index outside
 * [0, n_verts) or a non-finite vertex (host variant: on the host; _dev: the check kernel of r2s_mesh_distance_dev).  n_tris >
 * 2^30 or n_verts beyond 32 bits: R2S_ERR_UNSUPPORTED, before anything is read.  No GPU: R2S_ERR_NO_DEVICE.  n_tris == 0
 * succeeds with 0 patches. */
#define R2S_ORIENT_OUTWARD 1
int r2s_mesh_orient(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t flags, int32_t device,
                    int32_t *tris_out, int32_t *flip_out, int32_t *patch_of_tri_out, int64_t *n_patches, double ref_point[3],
                    int64_t totals[8]);
int r2s_last_mesh_orient(int64_t *counts_out, double *volume_out, int64_t capacity, int64_t *n_patches);
int r2s_mesh_orient_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, int32_t flags,
                        int32_t *d_tris_out, int32_t *d_flip_out, int32_t *d_patch_of_tri, int64_t *d_counts, double *d_volume,
                        int64_t patch_capacity, int64_t *n_patches, double ref_point[3], int64_t totals[8], void *stream);

/* ---- mesh fans: non-manifold vertices, found and split ------------------------------------------
 * Is every vertex a manifold vertex?  r2s_mesh_shells classifies EDGES; two bodies touching in one point, a surface pinched onto
 * itself in one point or a welded iso-surface that passes through a lattice point have clean edge counts and are still refused by
 * slicers, mesh Booleans and every half-edge structure.  The fans find such vertices and, on request, give every fan its own copy
 * of the vertex: the one repair that never changes geometry.  With the shells this decides "closed 2-manifold": the shells say
 * the edges are regular, the fans say the vertices are (the Euler characteristic and genus of a shell mean something only then).
 * verts float32 [n_verts][3], tris int32 [n_tris][3], 0-based; collapsed triangles, half-edges, undirected keys and edge classes
 * are exactly those of r2s_mesh_shells.  Integer and copy work only: there is no floating-point sum in this tool.
 *   - corner k = 3t + c: corner c of the non-collapsed triangle t; its vertex is v = tris[k].  Its two edges at v are half-edge c
 *     (i_c -> i_((c+1)%3)) and half-edge (c+2)%3 (i_((c+2)%3) -> i_c).  A collapsed triangle has no corners.
 *   - adjacent corners: two corners of the SAME vertex whose triangles share an undirected edge incident to that vertex, of any
 *     class.  All triangles on a non-manifold edge are therefore joined at both of its ends, as the shells join them.
 *   - fan: a connected component of the corners of one vertex.  Fans are numbered by ascending vertex, and within a vertex by
 *     ascending smallest corner id.  fan_of_corner[k] is that number, -1 for the three entries of a collapsed triangle.
 *   - integer record of a fan, int64[8]: [0] vertex, [1] first_corner (its smallest corner id), [2] n_corners (= triangles),
 *     [3] n_edges (distinct undirected edges at the vertex among the fan's triangles), [4] n_boundary, [5] n_flipped,
 *     [6] n_nonmanifold (those edges by class), [7] class: 2 complex if [6] > 0, else 1 open if [4] > 0, else 0 closed.
 *   - invariants: a closed fan is a single cycle, n_edges == n_corners; an open fan is a single path, n_boundary == 2 and
 *     n_edges == n_corners + 1.  (Without non-manifold edges every corner has two distinct edges at v and every edge one or two
 *     corners: a connected graph of degree <= 2.)
 *   - fans_of_vert[v], int32: 0 unused (unreferenced, or referenced by collapsed triangles only), 1 an ordinary vertex (if its
 *     fan is not complex), >= 2 a PINCHED vertex.
 *   - totals, int64[8]: [0] fans, [1] triangles (n_tris), [2] collapsed triangles, [3] used vertices, [4] unused vertices,
 *     [5] pinched vertices (two or more fans), [6] complex fans, [7] open fans.
 *   - split (requested by passing tris_out): the first fan of a vertex keeps index v; every further fan f gets index
 *     n_verts + (the number of non-first fans with a smaller fan number).  n_verts_out = n_verts + fans - used vertices.
 *     verts_out[j] is the source vertex bit for bit; vert_of_out[j] is j for j < n_verts, else the source index;
 *     tris_out[t][c] is the index of the fan of corner 3t + c.  Collapsed triangles and unused vertices are copied unchanged;
 *     triangle order and winding are untouched.
 *   - consequences.  No undirected edge is merged or divided by the split, because all corners of v on an edge (v, w) are in one
 *     fan.  On the output mesh r2s_mesh_shells therefore gives the same shell_of_tri, the same edge counts and classes, the same
 *     ref_point and bit-equal Float64 sums; only the vertex counts grow: totals[7] by n_verts_out - n_verts, and n_verts of a
 *     shell to the number of its fans (a shell pinched onto itself gains a vertex; a vertex at which two shells touch was
 *     counted in both already, so neither gains one).  The split is idempotent: on its output fans_of_vert <= 1 everywhere and a second split adds nothing.  Complex fans are NOT
 *     repaired: non-manifold edges stay.
 *   - determinism: the union-find hooks the larger root under the smaller, the counts are integer sums; no result depends on an
 *     atomic's arrival order.  Under a permutation of the triangles the partition follows exactly, and so does every record
 *     once first_corner is mapped.
 * r2s_mesh_fans: host arrays, `device` (-1 = current).  fan_of_corner_out [n_tris][3] and fans_of_vert_out [n_verts] may be NULL.
 * The split is written when tris_out [n_tris][3], verts_out [vert_capacity][3] and vert_of_out [vert_capacity] are given (all
 * three or none; with n_tris == 0 tris_out may be NULL) AND vert_capacity >= *n_verts_out; otherwise the three are left untouched
 * (ask without them, then call again).  *n_fans, *n_verts_out and totals are always written on success; the records become the
 * calling thread's last result, read with r2s_last_mesh_fans: counts_out [capacity][8]; *n_fans is always the full count, the
 * first min(capacity, n) records are written; counts_out may be NULL only with capacity == 0.
 * r2s_mesh_fans_dev: device arrays on the current device, read after the work queued on `stream`, which is the only stream the
 * call queues on; d_fan_of_corner, d_fans_of_vert (both may be NULL), d_counts [fan_capacity][8] and the three split outputs are
 * device pointers, n_fans / n_verts_out / totals host pointers.  The counts are always returned; the records are written only
 * when fan_capacity >= *n_fans, the split only when vert_capacity >= *n_verts_out (else they are left untouched: ask, then call
 * again).  Synchronous on return; it does not touch the thread's last result.  Work buffers are kept per device and freed by
 * r2s_release_cache.
 * R2S_ERR_ARG before any output is touched, as by r2s_mesh_shells: NULL arrays with a count, a negative count or capacity, NULL
 * n_fans / n_verts_out / totals, NULL records with a capacity, tris_out without verts_out / vert_of_out (or the reverse), an
 * output that overlaps an input, a triangle index outside [0, n_verts) or a non-finite vertex (host variant: on the host; _dev:
 * the check kernel of r2s_mesh_distance_dev).  3 * n_tris >= 2^31, n_verts beyond 32 bits or an *n_verts_out beyond them:
 * R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.  n_tris == 0 succeeds with 0 fans and, under the split, the vertices copied.
 * Not here: splitting along non-manifold edges, anything geometric; hole filling is r2s_mesh_holes below. */
int r2s_mesh_fans(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t device,
                  int32_t *fan_of_corner_out, int32_t *fans_of_vert_out, int32_t *tris_out, float *verts_out,
                  int32_t *vert_of_out, int64_t vert_capacity, int64_t *n_fans, int64_t *n_verts_out, int64_t totals[8]);
int r2s_last_mesh_fans(int64_t *counts_out, int64_t capacity, int64_t *n_fans);
int r2s_mesh_fans_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, int32_t *d_fan_of_corner,
                      int32_t *d_fans_of_vert, int64_t *d_counts, int64_t fan_capacity, int32_t *d_tris_out, float *d_verts_out,
                      int32_t *d_vert_of_out, int64_t vert_capacity, int64_t *n_fans, int64_t *n_verts_out, int64_t totals[8],
                      void *stream);

/* ---- mesh holes: boundary loops, found, measured and capped ---------------------------------------
 * Where is the mesh open, how large is each opening, and can it be closed?  r2s_mesh_shells COUNTS boundary edges; the winding
 * number, the OUTWARD rule and the signed distance mean something only on closed shells, and an STL with one missing triangle is
 * not one.  The holes report the RIMS of a mesh - its boundary loops and chains - and, on request, return a mesh in which every
 * selected closed rim is capped.  verts float32 [n_verts][3], tris int32 [n_tris][3], 0-based; collapsed triangles, half-edges,
 * undirected keys and edge classes are exactly those of r2s_mesh_shells.
 *   - boundary half-edge: half-edge h = 3t + c of a non-collapsed triangle whose undirected edge group has exactly one half-edge.
 *     It runs FROM tris[3t + c] TO tris[3t + (c + 1) % 3].
 *   - node: a vertex that is an end of at least one boundary half-edge.  Its class is taken over the ends at the vertex (a FROM
 *     end is outgoing, a TO end incoming), worded like the sections' classes: one outgoing and one incoming end REGULAR, one end
 *     OPEN, two ends of the same kind FLIPPED, three or more ends BRANCH.
 *   - rim: a connected component of the boundary half-edges; two are adjacent when they share a node of any class.  A rim is
 *     CLOSED iff all its nodes are regular; it is then one simple cycle of distinct vertex indices with n_edges == n_nodes >= 3
 *     (every node has one way in and one way out; a cycle of two would be one undirected edge with two half-edges, which is not
 *     a boundary edge).  Rims are numbered by ascending smallest half-edge id.
 *   - output order: inside a closed rim, from its smallest half-edge id along the successors (the successor of a half-edge is the
 *     half-edge whose FROM is this one's TO); inside any other rim, ascending half-edge id - no walk is promised there.
 *   - tables: rim_start int64 [n_rims + 1]; rim_edge int32 per output position, the half-edge id; per rim the integer record
 *     int64[8]: [0] first half-edge id, [1] n_edges, [2] n_nodes, [3] open, [4] flipped, [5] branch nodes, [6] status (0 not
 *     closed, 1 closed and not filled, 2 filled with one triangle, 3 filled with a fan), [7] index of the added vertex or -1;
 *     per rim the Float64 record double[7] about the shells' reference point r (the same definition, returned in ref_point):
 *     [0] length = sum sqrt((Dx Dx + Dy Dy) + Dz Dz), [1..3] sum A x B = (Ay Bz - Az By, Az Bx - Ax Bz, Ax By - Ay Bx),
 *     [4..6] sum A, with A = from - r, B = to - r, D = B - A, each coordinate widened to double; every operation is rounded on
 *     its own (no fma).  Of a closed rim 0.5 |sum A x B| is the area of its vector-area projection and r + sum A / n_edges the
 *     mean of its vertices.
 *   - summation: the sections' scheme on the output order.  Blocks of 256 consecutive output positions (block j = positions
 *     [256 j, 256 j + 256) of the whole table; a rim's first and last block may be shared with its neighbours, whose terms do
 *     not enter) are summed in a fixed binary tree: in round d = 1, 2, .., 128 position p takes position p + d when that lies in
 *     the same block and rim.  The nb block partials of a rim are cut into up to 64 runs of ceil(nb / 64) consecutive partials,
 *     each summed in ascending order; the run sums are joined in a fixed tree (round d = 1, 2, .., 32: run l takes run l + d).
 *     No floating-point atomic, no library reduction: the same input gives the same bits on every call and from both variants.
 *     Each sum is within (n_edges + K) 2^-53 T of the exact sum of the exact terms, T = the sum of the absolute values of the
 *     term's monomials, K = 5 (length), 4 (A x B), 1 (A): the roundings on the term's longest chain.
 *   - totals, int64[8]: [0] rims, [1] boundary half-edges, [2] collapsed triangles, [3] nodes, [4] open + flipped + branch nodes,
 *     [5] closed rims, [6] filled rims, [7] added triangles.
 *   - fill (requested by passing tris_out and verts_out): max_edges selects the rims - negative: every closed rim, 0: none,
 *     k > 0: the closed rims with n_edges <= k.  A selected rim of exactly 3 edges a -> b -> c -> a (a -> b its first half-edge)
 *     gets the one triangle (b, a, c) and no new vertex.  A longer selected rim gets one new vertex w and n_edges triangles
 *     (b, a, w), one per boundary half-edge a -> b, in output order.  w is computed per axis as r_a + S_a / n_edges in double
 *     (S = the rim's [4..6]; one division, one addition) and rounded to the nearest float32.  Added vertices follow the input
 *     vertices in rim order, added triangles follow the input triangles in rim order; input vertices and triangles are copied
 *     unchanged, bit for bit.  Non-closed rims are never filled.  Status and added vertex of the records, n_verts_out,
 *     n_tris_out and totals[6..7] state the selection whether or not the outputs had room; without a fill request nothing is
 *     selected.
 *   - consequences.  The cap of a rim is wound against it: every boundary half-edge a -> b of a filled rim meets exactly one new
 *     half-edge b -> a, so every filled boundary edge becomes a regular edge; every added edge {a, w} has exactly two opposite
 *     half-edges (a -> w from the triangle of the boundary half-edge that leaves a, w -> a from the one that arrives at a); no
 *     other edge gains or loses a half-edge.  On the output mesh r2s_mesh_shells therefore reports the boundary-edge total lower
 *     by exactly the filled edges, unchanged flipped and non-manifold totals and an unchanged shell_of_tri for the input
 *     triangles; r2s_mesh_fans reports one closed fan at each w and unchanged fans_of_vert at the input vertices.  The fill is
 *     idempotent under the same max_edges: the filled rims are gone, the others are untouched.
 *   - determinism: the union-find hooks the larger root under the smaller, the counts are integer sums, the Float64 sums have a
 *     fixed order; no result depends on an atomic's arrival order.  Under a permutation of the triangles or a rotation of their
 *     corners the partition and every integer follow once the half-edge ids are mapped; a closed rim is the same cycle from
 *     another start, so its sums may differ by the bound above.
 * r2s_mesh_holes: host arrays, `device` (-1 = current).  The fill is asked for by tris_out [tri_capacity][3] and verts_out
 * [vert_capacity][3] (both or none); verts_out is written when vert_capacity >= *n_verts_out, tris_out when tri_capacity >=
 * *n_tris_out, otherwise that array is left untouched (ask, then call again).  *n_rims, *n_edges (boundary half-edges),
 * *n_verts_out, *n_tris_out, ref_point and totals are always written on success; the tables become the calling thread's last
 * result, read with r2s_last_mesh_holes: rim_start_out [rim_capacity + 1], counts_out [rim_capacity][8], sums_out
 * [rim_capacity][7], rim_edge_out [edge_capacity]; the counts are always the full ones, the first min(capacity, n) entries of
 * each group are written (rim_start_out: one more); a group may be NULL only with capacity == 0.
 * r2s_mesh_holes_dev: device arrays on the current device, read after the work queued on `stream`, which is the only stream the
 * call queues on; the tables and the two fill outputs are device pointers, the counts, ref_point and totals host pointers.  The
 * counts are always returned; each group is written only when its capacity suffices - d_rim_start [rim_capacity + 1], d_counts
 * and d_sums when rim_capacity >= *n_rims, d_rim_edge when edge_capacity >= *n_edges, d_verts_out when vert_capacity >=
 * *n_verts_out, d_tris_out when tri_capacity >= *n_tris_out - else it is left untouched.  Synchronous on return; it does not
 * touch the thread's last result.  Work buffers are kept per device and freed by r2s_release_cache.
 * R2S_ERR_ARG before any output is touched, as by r2s_mesh_fans: NULL arrays with a count, a negative count or capacity, NULL
 * count / ref_point / totals pointers, NULL tables with a capacity, tris_out without verts_out (or the reverse), an output that
 * overlaps an input, a triangle index outside [0, n_verts) or a non-finite vertex (host variant: on the host; _dev: the check
 * kernel of r2s_mesh_distance_dev).  3 * n_tris >= 2^31, n_verts beyond 32 bits or an *n_verts_out beyond them:
 * R2S_ERR_UNSUPPORTED.  No GPU: R2S_ERR_NO_DEVICE.  n_tris == 0 succeeds with nothing and, under the fill, the vertices copied.
 * Not here: a pinched boundary vertex (two holes touching in a point) is a branch node and blocks the fill - the fans' split
 * makes it regular, so the recipe is weld -> orient -> split -> fill; rims through flipped nodes need the orient first; a fan cap
 * of a non-planar or non-star-shaped rim can intersect the surface, and r2s_mesh_intersections is the check.  Not offered:
 * filling only the rims a user names, planar caps with nesting (an iso-surface cut by the lattice border), caps without a
 * Steiner point, refinement or fairing of a cap. */
int r2s_mesh_holes(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t device, int64_t max_edges,
                   int32_t *tris_out, float *verts_out, int64_t vert_capacity, int64_t tri_capacity, int64_t *n_rims,
                   int64_t *n_edges, int64_t *n_verts_out, int64_t *n_tris_out, double ref_point[3], int64_t totals[8]);
int r2s_last_mesh_holes(int64_t *rim_start_out, int64_t *counts_out, double *sums_out, int64_t rim_capacity, int32_t *rim_edge_out,
                        int64_t edge_capacity, int64_t *n_rims, int64_t *n_edges);
int r2s_mesh_holes_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris, int64_t max_edges,
                       int64_t *d_rim_start, int64_t *d_counts, double *d_sums, int64_t rim_capacity, int32_t *d_rim_edge,
                       int64_t edge_capacity, int32_t *d_tris_out, float *d_verts_out, int64_t vert_capacity, int64_t tri_capacity,
                       int64_t *n_rims, int64_t *n_edges, int64_t *n_verts_out, int64_t *n_tris_out, double ref_point[3],
                       int64_t totals[8], void *stream);

/* ---- mesh index: self-intersection pairs --------------------------------------------------------
 * Does the surface pass through itself?  The shells' volume and "void" verdict, OUTWARD orientation, "material on the left" of a
 * section and the wall thickness all read the mesh as an embedded surface; this is the check that says whether they may.  For
 * every unordered pair of triangles of ONE mesh that intersect or touch: the pair, the number of such pairs per triangle, and
 * totals.  Against the same index (tree, device copies) as the distance and ray queries; the index is not changed.
 * Vertices: the float32 values widened to double.  Every product, sum, difference and quotient is rounded on its own (no fma).
 *   - collapsed triangle: two of its three vertex INDICES are equal.  It takes part in no pair and is counted (totals[5]).
 *   - box of a triangle: per axis the float32 min and max of its three vertices.
 *   - candidate pair (s, t): s < t, both non-collapsed, and the closed boxes overlap on all three axes:
 *     lo_s[k] <= hi_t[k] && lo_t[k] <= hi_s[k] for k = x, y, z, compared in float32.
 *   - shared indices of a candidate pair = the number of corners of s whose vertex index is also a corner of t:
 *       2 or 3: the pair is skipped and counted as adjacent (totals[3]).  Edge neighbours and duplicates always touch; a fold of a
 *               triangle onto its edge neighbour is coplanar and out of scope.
 *       1 (the index v): two segment tests: the edge of s opposite v against t, and the edge of t opposite v against s.  (The
 *               edges through v meet the other triangle at v by construction.)  Counted in totals[4].
 *       0: six segment tests: the three edges of s against t and the three edges of t against s.
 *     Edge c of a triangle (c = 0, 1, 2) runs from its corner c to its corner (c + 1) % 3, in that direction; the edge opposite
 *     corner c is edge (c + 1) % 3.
 *   - segment test (edge p -> q, triangle a b c): the ray pair test of r2s_mesh_index_raycast above, steps 1 to 7, with o = p
 *     and d = q - p (one subtraction per component, in double).  No box condition, no t_min / t_max.  A hit requires all of: not
 *     rejected by step 5, det != 0, and 0 <= t <= 1 (both ends inclusive).  d == 0 in all three components: no hit.
 *   - the pair is INTERSECTING iff any of its segment tests hits.  The predicate uses only the two triangles' own data and does
 *     not depend on which of them is s: under a permutation of the triangles the result follows the permutation exactly.  (No
 *     claim is made under a rotation of a triangle's corners: the edges' directions change.)
 *   - consequences.  A segment parallel to the triangle's plane has det == 0 and never hits: COPLANAR OVERLAP IS NOT REPORTED.
 *     CONTACT COUNTS: a vertex on a face, an edge through an edge, coincident coordinates under different indices all hit.  An
 *     unwelded triangle soup therefore reports every neighbour of every triangle: WELD FIRST (r2s_mesh_weld), so that
 *     neighbours share indices.  A zero-area triangle with distinct indices is ordinary input (its plane tests have det == 0;
 *     its edges are still tested against others).
 *   - hits_of_tri[t], int32: the number of intersecting pairs that contain t.
 *   - pairs [n][2], int32: s < t, sorted ascending by (s, t).
 *   - totals, int64[8]: [0] intersecting pairs, [1] triangles in at least one intersecting pair, [2] candidate pairs, [3]
 *     candidate pairs skipped as adjacent, [4] candidate pairs sharing exactly one index, [5] collapsed triangles, [6], [7] 0.
 *   - why the tree is exact: two triangles with a common point have overlapping closed boxes, and a node's box is the exact
 *     float32 min / max of its leaves' boxes, so every ancestor of t overlaps the box of s too: entering every node whose box
 *     overlaps the box of s reaches every candidate pair.  The results are those of a loop over all pairs s < t, bit for bit.
 *     All outputs are integers, no floating-point value leaves the call, nothing depends on the traversal order or on the
 *     arrival order of an atomic (integer atomics only; the pair list is sorted).
 * r2s_mesh_index_intersections: host arrays; hits_of_tri_out [n_tris] may be NULL.  totals is always written on success.  The
 * pair list is written only when pair_capacity >= totals[0]; otherwise pairs_out is left untouched: ask with pair_capacity 0,
 * then call again.  pairs_out may be NULL only with pair_capacity == 0.
 * r2s_mesh_index_intersections_dev: d_hits_of_tri (may be NULL) and d_pairs are device pointers on the index's device, which must
 * be current; totals is a host pointer.  Reads after the work queued on `stream`, runs its own work on `stream`, and is
 * synchronous on return (the count comes back on the host).
 * r2s_mesh_intersections / _dev: the same for a mesh without an index (host arrays and `device`, -1 = current; or device arrays
 * on the current device): a tree is built, used and dropped.
 * Work buffers are kept per device and freed by r2s_release_cache.  An empty mesh succeeds with zeros.
 * R2S_ERR_ARG before any device work, outputs untouched: a NULL index, NULL totals, NULL arrays with a count, NULL pairs with a
 * capacity, a negative count or capacity, a triangle index outside [0, n_verts) or a non-finite vertex (host variant: on the
 * host; _dev: the check kernel of r2s_mesh_distance_dev), an index on another device than the current one (_dev).
 * R2S_ERR_UNSUPPORTED: a tree deeper than the traversal stack (64 levels), more than 2^31 - 1 intersecting pairs.  No GPU:
 * R2S_ERR_NO_DEVICE.  Not here: coplanar overlap and fold-overs between edge neighbours, intersections between two different
 * meshes, the intersection curve, repair.  The inside / outside sign: r2s_mesh_index_winding. */
int r2s_mesh_index_intersections(const r2s_mesh_index *index, int32_t *hits_of_tri_out, int32_t *pairs_out,
                                 int64_t pair_capacity, int64_t totals[8]);
int r2s_mesh_index_intersections_dev(const r2s_mesh_index *index, int32_t *d_hits_of_tri, int32_t *d_pairs,
                                     int64_t pair_capacity, int64_t totals[8], void *stream);
int r2s_mesh_intersections(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t device,
                           int32_t *hits_of_tri_out, int32_t *pairs_out, int64_t pair_capacity, int64_t totals[8]);
int r2s_mesh_intersections_dev(const float *d_verts, int64_t n_verts, const int32_t *d_tris, int64_t n_tris,
                               int32_t *d_hits_of_tri, int32_t *d_pairs, int64_t pair_capacity, int64_t totals[8],
                               void *stream);

/* ---- mesh nesting: which closed patch encloses which, voids by depth ------------------------------
 * Is this void enclosed, and in which body?  r2s_mesh_shells calls a closed shell of negative volume a void without asking what
 * encloses it, and r2s_mesh_orient(OUTWARD) makes every closed patch a positive body.  The nesting is the containment forest of
 * the orient's patches, found with the exact axis-ray pair test of r2s_mesh_index_winding through the tree of the mesh index.
 * All outputs are integers, defined so that a loop over all (patch, triangle) pairs gives them bit for bit.  verts float32
 * [n_verts][3], tris int32 [n_tris][3], 0-based.
 *   - patches: collapsed triangles, half-edges, edge groups, patches, patch_of_tri and "closed patch" are exactly those of
 *     r2s_mesh_orient, with the same numbering (ascending smallest triangle index; -1 for a collapsed triangle).  No orientation
 *     is needed and none is read: the tool works on inconsistently wound input.
 *   - sample of a patch P: the float32 vertex at corner 0 of P's first (smallest-index) triangle, widened to double.
 *   - cross(P, Q), for a patch P and a CLOSED patch Q != P: the number of triangles of Q that are a crossing of the axis ray
 *     `ray` (0..5 as in r2s_mesh_index_winding) from P's sample, by steps 1 to 6 of that section: the effective signs with the
 *     tie rule, the own-box condition, det != 0, t > 0, every operation rounded on its own (no fma).  `side` is not used, only
 *     the parity counts.  Triangles of P itself, of open patches, and collapsed triangles take part in nothing.
 *   - containment: Q contains P iff cross(P, Q) is odd.  Every patch, open or closed, is a query; only closed patches are
 *     containers.
 *   - depth(P) = the number of containers of P.  parent(P) = the container of the largest depth, among equals the smallest patch
 *     number, -1 without a container.
 *   - P is IRREGULAR iff depth(P) > 0 and depth(parent(P)) != depth(P) - 1: its containers are not a chain, so patches pass
 *     through each other (r2s_mesh_index_intersections says where).
 *   - integer record of a patch, int64[8]: [0] first_tri, [1] n_tris, [2] status bits: 1 closed, 2 reversed in the output, 4
 *     irregular, [3] parent, [4] depth, [5] n_children, the number of patches whose parent it is, [6] the sum of cross(P, Q) over
 *     all closed Q != P, [7] 0.
 *   - totals, int64[8]: [0] patches, [1] triangles (n_tris), [2] collapsed, [3] closed patches, [4] containment pairs, equal to
 *     the sum of the depths, [5] the largest depth, [6] irregular patches, [7] triangles reversed in the output.
 *   - pair list: all (query, container) pairs as int64 (P << 32) | Q, sorted ascending.
 *   - flag R2S_NESTING_REWIND: tris_out receives the input triangles in their order, every triangle of a closed patch at ODD
 *     depth written (i0, i2, i1), everything else copied.  This is relative to the input: applied to the output of
 *     r2s_mesh_orient(OUTWARD) it yields positive bodies and negative voids, alternating with depth.  Without the flag tris_out
 *     may be NULL and is not written, no status has bit 2 and totals[7] is 0.  Any other flag bit: R2S_ERR_ARG.
 *   - why the tree is exact: the argument of r2s_mesh_index_winding carries over.  The own-box condition is part of the pair
 *     test, float32 min / max do not round, so every ancestor's box contains the leaf's; entering a child iff the same three
 *     comparisons hold on the child's box reaches every crossing of the definition.  The tree holds all triangles; whose they are
 *     is decided at the leaf.
 *   - limits: a sample that lies on another patch gets a ray-dependent answer (t > 0 is strict); the known rounding limit of the
 *     tie rule applies as stated there; a patch with a non-manifold or boundary edge is never a container: weld, split and fill
 *     first; one ray per call.  Not here: voting over rays, nesting of open surfaces, repair of irregular patches.
 *   - determinism: integer work only; the only atomics are integer adds and the cursor of the crossing list, which is sorted
 *     afterwards; nothing depends on an arrival order.  Under a permutation of the triangles every output follows the
 *     permutation, through the renumbering of the patches.  No claim is made under a rotation of a triangle's corners: the sample
 *     changes.
 * r2s_mesh_nesting: host arrays, `device` (-1 = current); a tree is built, used and dropped.  tris_out [n_tris][3] is required
 * with R2S_NESTING_REWIND when n_tris > 0 and must not overlap tris; patch_of_tri_out [n_tris] may be NULL.  *n_patches and
 * totals are always written on success; the records and the pair list become the calling thread's last result, read with
 * r2s_last_mesh_nesting: counts_out [capacity][8], pairs_out [pair_capacity]; *n_patches and *n_pairs are always the full counts,
 * the first min(capacity, n) records and min(pair_capacity, m) pairs are written; a pointer may be NULL only with its capacity 0.
 * r2s_mesh_nesting_dev: device arrays on the current device, read after the work queued on `stream`, which is the only stream the
 * call queues on.  index: an r2s_mesh_index of the SAME mesh on the current device, used and left unchanged (its triangle count
 * must be n_tris, else R2S_ERR_ARG), or NULL: a tree is built and dropped.  d_tris_out (with the flag), d_patch_of_tri (may be
 * NULL), d_counts [patch_capacity][8] and d_pairs [pair_capacity] are device pointers; n_patches, n_pairs and totals host
 * pointers, always written on success.  The triangles and the patch labels are always written; the records only when
 * patch_capacity >= *n_patches and the pairs only when pair_capacity >= *n_pairs (else that table is left untouched: ask with
 * capacity 0, then call again).  Synchronous on return; it does not touch the thread's last result.  Work buffers are kept per
 * device and freed by r2s_release_cache.
 * R2S_ERR_ARG before any output is touched, as by r2s_mesh_orient: NULL arrays with a count, a negative count or capacity, ray
 * outside 0..5, a bad flag, NULL tris_out with the flag and a count, tris_out overlapping tris, NULL n_patches / n_pairs /
 * totals, NULL tables with a capacity, an index of another triangle count or on another device, a triangle index outside
 * [0, n_verts) or a non-finite vertex (host variant: on the host; _dev: the check kernel of r2s_mesh_distance_dev).
 * R2S_ERR_UNSUPPORTED, outputs untouched: n_tris > 2^30 or n_verts beyond 32 bits (before anything is read), more than 2^31 - 1
 * crossings, a tree deeper than the traversal stack (64 levels).  No GPU: R2S_ERR_NO_DEVICE; there is no CPU fallback.
 * n_tris == 0 succeeds with 0 patches. */
#define R2S_NESTING_REWIND 1
int r2s_mesh_nesting(const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris, int32_t ray, int32_t flags,
                     int32_t device, int32_t *tris_out, int32_t *patch_of_tri_out, int64_t *n_patches, int64_t totals[8]);
int r2s_last_mesh_nesting(int64_t *counts_out, int64_t capacity, int64_t *pairs_out, int64_t pair_capacity, int64_t *n_patches,
                          int64_t *n_pairs);
int r2s_mesh_nesting_dev(const r2s_mesh_index *index, const float *d_verts, int64_t n_verts, const int32_t *d_tris,
                         int64_t n_tris, int32_t ray, int32_t flags, int32_t *d_tris_out, int32_t *d_patch_of_tri,
                         int64_t *d_counts, int64_t patch_capacity, int64_t *d_pairs, int64_t pair_capacity, int64_t *n_patches,
                         int64_t *n_pairs, int64_t totals[8], void *stream);

/* ---- on-disk output ------------------------------------------------------------------ */

/* binary STL of a triangle mesh (verts [n_verts][3], tris [n_tris][3] 0-based); host only, no device; ".stl" appended
 * when missing.  80-byte header that does not begin with "solid", uint32 facet count, 50 bytes per facet: the float32
 * normalised (v1-v0)x(v2-v0) ((0,0,0) for zero area), the three vertices, attribute 0.  >= 2^32 facets:
 * R2S_ERR_UNSUPPORTED; an index outside [0, n_verts): R2S_ERR_ARG. */
int r2s_export_stl(const char *filename, const float *verts, int64_t n_verts, const int32_t *tris, int64_t n_tris);

/* The triangles of an STL file as a soup: verts float32 [3 n_tris][3], triangle t = vertices 3t, 3t + 1, 3t + 2 (the input of
 * r2s_mesh_weld with tris == NULL).  Facet normals and attribute bytes are ignored.  Host only, no device.
 *   - the file is BINARY when its size equals 84 + 50 * count, count the little-endian uint32 at byte 80 (whatever the header
 *     says, "solid" included); the coordinates are taken bit for bit.
 *   - otherwise it is parsed as ASCII: solid [name] / facet normal nx ny nz / outer loop / vertex x y z (three times) / endloop /
 *     endfacet / endsolid [name].  Any whitespace between the words, any case of the keywords, several solid blocks in one file;
 *     a name runs to the next facet / endsolid (after solid) or solid (after endsolid) keyword.  Each coordinate is read with
 *     strtod and that double is rounded to float32 once.
 *   - R2S_ERR_ARG (the code of r2s_import_vtu for malformed files) with a text in r2s_last_error: a file that cannot be opened, a
 *     truncated file (binary: the size does not fit; ASCII: the text ends inside a solid), a facet without exactly three
 *     vertices, an unknown word, a coordinate that is not a number or not finite as float32.  *out is zeroed then.
 * verts is malloc'ed by the library: release it with r2s_free_stl_mesh (NULL-safe, zeroes the struct). */
typedef struct {
    int64_t n_tris;
    float *verts; /* [3 * n_tris][3] */
} r2s_stl_mesh;
int r2s_import_stl(const char *filename, r2s_stl_mesh *out);
void r2s_free_stl_mesh(r2s_stl_mesh *m);

/* exportSdfToVTI(filename, grid, values, value_label, smooth)       src/DataExport/ExportToVTI.jl:22-67
 * VTK ImageData: dimensions N*smooth+1 (smooth = 0: N+1, i.e. `nothing`), Origin = AABB_min, Spacing =
 * cell_size(/smooth), one point-data array `value_label` (Float32 or Float64, x fastest).  ".vti" is appended
 * when missing.  Host pointers; no device needed. */
int r2s_export_vti(const char *filename, const r2s_grid *grid, const void *values, int32_t is_float32,
                   int64_t n_values, const char *value_label, int32_t smooth);

/* the same data set with the payload deflated block-wise (compressor="vtkZLibDataCompressor", WriteVTK's default
 * on-disk form): level 0 = raw appended (r2s_export_vti), 1..9 = zlib level */
int r2s_export_vti_z(const char *filename, const r2s_grid *grid, const void *values, int32_t is_float32,
                     int64_t n_values, const char *value_label, int32_t smooth, int32_t level);

/* exportToVTU(fileName, X, IEN, VTK_CODE, rho)                       src/DataExport/ExportToVTU.jl:2-99
 * ASCII UnstructuredGrid of the mesh (VTK_CODE 12 = hexahedron, 10 = tetra), optional nodal "density". */
int r2s_export_vtu(const char *filename, const double *X, int64_t nnp, const int64_t *IEN, int64_t nel,
                   int32_t nen, int32_t vtk_code, const double *rho_n);

/* import_vtu_mesh(vtu_file) -> (X, IEN, rho)                         src/DataImport/VTUImport.jl:22-112
 * Mesh of an ASCII UnstructuredGrid file: hexahedra (VTK type 12, 8 nodes) or tetrahedra (10, 4 nodes), other
 * cells are skipped and counted; IEN comes back 1-based.  Element densities (:117-226): the first cell-data
 * field named density / rho / volfrac / ... (the reference's list), else the first cell-data field, else 1.0;
 * taken by position, padded with 1.0.  The arrays are malloc'ed by the library: release them with
 * r2s_free_vtu_mesh.  Every DataArray encoding ReadVTK reads is understood: ascii, binary (inline base64) and
 * appended (raw / base64), plain or zlib-compressed, header_type UInt32 / UInt64, little endian. */
typedef struct r2s_vtu_mesh {
    int64_t nnp, nel;
    int32_t nen;         /* 8 or 4 */
    int32_t elem_type;   /* R2S_HEX8 / R2S_TET4 */
    int64_t n_skipped;   /* cells of other types */
    double *X;           /* [nnp][3] */
    int64_t *IEN;        /* [nel][nen], 1-based */
    double *rho;         /* [nel] */
    char density_field[64]; /* cell-data field the densities came from ("" = default 1.0) */
} r2s_vtu_mesh;
int r2s_import_vtu(const char *filename, r2s_vtu_mesh *out);
void r2s_free_vtu_mesh(r2s_vtu_mesh *mesh);

/* MeshInformations(matread(file)) -> (X, IEN, rho)                    src/MeshGrid/MeshInformations.jl:3-12
 * MATLAB level-5 .mat file (compressed or not) with `rho` [nel] and the struct `msh` holding X (3 x nnp) and IEN
 * (nen x nel; IEN + 1 is returned, as the reference adds 1, :8).  Same result struct and ownership as
 * r2s_import_vtu (release with r2s_free_vtu_mesh).  v7.3 (HDF5) files are refused. */
int r2s_import_mat(const char *filename, r2s_vtu_mesh *out);

/* frees what the library keeps between calls: the per-device host sessions of the host-pointer entry points (plan,
 * device copies of the mesh, output volumes, pinned staging buffers) and the shared work buffers of the smoothing stage.
 * Must not run concurrently with any other call of the library (it destroys the sessions other calls lock). */
void r2s_release_cache(void);

/* ---- diagnostics ---- */
/* bytes of device memory the library's own buffers hold at this moment, over all devices and threads (what the calls in
 * flight, the caches and the live handles have allocated and not yet freed); after r2s_release_cache with no handle alive
 * and no call running it is what it was before the first call */
int64_t r2s_live_device_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* RHO2SDF_HIP_H */
