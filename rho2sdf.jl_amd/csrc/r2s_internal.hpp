// Cross-file internals of the library (C++ linkage, not part of the C ABI): device-pointer forms of the
// pre-stage and post-processing stages, used by the host-pointer entry points of their own files and by the
// chained r2s_rho2sdf() in r2s_host.hip, and the seam between r2s_redistance.hip and r2s_mesh_index.hip.  All of them run on the CURRENT device and are synchronous on return.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "r2s_common.hpp"

namespace r2s_int {

// ---- per-device work caches ----------------------------------------------------------------------------------------------
// Every PerDevice of the process, in the order they were constructed.  Each one puts itself here, so that r2s_release_cache()
// frees a new family's cache without being told about it.  The list is never destroyed, like the maps of its members, and it
// is created on first use: the order of static initialisation across files does not matter.  The members are objects of static
// storage, constructed one after the other while the library is loaded: the list needs no lock of its own, and
// r2s_release_cache(), which walks it, must not run concurrently with any other call anyway (include/rho2sdf_hip.h).
class PerDeviceCache {
public:
    virtual void release_all() = 0;

protected:
    PerDeviceCache();
    ~PerDeviceCache() = default;
};
std::vector<PerDeviceCache*>& per_device_caches();   // (r2s_post.hip)
inline PerDeviceCache::PerDeviceCache() { per_device_caches().push_back(this); }

// The work buffers a family of entry points keeps between calls, one W per device.  W holds its device buffers as DevBuf
// members (which free themselves), so that destroying an entry frees every one of them: there is no second list of the members to keep in step.
// A call locks `mu` for as long as it uses its entry.  The map is never destroyed: at process exit the HIP runtime may be
// gone before a static destructor runs, and the driver reclaims the memory anyway.
template <class W>
class PerDevice : public PerDeviceCache {
public:
    std::mutex mu;
    // the entry of `device` (empty on first use); the caller holds mu
    W& of(int device) { return map_[device]; }
    // the entry of the current device, or nullptr and the error in rc; the caller holds mu
    W* current(int& rc)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) {
            rc = fail(R2S_ERR_HIP, "hipGetDevice failed");
            return nullptr;
        }
        rc = 0;
        return &map_[dev];
    }
    // frees every entry with its own device current, then makes the caller's device current again
    void release_all() override
    {
        std::lock_guard<std::mutex> lock(mu);
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        for (auto it = map_.begin(); it != map_.end(); it = map_.erase(it)) (void)hipSetDevice(it->first);
        if (cur >= 0) (void)hipSetDevice(cur);
        (void)hipGetLastError();
    }

private:
    std::map<int, W>& map_ = *new std::map<int, W>;
};

// The three volume forms below read X and rho_n through dIEN unchecked: the caller has validated the connectivity
// (dense_in_nodes_dev does; the host-pointer entry points of r2s_pre.hip run a flag pass after the upload).
// calculate_mesh_volume (MeshVolume.jl:4-42): d_rho_e[nel] element densities
int mesh_volume_dev(const double* dX, const int64_t* dIEN, int64_t nel, int elem_type, const double* d_rho_e,
                    double* V_domain, double* V_frac, DevBuf* ws = nullptr);

// DenseInNodes (NodalDensities.jl:89-218); the ascending node -> element lists are built on the device.
// ws: five buffers the caller keeps between calls (nullptr: temporaries of the call)
int dense_in_nodes_dev(const double* dX, int64_t nnp, const int64_t* dIEN, int64_t nel, int elem_type, const double* d_rho_e,
                       double* d_rho_n_out, DevBuf* ws = nullptr);

// find_threshold_for_volume (Isocontour_volume.jl:77-154); TET4: the same bisection over the TET4 iso-volume
// (the reference has none, SURVEY 8(f)2 - see r2s_pre.hip)
int find_threshold_dev(const double* dX, const int64_t* dIEN, int64_t nel, int elem_type, const double* d_rho_n,
                       double target_volume, double tol, int maxit, double* rho_t_out, int* iters_out);

// calculate_isocontour_volume (Isocontour_volume.jl:1-75) at one threshold
int isocontour_volume_dev(const double* dX, const int64_t* dIEN, int64_t nel, int elem_type, const double* d_rho_n,
                          double thr, double* volume_out);

// analyze_sdf_components (SdfArtifactRemoval.jl:256-311): one entry per 6-connected component of {sdf >= threshold},
// in ascending root order; root = the component's smallest 0-based linear index
struct ComponentTable {
    std::vector<int64_t> root, size;
};
// replaces the calling thread's last table (r2s_last_components)
void set_last_components(ComponentTable&& t);

// remove_sdf_artifacts! on a device-resident field (SdfArtifactRemoval.jl:134-245); table != nullptr: also the component
// table of the same labelling (of the field before the flip)
int remove_artifacts_dev(double* d_sdf, const r2s_grid* g, double threshold, double min_ratio, hipStream_t st,
                         int64_t* n_flipped, ComponentTable* table = nullptr);

// RBFs_smoothing with device-resident input / output (RBFs4Smoothing.jl:321-377)
// fine_chunk (optional): the output field is evaluated in a few Z chunks; after the launch of each one (default stream)
// fine_chunk(first, last) is called with the range [first, last) of d_fine_out that kernel fills, so that the caller
// can send finished chunks to the host while the next one is computed.  A non-zero return aborts.
// fine_early: the chunks are evaluated BEFORE the level bisection and forwarded WITHOUT the level shift (the evaluation needs
// the weights only; the caller adds *th_out to what it received - the same Float32 sum); d_fine_out then stays WITHOUT the
// shift (its chunks may still be travelling when the level is known).
int rbf_smooth_dev(const double* d_sdf, const r2s_grid* g, int is_interp, int smooth, double kthr, double target_volume,
                   float* d_fine_out, float* th_out, int* cg_iters,
                   const std::function<int(int64_t, int64_t)>* fine_chunk = nullptr, void* workspace = nullptr,
                   bool fine_early = false);
// the first half of RBFs_smoothing alone (r2s_rbf_field_fit): process_vector, the weights and the level shift of the same
// code path as rbf_smooth_dev; sdf is a host array, d_weights_out a device array of the lattice's size on the CURRENT device
int rbf_fit_weights(const double* sdf, const r2s_grid* g, int is_interp, double kthr, double target_volume, float* d_weights_out,
                    float* th_out, int* cg_iters);
// one axis of create_grid (RBFs4Smoothing.jl:36-46): the Float32 coordinates of the coarse lattice
void rbf_coarse_axis(double mn, double mx, int n, std::vector<float>& c);
// workspace (optional): the call's device buffers, kept between calls on the CURRENT device (create / release there)
void* rbf_workspace_create();
void rbf_workspace_release(void* workspace);

// ---- Z-slab distributed post-processing (single process, one entry per device; SURVEY 8(e) second half) ----------
// A slab OWNS the grid planes [k0, k1) and HOLDS [h0, h1) (its planes plus the halo the stencils reach into);
// d_sdf is the Float64 field of the held planes on `device`, plane k at (k - h0) * plane.
struct Slab {
    int device;
    hipStream_t stream;
    int k0, k1, h0, h1;
    double* d_sdf;
};
// copies every held-but-not-owned plane from the slab that owns it (peer copies over xGMI); base[q] = the array of
// slab q (held planes), elem = bytes per value
int exchange_halo_slabs(const std::vector<Slab>& S, const std::vector<void*>& base, size_t elem, int64_t plane, int radius);
// remove_sdf_artifacts! with the components labelled per slab and merged across the slab interfaces on the host
// (boundary-plane labels only); owned planes of d_sdf are modified, halos are NOT refreshed
// (table != nullptr: also the whole grid's component table, equal to remove_artifacts_dev's)
int remove_artifacts_slabs(const std::vector<Slab>& S, const r2s_grid* g, double threshold, double min_ratio, int64_t* n_flipped,
                           ComponentTable* table = nullptr);
// RBFs_smoothing on slabs: halo exchanges of the CG direction / weights / LSF, plane-wise dot products summed in k
// order on the host, volume row sums reduced on slab 0 - bit-identical to rbf_smooth_dev on one device.
// fine_out_host: the caller's (host) array of the whole fine grid, filled slab by slab.
int rbf_smooth_slabs(const std::vector<Slab>& S, const r2s_grid* g, int is_interp, int smooth, double kthr, double target_volume,
                     float* fine_out_host, float* th_out, int* cg_iters);

// frees the cached per-device host sessions (r2s_host.hip); called by r2s_release_cache()
void release_host_sessions();

// ---- iso-surface extraction (r2s_surface.hip) -------------------------------------------------------------------------
struct Surface {
    std::vector<float> verts;    // [nv][3]
    std::vector<int32_t> tris;   // [nt][3], 0-based
};
// replaces the calling thread's last surface (r2s_last_isosurface)
void set_last_surface(Surface&& s);
// device work buffers of one extraction (kept by the caller between calls on the CURRENT device)
struct IsoWork {
    DevBuf rows, tiles, tot, field, verts, tris;
};
// the surface of a device field (Float32 or Float64, x fastest) on the current device, after the work queued on `st`;
// has_shift: Float32 values are read as f + shift (float32 sum), the level shift the host adds to an early fine field
int extract_isosurface_dev(const void* d_values, bool is_float32, const int64_t dims[3], const double origin[3], double spacing,
                           double iso, float shift, bool has_shift, hipStream_t st, IsoWork& w, Surface& out);
// the same from a host array (uploaded to the current device)
int extract_isosurface_host(const void* values, bool is_float32, const int64_t dims[3], const double origin[3], double spacing,
                            double iso, Surface& out);

// ---- mesh index (r2s_mesh_index.hip) and what its entry points share with r2s_redistance.hip -------------------------------
// the tree of a mesh index and the mesh it refers to (r2s_mesh_index owns all three; redistance_full borrows the mesh)
struct MiTree {
    const float* verts = nullptr;
    const int32_t* tris = nullptr;
    int64_t n_verts = 0, n_tris = 0;
    DevBuf nodes;
    int32_t root = 0;
    int32_t depth = 0;
    double absmax = 0.0;
};
// the tree over the device mesh (verts, tris) on the current device, after the work queued on `st`; synchronous
int mi_build_tree(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, hipStream_t st, MiTree& T);
// enqueues the query of n points (pts != null) or of the lattice (dims != null) on `st`; does not wait
int mi_query(const MiTree& T, const void* d_pts, bool pts_f32, int64_t n, const int64_t* dims, const double* origin, double spacing,
             const void* d_field, bool field_f32, double iso, void* d_out, bool out_f32, int32_t* d_closest, hipStream_t st);

// argument checks and mesh handling of both files, defined in r2s_redistance.hip; `who` heads the error text
int lattice_args(const char* who, const int64_t dims[3], const double origin[3], double spacing, double band);
int mesh_args(const char* who, const void* verts, int64_t n_verts, const void* tris, int64_t n_tris);
// every triangle index in [0, n_verts) and every vertex finite: a host mesh, and a device mesh (flag: one int32 the call may
// grow; synchronises `st`)
int check_mesh_host(const char* who, const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris);
int check_mesh_dev(const char* who, const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, DevBuf& flag,
                   hipStream_t st);
inline size_t real_bytes(int32_t is_float32) { return is_float32 ? sizeof(float) : sizeof(double); }
inline size_t vert_bytes(int64_t n_verts) { return 3 * sizeof(float) * (size_t)n_verts; }
inline size_t tri_bytes(int64_t n_tris) { return 3 * sizeof(int32_t) * (size_t)n_tris; }
// whether the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte (a null pointer or an empty range shares none)
inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes)
{
    if (!a || !b || !abytes || !bbytes) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}
// a caller's array as a byte range, for the overlap checks of the tools with several outputs
struct Span {
    const void* p;
    size_t bytes;
};
inline bool overlaps(const Span& a, const Span& b) { return overlaps(a.p, a.bytes, b.p, b.bytes); }
// sizes dv / dt for the mesh (at least one element each) and copies it in: from the host with hipMemcpy, or
// (from_device) from the current device on `st`
int upload_mesh(DevBuf& dv, DevBuf& dt, const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, bool from_device,
                hipStream_t st);

// ---- one call of a mesh topology tool (shells, sections, weld, orient, fans, holes, nesting) ----------------------------------
// What the host-pointer entry and the _dev entry of a tool do between their argument checks and the core, and how results go
// back, so that each tool has one body (X_run) for both kinds of caller.  W is the tool's work struct, with DevBuf members
// verts, tris and flag.  The call holds the lock of the tool's cache from open() until it is destroyed.
template <class W>
class MeshCall {
public:
    static constexpr bool STAGE_DEVICE_CALLER = true;   // (for staged)
    MeshCall(const char* who, PerDevice<W>& cache, const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device)
        : who_(who), cache_(cache), verts_(verts), tris_(tris), n_verts_(n_verts), n_tris_(n_tris), host_(true), device_(device) {}
    MeshCall(const char* who, PerDevice<W>& cache, const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, hipStream_t st)
        : who_(who), cache_(cache), verts_(d_verts), tris_(d_tris), n_verts_(n_verts), n_tris_(n_tris), host_(false), st_(st) {}
    // a host caller:   check_mesh_host, use_device(device), [before_lock], the lock, current(), upload_mesh into w.verts / w.tris
    // a device caller: check_device(0), [before_lock], the lock, current(), check_mesh_dev with w.flag
    // before_lock: a check of the tool's own that needs the device but not the work buffers (nesting: the index's device)
    template <class F = std::nullptr_t>
    int open(F before_lock = nullptr)
    {
        int rc = host_ ? check_mesh_host(who_, verts_, n_verts_, tris_, n_tris_) : 0;
        if (rc || (rc = host_ ? use_device(device_) : check_device(0))) return rc;
        if constexpr (!std::is_null_pointer_v<F>)
            if ((rc = before_lock())) return rc;
        lock_ = std::unique_lock<std::mutex>(cache_.mu);
        w_ = cache_.current(rc);
        if (rc) return rc;
        if (!host_) return check_mesh_dev(who_, verts_, n_verts_, tris_, n_tris_, w_->flag, st_);
        if ((rc = upload_mesh(w_->verts, w_->tris, verts_, n_verts_, tris_, n_tris_, false, nullptr))) return rc;
        verts_ = w_->verts.template as<float>();
        tris_ = tris_ ? w_->tris.template as<int32_t>() : nullptr;   // (weld: no triangle array is a soup, on the device too)
        return 0;
    }
    bool is_host() const { return host_; }
    const float* d_verts() const { return verts_; }
    const int32_t* d_tris() const { return tris_; }
    hipStream_t stream() const { return st_; }   // (a host caller's: the null stream)
    W& work() { return *w_; }
    // `bytes` from device memory to the caller's dst: a host caller's copy is done on return, a device caller's is queued on
    // the stream.  No dst, no bytes, or dst is where the kernels wrote already (staged): nothing to do.
    int deliver(void* dst, const void* src, size_t bytes)
    {
        if (!dst || !bytes || dst == src) return 0;
        if (host_) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        if (!host_) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st_));
        return 0;
    }
    // d_out = where the kernels write an output array of the caller's, delivered afterwards: a host caller's goes to `buf`, sized
    // here.  A device caller's is written in place by orient, fans, holes and weld, so what a refusal behind those kernels leaves
    // in it is unspecified; nesting alone passes STAGE_DEVICE_CALLER, so that its refusals leave the array untouched.
    template <class T>
    int staged(DevBuf& buf, T* caller, size_t bytes, T*& d_out, bool stage_device_caller = false)
    {
        d_out = caller;
        if (!host_ && !stage_device_caller) return 0;
        ENSURE(buf, bytes);
        d_out = buf.as<T>();
        return 0;
    }
    // one table of the result, `count` elements at src: a host caller keeps all of it in `kept` (for the tool's r2s_last_*), a
    // device caller gets it at d_dst when the tool's capacity rule says it fits
    template <class T>
    int table(std::vector<T>& kept, T* d_dst, bool fits, const DevBuf& src, size_t count)
    {
        if (host_) kept.resize(count);
        return host_ ? deliver(kept.data(), src.p, sizeof(T) * count) : fits ? deliver(d_dst, src.p, sizeof(T) * count) : 0;
    }
    // the cores are synchronous, the copies queued for a device caller are not
    int finish()
    {
        HIP_TRY(hipStreamSynchronize(st_));
        return 0;
    }

private:
    const char* who_;
    PerDevice<W>& cache_;
    const float* verts_;
    const int32_t* tris_;
    int64_t n_verts_, n_tris_;
    bool host_;
    int32_t device_ = -1;
    hipStream_t st_ = nullptr;
    std::unique_lock<std::mutex> lock_;
    W* w_ = nullptr;
};

// min(capacity, n) rows of `row` elements of a kept table to dst, which r2s_last_* has checked; the number copied
template <class T>
inline int64_t copy_rows(T* dst, const std::vector<T>& table, size_t row, int64_t capacity, int64_t n)
{
    const int64_t m = std::min(capacity, n);
    if (m > 0) std::memcpy(dst, table.data(), sizeof(T) * row * (size_t)m);
    return m;
}

}  // namespace r2s_int
