// Mesh weld: the vertices of a triangle mesh (or of a triangle soup) that are the same point become one vertex, the triangles
// are remapped, and collapsed / duplicate triangles and unused vertices are dropped on request (include/rho2sdf_hip.h,
// r2s_mesh_weld; DESIGN.md "Mesh weld").  Integer and copy work only: every output vertex is an input vertex, bit for bit.
//   mw_vkey_kernel     one thread per vertex: the three key words (exact mode: the order-preserving pattern of each float32
//                      with -0 folded onto +0; snap mode: floor(v / snap) + 2^31, out-of-range cells raise a flag), stored as
//                      z (32 bits) and (x << 32) | y (64 bits), payload the vertex index
//   -> stable rocPRIM radix sort of (z, index), mw_gather_kernel (the 64-bit word in that order), stable radix sort of
//      ((x, y), index): equal triples are adjacent, ascending index inside a run, so the head of a run is its representative
//   mw_vhead_kernel    run heads: position p where the triple differs from that of p - 1 -> rocPRIM inclusive max-scan of
//                      (head ? p : 0): the head position of every member
//   mw_rep_kernel      rep[i] = the index at the head of i's run, is_rep[i] -> rocPRIM exclusive scan: the class numbers in
//                      first-occurrence order -> mw_class_kernel: class_of[i], the number of classes
//   mw_tkey_kernel     one thread per triangle: the class triple, rotated so the smallest comes first; the key is
//                      (smallest << 32) | lower of the other two, and (higher << 1) | orientation bit; collapsed triangles get
//                      a key above every real one and are counted
//   -> the same two stable sorts -> mw_tdup_kernel: a member equal to the one before it is a duplicate; a member whose triple
//      equals the one before it with the other orientation bit marks an opposite pair (once per class: bit 0 sorts before 1)
//   mw_tkeep_kernel    which triangles survive the flags, which classes they reference -> two exclusive scans (triangles, classes)
//   mw_vout_kernel     vert_map, the copy of the surviving representatives;  mw_tout_kernel  tri_map, the remapped survivors
// Counts go through wavefront ballots and one integer atomic per wavefront.  The one floating-point operation pair of the file,
// the division and floor of the snap mode, lives in mw_cell().  The kernels up to mw_tkeep_kernel, mw_tout_kernel, the sort and the
// two stages mw_classes / mw_triangles are in r2s_mesh_weld.hpp, which r2s_mesh_simplify.hip shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_graph.hpp"
#include "r2s_mesh_weld.hpp"

using namespace r2s_int;

namespace {

// unum = the exclusive scan of used over the classes: final_of[c] (-1: dropped), the number of used classes
__global__ void __launch_bounds__(256) mw_final_kernel(const int32_t* __restrict__ used, const int32_t* __restrict__ unum, int64_t ncls,
                                                        int32_t drop_unused, int32_t* __restrict__ final_of, uint64_t* __restrict__ small)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncls) return;
    final_of[c] = drop_unused ? (used[c] ? unum[c] : -1) : (int32_t)c;
    if (c == ncls - 1) small[MW_USED] = (uint64_t)(unum[c] + used[c]);
}

__global__ void __launch_bounds__(256) mw_vout_kernel(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ class_of,
                                                       const int32_t* __restrict__ is_rep, const int32_t* __restrict__ final_of,
                                                       int32_t* __restrict__ vert_map, float* __restrict__ verts_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int32_t f = final_of[class_of[i]];
    vert_map[i] = f;
    if (f >= 0 && is_rep[i]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) verts_out[3 * (int64_t)f + k] = verts[3 * i + k];   // (a copy: the bits are kept)
    }
}

// work buffers of the weld calls, kept per device between calls (r2s_release_cache frees them)
struct WeldWork : MwBufs {
    DevBuf verts, tris, verts_out, tris_out, flag, unum, final_of;
};
PerDevice<WeldWork> g_weld_work;

// The weld of the device mesh on the current device, after the work queued on `st`; synchronous.  d_tris == nullptr: the soup.
// Nothing is written to d_verts_out / d_tris_out before the snap range check has passed.  Leaves vert_map in w.vert_map
// [n_verts] and tri_map in w.tri_map [n_tris].
int weld_core(const float* d_verts, int64_t nv, const int32_t* d_tris, int64_t nt, double snap, int32_t flags, hipStream_t st, WeldWork& w,
              float* d_verts_out, int32_t* d_tris_out, int64_t totals[8])
{
    for (int k = 0; k < 8; ++k) totals[k] = 0;
    if (nv == 0) return 0;   // (no vertex: no valid triangle either)
    int64_t ncls = 0;
    int rc = mw_classes(w, "mesh_weld", d_verts, nv, nt, snap, st, &ncls);
    if (rc) return rc;
    uint64_t h_small[MW_SMALL] = {};
    uint64_t* small = w.small.as<uint64_t>();
    const int32_t *class_of = w.class_of.as<int32_t>(), *is_rep = w.is_rep.as<int32_t>();
    ENSURE(w.unum, sizeof(int32_t) * (size_t)ncls);
    ENSURE(w.final_of, sizeof(int32_t) * (size_t)ncls);
    if ((rc = mw_triangles(w, d_tris, nt, ncls, flags, st))) return rc;
    int32_t *used = w.used.as<int32_t>(), *unum = w.unum.as<int32_t>(), *final_of = w.final_of.as<int32_t>();
    if ((rc = weld_scan(w, used, unum, ncls, st))) return rc;
    mw_final_kernel<<<ms_blocks(ncls), 256, 0, st>>>(used, unum, ncls, (flags & R2S_WELD_DROP_UNUSED) ? 1 : 0, final_of, small);
    HIP_TRY(hipGetLastError());
    mw_vout_kernel<<<ms_blocks(nv), 256, 0, st>>>(d_verts, nv, class_of, is_rep, final_of, w.vert_map.as<int32_t>(), d_verts_out);
    HIP_TRY(hipGetLastError());
    if (nt > 0) {
        mw_tout_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, nt, w.vert_map.as<int32_t>(), w.keep.as<int32_t>(), w.tnum.as<int32_t>(),
                                                     w.tri_map.as<int32_t>(), d_tris_out, small);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_used = (int64_t)h_small[MW_USED];
    totals[0] = (flags & R2S_WELD_DROP_UNUSED) ? n_used : ncls;
    totals[1] = (int64_t)h_small[MW_TRIS_OUT];
    totals[2] = nv - ncls;
    totals[3] = (int64_t)h_small[MW_COLLAPSED];
    totals[4] = (int64_t)h_small[MW_DUPLICATES];
    totals[5] = (int64_t)h_small[MW_OPPOSITE];
    totals[6] = ncls - n_used;
    return 0;
}

// the checks that need no device; *nt = the number of triangles (soup: n_verts / 3)
int weld_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, double snap, int32_t flags, const void* verts_out,
              const void* tris_out, const int64_t* totals, int64_t* nt)
{
    if (n_verts < 0 || n_tris < 0) return fail(R2S_ERR_ARG, "mesh_weld: null mesh array or negative count");
    if (!tris) {
        if (n_verts % 3 != 0) return fail(R2S_ERR_ARG, "mesh_weld: a soup (tris == NULL) needs n_verts divisible by 3 (got %lld)", (long long)n_verts);
        if (n_tris != 0 && n_tris != n_verts / 3)
            return fail(R2S_ERR_ARG, "mesh_weld: a soup (tris == NULL) has n_verts / 3 triangles (n_tris = %lld, n_verts = %lld)",
                        (long long)n_tris, (long long)n_verts);
        n_tris = n_verts / 3;
    }
    const int rc = mesh_args("mesh_weld", verts, n_verts, tris ? tris : verts, n_tris);
    if (rc) return rc;
    if (n_tris > MW_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_weld: %lld triangles exceed 2^30", (long long)n_tris);
    if (!(snap >= 0.0) || !std::isfinite(snap)) return fail(R2S_ERR_ARG, "mesh_weld: snap must be 0 or positive and finite");
    if (flags & ~(R2S_WELD_DROP_COLLAPSED | R2S_WELD_DROP_DUPLICATES | R2S_WELD_DROP_UNUSED))
        return fail(R2S_ERR_ARG, "mesh_weld: unknown flag bits in %d", (int)flags);
    if (!totals || (n_verts > 0 && !verts_out) || (n_tris > 0 && !tris_out)) return fail(R2S_ERR_ARG, "mesh_weld: null verts_out / tris_out / totals");
    *nt = n_tris;
    return 0;
}

// One call for both kinds of caller: the welded mesh (a host caller's through work buffers, tot[0] vertices and tot[1] triangles of
// them copied out), then vert_map, tri_map and the totals.  nt: the number of triangles, of a soup too.
int weld_run(MeshCall<WeldWork>& c, int64_t n_verts, int64_t nt, double snap, int32_t flags, float* verts_out, int32_t* tris_out,
             int32_t* vert_map_out, int32_t* tri_map_out, int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    WeldWork& w = c.work();
    int64_t tot[8];
    float* d_verts_out = nullptr;
    int32_t* d_tris_out = nullptr;
    if ((rc = c.staged(w.verts_out, verts_out, vert_bytes(std::max<int64_t>(n_verts, 1)), d_verts_out)) ||
        (rc = c.staged(w.tris_out, tris_out, tri_bytes(std::max<int64_t>(nt, 1)), d_tris_out)) ||
        (rc = weld_core(c.d_verts(), n_verts, c.d_tris(), nt, snap, flags, c.stream(), w, d_verts_out, d_tris_out, tot)) ||
        (rc = c.deliver(verts_out, d_verts_out, vert_bytes(tot[0]))) || (rc = c.deliver(tris_out, d_tris_out, tri_bytes(tot[1]))) ||
        (rc = c.deliver(vert_map_out, w.vert_map.p, sizeof(int32_t) * (size_t)n_verts)) ||
        (rc = c.deliver(tri_map_out, w.tri_map.p, sizeof(int32_t) * (size_t)nt)) || (rc = c.finish()))
        return rc;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_weld(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, double snap, int32_t flags, int32_t device,
                  float* verts_out, int32_t* tris_out, int32_t* vert_map_out, int32_t* tri_map_out, int64_t totals[8])
{
    int64_t nt = 0;
    if (const int rc = weld_args(verts, n_verts, tris, n_tris, snap, flags, verts_out, tris_out, totals, &nt)) return rc;
    MeshCall<WeldWork> call("mesh_weld", g_weld_work, verts, n_verts, tris, tris ? nt : 0, device);
    return weld_run(call, n_verts, nt, snap, flags, verts_out, tris_out, vert_map_out, tri_map_out, totals);
}

int r2s_mesh_weld_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, double snap, int32_t flags,
                      float* d_verts_out, int32_t* d_tris_out, int32_t* d_vert_map_out, int32_t* d_tri_map_out, int64_t totals[8],
                      void* stream)
{
    int64_t nt = 0;
    if (const int rc = weld_args(d_verts, n_verts, d_tris, n_tris, snap, flags, d_verts_out, d_tris_out, totals, &nt)) return rc;
    MeshCall<WeldWork> call("mesh_weld", g_weld_work, d_verts, n_verts, d_tris, d_tris ? nt : 0, (hipStream_t)stream);
    return weld_run(call, n_verts, nt, snap, flags, d_verts_out, d_tris_out, d_vert_map_out, d_tri_map_out, totals);
}

}  // extern "C"
