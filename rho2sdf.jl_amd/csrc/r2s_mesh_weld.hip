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
// the division and floor of the snap mode, lives in mw_cell().
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_graph.hpp"

using namespace r2s_int;

namespace {

constexpr int64_t MW_MAX_TRIS = (int64_t)1 << 30;
// slots of the small device array
constexpr int MW_OVERFLOW = 0, MW_CLASSES = 1, MW_COLLAPSED = 2, MW_DUPLICATES = 3, MW_OPPOSITE = 4, MW_TRIS_OUT = 5, MW_USED = 6;
constexpr int MW_SMALL = 8;

// the cell of one coordinate in snap mode: ONE division rounded in double, then floor.  Kept out of line and compiled without
// contraction or reassociation, so that no neighbouring arithmetic can be folded into it (the file is built without
// -ffast-math: a division is never replaced by a reciprocal product).
__device__ __attribute__((noinline)) double mw_cell(float v, double snap)
{
#pragma clang fp contract(off) reassociate(off)
    const double q = (double)v / snap;
    return floor(q);
}

// adds the number of set lanes to small[slot]: one atomic per wavefront (called by every thread of the block)
__device__ inline void mw_count(bool set, uint64_t* __restrict__ small, int slot)
{
    const unsigned long long m = __ballot(set);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)&small[slot], (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) mw_vkey_kernel(const float* __restrict__ verts, int64_t nv, double snap, uint32_t* __restrict__ kz,
                                                       uint64_t* __restrict__ kxy, uint32_t* __restrict__ idx, uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < nv) {
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = verts[3 * i + k];
            if (snap > 0.0) {
                const double q = mw_cell(f, snap);
                const bool in = q >= -2147483648.0 && q < 2147483648.0;   // (false for a non-finite quotient)
                bad = bad || !in;
                w[k] = in ? (uint32_t)((int64_t)q + 2147483648ll) : 0u;
            } else {
                const uint32_t u = __float_as_uint(f);
                w[k] = ms_ordered(__uint_as_float(u == 0x80000000u ? 0u : u));
            }
        }
        kz[i] = w[2];
        kxy[i] = ((uint64_t)w[0] << 32) | (uint64_t)w[1];
        idx[i] = (uint32_t)i;
    }
    mw_count(bad, small, MW_OVERFLOW);
}

// out[p] = src[order[p]]
__global__ void __launch_bounds__(256) mw_gather_kernel(const uint64_t* __restrict__ src, const uint32_t* __restrict__ order, int64_t n,
                                                         uint64_t* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) out[p] = src[order[p]];
}

// hp[p] = p where the key triple of sorted position p differs from that of p - 1 (a run head), else 0
__global__ void __launch_bounds__(256) mw_vhead_kernel(const uint64_t* __restrict__ sxy, const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ kz, int64_t nv, int32_t* __restrict__ hp)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const bool head = p == 0 || sxy[p] != sxy[p - 1] || kz[order[p]] != kz[order[p - 1]];
    hp[p] = head ? (int32_t)p : 0;
}

// hp = the inclusive max-scan: the head position of p's run
__global__ void __launch_bounds__(256) mw_rep_kernel(const uint32_t* __restrict__ order, const int32_t* __restrict__ hp, int64_t nv,
                                                      int32_t* __restrict__ rep, int32_t* __restrict__ is_rep)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const int32_t h = hp[p];
    const uint32_t i = order[p];
    rep[i] = (int32_t)order[h];
    is_rep[i] = h == (int32_t)p ? 1 : 0;
}

// num = the exclusive scan of is_rep: class_of[i] = num[rep[i]]
__global__ void __launch_bounds__(256) mw_class_kernel(const int32_t* __restrict__ rep, const int32_t* __restrict__ num,
                                                        const int32_t* __restrict__ is_rep, int64_t nv, int32_t* __restrict__ class_of,
                                                        uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    class_of[i] = num[rep[i]];
    if (i == nv - 1) small[MW_CLASSES] = (uint64_t)(num[i] + is_rep[i]);
}

// the classes of triangle t's corners (tris == nullptr: the soup, corners 3t, 3t + 1, 3t + 2); true when two are equal
__device__ inline bool mw_corners(const int32_t* __restrict__ tris, const int32_t* __restrict__ class_of, int64_t t, int32_t c[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = class_of[tris ? (int64_t)tris[3 * t + k] : 3 * t + k];
    return c[0] == c[1] || c[1] == c[2] || c[0] == c[2];
}

__global__ void __launch_bounds__(256) mw_tkey_kernel(const int32_t* __restrict__ tris, const int32_t* __restrict__ class_of, int64_t nt,
                                                       uint64_t ncls, uint32_t* __restrict__ khi, uint64_t* __restrict__ klo,
                                                       uint32_t* __restrict__ idx, uint64_t* __restrict__ small)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool col = false;
    if (t < nt) {
        int32_t c[3];
        col = mw_corners(tris, class_of, t, c);
        uint32_t m = (uint32_t)c[0], p = (uint32_t)c[1], q = (uint32_t)c[2];
        if (c[1] < c[0] && c[1] <= c[2]) m = (uint32_t)c[1], p = (uint32_t)c[2], q = (uint32_t)c[0];
        else if (c[2] < c[0] && c[2] < c[1]) m = (uint32_t)c[2], p = (uint32_t)c[0], q = (uint32_t)c[1];
        const uint32_t lo = p < q ? p : q, hi = p < q ? q : p;
        klo[t] = col ? (ncls << 32) : (((uint64_t)m << 32) | (uint64_t)lo);   // (m < ncls: the collapsed key is above every real one)
        khi[t] = col ? 0u : ((hi << 1) | (p > q ? 1u : 0u));
        idx[t] = (uint32_t)t;
    }
    mw_count(col, small, MW_COLLAPSED);
}

// one thread per sorted triangle: duplicate of the member before it, or the first of the other orientation in its class
__global__ void __launch_bounds__(256) mw_tdup_kernel(const uint64_t* __restrict__ slo, const uint32_t* __restrict__ order,
                                                       const uint32_t* __restrict__ khi, int64_t nt, uint64_t ncls,
                                                       int32_t* __restrict__ is_dup, uint64_t* __restrict__ small)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool dup = false, opp = false;
    if (p < nt) {
        const uint64_t k = slo[p];
        const uint32_t t = order[p];
        if ((k >> 32) < ncls && p > 0 && slo[p - 1] == k) {
            const uint32_t w = khi[t], wp = khi[order[p - 1]];
            dup = w == wp;
            opp = !dup && (w >> 1) == (wp >> 1);   // (bit 0 sorts first: this is the one step 0 -> 1 of the class)
        }
        is_dup[t] = dup ? 1 : 0;
    }
    mw_count(dup, small, MW_DUPLICATES);
    mw_count(opp, small, MW_OPPOSITE);
}

__global__ void __launch_bounds__(256) mw_tkeep_kernel(const int32_t* __restrict__ tris, const int32_t* __restrict__ class_of, int64_t nt,
                                                        const int32_t* __restrict__ is_dup, int32_t flags, int32_t* __restrict__ keep,
                                                        int32_t* __restrict__ used)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int32_t c[3];
    const bool col = mw_corners(tris, class_of, t, c);
    const bool k = !(col && (flags & R2S_WELD_DROP_COLLAPSED)) && !(is_dup[t] && (flags & R2S_WELD_DROP_DUPLICATES));
    keep[t] = k ? 1 : 0;
    if (k) used[c[0]] = used[c[1]] = used[c[2]] = 1;
}

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

// tnum = the exclusive scan of keep
__global__ void __launch_bounds__(256) mw_tout_kernel(const int32_t* __restrict__ tris, int64_t nt, const int32_t* __restrict__ vert_map,
                                                       const int32_t* __restrict__ keep, const int32_t* __restrict__ tnum,
                                                       int32_t* __restrict__ tri_map, int32_t* __restrict__ tris_out, uint64_t* __restrict__ small)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int32_t o = keep[t] ? tnum[t] : -1;
    tri_map[t] = o;
    if (o >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tris_out[3 * (int64_t)o + k] = vert_map[tris ? (int64_t)tris[3 * t + k] : 3 * t + k];
    }
    if (t == nt - 1) small[MW_TRIS_OUT] = (uint64_t)(tnum[t] + keep[t]);
}

// work buffers of the weld calls, kept per device between calls (r2s_release_cache frees them)
struct WeldWork {
    DevBuf verts, tris, verts_out, tris_out, flag, small, k32, k32b, k64, g64, s64, idx, idx2, temp, hp, hp2, rep, is_rep, num, class_of, is_dup,
        keep, tnum, used, unum, final_of, vert_map, tri_map;
};
PerDevice<WeldWork> g_weld_work;

// sorts n (z / high word, index) records of w.k32 / w.k64 / w.idx by the 64-bit word, then the 32-bit word, stably: the order
// ends in w.idx, the sorted 64-bit words in w.s64
int weld_sort(WeldWork& w, int64_t n, unsigned bits32, unsigned bits64, hipStream_t st)
{
    uint32_t *k32 = w.k32.as<uint32_t>(), *k32b = w.k32b.as<uint32_t>(), *idx = w.idx.as<uint32_t>(), *idx2 = w.idx2.as<uint32_t>();
    uint64_t *g64 = w.g64.as<uint64_t>(), *s64 = w.s64.as<uint64_t>();
    size_t tb = 0, tb2 = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, k32, k32b, idx, idx2, (size_t)n, 0u, bits32, st));
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb2, g64, s64, idx2, idx, (size_t)n, 0u, bits64, st));
    ENSURE(w.temp, std::max<size_t>(std::max(tb, tb2), 16));
    HIP_TRY(rocprim::radix_sort_pairs(w.temp.p, tb, k32, k32b, idx, idx2, (size_t)n, 0u, bits32, st));
    mw_gather_kernel<<<ms_blocks(n), 256, 0, st>>>(w.k64.as<uint64_t>(), idx2, n, g64);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(w.temp.p, tb2, g64, s64, idx2, idx, (size_t)n, 0u, bits64, st));
    return 0;
}

int weld_scan(WeldWork& w, const int32_t* in, int32_t* out, int64_t n, hipStream_t st)
{
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    ENSURE(w.temp, std::max<size_t>(tb, 16));
    HIP_TRY(rocprim::exclusive_scan(w.temp.p, tb, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    return 0;
}

// The weld of the device mesh on the current device, after the work queued on `st`; synchronous.  d_tris == nullptr: the soup.
// Nothing is written to d_verts_out / d_tris_out before the snap range check has passed.  Leaves vert_map in w.vert_map
// [n_verts] and tri_map in w.tri_map [n_tris].
int weld_core(const float* d_verts, int64_t nv, const int32_t* d_tris, int64_t nt, double snap, int32_t flags, hipStream_t st, WeldWork& w,
              float* d_verts_out, int32_t* d_tris_out, int64_t totals[8])
{
    for (int k = 0; k < 8; ++k) totals[k] = 0;
    if (nv == 0) return 0;   // (no vertex: no valid triangle either)
    uint64_t h_small[MW_SMALL] = {};
    ENSURE(w.small, sizeof h_small);
    uint64_t* small = w.small.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(small, 0, sizeof h_small, st));
    const int64_t nmax = std::max(nv, nt);
    ENSURE(w.k32, sizeof(uint32_t) * (size_t)nmax);
    ENSURE(w.k32b, sizeof(uint32_t) * (size_t)nmax);
    ENSURE(w.idx, sizeof(uint32_t) * (size_t)nmax);
    ENSURE(w.idx2, sizeof(uint32_t) * (size_t)nmax);
    ENSURE(w.k64, sizeof(uint64_t) * (size_t)nmax);
    ENSURE(w.g64, sizeof(uint64_t) * (size_t)nmax);
    ENSURE(w.s64, sizeof(uint64_t) * (size_t)nmax);
    ENSURE(w.hp, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.hp2, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.rep, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.is_rep, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.num, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.class_of, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.vert_map, sizeof(int32_t) * (size_t)nv);
    int32_t *hp = w.hp.as<int32_t>(), *hp2 = w.hp2.as<int32_t>(), *rep = w.rep.as<int32_t>(), *is_rep = w.is_rep.as<int32_t>();
    int32_t *num = w.num.as<int32_t>(), *class_of = w.class_of.as<int32_t>();
    mw_vkey_kernel<<<ms_blocks(nv), 256, 0, st>>>(d_verts, nv, snap, w.k32.as<uint32_t>(), w.k64.as<uint64_t>(), w.idx.as<uint32_t>(), small);
    HIP_TRY(hipGetLastError());
    int rc = weld_sort(w, nv, 32u, 64u, st);
    if (rc) return rc;
    mw_vhead_kernel<<<ms_blocks(nv), 256, 0, st>>>(w.s64.as<uint64_t>(), w.idx.as<uint32_t>(), w.k32.as<uint32_t>(), nv, hp);
    HIP_TRY(hipGetLastError());
    {
        size_t tb = 0;
        HIP_TRY(rocprim::inclusive_scan(nullptr, tb, hp, hp2, (size_t)nv, rocprim::maximum<int32_t>(), st));
        ENSURE(w.temp, std::max<size_t>(tb, 16));
        HIP_TRY(rocprim::inclusive_scan(w.temp.p, tb, hp, hp2, (size_t)nv, rocprim::maximum<int32_t>(), st));
    }
    mw_rep_kernel<<<ms_blocks(nv), 256, 0, st>>>(w.idx.as<uint32_t>(), hp2, nv, rep, is_rep);
    HIP_TRY(hipGetLastError());
    if ((rc = weld_scan(w, is_rep, num, nv, st))) return rc;
    mw_class_kernel<<<ms_blocks(nv), 256, 0, st>>>(rep, num, is_rep, nv, class_of, small);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_small[MW_OVERFLOW])
        return fail(R2S_ERR_ARG, "mesh_weld: snap = %g is too fine for the extent of the mesh (%llu vertices have a cell index outside [-2^31, 2^31))",
                    snap, (unsigned long long)h_small[MW_OVERFLOW]);
    const int64_t ncls = (int64_t)h_small[MW_CLASSES];
    ENSURE(w.used, sizeof(int32_t) * (size_t)ncls);
    ENSURE(w.unum, sizeof(int32_t) * (size_t)ncls);
    ENSURE(w.final_of, sizeof(int32_t) * (size_t)ncls);
    int32_t *used = w.used.as<int32_t>(), *unum = w.unum.as<int32_t>(), *final_of = w.final_of.as<int32_t>();
    HIP_TRY(hipMemsetAsync(used, 0, sizeof(int32_t) * (size_t)ncls, st));
    if (nt > 0) {
        ENSURE(w.is_dup, sizeof(int32_t) * (size_t)nt);
        ENSURE(w.keep, sizeof(int32_t) * (size_t)nt);
        ENSURE(w.tnum, sizeof(int32_t) * (size_t)nt);
        ENSURE(w.tri_map, sizeof(int32_t) * (size_t)nt);
        int32_t *is_dup = w.is_dup.as<int32_t>(), *keep = w.keep.as<int32_t>(), *tnum = w.tnum.as<int32_t>();
        mw_tkey_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, class_of, nt, (uint64_t)ncls, w.k32.as<uint32_t>(), w.k64.as<uint64_t>(),
                                                     w.idx.as<uint32_t>(), small);
        HIP_TRY(hipGetLastError());
        const unsigned cb = ms_bits((uint64_t)ncls);   // (the collapsed key, ncls in the high word, included)
        if ((rc = weld_sort(w, nt, std::min(cb + 1u, 32u), 32u + cb, st))) return rc;
        mw_tdup_kernel<<<ms_blocks(nt), 256, 0, st>>>(w.s64.as<uint64_t>(), w.idx.as<uint32_t>(), w.k32.as<uint32_t>(), nt, (uint64_t)ncls,
                                                     is_dup, small);
        HIP_TRY(hipGetLastError());
        mw_tkeep_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, class_of, nt, is_dup, flags, keep, used);
        HIP_TRY(hipGetLastError());
        if ((rc = weld_scan(w, keep, tnum, nt, st))) return rc;
    }
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
