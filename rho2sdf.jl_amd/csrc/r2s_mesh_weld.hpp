// The stages r2s_mesh_weld.hip and r2s_mesh_simplify.hip share, so that "the cell of a vertex" and "the class of a triangle" have
// one definition (include/rho2sdf_hip.h: the partition of r2s_mesh_simplify IS that of r2s_mesh_weld with snap = cell):
//   mw_cell, the one floating-point operation pair of the weld; the key, head, representative and class kernels; the triangle
//   key, duplicate, keep and output kernels; the two-key stable sort (weld_sort) and the scan (weld_scan);
//   mw_classes: the vertex stage up to class_of and the range check of the snap mode;
//   mw_triangles: the triangle stage up to keep / tnum / used.
// Everything has internal linkage, as in r2s_mesh_graph.hpp: each of the two files gets its own copy of a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_graph.hpp"

namespace {
using namespace r2s_int;

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

// the buffers of the two shared stages (a tool's work struct derives from this)
struct MwBufs {
    DevBuf small, k32, k32b, k64, g64, s64, idx, idx2, temp, hp, hp2, rep, is_rep, num, class_of, is_dup, keep, tnum, used, vert_map, tri_map;
};

// sorts n (z / high word, index) records of w.k32 / w.k64 / w.idx by the 64-bit word, then the 32-bit word, stably: the order
// ends in w.idx, the sorted 64-bit words in w.s64
int weld_sort(MwBufs& w, int64_t n, unsigned bits32, unsigned bits64, hipStream_t st)
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

int weld_scan(MwBufs& w, const int32_t* in, int32_t* out, int64_t n, hipStream_t st)
{
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    ENSURE(w.temp, std::max<size_t>(tb, 16));
    HIP_TRY(rocprim::exclusive_scan(w.temp.p, tb, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    return 0;
}

// The vertex stage on `st` for nv > 0 device vertices (the keys are sized for max(nv, nt): the triangle stage reuses them): leaves
// class_of [nv] (classes in first-occurrence order), rep and is_rep in w and *ncls = the number of classes; zeroes w.small first.
// Synchronises `st` once.  Snap mode: a cell index outside [-2^31, 2^31) is refused here, before any output is written.
int mw_classes(MwBufs& w, const char* who, const float* d_verts, int64_t nv, int64_t nt, double snap, hipStream_t st, int64_t* ncls)
{
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
        return fail(R2S_ERR_ARG, "%s: snap = %g is too fine for the extent of the mesh (%llu vertices have a cell index outside [-2^31, 2^31))",
                    who, snap, (unsigned long long)h_small[MW_OVERFLOW]);
    *ncls = (int64_t)h_small[MW_CLASSES];
    return 0;
}

// The triangle stage on `st` behind mw_classes: used [ncls] = the classes a surviving triangle references, and for nt > 0 is_dup,
// keep (what survives `flags`) and tnum, its exclusive scan; the collapsed, duplicate and opposite counts go to w.small.
int mw_triangles(MwBufs& w, const int32_t* d_tris, int64_t nt, int64_t ncls, int32_t flags, hipStream_t st)
{
    uint64_t* small = w.small.as<uint64_t>();
    const int32_t* class_of = w.class_of.as<int32_t>();
    ENSURE(w.used, sizeof(int32_t) * (size_t)ncls);
    int32_t* used = w.used.as<int32_t>();
    HIP_TRY(hipMemsetAsync(used, 0, sizeof(int32_t) * (size_t)ncls, st));
    if (nt == 0) return 0;
    ENSURE(w.is_dup, sizeof(int32_t) * (size_t)nt);
    ENSURE(w.keep, sizeof(int32_t) * (size_t)nt);
    ENSURE(w.tnum, sizeof(int32_t) * (size_t)nt);
    ENSURE(w.tri_map, sizeof(int32_t) * (size_t)nt);
    int32_t *is_dup = w.is_dup.as<int32_t>(), *keep = w.keep.as<int32_t>(), *tnum = w.tnum.as<int32_t>();
    mw_tkey_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, class_of, nt, (uint64_t)ncls, w.k32.as<uint32_t>(), w.k64.as<uint64_t>(),
                                                 w.idx.as<uint32_t>(), small);
    HIP_TRY(hipGetLastError());
    const unsigned cb = ms_bits((uint64_t)ncls);   // (the collapsed key, ncls in the high word, included)
    if (const int rc = weld_sort(w, nt, std::min(cb + 1u, 32u), 32u + cb, st)) return rc;
    mw_tdup_kernel<<<ms_blocks(nt), 256, 0, st>>>(w.s64.as<uint64_t>(), w.idx.as<uint32_t>(), w.k32.as<uint32_t>(), nt, (uint64_t)ncls, is_dup,
                                                 small);
    HIP_TRY(hipGetLastError());
    mw_tkeep_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, class_of, nt, is_dup, flags, keep, used);
    HIP_TRY(hipGetLastError());
    return weld_scan(w, keep, tnum, nt, st);
}

}  // namespace
