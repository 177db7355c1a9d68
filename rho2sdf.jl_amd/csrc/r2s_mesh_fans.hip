// Mesh fans: the fans of triangle corners round every vertex of a triangle mesh, the non-manifold (pinched) vertices, and the
// split that gives every fan its own copy of the vertex (include/rho2sdf_hip.h, r2s_mesh_fans; DESIGN.md "Mesh fans").
//   ms_sort_half_edges (r2s_mesh_graph.hpp) ms_key_kernel<3, false>: one half-edge key per corner, the orient's keys
//                      (min << 33 | max << 1 | direction), payload 3t + c; parent[k] = k on the graph of the 3 n_tris CORNERS
//                      -> rocPRIM radix sort of pairs
//   mf_union_kernel    every member of an edge run but its first: at each end of the edge, this triangle's corner at that end
//                      joins the predecessor's corner at that end (the shells' union-find: larger root under the smaller, so a
//                      fan's root is its smallest corner)
//   mf_flatten_kernel  label[k] = root(k), none for the corners of a collapsed triangle; root flags
//   -> rocPRIM exclusive scan (integers) -> mf_compact_kernel: the roots in corner order, keyed by their vertex
//   -> stable radix sort of the roots by vertex: the position is the fan number
//   mf_number_kernel   fan number of every root, vertex and first corner of every fan, fans_of_vert, "not the first fan of its
//                      vertex" -> rocPRIM exclusive scan -> mf_index_kernel: the vertex index every fan gets under the split
//   mf_corner_kernel   fan_of_corner, n_corners per fan;  mf_edge_kernel: the head of every edge run adds the edge and its class
//                      to the fan at each of its two ends;  mf_class_kernel: the class of every fan, the totals
//   mf_apply_*         the split: tris_out per corner, the copied vertices, the vertices of the further fans
// Integer work only: no floating-point instruction; the vertex coordinates are moved as 32-bit words.  Counts are integer atomics.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_graph.hpp"

using namespace r2s_int;

namespace {

constexpr int MF_NCNT = 8;
constexpr int64_t MF_MAX_TRIS = (((int64_t)1 << 31) - 1) / 3;   // 3 n_tris < 2^31: corner ids and fan numbers are int32
constexpr uint32_t MF_NONE = 0xffffffffu;                        // the label of a collapsed triangle's corners
// slots of the small device array
constexpr int MF_COLLAPSED = 0, MF_NFANS = 1, MF_NADDED = 2, MF_PINCHED = 3, MF_COMPLEX = 4, MF_OPEN = 5;
constexpr int MF_SMALL = 8;
// columns of the per-fan record
constexpr int MF_VERTEX = 0, MF_FIRST = 1, MF_NCORNERS = 2, MF_NEDGES = 3, MF_NONMANIFOLD = 6, MF_CLASS = 7;

__device__ inline uint32_t mf_next(uint32_t k) { return k % 3u == 2u ? k - 2u : k + 1u; }   // the next corner of k's triangle

// the corners of half-edge (key, k = 3t + c) at the smaller and at the larger vertex of its edge: the half-edge leaves corner c
// and arrives at corner (c + 1) % 3; direction bit 0: it leaves the smaller vertex
__device__ inline void mf_ends(uint64_t key, uint32_t k, uint32_t& at_min, uint32_t& at_max)
{
    const uint32_t nx = mf_next(k);
    const bool up = (key & 1ull) == 0ull;
    at_min = up ? k : nx;
    at_max = up ? nx : k;
}

// one thread per sorted half-edge: a member of a run joins its predecessor at both ends of the edge, whatever the run's class
__global__ void __launch_bounds__(256) mf_union_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                        uint64_t ckey, uint32_t* parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= nh) return;
    const uint64_t k = keys[i], p = keys[i - 1];
    if (k >= ckey || (k >> 1) != (p >> 1)) return;
    uint32_t a0, a1, b0, b1;
    mf_ends(p, vals[i - 1], a0, a1);
    mf_ends(k, vals[i], b0, b1);
    ms_union(parent, a0, b0);
    ms_union(parent, a1, b1);
}

// one thread per triangle: label[k] = root(k) (MF_NONE in a collapsed triangle), flag[k] = 1 for the first corner of a fan
__global__ void __launch_bounds__(256) mf_flatten_kernel(const int32_t* __restrict__ tris, int64_t n, uint32_t* parent, uint32_t* __restrict__ label,
                                                          int32_t* __restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int32_t i0, i1, i2;
    const bool col = ms_collapsed(tris, t, i0, i1, i2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t k = (uint32_t)(3 * t + c);
        const uint32_t r = col ? MF_NONE : ms_find(parent, k);
        label[k] = r;
        flag[k] = r == k ? 1 : 0;
    }
}

// pos = the exclusive scan of flag: the roots in corner order with their vertices; n_fans
__global__ void __launch_bounds__(256) mf_compact_kernel(const int32_t* __restrict__ tris, int64_t nh, const int32_t* __restrict__ flag,
                                                          const int32_t* __restrict__ pos, uint32_t* __restrict__ rkey, uint32_t* __restrict__ rval,
                                                          uint64_t* __restrict__ small)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nh) return;
    const int32_t f = flag[k], p = pos[k];
    if (f) {
        rkey[p] = (uint32_t)tris[k];
        rval[p] = (uint32_t)k;
    }
    if (k == nh - 1) small[MF_NFANS] = (uint64_t)(p + f);
}

// one thread per fan i (the roots sorted by vertex, ascending corner within a vertex): its number at its root, the head of
// its record, fans_of_vert, and whether it is a further fan of its vertex
__global__ void __launch_bounds__(256) mf_number_kernel(const uint32_t* __restrict__ fvert, const uint32_t* __restrict__ froot, int64_t nf,
                                                         int32_t* __restrict__ fan_at, int32_t* __restrict__ further, int64_t* __restrict__ counts,
                                                         int32_t* __restrict__ fans_of_vert)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const uint32_t v = fvert[i], r = froot[i];
    fan_at[r] = (int32_t)i;
    further[i] = (i > 0 && fvert[i - 1] == v) ? 1 : 0;
    counts[i * MF_NCNT + MF_VERTEX] = (int64_t)v;
    counts[i * MF_NCNT + MF_FIRST] = (int64_t)r;
    atomicAdd(&fans_of_vert[v], 1);
}

// extra = the exclusive scan of further: the vertex index of fan i under the split (int64: the host refuses what does not fit)
__global__ void __launch_bounds__(256) mf_index_kernel(const uint32_t* __restrict__ fvert, int64_t nf, int64_t n_verts,
                                                        const int32_t* __restrict__ further, const int32_t* __restrict__ extra,
                                                        int32_t* __restrict__ index_of, uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const int32_t f = further[i], e = extra[i];
    index_of[i] = f ? (int32_t)(n_verts + (int64_t)e) : (int32_t)fvert[i];
    if (i == nf - 1) small[MF_NADDED] = (uint64_t)((int64_t)e + f);
}

// one thread per corner: its fan, and one more corner for that fan
__global__ void __launch_bounds__(256) mf_corner_kernel(int64_t nh, const uint32_t* __restrict__ label, const int32_t* __restrict__ fan_at,
                                                         int32_t* __restrict__ fan_of_corner, int64_t* __restrict__ counts)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t fan = -1;
    if (k < nh) {
        const uint32_t l = label[k];
        if (l != MF_NONE) fan = fan_at[l];
        fan_of_corner[k] = fan;
    }
    const bool add[1] = {true};
    ms_count<1, MF_NCNT>(fan >= 0, fan, add, MF_NCORNERS, counts);
}

// one thread per sorted half-edge; the head of a run adds the edge and its class to the fan at the smaller and to the fan at the
// larger vertex (all corners of a vertex on one edge are in one fan: the head's corners name them)
__global__ void __launch_bounds__(256) mf_edge_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, const int32_t* __restrict__ fan_of_corner, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool add[4] = {false, false, false, false};   // an edge, boundary, flipped, non-manifold
    int32_t fa = -1, fb = -1;
    bool head = false;
    if (i < nh && keys[i] < ckey) {
        const int size = ms_run_size(keys, i, nh, head);
        if (head) {
            add[0] = true;
            add[1] = size == 1;
            add[2] = size == 2 && ((keys[i + 1] ^ keys[i]) & 1ull) == 0ull;
            add[3] = size == 3;
            uint32_t c0, c1;
            mf_ends(keys[i], vals[i], c0, c1);
            fa = fan_of_corner[c0];
            fb = fan_of_corner[c1];
        }
    }
    ms_count<4, MF_NCNT>(head, fa, add, MF_NEDGES, counts);
    __syncthreads();   // (ms_count's LDS words are read to its end)
    ms_count<4, MF_NCNT>(head, fb, add, MF_NEDGES, counts);
}

// one thread per fan: its class; pinched vertices (counted at a vertex's first fan), complex and open fans
__global__ void __launch_bounds__(256) mf_class_kernel(const uint32_t* __restrict__ fvert, int64_t nf, const int32_t* __restrict__ further,
                                                        int64_t* __restrict__ counts, uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool c[3] = {false, false, false};   // pinched, complex, open
    if (i < nf) {
        int64_t* rec = counts + i * MF_NCNT;
        const int64_t cls = rec[MF_NONMANIFOLD] > 0 ? 2 : (rec[4] > 0 ? 1 : 0);
        rec[MF_CLASS] = cls;
        c[0] = !further[i] && i + 1 < nf && fvert[i + 1] == fvert[i];
        c[1] = cls == 2;
        c[2] = cls == 1;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned long long m = __ballot(c[k]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)&small[MF_PINCHED + k], (unsigned long long)__popcll(m));
    }
}

// the split, one thread per corner: the index of the corner's fan; a collapsed triangle is copied
__global__ void __launch_bounds__(256) mf_apply_tris_kernel(const int32_t* __restrict__ tris, int64_t nh, const int32_t* __restrict__ fan_of_corner,
                                                             const int32_t* __restrict__ index_of, int32_t* __restrict__ tris_out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nh) return;
    const int32_t f = fan_of_corner[k];
    tris_out[k] = f < 0 ? tris[k] : index_of[f];
}

// the split, one thread per input vertex: the vertex itself, bit for bit
__global__ void __launch_bounds__(256) mf_apply_verts_kernel(const uint32_t* __restrict__ verts, int64_t n_verts, uint32_t* __restrict__ verts_out,
                                                              int32_t* __restrict__ vert_of_out)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) verts_out[3 * v + a] = verts[3 * v + a];
    vert_of_out[v] = (int32_t)v;
}

// the split, one thread per fan: a further fan of a vertex gets a copy of it at its new index
__global__ void __launch_bounds__(256) mf_apply_further_kernel(const uint32_t* __restrict__ verts, const uint32_t* __restrict__ fvert, int64_t nf,
                                                                const int32_t* __restrict__ further, const int32_t* __restrict__ index_of,
                                                                uint32_t* __restrict__ verts_out, int32_t* __restrict__ vert_of_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf || !further[i]) return;
    const int64_t j = (int64_t)index_of[i], v = (int64_t)fvert[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) verts_out[3 * j + a] = verts[3 * v + a];
    vert_of_out[j] = (int32_t)v;
}

// work buffers of the fan calls, kept per device between calls (r2s_release_cache frees them)
struct FanWork : MsHalfEdgeBufs {
    DevBuf verts, tris, flag, small, parent, label, rflag, pos, rkey, rkey2, rval, rval2, fan_at, further, extra, index_of, foc, fov, counts,
        tris_out, verts_out, vert_of;
};
PerDevice<FanWork> g_fans_work;

thread_local std::vector<int64_t> g_last_fans;   // [n][8]

// The fans of the device mesh on the current device, after the work queued on `st`; synchronous.  Leaves fan_of_corner in
// w.foc [3 n], fans_of_vert in w.fov [n_verts], the records in w.counts [n_fans] and what mf_apply needs in w.rkey2 / w.further
// / w.index_of; the scalars go to the host pointers.
int fans_core(int64_t n_verts, const int32_t* d_tris, int64_t n, hipStream_t st, FanWork& w, int64_t* n_fans, int64_t* n_verts_out,
              int64_t totals[8])
{
    uint64_t h_small[MF_SMALL] = {};
    ENSURE(w.small, sizeof h_small);
    uint64_t* small = w.small.as<uint64_t>();
    HIP_TRY(hipMemcpyAsync(small, h_small, sizeof h_small, hipMemcpyHostToDevice, st));
    ENSURE(w.fov, sizeof(int32_t) * (size_t)std::max<int64_t>(n_verts, 1));
    if (n_verts > 0) HIP_TRY(hipMemsetAsync(w.fov.p, 0, sizeof(int32_t) * (size_t)n_verts, st));
    const int64_t nh = 3 * n;
    const uint64_t ckey = ms_collapsed_key(n_verts);
    int64_t nf = 0;
    if (n > 0) {
        ENSURE(w.parent, sizeof(uint32_t) * (size_t)nh);
        ENSURE(w.label, sizeof(uint32_t) * (size_t)nh);
        ENSURE(w.rflag, sizeof(int32_t) * (size_t)nh);
        ENSURE(w.pos, sizeof(int32_t) * (size_t)nh);
        ENSURE(w.rkey, sizeof(uint32_t) * (size_t)nh);
        ENSURE(w.rval, sizeof(uint32_t) * (size_t)nh);
        ENSURE(w.fan_at, sizeof(int32_t) * (size_t)nh);
        ENSURE(w.foc, sizeof(int32_t) * (size_t)nh);
        uint32_t* parent = w.parent.as<uint32_t>();
        size_t tb = 0, sb = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, sb, w.rflag.as<int32_t>(), w.pos.as<int32_t>(), (int32_t)0, (size_t)nh,
                                        rocprim::plus<int32_t>(), st));
        int rc = ms_sort_half_edges<3, false>(w, d_tris, n, n_verts, parent, nullptr, small + MF_COLLAPSED, sb, st);
        if (rc) return rc;
        const uint64_t* keys2 = w.keys2.as<uint64_t>();
        const uint32_t* vals2 = w.vals2.as<uint32_t>();
        mf_union_kernel<<<ms_blocks(nh), 256, 0, st>>>(keys2, vals2, nh, ckey, parent);
        HIP_TRY(hipGetLastError());
        mf_flatten_kernel<<<ms_blocks(n), 256, 0, st>>>(d_tris, n, parent, w.label.as<uint32_t>(), w.rflag.as<int32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb, w.rflag.as<int32_t>(), w.pos.as<int32_t>(), (int32_t)0, (size_t)nh,
                                        rocprim::plus<int32_t>(), st));
        mf_compact_kernel<<<ms_blocks(nh), 256, 0, st>>>(d_tris, nh, w.rflag.as<int32_t>(), w.pos.as<int32_t>(), w.rkey.as<uint32_t>(),
                                                      w.rval.as<uint32_t>(), small);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        nf = (int64_t)h_small[MF_NFANS];
        ENSURE(w.counts, sizeof(int64_t) * MF_NCNT * (size_t)std::max<int64_t>(nf, 1));
        int64_t* counts = w.counts.as<int64_t>();
        if (nf > 0) {
            ENSURE(w.rkey2, sizeof(uint32_t) * (size_t)nf);
            ENSURE(w.rval2, sizeof(uint32_t) * (size_t)nf);
            ENSURE(w.further, sizeof(int32_t) * (size_t)nf);
            ENSURE(w.extra, sizeof(int32_t) * (size_t)nf);
            ENSURE(w.index_of, sizeof(int32_t) * (size_t)nf);
            uint32_t *rkey = w.rkey.as<uint32_t>(), *rkey2 = w.rkey2.as<uint32_t>(), *rval = w.rval.as<uint32_t>(), *rval2 = w.rval2.as<uint32_t>();
            int32_t *further = w.further.as<int32_t>(), *extra = w.extra.as<int32_t>();
            const unsigned vbits = ms_bits((uint64_t)n_verts);
            HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, rkey, rkey2, rval, rval2, (size_t)nf, 0u, vbits, st));
            HIP_TRY(rocprim::exclusive_scan(nullptr, sb, further, extra, (int32_t)0, (size_t)nf, rocprim::plus<int32_t>(), st));
            ENSURE(w.temp, std::max<size_t>(std::max(tb, sb), 16));
            HIP_TRY(rocprim::radix_sort_pairs(w.temp.p, tb, rkey, rkey2, rval, rval2, (size_t)nf, 0u, vbits, st));
            HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * MF_NCNT * (size_t)nf, st));
            mf_number_kernel<<<ms_blocks(nf), 256, 0, st>>>(rkey2, rval2, nf, w.fan_at.as<int32_t>(), further, counts, w.fov.as<int32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb, further, extra, (int32_t)0, (size_t)nf, rocprim::plus<int32_t>(), st));
            mf_index_kernel<<<ms_blocks(nf), 256, 0, st>>>(rkey2, nf, n_verts, further, extra, w.index_of.as<int32_t>(), small);
            HIP_TRY(hipGetLastError());
        }
        mf_corner_kernel<<<ms_blocks(nh), 256, 0, st>>>(nh, w.label.as<uint32_t>(), w.fan_at.as<int32_t>(), w.foc.as<int32_t>(), counts);
        HIP_TRY(hipGetLastError());
        if (nf > 0) {
            // (keys2 / vals2 still hold the sorted half-edges)
            mf_edge_kernel<<<ms_blocks(nh), 256, 0, st>>>(keys2, vals2, nh, ckey, w.foc.as<int32_t>(), counts);
            HIP_TRY(hipGetLastError());
            mf_class_kernel<<<ms_blocks(nf), 256, 0, st>>>(w.rkey2.as<uint32_t>(), nf, w.further.as<int32_t>(), counts, small);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t added = (int64_t)h_small[MF_NADDED], used = nf - added;
    if (n_verts + added > INT32_MAX)
        return fail(R2S_ERR_UNSUPPORTED, "mesh_fans: the split needs %lld vertices, beyond 32-bit indices", (long long)(n_verts + added));
    *n_fans = nf;
    *n_verts_out = n_verts + added;
    totals[0] = nf, totals[1] = n, totals[2] = (int64_t)h_small[MF_COLLAPSED], totals[3] = used, totals[4] = n_verts - used;
    totals[5] = (int64_t)h_small[MF_PINCHED], totals[6] = (int64_t)h_small[MF_COMPLEX], totals[7] = (int64_t)h_small[MF_OPEN];
    return 0;
}

// queues the split of the mesh fans_core has just analysed on `st` (room for n_verts_out vertices is the caller's business)
int fans_apply(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, int64_t nf, hipStream_t st, FanWork& w,
               int32_t* d_tris_out, float* d_verts_out, int32_t* d_vert_of_out)
{
    const uint32_t* vin = reinterpret_cast<const uint32_t*>(d_verts);
    uint32_t* vout = reinterpret_cast<uint32_t*>(d_verts_out);
    if (n > 0) {
        mf_apply_tris_kernel<<<ms_blocks(3 * n), 256, 0, st>>>(d_tris, 3 * n, w.foc.as<int32_t>(), w.index_of.as<int32_t>(), d_tris_out);
        HIP_TRY(hipGetLastError());
    }
    if (n_verts > 0) {
        mf_apply_verts_kernel<<<ms_blocks(n_verts), 256, 0, st>>>(vin, n_verts, vout, d_vert_of_out);
        HIP_TRY(hipGetLastError());
    }
    if (nf > 0) {
        mf_apply_further_kernel<<<ms_blocks(nf), 256, 0, st>>>(vin, w.rkey2.as<uint32_t>(), nf, w.further.as<int32_t>(), w.index_of.as<int32_t>(),
                                                            vout, d_vert_of_out);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the checks that need no device; *split: the split was asked for
int fans_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, const void* fan_of_corner, const void* fans_of_vert,
              const void* tris_out, const void* verts_out, const void* vert_of_out, int64_t vert_capacity, const int64_t* n_fans,
              const int64_t* n_verts_out, const int64_t* totals, bool* split)
{
    const int rc = mesh_args("mesh_fans", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (n_tris > MF_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_fans: 3 * %lld corners reach 2^31", (long long)n_tris);
    if (!n_fans || !n_verts_out || !totals) return fail(R2S_ERR_ARG, "mesh_fans: null n_fans / n_verts_out / totals");
    if (vert_capacity < 0) return fail(R2S_ERR_ARG, "mesh_fans: negative vert_capacity");
    *split = tris_out || verts_out || vert_of_out;
    if (*split && ((n_tris > 0 && !tris_out) || !verts_out || !vert_of_out))
        return fail(R2S_ERR_ARG, "mesh_fans: the split needs tris_out, verts_out and vert_of_out together");
    const Span in[2] = {{verts, vert_bytes(n_verts)}, {tris, tri_bytes(n_tris)}},
               out[5] = {{fan_of_corner, tri_bytes(n_tris)}, {fans_of_vert, sizeof(int32_t) * (size_t)n_verts}, {tris_out, tri_bytes(n_tris)},
                         {verts_out, vert_bytes(vert_capacity)}, {vert_of_out, sizeof(int32_t) * (size_t)vert_capacity}};
    for (const auto& o : out)
        for (const auto& i : in)
            if (overlaps(o, i)) return fail(R2S_ERR_ARG, "mesh_fans: an output overlaps an input");
    return 0;
}

// One call for both kinds of caller: the core, the split when it was asked for and vert_capacity holds n_verts_out vertices,
// then fan_of_corner, fans_of_vert, the records and the scalars.  A host caller's records are kept whole for r2s_last_mesh_fans;
// a device caller gets them when fan_capacity holds all of them, else none.
int fans_run(MeshCall<FanWork>& c, int64_t n_verts, int64_t n_tris, int32_t* fan_of_corner, int32_t* fans_of_vert, int64_t* d_counts,
             int64_t fan_capacity, bool split, int32_t* tris_out, float* verts_out, int32_t* vert_of_out, int64_t vert_capacity,
             int64_t* n_fans, int64_t* n_verts_out, int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    FanWork& w = c.work();
    std::vector<int64_t> tab;
    int64_t nf = 0, nvo = 0, tot[8];
    if ((rc = fans_core(n_verts, c.d_tris(), n_tris, c.stream(), w, &nf, &nvo, tot))) return rc;
    const bool room = split && vert_capacity >= nvo;
    int32_t *d_tris_out = nullptr, *d_vert_of = nullptr;
    float* d_verts_out = nullptr;
    if (room &&
        ((rc = c.staged(w.tris_out, tris_out, tri_bytes(std::max<int64_t>(n_tris, 1)), d_tris_out)) ||
         (rc = c.staged(w.verts_out, verts_out, vert_bytes(std::max<int64_t>(nvo, 1)), d_verts_out)) ||
         (rc = c.staged(w.vert_of, vert_of_out, sizeof(int32_t) * (size_t)std::max<int64_t>(nvo, 1), d_vert_of)) ||
         (rc = fans_apply(c.d_verts(), n_verts, c.d_tris(), n_tris, nf, c.stream(), w, d_tris_out, d_verts_out, d_vert_of))))
        return rc;
    if ((rc = c.table(tab, d_counts, fan_capacity >= nf, w.counts, (size_t)nf * MF_NCNT)) ||
        (rc = c.deliver(fan_of_corner, w.foc.p, tri_bytes(n_tris))) || (rc = c.deliver(fans_of_vert, w.fov.p, sizeof(int32_t) * (size_t)n_verts)) ||
        (rc = c.deliver(room ? tris_out : nullptr, d_tris_out, tri_bytes(n_tris))) ||
        (rc = c.deliver(room ? verts_out : nullptr, d_verts_out, vert_bytes(nvo))) ||
        (rc = c.deliver(room ? vert_of_out : nullptr, d_vert_of, sizeof(int32_t) * (size_t)nvo)) || (rc = c.finish()))
        return rc;
    if (c.is_host()) g_last_fans = std::move(tab);
    *n_fans = nf;
    *n_verts_out = nvo;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_fans(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device, int32_t* fan_of_corner_out,
                  int32_t* fans_of_vert_out, int32_t* tris_out, float* verts_out, int32_t* vert_of_out, int64_t vert_capacity,
                  int64_t* n_fans, int64_t* n_verts_out, int64_t totals[8])
{
    bool split = false;
    if (const int rc = fans_args(verts, n_verts, tris, n_tris, fan_of_corner_out, fans_of_vert_out, tris_out, verts_out, vert_of_out,
                                 vert_capacity, n_fans, n_verts_out, totals, &split))
        return rc;
    MeshCall<FanWork> call("mesh_fans", g_fans_work, verts, n_verts, tris, n_tris, device);
    return fans_run(call, n_verts, n_tris, fan_of_corner_out, fans_of_vert_out, nullptr, 0, split, tris_out, verts_out, vert_of_out, vert_capacity,
                    n_fans, n_verts_out, totals);
}

int r2s_last_mesh_fans(int64_t* counts_out, int64_t capacity, int64_t* n_fans)
{
    if (!n_fans || capacity < 0 || (capacity > 0 && !counts_out)) return fail(R2S_ERR_ARG, "last_mesh_fans: null output or negative capacity");
    *n_fans = (int64_t)(g_last_fans.size() / MF_NCNT);
    copy_rows(counts_out, g_last_fans, MF_NCNT, capacity, *n_fans);
    return 0;
}

int r2s_mesh_fans_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, int32_t* d_fan_of_corner,
                      int32_t* d_fans_of_vert, int64_t* d_counts, int64_t fan_capacity, int32_t* d_tris_out, float* d_verts_out,
                      int32_t* d_vert_of_out, int64_t vert_capacity, int64_t* n_fans, int64_t* n_verts_out, int64_t totals[8], void* stream)
{
    bool split = false;
    if (const int rc = fans_args(d_verts, n_verts, d_tris, n_tris, d_fan_of_corner, d_fans_of_vert, d_tris_out, d_verts_out, d_vert_of_out,
                                 vert_capacity, n_fans, n_verts_out, totals, &split))
        return rc;
    if (fan_capacity < 0 || (fan_capacity > 0 && !d_counts)) return fail(R2S_ERR_ARG, "mesh_fans: null table or negative fan_capacity");
    MeshCall<FanWork> call("mesh_fans", g_fans_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return fans_run(call, n_verts, n_tris, d_fan_of_corner, d_fans_of_vert, d_counts, fan_capacity, split, d_tris_out, d_verts_out, d_vert_of_out,
                    vert_capacity, n_fans, n_verts_out, totals);
}

}  // extern "C"
