// What r2s_mesh_shells.hip, r2s_mesh_sections.hip, r2s_mesh_orient.hip, r2s_mesh_fans.hip, r2s_mesh_holes.hip and
// r2s_mesh_nesting.hip share:
//   the box of the vertices behind the reference point (ms_bounds_kernel, ms_ref_point) and the collapsed-triangle test;
//   the half-edge table: ms_half_edge_keys writes the keys of one triangle, ms_key_kernel is the one key launch of shells,
//     orient, fans, holes and nesting (sections writes its keys in sx_tri_kernel with the same function), ms_sort_half_edges
//     sizes the buffers (MsHalfEdgeBufs), launches the keys and sorts the pairs; ms_run_size reads the sorted runs from any
//     member, ms_run_class names the class of a run at its head (the shells' edge classes, the sections' node classes);
//   the integer union-find with min-root (ms_find, ms_union) and the per-group integer counting (ms_count);
//   the component numbering behind the unions: ms_flatten_kernel<false> (sections, holes) and <true> (shells, nesting: triangles)
//     leave parent = root and flag the roots, the caller scans the flags, ms_number_kernel writes the group of every triangle
//     (shells, orient, nesting), with the sort pairs where asked;
//   the host stages around those kernels: ms_begin_small (shells, orient, holes, sections: the small array and the box),
//     ms_group_triangles (shells, orient, nesting: half-edge table, the tool's unions, flatten, scan, numbering) and
//     ms_sum_by_group (shells, orient: sort by group, segments, the tool's terms, combine);
//   the loop ordering of sections and holes, ms_order_loops: pointer jumping (ms_rank_init_kernel, ms_jump_kernel), the stable
//     sort by group, ms_start_kernel and ms_place_kernel;
//   the segmented Float64 sum every Float64 table of these tools is defined by (include/rho2sdf_hip.h): ms_block_sum, the tree
//     over 256 consecutive sorted items with one partial per (block, segment) at slot block + segment, and ms_combine_kernel,
//     one wavefront per segment; ms_segment_kernel finds the segment starts of shells and orient, with the first item of each.
// r2s_mesh_weld.hip takes the order-preserving bit pattern of a float32 and the launch / bit-count helpers from here.
// Everything has internal linkage: each file gets its own copy of a kernel, and a template only where it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "r2s_common.hpp"

namespace {

inline unsigned ms_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
inline unsigned ms_bits(uint64_t max_value)
{
    unsigned b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

__device__ inline uint32_t ms_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
inline float ms_unordered(uint32_t u)
{
    const uint32_t b = (u >> 31) ? (u & 0x7fffffffu) : ~u;
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}

__device__ inline bool ms_collapsed(const int32_t* __restrict__ tris, int64_t t, int32_t& i0, int32_t& i1, int32_t& i2)
{
    i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    return i0 == i1 || i1 == i2 || i0 == i2;
}

// bb[0..2] = min, bb[3..5] = max over all vertices, as ordered bit patterns (bb starts as ~0, ~0, ~0, 0, 0, 0)
__global__ void __launch_bounds__(256) ms_bounds_kernel(const float* __restrict__ verts, int64_t nverts, uint64_t* __restrict__ small)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (v < nverts) {
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = ms_ordered(verts[3 * v + k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t a = __shfl_xor(lo[k], d, 64), b = __shfl_xor(hi[k], d, 64);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin((unsigned long long*)&small[k], (unsigned long long)lo[k]);
            atomicMax((unsigned long long*)&small[3 + k], (unsigned long long)hi[k]);
        }
    }
}

// the reference point of the header from the six patterns ms_bounds_kernel left: per axis 0.5 * (lo + hi)
inline void ms_ref_point(const uint64_t* bb, int64_t n_verts, double r[3])
{
    for (int k = 0; k < 3; ++k)
        r[k] = n_verts > 0 ? 0.5 * ((double)ms_unordered((uint32_t)bb[k]) + (double)ms_unordered((uint32_t)bb[3 + k])) : 0.0;
}

// How shells, orient, holes and sections open their cores on `st`: h_small = 0 but for the three minima of the box, which
// start at the largest pattern, uploaded to `buf` (sized here), and ms_bounds_kernel over the vertices
template <int N>
int ms_begin_small(DevBuf& buf, uint64_t (&h_small)[N], const float* d_verts, int64_t n_verts, hipStream_t st)
{
    std::fill(h_small, h_small + N, (uint64_t)0);
    h_small[0] = h_small[1] = h_small[2] = 0xffffffffull;
    ENSURE(buf, sizeof h_small);
    HIP_TRY(hipMemcpyAsync(buf.p, h_small, sizeof h_small, hipMemcpyHostToDevice, st));
    if (n_verts > 0) {
        ms_bounds_kernel<<<ms_blocks(n_verts), 256, 0, st>>>(d_verts, n_verts, buf.as<uint64_t>());
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// parents are rewritten by other CUs during the kernel: bypass the per-CU L1
__device__ inline uint32_t ms_load(const uint32_t* L, uint32_t i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; every visited node is pointed at its grandparent (atomicMin: a parent only ever moves to a smaller ancestor)
__device__ inline uint32_t ms_find(uint32_t* L, uint32_t x)
{
    for (;;) {
        const uint32_t p = ms_load(L, x);
        if (p == x) return x;
        const uint32_t g = ms_load(L, p);
        if (g != p) atomicMin(&L[x], g);
        x = g;
    }
}

__device__ inline void ms_union(uint32_t* L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = ms_find(L, a);
        b = ms_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }   // link the larger root under the smaller
        if (atomicCAS(&L[a], a, b) == a) return;             // a was still a root
    }
}

// After the unions: parent[x] = the root of x, the smallest node of its group, and flag[x] = x is that root.  The exclusive
// scan of the flags numbers the groups by ascending root: the group of x is num[parent[x]].
__device__ inline void ms_flatten(uint32_t* parent, uint32_t x, int32_t* __restrict__ flag)
{
    const uint32_t r = ms_find(parent, x);
    if (r != x) atomicMin(&parent[x], r);
    flag[x] = r == x ? 1 : 0;
}

// TRIS: the nodes are triangles, and a collapsed one is in no group (flag 0); else tris is not read
template <bool TRIS>
__global__ void __launch_bounds__(256) ms_flatten_kernel(const int32_t* __restrict__ tris, int64_t n, uint32_t* parent, int32_t* __restrict__ flag)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    int32_t i0, i1, i2;
    if (TRIS && ms_collapsed(tris, x, i0, i1, i2)) {
        flag[x] = 0;
        return;
    }
    ms_flatten(parent, (uint32_t)x, flag);
}

// num = the exclusive scan of the root flags of n triangles: group_of[t] (-1: collapsed) and the number of groups.  The root of
// t is node[t], what ms_flatten_kernel<true> left in parent; DOUBLED: node[t] is the orient's info word, 2 root + parity with
// MS_DOUBLED_FLAG on top.  PAIRS: also the sort pair of t, a collapsed triangle behind every group.
constexpr uint32_t MS_DOUBLED_FLAG = 0x80000000u;   // bit 31 of a doubled-graph word is the caller's (orient: non-orientable)
template <bool DOUBLED, bool PAIRS>
__global__ void __launch_bounds__(256) ms_number_kernel(const int32_t* __restrict__ tris, int64_t n, const uint32_t* __restrict__ node,
                                                         const int32_t* __restrict__ num, const int32_t* __restrict__ flag,
                                                         int32_t* __restrict__ group_of, uint32_t* __restrict__ skey, uint32_t* __restrict__ sval,
                                                         uint64_t* __restrict__ n_groups)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int32_t ng = num[n - 1] + flag[n - 1];
    int32_t i0, i1, i2;
    const int32_t g = ms_collapsed(tris, t, i0, i1, i2) ? -1 : num[DOUBLED ? (node[t] & ~MS_DOUBLED_FLAG) >> 1 : node[t]];
    group_of[t] = g;
    if (PAIRS) {
        skey[t] = g < 0 ? (uint32_t)ng : (uint32_t)g;
        sval[t] = (uint32_t)t;
    }
    if (t == n - 1) *n_groups = (uint64_t)ng;
}

// The sorted half-edge keys are (min << 33) | (max << 1) | direction, the collapsed triangles' keys behind them (below).
// The number of members of the run of sorted half-edge i, capped at 3 (i is a real half-edge: keys[i] < ckey)
__device__ inline int ms_run_size(const uint64_t* __restrict__ keys, int64_t i, int64_t nh, bool& head)
{
    const uint64_t e = keys[i] >> 1;
    const bool p1 = i >= 1 && (keys[i - 1] >> 1) == e, p2 = p1 && i >= 2 && (keys[i - 2] >> 1) == e;
    const bool n1 = i + 1 < nh && (keys[i + 1] >> 1) == e, n2 = n1 && i + 2 < nh && (keys[i + 2] >> 1) == e;
    head = !p1;
    if (!p1 && !n1) return 1;
    return (p2 || (p1 && n1) || n2) ? 3 : 2;
}

// The class of the run whose FIRST member is sorted half-edge i (a real one): alone (a boundary edge), a regular pair (opposite
// directions), a pair in the same direction (a flipped edge), three or more (a non-manifold edge)
enum { MS_RUN_SINGLE = 0, MS_RUN_PAIR = 1, MS_RUN_SAME = 2, MS_RUN_MANY = 3 };
__device__ inline int ms_run_class(const uint64_t* __restrict__ keys, int64_t i, int64_t nh)
{
    const uint64_t k = keys[i], k1 = i + 1 < nh ? keys[i + 1] : ~0ull, k2 = i + 2 < nh ? keys[i + 2] : ~0ull;
    const bool two = (k1 >> 1) == (k >> 1), three = two && (k2 >> 1) == (k >> 1);
    if (!two) return MS_RUN_SINGLE;
    if (three) return MS_RUN_MANY;
    return ((k1 ^ k) & 1ull) == 0ull ? MS_RUN_SAME : MS_RUN_PAIR;
}

// adds 1 to counts[group][col0 + k] (rows of STRIDE) for every k < NC with add[k] set, over the workgroup's active threads: once
// per column when all of them name one group (a shell, a patch), else one atomic per entry.  Called by all 256 threads.
template <int NC, int STRIDE = 8>
__device__ inline void ms_count(bool active, int32_t group, const bool add[NC], int col0, int64_t* __restrict__ counts)
{
    __shared__ int32_t s_group, s_mixed;
    __shared__ uint32_t s_cnt[NC];
    if (threadIdx.x == 0) s_group = -1, s_mixed = 0;
    if (threadIdx.x < NC) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    if (active) atomicCAS(&s_group, -1, group);
    __syncthreads();
    if (active && group != s_group) s_mixed = 1;
    __syncthreads();
    if (s_mixed) {
        if (active) {
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (add[k]) atomicAdd((unsigned long long*)&counts[(int64_t)group * STRIDE + col0 + k], 1ull);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const unsigned long long m = __ballot(active && add[k]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt[k], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < NC && s_group >= 0 && s_cnt[threadIdx.x])
        atomicAdd((unsigned long long*)&counts[(int64_t)s_group * STRIDE + col0 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// ---- the half-edge table -------------------------------------------------------------------------------------------------
// The three half-edges of triangle t: key (min << 33) | (max << 1) | direction of the edge from corner c to corner c + 1
// (direction 1: it leaves the larger vertex), payload 3t + c.  A collapsed triangle gets ckey three times.  Returns whether t
// is collapsed; i = its vertices.
__device__ inline bool ms_half_edge_keys(const int32_t* __restrict__ tris, int64_t t, uint64_t ckey, uint64_t* __restrict__ keys,
                                         uint32_t* __restrict__ vals, int32_t i[3])
{
    const bool col = ms_collapsed(tris, t, i[0], i[1], i[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t u = (uint32_t)i[c], w = (uint32_t)i[c == 2 ? 0 : c + 1];
        const uint64_t mn = u < w ? u : w, mx = u < w ? w : u;
        keys[3 * t + c] = col ? ckey : ((mn << 33) | (mx << 1) | (uint64_t)(u > w));
        vals[3 * t + c] = (uint32_t)(3 * t + c);
    }
    return col;
}

// adds the wavefront's collapsed triangles to *n_collapsed.  Called by all 64 lanes.
__device__ inline void ms_count_collapsed(bool col, uint64_t* __restrict__ n_collapsed)
{
    const unsigned long long m = __ballot(col);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)n_collapsed, (unsigned long long)__popcll(m));
}

// one thread per triangle: its three half-edges, the collapsed count, and what the tool's graph needs in the same launch:
// parent[x] = x for the NPARENT nodes of the triangle (1: the triangle, 2: its two parities, 3: its corners, 0: no parent
// array), VFLAG: the flag of every vertex a real triangle names
template <int NPARENT, bool VFLAG>
__global__ void __launch_bounds__(256) ms_key_kernel(const int32_t* __restrict__ tris, int64_t n, uint64_t ckey, uint64_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals, uint32_t* __restrict__ parent, int32_t* __restrict__ vflag,
                                                      uint64_t* __restrict__ n_collapsed)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool col = false;
    if (t < n) {
        int32_t i[3];
        col = ms_half_edge_keys(tris, t, ckey, keys, vals, i);
#pragma unroll
        for (int k = 0; k < NPARENT; ++k) parent[NPARENT * t + k] = (uint32_t)(NPARENT * t + k);
        if (VFLAG && !col) {
#pragma unroll
            for (int c = 0; c < 3; ++c) vflag[i[c]] = 1;
        }
    }
    ms_count_collapsed(col, n_collapsed);
}

// the key of every half-edge of a collapsed triangle: above every key of a real edge (min < n_verts), so the sort leaves the
// collapsed triangles behind the real runs
inline uint64_t ms_collapsed_key(int64_t n_verts) { return (uint64_t)n_verts << 33; }
// the key bits the sort has to look at, the collapsed key included; n_verts < 2^31 keeps 33 + bits(n_verts) within the 64 bits
// of the key, and the clamp says so to rocPRIM whatever the argument checks admit
inline unsigned ms_key_bits(int64_t n_verts) { return std::min(33u + ms_bits((uint64_t)n_verts), 64u); }

// the buffers of the half-edge table: keys / vals as written, keys2 / vals2 sorted, temp for rocPRIM (a tool's work struct
// derives from this and uses temp for its other sorts and scans too)
struct MsHalfEdgeBufs {
    DevBuf keys, keys2, vals, vals2, temp;
};

// The sorted half-edge table of n > 0 device triangles on `st`: sizes the buffers, launches ms_key_kernel<NPARENT, VFLAG>
// (parent / vflag: the caller's arrays, null where the tool has none) and sorts the pairs by key into keys2 / vals2.  temp is
// sized for the sort and for `extra_temp` bytes, what the caller's scan behind the sort asks for, so that both share one
// allocation.
template <int NPARENT, bool VFLAG>
int ms_sort_half_edges(MsHalfEdgeBufs& b, const int32_t* d_tris, int64_t n, int64_t n_verts, uint32_t* parent, int32_t* vflag,
                       uint64_t* n_collapsed, size_t extra_temp, hipStream_t st)
{
    const size_t nh = 3 * (size_t)n;
    ENSURE(b.keys, sizeof(uint64_t) * nh);
    ENSURE(b.keys2, sizeof(uint64_t) * nh);
    ENSURE(b.vals, sizeof(uint32_t) * nh);
    ENSURE(b.vals2, sizeof(uint32_t) * nh);
    uint64_t *keys = b.keys.as<uint64_t>(), *keys2 = b.keys2.as<uint64_t>();
    uint32_t *vals = b.vals.as<uint32_t>(), *vals2 = b.vals2.as<uint32_t>();
    ms_key_kernel<NPARENT, VFLAG><<<ms_blocks(n), 256, 0, st>>>(d_tris, n, ms_collapsed_key(n_verts), keys, vals, parent, vflag, n_collapsed);
    HIP_TRY(hipGetLastError());
    const unsigned ebits = ms_key_bits(n_verts);
    size_t tb = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, keys, keys2, vals, vals2, nh, 0u, ebits, st));
    ENSURE(b.temp, std::max<size_t>(std::max(tb, extra_temp), 16));
    HIP_TRY(rocprim::radix_sort_pairs(b.temp.p, tb, keys, keys2, vals, vals2, nh, 0u, ebits, st));
    return 0;
}

// The component stage of shells, orient and nesting on `st`, for n > 0 device triangles: sizes parent (NPARENT nodes a triangle),
// rflag, num, group and, with PAIRS, skey / sval; the sorted half-edge table (ms_sort_half_edges<NPARENT, VFLAG>, temp sized for
// the sort and the scan together); the tool's unions over the sorted runs, launch_union(keys2, vals2, nh, ckey, parent); the
// flatten, launch_flatten(parent, rflag): ms_flatten_kernel<true>, or the orient's own, which leaves the roots in `info`; the
// exclusive scan of rflag into num; ms_number_kernel<DOUBLED, PAIRS> reading the roots from info (DOUBLED) or parent.
template <int NPARENT, bool VFLAG, bool DOUBLED, bool PAIRS, class Union, class Flatten>
int ms_group_triangles(MsHalfEdgeBufs& b, const int32_t* d_tris, int64_t n, int64_t n_verts, DevBuf& parent, int32_t* vflag, const uint32_t* info,
                       DevBuf& rflag, DevBuf& num, DevBuf& group, DevBuf* skey, DevBuf* sval, uint64_t* n_collapsed, uint64_t* n_groups,
                       Union launch_union, Flatten launch_flatten, hipStream_t st)
{
    ENSURE(parent, sizeof(uint32_t) * NPARENT * (size_t)n);
    for (DevBuf* per_tri : {&rflag, &num, &group, skey, sval})   // (skey / sval: null without PAIRS)
        if (per_tri) ENSURE(*per_tri, sizeof(int32_t) * (size_t)n);
    uint32_t* root = parent.as<uint32_t>();
    int32_t *flag = rflag.as<int32_t>(), *scan = num.as<int32_t>();
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, flag, scan, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    if (const int rc = ms_sort_half_edges<NPARENT, VFLAG>(b, d_tris, n, n_verts, root, vflag, n_collapsed, scan_bytes, st)) return rc;
    launch_union(b.keys2.as<uint64_t>(), b.vals2.as<uint32_t>(), 3 * n, ms_collapsed_key(n_verts), root);
    HIP_TRY(hipGetLastError());
    launch_flatten(root, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(b.temp.p, scan_bytes, flag, scan, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
    ms_number_kernel<DOUBLED, PAIRS><<<ms_blocks(n), 256, 0, st>>>(d_tris, n, DOUBLED ? info : root, scan, flag, group.as<int32_t>(),
                                                                 PAIRS ? skey->as<uint32_t>() : nullptr, PAIRS ? sval->as<uint32_t>() : nullptr, n_groups);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the segmented Float64 sum ---------------------------------------------------------------------------------------------
constexpr int MS_BLOCK = 256;   // sorted items per block of the Float64 sums (the header's definition)

// seg[s] = the first sorted position of segment s, seg[n_segments] = nvalid; counts[s][0] = the segment's first item
// (rows of STRIDE)
template <int STRIDE>
__global__ void __launch_bounds__(256) ms_segment_kernel(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval, int64_t nvalid,
                                                          int64_t n_segments, int64_t* __restrict__ seg, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvalid) return;
    const uint32_t s = skey[i];
    if (i == 0 || skey[i - 1] != s) {
        seg[s] = i;
        counts[(int64_t)s * STRIDE] = (int64_t)sval[i];
    }
    if (i == 0) seg[n_segments] = nvalid;
}

// Block b holds the sorted positions [256 b, 256 b + 256); `key` is the segment of the thread's item, v its NSUM terms.  A
// segmented fixed tree in LDS (round d = 1, 2, .., 128: an item takes the item d places on while that one is in its
// segment), then the first item of every segment in the block writes the partial of (block b, segment s) to slot b + s (both
// only grow along the sorted order, so the slots are distinct; there are fewer than blocks + segments of them).  Called by
// all 256 threads; v comes back changed.
template <int NSUM>
__device__ inline void ms_block_sum(bool active, uint32_t key, double v[NSUM], double* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double s_v[NSUM][MS_BLOCK];
    __shared__ uint32_t s_key[MS_BLOCK];
    const int j = threadIdx.x;
    if (!active) key = 0xffffffffu;
    s_key[j] = key;
#pragma unroll
    for (int q = 0; q < NSUM; ++q) s_v[q][j] = v[q];
    __syncthreads();
    const bool head = active && (j == 0 || s_key[j - 1] != key);
#pragma unroll
    for (int d = 1; d < MS_BLOCK; d <<= 1) {
        const bool take = active && j + d < MS_BLOCK && s_key[j + d] == key;
        double o[NSUM];
#pragma unroll
        for (int q = 0; q < NSUM; ++q) o[q] = take ? s_v[q][j + d] : 0.0;
        __syncthreads();
        if (take) {
#pragma unroll
            for (int q = 0; q < NSUM; ++q) {
                v[q] = v[q] + o[q];
                s_v[q][j] = v[q];
            }
        }
        __syncthreads();
    }
    if (head) {
        double* out = partial + ((int64_t)blockIdx.x + (int64_t)key) * NSUM;
#pragma unroll
        for (int q = 0; q < NSUM; ++q) out[q] = v[q];
    }
}

// one wavefront per segment [start[s], start[s + 1]): lane l sums the l-th run of `chunk` consecutive block partials in
// ascending block order, then the run sums are joined in a fixed tree (round d = 1, 2, .., 32: lane l takes lane l + d while
// that lane has a run).  n_items (optional): the segment's length goes to n_items[s * item_stride], the count column of shells
// and orient, at no launch of its own.
template <int NSUM>
__global__ void __launch_bounds__(256) ms_combine_kernel(const int64_t* __restrict__ start, int64_t n_segments, const double* __restrict__ partial,
                                                          double* __restrict__ sums, int64_t* __restrict__ n_items, int item_stride)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_segments) return;   // (the whole wavefront)
    const int64_t first = start[s], end = start[s + 1];
    const int64_t b0 = first / MS_BLOCK, nb = (end - 1) / MS_BLOCK - b0 + 1;
    const int64_t chunk = (nb + 63) / 64;
    const int m = (int)((nb + chunk - 1) / chunk);   // lanes with a run: 1 .. 64
    double v[NSUM];
#pragma unroll
    for (int q = 0; q < NSUM; ++q) v[q] = 0.0;
    if (lane < m) {
        const int64_t lo = lane * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
        const double* p = partial + (b0 + lo + s) * NSUM;
#pragma unroll
        for (int q = 0; q < NSUM; ++q) v[q] = p[q];
        for (int64_t b = lo + 1; b < hi; ++b) {
            p += NSUM;
#pragma unroll
            for (int q = 0; q < NSUM; ++q) v[q] = v[q] + p[q];
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int q = 0; q < NSUM; ++q) {
            const double o = __shfl_down(v[q], d, 64);
            if (lane + d < m) v[q] = v[q] + o;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NSUM; ++q) sums[s * NSUM + q] = v[q];
        if (n_items) n_items[s * item_stride] = end - first;
    }
}

// The Float64 table of shells and orient on `st`: the stable radix sort of the pairs ms_number_kernel left (skey = group, sval =
// triangle, n of them, the nvalid real ones in front) into skey2 / sval2, ms_segment_kernel<NCNT>, the tool's terms
// (launch_sum(blocks): its kernel around ms_block_sum<NSUM>, over skey2 / sval2 into partial) and ms_combine_kernel<NSUM> with
// the groups' lengths in column count_col of counts.  temp is sized for the sort and for extra_temp bytes, what the caller runs
// behind this on the same buffer; seg [n_groups + 1], partial [blocks + n_groups][NSUM], sums and counts are the caller's.
template <int NCNT, int NSUM, class Sum>
int ms_sum_by_group(DevBuf& temp, size_t extra_temp, int64_t n, int64_t nvalid, int64_t n_groups, uint32_t* skey, uint32_t* skey2,
                    uint32_t* sval, uint32_t* sval2, int64_t* seg, const double* partial, double* sums, int64_t* counts, int count_col,
                    Sum launch_sum, hipStream_t st)
{
    size_t tb = 0;
    const unsigned sbits = ms_bits((uint64_t)n_groups);
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, skey, skey2, sval, sval2, (size_t)n, 0u, sbits, st));
    ENSURE(temp, std::max<size_t>(std::max(tb, extra_temp), 16));
    HIP_TRY(rocprim::radix_sort_pairs(temp.p, tb, skey, skey2, sval, sval2, (size_t)n, 0u, sbits, st));
    ms_segment_kernel<NCNT><<<ms_blocks(nvalid), 256, 0, st>>>(skey2, sval2, nvalid, n_groups, seg, counts);
    HIP_TRY(hipGetLastError());
    launch_sum((unsigned)((nvalid + MS_BLOCK - 1) / MS_BLOCK));
    HIP_TRY(hipGetLastError());
    ms_combine_kernel<NSUM><<<(unsigned)((n_groups + 3) / 4), 256, 0, st>>>(seg, n_groups, partial, sums, counts + count_col, NCNT);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the loop ordering ------------------------------------------------------------------------------------------------------
// Lays the n items of a graph of chains out group by group (sections: segments by contour, holes: boundary half-edges by rim):
// a closed group, a single cycle along succ, in walking order from its head, every other group in ascending item id.
// (The three kernels without a parameter of their own are templates too, so that only a file that launches them compiles them.)
// The head of a group is its root.  The caller's ms_flatten_kernel<false> left parent = root, and the root is the smallest item of
// the group, so parent[i] == i names the head and nothing else has to say which item it is.

// (distance << 32) | pointer: an item of a closed group points at its successor at distance 1, the head and every item of
// another group at itself at distance 0
template <class OnlyWhereLaunched = void>
__global__ void __launch_bounds__(256) ms_rank_init_kernel(int64_t n, const uint32_t* __restrict__ group_of, const int32_t* __restrict__ closed,
                                                            const uint32_t* __restrict__ parent, const uint32_t* __restrict__ succ,
                                                            uint64_t* __restrict__ pp)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool walks = closed[group_of[i]] && parent[i] != (uint32_t)i;
    pp[i] = walks ? ((1ull << 32) | (uint64_t)succ[i]) : (uint64_t)i;
}

// one round of pointer jumping from `in` to `out`
template <class OnlyWhereLaunched = void>
__global__ void __launch_bounds__(256) ms_jump_kernel(int64_t n, const uint64_t* __restrict__ in, uint64_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = in[i], w = in[(uint32_t)v];
    out[i] = (((v >> 32) + (w >> 32)) << 32) | (uint64_t)(uint32_t)w;
}

// start[g] = the first sorted position of group g, start[n_groups] = n
template <class OnlyWhereLaunched = void>
__global__ void __launch_bounds__(256) ms_start_kernel(const uint32_t* __restrict__ skey, int64_t n, int64_t n_groups, int64_t* __restrict__ start)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = skey[i];
    if (i == 0 || skey[i - 1] != g) start[g] = i;
    if (i == 0) start[n_groups] = n;
}

// the output order: the stable sort left every group in ascending item id; a closed group is laid out by rank instead (rank 0 =
// the head, rank r = length - distance to the head along the successors).  The length of group g is counts[g * STRIDE + COL];
// MAP: what is placed is map[item], not the item.
template <int STRIDE, int COL, bool MAP>
__global__ void __launch_bounds__(256) ms_place_kernel(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval, int64_t n,
                                                        const int32_t* __restrict__ closed, const int64_t* __restrict__ counts,
                                                        const int64_t* __restrict__ start, const uint64_t* __restrict__ pp,
                                                        const uint32_t* __restrict__ map, uint32_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = skey[i], item = sval[i];
    int64_t pos = i;
    if (closed[g]) {
        const int64_t len = counts[(int64_t)g * STRIDE + COL], d = (int64_t)(pp[item] >> 32);
        const int64_t rank = d ? len - d : 0;
        if (rank < 0 || rank >= len) return;   // (cannot happen on a cycle; keeps the store inside the group's range)
        pos = start[g] + rank;
    }
    out[pos] = MAP ? map[item] : item;
}

// The whole stage on `st`: ms_rank_init_kernel, the jump rounds for a longest closed group of `longest` items (2^rounds >=
// longest) over pp0 / pp1, the stable radix sort of (skey = group, sval = item) into skey2 / sval2, out = 0, ms_start_kernel,
// ms_place_kernel.  Every buffer is the caller's; temp holds temp_bytes, what rocprim::radix_sort_pairs of these n pairs over
// ms_bits(n_groups) bits asked for.
template <int STRIDE, int COL, bool MAP>
int ms_order_loops(int64_t n, int64_t n_groups, uint64_t longest, const int32_t* closed, const uint32_t* parent, const uint32_t* succ,
                   const int64_t* counts, uint32_t* skey, uint32_t* skey2, uint32_t* sval, uint32_t* sval2, uint64_t* pp0, uint64_t* pp1,
                   void* temp, size_t temp_bytes, int64_t* start, const uint32_t* map, uint32_t* out, hipStream_t st)
{
    ms_rank_init_kernel<><<<ms_blocks(n), 256, 0, st>>>(n, skey, closed, parent, succ, pp0);
    HIP_TRY(hipGetLastError());
    for (uint64_t reach = 1; reach < longest; reach <<= 1) {
        ms_jump_kernel<><<<ms_blocks(n), 256, 0, st>>>(n, pp0, pp1);
        HIP_TRY(hipGetLastError());
        std::swap(pp0, pp1);
    }
    HIP_TRY(rocprim::radix_sort_pairs(temp, temp_bytes, skey, skey2, sval, sval2, (size_t)n, 0u, ms_bits((uint64_t)n_groups), st));
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(uint32_t) * (size_t)n, st));
    ms_start_kernel<><<<ms_blocks(n), 256, 0, st>>>(skey2, n, n_groups, start);
    HIP_TRY(hipGetLastError());
    ms_place_kernel<STRIDE, COL, MAP><<<ms_blocks(n), 256, 0, st>>>(skey2, sval2, n, closed, counts, start, pp0, map, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace
