// Mesh sections: the contours in which the planes h = c_k cut a triangle mesh, one segment per (triangle, crossed level), the
// node classes, and per contour the integer record and the Float64 length / area vector / first moments
// (include/rho2sdf_hip.h, r2s_mesh_sections; DESIGN.md "Mesh sections").  The shells' machinery one dimension down: the graph
// is on segments, nodes take the place of edges.
//   sx_height_kernel   h(v) per vertex;  ms_bounds_kernel (r2s_mesh_graph.hpp): the box of the vertices -> the reference point
//   sx_tri_kernel      per triangle the range of crossed levels (two binary searches in `levels`) and its three half-edge keys
//                      (ms_half_edge_keys, r2s_mesh_graph.hpp) -> rocPRIM exclusive scan (int64): segment offsets; radix sort
//                      of pairs
//   sx_expand_kernel   per segment its triangle (binary search in the offsets) and level, parent = successor = itself
//   sx_link_kernel     one thread per sorted half-edge with the member before it in the same run: both see the level range of
//                      the EDGE, so for every level in it the segments of the two triangles are united (integer union-find,
//                      min-root) and, in a run of exactly two ends of different kinds, the successor link is written - no
//                      second sort and no key wider than 64 bits
//   ms_flatten_kernel<false> (r2s_mesh_graph.hpp) parent = root, root flags -> scan -> sx_rootkey_kernel: (level << 32) | root of every
//                      root -> radix sort of those keys -> sx_contour_kernel: contour numbers by ascending (level, smallest segment)
//   sx_number_kernel   contour of every segment, n_segs;  sx_node_kernel: the edge runs again, the class of every node
//                      (ms_run_class, r2s_mesh_graph.hpp)
//   sx_closed_kernel   closed flags, the longest closed loop (integer atomicMax), the totals
//   ms_order_loops     (r2s_mesh_graph.hpp) ms_rank_init_kernel / ms_jump_kernel: distance to the head segment by pointer jumping,
//                      ping-pong buffers, ceil(log2(longest closed loop)) rounds -> stable radix sort of the segment ids by contour
//                      -> ms_start_kernel -> ms_place_kernel<8, 2, false>: closed contours are laid out by rank, the others keep
//                      ascending segment id
//   sx_sum_kernel      blocks of 256 output positions: the two points and the 7 terms of every segment -> ms_block_sum<7>
//                      (r2s_mesh_graph.hpp): a segmented fixed tree in LDS, one partial per (block, contour);
//                      ms_combine_kernel<7> (r2s_mesh_graph.hpp): one wavefront per contour
// Integer counts use integer atomics (one per wavefront and contour); no floating-point atomic and no library reduction
// touches the Float64 sums.
// Registers of the gfx950 build (hipcc -O3 -ffp-contract=off, -Rpass-analysis=kernel-resource-usage), VGPRs / scratch bytes:
//   sx_height 8 / 0, sx_tri 28 / 0, sx_expand 13 / 0, sx_link 22 / 0, ms_flatten 12 / 0, sx_rootkey 8 / 0, sx_contour 10 / 0,
//   sx_number 10 / 0, sx_node 22 / 0, sx_closed 23 / 0, ms_rank_init 4 / 0, ms_jump 8 / 0, ms_start 6 / 0,
//   ms_place<8, 2, false> 12 / 0, sx_sum 63 / 0 (15 KiB of LDS), ms_combine<7> 42 / 0, ms_bounds 18 / 0: no kernel uses scratch,
//   all run 8 waves per SIMD.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_graph.hpp"

using namespace r2s_int;

namespace {

constexpr int SX_NSUM = 7, SX_NCNT = 8;
constexpr int64_t SX_MAX_TRIS = (int64_t)1 << 30, SX_MAX_LEVELS = (int64_t)1 << 30, SX_MAX_SEGS = 0x7fffffffll;
// slots of the small device array: [0..5] the bounds, then
constexpr int SX_COLLAPSED = 6, SX_MAXLOOP = 7, SX_TOT = 8;   // [SX_TOT .. SX_TOT + 4]: nodes, open, flipped, branch, closed contours
constexpr int SX_SMALL = 16;

// the number of levels <= x (levels ascending): vertex of height x is above exactly the levels below that index
__device__ inline int32_t sx_upper(const double* __restrict__ levels, int32_t nl, double x)
{
    int32_t lo = 0, hi = nl;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (levels[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) sx_height_kernel(const float* __restrict__ verts, int64_t nverts, double nx, double ny, double nz,
                                                         double* __restrict__ h)
{
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nverts) return;
    h[v] = (nx * (double)verts[3 * v] + ny * (double)verts[3 * v + 1]) + nz * (double)verts[3 * v + 2];
}

// one thread per triangle (and one behind the last: cnt[n] = 0, so that the scan ends with the number of segments): the first
// crossed level and the number of crossed levels, the three half-edge keys, the collapsed count
__global__ void __launch_bounds__(256) sx_tri_kernel(const int32_t* __restrict__ tris, int64_t n, const double* __restrict__ h,
                                                      const double* __restrict__ levels, int32_t nl, uint64_t ckey, int32_t* __restrict__ first,
                                                      int64_t* __restrict__ cnt, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                      uint64_t* __restrict__ small)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool col = false;
    if (t == n) cnt[n] = 0;
    if (t < n) {
        int32_t i[3];
        col = ms_half_edge_keys(tris, t, ckey, keys, vals, i);
        int32_t f = 0, e = 0;
        if (!col) {
            const double h0 = h[i[0]], h1 = h[i[1]], h2 = h[i[2]];
            double lo = h0 < h1 ? h0 : h1, hi = h0 < h1 ? h1 : h0;
            lo = h2 < lo ? h2 : lo;
            hi = h2 > hi ? h2 : hi;
            f = sx_upper(levels, nl, lo);
            e = sx_upper(levels, nl, hi);
        }
        first[t] = f;
        cnt[t] = (int64_t)(e - f);
    }
    ms_count_collapsed(col, &small[SX_COLLAPSED]);
}

// one thread per segment: its triangle is the last one whose offset is <= s (a triangle without segments shares its offset
// with the next one)
__global__ void __launch_bounds__(256) sx_expand_kernel(const int64_t* __restrict__ offset, int64_t n, const int32_t* __restrict__ first,
                                                         int64_t nseg, int32_t* __restrict__ tri_of, int32_t* __restrict__ level_of,
                                                         uint32_t* __restrict__ parent, uint32_t* __restrict__ succ)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    int64_t lo = 0, hi = n;   // the first t in [0, n] with offset[t] > s
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (offset[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    const int64_t t = lo - 1;
    tri_of[s] = (int32_t)t;
    level_of[s] = first[t] + (int32_t)(s - offset[t]);
    parent[s] = (uint32_t)s;
    succ[s] = (uint32_t)s;
}

// the levels an edge crosses, [e0, e1), from the heights of its two ends; a_above: the end with the smaller index is the
// upper one (it is then above every level of the range, the other end below)
__device__ inline void sx_edge_range(uint64_t key, const double* __restrict__ h, const double* __restrict__ levels, int32_t nl, int32_t& e0,
                                     int32_t& e1, bool& a_above)
{
    const double ha = h[key >> 33], hb = h[(key >> 1) & 0xffffffffull];
    a_above = ha > hb;
    e0 = sx_upper(levels, nl, a_above ? hb : ha);
    e1 = sx_upper(levels, nl, a_above ? ha : hb);
}

// one thread per sorted half-edge that has the member before it in the same run
__global__ void __launch_bounds__(256) sx_link_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, const double* __restrict__ h, const double* __restrict__ levels, int32_t nl,
                                                       const int64_t* __restrict__ offset, const int32_t* __restrict__ first, uint32_t* parent,
                                                       uint32_t* __restrict__ succ)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= nh) return;
    const uint64_t k = keys[i], kp = keys[i - 1];
    if (k >= ckey || (kp >> 1) != (k >> 1)) return;
    int32_t e0, e1;
    bool a_above;
    sx_edge_range(k, h, levels, nl, e0, e1, a_above);
    if (e0 >= e1) return;
    const uint32_t t0 = vals[i - 1] / 3u, t1 = vals[i] / 3u;
    const uint32_t s0 = (uint32_t)(offset[t0] + (e0 - first[t0])), s1 = (uint32_t)(offset[t1] + (e0 - first[t1]));
    const bool exactly_two = (i < 2 || (keys[i - 2] >> 1) != (k >> 1)) && (i + 1 >= nh || (keys[i + 1] >> 1) != (k >> 1));
    // a half-edge that runs from the upper end to the lower one carries the segment's FROM node (an outgoing end)
    const bool out0 = ((kp & 1ull) == 0ull) == a_above, out1 = ((k & 1ull) == 0ull) == a_above;
    const bool regular = exactly_two && out0 != out1;
    for (uint32_t j = 0; j < (uint32_t)(e1 - e0); ++j) {
        ms_union(parent, s0 + j, s1 + j);
        if (regular) succ[out0 ? s1 + j : s0 + j] = out0 ? s0 + j : s1 + j;   // the incoming end's segment is followed by the outgoing one's
    }
}

// num = the exclusive scan of flag: the sort key of root number num[s]
__global__ void __launch_bounds__(256) sx_rootkey_kernel(int64_t nseg, const int32_t* __restrict__ flag, const int32_t* __restrict__ num,
                                                          const int32_t* __restrict__ level_of, uint64_t* __restrict__ rkeys)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg || !flag[s]) return;
    rkeys[num[s]] = ((uint64_t)(uint32_t)level_of[s] << 32) | (uint64_t)s;
}

// the sorted root keys: contour c has level key >> 32 and the smallest segment (uint32)key; num[root] becomes c
__global__ void __launch_bounds__(256) sx_contour_kernel(const uint64_t* __restrict__ rkeys, int64_t nc, int32_t* __restrict__ num,
                                                          int64_t* __restrict__ counts)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    const uint64_t k = rkeys[c];
    num[(uint32_t)k] = (int32_t)c;
    counts[c * SX_NCNT] = (int64_t)(k >> 32);
    counts[c * SX_NCNT + 1] = (int64_t)(uint32_t)k;
}

// adds 1 to counts[contour][col0 + k] for every k < NC with add[k] set, over the wavefront's active lanes: one atomic per
// column and distinct contour.  Called by all 64 lanes.
template <int NC>
__device__ inline void sx_count(bool active, uint32_t contour, const bool add[NC], int col0, int64_t* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t c0 = (uint32_t)__shfl((int)contour, leader, 64);
        const bool mine = active && contour == c0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const unsigned long long m = __ballot(mine && add[k]);
            if (lane == leader && m) atomicAdd((unsigned long long*)&counts[(int64_t)c0 * SX_NCNT + col0 + k], (unsigned long long)__popcll(m));
        }
        todo &= ~__ballot(mine);
    }
}

__global__ void __launch_bounds__(256) sx_number_kernel(int64_t nseg, const uint32_t* __restrict__ parent, const int32_t* __restrict__ num,
                                                         uint32_t* __restrict__ skey, uint32_t* __restrict__ sval, int64_t* __restrict__ counts)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = s < nseg;
    uint32_t c = 0;
    if (active) {
        c = (uint32_t)num[parent[s]];   // (ms_flatten_kernel left parent = root)
        skey[s] = c;
        sval[s] = (uint32_t)s;
    }
    const bool add[1] = {true};
    sx_count<1>(active, c, add, 2, counts);
}

// one thread per sorted half-edge; the first member of a run classifies the nodes of its edge, one per level of the range, and
// counts each into the contour of its own segment at that level
__global__ void __launch_bounds__(256) sx_node_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, const double* __restrict__ h, const double* __restrict__ levels, int32_t nl,
                                                       const int64_t* __restrict__ offset, const int32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ skey, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t len = 0, s0 = 0;
    bool add[4] = {true, false, false, false};   // node, open, flipped, branch
    if (i < nh) {
        const uint64_t k = keys[i];
        if (k < ckey && (i == 0 || (keys[i - 1] >> 1) != (k >> 1))) {
            int32_t e0, e1;
            bool a_above;
            sx_edge_range(k, h, levels, nl, e0, e1, a_above);
            if (e0 < e1) {
                const int cls = ms_run_class(keys, i, nh);
                add[1] = cls == MS_RUN_SINGLE;
                add[2] = cls == MS_RUN_SAME;   // the same direction along one edge: two ends of one kind
                add[3] = cls == MS_RUN_MANY;
                const uint32_t t = vals[i] / 3u;
                len = (uint32_t)(e1 - e0);
                s0 = (uint32_t)(offset[t] + (e0 - first[t]));
            }
        }
    }
    for (uint32_t j = 0; __ballot(j < len); ++j) {
        const bool active = j < len;
        sx_count<4>(active, active ? skey[s0 + j] : 0u, add, 3, counts);
    }
}

__global__ void __launch_bounds__(256) sx_closed_kernel(const int64_t* __restrict__ counts, int64_t nc, int32_t* __restrict__ closed,
                                                         uint64_t* __restrict__ small)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    long long v[5] = {0, 0, 0, 0, 0};
    long long loop = 0;
    if (c < nc) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = counts[c * SX_NCNT + 3 + k];
        const bool cl = v[1] == 0 && v[2] == 0 && v[3] == 0;
        closed[c] = cl ? 1 : 0;
        v[4] = cl ? 1 : 0;
        loop = cl ? counts[c * SX_NCNT + 2] : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(loop, d, 64);
        loop = o > loop ? o : loop;
    }
    if ((threadIdx.x & 63) == 0 && loop) atomicMax((unsigned long long*)&small[SX_MAXLOOP], (unsigned long long)loop);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd((unsigned long long*)&small[SX_TOT + k], (unsigned long long)v[k]);
    }
}

// the point of the node on the edge between corners u and w of a triangle at level ck, taken from the smaller vertex index
__device__ inline void sx_node_point(int32_t iu, int32_t iw, double hu, double hw, const double Xu[3], const double Xw[3], double ck, double p[3])
{
#pragma clang fp contract(off)
    const bool sw = iu > iw;
    const double hi = sw ? hw : hu, hj = sw ? hu : hw;
    const double t = (ck - hi) / (hj - hi);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double xi = sw ? Xw[a] : Xu[a], xj = sw ? Xu[a] : Xw[a];
        p[a] = xi + t * (xj - xi);
    }
}

// one thread per output position: the two points of its segment, and its 7 terms into the segmented sum of its block
// (ms_block_sum: slot block + contour)
__global__ void __launch_bounds__(MS_BLOCK) sx_sum_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           const double* __restrict__ h, const double* __restrict__ levels,
                                                           const uint32_t* __restrict__ skey, const uint32_t* __restrict__ order,
                                                           const int32_t* __restrict__ tri_of, const int32_t* __restrict__ level_of, int64_t nseg,
                                                           double nx, double ny, double nz, double rx, double ry, double rz,
                                                           int32_t* __restrict__ seg_tri, double* __restrict__ points, double* __restrict__ partial)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    const bool active = i < nseg;
    uint32_t key = 0xffffffffu;
    double v[SX_NSUM];
#pragma unroll
    for (int q = 0; q < SX_NSUM; ++q) v[q] = 0.0;
    if (active) {
        key = skey[i];
        const uint32_t s = order[i];
        const int64_t t = (int64_t)tri_of[s];
        const double ck = levels[level_of[s]];
        int32_t id[3];
        double hh[3], X[3][3];
        bool above[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            id[c] = tris[3 * t + c];
            hh[c] = h[id[c]];
            above[c] = hh[c] >= ck;
#pragma unroll
            for (int a = 0; a < 3; ++a) X[c][a] = (double)verts[3 * (int64_t)id[c] + a];
        }
        double from[3] = {0.0, 0.0, 0.0}, to[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int w = c == 2 ? 0 : c + 1;
            double p[3];
            sx_node_point(id[c], id[w], hh[c], hh[w], X[c], X[w], ck, p);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                from[a] = above[c] && !above[w] ? p[a] : from[a];
                to[a] = !above[c] && above[w] ? p[a] : to[a];
            }
        }
        seg_tri[i] = (int32_t)t;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            points[6 * i + a] = from[a];
            points[6 * i + 3 + a] = to[a];
        }
        const double Ax = from[0] - rx, Ay = from[1] - ry, Az = from[2] - rz;
        const double Bx = to[0] - rx, By = to[1] - ry, Bz = to[2] - rz;
        const double Dx = Bx - Ax, Dy = By - Ay, Dz = Bz - Az;
        const double Cx = Ay * Bz - Az * By, Cy = Az * Bx - Ax * Bz, Cz = Ax * By - Ay * Bx;
        const double w = (nx * Cx + ny * Cy) + nz * Cz;
        v[0] = sqrt((Dx * Dx + Dy * Dy) + Dz * Dz);
        v[1] = Cx, v[2] = Cy, v[3] = Cz;
        v[4] = w * (Ax + Bx);
        v[5] = w * (Ay + By);
        v[6] = w * (Az + Bz);
    }
    ms_block_sum<SX_NSUM>(active, key, v, partial);
}

// work buffers of the section calls, kept per device between calls (r2s_release_cache frees them)
struct SectionWork : MsHalfEdgeBufs {
    DevBuf verts, tris, flag, small, levels, h, first, cnt, offset, tri_of, level_of, parent, succ, rflag, num, rkeys, rkeys2, skey, skey2,
        sval, sval2, pp0, pp1, closed, start, order, partial, counts, sums, seg_tri, points;
};
PerDevice<SectionWork> g_section_work;

struct SectionTables {
    std::vector<int64_t> start;    // [n_contours + 1] (empty without contours)
    std::vector<int64_t> counts;   // [n_contours][8]
    std::vector<double> sums;      // [n_contours][7]
    std::vector<int32_t> seg_tri;  // [n_segments]
    std::vector<double> points;    // [n_segments][2][3]
};
thread_local SectionTables g_last_sections;

// The sections of the device mesh on the current device, after the work queued on `st`; synchronous.  Leaves the tables in
// w.start [n_contours + 1], w.counts / w.sums [n_contours] and w.seg_tri / w.points [n_segments]; the scalars go to the host
// pointers.
int sections_core(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, const double nrm[3], const double* h_levels,
                  int64_t n_levels, hipStream_t st, SectionWork& w, int64_t* n_contours, int64_t* n_segments, double ref_point[3],
                  int64_t totals[8])
{
    uint64_t h_small[SX_SMALL];
    if (const int rc = ms_begin_small(w.small, h_small, d_verts, n_verts, st)) return rc;
    uint64_t* small = w.small.as<uint64_t>();
    const int64_t nh = 3 * n;
    const int32_t nl = (int32_t)n_levels;
    const uint64_t ckey = ms_collapsed_key(n_verts);
    int64_t nseg = 0;
    if (n > 0) {
        ENSURE(w.levels, sizeof(double) * (size_t)std::max<int64_t>(n_levels, 1));
        ENSURE(w.h, sizeof(double) * (size_t)std::max<int64_t>(n_verts, 1));
        ENSURE(w.first, sizeof(int32_t) * (size_t)n);
        ENSURE(w.cnt, sizeof(int64_t) * (size_t)(n + 1));
        ENSURE(w.offset, sizeof(int64_t) * (size_t)(n + 1));
        ENSURE(w.keys, sizeof(uint64_t) * (size_t)nh);
        ENSURE(w.keys2, sizeof(uint64_t) * (size_t)nh);
        ENSURE(w.vals, sizeof(uint32_t) * (size_t)nh);
        ENSURE(w.vals2, sizeof(uint32_t) * (size_t)nh);
        if (n_levels > 0) HIP_TRY(hipMemcpyAsync(w.levels.p, h_levels, sizeof(double) * (size_t)n_levels, hipMemcpyHostToDevice, st));
        if (n_verts > 0) {
            sx_height_kernel<<<ms_blocks(n_verts), 256, 0, st>>>(d_verts, n_verts, nrm[0], nrm[1], nrm[2], w.h.as<double>());
            HIP_TRY(hipGetLastError());
        }
        sx_tri_kernel<<<ms_blocks(n + 1), 256, 0, st>>>(d_tris, n, w.h.as<double>(), w.levels.as<double>(), nl, ckey, w.first.as<int32_t>(),
                                                      w.cnt.as<int64_t>(), w.keys.as<uint64_t>(), w.vals.as<uint32_t>(), small);
        HIP_TRY(hipGetLastError());
        size_t tb = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, tb, w.cnt.as<int64_t>(), w.offset.as<int64_t>(), (int64_t)0, (size_t)(n + 1),
                                        rocprim::plus<int64_t>(), st));
        ENSURE(w.temp, std::max<size_t>(tb, 16));
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, tb, w.cnt.as<int64_t>(), w.offset.as<int64_t>(), (int64_t)0, (size_t)(n + 1),
                                        rocprim::plus<int64_t>(), st));
        HIP_TRY(hipMemcpyAsync(&nseg, w.offset.as<int64_t>() + n, sizeof nseg, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nseg > SX_MAX_SEGS) return fail(R2S_ERR_UNSUPPORTED, "mesh_sections: %lld segments exceed 2^31 - 1", (long long)nseg);
    double* r = ref_point;
    ms_ref_point(h_small, n_verts, r);
    const int64_t ncol = (int64_t)h_small[SX_COLLAPSED];
    int64_t nc = 0;
    if (nseg > 0) {
        const double *h = w.h.as<double>(), *levels = w.levels.as<double>();
        const int64_t* offset = w.offset.as<int64_t>();
        const int32_t* first = w.first.as<int32_t>();
        ENSURE(w.tri_of, sizeof(int32_t) * (size_t)nseg);
        ENSURE(w.level_of, sizeof(int32_t) * (size_t)nseg);
        ENSURE(w.parent, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.succ, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.rflag, sizeof(int32_t) * (size_t)nseg);
        ENSURE(w.num, sizeof(int32_t) * (size_t)nseg);
        ENSURE(w.skey, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.skey2, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.sval, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.sval2, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.pp0, sizeof(uint64_t) * (size_t)nseg);
        ENSURE(w.pp1, sizeof(uint64_t) * (size_t)nseg);
        ENSURE(w.order, sizeof(uint32_t) * (size_t)nseg);
        ENSURE(w.seg_tri, sizeof(int32_t) * (size_t)nseg);
        ENSURE(w.points, sizeof(double) * 6 * (size_t)nseg);
        uint64_t *keys = w.keys.as<uint64_t>(), *keys2 = w.keys2.as<uint64_t>();
        uint32_t *vals = w.vals.as<uint32_t>(), *vals2 = w.vals2.as<uint32_t>(), *parent = w.parent.as<uint32_t>(), *succ = w.succ.as<uint32_t>();
        int32_t *rflag = w.rflag.as<int32_t>(), *num = w.num.as<int32_t>();
        const unsigned ebits = ms_key_bits(n_verts);
        size_t tb = 0, tb2 = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, keys, keys2, vals, vals2, (size_t)nh, 0u, ebits, st));
        HIP_TRY(rocprim::exclusive_scan(nullptr, tb2, rflag, num, (int32_t)0, (size_t)nseg, rocprim::plus<int32_t>(), st));
        ENSURE(w.temp, std::max<size_t>(std::max(tb, tb2), 16));
        sx_expand_kernel<<<ms_blocks(nseg), 256, 0, st>>>(offset, n, first, nseg, w.tri_of.as<int32_t>(), w.level_of.as<int32_t>(), parent, succ);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_pairs(w.temp.p, tb, keys, keys2, vals, vals2, (size_t)nh, 0u, ebits, st));
        sx_link_kernel<<<ms_blocks(nh), 256, 0, st>>>(keys2, vals2, nh, ckey, h, levels, nl, offset, first, parent, succ);
        HIP_TRY(hipGetLastError());
        ms_flatten_kernel<false><<<ms_blocks(nseg), 256, 0, st>>>(nullptr, nseg, parent, rflag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, tb2, rflag, num, (int32_t)0, (size_t)nseg, rocprim::plus<int32_t>(), st));
        int32_t last[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&last[0], num + (nseg - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&last[1], rflag + (nseg - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        nc = (int64_t)last[0] + last[1];

        const int64_t nblk = (nseg + MS_BLOCK - 1) / MS_BLOCK;
        ENSURE(w.rkeys, sizeof(uint64_t) * (size_t)nc);
        ENSURE(w.rkeys2, sizeof(uint64_t) * (size_t)nc);
        ENSURE(w.closed, sizeof(int32_t) * (size_t)nc);
        ENSURE(w.start, sizeof(int64_t) * (size_t)(nc + 1));
        ENSURE(w.partial, sizeof(double) * SX_NSUM * (size_t)(nblk + nc));
        ENSURE(w.counts, sizeof(int64_t) * SX_NCNT * (size_t)nc);
        ENSURE(w.sums, sizeof(double) * SX_NSUM * (size_t)nc);
        int64_t* counts = w.counts.as<int64_t>();
        uint32_t *skey = w.skey.as<uint32_t>(), *skey2 = w.skey2.as<uint32_t>(), *sval = w.sval.as<uint32_t>(), *sval2 = w.sval2.as<uint32_t>();
        const unsigned rbits = 32u + ms_bits((uint64_t)std::max<int64_t>(n_levels, 1)), sbits = ms_bits((uint64_t)nc);
        HIP_TRY(rocprim::radix_sort_keys(nullptr, tb, w.rkeys.as<uint64_t>(), w.rkeys2.as<uint64_t>(), (size_t)nc, 0u, rbits, st));
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb2, skey, skey2, sval, sval2, (size_t)nseg, 0u, sbits, st));
        ENSURE(w.temp, std::max<size_t>(std::max(tb, tb2), 16));
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * SX_NCNT * (size_t)nc, st));
        sx_rootkey_kernel<<<ms_blocks(nseg), 256, 0, st>>>(nseg, rflag, num, w.level_of.as<int32_t>(), w.rkeys.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_keys(w.temp.p, tb, w.rkeys.as<uint64_t>(), w.rkeys2.as<uint64_t>(), (size_t)nc, 0u, rbits, st));
        sx_contour_kernel<<<ms_blocks(nc), 256, 0, st>>>(w.rkeys2.as<uint64_t>(), nc, num, counts);
        HIP_TRY(hipGetLastError());
        sx_number_kernel<<<ms_blocks(nseg), 256, 0, st>>>(nseg, parent, num, skey, sval, counts);
        HIP_TRY(hipGetLastError());
        // (keys2 / vals2 still hold the sorted half-edges)
        sx_node_kernel<<<ms_blocks(nh), 256, 0, st>>>(keys2, vals2, nh, ckey, h, levels, nl, offset, first, skey, counts);
        HIP_TRY(hipGetLastError());
        sx_closed_kernel<<<ms_blocks(nc), 256, 0, st>>>(counts, nc, w.closed.as<int32_t>(), small);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // the round count comes from the longest closed loop the device found
        if (const int rc = ms_order_loops<SX_NCNT, 2, false>(nseg, nc, h_small[SX_MAXLOOP], w.closed.as<int32_t>(), parent, succ, counts, skey,
                                                             skey2, sval, sval2, w.pp0.as<uint64_t>(), w.pp1.as<uint64_t>(), w.temp.p, tb2,
                                                             w.start.as<int64_t>(), nullptr, w.order.as<uint32_t>(), st))
            return rc;
        sx_sum_kernel<<<(unsigned)nblk, MS_BLOCK, 0, st>>>(d_verts, d_tris, h, levels, skey2, w.order.as<uint32_t>(), w.tri_of.as<int32_t>(),
                                                          w.level_of.as<int32_t>(), nseg, nrm[0], nrm[1], nrm[2], r[0], r[1], r[2],
                                                          w.seg_tri.as<int32_t>(), w.points.as<double>(), w.partial.as<double>());
        HIP_TRY(hipGetLastError());
        ms_combine_kernel<SX_NSUM><<<(unsigned)((nc + 3) / 4), 256, 0, st>>>(w.start.as<int64_t>(), nc, w.partial.as<double>(), w.sums.as<double>(),
                                                                          nullptr, 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_contours = nc, *n_segments = nseg;
    totals[0] = nc, totals[1] = nseg, totals[2] = ncol;
    for (int k = 0; k < 5; ++k) totals[3 + k] = nseg > 0 ? (int64_t)h_small[SX_TOT + k] : 0;
    return 0;
}

int sections_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, const double* normal, const double* levels,
                  int64_t n_levels, const int64_t* n_contours, const int64_t* n_segments, const double* ref_point, const int64_t* totals)
{
    const int rc = mesh_args("mesh_sections", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (n_tris > SX_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_sections: %lld triangles exceed 2^30", (long long)n_tris);
    if (!n_contours || !n_segments || !ref_point || !totals)
        return fail(R2S_ERR_ARG, "mesh_sections: null n_contours / n_segments / ref_point / totals");
    if (!normal || n_levels < 0 || (n_levels > 0 && !levels)) return fail(R2S_ERR_ARG, "mesh_sections: null normal / levels or a negative n_levels");
    if (n_levels > SX_MAX_LEVELS) return fail(R2S_ERR_UNSUPPORTED, "mesh_sections: %lld levels exceed 2^30", (long long)n_levels);
    bool zero = true;
    for (int k = 0; k < 3; ++k) {
        // (2^500 times the largest float32 cannot overflow: every height is finite)
        if (!std::isfinite(normal[k]) || std::fabs(normal[k]) > 0x1p500)
            return fail(R2S_ERR_ARG, "mesh_sections: the normal must be finite, with components of at most 2^500");
        zero = zero && normal[k] == 0.0;
    }
    if (zero) return fail(R2S_ERR_ARG, "mesh_sections: the normal is zero");
    for (int64_t k = 0; k < n_levels; ++k)
        if (!std::isfinite(levels[k]) || (k > 0 && !(levels[k - 1] < levels[k])))
            return fail(R2S_ERR_ARG, "mesh_sections: levels must be finite and strictly ascending (level %lld)", (long long)k);
    return 0;
}

int table_args(const void* start, const void* counts, const void* sums, int64_t contour_capacity, const void* seg_tri, const void* points,
               int64_t segment_capacity)
{
    if (contour_capacity < 0 || segment_capacity < 0 || (contour_capacity > 0 && (!start || !counts || !sums)) ||
        (segment_capacity > 0 && (!seg_tri || !points)))
        return fail(R2S_ERR_ARG, "mesh_sections: null tables or a negative capacity");
    return 0;
}

// where a device caller wants the tables and the room it has for them (a host caller: none)
struct SectionDevTables {
    int64_t *start = nullptr, *counts = nullptr;
    double* sums = nullptr;
    int64_t contour_capacity = 0;
    int32_t* seg_tri = nullptr;
    double* points = nullptr;
    int64_t segment_capacity = 0;
};

// One call for both kinds of caller: the core, then the five tables and the scalars.  A host caller's tables are kept whole for
// r2s_last_mesh_sections; a device caller gets them when both capacities hold everything, else none.
int sections_run(MeshCall<SectionWork>& c, int64_t n_verts, int64_t n_tris, const double normal[3], const double* levels, int64_t n_levels,
                 const SectionDevTables& d, int64_t* n_contours, int64_t* n_segments, double ref_point[3], int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    SectionWork& w = c.work();
    SectionTables tab;
    int64_t nc = 0, nseg = 0, tot[8];
    double r[3];
    if ((rc = sections_core(c.d_verts(), n_verts, c.d_tris(), n_tris, normal, levels, n_levels, c.stream(), w, &nc, &nseg, r, tot))) return rc;
    const size_t n = (size_t)nc, m = nc ? (size_t)nseg : 0;
    const bool fits = d.contour_capacity >= nc && d.segment_capacity >= nseg;
    if ((rc = c.table(tab.start, d.start, fits, w.start, n ? n + 1 : 0)) || (rc = c.table(tab.counts, d.counts, fits, w.counts, n * SX_NCNT)) ||
        (rc = c.table(tab.sums, d.sums, fits, w.sums, n * SX_NSUM)) || (rc = c.table(tab.seg_tri, d.seg_tri, fits, w.seg_tri, m)) ||
        (rc = c.table(tab.points, d.points, fits, w.points, m * 6)) || (rc = c.finish()))
        return rc;
    if (c.is_host()) g_last_sections = std::move(tab);
    *n_contours = nc;
    *n_segments = nseg;
    std::memcpy(ref_point, r, sizeof r);
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_sections(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const double normal[3], const double* levels,
                      int64_t n_levels, int32_t device, int64_t* n_contours, int64_t* n_segments, double ref_point[3], int64_t totals[8])
{
    if (const int rc = sections_args(verts, n_verts, tris, n_tris, normal, levels, n_levels, n_contours, n_segments, ref_point, totals)) return rc;
    MeshCall<SectionWork> call("mesh_sections", g_section_work, verts, n_verts, tris, n_tris, device);
    return sections_run(call, n_verts, n_tris, normal, levels, n_levels, {}, n_contours, n_segments, ref_point, totals);
}

int r2s_last_mesh_sections(int64_t* contour_start_out, int64_t* counts_out, double* sums_out, int64_t contour_capacity, int32_t* seg_tri_out,
                           double* seg_points_out, int64_t segment_capacity, int64_t* n_contours, int64_t* n_segments)
{
    if (!n_contours || !n_segments) return fail(R2S_ERR_ARG, "last_mesh_sections: null n_contours / n_segments");
    const int rc = table_args(contour_start_out, counts_out, sums_out, contour_capacity, seg_tri_out, seg_points_out, segment_capacity);
    if (rc) return rc;
    const SectionTables& t = g_last_sections;
    const int64_t nc = *n_contours = (int64_t)(t.counts.size() / SX_NCNT), nseg = *n_segments = (int64_t)t.seg_tri.size();
    const int64_t mc = copy_rows(counts_out, t.counts, SX_NCNT, contour_capacity, nc);
    copy_rows(sums_out, t.sums, SX_NSUM, contour_capacity, nc);
    if (mc > 0) copy_rows(contour_start_out, t.start, 1, mc + 1, nc + 1);   // (the end of the last contour copied with it)
    copy_rows(seg_tri_out, t.seg_tri, 1, segment_capacity, nseg);
    copy_rows(seg_points_out, t.points, 6, segment_capacity, nseg);
    return 0;
}

int r2s_mesh_sections_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, const double normal[3],
                          const double* levels, int64_t n_levels, int64_t* d_contour_start, int64_t* d_counts, double* d_sums,
                          int64_t contour_capacity, int32_t* d_seg_tri, double* d_seg_points, int64_t segment_capacity, int64_t* n_contours,
                          int64_t* n_segments, double ref_point[3], int64_t totals[8], void* stream)
{
    int rc = sections_args(d_verts, n_verts, d_tris, n_tris, normal, levels, n_levels, n_contours, n_segments, ref_point, totals);
    if (rc || (rc = table_args(d_contour_start, d_counts, d_sums, contour_capacity, d_seg_tri, d_seg_points, segment_capacity))) return rc;
    MeshCall<SectionWork> call("mesh_sections", g_section_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return sections_run(call, n_verts, n_tris, normal, levels, n_levels,
                        {d_contour_start, d_counts, d_sums, contour_capacity, d_seg_tri, d_seg_points, segment_capacity}, n_contours, n_segments,
                        ref_point, totals);
}

}  // extern "C"
