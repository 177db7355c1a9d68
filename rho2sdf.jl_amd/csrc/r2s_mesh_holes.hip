// Mesh holes: the rims of a triangle mesh (its boundary loops and chains), per rim the integer record and the Float64 length /
// area vector / vertex sum, and the fill that caps every selected closed rim (include/rho2sdf_hip.h, r2s_mesh_holes; DESIGN.md
// "Mesh holes").  The sections' machinery on the boundary half-edges: the graph is on half-edges, the nodes are vertices.
//   ms_sort_half_edges (r2s_mesh_graph.hpp) ms_key_kernel<0, false>: one half-edge key per corner, the shells' keys, payload
//                      3t + c -> rocPRIM radix sort of pairs
//   mh_flag_kernel     a run of size one (ms_run_size) is a boundary half-edge: the flag goes to its half-edge id
//   -> rocPRIM exclusive scan -> mh_compact_kernel: the boundary half-edges b = 0 .. n_b - 1 in ascending half-edge id
//   mh_end_kernel      the two ends of every boundary half-edge, keyed by vertex (end 2b: FROM, outgoing; end 2b + 1: TO, incoming);
//                      parent = successor = itself -> stable radix sort of the ends by vertex: a run is a node
//   mh_link_kernel     every member of a run joins the member before it (the shells' union-find: the larger root under the smaller,
//                      so a rim's root is its first half-edge); the head of a regular run writes the successor
//   ms_flatten_kernel<false> (r2s_mesh_graph.hpp) parent = root, root flags -> scan: the roots in ascending half-edge id are the rim numbers
//   mh_number_kernel   rim of every half-edge, first half-edge and n_edges of every rim;  mh_node_kernel: the runs again, the class
//                      of every node counted into its rim
//   mh_closed_kernel   closed flags, the longest closed rim (integer atomicMax), the totals, what the fill adds per rim
//   -> two exclusive scans (added vertices, added triangles) -> mh_fill_kernel: status and added vertex of every rim
//   ms_order_loops     (r2s_mesh_graph.hpp) ms_rank_init_kernel / ms_jump_kernel: distance to the first half-edge by pointer
//                      jumping, ping-pong buffers, ceil(log2(longest closed rim)) rounds -> stable radix sort of the half-edges by
//                      rim -> ms_start_kernel -> ms_place_kernel<8, 1, true>: closed rims are laid out by rank, the others keep
//                      ascending half-edge id; what is placed is the half-edge id bh[b]
//   mh_sum_kernel      blocks of 256 output positions, the 7 terms of every half-edge -> ms_block_sum<7> (r2s_mesh_graph.hpp): a
//                      segmented fixed tree in LDS, one partial per (block, rim);  ms_combine_kernel<7> (r2s_mesh_graph.hpp): one
//                      wavefront per rim
//   mh_apply_*         the fill: the added vertices and the added triangles (the input mesh is copied by the copy engine)
// Integer counts use integer atomics; no floating-point atomic and no library reduction touches the Float64 sums.
// Registers of the gfx950 build (hipcc -O3 -ffp-contract=off, -Rpass-analysis=kernel-resource-usage) are listed in DESIGN.md:
// no kernel uses scratch.
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

constexpr int MH_NSUM = 7, MH_NCNT = 8;
constexpr int64_t MH_MAX_TRIS = (((int64_t)1 << 31) - 1) / 3;   // 3 n_tris < 2^31: half-edge ids are int32
// slots of the small device array: [0..5] the bounds, then
constexpr int MH_COLLAPSED = 6, MH_NB = 7, MH_NRIMS = 8, MH_MAXLOOP = 9, MH_NODES = 10, MH_IRREGULAR = 11, MH_CLOSED = 12, MH_FILLED = 13,
              MH_ADDT = 14, MH_ADDV = 15;
constexpr int MH_SMALL = 16;
// columns of the per-rim record
constexpr int MH_FIRST = 0, MH_NEDGES = 1, MH_NNODES = 2, MH_STATUS = 6, MH_ADDED = 7;

// one thread per sorted half-edge: bflag[its id] = it is alone in its edge run (every id is written once)
__global__ void __launch_bounds__(256) mh_flag_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, int32_t* __restrict__ bflag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nh) return;
    bool head = false;
    bflag[vals[i]] = (keys[i] < ckey && ms_run_size(keys, i, nh, head) == 1) ? 1 : 0;
}

// bpos = the exclusive scan of bflag: the boundary half-edges in ascending id; n_b
__global__ void __launch_bounds__(256) mh_compact_kernel(int64_t nh, const int32_t* __restrict__ bflag, const int32_t* __restrict__ bpos,
                                                          uint32_t* __restrict__ bh, uint64_t* __restrict__ small)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= nh) return;
    const int32_t f = bflag[h], p = bpos[h];
    if (f) bh[p] = (uint32_t)h;
    if (h == nh - 1) small[MH_NB] = (uint64_t)(p + f);
}

// the vertices half-edge h runs from and to
__device__ inline void mh_from_to(const int32_t* __restrict__ tris, uint32_t h, int32_t& from, int32_t& to)
{
    from = tris[h];
    to = tris[h % 3u == 2u ? h - 2u : h + 1u];
}

// one thread per boundary half-edge b: its two ends keyed by vertex, parent[b] = succ[b] = b
__global__ void __launch_bounds__(256) mh_end_kernel(const int32_t* __restrict__ tris, const uint32_t* __restrict__ bh, int64_t nb,
                                                      uint32_t* __restrict__ ekey, uint32_t* __restrict__ eval, uint32_t* __restrict__ parent,
                                                      uint32_t* __restrict__ succ)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    int32_t from, to;
    mh_from_to(tris, bh[b], from, to);
    ekey[2 * b] = (uint32_t)from, eval[2 * b] = (uint32_t)(2 * b);
    ekey[2 * b + 1] = (uint32_t)to, eval[2 * b + 1] = (uint32_t)(2 * b + 1);
    parent[b] = (uint32_t)b;
    succ[b] = (uint32_t)b;
}

// the class of the node whose run of sorted ends holds position i: 0 regular, 1 open, 2 flipped, 3 branch (valid at the head of
// the run; the low bit of an end is its kind, 0 outgoing, 1 incoming)
__device__ inline int mh_node_class(const uint32_t* __restrict__ ekey, const uint32_t* __restrict__ eval, int64_t i, int64_t n2, bool& head)
{
    const uint32_t v = ekey[i];
    head = i == 0 || ekey[i - 1] != v;
    const bool n1 = i + 1 < n2 && ekey[i + 1] == v, n2nd = n1 && i + 2 < n2 && ekey[i + 2] == v;
    if (!n1) return 1;
    if (n2nd) return 3;
    return ((eval[i] ^ eval[i + 1]) & 1u) ? 0 : 2;
}

// one thread per sorted end: a member of a run joins the member before it, whatever the node's class; the head of a regular run
// writes the successor of the incoming half-edge
__global__ void __launch_bounds__(256) mh_link_kernel(const uint32_t* __restrict__ ekey, const uint32_t* __restrict__ eval, int64_t n2,
                                                       uint32_t* parent, uint32_t* __restrict__ succ)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n2) return;
    bool head = false;
    const int cls = mh_node_class(ekey, eval, i, n2, head);
    if (!head) {
        ms_union(parent, eval[i - 1] >> 1, eval[i] >> 1);
        return;
    }
    if (cls == 0) {
        const uint32_t e0 = eval[i], e1 = eval[i + 1];
        const uint32_t in = (e0 & 1u) ? e0 : e1, out = (e0 & 1u) ? e1 : e0;
        succ[in >> 1] = out >> 1;
    }
}

// num = the exclusive scan of flag: the rim of every half-edge, the sort pairs, first half-edge and n_edges of every rim; n_rims
__global__ void __launch_bounds__(256) mh_number_kernel(int64_t nb, const uint32_t* __restrict__ parent, const int32_t* __restrict__ flag,
                                                         const int32_t* __restrict__ num, const uint32_t* __restrict__ bh,
                                                         uint32_t* __restrict__ skey, uint32_t* __restrict__ sval, int64_t* __restrict__ counts,
                                                         uint64_t* __restrict__ small)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = b < nb;
    int32_t rim = -1;
    if (active) {
        rim = num[parent[b]];   // (ms_flatten_kernel left parent = root)
        skey[b] = (uint32_t)rim;
        sval[b] = (uint32_t)b;
        if (flag[b]) counts[(int64_t)rim * MH_NCNT + MH_FIRST] = (int64_t)bh[b];
        if (b == nb - 1) small[MH_NRIMS] = (uint64_t)(num[b] + flag[b]);
    }
    const bool add[1] = {true};
    ms_count<1, MH_NCNT>(active, rim, add, MH_NEDGES, counts);
}

// one thread per sorted end; the head of a run counts the node and its class into the rim of its half-edge
__global__ void __launch_bounds__(256) mh_node_kernel(const uint32_t* __restrict__ ekey, const uint32_t* __restrict__ eval, int64_t n2,
                                                       const uint32_t* __restrict__ skey, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    bool add[4] = {true, false, false, false};   // node, open, flipped, branch
    int32_t rim = -1;
    if (i < n2) {
        const int cls = mh_node_class(ekey, eval, i, n2, head);
        if (head) {
            add[1] = cls == 1, add[2] = cls == 2, add[3] = cls == 3;
            rim = (int32_t)skey[eval[i] >> 1];
        }
    }
    ms_count<4, MH_NCNT>(head, rim, add, MH_NNODES, counts);
}

// one thread per possible rim c < n_b (n_rims is read on the device): closed flag, the longest closed rim, the totals, and what the
// fill adds for the rim (0 beyond n_rims, so that the scans run over n_b entries)
__global__ void __launch_bounds__(256) mh_closed_kernel(int64_t nb, int32_t fill, int64_t max_edges, int64_t* __restrict__ counts,
                                                         int32_t* __restrict__ closed, int32_t* __restrict__ addv, int64_t* __restrict__ addt,
                                                         uint64_t* __restrict__ small)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nr = (int64_t)small[MH_NRIMS];
    long long v[4] = {0, 0, 0, 0};   // nodes, irregular nodes, closed rims, filled rims
    long long loop = 0;
    if (c < nb) {
        int32_t av = 0;
        int64_t at = 0;
        if (c < nr) {
            int64_t* rec = counts + c * MH_NCNT;
            const int64_t ne = rec[MH_NEDGES];
            v[0] = rec[MH_NNODES];
            v[1] = rec[3] + rec[4] + rec[5];
            const bool cl = v[1] == 0;
            closed[c] = cl ? 1 : 0;
            v[2] = cl ? 1 : 0;
            loop = cl ? ne : 0;
            const bool sel = cl && fill && (max_edges < 0 || ne <= max_edges);
            v[3] = sel ? 1 : 0;
            av = sel && ne > 3 ? 1 : 0;
            at = sel ? (ne > 3 ? ne : 1) : 0;
            rec[MH_STATUS] = cl ? 1 : 0;
            rec[MH_ADDED] = -1;
        }
        addv[c] = av;
        addt[c] = at;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(loop, d, 64);
        loop = o > loop ? o : loop;
    }
    if ((threadIdx.x & 63) == 0 && loop) atomicMax((unsigned long long*)&small[MH_MAXLOOP], (unsigned long long)loop);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd((unsigned long long*)&small[MH_NODES + k], (unsigned long long)v[k]);
    }
}

// voff / toff = the exclusive scans of addv / addt: status and added vertex of every selected rim, the added counts
__global__ void __launch_bounds__(256) mh_fill_kernel(int64_t nb, int64_t n_verts, const int32_t* __restrict__ addv, const int32_t* __restrict__ voff,
                                                       const int64_t* __restrict__ addt, const int64_t* __restrict__ toff,
                                                       int64_t* __restrict__ counts, uint64_t* __restrict__ small)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nb) return;
    if (addt[c] > 0) {
        counts[c * MH_NCNT + MH_STATUS] = addv[c] ? 3 : 2;
        counts[c * MH_NCNT + MH_ADDED] = addv[c] ? n_verts + (int64_t)voff[c] : -1;
    }
    if (c == nb - 1) {
        small[MH_ADDV] = (uint64_t)((int64_t)voff[c] + addv[c]);
        small[MH_ADDT] = (uint64_t)(toff[c] + addt[c]);
    }
}

// one thread per output position: the 7 terms of its half-edge into the segmented sum of its block (ms_block_sum: slot block + rim)
__global__ void __launch_bounds__(MS_BLOCK) mh_sum_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           const uint32_t* __restrict__ skey, const int32_t* __restrict__ rim_edge, int64_t nb,
                                                           double rx, double ry, double rz, double* __restrict__ partial)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    const bool active = i < nb;
    uint32_t key = 0xffffffffu;
    double v[MH_NSUM];
#pragma unroll
    for (int q = 0; q < MH_NSUM; ++q) v[q] = 0.0;
    if (active) {
        key = skey[i];
        int32_t from, to;
        mh_from_to(tris, (uint32_t)rim_edge[i], from, to);
        const float *pa = verts + 3 * (int64_t)from, *pb = verts + 3 * (int64_t)to;
        const double Ax = (double)pa[0] - rx, Ay = (double)pa[1] - ry, Az = (double)pa[2] - rz;
        const double Bx = (double)pb[0] - rx, By = (double)pb[1] - ry, Bz = (double)pb[2] - rz;
        const double Dx = Bx - Ax, Dy = By - Ay, Dz = Bz - Az;
        v[0] = sqrt((Dx * Dx + Dy * Dy) + Dz * Dz);
        v[1] = Ay * Bz - Az * By;
        v[2] = Az * Bx - Ax * Bz;
        v[3] = Ax * By - Ay * Bx;
        v[4] = Ax, v[5] = Ay, v[6] = Az;
    }
    ms_block_sum<MH_NSUM>(active, key, v, partial);
}

// the fill, one thread per rim: the added vertex of a fan cap, per axis r + S / n_edges in double, rounded to float32
__global__ void __launch_bounds__(256) mh_apply_vert_kernel(int64_t nr, const int64_t* __restrict__ counts, const double* __restrict__ sums,
                                                             double rx, double ry, double rz, float* __restrict__ verts_out)
{
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nr || counts[c * MH_NCNT + MH_STATUS] != 3) return;
    const int64_t j = counts[c * MH_NCNT + MH_ADDED];
    const double n = (double)counts[c * MH_NCNT + MH_NEDGES];
    const double* S = sums + c * MH_NSUM + 4;
    verts_out[3 * j] = (float)(rx + S[0] / n);
    verts_out[3 * j + 1] = (float)(ry + S[1] / n);
    verts_out[3 * j + 2] = (float)(rz + S[2] / n);
}

// the fill, one thread per output position: boundary half-edge a -> b of a fan cap adds (b, a, w); the first half-edge a -> b of
// a filled rim of three, a -> b -> c -> a, adds (b, a, c)
__global__ void __launch_bounds__(256) mh_apply_cap_kernel(const int32_t* __restrict__ tris, const uint32_t* __restrict__ skey,
                                                            const int32_t* __restrict__ rim_edge, int64_t nb, const int64_t* __restrict__ counts,
                                                            const int64_t* __restrict__ start, const int64_t* __restrict__ toff, int64_t n_tris,
                                                            int32_t* __restrict__ tris_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t c = (int64_t)skey[i], status = counts[c * MH_NCNT + MH_STATUS], rank = i - start[c];
    if (status < 2 || (status == 2 && rank != 0)) return;
    int32_t a, b, third = (int32_t)counts[c * MH_NCNT + MH_ADDED];
    mh_from_to(tris, (uint32_t)rim_edge[i], a, b);
    if (status == 2) {
        int32_t b2;
        mh_from_to(tris, (uint32_t)rim_edge[i + 1], b2, third);   // (a rim of three: position i + 1 is inside it)
    }
    int32_t* out = tris_out + 3 * (n_tris + toff[c] + rank);
    out[0] = b, out[1] = a, out[2] = third;
}

// work buffers of the hole calls, kept per device between calls (r2s_release_cache frees them)
struct HoleWork : MsHalfEdgeBufs {
    DevBuf verts, tris, flag, small, bflag, bpos, bh, ekey, ekey2, eval, eval2, parent, succ, rflag, num, skey, skey2, sval, sval2, counts,
        closed, addv, voff, addt, toff, pp0, pp1, start, rim_edge, partial, sums, tris_out, verts_out;
};
PerDevice<HoleWork> g_holes_work;

struct HoleTables {
    std::vector<int64_t> start;     // [n_rims + 1] (empty without rims)
    std::vector<int64_t> counts;    // [n_rims][8]
    std::vector<double> sums;       // [n_rims][7]
    std::vector<int32_t> rim_edge;  // [n_b]
};
thread_local HoleTables g_last_holes;

struct HoleSizes {
    int64_t n_rims = 0, n_edges = 0, n_verts_out = 0, n_tris_out = 0;
    double r[3] = {0.0, 0.0, 0.0};
    int64_t totals[8] = {};
};

// The rims of the device mesh on the current device, after the work queued on `st`; synchronous.  Leaves the tables in w.start
// [n_rims + 1], w.counts / w.sums [n_rims], w.rim_edge [n_b] and what holes_apply needs in w.skey2 / w.toff.
int holes_core(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, bool fill, int64_t max_edges, hipStream_t st,
               HoleWork& w, HoleSizes& out)
{
    uint64_t h_small[MH_SMALL];
    if (const int rc = ms_begin_small(w.small, h_small, d_verts, n_verts, st)) return rc;
    uint64_t* small = w.small.as<uint64_t>();
    const int64_t nh = 3 * n;
    const uint64_t ckey = ms_collapsed_key(n_verts);
    size_t tb = 0, sb = 0, sb2 = 0;
    if (n > 0) {
        ENSURE(w.bflag, sizeof(int32_t) * (size_t)nh);
        ENSURE(w.bpos, sizeof(int32_t) * (size_t)nh);
        ENSURE(w.bh, sizeof(uint32_t) * (size_t)nh);
        int32_t *bflag = w.bflag.as<int32_t>(), *bpos = w.bpos.as<int32_t>();
        HIP_TRY(rocprim::exclusive_scan(nullptr, sb, bflag, bpos, (int32_t)0, (size_t)nh, rocprim::plus<int32_t>(), st));
        int rc = ms_sort_half_edges<0, false>(w, d_tris, n, n_verts, nullptr, nullptr, small + MH_COLLAPSED, sb, st);
        if (rc) return rc;
        mh_flag_kernel<<<ms_blocks(nh), 256, 0, st>>>(w.keys2.as<uint64_t>(), w.vals2.as<uint32_t>(), nh, ckey, bflag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb, bflag, bpos, (int32_t)0, (size_t)nh, rocprim::plus<int32_t>(), st));
        mh_compact_kernel<<<ms_blocks(nh), 256, 0, st>>>(nh, bflag, bpos, w.bh.as<uint32_t>(), small);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ms_ref_point(h_small, n_verts, out.r);
    const int64_t nb = (int64_t)h_small[MH_NB], n2 = 2 * nb;
    int64_t nr = 0;
    if (nb > 0) {
        // n_rims <= n_b: everything per rim is sized for n_b of them, and the number of rims is read with the totals
        const int64_t nblk = (nb + MS_BLOCK - 1) / MS_BLOCK;
        ENSURE(w.ekey, sizeof(uint32_t) * (size_t)n2);
        ENSURE(w.ekey2, sizeof(uint32_t) * (size_t)n2);
        ENSURE(w.eval, sizeof(uint32_t) * (size_t)n2);
        ENSURE(w.eval2, sizeof(uint32_t) * (size_t)n2);
        ENSURE(w.parent, sizeof(uint32_t) * (size_t)nb);
        ENSURE(w.succ, sizeof(uint32_t) * (size_t)nb);
        ENSURE(w.rflag, sizeof(int32_t) * (size_t)nb);
        ENSURE(w.num, sizeof(int32_t) * (size_t)nb);
        ENSURE(w.skey, sizeof(uint32_t) * (size_t)nb);
        ENSURE(w.skey2, sizeof(uint32_t) * (size_t)nb);
        ENSURE(w.sval, sizeof(uint32_t) * (size_t)nb);
        ENSURE(w.sval2, sizeof(uint32_t) * (size_t)nb);
        ENSURE(w.counts, sizeof(int64_t) * MH_NCNT * (size_t)nb);
        ENSURE(w.closed, sizeof(int32_t) * (size_t)nb);
        ENSURE(w.addv, sizeof(int32_t) * (size_t)nb);
        ENSURE(w.voff, sizeof(int32_t) * (size_t)nb);
        ENSURE(w.addt, sizeof(int64_t) * (size_t)nb);
        ENSURE(w.toff, sizeof(int64_t) * (size_t)nb);
        ENSURE(w.pp0, sizeof(uint64_t) * (size_t)nb);
        ENSURE(w.pp1, sizeof(uint64_t) * (size_t)nb);
        ENSURE(w.start, sizeof(int64_t) * (size_t)(nb + 1));
        ENSURE(w.rim_edge, sizeof(int32_t) * (size_t)nb);
        ENSURE(w.partial, sizeof(double) * MH_NSUM * (size_t)(nblk + nb));
        ENSURE(w.sums, sizeof(double) * MH_NSUM * (size_t)nb);
        uint32_t *ekey = w.ekey.as<uint32_t>(), *ekey2 = w.ekey2.as<uint32_t>(), *eval = w.eval.as<uint32_t>(), *eval2 = w.eval2.as<uint32_t>();
        uint32_t *parent = w.parent.as<uint32_t>(), *succ = w.succ.as<uint32_t>(), *bh = w.bh.as<uint32_t>();
        uint32_t *skey = w.skey.as<uint32_t>(), *skey2 = w.skey2.as<uint32_t>(), *sval = w.sval.as<uint32_t>(), *sval2 = w.sval2.as<uint32_t>();
        int32_t *rflag = w.rflag.as<int32_t>(), *num = w.num.as<int32_t>(), *closed = w.closed.as<int32_t>();
        int32_t *addv = w.addv.as<int32_t>(), *voff = w.voff.as<int32_t>();
        int64_t *addt = w.addt.as<int64_t>(), *toff = w.toff.as<int64_t>(), *counts = w.counts.as<int64_t>();
        const unsigned vbits = ms_bits((uint64_t)n_verts);
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, ekey, ekey2, eval, eval2, (size_t)n2, 0u, vbits, st));
        HIP_TRY(rocprim::exclusive_scan(nullptr, sb, rflag, num, (int32_t)0, (size_t)nb, rocprim::plus<int32_t>(), st));
        HIP_TRY(rocprim::exclusive_scan(nullptr, sb2, addt, toff, (int64_t)0, (size_t)nb, rocprim::plus<int64_t>(), st));
        ENSURE(w.temp, std::max<size_t>(std::max(tb, std::max(sb, sb2)), 16));
        mh_end_kernel<<<ms_blocks(nb), 256, 0, st>>>(d_tris, bh, nb, ekey, eval, parent, succ);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_pairs(w.temp.p, tb, ekey, ekey2, eval, eval2, (size_t)n2, 0u, vbits, st));
        mh_link_kernel<<<ms_blocks(n2), 256, 0, st>>>(ekey2, eval2, n2, parent, succ);
        HIP_TRY(hipGetLastError());
        ms_flatten_kernel<false><<<ms_blocks(nb), 256, 0, st>>>(nullptr, nb, parent, rflag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb, rflag, num, (int32_t)0, (size_t)nb, rocprim::plus<int32_t>(), st));
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * MH_NCNT * (size_t)nb, st));
        mh_number_kernel<<<ms_blocks(nb), 256, 0, st>>>(nb, parent, rflag, num, bh, skey, sval, counts, small);
        HIP_TRY(hipGetLastError());
        mh_node_kernel<<<ms_blocks(n2), 256, 0, st>>>(ekey2, eval2, n2, skey, counts);
        HIP_TRY(hipGetLastError());
        mh_closed_kernel<<<ms_blocks(nb), 256, 0, st>>>(nb, fill ? 1 : 0, max_edges, counts, closed, addv, addt, small);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb, addv, voff, (int32_t)0, (size_t)nb, rocprim::plus<int32_t>(), st));
        HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb2, addt, toff, (int64_t)0, (size_t)nb, rocprim::plus<int64_t>(), st));
        mh_fill_kernel<<<ms_blocks(nb), 256, 0, st>>>(nb, n_verts, addv, voff, addt, toff, counts, small);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        nr = (int64_t)h_small[MH_NRIMS];

        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, skey, skey2, sval, sval2, (size_t)nb, 0u, ms_bits((uint64_t)nr), st));
        ENSURE(w.temp, std::max<size_t>(tb, 16));
        // the round count comes from the longest closed rim the device found
        if (const int rc = ms_order_loops<MH_NCNT, MH_NEDGES, true>(nb, nr, h_small[MH_MAXLOOP], closed, parent, succ, counts, skey, skey2, sval,
                                                                    sval2, w.pp0.as<uint64_t>(), w.pp1.as<uint64_t>(), w.temp.p, tb,
                                                                    w.start.as<int64_t>(), bh, w.rim_edge.as<uint32_t>(), st))
            return rc;
        mh_sum_kernel<<<(unsigned)nblk, MS_BLOCK, 0, st>>>(d_verts, d_tris, skey2, w.rim_edge.as<int32_t>(), nb, out.r[0], out.r[1], out.r[2],
                                                          w.partial.as<double>());
        HIP_TRY(hipGetLastError());
        ms_combine_kernel<MH_NSUM><<<(unsigned)((nr + 3) / 4), 256, 0, st>>>(w.start.as<int64_t>(), nr, w.partial.as<double>(), w.sums.as<double>(),
                                                                          nullptr, 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    const int64_t addv = nb > 0 ? (int64_t)h_small[MH_ADDV] : 0, addt = nb > 0 ? (int64_t)h_small[MH_ADDT] : 0;
    if (n_verts + addv > INT32_MAX)
        return fail(R2S_ERR_UNSUPPORTED, "mesh_holes: the fill needs %lld vertices, beyond 32-bit indices", (long long)(n_verts + addv));
    out.n_rims = nr, out.n_edges = nb, out.n_verts_out = n_verts + addv, out.n_tris_out = n + addt;
    out.totals[0] = nr, out.totals[1] = nb, out.totals[2] = (int64_t)h_small[MH_COLLAPSED];
    out.totals[3] = nb > 0 ? (int64_t)h_small[MH_NODES] : 0, out.totals[4] = nb > 0 ? (int64_t)h_small[MH_IRREGULAR] : 0;
    out.totals[5] = nb > 0 ? (int64_t)h_small[MH_CLOSED] : 0, out.totals[6] = nb > 0 ? (int64_t)h_small[MH_FILLED] : 0, out.totals[7] = addt;
    return 0;
}

// queues the filled mesh of the mesh holes_core has just analysed on `st`: the vertices when d_verts_out is given, the triangles
// when d_tris_out is (room for n_verts_out / n_tris_out is the caller's business)
int holes_apply(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, const HoleSizes& s, hipStream_t st, HoleWork& w,
                int32_t* d_tris_out, float* d_verts_out)
{
    if (d_verts_out) {
        if (n_verts > 0) HIP_TRY(hipMemcpyAsync(d_verts_out, d_verts, vert_bytes(n_verts), hipMemcpyDeviceToDevice, st));
        if (s.n_verts_out > n_verts) {
            mh_apply_vert_kernel<<<ms_blocks(s.n_rims), 256, 0, st>>>(s.n_rims, w.counts.as<int64_t>(), w.sums.as<double>(), s.r[0], s.r[1],
                                                                     s.r[2], d_verts_out);
            HIP_TRY(hipGetLastError());
        }
    }
    if (d_tris_out) {
        if (n > 0) HIP_TRY(hipMemcpyAsync(d_tris_out, d_tris, tri_bytes(n), hipMemcpyDeviceToDevice, st));
        if (s.n_tris_out > n) {
            mh_apply_cap_kernel<<<ms_blocks(s.n_edges), 256, 0, st>>>(d_tris, w.skey2.as<uint32_t>(), w.rim_edge.as<int32_t>(), s.n_edges,
                                                                     w.counts.as<int64_t>(), w.start.as<int64_t>(), w.toff.as<int64_t>(), n,
                                                                     d_tris_out);
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// the checks that need no device; *fill: the fill was asked for
int holes_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, const void* tris_out, const void* verts_out,
               int64_t vert_capacity, int64_t tri_capacity, const int64_t* n_rims, const int64_t* n_edges, const int64_t* n_verts_out,
               const int64_t* n_tris_out, const double* ref_point, const int64_t* totals, const Span* tables, int n_tables, bool* fill)
{
    const int rc = mesh_args("mesh_holes", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (n_tris > MH_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_holes: 3 * %lld half-edges reach 2^31", (long long)n_tris);
    if (!n_rims || !n_edges || !n_verts_out || !n_tris_out || !ref_point || !totals)
        return fail(R2S_ERR_ARG, "mesh_holes: null n_rims / n_edges / n_verts_out / n_tris_out / ref_point / totals");
    if (vert_capacity < 0 || tri_capacity < 0) return fail(R2S_ERR_ARG, "mesh_holes: negative vert_capacity / tri_capacity");
    *fill = tris_out || verts_out;
    if (*fill && (!tris_out || !verts_out)) return fail(R2S_ERR_ARG, "mesh_holes: the fill needs tris_out and verts_out together");
    const Span in[2] = {{verts, vert_bytes(n_verts)}, {tris, tri_bytes(n_tris)}};
    const Span out[2] = {{tris_out, tri_bytes(tri_capacity)}, {verts_out, vert_bytes(vert_capacity)}};
    for (const auto& i : in) {
        for (const auto& o : out)
            if (overlaps(o, i)) return fail(R2S_ERR_ARG, "mesh_holes: an output overlaps an input");
        for (int k = 0; k < n_tables; ++k)
            if (overlaps(tables[k], i)) return fail(R2S_ERR_ARG, "mesh_holes: an output overlaps an input");
    }
    return 0;
}

int table_args(const char* who, const void* start, const void* counts, const void* sums, int64_t rim_capacity, const void* rim_edge,
               int64_t edge_capacity)
{
    if (rim_capacity < 0 || edge_capacity < 0 || (rim_capacity > 0 && (!start || !counts || !sums)) || (edge_capacity > 0 && !rim_edge))
        return fail(R2S_ERR_ARG, "%s: null tables or a negative capacity", who);
    return 0;
}

// where a device caller wants the tables and the room it has for them (a host caller: none)
struct HoleDevTables {
    int64_t *start = nullptr, *counts = nullptr;
    double* sums = nullptr;
    int64_t rim_capacity = 0;
    int32_t* rim_edge = nullptr;
    int64_t edge_capacity = 0;
};

// One call for both kinds of caller: the core, the fill (the vertices when vert_capacity holds n_verts_out of them, the
// triangles when tri_capacity holds n_tris_out), then the tables and the scalars.  A host caller's tables are kept whole for
// r2s_last_mesh_holes; a device caller gets the three per-rim tables when rim_capacity holds all rims and rim_edge when
// edge_capacity holds all edges.
int holes_run(MeshCall<HoleWork>& c, int64_t n_verts, int64_t n_tris, int64_t max_edges, const HoleDevTables& d, bool fill, int32_t* tris_out,
              float* verts_out, int64_t vert_capacity, int64_t tri_capacity, int64_t* n_rims, int64_t* n_edges, int64_t* n_verts_out,
              int64_t* n_tris_out, double ref_point[3], int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    HoleWork& w = c.work();
    HoleTables tab;
    HoleSizes s;
    if ((rc = holes_core(c.d_verts(), n_verts, c.d_tris(), n_tris, fill, max_edges, c.stream(), w, s))) return rc;
    const bool vroom = fill && vert_capacity >= s.n_verts_out, troom = fill && tri_capacity >= s.n_tris_out;
    float* d_verts_out = nullptr;
    int32_t* d_tris_out = nullptr;
    if (vroom && (rc = c.staged(w.verts_out, verts_out, vert_bytes(std::max<int64_t>(s.n_verts_out, 1)), d_verts_out))) return rc;
    if (troom && (rc = c.staged(w.tris_out, tris_out, tri_bytes(std::max<int64_t>(s.n_tris_out, 1)), d_tris_out))) return rc;
    if ((vroom || troom) && (rc = holes_apply(c.d_verts(), n_verts, c.d_tris(), n_tris, s, c.stream(), w, d_tris_out, d_verts_out))) return rc;
    const size_t nr = (size_t)s.n_rims;
    const bool rims_fit = d.rim_capacity >= s.n_rims, edges_fit = d.edge_capacity >= s.n_edges;
    if ((rc = c.table(tab.start, d.start, rims_fit, w.start, nr ? nr + 1 : 0)) ||
        (rc = c.table(tab.counts, d.counts, rims_fit, w.counts, nr * MH_NCNT)) || (rc = c.table(tab.sums, d.sums, rims_fit, w.sums, nr * MH_NSUM)) ||
        (rc = c.table(tab.rim_edge, d.rim_edge, edges_fit, w.rim_edge, nr ? (size_t)s.n_edges : 0)) ||
        (rc = c.deliver(vroom ? verts_out : nullptr, d_verts_out, vert_bytes(s.n_verts_out))) ||
        (rc = c.deliver(troom ? tris_out : nullptr, d_tris_out, tri_bytes(s.n_tris_out))) || (rc = c.finish()))
        return rc;
    if (c.is_host()) g_last_holes = std::move(tab);
    *n_rims = s.n_rims, *n_edges = s.n_edges, *n_verts_out = s.n_verts_out, *n_tris_out = s.n_tris_out;
    std::memcpy(ref_point, s.r, sizeof s.r);
    std::memcpy(totals, s.totals, sizeof s.totals);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_holes(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device, int64_t max_edges,
                   int32_t* tris_out, float* verts_out, int64_t vert_capacity, int64_t tri_capacity, int64_t* n_rims, int64_t* n_edges,
                   int64_t* n_verts_out, int64_t* n_tris_out, double ref_point[3], int64_t totals[8])
{
    bool fill = false;
    if (const int rc = holes_args(verts, n_verts, tris, n_tris, tris_out, verts_out, vert_capacity, tri_capacity, n_rims, n_edges, n_verts_out,
                                  n_tris_out, ref_point, totals, nullptr, 0, &fill))
        return rc;
    MeshCall<HoleWork> call("mesh_holes", g_holes_work, verts, n_verts, tris, n_tris, device);
    return holes_run(call, n_verts, n_tris, max_edges, {}, fill, tris_out, verts_out, vert_capacity, tri_capacity, n_rims, n_edges, n_verts_out,
                     n_tris_out, ref_point, totals);
}

int r2s_last_mesh_holes(int64_t* rim_start_out, int64_t* counts_out, double* sums_out, int64_t rim_capacity, int32_t* rim_edge_out,
                        int64_t edge_capacity, int64_t* n_rims, int64_t* n_edges)
{
    if (!n_rims || !n_edges) return fail(R2S_ERR_ARG, "last_mesh_holes: null n_rims / n_edges");
    const int rc = table_args("last_mesh_holes", rim_start_out, counts_out, sums_out, rim_capacity, rim_edge_out, edge_capacity);
    if (rc) return rc;
    const HoleTables& t = g_last_holes;
    const int64_t nr = *n_rims = (int64_t)(t.counts.size() / MH_NCNT), nb = *n_edges = (int64_t)t.rim_edge.size();
    const int64_t mr = copy_rows(counts_out, t.counts, MH_NCNT, rim_capacity, nr);
    copy_rows(sums_out, t.sums, MH_NSUM, rim_capacity, nr);
    if (mr > 0) copy_rows(rim_start_out, t.start, 1, mr + 1, nr + 1);   // (the end of the last rim copied with it)
    copy_rows(rim_edge_out, t.rim_edge, 1, edge_capacity, nb);
    return 0;
}

int r2s_mesh_holes_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, int64_t max_edges, int64_t* d_rim_start,
                       int64_t* d_counts, double* d_sums, int64_t rim_capacity, int32_t* d_rim_edge, int64_t edge_capacity,
                       int32_t* d_tris_out, float* d_verts_out, int64_t vert_capacity, int64_t tri_capacity, int64_t* n_rims,
                       int64_t* n_edges, int64_t* n_verts_out, int64_t* n_tris_out, double ref_point[3], int64_t totals[8], void* stream)
{
    bool fill = false;
    int rc = table_args("mesh_holes", d_rim_start, d_counts, d_sums, rim_capacity, d_rim_edge, edge_capacity);
    if (rc) return rc;
    const Span tables[4] = {{d_rim_start, sizeof(int64_t) * ((size_t)rim_capacity + 1)},
                            {d_counts, sizeof(int64_t) * MH_NCNT * (size_t)rim_capacity},
                            {d_sums, sizeof(double) * MH_NSUM * (size_t)rim_capacity},
                            {d_rim_edge, sizeof(int32_t) * (size_t)edge_capacity}};
    if ((rc = holes_args(d_verts, n_verts, d_tris, n_tris, d_tris_out, d_verts_out, vert_capacity, tri_capacity, n_rims, n_edges, n_verts_out,
                         n_tris_out, ref_point, totals, tables, rim_capacity > 0 || edge_capacity > 0 ? 4 : 0, &fill)))
        return rc;
    MeshCall<HoleWork> call("mesh_holes", g_holes_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return holes_run(call, n_verts, n_tris, max_edges, {d_rim_start, d_counts, d_sums, rim_capacity, d_rim_edge, edge_capacity}, fill, d_tris_out,
                     d_verts_out, vert_capacity, tri_capacity, n_rims, n_edges, n_verts_out, n_tris_out, ref_point, totals);
}

}  // extern "C"
