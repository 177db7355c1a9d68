// Mesh nesting: which closed patch of a triangle mesh encloses which patch, the depth of every patch in that forest and the
// re-winding of the closed patches at odd depth (include/rho2sdf_hip.h, r2s_mesh_nesting; DESIGN.md "Mesh nesting").
//   ms_sort_half_edges (r2s_mesh_graph.hpp) ms_key_kernel<1, false>: the orient's half-edge keys, parent[t] = t -> rocPRIM radix
//                      sort of pairs
//   mn_union_kernel    the second member of every run of EXACTLY two joins its two triangles (the shells' union-find: larger
//                      root under the smaller, so a patch's root is its smallest triangle)
//   ms_flatten_kernel<true> (r2s_mesh_graph.hpp) parent = root, the flag of the first triangle of a patch -> rocPRIM exclusive
//                      scan -> ms_number_kernel<false, false> (r2s_mesh_graph.hpp): patch_of_tri, the orient's numbering; n_patches
//   mn_first_kernel    first_tri and n_tris of every patch; mn_edge_kernel: the half-edges in runs of one or of three and more,
//                      per patch; mn_record_kernel: closed[p], the record's start values
//   mn_cross_kernel<KZ, false>  one lane per query patch P, the per-lane LDS stack and the three-comparison cull of
//                      mwn_points_kernel from P's sample; a leaf of a closed foreign patch runs axis_cross (r2s_tri_math.hpp).
//                      The lane's count is the record's sum of crossings; one integer atomic per wavefront for the total.
//   mn_cross_kernel<KZ, true>   the same traversal again: every crossing takes a slot of a buffer of exactly that many keys
//                      (P << 32 | Q) through an integer cursor -> rocPRIM radix sort of the keys
//   mn_odd_kernel      the head of every run of equal keys walks its run: cross(P, Q); an odd run is a containment pair ->
//                      rocPRIM exclusive scan -> mn_compact_kernel: the sorted pair list
//   mn_depth_kernel    the head of every P segment of the pair list walks it: depth[P] = its length
//   mn_parent_kernel   the same walk with all depths known: the container of the largest depth, the first one (smallest Q) on a
//                      tie; n_children by integer atomicAdd
//   mn_final_kernel    one thread per patch: irregular, the status bits, the record; the sums of the totals (integer adds)
//   mn_maxdepth_kernel one workgroup: the largest depth
//   mn_rewind_kernel   one thread per triangle: (i0, i1, i2) -> (i0, i2, i1) in a closed patch at odd depth
// Integer work only; the only atomics are integer adds and the list cursor, whose list is sorted afterwards.
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
#include "r2s_mesh_tree.hpp"
#include "r2s_tri_math.hpp"

using namespace r2s_int;

namespace {

constexpr int MN_NCNT = 8;
constexpr int64_t MN_MAX_TRIS = (int64_t)1 << 30;
constexpr int32_t MN_FLAGS = 1;   // R2S_NESTING_REWIND
// slots of the small device array (uint64)
constexpr int MN_COLLAPSED = 0, MN_NPATCHES = 1, MN_CROSS = 2, MN_CURSOR = 3, MN_TOT = 4;   // [MN_TOT .. MN_TOT + 3]: closed patches, pairs, irregular, reversed triangles
constexpr int MN_MAXDEPTH = 8, MN_SMALL = 16;
// columns of the per-patch record
constexpr int MN_FIRST = 0, MN_NTRIS = 1, MN_STATUS = 2, MN_PARENT = 3, MN_DEPTH = 4, MN_CHILDREN = 5, MN_CROSSSUM = 6;
constexpr int64_t MN_CLOSED = 1, MN_REVERSED = 2, MN_IRREGULAR = 4;

// one thread per sorted half-edge: the second member of a run of exactly two joins the two triangles
__global__ void __launch_bounds__(256) mn_union_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                        uint64_t ckey, uint32_t* parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= nh || keys[i] >= ckey) return;
    bool head;
    if (ms_run_size(keys, i, nh, head) != 2 || head) return;
    ms_union(parent, vals[i - 1] / 3u, vals[i] / 3u);
}

// one thread per triangle: the first triangle of a patch writes first_tri; n_tris per patch
__global__ void __launch_bounds__(256) mn_first_kernel(int64_t n, const int32_t* __restrict__ flag, const int32_t* __restrict__ patch_of,
                                                        int64_t* __restrict__ counts)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t patch = -1;
    if (t < n) {
        patch = patch_of[t];
        if (flag[t]) counts[(int64_t)patch * MN_NCNT + MN_FIRST] = t;
    }
    const bool add[1] = {true};
    ms_count<1, MN_NCNT>(patch >= 0, patch, add, MN_NTRIS, counts);
}

// one thread per sorted half-edge: a half-edge in a run of one or of three and more counts into column MN_STATUS of its
// triangle's patch (mn_record_kernel turns that count into closed[p])
__global__ void __launch_bounds__(256) mn_edge_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, const int32_t* __restrict__ patch_of, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool open = false;
    int32_t patch = -1;
    if (i < nh && keys[i] < ckey) {
        bool head;
        open = ms_run_size(keys, i, nh, head) != 2;
        if (open) patch = patch_of[vals[i] / 3u];
    }
    const bool add[1] = {true};
    ms_count<1, MN_NCNT>(open, patch, add, MN_STATUS, counts);
}

__global__ void __launch_bounds__(256) mn_record_kernel(int64_t np, int64_t* __restrict__ counts, int32_t* __restrict__ closed)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    int64_t* rec = counts + p * MN_NCNT;
    closed[p] = rec[MN_STATUS] == 0 ? 1 : 0;
    rec[MN_STATUS] = 0;
    rec[MN_PARENT] = -1;
}

struct MnArgs {
    const MiNode* nodes;
    const float* verts;
    const int32_t* tris;
    int32_t root;                // node 0, or ~0 for a single triangle
    int neg;                     // the ray runs along -e_KZ
    int64_t np;
    const int32_t* patch_of;     // [ntris]
    const int32_t* closed;       // [np]
    int64_t* counts;             // [np][8]: MN_FIRST is read, MN_CROSSSUM written (the counting pass)
    unsigned long long* small;   // [MN_SMALL]
    uint64_t* keys;              // [nkeys] (the writing pass)
    unsigned long long nkeys;
};

// One lane per query patch, 64 consecutive patches per workgroup (one wavefront).  WRITE = false counts, WRITE = true lists.
template <int KZ, bool WRITE>
__global__ void __launch_bounds__(64) mn_cross_kernel(MnArgs g)
{
    __shared__ int32_t stk[MI_STACK * 64];
    const int lane = threadIdx.x;
    const int64_t P = (int64_t)blockIdx.x * 64 + lane;
    unsigned long long nc = 0;
    if (P < g.np) {
        constexpr int K1 = (KZ + 1) % 3, K2 = (KZ + 2) % 3;
        const float* s = g.verts + 3 * (int64_t)g.tris[3 * g.counts[P * MN_NCNT + MN_FIRST]];
        const Vec3 p = {(double)s[0], (double)s[1], (double)s[2]};
        const bool neg = g.neg != 0;
        const double o1 = vec_pick(p, K1), o2 = vec_pick(p, K2), oz = vec_pick(p, KZ);
        int sp = 0;
        int32_t cur = g.root;
        for (;;) {
            if (cur < 0) {
                const int32_t t = ~cur;
                const int32_t Q = g.patch_of[t];   // (-1: a collapsed triangle takes part in nothing)
                if (Q >= 0 && Q != (int32_t)P && g.closed[Q]) {
                    const int32_t* tv = g.tris + 3 * (int64_t)t;
                    const float *a = g.verts + 3 * (int64_t)tv[0], *b = g.verts + 3 * (int64_t)tv[1], *c = g.verts + 3 * (int64_t)tv[2];
                    const float fa[3] = {a[0], a[1], a[2]}, fb[3] = {b[0], b[1], b[2]}, fc[3] = {c[0], c[1], c[2]};
                    if (axis_cross<KZ>(p, neg, fa, fb, fc) != 0) {
                        ++nc;
                        if (WRITE) {
                            const unsigned long long pos = atomicAdd(&g.small[MN_CURSOR], 1ull);
                            if (pos < g.nkeys) g.keys[pos] = ((uint64_t)(uint32_t)P << 32) | (uint64_t)(uint32_t)Q;
                        }
                    }
                }
            } else {
                const MiNode nd = load_node(g.nodes + cur);
                const bool e0 = axis_enter<KZ>(nd.box[0], o1, o2, oz, neg), e1 = axis_enter<KZ>(nd.box[1], o1, o2, oz, neg);
                if (e0 && e1) {
                    stk[sp * 64 + lane] = nd.child[1];
                    ++sp;
                }
                if (e0 || e1) {
                    cur = e0 ? nd.child[0] : nd.child[1];
                    continue;
                }
            }
            if (sp == 0) break;
            --sp;
            cur = stk[sp * 64 + lane];
        }
        if (!WRITE) g.counts[P * MN_NCNT + MN_CROSSSUM] = (int64_t)nc;
    }
    if (WRITE) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nc += __shfl_xor(nc, d, 64);
    if (lane == 0 && nc) atomicAdd(&g.small[MN_CROSS], nc);
}

// one thread per sorted key: the head of a run of equal keys walks it; odd[i] = 1 where the run's length, cross(P, Q), is odd
__global__ void __launch_bounds__(256) mn_odd_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ odd)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    int32_t o = 0;
    if (i == 0 || keys[i - 1] != k) {
        int64_t j = i + 1;
        while (j < n && keys[j] == k) ++j;
        o = (int32_t)((j - i) & 1);
    }
    odd[i] = o;
}

// pos = the exclusive scan of odd: the containment pairs, in the order of the sorted keys
__global__ void __launch_bounds__(256) mn_compact_kernel(const uint64_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ odd,
                                                          const int32_t* __restrict__ pos, int64_t* __restrict__ pairs)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && odd[i]) pairs[pos[i]] = (int64_t)keys[i];
}

// one thread per pair: the first pair of a query P walks P's segment; depth[P] = its length (zeroed before)
__global__ void __launch_bounds__(256) mn_depth_kernel(const int64_t* __restrict__ pairs, int64_t n, int32_t* __restrict__ depth)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t P = pairs[i] >> 32;
    if (i > 0 && (pairs[i - 1] >> 32) == P) return;
    int64_t j = i + 1;
    while (j < n && (pairs[j] >> 32) == P) ++j;
    depth[P] = (int32_t)(j - i);
}

// the same walk: the container of the largest depth, the first of them (ascending Q) on a tie; one child more for it
__global__ void __launch_bounds__(256) mn_parent_kernel(const int64_t* __restrict__ pairs, int64_t n, const int32_t* __restrict__ depth,
                                                         int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t P = pairs[i] >> 32;
    if (i > 0 && (pairs[i - 1] >> 32) == P) return;
    int64_t best = -1;
    int32_t bd = -1;
    for (int64_t j = i; j < n && (pairs[j] >> 32) == P; ++j) {
        const int64_t Q = pairs[j] & 0xffffffffll;
        const int32_t d = depth[Q];
        if (d > bd) bd = d, best = Q;
    }
    counts[P * MN_NCNT + MN_PARENT] = best;
    atomicAdd((unsigned long long*)&counts[best * MN_NCNT + MN_CHILDREN], 1ull);
}

// one thread per patch: irregular, the status bits, the record; the sums of the totals
__global__ void __launch_bounds__(256) mn_final_kernel(int64_t np, int32_t flags, const int32_t* __restrict__ closed,
                                                        const int32_t* __restrict__ depth, int64_t* __restrict__ counts,
                                                        unsigned long long* __restrict__ small)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long c[4] = {0, 0, 0, 0};   // closed patches, pairs, irregular, reversed triangles
    if (p < np) {
        int64_t* rec = counts + p * MN_NCNT;
        const int32_t d = depth[p];
        const bool cl = closed[p] != 0;
        const bool irregular = d > 0 && depth[rec[MN_PARENT]] != d - 1;
        const bool reversed = (flags & MN_FLAGS) && cl && (d & 1);
        rec[MN_STATUS] = (cl ? MN_CLOSED : 0) | (reversed ? MN_REVERSED : 0) | (irregular ? MN_IRREGULAR : 0);
        rec[MN_DEPTH] = d;
        rec[7] = 0;
        c[0] = cl, c[1] = (unsigned long long)d, c[2] = irregular, c[3] = reversed ? (unsigned long long)rec[MN_NTRIS] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c[k] += __shfl_xor(c[k], s, 64);
        if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(&small[MN_TOT + k], c[k]);
    }
}

// one workgroup: the largest depth (a maximum needs no atomic here)
__global__ void __launch_bounds__(1024) mn_maxdepth_kernel(const int32_t* __restrict__ depth, int64_t np, unsigned long long* __restrict__ small)
{
    __shared__ int32_t s_max[16];
    int32_t m = 0;
    for (int64_t p = threadIdx.x; p < np; p += 1024) m = depth[p] > m ? depth[p] : m;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int32_t o = __shfl_xor(m, s, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) m = s_max[k] > m ? s_max[k] : m;
        small[MN_MAXDEPTH] = (unsigned long long)m;
    }
}

// one thread per triangle: reversed in a closed patch at odd depth, else copied
__global__ void __launch_bounds__(256) mn_rewind_kernel(const int32_t* __restrict__ tris, int64_t n, const int32_t* __restrict__ patch_of,
                                                         const int32_t* __restrict__ closed, const int32_t* __restrict__ depth,
                                                         int32_t* __restrict__ tris_out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    const int32_t p = patch_of[t];
    const bool rev = p >= 0 && closed[p] && (depth[p] & 1);
    tris_out[3 * t] = i0;
    tris_out[3 * t + 1] = rev ? i2 : i1;
    tris_out[3 * t + 2] = rev ? i1 : i2;
}

// work buffers of the nesting calls, kept per device between calls (r2s_release_cache frees them)
struct NestWork : MsHalfEdgeBufs {
    DevBuf verts, tris, tris_out, flag, small, parent, rflag, num, patch, counts, closed, depth, ckeys, ckeys2, odd, pos, pairs;
};
PerDevice<NestWork> g_nest_work;

struct NestTables {
    std::vector<int64_t> counts;   // [n][8]
    std::vector<int64_t> pairs;    // [m]
};
thread_local NestTables g_last_nest;

template <bool WRITE>
void launch_cross(const MnArgs& g, int kz, unsigned waves, hipStream_t st)
{
    if (kz == 0)
        mn_cross_kernel<0, WRITE><<<waves, 64, 0, st>>>(g);
    else if (kz == 1)
        mn_cross_kernel<1, WRITE><<<waves, 64, 0, st>>>(g);
    else
        mn_cross_kernel<2, WRITE><<<waves, 64, 0, st>>>(g);
}

// The nesting of the device mesh on the current device, after the work queued on `st`; synchronous.  index: the tree of the
// same mesh, or null: one is built here and dropped.  Leaves patch_of_tri in w.patch [n], the records in w.counts [n_patches],
// the sorted pair list in w.pairs [n_pairs] and, with the rewind flag, the triangles in d_tris_out [n]; the scalars go to the
// host pointers.  Nothing of the caller's is written before the last refusal.
int nesting_core(const MiTree* index, const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, int32_t ray, int32_t flags,
                 hipStream_t st, NestWork& w, int32_t* d_tris_out, int64_t* n_patches, int64_t* n_pairs, int64_t totals[8])
{
    *n_patches = *n_pairs = 0;
    for (int k = 0; k < 8; ++k) totals[k] = 0;
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    unsigned long long h_small[MN_SMALL] = {};
    ENSURE(w.small, sizeof h_small);
    unsigned long long* small = w.small.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(small, 0, sizeof h_small, st));
    const int64_t nh = 3 * n;
    const uint64_t ckey = ms_collapsed_key(n_verts);
    int rc = ms_group_triangles<1, false, false, false>(
        w, d_tris, n, n_verts, w.parent, nullptr, nullptr, w.rflag, w.num, w.patch, nullptr, nullptr, (uint64_t*)small + MN_COLLAPSED,
        (uint64_t*)small + MN_NPATCHES,
        [&](const uint64_t* keys2, const uint32_t* vals2, int64_t nhe, uint64_t ck, uint32_t* parent) {
            mn_union_kernel<<<ms_blocks(nhe), 256, 0, st>>>(keys2, vals2, nhe, ck, parent);
        },
        [&](uint32_t* parent, int32_t* flag) { ms_flatten_kernel<true><<<ms_blocks(n), 256, 0, st>>>(d_tris, n, parent, flag); }, st);
    if (rc) return rc;
    const uint64_t* hkeys = w.keys2.as<uint64_t>();
    const uint32_t* hvals = w.vals2.as<uint32_t>();
    int32_t *rflag = w.rflag.as<int32_t>(), *patch = w.patch.as<int32_t>();
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t np = (int64_t)h_small[MN_NPATCHES], ncol = (int64_t)h_small[MN_COLLAPSED];
    unsigned long long ncross = 0;
    int64_t npairs = 0;
    if (np > 0) {
        MiTree built;   // (dropped on return: the nodes free themselves)
        if (!index) {
            if ((rc = mi_build_tree(d_verts, n_verts, d_tris, n, st, built))) return rc;
            index = &built;
        }
        const MiTree& T = *index;
        if ((rc = check_depth(T))) return rc;
        ENSURE(w.counts, sizeof(int64_t) * MN_NCNT * (size_t)np);
        ENSURE(w.closed, sizeof(int32_t) * (size_t)np);
        ENSURE(w.depth, sizeof(int32_t) * (size_t)np);
        int64_t* counts = w.counts.as<int64_t>();
        int32_t *closed = w.closed.as<int32_t>(), *depth = w.depth.as<int32_t>();
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * MN_NCNT * (size_t)np, st));
        HIP_TRY(hipMemsetAsync(depth, 0, sizeof(int32_t) * (size_t)np, st));
        mn_first_kernel<<<ms_blocks(n), 256, 0, st>>>(n, rflag, patch, counts);
        HIP_TRY(hipGetLastError());
        mn_edge_kernel<<<ms_blocks(nh), 256, 0, st>>>(hkeys, hvals, nh, ckey, patch, counts);
        HIP_TRY(hipGetLastError());
        mn_record_kernel<<<ms_blocks(np), 256, 0, st>>>(np, counts, closed);
        HIP_TRY(hipGetLastError());
        MnArgs g = {};
        g.nodes = T.nodes.as<MiNode>();
        g.verts = T.verts, g.tris = T.tris, g.root = T.root, g.neg = ray >= 3 ? 1 : 0;
        g.np = np, g.patch_of = patch, g.closed = closed, g.counts = counts, g.small = small;
        const unsigned waves = (unsigned)((np + 63) / 64);
        launch_cross<false>(g, ray % 3, waves, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ncross = h_small[MN_CROSS];
        if (ncross > (unsigned long long)INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "mesh_nesting: %llu crossings exceed 2^31 - 1", ncross);
        if (ncross > 0) {
            const size_t nc = (size_t)ncross;
            ENSURE(w.ckeys, sizeof(uint64_t) * nc);
            ENSURE(w.ckeys2, sizeof(uint64_t) * nc);
            ENSURE(w.odd, sizeof(int32_t) * nc);
            ENSURE(w.pos, sizeof(int32_t) * nc);
            uint64_t *keys = w.ckeys.as<uint64_t>(), *keys2 = w.ckeys2.as<uint64_t>();
            int32_t *odd = w.odd.as<int32_t>(), *pos = w.pos.as<int32_t>();
            const unsigned bits = std::min(32u + ms_bits((uint64_t)np), 64u);
            size_t tb = 0, sb = 0;
            HIP_TRY(rocprim::radix_sort_keys(nullptr, tb, keys, keys2, nc, 0u, bits, st));
            HIP_TRY(rocprim::exclusive_scan(nullptr, sb, odd, pos, (int32_t)0, nc, rocprim::plus<int32_t>(), st));
            ENSURE(w.temp, std::max<size_t>(std::max(tb, sb), 16));
            g.keys = keys, g.nkeys = ncross;
            launch_cross<true>(g, ray % 3, waves, st);
            HIP_TRY(hipGetLastError());
            HIP_TRY(rocprim::radix_sort_keys(w.temp.p, tb, keys, keys2, nc, 0u, bits, st));
            mn_odd_kernel<<<ms_blocks((int64_t)nc), 256, 0, st>>>(keys2, (int64_t)nc, odd);
            HIP_TRY(hipGetLastError());
            HIP_TRY(rocprim::exclusive_scan(w.temp.p, sb, odd, pos, (int32_t)0, nc, rocprim::plus<int32_t>(), st));
            int32_t last[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(&last[0], pos + (nc - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&last[1], odd + (nc - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            npairs = (int64_t)last[0] + last[1];
            if (npairs > 0) {
                ENSURE(w.pairs, sizeof(int64_t) * (size_t)npairs);
                int64_t* pairs = w.pairs.as<int64_t>();
                mn_compact_kernel<<<ms_blocks((int64_t)nc), 256, 0, st>>>(keys2, (int64_t)nc, odd, pos, pairs);
                HIP_TRY(hipGetLastError());
                mn_depth_kernel<<<ms_blocks(npairs), 256, 0, st>>>(pairs, npairs, depth);
                HIP_TRY(hipGetLastError());
                mn_parent_kernel<<<ms_blocks(npairs), 256, 0, st>>>(pairs, npairs, depth, counts);
                HIP_TRY(hipGetLastError());
            }
        }
        mn_final_kernel<<<ms_blocks(np), 256, 0, st>>>(np, flags, closed, depth, counts, small);
        HIP_TRY(hipGetLastError());
        mn_maxdepth_kernel<<<1, 1024, 0, st>>>(depth, np, small);
        HIP_TRY(hipGetLastError());
        if (flags & MN_FLAGS) {
            mn_rewind_kernel<<<ms_blocks(n), 256, 0, st>>>(d_tris, n, patch, closed, depth, d_tris_out);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // (a tree built here is dropped behind this)
    } else if (flags & MN_FLAGS) {
        HIP_TRY(hipMemcpyAsync(d_tris_out, d_tris, tri_bytes(n), hipMemcpyDeviceToDevice, st));   // (every triangle is collapsed)
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_patches = np, *n_pairs = npairs;
    totals[0] = np, totals[1] = n, totals[2] = ncol;
    if (np > 0) {
        totals[3] = (int64_t)h_small[MN_TOT], totals[4] = (int64_t)h_small[MN_TOT + 1], totals[5] = (int64_t)h_small[MN_MAXDEPTH];
        totals[6] = (int64_t)h_small[MN_TOT + 2], totals[7] = (int64_t)h_small[MN_TOT + 3];
    }
    return 0;
}

// the checks that need no device
int nesting_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, int32_t ray, int32_t flags, const void* tris_out,
                 const int64_t* n_patches, const int64_t* totals)
{
    const int rc = mesh_args("mesh_nesting", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (n_tris > MN_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_nesting: %lld triangles exceed 2^30", (long long)n_tris);
    if (ray < 0 || ray > 5) return fail(R2S_ERR_ARG, "mesh_nesting: ray must be 0..5 (+x +y +z -x -y -z), got %d", (int)ray);
    if (flags & ~MN_FLAGS) return fail(R2S_ERR_ARG, "mesh_nesting: unknown flag bits in %d", (int)flags);
    if ((flags & MN_FLAGS) && n_tris > 0 && !tris_out) return fail(R2S_ERR_ARG, "mesh_nesting: null tris_out with R2S_NESTING_REWIND");
    if ((flags & MN_FLAGS) && overlaps(tris_out, tri_bytes(n_tris), tris, tri_bytes(n_tris)))
        return fail(R2S_ERR_ARG, "mesh_nesting: tris_out overlaps tris");
    if (!n_patches || !totals) return fail(R2S_ERR_ARG, "mesh_nesting: null n_patches / totals");
    return 0;
}

// One call for both kinds of caller: the core, then the triangles (with the rewind flag), patch_of_tri, the two tables and the
// scalars.  The triangles go to a work buffer first for either caller: a refusal behind the traversal leaves tris_out untouched.
// A host caller's tables are kept whole for r2s_last_mesh_nesting; a device caller gets each one when its capacity holds all of it.
int nesting_run(MeshCall<NestWork>& c, const r2s_mesh_index* index, int64_t n_verts, int64_t n_tris, int32_t ray, int32_t flags,
                int32_t* tris_out, int32_t* patch_of_tri, int64_t* d_counts, int64_t patch_capacity, int64_t* d_pairs, int64_t pair_capacity,
                int64_t* n_patches, int64_t* n_pairs, int64_t totals[8])
{
    int rc = c.open([&] { return index ? index_on_current_device("mesh_nesting", index) : 0; });
    if (rc) return rc;
    NestWork& w = c.work();
    NestTables tab;
    const bool rewind = (flags & MN_FLAGS) != 0;
    int64_t np = 0, npairs = 0, tot[8];
    int32_t* d_tris_out = nullptr;
    if (rewind && (rc = c.staged(w.tris_out, tris_out, tri_bytes(std::max<int64_t>(n_tris, 1)), d_tris_out, c.STAGE_DEVICE_CALLER))) return rc;
    if ((rc = nesting_core(index ? &index->tree : nullptr, c.d_verts(), n_verts, c.d_tris(), n_tris, ray, flags, c.stream(), w, d_tris_out, &np,
                           &npairs, tot)) ||
        (rc = c.table(tab.counts, d_counts, patch_capacity >= np, w.counts, (size_t)np * MN_NCNT)) ||
        (rc = c.table(tab.pairs, d_pairs, pair_capacity >= npairs, w.pairs, (size_t)npairs)) ||
        (rc = c.deliver(rewind ? tris_out : nullptr, d_tris_out, tri_bytes(n_tris))) ||
        (rc = c.deliver(patch_of_tri, w.patch.p, sizeof(int32_t) * (size_t)n_tris)) || (rc = c.finish()))
        return rc;
    if (c.is_host()) g_last_nest = std::move(tab);
    *n_patches = np;
    if (n_pairs) *n_pairs = npairs;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_nesting(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t ray, int32_t flags, int32_t device,
                     int32_t* tris_out, int32_t* patch_of_tri_out, int64_t* n_patches, int64_t totals[8])
{
    if (const int rc = nesting_args(verts, n_verts, tris, n_tris, ray, flags, tris_out, n_patches, totals)) return rc;
    MeshCall<NestWork> call("mesh_nesting", g_nest_work, verts, n_verts, tris, n_tris, device);
    return nesting_run(call, nullptr, n_verts, n_tris, ray, flags, tris_out, patch_of_tri_out, nullptr, 0, nullptr, 0, n_patches, nullptr, totals);
}

int r2s_last_mesh_nesting(int64_t* counts_out, int64_t capacity, int64_t* pairs_out, int64_t pair_capacity, int64_t* n_patches,
                          int64_t* n_pairs)
{
    if (!n_patches || !n_pairs || capacity < 0 || pair_capacity < 0 || (capacity > 0 && !counts_out) || (pair_capacity > 0 && !pairs_out))
        return fail(R2S_ERR_ARG, "last_mesh_nesting: null output or negative capacity");
    *n_patches = (int64_t)(g_last_nest.counts.size() / MN_NCNT), *n_pairs = (int64_t)g_last_nest.pairs.size();
    copy_rows(counts_out, g_last_nest.counts, MN_NCNT, capacity, *n_patches);
    copy_rows(pairs_out, g_last_nest.pairs, 1, pair_capacity, *n_pairs);
    return 0;
}

int r2s_mesh_nesting_dev(const r2s_mesh_index* index, const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, int32_t ray,
                         int32_t flags, int32_t* d_tris_out, int32_t* d_patch_of_tri, int64_t* d_counts, int64_t patch_capacity,
                         int64_t* d_pairs, int64_t pair_capacity, int64_t* n_patches, int64_t* n_pairs, int64_t totals[8], void* stream)
{
    if (const int rc = nesting_args(d_verts, n_verts, d_tris, n_tris, ray, flags, d_tris_out, n_patches, totals)) return rc;
    if (!n_pairs) return fail(R2S_ERR_ARG, "mesh_nesting: null n_pairs");
    if (patch_capacity < 0 || pair_capacity < 0 || (patch_capacity > 0 && !d_counts) || (pair_capacity > 0 && !d_pairs))
        return fail(R2S_ERR_ARG, "mesh_nesting: null tables or a negative capacity");
    if (index && index->tree.n_tris != n_tris)
        return fail(R2S_ERR_ARG, "mesh_nesting: the index holds %lld triangles, the mesh %lld", (long long)index->tree.n_tris, (long long)n_tris);
    MeshCall<NestWork> call("mesh_nesting", g_nest_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return nesting_run(call, index, n_verts, n_tris, ray, flags, d_tris_out, d_patch_of_tri, d_counts, patch_capacity, d_pairs, pair_capacity,
                       n_patches, n_pairs, totals);
}

}  // extern "C"
