// Mesh intersections: the pairs of triangles of one mesh that intersect or touch, found through the tree of the mesh index
// (include/rho2sdf_hip.h, r2s_mesh_index_intersections; DESIGN.md "Self-intersections").
//   mx_pairs_kernel<false>  one lane per triangle s, the per-lane LDS stack of mi_query_kernel: every node whose child box
//                           overlaps the box of s is entered, a leaf t > s runs the collapsed and shared-index checks and the
//                           segment tests (seg_tri_hit, r2s_tri_math.hpp).  Per-lane integer counters, summed over the wavefront,
//                           one integer atomic per wavefront and counter; integer atomicAdd into hits_of_tri for both members.
//   mx_involved_kernel      the number of triangles with hits_of_tri > 0
//   mx_pairs_kernel<true>   the same traversal again, run only when the caller has room for all pairs: every intersecting pair
//                           takes a slot of a buffer of exactly totals[0] keys (s << 32 | t) through an integer cursor
//   rocPRIM radix sort of the keys -> mx_unpack_kernel: pairs [n][2]
// Closed-box overlap is exact and conservative: two triangles with a common point have overlapping float32 boxes, and so has
// every ancestor of either leaf (mi_refit_kernel joins boxes with min / max, no rounding), so the traversal visits every
// candidate pair of the definition and the results are those of a loop over all pairs.  No floating-point value is stored.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_tree.hpp"
#include "r2s_tri_math.hpp"

using namespace r2s_int;

namespace {

// slots of the small device array (uint64): the first six are totals[0..5] of the header
constexpr int MX_PAIRS = 0, MX_INVOLVED = 1, MX_CAND = 2, MX_ADJ = 3, MX_ONE = 4, MX_COLLAPSED = 5, MX_CURSOR = 6, MX_SMALL = 8;

struct MxArgs {
    const MiNode* nodes;
    const float* verts;
    const int32_t* tris;
    int64_t ntris;
    int32_t root;              // node 0, or ~0 for a single triangle
    int32_t* hits;             // [ntris], zeroed (the counting pass)
    unsigned long long* small; // [MX_SMALL]
    uint64_t* keys;            // [nkeys] (the writing pass)
    unsigned long long nkeys;
};

// corner c of the nine floats of a triangle (a 0-2, b 3-5, c 6-8) by selects (an indexed register array would go to scratch)
struct MxF3 {
    float x, y, z;
};
__device__ inline float mx_pick(float a, float b, float c, int k) { return k == 0 ? a : (k == 1 ? b : c); }
// (all nine are read before the selects: a load inside an arm of ?: is merged into one load through a computed address)
__device__ inline MxF3 mx_corner(const float* f, int c)
{
    const float ax = f[0], ay = f[1], az = f[2], bx = f[3], by = f[4], bz = f[5], cx = f[6], cy = f[7], cz = f[8];
    return {mx_pick(ax, bx, cx, c), mx_pick(ay, by, cy, c), mx_pick(az, bz, cz, c)};
}
// own ? u : v, widened to double
__device__ inline Vec3 mx_sel(bool own, MxF3 u, MxF3 v) { return {(double)(own ? u.x : v.x), (double)(own ? u.y : v.y), (double)(own ? u.z : v.z)}; }

__device__ inline void mx_load_tri(const float* __restrict__ verts, int32_t i0, int32_t i1, int32_t i2, float f[9])
{
    const float *a = verts + 3 * (int64_t)i0, *b = verts + 3 * (int64_t)i1, *c = verts + 3 * (int64_t)i2;
    f[0] = a[0], f[1] = a[1], f[2] = a[2], f[3] = b[0], f[4] = b[1], f[5] = b[2], f[6] = c[0], f[7] = c[1], f[8] = c[2];
}

// closed overlap of the box (lo, hi) with the box b (lo xyz, hi xyz) on all three axes, in float32
__device__ inline bool mx_overlap(const float* lo, const float* hi, const float* b)
{
    return lo[0] <= b[3] && b[0] <= hi[0] && lo[1] <= b[4] && b[1] <= hi[1] && lo[2] <= b[5] && b[2] <= hi[2];
}

// the corner of (j0, j1, j2) that holds index v, 3 when none does
__device__ inline int mx_find(int32_t v, int32_t j0, int32_t j1, int32_t j2) { return v == j0 ? 0 : (v == j1 ? 1 : (v == j2 ? 2 : 3)); }

// Any of the segment tests in `mask` hits: bit c < 3 is edge c (corner c -> corner (c + 1) % 3) of fs against the triangle ft,
// bit 3 + c the edge c of ft against fs.  One test per round of a rolled loop: the code of seg_tri_hit exists once.
__device__ inline bool mx_pair_hits(const float* fs, const float* ft, unsigned mask)
{
    bool hit = false;
#pragma nounroll
    for (int k = 0; k < 6 && !hit; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const bool own = k < 3;
        const int c = own ? k : k - 3, c1 = c == 2 ? 0 : c + 1;
        // p -> q: edge c of the edge's own triangle; a b c: the other triangle
        const Vec3 p = mx_sel(own, mx_corner(fs, c), mx_corner(ft, c)), q = mx_sel(own, mx_corner(fs, c1), mx_corner(ft, c1));
        hit = seg_tri_hit(p, q, mx_sel(own, mx_corner(ft, 0), mx_corner(fs, 0)), mx_sel(own, mx_corner(ft, 1), mx_corner(fs, 1)),
                          mx_sel(own, mx_corner(ft, 2), mx_corner(fs, 2)));
    }
    return hit;
}

// One lane per triangle s, 64 consecutive triangles per workgroup (one wavefront).  WRITE = false counts, WRITE = true lists.
template <bool WRITE>
__global__ void __launch_bounds__(64) mx_pairs_kernel(MxArgs g)
{
#pragma clang fp contract(off)
    __shared__ int32_t stk[MI_STACK * 64];
    const int lane = threadIdx.x;
    const int64_t s64 = (int64_t)blockIdx.x * 64 + lane;
    const bool valid = s64 < g.ntris;
    const int32_t s = (int32_t)s64;
    unsigned long long n_hit = 0, n_cand = 0, n_adj = 0, n_one = 0;
    bool collapsed = false;
    if (valid) {
        const int32_t i0 = g.tris[3 * s64], i1 = g.tris[3 * s64 + 1], i2 = g.tris[3 * s64 + 2];
        collapsed = i0 == i1 || i1 == i2 || i0 == i2;
        if (!collapsed) {
            float fs[9], lo[3], hi[3];
            mx_load_tri(g.verts, i0, i1, i2, fs);
            tri_box(fs, fs + 3, fs + 6, lo, hi);
            int sp = 0;
            int32_t cur = g.root;
            for (;;) {
                if (cur < 0) {
                    const int32_t t = ~cur;
                    if (t > s) {
                        const int32_t* tv = g.tris + 3 * (int64_t)t;
                        const int32_t j0 = tv[0], j1 = tv[1], j2 = tv[2];
                        if (!(j0 == j1 || j1 == j2 || j0 == j2)) {
                            float ft[9], bx[6];
                            mx_load_tri(g.verts, j0, j1, j2, ft);
                            tri_box(ft, ft + 3, ft + 6, bx, bx + 3);
                            if (mx_overlap(lo, hi, bx)) {
                                ++n_cand;
                                // the corners of t that hold i0, i1, i2 (3: none); the indices of a triangle are distinct here
                                const int b0 = mx_find(i0, j0, j1, j2), b1 = mx_find(i1, j0, j1, j2), b2 = mx_find(i2, j0, j1, j2);
                                const int shared = (b0 < 3) + (b1 < 3) + (b2 < 3);
                                if (shared >= 2) {
                                    ++n_adj;
                                } else {
                                    unsigned mask = 0x3fu;
                                    if (shared == 1) {
                                        ++n_one;
                                        const int a = b0 < 3 ? 0 : (b1 < 3 ? 1 : 2);     // the corner of s at the shared vertex
                                        const int b = b0 < 3 ? b0 : (b1 < 3 ? b1 : b2);   // and that of t
                                        // the edge opposite corner a runs from corner (a + 1) % 3: edge number (a + 1) % 3
                                        mask = (1u << (a == 2 ? 0 : a + 1)) | (8u << (b == 2 ? 0 : b + 1));
                                    }
                                    if (mx_pair_hits(fs, ft, mask)) {
                                        ++n_hit;
                                        if (WRITE) {
                                            const unsigned long long pos = atomicAdd(&g.small[MX_CURSOR], 1ull);
                                            if (pos < g.nkeys) g.keys[pos] = ((uint64_t)(uint32_t)s << 32) | (uint64_t)(uint32_t)t;
                                        } else {
                                            atomicAdd(&g.hits[t], 1);
                                        }
                                    }
                                }
                            }
                        }
                    }
                } else {
                    const MiNode nd = load_node(g.nodes + cur);
                    // (a leaf child t <= s has nothing to add: its pair belongs to the lane of t)
                    const bool e0 = mx_overlap(lo, hi, nd.box[0]) && (nd.child[0] >= 0 || ~nd.child[0] > s);
                    const bool e1 = mx_overlap(lo, hi, nd.box[1]) && (nd.child[1] >= 0 || ~nd.child[1] > s);
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
            if (!WRITE && n_hit) atomicAdd(&g.hits[s], (int32_t)n_hit);
        }
    }
    if (WRITE) return;
    unsigned long long c[5] = {n_hit, n_cand, n_adj, n_one, collapsed ? 1ull : 0ull};
    const int slot[5] = {MX_PAIRS, MX_CAND, MX_ADJ, MX_ONE, MX_COLLAPSED};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c[k] += __shfl_xor(c[k], d, 64);
        if (lane == 0 && c[k]) atomicAdd(&g.small[slot[k]], c[k]);
    }
}

__global__ void __launch_bounds__(256) mx_involved_kernel(const int32_t* __restrict__ hits, int64_t n, unsigned long long* __restrict__ small)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long m = __ballot(t < n && hits[t] > 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&small[MX_INVOLVED], (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) mx_unpack_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ pairs)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    pairs[2 * i] = (int32_t)(uint32_t)(k >> 32);
    pairs[2 * i + 1] = (int32_t)(uint32_t)k;
}

// work buffers of the intersection calls, kept per device between calls (r2s_release_cache frees them)
struct IsectWork {
    DevBuf verts, tris, flag, small, hits, keys, keys2, temp, pairs;
};
PerDevice<IsectWork> g_mx_work;

inline unsigned mx_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
inline unsigned mx_bits(uint64_t max_value)
{
    unsigned b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

// The intersections of the tree's mesh on the current device, after the work queued on `st`; synchronous.  Leaves hits_of_tri in
// w.hits [n_tris]; the pair list goes to d_pairs (null: to w.pairs) when capacity >= the number of pairs, else nothing is
// written.  tot[0..7] are the header's totals.
// Two traversals rather than one into a capacity-bounded buffer: the count has to reach the host before anything may be written
// (a short buffer stays untouched), the key buffer then has exactly the size of the answer whatever capacity the caller names,
// and a call that only asks for the counts pays one traversal and no sort.
int isect_core(const MiTree& T, hipStream_t st, IsectWork& w, int32_t* d_pairs, int64_t capacity, int64_t tot[8])
{
    if (const int rc = check_depth(T)) return rc;
    for (int k = 0; k < 8; ++k) tot[k] = 0;
    const int64_t n = T.n_tris;
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    unsigned long long h_small[MX_SMALL] = {};
    ENSURE(w.small, sizeof h_small);
    ENSURE(w.hits, sizeof(int32_t) * (size_t)n);
    unsigned long long* small = w.small.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(small, 0, sizeof h_small, st));
    HIP_TRY(hipMemsetAsync(w.hits.p, 0, sizeof(int32_t) * (size_t)n, st));
    MxArgs g = {};
    g.nodes = T.nodes.as<MiNode>();
    g.verts = T.verts, g.tris = T.tris, g.ntris = n, g.root = T.root;
    g.hits = w.hits.as<int32_t>(), g.small = small;
    const unsigned waves = (unsigned)((n + 63) / 64);
    mx_pairs_kernel<false><<<waves, 64, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    mx_involved_kernel<<<mx_blocks(n), 256, 0, st>>>(w.hits.as<int32_t>(), n, small);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned long long np = h_small[MX_PAIRS];
    if (np > (unsigned long long)INT32_MAX)
        return fail(R2S_ERR_UNSUPPORTED, "mesh_intersections: %llu intersecting pairs exceed 2^31 - 1", np);
    if (np > 0 && (unsigned long long)capacity >= np) {
        ENSURE(w.keys, sizeof(uint64_t) * (size_t)np);
        ENSURE(w.keys2, sizeof(uint64_t) * (size_t)np);
        if (!d_pairs) {
            ENSURE(w.pairs, 2 * sizeof(int32_t) * (size_t)np);
            d_pairs = w.pairs.as<int32_t>();
        }
        uint64_t *keys = w.keys.as<uint64_t>(), *keys2 = w.keys2.as<uint64_t>();
        const unsigned bits = std::min(32u + mx_bits((uint64_t)n), 64u);
        size_t tb = 0;
        HIP_TRY(rocprim::radix_sort_keys(nullptr, tb, keys, keys2, (size_t)np, 0u, bits, st));
        ENSURE(w.temp, std::max<size_t>(tb, 16));
        g.keys = keys, g.nkeys = np;
        mx_pairs_kernel<true><<<waves, 64, 0, st>>>(g);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_keys(w.temp.p, tb, keys, keys2, (size_t)np, 0u, bits, st));
        mx_unpack_kernel<<<mx_blocks((int64_t)np), 256, 0, st>>>(keys2, (int64_t)np, d_pairs);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (int k = 0; k < 6; ++k) tot[k] = (int64_t)h_small[k];
    return 0;
}

int isect_args(const void* pairs, int64_t capacity, const int64_t* totals)
{
    if (!totals) return fail(R2S_ERR_ARG, "mesh_intersections: null totals");
    if (capacity < 0) return fail(R2S_ERR_ARG, "mesh_intersections: negative pair_capacity");
    if (capacity > 0 && !pairs) return fail(R2S_ERR_ARG, "mesh_intersections: null pairs with a capacity");
    return 0;
}

// the host-pointer tail of both host variants: copies what isect_core left on the device
int isect_download(IsectWork& w, int64_t n_tris, int32_t* hits_out, int32_t* pairs_out, int64_t capacity, const int64_t tot[8])
{
    if (hits_out && n_tris > 0) HIP_TRY(hipMemcpy(hits_out, w.hits.p, sizeof(int32_t) * (size_t)n_tris, hipMemcpyDeviceToHost));
    if (tot[0] > 0 && capacity >= tot[0]) HIP_TRY(hipMemcpy(pairs_out, w.pairs.p, 2 * sizeof(int32_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
    return 0;
}

// the device-pointer tail of both _dev variants (the pairs are in place already)
int isect_copy_dev(IsectWork& w, int64_t n_tris, int32_t* d_hits, hipStream_t st)
{
    if (d_hits && n_tris > 0) {
        HIP_TRY(hipMemcpyAsync(d_hits, w.hits.p, sizeof(int32_t) * (size_t)n_tris, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_index_intersections(const r2s_mesh_index* ix, int32_t* hits_of_tri_out, int32_t* pairs_out, int64_t pair_capacity,
                                 int64_t totals[8])
{
    if (!ix) return fail(R2S_ERR_ARG, "mesh_index_intersections: null index");
    int rc = isect_args(pairs_out, pair_capacity, totals);
    if (rc || (rc = check_device(0))) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(ix->device))) return rc;
    std::lock_guard<std::mutex> lock(g_mx_work.mu);
    IsectWork* w = g_mx_work.current(rc);
    if (rc) return rc;
    int64_t tot[8];
    if ((rc = isect_core(ix->tree, nullptr, *w, nullptr, pair_capacity, tot))) return rc;
    if ((rc = isect_download(*w, ix->tree.n_tris, hits_of_tri_out, pairs_out, pair_capacity, tot))) return rc;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

int r2s_mesh_index_intersections_dev(const r2s_mesh_index* ix, int32_t* d_hits_of_tri, int32_t* d_pairs, int64_t pair_capacity,
                                     int64_t totals[8], void* stream)
{
    if (!ix) return fail(R2S_ERR_ARG, "mesh_index_intersections: null index");
    int rc = isect_args(d_pairs, pair_capacity, totals);
    if (rc || (rc = check_device(0)) || (rc = index_on_current_device("mesh_index_intersections", ix))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_mx_work.mu);
    IsectWork* w = g_mx_work.current(rc);
    if (rc) return rc;
    int64_t tot[8];
    if ((rc = isect_core(ix->tree, st, *w, pair_capacity > 0 ? d_pairs : nullptr, pair_capacity, tot))) return rc;
    if ((rc = isect_copy_dev(*w, ix->tree.n_tris, d_hits_of_tri, st))) return rc;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

int r2s_mesh_intersections(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device,
                           int32_t* hits_of_tri_out, int32_t* pairs_out, int64_t pair_capacity, int64_t totals[8])
{
    int rc = mesh_args("mesh_intersections", verts, n_verts, tris, n_tris);
    if (rc || (rc = isect_args(pairs_out, pair_capacity, totals))) return rc;
    if ((rc = check_mesh_host("mesh_intersections", verts, n_verts, tris, n_tris)) || (rc = use_device(device))) return rc;
    std::lock_guard<std::mutex> lock(g_mx_work.mu);
    IsectWork* w = g_mx_work.current(rc);
    if (rc) return rc;
    if ((rc = upload_mesh(w->verts, w->tris, verts, n_verts, tris, n_tris, false, nullptr))) return rc;
    MiTree T;   // (built, used and dropped: the nodes free themselves)
    if ((rc = mi_build_tree(w->verts.as<float>(), n_verts, w->tris.as<int32_t>(), n_tris, nullptr, T))) return rc;
    int64_t tot[8];
    if ((rc = isect_core(T, nullptr, *w, nullptr, pair_capacity, tot))) return rc;
    if ((rc = isect_download(*w, n_tris, hits_of_tri_out, pairs_out, pair_capacity, tot))) return rc;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

int r2s_mesh_intersections_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, int32_t* d_hits_of_tri,
                               int32_t* d_pairs, int64_t pair_capacity, int64_t totals[8], void* stream)
{
    int rc = mesh_args("mesh_intersections", d_verts, n_verts, d_tris, n_tris);
    if (rc || (rc = isect_args(d_pairs, pair_capacity, totals)) || (rc = check_device(0))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_mx_work.mu);
    IsectWork* w = g_mx_work.current(rc);
    if (rc) return rc;
    if ((rc = check_mesh_dev("mesh_intersections", d_verts, n_verts, d_tris, n_tris, w->flag, st))) return rc;
    MiTree T;
    if ((rc = mi_build_tree(d_verts, n_verts, d_tris, n_tris, st, T))) return rc;
    int64_t tot[8];
    if ((rc = isect_core(T, st, *w, pair_capacity > 0 ? d_pairs : nullptr, pair_capacity, tot))) return rc;
    if ((rc = isect_copy_dev(*w, n_tris, d_hits_of_tri, st))) return rc;
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // extern "C"
