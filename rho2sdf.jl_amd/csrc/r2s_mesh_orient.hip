// Mesh orient: the orientable patches of a triangle mesh, a consistent winding for each, and the choice of that winding by the
// signed volume or by the majority (include/rho2sdf_hip.h, r2s_mesh_orient; DESIGN.md "Mesh orient").
//   ms_bounds_kernel   the box of all vertices -> the reference point (the shells' kernel)
//   ms_sort_half_edges (r2s_mesh_graph.hpp) ms_key_kernel<2, false>: one half-edge key per corner, the shells' keys, payload
//                      3t + c; parent[x] = x on the DOUBLED graph of 2 n_tris nodes, node 2t + s = "triangle t with parity s"
//                      -> rocPRIM radix sort of pairs
//   mo_union_kernel    the second member of every run of EXACTLY two: opposite directions join (2a, 2b) and (2a+1, 2b+1), equal
//                      directions join (2a, 2b+1) and (2a+1, 2b) (the shells' union-find: larger root under the smaller)
//   mo_flatten_kernel  root(2t) = 2f + rel[t] in an orientable patch with first triangle f, root(2t) = root(2t+1) = 2f in a
//                      non-orientable one: first triangle, parity and orientability of every triangle; root flags
//   -> rocPRIM exclusive scan (integers) -> ms_number_kernel<true, true> (r2s_mesh_graph.hpp): patch numbers, sort pairs
//   -> stable radix sort of the triangle ids by patch -> ms_segment_kernel (r2s_mesh_graph.hpp): where each patch starts, its
//      first triangle
//   mo_sum_kernel      blocks of 256 consecutive sorted triangles, the volume term negated where rel = 1 -> ms_block_sum<1>
//                      (r2s_mesh_graph.hpp): a segmented fixed tree in LDS, one partial per (block, patch) at slot block + patch
//   ms_combine_kernel<1> (r2s_mesh_graph.hpp) one wavefront per patch: up to 64 equal runs of its block partials in ascending
//                      order, then a fixed tree; n_tris of the patch
//   mo_parity_kernel   n1 per patch; mo_edge_kernel: the sorted edge runs again, boundary / non-manifold half-edges and the
//                      flipped edges of the input per patch
//   mo_decide_kernel   one thread per patch: closed, the whole-patch flip g, the record, the totals
//   mo_apply_kernel    one thread per triangle: flip = rel ^ g, (i0, i1, i2) -> (i0, i2, i1)
//   mo_remain_kernel   the sorted edge runs a third time: the flipped edges that remain in the output
// Integer counts use integer atomics; no floating-point atomic and no library reduction touches V.
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

constexpr int MO_NCNT = 8;
constexpr int64_t MO_MAX_TRIS = (int64_t)1 << 30;
constexpr int32_t MO_FLAGS = 1;   // R2S_ORIENT_OUTWARD
constexpr uint32_t MO_NONORIENTABLE = MS_DOUBLED_FLAG;   // bit 31 of info[t]; bits 0..30: root(2t) = 2 first_tri + rel
// slots of the small device array: [0..5] the bounds, then
constexpr int MO_COLLAPSED = 6, MO_NPATCHES = 7, MO_TOT = 8;   // [MO_TOT .. MO_TOT + 4]: flipped triangles, non-orientable, closed, by volume, remaining flipped edges
constexpr int MO_SMALL = 16;
// columns of the per-patch record
constexpr int MO_FIRST = 0, MO_NTRIS = 1, MO_NFLIP = 2, MO_STATUS = 3, MO_BOUNDARY = 4, MO_NONMANIFOLD = 5, MO_FLIPPED_IN = 6;

// one thread per sorted half-edge: the second member of a run of exactly two joins the two triangles on the doubled graph
__global__ void __launch_bounds__(256) mo_union_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                        uint64_t ckey, uint32_t* parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= nh) return;
    const uint64_t k = keys[i];
    if (k >= ckey) return;
    bool head;
    if (ms_run_size(keys, i, nh, head) != 2 || head) return;
    const uint32_t a = vals[i - 1] / 3u, b = vals[i] / 3u;
    const uint32_t same = (uint32_t)(((keys[i - 1] ^ k) & 1ull) == 0ull);   // equal directions: a flipped edge, the parities differ
    ms_union(parent, 2u * a, 2u * b + same);
    ms_union(parent, 2u * a + 1u, 2u * b + (same ^ 1u));
}

// info[t] = root(2t) | (root(2t) == root(2t + 1) ? MO_NONORIENTABLE : 0); flag[t] = 1 for the first triangle of a patch
__global__ void __launch_bounds__(256) mo_flatten_kernel(const int32_t* __restrict__ tris, int64_t n, uint32_t* parent, uint32_t* __restrict__ info,
                                                          int32_t* __restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int32_t i0, i1, i2;
    if (ms_collapsed(tris, t, i0, i1, i2)) {
        flag[t] = 0;
        info[t] = 0u;
        return;
    }
    const uint32_t r0 = ms_find(parent, (uint32_t)(2 * t)), r1 = ms_find(parent, (uint32_t)(2 * t + 1));
    info[t] = r0 | (r0 == r1 ? MO_NONORIENTABLE : 0u);
    flag[t] = r0 == (uint32_t)(2 * t) ? 1 : 0;
}

// the shells' volume term of one triangle, in the header's operation order
__device__ inline double mo_volume_term(const float* __restrict__ verts, int32_t i0, int32_t i1, int32_t i2, double rx, double ry, double rz)
{
#pragma clang fp contract(off)
    const float *pa = verts + 3 * (int64_t)i0, *pb = verts + 3 * (int64_t)i1, *pc = verts + 3 * (int64_t)i2;
    const double Ax = (double)pa[0] - rx, Ay = (double)pa[1] - ry, Az = (double)pa[2] - rz;
    const double Bx = (double)pb[0] - rx, By = (double)pb[1] - ry, Bz = (double)pb[2] - rz;
    const double Cx = (double)pc[0] - rx, Cy = (double)pc[1] - ry, Cz = (double)pc[2] - rz;
    const double det = (Ax * (By * Cz - Bz * Cy) + Ay * (Bz * Cx - Bx * Cz)) + Az * (Bx * Cy - By * Cx);
    return det / 6.0;
}

// one thread per sorted triangle: its volume term into the segmented sum of its block (ms_block_sum: slot block + patch)
__global__ void __launch_bounds__(MS_BLOCK) mo_sum_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           const uint32_t* __restrict__ info, const uint32_t* __restrict__ skey,
                                                           const uint32_t* __restrict__ stri, int64_t nvalid, double rx, double ry, double rz,
                                                           double* __restrict__ partial)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    const bool active = i < nvalid;
    uint32_t key = 0xffffffffu;
    double v[1] = {0.0};
    if (active) {
        key = skey[i];
        const int64_t t = (int64_t)stri[i];
        v[0] = mo_volume_term(verts, tris[3 * t], tris[3 * t + 1], tris[3 * t + 2], rx, ry, rz);
        if (info[t] & 1u) v[0] = -v[0];   // (a non-orientable patch has rel = 0 everywhere: the plain sum)
    }
    ms_block_sum<1>(active, key, v, partial);
}

// one thread per triangle: n1 of its patch, kept in column MO_NFLIP until mo_decide_kernel turns it into the flipped count
__global__ void __launch_bounds__(256) mo_parity_kernel(int64_t n, const uint32_t* __restrict__ info, const int32_t* __restrict__ patch_of,
                                                         int64_t* __restrict__ counts)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t patch = -1;
    bool odd = false;
    if (t < n) {
        patch = patch_of[t];
        odd = patch >= 0 && (info[t] & 1u);
    }
    const bool add[1] = {true};
    ms_count<1, MO_NCNT>(odd, patch, add, MO_NFLIP, counts);
}

// one thread per sorted half-edge: boundary and non-manifold half-edges count into the patch of their own triangle, a flipped
// edge (a run of two in the same direction: both triangles are in one patch) once, from its first member
__global__ void __launch_bounds__(256) mo_edge_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, const int32_t* __restrict__ patch_of, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool add[3] = {false, false, false};   // boundary, non-manifold, flipped
    int32_t patch = -1;
    bool any = false;
    if (i < nh && keys[i] < ckey) {
        bool head;
        const int size = ms_run_size(keys, i, nh, head);
        add[0] = size == 1;
        add[1] = size == 3;
        add[2] = size == 2 && head && ((keys[i + 1] ^ keys[i]) & 1ull) == 0ull;
        any = add[0] || add[1] || add[2];
        if (any) patch = patch_of[vals[i] / 3u];
    }
    ms_count<3, MO_NCNT>(any, patch, add, MO_BOUNDARY, counts);
}

// one thread per patch: closed, the whole-patch flip, the record and the volume as written; the totals
__global__ void __launch_bounds__(256) mo_decide_kernel(int64_t np, int32_t flags, const uint32_t* __restrict__ info, int64_t* __restrict__ counts,
                                                         double* __restrict__ vol, int32_t* __restrict__ gflag, uint64_t* __restrict__ small)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    long long c[4] = {0, 0, 0, 0};   // flipped triangles, non-orientable, closed, by volume
    if (s < np) {
        int64_t* rec = counts + s * MO_NCNT;
        const bool nonor = (info[rec[MO_FIRST]] & MO_NONORIENTABLE) != 0u;
        const bool closed = rec[MO_BOUNDARY] == 0 && rec[MO_NONMANIFOLD] == 0;
        const int64_t n1 = rec[MO_NFLIP], n0 = rec[MO_NTRIS] - n1;
        const double V = vol[s];
        bool g = false, by_volume = false;
        if (!nonor) {
            by_volume = (flags & MO_FLAGS) && closed && V != 0.0;
            g = by_volume ? V < 0.0 : n1 > n0;
        }
        const int64_t nflip = nonor ? 0 : (g ? n0 : n1);
        rec[MO_NFLIP] = nflip;
        rec[MO_STATUS] = (closed ? 1 : 0) | (nonor ? 2 : 0) | (by_volume ? 4 : 0);
        rec[7] = 0;
        if (g) vol[s] = -V;
        gflag[s] = g ? 1 : 0;
        c[0] = nflip, c[1] = nonor, c[2] = closed, c[3] = by_volume;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c[k] += __shfl_xor(c[k], d, 64);
        if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd((unsigned long long*)&small[MO_TOT + k], (unsigned long long)c[k]);
    }
}

// one thread per triangle: flip = rel ^ g of its patch (0 in a non-orientable patch and for a collapsed triangle)
__global__ void __launch_bounds__(256) mo_apply_kernel(const int32_t* __restrict__ tris, int64_t n, const uint32_t* __restrict__ info,
                                                        const int32_t* __restrict__ patch_of, const int32_t* __restrict__ gflag,
                                                        int32_t* __restrict__ tris_out, int32_t* __restrict__ flip)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int32_t i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    const int32_t s = patch_of[t];
    const uint32_t f = info[t];
    const bool fl = s >= 0 && !(f & MO_NONORIENTABLE) && (((f & 1u) != 0u) != (gflag[s] != 0));
    tris_out[3 * t] = i0;
    tris_out[3 * t + 1] = fl ? i2 : i1;
    tris_out[3 * t + 2] = fl ? i1 : i2;
    flip[t] = fl ? 1 : 0;
}

// one thread per sorted half-edge of the INPUT; the first member of a run of two tells whether the two half-edges still run in
// the same direction after the flips (a flipped triangle reverses all three of its half-edges)
__global__ void __launch_bounds__(256) mo_remain_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                         uint64_t ckey, const int32_t* __restrict__ flip, uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool left = false;
    if (i < nh && keys[i] < ckey) {
        bool head;
        if (ms_run_size(keys, i, nh, head) == 2 && head) {
            const uint32_t da = (uint32_t)(keys[i] & 1ull) ^ (uint32_t)flip[vals[i] / 3u];
            const uint32_t db = (uint32_t)(keys[i + 1] & 1ull) ^ (uint32_t)flip[vals[i + 1] / 3u];
            left = da == db;
        }
    }
    const unsigned long long m = __ballot(left);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)&small[MO_TOT + 4], (unsigned long long)__popcll(m));
}

// work buffers of the orient calls, kept per device between calls (r2s_release_cache frees them)
struct OrientWork : MsHalfEdgeBufs {
    DevBuf verts, tris, tris_out, flag, small, parent, info, rflag, num, patch, flip, skey, skey2, sval, sval2, seg, partial, counts, vol, gflag;
};
PerDevice<OrientWork> g_orient_work;

struct OrientTables {
    std::vector<int64_t> counts;   // [n][8]
    std::vector<double> volume;    // [n]
};
thread_local OrientTables g_last_orient;

// The oriented copy of the device mesh on the current device, after the work queued on `st`; synchronous.  Writes d_tris_out
// [n], leaves flip in w.flip and patch_of_tri in w.patch [n] and the tables in w.counts / w.vol [n_patches]; the scalars go to
// the host pointers.
int orient_core(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, int32_t flags, hipStream_t st, OrientWork& w,
                int32_t* d_tris_out, int64_t* n_patches, double ref_point[3], int64_t totals[8])
{
    uint64_t h_small[MO_SMALL];
    int rc = ms_begin_small(w.small, h_small, d_verts, n_verts, st);
    if (rc) return rc;
    uint64_t* small = w.small.as<uint64_t>();
    const int64_t nh = 3 * n;
    const uint64_t ckey = ms_collapsed_key(n_verts);
    if (n > 0) {
        ENSURE(w.info, sizeof(uint32_t) * (size_t)n);
        ENSURE(w.flip, sizeof(int32_t) * (size_t)n);
        ENSURE(w.skey2, sizeof(uint32_t) * (size_t)n);
        ENSURE(w.sval2, sizeof(uint32_t) * (size_t)n);
        uint32_t* info = w.info.as<uint32_t>();
        rc = ms_group_triangles<2, false, true, true>(
            w, d_tris, n, n_verts, w.parent, nullptr, info, w.rflag, w.num, w.patch, &w.skey, &w.sval, small + MO_COLLAPSED, small + MO_NPATCHES,
            [&](const uint64_t* keys2, const uint32_t* vals2, int64_t nhe, uint64_t ck, uint32_t* parent) {
                mo_union_kernel<<<ms_blocks(nhe), 256, 0, st>>>(keys2, vals2, nhe, ck, parent);
            },
            [&](uint32_t* parent, int32_t* rflag) { mo_flatten_kernel<<<ms_blocks(n), 256, 0, st>>>(d_tris, n, parent, info, rflag); }, st);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double* r = ref_point;
    ms_ref_point(h_small, n_verts, r);
    const int64_t np = (int64_t)h_small[MO_NPATCHES], ncol = (int64_t)h_small[MO_COLLAPSED], nvalid = n - ncol;
    if (n > 0) {
        const int64_t nblk = (nvalid + MS_BLOCK - 1) / MS_BLOCK;
        ENSURE(w.seg, sizeof(int64_t) * (size_t)(np + 1));
        ENSURE(w.partial, sizeof(double) * (size_t)(nblk + np + 1));
        ENSURE(w.counts, sizeof(int64_t) * MO_NCNT * (size_t)std::max<int64_t>(np, 1));
        ENSURE(w.vol, sizeof(double) * (size_t)std::max<int64_t>(np, 1));
        ENSURE(w.gflag, sizeof(int32_t) * (size_t)std::max<int64_t>(np, 1));
        int64_t* counts = w.counts.as<int64_t>();
        const uint32_t* info = w.info.as<uint32_t>();
        const int32_t* patch = w.patch.as<int32_t>();
        if (np > 0) {
            HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * MO_NCNT * (size_t)np, st));
            uint32_t *skey2 = w.skey2.as<uint32_t>(), *sval2 = w.sval2.as<uint32_t>();
            rc = ms_sum_by_group<MO_NCNT, 1>(
                w.temp, 0, n, nvalid, np, w.skey.as<uint32_t>(), skey2, w.sval.as<uint32_t>(), sval2, w.seg.as<int64_t>(),
                w.partial.as<double>(), w.vol.as<double>(), counts, MO_NTRIS,
                [&](unsigned blocks) {
                    mo_sum_kernel<<<blocks, MS_BLOCK, 0, st>>>(d_verts, d_tris, info, skey2, sval2, nvalid, r[0], r[1], r[2],
                                                               w.partial.as<double>());
                },
                st);
            if (rc) return rc;
            mo_parity_kernel<<<ms_blocks(n), 256, 0, st>>>(n, info, patch, counts);
            HIP_TRY(hipGetLastError());
            // (keys2 / vals2 still hold the sorted half-edges)
            mo_edge_kernel<<<ms_blocks(nh), 256, 0, st>>>(w.keys2.as<uint64_t>(), w.vals2.as<uint32_t>(), nh, ckey, patch, counts);
            HIP_TRY(hipGetLastError());
            mo_decide_kernel<<<ms_blocks(np), 256, 0, st>>>(np, flags, info, counts, w.vol.as<double>(), w.gflag.as<int32_t>(), small);
            HIP_TRY(hipGetLastError());
        }
        mo_apply_kernel<<<ms_blocks(n), 256, 0, st>>>(d_tris, n, info, patch, w.gflag.as<int32_t>(), d_tris_out, w.flip.as<int32_t>());
        HIP_TRY(hipGetLastError());
        if (np > 0) {
            mo_remain_kernel<<<ms_blocks(nh), 256, 0, st>>>(w.keys2.as<uint64_t>(), w.vals2.as<uint32_t>(), nh, ckey, w.flip.as<int32_t>(), small);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_patches = np;
    totals[0] = np, totals[1] = n, totals[2] = ncol;
    for (int k = 0; k < 5; ++k) totals[3 + k] = np > 0 ? (int64_t)h_small[MO_TOT + k] : 0;
    return 0;
}

int orient_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, int32_t flags, const void* tris_out,
                const int64_t* n_patches, const double* ref_point, const int64_t* totals)
{
    const int rc = mesh_args("mesh_orient", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (n_tris > MO_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_orient: %lld triangles exceed 2^30", (long long)n_tris);
    if (flags & ~MO_FLAGS) return fail(R2S_ERR_ARG, "mesh_orient: unknown flag bits in %d", (int)flags);
    if (n_tris > 0 && !tris_out) return fail(R2S_ERR_ARG, "mesh_orient: null tris_out");
    if (!n_patches || !ref_point || !totals) return fail(R2S_ERR_ARG, "mesh_orient: null n_patches / ref_point / totals");
    return 0;
}

// One call for both kinds of caller: the core, then the triangles, flip, patch_of_tri, the tables and the scalars.  A host
// caller's tables are kept whole for r2s_last_mesh_orient; a device caller gets them when patch_capacity holds all of them.
int orient_run(MeshCall<OrientWork>& c, int64_t n_verts, int64_t n_tris, int32_t flags, int32_t* tris_out, int32_t* flip_out,
               int32_t* patch_of_tri, int64_t* d_counts, double* d_volume, int64_t patch_capacity, int64_t* n_patches, double ref_point[3],
               int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    OrientWork& w = c.work();
    OrientTables tab;
    int64_t np = 0, tot[8];
    double r[3];
    int32_t* d_tris_out = nullptr;
    if ((rc = c.staged(w.tris_out, tris_out, tri_bytes(std::max<int64_t>(n_tris, 1)), d_tris_out)) ||
        (rc = orient_core(c.d_verts(), n_verts, c.d_tris(), n_tris, flags, c.stream(), w, d_tris_out, &np, r, tot)))
        return rc;
    const bool fits = patch_capacity >= np;
    if ((rc = c.table(tab.counts, d_counts, fits, w.counts, (size_t)np * MO_NCNT)) || (rc = c.table(tab.volume, d_volume, fits, w.vol, (size_t)np)) ||
        (rc = c.deliver(tris_out, d_tris_out, tri_bytes(n_tris))) || (rc = c.deliver(flip_out, w.flip.p, sizeof(int32_t) * (size_t)n_tris)) ||
        (rc = c.deliver(patch_of_tri, w.patch.p, sizeof(int32_t) * (size_t)n_tris)) || (rc = c.finish()))
        return rc;
    if (c.is_host()) g_last_orient = std::move(tab);
    *n_patches = np;
    std::memcpy(ref_point, r, sizeof r);
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_orient(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t flags, int32_t device,
                    int32_t* tris_out, int32_t* flip_out, int32_t* patch_of_tri_out, int64_t* n_patches, double ref_point[3],
                    int64_t totals[8])
{
    if (const int rc = orient_args(verts, n_verts, tris, n_tris, flags, tris_out, n_patches, ref_point, totals)) return rc;
    MeshCall<OrientWork> call("mesh_orient", g_orient_work, verts, n_verts, tris, n_tris, device);
    return orient_run(call, n_verts, n_tris, flags, tris_out, flip_out, patch_of_tri_out, nullptr, nullptr, 0, n_patches, ref_point, totals);
}

int r2s_last_mesh_orient(int64_t* counts_out, double* volume_out, int64_t capacity, int64_t* n_patches)
{
    if (!n_patches || capacity < 0 || (capacity > 0 && (!counts_out || !volume_out)))
        return fail(R2S_ERR_ARG, "last_mesh_orient: null output or negative capacity");
    const int64_t n = *n_patches = (int64_t)g_last_orient.volume.size();
    copy_rows(counts_out, g_last_orient.counts, MO_NCNT, capacity, n);
    copy_rows(volume_out, g_last_orient.volume, 1, capacity, n);
    return 0;
}

int r2s_mesh_orient_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, int32_t flags, int32_t* d_tris_out,
                        int32_t* d_flip_out, int32_t* d_patch_of_tri, int64_t* d_counts, double* d_volume, int64_t patch_capacity,
                        int64_t* n_patches, double ref_point[3], int64_t totals[8], void* stream)
{
    if (const int rc = orient_args(d_verts, n_verts, d_tris, n_tris, flags, d_tris_out, n_patches, ref_point, totals)) return rc;
    if (patch_capacity < 0 || (patch_capacity > 0 && (!d_counts || !d_volume)))
        return fail(R2S_ERR_ARG, "mesh_orient: null tables or negative patch_capacity");
    MeshCall<OrientWork> call("mesh_orient", g_orient_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return orient_run(call, n_verts, n_tris, flags, d_tris_out, d_flip_out, d_patch_of_tri, d_counts, d_volume, patch_capacity, n_patches,
                      ref_point, totals);
}

}  // extern "C"
