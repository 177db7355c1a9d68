// Mesh shells: the connected components of a triangle mesh over shared edges, the edge classes, and per shell the integer
// record and the Float64 area / volume / moments (include/rho2sdf_hip.h, r2s_mesh_shells; DESIGN.md "Mesh shells").
//   ms_bounds_kernel   the box of all vertices (integer atomics on order-preserving bit patterns) -> the reference point
//   ms_sort_half_edges (r2s_mesh_graph.hpp) ms_key_kernel<1, true>: one half-edge key per corner, (min << 33) | (max << 1) |
//                      direction, payload 3t + c, parent[t] = t, the referenced-vertex flags; collapsed triangles get a key
//                      above every real one -> rocPRIM radix sort of pairs
//   ms_union_kernel    one union per run member with the member before it (integer union-find: the larger root is hooked
//                      under the smaller with a compare-and-swap, paths are halved with atomicMin, so the final root of a
//                      component is its smallest triangle whatever the race)
//   ms_flatten_kernel<true> (r2s_mesh_graph.hpp) parent = root, root flags -> rocPRIM exclusive scan (integers) ->
//                      ms_number_kernel<false, true> (r2s_mesh_graph.hpp): shell numbers, the sort pairs
//   -> stable radix sort of the triangle ids by shell number -> ms_segment_kernel (r2s_mesh_graph.hpp): where each shell starts
//   ms_sum_kernel      blocks of 256 consecutive sorted triangles, the 11 terms per triangle -> ms_block_sum<11>
//                      (r2s_mesh_graph.hpp): a segmented fixed tree in LDS, one partial per (block, shell) at slot block + shell
//   ms_combine_kernel<11> (r2s_mesh_graph.hpp) one wavefront per shell: up to 64 equal runs of its block partials in ascending
//                      order, then a fixed tree; n_tris of the shell
//   ms_edge_kernel     the sorted edge runs again: class of each run (ms_run_class), counted into the shell of its first half-edge
//   ms_vkey_kernel     (shell << 32) | vertex per corner -> radix sort of keys -> ms_vcount_kernel: distinct vertices per shell
//   ms_totals_kernel   the column sums of the integer table and the number of referenced vertices
// Integer counts use integer atomics (a workgroup whose entries all fall into one shell adds once per column); no
// floating-point atomic and no library reduction touches the Float64 sums.
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

constexpr int MS_NSUM = 11, MS_NCNT = 8;
constexpr int64_t MS_MAX_TRIS = (int64_t)1 << 30;
// slots of the small device array: [0..5] the bounds, then
constexpr int MS_COLLAPSED = 6, MS_NSHELLS = 7, MS_TOT = 8;   // [MS_TOT .. MS_TOT + 4]: edges, boundary, flipped, non-manifold, vertices
constexpr int MS_SMALL = 16;

// one thread per sorted half-edge: joins its triangle to that of the member before it in the same run
__global__ void __launch_bounds__(256) ms_union_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                        uint64_t ckey, uint32_t* parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= nh) return;
    const uint64_t k = keys[i];
    if (k >= ckey || (keys[i - 1] >> 1) != (k >> 1)) return;
    ms_union(parent, vals[i - 1] / 3u, vals[i] / 3u);
}

// the 11 terms of one triangle in the header's operation order
__device__ inline void ms_terms(const float* __restrict__ verts, int32_t i0, int32_t i1, int32_t i2, double rx, double ry, double rz, double v[MS_NSUM])
{
#pragma clang fp contract(off)
    const float *pa = verts + 3 * (int64_t)i0, *pb = verts + 3 * (int64_t)i1, *pc = verts + 3 * (int64_t)i2;
    const double Ax = (double)pa[0] - rx, Ay = (double)pa[1] - ry, Az = (double)pa[2] - rz;
    const double Bx = (double)pb[0] - rx, By = (double)pb[1] - ry, Bz = (double)pb[2] - rz;
    const double Cx = (double)pc[0] - rx, Cy = (double)pc[1] - ry, Cz = (double)pc[2] - rz;
    const double Sx = (Ax + Bx) + Cx, Sy = (Ay + By) + Cy, Sz = (Az + Bz) + Cz;
    const double Ex = Bx - Ax, Ey = By - Ay, Ez = Bz - Az, Fx = Cx - Ax, Fy = Cy - Ay, Fz = Cz - Az;
    const double Nx = Ey * Fz - Ez * Fy, Ny = Ez * Fx - Ex * Fz, Nz = Ex * Fy - Ey * Fx;
    v[0] = 0.5 * sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
    const double det = (Ax * (By * Cz - Bz * Cy) + Ay * (Bz * Cx - Bx * Cz)) + Az * (Bx * Cy - By * Cx);
    v[1] = det / 6.0;
    v[2] = (det * Sx) / 24.0;
    v[3] = (det * Sy) / 24.0;
    v[4] = (det * Sz) / 24.0;
    v[5] = (det * (((Ax * Ax + Bx * Bx) + Cx * Cx) + Sx * Sx)) / 120.0;
    v[6] = (det * (((Ay * Ay + By * By) + Cy * Cy) + Sy * Sy)) / 120.0;
    v[7] = (det * (((Az * Az + Bz * Bz) + Cz * Cz) + Sz * Sz)) / 120.0;
    v[8] = (det * (((Ax * Ay + Bx * By) + Cx * Cy) + Sx * Sy)) / 120.0;
    v[9] = (det * (((Ax * Az + Bx * Bz) + Cx * Cz) + Sx * Sz)) / 120.0;
    v[10] = (det * (((Ay * Az + By * Bz) + Cy * Cz) + Sy * Sz)) / 120.0;
}

// one thread per sorted triangle: its 11 terms into the segmented sum of its block (ms_block_sum: slot block + shell)
__global__ void __launch_bounds__(MS_BLOCK) ms_sum_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           const uint32_t* __restrict__ skey, const uint32_t* __restrict__ stri, int64_t nvalid,
                                                           double rx, double ry, double rz, double* __restrict__ partial)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    const bool active = i < nvalid;
    uint32_t key = 0xffffffffu;
    double v[MS_NSUM];
#pragma unroll
    for (int q = 0; q < MS_NSUM; ++q) v[q] = 0.0;
    if (active) {
        key = skey[i];
        const int64_t t = (int64_t)stri[i];
        ms_terms(verts, tris[3 * t], tris[3 * t + 1], tris[3 * t + 2], rx, ry, rz, v);
    }
    ms_block_sum<MS_NSUM>(active, key, v, partial);
}

// one thread per sorted half-edge; the first member of a run classifies it and counts it into the shell of its triangle
__global__ void __launch_bounds__(256) ms_edge_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t nh,
                                                       uint64_t ckey, const int32_t* __restrict__ shell_of, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    bool add[4] = {false, false, false, false};   // edge, boundary, flipped, non-manifold
    int32_t shell = -1;
    if (i < nh) {
        const uint64_t k = keys[i];
        head = k < ckey && (i == 0 || (keys[i - 1] >> 1) != (k >> 1));
        if (head) {
            const int cls = ms_run_class(keys, i, nh);
            add[0] = true;
            add[1] = cls == MS_RUN_SINGLE;
            add[2] = cls == MS_RUN_SAME;
            add[3] = cls == MS_RUN_MANY;
            shell = shell_of[vals[i] / 3u];
        }
    }
    ms_count<4, MS_NCNT>(head, shell, add, 3, counts);
}

__global__ void __launch_bounds__(256) ms_vkey_kernel(const int32_t* __restrict__ tris, int64_t n, const int32_t* __restrict__ shell_of,
                                                       uint64_t nsh, uint64_t* __restrict__ vkeys)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int32_t s = shell_of[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) vkeys[3 * t + c] = s < 0 ? (nsh << 32) : (((uint64_t)(uint32_t)s << 32) | (uint64_t)(uint32_t)tris[3 * t + c]);
}

__global__ void __launch_bounds__(256) ms_vcount_kernel(const uint64_t* __restrict__ vkeys, int64_t nh, uint64_t nsh, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    int32_t shell = -1;
    if (i < nh) {
        const uint64_t k = vkeys[i];
        head = (k >> 32) < nsh && (i == 0 || vkeys[i - 1] != k);
        shell = (int32_t)(k >> 32);
    }
    const bool add[1] = {true};
    ms_count<1, MS_NCNT>(head, shell, add, 2, counts);
}

// small[MS_TOT + 0..3] = the sums of columns 3..6 over the shells, small[MS_TOT + 4] = the number of set vertex flags
__global__ void __launch_bounds__(256) ms_totals_kernel(const int64_t* __restrict__ counts, int64_t nsh, const int32_t* __restrict__ vflag,
                                                         int64_t nverts, uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    long long c[5] = {0, 0, 0, 0, 0};
    if (i < nsh) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = counts[i * MS_NCNT + 3 + k];
    }
    if (i < nverts) c[4] = vflag[i] ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c[k] += __shfl_xor(c[k], d, 64);
        if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd((unsigned long long*)&small[MS_TOT + k], (unsigned long long)c[k]);
    }
}

// work buffers of the shell calls, kept per device between calls (r2s_release_cache frees them)
struct ShellWork : MsHalfEdgeBufs {
    DevBuf verts, tris, flag, small, parent, rflag, num, shell, skey, skey2, sval, sval2, seg, partial, counts, sums, vflag;
};
PerDevice<ShellWork> g_shell_work;

struct ShellTables {
    std::vector<int64_t> counts;   // [n][8]
    std::vector<double> sums;      // [n][11]
};
thread_local ShellTables g_last_shells;

// The shells of the device mesh on the current device, after the work queued on `st`; synchronous.  Leaves shell_of_tri in
// w.shell [n_tris] and the tables in w.counts / w.sums [n_shells]; the scalars go to the host pointers.
int shells_core(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n, hipStream_t st, ShellWork& w, int64_t* n_shells,
                double ref_point[3], int64_t totals[8])
{
    uint64_t h_small[MS_SMALL];
    int rc = ms_begin_small(w.small, h_small, d_verts, n_verts, st);
    if (rc) return rc;
    uint64_t* small = w.small.as<uint64_t>();
    const int64_t nh = 3 * n;
    const uint64_t ckey = ms_collapsed_key(n_verts);
    if (n > 0) {
        ENSURE(w.skey2, sizeof(uint32_t) * (size_t)n);
        ENSURE(w.sval2, sizeof(uint32_t) * (size_t)n);
        ENSURE(w.vflag, sizeof(int32_t) * (size_t)std::max<int64_t>(n_verts, 1));
        HIP_TRY(hipMemsetAsync(w.vflag.p, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(n_verts, 1), st));
        rc = ms_group_triangles<1, true, false, true>(
            w, d_tris, n, n_verts, w.parent, w.vflag.as<int32_t>(), nullptr, w.rflag, w.num, w.shell, &w.skey, &w.sval, small + MS_COLLAPSED,
            small + MS_NSHELLS,
            [&](const uint64_t* keys2, const uint32_t* vals2, int64_t nhe, uint64_t ck, uint32_t* parent) {
                ms_union_kernel<<<ms_blocks(nhe), 256, 0, st>>>(keys2, vals2, nhe, ck, parent);
            },
            [&](uint32_t* parent, int32_t* rflag) { ms_flatten_kernel<true><<<ms_blocks(n), 256, 0, st>>>(d_tris, n, parent, rflag); }, st);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double* r = ref_point;
    ms_ref_point(h_small, n_verts, r);
    const int64_t nsh = (int64_t)h_small[MS_NSHELLS], ncol = (int64_t)h_small[MS_COLLAPSED], nvalid = n - ncol;
    if (nsh > 0) {
        const int64_t nblk = (nvalid + MS_BLOCK - 1) / MS_BLOCK;
        ENSURE(w.seg, sizeof(int64_t) * (size_t)(nsh + 1));
        ENSURE(w.partial, sizeof(double) * MS_NSUM * (size_t)(nblk + nsh));
        ENSURE(w.counts, sizeof(int64_t) * MS_NCNT * (size_t)nsh);
        ENSURE(w.sums, sizeof(double) * MS_NSUM * (size_t)nsh);
        int64_t* counts = w.counts.as<int64_t>();
        HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * MS_NCNT * (size_t)nsh, st));
        uint32_t *skey2 = w.skey2.as<uint32_t>(), *sval2 = w.sval2.as<uint32_t>();
        size_t tb2 = 0;
        const unsigned vbits = 32u + ms_bits((uint64_t)nsh);
        uint64_t *keys = w.keys.as<uint64_t>(), *keys2 = w.keys2.as<uint64_t>();
        // (the vertex-key sort below shares temp with the sort by shell)
        HIP_TRY(rocprim::radix_sort_keys(nullptr, tb2, keys, keys2, (size_t)nh, 0u, vbits, st));
        rc = ms_sum_by_group<MS_NCNT, MS_NSUM>(
            w.temp, tb2, n, nvalid, nsh, w.skey.as<uint32_t>(), skey2, w.sval.as<uint32_t>(), sval2, w.seg.as<int64_t>(),
            w.partial.as<double>(), w.sums.as<double>(), counts, 1,
            [&](unsigned blocks) {
                ms_sum_kernel<<<blocks, MS_BLOCK, 0, st>>>(d_verts, d_tris, skey2, sval2, nvalid, r[0], r[1], r[2], w.partial.as<double>());
            },
            st);
        if (rc) return rc;
        // (keys2 / vals2 still hold the sorted half-edges)
        ms_edge_kernel<<<ms_blocks(nh), 256, 0, st>>>(keys2, w.vals2.as<uint32_t>(), nh, ckey, w.shell.as<int32_t>(), counts);
        HIP_TRY(hipGetLastError());
        ms_vkey_kernel<<<ms_blocks(n), 256, 0, st>>>(d_tris, n, w.shell.as<int32_t>(), (uint64_t)nsh, keys);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_keys(w.temp.p, tb2, keys, keys2, (size_t)nh, 0u, vbits, st));
        ms_vcount_kernel<<<ms_blocks(nh), 256, 0, st>>>(keys2, nh, (uint64_t)nsh, counts);
        HIP_TRY(hipGetLastError());
        ms_totals_kernel<<<ms_blocks(std::max(nsh, n_verts)), 256, 0, st>>>(counts, nsh, w.vflag.as<int32_t>(), n_verts, small);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_shells = nsh;
    totals[0] = nsh, totals[1] = n, totals[2] = ncol;
    for (int k = 0; k < 5; ++k) totals[3 + k] = nsh > 0 ? (int64_t)h_small[MS_TOT + k] : 0;
    return 0;
}

int shells_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, const int64_t* n_shells, const double* ref_point,
                const int64_t* totals)
{
    const int rc = mesh_args("mesh_shells", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (n_tris > MS_MAX_TRIS) return fail(R2S_ERR_UNSUPPORTED, "mesh_shells: %lld triangles exceed 2^30", (long long)n_tris);
    if (!n_shells || !ref_point || !totals) return fail(R2S_ERR_ARG, "mesh_shells: null n_shells / ref_point / totals");
    return 0;
}

// One call for both kinds of caller: the core, then shell_of_tri, the tables and the scalars.  A host caller's tables are kept
// whole for r2s_last_mesh_shells; a device caller gets them when shell_capacity holds all of them, else none.
int shells_run(MeshCall<ShellWork>& c, int64_t n_verts, int64_t n_tris, int32_t* shell_of_tri, int64_t* d_counts, double* d_sums,
               int64_t shell_capacity, int64_t* n_shells, double ref_point[3], int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    ShellWork& w = c.work();
    ShellTables tab;
    int64_t nsh = 0, tot[8];
    double r[3];
    if ((rc = shells_core(c.d_verts(), n_verts, c.d_tris(), n_tris, c.stream(), w, &nsh, r, tot))) return rc;
    const bool fits = shell_capacity >= nsh;
    if ((rc = c.table(tab.counts, d_counts, fits, w.counts, (size_t)nsh * MS_NCNT)) ||
        (rc = c.table(tab.sums, d_sums, fits, w.sums, (size_t)nsh * MS_NSUM)) ||
        (rc = c.deliver(shell_of_tri, w.shell.p, sizeof(int32_t) * (size_t)n_tris)) || (rc = c.finish()))
        return rc;
    if (c.is_host()) g_last_shells = std::move(tab);
    *n_shells = nsh;
    std::memcpy(ref_point, r, sizeof r);
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_shells(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device, int32_t* shell_of_tri_out,
                    int64_t* n_shells, double ref_point[3], int64_t totals[8])
{
    if (const int rc = shells_args(verts, n_verts, tris, n_tris, n_shells, ref_point, totals)) return rc;
    MeshCall<ShellWork> call("mesh_shells", g_shell_work, verts, n_verts, tris, n_tris, device);
    return shells_run(call, n_verts, n_tris, shell_of_tri_out, nullptr, nullptr, 0, n_shells, ref_point, totals);
}

int r2s_last_mesh_shells(int64_t* counts_out, double* sums_out, int64_t capacity, int64_t* n_shells)
{
    if (!n_shells || capacity < 0 || (capacity > 0 && (!counts_out || !sums_out)))
        return fail(R2S_ERR_ARG, "last_mesh_shells: null output or negative capacity");
    const int64_t n = *n_shells = (int64_t)(g_last_shells.counts.size() / MS_NCNT);
    copy_rows(counts_out, g_last_shells.counts, MS_NCNT, capacity, n);
    copy_rows(sums_out, g_last_shells.sums, MS_NSUM, capacity, n);
    return 0;
}

int r2s_mesh_shells_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, int32_t* d_shell_of_tri,
                        int64_t* d_counts, double* d_sums, int64_t shell_capacity, int64_t* n_shells, double ref_point[3],
                        int64_t totals[8], void* stream)
{
    if (const int rc = shells_args(d_verts, n_verts, d_tris, n_tris, n_shells, ref_point, totals)) return rc;
    if (shell_capacity < 0 || (shell_capacity > 0 && (!d_counts || !d_sums)))
        return fail(R2S_ERR_ARG, "mesh_shells: null tables or negative shell_capacity");
    MeshCall<ShellWork> call("mesh_shells", g_shell_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return shells_run(call, n_verts, n_tris, d_shell_of_tri, d_counts, d_sums, shell_capacity, n_shells, ref_point, totals);
}

}  // extern "C"
