// Mesh simplify: vertex-clustering decimation (include/rho2sdf_hip.h, r2s_mesh_simplify; DESIGN.md "Mesh simplify").  The cells
// and classes are the weld's (r2s_mesh_weld.hpp: mw_classes, mw_triangles); what is new is the representative of a class: the
// Float64 mean of its members, or the point that minimises the summed plane quadrics of the triangles around it.
//   sm_member_kernel   one thread per triangle: the corners of a non-collapsed INPUT triangle are members
//   sm_first_kernel    one thread per vertex: first[c] = the smallest member index of class c (integer atomicMin: the result does
//                      not depend on the arrival order), the member count
//   sm_flag_kernel     the first member of every class a surviving triangle references -> rocPRIM exclusive scan: the output
//                      numbers, in first-occurrence order of the first member
//   sm_vmap_kernel     vert_map, and the items (output class, vertex) of the mean sum;  mw_tout_kernel  tri_map, tris_out
//   sm_qkey_kernel     the items (output class, triangle) of the quadric sum: one per DISTINCT class among the corners of a
//                      non-collapsed input triangle, written in triangle order
//   -> ms_sum_by_group twice (stable radix sort by class, segment starts, block sums, combine):
//      sm_mean_terms_kernel    ms_block_sum<3>:  the member's coordinates about ref_point
//      sm_quadric_terms_kernel ms_block_sum<10>: n n^T (6), d n (3), d^2 of the triangle's plane
//   sm_solve_kernel    one thread per output class: the mean, the cyclic Jacobi of the 3x3 quadric matrix, the truncated
//                      pseudo-inverse step from the mean, the pull-back to the closed cell, ONE rounding to float32, and the quadric
//                      error at the rounded point
// The 13 Float64 columns are summed as 3 + 10 because they have different items (members against (class, triangle) pairs); each
// column's additions are in the order the header defines either way.  No fma anywhere: the file is built with -ffp-contract=off
// and the arithmetic kernels say so again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_graph.hpp"
#include "r2s_mesh_weld.hpp"

using namespace r2s_int;

namespace {

// slots of the small device array behind the six of the box (ms_begin_small)
constexpr int SM_MEMBERS = 6, SM_NOUT = 7, SM_VITEMS = 8, SM_QITEMS = 9, SM_PULLED = 10, SM_SMALL = 12;
constexpr int SM_NCNT = 2;   // rows of the per-class counts: [0] the first member, [1] the number of members
constexpr int SM_NQ = 10;    // columns of the quadric sum
constexpr double SM_TINY_STEP = 0x1p-40;   // in cells: below this a step component is rounding noise and is not pulled back

__global__ void __launch_bounds__(256) sm_member_kernel(const int32_t* __restrict__ tris, int64_t nt, int32_t* __restrict__ member)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int32_t i0, i1, i2;
    if (!ms_collapsed(tris, t, i0, i1, i2)) member[i0] = member[i1] = member[i2] = 1;
}

__global__ void __launch_bounds__(256) sm_first_kernel(const int32_t* __restrict__ member, const int32_t* __restrict__ class_of, int64_t nv,
                                                        int32_t* __restrict__ first, uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool m = i < nv && member[i];
    if (m) atomicMin(&first[class_of[i]], (int32_t)i);
    mw_count(m, small, SM_MEMBERS);
}

__global__ void __launch_bounds__(256) sm_flag_kernel(const int32_t* __restrict__ member, const int32_t* __restrict__ class_of,
                                                       const int32_t* __restrict__ used, const int32_t* __restrict__ first, int64_t nv,
                                                       int32_t* __restrict__ fflag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int32_t c = class_of[i];
    fflag[i] = (member[i] && used[c] && first[c] == (int32_t)i) ? 1 : 0;
}

// fnum = the exclusive scan of fflag: the output number of a class is fnum[first member]
__global__ void __launch_bounds__(256) sm_vmap_kernel(const int32_t* __restrict__ member, const int32_t* __restrict__ class_of,
                                                       const int32_t* __restrict__ used, const int32_t* __restrict__ first,
                                                       const int32_t* __restrict__ fnum, const int32_t* __restrict__ fflag, int64_t nv,
                                                       int32_t* __restrict__ vert_map, uint32_t* __restrict__ vkey, uint32_t* __restrict__ vval,
                                                       uint64_t* __restrict__ small)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t nout = fnum[nv - 1] + fflag[nv - 1];
    int32_t f = -1;
    if (i < nv) {
        const int32_t c = class_of[i];
        if (member[i] && used[c]) f = fnum[first[c]];
        vert_map[i] = f;
        vkey[i] = f < 0 ? (uint32_t)nout : (uint32_t)f;   // (what is in no output class sorts behind every segment)
        vval[i] = (uint32_t)i;
        if (i == nv - 1) small[SM_NOUT] = (uint64_t)nout;
    }
    mw_count(f >= 0, small, SM_VITEMS);
}

__global__ void __launch_bounds__(256) sm_qkey_kernel(const int32_t* __restrict__ tris, int64_t nt, const int32_t* __restrict__ vert_map,
                                                       const int32_t* __restrict__ fnum, const int32_t* __restrict__ fflag, int64_t nv,
                                                       uint32_t* __restrict__ qkey, uint32_t* __restrict__ qval, uint64_t* __restrict__ small)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t nout = (uint32_t)(fnum[nv - 1] + fflag[nv - 1]);
    bool item[3] = {false, false, false};
    if (t < nt) {
        int32_t i[3];
        const bool col = ms_collapsed(tris, t, i[0], i[1], i[2]);
        int32_t f[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) f[k] = col ? -1 : vert_map[i[k]];
        item[0] = f[0] >= 0;
        item[1] = f[1] >= 0 && f[1] != f[0];
        item[2] = f[2] >= 0 && f[2] != f[0] && f[2] != f[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            qkey[3 * t + k] = item[k] ? (uint32_t)f[k] : nout;
            qval[3 * t + k] = (uint32_t)t;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) mw_count(item[k], small, SM_QITEMS);
}

__global__ void __launch_bounds__(256) sm_mean_terms_kernel(const float* __restrict__ verts, const uint32_t* __restrict__ skey,
                                                             const uint32_t* __restrict__ sval, int64_t nvalid, double r0, double r1, double r2,
                                                             double* __restrict__ partial)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = p < nvalid;
    double v[3] = {0.0, 0.0, 0.0};
    uint32_t key = 0u;
    if (active) {
        key = skey[p];
        const int64_t i = (int64_t)sval[p];
        v[0] = (double)verts[3 * i] - r0;
        v[1] = (double)verts[3 * i + 1] - r1;
        v[2] = (double)verts[3 * i + 2] - r2;
    }
    ms_block_sum<3>(active, key, v, partial);
}

__global__ void __launch_bounds__(256) sm_quadric_terms_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                                const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval,
                                                                int64_t nvalid, double r0, double r1, double r2, double* __restrict__ partial)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = p < nvalid;
    double v[SM_NQ];
#pragma unroll
    for (int q = 0; q < SM_NQ; ++q) v[q] = 0.0;
    uint32_t key = 0u;
    if (active) {
        key = skey[p];
        const int64_t t = (int64_t)sval[p];
        const double r[3] = {r0, r1, r2};
        double a[3], e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = (double)verts[3 * (int64_t)tris[3 * t] + k] - r[k];
            e1[k] = ((double)verts[3 * (int64_t)tris[3 * t + 1] + k] - r[k]) - a[k];
            e2[k] = ((double)verts[3 * (int64_t)tris[3 * t + 2] + k] - r[k]) - a[k];
        }
        const double n0 = e1[1] * e2[2] - e1[2] * e2[1];
        const double n1 = e1[2] * e2[0] - e1[0] * e2[2];
        const double n2 = e1[0] * e2[1] - e1[1] * e2[0];
        const double d = (n0 * a[0] + n1 * a[1]) + n2 * a[2];
        v[0] = n0 * n0, v[1] = n0 * n1, v[2] = n0 * n2, v[3] = n1 * n1, v[4] = n1 * n2, v[5] = n2 * n2;
        v[6] = d * n0, v[7] = d * n1, v[8] = d * n2, v[9] = d * d;
    }
    ms_block_sum<SM_NQ>(active, key, v, partial);
}

// cyclic Jacobi on a symmetric 3x3, the scheme of jacobi4 (r2s_pre.hip): sweeps over (0,1), (0,2), (1,2) until the off-diagonal
// sum of squares is exactly 0 (100 sweeps at most); w = the diagonal, the columns of V the eigenvectors.  Fully unrolled: every
// index is a constant, nothing goes to scratch.
__device__ inline void sm_jacobi3(double A[3][3], double w[3], double V[3][3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        const double off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2];
        if (off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double t = ((theta >= 0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = cs * akp - sn * akq;
                        A[k][q] = sn * akp + cs * akq;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double apk = A[p][k], aqk = A[q][k];
                        A[p][k] = cs * apk - sn * aqk;
                        A[q][k] = sn * apk + cs * aqk;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = cs * vkp - sn * vkq;
                        V[k][q] = sn * vkp + cs * vkq;
                    }
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = A[i][i];
}

// one thread per output class; counts [n][SM_NCNT], mean [n][3] and quad [n][SM_NQ] are the combined sums
__global__ void __launch_bounds__(256) sm_solve_kernel(const float* __restrict__ verts, int64_t nout, const int64_t* __restrict__ counts,
                                                        const double* __restrict__ mean, const double* __restrict__ quad, double cell,
                                                        int32_t rule, double r0, double r1, double r2, float* __restrict__ verts_out,
                                                        int64_t* __restrict__ members, double* __restrict__ error, int32_t* __restrict__ solved,
                                                        uint64_t* __restrict__ small)
{
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool pulled = false;
    if (c < nout) {
        const double r[3] = {r0, r1, r2};
        const int64_t v0 = counts[c * SM_NCNT], n = counts[c * SM_NCNT + 1];
        double m[3], x[3], lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            m[k] = mean[3 * c + k] / (double)n;
            x[k] = m[k];
            const double q = mw_cell(verts[3 * v0 + k], cell);
            lo[k] = q * cell - r[k];
            hi[k] = (q + 1.0) * cell - r[k];
        }
        const double* Q = quad + c * SM_NQ;
        const double S[3][3] = {{Q[0], Q[1], Q[2]}, {Q[1], Q[3], Q[4]}, {Q[2], Q[4], Q[5]}};
        const double b[3] = {Q[6], Q[7], Q[8]};
        int32_t code = 0;
        if (rule == R2S_SIMPLIFY_QUADRIC) {
            double A[3][3], w[3], V[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) A[i][j] = S[i][j];
            sm_jacobi3(A, w, V);
            const double wmax = fmax(fmax(w[0], w[1]), w[2]);
            if (wmax > 0.0) {
                double g[3];   // b - S m
#pragma unroll
                for (int k = 0; k < 3; ++k) g[k] = b[k] - ((S[k][0] * m[0] + S[k][1] * m[1]) + S[k][2] * m[2]);
                const double cut = 1e-3 * wmax;
                double step[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    if (!(w[e] < cut)) {
                        const double a = ((V[0][e] * g[0] + V[1][e] * g[1]) + V[2][e] * g[2]) / w[e];
#pragma unroll
                        for (int k = 0; k < 3; ++k) step[k] = step[k] + a * V[k][e];
                        ++code;
                    }
                }
                double s = 1.0;
                const double tiny = SM_TINY_STEP * cell;   // (an axis the step does not really move along constrains nothing)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double xk = m[k] + step[k];
                    if (step[k] > tiny && xk > hi[k]) s = fmin(s, (hi[k] - m[k]) / step[k]);
                    if (step[k] < -tiny && xk < lo[k]) s = fmin(s, (lo[k] - m[k]) / step[k]);
                }
                s = s < 0.0 ? 0.0 : s;
                pulled = s < 1.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) x[k] = pulled ? m[k] + s * step[k] : m[k] + step[k];
                if (pulled) code += 4;
            }
        }
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float o = (float)(x[k] + r[k]);   // (the one rounding to float32)
            verts_out[3 * c + k] = o;
            p[k] = (double)o - r[k];
        }
        double Sp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) Sp[k] = (S[k][0] * p[0] + S[k][1] * p[1]) + S[k][2] * p[2];
        const double quadratic = (p[0] * Sp[0] + p[1] * Sp[1]) + p[2] * Sp[2];
        const double linear = (b[0] * p[0] + b[1] * p[1]) + b[2] * p[2];
        error[c] = (quadratic - 2.0 * linear) + Q[9];
        members[c] = n;
        solved[c] = code;
    }
    mw_count(pulled, small, SM_PULLED);
}

// work buffers of the simplify calls, kept per device between calls (r2s_release_cache frees them)
struct SimplifyWork : MwBufs {
    DevBuf verts, tris, verts_out, tris_out, flag, box, member, first, fflag, fnum, vkey, vval, qkey, qval, skey2, sval2, seg, counts, counts_q,
        partial, mean, quad, members, error, solved;
};
PerDevice<SimplifyWork> g_simplify_work;

// the calling thread's last tables (r2s_last_mesh_simplify)
struct SimplifyTables {
    std::vector<int64_t> members;
    std::vector<double> error;
    std::vector<int32_t> solved;
};
thread_local SimplifyTables g_last_simplify;

// The simplified device mesh on the current device, after the work queued on `st`; synchronous.  Nothing is written to
// d_verts_out / d_tris_out before the cell range check has passed.  Leaves vert_map in w.vert_map [n_verts], tri_map in w.tri_map
// [n_tris] and the three tables in w.members / w.error / w.solved [totals[0]].
int simplify_core(const float* d_verts, int64_t nv, const int32_t* d_tris, int64_t nt, double cell, int32_t rule, int32_t flags, hipStream_t st,
                  SimplifyWork& w, float* d_verts_out, int32_t* d_tris_out, int64_t totals[8])
{
    for (int k = 0; k < 8; ++k) totals[k] = 0;
    if (nv == 0) return 0;   // (no vertex: no valid triangle either)
    int64_t ncls = 0;
    int rc = mw_classes(w, "mesh_simplify", d_verts, nv, nt, cell, st, &ncls);
    if (rc) return rc;
    uint64_t h_small[SM_SMALL];
    if ((rc = ms_begin_small(w.box, h_small, d_verts, nv, st))) return rc;
    uint64_t* small = w.box.as<uint64_t>();
    if ((rc = mw_triangles(w, d_tris, nt, ncls, flags | R2S_WELD_DROP_COLLAPSED, st))) return rc;
    ENSURE(w.member, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.fflag, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.fnum, sizeof(int32_t) * (size_t)nv);
    ENSURE(w.vkey, sizeof(uint32_t) * (size_t)nv);
    ENSURE(w.vval, sizeof(uint32_t) * (size_t)nv);
    ENSURE(w.first, sizeof(int32_t) * (size_t)ncls);
    int32_t *member = w.member.as<int32_t>(), *first = w.first.as<int32_t>(), *fflag = w.fflag.as<int32_t>(), *fnum = w.fnum.as<int32_t>();
    int32_t *class_of = w.class_of.as<int32_t>(), *used = w.used.as<int32_t>(), *vert_map = w.vert_map.as<int32_t>();
    HIP_TRY(hipMemsetAsync(member, 0, sizeof(int32_t) * (size_t)nv, st));
    HIP_TRY(hipMemsetAsync(first, 0x7f, sizeof(int32_t) * (size_t)ncls, st));   // (0x7f7f7f7f; only the classes with a member are read, and atomicMin has put it there)
    if (nt > 0) {
        sm_member_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, nt, member);
        HIP_TRY(hipGetLastError());
    }
    sm_first_kernel<<<ms_blocks(nv), 256, 0, st>>>(member, class_of, nv, first, small);
    HIP_TRY(hipGetLastError());
    sm_flag_kernel<<<ms_blocks(nv), 256, 0, st>>>(member, class_of, used, first, nv, fflag);
    HIP_TRY(hipGetLastError());
    if ((rc = weld_scan(w, fflag, fnum, nv, st))) return rc;
    sm_vmap_kernel<<<ms_blocks(nv), 256, 0, st>>>(member, class_of, used, first, fnum, fflag, nv, vert_map, w.vkey.as<uint32_t>(),
                                                 w.vval.as<uint32_t>(), small);
    HIP_TRY(hipGetLastError());
    if (nt > 0) {
        ENSURE(w.qkey, sizeof(uint32_t) * 3 * (size_t)nt);
        ENSURE(w.qval, sizeof(uint32_t) * 3 * (size_t)nt);
        mw_tout_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, nt, vert_map, w.keep.as<int32_t>(), w.tnum.as<int32_t>(), w.tri_map.as<int32_t>(),
                                                     d_tris_out, w.small.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        sm_qkey_kernel<<<ms_blocks(nt), 256, 0, st>>>(d_tris, nt, vert_map, fnum, fflag, nv, w.qkey.as<uint32_t>(), w.qval.as<uint32_t>(), small);
        HIP_TRY(hipGetLastError());
    }
    uint64_t h_weld[MW_SMALL];
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_weld, w.small.p, sizeof h_weld, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t nout = (int64_t)h_small[SM_NOUT], n_members = (int64_t)h_small[SM_MEMBERS];
    const int64_t n_vitems = (int64_t)h_small[SM_VITEMS], n_qitems = (int64_t)h_small[SM_QITEMS];
    totals[0] = nout;
    totals[1] = (int64_t)h_weld[MW_TRIS_OUT];
    totals[2] = n_members - nout;
    totals[3] = (int64_t)h_weld[MW_COLLAPSED];
    totals[4] = (int64_t)h_weld[MW_DUPLICATES];
    totals[5] = (int64_t)h_weld[MW_OPPOSITE];
    totals[6] = nv - n_members;
    if (nout == 0) return 0;
    // every output class has a surviving triangle, so a member and a (class, triangle) item: no segment of either sum is empty
    double ref[3];
    ms_ref_point(h_small, nv, ref);
    const int64_t nitems = std::max(nv, 3 * nt);
    const int64_t blocks_v = (n_vitems + MS_BLOCK - 1) / MS_BLOCK, blocks_q = (n_qitems + MS_BLOCK - 1) / MS_BLOCK;
    ENSURE(w.skey2, sizeof(uint32_t) * (size_t)nitems);
    ENSURE(w.sval2, sizeof(uint32_t) * (size_t)nitems);
    ENSURE(w.seg, sizeof(int64_t) * (size_t)(nout + 1));
    ENSURE(w.counts, sizeof(int64_t) * SM_NCNT * (size_t)nout);
    ENSURE(w.counts_q, sizeof(int64_t) * SM_NCNT * (size_t)nout);
    ENSURE(w.partial, sizeof(double) * (size_t)std::max((blocks_v + nout) * 3, (blocks_q + nout) * SM_NQ));
    ENSURE(w.mean, sizeof(double) * 3 * (size_t)nout);
    ENSURE(w.quad, sizeof(double) * SM_NQ * (size_t)nout);
    ENSURE(w.members, sizeof(int64_t) * (size_t)nout);
    ENSURE(w.error, sizeof(double) * (size_t)nout);
    ENSURE(w.solved, sizeof(int32_t) * (size_t)nout);
    uint32_t *skey2 = w.skey2.as<uint32_t>(), *sval2 = w.sval2.as<uint32_t>();
    double* partial = w.partial.as<double>();
    rc = ms_sum_by_group<SM_NCNT, 3>(w.temp, 0, nv, n_vitems, nout, w.vkey.as<uint32_t>(), skey2, w.vval.as<uint32_t>(), sval2, w.seg.as<int64_t>(),
                                     partial, w.mean.as<double>(), w.counts.as<int64_t>(), 1, [&](unsigned blocks) {
                                         sm_mean_terms_kernel<<<blocks, 256, 0, st>>>(d_verts, skey2, sval2, n_vitems, ref[0], ref[1], ref[2], partial);
                                     }, st);
    if (rc) return rc;
    rc = ms_sum_by_group<SM_NCNT, SM_NQ>(w.temp, 0, 3 * nt, n_qitems, nout, w.qkey.as<uint32_t>(), skey2, w.qval.as<uint32_t>(), sval2,
                                         w.seg.as<int64_t>(), partial, w.quad.as<double>(), w.counts_q.as<int64_t>(), 1, [&](unsigned blocks) {
                                             sm_quadric_terms_kernel<<<blocks, 256, 0, st>>>(d_verts, d_tris, skey2, sval2, n_qitems, ref[0], ref[1],
                                                                                           ref[2], partial);
                                         }, st);
    if (rc) return rc;
    sm_solve_kernel<<<ms_blocks(nout), 256, 0, st>>>(d_verts, nout, w.counts.as<int64_t>(), w.mean.as<double>(), w.quad.as<double>(), cell, rule,
                                                    ref[0], ref[1], ref[2], d_verts_out, w.members.as<int64_t>(), w.error.as<double>(),
                                                    w.solved.as<int32_t>(), small);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_small, small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    totals[7] = (int64_t)h_small[SM_PULLED];
    return 0;
}

// the checks that need no device
int simplify_args(const void* verts, int64_t n_verts, const void* tris, int64_t n_tris, double cell, int32_t rule, int32_t flags,
                  const void* verts_out, const void* tris_out, const int64_t* totals)
{
    if (const int rc = mesh_args("mesh_simplify", verts, n_verts, tris, n_tris)) return rc;
    if (!tris && n_verts > 0)
        return fail(R2S_ERR_ARG, "mesh_simplify: tris == NULL; the input is an indexed mesh (weld a soup with r2s_mesh_weld, snap = 0, first)");
    if (3 * n_tris > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "mesh_simplify: %lld triangles exceed 2^31 / 3", (long long)n_tris);
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(R2S_ERR_ARG, "mesh_simplify: cell must be positive and finite");
    if (rule != R2S_SIMPLIFY_MEAN && rule != R2S_SIMPLIFY_QUADRIC) return fail(R2S_ERR_ARG, "mesh_simplify: unknown rule %d", (int)rule);
    if (flags & ~R2S_WELD_DROP_DUPLICATES) return fail(R2S_ERR_ARG, "mesh_simplify: unknown flag bits in %d", (int)flags);
    if (!totals || (n_verts > 0 && !verts_out) || (n_tris > 0 && !tris_out))
        return fail(R2S_ERR_ARG, "mesh_simplify: null verts_out / tris_out / totals");
    return 0;
}

// One call for both kinds of caller: the simplified mesh (a host caller's through work buffers, tot[0] vertices and tot[1] triangles
// of them copied out), vert_map, tri_map, the totals, and the three tables, kept whole for r2s_last_mesh_simplify.
int simplify_run(MeshCall<SimplifyWork>& c, int64_t n_verts, int64_t nt, double cell, int32_t rule, int32_t flags, float* verts_out,
                 int32_t* tris_out, int32_t* vert_map_out, int32_t* tri_map_out, int64_t totals[8])
{
    int rc = c.open();
    if (rc) return rc;
    SimplifyWork& w = c.work();
    int64_t tot[8];
    float* d_verts_out = nullptr;
    int32_t* d_tris_out = nullptr;
    if ((rc = c.staged(w.verts_out, verts_out, vert_bytes(std::max<int64_t>(n_verts, 1)), d_verts_out)) ||
        (rc = c.staged(w.tris_out, tris_out, tri_bytes(std::max<int64_t>(nt, 1)), d_tris_out)) ||
        (rc = simplify_core(c.d_verts(), n_verts, c.d_tris(), nt, cell, rule, flags, c.stream(), w, d_verts_out, d_tris_out, tot)))
        return rc;
    SimplifyTables tab;
    tab.members.resize((size_t)tot[0]);
    tab.error.resize((size_t)tot[0]);
    tab.solved.resize((size_t)tot[0]);
    if (tot[0] > 0) {   // (small tables, read back after the core's wait for both kinds of caller)
        HIP_TRY(hipMemcpy(tab.members.data(), w.members.p, sizeof(int64_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tab.error.data(), w.error.p, sizeof(double) * (size_t)tot[0], hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tab.solved.data(), w.solved.p, sizeof(int32_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
    }
    if ((rc = c.deliver(verts_out, d_verts_out, vert_bytes(tot[0]))) || (rc = c.deliver(tris_out, d_tris_out, tri_bytes(tot[1]))) ||
        (rc = c.deliver(vert_map_out, w.vert_map.p, sizeof(int32_t) * (size_t)n_verts)) ||
        (rc = c.deliver(tri_map_out, w.tri_map.p, sizeof(int32_t) * (size_t)nt)) || (rc = c.finish()))
        return rc;
    g_last_simplify = std::move(tab);
    std::memcpy(totals, tot, sizeof tot);
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_simplify(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, double cell, int32_t rule, int32_t flags,
                      int32_t device, float* verts_out, int32_t* tris_out, int32_t* vert_map_out, int32_t* tri_map_out, int64_t totals[8])
{
    if (const int rc = simplify_args(verts, n_verts, tris, n_tris, cell, rule, flags, verts_out, tris_out, totals)) return rc;
    MeshCall<SimplifyWork> call("mesh_simplify", g_simplify_work, verts, n_verts, tris, n_tris, device);
    return simplify_run(call, n_verts, n_tris, cell, rule, flags, verts_out, tris_out, vert_map_out, tri_map_out, totals);
}

int r2s_mesh_simplify_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, double cell, int32_t rule, int32_t flags,
                          float* d_verts_out, int32_t* d_tris_out, int32_t* d_vert_map_out, int32_t* d_tri_map_out, int64_t totals[8],
                          void* stream)
{
    if (const int rc = simplify_args(d_verts, n_verts, d_tris, n_tris, cell, rule, flags, d_verts_out, d_tris_out, totals)) return rc;
    MeshCall<SimplifyWork> call("mesh_simplify", g_simplify_work, d_verts, n_verts, d_tris, n_tris, (hipStream_t)stream);
    return simplify_run(call, n_verts, n_tris, cell, rule, flags, d_verts_out, d_tris_out, d_vert_map_out, d_tri_map_out, totals);
}

int r2s_last_mesh_simplify(int64_t* members_out, double* error_out, int32_t* solved_out, int64_t capacity, int64_t* n_verts_out)
{
    if (!n_verts_out || capacity < 0 || (capacity > 0 && (!members_out || !error_out || !solved_out)))
        return fail(R2S_ERR_ARG, "last_mesh_simplify: null output or negative capacity");
    const SimplifyTables& t = g_last_simplify;
    *n_verts_out = (int64_t)t.members.size();
    copy_rows(members_out, t.members, 1, capacity, *n_verts_out);
    copy_rows(error_out, t.error, 1, capacity, *n_verts_out);
    copy_rows(solved_out, t.solved, 1, capacity, *n_verts_out);
    return 0;
}

}  // extern "C"
