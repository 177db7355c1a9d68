// Mesh winding: the signed count of crossings of an axis ray from every query point, the inside / outside verdict derived from
// it and the signed distance s * d (include/rho2sdf_hip.h, r2s_mesh_index_winding / _signed; DESIGN.md "Mesh winding").
// mwn_points_kernel: one lane per point, 64 points per workgroup, the per-lane LDS stack of mi_query_kernel.  The ray is one of
// the six axis directions, so a box is culled by three exact comparisons (axis_enter, r2s_mesh_tree.hpp) and no ordering of the children is needed: every
// child whose box passes is entered, the second one through the stack.  A leaf runs axis_cross (r2s_tri_math.hpp), which holds
// the own-box condition of the definition; two integer accumulators per lane, plain stores, no atomics.  With a distance
// buffer the lane then applies the inside rule to the distance mi_query_kernel left there for the same point, in place.
// The lattice entries go by rows (mwn_rows_kernel and mwn_prefix_kernel below); with R2S_WINDING_ROWS=0 they run the per-point
// kernel on the 4x4x4 blocks of mi_query_kernel.  The results are equal.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_tree.hpp"
#include "r2s_tri_math.hpp"

using namespace r2s_int;

namespace {

struct MwnArgs {
    const MiNode* nodes;
    const float* verts;
    const int32_t* tris;
    int64_t ntris;
    int32_t root;              // node 0, or ~triangle for a single triangle
    const void* pts;           // [n][3] (POINTS)
    int pts_f32;
    int64_t n;
    int64_t nx, ny, nz, nbx, nby;   // lattice and its 4x4x4 blocks (LATTICE)
    double o[3], h;
    int neg;                   // the ray runs along -e_KZ
    int32_t* winding;          // may be null
    int32_t* crossings;        // may be null
    void* dist;                // may be null; else the unsigned distances of the same points, signed in place by `rule`
    int dist_f32;
    int rule;
};

// One lane per query point.  LATTICE: a workgroup (one wave) is a 4x4x4 block of lattice points; else 64 consecutive points.
template <int KZ, bool LATTICE>
__global__ void __launch_bounds__(64) mwn_points_kernel(MwnArgs g)
{
    __shared__ int32_t stk[MI_STACK * 64];
    const int lane = threadIdx.x;
    int64_t i;
    bool valid;
    Vec3 p;
    if (LATTICE) {
        const int64_t b = blockIdx.x;
        const int64_t ix = (b % g.nbx) * 4 + (lane & 3), iy = ((b / g.nbx) % g.nby) * 4 + ((lane >> 2) & 3),
                      iz = (b / (g.nbx * g.nby)) * 4 + (lane >> 4);
        valid = ix < g.nx && iy < g.ny && iz < g.nz;
        i = (iz * g.ny + iy) * g.nx + ix;
        p = {g.o[0] + g.h * (double)ix, g.o[1] + g.h * (double)iy, g.o[2] + g.h * (double)iz};
    } else {
        i = (int64_t)blockIdx.x * 64 + lane;
        valid = i < g.n;
        p = {0.0, 0.0, 0.0};
        if (valid) {
            if (g.pts_f32) {
                const float* q = reinterpret_cast<const float*>(g.pts) + 3 * i;
                p = {(double)q[0], (double)q[1], (double)q[2]};
            } else {
                const double* q = reinterpret_cast<const double*>(g.pts) + 3 * i;
                p = {q[0], q[1], q[2]};
            }
        }
    }
    if (!valid) return;
    const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    int32_t wn = 0, nc = finite ? 0 : -1;
    if (finite && g.ntris > 0) {
        constexpr int K1 = (KZ + 1) % 3, K2 = (KZ + 2) % 3;
        const bool neg = g.neg != 0;
        const double o1 = vec_pick(p, K1), o2 = vec_pick(p, K2), oz = vec_pick(p, KZ);
        int sp = 0;
        int32_t cur = g.root;
        for (;;) {
            if (cur < 0) {
                const int32_t* tv = g.tris + 3 * (int64_t)(~cur);
                const int32_t ia = tv[0], ib = tv[1], ic = tv[2];
                if (ia != ib && ib != ic && ia != ic) {   // (a collapsed triangle takes part in nothing)
                    const float *a = g.verts + 3 * (int64_t)ia, *b = g.verts + 3 * (int64_t)ib, *c = g.verts + 3 * (int64_t)ic;
                    const float fa[3] = {a[0], a[1], a[2]}, fb[3] = {b[0], b[1], b[2]}, fc[3] = {c[0], c[1], c[2]};
                    const int side = axis_cross<KZ>(p, neg, fa, fb, fc);
                    wn -= side;
                    nc += side != 0;
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
    }
    if (g.winding) g.winding[i] = wn;
    if (g.crossings) g.crossings[i] = nc;
    if (g.dist) {
        const bool inside = g.rule == R2S_INSIDE_POSITIVE ? wn > 0 : (g.rule == R2S_INSIDE_NONZERO ? wn != 0 : (nc & 1) != 0);
        const double d = load_real(g.dist, g.dist_f32, i);
        store_real(g.dist, g.dist_f32, i, (inside ? d : -d) + 0.0);   // (-0 -> +0; NaN and inf pass through)
    }
}

// ---- the lattice by rows ------------------------------------------------------------------------------------------------------
// All points of a lattice row along the ray's axis share U, V, W, det and the two projected comparisons (axis_cross_2d), and
// what is left (axis_cross_1d) is monotone along the row.  mwn_rows_kernel: one lane per row, an 8x8 tile of rows per wave; the
// lane traverses the tree once with the two projected comparisons and the row's extent on the ray's axis, and for every triangle
// that can be crossed finds by bisection over the row index the threshold at which axis_cross_1d switches, evaluating that
// predicate itself at the lattice point as the per-point kernel forms it.  It then adds -side (and 1) to difference arrays kept
// in the output buffers (zeroed before): the lane owns its row, so these are plain read-modify-writes, no atomics.  Every write
// stays inside the row: a threshold at the row's end writes nothing.  mwn_prefix_kernel sums each row in place.
struct MwnRows {
    const MiNode* nodes;
    const float* verts;
    const int32_t* tris;
    int64_t ntris;
    int32_t root;
    int64_t n[3];              // nx, ny, nz
    double o[3], h;
    int neg;
    int32_t* winding;          // may be null
    int32_t* crossings;        // may be null
    int64_t stride;            // int32 words from one lattice point to the next (2: the low words of a float64 buffer)
    void* sign_out;            // may be null; else (prefix kernel) +1 / -1 by `rule` in the type of that buffer, which may be the
    int sign_f32;              // buffer the integers are in
    int rule;
};

// the row of this lane: its two fixed lattice indices -> false when outside; base = the linear index of its first point,
// rs = the step of the linear index along the row
template <int KZ>
__device__ inline bool mwn_row_of_lane(const MwnRows& g, int64_t& j1, int64_t& j2, int64_t& base, int64_t& rs)
{
    constexpr int K1 = (KZ + 1) % 3, K2 = (KZ + 2) % 3;
    constexpr int KF = K1 < K2 ? K1 : K2, KS = K1 < K2 ? K2 : K1;   // the tile's fast axis is the lower one (x where it is free)
    const int lane = threadIdx.x;
    const int64_t nbf = (g.n[KF] + 7) / 8, b = blockIdx.x;
    const int64_t jf = (b % nbf) * 8 + (lane & 7), js = (b / nbf) * 8 + (lane >> 3);
    if (jf >= g.n[KF] || js >= g.n[KS]) return false;
    j1 = KF == K1 ? jf : js, j2 = KF == K1 ? js : jf;
    const int64_t sa[3] = {1, g.n[0], g.n[0] * g.n[1]};
    base = j1 * sa[K1] + j2 * sa[K2], rs = sa[KZ];
    return true;
}

template <int KZ>
__global__ void __launch_bounds__(64) mwn_rows_kernel(MwnRows g)
{
    __shared__ int32_t stk[MI_STACK * 64];
    constexpr int K1 = (KZ + 1) % 3, K2 = (KZ + 2) % 3;
    const int lane = threadIdx.x;
    int64_t j1, j2, base, rs;
    if (!mwn_row_of_lane<KZ>(g, j1, j2, base, rs) || g.ntris <= 0) return;
    const bool neg = g.neg != 0;
    const int64_t nr = g.n[KZ];
    const double o1 = g.o[K1] + g.h * (double)j1, o2 = g.o[K2] + g.h * (double)j2;
    const double zlo = g.o[KZ] + g.h * (double)0, zhi = g.o[KZ] + g.h * (double)(nr - 1);
    const double zend = neg ? zhi : zlo;   // the point of the row that sees the most
    int sp = 0;
    int32_t cur = g.root;
    for (;;) {
        if (cur < 0) {
            const int32_t* tv = g.tris + 3 * (int64_t)(~cur);
            const int32_t ia = tv[0], ib = tv[1], ic = tv[2];
            if (ia != ib && ib != ic && ia != ic) {
                const float *a = g.verts + 3 * (int64_t)ia, *b = g.verts + 3 * (int64_t)ib, *c = g.verts + 3 * (int64_t)ic;
                const float fa[3] = {a[0], a[1], a[2]}, fb[3] = {b[0], b[1], b[2]}, fc[3] = {c[0], c[1], c[2]};
                double U, V, W;
                const int side = axis_cross_2d<KZ>(o1, o2, neg, fa, fb, fc, U, V, W);
                if (side != 0) {
                    // +e_KZ: crossed from the points [0, m); -e_KZ: from the points [m, nr)
                    int64_t lo = 0, hi = nr;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        const bool on = axis_cross_1d<KZ>(g.o[KZ] + g.h * (double)mid, neg, fa, fb, fc, U, V, W);
                        if (on != neg)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    const int64_t first = neg ? lo : 0, end = neg ? nr : lo;
                    if (first < end) {
                        const int64_t p0 = (base + first * rs) * g.stride, p1 = (base + end * rs) * g.stride;
                        if (g.winding) {
                            g.winding[p0] -= side;
                            if (end < nr) g.winding[p1] += side;
                        }
                        if (g.crossings) {
                            g.crossings[p0] += 1;
                            if (end < nr) g.crossings[p1] -= 1;
                        }
                    }
                }
            }
        } else {
            const MiNode nd = load_node(g.nodes + cur);
            const bool e0 = axis_enter<KZ>(nd.box[0], o1, o2, zend, neg), e1 = axis_enter<KZ>(nd.box[1], o1, o2, zend, neg);
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
}

// one lane per row (the lane that wrote its differences): running sums in place; with sign_out the one integer array present
// becomes the sign of the inside rule, +1 / -1 in the type of that buffer (read before written, element by element)
template <int KZ>
__global__ void __launch_bounds__(64) mwn_prefix_kernel(MwnRows g)
{
    int64_t j1, j2, base, rs;
    if (!mwn_row_of_lane<KZ>(g, j1, j2, base, rs)) return;
    const int64_t nr = g.n[KZ];
    int32_t wn = 0, nc = 0;
    for (int64_t i = 0; i < nr; ++i) {
        const int64_t e = base + i * rs, p = e * g.stride;
        if (g.winding) wn += g.winding[p];
        if (g.crossings) nc += g.crossings[p];
        if (g.sign_out) {
            const bool inside = g.rule == R2S_INSIDE_POSITIVE ? wn > 0 : (g.rule == R2S_INSIDE_NONZERO ? wn != 0 : (nc & 1) != 0);
            store_real(g.sign_out, g.sign_f32, e, inside ? 1.0 : -1.0);
        } else {
            if (g.winding) g.winding[p] = wn;
            if (g.crossings) g.crossings[p] = nc;
        }
    }
}

// -0 -> +0 over n values (the signed lattice by rows: mi_query_kernel leaves -0 for a point on the surface that counts as outside)
__global__ void __launch_bounds__(256) mwn_poszero_kernel(void* d, int f32, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) store_real(d, f32, i, load_real(d, f32, i) + 0.0);
}

// R2S_WINDING_ROWS=0: the lattice entries run mwn_points_kernel on 4x4x4 blocks instead of the row kernels (the same results)
bool use_rows()
{
    const char* e = std::getenv("R2S_WINDING_ROWS");
    return !(e && e[0] == '0');
}

// enqueues the row kernels on `st`: differences into the zeroed d_winding / d_crossings (int32 at `stride` words per point), then
// their running sums, or with sign_out the sign of `rule`
int mwn_rows(const MiTree& T, const int64_t* dims, const double* origin, double spacing, int ray, int32_t* d_winding, int32_t* d_crossings,
             int64_t stride, void* sign_out, bool sign_f32, int rule, hipStream_t st)
{
    if (const int rc = check_depth(T)) return rc;
    MwnRows g = {};
    g.nodes = T.nodes.as<MiNode>();
    g.verts = T.verts, g.tris = T.tris, g.ntris = T.n_tris, g.root = T.root;
    for (int a = 0; a < 3; ++a) g.n[a] = dims[a], g.o[a] = origin[a];
    g.h = spacing, g.neg = ray >= 3 ? 1 : 0;
    g.winding = d_winding, g.crossings = d_crossings, g.stride = stride;
    g.sign_out = sign_out, g.sign_f32 = sign_f32 ? 1 : 0, g.rule = rule;
    const int kz = ray % 3, k1 = (kz + 1) % 3, k2 = (kz + 2) % 3;
    const int64_t nb = ((dims[k1] + 7) / 8) * ((dims[k2] + 7) / 8);
    if (nb > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "mesh_index_winding: %lld row tiles exceed one launch", (long long)nb);
    const size_t bytes = sizeof(int32_t) * (size_t)stride * (size_t)(dims[0] * dims[1] * dims[2]);
    if (d_winding) HIP_TRY(hipMemsetAsync(d_winding, 0, bytes, st));
    if (d_crossings) HIP_TRY(hipMemsetAsync(d_crossings, 0, bytes, st));
    if (kz == 0) {
        mwn_rows_kernel<0><<<(unsigned)nb, 64, 0, st>>>(g);
        mwn_prefix_kernel<0><<<(unsigned)nb, 64, 0, st>>>(g);
    } else if (kz == 1) {
        mwn_rows_kernel<1><<<(unsigned)nb, 64, 0, st>>>(g);
        mwn_prefix_kernel<1><<<(unsigned)nb, 64, 0, st>>>(g);
    } else {
        mwn_rows_kernel<2><<<(unsigned)nb, 64, 0, st>>>(g);
        mwn_prefix_kernel<2><<<(unsigned)nb, 64, 0, st>>>(g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// enqueues the winding of n points (pts != null) or of the lattice (dims != null) on `st`; does not wait.  d_dist != null: also
// signs the distances there
int mwn_run(const MiTree& T, const void* d_pts, bool pts_f32, int64_t n, const int64_t* dims, const double* origin, double spacing, int ray,
            int32_t* d_winding, int32_t* d_crossings, void* d_dist, bool dist_f32, int rule, hipStream_t st)
{
    if (const int rc = check_depth(T)) return rc;
    MwnArgs g = {};
    g.nodes = T.nodes.as<MiNode>();
    g.verts = T.verts, g.tris = T.tris, g.ntris = T.n_tris, g.root = T.root;
    g.neg = ray >= 3 ? 1 : 0;
    g.winding = d_winding, g.crossings = d_crossings, g.dist = d_dist, g.dist_f32 = dist_f32 ? 1 : 0, g.rule = rule;
    const int kz = ray % 3;
    if (dims && !d_dist && use_rows()) return mwn_rows(T, dims, origin, spacing, ray, d_winding, d_crossings, 1, nullptr, false, 0, st);
    if (dims) {
        g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
        g.nbx = (g.nx + 3) / 4, g.nby = (g.ny + 3) / 4;
        const int64_t nb = g.nbx * g.nby * ((g.nz + 3) / 4);
        if (nb > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "mesh_index_winding: %lld voxel blocks exceed one launch", (long long)nb);
        for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
        g.h = spacing;
        if (kz == 0)
            mwn_points_kernel<0, true><<<(unsigned)nb, 64, 0, st>>>(g);
        else if (kz == 1)
            mwn_points_kernel<1, true><<<(unsigned)nb, 64, 0, st>>>(g);
        else
            mwn_points_kernel<2, true><<<(unsigned)nb, 64, 0, st>>>(g);
    } else {
        if (n == 0) return 0;
        g.pts = d_pts, g.pts_f32 = pts_f32 ? 1 : 0, g.n = n;
        const unsigned nb = (unsigned)((n + 63) / 64);
        if (kz == 0)
            mwn_points_kernel<0, false><<<nb, 64, 0, st>>>(g);
        else if (kz == 1)
            mwn_points_kernel<1, false><<<nb, 64, 0, st>>>(g);
        else
            mwn_points_kernel<2, false><<<nb, 64, 0, st>>>(g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// the unsigned distance of mi_query into d_dist, then its sign in place; both on `st`, does not wait
int mwn_signed(const MiTree& T, const void* d_pts, bool pts_f32, int64_t n, const int64_t* dims, const double* origin, double spacing,
               int rule, int ray, void* d_dist, bool out_f32, int32_t* d_closest, hipStream_t st)
{
    if (dims && use_rows()) {
        // No room is needed beside the output: the rows count into the distance buffer itself (one int32 per point, winding or
        // crossings as the rule asks), the prefix kernel turns that into a field of +1 / -1 in the buffer's type, and mi_query_kernel
        // takes its sign from a field: s = +1 where field >= 0.  Each lane reads its point's field value before it stores there.
        const bool odd = rule == R2S_INSIDE_ODD;
        int32_t* cnt = reinterpret_cast<int32_t*>(d_dist);
        if (const int rc = mwn_rows(T, dims, origin, spacing, ray, odd ? nullptr : cnt, odd ? cnt : nullptr, out_f32 ? 1 : 2, d_dist, out_f32,
                                    rule, st))
            return rc;
        if (const int rc = mi_query(T, nullptr, false, 0, dims, origin, spacing, d_dist, out_f32, 0.0, d_dist, out_f32, d_closest, st)) return rc;
        const int64_t nvox = dims[0] * dims[1] * dims[2];
        mwn_poszero_kernel<<<(unsigned)((nvox + 255) / 256), 256, 0, st>>>(d_dist, out_f32 ? 1 : 0, nvox);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (const int rc = mi_query(T, d_pts, pts_f32, n, dims, origin, spacing, nullptr, false, 0.0, d_dist, out_f32, d_closest, st)) return rc;
    return mwn_run(T, d_pts, pts_f32, n, dims, origin, spacing, ray, nullptr, nullptr, d_dist, out_f32, rule, st);
}

int ray_rule_args(const char* who, int32_t ray, int32_t rule)
{
    if (ray < 0 || ray > 5) return fail(R2S_ERR_ARG, "%s: ray must be 0..5 (+x +y +z -x -y -z), got %d", who, (int)ray);
    if (rule < R2S_INSIDE_POSITIVE || rule > R2S_INSIDE_ODD) return fail(R2S_ERR_ARG, "%s: rule must be 0..2, got %d", who, (int)rule);
    return 0;
}

int point_args(const char* who, const r2s_mesh_index* ix, const void* points, int64_t n, const void* out, int32_t ray, int32_t rule)
{
    if (!ix) return fail(R2S_ERR_ARG, "%s: null index", who);
    if (n < 0) return fail(R2S_ERR_ARG, "%s: negative point count", who);
    if (n > 0 && (!points || !out)) return fail(R2S_ERR_ARG, "%s: null points / output", who);
    if (const int rc = ray_rule_args(who, ray, rule)) return rc;
    if (n > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "%s: %lld points exceed one call", who, (long long)n);
    return 0;
}

int grid_args(const char* who, const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing, const void* out,
              int32_t ray, int32_t rule)
{
    if (const int rc = lattice_args(who, dims, origin, spacing, 1.0)) return rc;
    if (!ix || !out) return fail(R2S_ERR_ARG, "%s: null index / output", who);
    return ray_rule_args(who, ray, rule);
}

inline size_t lattice_size(const int64_t dims[3]) { return (size_t)(dims[0] * dims[1] * dims[2]); }

}  // namespace

extern "C" {

int r2s_mesh_index_winding(const r2s_mesh_index* ix, const void* points, int32_t points_are_float32, int64_t n, int32_t ray,
                           int32_t* winding_out, int32_t* crossings_out)
{
    int rc = point_args("mesh_index_winding", ix, points, n, winding_out, ray, R2S_INSIDE_POSITIVE);
    if (rc || n == 0) return rc;
    const size_t np = (size_t)n;
    const HostIo pts{points, nullptr, 3 * real_bytes(points_are_float32) * np}, w{nullptr, winding_out, sizeof(int32_t) * np},
        c{nullptr, crossings_out, sizeof(int32_t) * np};
    return staged_call(ix, {pts, w, c}, [&](DevBuf* b) {
        return mwn_run(ix->tree, b[0].p, points_are_float32 != 0, n, nullptr, nullptr, 0.0, ray, b[1].as<int32_t>(), b[2].as<int32_t>(), nullptr,
                       false, 0, nullptr);
    });
}

int r2s_mesh_index_winding_dev(const r2s_mesh_index* ix, const void* d_points, int32_t points_are_float32, int64_t n, int32_t ray,
                               int32_t* d_winding_out, int32_t* d_crossings_out, void* stream)
{
    int rc = point_args("mesh_index_winding", ix, d_points, n, d_winding_out, ray, R2S_INSIDE_POSITIVE);
    if (rc || n == 0) return rc;
    if ((rc = check_device(0)) || (rc = index_on_current_device("mesh_index_winding", ix))) return rc;
    return mwn_run(ix->tree, d_points, points_are_float32 != 0, n, nullptr, nullptr, 0.0, ray, d_winding_out, d_crossings_out, nullptr, false, 0,
                   (hipStream_t)stream);
}

int r2s_mesh_index_winding_lattice(const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing, int32_t ray,
                                   int32_t* winding_out, int32_t* crossings_out)
{
    const int rc = grid_args("mesh_index_winding_lattice", ix, dims, origin, spacing, winding_out, ray, R2S_INSIDE_POSITIVE);
    if (rc) return rc;
    const size_t bytes = sizeof(int32_t) * lattice_size(dims);
    const HostIo w{nullptr, winding_out, bytes}, c{nullptr, crossings_out, bytes};
    return staged_call(ix, {w, c}, [&](DevBuf* b) {
        return mwn_run(ix->tree, nullptr, false, 0, dims, origin, spacing, ray, b[0].as<int32_t>(), b[1].as<int32_t>(), nullptr, false, 0, nullptr);
    });
}

int r2s_mesh_index_winding_lattice_dev(const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing, int32_t ray,
                                       int32_t* d_winding_out, int32_t* d_crossings_out, void* stream)
{
    int rc = grid_args("mesh_index_winding_lattice", ix, dims, origin, spacing, d_winding_out, ray, R2S_INSIDE_POSITIVE);
    if (rc || (rc = check_device(0)) || (rc = index_on_current_device("mesh_index_winding_lattice", ix))) return rc;
    return mwn_run(ix->tree, nullptr, false, 0, dims, origin, spacing, ray, d_winding_out, d_crossings_out, nullptr, false, 0,
                   (hipStream_t)stream);
}

int r2s_mesh_index_signed(const r2s_mesh_index* ix, const void* points, int32_t points_are_float32, int64_t n, int32_t rule, int32_t ray,
                          int32_t out_is_float32, void* dist_out, int32_t* closest_tri_out)
{
    int rc = point_args("mesh_index_signed", ix, points, n, dist_out, ray, rule);
    if (rc || n == 0) return rc;
    const size_t np = (size_t)n;
    const HostIo pts{points, nullptr, 3 * real_bytes(points_are_float32) * np}, out{nullptr, dist_out, real_bytes(out_is_float32) * np},
        idx{nullptr, closest_tri_out, sizeof(int32_t) * np};
    return staged_call(ix, {pts, out, idx}, [&](DevBuf* b) {
        return mwn_signed(ix->tree, b[0].p, points_are_float32 != 0, n, nullptr, nullptr, 0.0, rule, ray, b[1].p, out_is_float32 != 0,
                          b[2].as<int32_t>(), nullptr);
    });
}

int r2s_mesh_index_signed_dev(const r2s_mesh_index* ix, const void* d_points, int32_t points_are_float32, int64_t n, int32_t rule, int32_t ray,
                              int32_t out_is_float32, void* d_dist_out, int32_t* d_closest_tri_out, void* stream)
{
    int rc = point_args("mesh_index_signed", ix, d_points, n, d_dist_out, ray, rule);
    if (rc || n == 0) return rc;
    if ((rc = check_device(0)) || (rc = index_on_current_device("mesh_index_signed", ix))) return rc;
    return mwn_signed(ix->tree, d_points, points_are_float32 != 0, n, nullptr, nullptr, 0.0, rule, ray, d_dist_out, out_is_float32 != 0,
                      d_closest_tri_out, (hipStream_t)stream);
}

int r2s_mesh_index_signed_lattice(const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing, int32_t rule,
                                  int32_t ray, int32_t out_is_float32, void* dist_out, int32_t* closest_tri_out)
{
    const int rc = grid_args("mesh_index_signed_lattice", ix, dims, origin, spacing, dist_out, ray, rule);
    if (rc) return rc;
    const size_t nvox = lattice_size(dims);
    const HostIo out{nullptr, dist_out, real_bytes(out_is_float32) * nvox}, idx{nullptr, closest_tri_out, sizeof(int32_t) * nvox};
    return staged_call(ix, {out, idx}, [&](DevBuf* b) {
        return mwn_signed(ix->tree, nullptr, false, 0, dims, origin, spacing, rule, ray, b[0].p, out_is_float32 != 0, b[1].as<int32_t>(), nullptr);
    });
}

int r2s_mesh_index_signed_lattice_dev(const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing, int32_t rule,
                                      int32_t ray, int32_t out_is_float32, void* d_dist_out, int32_t* d_closest_tri_out, void* stream)
{
    int rc = grid_args("mesh_index_signed_lattice", ix, dims, origin, spacing, d_dist_out, ray, rule);
    if (rc || (rc = check_device(0)) || (rc = index_on_current_device("mesh_index_signed_lattice", ix))) return rc;
    return mwn_signed(ix->tree, nullptr, false, 0, dims, origin, spacing, rule, ray, d_dist_out, out_is_float32 != 0, d_closest_tri_out,
                      (hipStream_t)stream);
}

int r2s_mesh_signed_distance(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int64_t dims[3],
                             const double origin[3], double spacing, int32_t rule, int32_t ray, int32_t out_is_float32, int32_t device, void* out)
{
    int rc = mesh_args("mesh_signed_distance", verts, n_verts, tris, n_tris);
    if (rc || (rc = lattice_args("mesh_signed_distance", dims, origin, spacing, 1.0))) return rc;
    if (!out) return fail(R2S_ERR_ARG, "mesh_signed_distance: null output");
    if ((rc = ray_rule_args("mesh_signed_distance", ray, rule))) return rc;
    if ((rc = check_mesh_host("mesh_signed_distance", verts, n_verts, tris, n_tris)) || (rc = check_device(device < 0 ? 0 : device))) return rc;
    DeviceScope scope;   // (device < 0: the current device)
    if (device >= 0 && (rc = scope.enter(device))) return rc;
    const size_t bytes = real_bytes(out_is_float32) * lattice_size(dims);
    DevBuf dv, dt, dd;
    if ((rc = upload_mesh(dv, dt, verts, n_verts, tris, n_tris, false, nullptr))) return rc;
    ENSURE(dd, bytes);
    MiTree T;   // (built, used and dropped: the nodes free themselves)
    if ((rc = mi_build_tree(dv.as<float>(), n_verts, dt.as<int32_t>(), n_tris, nullptr, T))) return rc;
    if ((rc = mwn_signed(T, nullptr, false, 0, dims, origin, spacing, rule, ray, dd.p, out_is_float32 != 0, nullptr, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dd.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int r2s_mesh_signed_distance_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, const int64_t dims[3],
                                 const double origin[3], double spacing, int32_t rule, int32_t ray, int32_t out_is_float32, void* d_out,
                                 void* stream)
{
    int rc = mesh_args("mesh_signed_distance", d_verts, n_verts, d_tris, n_tris);
    if (rc || (rc = lattice_args("mesh_signed_distance", dims, origin, spacing, 1.0))) return rc;
    if (!d_out) return fail(R2S_ERR_ARG, "mesh_signed_distance: null output");
    if ((rc = ray_rule_args("mesh_signed_distance", ray, rule)) || (rc = check_device(0))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    DevBuf flag;
    if ((rc = check_mesh_dev("mesh_signed_distance", d_verts, n_verts, d_tris, n_tris, flag, st))) return rc;
    MiTree T;
    if ((rc = mi_build_tree(d_verts, n_verts, d_tris, n_tris, st, T))) return rc;
    if ((rc = mwn_signed(T, nullptr, false, 0, dims, origin, spacing, rule, ray, d_out, out_is_float32 != 0, nullptr, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // (the tree is dropped on return)
    return 0;
}

}  // extern "C"
