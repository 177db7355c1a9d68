// Mesh index: a linear BVH over the triangles of a mesh, one stack traversal per query point and one per ray
// (include/rho2sdf_hip.h, r2s_mesh_index_*; DESIGN.md "Mesh index" and "Ray queries").
// Build: mi_bounds_kernel (mesh AABB, integer atomics on order-preserving bit patterns) -> mi_key_kernel (30-bit Morton code
// of the triangle's AABB centre << 32 | triangle index: unique keys) -> rocPRIM radix sort -> mi_tree_kernel (Karras 2012, one
// thread per internal node) -> mi_refit_kernel (one thread per leaf walks up; the second arrival at a node, counted by an
// integer flag, joins the two child boxes and carries the height on).  A node holds the float32 boxes of its two children,
// the children (>= 0: internal node, < 0: the leaf of triangle ~child) and their heights: 64 bytes, four 16-byte loads.
// Query: mi_query_kernel, one lane per point, the nearer child first, the other pushed on a per-lane LDS stack of MI_STACK
// entries.  A leaf builds the record of md_tile_kernel (build_record) in registers and calls pair_d2: the same arithmetic,
// hence the same numbers wherever both kernels answer.  Rays: see mi_ray_kernel.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_mesh_tree.hpp"
#include "r2s_tri_math.hpp"

using namespace r2s_int;

// (r2s_mesh_index, MiNode, load_node, tri_box and MI_STACK: r2s_mesh_tree.hpp)
namespace {

constexpr uint32_t MI_ROOT = 0xffffffffu;

__device__ inline uint32_t mi_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
inline float mi_unordered(uint32_t u)
{
    const uint32_t b = (u >> 31) ? (u & 0x7fffffffu) : ~u;
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}

__device__ inline void mi_tri_box(const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t t, float lo[3], float hi[3])
{
    tri_box(verts + 3 * (int64_t)tris[3 * t], verts + 3 * (int64_t)tris[3 * t + 1], verts + 3 * (int64_t)tris[3 * t + 2], lo, hi);
}

// bb[0..2] = min, bb[3..5] = max over the triangles' vertices, as ordered bit patterns (bb starts as ~0, ~0, ~0, 0, 0, 0)
__global__ void __launch_bounds__(256) mi_bounds_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t ntris,
                                                         uint32_t* __restrict__ bb)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (t < ntris) {
        float flo[3], fhi[3];
        mi_tri_box(verts, tris, t, flo, fhi);
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = mi_ordered(flo[k]), hi[k] = mi_ordered(fhi[k]);
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
            atomicMin(&bb[k], lo[k]);
            atomicMax(&bb[3 + k], hi[k]);
        }
    }
}

__device__ inline uint32_t mi_spread10(uint32_t x)
{
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

struct MiFrame {
    double lo[3], scale[3];   // scale = 1024 / extent, 0 for an axis of zero extent
};

__global__ void __launch_bounds__(256) mi_key_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris, int64_t ntris,
                                                      MiFrame f, uint64_t* __restrict__ keys)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ntris) return;
    float lo[3], hi[3];
    mi_tri_box(verts, tris, t, lo, hi);
    uint32_t q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = 0.5 * ((double)lo[k] + (double)hi[k]);
        double v = (c - f.lo[k]) * f.scale[k];
        v = v > 0.0 ? v : 0.0;   // (also NaN -> 0)
        q[k] = v < 1023.0 ? (uint32_t)v : 1023u;
    }
    const uint32_t code = mi_spread10(q[0]) | (mi_spread10(q[1]) << 1) | (mi_spread10(q[2]) << 2);
    keys[t] = ((uint64_t)code << 32) | (uint64_t)(uint32_t)t;
}

// length of the common prefix of keys i and j, -1 outside [0, n) (the keys are unique: never 64)
__device__ inline int mi_delta(const uint64_t* __restrict__ keys, int64_t n, int64_t i, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(keys[i] ^ keys[j]));
}

// Karras, "Maximizing parallelism in the construction of BVHs, octrees and k-d trees" (2012): internal node i of n - 1;
// parent[x] = 2 * node + side for internal node x < n - 1 and for leaf j at n - 1 + j
__global__ void __launch_bounds__(256) mi_tree_kernel(const uint64_t* __restrict__ keys, int64_t n, MiNode* __restrict__ nodes,
                                                       uint32_t* __restrict__ parent)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1) return;
    const int64_t d = mi_delta(keys, n, i, i + 1) > mi_delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = mi_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (mi_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (mi_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = mi_delta(keys, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (mi_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    const bool leaf0 = first == gamma, leaf1 = last == gamma + 1;
    nodes[i].child[0] = leaf0 ? ~(int32_t)(uint32_t)keys[gamma] : (int32_t)gamma;
    nodes[i].child[1] = leaf1 ? ~(int32_t)(uint32_t)keys[gamma + 1] : (int32_t)(gamma + 1);
    parent[leaf0 ? n - 1 + gamma : gamma] = (uint32_t)i * 2u;
    parent[leaf1 ? n - 1 + gamma + 1 : gamma + 1] = (uint32_t)i * 2u + 1u;
    if (i == 0) parent[0] = MI_ROOT;
}

// one thread per leaf (sorted position j); flags[node] counts arrivals; *depth = the height of the root
__global__ void __launch_bounds__(256) mi_refit_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                        const uint64_t* __restrict__ keys, int64_t n, MiNode* nodes,
                                                        const uint32_t* __restrict__ parent, int32_t* flags, int32_t* depth)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float lo[3], hi[3];
    mi_tri_box(verts, tris, (int64_t)(uint32_t)keys[j], lo, hi);
    int32_t h = 0;
    uint32_t up = parent[n - 1 + j];
    while (up != MI_ROOT) {
        const int64_t p = up >> 1;
        const int side = up & 1u;
        MiNode* nd = nodes + p;
#pragma unroll
        for (int k = 0; k < 3; ++k) nd->box[side][k] = lo[k], nd->box[side][3 + k] = hi[k];
        nd->height[side] = h;
        __threadfence();                              // the box is visible before the arrival is counted
        if (atomicAdd(&flags[p], 1) == 0) return;     // the first arrival stops; the second one has both boxes
        __threadfence();
        const volatile MiNode* o = nd;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], o->box[side ^ 1][k]);
            hi[k] = fmaxf(hi[k], o->box[side ^ 1][3 + k]);
        }
        const int32_t ho = o->height[side ^ 1];
        h = (h > ho ? h : ho) + 1;
        up = parent[p];
    }
    *depth = h;
}

struct MiQuery {
    const MiNode* nodes;
    const float* verts;
    const int32_t* tris;
    int64_t ntris;
    int32_t root;              // node 0, or ~triangle for a single triangle
    double absmax;             // largest absolute vertex coordinate
    const void* pts;           // [n][3] (POINTS)
    int pts_f32;
    int64_t n;
    int64_t nx, ny, nz, nbx, nby;   // lattice and its 4x4x4 blocks (LATTICE)
    double o[3], h;
    const void* field;         // may be null: the sign is +1 where field >= iso, else -1 (NaN: -1)
    int field_f32;
    double iso;
    void* out;
    int out_f32;
    int32_t* closest;
};

__device__ inline double mi_box_d2(Vec3 p, const float* __restrict__ b)
{
    const double gx = fmax(fmax((double)b[0] - p.x, p.x - (double)b[3]), 0.0);
    const double gy = fmax(fmax((double)b[1] - p.y, p.y - (double)b[4]), 0.0);
    const double gz = fmax(fmax((double)b[2] - p.z, p.z - (double)b[5]), 0.0);
    return gx * gx + gy * gy + gz * gz;
}

// box_d2 > (sqrt(best) + 2 m)^2 without the root: q = box_d2 - best - 4 m^2 > 0 and q^2 > 16 m^2 best (the threshold of
// md_tile_kernel; best = inf never skips, equal lower bounds never skip)
__device__ inline bool mi_farther(double box_d2, double best, double m2)
{
    const double q = box_d2 - best - 4.0 * m2;
    return q > 0.0 && q * q > 16.0 * m2 * best;
}

// One lane per query point.  LATTICE: a workgroup (one wave) is a 4x4x4 block of lattice points; else 64 consecutive points.
template <bool LATTICE>
__global__ void __launch_bounds__(64) mi_query_kernel(MiQuery g)
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
    double best = __builtin_huge_val();
    int32_t bi = INT32_MAX;
    if (finite && g.ntris > 0) {
        const double big = fmax(fmax(fabs(p.x), fabs(p.y)), fmax(fabs(p.z), g.absmax));
        const double m = ldexp(big, -40), m2 = m * m;
        int sp = 0;
        int32_t cur = g.root;
        for (;;) {
            if (cur < 0) {
                const int32_t t = ~cur;
                float bx[6];
                mi_tri_box(g.verts, g.tris, t, bx, bx + 3);
                if (!mi_farther(mi_box_d2(p, bx), best, m2)) {   // (a popped leaf: the minimum may have dropped since the push)
                    double r[REC];
                    build_record(r, g.verts, g.tris, t);
                    const double d = pair_d2(r, p);
                    if (d < best || (d == best && t < bi)) best = d, bi = t;
                }
            } else {
                const MiNode nd = load_node(g.nodes + cur);
                const double d0 = mi_box_d2(p, nd.box[0]), d1 = mi_box_d2(p, nd.box[1]);
                const bool swap = d1 < d0;
                const double dn = swap ? d1 : d0, df = swap ? d0 : d1;
                const int32_t cn = swap ? nd.child[1] : nd.child[0], cf = swap ? nd.child[0] : nd.child[1];
                if (!mi_farther(df, best, m2)) {
                    stk[sp * 64 + lane] = cf;
                    ++sp;
                }
                if (!mi_farther(dn, best, m2)) {
                    cur = cn;
                    continue;
                }
            }
            if (sp == 0) break;
            --sp;
            cur = stk[sp * 64 + lane];
        }
    }
    double d = finite ? sqrt(best) : __builtin_nan("");
    const int32_t idx = bi == INT32_MAX ? -1 : bi;
    if (g.field) {
        const double f = load_real(g.field, g.field_f32, i);
        if (!(f >= g.iso)) d = -d;
    }
    store_real(g.out, g.out_f32, i, d);
    if (g.closest) g.closest[i] = idx;
}

// ---- ray queries against the same tree (include/rho2sdf_hip.h, r2s_mesh_index_raycast; DESIGN.md "Ray queries") -----------
// mi_ray_kernel: one lane per ray, 64 rays per workgroup, the per-lane LDS stack of mi_query_kernel.  A node is read as four
// 16-byte words; both children's parameter intervals come from the slab arithmetic of the header (mr_slab), the child with
// the smaller lower end is entered first and the other one pushed unless its interval is empty or starts behind the best t.
// A popped leaf is tested again against the best t of that moment through its own box, a popped node through its children.
// The pair test is the watertight one of Woop, Benthin and Wald (2013) in double, every operation rounded on its own: the
// edge function of a shared edge is then the exact negative in the neighbouring triangle, which a fused multiply-add would break.
struct MiRay {
    const MiNode* nodes;
    const float* verts;
    const int32_t* tris;
    int64_t ntris;
    int32_t root;
    double absmax;
    const void* org;           // [n][3]
    const void* dir;           // [n][3]
    int rays_f32;
    int64_t n;
    double tmin, tmax;
    void* out;
    int out_f32;
    int32_t* tri;              // may be null
    int8_t* side;              // may be null
};

// the per-ray constants of the node and box tests: o, inv = 1 / d (0 marks d == 0: a reciprocal is never 0), the margin
struct MrSlab {
    double ox, oy, oz, ix, iy, iz, m, tmin, tmax;
};

__device__ inline void mr_axis(double l, double h, double o, double inv, double& lo, double& hi)
{
    if (inv != 0.0) {
        const double t1 = (l - o) * inv, t2 = (h - o) * inv;
        lo = fmax(lo, fmin(t1, t2));     // (fmin / fmax drop a NaN of 0 * inf: that end sets no bound)
        hi = fmin(hi, fmax(t1, t2));
    } else if (!(l <= o && o <= h)) {
        lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    }
}

// [lo, hi]: the ray's parameter interval through the float32 box b (lo xyz, hi xyz) inflated by m, within [tmin, tmax]
__device__ inline void mr_slab(const MrSlab& r, const float* __restrict__ b, double& lo, double& hi)
{
    lo = r.tmin, hi = r.tmax;
    mr_axis((double)b[0] - r.m, (double)b[3] + r.m, r.ox, r.ix, lo, hi);
    mr_axis((double)b[1] - r.m, (double)b[4] + r.m, r.oy, r.iy, lo, hi);
    mr_axis((double)b[2] - r.m, (double)b[5] + r.m, r.oz, r.iz, lo, hi);
}

__device__ inline bool mr_skip(double lo, double hi, double best) { return lo > hi || lo > best; }

// component k of (x, y, z) by selects (an indexed register array would go to scratch)
__device__ inline float mr_pick(const float* __restrict__ p, int k) { return k == 0 ? p[0] : (k == 1 ? p[1] : p[2]); }
__device__ inline double mr_pick(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__global__ void __launch_bounds__(64) mi_ray_kernel(MiRay g)
{
#pragma clang fp contract(off)
    __shared__ int32_t stk[MI_STACK * 64];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    if (i >= g.n) return;
    double ox, oy, oz, dx, dy, dz;
    if (g.rays_f32) {
        const float *q = reinterpret_cast<const float*>(g.org) + 3 * i, *e = reinterpret_cast<const float*>(g.dir) + 3 * i;
        ox = (double)q[0], oy = (double)q[1], oz = (double)q[2], dx = (double)e[0], dy = (double)e[1], dz = (double)e[2];
    } else {
        const double *q = reinterpret_cast<const double*>(g.org) + 3 * i, *e = reinterpret_cast<const double*>(g.dir) + 3 * i;
        ox = q[0], oy = q[1], oz = q[2], dx = e[0], dy = e[1], dz = e[2];
    }
    const bool ok = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) &&
                    (dx != 0.0 || dy != 0.0 || dz != 0.0);
    double best = __builtin_huge_val();
    int32_t bi = INT32_MAX;
    int bs = 0;
    if (ok && g.ntris > 0) {
        MrSlab r;
        r.ox = ox, r.oy = oy, r.oz = oz;
        r.ix = dx != 0.0 ? 1.0 / dx : 0.0, r.iy = dy != 0.0 ? 1.0 / dy : 0.0, r.iz = dz != 0.0 ? 1.0 / dz : 0.0;
        r.m = ldexp(fmax(fmax(fabs(ox), fabs(oy)), fmax(fabs(oz), g.absmax)), -40);
        r.tmin = g.tmin, r.tmax = g.tmax;
        // the shear frame: kz the axis of the largest |d| (lowest on ties), kx, ky the next two cyclically, swapped for d[kz] < 0
        int kz = 0;
        double big = fabs(dx);
        if (fabs(dy) > big) kz = 1, big = fabs(dy);
        if (fabs(dz) > big) kz = 2;
        int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
        const double dkz = mr_pick(dx, dy, dz, kz);
        if (dkz < 0.0) {
            const int s = kx;
            kx = ky, ky = s;
        }
        const double Sx = mr_pick(dx, dy, dz, kx) / dkz, Sy = mr_pick(dx, dy, dz, ky) / dkz, Sz = 1.0 / dkz;
        const double okx = mr_pick(ox, oy, oz, kx), oky = mr_pick(ox, oy, oz, ky), okz = mr_pick(ox, oy, oz, kz);
        int sp = 0;
        int32_t cur = g.root;
        for (;;) {
            if (cur < 0) {
                const int32_t t = ~cur;
                const int32_t* tv = g.tris + 3 * (int64_t)t;
                const float *a = g.verts + 3 * (int64_t)tv[0], *b = g.verts + 3 * (int64_t)tv[1], *c = g.verts + 3 * (int64_t)tv[2];
                const float fa[3] = {a[0], a[1], a[2]}, fb[3] = {b[0], b[1], b[2]}, fc[3] = {c[0], c[1], c[2]};
                float bx[6];
                tri_box(fa, fb, fc, bx, bx + 3);
                double lo, hi;
                mr_slab(r, bx, lo, hi);
                if (!mr_skip(lo, hi, best)) {
                    const double Az = (double)mr_pick(fa, kz) - okz, Bz = (double)mr_pick(fb, kz) - okz, Cz = (double)mr_pick(fc, kz) - okz;
                    const double Ax = ((double)mr_pick(fa, kx) - okx) - Sx * Az, Ay = ((double)mr_pick(fa, ky) - oky) - Sy * Az;
                    const double Bx = ((double)mr_pick(fb, kx) - okx) - Sx * Bz, By = ((double)mr_pick(fb, ky) - oky) - Sy * Bz;
                    const double Cx = ((double)mr_pick(fc, kx) - okx) - Sx * Cz, Cy = ((double)mr_pick(fc, ky) - oky) - Sy * Cz;
                    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
                    const bool mixed = (U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0);
                    const double det = (U + V) + W;
                    if (!mixed && det != 0.0) {
                        const double tt = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det;
                        if (tt >= lo && tt <= hi && (tt < best || (tt == best && t < bi))) best = tt, bi = t, bs = det > 0.0 ? 1 : -1;
                    }
                }
            } else {
                const MiNode nd = load_node(g.nodes + cur);
                double l0, h0, l1, h1;
                mr_slab(r, nd.box[0], l0, h0);
                mr_slab(r, nd.box[1], l1, h1);
                const bool s0 = mr_skip(l0, h0, best), s1 = mr_skip(l1, h1, best);
                const bool swap = s0 || (!s1 && l1 < l0);   // enter child 1 first
                const int32_t cn = swap ? nd.child[1] : nd.child[0], cf = swap ? nd.child[0] : nd.child[1];
                if (!s0 && !s1) {
                    stk[sp * 64 + lane] = cf;
                    ++sp;
                }
                if (!(s0 && s1)) {
                    cur = cn;
                    continue;
                }
            }
            if (sp == 0) break;
            --sp;
            cur = stk[sp * 64 + lane];
        }
    }
    const double tt = ok ? best + 0.0 : __builtin_nan("");   // (-0 -> +0: a zero t must not depend on which triangle gave it)
    store_real(g.out, g.out_f32, i, tt);
    if (g.tri) g.tri[i] = bi == INT32_MAX ? -1 : bi;
    if (g.side) g.side[i] = (int8_t)bs;
}

}  // namespace

namespace r2s_int {

// the traversal kernels keep one pending sibling per level on a per-lane stack of MI_STACK entries
int check_depth(const MiTree& T)
{
    if (T.depth <= MI_STACK) return 0;
    return fail(R2S_ERR_UNSUPPORTED, "mesh_index: tree depth %d exceeds the traversal stack of %d entries", T.depth, MI_STACK);
}

int index_on_current_device(const char* who, const r2s_mesh_index* ix)
{
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ix->device) return fail(R2S_ERR_ARG, "%s: the index lives on device %d, the current device is %d", who, ix->device, dev);
    return 0;
}

}  // namespace r2s_int

namespace {

int query_args(const char* who, const r2s_mesh_index* ix, const void* points, int64_t n, const void* out)
{
    if (!ix) return fail(R2S_ERR_ARG, "%s: null index", who);
    if (n < 0) return fail(R2S_ERR_ARG, "%s: negative point count", who);
    if (n > 0 && (!points || !out)) return fail(R2S_ERR_ARG, "%s: null points / output", who);
    if (n > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "%s: %lld points exceed one call", who, (long long)n);
    return 0;
}

int ray_args(const char* who, const r2s_mesh_index* ix, const void* origins, const void* dirs, int64_t n, double t_min, double t_max,
             const void* out)
{
    if (!ix) return fail(R2S_ERR_ARG, "%s: null index", who);
    if (n < 0) return fail(R2S_ERR_ARG, "%s: negative ray count", who);
    if (std::isnan(t_min) || std::isnan(t_max)) return fail(R2S_ERR_ARG, "%s: t_min / t_max is NaN", who);
    if (t_min > t_max) return fail(R2S_ERR_ARG, "%s: t_min > t_max", who);
    if (n > 0 && (!origins || !dirs || !out)) return fail(R2S_ERR_ARG, "%s: null origins / directions / output", who);
    if (n > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "%s: %lld rays exceed one call", who, (long long)n);
    return 0;
}

// enqueues the n > 0 rays on `st`; does not wait
int mi_raycast(const MiTree& T, const void* d_org, const void* d_dir, bool rays_f32, int64_t n, double t_min, double t_max, void* d_out,
               bool out_f32, int32_t* d_tri, int8_t* d_side, hipStream_t st)
{
    if (const int rc = check_depth(T)) return rc;
    MiRay g = {};
    g.nodes = T.nodes.as<MiNode>();
    g.verts = T.verts, g.tris = T.tris, g.ntris = T.n_tris, g.root = T.root, g.absmax = T.absmax;
    g.org = d_org, g.dir = d_dir, g.rays_f32 = rays_f32 ? 1 : 0, g.n = n;
    g.tmin = t_min, g.tmax = t_max;
    g.out = d_out, g.out_f32 = out_f32 ? 1 : 0, g.tri = d_tri, g.side = d_side;
    mi_ray_kernel<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the new index of a mesh that `fill` uploads and builds the tree of, on the current device
template <class F>
int new_index(r2s_mesh_index** out, F fill)
{
    r2s_mesh_index* ix = new r2s_mesh_index;
    int rc = hipGetDevice(&ix->device) == hipSuccess ? fill(ix) : fail(R2S_ERR_HIP, "hipGetDevice failed");
    if (rc) {
        r2s_mesh_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return 0;
}

}  // namespace

namespace r2s_int {

int mi_build_tree(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, hipStream_t st, MiTree& T)
{
    T.verts = d_verts, T.tris = d_tris, T.n_verts = n_verts, T.n_tris = n_tris;
    T.root = 0, T.depth = 0, T.absmax = 0.0;
    if (n_tris == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    const unsigned blocks = (unsigned)((n_tris + 255) / 256);
    DevBuf small, keys, sorted, temp, parent, flags;
    // small: [0..5] the bounds, [6] the depth
    uint32_t h_small[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    ENSURE(small, sizeof h_small);
    HIP_TRY(hipMemcpyAsync(small.p, h_small, sizeof h_small, hipMemcpyHostToDevice, st));
    mi_bounds_kernel<<<blocks, 256, 0, st>>>(d_verts, d_tris, n_tris, small.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_small, small.p, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    MiFrame f;
    for (int k = 0; k < 3; ++k) {
        const double lo = (double)mi_unordered(h_small[k]), hi = (double)mi_unordered(h_small[3 + k]);
        f.lo[k] = lo;
        f.scale[k] = hi > lo ? 1024.0 / (hi - lo) : 0.0;
        T.absmax = std::max(T.absmax, std::max(std::fabs(lo), std::fabs(hi)));
    }
    if (n_tris == 1) {
        T.root = ~0;   // (nothing to sort: the root is the leaf of triangle 0)
        return 0;
    }
    ENSURE(keys, sizeof(uint64_t) * (size_t)n_tris);
    ENSURE(sorted, sizeof(uint64_t) * (size_t)n_tris);
    mi_key_kernel<<<blocks, 256, 0, st>>>(d_verts, d_tris, n_tris, f, keys.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, temp_bytes, keys.as<uint64_t>(), sorted.as<uint64_t>(), (size_t)n_tris, 0u, 62u, st));
    ENSURE(temp, std::max<size_t>(temp_bytes, 16));
    HIP_TRY(rocprim::radix_sort_keys(temp.p, temp_bytes, keys.as<uint64_t>(), sorted.as<uint64_t>(), (size_t)n_tris, 0u, 62u, st));
    if (T.nodes.ensure_exact(sizeof(MiNode) * (size_t)(n_tris - 1)))
        return fail(R2S_ERR_NOMEM, "mesh_index: hipMalloc of %zu bytes for the tree failed", sizeof(MiNode) * (size_t)(n_tris - 1));
    ENSURE(parent, sizeof(uint32_t) * (size_t)(2 * n_tris - 1));
    ENSURE(flags, sizeof(int32_t) * (size_t)(n_tris - 1));
    HIP_TRY(hipMemsetAsync(flags.p, 0, sizeof(int32_t) * (size_t)(n_tris - 1), st));
    mi_tree_kernel<<<blocks, 256, 0, st>>>(sorted.as<uint64_t>(), n_tris, T.nodes.as<MiNode>(), parent.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    mi_refit_kernel<<<blocks, 256, 0, st>>>(d_verts, d_tris, sorted.as<uint64_t>(), n_tris, T.nodes.as<MiNode>(), parent.as<uint32_t>(),
                                          flags.as<int32_t>(), small.as<int32_t>() + 6);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&T.depth, small.as<int32_t>() + 6, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    T.root = 0;
    return 0;
}

int mi_query(const MiTree& T, const void* d_pts, bool pts_f32, int64_t n, const int64_t* dims, const double* origin, double spacing,
             const void* d_field, bool field_f32, double iso, void* d_out, bool out_f32, int32_t* d_closest, hipStream_t st)
{
    if (const int rc = check_depth(T)) return rc;
    MiQuery g = {};
    g.nodes = T.nodes.as<MiNode>();
    g.verts = T.verts, g.tris = T.tris, g.ntris = T.n_tris, g.root = T.root, g.absmax = T.absmax;
    g.field = d_field, g.field_f32 = field_f32 ? 1 : 0, g.iso = iso;
    g.out = d_out, g.out_f32 = out_f32 ? 1 : 0, g.closest = d_closest;
    if (dims) {
        g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
        g.nbx = (g.nx + 3) / 4, g.nby = (g.ny + 3) / 4;
        const int64_t nb = g.nbx * g.nby * ((g.nz + 3) / 4);
        if (nb > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "mesh_index: %lld voxel blocks exceed one launch", (long long)nb);
        for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
        g.h = spacing;
        mi_query_kernel<true><<<(unsigned)nb, 64, 0, st>>>(g);
    } else {
        if (n == 0) return 0;
        g.pts = d_pts, g.pts_f32 = pts_f32 ? 1 : 0, g.n = n;
        mi_query_kernel<false><<<(unsigned)((n + 63) / 64), 64, 0, st>>>(g);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace r2s_int

extern "C" {

int r2s_mesh_index_build(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device, r2s_mesh_index** out)
{
    int rc = mesh_args("mesh_index_build", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (!out) return fail(R2S_ERR_ARG, "mesh_index_build: null output");
    if ((rc = check_mesh_host("mesh_index_build", verts, n_verts, tris, n_tris)) || (rc = check_device(device < 0 ? 0 : device))) return rc;
    DeviceScope scope;   // (device < 0: the current device)
    if (device >= 0 && (rc = scope.enter(device))) return rc;
    return new_index(out, [&](r2s_mesh_index* ix) {
        const int rc = upload_mesh(ix->verts, ix->tris, verts, n_verts, tris, n_tris, false, nullptr);
        return rc ? rc : mi_build_tree(ix->verts.as<float>(), n_verts, ix->tris.as<int32_t>(), n_tris, nullptr, ix->tree);
    });
}

int r2s_mesh_index_build_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, void* stream,
                             r2s_mesh_index** out)
{
    int rc = mesh_args("mesh_index_build", d_verts, n_verts, d_tris, n_tris);
    if (rc) return rc;
    if (!out) return fail(R2S_ERR_ARG, "mesh_index_build: null output");
    if ((rc = check_device(0))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    DevBuf flag;
    if ((rc = check_mesh_dev("mesh_index_build", d_verts, n_verts, d_tris, n_tris, flag, st))) return rc;
    return new_index(out, [&](r2s_mesh_index* ix) {
        const int rc = upload_mesh(ix->verts, ix->tris, d_verts, n_verts, d_tris, n_tris, true, st);
        return rc ? rc : mi_build_tree(ix->verts.as<float>(), n_verts, ix->tris.as<int32_t>(), n_tris, st, ix->tree);
    });
}

void r2s_mesh_index_destroy(r2s_mesh_index* ix)
{
    if (!ix) return;
    const int device = ix->device;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) (void)hipSetDevice(device);
    delete ix;   // frees the mesh and the tree
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}

int r2s_mesh_index_info(const r2s_mesh_index* ix, int64_t out[4])
{
    if (!ix || !out) return fail(R2S_ERR_ARG, "mesh_index_info: null index / output");
    out[0] = ix->tree.n_tris;
    out[1] = ix->tree.n_tris > 0 ? 2 * ix->tree.n_tris - 1 : 0;
    out[2] = ix->tree.depth;
    out[3] = (int64_t)(ix->verts.cap + ix->tris.cap + ix->tree.nodes.cap);
    return 0;
}

int r2s_mesh_index_query(const r2s_mesh_index* ix, const void* points, int32_t points_are_float32, int64_t n, int32_t out_is_float32,
                         void* dist_out, int32_t* closest_tri_out)
{
    int rc = query_args("mesh_index_query", ix, points, n, dist_out);
    if (rc || n == 0) return rc;
    const size_t np = (size_t)n, psz = 3 * real_bytes(points_are_float32) * np, osz = real_bytes(out_is_float32) * np;
    const HostIo pts{points, nullptr, psz}, out{nullptr, dist_out, osz}, idx{nullptr, closest_tri_out, sizeof(int32_t) * np};
    return staged_call(ix, {pts, out, idx}, [&](DevBuf* b) {
        return mi_query(ix->tree, b[0].p, points_are_float32 != 0, n, nullptr, nullptr, 0.0, nullptr, false, 0.0, b[1].p, out_is_float32 != 0,
                        b[2].as<int32_t>(), nullptr);
    });
}

int r2s_mesh_index_query_dev(const r2s_mesh_index* ix, const void* d_points, int32_t points_are_float32, int64_t n, int32_t out_is_float32,
                             void* d_dist_out, int32_t* d_closest_tri_out, void* stream)
{
    int rc = query_args("mesh_index_query", ix, d_points, n, d_dist_out);
    if (rc || n == 0) return rc;
    if ((rc = check_device(0)) || (rc = index_on_current_device("mesh_index_query", ix))) return rc;
    return mi_query(ix->tree, d_points, points_are_float32 != 0, n, nullptr, nullptr, 0.0, nullptr, false, 0.0, d_dist_out,
                    out_is_float32 != 0, d_closest_tri_out, (hipStream_t)stream);
}

int r2s_mesh_index_raycast(const r2s_mesh_index* ix, const void* origins, const void* dirs, int32_t rays_are_float32, int64_t n,
                           double t_min, double t_max, int32_t out_is_float32, void* t_out, int32_t* tri_out, int8_t* side_out)
{
    int rc = ray_args("mesh_index_raycast", ix, origins, dirs, n, t_min, t_max, t_out);
    if (rc || n == 0) return rc;
    const size_t nr = (size_t)n, psz = 3 * real_bytes(rays_are_float32) * nr, osz = real_bytes(out_is_float32) * nr;
    const HostIo org{origins, nullptr, psz}, dir{dirs, nullptr, psz}, out{nullptr, t_out, osz}, idx{nullptr, tri_out, sizeof(int32_t) * nr},
        side{nullptr, side_out, nr};
    return staged_call(ix, {org, dir, out, idx, side}, [&](DevBuf* b) {
        return mi_raycast(ix->tree, b[0].p, b[1].p, rays_are_float32 != 0, n, t_min, t_max, b[2].p, out_is_float32 != 0, b[3].as<int32_t>(),
                          b[4].as<int8_t>(), nullptr);
    });
}

int r2s_mesh_index_raycast_dev(const r2s_mesh_index* ix, const void* d_origins, const void* d_dirs, int32_t rays_are_float32, int64_t n,
                               double t_min, double t_max, int32_t out_is_float32, void* d_t_out, int32_t* d_tri_out, int8_t* d_side_out,
                               void* stream)
{
    int rc = ray_args("mesh_index_raycast", ix, d_origins, d_dirs, n, t_min, t_max, d_t_out);
    if (rc || n == 0) return rc;
    if ((rc = check_device(0)) || (rc = index_on_current_device("mesh_index_raycast", ix))) return rc;
    return mi_raycast(ix->tree, d_origins, d_dirs, rays_are_float32 != 0, n, t_min, t_max, d_t_out, out_is_float32 != 0, d_tri_out,
                      d_side_out, (hipStream_t)stream);
}

int r2s_mesh_index_lattice(const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing, int32_t out_is_float32,
                           void* dist_out, int32_t* closest_tri_out)
{
    int rc = lattice_args("mesh_index_lattice", dims, origin, spacing, 1.0);
    if (rc) return rc;
    if (!ix || !dist_out) return fail(R2S_ERR_ARG, "mesh_index_lattice: null index / output");
    const size_t nvox = (size_t)(dims[0] * dims[1] * dims[2]);
    const HostIo out{nullptr, dist_out, real_bytes(out_is_float32) * nvox}, idx{nullptr, closest_tri_out, sizeof(int32_t) * nvox};
    return staged_call(ix, {out, idx}, [&](DevBuf* b) {
        return mi_query(ix->tree, nullptr, false, 0, dims, origin, spacing, nullptr, false, 0.0, b[0].p, out_is_float32 != 0,
                        b[1].as<int32_t>(), nullptr);
    });
}

int r2s_mesh_index_lattice_dev(const r2s_mesh_index* ix, const int64_t dims[3], const double origin[3], double spacing,
                               int32_t out_is_float32, void* d_dist_out, int32_t* d_closest_tri_out, void* stream)
{
    int rc = lattice_args("mesh_index_lattice", dims, origin, spacing, 1.0);
    if (rc) return rc;
    if (!ix || !d_dist_out) return fail(R2S_ERR_ARG, "mesh_index_lattice: null index / output");
    if ((rc = check_device(0)) || (rc = index_on_current_device("mesh_index_lattice", ix))) return rc;
    return mi_query(ix->tree, nullptr, false, 0, dims, origin, spacing, nullptr, false, 0.0, d_dist_out, out_is_float32 != 0,
                    d_closest_tri_out, (hipStream_t)stream);
}

}  // extern "C"
