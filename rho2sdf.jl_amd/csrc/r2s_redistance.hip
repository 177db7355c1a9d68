// Redistancing: the exact Euclidean distance from the points of a regular lattice to an indexed triangle mesh within a band,
// and the signed form on the iso-surface of a field (include/rho2sdf_hip.h, r2s_mesh_distance / r2s_redistance).
//
// Layout (DESIGN.md "Redistancing"):
//   1. md_bin_kernel<false>: one thread per triangle counts, per 8x8x8 voxel tile, the triangles whose AABB lies within the
//      band of the tile's box (box-to-box distance in double, with the margin below) - integer atomics only;
//   2. md_scan_kernel: exclusive 64-bit scan of the tile counts (one workgroup, no atomics);
//   3. per batch of tile layers (the pair list of a batch stays under the workspace budget): md_bin_kernel<true> fills the
//      batch's tile lists, md_tile_kernel runs one workgroup per tile of the batch.
// md_tile_kernel: 4 waves, every lane owns two voxels (x, y, z) and (x, y, z + 1) of its wave's 8x8x2 slab.  The tile's list is
// streamed through LDS in chunks of CHUNK triangle records that the workgroup builds from the float32 vertices (edges, normal,
// in-plane edge normals, reciprocals, AABB: all wave-uniform, read back as LDS broadcasts).  Per chunk every wave reduces the
// worst of its lanes' running minima (clamped to the band) and skips every triangle whose AABB is farther from the wave's
// voxel block than that.  Every lane keeps a running (d^2, index) with the lexicographic minimum, takes one sqrt at the end,
// applies band and sign and stores.  Tiles without triangles store +-band in the same kernel.
//
// Order independence: the order of a tile's list comes from an integer atomic cursor and is not reproducible, the result is:
// (d^2, index) is reduced with the lexicographic minimum, which is exact and commutative, and both culls are conservative by
// a margin (MdArgs::margin, 2^-40 of the largest coordinate, far above the rounding of a pair's distance and far below anything the
// bound of the tests can see): a skipped triangle is strictly farther than the lane's current minimum or than the band.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"

// the tree of a mesh index and the mesh it refers to (r2s_mesh_index owns all three; redistance_full borrows the mesh)
struct MiTree {
    const float* verts = nullptr;
    const int32_t* tris = nullptr;
    int64_t n_verts = 0, n_tris = 0;
    DevBuf nodes;
    int32_t root = 0;
    int32_t depth = 0;
    double absmax = 0.0;
};
struct r2s_mesh_index {
    int device = 0;
    DevBuf verts, tris;
    MiTree tree;
};

namespace {

constexpr int TS = 8;          // voxels per tile edge
constexpr int CHUNK = 128;     // triangle records per LDS chunk
constexpr int REC = 40;        // doubles per record
// record layout (doubles): a 0-2, b 3-5, ab 6-8, ac 9-11, bc 12-14, n 15-17, n x ab 18-20, n x ac 21-23, n x bc 24-26,
// 1/ab.ab 27, 1/ac.ac 28, 1/bc.bc 29, 1/n.n 30 (0 = the feature is degenerate), AABB lo 31-33, hi 34-36, index 37 (as int64)

struct MdArgs {
    int64_t nx, ny, nz;        // lattice points
    int64_t ntx, nty, ntz;     // tiles
    double o[3];
    double h, band, bandm;     // bandm = band + 2 * margin
    double margin;
    int64_t ntris;
};

struct Vec3 {
    double x, y, z;
};
__device__ __host__ inline Vec3 sub(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __host__ inline double dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __host__ inline Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// a*b - c*d with at most 1.5 ulp of error (Kahan's difference of products; the explicit fma is kept under -ffp-contract=off)
__device__ inline double diff_of_products(double a, double b, double c, double d)
{
    const double w = c * d;
    const double e = fma(-c, d, w);
    const double f = fma(a, b, -w);
    return f + e;
}
// the normal of a triangle must keep its direction when the edges are nearly parallel (slivers): with plain products the
// cancellation tilts the plane by 2^-53 / aspect, which shows as an error of that times the triangle's length
__device__ inline Vec3 cross_exact(Vec3 a, Vec3 b)
{
    return {diff_of_products(a.y, b.z, a.z, b.y), diff_of_products(a.z, b.x, a.x, b.z), diff_of_products(a.x, b.y, a.y, b.x)};
}

__device__ inline Vec3 load_vert(const float* __restrict__ v, int32_t i)
{
    const float* p = v + 3 * (int64_t)i;
    return {(double)p[0], (double)p[1], (double)p[2]};
}

__device__ inline double lattice(const MdArgs& g, int a, int64_t i) { return g.o[a] + g.h * (double)i; }

__device__ inline double gap(double alo, double ahi, double blo, double bhi)
{
    const double g0 = alo - bhi, g1 = blo - ahi;
    const double g = g0 > g1 ? g0 : g1;
    return g > 0.0 ? g : 0.0;
}

// conservative range of lattice indices within `r` of [lo, hi] on one axis, clamped to [0, n - 1]; false = none
__device__ inline bool index_range(double lo, double hi, double r, double o, double h, int64_t n, int64_t& i0, int64_t& i1)
{
    double a = floor((lo - r - o) / h) - 1.0, b = ceil((hi + r - o) / h) + 1.0;
    if (!(b >= 0.0) || !(a <= (double)(n - 1))) return false;
    a = a > 0.0 ? a : 0.0;
    b = b < (double)(n - 1) ? b : (double)(n - 1);
    i0 = (int64_t)a;
    i1 = (int64_t)b;
    return i0 <= i1;
}

// FILL = false: cnt[tile] += 1 for every tile within the band of triangle t's AABB.  FILL = true: only tile layers
// [lz0, lz1); cnt is the zeroed cursor array and list[off[tile] - off0 + cursor] = t.
template <bool FILL>
__global__ void __launch_bounds__(256) md_bin_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris, MdArgs g,
                                                      uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint64_t off0,
                                                      int64_t lz0, int64_t lz1, int32_t* __restrict__ list)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= g.ntris) return;
    const Vec3 a = load_vert(verts, tris[3 * t]), b = load_vert(verts, tris[3 * t + 1]), c = load_vert(verts, tris[3 * t + 2]);
    const double lo[3] = {fmin(a.x, fmin(b.x, c.x)), fmin(a.y, fmin(b.y, c.y)), fmin(a.z, fmin(b.z, c.z))};
    const double hi[3] = {fmax(a.x, fmax(b.x, c.x)), fmax(a.y, fmax(b.y, c.y)), fmax(a.z, fmax(b.z, c.z))};
    int64_t i0[3], i1[3];
    const int64_t n[3] = {g.nx, g.ny, g.nz};
    for (int ax = 0; ax < 3; ++ax)
        if (!index_range(lo[ax], hi[ax], g.bandm, g.o[ax], g.h, n[ax], i0[ax], i1[ax])) return;
    int64_t tz0 = i0[2] / TS, tz1 = i1[2] / TS;
    if (FILL) {
        tz0 = tz0 > lz0 ? tz0 : lz0;
        tz1 = tz1 < lz1 - 1 ? tz1 : lz1 - 1;
    }
    const double r2 = g.bandm * g.bandm;
    for (int64_t tz = tz0; tz <= tz1; ++tz) {
        const int64_t ze = tz * TS + TS - 1 < g.nz - 1 ? tz * TS + TS - 1 : g.nz - 1;
        const double gz = gap(lo[2], hi[2], lattice(g, 2, tz * TS), lattice(g, 2, ze));
        if (gz * gz > r2) continue;
        for (int64_t ty = i0[1] / TS; ty <= i1[1] / TS; ++ty) {
            const int64_t ye = ty * TS + TS - 1 < g.ny - 1 ? ty * TS + TS - 1 : g.ny - 1;
            const double gy = gap(lo[1], hi[1], lattice(g, 1, ty * TS), lattice(g, 1, ye));
            const double gyz = gy * gy + gz * gz;
            if (gyz > r2) continue;
            for (int64_t tx = i0[0] / TS; tx <= i1[0] / TS; ++tx) {
                const int64_t xe = tx * TS + TS - 1 < g.nx - 1 ? tx * TS + TS - 1 : g.nx - 1;
                const double gx = gap(lo[0], hi[0], lattice(g, 0, tx * TS), lattice(g, 0, xe));
                if (gx * gx + gyz > r2) continue;
                const int64_t tile = (tz * g.nty + ty) * g.ntx + tx;
                const uint32_t pos = atomicAdd(&cnt[tile], 1u);
                if (FILL) list[off[tile] - off0 + pos] = (int32_t)t;
            }
        }
    }
}

// off[0 .. n] = exclusive scan of cnt[0 .. n) in 64 bits (one workgroup)
__global__ void __launch_bounds__(1024) md_scan_kernel(const uint32_t* __restrict__ cnt, int64_t n, uint64_t* __restrict__ off)
{
    __shared__ uint64_t ws[16];
    const int64_t per = (n + 1023) / 1024, b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t s = 0;
    for (int64_t b = b0; b < b1; ++b) s += cnt[b];
    unsigned long long x = s;   // inclusive scan over the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long v = __shfl_up(x, d, 64);
        if (lane >= d) x += v;
    }
    if (lane == 63) ws[wave] = x;
    __syncthreads();
    uint64_t o = 0;
    for (int w = 0; w < wave; ++w) o += ws[w];
    if (threadIdx.x == 1023) off[n] = o + x;
    uint64_t run = o + x - s;
    for (int64_t b = b0; b < b1; ++b) {
        off[b] = run;
        run += cnt[b];
    }
}

// flag[0] = 1 when a triangle index lies outside [0, nverts) or a vertex coordinate is not finite
__global__ void __launch_bounds__(256) md_check_kernel(const float* __restrict__ verts, int64_t nverts, const int32_t* __restrict__ tris,
                                                        int64_t ntris, int32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < 3 * ntris) bad = tris[i] < 0 || (int64_t)tris[i] >= nverts;
    if (i < 3 * nverts) bad = bad || !isfinite(verts[i]);
    if (bad) flag[0] = 1;
}

// squared distance from p to the segment u + t e, t in [0, 1]; w = p - u, inv = 1 / e.e (0 for a zero-length segment)
__device__ inline double seg_d2(Vec3 w, Vec3 e, double inv)
{
    double t = dot(w, e) * inv;
    t = t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t;
    const Vec3 q = {w.x - t * e.x, w.y - t * e.y, w.z - t * e.z};
    return dot(q, q);
}

// squared distance from p to the triangle of record r (the definition of the header)
__device__ inline double pair_d2(const double* __restrict__ r, Vec3 p)
{
    const Vec3 a = {r[0], r[1], r[2]}, b = {r[3], r[4], r[5]};
    const Vec3 ab = {r[6], r[7], r[8]}, ac = {r[9], r[10], r[11]}, bc = {r[12], r[13], r[14]};
    const Vec3 ap = sub(p, a), bp = sub(p, b);
    double d2 = seg_d2(ap, ab, r[27]);
    const double d_ac = seg_d2(ap, ac, r[28]);
    d2 = d_ac < d2 ? d_ac : d2;
    const double d_bc = seg_d2(bp, bc, r[29]);
    d2 = d_bc < d2 ? d_bc : d2;
    const double inv_nn = r[30];
    if (inv_nn > 0.0) {
        const Vec3 mab = {r[18], r[19], r[20]}, mac = {r[21], r[22], r[23]}, mbc = {r[24], r[25], r[26]};
        // edge functions (ab x ap).n, (bc x bp).n, (ca x cp).n as dot products with the in-plane edge normals
        if (dot(ap, mab) >= 0.0 && dot(bp, mbc) >= 0.0 && -dot(ap, mac) >= 0.0) {
            const Vec3 n = {r[15], r[16], r[17]};
            const double s = dot(n, ap);
            const double dp = s * s * inv_nn;
            d2 = dp < d2 ? dp : d2;
        }
    }
    return d2;
}

__device__ inline void build_record(double* __restrict__ r, const float* __restrict__ verts, const int32_t* __restrict__ tris, int32_t t)
{
    const Vec3 a = load_vert(verts, tris[3 * (int64_t)t]), b = load_vert(verts, tris[3 * (int64_t)t + 1]),
               c = load_vert(verts, tris[3 * (int64_t)t + 2]);
    const Vec3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
    const Vec3 n = cross_exact(ab, ac);
    const Vec3 mab = cross(n, ab), mac = cross(n, ac), mbc = cross(n, bc);
    const double eab = dot(ab, ab), eac = dot(ac, ac), ebc = dot(bc, bc), nn = dot(n, n);
    r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = b.x, r[4] = b.y, r[5] = b.z;
    r[6] = ab.x, r[7] = ab.y, r[8] = ab.z, r[9] = ac.x, r[10] = ac.y, r[11] = ac.z, r[12] = bc.x, r[13] = bc.y, r[14] = bc.z;
    r[15] = n.x, r[16] = n.y, r[17] = n.z;
    r[18] = mab.x, r[19] = mab.y, r[20] = mab.z, r[21] = mac.x, r[22] = mac.y, r[23] = mac.z, r[24] = mbc.x, r[25] = mbc.y, r[26] = mbc.z;
    r[27] = eab > 0.0 ? 1.0 / eab : 0.0;
    r[28] = eac > 0.0 ? 1.0 / eac : 0.0;
    r[29] = ebc > 0.0 ? 1.0 / ebc : 0.0;
    const double inn = nn > 0.0 ? 1.0 / nn : 0.0;
    r[30] = isfinite(inn) ? inn : 0.0;   // (n.n underflowed: the plane term is not counted, the segments cover the triangle)
    r[31] = fmin(a.x, fmin(b.x, c.x)), r[32] = fmin(a.y, fmin(b.y, c.y)), r[33] = fmin(a.z, fmin(b.z, c.z));
    r[34] = fmax(a.x, fmax(b.x, c.x)), r[35] = fmax(a.y, fmax(b.y, c.y)), r[36] = fmax(a.z, fmax(b.z, c.z));
    reinterpret_cast<int64_t*>(r)[37] = (int64_t)t;
}

__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One workgroup per tile tile0 + blockIdx.x.  field (may be null): the sign is +1 where field >= iso, else -1 (NaN: -1).
__global__ void __launch_bounds__(256) md_tile_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris, MdArgs g,
                                                       const uint64_t* __restrict__ off, uint64_t off0, int64_t tile0,
                                                       const int32_t* __restrict__ list, const void* __restrict__ field,
                                                       int field_f32, double iso, void* __restrict__ out, int out_f32,
                                                       int32_t* __restrict__ closest)
{
    __shared__ double rec[CHUNK * REC];
    const int64_t tile = tile0 + (int64_t)blockIdx.x;
    const int64_t tx = tile % g.ntx, ty = (tile / g.ntx) % g.nty, tz = tile / (g.ntx * g.nty);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ix = tx * TS + (lane & 7), iy = ty * TS + (lane >> 3), iz = tz * TS + 2 * wave;
    const bool va = ix < g.nx && iy < g.ny && iz < g.nz, vb = va && iz + 1 < g.nz;
    const uint64_t beg = off[tile], cntl = off[tile + 1] - beg;
    const int32_t* __restrict__ my = list + (beg - off0);

    const double px = lattice(g, 0, ix), py = lattice(g, 1, iy);
    const Vec3 pa = {px, py, lattice(g, 2, iz)}, pb = {px, py, lattice(g, 2, iz + 1)};
    // the wave's voxel block, clipped to the lattice
    const int64_t xe = tx * TS + TS - 1 < g.nx - 1 ? tx * TS + TS - 1 : g.nx - 1;
    const int64_t ye = ty * TS + TS - 1 < g.ny - 1 ? ty * TS + TS - 1 : g.ny - 1;
    const int64_t zs = iz < g.nz - 1 ? iz : g.nz - 1, ze = iz + 1 < g.nz - 1 ? iz + 1 : g.nz - 1;
    const double blo[3] = {lattice(g, 0, tx * TS), lattice(g, 1, ty * TS), lattice(g, 2, zs)};
    const double bhi[3] = {lattice(g, 0, xe), lattice(g, 1, ye), lattice(g, 2, ze)};

    const double INF = __builtin_huge_val();
    const double band2m = g.bandm * g.bandm;
    double da = INF, db = INF;
    int32_t ia = INT32_MAX, ib = INT32_MAX;
    for (uint64_t base = 0; base < cntl; base += CHUNK) {
        const int nc = cntl - base < (uint64_t)CHUNK ? (int)(cntl - base) : CHUNK;
        __syncthreads();   // (the previous chunk's records are no longer read)
        if ((int)threadIdx.x < nc) build_record(rec + (int)threadIdx.x * REC, verts, tris, my[base + threadIdx.x]);
        __syncthreads();
        // the worst running minimum of the wave's voxels, clamped to the band: nothing farther can change a result
        double worst = va ? (da < band2m ? da : band2m) : 0.0;
        const double wb = vb ? (db < band2m ? db : band2m) : 0.0;
        worst = wave_max(wb > worst ? wb : worst);
        const double wr = sqrt(worst) + 2.0 * g.margin;
        const double thr2 = wr * wr;
        for (int j = 0; j < nc; ++j) {
            const double* __restrict__ r = rec + j * REC;
            const double gx = gap(r[31], r[34], blo[0], bhi[0]), gy = gap(r[32], r[35], blo[1], bhi[1]),
                         gz = gap(r[33], r[36], blo[2], bhi[2]);
            if (gx * gx + gy * gy + gz * gz > thr2) continue;   // wave-uniform
            const int32_t t = (int32_t)reinterpret_cast<const int64_t*>(r)[37];
            const double d0 = pair_d2(r, pa), d1 = pair_d2(r, pb);
            if (d0 < da || (d0 == da && t < ia)) da = d0, ia = t;
            if (d1 < db || (d1 == db && t < ib)) db = d1, ib = t;
        }
    }
    // epilogue: one sqrt, band, sign, store
    for (int v = 0; v < 2; ++v) {
        if (!(v ? vb : va)) continue;
        const int64_t i = ((iz + v) * g.ny + iy) * g.nx + ix;
        const double d2 = v ? db : da;
        int32_t idx = v ? ib : ia;
        double d = sqrt(d2);
        if (idx == INT32_MAX || !(d < g.band)) d = g.band, idx = -1;
        if (field) {
            const double f = field_f32 ? (double)reinterpret_cast<const float*>(field)[i] : reinterpret_cast<const double*>(field)[i];
            if (!(f >= iso)) d = -d;
        }
        if (out_f32)
            reinterpret_cast<float*>(out)[i] = (float)d;
        else
            reinterpret_cast<double*>(out)[i] = d;
        if (closest) closest[i] = idx;
    }
}

// ---- mesh index: a linear BVH over the triangles and one stack traversal per query point (DESIGN.md "Mesh index") ---------
// Build: mi_bounds_kernel (mesh AABB, integer atomics on order-preserving bit patterns) -> mi_key_kernel (30-bit Morton code
// of the triangle's AABB centre << 32 | triangle index: unique keys) -> rocPRIM radix sort -> mi_tree_kernel (Karras 2012, one
// thread per internal node) -> mi_refit_kernel (one thread per leaf walks up; the second arrival at a node, counted by an
// integer flag, joins the two child boxes and carries the height on).  A node holds the float32 boxes of its two children,
// the children (>= 0: internal node, < 0: the leaf of triangle ~child) and their heights: 64 bytes, four 16-byte loads.
// Query: mi_query_kernel, one lane per point, the nearer child first, the other pushed on a per-lane LDS stack of MI_STACK
// entries.  A leaf builds the record of md_tile_kernel (build_record) in registers and calls pair_d2: the same arithmetic,
// hence the same numbers wherever both kernels answer.
constexpr int MI_STACK = 64;   // stack entries per lane; a tree of height h needs at most h (one pending sibling per level)
constexpr uint32_t MI_ROOT = 0xffffffffu;

struct MiNode {
    float box[2][6];      // child c: lo xyz, hi xyz
    int32_t child[2];
    int32_t height[2];    // 0 = leaf
};
static_assert(sizeof(MiNode) == 64, "MiNode is read as four 16-byte words");

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
    const float *a = verts + 3 * (int64_t)tris[3 * t], *b = verts + 3 * (int64_t)tris[3 * t + 1], *c = verts + 3 * (int64_t)tris[3 * t + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(a[k], fminf(b[k], c[k]));
        hi[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
    }
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
                const uint4* w = reinterpret_cast<const uint4*>(g.nodes + cur);
                union {
                    uint4 q[4];
                    MiNode n;
                } u;
                u.q[0] = w[0], u.q[1] = w[1], u.q[2] = w[2], u.q[3] = w[3];
                const double d0 = mi_box_d2(p, u.n.box[0]), d1 = mi_box_d2(p, u.n.box[1]);
                const bool swap = d1 < d0;
                const double dn = swap ? d1 : d0, df = swap ? d0 : d1;
                const int32_t cn = swap ? u.n.child[1] : u.n.child[0], cf = swap ? u.n.child[0] : u.n.child[1];
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
        const double f = g.field_f32 ? (double)reinterpret_cast<const float*>(g.field)[i] : reinterpret_cast<const double*>(g.field)[i];
        if (!(f >= g.iso)) d = -d;
    }
    if (g.out_f32)
        reinterpret_cast<float*>(g.out)[i] = (float)d;
    else
        reinterpret_cast<double*>(g.out)[i] = d;
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
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    bx[k] = fminf(fa[k], fminf(fb[k], fc[k]));
                    bx[3 + k] = fmaxf(fa[k], fmaxf(fb[k], fc[k]));
                }
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
                const uint4* w = reinterpret_cast<const uint4*>(g.nodes + cur);
                union {
                    uint4 q[4];
                    MiNode n;
                } u;
                u.q[0] = w[0], u.q[1] = w[1], u.q[2] = w[2], u.q[3] = w[3];
                double l0, h0, l1, h1;
                mr_slab(r, u.n.box[0], l0, h0);
                mr_slab(r, u.n.box[1], l1, h1);
                const bool s0 = mr_skip(l0, h0, best), s1 = mr_skip(l1, h1, best);
                const bool swap = s0 || (!s1 && l1 < l0);   // enter child 1 first
                const int32_t cn = swap ? u.n.child[1] : u.n.child[0], cf = swap ? u.n.child[0] : u.n.child[1];
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
    if (g.out_f32)
        reinterpret_cast<float*>(g.out)[i] = (float)tt;
    else
        reinterpret_cast<double*>(g.out)[i] = tt;
    if (g.tri) g.tri[i] = bi == INT32_MAX ? -1 : bi;
    if (g.side) g.side[i] = (int8_t)bs;
}

// work buffers of the distance calls, kept per device between calls (r2s_release_cache frees them)
struct DistWork {
    DevBuf cnt, off, list, flag;            // binning
    DevBuf verts, tris, out, idx, field;   // host-pointer variants / the extracted surface
    void release()
    {
        DevBuf* all[] = {&cnt, &off, &list, &flag, &verts, &tris, &out, &idx, &field};
        for (DevBuf* b : all) b->release();
    }
};
std::mutex g_dist_mu;
std::map<int, DistWork> g_dist_work;

// [0] ms surface extraction, [1] ms binning (count, scan, fills), [2] ms tile kernel, [3] tile/triangle pairs, [4] batches,
// [5] triangles, [6] tiles, [7] tiles with triangles
thread_local double g_dist_stats[8];

int lattice_args(const char* who, const int64_t dims[3], const double origin[3], double spacing, double band)
{
    if (!dims || !origin) return fail(R2S_ERR_ARG, "%s: null dims / origin", who);
    if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2)
        return fail(R2S_ERR_ARG, "%s: every dimension must be >= 2 (got %lld x %lld x %lld)", who, (long long)dims[0],
                    (long long)dims[1], (long long)dims[2]);
    if (!(spacing > 0.0) || !std::isfinite(spacing)) return fail(R2S_ERR_ARG, "%s: spacing must be positive and finite", who);
    if (!(band > 0.0) || !std::isfinite(band)) return fail(R2S_ERR_ARG, "%s: band must be positive and finite", who);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a])) return fail(R2S_ERR_ARG, "%s: origin is not finite", who);
    if (dims[0] > INT32_MAX || dims[1] > INT32_MAX || dims[2] > INT32_MAX || dims[0] * dims[1] > INT64_MAX / 16 / dims[2])
        return fail(R2S_ERR_UNSUPPORTED, "%s: lattice too large", who);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(origin[a] + spacing * (double)(dims[a] - 1))) return fail(R2S_ERR_ARG, "%s: the lattice is not finite", who);
    return 0;
}

int mesh_args(const char* who, const void* verts, int64_t n_verts, const void* tris, int64_t n_tris)
{
    if (n_verts < 0 || n_tris < 0 || (n_verts > 0 && !verts) || (n_tris > 0 && !tris))
        return fail(R2S_ERR_ARG, "%s: null mesh array or negative count", who);
    if (n_verts > INT32_MAX || n_tris > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "%s: mesh does not fit 32-bit indices", who);
    return 0;
}

size_t workspace_budget()
{
    double mb = 1024.0;   // 1 GiB
    if (const char* e = std::getenv("R2S_REDIST_WORKSPACE_MB")) {
        const double v = std::atof(e);
        if (v > 0.0 && std::isfinite(v)) mb = v;
    }
    return (size_t)(mb * 1048576.0);
}

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st;
    float total = 0.0f;
    bool open = false;
    explicit Timer(hipStream_t s) : st(s)
    {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) a = b = nullptr;
    }
    ~Timer()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void start()
    {
        if (a) (void)hipEventRecord(a, st), open = true;
    }
    void stop()   // waits for the stream
    {
        if (!open) return;
        (void)hipEventRecord(b, st);
        (void)hipEventSynchronize(b);
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, a, b) == hipSuccess) total += ms;
        open = false;
    }
};

// distance of every lattice point to the device mesh on the current device, after the work queued on `st`; synchronous
int mesh_distance_core(const float* d_verts, const int32_t* d_tris, int64_t n_tris, const int64_t dims[3], const double origin[3],
                       double spacing, double band, const void* d_field, bool field_f32, double iso, void* d_out, bool out_f32,
                       int32_t* d_closest, hipStream_t st, DistWork& w)
{
    MdArgs g;
    g.nx = dims[0], g.ny = dims[1], g.nz = dims[2];
    g.ntx = (g.nx + TS - 1) / TS, g.nty = (g.ny + TS - 1) / TS, g.ntz = (g.nz + TS - 1) / TS;
    double big = band;
    for (int a = 0; a < 3; ++a) {
        g.o[a] = origin[a];
        big = std::max(big, std::max(std::fabs(origin[a]), std::fabs(origin[a] + spacing * (double)(dims[a] - 1))));
    }
    g.h = spacing;
    g.band = band;
    g.margin = std::ldexp(big + band, -40);
    g.bandm = band + 2.0 * g.margin;
    g.ntris = n_tris;
    const int64_t ntiles = g.ntx * g.nty * g.ntz, layer = g.ntx * g.nty;
    if (ntiles >= (int64_t)1 << 31) return fail(R2S_ERR_UNSUPPORTED, "mesh_distance: %lld tiles exceed one launch", (long long)ntiles);
    ENSURE(w.cnt, sizeof(uint32_t) * (size_t)ntiles);
    ENSURE(w.off, sizeof(uint64_t) * (size_t)(ntiles + 1));
    uint32_t* cnt = w.cnt.as<uint32_t>();
    uint64_t* off = w.off.as<uint64_t>();
    const unsigned tri_blocks = (unsigned)((n_tris + 255) / 256);
    Timer t_bin(st), t_tile(st);

    t_bin.start();
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (size_t)ntiles, st));
    if (n_tris > 0) md_bin_kernel<false><<<tri_blocks, 256, 0, st>>>(d_verts, d_tris, g, cnt, nullptr, 0, 0, g.ntz, nullptr);
    md_scan_kernel<<<1, 1024, 0, st>>>(cnt, ntiles, off);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> h_off((size_t)ntiles + 1);
    HIP_TRY(hipMemcpyAsync(h_off.data(), off, sizeof(uint64_t) * h_off.size(), hipMemcpyDeviceToHost, st));
    t_bin.stop();
    HIP_TRY(hipStreamSynchronize(st));

    // batches of whole tile layers whose lists fit the budget (a single layer that does not is a batch of its own)
    const uint64_t cap = std::max<uint64_t>(workspace_budget() / sizeof(int32_t), 1);
    int64_t n_batches = 0, n_active = 0;
    for (int64_t i = 0; i < ntiles; ++i) n_active += h_off[i + 1] > h_off[i];
    for (int64_t z0 = 0; z0 < g.ntz;) {
        int64_t z1 = z0 + 1;
        while (z1 < g.ntz && h_off[(size_t)((z1 + 1) * layer)] - h_off[(size_t)(z0 * layer)] <= cap) ++z1;
        const uint64_t o0 = h_off[(size_t)(z0 * layer)], pairs = h_off[(size_t)(z1 * layer)] - o0;
        if (pairs > 0) {
            t_bin.start();
            if (w.list.ensure_exact(sizeof(int32_t) * (size_t)pairs))
                return fail(R2S_ERR_NOMEM, "mesh_distance: hipMalloc of %zu bytes for the tile lists failed (R2S_REDIST_WORKSPACE_MB)",
                            sizeof(int32_t) * (size_t)pairs);
            HIP_TRY(hipMemsetAsync(cnt + z0 * layer, 0, sizeof(uint32_t) * (size_t)((z1 - z0) * layer), st));
            md_bin_kernel<true><<<tri_blocks, 256, 0, st>>>(d_verts, d_tris, g, cnt, off, o0, z0, z1, w.list.as<int32_t>());
            t_bin.stop();
        }
        t_tile.start();
        md_tile_kernel<<<(unsigned)((z1 - z0) * layer), 256, 0, st>>>(d_verts, d_tris, g, off, o0, z0 * layer, w.list.as<int32_t>(), d_field,
                                                                    field_f32 ? 1 : 0, iso, d_out, out_f32 ? 1 : 0, d_closest);
        HIP_TRY(hipGetLastError());
        t_tile.stop();
        ++n_batches;
        z0 = z1;
    }
    HIP_TRY(hipStreamSynchronize(st));
    g_dist_stats[1] = t_bin.total;
    g_dist_stats[2] = t_tile.total;
    g_dist_stats[3] = (double)h_off[(size_t)ntiles];
    g_dist_stats[4] = (double)n_batches;
    g_dist_stats[5] = (double)n_tris;
    g_dist_stats[6] = (double)ntiles;
    g_dist_stats[7] = (double)n_active;
    return 0;
}

DistWork& work_of_current_device(int& rc)
{
    int dev = 0;
    rc = hipGetDevice(&dev) == hipSuccess ? 0 : fail(R2S_ERR_HIP, "hipGetDevice failed");
    return g_dist_work[dev];
}

int redistance_core(const void* d_values, bool f32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                    double band, void* d_out, hipStream_t st, DistWork& w)
{
    Timer t_iso(st);
    t_iso.start();
    int64_t nv = 0, nt = 0;
    int rc = r2s_extract_isosurface_dev(d_values, f32 ? 1 : 0, dims, origin, spacing, iso, nullptr, 0, nullptr, 0, &nv, &nt, st);
    if (rc) return rc;
    if (nt > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "redistance: %lld triangles do not fit 32-bit indices", (long long)nt);
    if (nv > 0 || nt > 0) {
        ENSURE(w.verts, 3 * sizeof(float) * (size_t)std::max<int64_t>(nv, 1));
        ENSURE(w.tris, 3 * sizeof(int32_t) * (size_t)std::max<int64_t>(nt, 1));
        rc = r2s_extract_isosurface_dev(d_values, f32 ? 1 : 0, dims, origin, spacing, iso, w.verts.as<float>(), nv, w.tris.as<int32_t>(),
                                        nt, &nv, &nt, st);
        if (rc) return rc;
    }
    t_iso.stop();
    rc = mesh_distance_core(w.verts.as<float>(), w.tris.as<int32_t>(), nt, dims, origin, spacing, band, d_values, f32, iso, d_out, f32,
                            nullptr, st, w);
    g_dist_stats[0] = t_iso.total;
    return rc;
}

struct Scoped : DevBuf {
    Scoped() = default;
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
    ~Scoped() { release(); }
};

// the tree over the device mesh (verts, tris) on the current device, after the work queued on `st`; synchronous
int mi_build_tree(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, hipStream_t st, MiTree& T)
{
    T.verts = d_verts, T.tris = d_tris, T.n_verts = n_verts, T.n_tris = n_tris;
    T.root = 0, T.depth = 0, T.absmax = 0.0;
    if (n_tris == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    const unsigned blocks = (unsigned)((n_tris + 255) / 256);
    Scoped small, keys, sorted, temp, parent, flags;
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

// enqueues the query of n points (pts != null) or of the lattice (dims != null) on `st`; does not wait
int mi_query(const MiTree& T, const void* d_pts, bool pts_f32, int64_t n, const int64_t* dims, const double* origin, double spacing,
             const void* d_field, bool field_f32, double iso, void* d_out, bool out_f32, int32_t* d_closest, hipStream_t st)
{
    if (T.depth > MI_STACK)
        return fail(R2S_ERR_UNSUPPORTED, "mesh_index: tree depth %d exceeds the traversal stack of %d entries", T.depth, MI_STACK);
    MiQuery g = {};
    g.nodes = const_cast<MiTree&>(T).nodes.as<MiNode>();
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

int index_on_current_device(const char* who, const r2s_mesh_index* ix)
{
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ix->device) return fail(R2S_ERR_ARG, "%s: the index lives on device %d, the current device is %d", who, ix->device, dev);
    return 0;
}

// makes the index's device current for a host-pointer call and restores the caller's on scope exit
struct DeviceScope {
    int prev = -1;
    int enter(int device)
    {
        HIP_TRY(hipGetDevice(&prev));
        if (prev != device) HIP_TRY(hipSetDevice(device));
        return 0;
    }
    ~DeviceScope()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int redistance_full_core(const void* d_values, bool f32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                         void* d_out, hipStream_t st, DistWork& w)
{
    int64_t nv = 0, nt = 0;
    int rc = r2s_extract_isosurface_dev(d_values, f32 ? 1 : 0, dims, origin, spacing, iso, nullptr, 0, nullptr, 0, &nv, &nt, st);
    if (rc) return rc;
    if (nt > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "redistance_full: %lld triangles do not fit 32-bit indices", (long long)nt);
    if (nv > 0 || nt > 0) {
        ENSURE(w.verts, 3 * sizeof(float) * (size_t)std::max<int64_t>(nv, 1));
        ENSURE(w.tris, 3 * sizeof(int32_t) * (size_t)std::max<int64_t>(nt, 1));
        rc = r2s_extract_isosurface_dev(d_values, f32 ? 1 : 0, dims, origin, spacing, iso, w.verts.as<float>(), nv, w.tris.as<int32_t>(),
                                        nt, &nv, &nt, st);
        if (rc) return rc;
    }
    MiTree T;
    rc = mi_build_tree(w.verts.as<float>(), nv, w.tris.as<int32_t>(), nt, st, T);
    if (!rc) rc = mi_query(T, nullptr, false, 0, dims, origin, spacing, d_values, f32, iso, d_out, f32, nullptr, st);
    const hipError_t e = hipStreamSynchronize(st);
    T.nodes.release();
    if (!rc && e != hipSuccess) return fail(R2S_ERR_HIP, "redistance_full: %s", hipGetErrorString(e));
    return rc;
}

int full_args(const char* who, const int64_t dims[3], const double origin[3], double spacing, double iso, const void* a, const void* b)
{
    int rc = lattice_args(who, dims, origin, spacing, 1.0);
    if (rc) return rc;
    if (std::isnan(iso)) return fail(R2S_ERR_ARG, "%s: iso is NaN", who);
    if (!a || !b) return fail(R2S_ERR_ARG, "%s: null values / output", who);
    return 0;
}

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
    if (T.depth > MI_STACK)
        return fail(R2S_ERR_UNSUPPORTED, "mesh_index: tree depth %d exceeds the traversal stack of %d entries", T.depth, MI_STACK);
    MiRay g = {};
    g.nodes = const_cast<MiTree&>(T).nodes.as<MiNode>();
    g.verts = T.verts, g.tris = T.tris, g.ntris = T.n_tris, g.root = T.root, g.absmax = T.absmax;
    g.org = d_org, g.dir = d_dir, g.rays_f32 = rays_f32 ? 1 : 0, g.n = n;
    g.tmin = t_min, g.tmax = t_max;
    g.out = d_out, g.out_f32 = out_f32 ? 1 : 0, g.tri = d_tri, g.side = d_side;
    mi_ray_kernel<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(g);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

namespace r2s_int {

void release_dist_work()
{
    std::lock_guard<std::mutex> lock(g_dist_mu);
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) cur = -1;
    for (auto& kv : g_dist_work) {
        (void)hipSetDevice(kv.first);
        kv.second.release();
    }
    g_dist_work.clear();
    if (cur >= 0) (void)hipSetDevice(cur);
    (void)hipGetLastError();
}

}  // namespace r2s_int

extern "C" {

int r2s_mesh_distance(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int64_t dims[3],
                      const double origin[3], double spacing, double band, int32_t out_is_float32, int32_t device, void* dist_out,
                      int32_t* closest_tri_out)
{
    int rc = lattice_args("mesh_distance", dims, origin, spacing, band);
    if (rc || (rc = mesh_args("mesh_distance", verts, n_verts, tris, n_tris))) return rc;
    if (!dist_out) return fail(R2S_ERR_ARG, "mesh_distance: null output");
    for (int64_t i = 0; i < 3 * n_tris; ++i)
        if (tris[i] < 0 || tris[i] >= n_verts)
            return fail(R2S_ERR_ARG, "mesh_distance: triangle %lld has vertex index %d outside [0, %lld)", (long long)(i / 3), tris[i],
                        (long long)n_verts);
    for (int64_t i = 0; i < 3 * n_verts; ++i)
        if (!std::isfinite(verts[i])) return fail(R2S_ERR_ARG, "mesh_distance: vertex %lld is not finite", (long long)(i / 3));
    if ((rc = use_device(device))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_mu);
    DistWork& w = work_of_current_device(rc);
    if (rc) return rc;
    const size_t nvox = (size_t)(dims[0] * dims[1] * dims[2]), esz = out_is_float32 ? sizeof(float) : sizeof(double);
    ENSURE(w.verts, 3 * sizeof(float) * (size_t)std::max<int64_t>(n_verts, 1));
    ENSURE(w.tris, 3 * sizeof(int32_t) * (size_t)std::max<int64_t>(n_tris, 1));
    ENSURE(w.out, esz * nvox);
    if (closest_tri_out) ENSURE(w.idx, sizeof(int32_t) * nvox);
    if (n_verts) HIP_TRY(hipMemcpy(w.verts.p, verts, 3 * sizeof(float) * (size_t)n_verts, hipMemcpyHostToDevice));
    if (n_tris) HIP_TRY(hipMemcpy(w.tris.p, tris, 3 * sizeof(int32_t) * (size_t)n_tris, hipMemcpyHostToDevice));
    g_dist_stats[0] = 0.0;
    rc = mesh_distance_core(w.verts.as<float>(), w.tris.as<int32_t>(), n_tris, dims, origin, spacing, band, nullptr, false, 0.0, w.out.p,
                            out_is_float32 != 0, closest_tri_out ? w.idx.as<int32_t>() : nullptr, nullptr, w);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dist_out, w.out.p, esz * nvox, hipMemcpyDeviceToHost));
    if (closest_tri_out) HIP_TRY(hipMemcpy(closest_tri_out, w.idx.p, sizeof(int32_t) * nvox, hipMemcpyDeviceToHost));
    return 0;
}

int r2s_mesh_distance_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, const int64_t dims[3],
                          const double origin[3], double spacing, double band, int32_t out_is_float32, void* d_dist_out,
                          int32_t* d_closest_tri_out, void* stream)
{
    int rc = lattice_args("mesh_distance", dims, origin, spacing, band);
    if (rc || (rc = mesh_args("mesh_distance", d_verts, n_verts, d_tris, n_tris))) return rc;
    if (!d_dist_out) return fail(R2S_ERR_ARG, "mesh_distance: null output");
    if ((rc = check_device(0))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_mu);
    DistWork& w = work_of_current_device(rc);
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n_check = 3 * std::max(n_verts, n_tris);
    if (n_check > 0) {
        ENSURE(w.flag, sizeof(int32_t));
        HIP_TRY(hipMemsetAsync(w.flag.p, 0, sizeof(int32_t), st));
        md_check_kernel<<<(unsigned)((n_check + 255) / 256), 256, 0, st>>>(d_verts, n_verts, d_tris, n_tris, w.flag.as<int32_t>());
        HIP_TRY(hipGetLastError());
        int32_t bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, w.flag.p, sizeof bad, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad) return fail(R2S_ERR_ARG, "mesh_distance: a triangle index lies outside [0, %lld) or a vertex is not finite", (long long)n_verts);
    }
    g_dist_stats[0] = 0.0;
    return mesh_distance_core(d_verts, d_tris, n_tris, dims, origin, spacing, band, nullptr, false, 0.0, d_dist_out, out_is_float32 != 0,
                              d_closest_tri_out, st, w);
}

int r2s_redistance(const void* values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                   double band, int32_t device, void* out)
{
    int rc = lattice_args("redistance", dims, origin, spacing, band);
    if (rc) return rc;
    if (std::isnan(iso)) return fail(R2S_ERR_ARG, "redistance: iso is NaN");
    if (!values || !out) return fail(R2S_ERR_ARG, "redistance: null values / output");
    if ((rc = use_device(device))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_mu);
    DistWork& w = work_of_current_device(rc);
    if (rc) return rc;
    const size_t bytes = (is_float32 ? sizeof(float) : sizeof(double)) * (size_t)(dims[0] * dims[1] * dims[2]);
    ENSURE(w.field, bytes);
    ENSURE(w.out, bytes);
    HIP_TRY(hipMemcpy(w.field.p, values, bytes, hipMemcpyHostToDevice));
    if ((rc = redistance_core(w.field.p, is_float32 != 0, dims, origin, spacing, iso, band, w.out.p, nullptr, w))) return rc;
    HIP_TRY(hipMemcpy(out, w.out.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int r2s_redistance_dev(const void* d_values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing,
                       double iso, double band, void* d_out, void* stream)
{
    int rc = lattice_args("redistance", dims, origin, spacing, band);
    if (rc) return rc;
    if (std::isnan(iso)) return fail(R2S_ERR_ARG, "redistance: iso is NaN");
    if (!d_values || !d_out) return fail(R2S_ERR_ARG, "redistance: null values / output");
    if ((rc = check_device(0))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_mu);
    DistWork& w = work_of_current_device(rc);
    if (rc) return rc;
    return redistance_core(d_values, is_float32 != 0, dims, origin, spacing, iso, band, d_out, (hipStream_t)stream, w);
}

int r2s_mesh_index_build(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, int32_t device, r2s_mesh_index** out)
{
    int rc = mesh_args("mesh_index_build", verts, n_verts, tris, n_tris);
    if (rc) return rc;
    if (!out) return fail(R2S_ERR_ARG, "mesh_index_build: null output");
    for (int64_t i = 0; i < 3 * n_tris; ++i)
        if (tris[i] < 0 || tris[i] >= n_verts)
            return fail(R2S_ERR_ARG, "mesh_index_build: triangle %lld has vertex index %d outside [0, %lld)", (long long)(i / 3), tris[i],
                        (long long)n_verts);
    for (int64_t i = 0; i < 3 * n_verts; ++i)
        if (!std::isfinite(verts[i])) return fail(R2S_ERR_ARG, "mesh_index_build: vertex %lld is not finite", (long long)(i / 3));
    if ((rc = check_device(device < 0 ? 0 : device))) return rc;
    DeviceScope scope;
    int dev = device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if ((rc = scope.enter(dev))) return rc;
    r2s_mesh_index* ix = new r2s_mesh_index;
    ix->device = dev;
    rc = [&]() -> int {
        ENSURE(ix->verts, 3 * sizeof(float) * (size_t)std::max<int64_t>(n_verts, 1));
        ENSURE(ix->tris, 3 * sizeof(int32_t) * (size_t)std::max<int64_t>(n_tris, 1));
        if (n_verts) HIP_TRY(hipMemcpy(ix->verts.p, verts, 3 * sizeof(float) * (size_t)n_verts, hipMemcpyHostToDevice));
        if (n_tris) HIP_TRY(hipMemcpy(ix->tris.p, tris, 3 * sizeof(int32_t) * (size_t)n_tris, hipMemcpyHostToDevice));
        return mi_build_tree(ix->verts.as<float>(), n_verts, ix->tris.as<int32_t>(), n_tris, nullptr, ix->tree);
    }();
    if (rc) {
        r2s_mesh_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return 0;
}

int r2s_mesh_index_build_dev(const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, void* stream,
                             r2s_mesh_index** out)
{
    int rc = mesh_args("mesh_index_build", d_verts, n_verts, d_tris, n_tris);
    if (rc) return rc;
    if (!out) return fail(R2S_ERR_ARG, "mesh_index_build: null output");
    if ((rc = check_device(0))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n_check = 3 * std::max(n_verts, n_tris);
    if (n_check > 0) {
        Scoped flag;
        ENSURE(flag, sizeof(int32_t));
        HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int32_t), st));
        md_check_kernel<<<(unsigned)((n_check + 255) / 256), 256, 0, st>>>(d_verts, n_verts, d_tris, n_tris, flag.as<int32_t>());
        HIP_TRY(hipGetLastError());
        int32_t bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, flag.p, sizeof bad, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad) return fail(R2S_ERR_ARG, "mesh_index_build: a triangle index lies outside [0, %lld) or a vertex is not finite", (long long)n_verts);
    }
    r2s_mesh_index* ix = new r2s_mesh_index;
    rc = [&]() -> int {
        HIP_TRY(hipGetDevice(&ix->device));
        ENSURE(ix->verts, 3 * sizeof(float) * (size_t)std::max<int64_t>(n_verts, 1));
        ENSURE(ix->tris, 3 * sizeof(int32_t) * (size_t)std::max<int64_t>(n_tris, 1));
        if (n_verts) HIP_TRY(hipMemcpyAsync(ix->verts.p, d_verts, 3 * sizeof(float) * (size_t)n_verts, hipMemcpyDeviceToDevice, st));
        if (n_tris) HIP_TRY(hipMemcpyAsync(ix->tris.p, d_tris, 3 * sizeof(int32_t) * (size_t)n_tris, hipMemcpyDeviceToDevice, st));
        return mi_build_tree(ix->verts.as<float>(), n_verts, ix->tris.as<int32_t>(), n_tris, st, ix->tree);
    }();
    if (rc) {
        r2s_mesh_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return 0;
}

void r2s_mesh_index_destroy(r2s_mesh_index* ix)
{
    if (!ix) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != ix->device) (void)hipSetDevice(ix->device);
    ix->verts.release();
    ix->tris.release();
    ix->tree.nodes.release();
    if (prev >= 0 && prev != ix->device) (void)hipSetDevice(prev);
    (void)hipGetLastError();
    delete ix;
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
    if ((rc = check_device(0))) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(ix->device))) return rc;
    const size_t psz = 3 * (points_are_float32 ? sizeof(float) : sizeof(double)) * (size_t)n;
    const size_t osz = (out_is_float32 ? sizeof(float) : sizeof(double)) * (size_t)n;
    Scoped pts, out, idx;
    ENSURE(pts, psz);
    ENSURE(out, osz);
    if (closest_tri_out) ENSURE(idx, sizeof(int32_t) * (size_t)n);
    HIP_TRY(hipMemcpy(pts.p, points, psz, hipMemcpyHostToDevice));
    if ((rc = mi_query(ix->tree, pts.p, points_are_float32 != 0, n, nullptr, nullptr, 0.0, nullptr, false, 0.0, out.p, out_is_float32 != 0,
                       closest_tri_out ? idx.as<int32_t>() : nullptr, nullptr)))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dist_out, out.p, osz, hipMemcpyDeviceToHost));
    if (closest_tri_out) HIP_TRY(hipMemcpy(closest_tri_out, idx.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
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
    if ((rc = check_device(0))) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(ix->device))) return rc;
    const size_t psz = 3 * (rays_are_float32 ? sizeof(float) : sizeof(double)) * (size_t)n;
    const size_t osz = (out_is_float32 ? sizeof(float) : sizeof(double)) * (size_t)n;
    Scoped org, dir, out, idx, side;
    ENSURE(org, psz);
    ENSURE(dir, psz);
    ENSURE(out, osz);
    if (tri_out) ENSURE(idx, sizeof(int32_t) * (size_t)n);
    if (side_out) ENSURE(side, (size_t)n);
    HIP_TRY(hipMemcpy(org.p, origins, psz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dir.p, dirs, psz, hipMemcpyHostToDevice));
    if ((rc = mi_raycast(ix->tree, org.p, dir.p, rays_are_float32 != 0, n, t_min, t_max, out.p, out_is_float32 != 0,
                         tri_out ? idx.as<int32_t>() : nullptr, side_out ? side.as<int8_t>() : nullptr, nullptr)))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(t_out, out.p, osz, hipMemcpyDeviceToHost));
    if (tri_out) HIP_TRY(hipMemcpy(tri_out, idx.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (side_out) HIP_TRY(hipMemcpy(side_out, side.p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
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
    if ((rc = check_device(0))) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(ix->device))) return rc;
    const size_t nvox = (size_t)(dims[0] * dims[1] * dims[2]), osz = (out_is_float32 ? sizeof(float) : sizeof(double)) * nvox;
    Scoped out, idx;
    ENSURE(out, osz);
    if (closest_tri_out) ENSURE(idx, sizeof(int32_t) * nvox);
    if ((rc = mi_query(ix->tree, nullptr, false, 0, dims, origin, spacing, nullptr, false, 0.0, out.p, out_is_float32 != 0,
                       closest_tri_out ? idx.as<int32_t>() : nullptr, nullptr)))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dist_out, out.p, osz, hipMemcpyDeviceToHost));
    if (closest_tri_out) HIP_TRY(hipMemcpy(closest_tri_out, idx.p, sizeof(int32_t) * nvox, hipMemcpyDeviceToHost));
    return 0;
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

int r2s_redistance_full(const void* values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                        int32_t device, void* out)
{
    int rc = full_args("redistance_full", dims, origin, spacing, iso, values, out);
    if (rc || (rc = use_device(device))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_mu);
    DistWork& w = work_of_current_device(rc);
    if (rc) return rc;
    const size_t bytes = (is_float32 ? sizeof(float) : sizeof(double)) * (size_t)(dims[0] * dims[1] * dims[2]);
    ENSURE(w.field, bytes);
    ENSURE(w.out, bytes);
    HIP_TRY(hipMemcpy(w.field.p, values, bytes, hipMemcpyHostToDevice));
    if ((rc = redistance_full_core(w.field.p, is_float32 != 0, dims, origin, spacing, iso, w.out.p, nullptr, w))) return rc;
    HIP_TRY(hipMemcpy(out, w.out.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int r2s_redistance_full_dev(const void* d_values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing,
                            double iso, void* d_out, void* stream)
{
    int rc = full_args("redistance_full", dims, origin, spacing, iso, d_values, d_out);
    if (rc || (rc = check_device(0))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_mu);
    DistWork& w = work_of_current_device(rc);
    if (rc) return rc;
    return redistance_full_core(d_values, is_float32 != 0, dims, origin, spacing, iso, d_out, (hipStream_t)stream, w);
}

void r2s_last_distance_stats(double out[8])
{
    if (out) std::memcpy(out, g_dist_stats, sizeof g_dist_stats);
}

}  // extern "C"
