// Device-side triangle arithmetic shared by the tile kernel of r2s_redistance.hip and the traversals of r2s_mesh_index.hip:
// the triangle record and the point-to-triangle distance built on it (the same arithmetic, hence the same numbers wherever
// both answer), and the typed access to float32 / float64 fields and results.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int REC = 40;        // doubles per record
// record layout (doubles): a 0-2, b 3-5, ab 6-8, ac 9-11, bc 12-14, n 15-17, n x ab 18-20, n x ac 21-23, n x bc 24-26,
// 1/ab.ab 27, 1/ac.ac 28, 1/bc.bc 29, 1/n.n 30 (0 = the feature is degenerate), AABB lo 31-33, hi 34-36, index 37 (as int64)

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

// component k of v by selects (an indexed register array would go to scratch)
__device__ inline double vec_pick(Vec3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// Does the segment p -> q meet the triangle a b c?  The segment test of the header (r2s_mesh_index_intersections): the ray pair
// test, steps 1 to 7, with o = p and d = q - p, every operation rounded on its own; a hit is not mixed, det != 0 and
// 0 <= t <= 1.  The same arithmetic as the leaf of mi_ray_kernel without its box condition.
__device__ inline bool seg_tri_hit(Vec3 p, Vec3 q, Vec3 a, Vec3 b, Vec3 c)
{
#pragma clang fp contract(off)
    const Vec3 d = sub(q, p);
    if (d.x == 0.0 && d.y == 0.0 && d.z == 0.0) return false;
    int kz = 0;
    double big = fabs(d.x);
    if (fabs(d.y) > big) kz = 1, big = fabs(d.y);
    if (fabs(d.z) > big) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dkz = vec_pick(d, kz);
    if (dkz < 0.0) {
        const int s = kx;
        kx = ky, ky = s;
    }
    const double Sx = vec_pick(d, kx) / dkz, Sy = vec_pick(d, ky) / dkz, Sz = 1.0 / dkz;
    const double okx = vec_pick(p, kx), oky = vec_pick(p, ky), okz = vec_pick(p, kz);
    const double Az = vec_pick(a, kz) - okz, Bz = vec_pick(b, kz) - okz, Cz = vec_pick(c, kz) - okz;
    const double Ax = (vec_pick(a, kx) - okx) - Sx * Az, Ay = (vec_pick(a, ky) - oky) - Sy * Az;
    const double Bx = (vec_pick(b, kx) - okx) - Sx * Bz, By = (vec_pick(b, ky) - oky) - Sy * Bz;
    const double Cx = (vec_pick(c, kx) - okx) - Sx * Cz, Cy = (vec_pick(c, ky) - oky) - Sy * Cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const bool mixed = (U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0);
    const double det = (U + V) + W;
    if (mixed || det == 0.0) return false;
    const double t = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det;
    return t >= 0.0 && t <= 1.0;
}

// The effective sign of the edge function f of the directed projected edge P -> Q (the header, r2s_mesh_index_winding, step 4):
// the sign of f, and for f == 0 the sign f would take with the point moved by (eps, eps^2): that of Qy - Py, else of Px - Qx.
// P and Q are the vertices' own float32 coordinates widened to double, so the two differences are exact.
__device__ inline int edge_sign(double f, double px, double py, double qx, double qy)
{
    if (f != 0.0) return f > 0.0 ? 1 : -1;
    if (qy != py) return qy > py ? 1 : -1;
    return px > qx ? 1 : (px < qx ? -1 : 0);
}

// Does the axis ray from o along +e_KZ (neg: -e_KZ) cross the triangle a b c (float32 corners)?  The pair test of the header
// (r2s_mesh_index_winding, steps 1 to 6) in two halves, so that a lattice row, whose points share the first, runs the same
// arithmetic as a single point.  The caller has set collapsed triangles aside.  Every operation is rounded on its own.
// First half, what depends on o[kx], o[ky] only (o1, o2 = o[(KZ+1)%3], o[(KZ+2)%3]): the two projected comparisons of the own-box
// condition, U, V, W and their effective signs, det != 0.  -> 0 = no crossing for any o[kz], else `side`.
template <int KZ>
__device__ inline int axis_cross_2d(double o1, double o2, bool neg, const float* __restrict__ fa, const float* __restrict__ fb,
                                    const float* __restrict__ fc, double& U, double& V, double& W)
{
#pragma clang fp contract(off)
    constexpr int K1 = (KZ + 1) % 3, K2 = (KZ + 2) % 3;
    if (!((double)fminf(fa[K1], fminf(fb[K1], fc[K1])) <= o1 && o1 <= (double)fmaxf(fa[K1], fmaxf(fb[K1], fc[K1])))) return 0;
    if (!((double)fminf(fa[K2], fminf(fb[K2], fc[K2])) <= o2 && o2 <= (double)fmaxf(fa[K2], fmaxf(fb[K2], fc[K2])))) return 0;
    // kx, ky = K1, K2, swapped for a ray along -e_KZ
    const double okx = neg ? o2 : o1, oky = neg ? o1 : o2;
    const double ax = (double)(neg ? fa[K2] : fa[K1]), ay = (double)(neg ? fa[K1] : fa[K2]);
    const double bx = (double)(neg ? fb[K2] : fb[K1]), by = (double)(neg ? fb[K1] : fb[K2]);
    const double cx = (double)(neg ? fc[K2] : fc[K1]), cy = (double)(neg ? fc[K1] : fc[K2]);
    const double Ax = ax - okx, Ay = ay - oky, Bx = bx - okx, By = by - oky, Cx = cx - okx, Cy = cy - oky;
    U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const int su = edge_sign(U, bx, by, cx, cy), sv = edge_sign(V, cx, cy, ax, ay), sw = edge_sign(W, ax, ay, bx, by);
    if (su == 0 || su != sv || su != sw) return 0;
    return (U + V) + W != 0.0 ? su : 0;
}
// Second half, what depends on oz = o[KZ]: the box reaches ahead of the point, and t > 0.  Monotone in oz (true up to a threshold
// for +e_KZ, from a threshold on for -e_KZ): the subtraction, the product with a factor of fixed sign, the sum and the quotient are.
template <int KZ>
__device__ inline bool axis_cross_1d(double oz, bool neg, const float* __restrict__ fa, const float* __restrict__ fb,
                                     const float* __restrict__ fc, double U, double V, double W)
{
#pragma clang fp contract(off)
    if (neg ? !((double)fminf(fa[KZ], fminf(fb[KZ], fc[KZ])) <= oz) : !((double)fmaxf(fa[KZ], fmaxf(fb[KZ], fc[KZ])) >= oz)) return false;
    const double det = (U + V) + W;
    const double Sz = neg ? -1.0 : 1.0;
    const double Az = (double)fa[KZ] - oz, Bz = (double)fb[KZ] - oz, Cz = (double)fc[KZ] - oz;
    const double t = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det;
    return t > 0.0;
}
// the whole pair test for one point: 0 = no crossing, else `side`, the common effective sign of U, V, W
template <int KZ>
__device__ inline int axis_cross(Vec3 o, bool neg, const float* __restrict__ fa, const float* __restrict__ fb, const float* __restrict__ fc)
{
    double U, V, W;
    const int side = axis_cross_2d<KZ>(vec_pick(o, (KZ + 1) % 3), vec_pick(o, (KZ + 2) % 3), neg, fa, fb, fc, U, V, W);
    return side != 0 && axis_cross_1d<KZ>(vec_pick(o, KZ), neg, fa, fb, fc, U, V, W) ? side : 0;
}

// element i of a float32 (f32 != 0) or float64 array, read as / stored from a double
__device__ inline double load_real(const void* p, int f32, int64_t i)
{
    return f32 ? (double)reinterpret_cast<const float*>(p)[i] : reinterpret_cast<const double*>(p)[i];
}
__device__ inline void store_real(void* p, int f32, int64_t i, double v)
{
    if (f32)
        reinterpret_cast<float*>(p)[i] = (float)v;
    else
        reinterpret_cast<double*>(p)[i] = v;
}
