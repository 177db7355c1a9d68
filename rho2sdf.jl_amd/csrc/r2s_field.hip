// The smoothed level-set as a FUNCTION: f(p) = th + sum_j w_j exp(-(|p - x_j| / sigma)^2) over the coarse lattice nodes
// (RBFs4Smoothing.jl:219-248, :366), evaluated with its gradient at arbitrary points.  r2s_rbf_field keeps the weights and
// the level shift of one smoothing on its device; one kernel template serves evaluation, normals and projection.
//
// Shape of the work (kernel threshold 1e-3): ~76 of the ~216 lattice nodes of the support's bounding box lie inside the
// support, each costs one Float64 exp.  Points arrive in caller order, so a wavefront's points may sit anywhere in the lattice.
//   - FIELD_SG = 16 lanes share one point (4 points per wavefront).  Everything a lane branches on besides its own candidate
//     is uniform over the 16 lanes.
//   - pass 1: the lanes stride over the candidate box (the nodes within R + margin cells of the point, per axis), form the
//     Float32 distance with rbf_apply_point's arithmetic and COMPACT the nodes inside the support into a per-point list in
//     LDS (ballot + prefix count: the list is in candidate order, whatever the lanes do).  The cheap test is the divergent
//     part; the expensive part below runs on dense lanes.
//   - knn cap: the list's length is the number of in-bounds nodes inside the support.  Only when it exceeds 124 (never at
//     1e-3) each entry is ranked against the others by (distance, node index) and the 124 smallest take part.
//   - pass 2: the lanes stride over the list: weight gather, exp, Float64 partial sums of the value and of the three gradient
//     components (second-derivative modes: also of the six products d_a d_b); a fixed xor butterfly over the 16 lanes adds them.  The order of summation is a function of the point and
//     the lattice alone: no atomics, nothing depends on the point's place in the array or on the launch.
// No host work per point, no synchronisation besides one workgroup barrier (the exp table), no LDS traffic between points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_rbf_exp.hpp"

#define FIELD_SG 16
// The 16 lanes of a point hand their list to each other through LDS with __threadfence_block() only: that holds because a
// sub-group lies inside ONE wavefront (wave64 on gfx950), whose LDS operations complete in order.
static_assert(64 % FIELD_SG == 0 && FIELD_SG <= 64, "a point's lanes must share one wave64 wavefront");
#define FIELD_KNN 124   // knn(kdtree, p, 124), RBFs4Smoothing.jl:238

namespace {

struct FieldGeom {
    int nx, ny, nz;
    const float *cx, *cy, *cz;   // Float32 axes of create_grid
    const float* w;              // weights, x fastest
    double amin[3];
    double inv_h;                // 1 / cell_size
    double reach;                // support radius in cells + the margin that covers the Float32 rounding of the axes
    double inv_sigma;            // sigma = cell_size
    double gscale;               // -2 / sigma^2
    float max_distance;
    float th;                    // level shift
    float cell;                  // longest projection step
    int cap;                     // list entries per point (>= any support's node count)
};

enum { FIELD_VALUE = 0, FIELD_GRAD = 1, FIELD_NORMALS = 2, FIELD_PROJECT = 3, FIELD_HESS = 4, FIELD_CURV = 5 };

struct FieldOut {
    float* val;       // [n]
    float* grad;      // [n][3]; FIELD_NORMALS: the normals
    int32_t* taps;    // [n]
    float* points;    // FIELD_PROJECT: [n][3], moved in place
    int32_t* status;  // FIELD_PROJECT
    float* resid;
    int32_t* iters;
    int max_iter;
    float tol;
    float* hess;      // FIELD_HESS / FIELD_CURV: [n][6] = xx, yy, zz, xy, xz, yz
    float* curv;      // FIELD_CURV: [n][4] = mean, gauss, k1, k2
};

// value (with the level shift), derivatives up to order ORD (1: gradient, 2: gradient and Hessian xx, yy, zz, xy, xz, yz)
// and tap count at one finite point, by the 16 lanes of its sub-group; every lane returns the same numbers.  `h` is
// touched for ORD == 2 only.
template <int ORD>
__device__ __forceinline__ void field_point(const FieldGeom& G, uint2* __restrict__ list, const double* __restrict__ etab, int l,
                                            int sg_shift, float px, float py, float pz, float& val, float g[3], int& taps,
                                            float* h = nullptr)
{
    __threadfence_block();   // (projection: the previous step's reads of the list come first)
    const double q[3] = {((double)px - G.amin[0]) * G.inv_h, ((double)py - G.amin[1]) * G.inv_h, ((double)pz - G.amin[2]) * G.inv_h};
    const int nn[3] = {G.nx, G.ny, G.nz};
    int lo[3], b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double dlo = fmax(ceil(q[a] - G.reach), 0.0), dhi = fmin(floor(q[a] + G.reach), (double)(nn[a] - 1));
        lo[a] = dlo <= dhi ? (int)dlo : 0;
        b[a] = dlo <= dhi ? (int)dhi - (int)dlo + 1 : 0;   // <= 15 (checked when the field is made)
    }
    const int rows = b[1] * b[2], ncand = b[0] * rows;
    const float inv_bx = 1.0f / (float)max(b[0], 1), inv_by = 1.0f / (float)max(b[1], 1);
    int cnt = 0;
    for (int c0 = 0; c0 < ncand; c0 += FIELD_SG) {
        const int c = c0 + l;
        const bool valid = c < ncand;
        // c = (iz * by + iy) * bx + ix; quotients of small integers through the reciprocal (c + 0.5 keeps them exact)
        const int r = (int)(((float)c + 0.5f) * inv_bx), ix = c - r * b[0];
        const int iz = (int)(((float)r + 0.5f) * inv_by), iy = r - iz * b[1];
        float dist = 0.0f;
        bool pass = false;
        if (valid) {
            const float dx = px - G.cx[lo[0] + ix], dy = py - G.cy[lo[1] + iy], dz = pz - G.cz[lo[2] + iz];
            dist = sqrtf(dx * dx + dy * dy + dz * dz);
            pass = dist <= G.max_distance;
        }
        const unsigned sb = (unsigned)(__ballot(pass) >> sg_shift) & 0xFFFFu;
        const int pos = cnt + __popc(sb & ((1u << l) - 1u));
        if (pass && pos < G.cap) list[pos] = make_uint2(__float_as_uint(dist), (unsigned)((iz << 8) | (iy << 4) | ix));
        cnt += __popc(sb);
    }
    const bool overflow = cnt > G.cap;   // cannot happen while field_make's bound on the support holds; reported, not hidden
    cnt = min(cnt, G.cap);
    __threadfence_block();
    const bool capped = cnt > FIELD_KNN;
    double sv = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    double sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;   // ORD == 2: sums of wk d_a d_b
    for (int e = l; e < cnt; e += FIELD_SG) {
        const uint2 en = list[e];
        const float dist = __uint_as_float(en.x);
        bool take = true;
        if (capped) {   // rare: rank by (distance, node index); the key orders nodes of one box like their linear index
            int rank = 0;
            for (int j = 0; j < cnt; ++j) {
                const uint2 o = list[j];
                const float od = __uint_as_float(o.x);
                rank += (od < dist || (od == dist && o.y < en.y)) ? 1 : 0;
            }
            take = rank < FIELD_KNN;
        }
        if (take) {
            const int ci = lo[0] + (int)(en.y & 15u), cj = lo[1] + (int)((en.y >> 4) & 15u), ck = lo[2] + (int)(en.y >> 8);
            const double u = (double)dist * G.inv_sigma;
            const double wk = (double)G.w[((int64_t)ck * G.ny + cj) * G.nx + ci] * exp_neg_fast(u * u, etab);
            sv += wk;
            if (ORD >= 1) {
                const float dx = px - G.cx[ci], dy = py - G.cy[cj], dz = pz - G.cz[ck];
                const double tx = wk * (double)dx, ty = wk * (double)dy, tz = wk * (double)dz;
                sx += tx;
                sy += ty;
                sz += tz;
                if (ORD >= 2) {
                    sxx += tx * (double)dx;
                    syy += ty * (double)dy;
                    szz += tz * (double)dz;
                    sxy += tx * (double)dy;
                    sxz += tx * (double)dz;
                    syz += ty * (double)dz;
                }
            }
        }
    }
#pragma unroll
    for (int m = FIELD_SG / 2; m >= 1; m >>= 1) {
        sv += __shfl_xor(sv, m, FIELD_SG);
        if (ORD >= 1) {
            sx += __shfl_xor(sx, m, FIELD_SG);
            sy += __shfl_xor(sy, m, FIELD_SG);
            sz += __shfl_xor(sz, m, FIELD_SG);
        }
        if (ORD >= 2) {
            sxx += __shfl_xor(sxx, m, FIELD_SG);
            syy += __shfl_xor(syy, m, FIELD_SG);
            szz += __shfl_xor(szz, m, FIELD_SG);
            sxy += __shfl_xor(sxy, m, FIELD_SG);
            sxz += __shfl_xor(sxz, m, FIELD_SG);
            syz += __shfl_xor(syz, m, FIELD_SG);
        }
    }
    val = (float)sv + G.th;
    g[0] = (float)(sx * G.gscale);
    g[1] = (float)(sy * G.gscale);
    g[2] = (float)(sz * G.gscale);
    if (ORD >= 2) {   // H_ab = 4 / sigma^4 s_ab - 2 / sigma^2 delta_ab sv: the delta term is the value's own sum
        const double hs = G.gscale * G.gscale, dg = G.gscale * sv;
        h[0] = (float)(hs * sxx + dg);
        h[1] = (float)(hs * syy + dg);
        h[2] = (float)(hs * szz + dg);
        h[3] = (float)(hs * sxy);
        h[4] = (float)(hs * sxz);
        h[5] = (float)(hs * syz);
    }
    taps = overflow ? INT32_MIN : capped ? -FIELD_KNN : cnt;
}

template <int MODE>
__global__ void __launch_bounds__(256) rbf_field_kernel(FieldGeom G, const float* __restrict__ pts, int64_t n, FieldOut O)
{
    extern __shared__ uint2 field_lists[];   // [points of the workgroup][G.cap]: (Float32 distance, box-local node key)
    __shared__ double etab[64];
    if (threadIdx.x < 64) etab[threadIdx.x] = c_exp2_neg_64[threadIdx.x];
    __syncthreads();
    const int l = threadIdx.x & (FIELD_SG - 1), sg = threadIdx.x / FIELD_SG;
    const int sg_shift = (threadIdx.x & 63) & ~(FIELD_SG - 1);
    const int64_t t = (int64_t)blockIdx.x * (blockDim.x / FIELD_SG) + sg;
    if (t >= n) return;
    uint2* list = field_lists + (size_t)sg * G.cap;
    const float* src = MODE == FIELD_PROJECT ? O.points : pts;
    float px = src[3 * t], py = src[3 * t + 1], pz = src[3 * t + 2];
    const bool finite = isfinite(px) && isfinite(py) && isfinite(pz);
    const float fnan = __uint_as_float(0x7FC00000u);
    float val = fnan, g[3] = {fnan, fnan, fnan};
    int taps = 0;
    if (MODE == FIELD_VALUE || MODE == FIELD_GRAD) {
        if (finite) field_point<MODE == FIELD_GRAD ? 1 : 0>(G, list, etab, l, sg_shift, px, py, pz, val, g, taps);
        if (l == 0) {
            if (O.val) O.val[t] = val;
            if (MODE == FIELD_GRAD && O.grad) { O.grad[3 * t] = g[0]; O.grad[3 * t + 1] = g[1]; O.grad[3 * t + 2] = g[2]; }
            if (O.taps) O.taps[t] = taps;
        }
    } else if (MODE == FIELD_NORMALS) {
        float nv[3] = {0.0f, 0.0f, 0.0f};
        if (finite) {
            field_point<1>(G, list, etab, l, sg_shift, px, py, pz, val, g, taps);
            const double g2 = (double)g[0] * g[0] + (double)g[1] * g[1] + (double)g[2] * g[2];
            if (g2 > 0.0 && isfinite(g2)) {
                const double len = sqrt(g2);
                nv[0] = (float)(-(double)g[0] / len); nv[1] = (float)(-(double)g[1] / len); nv[2] = (float)(-(double)g[2] / len);
            }
        }
        if (l == 0) { O.grad[3 * t] = nv[0]; O.grad[3 * t + 1] = nv[1]; O.grad[3 * t + 2] = nv[2]; }
    } else if (MODE == FIELD_HESS || MODE == FIELD_CURV) {
        float h[6] = {fnan, fnan, fnan, fnan, fnan, fnan};
        if (finite) field_point<2>(G, list, etab, l, sg_shift, px, py, pz, val, g, taps, h);
        float cv[4] = {fnan, fnan, fnan, fnan};
        if (MODE == FIELD_CURV && finite) {
            // curvatures of the level set through p with the normal -g / |g|, in Float64 from the Float32 g and H above
            const double gx = g[0], gy = g[1], gz = g[2];
            const double hxx = h[0], hyy = h[1], hzz = h[2], hxy = h[3], hxz = h[4], hyz = h[5];
            const double g2 = gx * gx + gy * gy + gz * gz;
            if (g2 > 0.0 && isfinite(g2)) {
                const double ghg = gx * (hxx * gx + hxy * gy + hxz * gz) + gy * (hxy * gx + hyy * gy + hyz * gz) +
                                   gz * (hxz * gx + hyz * gy + hzz * gz);
                const double axx = hyy * hzz - hyz * hyz, ayy = hxx * hzz - hxz * hxz, azz = hxx * hyy - hxy * hxy;
                const double axy = hxz * hyz - hxy * hzz, axz = hxy * hyz - hxz * hyy, ayz = hxy * hxz - hxx * hyz;
                const double gag = gx * (axx * gx + axy * gy + axz * gz) + gy * (axy * gx + ayy * gy + ayz * gz) +
                                   gz * (axz * gx + ayz * gy + azz * gz);
                const double mean = -(g2 * (hxx + hyy + hzz) - ghg) / (2.0 * g2 * sqrt(g2));
                const double gauss = gag / (g2 * g2);
                const double root = sqrt(fmax(mean * mean - gauss, 0.0));
                cv[0] = (float)mean; cv[1] = (float)gauss; cv[2] = (float)(mean + root); cv[3] = (float)(mean - root);
            }
        }
        if (l == 0) {
            if (O.val) O.val[t] = val;
            if (O.grad) { O.grad[3 * t] = g[0]; O.grad[3 * t + 1] = g[1]; O.grad[3 * t + 2] = g[2]; }
            if (O.hess) {
#pragma unroll
                for (int a = 0; a < 6; ++a) O.hess[6 * t + a] = h[a];
            }
            if (O.taps) O.taps[t] = taps;
            if (MODE == FIELD_CURV) {
#pragma unroll
                for (int a = 0; a < 4; ++a) O.curv[4 * t + a] = cv[a];
            }
        }
    } else {
        int status = 3, it = 0;
        if (finite) {
            for (;;) {
                field_point<1>(G, list, etab, l, sg_shift, px, py, pz, val, g, taps);
                if (fabsf(val) <= O.tol) { status = 0; break; }
                if (it >= O.max_iter) { status = 1; break; }
                const double g2 = (double)g[0] * g[0] + (double)g[1] * g[1] + (double)g[2] * g[2];
                if (!(g2 > 0.0) || !isfinite(g2)) { status = 2; break; }
                double s = (double)val / g2;
                const double len = fabs((double)val) / sqrt(g2);
                if (len > (double)G.cell) s *= (double)G.cell / len;
                px = (float)((double)px - s * (double)g[0]);
                py = (float)((double)py - s * (double)g[1]);
                pz = (float)((double)pz - s * (double)g[2]);
                ++it;
            }
        }
        if (l == 0) {
            if (finite) { O.points[3 * t] = px; O.points[3 * t + 1] = py; O.points[3 * t + 2] = pz; }
            if (O.status) O.status[t] = status;
            if (O.resid) O.resid[t] = finite ? fabsf(val) : fnan;
            if (O.iters) O.iters[t] = it;
        }
    }
}

}  // namespace

struct r2s_rbf_field {
    int device;
    r2s_grid grid;
    double kthr;
    int64_t n;
    DevBuf w, cx, cy, cz;
    FieldGeom G;
};

namespace {

int field_args(const r2s_grid* g, double kthr)
{
    if (!(kthr >= R2S_RBF_MIN_KERNEL_THRESHOLD && kthr < 1.0))
        return fail(R2S_ERR_ARG, "kernel threshold must be in [%g, 1): got %g", R2S_RBF_MIN_KERNEL_THRESHOLD, kthr);
    if (g->N[0] < 1 || g->N[1] < 1 || g->N[2] < 1 || !(g->cell_size > 0.0) || !std::isfinite(g->cell_size))
        return fail(R2S_ERR_ARG, "grid: every N must be >= 1 and cell_size positive");
    // the box of a point is found from aabb_min and cell_size, the nodes lie on range(aabb_min, aabb_max): both must describe
    // the same lattice (r2s_grid_make's grids do), to well within the box's margin of 1 % of a cell
    for (int a = 0; a < 3; ++a) {
        const double end = g->aabb_min[a] + (double)g->N[a] * g->cell_size;
        if (!(std::fabs(g->aabb_max[a] - end) <= 1e-3 * g->cell_size))
            return fail(R2S_ERR_ARG, "grid: aabb_max[%d] = %.17g is not aabb_min + N * cell_size = %.17g", a, g->aabb_max[a], end);
    }
    const double n = (double)(g->N[0] + 1) * (double)(g->N[1] + 1) * (double)(g->N[2] + 1);
    if (n > 2147483647.0) return fail(R2S_ERR_UNSUPPORTED, "rbf field: more than 2^31 - 1 lattice nodes");
    return 0;
}

// geometry + axes on the current device; the weights buffer is allocated, not filled
int field_make(const r2s_grid* g, double kthr, int device, r2s_rbf_field** out)
{
    int dev = device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    r2s_rbf_field* f = new r2s_rbf_field();
    f->device = dev;
    f->grid = *g;
    f->kthr = kthr;
    FieldGeom& G = f->G;
    memset(&G, 0, sizeof G);
    G.nx = (int)g->N[0] + 1; G.ny = (int)g->N[1] + 1; G.nz = (int)g->N[2] + 1;
    f->n = (int64_t)G.nx * G.ny * G.nz;
    const double sigma = g->cell_size;                                          // :346
    const double R = std::sqrt(-std::log(kthr));
    G.max_distance = (float)std::sqrt(-std::log(kthr) * sigma * sigma);          // :221
    G.inv_h = 1.0 / g->cell_size;
    G.inv_sigma = 1.0 / sigma;
    G.gscale = -2.0 / (sigma * sigma);
    G.cell = (float)g->cell_size;
    // the Float32 axes differ from aabb_min + i * cell_size by their rounding (2^-24 relative, doubled for the range's
    // own arithmetic and the end point); the box of a point takes that, and 1 % of a cell, as margin
    double cmax = 0.0;
    for (int a = 0; a < 3; ++a) {
        G.amin[a] = g->aabb_min[a];
        cmax = std::max(cmax, std::max(std::fabs(g->aabb_min[a]), std::fabs(g->aabb_max[a])));
    }
    const double margin = 0.01 + cmax * std::ldexp(1.0, -21) * G.inv_h;
    G.reach = R + margin;
    auto destroy = [&]() { r2s_rbf_field_destroy(f); };
    if (!(2.0 * G.reach + 1.0 < 15.0)) {
        destroy();
        return fail(R2S_ERR_UNSUPPORTED, "rbf field: coordinates of magnitude %g are too coarse in Float32 for cells of %g", cmax, g->cell_size);
    }
    // every node inside a support lies within reach + sqrt(3)/2 cells of the lattice node nearest to the point
    {
        const double rb = G.reach + 0.8661;
        const int m = (int)std::ceil(rb);
        int count = 0;
        for (int k = -m; k <= m; ++k)
            for (int j = -m; j <= m; ++j)
                for (int i = -m; i <= m; ++i) count += (double)(i * i + j * j + k * k) <= rb * rb;
        G.cap = (count + 1) & ~1;
    }
    // the smallest workgroup (64 threads) holds 4 lists and the exp table in the LDS a launch gets without opting in
    if ((size_t)(64 / FIELD_SG) * G.cap * sizeof(uint2) + 512 > 48u * 1024u) {
        destroy();
        return fail(R2S_ERR_UNSUPPORTED, "rbf field: a support of up to %d nodes (threshold %g, coordinates of magnitude %g against cells of %g) "
                    "exceeds the evaluator's per-point list", G.cap, kthr, cmax, g->cell_size);
    }
    std::vector<float> ax[3];
    const int nn[3] = {G.nx, G.ny, G.nz};
    DevBuf* bufs[3] = {&f->cx, &f->cy, &f->cz};
    for (int a = 0; a < 3; ++a) {
        r2s_int::rbf_coarse_axis(g->aabb_min[a], g->aabb_max[a], nn[a], ax[a]);
        if (bufs[a]->ensure(sizeof(float) * (size_t)nn[a])) { destroy(); return fail(R2S_ERR_NOMEM, "hipMalloc failed"); }
        const hipError_t e = hipMemcpy(bufs[a]->p, ax[a].data(), sizeof(float) * (size_t)nn[a], hipMemcpyHostToDevice);
        if (e != hipSuccess) { destroy(); return fail(R2S_ERR_HIP, "%s", hipGetErrorString(e)); }
    }
    if (f->w.ensure_exact(sizeof(float) * (size_t)f->n)) { destroy(); return fail(R2S_ERR_NOMEM, "hipMalloc of %zu bytes failed", sizeof(float) * (size_t)f->n); }
    G.cx = f->cx.as<float>(); G.cy = f->cy.as<float>(); G.cz = f->cz.as<float>();
    G.w = f->w.as<float>();
    *out = f;
    return 0;
}

template <int MODE>
int field_launch(const r2s_rbf_field* f, const float* d_pts, int64_t n, const FieldOut& O, hipStream_t st)
{
    // points per workgroup: as many as keep the lists within 48 KB of LDS
    int threads = 256;
    while (threads > 64 && (size_t)(threads / FIELD_SG) * f->G.cap * sizeof(uint2) > 48u * 1024u) threads /= 2;
    const size_t lds = (size_t)(threads / FIELD_SG) * f->G.cap * sizeof(uint2);
    const int ppb = threads / FIELD_SG;
    const int64_t blocks = (n + ppb - 1) / ppb;
    if (blocks > 2147483647LL) return fail(R2S_ERR_UNSUPPORTED, "rbf field: too many points for one launch");
    rbf_field_kernel<MODE><<<(unsigned)blocks, threads, lds, st>>>(f->G, d_pts, n, O);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the field's device must be the current one for device-pointer calls
int field_on_current(const r2s_rbf_field* f)
{
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != f->device) return fail(R2S_ERR_ARG, "rbf field lives on device %d, the current device is %d", f->device, cur);
    return 0;
}

int eval_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_val, float* d_grad, int32_t* d_taps, hipStream_t st)
{
    FieldOut O;
    memset(&O, 0, sizeof O);
    O.val = d_val; O.grad = d_grad; O.taps = d_taps;
    if (!d_val && !d_grad && !d_taps) return 0;
    return d_grad ? field_launch<FIELD_GRAD>(f, d_points, n, O, st) : field_launch<FIELD_VALUE>(f, d_points, n, O, st);
}

int hessian_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_val, float* d_grad, float* d_hess, int32_t* d_taps,
                hipStream_t st)
{
    if (!d_hess) return eval_dev(f, d_points, n, d_val, d_grad, d_taps, st);   // (the same numbers from the cheaper kernel)
    FieldOut O;
    memset(&O, 0, sizeof O);
    O.val = d_val; O.grad = d_grad; O.hess = d_hess; O.taps = d_taps;
    return field_launch<FIELD_HESS>(f, d_points, n, O, st);
}

int curvature_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_curv, float* d_grad, float* d_hess, hipStream_t st)
{
    FieldOut O;
    memset(&O, 0, sizeof O);
    O.curv = d_curv; O.grad = d_grad; O.hess = d_hess;
    return field_launch<FIELD_CURV>(f, d_points, n, O, st);
}

int normals_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_normals, hipStream_t st)
{
    FieldOut O;
    memset(&O, 0, sizeof O);
    O.grad = d_normals;
    return field_launch<FIELD_NORMALS>(f, d_points, n, O, st);
}

int project_dev(const r2s_rbf_field* f, float* d_points, int64_t n, int max_iter, float tol, int32_t* d_status, float* d_resid,
                int32_t* d_iters, hipStream_t st)
{
    FieldOut O;
    memset(&O, 0, sizeof O);
    O.points = d_points; O.status = d_status; O.resid = d_resid; O.iters = d_iters; O.max_iter = max_iter; O.tol = tol;
    return field_launch<FIELD_PROJECT>(f, d_points, n, O, st);
}

// host arrays <-> temporaries on the field's device
struct HostIo {
    DevBuf b[5];
    int up(int i, const void* src, size_t bytes)
    {
        ENSURE(b[i], bytes);
        if (src) HIP_TRY(hipMemcpy(b[i].p, src, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    int down(int i, void* dst, size_t bytes)
    {
        if (dst) HIP_TRY(hipMemcpy(dst, b[i].p, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};

int points_args(const r2s_rbf_field* f, const void* points, int64_t n)
{
    if (!f) return fail(R2S_ERR_ARG, "null field");
    if (n < 0) return fail(R2S_ERR_ARG, "negative point count");
    if (n > 0 && !points) return fail(R2S_ERR_ARG, "null points");
    return 0;
}

int project_args(int32_t max_iter, float tol)
{
    if (max_iter < 0 || !(tol >= 0.0f)) return fail(R2S_ERR_ARG, "projection: max_iter must be >= 0 and tol >= 0");
    return 0;
}

}  // namespace

extern "C" {

int r2s_rbf_field_from_weights(const float* weights, const r2s_grid* grid, double kernel_threshold, float level_shift,
                               int32_t device, r2s_rbf_field** out)
{
    if (!weights || !grid || !out) return fail(R2S_ERR_ARG, "null argument");
    int rc = field_args(grid, kernel_threshold);
    if (rc || (rc = use_device(device))) return rc;
    r2s_rbf_field* f = nullptr;
    if ((rc = field_make(grid, kernel_threshold, device, &f))) return rc;
    const hipError_t e = hipMemcpy(f->w.p, weights, sizeof(float) * (size_t)f->n, hipMemcpyHostToDevice);
    if (e != hipSuccess) { r2s_rbf_field_destroy(f); return fail(R2S_ERR_HIP, "%s", hipGetErrorString(e)); }
    f->G.th = level_shift;
    *out = f;
    return 0;
}

int r2s_rbf_field_fit(const double* sdf, const r2s_grid* grid, int32_t is_interp, double kernel_threshold, double target_volume,
                      int32_t device, r2s_rbf_field** out, float* level_shift_out, int32_t* cg_iters_out)
{
    if (!sdf || !grid || !out) return fail(R2S_ERR_ARG, "null argument");
    int rc = field_args(grid, kernel_threshold);
    if (rc || (rc = use_device(device))) return rc;
    r2s_rbf_field* f = nullptr;
    if ((rc = field_make(grid, kernel_threshold, device, &f))) return rc;
    float th = 0.0f;
    int its = 0;
    rc = r2s_int::rbf_fit_weights(sdf, grid, is_interp, kernel_threshold, target_volume, f->w.as<float>(), &th, &its);
    if (rc) { r2s_rbf_field_destroy(f); return rc; }
    f->G.th = th;
    if (level_shift_out) *level_shift_out = th;
    if (cg_iters_out) *cg_iters_out = its;
    *out = f;
    return 0;
}

int r2s_rbf_field_weights(const r2s_rbf_field* f, float* weights_out, float* level_shift_out)
{
    if (!f) return fail(R2S_ERR_ARG, "null field");
    if (weights_out) {
        HIP_TRY(hipSetDevice(f->device));
        HIP_TRY(hipMemcpy(weights_out, f->w.p, sizeof(float) * (size_t)f->n, hipMemcpyDeviceToHost));
    }
    if (level_shift_out) *level_shift_out = f->G.th;
    return 0;
}

void r2s_rbf_field_destroy(r2s_rbf_field* f)
{
    if (!f) return;
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != f->device && hipSetDevice(f->device) == hipSuccess;
    delete f;   // (its buffers free themselves, on the field's device)
    if (sw) (void)hipSetDevice(cur);
}

int r2s_rbf_field_eval_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_val, float* d_grad, int32_t* d_taps,
                           void* stream)
{
    int rc = points_args(f, d_points, n);
    if (rc || n == 0 || (rc = field_on_current(f))) return rc;
    return eval_dev(f, d_points, n, d_val, d_grad, d_taps, (hipStream_t)stream);
}

int r2s_rbf_field_eval(const r2s_rbf_field* f, const float* points, int64_t n, float* val_out, float* grad_out, int32_t* taps_out)
{
    int rc = points_args(f, points, n);
    if (rc || n == 0 || (!val_out && !grad_out && !taps_out)) return rc;
    HIP_TRY(hipSetDevice(f->device));
    HostIo io;
    const size_t N = (size_t)n;
    rc = io.up(0, points, 12 * N);
    if (!rc && val_out) rc = io.up(1, nullptr, 4 * N);
    if (!rc && grad_out) rc = io.up(2, nullptr, 12 * N);
    if (!rc && taps_out) rc = io.up(3, nullptr, 4 * N);
    if (!rc) rc = eval_dev(f, io.b[0].as<float>(), n, val_out ? io.b[1].as<float>() : nullptr, grad_out ? io.b[2].as<float>() : nullptr,
                           taps_out ? io.b[3].as<int32_t>() : nullptr, nullptr);
    if (!rc) rc = io.down(1, val_out, 4 * N);
    if (!rc) rc = io.down(2, grad_out, 12 * N);
    if (!rc) rc = io.down(3, taps_out, 4 * N);
    return rc;
}

int r2s_rbf_field_hessian_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_val, float* d_grad, float* d_hess,
                              int32_t* d_taps, void* stream)
{
    int rc = points_args(f, d_points, n);
    if (rc || n == 0 || (rc = field_on_current(f))) return rc;
    return hessian_dev(f, d_points, n, d_val, d_grad, d_hess, d_taps, (hipStream_t)stream);
}

int r2s_rbf_field_hessian(const r2s_rbf_field* f, const float* points, int64_t n, float* val_out, float* grad_out, float* hess_out,
                          int32_t* taps_out)
{
    int rc = points_args(f, points, n);
    if (rc || n == 0 || (!val_out && !grad_out && !hess_out && !taps_out)) return rc;
    HIP_TRY(hipSetDevice(f->device));
    HostIo io;
    const size_t N = (size_t)n;
    rc = io.up(0, points, 12 * N);
    if (!rc && val_out) rc = io.up(1, nullptr, 4 * N);
    if (!rc && grad_out) rc = io.up(2, nullptr, 12 * N);
    if (!rc && taps_out) rc = io.up(3, nullptr, 4 * N);
    if (!rc && hess_out) rc = io.up(4, nullptr, 24 * N);
    if (!rc) rc = hessian_dev(f, io.b[0].as<float>(), n, val_out ? io.b[1].as<float>() : nullptr, grad_out ? io.b[2].as<float>() : nullptr,
                              hess_out ? io.b[4].as<float>() : nullptr, taps_out ? io.b[3].as<int32_t>() : nullptr, nullptr);
    if (!rc) rc = io.down(1, val_out, 4 * N);
    if (!rc) rc = io.down(2, grad_out, 12 * N);
    if (!rc) rc = io.down(3, taps_out, 4 * N);
    if (!rc) rc = io.down(4, hess_out, 24 * N);
    return rc;
}

int r2s_rbf_field_curvature_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_curv, float* d_grad, float* d_hess,
                                void* stream)
{
    int rc = points_args(f, d_points, n);
    if (rc || n == 0) return rc;
    if (!d_curv) return fail(R2S_ERR_ARG, "null curvature output");
    if ((rc = field_on_current(f))) return rc;
    return curvature_dev(f, d_points, n, d_curv, d_grad, d_hess, (hipStream_t)stream);
}

int r2s_rbf_field_curvature(const r2s_rbf_field* f, const float* points, int64_t n, float* curv_out, float* grad_out, float* hess_out)
{
    int rc = points_args(f, points, n);
    if (rc || n == 0) return rc;
    if (!curv_out) return fail(R2S_ERR_ARG, "null curvature output");
    HIP_TRY(hipSetDevice(f->device));
    HostIo io;
    const size_t N = (size_t)n;
    rc = io.up(0, points, 12 * N);
    if (!rc) rc = io.up(1, nullptr, 16 * N);
    if (!rc && grad_out) rc = io.up(2, nullptr, 12 * N);
    if (!rc && hess_out) rc = io.up(3, nullptr, 24 * N);
    if (!rc) rc = curvature_dev(f, io.b[0].as<float>(), n, io.b[1].as<float>(), grad_out ? io.b[2].as<float>() : nullptr,
                                hess_out ? io.b[3].as<float>() : nullptr, nullptr);
    if (!rc) rc = io.down(1, curv_out, 16 * N);
    if (!rc) rc = io.down(2, grad_out, 12 * N);
    if (!rc) rc = io.down(3, hess_out, 24 * N);
    return rc;
}

int r2s_rbf_field_normals_dev(const r2s_rbf_field* f, const float* d_points, int64_t n, float* d_normals, void* stream)
{
    int rc = points_args(f, d_points, n);
    if (rc || n == 0) return rc;
    if (!d_normals) return fail(R2S_ERR_ARG, "null normals");
    if ((rc = field_on_current(f))) return rc;
    return normals_dev(f, d_points, n, d_normals, (hipStream_t)stream);
}

int r2s_rbf_field_normals(const r2s_rbf_field* f, const float* points, int64_t n, float* normals_out)
{
    int rc = points_args(f, points, n);
    if (rc || n == 0) return rc;
    if (!normals_out) return fail(R2S_ERR_ARG, "null normals");
    HIP_TRY(hipSetDevice(f->device));
    HostIo io;
    const size_t N = (size_t)n;
    rc = io.up(0, points, 12 * N);
    if (!rc) rc = io.up(1, nullptr, 12 * N);
    if (!rc) rc = normals_dev(f, io.b[0].as<float>(), n, io.b[1].as<float>(), nullptr);
    if (!rc) rc = io.down(1, normals_out, 12 * N);
    return rc;
}

int r2s_rbf_field_project_dev(const r2s_rbf_field* f, float* d_points_inout, int64_t n, int32_t max_iter, float tol,
                              int32_t* d_status, float* d_resid, int32_t* d_iters, void* stream)
{
    int rc = points_args(f, d_points_inout, n);
    if (rc || (rc = project_args(max_iter, tol)) || n == 0 || (rc = field_on_current(f))) return rc;
    return project_dev(f, d_points_inout, n, max_iter, tol, d_status, d_resid, d_iters, (hipStream_t)stream);
}

int r2s_rbf_field_project(const r2s_rbf_field* f, float* points_inout, int64_t n, int32_t max_iter, float tol, int32_t* status_out,
                          float* resid_out, int32_t* iters_out)
{
    int rc = points_args(f, points_inout, n);
    if (rc || (rc = project_args(max_iter, tol)) || n == 0) return rc;
    HIP_TRY(hipSetDevice(f->device));
    HostIo io;
    const size_t N = (size_t)n;
    rc = io.up(0, points_inout, 12 * N);
    if (!rc && status_out) rc = io.up(1, nullptr, 4 * N);
    if (!rc && resid_out) rc = io.up(2, nullptr, 4 * N);
    if (!rc && iters_out) rc = io.up(3, nullptr, 4 * N);
    if (!rc) rc = project_dev(f, io.b[0].as<float>(), n, max_iter, tol, status_out ? io.b[1].as<int32_t>() : nullptr,
                              resid_out ? io.b[2].as<float>() : nullptr, iters_out ? io.b[3].as<int32_t>() : nullptr, nullptr);
    if (!rc) rc = io.down(0, points_inout, 12 * N);
    if (!rc) rc = io.down(1, status_out, 4 * N);
    if (!rc) rc = io.down(2, resid_out, 4 * N);
    if (!rc) rc = io.down(3, iters_out, 4 * N);
    return rc;
}

}  // extern "C"
