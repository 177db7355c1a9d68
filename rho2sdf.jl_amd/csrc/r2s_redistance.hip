// Redistancing: the exact Euclidean distance from the points of a regular lattice to an indexed triangle mesh within a band,
// and the signed forms on the iso-surface of a field: banded, and unbanded through the mesh index of r2s_mesh_index.hip
// (include/rho2sdf_hip.h, r2s_mesh_distance / r2s_redistance / r2s_redistance_full); the lattice and mesh checks both files use.
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

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"
#include "r2s_tri_math.hpp"

using namespace r2s_int;

namespace {

constexpr int TS = 8;          // voxels per tile edge
constexpr int CHUNK = 128;     // triangle records per LDS chunk

struct MdArgs {
    int64_t nx, ny, nz;        // lattice points
    int64_t ntx, nty, ntz;     // tiles
    double o[3];
    double h, band, bandm;     // bandm = band + 2 * margin
    double margin;
    int64_t ntris;
};

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
            const double f = load_real(field, field_f32, i);
            if (!(f >= iso)) d = -d;
        }
        store_real(out, out_f32, i, d);
        if (closest) closest[i] = idx;
    }
}

// work buffers of the distance calls, kept per device between calls (r2s_release_cache frees them)
struct DistWork {
    DevBuf cnt, off, list, flag;            // binning
    DevBuf verts, tris, out, idx, field;   // host-pointer variants / the extracted surface
};
PerDevice<DistWork> g_dist_work;

// [0] ms surface extraction, [1] ms binning (count, scan, fills), [2] ms tile kernel, [3] tile/triangle pairs, [4] batches,
// [5] triangles, [6] tiles, [7] tiles with triangles
thread_local double g_dist_stats[8];

}  // namespace

namespace r2s_int {

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

int check_mesh_host(const char* who, const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris)
{
    for (int64_t i = 0; i < 3 * n_tris; ++i)
        if (tris[i] < 0 || tris[i] >= n_verts)
            return fail(R2S_ERR_ARG, "%s: triangle %lld has vertex index %d outside [0, %lld)", who, (long long)(i / 3), tris[i],
                        (long long)n_verts);
    for (int64_t i = 0; i < 3 * n_verts; ++i)
        if (!std::isfinite(verts[i])) return fail(R2S_ERR_ARG, "%s: vertex %lld is not finite", who, (long long)(i / 3));
    return 0;
}

int check_mesh_dev(const char* who, const float* d_verts, int64_t n_verts, const int32_t* d_tris, int64_t n_tris, DevBuf& flag,
                   hipStream_t st)
{
    const int64_t n_check = 3 * std::max(n_verts, n_tris);
    if (n_check == 0) return 0;
    ENSURE(flag, sizeof(int32_t));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int32_t), st));
    md_check_kernel<<<(unsigned)((n_check + 255) / 256), 256, 0, st>>>(d_verts, n_verts, d_tris, n_tris, flag.as<int32_t>());
    HIP_TRY(hipGetLastError());
    int32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, flag.p, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(R2S_ERR_ARG, "%s: a triangle index lies outside [0, %lld) or a vertex is not finite", who, (long long)n_verts);
    return 0;
}

int upload_mesh(DevBuf& dv, DevBuf& dt, const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, bool from_device,
                hipStream_t st)
{
    ENSURE(dv, vert_bytes(std::max<int64_t>(n_verts, 1)));
    ENSURE(dt, tri_bytes(std::max<int64_t>(n_tris, 1)));
    const auto copy = [&](void* dst, const void* src, size_t bytes) {
        return from_device ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    };
    if (n_verts) HIP_TRY(copy(dv.p, verts, vert_bytes(n_verts)));
    if (n_tris) HIP_TRY(copy(dt.p, tris, tri_bytes(n_tris)));
    return 0;
}

}  // namespace r2s_int

namespace {

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
    Event a, b;
    hipStream_t st;
    float total = 0.0f;
    bool open = false;
    explicit Timer(hipStream_t s) : st(s)
    {
        if (hipEventCreate(&a.h) != hipSuccess || hipEventCreate(&b.h) != hipSuccess) (void)hipGetLastError();
    }
    void start()
    {
        if (a.h && b.h) (void)hipEventRecord(a, st), open = true;
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

// the iso-surface of the device field into w.verts / w.tris (count, size the buffers, fill); nv / nt: its vertices / triangles
int extract_surface(const char* who, const void* d_values, bool f32, const int64_t dims[3], const double origin[3], double spacing,
                    double iso, hipStream_t st, DistWork& w, int64_t& nv, int64_t& nt)
{
    nv = nt = 0;
    int rc = r2s_extract_isosurface_dev(d_values, f32 ? 1 : 0, dims, origin, spacing, iso, nullptr, 0, nullptr, 0, &nv, &nt, st);
    if (rc) return rc;
    if (nt > INT32_MAX) return fail(R2S_ERR_UNSUPPORTED, "%s: %lld triangles do not fit 32-bit indices", who, (long long)nt);
    if (nv == 0 && nt == 0) return 0;
    ENSURE(w.verts, vert_bytes(std::max<int64_t>(nv, 1)));
    ENSURE(w.tris, tri_bytes(std::max<int64_t>(nt, 1)));
    return r2s_extract_isosurface_dev(d_values, f32 ? 1 : 0, dims, origin, spacing, iso, w.verts.as<float>(), nv, w.tris.as<int32_t>(), nt,
                                      &nv, &nt, st);
}

int redistance_core(const void* d_values, bool f32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                    double band, void* d_out, hipStream_t st, DistWork& w)
{
    Timer t_iso(st);
    t_iso.start();
    int64_t nv, nt;
    int rc = extract_surface("redistance", d_values, f32, dims, origin, spacing, iso, st, w, nv, nt);
    if (rc) return rc;
    t_iso.stop();
    rc = mesh_distance_core(w.verts.as<float>(), w.tris.as<int32_t>(), nt, dims, origin, spacing, band, d_values, f32, iso, d_out, f32,
                            nullptr, st, w);
    g_dist_stats[0] = t_iso.total;
    return rc;
}

int redistance_full_core(const void* d_values, bool f32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                         void* d_out, hipStream_t st, DistWork& w)
{
    int64_t nv, nt;
    int rc = extract_surface("redistance_full", d_values, f32, dims, origin, spacing, iso, st, w, nv, nt);
    if (rc) return rc;
    MiTree T;   // (the nodes are freed on return: after the stream has drained)
    rc = mi_build_tree(w.verts.as<float>(), nv, w.tris.as<int32_t>(), nt, st, T);
    if (!rc) rc = mi_query(T, nullptr, false, 0, dims, origin, spacing, d_values, f32, iso, d_out, f32, nullptr, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) return fail(R2S_ERR_HIP, "redistance_full: %s", hipGetErrorString(e));
    return rc;
}

// The four r2s_redistance* entry points: banded (redistance_core) or not (redistance_full_core); on a host field, staged through
// w.field / w.out on `device`, or (host = false) on a device field of the current device after the work queued on `stream`.
int redistance_call(const char* who, bool banded, bool host, const void* values, int32_t is_float32, const int64_t dims[3],
                    const double origin[3], double spacing, double iso, double band, int32_t device, void* out, void* stream)
{
    int rc = lattice_args(who, dims, origin, spacing, banded ? band : 1.0);
    if (rc) return rc;
    if (std::isnan(iso)) return fail(R2S_ERR_ARG, "%s: iso is NaN", who);
    if (!values || !out) return fail(R2S_ERR_ARG, "%s: null values / output", who);
    if ((rc = host ? use_device(device) : check_device(0))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_work.mu);
    DistWork* wp = g_dist_work.current(rc);
    if (rc) return rc;
    DistWork& w = *wp;
    const size_t bytes = real_bytes(is_float32) * (size_t)(dims[0] * dims[1] * dims[2]);
    const void* d_values = values;
    void* d_out = out;
    if (host) {
        ENSURE(w.field, bytes);
        ENSURE(w.out, bytes);
        HIP_TRY(hipMemcpy(w.field.p, values, bytes, hipMemcpyHostToDevice));
        d_values = w.field.p, d_out = w.out.p;
    }
    rc = banded ? redistance_core(d_values, is_float32 != 0, dims, origin, spacing, iso, band, d_out, (hipStream_t)stream, w)
                : redistance_full_core(d_values, is_float32 != 0, dims, origin, spacing, iso, d_out, (hipStream_t)stream, w);
    if (rc || !host) return rc;
    HIP_TRY(hipMemcpy(out, w.out.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int r2s_mesh_distance(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int64_t dims[3],
                      const double origin[3], double spacing, double band, int32_t out_is_float32, int32_t device, void* dist_out,
                      int32_t* closest_tri_out)
{
    int rc = lattice_args("mesh_distance", dims, origin, spacing, band);
    if (rc || (rc = mesh_args("mesh_distance", verts, n_verts, tris, n_tris))) return rc;
    if (!dist_out) return fail(R2S_ERR_ARG, "mesh_distance: null output");
    if ((rc = check_mesh_host("mesh_distance", verts, n_verts, tris, n_tris)) || (rc = use_device(device))) return rc;
    std::lock_guard<std::mutex> lock(g_dist_work.mu);
    DistWork* wp = g_dist_work.current(rc);
    if (rc) return rc;
    DistWork& w = *wp;
    const size_t nvox = (size_t)(dims[0] * dims[1] * dims[2]), esz = real_bytes(out_is_float32);
    ENSURE(w.out, esz * nvox);
    if (closest_tri_out) ENSURE(w.idx, sizeof(int32_t) * nvox);
    if ((rc = upload_mesh(w.verts, w.tris, verts, n_verts, tris, n_tris, false, nullptr))) return rc;
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
    std::lock_guard<std::mutex> lock(g_dist_work.mu);
    DistWork* wp = g_dist_work.current(rc);
    if (rc) return rc;
    DistWork& w = *wp;
    const hipStream_t st = (hipStream_t)stream;
    if ((rc = check_mesh_dev("mesh_distance", d_verts, n_verts, d_tris, n_tris, w.flag, st))) return rc;
    g_dist_stats[0] = 0.0;
    return mesh_distance_core(d_verts, d_tris, n_tris, dims, origin, spacing, band, nullptr, false, 0.0, d_dist_out, out_is_float32 != 0,
                              d_closest_tri_out, st, w);
}

int r2s_redistance(const void* values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                   double band, int32_t device, void* out)
{
    return redistance_call("redistance", true, true, values, is_float32, dims, origin, spacing, iso, band, device, out, nullptr);
}

int r2s_redistance_dev(const void* d_values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing,
                       double iso, double band, void* d_out, void* stream)
{
    return redistance_call("redistance", true, false, d_values, is_float32, dims, origin, spacing, iso, band, 0, d_out, stream);
}

int r2s_redistance_full(const void* values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing, double iso,
                        int32_t device, void* out)
{
    return redistance_call("redistance_full", false, true, values, is_float32, dims, origin, spacing, iso, 0.0, device, out, nullptr);
}

int r2s_redistance_full_dev(const void* d_values, int32_t is_float32, const int64_t dims[3], const double origin[3], double spacing,
                            double iso, void* d_out, void* stream)
{
    return redistance_call("redistance_full", false, false, d_values, is_float32, dims, origin, spacing, iso, 0.0, 0, d_out, stream);
}

void r2s_last_distance_stats(double out[8])
{
    if (out) std::memcpy(out, g_dist_stats, sizeof g_dist_stats);
}

}  // extern "C"
