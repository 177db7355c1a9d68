// What r2s_mesh_shells.hip, r2s_mesh_sections.hip, r2s_mesh_orient.hip, r2s_mesh_fans.hip and r2s_mesh_holes.hip share: the box
// of the vertices behind the reference point, the collapsed-triangle test, the integer union-find with min-root, (shells, orient,
// fans, holes) the per-group integer counting and (orient, fans, holes) the size of a run of sorted half-edges.  r2s_mesh_weld.hip takes the order-preserving bit pattern
// of a float32 and the launch / bit-count helpers from here.  Everything has internal linkage: each file gets its own copy of
// the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace {

__device__ inline uint32_t ms_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
inline float ms_unordered(uint32_t u)
{
    const uint32_t b = (u >> 31) ? (u & 0x7fffffffu) : ~u;
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}

__device__ inline bool ms_collapsed(const int32_t* __restrict__ tris, int64_t t, int32_t& i0, int32_t& i1, int32_t& i2)
{
    i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    return i0 == i1 || i1 == i2 || i0 == i2;
}

// bb[0..2] = min, bb[3..5] = max over all vertices, as ordered bit patterns (bb starts as ~0, ~0, ~0, 0, 0, 0)
__global__ void __launch_bounds__(256) ms_bounds_kernel(const float* __restrict__ verts, int64_t nverts, uint64_t* __restrict__ small)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (v < nverts) {
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = ms_ordered(verts[3 * v + k]);
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
            atomicMin((unsigned long long*)&small[k], (unsigned long long)lo[k]);
            atomicMax((unsigned long long*)&small[3 + k], (unsigned long long)hi[k]);
        }
    }
}

// the reference point of the header from the six patterns ms_bounds_kernel left: per axis 0.5 * (lo + hi)
inline void ms_ref_point(const uint64_t* bb, int64_t n_verts, double r[3])
{
    for (int k = 0; k < 3; ++k)
        r[k] = n_verts > 0 ? 0.5 * ((double)ms_unordered((uint32_t)bb[k]) + (double)ms_unordered((uint32_t)bb[3 + k])) : 0.0;
}

// parents are rewritten by other CUs during the kernel: bypass the per-CU L1
__device__ inline uint32_t ms_load(const uint32_t* L, uint32_t i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; every visited node is pointed at its grandparent (atomicMin: a parent only ever moves to a smaller ancestor)
__device__ inline uint32_t ms_find(uint32_t* L, uint32_t x)
{
    for (;;) {
        const uint32_t p = ms_load(L, x);
        if (p == x) return x;
        const uint32_t g = ms_load(L, p);
        if (g != p) atomicMin(&L[x], g);
        x = g;
    }
}

__device__ inline void ms_union(uint32_t* L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = ms_find(L, a);
        b = ms_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }   // link the larger root under the smaller
        if (atomicCAS(&L[a], a, b) == a) return;             // a was still a root
    }
}

// (orient, fans, holes) the sorted half-edge keys are (min << 33) | (max << 1) | direction, the collapsed triangles' keys behind them.
// The number of members of the run of sorted half-edge i, capped at 3 (i is a real half-edge: keys[i] < ckey)
__device__ inline int ms_run_size(const uint64_t* __restrict__ keys, int64_t i, int64_t nh, bool& head)
{
    const uint64_t e = keys[i] >> 1;
    const bool p1 = i >= 1 && (keys[i - 1] >> 1) == e, p2 = p1 && i >= 2 && (keys[i - 2] >> 1) == e;
    const bool n1 = i + 1 < nh && (keys[i + 1] >> 1) == e, n2 = n1 && i + 2 < nh && (keys[i + 2] >> 1) == e;
    head = !p1;
    if (!p1 && !n1) return 1;
    return (p2 || (p1 && n1) || n2) ? 3 : 2;
}

// adds 1 to counts[group][col0 + k] (rows of STRIDE) for every k < NC with add[k] set, over the workgroup's active threads: once
// per column when all of them name one group (a shell, a patch), else one atomic per entry.  Called by all 256 threads.
template <int NC, int STRIDE = 8>
__device__ inline void ms_count(bool active, int32_t group, const bool add[NC], int col0, int64_t* __restrict__ counts)
{
    __shared__ int32_t s_group, s_mixed;
    __shared__ uint32_t s_cnt[NC];
    if (threadIdx.x == 0) s_group = -1, s_mixed = 0;
    if (threadIdx.x < NC) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    if (active) atomicCAS(&s_group, -1, group);
    __syncthreads();
    if (active && group != s_group) s_mixed = 1;
    __syncthreads();
    if (s_mixed) {
        if (active) {
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (add[k]) atomicAdd((unsigned long long*)&counts[(int64_t)group * STRIDE + col0 + k], 1ull);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const unsigned long long m = __ballot(active && add[k]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt[k], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < NC && s_group >= 0 && s_cnt[threadIdx.x])
        atomicAdd((unsigned long long*)&counts[(int64_t)s_group * STRIDE + col0 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

inline unsigned ms_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
inline unsigned ms_bits(uint64_t max_value)
{
    unsigned b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

}  // namespace
