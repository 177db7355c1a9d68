// What the traversals of the mesh index share across files (r2s_mesh_index.hip: distance and ray queries; r2s_mesh_intersect.hip:
// self-intersection pairs; r2s_mesh_winding.hip: winding number and signed distance; r2s_mesh_nesting.hip: containment of
// patches): the index object, the node of its tree and how
// a wavefront reads it, the box of a triangle, the depth of the per-lane stack, the host checks every entry point on an index makes
// and the staging of a host-pointer call.  One definition for all files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "r2s_common.hpp"
#include "r2s_internal.hpp"

// (the DevBuf members free themselves: r2s_mesh_index_destroy deletes the index with its device current)
struct r2s_mesh_index {
    int device = 0;
    DevBuf verts, tris;
    r2s_int::MiTree tree;
};

namespace r2s_int {

constexpr int MI_STACK = 64;   // stack entries per lane; a tree of height h needs at most h (one pending sibling per level)

struct MiNode {
    float box[2][6];      // child c: lo xyz, hi xyz
    int32_t child[2];
    int32_t height[2];    // 0 = leaf
};
static_assert(sizeof(MiNode) == 64, "MiNode is read as four 16-byte words");

__device__ inline MiNode load_node(const MiNode* p)
{
    const uint4* w = reinterpret_cast<const uint4*>(p);
    union {
        uint4 q[4];
        MiNode n;
    } u;
    u.q[0] = w[0], u.q[1] = w[1], u.q[2] = w[2], u.q[3] = w[3];
    return u.n;
}

// the AABB of the triangle with the corners a, b, c (three floats each)
__device__ inline void tri_box(const float* a, const float* b, const float* c, float lo[3], float hi[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(a[k], fminf(b[k], c[k]));
        hi[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
    }
}

// may the axis ray from o along +e_KZ (neg: -e_KZ) meet something inside the float32 box b (lo xyz, hi xyz)?  The three exact
// comparisons of the own-box condition of the pair test (axis_cross, r2s_tri_math.hpp): the cull of the winding and of the nesting
template <int KZ>
__device__ inline bool axis_enter(const float* __restrict__ b, double o1, double o2, double oz, bool neg)
{
    constexpr int K1 = (KZ + 1) % 3, K2 = (KZ + 2) % 3;
    const bool ahead = neg ? (double)b[KZ] <= oz : (double)b[3 + KZ] >= oz;
    return (double)b[K1] <= o1 && o1 <= (double)b[3 + K1] && (double)b[K2] <= o2 && o2 <= (double)b[3 + K2] && ahead;
}

// the traversal kernels keep one pending sibling per level on a per-lane stack of MI_STACK entries (r2s_mesh_index.hip)
int check_depth(const MiTree& T);
// R2S_ERR_ARG unless the index's device is the current one; `who` heads the error text (r2s_mesh_index.hip)
int index_on_current_device(const char* who, const r2s_mesh_index* ix);

// makes the index's device current for a host-pointer call and restores the caller's on scope exit
struct DeviceScope {
    int prev = -1;
    int enter(int device)
    {
        HIP_TRY(hipGetDevice(&prev));
        if (prev != device) HIP_TRY(hipSetDevice(device));
        return 0;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};


// One array of a host-pointer call: `bytes` on the device, uploaded from `in`, downloaded to `out` (both null: not wanted, no buffer)
struct HostIo {
    const void* in;
    void* out;
    size_t bytes;
};

// a host-pointer call: on the index's device, stage the arrays, run `enqueue` on their buffers (null stream), wait, copy the results back
template <class F>
int staged_call(const r2s_mesh_index* ix, const std::vector<HostIo>& io, F enqueue)
{
    int rc = check_device(0);
    if (rc) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(ix->device))) return rc;
    std::vector<DevBuf> buf(io.size());   // (freed before the caller's device is current again)
    for (size_t k = 0; k < io.size(); ++k) {
        if (io[k].in || io[k].out) ENSURE(buf[k], io[k].bytes);
        if (io[k].in) HIP_TRY(hipMemcpy(buf[k].p, io[k].in, io[k].bytes, hipMemcpyHostToDevice));
    }
    if ((rc = enqueue(buf.data()))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (size_t k = 0; k < io.size(); ++k)
        if (io[k].out) HIP_TRY(hipMemcpy(io[k].out, buf[k].p, io[k].bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace r2s_int
