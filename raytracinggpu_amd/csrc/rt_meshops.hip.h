// rt_meshops.hip.h -- device-side mesh transform + BVH refit.  Included by rt_capi.hip.
//
// transform_kernel  = the `transform` kernel of global_launcher.cu:340-365 (realtime_render.cu:1151-1166 launches the
//                     same): v' = R v (row-major 3x3, products summed left to right) then += translation.
// retri_kernel      = the per-triangle precompute of rt_scene_upload on the device: (A, e1, e2, N) with the operations
//                     of moller_trumbore (cpu:227-229), triangles in visit order.
// refit_kernel      = every node's box recomputed for the EXISTING tree and triangle order: a leaf's box is
//                     compute_bbox of its triangles (cpu:180-188: INF-initialised std::min / std::max), an internal
//                     node's box the union of its children's, which is compute_bbox of its whole range.  One workgroup
//                     walks the levels bottom-up (the tree has a few thousand nodes; this is a step before the hot path).
//                     The synthetic union nodes of a forest (rt_host_scene.hip.h build_forest) are recomputed the way
//                     build_forest makes them: per axis the min / max over both children's lo AND hi, then one float
//                     step outwards on every face -- so a refitted forest is laid out as a fresh upload of the moved meshes.
// The reference never refits (its transform variant has no BVH and buildBVH runs once on the host); rebuilding on the
// host after a transform remains possible through rt_scene_upload.
#pragma once
#include "rt_travq.hip.h"

namespace rtk {

struct Mat3 { float r[9]; float t[3]; };

__global__ __launch_bounds__(256) void transform_kernel(float4 *__restrict__ verts, int nv, const Mat3 m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const float4 v = verts[i];
    float x = m.r[0] * v.x + m.r[1] * v.y + m.r[2] * v.z;
    float y = m.r[3] * v.x + m.r[4] * v.y + m.r[5] * v.z;
    float z = m.r[6] * v.x + m.r[7] * v.y + m.r[8] * v.z;
    x += m.t[0]; y += m.t[1]; z += m.t[2];
    verts[i] = make_float4(x, y, z, 0.f);
}

__global__ __launch_bounds__(256) void retri_kernel(const int4 *__restrict__ tidx, const float4 *__restrict__ verts, float4 *__restrict__ tri, int nt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int4 ix = tidx[t];
    const float4 a = verts[ix.x], b = verts[ix.y], c = verts[ix.z];
    const f3 A = mk(a.x, a.y, a.z), B = mk(b.x, b.y, b.z), C = mk(c.x, c.y, c.z);
    const f3 e1 = B - A, e2 = C - A, N = cross(e1, e2);               // cpu:227-229
    tri[3 * (size_t)t + 0] = make_float4(A.x, A.y, A.z, e1.x);
    tri[3 * (size_t)t + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    tri[3 * (size_t)t + 2] = make_float4(e2.z, N.x, N.y, N.z);
}

constexpr int kMaxSynthetic = kMaxMeshes - 1;               // a forest of K <= 16 meshes has K - 1 synthetic nodes

struct RefitArgs {
    float4 *node_lo, *node_hi, *nodes2, *nodesq, *nodesb;   // the node layouts (pre-order SoA, pre-order interleaved, breadth-first as boxes and as centre / half extent)
    const int *q2thr, *left_of, *lvl_nodes, *lvl_off;
    const int4 *tidx;
    const float4 *verts;
    int n_nodes, n_levels;
    int n_syn;                                              // the forest's synthetic nodes (pre-order indices); 0 for one mesh
    int syn[kMaxSynthetic];
};

// std::nextafter(x, -inf) / (x, +inf) on the bits (no denormal flush can touch them): what build_forest does on the host
__device__ __forceinline__ float step_down(float x) {
    if (x != x || x == -INFINITY) return x;
    if (x == 0.f) return __int_as_float((int)0x80000001);
    const int b = __float_as_int(x);
    return __int_as_float(x > 0.f ? b - 1 : b + 1);
}
__device__ __forceinline__ float step_up(float x) {
    if (x != x || x == INFINITY) return x;
    if (x == 0.f) return __int_as_float(1);
    const int b = __float_as_int(x);
    return __int_as_float(x > 0.f ? b + 1 : b - 1);
}
__device__ __forceinline__ float fmin_std(float a, float b) { return b < a ? b : a; }   // std::min
__device__ __forceinline__ float fmax_std(float a, float b) { return a < b ? b : a; }   // std::max

__global__ __launch_bounds__(1024) void refit_kernel(const RefitArgs a) {
    for (int L = a.n_levels - 1; L >= 0; --L) {
        for (int k = a.lvl_off[L] + (int)threadIdx.x; k < a.lvl_off[L + 1]; k += (int)blockDim.x) {
            const int x = a.lvl_nodes[k];
            float4 lo = a.node_lo[x], hi = a.node_hi[x];
            const int hiw = __float_as_int(hi.w), low = __float_as_int(lo.w);
            f3 mn = mk(1e9f, 1e9f, 1e9f), mx = mk(-1e9f, -1e9f, -1e9f);          // BoundingBox(), cpu:135 (INF narrowed)
            if (hiw >= 0) {                                            // leaf: compute_bbox over triangles [low, hiw)
                for (int t = low; t < hiw; ++t) {
                    const int4 ix = a.tidx[t];
                    const int vi[3] = {ix.x, ix.y, ix.z};
                    for (int j = 0; j < 3; ++j) {
                        const float4 v = a.verts[vi[j]];
                        mn.x = v.x < mn.x ? v.x : mn.x; mn.y = v.y < mn.y ? v.y : mn.y; mn.z = v.z < mn.z ? v.z : mn.z;   // std::min(mn, v)
                        mx.x = mx.x < v.x ? v.x : mx.x; mx.y = mx.y < v.y ? v.y : mx.y; mx.z = mx.z < v.z ? v.z : mx.z;   // std::max(mx, v)
                    }
                }
            } else {                                                   // internal: children x + 1 and left_of[x] (one level down: done)
                const int c[2] = {x + 1, a.left_of[x]};
                bool syn = false;
                for (int j = 0; j < a.n_syn; ++j) syn |= a.syn[j] == x;
                if (syn) {                                             // build_forest's union: min / max over lo and hi of the left child, then of the right one; one step outwards
                    const float4 l0 = a.node_lo[c[1]], h0 = a.node_hi[c[1]], l1 = a.node_lo[c[0]], h1 = a.node_hi[c[0]];
                    lo.x = step_down(fmin_std(fmin_std(l0.x, h0.x), fmin_std(l1.x, h1.x))); hi.x = step_up(fmax_std(fmax_std(l0.x, h0.x), fmax_std(l1.x, h1.x)));
                    lo.y = step_down(fmin_std(fmin_std(l0.y, h0.y), fmin_std(l1.y, h1.y))); hi.y = step_up(fmax_std(fmax_std(l0.y, h0.y), fmax_std(l1.y, h1.y)));
                    lo.z = step_down(fmin_std(fmin_std(l0.z, h0.z), fmin_std(l1.z, h1.z))); hi.z = step_up(fmax_std(fmax_std(l0.z, h0.z), fmax_std(l1.z, h1.z)));
                    a.node_lo[x] = lo; a.node_hi[x] = hi;
                    continue;
                }
                for (int j = 0; j < 2; ++j) {
                    const float4 cl = a.node_lo[c[j]], ch = a.node_hi[c[j]];
                    mn.x = cl.x < mn.x ? cl.x : mn.x; mn.y = cl.y < mn.y ? cl.y : mn.y; mn.z = cl.z < mn.z ? cl.z : mn.z;
                    mx.x = mx.x < ch.x ? ch.x : mx.x; mx.y = mx.y < ch.y ? ch.y : mx.y; mx.z = mx.z < ch.z ? ch.z : mx.z;
                }
            }
            lo.x = mn.x; lo.y = mn.y; lo.z = mn.z; hi.x = mx.x; hi.y = mx.y; hi.z = mx.z;
            a.node_lo[x] = lo; a.node_hi[x] = hi;
        }
        __threadfence_block();
        __syncthreads();
    }
    // the other two layouts carry the same boxes (their .w fields keep their own meaning)
    for (int x = (int)threadIdx.x; x < a.n_nodes; x += (int)blockDim.x) {
        const float4 lo = a.node_lo[x], hi = a.node_hi[x];
        float4 l2 = a.nodes2[2 * x], h2 = a.nodes2[2 * x + 1];
        l2.x = lo.x; l2.y = lo.y; l2.z = lo.z; h2.x = hi.x; h2.y = hi.y; h2.z = hi.z;
        a.nodes2[2 * x] = l2; a.nodes2[2 * x + 1] = h2;
    }
    for (int k = 1 + (int)threadIdx.x; k <= a.n_nodes; k += (int)blockDim.x) {   // breadth-first array: node k lives at index k (0 is padding)
        const int x = a.q2thr[k];
        const float4 lo = a.node_lo[x], hi = a.node_hi[x];
        float4 lq = a.nodesq[2 * k], hq = a.nodesq[2 * k + 1];
        lq.x = lo.x; lq.y = lo.y; lq.z = lo.z; hq.x = hi.x; hq.y = hi.y; hq.z = hi.z;
        a.nodesq[2 * k] = lq; a.nodesq[2 * k + 1] = hq;
        float4 cb = a.nodesb[2 * k], hb = a.nodesb[2 * k + 1];        // wf_travq's form of the same box (their .w fields keep payload and kind)
        cb.x = box_centre(lo.x, hi.x); cb.y = box_centre(lo.y, hi.y); cb.z = box_centre(lo.z, hi.z);
        hb.x = box_half(lo.x, hi.x); hb.y = box_half(lo.y, hi.y); hb.z = box_half(lo.z, hi.z);
        a.nodesb[2 * k] = cb; a.nodesb[2 * k + 1] = hb;
    }
}

// ---- The same refit across the chip (rt_mesh_set_vertices*: a mesh that changes shape every frame).  refit_kernel above is one workgroup: adequate for a mesh moved once, one
// compute unit of 256 for a tree of a million nodes.  Here every leaf has a thread, and the internal nodes are made by the climb of qdp_up_kernel (rt_qnodes.hip.h, whose header
// carries the memory-model argument) and lbvh_boxes_kernel (rt_lbvh.hip.h): the thread publishes its node's box, fences, announces itself at the parent's counter; the first
// arrival returns, the second fences and reads BOTH children past the L1 -- in refit_kernel's fixed order (x + 1, then left_of[x]) and with refit_kernel's expressions, so a box is
// a function of the tree and the vertices, never of which sibling came second, and equals refit_kernel's bit for bit.  No lane waits for another: no flag is spun on, no barrier
// spans the grid, no workgroup hands work on; a climb is bounded by the node count.
//   * ONE lane per leaf, its triangles in ascending order, corners x, y, z: the serial loop of refit_kernel, word for word, so -0 / +0 ties and a NaN vertex come out as there.
//     (Splitting a leaf's range over lanes would be exact too -- `v < mn ? v : mn` keeps the FIRST of equal values and never takes a NaN, so merging the partial results of
//     consecutive ranges in range order with the same comparison gives the first occurrence of the minimum, as the serial loop does -- but the LBVH's leaves hold at most
//     32 triangles and the reference's stop rule leaves fewer than five unless centroids coincide: the leaf that would gain is a degenerate mesh's, and the lane that
//     made the leaf goes on to climb with the box in registers.)
//   * The parent of every node in pre-order indices comes from left_of on the device (refit_parent_kernel): the LBVH's device-side install never has the tree on the host.
//     parent[] is filled with -1 and the counters with 0 on the stream before every refit.
//   * The three derived layouts are copied by a grid-wide kernel after the climb (refit_kernel's two closing loops).
struct RefitWide { RefitArgs r; int *parent, *cnt; };

__global__ __launch_bounds__(256) void refit_parent_kernel(const RefitWide a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.r.n_nodes || __float_as_int(a.r.node_hi[x].w) >= 0) return;          // leaves have no children
    const int l = a.r.left_of[x];
    if (x + 1 < a.r.n_nodes) a.parent[x + 1] = x;
    if (l > x + 1 && l < a.r.n_nodes) a.parent[l] = x;
}

__global__ __launch_bounds__(256) void refit_up_kernel(const RefitWide a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.r.n_nodes) return;
    const int hiw = __float_as_int(a.r.node_hi[x].w), low = __float_as_int(a.r.node_lo[x].w);
    if (hiw < 0) return;                                                            // leaves start the climb
    auto put = [&](int n, f3 mn, f3 mx) {                                           // the box alone: the .w fields (skip link / triangle range) are the tree's and stay
        float *lo = reinterpret_cast<float *>(a.r.node_lo + n), *hi = reinterpret_cast<float *>(a.r.node_hi + n);
        lo[0] = mn.x; lo[1] = mn.y; lo[2] = mn.z; hi[0] = mx.x; hi[1] = mx.y; hi[2] = mx.z;
    };
    auto ld = [&](const float4 *q) {                                                // a child's box: written by another workgroup, read past the L1
        const float *p = reinterpret_cast<const float *>(q);
        return mk(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                  __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    };
    {
        f3 mn = mk(1e9f, 1e9f, 1e9f), mx = mk(-1e9f, -1e9f, -1e9f);              // BoundingBox(), cpu:135 (INF narrowed)
        for (int t = low; t < hiw; ++t) {                                           // compute_bbox over triangles [low, hiw), as refit_kernel
            const int4 ix = a.r.tidx[t];
            const int vi[3] = {ix.x, ix.y, ix.z};
            for (int j = 0; j < 3; ++j) {
                const float4 v = a.r.verts[vi[j]];
                mn.x = v.x < mn.x ? v.x : mn.x; mn.y = v.y < mn.y ? v.y : mn.y; mn.z = v.z < mn.z ? v.z : mn.z;   // std::min(mn, v)
                mx.x = mx.x < v.x ? v.x : mx.x; mx.y = mx.y < v.y ? v.y : mx.y; mx.z = mx.z < v.z ? v.z : mx.z;   // std::max(mx, v)
            }
        }
        put(x, mn, mx);
    }
    int cur = a.parent[x];
    for (int guard = 0; cur >= 0 && cur < a.r.n_nodes && guard <= a.r.n_nodes; ++guard) {   // (a climb is at most the tree's depth long; the range test and the guard only bound a corrupted tree)
        __threadfence();                                                            // my box is visible before I announce myself
        if (atomicAdd(&a.cnt[cur], 1) == 0) return;                                 // first to arrive: the sibling's thread goes on from here
        __threadfence();
        const int c[2] = {cur + 1, a.r.left_of[cur]};
        if (c[0] >= a.r.n_nodes || c[1] < 0 || c[1] >= a.r.n_nodes) return;
        bool syn = false;
        for (int j = 0; j < a.r.n_syn; ++j) syn |= a.r.syn[j] == cur;
        f3 mn = mk(1e9f, 1e9f, 1e9f), mx = mk(-1e9f, -1e9f, -1e9f);
        if (syn) {                                                                  // build_forest's union, as refit_kernel: min / max over lo and hi of the left child, then of the right one; one step outwards
            const f3 l0 = ld(a.r.node_lo + c[1]), h0 = ld(a.r.node_hi + c[1]), l1 = ld(a.r.node_lo + c[0]), h1 = ld(a.r.node_hi + c[0]);
            mn.x = step_down(fmin_std(fmin_std(l0.x, h0.x), fmin_std(l1.x, h1.x))); mx.x = step_up(fmax_std(fmax_std(l0.x, h0.x), fmax_std(l1.x, h1.x)));
            mn.y = step_down(fmin_std(fmin_std(l0.y, h0.y), fmin_std(l1.y, h1.y))); mx.y = step_up(fmax_std(fmax_std(l0.y, h0.y), fmax_std(l1.y, h1.y)));
            mn.z = step_down(fmin_std(fmin_std(l0.z, h0.z), fmin_std(l1.z, h1.z))); mx.z = step_up(fmax_std(fmax_std(l0.z, h0.z), fmax_std(l1.z, h1.z)));
        } else {
            for (int j = 0; j < 2; ++j) {
                const f3 cl = ld(a.r.node_lo + c[j]), ch = ld(a.r.node_hi + c[j]);
                mn.x = cl.x < mn.x ? cl.x : mn.x; mn.y = cl.y < mn.y ? cl.y : mn.y; mn.z = cl.z < mn.z ? cl.z : mn.z;
                mx.x = mx.x < ch.x ? ch.x : mx.x; mx.y = mx.y < ch.y ? ch.y : mx.y; mx.z = mx.z < ch.z ? ch.z : mx.z;
            }
        }
        put(cur, mn, mx);
        cur = a.parent[cur];
    }
}

// the other layouts carry the same boxes (their .w fields keep their own meaning): thread k copies pre-order node k into nodes2 and breadth-first node k (0 is padding) into nodesq / nodesb
__global__ __launch_bounds__(256) void refit_copy_kernel(const RefitArgs a) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > a.n_nodes) return;
    if (k < a.n_nodes) {
        const float4 lo = a.node_lo[k], hi = a.node_hi[k];
        float4 l2 = a.nodes2[2 * k], h2 = a.nodes2[2 * k + 1];
        l2.x = lo.x; l2.y = lo.y; l2.z = lo.z; h2.x = hi.x; h2.y = hi.y; h2.z = hi.z;
        a.nodes2[2 * k] = l2; a.nodes2[2 * k + 1] = h2;
    }
    if (k >= 1) {
        const int x = a.q2thr[k];
        const float4 lo = a.node_lo[x], hi = a.node_hi[x];
        float4 lq = a.nodesq[2 * k], hq = a.nodesq[2 * k + 1];
        lq.x = lo.x; lq.y = lo.y; lq.z = lo.z; hq.x = hi.x; hq.y = hi.y; hq.z = hi.z;
        a.nodesq[2 * k] = lq; a.nodesq[2 * k + 1] = hq;
        float4 cb = a.nodesb[2 * k], hb = a.nodesb[2 * k + 1];        // wf_travq's form of the same box (their .w fields keep payload and kind)
        cb.x = box_centre(lo.x, hi.x); cb.y = box_centre(lo.y, hi.y); cb.z = box_centre(lo.z, hi.z);
        hb.x = box_half(lo.x, hi.x); hb.y = box_half(lo.y, hi.y); hb.z = box_half(lo.z, hi.z);
        a.nodesb[2 * k] = cb; a.nodesb[2 * k + 1] = hb;
    }
}

// the caller's positions (`stride` floats apart: xyz or xyzw records) into the mesh's range of the float4 vertex buffer, .w = 0 as an upload leaves it
__global__ __launch_bounds__(256) void repack_vertices_kernel(const float *__restrict__ src, int stride, float4 *__restrict__ verts, int nv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const float *p = src + (size_t)i * stride;
    verts[i] = make_float4(p[0], p[1], p[2], 0.f);
}

}  // namespace rtk
