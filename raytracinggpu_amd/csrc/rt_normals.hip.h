// rt_normals.hip.h -- rt_mesh_compute_normals[_of]: the vertex normals of a mesh's CURRENT shape on the device.  Included by rt_capi.hip beside
// rt_meshops.hip.h, whose retri_kernel writes the face normals these kernels sum.
//
// vertex_normals_kernel  = one lane per position vertex.  The lane walks the vertex's range of the adjacency (CSR: `off` by vertex, `rank` = the visit ranks of the corners
//                          that name it, ascending in the mesh's own triangle order, a triangle that names the vertex twice listed twice) SERIALLY: S = the first face
//                          normal, then S = S + N component by component -- the order is the definition (raytrace_hip.h), so no atomics, no LDS and no cross-lane sum.
//                          N = tri[3 t + 2].yzw = cross(B - A, C - A), twice the triangle's area long: the area weight.  n = normalize(S), or zeros where !(dot(S, S) > 0)
//                          (no triangle, faces that cancel, degenerate faces, a NaN).  A valence is a handful (5.3 on the cat), and the 48-byte records of neighbouring
//                          vertices share cache lines; a lane's loop is as long as the longest valence of its wave.
// corner_normals_kernel  = one lane per corner of the part's visit range: nrm[3 t + k] = (vn[tidx[t].k], 0), the layout smooth_normal reads.
#pragma once
#include "rt_meshops.hip.h"

namespace rtk {

__global__ __launch_bounds__(256) void vertex_normals_kernel(const int *__restrict__ off, const int *__restrict__ rank, const float4 *__restrict__ tri, int n_tris,
                                                             float4 *__restrict__ vn, int v0, int nv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int v = v0 + i;
    const int b = off[v], e = off[v + 1];
    f3 S = mk(0.f, 0.f, 0.f);
    bool first = true;
    for (int j = b; j < e; ++j) {
        const int t = rank[j];
        if ((unsigned)t >= (unsigned)n_tris) continue;                // (the adjacency is the host's own; the test only bounds a corrupted one)
        const float4 q2 = tri[3 * (size_t)t + 2];
        const f3 N = mk(q2.y, q2.z, q2.w);
        S = first ? N : S + N;                                        // the first face normal as it is (a -0 stays -0), then one rounding per component and face
        first = false;
    }
    f3 n = mk(0.f, 0.f, 0.f);
    if (dot(S, S) > 0.f) n = normalize(S);
    vn[v] = make_float4(n.x, n.y, n.z, 0.f);
}

__global__ __launch_bounds__(256) void corner_normals_kernel(const int4 *__restrict__ tidx, const float4 *__restrict__ vn, int n_verts, float4 *__restrict__ nrm, int n_corners) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_corners) return;
    const int4 ix = tidx[c / 3];
    const int k = c % 3, v = k == 0 ? ix.x : (k == 1 ? ix.y : ix.z);
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)v < (unsigned)n_verts) n = vn[v];
    nrm[c] = make_float4(n.x, n.y, n.z, 0.f);
}

}  // namespace rtk
