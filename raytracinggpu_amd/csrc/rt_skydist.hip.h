// rt_skydist.hip.h -- the sampling table of the environment map (rt_scene_set_environment_sampling; the rule: raytrace_hip.h "sky sampling"; the draw: sky_draw in
// rt_shade.hip.h), built on the device in four launches over the texels t = y * n + x:
//   sky_dist_weights    W(t) = fl(B9(t) / fl(m rt_sqrtf(m))): the 3 x 3 clamped sum of Y = fl(fl(R + G) + B) over the solid-angle factor at the texel's centre, and
//                       the map's maximum (the bits of non-negative floats order as the floats do: an atomic max on them is exact in any order)
//   sky_dist_quantise   c(t) = W > 0 ? max(1, (uint32)(fl(W / Wmax) 2^31)) : 0, and the sum of c over every kSkyBlock texels
//   sky_dist_scan       ONE workgroup: the inclusive 64-bit scan of those sums, in place, kSkyScanLevel per round with a running carry
//   sky_dist_prefix     prefix[t] = the sums of the blocks before + the inclusive scan inside the block
// The shape is the sample plan's (rt_adaptive.hip.h): nothing waits for another workgroup, and the sums are integers, so the table is the same whatever the workgroup
// count.  The host reads the maximum back between the first two launches (zero: the table is empty) and the total after the last.
#pragma once
#include "rt_kernels.hip.h"

namespace rtk {

constexpr int kSkyScanLevel = 1024;                  // block sums the scan's one workgroup takes per round

__global__ __launch_bounds__(kSkyBlock) void sky_dist_weights(const float4 *__restrict__ texels, int n, float *__restrict__ W, unsigned int *__restrict__ wmax_bits) {
    __shared__ unsigned int smax[kSkyBlock];
    const int t = blockIdx.x * kSkyBlock + (int)threadIdx.x;
    float w = 0.f;
    if (t < n * n) {
        const int y = t / n, x = t - y * n;
        float b9 = 0.f;                                                // (+0 + Y = Y exactly: Y is +0 or positive)
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = tex_wrap(y + dy, n, 1);
            for (int dx = -1; dx <= 1; ++dx) {
                const float4 v = texels[yy * n + tex_wrap(x + dx, n, 1)];
                b9 = b9 + ((v.x + v.y) + v.z);
            }
        }
        const float nf = (float)n;
        const f3 p = sky_oct_point(sky_q((float)x + 0.5f, nf), sky_q((float)y + 0.5f, nf));
        const float m = norm2(p);
        w = div_quot(b9, m * rt_sqrtf(m));
        W[t] = w;
    }
    smax[threadIdx.x] = __float_as_uint(w);
    __syncthreads();
    for (int s = kSkyBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { const unsigned int o = smax[threadIdx.x + s]; if (o > smax[threadIdx.x]) smax[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(wmax_bits, smax[0]);
}

// The weights of the table of the EMISSIVE MESHES (raytrace_hip.h "emissive meshes"; the draw: emit_draw in rt_shade.hip.h) over the scene's triangles in visit order:
// W(t) = fl(A2(t) Y(obj of t)), A2 = rt_sqrtf(norm2(Nt)) of the record's raw normal, +0 for a triangle of a mesh that does not emit; the maximum as above.  The other
// three launches are the sky's, unchanged.  The meshes' triangle ranges come as an argument read in a wave-uniform loop (mesh_of_tri's): no lane indexes it.
struct EmitMeshes { int n; int tri_begin[kMaxMeshes]; float Y[kMaxMeshes]; };   // in object order, as Scene::mesh; Y of each mesh's radiance
__global__ __launch_bounds__(kSkyBlock) void emit_dist_weights(const float4 *__restrict__ tri, int nt, const EmitMeshes em, float *__restrict__ W, unsigned int *__restrict__ wmax_bits) {
    __shared__ unsigned int smax[kSkyBlock];
    const int t = blockIdx.x * kSkyBlock + (int)threadIdx.x;
    float w = 0.f;
    if (t < nt) {
        float Y = em.Y[0];
        for (int k = 1; k < em.n; ++k) Y = (t >= em.tri_begin[k]) ? em.Y[k] : Y;
        const float4 q2 = tri[3 * (size_t)t + 2];
        if (Y > 0.f) w = rt_sqrtf(norm2(mk(q2.y, q2.z, q2.w))) * Y;
        W[t] = w;
    }
    smax[threadIdx.x] = __float_as_uint(w);
    __syncthreads();
    for (int s = kSkyBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { const unsigned int o = smax[threadIdx.x + s]; if (o > smax[threadIdx.x]) smax[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(wmax_bits, smax[0]);
}

__global__ __launch_bounds__(kSkyBlock) void sky_dist_quantise(const float *__restrict__ W, int count, const unsigned int *__restrict__ wmax_bits, unsigned int *__restrict__ c,
                                                               unsigned long long *__restrict__ blk) {
    __shared__ unsigned long long ssum[kSkyBlock];
    const int t = blockIdx.x * kSkyBlock + (int)threadIdx.x;
    unsigned int ct = 0u;
    if (t < count) {
        const float w = W[t], wmax = __uint_as_float(wmax_bits[0]);
        if (w > 0.f) {
            const unsigned int k = (unsigned int)(div_quot(w, wmax) * 0x1p31f);   // the quotient is at most 1: the product is exact and at most 2^31
            ct = k < 1u ? 1u : k;
        }
        c[t] = ct;
    }
    ssum[threadIdx.x] = ct;
    __syncthreads();
    for (int s = kSkyBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) ssum[threadIdx.x] += ssum[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = ssum[0];
}

// inclusive scan of s[0 .. L) in LDS, L = blockDim.x (every thread of the workgroup calls it)
__device__ __forceinline__ void sky_lds_scan(unsigned long long *s, int L) {
    for (int off = 1; off < L; off <<= 1) {
        const unsigned long long v = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kSkyScanLevel) void sky_dist_scan(unsigned long long *__restrict__ blk, int nb) {
    __shared__ unsigned long long s[kSkyScanLevel];
    unsigned long long carry = 0ull;
    for (int b0 = 0; b0 < nb; b0 += kSkyScanLevel) {                   // (trip count uniform over the workgroup)
        const int b = b0 + (int)threadIdx.x;
        s[threadIdx.x] = b < nb ? blk[b] : 0ull;
        __syncthreads();
        sky_lds_scan(s, kSkyScanLevel);
        if (b < nb) blk[b] = carry + s[threadIdx.x];
        carry += s[kSkyScanLevel - 1];
        __syncthreads();                                               // s is rewritten by the next round
    }
}

__global__ __launch_bounds__(kSkyBlock) void sky_dist_prefix(const unsigned int *__restrict__ c, int count, const unsigned long long *__restrict__ blk,
                                                             unsigned long long *__restrict__ prefix) {
    __shared__ unsigned long long s[kSkyBlock];
    const int t = blockIdx.x * kSkyBlock + (int)threadIdx.x;
    s[threadIdx.x] = t < count ? (unsigned long long)c[t] : 0ull;
    __syncthreads();
    sky_lds_scan(s, kSkyBlock);
    if (t < count) prefix[t] = (blockIdx.x > 0 ? blk[blockIdx.x - 1] : 0ull) + s[threadIdx.x];
}

}  // namespace rtk
