// rt_demodulate.hip.h -- rt_demodulate[_device] / rt_modulate[_device]: divide the recorded surface's albedo out of a colour frame, multiply it back in.
// Included at the end of rt_capi.hip (same translation unit: the host half uses rt_host_post.hip.h); it reads plane 2 of rt_aov_surface.hip.h.
//
// Scene::getColor makes a pixel whose chain ends on a diffuse surface exactly albedo (.) (l / pi + what follows) (fold_segment, cpu:624, 642-644): the noise is in the
// second factor.  A filter that runs between the two calls works on that factor, and a texture's detail -- all of it in the first -- comes back untouched.
// One elementwise kernel, two instantiations: 16 bytes of colour and 16 of plane 2 in, 16 out per pixel.  The quotient is the correctly rounded one: the shared
// sequence of rt_div.h where its range holds, the literal division behind a wave-uniform branch elsewhere (raytrace_hip.h states the contract;
// tests/surface_model.py is its numpy twin).
#pragma once
#include "rt_div.h"

namespace rtk {

// c / d (DIVIDE) or c * d for a divisor d > 0
template <bool DIVIDE>
__device__ __forceinline__ float dm_channel(float c, float a, float albedo_floor, bool &slow) {
    const float d = fmaxf(a, albedo_floor);                           // maxNum: a NaN albedo takes the floor
    if (!(d > 0.f)) return c;                                         // zero, negative or NaN: the channel passes through
    if (!DIVIDE) return c * d;
    slow = slow || !(div_in_range(d) && div_in_range(c));
    return div_by(c, d, div_refine(d, __builtin_amdgcn_rcpf(d)));
}

template <bool DIVIDE>
__global__ __launch_bounds__(256) void demodulate_kernel(const float4 *C, const float4 *__restrict__ A, float4 *out, int n, float albedo_floor) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = C[i], a = A[i];                                  // (out may be C itself: in place)
    float4 o = c;
    if (a.w == 1.f) {
        bool slow = false;
        o.x = dm_channel<DIVIDE>(c.x, a.x, albedo_floor, slow);
        o.y = dm_channel<DIVIDE>(c.y, a.y, albedo_floor, slow);
        o.z = dm_channel<DIVIDE>(c.z, a.z, albedo_floor, slow);
        if (DIVIDE) {
            if (__builtin_expect(__ballot(slow) != 0ull, 0)) {
                if (slow) {                                           // outside the shared sequence's range (a zero colour, a denormal): the literal quotient
                    const float dx = fmaxf(a.x, albedo_floor), dy = fmaxf(a.y, albedo_floor), dz = fmaxf(a.z, albedo_floor);
                    if (dx > 0.f) o.x = c.x / dx;
                    if (dy > 0.f) o.y = c.y / dy;
                    if (dz > 0.f) o.z = c.z / dz;
                }
            }
        }
    }
    out[i] = o;
}

}  // namespace rtk

static int dm_check(rt_ctx *ctx, const void *color, const void *aov, int64_t n_pixels, const void *out) {
    if (!color || !aov || !out) return fail(ctx, RT_ERR_INVALID, "color/aov/out is NULL");
    if (n_pixels <= 0 || n_pixels >= kPostMaxPixels) return fail(ctx, RT_ERR_INVALID, "n_pixels must be positive and below 2^28");
    const size_t bytes = (size_t)n_pixels * sizeof(float4);
    if ((out != color && overlaps(out, bytes, color, bytes)) || overlaps(out, bytes, aov, 3 * bytes))
        return fail(ctx, RT_ERR_INVALID, "the output overlaps an input (only out == color, in place, is allowed)");
    return RT_OK;
}

template <bool DIVIDE>
static int dm_device(rt_ctx *ctx, const void *color_dev, const void *aov_dev, int64_t n_pixels, float albedo_floor, void *out_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = dm_check(ctx, color_dev, aov_dev, n_pixels, out_dev);
    if (rc != RT_OK) return rc;
    const int n = (int)n_pixels;
    const size_t bytes = (size_t)n * sizeof(float4);
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    note_between(ctx, q, {{color_dev, bytes}, {out_dev, bytes}});     // a pipelined frame must not overtake this read of a frame / write of an image
    hipLaunchKernelGGL(rtk::demodulate_kernel<DIVIDE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, static_cast<const float4 *>(color_dev),
                       static_cast<const float4 *>(aov_dev) + 2 * (size_t)n, static_cast<float4 *>(out_dev), n, albedo_floor);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

template <bool DIVIDE>
static int dm_host(rt_ctx *ctx, const float *color_host, const float *aov_host, int64_t n_pixels, float albedo_floor, float *out_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    const int rc = dm_check(ctx, color_host, aov_host, n_pixels, out_host);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)n_pixels * sizeof(float4);
    // colour (filtered in place: the result is where it was), the three planes
    return staged(ctx, {{color_host, bytes}, {aov_host, 3 * bytes}}, 0, bytes, out_host,
                  [&](uint8_t *d) { return dm_device<DIVIDE>(ctx, d, d + bytes, n_pixels, albedo_floor, d, nullptr); });
}

extern "C" int rt_demodulate_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, int64_t n_pixels, float albedo_floor, void *out_rgba_dev, void *stream) {
    return dm_device<true>(ctx, color_rgba_dev, aov_dev, n_pixels, albedo_floor, out_rgba_dev, stream);
}
extern "C" int rt_modulate_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, int64_t n_pixels, float albedo_floor, void *out_rgba_dev, void *stream) {
    return dm_device<false>(ctx, color_rgba_dev, aov_dev, n_pixels, albedo_floor, out_rgba_dev, stream);
}
extern "C" int rt_demodulate(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, int64_t n_pixels, float albedo_floor, float *out_rgba_host) {
    return dm_host<true>(ctx, color_rgba_host, aov_host, n_pixels, albedo_floor, out_rgba_host);
}
extern "C" int rt_modulate(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, int64_t n_pixels, float albedo_floor, float *out_rgba_host) {
    return dm_host<false>(ctx, color_rgba_host, aov_host, n_pixels, albedo_floor, out_rgba_host);
}
