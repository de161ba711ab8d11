// rt_rectify.hip.h -- rt_history_rectify[_device]: the long history of rt_temporal_accumulate_fast* clamped to the band of the fast one (history rectification:
// what makes the chain follow a light that moves, where no object, normal or plane changes and the reprojection accepts every pixel).
// Included at the end of rt_capi.hip, after rt_temporal.hip.h (same translation unit: lum709 of rt_denoise.hip.h, rt_sqrtf of rt_kernels.hip.h, rt_host_post.hip.h).
//
// Per pixel with a history older than the fast one: mean and deviation of the fast colour over the (2 R + 1)^2 window's pixels of the same object, the long colour
// clamped into mean +- k_clamp deviations, and where that moved it the history length cut to the fast one's and both moments shifted by the change of luminance
// (raytrace_hip.h states the formula; it is the contract: binary32, one rounding per operation, rows outer, dx inner; tests/rectify_model.py is its numpy twin).
// How it runs: one lane per pixel, a workgroup a tile of kRcTileW x kRcTileH of them (a wave = two rows of 32).  The window is an LDS tile with a halo of R: a
// neighbour gives its fast colour and its id and nothing else, so the two are packed into ONE 16-byte record (Fr, Fg, Fb, id) and a tap is one ds_read_b128 instead of
// two global loads of which one uses 4 bytes of 16.  A tap outside the image is staged with an id of NaN, which equals no id: the tap loop has no coordinate test.
// Bank conflicts: a 16-lane group of a ds_read_b128 lies within one 32-lane half, i.e. one tile row, and reads records x + {0-3, 12-15, 20-27} (or the other half),
// 16 distinct records modulo 16 = all 64 banks once, whatever the row pitch; the staging stores are consecutive records.  LDS is (32 + 2 R)(8 + 2 R) 16 B = 5.3, 6.8,
// 8.3 KiB a workgroup, far from limiting occupancy.  The pixel's own records (history 32 B, fast 16 B, plane 0's 16 B) are dense float4 loads, the output two dense
// float4 stores.  R is a template parameter: the 9, 25 or 49 taps are unrolled.  out == history is allowed: a lane reads its own two records before it writes them,
// and no lane reads another's (hence no __restrict__ on those two).
#pragma once
#include "rt_div.h"

namespace rtk {

constexpr int kRcTileW = 32, kRcTileH = 8;            // 256 lanes

template <int R>
__global__ __launch_bounds__(kRcTileW *kRcTileH) void history_rectify_kernel(const float4 *hist, const float4 *__restrict__ fast, const float4 *__restrict__ g, float4 *out, int W,
                                                                              int H, int tiles_x, float k_clamp) {
    constexpr int TW = kRcTileW + 2 * R, TH = kRcTileH + 2 * R;
    __shared__ float4 tile[TW * TH];
    const int tile_y = (int)blockIdx.x / tiles_x, tile_x = (int)blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * kRcTileW - R, y0 = tile_y * kRcTileH - R;
    for (int t = (int)threadIdx.x; t < TW * TH; t += kRcTileW * kRcTileH) {
        const int ty = t / TW, qx = x0 + (t - ty * TW), qy = y0 + ty;
        float4 rec = make_float4(0.f, 0.f, 0.f, __builtin_nanf(""));
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
            const float4 Fq = fast[q];
            rec = make_float4(Fq.x, Fq.y, Fq.z, g[q].w);
        }
        tile[t] = rec;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & (kRcTileW - 1), ly = (int)threadIdx.x / kRcTileW;
    const int x = x0 + R + lx, y = y0 + R + ly;
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)W * (size_t)H, pix = (size_t)y * (size_t)W + (size_t)x;
    const float4 H0 = hist[pix], H1 = hist[plane + pix];
    const float nf = fast[pix].w;
    const float id = tile[(ly + R) * TW + lx + R].w;
    float4 o0 = H0, o1 = H1;
    if (id != -1.f && !(H1.z <= nf)) {                                // (a NaN length on either side: not a copy)
        float s1[3] = {0.f, 0.f, 0.f}, s2[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const float4 q = tile[(ly + R + dy) * TW + lx + R + dx];
                if ((dx == 0 && dy == 0) || q.w == id) {              // the pixel itself always counts (its id may be a NaN)
                    s1[0] = s1[0] + q.x; s1[1] = s1[1] + q.y; s1[2] = s1[2] + q.z;
                    s2[0] = s2[0] + q.x * q.x; s2[1] = s2[1] + q.y * q.y; s2[2] = s2[2] + q.z * q.z;
                    cnt = cnt + 1.f;
                }
            }
        }
        const float r1 = div_refine(cnt, __builtin_amdgcn_rcpf(cnt));   // cnt >= 1: the pixel itself
        const float h[3] = {H0.x, H0.y, H0.z};
        float c[3];
        bool moved = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float mu = div_by(s1[k], cnt, r1), e2 = div_by(s2[k], cnt, r1);
            if (!(div_in_range(s1[k]) && div_in_range(s2[k]))) { mu = s1[k] / cnt; e2 = s2[k] / cnt; }
            const float sg = rt_sqrtf(fmaxf(0.f, e2 - mu * mu));
            const float lo = mu - k_clamp * sg, hi = mu + k_clamp * sg;
            c[k] = fminf(fmaxf(h[k], lo), hi);
            moved = moved || !(c[k] == h[k]);
        }
        if (moved) {
            const float4 Hc = make_float4(c[0], c[1], c[2], H0.w);
            const float d = lum709(Hc) - lum709(H0);
            const float m1 = H1.x + d;
            o0 = Hc;
            o1 = make_float4(m1, H1.y + (m1 * m1 - H1.x * H1.x), nf, H1.w);
        }
    }
    out[pix] = o0;
    out[plane + pix] = o1;
}

}  // namespace rtk

static int rc_check(rt_ctx *ctx, const void *hist, const void *fast, const void *aov, int width, int height, const rt_rectify_params *rp, const void *out) {
    if (!hist || !fast || !aov || !rp || !out) return fail(ctx, RT_ERR_INVALID, "history/fast/aov/params/out is NULL");
    if (rp->radius < 1 || rp->radius > 3) return fail(ctx, RT_ERR_INVALID, "radius %d outside [1,3]", rp->radius);
    if (!(rp->k_clamp >= 0.f)) return fail(ctx, RT_ERR_INVALID, "k_clamp %g is not >= 0", (double)rp->k_clamp);
    if (int rc = check_frame_size(ctx, width, height); rc != RT_OK) return rc;
    const size_t bytes = (size_t)width * height * sizeof(float4);
    // in place on the history exactly, or apart from it; never over the fast plane or plane 0
    if ((out != hist && overlaps(out, 2 * bytes, hist, 2 * bytes)) || overlaps(out, 2 * bytes, fast, bytes) || overlaps(out, 2 * bytes, aov, bytes))
        return fail(ctx, RT_ERR_INVALID, "the output overlaps an input (only out == history exactly is allowed)");
    return RT_OK;
}

extern "C" int rt_history_rectify_device(rt_ctx *ctx, const void *history_dev, const void *fast_dev, const void *aov_dev, int width, int height, const rt_rectify_params *rp,
                                         void *out_history_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = rc_check(ctx, history_dev, fast_dev, aov_dev, width, height, rp, out_history_dev);
    if (rc != RT_OK) return rc;
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    const size_t bytes = (size_t)width * height * sizeof(float4);
    note_between(ctx, q, {{history_dev, 2 * bytes}, {fast_dev, bytes}, {aov_dev, bytes}, {out_history_dev, 2 * bytes}});
    // one flat grid of tiles (below 2^28 pixels: at most 2^20 + 2^23 + 2^25 + 1 tiles; a tile index fits an int and the grid's x does not wrap)
    const int tiles_x = (width + rtk::kRcTileW - 1) / rtk::kRcTileW, tiles_y = (height + rtk::kRcTileH - 1) / rtk::kRcTileH;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y)), block(rtk::kRcTileW * rtk::kRcTileH);
    const float4 *h = static_cast<const float4 *>(history_dev), *f = static_cast<const float4 *>(fast_dev), *g = static_cast<const float4 *>(aov_dev);
    float4 *o = static_cast<float4 *>(out_history_dev);
    if (rp->radius == 1) hipLaunchKernelGGL(rtk::history_rectify_kernel<1>, grid, block, 0, q, h, f, g, o, width, height, tiles_x, rp->k_clamp);
    else if (rp->radius == 2) hipLaunchKernelGGL(rtk::history_rectify_kernel<2>, grid, block, 0, q, h, f, g, o, width, height, tiles_x, rp->k_clamp);
    else hipLaunchKernelGGL(rtk::history_rectify_kernel<3>, grid, block, 0, q, h, f, g, o, width, height, tiles_x, rp->k_clamp);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// the host form: the history, the fast plane, plane 0 of the guide, the result
extern "C" int rt_history_rectify(rt_ctx *ctx, const float *history_host, const float *fast_host, const float *aov_host, int width, int height, const rt_rectify_params *rp,
                                  float *out_history_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    const int rc = rc_check(ctx, history_host, fast_host, aov_host, width, height, rp, out_history_host);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)width * height * sizeof(float4);
    return staged(ctx, {{history_host, 2 * bytes}, {fast_host, bytes}, {aov_host, bytes}}, 4 * bytes, 2 * bytes, out_history_host,
                  [&](uint8_t *d) { return rt_history_rectify_device(ctx, d, d + 2 * bytes, d + 3 * bytes, width, height, rp, d + 4 * bytes, nullptr); });
}
