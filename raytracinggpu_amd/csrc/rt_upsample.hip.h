// rt_upsample.hip.h -- rt_upsample[_device]: a frame (or a history) traced at 1 / f of the resolution, rebuilt at full resolution under the guidance of the
// full-resolution planes of rt_render_aov*.  Included at the end of rt_capi.hip (same translation unit: the host half uses rt_host_post.hip.h).
//
// Per full-resolution pixel: the 2 x 2 bilinear footprint in the low-resolution image, every tap weighted by how well its first hit agrees with the pixel's own --
// same object, normal, tangent plane (rt_denoise's terms) -- and plain bilinear where no tap survives (raytrace_hip.h states the formula; it is the contract:
// binary32, one rounding per operation, taps in row-major order, tests/upsample_model.py is its numpy twin).
// How it runs: one lane per full-resolution pixel, a workgroup a tile of kUpTileW x kUpTileH of them, so that its taps are a rectangle of at most
// (kUpTileW / f + 2) x (kUpTileH / f + 2) low-resolution pixels.  The taps are LEFT TO THE CACHES, not staged in LDS: a lane's (2 + NP) * 4 records are loaded from
// coordinates clamped into the image, unconditionally and all at once (no load waits for a test), and a wave's 64 lanes ask for 32 / f + 1 records a row -- a few
// lines of L1 each.  What decides is bytes: 32 + 16 NP bytes per pixel of planes read and frame written against (32 + 16 NP) / f^2 of low-resolution data, which the
// f^2 .. (f + 1)^2 lanes that share a record fetch from HBM once (DESIGN.md section 5.11 has the times beside that floor).  No LDS, no barrier.
// f is a kernel argument, not a template parameter: it enters the tap coordinates alone, whose quotient by f is rt_div.h's shared sequence either way (its range,
// [2^-60, 2^60], always holds for x + 0.5 and f).  Instantiated on f the kernel has 331 vector instructions against 348 at f = 2 and 506 against 503 at f = 3, the
// same registers, and there would be three times as many kernels.
#pragma once
#include "rt_div.h"

namespace rtk {

constexpr int kUpTileW = 32, kUpTileH = 8;            // 256 lanes; a wave = rows 2 w, 2 w + 1 of the tile

struct UpParams { int f; float k_normal, k_position; };

// the tap coordinate of full-resolution coordinate x: g = (x + 0.5) / f - 0.5 (correctly rounded: rf = div_refine(f, rcp(f))), i = floor(g), fr = g - floor(g)
__device__ __forceinline__ void up_coord(int x, float ff, float rf, int &i, float &fr) {
    const float g = div_by((float)x + 0.5f, ff, rf) - 0.5f;
    const float fl = floorf(g);
    i = (int)fl;
    fr = g - fl;
}

// low: NP planes of w * h float4; lg: the low-resolution planes (0 and 1 are read); g: the full-resolution planes (0 and 1 are read); out: NP planes of W * H float4
template <int NP>
__global__ __launch_bounds__(kUpTileW * kUpTileH) void upsample_kernel(const float4 *__restrict__ low, const float4 *__restrict__ lg, const float4 *__restrict__ g,
                                                                        float4 *__restrict__ out, int W, int H, int tiles_x, const UpParams k) {
    const int tile_y = (int)blockIdx.x / tiles_x, tile_x = (int)blockIdx.x - tile_y * tiles_x;
    const int x = tile_x * kUpTileW + ((int)threadIdx.x & (kUpTileW - 1)), y = tile_y * kUpTileH + (int)threadIdx.x / kUpTileW;
    if (x >= W || y >= H) return;
    const int w = W / k.f, h = H / k.f;
    const size_t plane = (size_t)W * (size_t)H, lplane = (size_t)w * (size_t)h, pix = (size_t)y * (size_t)W + (size_t)x;
    const float ff = (float)k.f, rf = div_refine(ff, __builtin_amdgcn_rcpf(ff));
    int ix, iy;
    float fx, fy;
    up_coord(x, ff, rf, ix, fx);
    up_coord(y, ff, rf, iy, fy);
    // the four taps: all their records at once, from coordinates clamped into the image (a tap outside is never used)
    float4 Nq[4], Pq[4], Lq[NP][4];
    bool inside[4];
    float b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int qx = ix + (t & 1), qy = iy + (t >> 1);
        inside[t] = qx >= 0 && qx < w && qy >= 0 && qy < h;
        const size_t q = (size_t)min(max(qy, 0), h - 1) * (size_t)w + (size_t)min(max(qx, 0), w - 1);
        Nq[t] = lg[q];
        Pq[t] = lg[lplane + q];
#pragma unroll
        for (int p = 0; p < NP; ++p) Lq[p][t] = low[(size_t)p * lplane + q];
        b[t] = ((t & 1) ? fx : 1.f - fx) * ((t >> 1) ? fy : 1.f - fy);
    }
    const float4 Np = g[pix], Pp = g[plane + pix];
    float S[NP][4], Wt = 0.f, w0 = 0.f;
    bool first = true;
#pragma unroll
    for (int p = 0; p < NP; ++p) S[p][0] = S[p][1] = S[p][2] = S[p][3] = 0.f;
    auto take = [&](int t, float wt) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            S[p][0] = S[p][0] + wt * Lq[p][t].x; S[p][1] = S[p][1] + wt * Lq[p][t].y; S[p][2] = S[p][2] + wt * Lq[p][t].z; S[p][3] = S[p][3] + wt * Lq[p][t].w;
        }
        Wt = Wt + wt;
        if (first) w0 = Lq[0][t].w;
        first = false;
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!inside[t] || Nq[t].w != Np.w) continue;                  // outside, or another object (a miss matches a miss; false for a NaN id)
        float wt = b[t] * dn_term(dn_sqdiff(Np, Nq[t]), k.k_normal);
        if (k.k_position != 0.f) {
            const float e = (Np.x * (Pq[t].x - Pp.x) + Np.y * (Pq[t].y - Pp.y)) + Np.z * (Pq[t].z - Pp.z);
            wt = wt * fmaxf(0.f, 1.f - (e * e) * k.k_position);
        }                                                             // (else: times exactly 1)
        if (wt > 0.f) take(t, wt);                                    // (false for a NaN weight: a NaN guide makes a tap weigh nothing)
    }
    if (Wt == 0.f) {                                                  // no tap counted: plain bilinear over the taps inside the image, whatever the guides say
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (inside[t]) take(t, b[t]);
    }
    // S / W, correctly rounded: up to eight numerators over one denominator (rt_div.h), the literal quotient outside the shared sequence's range
    const float r1 = div_refine(Wt, __builtin_amdgcn_rcpf(Wt));
    float o[NP][4];
    bool fast = div_in_range(Wt);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (p == 0 && c == 3) continue;
            o[p][c] = div_by(S[p][c], Wt, r1);
            fast = fast && div_in_range(S[p][c]);
        }
    }
    if (__builtin_expect(__ballot(!fast) != 0ull, 0)) {
        if (!fast) {                                                  // (a zero or denormal sum, a weight below 2^-60)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (!(p == 0 && c == 3)) o[p][c] = S[p][c] / Wt;
            }
        }
    }
    o[0][3] = w0;                                                     // the first counted tap's: a ray count stays exact
#pragma unroll
    for (int p = 0; p < NP; ++p) out[(size_t)p * plane + pix] = make_float4(o[p][0], o[p][1], o[p][2], o[p][3]);
}

}  // namespace rtk

// the sizes of a checked call
struct UpSizes { size_t low, low_aov, aov, out; };                    // bytes of each of the four ranges
static UpSizes up_sizes(int width, int height, const rt_upsample_params *up) {
    const size_t full = (size_t)width * height * sizeof(float4), low = full / ((size_t)up->factor * up->factor);
    return {up->n_planes * low, 3 * low, 3 * full, up->n_planes * full};
}

static int up_check(rt_ctx *ctx, const void *low, const void *low_aov, const void *aov, int width, int height, const rt_upsample_params *up, const void *out) {
    if (!low || !low_aov || !aov || !up || !out) return fail(ctx, RT_ERR_INVALID, "low/low_aov/aov/params/out is NULL");
    if (up->factor < 2 || up->factor > 4) return fail(ctx, RT_ERR_INVALID, "factor %d outside [2,4]", up->factor);
    if (up->n_planes < 1 || up->n_planes > 2) return fail(ctx, RT_ERR_INVALID, "n_planes %d outside [1,2]", up->n_planes);
    if (int rc = check_frame_size(ctx, width, height); rc != RT_OK) return rc;
    if (width % up->factor || height % up->factor) return fail(ctx, RT_ERR_INVALID, "%d x %d is no multiple of factor %d", width, height, up->factor);
    const UpSizes s = up_sizes(width, height, up);
    if (overlaps(out, s.out, low, s.low) || overlaps(out, s.out, low_aov, s.low_aov) || overlaps(out, s.out, aov, s.aov))
        return fail(ctx, RT_ERR_INVALID, "the output overlaps an input");
    return RT_OK;
}

extern "C" int rt_upsample_device(rt_ctx *ctx, const void *low_dev, const void *low_aov_dev, const void *aov_dev, int width, int height, const rt_upsample_params *up,
                                  void *out_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = up_check(ctx, low_dev, low_aov_dev, aov_dev, width, height, up, out_dev);
    if (rc != RT_OK) return rc;
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    const UpSizes s = up_sizes(width, height, up);
    // a pipelined frame must not overtake these reads of frames and planes / this write of an image
    note_between(ctx, q, {{low_dev, s.low}, {low_aov_dev, s.low_aov}, {aov_dev, s.aov}, {out_dev, s.out}});
    // (below 2^28 pixels: at most 2^20 + 2^25 tiles, and a tile index fits an int)
    const int tiles_x = (width + rtk::kUpTileW - 1) / rtk::kUpTileW, tiles_y = (height + rtk::kUpTileH - 1) / rtk::kUpTileH;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y)), block(rtk::kUpTileW * rtk::kUpTileH);
    const rtk::UpParams k{up->factor, up->k_normal, up->k_position};
    const float4 *low = static_cast<const float4 *>(low_dev), *lg = static_cast<const float4 *>(low_aov_dev), *g = static_cast<const float4 *>(aov_dev);
    if (up->n_planes == 1) hipLaunchKernelGGL(rtk::upsample_kernel<1>, grid, block, 0, q, low, lg, g, static_cast<float4 *>(out_dev), width, height, tiles_x, k);
    else hipLaunchKernelGGL(rtk::upsample_kernel<2>, grid, block, 0, q, low, lg, g, static_cast<float4 *>(out_dev), width, height, tiles_x, k);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// the host form: the low-resolution planes of values, then planes 0 and 1 of either guide (plane 2 is not read: it keeps its room and is not copied), the result
extern "C" int rt_upsample(rt_ctx *ctx, const float *low_host, const float *low_aov_host, const float *aov_host, int width, int height, const rt_upsample_params *up,
                           float *out_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    const int rc = up_check(ctx, low_host, low_aov_host, aov_host, width, height, up, out_host);
    if (rc != RT_OK) return rc;
    const UpSizes s = up_sizes(width, height, up);
    const size_t lp = s.low_aov / 3, fp = s.aov / 3;
    return staged(ctx, {{low_host, s.low}, {low_aov_host, 2 * lp}, {nullptr, lp}, {aov_host, 2 * fp}, {nullptr, fp}}, s.low + s.low_aov + s.aov, s.out, out_host,
                  [&](uint8_t *d) { return rt_upsample_device(ctx, d, d + s.low, d + s.low + s.low_aov, width, height, up, d + s.low + s.low_aov + s.aov, nullptr); });
}
