// rt_temporal.hip.h -- rt_temporal_accumulate[_device]: reproject the previous frame's history onto the current frame and blend (the temporal half of SVGF).
// Included at the end of rt_capi.hip, after rt_denoise.hip.h: the kernel measures luminance with its lum709, and its variance-guided instantiation reads what this writes.
//
// The caller owns every buffer: the current colour frame and planes (rt_render*, rt_render_aov*), the previous frame's planes 0 and 1, the previous history, the
// new history (two float4 planes: colour | rays, then luminance moments | history length | variance).  Per pixel with a hit: the hit point and normal are taken
// back to the previous frame by the object's rigid motion, the point is projected through the previous camera -- the inverse of pixel_dir / posed_dir of
// rt_shade.hip.h as they are written: the posed camera adds its position INTO the direction, and the inverse undoes that -- and the nearest previous pixel, then
// the other three of the 2 x 2 footprint, is accepted if it shows the same object, a normal and a tangent plane that agree.  Nearest, not bilinear: with nothing
// moving the history is exactly the running mean.  raytrace_hip.h states the arithmetic; it is the contract (binary32, one rounding per operation, no
// contraction; tests/temporal_model.py is its numpy twin).
// How it runs: one lane per pixel, a wave = 64 consecutive pixels of a row, dense float4 loads and stores; the previous frame's reads are a gather that is as
// coherent as the motion is; the motion table sits in the kernel-argument segment and a lane reads the record of its own object.  While a pixel's history is
// shorter than 4 frames its variance is the spatial one over the 5 x 5 current-frame neighbours of the same object: the divergent tail of the kernel, 25 direct
// loads through L1 -- every pixel on a first frame or after a cut, few in steady state.
#pragma once
#include "rt_div.h"

namespace rtk {

struct TpMotion { float r[9], t[3]; };                               // previous = r (row-major) * current + t
struct TpMotions { TpMotion m[RT_MAX_OBJECTS]; };
struct TpArgs {
    float o[3], bx[3], by[3], bz[3];                                  // the previous camera: position and basis (the identity for the fixed camera)
    float cx, cy, b;                                                  // o . bx, o . by, o . bz + z for the posed camera; 0, 0, z for the fixed one
    float half_w, half_h, max_hist, alpha_min, min_ndot, max_pd2;
    uint32_t mask;
    int have_prev, have_motion;
};

// FAST (rt_temporal_accumulate_fast*): the second, short history rides on the SAME accepted tap; its three arguments -- the previous fast plane, the new one, the
// length limit -- exist in that instantiation alone, so temporal_accumulate_kernel<false> has the arguments and the instructions the kernel always had.
struct TpFast { const float4 *__restrict__ pf; float4 *__restrict__ of; float fast_hist; };
template <bool FAST, class... Fast>
__global__ __launch_bounds__(256) void temporal_accumulate_kernel(const float4 *__restrict__ C, const float4 *__restrict__ g, const float4 *__restrict__ pg,
                                                                   const float4 *__restrict__ ph, float4 *__restrict__ out, int W, int H, const TpArgs a, const TpMotions mt,
                                                                   const Fast... fast) {
    static_assert(sizeof...(Fast) == (FAST ? 1 : 0), "the fast instantiation takes one TpFast");
    const size_t plane = (size_t)W * (size_t)H;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * W);
    const float4 Cp = C[i], Np = g[i];
    float4 o0 = Cp, o1 = make_float4(0.f, 0.f, 0.f, 0.f);             // a miss: a copy, no history, no variance
    [[maybe_unused]] float4 f0;
    if constexpr (FAST) f0 = make_float4(Cp.x, Cp.y, Cp.z, 0.f);      // a miss: the colour, no history
    if (Np.w != -1.f) {
        const float lp = lum709(Cp);
        float n = 1.f, cr = Cp.x, cg = Cp.y, cb = Cp.z, m1 = lp, m2 = lp * lp;
        if constexpr (FAST) f0.w = 1.f;
        const int id = (int)Np.w;
        if (a.have_prev && !((a.mask >> (id & 31)) & 1u)) {
            const float4 Pp = g[plane + i];
            float px = Pp.x, py = Pp.y, pz = Pp.z, nx = Np.x, ny = Np.y, nz = Np.z;
            if (a.have_motion) {
                const TpMotion &m = mt.m[id & (RT_MAX_OBJECTS - 1)];
                px = ((m.r[0] * Pp.x + m.r[1] * Pp.y) + m.r[2] * Pp.z) + m.t[0];
                py = ((m.r[3] * Pp.x + m.r[4] * Pp.y) + m.r[5] * Pp.z) + m.t[1];
                pz = ((m.r[6] * Pp.x + m.r[7] * Pp.y) + m.r[8] * Pp.z) + m.t[2];
                nx = (m.r[0] * Np.x + m.r[1] * Np.y) + m.r[2] * Np.z;
                ny = (m.r[3] * Np.x + m.r[4] * Np.y) + m.r[5] * Np.z;
                nz = (m.r[6] * Np.x + m.r[7] * Np.y) + m.r[8] * Np.z;
            }
            // the previous camera's image-plane coordinates of P': d = k^-1 (o + bz z + bx X + by Y)
            const float dx = px - a.o[0], dy = py - a.o[1], dz = pz - a.o[2];
            const float k = div_quot(a.b, (dx * a.bz[0] + dy * a.bz[1]) + dz * a.bz[2]);
            const float X = ((dx * a.bx[0] + dy * a.bx[1]) + dz * a.bx[2]) * k - a.cx;
            const float Y = ((dx * a.by[0] + dy * a.by[1]) + dz * a.by[2]) * k - a.cy;
            const float gx = X + a.half_w, gy = a.half_h - Y;         // pixel (px, row)'s centre is (px + 0.5, row + 0.5) here
            if (k > 0.f && gx >= -1.f && gx <= (float)W && gy >= -1.f && gy <= (float)H) {   // (false for a NaN, and for a point behind the camera)
                const float fx = floorf(gx), fy = floorf(gy);
                const int ix = (int)fx, iy = (int)fy;
                const int jx = gx - fx >= 0.5f ? ix + 1 : ix - 1, jy = gy - fy >= 0.5f ? iy + 1 : iy - 1;
#pragma unroll 1
                for (int t = 0; t < 4; ++t) {
                    const int qx = (t & 1) ? jx : ix, qy = (t & 2) ? jy : iy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                    const float4 Nq = pg[q];
                    if (Nq.w != Np.w) continue;
                    if (!((nx * Nq.x + ny * Nq.y) + nz * Nq.z >= a.min_ndot)) continue;
                    const float4 Pq = pg[plane + q];
                    const float e = (nx * (Pq.x - px) + ny * (Pq.y - py)) + nz * (Pq.z - pz);
                    if (!(e * e <= a.max_pd2)) continue;
                    const float4 H0 = ph[q], H1 = ph[plane + q];
                    n = fminf(H1.z + 1.f, a.max_hist);
                    const float al = fmaxf(div_quot(1.f, n), a.alpha_min);
                    cr = H0.x + al * (Cp.x - H0.x); cg = H0.y + al * (Cp.y - H0.y); cb = H0.z + al * (Cp.z - H0.z);
                    m1 = H1.x + al * (lp - H1.x);
                    m2 = H1.y + al * (lp * lp - H1.y);
                    if constexpr (FAST) {                             // the fast history of the same tap, its own length and weight
                        const TpFast &f = (fast, ...);
                        const float4 Fq = f.pf[q];
                        const float nf = fminf(Fq.w + 1.f, f.fast_hist);
                        const float af = fmaxf(div_quot(1.f, nf), a.alpha_min);
                        f0 = make_float4(Fq.x + af * (Cp.x - Fq.x), Fq.y + af * (Cp.y - Fq.y), Fq.z + af * (Cp.z - Fq.z), nf);
                    }
                    break;
                }
            }
        }
        float var = fmaxf(0.f, m2 - m1 * m1);
        if (n < 4.f) {                                                // too short a history: the spatial estimate over the 5 x 5 neighbours of the same object
            float s1 = 0.f, s2 = 0.f, cnt = 0.f;
            for (int dy = -2; dy <= 2; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= H) continue;
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= W) continue;
                    const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                    if (g[q].w != Np.w) continue;
                    const float l = lum709(C[q]);
                    s1 = s1 + l; s2 = s2 + l * l; cnt = cnt + 1.f;
                }
            }
            const float r1 = div_refine(cnt, __builtin_amdgcn_rcpf(cnt));   // cnt >= 1: the pixel itself
            float e1 = div_by(s1, cnt, r1), e2 = div_by(s2, cnt, r1);
            if (!(div_in_range(s1) && div_in_range(s2))) { e1 = s1 / cnt; e2 = s2 / cnt; }
            var = fmaxf(0.f, e2 - e1 * e1);
        }
        o0 = make_float4(cr, cg, cb, Cp.w);
        o1 = make_float4(m1, m2, n, var);
    }
    out[i] = o0;
    out[plane + i] = o1;
    if constexpr (FAST) (fast, ...).of[i] = f0;
}

}  // namespace rtk

// everything but aliasing, which the two forms test on their own pointers
static int tp_check(rt_ctx *ctx, const void *color, const void *aov, const void *prev_aov, const void *prev_hist, int width, int height, const rt_temporal_params *tp,
                    const rt_reproject *rp, const void *out) {
    if (!color || !aov || !tp || !out) return fail(ctx, RT_ERR_INVALID, "color/aov/params/out is NULL");
    if ((prev_aov == nullptr) != (prev_hist == nullptr)) return fail(ctx, RT_ERR_INVALID, "the previous planes and the previous history come together or not at all");
    if (prev_aov && !rp) return fail(ctx, RT_ERR_INVALID, "a previous frame needs a reprojection record");
    if (int rc = check_frame_size(ctx, width, height); rc != RT_OK) return rc;
    if (tp->max_history < 1) return fail(ctx, RT_ERR_INVALID, "max_history %d < 1", tp->max_history);
    return RT_OK;
}
static bool tp_aliased(const void *color, const void *aov, const void *prev_aov, const void *prev_hist, size_t bytes, const void *out) {
    return overlaps(out, 2 * bytes, color, bytes) || overlaps(out, 2 * bytes, aov, 2 * bytes) ||
           (prev_aov && (overlaps(out, 2 * bytes, prev_aov, 2 * bytes) || overlaps(out, 2 * bytes, prev_hist, 2 * bytes)));   // (tp_check: both or neither)
}

// the kernels' arguments from the parameters and the reprojection record
static void tp_args(int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, bool have_prev, rtk::TpArgs &a, rtk::TpMotions &mt) {
    a.bx[0] = a.by[1] = a.bz[2] = 1.f;
    a.half_w = (float)width / 2; a.half_h = (float)height / 2;
    a.max_hist = (float)tp->max_history; a.alpha_min = tp->alpha_min; a.min_ndot = tp->min_normal_dot; a.max_pd2 = tp->max_plane_dist * tp->max_plane_dist;
    a.have_prev = have_prev;
    if (a.have_prev) {
        a.mask = rp->no_history_mask;
        if (rp->posed) {                                              // make_frame's posed camera
            for (int c = 0; c < 3; ++c) a.o[c] = rp->pose.position[c];
            camera_basis(rp->pose.yaw, rp->pose.pitch, a.bx, a.by, a.bz);
            const float z = -(float)width / (2 * (float)std::tan((double)(rp->pose.fov / 2)));
            a.cx = (a.o[0] * a.bx[0] + a.o[1] * a.bx[1]) + a.o[2] * a.bx[2];
            a.cy = (a.o[0] * a.by[0] + a.o[1] * a.by[1]) + a.o[2] * a.by[2];
            a.b = ((a.o[0] * a.bz[0] + a.o[1] * a.bz[1]) + a.o[2] * a.bz[2]) + z;
        } else {
            for (int c = 0; c < 3; ++c) a.o[c] = rp->camera.position[c];
            a.b = -(float)width / (2 * (float)std::tan((double)(rp->camera.fov / 2)));
        }
        if (rp->motion) {
            a.have_motion = 1;
            for (int k = 0; k < RT_MAX_OBJECTS; ++k) {
                for (int c = 0; c < 9; ++c) mt.m[k].r[c] = rp->motion[k].rotation[c];
                for (int c = 0; c < 3; ++c) mt.m[k].t[c] = rp->motion[k].translation[c];
            }
        }
    }
}

extern "C" int rt_temporal_accumulate_device(rt_ctx *ctx, const void *color_dev, const void *aov_dev, const void *prev_aov_dev, const void *prev_history_dev, int width, int height,
                                             const rt_temporal_params *tp, const rt_reproject *rp, void *out_history_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = tp_check(ctx, color_dev, aov_dev, prev_aov_dev, prev_history_dev, width, height, tp, rp, out_history_dev);
    if (rc != RT_OK) return rc;
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    if (tp_aliased(color_dev, aov_dev, prev_aov_dev, prev_history_dev, bytes, out_history_dev)) return fail(ctx, RT_ERR_INVALID, "the output overlaps an input");
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    rtk::TpArgs a{};
    rtk::TpMotions mt{};
    tp_args(width, height, tp, rp, prev_aov_dev != nullptr, a, mt);
    note_between(ctx, q, {{color_dev, bytes}, {out_history_dev, 2 * bytes}});   // a pipelined frame must not overtake this read of a frame / write of a history
    hipLaunchKernelGGL(rtk::temporal_accumulate_kernel<false>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, q, static_cast<const float4 *>(color_dev), static_cast<const float4 *>(aov_dev),
                       static_cast<const float4 *>(prev_aov_dev), static_cast<const float4 *>(prev_history_dev), static_cast<float4 *>(out_history_dev), width, height, a, mt);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

extern "C" int rt_temporal_accumulate(rt_ctx *ctx, const float *color_host, const float *aov_host, const float *prev_aov_host, const float *prev_history_host, int width, int height,
                                      const rt_temporal_params *tp, const rt_reproject *rp, float *out_history_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    int rc = tp_check(ctx, color_host, aov_host, prev_aov_host, prev_history_host, width, height, tp, rp, out_history_host);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)width * height * sizeof(float4);
    if (tp_aliased(color_host, aov_host, prev_aov_host, prev_history_host, bytes, out_history_host)) return fail(ctx, RT_ERR_INVALID, "the output overlaps an input");
    // colour, planes 0 and 1, the previous planes 0 and 1, the previous history (room kept on a first frame), the new history
    const float *pa = prev_aov_host, *ph = prev_history_host;
    return staged(ctx, {{color_host, bytes}, {aov_host, 2 * bytes}, {pa, 2 * bytes}, {ph, 2 * bytes}}, 7 * bytes, 2 * bytes, out_history_host, [&](uint8_t *d) {
        return rt_temporal_accumulate_device(ctx, d, d + bytes, pa ? d + 3 * bytes : nullptr, pa ? d + 5 * bytes : nullptr, width, height, tp, rp, d + 7 * bytes, nullptr);
    });
}

// ---- rt_temporal_accumulate_fast[_device]: the same call with a second, short history beside the long one (raytrace_hip.h; what rt_history_rectify clamps to) ----
// what the fast form checks on top of tp_check, and tp_aliased extended to the two new buffers: no output over an input, nor over the other output
static int tpf_check(rt_ctx *ctx, const void *color, const void *aov, const void *prev_aov, const void *prev_hist, const void *prev_fast, int width, int height,
                     const rt_temporal_params *tp, const rt_reproject *rp, int fast_history, const void *out, const void *out_fast) {
    if (!out_fast) return fail(ctx, RT_ERR_INVALID, "out_fast is NULL");
    if (int rc = tp_check(ctx, color, aov, prev_aov, prev_hist, width, height, tp, rp, out); rc != RT_OK) return rc;
    if ((prev_fast == nullptr) != (prev_hist == nullptr)) return fail(ctx, RT_ERR_INVALID, "the previous fast plane comes exactly when the previous history does");
    if (fast_history < 1) return fail(ctx, RT_ERR_INVALID, "fast_history %d < 1", fast_history);
    const size_t bytes = (size_t)width * height * sizeof(float4);
    if (tp_aliased(color, aov, prev_aov, prev_hist, bytes, out) || (prev_fast && overlaps(out, 2 * bytes, prev_fast, bytes)) || overlaps(out, 2 * bytes, out_fast, bytes) ||
        overlaps(out_fast, bytes, color, bytes) || overlaps(out_fast, bytes, aov, 2 * bytes) ||
        (prev_aov && (overlaps(out_fast, bytes, prev_aov, 2 * bytes) || overlaps(out_fast, bytes, prev_hist, 2 * bytes) || overlaps(out_fast, bytes, prev_fast, bytes))))
        return fail(ctx, RT_ERR_INVALID, "an output overlaps an input or the other output");
    return RT_OK;
}

extern "C" int rt_temporal_accumulate_fast_device(rt_ctx *ctx, const void *color_dev, const void *aov_dev, const void *prev_aov_dev, const void *prev_history_dev,
                                                  const void *prev_fast_dev, int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, int fast_history,
                                                  void *out_history_dev, void *out_fast_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = tpf_check(ctx, color_dev, aov_dev, prev_aov_dev, prev_history_dev, prev_fast_dev, width, height, tp, rp, fast_history, out_history_dev, out_fast_dev);
    if (rc != RT_OK) return rc;
    const size_t npix = (size_t)width * height, bytes = npix * sizeof(float4);
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    rtk::TpArgs a{};
    rtk::TpMotions mt{};
    tp_args(width, height, tp, rp, prev_aov_dev != nullptr, a, mt);
    note_between(ctx, q, {{color_dev, bytes}, {out_history_dev, 2 * bytes}, {out_fast_dev, bytes}});
    hipLaunchKernelGGL((rtk::temporal_accumulate_kernel<true, rtk::TpFast>), dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, q, static_cast<const float4 *>(color_dev),
                       static_cast<const float4 *>(aov_dev), static_cast<const float4 *>(prev_aov_dev), static_cast<const float4 *>(prev_history_dev),
                       static_cast<float4 *>(out_history_dev), width, height, a, mt, rtk::TpFast{static_cast<const float4 *>(prev_fast_dev), static_cast<float4 *>(out_fast_dev), (float)fast_history});
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

extern "C" int rt_temporal_accumulate_fast(rt_ctx *ctx, const float *color_host, const float *aov_host, const float *prev_aov_host, const float *prev_history_host,
                                           const float *prev_fast_host, int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, int fast_history,
                                           float *out_history_host, float *out_fast_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    int rc = tpf_check(ctx, color_host, aov_host, prev_aov_host, prev_history_host, prev_fast_host, width, height, tp, rp, fast_history, out_history_host, out_fast_host);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)width * height * sizeof(float4);
    // rt_temporal_accumulate's seven planes, the previous fast plane (room kept on a first frame), the new fast plane, the new history
    const float *pa = prev_aov_host, *ph = prev_history_host, *pf = prev_fast_host;
    return staged(ctx, {{color_host, bytes}, {aov_host, 2 * bytes}, {pa, 2 * bytes}, {ph, 2 * bytes}, {pf, bytes}}, 9 * bytes, 2 * bytes, out_history_host, [&](uint8_t *d) {
        const int r = rt_temporal_accumulate_fast_device(ctx, d, d + bytes, pa ? d + 3 * bytes : nullptr, pa ? d + 5 * bytes : nullptr, pa ? d + 7 * bytes : nullptr, width, height,
                                                         tp, rp, fast_history, d + 9 * bytes, d + 8 * bytes, nullptr);
        if (r != RT_OK) return r;
        RT_HIP(ctx, hipMemcpyAsync(out_fast_host, d + 8 * bytes, bytes, hipMemcpyDeviceToHost, own_stream(ctx)));   // (staged waits for the stream)
        return (int)RT_OK;
    });
}
