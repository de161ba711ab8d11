// rt_kat.hip.h -- known-answer entry points: the DEVICE primitives of the render path fed with explicit inputs.
// Included by rt_capi.hip (same library: the functions called here are the ones the render kernels inline).
//
// The reference's own Sphere::intersect (cpu_launcher.cpp:512-527), BoundingBox::intersect (cpu:146-157),
// moller_trumbore (cpu:226-236) and TriangleMesh::intersect (cpu:238-313) produced tests/golden/kat.npz; these
// kernels run the same inputs through sphere_test, slab / slab_filtered / qbox_filter, qtri_test and the two mesh
// walks, one lane per row, and report how often the error-bounded filters decided and how often the literal
// divisions ran -- so that the rare branches (zero direction components, 0/0 slabs, rays through edges and
// vertices, |det| <= 1e-30) are shown to be reached on the device, not only through images.
#pragma once
#include "rt_travq.hip.h"

namespace rtk {

__device__ __forceinline__ void kat_count(unsigned long long *cnt, bool decided, bool active) {
    const unsigned long long md = __ballot(active && decided), ml = __ballot(active && !decided);
    if ((threadIdx.x & 63) == 0) {
        if (md) atomicAdd(&cnt[0], (unsigned long long)__popcll(md));
        if (ml) atomicAdd(&cnt[1], (unsigned long long)__popcll(ml));
    }
}

// in: C[3] R O[3] u[3]; out: hit t N[3]  (N = normalize(O + t u - C), cpu:524-525)
// rt_sqrtf (rt_kernels.hip.h): one value per lane; waves hold plain and special arguments mixed, so both of its routes run
__global__ __launch_bounds__(256) void kat_sqrt_kernel(const float *__restrict__ in, int n, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rt_sqrtf(in[i]);
}

__global__ __launch_bounds__(256) void kat_sphere_kernel(const float *__restrict__ in, int n, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = in + 10 * (size_t)i;
    Sphere s{};
    s.cx = r[0]; s.cy = r[1]; s.cz = r[2]; s.R = r[3]; s.R2 = r[3] * r[3];
    const f3 O = mk(r[4], r[5], r[6]), u = mk(r[7], r[8], r[9]);
    float t = 0.f;
    const bool hit = sphere_test(s, O, u, t);
    f3 N = mk(0, 0, 0);
    if (hit) N = normalize(O + t * u - mk(s.cx, s.cy, s.cz));
    float *o = out + 5 * (size_t)i;
    o[0] = hit ? 1.f : 0.f; o[1] = t; o[2] = N.x; o[3] = N.y; o[4] = N.z;
}

// in: mn[3] mx[3] O[3] u[3]; out: hit.  route 0: literal slab; 1: slab_filtered (RayInv: root-box pre-test, stackless
// walks); 2: qbox_filter with the per-ray table entry of wf_path, literal slab when undecided; 3: wf_travq's centre / half-extent
// filter (cbox_filter: the box as rt_scene_upload stores it, the per-ray constants of the refill), literal slab when undecided
__global__ __launch_bounds__(256) void kat_box_kernel(const float *__restrict__ in, int n, int route, float *__restrict__ out, unsigned long long *cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    bool hit = false, decided = false;
    if (active) {
        const float *r = in + 12 * (size_t)i;
        const float4 lo = make_float4(r[0], r[1], r[2], 0), hi = make_float4(r[3], r[4], r[5], 0);
        const f3 O = mk(r[6], r[7], r[8]), u = mk(r[9], r[10], r[11]);
        if (route == 0) {
            hit = slab(lo, hi, O, u);
        } else if (route == 1) {
            hit = slab_filtered(lo, hi, O, u, ray_inv(u), decided);
        } else if (route == 2) {
            const RayBox rb = ray_box(O, u);
            const float4 A = make_float4(rb.rx, rb.ry, rb.rz, rb.safe ? rb.c0 : __builtin_inff());
            const float4 C = make_float4(O.x, O.y, O.z, u.x);
            decided = qbox_filter(lo, hi, A, C, hit);
            if (!decided) hit = slab(lo, hi, O, u);
        } else {
            // the scene-wide quantities of install_scene, for this one box: magnitudes, and whether the fast filter may run at all
            const float v[6] = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z};
            bool fast = true;
            for (int a = 0; a < 3; ++a) fast = fast && v[a] <= v[a + 3] && fabsf(v[a]) < 1e8f && fabsf(v[a + 3]) < 1e8f;
            const f3 bm = mk(fmaxf(fabsf(lo.x), fabsf(hi.x)), fmaxf(fabsf(lo.y), fabsf(hi.y)), fmaxf(fabsf(lo.z), fabsf(hi.z)));
            const RayBoxC rb = ray_box_c(O, u, bm, fast);
            const float4 n0 = make_float4(box_centre(lo.x, hi.x), box_centre(lo.y, hi.y), box_centre(lo.z, hi.z), 0.f);
            const float4 n1 = make_float4(box_half(lo.x, hi.x), box_half(lo.y, hi.y), box_half(lo.z, hi.z), 0.f);
            bool miss;
            cbox_filter(n0, n1, make_float4(rb.rx, rb.ry, rb.rz, rb.c0), make_float4(rb.ox, rb.oy, rb.oz, 0.f), hit, miss);
            decided = hit || miss;
            if (!decided) hit = slab(lo, hi, O, u);
        }
        out[i] = hit ? 1.f : 0.f;
    }
    kat_count(cnt, decided, active);
}

// in: A[3] B[3] C[3] O[3] u[3]; out: hit t N[3]  (N = e1 x e2, unnormalised, always written: cpu:229)
__global__ __launch_bounds__(256) void kat_tri_kernel(const float *__restrict__ in, int n, float *__restrict__ out, unsigned long long *cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    int how = 0;
    if (active) {
        const float *r = in + 15 * (size_t)i;
        const f3 A = mk(r[0], r[1], r[2]), B = mk(r[3], r[4], r[5]), C = mk(r[6], r[7], r[8]);
        const f3 O = mk(r[9], r[10], r[11]), u = mk(r[12], r[13], r[14]);
        const f3 e1 = B - A, e2 = C - A, N = cross(e1, e2);               // the triangle record of rt_scene_upload / retri_kernel
        const float4 q0 = make_float4(A.x, A.y, A.z, e1.x), q1 = make_float4(e1.y, e1.z, e2.x, e2.y), q2 = make_float4(e2.z, N.x, N.y, N.z);
        float t = 0.f;
        // moller_trumbore alone accepts t > 0 (cpu:235); the leaf loop's t > 1e-4 and t < t_min belong to the traversal
        const bool hit = qtri_test(q0, q1, q2, O, u, 0.f, t, how);
        float *o = out + 5 * (size_t)i;
        o[0] = hit ? 1.f : 0.f; o[1] = t; o[2] = N.x; o[3] = N.y; o[4] = N.z;
    }
    kat_count(cnt, (how & 3) != 2, active);
}

// in: O[3] u[3]; out: hit t N[3] (N normalised, cpu:308) against the uploaded mesh.  route 0: the work-stack kernels'
// primitives (root box by slab_filtered as wf_emit_ray does, then qbox_filter / slab and qtri_test over the pre-order
// skip-pointer array, nearest = min over (bits(t) << 32 | visit rank)); route 1: mesh_intersect (stackless walk of the
// lock-step and persistent kernels).  cnt[0..1]: box tests decided / literal, cnt[2..3]: triangle tests decided / literal.
__global__ __launch_bounds__(256) void kat_mesh_kernel(const Scene sc, const float *__restrict__ in, int n, float tri_tmin, int route,
                                                       float *__restrict__ out, unsigned long long *cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    unsigned int bd = 0, bl = 0, td = 0, tl = 0;
    if (active) {
        const float *r = in + 6 * (size_t)i;
        const f3 O = mk(r[0], r[1], r[2]), u = mk(r[3], r[4], r[5]);
        bool hit = false; float t = 1e9f; f3 N = mk(0, 0, 0);
        if (route == 1) {
            Work wk;
            f3 Nr;
            int tri_; hit = mesh_intersect<false>(sc, O, u, tri_tmin, t, Nr, tri_, wk);
            if (hit) N = normalize(Nr);
        } else if (sc.n_nodes > 0) {
            bool dec;
            const bool root = slab_filtered(sc.root_lo, sc.root_hi, O, u, ray_inv(u), dec);
            if (dec) bd++; else bl++;
            unsigned long long best = WF_NOHIT;
            if (root) {
                const RayBox rb = ray_box(O, u);
                const float4 A = make_float4(rb.rx, rb.ry, rb.rz, rb.safe ? rb.c0 : __builtin_inff());
                const float4 C = make_float4(O.x, O.y, O.z, u.x);
                const int root_hiw = __float_as_int(sc.root_hi.w);
                auto leaf = [&](int first, int end) {
                    for (int k = first; k < end; ++k) {
                        const float4 *tp = sc.tri + 3 * (size_t)k;
                        float tt; int how;
                        if (qtri_test(tp[0], tp[1], tp[2], O, u, tri_tmin, tt, how)) {
                            const unsigned long long key = (unsigned long long)__float_as_uint(tt) << 32 | (unsigned int)k;
                            if (key < best) best = key;
                        }
                        if ((how & 3) == 2) tl++; else td++;
                    }
                };
                if (root_hiw >= 0) {
                    leaf(__float_as_int(sc.root_lo.w), root_hiw);
                } else {
                    for (int x = 1; x < sc.n_nodes;) {
                        const float4 lo = sc.nodes[2 * x], hi = sc.nodes[2 * x + 1];
                        const int hiw = __float_as_int(hi.w), low = __float_as_int(lo.w);
                        bool h;
                        if (qbox_filter(lo, hi, A, C, h)) bd++; else { h = slab(lo, hi, O, u); bl++; }
                        if (h && hiw >= 0) leaf(low, hiw);
                        x = (h || hiw >= 0) ? x + 1 : low;
                    }
                }
            }
            if (best != WF_NOHIT) {
                hit = true;
                t = __uint_as_float((unsigned int)(best >> 32));
                const float4 q2 = sc.tri[3 * (size_t)(unsigned int)best + 2];
                N = normalize(mk(q2.y, q2.z, q2.w));
            }
        }
        float *o = out + 5 * (size_t)i;
        o[0] = hit ? 1.f : 0.f; o[1] = t; o[2] = N.x; o[3] = N.y; o[4] = N.z;
    }
    const uint32_t s0 = wave_sum(bd), s1 = wave_sum(bl), s2 = wave_sum(td), s3 = wave_sum(tl);
    if ((threadIdx.x & 63) == 0) {
        if (s0) atomicAdd(&cnt[0], (unsigned long long)s0);
        if (s1) atomicAdd(&cnt[1], (unsigned long long)s1);
        if (s2) atomicAdd(&cnt[2], (unsigned long long)s2);
        if (s3) atomicAdd(&cnt[3], (unsigned long long)s3);
    }
}

// in: u[3]; out: E[3] = sky_radiance(u) of the map the context holds (the lookup of wf_advance's kFormSky forms, on explicit directions)
__global__ __launch_bounds__(256) void kat_sky_kernel(const WfSky sky, const float *__restrict__ in, int n, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 E = sky_radiance(sky, mk(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]));
    out[3 * (size_t)i] = E.x; out[3 * (size_t)i + 1] = E.y; out[3 * (size_t)i + 2] = E.z;
}

// in: hs, seg; out: the texel, the direction and g at mx = 1 of sky_draw / sky_weight (the draw a sky-sampling wf_advance form makes per diffuse segment)
template <bool FLAT>
__global__ __launch_bounds__(256) void kat_sky_sample_kernel(const WfSkyDist sd, const uint32_t *__restrict__ hs, const int *__restrict__ seg, int count, uint32_t *__restrict__ texel,
                                                             float *__restrict__ dir, float *__restrict__ g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const SkyDraw s = sky_draw<FLAT>(sd, hs[i], seg[i]);
    texel[i] = s.t;
    dir[3 * (size_t)i] = s.w.x; dir[3 * (size_t)i + 1] = s.w.y; dir[3 * (size_t)i + 2] = s.w.z;
    g[i] = sky_weight(sd, s.t, s.m, s.r, 1.f);
}

// in: hs, seg; out: the triangle (visit order) and the point of emit_draw (the draw of a shadow ray towards the emissive meshes)
__global__ __launch_bounds__(256) void kat_emit_sample_kernel(const WfEmit em, const float4 *__restrict__ tri_rec, const uint32_t *__restrict__ hs, const int *__restrict__ seg, int count,
                                                              uint32_t *__restrict__ tri, float *__restrict__ point) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const EmitDraw s = emit_draw(em, tri_rec, hs[i], seg[i]);
    tri[i] = s.t;
    point[3 * (size_t)i] = s.Q.x; point[3 * (size_t)i + 1] = s.Q.y; point[3 * (size_t)i + 2] = s.Q.z;
}

// in: 16 words per item -- n_in, n_out, the ray's index, eps, P, N, u as binary32, then hs and seg as 32-bit integers, one word of padding; out: 9 words per item -- R,
// the code (kFresnel*, an integer), the new O and u, the index after: fresnel_step (the step a wf_advance fresnel form takes at a flagged hit) on explicit items
__global__ __launch_bounds__(256) void kat_fresnel_kernel(const float *__restrict__ in, int count, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float *a = in + 16 * (size_t)i;
    Material m{};
    m.n_in = a[0]; m.n_out = a[1];
    f3 O = mk(0.f, 0.f, 0.f), u = mk(a[10], a[11], a[12]);
    const FresnelStep s = fresnel_step(m, a[2], a[3], mk(a[4], a[5], a[6]), mk(a[7], a[8], a[9]), O, u, __float_as_uint(a[13]), __float_as_int(a[14]));
    float *o = out + 9 * (size_t)i;
    o[0] = s.R; o[1] = __int_as_float(s.code);
    o[2] = O.x; o[3] = O.y; o[4] = O.z; o[5] = u.x; o[6] = u.y; o[7] = u.z;
    o[8] = s.r.refr_after;
}

// in: 16 words per item -- alpha, eps, P, N, u as binary32, then hs and seg as 32-bit integers, three words of padding; out: 12 words per item -- h, the code (kGloss*,
// an integer), the new O and u, two words of padding: gloss_step (the step a wf_advance gloss form takes at a rough mirror) on explicit items
__global__ __launch_bounds__(256) void kat_gloss_kernel(const float *__restrict__ in, int count, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float *a = in + 16 * (size_t)i;
    f3 O = mk(0.f, 0.f, 0.f), u = mk(a[8], a[9], a[10]);
    const GlossStep s = gloss_step(a[1], a[0], mk(a[2], a[3], a[4]), mk(a[5], a[6], a[7]), O, u, __float_as_uint(a[11]), __float_as_int(a[12]));
    float *o = out + 12 * (size_t)i;
    o[0] = s.h.x; o[1] = s.h.y; o[2] = s.h.z; o[3] = __int_as_float(s.code);
    o[4] = O.x; o[5] = O.y; o[6] = O.z; o[7] = u.x; o[8] = u.y; o[9] = u.z;
    o[10] = 0.f; o[11] = 0.f;
}

}  // namespace rtk

namespace {

// rows of `width` floats in, `owidth` floats out, up to 4 counters back
template <typename Launch>
int kat_run(rt_ctx *ctx, const float *in, int n, int width, float *out, int owidth, rt_kat_counts *counts, Launch launch) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, RT_ERR_INVALID, "bad KAT arguments");
    if (counts) *counts = rt_kat_counts{};
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    DevBuf din, dout, dcnt;
    int rc;
    if ((rc = upload(ctx, din, in, (size_t)n * width * sizeof(float))) != RT_OK || (rc = ensure(ctx, dout, (size_t)n * owidth * sizeof(float))) != RT_OK ||
        (rc = ensure(ctx, dcnt, 4 * sizeof(unsigned long long))) != RT_OK) return rc;
    hipError_t e = hipMemsetAsync(dcnt.p, 0, 4 * sizeof(unsigned long long), own_stream(ctx));
    if (e == hipSuccess) {
        launch(static_cast<const float *>(din.p), static_cast<float *>(dout.p), static_cast<unsigned long long *>(dcnt.p), dim3((unsigned)((n + 255) / 256)), dim3(256));
        e = hipGetLastError();
    }
    unsigned long long h[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, (size_t)n * owidth * sizeof(float), hipMemcpyDeviceToHost, own_stream(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(h, dcnt.p, sizeof(h), hipMemcpyDeviceToHost, own_stream(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(own_stream(ctx));
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "KAT launch: %s", hipGetErrorString(e));
    if (counts) { counts->n = (uint64_t)n; counts->box_decided = h[0]; counts->box_literal = h[1]; counts->tri_decided = h[2]; counts->tri_literal = h[3]; }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_kat_sqrt(rt_ctx *ctx, const float *in, int n, float *out) {
    return kat_run(ctx, in, n, 1, out, 1, nullptr, [&](const float *di, float *dres, unsigned long long *, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_sqrt_kernel, g, b, 0, own_stream(ctx), di, n, dres);
    });
}

int rt_kat_sphere(rt_ctx *ctx, const float *in, int n, float *out) {
    return kat_run(ctx, in, n, 10, out, 5, nullptr, [&](const float *di, float *dres, unsigned long long *, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_sphere_kernel, g, b, 0, own_stream(ctx), di, n, dres);
    });
}

int rt_kat_box(rt_ctx *ctx, const float *in, int n, int route, float *out, rt_kat_counts *counts) {
    if (route < 0 || route > 3) return fail(ctx, RT_ERR_INVALID, "route must be 0 (literal), 1 (slab_filtered), 2 (qbox_filter) or 3 (cbox_filter)");
    return kat_run(ctx, in, n, 12, out, 1, counts, [&](const float *di, float *dres, unsigned long long *dc, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_box_kernel, g, b, 0, own_stream(ctx), di, n, route, dres, dc);
    });
}

int rt_kat_triangle(rt_ctx *ctx, const float *in, int n, float *out, rt_kat_counts *counts) {
    const int rc = kat_run(ctx, in, n, 15, out, 5, counts, [&](const float *di, float *dres, unsigned long long *dc, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_tri_kernel, g, b, 0, own_stream(ctx), di, n, dres, dc);
    });
    if (rc == RT_OK && counts) { counts->tri_decided = counts->box_decided; counts->tri_literal = counts->box_literal; counts->box_decided = counts->box_literal = 0; }
    return rc;
}

int rt_kat_mesh(rt_ctx *ctx, const float *in, int n, float tri_tmin, int route, float *out, rt_kat_counts *counts) {
    if (ctx && !ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (route < 0 || route > 1) return fail(ctx, RT_ERR_INVALID, "route must be 0 (work-stack primitives) or 1 (stackless mesh_intersect)");
    return kat_run(ctx, in, n, 6, out, 5, counts, [&](const float *di, float *dres, unsigned long long *dc, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_mesh_kernel, g, b, 0, own_stream(ctx), ctx->scene, di, n, tri_tmin, route, dres, dc);
    });
}

// the Fresnel step on explicit items (raytrace_hip.h "fresnel"): needs a context, not a scene
int rt_kat_fresnel(rt_ctx *ctx, int count, const uint32_t *items, uint32_t *out) {
    return kat_run(ctx, reinterpret_cast<const float *>(items), count, 16, reinterpret_cast<float *>(out), 9, nullptr, [&](const float *di, float *dres, unsigned long long *, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_fresnel_kernel, g, b, 0, own_stream(ctx), di, count, dres);
    });
}

// the rough mirror's step on explicit items (raytrace_hip.h "roughness"): needs a context, not a scene
int rt_kat_gloss(rt_ctx *ctx, int count, const uint32_t *items, uint32_t *out) {
    return kat_run(ctx, reinterpret_cast<const float *>(items), count, 16, reinterpret_cast<float *>(out), 12, nullptr, [&](const float *di, float *dres, unsigned long long *, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_gloss_kernel, g, b, 0, own_stream(ctx), di, count, dres);
    });
}

int rt_kat_environment(rt_ctx *ctx, int n_dirs, const float *dirs, float *rgb_out) {
    if (ctx && !ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (ctx && ctx->env_n <= 0) return fail(ctx, RT_ERR_INVALID, "the scene has no environment (rt_scene_set_environment)");
    return kat_run(ctx, dirs, n_dirs, 3, rgb_out, 3, nullptr, [&](const float *di, float *dres, unsigned long long *, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::kat_sky_kernel, g, b, 0, own_stream(ctx), rtk::WfSky{static_cast<const float4 *>(ctx->env.p), ctx->env_n}, di, n_dirs, dres);
    });
}

// the sampling table as the device built it: c and prefix (n * n each, either may be NULL) and the total; an empty table is total 0 and zeros
int rt_kat_environment_table(rt_ctx *ctx, uint32_t *c_out, uint64_t *prefix_out, uint64_t *total) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (!total) return fail(ctx, RT_ERR_INVALID, "total is NULL");
    if (ctx->env_n <= 0 || !(ctx->env_share > 0.f)) return fail(ctx, RT_ERR_INVALID, "no table: the scene has no environment or the share is 0 (rt_scene_set_environment_sampling)");
    const size_t count = (size_t)ctx->env_n * (size_t)ctx->env_n;
    if (ctx->env_total == 0) {
        if (c_out) memset(c_out, 0, count * sizeof(uint32_t));
        if (prefix_out) memset(prefix_out, 0, count * sizeof(uint64_t));
        *total = 0;
        return RT_OK;
    }
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const rtk::WfSkyDist sd = sky_dist_of(ctx);
    if (c_out) RT_HIP(ctx, hipMemcpy(c_out, sd.c, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (prefix_out) RT_HIP(ctx, hipMemcpy(prefix_out, sd.prefix, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *total = ctx->env_total;
    return RT_OK;
}

int rt_kat_environment_sample(rt_ctx *ctx, int count, const uint32_t *hs, const int32_t *seg, uint32_t *texel_out, float *dir_out, float *g_out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (count < 0 || (count > 0 && (!hs || !seg || !texel_out || !dir_out || !g_out))) return fail(ctx, RT_ERR_INVALID, "bad KAT arguments");
    if (ctx->env_n <= 0 || ctx->env_total == 0) return fail(ctx, RT_ERR_INVALID, "no table to draw from: no environment, share 0 or a map that is zero throughout (rt_scene_set_environment_sampling)");
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    hipStream_t q = own_stream(ctx);
    DevBuf dhs, dseg, dout;                                            // out: the texel, three floats of direction and g per draw
    int rc;
    if ((rc = upload(ctx, dhs, hs, (size_t)count * 4)) != RT_OK || (rc = upload(ctx, dseg, seg, (size_t)count * 4)) != RT_OK || (rc = ensure(ctx, dout, (size_t)count * 20)) != RT_OK) return rc;
    uint32_t *dt = static_cast<uint32_t *>(dout.p);
    float *dd = reinterpret_cast<float *>(dt + count), *dg = dd + 3 * (size_t)count;
    const auto kernel = ctx->knobs.sky_search != 0 ? rtk::kat_sky_sample_kernel<false> : rtk::kat_sky_sample_kernel<true>;   // (RT_SKY_SEARCH=0: the flat search)
    hipLaunchKernelGGL(kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, q, sky_dist_of(ctx), static_cast<const uint32_t *>(dhs.p),
                       static_cast<const int *>(dseg.p), count, dt, dd, dg);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(texel_out, dt, (size_t)count * 4, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipMemcpyAsync(dir_out, dd, (size_t)count * 12, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipMemcpyAsync(g_out, dg, (size_t)count * 4, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "KAT launch: %s", hipGetErrorString(e));
    return RT_OK;
}

// the emitters' sampling table as the device built it: c and prefix (n_triangles each, either may be NULL: a first call with both NULL asks for the count) and the total;
// no emitter, or an empty table: total 0 and zeros
int rt_kat_emission_table(rt_ctx *ctx, uint32_t *c_out, uint64_t *prefix_out, uint64_t *total, int32_t *n_triangles) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    if (!total || !n_triangles) return fail(ctx, RT_ERR_INVALID, "total or n_triangles is NULL");
    if (int rc = emit_refresh(ctx); rc != RT_OK) return rc;
    const size_t count = (size_t)(ctx->scene.n_tris > 0 ? ctx->scene.n_tris : 0);
    if (ctx->emit_total == 0) {
        if (c_out) memset(c_out, 0, count * sizeof(uint32_t));
        if (prefix_out) memset(prefix_out, 0, count * sizeof(uint64_t));
    } else {
        RT_HIP(ctx, hipSetDevice(ctx->device));
        const rtk::WfEmit em = emit_dist_of(ctx);
        if (c_out) RT_HIP(ctx, hipMemcpy(c_out, em.c, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (prefix_out) RT_HIP(ctx, hipMemcpy(prefix_out, em.prefix, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    *total = ctx->emit_total;
    *n_triangles = (int32_t)count;
    return RT_OK;
}

int rt_kat_emission_sample(rt_ctx *ctx, int count, const uint32_t *hs, const int32_t *seg, uint32_t *tri_out, float *point_out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    if (count < 0 || (count > 0 && (!hs || !seg || !tri_out || !point_out))) return fail(ctx, RT_ERR_INVALID, "bad KAT arguments");
    if (int rc = emit_refresh(ctx); rc != RT_OK) return rc;
    if (ctx->emit_total == 0) return fail(ctx, RT_ERR_INVALID, "no table to draw from: no mesh emits, or every emitting triangle has no area (rt_scene_set_emission)");
    if (count == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    hipStream_t q = own_stream(ctx);
    DevBuf dhs, dseg, dout;                                            // out: the triangle and three floats of the point per draw
    int rc;
    if ((rc = upload(ctx, dhs, hs, (size_t)count * 4)) != RT_OK || (rc = upload(ctx, dseg, seg, (size_t)count * 4)) != RT_OK || (rc = ensure(ctx, dout, (size_t)count * 16)) != RT_OK) return rc;
    uint32_t *dt = static_cast<uint32_t *>(dout.p);
    float *dq = reinterpret_cast<float *>(dt + count);
    hipLaunchKernelGGL(rtk::kat_emit_sample_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, q, emit_dist_of(ctx), ctx->scene.tri, static_cast<const uint32_t *>(dhs.p),
                       static_cast<const int *>(dseg.p), count, dt, dq);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(tri_out, dt, (size_t)count * 4, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipMemcpyAsync(point_out, dq, (size_t)count * 12, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "KAT launch: %s", hipGetErrorString(e));
    return RT_OK;
}

// FNV-1a over the device arrays the traversal kernels read: out[0] the float sibling pairs (nodesb), [1] the 16-bit fixed-point pairs (nodesh), [2] the 4-wide quads
// (nodesw: WHICH four nodes a quad holds is the surface-area DP's choice, rt_qnodes.hip.h), [3] the leaf boxes by triangle (leaflh); 0 = the array is not in use.
int rt_kat_layout_hash(rt_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return fail(ctx, RT_ERR_INVALID, "bad arguments");
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    RT_OWN_STREAM(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const rtk::Scene &sc = ctx->scene;
    const void *src[4] = {sc.nodesb, sc.nodesh, sc.nodesw, sc.leaflh};
    const size_t bytes[4] = {2 * ((size_t)sc.n_nodes + 1) * 16, ((size_t)sc.n_nodes + 1) * 16, ((size_t)(sc.n_nodes & ~1) + 2) * 32 /* quads of the pairs c = 0, 2, .. <= n_nodes */, (size_t)sc.n_tris * 32};
    std::vector<unsigned char> h;
    for (int k = 0; k < 4; ++k) {
        out[k] = 0;
        if (!src[k] || sc.n_nodes <= 0) continue;
        h.resize(bytes[k]);
        if (int rc = copy_back(ctx, h.data(), src[k], bytes[k]); rc != RT_OK) return rc;
        uint64_t x = 0xcbf29ce484222325ull;
        for (unsigned char c : h) x = (x ^ c) * 0x100000001b3ull;
        out[k] = x ? x : 1;
    }
    return RT_OK;
}

}  // extern "C"
