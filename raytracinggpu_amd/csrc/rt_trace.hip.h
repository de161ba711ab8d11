// rt_trace.hip.h -- rt_trace_rays: a batch of explicit rays through the PRODUCTION traversal launches.
// Included at the end of rt_capi.hip (same translation unit: it uses the traversal plan and launch geometry of the render path, plan_trav / wf_geometry / path_geometry).
//
// TriangleMesh::intersect (cpu_launcher.cpp:238-313; optimized.cu:220-285) is callable with ANY ray; in the render path rays reach
// the traversal kernels only through the uniform kernels (camera rays, bounce and shadow rays), which never produce a zero or
// denormal direction component, an origin inside the mesh on purpose, or the other corner cases the reference's own vectors cover.
// rt_trace_rays writes the caller's rays into the traversal queue exactly as wf_emit_ray does (root-box test, cpu:279, by the
// same slab_filtered; slot-order records) and runs the same kernel instantiations with the same launch geometry a frame uses:
// wf_travq (work stack: BOX / TRI steps, refill, leaf queue, serial drain under RT_TRAVQ_CAP), wf_trav (per-lane stackless walk
// with work splitting) or wf_path (the fused kernel, explicit-ray items).  out[i] = (hit, t, N.xyz) with N normalised as cpu:308.
#pragma once

namespace rtk {

// one lane per ray slot pair: rays r < n are the caller's, the rest of the 2 n_paths slots carry no ray
__global__ __launch_bounds__(256) void trace_emit_kernel(const Scene sc, const WfState st, const float *__restrict__ rays, int n) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2 * st.n_paths) return;
    const int q = wf_ray_to_slot(st, r);
    bool need = false;
    f3 O = mk(0, 0, 0), u = mk(0, 0, 1);
    if (r < n) {
        const float *p = rays + 6 * (size_t)r;
        O = mk(p[0], p[1], p[2]); u = mk(p[3], p[4], p[5]);
        if (sc.mesh_slot >= 0 && sc.n_nodes > 0) need = slab_filtered(sc.root_lo, sc.root_hi, O, u, ray_inv(u));   // wf_emit_ray's root-box test
    }
    st.M[r] = WF_NOHIT;
    st.QR[2 * (size_t)q] = make_float4(O.x, O.y, O.z, u.x);
    st.QR[2 * (size_t)q + 1] = make_float4(u.y, u.z, __int_as_float(need ? PQ_TRAV : 0), 0.f);
}

__global__ __launch_bounds__(256) void trace_close_kernel(const Scene sc, const unsigned long long *__restrict__ M, int n, float *__restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const unsigned long long m = M[r];
    float *o = out + 5 * (size_t)r;
    if (m == WF_NOHIT) { o[0] = 0.f; o[1] = 1e9f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f; return; }   // t = INF narrowed (cpu:283)
    const float4 q2 = sc.tri[3 * (size_t)(unsigned int)m + 2];
    const f3 N = normalize(mk(q2.y, q2.z, q2.w));                     // cpu:308
    o[0] = 1.f; o[1] = __uint_as_float((unsigned int)(m >> 32)); o[2] = N.x; o[3] = N.y; o[4] = N.z;
}

// rt_kat_surface: the mesh hit of each ray (the production traversal's result) and what wf_advance<kFormTex> makes of it -- tex_albedo, the one device function both call.
// out[r] = (object slot or -1, triangle in its mesh's uploaded order, t, u, v, albedo rgb); an untextured mesh reports uv (0, 0) and its constant albedo.
__global__ __launch_bounds__(256) void kat_surface_kernel(const Scene sc, const TexScene ts, const unsigned long long *__restrict__ M, const float *__restrict__ rays,
                                                          const int *__restrict__ visit2local, int n, float *__restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const unsigned long long m = M[r];
    float *o = out + 8 * (size_t)r;
    if (m == WF_NOHIT) { o[0] = -1.f; o[1] = -1.f; o[2] = 1e9f; o[3] = o[4] = o[5] = o[6] = o[7] = 0.f; return; }
    const int tri = (int)(unsigned int)m;
    const int obj = mesh_obj_of_tri(sc, tri);
    const float *p = rays + 6 * (size_t)r;
    const f3 O = mk(p[0], p[1], p[2]), u = mk(p[3], p[4], p[5]);
    float2 uv = make_float2(0.f, 0.f);
    f3 alb;
    if ((ts.mask >> obj) & 1) {
        alb = tex_albedo(sc, ts, obj, tri, tri_bary(sc, tri, O, u), uv);
    } else {
        const Material mt = material_of(sc, obj);
        alb = mk(mt.ar, mt.ag, mt.ab);
    }
    o[0] = (float)obj; o[1] = (float)visit2local[tri]; o[2] = __uint_as_float((unsigned int)(m >> 32));
    o[3] = uv.x; o[4] = uv.y; o[5] = alb.x; o[6] = alb.y; o[7] = alb.z;
}

}  // namespace rtk

// n ray slots through the traversal launch of a frame of a default context (plan_trav without RT_TRAVQ_LDS staging, one sub-frame) on stream q, with the traversal results
// in bufM and the queue in bufQR.  emit(st, grid, block): the launch that writes every one of the 2 st.n_paths slots' records and M entries (trace_emit_kernel's contract).
// M: bits(t) << 32 | triangle (visit order) per ray, WF_NOHIT if none.  variant: wavefront_queue (wf_travq) or wavefront (wf_trav).
// TraceLaunch: that launch, kept, for a caller that rewrites the records in place and traverses them again (trace_again: rt_render_aov_surface's rounds).
struct TraceLaunch { TravPlan t; rtk::Frame fr; rtk::WfState st; int64_t tblocks; };
template <class Emit>
static int trace_queue(rt_ctx *ctx, int n, float tri_tmin, int variant, hipStream_t q, DevBuf &bufM, DevBuf &bufQR, TraceLaunch &tl, Emit emit) {
    const rtk::Scene &sc = ctx->scene;
    if (variant == RT_VARIANT_WAVEFRONT_QUEUE && (sc.n_nodes + 2 >= (1 << rtk::kQNodeBits) || !ctx->travq_ok)) variant = RT_VARIANT_WAVEFRONT;
    const Knobs &kn = ctx->knobs;
    int rc;
    rtk::Frame &fr = tl.fr;
    fr = rtk::Frame{};
    fr.tri_tmin = tri_tmin; fr.segs = 1; fr.spp = 1; fr.W = 1; fr.H = 1; fr.n_rows = 1; fr.tile_rows = 1; fr.tile_step = 1; fr.out_tile_step = 1;
    Variant v{};
    v.variant = v.asked = variant;
    TravPlan &t = tl.t;
    if ((rc = plan_trav(ctx, v, false, 0, t)) != RT_OK) return rc;
    rtk::WfState &st = tl.st;
    st = rtk::WfState{};
    st.n_paths = ((n + 1) / 2 + 1) / 2 * 2;                           // 2 n_paths ray slots >= n, a multiple of 4
    st.n_px = st.n_paths; st.tiles_x = 1;
    const int64_t tblocks = tl.tblocks = wf_geometry(kn, ctx->n_cus, t.bpc, 1, t.wpb, t.queue, st);
    const size_t q_slots = (size_t)st.slots_per_block * (size_t)tblocks;
    if ((rc = ensure(ctx, bufM, 2 * (size_t)st.n_paths * 8)) != RT_OK || (rc = ensure(ctx, bufQR, q_slots * 32)) != RT_OK) return rc;
    RT_HIP(ctx, hipMemsetAsync(bufQR.p, 0, q_slots * 32, q));        // padding slots carry no ray
    st.QR = static_cast<float4 *>(bufQR.p);
    st.M = static_cast<unsigned long long *>(bufM.p);
    st.init_m = t.queue ? 0 : 1;
    st.epoch = 0; st.nonce = 0;
    emit(st, dim3((unsigned)((2 * st.n_paths + 255) / 256)), dim3(256));
    if (t.have_mesh) launch_trav(t, tblocks, q, sc, fr, st);
    return RT_OK;
}
template <class Emit>
static int trace_queue(rt_ctx *ctx, int n, float tri_tmin, int variant, hipStream_t q, DevBuf &bufM, DevBuf &bufQR, unsigned long long *&M, Emit emit) {
    TraceLaunch tl;
    const int rc = trace_queue(ctx, n, tri_tmin, variant, q, bufM, bufQR, tl, emit);
    if (rc == RT_OK) M = tl.st.M;
    return rc;
}
// the traversal launch of tl once more, over the records its queue holds now (every ray's M entry initialised by whoever wrote them, as an emitter does)
static void trace_again(rt_ctx *ctx, const TraceLaunch &tl, hipStream_t q) {
    if (tl.t.have_mesh) launch_trav(tl.t, tl.tblocks, q, ctx->scene, tl.fr, tl.st);
}

// The caller's rays (din: n x 6 floats on the device) through the production traversal of `variant`; M: bits(t) << 32 | triangle (visit order) per ray, WF_NOHIT if none
static int trace_to_m(rt_ctx *ctx, const float *din, int n, float tri_tmin, int variant, unsigned long long *&M) {
    const rtk::Scene &sc = ctx->scene;
    if (variant == RT_VARIANT_PATH && sc.n_nodes + 2 >= (1 << rtk::kPNodeBits)) variant = RT_VARIANT_WAVEFRONT;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    hipStream_t q = own_stream(ctx);
    const Knobs &kn = ctx->knobs;
    M = nullptr;
    if (variant != RT_VARIANT_PATH) {
        ctx->qf_sig = 0;                                               // the queue is the render path's: it zeroes its own layout again
        return trace_queue(ctx, n, tri_tmin, variant, q, ctx->wfM, ctx->wfQR, M, [&](const rtk::WfState &st, dim3 g, dim3 b) {
            hipLaunchKernelGGL(rtk::trace_emit_kernel, g, b, 0, q, sc, st, din, n);
        });
    }
    // the fused kernel: items = the rays, in wf_path's own launch geometry (path_geometry, as launch_path uses it)
    int rc;
    rtk::Frame fr{};
    fr.tri_tmin = tri_tmin; fr.segs = 1; fr.spp = 1; fr.W = 1; fr.H = 1; fr.n_rows = 1; fr.tile_rows = 1; fr.tile_step = 1; fr.out_tile_step = 1;
    const size_t lds = (size_t)(rtk::kQBlock / 64) * rtk::PCarve::bytes(1) + 16;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, rtk::wf_path<false>, rtk::kQBlock, lds) != hipSuccess || nb < 1) return fail(ctx, RT_ERR_UNSUPPORTED, "wf_path does not fit a CU");
    rtk::PathState ps{};
    ps.n_paths = (n + 63) / 64 * 64; ps.tiles_x = 1; ps.samp0 = 0; ps.n_samp = 1; ps.samp_out = nullptr;
    ps.n_groups = ps.n_paths / 4;
    if ((rc = ensure(ctx, ctx->wfM, (size_t)ps.n_paths * 8)) != RT_OK) return rc;
    M = static_cast<unsigned long long *>(ctx->wfM.p);
    ps.ext_rays = din; ps.ext_out = M; ps.n_ext = n;
    const int64_t tblocks = path_geometry(kn, ctx->n_cus, std::min(kn.path_bpc, nb), 1, ps);
    RT_HIP(ctx, hipMemsetAsync(M, 0xff, (size_t)ps.n_paths * 8, q));      // rays the kernel never reaches (none) would read as no hit
    hipLaunchKernelGGL(rtk::wf_path<false>, dim3((unsigned)tblocks), dim3(rtk::kQBlock), lds, q, sc, fr, ps, capped_stack(kn, rtk::kPStack), kn.path_low, kn.path_shade_min);
    return RT_OK;
}

extern "C" int rt_trace_rays(rt_ctx *ctx, const float *rays, int n, float tri_tmin, int variant, float *out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (n < 0 || (n > 0 && (!rays || !out))) return fail(ctx, RT_ERR_INVALID, "bad ray batch");
    if (n >= (1 << 28)) return fail(ctx, RT_ERR_INVALID, "at most 2^28 rays per call");
    if (variant == RT_VARIANT_AUTO) variant = RT_VARIANT_WAVEFRONT_QUEUE;
    if (variant != RT_VARIANT_WAVEFRONT_QUEUE && variant != RT_VARIANT_WAVEFRONT && variant != RT_VARIANT_PATH)
        return fail(ctx, RT_ERR_UNSUPPORTED, "rt_trace_rays runs the traversal of variant wavefront_queue (wf_travq), wavefront (wf_trav) or path (wf_path)");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    hipStream_t q = own_stream(ctx);
    DevBuf din, dout;
    int rc;
    if ((rc = upload(ctx, din, rays, (size_t)n * 6 * sizeof(float))) != RT_OK || (rc = ensure(ctx, dout, (size_t)n * 5 * sizeof(float))) != RT_OK) return rc;
    unsigned long long *M = nullptr;
    if ((rc = trace_to_m(ctx, static_cast<const float *>(din.p), n, tri_tmin, variant, M)) != RT_OK) return rc;
    hipLaunchKernelGGL(rtk::trace_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, ctx->scene, M, n, static_cast<float *>(dout.p));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "rt_trace_rays: %s", hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_kat_surface(rt_ctx *ctx, const float *rays, int n, float tri_tmin, float *out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    if (n < 0 || (n > 0 && (!rays || !out))) return fail(ctx, RT_ERR_INVALID, "bad ray batch");
    if (n >= (1 << 28)) return fail(ctx, RT_ERR_INVALID, "at most 2^28 rays per call");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    if (int rr = refresh_host_mesh(ctx); rr != RT_OK) return rr;
    hipStream_t q = own_stream(ctx);
    // visit rank -> the triangle's index in its own mesh's uploaded order
    std::vector<int> local(std::max<size_t>(ctx->tri_perm.size(), 1), -1);
    for (size_t t = 0; t < ctx->tri_perm.size(); ++t) {
        const int g = ctx->tri_perm[t];
        for (const rt_ctx::MeshPart &p : ctx->parts) if (g >= p.tri_off && g < p.tri_off + p.nt) local[t] = g - p.tri_off;
    }
    DevBuf din, dout, dloc;
    int rc;
    if ((rc = upload(ctx, din, rays, (size_t)n * 6 * sizeof(float))) != RT_OK || (rc = ensure(ctx, dout, (size_t)n * 8 * sizeof(float))) != RT_OK ||
        (rc = upload(ctx, dloc, local.data(), local.size() * sizeof(int))) != RT_OK) return rc;
    unsigned long long *M = nullptr;
    if ((rc = trace_to_m(ctx, static_cast<const float *>(din.p), n, tri_tmin, RT_VARIANT_WAVEFRONT_QUEUE, M)) != RT_OK) return rc;
    hipLaunchKernelGGL(rtk::kat_surface_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, q, ctx->scene, tex_scene(ctx), M, static_cast<const float *>(din.p),
                       static_cast<const int *>(dloc.p), n, static_cast<float *>(dout.p));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) return fail(ctx, RT_ERR_HIP, "rt_kat_surface: %s", hipGetErrorString(e));
    return RT_OK;
}
