// rt_aov_surface.hip.h -- rt_render_aov_surface[_device]: the feature buffers of the first DIFFUSE surface a pixel shows, reached through mirrors and glass.
// Included at the end of rt_capi.hip, after rt_aov.hip.h: the step kernel is built from its device functions (aov_close_query, aov_albedo), the entry
// starts with its host prologue (aov_begin: aov_emit_kernel through the traversal launch of trace_queue).
//
// The specular branches of Scene::getColor (cpu_launcher.cpp:573-604) draw no random number: reflection, total reflection or refraction, whichever the ray's index
// and the surface decide.  The pixel-centre camera ray's chain to its first diffuse surface is therefore a function of the scene alone, and along it the colour is
// handed through unchanged, so that surface's albedo factors out of the pixel as it does at a diffuse first hit.  The chain here is the render kernels' own: every
// segment is intersected as aov_close_kernel intersects the camera ray (spheres_near2, the production traversal, mesh_beats_sphere) and continued by mirror_step /
// refract_step of rt_shade.hip.h.
// How it runs: aov_emit_kernel writes the camera rays into the call's own queue; then max_specular + 1 rounds of (traversal launch, step kernel) follow on the
// stream, whatever the scene -- nothing is read back in between.  The step kernel closes each live pixel's query from the segment's queue record and either writes
// the three planes and retires the pixel, or writes the next segment's record (with wf_emit_ray's root-box test) over the old one.  A retired pixel's record
// carries no PQ_TRAV flag: the traversal launches that follow pass it by.  Per-pixel state between the rounds is one 16-byte record (SurfState).
#pragma once

namespace rtk {

// one pixel's chain between two rounds: Ray::refraction_index of the segment in flight, segments behind it, the camera ray's own hit, still in flight?
struct __attribute__((aligned(16))) SurfState { float refr; int k, first_id, live; };
static_assert(sizeof(SurfState) == 16, "one 16-byte load and store per pixel and round");

// Round `FIRST ? 0 : k` of the chain.  FIRST: every pixel is live with the state of a camera ray, and the state buffer is not read.  LAST: the round of
// k == max_specular, in which every live pixel retires: no record is emitted (and no state written: nothing reads it).
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void aov_surface_step_kernel(const Scene sc, const TexScene ts, const WfState st, float eps, int max_specular, int n,
                                                                 SurfState *__restrict__ state, float4 *__restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    SurfState s{1.f, 0, -1, 1};
    if (!FIRST) {
        s = state[r];
        if (!s.live) return;
    }
    const size_t q = (size_t)wf_ray_to_slot(st, r);
    const float4 r0 = st.QR[2 * q], r1 = st.QR[2 * q + 1];                // the segment's ray, as the traversal read it
    f3 O = mk(r0.x, r0.y, r0.z), u = mk(r0.w, r1.x, r1.y);
    const AovHit h = aov_close_query(sc, O, u, st.M[r]);
    const int win = h.obj;
    if (FIRST) s.first_id = win;
    float4 o0 = make_float4(0.f, 0.f, 0.f, -1.f), o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = o1;   // a miss, after any number of segments
    bool cont = false;
    if (win >= 0) {
        const f3 P = O + h.t * u;                                       // cpu:560
        Bary bary{0.f, 0.f, 0.f};
        bool have_bary = false;
        const f3 N = hit_normal(sc, win, h.tri, O, u, P, bary, have_bary);
        const Material mt = material_of(sc, win);
        const bool specular = mt.mirror || mt.n_in != mt.n_out;
        if (!LAST && specular && s.k < max_specular) {                    // cpu:573-604: the chain goes on
            if (mt.mirror) mirror_step(eps, P, N, O, u);
            else s.refr = refract_step(mt, s.refr, eps, P, N, O, u).refr_after;
            s.k += 1;
            cont = true;
        } else {                                                          // diffuse, or the bound is reached: this hit is the one recorded
            const f3 alb = aov_albedo(sc, ts, h, O, u, bary, have_bary);
            const int code = s.k == 0 ? win : win + 16 * s.first_id + 256 * s.k;   // the path code: at most 15 + 240 + 256 * 15 = 4095, exact in binary32
            o0 = make_float4(N.x, N.y, N.z, (float)code);
            o1 = make_float4(P.x, P.y, P.z, 1.f);
            o2 = make_float4(alb.x, alb.y, alb.z, specular ? 0.f : 1.f);
        }
    }
    if (cont) {
        bool need = false;
        if (sc.mesh_slot >= 0 && sc.n_nodes > 0) need = slab_filtered(sc.root_lo, sc.root_hi, O, u, ray_inv(u));   // wf_emit_ray's root-box test
        st.M[r] = WF_NOHIT;
        st.QR[2 * q] = make_float4(O.x, O.y, O.z, u.x);
        st.QR[2 * q + 1] = make_float4(u.y, u.z, __int_as_float(need ? PQ_TRAV : 0), 0.f);
        state[r] = s;
        return;
    }
    out[r] = o0;
    out[(size_t)n + r] = o1;
    out[2 * (size_t)n + r] = o2;
    if (!LAST) {
        st.QR[2 * q + 1] = make_float4(r1.x, r1.y, 0.f, 0.f);            // retired: no later round traverses this record
        s.live = 0;
        state[r] = s;
    }
}

}  // namespace rtk

extern "C" int rt_render_aov_surface_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, int max_specular, void *out_aov_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (max_specular < 0 || max_specular > RT_MAX_SEGMENTS - 1) return fail(ctx, RT_ERR_INVALID, "max_specular %d outside [0,%d]", max_specular, RT_MAX_SEGMENTS - 1);
    AovCall a;                                                            // round 0: the camera rays, through the queue launch of rt_render_aov
    if (int rc = aov_begin(ctx, p, pose, rows, out_aov_dev, stream, max_specular > 0 ? sizeof(rtk::SurfState) : 0, a); rc != RT_OK || a.n == 0) return rc;
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    const rtk::TexScene ts = tex_scene(ctx);
    rtk::SurfState *state = static_cast<rtk::SurfState *>(ctx->aov_state.p);
    float4 *out = static_cast<float4 *>(out_aov_dev);
    for (int k = 0; k <= max_specular; ++k) {
        if (k > 0) trace_again(ctx, a.tl, a.q);                              // the records the step kernel left: live ones carry PQ_TRAV, as an emitter's do
        const bool first = k == 0, final = k == max_specular;
        auto step = first ? (final ? rtk::aov_surface_step_kernel<true, true> : rtk::aov_surface_step_kernel<true, false>)
                          : (final ? rtk::aov_surface_step_kernel<false, true> : rtk::aov_surface_step_kernel<false, false>);
        hipLaunchKernelGGL(step, grid, block, 0, a.q, a.scn, ts, a.tl.st, p->eps, max_specular, a.n, state, out);
    }
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

extern "C" int rt_render_aov_surface(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, int max_specular, float *out_aov_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    return aov_to_host(ctx, p, rows, out_aov_host, [&](const rt_rows *r, void *dev) { return rt_render_aov_surface_device(ctx, p, pose, r, max_specular, dev, nullptr); });
}
