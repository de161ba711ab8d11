// rt_aov.hip.h -- rt_render_aov[_device]: the first-hit feature buffers (G-buffer) of a frame, for the edge-avoiding filter of rt_denoise.hip.h; and
// rt_render_aov_motion[_device]: the same planes with the two previous-frame planes a deforming or moving scene is reprojected from.
// Included at the end of rt_capi.hip, after rt_trace.hip.h (same translation unit: it runs the traversal launch of rt_trace_rays, trace_queue; the host half uses
// rt_host_post.hip.h).  The device functions and the host prologue here are rt_aov_surface.hip.h's too.
//
// One ray per pixel of the rows: the pixel-centre camera ray (camera_dir with sigma = 0: no sample key is read), intersected with the scene as
// Scene::intersect_all does (cpu_launcher.cpp:545-564): every sphere by the sphere search of wf_advance (spheres_near2), the meshes by the production
// traversal (wf_travq with the launch plan of a frame), the two joined by mesh_beats_sphere -- the strict '<' in object order.  The normal is hit_normal, the
// albedo the object's or tex_albedo's: the device functions of rt_shade.hip.h / rt_wavefront.hip.h the render kernels call, so the planes hold the very values
// the first segment of a path is shaded with.  Nothing here touches the render path's state: the queue and the results live in buffers of their own.
#pragma once

namespace rtk {

// the camera ray of AOV item r: pixel (r % W) of local row (r / W)
__device__ __forceinline__ void aov_ray(const Scene &sc, const Frame &fr, int r, f3 &O, f3 &u) {
    const int lrow = r / fr.W, px = r - lrow * fr.W;
    O = mk(sc.camx, sc.camy, sc.camz);
    u = camera_dir(fr, O, fr.z, px, image_row(fr, lrow), 0u);      // fr.sigma == 0: the key is not read
}

// Closes the query of ray (O, u) as wf_advance closes a continuation ray's: every sphere by spheres_near2, m the traversal's result word for the meshes, the two joined
// by mesh_beats_sphere.  obj < 0: a miss; tri < 0: a sphere.
struct AovHit { float t; int obj, tri; };
__device__ __forceinline__ AovHit aov_close_query(const Scene &sc, f3 O, f3 u, unsigned long long m) {
    SphereNear hy, hx;
    spheres_near2(sc, O, u, true, u, false, hy, hx);
    AovHit h{hy.t, hy.obj, -1};
    if (m != WF_NOHIT) {
        const float tm = __uint_as_float((unsigned int)(m >> 32));
        const int mobj = mesh_obj_of_tri(sc, (int)(unsigned int)m);
        if (mesh_beats_sphere(h.t, h.obj, tm, mobj)) { h.t = tm; h.obj = mobj; h.tri = (int)(unsigned int)m; }
    }
    return h;
}

// the albedo the planes record for hit h of ray (O, u): the object's, or tex_albedo's on a textured mesh (bary: hit_normal's, where it made them)
__device__ __forceinline__ f3 aov_albedo(const Scene &sc, const TexScene &ts, const AovHit &h, f3 O, f3 u, Bary bary, bool have_bary) {
    if (h.tri >= 0 && ((ts.mask >> h.obj) & 1)) {
        if (!have_bary) bary = tri_bary(sc, h.tri, O, u);
        float2 uv;
        return tex_albedo(sc, ts, h.obj, h.tri, bary, uv);
    }
    const Material mt = material_of(sc, h.obj);
    return mk(mt.ar, mt.ag, mt.ab);
}

// trace_emit_kernel with the rays made here: one lane per ray slot pair, rays r < n are the pixels', the rest of the 2 n_paths slots carry no ray
__global__ __launch_bounds__(256) void aov_emit_kernel(const Scene sc, const Frame fr, const WfState st, int n) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2 * st.n_paths) return;
    const int q = wf_ray_to_slot(st, r);
    bool need = false;
    f3 O = mk(0, 0, 0), u = mk(0, 0, 1);
    if (r < n) {
        aov_ray(sc, fr, r, O, u);
        if (sc.mesh_slot >= 0 && sc.n_nodes > 0) need = slab_filtered(sc.root_lo, sc.root_hi, O, u, ray_inv(u));   // wf_emit_ray's root-box test
    }
    st.M[r] = WF_NOHIT;
    st.QR[2 * (size_t)q] = make_float4(O.x, O.y, O.z, u.x);
    st.QR[2 * (size_t)q + 1] = make_float4(u.y, u.z, __int_as_float(need ? PQ_TRAV : 0), 0.f);
}

// closes the query as wf_advance closes a continuation ray's and writes the three planes (n float4 each, consecutive)
// MOTION (rt_render_aov_motion*): the same pixel also writes the two PREVIOUS-FRAME planes -- (N', id) and (P', 1) in the layout of planes 0 and 1 -- that
// rt_temporal_accumulate* takes as its `aov` with no motion table.  Its one argument -- the snapshot vertices, the two planes, the snapshot mask, the rigid table --
// exists in that instantiation alone, so aov_close_kernel<false> has the arguments and the instructions the kernel always had.  A hit on a mesh whose bit is set gathers
// one int4 and three float4 of verts_prev, as coherent as the image is: neighbouring pixels hit the same or neighbouring triangles.  The table sits in the
// kernel-argument segment and a lane reads the record of its own object, as temporal_accumulate_kernel does.
struct AovRigid { float r[9], t[3]; };                               // previous = r (row-major) * current + t
struct AovMotion {
    const float4 *__restrict__ verts_prev;                            // Scene::verts as rt_mesh_snapshot_vertices kept them (read only where a bit of snap_mask is set)
    float4 *__restrict__ prev;                                        // 2 n float4
    uint32_t snap_mask;
    int have_motion;
    AovRigid m[RT_MAX_OBJECTS];
};
// ... and the form the host picks only while a SMOOTH mesh holds a normal snapshot (rt_mesh_snapshot_normals): N' of a hit on such a mesh is smooth_normal's expression over
// the snapshot's three corner normals -- the previous frame's plane 0 at this barycentric point of this triangle, bit for bit -- a 48-byte gather per such pixel.  A third
// instantiation, told apart by the argument's type: the two older ones keep their names, their arguments and their instructions.
struct AovMotionNormals : AovMotion {
    const float4 *__restrict__ nrm_prev;                              // Scene::nrm as rt_mesh_snapshot_normals kept it (read only where a bit of nsnap_mask is set)
    uint32_t nsnap_mask;
};
template <bool MOTION, class... Mo>
__global__ __launch_bounds__(256) void aov_close_kernel(const Scene sc, const Frame fr, const TexScene ts, const unsigned long long *__restrict__ M, int n, float4 *__restrict__ out,
                                                        const Mo... mo) {
    static_assert(sizeof...(Mo) == (MOTION ? 1 : 0), "the motion instantiation takes one AovMotion");
    constexpr bool NPREV = (std::is_same_v<Mo, AovMotionNormals> || ...);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    f3 O, u;
    aov_ray(sc, fr, r, O, u);
    const AovHit h = aov_close_query(sc, O, u, M[r]);
    float4 o0 = make_float4(0.f, 0.f, 0.f, -1.f), o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = o1;
    [[maybe_unused]] float4 p0, p1;
    if constexpr (MOTION) { p0 = make_float4(0.f, 0.f, 0.f, -1.f); p1 = make_float4(0.f, 0.f, 0.f, 0.f); }   // a miss
    if (h.obj >= 0) {
        const f3 P = O + h.t * u;                                     // cpu:560
        Bary bary{0.f, 0.f, 0.f};
        bool have_bary = false;
        const f3 N = hit_normal(sc, h.obj, h.tri, O, u, P, bary, have_bary);
        const f3 alb = aov_albedo(sc, ts, h, O, u, bary, have_bary);
        o0 = make_float4(N.x, N.y, N.z, (float)h.obj);
        o1 = make_float4(P.x, P.y, P.z, 1.f);
        o2 = make_float4(alb.x, alb.y, alb.z, 0.f);
        if constexpr (MOTION) {
            const AovMotion &am = (mo, ...);
            f3 Np = N, Pp = P;
            if (h.tri >= 0 && ((am.snap_mask >> h.obj) & 1u)) {       // the same barycentric point of the triangle's previous corners
                const bool smooth = have_bary;                        // (hit_normal: have_bary == smooth_hit)
                if (!have_bary) bary = tri_bary(sc, h.tri, O, u);
                const int4 ix = sc.tidx[h.tri];
                const float4 a = am.verts_prev[ix.x], b = am.verts_prev[ix.y], c = am.verts_prev[ix.z];
                const f3 A = mk(a.x, a.y, a.z), B = mk(b.x, b.y, b.z), C = mk(c.x, c.y, c.z);
                Pp = (bary.alpha * A + bary.beta * B) + bary.gamma * C;
                if (!smooth) Np = normalize(cross(B - A, C - A));     // retri_kernel's and flat_normal's operations: the previous frame's plane 0, bit for bit
            } else if (am.have_motion) {                              // temporal_accumulate_kernel's expressions with the record of this object
                const AovRigid &m = am.m[h.obj & (RT_MAX_OBJECTS - 1)];
                Pp = mk(((m.r[0] * P.x + m.r[1] * P.y) + m.r[2] * P.z) + m.t[0], ((m.r[3] * P.x + m.r[4] * P.y) + m.r[5] * P.z) + m.t[1],
                        ((m.r[6] * P.x + m.r[7] * P.y) + m.r[8] * P.z) + m.t[2]);
                Np = mk((m.r[0] * N.x + m.r[1] * N.y) + m.r[2] * N.z, (m.r[3] * N.x + m.r[4] * N.y) + m.r[5] * N.z, (m.r[6] * N.x + m.r[7] * N.y) + m.r[8] * N.z);
            }
            if constexpr (NPREV) {                                    // ahead of the record's rotation and of N' = N: the normal the previous frame shaded with
                const AovMotionNormals &an = (mo, ...);
                if (have_bary && ((an.nsnap_mask >> h.obj) & 1u)) {
                    const float4 na = an.nrm_prev[3 * h.tri], nb = an.nrm_prev[3 * h.tri + 1], nc = an.nrm_prev[3 * h.tri + 2];
                    Np = normalize((bary.alpha * mk(na.x, na.y, na.z) + bary.beta * mk(nb.x, nb.y, nb.z)) + bary.gamma * mk(nc.x, nc.y, nc.z));
                }
            }
            p0 = make_float4(Np.x, Np.y, Np.z, (float)h.obj);
            p1 = make_float4(Pp.x, Pp.y, Pp.z, 1.f);
        }
    }
    out[r] = o0;
    out[(size_t)n + r] = o1;
    out[2 * (size_t)n + r] = o2;
    if constexpr (MOTION) {
        const AovMotion &am = (mo, ...);
        am.prev[r] = p0;
        am.prev[(size_t)n + r] = p1;
    }
}

}  // namespace rtk

// what rt_render_aov_device and rt_render_aov_surface_device ask of their arguments alike; n: the pixels of the rows (0: nothing to do)
static int aov_check(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, const void *out_aov_dev, int &n) {
    n = 0;
    if (!ctx->have_scene) return fail(ctx, RT_ERR_NO_SCENE, "rt_scene_upload has not been called");
    if (!p || !rows || !out_aov_dev) return fail(ctx, RT_ERR_INVALID, "params/rows/out is NULL");
    if (p->width <= 0 || p->height <= 0) return fail(ctx, RT_ERR_INVALID, "width/height must be positive");
    if (rows->n_rows < 0 || rows->row0 < 0 || rows->tile_rows <= 0 || rows->tile_step <= 0) return fail(ctx, RT_ERR_INVALID, "bad row specification");
    if (rows->n_rows == 0) return RT_OK;
    const int64_t last = rows->n_rows - 1;
    const int64_t last_row = rows->row0 + (last / rows->tile_rows) * rows->tile_rows * (int64_t)rows->tile_step + (last % rows->tile_rows);
    if (last_row >= p->height) return fail(ctx, RT_ERR_INVALID, "rows reach image row %lld >= height %d", (long long)last_row, p->height);
    const int64_t n64 = (int64_t)rows->n_rows * p->width;
    if (n64 >= kPostMaxPixels) return fail(ctx, RT_ERR_INVALID, "at most 2^28 pixels per call");
    n = (int)n64;
    return RT_OK;
}
// the host forms: the planes of device(rows, planes on the device) copied out; rows == NULL = the whole frame
template <class Device>
static int aov_to_host(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, float *out_aov_host, Device device) {
    RT_OWN_STREAM(ctx);
    if (!p || !out_aov_host) return fail(ctx, RT_ERR_INVALID, "params/out is NULL");
    const rt_rows whole{0, p->height, p->height > 0 ? p->height : 1, 1};
    if (!rows) rows = &whole;
    const size_t bytes = 3 * (size_t)(rows->n_rows > 0 ? rows->n_rows : 0) * (p->width > 0 ? p->width : 0) * sizeof(float4);
    return staged(ctx, {}, 0, bytes, out_aov_host, [&](uint8_t *d) { return device(rows, d); });
}

// What the two device entries do alike, up to the camera rays' traversal: the argument checks (n == 0 with RT_OK: nothing to do, nothing was issued), the stream,
// aov_state for state_bytes per pixel (rt_render_aov_surface's record between its rounds; 0: none), the frame of a render call with these parameters (make_frame: camera distance, pose, rows) without the jitter, the pipelining note -- a pipelined frame must not start
// behind the write of the planes -- and aov_emit_kernel through the queue launch.
struct AovCall { int n; hipStream_t q; rtk::Scene scn; rtk::Frame fr; TraceLaunch tl; };
static int aov_begin(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, void *out_aov_dev, void *stream, size_t state_bytes, AovCall &a) {
    int rc = aov_check(ctx, p, rows, out_aov_dev, a.n);
    if (rc != RT_OK || a.n == 0) return rc;
    if ((rc = call_stream(ctx, stream, a.q)) != RT_OK) return rc;
    if (state_bytes && (rc = ensure(ctx, ctx->aov_state, (size_t)a.n * state_bytes)) != RT_OK) return rc;
    Chunk c{p, rows, a.q, nullptr, nullptr, false, 1, 1, {}, {}, nullptr};
    make_frame(ctx, out_aov_dev, pose, c);
    c.fr.sigma = 0.f;
    a.scn = c.scn; a.fr = c.fr;
    note_between(ctx, a.q, {{out_aov_dev, 3 * (size_t)a.n * sizeof(float4)}});
    return trace_queue(ctx, a.n, p->tri_tmin, RT_VARIANT_WAVEFRONT_QUEUE, a.q, ctx->aovM, ctx->aovQR, a.tl, [&](const rtk::WfState &st, dim3 g, dim3 b) {
        hipLaunchKernelGGL(rtk::aov_emit_kernel, g, b, 0, a.q, a.scn, a.fr, st, a.n);
    });
}

extern "C" int rt_render_aov_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, void *out_aov_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    AovCall a;
    if (int rc = aov_begin(ctx, p, pose, rows, out_aov_dev, stream, 0, a); rc != RT_OK || a.n == 0) return rc;
    hipLaunchKernelGGL(rtk::aov_close_kernel<false>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, a.q, a.scn, a.fr, tex_scene(ctx), a.tl.st.M, a.n, static_cast<float4 *>(out_aov_dev));
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

extern "C" int rt_render_aov(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, float *out_aov_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    return aov_to_host(ctx, p, rows, out_aov_host, [&](const rt_rows *r, void *dev) { return rt_render_aov_device(ctx, p, pose, r, dev, nullptr); });
}

// ---- rt_render_aov_motion[_device]: the same call, which also writes the previous-frame planes of a deforming or moving scene (raytrace_hip.h; the kernel's MOTION form) ----
extern "C" int rt_render_aov_motion_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, const rt_motion *motion, void *out_aov_dev,
                                           void *out_prev_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int n = 0;
    if (int rc = aov_check(ctx, p, rows, out_aov_dev, n); rc != RT_OK) return rc;
    if (!out_prev_dev) return fail(ctx, RT_ERR_INVALID, "out_prev is NULL");
    if (overlaps(out_aov_dev, 3 * (size_t)n * sizeof(float4), out_prev_dev, 2 * (size_t)n * sizeof(float4))) return fail(ctx, RT_ERR_INVALID, "out_prev overlaps out_aov");
    AovCall a;
    if (int rc = aov_begin(ctx, p, pose, rows, out_aov_dev, stream, 0, a); rc != RT_OK || a.n == 0) return rc;
    note_between(ctx, a.q, {{out_prev_dev, 2 * (size_t)a.n * sizeof(float4)}});
    rtk::AovMotionNormals am{};
    am.verts_prev = static_cast<const float4 *>(ctx->verts_prev.p);
    am.prev = static_cast<float4 *>(out_prev_dev);
    am.snap_mask = ctx->verts_prev.p ? ctx->snap_mask : 0u;           // (a set bit means the buffer exists: rt_mesh_snapshot_vertices)
    if (am.snap_mask && ctx->snap_ev && a.q != ctx->stream_) RT_HIP(ctx, hipStreamWaitEvent(a.q, ctx->snap_ev, 0));   // the snapshot's copy ran on the context's stream
    if (motion) {
        am.have_motion = 1;
        for (int k = 0; k < RT_MAX_OBJECTS; ++k) {
            for (int c = 0; c < 9; ++c) am.m[k].r[c] = motion[k].rotation[c];
            for (int c = 0; c < 3; ++c) am.m[k].t[c] = motion[k].translation[c];
        }
    }
    // the previous shading normals: only while a mesh that shades smoothly holds a normal snapshot (a set bit means nrm_prev exists: rt_mesh_snapshot_normals)
    am.nsnap_mask = ctx->nrm_prev.p ? ctx->nsnap_mask & (uint32_t)a.scn.smooth_mask : 0u;
    const dim3 grid((unsigned)((a.n + 255) / 256));
    if (am.nsnap_mask) {
        am.nrm_prev = static_cast<const float4 *>(ctx->nrm_prev.p);
        if (ctx->nsnap_ev && a.q != ctx->stream_) RT_HIP(ctx, hipStreamWaitEvent(a.q, ctx->nsnap_ev, 0));
        hipLaunchKernelGGL((rtk::aov_close_kernel<true, rtk::AovMotionNormals>), grid, dim3(256), 0, a.q, a.scn, a.fr, tex_scene(ctx), a.tl.st.M, a.n, static_cast<float4 *>(out_aov_dev), am);
    } else {
        const rtk::AovMotion plain = am;                              // (the argument the kernel always had)
        hipLaunchKernelGGL((rtk::aov_close_kernel<true, rtk::AovMotion>), grid, dim3(256), 0, a.q, a.scn, a.fr, tex_scene(ctx), a.tl.st.M, a.n, static_cast<float4 *>(out_aov_dev), plain);
    }
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

extern "C" int rt_render_aov_motion(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, const rt_motion *motion, float *out_aov_host,
                                    float *out_prev_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!p || !out_aov_host || !out_prev_host) return fail(ctx, RT_ERR_INVALID, "params/out/out_prev is NULL");
    const rt_rows whole{0, p->height, p->height > 0 ? p->height : 1, 1};
    if (!rows) rows = &whole;
    const size_t plane = (size_t)(rows->n_rows > 0 ? rows->n_rows : 0) * (p->width > 0 ? p->width : 0) * sizeof(float4);
    if (overlaps(out_aov_host, 3 * plane, out_prev_host, 2 * plane)) return fail(ctx, RT_ERR_INVALID, "out_prev overlaps out_aov");
    // the previous-frame planes, then the three planes (the result staged copies out)
    return staged(ctx, {}, 2 * plane, 3 * plane, out_aov_host, [&](uint8_t *d) {
        const int r = rt_render_aov_motion_device(ctx, p, pose, rows, motion, d + 2 * plane, d, nullptr);
        if (r != RT_OK) return r;
        if (plane) RT_HIP(ctx, hipMemcpyAsync(out_prev_host, d, 2 * plane, hipMemcpyDeviceToHost, own_stream(ctx)));   // (staged waits for the stream)
        return (int)RT_OK;
    });
}
