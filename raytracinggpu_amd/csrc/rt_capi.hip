// rt_capi.hip -- implementation of include/raytrace_hip.h (libraytrace_hip.so).
// Host side of the gfx950 render path: context, scene upload (layout conversion
// from the reference's arrays to the kernel's SoA layout), launches, timing.
#include "../../include/raytrace_hip.h"
#include "rt_kernels.hip.h"
#include "rt_persistent.hip.h"
#include "rt_wavefront.hip.h"
#include "rt_travq.hip.h"
#include "rt_path.hip.h"
#include "rt_meshops.hip.h"
#include "rt_normals.hip.h"
#include "rt_qnodes.hip.h"
#include "rt_bvhbuild.hip.h"
#include "rt_lbvh.hip.h"
#include "rt_adaptive.hip.h"
#include "rt_skydist.hip.h"
#include "rt_still.h"
#include "rt_rowcut.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "rt_host_ctx.hip.h"      // rt_ctx, knobs, buffers, errors
#include "rt_host_post.hip.h"     // what the device entries and the post-process stages share: the call's stream, the pipelining note, checks, host-form staging
#include "rt_host_scene.hip.h"    // scene upload: layouts, fixed-point nodes, forests
#include "rt_host_render.hip.h"   // frames as launches

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(int *count) {
    if (!count) return fail(nullptr, RT_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(nullptr, RT_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return RT_OK;
}

int rt_ctx_create(rt_ctx **out, int device_id) {
    if (!out) return fail(nullptr, RT_ERR_INVALID, "ctx out-pointer is NULL");
    *out = nullptr;
    int n = 0;
    PhaseClock pc;
    int rc = rt_device_count(&n);
    pc.lap("hipGetDeviceCount (runtime initialisation)");
    if (rc != RT_OK) return rc;
    if (n == 0) return fail(nullptr, RT_ERR_NO_DEVICE, "no HIP device visible");
    if (device_id < 0 || device_id >= n) return fail(nullptr, RT_ERR_INVALID, "device %d out of range [0,%d)", device_id, n);
    rt_ctx *ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "out of host memory");
    ctx->device = device_id;
    ctx->knobs = read_knobs();
    { const char *e = getenv("RT_LBVH_HOST_INSTALL"); ctx->lbvh_host_install = (e && *e && atoi(e) != 0) ? 1 : 0; }
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device_id);
    pc.lap("hipSetDevice");
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device_id);
    pc.lap("hipGetDeviceProperties");
    if (e == hipSuccess) e = ctx->ev_k0.create();
    if (e == hipSuccess) e = ctx->ev_k1.create();
    if (e == hipSuccess) e = ctx->ev_t0.create();
    if (e == hipSuccess) e = ctx->ev_t1.create();
    for (Event &ev : ctx->ev_trav) if (e == hipSuccess) e = ev.create();
    for (Event &ev : ctx->ev_adv) if (e == hipSuccess) e = ev.create();
    if (e == hipSuccess) e = ctx->fork_ev.create(hipEventDisableTiming);
    for (int k = 0; k < rt_ctx::kSlots; ++k) if (e == hipSuccess) e = ctx->slot_half[k].create(hipEventDisableTiming);
    for (int k = 0; k < rt_ctx::kSlots; ++k) {
        if (e == hipSuccess) e = ctx->slot_rendered[k].create(hipEventDisableTiming);
        if (e == hipSuccess) e = ctx->slot_done[k].create(hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        int code = fail(nullptr, RT_ERR_HIP, "context creation: %s", hipGetErrorString(e));
        rt_ctx_destroy(ctx);
        return code;
    }
    pc.lap("events");
    snprintf(ctx->name, sizeof(ctx->name), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    ctx->n_cus = prop.multiProcessorCount;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        int code = fail(nullptr, RT_ERR_NO_DEVICE, "device %d is %s; this library contains gfx950 code only", device_id, prop.gcnArchName);
        rt_ctx_destroy(ctx);
        return code;
    }
    *out = ctx;
    return RT_OK;
}

int rt_ctx_destroy(rt_ctx *ctx) {
    if (!ctx) return RT_OK;
    delete ctx;                                                      // ~rt_ctx waits for the context's streams, the members release themselves
    return RT_OK;
}

const char *rt_last_error(const rt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int rt_device_name(const rt_ctx *ctx, char *buf, size_t buflen) {
    if (!ctx || !buf || buflen == 0) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    snprintf(buf, buflen, "%s", ctx->name);
    return RT_OK;
}

int rt_scene_upload_meshes(rt_ctx *ctx, const rt_sphere *spheres, int n_spheres, const rt_mesh *meshes, int n_meshes,
                           const rt_light *light, const rt_camera *camera) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    ctx->have_scene = false;                                             // a call that fails, for whatever reason, leaves NO scene (install_scene sets it): what follows has dropped half of the old one
    ctx->parts_valid = false;                                            // (the per-mesh records describe the scene this call installs, or none)
    ctx->tex_mask = 0;                                                   // a new scene is untextured, also when this call fails
    ctx->snap_mask = 0;                                                  // ... and holds no vertex snapshot (rt_mesh_snapshot_vertices),
    ctx->nsnap_mask = 0; ctx->vnrm_mask = 0;                             // no normal snapshot and no computed vertex normals (rt_mesh_snapshot_normals, rt_mesh_compute_normals*)
    ctx->vcsr_valid = false;
    ctx->env_share = 0.f; ctx->env_total = 0;                            // ... draws no shadow rays towards one (rt_scene_set_environment_sampling)
    ctx->env_n = 0; ctx->env_rgb.clear();                                // ... and has no environment (rt_scene_set_environment; the buffer stays for the frames in flight; the still view: below)
    memset(ctx->emit_le, 0, sizeof(ctx->emit_le)); ctx->emit_mask = 0;    // ... and no mesh of it emits (rt_scene_set_emission; the buffer stays for the frames in flight),
    ctx->emit_total = 0; ctx->emit_dirty = false; ctx->emit_share = 0.5f; // the share at its default
    ctx->fresnel_mask = 0;                                               // ... and none of its objects is flagged (rt_material_set_fresnel)
    memset(ctx->gloss_alpha, 0, sizeof(ctx->gloss_alpha));               // ... and none has a roughness (rt_material_set_roughness)
    ctx->tint_mask = 0;                                                  // ... and none is tinted (rt_material_set_tint)
    ctx->still.shading_changed();
    ctx->still.mesh_changed();
    if (n_spheres < 0 || (n_spheres > 0 && !spheres)) return fail(ctx, RT_ERR_INVALID, "bad sphere array");
    if (n_meshes < 0 || (n_meshes > 0 && !meshes)) return fail(ctx, RT_ERR_INVALID, "bad mesh array");
    if (!light || !camera) return fail(ctx, RT_ERR_INVALID, "light/camera is NULL");
    const int n_objects = n_spheres + n_meshes;
    if (n_spheres > RT_MAX_SPHERES || n_objects > RT_MAX_OBJECTS)
        return fail(ctx, RT_ERR_INVALID, "at most %d objects (reference: Geometry* objects[10])", RT_MAX_OBJECTS);
    rtk::Scene sc{};
    // the meshes in object order; the spheres fill, in array order, the positions the meshes leave free (Scene::addObject numbers the objects as they come, cpu:539-542)
    std::vector<int> order(n_meshes);
    for (int k = 0; k < n_meshes; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return meshes[a].object_slot < meshes[b].object_slot; });
    bool taken[RT_MAX_OBJECTS] = {};
    for (int k = 0; k < n_meshes; ++k) {
        const rt_mesh &m = meshes[order[k]];
        if (m.object_slot < 0 || m.object_slot >= n_objects) return fail(ctx, RT_ERR_INVALID, "mesh object_slot %d outside [0,%d]", m.object_slot, n_objects - 1);
        if (taken[m.object_slot]) return fail(ctx, RT_ERR_INVALID, "two meshes at object_slot %d", m.object_slot);
        taken[m.object_slot] = true;
        sc.mesh[k] = rtk::MeshRec{0, m.object_slot};
        sc.obj_a[m.object_slot] = make_float4(0.f, 0.f, 0.f, __builtin_bit_cast(float, (int)(m.mirror ? 1 : 0)));
        sc.obj_b[m.object_slot] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], 0.f);
        // Geometry() (cpu:110) gives a mesh the indices 1 / 1; a zero-initialised rt_mesh (ABI 5 callers) says 0 / 0: the same diffuse object, stored as 1 / 1
        const bool unset = m.in_refraction_index == 0.f && m.out_refraction_index == 0.f;
        sc.obj_n[m.object_slot] = make_float2(unset ? 1.f : m.in_refraction_index, unset ? 1.f : m.out_refraction_index);
    }
    sc.n_meshes = n_meshes;
    int pos = 0;
    for (int i = 0; i < n_spheres; ++i) {
        while (pos < n_objects && taken[pos]) ++pos;
        put_sphere(sc, i, pos, spheres[i]);
        ++pos;
    }
    sc.n_spheres = n_spheres;
    sc.n_objects = n_objects;
    sc.mesh_slot = n_meshes > 0 ? sc.mesh[0].obj : -1;
    put_light(sc, *light);
    ctx->n_lights = 1;                                                   // the scene this call installs has the one uploaded light (rt_scene_set_lights)
    memset(ctx->light_radii, 0, sizeof(ctx->light_radii));               // ... a point (rt_scene_set_light_radii; the still view: shading_changed above)
    ctx->lens_radius = 0.f; ctx->lens_focus = 1.f;                       // ... seen through a pinhole (rt_camera_set_lens; the still view: mesh_changed above)
    ctx->shutter = rt_shutter{}; ctx->shutter_on = false;                // ... at one instant (rt_scene_set_shutter)
    sc.camx = camera->position[0]; sc.camy = camera->position[1]; sc.camz = camera->position[2]; sc.fov = camera->fov;

    PhaseClock pc;
    std::vector<int> real;                                               // meshes with something to traverse, in object order
    for (int k = 0; k < n_meshes; ++k) if (meshes[order[k]].n_triangles > 0 && meshes[order[k]].n_nodes > 0) real.push_back(order[k]);
    // the reference's own scenes hold one mesh (or none; a mesh without triangles is an object that is never hit, cpu:322-325)
    const int rc = install_meshes(ctx, sc, meshes, real, n_meshes > 0 ? &meshes[order[0]] : nullptr);
    pc.lap("rt_scene_upload (layouts, hipMalloc, copies)");
    return rc;
}

int rt_scene_upload(rt_ctx *ctx, const rt_sphere *spheres, int n_spheres, const rt_mesh *mesh,
                    const rt_light *light, const rt_camera *camera) {
    return rt_scene_upload_meshes(ctx, spheres, n_spheres, mesh, mesh ? 1 : 0, light, camera);
}

int rt_render_device(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, void *out_rgba_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    hipStream_t q_;
    if (int rc = call_stream(ctx, stream, q_); rc != RT_OK) return rc;
    return launch_render(ctx, p, rows, out_rgba_dev, q_);
}

int rt_render_device_batch(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, const rt_frame_desc *frames, int n_frames, void *stream) {
    return rt_render_device_batch_scenes(ctx, p, rows, frames, nullptr, 0, n_frames, stream);
}

int rt_render_device_batch_scenes(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, const rt_frame_desc *frames, const rt_frame_scene *scenes, int n_spheres,
                                  int n_frames, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    hipStream_t q_;
    if (int rc = call_stream(ctx, stream, q_); rc != RT_OK) return rc;
    if (!p || !rows || !frames) return fail(ctx, RT_ERR_INVALID, "params / rows / frames is NULL");
    if (n_frames < 1 || n_frames > RT_MAX_BATCH) return fail(ctx, RT_ERR_INVALID, "n_frames %d outside [1,%d]", n_frames, RT_MAX_BATCH);
    if (p->num_rays != 1) return fail(ctx, RT_ERR_UNSUPPORTED, "a batch renders one sample per pixel and frame (num_rays = %d)", p->num_rays);
    if (p->width <= 0 || p->height <= 0) return fail(ctx, RT_ERR_INVALID, "width/height must be positive");
    if (scenes && ctx->have_scene && n_spheres != ctx->scene.n_spheres)
        return fail(ctx, RT_ERR_INVALID, "n_spheres %d is not the uploaded scene's %d", n_spheres, ctx->scene.n_spheres);
    // the frames' own lights and sphere poses as the store kernel takes them (rt_frame_scene and rtk::AnimSrc are the same 16 + 16 * RT_MAX_SPHERES bytes)
    static_assert(sizeof(rt_frame_scene) == sizeof(rtk::AnimSrc) && RT_MAX_SPHERES == rtk::kMaxSpheres, "rt_frame_scene is copied into rtk::AnimSrc");
    std::vector<rtk::AnimSrc> anim(scenes ? n_frames : 0);
    if (scenes) memcpy(anim.data(), scenes, anim.size() * sizeof(rtk::AnimSrc));
    rtk::Batch bt{};
    bt.n = n_frames;
    const uint8_t *lo = nullptr, *hi = nullptr;
    const size_t bytes = (size_t)std::max(rows->n_rows, 0) * p->width * sizeof(float4);
    for (int k = 0; k < n_frames; ++k) {
        const rt_frame_desc &f = frames[k];
        if (!f.out_rgba_dev) return fail(ctx, RT_ERR_INVALID, "frame %d: output pointer is NULL", k);
        const uint8_t *o = static_cast<const uint8_t *>(f.out_rgba_dev);
        for (int j = 0; j < k; ++j) {
            const uint8_t *oj = static_cast<const uint8_t *>(frames[j].out_rgba_dev);
            if (o < oj + bytes && oj < o + bytes) return fail(ctx, RT_ERR_INVALID, "frames %d and %d render into overlapping buffers", j, k);
        }
        lo = (!lo || o < lo) ? o : lo; hi = (!hi || o + bytes > hi) ? o + bytes : hi;
        // cpu:694 `-W / (2 * tan(alpha/2))` for this frame's camera (evaluated as make_frame evaluates the uploaded camera's)
        bt.f[k] = rtk::BatchFrame{f.camera.position[0], f.camera.position[1], f.camera.position[2],
                                  -(float)p->width / (2 * (float)std::tan((double)(f.camera.fov / 2))), f.seed, 0, static_cast<float4 *>(f.out_rgba_dev)};
    }
    // one chunk: the batch exists for SMALL shares (a share too big for one chunk fills the chip by itself: render its frames one by one)
    const BetweenGuard between = begin_render_call(ctx->pipe, lo, hi);   // (the frames' buffers and whatever lies between them: conservative for the pipelining rule)
    return launch_render_chunk(ctx, p, rows, frames[0].out_rgba_dev, q_, nullptr, nullptr, true, true, &bt, scenes ? anim.data() : nullptr);
}

int rt_render(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, float *out_rgba_host) {
    rt_rows rows; int64_t npix;
    int rc = host_rows(ctx, p, row_begin, row_end, out_rgba_host, rows, npix);
    if (rc != RT_OK) return rc;
    if ((rc = launch_render(ctx, p, &rows, ctx->scratch_rgba.p, own_stream(ctx))) != RT_OK) return rc;
    return copy_back(ctx, out_rgba_host, ctx->scratch_rgba.p, (size_t)npix * sizeof(float4));
}

int rt_ctx_set_pipelining(rt_ctx *ctx, int on) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    ctx->pipe.on = on != 0;
    ctx->pipe.valid = false;
    return RT_OK;
}

int rt_stats_enable(rt_ctx *ctx, int on) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    ctx->stats_on = on != 0;
    return RT_OK;
}

int rt_render_async(rt_ctx *ctx, const rt_params *p, int slot, void *out_host, int rgb8) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!p) return fail(ctx, RT_ERR_INVALID, "params is NULL");
    if (slot < 0 || slot >= rt_ctx::kSlots) return fail(ctx, RT_ERR_INVALID, "slot %d outside [0,%d)", slot, rt_ctx::kSlots);
    if (!out_host) return fail(ctx, RT_ERR_INVALID, "output pointer is NULL");
    if (p->width <= 0 || p->height <= 0) return fail(ctx, RT_ERR_INVALID, "width/height must be positive");
    const int64_t npix = (int64_t)p->width * p->height;
    int rc = ensure(ctx, ctx->slot_rgba[slot], (size_t)npix * sizeof(float4));
    if (rc != RT_OK) return rc;
    if (rgb8 && (rc = ensure(ctx, ctx->slot_rgb8[slot], (size_t)npix * 3 + 16)) != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // the slot's previous frame may still be on its way to the host: the kernels that overwrite its device buffer wait for that copy
    if (ctx->slot_pending[slot]) RT_HIP(ctx, hipStreamWaitEvent(own_stream(ctx), ctx->slot_done[slot], 0));
    rt_rows rows{0, p->height, p->height, 1};
    // frames alternate between the two slots: with the sub-frames' chains on their own streams frame k+1 follows frame k chain by chain
    // (start_chains); what its kernels must not overtake -- the slot's previous copy -- is handed to the chains directly
    const bool pipe_was = ctx->pipe.on;
    ctx->pipe.on = ctx->knobs.async_pipeline != 0;
    ctx->pipe.extra_wait = ctx->slot_pending[slot] ? ctx->slot_done[slot] : nullptr;
    rc = launch_render(ctx, p, &rows, ctx->slot_rgba[slot].p, own_stream(ctx));
    ctx->pipe.on = pipe_was;
    ctx->pipe.extra_wait = nullptr;
    if (rc != RT_OK) return rc;
    if (rgb8 && (rc = launch_tonemap(ctx, ctx->slot_rgba[slot].p, npix, ctx->slot_rgb8[slot].p, own_stream(ctx))) != RT_OK) return rc;
    RT_HIP(ctx, hipEventRecord(ctx->slot_rendered[slot], own_stream(ctx)));
    if ((rc = need_copy_streams(ctx, ctx->knobs.copy_split != 0)) != RT_OK) return rc;
    // the copy runs on its own stream: the next frame's kernels (other slot) do not queue behind it
    RT_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->slot_rendered[slot], 0));
    const size_t bytes = rgb8 ? (size_t)npix * 3 : (size_t)npix * sizeof(float4);
    const uint8_t *src = static_cast<const uint8_t *>(rgb8 ? ctx->slot_rgb8[slot].p : ctx->slot_rgba[slot].p);
    const size_t half = ctx->knobs.copy_split && bytes >= (4u << 20) ? (bytes / 2 + 4095) / 4096 * 4096 : bytes;   // big frames: two halves on two copy streams
    RT_HIP(ctx, hipMemcpyAsync(out_host, src, half, hipMemcpyDeviceToHost, ctx->copy_stream));
    if (half < bytes) {
        RT_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream2, ctx->slot_rendered[slot], 0));
        RT_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(out_host) + half, src + half, bytes - half, hipMemcpyDeviceToHost, ctx->copy_stream2));
        RT_HIP(ctx, hipEventRecord(ctx->slot_half[slot], ctx->copy_stream2));
        RT_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->slot_half[slot], 0));
    }
    RT_HIP(ctx, hipEventRecord(ctx->slot_done[slot], ctx->copy_stream));
    ctx->slot_pending[slot] = true;
    return RT_OK;
}

int rt_wait(rt_ctx *ctx, int slot) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (slot < 0 || slot >= rt_ctx::kSlots) return fail(ctx, RT_ERR_INVALID, "slot %d outside [0,%d)", slot, rt_ctx::kSlots);
    if (!ctx->slot_pending[slot]) return fail(ctx, RT_ERR_INVALID, "slot %d has no frame in flight", slot);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipEventSynchronize(ctx->slot_done[slot]));
    ctx->slot_pending[slot] = false;
    return RT_OK;
}

int rt_tonemap_device(rt_ctx *ctx, const void *rgba_dev, int64_t n_pixels, void *rgb8_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    hipStream_t q_;
    if (int rc = call_stream(ctx, stream, q_); rc != RT_OK) return rc;
    return launch_tonemap(ctx, rgba_dev, n_pixels, rgb8_dev, q_);
}

int rt_render_rgb8(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, uint8_t *out_rgb8_host) {
    PhaseClock pc;
    rt_rows rows; int64_t npix;
    int rc = host_rows(ctx, p, row_begin, row_end, out_rgb8_host, rows, npix);
    if (rc != RT_OK) return rc;
    if ((rc = ensure(ctx, ctx->scratch_rgb8, (size_t)npix * 3 + 16)) != RT_OK) return rc;
    pc.lap("rt_render_rgb8: frame buffers (hipMalloc)");
    if ((rc = launch_render(ctx, p, &rows, ctx->scratch_rgba.p, own_stream(ctx))) != RT_OK) return rc;
    pc.lap("rt_render_rgb8: enqueue (path state, code object)");
    if ((rc = launch_tonemap(ctx, ctx->scratch_rgba.p, npix, ctx->scratch_rgb8.p, own_stream(ctx))) != RT_OK) return rc;
    if (pc.on) { RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx))); pc.lap("rt_render_rgb8: kernels (wait)"); }
    if ((rc = copy_back(ctx, out_rgb8_host, ctx->scratch_rgb8.p, (size_t)npix * 3)) != RT_OK) return rc;
    pc.lap("rt_render_rgb8: copy to the host");
    return RT_OK;
}

int rt_count_work(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, rt_work *out) {
    rt_rows rows; int64_t npix;
    int rc = host_rows(ctx, p, row_begin, row_end, out, rows, npix);
    if (rc != RT_OK) return rc;
    if ((rc = ensure(ctx, ctx->work, 24 * sizeof(unsigned long long))) != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipMemsetAsync(ctx->work.p, 0, 24 * sizeof(unsigned long long), own_stream(ctx)));
    rc = launch_render(ctx, p, &rows, ctx->scratch_rgba.p, own_stream(ctx), static_cast<unsigned long long *>(ctx->work.p));
    if (rc != RT_OK) return rc;
    unsigned long long h[24];
    RT_HIP(ctx, hipMemcpyAsync(h, ctx->work.p, sizeof(h), hipMemcpyDeviceToHost, own_stream(ctx)));
    std::vector<float> fb((size_t)npix * 4);
    if ((rc = copy_back(ctx, fb.data(), ctx->scratch_rgba.p, fb.size() * sizeof(float))) != RT_OK) return rc;
    double rays = 0;                                  // .w of every pixel = rays traced for it (exact in binary32)
    for (size_t k = 3; k < fb.size(); k += 4) rays += fb[k];
    out->rays = (uint64_t)rays; out->box_tests = h[1]; out->nodes = h[2]; out->tri_tests = h[3];
    out->box_literal = h[5]; out->tri_literal = h[6];
    for (int k = 0; k < 12; ++k) out->steps[k] = h[8 + k];
    for (int k = 0; k < 4; ++k) ctx->dead_counts[k] = h[20 + k];
    ctx->dead_last_count = h[7];
    // the counting instantiation checks every index that reaches an address (rt_travq.hip.h WQ_CHECK, rt_path.hip.h)
    if (h[4] != 0) return fail(ctx, RT_ERR_INTERNAL, "traversal invariant violated (mask 0x%llx: 1 path, 2 triangle, 4 node, 8 stack, 16 leaf queue, 32 staging)", h[4]);
    return RT_OK;
}

int rt_dead_channel_counts(rt_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return fail(ctx, RT_ERR_INVALID, "bad arguments");
    for (int k = 0; k < 4; ++k) out[k] = ctx->dead_counts[k];
    return RT_OK;
}

int rt_dead_last_count(rt_ctx *ctx, uint64_t *out) {
    if (!ctx || !out) return fail(ctx, RT_ERR_INVALID, "bad arguments");
    *out = ctx->dead_last_count;
    return RT_OK;
}

#include "rt_host_mesh.hip.h"     // rt_mesh_set_normals / transform / rebuild (reference tree, LBVH)
#include "rt_host_tex.hip.h"      // rt_mesh_set_texture[_of]
#include "rt_host_edit.hip.h"     // rt_scene_get / set / move: the light and the spheres of the scene in use

// the four counters of one level of the still view (rt_still.h StillLevel::counts)
static int still_counts(const rt_ctx *ctx, rtk::StillLevel rtk::StillView::*level, uint64_t out[4]) {
    if (!ctx || !out) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    for (int k = 0; k < 4; ++k) out[k] = (ctx->still.*level).counts[k];
    return RT_OK;
}
int rt_first_hit_cache_counts(const rt_ctx *ctx, uint64_t out[4]) { return still_counts(ctx, &rtk::StillView::hit, out); }
int rt_first_shadow_cache_counts(const rt_ctx *ctx, uint64_t out[4]) { return still_counts(ctx, &rtk::StillView::shadow, out); }
int rt_first_shade_cache_counts(const rt_ctx *ctx, uint64_t out[4]) { return still_counts(ctx, &rtk::StillView::records, out); }

int rt_camera_basis(const rt_camera_pose *pose, float bx[3], float by[3], float bz[3]) {
    if (!pose || !bx || !by || !bz) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    camera_basis(pose->yaw, pose->pitch, bx, by, bz);
    return RT_OK;
}

int rt_render_pose(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, float *out_rgba_host) {
    rt_rows rows; int64_t npix;
    int rc = host_rows(ctx, p, 0, p ? p->height : 0, out_rgba_host, rows, npix);
    if (rc != RT_OK) return rc;
    if (!pose) return fail(ctx, RT_ERR_INVALID, "pose is NULL");
    if ((rc = launch_render(ctx, p, &rows, ctx->scratch_rgba.p, own_stream(ctx), nullptr, pose)) != RT_OK) return rc;
    return copy_back(ctx, out_rgba_host, ctx->scratch_rgba.p, (size_t)npix * sizeof(float4));
}

int rt_render_pose_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, void *out_rgba_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    hipStream_t q_;
    if (int rc = call_stream(ctx, stream, q_); rc != RT_OK) return rc;
    if (!pose) return fail(ctx, RT_ERR_INVALID, "pose is NULL");
    return launch_render(ctx, p, rows, out_rgba_dev, q_, nullptr, pose);
}

// ---- adaptive sampling (rt_adaptive.hip.h; the launches: rt_host_render.hip.h) ----
static int counts_check(rt_ctx *ctx, const rt_params *p, const void *counts, const void *base, const void *out) {
    if (!p || !counts || !out) return fail(ctx, RT_ERR_INVALID, "params / counts / out is NULL");
    if (p->width <= 0 || p->height <= 0) return fail(ctx, RT_ERR_INVALID, "width/height must be positive");
    const size_t npix = (size_t)p->width * p->height;
    if (overlaps(out, npix * sizeof(float4), counts, npix)) return fail(ctx, RT_ERR_INVALID, "the output overlaps the counts");
    if (base && base != out && overlaps(out, npix * sizeof(float4), base, npix * sizeof(float4))) return fail(ctx, RT_ERR_INVALID, "base must be the output itself or clear of it");
    return RT_OK;
}

int rt_render_counts_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const uint8_t *counts_dev, const void *base_rgba_dev, void *out_rgba_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = counts_check(ctx, p, counts_dev, base_rgba_dev, out_rgba_dev); rc != RT_OK) return rc;
    hipStream_t q_;
    if (int rc = call_stream(ctx, stream, q_); rc != RT_OK) return rc;
    return launch_render_counts(ctx, p, pose, counts_dev, base_rgba_dev, out_rgba_dev, q_);
}

int rt_render_counts(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const uint8_t *counts_host, const float *base_rgba_host, float *out_rgba_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (int rc = counts_check(ctx, p, counts_host, base_rgba_host, out_rgba_host); rc != RT_OK) return rc;
    const size_t npix = (size_t)p->width * p->height, frame = npix * sizeof(float4);
    // the frame (base staged into it: the device form runs in place), then the counts
    return staged(ctx, {{base_rgba_host, frame}, {counts_host, npix}}, 0, frame, out_rgba_host, [&](uint8_t *d) {
        return rt_render_counts_device(ctx, p, pose, d + frame, base_rgba_host ? d : nullptr, d, nullptr);
    });
}

int rt_render_counts_info(const rt_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    for (int k = 0; k < 4; ++k) out[k] = ctx->ad_info[k];
    return RT_OK;
}

static int sample_counts_check(rt_ctx *ctx, const void *history, int width, int height, const rt_sample_count_params *cp, const void *counts) {
    if (!history || !cp || !counts) return fail(ctx, RT_ERR_INVALID, "history / params / counts is NULL");
    if (int rc = check_frame_size(ctx, width, height); rc != RT_OK) return rc;
    if (cp->max_samples < 1 || cp->max_samples > RT_MAX_SAMPLE_COUNT) return fail(ctx, RT_ERR_INVALID, "max_samples %d outside [1,%d]", cp->max_samples, RT_MAX_SAMPLE_COUNT);
    if (cp->new_surface_samples < 1 || cp->new_surface_samples > cp->max_samples)
        return fail(ctx, RT_ERR_INVALID, "new_surface_samples %d outside [1, max_samples = %d]", cp->new_surface_samples, cp->max_samples);
    if (cp->short_history < 0) return fail(ctx, RT_ERR_INVALID, "short_history %d < 0", cp->short_history);
    return RT_OK;
}

int rt_sample_counts_device(rt_ctx *ctx, const void *history_dev, int width, int height, const rt_sample_count_params *cp, uint8_t *counts_dev, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = sample_counts_check(ctx, history_dev, width, height, cp, counts_dev);
    if (rc != RT_OK) return rc;
    const size_t npix = (size_t)width * height;
    if (overlaps(counts_dev, npix, history_dev, 2 * npix * sizeof(float4))) return fail(ctx, RT_ERR_INVALID, "the counts overlap the history");
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    const rtk::SampleCountArgs a{(float)(cp->max_samples - 1), (float)cp->short_history, (float)(cp->new_surface_samples - 1), cp->k_rel, cp->lum_floor};
    note_between(ctx, q, {{history_dev, 2 * npix * sizeof(float4)}, {counts_dev, npix}});
    hipLaunchKernelGGL(rtk::sample_counts_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, q, static_cast<const float4 *>(history_dev) + npix, (int64_t)npix, a, counts_dev);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int rt_sample_counts(rt_ctx *ctx, const float *history_host, int width, int height, const rt_sample_count_params *cp, uint8_t *counts_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (int rc = sample_counts_check(ctx, history_host, width, height, cp, counts_host); rc != RT_OK) return rc;
    const size_t npix = (size_t)width * height, hist = 2 * npix * sizeof(float4);
    return staged(ctx, {{history_host, hist}}, hist, npix, counts_host, [&](uint8_t *d) { return rt_sample_counts_device(ctx, d, width, height, cp, d + hist, nullptr); });
}

int rt_kat_sample_plan(rt_ctx *ctx, const uint8_t *counts_host, int width, int height, int first_sample, uint32_t *offs_out, int32_t *items_out, uint64_t *n_items_out,
                       int32_t span_out[2]) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!counts_host || !n_items_out) return fail(ctx, RT_ERR_INVALID, "counts / n_items_out is NULL");
    if (width <= 0 || height <= 0) return fail(ctx, RT_ERR_INVALID, "width/height must be positive");
    if (first_sample < 0 || first_sample > 1) return fail(ctx, RT_ERR_INVALID, "first_sample must be 0 or 1");
    if (span_out) { span_out[0] = rtk::kPlanBlock; span_out[1] = rtk::kPlanBlock * rtk::kPlanLevel; }
    RT_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf dc;
    int rc = upload(ctx, dc, counts_host, (size_t)width * height);
    if (rc != RT_OK) return rc;
    rtk::PlanArgs pa;
    uint64_t total = 0;
    if ((rc = plan_samples(ctx, static_cast<const uint8_t *>(dc.p), width, height, first_sample, true, own_stream(ctx), pa, total)) != RT_OK) return rc;
    *n_items_out = total;
    if (offs_out) RT_HIP(ctx, hipMemcpyAsync(offs_out, ctx->adOffs.p, ((size_t)pa.n_slots + 1) * 4, hipMemcpyDeviceToHost, own_stream(ctx)));
    std::vector<uint32_t> rec(items_out ? total : 0);
    if ((rc = copy_back(ctx, rec.data(), ctx->adItems.p, rec.size() * 4)) != RT_OK) return rc;
    for (size_t k = 0; k < rec.size(); ++k) {                           // decoded: (x, y, sample)
        const int slot = (int)(rec[k] >> rtk::kItemShift), tile = slot >> 6, q = slot & 63;
        items_out[3 * k] = (tile % pa.tiles_x) * 8 + (q & 7);
        items_out[3 * k + 1] = (tile / pa.tiles_x) * 8 + (q >> 3);
        items_out[3 * k + 2] = (int32_t)(rec[k] & 63u);
    }
    return RT_OK;
}

int rt_progressive_reset(rt_ctx *ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    ctx->prog_frames = 0;                                             // buffer_reset, realtime:1246-1251
    return RT_OK;
}

int rt_progressive_frames(const rt_ctx *ctx, int *frames) {
    if (!ctx || !frames) return fail(nullptr, RT_ERR_INVALID, "bad arguments");
    *frames = ctx->prog_frames;
    return RT_OK;
}

int rt_progressive_frame(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, float *display_rgba_host, uint8_t *rgb8_host) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!p || !pose) return fail(ctx, RT_ERR_INVALID, "params/pose is NULL");
    if (p->width <= 0 || p->height <= 0) return fail(ctx, RT_ERR_INVALID, "width/height must be positive");
    const int64_t npix = (int64_t)p->width * p->height;
    const size_t bytes = (size_t)npix * sizeof(float4);
    int rc;
    if ((rc = ensure(ctx, ctx->scratch_rgba, bytes)) != RT_OK || (rc = ensure(ctx, ctx->accum, 2 * bytes)) != RT_OK ||
        (rc = ensure(ctx, ctx->scratch_rgb8, (size_t)npix * 3 + 16)) != RT_OK)
        return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->prog_frames == 0 || ctx->prog_w != p->width || ctx->prog_h != p->height) {   // realtime:1246-1251 (a new size also resets)
        RT_HIP(ctx, hipMemsetAsync(ctx->accum.p, 0, bytes, own_stream(ctx)));
        ctx->prog_frames = 0; ctx->prog_w = p->width; ctx->prog_h = p->height;
    }
    const int frame_no = ctx->prog_frames + 1;                        // frames++, realtime:1253
    rt_params q = *p;
    uint32_t a = (uint32_t)frame_no;                                  // WangHash(frames), realtime:1190-1197, seeds the frame's RNG
    a = (a ^ 61u) ^ (a >> 16); a = a + (a << 3); a = a ^ (a >> 4); a = a * 0x27d4eb2du; a = a ^ (a >> 15);
    q.seed = a;
    rt_rows rows{0, p->height, p->height, 1};
    if ((rc = launch_render(ctx, &q, &rows, ctx->scratch_rgba.p, own_stream(ctx), nullptr, pose)) != RT_OK) return rc;
    float4 *accum = static_cast<float4 *>(ctx->accum.p), *display = accum + npix;
    hipLaunchKernelGGL(rtk::accumulate_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, own_stream(ctx),
                       static_cast<const float4 *>(ctx->scratch_rgba.p), accum, display, static_cast<uint8_t *>(ctx->scratch_rgb8.p), npix, frame_no);
    RT_HIP(ctx, hipGetLastError());
    ctx->prog_frames = frame_no;
    if (display_rgba_host) RT_HIP(ctx, hipMemcpyAsync(display_rgba_host, display, bytes, hipMemcpyDeviceToHost, own_stream(ctx)));
    return copy_back(ctx, rgb8_host, ctx->scratch_rgb8.p, rgb8_host ? (size_t)npix * 3 : 0);
}

// accumulate_kernel itself on the caller's values: buffers of the call's own, so no scene is needed and the context's progressive state is not touched.  The bytes land
// between two guards of 16 bytes of 0xA5 on the device, which must come back as they were.
int rt_kat_progressive(rt_ctx *ctx, const float *accum_in, const float *frame, int n, int framenumber, float *accum_out, float *display_out, uint8_t *rgb8_out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (n < 0 || framenumber < 1 || (n > 0 && (!accum_in || !frame))) return fail(ctx, RT_ERR_INVALID, "bad KAT arguments");
    if (n == 0) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * sizeof(float4), guard = 16, nb = (size_t)n * 3;
    DevBuf dacc, dfr, ddisp, d8;
    int rc;
    if ((rc = upload(ctx, dacc, accum_in, bytes)) != RT_OK || (rc = upload(ctx, dfr, frame, bytes)) != RT_OK || (rc = ensure(ctx, ddisp, bytes)) != RT_OK ||
        (rc = ensure(ctx, d8, nb + 2 * guard)) != RT_OK)
        return rc;
    RT_HIP(ctx, hipMemsetAsync(d8.p, 0xA5, nb + 2 * guard, own_stream(ctx)));
    hipLaunchKernelGGL(rtk::accumulate_kernel, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, own_stream(ctx), static_cast<const float4 *>(dfr.p),
                       static_cast<float4 *>(dacc.p), static_cast<float4 *>(ddisp.p), static_cast<uint8_t *>(d8.p) + guard, (int64_t)n, framenumber);
    RT_HIP(ctx, hipGetLastError());
    if (accum_out) RT_HIP(ctx, hipMemcpyAsync(accum_out, dacc.p, bytes, hipMemcpyDeviceToHost, own_stream(ctx)));
    if (display_out) RT_HIP(ctx, hipMemcpyAsync(display_out, ddisp.p, bytes, hipMemcpyDeviceToHost, own_stream(ctx)));
    std::vector<uint8_t> h8(nb + 2 * guard);
    if ((rc = copy_back(ctx, h8.data(), d8.p, h8.size())) != RT_OK) return rc;
    for (size_t k = 0; k < guard; ++k)
        if (h8[k] != 0xA5 || h8[guard + nb + k] != 0xA5) return fail(ctx, RT_ERR_INTERNAL, "accumulate_kernel wrote outside its %zu bytes", nb);
    if (rgb8_out) memcpy(rgb8_out, h8.data() + guard, nb);
    return RT_OK;
}

int rt_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return fail(nullptr, RT_ERR_INVALID, "ptr is NULL");
    *ptr = nullptr;
    hipError_t e = hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) { *ptr = nullptr; return fail(nullptr, RT_ERR_HIP, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    return RT_OK;
}

int rt_host_free(void *ptr) {
    if (!ptr) return RT_OK;
    hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess) return fail(nullptr, RT_ERR_HIP, "hipHostFree: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_ctx_selfcheck(rt_ctx *ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    for (const DevBuf *b : ctx->bufs) {
        if (!b->p) continue;
        hipPointerAttribute_t at{};
        RT_HIP(ctx, hipPointerGetAttributes(&at, b->p));
        if (at.device != ctx->device) return fail(ctx, RT_ERR_INTERNAL, "a buffer of the context of device %d lives on device %d", ctx->device, at.device);
    }
    return RT_OK;
}

int rt_device_alloc(rt_ctx *ctx, void **ptr, size_t bytes) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!ptr) return fail(ctx, RT_ERR_INVALID, "ptr is NULL");
    *ptr = nullptr;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(ptr, bytes ? bytes : 16);
    if (e != hipSuccess) { *ptr = nullptr; return fail(ctx, RT_ERR_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    return RT_OK;
}

int rt_device_free(void *ptr) {
    if (!ptr) return RT_OK;
    hipError_t e = hipFree(ptr);
    if (e != hipSuccess) return fail(nullptr, RT_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_device_to_host(rt_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (bytes && (!dst_host || !src_dev)) return fail(ctx, RT_ERR_INVALID, "bad copy arguments");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return copy_back(ctx, dst_host, src_dev, bytes);
}

int rt_synchronize(rt_ctx *ctx) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));
    return RT_OK;
}

int rt_get_stats(rt_ctx *ctx, rt_stats *stats) {
    if (!ctx || !stats) return fail(ctx, RT_ERR_INVALID, "bad arguments");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    ctx->stats.kernel_ms = 0.f;
    ctx->stats.tonemap_ms = 0.f;
    ctx->stats.trav_ms = 0.f;
    ctx->stats.trav_launches = 0;
    ctx->stats.adv_ms = 0.f; ctx->stats.adv_launches = 0; ctx->stats.adv_paths = 0;
    if (ctx->have_kernel_time) {
        RT_HIP(ctx, hipEventSynchronize(ctx->ev_k1));
        RT_HIP(ctx, hipEventElapsedTime(&ctx->stats.kernel_ms, ctx->ev_k0, ctx->ev_k1));
        for (int k = 0; k < ctx->n_trav_events; ++k) {
            float ms = 0.f;
            RT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_trav[2 * k], ctx->ev_trav[2 * k + 1]));
            ctx->stats.trav_ms += ms;
        }
        ctx->stats.trav_launches = ctx->n_trav_events;
        for (int k = 0; k < ctx->n_adv_events; ++k) {
            float ms = 0.f;
            RT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_adv[2 * k], ctx->ev_adv[2 * k + 1]));
            ctx->stats.adv_ms += ms;
        }
        ctx->stats.adv_launches = ctx->n_adv_events;
        ctx->stats.adv_paths = ctx->adv_paths;
    }
    if (ctx->have_tonemap_time) {
        RT_HIP(ctx, hipEventSynchronize(ctx->ev_t1));
        RT_HIP(ctx, hipEventElapsedTime(&ctx->stats.tonemap_ms, ctx->ev_t0, ctx->ev_t1));
    }
    *stats = ctx->stats;
    return RT_OK;
}

}  // extern "C"

#include "rt_multi.hip.h"
#include "rt_kat.hip.h"
#include "rt_trace.hip.h"
#include "rt_aov.hip.h"           // the order matters from here on: each of the next three uses what the one before it defines (their headers say what)
#include "rt_aov_surface.hip.h"
#include "rt_denoise.hip.h"
#include "rt_temporal.hip.h"
#include "rt_demodulate.hip.h"
#include "rt_upsample.hip.h"
#include "rt_rectify.hip.h"        // after rt_temporal.hip.h: it clamps the history that rt_temporal_accumulate_fast writes
