// rt_host_edit.hip.h -- the light and the spheres of the scene in use, edited in place: MoveLightSource / MoveObject of realtime_render.cu:1072-1098 and the
// general set / get they are instances of.  The light and the spheres live in rtk::Scene alone -- a kernel argument, copied at every launch (make_frame) -- so an edit is a
// host-side store into ctx->scene: no device memory is touched, nothing derived from a mesh is looked at, and a frame already enqueued keeps the values its launches captured.
// Included inside rt_capi.hip's extern "C" block.

static int edit_scene_check(rt_ctx *ctx) {
    if (!ctx->have_scene || !ctx->parts_valid) return fail(ctx, RT_ERR_NO_SCENE, "no scene: rt_scene_upload* has not been called or the last call failed");
    return RT_OK;
}
// index into Scene::sph of the sphere at position object_slot of Scene::objects; -1: outside the scene, or a mesh's position
static int sphere_at(const rtk::Scene &sc, int object_slot) {
    for (int k = 0; k < sc.n_spheres; ++k) if (sc.sph[k].obj == object_slot) return k;
    return -1;
}

int rt_light_orbit(const rt_light *in, float angular_speed, float dt, rt_light *out) {
    if (!in || !out) return fail(nullptr, RT_ERR_INVALID, "light in / out is NULL");
    // realtime:1078-1088 with C = (0, 0, 0), every operation in binary32 in the order written there (powf(x, 2) = x * x)
    const float Cx = 0.f, Cz = 0.f;
    const float dx = Cx - in->position[0], dz = Cz - in->position[2];
    const float radius = sqrtf(dx * dx + dz * dz);
    const float current = atan2f(in->position[2] - Cz, in->position[0] - Cx);
    const float angle = current + angular_speed * dt;
    rt_light l = *in;
    l.position[0] = Cx + radius * cosf(angle);
    l.position[2] = Cz + radius * sinf(angle);
    *out = l;
    return RT_OK;
}

int rt_scene_get_light(const rt_ctx *ctx, rt_light *out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);                               // (the error text is the only thing written)
    if (!out) return fail(c, RT_ERR_INVALID, "out is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    const rtk::Scene &sc = ctx->scene;
    *out = rt_light{{sc.Lx, sc.Ly, sc.Lz}, sc.intensity};
    return RT_OK;
}

// The radii of the list (raytrace_hip.h "soft shadows") become these n, the rest 0.  A radius that changes is a light change for the still view: which levels a chain may
// keep depends on it, and the shadow words of a point light are not a shell's.
static void put_radii(rt_ctx *ctx, const float *radii, int n) {
    bool changed = false;
    for (int k = 0; k < RT_MAX_LIGHTS; ++k) {
        const float r = k < n ? radii[k] : 0.f;
        changed = changed || memcmp(&r, &ctx->light_radii[k], sizeof(float)) != 0;
        ctx->light_radii[k] = r;
    }
    if (changed) ctx->still.shading_changed();
}
// the list becomes this one light; keep_radius: it is the light that was there, moved or edited (a lamp that moves keeps its size) -- otherwise a new light, a point
static int set_one_light(rt_ctx *ctx, const rt_light *light, bool keep_radius) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!light) return fail(ctx, RT_ERR_INVALID, "light is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    put_light(ctx->scene, *light);
    ctx->n_lights = 1;                                                   // the list is this one light
    put_radii(ctx, ctx->light_radii, keep_radius ? 1 : 0);
    return RT_OK;
}

int rt_scene_set_light(rt_ctx *ctx, const rt_light *light) { return set_one_light(ctx, light, false); }

// ---- several point lights (raytrace_hip.h "several point lights"): the list is host state too; a frame's launches capture the table make_frame derives from it ----
// prefix[0] = I_0, prefix[k] = fl(prefix[k - 1] + I_k): one binary32 addition each (-ffp-contract=off), in index order
static_assert(RT_MAX_LIGHTS == rtk::kMaxLights, "rtk::WfLights holds RT_MAX_LIGHTS lights");
static void light_prefix(const rt_light *lights, int n, float *prefix) {
    for (int k = 0; k < n; ++k) prefix[k] = k == 0 ? lights[0].intensity : prefix[k - 1] + lights[k].intensity;
}
// what a list of several must satisfy for the pick to be defined: non-negative finite intensities (sign bit clear: no -0), a finite total above 0
static int lights_check(rt_ctx *ctx, const rt_light *lights, int n) {
    float prefix[RT_MAX_LIGHTS];
    for (int k = 0; k < n; ++k) {
        const float I = lights[k].intensity;
        if (std::signbit(I) || !std::isfinite(I)) return fail(ctx, RT_ERR_INVALID, "light %d: intensity %g has its sign bit set or is not finite", k, (double)I);
    }
    light_prefix(lights, n, prefix);
    if (!std::isfinite(prefix[n - 1]) || prefix[n - 1] == 0.f) return fail(ctx, RT_ERR_INVALID, "the lights' total intensity %g is not finite or is 0", (double)prefix[n - 1]);
    return RT_OK;
}
// the list becomes these n lights (checked by the caller)
static void put_lights(rt_ctx *ctx, const rt_light *lights, int n) {
    rt_light tmp[RT_MAX_LIGHTS];
    memcpy(tmp, lights, (size_t)n * sizeof(rt_light));                   // (lights may point into ctx->lights)
    memcpy(ctx->lights, tmp, (size_t)n * sizeof(rt_light));
    put_light(ctx->scene, tmp[0]);
    ctx->n_lights = n;
}

int rt_scene_set_lights(rt_ctx *ctx, const rt_light *lights, int n) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!lights) return fail(ctx, RT_ERR_INVALID, "lights is NULL");
    if (n < 1 || n > RT_MAX_LIGHTS) return fail(ctx, RT_ERR_INVALID, "n %d outside [1,%d]", n, RT_MAX_LIGHTS);
    if (n == 1) return rt_scene_set_light(ctx, lights);                  // one light: whatever rt_scene_set_light accepts
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (int rc = lights_check(ctx, lights, n); rc != RT_OK) return rc;
    put_lights(ctx, lights, n);
    put_radii(ctx, nullptr, 0);                                          // new lights: points
    return RT_OK;
}

int rt_scene_get_lights(const rt_ctx *ctx, rt_light *out, int cap, int *n) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!n) return fail(c, RT_ERR_INVALID, "n is NULL");
    if (cap < 0 || (cap > 0 && !out)) return fail(c, RT_ERR_INVALID, "out is NULL with cap %d", cap);
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    *n = ctx->n_lights;
    if (cap == 0) return RT_OK;                                          // the count alone
    if (cap < ctx->n_lights) return fail(c, RT_ERR_INVALID, "cap %d is below the scene's %d lights", cap, ctx->n_lights);
    if (ctx->n_lights == 1) return rt_scene_get_light(ctx, out);
    memcpy(out, ctx->lights, (size_t)ctx->n_lights * sizeof(rt_light));
    return RT_OK;
}

int rt_scene_set_light_at(rt_ctx *ctx, int k, const rt_light *light) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!light) return fail(ctx, RT_ERR_INVALID, "light is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (k < 0 || k >= ctx->n_lights) return fail(ctx, RT_ERR_INVALID, "light %d outside the scene's %d", k, ctx->n_lights);
    if (ctx->n_lights == 1) return set_one_light(ctx, light, true);
    rt_light l[RT_MAX_LIGHTS];
    memcpy(l, ctx->lights, sizeof(l));
    l[k] = *light;
    if (int rc = lights_check(ctx, l, ctx->n_lights); rc != RT_OK) return rc;
    put_lights(ctx, l, ctx->n_lights);
    return RT_OK;
}

int rt_scene_move_light_at(rt_ctx *ctx, int k, float angular_speed, float dt) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_light l[RT_MAX_LIGHTS];
    int n = 0;
    int rc = rt_scene_get_lights(ctx, l, RT_MAX_LIGHTS, &n);
    if (rc != RT_OK) return rc;
    if (k < 0 || k >= n) return fail(ctx, RT_ERR_INVALID, "light %d outside the scene's %d", k, n);
    if ((rc = rt_light_orbit(&l[k], angular_speed, dt, &l[k])) != RT_OK) return rc;
    return rt_scene_set_light_at(ctx, k, &l[k]);
}

// ---- lights with a radius (raytrace_hip.h "soft shadows"): one radius per light of the list, host state beside it ----
static int radius_check(rt_ctx *ctx, int k, float r) {
    if (std::signbit(r) || !std::isfinite(r)) return fail(ctx, RT_ERR_INVALID, "light %d: radius %g has its sign bit set or is not finite", k, (double)r);
    return RT_OK;
}

int rt_scene_set_light_radii(rt_ctx *ctx, const float *radii, int n) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!radii) return fail(ctx, RT_ERR_INVALID, "radii is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (n != ctx->n_lights) return fail(ctx, RT_ERR_INVALID, "n %d is not the scene's %d lights", n, ctx->n_lights);
    for (int k = 0; k < n; ++k) if (int rc = radius_check(ctx, k, radii[k]); rc != RT_OK) return rc;
    float r[RT_MAX_LIGHTS];
    memcpy(r, radii, (size_t)n * sizeof(float));                         // (radii may point into ctx->light_radii)
    put_radii(ctx, r, n);
    return RT_OK;
}

int rt_scene_get_light_radii(const rt_ctx *ctx, float *out, int cap, int *n) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!n) return fail(c, RT_ERR_INVALID, "n is NULL");
    if (cap < 0 || (cap > 0 && !out)) return fail(c, RT_ERR_INVALID, "out is NULL with cap %d", cap);
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    *n = ctx->n_lights;
    if (cap == 0) return RT_OK;                                          // the count alone
    if (cap < ctx->n_lights) return fail(c, RT_ERR_INVALID, "cap %d is below the scene's %d lights", cap, ctx->n_lights);
    memcpy(out, ctx->light_radii, (size_t)ctx->n_lights * sizeof(float));
    return RT_OK;
}

int rt_scene_set_light_radius_at(rt_ctx *ctx, int k, float radius) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (k < 0 || k >= ctx->n_lights) return fail(ctx, RT_ERR_INVALID, "light %d outside the scene's %d", k, ctx->n_lights);
    if (int rc = radius_check(ctx, k, radius); rc != RT_OK) return rc;
    float r[RT_MAX_LIGHTS];
    memcpy(r, ctx->light_radii, sizeof(r));
    r[k] = radius;
    put_radii(ctx, r, ctx->n_lights);
    return RT_OK;
}

// ---- the camera's thin lens (raytrace_hip.h "thin lens"): host state; the opening launch of every chain captures it ----
int rt_camera_set_lens(rt_ctx *ctx, float aperture_radius, float focus_distance) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (std::signbit(aperture_radius) || !std::isfinite(aperture_radius))
        return fail(ctx, RT_ERR_INVALID, "aperture radius %g has its sign bit set or is not finite", (double)aperture_radius);
    if (aperture_radius > 0.f && !(std::isfinite(focus_distance) && focus_distance > 0.f))
        return fail(ctx, RT_ERR_INVALID, "focus distance %g is not finite or not above 0", (double)focus_distance);
    if ((aperture_radius > 0.f) != (ctx->lens_radius > 0.f)) ctx->still.lens_changed();   // on or off: the still view's levels are emptied (rt_still.h)
    ctx->lens_radius = aperture_radius;
    ctx->lens_focus = focus_distance;
    return RT_OK;
}

int rt_camera_get_lens(const rt_ctx *ctx, float *aperture_radius, float *focus_distance) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!aperture_radius || !focus_distance) return fail(const_cast<rt_ctx *>(ctx), RT_ERR_INVALID, "aperture_radius / focus_distance is NULL");
    *aperture_radius = ctx->lens_radius;
    *focus_distance = ctx->lens_focus;
    return RT_OK;
}

// ---- the shutter motion (raytrace_hip.h "shutter"): host state; every launch of a chain captures the table make_frame derives from it ----
int rt_scene_set_shutter(rt_ctx *ctx, const rt_shutter *shutter) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    const rt_shutter closed = {};
    const rt_shutter &s = shutter ? *shutter : closed;                   // NULL closes the shutter
    bool on = false;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s.light[a])) return fail(ctx, RT_ERR_INVALID, "shutter: the light's displacement has a component that is not finite");
        on = on || s.light[a] != 0.f;
    }
    for (int slot = 0; slot < RT_MAX_OBJECTS; ++slot) {
        bool moves = false;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(s.object[slot][a])) return fail(ctx, RT_ERR_INVALID, "shutter: the displacement of object_slot %d has a component that is not finite", slot);
            moves = moves || s.object[slot][a] != 0.f;
        }
        if (moves && slot >= ctx->scene.n_objects) return fail(ctx, RT_ERR_INVALID, "shutter: object_slot %d moves, beyond the scene's %d objects", slot, ctx->scene.n_objects);
        if (moves && sphere_at(ctx->scene, slot) < 0) return fail(ctx, RT_ERR_INVALID, "shutter: object_slot %d is a mesh: meshes do not move within an exposure", slot);
        on = on || moves;
    }
    if (on != ctx->shutter_on) ctx->still.shutter_changed();             // on or off: the still view's levels are emptied (rt_still.h)
    ctx->shutter = s;
    ctx->shutter_on = on;
    return RT_OK;
}

int rt_scene_get_shutter(const rt_ctx *ctx, rt_shutter *out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!out) return fail(c, RT_ERR_INVALID, "out is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    *out = ctx->shutter;
    return RT_OK;
}

// ---- sky sampling (raytrace_hip.h "sky sampling"): the table of the map the context holds, for a share `share` (rt_skydist.hip.h) ----
// The table of the n x n map at `texels` (device memory) for a share `share`, built into `built`: a buffer of its own and the total; total 0 -- no map, share 0 or a map
// that is zero throughout -- is no table.  Nothing of the context changes here: the caller installs what was built once every step has succeeded (SkyDistBuilt::install),
// and a failure leaves the state as it was.  The device is idle when this returns with a table (the frames that captured the old one are done: the rule of the map's buffer).
struct SkyDistBuilt {
    DevBuf buf; unsigned long long total = 0; int nb = 0;
    void install(rt_ctx *ctx) { ctx->env_total = total; if (total > 0) { ctx->env_dist = std::move(buf); ctx->env_dist_nb = nb; } }
};
static int sky_dist_build(rt_ctx *ctx, const void *texels, int n_map, float share, SkyDistBuilt &built) {
    if (n_map <= 0 || !(share > 0.f)) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_OWN_STREAM(ctx);
    hipStream_t q = own_stream(ctx);
    const int n = n_map, count = n * n, nb = (count + rtk::kSkyBlock - 1) / rtk::kSkyBlock;
    DevBuf tmp;
    DevBuf &fresh = built.buf;
    int rc;
    if ((rc = ensure(ctx, tmp, (size_t)count * sizeof(float) + 16)) != RT_OK || (rc = ensure(ctx, fresh, (size_t)count * 12 + (size_t)nb * 8)) != RT_OK) return rc;
    float *W = static_cast<float *>(tmp.p);
    unsigned int *wmax = reinterpret_cast<unsigned int *>(W + count);
    unsigned long long *prefix = static_cast<unsigned long long *>(fresh.p), *blk = prefix + count;
    unsigned int *c = reinterpret_cast<unsigned int *>(blk + nb);
    const dim3 g((unsigned)nb), b(rtk::kSkyBlock);
    RT_HIP(ctx, hipMemsetAsync(wmax, 0, sizeof(unsigned int), q));
    hipLaunchKernelGGL(rtk::sky_dist_weights, g, b, 0, q, static_cast<const float4 *>(texels), n, W, wmax);
    RT_HIP(ctx, hipGetLastError());
    unsigned int wmax_bits = 0;
    RT_HIP(ctx, hipMemcpyAsync(&wmax_bits, wmax, sizeof(wmax_bits), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipStreamSynchronize(q));
    if (wmax_bits == 0) return RT_OK;                                  // the lookup is 0 throughout: the table is empty
    hipLaunchKernelGGL(rtk::sky_dist_quantise, g, b, 0, q, W, count, wmax, c, blk);
    hipLaunchKernelGGL(rtk::sky_dist_scan, dim3(1), dim3(rtk::kSkyScanLevel), 0, q, blk, nb);
    hipLaunchKernelGGL(rtk::sky_dist_prefix, g, b, 0, q, c, count, blk, prefix);
    RT_HIP(ctx, hipGetLastError());
    unsigned long long total = 0;
    RT_HIP(ctx, hipMemcpyAsync(&total, blk + (nb - 1), sizeof(total), hipMemcpyDeviceToHost, q));
    RT_HIP(ctx, hipStreamSynchronize(q));
    RT_HIP(ctx, hipDeviceSynchronize());
    built.nb = nb;
    built.total = total;
    return RT_OK;
}

int rt_scene_set_environment_sampling(rt_ctx *ctx, float share) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (!(share >= 0.f && share <= 1.f)) return fail(ctx, RT_ERR_INVALID, "environment sampling: the share %g is outside [0, 1]", (double)share);
    if (share == 0.f) share = 0.f;                                     // (-0 is 0)
    if (share == ctx->env_share) return RT_OK;
    // the table depends on the map alone: it is built when the share becomes positive and dropped when it becomes 0
    if (!(share > 0.f) || !(ctx->env_share > 0.f)) {
        SkyDistBuilt built;
        if (int rc = sky_dist_build(ctx, ctx->env.p, ctx->env_n, share, built); rc != RT_OK) return rc;   // (a failure: share and table as they were)
        built.install(ctx);
    }
    ctx->env_share = share;
    ctx->still.sky_changed();
    return RT_OK;
}

int rt_scene_get_environment_sampling(const rt_ctx *ctx, float *share) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!share) return fail(c, RT_ERR_INVALID, "share is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    *share = ctx->env_share;
    return RT_OK;
}

// ---- emissive meshes (raytrace_hip.h "emissive meshes"): host state plus the table over the scene's triangles (rt_skydist.hip.h) ----
// index into Scene::mesh of the mesh at position object_slot of Scene::objects; -1: outside the scene, or a sphere's position
static int mesh_at(const rtk::Scene &sc, int object_slot) {
    for (int k = 0; k < sc.n_meshes; ++k) if (sc.mesh[k].obj == object_slot) return k;
    return -1;
}
// (the table itself: emit_dist_of and emit_refresh in rt_host_render.hip.h, where a frame's chain asks for it)

// a component of a radiance: in [+0, 2^96), the range of the environment's texels (NaN, +-inf, negative and -0 fail the bit test)
static bool emit_component_ok(float v) { return __builtin_bit_cast(uint32_t, v) < 0x6f800000u; }

int rt_scene_set_emission(rt_ctx *ctx, int object_slot, const float rgb[3]) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (!rgb) return fail(ctx, RT_ERR_INVALID, "emission: rgb is NULL");
    if (mesh_at(ctx->scene, object_slot) < 0) return fail(ctx, RT_ERR_INVALID, "emission: object_slot %d is outside the scene or a sphere's; only a mesh emits", object_slot);
    for (int k = 0; k < 3; ++k)
        if (!emit_component_ok(rgb[k])) return fail(ctx, RT_ERR_INVALID, "emission: component %d (%g) is outside [+0, 2^96)", k, (double)rgb[k]);
    float *le = ctx->emit_le[object_slot];
    if (memcmp(le, rgb, 3 * sizeof(float)) == 0) return RT_OK;
    memcpy(le, rgb, 3 * sizeof(float));
    const bool emits = rgb[0] > 0.f || rgb[1] > 0.f || rgb[2] > 0.f;
    ctx->emit_mask = emits ? ctx->emit_mask | (1u << object_slot) : ctx->emit_mask & ~(1u << object_slot);
    ctx->emit_dirty = true;
    // (The still view is left alone.  Its keys hold nothing an emission changes, a chain under an emitter neither reads nor writes its three buffers -- no begin, every
    // level off -- and the scene without its emitter is the scene the levels were stored for: a scene that lost its last emitter finds them as it left them.)
    return RT_OK;
}

int rt_scene_get_emission(const rt_ctx *ctx, int object_slot, float rgb[3]) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!rgb) return fail(c, RT_ERR_INVALID, "emission: rgb is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    if (mesh_at(ctx->scene, object_slot) < 0) return fail(c, RT_ERR_INVALID, "emission: object_slot %d is outside the scene or a sphere's; only a mesh emits", object_slot);
    memcpy(rgb, ctx->emit_le[object_slot], 3 * sizeof(float));
    return RT_OK;
}

int rt_scene_set_emission_sampling(rt_ctx *ctx, float share) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (!(share >= 0.f && share <= 1.f)) return fail(ctx, RT_ERR_INVALID, "emission sampling: the share %g is outside [0, 1]", (double)share);
    if (share == 0.f) share = 0.f;                                     // (-0 is 0)
    ctx->emit_share = share;                                           // (the table depends on the scene and the radiances alone)
    return RT_OK;
}

int rt_scene_get_emission_sampling(const rt_ctx *ctx, float *share) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!share) return fail(c, RT_ERR_INVALID, "share is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    *share = ctx->emit_share;
    return RT_OK;
}

// ---- Fresnel dielectrics (raytrace_hip.h "fresnel"): one bit per object position, host state alone ----
// (Whether a bit is effective is decided when a chain is planned, from the materials as they are then: fresnel_effective in rt_host_render.hip.h.  The still view is
// left alone, as by rt_scene_set_emission: a chain under an effective bit neither reads nor writes its buffers, and the scene without the bit is the scene they were stored for.)
int rt_material_set_fresnel(rt_ctx *ctx, int object_slot, int on) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (object_slot < 0 || object_slot >= ctx->scene.n_objects) return fail(ctx, RT_ERR_INVALID, "fresnel: object_slot %d is outside the scene", object_slot);
    ctx->fresnel_mask = on ? ctx->fresnel_mask | (1u << object_slot) : ctx->fresnel_mask & ~(1u << object_slot);
    return RT_OK;
}

int rt_material_get_fresnel(const rt_ctx *ctx, int object_slot, int *on) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    if (!on) return fail(c, RT_ERR_INVALID, "fresnel: on is NULL");
    if (object_slot < 0 || object_slot >= ctx->scene.n_objects) return fail(c, RT_ERR_INVALID, "fresnel: object_slot %d is outside the scene", object_slot);
    *on = (int)((ctx->fresnel_mask >> object_slot) & 1u);
    return RT_OK;
}

// ---- rough mirrors (raytrace_hip.h "roughness"): one alpha per object position, host state alone ----
// (Whether a value is effective is decided when a chain is planned, from the materials as they are then: gloss_effective in rt_host_render.hip.h.  The still view is
// left alone, as by rt_material_set_fresnel: a chain under an effective roughness neither reads nor writes its buffers.)
int rt_material_set_roughness(rt_ctx *ctx, int object_slot, float alpha) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (object_slot < 0 || object_slot >= ctx->scene.n_objects) return fail(ctx, RT_ERR_INVALID, "roughness: object_slot %d is outside the scene", object_slot);
    if (!(alpha == 0.f || (alpha >= 0x1p-12f && alpha <= 1.f))) return fail(ctx, RT_ERR_INVALID, "roughness: alpha %g is neither 0 nor in [2^-12, 1]", (double)alpha);
    ctx->gloss_alpha[object_slot] = alpha == 0.f ? 0.f : alpha;          // (-0 is stored as +0)
    return RT_OK;
}

int rt_material_get_roughness(const rt_ctx *ctx, int object_slot, float *alpha) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    if (!alpha) return fail(c, RT_ERR_INVALID, "roughness: alpha is NULL");
    if (object_slot < 0 || object_slot >= ctx->scene.n_objects) return fail(c, RT_ERR_INVALID, "roughness: object_slot %d is outside the scene", object_slot);
    *alpha = ctx->gloss_alpha[object_slot];
    return RT_OK;
}

// ---- tinted mirrors and glass (raytrace_hip.h "tint"): one bit per object position, host state alone ----
// (Whether a bit is effective is decided when a chain is planned, from the materials as they are then: tint_effective in rt_host_render.hip.h.  The still view is left
// alone, as by rt_material_set_fresnel: a chain under an effective tint neither reads nor writes its buffers, and the scene without the bit is the scene they were stored for.)
int rt_material_set_tint(rt_ctx *ctx, int object_slot, int on) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (object_slot < 0 || object_slot >= ctx->scene.n_objects) return fail(ctx, RT_ERR_INVALID, "tint: object_slot %d is outside the scene", object_slot);
    ctx->tint_mask = on ? ctx->tint_mask | (1u << object_slot) : ctx->tint_mask & ~(1u << object_slot);
    return RT_OK;
}

int rt_material_get_tint(const rt_ctx *ctx, int object_slot, int *on) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    if (!on) return fail(c, RT_ERR_INVALID, "tint: on is NULL");
    if (object_slot < 0 || object_slot >= ctx->scene.n_objects) return fail(c, RT_ERR_INVALID, "tint: object_slot %d is outside the scene", object_slot);
    *on = (int)((ctx->tint_mask >> object_slot) & 1u);
    return RT_OK;
}

// ---- the environment map (raytrace_hip.h "environment"): host state plus one device buffer of the context's; make_frame captures pointer and size ----
int rt_scene_set_environment(rt_ctx *ctx, int n, const float *rgb) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    if (n < 0 || n > RT_MAX_ENVIRONMENT) return fail(ctx, RT_ERR_INVALID, "environment: n %d outside [0,%d]", n, RT_MAX_ENVIRONMENT);
    if (n > 0 && !rgb) return fail(ctx, RT_ERR_INVALID, "environment: rgb is NULL with n %d", n);
    if (n == 0 || !rgb) {                                                // removed (the buffer stays until the next map: frames in flight may read it)
        if (ctx->env_n > 0) ctx->still.sky_changed();
        ctx->env_n = 0; ctx->env_rgb.clear();
        ctx->env_total = 0;                                              // ... and its table with it; the share stays
        return RT_OK;
    }
    const size_t count = (size_t)n * (size_t)n;
    std::vector<float4> texels(count);
    for (size_t k = 0; k < count; ++k) {
        for (int a = 0; a < 3; ++a) {
            uint32_t bits;
            memcpy(&bits, &rgb[3 * k + a], sizeof(bits));
            // finite, sign bit clear, below 2^96: the bilinear sum stays finite and the dead-channel elision exact (rt_wavefront.hip.h wf_dead_channels)
            if (bits >= rtk::kDeadDirectEnd)
                return fail(ctx, RT_ERR_INVALID, "environment: texel (%d, %d) channel %d is %g: a radiance is finite, has a clear sign bit and is below 2^96", (int)(k % n), (int)(k / n), a, (double)rgb[3 * k + a]);
        }
        texels[k] = make_float4(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2], 0.f);
    }
    // A new map gets a new buffer; the old one is given back after the frames that captured it (the rule of rt_mesh_set_texture_of: the device is idle first)
    DevBuf fresh;
    if (int rc = upload(ctx, fresh, texels.data(), count * sizeof(float4)); rc != RT_OK) return rc;
    RT_HIP(ctx, hipDeviceSynchronize());
    SkyDistBuilt built;                                                  // the new map's table, if the share is positive: before anything of the context changes
    if (int rc = sky_dist_build(ctx, fresh.p, n, ctx->env_share, built); rc != RT_OK) return rc;
    built.install(ctx);
    ctx->env = std::move(fresh);
    ctx->env_rgb.assign(rgb, rgb + 3 * count);
    ctx->env_n = n;
    ctx->still.sky_changed();
    return RT_OK;                                                      // (the share stays)
}

int rt_scene_get_environment(const rt_ctx *ctx, int *n, float *rgb) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!n) return fail(c, RT_ERR_INVALID, "n is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    *n = ctx->env_n;
    if (rgb && ctx->env_n > 0) memcpy(rgb, ctx->env_rgb.data(), ctx->env_rgb.size() * sizeof(float));
    return RT_OK;
}

int rt_scene_get_sphere(const rt_ctx *ctx, int object_slot, rt_sphere *out) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_ctx *c = const_cast<rt_ctx *>(ctx);
    if (!out) return fail(c, RT_ERR_INVALID, "out is NULL");
    if (int rc = edit_scene_check(c); rc != RT_OK) return rc;
    const rtk::Scene &sc = ctx->scene;
    const int k = sphere_at(sc, object_slot);
    if (k < 0) return fail(c, RT_ERR_INVALID, "object_slot %d is not a sphere of the scene (%d objects)", object_slot, sc.n_objects);
    const rtk::Sphere &s = sc.sph[k];
    const float4 a = sc.obj_a[object_slot], b = sc.obj_b[object_slot];
    const float2 n = sc.obj_n[object_slot];
    *out = rt_sphere{{s.cx, s.cy, s.cz}, s.R, {b.x, b.y, b.z}, __builtin_bit_cast(int, a.w), n.x, n.y};
    return RT_OK;
}

int rt_scene_set_sphere(rt_ctx *ctx, int object_slot, const rt_sphere *sphere) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!sphere) return fail(ctx, RT_ERR_INVALID, "sphere is NULL");
    if (int rc = edit_scene_check(ctx); rc != RT_OK) return rc;
    const int k = sphere_at(ctx->scene, object_slot);
    if (k < 0) return fail(ctx, RT_ERR_INVALID, "object_slot %d is not a sphere of the scene (%d objects)", object_slot, ctx->scene.n_objects);
    put_sphere(ctx->scene, k, object_slot, *sphere);
    return RT_OK;
}

int rt_scene_move_light(rt_ctx *ctx, float angular_speed, float dt) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    rt_light l;
    int rc = rt_scene_get_light(ctx, &l);
    if (rc == RT_OK) rc = rt_light_orbit(&l, angular_speed, dt, &l);
    if (rc == RT_OK) rc = set_one_light(ctx, &l, true);                  // light 0, moved: it keeps its radius
    return rc;
}

int rt_scene_move_sphere(rt_ctx *ctx, int object_slot, const float v[3], float dt) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    if (!v) return fail(ctx, RT_ERR_INVALID, "v is NULL");
    rt_sphere s;
    int rc = rt_scene_get_sphere(ctx, object_slot, &s);
    if (rc != RT_OK) return rc;
    for (int a = 0; a < 3; ++a) {                                        // sp->C = sp->C + v * dt (realtime:1096): the product, then the sum, each rounded to binary32
        const float step = v[a] * dt;
        s.center[a] = s.center[a] + step;
    }
    return rt_scene_set_sphere(ctx, object_slot, &s);
}
