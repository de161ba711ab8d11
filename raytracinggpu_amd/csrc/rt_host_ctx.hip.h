// rt_host_ctx.hip.h -- host side of libraytrace_hip.so, part 1 of 4 (textually included by rt_capi.hip, one translation unit): the owning handles (DevBuf, Event, Stream:
// whoever declares one owns it, its destructor gives it back), the context (rt_ctx: its buffers list themselves in rt_ctx::bufs as they are declared, ~rt_ctx waits for
// the context's streams and the members do the rest), its knobs (environment variables read once per context), error reporting, the stream a call runs on when the
// caller passes none.
#pragma once

namespace {

thread_local std::string g_last_error;

// Device memory.  A context's buffer is declared `DevBuf x{bufs};` and is thereby on the list rt_ctx_selfcheck walks; a temporary takes the default constructor.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    explicit DevBuf(std::vector<DevBuf *> &list) { list.push_back(this); }
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf owns its memory: it moves, it is never copied");

// N buffers of a context (the elements of a plain array member could not each be handed the list)
template <int N>
struct DevBufs {
    DevBuf b[N];
    explicit DevBufs(std::vector<DevBuf *> &list) { for (DevBuf &x : b) list.push_back(&x); }
    DevBuf &operator[](int k) { return b[k]; }
};

// An event / a stream of the owner's: null until create(), which returns the runtime's status; reads as the raw handle wherever one is expected.
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(const Event &) = delete; Event &operator=(const Event &) = delete;
    ~Event() { if (h) (void)hipEventDestroy(h); }
    hipError_t create(unsigned flags = hipEventDefault) { const hipError_t e = hipEventCreateWithFlags(&h, flags); if (e != hipSuccess) h = nullptr; return e; }
    operator hipEvent_t() const { return h; }
};
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete; Stream &operator=(const Stream &) = delete;
    ~Stream() { if (h) (void)hipStreamDestroy(h); }
    hipError_t create() { const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking); if (e != hipSuccess) h = nullptr; return e; }
    hipError_t create(int priority) { const hipError_t e = hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority); if (e != hipSuccess) h = nullptr; return e; }
    operator hipStream_t() const { return h; }
};

}  // namespace

// Tuning / test knobs: environment variables read ONCE, when the context is created (rt_ctx_create).  Defaults are the
// measured optimum on MI355X; tests create a context under a modified environment to reach the rare code paths.
struct Knobs {
    int travq_R = 64;          // RT_TRAVQ_R: ray slots per wave of the work-stack kernel (32 | 64).  (128 -- two slots per lane, two sibling pairs per lane and BOX step -- measured 19 % slower
                               // per frame: 10 waves per CU instead of 16, profiles/round4/ab_128_rays_per_wave.txt; its instantiations left the library in round 5, the kernel source still
                               // carries the two-bank form behind R > 64)
    int travq_cap = 0;         // RT_TRAVQ_CAP: stack capacity (>= 128; tests force the serial drain); 0 = the carve's capacity
    int travq_lds = 0;         // RT_TRAVQ_LDS: waves of the ONE workgroup per CU that stages the top of the BVH in LDS; 0 = nodes through L1/L2
    int q_low = 48;            // RT_TRAVQ_LOW: refill while the stack holds fewer sibling pairs than this (measured 1.19 / 1.21 / 1.25 ms per frame for 48 / 64 / 96)
    int q16 = -1;              // RT_TRAVQ_Q16: the BOX step reads 16-bit fixed-point sibling pairs (32 bytes: two loads instead of four; rt_qnodes.hip.h) when the tree allows it.
                               // -1 (default) = for trees of at least kQ16AutoNodes nodes, 0 = never, 1 = always.  Bit-exact either way; on the cat (2 019 nodes, L1-resident) it measures
                               // +-0 once every leaf decision is exact (profiles/round4/ab_fixed_point_pairs.txt), on 55 000 / 533 000 nodes -8 % / -18 % per frame (big_mesh_bench.txt)
    int qw = -1;               // RT_TRAVQ_QW: the BOX step is four boxes wide (fixed-point quads: the children of both nodes of a sibling pair in 64 bytes, every other level of the tree
                               // skipped; leaves flagged and decided as the fixed-point pairs decide them; rt_travq.hip.h, QW).  -1 (default) = 1 = on where the tree allows the format (boxes nest, leaves of
                               // at most 127 triangles, fewer than 2^21 nodes), 0 = off.  Bit-exact either way; cat 1920x1080: 0.934 -> 0.861 ms per frame (profiles/round5/ab_wide_nodes.txt)
    int quad_sel = 1;          // RT_TRAVQ_QSEL=0: the quads of the 4-wide step take every other level of the tree (A/B; default: the four nodes a surface-area DP picks, rt_qnodes.hip.h)
    int anyhit = 1;            // RT_TRAVQ_ANYHIT=0: shadow rays are traced to the end like every other ray (A/B, cross-check; default: the fixed-point traversal kernels stop a shadow ray at the
                               // first accepted triangle that certainly shades, rt_wavefront.hip.h wf_anyhit_bound).  Bit-exact either way
    int dead_channels = 1;     // RT_DEAD_CHANNELS=0: a diffuse segment whose three colour channels are dead (a zero albedo component earlier on the path in each) still traces its
                               // shadow ray (A/B, cross-check; default: with any-hit on it does not, rt_wavefront.hip.h wf_dead_channels).  Bit-exact either way
    int dead_last = 1;         // RT_DEAD_LAST=0: the last continuation ray of a path whose three colour channels are dead is traced through the mesh like every other (A/B, cross-check;
                               // default: where the scene allows it and the ray certainly hits a sphere it is not, rt_deadlast.h, rt_wavefront.hip.h kPolDeadLast).  Bit-exact either way
    int travq_rows = 1;        // RT_TRAVQ_ROWS=0: every wf_travq launch scans the whole queue (A/B, cross-check; default: the first launch of a chain enumerates the rows that hold continuation
                               // rays only and the last the rows that hold shadow rays only, rt_qrows.h).  Bit-exact either way
    int first_hit_cache = 1;   // RT_FIRST_HIT_CACHE=0: every chain traces its camera rays (A/B, cross-check, and the figure of a moving camera; default: a still camera's primary mesh hits
                               // are traced once and kept, rt_still.h).  Bit-exact either way
    int first_shadow_cache = 1; // RT_FIRST_SHADOW_CACHE=0: every chain traces the shadow rays of its first segment (A/B, cross-check, and the figure of a moving light; default: under a still
                               // camera AND a still light, scene and shading state they are traced once and kept, rt_still.h).  Off with RT_FIRST_HIT_CACHE=0.  Bit-exact either way
    int first_shade_cache = 1; // RT_FIRST_SHADE_CACHE=0: every chain of a still view opens with wf_advance<kFormFirst> and closes segment 0 (A/B, cross-check; default: once the first-shadow cache has held
                               // for two chains, a path's state after its shaded first hit is kept and later chains resume from it, rt_still.h).  Off with either older
                               // knob at 0, and for scenes with a textured mesh.  Bit-exact either way
    int chain_ends = 1;        // RT_CHAIN_ENDS=0: the last wf_advance launch of a plain chain is the generic kernel (A/B, cross-check; default: wf_advance<kFormClose>, which only closes
                               // the last segment's shadow rays and folds, rt_wavefront.hip.h CLOSE, rt_still.h kAdvClose).  Bit-exact either way
    int stream_policy = 3;     // RT_STREAM_POLICY: a bit per group of use-once streams whose accesses in wf_advance go past the Infinity Cache (rt_wavefront.hip.h kPol*: 1 the
                               // first-shade records a resumed chain loads, 2 the pixel store of the fold); 0: every access the plain instruction, the code of before the policy
                               // (A/B, cross-check).  Bit-exact whatever the value; headline -1.1 ... -1.4 %
    int sky_search = 1;        // RT_SKY_SEARCH=0: the draw of rt_kat_environment_sample searches the prefixes with one flat binary search (A/B, cross-check; default: the block level
                               // first, then inside one block, rt_shade.hip.h sky_pick).  Bit-exact either way
    int refit_wide = 1;        // RT_REFIT_WIDE=0: rt_mesh_set_vertices* refits with the one-workgroup refit_kernel, as rt_mesh_transform does (A/B, cross-check; default: the climb across
                               // the chip, rt_meshops.hip.h refit_up_kernel).  Bit-exact either way
    int auto_lockstep = 1;     // RT_AUTO_LOCKSTEP=0: RT_VARIANT_AUTO stays the wavefront pipeline for scenes without a mesh (A/B; default: the lock-step kernel renders them)
    int qw_count = 0;          // RT_TRAVQ_QW_COUNT=1: rt_count_work runs the 4-wide kernel's counting instantiation (its own step counters; the box / node counts then describe
                               // THAT kernel, not the reference's traversal)
    float lbvh_ct = 0.f;       // RT_LBVH_CT: cost of a triangle test relative to a box test in the LBVH's leaf cut (0 = kLbvhCt)
    int q_minfree = 0;         // RT_TRAVQ_MINFREE: ... and at least this many slots are free (0 = R / 4)
    int parts = 2;             // RT_PARTS: concurrent sub-frames of the wavefront pipeline
    int bpc5 = 0;              // (fixed; RT_TRAVQ_BPC5 was an environment knob until round 5) allow a fifth workgroup per CU
    int trav_waves = 0;        // RT_TRAV_WAVES: cap on traversal workgroups per CU
    int oversub = 2;           // RT_TRAVQ_OVERSUB: grid oversubscription of the work-stack kernel
    int oversub_min = 0;       // (fixed; RT_TRAVQ_OVERSUB_MIN was an environment knob until round 5)
    int min_groups = 16;       // RT_TRAV_MIN_GROUPS: ray groups per wave below which a launch uses fewer workgroups
    int log2S = -1;            // RT_TRAV_LOG2S: cap on the scramble period (experiment)
    int path_low = 96;         // (fixed; RT_PATH_LOW was an environment knob until round 5) wf_path runs a SHADE step only while the stack holds fewer sibling pairs than this
    int path_shade_min = 32;   // (fixed; RT_PATH_SHADE_MIN was an environment knob until round 5) ... and at least this many of the wave's 64 paths are ready (or nothing else is left to do)
    int path_oversub = 2;      // (fixed; RT_PATH_OVERSUB was an environment knob until round 5) grid oversubscription of wf_path
    int path_bpc = 4;          // (fixed; RT_PATH_BPC was an environment knob until round 5) workgroups (4 waves) per CU
    int path_parts = 1;        // (fixed; RT_PATH_PARTS was an environment knob until round 5) concurrent sub-frames (launches on separate streams)
    long long path_samp_bytes = 400ll << 20; // RT_PATH_SAMP_MB: state of the samples traced together (frames with num_rays > 1; ~130 B per sample and pixel slot).
                                             // Measured: a chain is fastest while its state stays near the 256 MB Infinity Cache -- 512x512, 64 samples: 23.5 / 8.8 / 8.0 /
                                             // 8.8 ms for 30 / 192 / 400 / 4096 MB; 1920x1080 (277 MB per sample): one sample per chain is best (71.5 vs 76.9 ms at 13)
    double chunk_mpx = 2.3;    // RT_CHUNK_MPX: pixels (millions) of one sequential chunk of a big frame in the wavefront pipeline; 0 = never cut
    int part_prio = 0;         // RT_PART_PRIO=1: the second sub-frame's stream in the high-priority class, which has its own pool of hardware queues.  A process
                               // that holds SEVERAL contexts (rt_multi does this itself; bench.py with N > 1) should set it: with more streams than the runtime has
                               // hardware queues (four) two active streams may share one and a context's sub-frames then run one after the other (1/8 of
                               // 7680x4320: 2.7 instead of 2.0 ms).  Off by default: a lone context is 1 % faster with both sub-frames at equal priority.
    int adv_block = 64;        // RT_ADV_BLOCK: threads per workgroup of wf_advance (64 / 128 / 256).  One-wave workgroups slip into the wave slots the traversal
                               // kernel of the other sub-frame frees one by one: 0.970 -> 0.957 ms per frame (128: 0.963; profiles/round3/ab_advance_block.log)
    int copy_prio = 1;         // (fixed; RT_COPY_PRIO was an environment knob until round 5) the copy streams of rt_render_async in the low-priority class (1, default), the normal one (0) or the high one (-1).  The
                               // runtime keeps a pool of hardware queues per class; in the normal class the copy stream can share a queue with one of the
                               // sub-frame streams and the copy then waits behind kernels (pipelined float4 frames 1.72 instead of 1.19 ms)
    int async_pipeline = 1;    // RT_ASYNC_PIPELINE=0: rt_render_async joins the sub-frames of frame k before frame k+1 starts (as rt_render_device does without rt_ctx_set_pipelining)
    int copy_split = 0;        // (fixed; RT_COPY_SPLIT=1 was an environment knob until round 5) rt_render_async sends the two halves of a big frame through two copy streams (measured SLOWER: 1.62 vs 1.48 ms per
                               // pipelined 1080p float4 frame -- one DMA already runs at the rate the PCIe link gives, two share it and add an event hop)
    int debug_trav = -2;       // RT_DEBUG_TRAV: traversal launch whose per-wave records are dumped (-DRT_DEBUG builds only)
};

static Knobs read_knobs() {
    Knobs k;
    auto geti = [](const char *name, int &out) { const char *e = getenv(name); if (e && *e) { out = atoi(e); return true; } return false; };
    int v;
    // --- knobs a caller or a test may set: which (bit-identical) kernel form runs, how a call is cut up.  INTEGRATION.md section 4 lists them.
    if (geti("RT_TRAVQ_R", v) && (v == 32 || v == 64)) k.travq_R = v;
    if (geti("RT_TRAVQ_CAP", v) && v >= 128) k.travq_cap = v;
    if (geti("RT_TRAVQ_LDS", v) && v >= 1 && v <= 16) k.travq_lds = v;
    if (geti("RT_TRAVQ_Q16", v) && v >= -1 && v <= 1) k.q16 = v;
    if (geti("RT_TRAVQ_QW", v) && v >= -1 && v <= 1) k.qw = v;
    if (geti("RT_TRAVQ_QW_COUNT", v)) k.qw_count = v != 0;
    if (geti("RT_AUTO_LOCKSTEP", v)) k.auto_lockstep = v != 0;
    if (geti("RT_TRAVQ_QSEL", v)) k.quad_sel = v != 0;
    if (geti("RT_TRAVQ_ANYHIT", v)) k.anyhit = v != 0;
    if (geti("RT_DEAD_CHANNELS", v)) k.dead_channels = v != 0;
    if (geti("RT_DEAD_LAST", v)) k.dead_last = v != 0;
    if (geti("RT_SKY_SEARCH", v)) k.sky_search = v != 0;
    if (geti("RT_TRAVQ_ROWS", v)) k.travq_rows = v != 0;
    if (geti("RT_FIRST_HIT_CACHE", v)) k.first_hit_cache = v != 0;
    if (geti("RT_FIRST_SHADOW_CACHE", v)) k.first_shadow_cache = v != 0;
    if (geti("RT_FIRST_SHADE_CACHE", v)) k.first_shade_cache = v != 0;
    if (geti("RT_CHAIN_ENDS", v)) k.chain_ends = v != 0;
    if (geti("RT_STREAM_POLICY", v) && v >= 0 && v <= 3) k.stream_policy = v;
    if (geti("RT_REFIT_WIDE", v)) k.refit_wide = v != 0;
    if (geti("RT_PARTS", v) && v >= 1 && v <= 8) k.parts = v;
    if (geti("RT_PART_PRIO", v)) k.part_prio = v != 0;
    { const char *e = getenv("RT_CHUNK_MPX"); if (e && *e) { const double d = atof(e); if (d >= 0 && d < 1e4) k.chunk_mpx = d; } }
    if (geti("RT_ASYNC_PIPELINE", v)) k.async_pipeline = v != 0;
    if (geti("RT_PATH_SAMP_MB", v) && v >= 1) k.path_samp_bytes = (long long)v << 20;
    // --- launch-geometry knobs of the A/B tools (tools/ab_variants.sh, share_*.py): honoured only under RT_EXPERIMENT=1, so that a stray variable in a
    //     caller's environment cannot move a product frame off its measured optimum
    if (geti("RT_EXPERIMENT", v) && v != 0) {
        if (geti("RT_TRAVQ_LOW", v) && v >= 32 && v <= 320) k.q_low = v;
        if (geti("RT_TRAVQ_MINFREE", v) && v >= 1 && v <= 64) k.q_minfree = v;
        if (const char *e = std::getenv("RT_LBVH_CT")) { const float f = (float)std::atof(e); if (f > 0.f && f < 100.f) k.lbvh_ct = f; }
        if (geti("RT_TRAV_WAVES", v) && v >= 1) k.trav_waves = v;
        if (geti("RT_TRAVQ_OVERSUB", v) && v >= 1 && v <= 16) k.oversub = v;
        if (geti("RT_TRAV_MIN_GROUPS", v) && v >= 4) k.min_groups = v;
        if (geti("RT_TRAV_LOG2S", v) && v >= 0) k.log2S = v;
        if (geti("RT_ADV_BLOCK", v) && (v == 64 || v == 128 || v == 256)) k.adv_block = v;
    }
#ifdef RT_DEBUG
    if (geti("RT_DEBUG_TRAV", v)) k.debug_trav = v;
#endif
    return k;
}

struct rt_ctx {
    int device = 0;
    Knobs knobs;
    Stream stream_;                                                  // the context's own stream: created when first needed (own_stream)
    Event ev_k0, ev_k1, ev_t0, ev_t1;
    std::vector<DevBuf *> bufs;                                      // every device buffer of the context: each one's declaration below puts it here (rt_ctx_selfcheck)
    bool have_scene = false, have_kernel_time = false, have_tonemap_time = false;
    rtk::Scene scene{};
    // The scene's lights (rt_scene_set_lights, rt_host_edit.hip.h).  One light lives in `scene` alone, as ever; a list of several is kept here, its first entry also in
    // `scene` (rt_scene_get_light answers it), and reaches the kernels as the rtk::WfLights argument make_frame derives from it.  rt_scene_upload* and rt_scene_set_light
    // set n_lights back to 1.
    rt_light lights[rtk::kMaxLights] = {};
    int n_lights = 1;
    // ... and their radii (rt_scene_set_light_radii): entry k belongs to light k of the list, a list of one included; all 0 unless that entry set them
    float light_radii[rtk::kMaxLights] = {};
    // The camera's thin lens (rt_camera_set_lens): aperture radius and focus distance in scene units.  Host state like the lights: make_frame captures it by value, and a
    // radius above 0 makes every chain open with wf_advance<kFormFirst | kFormLens>.  rt_scene_upload* leaves a pinhole: the camera comes with the upload.
    float lens_radius = 0.f, lens_focus = 1.f;
    // The shutter motion (rt_scene_set_shutter): what the light and every object slot travel over one frame's exposure.  Host state like the lens: make_frame captures it by
    // value.  shutter_on: some component is not +-0 -- every launch of every chain is then a kFormShutter form.  rt_scene_upload* closes it.
    rt_shutter shutter = {};
    bool shutter_on = false;
    // The environment map (rt_scene_set_environment): env_n x env_n texels, host copy (3 floats each, row 0 first) and the device's (float4 each).  env_n == 0: no
    // environment.  make_frame captures pointer and size by value; a new map gets a new buffer, and the old one is given back once no frame in flight can read it.
    // rt_scene_upload* removes it: it belongs to the scene.
    int env_n = 0;
    std::vector<float> env_rgb;
    DevBuf env{bufs};
    // Sky sampling (rt_scene_set_environment_sampling): the share of the shadow rays that go to the map, and the table the draws search -- one buffer, the prefixes
    // (n * n of 64 bits), the block level (env_dist_nb) and c (n * n of 32 bits) in this order.  env_total == 0: no table (the share is 0, no map, or the map is zero
    // throughout).  A rebuilt table gets a new buffer, as a new map does.  rt_scene_upload* resets the share.
    float env_share = 0.f;
    unsigned long long env_total = 0;
    int env_dist_nb = 0;
    DevBuf env_dist{bufs};
    // Emissive meshes (rt_scene_set_emission): the radiance of every object position (zeros: it does not emit), the mask of the emitting ones, the share of the shadow
    // rays that go to them, and the table the draws search -- one buffer: the prefixes (emit_nt of 64 bits), the block level (emit_nb), c (emit_nt of 32 bits) and, at the
    // next multiple of 16 bytes, the radiances (kMaxObjects float4: r, g, b, Y).  emit_total == 0: no table.  The table is stale while emit_dirty is set or emit_gen is
    // not the still view's triangle generation (every entry that changes a triangle or the visit order moves that, and nothing else does); emit_refresh (rt_host_render.hip.h) rebuilds it, into a
    // new buffer, before anything reads it.  rt_scene_upload* clears the emission and sets the share to 0.5.
    float emit_le[rtk::kMaxObjects][3] = {};
    unsigned emit_mask = 0;
    float emit_share = 0.5f;
    bool emit_dirty = false;
    uint64_t emit_gen = 0;
    unsigned long long emit_total = 0;
    int emit_nt = 0, emit_nb = 0;
    DevBuf emit_dist{bufs};
    // Fresnel dielectrics (rt_material_set_fresnel): one bit per object position.  A bit is EFFECTIVE only where the object's material takes the refraction branch, read
    // when a chain is planned (fresnel_effective, rt_host_render.hip.h).  rt_scene_upload* clears every bit.
    unsigned fresnel_mask = 0;
    // Rough mirrors (rt_material_set_roughness): one binary32 alpha per object position, 0 (smooth) or in [2^-12, 1].  A value is EFFECTIVE only where the object's
    // material takes the mirror branch, read when a chain is planned (gloss_effective, rt_host_render.hip.h).  rt_scene_upload* clears every value.
    float gloss_alpha[rtk::kMaxObjects] = {};
    // Tinted mirrors and glass (rt_material_set_tint): one bit per object position.  A bit is EFFECTIVE only where the object's material takes a specular arm, read when a
    // chain is planned (tint_effective, rt_host_render.hip.h).  rt_scene_upload* clears every bit.
    unsigned tint_mask = 0;
    DevBuf nrm{bufs};                                                 // smooth shading: 3 normals per triangle, visit order
    // textured meshes (rt_mesh_set_texture[_of]): 3 UVs per triangle in visit order (one buffer for the forest; a mesh's entries are read only while its bit is set),
    // the device copy of the per-object records, and per object its decode table (256 floats) followed by its texels.  rt_scene_upload* clears tex_mask first.
    DevBuf tex_uv{bufs}, tex_table{bufs};
    DevBufs<rtk::kMaxObjects> tex_img{bufs};
    rtk::TexDesc tex_desc[rtk::kMaxObjects] = {};
    int tex_mask = 0;
    std::vector<int> tri_perm;                                       // visit order -> triangle index in the uploaded (BVH-order) arrays
    std::vector<int> up_indices;                                     // vertex indices of the uploaded triangles, 3 per triangle
    int n_up_tris = 0;
    DevBuf tidx_up{bufs};                                             // the same on the device (int4 per triangle)
    DevBuf bb_idx{bufs}, bb_cnt{bufs}, bb_pa{bufs}, bb_pb{bufs}, bb_tmp{bufs}, bb_nodes_i{bufs}, bb_nodes_f{bufs}, bb_counter{bufs}, bb_lvl{bufs}, bb_size{bufs}, bb_pre{bufs}, bb_arr{bufs};   // device BVH build scratch
    DevBuf left_dev{bufs}, lvl_nodes{bufs}, lvl_off{bufs};           // tree topology for the device-side refit
    DevBuf refit_parent{bufs}, refit_cnt{bufs};                      // the chip-wide refit of rt_mesh_set_vertices* (rt_meshops.hip.h refit_up_kernel): parent of every pre-order node, arrival counters
    DevBuf lb_pool{bufs}, lb_pool2{bufs}, perm_dev{bufs};            // LBVH builder / layout scratch (rt_lbvh.hip.h), carved pools; visit rank -> uploaded index on the device
    rtk::LbvhArgs lb_args{};                                         // the builder's arrays of the last LBVH build (valid until the next one)
    bool host_mesh_stale = false;                                    // tri_perm / up_indices describe an older layout: the device copies (perm_dev, tidx_up) are current
    int lbvh_host_install = 0;                                       // RT_LBVH_HOST_INSTALL=1: re-lay an LBVH tree out on the host, as the reference-mode rebuild does (tests compare the two)
    rt_build_stats build{};                                          // what the last rt_mesh_rebuild_mode did
    int n_levels = 0;
    DevBuf nodesh{bufs}, tri2leaf{bufs};                            // 16-bit fixed-point sibling pairs and the triangle -> leaf table (rt_qnodes.hip.h)
    DevBuf leaflh{bufs};                                            // (lo, hi) of each triangle's leaf, by triangle (the flagged-leaf check of the fixed-point kernels)
    DevBuf nodesw{bufs}, qdp_parent{bufs}, qdp_cnt{bufs}, qdp_g{bufs}, qdp_ch{bufs};   // 4-wide fixed-point nodes (RT_TRAVQ_QW) and the scratch of the DP that picks which four nodes a quad holds (rt_qnodes.hip.h)
    unsigned chain_nonce[8] = {};                                   // launch chains started so far, PER SUB-FRAME (WfState::nonce): every part owns its own region of the ray queue, so each
                                                                    // region must cycle through all four values (one context-wide counter gave a part only two of them with two parts: ADVICE round 4)
    int q16_leaf_shift = 0;                                         // where a leaf's triangle count sits in its payload word (rtk::q16_leaf_shift), 0 = leaves too large
    bool q16_topo_ok = false;                                       // the tree's shape allows them (leaf sizes, node count, boxes nest)
    bool qw_topo_ok = false;                                        // ... and no leaf is empty: places 0 and 2 of a quad must hold a node (the pairs cope with an empty leaf)
    // One record per mesh WITH triangles, in object order: the only description of the scene's meshes (a one-mesh scene is a forest of one, without a synthetic node).
    // Invariant: whenever have_scene is true, `parts` (and, for more than one part, forest_arr / pre_of) describe ctx->scene.  With more than one part the plain
    // rt_mesh_set_normals / rebuild / set_texture are refused (the *_of entries address one mesh).  parts_valid: the last rt_scene_upload* (or rebuild) returned RT_OK; it is
    // cleared at the top of every rt_scene_upload*, so that after a failed upload the *_of and texture entries answer RT_ERR_NO_SCENE (the plain entries look at have_scene alone).
    struct MeshPart {
        int obj;                                                    // object slot (position in Scene::objects)
        int voff, nv;                                               // vertex range in `verts`
        int tri_off, nt;                                            // triangle range in the uploaded order (tidx_up, up_indices)
        int noff, nn;                                               // node range in forest_arr (bvh_arr10 indices)
        bool smooth;                                                // its entries of `nrm` are set (rt_mesh_set_normals_of)
    };
    std::vector<MeshPart> parts;
    bool parts_valid = false;
    std::vector<float> forest_arr;                                  // the forest's bvh_arr10 as installed (build_forest): topology and triangle ranges of every mesh (boxes: see pre_of)
    std::vector<int> pre_of;                                        // forest_arr index -> pre-order index of the same node on the device (node_lo / node_hi hold its current box)
    int n_syn = 0, syn[rtk::kMaxSynthetic] = {};                    // the forest's synthetic union nodes (pre-order indices): refit_kernel widens them as build_forest does
    DevBuf node_lo{bufs}, node_hi{bufs}, nodes2{bufs}, nodesq{bufs}, nodesb{bufs}, q2thr{bufs}, tri{bufs}, verts{bufs}, tidx{bufs}, scratch_rgba{bufs}, scratch_rgb8{bufs}, work{bufs}, queue{bufs};
    // rt_mesh_snapshot_vertices: `verts` as they were when a mesh was last snapshotted (n_verts float4, the same indexing; allocated by the first snapshot) and the objects
    // whose range of it is current.  Read by rt_render_aov_motion* alone: nothing a render reads, so no still-view cache hangs on it.  rt_scene_upload* clears the mask.
    DevBuf verts_prev{bufs};
    uint32_t snap_mask = 0;
    Event snap_ev;                                                   // the last snapshot's copy on the context's stream: a motion call on ANOTHER stream waits for it
    // rt_mesh_compute_normals[_of] (rt_normals.hip.h): the adjacency of the scene's position vertices in CSR form -- vcsr_off: n_verts + 1 offsets; vcsr_rank: per vertex the
    // visit ranks of the corners that name it, ascending in the uploaded triangle order -- built on the host by the first call and kept until the triangle order or the
    // visit order changes (rt_scene_upload*, every rebuild); vnrm: the normals it computes (n_verts float4, indexed like `verts`) and vnrm_mask the objects whose range of
    // it was written since the upload (rt_mesh_get_vertex_normals).
    DevBuf vcsr_off{bufs}, vcsr_rank{bufs}, vnrm{bufs};
    bool vcsr_valid = false;
    uint32_t vnrm_mask = 0;
    // rt_mesh_snapshot_normals: `nrm` as it was when a smooth mesh was last snapshotted (3 n_tris float4, by visit rank; allocated by the first snapshot), the objects whose
    // range of it is current, and the event of the last copy.  Read by rt_render_aov_motion* alone.  Indexed by visit rank: an upload AND every rebuild clear the mask.
    DevBuf nrm_prev{bufs};
    uint32_t nsnap_mask = 0;
    Event nsnap_ev;
    int n_cus = 0;
    DevBuf wfM{bufs}, wfT{bufs}, wfLS{bufs}, wfSID{bufs}, wfSamp{bufs};   // wavefront path state (HBM); wfSamp / wfT: per-sample colours and their running sum (num_rays > 1)
    DevBuf wfDCH{bufs};                                             // ... the dead-channel byte of each path (wf_dead_channels)
    unsigned long long dead_counts[4] = {};                          // of the last rt_count_work: rt_dead_channel_counts
    unsigned long long dead_last_count = 0;                          // ... and rt_dead_last_count
    // A still view's three levels (rt_still.h): per pixel slot of each sub-frame at its pxbase, the traversal result of the camera ray (8 bytes), of
    // segment 0's shadow ray (8 bytes) and the path after its shaded first hit (32 bytes, rtk::WfShade; allocated only once a chain may store it).  `still` says which
    // parts of them hold what, under which keys (rt_host_render.hip.h still_begin)
    DevBuf wfM0{bufs}, wfX0{bufs}, wfS0{bufs};
    rtk::StillView still;
    DevBuf wfL3{bufs};                                              // ... and the three-channel direct term of each diffuse segment (wf_advance<kFormSkySample>; allocated by the first sampling frame)
    DevBuf wfALB{bufs};                                             // ... and the albedo of each textured diffuse segment (wf_advance<kFormTex>; allocated by the first textured frame)
    DevBuf wfQR{bufs};                                              // traversal queue in slot order: the rays (32 B each)
    DevBuf pathSamp{bufs}, pathT{bufs};                             // wf_path with num_rays > 1: per-sample colours, running sum
    DevBuf dbgbuf{bufs};                                            // -DRT_DEBUG builds: per-wave traversal records
    DevBuf batch_dev{bufs};                                         // rt_render_device_batch: the frames' descriptors, one copy per sub-frame
    DevBuf anim_dev{bufs};                                          // rt_render_device_batch_scenes: the frames' lights and sphere poses (rtk::AnimFrame), one copy per sub-frame
    DevBuf aovM{bufs}, aovQR{bufs};                                 // rt_render_aov*: traversal results and ray queue of its own (the render path's are never touched)
    DevBuf aov_state{bufs};                                         // rt_render_aov_surface*: one record per pixel between the rounds of its chain (rtk::SurfState)
    DevBuf dn_tmp{bufs};                                            // rt_denoise*: the ping-pong frame of the passes
    DevBufs<2> dnv_var{bufs};                                        // rt_denoise_var*: the variance planes between passes
    DevBuf post_io{bufs};                                           // the host forms of rt_render_aov*, rt_denoise*, rt_temporal_accumulate, rt_[de]modulate: inputs and result (staged, rt_host_post.hip.h)
    DevBuf accum{bufs};                                             // progressive mode: sum of the frames so far (float4 per pixel)
    // rt_render_counts* (rt_adaptive.hip.h): the plan's workgroup totals and their offsets, offs[] and the item records; the list chains' own ray queue (the dense
    // chains' queue, its zero fill and its chain numbers are never touched) and the running sums of a list cut into several chains.  The rest of a list chain's
    // state is the dense chain's buffers (wfM, wfSamp, wfLS, wfSID, wfDCH, wfALB)
    DevBuf adTot{bufs}, adOffs{bufs}, adItems{bufs}, adQR{bufs}, adT{bufs};
    uint64_t ad_qf_sig = 0;                                         // layout adQR was last zeroed for
    unsigned ad_nonce = 0;                                          // list chains started so far (WfState::nonce)
    uint64_t ad_info[4] = {};                                       // of the last rt_render_counts*: items traced, chains, pixel slots, paths of the largest chain (rt_render_counts_info)
    int prog_frames = 0, prog_w = 0, prog_h = 0;
    uint64_t qf_sig = 0;                                            // layout the queue flags were last zeroed for
    // workgroups per CU of the kernels whose grid is sized by it (blocks_per_cu: asked once, 0 = not yet), each slot + STATS: wf_trav; wf_travq (+ 2 * (R == 32) + 4 * (R == 128));
    // its 4-wide form; render_persistent
    enum { kOccTrav = 0, kOccTravq = 2, kOccTravqQw = 8, kOccPersist = 10, kOccSlots = 12 };
    int occ_blocks[kOccSlots] = {};
    static constexpr int kMaxParts = 8;
    Stream part_stream[kMaxParts];
    Event part_ev[kMaxParts];
    Event fork_ev;
    // Chains on streams of their own (start_chains / end_chains): consecutive chunks of one call -- and, with rt_ctx_set_pipelining, consecutive
    // frames into different buffers -- follow each other per sub-frame without a join in between.
    struct Pipe {
        bool on = false;                   // rt_ctx_set_pipelining: frames of consecutive calls may overlap
        Event fork2[2];                    // the caller's stream at the start of this call / of the previous one
        int cur = 0;
        bool valid = false, prev_valid = false;   // the call before this one ended with its chains on their own streams (joined into `stream`)
        int open_parts = 0;                // chains of an earlier chunk of THIS call that have not been joined into the caller's stream
        hipStream_t stream = nullptr;      // ... and was issued on this stream,
        uint64_t sig = 0;                  // ... with this state layout (sub-frames, sizes, offsets) in its last chunk,
        const uint8_t *out_lo = nullptr, *out_hi = nullptr;   // ... into this output range
        int call_chunk = 0, call_chunks = 1;                  // position of the chunk being issued in its call (launch_render)
        const uint8_t *call_lo = nullptr, *call_hi = nullptr; // output range of the call being issued
        hipEvent_t extra_wait = nullptr;   // this call's chains also wait for this event (rt_render_async: the slot's previous copy)
        // What the library ITSELF put on the caller's stream since the previous render call and what that work touches (rt_tonemap_device:
        // reads a frame, writes an image).  A frame that starts behind the PREVIOUS call does not wait for it, so a frame whose output overlaps
        // one of these ranges must not take the relaxed start: the product falls back to the full fork, a -DRT_DEBUG build refuses the call
        // with RT_ERR_INVALID so that the caller learns its sequence breaks the rule of rt_ctx_set_pipelining.  (Work the caller submits
        // through HIP directly is invisible to the library: no run-time check can cover it.)
        struct Range { const uint8_t *lo, *hi; hipStream_t stream; };
        std::vector<Range> between;
        bool between_overflow = false;     // more than 64 ranges came in between two render calls: treated as a hazard
    } pipe;
    bool trav_attr_set = false;
    bool stats_on = false;                                          // rt_stats_enable: bracket the traversal launches with timing events (production frames record none)
    static constexpr int kSlots = 2;                                // rt_render_async: double-buffered device frames, one copy stream
    DevBufs<kSlots> slot_rgba{bufs}, slot_rgb8{bufs};
    Event slot_rendered[kSlots], slot_done[kSlots];
    bool slot_pending[kSlots] = {false, false};
    Stream copy_stream, copy_stream2;                               // two copy streams: the halves of a frame go out through two DMA engines
    Event slot_half[kSlots];
    bool travq_ok = true;                                           // the uploaded tree fits wf_travq's entry formats (leaf sizes, triangle offsets)
    static constexpr int kMaxTravEvents = 2 * RT_MAX_SEGMENTS;
    Event ev_trav[2 * kMaxTravEvents];
    Event ev_adv[2 * kMaxTravEvents];                               // ... and of the uniform kernel's launches (rt_stats_enable)
    int n_trav_events = 0, n_adv_events = 0, adv_paths = 0;
    rt_stats stats{};
    std::string err;
    char name[256] = {0};

    rt_ctx() = default;
    rt_ctx(const rt_ctx &) = delete; rt_ctx &operator=(const rt_ctx &) = delete;   // (bufs points at the members; a context lives on the heap from rt_ctx_create to rt_ctx_destroy)
    // Ordering, not ownership: nothing of the context is given back while one of its streams still runs -- its own, the sub-frame chains of frames issued on a caller's
    // stream, the copies of rt_render_async.  The members then release themselves.
    ~rt_ctx() {
        (void)hipSetDevice(device);
        if (stream_) (void)hipStreamSynchronize(stream_);
        for (hipStream_t q : part_stream) if (q) (void)hipStreamSynchronize(q);
        if (copy_stream) (void)hipStreamSynchronize(copy_stream);
        if (copy_stream2) (void)hipStreamSynchronize(copy_stream2);
    }
};

namespace {

// The stream a call runs on when the caller passes none.  Created on first use: a context driven on the caller's streams (bench.py,
// rt_render_device with a stream) owns no stream of its own -- idle streams still take part in the runtime's mapping of streams onto
// its few hardware queues.
hipStream_t own_stream(rt_ctx *ctx) {
    if (!ctx->stream_) {
        (void)hipSetDevice(ctx->device);
        const hipError_t e = ctx->stream_.create();
        if (e != hipSuccess) { (void)hipGetLastError(); ctx->err = std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e); g_last_error = ctx->err; }
    }
    return ctx->stream_;   // nullptr: the entry points fail with RT_ERR_HIP (RT_OWN_STREAM) rather than fall back to the legacy default stream
}

// RT_TIMING=1: host-side wall time of the library's start-up phases on stderr (rt_launcher --timing 1 sets it): where a short program's time goes
// -- runtime initialisation, the first launch's code-object load, uploads, the frame itself, the copy back.
struct PhaseClock {
    bool on;
    std::chrono::steady_clock::time_point t;
    PhaseClock() : on([] { const char *e = getenv("RT_TIMING"); return e && *e && atoi(e) != 0; }()), t(std::chrono::steady_clock::now()) {}
    void lap(const char *what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "timing: %-44s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

int fail(rt_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (ctx) ctx->err = buf;
    return code;
}

#define RT_HIP(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) return fail(ctx, RT_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// Entry points that run on the context's own stream: its creation must have succeeded (a failure used to fall back to
// stream 0 without a word).
#define RT_OWN_STREAM(ctx)                                                                              \
    do {                                                                                                \
        if (!own_stream(ctx)) return fail(ctx, RT_ERR_HIP, "the context's stream: %s", (ctx)->err.c_str()); \
    } while (0)

// Every allocation happens on the context's device, whatever the calling thread's current device is.
int ensure(rt_ctx *ctx, DevBuf &b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return RT_OK;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    b.release();
    RT_HIP(ctx, hipMalloc(&b.p, bytes ? bytes : 16));
    b.bytes = bytes ? bytes : 16;
    return RT_OK;
}

// what wf_advance<kFormTex> and kat_surface_kernel read of the textures (ALB: set per launch)
rtk::TexScene tex_scene(const rt_ctx *ctx) {
    rtk::TexScene ts{};
    ts.uv = static_cast<const float2 *>(ctx->tex_uv.p);
    ts.desc = static_cast<const rtk::TexDesc *>(ctx->tex_table.p);
    ts.mask = ctx->tex_mask;
    return ts;
}

// Host -> device, complete on return.  (hipMemcpy = the NULL stream.  Round 6 tried the context's own stream instead, to spare a C++ program one hardware queue: the ~27 ms the
// FIRST copy of a process costs -- the runtime creating a queue and its staging -- just moved to that stream, and the headline frame read 1 % slower:
// profiles/round6/launcher_timing.txt.)
int upload(rt_ctx *ctx, DevBuf &b, const void *src, size_t bytes) {
    int rc = ensure(ctx, b, bytes);
    if (rc != RT_OK) return rc;
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (bytes) RT_HIP(ctx, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}


}  // namespace
