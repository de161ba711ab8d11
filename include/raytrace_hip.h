/*
 * raytrace_hip.h -- C-ABI of libraytrace_hip.so: the MI355X (gfx950) render path.
 *
 * Drop-in boundary for the per-pixel render of souhhcong/RaytracingGPU.  The
 * reference has no library interface: its render path is the CUDA sequence in
 * optimized.cu main() --
 *     cudaMalloc/cudaMemcpy of arr_bvh, indices, vertices      (optimized.cu:811-826)
 *     KernelLaunch<<<H*W/128,128,smem>>>(d_colors, W, H, num_rays, num_bounce,
 *                  d_indices, ni, d_vertices, nv, d_arr_bvh)   (optimized.cu:828-847)
 *     cudaDeviceSynchronize + cudaMemcpy D2H of the image      (optimized.cu:849-856)
 * -- and, on the CPU, the pixel loop of cpu_launcher.cpp:693-718.  Each entry point
 * below names the reference lines it replaces.  Plain pointers and sizes only; no
 * HIP, torch or C++ types cross this boundary.  Every function returns RT_OK (0) or
 * a negative rt_status, never exits and never throws (the reference's gpuErrchk
 * prints and calls exit(), optimized.cu:24-30).
 *
 * Result contract: for sigma == 0 the linear float colour written by rt_render* is
 * bit-identical to cpu_launcher.cpp's Scene::getColor average (color_avg, cpu:713)
 * when the reference's uniform() is replaced by the counter RNG of DESIGN.md; the
 * 8-bit image is cpu:714-716.  There is no CPU fallback in this library.
 */
#ifndef RAYTRACE_HIP_H
#define RAYTRACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6
#define RT_MAX_SPHERES 16      /* reference: Geometry* objects[10], optimized.cu:663 */
#define RT_MAX_OBJECTS 16      /* spheres + meshes of one scene (Scene::objects, cpu:538-543)                     */
#define RT_MAX_SEGMENTS 16     /* reference: MAX_RAY_DEPTH 10, optimized.cu:22       */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,       /* bad argument (message in rt_last_error)            */
    RT_ERR_NO_DEVICE = -2,     /* no gfx950 device / HIP runtime unusable            */
    RT_ERR_HIP = -3,           /* a HIP call failed (message in rt_last_error)       */
    RT_ERR_NO_SCENE = -4,      /* render before rt_scene_upload                      */
    RT_ERR_UNSUPPORTED = -5,   /* e.g. LDS variant that does not fit the mesh        */
    RT_ERR_INTERNAL = -6       /* an invariant of the library did not hold (a bug)   */
} rt_status;

/* kernel variants (BASELINE.json configs 3/4); all produce bit-identical results */
typedef enum rt_variant {
    RT_VARIANT_AUTO = 0,       /* the fastest measured variant: RT_VARIANT_WAVEFRONT_QUEUE; for a scene
                                  without a mesh (and no pose / smooth normals): RT_VARIANT_LOCKSTEP   */
    RT_VARIANT_GLOBAL = 1,     /* persistent lanes (micro-op scheduler); SoA nodes + packed
                                  triangles read from HBM through L2/L1                             */
    RT_VARIANT_LDS_VERTS = 2,  /* work-stack traversal (as 8) with the vertex array staged in LDS by a
                                  cooperative copy per workgroup (different-versions/
                                  optimized_vertices-in-shared.cu:681-686): a triangle test reads three
                                  indices + three LDS vertices; one workgroup per CU; RT_ERR_UNSUPPORTED
                                  when the vertices leave no room for a wave's carve in the 160 KB    */
    RT_VARIANT_LDS_TOP = 3,    /* work-stack traversal with the top BVH levels (breadth-first prefix of
                                  the node array, all of it if it fits) staged in LDS                */
    RT_VARIANT_LDS_ALL = 4,    /* both: vertices + as much of the top of the BVH as fits beside them  */
    RT_VARIANT_LOCKSTEP = 5,   /* one lane bound to one pixel for the whole frame, lock-step ray
                                  queries: the structure of KernelLaunch (optimized.cu:670-772);
                                  kept as the baseline the other variants are measured against      */
    RT_VARIANT_WAVEFRONT = 6,  /* uniform per-pixel shade/generate kernels alternating with a lean
                                  persistent traversal kernel; path state as float4 SoA in HBM;
                                  BVH nodes and triangles read from HBM through L2/L1               */
    RT_VARIANT_WAVEFRONT_LDS = 7, /* the same with every BVH node staged in LDS (one 1024-thread
                                  workgroup per CU shares the copy); RT_ERR_UNSUPPORTED when the
                                  nodes do not fit the 160 KB                                       */
    RT_VARIANT_WAVEFRONT_QUEUE = 8, /* wavefront pipeline whose traversal kernel keeps a per-wave LDS
                                  work stack of (ray slot, sibling pair) entries: every lane tests the two
                                  boxes of a pair, or two triangles, per step; no per-lane walk
                                  (rt_travq.hip.h).  The default (RT_VARIANT_AUTO)                  */
    RT_VARIANT_PATH = 9        /* the whole render in ONE persistent launch: a wave owns 64 paths (one per lane) from
                                  camera ray to framebuffer store; the work-stack traversal and the
                                  shading of ready paths alternate inside the wave, path state lives
                                  in LDS, nothing but the pixel leaves the CU (rt_path.hip.h)       */
} rt_variant;

typedef struct rt_ctx rt_ctx;

/* Sphere(C, R, albedo, mirror, n_in, n_out): cpu_launcher.cpp:505-511, Geometry cpu:106-118 */
typedef struct rt_sphere {
    float   center[3];
    float   radius;
    float   albedo[3];
    int32_t mirror;
    float   in_refraction_index;
    float   out_refraction_index;
} rt_sphere;

/* The mesh exactly as optimized.cu hands it to KernelLaunch (optimized.cu:670, 811-826):
 * Vector vertices[nv] (3 x f32), TriangleIndices indices[nt] in BVH order (only
 * vtxi,vtxj,vtxk are read, optimized.cu:271) and the bvhTreeToArray float[10] node array
 * (optimized.cu:512-534: [0]=left [1]=right(-1 leaf) [2..4]=mn [5..7]=mx [8]=tri_start [9]=tri_end). */
typedef struct rt_mesh {
    const float   *vertices;       /* n_vertices * 3                                          */
    int32_t        n_vertices;
    const int32_t *indices;        /* vtxi,vtxj,vtxk of triangle t at indices[t*index_stride] */
    int32_t        index_stride;   /* 3 = compact, 10 = sizeof(TriangleIndices)/4             */
    int32_t        n_triangles;
    const float   *bvh_arr10;      /* n_nodes * 10                                            */
    int32_t        n_nodes;
    float          albedo[3];      /* mesh_ptr->albedo, cpu:683                               */
    int32_t        object_slot;    /* position in Scene::objects (cpu_launcher: 6 = last,
                                      optimized.cu:690-700: 1); decides exact-tie order cpu:554 */
    /* ABI 6: the rest of Geometry (cpu:106-118), which a TriangleMesh inherits like a Sphere does and Scene::getColor reads
     * for WHICHEVER object was hit (cpu:573 objects[id]->mirror, cpu:580 the two indices).  A zero-initialised rt_mesh
     * (0 / 0 / 0) is the diffuse mesh of Geometry() (cpu:110: mirror 0, indices 1 / 1): equal indices take the diffuse branch. */
    int32_t        mirror;
    float          in_refraction_index;
    float          out_refraction_index;
} rt_mesh;

/* Scene::L / Scene::intensity (cpu:650-651), camera C and alpha (cpu:666,691) */
typedef struct rt_light  { float position[3]; float intensity; } rt_light;
typedef struct rt_camera { float position[3]; float fov; } rt_camera;

typedef struct rt_params {
    int32_t  width, height;        /* W,H (reference: 512, cpu:661-662)                       */
    int32_t  num_rays;             /* argv[1], cpu:659                                        */
    int32_t  num_bounce;           /* argv[2], cpu:659                                        */
    int32_t  depth_convention;     /* 0: cpu_launcher, b => b+1 segments (cpu:567)
                                      1: optimized.cu, b => b segments (optimized.cu:566)     */
    float    sigma;                /* anti-aliasing jitter: 0 (cpu:704) / 0.2 (optimized.cu:753) */
    float    eps;                  /* 1e-3 (cpu:575) / 1e-4 (optimized.cu:575)                */
    float    tri_tmin;             /* 1e-4f (cpu:301) / 0 (optimized.cu:275)                  */
    uint32_t seed;                 /* counter RNG seed; optimized.cu:745 uses 123456          */
    int32_t  variant;              /* rt_variant                                              */
} rt_params;

/* Which rows a call renders.  Local row r (0 <= r < n_rows) is image row
 *     row0 + (r / tile_rows) * tile_rows * tile_step + (r % tile_rows).
 * Contiguous range [a,b): {a, b-a, b-a, 1}.  Interleaved tiles of rank k of G
 * (SURVEY 8e): {k*R, n_local_rows, R, G}. */
typedef struct rt_rows {
    int32_t row0;
    int32_t n_rows;
    int32_t tile_rows;
    int32_t tile_step;
} rt_rows;

typedef struct rt_stats {
    float    kernel_ms;            /* HIP-event time of the last render kernel                */
    float    tonemap_ms;           /* of the last tonemap kernel (0 if none)                  */
    uint64_t pixels;               /* pixels of the last render call                          */
    int32_t  variant;              /* variant that actually ran                               */
    int32_t  lds_bytes;            /* dynamic + static LDS per workgroup                      */
    int32_t  block_threads;
    int32_t  grid_blocks;
    float    trav_ms;              /* wavefront variant: summed HIP-event time of the traversal kernel
                                      launches of the last sample of the last frame, and how many    */
    int32_t  trav_launches;
    int32_t  parts;                /* wavefront variant: concurrent sub-frames the call was cut into      */
    int32_t  adv_launches;         /* ... and the same for the uniform kernel (wf_advance, the launches after the first): */
    float    adv_ms;               /*     summed HIP-event time, launches, paths per launch (rt_stats_enable)             */
    int32_t  adv_paths;
    int32_t  travq_mode;           /* work-stack traversal kernel of the last render: 0 = sibling pairs (64-byte float nodes), 1 = 16-bit fixed-point pairs,
                                      2 = 4-wide fixed-point nodes (the default wherever the format fits: boxes nest, leaves of 1 .. 127 triangles, fewer than 2^21 nodes);
                                      -1 = another traversal kernel / no mesh */
    int32_t  reserved;
} rt_stats;

/* --- device / context -------------------------------------------------------- */
/* replaces the implicit CUDA device 0 of optimized.cu */
int rt_abi_version(void);
int rt_device_count(int *count);
int rt_ctx_create(rt_ctx **ctx, int device_id);
int rt_ctx_destroy(rt_ctx *ctx);
const char *rt_last_error(const rt_ctx *ctx);          /* ctx may be NULL: last global error */
int rt_device_name(const rt_ctx *ctx, char *buf, size_t buflen);

/* --- scene upload: replaces optimized.cu:811-826 (H2D of arr_bvh/indices/vertices)
 *     and the in-kernel scene construction optimized.cu:679-726 --------------------
 * All host arrays are copied; the caller keeps ownership.  mesh may be NULL
 * (spheres only: what the reference renders when the OBJ is missing, cpu:322-325). */
int rt_scene_upload(rt_ctx *ctx, const rt_sphere *spheres, int n_spheres, const rt_mesh *mesh,
                    const rt_light *light, const rt_camera *camera);
/* ... with any number of meshes (ABI 6): Scene::objects is a std::vector<Geometry*> scanned in insertion order with a strict '<'
 * (cpu:538-564; optimized.cu:663 `Geometry* objects[10]`), so a scene may hold several TriangleMesh objects at any positions.
 * meshes[k].object_slot are distinct positions in [0, n_spheres + n_meshes); the spheres fill the remaining positions in array
 * order.  At most RT_MAX_OBJECTS objects.  Each mesh keeps the tree its own buildBVH made (cpu:190-224) and its own root-box test
 * (cpu:279); inside the library the trees hang below synthetic nodes whose boxes are the unions of their children, the triangles
 * are stored mesh after mesh in object order, and one traversal finds the minimum over (t, object position, scan rank) -- the
 * result of the reference's loop over the objects.  A mesh without triangles stays an object that is never hit (missing OBJ,
 * cpu:322-325).  Every kernel variant renders such scenes.  With more than one mesh that has triangles the plain per-mesh operations -- rt_mesh_set_normals, rt_mesh_rebuild* --
 * are refused (RT_ERR_UNSUPPORTED) and rt_mesh_transform moves them all; rt_mesh_transform_of / rt_mesh_set_normals_of / rt_mesh_rebuild_of (below) address ONE mesh by
 * its object_slot. */
int rt_scene_upload_meshes(rt_ctx *ctx, const rt_sphere *spheres, int n_spheres, const rt_mesh *meshes, int n_meshes,
                           const rt_light *light, const rt_camera *camera);

/* --- render: replaces KernelLaunch + cudaDeviceSynchronize + D2H, optimized.cu:828-856,
 *     i.e. the pixel loop cpu:693-713.  Output: n_rows*width float4, .xyz = linear
 *     colour average (color_avg, cpu:713), .w = rays traced for the pixel. ------- */
int rt_render(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, float *out_rgba_host);
/* same, into device memory, asynchronous on `stream` (a hipStream_t, NULL = the
 * context's own stream); rows may be interleaved tiles (multi-GPU) */
int rt_render_device(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, void *out_rgba_dev, void *stream);

/* --- a BATCH of frames in one launch chain (ABI 6).  A process that renders a small share of every frame -- one rank of eight on 1920x1080 owns
 *     0.26 Mpixel -- cannot fill the chip with the eleven dependent launches of ONE such frame, and a frame per stream runs out of hardware queues
 *     (four per process).  Here n_frames (<= RT_MAX_BATCH) frames of the same size and rows are traced as the items of ONE chain -- the machinery
 *     that traces the samples of a pixel as parallel items -- each with its OWN camera (position, fov: cpu:666, 691-699), its own seed and its own
 *     output buffer: a sequence of frames of a moving camera / a progressive render, not one frame repeated.  Frame k's buffer holds exactly what
 *     rt_render_device writes for the scene with that camera and p->seed = frames[k].seed (bit for bit: per-pixel arithmetic does not depend on
 *     what else is in the launch).  num_rays == 1; wavefront variants; p->seed is ignored; asynchronous on `stream`.  Throughput, not latency: the
 *     n frames finish together.  Replaces n x (KernelLaunch + sync, optimized.cu:828-849). */
#define RT_MAX_BATCH 16
typedef struct rt_frame_desc {
    rt_camera camera;              /* this frame's camera (Camera C / alpha, cpu:666,691)      */
    uint32_t  seed;                /* this frame's counter-RNG seed (rt_params.seed)           */
    uint32_t  reserved;
    void     *out_rgba_dev;        /* n_rows * width float4, as rt_render_device               */
} rt_frame_desc;
int rt_render_device_batch(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, const rt_frame_desc *frames, int n_frames, void *stream);

/* --- an ANIMATED scene (ABI 6, additive): the light and the spheres of the scene in use, changed in place.  realtime_render.cu moves them between two frames
 *     of a running sequence with two one-thread kernels, MoveLightSource (:1072-1090) and MoveObject (:1092-1098); here they are the part of the scene that lives
 *     in the kernels' arguments, so an edit is a host-side store: no mesh is re-sent or re-laid out, and smooth normals, textures, device-side transforms and
 *     rebuilt trees stay as they are (rt_kat_layout_hash does not change) -- where a new rt_scene_upload* would drop all of them.
 *       get / set_light   Scene::L and Scene::intensity (cpu:650-651);
 *       get / set_sphere  the sphere at position object_slot of Scene::objects (as rt_mesh.object_slot and MoveObject's `index` count): geometry AND material;
 *       move_sphere       MoveObject: C' = C + v * dt per component in binary32, the product first (two roundings) -- reproducible exactly;
 *       move_light        MoveLightSource: get, rt_light_orbit, set;
 *       rt_light_orbit    (host function, no context) the light turned about the y axis through the origin: radius = sqrtf(x * x + z * z) (the reference's
 *                         powf(d, 2) as d * d), angle = atan2f(z, x) + angular_speed * dt, x' = radius * cosf(angle), z' = radius * sinf(angle), y and the
 *                         intensity untouched; binary32 throughout, with the host's C library.  Pinned: MoveLightSource itself, run as a host function with the same C library, gives the
 *                         same bits for 100 lights and a chain of 20 steps (tests/golden/ref_realtime.npz, tests/test_realtime_pinned.py; MoveObject likewise); x', z' are also
 *                         held to the formula in binary64 within 16 * 2^-24 * radius.
 *     Contract: after any sequence of these calls every render entry (rt_render*, _device, _batch, _async, _pose*, rt_progressive_frame, rt_trace_rays,
 *     rt_count_work; every rt_variant) produces, bit for bit, what it produces after rt_scene_upload* of the same meshes with the edited light / spheres:
 *     what an upload derives from a sphere (R * R as one binary32 product, the per-object centre, mirror bit, albedo and indices) is derived again by the same code.
 *     A frame uses the scene as it is when its render call is made: kernel arguments are captured at launch, so an edit between two frames in flight
 *     (rt_ctx_set_pipelining, rt_render_async) needs no synchronisation.  Progressive accumulation is the caller's to reset (rt_progressive_reset; buffer_reset,
 *     realtime:1246-1250).  RT_ERR_INVALID, scene unchanged: object_slot outside the scene or a mesh's.  RT_ERR_NO_SCENE: no upload, or the last rt_scene_upload*
 *     failed.  rt_multi_* contexts have no such entries: upload again. ------------------------------------------------------------------------------------ */
int rt_scene_get_light(const rt_ctx *ctx, rt_light *out);
int rt_scene_set_light(rt_ctx *ctx, const rt_light *light);
int rt_scene_get_sphere(const rt_ctx *ctx, int object_slot, rt_sphere *out);
int rt_scene_set_sphere(rt_ctx *ctx, int object_slot, const rt_sphere *sphere);
int rt_scene_move_light(rt_ctx *ctx, float angular_speed, float dt);                       /* MoveLightSource, realtime:1072-1090 (dt there: 2e-2f) */
int rt_scene_move_sphere(rt_ctx *ctx, int object_slot, const float v[3], float dt);        /* MoveObject, realtime:1092-1098 (dt there: 0.2)         */
int rt_light_orbit(const rt_light *in, float angular_speed, float dt, rt_light *out);      /* in == out is allowed                                    */

/* --- SEVERAL POINT LIGHTS (ABI 6, additive).  A scene holds n lights, 1 <= n <= RT_MAX_LIGHTS.  A diffuse segment still emits ONE shadow ray: to the light that the
 *     sample's key picks with probability proportional to its intensity.  With that choice the estimator's weight I_k / p_k is the same number for every light -- the
 *     total intensity -- so the frame is an unbiased estimate of the sum of the n one-light frames (direct AND indirect light) at the cost of one of them.
 *     THE RULE, in binary32 with one rounding per operation:
 *       prefix[0] = I_0;  prefix[k] = fl(prefix[k - 1] + I_k);  total = prefix[n - 1].
 *       Segment d of a path whose sample key is hs = sample_hash(pixel_hash(...), samp) -- the key the segment's bounce already uses -- draws
 *       r = uniform01(hs, d + 1, 2),  x = fl(r * total),  and k = the least index with prefix[k] >= x and prefix[k] > 0.
 *       (Depth d + 1 with dim 2 collides with nothing: the jitter reads depth 0 with dims 2 and 3, the bounce of segment d depth d with dims 0 and 1.)
 *       The segment's shadow ray goes to L_k and its direct term is direct_term(total, L_k, P, N): the position is L_k's, the only intensity the shading sees is `total`,
 *       I_k is never used on its own.  Everything else is the one-light code on the operand L_k (shadow direction, any-hit bound, sphere shadowing, cpu:615, the moot-ray
 *       and dead-channel rules).  The launch that closes the shadow ray picks k again from (hs, d): no path state is added.
 *     What follows from the rule:
 *       r lies in (0, 1], so x <= total and a k always exists;
 *       a light of intensity 0 is never picked, whatever r is (prefix[k] == prefix[k - 1] >= x would have picked an earlier light; in front, prefix[k] > 0 fails);
 *       GRANULARITY: a light that the running sum absorbs (prefix[k] == prefix[k - 1], as 1 after 1e10) is never picked either -- order a list of very unequal
 *       lights by rising intensity.
 *     The list is host state like the one light: no device memory is written, and a frame in flight keeps the table its launches captured.
 *       rt_scene_upload*        leaves a list of the one uploaded light;        rt_scene_set_light   replaces the list with one light;
 *       rt_scene_get_light      answers light 0;                                rt_scene_set_lights  replaces the list (n == 1: rt_scene_set_light);
 *       rt_scene_get_lights     n always receives the count; out receives the list if cap >= count, cap == 0 asks for the count alone (out may be NULL);
 *       rt_scene_set_light_at   replaces light k of the list;                   rt_scene_move_light_at  get, rt_light_orbit on light k, set.
 *     With n == 1 every call and every frame is what it is without these entries, launch for launch.  RT_ERR_INVALID, list untouched: a NULL pointer, n outside
 *     [1, RT_MAX_LIGHTS], k outside the list, cap below the count; and for a list of several: an intensity whose sign bit is set or that is not finite, a total that is
 *     not finite or is 0.  (One light: whatever rt_scene_set_light accepts.)
 *     While n > 1: rt_render*, _device, _device_batch, _async, _pose*, rt_progressive_frame render it through the wavefront variants (auto, wavefront, wavefront_lds,
 *     wavefront_queue, lds_*; auto never resolves to lockstep); several samples, row shares and a posed camera included.  A still view keeps and uses the camera rays'
 *     hits but neither the first shadow rays nor the shaded first hits: segment 0's shadow ray depends on the sample.  RT_ERR_UNSUPPORTED, outputs untouched:
 *     rt_render_device_batch_scenes with scenes, rt_render_counts*, rt_count_work, the variants path, lockstep and global.  rt_multi_* contexts have no such
 *     entries and always hold one light. */
#define RT_MAX_LIGHTS 16
int rt_scene_set_lights(rt_ctx *ctx, const rt_light *lights, int n);
int rt_scene_get_lights(const rt_ctx *ctx, rt_light *out, int cap, int *n);
int rt_scene_set_light_at(rt_ctx *ctx, int k, const rt_light *light);
int rt_scene_move_light_at(rt_ctx *ctx, int k, float angular_speed, float dt);

/* --- SOFT SHADOWS: point lights with a radius (ABI 6, additive).  Light k of the list has a radius rho_k >= 0: it is a shell of isotropic point emitters of total
 *     intensity I_k on the sphere of radius rho_k about L_k.  It is NOT geometry: camera, bounce and shadow rays pass through it and it occludes nothing.  A diffuse
 *     segment still emits ONE shadow ray, to one point of the shell of the light it picks, so the frame is an unbiased estimate of the sum, over the shell, of the
 *     point-light frames ("several point lights" above): nothing of Scene::getColor is restated differently.
 *     THE RULE.  Segment d of the path with sample key hs picks k as above.  While any radius of the list is above 0 it then does, in binary32 with one rounding per
 *     operation:
 *       r1 = uniform01(hs, D + d, 0),  r2 = uniform01(hs, D + d, 1)  with D = 1u << 29.  (The RNG keys on depth * 4 + dim modulo 2^32: these draws sit at 2^31 + 4 d + dim.
 *       Every draw in use -- jitter, bounce, pick -- sits below 4 (segs + 1): nothing collides.  Dim 3 at depth d + 1 alone would give only one free number.)
 *       z = 1 - 2 r1                           in [-1, 1): -1 is reached (r1 = 1), 1 is not (r1 > 0); exact
 *       s = rt_sqrtf(1 - z z)                  (z z <= 1: never negative)
 *       (sn, cs) = rt_sincos_2pi(2 pi (double)r2)
 *       x = (float)(cs (double)s),  y = (float)(sn (double)s)                      -- the forms cosine_bounce uses
 *       L' = L_k + rho_k (x, y, z)             per component, the product first.
 *     The shadow ray goes to L' and the direct term is direct_term(total, L', P, N); everything else is the one-light code on the operand L' (shadow direction, any-hit
 *     bound, the sphere decision at emission, cpu:615 at the close, the moot-ray and dead-channel rules).  The launch that closes the shadow ray derives L' again from
 *     (hs, d): no path state is added.  A light of rho_k == 0 in a soft list uses L_k itself: the addition is skipped, a -0 coordinate keeps its bits.
 *     The radii are host state beside the list; a frame in flight keeps what its launches captured.
 *       rt_scene_upload*, rt_scene_set_light, rt_scene_set_lights            leave every radius 0: the new light replaces the old;
 *       rt_scene_set_light_at, rt_scene_move_light_at, rt_scene_move_light   keep the radius of the light they touch, in a list of one too: a lamp that moves keeps its size;
 *       rt_scene_set_light_radii       n must equal the list's count;        rt_scene_set_light_radius_at   the radius of light k;
 *       rt_scene_get_light_radii       the cap / count convention of rt_scene_get_lights.
 *     RT_ERR_INVALID, radii and list untouched: a NULL pointer, n different from the count, k outside the list, cap below the count, a radius whose sign bit is set or
 *     that is not finite.  A list of ONE soft light takes whatever intensity rt_scene_set_light takes.
 *     "Soft": some radius of the list is above 0.  With every radius 0 every call and every frame is what it is without these entries, launch for launch.  A soft scene
 *     behaves everywhere as a scene of several lights does, a list of one included: the wavefront variants render it (auto never resolves to lockstep), a still view keeps
 *     and uses the camera rays' hits only, and rt_render_device_batch_scenes with scenes, rt_render_counts*, rt_count_work and the variants path, lockstep and global
 *     answer RT_ERR_UNSUPPORTED with their outputs untouched.  A radius that changes counts as a light change for the still view.  rt_multi_* contexts have no such entries. */
int rt_scene_set_light_radii(rt_ctx *ctx, const float *radii, int n);
int rt_scene_get_light_radii(const rt_ctx *ctx, float *out, int cap, int *n);
int rt_scene_set_light_radius_at(rt_ctx *ctx, int k, float radius);

/* --- THIN LENS: a camera with an aperture and a focus distance (ABI 6, additive).  The context carries a lens: an aperture radius R >= 0 and a focus distance f > 0, both in
 *     scene units; f is measured along the optical axis, so the plane of focus is perpendicular to the axis.  A point on the plane of focus is seen at the pinhole's pixel
 *     from every point of the lens; everything else spreads over its circle of confusion.  No counterpart in the reference: its cameras are pinholes.
 *     "Lens on": R > 0.  With R == 0 every call and every frame is what it is without these entries, launch for launch.
 *     THE RULE.  With the lens on, sample samp of pixel (px, row) does, in binary32 with one rounding per operation, with the key hs = sample_hash(pixel_hash(fr, row, px,
 *     seed), samp), O the camera position (the uploaded camera, a batch frame's camera, the pose's position), u = camera_dir(...) the unit direction as it is without a
 *     lens, jitter included (the lens composes with sigma != 0), and the basis  ex = (1,0,0), ey = (0,1,0), a = (0,0,-1)  of the fixed camera or  ex = bx, ey = by,
 *     a = -bz  of a posed one (z is negative, so the view axis is -bz; the negation is exact):
 *       c = dot(u, a)                          in dot's operand order: (u.x a.x + u.y a.y) + u.z a.z
 *       if !(c > 0) the ray stays (O, u).      (The posed camera keeps its position inside the direction -- posed_dir, the reference's own quirk: the rule is stated on u,
 *                                              whatever it is.  There c has the sign of |z| - dot(C, bz), |z| = W / (2 tan(fov / 2)), for every pixel alike: from the
 *                                              reference's default pose, C = (0, 0, 55) with fov pi / 2, a frame less than about 105 pixels wide is the pinhole's.)
 *       t = f / c                              a correctly rounded quotient
 *       F = O + t u                            per component, the product first
 *       r1 = uniform01(hs, D, 0),  r2 = uniform01(hs, D, 1)  with D = 1u << 28.  (The RNG keys on depth * 4 + dim modulo 2^32: these draws sit at 2^30 + dim.  Jitter, bounce
 *                                              and pick draws sit below 4 (segs + 1), the shell draws of soft shadows at 2^31 + 4 d + dim: nothing collides.)
 *       s = rt_sqrtf(r1)                       in (0, 1]
 *       (sn, cs) = rt_sincos_2pi(2 pi (double)r2)
 *       dx = (float)(cs (double)s),  dy = (float)(sn (double)s)                    -- the forms cosine_bounce uses; (dx, dy) is uniform on the unit disc by area
 *       lx = R dx,  ly = R dy
 *       O' = (O + lx ex) + ly ey               per component, the products first.  The fixed camera uses the same expression with the literal basis, so a -0 coordinate
 *                                              of O may become +0 (-0 + (+0) = +0).
 *       u' = normalize(F - O')
 *     The path starts with the ray (O', u'): the sphere decision at emission, the traversal, shading and ray counts are the pinhole code on that ray; a camera ray still
 *     counts as one ray.  One kernel knows the rule: wf_advance<kFormFirst | kFormLens>, the opening launch of every chain while the lens is on; the later launches are whichever kernels the
 *     scene picks without a lens (several lights, soft lights, textures, smooth normals).
 *     The lens is host state; a frame in flight keeps what its launches captured.  rt_scene_upload* leaves a pinhole (R = 0, f = 1): the camera comes with the upload.
 *     RT_ERR_INVALID, the lens untouched: a NULL pointer, a radius whose sign bit is set or that is not finite, and with R > 0 a focus distance that is not finite or not
 *     above 0 (with R == 0 the focus distance is stored as given and never read).
 *     Lens on is rendered by every entry that runs wf_advance -- rt_render*, _device, _device_batch (each frame's own camera), _async, _pose*, rt_progressive_frame -- under
 *     the variants auto, wavefront, wavefront_lds, wavefront_queue and lds_* (auto never resolves to lockstep), with several samples, row shares, RT_PARTS cuts and
 *     pipelining.  RT_ERR_UNSUPPORTED, outputs untouched: rt_render_device_batch_scenes with scenes, rt_render_counts*, rt_count_work and the variants path, lockstep and
 *     global.  rt_multi_* contexts have no such entries.
 *     STILL VIEWS.  With a lens a pixel's camera ray depends on the sample whatever sigma is: while the lens is on no chain fills or uses the first-hit, first-shadow or
 *     first-shade cache and none of their counters moves.  Turning the lens on or off empties all three: the first pinhole frame afterwards is a cold frame.
 *     FEATURE BUFFERS.  rt_render_aov*, _motion and _surface keep the pixel-centre pinhole ray and the reprojection keeps the pinhole camera: the guides of a defocused frame
 *     are sharp. */
int rt_camera_set_lens(rt_ctx *ctx, float aperture_radius, float focus_distance);
int rt_camera_get_lens(const rt_ctx *ctx, float *aperture_radius, float *focus_distance);

/* --- SHUTTER: motion blur -- the spheres and the light move within one frame's exposure (ABI 6, additive).  The context carries a shutter motion: a displacement dL of the
 *     light over the exposure and a displacement dC[slot] for every object slot of Scene::objects.  No counterpart in the reference: its frames are instants
 *     (MoveLightSource / MoveObject act between two frames).
 *     "Shutter on": some component of some displacement is not +-0.  With the shutter off every call and every frame is what it is without these entries, launch for launch.
 *     THE RULE.  Sample samp of pixel (px, row) has the key hs = sample_hash(pixel_hash(fr, row, px, seed), samp).  Its time is
 *       tau = uniform01(hs, 1u << 28, 2)       in (0, 1].  (The RNG keys on depth * 4 + dim modulo 2^32: the draw sits at 2^30 + 2.  The lens uses 2^30 + 0 and 2^30 + 1;
 *                                              jitter, bounce and pick draws sit below 4 (segs + 1), the shell draws of soft shadows at 2^31 + ...: nothing collides.)
 *     Every launch of the path draws tau again from hs: no path state grows.  In binary32, one rounding per operation, the product first, no fused multiply-add:
 *       C' = C + dC tau                        per component, for every sphere -- MoveObject's arithmetic (realtime:1096): rt_scene_move_sphere(v = dC, dt = 1) gives the
 *                                              tau = 1 pose exactly
 *       L' = L + dL tau                        the light, in the same form (linear, not the orbit of rt_scene_move_light)
 *     R * R and the materials do not move.  For that path every sphere test, sphere normal, shadow direction, the comparison that decides whether the light is hidden, and
 *     the direct term use C' and L', in every segment: one path sees one instant, so nested glass stays consistent.  Meshes do not move within an exposure: their slots'
 *     displacements must be +-0.  The camera does not move.  The step is shutter_time / shutter_pose in rt_shade.hip.h; four forms of wf_advance know it
 *     (kFormShutter: the two opening launches, with and without the lens, and the later launches with and without textures).
 *     The motion is host state: make_frame captures it as it captures the lens, and a frame in flight keeps what its launches captured.  rt_scene_upload* leaves the
 *     shutter closed; rt_scene_set_sphere, rt_scene_move_sphere, rt_scene_set_light and rt_scene_move_light keep it.  rt_scene_set_shutter(ctx, NULL) closes it.
 *     RT_ERR_INVALID, the state untouched: a component that is not finite, a displacement that is not +-0 for a mesh's slot or for a slot beyond the scene's objects, a
 *     NULL out.  RT_ERR_NO_SCENE: no upload, or the last rt_scene_upload* failed.  A refused get writes nothing.
 *     Shutter on is rendered by every entry that runs wf_advance -- rt_render*, _device, _device_batch, _async, _pose*, rt_progressive_frame -- under the variants auto
 *     (never lockstep), wavefront, wavefront_lds, wavefront_queue and lds_*, with several samples, row shares, RT_PARTS cuts and pipelining, with or without the lens.
 *     RT_ERR_UNSUPPORTED, outputs untouched, "shutter" in the error text: rt_render_device_batch_scenes with scenes, rt_render_counts*, rt_count_work, the variants
 *     path, lockstep and global, and every render while the scene holds several lights or a light with a radius above 0.
 *     STILL VIEWS.  A path's spheres and light depend on the sample: while the shutter is on no chain fills or uses the first-hit, first-shadow or first-shade cache and
 *     none of their counters moves.  Turning the shutter on or off empties all three.
 *     FEATURE BUFFERS and rt_trace_rays see the start-of-exposure pose (C, L): the scene as it is stored. */
typedef struct { float light[3]; float object[RT_MAX_OBJECTS][3]; } rt_shutter;
int rt_scene_set_shutter(rt_ctx *ctx, const rt_shutter *shutter);
int rt_scene_get_shutter(const rt_ctx *ctx, rt_shutter *out);

/* --- ENVIRONMENT: a radiance map for the rays that miss the scene (ABI 6, additive).  No counterpart in the reference, whose room is closed: a miss is black there
 *     (cpu:571).  The context may hold an environment: a square map of n x n texels, 1 <= n <= RT_MAX_ENVIRONMENT, each three binary32 radiances (on the device a float4,
 *     16 B per texel).  The layout is octahedral with +y as the pole: the lookup needs no transcendental function and is bit for bit.  "Environment on": a map is set.  An
 *     all-zero map is still on; a 1 x 1 map is a constant sky.
 *     THE LOOKUP.  E = sky_radiance(u) for a ray direction u as the queue record holds it, not renormalised.  Binary32, one rounding per operation, no fused
 *     multiply-add; the quotients are the correctly rounded ones (rt_div.h).  |v| is v with its sign bit cleared.
 *       1. s = (|ux| + |uy|) + |uz|.  If s is not a finite number above 0 (NaN included): E = (+0, +0, +0).
 *       2. px = ux / s, pz = uz / s.
 *       3. If uy < 0:  qx = (1 - |pz|) * sg(px),  qz = (1 - |px|) * sg(pz),  sg(v) = v < 0 ? -1 : 1  (so sg(-0) = sg(+0) = 1; the products are formed).  Otherwise q = p
 *          (uy = -0 and uy = +0 included).
 *       4. a = qx * 0.5 + 0.5,  b = qz * 0.5 + 0.5: the product first.  The centre of the map is the zenith (+y), its corners are the nadir (-y), the left and right
 *          mid-edges are -x and +x, the top mid-edge (row 0) is -z, the way the fixed camera looks, the bottom mid-edge +z.
 *       5. sx = a * (float)n - 0.5,  sy = b * (float)n - 0.5: the product first.  Then the bilinear form of the textures on the float texels:
 *          x0 = floor(sx), fx = sx - x0 (tex_floor), likewise y0, fy;  xa = clamp(x0), xb = clamp(x0 + 1) to [0, n - 1] (tex_wrap, RT_TEX_CLAMP), likewise ya, yb;
 *          gx = 1 - fx, gy = 1 - fy;  per channel  E = (t[ya][xa] * gx + t[ya][xb] * fx) * gy + (t[yb][xa] * gx + t[yb][xb] * fx) * fy  -- tex_sample's expression.
 *          Clamping at the border instead of wrapping to the octahedral neighbour is part of the rule: along the border of the map, which is the lower hemisphere's
 *          fold lines from the horizon down to the nadir, the lookup is up to half a texel short of the interpolation a wrap would give.
 *     The step is sky_radiance in rt_shade.hip.h; the model is tests/sky_model.py.
 *     WHERE IT ENTERS.  When the close of a camera or continuation ray of segment d finds no object, the path's fold starts from ans = E instead of (0, 0, 0).
 *     Everything else is as without a map: the ray counts (.w), the order of the fold, the sampling.  A path of no segments traces no ray and stays black.  The bounce ray
 *     of the last segment is never built, so it meets no sky.  Shadow rays do not see the environment: it lights surfaces through the cosine bounces only.  The point
 *     light is still there; intensity 0 gives a scene lit by the sky alone.  Mirrors and glass show the environment: their continuation rays are ordinary rays.
 *     WHAT A TEXEL MAY BE.  Finite, sign bit clear, below 2^96: as an unsigned integer its bits are < 0x6f800000.  The bilinear sum stays finite and the dead-channel
 *     elision exact.
 *     rt_scene_set_environment(ctx, n, rgb): n * n * 3 floats, row 0 first; rgb == NULL or n == 0 removes the map.  rt_scene_get_environment(ctx, &n, rgb_or_NULL): n (0: no
 *     map) and, if rgb is not NULL, the n * n * 3 floats as stored.  The map is host state plus one device buffer of the context's.  A frame captures the buffer when it is
 *     enqueued and keeps it: replacing a map allocates a new buffer, and the old one is released after the frames that captured it.  rt_scene_upload* removes the
 *     environment: it belongs to the scene.  The sphere, light, lens and shutter edits keep it.
 *     RT_ERR_INVALID, the state untouched: n < 0 or n > RT_MAX_ENVIRONMENT, n > 0 with a NULL rgb, a texel that fails the bit test (NaN, +-inf, negative, -0, >= 2^96), a
 *     NULL n of the get.  RT_ERR_NO_SCENE: no upload, or the last rt_scene_upload* failed.  A refused get writes nothing.
 *     Environment on is rendered by every entry that runs wf_advance -- rt_render*, _device, _device_batch, _async, _pose*, rt_progressive_frame -- under the variants auto
 *     (never lockstep), wavefront, wavefront_lds, wavefront_queue and lds_*, with several samples, row shares, RT_PARTS cuts and pipelining, with or without the lens, with
 *     one light, a list of lights or lights with radii (a list without a radius renders through the soft forms with radii 0: the same light, bit for bit).
 *     RT_ERR_UNSUPPORTED, outputs untouched, "environment" in the error text: rt_render_device_batch_scenes with scenes, rt_render_counts*, rt_count_work, the variants
 *     path, lockstep and global, and every render while the shutter is on.
 *     STILL VIEWS.  While the environment is on no chain fills or uses the first-hit, first-shadow or first-shade cache and none of their counters moves.  Setting,
 *     replacing or removing a map empties all three.
 *     FEATURE BUFFERS, rt_trace_rays, the filters and the SVGF sequence do not change: a pixel that sees the sky still has no object. */
#define RT_MAX_ENVIRONMENT 1024
int rt_scene_set_environment(rt_ctx *ctx, int n, const float *rgb);
int rt_scene_get_environment(const rt_ctx *ctx, int *n, float *rgb);
/* known answers of the lookup: sky_radiance on n_dirs explicit directions (n_dirs x 3 in, n_dirs x 3 out) against the map the context holds; RT_ERR_INVALID without one */
int rt_kat_environment(rt_ctx *ctx, int n_dirs, const float *dirs, float *rgb_out);

/* --- SKY SAMPLING: directions drawn from the environment map by radiance (ABI 6, additive).  Under a map whose energy sits in a small bright region -- a sun -- a cosine
 *     bounce finds the light about as often as the region's share of the sphere.  The context therefore carries a share in [0, 1] (default 0: off) and, while the share is
 *     positive and a map is set, a SAMPLING TABLE built on the device from the map.  A diffuse segment still emits ONE shadow ray; the sky is one more thing it may go to.  The
 *     device steps are sky_draw and sky_weight in rt_shade.hip.h, beside sky_radiance; the model is tests/sky_sample_model.py.  With share 0, without a map, or under an
 *     all-zero map (empty table) every frame is launch for launch what it is without this call.
 *     Binary32 with one rounding per operation, no fused multiply-add, quotients correctly rounded (rt_div.h), unless stated otherwise.
 *     THE TABLE.  Texels t = y * n + x, row-major.
 *       1. Y(t) = fl(fl(R + G) + B).
 *       2. B9(t) = the sum of Y over the 3 x 3 neighbourhood, indices clamped to the map, dy = -1..1 outer, dx = -1..1 inner, added in that order.  The bilinear taps of
 *          every direction whose lookup lands in texel t's square lie inside it: B9(t) = 0 only where the lookup is 0 throughout, and the lookup never exceeds B9(t).
 *       3. The solid-angle factor at the texel's centre: ax = fl(fl(x + 0.5) / n), qx = fl(2 ax - 1), likewise qz from y.  The octahedral point p of (qx, qz), 1-norm 1:
 *          py = fl(fl(1 - |qx|) - |qz|) in both hemispheres; where py < 0 (below the horizon) px = fl(1 - |qz|) * sg(qx), pz = fl(1 - |qx|) * sg(qz), sg(v) = v < 0 ? -1 : 1,
 *          otherwise px = qx, pz = qz.  (The fold is decided by the sign of the rounded py, not by |qx| + |qz| > 1: one expression serves both.)
 *          m = fl(fl(fl(px px) + fl(py py)) + fl(pz pz)), W(t) = fl(B9(t) / fl(m * rt_sqrtf(m))).  A texel of the q-square, area 4 / n^2, subtends (4 / n^2) / |p|^3.
 *       4. Wmax = max W(t).  Wmax == 0: the table is EMPTY.  Otherwise c(t) = W(t) > 0 ? max(1, (uint32)(fl(W(t) / Wmax) * 2^31)) : 0.
 *       5. prefix[t] = the inclusive 64-bit sum of c; total = prefix[n n - 1] <= 2^51.  Integer sums: any parallel scan gives the same table.
 *     THE DRAW of segment d of the path whose sample key is hs: four draws at depth (3 << 28) + d, dims 0 to 3 (keys 3 2^30 + 4 d + dim; the lens and the shutter sit at
 *     2^30 + {0, 1, 2}, the shells at 2^31 + 4 d + {0, 1}).  ka, kb = the 24-bit integers behind draws 0 and 1 (uniform01 = (k + 1) 2^-24); K = ka 2^24 + kb;
 *     X = ((K * total) >> 48) + 1, the product 128 bits wide, X in [1, total]; t = the least texel with prefix[t] >= X (so c(t) > 0).  How the device searches is not part
 *     of the rule.
 *     THE DIRECTION.  jx, jz = draws 2 and 3; ax = fl(fl(x + jx) / n), qx = fl(2 ax - 1), likewise qz from the row and jz; p and m as in step 3; r = rt_sqrtf(m);
 *     w = p / r in normalize()'s form (three correctly rounded quotients).
 *     THE ESTIMATE.  With mx = max(dot(N, w), 0) and E = sky_radiance(w):  g = (float)((((double)mx * 4.0) * (double)total) / ((((double)c(t) * (double)(n n)) * (double)m) *
 *     (double)r)) -- binary64, rounded to binary32 once -- which is mx / pdf, pdf = c(t) / total * n^2 / 4 * |p|^3; the direct term is g * E per channel.  It is unbiased for
 *     the environment as sky_radiance looks it up.  A draw that rounds onto a neighbouring texel's edge (jx = 1) is evaluated with c(t) of the texel it was drawn from: a set
 *     of measure zero.
 *     THE SHARE.  The effective share s is 0 if the table is empty, 1 if the lights' total intensity is +-0, the share otherwise.  Segment d of sample key hs draws
 *     r_s = uniform01(hs, d + 1, 3) (key 4 (d + 1) + 3, which no jitter, bounce or pick draw reaches); its one shadow ray goes to the sky iff r_s <= s.  Then the direct term
 *     is l_rgb = w_sky * (g * E) per channel, w_sky = fl(1 / s).  Otherwise the ray goes to the light the list picks, unchanged, and its l is multiplied by w_light =
 *     fl(1 / (1 - s)); the term is (l, l, l).  Both weights are computed on the host.  At s = 1 the lights are never sampled.
 *     THE RAY to the sky starts at P_adjusted with direction w and has no far end: it is blocked iff any sphere or any accepted triangle is hit (with any-hit on its bound is
 *     +inf: the first accepted triangle ends it), and a blocked ray's term is +0 in the three channels.  It is not traced when the three words of l_rgb are +0.  The launch
 *     that closes it knows it went to the sky from r_s alone.  It counts in .w as any shadow ray: .w of a sampled frame is .w at share 0.
 *     THE MISS.  While s > 0 a continuation ray that left a DIFFUSE segment and leaves the scene starts the fold from +0 -- the shadow rays have accounted for the sky there;
 *     a camera ray and the continuation of a mirror or glass hit still start from E.  THE FOLD runs with the per-channel term: fl(fl(l_c alb_c) / pi) + fl(alb_c ans_c).
 *     DEAD CHANNELS: a segment whose ray goes to the sky clears the path's mask, as a segment that fails the guard does; a light's weighted term is guarded as before.
 *     Rendered by what renders the environment (the wavefront variants, any lights -- always through the soft lights' table --, the lens, poses, row shares, RT_PARTS,
 *     batches, rt_render_async, pipelining); refused by what refuses the environment, with "environment sampling" in the error text while the share is positive.
 *     rt_scene_set_environment_sampling(ctx, share): RT_ERR_INVALID, the state untouched, for a share outside [0, 1] or NaN; RT_ERR_NO_SCENE without an upload.  The table is
 *     built when the share becomes positive while a map is set and when a map is set or replaced while the share is positive; removing the map or a share of 0 drops it.  A
 *     replaced table is released after the frames in flight, as the map's own buffer is; a call that fails leaves share, map and table as they were.  rt_scene_upload* resets the share to 0; setting, replacing or removing a map and
 *     the sphere, light, lens and shutter edits keep it.  Every change empties the still view's caches.  rt_scene_get_environment_sampling(ctx, &share): the share as set.
 *     Known answers: rt_kat_environment_table reads the table back -- c and prefix, n * n each, either may be NULL, and the total; an empty table is total 0 and zeros;
 *     RT_ERR_INVALID without a map or with share 0.  rt_kat_environment_sample runs the draw on `count` explicit (hs, seg) pairs: the texel, the direction (count x 3) and g
 *     at mx = 1; RT_ERR_INVALID without a table to draw from. */
int rt_scene_set_environment_sampling(rt_ctx *ctx, float share);
int rt_scene_get_environment_sampling(const rt_ctx *ctx, float *share);
int rt_kat_environment_table(rt_ctx *ctx, uint32_t *c_out, uint64_t *prefix_out, uint64_t *total);
int rt_kat_environment_sample(rt_ctx *ctx, int count, const uint32_t *hs, const int32_t *seg, uint32_t *texel_out, float *dir_out, float *g_out);

/* --- EMISSIVE MESHES: area lights seen by paths and sampled by shadow rays (ABI 6, additive).  A mesh object may carry a radiance Le = (r, g, b), every component in
 *     [+0, 2^96) as the environment's texels; Le all +0: the mesh does not emit.  Spheres cannot emit.  An emitter is two-sided and is geometry like any other mesh: it
 *     occludes every ray.  It absorbs: its albedo, mirror flag, refraction indices, smooth normals and texture are not read by the render chain.  With no emitter set every
 *     frame is launch for launch what it is without these entries, and no new kernel runs.  The device steps are emit_draw and emit_weight in rt_shade.hip.h, beside
 *     sky_draw and sky_weight; the model is tests/emission_model.py.
 *     Binary32 with one rounding per operation, no fused multiply-add, quotients correctly rounded (rt_div.h), unless stated otherwise.
 *     THE HIT.  A continuation ray of segment d whose nearest object -- mesh and sphere winners decided as ever -- is an emitter ends its path there: no shadow ray and no
 *     continuation ray are emitted, SID[d] = 0xff, and the fold starts from E: E = Le if d == 0, or SID[d - 1] == 0xff (a mirror or glass hit), or the effective share s
 *     is 0; otherwise E = +0 -- the segment's shadow rays have accounted for the emitters (the rule of sky sampling's miss).  The ray counts in .w as any continuation ray.
 *     THE TABLE runs over all triangles of the scene in stored (visit) order: the leaves of each mesh's tree as the traversal reaches them (the right child before the left,
 *     ascending inside a leaf; after a rebuild the order tri_order_out and the new tree give), the meshes one after the other in object order.
 *       1. A2(t) = rt_sqrtf(norm2(Nt)), Nt the record's raw cross(e1, e2): twice the area.
 *       2. Y(obj) = fl(fl(r + g) + b) of the mesh's radiance.
 *       3. W(t) = fl(A2(t) Y(obj of t)); +0 for the triangles of a mesh that does not emit.  Every W(t) must be finite: a W that overflows (a radiance near 2^96 on a
 *          triangle whose A2 is 2^32 or more) would make every quotient of step 4 zero or NaN and the table flat, so the build refuses it -- RT_ERR_INVALID, "emission"
 *          in the text, from the frame or known answer that asked for the table, until a radiance is lowered.
 *       4. and 5. are steps 4 and 5 of the sky table, word for word: Wmax = max W(t), Wmax == 0: the table is EMPTY; c(t) = W(t) > 0 ? max(1, (uint32)(fl(W(t) / Wmax)
 *          * 2^31)) : 0; prefix[t] = the inclusive 64-bit sum of c; total = the last prefix <= 2^51.
 *     THE DRAW of segment d of the path whose sample key is hs: four draws at depth (1 << 27) + d, dims 0 to 3 (keys 2^29 + 4 d + dim; the jitter, bounce, pick and share
 *     draws sit at 4 d' + dim with d' <= RT_MAX_SEGMENTS, the lens and the shutter at 2^30 + {0, 1, 2}, the shells at 2^31 + 4 d + {0, 1}, the sky's draws at 3 2^30 + 4 d +
 *     dim: none reaches these).  K, X and the triangle t as in the sky's draw (uniform24 of dims 0 and 1; the least t with prefix[t] >= X, so c(t) > 0).  r1, r2 =
 *     uniform01 of dims 2 and 3; if fl(r1 + r2) > 1 then r1 = fl(1 - r1), r2 = fl(1 - r2).  Q = fl(fl(A + fl(r1 e1)) + fl(r2 e2)) per component, from t's record.
 *     THE ESTIMATE at a diffuse hit P with normal N: v = Q - P, d2 = norm2(v), wl = normalize(v), mx = max(dot(N, wl), 0), cl = |dot(normalize(Nt), wl)|,
 *     g = (float)(((((double)mx (double)cl) (double)A2) (double)total) / ((2.0 (double)c(t)) (double)d2)) -- binary64, rounded to binary32 once -- which is mx cl / d2
 *     over the area density c / total * 2 / A2.  The direct term is l_c = w_emit * (g * Le_c) per channel, Le the radiance of t's mesh.
 *     THE RAY starts at Pa = P + eps N and aims at L' = Q + kappa (Pa - Q), kappa = 2^-10: per component fl(Q_k + fl(kappa fl(Pa_k - Q_k))).  From there on it is a point
 *     light's shadow ray to L': shadow_dir, the any-hit bound of (Pa, nl), the spheres, and it is blocked iff light_hidden(Pa, Pp, L').  Why kappa: the ray meets the
 *     emitter's own plane at nl / (1 - kappa), nl = |L' - Pa| -- a relative margin of 2^-10 in length, 2^-9 in the squared lengths light_hidden compares, over the 2^-20
 *     or so of rounding that comparison carries, whatever the scene's scale and eps are: the emitter never shadows its own sample.  The price is a known blind band: an
 *     occluder within 0.1 % of the distance in front of the emitter is not seen by that ray.  The ray is not traced when the three words of l are +0 and any-hit is on.  It
 *     counts in .w as any shadow ray.
 *     THE SHARE.  The context holds a share in [0, 1]; the default is 0.5 and rt_scene_upload* resets it to 0.5.  The effective s is 0 if the table is empty or the share
 *     is 0, 1 if the lights' total intensity is +-0, the share otherwise.  Segment d draws r_s = uniform01(hs, d + 1, 3); its one shadow ray goes to an emitter iff r_s <= s,
 *     with w_emit = fl(1 / s); otherwise to the light the list picks (a point of its shell), unchanged, and its l is multiplied by w_light = fl(1 / (1 - s)), the term
 *     (l, l, l).  Both weights are host divisions.  THE FOLD runs per channel, as under sky sampling.
 *     DEAD CHANNELS: a segment whose ray goes to an emitter clears the path's mask; a light's weighted term is guarded as before.  RT_DEAD_CHANNELS=0 renders the same words.
 *     Rendered by the wavefront variants' launch chain (two forms of wf_advance, kFormEmit; any lights, always through the soft lights' table; the lens, poses, row
 *     shares, RT_PARTS, batches, rt_render_async, pipelining), which keeps no still-view cache while a mesh emits.  RT_ERR_UNSUPPORTED, outputs untouched, "emission" in the
 *     error text: the variants path, lockstep and global, rt_count_work, rt_render_counts*, rt_render_device_batch_scenes with scenes, and any frame while the scene also
 *     has an environment or the shutter is on.  The feature-buffer and denoiser entries see an emitter as the ordinary object it is.  rt_multi_* contexts have no such entries.
 *     rt_scene_set_emission(ctx, object_slot, rgb): RT_ERR_INVALID, the state untouched, for a sphere's slot, a slot outside the scene, a NULL rgb, a component outside
 *     [+0, 2^96) or NaN (-0 included); RT_ERR_NO_SCENE without an upload.  rt_scene_get_emission: the radiance as set, zeros for a mesh that does not emit.
 *     rt_scene_set_emission_sampling(ctx, share): RT_ERR_INVALID for a share outside [0, 1] or NaN.  A refused get writes nothing.  rt_scene_upload* clears all emission.
 *     Neither call touches the still view: a chain under an emitter neither reads nor writes its caches, and a scene whose emission was set and removed again finds
 *     them as it left them -- its frames and its cache counters are those of a context that never heard of these calls.
 *     The table is rebuilt, into a buffer of its own that replaces the old one after a device-wide wait, before the next frame or known answer that follows a change of
 *     an emission or of the scene's triangles (rt_mesh_transform[_of], rt_mesh_rebuild[_of|_mode], rt_mesh_set_vertices*).
 *     Known answers: rt_kat_emission_table reads the table back -- c and prefix, n_triangles each (the scene's count, written to *n_triangles: either array may be NULL,
 *     a first call with both NULL asks for the count) and the total; no emitter or an empty table: total 0 and zeros.  rt_kat_emission_sample runs the draw on `count`
 *     explicit (hs, seg) pairs: the triangle and the point Q (count x 3); RT_ERR_INVALID without a table to draw from. */
int rt_scene_set_emission(rt_ctx *ctx, int object_slot, const float rgb[3]);
int rt_scene_get_emission(const rt_ctx *ctx, int object_slot, float rgb[3]);
int rt_scene_set_emission_sampling(rt_ctx *ctx, float share);
int rt_scene_get_emission_sampling(const rt_ctx *ctx, float *share);
int rt_kat_emission_table(rt_ctx *ctx, uint32_t *c_out, uint64_t *prefix_out, uint64_t *total, int32_t *n_triangles);
int rt_kat_emission_sample(rt_ctx *ctx, int count, const uint32_t *hs, const int32_t *seg, uint32_t *tri_out, float *point_out);

/* --- FRESNEL DIELECTRICS: glass reflects or refracts, chosen per sample (ABI 6, additive).  The reference's glass only ever refracts (cpu:580-604) and reflects only at
 *     total internal reflection.  An object whose flag is set reflects with probability R, the unpolarised Fresnel reflectance of its surface, and refracts otherwise;
 *     either ray carries weight R / R = (1 - R) / (1 - R) = 1, so no throughput is stored and no path state grows.  Off by default and per object; with no EFFECTIVE
 *     flag every frame is launch for launch what it is without these entries, and no new kernel runs.  The device step is fresnel_step in rt_shade.hip.h, beside
 *     refract_step; the model is tests/fresnel_model.py.
 *     Binary32 with one rounding per operation, no fused multiply-add, quotients correctly rounded, fl() one rounding.
 *     THE FLAG.  The context holds one bit per object position (up to RT_MAX_OBJECTS = 16).  rt_material_set_fresnel(ctx, object_slot, on) sets it (on != 0) or clears it,
 *     rt_material_get_fresnel reads it (1 or 0).  Any slot of the uploaded scene is accepted, sphere or mesh.  RT_ERR_NO_SCENE without an upload; RT_ERR_INVALID, the state
 *     and the output untouched, for a slot outside the scene or a NULL output.  rt_scene_upload* clears every bit.  A bit is EFFECTIVE only where a hit would take the
 *     reference's refraction branch: mirror == 0 and n_in != n_out, read from the materials as they are when a frame's chain is planned (rt_scene_set_sphere may change a
 *     material after the flag was set).  A flag on a mirror or on a diffuse object changes nothing.
 *     THE HIT.  The continuation ray (O, u) of segment d, whose index is refr, hits an effectively flagged object at P with normal N.
 *       1. out2in = (refr == n_out); ratio = out2in ? n_out / n_in : n_in / n_out, and N = -N if not out2in; un = dot(u, N); k = fl(fl(ratio ratio) fl(1 - fl(un un))).
 *          If ((out2in and refr > n_in) or (not out2in and refr > n_out)) and k > 1 the ray is TOTALLY REFLECTED: O = P + eps N, u = u - fl(2 un) N, the index stays.  All
 *          of this is refract_step's, word for word.
 *       2. Otherwise n1 = out2in ? n_out : n_in, n2 = out2in ? n_in : n_out, ci = |un|, ct = rt_sqrtf(fl(1 - k)) -- the value the refracted direction uses --
 *          a = fl(n1 ci), b = fl(n2 ct), c = fl(n1 ct), e = fl(n2 ci), rs = fl(fl(a - b) / fl(a + b)), rp = fl(fl(c - e) / fl(c + e)),
 *          R = fl(0.5 fl(fl(rs rs) + fl(rp rp))): the Fresnel equations themselves, not Schlick's approximation; two quotients, no pow.
 *       3. r_f = uniform01(hs, (1u << 26) + d, 0), hs the sample's key: the RNG keys on depth * 4 + dim, so this draw sits at 2^28 + 4 d -- above the jitter, bounce, pick
 *          and share draws (4 d' + dim, d' <= RT_MAX_SEGMENTS + 1: below 2^7) and below the emitters' draws (2^29 + 4 d + dim); the lens and the shutter sit at
 *          2^30 + {0, 1, 2}, the shells at 2^31 + 4 d + {0, 1}, the sky's draws at 3 2^30 + 4 d + dim.  With d <= RT_MAX_SEGMENTS the key stays below 2^28 + 2^7: none of
 *          the others reaches it.
 *       4. REFLECT iff r_f <= R: the reflected ray is the total-reflection branch's own, O = P + eps N, u = u - fl(2 un) N; the ray's index and its refr code stay.
 *          Otherwise the refracted ray is exactly the reference's: O = P - eps N, u = fl(-ct) N + ratio (u - un N), the index becomes out2in ? n_in : n_out.  A NaN R
 *          refracts (the comparison is false): a negative radicand in nested glass with unmatched indices (the reference's quirk: k > 1 where the index test fails), or
 *          0 / 0 at ci = ct = 0 -- the reference's ray, so an unflagged frame and a flagged one agree on such a hit.
 *     Nothing else of the path changes: a specular segment emits no shadow ray, SID[d] = 0xff, .w counts one continuation ray, and shadow rays still stop at glass.
 *     R is in [0, 1] outside total reflection, exactly 1 at ci = 0 from the thin side, and 0.040000003 (0x3D23D70B) at normal incidence for 1 <-> 1.5.
 *     Rendered by the wavefront variants' launch chain (four forms of wf_advance, kFormFresnel: with and without textures, with and without the soft lights' table, which
 *     any light list or radius takes; the lens, poses, row shares, RT_PARTS, plain batches, rt_render_async, pipelining), which keeps no still-view cache under an effective
 *     flag; setting and removing a flag leaves the caches as they were -- frames and cache counters are those of a context that never heard of these calls.
 *     RT_ERR_UNSUPPORTED, outputs untouched, "fresnel" in the error text, under an effective flag: the variants path, lockstep and global, rt_count_work,
 *     rt_render_counts*, rt_render_device_batch_scenes with scenes, and any frame while the scene also has an environment, the shutter is on or a mesh emits.
 *     The feature-buffer entries (rt_render_aov*, rt_render_aov_surface*) keep following the refracted branch: no virtual image of a reflection.  rt_multi_* contexts have
 *     no such entries.
 *     Known answer: rt_kat_fresnel runs the device step on `count` explicit items; it needs no scene.  items: 16 32-bit words per item -- binary32 n_in, n_out, the ray's
 *     index, eps, P (3), N (3), u (3), then the integers hs and seg, then one unused word.  out: 9 words per item -- binary32 R (+0 for a totally reflected ray), the
 *     integer code (0 refracted, 1 reflected, 2 totally reflected), the new O (3) and u (3), the index after. */
int rt_material_set_fresnel(rt_ctx *ctx, int object_slot, int on);
int rt_material_get_fresnel(const rt_ctx *ctx, int object_slot, int *on);
int rt_kat_fresnel(rt_ctx *ctx, int count, const uint32_t *items, uint32_t *out);

/* --- ROUGH MIRRORS: a GGX roughness per object, one facet drawn per hit (ABI 6, additive).  The reference's mirror is perfect (cpu:573-579).  An object with a roughness
 *     alpha reflects each ray about a facet normal h drawn per hit instead of about the shading normal N; the reflected ray carries weight 1, so no throughput is stored
 *     and no path state grows.  Off by default and per object; with no EFFECTIVE roughness every frame is launch for launch what it is without these entries, and no new
 *     kernel runs.  The device step is gloss_step in rt_shade.hip.h, beside mirror_step; the model is tests/gloss_model.py.
 *     THE LOBE, honestly: facet normals GGX-distributed with width alpha about the shading normal (h is drawn with density D(h) (n.h)), reflectance 1, NO
 *     shadowing-masking term; a ray that a facet would send below the surface is folded back above it (mirrored about N).  This conserves energy -- every ray leaves
 *     with weight 1 -- and is not reciprocal.
 *     Binary32 with one rounding per operation, no fused multiply-add, quotients correctly rounded, fl() one rounding; the square roots are rt_sqrtf; sine and cosine are
 *     rt_sincos_2pi on the binary64 product, in cosine_bounce's forms.
 *     THE VALUE.  The context holds one binary32 alpha per object position (up to RT_MAX_OBJECTS = 16).  rt_material_set_roughness(ctx, object_slot, alpha) sets it,
 *     rt_material_get_roughness reads it as set.  Accepted: 0 (smooth, the default; -0 is stored as +0) and [2^-12, 1].  Any slot of the uploaded scene is accepted, sphere
 *     or mesh.  RT_ERR_NO_SCENE without an upload; RT_ERR_INVALID, the state and the output untouched, for a slot outside the scene, a NULL output or any other value, NaN
 *     included.  rt_scene_upload* clears every value.  A value is EFFECTIVE only where alpha > 0 and the object's material takes the mirror branch (mirror != 0), read
 *     from the materials as they are when a frame's chain is planned (rt_scene_set_sphere may change a material after the value was set).  A roughness on a diffuse or a
 *     glass object changes nothing.
 *     THE HIT.  The continuation ray (O, u) of segment d hits an object with an effective roughness at P with normal N, where the mirror's arm runs otherwise.
 *       1. N is the hit's normal exactly as mirror_step receives it, NOT oriented towards the ray.  un = dot(u, N).  O = fl(P + eps N): mirror_step's, word for word.
 *       2. r1 = uniform01(hs, 2^25 + d, 0), r2 = uniform01(hs, 2^25 + d, 1), hs the sample's key: the RNG keys on depth * 4 + dim, so the draws sit at 2^27 + 4 d + dim --
 *          above the jitter, bounce, pick and share draws (4 d' + dim, d' <= RT_MAX_SEGMENTS + 1: below 2^7) and below Fresnel's 2^28 + 4 d, the emitters' 2^29 + 4 d + dim, the lens and the
 *          shutter at 2^30 + {0, 1, 2}, the shells' 2^31 + 4 d + {0, 1} and the sky's 3 2^30 + 4 d + dim.  With d <= RT_MAX_SEGMENTS the key stays below
 *          2^27 + 2^7: none of the others reaches it.
 *       3. The facet's polar angle, which samples D(h) (n.h):  a2 = fl(alpha alpha), m = fl(a2 - 1), c2 = fl(fl(1 - r1) / fl(1 + fl(m r1))), c = rt_sqrtf(c2),
 *          s = rt_sqrtf(fl(1 - c2)).  THE RANGE, for alpha in [2^-12, 1] and r1 a multiple of 2^-24 in (0, 1]: 1 - r1 is exact (a multiple of 2^-24 in [0, 1)).  m is in
 *          [-1, 0] (a2 is in [2^-24, 1], and a2 - 1 rounds to no less than -1), so the exact 1 + m r1 is >= 1 - r1 >= 0, and rounding is monotone and 1 - r1 is
 *          representable: fl(m r1) >= -r1 and the denominator is >= 1 - r1.  It is positive: at r1 < 1 it is >= 1 - r1 >= 2^-24; at r1 = 1 it is fl(1 + m) = fl(a2),
 *          at least 2^-24 (exactly 2^-24 at alpha = 2^-12; m = fl(2^-24 - 1) = -(1 - 2^-24) is exact).  So the quotient is in [0, 1], c2 is in [0, 1], 1 - c2 is in
 *          [0, 1], and neither root sees a negative operand.
 *       4. The azimuth and the facet: (sn, cs) = rt_sincos_2pi(2 pi (double) r2); x = (float)(cs (double) s), y = (float)(sn (double) s); T1, T2 are cosine_bounce's
 *          tangent frame about N, the same expressions (T1 = normalize((-Ny, Nx, 0)) if Nx != 0 and Ny != 0, else normalize((-Nz, 0, Nx)); T2 = cross(N, T1));
 *          h = (x T1 + y T2) + c N.  (A normal of exactly (0, +-1, 0) has no tangent frame -- the second vector is zero, its quotient 0 / 0 -- for a facet as for a
 *          diffuse bounce: h and the ray are NaN there.)
 *       5. Reflect about the facet: uh = dot(u, h); u' = u - fl(2 uh) h.
 *       6. Keep the ray above the surface: vn = dot(u', N); if vn != 0 and (vn < 0) == (un < 0), the facet sent the ray into the surface, and it is mirrored back
 *          out: u' = u' - fl(2 vn) N (FOLDED BACK).
 *       7. The ray is not renormalised (the mirror's is not either); its index and its refr code stay, as at a mirror.  No shadow ray is emitted, SID[d] = 0xff, .w
 *          counts one continuation ray, and shadow rays still stop at the object.
 *     Rendered by the wavefront variants' launch chain (four forms of wf_advance, kFormGloss: with and without textures, with and without the soft lights' table, which
 *     any light list or radius takes; the lens, poses, row shares, RT_PARTS, plain batches, rt_render_async, pipelining), which keeps no still-view cache under an effective
 *     roughness; setting and removing a value leaves the caches as they were -- frames and cache counters are those of a context that never heard of these calls.  Under
 *     RT_VARIANT_AUTO a scene of spheres alone takes the wavefront chain while a roughness is effective.
 *     RT_ERR_UNSUPPORTED, outputs untouched, "roughness" in the error text, under an effective roughness: the variants path, lockstep and global, rt_count_work,
 *     rt_render_counts*, rt_render_device_batch_scenes with scenes, and any frame while the scene also has an environment, the shutter is on, a mesh emits or a Fresnel
 *     flag is effective.  The feature-buffer entries (rt_render_aov*, rt_render_aov_surface*) keep following the smooth mirror ray.  rt_multi_* contexts have no such
 *     entries.
 *     Known answer: rt_kat_gloss runs the device step on `count` explicit items; it needs no scene.  items: 16 32-bit words per item -- binary32 alpha, eps, P (3), N (3),
 *     u (3) at words 0 to 10, then the integers hs (word 11) and seg (word 12), then three unused words.  out: 12 words per item -- binary32 h (3) at words 0 to 2, the
 *     integer code at word 3 (0 plain, 1 folded back), the new O (3) at words 4 to 6 and u (3) at words 7 to 9, then two unused words, written as 0. */
int rt_material_set_roughness(rt_ctx *ctx, int object_slot, float alpha);
int rt_material_get_roughness(const rt_ctx *ctx, int object_slot, float *alpha);
int rt_kat_gloss(rt_ctx *ctx, int count, const uint32_t *items, uint32_t *out);

/* --- TINT: a specular colour per object, carried by the fold (ABI 6, additive).  The reference ignores the albedo of a mirror and of glass (cpu:573-607): every
 *     mirror is silver and every glass ball clear.  A flagged mirror or glass object multiplies what is seen in it or through it by its own albedo, per channel.  The
 *     path stores no new state for that: the throughput of a path IS its fold, fold_segment(ans, l, alb) = fl(fl(fl(l alb) / pi) + fl(alb ans)) per channel back to
 *     front over the segments that are not marked 0xff, and a tinted specular segment is recorded as a segment of direct term +0.  Off by default and per object; with
 *     no EFFECTIVE flag every frame is launch for launch what it is without these entries, and no new kernel runs.  The model is tests/tint_model.py.
 *     THE FLAG.  The context holds one bit per object position (up to RT_MAX_OBJECTS = 16).  rt_material_set_tint(ctx, object_slot, on) sets it (on != 0) or clears it,
 *     rt_material_get_tint reads it (1 or 0).  Any slot of the uploaded scene is accepted, sphere or mesh.  RT_ERR_NO_SCENE without an upload; RT_ERR_INVALID, the state
 *     and the output untouched, for a slot outside the scene or a NULL output.  rt_scene_upload* clears every flag.
 *     EFFECTIVE.  A flag is effective only where it is set and the object's material takes a specular arm: mirror != 0 (smooth, or rough by rt_material_set_roughness), or
 *     n_in != n_out -- read from the materials as they are when a frame's chain is planned (rt_scene_set_sphere may change a material after the flag was set: a flag on
 *     a diffuse sphere does nothing and starts to act when the sphere is made a mirror).
 *     THE COLOUR is the object's albedo as the material table holds it: from the upload, from rt_scene_set_sphere, a mesh's uploaded albedo.  A texture is not sampled at
 *     a specular hit: a textured mirror mesh is tinted by its material albedo.  The colour is meant to lie in [+0, 1] per channel; the fold is applied to whatever the
 *     table holds (a component of -0 or below gives the direct term's fl(fl(0 alb) / pi) the sign bit: -0 + x is x unless x is -0).
 *     THE HIT.  The continuation ray of segment d hits an effectively tinted object.  It takes exactly the arm it takes without the flag (mirror_step, gloss_step,
 *     refract_step) and builds the same ray; it emits no shadow ray; .w counts what it counted.  It records SID[d] = the object's id and LS[d] = +0 where an unflagged
 *     specular hit records SID[d] = 0xff.  The fold then forms, for that segment, fl(fl(fl((+0) alb) / pi) + fl(alb ans)) = fl(alb ans) per channel for alb >= +0:
 *     what follows the hit, times the tint, one rounding.  A path whose first hit is a tinted mirror of tint t over a remainder X is fl(t X) per channel.
 *     GLASS.  Every crossing of an interface is a hit, so glass is tinted PER INTERFACE: a ball seen through is tinted twice, once in and once out, fl(t fl(t X)); a
 *     ray that is totally reflected inside is tinted once more per reflection.  This is a SURFACE tint, NOT Beer's law: the colour does not depend on the distance
 *     travelled inside the object, and a thick and a thin part of a mesh are tinted alike.
 *     DEAD CHANNELS.  The tinted segment goes through the dead-channel rule exactly as a diffuse segment of albedo alb and direct term +0 does
 *     (wf_dead_channels(dead, alb, +0)): a zero channel of the tint kills that channel for the shadow rays of the segments behind it, a component above 1 resets the
 *     mask.  To the fold the segment IS such a diffuse segment, so the argument for the elided shadow rays holds word for word, and frames under RT_DEAD_CHANNELS=0
 *     are the default's words.  RT_DEAD_LAST applies only where every object is diffuse (csrc/rt_deadlast.h, condition (1)) and only in the plain chain: never here.
 *     THE CLOSE OF A SHADOW RAY.  The launch after segment d decides whether a shadow ray of segment d is in flight from the path's flag word (PF_HASX, set where the
 *     ray was emitted) and never from SID: a tinted segment, which emits none, is not taken for one that did, and its LS[d] stays +0.
 *     Rendered by the wavefront variants' launch chain (four forms of wf_advance, kFormTint, each with the rough mirrors' arm compiled in -- a scene without an
 *     effective roughness runs them with an empty roughness mask and takes the smooth mirror arm: with and without textures, with and without the soft lights' table,
 *     which any light list or radius takes; the lens, poses, row shares, RT_PARTS, plain batches, rt_render_async, pipelining), which keeps no still-view cache under an
 *     effective tint; setting and removing a flag leaves the caches as they were -- frames and cache counters are those of a context that never heard of these calls.
 *     Under RT_VARIANT_AUTO a scene of spheres alone takes the wavefront chain while a tint is effective.
 *     RT_ERR_UNSUPPORTED, outputs untouched, "tint" in the error text, under an effective tint: the variants path, lockstep and global, rt_count_work,
 *     rt_render_counts*, rt_render_device_batch_scenes with scenes, and any frame while the scene also has an environment, the shutter is on, a mesh emits or a Fresnel
 *     flag is effective.  The feature-buffer entries (rt_render_aov*, rt_render_aov_surface*) are unchanged: their albedo plane is not demodulated by a tint.
 *     rt_multi_* contexts have no such entries.  There is no known-answer entry: no new device step exists for one to call. */
int rt_material_set_tint(rt_ctx *ctx, int object_slot, int on);
int rt_material_get_tint(const rt_ctx *ctx, int object_slot, int *on);

/* --- ... and per FRAME of a batch: a sequence in which the light orbits and spheres move, at the throughput of rt_render_device_batch.  Frame k's buffer holds
 *     exactly what rt_render_device writes after the scene is uploaded with frames[k].camera, scenes[k].light and the uploaded spheres moved to
 *     scenes[k].spheres[0 .. n_spheres) (in the order of the uploaded spheres array; materials, object positions and meshes as uploaded), p->seed =
 *     frames[k].seed -- ray counts (.w) included.  n_spheres must equal the uploaded count (RT_ERR_INVALID); every other rule of rt_render_device_batch holds
 *     (num_rays 1, wavefront variants, RT_MAX_BATCH, distinct buffers; textured and smooth-shaded scenes render).  scenes == NULL is rt_render_device_batch.  The
 *     uploaded scene is not changed (rt_scene_get_light answers as before).  Frames of a plain batch and lone frames run the kernels they ran: only an
 *     animated batch reads the per-frame table.  Not per frame: sphere materials, the sphere count, meshes (rt_scene_set_sphere / rt_mesh_transform between
 *     batches).  Replaces n x (MoveLightSource, MoveObject, KernelLaunch + sync; realtime_render.cu disp()). */
typedef struct rt_sphere_pose { float center[3]; float radius; } rt_sphere_pose;
typedef struct rt_frame_scene {    /* what differs from the uploaded scene in ONE frame of a batch */
    rt_light       light;
    rt_sphere_pose spheres[RT_MAX_SPHERES];
} rt_frame_scene;
int rt_render_device_batch_scenes(rt_ctx *ctx, const rt_params *p, const rt_rows *rows, const rt_frame_desc *frames,
                                  const rt_frame_scene *scenes, int n_spheres, int n_frames, void *stream);

/* --- tonemap: cpu:714-716 (gamma 1/2.2 in binary64, min 255, truncate) -------
 *     byte = (unsigned char)min(pow((double)c, 1./2.2), 255.) of .x, .y, .z; .w is not read.  Special values, as the oracle records them: NaN -> 0; a finite
 *     negative c (-1e-45 included) -> pow is NaN -> 0; +-0 -> 0; +inf -> 255; -inf -> 255 (pow(-inf, y) is +inf for this y).  Denormals are ordinary inputs: 0.
 *     rgb8_dev may be any address: an image that starts on a 4-byte boundary is written as 32-bit words, any other byte by byte; either way exactly
 *     3 * n_pixels bytes are written.  n_pixels == 0 writes nothing.  tests/test_gpu_gamma_bytes.py holds the bytes to the exactly rounded power at every code
 *     boundary (tests/gamma_model.py). */
int rt_tonemap_device(rt_ctx *ctx, const void *rgba_dev, int64_t n_pixels, void *rgb8_dev, void *stream);
/* render + tonemap + D2H of the interleaved RGB8 image (what stbi_write_png gets, cpu:719) */
int rt_render_rgb8(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, uint8_t *out_rgb8_host);

/* --- work accounting: renders rows [row_begin,row_end) with the counting instantiation of
 *     the kernel and returns the traversal work; 1 ray = 1 Scene::intersect_all call (cpu:545).  The
 *     algorithmic bytes of the roofline are 24 B*box_tests + 16 B*nodes + 48 B*tri_tests + 16 B*pixels. */
typedef struct rt_work {
    uint64_t rays;                 /* intersect_all calls (primary + shadow + bounce)         */
    uint64_t box_tests;            /* BoundingBox::intersect calls, root included             */
    uint64_t nodes;                /* BVH nodes whose box was hit (= nodes the reference pops) */
    uint64_t tri_tests;            /* moller_trumbore calls                                   */
    uint64_t box_literal;          /* of box_tests: decided by the literal divisions of cpu:147-152 (the error-bounded filter deferred) */
    uint64_t tri_literal;          /* of tri_tests: barycentrics by the literal divisions of cpu:232-233                                */
    uint64_t steps[12];            /* work-stack traversal kernel, summed over its waves and launches: loop iterations, refill passes,
                                    * refill rounds, queue fetches, TRI steps (128 triangle tests), BOX steps (64 sibling pairs),
                                    * literal-box fall-backs, serial drains; then blocks a step enters only when some lane needs them:
                                    * t-division blocks of the triangle tests (2 per TRI step at most), first and second leaf-queue
                                    * push of a BOX step; TRI steps in which a shadow ray stopped at a hit that certainly shades (any-hit; 0 for the
                                    * binary instantiation, which never stops early).  bench.py prices the vector-issue roofline with them. */
} rt_work;
/* The counters describe the REFERENCE-EQUIVALENT traversal (the binary instantiation of the kernel: every box the reference tests, cpu:284-293), whatever
 * kernel produces the frames: with the 16-bit fixed-point pairs (RT_TRAVQ_Q16) or the 4-wide BOX step
 * (RT_TRAVQ_QW) the production kernel enters a superset of the internal nodes and skips levels, stops a shadow ray at the first accepted triangle that certainly
 * shades and does not trace a shadow ray that a sphere shades already (any-hit, RT_TRAVQ_ANYHIT=0 turns both off: cpu:615 is monotone in the nearest hit's t, so the
 * frame is the same bit for bit), and its own visits are not what box_tests / nodes / tri_tests
 * report -- unless RT_TRAVQ_QW_COUNT=1 asks for the 4-wide kernel's own counting instantiation (experiments).
 * With several meshes (rt_scene_upload_meshes) the tree in use holds synthetic union nodes above the meshes' roots: box_tests / nodes count those too (one test of the
 * forest's root where the reference tests every mesh's root, cpu:279), tri_tests are the reference's. */
int rt_count_work(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, rt_work *out);
/* Of the last rt_count_work of the default pipeline: continuation rays and shadow rays handed to the mesh traversal (they passed the root box), shadow rays not
 * traced because every colour channel of their path was dead (a diffuse surface with a zero albedo component in each channel earlier on the path: neither answer can
 * change the pixel; RT_DEAD_CHANNELS=0 traces them; only surfaces with albedo components in [0, 1] and a direct term below 2^96 count), and paths with
 * such a ray whose fold met a negative or non-finite operand or a colour of 2^126 and more (a statistic: their pixels are the reference's all the same; 0 in any scene
 * with finite non-negative albedos and colours below 2^126).  The rule needs any-hit: the last two are 0 unless RT_TRAVQ_QW_COUNT=1. */
int rt_dead_channel_counts(rt_ctx *ctx, uint64_t out[4]);
/* Beside them, of the same rt_count_work: continuation rays (they passed the root box, and are among the first counter above) that the dead-last rule leaves out of
 * the traversal in a frame of the same scene and knobs (the counting run itself traces them all).  The rule: in a chain of three segments or more, the LAST continuation ray of a path whose three colour channels are dead after the segment that
 * emits it, and which the sphere tests show to hit a sphere for certain, is closed as that sphere's hit -- the pixel is +0 in every channel and the ray count the same
 * whatever the mesh would have said.  Only where the scene allows it, decided at every call from the scene as it is then: every object diffuse with albedo components
 * in [0, 1], no mesh shading with vertex normals, a finite light that stays clear of every sphere's surface and of the mesh's root box (csrc/rt_deadlast.h); only the plain chain (no
 * texture, light list, lens, shutter, environment, emitter, fresnel flag, batch scenes or list).  RT_DEAD_LAST=0 traces the rays; frames are the same bit for bit.
 * Needs any-hit and the dead-channel rule: 0 unless RT_TRAVQ_QW_COUNT=1. */
int rt_dead_last_count(rt_ctx *ctx, uint64_t *out);
/* The first-hit cache of the default pipeline: with sigma == 0 the camera ray of a pixel does not depend on the sample, so the mesh hits of a still
 * camera's primary rays are traced once per context and kept until the camera, the frame geometry, the row share, tri_tmin, the traversal form, the stream or the mesh
 * changes (RT_FIRST_HIT_CACHE=0 traces them in every chain; frames are the same bit for bit).  Since the context was created: launch chains that did not enqueue
 * their first traversal launch, chains whose first launch filled the cache, chains that were not eligible (jittered camera, batch, counting run, rt_stats_enable,
 * another pipeline, no mesh, knob off), and key comparisons that emptied a filled cache. */
int rt_first_hit_cache_counts(const rt_ctx *ctx, uint64_t out[4]);
/* The first-shadow cache beside it: under the same conditions the shadow ray of a pixel's FIRST segment depends on the camera ray, on what it hits
 * and how that is shaded, on the light and on eps -- not on the sample or the seed -- so its traversal result is kept per pixel slot as well (8 bytes per pixel slot more:
 * 16.6 MB per context at 1920x1080, allocated by the first eligible frame) and later chains hand no such ray to the traversal: every sample after the first of a frame,
 * every frame of a still view under a still light.  Kept until the first-hit cache is emptied or the light, eps, a sphere, the object order, a material, the smooth normals,
 * a texture or an elision knob (RT_TRAVQ_ANYHIT, RT_DEAD_CHANNELS) changes; a frame that misses traces and stores again.  RT_FIRST_SHADOW_CACHE=0 traces the rays in every
 * chain, and so does RT_FIRST_HIT_CACHE=0 (the chain of a moving camera, launch for launch); frames are the same bit for bit.  Since the context was created: chains that
 * read the cache, chains that filled it, chains that were not eligible (whatever makes the first-hit cache ineligible, or the knob), and key comparisons that emptied a
 * filled cache.  rt_first_hit_cache_counts keeps its meaning: a light or sphere edit moves these counters, not those. */
int rt_first_shadow_cache_counts(const rt_ctx *ctx, uint64_t out[4]);
/* The first-shade cache on top of it: once the first-shadow cache's key has held for two chains, the state of a pixel slot's path after its first
 * hit is shaded and its shadow ray decided -- everything before the bounce direction, the first thing that reads the seed -- is kept as well (32 bytes per pixel slot more:
 * 66 MB per context at 1920x1080, allocated by the first chain that fills it), and later chains open with one launch that resumes every path there, in place of the
 * launch that sets up the camera rays and the one that closes segment 0.  It lives under the first-shadow cache's key and is emptied with it.  RT_FIRST_SHADE_CACHE=0
 * turns it off, and so does either older knob; a scene with a textured mesh is not eligible.  Frames are the same bit for bit.  Since the context was created: chains
 * that resumed, chains that filled the cache, chains that were not eligible (whatever makes the first-shadow cache ineligible, a textured mesh, or the knob), and
 * replacements of the key that emptied a filled cache.  A resumed chain counts as a skip in rt_first_hit_cache_counts and rt_first_shadow_cache_counts: both keep their
 * meaning. */
int rt_first_shade_cache_counts(const rt_ctx *ctx, uint64_t out[4]);

int rt_synchronize(rt_ctx *ctx);
int rt_get_stats(rt_ctx *ctx, rt_stats *stats);        /* waits for the last render to finish */
/* trav_ms / trav_launches are measured only on request (on != 0): production frames record no per-launch timing events */
int rt_stats_enable(rt_ctx *ctx, int on);
/* Frames in flight for a caller that renders frame after frame on ONE stream into ALTERNATING device buffers (rt_render_device,
 * rt_render_pose_device).  A frame is rendered as two sub-frames on two internal streams; normally both are forked from the caller's
 * stream when the call is made and joined back into it, so frame k+1 starts when ALL of frame k has finished and one internal stream
 * idles at every frame boundary (~5 % of a 1080p frame).  With pipelining on, a frame whose output buffer does not overlap the previous
 * frame's is ordered behind what was on the caller's stream when the PREVIOUS render call was made, and each of its sub-frames follows
 * the same sub-frame of the previous frame directly.  What the caller gives up: work submitted to the stream BETWEEN two render calls
 * is not waited for by the second call's kernels (work submitted before the first of the two is; consumers of a frame submitted after
 * its call still see it complete, the join into the caller's stream stays).  So: alternate between two (or more) output buffers, and
 * do not let anything the frame depends on -- a fill of its buffer, a wait for a reader on another stream -- be younger than the previous
 * call.  Same stream, same size and parameters' layout, else the frame falls back to the full fork (results never change, only overlap).
 * rt_render_async does this internally for its two slots (RT_ASYNC_PIPELINE=0 turns that off).  Off by default.
 * What the library can check it does: work it put on the stream itself since the previous render call (rt_tonemap_device) is remembered
 * with the buffers it reads and writes; a frame that would render into one of them takes the full fork instead (product build: results
 * and ordering stay right, only the overlap is lost) and is REFUSED with RT_ERR_INVALID by a -DRT_DEBUG build
 * (libraytrace_hip_debug.so), so that a test run shows the sequence breaks the rule.  Work the caller submits through HIP directly is
 * invisible to any library: that part of the rule stays the caller's. */
int rt_ctx_set_pipelining(rt_ctx *ctx, int on);

/* --- pipelined frames for a host caller.  optimized.cu renders, synchronises and then copies (optimized.cu:849-856), so the
 *     33 MB of a 1080p float frame cross PCIe strictly after the kernels.  rt_render_async renders the whole frame into one of
 *     two device buffers (slot 0 / 1) and starts its device-to-host copy on a separate copy stream; rt_wait(slot) blocks until that
 *     slot's frame is in out_host.  Calling rt_render_async(slot ^ 1) before rt_wait(slot) overlaps frame k's copy with frame
 *     k+1's kernels.  out_host: width*height float4 (rgb8 == 0) or width*height*3 bytes (rgb8 != 0: the tonemapped image of
 *     cpu:714-716); memory from rt_host_alloc makes the copy one DMA.  Re-using a slot whose frame has not been waited for is
 *     allowed: its kernels wait for the pending copy. */
int rt_render_async(rt_ctx *ctx, const rt_params *p, int slot, void *out_host, int rgb8);
int rt_wait(rt_ctx *ctx, int slot);
/* every device buffer of the context lives on the context's device (RT_ERR_INTERNAL otherwise): a context used from a thread
 * whose current device is another GPU must not allocate there (the CUDA programs of the reference only ever see device 0) */
int rt_ctx_selfcheck(rt_ctx *ctx);

/* --- pinned host memory for frame buffers.  optimized.cu copies its image into pageable memory (`new char[]`,
 *     optimized.cu:851-856); a buffer from rt_host_alloc lets the D2H copy of rt_render / rt_render_rgb8 /
 *     rt_render_multi run as one DMA at the PCIe rate instead of being staged by the runtime. ------------------ */
int rt_host_alloc(void **ptr, size_t bytes);
int rt_host_free(void *ptr);
/* device memory on the context's device for rt_render_device / rt_tonemap_device callers that have no HIP of their own
 * (the C++ host API stays free of hip_runtime.h) */
int rt_device_alloc(rt_ctx *ctx, void **ptr, size_t bytes);
int rt_device_free(void *ptr);
int rt_device_to_host(rt_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* synchronous copy on the context's stream */

/* --- a batch of explicit rays through the PRODUCTION traversal launches.  TriangleMesh::intersect (cpu_launcher.cpp:238-313,
 *     optimized.cu:220-285) is callable with any ray; this entry writes the caller's rays into the traversal queue exactly as the
 *     render path's emitter does (root-box test of cpu:279 included) and runs the same kernel instantiation with the launch geometry
 *     of a frame: variant RT_VARIANT_WAVEFRONT_QUEUE (or AUTO: wf_travq, the default traversal), RT_VARIANT_WAVEFRONT (wf_trav) or
 *     RT_VARIANT_PATH (wf_path).  rays: n x 6 floats (O.xyz, u.xyz; u is used as given, the reference does not renormalise either);
 *     out: n x 5 floats (hit 0 / 1, t, N.xyz normalised as cpu:308; a miss leaves t = 1e9 = INF narrowed, cpu:283).
 *     tri_tmin: the leaf loop's t > tri_tmin (cpu:301: 1e-4; 0 = moller_trumbore's own t > 0). */
int rt_trace_rays(rt_ctx *ctx, const float *rays, int n, float tri_tmin, int variant, float *out);

/* --- known-answer entry points (test interface; same library, same device functions the render kernels inline).
 *     One lane per row.  Inputs/outputs use the layouts of tests/golden/kat.npz, which the reference's own functions
 *     produced (oracle/ref_harness.cpp):
 *       sphere   in C[3] R O[3] u[3]          out hit t N[3]      Sphere::intersect, cpu:512-527
 *       box      in mn[3] mx[3] O[3] u[3]     out hit             BoundingBox::intersect, cpu:146-157
 *                route 0 literal divisions, 1 slab_filtered (root-box pre-test, stackless walks), 2 qbox_filter + literal
 *                fall-back (work-stack kernels)
 *       triangle in A[3] B[3] C[3] O[3] u[3]  out hit t N[3]      moller_trumbore, cpu:226-236 (N = e1 x e2, unnormalised)
 *       mesh     in O[3] u[3]                 out hit t N[3]      TriangleMesh::intersect, cpu:238-313, on the uploaded mesh
 *                route 0 the work-stack kernels' primitives, 1 the stackless mesh_intersect of the lock-step kernels
 *     counts: how many tests the error-bounded filters decided and how many fell back to the literal divisions. --- */
typedef struct rt_kat_counts {
    uint64_t n;
    uint64_t box_decided, box_literal;
    uint64_t tri_decided, tri_literal;
} rt_kat_counts;
int rt_kat_sphere(rt_ctx *ctx, const float *in, int n, float *out);
int rt_kat_sqrt(rt_ctx *ctx, const float *in, int n, float *out);   /* out[i] = the device's correctly rounded square root (every sqrt of cpu_launcher.cpp: Vector::norm, Sphere::intersect, getColor) */
int rt_kat_box(rt_ctx *ctx, const float *in, int n, int route, float *out, rt_kat_counts *counts);
int rt_kat_triangle(rt_ctx *ctx, const float *in, int n, float *out, rt_kat_counts *counts);
int rt_kat_mesh(rt_ctx *ctx, const float *in, int n, float tri_tmin, int route, float *out, rt_kat_counts *counts);
/* 64-bit hashes of the device-side node layouts the upload (or a refit / rebuild) derived for the traversal kernels: [0] float sibling pairs, [1] 16-bit fixed-point
 * pairs, [2] 4-wide quads (which four nodes a quad holds is chosen by a surface-area DP on the device), [3] leaf boxes by triangle; 0 = not in use.  Two uploads of one
 * tree give equal hashes: the layouts -- and with them the work a frame does -- are a function of the tree alone. */
int rt_kat_layout_hash(rt_ctx *ctx, uint64_t out[4]);

/* --- device-side mesh transform: the `transform` kernel of global_launcher.cu:340-365 / transformMesh
 *     (realtime_render.cu:1151-1166) applied to the uploaded vertices -- v' = R v (row-major 3x3), then += translation --
 *     followed, on the device, by the triangle precompute and a REFIT of the BVH: same tree, same triangle order, every
 *     node's box recomputed as compute_bbox (cpu_launcher.cpp:180-188) of its range.  (The reference never refits: to get
 *     the tree buildBVH would build for the moved mesh, rebuild on the host and call rt_scene_upload.) ------------------ */
int rt_mesh_transform(rt_ctx *ctx, const float rotation[9], const float translation[3]);

/* --- device-side BVH BUILD: TriangleMesh::buildBVH (cpu_launcher.cpp:190-224; the reference's device twin is the
 *     one-thread recursive buildBVH of global_launcher.cu:298-331, launched by KernelInit :848-881) over the uploaded triangles
 *     with the vertices as they are on the device now (i.e. after rt_mesh_transform): level by level, one workgroup per node --
 *     box of the range, longest axis, midpoint split, the reference's in-place partition, its stop rule -- then the numbering
 *     of bvhTreeToArray (optimized.cu:512-534).  The tree equals the host builder's bit for bit: boxes, node indices, and the
 *     order the partition leaves the triangles in.  The library then re-lays the mesh out for its kernels as rt_scene_upload
 *     does; the uploaded order becomes the new BVH order (the reference partitions `indices` in place too).
 *     Optional outputs: bvh_arr10_out (capacity (2 * n_triangles + 2) * 10 floats), tri_order_out[n_triangles] (position ->
 *     index of the triangle in the order before this call), n_nodes_out.
 *     Failure: an error during the BUILD leaves the scene in use untouched.  An allocation failure during the re-layout that
 *     follows (RT_ERR_HIP: out of device memory) leaves the context WITHOUT a scene (RT_ERR_NO_SCENE from the render calls):
 *     upload again.  Cost model: one workgroup per node and one blocking read-back per level, so the top levels of a mesh far
 *     larger than the cat's 3 954 triangles run on a single CU each (the build is a step before the hot path, not part of it). */
int rt_mesh_rebuild(rt_ctx *ctx, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out);   /* = rt_mesh_rebuild_mode(RT_BVH_REFERENCE) */

/* --- ... or a DIFFERENT, better tree, built in parallel (SURVEY 8f3 "and a GPU LBVH build"; opt-in, RT_BVH_REFERENCE stays the default
 *     everywhere).  The reference's stop rule (cpu_launcher.cpp:217) leaves leaves that grow with the mesh -- 2 M triangles: 357 triangle
 *     tests per ray -- and its device builder is ONE thread (global_launcher.cu:298-331, :848-881).  RT_BVH_LBVH: Morton codes of the
 *     triangle centroids (63 bits), radix sort, the binary radix tree over the sorted codes with one thread per node (Karras 2012),
 *     boxes bottom-up by min / max of the vertex coordinates (the values compute_bbox, cpu:180-188, folds for the node's range), and for
 *     every node the surface-area heuristic's choice between ONE leaf (at most 32 triangles) and its subtree -- the reference's traversal
 *     never prunes by distance, so a ray pays for every box it pierces and every triangle of every leaf it enters: the cost the SAH models.  Same outputs in the same formats -- the flat `float[10]` tree of bvhTreeToArray and the order the
 *     triangles are left in -- so every kernel variant runs on it unchanged and a CPU checker can be handed the very same tree
 *     (oracle: or_mesh_set_bvh).  What changes against the reference tree: WHICH triangles a ray tests (far fewer), never what a
 *     test returns; the image differs from the reference tree's only where two triangles are hit at bit-equal t (shared edges: the
 *     scan order breaks the tie, cpu:301 / SURVEY H5).  A mesh of at most four triangles is a single leaf in either mode (the reference builder runs).
 *     rt_mesh_build_stats: what the last rebuild did (device_build_ms = the builder's kernels, HIP events; install_ms = the
 *     re-layout for the render kernels that follows, host side). */
typedef enum rt_bvh_mode { RT_BVH_REFERENCE = 0, RT_BVH_LBVH = 1 } rt_bvh_mode;
typedef struct rt_build_stats {
    int32_t mode;                  /* the mode that ran                                        */
    int32_t n_triangles, n_nodes;
    int32_t n_leaves, max_leaf_tris, max_depth;   /* RT_BVH_LBVH only (0 otherwise)            */
    float   device_build_ms;       /* builder kernels + sort, HIP events on the context's stream */
    float   install_ms;            /* the kernels' formats: on the device for RT_BVH_LBVH (closed forms over the builder's arrays), else
                                      read-back + re-layout on the host + upload; wall clock                                    */
    int32_t install_on_device;
    int32_t reserved;
} rt_build_stats;
int rt_mesh_rebuild_mode(rt_ctx *ctx, int mode, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out);
int rt_mesh_build_stats(const rt_ctx *ctx, rt_build_stats *out);

/* --- smooth (interpolated) normals: get_smooth_normal of realtime_render.cu:221-245 / global_launcher.cu:207-231
 *     -- beta, gamma by the literal divisions, alpha = 1 - beta - gamma, N = normalize(alpha Na + beta Nb + gamma Nc) --
 *     replaces the flat normal of the winning triangle.  normals_xyz: n_normals * 3; nidx: TriangleIndices::ni,nj,nk of
 *     triangle t at nidx[t * index_stride .. +2], triangles in the order of rt_mesh.indices (for a TriangleIndices array
 *     pass &indices[0].ni and stride 10).  Call after rt_scene_upload (a new upload drops them); NULL = flat again.
 *     rt_mesh_transform then moves the normals the way the reference's kernel does.  Wavefront variants only. ---------- */
int rt_mesh_set_normals(rt_ctx *ctx, const float *normals_xyz, int n_normals, const int32_t *nidx, int index_stride, int n_triangles);

/* --- the same for ONE mesh of the scene (ABI 6, additive): the reference's classes give every TriangleMesh in Scene::objects its own normals and its own tree
 *     (cpu_launcher.cpp:190-224, :538-564) and its transformMesh moves the arrays of one mesh (global_launcher.cu:932-946).  object_slot = rt_mesh.object_slot
 *     at upload (the mesh's position in Scene::objects).  On a scene with one mesh each equals its plain entry; on a forest of several meshes:
 *       transform_of    the mesh's vertices (its smooth normals too, translation added), its triangle records, then a refit of the whole forest (the synthetic union
 *                       nodes above the meshes' roots widened by one float step per face, as an upload makes them: the layout equals a fresh upload of the moved meshes);
 *       set_normals_of  nidx rows in the mesh's own triangle order (as uploaded, or as its last rt_mesh_rebuild_of reported), normal indices into its own array;
 *                       NULL arrays = that mesh flat again; the other meshes keep their shading;
 *       rebuild_of      mode as rt_mesh_rebuild_mode, over the mesh's triangles and current vertices; bvh_arr10_out (capacity (2 * n + 2) * 10 floats, n = the mesh's
 *                       triangles), tri_order_out[n] and n_nodes_out are in the mesh's own index space -- what buildBVH makes of that TriangleMesh; every other mesh
 *                       keeps its tree, vertices and boxes as the device holds them; the forest is re-laid out on the host (no device-side install).
 *     RT_ERR_INVALID: object_slot outside the scene or a sphere's (scene unchanged).  A mesh without triangles: RT_OK, nothing happens.  RT_ERR_NO_SCENE: no upload,
 *     or the last rt_scene_upload* failed.  Failures as the plain entries: a build error leaves the scene as it was. ------------------------------------------ */
int rt_mesh_transform_of(rt_ctx *ctx, int object_slot, const float rotation[9], const float translation[3]);
int rt_mesh_set_normals_of(rt_ctx *ctx, int object_slot, const float *normals_xyz, int n_normals, const int32_t *nidx, int index_stride, int n_triangles);
int rt_mesh_rebuild_of(rt_ctx *ctx, int object_slot, int mode, float *bvh_arr10_out, int32_t *tri_order_out, int32_t *n_nodes_out);

/* --- deforming meshes (ABI 6, additive): new positions for every vertex of a mesh, in place -- a skinned, simulated or morphing mesh, once per frame.  n_vertices must
 *     equal the count the mesh was uploaded with, the Vectors in the uploaded order.  Everything else stays: the triangle indices, the tree's topology and visit order
 *     (a REFIT, not a rebuild), materials, the normals that were set, textures and UVs, the transforms applied so far (the new positions simply replace their result).
 *     The entry then does on the device what rt_mesh_transform does after moving the vertices: the triangle records of the mesh, every box of the tree in use (a leaf's
 *     box is compute_bbox, cpu_launcher.cpp:180-188, of its triangles; a forest's synthetic union nodes widened by one float step as an upload makes them), the
 *     fixed-point layouts -- the layout equals, bit for bit, a fresh upload of (new vertices, same triangle order, the refitted tree), and both caches of a still view
 *     are emptied.  The boxes are made across the whole chip (every leaf a thread, the internal nodes by a bottom-up climb in which no lane waits for another),
 *     rt_mesh_transform's one-workgroup refit bit for bit; RT_REFIT_WIDE=0 selects that one here too.
 *       rt_mesh_set_vertices         the scene's one mesh (RT_ERR_UNSUPPORTED on a scene of several, as rt_mesh_set_normals), xyz_host: n_vertices * 3 floats;
 *       rt_mesh_set_vertices_of      the mesh at object_slot (= rt_mesh.object_slot at upload);
 *       rt_mesh_set_vertices_device  positions in DEVICE memory, records stride_floats (3 or 4) floats apart, read on the context's own stream in the order of
 *                                    the call (as rt_mesh_transform's launches are ordered: work the caller issued on ANOTHER stream is the caller's to finish
 *                                    first); object_slot -1 = the scene's one mesh.
 *     SMOOTH NORMALS ARE THE CALLER'S DATA, as in the reference (TriangleMesh::normals comes from the file), and these entries leave them alone.  A caller that
 *     deforms a smooth mesh either passes the normals of the new shape to rt_mesh_set_normals[_of] again, or has them made on the device from the new shape:
 *     rt_mesh_compute_normals[_of] below.
 *     The call WAITS on the context's stream once, for the refitted root box (32 bytes): it travels to the render kernels as an argument and the fixed-point grid
 *     hangs on it -- the same wait rt_mesh_transform has.
 *     A refit keeps the topology: after large deformations the boxes overlap more and a ray does more work, never different work's result.  Rebuild now and then
 *     (rt_mesh_rebuild_mode(RT_BVH_LBVH)).
 *     RT_ERR_INVALID (scene untouched): a NULL pointer, n_vertices different from the mesh's, a stride other than 3 or 4, object_slot outside the scene or a
 *     sphere's.  A mesh without triangles: RT_OK, nothing happens.  RT_ERR_NO_SCENE: no upload, or (the _of and device forms) the last rt_scene_upload* failed. */
int rt_mesh_set_vertices(rt_ctx *ctx, const float *xyz_host, int n_vertices);
int rt_mesh_set_vertices_of(rt_ctx *ctx, int object_slot, const float *xyz_host, int n_vertices);
int rt_mesh_set_vertices_device(rt_ctx *ctx, int object_slot, const void *xyz_dev, int stride_floats, int n_vertices);

/* --- vertex normals of a mesh's CURRENT shape, computed on the device (ABI 6, additive).  The mesh gets one normal per POSITION vertex -- the area-weighted sum of the
 *     face normals of its incident triangles, normalised -- and then shades with them exactly as if the caller had passed that array to rt_mesh_set_normals[_of] with the
 *     triangles' own vertex indices as nidx.  The reference has no such computation; the arithmetic below is the contract (binary32, one rounding per operation in the
 *     order written, no contraction):
 *       N(t) = cross(B - A, C - A) of triangle t's CURRENT corners (cpu_launcher.cpp:227-229: the N of the triangle's record; twice the area long, so the sum is
 *              area-weighted);
 *       S(v) = the N of the first corner that names v, then S = S + N component by component over the others, in ascending order of the mesh's own triangle order --
 *              as uploaded, or as the last rt_mesh_rebuild* reported: the order rt_mesh_set_normals_of's nidx rows follow -- corners 0, 1, 2 within a triangle; a
 *              triangle that names v twice contributes twice.  (A triangle that lies in no leaf of the tree is never hit and takes no part.)
 *       n(v) = S / sqrt((S.x S.x + S.y S.y) + S.z S.z) with the correctly rounded square root and divisions of every normalisation here (cpu:58-63), or (0, 0, 0)
 *              where that sum of squares is not > 0: a vertex no triangle names, faces that cancel or are all degenerate, a NaN.  A zero vertex normal drops out of
 *              the interpolation of get_smooth_normal;
 *       every corner k of every triangle t of the mesh then shades with n(vertex k of t).
 *     The work runs on the context's own stream in the order of the call, behind the rt_mesh_set_vertices* / rt_mesh_transform* issued so far (work the caller issued on
 *     ANOTHER stream is the caller's to finish first).  The FIRST call after an upload or a rebuild builds the mesh's adjacency on the host and uploads it; later calls
 *     enqueue two launches and do not wait.  The shading-level caches of a still view are emptied, as by rt_mesh_set_normals.
 *       rt_mesh_compute_normals      the scene's one mesh (RT_ERR_UNSUPPORTED on a scene of several, as rt_mesh_set_normals);
 *       rt_mesh_compute_normals_of   the mesh at object_slot; the other meshes' normals and shading stay.
 *     What follows from the normals being ordinary smooth normals: rt_mesh_transform* rotates AND translates them as any others (the reference's kernel does); a rebuild
 *     carries them with their triangles; rt_mesh_set_normals_of(.., NULL, ..) returns the mesh to flat shading; a later rt_mesh_set_normals_of with the caller's own array
 *     replaces them; textures and UVs stay.  THE RECIPE for a smooth mesh that changes shape: rt_mesh_set_vertices*, then rt_mesh_compute_normals*, then the frame.
 *     rt_mesh_get_vertex_normals copies the per-vertex normals (n_vertices * 3 floats, the uploaded vertex order) to the host as the last rt_mesh_compute_normals* of
 *     that mesh wrote them, with one wait on the stream; object_slot -1 = the scene's one mesh.  It does NOT follow a later rt_mesh_transform* (which moves the corners'
 *     copies, not this array).  RT_ERR_INVALID: none was computed for the mesh since the upload, n_vertices is not the mesh's, a NULL pointer.
 *     Errors otherwise as rt_mesh_set_vertices*; a mesh without triangles: RT_OK, nothing happens. */
int rt_mesh_compute_normals(rt_ctx *ctx);
int rt_mesh_compute_normals_of(rt_ctx *ctx, int object_slot);
int rt_mesh_get_vertex_normals(rt_ctx *ctx, int object_slot, float *out_xyz, int n_vertices);

/* --- textured meshes (ABI 6, additive): MTL's map_Kd over OBJ's per-corner vt.  The albedo of a hit on a textured mesh is
 *     mesh albedo (.) sampled texel (Kd x map_Kd), a per-channel binary32 product with the mesh albedo first; it replaces the albedo
 *     of the fold (cpu:624, 642) and nothing else: the mesh stays diffuse, mirror or glass by its rt_mesh fields.  Every operation below
 *     is one IEEE binary32 rounding in the order written (the library is built with -ffp-contract=off), so a float32 model reproduces it:
 *       uv       alpha, beta, gamma exactly as smooth shading computes them (beta = dot(e2, cross(A - O, u)) / dot(u, N), gamma = -dot(e1, ...) /
 *                dot(u, N), alpha = 1 - beta - gamma; A, e1 = B - A, e2 = C - A, N = e1 x e2 of the hit triangle, (O, u) the ray), then
 *                uv = (alpha uv_a + beta uv_b) + gamma uv_c per component;
 *       texel    8-bit RGB or RGBA, width x height texels, the first row given is the TOP of the image, alpha is never read; a channel's
 *                value is decode[byte] (256 floats from the caller; NULL = byte / 255.0f, correctly rounded);
 *       nearest  x = floor(u W), y = floor((1 - v) H);
 *       bilinear s = u W - 0.5, t = (1 - v) H - 0.5, x0 = floor(s), fx = s - x0, y0 = floor(t), fy = t - y0, x1 = x0 + 1, y1 = y0 + 1;
 *                value = (T(x0,y0) (1 - fx) + T(x1,y0) fx) (1 - fy) + (T(x0,y1) (1 - fx) + T(x1,y1) fx) fy;
 *       wrap     on the integer indices: repeat = non-negative modulo, clamp = into [0, W - 1] / [0, H - 1];
 *       range    a coordinate (u W, (1 - v) H, s or t) that is NaN or outside [-2^31, 2^31) gives index 0 and fraction 0 (before the wrap).
 *     So a texture whose every texel decodes to c renders exactly as the untextured mesh with albedo fl(albedo c) (nearest filtering).
 *     uvs: n_uvs x 2 floats (OBJ vt); uvidx: the UV indices of triangle t's three corners at uvidx[t * index_stride .. + 2], triangles in the
 *     mesh's uploaded order (or as its last rebuild reported; for a TriangleIndices array pass &indices[0].uvi and stride 10).  The library
 *     copies everything.  uvs, uvidx or tex NULL: the mesh untextured again (rt_mesh_set_texture: every mesh).  rt_scene_upload* clears all
 *     textures; rt_mesh_transform* keep the UVs (they belong to the corners); rt_mesh_rebuild* carry them with their triangles.
 *     RT_ERR_INVALID, nothing changed: a bad object_slot or a sphere's, a UV index outside [0, n_uvs), n_triangles below the mesh's count,
 *     width or height <= 0, channels other than 3 / 4, an unknown filter or wrap.  A mesh without triangles: RT_OK, nothing happens.
 *     Variants: those that run wf_advance -- auto, wavefront, wavefront_lds, wavefront_queue, lds_* (frames, batches, poses, progressive
 *     frames, num_rays > 1); a textured scene makes path, lockstep and global return RT_ERR_UNSUPPORTED.  rt_multi_* contexts stay
 *     untextured.  Spheres are never textured. --------------------------------------------------------------------------------------- */
typedef enum rt_tex_filter { RT_TEX_NEAREST = 0, RT_TEX_BILINEAR = 1 } rt_tex_filter;
typedef enum rt_tex_wrap { RT_TEX_REPEAT = 0, RT_TEX_CLAMP = 1 } rt_tex_wrap;
typedef struct rt_texture {
    const uint8_t *texels;         /* height rows of width texels, top row first, channels bytes each */
    int32_t        width, height, channels;
    int32_t        filter, wrap;   /* rt_tex_filter, rt_tex_wrap                                       */
    const float   *decode;         /* 256 floats, or NULL = byte / 255                                  */
} rt_texture;
int rt_mesh_set_texture(rt_ctx *ctx, const float *uvs, int n_uvs, const int32_t *uvidx, int index_stride, int n_triangles, const rt_texture *tex);
int rt_mesh_set_texture_of(rt_ctx *ctx, int object_slot, const float *uvs, int n_uvs, const int32_t *uvidx, int index_stride, int n_triangles, const rt_texture *tex);
/* known answers of the texture lookup: rays (n x 6: O, u) through the production traversal (wf_travq), then the device function the
 * shading kernel calls for the hit.  out: n x 8 = (object slot of the mesh hit or -1, triangle index in that mesh's uploaded order, t,
 * u, v, albedo rgb); an untextured mesh reports uv = (0, 0) and its own albedo, a miss (-1, -1, 1e9, 0, ...). */
int rt_kat_surface(rt_ctx *ctx, const float *rays, int n, float tri_tmin, float *out);

/* --- posed camera + progressive accumulation: the headless form of realtime_render.cu.  Camera
 *     {C, yaw, pitch} with Camera::rotate() (realtime_render.cu:803-861); ray generation and per-sample averaging of its
 *     KernelLaunch (:1100-1134: u_center = C + bz*z + bx*X + by*Y, outcolor += color * (1./num_rays)); accumulation and
 *     display of :1136-1147 (accumbuffer += frame; display = accumbuffer / framenumber; powf(c, 1/2.2f)); the frame's RNG
 *     seed is WangHash(framenumber) (:1190-1197, :1268).  Wavefront variants only.  Parity: PINNED.  The reference's own
 *     Camera::rotate and KernelLaunch, run as host functions, wrote tests/golden/ref_realtime.npz (the basis, every camera
 *     ray of small frames with and without jitter, the 8-bit output around every code boundary); the oracle and
 *     rt_camera_basis equal it bit for bit (tests/test_realtime_pinned.py), the device equals it through smooth normals of
 *     those rays and through the oracle (tests/test_gpu_realtime_pinned.py).
 *     ONE RECORDED DEVIATION, rt_render_pose and everything posed: z = -W / (2 tan(fov / 2)) uses the CORRECTLY ROUNDED
 *     binary32 tangent (binary64 tan, narrowed), as the fixed camera does where g++ folds cpu:694; realtime:1112 calls tanf
 *     at run time, which is not correctly rounded and may differ between C libraries.  Of the fovs pi / 2, pi / 3, 1.0 and
 *     0.7 the two differ at pi / 3 alone (0x1.279a74p-1 here, 0x1.279a76p-1 from glibc's tanf); there the rays equal the
 *     reference's once z is the reference's. ----------- */
typedef struct rt_camera_pose { float position[3]; float yaw; float pitch; float fov; } rt_camera_pose;
int rt_camera_basis(const rt_camera_pose *pose, float bx[3], float by[3], float bz[3]);   /* Camera::rotate(), host */
/* one frame with the posed camera (no accumulation): full frame to host / rows to device memory */
int rt_render_pose(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, float *out_rgba_host);
int rt_render_pose_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, void *out_rgba_dev, void *stream);
/* disp(): buffer_reset / frames++ / KernelLaunch / display.  Outputs may be NULL.  display: height*width float4
 * (.xyz = accumulated colour / frames, .w = rays traced so far); rgb8: interleaved RGB8 */
int rt_progressive_reset(rt_ctx *ctx);
int rt_progressive_frame(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, float *display_rgba_host, uint8_t *rgb8_host);
int rt_progressive_frames(const rt_ctx *ctx, int *frames);
/* The 8-bit image of rt_progressive_frame is realtime:1136-1147, in binary32: v = (double)powf(c, 1 / 2.2f); if (!(v < 255.)) v = 255.; (unsigned char)v.
 * Its exponent is the binary32 1 / 2.2f, not 1./2.2: its code boundaries are not rt_tonemap_device's.  Special values, as the reference's own kernel recorded them
 * (tests/golden/ref_realtime.npz): NaN -> 255 (it fails the `<`); a negative c, -1e-45 and -inf included -> powf is NaN -> 255; +-0 -> 0; +inf -> 255.
 * Known answer (ABI 6, additive): rt_kat_progressive runs the production kernel of rt_progressive_frame on the caller's values.  n float4 of accumbuffer and of the
 * new frame in; accumbuffer + frame, the display values (accumbuffer * (1.0f / framenumber), .w = accumbuffer.w) and the n * 3 bytes out, each may be NULL.  Host
 * memory; no scene is needed, and the context's own progressive state (rt_progressive_frames, its buffers) is untouched.  RT_ERR_INVALID: n < 0, framenumber < 1,
 * a NULL input with n > 0.  n == 0 writes nothing. */
int rt_kat_progressive(rt_ctx *ctx, const float *accum_in, const float *frame, int n, int framenumber, float *accum_out, float *display_out, uint8_t *rgb8_out);

/* --- first-hit feature buffers (G-buffer) and an edge-avoiding denoiser (ABI 6, additive).  A frame of one sample per pixel is noise; the remedy that needs
 *     no further frames is a filter guided by what the camera ray of each pixel hit first.
 *     rt_render_aov*: for every pixel of `rows` the pixel-centre camera ray -- the fixed camera of cpu:694-699 (pose == NULL) or the posed camera of
 *     rt_render_pose; p->sigma, num_rays, num_bounce, seed and variant are ignored -- is intersected with the scene exactly as Scene::intersect_all does
 *     (cpu:545-564: all spheres and all meshes in object order, strict '<', p->tri_tmin at the leaves; the meshes through the production traversal).  Output:
 *     THREE dense planes of n_rows * width float4, consecutive in one buffer (plane i starts at byte i * n_rows * width * 16):
 *       plane 0  .xyz = the unit normal Scene::getColor shades the hit with (sphere, flat triangle, or interpolated where normals are set),
 *                .w   = the object id (position in Scene::objects) as a float, -1 on a miss;
 *       plane 1  .xyz = the hit point P = O + t u (cpu:560), .w = 1 on a hit, 0 on a miss;
 *       plane 2  .xyz = the albedo the shading step uses: the object's, or mesh albedo (.) texture sample on a textured mesh; .w = 0.
 *     A miss writes zeros in every .xyz.  The FIRST hit is recorded whatever its material: a mirror or glass object reports itself, not what it reflects or
 *     refracts.  The call reads the scene as a render call does, keeps its own queue (it may be issued between two frames in flight), and is asynchronous on
 *     `stream` (NULL = the context's own).  rt_render_aov copies the planes to the host; rows == NULL = the whole frame.
 *     rt_denoise*: n_passes passes of the a-trous filter over a width x height float4 colour frame (.w = the ray count, as rt_render* writes it) guided by the
 *     three planes of the same frame.  The arithmetic is the contract -- binary32, one rounding per operation, no contraction.  Pass k = 0 .. n_passes - 1,
 *     step s = 2^k, input frame C (the colour, then the previous pass's output); pixel p = (x, y) with id_p, N_p, P_p, A_p from the planes:
 *       id_p == -1: out = C_p.  Otherwise, for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = (x + dx s, y + dy s), skipped if outside the image or id_q != id_p:
 *         h  = H[|dy|] * H[|dx|], H = {3/8, 1/4, 1/16};
 *         dn = (N_p.x - N_q.x)^2 + (N_p.y - N_q.y)^2 + (N_p.z - N_q.z)^2, summed left to right; da (albedos) and dc (C_p.rgb, C_q.rgb) in the same form;
 *         e  = N_p.x (P_q.x - P_p.x) + N_p.y (P_q.y - P_p.y) + N_p.z (P_q.z - P_p.z), dp = e e: q's squared distance from p's tangent plane;
 *         wn = max(0, 1 - dn k_normal), wp, wa likewise with k_position, k_albedo; wc with k_color 4^k (the colour tolerance halves per pass);
 *         a k_* of exactly 0 makes its term exactly 1;
 *         w  = h wn wp wa wc, multiplied left to right; the tap counts only if w > 0 (a NaN guide does not spread): S += w C_q.rgb, W += w;
 *       out.rgb = S / W (correctly rounded; the centre tap always contributes 9/64), out.w = C_p.w.
 *     RT_ERR_INVALID, output untouched: n_passes outside [1, RT_DENOISE_MAX_PASSES], an output that overlaps the colour frame or the planes, a NULL pointer,
 *     width or height <= 0, 2^28 pixels or more, or a frame so thin that a pass would need 2^31 workgroups (a pass tiles each of its s x s sub-images by 32 x 8:
 *     one or two pixels of width and more than 2^27 - 1024 rows with n_passes 8, one pixel and more than 2^28 - 512 rows with n_passes 7; rt_denoise_var likewise).
 *     Whole frames only: a row share of a tiled multi-GPU frame lacks the 2 (2^n_passes - 1)-row halo -- denoise the gathered frame. --- */
#define RT_DENOISE_MAX_PASSES 8
typedef struct rt_denoise_params {
    int32_t n_passes;              /* 1 .. RT_DENOISE_MAX_PASSES                                    */
    float   k_normal, k_position, k_albedo, k_color;
} rt_denoise_params;
int rt_render_aov_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, void *out_aov_dev, void *stream);
int rt_render_aov(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, float *out_aov_host);
int rt_denoise_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, int width, int height, const rt_denoise_params *dp, void *out_rgba_dev, void *stream);
int rt_denoise(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, int width, int height, const rt_denoise_params *dp, float *out_rgba_host);

/* --- temporal accumulation with reprojection, and the filter guided by variance (ABI 6, additive): the spatiotemporal half of the denoiser (SVGF).  A moving
 *     scene never gets more than one sample per pixel from rt_progressive_frame; the planes of rt_render_aov* hold what reusing earlier frames needs.  The caller
 *     owns all state: per frame it keeps the planes and the history it was given, and hands them back as "previous" with the next frame.
 *     rt_temporal_accumulate*: inputs -- the current width x height colour frame C (float4, .w = rays), the current planes (planes 0 and 1 are read; the albedo
 *     plane is not an input), the previous frame's planes 0 and 1 (2 * width * height float4), the previous history, a reprojection record.  Output: the new
 *     HISTORY, two dense planes of width * height float4, consecutive:
 *       history plane 0  .xyz = the accumulated colour, .w = C_p.w (the current frame's ray count);
 *       history plane 1  (m1, m2, n, V) = the first and second moment of the luminance l = (0.2126 r + 0.7152 g) + 0.0722 b, the history length, the variance.
 *     prev_aov == NULL and prev_history == NULL (both or neither): the first frame, or a cut; nobody has history.  `rp` (required with a previous frame):
 *       posed == 0: the previous camera is `camera` (cpu:694-699); posed == 1: it is `pose` with the basis of rt_camera_basis.  The POSED CAMERA adds its
 *       position INTO the ray direction (realtime_render.cu:1115: u = normalize(C + bz z + bx X + by Y), ray origin C): the projection below inverts exactly
 *       that, not a textbook camera;
 *       motion: NULL = nothing moved, else RT_MAX_OBJECTS records indexed by object id, each the rigid motion "previous from current" of that object:
 *       P_prev = rotation (3 x 3, row-major) P_cur + translation (a sphere moved by rt_scene_move_sphere: identity, previous centre - current centre; a mesh moved
 *       by rt_mesh_transform_of(R, T): R^T, -R^T T);
 *       no_history_mask: bit i set = object i never reuses history (mirror and glass report themselves in the planes, not what they show: mask them).
 *     The arithmetic is the contract -- binary32, one rounding per operation, no contraction, sums left to right, quotients correctly rounded.  Constants from
 *     the record: O = the previous camera's position; (bx, by, bz) = its basis, the identity when posed == 0; z = -(float)width / (2 (float)tan((double)(fov / 2)));
 *     posed: cx = O.bx, cy = O.by, b = O.bz + z, each dot (O.x b.x + O.y b.y) + O.z b.z; fixed: cx = cy = 0, b = z.  Pixel p = (x, y), id_p = plane 0 .w:
 *       id_p == -1 (a miss): history 0 = C_p, history 1 = (0, 0, 0, 0).  Otherwise l = l(C_p) and, to begin with, n = 1, colour = C_p.rgb, m1 = l, m2 = l l.
 *       If a previous frame is given and bit id_p of the mask is clear:
 *         motion != NULL: P' = ((R0 P.x + R1 P.y) + R2 P.z) + T0 (rows 1, 2 likewise), N' = (R0 N.x + R1 N.y) + R2 N.z; motion == NULL: P' = P_p, N' = N_p;
 *         d = P' - O;  k = b / ((d.x bz.x + d.y bz.y) + d.z bz.z);  X = ((d.x bx.x + d.y bx.y) + d.z bx.z) k - cx;  Y likewise with by, cy;
 *         gx = X + (float)width / 2,  gy = (float)height / 2 - Y   (previous pixel (i, j)'s centre is gx = i + 0.5, gy = j + 0.5);
 *         no history unless k > 0 (else P' is behind the camera) and -1 <= gx <= width and -1 <= gy <= height;
 *         ix = floor(gx), iy = floor(gy) (the nearest previous pixel, round half up); jx = ix + 1 if gx - floor(gx) >= 0.5 else ix - 1; jy likewise;
 *         the taps q = (ix, iy), (jx, iy), (ix, jy), (jx, jy) in this order; the FIRST valid one wins.  q is valid when it lies inside the image, id_q == id_p,
 *         (N'.x N_q.x + N'.y N_q.y) + N'.z N_q.z >= min_normal_dot, and e e <= max_plane_dist max_plane_dist with
 *         e = (N'.x (P_q.x - P'.x) + N'.y (P_q.y - P'.y)) + N'.z (P_q.z - P'.z)   (N_q, P_q: the PREVIOUS planes).  Nearest, not bilinear: with nothing moving
 *         the history is exactly the running mean and does not blur.
 *         With a valid tap (H_q, (m1_q, m2_q, n_q, .) = the previous history at q): n = min(n_q + 1, (float)max_history), a = max(1 / n, alpha_min),
 *         colour = H_q + a (C_p - H_q) per channel, m1 = m1_q + a (l - m1_q), m2 = m2_q + a (l l - m2_q).
 *       V = max(0, m2 - m1 m1).  While n < 4 it is replaced by the spatial estimate: over dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), the CURRENT frame's pixels
 *       q = (x + dx, y + dy) inside the image with id_q == id_p: s1 += l(C_q), s2 += l(C_q) l(C_q), c += 1; V = max(0, s2 / c - (s1 / c) (s1 / c)).
 *       history 0 = (colour, C_p.w), history 1 = (m1, m2, n, V).
 *     rt_denoise_var*: rt_denoise's passes over history plane 0, with the colour term driven by the variance and the variance filtered along.  Pass k, step
 *     s = 2^k, input colour C (history plane 0, then the previous pass's output) and variance V (history plane 1 .w, then the previous pass's): everything as
 *     stated for rt_denoise except
 *         wc = 1 if dl dl == 0, else max(0, 1 - (dl dl) / D),  dl = l(C_p) - l(C_q),  D = k_sigma V_p + var_floor   (replaces the k_color 4^k term);
 *         and with every tap taken (w > 0): SV += (w w) V_q;   V_out = SV / (W W);   a miss keeps its V.
 *     k_sigma has no unit; var_floor is in the caller's colour units squared.  Output: the filtered colour alone (.w = the history's).
 *     rt_svgf_filter*: rt_denoise_var's inputs (the two history planes of rt_temporal_accumulate*, three guide planes) and its passes, with two switches that finish
 *     SVGF.  Same contract: binary32, one rounding per operation, no contraction, sums left to right with dy outer and dx inner, quotients correctly rounded.  Pass k
 *     (step s = 2^k) is rt_denoise_var's pass word for word, except:
 *       PRE-FILTER (prefilter == 1).  For a pixel p with id_p != -1, over the pass's input variance V: for dy = -1 .. 1 (outer), dx = -1 .. 1 (inner),
 *       q = (x + dx s, y + dy s), skipped if outside the image or id_q != id_p:
 *         g = G[|dy|] * G[|dx|], G = {1/2, 1/4}   (1/4, 1/8, 1/16: exact);   SG += g V_q;   WG += g;
 *         Vg = SG / WG;   D = k_sigma Vg + var_floor   (replaces D = k_sigma V_p + var_floor).
 *       The taps are the pass's own sub-image neighbours: pass 0 is the textbook 3 x 3 Gaussian, later passes smooth at their own step a variance the earlier
 *       passes have already filtered at theirs (a deviation from implementations that always use step 1).  Only D changes: the variance carried to the next pass
 *       is still V_out = SV / (W W) over the unfiltered V_q.
 *       FEEDBACK (feedback_pass == f >= 0).  out_history is a complete history, fit to be the next rt_temporal_accumulate*'s prev_history: plane 0 = (.rgb of pass
 *       f's output, .w of the input history's plane 0); plane 1 = the input history's plane 1, bit for bit -- moments, length and variance stay those of the raw
 *       luminance; only colour is fed back.
 *     With prefilter == 0 and feedback_pass == -1 the output is rt_denoise_var's bit for bit.  out_history is NULL exactly when feedback_pass == -1.
 *     RT_ERR_INVALID, both outputs untouched: any other combination of out_history and feedback_pass; prefilter outside {0, 1}; feedback_pass outside
 *     [-1, n_passes - 1]; everything rt_denoise_var* refuses; any overlap of either output with an input or with the other output.
 *     NON-FINITE INPUTS (all three entries).  min and max above are IEEE minNum and maxNum: of a NaN and a number they give the number; comparisons with a NaN are
 *     false.  So a NaN distance (a NaN in a normal, a position, an albedo, a variance, or in a colour while k_color != 0) makes its term 0 and the tap weigh nothing:
 *     a NaN in a guide or a colour changes no OTHER pixel, unless k_color == 0 in rt_denoise, where a non-finite colour is summed into every pixel whose stencil
 *     takes it (rt_denoise_var's luminance term always weighs it 0).  A pixel whose own weights all vanish -- its own N, P or A is NaN, or its colour is non-finite while k_color != 0 -- is 0 / 0 = NaN in .rgb.
 *     A variance of NaN or 0 with var_floor 0 leaves the taps of equal luminance (the pixel itself among them); the filtered variance carries NaN and Inf on.
 *     rt_svgf_filter's Gaussian excludes no tap for a non-finite V_q: a NaN variance makes Vg and so D NaN for up to nine pixels (the pixels of its object within
 *     one step of it), which then keep only their taps of equal luminance; an Inf variance makes their D Inf (or NaN where k_sigma == 0) likewise.
 *     rt_temporal_accumulate: a NaN in N', P', gx or gy reuses no history; a NaN n_q gives n = max_history; NaN moments, or a non-finite colour among the neighbours of the spatial estimate, give V = max(0, NaN) = 0; a NaN in the
 *     previous history's colour or moments is blended like a number and so stays in that surface point's history until its tap is rejected.  Non-finite history is
 *     not rejected.  The sign and payload of a NaN written are not specified.
 *     RT_ERR_INVALID, output untouched: a NULL required pointer; an output that overlaps any input; width or height <= 0; max_history < 1; previous planes
 *     without previous history or the reverse; a previous frame without `rp`; n_passes outside [1, RT_DENOISE_MAX_PASSES].  Whole frames only. --- */
typedef struct rt_temporal_params {
    int32_t max_history;           /* >= 1: the history length stops growing here (a = 1 / n stops shrinking)      */
    float   alpha_min;             /* the least weight of the current frame; 0 = the running mean up to max_history */
    float   min_normal_dot;        /* N' . N_q at least this                                                        */
    float   max_plane_dist;        /* |N' . (P_q - P')| at most this, in scene units                                */
} rt_temporal_params;
typedef struct rt_motion { float rotation[9]; float translation[3]; } rt_motion;   /* previous = rotation (row-major) current + translation */
typedef struct rt_reproject {
    int32_t          posed;        /* 0: `camera` is the previous camera, 1: `pose` is                              */
    rt_camera        camera;
    rt_camera_pose   pose;
    uint32_t         no_history_mask;
    const rt_motion *motion;       /* RT_MAX_OBJECTS records by object id, or NULL: everything is static            */
} rt_reproject;
typedef struct rt_denoise_var_params {
    int32_t n_passes;              /* 1 .. RT_DENOISE_MAX_PASSES                                                    */
    float   k_normal, k_position, k_albedo, k_sigma, var_floor;
} rt_denoise_var_params;
int rt_temporal_accumulate_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, const void *prev_aov_dev, const void *prev_history_dev, int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, void *out_history_dev, void *stream);
int rt_temporal_accumulate(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, const float *prev_aov_host, const float *prev_history_host, int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, float *out_history_host);
int rt_denoise_var_device(rt_ctx *ctx, const void *history_dev, const void *aov_dev, int width, int height, const rt_denoise_var_params *vp, void *out_rgba_dev, void *stream);
int rt_denoise_var(rt_ctx *ctx, const float *history_host, const float *aov_host, int width, int height, const rt_denoise_var_params *vp, float *out_rgba_host);
typedef struct rt_svgf_params {
    int32_t n_passes;              /* 1 .. RT_DENOISE_MAX_PASSES                                                    */
    int32_t feedback_pass;         /* -1: none; else 0 .. n_passes - 1: this pass's colour goes into out_history    */
    int32_t prefilter;             /* 0 or 1: the 3 x 3 Gaussian of the variance drives the colour term             */
    float   k_normal, k_position, k_albedo, k_sigma, var_floor;
} rt_svgf_params;                  /* 32 bytes */
int rt_svgf_filter_device(rt_ctx *ctx, const void *history_dev, const void *aov_dev, int width, int height, const rt_svgf_params *sp, void *out_rgba_dev, void *out_history_dev, void *stream);
int rt_svgf_filter(rt_ctx *ctx, const float *history_host, const float *aov_host, int width, int height, const rt_svgf_params *sp, float *out_rgba_host, float *out_history_host);

/* --- reprojecting a DEFORMING mesh: vertex snapshots and previous-frame planes (ABI 6, additive).  A motion record is rigid; a mesh that rt_mesh_set_vertices*
 *     reshapes has none.  But a surface point of a mesh is named by (triangle, barycentrics), and where it was a frame ago is the same barycentric combination of
 *     that triangle's PREVIOUS corners.  So the library keeps a mesh's previous vertices, and the call that writes the planes also writes where every pixel's point
 *     and normal were in the previous frame -- two planes in the layout of planes 0 and 1, which rt_temporal_accumulate[_fast]* takes as its `aov` argument with
 *     rp->motion == NULL: that kernel reads the current frame's point and normal from nowhere else, and moves them by nothing.
 *     rt_mesh_snapshot_vertices(keep = 1): the current device positions of the mesh at object_slot (-1: of every mesh with triangles) are copied into a buffer of
 *     the context's with the indexing of the vertices themselves, device to device on the context's own stream, in the order of the call (as
 *     rt_mesh_set_vertices_device's read is ordered); the host does not wait (an rt_render_aov_motion_device issued on ANOTHER stream waits for the copy on
 *     that stream); the object's bit of the snapshot mask is set.  keep = 0 clears the bit: the object
 *     follows the motion table again.  rt_mesh_snapshot_mask reports the bits.  Call it once per frame BEFORE that frame's edits (any number of
 *     rt_mesh_set_vertices* and rt_mesh_transform* calls; neither touches a snapshot).  rt_scene_upload* drops every snapshot; rt_mesh_rebuild* keeps them, in both
 *     modes (a rebuild reorders triangles, not vertices).  A snapshot is nothing a render reads: the caches of a still view and their counters are as they were.
 *     RT_ERR_NO_SCENE: no upload, or the last one failed.  RT_ERR_INVALID, nothing changed: keep outside {0, 1}, a sphere's slot, a slot outside the scene.  A mesh
 *     without triangles: RT_OK, nothing happens.  rt_multi_* contexts have no snapshots.
 *     rt_render_aov_motion*: rays, rows, stream, pipelining and errors as rt_render_aov*; ONE traversal.  out_aov: the three planes of rt_render_aov*, word for
 *     word.  out_prev: two dense planes of n_rows * width float4, consecutive: plane 0 = (N', id), plane 1 = (P', 1); a miss writes (0, 0, 0, -1) and (0, 0, 0, 0).
 *     The arithmetic is the contract -- binary32, one rounding per operation, no contraction, sums left to right.  Per pixel with a hit (id, N, P: what planes 0
 *     and 1 get; (O, u): its camera ray):
 *       a MESH hit on triangle tri (visit order) while bit id of the snapshot mask is set:
 *         (alpha, beta, gamma) exactly as smooth shading and the texture lookup compute them (see textured meshes above), from the CURRENT triangle;
 *         A', B', C' = the snapshot's positions of the triangle's three corners;   P' = (alpha A' + beta B') + gamma C' per component;
 *         N' = N where the mesh shades with interpolated normals (unless it holds a NORMAL snapshot, below; without one min_normal_dot bounds how far a shading
 *         normal may turn in a frame), else N' = normalize(cross(B' - A', C' - A')): bit for bit the normal the previous frame's plane 0 held for this triangle;
 *       otherwise, motion != NULL (RT_MAX_OBJECTS records by object id, copied by the call): rt_temporal_accumulate's expressions with record id,
 *         P' = ((R0 P.x + R1 P.y) + R2 P.z) + T0 (rows 1, 2 likewise), N' = (R0 N.x + R1 N.y) + R2 N.z;
 *       otherwise P' = P, N' = N.
 *       and, whichever of the three decided P': a hit on a mesh that shades with interpolated normals while bit id of the NORMAL-snapshot mask is set gets
 *         N' = normalize((alpha n'_a + beta n'_b) + gamma n'_c), n' = the snapshot's three corner normals of triangle tri: get_smooth_normal's expression with the
 *         barycentrics above -- bit for bit what the previous frame's plane 0 held at this barycentric point of this triangle.  It takes precedence over the
 *         record's rotation of N.
 *     rt_mesh_snapshot_normals(keep = 1) is rt_mesh_snapshot_vertices' twin for the shading normals: the mesh's corner normals as they are NOW (3 float4 per
 *     triangle) are copied into a buffer of the context's, device to device on the context's own stream, the host does not wait, the object's bit of a second mask
 *     is set; on a mesh that shades flat it does nothing and the bit stays clear.  keep = 0 clears the bit; rt_mesh_normal_snapshot_mask reports the bits.  The
 *     copy is indexed by the triangles' position in the tree's visit order, so rt_scene_upload* AND EVERY rt_mesh_rebuild* CLEAR THE WHOLE NORMAL-SNAPSHOT MASK
 *     (the vertex snapshots survive a rebuild as before): snapshot again in the frame after a rebuild.  Nothing a render reads; errors as rt_mesh_snapshot_vertices.
 *     A snapshot takes precedence over the object's motion record.  NON-FINITE: a degenerate previous triangle (two corners equal) gives N' = NaN, which reuses
 *     no history (rt_temporal_accumulate: a NaN in N' rejects every tap); a NaN barycentric gives a NaN P' likewise.
 *     THE RECIPE, per frame:  (1) rt_mesh_snapshot_vertices and, for a smooth mesh, rt_mesh_snapshot_normals;  (2) the frame's edits, for a smooth mesh closed by
 *     rt_mesh_compute_normals* (or rt_mesh_set_normals*);  (3) rt_render*;  (4) rt_render_aov_motion* with the table for the spheres and
 *     the rigid meshes;  (5) rt_temporal_accumulate[_fast]* with aov = THE TWO PREVIOUS-FRAME PLANES, prev_aov = the previous frame's CURRENT planes 0 and 1 and
 *     rp->motion = NULL.  Everything else -- rt_denoise*, rt_svgf_filter*, rt_history_rectify*, rt_demodulate*, rt_upsample*, rt_sample_counts* -- keeps taking
 *     the current planes.
 *     RT_ERR_INVALID, both outputs untouched: everything rt_render_aov* refuses; out_prev NULL; out_prev overlapping out_aov.
 *     Not covered: what a mirror or glass surface shows, rt_render_aov_surface*, rt_multi_*, batches. --- */
int rt_mesh_snapshot_vertices(rt_ctx *ctx, int object_slot, int keep);
int rt_mesh_snapshot_mask(const rt_ctx *ctx, uint32_t *mask);
int rt_mesh_snapshot_normals(rt_ctx *ctx, int object_slot, int keep);
int rt_mesh_normal_snapshot_mask(const rt_ctx *ctx, uint32_t *mask);
int rt_render_aov_motion_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, const rt_motion *motion, void *out_aov_dev, void *out_prev_dev, void *stream);
int rt_render_aov_motion(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, const rt_motion *motion, float *out_aov_host, float *out_prev_host);

/* --- the planes of the first DIFFUSE surface, and filtering irradiance instead of colour (ABI 6, additive).  The specular branches of Scene::getColor
 *     (cpu:573-604) draw no random number -- reflection, total reflection or refraction, no Fresnel coin -- so the chain of the pixel-centre ray from the camera to
 *     its first diffuse surface is a function of the scene alone, the colour is handed through it unchanged, and that surface's albedo factors out of the pixel:
 *     pixel = albedo (.) (l / pi + what follows) (cpu:624, 642-644), as at a diffuse first hit.
 *     rt_render_aov_surface*: rays, rows, stream, pipelining and errors as rt_render_aov*; p->eps and p->tri_tmin are read; sigma, num_rays, num_bounce, seed,
 *     variant and depth_convention are ignored.  Per pixel: (O, u) = the camera ray, refr = 1, k = 0; repeat:
 *       intersect as Scene::intersect_all does (as rt_render_aov*); a miss ends the chain as a MISS;
 *       a hit object that is neither a mirror nor has n_in != n_out ends it DIFFUSE;
 *       otherwise, with k == max_specular, it ends EXHAUSTED, and that specular hit is the one recorded;
 *       otherwise the ray goes on as getColor continues it -- a mirror: O = P + eps N, u = u - (2 (u.N)) N; any other: cpu:580-604 with the ray's index refr
 *       (total reflection, or refraction and refr = n_in or n_out) -- and k = k + 1.
 *     N is the normal getColor shades the hit with for the segment's OWN ray, the albedo the object's or the texture's at the arriving segment's barycentrics.
 *     Output: three planes in the layout of rt_render_aov*, so whatever reads three consecutive planes takes them as they are:
 *       plane 0  .xyz = N of the recorded hit, .w = the PATH CODE, an exact small float: id when k == 0, else id + 16 first_id + 256 k (id: the recorded hit's
 *                object, first_id: the camera ray's first hit; at most 4095); -1 on a miss after any number of segments.  The filters' "same object" test becomes
 *                "same surface seen the same way": a wall seen directly, in the mirror and through the glass sphere carries three codes.  code mod 16 is the
 *                object, floor(code / 256) the chain length;
 *       plane 1  .xyz = the recorded hit point, .w = 1 on a hit, 0 on a miss;
 *       plane 2  .xyz = the recorded hit's albedo, .w = 1 when the chain ended DIFFUSE -- there the albedo factors out of the pixel -- and 0 otherwise.
 *     A miss writes zeros in every .xyz.  max_specular == 0 gives the planes of rt_render_aov* word for word except plane 2 .w.  The call runs max_specular + 1
 *     traversal launches whatever the scene and reads nothing back in between.  max_specular outside [0, RT_MAX_SEGMENTS - 1]: RT_ERR_INVALID, output untouched.
 *     rt_demodulate* / rt_modulate*: a colour frame of n_pixels float4 and three planes of n_pixels float4, of which plane 2 is read.  In binary32, for pixel p
 *     with colour C and A = plane 2:
 *       A.w != 1: out = C (with the planes of rt_render_aov*, whose plane 2 .w is 0, both calls are the identity; nothing is divided by a mirror's black albedo);
 *       otherwise per channel c: d = max(A.c, albedo_floor) (maxNum); d > 0: demodulate gives C.c / d, correctly rounded, modulate gives C.c * d; d not > 0 (zero,
 *       negative or NaN): the channel passes through both ways.  .w passes through.
 *     out == color exactly (in place) is allowed.  RT_ERR_INVALID, output untouched: any other overlap of the output with an input, a NULL pointer, n_pixels <= 0
 *     or >= 2^28.
 *     THE PIPELINE these are for: surface planes -> rt_demodulate -> rt_denoise / rt_denoise_var with the surface planes as the guide and k_albedo = 0 ->
 *     rt_modulate with the same planes and floor.
 *     rt_temporal_accumulate* keeps taking the FIRST-HIT planes of rt_render_aov*: a hit point seen in a mirror does not reproject like a surface point, and
 *     no_history_mask is indexed by object id, not by path code (reprojecting the virtual image is not provided).  The history may be accumulated on demodulated
 *     colour as long as the planes that demodulate a frame are the surface planes of that same frame. --- */
int rt_render_aov_surface_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, int max_specular, void *out_aov_dev, void *stream);
int rt_render_aov_surface(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const rt_rows *rows, int max_specular, float *out_aov_host);
int rt_demodulate_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, int64_t n_pixels, float albedo_floor, void *out_rgba_dev, void *stream);
int rt_demodulate(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, int64_t n_pixels, float albedo_floor, float *out_rgba_host);
int rt_modulate_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, int64_t n_pixels, float albedo_floor, void *out_rgba_dev, void *stream);
int rt_modulate(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, int64_t n_pixels, float albedo_floor, float *out_rgba_host);

/* --- guided upsampling: trace at 1 / f of the resolution, rebuild at full resolution (ABI 6, additive).  A SPEED KNOB, not a quality feature: a quarter (f = 2) or
 *     a sixteenth (f = 4) of the rays for a larger error than the same chain at full resolution (DESIGN.md section 5.11 has both); nothing uses it unless asked.
 *     The noisy colour is traced at w x h = (width / f) x (height / f); the planes of rt_render_aov[_surface]* are taken at both resolutions (the full-resolution
 *     ones cost one traversal round of camera rays and shade nothing).  With the camera's z = -W / (2 tan(fov / 2)) the low-resolution pixel (i, j) looks exactly
 *     through the common corner of its f x f full-resolution pixels: the two sets of planes describe one image plane.
 *     rt_upsample*: width x height is the FULL resolution.  low: n_planes consecutive planes of w x h float4 (1: a colour frame; 2: a history, both planes of
 *     rt_temporal_accumulate*).  low_aov, aov: three-plane buffers as rt_render_aov* writes them at the low and at the full resolution; planes 0 and 1 are read,
 *     plane 2 is not.  out: n_planes planes of width x height float4.  The arithmetic is the contract -- binary32, one rounding per operation, no contraction, sums
 *     left to right, quotients correctly rounded.  Full-resolution pixel p = (x, y) with id_p, N_p, P_p from `aov`:
 *       gx = ((float)x + 0.5f) / (float)f - 0.5f,  ix = floor(gx),  fx = gx - floor(gx);  gy, iy, fy likewise from y;
 *       the taps, in this order: q = (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1); bx = 1 - fx for the left column and fx for the right, by likewise for
 *       the upper and the lower row, b = bx by;
 *       a tap is skipped if it lies outside the w x h image or id_q != id_p (a miss matches a miss); otherwise, with N_q, P_q from `low_aov`,
 *         dn = (N_p.x - N_q.x)^2 + (N_p.y - N_q.y)^2 + (N_p.z - N_q.z)^2 and e = N_p.x (P_q.x - P_p.x) + N_p.y (P_q.y - P_p.y) + N_p.z (P_q.z - P_p.z), dp = e e,
 *         exactly as rt_denoise forms them;  wn = max(0, 1 - dn k_normal), wp = max(0, 1 - dp k_position); a k_* of exactly 0 makes its term exactly 1;
 *         w = b wn wp, multiplied left to right; the tap COUNTS only if w > 0: S_i += w L_q for every plane i and channel, W += w;
 *       if no tap counted (W == 0): the four taps are taken again and every tap inside the image counts with w = b, whatever the guides say -- plain bilinear
 *       (at least one of them has b > 0; one with b == 0, which f = 3 has, still adds 0 L_q and may be the first counted tap);
 *       out = S / W per channel, except plane 0's .w, which is the .w of the first counted tap: a ray count stays exact.
 *     A pixel that is a miss is upsampled like any other, among the misses of its footprint.
 *     NON-FINITE INPUTS: as for the filters above, max is maxNum and comparisons with a NaN are false.  A NaN in N_q or P_q, or an id_q of NaN, makes that tap weigh
 *     nothing; a pixel whose own N_p, P_p or id_p is NaN counts no tap and takes the plain bilinear value.  A non-finite VALUE L_q is summed like a number into every
 *     pixel that counts its tap (Inf - Inf and 0 Inf give NaN) and changes no other pixel.  The sign and payload of a NaN written are not specified.
 *     RT_ERR_INVALID, output untouched: a NULL pointer; factor outside [2, 4]; n_planes outside [1, 2]; width or height <= 0 or no multiple of factor; 2^28
 *     full-resolution pixels or more; an output that overlaps any input (low_aov and aov counted with their three planes).
 *     THE TWO PIPELINES this serves (f = factor; history stays at the low resolution throughout):
 *       A: the whole chain at w x h -- render, planes, rt_temporal_accumulate, rt_svgf_filter -- then rt_upsample with n_planes = 1 on the filtered frame;
 *       B: render, planes and rt_temporal_accumulate at w x h, then rt_upsample with n_planes = 2 on the history, then rt_svgf_filter at full resolution with the
 *          full-resolution planes.  The upsampled history serves that one frame's filter and is never fed back (a fed-back history of B is at full resolution: drop it).
 *     In both, rt_demodulate runs at the low resolution with the low planes BEFORE the upsample and rt_modulate at full resolution with the full planes AFTER it:
 *     irradiance is what is interpolated, and a texture's detail comes back from the full-resolution albedo plane.  That is why the weights have no albedo term. --- */
typedef struct rt_upsample_params {
    int32_t factor;                /* f: 2, 3 or 4                                                                  */
    int32_t n_planes;              /* 1: a colour frame; 2: a history (both planes of rt_temporal_accumulate)       */
    float   k_normal, k_position;
} rt_upsample_params;              /* 16 bytes */
int rt_upsample_device(rt_ctx *ctx, const void *low_dev, const void *low_aov_dev, const void *aov_dev, int width, int height, const rt_upsample_params *up, void *out_dev, void *stream);
int rt_upsample(rt_ctx *ctx, const float *low_host, const float *low_aov_host, const float *aov_host, int width, int height, const rt_upsample_params *up, float *out_host);

/* --- a responsive history: a fast history beside the long one, and the long one clamped to it (ABI 6, additive; history rectification, "anti-lag").  The
 *     accumulation accepts a previous pixel that shows the same object, normal and tangent plane; none of these changes when the LIGHT moves or a moving object drags
 *     its shadow over a wall, so an old shadow lingers for up to max_history frames.  A second history of a few frames follows such a change quickly; where the long
 *     history has left the band the fast one spans in the pixel's neighbourhood it is clamped into it and made as short as the fast one, so that it converges again.
 *     Pure post-processing; rt_temporal_accumulate* and every other entry are unchanged.  DESIGN.md section 5.12 has the measurements and the defaults.
 *     rt_temporal_accumulate_fast*: rt_temporal_accumulate* with an input prev_fast (one plane of width * height float4, given exactly when prev_history is given, NULL
 *     otherwise), an output out_fast (one such plane) and fast_history >= 1.  out_history is word for word what rt_temporal_accumulate* writes for the same inputs.
 *     The fast plane is (Fr, Fg, Fb, n_f).  It takes the SAME tap q the long history took -- one reprojection, not a second search:
 *       tap q accepted (F_q = prev_fast at q):  n_f = min(F_q.w + 1, (float)fast_history),  a_f = max(1 / n_f, alpha_min),  F = F_q.rgb + a_f (C_p.rgb - F_q.rgb);
 *       no tap, the first frame, an object masked by no_history_mask:  F = C_p.rgb, n_f = 1;      a miss:  (C_p.rgb, 0).
 *     Same contract: binary32, one rounding per operation, the quotient correctly rounded, min and max are minNum and maxNum (a NaN F_q.w gives n_f = fast_history).
 *     RT_ERR_INVALID, both outputs untouched: everything rt_temporal_accumulate* refuses; out_fast NULL; prev_fast without prev_history or the reverse;
 *     fast_history < 1; either output overlapping any input (prev_fast among them) or the other output.
 *     rt_history_rectify*: inputs -- the history just written (two planes), the fast plane just written, the current planes (only plane 0, normal | id, is read), the
 *     parameters.  Output: a history (two planes).  Pixel p = (x, y) with id_p = plane 0 .w, H0_p = (H.rgb, rays), H1_p = (m1, m2, n, V), F_p = (F.rgb, n_f):
 *       id_p == -1 (a miss), or H1_p.z <= F_p.w (the long history holds nothing older than the fast one):  a copy, every word.   (A NaN on either side of <=: no copy.)
 *       Otherwise, over the (2 radius + 1)^2 window, dy = -radius .. radius (outer), dx = -radius .. radius (inner), q = (x + dx, y + dy) inside the image with
 *       id_q == id_p -- the pixel itself always counts, whatever its id:
 *         per channel c:  s1_c += F_q.c;   s2_c += F_q.c F_q.c;   cnt += 1;
 *         mu_c = s1_c / cnt;   e2_c = s2_c / cnt;   sg_c = sqrt(max(0, e2_c - mu_c mu_c))   (quotients and root correctly rounded);
 *         lo_c = mu_c - k_clamp sg_c;   hi_c = mu_c + k_clamp sg_c;   H'_c = min(max(H_c, lo_c), hi_c).
 *       If no channel moved (H'_c == H_c for all three):  a copy, every word.
 *       Else:  plane 0 = (H', H0_p.w);   n' = F_p.w;   d = l(H') - l(H)  (l: the luminance of rt_temporal_accumulate);   m1' = m1 + d;
 *              m2' = m2 + (m1' m1' - m1 m1);   plane 1 = (m1', m2', n', V).
 *     A clamped pixel's history is only as long as the fast one, so the next frames blend it at 1 / (n_f + 1) and it converges again; shifting both moments keeps
 *     m2 - m1 m1, the variance the filter reads, where it was.  k_clamp == 0 makes the band the point mu.
 *     NON-FINITE INPUTS, from minNum / maxNum and the comparisons alone (nothing is special-cased): a NaN H_c is replaced by lo_c (a NaN never equals itself: the
 *     pixel counts as moved); a NaN F_q.c in the window makes mu_c, lo_c and hi_c NaN and leaves H_c as it is; a +-Inf F_q.c makes mu_c that Inf and sg_c =
 *     sqrt(max(0, NaN)) = 0, so every pixel whose window holds it is clamped to the Inf; a NaN id_p matches no neighbour and the window is the pixel alone; NaN moments
 *     are shifted like numbers.  The sign and payload of a NaN written are not specified.
 *     out == history EXACTLY (in place) is allowed: a pixel reads and writes its own two records only.  RT_ERR_INVALID, output untouched: a NULL pointer; radius
 *     outside [1, 3]; k_clamp negative or NaN; width or height <= 0 or 2^28 pixels or more; any other overlap of the output with an input.
 *     THE SEQUENCE per frame: rt_temporal_accumulate_fast -> rt_history_rectify in place on the accumulated history -> rt_svgf_filter (or rt_upsample with n_planes = 2
 *     in pipeline B); the rectified history and the fast plane are next frame's prev_history and prev_fast.  A cut passes neither. --- */
typedef struct rt_rectify_params {
    int32_t radius;                /* 1 .. 3: the window is (2 radius + 1)^2 pixels                                 */
    float   k_clamp;               /* >= 0: the band is the mean +- k_clamp standard deviations of the fast colour  */
} rt_rectify_params;               /* 8 bytes */
int rt_temporal_accumulate_fast_device(rt_ctx *ctx, const void *color_rgba_dev, const void *aov_dev, const void *prev_aov_dev, const void *prev_history_dev, const void *prev_fast_dev, int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, int fast_history, void *out_history_dev, void *out_fast_dev, void *stream);
int rt_temporal_accumulate_fast(rt_ctx *ctx, const float *color_rgba_host, const float *aov_host, const float *prev_aov_host, const float *prev_history_host, const float *prev_fast_host, int width, int height, const rt_temporal_params *tp, const rt_reproject *rp, int fast_history, float *out_history_host, float *out_fast_host);
int rt_history_rectify_device(rt_ctx *ctx, const void *history_dev, const void *fast_dev, const void *aov_dev, int width, int height, const rt_rectify_params *rp, void *out_history_dev, void *stream);
int rt_history_rectify(rt_ctx *ctx, const float *history_host, const float *fast_host, const float *aov_host, int width, int height, const rt_rectify_params *rp, float *out_history_host);

/* --- adaptive sampling: per-pixel sample counts, traced as a compacted list (ABI 6, additive).  rt_params.num_rays spends samples uniformly; the denoising chain
 *     knows where a frame is bad (a pixel revealed this frame has n = 1 and a guessed variance).  These entries put samples where a caller, or a history, asks for
 *     them, at the cost of the paths actually traced.  Nothing else reads them; DESIGN.md section 5.13 has the measurements.
 *     rt_render_counts*: counts is width * height bytes, pixel (x, y) at counts[y * width + x]; out (and base) are whole frames of width * height float4.  With
 *     c = counts[y * width + x]: pixel (x, y) of out holds, bit for bit and .w included, what rt_render_device writes there for the same scene and p with
 *     p->num_rays = c -- with a pose, what rt_render_pose_device writes, its inv_n = (float)(1. / c) weighting per pixel.  (Sample s of a pixel does not depend on
 *     num_rays, samples are independent paths, and they are added in sample order.)
 *       With base == NULL a pixel with c == 0 is (0, 0, 0, 0).
 *       p->num_rays is not read.  sigma, depth_convention, num_bounce, eps, tri_tmin and seed are honoured as elsewhere (segments <= 0: black).
 *       Counts above RT_MAX_SAMPLE_COUNT are read as RT_MAX_SAMPLE_COUNT.
 *       With base != NULL the caller promises that base is the whole frame rt_render_device / rt_render_pose_device wrote for this p, pose and scene with
 *       num_rays = 1.  Pixels with c <= 1 are copied from it; pixels with c >= 2 trace only samples 1 .. c - 1 and start their sum from base.  The result is the
 *       same bits as without base: a one-sample frame stores (0 + a0) / 1.  out == base is allowed: each pixel is read and written by one lane.
 *       Whole frames only (no rt_rows).  Variant RT_VARIANT_AUTO or RT_VARIANT_WAVEFRONT_QUEUE (here AUTO always means the work-stack pipeline); any other variant,
 *       or a tree that pipeline cannot take, returns RT_ERR_UNSUPPORTED.  Several meshes, materials, smooth normals, textured meshes and device-transformed or
 *       rebuilt meshes render as in rt_render_device.  Not supported: batches, rt_multi_*, the async slots, progressive accumulation, rt_count_work.
 *       The first-hit cache is neither read, filled nor invalidated: rt_first_hit_cache_counts does not move.
 *       RT_ERR_INVALID, outputs untouched: a NULL ctx, p, counts or out; out overlapping counts; base overlapping out without being out; width or height <= 0;
 *       2^26 pixel slots (8 x 8 tiles x 64) or more; whatever rt_render_device refuses of p.
 *       THE ENTRY WAITS ON THE STREAM ONCE: the pixels' samples are laid out as a list by three small launches (sums per workgroup, a scan of those, the scatter),
 *       and the host reads the list's length back (4 bytes) to size the launch chains.  Everything else is asynchronous on `stream`.  A list longer than one
 *       chain's state may hold (RT_PATH_SAMP_MB, 2^29 paths) is cut into consecutive chains; rt_render_counts_info: of the context's last rt_render_counts* call,
 *       out[0] samples traced, [1] launch chains, [2] pixel slots, [3] paths of the largest chain.
 *     rt_sample_counts*: counts from a history -- elementwise over plane 1 of rt_temporal_accumulate*, (m1, m2, n, V) per pixel (history is the two-plane buffer;
 *     plane 0 is not read).  The arithmetic is the contract: binary32, one rounding per operation, the quotient correctly rounded, min / max are IEEE minNum / maxNum:
 *       n == 0 (a miss):  count = 1
 *       e_n   = (n < (float)short_history) ? (float)(new_surface_samples - 1) : 0
 *       rel   = V / (m1 m1 + lum_floor)
 *       e_v   = floor(k_rel rel), taken as 0 unless it compares >= 1 (so a NaN gives 0)
 *       count = 1 + min((float)(max_samples - 1), max(e_n, e_v))
 *     A NaN n is neither a miss nor short (e_n = 0); an infinite rel asks for max_samples.  RT_ERR_INVALID, counts untouched: max_samples outside
 *     [1, RT_MAX_SAMPLE_COUNT], new_surface_samples outside [1, max_samples], short_history < 0, a NULL pointer, width or height <= 0 or 2^28 pixels or more, counts
 *     overlapping the history.
 *     THE SEQUENCE per frame (SvgfSequence(adaptive=...)): render one sample -> planes -> rt_temporal_accumulate -> rt_sample_counts on the accumulated history ->
 *     rt_render_counts with base = out = the colour frame -> rt_temporal_accumulate again, from the same previous history into the same buffer -> the filter.  The
 *     history blends a 4-sample pixel like a 1-sample one (no per-sample weights).
 *     rt_kat_sample_plan (test interface): the list of `counts` alone, samples [first_sample, c) of every pixel, first_sample 0 or 1.  offs_out (or NULL):
 *     tiles_x * tiles_y * 64 + 1 offsets in pixel-slot order (8 x 8 tiles, row-major tiles, row-major inside a tile); items_out (or NULL): *n_items_out records
 *     (x, y, sample), slot-major then sample -- the caller sizes it from its counts; span_out (or NULL): [0] the pixel slots one workgroup of the scan covers,
 *     [1] the slots one round of the scan of workgroup sums covers. --- */
#define RT_MAX_SAMPLE_COUNT 64
typedef struct rt_sample_count_params {
    int32_t max_samples;           /* 1 .. RT_MAX_SAMPLE_COUNT: no pixel gets more                                  */
    int32_t short_history;         /* a pixel whose history is shorter than this many frames is newly revealed      */
    int32_t new_surface_samples;   /* 1 .. max_samples: what such a pixel gets                                      */
    float   k_rel, lum_floor;      /* extra samples per unit of relative variance V / (m1^2 + lum_floor)            */
    int32_t reserved;
} rt_sample_count_params;          /* 24 bytes */
int rt_render_counts_device(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose /* NULL: the uploaded camera */, const uint8_t *counts_dev, const void *base_rgba_dev /* or NULL */, void *out_rgba_dev, void *stream);
int rt_render_counts(rt_ctx *ctx, const rt_params *p, const rt_camera_pose *pose, const uint8_t *counts_host, const float *base_rgba_host, float *out_rgba_host);
int rt_render_counts_info(const rt_ctx *ctx, uint64_t out[4]);
int rt_sample_counts_device(rt_ctx *ctx, const void *history_dev, int width, int height, const rt_sample_count_params *cp, uint8_t *counts_dev, void *stream);
int rt_sample_counts(rt_ctx *ctx, const float *history_host, int width, int height, const rt_sample_count_params *cp, uint8_t *counts_host);
int rt_kat_sample_plan(rt_ctx *ctx, const uint8_t *counts_host, int width, int height, int first_sample, uint32_t *offs_out, int32_t *items_out, uint64_t *n_items_out, int32_t span_out[2]);

/* --- one host process, several devices (SURVEY 8b rt_render_multi; the reference uses the implicit device 0,
 *     optimized.cu:828-856).  The frame is cut into RT_MULTI_TILE_ROWS-row tiles, tile k -> device k mod n
 *     (interleaved); the scene is replicated; every device renders its tiles; each peer pushes them over
 *     xGMI into the root device (device_ids[0]); one kernel on the root restores row order.  The result is bitwise
 *     the single-device frame.  Device ids may repeat (several contexts on one device).  The one-process-per-GPU
 *     path (rt_render_device + an RCCL gather) is the other way to use several GPUs. ------------- */
#define RT_MAX_DEVICES 16
#define RT_MULTI_TILE_ROWS 8
typedef struct rt_multi rt_multi;
typedef struct rt_multi_stats {
    int32_t  n_devices;
    int32_t  device_id[RT_MAX_DEVICES];
    float    kernel_ms[RT_MAX_DEVICES];   /* HIP-event time of each device's render kernels                  */
    float    gather_ms;                   /* root: end of its own render -> frame assembled (waits for peers) */
    float    frame_ms;                    /* host wall clock of the whole call                                */
    uint64_t rays;                        /* rays traced for the frame (sum of the .w channel)                */
    uint64_t gather_bytes;                /* bytes the peers moved into the root device for the last frame   */
    int32_t  peer_access[RT_MAX_DEVICES]; /* 1: device k writes the root's memory directly (peer access over xGMI),
                                             0: no peer path, the runtime stages the copy; -1: same device as the root */
    float    submit_ms;                   /* host: call entry -> every device's launches, events and peer copy issued (one submit
                                             thread per device; frame_ms - submit_ms is spent waiting for the devices)          */
} rt_multi_stats;
int rt_multi_create(rt_multi **m, const int *device_ids, int n_devices);
int rt_multi_destroy(rt_multi *m);
const char *rt_multi_last_error(const rt_multi *m);   /* m may be NULL: last global error */
int rt_multi_scene_upload(rt_multi *m, const rt_sphere *spheres, int n_spheres, const rt_mesh *mesh,
                          const rt_light *light, const rt_camera *camera);
int rt_multi_scene_upload_meshes(rt_multi *m, const rt_sphere *spheres, int n_spheres, const rt_mesh *meshes, int n_meshes,
                                 const rt_light *light, const rt_camera *camera);   /* as rt_scene_upload_meshes, on every device */
/* full frame, height*width float4, to host memory / to memory of the root device */
int rt_render_multi(rt_multi *m, const rt_params *p, float *out_rgba_host);
int rt_render_multi_device(rt_multi *m, const rt_params *p, void *out_rgba_dev_on_root);
/* the PNG path: every device tonemaps its tiles (cpu:714-716) and the exchange moves the 8-bit image, 3 bytes per pixel
 * instead of 16 (the reference copies its 8-bit image off the device too, optimized.cu:856); height*width*3 bytes, the
 * bytes rt_render_rgb8 gives on one device */
int rt_render_multi_rgb8(rt_multi *m, const rt_params *p, uint8_t *out_rgb8_host);
int rt_multi_get_stats(rt_multi *m, rt_multi_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RAYTRACE_HIP_H */
