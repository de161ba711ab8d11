"""ctypes binding of libraytrace_hip.so (include/raytrace_hip.h).

Plumbing only: the render path is the HIP library.  There is no CPU fallback --
if the shared library is missing or no gfx950 device is visible this module
raises instead of rendering with something else.
"""
import ctypes as C
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_LIB") or os.path.join(HERE, "libraytrace_hip.so")   # RT_LIB: an experimental build (tools/)

RT_OK = 0
VARIANT_AUTO, VARIANT_GLOBAL, VARIANT_LDS_VERTS, VARIANT_LDS_TOP, VARIANT_LDS_ALL, VARIANT_LOCKSTEP, VARIANT_WAVEFRONT, VARIANT_WAVEFRONT_LDS, VARIANT_WAVEFRONT_QUEUE, VARIANT_PATH = range(10)
VARIANTS = {"auto": 0, "global": 1, "lds_verts": 2, "lds_top": 3, "lds_all": 4, "lockstep": 5, "wavefront": 6, "wavefront_lds": 7, "wavefront_queue": 8, "path": 9}

# every symbol include/raytrace_hip.h declares (tests check the .so exports each)
EXPORTS = ["rt_abi_version", "rt_device_count", "rt_ctx_create", "rt_ctx_destroy", "rt_last_error",
           "rt_device_name", "rt_scene_upload", "rt_scene_upload_meshes", "rt_render", "rt_render_device", "rt_render_device_batch", "rt_tonemap_device",
           "rt_render_rgb8", "rt_synchronize", "rt_get_stats", "rt_ctx_selfcheck", "rt_count_work",
           "rt_mesh_transform", "rt_mesh_set_normals", "rt_camera_basis", "rt_render_pose", "rt_render_pose_device", "rt_progressive_reset", "rt_progressive_frame",
           "rt_progressive_frames",
           "rt_multi_create", "rt_multi_destroy", "rt_multi_last_error", "rt_multi_scene_upload", "rt_multi_scene_upload_meshes", "rt_render_multi",
           "rt_render_multi_device", "rt_render_multi_rgb8", "rt_multi_get_stats",
           "rt_stats_enable", "rt_ctx_set_pipelining", "rt_render_async", "rt_wait", "rt_trace_rays", "rt_mesh_rebuild", "rt_mesh_rebuild_mode", "rt_mesh_build_stats", "rt_host_alloc", "rt_host_free", "rt_device_alloc", "rt_device_free", "rt_device_to_host", "rt_kat_sphere", "rt_kat_sqrt", "rt_kat_box", "rt_kat_triangle", "rt_kat_mesh", "rt_kat_layout_hash",
           "rt_mesh_transform_of", "rt_mesh_set_normals_of", "rt_mesh_rebuild_of", "rt_mesh_set_texture", "rt_mesh_set_texture_of", "rt_kat_surface",
           "rt_scene_get_light", "rt_scene_set_light", "rt_scene_get_sphere", "rt_scene_set_sphere", "rt_scene_move_light", "rt_scene_move_sphere", "rt_light_orbit",
           "rt_render_device_batch_scenes",
           "rt_render_aov_device", "rt_render_aov", "rt_denoise_device", "rt_denoise",
           "rt_temporal_accumulate_device", "rt_temporal_accumulate", "rt_denoise_var_device", "rt_denoise_var",
           "rt_svgf_filter_device", "rt_svgf_filter",
           "rt_render_aov_surface_device", "rt_render_aov_surface", "rt_demodulate_device", "rt_demodulate", "rt_modulate_device", "rt_modulate",
           "rt_upsample_device", "rt_upsample",
           "rt_temporal_accumulate_fast_device", "rt_temporal_accumulate_fast", "rt_history_rectify_device", "rt_history_rectify",
           "rt_dead_channel_counts", "rt_first_hit_cache_counts", "rt_first_shadow_cache_counts", "rt_first_shade_cache_counts",
           "rt_render_counts_device", "rt_render_counts", "rt_render_counts_info", "rt_sample_counts_device", "rt_sample_counts", "rt_kat_sample_plan",
           "rt_mesh_set_vertices", "rt_mesh_set_vertices_of", "rt_mesh_set_vertices_device",
           "rt_mesh_snapshot_vertices", "rt_mesh_snapshot_mask", "rt_render_aov_motion_device", "rt_render_aov_motion",
           "rt_mesh_compute_normals", "rt_mesh_compute_normals_of", "rt_mesh_get_vertex_normals", "rt_mesh_snapshot_normals", "rt_mesh_normal_snapshot_mask",
           "rt_scene_set_lights", "rt_scene_get_lights", "rt_scene_set_light_at", "rt_scene_move_light_at",
           "rt_scene_set_light_radii", "rt_scene_get_light_radii", "rt_scene_set_light_radius_at",
           "rt_camera_set_lens", "rt_camera_get_lens", "rt_scene_set_shutter", "rt_scene_get_shutter",
           "rt_scene_set_environment", "rt_scene_get_environment", "rt_kat_environment",
           "rt_scene_set_environment_sampling", "rt_scene_get_environment_sampling", "rt_kat_environment_table", "rt_kat_environment_sample",
           "rt_scene_set_emission", "rt_scene_get_emission", "rt_scene_set_emission_sampling", "rt_scene_get_emission_sampling",
           "rt_kat_emission_table", "rt_kat_emission_sample",
           "rt_material_set_fresnel", "rt_material_get_fresnel", "rt_kat_fresnel", "rt_dead_last_count",
           "rt_material_set_roughness", "rt_material_get_roughness", "rt_kat_gloss",
           "rt_kat_progressive", "rt_material_set_tint", "rt_material_get_tint"]
MAX_OBJECTS = 16
MAX_LIGHTS = 16
MAX_DEVICES = 16


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libraytrace_hip: status {code}: {msg}")
        self.code = code


class Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("albedo", C.c_float * 3), ("mirror", C.c_int32),
                ("in_refraction_index", C.c_float), ("out_refraction_index", C.c_float)]


class Mesh(C.Structure):
    _fields_ = [("vertices", C.POINTER(C.c_float)), ("n_vertices", C.c_int32),
                ("indices", C.POINTER(C.c_int32)), ("index_stride", C.c_int32), ("n_triangles", C.c_int32),
                ("bvh_arr10", C.POINTER(C.c_float)), ("n_nodes", C.c_int32),
                ("albedo", C.c_float * 3), ("object_slot", C.c_int32),
                ("mirror", C.c_int32), ("in_refraction_index", C.c_float), ("out_refraction_index", C.c_float)]   # ABI 6: Geometry's other fields (cpu:113-116)


class Light(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("intensity", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("fov", C.c_float)]


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_rays", C.c_int32), ("num_bounce", C.c_int32),
                ("depth_convention", C.c_int32), ("sigma", C.c_float), ("eps", C.c_float), ("tri_tmin", C.c_float),
                ("seed", C.c_uint32), ("variant", C.c_int32)]


class Rows(C.Structure):
    _fields_ = [("row0", C.c_int32), ("n_rows", C.c_int32), ("tile_rows", C.c_int32), ("tile_step", C.c_int32)]


class FrameDesc(C.Structure):
    _fields_ = [("camera", Camera), ("seed", C.c_uint32), ("reserved", C.c_uint32), ("out_rgba_dev", C.c_void_p)]


MAX_BATCH = 16
MAX_SPHERES = 16


class SpherePose(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float)]


class Shutter(C.Structure):
    """what the light and every object slot travel over one frame's exposure (rt_shutter)"""
    _fields_ = [("light", C.c_float * 3), ("object", (C.c_float * 3) * MAX_OBJECTS)]


class FrameScene(C.Structure):
    """what differs from the uploaded scene in one frame of an animated batch (rt_frame_scene)"""
    _fields_ = [("light", Light), ("spheres", SpherePose * MAX_SPHERES)]


class Work(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("box_tests", C.c_uint64), ("nodes", C.c_uint64), ("tri_tests", C.c_uint64),
                ("box_literal", C.c_uint64), ("tri_literal", C.c_uint64), ("steps", C.c_uint64 * 12)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("tonemap_ms", C.c_float), ("pixels", C.c_uint64), ("variant", C.c_int32),
                ("lds_bytes", C.c_int32), ("block_threads", C.c_int32), ("grid_blocks", C.c_int32),
                ("trav_ms", C.c_float), ("trav_launches", C.c_int32), ("parts", C.c_int32), ("adv_launches", C.c_int32),
                ("adv_ms", C.c_float), ("adv_paths", C.c_int32), ("travq_mode", C.c_int32), ("reserved", C.c_int32)]


class BuildStats(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_triangles", C.c_int32), ("n_nodes", C.c_int32), ("n_leaves", C.c_int32), ("max_leaf_tris", C.c_int32),
                ("max_depth", C.c_int32), ("device_build_ms", C.c_float), ("install_ms", C.c_float), ("install_on_device", C.c_int32), ("reserved", C.c_int32)]


BVH_MODES = {"reference": 0, "lbvh": 1}


class Texture(C.Structure):
    _fields_ = [("texels", C.POINTER(C.c_uint8)), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("filter", C.c_int32), ("wrap", C.c_int32), ("decode", C.POINTER(C.c_float))]


TEX_FILTERS = {"nearest": 0, "bilinear": 1}
TEX_WRAPS = {"repeat": 0, "clamp": 1}


class KatCounts(C.Structure):
    _fields_ = [("n", C.c_uint64), ("box_decided", C.c_uint64), ("box_literal", C.c_uint64), ("tri_decided", C.c_uint64), ("tri_literal", C.c_uint64)]


class CameraPose(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("yaw", C.c_float), ("pitch", C.c_float), ("fov", C.c_float)]


class DenoiseParams(C.Structure):
    _fields_ = [("n_passes", C.c_int32), ("k_normal", C.c_float), ("k_position", C.c_float), ("k_albedo", C.c_float), ("k_color", C.c_float)]


# The defaults of make_denoise_params: chosen by the experiment of DESIGN.md section 5.7 (RMSE of a 1-sample frame against a 1024-sample one, cat and sphere scenes).
# k_color weighs squared differences of LINEAR colour, so it scales with 1 / light intensity^2: 5e-12 suits the reference's light (3e10, colours up to ~1e6).
DENOISE_DEFAULTS = dict(n_passes=3, k_normal=2.0, k_position=0.25, k_albedo=16.0, k_color=5e-12)


def _filled(params, defaults, **given):
    """params with every given field set: to its value, or to defaults[name] where that is None"""
    for name, v in given.items():
        setattr(params, name, defaults[name] if v is None else v)
    return params


def make_denoise_params(n_passes=None, k_normal=None, k_position=None, k_albedo=None, k_color=None):
    """rt_denoise_params; None = the default of DENOISE_DEFAULTS.  A k of 0 switches its term off."""
    return _filled(DenoiseParams(), DENOISE_DEFAULTS, n_passes=n_passes, k_normal=k_normal, k_position=k_position, k_albedo=k_albedo, k_color=k_color)


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_int32), ("alpha_min", C.c_float), ("min_normal_dot", C.c_float), ("max_plane_dist", C.c_float)]


class Motion(C.Structure):
    _fields_ = [("rotation", C.c_float * 9), ("translation", C.c_float * 3)]


class Reproject(C.Structure):
    _fields_ = [("posed", C.c_int32), ("camera", Camera), ("pose", CameraPose), ("no_history_mask", C.c_uint32), ("motion", C.POINTER(Motion))]


class DenoiseVarParams(C.Structure):
    _fields_ = [("n_passes", C.c_int32), ("k_normal", C.c_float), ("k_position", C.c_float), ("k_albedo", C.c_float), ("k_sigma", C.c_float), ("var_floor", C.c_float)]


# The defaults of make_temporal_params / make_denoise_var_params.  max_history 32 with alpha_min 0: the running mean of up to 32 frames;
# min_normal_dot 0.9 and max_plane_dist 0.5 scene units: the tolerances of rt_denoise's own normal and plane terms (weight 0 at |dN|^2 = 0.5, at 2 units), tightened
# because a wrong reuse stays in the history.  k_sigma has no unit (the tolerance in units of the pixel's own variance); var_floor 0: nothing tied to the light.
TEMPORAL_DEFAULTS = dict(max_history=32, alpha_min=0.0, min_normal_dot=0.9, max_plane_dist=0.5)
DENOISE_VAR_DEFAULTS = dict(n_passes=3, k_normal=2.0, k_position=0.25, k_albedo=16.0, k_sigma=16.0, var_floor=0.0)


def make_temporal_params(max_history=None, alpha_min=None, min_normal_dot=None, max_plane_dist=None):
    """rt_temporal_params; None = the default of TEMPORAL_DEFAULTS."""
    given = dict(max_history=max_history, alpha_min=alpha_min, min_normal_dot=min_normal_dot, max_plane_dist=max_plane_dist)
    t = TemporalParams()
    for name, v in given.items():
        setattr(t, name, TEMPORAL_DEFAULTS[name] if v is None else v)
    return t


def make_denoise_var_params(n_passes=None, k_normal=None, k_position=None, k_albedo=None, k_sigma=None, var_floor=None):
    """rt_denoise_var_params; None = the default of DENOISE_VAR_DEFAULTS.  A k_normal / k_position / k_albedo of 0 switches its term off."""
    return _filled(DenoiseVarParams(), DENOISE_VAR_DEFAULTS, n_passes=n_passes, k_normal=k_normal, k_position=k_position, k_albedo=k_albedo, k_sigma=k_sigma,
                   var_floor=var_floor)


class SvgfParams(C.Structure):
    _fields_ = [("n_passes", C.c_int32), ("feedback_pass", C.c_int32), ("prefilter", C.c_int32),
                ("k_normal", C.c_float), ("k_position", C.c_float), ("k_albedo", C.c_float), ("k_sigma", C.c_float), ("var_floor", C.c_float)]


# The defaults of make_svgf_params: rt_denoise_var's weights, and the two switches as the table of DESIGN.md section 5.10 decided them -- the pre-filter alone had the
# least error on all three sequences; feeding pass 0 back gained on the baseline on two of them, on the pre-filter alone on none, and lost on the sphere scene.
SVGF_DEFAULTS = dict(DENOISE_VAR_DEFAULTS, feedback_pass=-1, prefilter=1)


def make_svgf_params(n_passes=None, feedback_pass=None, prefilter=None, k_normal=None, k_position=None, k_albedo=None, k_sigma=None, var_floor=None):
    """rt_svgf_params; None = the default of SVGF_DEFAULTS.  feedback_pass -1 = no history is written; prefilter 0 / 1."""
    return _filled(SvgfParams(), SVGF_DEFAULTS, n_passes=n_passes, feedback_pass=feedback_pass, prefilter=prefilter, k_normal=k_normal, k_position=k_position,
                   k_albedo=k_albedo, k_sigma=k_sigma, var_floor=var_floor)


class UpsampleParams(C.Structure):
    _fields_ = [("factor", C.c_int32), ("n_planes", C.c_int32), ("k_normal", C.c_float), ("k_position", C.c_float)]


# The defaults of make_upsample_params: the filters' own normal and plane tolerances (DESIGN.md section 5.11 measured the guided upsample with them).
UPSAMPLE_DEFAULTS = dict(k_normal=DENOISE_VAR_DEFAULTS["k_normal"], k_position=DENOISE_VAR_DEFAULTS["k_position"])


def make_upsample_params(factor, n_planes=1, k_normal=None, k_position=None):
    """rt_upsample_params: factor 2 .. 4, n_planes 1 (a colour frame) or 2 (a history); None = the default of UPSAMPLE_DEFAULTS.  A k of 0 switches its term off."""
    u = UpsampleParams(int(factor), int(n_planes))
    return _filled(u, UPSAMPLE_DEFAULTS, k_normal=k_normal, k_position=k_position)


class RectifyParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("k_clamp", C.c_float)]


# The defaults of make_rectify_params and of SvgfSequence's fast_history: the row of the scan of DESIGN.md section 5.12 with the least error on the moving-light
# sequence after the light starts to move, among those that lose least on the two static sequences.
RECTIFY_DEFAULTS = dict(radius=1, k_clamp=1.0)
FAST_HISTORY_DEFAULT = 4


def make_rectify_params(radius=None, k_clamp=None):
    """rt_rectify_params: the window is (2 radius + 1)^2 pixels, radius 1 .. 3; the band is the fast history's mean +- k_clamp standard deviations over it, k_clamp >= 0;
    None = the default of RECTIFY_DEFAULTS."""
    return _filled(RectifyParams(), RECTIFY_DEFAULTS, radius=radius, k_clamp=k_clamp)


class SampleCountParams(C.Structure):
    _fields_ = [("max_samples", C.c_int32), ("short_history", C.c_int32), ("new_surface_samples", C.c_int32), ("k_rel", C.c_float), ("lum_floor", C.c_float),
                ("reserved", C.c_int32)]


MAX_SAMPLE_COUNT = 64
# The defaults of make_sample_count_params: the row of the table of DESIGN.md section 5.13 chosen there.
SAMPLE_COUNT_DEFAULTS = dict(max_samples=4, short_history=2, new_surface_samples=4, k_rel=0.0, lum_floor=1e-4)


def make_sample_count_params(max_samples=None, short_history=None, new_surface_samples=None, k_rel=None, lum_floor=None):
    """rt_sample_count_params: a pixel whose history is shorter than short_history frames gets new_surface_samples samples, any other 1 + floor(k_rel V / (m1^2 +
    lum_floor)), none more than max_samples (1 .. MAX_SAMPLE_COUNT); None = the default of SAMPLE_COUNT_DEFAULTS."""
    return _filled(SampleCountParams(), SAMPLE_COUNT_DEFAULTS, max_samples=max_samples, short_history=short_history, new_surface_samples=new_surface_samples,
                   k_rel=k_rel, lum_floor=lum_floor)


def static_motion():
    """[MAX_OBJECTS, 12] float32: the motion table in which nothing moved (rotation = identity, translation = 0); row i = object i's rotation[9] | translation[3]."""
    m = np.zeros((MAX_OBJECTS, 12), np.float32)
    m[:, 0] = m[:, 4] = m[:, 8] = 1
    return m


def motion_from_spheres(previous, current, motion=None):
    """The motion table of spheres that were translated between two frames: previous / current = the spheres of the two frames in object order (tuples as
    scene_upload takes them, or bare centres); translation = previous centre - current centre, in binary32.  motion: a table to fill in (default: static_motion())."""
    m = static_motion() if motion is None else motion
    if len(previous) != len(current) or len(current) > MAX_OBJECTS:
        raise RtError(-1, "motion_from_spheres: two lists of the same spheres, at most %d" % MAX_OBJECTS)
    centre = lambda s: np.asarray(s[0] if np.ndim(s[0]) else s, np.float32)
    for i, (a, b) in enumerate(zip(previous, current)):
        m[i, 9:] = centre(a) - centre(b)
    return m


def motion_from_mesh_transform(rotation, translation, object_slot, motion=None):
    """The motion record of the mesh at object_slot after mesh_transform(rotation, translation, object_slot) (v' = R v + T): its inverse, v = R^T v' - R^T T, with
    R^T T formed in binary32 as (R0 T.x + R3 T.y) + R6 T.z.  motion: a table to fill in (default: static_motion())."""
    m = static_motion() if motion is None else motion
    r = np.ascontiguousarray(rotation, np.float32).reshape(3, 3)
    t = np.ascontiguousarray(translation, np.float32).reshape(3)
    rt_ = np.ascontiguousarray(r.T)
    m[object_slot, :9] = rt_.reshape(9)
    m[object_slot, 9:] = -((rt_[:, 0] * t[0] + rt_[:, 1] * t[1]) + rt_[:, 2] * t[2])
    return m


def make_reproject(camera=None, pose=None, motion=None, no_history_mask=0):
    """rt_reproject: the previous frame's camera -- pose (a CameraPose) if given, else camera = (position, fov), None = the default camera of scene_upload -- the
    motion table ([MAX_OBJECTS, 12] as static_motion() lays it out, None = everything static) and the mask of objects that never reuse history.  The record keeps the table alive."""
    r = Reproject()
    if pose is not None:
        r.posed = 1
        r.pose = pose
    else:
        pos, fov = camera if camera is not None else ((0.0, 0.0, 55.0), None)
        r.camera.position[:] = pos
        r.camera.fov = np.float32(np.pi / 3) if fov is None else fov
    r.no_history_mask = int(no_history_mask)
    if motion is not None:
        m = np.ascontiguousarray(motion, np.float32)
        if m.shape != (MAX_OBJECTS, 12):
            raise RtError(-1, f"make_reproject: motion {m.shape} must be [{MAX_OBJECTS}, 12]")
        r._table = m
        r.motion = m.ctypes.data_as(C.POINTER(Motion))
    return r


def make_pose(position=(0.0, 0.0, 55.0), yaw=0.0, pitch=0.3, fov=None):
    """Camera() of realtime_render.cu:805-810 (C = (0,0,55), yaw 0, pitch 0.3); Scene::pov = PI / 2 (realtime:1021)."""
    q = CameraPose()
    q.position[:] = position
    q.yaw, q.pitch = yaw, pitch
    q.fov = np.float32(np.pi / 2) if fov is None else np.float32(fov)
    return q


class MultiStats(C.Structure):
    _fields_ = [("n_devices", C.c_int32), ("device_id", C.c_int32 * MAX_DEVICES), ("kernel_ms", C.c_float * MAX_DEVICES),
                ("gather_ms", C.c_float), ("frame_ms", C.c_float), ("rays", C.c_uint64), ("gather_bytes", C.c_uint64),
                ("peer_access", C.c_int32 * MAX_DEVICES), ("submit_ms", C.c_float)]


_lib = None


def load():
    """Load libraytrace_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and
    # its libraries ask for it as "libamdhip64.so", so a system copy loaded first is NOT reused and the second
    # runtime then finds no GPU.  Loading torch first makes this library's NEEDED libamdhip64.so.7 resolve to
    # the copy torch already mapped.  (The C++ launcher, which has no torch, uses /opt/rocm's.)
    if os.environ.get("RT_WITHOUT_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    if os.environ.get("RT_LIB"):      # an experimental / older build may lack the newest entry points: give them inert stand-ins
        class _Missing:
            argtypes = restype = None

        class _MissingCounter(_Missing):      # an entry that only reads counters (rt_*_count[s]): RT_OK and nothing written, the caller's zeros stand
            def __call__(self, *args):
                return 0
        for name in EXPORTS:
            if not hasattr(L, name):
                setattr(L, name, _MissingCounter() if name.endswith(("_count", "_counts")) else _Missing())
    vp = C.c_void_p
    L.rt_abi_version.restype = C.c_int
    L.rt_device_count.argtypes = [C.POINTER(C.c_int)]
    L.rt_ctx_create.argtypes = [C.POINTER(vp), C.c_int]
    L.rt_ctx_destroy.argtypes = [vp]
    L.rt_last_error.argtypes = [vp]
    L.rt_last_error.restype = C.c_char_p
    L.rt_device_name.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rt_scene_upload.argtypes = [vp, C.POINTER(Sphere), C.c_int, C.POINTER(Mesh), C.POINTER(Light), C.POINTER(Camera)]
    L.rt_scene_upload_meshes.argtypes = [vp, C.POINTER(Sphere), C.c_int, C.POINTER(Mesh), C.c_int, C.POINTER(Light), C.POINTER(Camera)]
    L.rt_render.argtypes = [vp, C.POINTER(Params), C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.rt_render_device.argtypes = [vp, C.POINTER(Params), C.POINTER(Rows), vp, vp]
    L.rt_render_device_batch.argtypes = [vp, C.POINTER(Params), C.POINTER(Rows), C.POINTER(FrameDesc), C.c_int, vp]
    L.rt_tonemap_device.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.rt_render_rgb8.argtypes = [vp, C.POINTER(Params), C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    L.rt_count_work.argtypes = [vp, C.POINTER(Params), C.c_int, C.c_int, C.POINTER(Work)]
    L.rt_dead_channel_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rt_dead_last_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    for n in ("rt_first_hit_cache_counts", "rt_first_shadow_cache_counts", "rt_first_shade_cache_counts"):
        getattr(L, n).argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rt_synchronize.argtypes = [vp]
    L.rt_ctx_selfcheck.argtypes = [vp]
    L.rt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.rt_stats_enable.argtypes = [vp, C.c_int]
    L.rt_ctx_set_pipelining.argtypes = [vp, C.c_int]
    L.rt_render_async.argtypes = [vp, C.POINTER(Params), C.c_int, vp, C.c_int]
    L.rt_wait.argtypes = [vp, C.c_int]
    L.rt_trace_rays.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_int, C.POINTER(C.c_float)]
    fp3 = C.POINTER(C.c_float)
    L.rt_mesh_transform.argtypes = [vp, fp3, fp3]
    L.rt_mesh_set_normals.argtypes = [vp, fp3, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int]
    L.rt_camera_basis.argtypes = [C.POINTER(CameraPose), fp3, fp3, fp3]
    L.rt_render_pose.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), fp3]
    L.rt_render_pose_device.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), vp, vp]
    L.rt_progressive_reset.argtypes = [vp]
    L.rt_progressive_frame.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), fp3, C.POINTER(C.c_uint8)]
    L.rt_progressive_frames.argtypes = [vp, C.POINTER(C.c_int)]
    L.rt_multi_create.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
    L.rt_multi_destroy.argtypes = [vp]
    L.rt_multi_last_error.argtypes = [vp]
    L.rt_multi_last_error.restype = C.c_char_p
    L.rt_multi_scene_upload.argtypes = [vp, C.POINTER(Sphere), C.c_int, C.POINTER(Mesh), C.POINTER(Light), C.POINTER(Camera)]
    L.rt_multi_scene_upload_meshes.argtypes = [vp, C.POINTER(Sphere), C.c_int, C.POINTER(Mesh), C.c_int, C.POINTER(Light), C.POINTER(Camera)]
    L.rt_render_multi.argtypes = [vp, C.POINTER(Params), C.POINTER(C.c_float)]
    L.rt_render_multi_device.argtypes = [vp, C.POINTER(Params), vp]
    L.rt_render_multi_rgb8.argtypes = [vp, C.POINTER(Params), C.POINTER(C.c_uint8)]
    L.rt_multi_get_stats.argtypes = [vp, C.POINTER(MultiStats)]
    L.rt_mesh_rebuild.argtypes = [vp, fp3, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rt_mesh_rebuild_mode.argtypes = [vp, C.c_int, fp3, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rt_mesh_build_stats.argtypes = [vp, C.POINTER(BuildStats)]
    L.rt_mesh_transform_of.argtypes = [vp, C.c_int, fp3, fp3]
    L.rt_mesh_set_normals_of.argtypes = [vp, C.c_int, fp3, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int]
    L.rt_mesh_rebuild_of.argtypes = [vp, C.c_int, C.c_int, fp3, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rt_mesh_set_vertices.argtypes = [vp, fp3, C.c_int]
    L.rt_mesh_set_vertices_of.argtypes = [vp, C.c_int, fp3, C.c_int]
    L.rt_mesh_set_vertices_device.argtypes = [vp, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.rt_mesh_snapshot_vertices.argtypes = [vp, C.c_int, C.c_int]
    L.rt_mesh_snapshot_mask.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rt_mesh_compute_normals.argtypes = [vp]
    L.rt_mesh_compute_normals_of.argtypes = [vp, C.c_int]
    L.rt_mesh_get_vertex_normals.argtypes = [vp, C.c_int, fp3, C.c_int]
    L.rt_mesh_snapshot_normals.argtypes = [vp, C.c_int, C.c_int]
    L.rt_mesh_normal_snapshot_mask.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rt_mesh_set_texture.argtypes = [vp, fp3, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(Texture)]
    L.rt_mesh_set_texture_of.argtypes = [vp, C.c_int, fp3, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(Texture)]
    L.rt_kat_surface.argtypes = [vp, fp3, C.c_int, C.c_float, fp3]
    L.rt_scene_get_light.argtypes = [vp, C.POINTER(Light)]
    L.rt_scene_set_light.argtypes = [vp, C.POINTER(Light)]
    L.rt_scene_get_sphere.argtypes = [vp, C.c_int, C.POINTER(Sphere)]
    L.rt_scene_set_sphere.argtypes = [vp, C.c_int, C.POINTER(Sphere)]
    L.rt_scene_move_light.argtypes = [vp, C.c_float, C.c_float]
    L.rt_scene_move_sphere.argtypes = [vp, C.c_int, fp3, C.c_float]
    L.rt_light_orbit.argtypes = [C.POINTER(Light), C.c_float, C.c_float, C.POINTER(Light)]
    L.rt_scene_set_lights.argtypes = [vp, C.POINTER(Light), C.c_int]
    L.rt_scene_get_lights.argtypes = [vp, C.POINTER(Light), C.c_int, C.POINTER(C.c_int)]
    L.rt_scene_set_light_at.argtypes = [vp, C.c_int, C.POINTER(Light)]
    L.rt_scene_move_light_at.argtypes = [vp, C.c_int, C.c_float, C.c_float]
    L.rt_scene_set_light_radii.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    L.rt_scene_get_light_radii.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.rt_scene_set_light_radius_at.argtypes = [vp, C.c_int, C.c_float]
    L.rt_camera_set_lens.argtypes = [vp, C.c_float, C.c_float]
    L.rt_camera_get_lens.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rt_scene_set_shutter.argtypes = [vp, C.POINTER(Shutter)]
    L.rt_scene_get_shutter.argtypes = [vp, C.POINTER(Shutter)]
    L.rt_scene_set_environment.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.rt_scene_get_environment.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.rt_kat_environment.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rt_scene_set_environment_sampling.argtypes = [vp, C.c_float]
    L.rt_scene_get_environment_sampling.argtypes = [vp, C.POINTER(C.c_float)]
    L.rt_kat_environment_table.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rt_kat_environment_sample.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rt_scene_set_emission.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.rt_scene_get_emission.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.rt_scene_set_emission_sampling.argtypes = [vp, C.c_float]
    L.rt_scene_get_emission_sampling.argtypes = [vp, C.POINTER(C.c_float)]
    L.rt_kat_emission_table.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    L.rt_kat_emission_sample.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.rt_material_set_fresnel.argtypes = [vp, C.c_int, C.c_int]
    L.rt_material_get_fresnel.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.rt_kat_fresnel.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rt_material_set_roughness.argtypes = [vp, C.c_int, C.c_float]
    L.rt_material_get_roughness.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.rt_kat_gloss.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rt_material_set_tint.argtypes = [vp, C.c_int, C.c_int]
    L.rt_material_get_tint.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.rt_kat_progressive.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    L.rt_render_device_batch_scenes.argtypes = [vp, C.POINTER(Params), C.POINTER(Rows), C.POINTER(FrameDesc), C.POINTER(FrameScene), C.c_int, C.c_int, vp]
    L.rt_render_aov_device.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), vp, vp]
    L.rt_render_aov.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), fp3]
    L.rt_render_aov_motion_device.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), C.POINTER(Motion), vp, vp, vp]
    L.rt_render_aov_motion.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), C.POINTER(Motion), fp3, fp3]
    L.rt_denoise_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(DenoiseParams), vp, vp]
    L.rt_denoise.argtypes = [vp, fp3, fp3, C.c_int, C.c_int, C.POINTER(DenoiseParams), fp3]
    L.rt_temporal_accumulate_device.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(TemporalParams), C.POINTER(Reproject), vp, vp]
    L.rt_temporal_accumulate.argtypes = [vp, fp3, fp3, fp3, fp3, C.c_int, C.c_int, C.POINTER(TemporalParams), C.POINTER(Reproject), fp3]
    L.rt_denoise_var_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(DenoiseVarParams), vp, vp]
    L.rt_denoise_var.argtypes = [vp, fp3, fp3, C.c_int, C.c_int, C.POINTER(DenoiseVarParams), fp3]
    L.rt_svgf_filter_device.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(SvgfParams), vp, vp, vp]
    L.rt_svgf_filter.argtypes = [vp, fp3, fp3, C.c_int, C.c_int, C.POINTER(SvgfParams), fp3, fp3]
    L.rt_render_aov_surface_device.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), C.c_int, vp, vp]
    L.rt_render_aov_surface.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), C.POINTER(Rows), C.c_int, fp3]
    L.rt_demodulate_device.argtypes = [vp, vp, vp, C.c_int64, C.c_float, vp, vp]
    L.rt_demodulate.argtypes = [vp, fp3, fp3, C.c_int64, C.c_float, fp3]
    L.rt_modulate_device.argtypes = [vp, vp, vp, C.c_int64, C.c_float, vp, vp]
    L.rt_modulate.argtypes = [vp, fp3, fp3, C.c_int64, C.c_float, fp3]
    L.rt_upsample_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(UpsampleParams), vp, vp]
    L.rt_upsample.argtypes = [vp, fp3, fp3, fp3, C.c_int, C.c_int, C.POINTER(UpsampleParams), fp3]
    L.rt_temporal_accumulate_fast_device.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(TemporalParams), C.POINTER(Reproject), C.c_int, vp, vp, vp]
    L.rt_temporal_accumulate_fast.argtypes = [vp, fp3, fp3, fp3, fp3, fp3, C.c_int, C.c_int, C.POINTER(TemporalParams), C.POINTER(Reproject), C.c_int, fp3, fp3]
    L.rt_history_rectify_device.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(RectifyParams), vp, vp]
    L.rt_history_rectify.argtypes = [vp, fp3, fp3, fp3, C.c_int, C.c_int, C.POINTER(RectifyParams), fp3]
    u8p = C.POINTER(C.c_uint8)
    L.rt_render_counts_device.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), vp, vp, vp, vp]
    L.rt_render_counts.argtypes = [vp, C.POINTER(Params), C.POINTER(CameraPose), u8p, fp3, fp3]
    L.rt_render_counts_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rt_sample_counts_device.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(SampleCountParams), vp, vp]
    L.rt_sample_counts.argtypes = [vp, fp3, C.c_int, C.c_int, C.POINTER(SampleCountParams), u8p]
    L.rt_kat_sample_plan.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    L.rt_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.rt_device_alloc.argtypes = [vp, C.POINTER(vp), C.c_size_t]
    L.rt_device_free.argtypes = [vp]
    L.rt_device_to_host.argtypes = [vp, vp, vp, C.c_size_t]
    L.rt_host_free.argtypes = [vp]
    L.rt_kat_sphere.argtypes = [vp, fp3, C.c_int, fp3]
    L.rt_kat_sqrt.argtypes = [vp, fp3, C.c_int, fp3]
    L.rt_kat_box.argtypes = [vp, fp3, C.c_int, C.c_int, fp3, C.POINTER(KatCounts)]
    L.rt_kat_triangle.argtypes = [vp, fp3, C.c_int, fp3, C.POINTER(KatCounts)]
    L.rt_kat_mesh.argtypes = [vp, fp3, C.c_int, C.c_float, C.c_int, fp3, C.POINTER(KatCounts)]
    L.rt_kat_layout_hash.argtypes = [vp, C.POINTER(C.c_uint64)]
    _lib = L
    return L


class PinnedArray:
    """A float32 / uint8 numpy array over rt_host_alloc memory (frame buffer for rt_render*: the D2H copy is one DMA).

    The allocation lives as long as ANY view of it: `array`, its slices and whatever a render call returned all keep the underlying
    ctypes buffer alive, and the pinned memory is released when that buffer is collected -- close() only drops this object's own
    reference, it never frees memory somebody still looks at."""

    def __init__(self, shape, dtype=np.float32):
        L = load()
        p = C.c_void_p()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        rc = L.rt_host_alloc(C.byref(p), max(n, 16))
        if rc != RT_OK:
            raise RtError(rc, L.rt_last_error(None).decode())
        buf = (C.c_uint8 * max(n, 16)).from_address(p.value)
        weakref.finalize(buf, L.rt_host_free, C.c_void_p(p.value))    # runs when the last numpy view of `buf` is gone
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        self.array = None


def camera_basis(pose):
    """Camera::rotate() (realtime_render.cu:823-846) as the library computes it -> (bx, by, bz)."""
    out = [np.zeros(3, np.float32) for _ in range(3)]
    rc = load().rt_camera_basis(C.byref(pose), *[o.ctypes.data_as(C.POINTER(C.c_float)) for o in out])
    if rc != RT_OK:
        raise RtError(rc, "rt_camera_basis")
    return out


def light_orbit(light, angular_speed, dt=2e-2):
    """rt_light_orbit: MoveLightSource's motion (realtime_render.cu:1072-1090) of light = (position, intensity), as the library computes it -> (position, intensity)."""
    a, b = Light(), Light()
    a.position[:] = light[0]
    a.intensity = light[1]
    rc = load().rt_light_orbit(C.byref(a), C.c_float(angular_speed), C.c_float(dt), C.byref(b))
    if rc != RT_OK:
        raise RtError(rc, "rt_light_orbit")
    return tuple(float(x) for x in b.position), float(b.intensity)


def device_count():
    n = C.c_int(0)
    rc = load().rt_device_count(C.byref(n))
    return n.value if rc == RT_OK else 0


def make_params(width, height, num_rays=1, num_bounce=0, depth_convention=0, sigma=0.0, eps=1e-3, tri_tmin=1e-4,
                seed=123456, variant="auto"):
    p = Params()
    p.width, p.height, p.num_rays, p.num_bounce = width, height, num_rays, num_bounce
    p.depth_convention, p.sigma, p.eps, p.tri_tmin, p.seed = depth_convention, sigma, eps, tri_tmin, seed
    p.variant = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    return p


def interleaved_rows(height, tile_rows, rank, world):
    """Row tiles k*world+rank of `tile_rows` rows each.  Returns (Rows, image row indices)."""
    n_tiles = (height + tile_rows - 1) // tile_rows
    mine = list(range(rank, n_tiles, world))
    idx = np.concatenate([np.arange(t * tile_rows, min((t + 1) * tile_rows, height)) for t in mine]) if mine \
        else np.zeros(0, np.int64)
    r = Rows(rank * tile_rows, len(idx), tile_rows, world)
    return r, idx


def _marshal_scene(spheres, mesh, light, camera):
    """C structs of a scene description (shared by Context and MultiContext)."""
    arr = (Sphere * max(len(spheres), 1))()
    for i, s in enumerate(spheres):
        c, r, a = s[0], s[1], s[2]
        arr[i].center[:] = c
        arr[i].radius = r
        arr[i].albedo[:] = a
        arr[i].mirror = int(s[3]) if len(s) > 3 else 0
        arr[i].in_refraction_index = s[4] if len(s) > 4 else 1.0
        arr[i].out_refraction_index = s[5] if len(s) > 5 else 1.0
    meshes = [] if mesh is None else (list(mesh) if isinstance(mesh, (list, tuple)) else [mesh])
    marr, keep = (Mesh * max(len(meshes), 1))(), []
    taken = {d["object_slot"] for d in meshes if d.get("object_slot") is not None}
    free = (k for k in range(len(spheres) + len(meshes)) if k not in taken)
    for m, d in zip(marr, meshes):
        v = np.ascontiguousarray(d["vertices"], np.float32).reshape(-1, 3)
        ix = np.ascontiguousarray(d["indices"], np.int32)
        stride = ix.shape[1] if ix.ndim == 2 else 3
        bv = np.ascontiguousarray(d["bvh_arr10"], np.float32).reshape(-1, 10)
        m.vertices = v.ctypes.data_as(C.POINTER(C.c_float)); m.n_vertices = len(v)
        m.indices = ix.ctypes.data_as(C.POINTER(C.c_int32)); m.index_stride = stride
        m.n_triangles = ix.size // stride
        m.bvh_arr10 = bv.ctypes.data_as(C.POINTER(C.c_float)); m.n_nodes = len(bv)
        m.albedo[:] = d.get("albedo", (0.25, 0.25, 0.25))
        # a lone mesh without a slot is added last (cpu:685); several meshes without slots follow the spheres in list order
        m.object_slot = d["object_slot"] if d.get("object_slot") is not None else (len(spheres) if len(meshes) == 1 else next(free))
        m.mirror = int(d.get("mirror", 0))
        m.in_refraction_index = d.get("in_refraction_index", 1.0)
        m.out_refraction_index = d.get("out_refraction_index", 1.0)
        keep.append((v, ix, bv))
    lt = Light(); lt.position[:] = light[0]; lt.intensity = light[1]
    cam = Camera(); cam.position[:] = camera[0]
    # float alpha = PI/3 (cpu:666)
    cam.fov = np.float32(np.pi / 3) if camera[1] is None else np.float32(camera[1])
    return arr, len(spheres), marr, len(meshes), lt, cam, keep


class Context:
    """One rt_ctx = one GPU.  Methods mirror the C-ABI one to one."""

    def __init__(self, device_id=0):
        self._L = load()
        self._h = C.c_void_p()
        rc = self._L.rt_ctx_create(C.byref(self._h), device_id)
        if rc != RT_OK:
            raise RtError(rc, self._L.rt_last_error(None).decode())
        self._keep = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rt_ctx_destroy(self._h)                           # synchronises the copy streams: no frame is in flight afterwards
            self._h = C.c_void_p()
        if getattr(self, "_async_out", None):
            self._async_out.clear()

    __del__ = close

    def _check(self, rc):
        if rc != RT_OK:
            raise RtError(rc, self._L.rt_last_error(self._h).decode())

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        self._check(self._L.rt_device_name(self._h, buf, 256))
        return buf.value.decode()

    def scene_upload(self, spheres, mesh=None, light=((-10.0, 20.0, 40.0), 3e10), camera=((0.0, 0.0, 55.0), None)):
        """spheres: iterable of (center, radius, albedo[, mirror, n_in, n_out]);
        mesh: dict(vertices, indices, bvh_arr10, albedo, object_slot[, mirror, in_refraction_index, out_refraction_index]) with the reference's array
        layouts, or a list of such dicts (several TriangleMesh objects in Scene::objects: rt_scene_upload_meshes)."""
        arr, n, marr, nm, lt, cam, self._keep = _marshal_scene(spheres, mesh, light, camera)
        self._mesh_nv = {int(marr[k].object_slot): int(marr[k].n_vertices) for k in range(nm)}   # (mesh_vertex_normals sizes its result by it)
        if nm <= 1 and not isinstance(mesh, (list, tuple)):
            self._check(self._L.rt_scene_upload(self._h, arr, n, marr if nm else None, C.byref(lt), C.byref(cam)))
        else:
            self._check(self._L.rt_scene_upload_meshes(self._h, arr, n, marr, nm, C.byref(lt), C.byref(cam)))

    def render(self, params, row_begin=0, row_end=None, out=None):
        """out: optional preallocated [rows, W, 4] float32 array (e.g. PinnedArray(...).array)."""
        row_end = params.height if row_end is None else row_end
        if out is None:
            out = np.empty((max(row_end - row_begin, 0), params.width, 4), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == max(row_end - row_begin, 0) * params.width * 4
        self._check(self._L.rt_render(self._h, C.byref(params), row_begin, row_end, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_rgb8(self, params, row_begin=0, row_end=None):
        row_end = params.height if row_end is None else row_end
        out = np.empty((max(row_end - row_begin, 0), params.width, 3), np.uint8)
        self._check(self._L.rt_render_rgb8(self._h, C.byref(params), row_begin, row_end, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def render_device(self, params, rows, out_ptr, stream=None):
        """Asynchronous render into device memory (e.g. a torch tensor's data_ptr())."""
        self._check(self._L.rt_render_device(self._h, C.byref(params), C.byref(rows), C.c_void_p(out_ptr),
                                             C.c_void_p(stream) if stream else None))

    def render_device_batch(self, params, rows, frames, stream=None, scenes=None):
        """rt_render_device_batch: `frames` = iterable of (out_ptr, camera_position, fov or None, seed); ONE launch chain traces them all (num_rays == 1).
        scenes: per frame (light, [(centre, radius), ...]) with light = (position, intensity) and one pose per uploaded sphere, in the uploaded order: the frame's own
        light and sphere poses (rt_render_device_batch_scenes); None = the uploaded scene in every frame."""
        frames = list(frames)
        arr = (FrameDesc * max(len(frames), 1))()
        for d, (ptr, pos, fov, seed) in zip(arr, frames):
            d.camera.position[:] = pos
            d.camera.fov = np.float32(np.pi / 3) if fov is None else np.float32(fov)
            d.seed = int(seed)
            d.out_rgba_dev = int(ptr)
        if scenes is None:
            self._check(self._L.rt_render_device_batch(self._h, C.byref(params), C.byref(rows), arr, len(frames), C.c_void_p(stream) if stream else None))
            return
        scenes = list(scenes)
        if len(scenes) != len(frames):
            raise ValueError("scenes: one (light, sphere poses) per frame")
        n_sph = len(scenes[0][1]) if scenes else 0
        sarr = (FrameScene * max(len(scenes), 1))()
        for d, (light, poses) in zip(sarr, scenes):
            poses = list(poses)
            if len(poses) != n_sph or n_sph > MAX_SPHERES:
                raise ValueError("scenes: every frame poses the same (uploaded) spheres")
            d.light.position[:] = light[0]
            d.light.intensity = light[1]
            for q, (centre, radius) in zip(d.spheres, poses):
                q.center[:] = centre
                q.radius = radius
        self._check(self._L.rt_render_device_batch_scenes(self._h, C.byref(params), C.byref(rows), arr, sarr, n_sph, len(frames), C.c_void_p(stream) if stream else None))

    # --- the light and the spheres of the scene in use, edited in place (rt_scene_*): no mesh work, smooth normals / textures / transforms / rebuilt trees stay
    def light(self):
        """rt_scene_get_light -> (position, intensity)"""
        l = Light()
        self._check(self._L.rt_scene_get_light(self._h, C.byref(l)))
        return tuple(float(x) for x in l.position), float(l.intensity)

    def set_light(self, position, intensity):
        l = Light()
        l.position[:] = position
        l.intensity = intensity
        self._check(self._L.rt_scene_set_light(self._h, C.byref(l)))

    # --- several point lights (rt_scene_set_lights): one picked per diffuse hit, by intensity; a light is (position, intensity)
    def set_lights(self, lights):
        """rt_scene_set_lights: the scene's lights become this list of (position, intensity), 1 .. MAX_LIGHTS of them"""
        lights = list(lights)
        arr = (Light * max(len(lights), 1))()
        for l, (position, intensity) in zip(arr, lights):
            l.position[:] = position
            l.intensity = intensity
        self._check(self._L.rt_scene_set_lights(self._h, arr, len(lights)))

    def lights(self):
        """rt_scene_get_lights -> [(position, intensity), ...]"""
        arr = (Light * MAX_LIGHTS)()
        n = C.c_int(0)
        self._check(self._L.rt_scene_get_lights(self._h, arr, MAX_LIGHTS, C.byref(n)))
        return [(tuple(float(x) for x in arr[k].position), float(arr[k].intensity)) for k in range(n.value)]

    def set_light_at(self, k, position, intensity):
        """rt_scene_set_light_at: light k of the list"""
        l = Light()
        l.position[:] = position
        l.intensity = intensity
        self._check(self._L.rt_scene_set_light_at(self._h, int(k), C.byref(l)))

    def move_light_at(self, k, angular_speed, dt=2e-2):
        """MoveLightSource (realtime_render.cu:1072-1090) on light k of the list"""
        self._check(self._L.rt_scene_move_light_at(self._h, int(k), C.c_float(angular_speed), C.c_float(dt)))

    # --- soft shadows (rt_scene_set_light_radii): light k is a shell of radius radii[k] about its position, one point of it per shadow ray
    def set_light_radii(self, radii):
        """rt_scene_set_light_radii: one radius per light of the list"""
        radii = [float(r) for r in radii]
        arr = (C.c_float * max(len(radii), 1))(*radii)
        self._check(self._L.rt_scene_set_light_radii(self._h, arr, len(radii)))

    def light_radii(self):
        """rt_scene_get_light_radii -> [radius, ...]"""
        arr = (C.c_float * MAX_LIGHTS)()
        n = C.c_int(0)
        self._check(self._L.rt_scene_get_light_radii(self._h, arr, MAX_LIGHTS, C.byref(n)))
        return [float(arr[k]) for k in range(n.value)]

    def set_light_radius_at(self, k, radius):
        """rt_scene_set_light_radius_at: the radius of light k of the list"""
        self._check(self._L.rt_scene_set_light_radius_at(self._h, int(k), C.c_float(radius)))

    # --- thin lens (rt_camera_set_lens): an aperture radius and a focus distance; radius 0 is the pinhole
    def set_lens(self, radius, focus):
        """rt_camera_set_lens: aperture radius and focus distance along the view axis, in scene units"""
        self._check(self._L.rt_camera_set_lens(self._h, C.c_float(radius), C.c_float(focus)))

    def lens(self):
        """rt_camera_get_lens -> (radius, focus)"""
        r, f = C.c_float(0), C.c_float(0)
        self._check(self._L.rt_camera_get_lens(self._h, C.byref(r), C.byref(f)))
        return float(r.value), float(f.value)

    # --- shutter (rt_scene_set_shutter): what the light and the spheres travel within one frame's exposure; all zero is the closed shutter
    def set_shutter(self, light=None, objects=None):
        """rt_scene_set_shutter: light = the light's displacement over the exposure, objects = {object_slot: displacement}; neither: NULL, the shutter is closed"""
        if light is None and objects is None:
            self._check(self._L.rt_scene_set_shutter(self._h, None))
            return
        s = Shutter()
        s.light[:] = [float(x) for x in (light if light is not None else (0.0, 0.0, 0.0))]
        for slot, v in (objects or {}).items():
            s.object[int(slot)][:] = [float(x) for x in v]
        self._check(self._L.rt_scene_set_shutter(self._h, C.byref(s)))

    def shutter(self):
        """rt_scene_get_shutter -> (light [3], objects [MAX_OBJECTS, 3]) as float32 arrays"""
        s = Shutter()
        self._check(self._L.rt_scene_get_shutter(self._h, C.byref(s)))
        return np.array(s.light, np.float32), np.array([list(o) for o in s.object], np.float32)

    # --- environment (rt_scene_set_environment): an octahedral radiance map for the rays that miss the scene
    def set_environment(self, rgb=None):
        """rt_scene_set_environment: rgb = an [n, n, 3] float32 array, row 0 first (environment.py makes them); None: the map is removed"""
        if rgb is None:
            self._check(self._L.rt_scene_set_environment(self._h, 0, None))
            return
        a = np.ascontiguousarray(rgb, dtype=np.float32)
        if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
            raise ValueError(f"an environment is an [n, n, 3] array, not {a.shape}")
        self._check(self._L.rt_scene_set_environment(self._h, int(a.shape[0]), a.ctypes.data_as(C.POINTER(C.c_float))))

    def environment(self):
        """rt_scene_get_environment -> the [n, n, 3] float32 array as stored, or None without a map"""
        n = C.c_int(0)
        self._check(self._L.rt_scene_get_environment(self._h, C.byref(n), None))
        if n.value == 0:
            return None
        out = np.empty((n.value, n.value, 3), np.float32)
        self._check(self._L.rt_scene_get_environment(self._h, C.byref(n), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def kat_environment(self, dirs):
        """rt_kat_environment: sky_radiance on [n, 3] explicit directions against the context's map -> [n, 3] float32"""
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros_like(d)
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_kat_environment(self._h, int(d.shape[0]), d.ctypes.data_as(fp), out.ctypes.data_as(fp)))
        return out

    # --- sky sampling (rt_scene_set_environment_sampling): the share of the shadow rays drawn from the map by radiance, and the table's known answers
    def set_environment_sampling(self, share):
        """rt_scene_set_environment_sampling: share in [0, 1]; 0 is off"""
        self._check(self._L.rt_scene_set_environment_sampling(self._h, C.c_float(share)))

    def environment_sampling(self):
        """rt_scene_get_environment_sampling -> the share as set"""
        s = C.c_float(0)
        self._check(self._L.rt_scene_get_environment_sampling(self._h, C.byref(s)))
        return float(s.value)

    def kat_environment_table(self):
        """rt_kat_environment_table for the context's n x n map -> (c [n * n] uint32, prefix [n * n] uint64, total); an empty table: zeros and 0"""
        nn = C.c_int(0)
        self._check(self._L.rt_scene_get_environment(self._h, C.byref(nn), None))
        n = nn.value
        c = np.zeros(int(n) * int(n), np.uint32)
        prefix = np.zeros(int(n) * int(n), np.uint64)
        total = C.c_uint64(0)
        self._check(self._L.rt_kat_environment_table(self._h, c.ctypes.data_as(C.POINTER(C.c_uint32)), prefix.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total)))
        return c, prefix, int(total.value)

    def kat_environment_sample(self, hs, seg):
        """rt_kat_environment_sample: the draw on explicit sample keys hs [k] uint32 and segments seg [k] -> (texel [k] uint32, direction [k, 3] float32, g at mx = 1 [k] float32)"""
        h = np.ascontiguousarray(hs, dtype=np.uint32).ravel()
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(seg, np.int32), h.shape), dtype=np.int32)
        texel, dirs, g = np.zeros(h.size, np.uint32), np.zeros((h.size, 3), np.float32), np.zeros(h.size, np.float32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._check(self._L.rt_kat_environment_sample(self._h, int(h.size), h.ctypes.data_as(up), d.ctypes.data_as(C.POINTER(C.c_int32)), texel.ctypes.data_as(up),
                                                      dirs.ctypes.data_as(fp), g.ctypes.data_as(fp)))
        return texel, dirs, g

    # --- emissive meshes (rt_scene_set_emission): a mesh's radiance, the share of the shadow rays drawn towards the emitters, and the table's known answers
    def set_emission(self, object_slot, rgb):
        """rt_scene_set_emission: the radiance (r, g, b) of the mesh at object_slot; (0, 0, 0): it does not emit"""
        v = (C.c_float * 3)(*[float(x) for x in rgb])
        self._check(self._L.rt_scene_set_emission(self._h, int(object_slot), v))

    def emission(self, object_slot):
        """rt_scene_get_emission -> (r, g, b) as set"""
        v = (C.c_float * 3)()
        self._check(self._L.rt_scene_get_emission(self._h, int(object_slot), v))
        return tuple(float(x) for x in v)

    def set_emission_sampling(self, share):
        """rt_scene_set_emission_sampling: share in [0, 1]; an upload sets 0.5"""
        self._check(self._L.rt_scene_set_emission_sampling(self._h, C.c_float(share)))

    def emission_sampling(self):
        """rt_scene_get_emission_sampling -> the share as set"""
        s = C.c_float(0)
        self._check(self._L.rt_scene_get_emission_sampling(self._h, C.byref(s)))
        return float(s.value)

    def kat_emission_table(self):
        """rt_kat_emission_table -> (c [n_triangles] uint32, prefix [n_triangles] uint64, total) over the scene's triangles in stored order; no emitter or an empty table: zeros and 0"""
        total, nt = C.c_uint64(0), C.c_int32(0)
        self._check(self._L.rt_kat_emission_table(self._h, None, None, C.byref(total), C.byref(nt)))
        c = np.zeros(int(nt.value), np.uint32)
        prefix = np.zeros(int(nt.value), np.uint64)
        self._check(self._L.rt_kat_emission_table(self._h, c.ctypes.data_as(C.POINTER(C.c_uint32)), prefix.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total), C.byref(nt)))
        return c, prefix, int(total.value)

    def kat_emission_sample(self, hs, seg):
        """rt_kat_emission_sample: the draw on explicit sample keys hs [k] uint32 and segments seg [k] -> (triangle [k] uint32 in stored order, point [k, 3] float32)"""
        h = np.ascontiguousarray(hs, dtype=np.uint32).ravel()
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(seg, np.int32), h.shape), dtype=np.int32)
        tri, point = np.zeros(h.size, np.uint32), np.zeros((h.size, 3), np.float32)
        up = C.POINTER(C.c_uint32)
        self._check(self._L.rt_kat_emission_sample(self._h, int(h.size), h.ctypes.data_as(up), d.ctypes.data_as(C.POINTER(C.c_int32)), tri.ctypes.data_as(up),
                                                   point.ctypes.data_as(C.POINTER(C.c_float))))
        return tri, point

    # --- Fresnel dielectrics (rt_material_set_fresnel): the per-object flag and the device step's known answer
    def set_fresnel(self, object_slot, on=True):
        """rt_material_set_fresnel: the object at object_slot reflects with its Fresnel reflectance and refracts otherwise (effective on glass alone); an upload clears it"""
        self._check(self._L.rt_material_set_fresnel(self._h, int(object_slot), int(bool(on))))

    def fresnel(self, object_slot):
        """rt_material_get_fresnel -> the flag as set"""
        on = C.c_int(0)
        self._check(self._L.rt_material_get_fresnel(self._h, int(object_slot), C.byref(on)))
        return bool(on.value)

    def kat_fresnel(self, n_in, n_out, refr, eps, P, N, u, hs, seg):
        """rt_kat_fresnel: the device step on k explicit items (scalars broadcast; P, N, u [k, 3]) -> (R [k] float32, code [k] int32: 0 refracted, 1 reflected,
        2 totally reflected, O [k, 3], u [k, 3], the index after [k])"""
        h = np.ascontiguousarray(hs, dtype=np.uint32).ravel()
        k = h.size
        items = np.zeros((k, 16), np.uint32)
        f = items.view(np.float32)
        f[:, 0], f[:, 1], f[:, 2], f[:, 3] = n_in, n_out, refr, eps
        f[:, 4:7], f[:, 7:10], f[:, 10:13] = np.asarray(P, np.float32).reshape(-1, 3), np.asarray(N, np.float32).reshape(-1, 3), np.asarray(u, np.float32).reshape(-1, 3)
        items[:, 13] = h
        items[:, 14] = np.broadcast_to(np.asarray(seg, np.int32), (k,)).view(np.uint32) if np.ndim(seg) else np.uint32(int(seg))
        out = np.zeros((k, 9), np.uint32)
        up = C.POINTER(C.c_uint32)
        self._check(self._L.rt_kat_fresnel(self._h, int(k), items.ctypes.data_as(up), out.ctypes.data_as(up)))
        g = out.view(np.float32)
        return g[:, 0].copy(), out[:, 1].astype(np.int32), g[:, 2:5].copy(), g[:, 5:8].copy(), g[:, 8].copy()

    # --- rough mirrors (rt_material_set_roughness): the per-object GGX roughness and the device step's known answer
    def set_roughness(self, object_slot, alpha):
        """rt_material_set_roughness: the object at object_slot reflects about a GGX facet of width alpha (0: smooth; effective on mirrors alone); an upload clears it"""
        self._check(self._L.rt_material_set_roughness(self._h, int(object_slot), float(alpha)))

    def roughness(self, object_slot):
        """rt_material_get_roughness -> alpha as set"""
        a = C.c_float(0)
        self._check(self._L.rt_material_get_roughness(self._h, int(object_slot), C.byref(a)))
        return float(a.value)

    def kat_gloss(self, alpha, eps, P, N, u, hs, seg):
        """rt_kat_gloss: the device step on k explicit items (scalars broadcast; P, N, u [k, 3]) -> (h [k, 3] float32, code [k] int32: 0 plain, 1 folded back,
        O [k, 3], u [k, 3])"""
        h = np.ascontiguousarray(hs, dtype=np.uint32).ravel()
        k = h.size
        items = np.zeros((k, 16), np.uint32)
        f = items.view(np.float32)
        f[:, 0], f[:, 1] = alpha, eps
        f[:, 2:5], f[:, 5:8], f[:, 8:11] = np.asarray(P, np.float32).reshape(-1, 3), np.asarray(N, np.float32).reshape(-1, 3), np.asarray(u, np.float32).reshape(-1, 3)
        items[:, 11] = h
        items[:, 12] = np.broadcast_to(np.asarray(seg, np.int32), (k,)).view(np.uint32) if np.ndim(seg) else np.uint32(int(seg))
        out = np.zeros((k, 12), np.uint32)
        up = C.POINTER(C.c_uint32)
        self._check(self._L.rt_kat_gloss(self._h, int(k), items.ctypes.data_as(up), out.ctypes.data_as(up)))
        g = out.view(np.float32)
        return g[:, 0:3].copy(), out[:, 3].astype(np.int32), g[:, 4:7].copy(), g[:, 7:10].copy()

    # --- tinted mirrors and glass (rt_material_set_tint): the per-object flag
    def set_tint(self, object_slot, on=True):
        """rt_material_set_tint: what is seen in or through the mirror or glass object at object_slot is multiplied by its albedo (effective on mirrors and glass alone);
        an upload clears it"""
        self._check(self._L.rt_material_set_tint(self._h, int(object_slot), 1 if on else 0))

    def tint(self, object_slot):
        """rt_material_get_tint -> bool"""
        v = C.c_int(0)
        self._check(self._L.rt_material_get_tint(self._h, int(object_slot), C.byref(v)))
        return bool(v.value)

    def sphere(self, object_slot):
        """rt_scene_get_sphere -> (centre, radius, albedo, mirror, n_in, n_out): the tuple scene_upload takes"""
        s = Sphere()
        self._check(self._L.rt_scene_get_sphere(self._h, int(object_slot), C.byref(s)))
        return (tuple(float(x) for x in s.center), float(s.radius), tuple(float(x) for x in s.albedo), int(s.mirror),
                float(s.in_refraction_index), float(s.out_refraction_index))

    def set_sphere(self, object_slot, sphere):
        """rt_scene_set_sphere: geometry and material of the sphere at position object_slot of Scene::objects; sphere as scene_upload takes it"""
        arr = _marshal_scene([sphere], None, ((0.0, 0.0, 0.0), 0.0), ((0.0, 0.0, 0.0), None))[0]
        self._check(self._L.rt_scene_set_sphere(self._h, int(object_slot), C.byref(arr[0])))

    def move_light(self, angular_speed, dt=2e-2):
        """MoveLightSource (realtime_render.cu:1072-1090)"""
        self._check(self._L.rt_scene_move_light(self._h, C.c_float(angular_speed), C.c_float(dt)))

    def move_sphere(self, object_slot, v, dt=0.2):
        """MoveObject (realtime_render.cu:1092-1098): C += v * dt"""
        vv = np.ascontiguousarray(v, np.float32).reshape(3)
        self._check(self._L.rt_scene_move_sphere(self._h, int(object_slot), vv.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(dt)))

    def render_async(self, params, out, slot=0, rgb8=False):
        """rt_render_async: whole frame into device buffer `slot` (0 / 1), device-to-host copy into `out` on the copy stream;
        wait(slot) returns when `out` holds the frame.  out: [H, W, 4] float32 or, rgb8, [H, W, 3] uint8 (PinnedArray: one DMA)."""
        want = (np.uint8, 3) if rgb8 else (np.float32, 4)
        assert out.dtype == want[0] and out.flags.c_contiguous and out.size == params.height * params.width * want[1]
        # the copy stream writes into `out` until wait(slot): the context keeps the array (and through it a PinnedArray's block, which is
        # freed when its last view goes) alive for exactly that long -- a caller may drop its own reference at once
        if not hasattr(self, "_async_out"):
            self._async_out = {}
        self._async_out[int(slot)] = out
        self._check(self._L.rt_render_async(self._h, C.byref(params), int(slot), C.c_void_p(out.ctypes.data), 1 if rgb8 else 0))

    def wait(self, slot=0):
        try:
            self._check(self._L.rt_wait(self._h, int(slot)))
        finally:
            getattr(self, "_async_out", {}).pop(int(slot), None)

    def trace_rays(self, rays, tri_tmin=1e-4, variant="auto"):
        """rt_trace_rays: rays [n, 6] (O, u) through the production traversal kernel of `variant` -> [n, 5] (hit, t, N)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.empty((rays.shape[0], 5), np.float32)
        v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
        self._check(self._L.rt_trace_rays(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), rays.shape[0], C.c_float(tri_tmin), v,
                                          out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def stats_enable(self, on=True):
        """trav_ms / trav_launches of stats() are measured only while enabled (production frames record no per-launch events)."""
        self._check(self._L.rt_stats_enable(self._h, 1 if on else 0))

    def _still_counts(self, entry, first):
        """the four counters of one level of the still view (csrc/rt_still.h)"""
        fc = (C.c_uint64 * 4)()
        self._check(getattr(self._L, entry)(self._h, fc))
        return dict(zip((first, "filled", "ineligible", "key_misses"), (int(v) for v in fc)))

    def first_hit_cache_counts(self):
        """rt_first_hit_cache_counts: launch chains of this context that skipped their first traversal launch, that filled the cache, that were not eligible, and
        key comparisons that emptied a filled cache."""
        return self._still_counts("rt_first_hit_cache_counts", "skipped")

    def first_shadow_cache_counts(self):
        """rt_first_shadow_cache_counts: launch chains of this context that handed no shadow ray of their first segment to the traversal (the cached answers were read),
        that filled the cache, that were not eligible, and key comparisons that emptied a filled cache."""
        return self._still_counts("rt_first_shadow_cache_counts", "skipped")

    def first_shade_cache_counts(self):
        """rt_first_shade_cache_counts: launch chains of this context that resumed their paths at the shaded first hit (one launch in place of the camera-ray launch and the
        close of segment 0), that filled the cache, that were not eligible, and replacements of the first-shadow cache's key that emptied a filled cache."""
        return self._still_counts("rt_first_shade_cache_counts", "resumed")

    def set_pipelining(self, on=True):
        """rt_ctx_set_pipelining: consecutive render_device calls on one stream into alternating buffers overlap at the frame boundary."""
        self._check(self._L.rt_ctx_set_pipelining(self._h, 1 if on else 0))

    def tonemap_device(self, rgba_ptr, n_pixels, rgb8_ptr, stream=None):
        self._check(self._L.rt_tonemap_device(self._h, C.c_void_p(rgba_ptr), n_pixels, C.c_void_p(rgb8_ptr),
                                              C.c_void_p(stream) if stream else None))

    def count_work(self, params, row_begin=0, row_end=None, detail=False):
        """Traversal work of a frame from the counting instantiation of the kernel: rays, box tests, nodes, triangle
        tests -- what the oracle counts.  detail=True adds the tests the literal divisions decided and the work-stack kernel's
        step counters."""
        row_end = params.height if row_end is None else row_end
        w = Work()
        self._check(self._L.rt_count_work(self._h, C.byref(params), row_begin, row_end, C.byref(w)))
        out = {k: int(getattr(w, k)) for k in ("rays", "box_tests", "nodes", "tri_tests")}
        if not detail:
            return out
        out.update(box_literal=int(w.box_literal), tri_literal=int(w.tri_literal))
        dc = (C.c_uint64 * 4)()
        self._check(self._L.rt_dead_channel_counts(self._h, dc))
        out["dead_channels"] = dict(zip(("trav_continuation", "trav_shadow", "elided", "unsure"), (int(v) for v in dc)))   # rt_dead_channel_counts
        dl = C.c_uint64(0)
        self._check(self._L.rt_dead_last_count(self._h, C.byref(dl)))
        out["dead_last"] = int(dl.value)                              # rt_dead_last_count
        out["steps"] = dict(zip(("iterations", "refill_passes", "refill_rounds", "fetches", "tri_steps", "box_steps", "literal_box_fallbacks", "serial_drains",
                                 "tdiv_blocks", "leaf_push_blocks", "leaf_push2_blocks", "anyhit_stop_steps"),
                                (int(v) for v in w.steps)))
        return out

    def mesh_transform(self, rotation, translation, object_slot=None):
        """Device-side `transform` kernel (global_launcher.cu:340-365) on the uploaded mesh + triangle precompute + BVH refit.
        object_slot: move only the mesh at that position in Scene::objects (rt_mesh_transform_of); None = every mesh (rt_mesh_transform)."""
        r = np.ascontiguousarray(rotation, np.float32).reshape(9)
        t = np.ascontiguousarray(translation, np.float32).reshape(3)
        rp, tp = r.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float))
        if object_slot is None:
            self._check(self._L.rt_mesh_transform(self._h, rp, tp))
        else:
            self._check(self._L.rt_mesh_transform_of(self._h, int(object_slot), rp, tp))

    def mesh_set_vertices(self, vertices=None, object_slot=None, device_ptr=None, stride=3, n_vertices=None):
        """A mesh that changes shape: new positions [n, 3] for every vertex, in the uploaded order (rt_mesh_set_vertices[_of]); indices, tree topology, normals, UVs and
        textures stay and every box is refitted on the device.  Smooth normals are the caller's: pass the new ones to mesh_set_normals again, or call mesh_compute_normals.
        device_ptr= (with n_vertices= and stride= 3 or 4 floats per record): the positions are in device memory and are read on the context's stream
        (rt_mesh_set_vertices_device).  object_slot: the mesh at that position in Scene::objects; None = the scene's one mesh."""
        if device_ptr is not None:
            if vertices is not None or n_vertices is None:
                raise ValueError("mesh_set_vertices: device_ptr= goes with n_vertices= and without an array")
            self._check(self._L.rt_mesh_set_vertices_device(self._h, -1 if object_slot is None else int(object_slot), C.c_void_p(int(device_ptr)), int(stride), int(n_vertices)))
            return
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        vp_ = v.ctypes.data_as(C.POINTER(C.c_float))
        if object_slot is None:
            self._check(self._L.rt_mesh_set_vertices(self._h, vp_, len(v)))
        else:
            self._check(self._L.rt_mesh_set_vertices_of(self._h, int(object_slot), vp_, len(v)))

    def mesh_snapshot_vertices(self, object_slot=None, keep=True):
        """rt_mesh_snapshot_vertices: keep the positions a mesh has NOW as its previous ones, for render_aov_motion -- once per frame, before that frame's
        mesh_set_vertices / mesh_transform calls.  object_slot: the mesh at that position in Scene::objects; None = every mesh with triangles.  keep=False drops the
        snapshot: the object follows the rigid motion table again.  A device-to-device copy on the context's stream; the host does not wait."""
        self._check(self._L.rt_mesh_snapshot_vertices(self._h, -1 if object_slot is None else int(object_slot), int(keep)))

    def mesh_snapshot_mask(self):
        """rt_mesh_snapshot_mask: bit i set = object i holds a vertex snapshot."""
        m = C.c_uint32(0)
        self._check(self._L.rt_mesh_snapshot_mask(self._h, C.byref(m)))
        return int(m.value)

    def mesh_compute_normals(self, object_slot=None):
        """rt_mesh_compute_normals[_of]: the mesh gets one normal per position vertex -- the area-weighted sum of its incident triangles' face normals, normalised, of the
        shape the mesh has NOW on the device -- and shades with them as after mesh_set_normals(those, the triangles' vertex indices).  On the context's stream behind the
        mesh_set_vertices / mesh_transform calls issued so far; after the first call the host does not wait.  object_slot: the mesh at that position in
        Scene::objects (rt_mesh_compute_normals_of); None = the scene's one mesh."""
        if object_slot is None:
            self._check(self._L.rt_mesh_compute_normals(self._h))
        else:
            self._check(self._L.rt_mesh_compute_normals_of(self._h, int(object_slot)))

    def mesh_vertex_normals(self, object_slot=None, n_vertices=None):
        """rt_mesh_get_vertex_normals -> [nv, 3] float32: the per-vertex normals as the last mesh_compute_normals of that mesh wrote them (a later mesh_transform is not
        followed).  object_slot None = the scene's one mesh.  n_vertices: the mesh's vertex count; None = the count it was uploaded with through this Context."""
        nv = n_vertices
        if nv is None:
            known = getattr(self, "_mesh_nv", {})
            nv = known.get(int(object_slot)) if object_slot is not None else (next(iter(known.values())) if len(known) == 1 else None)
        if nv is None:
            raise RtError(-1, "mesh_vertex_normals: pass n_vertices= (this Context uploaded no such mesh)")
        out = np.zeros((int(nv), 3), np.float32)
        self._check(self._L.rt_mesh_get_vertex_normals(self._h, -1 if object_slot is None else int(object_slot), out.ctypes.data_as(C.POINTER(C.c_float)), int(nv)))
        return out

    def mesh_snapshot_normals(self, object_slot=None, keep=True):
        """rt_mesh_snapshot_normals: keep the shading normals a smooth mesh has NOW as its previous ones, for render_aov_motion's N' -- once per frame beside
        mesh_snapshot_vertices, before that frame's edits and its mesh_compute_normals.  object_slot None = every smooth mesh; a flat mesh: nothing happens.
        keep=False drops the snapshot.  An upload and every mesh_rebuild drop all of them.  A device-to-device copy on the context's stream; the host does not wait."""
        self._check(self._L.rt_mesh_snapshot_normals(self._h, -1 if object_slot is None else int(object_slot), int(keep)))

    def mesh_normal_snapshot_mask(self):
        """rt_mesh_normal_snapshot_mask: bit i set = object i holds a normal snapshot."""
        m = C.c_uint32(0)
        self._check(self._L.rt_mesh_normal_snapshot_mask(self._h, C.byref(m)))
        return int(m.value)

    def mesh_rebuild(self, n_triangles, mode="reference", object_slot=None):
        """Device-side BVH build over the uploaded triangles and the current device vertices -> (bvh_arr10 [n_nodes, 10], order [n_triangles]).
        mode "reference": TriangleMesh::buildBVH bit for bit; "lbvh": Morton sort + parallel hierarchy, leaves cut by the surface-area heuristic (at most 32 triangles).
        object_slot: rebuild only the mesh at that position (rt_mesh_rebuild_of); n_triangles is then that mesh's count and the outputs are in its own index space."""
        arr = np.zeros(((2 * n_triangles + 2), 10), np.float32)
        order = np.zeros(n_triangles, np.int32)
        n = C.c_int32(0)
        ap, op = arr.ctypes.data_as(C.POINTER(C.c_float)), order.ctypes.data_as(C.POINTER(C.c_int32))
        if object_slot is None:
            self._check(self._L.rt_mesh_rebuild_mode(self._h, BVH_MODES[mode], ap, op, C.byref(n)))
        else:
            self._check(self._L.rt_mesh_rebuild_of(self._h, int(object_slot), BVH_MODES[mode], ap, op, C.byref(n)))
        return arr[:n.value].copy(), order

    def build_stats(self):
        s = BuildStats()
        self._check(self._L.rt_mesh_build_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in BuildStats._fields_}

    def mesh_set_normals(self, normals, nidx, object_slot=None):
        """Smooth shading: vertex normals + per-triangle (ni, nj, nk) rows in the order of the uploaded indices; None = flat.
        object_slot: only the mesh at that position, rows in its own triangle order (rt_mesh_set_normals_of); None = the scene's one mesh."""
        if normals is None:
            if object_slot is None:
                self._check(self._L.rt_mesh_set_normals(self._h, None, 0, None, 3, 0))
            else:
                self._check(self._L.rt_mesh_set_normals_of(self._h, int(object_slot), None, 0, None, 3, 0))
            return
        n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        ix = np.ascontiguousarray(nidx, np.int32).reshape(-1, 3)
        np_, ip = n.ctypes.data_as(C.POINTER(C.c_float)), ix.ctypes.data_as(C.POINTER(C.c_int32))
        if object_slot is None:
            self._check(self._L.rt_mesh_set_normals(self._h, np_, len(n), ip, 3, len(ix)))
        else:
            self._check(self._L.rt_mesh_set_normals_of(self._h, int(object_slot), np_, len(n), ip, 3, len(ix)))

    def mesh_set_texture(self, uvs, uvidx, texels, filter="nearest", wrap="repeat", decode=None, object_slot=None):
        """map_Kd of a textured mesh (rt_mesh_set_texture[_of]): uvs [n, 2] (OBJ vt), uvidx [n_triangles, 3] per-corner UV indices in the order of the
        uploaded indices, texels uint8 [height, width, 3 or 4] (top row first), filter "nearest" / "bilinear", wrap "repeat" / "clamp" (or the
        enum values), decode: 256 floats (None = byte / 255).  uvs or texels None = untextured again.  object_slot: only the mesh at that position."""
        fn = (lambda *a: self._L.rt_mesh_set_texture(self._h, *a)) if object_slot is None else (lambda *a: self._L.rt_mesh_set_texture_of(self._h, int(object_slot), *a))
        if uvs is None or texels is None:
            self._check(fn(None, 0, None, 3, 0, None))
            return
        uv = np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
        ix = np.ascontiguousarray(uvidx, np.int32).reshape(-1, 3)
        tx = np.ascontiguousarray(texels, np.uint8)
        if tx.ndim != 3:
            raise ValueError("texels: [height, width, channels] uint8")
        tex = Texture()
        tex.texels = tx.ctypes.data_as(C.POINTER(C.c_uint8))
        tex.height, tex.width, tex.channels = tx.shape
        tex.filter = TEX_FILTERS[filter] if isinstance(filter, str) else int(filter)
        tex.wrap = TEX_WRAPS[wrap] if isinstance(wrap, str) else int(wrap)
        dec = None
        if decode is not None:
            dec = np.ascontiguousarray(decode, np.float32).reshape(-1)
            if dec.size != 256:
                raise ValueError("decode: 256 floats")
            tex.decode = dec.ctypes.data_as(C.POINTER(C.c_float))
        self._check(fn(uv.ctypes.data_as(C.POINTER(C.c_float)), len(uv), ix.ctypes.data_as(C.POINTER(C.c_int32)), 3, len(ix), C.byref(tex)))

    def kat_surface(self, rays, tri_tmin=1e-4):
        """rt_kat_surface: rays [n, 6] through the production traversal, then the shading kernel's texture lookup -> [n, 8]
        (object slot or -1, triangle in its mesh's uploaded order, t, u, v, albedo rgb)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 8), np.float32)
        self._check(self._L.rt_kat_surface(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), rays.shape[0], C.c_float(tri_tmin),
                                           out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # --- first-hit feature buffers and the edge-avoiding filter they guide (rt_render_aov*, rt_denoise*)
    @staticmethod
    def _f32(a, shape_ok, message):
        """a as a contiguous float32 array whose shape passes shape_ok, else RtError(-1, message)"""
        a = np.ascontiguousarray(a, np.float32)
        if not shape_ok(a.shape):
            raise RtError(-1, message)
        return a

    @staticmethod
    def _out(name, out, shape):
        """the optional preallocated result of `name`: a contiguous float32 array of `shape` (None: a new one, zeroed)"""
        if out is None:
            return np.zeros(shape, np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != shape:
            raise RtError(-1, f"{name}: out must be a contiguous float32 array of shape {shape}")
        return out

    @staticmethod
    def _rows_or_whole(params, rows):
        """rows, or the Rows of the whole frame: what the *_aov*_device entries take when the caller names none"""
        return Rows(0, params.height, max(params.height, 1), 1) if rows is None else rows

    def render_aov(self, params, pose=None, rows=None):
        """rt_render_aov: the G-buffer of the pixel-centre camera rays -> [3, n_rows, W, 4] float32: plane 0 (normal, object id or -1), plane 1 (hit point, 1 / 0),
        plane 2 (albedo, 0).  pose: a CameraPose (None = the uploaded camera); rows: a Rows (None = the whole frame).  The first hit, whatever its material."""
        n_rows = params.height if rows is None else rows.n_rows
        out = np.zeros((3, max(n_rows, 0), params.width, 4), np.float32)
        self._check(self._L.rt_render_aov(self._h, C.byref(params), C.byref(pose) if pose is not None else None, C.byref(rows) if rows is not None else None,
                                          out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_aov_device(self, params, out_ptr, pose=None, rows=None, stream=None):
        """rt_render_aov_device: the same three planes into device memory (3 * n_rows * W float4), asynchronous on `stream`."""
        self._check(self._L.rt_render_aov_device(self._h, C.byref(params), C.byref(pose) if pose is not None else None, C.byref(self._rows_or_whole(params, rows)),
                                                 C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    @staticmethod
    def _motion_table(name, motion):
        """(the [MAX_OBJECTS, 12] float32 table kept alive, its rt_motion pointer) of a motion= argument; None = (None, None)"""
        if motion is None:
            return None, None
        m = np.ascontiguousarray(motion, np.float32)
        if m.shape != (MAX_OBJECTS, 12):
            raise RtError(-1, f"{name}: motion {m.shape} must be [{MAX_OBJECTS}, 12]")
        return m, m.ctypes.data_as(C.POINTER(Motion))

    def render_aov_motion(self, params, pose=None, rows=None, motion=None):
        """rt_render_aov_motion: render_aov's three planes and, from the same traversal, the two PREVIOUS-FRAME planes -> (aov [3, n_rows, W, 4], prev [2, n_rows, W, 4]):
        prev[0] = (N', object id or -1), prev[1] = (P', 1 / 0): where each pixel's surface point and normal were in the previous frame -- a mesh with a vertex snapshot
        (mesh_snapshot_vertices) by its triangle's previous corners, every other object by its record of motion ([MAX_OBJECTS, 12] as static_motion() lays it out;
        None = static).  temporal_accumulate takes prev as its aov, with a reprojection record whose motion is None."""
        n_rows = params.height if rows is None else rows.n_rows
        out = np.zeros((3, max(n_rows, 0), params.width, 4), np.float32)
        prev = np.zeros((2, max(n_rows, 0), params.width, 4), np.float32)
        _keep, mp = self._motion_table("render_aov_motion", motion)
        self._check(self._L.rt_render_aov_motion(self._h, C.byref(params), C.byref(pose) if pose is not None else None, C.byref(rows) if rows is not None else None,
                                                 mp, out.ctypes.data_as(C.POINTER(C.c_float)), prev.ctypes.data_as(C.POINTER(C.c_float))))
        return out, prev

    def render_aov_motion_device(self, params, out_ptr, prev_ptr, pose=None, rows=None, motion=None, stream=None):
        """rt_render_aov_motion_device: the three planes (3 * n_rows * W float4 at out_ptr) and the two previous-frame planes (2 * n_rows * W float4 at prev_ptr) into
        device memory, asynchronous on `stream`.  The motion table is copied by the call."""
        _keep, mp = self._motion_table("render_aov_motion_device", motion)
        self._check(self._L.rt_render_aov_motion_device(self._h, C.byref(params), C.byref(pose) if pose is not None else None, C.byref(self._rows_or_whole(params, rows)),
                                                        mp, C.c_void_p(out_ptr), C.c_void_p(prev_ptr), C.c_void_p(stream) if stream else None))

    def denoise(self, color, aov, n_passes=None, k_normal=None, k_position=None, k_albedo=None, k_color=None, out=None):
        """rt_denoise: the a-trous filter over color [H, W, 4] guided by aov [3, H, W, 4] (render_aov of the same frame) -> [H, W, 4].  Parameters as
        make_denoise_params.  out: optional preallocated result; it must not share memory with an input."""
        bad = f"denoise: color {np.shape(color)} must be [H, W, 4] and aov {np.shape(aov)} [3, H, W, 4] of the same frame"
        color = self._f32(color, lambda s: len(s) == 3 and s[2] == 4, bad)
        aov = self._f32(aov, lambda s: s == (3,) + color.shape, bad)
        out = self._out("denoise", out, color.shape)
        dp = make_denoise_params(n_passes, k_normal, k_position, k_albedo, k_color)
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_denoise(self._h, color.ctypes.data_as(fp), aov.ctypes.data_as(fp), color.shape[1], color.shape[0], C.byref(dp), out.ctypes.data_as(fp)))
        return out

    def denoise_device(self, color_ptr, aov_ptr, width, height, out_ptr, n_passes=None, k_normal=None, k_position=None, k_albedo=None, k_color=None, stream=None):
        """rt_denoise_device: device pointers (a frame of rt_render_device, the planes of render_aov_device, the result), asynchronous on `stream`."""
        dp = make_denoise_params(n_passes, k_normal, k_position, k_albedo, k_color)
        self._check(self._L.rt_denoise_device(self._h, C.c_void_p(color_ptr), C.c_void_p(aov_ptr), int(width), int(height), C.byref(dp), C.c_void_p(out_ptr),
                                              C.c_void_p(stream) if stream else None))

    # --- temporal accumulation and the variance-guided filter (rt_temporal_accumulate*, rt_denoise_var*)
    def temporal_accumulate(self, color, aov, prev_aov=None, prev_history=None, reproject=None, params=None, out=None):
        """rt_temporal_accumulate: color [H, W, 4] and aov [3 or 2, H, W, 4] of the current frame, prev_aov [>= 2, H, W, 4] and prev_history [2, H, W, 4] of the previous
        one (both None: the first frame), reproject = make_reproject(...), params = make_temporal_params(...) -> the new history [2, H, W, 4]: plane 0 colour | rays,
        plane 1 (m1, m2, history length, variance).  out: optional preallocated result; it must not share memory with an input."""
        bad = f"temporal_accumulate: color {np.shape(color)} must be [H, W, 4] and aov {np.shape(aov)} [3, H, W, 4] of the same frame"
        color = self._f32(color, lambda s: len(s) == 3 and s[2] == 4, bad)
        planes_ok = lambda s: len(s) == 4 and s[0] >= 2 and s[1:] == color.shape                     # two planes or more of this frame's size
        aov = self._f32(aov, planes_ok, bad)
        fp = C.POINTER(C.c_float)
        pa = ph = None
        if prev_aov is not None:
            prev_aov = self._f32(prev_aov, planes_ok, f"temporal_accumulate: prev_aov {np.shape(prev_aov)} must be [3, H, W, 4] of the same frame size")
            pa = prev_aov.ctypes.data_as(fp)
        if prev_history is not None:
            prev_history = self._f32(prev_history, lambda s: s == (2,) + color.shape,
                                     f"temporal_accumulate: prev_history {np.shape(prev_history)} must be [2, H, W, 4] of the same frame size")
            ph = prev_history.ctypes.data_as(fp)
        out = self._out("temporal_accumulate", out, (2,) + color.shape)
        tp = make_temporal_params() if params is None else params
        self._check(self._L.rt_temporal_accumulate(self._h, color.ctypes.data_as(fp), aov.ctypes.data_as(fp), pa, ph, color.shape[1], color.shape[0], C.byref(tp),
                                                   C.byref(reproject) if reproject is not None else None, out.ctypes.data_as(fp)))
        return out

    def temporal_accumulate_device(self, color_ptr, aov_ptr, prev_aov_ptr, prev_history_ptr, width, height, out_ptr, reproject=None, params=None, stream=None):
        """rt_temporal_accumulate_device: device pointers (0 / None for the previous pair = the first frame), asynchronous on `stream`."""
        tp = make_temporal_params() if params is None else params
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_temporal_accumulate_device(self._h, opt(color_ptr), opt(aov_ptr), opt(prev_aov_ptr), opt(prev_history_ptr), int(width), int(height), C.byref(tp),
                                                          C.byref(reproject) if reproject is not None else None, opt(out_ptr), C.c_void_p(stream) if stream else None))

    def _history_and_aov(self, name, history, aov):
        """the inputs of denoise_var and svgf_filter as float32 arrays: history [2, H, W, 4] and aov [3, H, W, 4] of the same frame"""
        bad = f"{name}: history {np.shape(history)} must be [2, H, W, 4] and aov {np.shape(aov)} [3, H, W, 4] of the same frame"
        history = self._f32(history, lambda s: len(s) == 4 and s[0] == 2 and s[3] == 4, bad)
        return history, self._f32(aov, lambda s: s == (3,) + history.shape[1:], bad)

    def denoise_var(self, history, aov, n_passes=None, k_normal=None, k_position=None, k_albedo=None, k_sigma=None, var_floor=None, out=None):
        """rt_denoise_var: the a-trous filter over history [2, H, W, 4] (temporal_accumulate's) guided by aov [3, H, W, 4], the colour term measured against the
        history's variance -> the filtered colour [H, W, 4].  Parameters as make_denoise_var_params."""
        history, aov = self._history_and_aov("denoise_var", history, aov)
        out = self._out("denoise_var", out, history.shape[1:])
        vp_ = make_denoise_var_params(n_passes, k_normal, k_position, k_albedo, k_sigma, var_floor)
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_denoise_var(self._h, history.ctypes.data_as(fp), aov.ctypes.data_as(fp), history.shape[2], history.shape[1], C.byref(vp_), out.ctypes.data_as(fp)))
        return out

    def denoise_var_device(self, history_ptr, aov_ptr, width, height, out_ptr, n_passes=None, k_normal=None, k_position=None, k_albedo=None, k_sigma=None, var_floor=None, stream=None):
        """rt_denoise_var_device: device pointers (a history of temporal_accumulate_device, the planes, the result), asynchronous on `stream`."""
        vp_ = make_denoise_var_params(n_passes, k_normal, k_position, k_albedo, k_sigma, var_floor)
        self._check(self._L.rt_denoise_var_device(self._h, C.c_void_p(history_ptr), C.c_void_p(aov_ptr), int(width), int(height), C.byref(vp_), C.c_void_p(out_ptr),
                                                  C.c_void_p(stream) if stream else None))

    def svgf_filter(self, history, aov, params=None, out=None, out_history=None):
        """rt_svgf_filter: denoise_var's inputs, params = make_svgf_params(...) -> (the filtered colour [H, W, 4], the history [2, H, W, 4] to hand the next
        temporal_accumulate as prev_history -- None when params.feedback_pass is -1).  out, out_history: optional preallocated results."""
        history, aov = self._history_and_aov("svgf_filter", history, aov)
        sp = make_svgf_params() if params is None else params
        out = self._out("svgf_filter", out, history.shape[1:])
        if sp.feedback_pass != -1 or out_history is not None:
            out_history = self._out("svgf_filter", out_history, history.shape)
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_svgf_filter(self._h, history.ctypes.data_as(fp), aov.ctypes.data_as(fp), history.shape[2], history.shape[1], C.byref(sp), out.ctypes.data_as(fp),
                                           out_history.ctypes.data_as(fp) if out_history is not None else None))
        return out, out_history

    def svgf_filter_device(self, history_ptr, aov_ptr, width, height, out_ptr, out_history_ptr=None, params=None, stream=None):
        """rt_svgf_filter_device: device pointers (a history of temporal_accumulate_device, the planes, the result, the fed-back history or 0 / None), asynchronous
        on `stream`."""
        sp = make_svgf_params() if params is None else params
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_svgf_filter_device(self._h, opt(history_ptr), opt(aov_ptr), int(width), int(height), C.byref(sp), opt(out_ptr), opt(out_history_ptr),
                                                  C.c_void_p(stream) if stream else None))

    # --- the fast history beside the long one, and the long one clamped to it (rt_temporal_accumulate_fast*, rt_history_rectify*)
    def temporal_accumulate_fast(self, color, aov, prev_aov=None, prev_history=None, prev_fast=None, reproject=None, params=None, fast_history=None, out=None, out_fast=None):
        """rt_temporal_accumulate_fast: temporal_accumulate's inputs and prev_fast [H, W, 4] (given exactly when prev_history is) -> (the history [2, H, W, 4], word for
        word temporal_accumulate's, and the fast plane [H, W, 4]: colour | fast history length, at most fast_history -- None: FAST_HISTORY_DEFAULT)."""
        bad = f"temporal_accumulate_fast: color {np.shape(color)} must be [H, W, 4] and aov {np.shape(aov)} [3, H, W, 4] of the same frame"
        color = self._f32(color, lambda s: len(s) == 3 and s[2] == 4, bad)
        planes_ok = lambda s: len(s) == 4 and s[0] >= 2 and s[1:] == color.shape
        aov = self._f32(aov, planes_ok, bad)
        fp = C.POINTER(C.c_float)
        given = []
        for name, a, ok in (("prev_aov", prev_aov, planes_ok), ("prev_history", prev_history, lambda s: s == (2,) + color.shape), ("prev_fast", prev_fast, lambda s: s == color.shape)):
            if a is not None:
                a = self._f32(a, ok, f"temporal_accumulate_fast: {name} {np.shape(a)} does not fit a frame of {color.shape}")
            given.append(a)
        out = self._out("temporal_accumulate_fast", out, (2,) + color.shape)
        out_fast = self._out("temporal_accumulate_fast", out_fast, color.shape)
        tp = make_temporal_params() if params is None else params
        self._check(self._L.rt_temporal_accumulate_fast(self._h, color.ctypes.data_as(fp), aov.ctypes.data_as(fp), *(None if a is None else a.ctypes.data_as(fp) for a in given),
                                                        color.shape[1], color.shape[0], C.byref(tp), C.byref(reproject) if reproject is not None else None,
                                                        FAST_HISTORY_DEFAULT if fast_history is None else int(fast_history), out.ctypes.data_as(fp), out_fast.ctypes.data_as(fp)))
        return out, out_fast

    def temporal_accumulate_fast_device(self, color_ptr, aov_ptr, prev_aov_ptr, prev_history_ptr, prev_fast_ptr, width, height, out_ptr, out_fast_ptr, reproject=None, params=None,
                                        fast_history=None, stream=None):
        """rt_temporal_accumulate_fast_device: device pointers (0 / None for the previous three = the first frame), asynchronous on `stream`."""
        tp = make_temporal_params() if params is None else params
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_temporal_accumulate_fast_device(self._h, opt(color_ptr), opt(aov_ptr), opt(prev_aov_ptr), opt(prev_history_ptr), opt(prev_fast_ptr), int(width),
                                                               int(height), C.byref(tp), C.byref(reproject) if reproject is not None else None,
                                                               FAST_HISTORY_DEFAULT if fast_history is None else int(fast_history), opt(out_ptr), opt(out_fast_ptr),
                                                               C.c_void_p(stream) if stream else None))

    def history_rectify(self, history, fast, aov, params=None, out=None):
        """rt_history_rectify: history [2, H, W, 4] and fast [H, W, 4] of temporal_accumulate_fast, aov [>= 1, H, W, 4] (plane 0 is read), params =
        make_rectify_params(...) -> the rectified history [2, H, W, 4].  out: optional preallocated result; it may be `history` itself (in place)."""
        bad = f"history_rectify: history {np.shape(history)} must be [2, H, W, 4], fast {np.shape(fast)} [H, W, 4] and aov {np.shape(aov)} [1 or more, H, W, 4] of the same frame"
        history = self._f32(history, lambda s: len(s) == 4 and s[0] == 2 and s[3] == 4, bad)
        fast = self._f32(fast, lambda s: s == history.shape[1:], bad)
        aov = self._f32(aov, lambda s: len(s) == 4 and s[0] >= 1 and s[1:] == history.shape[1:], bad)
        out = self._out("history_rectify", out, history.shape)
        rp = make_rectify_params() if params is None else params
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_history_rectify(self._h, history.ctypes.data_as(fp), fast.ctypes.data_as(fp), aov.ctypes.data_as(fp), history.shape[2], history.shape[1],
                                               C.byref(rp), out.ctypes.data_as(fp)))
        return out

    def history_rectify_device(self, history_ptr, fast_ptr, aov_ptr, width, height, out_ptr, params=None, stream=None):
        """rt_history_rectify_device: device pointers (out_ptr == history_ptr: in place), asynchronous on `stream`."""
        rp = make_rectify_params() if params is None else params
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_history_rectify_device(self._h, opt(history_ptr), opt(fast_ptr), opt(aov_ptr), int(width), int(height), C.byref(rp), opt(out_ptr),
                                                      C.c_void_p(stream) if stream else None))

    # --- the planes of the first diffuse surface, and the albedo divided out of / multiplied into a frame (rt_render_aov_surface*, rt_demodulate*, rt_modulate*)
    def render_aov_surface(self, params, max_specular, pose=None, rows=None):
        """rt_render_aov_surface: the planes of render_aov for the first DIFFUSE surface of each pixel, reached through at most max_specular mirror / glass
        segments -> [3, n_rows, W, 4] float32: plane 0 (normal, path code or -1: see decode_path), plane 1 (hit point, 1 / 0), plane 2 (albedo, 1 where the chain
        ended on a diffuse surface -- the albedo factors out of the pixel there -- else 0)."""
        n_rows = params.height if rows is None else rows.n_rows
        out = np.zeros((3, max(n_rows, 0), params.width, 4), np.float32)
        self._check(self._L.rt_render_aov_surface(self._h, C.byref(params), C.byref(pose) if pose is not None else None, C.byref(rows) if rows is not None else None,
                                                  int(max_specular), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_aov_surface_device(self, params, max_specular, out_ptr, pose=None, rows=None, stream=None):
        """rt_render_aov_surface_device: the same three planes into device memory (3 * n_rows * W float4), asynchronous on `stream`."""
        self._check(self._L.rt_render_aov_surface_device(self._h, C.byref(params), C.byref(pose) if pose is not None else None, C.byref(self._rows_or_whole(params, rows)),
                                                         int(max_specular), C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    @staticmethod
    def decode_path(code):
        """The path code of plane 0 .w of render_aov_surface -> (id, first_id, k): the recorded object, the camera ray's first hit, the specular segments between
        them (k == 0: first_id is id itself).  A miss (-1) -> (-1, -1, 0).  Arrays decode elementwise."""
        c = np.asarray(code).astype(np.int64)
        miss = c < 0
        k = np.where(miss, 0, c // 256)
        ident = np.where(miss, -1, c % 16)
        first = np.where(miss, -1, np.where(k == 0, ident, (c // 16) % 16))
        if np.ndim(code) == 0:
            return int(ident), int(first), int(k)
        return ident, first, k

    def _modulate(self, name, color, aov, albedo_floor, out):
        bad = f"{name}: color {np.shape(color)} must be [..., 4] and aov {np.shape(aov)} [3, ..., 4] of the same frame"
        color = self._f32(color, lambda s: len(s) >= 1 and s[-1] == 4, bad)
        aov = self._f32(aov, lambda s: s == (3,) + color.shape, bad)
        out = self._out(name, out, color.shape)
        fp = C.POINTER(C.c_float)
        self._check(getattr(self._L, "rt_" + name)(self._h, color.ctypes.data_as(fp), aov.ctypes.data_as(fp), color.size // 4, float(albedo_floor), out.ctypes.data_as(fp)))
        return out

    def demodulate(self, color, aov, albedo_floor=0.0, out=None):
        """rt_demodulate: color [H, W, 4] with the albedo of aov [3, H, W, 4] plane 2 divided out where its .w is 1 (the planes of render_aov_surface; those of
        render_aov make it the identity) -> [H, W, 4].  A channel whose max(albedo, albedo_floor) is not > 0 passes through.  out may be color itself."""
        return self._modulate("demodulate", color, aov, albedo_floor, out)

    def modulate(self, color, aov, albedo_floor=0.0, out=None):
        """rt_modulate: the inverse of demodulate with the same planes and floor: the albedo multiplied back in."""
        return self._modulate("modulate", color, aov, albedo_floor, out)

    def demodulate_device(self, color_ptr, aov_ptr, n_pixels, out_ptr, albedo_floor=0.0, stream=None):
        """rt_demodulate_device: device pointers (a frame, three planes of n_pixels float4, the result -- color_ptr itself or disjoint), asynchronous on `stream`."""
        self._check(self._L.rt_demodulate_device(self._h, C.c_void_p(color_ptr), C.c_void_p(aov_ptr), int(n_pixels), float(albedo_floor), C.c_void_p(out_ptr),
                                                 C.c_void_p(stream) if stream else None))

    def modulate_device(self, color_ptr, aov_ptr, n_pixels, out_ptr, albedo_floor=0.0, stream=None):
        """rt_modulate_device: as demodulate_device, multiplying."""
        self._check(self._L.rt_modulate_device(self._h, C.c_void_p(color_ptr), C.c_void_p(aov_ptr), int(n_pixels), float(albedo_floor), C.c_void_p(out_ptr),
                                               C.c_void_p(stream) if stream else None))

    # --- guided upsampling of a frame or a history traced at 1 / factor of the resolution (rt_upsample*)
    def upsample(self, low, low_aov, aov, factor, k_normal=None, k_position=None, out=None):
        """rt_upsample: low [h, w, 4] (a colour frame) or [2, h, w, 4] (a history of temporal_accumulate), low_aov [3, h, w, 4] and aov [3, factor h, factor w, 4]
        (render_aov at both resolutions) -> the frame [H, W, 4] or the history [2, H, W, 4] at full resolution.  Parameters as make_upsample_params."""
        bad = (f"upsample: low {np.shape(low)} must be [h, w, 4] or [2, h, w, 4], low_aov {np.shape(low_aov)} [3, h, w, 4] and aov {np.shape(aov)} "
               f"[3, {factor} h, {factor} w, 4]")
        low = self._f32(low, lambda s: len(s) in (3, 4) and s[-1] == 4 and (len(s) == 3 or s[0] == 2), bad)
        n_planes, (h, w) = (1 if low.ndim == 3 else 2), low.shape[-3:-1]
        low_aov = self._f32(low_aov, lambda s: s == (3, h, w, 4), bad)
        aov = self._f32(aov, lambda s: s == (3, h * int(factor), w * int(factor), 4), bad)
        out = self._out("upsample", out, low.shape[:-3] + aov.shape[1:])
        up = make_upsample_params(factor, n_planes, k_normal, k_position)
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_upsample(self._h, low.ctypes.data_as(fp), low_aov.ctypes.data_as(fp), aov.ctypes.data_as(fp), aov.shape[2], aov.shape[1], C.byref(up),
                                        out.ctypes.data_as(fp)))
        return out

    def upsample_device(self, low_ptr, low_aov_ptr, aov_ptr, width, height, factor, out_ptr, n_planes=1, k_normal=None, k_position=None, stream=None):
        """rt_upsample_device: device pointers (n_planes planes at (width / factor) x (height / factor), the planes at that and at the full resolution, the
        n_planes full-resolution planes of the result), asynchronous on `stream`.  width, height: the FULL resolution."""
        up = make_upsample_params(factor, n_planes, k_normal, k_position)
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_upsample_device(self._h, opt(low_ptr), opt(low_aov_ptr), opt(aov_ptr), int(width), int(height), C.byref(up), opt(out_ptr),
                                               C.c_void_p(stream) if stream else None))

    # --- adaptive sampling: per-pixel sample counts traced as a compacted list, and counts from a history (rt_render_counts*, rt_sample_counts*)
    @staticmethod
    def _u8(name, a, shape):
        a = np.ascontiguousarray(a)
        if a.dtype != np.uint8 or a.shape != shape:
            raise RtError(-1, f"{name}: counts {a.shape} {a.dtype} must be a uint8 array of shape {shape}")
        return a

    def render_counts(self, params, counts, pose=None, base=None, out=None):
        """rt_render_counts: counts [H, W] uint8 -> the frame [H, W, 4] float32 whose pixel (x, y) is that of a frame with num_rays = counts[y, x] (0: zeros; above
        MAX_SAMPLE_COUNT: MAX_SAMPLE_COUNT).  base: the one-sample frame of the same params, pose and scene (pixels with a count <= 1 are copied from it, the others
        trace samples 1 ..); out: optional preallocated result, which may be `base`.  params.num_rays is not read."""
        shape = (params.height, params.width)
        counts = self._u8("render_counts", counts, shape)
        if base is not None:
            base = self._f32(base, lambda s: s == shape + (4,), f"render_counts: base {np.shape(base)} must be {shape + (4,)}")
        out = self._out("render_counts", out, shape + (4,))
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_render_counts(self._h, C.byref(params), C.byref(pose) if pose is not None else None, counts.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             base.ctypes.data_as(fp) if base is not None else None, out.ctypes.data_as(fp)))
        return out

    def render_counts_device(self, params, counts_ptr, out_ptr, pose=None, base_ptr=None, stream=None):
        """rt_render_counts_device: device pointers (counts: H * W bytes; base_ptr == out_ptr: in place).  Waits on `stream` once (the list's length comes back to
        the host), the rest is asynchronous."""
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_render_counts_device(self._h, C.byref(params), C.byref(pose) if pose is not None else None, opt(counts_ptr), opt(base_ptr), opt(out_ptr),
                                                    C.c_void_p(stream) if stream else None))

    def render_counts_info(self):
        """rt_render_counts_info: of the last render_counts* call -> dict(items, chains, slots, chain_paths)."""
        out = (C.c_uint64 * 4)()
        self._check(self._L.rt_render_counts_info(self._h, out))
        return dict(items=int(out[0]), chains=int(out[1]), slots=int(out[2]), chain_paths=int(out[3]))

    def sample_counts(self, history, params=None):
        """rt_sample_counts: history [2, H, W, 4] of temporal_accumulate (plane 1 is read), params = make_sample_count_params(...) -> counts [H, W] uint8."""
        history = self._f32(history, lambda s: len(s) == 4 and s[0] == 2 and s[3] == 4, f"sample_counts: history {np.shape(history)} must be [2, H, W, 4]")
        cp = make_sample_count_params() if params is None else params
        out = np.zeros(history.shape[1:3], np.uint8)
        self._check(self._L.rt_sample_counts(self._h, history.ctypes.data_as(C.POINTER(C.c_float)), history.shape[2], history.shape[1], C.byref(cp),
                                             out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def sample_counts_device(self, history_ptr, width, height, counts_ptr, params=None, stream=None):
        """rt_sample_counts_device: device pointers (history: two planes; counts: H * W bytes), asynchronous on `stream`."""
        cp = make_sample_count_params() if params is None else params
        opt = lambda p: C.c_void_p(p) if p else None
        self._check(self._L.rt_sample_counts_device(self._h, opt(history_ptr), int(width), int(height), C.byref(cp), opt(counts_ptr), C.c_void_p(stream) if stream else None))

    def kat_sample_plan(self, counts, first_sample=0):
        """rt_kat_sample_plan: counts [H, W] uint8 -> (offs [slots + 1] uint32 in pixel-slot order, items [n, 3] int32 of (x, y, sample), span (slots per workgroup,
        slots per round of the scan of workgroup sums))."""
        counts = np.ascontiguousarray(counts)
        if counts.dtype != np.uint8 or counts.ndim != 2:
            raise RtError(-1, f"kat_sample_plan: counts {counts.shape} {counts.dtype} must be a [H, W] uint8 array")
        H, W = counts.shape
        slots = ((W + 7) // 8) * ((H + 7) // 8) * 64
        n_max = int(np.maximum(np.minimum(counts, MAX_SAMPLE_COUNT).astype(np.int64) - int(first_sample), 0).sum())
        offs, items = np.zeros(slots + 1, np.uint32), np.zeros((n_max, 3), np.int32)
        n, span = C.c_uint64(), (C.c_int32 * 2)()
        cp = counts.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self._L.rt_kat_sample_plan(self._h, cp, W, H, int(first_sample), None, None, C.byref(n), None))   # the length first: `items` is sized from the counts
        if n.value != n_max:
            raise RtError(-6, f"kat_sample_plan: the plan holds {n.value} items, the counts {n_max}")
        self._check(self._L.rt_kat_sample_plan(self._h, cp, W, H, int(first_sample), offs.ctypes.data_as(C.POINTER(C.c_uint32)), items.ctypes.data_as(C.POINTER(C.c_int32)),
                                               C.byref(n), span))
        return offs, items, (int(span[0]), int(span[1]))

    def render_pose(self, params, pose):
        """One frame with realtime_render.cu's posed camera and per-sample averaging (no accumulation)."""
        out = np.empty((params.height, params.width, 4), np.float32)
        self._check(self._L.rt_render_pose(self._h, C.byref(params), C.byref(pose), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_pose_device(self, params, pose, out_ptr, rows=None, stream=None):
        """rt_render_pose_device: render_pose's frame into device memory (rows: a Rows, None = the whole frame), asynchronous on `stream`."""
        self._check(self._L.rt_render_pose_device(self._h, C.byref(params), C.byref(pose), C.byref(self._rows_or_whole(params, rows)), C.c_void_p(out_ptr),
                                                  C.c_void_p(stream) if stream else None))

    def device_alloc(self, n_bytes):
        """rt_device_alloc: n_bytes of memory on the context's device -> its address (free it with device_free)."""
        p = C.c_void_p()
        self._check(self._L.rt_device_alloc(self._h, C.byref(p), int(n_bytes)))
        return p.value

    def device_free(self, ptr):
        if ptr:
            self._check(self._L.rt_device_free(C.c_void_p(ptr)))

    def device_to_host(self, ptr, shape):
        """rt_device_to_host: float32 device memory -> a new array of `shape`, after everything on the context's own stream."""
        out = np.empty(shape, np.float32)
        self._check(self._L.rt_device_to_host(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
        return out

    def progressive_reset(self):
        self._check(self._L.rt_progressive_reset(self._h))

    def progressive_frame(self, params, pose):
        """frames++, render with seed WangHash(frames), accumulate; returns (display float4, rgb8)."""
        disp = np.empty((params.height, params.width, 4), np.float32)
        rgb8 = np.empty((params.height, params.width, 3), np.uint8)
        self._check(self._L.rt_progressive_frame(self._h, C.byref(params), C.byref(pose), disp.ctypes.data_as(C.POINTER(C.c_float)),
                                                 rgb8.ctypes.data_as(C.POINTER(C.c_uint8))))
        return disp, rgb8

    def progressive_frames(self):
        n = C.c_int(0)
        self._check(self._L.rt_progressive_frames(self._h, C.byref(n)))
        return n.value

    def kat_progressive(self, accum, frame, framenumber):
        """rt_kat_progressive: the progressive kernel on explicit values, accum and frame [n, 4] float32 -> (accum + frame [n, 4], display [n, 4], rgb8 [n, 3]);
        the context's own progressive state is not touched"""
        a = np.ascontiguousarray(accum, np.float32).reshape(-1, 4)
        f = np.ascontiguousarray(frame, np.float32).reshape(-1, 4)
        if a.shape != f.shape:
            raise ValueError(f"accum {a.shape} and frame {f.shape} differ")
        acc, disp, rgb8 = np.empty_like(a), np.empty_like(a), np.empty((len(a), 3), np.uint8)
        fp = C.POINTER(C.c_float)
        self._check(self._L.rt_kat_progressive(self._h, a.ctypes.data_as(fp), f.ctypes.data_as(fp), len(a), int(framenumber), acc.ctypes.data_as(fp),
                                               disp.ctypes.data_as(fp), rgb8.ctypes.data_as(C.POINTER(C.c_uint8))))
        return acc, disp, rgb8

    def synchronize(self):
        self._check(self._L.rt_synchronize(self._h))

    def selfcheck(self):
        """Every device buffer of the context lives on the context's device."""
        self._check(self._L.rt_ctx_selfcheck(self._h))

    def _kat(self, fn, rows, width, owidth, *extra, counts=True):
        a = np.ascontiguousarray(rows, np.float32).reshape(-1, width)
        out = np.zeros((len(a), owidth), np.float32)
        c = KatCounts()
        fp = C.POINTER(C.c_float)
        args = [self._h, a.ctypes.data_as(fp), len(a), *extra, out.ctypes.data_as(fp)] + ([C.byref(c)] if counts else [])
        self._check(fn(*args))
        return out, {k: int(getattr(c, k)) for k, _ in KatCounts._fields_}

    def kat_sphere(self, rows):
        return self._kat(self._L.rt_kat_sphere, rows, 10, 5, counts=False)[0]

    def kat_sqrt(self, x):
        return self._kat(self._L.rt_kat_sqrt, x, 1, 1, counts=False)[0][:, 0]

    def kat_box(self, rows, route):
        out, c = self._kat(self._L.rt_kat_box, rows, 12, 1, int(route))
        return out[:, 0], c

    def kat_triangle(self, rows):
        return self._kat(self._L.rt_kat_triangle, rows, 15, 5)

    def kat_mesh(self, rows, tri_tmin=1e-4, route=0):
        return self._kat(self._L.rt_kat_mesh, rows, 6, 5, C.c_float(tri_tmin), int(route))

    def layout_hash(self):
        """rt_kat_layout_hash -> dict(pairs, fixed_pairs, quads, leaf_boxes) of 64-bit hashes (0 = that layout is not in use)."""
        h = (C.c_uint64 * 4)()
        self._check(self._L.rt_kat_layout_hash(self._h, h))
        return dict(zip(("pairs", "fixed_pairs", "quads", "leaf_boxes"), (int(x) for x in h)))

    def stats_after_render(self, params):
        """Render one frame with `params` and return rt_get_stats of it (which traversal kernel ran: travq_mode)."""
        self.render(params)
        return self.stats()

    def stats(self):
        s = Stats()
        self._check(self._L.rt_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}


class MultiContext:
    """One host process, several devices (rt_multi_*): interleaved 8-row tiles, peer copies to device_ids[0]."""

    def __init__(self, device_ids):
        self._L = load()
        self._h = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*device_ids)
        rc = self._L.rt_multi_create(C.byref(self._h), ids, len(device_ids))
        if rc != RT_OK:
            raise RtError(rc, self._L.rt_multi_last_error(None).decode())
        self._keep = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.rt_multi_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _check(self, rc):
        if rc != RT_OK:
            raise RtError(rc, self._L.rt_multi_last_error(self._h).decode())

    def scene_upload(self, spheres, mesh=None, light=((-10.0, 20.0, 40.0), 3e10), camera=((0.0, 0.0, 55.0), None)):
        arr, n, marr, nm, lt, cam, self._keep = _marshal_scene(spheres, mesh, light, camera)
        if nm <= 1 and not isinstance(mesh, (list, tuple)):
            self._check(self._L.rt_multi_scene_upload(self._h, arr, n, marr if nm else None, C.byref(lt), C.byref(cam)))
        else:
            self._check(self._L.rt_multi_scene_upload_meshes(self._h, arr, n, marr, nm, C.byref(lt), C.byref(cam)))

    def render(self, params):
        out = np.empty((params.height, params.width, 4), np.float32)
        self._check(self._L.rt_render_multi(self._h, C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_device(self, params, out_ptr):
        self._check(self._L.rt_render_multi_device(self._h, C.byref(params), C.c_void_p(out_ptr)))

    def render_rgb8(self, params):
        """Every device tonemaps its tiles; the exchange moves the 8-bit image (3 bytes per pixel)."""
        out = np.empty((params.height, params.width, 3), np.uint8)
        self._check(self._L.rt_render_multi_rgb8(self._h, C.byref(params), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def stats(self):
        s = MultiStats()
        self._check(self._L.rt_multi_get_stats(self._h, C.byref(s)))
        n = s.n_devices
        return {"n_devices": n, "device_id": list(s.device_id)[:n], "kernel_ms": list(s.kernel_ms)[:n],
                "gather_ms": s.gather_ms, "frame_ms": s.frame_ms, "rays": int(s.rays), "gather_bytes": int(s.gather_bytes),
                "peer_access": list(s.peer_access)[:n], "submit_ms": s.submit_ms}
