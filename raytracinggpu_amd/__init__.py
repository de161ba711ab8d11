"""raytracinggpu_amd -- MI355X-native render path for souhhcong/RaytracingGPU.

The product is libraytrace_hip.so (hand-written HIP for gfx950 behind the C-ABI of
include/raytrace_hip.h) plus the C++ host API of include/raytracer.hpp.  This
Python package is plumbing for tests and bench.py: a ctypes binding and the scene
presets of the reference programs.
"""
from . import _capi, environment, scenes  # noqa: F401  (tiling imports torch: import it explicitly where needed)
from ._capi import FAST_HISTORY_DEFAULT, MAX_SAMPLE_COUNT, RECTIFY_DEFAULTS, SAMPLE_COUNT_DEFAULTS, UPSAMPLE_DEFAULTS, Context, MultiContext, PinnedArray, RectifyParams, RtError, SampleCountParams, UpsampleParams, camera_basis, device_count, interleaved_rows, light_orbit, make_denoise_params, make_denoise_var_params, make_params, make_pose, make_rectify_params, make_reproject, make_sample_count_params, make_svgf_params, make_temporal_params, make_upsample_params, motion_from_mesh_transform, motion_from_spheres, static_motion  # noqa: F401
from .svgf import SvgfSequence  # noqa: F401
