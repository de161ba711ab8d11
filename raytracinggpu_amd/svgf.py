"""SvgfSequence: the per-frame denoising chain and the buffers it swaps, over the device entry points of a Context.

render -> render_aov_device -> temporal_accumulate_device -> svgf_filter_device on one stream.  The accumulation of frame t takes as its previous history what the
filter of frame t - 1 fed back (svgf_filter's out_history; the accumulated history itself when the parameters feed nothing back), and the planes of frame t - 1."""
from ._capi import CameraPose, RtError, make_reproject, make_svgf_params, make_temporal_params


class SvgfSequence:
    """Owns two histories (the accumulated one and the one handed on), two sets of planes, a colour frame and an output, all from the context's device allocator.

    ctx: a Context with its scene uploaded.  svgf = make_svgf_params(...), temporal = make_temporal_params(...) (None: the defaults).  camera: the fixed camera
    (position, fov) the scene was uploaded with, for frames without a pose (None: scene_upload's default).  stream: the stream of every call (None: the context's)."""

    def __init__(self, ctx, width, height, svgf=None, temporal=None, camera=None, stream=None):
        self.ctx, self.width, self.height, self.stream = ctx, int(width), int(height), stream
        self.svgf = make_svgf_params() if svgf is None else svgf
        self.temporal = make_temporal_params() if temporal is None else temporal
        self.camera = camera
        frame = self.width * self.height * 16
        self._ptrs = []
        try:
            self.color, self.out, self.accumulated, self.history, *self.planes = (self._alloc(n * frame) for n in (1, 1, 2, 2, 3, 3))
        except RtError:
            self.close()
            raise
        self._have_previous = False
        self._previous_pose = None

    def _alloc(self, n_bytes):
        self._ptrs.append(self.ctx.device_alloc(n_bytes))
        return self._ptrs[-1]

    def frame(self, params, pose=None, motion=None, no_history_mask=0, cut=False):
        """One frame of the chain -> the device address of the filtered frame (self.out: width x height float4, valid until the next call; asynchronous on the
        stream).  params: the frame's render parameters (a new seed per frame); pose: its CameraPose (None: the uploaded camera); motion: the table "previous from
        current" of what moved since the previous frame (None: nothing); cut=True, and the first call, use no previous frame."""
        if (params.width, params.height) != (self.width, self.height):
            raise RtError(-1, f"SvgfSequence.frame: params are {params.width} x {params.height}, the sequence {self.width} x {self.height}")
        c, s, W, H = self.ctx, self.stream, self.width, self.height
        planes, previous = self.planes
        if pose is not None:
            c.render_pose_device(params, pose, self.color, stream=s)
        else:
            c.render_device(params, c._rows_or_whole(params, None), self.color, stream=s)
        c.render_aov_device(params, planes, pose=pose, stream=s)
        if cut or not self._have_previous:
            c.temporal_accumulate_device(self.color, planes, None, None, W, H, self.accumulated, params=self.temporal, stream=s)
        else:
            rp = make_reproject(camera=self.camera, pose=self._previous_pose, motion=motion, no_history_mask=no_history_mask)
            c.temporal_accumulate_device(self.color, planes, previous, self.history, W, H, self.accumulated, reproject=rp, params=self.temporal, stream=s)
        if self.svgf.feedback_pass >= 0:
            c.svgf_filter_device(self.accumulated, planes, W, H, self.out, self.history, params=self.svgf, stream=s)
        else:                                                          # nothing is fed back: the accumulated history is the one handed on
            c.svgf_filter_device(self.accumulated, planes, W, H, self.out, None, params=self.svgf, stream=s)
            self.accumulated, self.history = self.history, self.accumulated
        self.planes = [previous, planes]
        self._have_previous = True
        self._previous_pose = None if pose is None else CameraPose.from_buffer_copy(pose)
        return self.out

    def close(self):
        """Frees the buffers (after the context's work: the caller synchronises its own stream first)."""
        ptrs, self._ptrs = self._ptrs, []
        for p in ptrs:
            self.ctx.device_free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
