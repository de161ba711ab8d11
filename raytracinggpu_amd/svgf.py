"""SvgfSequence: the per-frame denoising chain and the buffers it swaps, over the device entry points of a Context.

render -> render_aov_device -> temporal_accumulate_device -> svgf_filter_device on one stream.  The accumulation of frame t takes as its previous history what the
filter of frame t - 1 fed back (svgf_filter's out_history; the accumulated history itself when the parameters feed nothing back), and the planes of frame t - 1.

upsample = f in 2 .. 4 (off by default: a speed knob that costs quality) traces and accumulates at 1 / f of the resolution and rebuilds the
full-resolution frame with upsample_device, guided by full-resolution planes rendered once per frame:
  filter_at="low"  (pipeline A)  the whole chain at the low resolution, then the filtered frame is upsampled;
  filter_at="full" (pipeline B)  the accumulated history is upsampled (both planes) and svgf_filter_device runs at full resolution.
History, previous planes, reprojection, motion tables and cut all stay at the low resolution, as without the option.

rectify = make_rectify_params(...) (off by default) keeps a fast history beside the long one (temporal_accumulate_fast_device) and clamps the accumulated history to it
in place (history_rectify_device) before the filter, or before the upsample of pipeline B: the chain then follows a light or a shadow that moves (DESIGN.md section
5.12).  The fast plane lives at the low resolution with the rest of the state.

adaptive = make_sample_count_params(...) (off by default; only at upsample == 1) spends more samples where the history says the frame is bad: after the accumulation
sample_counts_device turns the accumulated history into per-pixel counts, render_counts_device adds the missing samples to the colour frame in place (base = the
one-sample frame), and the accumulation runs again from the same previous history into the same buffer; then the chain goes on as without the option (DESIGN.md
section 5.13).  render_counts_device waits on the stream once per frame.

deforming = True (off by default) follows meshes that change shape (mesh_set_vertices) as well as rigid motion: render_aov_motion_device takes render_aov_device's
place and also writes the PREVIOUS-FRAME planes -- where each pixel's surface point and normal were a frame ago, by the vertex snapshot of a deforming mesh
(the caller's mesh_snapshot_vertices, once per frame before its edits) or by the motion table -- and the accumulation reprojects from those with a record whose
motion is None.  Everything else (the clamp, the filter, the upsample, the sample counts) keeps taking the current planes."""
from ._capi import FAST_HISTORY_DEFAULT, CameraPose, Params, RtError, make_reproject, make_svgf_params, make_temporal_params


class SvgfSequence:
    """Owns two histories (the accumulated one and the one handed on), two sets of planes, a colour frame and an output, all from the context's device allocator;
    with upsample > 1 those are at the low resolution, and the full-resolution planes and the frame (A) or history (B) between the two resolutions come on top.

    ctx: a Context with its scene uploaded.  svgf = make_svgf_params(...), temporal = make_temporal_params(...) (None: the defaults).  camera: the fixed camera
    (position, fov) the scene was uploaded with, for frames without a pose (None: scene_upload's default).  stream: the stream of every call (None: the context's).
    upsample, filter_at: see the module; up_k_normal, up_k_position: the upsample's weights (None: UPSAMPLE_DEFAULTS).  rectify: None, or the RectifyParams of the
    clamp (the sequence then owns two fast planes more and swaps them); fast_history: the fast history's length limit.  adaptive: None, or the SampleCountParams of
    the per-pixel sample counts (the sequence then owns a plane of counts, one byte per pixel).  deforming: the accumulation reprojects from previous-frame planes
    (the sequence then owns two planes more at the working resolution); motion= of frame() then goes to render_aov_motion_device.

    The per-frame recipe of a deforming sequence with a SMOOTH mesh, all on the context: ctx.mesh_snapshot_vertices(); ctx.mesh_snapshot_normals(); the frame's edits
    (ctx.mesh_set_vertices(...), ctx.mesh_transform(...)); ctx.mesh_compute_normals() (or mesh_set_normals with the caller's own); then frame(...).  The sequence
    itself issues no other call for it: render_aov_motion_device honours the context's normal-snapshot mask, and N' of the smooth mesh is the normal the previous
    frame shaded with instead of the current one (without the snapshot min_normal_dot throws the history away wherever the surface turned).
    A flat mesh needs the vertex snapshot alone."""

    def __init__(self, ctx, width, height, svgf=None, temporal=None, camera=None, stream=None, upsample=1, filter_at="low", up_k_normal=None, up_k_position=None,
                 rectify=None, fast_history=FAST_HISTORY_DEFAULT, adaptive=None, deforming=False):
        self.ctx, self.width, self.height, self.stream = ctx, int(width), int(height), stream
        self.svgf = make_svgf_params() if svgf is None else svgf
        self.temporal = make_temporal_params() if temporal is None else temporal
        self.camera = camera
        self.upsample, self.filter_at, self.up_k = int(upsample), filter_at, (up_k_normal, up_k_position)
        self.rectify, self.fast_history = rectify, int(fast_history)
        self.adaptive = adaptive
        self.deforming = bool(deforming)
        f = self.upsample
        if f < 1 or f > 4 or filter_at not in ("low", "full"):
            raise RtError(-1, f"SvgfSequence: upsample {upsample} must be 1 .. 4 and filter_at {filter_at!r} 'low' or 'full'")
        if self.width % f or self.height % f:
            raise RtError(-1, f"SvgfSequence: {self.width} x {self.height} is no multiple of upsample {f}")
        if adaptive is not None and f != 1:
            raise RtError(-1, f"SvgfSequence: adaptive sampling runs at upsample == 1 only (upsample = {f})")
        if f > 1 and filter_at == "full" and self.svgf.feedback_pass >= 0:
            raise RtError(-1, "SvgfSequence: filter_at='full' filters an upsampled history, which is never fed back: feedback_pass must be -1")
        self.low_width, self.low_height = self.width // f, self.height // f
        frame, full = self.low_width * self.low_height * 16, self.width * self.height * 16
        self._ptrs = []
        try:
            self.color, self.accumulated, self.history, *self.planes = (self._alloc(n * frame) for n in (1, 2, 2, 3, 3))
            self.out = self._alloc(full)
            if f > 1:
                self.full_planes = self._alloc(3 * full)
                self.between = self._alloc(frame if filter_at == "low" else 2 * full)   # A: the filtered low-resolution frame; B: the upsampled history
            if rectify is not None:
                self.fast, self.previous_fast = self._alloc(frame), self._alloc(frame)
            if adaptive is not None:
                self.counts = self._alloc(self.width * self.height)
            if self.deforming:
                self.previous_frame_planes = self._alloc(2 * frame)
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
        stream).  params: the frame's render parameters at the FULL resolution (a new seed per frame; with upsample > 1 the low-resolution ones are these with the
        size divided); pose: its CameraPose (None: the uploaded camera); motion: the table "previous from current" of what moved since the previous frame (None:
        nothing); cut=True, and the first call, use no previous frame."""
        if (params.width, params.height) != (self.width, self.height):
            raise RtError(-1, f"SvgfSequence.frame: params are {params.width} x {params.height}, the sequence {self.width} x {self.height}")
        c, s, W, H, f = self.ctx, self.stream, self.low_width, self.low_height, self.upsample
        full = params
        if f > 1:
            params = Params.from_buffer_copy(full)
            params.width, params.height = W, H
        planes, previous = self.planes
        if pose is not None:
            c.render_pose_device(params, pose, self.color, stream=s)
        else:
            c.render_device(params, c._rows_or_whole(params, None), self.color, stream=s)
        source = planes                                                # the planes the accumulation reprojects from
        if self.deforming:                                             # ... are the previous-frame planes: the motion is in them, the record carries none
            source = self.previous_frame_planes
            c.render_aov_motion_device(params, planes, source, pose=pose, motion=motion, stream=s)
            motion = None
        else:
            c.render_aov_device(params, planes, pose=pose, stream=s)
        first = cut or not self._have_previous
        rp = None if first else make_reproject(camera=self.camera, pose=self._previous_pose, motion=motion, no_history_mask=no_history_mask)
        self._accumulate(source, planes, previous, first, rp, W, H)
        if self.adaptive is not None:                                  # more samples where the history asks for them, then the accumulation over again
            c.sample_counts_device(self.accumulated, W, H, self.counts, params=self.adaptive, stream=s)
            c.render_counts_device(params, self.counts, self.color, pose=pose, base_ptr=self.color, stream=s)
            self._accumulate(source, planes, previous, first, rp, W, H)
        if self.rectify is not None:
            self.fast, self.previous_fast = self.previous_fast, self.fast
        return self._filter(full, planes, previous, pose)

    def _accumulate(self, source, planes, previous, first, rp, W, H):
        """the accumulation of the colour frame into self.accumulated (and self.fast), with the clamp if the sequence has one.  source: the planes it reprojects from
        (the current planes, or the previous-frame planes of a deforming sequence); planes: the current ones, which the clamp keeps taking"""
        c, s = self.ctx, self.stream
        if self.rectify is None and first:
            c.temporal_accumulate_device(self.color, source, None, None, W, H, self.accumulated, params=self.temporal, stream=s)
        elif self.rectify is None:
            c.temporal_accumulate_device(self.color, source, previous, self.history, W, H, self.accumulated, reproject=rp, params=self.temporal, stream=s)
        else:                                                          # the fast history beside the long one, then the long one clamped to it, in place
            c.temporal_accumulate_fast_device(self.color, source, None if first else previous, None if first else self.history, None if first else self.previous_fast, W, H,
                                              self.accumulated, self.fast, reproject=rp, params=self.temporal, fast_history=self.fast_history, stream=s)
            c.history_rectify_device(self.accumulated, self.fast, planes, W, H, self.accumulated, params=self.rectify, stream=s)

    def _filter(self, full, planes, previous, pose):
        """the rest of the frame: the upsample's planes, the filter, the swaps"""
        c, s, W, H, f = self.ctx, self.stream, self.low_width, self.low_height, self.upsample
        if f > 1:
            c.render_aov_device(full, self.full_planes, pose=pose, stream=s)
        if f > 1 and self.filter_at == "full":                         # B: the history goes up, the filter runs on it at full resolution
            c.upsample_device(self.accumulated, planes, self.full_planes, self.width, self.height, f, self.between, 2, *self.up_k, stream=s)
            c.svgf_filter_device(self.between, self.full_planes, self.width, self.height, self.out, None, params=self.svgf, stream=s)
            self.accumulated, self.history = self.history, self.accumulated
        else:
            filtered = self.out if f == 1 else self.between
            if self.svgf.feedback_pass >= 0:
                c.svgf_filter_device(self.accumulated, planes, W, H, filtered, self.history, params=self.svgf, stream=s)
            else:                                                      # nothing is fed back: the accumulated history is the one handed on
                c.svgf_filter_device(self.accumulated, planes, W, H, filtered, None, params=self.svgf, stream=s)
                self.accumulated, self.history = self.history, self.accumulated
            if f > 1:                                                  # A: the filtered frame goes up
                c.upsample_device(filtered, planes, self.full_planes, self.width, self.height, f, self.out, 1, *self.up_k, stream=s)
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
