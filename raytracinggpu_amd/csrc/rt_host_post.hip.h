// rt_host_post.hip.h -- host side of libraytrace_hip.so (textually included by rt_capi.hip, one translation unit, after rt_host_ctx.hip.h and before everything that issues
// work): what the device entries and the post-process stages (rt_aov*.hip.h, rt_denoise.hip.h, rt_temporal.hip.h, rt_demodulate.hip.h) share -- the stream a call runs on,
// the note a pipelined render needs of it, the argument checks they have in common, the copy to the host that ends a host form, the opening of the render entries' row-range host forms, and the staging
// of a post-process host form through one buffer of the context.
#pragma once
#include <initializer_list>

namespace {

// The stream a device entry runs on: the caller's, or else the context's own (which must exist).  Sets the context's device.
int call_stream(rt_ctx *ctx, void *stream, hipStream_t &q) {
    q = stream ? static_cast<hipStream_t>(stream) : own_stream(ctx);
    if (!q) return fail(ctx, RT_ERR_HIP, "the context's stream: %s", ctx->err.c_str());
    RT_HIP(ctx, hipSetDevice(ctx->device));
    return RT_OK;
}

// What a call that is no render call puts on stream q and touches there, for the pipelined render that follows (Pipe::between: a frame must not overtake a read of its
// own buffer or start behind a write into it).  The rule: a call's ranges are kept all together or not at all, and the list never grows past kBetweenMax -- a call that
// would take it there sets between_overflow instead, and the next frame takes the full fork.
struct DevRange { const void *p; size_t bytes; };
constexpr size_t kBetweenMax = 64;
void note_between(rt_ctx *ctx, hipStream_t q, std::initializer_list<DevRange> ranges) {
    rt_ctx::Pipe &pl = ctx->pipe;
    if (!pl.on) return;
    if (pl.between.size() + ranges.size() > kBetweenMax) { pl.between_overflow = true; return; }
    for (const DevRange &r : ranges) {
        const uint8_t *lo = static_cast<const uint8_t *>(r.p);
        pl.between.push_back({lo, lo + r.bytes, q});
    }
}

// do [a, a + na) and [b, b + nb) share a byte?
bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uint8_t *x = static_cast<const uint8_t *>(a), *y = static_cast<const uint8_t *>(b);
    return x < y + nb && y < x + na;
}

// the pixels of one post-process call stay below this: int pixel indices, and every launch's grid fits (rt_denoise.hip.h looks at its passes' grids itself)
constexpr int64_t kPostMaxPixels = 1 << 28;
int check_frame_size(rt_ctx *ctx, int width, int height) {
    if (width <= 0 || height <= 0 || (int64_t)width * height >= kPostMaxPixels) return fail(ctx, RT_ERR_INVALID, "width/height must be positive, at most 2^28 pixels");
    return RT_OK;
}

// Device -> host on the context's stream (which exists: RT_OWN_STREAM), complete on return: how a host form ends.  bytes == 0: only the wait.
int copy_back(rt_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (bytes) RT_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, own_stream(ctx)));
    RT_HIP(ctx, hipStreamSynchronize(own_stream(ctx)));
    return RT_OK;
}

// How the host forms over the image rows [row_begin, row_end) open (rt_render, rt_render_rgb8, rt_count_work; rt_render_pose: every row): the arguments, the context's
// stream, scratch_rgba with room for the rows.  rows: the range as one tile; npix: its pixels.  `out` is only looked at for NULL.
int host_rows(rt_ctx *ctx, const rt_params *p, int row_begin, int row_end, const void *out, rt_rows &rows, int64_t &npix) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    if (!p || !out) return fail(ctx, RT_ERR_INVALID, "params/out is NULL");
    if (row_begin < 0 || row_end < row_begin || row_end > p->height) return fail(ctx, RT_ERR_INVALID, "bad row range [%d,%d)", row_begin, row_end);
    const int n = row_end - row_begin;
    npix = (int64_t)n * (p->width > 0 ? p->width : 0);
    rows = rt_rows{row_begin, n, n > 0 ? n : 1, 1};
    return ensure(ctx, ctx->scratch_rgba, (size_t)npix * sizeof(float4));
}

// A host form on top of its device form.  One buffer of the context (post_io: every host form synchronises before it returns, so no two hold it at once) takes the
// input segments one behind the other (a segment without a pointer keeps its room and is not copied) and the result, out_bytes at out_off; device(base) issues the
// device form on the context's stream over that buffer; then the result goes to out_host and the stream is waited for.
struct HostSeg { const void *p; size_t bytes; };
template <class Device>
int staged(rt_ctx *ctx, std::initializer_list<HostSeg> in, size_t out_off, size_t out_bytes, void *out_host, Device device) {
    size_t total = out_off + out_bytes, off = 0;
    for (const HostSeg &s : in) off += s.bytes;
    int rc = ensure(ctx, ctx->post_io, std::max(total, off));
    if (rc != RT_OK) return rc;
    uint8_t *base = static_cast<uint8_t *>(ctx->post_io.p);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    off = 0;
    for (const HostSeg &s : in) {
        if (s.p) RT_HIP(ctx, hipMemcpyAsync(base + off, s.p, s.bytes, hipMemcpyHostToDevice, own_stream(ctx)));
        off += s.bytes;
    }
    if ((rc = device(base)) != RT_OK) return rc;
    return copy_back(ctx, out_host, base + out_off, out_bytes);
}

}  // namespace
