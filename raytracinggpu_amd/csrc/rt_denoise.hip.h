// rt_denoise.hip.h -- rt_denoise[_device]: the edge-avoiding a-trous filter over a colour frame, guided by the planes of rt_render_aov (rt_aov.hip.h).
// Included at the end of rt_capi.hip, after rt_aov_surface.hip.h (same translation unit: the host half uses rt_host_post.hip.h).
//
// Pass k (step s = 2^k) is one launch: a 5x5 B3-spline stencil with holes, every tap weighted by how well its first hit agrees with the centre's -- same object,
// normal, tangent plane, albedo, colour (raytrace_hip.h states the formula; it is the contract: binary32, one rounding per operation, taps in row-major order,
// tests/denoise_model.py is its numpy twin).
// How a pass runs: a stencil with holes of s never leaves the pixels that share (x mod s, y mod s), so the image is s x s independent sub-images on which the stencil
// is the DENSE 5x5 one.  A workgroup takes a tile of kDnTileW x kDnTileH pixels of one sub-image, one lane per pixel, brings the tile's four planes with a halo of 2
// sub-image pixels into LDS once (plane after plane: N|id, P, albedo, colour; 27 KiB, whatever s is) and reads its 25 taps from there as ds_read_b128s: 6.75 global
// 16-byte loads per pixel instead of 100.  For s > 1 those loads and the store are strided by 16 s bytes; the workgroups of the s x-phases of one tile are numbered
// next to each other and the numbering keeps neighbours on one XCD, so the rest of every line they fetch is used from the same L2.  (Loading the taps directly --
// coalesced rows through L1, no LDS -- measured 280-340 us per 1080p pass at s >= 4 against 82 us for the tiled s = 1 pass: DESIGN.md section 5.7.)
// A tap whose object id differs is dropped before its other three records are looked at.
//
// rt_denoise_var[_device] is the same kernel's second instantiation (VAR): the colour term is measured against the pixel's own variance -- the history of
// rt_temporal.hip.h carries it -- instead of k_color, and the variance is filtered along: a fifth plane of one float per pixel rides in the LDS tile (28.7 KiB),
// read from .w of history plane 1 on pass 0 and from a float plane of the context between passes.  The plain instantiation is instruction for instruction what it
// was before the parameter existed (its argument list is the same: the VAR arguments are a parameter pack that is empty for it).
//
// rt_svgf_filter[_device] is the third instantiation (VAR with a DnSvgf pack): rt_denoise_var's pass with two switches.  PRE-FILTER: the colour tolerance D is
// formed from the 3 x 3 Gaussian of the variance over the pass's own sub-image neighbours of the same object -- nine floats that are in dn_var already, one quotient
// more per pixel and pass, no global load, no byte of LDS more.  FEEDBACK: pass f's colour is plane 0 of a second history the caller hands to the next accumulation.  It costs no pass
// over the colour: pass f writes there INSTEAD of the ping-pong buffer and pass f + 1 reads from there (the last pass, which must land in the output, writes both);
// the lanes of pass f copy their pixel's plane-1 record along.  .w and the miss pixels come out right by themselves: every pass hands C_p.w and a miss's C_p through.
#pragma once
#include <type_traits>
#include "rt_div.h"

namespace rtk {

constexpr int kDnTileW = 32, kDnTileH = 8;           // 256 lanes; a wave = rows 2 w, 2 w + 1 of the tile
constexpr int kDnHalo = 2;                           // in pixels of the sub-image
constexpr int kDnTw = kDnTileW + 2 * kDnHalo, kDnTh = kDnTileH + 2 * kDnHalo;
constexpr int kDnXcds = 8;                           // consecutive workgroup ids go round the XCDs

struct DnParams { float k_normal, k_position, k_albedo, k_color; };   // k_color already scaled by 4^k (VAR: not read)
// the VAR instantiation's own arguments: the variance plane read (v_stride floats apart: 4 = .w of a float4 plane, 1 = a float plane), the one written (or nullptr)
struct DnVar { const float *v_in; float *v_out; int v_stride; float k_sigma, var_floor; };
// the SVGF instantiation's: those, the pre-filter switch, and for the feedback pass (else all nullptr) a second frame to write the pass's colour into (fb_out; nullptr
// where the pass's own `out` is the history already) and the history's plane 1 to copy, record for record (h1_in -> h1_out)
struct DnSvgf { DnVar v; int prefilter; float4 *fb_out; const float4 *h1_in; float4 *h1_out; };
// Rec. 709 luminance, in this order of operations (rt_temporal.hip.h measures its moments with it too)
__device__ __forceinline__ float lum709(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

__device__ __forceinline__ float dn_sqdiff(float4 a, float4 b) {
    const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return (x * x + y * y) + z * z;
}
// max(0, 1 - d k); a k of exactly 0 makes the term exactly 1, whatever d is
__device__ __forceinline__ float dn_term(float d, float k) { return k == 0.f ? 1.f : fmaxf(0.f, 1.f - d * k); }

// The pixel's filtered value.  fetch(plane, dx, dy): record `plane` (0 N|id, 1 P, 2 albedo, 3 colour) of the pixel (x + dx s, y + dy s), which lies inside the image.
// VAR: fetch_v(dx, dy) is that pixel's variance, kv the variance term's two constants, v_out the filtered variance.
// PRE (the SVGF instantiation) with prefilter != 0: D comes from the 3 x 3 Gaussian of the variance instead of V_p; v_out does not change.
template <bool VAR, bool PRE = false, class Fetch, class FetchV>
__device__ __forceinline__ float4 dn_pixel(int x, int y, int W, int H, int s, const DnParams &k, Fetch fetch, FetchV fetch_v, float k_sigma, float var_floor, float &v_out,
                                           [[maybe_unused]] int prefilter = 0) {
    const float4 Np = fetch(0, 0, 0), Cp = fetch(3, 0, 0);
    float lp = 0.f, D = 0.f, Dr = 0.f, Sv = 0.f;
    bool d_fast = false;
    if constexpr (VAR) v_out = fetch_v(0, 0);
    if (Np.w == -1.f) return Cp;                                      // a miss: nothing to guide the filter
    if constexpr (VAR) {
        lp = lum709(Cp);
        float Vd = v_out;
        if constexpr (PRE) {
            if (prefilter) {                                          // (wave-uniform)
                const float Gk[2] = {0.5f, 0.25f};
                float Sg = 0.f, Wg = 0.f;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int qx = x + dx * s, qy = y + dy * s;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        if (fetch(0, dx, dy).w != Np.w) continue;
                        const float g = Gk[dy < 0 ? -dy : dy] * Gk[dx < 0 ? -dx : dx];
                        Sg = Sg + g * fetch_v(dx, dy);
                        Wg = Wg + g;
                    }
                }
                Vd = div_quot(Sg, Wg);                                // (the centre always counts: Wg >= 1/4)
            }
        }
        D = k_sigma * Vd + var_floor;                                 // the colour tolerance, in the colour's own units squared
        Dr = div_refine(D, __builtin_amdgcn_rcpf(D));
        d_fast = div_in_range(D);
    }
    const float4 Pp = fetch(1, 0, 0), Ap = fetch(2, 0, 0);
    const float Hk[3] = {0.375f, 0.25f, 0.0625f};
    float Sx = 0.f, Sy = 0.f, Sz = 0.f, Wt = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s, qy = y + dy * s;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float4 Nq = fetch(0, dx, dy);
            if (Nq.w != Np.w) continue;                               // another object (or a miss)
            const float h = Hk[dy < 0 ? -dy : dy] * Hk[dx < 0 ? -dx : dx];
            float w = h * dn_term(dn_sqdiff(Np, Nq), k.k_normal);
            if (k.k_position != 0.f) {
                const float4 Pq = fetch(1, dx, dy);
                const float e = (Np.x * (Pq.x - Pp.x) + Np.y * (Pq.y - Pp.y)) + Np.z * (Pq.z - Pp.z);
                w = w * fmaxf(0.f, 1.f - (e * e) * k.k_position);
            }                                                         // (else: times exactly 1)
            if (k.k_albedo != 0.f) w = w * fmaxf(0.f, 1.f - dn_sqdiff(Ap, fetch(2, dx, dy)) * k.k_albedo);
            const float4 Cq = fetch(3, dx, dy);
            if constexpr (VAR) {
                const float dl = lp - lum709(Cq), dl2 = dl * dl;
                if (dl2 != 0.f) {                                     // (equal luminance: the term is exactly 1, no quotient is formed)
                    float qd = div_by(dl2, D, Dr);
                    if (!(d_fast && div_in_range(dl2))) qd = dl2 / D;
                    w = w * fmaxf(0.f, 1.f - qd);
                }
            } else {
                w = w * dn_term(dn_sqdiff(Cp, Cq), k.k_color);
            }
            if (w > 0.f) {                                            // (false for a NaN weight: a NaN guide does not spread)
                Sx = Sx + w * Cq.x; Sy = Sy + w * Cq.y; Sz = Sz + w * Cq.z;
                Wt = Wt + w;
                if constexpr (VAR) Sv = Sv + (w * w) * fetch_v(dx, dy);
            }
        }
    }
    // S / W, correctly rounded: three numerators over one denominator (rt_div.h), the literal quotient outside the shared sequence's range
    const float r1 = div_refine(Wt, __builtin_amdgcn_rcpf(Wt));
    float ox = div_by(Sx, Wt, r1), oy = div_by(Sy, Wt, r1), oz = div_by(Sz, Wt, r1);
    const bool fast = div_in_range(Wt) && div_in_range(Sx) && div_in_range(Sy) && div_in_range(Sz);
    if (__builtin_expect(__ballot(!fast) != 0ull, 0)) {
        if (!fast) { ox = Sx / Wt; oy = Sy / Wt; oz = Sz / Wt; }
    }
    if constexpr (VAR) {                                              // the variance of the weighted mean: sum w^2 V / (sum w)^2
        v_out = div_quot(Sv, Wt * Wt);
    }
    return make_float4(ox, oy, oz, Cp.w);
}

// g: the three guide planes (W * H float4 each, consecutive), C: the pass's input frame.  tiles_x, tiles_y: tiles of a sub-image; n_blocks = tiles_x * tiles_y * s * s.
// VAR: one more argument, a DnVar or a DnSvgf (the pack is empty for the plain filter, whose argument list is the one it always had).
template <bool VAR, class... Var>
__global__ __launch_bounds__(kDnTileW * kDnTileH) void denoise_pass_kernel(const float4 *__restrict__ C, const float4 *__restrict__ g, float4 *__restrict__ out,
                                                                            int W, int H, int s, int tiles_x, int tiles_y, int n_blocks, const DnParams k, const Var... var) {
    static_assert(sizeof...(Var) == (VAR ? 1 : 0), "the VAR instantiation takes one DnVar or DnSvgf");
    constexpr bool SVGF = (std::is_same_v<Var, DnSvgf> || ...);
    __shared__ float4 dn_tile[4 * kDnTw * kDnTh];    // [4 planes][kDnTh rows][kDnTw]: neighbouring lanes read neighbouring 16 bytes
    __shared__ float dn_var[VAR ? kDnTw * kDnTh : 1];                 // VAR: the variance of the same pixels
    [[maybe_unused]] DnVar kv{nullptr, nullptr, 1, 0.f, 0.f};
    [[maybe_unused]] DnSvgf ks{kv, 0, nullptr, nullptr, nullptr};
    if constexpr (SVGF) { ks = (var, ...); kv = ks.v; }
    else if constexpr (VAR) kv = (var, ...);
    // workgroup id -> work item: ids b, b + 8, b + 16 .. run on one XCD and take consecutive items (the grid is padded to a multiple of kDnXcds)
    const int per_xcd = (int)gridDim.x / kDnXcds;
    const int item = ((int)blockIdx.x % kDnXcds) * per_xcd + (int)blockIdx.x / kDnXcds;
    if (item >= n_blocks) return;                                     // (the whole workgroup: no barrier is left behind)
    // item = ((tile_y * s + phase_y) * tiles_x + tile_x) * s + phase_x: the x-phases of a tile are neighbours
    const int phase_x = item % s, i1 = item / s;
    const int tile_x = i1 % tiles_x, i2 = i1 / tiles_x;
    const int phase_y = i2 % s, tile_y = i2 / s;
    const size_t plane = (size_t)W * (size_t)H;
    const int tx = threadIdx.x & (kDnTileW - 1), ty = threadIdx.x / kDnTileW;
    const int sx0 = tile_x * kDnTileW - kDnHalo, sy0 = tile_y * kDnTileH - kDnHalo;   // the LDS tile's origin, in sub-image pixels
    for (int i = threadIdx.x; i < kDnTw * kDnTh; i += kDnTileW * kDnTileH) {
        const int ly = i / kDnTw, lx = i - ly * kDnTw;
        const int qx = (sx0 + lx) * s + phase_x, qy = (sy0 + ly) * s + phase_y;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;         // never read: the taps test the image's bounds themselves
        const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
#pragma unroll
        for (int p = 0; p < 3; ++p) dn_tile[p * kDnTw * kDnTh + i] = g[(size_t)p * plane + q];
        dn_tile[3 * kDnTw * kDnTh + i] = C[q];
        if constexpr (VAR) dn_var[i] = kv.v_in[q * (size_t)kv.v_stride];
    }
    __syncthreads();
    const int x = (tile_x * kDnTileW + tx) * s + phase_x, y = (tile_y * kDnTileH + ty) * s + phase_y;
    if (x >= W || y >= H) return;
    const int centre = (ty + kDnHalo) * kDnTw + tx + kDnHalo;        // a tap at (dx s, dy s) is the sub-image's neighbour (dx, dy)
    const size_t pix = (size_t)y * W + x;
    float v = 0.f;
    const float4 c = dn_pixel<VAR, SVGF>(x, y, W, H, s, k, [&](int p, int dx, int dy) -> float4 { return dn_tile[p * kDnTw * kDnTh + centre + dy * kDnTw + dx]; },
                                         [&](int dx, int dy) -> float { return dn_var[VAR ? centre + dy * kDnTw + dx : 0]; }, kv.k_sigma, kv.var_floor, v, ks.prefilter);
    out[pix] = c;
    if constexpr (SVGF) {
        if (ks.fb_out) ks.fb_out[pix] = c;
        if (ks.h1_out) ks.h1_out[pix] = ks.h1_in[pix];
    }
    if constexpr (VAR) { if (kv.v_out) kv.v_out[pix] = v; }
}

}  // namespace rtk

// The grid of pass k (step s = 2^k): the tiles of the largest sub-image (phase 0), ceil(ceil(W / s) / tile) each way, and n_blocks = tiles_x * tiles_y * s * s workgroups
// with work; the launch pads n_blocks to a multiple of kDnXcds.
struct DnGrid { int64_t tiles_x, tiles_y, n_blocks; };
static DnGrid dn_grid(int width, int height, int k) {
    const int s = 1 << k;
    const int64_t tiles_x = ((width + s - 1) / s + rtk::kDnTileW - 1) / rtk::kDnTileW, tiles_y = ((height + s - 1) / s + rtk::kDnTileH - 1) / rtk::kDnTileH;
    return {tiles_x, tiles_y, tiles_x * tiles_y * s * s};
}

// Does every pass's grid fit a launch (fewer than 2^31 workgroups, which is also what the kernel's int item arithmetic holds)?  Tiles round every sub-image up, so
// thin frames cost most.  Below 2^28 pixels: the widest frame, 2^28 - 1 by 1, is ceil(2^21 / 32) x 1 tiles x 128 x 128 = 2^30 workgroups at step 128 and fits; the
// highest, 1 by 2^28 - 1, is 1 x ceil(2^21 / 8) tiles x 128 x 128 = 2^32 there (8-row tiles against 32-pixel ones) and already 2^31 at step 64, and does not.  What
// is refused: one or two pixels of width with n_passes 8 from 2^27 - 1023 rows on, one pixel of width with n_passes 7 from 2^28 - 511 rows on.
static bool dn_grids_fit(int width, int height, int n_passes) {
    for (int k = 0; k < n_passes; ++k)
        if (dn_grid(width, height, k).n_blocks + rtk::kDnXcds > (int64_t)INT32_MAX) return false;
    return true;
}

// One call of the family, whichever of the six entries it came through: rt_denoise* over a colour frame (Plain), rt_denoise_var* over a history of
// rt_temporal_accumulate (Var: two planes, the variance is .w of plane 1), rt_svgf_filter* (Svgf: Var with the two switches).  Everything below dn_call is written once.
enum class DnKind { Plain, Var, Svgf };
struct DnCall {
    DnKind kind;
    const void *in, *aov;                            // in: the colour frame (Plain) or the history
    int width, height;
    const void *params;                              // the entry's own structure, looked at for NULL only: dn_call has copied its fields
    void *out, *out_history;                         // out_history: Svgf with feedback, else nullptr
    int n_passes = 0;
    float k_normal = 0.f, k_position = 0.f, k_albedo = 0.f, k_color = 0.f, k_sigma = 0.f, var_floor = 0.f;   // k_color: Plain; k_sigma, var_floor: the other two
    int prefilter = 0, feedback_pass = -1;           // (Svgf's)
    int in_planes() const { return kind == DnKind::Plain ? 1 : 2; }
};
static DnCall dn_call(const void *in, const void *aov, int width, int height, const rt_denoise_params *dp, void *out) {
    DnCall c{DnKind::Plain, in, aov, width, height, dp, out, nullptr};
    if (dp) c.n_passes = dp->n_passes, c.k_normal = dp->k_normal, c.k_position = dp->k_position, c.k_albedo = dp->k_albedo, c.k_color = dp->k_color;
    return c;
}
static DnCall dn_call(const void *in, const void *aov, int width, int height, const rt_denoise_var_params *vp, void *out) {
    DnCall c{DnKind::Var, in, aov, width, height, vp, out, nullptr};
    if (vp) c.n_passes = vp->n_passes, c.k_normal = vp->k_normal, c.k_position = vp->k_position, c.k_albedo = vp->k_albedo, c.k_sigma = vp->k_sigma, c.var_floor = vp->var_floor;
    return c;
}
static DnCall dn_call(const void *in, const void *aov, int width, int height, const rt_svgf_params *sp, void *out, void *out_history) {
    DnCall c{DnKind::Svgf, in, aov, width, height, sp, out, out_history};
    if (sp) {
        c.n_passes = sp->n_passes, c.k_normal = sp->k_normal, c.k_position = sp->k_position, c.k_albedo = sp->k_albedo, c.k_sigma = sp->k_sigma, c.var_floor = sp->var_floor;
        c.prefilter = sp->prefilter, c.feedback_pass = sp->feedback_pass;
    }
    return c;
}

// What every entry and both forms ask of their arguments.  No output may share a byte with an input or with the other output.
static int dn_check(rt_ctx *ctx, const DnCall &c) {
    if (!c.in || !c.aov || !c.params || !c.out) return fail(ctx, RT_ERR_INVALID, "%s/aov/params/out is NULL", c.kind == DnKind::Plain ? "color" : "history");
    if (int rc = check_frame_size(ctx, c.width, c.height); rc != RT_OK) return rc;
    if (c.n_passes < 1 || c.n_passes > RT_DENOISE_MAX_PASSES) return fail(ctx, RT_ERR_INVALID, "n_passes %d outside [1,%d]", c.n_passes, RT_DENOISE_MAX_PASSES);
    if (!dn_grids_fit(c.width, c.height, c.n_passes))
        return fail(ctx, RT_ERR_INVALID, "a %d x %d frame needs 2^31 or more workgroups in one of %d passes", c.width, c.height, c.n_passes);
    const size_t bytes = (size_t)c.width * c.height * sizeof(float4);
    if (overlaps(c.out, bytes, c.in, c.in_planes() * bytes) || overlaps(c.out, bytes, c.aov, 3 * bytes)) return fail(ctx, RT_ERR_INVALID, "the output overlaps an input");
    if (c.kind != DnKind::Svgf) return RT_OK;
    if (c.prefilter != 0 && c.prefilter != 1) return fail(ctx, RT_ERR_INVALID, "prefilter %d is neither 0 nor 1", c.prefilter);
    if (c.feedback_pass < -1 || c.feedback_pass >= c.n_passes) return fail(ctx, RT_ERR_INVALID, "feedback_pass %d outside [-1,%d]", c.feedback_pass, c.n_passes - 1);
    if ((c.feedback_pass == -1) != (c.out_history == nullptr)) return fail(ctx, RT_ERR_INVALID, "out_history goes with feedback_pass >= 0, and only with it");
    if (c.out_history && (overlaps(c.out_history, 2 * bytes, c.in, 2 * bytes) || overlaps(c.out_history, 2 * bytes, c.aov, 3 * bytes) || overlaps(c.out_history, 2 * bytes, c.out, bytes)))
        return fail(ctx, RT_ERR_INVALID, "out_history overlaps an input or the output");
    return RT_OK;
}

// What pass k reads and writes; v is what the Var (v.v alone) and Svgf instantiations are handed (Plain: not looked at).
struct DnPass { const float4 *src; float4 *dst; rtk::DnSvgf v; };

// The plan of a checked call's passes, and the context's buffers it needs.  Where the passes write: the last one into the output; pass f (the feedback pass) into plane 0
// of the second history -- and, where f is the last pass, into both; the others alternate between the output and the context's ping-pong frame, counted back from the
// last pass behind f and from pass f - 1 before it, so that no pass reads the frame it writes and nothing is written into the second history after pass f.  Without
// feedback (f = -1) that is the plain alternation that ends in the output.  The variance goes from .w of history plane 1 through the context's two float planes, and the
// last pass writes none.  Plane 1 of the second history is copied by pass f's lanes: 6.5 - 8.2 us of a 1080p call against 14.8 us for a device-to-device copy on the
// stream.
static int dn_plan(rt_ctx *ctx, const DnCall &c, DnPass *pass) {
    const size_t npix = (size_t)c.width * c.height;
    const int n = c.n_passes, f = c.feedback_pass;
    const bool var = c.kind != DnKind::Plain;
    // 0: the output, 1: the context's frame, 2: plane 0 of the second history
    int where[RT_DENOISE_MAX_PASSES], rc;
    bool tmp = false;
    for (int k = 0; k < n; ++k) {
        // (before pass f: counted back from pass f - 1, which takes the output -- or the context's frame where pass f is the last one and takes the output itself)
        where[k] = k == n - 1 ? 0 : k == f ? 2 : k > f ? (n - 1 - k) & 1 : (f - 1 - k + (f == n - 1)) & 1;
        tmp = tmp || where[k] == 1;
    }
    if (tmp && (rc = ensure(ctx, ctx->dn_tmp, npix * sizeof(float4))) != RT_OK) return rc;
    if (var && n > 1 && (rc = ensure(ctx, ctx->dnv_var[0], npix * sizeof(float))) != RT_OK) return rc;
    if (var && n > 2 && (rc = ensure(ctx, ctx->dnv_var[1], npix * sizeof(float))) != RT_OK) return rc;
    const float4 *in = static_cast<const float4 *>(c.in);
    float4 *fb = static_cast<float4 *>(c.out_history), *const frames[3] = {static_cast<float4 *>(c.out), static_cast<float4 *>(ctx->dn_tmp.p), fb};
    for (int k = 0; k < n; ++k) {
        DnPass &p = pass[k];
        p.src = k == 0 ? in : pass[k - 1].dst;
        p.dst = frames[where[k]];
        if (!var) continue;
        p.v = {{k == 0 ? reinterpret_cast<const float *>(in + npix) + 3 : static_cast<const float *>(ctx->dnv_var[(k - 1) & 1].p),
                k == n - 1 ? nullptr : static_cast<float *>(ctx->dnv_var[k & 1].p), k == 0 ? 4 : 1, c.k_sigma, c.var_floor},
               c.prefilter, k == f && p.dst != fb ? fb : nullptr, k == f ? in + npix : nullptr, k == f ? fb + npix : nullptr};
    }
    return RT_OK;
}

static int dn_device(rt_ctx *ctx, const DnCall &c, void *stream) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    int rc = dn_check(ctx, c);
    if (rc != RT_OK) return rc;
    hipStream_t q;
    if ((rc = call_stream(ctx, stream, q)) != RT_OK) return rc;
    DnPass pass[RT_DENOISE_MAX_PASSES] = {};
    if ((rc = dn_plan(ctx, c, pass)) != RT_OK) return rc;
    const size_t bytes = (size_t)c.width * c.height * sizeof(float4);
    // a pipelined frame must not overtake this read of a frame / write of an image
    if (c.out_history) note_between(ctx, q, {{c.in, c.in_planes() * bytes}, {c.out, bytes}, {c.out_history, 2 * bytes}});
    else note_between(ctx, q, {{c.in, c.in_planes() * bytes}, {c.out, bytes}});
    const float4 *guide = static_cast<const float4 *>(c.aov);
    const dim3 block(rtk::kDnTileW * rtk::kDnTileH);
    for (int k = 0; k < c.n_passes; ++k) {
        const DnPass &p = pass[k];
        const int s = 1 << k;
        const DnGrid g = dn_grid(c.width, c.height, k);
        const dim3 grid((unsigned)((g.n_blocks + rtk::kDnXcds - 1) / rtk::kDnXcds * rtk::kDnXcds));
        const rtk::DnParams kp{c.k_normal, c.k_position, c.k_albedo, c.kind == DnKind::Plain ? c.k_color * (float)(1 << (2 * k)) : 0.f};   // 4^k: an exact scale
        const int tiles_x = (int)g.tiles_x, tiles_y = (int)g.tiles_y, n_blocks = (int)g.n_blocks;
        switch (c.kind) {                                             // (Svgf first: the code object holds the instantiations in the order they are named here, and keeps its order)
        case DnKind::Svgf: hipLaunchKernelGGL((rtk::denoise_pass_kernel<true, rtk::DnSvgf>), grid, block, 0, q, p.src, guide, p.dst, c.width, c.height, s, tiles_x, tiles_y, n_blocks, kp, p.v); break;
        case DnKind::Plain: hipLaunchKernelGGL(rtk::denoise_pass_kernel<false>, grid, block, 0, q, p.src, guide, p.dst, c.width, c.height, s, tiles_x, tiles_y, n_blocks, kp); break;
        case DnKind::Var: hipLaunchKernelGGL((rtk::denoise_pass_kernel<true, rtk::DnVar>), grid, block, 0, q, p.src, guide, p.dst, c.width, c.height, s, tiles_x, tiles_y, n_blocks, kp, p.v.v); break;
        }
    }
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// the host form: the input's planes, the three guide planes, room for the second history (with feedback only), the result
static int dn_host(rt_ctx *ctx, const DnCall &c) {
    if (!ctx) return fail(nullptr, RT_ERR_INVALID, "ctx is NULL");
    RT_OWN_STREAM(ctx);
    const int rc = dn_check(ctx, c);
    if (rc != RT_OK) return rc;
    const size_t bytes = (size_t)c.width * c.height * sizeof(float4), in_bytes = c.in_planes() * bytes, fb_off = in_bytes + 3 * bytes, fb_bytes = c.out_history ? 2 * bytes : 0;
    return staged(ctx, {{c.in, in_bytes}, {c.aov, 3 * bytes}, {nullptr, fb_bytes}}, fb_off + fb_bytes, bytes, c.out, [&](uint8_t *d) {
        DnCall dc = c;
        dc.in = d, dc.aov = d + in_bytes, dc.out = d + fb_off + fb_bytes, dc.out_history = c.out_history ? d + fb_off : nullptr;
        const int r = dn_device(ctx, dc, nullptr);
        if (r != RT_OK || !c.out_history) return r;
        RT_HIP(ctx, hipMemcpyAsync(c.out_history, d + fb_off, fb_bytes, hipMemcpyDeviceToHost, own_stream(ctx)));   // (staged waits for the stream)
        return (int)RT_OK;
    });
}

extern "C" int rt_denoise_device(rt_ctx *ctx, const void *color_dev, const void *aov_dev, int width, int height, const rt_denoise_params *dp, void *out_dev, void *stream) {
    return dn_device(ctx, dn_call(color_dev, aov_dev, width, height, dp, out_dev), stream);
}
extern "C" int rt_denoise(rt_ctx *ctx, const float *color_host, const float *aov_host, int width, int height, const rt_denoise_params *dp, float *out_host) {
    return dn_host(ctx, dn_call(color_host, aov_host, width, height, dp, out_host));
}
extern "C" int rt_denoise_var_device(rt_ctx *ctx, const void *history_dev, const void *aov_dev, int width, int height, const rt_denoise_var_params *vp, void *out_dev, void *stream) {
    return dn_device(ctx, dn_call(history_dev, aov_dev, width, height, vp, out_dev), stream);
}
extern "C" int rt_denoise_var(rt_ctx *ctx, const float *history_host, const float *aov_host, int width, int height, const rt_denoise_var_params *vp, float *out_host) {
    return dn_host(ctx, dn_call(history_host, aov_host, width, height, vp, out_host));
}
extern "C" int rt_svgf_filter_device(rt_ctx *ctx, const void *history_dev, const void *aov_dev, int width, int height, const rt_svgf_params *sp, void *out_dev, void *out_history_dev, void *stream) {
    return dn_device(ctx, dn_call(history_dev, aov_dev, width, height, sp, out_dev, out_history_dev), stream);
}
extern "C" int rt_svgf_filter(rt_ctx *ctx, const float *history_host, const float *aov_host, int width, int height, const rt_svgf_params *sp, float *out_host, float *out_history_host) {
    return dn_host(ctx, dn_call(history_host, aov_host, width, height, sp, out_host, out_history_host));
}
