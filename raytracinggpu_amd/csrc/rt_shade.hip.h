// rt_shade.hip.h -- the arithmetic of one path step, written once for the four render structures.
//
// Scene::getColor (cpu_launcher.cpp:566-648) and the camera ray (cpu:699-709) as functions over values.  The render kernels -- render_kernel
// (rt_kernels.hip.h), render_persistent (rt_persistent.hip.h), wf_advance (rt_wavefront.hip.h), wf_path (rt_path.hip.h) -- keep their own control
// flow and state (a loop over segments, a phase machine, queue records in HBM, tables in LDS) and call these for everything they compute alike,
// so a material rule is changed in one place and the four stay bit-identical by construction.  No function here knows its caller.  Every
// expression keeps the operand order and the single roundings of the reference (DESIGN.md "Numerics").
//
// Included by rt_kernels.hip.h once the vector, RNG, Scene, Frame and Material definitions it needs are visible.
#pragma once

namespace rtk {

// ---- pixels and samples ----
// image row of local row `lrow` of a (sub-)frame: rows come in tiles of tile_rows, every tile_step-th tile of the image from row0 on
__device__ __forceinline__ int image_row(const Frame &fr, int lrow) {
    return fr.row0 + (lrow / fr.tile_rows) * fr.tile_rows * fr.tile_step + (lrow % fr.tile_rows);
}
// the counter RNG's key of a pixel, and of its sample `samp` (DESIGN.md "RNG"): keyed by the GLOBAL pixel, so a tile of a frame draws what the whole frame draws
__device__ __forceinline__ uint32_t pixel_hash(const Frame &fr, int row, int px, uint32_t seed) {
    return mix32(((uint32_t)row * (uint32_t)fr.W + (uint32_t)px) ^ mix32(seed));
}
__device__ __forceinline__ uint32_t sample_hash(uint32_t hp, int samp) { return mix32(hp ^ ((uint32_t)samp * 0x9E3779B1U)); }

// The camera ray's direction, cpu:699-709, in three parts.  pixel_dir: pixel (px, row) seen from the camera of cpu_launcher (z = -W / (2 tan(fov / 2)): looking down -z).
__device__ __forceinline__ f3 pixel_dir(const Frame &fr, int px, int row, float z) {
    // cpu:699: +0.5/-0.5 are double literals, narrowed by the Vector constructor
    return mk((float)((double)((float)px - (float)fr.W / 2) + 0.5), (float)((double)((float)fr.H / 2 - (float)row) - 0.5), z);
}
// ... seen from a posed camera at C with the basis of the Frame, realtime:1115: cam.C + cam.bz * z + cam.bx * X + cam.by * Y (the position is part of the direction there)
__device__ __forceinline__ f3 posed_dir(const Frame &fr, f3 C, f3 uc) {
    const f3 Bx = mk(fr.bx[0], fr.bx[1], fr.bx[2]), By = mk(fr.by[0], fr.by[1], fr.by[2]), Bz = mk(fr.bz[0], fr.bz[1], fr.bz[2]);
    const f3 a = C + mk(Bz.x * uc.z, Bz.y * uc.z, Bz.z * uc.z);
    const f3 b = a + mk(Bx.x * uc.x, Bx.y * uc.x, Bx.z * uc.x);
    return b + mk(By.x * uc.y, By.y * uc.y, By.z * uc.y);
}
// ... moved by the anti-aliasing jitter of cpu:705-707 (Box-Muller from dims 2, 3 of the sample's key hs) and normalised (cpu:709).  With sigma == 0 the jitter is
// exactly +-0 and the direction is unchanged: the key is not read.
__device__ __forceinline__ f3 jitter_dir(const Frame &fr, f3 v, uint32_t hs) {
    if (fr.sigma != 0.f) {
        const float r1 = uniform01(hs, 0, 2), r2 = uniform01(hs, 0, 3);
        const float bm = fr.sigma * rt_sqrtf(-2 * logf(r1));
        double sn, cs;
        rt_sincos_2pi(2 * 3.14159265358979323846 * (double)r2, sn, cs);
        v = v + mk((float)((double)bm * cs), (float)((double)bm * sn), 0.f);
    }
    return normalize(v);
}
// The whole of it for a Frame that may carry a pose (cam_mode 1).  The kernels that the host never hands a pose (render_kernel, render_persistent) compose
// jitter_dir(pixel_dir) themselves: the pose branch costs them registers (one wave of occupancy in render_persistent's counting instantiation).
__device__ __forceinline__ f3 camera_dir(const Frame &fr, f3 C, float z, int px, int row, uint32_t hs) {
    f3 v = pixel_dir(fr, px, row, z);
    if (fr.cam_mode == 1) v = posed_dir(fr, C, v);
    return jitter_dir(fr, v, hs);
}
// The THIN LENS (rt_camera_set_lens; the rule: raytrace_hip.h "thin lens"): the camera ray (O, u) of the sample with key hs becomes the ray from a point of the lens -- the
// disc of radius R about O, perpendicular to the view axis a -- through the point where (O, u) meets the plane of focus at distance f along a.  The two draws sit at depth
// 2^28 (the RNG keys on depth * 4 + dim modulo 2^32: 2^30 + dim, which no jitter, bounce, pick or shell draw reaches), in the forms cosine_bounce uses.  A ray that does not
// look along the axis (c <= 0 or a NaN) stays as it is.  The fixed camera's basis is the literal one in the same expressions: a -0 coordinate of O may become +0.
__device__ __forceinline__ void lens_ray(const Frame &fr, float R, float f, uint32_t hs, f3 &O, f3 &u) {
    const bool posed = fr.cam_mode == 1;
    const f3 ex = posed ? mk(fr.bx[0], fr.bx[1], fr.bx[2]) : mk(1.f, 0.f, 0.f);
    const f3 ey = posed ? mk(fr.by[0], fr.by[1], fr.by[2]) : mk(0.f, 1.f, 0.f);
    const f3 a = posed ? mk(-fr.bz[0], -fr.bz[1], -fr.bz[2]) : mk(0.f, 0.f, -1.f);   // z is negative: the view axis is -bz
    const float c = dot(u, a);
    if (!(c > 0.f)) return;
    const float t = f / c;
    const f3 F = O + t * u;
    const float r1 = uniform01(hs, 1u << 28, 0);
    const float r2 = uniform01(hs, 1u << 28, 1);
    const float s = rt_sqrtf(r1);                                     // (0, 1]: uniform on the disc by area
    double sn, cs;
    rt_sincos_2pi(2 * 3.14159265358979323846 * (double)r2, sn, cs);
    const float dx = (float)(cs * (double)s);
    const float dy = (float)(sn * (double)s);
    const float lx = R * dx, ly = R * dy;
    O = (O + lx * ex) + ly * ey;
    u = normalize(F - O);
}
// The SHUTTER (rt_scene_set_shutter; the rule: raytrace_hip.h "shutter"): the time of the sample with key hs, in (0, 1] -- the one draw at depth 2^28, dim 2 (key 2^30 + 2,
// beside the lens's two) -- and where a point that travels d over the exposure is at that time: C + d tau per component, the product first, each rounded once
// (MoveObject's arithmetic, realtime:1096).  Every launch of a path draws tau again from hs: no path state grows.
__device__ __forceinline__ float shutter_time(uint32_t hs) { return uniform01(hs, 1u << 28, 2); }
__device__ __forceinline__ f3 shutter_pose(f3 C, f3 d, float tau) { return mk(C.x + d.x * tau, C.y + d.y * tau, C.z + d.z * tau); }

// ---- texel coordinates (the textures of rt_wavefront.hip.h and the environment map below) ----
// floor of a texel coordinate as an int, and the fraction c - floor(c).  A coordinate outside [-2^31, 2^31) -- NaN and +-inf included -- is index 0 with fraction 0.
__device__ __forceinline__ int tex_floor(float c, float &frac) {
    const bool ok = c >= -2147483648.f && c < 2147483648.f;
    const float f = floorf(c);
    frac = ok ? c - f : 0.f;
    return ok ? (int)f : 0;
}
__device__ __forceinline__ int tex_wrap(int i, int n, int wrap) {
    if (wrap != 0) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);        // clamp
    const int r = i % n;                                               // repeat: non-negative modulo
    return r < 0 ? r + n : r;
}

// The ENVIRONMENT (rt_scene_set_environment; the rule: raytrace_hip.h "environment"): the radiance a ray of direction u meets when it leaves the scene.  The map is n x n
// float4 texels (w unused), octahedral with +y as the pole: no transcendental function, every operation one binary32 rounding, the two quotients correctly rounded
// (rt_div.h: one reciprocal for both, the literal divisions outside its range).  Bilinear in tex_sample's form, clamped at the border.  A direction whose 1-norm is not a
// finite number above 0 meets nothing: +0.  The map is small and read again and again: plain loads, no stream policy.  (n <= 1024: the index mask says so to the compiler.)
struct WfSky { const float4 *texels; int n; };
__device__ __forceinline__ f3 sky_radiance(const WfSky &sky, f3 u) {
    const float s = (fabsf(u.x) + fabsf(u.y)) + fabsf(u.z);
    if (!(s > 0.f && s < __builtin_inff())) return mk(0.f, 0.f, 0.f);
    const bool fast = div_in_range(u.x) && div_in_range(u.z) && div_in_range(s);
    const float r1 = div_refine(s, __builtin_amdgcn_rcpf(s));
    float px = div_by(u.x, s, r1), pz = div_by(u.z, s, r1);
    if (__builtin_expect(__ballot(!fast) != 0ull, 0)) {
        if (!fast) { px = u.x / s; pz = u.z / s; }
    }
    float qx = px, qz = pz;
    if (u.y < 0.f) {                                                   // the lower hemisphere folds outwards, to the corners
        qx = (1.f - fabsf(pz)) * (px < 0.f ? -1.f : 1.f);
        qz = (1.f - fabsf(px)) * (pz < 0.f ? -1.f : 1.f);
    }
    const float a = qx * 0.5f + 0.5f, b = qz * 0.5f + 0.5f;            // [0, 1]: the centre is the zenith, row 0 is -z
    const int n = sky.n;
    const float nf = (float)n;
    float fx, fy;
    const int x0 = tex_floor(a * nf - 0.5f, fx), y0 = tex_floor(b * nf - 0.5f, fy);
    const int xa = tex_wrap(x0, n, 1), xb = tex_wrap(x0 + 1, n, 1), ya = tex_wrap(y0, n, 1), yb = tex_wrap(y0 + 1, n, 1);
    constexpr unsigned kMask = (1u << 20) - 1;                         // n * n - 1 at n = 1024
    const float4 t00 = sky.texels[(unsigned)(ya * n + xa) & kMask], t10 = sky.texels[(unsigned)(ya * n + xb) & kMask];
    const float4 t01 = sky.texels[(unsigned)(yb * n + xa) & kMask], t11 = sky.texels[(unsigned)(yb * n + xb) & kMask];
    const float gx = 1.f - fx, gy = 1.f - fy;
    return mk((t00.x * gx + t10.x * fx) * gy + (t01.x * gx + t11.x * fx) * fy,
              (t00.y * gx + t10.y * fx) * gy + (t01.y * gx + t11.y * fx) * fy,
              (t00.z * gx + t10.z * fx) * gy + (t01.z * gx + t11.z * fx) * fy);
}

// SKY SAMPLING (rt_scene_set_environment_sampling; the rule: raytrace_hip.h "sky sampling"): a direction drawn from the map by radiance.  The table is integers -- c(t) per
// texel, its inclusive 64-bit sums, their total -- built on the device (rt_skydist.hip.h), so the texel of a draw is a function of the table alone.  blk is the coarse
// level of the search: the prefix at the last texel of every kSkyBlock texels (at most 4096 words, 32 KB: they stay in cache), then a search inside one block.
constexpr int kSkyBlock = 256;
struct WfSkyDist {
    const unsigned long long *prefix;        // [n * n] inclusive sums of c, texel t = y * n + x
    const unsigned long long *blk;           // [nb] blk[b] = prefix[min((b + 1) * kSkyBlock, n * n) - 1]
    const unsigned int *c;                   // [n * n]
    unsigned long long total;                // prefix[n * n - 1], in [1, 2^51]
    int n, nb;
    // ... and what a frame's sampling forms take with it (wf_advance<kFormSkySample>; zero in the known-answer entries): the effective share s in (0, 1], the two
    // weights fl(1 / s) and fl(1 / (1 - s)) (the latter unused at s = 1), and the three-channel direct term of diffuse segment d of path i, L3[d * n_paths + i]
    float s, w_sky, w_light;
    float4 *L3;
};
// the 24-bit integer k behind a draw: uniform01 = (k + 1) * 2^-24
__device__ __forceinline__ uint32_t uniform24(uint32_t hs, uint32_t depth, uint32_t dim) { return mix32(hs ^ ((depth * 4U + dim) * 0x85EBCA77U)) >> 8; }
// q = 2 a - 1 with a = fl(xs / n), the quotient correctly rounded (2 a is exact: one rounding each)
__device__ __forceinline__ float sky_q(float xs, float nf) { return div_quot(xs, nf) * 2.f - 1.f; }
// the octahedral point of (qx, qz), 1-norm 1, not normalised: py = fl(fl(1 - |qx|) - |qz|) in both hemispheres, and where py < 0 the fold of sky_radiance's step 3 undone
__device__ __forceinline__ f3 sky_oct_point(float qx, float qz) {
    const float h = (1.f - fabsf(qx)) - fabsf(qz);
    float px = qx, pz = qz;
    if (h < 0.f) {
        px = (1.f - fabsf(qz)) * (qx < 0.f ? -1.f : 1.f);
        pz = (1.f - fabsf(qx)) * (qz < 0.f ? -1.f : 1.f);
    }
    return mk(px, h, pz);
}
// the least texel t with prefix[t] >= X, for X in [1, total]: the least block whose last prefix reaches X, then the least texel inside it.  Every index stays inside
// [0, nb) and [0, n * n) whatever X is.
// FLAT: one binary search over all n * n prefixes, 20 dependent loads at n = 1024 (RT_SKY_SEARCH=0: the form the two levels are measured against; the same texel).
template <bool FLAT = false>
__device__ __forceinline__ unsigned int sky_pick(const WfSkyDist &sd, unsigned long long X) {
    int lo = 0, hi = sd.nb - 1;
    while (!FLAT && lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sd.blk[mid] >= X) hi = mid; else lo = mid + 1;
    }
    const int count = sd.n * sd.n;
    int tlo = lo * kSkyBlock, thi = tlo + kSkyBlock < count ? tlo + kSkyBlock - 1 : count - 1;
    if (FLAT) { tlo = 0; thi = count - 1; }
    while (tlo < thi) {
        const int mid = (tlo + thi) >> 1;
        if (sd.prefix[mid] >= X) thi = mid; else tlo = mid + 1;
    }
    return (unsigned int)tlo;
}
// the draw of segment `seg` of the path whose sample key is hs: the texel, the unit direction, and m = |p|^2, r = |p| of the octahedral point p behind it
struct SkyDraw { unsigned int t; f3 w; float m, r; };
template <bool FLAT = false>
__device__ __forceinline__ SkyDraw sky_draw(const WfSkyDist &sd, uint32_t hs, int seg) {
    const uint32_t depth = (3u << 28) + (uint32_t)seg;
    const unsigned long long K = ((unsigned long long)uniform24(hs, depth, 0) << 24) | (unsigned long long)uniform24(hs, depth, 1);
    const unsigned long long X = ((__umul64hi(K, sd.total) << 16) | ((K * sd.total) >> 48)) + 1ull;   // (K total >> 48) + 1: K < 2^48 and total <= 2^51, the high word is below 2^35
    SkyDraw s;
    s.t = sky_pick<FLAT>(sd, X);
    const unsigned int y = s.t / (unsigned int)sd.n, x = s.t - y * (unsigned int)sd.n;
    const float nf = (float)sd.n;
    const float jx = uniform01(hs, depth, 2), jz = uniform01(hs, depth, 3);
    const f3 p = sky_oct_point(sky_q((float)x + jx, nf), sky_q((float)y + jz, nf));
    s.m = norm2(p);
    s.w = normalize(p, s.r);
    return s;
}
// g = mx / pdf in binary64, rounded once: pdf = c(t) / total * n^2 / 4 * |p|^3
__device__ __forceinline__ float sky_weight(const WfSkyDist &sd, unsigned int t, float m, float r, float mx) {
    const double num = ((double)mx * 4.0) * (double)sd.total;
    const double den = (((double)sd.c[t] * (double)(sd.n * sd.n)) * (double)m) * (double)r;
    return (float)(num / den);
}

// EMISSIVE MESHES (rt_scene_set_emission; the rule: raytrace_hip.h "emissive meshes"): a point drawn from the emitting triangles by area times radiance.  The table has the
// sky table's form -- c(t) per triangle of the scene in stored (visit) order, its inclusive 64-bit sums, their total, a block level of kSkyBlock -- and is built by the
// same kernels from other weights (rt_skydist.hip.h emit_dist_weights).
struct WfEmit {
    const unsigned long long *prefix;        // [nt] inclusive sums of c, triangle t in visit order (Scene::tri)
    const unsigned long long *blk;           // [nb] blk[b] = prefix[min((b + 1) * kSkyBlock, nt) - 1]
    const unsigned int *c;                   // [nt]
    const float4 *le;                        // [kMaxObjects] by OBJECT position: (Le r, g, b, Y = fl(fl(r + g) + b)); zeros for what does not emit
    unsigned long long total;                // prefix[nt - 1], in [1, 2^51]; 0: no table (then s is 0 and nothing above is read)
    int nt, nb;
    // ... and what a frame's emission forms take with it (wf_advance<kFormEmit>; zero in the known-answer entries): the effective share s in [0, 1], the two weights
    // fl(1 / s) and fl(1 / (1 - s)) (each unused where its rays are never drawn), the mask of the emitting object positions, and per diffuse segment d of path i
    // L3[d * n_paths + i] = (the three-channel direct term, norm2(L' - Pa): the far end of the segment's shadow ray as light_hidden compares it)
    float s, w_emit, w_light;
    unsigned int mask;
    float4 *L3;
};
constexpr float kEmitKappa = 0x1p-10f;       // a shadow ray towards the point Q of an emitter aims at L' = Q + kappa (Pa - Q): raytrace_hip.h "emissive meshes" says why
// the least triangle t with prefix[t] >= X, for X in [1, total] (so c(t) > 0): sky_pick's two levels over nt entries; every index stays inside [0, nb) and [0, nt)
__device__ __forceinline__ unsigned int emit_pick(const WfEmit &em, unsigned long long X) {
    int lo = 0, hi = em.nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (em.blk[mid] >= X) hi = mid; else lo = mid + 1;
    }
    int tlo = lo * kSkyBlock, thi = tlo + kSkyBlock < em.nt ? tlo + kSkyBlock - 1 : em.nt - 1;
    while (tlo < thi) {
        const int mid = (tlo + thi) >> 1;
        if (em.prefix[mid] >= X) thi = mid; else tlo = mid + 1;
    }
    return (unsigned int)tlo;
}
// the draw of segment `seg` of the path whose sample key is hs: the triangle, the point Q on it, and the record's raw normal Nt = cross(e1, e2)
struct EmitDraw { unsigned int t; f3 Q, Nt; };
__device__ __forceinline__ EmitDraw emit_draw(const WfEmit &em, const float4 *__restrict__ tri, uint32_t hs, int seg) {
    const uint32_t depth = (1u << 27) + (uint32_t)seg;
    const unsigned long long K = ((unsigned long long)uniform24(hs, depth, 0) << 24) | (unsigned long long)uniform24(hs, depth, 1);
    const unsigned long long X = ((__umul64hi(K, em.total) << 16) | ((K * em.total) >> 48)) + 1ull;   // (K total >> 48) + 1, as sky_draw
    EmitDraw s;
    s.t = emit_pick(em, X);
    float r1 = uniform01(hs, depth, 2), r2 = uniform01(hs, depth, 3);
    if (r1 + r2 > 1.f) { r1 = 1.f - r1; r2 = 1.f - r2; }               // the other half of the parallelogram, folded back
    const float4 q0 = tri[3 * (size_t)s.t], q1 = tri[3 * (size_t)s.t + 1], q2 = tri[3 * (size_t)s.t + 2];
    const f3 A = mk(q0.x, q0.y, q0.z), e1 = mk(q0.w, q1.x, q1.y), e2 = mk(q1.z, q1.w, q2.x);
    s.Q = (A + r1 * e1) + r2 * e2;
    s.Nt = mk(q2.y, q2.z, q2.w);
    return s;
}
// g = mx cl / d2 over the area density c(t) / total * 2 / A2, in binary64, rounded once: mx = max(dot(N, wl), 0) at the shaded point, wl the unit vector towards Q,
// d2 = |Q - P|^2, cl = |dot(normalize(Nt), wl)| and A2 = rt_sqrtf(norm2(Nt)) (twice the triangle's area)
__device__ __forceinline__ float emit_weight(const WfEmit &em, const EmitDraw &s, f3 wl, float d2, float mx) {
    float A2;                                                          // (normalize's own norm: rt_sqrtf(norm2(Nt)))
    const float cl = fabsf(dot(normalize(s.Nt, A2), wl));
    const double num = (((double)mx * (double)cl) * (double)A2) * (double)em.total;
    const double den = (2.0 * (double)em.c[s.t]) * (double)d2;
    return (float)(num / den);
}

// ---- the hit ----
// alpha, beta, gamma of triangle `tri` (visit order) for the ray (O, u): get_smooth_normal's expressions (realtime_render.cu:221-245).  The smooth normal, the
// texture lookup (tex_albedo, rt_wavefront.hip.h) and rt_kat_surface read these.
struct Bary { float alpha, beta, gamma; };
__device__ __forceinline__ Bary tri_bary(const Scene &sc, int tri, f3 O, f3 u) {
    const float4 q0 = sc.tri[3 * tri], q1 = sc.tri[3 * tri + 1], q2 = sc.tri[3 * tri + 2];
    const f3 A = mk(q0.x, q0.y, q0.z), e1 = mk(q0.w, q1.x, q1.y), e2 = mk(q1.z, q1.w, q2.x), Nt = mk(q2.y, q2.z, q2.w);
    Bary b;
    b.beta = dot(e2, cross(A - O, u)) / dot(u, Nt);
    b.gamma = -dot(e1, cross(A - O, u)) / dot(u, Nt);
    b.alpha = 1 - b.beta - b.gamma;
    return b;
}
// The unit normal of a hit, three ways.  Does object `win`, hit on triangle `tri_win` (visit order; < 0: a sphere), shade with interpolated vertex normals?
__device__ __forceinline__ bool smooth_hit(const Scene &sc, int win, int tri_win) { return tri_win >= 0 && sc.nrm != nullptr && ((sc.smooth_mask >> win) & 1); }
// get_smooth_normal (realtime_render.cu:221-245) for the ray (O, u); hands back the barycentrics it formed
__device__ __forceinline__ f3 smooth_normal(const Scene &sc, int tri, f3 O, f3 u, Bary &bary) {
    bary = tri_bary(sc, tri, O, u);
    const float4 na = sc.nrm[3 * tri], nb = sc.nrm[3 * tri + 1], nc = sc.nrm[3 * tri + 2];
    return normalize((bary.alpha * mk(na.x, na.y, na.z) + bary.beta * mk(nb.x, nb.y, nb.z)) + bary.gamma * mk(nc.x, nc.y, nc.z));
}
__device__ __forceinline__ f3 flat_normal(const Scene &sc, int tri) { const float4 q2 = sc.tri[3 * tri + 2]; return normalize(mk(q2.y, q2.z, q2.w)); }   // cpu:308
__device__ __forceinline__ f3 sphere_normal(const Scene &sc, int obj, f3 P) { return normalize(P - sphere_centre_of(sc, obj)); }                      // cpu:524-525
// ... and the choice between them for the hit P of ray (O, u).  (wf_path spells the same choice out around its index checks; as one call there it costs scalar
// registers: 14 more kernel-argument reloads, 1.6 % of its frame time.)
__device__ __forceinline__ f3 hit_normal(const Scene &sc, int win, int tri_win, f3 O, f3 u, f3 P, Bary &bary, bool &have_bary) {
    have_bary = smooth_hit(sc, win, tri_win);
    if (have_bary) return smooth_normal(sc, tri_win, O, u, bary);
    return tri_win >= 0 ? flat_normal(sc, tri_win) : sphere_normal(sc, win, P);
}

// ---- Scene::getColor's branches ----
// cpu:573-579: the ray (O, u) that hit a mirror at P with normal N becomes the reflected ray
__device__ __forceinline__ void mirror_step(float eps, f3 P, f3 N, f3 &O, f3 &u) {
    O = P + eps * N;
    u = u - (2 * dot(u, N)) * N;
}
// cpu:580-604: the same at a surface with n_in != n_out, for a ray whose Ray::refraction_index is `refr`: total reflection, or the refracted ray.  crossed: the ray
// went through the surface, and its index is now refr_after = out2in ? n_in : n_out (out2in: it came from the n_out side).
struct Refraction { bool crossed, out2in; float refr_after; };
__device__ __forceinline__ Refraction refract_step(const Material &m, float refr, float eps, f3 P, f3 N, f3 &O, f3 &u) {
    Refraction r;
    float ratio;
    r.out2in = refr == m.n_out;
    if (r.out2in) ratio = m.n_out / m.n_in;
    else { ratio = m.n_in / m.n_out; N = -N; }
    const float un = dot(u, N);
    if (((r.out2in && refr > m.n_in) || (!r.out2in && refr > m.n_out)) && (ratio * ratio) * (1 - un * un) > 1) {
        O = P + eps * N;
        u = u - (2 * un) * N;
        r.crossed = false;
        r.refr_after = refr;
    } else {
        O = P - eps * N;
        const f3 Nc = (-rt_sqrtf(1 - (ratio * ratio) * (1 - un * un))) * N;
        const f3 Tc = ratio * (u - un * N);
        u = Nc + Tc;
        r.crossed = true;
        r.refr_after = r.out2in ? m.n_in : m.n_out;
    }
    return r;
}
// FRESNEL DIELECTRICS (rt_material_set_fresnel; the rule: raytrace_hip.h "fresnel"): refract_step for a flagged object -- outside total reflection the ray is reflected
// with probability R, the unpolarised Fresnel reflectance of the interface, and refracted otherwise; either ray carries weight 1, so nothing of the path's state grows.
// The one draw sits at depth 2^26 + seg (key 2^28 + 4 seg).  A NaN R refracts (r_f <= NaN is false): the reference's ray.
struct WfFresnel { unsigned int mask; };     // bit k: the object at position k is EFFECTIVELY flagged (its bit is set, mirror == 0 and n_in != n_out: formed on the host)
constexpr int kFresnelRefracted = 0, kFresnelReflected = 1, kFresnelTotal = 2;
__device__ __forceinline__ float fresnel_reflectance(float n1, float n2, float ci, float ct) {
    const float a = n1 * ci, b = n2 * ct, c = n1 * ct, e = n2 * ci;
    const float rs = (a - b) / (a + b), rp = (c - e) / (c + e);
    return 0.5f * (rs * rs + rp * rp);
}
// R: the reflectance (+0 where the ray is totally reflected: none is formed); code: kFresnel*
struct FresnelStep { Refraction r; float R; int code; };
__device__ __forceinline__ FresnelStep fresnel_step(const Material &m, float refr, float eps, f3 P, f3 N, f3 &O, f3 &u, uint32_t hs, int seg) {
    FresnelStep s;
    Refraction &r = s.r;
    float ratio;
    r.out2in = refr == m.n_out;
    if (r.out2in) ratio = m.n_out / m.n_in;
    else { ratio = m.n_in / m.n_out; N = -N; }
    const float un = dot(u, N);
    const float k = (ratio * ratio) * (1 - un * un);
    s.R = 0.f;
    bool reflect = ((r.out2in && refr > m.n_in) || (!r.out2in && refr > m.n_out)) && k > 1;
    s.code = reflect ? kFresnelTotal : kFresnelRefracted;
    const float ct = rt_sqrtf(1 - k);                                  // (a NaN under total reflection: not read there)
    if (!reflect) {
        s.R = fresnel_reflectance(r.out2in ? m.n_out : m.n_in, r.out2in ? m.n_in : m.n_out, fabsf(un), ct);
        reflect = uniform01(hs, (1u << 26) + (uint32_t)seg, 0) <= s.R;
        if (reflect) s.code = kFresnelReflected;
    }
    if (reflect) {
        O = P + eps * N;
        u = u - (2 * un) * N;
        r.crossed = false;
        r.refr_after = refr;
    } else {
        O = P - eps * N;
        const f3 Nc = (-ct) * N;
        const f3 Tc = ratio * (u - un * N);
        u = Nc + Tc;
        r.crossed = true;
        r.refr_after = r.out2in ? m.n_in : m.n_out;
    }
    return s;
}

// cpu:614: the shadow ray from P_adjusted to the light, NORMED_VEC (cpu:30): (L - Pa) / nl with nl = sqrt(norm2(L - Pa))
__device__ __forceinline__ f3 shadow_dir(f3 L, f3 Pa, float &nl) { return normalize(L - Pa, nl); }
__device__ __forceinline__ f3 shadow_dir(f3 L, f3 Pa) { float nl; return shadow_dir(L, Pa, nl); }
// cpu:615: is the light hidden from P_adjusted, given the shadow ray's nearest hit point Pp (cpu:560) -- or its ray (Pa, u) and the hit's t?
__device__ __forceinline__ bool light_hidden(f3 Pa, f3 Pp, f3 L) { return norm2(Pp - Pa) <= norm2(L - Pa); }
__device__ __forceinline__ bool light_hidden(f3 Pa, f3 u, float t, f3 L) { return light_hidden(Pa, Pa + t * u, L); }
// ... with the right-hand side norm2(L - Pa) formed where the ray was emitted and carried to its close (the emission forms: WfEmit::L3's fourth word)
__device__ __forceinline__ bool light_hidden_far2(f3 Pa, f3 u, float t, float far2) { return norm2((Pa + t * u) - Pa) <= far2; }
// cpu:620-623: the scalar l of a diffuse hit at P with normal N under a visible light (the quotient and the product in binary64, as the reference's promotions make them)
__device__ __forceinline__ float direct_term(float intensity, f3 L, f3 P, f3 N) {
    const f3 wl = normalize(L - P);
    const float dn = dot(N, wl);
    const float mx = (dn < 0.f) ? 0.f : dn;                           // std::max(dn, 0.f)
    return (float)((double)intensity / (4 * 3.14159265358979323846 * (double)norm2(L - P)) * (double)mx);   // cpu:623
}
__device__ __forceinline__ float direct_term(const Scene &sc, f3 L, f3 P, f3 N) { return direct_term(sc.intensity, L, P, N); }
// cpu:627-641: the cosine-weighted direction about N of segment d's bounce, from the sample key's dims 0, 1 at depth d
__device__ __forceinline__ f3 cosine_bounce(f3 N, uint32_t hs, int d) {
    const float r1 = uniform01(hs, (uint32_t)d, 0);                   // cpu:628-629
    const float r2 = uniform01(hs, (uint32_t)d, 1);
    double sn, cs;
    rt_sincos_2pi(2 * 3.14159265358979323846 * (double)r1, sn, cs);
    const float s1 = rt_sqrtf(1 - r2);
    const float x = (float)(cs * (double)s1);                         // cpu:630
    const float y = (float)(sn * (double)s1);                         // cpu:631
    const float zz = rt_sqrtf(r2);                                    // cpu:632
    // T1 = normalize((-Ny, Nx, 0)) if Nx != 0 && Ny != 0 else normalize((-Nz, 0, Nx)) (cpu:634-638): two quotients, the third component is +0 / n
    const bool t1a = N.y != 0 && N.x != 0;
    float t1p, t1q, t1z;
    normalize_pq0(t1a ? -N.y : -N.z, N.x, t1p, t1q, t1z);
    const f3 T1 = t1a ? mk(t1p, t1q, t1z) : mk(t1p, t1z, t1q);
    const f3 T2 = cross(N, T1);
    return x * T1 + y * T2 + zz * N;                                  // cpu:641
}
// ROUGH MIRRORS (rt_material_set_roughness; the rule: raytrace_hip.h "roughness"): mirror_step for an object with an effective roughness alpha -- the ray is reflected
// about a facet normal h drawn from the GGX distribution D(h) (n.h) of width alpha about N, from the two draws at depth 2^25 + seg (keys 2^27 + 4 seg + {0, 1}), in
// cosine_bounce's forms and tangent frame; a ray the facet sends into the surface is mirrored back out about N.  The ray carries weight 1: nothing of the path's state
// grows.  1 - r1 is exact, the denominator is >= 1 - r1 > 0 or 2^-24 at r1 = 1: c2 is in [0, 1] and neither root sees a negative operand.
constexpr int kGlossPlain = 0, kGlossFolded = 1;
// h: the facet's normal; code: kGloss*
struct GlossStep { f3 h; int code; };
__device__ __forceinline__ GlossStep gloss_step(float eps, float alpha, f3 P, f3 N, f3 &O, f3 &u, uint32_t hs, int seg) {
    GlossStep g;
    const float un = dot(u, N);
    O = P + eps * N;
    const float r1 = uniform01(hs, (1u << 25) + (uint32_t)seg, 0);
    const float r2 = uniform01(hs, (1u << 25) + (uint32_t)seg, 1);
    const float a2 = alpha * alpha;
    const float m = a2 - 1;
    const float c2 = (1 - r1) / (1 + m * r1);
    const float c = rt_sqrtf(c2);
    const float s = rt_sqrtf(1 - c2);
    double sn, cs;
    rt_sincos_2pi(2 * 3.14159265358979323846 * (double)r2, sn, cs);
    const float x = (float)(cs * (double)s);
    const float y = (float)(sn * (double)s);
    const bool t1a = N.y != 0 && N.x != 0;                            // cosine_bounce's tangent frame
    float t1p, t1q, t1z;
    normalize_pq0(t1a ? -N.y : -N.z, N.x, t1p, t1q, t1z);
    const f3 T1 = t1a ? mk(t1p, t1q, t1z) : mk(t1p, t1z, t1q);
    const f3 T2 = cross(N, T1);
    g.h = x * T1 + y * T2 + c * N;
    u = u - (2 * dot(u, g.h)) * g.h;
    const float vn = dot(u, N);
    g.code = kGlossPlain;
    if (vn != 0 && (vn < 0) == (un < 0)) {                            // the facet sent the ray into the surface: back out
        u = u - (2 * vn) * N;
        g.code = kGlossFolded;
    }
    return g;
}
// cpu:624, 642-644: the colour of a path from a diffuse segment on -- its direct light l * albedo / pi plus albedo (.) the colour `ans` of what follows it
__device__ __forceinline__ f3 fold_segment(f3 ans, float l, f3 alb) {
    const float PI_F = (float)3.14159265358979323846;
    return (l * alb) / PI_F + alb * ans;
}
// ... with a direct term per channel (sky sampling: the environment's estimate has three); (l, l, l) gives the same words as the scalar form
__device__ __forceinline__ f3 fold_segment(f3 ans, f3 l, f3 alb) {
    const float PI_F = (float)3.14159265358979323846;
    return (l * alb) / PI_F + alb * ans;
}

}  // namespace rtk
