// rt_deadlast.h -- DEAD LAST: whether a launch chain may leave the last continuation ray of a path whose three colour channels are dead out of the traversal
// (rt_wavefront.hip.h kPolDeadLast, DESIGN.md section 5.1 "Dead paths").  Decided on the host at EVERY enqueue from the Scene the launches are about to take, never kept
// between calls: no edit entry can leave it stale.
//
// What the device rule does: a path with every channel dead (wf_dead_channels) whose last continuation ray certainly hits a SPHERE is closed by the next launch as that
// sphere's hit, whatever the mesh would have said.  The pixel needs two things of the segment so shaded: a ray count, and an `ans` that is FINITE -- every channel's kill
// sits at an earlier segment and hands up fl(fl(l (+0)) / pi) + fl((+0) x) = +0 for any finite x.  Both must hold for the object the reference's ray really hits (any
// sphere, any triangle) and for the sphere the kernel shades in its place; only the scene can promise that:
//   (1) every object is DIFFUSE by the kernel's own test (!mirror && n_in == n_out): the hit, whichever it is, adds exactly one shadow ray and no further ray;
//   (2) every object's three albedo components lie in [+0, 1] as bits (the guard of wf_dead_channels): fl(l alb) / pi + alb (+0) is finite for a finite l;
//   (2b) no mesh shades with VERTEX NORMALS (Scene::smooth_mask == 0, Scene::nrm == nullptr): a smooth normal is normalize(a Na + b Nb + c Nc) of normals nobody
//       validates -- corner normals that cancel or are zero (rt_mesh_compute_normals writes (0,0,0) where faces cancel), a caller's NaN -- so the reference's hit on such a
//       triangle has N = NaN, mx = NaN and a NaN pixel where the sphere shaded in its place gives +0.  A flat normal is the hit triangle's own e1 x e2;
//   (3) THE LIGHT: the direct term l = fl(intensity / (4 pi |L - P|^2) mx) (direct_term, binary64 inside, mx = max(N . wl, 0) <= 1 + 2^-21) is finite and below 2^96
//       at every point P a hit can compute.
// The bound of (3) and its error budget.  Let S be the radius of a ball about the origin that holds every sphere, every mesh's root box and the light, and dmin the
// smallest distance from L to a sphere's surface (| |L - C| - R |) and to a root box (0 inside: refused).  A computed hit point is P = fl(O + fl(t u)) with O on a surface
// (|O| <= S: the ray in question leaves a diffuse hit) and the true hit inside the ball:
//   - a sphere's t = -d -+ sqrt(d^2 - c), c = |O - C|^2 - R2 (sphere_dir): with D = |O - C| <= 2 S, c carries at most 6 * 2^-24 D^2 of rounding, d^2 at most 2^-21 D^2, so
//     the discriminant is off by less than 2^-20 D^2 and its root by less than 2^-10 D (|sqrt(a + e) - sqrt(a)| <= sqrt|e|, the grazing ray's case); d itself by 2^-22 D:
//     |t - t_true| < 2^-9 S (1 + 2^-8) -- with the roundings of the last line below, 2^-9 S (1 + 2^-7);
//   - a triangle's t is TAKEN to obey the same budget (an accepted hit's point lies in its leaf's box, inside the root box, to that accuracy), and its flat normal to
//     be finite.  This is an assumption, not a bound: a triangle accepted with a determinant at the edge of binary32 can have a t that is off by more, or a cross
//     product that underflows to zero.  The rule is exact for sphere hits by construction and for triangle hits up to this assumption;
//   - the roundings of O + t u add 3 * 2^-24 * 3 S, and |u| <= 1 + 2^-22.
// So P lies within 2^-9 S (1 + 2^-7) of a surface point or of the root box; the MARGIN taken is twice that and more, 2^-8 S, and de = dmin - margin must stay positive
// (and above 1e-12: no square of the budget is denormal, as in wf_anyhit_bound).  Then |L - P| >= de, the binary32 norm2(L - P) >= de^2 (1 - 2^-20), and
//   l <= intensity (1 + 2^-20) / (4 pi de^2)  -- required below 2^96 with a further factor 1.001 to spare; intensity itself finite with a clear sign bit.
// A light that fails any of it -- inside a root box, on or within the margin of a surface, non-finite, too bright for its distance -- REFUSES: every ray is traced as before.
// Plain C++: the library and the host library (rth_dead_last_permit, tests/test_dead_last_guard.py) compile the same text.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace rtk {

constexpr int kDeadLastMaxObjects = 16;              // kMaxSpheres, RT_MAX_OBJECTS

// What the permission reads of a Scene, as plain numbers (rt_host_render.hip.h dead_last_scene fills it from the rtk::Scene of the launch)
struct DeadLastScene {
    int n_spheres, n_objects;
    float sph[kDeadLastMaxObjects][4];               // (centre, R) of sphere k, in the order of Scene::sph
    float alb[kDeadLastMaxObjects][3];               // by OBJECT id: albedo,
    int mirror[kDeadLastMaxObjects];                 // ... mirror,
    float n_in[kDeadLastMaxObjects], n_out[kDeadLastMaxObjects];   // ... the two indices
    float L[3], intensity;
    int have_box;                                    // the scene has a mesh to traverse: the root box below
    float lo[3], hi[3];
    int smooth;                                      // some mesh shades with vertex normals (Scene::smooth_mask != 0 or Scene::nrm != nullptr)
};

inline uint32_t dead_last_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the scene-level conditions (1) - (3)
inline bool dead_last_scene_ok(const DeadLastScene &s) {
    if (s.smooth != 0) return false;                                                             // (2b)
    if (s.n_spheres < 0 || s.n_spheres > kDeadLastMaxObjects || s.n_objects < 0 || s.n_objects > kDeadLastMaxObjects) return false;
    for (int k = 0; k < s.n_objects; ++k) {
        if (s.mirror[k] != 0 || !(s.n_in[k] == s.n_out[k])) return false;                        // (1), the kernel's test: a NaN index is not diffuse there either
        for (int c = 0; c < 3; ++c) if (dead_last_bits(s.alb[k][c]) > 0x3f800000u) return false;   // (2): bits of 1; a negative number, -0, inf and every NaN lie above
    }
    if (dead_last_bits(s.intensity) >= 0x7f800000u) return false;                                // finite, sign bit clear
    const double Lx = s.L[0], Ly = s.L[1], Lz = s.L[2];
    double S = sqrt(Lx * Lx + Ly * Ly + Lz * Lz), dmin = INFINITY;
    if (!isfinite(S)) return false;
    for (int k = 0; k < s.n_spheres; ++k) {
        const double cx = s.sph[k][0], cy = s.sph[k][1], cz = s.sph[k][2], R = s.sph[k][3];
        if (!isfinite(cx) || !isfinite(cy) || !isfinite(cz) || !isfinite(R) || !(R > 0.0)) return false;
        S = fmax(S, sqrt(cx * cx + cy * cy + cz * cz) + R);
        const double dx = Lx - cx, dy = Ly - cy, dz = Lz - cz;
        dmin = fmin(dmin, fabs(sqrt(dx * dx + dy * dy + dz * dz) - R));
    }
    if (s.have_box) {
        double far2 = 0.0, out2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double lo = s.lo[c], hi = s.hi[c], l = s.L[c];
            if (!isfinite(lo) || !isfinite(hi) || !(lo <= hi)) return false;
            far2 += fmax(lo * lo, hi * hi);
            const double o = l < lo ? lo - l : l > hi ? l - hi : 0.0;
            out2 += o * o;
        }
        S = fmax(S, sqrt(far2));
        dmin = fmin(dmin, sqrt(out2));                                                           // 0: the light is inside the box or on it
    }
    if (!(S < 1e18)) return false;                                                               // no square of a coordinate overflows binary32
    const double de = dmin - S * 0x1p-8;                                                         // the margin
    if (!(de > 1e-12)) return false;                                                             // (a scene without any surface: dmin = inf, nothing to hit, nothing to refuse)
    return (double)s.intensity * 1.001 / (4 * 3.14159265358979323846 * de * de) < 0x1p96;
}

// The permission of one chain: a plain chain (rt_still.h adv_plain_chain on the work-stack traversal), any-hit and the dead-channel rule on, the knob RT_DEAD_LAST not 0,
// and the scene's conditions.  A counting chain carries the same bit and COUNTS the rays the rule would leave out; it traces them all.
inline bool dead_last_permit(bool plain, bool anyhit, bool deadch, int knob, const DeadLastScene &s) {
    return plain && anyhit && deadch && knob != 0 && dead_last_scene_ok(s);
}

}  // namespace rtk
