// rt_still.h -- what a launch chain of a STILL VIEW may skip: the state of the three levels kept between frames, and the launches of one chain.
//
// With sigma == 0 the start of every path repeats from frame to frame as long as nothing it depends on changes.  Three levels are kept per pixel slot, each in a buffer of its
// own laid out by the parts' pxbase, each level resting on the one before:
//     hit     (wfM0)  the traversal result of the camera ray.               Depends on the RAY KEY: camera, frame geometry, the cut into parts, tri_tmin, the mesh.
//     shadow  (wfX0)  the traversal result of segment 0's shadow ray.       Depends on the SHADING KEY: the ray key, the whole Scene, eps, textures, the elision rules.
//     records (wfS0)  the path after its shaded first hit (rtk::WfShade).   Depends on the shading key too: it has no key of its own.
// A chain of part j FILLS a level (traces as ever and stores), USES it (the launch that would have produced the words is not enqueued, or reads them) or leaves it OFF.
// The records are stored only by a chain that USES the shadow level -- the key has then held for two chains: a light that moves every frame never pays for a fill.
//
// The rules, each enforced in one place below:
//   - A part's words are written and read on ONE stream, inside chains only, and that stream is part of the ray key.  mark() is called at ENQUEUE: the next chain of the part
//     runs behind this one on the same stream, also under the relaxed start of pipelined frames (frame k + 1's chain of a part follows frame k's on the part's own stream).
//     A call whose chains run on other streams is a miss.                                                                             (StillLevel::chain, the caller's key)
//   - Replacing the ray key replaces the shading key; replacing the shading key empties the records; a new allocation of a level's buffer empties that level.  (begin)
//   - Keys are compared as bits: the caller zeroes its key's padding and puts the whole Scene in.  A wrong miss costs a refill, a wrong hit a silently wrong frame.  (StillKey::same)
//   - What lives behind a pointer of the keys and is edited in place reaches them through two generation counters.                    (mesh_changed, shading_changed)
//   - The eligibility levels nest: 0 none, 1 hit, 2 hit + shadow, 3 all three.  Chains of level 0 count as ineligible and touch nothing else; the list chains of
//     rt_render_counts* do not come here at all, nor do the chains of a frame whose camera has a lens, whose shutter is on or whose scene has an environment (lens_changed).   (begin, chain)
// Plain C++: the library and the host library (rth_still_replay, tests/test_still_view_model.py) compile the same text.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace rtk {

enum StillMode { kStillOff = 0, kStillFill = 1, kStillUse = 2 };
constexpr int kStillParts = 8;                       // rt_ctx::kMaxParts
constexpr int kStillMaxSteps = 17;                   // RT_MAX_SEGMENTS + 1

// One level: which parts hold words stored under the key in force, and its four counters -- chains that used the level / filled it / were ineligible; times the level was
// emptied while it held something (rt_first_{hit,shadow,shade}_cache_counts)
struct StillLevel {
    bool filled[kStillParts] = {};
    uint64_t counts[4] = {};
    void clear() {
        bool any = false;
        for (bool &f : filled) { any = any || f; f = false; }
        if (any) ++counts[3];
    }
    void mark(int j) { filled[j] = true; }
    // one chain of part j.  eligible: the chunk's level reaches this one; ready: what the level rests on is there (a chain that is eligible but not ready leaves the level
    // off and counts nowhere)
    StillMode chain(int j, bool eligible, bool ready = true) {
        if (!eligible) { ++counts[2]; return kStillOff; }
        if (!ready) return kStillOff;
        if (filled[j]) { ++counts[0]; return kStillUse; }
        ++counts[1]; mark(j);
        return kStillFill;
    }
};

// What a level's words were stored under: the caller's bytes, the generations and the allocation
struct StillKey {
    std::vector<unsigned char> bytes;                // empty: no key yet
    uint64_t gen[2] = {};
    const void *buf = nullptr;
    bool same(const void *p, size_t n, uint64_t g0, uint64_t g1, const void *b) const {
        return bytes.size() == n && n != 0 && memcmp(bytes.data(), p, n) == 0 && gen[0] == g0 && gen[1] == g1 && buf == b;
    }
    void set(const void *p, size_t n, uint64_t g0, uint64_t g1, const void *b) {
        bytes.assign(static_cast<const unsigned char *>(p), static_cast<const unsigned char *>(p) + n);   // (no allocation once it has held a key of this size)
        gen[0] = g0; gen[1] = g1; buf = b;
    }
};

struct StillChain { StillMode hit, shadow, records; };

struct StillView {
    StillLevel hit, shadow, records;
    // Every entry that can change a triangle, the visit order or the tree calls this: the hit words are stale (and with them everything above)
    void mesh_changed() { ++mesh_gen; ++tri_gen; }
    // Every entry that writes what shading reads behind a pointer of the Scene -- normals, UVs, texels, texture records: the shadow words and the records are stale
    void shading_changed() { ++shade_gen; }
    // rt_camera_set_lens turning the lens on or off.  Chains of a frame with the lens on do not come here at all (neither begin nor chain: no counter moves), so nothing
    // else would tell the first pinhole frame after them that frames went by in between: every level is stale
    void lens_changed() { ++mesh_gen; }
    // rt_scene_set_shutter turning the shutter on or off: the same, for the same reason (a shutter frame's chains do not come here either)
    void shutter_changed() { ++mesh_gen; }
    // rt_scene_set_environment setting, replacing or removing the map: the same again (a chain under an environment does not come here; a replaced map between two such
    // frames costs the next frame without one nothing more than the refill it owes anyway)
    void sky_changed() { ++mesh_gen; }
    // what mesh_changed alone has counted -- the triangles, not the lens, the shutter or the sky: the emitters' sampling table is rebuilt when it moved
    // (rt_host_render.hip.h emit_refresh)
    uint64_t triangle_generation() const { return tri_gen; }

    // Before a chunk's chains are enqueued, after their streams are settled.  level: what the chunk is eligible for; the keys are read up to that level only; M0 / X0 / S0: where
    // the three buffers are now.  Any difference from what a level was stored under empties it and every level above.
    void begin(int level, const void *ray, size_t ray_n, const void *shade, size_t shade_n, const void *M0, const void *X0, const void *S0) {
        if (rec_buf != S0) { records.clear(); rec_buf = S0; }
        if (level >= 1 && !ray_key.same(ray, ray_n, mesh_gen, 0, M0)) {
            hit.clear();
            ray_key.set(ray, ray_n, mesh_gen, 0, M0);
            ++ray_gen;
        }
        if (level >= 2 && !shade_key.same(shade, shade_n, ray_gen, shade_gen, X0)) {
            shadow.clear();
            shade_key.set(shade, shade_n, ray_gen, shade_gen, X0);
            records.clear();
        }
        lvl = level;
    }
    // Whether a chain of the coming chunk may store records, asked BEFORE begin (the buffers are sized before the streams are settled): the shadow level holds a part's
    // words, so a chain may use it, and its key's Scene -- the head of the shading key -- is this chunk's.  A light that moves every frame allocates nothing.
    bool may_store_records(const void *scene, size_t n) const {
        bool any = false;
        for (bool f : shadow.filled) any = any || f;
        return any && shade_key.bytes.size() >= n && memcmp(shade_key.bytes.data(), scene, n) == 0;
    }
    // One chain of part j under the level of the last begin; records_ok: the records' buffer exists at this chunk's size.  A chain that resumes from the records also
    // counts as having used the two levels below: it enqueued neither their launches.
    StillChain chain(int j, bool records_ok) {
        StillChain c;
        c.hit = hit.chain(j, lvl >= 1);
        c.shadow = shadow.chain(j, lvl >= 2);
        c.records = records.chain(j, lvl >= 3, c.shadow == kStillUse && records_ok);
        return c;
    }

  private:
    StillKey ray_key, shade_key;
    const void *rec_buf = nullptr;
    uint64_t mesh_gen = 0, shade_gen = 0, ray_gen = 0, tri_gen = 0;
    int lvl = 0;
};

// The launches of one chain.  It opens with one wf_advance -- begin, or resume from the records -- and goes on through positions first .. n - 1: at position `it` a
// traversal launch (if any) and the wf_advance that closes what it traced.
enum StillWin { kWinNone = 0, kWinY = 1, kWinX = 2 };            // the rows of the queue a traversal launch enumerates (rt_qrows.h)
enum StillAdv { kAdvBegin = 0, kAdvResume = 1, kAdvPlain = 2, kAdvFill = 3, kAdvClose = 4 };
struct StillStep {
    bool trav;                // the traversal launch is enqueued
    int win;                  // ... over this window
    bool trav_m0;             // ... and writes the part's block of the hit level instead of M
    int m0, x0;               // WfState::m0 / x0 of the wf_advance: it reads the hit level; 1 stores / 2 reads the shadow level
    int adv;                  // kAdvPlain, or kAdvFill: it stores the part's records; kAdvClose: the kernel of a plain chain's last position (RT_CHAIN_ENDS; rt_wavefront.hip.h wf_advance<kFormClose>)
};
struct StillPlan {
    int open;                 // kAdvBegin or kAdvResume
    int open_m0;              // WfState::m0 of the opening launch (only the first sample's camera rays go to the traversal)
    int kill_x;               // WfShade::kill_x: a resumed chain without a Y window clears its items' shadow slots instead
    int first, n;
    StillStep step[kStillMaxSteps];
};
// segs: ray segments of a path (0: the chain has no position at all); rows: traversal launches take windows (the work-stack kernel under RT_TRAVQ_ROWS);
// has_y: this part's queue has a Y window that is not every row; ends: the chain is a plain one (enqueue_chain) and takes the closing kernel
inline StillPlan still_plan(const StillChain &c, int segs, bool have_mesh, bool rows, bool has_y, bool ends = false) {
    StillPlan p;
    const bool resume = c.records == kStillUse;
    p.open = resume ? kAdvResume : kAdvBegin;
    p.open_m0 = (!resume && c.hit != kStillOff) ? 1 : 0;
    p.kill_x = (resume && !(rows && has_y)) ? 1 : 0;
    p.first = resume ? 1 : 0;                                     // a resumed chain starts where segment 0 is closed
    p.n = segs > 0 ? segs + 1 : 0;
    for (int it = 0; it < p.n; ++it) {
        StillStep &s = p.step[it];
        // the first launch of a chain that uses the hit level has nothing to trace; the second launch of a chain of one segment that uses the shadow level would trace
        // segment 0's shadow rays and nothing else
        s.trav = have_mesh && !(it == 0 && c.hit == kStillUse) && !(it == 1 && segs == 1 && c.shadow == kStillUse);
        // the first launch can meet no shadow ray and the last no continuation ray; neither can the first launch of a resumed chain, at position 1
        const bool only_y = it == 0 || (it == 1 && resume);
        s.win = !(rows && s.trav) ? kWinNone : only_y ? (has_y ? kWinY : kWinNone) : it == segs ? kWinX : kWinNone;
        s.trav_m0 = s.trav && it == 0 && c.hit != kStillOff;
        s.m0 = (it == 0 && c.hit != kStillOff) ? 1 : 0;            // the launch that closes segment 0 reads the camera rays' results from the hit level
        s.x0 = (it <= 1 && !resume) ? (int)c.shadow : 0;           // the launch that emits segment 0's shadow rays and the one that closes them
        s.adv = (it == 0 && c.records == kStillFill) ? kAdvFill : kAdvPlain;
    }
    // The last launch meets no continuation ray: it closes segment segs - 1's shadow rays and folds (never the launch that stores the records: that one is at position 0)
    if (ends && segs > 0) p.step[segs].adv = kAdvClose;
    return p;
}

// ---- the FORM of a wf_advance launch: which instantiation of rt_wavefront.hip.h's one kernel template it runs ----
// One word of flag bits, the kernel's first template argument.  What each bit compiles in is told at wf_advance_path; which words are built at all is the switch of
// launch_advance (rt_host_render.hip.h) and the table of DESIGN.md section 5.2.
// stats: counts work (rt_count_work), Work is filled and flushed; first: the opening launch, camera rays instead of closing queries; close: the last launch of a plain chain;
// and the bits that bring the kernel an extra argument -- tex: textured meshes (TexScene); anim: a frame of an animated batch (const AnimFrame *__restrict__); list: the items
// are (pixel slot, sample) records (WfList); fill / resume: stores the first-shade records / opens a chain from them (WfShade); lights: several point lights (WfLights); soft:
// lights with a radius (WfSoftLights; in place of lights, never both); lens: the thin lens, with first (WfLens); shutter: the spheres and the light at the sample's own
// time (WfShutter), in every launch of the chain; sky: a ray that misses meets the environment map (WfSky), in every launch after the opening one -- its extra comes last
constexpr unsigned kFormStats = 1u << 0, kFormFirst = 1u << 1, kFormTex = 1u << 2, kFormAnim = 1u << 3, kFormList = 1u << 4, kFormFill = 1u << 5, kFormResume = 1u << 6,
                   kFormLights = 1u << 7, kFormSoft = 1u << 8, kFormLens = 1u << 9, kFormClose = 1u << 10, kFormShutter = 1u << 11, kFormSky = 1u << 12,
                   kFormSkySample = 1u << 13,                // sky sampling: a segment's shadow ray may go to the environment, drawn from its table (WfSkyDist, after the WfSky)
                   kFormEmit = 1u << 14,                     // emissive meshes: a ray that hits an emitter ends there, a segment's shadow ray may go to one (WfEmit, after the WfSoftLights)
                   kFormFresnel = 1u << 15,                  // Fresnel dielectrics: a ray that hits a flagged glass object is reflected or refracted, one draw (WfFresnel, last)
                   kFormGloss = 1u << 16,                    // rough mirrors: a ray that hits a mirror with a roughness is reflected about a GGX facet, two draws (WfGloss, last)
                   kFormTint = 1u << 17;                     // tinted mirrors and glass: a specular segment of a flagged object is folded with the object's albedo (WfTint, last; always with kFormGloss)
constexpr unsigned kFormNotBuilt = ~0u;              // adv_form: no entry asks for this launch, and no kernel exists for it

// What decides the form besides the step: the chain's facts.  counting: rt_count_work; anim: a batch with per-frame scenes; list: rt_render_counts*; lights: 0 the Scene's
// one point light, 1 several, 2 some with a radius; shutter: the shutter is on (rt_scene_set_shutter) -- defaulted: a chain without one is written as before; sky: the scene has an
// environment (rt_scene_set_environment) -- last and defaulted, for the same reason
// emit: a mesh of the scene emits (rt_scene_set_emission) -- last and defaulted as well
// fresnel: an object of the scene is effectively flagged (rt_material_set_fresnel) -- last and defaulted as well
// gloss: an object of the scene has an effective roughness (rt_material_set_roughness) -- last and defaulted as well
// tint: an object of the scene is effectively tinted (rt_material_set_tint) -- last and defaulted as well
struct AdvFacts { bool counting, tex, anim, list, lens; int lights; bool shutter = false; bool sky = false; bool sample = false; bool emit = false; bool fresnel = false; bool gloss = false; bool tint = false; };   // sample: sky sampling is in effect (with sky), last and defaulted too
// The plain chain -- every launch after the opening one the form 0 or kFormStats (or the launch that stores the records): still_plan's `ends`, for a work-stack chain
inline bool adv_plain_chain(const AdvFacts &f) { return !f.tex && !f.anim && !f.list && !f.lens && f.lights == 0 && !f.shutter && !f.sky && !f.emit && !f.fresnel && !f.gloss && !f.tint; }
// The form of the launch a chain of these facts enqueues for `adv` (StillAdv: StillPlan::open for the opening launch, StillStep::adv for the later ones)
inline unsigned adv_form(const AdvFacts &f, int adv) {
    // counting, a list and an animated batch exclude one another, and each refuses several lights, a radius and the lens before a chain is planned (lights_refuse)
    const int special = (f.counting ? 1 : 0) + (f.anim ? 1 : 0) + (f.list ? 1 : 0);
    if (f.lights < 0 || f.lights > 2 || special > 1 || (special == 1 && (f.lights != 0 || f.lens))) return kFormNotBuilt;
    // The shutter: every launch of the chain forms the sample's pose, so every launch has the bit.  Built for a frame of one point light alone: counting, a list, an
    // animated batch, several lights and a radius refuse it (lights_refuse); no still view (no records), and the closing kernel reads the Scene's L: not a plain chain
    // The environment: a ray meets it where it is closed, so the opening launch is what it was and every later launch has the bit.  Counting, a list, an animated batch and
    // the shutter refuse it (lights_refuse); no still view (no fill, no resume), and the closing kernel closes no continuation ray: not a plain chain.  A light list without
    // a radius goes through the soft forms with radii 0 (a radius-0 light is the light itself, bit for bit): four later forms, not six
    if (f.sample && !f.sky) return kFormNotBuilt;
    // Tinted mirrors and glass: the specular segment is recorded where a continuation ray is closed, so the opening launch is what it was (the lens included) and every
    // later launch has the bit -- together with kFormGloss, whether a mirror of the scene is rough or not (an empty WfGloss mask: the smooth mirror arm): four forms, not
    // eight.  Counting, a list, an animated batch, the shutter, an environment, an emitter and an effective Fresnel flag refuse it (lights_refuse); no still view (the
    // records hold no segment but the first, and the closing kernel's fold would have to be a tint form too) and not a plain chain
    if (f.tint) {
        if (special != 0 || f.shutter || f.sky || f.emit || f.fresnel) return kFormNotBuilt;
        if (adv == kAdvBegin) return kFormFirst | (f.lens ? kFormLens : 0u);
        if (adv == kAdvPlain) return (f.tex ? kFormTex : 0u) | (f.lights != 0 ? kFormSoft : 0u) | kFormGloss | kFormTint;
        return kFormNotBuilt;
    }
    // Rough mirrors: the facet is drawn where a continuation ray is closed, so the opening launch is what it was (the lens included) and every later launch has the
    // bit.  Counting, a list, an animated batch, the shutter, an environment, an emitter and an effective Fresnel flag refuse it (lights_refuse); no still view (no
    // fill, no resume: the records hold one continuation ray per pixel slot, a rough first hit has one per sample) and not a plain chain.  A light list or a radius
    // takes the soft route: four forms
    if (f.gloss) {
        if (special != 0 || f.shutter || f.sky || f.emit || f.fresnel) return kFormNotBuilt;
        if (adv == kAdvBegin) return kFormFirst | (f.lens ? kFormLens : 0u);
        if (adv == kAdvPlain) return (f.tex ? kFormTex : 0u) | (f.lights != 0 ? kFormSoft : 0u) | kFormGloss;
        return kFormNotBuilt;
    }
    // Fresnel dielectrics: the choice is made where a continuation ray is closed, so the opening launch is what it was (the lens included) and every later launch has
    // the bit.  Counting, a list, an animated batch, the shutter, an environment and an emitter refuse it (lights_refuse); no still view (no fill, no resume: the records
    // hold one continuation ray per pixel slot, a flagged hit has one per sample) and not a plain chain.  A light list or a radius takes the soft route: four forms
    if (f.fresnel) {
        if (special != 0 || f.shutter || f.sky || f.emit) return kFormNotBuilt;
        if (adv == kAdvBegin) return kFormFirst | (f.lens ? kFormLens : 0u);
        if (adv == kAdvPlain) return (f.tex ? kFormTex : 0u) | (f.lights != 0 ? kFormSoft : 0u) | kFormFresnel;
        return kFormNotBuilt;
    }
    // Emissive meshes: an emitter is met where a continuation ray is closed and sampled where a segment is shaded, so the opening launch is what it was and every later
    // launch has the bit.  An environment, the shutter, counting, a list and an animated batch refuse it (lights_refuse); no still view, not a plain chain; any light
    // configuration takes the soft route, as under sky sampling: two forms
    if (f.emit) {
        if (special != 0 || f.shutter || f.sky) return kFormNotBuilt;
        if (adv == kAdvBegin) return kFormFirst | (f.lens ? kFormLens : 0u);
        if (adv == kAdvPlain) return (f.tex ? kFormTex : 0u) | kFormSoft | kFormEmit;
        return kFormNotBuilt;
    }
    if (f.sky) {
        if (special != 0 || f.shutter) return kFormNotBuilt;
        if (adv == kAdvBegin) return kFormFirst | (f.lens ? kFormLens : 0u);
        // sky sampling: any light configuration takes the soft route (one point light is a soft list of one at radius 0): two forms
        if (adv == kAdvPlain && f.sample) return (f.tex ? kFormTex : 0u) | kFormSoft | kFormSky | kFormSkySample;
        if (adv == kAdvPlain) return (f.tex ? kFormTex : 0u) | (f.lights != 0 ? kFormSoft : 0u) | kFormSky;
        return kFormNotBuilt;
    }
    if (f.shutter) {
        if (special != 0 || f.lights != 0) return kFormNotBuilt;
        if (adv == kAdvBegin) return kFormFirst | (f.lens ? kFormLens : 0u) | kFormShutter;
        if (adv == kAdvPlain) return (f.tex ? kFormTex : 0u) | kFormShutter;
        return kFormNotBuilt;
    }
    const unsigned stats = f.counting ? kFormStats : 0u;
    switch (adv) {
    case kAdvBegin: return kFormFirst | (f.anim ? kFormAnim : f.list ? kFormList : f.lens ? kFormLens : stats);   // a camera ray knows no texture and no light
    case kAdvResume:
    case kAdvFill:                                    // the records level: a still view (never counting, a batch, a list or a lens) of one point light and no texture
        if (special != 0 || f.lens || f.lights != 0 || f.tex) return kFormNotBuilt;
        return adv == kAdvFill ? kFormFill : kFormResume;
    case kAdvClose: return adv_plain_chain(f) ? kFormClose | stats : kFormNotBuilt;
    case kAdvPlain:                                   // (a lens chain's later launches are the scene's own)
        return (f.tex ? kFormTex : 0u) | (f.anim ? kFormAnim : f.list ? kFormList : f.lights == 2 ? kFormSoft : f.lights == 1 ? kFormLights : stats);
    }
    return kFormNotBuilt;
}

}  // namespace rtk
