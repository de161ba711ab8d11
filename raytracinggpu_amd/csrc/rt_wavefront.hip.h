// rt_wavefront.hip.h -- wavefront render pipeline for gfx950 (default variant).
//
// The per-pixel render of cpu_launcher.cpp:693-718 / KernelLaunch (optimized.cu:670-772) split by
// divergence behaviour instead of by pixel:
//
//   wf_advance<kFormFirst>  one lane per pixel, uniform: camera ray of sample s, its ray/sphere tests
//              (cpu:512-527) and the mesh's root-box test (cpu:279); path record initialised
//   wf_travq   (rt_travq.hip.h; the pipeline's traversal kernel by default) the BVH traversal as a per-wave work stack of
//              (ray slot, sibling pair) entries: BoundingBox::intersect cpu:146-157, moller_trumbore cpu:226-236, traversal
//              cpu:277-311
//   wf_trav    (variants wavefront / wavefront_lds) persistent lanes, one RAY (or a sub-range of one ray's traversal) per lane:
//              stackless BVH walk.  Two micro-ops (BOX, TRI) chosen by wave vote; lanes refill from the wave's own, spatially
//              scrambled, share of the rays; when that runs out busy lanes hand parts of their traversal
//              to idle lanes (see "work splitting" below).
//   wf_advance one lane per pixel, uniform: closes the query (Scene::intersect_all cpu:545-564), then
//              Scene::getColor's branch for it -- material / shadow ray or direct light + cosine bounce
//              (the arithmetic of each: rt_shade.hip.h) -- writes the next ray with its sphere and root-box
//              tests, or folds the finished path, accumulates the sample (cpu:711) and, after the last
//              sample, stores the pixel as one float4 (cpu:713)
//
// A shadow ray and the continuation (bounce / mirror / refraction) ray that leave the same hit point do not
// depend on each other, so both are traced by the SAME traversal launch: per sample the sequence is
//     advance<FIRST>, (trav, advance) x (segments + 1)
// with launch j tracing the shadow rays of segment j-1 and the continuation rays of segment j.  The path records (16 bytes)
// live in HBM as float4 indexed by a TILE-ORDER path index (8x8 pixel tiles: a wave's 64 consecutive paths are one
// tile, every record access is a fully coalesced 1 KiB wave transaction); the rays themselves live only in the traversal queue
// (slot order), see WfState.
//
// Work splitting.  The reference never prunes by distance, so which nodes and triangles a ray
// visits does not depend on what it has hit so far, and the nearest hit is  min over visited triangles of
// (t, visit rank)  -- the strict '<' of cpu:301 keeps the earliest of equal t.  In the stackless layout the
// traversal of node range [a,b) that starts at a is self-contained whenever a is a node the walk is certain
// to reach: the node after any subtree (skip(X)) is such a node.  So a lane at node X owning [X,b) can keep
// [X,skip(X)) and give [skip(X),b) to an idle lane; a lane inside a leaf can give away everything after the
// leaf, or half of the leaf's triangles.  Triangles are stored in visit order, so rank == triangle index,
// and sub-results meet in one 64-bit atomic min on (bits(t) << 32 | index).  Results stay bit-identical.
#pragma once
#include "rt_kernels.hip.h"
#include "rt_qrows.h"
#include "rt_still.h"
#include <type_traits>

namespace rtk {

// path record flags (F.x; rt_path.hip.h keeps the same record in LDS)
constexpr int PF_ALIVE = 1, PF_HASX = 2, PF_HASY = 4;       // path being traced; a shadow ray (X) of segment d-1's hit / a continuation ray (Y) of segment d is in flight
constexpr int PF_MESHX = 8, PF_MESHY = 16;                  // that ray passed the mesh's root box: its traversal result M[] is meaningful
constexpr int PF_DEPTH_SHIFT = 5, PF_DEPTH_MASK = 31;       // segment index d of the continuation ray in flight (or of the next one), 0..16
constexpr int PF_RAYS_SHIFT = 10, PF_RAYS_MASK = 63;        // rays traced so far for this sample (<= 2 * 16 + 1)
constexpr int PF_WINS_SHIFT = 16;                           // 10 bits: the Y ray's nearest sphere before / after the mesh slot (object id + 1)
constexpr int PF_XSPHERE = 1 << 26;                         // the X ray is blocked by a sphere already (cpu:615 true whatever the mesh says)
constexpr unsigned long long WF_NOHIT = ~0ull;
// the wavefront pipeline keeps the path's flag word in its continuation (Y) slot's queue record; bits 0..15 as above, then:
constexpr int PQ_WIN_SHIFT = 16;                            // 5 bits: object id + 1 of the Y ray's nearest sphere (0 = none); its t is the record's last word
constexpr int PQ_ANYHIT = 1 << 21;                          // (X slot only) the record's last word is the shadow ray's ANY-HIT bound: see wf_anyhit_bound
constexpr int PQ_XSPHERE = 1 << 22;                         // PF_XSPHERE of this record
constexpr int PQ_REFR_SHIFT = 23;                           // 6 bits: Ray::refraction_index of the Y ray: 0 = 1.0, else (object id + 1) << 1 | (0: that object's n_in, 1: its n_out)
constexpr int PQ_TRAV = 1 << 29;                            // (either slot) the record's ray passed the mesh's root box: the traversal launch whose number (WfState::epoch) equals the
                                                            // record's depth field picks it up.  A shadow ray that misses the root box is not written at all: what its slot still
                                                            // holds is an older launch's record (other depth or another chain's number), or the zero of the layout's memset
constexpr int PQ_NONCE_SHIFT = 30, PQ_NONCE_MASK = 3;        // (either slot) the launch chain's number mod 4, so that wf_advance<kFormFirst> need not clear the shadow slots of the previous chain
constexpr int PQ_LIVE_MASK = (int)((unsigned)PQ_TRAV | ((unsigned)PF_DEPTH_MASK << PF_DEPTH_SHIFT) | ((unsigned)PQ_NONCE_MASK << PQ_NONCE_SHIFT));
// the record is live for traversal launch `epoch` of the chain numbered `nonce`: one masked compare.  A stale shadow record that passes (written four chains ago at the
// same depth into a slot nobody wrote since) costs one wasted traversal and nothing else: wf_advance reads a shadow ray's result only if ITS OWN flag word says the
// ray went to the mesh (PF_MESHX).  A RESUMED chain (first-shade cache, wf_advance<kFormResume>) writes no depth-1 shadow record at all, so a stale one of that depth would pass
// every fourth chain for as long as the view stands still: the chain's traversal launch 1 carries continuation rays only and enumerates the Y window (rt_qrows.h), in which
// only the one mixed row can hold such a record; where there is no window the resume kernel writes the dead second half into its item's X slot (WfShade::kill_x)
__device__ __forceinline__ bool wq_live(int w0, int epoch, int nonce) {
    return (w0 & PQ_LIVE_MASK) == (int)((unsigned)PQ_TRAV | (unsigned)epoch << PF_DEPTH_SHIFT | (unsigned)nonce << PQ_NONCE_SHIFT);
}

// ANY-HIT bound of a shadow ray.  cpu:615 asks whether |P' - Pa|^2 <= |L - Pa|^2 for P' = Pa + t_min u, the NEAREST hit of the shadow ray (Pa = P_adjusted, u = (L - Pa) /
// |L - Pa|), and uses nothing else of that hit.  Every rounding on the left is monotone in t (fl(t u_k), fl(Pa_k + .), fl(. - Pa_k), the squares, the sums: the magnitude of
// each component grows with t, see the comment at the close of the X query in wf_advance_path), so the comparison holds for the nearest hit iff it holds for SOME accepted
// hit: a traversal that has accepted one triangle whose t certainly passes may stop -- the frame cannot tell.  "Certainly": with nl = fl(sqrt(fl|L - Pa|^2)) (the value
// normalize() divides by), g_k = fl(fl(Pa_k + fl(t u_k)) - Pa_k) obeys |g_k| <= t |u_k| (1 + 3 * 2^-24) + 2^-24 (1 + 2^-23) |Pa_k|, |u| <= 1 + 2^-22, so the left side's
// square root is at most t (1 + 2^-20) + 2^-22 |Pa|_1, while the right side's is at least nl (1 - 2^-24).  Any t <= nl (1 - 2^-15) - 2^-20 |Pa|_1 is therefore inside with
// a margin of more than 2^-16 nl (the bound's own two roundings are 2^-24 each); hits between this bound and the light (a band 3e-5 of the distance wide) simply do not stop
// the traversal, whose complete result then decides as before.  -inf = never (a light within 1e-12 of the surface or so far that the squared distance overflows; with a NaN
// anywhere the bound is a NaN or -inf: every comparison with it is false).
__device__ __forceinline__ float wf_anyhit_bound(f3 Pa, float nl) {
    const float b = fmaf(nl, 1.f - 0x1p-15f, -0x1p-20f * ((fabsf(Pa.x) + fabsf(Pa.y)) + fabsf(Pa.z)));
    return (nl > 1e-12f && nl < 1e30f) ? b : -__builtin_inff();      // (above 1e-12 no square that matters to the budget is denormal; a finite nl is below 1.9e19 anyway: beyond it |L - Pa|^2 is +inf)
}

// DEAD CHANNELS of a path.  The fold is, per channel, ans_k = fl(fl(fl(l_k alb_k) / pi) + fl(alb_k ans_{k+1})) (fold_segment), back to front.  A channel c is DEAD from the
// first diffuse segment m whose albedo in c is +0 (the bits: a -0, a denormal or a NaN is not): whatever later segments hand up, segment m passes on
// fl(fl(l_m (+0)) / pi) + fl((+0) x) = +0 + (+-0) = +0 -- if l_m has a clear sign bit and is finite, and x = ans_{m+1}[c] is finite.  A diffuse segment j whose three channels
// are dead (its own albedo counted) has a shadow ray that decides only between l_j = lvis and l_j = +0, and neither value can reach the pixel: with any-hit on the ray is
// not traced (x_moot below, the rule of the direct term that is +0 either way with a second reason) and LS keeps lvis.  The pixel is the same (NaN for NaN) if, in the chain
// the reference folds (W: every elided l_j is lvis_j or +0) and in the chain the kernel folds (A: every elided l_j = lvis_j), each dead channel arrives at its kill m with an
// x that is finite in both chains or in neither (0 x is then NaN in both).  The argument rests on what is known when the ray is emitted and on nothing else:
//   (1) the GUARD: a segment counts (kills channels, keeps the mask) only if its three albedo components lie in [+0, 1] and its lvis in [+0, 2^96) -- as unsigned integers,
//       bits <= 0x3f800000 and < 0x6f800000, which rules out negative numbers, -0, inf and every NaN at once.  A segment that fails clears the mask (wf_dead_channels): kills
//       before it are forgotten, so a run of segments from the earliest kill in use to the last elided segment after it holds guarded segments only.
//   (2) inside such a run the two chains differ by the elided direct terms alone, and what enters the run from below (Z, the ans of the segment after it) is the same in
//       both: deeper runs hand up what they were handed (each channel passes a kill of its own run), and below the deepest run Z is what the fold starts from -- +0, or
//       under an environment the E the path's last ray met (sky_radiance), computed at the miss from the ray alone, before and apart from any elision: the same in both
//       chains too, and finite with a clear sign bit (every texel lies in [+0, 2^96), rt_scene_set_environment, and the four bilinear weights lie in [0, 1]: the sum stays below 2^98).  Z non-finite: both chains carry an inf of one sign or a NaN through the
//       run (alb Z is the same product in both, a finite direct term changes neither), so x is non-finite in both.  Z finite: a product with an albedo <= 1 cannot
//       overflow, and a sum cannot either -- a direct term below 2^96 / pi is less than half an ulp of anything from 2^127 on and leaves it as it is, and below 2^127 the
//       sum stays below 2^127 + 2^96 -- so x is finite in both and the dead channels are +0 in both.  Above the run the two chains fold the same numbers.
// An albedo above 1 or a direct term of 2^96 and more was admitted by the first version of the guard, which then needed "no ans of chain A reaches 2^126" on top, a condition
// nobody can know at emission: a light of 3e38 over walls of albedo 4 took chain A to inf where the reference's stayed finite (NaN against +0 in 346 words of a 64 x 48
// frame, tests/test_gpu_scene_fuzz.py light_edge seed 19).  The counting instantiation still reports paths with an elided ray whose fold leaves that old range
// (wf_fold_bounded, rt_dead_channel_counts: unsure) -- a statistic now, their pixels are the reference's.  tests/test_dead_channels.py restates guard and fold in numpy
// binary32 and compares every chain with an elided ray.
// State: one byte per path, WfState::DCH[i] (bits 0..2: the dead channels, bit 3: a ray was elided), zeroed by wf_advance<kFormFirst>, read by every diffuse segment and written
// when it changes (at most 4 times per path): 1 B written per path and chain, <= 1 B read per path and launch.  (Bit 21 of the Y slot's flag word is NOT free for it: wf_travq
// tests PQ_ANYHIT on every record it fetches, continuation rays included, and would take the nearest sphere's t for an any-hit bound.)
constexpr unsigned kDeadAlbedoMax = 0x3f800000u;            // bits of 1: the largest albedo component of a segment that counts
constexpr unsigned kDeadDirectEnd = 0x6f800000u;            // bits of 2^96: a segment that counts has its direct term below it
constexpr unsigned kFoldFinite = 0x7f800000u;               // bits of +inf: a float whose bits are below it, as an unsigned integer, is finite with a clear sign bit
constexpr unsigned kFoldBound = 0x7e800000u;                // bits of 2^126
__device__ __forceinline__ unsigned wf_umax3(f3 v) { return max(max(__float_as_uint(v.x), __float_as_uint(v.y)), __float_as_uint(v.z)); }
// the dead channels after a diffuse segment with albedo alb and direct term lvis, given those before it
__device__ __forceinline__ int wf_dead_channels(int dead, f3 alb, float lvis) {
    const bool good = wf_umax3(alb) <= kDeadAlbedoMax && __float_as_uint(lvis) < kDeadDirectEnd;
    const int kill = (__float_as_uint(alb.x) == 0u ? 1 : 0) | (__float_as_uint(alb.y) == 0u ? 2 : 0) | (__float_as_uint(alb.z) == 0u ? 4 : 0);
    return good ? (dead | kill) : 0;
}
// (statistic) one folded segment inside the range the first version of the rule was argued for: its operands and its result
__device__ __forceinline__ bool wf_fold_bounded(f3 ans, float l, f3 alb) {
    return __float_as_uint(l) < kFoldFinite && wf_umax3(alb) < kFoldFinite && wf_umax3(ans) < kFoldBound;
}

// A BATCH of frames in one launch chain (rt_render_device_batch): the items of a chain are (frame f, pixel slot) pairs -- the machinery that traces several samples of a pixel
// as parallel items (n_paths = n_px x items per pixel), with a camera, a seed and an output buffer PER FRAME instead of per-sample colours to reduce.  A rank that renders a
// small share of a frame (1/8 of 1920x1080 = 0.26 Mpixel) fills the chip with K frames' worth of paths per launch instead of K chains on K streams.  Only wf_advance reads it.
// The descriptors live in device memory (WfState::batch: one copy per sub-frame, written by batch_store_kernel at the head of that sub-frame's own chain) and are read with
// a wave-uniform index: as kernel arguments a dynamically indexed array is copied to scratch by the compiler (2 KB per lane, measured).
constexpr int kMaxBatch = 16;
struct BatchFrame { float camx, camy, camz, z; uint32_t seed; int pad; float4 *out; };
struct Batch { int n; int pad; BatchFrame f[kMaxBatch]; };
__global__ void batch_store_kernel(const Batch bt, BatchFrame *__restrict__ dst) {
    const int k = threadIdx.x;
    if (k < kMaxBatch) dst[k] = bt.f[k < bt.n ? k : 0];               // (constant trip structure: one lane per descriptor)
}

// An ANIMATED batch (rt_render_device_batch_scenes): besides its camera every frame has its own light and its own sphere poses -- MoveLightSource / MoveObject
// (realtime_render.cu:1072-1098) between the frames of a sequence.  Everything else of the scene (materials, object positions, meshes) is the uploaded Scene of the kernel
// arguments.  The table lives next to the BatchFrame descriptors under the same protocol (one copy per sub-frame, written at the head of that sub-frame's own chain) and is read
// by wf_advance's animated instantiations alone, through the frame's wave-uniform address: the light and sph[] by scalar loads, ctr[] with the hit object's id.
struct AnimFrame {
    float Lx, Ly, Lz, intensity;             // Scene::L, Scene::intensity of this frame
    float4 sph[kMaxSpheres];                 // (centre, R2 = R * R as one binary32 product) of sphere k, in the order of Scene::sph
    float4 ctr[kMaxSpheres];                 // the same centres by OBJECT id (Scene::obj_a's xyz; a mesh's entry is 0)
};
// The caller's records of kAnimStore frames per launch: 16 frames of 16 + 16 * 16 bytes do not fit the 4 KB of a kernel's arguments
constexpr int kAnimStore = 8;
struct AnimPose { float cx, cy, cz, R; };
struct AnimSrc { float Lx, Ly, Lz, intensity; AnimPose s[kMaxSpheres]; };
struct AnimStore { int n, n_spheres, obj[kMaxSpheres]; AnimSrc f[kAnimStore]; };
static_assert(sizeof(AnimStore) + sizeof(void *) <= 4096, "anim_store_kernel's arguments must fit 4 KB");
// one lane per (frame, k): sphere k's record and the centre of OBJECT k, of frames [0, as.n) of this launch
__global__ __launch_bounds__(kAnimStore * kMaxSpheres) void anim_store_kernel(const AnimStore as, AnimFrame *__restrict__ dst) {
    const int f = threadIdx.x / kMaxSpheres, k = threadIdx.x % kMaxSpheres;
    if (f >= as.n) return;
    const AnimSrc &src = as.f[f];
    AnimFrame &d = dst[f];
    if (k == 0) { d.Lx = src.Lx; d.Ly = src.Ly; d.Lz = src.Lz; d.intensity = src.intensity; }
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f), c = rec;
    for (int j = 0; j < as.n_spheres; ++j) {
        const AnimPose s = src.s[j];
        if (j == k) rec = make_float4(s.cx, s.cy, s.cz, s.R * s.R);   // R * R: one binary32 product, as rt_scene_upload forms it (cpu:513)
        if (as.obj[j] == k) c = make_float4(s.cx, s.cy, s.cz, 0.f);
    }
    d.sph[k] = rec;
    d.ctr[k] = c;
}

// Path state of the wavefront pipeline, in HBM.  A ray lives in ONE place: its 32-byte record in the traversal queue (slot order;
// the four rays of a group are one 128-byte line), which the uniform kernel writes when it emits the ray, the traversal kernel
// reads, and the next uniform launch reads back to compute the hit point.  The record's two spare words hold the PATH's state as
// well (flag word and the nearest sphere's t: round 4; rounds 2-3 kept a 16-byte path record beside the queue), so a path that is
// alive costs one 32-byte read and one 32-byte write of its Y slot, the X slot's record when a shadow ray leaves, 8 bytes of
// traversal result per ray and 5 bytes per shaded segment (round 1: ~300 B per path and launch, rounds 2-3: 154).
struct WfState {
    unsigned long long *M;   // [2 n_paths] traversal result by ray (Y rays at [0, n_paths), X rays at [n_paths, 2 n_paths)): bits(t) << 32 | triangle index (visit order); WF_NOHIT if none
    float4 *samp_out;     // frames with more than one sample: [n_paths] (colour of the item's sample, rays traced); path_reduce adds them in sample order
    float *LS;            // l (cpu:623) of every diffuse segment, written when the segment is shaded and zeroed if its shadow ray is blocked: LS[d * n_paths + i]
    unsigned char *SID;   // object id of the surface shaded at segment d, 0xff if it was not diffuse: SID[d * n_paths + i]
    int n_paths;          // items of this launch chain: n_px * (samples traced together); item i = sample (samp0 + i / n_px) of pixel slot i % n_px
    int n_px;             // pixel slots of the sub-frame: tiles_x * tiles_y * 64
    unsigned int n_px_m, tiles_x_m, Q_m;   // floor(2^32 / d) for the three divisors the uniform kernel divides by (wf_div)
    int samp0;            // first sample of the chain
    int tiles_x;
    // traversal scheduling: ray-slot q in [0, slots) maps to ray 4*g + (q & 3), g = ((q>>2) & (S-1)) * Q + ((q>>2) >> log2S)
    int log2S, Q, n_groups;   // n_groups = 2 n_paths / 4 (ray groups);  S * Q >= n_groups
    int slots_per_block;      // multiple of 4: ray slots owned by one workgroup, handed to its waves on demand
    int nonce;                // number of the launch chain mod 4 (from a counter of the context): part of every live record's flag word
    int epoch;                // index of the traversal launch inside its chain (0 after wf_advance<kFormFirst>): a queue record is live iff its flag word carries PQ_TRAV and this number
    int init_m;               // the traversal kernel merges partial results with atomicMin (wf_trav's work splitting): emitters initialise M
    unsigned long long *dbg;  // optional per-wave debug record (-DRT_DEBUG)
    int anyhit;               // shadow rays carry their any-hit bound (PQ_ANYHIT): the fixed-point instantiations of wf_travq stop a shadow ray at the first accepted triangle that certainly
                              // shades; a shadow ray that a sphere shades already is not traced through the mesh; a shadow ray whose segment has the direct term +0 either way is not traced
    int m0;                   // first-hit cache (rt_host_ctx.hip.h FirstHit), set in two launches of an eligible chain and zero in every other: M is the part's block of the cache, one word per
                              // PIXEL SLOT.  wf_advance<kFormFirst>: only the items of the chain's first sample are handed to the traversal; the launch that closes segment 0: the Y result of item i
                              // is M[i - s_rel * n_px].  (The field sits in what was padding before `batch`: no kernel's argument layout moves.)
    const BatchFrame *batch;  // rt_render_device_batch: n_batch frame descriptors in device memory (item i belongs to frame i / n_px); nullptr / 0 = the launch's own camera, seed, output
    int n_batch;
    int policy;               // stream policy (kPol*, RT_STREAM_POLICY): which use-once streams of wf_advance go past the Infinity Cache; 0 = every access the plain instruction.  Wave-uniform;
                              // only wf_advance_path reads it.  (The field sits in what was padding before `QR`: no kernel's argument layout moves.)
    // traversal queue: the rays in TRAVERSAL-SLOT order, so that the slots a traversal workgroup owns are contiguous and one
    // round trip brings flag and record
    float4 *QR;               // [2 slots] record of slot q: QR[2q] = (O.xyz, u.x), QR[2q+1] = (u.y, u.z, bits(W0), W1).  Y slot (ray r < n_paths): W0 = the path's
                              // flag word (PF_* | PQ_*; 0 = no path), W1 = t of the Y ray's nearest sphere; X slot: W0 = PQ_TRAV | depth | chain number (| PQ_ANYHIT: W1 = the any-hit bound), written only when the ray needs traversal
    unsigned char *DCH;       // [n_paths] dead channels of path i (bits 0..2) and whether one of its shadow rays was elided for them (bit 3); wf_advance<kFormFirst> zeroes it (deadch only)
    int deadch;               // any-hit is on and so is the dead-channel rule: a diffuse segment whose three channels are dead does not trace its shadow ray (wf_dead_channels)
    QRows win;                // wf_travq: the rows of the queue this launch enumerates (rt_qrows.h; slots_per_block is then a share of the window); all zero = every row, the slot index as it is
    unsigned long long *X0;   // first-shadow cache (rt_host_ctx.hip.h FirstShadow): the part's block, one word per PIXEL SLOT -- what wf_travq wrote into M for the slot's segment-0 shadow ray
    int x0;                   // ... 0 off, 1 fill, 2 read; non-zero in two wf_advance launches of an eligible chain and in no other.  The one that emits segment 0's shadow rays (m0 is
                              // set there): a ray whose answer is cached (read), or is the first sample's ray of its pixel slot (fill, a later sample's item), gets its record without
                              // PQ_TRAV.  The next one, which closes them: the result word is X0[slot] (read), or M of the first sample's ray, which a first-sample item also stores (fill)
};

// THE STREAM POLICY (WfState::policy; DESIGN.md section 4 "which streams deserve the Infinity Cache", tools/stream_reuse.py).  The path state that one launch writes and the
// next reads -- QR, M, DCH -- lives on hits of the 256 MiB Infinity Cache; a stream whose next use is a whole frame away cannot hit and only evicts it.  A set bit marks
// the accesses of one such group non-temporal (__builtin_nontemporal_load / _store: the `nt` bit of the global instruction); a clear bit leaves the plain instruction.
// The bit is wave-uniform (a kernel argument): a scalar branch around either form of the same access, never a different address or value.  Two groups are kept; the two
// that were measured and taken out again (LS / SID of the segments folded out of reach, what a still view stores once): DESIGN.md section 11.
constexpr int kPolRecords = 1;                               // the first-shade records wf_advance<kFormResume> loads: once per frame (a chain of one sample per pixel slot)
constexpr int kPolPixels = 2;                                // the pixel store of the fold: no launch of the chain reads the frame
// DEAD LAST (rt_deadlast.h: the permission, decided by the host at every enqueue; DESIGN.md section 5.1 "Dead paths").  One more wave-uniform bit of the same word, not a
// stream group: the chain's LAST continuation ray (segment segs - 1) of a path whose three channels are dead after the segment that emits it, and whose sphere tests found
// a hit, is not given its root test.  It leaves without PF_MESHY | PQ_TRAV, exactly as a ray that failed the root test: the next launch closes it as the sphere's hit,
// stores that sphere's SID and lvis, elides and counts the segment's shadow ray as the dead-channel rule does (the mask stays 7: the permission keeps lvis below 2^96;
// a -0 from a surface edge-on to the light clears it and traces the shadow ray, finite all the same)
// and the path finishes in the launch it always finished in.  The frame cannot tell: each channel's kill sits at a segment <= segs - 2 and turns any FINITE ans of the last
// segment into +0 -- finite for whatever the ray would really have hit and for the sphere shaded in its place is what the permission promises -- and .w counts the ray at
// emission, then one shadow ray for the hit, which is certain (a sphere is hit, whatever the mesh says) and diffuse (every object is).  Only the plain later launch (form 0)
// skips; its counting twin (kFormStats) traces every ray and counts the ones the rule would have kept from the traversal, those that pass the root box (Work::dead_last).
constexpr int kPolDeadLast = 1 << 8;
typedef float pol_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 pol_load(const float4 *p, bool nt) {
    if (nt) { const pol_f4 v = __builtin_nontemporal_load(reinterpret_cast<const pol_f4 *>(p)); return make_float4(v.x, v.y, v.z, v.w); }
    return *p;
}
__device__ __forceinline__ void pol_store(float4 *p, float4 v, bool nt) {
    if (nt) { pol_f4 w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; __builtin_nontemporal_store(w, reinterpret_cast<pol_f4 *>(p)); }
    else *p = v;
}

// n / d for 0 <= n < 2^32 with m = floor(2^32 / d) from the host: the estimate mulhi(n, m) is the quotient or one below it
// (n * m / 2^32 > n / d - 1), so one correction makes it exact -- 5 vector instructions instead of the ~22 of an integer division.
__device__ __forceinline__ int wf_div(int n, int d, unsigned int m) {
    unsigned int q = __umulhi((unsigned int)n, m);
    q += ((unsigned int)n - q * (unsigned int)d >= (unsigned int)d) ? 1u : 0u;
    return (int)q;
}
__host__ __device__ inline unsigned int wf_div_magic(int d) { return d <= 1 ? 0xffffffffu : (unsigned int)(0x100000000ull / (unsigned long long)d); }

__device__ __forceinline__ void wf_decode(const WfState &st, const Frame &fr, int slot, int &px, int &lrow, bool &valid) {
    const int tile = slot >> 6, p = slot & 63;
    const int ty = wf_div(tile, st.tiles_x, st.tiles_x_m);
    px = (tile - ty * st.tiles_x) * 8 + (p & 7);
    lrow = ty * 8 + (p >> 3);
    valid = px < fr.W && lrow < fr.n_rows;
}

// Scene::intersect_all's running minimum over the SPHERES alone, for the two rays that leave one point (origins equal bit for bit: the origin part of every sphere test
// is shared): (t, object id) of the nearest sphere with the strict '<' of cpu:554 (the earliest of equal t).  The meshes join when the traversal is back: a triangle at tm replaces the sphere iff tm < t, or tm == t and the
// triangle's mesh comes before the sphere in Scene::objects -- the lexicographic minimum over (t, position) IS what the reference's loop keeps.
struct SphereNear { float t; int obj; };
__device__ __forceinline__ SphereNear spheres_near1(const Scene &sc, f3 O, f3 u) {   // ... for one ray (wf_path)
    SphereNear h; h.t = 1e9f; h.obj = -1;
    for (int k = 0; k < sc.n_spheres; ++k) {
        float t;
        if (sphere_test(sc.sph[k], O, u, t) && t < h.t) { h.t = t; h.obj = sc.sph[k].obj; }
    }
    return h;
}
// (sphere_at(k): sphere k of the scene -- Scene::sph, or the pose a frame of an animated batch gives it)
template <class SphereAt>
__device__ __forceinline__ void spheres_near2(int n_spheres, SphereAt sphere_at, f3 O, f3 uy, bool on_y, f3 ux, bool on_x, SphereNear &hy, SphereNear &hx) {
    hy.t = 1e9f; hy.obj = -1;
    hx = hy;
    for (int k = 0; k < n_spheres; ++k) {
        const auto &s = sphere_at(k);
        const SphereOrigin so = sphere_origin(s, O);
        float t;
        if (on_y && sphere_dir(s, so, O, uy, t)) { if (t < hy.t) { hy.t = t; hy.obj = s.obj; } }
        if (on_x && sphere_dir(s, so, O, ux, t)) { if (t < hx.t) { hx.t = t; hx.obj = s.obj; } }
    }
}
__device__ __forceinline__ void spheres_near2(const Scene &sc, f3 O, f3 uy, bool on_y, f3 ux, bool on_x, SphereNear &hy, SphereNear &hx) {
    spheres_near2(sc.n_spheres, [&](int k) -> const Sphere & { return sc.sph[k]; }, O, uy, on_y, ux, on_x, hy, hx);
}
// ... with the spheres where this frame of an animated batch has them (AnimFrame::sph: centre and R2; which object a sphere is does not change)
__device__ __forceinline__ void spheres_near2(const Scene &sc, const float4 *__restrict__ pose, f3 O, f3 uy, bool on_y, f3 ux, bool on_x, SphereNear &hy, SphereNear &hx) {
    spheres_near2(sc.n_spheres, [&](int k) { const float4 c = pose[k]; return Sphere{c.x, c.y, c.z, 0.f, c.w, sc.sph[k].obj}; }, O, uy, on_y, ux, on_x, hy, hx);
}
// inverse of wf_slot_to_path: the traversal slot of ray r
__device__ __forceinline__ int wf_ray_to_slot(const WfState &st, int r) {
    const int g = r >> 2;
    const int a = wf_div(g, st.Q, st.Q_m), col = g - a * st.Q;
    return ((col << st.log2S | a) << 2) | (r & 3);
}

// The mesh's root-box test of an emitted ray (cpu:279; wave-uniform node data from kernel arguments): whether the ray needs traversal.
template <bool STATS>
__device__ __forceinline__ bool wf_root_test(const Scene &sc, const WfState &st, int r, f3 O, f3 u, Work &wk) {
    bool need = false;
    if (sc.mesh_slot >= 0 && sc.n_nodes > 0) {
        if (STATS) wk.box++;
        if (slab_filtered(sc.root_lo, sc.root_hi, O, u, ray_inv(u))) {
            if (STATS) wk.nodes++;
            need = true;
            if (st.init_m) st.M[r] = WF_NOHIT;
        }
    }
    return need;
}

template <bool STATS>
__device__ __forceinline__ void wf_flush_work(const Frame &fr, Work &wk) {
    if (STATS) {
        const uint32_t b = wave_sum(wk.box), n = wave_sum(wk.nodes), t = wave_sum(wk.tris), lb = wave_sum(wk.lit_box), lt = wave_sum(wk.lit_tri);
        // rays handed to the traversal (continuation, shadow), shadow rays the dead-channel rule elided, paths outside its guarantee: rt_dead_channel_counts
        const uint32_t ty = wave_sum(wk.trav_y), tx = wave_sum(wk.trav_x), de = wave_sum(wk.dead_elided), du = wave_sum(wk.dead_unsure);
        const uint32_t dl = wave_sum(wk.dead_last);                    // continuation rays the dead-last rule would skip (kPolDeadLast): rt_dead_last_count
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&fr.work[1], (unsigned long long)b);
            atomicAdd(&fr.work[2], (unsigned long long)n); atomicAdd(&fr.work[3], (unsigned long long)t);
            if (lb) atomicAdd(&fr.work[5], (unsigned long long)lb);
            if (lt) atomicAdd(&fr.work[6], (unsigned long long)lt);
            if (ty) atomicAdd(&fr.work[20], (unsigned long long)ty);
            if (tx) atomicAdd(&fr.work[21], (unsigned long long)tx);
            if (de) atomicAdd(&fr.work[22], (unsigned long long)de);
            if (du) atomicAdd(&fr.work[23], (unsigned long long)du);
            if (dl) atomicAdd(&fr.work[7], (unsigned long long)dl);
        }
    }
}

// ---- wf_trav: persistent stackless traversal -----------------------------------------------------------
// Hot loop = BOX steps only.  A lane that hits a leaf appends (first, count) to its private LDS leaf list and
// keeps walking; nothing else happens in the loop but one wave vote.  When fewer than kBoxMin lanes can
// still walk, a SERVICE pass runs: leaf lists are expanded into the wave's LDS ring of (owner lane, triangle)
// entries, the ring is consumed 64 entries at a time by full-occupancy TRI steps (ray data from the owners'
// LDS copies, results merged by a 64-bit LDS min on bits(t) << 32 | triangle), finished tasks retire, idle
// lanes refill from the wave's scrambled share of the rays or take a split from a busy lane.
constexpr int kTravBlock = 512;             // nodes from HBM/L2: 512-thread blocks (8 waves share one slot pool), 3 per CU
constexpr int kTravBlockLds = 1024;         // nodes staged in LDS: ONE 1024-thread block per CU shares the copy
#ifndef RT_BOXMIN
#define RT_BOXMIN 36
#endif
constexpr int kBoxMin = RT_BOXMIN;                 // service when fewer lanes than this can take a BOX step

// per-wave LDS carve: ray0[64] ray1[64] (float4) | best[64] (u64) | ring[QCAP] (u32) | leaf[LEAFCAP][64] (u32)
template <int QCAP, int LEAFCAP> struct TravCarve {
    static constexpr int kRay = 0, kBest = 2048, kRing = 2560, kLeaf = kRing + 4 * QCAP, kBytes = kLeaf + 256 * LEAFCAP;
};

__device__ __forceinline__ int wf_slot_to_path(const WfState &st, int q) {
    const int gs = q >> 2;
    const int col = gs >> st.log2S;                  // >= Q for the padding slots of the last waves
    const int g = (gs & ((1 << st.log2S) - 1)) * st.Q + col;
    return (col < st.Q && g < st.n_groups) ? 4 * g + (q & 3) : -1;
}

// single-instruction min/max (the operands are results of arithmetic, never signalling NaNs; IEEE-mode
// v_min/v_max return the other operand for a quiet NaN, which the callers exclude beforehand)
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float vmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float vmax3abs(float a, float b, float c) { float r; asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// Per-ray constants of the fused box filter.  q~ = fma(bound, r, -fl(O*r)) differs from the reference's
// RN((bound - O)/u) by at most 2^-21 |q| + 2^-24 |O*r| (+ denormal slack): r carries 2^-23, fl(O*r) 2^-24 of
// |O*r|, the fma 2^-24, the reference's own subtraction and division 2^-24 each.
struct RayBox { float rx, ry, rz, ox, oy, oz, c0; bool safe; };
__device__ __forceinline__ RayBox ray_box(f3 O, f3 u) {
    RayBox b;
    b.rx = __builtin_amdgcn_rcpf(u.x); b.ry = __builtin_amdgcn_rcpf(u.y); b.rz = __builtin_amdgcn_rcpf(u.z);
    b.ox = O.x * b.rx; b.oy = O.y * b.ry; b.oz = O.z * b.rz;
    const float omax = vmax3abs(b.ox, b.oy, b.oz);
    b.c0 = 2.f * (omax * 0x1p-24f + kAbs);
    const float umin = fminf(fminf(fabsf(u.x), fabsf(u.y)), fabsf(u.z)), umax = fmaxf(fmaxf(fabsf(u.x), fabsf(u.y)), fabsf(u.z));
    b.safe = umin > kTiny && umax < kBig && omax < kBig;      // false for 0, denormal, inf, NaN anywhere
    return b;
}

template <bool STATS, bool LDSN>
__global__ __launch_bounds__(LDSN ? kTravBlockLds : kTravBlock) void wf_trav(const Scene sc, const Frame fr, const WfState st) {
    constexpr int kQCap = LDSN ? 256 : 512;         // ring entries per wave (power of two)
    constexpr int kLeafCap = LDSN ? 4 : 8;          // leaf-list entries per lane
    using Carve = TravCarve<kQCap, kLeafCap>;
    extern __shared__ __attribute__((aligned(16))) unsigned char trav_smem[];
    unsigned char *const smem = trav_smem;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wib = tid >> 6;                       // wave in block
    const int wave = (blockIdx.x * blockDim.x + tid) >> 6;
    // LDS: [LDSN: every node, 2 x float4 each] then one carve per wave
    const float4 *nodes = sc.nodes;
    unsigned char *wl = smem + wib * Carve::kBytes;
    if (LDSN) {
        float4 *ln = reinterpret_cast<float4 *>(smem);
        for (int k = tid; k < 2 * sc.n_nodes; k += blockDim.x) ln[k] = sc.nodes[k];
        __syncthreads();
        nodes = ln;
        wl += (size_t)sc.n_nodes * 32;
    }
    // the workgroup's slot cursor: waves take slots with one LDS atomic per refill, which evens out the cost
    // variance between the waves of a workgroup
    int *const blk_cur = reinterpret_cast<int *>(smem + (LDSN ? (size_t)sc.n_nodes * 32 : 0) + (blockDim.x >> 6) * Carve::kBytes);
    if (tid == 0) *blk_cur = 0;
    __syncthreads();
    float4 *const lray0 = reinterpret_cast<float4 *>(wl + Carve::kRay);
    float4 *const lray1 = lray0 + 64;
    unsigned long long *const lbest = reinterpret_cast<unsigned long long *>(wl + Carve::kBest);
    unsigned int *const q = reinterpret_cast<unsigned int *>(wl + Carve::kRing);
    unsigned int *const leaf = reinterpret_cast<unsigned int *>(wl + Carve::kLeaf) + lane;     // leaf[k * 64]
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    // lane state: a task = traversal of node range [node, nend) of ray `ray`
    int ray = -1;                       // path index, -1 = idle
    f3 O = mk(0, 0, 0), u = mk(0, 0, 1);
    RayBox rb = ray_box(O, u);
    int node = 0, nend = 0, sk = 0;
    int nl = 0;                         // entries in the lane's leaf list
    int pend_first = 0, pend_cnt = 0;   // triangle range currently being queued
    unsigned int last_pos = 0;          // ring position after this task's last queued entry
    bool shared = false;                // this ray's traversal was split: merge with a global atomic
    // wave-uniform: the wave's own ray slots and its ring cursors (monotonic positions)
    const int blk_base = blockIdx.x * st.slots_per_block;
    const int blk_n = st.slots_per_block;
    bool drained = false;
    unsigned int qhead = 0, qtail = 0;
    Work wk;
#ifdef RT_DEBUG
    const bool dbg_on = st.dbg != nullptr;
#else
    constexpr bool dbg_on = false;
#endif
    const unsigned long long dbg_t0 = dbg_on ? __builtin_amdgcn_s_memrealtime() : 0ull;
    unsigned int dbg_steps = 0, dbg_lanes = 0, dbg_splits = 0;
    unsigned long long cy_box = 0, cy_tri = 0, cy_exp = 0, cy_ref = 0, stamp = 0;
#define WF_STAMP(acc) do { if (dbg_on) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); acc += t_ - stamp; stamp = t_; } } while (0)
    if (dbg_on) stamp = __builtin_amdgcn_s_memtime();
    bool boxable = false;
    for (;;) {
        int nB = __popcll(__ballot(boxable));
        if (nB < kBoxMin) {
            // =============================== SERVICE ===============================
            for (;;) {
                WF_STAMP(cy_box);
                // ---- (1) expand leaf lists into the ring, one entry per lane and round ----
                for (;;) {
                    if (pend_cnt == 0 && nl > 0) {
                        nl--;
                        const unsigned int e = leaf[nl * 64];
                        pend_first = (int)(e & 0x3ffffffu); pend_cnt = (int)(e >> 26);
                    }
                    const unsigned long long pm = __ballot(pend_cnt > 0);
                    if (!pm || (unsigned int)kQCap - (qtail - qhead) < 64u) break;
                    if (pend_cnt > 0) {
                        const unsigned int pos = qtail + (unsigned int)__popcll(pm & lane_lt);
                        q[pos & (kQCap - 1)] = (unsigned int)lane << 26 | (unsigned int)pend_first;
                        pend_first++; pend_cnt--;
                        last_pos = pos + 1u;
                    }
                    qtail += (unsigned int)__popcll(pm);
                }
                WF_STAMP(cy_exp);
                // ---- (2) TRI steps: 64 queued (owner, triangle) pairs, one per lane ----
                const bool walkable = ray >= 0 && node < nend && nl < kLeafCap && pend_cnt == 0;
                const int nW = __popcll(__ballot(walkable));
                for (;;) {
                    const unsigned int count = qtail - qhead;
                    if (count < 64u && !(count > 0u && nW < kBoxMin)) break;
                    const unsigned int n = count < 64u ? count : 64u;
                    dbg_steps++; dbg_lanes += n;
                    if ((unsigned int)lane < n) {
                        const unsigned int e = q[(qhead + (unsigned int)lane) & (kQCap - 1)];
                        const int o = (int)(e >> 26);
                        const int i = (int)(e & 0x3ffffffu);
                        const float4 *tp = sc.tri + 3 * i;
                        const float4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
                        const float4 r0 = lray0[o], r1 = lray1[o];
                        const f3 Oo = mk(r0.x, r0.y, r0.z), uo = mk(r0.w, r1.x, r1.y);
                        const f3 A = mk(q0.x, q0.y, q0.z), e1 = mk(q0.w, q1.x, q1.y), e2 = mk(q1.z, q1.w, q2.x);
                        const f3 N = mk(q2.y, q2.z, q2.w);
                        const float det = dot(uo, N);               // moller_trumbore, cpu:226-236
                        const f3 AO = A - Oo;
                        const f3 c = cross(AO, uo);
                        const float bn = dot(e2, c);
                        const float gn = -dot(e1, c);
                        const float rd = __builtin_amdgcn_rcpf(det);
                        const float b = bn * rd, g = gn * rd;
                        const float eb = fmaf(fabsf(b), kRel, kAbs), eg = fmaf(fabsf(g), kRel, kAbs);
                        const float sum = b + g;
                        const float es = fmaf(fabsf(sum), 0x1p-22f, eb + eg);
                        const bool trust = fabsf(det) > kTiny;      // also false for det == 0 and NaN
                        const bool reject = trust && (b < -eb || b > 1.f + eb || g < -eg || g > 1.f + eg || sum > 1.f + es);
                        bool ok = trust && b >= eb && b <= 1.f - eb && g >= eg && g <= 1.f - eg && sum <= 1.f - es;
                        if (!reject && !ok && det != 0) {           // undecided: the literal tests (rare)
                            const float beta = bn / det;
                            const float gamma = gn / det;
                            ok = (0 <= beta && beta <= 1) && (0 <= gamma && gamma <= 1) && (beta + gamma <= 1);
                        }
                        if (ok) {
                            const float t = dot(AO, N) / det;
                            if (t > 0 && t > fr.tri_tmin && t < 1e9f)    // cpu:235,301; the min is the strict '<' scan
                                atomicMin(&lbest[o], (unsigned long long)__float_as_uint(t) << 32 | (unsigned int)i);
                        }
                    }
                    qhead += n;
                }
                WF_STAMP(cy_tri);
                // ---- (3) retire tasks whose nodes are walked and whose queued triangles have all been tested ----
                if (ray >= 0 && node >= nend && nl == 0 && pend_cnt == 0 && (int)(qhead - last_pos) >= 0) {
                    const unsigned long long key = lbest[lane];
                    if (key != WF_NOHIT) {
                        if (shared) atomicMin(&st.M[ray], key);
                        else st.M[ray] = key;
                    }
                    ray = -1;
                }
                // ---- (4) refill idle lanes from the wave's slots, or split ----
                const unsigned long long idle = __ballot(ray < 0);
                const int n_idle = __popcll(idle);
                if (n_idle && !drained) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(blk_cur, n_idle);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base + n_idle >= blk_n) drained = true;
                    if (ray < 0) {
                        const int qo = base + __popcll(idle & lane_lt);
                        const float4 rq = qo < blk_n ? st.QR[2 * ((size_t)blk_base + qo) + 1] : make_float4(0, 0, 0, 0);
                        const int rf = wq_live(__float_as_int(rq.z), st.epoch, st.nonce) ? wf_slot_to_path(st, blk_base + qo) + 1 : 0;   // ray + 1 if the slot's ray needs traversal
                        if (rf != 0) {
                            const int path = rf - 1;
                            {
                                const float4 r0 = st.QR[2 * ((size_t)blk_base + qo)];
                                const float4 r1 = make_float4(rq.x, rq.y, 0.f, 0.f);
                                O = mk(r0.x, r0.y, r0.z); u = mk(r0.w, r1.x, r1.y);
                                rb = ray_box(O, u);
                                lray0[lane] = r0; lray1[lane] = r1; lbest[lane] = WF_NOHIT;
                                // the root box was tested when the ray was emitted; start below it
                                const int rw = __float_as_int(sc.root_hi.w);
                                node = rw < 0 ? 1 : sc.n_nodes; nend = sc.n_nodes; sk = 0; nl = 0;
                                pend_first = rw < 0 ? 0 : __float_as_int(sc.root_lo.w);
                                pend_cnt = rw < 0 ? 0 : rw - pend_first;
                                if (STATS && rw >= 0) wk.tris += (uint32_t)pend_cnt;
                                last_pos = qhead; shared = false;
                                ray = path;
                            }
                        }
                    }
                } else if (n_idle >= 4 && n_idle < 64) {
                    // a busy lane below a hit internal node X keeps [node, skip(X)) and gives [skip(X), nend) away
                    const bool d_skip = ray >= 0 && sk > node && sk < nend;
                    const unsigned long long donors = __ballot(d_skip);
                    if (donors) {
                        const int n_pairs = min(n_idle, __popcll(donors));
                        const int my_idle_rank = __popcll(idle & lane_lt);
                        const int my_donor_rank = __popcll(donors & lane_lt);
                        int partner = -1;
                        if (ray < 0 && my_idle_rank < n_pairs) {   // lane id of the my_idle_rank-th donor
                            unsigned long long m = donors;
                            for (int k = 0; k < my_idle_rank; ++k) m &= m - 1;
                            partner = __ffsll((long long)m) - 1;
                        }
                        const bool is_donor = ((donors >> lane) & 1ull) && my_donor_rank < n_pairs;
                        int g_node = 0, g_nend = 0;
                        if (is_donor) { g_node = sk; g_nend = nend; nend = sk; shared = true; }
                        const int src = partner >= 0 ? partner : lane;
                        const int r_ray = __shfl(ray, src, 64);
                        const float r_ox = __shfl(O.x, src, 64), r_oy = __shfl(O.y, src, 64), r_oz = __shfl(O.z, src, 64);
                        const float r_ux = __shfl(u.x, src, 64), r_uy = __shfl(u.y, src, 64), r_uz = __shfl(u.z, src, 64);
                        const int r_node = __shfl(g_node, src, 64), r_nend = __shfl(g_nend, src, 64);
                        if (partner >= 0) {
                            ray = r_ray; O = mk(r_ox, r_oy, r_oz); u = mk(r_ux, r_uy, r_uz); rb = ray_box(O, u);
                            lray0[lane] = make_float4(O.x, O.y, O.z, u.x); lray1[lane] = make_float4(u.y, u.z, 0, 0);
                            lbest[lane] = WF_NOHIT;
                            node = r_node; nend = r_nend; sk = 0; nl = 0; pend_cnt = 0;
                            last_pos = qhead; shared = true;
                        }
                        dbg_splits += n_pairs;
                    }
                }
                WF_STAMP(cy_ref);
                // ---- done servicing? ----
                boxable = ray >= 0 && node < nend && nl < kLeafCap && pend_cnt == 0;
                nB = __popcll(__ballot(boxable));
                if (nB >= kBoxMin) break;
                const bool more = (qtail != qhead) || __ballot(pend_cnt > 0 || nl > 0) != 0ull || (!drained && __ballot(ray < 0) != 0ull);
                if (more) continue;                                  // queue to drain / lists to expand / rays to fetch
                if (nB > 0) break;                                   // run with the lanes we have
                if (__ballot(ray >= 0) == 0ull) goto finished;       // nothing left anywhere
                // busy lanes that are neither walkable nor retired can only be waiting for the ring, which is empty,
                // so the next pass retires them
            }
        }
        // =============================== BOX step ===============================
        dbg_steps++; dbg_lanes += nB;
        if (boxable) {
            const float4 *np = nodes + 2 * node;
            const float4 lo = np[0], hi = np[1];
            const int hiw = __float_as_int(hi.w);
            const int low = __float_as_int(lo.w);
            if (STATS) wk.box++;
            // BoundingBox::intersect (cpu:146-157) through the fused filter
            const float ax = fmaf(lo.x, rb.rx, -rb.ox), bx = fmaf(hi.x, rb.rx, -rb.ox);
            const float ay = fmaf(lo.y, rb.ry, -rb.oy), by = fmaf(hi.y, rb.ry, -rb.oy);
            const float az = fmaf(lo.z, rb.rz, -rb.oz), bz = fmaf(hi.z, rb.rz, -rb.oz);
            const float tn = vmax3(vmin(ax, bx), vmin(ay, by), vmin(az, bz));
            const float tf = vmin3(vmax(ax, bx), vmax(ay, by), vmax(az, bz));
            const float M = vmax(vmax3abs(ax, bx, ay), vmax3abs(by, az, bz));
            const float d = tf - tn;
            const float band = fmaf(M, 2.f * kRel, rb.c0);
            bool hit = d > band;
            const bool decided = rb.safe && M < kBig && (hit || d < -band);
            // literal arithmetic for undecided lanes: behind a wave-uniform branch so that the six IEEE divisions are
            // skipped, not if-converted, when (as almost always) every lane decided
            if (__builtin_expect(__ballot(!decided) != 0ull, 0)) {
                if (!decided) hit = slab(lo, hi, O, u);
            }
            int next = node + 1;
            if (hit) {
                if (STATS) wk.nodes++;
                if (hiw >= 0) {                                // leaf: triangles [low, hiw)
                    const int cnt = hiw - low;
                    if (STATS) wk.tris += (uint32_t)cnt;
                    if (cnt <= 63) { leaf[nl * 64] = (unsigned int)cnt << 26 | (unsigned int)low; nl++; }
                    else { pend_first = low; pend_cnt = cnt; }
                } else {
                    sk = low;                                  // everything from skip(node) on can be given away
                }
            } else if (hiw < 0) {
                next = low;
            }
            node = next;
            boxable = next < nend && nl < kLeafCap && pend_cnt == 0;
        }
    }
finished:
    if (dbg_on && lane == 0) {
        st.dbg[6 * wave + 0] = dbg_t0; st.dbg[6 * wave + 1] = __builtin_amdgcn_s_memrealtime();
        st.dbg[6 * wave + 2] = dbg_steps; st.dbg[6 * wave + 3] = dbg_lanes; st.dbg[6 * wave + 4] = dbg_splits; st.dbg[6 * wave + 5] = 0;
        unsigned long long *d2 = st.dbg + 6 * 65536 + 4 * wave;
        d2[0] = cy_box; d2[1] = cy_exp; d2[2] = cy_tri; d2[3] = cy_ref;
    }
#undef WF_STAMP
    wf_flush_work<STATS>(fr, wk);
}

// ---- textured meshes (rt_mesh_set_texture[_of], raytrace_hip.h) ----------------------------------------------
// A texture is the first material property that changes from one hit to the next: a diffuse segment of a textured mesh stores its albedo
// (mesh albedo (.) sampled texel, MTL's Kd x map_Kd) in ALB when it is shaded and the fold reads it there (SID == kSidTextured) instead of
// looking the object's constant albedo up.  Only wf_advance<kFormTex> carries this code; frames without a textured mesh run wf_advance unchanged.
constexpr int kMaxObjects = 16;              // RT_MAX_OBJECTS: the texture table is indexed by object id
constexpr int kSidTextured = 0xfe;           // SID of a textured diffuse segment (object ids are < kMaxObjects, 0xff = not diffuse)
struct TexDesc {                             // the texture of one object
    const uint8_t *texels;                   // h rows of w texels, top row first, ch (3 or 4) bytes each; alpha is never read
    const float *decode;                     // 256 floats: the channel value of a byte
    int w, h, ch, filter, wrap, pad;         // filter 0 nearest / 1 bilinear, wrap 0 repeat / 1 clamp
};
struct TexScene {
    const float2 *uv;                        // 3 per triangle (corners a, b, c = the vertices of its record), visit order; read for textured meshes only
    const TexDesc *desc;                     // [kMaxObjects] by object id (device memory: read with a per-lane index)
    float4 *ALB;                             // albedo of textured diffuse segment d of path i: ALB[d * n_paths + i]
    int mask;                                // bit k: object k is a textured mesh
};
// (tex_floor and tex_wrap, the texel coordinate's floor and its wrap, are in rt_shade.hip.h: the environment map's lookup shares them)
__device__ __forceinline__ f3 tex_texel(const TexDesc &td, int x, int y) {
    const uint8_t *p = td.texels + ((size_t)y * (size_t)td.w + (size_t)x) * (size_t)td.ch;
    return mk(td.decode[p[0]], td.decode[p[1]], td.decode[p[2]]);
}
// the texture at (u, v): nearest x = floor(u W), y = floor((1 - v) H); bilinear from s = u W - 0.5, t = (1 - v) H - 0.5 -- every operation one binary32 rounding
__device__ __forceinline__ f3 tex_sample(const TexDesc &td, float u, float v) {
    const float W = (float)td.w, H = (float)td.h;
    float fx, fy;
    if (td.filter == 0) {
        const int x = tex_wrap(tex_floor(u * W, fx), td.w, td.wrap), y = tex_wrap(tex_floor((1.f - v) * H, fy), td.h, td.wrap);
        return tex_texel(td, x, y);
    }
    const int x0 = tex_floor(u * W - 0.5f, fx), y0 = tex_floor((1.f - v) * H - 0.5f, fy);
    const int xa = tex_wrap(x0, td.w, td.wrap), xb = tex_wrap(x0 + 1, td.w, td.wrap);
    const int ya = tex_wrap(y0, td.h, td.wrap), yb = tex_wrap(y0 + 1, td.h, td.wrap);
    const f3 t00 = tex_texel(td, xa, ya), t10 = tex_texel(td, xb, ya), t01 = tex_texel(td, xa, yb), t11 = tex_texel(td, xb, yb);
    const float gx = 1.f - fx, gy = 1.f - fy;
    return mk((t00.x * gx + t10.x * fx) * gy + (t01.x * gx + t11.x * fx) * fy,
              (t00.y * gx + t10.y * fx) * gy + (t01.y * gx + t11.y * fx) * fy,
              (t00.z * gx + t10.z * fx) * gy + (t01.z * gx + t11.z * fx) * fy);
}
// albedo of a hit on triangle `tri` of textured object `obj`: uv = (alpha uv_a + beta uv_b) + gamma uv_c, then mesh albedo (.) texture(uv).  wf_advance<kFormTex> and
// rt_kat_surface call this one function.
__device__ __forceinline__ f3 tex_albedo(const Scene &sc, const TexScene &ts, int obj, int tri, const Bary &b, float2 &uv) {
    const float2 ua = ts.uv[3 * tri], ub = ts.uv[3 * tri + 1], uc = ts.uv[3 * tri + 2];
    uv.x = (b.alpha * ua.x + b.beta * ub.x) + b.gamma * uc.x;
    uv.y = (b.alpha * ua.y + b.beta * ub.y) + b.gamma * uc.y;
    const TexDesc td = ts.desc[obj];
    const f3 s = tex_sample(td, uv.x, uv.y);
    const Material m = material_of(sc, obj);
    return mk(m.ar * s.x, m.ag * s.y, m.ab * s.z);
}

// ---- wf_advance: close the queries, shade, emit the next rays -----------------------------------------------
// FIRST: the launch that opens the chain's samples -- camera rays instead of closing queries.
// TEX (wf_advance<kFormTex>, never FIRST): textured meshes -- the albedo of a textured diffuse hit goes to ts.ALB and the fold reads it from there.
// ANIM (wf_advance<kFormAnim>, wf_advance<kFormTex | kFormAnim>; batches only): the frame's light and sphere poses come from anim[frame] instead of the Scene -- the same device functions on
// other operands; the other instantiations never look at `anim`.
// LIST (wf_advance<kFormList>, wf_advance<kFormTex | kFormList>; the chains of rt_adaptive.hip.h): the chain's items are a list of (pixel slot, sample) records instead of the grid "pixel slot x sample" --
// pixel, sample and validity come from list.items[i]; every item writes samp_out[i]; the other instantiations never look at `list`.
// The samples of a pixel are independent paths (the reference's loop cpu:701-712 carries nothing but the sum): a chain traces
// several of them at once as items, each writes its colour, and path_reduce adds the colours in sample order.
// code-object markers (labels, not instructions): tools/static_counts.py cuts the production instantiation into regions at them -- what a path pays for, region by region
#ifdef RT_NO_MARKS
#define ADV_MARK(name) do { } while (0)
#else
// (the compiler numbers the labels through the translation unit: the LIGHTS instantiations of wf_advance_path plant none, so that every other kernel's labels, and with
// them its text, stay what they were before those two existed -- tools/asm_compare.py; neither does the LENS instantiation, nor the SHUTTER ones, nor the SKY ones, nor the EMIT ones, nor the FRESNEL ones, nor the GLOSS ones -- the TINT ones are GLOSS ones)
#define ADV_MARK(name) do { if constexpr (!LIGHTS && !LENS && !SHUTTER && !SKY && !SAMPLE && !EMIT && !FRESNEL && !GLOSS) asm volatile("rt_mark_adv_" name "_%=:" ::); } while (0)
#endif
struct WfList {
    const unsigned int *items;   // [n_paths] pixel slot << 6 | sample index; entries from n on are padding
    int n;                       // items of this chain (n_paths is n rounded up to 64)
};
// The FIRST-SHADE cache (rt_host_ctx.hip.h FirstShade; wf_advance<kFormFill>, wf_advance<kFormResume>): one 32-byte record per PIXEL SLOT, the part's block -- the slot's path after
// segment 0 is shaded and its shadow ray decided, before the bounce direction (the first thing that reads the sample's key).  rec[2 k] = (origin of the continuation ray:
// P_adjusted of a diffuse hit, the mirrored / refracted origin otherwise; V.x), rec[2 k + 1] = (V.y, V.z, l0, word): V the normal of a diffuse hit, the continuation
// direction of a specular one; l0 the FINAL direct term of segment 0 (lvis, or +0 where a sphere or the mesh shades it; a moot or elided ray keeps lvis, as LS does);
// word = kind | SID byte << 8 | refr_code << 16 | DCH byte after segment 0 << 22 | rays counted so far (the continuation ray not among them) << 26.
constexpr int kShadeMiss = 0, kShadeDiffuse = 1, kShadeSpecular = 2;
constexpr int SH_SID_SHIFT = 8, SH_REFR_SHIFT = 16, SH_DCH_SHIFT = 22, SH_RAYS_SHIFT = 26;
struct WfShade {
    float4 *rec;                 // [2 n_px]
    int kill_x;                  // (resume) the chain's traversal launch 1 scans shadow rows: every item writes the dead second half into its X slot (see wq_live)
};
__device__ __forceinline__ void wf_shade_store(const WfShade &sh, int slot, int kind, f3 O, f3 V, float l0, int sid, int refr_code, int dch, int nrays) {
    const int word = kind | (sid << SH_SID_SHIFT) | (refr_code << SH_REFR_SHIFT) | (dch << SH_DCH_SHIFT) | (int)((unsigned)nrays << SH_RAYS_SHIFT);
    sh.rec[2 * (size_t)slot] = make_float4(O.x, O.y, O.z, V.x);
    sh.rec[2 * (size_t)slot + 1] = make_float4(V.y, V.z, l0, __int_as_float(word));
}
// Whether the shadow ray of a path with flag word F is blocked (cpu:615): by a sphere (decided at emission: PQ_XSPHERE), or by the triangle of its traversal word.  The close
// of the X query and the first-shade fill both decide through this one function: load_m() is the ray's word (read only if the ray went to the mesh), load_ray(O, u) the ray;
// xm: the word if it was read.
template <class LoadM, class LoadRay>
__device__ __forceinline__ bool wf_x_shadowed(int F, f3 L, LoadM load_m, LoadRay load_ray, unsigned long long &xm) {
    bool shadowed = (F & PQ_XSPHERE) != 0;
    if (!shadowed && (F & PF_MESHX)) {
        const unsigned long long m = load_m();
        xm = m;
        if (m != WF_NOHIT) {
            f3 Oxr, uxr;
            load_ray(Oxr, uxr);
            shadowed = light_hidden(Oxr, uxr, __uint_as_float((unsigned int)(m >> 32)), L);   // (Ox is P_adjusted)
        }
    }
    return shadowed;
}
// SHADE 1 (wf_advance<kFormFill>): the launch that emits segment 0's shadow rays in a chain that READS the first-shadow cache also stores the first-shade records of its
// first-sample items.  SHADE 2 (wf_advance<kFormResume>): the launch that opens a chain whose part's records are stored -- in place of wf_advance<kFormFirst> and the launch that closes
// segment 0.  The other instantiations never look at `sh`.
// SEVERAL POINT LIGHTS (rt_scene_set_lights; the rule: raytrace_hip.h "several point lights").  A diffuse segment still emits ONE shadow ray: to the light the sample's key
// picks with probability proportional to its intensity, so that the estimator's weight I_k / p_k is the same number for every light -- the total.  The table is a kernel
// argument of the two instantiations that read it (wf_advance<kFormLights>, wf_advance<kFormTex | kFormLights>: LIGHTS) and of no other kernel: rtk::Scene does not grow.
constexpr int kMaxLights = 16;               // RT_MAX_LIGHTS
struct WfLights {
    float4 pos[kMaxLights];                  // (position of light k, prefix[k] = fl(prefix[k - 1] + I_k)); entries from n on repeat the last one
    float total;                             // prefix[n - 1]: the only intensity the shading sees
    int n;
};
// the light of segment `seg` of the path whose sample key is hs: r = uniform01(hs, seg + 1, 2), x = fl(r total), the least k with prefix[k] >= x and prefix[k] > 0.  The
// prefix sums do not decrease and r is in (0, 1], so both conditions hold from some k <= n - 1 on: k is the number of entries that fail.  The loop reads the table with a
// wave-uniform index (scalar loads); the one per-lane read is the position, from the argument segment.
__device__ __forceinline__ f3 wf_light_pick(const WfLights &lt, uint32_t hs, int seg) {
    const float x = uniform01(hs, (uint32_t)(seg + 1), 2) * lt.total;
    int k = 0;
    for (int j = 0; j < lt.n; ++j) k += (lt.pos[j].w >= x && lt.pos[j].w > 0.f) ? 0 : 1;
    const float4 p = lt.pos[k < kMaxLights - 1 ? k : kMaxLights - 1];
    return mk(p.x, p.y, p.z);
}
// LIGHTS WITH A RADIUS (rt_scene_set_light_radii; the rule: raytrace_hip.h "soft shadows").  Light k is a shell of point emitters of radius rho_k about L_k; a segment's
// operand is one point of it, L' = L_k + rho_k w(hs, seg), and everything downstream is the point-light code on L'.  The two instantiations that read the radii
// (wf_advance<kFormSoft>, wf_advance<kFormTex | kFormSoft>: LIGHTS == 2) take the table extended by them; WfLights as the LIGHTS == 1 kernels receive it is what it was.
struct WfSoftLights {
    WfLights lt;
    float radius[kMaxLights];                // rho_k; entries from n on repeat the last one
};
// the point of the picked light that segment `seg` sees: w uniform on the unit sphere from the two draws at depth 2^29 + seg (the RNG keys on depth * 4 + dim modulo 2^32:
// 2^31 + 4 seg + dim, which no jitter, bounce or pick draw reaches), in the forms cosine_bounce uses; a light of radius 0 is L_k itself, bit for bit (-0 included).  A soft
// list of ONE light has every entry of the table equal: whatever its intensity is -- zero, negative, NaN -- the index lands on it.
__device__ __forceinline__ f3 wf_light_point(const WfSoftLights &sl, uint32_t hs, int seg) {
    const float xk = uniform01(hs, (uint32_t)(seg + 1), 2) * sl.lt.total;   // wf_light_pick's k (that function, as the LIGHTS == 1 kernels compile it, stays as it is)
    int k = 0;
    for (int j = 0; j < sl.lt.n; ++j) k += (sl.lt.pos[j].w >= xk && sl.lt.pos[j].w > 0.f) ? 0 : 1;
    k = k < kMaxLights - 1 ? k : kMaxLights - 1;
    const float4 p = sl.lt.pos[k];
    const float rho = sl.radius[k];
    f3 L = mk(p.x, p.y, p.z);
    if (rho > 0.f) {
        const float r1 = uniform01(hs, (1u << 29) + (uint32_t)seg, 0);
        const float r2 = uniform01(hs, (1u << 29) + (uint32_t)seg, 1);
        const float z = 1 - 2 * r1;                                   // [-1, 1), exact
        const float s = rt_sqrtf(1 - z * z);
        double sn, cs;
        rt_sincos_2pi(2 * 3.14159265358979323846 * (double)r2, sn, cs);
        const float x = (float)(cs * (double)s);
        const float y = (float)(sn * (double)s);
        L = mk(L.x + rho * x, L.y + rho * y, L.z + rho * z);
    }
    return L;
}
// A THIN LENS (rt_camera_set_lens; the rule: raytrace_hip.h "thin lens", the step: lens_ray in rt_shade.hip.h).  The camera ray is built in one place, the opening launch of a
// chain: with the lens on that launch is wf_advance<kFormFirst | kFormLens> (LENS, always FIRST), which takes the lens by value; every later launch of the chain is whichever kernel the scene
// picks without a lens.  rtk::Scene and rtk::Frame do not grow.
struct WfLens { float radius, focus; };
// ROUGH MIRRORS (rt_material_set_roughness; the rule: raytrace_hip.h "roughness", the step: gloss_step in rt_shade.hip.h).  The table is a kernel argument of the four
// forms that read it (kFormGloss) and of no other kernel; the one per-lane read is alpha[] with the hit object's id, from the argument segment, as WfSoftLights::radius[k].
struct WfGloss {
    unsigned int mask;                       // bit k: the object at position k has an EFFECTIVE roughness (alpha > 0 and mirror != 0: formed on the host)
    float alpha[kMaxObjects];                // the roughness by object id; read only where the bit is set
};
// TINTED MIRRORS AND GLASS (rt_material_set_tint; the rule: raytrace_hip.h "tint").  The path's throughput is the fold: a specular hit of segment d on an effectively
// tinted object writes SID[d] = its object id and LS[d] = +0 where any other specular hit writes SID[d] = 0xff, and the fold -- which does not change -- then takes the
// segment for a diffuse one of direct term +0: fl(fl(fl(0 alb) / pi) + fl(alb ans)) = fl(alb ans) per channel, the object's albedo as a tint.  No shadow ray leaves the
// segment and none is taken to have left it: the launch that closes segment d's shadow ray asks the path's flag word (PF_HASX, set at emission where emitX is), never SID.
// The mask is a kernel argument of the four forms that read it (kFormTint, always with kFormGloss) and of no other kernel.
struct WfTint {
    unsigned int mask;                       // bit k: the object at position k is EFFECTIVELY tinted (flagged and mirror != 0 or n_in != n_out: formed on the host)
};
// THE SHUTTER (rt_scene_set_shutter; the rule: raytrace_hip.h "shutter", the step: shutter_time / shutter_pose in rt_shade.hip.h).  Over the exposure the light travels dL and
// sphere k travels its displacement; a path sees the scene at ONE time tau, drawn from its sample's key, and every launch of its chain -- the SHUTTER forms, kFormShutter --
// draws tau again and forms the light and the centres at that time where the Scene's would be read: the close of a shadow ray, the sphere normal, the shadow direction and
// the direct term, the sphere tests at emission.  R2 and the materials do not move; meshes do not move.  The table is a kernel argument of the four forms that read it.
// (BatchFrame's hazard -- an argument array indexed per lane goes to scratch -- is met as WfLights::pos[k] meets it: the loop over the spheres reads sph[] with a wave-uniform
// index; the one per-lane read is obj[] with the hit object's id.)
struct WfShutter {
    float4 light;                            // dL (w unused)
    float4 sph[kMaxSpheres];                 // the displacement of sphere k, in the order of Scene::sph
    float4 obj[kMaxSpheres];                 // the same displacements by OBJECT id (a mesh's entry is 0), for the normal
};
__device__ __forceinline__ f3 wf_xyz(float4 v) { return mk(v.x, v.y, v.z); }
// THE CHAIN'S CLOSE (wf_advance<kFormClose>: CLOSE; the plain chain only, rt_still.h still_plan).  The chain's last launch, at position segs, meets no continuation ray: it closes
// the shadow rays of segment segs - 1 and folds -- the close of a continuation ray, the shading and the emission are compiled out, and so is the dead half-record of a
// finished path (see the fold).  (Folding a path a launch early, in the last shading launch, where its shadow ray is not handed to the traversal, was built beside it
// and lost: DESIGN.md section 11.)
// THE FORM (rt_still.h kForm*): one word says which of the above a launch compiles in, and the kernel's extra arguments follow from it -- after (sc, fr, st) a kernel takes,
// in this order, the TexScene (kFormTex), the AnimFrame table (kFormAnim), the WfList (kFormList), the WfShade (kFormFill, kFormResume), the WfLights (kFormLights) or the
// WfSoftLights (kFormSoft), the WfLens (kFormLens), the WfShutter (kFormShutter), the WfSky (kFormSky), each only if its bit is set.  The path takes all nine; what a form
// does not take it never reads (the kernel below passes an empty one or null).
// THE ENVIRONMENT (rt_scene_set_environment; the rule: raytrace_hip.h "environment", the lookup: sky_radiance in rt_shade.hip.h).  A miss is seen in one place, the close of
// a continuation ray; a path that misses emits nothing more and folds in the same launch, so the radiance it met lives in registers from the miss to the fold, which
// starts from it instead of from black (SKY: the later launches' forms kFormSky, with and without textures and the soft lights' table).  No path state grows.
using AnimTable = const AnimFrame *__restrict__;                      // (the qualifier is part of the kernel's parameter type: without it the loads of wf_advance<kFormTex | kFormAnim> come in another order)
template <unsigned FORM>
__device__ __forceinline__ void wf_advance_path(const Scene &sc, const Frame &fr, const WfState &st, const int i, Work &wk, const TexScene &ts, const AnimFrame *__restrict__ anim,
                                                const WfList &list, const WfShade &sh, const WfLights *__restrict__ lt, const WfSoftLights *__restrict__ sl, const WfLens *__restrict__ ln,
                                                const WfShutter *__restrict__ shu, const WfSky *__restrict__ sky, const WfSkyDist *__restrict__ sd = nullptr,
                                                const WfEmit *__restrict__ em = nullptr, const WfFresnel *__restrict__ fz = nullptr,
                                                const WfGloss *__restrict__ gz = nullptr, const WfTint *__restrict__ tz = nullptr) {
    constexpr bool STATS = FORM & kFormStats, FIRST = FORM & kFormFirst, TEX = FORM & kFormTex, ANIM = FORM & kFormAnim, LIST = FORM & kFormList;
    constexpr bool FILL = FORM & kFormFill, RESUME = FORM & kFormResume, LENS = FORM & kFormLens, CLOSE = FORM & kFormClose, SHUTTER = FORM & kFormShutter, SKY = FORM & kFormSky;
    constexpr bool SAMPLE = FORM & kFormSkySample;                     // sky sampling: a segment's one shadow ray may go to the environment (always with SKY and the soft lights' table)
    // emissive meshes: a continuation ray that hits an emitter ends its path there, and a segment's one shadow ray may go to a point of one (always with the soft lights'
    // table, never with SKY)
    constexpr bool EMIT = FORM & kFormEmit;
    // Fresnel dielectrics: a continuation ray that hits an effectively flagged object is reflected or refracted, one draw (fresnel_step beside refract_step; never with
    // SKY, SHUTTER or EMIT, and in the later launches of a chain alone)
    constexpr bool FRESNEL = FORM & kFormFresnel;
    // rough mirrors: a continuation ray that hits a mirror with an effective roughness is reflected about a facet, two draws (gloss_step beside mirror_step; never with
    // SKY, SHUTTER, EMIT or FRESNEL, and in the later launches of a chain alone)
    constexpr bool GLOSS = FORM & kFormGloss;
    // tinted mirrors and glass: a specular hit of an effectively tinted object is recorded as a segment of the object's albedo and direct term +0 (always with GLOSS,
    // whose mask may be empty; never with SKY, SHUTTER, EMIT or FRESNEL, and in the later launches of a chain alone)
    constexpr bool TINT = FORM & kFormTint;
    constexpr int LIGHTS = (FORM & kFormSoft) ? 2 : (FORM & kFormLights) ? 1 : 0;
    constexpr bool DEAD_LAST = (FORM & ~kFormStats) == 0u;             // the plain later launch and its counting twin: the one form with the dead-last rule (kPolDeadLast)
    // The plain chain's later launches (form 0, the closing kernel, their counting twins) ask for a path's words in ROUNDS, not one dependent load after the other: the Y
    // record whole, then -- the flag word known -- the mesh words and the dead-channel byte together, and the shadow ray is formed again from the Y record and the light
    // instead of being read back.  Every other form keeps the order it had.
    constexpr bool PLAIN = (FORM & ~(kFormStats | kFormClose)) == 0u;
    // the stream policy's store in the fold (kPolPixels), in every form but the textured animated batch's: at 64 registers that kernel has no room for the second form
    // of the store (16 bytes of scratch) and keeps the plain one
    constexpr bool POL_PIXELS = !(TEX && ANIM);
    const float4 kDead = make_float4(0, 0, 0, 0);                     // second half of a queue record without a ray (and, in a Y slot, without a path)
    const int rx = st.n_paths + i;                                    // ray index of this path's shadow ray
    const int qy = wf_ray_to_slot(st, i), qx = wf_ray_to_slot(st, rx);
    const float4 y1 = (FIRST || RESUME) ? kDead : st.QR[2 * (size_t)qy + 1];      // (u.y, u.z, flag word, t of the nearest sphere) of the continuation ray in flight
    // (PLAIN) the other half of the Y record's sector, asked for in the same round: behind the return below the compiler may not issue it until y1 is back
    float4 y0 = kDead;
    if constexpr (PLAIN && !CLOSE) y0 = st.QR[2 * (size_t)qy];
    const int F = __float_as_int(y1.z);
    if (!FIRST && !RESUME && !(F & PF_ALIVE)) {                                  // finished (or padding): its queue flags are already 0
        if (st.x0 == 1 && !st.m0 && i < st.n_px) st.X0[i] = WF_NOHIT;  // (first-shadow fill: no word of a filled part is stale)
        return;
    }
    f3 L = mk(sc.Lx, sc.Ly, sc.Lz);
    int refr_code = (FIRST || RESUME) ? 0 : (F >> PQ_REFR_SHIFT) & 63;            // Ray::refraction_index = 1 (cpu:100)
    int d = 0, nrays = 0;
    bool emitY = false, emitX = false, finished = false;
    float x_bound = -__builtin_inff();                                // any-hit bound of the shadow ray (wf_anyhit_bound)
    bool x_sky = false;                                               // (SAMPLE) the shadow ray in question -- closed, then emitted -- goes to the sky
    bool x_moot = false;                                              // the shadow ray's answer cannot reach the pixel (direct term +0 either way, or every channel dead)
    bool y_dead = false;                                              // (DEAD_LAST) the bounce ray leaves a diffuse segment after which every channel of the path is dead
    f3 Oy = mk(0, 0, 0), uy = mk(0, 0, 1), Ox = mk(0, 0, 0), ux = mk(0, 0, 1);
    f3 E = mk(0, 0, 0);                                               // (SKY) what the path's last ray met beyond the scene, (EMIT) the radiance of the emitter it hit: the fold starts from it
    int px, lrow; bool valid;
    int s_rel = 0;
    if (st.n_paths != st.n_px) s_rel = wf_div(i, st.n_px, st.n_px_m);
    // (PLAIN) the round behind the flag word: the continuation ray's mesh word, the shadow ray's (from where x_close0 and x0 below say) and the dead-channel byte, each only
    // for the path that consumes it, none consumed before all are asked for.  (CLOSE) the fold's SID and LS words ride in the same round: their addresses need i and the
    // segment alone.  kFoldRound segments, back to front from the last one, are held in registers; a longer chain folds the rest as it always did.
    constexpr int kFoldRound = 3;
    unsigned long long pre_ym = WF_NOHIT, pre_xm = WF_NOHIT;
    int pre_dch = 0;
    int pre_sid[kFoldRound];
    float pre_ls[kFoldRound];
    if constexpr (PLAIN) {
        if (!CLOSE && (F & (PF_HASY | PF_MESHY)) == (PF_HASY | PF_MESHY)) pre_ym = st.M[st.m0 ? i - s_rel * st.n_px : i];
        if ((F & (PF_HASX | PQ_XSPHERE | PF_MESHX)) == (PF_HASX | PF_MESHX)) {   // the condition under which wf_x_shadowed asks for the word
            const int first = s_rel * st.n_px;
            pre_xm = !(st.x0 != 0 && !st.m0) ? st.M[rx] : st.x0 == 2 ? st.X0[i - first] : st.M[rx - first];
        }
        if (!CLOSE && st.deadch) pre_dch = st.DCH[i];
        if constexpr (CLOSE) {
            const int dF = (F >> PF_DEPTH_SHIFT) & PF_DEPTH_MASK;
            const int nsegF = dF < fr.segs ? dF : fr.segs;
#pragma unroll
            for (int j = 0; j < kFoldRound; ++j) {
                const int k = nsegF - 1 - j;
                pre_sid[j] = 0xff; pre_ls[j] = 0.f;
                if (k >= 0) { pre_sid[j] = st.SID[(size_t)k * st.n_paths + i]; pre_ls[j] = st.LS[(size_t)k * st.n_paths + i]; }
            }
        }
    }
    // a batch: item i belongs to frame s_rel (a wave's 64 items share it: n_px is a multiple of 64), whose camera, seed and output replace the launch's -- from scalar registers
    float camx = sc.camx, camy = sc.camy, camz = sc.camz, fr_z = fr.z;
    uint32_t fr_seed = fr.seed;
    float4 *fr_out = fr.out;
    int samp = st.samp0 + s_rel;
    bool in_batch = true;
    int af_k = 0;                                                     // (ANIM) this wave's frame in the table
    if (st.n_batch > 0) {
        const int f = __builtin_amdgcn_readfirstlane(s_rel);
        in_batch = f < st.n_batch;
        const BatchFrame b = st.batch[f & (kMaxBatch - 1)];             // wave-uniform address: scalar loads
        camx = b.camx; camy = b.camy; camz = b.camz;
        fr_z = b.z; fr_seed = b.seed; fr_out = b.out;
        samp = 0;
        if (ANIM) af_k = f & (kMaxBatch - 1);
    }
    const AnimFrame *const af = ANIM ? anim + af_k : nullptr;         // wave-uniform
    float intensity = sc.intensity;
    if (ANIM) { L = mk(af->Lx, af->Ly, af->Lz); intensity = af->intensity; }
    wf_decode(st, fr, i - s_rel * st.n_px, px, lrow, valid);
    valid = valid && samp < fr.spp && in_batch;                       // the last chain of a frame may be short of samples
    if (LIST) {                                                       // the item's record instead (a list chain has n_px == n_paths: s_rel is 0); its last wave may end in padding
        const unsigned int rec = i < list.n ? list.items[i] : 0u;
        samp = (int)(rec & 63u);
        wf_decode(st, fr, (int)(rec >> 6), px, lrow, valid);
        valid = valid && i < list.n;
    }
    const int row = image_row(fr, lrow);
    float tau = 0.f;                                                  // (SHUTTER) the path's time, and the light where it is then
    if constexpr (SHUTTER) {
        tau = shutter_time(sample_hash(pixel_hash(fr, row, px, fr_seed), samp));
        L = shutter_pose(L, wf_xyz(shu->light), tau);
    }
    // (FILL) what the slot's record holds, gathered while segment 0 is shaded; (RESUME) the record
    f3 shO = mk(0, 0, 0), shV = mk(0, 0, 1);
    float sh_l = 0.f;
    int sh_kind = kShadeMiss, sh_sid = 0xff, sh_dch = 0, sh_rays = 0;
    float4 ra = kDead, rb = kDead;
    if (RESUME) {
        if (!valid) { st.QR[2 * (size_t)qy + 1] = kDead; return; }       // as wf_advance<kFormFirst> leaves a pixel slot outside the frame
        if (sh.kill_x) st.QR[2 * (size_t)qx + 1] = kDead;
        // (a chain that traces several samples as items reads a slot's record once per sample in this one launch: not a use-once stream, the plain load)
        const bool nt_rec = (st.policy & kPolRecords) != 0 && st.n_paths == st.n_px;
        ra = pol_load(&sh.rec[2 * (size_t)(i - s_rel * st.n_px)], nt_rec); rb = pol_load(&sh.rec[2 * (size_t)(i - s_rel * st.n_px) + 1], nt_rec);
    }

    if (FIRST) {
        if (!valid) { st.QR[2 * (size_t)qy + 1] = kDead; return; }       // (the X slot of a pixel outside the frame is never written: zero from the layout's memset)
        if (st.deadch) st.DCH[i] = 0;                                  // no channel of the new path is dead
        if (fr.segs <= 0) {
            finished = true;                                          // optimized.cu convention with num_bounce 0: black
        } else {
            Oy = mk(camx, camy, camz);
            uy = camera_dir(fr, Oy, fr_z, px, row, sample_hash(pixel_hash(fr, row, px, fr_seed), samp));
            if (LENS) lens_ray(fr, ln->radius, ln->focus, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), Oy, uy);   // from a point of the lens through the pinhole ray's point of focus
            emitY = true;                                             // continuation ray of segment 0
            nrays = 1;
        }
    } else {
        ADV_MARK("closex_begin");
        d = (F >> PF_DEPTH_SHIFT) & PF_DEPTH_MASK;                    // segment of the continuation ray in flight
        nrays = (F >> PF_RAYS_SHIFT) & PF_RAYS_MASK;
        if (RESUME) {                                                 // segment 0 is shaded and its shadow ray decided: the record's state
            const int rw = __float_as_int(rb.w);
            sh_kind = rw & 3;
            nrays = (int)((unsigned)rw >> SH_RAYS_SHIFT);
            refr_code = (rw >> SH_REFR_SHIFT) & 63;
            if (st.deadch) st.DCH[i] = (unsigned char)((rw >> SH_DCH_SHIFT) & 15);
        }
        // ---- (1) the shadow ray of segment d-1's hit came back: direct light or not (light_hidden) ----
        // cpu:615 compares |P' - P_adj|^2, P' = P_adj + t_min u, with |L - P_adj|^2; it is monotone in t_min (every rounding involved is),
        // so it holds iff it holds for the nearest sphere (decided when the ray was emitted: PF_XSPHERE) or for the nearest triangle
        // first-shadow cache: in the launch that closes segment 0's shadow rays the word comes from the cache (read), or from the ray of the first sample's item of this pixel
        // slot (fill: the ray every sample of the slot shares -- not from X0, which this launch writes).  Some accepted hit of the same ray decides as the nearest does.
        const bool x_close0 = st.x0 != 0 && !st.m0;
        unsigned long long xm = WF_NOHIT;
        if (LIGHTS == 1 && (F & PF_HASX)) L = wf_light_pick(*lt, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d - 1);   // the light segment d-1's shadow ray went to, picked again
        // (SAMPLE) segment d-1's shadow ray went to the sky: known from its share draw alone, no search
        if constexpr (SAMPLE) x_sky = (F & PF_HASX) && uniform01(sample_hash(pixel_hash(fr, row, px, fr_seed), samp), (uint32_t)d, 3) <= sd->s;
        if constexpr (!EMIT)                                          // (EMIT: the far end of the ray travels with its term, no second draw)
        if (LIGHTS == 2 && (F & PF_HASX) && !(SAMPLE && x_sky)) L = wf_light_point(*sl, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d - 1);   // ... and the point of its shell
        if constexpr (SAMPLE) {                                       // the stored three-channel term does not count if the ray was blocked: a sky ray by anything at all
            if (F & PF_HASX) {
                bool shadowed;
                if (x_sky) shadowed = (F & PQ_XSPHERE) != 0 || ((F & PF_MESHX) != 0 && st.M[rx] != WF_NOHIT);
                else shadowed = wf_x_shadowed(F, L, [&] { return st.M[rx]; }, [&](f3 &Oxr, f3 &uxr) {
                    const float4 x0 = st.QR[2 * (size_t)qx], x1 = st.QR[2 * (size_t)qx + 1];
                    Oxr = mk(x0.x, x0.y, x0.z); uxr = mk(x0.w, x1.x, x1.y);
                }, xm);
                if (shadowed) sd->L3[(size_t)(d - 1) * st.n_paths + i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else if constexpr (EMIT) {                                  // ... to a light or to an emitter: the far end travels with the term, no second draw
            if (F & PF_HASX) {
                bool shadowed = (F & PQ_XSPHERE) != 0;
                float4 l4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!shadowed && (F & PF_MESHX)) {
                    const unsigned long long m = st.M[rx];
                    if (m != WF_NOHIT) {
                        const float4 x0 = st.QR[2 * (size_t)qx], x1 = st.QR[2 * (size_t)qx + 1];
                        l4 = em->L3[(size_t)(d - 1) * st.n_paths + i];
                        shadowed = light_hidden_far2(mk(x0.x, x0.y, x0.z), mk(x0.w, x1.x, x1.y), __uint_as_float((unsigned int)(m >> 32)), l4.w);
                    }
                }
                if (shadowed) em->L3[(size_t)(d - 1) * st.n_paths + i] = make_float4(0.f, 0.f, 0.f, l4.w);
            }
        } else if constexpr (PLAIN) {
            // The word is in flight since the round behind the flags.  The ray: in these forms a shadow ray leaves a diffuse hit alone, from the point the continuation
            // ray leaves (Ox == Oy == P_adjusted), towards the Scene's light: the origin is the Y record's first half -- which the launch that shades the chain's last
            // segment stores for this purpose, where no continuation ray leaves -- and the direction is shadow_dir of the operands the emission gave it, the same
            // function on the same 32-bit words.  One route keeps the read-back: a chain of ONE segment whose shadow rays the launch that stores the first-shade
            // records emitted (x_close0 at the last position): that form leaves the default origin in the Y record.
            if (F & PF_HASX) {
                const bool x_readback = x_close0 && fr.segs == 1;
                const bool shadowed = wf_x_shadowed(F, L, [&] { return pre_xm; }, [&](f3 &Oxr, f3 &uxr) {
                    if (x_readback) {
                        const float4 x0 = st.QR[2 * (size_t)qx], x1 = st.QR[2 * (size_t)qx + 1];
                        Oxr = mk(x0.x, x0.y, x0.z); uxr = mk(x0.w, x1.x, x1.y);
                    } else {
                        if constexpr (CLOSE) y0 = st.QR[2 * (size_t)qy];
                        float nl;
                        Oxr = mk(y0.x, y0.y, y0.z); uxr = shadow_dir(L, Oxr, nl);
                    }
                }, xm);
                if (shadowed) {
                    st.LS[(size_t)(d - 1) * st.n_paths + i] = 0.f;
                    if constexpr (CLOSE) if (d <= fr.segs) pre_ls[0] = 0.f;       // segment d - 1 is the first the fold takes: the word held for it
                }
            }
        } else
        if (!RESUME && (F & PF_HASX)) {
            const bool shadowed = wf_x_shadowed(F, L, [&] {
                const int first = s_rel * st.n_px;                    // (0 unless the chain traces several samples as items)
                return !x_close0 ? st.M[rx] : st.x0 == 2 ? st.X0[i - first] : st.M[rx - first];
            }, [&](f3 &Oxr, f3 &uxr) {
                const float4 x0 = st.QR[2 * (size_t)qx], x1 = st.QR[2 * (size_t)qx + 1];
                Oxr = mk(x0.x, x0.y, x0.z); uxr = mk(x0.w, x1.x, x1.y);
            }, xm);
            if (shadowed) st.LS[(size_t)(d - 1) * st.n_paths + i] = 0.f;               // the l stored when the segment was shaded does not count
        }
        if (!RESUME && x_close0 && st.x0 == 1 && s_rel == 0) st.X0[i] = xm;      // fill: every first-sample path, WF_NOHIT where no shadow ray of its went through the mesh
        ADV_MARK("closex_end");
        // ---- (2) the continuation ray of segment d came back: Scene::getColor's branch for its hit ----
        if (!CLOSE && (RESUME || (F & PF_HASY))) {                    // (CLOSE: no continuation ray reaches the chain's last launch)
            ADV_MARK("closey_begin");
            const float4 r0 = RESUME ? ra : PLAIN ? y0 : st.QR[2 * (size_t)qy];
            f3 O = mk(r0.x, r0.y, r0.z), u = RESUME ? mk(ra.w, rb.x, rb.y) : mk(r0.w, y1.x, y1.y);   // (RESUME: the continuation ray of a specular hit; P_adjusted and N of a diffuse one)
            int sid = 0xff;                                           // object id if the hit is diffuse
            // Scene::intersect_all's running minimum (strict '<' in object order, cpu:554) = the lexicographic minimum over (t, position in Scene::objects):
            // the spheres' own winner was decided at emission (spheres_near2), the meshes' by the traversal; between the two a tie goes to the earlier object
            float t_min = y1.w;
            int win = ((F >> PQ_WIN_SHIFT) & 31) - 1, tri_win = -1;
            if (RESUME) win = sh_kind == kShadeMiss ? -1 : 0;         // (which object: the record's SID says, to the fold)
            if (!RESUME && (F & PF_MESHY)) {
                const unsigned long long m = PLAIN ? pre_ym : st.M[st.m0 ? i - s_rel * st.n_px : i];   // (m0: the camera ray's result, kept per pixel slot)
                if (m != WF_NOHIT) {
                    const float tm = __uint_as_float((unsigned int)(m >> 32));
                    const int mobj = mesh_obj_of_tri(sc, (int)(unsigned int)m);   // the meshes' own winner: minimum over (t, object position, scan rank) by the order the triangles are stored in
                    if (mesh_beats_sphere(t_min, win, tm, mobj)) { t_min = tm; win = mobj; tri_win = (int)(unsigned int)m; }   // a tie goes to whichever comes first in Scene::objects (no sphere: win = -1, 1e9 > tm)
                }
            }
            if constexpr (EMIT) {
                // The nearest object emits: the path ends here, as at a miss (no shadow ray, no continuation ray, SID 0xff), and the fold starts from the emitter's
                // radiance -- unless the ray left a diffuse segment while emitters are sampled: that segment's shadow rays have accounted for them (the rule of sky
                // sampling's miss)
                if (win >= 0 && ((em->mask >> win) & 1u) != 0) {
                    if (d == 0 || !(em->s > 0.f) || st.SID[(size_t)(d - 1) * st.n_paths + i] == 0xff) {
                        const float4 le = em->le[win];
                        E = mk(le.x, le.y, le.z);
                    }
                    win = -1;
                }
            }
            if (win >= 0) {                                           // a miss emits nothing: black (cpu:571), or under an environment E below
                const f3 P = O + t_min * u;                           // cpu:560
                Bary bary{0.f, 0.f, 0.f};                             // (TEX) the smooth normal's barycentrics, shared with the texture lookup
                bool have_bary = false;
                f3 N;
                Material m_plain{};
                if (RESUME) N = u;
                else if (ANIM && tri_win < 0) { const float4 c = af->ctr[win]; N = normalize(P - mk(c.x, c.y, c.z)); }   // sphere_normal (cpu:524-525) about this frame's centre
                else if (SHUTTER && tri_win < 0) N = normalize(P - shutter_pose(sphere_centre_of(sc, win), wf_xyz(shu->obj[win]), tau));   // ... about the centre at the path's time
                else if constexpr (PLAIN) {
                    // The hit object's three records in ONE round, asked for before the triangle's: left to itself the compiler moves each load into the branch that
                    // reads it -- the centre, then the mirror flag of the same record, then the indices, then the albedo: four dependent trips for a wall.  The empty
                    // statement below reads every word where the normal is done, so all are in flight together (it has no instruction of its own).
                    const float4 oa = sc.obj_a[win], ob = sc.obj_b[win];
                    const float2 on = sc.obj_n[win];
                    N = tri_win >= 0 ? hit_normal(sc, win, tri_win, O, u, P, bary, have_bary) : normalize(P - sphere_centre_from(oa));   // (sphere_normal on the words of its record)
                    asm volatile("" :: "v"(oa.w), "v"(ob.x), "v"(ob.y), "v"(ob.z), "v"(on.x), "v"(on.y));
                    m_plain = material_from(oa, ob, on);
                }
                else N = hit_normal(sc, win, tri_win, O, u, P, bary, have_bary);
                const Material m = PLAIN ? m_plain : material_of(sc, win);
                ADV_MARK("closey_end");
                bool cont = false;                                    // a continuation ray of segment d+1 was built in (O,u)
                bool fresnel_hit = false;                             // (FRESNEL) the object is effectively flagged: glass that reflects or refracts, chosen by one draw
                if constexpr (FRESNEL) fresnel_hit = ((fz->mask >> win) & 1u) != 0;
                bool gloss_hit = false;                               // (GLOSS) the object is a mirror with an effective roughness
                if constexpr (GLOSS) gloss_hit = ((gz->mask >> win) & 1u) != 0;
                if (gloss_hit) {
                    if constexpr (GLOSS) {                            // the mirror branch below with gloss_step in mirror_step's place
                        gloss_step(fr.eps, gz->alpha[win], P, N, O, u, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d);
                        cont = true;
                    }
                } else if (!RESUME && m.mirror) {
                    mirror_step(fr.eps, P, N, O, u);
                    cont = true;
                } else if (fresnel_hit) {
                    if constexpr (FRESNEL) {                          // the refraction branch below with fresnel_step in refract_step's place
                        float refr = 1.f;
                        if (refr_code != 0) { const Material mr = material_of(sc, (refr_code >> 1) - 1); refr = (refr_code & 1) ? mr.n_out : mr.n_in; }
                        const Refraction r = fresnel_step(m, refr, fr.eps, P, N, O, u, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d).r;
                        if (r.crossed) refr_code = (win + 1) << 1 | (r.out2in ? 0 : 1);
                        cont = true;
                    }
                } else if (RESUME && sh_kind == kShadeSpecular) {     // the record's ray (O, u) and refr_code are the continuation's
                    cont = true;
                } else if (!RESUME && m.n_in != m.n_out) {
                    float refr = 1.f;                                 // the ray's index: 1, or the n_in / n_out of the surface it last crossed
                    if (refr_code != 0) { const Material mr = material_of(sc, (refr_code >> 1) - 1); refr = (refr_code & 1) ? mr.n_out : mr.n_in; }
                    const Refraction r = refract_step(m, refr, fr.eps, P, N, O, u);
                    if (r.crossed) refr_code = (win + 1) << 1 | (r.out2in ? 0 : 1);    // refr = out2in ? m.n_in : m.n_out
                    cont = true;
                } else {                                              // diffuse
                    ADV_MARK("diffuse_begin");
                    const f3 Pa = RESUME ? O : P + fr.eps * N;
                    if (RESUME) {
                        st.LS[i] = rb.z;                              // final: no shadow ray of segment 0 is in flight
                        sid = (__float_as_int(rb.w) >> SH_SID_SHIFT) & 255;
                    } else if constexpr (SAMPLE) {
                        const uint32_t hs = sample_hash(pixel_hash(fr, row, px, fr_seed), samp);
                        x_sky = uniform01(hs, (uint32_t)(d + 1), 3) <= sd->s;   // this segment's one shadow ray goes to the sky, or to the light the list picks
                        f3 l3;
                        Ox = Pa;
                        if (x_sky) {
                            const SkyDraw dr = sky_draw(*sd, hs, d);
                            ux = dr.w;
                            x_bound = __builtin_inff();               // no far end: the first accepted triangle ends it
                            const float dn = dot(N, dr.w);
                            const float g = sky_weight(*sd, dr.t, dr.m, dr.r, (dn < 0.f) ? 0.f : dn);
                            const f3 Es = sky_radiance(*sky, dr.w);
                            l3 = mk(sd->w_sky * (g * Es.x), sd->w_sky * (g * Es.y), sd->w_sky * (g * Es.z));
                        } else {
                            float nl;
                            L = wf_light_point(*sl, hs, d);
                            ux = shadow_dir(L, Pa, nl);
                            x_bound = wf_anyhit_bound(Pa, nl);
                            const float lv = direct_term(sl->lt.total, L, P, N) * sd->w_light;
                            l3 = mk(lv, lv, lv);
                        }
                        nrays += 1;
                        sd->L3[(size_t)d * st.n_paths + i] = make_float4(l3.x, l3.y, l3.z, 0.f);
                        emitX = true;
                        x_moot = st.anyhit && (__float_as_uint(l3.x) | __float_as_uint(l3.y) | __float_as_uint(l3.z)) == 0u;
                        sid = win;
                        f3 alb = mk(m.ar, m.ag, m.ab);
                        if (TEX && tri_win >= 0 && ((ts.mask >> win) & 1)) {
                            if (!have_bary) bary = tri_bary(sc, tri_win, O, u);
                            float2 uv;
                            alb = tex_albedo(sc, ts, win, tri_win, bary, uv);
                            ts.ALB[(size_t)d * st.n_paths + i] = make_float4(alb.x, alb.y, alb.z, 0.f);
                            sid = kSidTextured;
                        }
                        // the dead channels: the guard's argument is about a scalar term in [+0, 2^96) -- a light's weighted term is one; a segment whose ray goes to the
                        // sky clears the mask, as a segment that fails the guard does
                        if (st.deadch) {
                            const int was = st.DCH[i];
                            int now = (was & 8) | (x_sky ? 0 : wf_dead_channels(was & 7, alb, l3.x));
                            if ((now & 7) == 7 && !x_moot) { x_moot = true; now |= 8; }
                            if (now != was) st.DCH[i] = (unsigned char)now;
                        }
                    } else if constexpr (EMIT) {
                        const uint32_t hs = sample_hash(pixel_hash(fr, row, px, fr_seed), samp);
                        const bool x_emit = uniform01(hs, (uint32_t)(d + 1), 3) <= em->s;   // this segment's one shadow ray goes to an emitter, or to the light the list picks
                        f3 l3;
                        if (x_emit) {
                            const EmitDraw dr = emit_draw(*em, sc.tri, hs, d);
                            const f3 v = dr.Q - P;
                            const float d2 = norm2(v);
                            const f3 wl = normalize(v);
                            const float dn = dot(N, wl);
                            const float g = emit_weight(*em, dr, wl, d2, (dn < 0.f) ? 0.f : dn);
                            const float4 le = em->le[mesh_obj_of_tri(sc, (int)dr.t)];
                            l3 = mk(em->w_emit * (g * le.x), em->w_emit * (g * le.y), em->w_emit * (g * le.z));
                            L = dr.Q + kEmitKappa * (Pa - dr.Q);      // short of the emitter's own plane
                        } else {
                            L = wf_light_point(*sl, hs, d);
                            const float lv = direct_term(sl->lt.total, L, P, N) * em->w_light;
                            l3 = mk(lv, lv, lv);
                        }
                        float nl;
                        Ox = Pa; ux = shadow_dir(L, Pa, nl);          // from here on a point light's shadow ray
                        x_bound = wf_anyhit_bound(Pa, nl);
                        nrays += 1;
                        em->L3[(size_t)d * st.n_paths + i] = make_float4(l3.x, l3.y, l3.z, norm2(L - Pa));
                        emitX = true;
                        x_moot = st.anyhit && (__float_as_uint(l3.x) | __float_as_uint(l3.y) | __float_as_uint(l3.z)) == 0u;
                        sid = win;
                        f3 alb = mk(m.ar, m.ag, m.ab);
                        if (TEX && tri_win >= 0 && ((ts.mask >> win) & 1)) {
                            if (!have_bary) bary = tri_bary(sc, tri_win, O, u);
                            float2 uv;
                            alb = tex_albedo(sc, ts, win, tri_win, bary, uv);
                            ts.ALB[(size_t)d * st.n_paths + i] = make_float4(alb.x, alb.y, alb.z, 0.f);
                            sid = kSidTextured;
                        }
                        // the dead channels, as under sky sampling: a segment whose ray goes to an emitter clears the mask, a light's weighted term is guarded as before
                        if (st.deadch) {
                            const int was = st.DCH[i];
                            int now = (was & 8) | (x_emit ? 0 : wf_dead_channels(was & 7, alb, l3.x));
                            if ((now & 7) == 7 && !x_moot) { x_moot = true; now |= 8; }
                            if (now != was) st.DCH[i] = (unsigned char)now;
                        }
                    } else {
                        float nl;
                        if (LIGHTS == 1) { L = wf_light_pick(*lt, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d); intensity = lt->total; }   // this segment's light, at the intensity of all
                        if (LIGHTS == 2) { L = wf_light_point(*sl, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d); intensity = sl->lt.total; }   // ... a point of its shell
                        Ox = Pa; ux = shadow_dir(L, Pa, nl);                // the shadow ray of segment d
                        if constexpr (PLAIN) Oy = Pa;                       // ... whose origin the launch that closes it takes from the Y record, continuation ray or none
                        x_bound = wf_anyhit_bound(Pa, nl);
                        nrays += 1;
                        // the segment's direct term if the light turns out to be visible; kept until the shadow ray is back
                        const float lvis = (ANIM || LIGHTS) ? direct_term(intensity, L, P, N) : direct_term(sc, L, P, N);
                        st.LS[(size_t)d * st.n_paths + i] = lvis;
                        // A surface that faces away from the light (mx = 0) has the direct term +0 whether the light is visible or not: shaded, cpu:616 stores the literal 0; lit,
                        // cpu:623 computes l = +0 -- the same 32 bits (a NaN or a -0 from a degenerate light is not +0 and keeps its ray).  The reference still calls intersect_all
                        // for it (the ray is counted), but nothing of its answer can reach the pixel: with any-hit on the ray is neither set up nor traced.  These are the shadow
                        // rays that start on the mesh's far side and run through its whole body: 4.7 % of a headline frame's traversal work.
                        // (The path still spends a launch on the ray -- PF_HASX without PF_MESHX, closed as a ray that missed the mesh -- so that it finishes in the launch it always
                        // finished in: folding a launch early costs the uniform kernel more than the traversal saves.)
                        emitX = true;
                        x_moot = st.anyhit && __float_as_uint(lvis) == 0u;
                        sid = win;
                        f3 alb = mk(m.ar, m.ag, m.ab);                    // the albedo the fold will use
                        if (TEX && tri_win >= 0 && ((ts.mask >> win) & 1)) {   // a textured mesh: this segment's albedo, evaluated once, for the fold
                            if (!have_bary) bary = tri_bary(sc, tri_win, O, u);
                            float2 uv;
                            alb = tex_albedo(sc, ts, win, tri_win, bary, uv);
                            ts.ALB[(size_t)d * st.n_paths + i] = make_float4(alb.x, alb.y, alb.z, 0.f);
                            sid = kSidTextured;
                        }
                        // Every channel dead, this segment's albedo counted: lvis or +0, the pixel is the same (wf_dead_channels) -- moot for a second reason
                        if (st.deadch) {
                            const int was = PLAIN ? pre_dch : st.DCH[i];
                            int now = (was & 8) | wf_dead_channels(was & 7, alb, lvis);
                            if ((now & 7) == 7 && !x_moot) {
                                x_moot = true;
                                now |= 8;
                                if (STATS) wk.dead_elided++;
                            }
                            if (now != was) st.DCH[i] = (unsigned char)now;
                            if (FILL) sh_dch = now;
                            if (DEAD_LAST) y_dead = (now & 7) == 7;
                        }
                        if (FILL) { shO = Pa; shV = N; sh_l = lvis; sh_kind = kShadeDiffuse; sh_sid = sid; }
                    }
                    ADV_MARK("diffuse_end");
                    if (d + 1 < fr.segs) {                            // the bounce ray: needs the sample's key and N only
                        ADV_MARK("bounce_begin");
                        u = cosine_bounce(N, sample_hash(pixel_hash(fr, row, px, fr_seed), samp), d);
                        O = Pa;
                        refr_code = 0;                                // Ray(P_adjusted, random_direction): index 1
                        cont = true;
                        ADV_MARK("bounce_end");
                    }
                }
                if constexpr (TINT) {
                    // The arm above was a specular one (the mask holds effective bits alone) and built the ray it always builds; no shadow ray leaves.  To the fold the
                    // segment is a diffuse one of this albedo and direct term +0, and so it is to the dead channels (the material table's albedo, textured or not)
                    if (((tz->mask >> win) & 1u) != 0) {
                        sid = win;
                        st.LS[(size_t)d * st.n_paths + i] = 0.f;
                        if (st.deadch) {
                            const int was = st.DCH[i];
                            const int now = (was & 8) | wf_dead_channels(was & 7, mk(m.ar, m.ag, m.ab), 0.f);
                            if (now != was) st.DCH[i] = (unsigned char)now;
                        }
                    }
                }
                if (FILL && sid == 0xff) { shO = O; shV = u; sh_kind = kShadeSpecular; }   // mirror or glass: the continuation ray
                if (FILL) sh_rays = nrays;
                if (cont && d + 1 < fr.segs) {
                    emitY = true; Oy = O; uy = u;                     // continuation ray of segment d+1
                    nrays += 1;
                }
            } else if constexpr (SKY) {
                // (SAMPLE) a ray that left a diffuse segment starts the fold from +0: that segment's shadow rays have accounted for the sky
                if (!SAMPLE || d == 0 || st.SID[(size_t)(d - 1) * st.n_paths + i] == 0xff)
                    E = sky_radiance(*sky, u);                        // the environment, in the direction the record holds
            }
            st.SID[(size_t)d * st.n_paths + i] = (unsigned char)sid;
            d = d + 1;
        }
        finished = !(emitX || emitY);
    }

    if (finished) {   // nothing in flight: fold the path back to front, accumulate the sample (cpu:711)
        ADV_MARK("fold_begin");
        if (FILL && s_rel == 0)                                       // no shadow ray left: a miss, or a specular hit of a one-segment path
            wf_shade_store(sh, i, sh_kind, shO, shV, 0.f, 0xff, sh_kind == kShadeSpecular ? refr_code : 0, 0, sh_kind == kShadeMiss ? nrays : sh_rays);
        f3 ans = (SKY || EMIT) ? E : mk(0, 0, 0);
        bool fold_sure = true;                                        // (counting instantiation) every folded segment passed wf_fold_bounded
        const int nseg = d < fr.segs ? d : fr.segs;
        if constexpr (PLAIN && CLOSE) {                               // the segments whose words the round behind the flags asked for, in the fold's order
            // ... and their albedos in one round as well (a segment without one asks for object 0's; the empty statement keeps the loads where they are written)
            f3 pre_alb[kFoldRound];
#pragma unroll
            for (int j = 0; j < kFoldRound; ++j) {
                const float4 b = sc.obj_b[pre_sid[j] != 0xff ? pre_sid[j] : 0];
                pre_alb[j] = mk(b.x, b.y, b.z);
            }
            static_assert(kFoldRound == 3, "the statement below names every albedo");
            asm volatile("" :: "v"(pre_alb[0].x), "v"(pre_alb[1].x), "v"(pre_alb[2].x));
#pragma unroll
            for (int j = 0; j < kFoldRound; ++j) {
                const int sid = pre_sid[j];                           // (0xff past the path's first segment)
                if (sid != 0xff) {
                    const f3 alb = pre_alb[j];
                    const float l = pre_ls[j];
                    ans = fold_segment(ans, l, alb);
                    if (STATS && !wf_fold_bounded(ans, l, alb)) fold_sure = false;
                }
            }
        }
        for (int k = nseg - 1 - ((PLAIN && CLOSE) ? kFoldRound : 0); k >= 0; --k) {
            const int sid = st.SID[(size_t)k * st.n_paths + i];
            if (sid != 0xff) {
                f3 alb;
                if (TEX && sid == kSidTextured) {                     // the albedo the segment stored when it was shaded
                    const float4 a = ts.ALB[(size_t)k * st.n_paths + i];
                    alb = mk(a.x, a.y, a.z);
                } else {
                    const Material m = material_of(sc, sid);
                    alb = mk(m.ar, m.ag, m.ab);
                }
                if constexpr (SAMPLE) {                               // the segment's three-channel term
                    const float4 l4 = sd->L3[(size_t)k * st.n_paths + i];
                    ans = fold_segment(ans, mk(l4.x, l4.y, l4.z), alb);
                } else if constexpr (EMIT) {
                    const float4 l4 = em->L3[(size_t)k * st.n_paths + i];
                    ans = fold_segment(ans, mk(l4.x, l4.y, l4.z), alb);
                } else {
                const float l = st.LS[(size_t)k * st.n_paths + i];
                ans = fold_segment(ans, l, alb);
                if (STATS && !wf_fold_bounded(ans, l, alb)) fold_sure = false;
                }
            }
        }
        if (STATS && !fold_sure && st.deadch && (st.DCH[i] & 8)) wk.dead_unsure++;   // a ray of this path was elided and its chain leaves what the elision was argued for
        if (st.samp_out != nullptr) {                                 // more than one sample per pixel: path_reduce (a list chain: sample_fold) sums in sample order
            st.samp_out[i] = make_float4(ans.x, ans.y, ans.z, (float)nrays);
        } else {                                                      // one sample: T = 0 + ans, out = T / n (cpu:711-713 + the framebuffer store)
            float4 t = make_float4(0, 0, 0, 0);
            if (fr.cam_mode == 1) { t.x += ans.x * fr.inv_n; t.y += ans.y * fr.inv_n; t.z += ans.z * fr.inv_n; }   // realtime:1131
            else { t.x += ans.x; t.y += ans.y; t.z += ans.z; }
            t.w += (float)nrays;
            const float n = fr.cam_mode == 1 ? 1.f : (float)fr.spp;
            pol_store(&fr_out[out_index(fr, lrow, px)], make_float4(t.x / n, t.y / n, t.z / n, t.w), POL_PIXELS && (st.policy & kPolPixels) != 0);
        }
        // The path is over; its X slot keeps a record of an older launch, which no later one takes for its own.  (CLOSE: the chain is over too, and the store is dropped.
        // Whatever the Y slot's second half holds then -- a flag word without PQ_TRAV, so no traversal launch takes it for a ray -- the next chain of this part of the queue
        // rewrites before any of its traversal launches runs, for EVERY item i < n_paths of its opening launch: wf_advance<kFormFirst> and its animated and lens forms store kDead
        // for an item that is not valid (outside the frame, past spp, past the batch), fold an item of a chain of no segments, which stores kDead, and store the record's
        // state for every other; wf_advance<kFormResume> stores kDead for an item that is not valid and folds or emits every other, never taking the early return of a path that
        // is not alive.  A chain of another layout starts behind the queue's zero fill (start_chains: q_sig); the list chains have a queue of their own.)
        if (!CLOSE) st.QR[2 * (size_t)qy + 1] = kDead;
        ADV_MARK("fold_end");
        return;
    }

    // ---- (3) emission: sphere tests (cpu:512-527), root-box test (cpu:279), queue records ----
    int flags = PF_ALIVE | (d << PF_DEPTH_SHIFT) | (nrays << PF_RAYS_SHIFT) | (refr_code << PQ_REFR_SHIFT) | (int)((unsigned)st.nonce << PQ_NONCE_SHIFT);
    SphereNear h, hx;
    ADV_MARK("spheres_begin");
    if (ANIM) spheres_near2(sc, af->sph, emitX ? Ox : Oy, uy, emitY, ux, emitX && !x_moot, h, hx);
    else if constexpr (SHUTTER)                                       // the spheres where they are at the path's time (k is wave-uniform: scalar loads)
        spheres_near2(sc.n_spheres, [&](int k) {
            const Sphere &s0 = sc.sph[k];
            const f3 c = shutter_pose(mk(s0.cx, s0.cy, s0.cz), wf_xyz(shu->sph[k]), tau);
            return Sphere{c.x, c.y, c.z, s0.R, s0.R2, s0.obj};
        }, emitX ? Ox : Oy, uy, emitY, ux, emitX && !x_moot, h, hx);
    else spheres_near2(sc, emitX ? Ox : Oy, uy, emitY, ux, emitX && !x_moot, h, hx);   // a shadow ray and a bounce ray leave the same point (Oy == Ox == P_adjusted)
    ADV_MARK("spheres_end");
    float t_sph = 0.f;
    if (emitX) {
        const float tS = hx.t;                                        // only the value of the shadow ray's nearest hit matters
        flags |= PF_HASX;
        if (!x_moot && ((SAMPLE && x_sky) ? hx.obj >= 0 : light_hidden(Ox, ux, tS, L))) flags |= PQ_XSPHERE;      // cpu:615 holds for the sphere already: whatever the mesh says, the segment is shaded (the comparison is monotone in t)
        // ... so with any-hit on that ray is not traced through the mesh at all (intersect_all does: a run that counts the reference's work has any-hit off)
        if (!x_moot && (!(flags & PQ_XSPHERE) || !st.anyhit) && wf_root_test<STATS>(sc, st, rx, Ox, ux, wk)) {   // only then does anybody read the record: the traversal, and this kernel if the mesh is hit
            flags |= PF_MESHX;
            if (STATS) wk.trav_x++;
            // first-shadow cache: the ray's answer is known (read) or is another item's (fill, a later sample) -- the record is written for the close, the traversal never fetches it
            const int x_trav = (st.x0 != 0 && st.m0 && (st.x0 == 2 || s_rel != 0)) ? 0 : PQ_TRAV;
            st.QR[2 * (size_t)qx] = make_float4(Ox.x, Ox.y, Ox.z, ux.x);
            st.QR[2 * (size_t)qx + 1] = make_float4(ux.y, ux.z, __int_as_float((int)((unsigned)(x_trav | (st.anyhit ? PQ_ANYHIT : 0) | (d << PF_DEPTH_SHIFT)) | (unsigned)st.nonce << PQ_NONCE_SHIFT)), x_bound);
        }
    }
    if (FILL && s_rel == 0) {                                         // the slot's record, with the shadow ray decided as the next launch's close decides it: from the cached word
        float l0 = sh_l;
        unsigned long long xw = WF_NOHIT;
        if (emitX && wf_x_shadowed(flags, L, [&] { return st.X0[i]; }, [&](f3 &Oxr, f3 &uxr) { Oxr = Ox; uxr = ux; }, xw)) l0 = 0.f;
        wf_shade_store(sh, i, sh_kind, shO, shV, l0, sh_sid, sh_kind == kShadeSpecular ? refr_code : 0, sh_dch, sh_rays);
    }
    if (emitY) {
        t_sph = h.t;
        flags |= PF_HASY | (((h.obj + 1) & 31) << PQ_WIN_SHIFT);
        // dead last: the chain's last continuation ray of a dead path that hits a sphere for certain (d is the emitted ray's segment; a chain of fewer than three
        // segments is left alone)
        bool dead_y = false;
        if constexpr (DEAD_LAST) dead_y = (st.policy & kPolDeadLast) != 0 && y_dead && d == fr.segs - 1 && fr.segs >= 3 && h.obj >= 0;
        if (!(dead_y && !STATS) && wf_root_test<STATS>(sc, st, i, Oy, uy, wk)) {
            flags |= PF_MESHY | PQ_TRAV;
            if (FIRST && st.m0 && s_rel != 0) flags &= ~PQ_TRAV;      // the same camera ray as the first sample's item of this pixel slot: closed from its word, never fetched by the traversal
            if (STATS) wk.trav_y++;
            if (STATS && dead_y) wk.dead_last++;                      // (the counting form) the rule takes this ray out of the traversal
        }
    }
    // whole sectors also when no continuation ray leaves.  (PLAIN) the half is read then as well: a shadow ray that leaves alone has its origin here (Oy = P_adjusted, set
    // in the diffuse branch), and the launch that closes it -- the closing kernel, or form 0 in its place -- takes it from this store instead of reading the X record back.
    // In the other forms nobody reads the half of a path without a continuation ray.
    st.QR[2 * (size_t)qy] = make_float4(Oy.x, Oy.y, Oy.z, uy.x);
    st.QR[2 * (size_t)qy + 1] = make_float4(emitY ? uy.y : 0.f, emitY ? uy.z : 0.f, __int_as_float(flags), t_sph);   // the path's state travels with its Y slot
}

// The one kernel.  Its extras are found by type: adv_extra_or the one of type T among them, or `none`; adv_extra its address, or null.  (The kernel itself hands them to the
// path, with nothing in between: through one more function the counting forms come out with two counters' registers swapped -- profiles/advance_forms.)
template <class T> __device__ __forceinline__ const T &adv_extra_or(const T &none) { return none; }
template <class T, class E, class... Rest> __device__ __forceinline__ const T &adv_extra_or(const T &none, const E &e, const Rest &... rest) {
    if constexpr (std::is_same_v<T, E>) return e; else return adv_extra_or(none, rest...);
}
template <class T> __device__ __forceinline__ const T *adv_extra() { return nullptr; }
template <class T, class E, class... Rest> __device__ __forceinline__ const T *adv_extra(const E &e, const Rest &... rest) {
    if constexpr (std::is_same_v<T, E>) return &e; else return adv_extra<T>(rest...);
}
template <class T, class... Extra> constexpr bool adv_takes = (std::is_same_v<T, Extra> || ...);
// Eight waves per SIMD (64 registers) for every form but one: in wf_advance<kFormTex | kFormSoft> the texture lookup's live values and a second binary64 sincos do not fit
// 64 registers together: 8 spilled.  Seven waves per SIMD, 72 registers, no scratch.
// The sampling forms carry the draw (a 64-bit search, a binary64 quotient) beside the soft lights' sincos: six waves per SIMD, 80 registers.
// The emission forms carry the same kind of draw.  soft | emit: at eight waves 4 scalar registers spill, at seven nothing does (60 registers); tex | soft | emit: 32 bytes of
// scratch at eight, 16 at seven, none at six (74 registers).
// The fresnel forms carry one draw and two quotients more than their counterparts.  fresnel and soft | fresnel: eight waves, 52 and 54 registers, nothing spills;
// tex | fresnel: at eight waves 2 scalar registers spill, at seven nothing does; tex | soft | fresnel: seven, as its counterpart.
// The gloss forms carry two draws, one quotient, two roots, the sincos and the tangent frame more than their counterparts (+ 385 vector instructions).  gloss and
// soft | gloss: eight waves, 52 and 54 registers, nothing spills; tex | gloss: at eight waves 2 scalar registers spill, at seven nothing does; tex | soft | gloss:
// seven, as its counterpart.
// The tint forms are the gloss forms with one mask test, two stores and the dead-channel byte's update more: the same waves as their counterparts.
constexpr int adv_waves(unsigned form) { return (form & kFormGloss) ? ((form & kFormTex) ? 7 : 8) : (form & kFormFresnel) ? ((form & kFormTex) ? 7 : 8) : (form & kFormEmit) ? ((form & kFormTex) ? 6 : 7) : (form & kFormSkySample) ? 6 : (form & kFormTex) && (form & kFormSoft) ? 7 : 8; }
template <unsigned FORM, class... Extra>
__global__ __launch_bounds__(256, adv_waves(FORM)) void wf_advance(const Scene sc, const Frame fr, const WfState st, const Extra... extra) {
    static_assert(adv_takes<TexScene, Extra...> == ((FORM & kFormTex) != 0) && adv_takes<AnimTable, Extra...> == ((FORM & kFormAnim) != 0) &&
                  adv_takes<WfList, Extra...> == ((FORM & kFormList) != 0) && adv_takes<WfShade, Extra...> == ((FORM & (kFormFill | kFormResume)) != 0) &&
                  adv_takes<WfLights, Extra...> == ((FORM & kFormLights) != 0) && adv_takes<WfSoftLights, Extra...> == ((FORM & kFormSoft) != 0) &&
                  adv_takes<WfLens, Extra...> == ((FORM & kFormLens) != 0) && adv_takes<WfShutter, Extra...> == ((FORM & kFormShutter) != 0) &&
                  adv_takes<WfSky, Extra...> == ((FORM & kFormSky) != 0) && adv_takes<WfSkyDist, Extra...> == ((FORM & kFormSkySample) != 0) &&
                  adv_takes<WfEmit, Extra...> == ((FORM & kFormEmit) != 0) && adv_takes<WfFresnel, Extra...> == ((FORM & kFormFresnel) != 0) &&
                  adv_takes<WfGloss, Extra...> == ((FORM & kFormGloss) != 0) && adv_takes<WfTint, Extra...> == ((FORM & kFormTint) != 0),
                  "a form's extras are the ones its bits name");
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    Work wk;
    if (i < st.n_paths)
        wf_advance_path<FORM>(sc, fr, st, i, wk, adv_extra_or(TexScene{}, extra...), adv_extra_or<AnimTable>(nullptr, extra...), adv_extra_or(WfList{}, extra...), adv_extra_or(WfShade{}, extra...),
                              adv_extra<WfLights>(extra...), adv_extra<WfSoftLights>(extra...), adv_extra<WfLens>(extra...), adv_extra<WfShutter>(extra...), adv_extra<WfSky>(extra...), adv_extra<WfSkyDist>(extra...),
                              adv_extra<WfEmit>(extra...), adv_extra<WfFresnel>(extra...), adv_extra<WfGloss>(extra...), adv_extra<WfTint>(extra...));
    wf_flush_work<(FORM & kFormStats) != 0>(fr, wk);                  // (the counting forms) every lane of the wave arrives here (wave-level sums)
}

}  // namespace rtk
