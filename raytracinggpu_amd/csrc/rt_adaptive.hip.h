// rt_adaptive.hip.h -- adaptive sampling (rt_render_counts*, rt_sample_counts*, rt_kat_sample_plan; raytrace_hip.h): a frame whose pixels get different numbers of
// samples, traced as a COMPACTED LIST of (pixel slot, sample) items instead of the dense grid "pixel slot x sample" of a frame with num_rays samples everywhere.
//
//   plan     three launches over the pixel slots (the 8 x 8 tile order of wf_decode: a wave's 64 slots are one tile):
//              sample_plan_totals   the samples to trace of every workgroup's kPlanBlock slots, summed
//              sample_plan_scan     ONE workgroup: exclusive scan of those totals, kPlanLevel of them per round with a running carry; the grand total
//              sample_plan_scatter  every slot's offset (workgroup's offset + waves before + DPP scan inside the wave) into offs[], and the item records
//                                   slot << 6 | sample of its samples, slot-major then sample, written by the whole wave (coalesced)
//            Nothing waits for another workgroup and no atomic decides an order: the list is a function of the counts.  The host reads the grand total back once
//            (it sizes the list and the chains) between the scan and the scatter.
//   chain    wf_advance<kFormList [| kFormFirst | kFormTex]> (rt_wavefront.hip.h): the LIST form -- (px, lrow, samp, valid) come from the item record; every item writes its
//            colour to samp_out[i].  The launches between are the dense chain's own (wf_travq and all).
//   fold     sample_fold: one lane per pixel slot adds its items' colours in sample order (cpu:711), from `base` if the caller brought the first sample, divides as
//            path_reduce does with the pixel's own count, and stores the pixel.  A list cut into several chains is folded chain by chain (T carries the sum).
//   counts   sample_counts_kernel: elementwise, how many samples a pixel wants from its history (m1, m2, n, V).
#pragma once
#include "rt_wavefront.hip.h"
#include "rt_travq.hip.h"

namespace rtk {

constexpr int kMaxSampleCount = 64;                  // RT_MAX_SAMPLE_COUNT: a sample index fits the low 6 bits of an item record
constexpr int kPlanBlock = 256;                      // slots (threads) of one workgroup of the plan's first and third launch: four tiles
constexpr int kPlanLevel = 1024;                     // workgroup totals the scan's one workgroup takes per round
constexpr int kItemShift = 6;                        // item record: pixel slot << 6 | sample index
constexpr int64_t kPlanMaxSlots = (int64_t)1 << 26;  // slot << 6 is 32 bits, and 64 samples on every slot still count in 32 bits

struct PlanArgs {
    const uint8_t *counts;       // [H * W], pixel order
    int W, H, tiles_x, n_slots;  // n_slots = tiles_x * tiles_y * 64
    int first;                   // samples [first, c) of a pixel are traced (1: the caller brought sample 0 as `base`)
};
// the pixel of a slot (wf_decode's order, whole frame), its count read as at most kMaxSampleCount (0 outside the frame)
__device__ __forceinline__ int plan_count(const PlanArgs &a, int slot, int &px, int &row) {
    const int tile = slot >> 6, p = slot & 63;
    const int ty = tile / a.tiles_x;
    px = (tile - ty * a.tiles_x) * 8 + (p & 7);
    row = ty * 8 + (p >> 3);
    if (slot >= a.n_slots || px >= a.W || row >= a.H) return 0;
    const int c = a.counts[(size_t)row * a.W + px];
    return c > kMaxSampleCount ? kMaxSampleCount : c;
}
__device__ __forceinline__ unsigned int plan_traced(const PlanArgs &a, int slot) {
    int px, row;
    const int c = plan_count(a, slot, px, row);
    return c > a.first ? (unsigned int)(c - a.first) : 0u;
}

// launch 1: block_tot[b] = samples to trace of slots [b * kPlanBlock, (b + 1) * kPlanBlock).  (Every lane of every wave stays to the end: the DPP sums want 64 lanes.)
__global__ __launch_bounds__(kPlanBlock) void sample_plan_totals(const PlanArgs a, unsigned int *__restrict__ block_tot) {
    __shared__ unsigned int wsum[kPlanBlock / 64];
    const int slot = blockIdx.x * kPlanBlock + threadIdx.x;
    const unsigned int s = wave_sum(plan_traced(a, slot));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int k = 0; k < kPlanBlock / 64; ++k) t += wsum[k];
        block_tot[blockIdx.x] = t;
    }
}

// launch 2, one workgroup: block_off[b] = sum of block_tot[0 .. b); total[0] = the sum of them all.  kPlanLevel totals per round, the carry in a register of every lane.
__global__ __launch_bounds__(kPlanLevel) void sample_plan_scan(const unsigned int *__restrict__ block_tot, int n_blocks, unsigned int *__restrict__ block_off,
                                                               unsigned int *__restrict__ total) {
    __shared__ unsigned int wsum[kPlanLevel / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int carry = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += kPlanLevel) {                // (trip count uniform over the workgroup)
        const int b = b0 + (int)threadIdx.x;
        const unsigned int v = b < n_blocks ? block_tot[b] : 0u;
        const unsigned int incl = wave_incl_scan(v);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned int before = 0, all = 0;
        for (int k = 0; k < kPlanLevel / 64; ++k) { const unsigned int w = wsum[k]; if (k < wave) before += w; all += w; }
        if (b < n_blocks) block_off[b] = carry + before + (incl - v);
        carry += all;
        __syncthreads();                                               // wsum is rewritten by the next round
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// launch 3: offs[slot] for every slot and offs[n_slots] = the total; with `items`, the wave's records -- its items are the contiguous range behind its first slot's offset,
// item j of the wave belongs to the first lane whose inclusive sum exceeds j (a binary search over the wave's 64 sums in LDS)
__global__ __launch_bounds__(kPlanBlock) void sample_plan_scatter(const PlanArgs a, const unsigned int *__restrict__ block_off, const unsigned int *__restrict__ total,
                                                                  unsigned int *__restrict__ offs, unsigned int *__restrict__ items) {
    __shared__ unsigned int wsum[kPlanBlock / 64];
    __shared__ unsigned int wincl[kPlanBlock / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = blockIdx.x * kPlanBlock + threadIdx.x;
    const unsigned int t = plan_traced(a, slot);
    const unsigned int incl = wave_incl_scan(t);
    wincl[wave][lane] = incl;
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned int wbase = block_off[blockIdx.x];
    for (int k = 0; k < wave; ++k) wbase += wsum[k];
    if (slot < a.n_slots) offs[slot] = wbase + (incl - t);
    if (slot == 0) offs[a.n_slots] = total[0];
    if (items == nullptr) return;
    const unsigned int wtot = wsum[wave];
    const int slot0 = slot - lane;
    for (unsigned int j = (unsigned int)lane; j < wtot; j += 64u) {
        int lo = 0, hi = 63;                                           // the first lane l with wincl[l] > j (exists: j < wincl[63])
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (wincl[wave][mid] > j) hi = mid; else lo = mid + 1;
        }
        const unsigned int excl = lo > 0 ? wincl[wave][lo - 1] : 0u;
        items[(size_t)wbase + j] = (unsigned int)(slot0 + lo) << kItemShift | ((unsigned int)a.first + (j - excl));
    }
}

// ---- the fold ----
// Items [i0, i1) of the list are the chain whose colours samp_out holds (samp_out[j - i0]); last: the list ends at i1.  A slot with items in this chain adds them to its
// sum -- begun here (offs[slot] >= i0) from nothing or from `base`, else from T -- and stores the pixel if its items end here, else T.  A slot without items is stored by
// the chain its offset falls into (the last one takes those at the very end).  Each pixel of out / base / T is read and written by one lane: out == base is safe.
struct FoldArgs {
    PlanArgs plan;
    const unsigned int *offs;
    const float4 *samp_out;
    const float4 *base;          // or nullptr
    float4 *T;                   // [n_slots]; touched only when the list is cut into several chains
    unsigned int i0, i1;
    int last;
};
__global__ __launch_bounds__(256) void sample_fold(const Frame fr, const FoldArgs f) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= f.plan.n_slots) return;
    int px, row;
    const int c = plan_count(f.plan, slot, px, row);
    if (px >= fr.W || row >= fr.H) return;
    const unsigned int a = f.offs[slot], b = f.offs[slot + 1];
    const size_t o = out_index(fr, row, px);
    if (a == b) {                                                      // nothing traced for this pixel: no sample at all, or only the one `base` holds
        if (!((a >= f.i0 && a < f.i1) || (f.last && a == f.i1))) return;
        fr.out[o] = f.base ? f.base[o] : make_float4(0, 0, 0, 0);
        return;
    }
    const unsigned int lo = a > f.i0 ? a : f.i0, hi = b < f.i1 ? b : f.i1;
    if (lo >= hi) return;
    const float inv_n = fr.cam_mode == 1 ? (float)(1. / (double)c) : 1.f;   // realtime:1131 with this pixel's count
    float4 t;
    if (a >= f.i0) {
        t = make_float4(0, 0, 0, 0);
        if (f.base) {                                                  // sample 0, as a one-sample frame stored it: (0 + a0) / 1
            const float4 s = f.base[o];
            if (fr.cam_mode == 1) { t.x += s.x * inv_n; t.y += s.y * inv_n; t.z += s.z * inv_n; }
            else { t.x += s.x; t.y += s.y; t.z += s.z; }
            t.w += s.w;
        }
    } else {
        t = f.T[slot];
    }
    for (unsigned int j = lo; j < hi; ++j) {
        const float4 s = f.samp_out[j - f.i0];
        if (fr.cam_mode == 1) { t.x += s.x * inv_n; t.y += s.y * inv_n; t.z += s.z * inv_n; }
        else { t.x += s.x; t.y += s.y; t.z += s.z; }
        t.w += s.w;
    }
    if (b <= f.i1) {
        const float n = fr.cam_mode == 1 ? 1.f : (float)c;
        fr.out[o] = make_float4(t.x / n, t.y / n, t.z / n, t.w);
    } else {
        f.T[slot] = t;
    }
}

// ---- counts from a history (rt_sample_counts*): plane 1 of rt_temporal_accumulate*, (m1, m2, n, V) per pixel; the formula is in raytrace_hip.h ----
struct SampleCountArgs { float max_extra, short_history, new_extra, k_rel, lum_floor; };
__global__ __launch_bounds__(256) void sample_counts_kernel(const float4 *__restrict__ plane1, int64_t npix, const SampleCountArgs a, uint8_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 h = plane1[i];
    float count = 1.f;
    if (!(h.z == 0.f)) {
        const float e_n = h.z < a.short_history ? a.new_extra : 0.f;
        const float rel = h.w / (h.x * h.x + a.lum_floor);
        float e_v = floorf(a.k_rel * rel);
        if (!(e_v >= 1.f)) e_v = 0.f;
        count = 1.f + fminf(a.max_extra, fmaxf(e_n, e_v));
    }
    counts[i] = (uint8_t)(int)count;
}

}  // namespace rtk
