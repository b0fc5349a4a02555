// gfx950 (MI355X, wave64) kernels of the wavefront path tracer.
//
//   k_generate      main.rs:186-199   seed draw, shuffled-scrambled Sobol jitter, camera ray (pt_camera.h: primary_ray by the camera kind CAM --
//                   pinhole, the thin lens of pt_set_lens, the panoramic and orthographic cameras of pt_set_projection; the last three's
//                   rays have origins of their own, which bounce 0's FIRST_OWN_* variants of the passes below read)
//   k_closest       tlas.rs:66-110 + blas.rs:214-256 + boundingbox.rs:115-131 + primitive.rs:117-178
//                   persistent-threads ordered traversal; BVH staged in LDS; per-lane stack in LDS;
//                   ballot/mbcnt refill of idle lanes from the ray queue; material binning of the hits;
//                   paths that end at the hit or miss are finished here (integrator.rs:207-214, 263-266)
//   k_any           tlas.rs:111-144 + blas.rs:257-294   (shadow rays; finishes paths that died owing one explicit-light estimate)
//   k_shade_surface<class>, k_shade_terminal   integrator.rs:163-270 split per material class; the NEE of the previous bounce is
//                   resolved first; BSDF-sampled NEE rays that miss the lights' root box are answered on the spot
//                   (LDS-resident scenes: the Lambertian pass also walks its own explicit-light shadow rays, inline_any: no shadow queue, no k_any launch)
//   k_accumulate    integrator.rs:272-280 + accumulate.wgsl:20-23 in sample order
//
// Arithmetic: pt_math.h / pt_materials.h.  Built with -ffp-contract=off; v_min/v_max are used in the slab test only
// where they provably equal the SSE select semantics of the reference (see slab()).
#include "pt_kernels.h"
#include "pt_camera.h"
#include "pt_probe.h"
#include "pt_materials.h"
#include "pt_queue_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

namespace pt {
namespace {

#ifndef PT_STEPS_PER_ROUND
#define PT_STEPS_PER_ROUND 8
#endif
#ifndef PT_REFILL_BELOW
#define PT_REFILL_BELOW 40
#endif
#ifndef PT_STEPS_PER_ROUND_GLOBAL_BVH
#define PT_STEPS_PER_ROUND_GLOBAL_BVH 4
#endif
#ifndef PT_REFILL_BELOW_GLOBAL_BVH
#define PT_REFILL_BELOW_GLOBAL_BVH 56
#endif
#ifndef PT_STEPS_ANY
#define PT_STEPS_ANY 4 // any-hit rays are short: same-box sweep 3 / 4 / 5 / 6 / 8 / 10 / 12: 70.8 / 67.6 / 69.0 / 69.4 / 69.9 / 69.3 / 69.6 ms per frame
#endif
#ifndef PT_REFILL_BELOW_ANY
#define PT_REFILL_BELOW_ANY PT_REFILL_BELOW
#endif
// waves per SIMD the compiler must leave room for in the traversal kernels (second parameter of __launch_bounds__): FIVE, for every variant.
// BVH in global memory: the kernels wait on L2 — one more DEPENDENT load per branch level, an L1 hit, costs the closest-hit kernel 10-13 %
// (experiments/r04_latency_probe.patch, round 4) — so a fifth wave pays, provided it is not bought with scratch: round 2 asked the compiler for 5 or
// 6 waves of the kernel as it was (123-127 VGPRs wanted: 72-164 B of scratch) and got +-0 / -15 %; round 4 first took the register peak away — the
// closest-hit leaves test ONE triangle at a time instead of two side by side (123 -> 105 VGPRs) — and then 96 VGPRs cost 8-20 B of scratch, all of it
// in the service sections.  Same-box A/B, whole frame at 64 spp, atrium / 82 k mesh / 328 k mesh / spheres: pairs at 4 waves 325 / 73.6 / 123.5 / 54.4 ms,
// single at 4 waves 309 / 70.1 / 119.6 / 52.9, single at 5 waves 281 / 67.2 / 115.0 / 49.6 (-14 / -9 / -7 / -9 %); 6 waves (80 VGPRs, 64-88 B of
// scratch, 13 stack levels in LDS) 315 / 71.7 / 124.0 / 54.4; any-hit alone at 6: 295 / 68.3 / 114.7 / 51.4.
// BVH in LDS: these kernels run at 0.80-0.87 of VALU issue at four waves, and the same change fills most of the rest: Cornell 256 spp 66.3 -> 61.4 ms,
// its 1/8 share 10.1 -> 9.4 ms, mixed materials 77.4 -> 72.2 ms (k_trace_fused then carries 48 B of scratch).  Pairs at five waves 63.3 / 9.55 / 74.8; single
// at four 65.1 / 10.1 / 75.6; closest-hit four + any-hit five 64.5 / 9.7 / 74.7; closest-hit five + any-hit six 62.9 / 9.5 / 74.5; six for both 66.4 / 10.0 / 77.3;
// world + NEE launches unfused at five 62.1 / 9.5 / 73.5.
#ifndef PT_WAVES_LDS_BVH
#define PT_WAVES_LDS_BVH 5
#endif
#ifndef PT_WAVES_LDS_BVH_ANY
#define PT_WAVES_LDS_BVH_ANY 5
#endif
#ifndef PT_WAVES_GLOBAL_BVH
#define PT_WAVES_GLOBAL_BVH 5
#endif
#ifndef PT_WAVES_GLOBAL_BVH_ANY
#define PT_WAVES_GLOBAL_BVH_ANY 5
#endif
// One-ray walk (IDENT kernels), BVH in LDS: SIX workgroups of 256 per CU (six waves per SIMD), set as the cap of the resident grid (resident_grid), not as
// the compiler's bound.  Built without fp32 pairing (csrc/Makefile) these kernels take 64-79 VGPRs and no scratch, so six fit — the "six is slower" above was
// measured with 64-120 B of scratch.  Same-box A/B, Cornell frame, six runs each (profiles/r08_fp32_pairing.md): grid capped at five 53.79-54.22 ms, at six
// 53.35-53.67; rank 0's 1/8 share 8.33-8.57 -> 8.21-8.25; one pipeline, k_trace_fused per launch 2506 -> 2340 us, the primary k_closest the same at either.
// __launch_bounds__(256, 6) on top of the cap changes no instruction of these kernels (register names in a handful) and was SLOWER in every run, 54.66-55.25:
// the bound stays at five, the wave count is pinned from above here and watched from below by tools/resource_table.py.
// Six workgroups per CU need <= 26.6 KB of LDS each (the Cornell blob plus stacks: ~24 KB); larger scenes run what fits.
#ifndef PT_TRACE_WAVES_LDS_IDENT
#define PT_TRACE_WAVES_LDS_IDENT 6
#endif
// waves per SIMD a traversal kernel's resident grid is capped at (0: whatever the runtime reports for its registers and LDS)
constexpr uint32_t trace_waves_cap(bool lds, bool ident) { return lds && ident ? PT_TRACE_WAVES_LDS_IDENT : 0; }
// branch levels expanded per traversal step of k_closest (1 = one node per step)
#ifndef PT_BRANCH_LEVELS
#define PT_BRANCH_LEVELS 4
#endif
#ifndef PT_BRANCH_LEVELS_ANY
#define PT_BRANCH_LEVELS_ANY 4
#endif
#ifndef PT_BRANCH_LEVELS_INLINE
#define PT_BRANCH_LEVELS_INLINE 6 // ... of the shadow walk inside the Lambertian shading pass (inline_any; no refill there, so fewer, longer steps: same-box 1 / 2 / 3 / 4 / 6 / 8: Cornell frame 59.05 / 57.9 / 57.8 / 57.4 / 56.95 / 56.9 ms, one pipeline 60.8 / 59.9 / 59.9 / 59.3 / 59.0 / 59.3)
#endif
// frames with fewer local pixels than this use four lanes per pixel in k_accumulate (k_accumulate<FEW_PIXELS>)
#ifndef PT_ACC_QUAD_BELOW
#define PT_ACC_QUAD_BELOW (1u << 30) // (whole 1080p frame: 0.675 -> 0.55 ms; beyond 2^30 pixels the thread index would overflow)
#endif
// PT_STEP_STATS (variant builds, tools/step_stats.py): per traversal step of k_closest, how many lanes take each section
#ifndef PT_STEP_STATS
#define PT_STEP_STATS 0
#endif
// PT_WAVE_TIMES (variant builds, tools/wave_times.py): when the waves of a k_closest launch start, first have rays, find the queue empty, end
#ifndef PT_WAVE_TIMES
#define PT_WAVE_TIMES 0
#endif
// tapered chunks: 64-ray chunks per wave in a queue's last level (0 = chunks of one size; chunk_of)
#ifndef PT_TAPER
#define PT_TAPER 2
#endif
#ifndef PT_TAPER_ANY
#define PT_TAPER_ANY 0
#endif
#ifndef PT_RESERVICE
#define PT_RESERVICE 1
#endif
#ifndef PT_CLAIM_AHEAD
#define PT_CLAIM_AHEAD 0 // rays left in a chunk when the next one is claimed; 0 = as soon as the chunk is taken up (same-box A/B of 64 / 128 / 256: +0.3 ms for a 1/8 share, +3 ms per frame)
#endif
// threads per shading workgroup (a workgroup makes one reservation per queue and iteration: block_append4)
// waves per SIMD the surface shading kernels must leave room for (1: whatever the registers they want allow — 102-130 VGPRs: four, GGX with volumes three).
// Five: the Lambertian kernel fits 96 VGPRs without scratch (90-95 since round 8; with the inline shadow walk 90, where SLP pairing had cost 52 B of scratch).  Round 3 measured that at FOUR traversal waves: the pass's own launches 22.39 -> 22.26 ms, the
// two-pipeline frame +1 ms.  Round 4, traversal kernels at five waves: one pipeline 62.35 -> 62.63 ms (nothing), but the default two-pipeline frame
// 61.2 -> 59.0 ms and mixed materials 72.8 -> 70.0 ms: the fifth wave lets one pipeline's shading pass run beside the other's traversal.  Six (80 VGPRs, 60 B
// of scratch): 64.4 / 76.0 ms.
#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 5
#endif
#ifndef PT_SHADE_WAVES_DIEL
#define PT_SHADE_WAVES_DIEL 5   // (93 VGPRs, no scratch since the build dropped fp32 pairing: profiles/r08_fp32_pairing.md)
#endif
#ifndef PT_SHADE_WAVES_GGX
#define PT_SHADE_WAVES_GGX 5    // (better than four waves even with the 64 B of scratch it had until round 8: mixed materials 71.5 -> 70.3 ms; now 96 VGPRs, no scratch)
#endif
#ifndef PT_SHADE_WAVES_VOLUMES
#define PT_SHADE_WAVES_VOLUMES 4 // kernels of scenes with participating media (five: 32-104 B of scratch; media scene 47.2 -> 48.7 ms.  Without fp32 pairing the specular and
                                 // dielectric ones fit 96 VGPRs without scratch, the Lambertian and GGX ones want 113-120: cornell_media at 256 spp 163.2 / 163.8 ms at four, 164.2 / 163.8 at five)
#endif
constexpr int shade_waves(uint32_t qclass, bool volumes)
{
    return volumes ? PT_SHADE_WAVES_VOLUMES : (qclass == Q_GGX ? PT_SHADE_WAVES_GGX : (qclass == Q_DIELECTRIC ? PT_SHADE_WAVES_DIEL : PT_SHADE_WAVES));
}
// LDS-resident scenes: the Lambertian shading pass traces its explicit-light shadow ray itself (inline_any) instead of queueing it for k_any<SHADOW>: same box,
// Cornell frame 58.45 -> 57.5 ms, one pipeline 62.1 -> 59.8, 1/4 and 1/8 share 16.4 / 9.4 -> 15.6 / 8.95, mixed materials 64 spp 21.1 -> 20.0.  At four waves per SIMD
// (PT_SHADE_WAVES_INLINE, 128 VGPRs) it wins on one pipeline only (61.7) and loses the two-pipeline overlap (61.5); five waves need the walk AFTER the record store.
#ifndef PT_INLINE_SHADOW
#define PT_INLINE_SHADOW 1
#endif
#ifndef PT_IDENT_SHADE
#define PT_IDENT_SHADE 1 // the Lambertian shading pass's inline shadow walk also takes the one-ray walk on identity-only scenes (ident_ray)
#endif
#ifndef PT_SHADE_WAVES_INLINE
#define PT_SHADE_WAVES_INLINE 5
#endif
#ifndef PT_SHADE_THREADS
#define PT_SHADE_THREADS 256
#endif
#ifndef PT_CHUNK_DIV
#define PT_CHUNK_DIV 4
#endif
// scenes whose BVH stays in global memory have long rays: smaller chunks, shorter launch tails (same-box A/B on the 82 k / 328 k meshes: -3 % / -7 %)
#ifndef PT_CHUNK_DIV_GLOBAL_BVH
#define PT_CHUNK_DIV_GLOBAL_BVH 16
#endif
// traversal steps between refill checks, and: refill idle lanes when at most this many lanes are still traversing.  Scenes whose BVH
// stays in global memory (long rays, every step waits on L2) want their lanes refilled sooner and more often: same-box A/B of
// 32…62 lanes x 4…16 steps on the 82 k / 328 k meshes: 56 lanes x 4 steps -6 % / -5 % against the LDS scenes' 40 x 8.
template <bool LDS_SCENE> struct Refill
{
    static constexpr int kSteps = LDS_SCENE ? PT_STEPS_PER_ROUND : PT_STEPS_PER_ROUND_GLOBAL_BVH;
    static constexpr int kStepsAny = LDS_SCENE ? PT_STEPS_ANY : PT_STEPS_PER_ROUND_GLOBAL_BVH;
    static constexpr int kBelow = LDS_SCENE ? PT_REFILL_BELOW : PT_REFILL_BELOW_GLOBAL_BVH;
    static constexpr int kBelowAny = LDS_SCENE ? PT_REFILL_BELOW_ANY : PT_REFILL_BELOW_GLOBAL_BVH;
};

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// Persistent-thread work fetch: FetchPlan, chunk_of and fetch_plan (pt_queue_plan.h) say which rays are whose; the claims themselves follow.
// the plan of the launch this thread runs in.  (The launch's shape is read HERE, the block size first: read at the call sites the compiler
// merged the kernels' two plans differently, and the move of this arithmetic into the header was to leave the generated code as it was.)
__device__ __forceinline__ FetchPlan fetch_plan(uint32_t n, uint32_t chunk_div, uint32_t taper)
{
    const uint32_t wpb = blockDim.x >> 6;
    return pt::fetch_plan(n, chunk_div, taper, gridDim.x, wpb);
}
struct WaveRange
{
    uint32_t cur, end;
    uint32_t home;    // partition this wave tries first
    bool drained;     // the queue has no chunk left for this wave
    // The claim for the chunk AFTER the current one is issued when the current one is taken up and its answer is looked at only
    // when the current one runs out, so the atomic's round trip overlaps the traversal instead of stalling the wave (a same-box
    // A/B of synchronous claims: every halving of the chunk size cost ~2 % of the frame).  A claim that succeeded owns its chunk:
    // the wave always looks at the answer before it leaves.
    bool nx_valid;    // a claim is outstanding
    uint32_t nx_p;    // ... on this partition
    uint32_t nx_got;  // ... and this is the atomic's return value (lane 0): the chunk's index in the partition
};
__device__ __forceinline__ void prefetch_claim(WaveRange& wr, uint32_t* heads, const FetchPlan& pl)
{
    wr.nx_valid = true;
    wr.nx_p = wr.home;
    if (lane_id() == 0u) wr.nx_got = atomicAdd(heads + wr.home * kHeadStrideWords, 1u);
}
// chunk `idx` of partition p, clipped to the queue; false if nothing of it exists
__device__ __forceinline__ bool take_claim(WaveRange& wr, const FetchPlan& pl, uint32_t p, uint32_t idx)
{
    return claim_range(pl, p, idx, wr.cur, wr.end);
}
__device__ __forceinline__ WaveRange first_range(const FetchPlan& pl, uint32_t* heads)
{
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform: keep the range in SGPRs
    WaveRange wr;
    static_range(pl, wave, wr.cur, wr.end);
    wr.home = (wave * 7u) & (kQueueHeads - 1u); // neighbouring waves start on different cursors
    wr.drained = pl.n_static >= pl.n;            // nothing is handed out dynamically
    wr.nx_valid = false;
    wr.nx_p = 0u;
    wr.nx_got = 0u;
    if (!wr.drained && (PT_CLAIM_AHEAD == 0 || wr.end - wr.cur <= (uint32_t)PT_CLAIM_AHEAD)) prefetch_claim(wr, heads, pl);
    return wr;
}
// returns how many of the wave's idle lanes receive a ray; lane i (rank r among idle lanes) gets ray first + r
__device__ __forceinline__ uint32_t claim_rays(WaveRange& wr, uint32_t* heads, const FetchPlan& pl, uint32_t n_idle, uint32_t& first)
{
    if (wr.cur >= wr.end && !wr.drained)
    {
        bool have = false;
        if (wr.nx_valid)
        {
            const uint32_t got = __builtin_amdgcn_readfirstlane(wr.nx_got);
            wr.nx_valid = false;
            have = take_claim(wr, pl, wr.nx_p, got);
        }
        const uint32_t l = lane_id();
        while (!have) // the home partition is empty: look at all cursors; at most kQueueHeads rounds (a failed claim = an empty partition)
        {
            const uint32_t h = __hip_atomic_load(heads + l * kHeadStrideWords, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t st_l = 0u, len_l = 0u;
            const bool more = chunk_of(pl, h, st_l, len_l) && (uint64_t)l * pl.psize + st_l < (uint64_t)(pl.n - pl.n_static);
            const uint64_t m = __ballot(more);
            if (m == 0ull) { wr.drained = true; wr.cur = wr.end = pl.n; break; }
            const uint64_t rot = wr.home == 0u ? m : ((m >> wr.home) | (m << (64u - wr.home)));
            const uint32_t p = (wr.home + (uint32_t)__builtin_ctzll(rot)) & (kQueueHeads - 1u);
            uint32_t got = 0;
            if (l == 0u) got = atomicAdd(heads + p * kHeadStrideWords, 1u);
            got = __builtin_amdgcn_readfirstlane(got);
            wr.home = p;
            have = take_claim(wr, pl, p, got);
        }
        if (!wr.drained && PT_CLAIM_AHEAD == 0) prefetch_claim(wr, heads, pl);
    }
    const uint32_t take = min(n_idle, wr.end - wr.cur);
    first = wr.cur;
    wr.cur += take;
    // The next chunk is claimed when the current one has PT_CLAIM_AHEAD rays left — a couple of refills, time enough for the atomic's
    // round trip — not when it is taken up: what a wave owns when the queue runs dry is then about one chunk, not two, and the
    // launch's tail is that much shorter.
    if (PT_CLAIM_AHEAD != 0 && !wr.nx_valid && !wr.drained && wr.end - wr.cur <= (uint32_t)PT_CLAIM_AHEAD) prefetch_claim(wr, heads, pl);
    return take;
}

// exact count of what a wave processed, added to the cursor line of its home partition (64 addresses per queue instead of one)
__device__ __forceinline__ void add_tally(uint32_t* heads, uint32_t per_lane, uint32_t word)
{
    uint32_t total = per_lane;
    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (total != 0u && lane_id() == 0u) atomicAdd(heads + ((wave * 7u) & (kQueueHeads - 1u)) * kHeadStrideWords + word, total);
}

// Queue appends.  A returning atomic on ONE queue-tail word sustains ~88 operations per microsecond on MI355X (price list
// "dequeue"), and a wavefront renderer wants ~10^10 appended entries per second, so nobody appends entry by entry:
//  * a TRAVERSAL WAVE (k_closest -> shade queues) RESERVES a private region of the output queue with one atomic, fills it locally
//    and reserves the next one when it runs out.  Whatever is left of its last region when the wave exits is filled with HOLE
//    markers that consumers skip; these queues' extents therefore count slots, not entries.  The surface classes' queues hand their
//    regions out over up to 64 striped tail words (wave_reserve_striped below); the terminal queue, which sees little traffic, keeps
//    one tail and regions of 64 slots, or slots_in / (waves * 16) clamped to [64, 8192] when an environment map sends every miss there (region_size);
//  * a SHADING WORKGROUP (-> ray queues, terminal queue) reserves exactly what it appends, once per queue and iteration
//    (block_append4): those queues are dense.  Holes are not free — a hole is an idle lane until the next refill — and were measured
//    to cost more than the reservations they save, see block_append4.
// (Tried: regions shared by the four waves of a traversal workgroup through an LDS cursor: tail atomics / 4, but the per-retirement
// LDS atomic cost 2 ms per frame.)
//
// Capacity: a reservation that would pass the queue's capacity is diverted to the queue's dump area (kQueueDumpSlots slots past the
// capacity, shared by everybody who overflows) and raises the batch's overflow flag: nothing is ever stored out of bounds, the
// host turns the flag into PT_ERR_LIMIT.  Consumers clamp the slot count they read to the capacity.
enum : uint32_t { PRIMARY_MISS = 0xffu /* PathState::occl: the camera ray left the scene at once (radiance = ambient) */ };
enum : uint32_t { HOLE = 0xffffffffu, PATH_ENDS = 0x80000000u /* shadow-ray path ids: see k_any */ };
struct Region { uint32_t cur, end; };
// one thread: next region of `rsize` slots, or the dump area when the queue is full
__device__ __forceinline__ uint32_t next_region(const Region& rg, uint32_t* counter, uint32_t rsize, uint32_t cap, uint32_t* overflow)
{
    if (rg.end > cap) return cap; // already diverted: stay in the dump area and leave the counter alone (it must not wrap)
    const uint32_t nb = atomicAdd(counter, rsize);
    if (cap < rsize || nb > cap - rsize)
    {
        __hip_atomic_store(overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return cap;
    }
    return nb;
}
// wave-uniform: take `total` slots; entries ranked below `left` go to base0 + rank, the others to base1 + (rank - left)
struct Placement { uint32_t base0, left, base1; };
__device__ __forceinline__ uint32_t place(const Placement& p, uint32_t rank) { return rank < p.left ? p.base0 + rank : p.base1 + (rank - p.left); }
__device__ __forceinline__ Placement wave_reserve(Region& rg, uint32_t* counter, uint32_t total, uint32_t rsize, uint32_t cap, uint32_t* overflow)
{
    Placement p{rg.cur, rg.end - rg.cur, 0u};
    if (total > p.left)
    {
        uint32_t nb = 0;
        if (lane_id() == 0u) nb = next_region(rg, counter, rsize, cap, overflow);
        nb = __shfl(nb, 0);
        p.base1 = nb;
        rg.cur = nb + (total - p.left);
        rg.end = nb + rsize;
    }
    else rg.cur += total;
    return p;
}

// ---- striped tails (pt_types.h): the same region scheme with the reservations spread over up to 64 tail words (Stripes, stripes_for: pt_queue_plan.h)
// one thread: the next region of stripe `rot & (K - 1)`, or the dump area when the queue is full
__device__ __forceinline__ uint32_t next_region_striped(const Region& rg, uint32_t* tails, const Stripes st, uint32_t rot, uint32_t cap, uint32_t* overflow)
{
    if (rg.end > cap) return cap; // already diverted: stay in the dump area
    const uint32_t k = rot & ((1u << st.log_k) - 1u);
    const uint32_t r = atomicAdd(tails + k * kTailStrideWords, 1u);
    const uint64_t base = stripe_region_base(st, r, k);
    if (!stripe_region_fits(st, base, cap))
    {
        __hip_atomic_store(overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return cap;
    }
    return (uint32_t)base;
}
// wave-uniform, like wave_reserve; `rot` moves on with every reservation so that a producer visits all stripes in turn
__device__ __forceinline__ Placement wave_reserve_striped(Region& rg, uint32_t* tails, const Stripes st, uint32_t& rot, uint32_t total, uint32_t cap, uint32_t* overflow)
{
    Placement p{rg.cur, rg.end - rg.cur, 0u};
    if (total > p.left)
    {
        uint32_t nb = 0;
        if (lane_id() == 0u) nb = next_region_striped(rg, tails, st, rot, cap, overflow);
        nb = __builtin_amdgcn_readfirstlane(nb);
        rot += 1u;
        p.base1 = nb;
        rg.cur = nb + (total - p.left);
        rg.end = nb + (1u << st.log_r);
    }
    else rg.cur += total;
    return p;
}
// consumer side.  Lane l of the calling wave loads tail l; returns the queue's extent in slots (clamped to cap), wave-uniform
__device__ __forceinline__ uint32_t stripe_load(const uint32_t* tails, const Stripes st, uint32_t cap, uint32_t& my_tail)
{
    const uint32_t l = lane_id();
    my_tail = l < (1u << st.log_k) ? tails[l * kTailStrideWords] : 0u;
    uint32_t ext = stripe_extent(st, l, my_tail, cap);
    for (int off = 32; off > 0; off >>= 1) ext = max(ext, (uint32_t)__shfl_xor((int)ext, off));
    return ext;
}
// Block-wide queue append for up to four queues at once: the workgroup reserves EXACTLY what it appends, one atomic per queue and
// call (two barriers).  Regions per workgroup, as the traversal waves use them, were tried first (region = slots_in / (workgroups * 16),
// at least 256): fewer atomics, but whatever 3072 workgroups leave of their last regions are holes in the next launch's queue — for
// a 0.14 M-ray bounce of a 1/8 share 0.4 M of them — and holes cost more than the atomics even where those run at the one-word limit
// (~88 per microsecond is what a full-speed shading launch makes: 22 entries per ns / 256).  Same-box A/B, exact against regions:
// whole frame 69.6 -> 69.0 ms, 1/2 share 36.9 -> 35.4, 1/4 19.3 -> 18.6, 1/8 10.8 -> 10.2 ms, 1-spp frame 1.40 -> 1.22 ms, mixed
// materials 14.5 -> 12.8 ms, 82 k mesh 14.1 -> 13.4 ms.
struct BlockAppend
{
    uint32_t wave_cnt[4][PT_SHADE_THREADS / 64];
    uint32_t wave_rank[4][PT_SHADE_THREADS / 64]; // rank of the wave's first entry inside the workgroup's tile
    uint32_t base[4];
};
__device__ __forceinline__ void block_append4(BlockAppend& sh, uint32_t* const counters[4], const bool pred[4], const uint32_t caps[4], uint32_t* overflow, uint32_t pos[4])
{
    const uint32_t wid = threadIdx.x >> 6;
    uint64_t m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        m[q] = __ballot(pred[q]);
        if (lane_id() == 0u) sh.wave_cnt[q][wid] = (uint32_t)__popcll(m[q]);
    }
    __syncthreads();
    if (threadIdx.x < 4u)
    {
        const uint32_t q = threadIdx.x;
        const uint32_t nw = blockDim.x >> 6;
        uint32_t total = 0;
        for (uint32_t w = 0; w < nw; ++w) { sh.wave_rank[q][w] = total; total += sh.wave_cnt[q][w]; }
        uint32_t base = caps[q]; // a full queue: the entries go to its dump area (kQueueDumpSlots >= a workgroup's 256), nothing is stored out of bounds
        if (total != 0u)
        {
            const uint32_t nb = atomicAdd(counters[q], total);
            if (nb > caps[q] || total > caps[q] - nb) __hip_atomic_store(overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else base = nb;
        }
        sh.base[q] = base;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) pos[q] = sh.base[q] + sh.wave_rank[q][wid] + mbcnt64(m[q]);
    __syncthreads(); // the shared tables are rewritten by the next iteration
}

__device__ __forceinline__ f3 xyz(const f4& v) { return f3{v.x, v.y, v.z}; }
__device__ __forceinline__ float asf(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t asu(float f) { return __float_as_uint(f); }

// Streaming accesses of the shading pass: rays and hit records are written once and read once, by the next kernel, long after the
// ~200 GB in between have flushed every cache; "nt" accesses keep them from displacing the records and scene tables in L2
// (same-box A/B: -0.6 ms per frame; the 64-byte path records must NOT be streamed: their four words merge in L2, +4 ms without).
typedef float nt4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void nt_store(f4* p, f4 v) { __builtin_nontemporal_store(nt4_t{v.x, v.y, v.z, v.w}, reinterpret_cast<nt4_t*>(p)); }
__device__ __forceinline__ f4 nt_load(const f4* p) { const nt4_t v = __builtin_nontemporal_load(reinterpret_cast<const nt4_t*>(p)); return f4{v.x, v.y, v.z, v.w}; }


// AABB::intersect / intersect_t (boundingbox.rs:97-131):
//   t0 = (min - o) * inv, t1 = (max - o) * inv;  t_small = min(max(t0, EPS), max(t1, EPS));  t_big = max(min(t0, t_max), min(t1, t_max));
//   hit iff max_element(t_small) <= min_element(t_big), t_enter = max_element(t_small)      (glam min/max = SSE selects: b wins on NaN)
// evaluated with half the min/max work by picking, per axis, the plane the ray reaches first.  Subtraction and the multiply by
// inv are monotone, so for inv >= 0 (incl. +inf) t0 <= t1 and for inv < 0 (incl. -inf) t1 <= t0 whenever both are numbers; then
// t_small = max(t_near, EPS) and t_big = min(t_far, t_max) exactly.  A NaN arises only as 0 * inf (origin on the plane, zero
// direction component): the reference's selects turn that axis into (EPS, t_max), i.e. no constraint, and so do IEEE
// maxNum/minNum (v_max3_f32/v_min3_f32), which drop a NaN operand.  If both planes give NaN the axis is unconstrained on both
// sides as well.  Zero signs cannot reach the result (t_enter >= EPS; t_big is only compared).  Requires t_max not NaN (a NaN
// t_max fails every reference box test; call sites handle it).
__device__ __forceinline__ bool slab(const uint4 w0, const uint4 w1, const f3 o, const f3 inv, const float t_max, float& t_enter)
{
    const bool nx = inv.x < 0.0f, ny = inv.y < 0.0f, nz = inv.z < 0.0f;
    // (near, far) pairs: one v_pk_add_f32 + one v_pk_mul_f32 per axis
    typedef float pair_t __attribute__((ext_vector_type(2)));
    const pair_t px = (pair_t{asf(nx ? w1.x : w0.x), asf(nx ? w0.x : w1.x)} - pair_t{o.x, o.x}) * pair_t{inv.x, inv.x};
    const pair_t py = (pair_t{asf(ny ? w1.y : w0.y), asf(ny ? w0.y : w1.y)} - pair_t{o.y, o.y}) * pair_t{inv.y, inv.y};
    const pair_t pz = (pair_t{asf(nz ? w1.z : w0.z), asf(nz ? w0.z : w1.z)} - pair_t{o.z, o.z}) * pair_t{inv.z, inv.z};
    const float tnx = px.x, tfx = px.y, tny = py.x, tfy = py.y, tnz = pz.x, tfz = pz.y;
    const float ts = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), PT_EPSILON);
    const float tb = fminf(fminf(fminf(tfx, tfy), tfz), t_max);
    t_enter = ts;
    return ts <= tb;
}

__device__ __forceinline__ bool sign_differs(float a, float b) // a.signum() != b.signum()
{
    return __builtin_isunordered(a, b) || (((asu(a) ^ asu(b)) >> 31) != 0u);
}

// Triangle::intersect_naive on the pre-translated origin (primitive.rs:117-155)
__device__ __forceinline__ bool tri_planes(const uint4 p0, const uint4 p1, const uint4 p2, const f3 o, const f3 d, const float t_max,
                                           const float t_est, float& td, float& ud, float& vd, float& det)
{
    const f3 mo = fma3(d, bc3(t_est), o); // ray.at(t_estimate)
    const float t_min = PT_EPSILON - t_est, t_mx = t_max - t_est;
    const f4 n0{asf(p0.x), asf(p0.y), asf(p0.z), asf(p0.w)};
    det = dot3(d, xyz(n0));
    td = -dot4(f4{mo.x, mo.y, mo.z, -1.0f}, n0);
    const bool out_t = sign_differs(td - det * t_min, det * t_mx - td);
    const f3 p = det * mo + td * d;
    const f4 p4{p.x, p.y, p.z, det};
    ud = dot4(p4, f4{asf(p1.x), asf(p1.y), asf(p1.z), asf(p1.w)});
    const bool out_u = sign_differs(ud, det - ud);
    vd = dot4(p4, f4{asf(p2.x), asf(p2.y), asf(p2.z), asf(p2.w)});
    const bool out_v = sign_differs(vd, det - ud - vd);
    // the three rejections of primitive.rs:122-140 without early exits: the traversal loop is more sensitive to exec-mask operations
    // than to the ~25 VALU operations a rejected triangle would have skipped (same-box A/B: -0.9 ms per frame)
    return !(out_t | out_u | out_v);
}

// the same test in two parts, for leaves that evaluate two triangles side by side: everything that does not depend on t_max ...
struct TriEval { float td, ud, vd, det; bool uv_ok; };
__device__ __forceinline__ TriEval tri_eval(const uint4* tp, const f3 mo, const f3 d)
{
    TriEval e;
    const uint4 p0 = tp[0], p1 = tp[1], p2 = tp[2];
    const f4 n0{asf(p0.x), asf(p0.y), asf(p0.z), asf(p0.w)};
    e.det = dot3(d, xyz(n0));
    e.td = -dot4(f4{mo.x, mo.y, mo.z, -1.0f}, n0);
    const f3 p = e.det * mo + e.td * d;
    const f4 p4{p.x, p.y, p.z, e.det};
    e.ud = dot4(p4, f4{asf(p1.x), asf(p1.y), asf(p1.z), asf(p1.w)});
    e.vd = dot4(p4, f4{asf(p2.x), asf(p2.y), asf(p2.z), asf(p2.w)});
    const bool out_u = sign_differs(e.ud, e.det - e.ud), out_v = sign_differs(e.vd, e.det - e.ud - e.vd);
    e.uv_ok = !out_u && !out_v;
    return e;
}
// ... and the range test against the current t_max (primitive.rs:122-123)
__device__ __forceinline__ bool tri_in_range(const TriEval& e, float t_min, float t_mx) { return !sign_differs(e.td - e.det * t_min, e.det * t_mx - e.td); }

struct Blob
{
    const uint4* nodes; // 2 words per node
    const uint4* tris;  // 3 words per triangle
    const uint4* inst;  // INST_WORDS words per instance
    const uint2* leaves; // big-leaf table {first, count} (NODE_TRIS_BIG)
};
// triangles of a leaf link
__device__ __forceinline__ void leaf_range(const Blob& bl, uint32_t kind, uint32_t payload, uint32_t& first, uint32_t& count)
{
    if (kind == NODE_TRIS) { first = payload & LEAF_FIRST_MASK; count = (payload >> LEAF_FIRST_BITS) + 1u; }
    else { const uint2 lf = bl.leaves[payload]; first = lf.x; count = lf.y; }
}

struct LaneRay { f3 o, d, inv; };

// Ray::transform(inv_matrix)  ray.rs:22-28
//
// Identity instances (every Cornell model) take a shortcut that is bit-identical to the full arithmetic.  glam's
// inverse of the identity has matrix3 = I (+0 zeros) and translation = -0, so for a finite vector v
//   ((1*vx + 0*vy) + 0*vz) [+ -0]  ==  vx                      when vx != 0
//                                  ==  zero signed by sign(vx) & sign(vy) & sign(vz)   when vx == +-0
// (a sum of zeros is -0 only if every addend is -0); 1/v'x is then the world-space reciprocal or +-inf.
//
// `root0` / `root1`: the instance record's copy of the BLAS root node (DInstance::root_node).  EAGER (BVH in global memory): the six
// words a visit needs — matrix rows, meta, root node — are loaded TOGETHER, one memory round trip instead of three dependent ones
// (meta -> rows; meta.root -> root node), and pinned so that the compiler cannot sink the row loads into the branch that uses them.
__device__ __forceinline__ void pin(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
template <bool EAGER, bool ROOT_BOX>
__device__ __forceinline__ LaneRay to_object(const Blob& bl, uint32_t inst, const LaneRay& w, bool ray_finite, uint4& root0, uint4& root1)
{
    const uint4* ip = bl.inst + INST_WORDS * inst;
    uint4 r0, r1, r2;
    if (EAGER)
    {
        r0 = ip[0]; r1 = ip[1]; r2 = ip[2];
    }
    const uint4 meta = ip[INST_META_WORD];
    if (ROOT_BOX) { root0 = ip[INST_ROOT_WORD]; root1 = ip[INST_ROOT_WORD + 1u]; }
    else root0.w = reinterpret_cast<const uint32_t*>(ip + INST_ROOT_WORD)[3];
    if (EAGER) { pin(r0); pin(r1); pin(r2); }
    LaneRay r;
    if ((meta.w & INSTANCE_IDENTITY) != 0u && ray_finite)
    {
        const uint32_t so = asu(w.o.x) & asu(w.o.y) & asu(w.o.z) & 0x80000000u;
        const uint32_t sd = asu(w.d.x) & asu(w.d.y) & asu(w.d.z) & 0x80000000u;
        r.o.x = w.o.x != 0.0f ? w.o.x : asf(so);
        r.o.y = w.o.y != 0.0f ? w.o.y : asf(so);
        r.o.z = w.o.z != 0.0f ? w.o.z : asf(so);
        r.d.x = w.d.x != 0.0f ? w.d.x : asf(sd);
        r.d.y = w.d.y != 0.0f ? w.d.y : asf(sd);
        r.d.z = w.d.z != 0.0f ? w.d.z : asf(sd);
        r.inv.x = w.d.x != 0.0f ? w.inv.x : asf(sd | 0x7f800000u);
        r.inv.y = w.d.y != 0.0f ? w.inv.y : asf(sd | 0x7f800000u);
        r.inv.z = w.d.z != 0.0f ? w.inv.z : asf(sd | 0x7f800000u);
        return r;
    }
    if (!EAGER) { r0 = ip[0]; r1 = ip[1]; r2 = ip[2]; }
    r.o.x = ((asf(r0.x) * w.o.x + asf(r0.y) * w.o.y) + asf(r0.z) * w.o.z) + asf(r0.w);
    r.o.y = ((asf(r1.x) * w.o.x + asf(r1.y) * w.o.y) + asf(r1.z) * w.o.z) + asf(r1.w);
    r.o.z = ((asf(r2.x) * w.o.x + asf(r2.y) * w.o.y) + asf(r2.z) * w.o.z) + asf(r2.w);
    r.d.x = (asf(r0.x) * w.d.x + asf(r0.y) * w.d.y) + asf(r0.z) * w.d.z;
    r.d.y = (asf(r1.x) * w.d.x + asf(r1.y) * w.d.y) + asf(r1.z) * w.d.z;
    r.d.z = (asf(r2.x) * w.d.x + asf(r2.y) * w.d.y) + asf(r2.z) * w.d.z;
    r.inv = rcp3(r.d);
    return r;
}

// Identity-only TLAS (IDENT kernels, SceneView::ident_tlas): every instance the walk can meet is an identity instance, so the object ray
// is the same function of the world ray everywhere, and the walk keeps ONE ray per lane for TLAS boxes, BLAS boxes and triangles:
// o and d are to_object's identity image (bit-exact, triangles see what they see today), inv is the WORLD ray's reciprocal.  An
// instance visit is then "note the instance, continue at its BLAS root"; no matrix, no in_blas / blas_base, no per-level select.
//   TLAS boxes: slab(box, o', inv) == slab(box, o, inv).  o' differs from o only in the sign of a zero component; (m - o) then
//     differs only in the sign of a zero, times inv only in the sign of a zero (or is NaN in both: 0 * inf).  A zero t can never be
//     t_enter (max with EPS > 0), and a zero far bound fails `ts <= tb` whatever its sign: the hit bit and t_enter agree.
//   BLAS boxes: the reference uses 1/d' (to_object: +-inf signed like d' where d is +-0), here 1/d (signed like d).  They differ
//     only on an axis c with d_c = +-0, and only when o_c lies outside the box's slab on c: one sign gives the empty interval
//     (-inf, -inf) (a miss), the other (+inf, +inf), a hit only with t_enter = +inf.  Every box under that one lies outside on c too
//     (a BVH node's box encloses its children's), so every triangle under it is tested at t_estimate = +inf, where
//     ray.at(t_estimate) has the coordinate d_c * inf + o_c = NaN and tri_planes / tri_eval reject it.  A subtree entered at +inf
//     therefore accepts nothing, and the triangles that can be accepted are met in the same order with the same t_estimate: same
//     answer.  (The BLAS root itself, entered at t = 0 with no box test by the closest-hit walk, sees the exact o', d'.)  The
//     other choice, 1/d' also on TLAS boxes, would not be exact: it can enter an instance the reference skips, and that instance's
//     root leaf is tested at t = 0.
//   Non-finite rays (a component of o or d inf or NaN): to_object's full arithmetic multiplies it by a zero of the inverse
//     matrix, so o' or d' carries a NaN in some component, and so does ray.at(t) for every t: no triangle of an identity
//     instance is ever accepted.  IDENT walks retire such a ray at set-up with the answer "nothing hit" (closest: MISS_ID,
//     t = inf; any: not occluded).
__device__ __forceinline__ LaneRay ident_ray(const LaneRay& w)
{
    const uint32_t so = asu(w.o.x) & asu(w.o.y) & asu(w.o.z) & 0x80000000u;
    const uint32_t sd = asu(w.d.x) & asu(w.d.y) & asu(w.d.z) & 0x80000000u;
    LaneRay r;
    r.o.x = w.o.x != 0.0f ? w.o.x : asf(so);
    r.o.y = w.o.y != 0.0f ? w.o.y : asf(so);
    r.o.z = w.o.z != 0.0f ? w.o.z : asf(so);
    r.d.x = w.d.x != 0.0f ? w.d.x : asf(sd);
    r.d.y = w.d.y != 0.0f ? w.d.y : asf(sd);
    r.d.z = w.d.z != 0.0f ? w.d.z : asf(sd);
    r.inv = w.inv;
    return r;
}
// the world ray's six sign bits (o.xyz in bits 0-2, d.xyz in bits 3-5): with them ident_ray's o and d give back the world ray exactly
__device__ __forceinline__ uint32_t ray_signs(const LaneRay& w)
{
    return (asu(w.o.x) >> 31) | ((asu(w.o.y) >> 31) << 1) | ((asu(w.o.z) >> 31) << 2) |
           ((asu(w.d.x) >> 31) << 3) | ((asu(w.d.y) >> 31) << 4) | ((asu(w.d.z) >> 31) << 5);
}
__device__ __forceinline__ f3 with_signs(const f3 v, uint32_t bits)
{
    return f3{asf((asu(v.x) & 0x7fffffffu) | ((bits & 1u) << 31)), asf((asu(v.y) & 0x7fffffffu) | (((bits >> 1) & 1u) << 31)),
              asf((asu(v.z) & 0x7fffffffu) | (((bits >> 2) & 1u) << 31))};
}

// the scene's tables in a blob that starts at `base` (global memory, or its copy in LDS)
__device__ __forceinline__ Blob blob_at(const SceneView& sv, const uint4* base)
{
    Blob b;
    b.nodes = base;
    b.tris = base + 2u * sv.n_nodes;
    b.inst = base + 2u * sv.n_nodes + 3u * sv.n_tris;
    b.leaves = reinterpret_cast<const uint2*>(base + 2u * sv.n_nodes + 3u * sv.n_tris + INST_WORDS * sv.n_instances);
    return b;
}
template <bool LDS_SCENE>
__device__ __forceinline__ Blob stage_scene(const SceneView& sv, const uint4* __restrict__ gblob, uint4* smem, uint32_t& words)
{
    const uint4* base = gblob;
    words = 0;
    if (LDS_SCENE)
    {
        words = sv.blob_bytes >> 4;
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) smem[i] = gblob[i];
        __syncthreads();
        base = smem;
    }
    return blob_at(sv, base);
}

// CLOSEST_PRIMARY = CLOSEST_WORLD for bounce 0: every ray starts at the eye (only directions are stored, ray index == path id)
// and a miss ends the path on the spot (integrator.rs:263-266 with accumulated = 0, path_weight = 1).
// CLOSEST_PRIMARY_LENS = CLOSEST_PRIMARY under a thin lens (pt_set_lens): the camera rays' origins are read from the queue like any
// bounce's and go into the shade records (ShadeQueue::c), since no two of them start at the same point.
// CLOSEST_WORLD_EMTEX = CLOSEST_WORLD of a scene with an emission texture (pt_set_material_emission_texture): a path that ends at a light
// is NOT finished here, where the emitted colour of the hit point cannot be looked up, but goes to the terminal queue with its hit record
// (k_shade_terminal<LENS, TexView>); a miss is finished here as ever.
enum { CLOSEST_WORLD = 0, CLOSEST_LIGHTS = 1, CLOSEST_HOOK = 2, CLOSEST_PRIMARY = 3, CLOSEST_PRIMARY_LENS = 4, CLOSEST_WORLD_EMTEX = 5, CLOSEST_MODES = 6 };
constexpr bool closest_is_primary(int mode) { return mode == CLOSEST_PRIMARY || mode == CLOSEST_PRIMARY_LENS; }
constexpr bool closest_is_world(int mode) { return mode == CLOSEST_WORLD || mode == CLOSEST_WORLD_EMTEX; }

struct ClosestOut
{
    f4* hits;              // HOOK: dense by ray index; WORLD/PRIMARY: only rays whose path goes to the terminal queue; LIGHTS: by ray index (slot)
    f4* q_base;            // surface classes' hit records in queue order: see WavefrontBuffers::q_shade_base
    uint32_t q_stride, q_class_slot;
    uint2* q_term;         // terminal queue entries {ray index, path id}
    uint32_t* n_shade;     // counters row: n_shade[Q_COUNT]
    uint4* wave_times;     // PT_WAVE_TIMES builds: [kWaveTimeSlots] records of this launch, else unused
    uint32_t* tails;       // the row's striped tails [Q_COUNT][kTailWordsPerQueue] (surface classes; the terminal queue keeps n_shade[Q_TERMINAL])
    uint32_t cap_shade, cap_term; // queue capacities (slots)
    uint32_t class_mask;   // shade classes present in the scene (bit Q_TERMINAL always set)
    uint32_t* overflow;    // batch-wide "a queue was full" flag
    // CLOSEST_LIGHTS (fused NEE chain): world root for the follow-up any-hit, result codes by path id
    uint32_t world_root;
    uint8_t* occl;
    // CLOSEST_PRIMARY (eye: not CLOSEST_PRIMARY_LENS)
    f3 eye;
    f4* radiance;
    f4* first_pos;
    uint32_t* first_id;
    // environment-map builds of the frame only (a primary miss is then shaded by the terminal pass, but its id / position defaults are written here):
    // how a path id splits into (sample, pixel) — RenderParams::blk_* — and from which batch-local sample on id / position are kept
    uint32_t keep_s_id, keep_s_pos, blk_log, n_blk, blk_last, act_pixels;
    FastDiv div_blk_paths, div_blk_last;
    uint32_t finalize_miss;               // 0 when an environment map is set: misses then go to the terminal queue like any bounce
    // CLOSEST_WORLD: paths that end at this hit or miss are finished here
    const DPathRec* rec;
    uint32_t enable_nee;
};

// Per-lane traversal stack of (node, t_enter) entries.  The position `sp` is opaque to the traversal loop:
//  * Stack8<false> (the whole stack fits the LDS budget): sp IS the entry's byte offset inside the workgroup's dynamic LDS, so a push
//    or pop is one ds_write_b64 / ds_read_b64 with no address arithmetic beyond the add that moves sp;
//  * Stack8<true> (BVH deeper than PT_STACK_LDS_LEVELS): sp is the level; the deepest levels live in global memory
//    ([level][global lane], coalesced) so that occupancy does not collapse.  LDS and global accesses stay separate instructions
//    (no flat addressing).
template <bool SPILL>
struct Stack8;
template <>
struct Stack8<false>
{
    char* base;             // start of dynamic LDS
    uint32_t bottom, step;  // this lane's level-0 offset; bytes per level (8 * blockDim.x)
    __device__ __forceinline__ static Stack8 make(uint4* smem, uint32_t blob_words, const SceneView&)
    {
        return Stack8{reinterpret_cast<char*>(smem), blob_words * 16u + threadIdx.x * 8u, blockDim.x * 8u};
    }
    __device__ __forceinline__ uint32_t empty() const { return bottom; }
    __device__ __forceinline__ uint32_t up(uint32_t sp) const { return sp + step; }
    __device__ __forceinline__ uint32_t down(uint32_t sp) const { return sp - step; }
    __device__ __forceinline__ uint2 get(uint32_t sp) const { return *reinterpret_cast<const uint2*>(base + sp); }
    __device__ __forceinline__ void put(uint32_t sp, uint2 v) const { *reinterpret_cast<uint2*>(base + sp) = v; }
};
template <>
struct Stack8<true>
{
    uint2* lds;
    uint2* spill;
    uint32_t stride, lds_levels, spill_stride;
    __device__ __forceinline__ static Stack8 make(uint4* smem, uint32_t blob_words, const SceneView& sv)
    {
        return Stack8{reinterpret_cast<uint2*>(smem + blob_words) + threadIdx.x,
                      reinterpret_cast<uint2*>(sv.stack_spill) + (blockIdx.x * blockDim.x + threadIdx.x), blockDim.x, sv.stack_lds, gridDim.x * blockDim.x};
    }
    __device__ __forceinline__ uint32_t empty() const { return 0u; }
    __device__ __forceinline__ uint32_t up(uint32_t sp) const { return sp + 1u; }
    __device__ __forceinline__ uint32_t down(uint32_t sp) const { return sp - 1u; }
    __device__ __forceinline__ uint2 get(uint32_t sp) const
    {
        uint2 v;
        if (sp < lds_levels) v = lds[__umul24(sp, stride)];
        else v = spill[(size_t)(sp - lds_levels) * spill_stride];
        return v;
    }
    __device__ __forceinline__ void put(uint32_t sp, uint2 v) const
    {
        if (sp < lds_levels) lds[__umul24(sp, stride)] = v;
        else spill[(size_t)(sp - lds_levels) * spill_stride] = v;
    }
};

// ---- diagnostics of variant builds: the members are empty when the macro is 0
// PT_STEP_STATS: per traversal step, how many lanes take each section.  Words 8..15 of the launch's cursor lines (tools/step_stats.py,
// pt_last_batch_step_stats): wave-steps executed, lanes active in them, lanes taking the instance / branch / leaf section, and (words
// 13..15) wave-steps in which at least one lane took that section.
struct StepStats
{
    enum { INST = 0, BRANCH = 1, LEAF = 2 };
#if PT_STEP_STATS
    uint32_t iter = 0, lanes = 0, lane[3] = {0u, 0u, 0u}, wave[3] = {0u, 0u, 0u};
#endif
    // the wave starts a step (every lane calls this)
    __device__ __forceinline__ void step(bool active)
    {
#if PT_STEP_STATS
        const uint64_t am = __ballot(active);
        if (am != 0ull) { iter += 1u; lanes += (uint32_t)__popcll(am); }
#endif
    }
    // the lanes that reach section s of the step: x = this lane takes it
    __device__ __forceinline__ void section(int s, bool x)
    {
#if PT_STEP_STATS
        const uint64_t m = __ballot(x);
        lane[s] += x ? 1u : 0u;
        if (m != 0ull && lane_id() == (uint32_t)__builtin_ctzll(m)) wave[s] += 1u;
#endif
    }
    __device__ __forceinline__ void flush(uint32_t* heads) const
    {
#if PT_STEP_STATS
        const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        uint32_t* line = heads + ((w * 7u) & (kQueueHeads - 1u)) * kHeadStrideWords;
        if (lane_id() == 0u) { atomicAdd(line + 8, iter); atomicAdd(line + 9, lanes); }
        uint32_t a = lane[0], b = lane[1], c = lane[2];
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); c += __shfl_xor(c, off); }
        if (lane_id() == 0u) { atomicAdd(line + 10, a); atomicAdd(line + 11, b); atomicAdd(line + 12, c); }
        a = wave[0]; b = wave[1]; c = wave[2];
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); c += __shfl_xor(c, off); }
        if (lane_id() == 0u) { atomicAdd(line + 13, a); atomicAdd(line + 14, b); atomicAdd(line + 15, c); }
#endif
    }
};
// PT_WAVE_TIMES: one record per wave (100 MHz ticks, low 32 bits): start, first rays, queue found empty, end; the host reduces them
// (pt_last_batch_step_stats, tools/wave_times.py)
struct WaveTimes
{
#if PT_WAVE_TIMES
    uint32_t start = (uint32_t)wall_clock64(), first = 0u, drained = 0u;
#endif
    __device__ __forceinline__ void check_drained(bool no_more)
    {
#if PT_WAVE_TIMES
        if (no_more && drained == 0u) drained = (uint32_t)wall_clock64() | 1u;
#endif
    }
    __device__ __forceinline__ void check_first(uint32_t take)
    {
#if PT_WAVE_TIMES
        if (first == 0u && take != 0u) first = (uint32_t)wall_clock64() | 1u;
#endif
    }
    __device__ __forceinline__ void write(uint4* times)
    {
#if PT_WAVE_TIMES
        if (lane_id() == 0u && times)
        {
            const uint32_t end = (uint32_t)wall_clock64();
            if (drained == 0u) drained = end;
            if (first == 0u) first = start;
            const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
            if (w < kWaveTimeSlots) times[w] = make_uint4(start, first, drained, end | 1u);
        }
#endif
    }
};
#if PT_WAVE_TIMES
__device__ uint4* g_any_times = nullptr; // where the shadow-ray launch in flight puts its per-wave time records (set in-stream by launch_trace_shadow)
#else
constexpr uint4* g_any_times = nullptr;
#endif

// A shadow ray's answer applied to its path: blocked, it erases the path's explicit-light candidate (integrator.rs:55-56,73), so the next
// shading pass needs no visibility word; visible, it leaves it alone.  A path that died in the shading pass with nothing else owed (`ends`)
// has its radiance completed instead: accumulated += path_weight * (explicit + 0), integrator.rs:231-234.  radiance(): where that goes
// (asked for only then).
template <typename Radiance>
__device__ __forceinline__ void apply_shadow(DPathRec* rec, bool ends, bool blocked, Radiance&& radiance)
{
    if (ends)
    {
        const f3 e = blocked ? f3{0.0f, 0.0f, 0.0f} : xyz(rec->nee_e);
        const f3 acc = xyz(rec->acc) + xyz(rec->nee_pw) * (e + f3{0.0f, 0.0f, 0.0f});
        radiance() = f4{acc.x, acc.y, acc.z, 0.0f};
    }
    else if (blocked)
    {
        float* e = reinterpret_cast<float*>(&rec->nee_e);
        e[0] = 0.0f; e[1] = 0.0f; e[2] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------ closest hit
// a traversal kernel's single argument (one struct, so that it starts at offset 0 of the kernel-argument segment)
struct ClosestKArgs
{
    SceneView sv;
    const uint4* gblob;
    const f4* ra;
    const f4* rb;
    const uint32_t* n_ptr;
    uint32_t* heads;
    uint32_t root, cap_in;
    ClosestOut out;
};
typedef const __attribute__((address_space(4))) ClosestKArgs* ClosestKArgsPtr;
typedef const __attribute__((address_space(4))) ClosestOut* ClosestOutPtr;
// (the empty asm keeps the compiler from hoisting the loads made through the pointer out of the section that makes them)
__device__ __forceinline__ ClosestOutPtr launder_args(ClosestOutPtr p)
{
    asm volatile("" : "+s"(p));
    return p;
}
// (the kernel's body as a function of the staged scene: k_closest is one launch of it, k_trace_fused runs it before another)
template <int BVH, int MODE, bool SPILL, bool IDENT>
__device__ __forceinline__ void closest_body(const SceneView& sv, const Blob& bl, const uint32_t blob_words, uint4* smem, const uint32_t root, const f4* __restrict__ ra,
                                             const f4* __restrict__ rb, const uint32_t* __restrict__ n_ptr, const uint32_t cap_in,
                                             uint32_t* __restrict__ heads, const ClosestOutPtr outp)
{
    constexpr bool LDS_SCENE = BVH != 0; // BVH: 0 in global memory, 1 in LDS
    const FetchPlan plan = fetch_plan(min(*n_ptr, cap_in), LDS_SCENE ? (uint32_t)PT_CHUNK_DIV : (uint32_t)PT_CHUNK_DIV_GLOBAL_BVH, (uint32_t)PT_TAPER);
    if (blockIdx.x >= plan.blocks) return; // a short queue keeps only as many workgroups as it has 64-ray chunks
    // per-lane stack of (node, t_enter), [level][thread] in LDS (conflict-free ds_read_b64 / ds_write_b64)
    const Stack8<SPILL> stk = Stack8<SPILL>::make(smem, blob_words, sv);
    const uint32_t prim_bits = sv.prim_bits;

    bool active = false, pending = false, ray_finite = false;
    uint32_t ray_idx = 0, pid = 0;
    LaneRay w{}, ob{};    // IDENT: ob is the lane's only ray (ident_ray); w is rebuilt from it and w_signs when the ray retires
    uint32_t w_signs = 0u;
    float t_max = 0.0f, bt = 0.0f;
    float hud = 0.0f, hvd = 0.0f, hdet = 1.0f; // best hit's (u, v) numerators and determinant: divided once, when the ray retires (primitive.rs:158-160)
    uint32_t bid = MISS_ID, sp = stk.empty(), blas_base = 0, inst = 0;
    bool in_blas = false;
    bool any_phase = false;   // CLOSEST_LIGHTS: the lights-TLAS hit exists, now any-hit against the world (integrator.rs:103)
    uint32_t chain_code = 0u; // 0 light visible, 1 blocked, 2 no light on the ray
    WaveRange wr = first_range(plan, heads);
    // material binning (CLOSEST_WORLD / PRIMARY): a retiring ray's hit record goes straight to its class's shade queue, into a region
    // of that queue this wave has reserved (wave_reserve: one atomic per region, none per entry)
    uint32_t light_hits = 0, valid_rays = 0;
    StepStats ss;
    WaveTimes wt;
    Region bin_region[Q_COUNT];
#pragma unroll
    for (uint32_t c = 0; c < Q_COUNT; ++c) bin_region[c] = Region{0u, 0u};
    // the terminal queue's regions.  Without an environment map its entries are rare (paths that also cast a BSDF-sampled NEE ray): the
    // smallest region a wave can use keeps the queue's extent, and what k_shade_terminal reads, small (whole frame: its first launch
    // 185 -> ~30 us).  With one, every miss goes there: regions sized like any busy queue's.
    // The launch description is read through the kernel-argument segment where it is needed (the service section and the epilogue:
    // s_load, scalar cache) instead of living in scalar registers across the traversal loop, which has none to spare (66 were spilled
    // to vector lanes and read back with v_readlane in every service)
    const uint32_t lights_world_root = MODE == CLOSEST_LIGHTS ? outp->world_root : 0u;
    const uint32_t rsize = outp->finalize_miss != 0u ? 64u : region_size(plan.n, plan.blocks * (blockDim.x >> 6), 64u);
    const Stripes stripes = stripes_for(plan.n);
    uint32_t stripe_rot = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    for (;;)
    {
        uint64_t act = __ballot(active);
        const bool no_more = wr.drained && wr.cur >= wr.end;
        wt.check_drained(no_more);
        const bool service = no_more ? (act == 0ull) : (__popcll(act) <= Refill<LDS_SCENE>::kBelow);
        if (service)
        {
            const ClosestOutPtr out = launder_args(outp);
            // ---- retire finished lanes
            const uint64_t pm = __ballot(pending);
            if (pm != 0ull)
            {
                if (closest_is_world(MODE) || closest_is_primary(MODE))
                {
                    if (IDENT && pending) { w.o = with_signs(ob.o, w_signs); w.d = with_signs(ob.d, w_signs >> 3); } // the world ray, bit-exact
                    uint64_t qm = pm;
                    if (closest_is_primary(MODE))
                    {
                        // a primary miss is a finished path: accumulated = 0 + 0.006 * 1 (integrator.rs:265), defaults of :156-157
                        const bool missed = pending && bid == MISS_ID && out->finalize_miss != 0u;
                        // one byte per camera ray instead of a 16-byte radiance record for the (usually many) rays that leave at once:
                        // k_accumulate reads PRIMARY_MISS as radiance (0.006, 0.006, 0.006)
                        if (pending) out->occl[ray_idx] = missed ? (uint8_t)PRIMARY_MISS : (uint8_t)0u;
                        // (a plain miss leaves nothing else behind: k_accumulate reads PRIMARY_MISS as id 255, position r.at(1e5), integrator.rs:156-157)
                        if (!missed && pending && bid == MISS_ID)
                        {
                            // environment map present: the terminal pass shades the miss; defaults of integrator.rs:156-157 still apply
                            const FastDiv dbp{out->div_blk_paths.magic, out->div_blk_paths.shift, out->div_blk_paths.one, out->div_blk_paths.d};
                            const FastDiv dbl{out->div_blk_last.magic, out->div_blk_last.shift, out->div_blk_last.one, out->div_blk_last.d};
                            const uint32_t b = fastdiv(ray_idx, dbp), rem = ray_idx - b * (out->act_pixels << out->blk_log);
                            const bool short_blk = b + 1u == out->n_blk;
                            const uint32_t k = short_blk ? fastdiv(rem, dbl) : (rem >> out->blk_log);
                            const uint32_t sl = (b << out->blk_log) + (rem - k * (short_blk ? out->blk_last : (1u << out->blk_log)));
                            if (sl >= out->keep_s_id) out->first_id[(sl - out->keep_s_id) * out->act_pixels + k] = 255u;
                            if (sl == out->keep_s_pos)
                            {
                                const f3 far = fma3(w.d, bc3(1e5f), w.o);
                                out->first_pos[k] = f4{far.x, far.y, far.z, 1e5f};
                            }
                        }
                        qm = __ballot(pending && !missed);
                        pending = pending && !missed;
                    }
                    if (closest_is_world(MODE))
                    {
                        // A path that ends here — the ray left the scene (integrator.rs:263-266, no environment map) or found a light
                        // (:207-214) — is finished in this kernel, whose memory pipes are idle, instead of a terminal-queue round trip:
                        // add what the last bounce still owes (explicit-light estimate; a blocked shadow ray has zeroed it), then the
                        // ambient term or the emission.  The rare path that also cast a BSDF-sampled NEE ray goes to the queue as before.
                        bool ends = false, emissive = false;
                        uint32_t mat_id = 0;
                        if (pending)
                        {
                            if (bid == MISS_ID) ends = out->finalize_miss != 0u;
                            else
                            {
                                const uint4 meta = bl.inst[INST_WORDS * (bid >> prim_bits) + INST_META_WORD];
                                emissive = ends = MODE == CLOSEST_WORLD && (meta.w & 0xffu) == (uint32_t)Q_TERMINAL; // (EMTEX: the terminal pass shades a light hit)
                                mat_id = meta.z;
                            }
                        }
                        if (ends)
                        {
                            const DPathRec& rec = out->rec[pid];
                            const f4 acc4 = rec.acc;
                            const uint32_t flags = asu(acc4.w);
                            if (!(flags & FLAG_BSDF_CAST))
                            {
                                f3 acc = xyz(acc4);
                                if (flags & FLAG_NEE_PENDING) acc = acc + xyz(rec.nee_pw) * (xyz(rec.nee_e) + f3{0.0f, 0.0f, 0.0f}); // integrator.rs:231-234
                                const f3 pw = xyz(rec.pw);
                                if (!emissive) acc = acc + f3{0.006f, 0.006f, 0.006f} * pw;
                                else if (!out->enable_nee || (flags & FLAG_LAST_DELTA))
                                {
                                    const DMaterial& m = sv.materials[mat_id];
                                    acc = fma3(f3{m.colour[0], m.colour[1], m.colour[2]}, pw, acc);
                                }
                                out->radiance[pid] = f4{acc.x, acc.y, acc.z, 0.0f};
                                pending = false;
                            }
                        }
                        qm = __ballot(pending);
                    }
                    if (qm != 0ull)
                    {
                        // bin by shade class.  Surface classes get the whole hit record in queue order (the shading pass then reads
                        // linearly and never gathers by ray index); terminal entries stay {ray index, path id} + hits[ray index].
                        uint32_t cls = Q_COUNT;
                        if (pending) cls = bid != MISS_ID ? (bl.inst[INST_WORDS * (bid >> prim_bits) + INST_META_WORD].w & 0xffu) : (uint32_t)Q_TERMINAL;
                        const f4 hit{bt, hud / hdet, hvd / hdet, asf(bid)};
#pragma unroll
                        for (uint32_t c = 0; c < Q_COUNT; ++c)
                        {
                            if (!((out->class_mask >> c) & 1u)) continue;
                            const uint64_t m = __ballot(cls == c);
                            if (m == 0ull) continue;
                            const Placement pl = c == Q_TERMINAL
                                ? wave_reserve(bin_region[c], out->n_shade + c, (uint32_t)__popcll(m), rsize, out->cap_term, out->overflow)
                                : wave_reserve_striped(bin_region[c], out->tails + c * kTailWordsPerQueue, stripes, stripe_rot, (uint32_t)__popcll(m), out->cap_shade, out->overflow);
                            if (cls == c)
                            {
                                const uint32_t pos = place(pl, mbcnt64(m));
                                if (c == Q_TERMINAL)
                                {
                                    out->hits[ray_idx] = hit;
                                    out->q_term[pos] = make_uint2(ray_idx, pid);
                                }
                                else
                                {
                                    f4* const qa = out->q_base + (size_t)(3u * ((out->q_class_slot >> (4u * c)) & 0xfu)) * out->q_stride + pos;
                                    nt_store(qa, f4{w.d.x, w.d.y, w.d.z, asf(pid)});
                                    nt_store(qa + out->q_stride, hit);
                                    if (MODE != CLOSEST_PRIMARY) nt_store(qa + 2u * (size_t)out->q_stride, f4{w.o.x, w.o.y, w.o.z, 0.0f});
                                }
                            }
                        }
                    }
                }
                else if (MODE == CLOSEST_LIGHTS)
                {
                    if (pending)
                    {
                        out->occl[pid] = (uint8_t)chain_code;
                        if (chain_code == 0u) out->hits[ray_idx] = f4{bt, hud / hdet, hvd / hdet, asf(bid)}; // only a visible light is ever read back
                    }
                }
                else
                {
                    if (pending) out->hits[ray_idx] = f4{bt, hud / hdet, hvd / hdet, asf(bid)};
                }
                pending = false;
            }
            if (no_more) break;
            // ---- refill idle lanes from the wave's private range
            const uint64_t idle = ~act;
            uint32_t first;
            const uint32_t take = claim_rays(wr, heads, plan, (uint32_t)__popcll(idle), first);
            const uint32_t rank = mbcnt64(idle);
            if (!active && rank < take)
            {
                const uint32_t mine = first + rank;
                const f4 b = rb[mine];
                ray_idx = mine;
                pid = asu(b.w);
                if (pid != HOLE) {
                valid_rays += 1u;
                if (MODE == CLOSEST_PRIMARY)
                {
                    w.o = f3{out->eye.x, out->eye.y, out->eye.z};
                    t_max = asf(0x7f800000u);
                }
                else
                {
                    const f4 a = ra[mine]; // (asking for both words of the ray together: +-0, and 8 B more scratch at five waves)
                    w.o = xyz(a);
                    t_max = a.w;
                }
                w.d = xyz(b);
                w.inv = rcp3(w.d);
                ray_finite = finite3(w.o) && finite3(w.d);
                if (IDENT) { ob = ident_ray(w); w_signs = ray_signs(w); }
                bid = MISS_ID;
                any_phase = false;
                chain_code = 2u;
                bt = asf(0x7f800000u);
                hud = 0.0f;
                hvd = 0.0f;
                hdet = 1.0f;
                in_blas = false;
                sp = stk.empty();
                // TLAS::intersect: root box test, then (root, 0.0)   tlas.rs:68-74
                float te;
                const uint4 root0 = bl.nodes[2u * root];
                // (IDENT: a non-finite ray can hit nothing, see ident_ray)
                const bool ok = (t_max == t_max) && (!IDENT || ray_finite) && slab(root0, bl.nodes[2u * root + 1u], IDENT ? ob.o : w.o, w.inv, t_max, te);
                if (ok)
                {
                    stk.put(sp, make_uint2(root0.w, 0u));    // entries are (link, t_enter); the root goes in with t_enter 0
                    sp = stk.up(sp);
                    active = true;
                }
                else { pending = true; }
                } // not a hole
            }
            wt.check_first(take);
            act = __ballot(active);
            if (act == 0ull) continue; // retires the lanes that missed the root box, then refills again or exits
            // the wave's chunk ended inside this refill: go round again at once for the next chunk instead of stepping with idle lanes
            if (PT_RESERVICE && take < (uint32_t)__popcll(idle) && !wr.drained && (uint32_t)__popcll(act) <= (uint32_t)Refill<LDS_SCENE>::kBelow) continue;
        }

#pragma unroll 1
        for (int it = 0; it < Refill<LDS_SCENE>::kSteps; ++it)
        {
            ss.step(active);
            if (!active) continue;
            if (!IDENT && in_blas && sp == blas_base) in_blas = false; // BLAS::intersect returned  blas.rs:255
            if (MODE == CLOSEST_LIGHTS && any_phase)
            {
                // TLAS::any_intersect on the world with t_max = light_t * (1 - EPS)   tlas.rs:111-144, blas.rs:257-294; entries are
                // (link, entry distance) of nodes whose box was already met, as in k_any
                if (sp == stk.empty()) { active = false; pending = true; chain_code = 0u; continue; }
                sp = stk.down(sp);
                const uint2 e = stk.get(sp);
                uint32_t link = e.x;
                float t_enter = asf(e.y);
                if ((link >> NODE_KIND_SHIFT) == NODE_INSTANCE)
                {
                    uint4 r0, r1;
                    if (IDENT)
                    {
                        const uint4* ip = bl.inst + INST_WORDS * (link & NODE_PAYLOAD_MASK) + INST_ROOT_WORD;
                        r0 = ip[0]; r1 = ip[1];
                    }
                    else
                    {
                        ob = to_object<!LDS_SCENE, true>(bl, link & NODE_PAYLOAD_MASK, w, ray_finite, r0, r1);
                        in_blas = true;
                        blas_base = sp;
                    }
                    if (!slab(r0, r1, ob.o, ob.inv, t_max, t_enter)) continue;
                    link = r0.w;
                }
                const uint32_t kkind = link >> NODE_KIND_SHIFT, kpay = link & NODE_PAYLOAD_MASK;
                if (kkind == NODE_BRANCH)
                {
                    const uint4* cp = bl.nodes + 2u * kpay;
                    const uint4 l0 = cp[0], l1 = cp[1], r0 = cp[2], r1 = cp[3];
                    const f3 so = (IDENT || in_blas) ? ob.o : w.o, sinv = (IDENT || in_blas) ? ob.inv : w.inv;
                    float tl, tr;
                    const bool hl = slab(l0, l1, so, sinv, t_max, tl);
                    const bool hr = slab(r0, r1, so, sinv, t_max, tr);
                    if (hl) { stk.put(sp, make_uint2(l0.w, asu(tl))); sp = stk.up(sp); }
                    if (hr) { stk.put(sp, make_uint2(r0.w, asu(tr))); sp = stk.up(sp); }
                }
                else
                {
                    uint32_t first, count;
                    leaf_range(bl, kkind, kpay, first, count);
                    for (uint32_t k = 0; k < count; ++k)
                    {
                        const uint4* tp = bl.tris + 3u * (first + k);
                        float td, ud, vd, det;
                        if (tri_planes(tp[0], tp[1], tp[2], ob.o, ob.d, t_max, t_enter, td, ud, vd, det))
                        {
                            active = false;
                            pending = true;
                            chain_code = 1u;
                            break;
                        }
                    }
                }
                continue;
            }
            if (sp == stk.empty())
            {
                if (MODE == CLOSEST_LIGHTS && bid != MISS_ID)
                {
                    // integrator.rs:100-103: the light was hit; the same ray now asks the world for any blocker before it
                    light_hits += 1u;
                    any_phase = true;
                    in_blas = false;
                    t_max = bt * (1.0f - PT_EPSILON);
                    float te = 0.0f;
                    const uint4 wr0 = bl.nodes[2u * lights_world_root];
                    // NaN t_max: every box test fails -> visible; so does a ray that misses the world's root box (tlas.rs:118-121)
                    if (t_max == t_max && slab(wr0, bl.nodes[2u * lights_world_root + 1u], IDENT ? ob.o : w.o, IDENT ? ob.inv : w.inv, t_max, te)) { stk.put(sp, make_uint2(wr0.w, asu(te))); sp = stk.up(sp); }
                    else { active = false; pending = true; chain_code = 0u; }
                    continue;
                }
                active = false;
                pending = true;
                continue;
            }
            sp = stk.down(sp);
            const uint2 e = stk.get(sp);
            if (asf(e.y) > t_max) continue;                  // tlas.rs:80-83 / blas.rs:222-225
            uint32_t link = e.x;
            float t_est = asf(e.y);
            ss.section(StepStats::INST, (link >> NODE_KIND_SHIFT) == NODE_INSTANCE);
            if ((link >> NODE_KIND_SHIFT) == NODE_INSTANCE)
            {
                // TLAS leaf: transform the ray, run the BLAS with the current t_max  tlas.rs:88-99.  BLAS::intersect pushes its root
                // with t_enter = 0 and no box test (blas.rs:217) and pops it at once: that pop happens here, in the same step.
                uint4 root0, root1;
                inst = link & NODE_PAYLOAD_MASK;
                if (IDENT) root0.w = reinterpret_cast<const uint32_t*>(bl.inst + INST_WORDS * inst + INST_ROOT_WORD)[3];
                else
                {
                    ob = to_object<!LDS_SCENE, false>(bl, inst, w, ray_finite, root0, root1);
                    in_blas = true;
                    blas_base = sp;
                }
                if (0.0f > t_max) continue;                  // the root's pop test  blas.rs:222-225
                link = root0.w;
                t_est = 0.0f;
            }
            uint32_t kind = link >> NODE_KIND_SHIFT, payload = link & NODE_PAYLOAD_MASK;
            ss.section(StepStats::BRANCH, kind == NODE_BRANCH);
            // push_to_stack  blas.rs:133-162.  A near child that is itself a branch is expanded in the SAME step (up to PT_BRANCH_LEVELS
            // levels) instead of going through the stack: the kernel pays per wave-step far more than per section of a step
            // (profiles/r02_step_stats_cornell.md), and the reference would pop exactly that child next (its pop test t_enter > t_max
            // cannot fire: the box was just met within t_max).
#pragma unroll 1
            for (int lvl = 0; lvl < PT_BRANCH_LEVELS && kind == NODE_BRANCH; ++lvl)
            {
                const uint4* cp = bl.nodes + 2u * payload; // the children are one contiguous 64-byte record pair
                const uint4 l0 = cp[0], l1 = cp[1], r0 = cp[2], r1 = cp[3];
                const f3 o = (IDENT || in_blas) ? ob.o : w.o, inv = (IDENT || in_blas) ? ob.inv : w.inv;
                float tl, tr;
                const bool hl = slab(l0, l1, o, inv, t_max, tl);
                const bool hr = slab(r0, r1, o, inv, t_max, tr);
                // both hit: the farther child goes underneath (ties: left underneath, right popped first); one hit: that child
                const bool left_near = tl < tr;
                const uint2 le = make_uint2(l0.w, asu(tl)), re = make_uint2(r0.w, asu(tr));
                if (hl && hr) { stk.put(sp, left_near ? re : le); sp = stk.up(sp); }
                kind = NODE_INSTANCE; // nothing more to do in this step unless the near child says otherwise
                if (hl || hr)
                {
                    // the entry the reference pops next.  A triangle leaf is dealt with in this very step, a branch in the next level of
                    // this loop; an instance (or a branch beyond the last level) goes on the stack
                    const uint2 near = (hl && (left_near || !hr)) ? le : re;
                    const uint32_t nk = near.x >> NODE_KIND_SHIFT;
                    if ((nk & 1u) != 0u || (nk == NODE_BRANCH && lvl + 1 < PT_BRANCH_LEVELS))
                    {
                        kind = nk;
                        payload = near.x & NODE_PAYLOAD_MASK;
                        t_est = asf(near.y);
                    }
                    else { stk.put(sp, near); sp = stk.up(sp); }
                }
            }
            ss.section(StepStats::LEAF, (kind & 1u) != 0u);
            if (kind & 1u)
            {
                uint32_t first, count;
                leaf_range(bl, kind, payload, first, count);
                // blas.rs:230-251, in leaf order, each triangle against the t_max the one before may have lowered.  (Rounds 1-3 evaluated two triangles
                // side by side — -2.2 ms per Cornell frame at four waves per SIMD — which cost 18 VGPRs; without it the kernels fit five waves: round 4.)
                const f3 mo = fma3(ob.d, bc3(t_est), ob.o);  // ray.at(t_estimate)  primitive.rs:150
                const float t_min = PT_EPSILON - t_est;
                auto accept = [&](const TriEval& e, uint32_t tri) {
                    if (e.uv_ok && tri_in_range(e, t_min, t_max - t_est))
                    {
                        // primitive.rs:158-170: (t,u,v) = xyz / det ; t += t_estimate
                        bt = e.td / e.det + t_est;
                        hud = e.ud;
                        hvd = e.vd;
                        hdet = e.det;
                        t_max = bt;                          // a NaN here rejects everything that follows (tri_in_range is unordered)
                        bid = (inst << prim_bits) | tri;
                    }
                };
                for (uint32_t k = 0; k < count; ++k) accept(tri_eval(bl.tris + 3u * (first + k), mo, ob.d), first + k);
                if (bt != bt) { sp = stk.empty(); in_blas = false; } // NaN t_max: nothing else can be accepted anywhere
            }
        }
    }
    if (closest_is_world(MODE) || closest_is_primary(MODE))
    {
        const ClosestOutPtr out = launder_args(outp);
        // hand back what is left of this wave's regions as holes (a hole is a path id of HOLE)
        const f4 hole{0.0f, 0.0f, 0.0f, asf(HOLE)};
        for (uint32_t i = bin_region[Q_TERMINAL].cur + lane_id(); i < bin_region[Q_TERMINAL].end; i += 64u) out->q_term[i] = make_uint2(HOLE, 0u);
#pragma unroll
        for (uint32_t c = 1; c < Q_COUNT; ++c)
        {
            f4* const qa = out->q_base + (size_t)(3u * ((out->q_class_slot >> (4u * c)) & 0xfu)) * out->q_stride;
            for (uint32_t i = bin_region[c].cur + lane_id(); i < bin_region[c].end; i += 64u) qa[i] = hole;
        }
    }
    wt.write(outp->wave_times);
    ss.flush(heads);
    if (MODE != CLOSEST_HOOK) add_tally(heads, valid_rays, HEAD_TALLY0);
    // any-hit casts of integrator.rs:103
    if (MODE == CLOSEST_LIGHTS) add_tally(heads, light_hits, HEAD_TALLY1);
}
template <int BVH, int MODE, bool SPILL, bool IDENT = false>
__global__ void __launch_bounds__(256, BVH != 0 ? PT_WAVES_LDS_BVH : PT_WAVES_GLOBAL_BVH) k_closest(const ClosestKArgs a)
{
    constexpr bool LDS_SCENE = BVH != 0;
    extern __shared__ uint4 smem[];
    // (workgroups the queue has no 64-ray chunk for leave before staging anything)
    if (blockIdx.x >= fetch_plan(min(*a.n_ptr, a.cap_in), LDS_SCENE ? (uint32_t)PT_CHUNK_DIV : (uint32_t)PT_CHUNK_DIV_GLOBAL_BVH, (uint32_t)PT_TAPER).blocks) return;
    uint32_t blob_words;
    const Blob bl = stage_scene<LDS_SCENE>(a.sv, a.gblob, smem, blob_words);
    const ClosestOutPtr outp = &((ClosestKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr())->out;
    closest_body<BVH, MODE, SPILL, IDENT>(a.sv, bl, blob_words, smem, a.root, a.ra, a.rb, a.n_ptr, a.cap_in, a.heads, outp);
}

// ------------------------------------------------------------------------------------------------ any hit
enum { ANY_SHADOW = 0, ANY_HOOK = 2, ANY_MODES = 3 };

// TLAS::any_intersect / BLAS::any_intersect (tlas.rs:111-144, blas.rs:257-294) pop a node, test ITS box and push both children
// untested.  The answer is a disjunction over the triangles of every leaf whose box the ray meets, each tested with that
// box's own entry distance, so neither the visiting order nor the moment a box is tested can change it.  Here a node's box is
// tested when its parent is expanded (the instance's BLAS root right after the ray transform) and only nodes that were hit go
// on the stack, with their entry distance: a missed child costs a slab test instead of a full traversal step.
template <int BVH, int MODE, bool SPILL, bool IDENT>
__device__ __forceinline__ void any_body(const SceneView& sv, const Blob& bl, const uint32_t blob_words, uint4* smem, const uint32_t root, const f4* __restrict__ ra,
                                         const f4* __restrict__ rb, const uint32_t* __restrict__ n_ptr, const uint32_t cap_in,
                                         uint32_t* __restrict__ heads, uint32_t* __restrict__ occluded,
                                         f4* __restrict__ radiance)
{
    constexpr bool LDS_SCENE = BVH != 0; // BVH: 0 in global memory, 1 in LDS
    const FetchPlan plan = fetch_plan(min(*n_ptr, cap_in), LDS_SCENE ? (uint32_t)PT_CHUNK_DIV : (uint32_t)PT_CHUNK_DIV_GLOBAL_BVH, (uint32_t)PT_TAPER_ANY);
    if (blockIdx.x >= plan.blocks) return;
    const Stack8<SPILL> stk = Stack8<SPILL>::make(smem, blob_words, sv); // entries (node, entry distance of its box)

    bool active = false, ray_finite = false;
    uint32_t out_idx = 0, valid_rays = 0;
    LaneRay w{}, ob{};
    float t_max = 0.0f;
    uint32_t sp = stk.empty(), blas_base = 0;
    // ANY_SHADOW: `occluded` is PathState::rec, and a shadow ray whose path id carries PATH_ENDS completes its path (apply_shadow);
    // ANY_HOOK: one word per ray
    bool path_ends = false;
    auto put_result_at = [&](uint32_t idx, bool ends, uint32_t v) {
        if (MODE == ANY_SHADOW) apply_shadow(reinterpret_cast<DPathRec*>(occluded) + idx, ends, v != 0u, [&]() -> f4& { return radiance[idx]; });
        else occluded[idx] = v;
    };
    auto put_result = [&](uint32_t v) { put_result_at(out_idx, path_ends, v); };
    bool in_blas = false;
    WaveTimes wt;
    StepStats ss;
    WaveRange wr = first_range(plan, heads);

    for (;;)
    {
        uint64_t act = __ballot(active);
        const bool no_more = wr.drained && wr.cur >= wr.end;
        wt.check_drained(no_more);
        const bool service = no_more ? (act == 0ull) : (__popcll(act) <= Refill<LDS_SCENE>::kBelowAny);
        if (service)
        {
            if (no_more) break;
            const uint64_t idle = ~act;
            uint32_t first;
            const uint32_t take = claim_rays(wr, heads, plan, (uint32_t)__popcll(idle), first);
            const uint32_t rank = mbcnt64(idle);
            if (!active && rank < take)
            {
                const uint32_t mine = first + rank;
                const f4 a = ra[mine], b = rb[mine];
                const uint32_t tag = asu(b.w);
                if (tag != HOLE) {
                valid_rays += 1u;
                path_ends = MODE == ANY_SHADOW && (tag & PATH_ENDS) != 0u;
                out_idx = (MODE == ANY_HOOK) ? mine : (tag & ~PATH_ENDS);
                w.o = xyz(a);
                w.d = xyz(b);
                w.inv = rcp3(w.d);
                ray_finite = finite3(w.o) && finite3(w.d);
                if (IDENT) ob = ident_ray(w);
                t_max = a.w;
                in_blas = false;
                sp = stk.empty();
                // the TLAS root's own box (tlas.rs:118-121); a NaN t_max fails every reference box test -> not occluded (and so, with
                // IDENT, does a non-finite ray: ident_ray)
                float te;
                const uint4 root0 = bl.nodes[2u * root];
                const bool ok = (t_max == t_max) && (!IDENT || ray_finite) && slab(root0, bl.nodes[2u * root + 1u], IDENT ? ob.o : w.o, w.inv, t_max, te);
                if (ok)
                {
                    stk.put(sp, make_uint2(root0.w, asu(te)));
                    sp = stk.up(sp);
                    active = true;
                }
                else put_result(0u);
                } // not a hole
            }
            act = __ballot(active);
            if (act == 0ull) continue;
            if (PT_RESERVICE && take < (uint32_t)__popcll(idle) && !wr.drained && (uint32_t)__popcll(act) <= (uint32_t)Refill<LDS_SCENE>::kBelowAny) continue;
        }

#pragma unroll 1
        for (int it = 0; it < Refill<LDS_SCENE>::kStepsAny; ++it)
        {
            ss.step(active);
            if (!active) continue;
            if (!IDENT && in_blas && sp == blas_base) in_blas = false;
            if (sp == stk.empty())
            {
                active = false;
                put_result(0u);
                continue;
            }
            sp = stk.down(sp);
            const uint2 e = stk.get(sp);                     // (link, entry distance) of a node whose box the ray meets
            uint32_t link = e.x;
            float t_enter = asf(e.y);
            ss.section(StepStats::INST, (link >> NODE_KIND_SHIFT) == NODE_INSTANCE);
            if ((link >> NODE_KIND_SHIFT) == NODE_INSTANCE)
            {
                // TLAS leaf: transform the ray; the BLAS root's box is the first thing BLAS::any_intersect tests  blas.rs:262-264
                uint4 r0, r1;
                if (IDENT)
                {
                    const uint4* ip = bl.inst + INST_WORDS * (link & NODE_PAYLOAD_MASK) + INST_ROOT_WORD;
                    r0 = ip[0]; r1 = ip[1];
                }
                else
                {
                    ob = to_object<!LDS_SCENE, true>(bl, link & NODE_PAYLOAD_MASK, w, ray_finite, r0, r1);
                    in_blas = true;
                    blas_base = sp;
                }
                if (!slab(r0, r1, ob.o, ob.inv, t_max, t_enter)) continue;
                link = r0.w;
            }
            uint32_t kind = link >> NODE_KIND_SHIFT, payload = link & NODE_PAYLOAD_MASK;
            ss.section(StepStats::BRANCH, kind == NODE_BRANCH);
            // up to PT_BRANCH_LEVELS_ANY levels per step: the child that would be popped next (right if met, else left) is expanded or
            // tested at once instead of going through the stack (the kernel pays per wave-step, profiles/r02_step_stats_cornell.md)
#pragma unroll 1
            for (int lvl = 0; lvl < PT_BRANCH_LEVELS_ANY && kind == NODE_BRANCH; ++lvl)
            {
                const uint4* cp = bl.nodes + 2u * payload;
                const uint4 l0 = cp[0], l1 = cp[1], r0 = cp[2], r1 = cp[3];
                const f3 o = (IDENT || in_blas) ? ob.o : w.o, inv = (IDENT || in_blas) ? ob.inv : w.inv;
                float tl, tr;
                const bool hl = slab(l0, l1, o, inv, t_max, tl);
                const bool hr = slab(r0, r1, o, inv, t_max, tr);
                if (hl && hr) { stk.put(sp, make_uint2(l0.w, asu(tl))); sp = stk.up(sp); }   // left then right: right is popped first
                kind = NODE_INSTANCE; // nothing more in this step unless the next child says otherwise
                if (hl || hr)
                {
                    const uint2 next = hr ? make_uint2(r0.w, asu(tr)) : make_uint2(l0.w, asu(tl));
                    const uint32_t nk = next.x >> NODE_KIND_SHIFT;
                    if ((nk & 1u) != 0u || (nk == NODE_BRANCH && lvl + 1 < PT_BRANCH_LEVELS_ANY))
                    {
                        kind = nk;
                        payload = next.x & NODE_PAYLOAD_MASK;
                        t_enter = asf(next.y);
                    }
                    else { stk.put(sp, next); sp = stk.up(sp); }
                }
            }
            ss.section(StepStats::LEAF, (kind & 1u) != 0u);
            if (kind & 1u)
            {
                uint32_t first, count;
                leaf_range(bl, kind, payload, first, count);
                for (uint32_t k = 0; k < count; ++k)         // intersect_bool  primitive.rs:181-189
                {
                    const uint4* tp = bl.tris + 3u * (first + k);
                    float td, ud, vd, det;
                    if (tri_planes(tp[0], tp[1], tp[2], ob.o, ob.d, t_max, t_enter, td, ud, vd, det))
                    {
                        active = false;
                        put_result(1u);
                        break;
                    }
                }
            }
        }
    }
    if (MODE == ANY_SHADOW)
    {
        ss.flush(heads); // (the shadow queue's cursor lines, as k_closest's: tools/step_stats.py any)
        add_tally(heads, valid_rays, HEAD_TALLY0);
        wt.write(g_any_times);
    }
}
template <int BVH, int MODE, bool SPILL, bool IDENT = false>
__global__ void __launch_bounds__(256, BVH != 0 ? PT_WAVES_LDS_BVH_ANY : PT_WAVES_GLOBAL_BVH_ANY) k_any(const SceneView sv, const uint4* __restrict__ gblob, const uint32_t root, const f4* __restrict__ ra,
                                              const f4* __restrict__ rb, const uint32_t* __restrict__ n_ptr, const uint32_t cap_in,
                                              uint32_t* __restrict__ heads, uint32_t* __restrict__ occluded,
                                              f4* __restrict__ radiance)
{
    constexpr bool LDS_SCENE = BVH != 0;
    extern __shared__ uint4 smem[];
    if (blockIdx.x >= fetch_plan(min(*n_ptr, cap_in), LDS_SCENE ? (uint32_t)PT_CHUNK_DIV : (uint32_t)PT_CHUNK_DIV_GLOBAL_BVH, (uint32_t)PT_TAPER_ANY).blocks) return;
    uint32_t blob_words;
    const Blob bl = stage_scene<LDS_SCENE>(sv, gblob, smem, blob_words);
    any_body<BVH, MODE, SPILL, IDENT>(sv, bl, blob_words, smem, root, ra, rb, n_ptr, cap_in, heads, occluded, radiance);
}

// One launch for two of the three traversals between two shading passes: the world closest-hit rays of bounce b, then the (few)
// BSDF-sampled NEE rays the shading pass of bounce b - 1 cast.  Neither needs the other's results — the world launch finishes only
// paths that cast no BSDF-sampled ray — so a wave that finds the first queue drained goes on to the second without waiting for
// anybody: the NEE launch's own grid, its launch tail and the side stream's fork / join disappear from every bounce.
// (The shadow rays of bounce b - 1 cannot join them: a path that ends at the world hit still owes its explicit-light estimate, and
// k_closest<WORLD> reads what the shadow-ray launch left of it.  Tried all the same, with such paths sent through the terminal queue
// instead: what the two saved launch tails return, the terminal pass takes.)
struct FusedArgs
{
    const f4 *wa, *wb;          // world closest-hit rays of this bounce
    const uint32_t* wn;
    uint32_t* wheads;
    const f4 *la, *lb;          // BSDF-sampled NEE rays of the bounce before
    const uint32_t* ln;
    uint32_t* lheads;
    uint32_t world_root, lights_root, cap_in;
};
struct FusedKArgs
{
    SceneView sv;
    const uint4* gblob;
    FusedArgs fa;
    ClosestOut wout, lout;
};
template <int BVH, bool SPILL, bool IDENT = false>
__global__ void __launch_bounds__(256, BVH != 0 ? PT_WAVES_LDS_BVH : PT_WAVES_GLOBAL_BVH) k_trace_fused(const FusedKArgs a)
{
    constexpr bool LDS_SCENE = BVH != 0;
    extern __shared__ uint4 smem[];
    const uint32_t cdiv = LDS_SCENE ? (uint32_t)PT_CHUNK_DIV : (uint32_t)PT_CHUNK_DIV_GLOBAL_BVH;
    const uint32_t need = max(fetch_plan(min(*a.fa.wn, a.fa.cap_in), cdiv, (uint32_t)PT_TAPER).blocks, fetch_plan(min(*a.fa.ln, a.fa.cap_in), cdiv, (uint32_t)PT_TAPER).blocks);
    if (blockIdx.x >= need) return;
    uint32_t blob_words;
    const Blob bl = stage_scene<LDS_SCENE>(a.sv, a.gblob, smem, blob_words);
    typedef const __attribute__((address_space(4))) FusedKArgs* FusedKArgsPtr;
    const FusedKArgsPtr k = (FusedKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    closest_body<BVH, CLOSEST_WORLD, SPILL, IDENT>(a.sv, bl, blob_words, smem, a.fa.world_root, a.fa.wa, a.fa.wb, a.fa.wn, a.fa.cap_in, a.fa.wheads, &k->wout);
    closest_body<BVH, CLOSEST_LIGHTS, SPILL, IDENT>(a.sv, bl, blob_words, smem, a.fa.lights_root, a.fa.la, a.fa.lb, a.fa.ln, a.fa.cap_in, a.fa.lheads, &k->lout);
}

// ------------------------------------------------------------------------------------------------ path bookkeeping
struct PixelId { uint32_t gpixel, sample, lpixel, gx, gy; };

__device__ __forceinline__ uint32_t global_row(const RenderParams& rp, uint32_t ly)
{
    const uint32_t strip = fastdiv(ly, rp.div_strip_rows);
    return (strip * rp.world_size + rp.rank) * rp.strip_rows + (ly - strip * rp.strip_rows);
}
// path id <-> (batch-local sample, index of the pixel in the active rectangle): pid_split, pid_join (pt_queue_plan.h)
__device__ __forceinline__ PixelId path_pixel(const RenderParams& rp, uint32_t pid, uint32_t* s_local = nullptr, uint32_t* k_out = nullptr)
{
    const PidParts pp = pid_split(rp, pid);
    if (s_local) *s_local = pp.s;
    if (k_out) *k_out = pp.k;
    const uint32_t r = fastdiv(pp.k, rp.div_act_w), x = rp.act_x0 + (pp.k - r * rp.act_w);
    const uint32_t ly = rp.act_ly0 + r;
    const uint32_t gy = global_row(rp, ly);
    return PixelId{gy * rp.width + x, rp.first_sample + pp.s, ly * rp.width + x, x, gy};
}

// Adaptive list (pt_render_adaptive): the batch's path ids index the entries {local pixel, n_p} of the list k_adaptive_write made
// (RenderParams::act_pixels = its length) instead of the active rectangle.  Entry k's batch-local sample s is the pixel's sample
// n_p + first_sample + s: a pixel's samples continue from its own count, whatever the other pixels hold.
__device__ __forceinline__ PixelId path_pixel_list(const RenderParams& rp, const uint2* __restrict__ list, uint32_t pid, uint32_t* s_local = nullptr,
                                                   uint32_t* k_out = nullptr)
{
    const PidParts pp = pid_split(rp, pid);
    if (s_local) *s_local = pp.s;
    if (k_out) *k_out = pp.k;
    const uint2 e = list[pp.k];
    const uint32_t ly = fastdiv(e.x, rp.div_width), x = e.x - ly * rp.width;
    const uint32_t gy = global_row(rp, ly);
    return PixelId{gy * rp.width + x, e.y + rp.first_sample + pp.s, e.x, x, gy};
}

// main.rs:186-199.  CAM (CameraKind, pt_camera.h): the camera ray is primary_ray's for the kind.  Every kind but the pinhole stores the ray's
// origin beside its direction (a lens ray's and an orthographic ray's are their own; a panorama's is the eye, so that both projections run one
// set of bounce-0 kernels); the pinhole's bounce 0 knows the eye.  No state is initialised: bounce 0 knows path_weight = 1, accumulated = 0
// and the draws consumed (integrator.rs:153-161; the lens TWO, the others ONE).  LIST: over an adaptive list (path_pixel_list)
template <uint32_t CAM, bool LIST>
__global__ void __launch_bounds__(256) k_generate(const RenderParams rp, const CameraArg<CAM> cam, const RayQueue rq, Counters* ctr, const uint2* __restrict__ list)
{
    const uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid == 0u) ctr[0].n_closest = rp.n_paths;
    if (pid >= rp.n_paths) return;
    const PixelId px = LIST ? path_pixel_list(rp, list, pid) : path_pixel(rp, pid);
    f3 o;
    const f3 dir = primary_ray<CAM>(rp, cam, px.gx, px.gy, px.sample, &o);
    if (CAM != CAM_PINHOLE) rq.a[pid] = f4{o.x, o.y, o.z, __builtin_inff()};
    rq.b[pid] = f4{dir.x, dir.y, dir.z, asf(pid)};
}

// Ray list (pt_integrate_rays): the batch's path ids index the window of the caller's rays (RayView), one path per ray, and a path's stream is
// the one its table entry names: {pixel, sample} as given, not a pixel of the image.  (pid_split would return the same s = 0, k = pid.)
__device__ __forceinline__ PixelId path_pixel_rays(const uint2* __restrict__ keys, uint32_t pid, uint32_t* s_local, uint32_t* k_out)
{
    *s_local = 0u;
    *k_out = pid;
    const uint2 e = keys[pid];
    return PixelId{e.x, e.y, 0u, 0u, 0u};
}

// the camera's place in a ray batch: a copy of the window's rays into the bounce-0 queue
__global__ void __launch_bounds__(256) k_generate_rays(const uint32_t n, const float* __restrict__ o, const float* __restrict__ d, const RayQueue rq, Counters* ctr)
{
    const uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid == 0u) ctr[0].n_closest = n;
    if (pid >= n) return;
    const float* po = o + 3u * (size_t)pid;
    const float* pd = d + 3u * (size_t)pid;
    rq.a[pid] = f4{po[0], po[1], po[2], __builtin_inff()};
    rq.b[pid] = f4{pd[0], pd[1], pd[2], asf(pid)};
}

struct ShadeIO
{
    PathState st;
    RayQueue rq_in, rq_out, rq_shadow, rq_lchain_prev, rq_lchain;
    f4* lchain_nb;            // this bounce's BSDF-sampled rays: bsdf rgb | weakening, by rq_lchain slot
    const f4* lchain_nb_prev; // last bounce's
    const f4* lchain_hit;     // last bounce's light hits, by rq_lchain_prev slot
    const f4* hits;           // terminal pass only: hits of the rays that went to the terminal queue, by ray index
    union
    {
        const uint2* entries; // terminal pass: {ray index | ENTRY_DEAD, path id}
        const uint2* list;    // surface passes of an adaptive render (k_shade_surface<.., PATHS_LIST, ..>): the list's {local pixel, n_p} entries;
                              // of a ray batch (k_shade_surface<.., PATHS_RAYS, ..>): the window's {pixel, sample} stream keys (RayView::key)
    };
    ShadeQueue q_in;          // surface pass: this class's hit records in queue order
    const uint32_t* tails_in; // ... and the queue's striped tails
    uint2* q_term_next;
    uint32_t cap_slots, cap_slots_term, cap_slots_shade; // queue capacities (slots)
    Counters* ctr;     // row of this bounce
    uint32_t* lchain_heads; // cursor lines of this bounce's BSDF-sampled NEE queue (the culled tally goes there)
    uint32_t* shadow_heads; // cursor lines of this bounce's shadow-ray queue (INLINE: the tally of shadow rays traced by the shading pass itself)
    Counters* ctr_next;
    f4 primary_a;      // bounce 0: origin.xyz | +inf of every primary ray
    EnvView env;       // equirect environment for misses (w == 0: constant ambient, integrator.rs:263-266)
};

// MIS power heuristic  integrator.rs:22
__device__ __forceinline__ float mis2(float f, float g) { return sq(f) / (sq(f) + sq(g)); }

// shading normal of a hit: Triangle::get_normal + face-forward in object space (primitive.rs:57-63,161-165),
// then the deferred instance transform (tlas.rs:105)
__device__ __forceinline__ f3 hit_normal(const SceneView& sv, uint32_t inst, uint32_t tri, float u, float v, f3 dir_world, bool& front)
{
    const DTriVerts tv = sv.tri_shade[tri];
    const float wgt = 1.0f - u - v;
    const m33 nm{xyz(tv.a), xyz(tv.b), xyz(tv.c)};
    f3 n = unit3(mul(nm, f3{wgt, u, v}));
    const DInstance& in = sv.instances[inst];
    const f3 d_obj{(in.inv[0] * dir_world.x + in.inv[1] * dir_world.y) + in.inv[2] * dir_world.z,
                   (in.inv[4] * dir_world.x + in.inv[5] * dir_world.y) + in.inv[6] * dir_world.z,
                   (in.inv[8] * dir_world.x + in.inv[9] * dir_world.y) + in.inv[10] * dir_world.z};
    front = dot3(d_obj, n) < 0.0f;
    if (!front) n = -n;
    return f3{(in.fwd[0] * n.x + in.fwd[1] * n.y) + in.fwd[2] * n.z, (in.fwd[4] * n.x + in.fwd[5] * n.y) + in.fwd[6] * n.z,
              (in.fwd[8] * n.x + in.fwd[9] * n.y) + in.fwd[10] * n.z};
}

// add the previous bounce's direct-light estimate: accumulated += path_weight * (explicit + bsdf)   integrator.rs:231-234
// TEX (a textured scene): the light's emitted colour is its surface colour at the light hit, and the pdf the sampler has for the hit triangle
// is the host's own weight / sum (HostScene::build_lights: area * |emitted colour at kLightWeightUV| / sum), which a textured scene keeps per
// light triangle in tri_shade[tri].a.w: the same operations as below, done once on the host.  get_tex() is the kernel's texture view
template <bool TEX = false, typename GetTex = int>
__device__ __forceinline__ void resolve_nee(const SceneView& sv, const ShadeIO& io, uint32_t pid, const DPathRec& rec, f3& acc, uint32_t& flags,
                                            [[maybe_unused]] GetTex get_tex = GetTex{})
{
    if (!(flags & FLAG_NEE_PENDING)) return;
    const f4 e4 = rec.nee_e;
    const f4 pw4 = rec.nee_pw;
    f3 e = xyz(e4);
    // (a blocked explicit shadow ray has already zeroed nee_e in the record: k_any<SHADOW>)
    f3 s{0.0f, 0.0f, 0.0f};
    if (flags & FLAG_BSDF_CAST)
    {
        if (io.st.occl[pid] == 0u && pw4.w > 0.0f)                       // integrator.rs:100,103,108 (0 = light hit and visible)
        {
            const uint32_t slot = asu(e4.w); // of the BSDF-sampled ray in last bounce's rq_lchain
            const f4 lh = io.lchain_hit[slot];
            const uint32_t lid = asu(lh.w);
            const f4 b4 = io.lchain_nb_prev[slot];
            const uint32_t inst = lid >> sv.prim_bits, tri = lid & ((1u << sv.prim_bits) - 1u);
            const DInstance& in = sv.instances[inst];
            const DMaterial& lm = sv.materials[in.material];
            f3 emitted{lm.colour[0], lm.colour[1], lm.colour[2]};
            const DTriIsect ti = sv.tri_isect[tri];
            const float area = 0.5f * len3(xyz(ti.n0));                    // primitive.rs:94
            float sample_pdf;                                             // light_sampler.rs:39, integrator.rs:111
            if constexpr (TEX)
            {
                sample_pdf = sv.tri_shade[tri].a.w / area;
                emitted = surface_colour(get_tex(), lm.texture, emitted, tri, lh.y, lh.z);
            }
            else sample_pdf = (area * len3(emitted) / sv.light_weight_sum) / area;
            const f3 dir = xyz(io.rq_lchain_prev.b[slot]);
            bool ff;
            const f3 ln = hit_normal(sv, inst, tri, lh.y, lh.z, dir, ff);
            const float cosine = fabsf(dot3(dir, ln));
            const float light_pdf = sample_pdf * (lh.x * lh.x / cosine);   // integrator.rs:115
            const float weight = mis2(pw4.w, light_pdf);
            s = emitted * weight * b4.w * xyz(b4) / pw4.w;                 // integrator.rs:119-123
        }
    }
    acc = acc + xyz(pw4) * (e + s);
    flags &= ~(FLAG_NEE_PENDING | FLAG_BSDF_CAST);
}

// ------------------------------------------------------------------------------------------------ shading
// Q_TERMINAL: misses (integrator.rs:254-269), emissive hits (:207-214) and paths that already ended but still owe an NEE resolve.
// LENS (pt_set_lens): a camera ray's origin is its own, read from the ray queue at bounce 0 as at any other
template <typename T>
__device__ __forceinline__ const T& first_of(const T& t) { return t; }
// Tex (the terminal pass of a scene with an emission texture: one trailing TexView argument, which no other instantiation has): an emissive
// hit's emitted colour is its surface colour, and so is the light's in the resolve (resolve_nee<TEX>)
template <bool LENS = false, typename... Tex>
__global__ void __launch_bounds__(256) k_shade_terminal(const SceneView sv, const RenderParams rp, const ShadeIO io, const uint32_t bounce, const Tex... tex)
{
    constexpr bool TEX = sizeof...(Tex) != 0;
    static_assert(sizeof...(Tex) <= 1, "at most the texture view");
    const uint32_t n = min(io.ctr->n_shade[Q_TERMINAL], io.cap_slots_term);
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += gridDim.x * blockDim.x)
    {
        const uint2 e2 = io.entries[idx];
        const uint32_t entry = e2.x, pid = e2.y;
        if (entry == HOLE) continue;
        const bool dead = (entry & ENTRY_DEAD) != 0u;
        f4 ra{}, rb{}, hit{};
        if (!dead)
        {
            hit = io.hits[entry];
            if (asu(hit.w) != MISS_ID) // a miss needs no origin, and its direction only for the environment lookup
            {
                ra = (!LENS && bounce == 0u) ? io.primary_a : io.rq_in.a[entry];
                rb = io.rq_in.b[entry];
            }
            else if (io.env.w != 0u) rb = io.rq_in.b[entry];
        }
        f3 acc{0.0f, 0.0f, 0.0f};
        uint32_t flags = 0u;
        if (bounce != 0u)
        {
            const DPathRec& rec = io.st.rec[pid];
            const f4 acc4 = rec.acc;
            acc = xyz(acc4);
            flags = asu(acc4.w);
            if constexpr (TEX) resolve_nee<true>(sv, io, pid, rec, acc, flags, [&]() -> const TexView& { return first_of(tex...); });
            else resolve_nee(sv, io, pid, rec, acc, flags);
        }
        if (!dead)
        {
            const f3 pw = bounce == 0u ? f3{1.0f, 1.0f, 1.0f} : xyz(io.st.rec[pid].pw);
            const uint32_t hid = asu(hit.w);
            if (hid == MISS_ID)
            {
                if (io.env.w != 0u) acc = acc + env_lookup(io.env, xyz(rb)) * pw;      // integrator.rs:256-262
                else acc = acc + f3{0.006f, 0.006f, 0.006f} * pw;                      // integrator.rs:263-266
            }
            else
            {
                const uint32_t inst = hid >> sv.prim_bits;
                const DInstance& in = sv.instances[inst];
                if (bounce == 0u)                                                     // integrator.rs:181-185
                {
                    const PidParts pp = pid_split(rp, pid);
                    if (pp.s == rp.keep_s_pos)
                    {
                        const f3 p = fma3(xyz(rb), bc3(hit.x), xyz(ra));
                        io.st.first_pos[pp.k] = f4{p.x, p.y, p.z, hit.x};
                    }
                    if (pp.s >= rp.keep_s_id) io.st.first_id[(pp.s - rp.keep_s_id) * rp.act_pixels + pp.k] = in.blas & 0xffu;
                }
                const DMaterial& m = sv.materials[in.material];
                if (!rp.enable_nee || (flags & FLAG_LAST_DELTA) || bounce == 0u)       // integrator.rs:209-212
                {
                    f3 emitted{m.colour[0], m.colour[1], m.colour[2]};
                    if constexpr (TEX) emitted = surface_colour(first_of(tex...), m.texture, emitted, hid & ((1u << sv.prim_bits) - 1u), hit.y, hit.z);
                    acc = fma3(emitted, pw, acc);
                }
            }
        }
        io.st.radiance[pid] = f4{acc.x, acc.y, acc.z, 0.0f}; // every entry of this queue is a finished path
    }
}

// TLAS::any_intersect for ONE ray per lane, run by the whole wave until its last ray is done (no refill): the shading pass of an LDS-resident scene
// answers its own explicit-light shadow ray with it (k_shade_surface<.., SHADOW_INLINE.., ..>).  Steps as in any_body: a node's box is tested when its parent is
// expanded, only nodes that were met go on the stack; the answer is a disjunction, so the order cannot change it.
template <bool IDENT>
__device__ __forceinline__ bool inline_any(const Blob& bl, const Stack8<false>& stk, const uint32_t root, const f4 ra, const f4 rb, const bool want)
{
    bool active = false, blocked = false, in_blas = false, ray_finite = false;
    LaneRay w{}, ob{};
    const float t_max = ra.w;
    uint32_t sp = stk.empty(), blas_base = 0u;
    if (want)
    {
        w.o = xyz(ra);
        w.d = xyz(rb);
        w.inv = rcp3(w.d);
        ray_finite = finite3(w.o) && finite3(w.d);
        if (IDENT) ob = ident_ray(w);
        float te;
        const uint4 root0 = bl.nodes[2u * root];
        if ((t_max == t_max) && (!IDENT || ray_finite) && slab(root0, bl.nodes[2u * root + 1u], IDENT ? ob.o : w.o, w.inv, t_max, te))
        {
            stk.put(sp, make_uint2(root0.w, asu(te)));
            sp = stk.up(sp);
            active = true;
        }
    }
    while (__ballot(active) != 0ull)
    {
        if (!active) continue;
        if (!IDENT && in_blas && sp == blas_base) in_blas = false;
        if (sp == stk.empty()) { active = false; continue; }
        sp = stk.down(sp);
        const uint2 e = stk.get(sp);
        uint32_t link = e.x;
        float t_enter = asf(e.y);
        if ((link >> NODE_KIND_SHIFT) == NODE_INSTANCE)
        {
            uint4 r0, r1;
            if (IDENT)
            {
                const uint4* ip = bl.inst + INST_WORDS * (link & NODE_PAYLOAD_MASK) + INST_ROOT_WORD;
                r0 = ip[0]; r1 = ip[1];
            }
            else
            {
                ob = to_object<false, true>(bl, link & NODE_PAYLOAD_MASK, w, ray_finite, r0, r1);
                in_blas = true;
                blas_base = sp;
            }
            if (!slab(r0, r1, ob.o, ob.inv, t_max, t_enter)) continue;
            link = r0.w;
        }
        uint32_t kind = link >> NODE_KIND_SHIFT, payload = link & NODE_PAYLOAD_MASK;
#pragma unroll 1
        for (int lvl = 0; lvl < PT_BRANCH_LEVELS_INLINE && kind == NODE_BRANCH; ++lvl)
        {
            const uint4* cp = bl.nodes + 2u * payload;
            const uint4 l0 = cp[0], l1 = cp[1], r0 = cp[2], r1 = cp[3];
            const f3 o = (IDENT || in_blas) ? ob.o : w.o, inv = (IDENT || in_blas) ? ob.inv : w.inv;
            float tl, tr;
            const bool hl = slab(l0, l1, o, inv, t_max, tl);
            const bool hr = slab(r0, r1, o, inv, t_max, tr);
            if (hl && hr) { stk.put(sp, make_uint2(l0.w, asu(tl))); sp = stk.up(sp); }
            kind = NODE_INSTANCE;
            if (hl || hr)
            {
                const uint2 next = hr ? make_uint2(r0.w, asu(tr)) : make_uint2(l0.w, asu(tl));
                const uint32_t nk = next.x >> NODE_KIND_SHIFT;
                if ((nk & 1u) != 0u || (nk == NODE_BRANCH && lvl + 1 < PT_BRANCH_LEVELS_INLINE))
                {
                    kind = nk;
                    payload = next.x & NODE_PAYLOAD_MASK;
                    t_enter = asf(next.y);
                }
                else { stk.put(sp, next); sp = stk.up(sp); }
            }
        }
        if (kind & 1u)
        {
            uint32_t first, count;
            leaf_range(bl, kind, payload, first, count);
            for (uint32_t k = 0; k < count; ++k)
            {
                const uint4* tp = bl.tris + 3u * (first + k);
                float td, ud, vd, det;
                if (tri_planes(tp[0], tp[1], tp[2], ob.o, ob.d, t_max, t_enter, td, ud, vd, det))
                {
                    active = false;
                    blocked = true;
                    break;
                }
            }
        }
    }
    return blocked;
}

// Surface classes.  One kernel per queue class; RNG draws in program order of integrator.rs:231-251.
// The launch description as ONE kernel argument (offset 0 of the kernel-argument segment), so that a section of the kernel can read its
// fields from there when it runs (shade_args) instead of holding them in scalar registers across the whole iteration.
struct ShadeKArgs { SceneView sv; RenderParams rp; ShadeIO io; uint32_t bounce; const uint4* gblob; uint32_t world_root; };
typedef const __attribute__((address_space(4))) ShadeKArgs* ShadeKArgsPtr;
__device__ __forceinline__ const ShadeKArgs& shade_args()
{
    ShadeKArgsPtr p = (ShadeKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));        // loads through p cannot move above this point
    return *(const ShadeKArgs*)p;
}
// TEX variants: the texture view rides behind the launch description in their argument only (as CameraLensView does for k_accumulate): the
// other instantiations' arguments, and with them their code, are what they were
struct ShadeKArgsTex : ShadeKArgs { TexView tex; };
typedef const __attribute__((address_space(4))) ShadeKArgsTex* ShadeKArgsTexPtr;
__device__ __forceinline__ const TexView& shade_args_tex()
{
    ShadeKArgsTexPtr p = (ShadeKArgsTexPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return ((const ShadeKArgsTex*)p)->tex;
}
// NMAP variants: the tangent pointer rides behind the texture view in the same way (TexNView begins with the TexView, at ShadeKArgsTex's offset)
struct ShadeKArgsNmap : ShadeKArgs { TexNView tex; };
static_assert(sizeof(ShadeKArgsNmap) == sizeof(ShadeKArgsTex) + sizeof(const f4*) && alignof(TexNView) == alignof(TexView), "the texture view sits where ShadeKArgsTex has it: shade_args_tex serves both");
typedef const __attribute__((address_space(4))) ShadeKArgsNmap* ShadeKArgsNmapPtr;
__device__ __forceinline__ const TexNView& shade_args_texn()
{
    ShadeKArgsNmapPtr p = (ShadeKArgsNmapPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return ((const ShadeKArgsNmap*)p)->tex;
}
#define PT_SHADE_ARGS                                                                                                              \
    const ShadeKArgs& ka_ = shade_args();                                                                                          \
    [[maybe_unused]] const SceneView& sv = ka_.sv;                                                                                 \
    [[maybe_unused]] const RenderParams& rp = ka_.rp;                                                                              \
    [[maybe_unused]] const ShadeIO& io = ka_.io;
// The variants of the pass are the points of six axes (DESIGN.md has the table; QCLASS is the queue class Q_LAMBERT .. Q_GGX):
enum ShadeMedia : uint32_t { MEDIA_NONE, MEDIA_VOLUMES, MEDIA_COUNT };                    // SceneView::has_volumes
enum ShadeShadow : uint32_t { SHADOW_QUEUED, SHADOW_INLINE, SHADOW_INLINE_IDENT, SHADOW_COUNT }; // the explicit-light shadow ray: queued for k_any<SHADOW>, walked here (inline_any), walked here with one ray (ident_ray)
enum ShadePaths : uint32_t { PATHS_RECT, PATHS_LIST, PATHS_RAYS, PATHS_COUNT };           // path ids index the active rectangle, an adaptive list (ShadeIO::list, path_pixel_list) or a ray table (path_pixel_rays)
enum ShadeFirst : uint32_t { FIRST_SHARED, FIRST_OWN_TWO_DRAWS, FIRST_OWN_ONE_DRAW, FIRST_COUNT }; // the ray's origin is the eye's / the queue's own (every bounce but 0; bounce 0 of the pinhole), or comes with its record at bounce 0:
                                                                                         // a lens ray (two draws consumed; a ray table's: rp.ray_draws), a projected ray (one)
enum ShadeSurface : uint32_t { SURF_PLAIN, SURF_TEX, SURF_TEX_EMTEX, SURF_TEX_NMAP, SURF_TEX_EMTEX_NMAP, SURF_COUNT };
constexpr bool surf_emtex(uint32_t surface) { return surface == SURF_TEX_EMTEX || surface == SURF_TEX_EMTEX_NMAP; }
constexpr bool surf_nmap(uint32_t surface) { return surface == SURF_TEX_NMAP || surface == SURF_TEX_EMTEX_NMAP; }
// the points that exist: the inline walk is the untextured Lambertian pass's of a scene without media (shade_traces_shadow: a textured scene
// queues its shadow rays), and a ray table's bounce 0 takes its draw count from the launch, never "one"
constexpr bool shade_variant_ok(uint32_t q, uint32_t media, uint32_t shadow, uint32_t paths, uint32_t first, uint32_t surface)
{
    return q != Q_TERMINAL && q < Q_COUNT && media < MEDIA_COUNT && shadow < SHADOW_COUNT && paths < PATHS_COUNT && first < FIRST_COUNT && surface < SURF_COUNT &&
           (shadow == SHADOW_QUEUED || (q == Q_LAMBERT && media == MEDIA_NONE && surface == SURF_PLAIN)) && !(paths == PATHS_RAYS && first == FIRST_OWN_ONE_DRAW);
}
// the argument follows from SURFACE: the texture view, and behind it the tangents, ride behind the launch description
template <uint32_t SURFACE>
using ShadeArg = std::conditional_t<surf_nmap(SURFACE), ShadeKArgsNmap, std::conditional_t<SURFACE != SURF_PLAIN, ShadeKArgsTex, ShadeKArgs>>;
// SURF_TEX.. (a built scene with a textured material): the colour of the material at the hit is the surface colour (surface_colour,
// pt_materials.h).  The lookup is a chain of dependent loads (instance -> material -> UVs and table -> four texels).  It sits where the
// material is loaded, behind the NEE resolve: every TEX variant then has the registers, the scratch and the waves of its untextured twin.
// PT_TEX_EARLY=1 starts it right behind the path record's loads instead, so that the two wait for memory together; the colour is then live
// across the resolve and the specular / dielectric media variants drop from five waves to four and three others gain 12-40 bytes of
// scratch (tools/resource_table.py; profiles/r12_textures.md), so that is not the build.
#ifndef PT_TEX_EARLY
#define PT_TEX_EARLY 0
#endif
// ..EMTEX (some emissive material has an emission texture): a light's emitted colour is its surface colour too, at the point the explicit
// estimate sampled and at the light hit of the resolve (resolve_nee<true>).  ..NMAP (some material has a normal map): the shading normal is
// shading_normal (pt_materials.h), a second chain of the same kind right behind the colour lookup; `front` stays the unperturbed normal's.
// Each is a value of its own: the TEX variants of a scene without textured lights or normal maps stay the kernels they were.
template <uint32_t QCLASS, uint32_t MEDIA, uint32_t SHADOW, uint32_t PATHS, uint32_t FIRST, uint32_t SURFACE>
__global__ void __launch_bounds__(PT_SHADE_THREADS, SHADOW != SHADOW_QUEUED ? PT_SHADE_WAVES_INLINE : shade_waves(QCLASS, MEDIA == MEDIA_VOLUMES))
k_shade_surface(const ShadeArg<SURFACE> kargs)
{
    static_assert(shade_variant_ok(QCLASS, MEDIA, SHADOW, PATHS, FIRST, SURFACE), "no such variant of the surface pass");
    constexpr bool VOLUMES = MEDIA == MEDIA_VOLUMES, INLINE = SHADOW != SHADOW_QUEUED, IDENT = SHADOW == SHADOW_INLINE_IDENT;
    constexpr bool LIST = PATHS == PATHS_LIST, RAYS = PATHS == PATHS_RAYS, LENS = FIRST != FIRST_SHARED, ONE_DRAW = FIRST == FIRST_OWN_ONE_DRAW;
    constexpr bool TEX = SURFACE != SURF_PLAIN, EMTEX = surf_emtex(SURFACE), NMAP = surf_nmap(SURFACE);
    extern __shared__ uint4 smem_dyn[];
    // Only what the loop header needs is taken from the argument here; each section of an iteration re-reads the launch description from
    // the kernel-argument segment (PT_SHADE_ARGS: scalar loads that hit the constant cache) instead of keeping ~130 words of it in ~100
    // scalar registers for the whole iteration: spilled scalars 81 -> 0 (every class), static VALU 1947 -> 1747 (no v_readlane / v_writelane).
    const ShadeIO& io = kargs.io;
    const uint32_t bounce = kargs.bounce;
    __shared__ BlockAppend sh_append;
    __shared__ uint32_t sh_tail[kTailStripes];
    __shared__ uint32_t sh_extent;
    // the queue's extent and the regions the shorter stripes never reached (stripe_valid); keyed like the producer's (k_closest of this bounce)
    const Stripes stripes = stripes_for(min(io.ctr->n_closest, io.cap_slots));
    if (threadIdx.x < kTailStripes)
    {
        uint32_t mine;
        const uint32_t ext = stripe_load(io.tails_in, stripes, io.cap_slots_shade, mine);
        sh_tail[threadIdx.x] = mine;
        if (threadIdx.x == 0u)
        {
            sh_extent = ext;
            if (blockIdx.x == 0u) io.ctr->n_shade[QCLASS] = ext; // for the host's per-bounce table only
        }
    }
    // INLINE: the BVH blob and the per-lane stacks in dynamic LDS, as in the traversal kernels (stage_scene ends with the barrier)
    if (INLINE) { uint32_t words; (void)stage_scene<true>(kargs.sv, kargs.gblob, smem_dyn, words); }
    else __syncthreads();
    uint32_t traced = 0u; // INLINE: wave-uniform (a scalar register): shadow rays this wave has answered
    const uint32_t n = sh_extent;
    const uint32_t total = ((n + blockDim.x - 1u) / blockDim.x) * blockDim.x; // whole blocks take part in the queue appends
    uint32_t culled = 0;
    // Everything this pass needs of a hit arrives in queue order (ShadeQueue): direction | path id, t u v | hit id, origin.  The first
    // word of the NEXT iteration is fetched one iteration ahead, so the path-record load that depends on its path id starts as soon
    // as an iteration begins instead of one memory round trip later.
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const f4 hole_a{0.0f, 0.0f, 0.0f, asf(HOLE)};
    f4 a_next = idx < n ? nt_load(io.q_in.a + idx) : hole_a;
    for (; idx < total; idx += stride)
    {
        const f4 rb = a_next;
        if (!INLINE) a_next = (idx + stride) < n ? nt_load(io.q_in.a + idx + stride) : hole_a; // (INLINE: requested after the shadow walk, which wants the registers)
        bool valid = idx < n && stripe_valid(sh_tail, stripes, idx) && asu(rb.w) != HOLE;
        bool want_shadow = false, want_lchain = false, want_next = false, want_dead = false, ends_with_shadow = false, cull_now = false;
        f4 sh_a{}, sh_b{}, lc_a{}, lc_b{}, nx_a{}, nx_b{};
        uint32_t pid = 0, flags = 0;
        f3 acc{}, pw{};
        f4 nee_e{}, nee_pw{}, nee_b{};
        uint32_t draws = 0;
        if (valid)
        {
            PT_SHADE_ARGS
            pid = asu(rb.w);
            const f4 hit = nt_load(io.q_in.b + idx);
            const f4 ra = (!LENS && bounce == 0u) ? io.primary_a : nt_load(io.q_in.c + idx);
            f4 pw4{1.0f, 1.0f, 1.0f, asf(RAYS ? rp.ray_draws : (LENS && !ONE_DRAW) ? 2u : 1u)}; // bounce 0: path_weight = 1, accumulated = 0, the seed draw consumed (LENS: and the lens point's)
            acc = f3{0.0f, 0.0f, 0.0f};
            flags = 0u;
            [[maybe_unused]] f3 surf{};
            [[maybe_unused]] auto textured = [&]() -> f3 {
                const uint32_t hid_ = asu(hit.w);
                const DMaterial& dm = sv.materials[sv.instances[hid_ >> sv.prim_bits].material];
                return surface_colour(shade_args_tex(), dm.texture, f3{dm.colour[0], dm.colour[1], dm.colour[2]}, hid_ & ((1u << sv.prim_bits) - 1u), hit.y, hit.z);
            };
            if (bounce != 0u)
            {
                const DPathRec& rec = io.st.rec[pid];
                const f4 acc4 = rec.acc;
                pw4 = rec.pw;
                if (TEX && PT_TEX_EARLY) surf = textured();
                acc = xyz(acc4);
                flags = asu(acc4.w);
                if constexpr (EMTEX) resolve_nee<true>(sv, io, pid, rec, acc, flags, [&]() -> const TexView& { return shade_args_tex(); });
                else resolve_nee(sv, io, pid, rec, acc, flags);
            }
            else if (TEX && PT_TEX_EARLY) surf = textured();
            pw = xyz(pw4);

            const f3 ro = xyz(ra), rd = xyz(rb);
            const uint32_t hid = asu(hit.w);
            const uint32_t inst = hid >> sv.prim_bits, tri = hid & ((1u << sv.prim_bits) - 1u);
            const DInstance& in = sv.instances[inst];
            MatView mat = load_material(sv.materials, in.material);
            // a roughness map (pt_set_material_roughness_texture): the GGX alpha of this hit, a run-time test inside the TEX variants of the
            // GGX class, as `texture == 0u` is inside surface_colour; no other kernel reads the word.  Behind the colour's lookup: started before
            // it behind a barrier, the plain SURF_TEX kernels gain 8 bytes of scratch, which here they do not (profiles/r33_roughness_maps.md)
            if (TEX) mat.colour = PT_TEX_EARLY ? surf : textured();
            if constexpr (TEX && QCLASS == Q_GGX)
                mat.alpha = surface_alpha(shade_args_tex(), sv.materials[in.material].roughness_texture, mat.alpha, tri, hit.y, hit.z);
            // the queue class fixes the material kind: let the compiler drop the other materials' code from this kernel
            if (QCLASS == Q_LAMBERT) mat.kind = (VOLUMES && mat.kind == MAT_EMISSIVE) ? (uint32_t)MAT_EMISSIVE : (uint32_t)MAT_LAMBERTIAN;
            else if (QCLASS == Q_SPECULAR) mat.kind = MAT_SPECULAR;
            else if (QCLASS == Q_DIELECTRIC) mat.kind = MAT_DIELECTRIC;
            else mat.kind = mat.kind == MAT_GGX_DIELECTRIC ? (uint32_t)MAT_GGX_DIELECTRIC : (uint32_t)MAT_GGX_METAL;
            bool front;
            f3 normal;
            if constexpr (NMAP) normal = shading_normal(sv.tri_shade, sv.instances, sv.materials, shade_args_texn(), inst, tri, hit.y, hit.z, rd, front);
            else normal = hit_normal(sv, inst, tri, hit.y, hit.z, rd, front);
            const f3 p = fma3(rd, bc3(hit.x), ro);                                     // r.at(hit_info.t)
            uint32_t s_local, k_pix;
            const PixelId px = RAYS   ? path_pixel_rays(io.list, pid, &s_local, &k_pix)
                               : LIST ? path_pixel_list(rp, io.list, pid, &s_local, &k_pix)
                                      : path_pixel(rp, pid, &s_local, &k_pix);
            if (bounce == 0u)                                                          // integrator.rs:181-185
            {
                if (s_local == rp.keep_s_pos) io.st.first_pos[k_pix] = f4{p.x, p.y, p.z, hit.x};
                if (s_local >= rp.keep_s_id) io.st.first_id[(s_local - rp.keep_s_id) * rp.act_pixels + k_pix] = in.blas & 0xffu;
            }
            Stream rng{stream_key(rp.seed, px.gpixel, px.sample), asu(pw4.w)};
            const f3 wi = -rd;                                                         // integrator.rs:187
            const bool is_delta = mat_is_delta(mat.kind);

            // ---- participating media  integrator.rs:189-205: free-flight scattering in every volume the path is inside
            bool scattered = false;
            float s_t = 0.0f;
            f3 s_dir{0.0f, 0.0f, 0.0f};
            uint64_t vst = kVStackEmpty, vst_in = kVStackEmpty;
            if (VOLUMES)
            {
                if (bounce != 0u) vst = io.st.vstack[pid];
                vst_in = vst;
                if (vst != kVStackEmpty)
                {
                    for (uint32_t slot = 0; slot < kVStackSlots; ++slot)       // the stack is packed: the first empty slot ends it
                    {
                        const uint32_t vm = (uint32_t)(vst >> (8u * slot)) & 0xffu;
                        if (vm == 0xffu) break;
                        const DMaterial& dm = sv.materials[vm];
                        if (dm.vol_flags & 2u)                                         // VolumeScatter::scatter  volume.rs:83-97
                        {
                            const float t = -ln_det(rng.f32()) / dm.vol_c;
                            if (!(t > hit.x))
                            {
                                const f3 d = hg_direction(dm.vol_g, rng, rd);
                                if (!scattered || total_order_key(t) < total_order_key(s_t)) { s_t = t; s_dir = d; } // min_by(total_cmp), first wins
                                scattered = true;
                            }
                        }
                    }
                    const float dist = scattered ? s_t : hit.x;
                    f3 wgt{1.0f, 1.0f, 1.0f};
                    for (uint32_t slot = 0; slot < kVStackSlots; ++slot)
                    {
                        const uint32_t vm = (uint32_t)(vst >> (8u * slot)) & 0xffu;
                        if (vm == 0xffu) break;
                        const DMaterial& dm = sv.materials[vm];
                        if (dm.vol_flags & 1u) wgt = wgt * beer_lambert(f3{dm.vol_abs[0], dm.vol_abs[1], dm.vol_abs[2]}, dist);
                    }
                    pw = pw * wgt;
                }
            }
            f3 ndir{0.0f, 0.0f, 0.0f}, next_o = p;
            bool alive = true;
            if (scattered)
            {
                // integrator.rs:196-200: the path continues from inside the medium; no surface interaction this iteration
                flags |= FLAG_LAST_DELTA;
                next_o = fma3(rd, bc3(s_t), ro);
                ndir = s_dir;
            }
            else if (mat.kind == MAT_EMISSIVE)
            {
                // only reached when the scene has volumes (emissive hits are then shaded here, after the media)  integrator.rs:207-214
                if (!rp.enable_nee || (flags & FLAG_LAST_DELTA) || bounce == 0u) acc = fma3(mat.colour, pw, acc);
                alive = false;
            }
            else
            {
            if (VOLUMES && sv.materials[in.material].has_volume != 0u)     // integrator.rs:217-227
            {
                // keyed by the instance's material index, which is one volume per model: the host gives every further model of a
                // volume-bearing material its own copy (HostScene::flatten)
                const uint32_t me = in.material & 0xffu;
                uint32_t depth = 0u;
                int found = -1;
                for (uint32_t slot = 0; slot < kVStackSlots; ++slot)
                {
                    const uint32_t vm = (uint32_t)(vst >> (8u * slot)) & 0xffu;
                    if (vm == 0xffu) break;
                    if (vm == me && found < 0) found = (int)slot;
                    ++depth;
                }
                if (front)
                {
                    if (found < 0)
                    {
                        if (depth < kVStackSlots) vst = (vst & ~(0xffull << (8u * depth))) | ((uint64_t)me << (8u * depth));
                        // a volume the stack cannot hold: the path would skip its media, so the batch is void (the host reports PT_ERR_LIMIT)
                        else __hip_atomic_store(&io.ctr->vstack_full, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                else if (found >= 0)
                {
                    // remove and close the gap so that insertion order is kept: the slots above `found` move down one, the top one empties
                    const uint64_t below = (1ull << (8u * (uint32_t)found)) - 1ull;
                    vst = (vst & below) | (((vst >> 8u) | (0xffull << 56u)) & ~below);
                }
            }
            if (rp.enable_nee && !is_delta)                                            // integrator.rs:231
            {
                // ---- estimate_direct_explicit  integrator.rs:25-74
                {
                    PT_SHADE_ARGS
                    const float x = rng.f32();                                         // light_sampler.rs:33
                    // binary_search_by(total_cmp): for a non-decreasing cdf Ok(i)/Err(i) = number of entries below x
                    uint32_t li = 0, hi = sv.n_lights;
                    const int32_t xk = total_order_key(x);
                    while (li < hi)
                    {
                        const uint32_t mid = (li + hi) >> 1;
                        if (total_order_key(sv.lights[mid].cdf) < xk) li = mid + 1u; else hi = mid;
                    }
                    if (li >= sv.n_lights) li = sv.n_lights - 1u;                       // clamp (reference would index out of bounds)
                    const DLight L = sv.lights[li];
                    float lu = rng.f32();                                              // primitive.rs:81-88
                    float lv = rng.f32();
                    if (lu + lv > 1.0f) { lu = 1.0f - lu; lv = 1.0f - lv; }
                    const float lw = 1.0f - lu - lv;
                    const DTriVerts lp = sv.tri_pos[L.tri], ln = sv.tri_shade[L.tri];
                    const f3 point = mul(m33{xyz(lp.a), xyz(lp.b), xyz(lp.c)}, f3{lw, lu, lv});
                    const f3 lnormal = unit3(mul(m33{xyz(ln.a), xyz(ln.b), xyz(ln.c)}, f3{lw, lu, lv}));
                    const f3 d = point - p;
                    const float dist2 = len_sq(d);
                    const float dist = sqrtf(dist2);
                    const f3 dir = unit3(d);
                    f3 ce{0.0f, 0.0f, 0.0f};
                    if (dot3(dir, normal) > 0.0f)                                      // integrator.rs:55
                    {
                        const BsdfSample bp = mat_bsdf_pdf(mat, wi, dir, normal, front);
                        const DTriIsect ti = sv.tri_isect[L.tri];
                        const float sample_pdf = L.pdf / (0.5f * len3(xyz(ti.n0)));    // integrator.rs:61
                        const float cosine = fabsf(dot3(dir, lnormal));
                        const float light_pdf = sample_pdf * (dist2 / cosine);         // integrator.rs:65
                        const float weight = mis2(light_pdf, bp.pdf);
                        const DMaterial& lm = sv.materials[L.material];
                        f3 emitted{lm.colour[0], lm.colour[1], lm.colour[2]};
                        // EMTEX: the emitted colour at the sampled point, whose barycentrics (lu, lv) are the hit record's convention
                        if constexpr (EMTEX) emitted = surface_colour(shade_args_tex(), lm.texture, emitted, L.tri, lu, lv);
                        ce = emitted * weight * mat_weakening(mat.kind, dir, normal) * bp.bsdf / light_pdf;
                        want_shadow = true;
                        sh_a = f4{p.x, p.y, p.z, (1.0f - PT_EPSILON) * dist};          // integrator.rs:56
                        sh_b = f4{dir.x, dir.y, dir.z, asf(pid)};
                    }
                    nee_e = f4{ce.x, ce.y, ce.z, 0.0f};
                }
                // ---- estimate_direct_bsdf  integrator.rs:77-130
                {
                    PT_SHADE_ARGS
                    const f3 dir = mat_scatter(mat, rng, rd, normal, front);
                    if (dot3(dir, normal) > 0.0f)                                      // integrator.rs:96
                    {
                        const BsdfSample bp = mat_bsdf_pdf(mat, wi, dir, normal, front);
                        // scene.lights.intersect(ray) starts with the root box of the lights TLAS (tlas.rs:68-74).  That test is done
                        // here, with the very arithmetic k_closest uses at refill: a ray that fails it (nearly all of them: the lights
                        // are small) finds no light, contributes nothing (integrator.rs:100-102) and never becomes a queue entry.
                        float te;
                        const uint4* const lr = reinterpret_cast<const uint4*>(sv.nodes + sv.lights_root);
                        const bool may_hit = slab(lr[0], lr[1], p, rcp3(dir), asf(0x7f800000u), te);
                        if (may_hit)
                        {
                            nee_b = f4{bp.bsdf.x, bp.bsdf.y, bp.bsdf.z, mat_weakening(mat.kind, dir, normal)};
                            nee_pw.w = bp.pdf;
                            want_lchain = true;
                            lc_a = f4{p.x, p.y, p.z, asf(0x7f800000u)};
                            lc_b = f4{dir.x, dir.y, dir.z, asf(pid)};
                            flags |= FLAG_BSDF_CAST;
                        }
                        else if (!INLINE) culled += 1u;
                        else cull_now = true;
                    }
                }
                nee_pw.x = pw.x; nee_pw.y = pw.y; nee_pw.z = pw.z;
                flags |= FLAG_NEE_PENDING;
            }

            // ---- continuation  integrator.rs:236-251
            ndir = mat_scatter(mat, rng, rd, normal, front);
            const BsdfSample info = mat_bsdf_pdf(mat, wi, ndir, normal, front);
            alive = !(info.pdf < 0.0f);                                                // MIN_PDF = 0  integrator.rs:243
            if (alive)
            {
                pw = pw * (mat_weakening(mat.kind, ndir, normal) * info.bsdf / info.pdf); // integrator.rs:249
                flags = is_delta ? (flags | FLAG_LAST_DELTA) : (flags & ~FLAG_LAST_DELTA);
            }
            } // surface interaction
            if (alive)
            {
                {
                const uint32_t nb = bounce + 1u;
                if (nb > rp.max_bounces) alive = false;                                 // for b in 0..=max_bounces
                else if (nb > 3u)                                                       // Russian roulette of the next iteration  integrator.rs:166-177
                {
                    const float survive = min_num(hmax3(pw), 0.9999f);
                    if (rng.f32() > survive) alive = false;
                    else pw = pw / survive;
                }
                }
            }
            if (alive && VOLUMES && (vst != vst_in || bounce == 0u)) io.st.vstack[pid] = vst;
            draws = rng.k;
            if (alive)
            {
                want_next = true;
                nx_a = f4{next_o.x, next_o.y, next_o.z, asf(0x7f800000u)};
                nx_b = f4{ndir.x, ndir.y, ndir.z, asf(pid)};
            }
            else if (flags & FLAG_NEE_PENDING)
            {
                // the path is over but still owes this bounce's direct light (integrator.rs:231-234)
                if (flags & FLAG_BSDF_CAST) want_dead = true;            // both estimates pending: the terminal pass adds them
                else if (want_shadow) { ends_with_shadow = true; sh_b.w = asf(pid | PATH_ENDS); } // the shadow-ray kernel finishes it
                else acc = acc + xyz(nee_pw) * (xyz(nee_e) + f3{0.0f, 0.0f, 0.0f});  // nothing was cast: explicit = bsdf = 0
            }
        }
        // ---- block-aggregated queue appends (every thread of the block reaches this): one atomic per queue per block
        PT_SHADE_ARGS
        uint32_t* const ctrs[4] = {&io.ctr->n_shadow, &io.ctr->n_lchain, &io.ctr_next->n_closest, &io.ctr_next->n_shade[Q_TERMINAL]};
        const bool preds[4] = {want_shadow && !INLINE, want_lchain, want_next, want_dead};
        const uint32_t caps[4] = {io.cap_slots, io.cap_slots, io.cap_slots, io.cap_slots_term};
        uint32_t pos[4];
        block_append4(sh_append, ctrs, preds, caps, &io.ctr->overflow, pos);
        if (want_shadow && !INLINE) { nt_store(io.rq_shadow.a + pos[0], sh_a); nt_store(io.rq_shadow.b + pos[0], sh_b); }
        if (want_lchain) { io.rq_lchain.a[pos[1]] = lc_a; io.rq_lchain.b[pos[1]] = lc_b; io.lchain_nb[pos[1]] = nee_b; nee_e.w = asf(pos[1]); }
        if (want_next) { nt_store(io.rq_out.a + pos[2], nx_a); nt_store(io.rq_out.b + pos[2], nx_b); }
        if (want_dead) io.q_term_next[pos[3]] = make_uint2(pid | ENTRY_DEAD, pid);
        const bool write_rec = valid && (want_next || want_dead || ends_with_shadow);
        if (valid && !write_rec) io.st.radiance[pid] = f4{acc.x, acc.y, acc.z, 0.0f}; // the path ended here, nothing owed
        // The 64-byte record is stored by the four lanes of a quad together, one whole record per store instruction (each lane a
        // 16-byte word): L2 then sees one full-sector write per record instead of four partial ones.  4x4 transposes inside the quad.
        {
            float m[4][4] = {{pw.x, pw.y, pw.z, asf(draws)}, {acc.x, acc.y, acc.z, asf(flags)}, {nee_e.x, nee_e.y, nee_e.z, nee_e.w}, {nee_pw.x, nee_pw.y, nee_pw.z, nee_pw.w}};
            const uint32_t q = threadIdx.x & 3u;
#pragma unroll
            for (int c = 0; c < 4; ++c) // component c of the four words: m[word][c]
            {
                float a0 = m[0][c], a1 = m[1][c], a2 = m[2][c], a3 = m[3][c];
                // exchange with lane ^ 1
                { const float t = (q & 1u) ? a0 : a1; const float r = asf(__builtin_amdgcn_mov_dpp(asu(t), 0xB1, 0xF, 0xF, true)); if (q & 1u) a0 = r; else a1 = r; }
                { const float t = (q & 1u) ? a2 : a3; const float r = asf(__builtin_amdgcn_mov_dpp(asu(t), 0xB1, 0xF, 0xF, true)); if (q & 1u) a2 = r; else a3 = r; }
                // exchange with lane ^ 2
                { const float t = (q & 2u) ? a0 : a2; const float r = asf(__builtin_amdgcn_mov_dpp(asu(t), 0x4E, 0xF, 0xF, true)); if (q & 2u) a0 = r; else a2 = r; }
                { const float t = (q & 2u) ? a1 : a3; const float r = asf(__builtin_amdgcn_mov_dpp(asu(t), 0x4E, 0xF, 0xF, true)); if (q & 2u) a1 = r; else a3 = r; }
                m[0][c] = a0; m[1][c] = a1; m[2][c] = a2; m[3][c] = a3; // now m[k][c] = component c of word q of quad member k
            }
            const uint32_t wr = write_rec ? 1u : 0u;
#define PT_QUAD_STORE(K, SEL)                                                                                                   \
            {                                                                                                                      \
                const uint32_t pid_k = __builtin_amdgcn_mov_dpp(pid, SEL, 0xF, 0xF, true); /* quad_perm [K,K,K,K] */               \
                const uint32_t wr_k = __builtin_amdgcn_mov_dpp(wr, SEL, 0xF, 0xF, true);                                           \
                if (wr_k != 0u) reinterpret_cast<f4*>(io.st.rec + pid_k)[q] = f4{m[K][0], m[K][1], m[K][2], m[K][3]};             \
            }
            PT_QUAD_STORE(0, 0x00) PT_QUAD_STORE(1, 0x55) PT_QUAD_STORE(2, 0xAA) PT_QUAD_STORE(3, 0xFF)
#undef PT_QUAD_STORE
        }
        if (INLINE)
        {
            // the explicit-light shadow ray is answered here, after the record is on its way, and applied to it as k_any<SHADOW> does (apply_shadow)
            // (the stack's base is recomputed here, behind an opaque move, rather than kept in a register across the iteration)
            // ... and so is the description of the staged scene (re-read from the kernel-argument segment like every other section's)
            uint32_t tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const ShadeKArgs& ka2 = shade_args();
            const uint32_t blob_words = ka2.sv.blob_bytes >> 4;
            const Blob bl = blob_at(ka2.sv, smem_dyn);
            const Stack8<false> stk{reinterpret_cast<char*>(smem_dyn), blob_words * 16u + tid * 8u, blockDim.x * 8u};
            traced += (uint32_t)__popcll(__ballot(want_shadow)); // (both counted here, where the whole wave is: wave-uniform values in scalar registers)
            culled += (uint32_t)__popcll(__ballot(cull_now));
            const bool blocked = inline_any<IDENT>(bl, stk, ka2.world_root, sh_a, sh_b, want_shadow);
            if (want_shadow) apply_shadow(shade_args().io.st.rec + pid, ends_with_shadow, blocked, [&]() -> f4& { return shade_args().io.st.radiance[pid]; });
            a_next = (idx + stride) < n ? nt_load(shade_args().io.q_in.a + idx + stride) : hole_a;
        }
    }
    if (!INLINE) add_tally(io.lchain_heads, culled, HEAD_TALLY2);
    else if (lane_id() == 0u)
    {
        // (both counts are wave-uniform here)
        const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        const uint32_t line = ((wave * 7u) & (kQueueHeads - 1u)) * kHeadStrideWords;
        if (culled != 0u) atomicAdd(io.lchain_heads + line + HEAD_TALLY2, culled);
        if (traced != 0u) atomicAdd(io.shadow_heads + line + HEAD_TALLY0, traced);
    }
}

#undef PT_SHADE_ARGS

// position r.at(1e5) of a camera ray that left the scene at once (integrator.rs:156), for whichever camera view it is given
template <typename CAM>
__device__ __forceinline__ f3 miss_position(const RenderParams& rp, const CAM& cam, uint32_t gx, uint32_t gy, uint32_t sample)
{
    f3 o;
    const f3 d = primary_ray(rp, cam, gx, gy, sample, &o);
    return fma3(d, bc3(1e5f), o);
}

// integrator.rs:272-280: finite check, clamp_length_max(100), alpha 1
__device__ __forceinline__ f3 finalise(f3 acc)
{
    if (!finite3(acc)) return f3{0.0f, 0.0f, 0.0f};
    return clamp_len_max(acc, 100.0f);
}

// luminance of a finalised sample (PT_FLAG_ADAPTIVE's moments and selection): every product and sum rounded in f32 (no contraction)
__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// accumulate.wgsl:20-23 applied once per sample, in sample order; id history shift main.rs:206.  A pixel outside the active rectangle
// (RenderParams::act_*) never had a path: each of its samples is the miss result of integrator.rs:263-266 — radiance 0.006, id 255,
// position r.at(1e5) of that sample's camera ray (:156-157) — added sample by sample like any other.
// The sum must be taken in sample order (float addition does not associate), the loads and the per-sample finite check / clamp need not
// wait for each other.  !FEW_PIXELS: one thread per LOCAL pixel, eight samples' loads in flight.  FEW_PIXELS (one rank's share of a
// sharded frame: the active pixels fill ~250 workgroups, one wave per SIMD, and the kernel waits on memory latency): FOUR lanes per
// pixel; lane q loads and finalises samples q, q + 4, ... and all four lanes then add the quad's values in sample order (DPP quad
// broadcasts; the sums are redundant, the loads are not): four times the loads in flight.
//
// MOMENTS (PT_FLAG_ADAPTIVE): moments[pixel] += L * L once per sample beside the colour, in the same order, L = luminance of the finalised
// sample.  LIST (pt_render_adaptive): one thread (quad) per entry of the adaptive list instead of per local pixel; unlisted pixels are
// not touched, and entry k's sample s is the pixel's sample n_p + first_sample + s (path_pixel_list).
//
// CAM (CameraView, CameraLensView or CameraProjView: pt_camera.h): the camera ray of a miss is that view's, so r.at(1e5) starts at the lens
// ray's point of the lens disk or at the projected ray's origin.  The lens or the projection rides behind the camera in that argument only:
// the pinhole instantiations' arguments are what they were.
template <typename CAM, bool FEW_PIXELS, bool MOMENTS = false, bool LIST = false>
__global__ void __launch_bounds__(256) k_accumulate(const RenderParams rp, const CAM cam, const PathState st,
                                                     f4* accum, f4* position, uint32_t* id, const uint32_t write_position, const uint32_t add_to_accum,
                                                     float* moments, const uint2* list)
{
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = FEW_PIXELS ? tid >> 2 : tid, q = FEW_PIXELS ? (tid & 3u) : 0u;
    if (t >= (LIST ? rp.act_pixels : rp.local_pixels)) return;
    uint2 entry{t, 0u};
    if (LIST) entry = list[t];
    const uint32_t lp = entry.x;
    f4 a = accum[lp];
    float qv = 0.0f;
    if (MOMENTS) qv = moments[lp];
    uint32_t idv = id[lp];
    const uint32_t ly = fastdiv(lp, rp.div_width), x = lp - ly * rp.width;
    if (!LIST && (x - rp.act_x0 >= rp.act_w || ly - rp.act_ly0 >= rp.act_rows))
    {
        for (uint32_t s = 0; s < rp.batch_samples; ++s)
        {
            a = f4{a.x + 0.006f, a.y + 0.006f, a.z + 0.006f, a.w + 1.0f};
            if (MOMENTS) { const float l = luminance(0.006f, 0.006f, 0.006f); qv = qv + l * l; }
        }
        for (uint32_t s = rp.batch_samples >= 2u ? rp.batch_samples - 2u : 0u; s < rp.batch_samples; ++s) idv = (idv << 16) | 255u;
        if (q != 0u) return;
        if (add_to_accum) accum[lp] = a;
        if (MOMENTS && add_to_accum) moments[lp] = qv;
        id[lp] = idv;
        if (write_position)
        {
            const f3 far = miss_position(rp, cam, x, global_row(rp, ly), rp.first_sample + rp.batch_samples - 1u);
            position[lp] = f4{far.x, far.y, far.z, 1e5f};
        }
        return;
    }
    const uint32_t k = LIST ? t : (ly - rp.act_ly0) * rp.act_w + (x - rp.act_x0);
    if (FEW_PIXELS)
    {
        constexpr uint32_t G = 4; // samples per lane and round: 16 per pixel
        for (uint32_t s0 = 0; s0 < rp.batch_samples; s0 += 4u * G)
        {
            uint32_t oc[G];
            f4 rad[G];
#pragma unroll
            for (uint32_t j = 0; j < G; ++j)
            {
                const uint32_t s = s0 + 4u * j + q;
                const uint32_t pid = pid_join(rp, s, k);
                oc[j] = s < rp.batch_samples ? (uint32_t)st.occl[pid] : (uint32_t)PRIMARY_MISS;
                // (a primary miss's record is stale memory inside the allocation: read and dropped, so that the load need not wait for the byte)
                rad[j] = s < rp.batch_samples ? st.radiance[pid] : f4{};
            }
            f3 c[G];
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) c[j] = finalise(oc[j] != PRIMARY_MISS ? xyz(rad[j]) : f3{0.006f, 0.006f, 0.006f});
#pragma unroll
            for (uint32_t j = 0; j < G; ++j)
            {
#define PT_QUAD_ADD(SEL, QQ)                                                                                                           \
                if (s0 + 4u * j + (QQ) < rp.batch_samples)                                                                          \
                {                                                                                                                      \
                    const float cx = asf(__builtin_amdgcn_mov_dpp(asu(c[j].x), SEL, 0xF, 0xF, true));                                 \
                    const float cy = asf(__builtin_amdgcn_mov_dpp(asu(c[j].y), SEL, 0xF, 0xF, true));                                 \
                    const float cz = asf(__builtin_amdgcn_mov_dpp(asu(c[j].z), SEL, 0xF, 0xF, true));                                 \
                    a = f4{a.x + cx, a.y + cy, a.z + cz, a.w + 1.0f};                                                                  \
                    if (MOMENTS) { const float l = luminance(cx, cy, cz); qv = qv + l * l; }                                           \
                }
                PT_QUAD_ADD(0x00, 0u) PT_QUAD_ADD(0x55, 1u) PT_QUAD_ADD(0xAA, 2u) PT_QUAD_ADD(0xFF, 3u)
#undef PT_QUAD_ADD
            }
        }
        if (q != 0u) return;
        // (id << 16) | new once per sample: only the batch's last two samples are kept (RenderParams::keep_s_id); a camera ray that left the
        // scene at once wrote nothing but its PRIMARY_MISS byte: id 255 (integrator.rs:157)
        for (uint32_t s = rp.keep_s_id; s < rp.batch_samples; ++s)
        {
            const bool miss = st.occl[pid_join(rp, s, k)] == PRIMARY_MISS;
            idv = (idv << 16) | (miss ? 255u : st.first_id[(s - rp.keep_s_id) * rp.act_pixels + k]);
        }
    }
    else
    {
        constexpr uint32_t G = 8;
        for (uint32_t s0 = 0; s0 < rp.batch_samples; s0 += G)
        {
            uint32_t oc[G];
            f4 rad[G];
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) oc[j] = (s0 + j) < rp.batch_samples ? (uint32_t)st.occl[pid_join(rp, s0 + j, k)] : (uint32_t)PRIMARY_MISS;
#pragma unroll
            for (uint32_t j = 0; j < G; ++j) rad[j] = oc[j] != PRIMARY_MISS ? st.radiance[pid_join(rp, s0 + j, k)] : f4{0.006f, 0.006f, 0.006f, 0.0f};
#pragma unroll
            for (uint32_t j = 0; j < G; ++j)
            {
                if ((s0 + j) >= rp.batch_samples) break;
                const f3 c = finalise(xyz(rad[j]));
                a = f4{a.x + c.x, a.y + c.y, a.z + c.z, a.w + 1.0f};
                if (MOMENTS) { const float l = luminance(c.x, c.y, c.z); qv = qv + l * l; }
                // (id << 16) | new once per sample: only the last two samples survive in 32 bits; a PRIMARY_MISS is id 255 (integrator.rs:157)
                if (s0 + j >= rp.keep_s_id) idv = (idv << 16) | (oc[j] == PRIMARY_MISS ? 255u : st.first_id[(s0 + j - rp.keep_s_id) * rp.act_pixels + k]);
            }
        }
    }
    if (add_to_accum) accum[lp] = a;
    if (MOMENTS && add_to_accum) moments[lp] = qv;
    id[lp] = idv;
    if (write_position)
    {
        // the batch's last sample.  A camera ray that left the scene at once has no record: r.at(1e5) of that sample's ray (integrator.rs:156)
        if (st.occl[pid_join(rp, rp.keep_s_pos, k)] == PRIMARY_MISS)
        {
            const f3 far = miss_position(rp, cam, x, global_row(rp, ly), entry.y + rp.first_sample + rp.keep_s_pos);
            position[lp] = f4{far.x, far.y, far.z, 1e5f};
        }
        else position[lp] = st.first_pos[k];
    }
}

// per-sample radiance (pt_render_samples): out[sample * local_pixels + local pixel]
__global__ void __launch_bounds__(256) k_store_samples(const RenderParams rp, const PathState st, f4* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rp.local_pixels * rp.batch_samples) return;
    const uint32_t s = i / rp.local_pixels, lp = i - s * rp.local_pixels;
    const uint32_t ly = fastdiv(lp, rp.div_width), x = lp - ly * rp.width;
    f3 c{0.006f, 0.006f, 0.006f};
    if (x - rp.act_x0 < rp.act_w && ly - rp.act_ly0 < rp.act_rows)
    {
        const uint32_t pid = pid_join(rp, s, (ly - rp.act_ly0) * rp.act_w + (x - rp.act_x0));
        c = finalise(st.occl[pid] == PRIMARY_MISS ? f3{0.006f, 0.006f, 0.006f} : xyz(st.radiance[pid]));
    }
    out[i] = f4{c.x, c.y, c.z, 1.0f};
}

// key[i], sample[i] of the caller's two arrays -> the ray table's {pixel, sample} entries
__global__ void __launch_bounds__(256) k_pack_ray_keys(const uint64_t n, const uint32_t* __restrict__ key, const uint32_t* __restrict__ sample, uint2* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_uint2(key[i], sample[i]);
}

// the finisher of a ray batch (pt_integrate_rays) in k_accumulate's place: the finalised sample, first hit and id byte of path i to entry i of the
// outputs (each may be null).  A ray that left the scene at once has no record but its PRIMARY_MISS byte: the ambient term, r.at(1e5) of the
// table's ray and id 255 (integrator.rs:156-157, 263-266), as k_accumulate rebuilds a camera ray's.
__global__ void __launch_bounds__(256) k_store_rays(const uint32_t n, const float* __restrict__ o, const float* __restrict__ d, const PathState st,
                                                     f4* __restrict__ radiance, f4* __restrict__ position, uint8_t* __restrict__ id)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool miss = st.occl[i] == PRIMARY_MISS;
    if (radiance)
    {
        const f3 c = finalise(miss ? f3{0.006f, 0.006f, 0.006f} : xyz(st.radiance[i]));
        radiance[i] = f4{c.x, c.y, c.z, 1.0f};
    }
    if (position)
    {
        f4 p;
        if (miss)
        {
            const float* po = o + 3u * (size_t)i;
            const float* pd = d + 3u * (size_t)i;
            const f3 far = fma3(f3{pd[0], pd[1], pd[2]}, bc3(1e5f), f3{po[0], po[1], po[2]});
            p = f4{far.x, far.y, far.z, 1e5f};
        }
        else p = st.first_pos[i];
        position[i] = p;
    }
    if (id) id[i] = miss ? (uint8_t)255u : (uint8_t)st.first_id[i];
}

// ------------------------------------------------------------------------------------------------ irradiance probes (pt_bake_probes)
// rays [first, first + count) of a bake into entries [0, count) of a ray table: sample first_sample + r % n_samples of probe r / n_samples
__global__ void __launch_bounds__(256) k_probe_rays(const ProbeBake pb, const uint64_t first, const uint32_t count, float* __restrict__ o,
                                                     float* __restrict__ d, uint2* __restrict__ key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t r = first + i;
    const uint32_t j = (uint32_t)(r / pb.n_samples), s = pb.first_sample + (uint32_t)(r - (uint64_t)j * pb.n_samples);
    float dir[3], y[9];
    probe_ray(pb.seed, pb.n_sobol, pb.key_base + j, s, dir, y);
    const float* pp = pb.position + 3u * (size_t)j;
    float* po = o + 3u * (size_t)i;
    float* pd = d + 3u * (size_t)i;
    po[0] = pp[0]; po[1] = pp[1]; po[2] = pp[2];
    pd[0] = dir[0]; pd[1] = dir[1]; pd[2] = dir[2];
    key[i] = make_uint2(pb.key_base + j, s);
}
// sh27[probe][k][c] += L[c] * y_k over the window's rays of that probe, in sample order: one thread per (probe, k, c), a serial fold by
// definition (float addition does not associate) and no atomics.  The 27 threads of a probe read the same d and L (one fetch per wave).
__global__ void __launch_bounds__(256) k_probe_project(const ProbeBake pb, const uint64_t first, const uint32_t count, const float* __restrict__ d,
                                                        const f4* __restrict__ radiance, float* __restrict__ sh27)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p0 = (uint32_t)(first / pb.n_samples), p1 = (uint32_t)((first + count - 1u) / pb.n_samples);
    if (t / 27u > p1 - p0) return;
    const uint32_t j = p0 + t / 27u, kc = t % 27u, k = kc / 3u, c = kc - 3u * k;
    const uint64_t lo = (uint64_t)j * pb.n_samples, hi = lo + pb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    float acc = sh27[(size_t)j * 27u + kc];
    for (uint32_t i = i0; i < i1; ++i)
    {
        const float* pd = d + 3u * (size_t)i;
        const float dir[3] = {pd[0], pd[1], pd[2]};
        float y[9];
        probe_sh9(dir, y);
        const f4 l4 = radiance[i];
        const float l = c == 0u ? l4.x : c == 1u ? l4.y : l4.z;
        acc = acc + l * y[k];
    }
    sh27[(size_t)j * 27u + kc] = acc;
}
// pt_probe_backfaces: the closest hits of rays [first, first + count) of a bake (hits[i] of ray first + i, its direction d[i]) counted into
// hits_out[probe] and back_out[probe]: one wave per probe the window touches, its lanes striding the probe's rays of the window, a wave
// reduction, and lane 0 adds the two integers to what the counts hold.  A wave owns its probe for the launch and the launches of a call
// follow each other on one stream: no atomics, and integers do not care how the rays were cut.  The front flag is hit_normal's.
__global__ void __launch_bounds__(256) k_probe_backfaces(const SceneView sv, const ProbeBake pb, const uint64_t first, const uint32_t count,
                                                         const float* __restrict__ d, const f4* __restrict__ hits, uint32_t* __restrict__ hits_out,
                                                         uint32_t* __restrict__ back_out)
{
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t p0 = (uint32_t)(first / pb.n_samples), p1 = (uint32_t)((first + count - 1u) / pb.n_samples);
    if (wave > p1 - p0) return; // (wave-uniform)
    const uint32_t j = p0 + wave;
    const uint64_t lo = (uint64_t)j * pb.n_samples, hi = lo + pb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    uint32_t n_hit = 0u, n_back = 0u;
    for (uint32_t i = i0 + lane_id(); i < i1; i += 64u)
    {
        const f4 hit = hits[i];
        const uint32_t hid = asu(hit.w);
        if (hid == MISS_ID) continue;
        const float* pd = d + 3u * (size_t)i;
        bool front;
        hit_normal(sv, hid >> sv.prim_bits, hid & ((1u << sv.prim_bits) - 1u), hit.y, hit.z, f3{pd[0], pd[1], pd[2]}, front);
        n_hit += 1u;
        n_back += front ? 0u : 1u;
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        n_hit += (uint32_t)__shfl_down((int)n_hit, off, 64);
        n_back += (uint32_t)__shfl_down((int)n_back, off, 64);
    }
    if (lane_id() == 0u)
    {
        hits_out[j] = hits_out[j] + n_hit;
        back_out[j] = back_out[j] + n_back;
    }
}
// pt_bake_probe_depth: the closest hits of the same window folded into the probes' octahedral depth maps: counts[probe][texel] += 1,
// sums[probe][texel] += (d, d * d), d = the hit's t clamped to max_distance (a miss: max_distance), texel = probe_oct_texel of the ray's
// direction.  Float addition does not associate, so a texel's adds happen in sample order: k_probe_backfaces' ownership (one wave per probe
// the window touches, launches of a call serial on one stream, no atomics), the wave walking its probe's rays of the window 64 at a time in
// sample order.  Each lane computes its ray's (texel, d); the wave then steps through the 64 entries with a wave-uniform lane read, and
// lane texel & 63 adds into its accumulator texel >> 6 (R * R <= 256: at most four a lane, chosen by a uniform branch and not by a dynamic
// register index).  The accumulators are loaded from and stored to the arrays once per launch.
__device__ __forceinline__ void depth_add(float& s0, float& s1, uint32_t& n, float dd)
{
    s0 = s0 + dd;
    s1 = s1 + dd * dd;
    n += 1u;
}
__global__ void __launch_bounds__(256) k_probe_depth_fold(const ProbeBake pb, const uint64_t first, const uint32_t count, const float* __restrict__ d,
                                                          const f4* __restrict__ hits, const uint32_t res, const float max_distance,
                                                          DProbeDepth* __restrict__ sums, uint32_t* __restrict__ counts)
{
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t p0 = (uint32_t)(first / pb.n_samples), p1 = (uint32_t)((first + count - 1u) / pb.n_samples);
    if (wave > p1 - p0) return; // (wave-uniform)
    const uint32_t j = p0 + wave;
    const uint64_t lo = (uint64_t)j * pb.n_samples, hi = lo + pb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    const uint32_t rr = res * res, lane = lane_id();
    const size_t base = (size_t)j * rr;
    float a0 = 0.0f, b0 = 0.0f, a1 = 0.0f, b1 = 0.0f, a2 = 0.0f, b2 = 0.0f, a3 = 0.0f, b3 = 0.0f;
    uint32_t n0 = 0u, n1 = 0u, n2 = 0u, n3 = 0u;
    if (lane < rr) { const DProbeDepth s = sums[base + lane]; a0 = s.m1; b0 = s.m2; n0 = counts[base + lane]; }
    if (lane + 64u < rr) { const DProbeDepth s = sums[base + lane + 64u]; a1 = s.m1; b1 = s.m2; n1 = counts[base + lane + 64u]; }
    if (lane + 128u < rr) { const DProbeDepth s = sums[base + lane + 128u]; a2 = s.m1; b2 = s.m2; n2 = counts[base + lane + 128u]; }
    if (lane + 192u < rr) { const DProbeDepth s = sums[base + lane + 192u]; a3 = s.m1; b3 = s.m2; n3 = counts[base + lane + 192u]; }
    for (uint32_t at = i0; at < i1; at += 64u)
    {
        const uint32_t i = at + lane;
        uint32_t texel = 0u;
        float dd = max_distance;
        if (i < i1)
        {
            const f4 hit = hits[i];
            if (asu(hit.w) != MISS_ID) dd = hit.x < max_distance ? hit.x : max_distance;
            const float* pd = d + 3u * (size_t)i;
            const float dir[3] = {pd[0], pd[1], pd[2]};
            texel = probe_oct_texel(dir, res); // < res * res <= 256
        }
        const uint32_t m = i1 - at < 64u ? i1 - at : 64u; // (wave-uniform)
        for (uint32_t e = 0; e < m; ++e)
        {
            const uint32_t te = (uint32_t)__builtin_amdgcn_readlane((int)texel, (int)e);
            const float de = asf((uint32_t)__builtin_amdgcn_readlane((int)asu(dd), (int)e));
            const uint32_t q = te >> 6; // (wave-uniform)
            if ((te & 63u) == lane)
            {
                if (q == 0u) depth_add(a0, b0, n0, de);
                else if (q == 1u) depth_add(a1, b1, n1, de);
                else if (q == 2u) depth_add(a2, b2, n2, de);
                else depth_add(a3, b3, n3, de);
            }
        }
    }
    if (lane < rr) { sums[base + lane] = DProbeDepth{a0, b0}; counts[base + lane] = n0; }
    if (lane + 64u < rr) { sums[base + lane + 64u] = DProbeDepth{a1, b1}; counts[base + lane + 64u] = n1; }
    if (lane + 128u < rr) { sums[base + lane + 128u] = DProbeDepth{a2, b2}; counts[base + lane + 128u] = n2; }
    if (lane + 192u < rr) { sums[base + lane + 192u] = DProbeDepth{a3, b3}; counts[base + lane + 192u] = n3; }
}
// pt_bake_probe_radiance: the integrated radiance of the same window's rays folded into the probes' octahedral radiance maps:
// counts[probe][texel] += 1, sums[probe][texel][c] += L[c].  k_probe_depth_fold's ownership and walk: one wave per probe the window touches,
// a texel's adds in sample order, lane texel & 63 adding into its accumulator set texel >> 6 (four sets of three channels and a count,
// chosen by a uniform branch), loaded from and stored to the arrays once per launch.
struct RadAcc
{
    float r, g, b;
    uint32_t n;
};
__device__ __forceinline__ void radiance_add(RadAcc& a, float lr, float lg, float lb)
{
    a.r = a.r + lr;
    a.g = a.g + lg;
    a.b = a.b + lb;
    a.n += 1u;
}
__device__ __forceinline__ RadAcc radiance_load(const float* __restrict__ sums, const uint32_t* __restrict__ counts, size_t texel)
{
    return RadAcc{sums[3u * texel], sums[3u * texel + 1u], sums[3u * texel + 2u], counts[texel]};
}
__device__ __forceinline__ void radiance_store(float* __restrict__ sums, uint32_t* __restrict__ counts, size_t texel, const RadAcc& a)
{
    sums[3u * texel] = a.r; sums[3u * texel + 1u] = a.g; sums[3u * texel + 2u] = a.b;
    counts[texel] = a.n;
}
__global__ void __launch_bounds__(256) k_probe_radiance_fold(const ProbeBake pb, const uint64_t first, const uint32_t count, const float* __restrict__ d,
                                                             const f4* __restrict__ radiance, const uint32_t res, float* __restrict__ sums,
                                                             uint32_t* __restrict__ counts)
{
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t p0 = (uint32_t)(first / pb.n_samples), p1 = (uint32_t)((first + count - 1u) / pb.n_samples);
    if (wave > p1 - p0) return; // (wave-uniform)
    const uint32_t j = p0 + wave;
    const uint64_t lo = (uint64_t)j * pb.n_samples, hi = lo + pb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    const uint32_t rr = res * res, lane = lane_id();
    const size_t base = (size_t)j * rr;
    RadAcc a0{0.0f, 0.0f, 0.0f, 0u}, a1 = a0, a2 = a0, a3 = a0;
    if (lane < rr) a0 = radiance_load(sums, counts, base + lane);
    if (lane + 64u < rr) a1 = radiance_load(sums, counts, base + lane + 64u);
    if (lane + 128u < rr) a2 = radiance_load(sums, counts, base + lane + 128u);
    if (lane + 192u < rr) a3 = radiance_load(sums, counts, base + lane + 192u);
    for (uint32_t at = i0; at < i1; at += 64u)
    {
        const uint32_t i = at + lane;
        uint32_t texel = 0u;
        f4 l4{0.0f, 0.0f, 0.0f, 0.0f};
        if (i < i1)
        {
            l4 = radiance[i];
            const float* pd = d + 3u * (size_t)i;
            const float dir[3] = {pd[0], pd[1], pd[2]};
            texel = probe_oct_texel(dir, res); // < res * res <= 256
        }
        const uint32_t m = i1 - at < 64u ? i1 - at : 64u; // (wave-uniform)
        for (uint32_t e = 0; e < m; ++e)
        {
            const uint32_t te = (uint32_t)__builtin_amdgcn_readlane((int)texel, (int)e);
            const float lr = asf((uint32_t)__builtin_amdgcn_readlane((int)asu(l4.x), (int)e));
            const float lg = asf((uint32_t)__builtin_amdgcn_readlane((int)asu(l4.y), (int)e));
            const float lb = asf((uint32_t)__builtin_amdgcn_readlane((int)asu(l4.z), (int)e));
            const uint32_t q = te >> 6; // (wave-uniform)
            if ((te & 63u) == lane)
            {
                if (q == 0u) radiance_add(a0, lr, lg, lb);
                else if (q == 1u) radiance_add(a1, lr, lg, lb);
                else if (q == 2u) radiance_add(a2, lr, lg, lb);
                else radiance_add(a3, lr, lg, lb);
            }
        }
    }
    if (lane < rr) radiance_store(sums, counts, base + lane, a0);
    if (lane + 64u < rr) radiance_store(sums, counts, base + lane + 64u, a1);
    if (lane + 128u < rr) radiance_store(sums, counts, base + lane + 128u, a2);
    if (lane + 192u < rr) radiance_store(sums, counts, base + lane + 192u, a3);
}
// pt_probe_radiance_prefilter: one workgroup per (probe, level) of R * R lanes rounded up to whole waves, one lane per output texel.  The
// probe's means and the map's direction / solid-angle table are staged in LDS once (32 bytes a texel, sized at the launch: 8 KiB at R = 16,
// 2 KiB at R = 8, so that LDS never holds the single-wave workgroups of small maps below eight waves per SIMD); the quadrature of a lane then
// walks the input texels serially, in the order that defines the sum, and every lane reads the same LDS address at a time: a broadcast.  No
// atomics.
struct PrefilterArgs
{
    uint32_t res, n_levels;
    float alpha[8];
};
__global__ void __launch_bounds__(256) k_probe_radiance_prefilter(const PrefilterArgs a, const float* __restrict__ sums, const uint32_t* __restrict__ counts,
                                                                  f4* __restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) f4 s_prefilter[]; // rr entries of {dir, omega}, then rr of {mean, filled}
    const uint32_t rr = a.res * a.res;
    f4* const s_dirw = s_prefilter;
    f4* const s_mean = s_prefilter + rr;
    const uint32_t probe = blockIdx.x / a.n_levels, level = blockIdx.x - probe * a.n_levels, t = threadIdx.x;
    if (t < rr) // (blockDim.x >= rr)
    {
        float dir[3], omega;
        probe_oct_dir(t, a.res, dir, &omega);
        s_dirw[t] = f4{dir[0], dir[1], dir[2], omega};
        const size_t at = (size_t)probe * rr + t;
        const float s3[3] = {sums[3u * at], sums[3u * at + 1u], sums[3u * at + 2u]};
        s_mean[t] = probe_radiance_mean(s3, counts[at]);
    }
    __syncthreads();
    if (t >= rr) return;
    table[(size_t)blockIdx.x * rr + t] = probe_prefilter_texel(s_dirw, s_mean, rr, a.alpha[level], t);
}

// ------------------------------------------------------------------------------------------------ adaptive selection (PT_FLAG_ADAPTIVE)
// (the criterion itself, adaptive_active, is pt_types.h's: the texel selection of pt_lightmap.hip and the host share it)
// Two passes, no atomic append: the list comes out in ascending pixel order whatever the scheduling.  Block b owns local pixels
// [b * kSelectPerBlock, (b + 1) * kSelectPerBlock), thread i of it pixels b * kSelectPerBlock + j * 256 + i (j = 0..3).
// k_adaptive_count: active pixels per block -> counts[b]; a bad count anywhere sets header[1].
__global__ void __launch_bounds__(256) k_adaptive_count(const f4* __restrict__ accum, const float* __restrict__ moments, const uint32_t n_pixels,
                                                        const AdaptiveCrit cr, uint32_t* counts, uint32_t* header)
{
    __shared__ uint32_t sh_cnt[4];
    const uint32_t base = blockIdx.x * kSelectPerBlock;
    uint32_t mine = 0u;
    bool any_bad = false;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerBlock / 256u; ++j)
    {
        const uint32_t p = base + j * 256u + threadIdx.x;
        if (p >= n_pixels) break;
        uint32_t n_p;
        bool bad;
        mine += adaptive_active(accum[p], moments[p], cr, n_p, bad) ? 1u : 0u;
        any_bad |= bad;
    }
    if (any_bad) atomicOr(header + 1, 1u);
    uint32_t w = mine;
    for (int off = 32; off > 0; off >>= 1) w += (uint32_t)__shfl_xor((int)w, off);
    if (lane_id() == 0u) sh_cnt[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0u) counts[blockIdx.x] = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
}
// k_adaptive_write: the block's offset is the sum of the counts of the blocks before it; each group of 256 pixels is compacted with
// one ballot per wave, mbcnt for a lane's rank in its wave and the waves' counts in LDS.  The last block writes the total to header[0].
__global__ void __launch_bounds__(256) k_adaptive_write(const f4* __restrict__ accum, const float* __restrict__ moments, const uint32_t n_pixels,
                                                        const AdaptiveCrit cr, const uint32_t* __restrict__ counts, uint2* list, uint32_t* header)
{
    __shared__ uint32_t sh_sum[4];
    __shared__ uint32_t sh_wave[kSelectPerBlock / 256u][4];
    const uint32_t wid = threadIdx.x >> 6;
    uint32_t before = 0u;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256u) before += counts[b];
    for (int off = 32; off > 0; off >>= 1) before += (uint32_t)__shfl_xor((int)before, off);
    if (lane_id() == 0u) sh_sum[wid] = before;
    const uint32_t base = blockIdx.x * kSelectPerBlock;
    bool act[kSelectPerBlock / 256u];
    uint32_t np[kSelectPerBlock / 256u];
    uint64_t m[kSelectPerBlock / 256u];
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerBlock / 256u; ++j)
    {
        const uint32_t p = base + j * 256u + threadIdx.x;
        bool bad;
        np[j] = 0u;
        act[j] = p < n_pixels && adaptive_active(accum[p], moments[p], cr, np[j], bad);
        m[j] = __ballot(act[j]);
        if (lane_id() == 0u) sh_wave[j][wid] = (uint32_t)__popcll(m[j]);
    }
    __syncthreads();
    uint32_t off = sh_sum[0] + sh_sum[1] + sh_sum[2] + sh_sum[3];
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerBlock / 256u; ++j)
    {
        uint32_t pos = off;
        for (uint32_t w2 = 0; w2 < wid; ++w2) pos += sh_wave[j][w2];
        if (act[j]) list[pos + mbcnt64(m[j])] = uint2{base + j * 256u + threadIdx.x, np[j]};
        off += sh_wave[j][0] + sh_wave[j][1] + sh_wave[j][2] + sh_wave[j][3];
    }
    if (blockIdx.x + 1u == gridDim.x && threadIdx.x == 0u) header[0] = off;
}

// ------------------------------------------------------------------------------------------------ probes
__global__ void k_sobol_probe(uint32_t n_points, uint32_t n, const uint32_t* index, const uint32_t* seed, float* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ss_sobol(n_points, index[i], seed[i], &out[2 * i], &out[2 * i + 1]);
}
__global__ void k_math_probe(int fn, uint32_t n, const float* a, const float* b, float* o0, float* o1, uint64_t seed)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (fn)
    {
    case 0: sincos_det(a[i], &o0[i], &o1[i]); break;
    case 1: o0[i] = exp_det(a[i]); break;
    case 2: o0[i] = ln_det(a[i]); break;
    case 3: o0[i] = hypot_det(a[i], b[i]); break;
    case 4: o0[i] = a[i] / b[i]; break;
    case 5: o0[i] = sqrtf(a[i]); break;
    case 6: o0[i] = tan_det(a[i]); break;
    case 8: o0[i] = atan2_det(a[i], b[i]); break;
    case 9: o0[i] = asin_det(a[i]); break;
    case 7:
    {
        Stream r{stream_key(seed, asu(a[i]), asu(b[i])), 0u};
        o0[i] = asf(r.u32());
        o1[i] = r.f32();
        break;
    }
    }
}
__global__ void k_material_probe(const SceneView sv, int material, uint32_t n, const float* incoming, const float* normal, const uint8_t* front,
                                 const uint32_t* pixel, const uint32_t* sample, uint32_t draws, uint64_t seed, float* out9)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MatView m = load_material(sv.materials, (uint32_t)material);
    Stream rng{stream_key(seed, pixel[i], sample[i]), draws};
    const f3 in{incoming[3 * i], incoming[3 * i + 1], incoming[3 * i + 2]}, nn{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
    const bool ff = front[i] != 0;
    const f3 wo = mat_scatter(m, rng, in, nn, ff);
    const BsdfSample bp = mat_bsdf_pdf(m, -in, wo, nn, ff);
    float* o = out9 + 9 * i;
    o[0] = wo.x; o[1] = wo.y; o[2] = wo.z;
    o[3] = bp.bsdf.x; o[4] = bp.bsdf.y; o[5] = bp.bsdf.z;
    o[6] = bp.pdf;
    o[7] = mat_weakening(m.kind, wo, nn);
    o[8] = (float)(rng.k - draws);
}

// VolumeScatter::scatter (volume.rs:83-97) and VolumeAbsorption::get_transmission (volume.rs:113) of one material's volume, as the
// shading pass evaluates them: out9[i*9..] = scattered (0/1), t, direction xyz, transmission over dist[i] rgb, draws consumed
__global__ void k_volume_probe(const SceneView sv, int material, uint32_t n, const float* incoming, const float* t_max, const float* dist,
                               const uint32_t* pixel, const uint32_t* sample, uint32_t draws, uint64_t seed, float* out9)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DMaterial& dm = sv.materials[material];
    Stream rng{stream_key(seed, pixel[i], sample[i]), draws};
    const f3 rd{incoming[3 * i], incoming[3 * i + 1], incoming[3 * i + 2]};
    float* o = out9 + 9 * i;
    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 0.0f; o[4] = 0.0f;
    if (dm.vol_flags & 2u)                                                  // as k_shade_surface's media loop
    {
        const float t = -ln_det(rng.f32()) / dm.vol_c;
        if (!(t > t_max[i]))
        {
            const f3 d = hg_direction(dm.vol_g, rng, rd);
            o[0] = 1.0f; o[1] = t; o[2] = d.x; o[3] = d.y; o[4] = d.z;
        }
    }
    f3 w{1.0f, 1.0f, 1.0f};
    if (dm.vol_flags & 1u) w = beer_lambert(f3{dm.vol_abs[0], dm.vol_abs[1], dm.vol_abs[2]}, dist[i]);
    o[5] = w.x; o[6] = w.y; o[7] = w.z;
    o[8] = (float)(rng.k - draws);
}

// MaterialTrait::get_bsdf_pdf as next-event estimation calls it (integrator.rs:41-46): at a caller-chosen outgoing direction, which is the
// light's and need not lie anywhere near the lobe.  out4[i*4..] = bsdf rgb, pdf of mat_bsdf_pdf(m, -incoming, outgoing, normal, front)
__global__ void k_bsdf_probe(const SceneView sv, int material, uint32_t n, const float* incoming, const float* outgoing, const float* normal,
                             const uint8_t* front, float* out4)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MatView m = load_material(sv.materials, (uint32_t)material);
    const f3 in{incoming[3 * i], incoming[3 * i + 1], incoming[3 * i + 2]}, wo{outgoing[3 * i], outgoing[3 * i + 1], outgoing[3 * i + 2]};
    const f3 nn{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]};
    const BsdfSample bp = mat_bsdf_pdf(m, -in, wo, nn, front[i] != 0);
    float* o = out4 + 4 * i;
    o[0] = bp.bsdf.x; o[1] = bp.bsdf.y; o[2] = bp.bsdf.z;
    o[3] = bp.pdf;
}

// ------------------------------------------------------------------------------------------------ denoiser guides (pt_render_guides)
// The camera ray of sample rp.first_sample of EVERY local pixel (no active rectangle: a ray outside it is answered by the root-box test)
// as one ray of a hook queue, ray index = local pixel: exactly the ray k_generate<CAM> makes for that (pixel, sample).
template <uint32_t CAM>
__global__ void __launch_bounds__(256) k_guide_rays(const RenderParams rp, const CameraArg<CAM> cam, const RayQueue rq, uint32_t* __restrict__ n_and_heads)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u) n_and_heads[0] = rp.local_pixels;
    if (i >= rp.local_pixels) return;
    const uint32_t ly = fastdiv(i, rp.div_width), x = i - ly * rp.width;
    f3 o;
    const f3 dir = primary_ray<CAM>(rp, cam, x, global_row(rp, ly), rp.first_sample, &o);
    rq.a[i] = f4{o.x, o.y, o.z, __builtin_inff()};
    rq.b[i] = f4{dir.x, dir.y, dir.z, asf(i)};
}

// the unit hook of the surface colour, over surface_colour (pt_materials.h) as the TEX shading passes and the guides are
__device__ __forceinline__ f3 surface_colour_at(const SceneView& sv, const TexView& tex, uint32_t inst, uint32_t tri, float u, float v)
{
    const DMaterial& dm = sv.materials[sv.instances[inst].material];
    return surface_colour(tex, dm.texture, f3{dm.colour[0], dm.colour[1], dm.colour[2]}, tri, u, v);
}
// ---- one hop of the followed chains (pt_api.cpp, walk_chains), stated once for the guides and the baked view.  chain_hop<FIRST> is what
// their kernels share: the slot's hit, ray and pixel, the colour product and t sum out of state[pixel], whether the chain goes on, its
// parked state, its next ray and the append to `next`.  The Ending says what a chain that stops here leaves: miss(first, slot, pixel, d)
// for a ray that left the scene, surface(ChainEnd) for a surface the chain is not followed through (or the hop cap); both return a value
// and store(pixel, value) puts it away at the hop's one tail.  (Endings that stored in miss() and in surface() themselves cost the probe
// ending 28 registers and two waves per SIMD: profiles/r25_chain_hop.md.)  An ending with kFirstHit is also told, at hop 0, the hit id of every
// slot: first_hit(pixel, id), before anything else is decided.
struct ChainEnd // the surface a chain ends on
{
    uint32_t slot, px, inst, tri, kind;
    f4 hit;          // the slot's: this hop's t | u | v | id
    float t;         // summed over the hops where the ending asks (kSumT)
    f3 d, c, p, nrm; // the ray's direction, the colour product with this surface in it, the hit position, the face-forwarded world normal
    bool front;
};
// the lanes of a wave that go on append their next rays: one ballot and one atomic on the queue's count word per wave, the lane's rank by
// mbcnt.  Every lane of the block must call it (no early exit before it), so that lane 0 of each wave can reserve for the others
__device__ __forceinline__ void chain_append(const ChainHop& a, bool go_on, const f4& next_a, const f4& next_b)
{
    const uint64_t m = __ballot(go_on);
    if (m == 0ull) return;
    uint32_t base = 0u;
    if (lane_id() == 0u) base = atomicAdd(a.n_next, (uint32_t)__popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (go_on)
    {
        const uint32_t pos = base + mbcnt64(m); // < the chains that go on <= n <= a.cap, the queues' slots
        a.next.a[pos] = next_a;
        a.next.b[pos] = next_b;
    }
}
template <bool FIRST, class Ending>
__device__ __forceinline__ void chain_hop(const SceneView& sv, const TexView& tex, const ChainHop& a, const Ending& e)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = min(*a.n_in, a.cap);
    bool go_on = false;
    f4 next_a{}, next_b{};
    if (i < n)
    {
        const f4 hit = a.hits[i];
        const f4 rb = a.in.b[i];
        const uint32_t px = asu(rb.w);
        const f3 d = xyz(rb);
        f3 out{};
        const uint32_t hid = asu(hit.w);
        if constexpr (FIRST && Ending::kFirstHit) e.first_hit(px, hid); // every ray of the window, whatever becomes of its chain
        if (hid == MISS_ID) out = e.miss(FIRST, i, px, d);
        else
        {
            // (one gather after the other, each behind a compiler barrier, an ending's own gathers last: hoisting all their loads to the top
            // costs scratch at 64 VGPRs)
            const uint32_t inst = hid >> sv.prim_bits, tri = hid & ((1u << sv.prim_bits) - 1u);
            const DMaterial& dm = sv.materials[sv.instances[inst].material];
            f3 c = surface_colour(tex, dm.texture, f3{dm.colour[0], dm.colour[1], dm.colour[2]}, tri, hit.y, hit.z);
            float t = hit.x;
            if (!FIRST)
            {
                const f4 s = a.state[px];
                c = xyz(s) * c;
                if (Ending::kSumT) t = s.w + t;
            }
            const uint32_t kind = dm.kind;
            __asm__ volatile("" ::: "memory");
            bool front;
            const f3 nrm = hit_normal(sv, inst, tri, hit.y, hit.z, d, front);
            const FollowDir f = guide_follow_dir(kind, dm.ior, d, nrm, front);
            go_on = f.followed && a.hop < a.max_hops;
            __asm__ volatile("" ::: "memory");
            const f3 p = fma3(d, bc3(hit.x), xyz(a.in.a[i]));
            if (go_on)
            {
                a.state[px] = f4{c.x, c.y, c.z, t};
                next_a = f4{p.x, p.y, p.z, __builtin_inff()};
                next_b = f4{f.wo.x, f.wo.y, f.wo.z, asf(px)};
            }
            else out = e.surface(ChainEnd{i, px, inst, tri, kind, hit, t, d, c, p, nrm, front});
        }
        if (!go_on) e.store(px, out);
    }
    chain_append(a, go_on, next_a, next_b);
}
// ---- the guides (pt_render_guides, pt_render_guides_followed, pt_accumulate_albedo[_followed]; include/pt_api.h states the chain)
// Hop a.hop of every live chain: one thread per ray slot of the `in` hook queue (slot = local pixel at hop 0, compacted afterwards; the
// ray's pixel rides in rq.b[].w, its origin in rq.a[]), its closest hit in hits[slot].  A chain that ends here (a miss, a rough surface,
// the hop cap) writes its pixel's final guides: position r.at(t) | t as the render keeps it (r.at(1e5) | 1e5 for a miss,
// integrator.rs:156; t summed over the hops), the face-forwarded world shading normal of the hit (HitInfo's, primitive.rs:161-165 +
// tlas.rs:105; 0 for a miss), the hit's model (BLAS index, its hop count in bits 31..28; MISS_ID for a miss: the low byte is the id byte
// of main.rs:206), the world-TLAS leaf of the hit in allocation order (the index of pt_tlas_instances(ctx, 0, ..); MISS_ID for a miss),
// which pt_frame_moving reprojects a moved instance's pixels by, the albedo product (0 for a miss) and the hop count.  ACCUM: it adds its
// albedo product and 1 to the pixel's mean-albedo sums instead, one binary32 add per component and (1, 1, 1) for a miss, so that the
// background passes the demodulation undivided; one thread owns a pixel and launches follow each other in sample order on one stream: no
// atomics, and the order of a pixel's adds is the order of its samples.  A chain that goes on parks its running albedo product | t sum in
// state[pixel] and appends ray hop + 1 to the `next` queue: one ballot and one atomic on the queue's count word per wave, the lane's rank
// by mbcnt.  That word is what the next hop's k_closest and k_guide_follow read as their ray count, so nothing comes back to the host
// between hops.  Where a chain lands in `next` shows in nothing it writes: every output is addressed by pixel.
// First-hit guides are the chains of max_hops = 0.  At the last hop (a.hop == a.max_hops) no lane goes on, so `next` and n_next are never
// dereferenced, and hop 0 never reads `state`: the host passes null for what a launch cannot touch (all three at max_hops = 0).
template <bool ACCUM>
struct GuideEnding
{
    const SceneView& sv;
    const FollowArgs& a;
    static constexpr bool kSumT = true; // position.w is the t of the whole chain
    static constexpr bool kFirstHit = false;
    __device__ __forceinline__ f3 miss(bool first, uint32_t i, uint32_t px, const f3& d) const
    {
        if (!ACCUM)
        {
            const f3 far = fma3(d, bc3(1e5f), xyz(a.in.a[i]));
            a.position[px] = f4{far.x, far.y, far.z, 1e5f};
            a.normal[px] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            a.model[px] = MISS_ID;
            a.instance[px] = MISS_ID;
        }
        return bc3(ACCUM ? 1.0f : 0.0f);
    }
    __device__ __forceinline__ f3 surface(const ChainEnd& h) const
    {
        if (!ACCUM)
        {
            a.position[h.px] = f4{h.p.x, h.p.y, h.p.z, h.t};
            a.normal[h.px] = f4{h.nrm.x, h.nrm.y, h.nrm.z, 0.0f};
            a.model[h.px] = sv.instances[h.inst].blas | (a.hop << 28);
            a.instance[h.px] = h.inst;
        }
        return h.c;
    }
    __device__ __forceinline__ void store(uint32_t px, const f3& c) const
    {
        if (ACCUM)
        {
            const f4 s = a.sum[px];
            a.sum[px] = f4{s.x + c.x, s.y + c.y, s.z + c.z, s.w + 1.0f};
        }
        else
        {
            a.albedo[px] = f4{c.x, c.y, c.z, 0.0f};
            a.hops[px] = (uint8_t)a.hop;
        }
    }
};
template <bool ACCUM, bool FIRST>
__global__ void __launch_bounds__(256, 8) k_guide_follow(const SceneView sv, const TexView tex, const FollowArgs a)
{
    chain_hop<FIRST>(sv, tex, a, GuideEnding<ACCUM>{sv, a});
}
// ---- the baked view (pt_render_baked; include/pt_api.h states the sample).  The same chains with another ending: a chain that ends adds its
// baked sample B and 1 to sum[pixel], one binary32 add per component, no finite check and no clamp.  B = the running colour product R on a
// light; R * the lightmap at the hit on a front face of a leaf that has a map; R * unlit on any other surface; the environment (or the
// constant ambient) of a miss, times R of the hop before unless the camera ray itself missed.  What lights a final surface beside that is the
// ending's four axes, decided on the host (pt_api.cpp, baked_light) and handed over as a BakedKey:
// GRID, with a probe grid set (pt_set_probe_grid): a final surface that no map lights is lit by the grid where the grid is lit, by unlit where
// not; P and n are the guides' (the hit position, the face-forwarded unperturbed normal).
// VIS, with depth set on the grid (pt_set_probe_grid_depth): the grid's lookups are the ones with visibility.
// SPEC, with radiance set on the grid (pt_set_probe_grid_radiance): a chain that ends on GGX metal, on either face, reflects the grid's
// prefiltered radiance, B = R * S, where probe_grid_specular is lit, whether or not a map lights the surface (a map holds irradiance, which a
// metal does not reflect diffusely); where it is not lit, and on every other kind, the ending is what it is without SPEC.  The metal branch
// comes first and returns, so a lane holds one lookup's registers at a time.  P, n and d are ChainEnd's; the alpha is the hit's (surface_alpha).
// DIR, with a gradient set and a normal-mapped material in the scene (pt_set_lightmap_directional): n' = shading_normal of the hit, delta =
// n' - n (zero by construction without a normal texture); a front face of a mapped leaf reads lightmap_at_directional, and the grid takes n'.
// n' is gathered behind a barrier of its own, after the hop's gathers and before the map's, so one lookup's registers are live at a time.
// VIS and SPEC are the grid's, so the points of the axes that are kernels are the ten of baked_variant_ok.
constexpr bool baked_variant_ok(uint32_t grid, uint32_t vis, uint32_t spec, uint32_t dir) { return grid || (!vis && !spec); }
// The plain ending runs at eight waves per SIMD.  The corner of a grid being evaluated and the one in flight are 56 registers and the probe
// ending must not spill, so with a grid the bounds leave 128; it takes 66 (seven waves per SIMD) and no scratch, and every DIR ending fits
// under the same bounds (profiles/r30_baked_axes.md has the registers of all ten)
constexpr int baked_min_blocks(bool grid, bool dir) { return grid || dir ? 4 : 8; }
// The value B of a chain that ends, stated once for the endings that differ in where B goes: the baked view's (BakedEnding, Args = BakedArgs:
// added into the pixel's sums) and the baked rays' (BakedRayEnding, Args = BakedRayArgs: stored per ray).  Args has the hop's ChainHop, env and unlit.
template <class Args, bool GRID, bool VIS, bool SPEC, bool DIR>
struct BakedValue
{
    const SceneView& sv;
    const TexNView& texn;
    const BakedLight& light; // a variant reads the views of its axes and no other
    const Args& a;
    // nothing here reads t, and carrying its sum through both barriers costs the probe ending's later hops a 67th register (the parent's 66 are
    // the bound: profiles/r25_chain_hop.md), so state[pixel].w holds one hop's t here
    static constexpr bool kSumT = false;
    __device__ __forceinline__ f3 miss(bool first, uint32_t i, uint32_t px, const f3& d) const
    {
        const f3 b = a.env.w ? env_lookup(a.env, d) : f3{0.006f, 0.006f, 0.006f};
        return first ? b : xyz(a.state[px]) * b;
    }
    __device__ __forceinline__ f3 surface(const ChainEnd& h) const
    {
        if constexpr (SPEC)
        {
            if (h.kind == MAT_GGX_METAL)
            {
                // the alpha AT THE HIT: the material's own without a roughness map (pt_set_material_roughness_texture), surface_alpha's with
                // one; its four texels are gathered and blended before the barrier, so one lookup's registers are live at a time
                const DMaterial& dm = sv.materials[sv.instances[h.inst].material];
                const float alpha = surface_alpha(texn, dm.roughness_texture, dm.alpha, h.tri, h.hit.y, h.hit.z);
                __asm__ volatile("" ::: "memory");
                f3 s;
                if (probe_grid_specular<VIS>(light.grid, light.rad, fma3(h.d, bc3(h.hit.x), xyz(a.in.a[h.slot])), h.nrm, h.d, alpha, &s, VIS ? &light.depth : nullptr))
                    return h.c * s;
            }
        }
        if (h.kind == MAT_EMISSIVE) return h.c;
        f3 l{a.unlit[0], a.unlit[1], a.unlit[2]};
        bool mapped = false;
        f3 np = h.nrm;
        if constexpr (DIR)
        {
            if (GRID || h.front)
            {
                __asm__ volatile("" ::: "memory");
                f3 delta;
                np = shading_normal_delta(sv.tri_shade, sv.instances, sv.materials, texn, h.inst, h.tri, h.hit.y, h.hit.z, h.d, h.nrm, &delta);
                if (h.front)
                {
                    __asm__ volatile("" ::: "memory");
                    const f3 m = lightmap_at_directional(light.lm, light.ld, h.inst, h.tri, h.hit.y, h.hit.z, delta, &mapped);
                    if (mapped) l = m;
                }
            }
        }
        else if (h.front) // the bake lit the front side only
        {
            const f3 m = lightmap_at(light.lm, h.inst, h.tri, h.hit.y, h.hit.z, &mapped);
            if (mapped) l = m;
        }
        if (GRID && !mapped) // the grid lights what no map lights, where it is lit itself
        {
            // the grid's corners after the map's four texels, and P made again behind the barrier: h.p kept across the map's gather is five
            // registers more
            __asm__ volatile("" ::: "memory");
            f3 irr;
            if (probe_grid_lookup<VIS>(light.grid, fma3(h.d, bc3(h.hit.x), xyz(a.in.a[h.slot])), np, &irr, VIS ? &light.depth : nullptr)) l = irr;
        }
        return h.c * l;
    }
};
template <bool GRID, bool VIS, bool SPEC, bool DIR>
struct BakedEnding : BakedValue<BakedArgs, GRID, VIS, SPEC, DIR>
{
    static constexpr bool kFirstHit = false;
    __device__ __forceinline__ void store(uint32_t px, const f3& b) const
    {
        const f4 s = this->a.sum[px];
        this->a.sum[px] = f4{s.x + b.x, s.y + b.y, s.z + b.z, s.w + 1.0f};
    }
};
template <bool FIRST, bool GRID, bool VIS, bool SPEC, bool DIR>
__global__ void __launch_bounds__(256, baked_min_blocks(GRID, DIR)) k_baked_follow(const SceneView sv, const TexNView tex, const BakedLight light, const BakedArgs a)
{
    static_assert(baked_variant_ok(GRID, VIS, SPEC, DIR), "no such ending");
    chain_hop<FIRST>(sv, tex, a, BakedEnding<GRID, VIS, SPEC, DIR>{{sv, tex, light, a}});
}
// ---- baked rays (pt_baked_rays, the gather of pt_bake_lightmap_gather): the baked view's chains over a window of caller rays, the queue's
// "pixel" word being the ray's index in the window.  The value is BakedValue's; a chain that ends STORES out[ray] = B | its hop, with no
// arithmetic on B, and hop 0 writes the id byte of every ray of the window: the low byte of the first hit's model (BLAS) index as the path
// tracer's first_id keeps it, 255 for a miss.  Either output may be null.  The bounds are k_baked_follow's: the ending's registers are the
// same functions' and the tail is a store where the view's is a load, four adds and a store (profiles/r35_lightmap_gather.md has the report).
template <bool GRID, bool VIS, bool SPEC, bool DIR>
struct BakedRayEnding : BakedValue<BakedRayArgs, GRID, VIS, SPEC, DIR>
{
    static constexpr bool kFirstHit = true;
    __device__ __forceinline__ void first_hit(uint32_t ray, uint32_t hid) const
    {
        if (this->a.id) this->a.id[ray] = hid == MISS_ID ? (uint8_t)255u : (uint8_t)(this->sv.instances[hid >> this->sv.prim_bits].blas & 0xffu);
    }
    __device__ __forceinline__ void store(uint32_t ray, const f3& b) const
    {
        if (this->a.out) this->a.out[ray] = f4{b.x, b.y, b.z, (float)this->a.hop};
    }
};
template <bool FIRST, bool GRID, bool VIS, bool SPEC, bool DIR>
__global__ void __launch_bounds__(256, baked_min_blocks(GRID, DIR)) k_baked_rays(const SceneView sv, const TexNView tex, const BakedLight light, const BakedRayArgs a)
{
    static_assert(baked_variant_ok(GRID, VIS, SPEC, DIR), "no such ending");
    chain_hop<FIRST>(sv, tex, a, BakedRayEnding<GRID, VIS, SPEC, DIR>{{sv, tex, light, a}});
}
// unit hook of the directional lookup: rgb, mapped = lightmap_at_directional with delta = n' - n of the hit under the ray direction dir
__global__ void __launch_bounds__(256) k_lightmap_lookup_directional(const SceneView sv, const TexNView tex, const LmView lm, const LmDirView ld, const uint32_t n,
                                                                     const uint32_t* __restrict__ instance, const uint32_t* __restrict__ tri,
                                                                     const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ dir,
                                                                     float* __restrict__ rgb, uint8_t* __restrict__ mapped)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 d{dir[3u * (size_t)i], dir[3u * (size_t)i + 1u], dir[3u * (size_t)i + 2u]};
    bool front, has;
    const f3 nrm = unperturbed_normal(sv.tri_shade, sv.instances, instance[i], tri[i], u[i], v[i], d, front);
    f3 delta;
    (void)shading_normal_delta(sv.tri_shade, sv.instances, sv.materials, tex, instance[i], tri[i], u[i], v[i], d, nrm, &delta);
    const f3 c = lightmap_at_directional(lm, ld, instance[i], tri[i], u[i], v[i], delta, &has);
    rgb[3u * (size_t)i] = c.x; rgb[3u * (size_t)i + 1u] = c.y; rgb[3u * (size_t)i + 2u] = c.z;
    mapped[i] = has ? 1u : 0u;
}
// unit hook of the probe grid's lookup (pt_probe_grid_lookup): rgb, lit = probe_grid_lookup<VIS>, VIS with depth set on the grid
template <bool VIS>
__global__ void __launch_bounds__(256, 4) k_probe_grid_lookup(const ProbeGridView grid, const ProbeDepthView depth, const uint32_t n, const float* __restrict__ position,
                                                              const float* __restrict__ normal, float* __restrict__ rgb, uint8_t* __restrict__ lit)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* pp = position + 3u * (size_t)i;
    const float* pn = normal + 3u * (size_t)i;
    f3 c;
    const bool has = probe_grid_lookup<VIS>(grid, f3{pp[0], pp[1], pp[2]}, f3{pn[0], pn[1], pn[2]}, &c, &depth);
    rgb[3u * (size_t)i] = c.x; rgb[3u * (size_t)i + 1u] = c.y; rgb[3u * (size_t)i + 2u] = c.z;
    lit[i] = has ? 1u : 0u;
}
// unit hook of the reflection probes' lookup (pt_probe_grid_specular): rgb, lit = probe_grid_specular<VIS>, VIS with depth set on the grid
template <bool VIS>
__global__ void __launch_bounds__(256, 4) k_probe_grid_specular(const ProbeGridView grid, const ProbeRadianceView rad, const ProbeDepthView depth, const uint32_t n,
                                                                const float* __restrict__ position, const float* __restrict__ normal,
                                                                const float* __restrict__ incoming, const float* __restrict__ alpha, float* __restrict__ rgb,
                                                                uint8_t* __restrict__ lit)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* pp = position + 3u * (size_t)i;
    const float* pn = normal + 3u * (size_t)i;
    const float* pi = incoming + 3u * (size_t)i;
    f3 c;
    const bool has = probe_grid_specular<VIS>(grid, rad, f3{pp[0], pp[1], pp[2]}, f3{pn[0], pn[1], pn[2]}, f3{pi[0], pi[1], pi[2]}, alpha[i], &c, &depth);
    rgb[3u * (size_t)i] = c.x; rgb[3u * (size_t)i + 1u] = c.y; rgb[3u * (size_t)i + 2u] = c.z;
    lit[i] = has ? 1u : 0u;
}
// unit hook of the lightmap lookup: rgb, mapped = lightmap_at
__global__ void __launch_bounds__(256) k_lightmap_lookup(const LmView lm, const uint32_t n, const uint32_t* __restrict__ instance, const uint32_t* __restrict__ tri,
                                                         const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ rgb,
                                                         uint8_t* __restrict__ mapped)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool has;
    const f3 c = lightmap_at(lm, instance[i], tri[i], u[i], v[i], &has);
    rgb[3u * (size_t)i] = c.x; rgb[3u * (size_t)i + 1u] = c.y; rgb[3u * (size_t)i + 2u] = c.z;
    mapped[i] = has ? 1u : 0u;
}
// unit hook of guide_follow_dir: out4 = wo | followed
__global__ void __launch_bounds__(256) k_guide_follow_dir(const SceneView sv, const int material, const uint32_t n, const float* __restrict__ incoming,
                                                          const float* __restrict__ normal, const uint8_t* __restrict__ front, float* __restrict__ out4)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DMaterial& dm = sv.materials[material];
    const FollowDir f = guide_follow_dir(dm.kind, dm.ior, f3{incoming[3 * i], incoming[3 * i + 1], incoming[3 * i + 2]},
                                         f3{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]}, front[i] != 0);
    float* o = out4 + 4 * (size_t)i;
    o[0] = f.wo.x; o[1] = f.wo.y; o[2] = f.wo.z;
    o[3] = f.followed ? 1.0f : 0.0f;
}
__global__ void __launch_bounds__(256) k_surface_colour(const SceneView sv, const TexView tex, const uint32_t n, const uint32_t* __restrict__ instance,
                                                        const uint32_t* __restrict__ tri, const float* __restrict__ u, const float* __restrict__ v,
                                                        float* __restrict__ rgb)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f3 c = surface_colour_at(sv, tex, instance[i], tri[i], u[i], v[i]);
    rgb[3u * (size_t)i] = c.x; rgb[3u * (size_t)i + 1u] = c.y; rgb[3u * (size_t)i + 2u] = c.z;
}
// unit hook of surface_alpha (pt_surface_roughness): alpha[i] <- surface_roughness_at (pt_materials.h), as the host evaluation
__global__ void __launch_bounds__(256) k_surface_roughness(const SceneView sv, const TexView tex, const uint32_t n, const uint32_t* __restrict__ instance,
                                                           const uint32_t* __restrict__ tri, const float* __restrict__ u, const float* __restrict__ v,
                                                           float* __restrict__ alpha)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    alpha[i] = surface_roughness_at(sv.instances, sv.materials, tex, instance[i], tri[i], u[i], v[i]);
}
// unit hook of shading_normal: out4 = world shading normal | front
__global__ void __launch_bounds__(256) k_shading_normal(const SceneView sv, const TexNView tex, const uint32_t n, const uint32_t* __restrict__ instance,
                                                        const uint32_t* __restrict__ tri, const float* __restrict__ u, const float* __restrict__ v,
                                                        const float* __restrict__ dir, float* __restrict__ out4)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool front;
    const f3 nn = shading_normal(sv.tri_shade, sv.instances, sv.materials, tex, instance[i], tri[i], u[i], v[i],
                                 f3{dir[3u * (size_t)i], dir[3u * (size_t)i + 1u], dir[3u * (size_t)i + 2u]}, front);
    float* o = out4 + 4u * (size_t)i;
    o[0] = nn.x; o[1] = nn.y; o[2] = nn.z;
    o[3] = front ? 1.0f : 0.0f;
}

} // namespace

// ================================================================================================ launchers
// A launcher decides each axis of its kernel's variant once, as a plain integer, and turns the integers into template arguments here:
// f(std::integral_constant<uint32_t, value>{}) for a value below N ...
template <uint32_t N, typename F>
static void pick(uint32_t value, F&& f)
{
    if constexpr (N > 1u)
        if (value != N - 1u) return pick<N - 1u>(value, f);
    f(std::integral_constant<uint32_t, N - 1u>{});
}
// ... and f(constant...) for one value per axis, value[k] below the k-th N
template <uint32_t... N, typename F, typename... C>
static void pick_axes(const uint32_t (&value)[sizeof...(N)], F&& f, C... held)
{
    [[maybe_unused]] constexpr uint32_t bound[] = {N...};
    constexpr size_t k = sizeof...(C);
    if constexpr (k == sizeof...(N)) f(held...);
    else pick<bound[k]>(value[k], [&](auto c) { pick_axes<N...>(value, f, held..., c); });
}

// The launch log (pt_kernels.h): the thread's current one, and the row a keyed launcher writes where it has decided its axes.
static thread_local LaunchLog* t_launch_log = nullptr;
LaunchLogScope::LaunchLogScope(LaunchLog* log) : prev(t_launch_log) { t_launch_log = log; }
LaunchLogScope::~LaunchLogScope() { t_launch_log = prev; }
template <size_t N>
static void log_launch(uint32_t launcher, uint32_t b, const uint32_t (&value)[N])
{
    static_assert(N <= kLaunchAxes, "");
    if (!t_launch_log) return;
    LaunchRow row{launcher, b, {}};
    for (size_t k = 0; k < N; ++k) row.axis[k] = value[k];
    t_launch_log->push_back(row);
}
// ... pick_axes over the launcher's bounds (launch_axes<LAUNCHER>, an integer_sequence), with the row logged: the values the log holds are
// the ones the kernel is picked by
template <uint32_t... N, typename F>
static void pick_axes_of(std::integer_sequence<uint32_t, N...>, const uint32_t (&value)[sizeof...(N)], F&& f)
{
    pick_axes<N...>(value, f);
}
template <uint32_t LAUNCHER, uint32_t... N, typename F>
static void pick_logged(std::integer_sequence<uint32_t, N...> axes, uint32_t b, const uint32_t (&value)[sizeof...(N)], F&& f)
{
    log_launch(LAUNCHER, b, value);
    pick_axes_of(axes, value, f);
}
// The axes of the keyed launchers (launch_axes) and the points of them that are kernels: the predicates below are what the launchers
// instantiate under (a static_assert or an `if constexpr`) and what variant_compiled answers with.
constexpr bool closest_mode_ok(uint32_t mode) { return mode < CLOSEST_MODES; }
constexpr bool any_mode_ok(uint32_t mode) { return mode == ANY_SHADOW || mode == ANY_HOOK; }
// the fused launch is the LDS-resident scenes' (pt_api.cpp: a BVH in global memory keeps the two launches apart), so it has no global-BVH kernels
constexpr bool fused_variant_ok(uint32_t bvh, uint32_t spill, uint32_t ident) { return bvh == 1u && spill < 2u && ident < 2u; }
// one thread per pixel is the pass of frames of PT_ACC_QUAD_BELOW pixels and more: no kernel where the quad pass takes every frame there can be
constexpr bool accumulate_variant_ok(uint32_t kind, uint32_t few, uint32_t mode)
{
    return kind < CAM_KINDS && mode < 3u && (few == 1u || (few == 0u && (uint64_t)PT_ACC_QUAD_BELOW < (1ull << 30)));
}
template <uint32_t LAUNCHER> struct launch_axes;
template <> struct launch_axes<LAUNCH_SHADE> : std::integer_sequence<uint32_t, Q_COUNT, MEDIA_COUNT, SHADOW_COUNT, PATHS_COUNT, FIRST_COUNT, SURF_COUNT> {};
template <> struct launch_axes<LAUNCH_TERMINAL> : std::integer_sequence<uint32_t, 2, 2> {};
template <> struct launch_axes<LAUNCH_CLOSEST> : std::integer_sequence<uint32_t, CLOSEST_MODES, 2, 2, 2> {};
template <> struct launch_axes<LAUNCH_ANY> : std::integer_sequence<uint32_t, ANY_MODES, 2, 2, 2> {};
template <> struct launch_axes<LAUNCH_FUSED> : std::integer_sequence<uint32_t, 2, 2, 2> {};
template <> struct launch_axes<LAUNCH_GENERATE> : std::integer_sequence<uint32_t, CAM_KINDS, 2> {};
template <> struct launch_axes<LAUNCH_GUIDE_RAYS> : std::integer_sequence<uint32_t, CAM_KINDS> {};
template <> struct launch_axes<LAUNCH_ACCUMULATE> : std::integer_sequence<uint32_t, CAM_KINDS, 2, 3> {};
template <uint32_t... N>
static uint32_t copy_bounds(std::integer_sequence<uint32_t, N...>, uint32_t bound[kLaunchAxes])
{
    const uint32_t b[] = {N...};
    for (size_t k = 0; k < sizeof...(N); ++k) bound[k] = b[k];
    return (uint32_t)sizeof...(N);
}
uint32_t variant_axes(uint32_t launcher, uint32_t bound[kLaunchAxes])
{
    for (uint32_t k = 0; k < kLaunchAxes; ++k) bound[k] = 0u;
    uint32_t n = 0;
    if (launcher < LAUNCH_COUNT) pick<LAUNCH_COUNT>(launcher, [&](auto l) { n = copy_bounds(launch_axes<l>{}, bound); });
    return n;
}
bool variant_compiled(uint32_t launcher, const uint32_t a[kLaunchAxes])
{
    uint32_t bound[kLaunchAxes];
    const uint32_t n = variant_axes(launcher, bound);
    if (n == 0u) return false;
    for (uint32_t k = 0; k < n; ++k)
        if (a[k] >= bound[k]) return false;
    switch (launcher)
    {
    case LAUNCH_SHADE: return shade_variant_ok(a[0], a[1], a[2], a[3], a[4], a[5]);
    case LAUNCH_CLOSEST: return closest_mode_ok(a[0]);
    case LAUNCH_ANY: return any_mode_ok(a[0]);
    case LAUNCH_FUSED: return fused_variant_ok(a[0], a[1], a[2]);
    case LAUNCH_ACCUMULATE: return accumulate_variant_ok(a[0], a[1], a[2]);
    default: return true; // every point inside the bounds
    }
}
uint32_t accumulate_max_pixels() { return accumulate_variant_ok(0u, 0u, 0u) ? ~0u : (uint32_t)PT_ACC_QUAD_BELOW - 1u; }

// How a camera kind reaches a kernel: camera_kind reads it off the optics, pick makes it a constant, camera_arg builds the one argument of
// that kind (CameraArg, pt_camera.h) and the kernel's primary_ray overload is chosen by the argument's type.
static uint32_t camera_kind(const CameraOptics& opt)
{
    if (proj_set(opt.proj)) return opt.proj.kind == PROJ_PANORAMA ? CAM_PANORAMA : CAM_ORTHOGRAPHIC;
    return lens_set(opt.lens) ? CAM_LENS : CAM_PINHOLE;
}
template <uint32_t KIND>
static CameraArg<KIND> camera_arg(const CameraView& cam, const CameraOptics& opt)
{
    CameraArg<KIND> c{};
    static_cast<CameraView&>(c) = cam;
    if constexpr (KIND == CAM_LENS) c.lens = opt.lens;
    else if constexpr (KIND != CAM_PINHOLE) c.proj = opt.proj;
    return c;
}

void launch_generate(hipStream_t s, const RenderParams& rp, const CameraView& cam, const CameraOptics& opt, const WavefrontBuffers& wb, const uint2* list)
{
    const uint32_t blocks = (rp.n_paths + 255u) / 256u;
    pick_logged<LAUNCH_GENERATE>(launch_axes<LAUNCH_GENERATE>{}, 0u, {camera_kind(opt), list ? 1u : 0u}, [&](auto kind, auto ls) {
        hipLaunchKernelGGL((k_generate<kind, ls != 0u>), dim3(blocks), dim3(256), 0, s, rp, camera_arg<kind>(cam, opt), wb.rq[0], wb.counters, list);
    });
}

// A persistent grid must be RESIDENT: workgroups that the device cannot hold at once start only when others have left, and by then
// the queue's dynamic part is gone and the late-comers' static chunks are the launch's tail.  So the grid is what the kernel's
// registers and LDS allow per CU (asked of the runtime once per kernel variant and LDS size; at most waves_cap waves per SIMD where the
// kernel's wave count is pinned: trace_waves_cap), times the CU count, capped by tl.grid_blocks (the spill area is sized for that).
#ifndef PT_RESIDENT_GRID
#define PT_RESIDENT_GRID 1
#endif
template <typename K>
static uint32_t resident_grid(K kernel, const TraceLaunch& tl, size_t lds, uint32_t waves_cap)
{
#if PT_RESIDENT_GRID
    struct Key { const void* f; uint32_t threads; size_t lds; int dev; int per_cu; };
    static std::mutex mu;
    static std::vector<Key> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    // a workgroup of block_threads threads is block_threads / 256 waves on each of the CU's four SIMDs
    const uint32_t cap = waves_cap ? std::max(1u, waves_cap * 256u / tl.block_threads) : ~0u;
    std::lock_guard<std::mutex> lk(mu);
    for (const Key& k : cache)
        if (k.f == (const void*)kernel && k.threads == tl.block_threads && k.lds == lds && k.dev == dev) return std::min<uint32_t>(tl.grid_blocks, tl.n_cus * std::min((uint32_t)k.per_cu, cap));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)tl.block_threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    cache.push_back(Key{(const void*)kernel, tl.block_threads, lds, dev, per_cu});
    return std::min<uint32_t>(tl.grid_blocks, tl.n_cus * std::min((uint32_t)per_cu, cap));
#else
    return tl.grid_blocks;
#endif
}

// the TLASes a launch from `root` walks: its own, and for CLOSEST_LIGHTS the world's as well (the any-hit phase)
static uint32_t tlas_bits(const TraceLaunch& tl, uint32_t root, bool with_world)
{
    const uint32_t own = root == tl.scene.world_root ? (uint32_t)IDENT_TLAS_WORLD : root == tl.scene.lights_root ? (uint32_t)IDENT_TLAS_LIGHTS : ~0u;
    return own | (with_world ? (uint32_t)IDENT_TLAS_WORLD : 0u);
}
// the IDENT kernels (one ray per lane, ident_ray) walk a launch whose every TLAS holds identity instances only
static bool ident_walk(const TraceLaunch& tl, uint32_t bits) { return (tl.ident_tlas & bits) == bits; }

// The traversal kernels' variant for a launch, picked once: f(BVH, SPILL, IDENT) with each as a std::integral_constant.  BVH 1: the
// scene's BVH is staged in LDS; SPILL: the stack's deepest levels live in global memory (Stack8<true>); IDENT: ident_walk.
// (LAUNCHER, mode, b: the launch log's row; mode is the kernel's MODE where it has one)
template <uint32_t LAUNCHER, typename F>
static void with_trace_variant(uint32_t mode, uint32_t b, const TraceLaunch& tl, bool ident, F&& f)
{
    const uint32_t bvh = tl.lds_scene ? 1u : 0u, spill = tl.scene.stack_entries > tl.scene.stack_lds ? 1u : 0u, id = ident ? 1u : 0u;
    if constexpr (LAUNCHER == LAUNCH_FUSED) log_launch(LAUNCHER, b, {bvh, spill, id});
    else log_launch(LAUNCHER, b, {mode, bvh, spill, id});
    pick_axes_of(launch_axes<LAUNCH_FUSED>{}, {bvh, spill, id}, f); // (BVH, spill, walk: the fused launcher's axes, and the last three of k_closest's and k_any's)
}
// a persistent traversal grid (resident_grid, per kernel) with the launch's dynamic LDS
template <typename K, typename... A>
static void launch_resident(K kernel, uint32_t waves_cap, const TraceLaunch& tl, hipStream_t s, const A&... args)
{
    const size_t lds = trace_lds_bytes(tl);
    hipLaunchKernelGGL(kernel, dim3(resident_grid(kernel, tl, lds, waves_cap)), dim3(tl.block_threads), lds, s, args...);
}

template <int MODE>
static void launch_closest_impl(hipStream_t s, const TraceLaunch& tl, uint32_t root, const RayQueue& rq, const uint32_t* n_ptr, uint32_t cap_in,
                                uint32_t* heads, const ClosestOut& out, uint32_t b = 0u)
{
    static_assert(closest_mode_ok(MODE), "no such mode of k_closest");
    const ClosestKArgs ka{tl.scene, (const uint4*)tl.blob, rq.a, rq.b, n_ptr, heads, root, cap_in, out};
    with_trace_variant<LAUNCH_CLOSEST>(MODE, b, tl, ident_walk(tl, tlas_bits(tl, root, MODE == CLOSEST_LIGHTS)), [&](auto bvh, auto spill, auto ident) {
        launch_resident(k_closest<bvh, MODE, spill, ident>, trace_waves_cap(bvh != 0, ident), tl, s, ka);
    });
}
template <int MODE>
static void launch_any_impl(hipStream_t s, const TraceLaunch& tl, uint32_t root, const RayQueue& rq, const uint32_t* n_ptr, uint32_t cap_in,
                            uint32_t* heads, uint32_t* occluded, f4* radiance = nullptr, uint32_t b = 0u)
{
    static_assert(any_mode_ok(MODE), "no such mode of k_any");
    const uint4* blob = (const uint4*)tl.blob;
    with_trace_variant<LAUNCH_ANY>(MODE, b, tl, ident_walk(tl, tlas_bits(tl, root, false)), [&](auto bvh, auto spill, auto ident) {
        launch_resident(k_any<bvh, MODE, spill, ident>, trace_waves_cap(bvh != 0, ident), tl, s, tl.scene, blob, root, rq.a, rq.b, n_ptr, cap_in, heads, occluded, radiance);
    });
}

static uint32_t* row_heads(const WavefrontBuffers& wb, uint32_t row, uint32_t which)
{
    return wb.heads + ((size_t)row * HEADS_PER_ROW + which) * kHeadWordsPerQueue;
}

// what the world closest-hit launch of bounce b writes (shade queues, terminal queue, counters row b); for b >= 1 (CLOSEST_WORLD) also
// the paths it finishes
static ClosestOut world_out(const WavefrontBuffers& wb, uint32_t b, const RenderParams& rp, const EnvView& env)
{
    Counters* row = wb.counters + b;
    ClosestOut out{};
    out.hits = wb.hits;
    out.q_base = wb.q_shade_base;
    out.q_stride = wb.q_stride;
    out.q_class_slot = wb.q_class_slot;
    out.q_term = wb.q_term[b & 1u];
    out.n_shade = row->n_shade;
    out.tails = wb.tails + (size_t)b * Q_COUNT * kTailWordsPerQueue;
    out.cap_shade = wb.cap_slots_shade;
    out.cap_term = wb.cap_slots_term;
    out.class_mask = wb.class_mask | (1u << Q_TERMINAL);
    out.overflow = &row->overflow;
    out.finalize_miss = env.w == 0u ? 1u : 0u;
    if (b != 0u)
    {
        out.rec = wb.st.rec;
        out.radiance = wb.st.radiance;
        out.enable_nee = rp.enable_nee;
    }
    return out;
}

void launch_trace_world(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b, const RenderParams& rp, const CameraView& cam,
                        const CameraOptics& opt, const EnvView& env, bool ray_list)
{
    Counters* row = wb.counters + b;
    ClosestOut out = world_out(wb, b, rp, env);
    out.wave_times = wb.wave_times ? wb.wave_times + (size_t)b * kWaveTimeSlots : nullptr;
    if (b == 0u)
    {
        out.eye = f3{cam.eye[0], cam.eye[1], cam.eye[2]};
        out.radiance = wb.st.radiance;
        out.occl = wb.st.occl;
        out.first_pos = wb.st.first_pos;
        out.first_id = wb.st.first_id;
        out.keep_s_id = rp.keep_s_id; out.keep_s_pos = rp.keep_s_pos;
        out.blk_log = rp.blk_log; out.n_blk = rp.n_blk; out.blk_last = rp.blk_last; out.act_pixels = rp.act_pixels;
        out.div_blk_paths = rp.div_blk_paths; out.div_blk_last = rp.div_blk_last;
        if (lens_set(opt.lens) || proj_set(opt.proj) || ray_list) launch_closest_impl<CLOSEST_PRIMARY_LENS>(s, tl, tl.scene.world_root, wb.rq[0], &row->n_closest, wb.cap_slots, row_heads(wb, b, HEADS_CLOSEST), out, b);
        else launch_closest_impl<CLOSEST_PRIMARY>(s, tl, tl.scene.world_root, wb.rq[0], &row->n_closest, wb.cap_slots, row_heads(wb, b, HEADS_CLOSEST), out, b);
    }
    else if (tl.emission_tex) launch_closest_impl<CLOSEST_WORLD_EMTEX>(s, tl, tl.scene.world_root, wb.rq[b & 1u], &row->n_closest, wb.cap_slots, row_heads(wb, b, HEADS_CLOSEST), out, b);
    else launch_closest_impl<CLOSEST_WORLD>(s, tl, tl.scene.world_root, wb.rq[b & 1u], &row->n_closest, wb.cap_slots, row_heads(wb, b, HEADS_CLOSEST), out, b);
}
// world closest hit of bounce b (b >= 1) + the BSDF-sampled NEE rays of bounce b - 1 in one launch (k_trace_fused)
void launch_trace_fused(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b, const RenderParams& rp, const EnvView& env)
{
    Counters* row = wb.counters + b;
    Counters* prev = wb.counters + (b - 1u);
    const ClosestOut wout = world_out(wb, b, rp, env);
    ClosestOut lout{};
    lout.hits = wb.lchain_hit;
    lout.world_root = tl.scene.world_root;
    lout.occl = wb.st.occl;
    FusedArgs fa{};
    fa.wa = wb.rq[b & 1u].a; fa.wb = wb.rq[b & 1u].b; fa.wn = &row->n_closest; fa.wheads = row_heads(wb, b, HEADS_CLOSEST);
    fa.la = wb.rq_lchain[(b - 1u) & 1u].a; fa.lb = wb.rq_lchain[(b - 1u) & 1u].b; fa.ln = &prev->n_lchain; fa.lheads = row_heads(wb, b - 1u, HEADS_LCHAIN);
    fa.world_root = tl.scene.world_root; fa.lights_root = tl.scene.lights_root; fa.cap_in = wb.cap_slots;
    const FusedKArgs ka{tl.scene, (const uint4*)tl.blob, fa, wout, lout};
    bool launched = false;
    with_trace_variant<LAUNCH_FUSED>(0u, b, tl, ident_walk(tl, IDENT_TLAS_WORLD | IDENT_TLAS_LIGHTS), [&](auto bvh, auto spill, auto ident) {
        if constexpr (fused_variant_ok(bvh, spill, ident))
        {
            launched = true;
            launch_resident(k_trace_fused<bvh, spill, ident>, trace_waves_cap(bvh != 0, ident), tl, s, ka);
        }
    });
    if (!launched) // a missing kernel is an error, never a skipped pass
    {
        fprintf(stderr, "launch_trace_fused: no fused traversal for a BVH in global memory\n");
        abort();
    }
}
void launch_trace_shadow(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b)
{
    Counters* row = wb.counters + b;
#if PT_WAVE_TIMES
    {
        uint4* where = wb.wave_times_any ? wb.wave_times_any + (size_t)b * kWaveTimeSlots : nullptr;
        (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_any_times), &where, sizeof(where), 0, hipMemcpyHostToDevice, s);
    }
#endif
    launch_any_impl<ANY_SHADOW>(s, tl, tl.scene.world_root, wb.rq_shadow, &row->n_shadow, wb.cap_slots, row_heads(wb, b, HEADS_SHADOW),
                                reinterpret_cast<uint32_t*>(wb.st.rec), wb.st.radiance, b);
}
void launch_trace_lchain(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b)
{
    Counters* row = wb.counters + b;
    ClosestOut out{};
    out.hits = wb.lchain_hit;
    out.n_shade = nullptr;
    out.world_root = tl.scene.world_root;
    out.occl = wb.st.occl;
    launch_closest_impl<CLOSEST_LIGHTS>(s, tl, tl.scene.lights_root, wb.rq_lchain[b & 1u], &row->n_lchain, wb.cap_slots, row_heads(wb, b, HEADS_LCHAIN), out, b);
}
// (A textured scene queues its shadow rays: the inline walk would need INLINE x TEX variants of the pass whose registers are the tightest.)
// The Lambertian shading pass walks its own shadow rays when the scene's BVH and a workgroup's stacks take no more LDS than five workgroups per CU can share
// (the pass keeps its five waves per SIMD), nothing spills from the stacks, the scene has no media (those kernels are short of registers as it is) and the
// traversal workgroups have the shading pass's shape (the stack layout is per thread of a workgroup).
bool shade_traces_shadow(const TraceLaunch& tl)
{
    return PT_INLINE_SHADOW != 0 && !tl.tex && tl.lds_scene && tl.scene.stack_entries <= tl.scene.stack_lds && !tl.scene.has_volumes && tl.block_threads == PT_SHADE_THREADS &&
           trace_lds_bytes(tl) + 1024 <= 32 * 1024;
}
void launch_shade(hipStream_t s, uint32_t qclass, const SceneView& sv, const RenderParams& rp, const WavefrontBuffers& wb, uint32_t b,
                  uint32_t grid_blocks, const CameraView& cam, const CameraOptics& opt, const EnvView& env, const TraceLaunch* tl, const uint2* list,
                  const uint2* ray_keys)
{
    const TexView* const tex = tl ? tl->tex : nullptr;
    if (ray_keys) list = nullptr; // (a ray batch has no pixels)
    const bool proj0 = b == 0u && proj_set(opt.proj) && ray_keys == nullptr;   // projection (pt_set_projection): origins of their own, ONE draw consumed
    const bool lens0 = proj0 || (b == 0u && (lens_set(opt.lens) || ray_keys != nullptr)); // only bounce 0 knows of the camera: its rays' origins and the draws they consumed
    ShadeIO io{};
    io.env = env;
    io.primary_a = f4{cam.eye[0], cam.eye[1], cam.eye[2], __builtin_inff()};
    io.st = wb.st;
    io.rq_in = wb.rq[b & 1u];
    io.rq_out = wb.rq[(b + 1u) & 1u];
    io.rq_shadow = wb.rq_shadow;
    io.rq_lchain = wb.rq_lchain[b & 1u];
    io.rq_lchain_prev = wb.rq_lchain[(b + 1u) & 1u];
    io.lchain_nb = wb.lchain_nb[b & 1u];
    io.lchain_nb_prev = wb.lchain_nb[(b + 1u) & 1u];
    io.lchain_hit = wb.lchain_hit;
    io.hits = wb.hits;
    io.entries = wb.q_term[b & 1u];
    if (qclass != Q_TERMINAL)
    {
        io.q_in = shade_queue(wb, qclass);
        io.tails_in = wb.tails + ((size_t)b * Q_COUNT + qclass) * kTailWordsPerQueue;
    }
    io.q_term_next = wb.q_term[(b + 1u) & 1u];
    io.cap_slots = wb.cap_slots;
    io.cap_slots_term = wb.cap_slots_term;
    io.cap_slots_shade = wb.cap_slots_shade;
    io.ctr = wb.counters + b;
    io.lchain_heads = row_heads(wb, b, HEADS_LCHAIN);
    io.shadow_heads = row_heads(wb, b, HEADS_SHADOW);
    io.ctr_next = wb.counters + b + 1u;
    const uint32_t surface_blocks = (grid_blocks * 256u + PT_SHADE_THREADS - 1u) / PT_SHADE_THREADS; // grid_blocks is in units of 256 threads
    const bool inl = tl && shade_traces_shadow(*tl);
    if (list && qclass != Q_TERMINAL) io.list = list; // (the surface passes read no terminal entries)
    if (ray_keys && qclass != Q_TERMINAL) io.list = ray_keys;
    const ShadeKArgs ka{sv, rp, io, b, inl ? (const uint4*)tl->blob : nullptr, inl ? tl->scene.world_root : 0u};
    const TexNView texn = tex ? TexNView{*tex, tl->tri_tan} : TexNView{};
    if (qclass == Q_TERMINAL)
    {
        // (TexView: the terminal pass of a scene with an emission texture looks a light hit's colour up)
        pick_logged<LAUNCH_TERMINAL>(launch_axes<LAUNCH_TERMINAL>{}, b, {lens0 ? 1u : 0u, tex && tl->emission_tex ? 1u : 0u}, [&](auto lens, auto emtex) {
            if constexpr (emtex != 0u) hipLaunchKernelGGL((k_shade_terminal<lens != 0u, TexView>), dim3(grid_blocks), dim3(256), 0, s, sv, rp, io, b, *tex);
            else hipLaunchKernelGGL((k_shade_terminal<lens != 0u>), dim3(grid_blocks), dim3(256), 0, s, sv, rp, io, b);
        });
        return;
    }
    // the six axes of the surface pass (k_shade_surface), each decided here and nowhere else
    const uint32_t media = sv.has_volumes ? MEDIA_VOLUMES : MEDIA_NONE;
    const uint32_t shadow = !(inl && qclass == Q_LAMBERT) ? SHADOW_QUEUED : (PT_IDENT_SHADE && ident_walk(*tl, IDENT_TLAS_WORLD)) ? SHADOW_INLINE_IDENT : SHADOW_INLINE;
    const uint32_t paths = ray_keys ? PATHS_RAYS : list ? PATHS_LIST : PATHS_RECT;
    const uint32_t first = proj0 ? FIRST_OWN_ONE_DRAW : lens0 ? FIRST_OWN_TWO_DRAWS : FIRST_SHARED;
    const uint32_t surface = !tex ? SURF_PLAIN : tl->tri_tan ? (tl->emission_tex ? SURF_TEX_EMTEX_NMAP : SURF_TEX_NMAP) : (tl->emission_tex ? SURF_TEX_EMTEX : SURF_TEX);
    const size_t lds = inl ? trace_lds_bytes(*tl) : 0; // (an untextured scene whose Lambertian pass walks its shadow rays: every class's launch carries the walk's LDS)
    bool launched = false;
    pick_logged<LAUNCH_SHADE>(launch_axes<LAUNCH_SHADE>{}, b, {qclass, media, shadow, paths, first, surface},
        [&](auto q, auto md, auto sh, auto pa, auto fi, auto su) {
            if constexpr (shade_variant_ok(q, md, sh, pa, fi, su)) // (the other points are no kernels: nothing is instantiated for them)
            {
                launched = true;
                ShadeArg<su> arg{};
                static_cast<ShadeKArgs&>(arg) = ka;
                if constexpr (su != SURF_PLAIN) arg.tex = texn; // (ShadeKArgsTex keeps the texture view, ShadeKArgsNmap the tangents behind it too)
                hipLaunchKernelGGL((k_shade_surface<q, md, sh, pa, fi, su>), dim3(surface_blocks), dim3(PT_SHADE_THREADS), lds, s, arg);
            }
        });
    if (!launched) // a missing kernel is an error, never a skipped pass
    {
        fprintf(stderr, "launch_shade: no surface pass for class %u, media %u, shadow %u, paths %u, first %u, surface %u\n", qclass, media, shadow, paths, first, surface);
        abort();
    }
}

void launch_accumulate(hipStream_t s, const RenderParams& rp, const CameraView& cam, const CameraOptics& opt, const WavefrontBuffers& wb, f4* accum, f4* position,
                       uint32_t* id, uint32_t write_position, uint32_t add_to_accum, float* moments, const uint2* list)
{
    const uint32_t n = list ? rp.act_pixels : rp.local_pixels;
    if (n == 0u) return;
    const bool quad = n < (uint32_t)PT_ACC_QUAD_BELOW;
    const dim3 grid(quad ? (n * 4u + 255u) / 256u : (n + 255u) / 256u);
    // (a list comes with moments: pt_render_adaptive)
    bool launched = false;
    pick_logged<LAUNCH_ACCUMULATE>(launch_axes<LAUNCH_ACCUMULATE>{}, 0u, {camera_kind(opt), quad ? 1u : 0u, list ? 2u : moments ? 1u : 0u}, [&](auto kind, auto few, auto mode) {
        if constexpr (accumulate_variant_ok(kind, few, mode))
        {
            launched = true;
            hipLaunchKernelGGL((k_accumulate<CameraArg<kind>, few != 0u, mode >= 1u, mode == 2u>), grid, dim3(256), 0, s, rp, camera_arg<kind>(cam, opt), wb.st, accum, position, id,
                               write_position, add_to_accum, moments, list);
        }
    });
    if (!launched) // (pt_set_config admits no frame of more than accumulate_max_pixels local pixels)
    {
        fprintf(stderr, "launch_accumulate: no kernel for %u pixels\n", n);
        abort();
    }
}
uint32_t adaptive_select_blocks(uint32_t n_pixels) { return (n_pixels + kSelectPerBlock - 1u) / kSelectPerBlock; }
void launch_adaptive_select(hipStream_t s, const f4* accum, const float* moments, uint32_t n_pixels, const AdaptiveCrit& cr, uint32_t* counts, uint2* list,
                            uint32_t* header)
{
    const uint32_t blocks = adaptive_select_blocks(n_pixels);
    if (blocks == 0u) return;
    hipLaunchKernelGGL(k_adaptive_count, dim3(blocks), dim3(256), 0, s, accum, moments, n_pixels, cr, counts, header);
    hipLaunchKernelGGL(k_adaptive_write, dim3(blocks), dim3(256), 0, s, accum, moments, n_pixels, cr, (const uint32_t*)counts, list, header);
}
void launch_generate_rays(hipStream_t s, const RenderParams& rp, const RayView& rays, const WavefrontBuffers& wb)
{
    hipLaunchKernelGGL(k_generate_rays, dim3((rp.n_paths + 255u) / 256u), dim3(256), 0, s, rp.n_paths, rays.o, rays.d, wb.rq[0], wb.counters);
}
void launch_pack_ray_keys(hipStream_t s, uint64_t n, const uint32_t* key, const uint32_t* sample, uint2* out)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_pack_ray_keys, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, n, key, sample, out);
}
void launch_store_rays(hipStream_t s, const RenderParams& rp, const RayView& rays, const WavefrontBuffers& wb, f4* radiance, f4* position, uint8_t* id)
{
    if (rp.n_paths == 0u) return;
    hipLaunchKernelGGL(k_store_rays, dim3((rp.n_paths + 255u) / 256u), dim3(256), 0, s, rp.n_paths, rays.o, rays.d, wb.st, radiance, position, id);
}
void launch_probe_rays(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, float* o, float* d, uint2* key)
{
    if (count == 0u) return;
    hipLaunchKernelGGL(k_probe_rays, dim3((count + 255u) / 256u), dim3(256), 0, s, pb, first, count, o, d, key);
}
void launch_probe_project(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* radiance, float* sh27)
{
    if (count == 0u) return;
    const uint64_t probes = (first + count - 1u) / pb.n_samples - first / pb.n_samples + 1u;
    hipLaunchKernelGGL(k_probe_project, dim3((uint32_t)((probes * 27u + 255u) / 256u)), dim3(256), 0, s, pb, first, count, d, radiance, sh27);
}
void launch_store_samples(hipStream_t s, const RenderParams& rp, const WavefrontBuffers& wb, f4* out)
{
    const uint32_t blocks = (uint32_t)(((uint64_t)rp.local_pixels * rp.batch_samples + 255u) / 256u);
    hipLaunchKernelGGL(k_store_samples, dim3(blocks), dim3(256), 0, s, rp, wb.st, out);
}

void launch_trace_rays_closest(hipStream_t s, const TraceLaunch& tl, uint32_t root, RayQueue rq, uint32_t n, uint32_t* n_and_heads, f4* hits)
{
    ClosestOut out{};
    out.hits = hits;
    launch_closest_impl<CLOSEST_HOOK>(s, tl, root, rq, n_and_heads, n, n_and_heads + 32, out);
}
void launch_trace_rays_any(hipStream_t s, const TraceLaunch& tl, uint32_t root, RayQueue rq, uint32_t n, uint32_t* n_and_heads, uint32_t* occluded)
{
    launch_any_impl<ANY_HOOK>(s, tl, root, rq, n_and_heads, n, n_and_heads + 32, occluded);
}
void launch_sobol_probe(hipStream_t s, uint32_t n_points, uint32_t n, const uint32_t* index, const uint32_t* seed, float* out_xy)
{
    hipLaunchKernelGGL(k_sobol_probe, dim3((n + 255u) / 256u), dim3(256), 0, s, n_points, n, index, seed, out_xy);
}
void launch_math_probe(hipStream_t s, int fn, uint32_t n, const float* a, const float* b, float* o0, float* o1, uint64_t seed)
{
    hipLaunchKernelGGL(k_math_probe, dim3((n + 255u) / 256u), dim3(256), 0, s, fn, n, a, b, o0, o1, seed);
}
void launch_material_probe(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* normal,
                           const uint8_t* front, const uint32_t* pixel, const uint32_t* sample, uint32_t draws, uint64_t seed, float* out9)
{
    hipLaunchKernelGGL(k_material_probe, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, material, n, incoming, normal, front, pixel, sample, draws, seed,
                       out9);
}

void launch_volume_probe(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* t_max, const float* dist,
                         const uint32_t* pixel, const uint32_t* sample, uint32_t draws, uint64_t seed, float* out9)
{
    hipLaunchKernelGGL(k_volume_probe, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, material, n, incoming, t_max, dist, pixel, sample, draws, seed, out9);
}
void launch_bsdf_probe(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* outgoing,
                       const float* normal, const uint8_t* front, float* out4)
{
    hipLaunchKernelGGL(k_bsdf_probe, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, material, n, incoming, outgoing, normal, front, out4);
}

void launch_guide_rays(hipStream_t s, const RenderParams& rp, const CameraView& cam, const CameraOptics& opt, RayQueue rq, uint32_t* n_and_heads)
{
    pick_logged<LAUNCH_GUIDE_RAYS>(launch_axes<LAUNCH_GUIDE_RAYS>{}, 0u, {camera_kind(opt)}, [&](auto kind) {
        hipLaunchKernelGGL(k_guide_rays<kind>, dim3((rp.local_pixels + 255u) / 256u), dim3(256), 0, s, rp, camera_arg<kind>(cam, opt), rq, n_and_heads);
    });
}
// a hop's launch: none without slots, one thread per slot, the FIRST instantiation at hop 0 (it never reads `state`)
template <class Kernel, class... Args>
void launch_chain_hop(hipStream_t s, const ChainHop& a, Kernel first, Kernel later, const Args&... args)
{
    if (a.cap == 0u) return;
    hipLaunchKernelGGL(a.hop == 0u ? first : later, dim3((a.cap + 255u) / 256u), dim3(256), 0, s, args...);
}
void launch_guide_follow(hipStream_t s, const SceneView& sv, const TexView& tex, const FollowArgs& a)
{
    if (a.sum) launch_chain_hop(s, a, k_guide_follow<true, true>, k_guide_follow<true, false>, sv, tex, a);
    else launch_chain_hop(s, a, k_guide_follow<false, true>, k_guide_follow<false, false>, sv, tex, a);
}
// the baked view's ending by its axes: key says what lights a final surface (BakedKey), light holds the views that go with it
typedef std::integer_sequence<uint32_t, 2, 2, 2, 2> baked_axes; // grid, vis, spec, dir
void launch_baked_follow(hipStream_t s, const SceneView& sv, const TexNView& tex, const BakedLight& light, const BakedKey& key, const BakedArgs& a)
{
    bool launched = false;
    pick_axes_of(baked_axes{}, {key.grid, key.vis, key.spec, key.dir}, [&](auto grid, auto vis, auto spec, auto dir) {
        if constexpr (baked_variant_ok(grid, vis, spec, dir)) // (depth and radiance are a grid's: the other six points are no kernels)
        {
            launched = true;
            launch_chain_hop(s, a, k_baked_follow<true, grid != 0u, vis != 0u, spec != 0u, dir != 0u>, k_baked_follow<false, grid != 0u, vis != 0u, spec != 0u, dir != 0u>, sv,
                             tex, light, a);
        }
    });
    if (!launched) // a missing kernel is an error, never a skipped pass
    {
        fprintf(stderr, "launch_baked_follow: no ending for grid %u, vis %u, spec %u, dir %u\n", key.grid, key.vis, key.spec, key.dir);
        abort();
    }
}
// ... and the same ten points with the rays' ending
void launch_baked_rays(hipStream_t s, const SceneView& sv, const TexNView& tex, const BakedLight& light, const BakedKey& key, const BakedRayArgs& a)
{
    bool launched = false;
    pick_axes_of(baked_axes{}, {key.grid, key.vis, key.spec, key.dir}, [&](auto grid, auto vis, auto spec, auto dir) {
        if constexpr (baked_variant_ok(grid, vis, spec, dir))
        {
            launched = true;
            launch_chain_hop(s, a, k_baked_rays<true, grid != 0u, vis != 0u, spec != 0u, dir != 0u>, k_baked_rays<false, grid != 0u, vis != 0u, spec != 0u, dir != 0u>, sv, tex,
                             light, a);
        }
    });
    if (!launched)
    {
        fprintf(stderr, "launch_baked_rays: no ending for grid %u, vis %u, spec %u, dir %u\n", key.grid, key.vis, key.spec, key.dir);
        abort();
    }
}
void launch_probe_grid_lookup(hipStream_t s, const ProbeGridView& grid, const ProbeDepthView* depth, uint32_t n, const float* position, const float* normal, float* rgb,
                              uint8_t* lit)
{
    if (n == 0u) return;
    if (depth) hipLaunchKernelGGL(k_probe_grid_lookup<true>, dim3((n + 255u) / 256u), dim3(256), 0, s, grid, *depth, n, position, normal, rgb, lit);
    else hipLaunchKernelGGL(k_probe_grid_lookup<false>, dim3((n + 255u) / 256u), dim3(256), 0, s, grid, ProbeDepthView{}, n, position, normal, rgb, lit);
}
void launch_rays_to_queue(hipStream_t s, uint32_t n, const float* o, const float* d, RayQueue rq, uint32_t* n_and_heads)
{
    if (n == 0u) return;
    // (k_generate_rays writes the count into word 0 of what it is handed: a batch's first counter row there, a hook queue's count word here)
    static_assert(__builtin_offsetof(Counters, n_closest) == 0, "a hook queue's count word is read as Counters::n_closest");
    hipLaunchKernelGGL(k_generate_rays, dim3((n + 255u) / 256u), dim3(256), 0, s, n, o, d, rq, (Counters*)n_and_heads);
}
void launch_probe_backfaces(hipStream_t s, const SceneView& sv, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* hits,
                            uint32_t* hits_out, uint32_t* back_out)
{
    if (count == 0u) return;
    const uint64_t probes = (first + count - 1u) / pb.n_samples - first / pb.n_samples + 1u;
    hipLaunchKernelGGL(k_probe_backfaces, dim3((uint32_t)((probes * 64u + 255u) / 256u)), dim3(256), 0, s, sv, pb, first, count, d, hits, hits_out, back_out);
}
void launch_probe_depth_fold(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* hits, uint32_t res,
                             float max_distance, DProbeDepth* sums, uint32_t* counts)
{
    if (count == 0u) return;
    const uint64_t probes = (first + count - 1u) / pb.n_samples - first / pb.n_samples + 1u;
    hipLaunchKernelGGL(k_probe_depth_fold, dim3((uint32_t)((probes * 64u + 255u) / 256u)), dim3(256), 0, s, pb, first, count, d, hits, res, max_distance, sums,
                       counts);
}
void launch_lightmap_lookup_directional(hipStream_t s, const SceneView& sv, const TexNView& tex, const LmView& lm, const LmDirView& ld, uint32_t n,
                                        const uint32_t* instance, const uint32_t* tri, const float* u, const float* v, const float* dir, float* rgb, uint8_t* mapped)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_lightmap_lookup_directional, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, tex, lm, ld, n, instance, tri, u, v, dir, rgb, mapped);
}
void launch_probe_radiance_fold(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* radiance, uint32_t res,
                                float* sums, uint32_t* counts)
{
    if (count == 0u) return;
    const uint64_t probes = (first + count - 1u) / pb.n_samples - first / pb.n_samples + 1u;
    hipLaunchKernelGGL(k_probe_radiance_fold, dim3((uint32_t)((probes * 64u + 255u) / 256u)), dim3(256), 0, s, pb, first, count, d, radiance, res, sums, counts);
}
void launch_probe_radiance_prefilter(hipStream_t s, uint32_t res, uint32_t n_probes, uint32_t n_levels, const float* alpha, const float* sums,
                                     const uint32_t* counts, f4* table)
{
    if (n_probes == 0u) return;
    PrefilterArgs a{res, n_levels, {}};
    for (uint32_t l = 0; l < n_levels && l < 8u; ++l) a.alpha[l] = alpha[l];
    hipLaunchKernelGGL(k_probe_radiance_prefilter, dim3(n_probes * n_levels), dim3((res * res + 63u) / 64u * 64u), res * res * 2u * sizeof(f4), s, a, sums, counts, table);
}
void launch_probe_grid_specular(hipStream_t s, const ProbeGridView& grid, const ProbeRadianceView& rad, const ProbeDepthView* depth, uint32_t n,
                                const float* position, const float* normal, const float* incoming, const float* alpha, float* rgb, uint8_t* lit)
{
    if (n == 0u) return;
    if (depth) hipLaunchKernelGGL(k_probe_grid_specular<true>, dim3((n + 255u) / 256u), dim3(256), 0, s, grid, rad, *depth, n, position, normal, incoming, alpha, rgb, lit);
    else
        hipLaunchKernelGGL(k_probe_grid_specular<false>, dim3((n + 255u) / 256u), dim3(256), 0, s, grid, rad, ProbeDepthView{}, n, position, normal, incoming, alpha,
                           rgb, lit);
}
void launch_lightmap_lookup(hipStream_t s, const LmView& lm, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u, const float* v,
                            float* rgb, uint8_t* mapped)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_lightmap_lookup, dim3((n + 255u) / 256u), dim3(256), 0, s, lm, n, instance, tri, u, v, rgb, mapped);
}
void launch_guide_follow_dir(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* normal, const uint8_t* front,
                             float* out4)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_guide_follow_dir, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, material, n, incoming, normal, front, out4);
}
void launch_surface_colour(hipStream_t s, const SceneView& sv, const TexView& tex, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u,
                           const float* v, float* rgb)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_surface_colour, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, tex, n, instance, tri, u, v, rgb);
}
void launch_surface_roughness(hipStream_t s, const SceneView& sv, const TexView& tex, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u,
                              const float* v, float* alpha)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_surface_roughness, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, tex, n, instance, tri, u, v, alpha);
}
void launch_shading_normal(hipStream_t s, const SceneView& sv, const TexNView& tex, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u,
                           const float* v, const float* dir, float* out4)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_shading_normal, dim3((n + 255u) / 256u), dim3(256), 0, s, sv, tex, n, instance, tri, u, v, dir, out4);
}

} // namespace pt
