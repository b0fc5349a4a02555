// How a render request is cut into batches of samples and spread over the wavefront pipelines (pt_api.cpp: run_batches), and how
// many paths of wavefront state the device memory holds.  Plain arithmetic on a few integers, free of HIP so that the host sanitizer
// driver (host_sanitize.cpp plan) can test it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifndef PT_SPLIT_MIN_PATHS
#define PT_SPLIT_MIN_PATHS (24u << 20) // BVHs in global memory: a request that fits is cut in two for two pipelines from this many paths on (see plan_batches)
#endif
#ifndef PT_SPLIT_MIN_PATHS_LDS
#define PT_SPLIT_MIN_PATHS_LDS (24u << 20)
#endif
#ifndef PT_PIPES4_MIN_PATHS
#define PT_PIPES4_MIN_PATHS (~0ull) // four pipelines by default: never (see plan_batches); pt_config.pipelines = 4 asks for them
#endif

namespace pt {

constexpr uint32_t kMaxPipelines = 4;

// Paths of wavefront state that fit beside everything else: 85 % of the free device memory plus what the pipelines' pools already hold.
// Bytes per path (ensure_wavefront): 323 in records, ray queues and terminal queues + 54 per surface class present in the scene (its
// 48-byte shade queue with an eighth of slack) + 8 with volumes.  (Rounds 1-3 assumed 410 whatever the scene: right for one class,
// but the four-class atrium then asked for 268 GiB of a 268.2 GiB device.)  Path ids are 29-bit.
inline size_t max_paths_for(size_t free_bytes, size_t held_bytes, uint32_t n_classes, bool volumes)
{
    const double per_path = 330.0 + 56.0 * std::max(n_classes, 1u) + (volumes ? 8.0 : 0.0) + 24.0;
    const size_t max_paths = (size_t)((double)(free_bytes + held_bytes) * 0.85 / per_path);
    return std::min<size_t>(std::max<size_t>(max_paths, 1u << 20), (1ull << 29) - 1);
}

struct PlanRequest
{
    uint32_t n_samples = 0;              // > 0
    size_t act_pixels = 1;               // pixels whose camera rays are generated (>= 1)
    bool samples_out = false;            // the samples are returned (pt_render_samples): one pipeline, a read-back after each batch
    uint32_t pipelines = 0, batch_spp = 0; // pt_config
    bool lds_scene = false;              // the BVH is resident in LDS
    size_t max_paths = 0;                // max_paths_for, or its fallback
    size_t cap_paths[kMaxPipelines] = {}; // paths the pipelines' pools hold now
};
struct BatchPlan
{
    uint32_t batch = 0, n_batches = 0, n_pipes = 0; // batch == 0: refused, a batch would need path ids beyond 29 bits
};

// By default the whole request stays resident when HBM allows; otherwise (or with pt_config.batch_spp) it is cut into equal batches that
// alternate between `pipelines` wavefront pipelines on their own HIP streams, so that one batch's launch tails overlap the other's launches.
inline BatchPlan plan_batches(const PlanRequest& q)
{
    const uint32_t n_samples = q.n_samples;
    const size_t act_pixels = q.act_pixels, max_paths = q.max_paths;
    uint32_t want_pipes = q.samples_out ? 1u : std::min<uint32_t>(q.pipelines ? q.pipelines : 2u, kMaxPipelines);
    uint32_t batch = q.batch_spp ? q.batch_spp : (uint32_t)std::max<size_t>(1, max_paths / act_pixels);
    batch = std::min(batch, n_samples);
    uint32_t n_batches = (n_samples + batch - 1) / batch;
    // (A request that fits at once runs as ONE batch on one pipeline.  Cutting a small one — a rank's share of a sharded frame — in two
    // for two pipelines used to hide its launch tails (-8 %); since the tails were shortened at the source (striped tails, tapered
    // chunks) it costs 5 % instead: twice the launches, and two persistent kernels fighting for the same wave slots.)
    // ... with one exception: BVHs in global memory.  Their rays are long, the launches end in long tails, and smaller batches on several
    // pipelines overlap them (same box, 82 k-triangle mesh at 1080p unless noted):
    //   32 spp   one batch 43.9 ms   2 x 16 on two pipelines 40.8   4 x 8 on four 44.9
    //   128 spp                      2 x 64: 149.1                  4 x 32: 149.3
    //   512 spp  one batch 629.5     2 x 256: 580 (4 x 128 on TWO pipelines: 583-588)   3 x 171 on three: 572   4 x 128 on four: 561
    //   328 k mesh, 1024 spp         2 x 512: 1903                  3 x 342: 1889       4 x 256: 1846
    //   8 spp (4 M paths) 14.21 -> 14.26: nothing; three spheres, 8 spp (7.8 M paths): 10.46 -> 9.95 (four pipelines: 11.3)
    // so (rounds 2-3, FOUR waves per SIMD): two pipelines from 6 M paths on.  Round 4, FIVE waves per SIMD — the kernels hide more of their own latency, a second
    // persistent grid has less to fill — same box, one pipeline against the split: 82 k mesh 64 spp 67.2 -> 64.9 ms, 512 spp 497 -> 475; 328 k mesh 64 spp 115.1 -> 113.5,
    // 1024 spp (bench.py) 1663 -> 1637; atrium 256 spp 1127-1141 -> 1112-1114, but 64 spp 280.7 -> 288.2 and 8 spp 38.7 -> 39.5; spheres +-0: the split went off ...
    // ... and came back once the surface shading kernels ran at five waves too (one pipeline's shading beside the other's traversal), same box, one batch against
    // two halves: atrium 16 / 64 spp 74.1 -> 71.8 / 281.6 -> 272.7 ms, 82 k mesh 16 / 64 spp 20.4 -> 20.3 / 64.7 -> 62.7, 328 k mesh 64 spp 113.5 -> 108.6, three spheres
    // 16 / 64 spp 15.1 -> 15.2 / 49.4 -> 47.7: from PT_SPLIT_MIN_PATHS = 24 M paths on, as for LDS scenes.  (Requests that do not fit always alternated between two
    // pipelines.)  Four (from PT_PIPES4_MIN_PATHS on) did not hold up under bench.py: 82 k mesh at 512 spp
    // 573 -> 588 ms, 328 k mesh at 1024 spp 1979 -> 1959 ms, three spheres at 4096^2 x 1024 spp 12.15 -> 12.43 s; off.
    const uint64_t total_paths = (uint64_t)n_samples * act_pixels;
    if (!q.samples_out && !q.pipelines && !q.lds_scene && total_paths >= (uint64_t)PT_PIPES4_MIN_PATHS) want_pipes = kMaxPipelines;
    // (Round 4: with five waves per SIMD in the traversal AND the surface shading kernels one pipeline's shading pass runs beside the other's traversal, and the split pays
    // from a quarter of the headline frame on: whole frame 62.4 -> 59.0 ms, rank 0's half 32.4 -> 30.5, its quarter 17.1 -> 16.4, its eighth (16.6 M paths) 9.44 -> 9.38:
    // from PT_SPLIT_MIN_PATHS_LDS = 24 M paths on.)  Round 3:
    // LDS-resident BVHs gain only on very large requests (with round 3's launch structure): the 133 M-path headline frame 68.3 -> 67.2 ms
    // (bench.py, three interleaved repeats), mixed materials at 66 M paths 42.9 -> 42.3 ms, but rank 0's half of the sharded frame (66 M
    // paths) 35.0 -> 35.7 ms and its quarter +-0: from PT_SPLIT_MIN_PATHS_LDS paths on.
    if (!q.batch_spp && n_batches < want_pipes && want_pipes >= 2 && total_paths >= (q.lds_scene ? (uint64_t)PT_SPLIT_MIN_PATHS_LDS : (uint64_t)PT_SPLIT_MIN_PATHS))
    {
        n_batches = std::min<uint32_t>(want_pipes, n_samples);
        batch = (n_samples + n_batches - 1) / n_batches;
    }
    const uint32_t n_pipes = std::min(want_pipes, n_batches);
    if (!q.batch_spp && n_batches > 1 && (uint64_t)batch * act_pixels * n_pipes > max_paths)
    {
        // the request does not fit at once: the pipelines share the memory
        batch = (uint32_t)std::max<size_t>(1, max_paths / n_pipes / act_pixels);
        n_batches = (n_samples + batch - 1) / batch;
    }
    if (!q.batch_spp && n_batches > 1)
    {
        // pools that an earlier request left (a 64-spp warm-up before a 4096-spp render, say) are kept when they are nearly large enough:
        // rounding n_samples / n_batches up differently must not cost a reallocation of hundreds of GB (seconds) inside a render
        size_t cap_min = ~(size_t)0;
        for (uint32_t i = 0; i < n_pipes; ++i) cap_min = std::min(cap_min, q.cap_paths[i]);
        const size_t want = (size_t)batch * act_pixels;
        if (cap_min >= act_pixels && cap_min < want && cap_min * 4 >= want * 3)
        {
            batch = (uint32_t)(cap_min / act_pixels);
            n_batches = (n_samples + batch - 1) / batch;
        }
    }
    batch = (n_samples + n_batches - 1) / n_batches;
    if ((uint64_t)batch * act_pixels >= (1ull << 29)) return BatchPlan{};
    return BatchPlan{batch, n_batches, n_pipes};
}

} // namespace pt
