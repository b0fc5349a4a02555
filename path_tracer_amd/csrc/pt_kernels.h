// Launch interface of the gfx950 kernels (pt_kernels.hip).  No launcher allocates, frees or synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "pt_materials.h"
#include "pt_temporal.h"
#include "pt_types.h"

namespace pt {

struct TraceLaunch
{
    SceneView scene;
    const void* blob;        // contiguous nodes | tri_isect | instances (device), copied to LDS when lds_scene
    bool lds_scene;
    uint32_t ident_tlas;     // IDENT_TLAS_*: TLASes the IDENT kernels may walk (one ray per lane)
    uint32_t grid_blocks;    // upper bound of the persistent grid (the launchers shrink it to what is resident at once)
    uint32_t n_cus;
    uint32_t block_threads;  // 64..256
    const TexView* tex;      // the built scene has a textured material: its texture view (the surface passes are the TEX variants), else null
    bool emission_tex;       // ... and some EMISSIVE material is among them (pt_set_material_emission_texture): a light hit's colour is looked up, so the
                             // terminal pass is its TEX variant and the world closest-hit launches leave light hits to it (CLOSEST_WORLD_EMTEX)
    const f4* tri_tan;       // ... and some material has a normal map (pt_set_material_normal_texture): the per-triangle tangents (the surface passes are
                             // the normal-map variants), else null
};

// dynamic LDS of a traversal workgroup: the staged BVH blob (LDS scenes) + the per-lane (node, t_enter) stacks
inline size_t trace_lds_bytes(bool lds_scene, uint32_t blob_bytes, uint32_t stack_lds, uint32_t block_threads)
{
    return (lds_scene ? (size_t)blob_bytes : 0) + (size_t)stack_lds * block_threads * 8;
}
inline size_t trace_lds_bytes(const TraceLaunch& tl) { return trace_lds_bytes(tl.lds_scene, tl.scene.blob_bytes, tl.scene.stack_lds, tl.block_threads); }

struct WavefrontBuffers
{
    PathState st;
    RayQueue rq[2];       // world closest-hit rays, double buffered by bounce parity
    RayQueue rq_shadow;   // explicit-light shadow rays
    RayQueue rq_lchain[2]; // BSDF-sampled NEE rays, double buffered by bounce parity (the next shading pass re-reads directions)
    f4* lchain_nb[2];     // per BSDF-sampled ray, same slots and parity: bsdf rgb of the sampled direction | weakening
    f4* lchain_hit;       // per BSDF-sampled ray: its lights-TLAS closest hit t,u,v | id, written only when the light is visible
    f4* hits;             // world closest hits of rays whose path goes to the terminal queue, by ray index (and the unit hooks' output)
    // surface classes: self-contained hit records in queue order (ShadeQueue).  One allocation for all classes present in the scene:
    // class q's arrays a, b, c start at q_shade_base + (3 * slot(q) + {0,1,2}) * q_stride, slot(q) = nibble q of q_class_slot
    // (one base pointer instead of fifteen: the traversal kernels are short of scalar registers)
    f4* q_shade_base;
    uint32_t q_stride;     // slots per array (capacity + dump area)
    uint32_t q_class_slot;
    uint2* q_term[2];     // terminal queue {ray index | path id + ENTRY_DEAD, path id}, double buffered by bounce parity
    Counters* counters;   // [max_bounces + 2]
    uint32_t* heads;      // [max_bounces + 2][HEADS_PER_ROW][kHeadWordsPerQueue] claim cursors of the ray queues
    uint4* wave_times;    // PT_WAVE_TIMES builds only: [max_bounces + 2][kWaveTimeSlots] (k_closest launches), else nullptr
    uint4* wave_times_any; // ... the same for the shadow-ray launches
    uint32_t* tails;      // [max_bounces + 2][Q_COUNT][kTailWordsPerQueue] striped tails of the shade queues (pt_types.h)
    uint32_t cap_slots;   // capacity of every ray queue (each allocated with kQueueDumpSlots more)
    uint32_t cap_slots_shade; // capacity of the surface shade queues (= cap_slots except in the overflow test)
    uint32_t cap_slots_term;
    uint32_t class_mask;  // bit q: the scene has instances of shade class q
};

// the word of a ShadeQueue::a record (direction.xyz | path id) that holds the path id: what reads the ids back from the host goes by it
enum : uint32_t { kShadePidWord = 3u };
static_assert(sizeof(f4) == 4 * sizeof(uint32_t) && kShadePidWord == offsetof(f4, w) / sizeof(uint32_t), "ShadeQueue::a keeps the path id in .w of a 16-byte record");
inline ShadeQueue shade_queue(const WavefrontBuffers& wb, uint32_t q)
{
    const size_t slot = (wb.q_class_slot >> (4u * q)) & 0xfu;
    f4* a = wb.q_shade_base + 3u * slot * (size_t)wb.q_stride;
    return ShadeQueue{a, a + wb.q_stride, a + 2u * (size_t)wb.q_stride};
}

// One batch of a caller's ray list (pt_integrate_rays): the window's rays, every pointer already offset to the window's first ray.  Path id =
// index inside the window, one path per ray (RenderParams: act_pixels = n_paths = the window's length, batch_samples = 1, so pid_split is the
// identity and PathState::first_pos / first_id hold one record per path; RenderParams::ray_draws = the draws every path starts with).
//   o, d : 3 floats per ray (the caller's layout); d is used as given
//   key  : {pixel, sample} of the ray's stream (stream_key): what the pixel grid or an adaptive list supplies for a camera path
struct RayView
{
    const float* o;
    const float* d;
    const uint2* key;
};
// out[i] <- {key[i], sample[i]}: RayView::key of a whole list from the caller's two arrays (device pointers)
void launch_pack_ray_keys(hipStream_t s, uint64_t n, const uint32_t* key, const uint32_t* sample, uint2* out);
// rq[0] <- the window's rays (t_max +inf, ray index = path id), counters[0].n_closest <- their number
void launch_generate_rays(hipStream_t s, const RenderParams& rp, const RayView& rays, const WavefrontBuffers& wb);
// the finisher of a ray batch in launch_accumulate's place: per path the finalised sample (rgb, 1), the first hit r.at(t) | t and its id byte
// (a miss: r.at(1e5) | 1e5 and 255) to entry [path id] of the three outputs, each of which may be null
void launch_store_rays(hipStream_t s, const RenderParams& rp, const RayView& rays, const WavefrontBuffers& wb, f4* radiance, f4* position, uint8_t* id);
// irradiance probes (pt_bake_probes; the definition is include/pt_api.h's and pt_probe.h's).  Ray r of a bake is sample first_sample + r % n_samples
// of probe r / n_samples.  launch_probe_rays fills rays [first, first + count) of the bake into a ray table at the same indices;
// launch_probe_project folds the radiance of those rays (d, radiance: the same window, as integrated) into sh27 in sample order, one thread per
// (probe, coefficient, channel)
struct ProbeBake
{
    const float* position; // 3 floats per probe
    uint32_t n_probes, first_sample, n_samples, key_base, n_sobol;
    uint64_t seed;
};
void launch_probe_rays(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, float* o, float* d, uint2* key);
void launch_probe_project(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* radiance, float* sh27);

// lightmaps (pt_bake_lightmap; the definition is include/pt_api.h's and pt_lightmap.h's; the kernels are pt_lightmap.hip's).  One placement of one
// model, uploaded per call: its load-order UVs (6 floats per triangle), positions and normals (9 each) and the instance's forward matrix.
struct LightmapView
{
    const float* uv;
    const float* positions;
    const float* normals;
    uint32_t n_tris, w, h;
    xf34 m;
};
// a coverage work item {triangle, first} walks texels [first, first + kLightmapSlice) of the triangle's texel rectangle (lm_box), so a triangle
// with a huge rectangle is many items
constexpr uint32_t kLightmapSlice = 2048u;
// owner[k] <- the lowest triangle index whose UVs contain the centre of texel k, MISS_ID where none does (w * h words)
void launch_lightmap_cover(hipStream_t s, const LightmapView& lm, const uint2* items, uint32_t n_items, uint32_t* owner);
// per texel: (u, v) of its owner, the surface point and the normal (3 floats each), the coverage byte (1 / 0); an uncovered texel gets zeros
void launch_lightmap_resolve(hipStream_t s, const LightmapView& lm, const uint32_t* owner, float* uv2, float* position, float* normal, uint8_t* coverage);
// Ray r of a bake is sample first_sample + r % n_samples of covered texel texels[r / n_samples] (texel indices, ascending); position and normal
// are launch_lightmap_resolve's, sum the map's w * h * 3 sums.  launch_lightmap_rays fills rays [first, first + count) of the bake into a ray
// table at indices [0, count); launch_lightmap_fold adds the radiance of those rays (the same window, as integrated) to sum in sample order, one
// thread per (covered texel, channel)
struct LightmapBake
{
    const uint32_t* texels;
    const float* position;
    const float* normal;
    uint32_t n_covered, first_sample, n_samples, key_base, n_sobol;
    float bias;
    uint64_t seed;
};
void launch_lightmap_rays(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, float* o, float* d, uint2* key);
// sumsq (pt_bake_lightmap_moments; null: pt_bake_lightmap's launch as it was): the map's w * h second moments, Q[texel] += l(L) * l(L) in the same order
void launch_lightmap_fold(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const f4* radiance, float* sum, float* sumsq = nullptr);
// pt_bake_lightmap_directional: the same window folded by twelve threads per covered texel, the three sums as above and the nine first moments
// dir[texel][axis][channel] += L[channel] * d[axis] (d: the window's ray table, launch_lightmap_rays' directions) in the same order
void launch_lightmap_fold_directional(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const f4* radiance, const float* d, float* sum, float* dir);
// Adaptive bakes (pt_bake_lightmap_adaptive): the items are the entries {texel, its sample count} of launch_lightmap_select's list instead of
// every covered texel, and ray r is sample list[r / n_samples].y + r % n_samples of texel list[r / n_samples].x; otherwise LightmapBake, and
// the same rays and fold kernels, instantiated over this record.
struct LightmapAdaptiveBake
{
    const uint2* list;
    const float* position;
    const float* normal;
    uint32_t n_active, n_samples, key_base, n_sobol;
    float bias;
    uint64_t seed;
};
void launch_lightmap_rays(hipStream_t s, const LightmapAdaptiveBake& lb, uint64_t first, uint32_t count, float* o, float* d, uint2* key);
void launch_lightmap_fold(hipStream_t s, const LightmapAdaptiveBake& lb, uint64_t first, uint32_t count, const f4* radiance, float* sum, float* sumsq);
// Direct light sampled at the texel (pt_bake_lightmap_direct, pt_bake_lightmap_adaptive_direct; lm_light_sample, pt_lightmap.h).
// launch_lightmap_light_samples writes the light samples of rays [first, first + count) of a bake into entries [0, count) of a ray queue, as
// shadow rays (o | t_max, dir | entry; a hole where none is cast), and of a ce table, and the count into n_and_heads[0]: the queue is
// launch_trace_rays_any's.  launch_lightmap_fold_direct is launch_lightmap_fold over X = G + D of the same window.
struct LmLightView;
struct LightmapDirectWindow
{
    const f4* radiance;       // the gather rays' radiance, as launch_lightmap_fold takes it
    const uint8_t* id;        // ... and their first-hit id bytes (launch_store_rays)
    const uint8_t* emissive;  // 256 bytes: non-zero where the id byte means an emissive model
    const f4* ce;             // the light samples
    const uint32_t* occluded; // ... and their shadow rays' results (holes unwritten)
};
void launch_lightmap_light_samples(hipStream_t s, const LightmapBake& lb, const LmLightView& lv, uint32_t light_key_base, uint64_t first, uint32_t count, RayQueue q,
                                   f4* ce, uint32_t* n_and_heads);
void launch_lightmap_light_samples(hipStream_t s, const LightmapAdaptiveBake& lb, const LmLightView& lv, uint32_t light_key_base, uint64_t first, uint32_t count,
                                   RayQueue q, f4* ce, uint32_t* n_and_heads);
void launch_lightmap_fold_direct(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const LightmapDirectWindow& w, float* sum, float* sumsq);
void launch_lightmap_fold_direct(hipStream_t s, const LightmapAdaptiveBake& lb, uint64_t first, uint32_t count, const LightmapDirectWindow& w, float* sum, float* sumsq);
// unit hook (pt_lightmap_light_sample): lm_light_sample of n caller-given (key, sample, origin, normal); dir_t = dir | t_max, ce = ce | 1.0f where a ray is cast
void launch_lightmap_light_sample_hook(hipStream_t s, const LmLightView& lv, uint64_t seed, uint32_t n, const uint32_t* key, const uint32_t* sample,
                                       const float* origin, const float* normal, uint32_t* light, f4* dir_t, f4* ce);
// The texel selection: texel k is ACTIVE iff coverage[k] (launch_lightmap_resolve's byte) and adaptive_active (pt_types.h) of (sum[k],
// sumsq[k], counts[k]).  Two passes over the table, no atomic append: list <- {k, counts[k]} of the active texels in ascending k (room for
// n_texels entries), header[0] <- their number, header[1] |= 1 when an ACTIVE OR INACTIVE covered texel has counts[k] + n_samples > 2^24.
// header: 4 zeroed words; block_counts: lightmap_select_blocks(n_texels) words of scratch.  Uncovered texels are read for their byte only.
struct LightmapSelect
{
    const uint8_t* coverage;
    const float *sum, *sumsq;
    const uint32_t* counts;
    uint32_t n_texels, n_samples;
    AdaptiveCrit cr;
};
uint32_t lightmap_select_blocks(uint32_t n_texels);
void launch_lightmap_select(hipStream_t s, const LightmapSelect& sel, uint32_t* block_counts, uint2* list, uint32_t* header);
// counts[list[i].x] += n_samples for i < n_active: once per call, after its last window was folded
void launch_lightmap_advance(hipStream_t s, const uint2* list, uint32_t n_active, uint32_t n_samples, uint32_t* counts);
// pt_lightmap_gradient: grad <- lm_gradient (pt_lightmap.h) of every texel of launch_lightmap_resolve's table (coverage, normal), zeros where uncovered
void launch_lightmap_gradient(hipStream_t s, uint32_t n_texels, const uint8_t* coverage, const float* normal, uint32_t n_samples, const float* dir, float* grad);
// one dilation pass (lm_dilate) of a w x h map from (rgb, cov) to (rgb_out, cov_out)
void launch_lightmap_dilate(hipStream_t s, uint32_t w, uint32_t h, const float* rgb, const uint8_t* cov, float* rgb_out, uint8_t* cov_out);
// the texel filter (pt_lightmap_denoise: pt_filter.h's a-trous core under pt_lightmap_filter.h's texel rule) of the map of lm: prim, position, normal are
// launch_lightmap_resolve's table, sum (w * h * 3) and sumsq (w * h; read with `moments` only, else the spatial variance) the bake's; cv_a, cv_b,
// pa, nv: scratch of w * h 16-byte entries each; rgb <- the means (w * h * 3, zeros where uncovered); area (may be null) <- the texel areas;
// counts (pt_lightmap_denoise_counts; null: every texel has n_samples): the sample count of each texel, w * h words, n_samples then unread
struct LmFilterK;
struct LmFilterImages
{
    const uint32_t* prim;
    const float *position, *normal, *sum, *sumsq;
    const uint32_t* counts;
    f4 *cv_a, *cv_b, *pa, *nv;
    float* rgb;
    float* area;
};
void launch_lightmap_denoise(hipStream_t s, const LightmapView& lm, const LmFilterK& p, uint32_t n_samples, bool moments, const LmFilterImages& im);

// ---- the keyed launchers' variants, for tests (pt_variant_axes, pt_variant_compiled, pt_last_launches; include/pt_api.h has the axes' values).
// A keyed launcher turns integers into template arguments (pick_axes, pt_kernels.hip); the axes' bounds and the predicate that says which of
// their points are kernels are the ones the launcher itself instantiates from.
enum Launcher : uint32_t
{
    LAUNCH_SHADE,      // k_shade_surface: qclass, media, shadow, paths, first, surface
    LAUNCH_TERMINAL,   // k_shade_terminal: lens, emission texture
    LAUNCH_CLOSEST,    // k_closest: MODE, bvh, spill, ident
    LAUNCH_ANY,        // k_any: MODE, bvh, spill, ident
    LAUNCH_FUSED,      // k_trace_fused: bvh, spill, ident
    LAUNCH_GENERATE,   // k_generate: camera kind, list
    LAUNCH_GUIDE_RAYS, // k_guide_rays: camera kind
    LAUNCH_ACCUMULATE, // k_accumulate: camera kind, few, mode (0 sums, 1 sums and moments, 2 those of a list)
    LAUNCH_COUNT
};
constexpr uint32_t kLaunchAxes = 6;
// bound[k] <- the number of values of the launcher's k-th axis; the number of axes (0: no such launcher)
uint32_t variant_axes(uint32_t launcher, uint32_t bound[kLaunchAxes]);
// true: the point (its first variant_axes values) is a kernel of the code object
bool variant_compiled(uint32_t launcher, const uint32_t axis[kLaunchAxes]);
// One row per keyed launch, written where the launcher has decided the axes: the launcher, the counter row (bounce) it works on (0 where
// it has none) and the axis values it dispatched on, unused ones 0.
struct LaunchRow
{
    uint32_t launcher, b, axis[kLaunchAxes];
};
typedef std::vector<LaunchRow> LaunchLog;
// while one lives, the keyed launches of its thread are appended to `log` (null: to none); scopes nest
struct LaunchLogScope
{
    explicit LaunchLogScope(LaunchLog* log);
    ~LaunchLogScope();
    LaunchLogScope(const LaunchLogScope&) = delete;
    LaunchLogScope& operator=(const LaunchLogScope&) = delete;
    LaunchLog* prev;
};
// the most local pixels launch_accumulate has a kernel for
uint32_t accumulate_max_pixels();

// list: an adaptive list (launch_adaptive_select's {local pixel, n_p} entries, rp.act_pixels of them) whose pixels the batch's paths belong
// to instead of the active rectangle's (pt_render_adaptive), or null
// opt.lens: with a radius above 0 (lens_set) the launchers that take one run the thin-lens variants of their kernels (pt_set_lens); the pinhole
// kernels are the ones they always were
inline bool lens_set(const LensView& lens) { return lens.radius > 0.0f; }
// opt.proj: with a kind other than PROJ_PERSPECTIVE (proj_set) they run the projection variants (pt_set_projection), whose camera rays carry origins
// of their own like a lens's but consume one draw
inline bool proj_set(const ProjView& proj) { return proj.kind != PROJ_PERSPECTIVE; }
void launch_generate(hipStream_t s, const RenderParams& rp, const CameraView& cam, const CameraOptics& opt, const WavefrontBuffers& wb, const uint2* list = nullptr);
// closest hit against the world TLAS for bounce `b`: reads rq[b&1], writes hits + shade queues of row b
// (ray_list: bounce 0 of a ray batch, whose rays have origins of their own like a lens's)
void launch_trace_world(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b, const RenderParams& rp, const CameraView& cam,
                        const CameraOptics& opt, const EnvView& env, bool ray_list = false);
// the same for bounce b >= 1 together with the BSDF-sampled NEE launch of bounce b - 1, as ONE launch (a wave goes from queue to queue)
void launch_trace_fused(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b, const RenderParams& rp, const EnvView& env);
// NEE rays produced by the shading of bounce `b` (counter row b)
void launch_trace_shadow(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b);
// BSDF-sampled NEE rays: closest hit against the lights TLAS, then (same kernel, same lane) any-hit against the world
void launch_trace_lchain(hipStream_t s, const TraceLaunch& tl, const WavefrontBuffers& wb, uint32_t b);
// shading of bounce b for one queue class
// (ray_keys: RayView::key of a ray batch, whose paths take their stream from it and start at RenderParams::ray_draws draws)
// (tl: the scene's traversal launch description; with it the Lambert / GGX passes of an LDS-resident scene may trace their own shadow rays,
//  and the passes of a textured scene (tl->tex) look the surface colour up)
void launch_shade(hipStream_t s, uint32_t qclass, const SceneView& sv, const RenderParams& rp, const WavefrontBuffers& wb, uint32_t b,
                  uint32_t grid_blocks, const CameraView& cam, const CameraOptics& opt, const EnvView& env, const TraceLaunch* tl = nullptr,
                  const uint2* list = nullptr, const uint2* ray_keys = nullptr);
// true: the shading pass answers the explicit-light shadow rays itself and nothing is queued for launch_trace_shadow
bool shade_traces_shadow(const TraceLaunch& tl);
// accum[pixel] += sum over batch samples in order of (finalised rgb, 1); position/id of the last samples.  With moments also
// moments[pixel] += L * L of each finalised sample beside it (PT_FLAG_ADAPTIVE); with a list (which needs moments) only the listed
// pixels, in list order
void launch_accumulate(hipStream_t s, const RenderParams& rp, const CameraView& cam, const CameraOptics& opt, const WavefrontBuffers& wb, f4* accum, f4* position,
                       uint32_t* id, uint32_t write_position, uint32_t add_to_accum, float* moments = nullptr, const uint2* list = nullptr);
void launch_store_samples(hipStream_t s, const RenderParams& rp, const WavefrontBuffers& wb, f4* out);
// adaptive selection of n_pixels local pixels: list <- {pixel, n_p} of every active pixel in ascending order, header[0] <- their number,
// header[1] |= 1 if some count is not an integer in [0, 2^24] (the caller zeroes header[1]); counts: adaptive_select_blocks words
uint32_t adaptive_select_blocks(uint32_t n_pixels);
void launch_adaptive_select(hipStream_t s, const f4* accum, const float* moments, uint32_t n_pixels, const AdaptiveCrit& cr, uint32_t* counts, uint2* list,
                            uint32_t* header);

// after the path (pt_post.hip)
void launch_post_accumulate(hipStream_t s, uint32_t n, const f4* input, f4* accum);
void launch_post_velocity(hipStream_t s, int w, int h, const f4* position, const float* m16, float* velocity_xy);
// pt_frame_moving's motion table, one row per world-TLAS instance: rows of its inverse matrix now and of its forward matrix in the previous
// frame's build; moved = 0 where it has no previous matrix or that matrix is bit-equal to the current one (the point is then passed on)
struct MotionRow
{
    float inv[12], prv[12];
    uint32_t moved, pad[3];
};
static_assert(sizeof(MotionRow) == 112, "");
void launch_post_motion(hipStream_t s, uint32_t n, const f4* position, const uint32_t* instance, uint32_t n_instances, const MotionRow* rows, f4* x_prev);
void launch_post_reproject(hipStream_t s, int w, int h, const f4* input, const f4* accum, const float* velocity_xy, const uint32_t* id, f4* output);
void launch_post_tonemap(hipStream_t s, uint32_t n, const f4* accum, f4* out);
void launch_post_rgb8(hipStream_t s, uint32_t n, const f4* accum, uint8_t* out);
void launch_post_deinterleave(hipStream_t s, uint32_t w, uint32_t h, uint32_t world, uint32_t strip, uint32_t pad_rows, const f4* parts, f4* full);

// edge-aware a-trous denoiser (pt_denoise, pt_post_denoise; the definition is include/pt_api.h's, the per-pixel arithmetic and the
// parameters DenoiseK pt_filter.h's).
// the filter's images (w x h).  Guides: position xyz | t, normal xyz | -, model (MISS_ID = miss); moments null = spatial variance.  albedo null:
// pt_denoise / pt_post_denoise.  Else pt_denoise_albedo / pt_post_denoise_albedo: the same filter on the accumulation divided by the albedo
// (xyz per pixel; albedo_is_sum: the mean-albedo sums, xyz / w), the last level multiplying it back
struct DenoiseImages
{
    const f4* accum;
    const float* moments;
    const f4* position;
    const f4* normal;
    const uint32_t* model;
    const f4* albedo;
    bool albedo_is_sum;
    f4 *cv_a, *cv_b; // scratch: colour | variance
    f4* nv;          // scratch: normal | valid
    f4* kd;          // scratch, with an albedo only: the per-pixel divisor
    f4* out;         // the result (c, 1) or (0, 0, 0, 0)
};
void launch_denoise(hipStream_t s, int w, int h, const DenoiseK& p, const DenoiseImages& im);
// the temporal stage (pt_frame_temporal, pt_post_temporal; the per-pixel steps are pt_temporal.h's).  n_prev <- the normal guide carried back
// like launch_post_motion carries the position; hist_out, mom_out <- steps 1-4 of every pixel of im under the options rescue and mean_length;
// albedo (null: no demodulation): cur is divided by the divisor made of it, which goes to kd
void launch_temporal_motion_normal(hipStream_t s, uint32_t n, const f4* normal, const uint32_t* instance, uint32_t n_instances, const MotionRow* rows, f4* n_prev);
void launch_temporal_reproject(hipStream_t s, const TemporalImages& im, const TemporalK& k, bool rescue, bool mean_length, const f4* albedo, f4* kd, f4* hist_out,
                               f2* mom_out);
// step 5: var <- the variance of every pixel of (cn, mom); cv, nv (either may be null) <- the filter's (C | var) and (normal | 1) images
void launch_temporal_variance(hipStream_t s, int w, int h, const DenoiseK& p, float alpha, const f4* cn, const f2* mom, const f4* position, const f4* normal,
                              const uint32_t* model, f4* cv, f4* nv, float* var);
// steps 6 and 7: launch_denoise's level loop on cv_a (every pixel valid) to out, and after level 0 the store: xq, gq <- the current guides, with
// feedback hist.rgb <- level 0's output; kmul (null: none): the result, and only the result, is multiplied by it
void launch_temporal_filter(hipStream_t s, int w, int h, const DenoiseK& p, bool feedback, const f4* position, const f4* normal, const uint32_t* model, f4* cv_a,
                            f4* cv_b, f4* nv, const f4* kmul, f4* out, f4* hist, f4* xq, f4* gq);
// the camera rays of sample rp.first_sample of every local pixel into a hook queue (ray index = local pixel), n_and_heads[0] <- local pixels
void launch_guide_rays(hipStream_t s, const RenderParams& rp, const CameraView& cam, const CameraOptics& opt, RayQueue rq, uint32_t* n_and_heads);
// unit hook (pt_surface_colour): rgb[i] <- surface colour of world instance[i], leaf-order triangle tri[i] at barycentrics u[i], v[i]
void launch_surface_colour(hipStream_t s, const SceneView& sv, const TexView& tex, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u,
                           const float* v, float* rgb);
// unit hook (pt_surface_roughness): alpha[i] <- surface_roughness_at (pt_materials.h) of the same queries; tex is all null in a scene without textures
// (no material then asks for it)
void launch_surface_roughness(hipStream_t s, const SceneView& sv, const TexView& tex, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u,
                              const float* v, float* alpha);
// unit hook (pt_shading_normal): out4[i] <- shading_normal (pt_materials.h) of world instance[i], leaf-order triangle tri[i] at barycentrics u[i], v[i]
// for the world direction dir[i] | front.  tex.tri_tan is null in a scene without a normal map (no material then asks for it)
void launch_shading_normal(hipStream_t s, const SceneView& sv, const TexNView& tex, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u,
                           const float* v, const float* dir, float* out4);

// unit hooks
// One hop of the guide chains, what every ending is handed (pt_api.cpp, walk_chains).  `in`: the hook queue launch_trace_rays_closest just traced
// into hits (n_in: its count word); chains that go on are appended to `next` (n_next: its count word, zero before the launch; both queues hold cap
// slots; both null at the last hop, where no chain goes on).  Hop `hop` of at most max_hops; the kernels of every ending are shells over one
// chain_hop (pt_kernels.hip) that reads all of this
struct ChainHop
{
    RayQueue in, next;
    const f4* hits;
    const uint32_t* n_in;
    uint32_t* n_next;
    f4* state;             // per pixel: running colour product | t of a chain that goes on, summed by the guides (may be null at max_hops 0)
    uint32_t cap, hop, max_hops;
};
// pt_render_guides[_followed] / pt_accumulate_albedo[_followed]: the guides' ending (first-hit guides: max_hops 0).  sum null: a chain
// that ends writes the six guides of its pixel; else it adds its albedo product to sum[pixel]
struct FollowArgs : ChainHop
{
    f4 *position, *normal, *albedo;
    uint32_t *model, *instance;
    uint8_t* hops;
    f4* sum;
};
void launch_guide_follow(hipStream_t s, const SceneView& sv, const TexView& tex, const FollowArgs& a);
// pt_render_baked: the same chains with the baked view's ending (include/pt_api.h states it): a chain that ends adds its baked sample and 1 to
// sum[pixel]; state[].w is not read.  env.w == 0: the constant ambient
struct BakedArgs : ChainHop
{
    f4* sum;
    EnvView env;
    float unlit[3];
};
// What lights a final surface of the baked view, every variant's one argument: the lightmap tables, their gradients (null without one), the
// probe grid, its depth moments and its prefiltered radiance (zeroed where not set).  A variant reads the views of its axes and no other.
struct BakedLight
{
    LmView lm;
    LmDirView ld;
    ProbeGridView grid;
    ProbeDepthView depth;
    ProbeRadianceView rad;
};
// ... and the ending's four axes, 0 or 1 each: a probe grid set (it lights a final surface that no map lights); depth set on it (its lookups
// are the ones with visibility); radiance set on it (GGX metal reflects it); a gradient in use and a normal-mapped material in the scene (maps
// and grid are read under the perturbed normal).  vis and spec are the grid's: a key with either and no grid names no kernel and aborts
struct BakedKey
{
    uint32_t grid, vis, spec, dir;
};
void launch_baked_follow(hipStream_t s, const SceneView& sv, const TexNView& tex, const BakedLight& light, const BakedKey& key, const BakedArgs& a);
// pt_baked_rays and the gather bakes: the same chains over a window of caller rays (the queue's "pixel" word is the ray's index in the window,
// state holds an entry per ray of it).  A chain that ends stores out[ray] = B | its hop; hop 0 writes id[ray], the first hit's id byte as
// pt_integrate_rays reports it, for every ray of the window.  Either output may be null.  The ending's axes and views are the baked view's.
struct BakedRayArgs : ChainHop
{
    f4* out;
    uint8_t* id;
    EnvView env;
    float unlit[3];
};
void launch_baked_rays(hipStream_t s, const SceneView& sv, const TexNView& tex, const BakedLight& light, const BakedKey& key, const BakedRayArgs& a);
// unit hook (pt_probe_grid_lookup): probe_grid_lookup (pt_probe.h) at n positions and normals (3 floats each), with visibility where depth is
// not null
void launch_probe_grid_lookup(hipStream_t s, const ProbeGridView& grid, const ProbeDepthView* depth, uint32_t n, const float* position, const float* normal, float* rgb,
                              uint8_t* lit);
// pt_probe_backfaces: a ray table's entries [0, n) (o, d: 3 floats per ray) as a hook queue (t_max +inf, ray index = entry), its count word set;
// then the closest hits of rays [first, first + count) of the bake `pb` (d, hits: the window) counted per probe into hits_out and back_out,
// which continue from what they hold: one wave per probe, no atomics
void launch_rays_to_queue(hipStream_t s, uint32_t n, const float* o, const float* d, RayQueue rq, uint32_t* n_and_heads);
void launch_probe_backfaces(hipStream_t s, const SceneView& sv, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* hits,
                            uint32_t* hits_out, uint32_t* back_out);
// pt_bake_probe_depth: the same window's hits folded into the probes' R x R octahedral depth maps (sums: the two moments' sums per texel,
// counts: the rays per texel; both continue from what they hold), in sample order per texel: one wave per probe, no atomics
void launch_probe_depth_fold(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* hits, uint32_t res,
                             float max_distance, DProbeDepth* sums, uint32_t* counts);
// reflection probes.  pt_bake_probe_radiance: the same window's integrated radiance folded into the probes' R x R octahedral radiance maps
// (sums: r, g, b per texel, counts: the rays per texel; both continue from what they hold), in sample order per texel: one wave per probe,
// no atomics.  pt_probe_radiance_prefilter: table[probe][level][texel] = the GGX prefilter of the means, one workgroup per (probe, level).
// pt_probe_grid_specular's unit hook: probe_grid_specular (pt_probe.h) of n queries, with visibility where depth is not null
void launch_probe_radiance_fold(hipStream_t s, const ProbeBake& pb, uint64_t first, uint32_t count, const float* d, const f4* radiance, uint32_t res,
                                float* sums, uint32_t* counts);
void launch_probe_radiance_prefilter(hipStream_t s, uint32_t res, uint32_t n_probes, uint32_t n_levels, const float* alpha, const float* sums,
                                     const uint32_t* counts, f4* table);
void launch_probe_grid_specular(hipStream_t s, const ProbeGridView& grid, const ProbeRadianceView& rad, const ProbeDepthView* depth, uint32_t n,
                                const float* position, const float* normal, const float* incoming, const float* alpha, float* rgb, uint8_t* lit);
// unit hook (pt_lightmap_lookup): lightmap_at (pt_materials.h) of world instance[i], leaf-order triangle tri[i] at barycentrics u[i], v[i]
void launch_lightmap_lookup(hipStream_t s, const LmView& lm, uint32_t n, const uint32_t* instance, const uint32_t* tri, const float* u, const float* v,
                            float* rgb, uint8_t* mapped);
// unit hook (pt_lightmap_lookup_directional): lightmap_at_directional of n hits with ray directions dir (3 floats each)
void launch_lightmap_lookup_directional(hipStream_t s, const SceneView& sv, const TexNView& tex, const LmView& lm, const LmDirView& ld, uint32_t n,
                                        const uint32_t* instance, const uint32_t* tri, const float* u, const float* v, const float* dir, float* rgb, uint8_t* mapped);
// pt_guide_follow_dir(on_device = 1): guide_follow_dir (pt_materials.h) of n hits of `material`, out4 = wo | followed
void launch_guide_follow_dir(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* normal, const uint8_t* front,
                             float* out4);
// n_and_heads: word 0 = number of rays, words [32, 32 + kHeadWordsPerQueue) = zeroed claim cursors
void launch_trace_rays_closest(hipStream_t s, const TraceLaunch& tl, uint32_t root, RayQueue rq, uint32_t n, uint32_t* n_and_heads, f4* hits);
void launch_trace_rays_any(hipStream_t s, const TraceLaunch& tl, uint32_t root, RayQueue rq, uint32_t n, uint32_t* n_and_heads, uint32_t* occluded);
void launch_sobol_probe(hipStream_t s, uint32_t n_points, uint32_t n, const uint32_t* index, const uint32_t* seed, float* out_xy);
void launch_math_probe(hipStream_t s, int fn, uint32_t n, const float* a, const float* b, float* o0, float* o1, uint64_t seed);
void launch_material_probe(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* normal,
                           const uint8_t* front, const uint32_t* pixel, const uint32_t* sample, uint32_t draws, uint64_t seed, float* out9);
void launch_volume_probe(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* t_max, const float* dist,
                         const uint32_t* pixel, const uint32_t* sample, uint32_t draws, uint64_t seed, float* out9);
void launch_bsdf_probe(hipStream_t s, const SceneView& sv, int material, uint32_t n, const float* incoming, const float* outgoing,
                       const float* normal, const uint8_t* front, float* out4);

} // namespace pt
