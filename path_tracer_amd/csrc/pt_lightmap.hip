// Lightmap baking (pt_bake_lightmap, pt_lightmap_texels, pt_lightmap_dilate) as gfx950 kernels; no reference counterpart.  The arithmetic is
// pt_lightmap.h's, shared with the host evaluations; include/pt_api.h states it.
//
//   k_lm_cover     a workgroup per (triangle, slice of its texel rectangle): the coverage predicate, atomicMin of the triangle index
//   k_lm_resolve   a thread per texel: (u, v) of the owner, surface point and normal under the instance matrix, coverage byte
//   k_lm_rays      a thread per ray: origin P + bias * n, a cosine-distributed direction over n, the stream key
//   k_lm_fold      a thread per (covered texel, channel): the window's radiance added to the texel's sum in sample order; with MOMENTS a
//                  fourth thread per texel adds l(L) * l(L) to its second moment (pt_bake_lightmap_moments)
//   k_lm_select_*  pt_bake_lightmap_adaptive: the active texels {texel, its sample count} compacted in ascending order, two passes, no atomics;
//                  k_lm_rays and k_lm_fold run over that list (LightmapAdaptiveBake) as they run over the covered texels; k_lm_advance
//   k_lm_fold_dir  pt_bake_lightmap_directional: twelve threads per covered texel, the three sums as k_lm_fold and nine first moments L[c] * d[a]
//   k_lm_gradient  a thread per texel: the tangential gradient of the first moments (lm_gradient)
//   k_lm_dilate    a thread per texel: one dilation pass from one buffer pair to the other
//   k_lmf_*        pt_lightmap_denoise: pt_filter.h's a-trous core under pt_lightmap_filter.h's texel rule.  One thread per texel; the spatial variance and the levels
//                  in 16 x 16 workgroups, ping-pong.  Gather-bound like k_dn_level: a tap is three 16-byte loads (colour | variance, P | area,
//                  n | valid), and the valid word decides whether the other two are made
#include <hip/hip_runtime.h>

#include "pt_kernels.h"
#include "pt_lightmap.h"
#include "pt_lightmap_filter.h"

namespace pt {
namespace {

__global__ void __launch_bounds__(256) k_lm_fill(const uint32_t n, const uint32_t value, uint32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = value;
}

// Work item {triangle, first}: texels [first, first + kLightmapSlice) of the triangle's rectangle, row-major inside it.  Whatever order the
// items run in, the lowest triangle index that contains a centre ends up as its owner.
__global__ void __launch_bounds__(256) k_lm_cover(const LightmapView lm, const uint2* __restrict__ items, uint32_t* __restrict__ owner)
{
    const uint2 item = items[blockIdx.x];
    const uint32_t tri = item.x;
    if (tri >= lm.n_tris) return;
    const float* puv = lm.uv + 6u * (size_t)tri;
    const float uv[6] = {puv[0], puv[1], puv[2], puv[3], puv[4], puv[5]};
    LmBox box;
    if (!lm_box(uv, lm.w, lm.h, &box)) return;
    const uint32_t n = box.bw * box.bh; // at most w * h <= 2^26
    const uint32_t end = item.y + kLightmapSlice < n ? item.y + kLightmapSlice : n;
    for (uint32_t t = item.y + threadIdx.x; t < end; t += blockDim.x)
    {
        const uint32_t dj = t / box.bw, i = box.i0 + (t - dj * box.bw), j = box.j0 + dj;
        double u, v;
        if (lm_contains(uv, lm_centre(i, lm.w), lm_centre(j, lm.h), &u, &v)) atomicMin(owner + ((size_t)j * lm.w + i), tri);
    }
}

__global__ void __launch_bounds__(256) k_lm_resolve(const LightmapView lm, const uint32_t* __restrict__ owner, float* __restrict__ uv2,
                                                     float* __restrict__ position, float* __restrict__ normal, uint8_t* __restrict__ coverage)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= lm.w * lm.h) return;
    const uint32_t tri = owner[k];
    float u32 = 0.0f, v32 = 0.0f;
    f3 P{0.0f, 0.0f, 0.0f}, n{0.0f, 0.0f, 0.0f};
    if (tri < lm.n_tris)
    {
        const float* puv = lm.uv + 6u * (size_t)tri;
        const float uv[6] = {puv[0], puv[1], puv[2], puv[3], puv[4], puv[5]};
        const uint32_t j = k / lm.w, i = k - j * lm.w;
        double u = 0.0, v = 0.0;
        (void)lm_contains(uv, lm_centre(i, lm.w), lm_centre(j, lm.h), &u, &v);
        u32 = (float)u; v32 = (float)v;
        float p9[9], n9[9];
        for (int q = 0; q < 9; ++q) { p9[q] = lm.positions[9u * (size_t)tri + q]; n9[q] = lm.normals[9u * (size_t)tri + q]; }
        lm_surface(p9, n9, lm.m, u32, v32, &P, &n);
    }
    uv2[2u * (size_t)k] = u32; uv2[2u * (size_t)k + 1u] = v32;
    float* pp = position + 3u * (size_t)k;
    float* pn = normal + 3u * (size_t)k;
    pp[0] = P.x; pp[1] = P.y; pp[2] = P.z;
    pn[0] = n.x; pn[1] = n.y; pn[2] = n.z;
    coverage[k] = tri < lm.n_tris ? (uint8_t)1u : (uint8_t)0u;
}

// item `rank` of a bake, {texel, the texel's first sample of the call}: the rank-th covered texel from the call's first_sample, or (adaptive)
// the rank-th entry of the selection's list, whose texel continues from its own count
__device__ __forceinline__ uint2 bake_item(const LightmapBake& lb, uint32_t rank) { return make_uint2(lb.texels[rank], lb.first_sample); }
__device__ __forceinline__ uint2 bake_item(const LightmapAdaptiveBake& lb, uint32_t rank) { return lb.list[rank]; }

// rays [first, first + count) of a bake into entries [0, count) of a ray table: sample first_sample + r % n_samples of covered texel r / n_samples,
// or, over a LightmapAdaptiveBake, sample list[r / n_samples].y + r % n_samples of texel list[r / n_samples].x
template <class Bake>
__global__ void __launch_bounds__(256) k_lm_rays(const Bake lb, const uint64_t first, const uint32_t count, float* __restrict__ o,
                                                  float* __restrict__ d, uint2* __restrict__ key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t r = first + i;
    const uint32_t rank = (uint32_t)(r / lb.n_samples);
    const uint2 item = bake_item(lb, rank);
    const uint32_t s = item.y + (uint32_t)(r - (uint64_t)rank * lb.n_samples);
    const uint32_t k = item.x;
    const float* pp = lb.position + 3u * (size_t)k;
    const float* pn = lb.normal + 3u * (size_t)k;
    const f3 n{pn[0], pn[1], pn[2]};
    const f3 org = lm_origin(f3{pp[0], pp[1], pp[2]}, n, lb.bias);
    const f3 dir = lightmap_ray(lb.seed, lb.n_sobol, lb.key_base + k, s, n);
    float* po = o + 3u * (size_t)i;
    float* pd = d + 3u * (size_t)i;
    po[0] = org.x; po[1] = org.y; po[2] = org.z;
    pd[0] = dir.x; pd[1] = dir.y; pd[2] = dir.z;
    key[i] = make_uint2(lb.key_base + k, s);
}

// one channel's chain of k_lm_fold: *dst += src[4 * i] for i in [i0, i1), in order.  The adds form one dependent chain; the loads do not depend on
// it, so eight samples are fetched before their adds, and the next eight can be in flight while those adds run
__device__ __forceinline__ void fold_channel(float* __restrict__ dst, const float* __restrict__ src, uint32_t i0, uint32_t i1)
{
    float acc = *dst;
    uint32_t i = i0;
    for (; i + 8u <= i1; i += 8u)
    {
        float l[8];
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) l[q] = src[4u * (size_t)(i + q)];
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) acc = acc + l[q];
    }
    for (; i < i1; ++i) acc = acc + src[4u * (size_t)i];
    *dst = acc;
}

// sum[texel][c] += L[c] over the window's rays of that texel, in sample order: one thread per (covered texel, channel), a serial fold by
// definition (float addition does not associate) and no atomics: fold_channel.
// MOMENTS: four threads per texel; the fourth folds Q[texel] += l(L) * l(L) over the same rays in the same order, and the other three run
// the code they run without it
template <bool MOMENTS, class Bake>
__global__ void __launch_bounds__(256) k_lm_fold(const Bake lb, const uint64_t first, const uint32_t count, const f4* __restrict__ radiance,
                                                  float* __restrict__ sum, float* __restrict__ sumsq)
{
    constexpr uint32_t CH = MOMENTS ? 4u : 3u;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p0 = (uint32_t)(first / lb.n_samples), p1 = (uint32_t)((first + count - 1u) / lb.n_samples);
    if (t / CH > p1 - p0) return;
    const uint32_t rank = p0 + t / CH, c = t % CH;
    const uint64_t lo = (uint64_t)rank * lb.n_samples, hi = lo + lb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    if (MOMENTS && c == 3u)
    {
        float* q = sumsq + bake_item(lb, rank).x;
        float acc = *q;
        for (uint32_t i = i0; i < i1; ++i)
        {
            const float l = lum(radiance[i]);
            acc = acc + l * l;
        }
        *q = acc;
        return;
    }
    fold_channel(sum + 3u * (size_t)bake_item(lb, rank).x + c, (const float*)radiance + c, i0, i1);
}

// ---- direct light sampled at the texel (pt_bake_lightmap_direct, pt_bake_lightmap_adaptive_direct)
constexpr uint32_t kQueueHole = 0xffffffffu; // the ray queues' tag of a slot no ray took: the any-hit walk skips the entry and writes no result

// one light sample into entry i of a ray queue and of the ce table: (o | t_max, dir | i), or a hole where no shadow ray is cast
__device__ __forceinline__ void put_light_sample(const LmLightSample& ls, const f3 o, const uint32_t i, f4* __restrict__ qa, f4* __restrict__ qb, f4* __restrict__ ce)
{
    qa[i] = ls.cast ? f4{o.x, o.y, o.z, ls.t_max} : f4{0.0f, 0.0f, 0.0f, 0.0f};
    qb[i] = ls.cast ? f4{ls.dir.x, ls.dir.y, ls.dir.z, __uint_as_float(i)} : f4{0.0f, 0.0f, 0.0f, __uint_as_float(kQueueHole)};
    ce[i] = f4{ls.ce.x, ls.ce.y, ls.ce.z, 0.0f};
}

// the light samples of rays [first, first + count) of a bake, k_lm_rays' (rank, s) decomposition: lm_light_sample of the texel's origin and
// normal under the stream of pixel light_key_base + texel.  Three contiguous 16-byte stores per lane, no atomics; thread 0 writes the
// queue's count word (n_and_heads[0], what launch_trace_rays_any reads)
template <class Bake>
__global__ void __launch_bounds__(256) k_lm_light_samples(const Bake lb, const LmLightView lv, const uint32_t light_key_base, const uint64_t first, const uint32_t count,
                                                           f4* __restrict__ qa, f4* __restrict__ qb, f4* __restrict__ ce, uint32_t* __restrict__ n_and_heads)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (i == 0u) n_and_heads[0] = count;
    const uint64_t r = first + i;
    const uint32_t rank = (uint32_t)(r / lb.n_samples);
    const uint2 item = bake_item(lb, rank);
    const uint32_t s = item.y + (uint32_t)(r - (uint64_t)rank * lb.n_samples);
    const uint32_t k = item.x;
    const float* pp = lb.position + 3u * (size_t)k;
    const float* pn = lb.normal + 3u * (size_t)k;
    const f3 n{pn[0], pn[1], pn[2]};
    const f3 org = lm_origin(f3{pp[0], pp[1], pp[2]}, n, lb.bias);
    put_light_sample(lm_light_sample(lv, lb.seed, light_key_base + k, s, org, n), org, i, qa, qb, ce);
}

// pt_lightmap_light_sample on the device: the same body over caller-given keys, samples, origins and normals; the outputs are the hook's
__global__ void __launch_bounds__(256) k_lm_light_sample_hook(const LmLightView lv, const uint64_t seed, const uint32_t n, const uint32_t* __restrict__ key,
                                                               const uint32_t* __restrict__ sample, const float* __restrict__ origin, const float* __restrict__ normal,
                                                               uint32_t* __restrict__ light, f4* __restrict__ dir_t, f4* __restrict__ ce)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* po = origin + 3u * (size_t)i;
    const float* pn = normal + 3u * (size_t)i;
    const LmLightSample ls = lm_light_sample(lv, seed, key[i], sample[i], f3{po[0], po[1], po[2]}, f3{pn[0], pn[1], pn[2]});
    light[i] = ls.light;
    dir_t[i] = f4{ls.dir.x, ls.dir.y, ls.dir.z, ls.t_max};
    ce[i] = f4{ls.ce.x, ls.ce.y, ls.ce.z, ls.cast ? 1.0f : 0.0f};
}

// k_lm_fold over X = G + D (lm_direct_x): per sample from the gather ray's radiance and first-hit id byte, the 256-entry table of the bytes
// that mean an emissive model, the light sample's ce and its shadow ray's result.  Threads per texel and the chain as k_lm_fold has them:
// eight samples' loads ahead of their adds.  A hole's `occluded` word was never written, and its ce is 0 either way
__device__ __forceinline__ float direct_x(const f4* __restrict__ radiance, const uint8_t* __restrict__ id, const uint8_t* __restrict__ emissive,
                                          const f4* __restrict__ ce, const uint32_t* __restrict__ occluded, const uint32_t i, const uint32_t c)
{
    return lm_direct_x(((const float*)(radiance + i))[c], emissive[id[i]] != 0u, ((const float*)(ce + i))[c], occluded[i] != 0u);
}
template <bool MOMENTS, class Bake>
__global__ void __launch_bounds__(256) k_lm_fold_direct(const Bake lb, const uint64_t first, const uint32_t count, const f4* __restrict__ radiance,
                                                         const uint8_t* __restrict__ id, const uint8_t* __restrict__ emissive, const f4* __restrict__ ce,
                                                         const uint32_t* __restrict__ occluded, float* __restrict__ sum, float* __restrict__ sumsq)
{
    constexpr uint32_t CH = MOMENTS ? 4u : 3u;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p0 = (uint32_t)(first / lb.n_samples), p1 = (uint32_t)((first + count - 1u) / lb.n_samples);
    if (t / CH > p1 - p0) return;
    const uint32_t rank = p0 + t / CH, c = t % CH;
    const uint64_t lo = (uint64_t)rank * lb.n_samples, hi = lo + lb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    if (MOMENTS && c == 3u)
    {
        float* q = sumsq + bake_item(lb, rank).x;
        float acc = *q;
        for (uint32_t i = i0; i < i1; ++i)
        {
            const f4 x{direct_x(radiance, id, emissive, ce, occluded, i, 0u), direct_x(radiance, id, emissive, ce, occluded, i, 1u),
                       direct_x(radiance, id, emissive, ce, occluded, i, 2u), 0.0f};
            const float l = lum(x);
            acc = acc + l * l;
        }
        *q = acc;
        return;
    }
    float* dst = sum + 3u * (size_t)bake_item(lb, rank).x + c;
    float acc = *dst;
    uint32_t i = i0;
    for (; i + 8u <= i1; i += 8u)
    {
        float x[8];
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) x[q] = direct_x(radiance, id, emissive, ce, occluded, i + q, c);
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) acc = acc + x[q];
    }
    for (; i < i1; ++i) acc = acc + direct_x(radiance, id, emissive, ce, occluded, i, c);
    *dst = acc;
}

// ---- the texel selection of an adaptive bake (pt_bake_lightmap_adaptive, pt_lightmap_adaptive_mask)
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// is texel k < n_texels active?  n_k: its count; over: a covered texel whose count the call would take beyond 2^24, where f32 stops counting.
// An uncovered texel is read for its coverage byte and nothing else.
__device__ __forceinline__ bool texel_active(const LightmapSelect& sel, const uint32_t k, uint32_t& n_k, bool& over)
{
    n_k = 0u;
    over = false;
    if (!sel.coverage[k]) return false;
    n_k = sel.counts[k];
    over = (uint64_t)n_k + sel.n_samples > (1ull << 24);
    const float* s = sel.sum + 3u * (size_t)k;
    uint32_t n_p;
    bool bad; // (not below the limit: the float is then the count)
    return adaptive_active(f4{s[0], s[1], s[2], (float)n_k}, sel.sumsq[k], sel.cr, n_p, bad);
}

// k_adaptive_count / k_adaptive_write's two passes (pt_kernels.hip) over the texel table: block b owns texels [b * kSelectPerBlock,
// (b + 1) * kSelectPerBlock), thread i of it texels b * kSelectPerBlock + j * 256 + i (j = 0..3), so the list comes out in ascending texel order
// whatever the scheduling.  k_lm_select_count: active texels per block -> block_counts[b]; a count over the limit anywhere sets header[1].
__global__ void __launch_bounds__(256) k_lm_select_count(const LightmapSelect sel, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ header)
{
    __shared__ uint32_t sh_cnt[4];
    const uint32_t base = blockIdx.x * kSelectPerBlock;
    uint32_t mine = 0u;
    bool any_over = false;
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerBlock / 256u; ++j)
    {
        const uint32_t k = base + j * 256u + threadIdx.x;
        if (k >= sel.n_texels) break;
        uint32_t n_k;
        bool over;
        mine += texel_active(sel, k, n_k, over) ? 1u : 0u;
        any_over |= over;
    }
    if (any_over) atomicOr(header + 1, 1u);
    uint32_t w = mine;
    for (int off = 32; off > 0; off >>= 1) w += (uint32_t)__shfl_xor((int)w, off);
    if (lane_id() == 0u) sh_cnt[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0u) block_counts[blockIdx.x] = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
}
// k_lm_select_write: the block's offset is the sum of the counts of the blocks before it; each group of 256 texels is compacted with one
// ballot per wave, mbcnt for a lane's rank in its wave and the waves' counts in LDS.  The last block writes the total to header[0].
__global__ void __launch_bounds__(256) k_lm_select_write(const LightmapSelect sel, const uint32_t* __restrict__ block_counts, uint2* __restrict__ list,
                                                          uint32_t* __restrict__ header)
{
    __shared__ uint32_t sh_sum[4];
    __shared__ uint32_t sh_wave[kSelectPerBlock / 256u][4];
    const uint32_t wid = threadIdx.x >> 6;
    uint32_t before = 0u;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256u) before += block_counts[b];
    for (int off = 32; off > 0; off >>= 1) before += (uint32_t)__shfl_xor((int)before, off);
    if (lane_id() == 0u) sh_sum[wid] = before;
    const uint32_t base = blockIdx.x * kSelectPerBlock;
    bool act[kSelectPerBlock / 256u];
    uint32_t nk[kSelectPerBlock / 256u];
    uint64_t m[kSelectPerBlock / 256u];
#pragma unroll
    for (uint32_t j = 0; j < kSelectPerBlock / 256u; ++j)
    {
        const uint32_t k = base + j * 256u + threadIdx.x;
        bool over;
        nk[j] = 0u;
        act[j] = k < sel.n_texels && texel_active(sel, k, nk[j], over);
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
        if (act[j]) list[pos + mbcnt64(m[j])] = make_uint2(base + j * 256u + threadIdx.x, nk[j]);
        off += sh_wave[j][0] + sh_wave[j][1] + sh_wave[j][2] + sh_wave[j][3];
    }
    if (blockIdx.x + 1u == gridDim.x && threadIdx.x == 0u) header[0] = off;
}
// the call's samples are in the sums: every listed texel's count moves on, once, after the last window's fold
__global__ void __launch_bounds__(256) k_lm_advance(const uint2* __restrict__ list, const uint32_t n_active, const uint32_t n_samples, uint32_t* __restrict__ counts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_active) return;
    const uint2 e = list[i];
    counts[e.x] = e.y + n_samples;
}

// pt_bake_lightmap_directional: twelve threads per covered texel.  The first three fold the sums with the code they run in k_lm_fold; thread
// 3 + 3 * a + c folds the first moment M[texel][a][c] += L[c] * d[a] over the same rays in the same order, d being the window's ray table
// (k_lm_rays' directions, still live after the integration: lightmap_ray's bits).  The product is rounded, then the add; each chain is one
// dependent add chain like the sums', so it keeps their shape: eight samples' loads ahead of their adds
__global__ void __launch_bounds__(256) k_lm_fold_dir(const LightmapBake lb, const uint64_t first, const uint32_t count, const f4* __restrict__ radiance,
                                                      const float* __restrict__ d, float* __restrict__ sum, float* __restrict__ dir)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p0 = (uint32_t)(first / lb.n_samples), p1 = (uint32_t)((first + count - 1u) / lb.n_samples);
    if (t / 12u > p1 - p0) return;
    const uint32_t rank = p0 + t / 12u, c = t % 12u;
    const uint64_t lo = (uint64_t)rank * lb.n_samples, hi = lo + lb.n_samples;
    const uint32_t i0 = (uint32_t)((lo > first ? lo : first) - first), i1 = (uint32_t)((hi < first + count ? hi : first + count) - first);
    if (c < 3u)
    {
        fold_channel(sum + 3u * (size_t)lb.texels[rank] + c, (const float*)radiance + c, i0, i1);
        return;
    }
    const uint32_t m = c - 3u, axis = m / 3u;
    float* dst = dir + 9u * (size_t)lb.texels[rank] + m;
    const float* src = (const float*)radiance + (m - 3u * axis);
    const float* dsrc = d + axis;
    float acc = *dst;
    uint32_t i = i0;
    for (; i + 8u <= i1; i += 8u)
    {
        float l[8], w[8];
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) { l[q] = src[4u * (size_t)(i + q)]; w[q] = dsrc[3u * (size_t)(i + q)]; }
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) acc = acc + l[q] * w[q];
    }
    for (; i < i1; ++i) acc = acc + src[4u * (size_t)i] * dsrc[3u * (size_t)i];
    *dst = acc;
}

// pt_lightmap_gradient on the device: lm_gradient (pt_lightmap.h) of every texel of the table k_lm_cover / k_lm_resolve made; zeros where uncovered
__global__ void __launch_bounds__(256) k_lm_gradient(const uint32_t n, const uint8_t* __restrict__ coverage, const float* __restrict__ normal, const float n_samples,
                                                      const float* __restrict__ dir, float* __restrict__ grad)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float in[9], out[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (coverage[k])
    {
#pragma unroll
        for (uint32_t q = 0; q < 9u; ++q) in[q] = dir[9u * (size_t)k + q];
        const float* pn = normal + 3u * (size_t)k;
        lm_gradient(in, f3{pn[0], pn[1], pn[2]}, n_samples, out);
    }
#pragma unroll
    for (uint32_t q = 0; q < 9u; ++q) grad[9u * (size_t)k + q] = out[q];
}

__global__ void __launch_bounds__(256) k_lm_dilate(const uint32_t w, const uint32_t h, const float* __restrict__ rgb, const uint8_t* __restrict__ cov,
                                                    float* __restrict__ rgb_out, uint8_t* __restrict__ cov_out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= w * h) return;
    const uint32_t j = k / w, i = k - j * w;
    float out[3];
    const bool filled = lm_dilate(rgb, cov, w, h, i, j, out);
    if (!filled) { out[0] = rgb[3u * (size_t)k]; out[1] = rgb[3u * (size_t)k + 1u]; out[2] = rgb[3u * (size_t)k + 2u]; }
    rgb_out[3u * (size_t)k] = out[0]; rgb_out[3u * (size_t)k + 1u] = out[1]; rgb_out[3u * (size_t)k + 2u] = out[2];
    cov_out[k] = filled ? (uint8_t)2u : cov[k];
}

// ---- the texel filter (pt_lightmap_denoise)
// COUNTS (pt_lightmap_denoise_counts): a texel's sample count is counts[k] instead of the map's n
template <bool COUNTS>
__global__ void __launch_bounds__(256) k_lmf_prep(const LightmapView lm, const uint32_t* __restrict__ prim, const float* __restrict__ position,
                                                   const float* __restrict__ normal, const float* __restrict__ sum, const float* __restrict__ sumsq, const float n,
                                                   const uint32_t* __restrict__ counts, f4* __restrict__ cv, f4* __restrict__ pa, f4* __restrict__ nv,
                                                   float* __restrict__ area)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= lm.w * lm.h) return;
    lmf_prep(k, lm.w, lm.h, prim, position, normal, lm.positions, lm.uv, sum, sumsq, COUNTS ? (float)counts[k] : n, cv, pa, nv);
    if (area) area[k] = pa[k].w;
}

__global__ void __launch_bounds__(256) k_lmf_spatial_var(const int w, const int h, const LmFilterK p, const f4* __restrict__ cv_in, const f4* __restrict__ pa,
                                                          const f4* __restrict__ nv, f4* __restrict__ cv_out)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    if (nv[i].w == 0.0f) { cv_out[i] = f4{0.0f, 0.0f, 0.0f, 0.0f}; return; }
    const f4 c = cv_in[i];
    cv_out[i] = f4{c.x, c.y, c.z, spatial_variance(TexelRule(p, pa, nv, i), w, h, p, cv_in, pa, nv, x, y)};
}

// FINAL: the last level writes the map's rgb (zeros for an uncovered texel) instead of (c', var')
template <bool FINAL>
__global__ void __launch_bounds__(256) k_lmf_level(const int w, const int h, const int s, const LmFilterK p, const f4* __restrict__ cv_in, const f4* __restrict__ pa,
                                                    const f4* __restrict__ nv, f4* __restrict__ cv_out, float* __restrict__ rgb)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    f4 c{0.0f, 0.0f, 0.0f, 0.0f};
    if (nv[i].w != 0.0f) c = atrous_level(TexelRule(p, pa, nv, i), w, h, s, p, cv_in, pa, nv, x, y);
    if (FINAL) { rgb[3u * i] = c.x; rgb[3u * i + 1u] = c.y; rgb[3u * i + 2u] = c.z; }
    else cv_out[i] = c;
}

inline dim3 blocks_for(uint64_t n) { return dim3((uint32_t)((n + 255u) / 256u)); }

} // namespace

void launch_lightmap_cover(hipStream_t s, const LightmapView& lm, const uint2* items, uint32_t n_items, uint32_t* owner)
{
    hipLaunchKernelGGL(k_lm_fill, blocks_for((uint64_t)lm.w * lm.h), dim3(256), 0, s, lm.w * lm.h, MISS_ID, owner);
    if (n_items) hipLaunchKernelGGL(k_lm_cover, dim3(n_items), dim3(256), 0, s, lm, items, owner);
}
void launch_lightmap_resolve(hipStream_t s, const LightmapView& lm, const uint32_t* owner, float* uv2, float* position, float* normal, uint8_t* coverage)
{
    hipLaunchKernelGGL(k_lm_resolve, blocks_for((uint64_t)lm.w * lm.h), dim3(256), 0, s, lm, owner, uv2, position, normal, coverage);
}
void launch_lightmap_rays(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, float* o, float* d, uint2* key)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_lm_rays<LightmapBake>, blocks_for(count), dim3(256), 0, s, lb, first, count, o, d, key);
}
void launch_lightmap_rays(hipStream_t s, const LightmapAdaptiveBake& lb, uint64_t first, uint32_t count, float* o, float* d, uint2* key)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_lm_rays<LightmapAdaptiveBake>, blocks_for(count), dim3(256), 0, s, lb, first, count, o, d, key);
}
void launch_lightmap_fold(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const f4* radiance, float* sum, float* sumsq)
{
    if (count == 0) return;
    const uint64_t texels = (first + count - 1u) / lb.n_samples - first / lb.n_samples + 1u;
    if (sumsq) hipLaunchKernelGGL((k_lm_fold<true, LightmapBake>), blocks_for(texels * 4u), dim3(256), 0, s, lb, first, count, radiance, sum, sumsq);
    else hipLaunchKernelGGL((k_lm_fold<false, LightmapBake>), blocks_for(texels * 3u), dim3(256), 0, s, lb, first, count, radiance, sum, sumsq);
}
void launch_lightmap_fold(hipStream_t s, const LightmapAdaptiveBake& lb, uint64_t first, uint32_t count, const f4* radiance, float* sum, float* sumsq)
{
    if (count == 0) return;
    const uint64_t texels = (first + count - 1u) / lb.n_samples - first / lb.n_samples + 1u;
    hipLaunchKernelGGL((k_lm_fold<true, LightmapAdaptiveBake>), blocks_for(texels * 4u), dim3(256), 0, s, lb, first, count, radiance, sum, sumsq);
}
template <class Bake>
static void light_samples(hipStream_t s, const Bake& lb, const LmLightView& lv, uint32_t light_key_base, uint64_t first, uint32_t count, RayQueue q, f4* ce,
                          uint32_t* n_and_heads)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_lm_light_samples<Bake>, blocks_for(count), dim3(256), 0, s, lb, lv, light_key_base, first, count, q.a, q.b, ce, n_and_heads);
}
void launch_lightmap_light_samples(hipStream_t s, const LightmapBake& lb, const LmLightView& lv, uint32_t light_key_base, uint64_t first, uint32_t count, RayQueue q,
                                   f4* ce, uint32_t* n_and_heads)
{
    light_samples(s, lb, lv, light_key_base, first, count, q, ce, n_and_heads);
}
void launch_lightmap_light_samples(hipStream_t s, const LightmapAdaptiveBake& lb, const LmLightView& lv, uint32_t light_key_base, uint64_t first, uint32_t count,
                                   RayQueue q, f4* ce, uint32_t* n_and_heads)
{
    light_samples(s, lb, lv, light_key_base, first, count, q, ce, n_and_heads);
}
void launch_lightmap_light_sample_hook(hipStream_t s, const LmLightView& lv, uint64_t seed, uint32_t n, const uint32_t* key, const uint32_t* sample,
                                       const float* origin, const float* normal, uint32_t* light, f4* dir_t, f4* ce)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_lm_light_sample_hook, blocks_for(n), dim3(256), 0, s, lv, seed, n, key, sample, origin, normal, light, dir_t, ce);
}
void launch_lightmap_fold_direct(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const LightmapDirectWindow& w, float* sum, float* sumsq)
{
    if (count == 0) return;
    const uint64_t texels = (first + count - 1u) / lb.n_samples - first / lb.n_samples + 1u;
    if (sumsq) hipLaunchKernelGGL((k_lm_fold_direct<true, LightmapBake>), blocks_for(texels * 4u), dim3(256), 0, s, lb, first, count, w.radiance, w.id, w.emissive, w.ce, w.occluded, sum, sumsq);
    else hipLaunchKernelGGL((k_lm_fold_direct<false, LightmapBake>), blocks_for(texels * 3u), dim3(256), 0, s, lb, first, count, w.radiance, w.id, w.emissive, w.ce, w.occluded, sum, sumsq);
}
void launch_lightmap_fold_direct(hipStream_t s, const LightmapAdaptiveBake& lb, uint64_t first, uint32_t count, const LightmapDirectWindow& w, float* sum, float* sumsq)
{
    if (count == 0) return;
    const uint64_t texels = (first + count - 1u) / lb.n_samples - first / lb.n_samples + 1u;
    hipLaunchKernelGGL((k_lm_fold_direct<true, LightmapAdaptiveBake>), blocks_for(texels * 4u), dim3(256), 0, s, lb, first, count, w.radiance, w.id, w.emissive, w.ce, w.occluded, sum, sumsq);
}
uint32_t lightmap_select_blocks(uint32_t n_texels) { return (n_texels + kSelectPerBlock - 1u) / kSelectPerBlock; }
void launch_lightmap_select(hipStream_t s, const LightmapSelect& sel, uint32_t* block_counts, uint2* list, uint32_t* header)
{
    const uint32_t blocks = lightmap_select_blocks(sel.n_texels);
    if (blocks == 0) return;
    hipLaunchKernelGGL(k_lm_select_count, dim3(blocks), dim3(256), 0, s, sel, block_counts, header);
    hipLaunchKernelGGL(k_lm_select_write, dim3(blocks), dim3(256), 0, s, sel, (const uint32_t*)block_counts, list, header);
}
void launch_lightmap_advance(hipStream_t s, const uint2* list, uint32_t n_active, uint32_t n_samples, uint32_t* counts)
{
    if (n_active == 0) return;
    hipLaunchKernelGGL(k_lm_advance, blocks_for(n_active), dim3(256), 0, s, list, n_active, n_samples, counts);
}
void launch_lightmap_fold_directional(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const f4* radiance, const float* d, float* sum, float* dir)
{
    if (count == 0) return;
    const uint64_t texels = (first + count - 1u) / lb.n_samples - first / lb.n_samples + 1u;
    hipLaunchKernelGGL(k_lm_fold_dir, blocks_for(texels * 12u), dim3(256), 0, s, lb, first, count, radiance, d, sum, dir);
}
void launch_lightmap_gradient(hipStream_t s, uint32_t n_texels, const uint8_t* coverage, const float* normal, uint32_t n_samples, const float* dir, float* grad)
{
    hipLaunchKernelGGL(k_lm_gradient, blocks_for(n_texels), dim3(256), 0, s, n_texels, coverage, normal, (float)n_samples, dir, grad);
}
void launch_lightmap_dilate(hipStream_t s, uint32_t w, uint32_t h, const float* rgb, const uint8_t* cov, float* rgb_out, uint8_t* cov_out)
{
    hipLaunchKernelGGL(k_lm_dilate, blocks_for((uint64_t)w * h), dim3(256), 0, s, w, h, rgb, cov, rgb_out, cov_out);
}

void launch_lightmap_denoise(hipStream_t s, const LightmapView& lm, const LmFilterK& p, uint32_t n_samples, bool moments, const LmFilterImages& im)
{
    const int w = (int)lm.w, h = (int)lm.h;
    const dim3 tile(16, 16), grid((lm.w + 15u) / 16u, (lm.h + 15u) / 16u);
    f4* cur = im.cv_a;
    f4* other = im.cv_b;
    const float* q = moments ? im.sumsq : (const float*)nullptr;
    if (im.counts) hipLaunchKernelGGL(k_lmf_prep<true>, blocks_for((uint64_t)lm.w * lm.h), dim3(256), 0, s, lm, im.prim, im.position, im.normal, im.sum, q, 0.0f, im.counts, cur, im.pa, im.nv, im.area);
    else hipLaunchKernelGGL(k_lmf_prep<false>, blocks_for((uint64_t)lm.w * lm.h), dim3(256), 0, s, lm, im.prim, im.position, im.normal, im.sum, q, (float)n_samples, im.counts, cur, im.pa, im.nv, im.area);
    if (!moments)
    {
        hipLaunchKernelGGL(k_lmf_spatial_var, grid, tile, 0, s, w, h, p, (const f4*)cur, (const f4*)im.pa, (const f4*)im.nv, other);
        std::swap(cur, other);
    }
    for (uint32_t it = 0; it < p.iterations; ++it)
    {
        if (it + 1u == p.iterations) hipLaunchKernelGGL(k_lmf_level<true>, grid, tile, 0, s, w, h, 1 << it, p, (const f4*)cur, (const f4*)im.pa, (const f4*)im.nv, other, im.rgb);
        else hipLaunchKernelGGL(k_lmf_level<false>, grid, tile, 0, s, w, h, 1 << it, p, (const f4*)cur, (const f4*)im.pa, (const f4*)im.nv, other, im.rgb);
        std::swap(cur, other);
    }
}

} // namespace pt
