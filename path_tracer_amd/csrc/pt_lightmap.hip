// Lightmap baking (pt_bake_lightmap, pt_lightmap_texels, pt_lightmap_dilate) as gfx950 kernels; no reference counterpart.  The arithmetic is
// pt_lightmap.h's, shared with the host evaluations; include/pt_api.h states it.
//
//   k_lm_cover     a workgroup per (triangle, slice of its texel rectangle): the coverage predicate, atomicMin of the triangle index
//   k_lm_resolve   a thread per texel: (u, v) of the owner, surface point and normal under the instance matrix, coverage byte
//   k_lm_rays      a thread per ray: origin P + bias * n, a cosine-distributed direction over n, the stream key
//   k_lm_fold      a thread per (covered texel, channel): the window's radiance added to the texel's sum in sample order; with MOMENTS a
//                  fourth thread per texel adds l(L) * l(L) to its second moment (pt_bake_lightmap_moments)
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

// rays [first, first + count) of a bake into entries [0, count) of a ray table: sample first_sample + r % n_samples of covered texel r / n_samples
__global__ void __launch_bounds__(256) k_lm_rays(const LightmapBake lb, const uint64_t first, const uint32_t count, float* __restrict__ o,
                                                  float* __restrict__ d, uint2* __restrict__ key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t r = first + i;
    const uint32_t rank = (uint32_t)(r / lb.n_samples), s = lb.first_sample + (uint32_t)(r - (uint64_t)rank * lb.n_samples);
    const uint32_t k = lb.texels[rank];
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
template <bool MOMENTS>
__global__ void __launch_bounds__(256) k_lm_fold(const LightmapBake lb, const uint64_t first, const uint32_t count, const f4* __restrict__ radiance,
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
        float* q = sumsq + lb.texels[rank];
        float acc = *q;
        for (uint32_t i = i0; i < i1; ++i)
        {
            const float l = lum(radiance[i]);
            acc = acc + l * l;
        }
        *q = acc;
        return;
    }
    fold_channel(sum + 3u * (size_t)lb.texels[rank] + c, (const float*)radiance + c, i0, i1);
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
__global__ void __launch_bounds__(256) k_lmf_prep(const LightmapView lm, const uint32_t* __restrict__ prim, const float* __restrict__ position,
                                                   const float* __restrict__ normal, const float* __restrict__ sum, const float* __restrict__ sumsq, const float n,
                                                   f4* __restrict__ cv, f4* __restrict__ pa, f4* __restrict__ nv, float* __restrict__ area)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= lm.w * lm.h) return;
    lmf_prep(k, lm.w, lm.h, prim, position, normal, lm.positions, lm.uv, sum, sumsq, n, cv, pa, nv);
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
    hipLaunchKernelGGL(k_lm_rays, blocks_for(count), dim3(256), 0, s, lb, first, count, o, d, key);
}
void launch_lightmap_fold(hipStream_t s, const LightmapBake& lb, uint64_t first, uint32_t count, const f4* radiance, float* sum, float* sumsq)
{
    if (count == 0) return;
    const uint64_t texels = (first + count - 1u) / lb.n_samples - first / lb.n_samples + 1u;
    if (sumsq) hipLaunchKernelGGL(k_lm_fold<true>, blocks_for(texels * 4u), dim3(256), 0, s, lb, first, count, radiance, sum, sumsq);
    else hipLaunchKernelGGL(k_lm_fold<false>, blocks_for(texels * 3u), dim3(256), 0, s, lb, first, count, radiance, sum, sumsq);
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
    hipLaunchKernelGGL(k_lmf_prep, blocks_for((uint64_t)lm.w * lm.h), dim3(256), 0, s, lm, im.prim, im.position, im.normal, im.sum, moments ? im.sumsq : (const float*)nullptr,
                       (float)n_samples, cur, im.pa, im.nv, im.area);
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
