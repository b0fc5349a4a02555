// The texel-space denoiser (pt_lightmap_denoise): pt_denoise's a-trous filter on a lightmap's texel table, with one added tap term, REACH,
// which keeps charts that are neighbours in UV space and far apart in the world from exchanging light.  The spatial variance and the level
// are pt_filter.h's core under the texel rule below; what is the texel filter's own stands here, once for the gfx950 kernels
// (pt_lightmap.hip) and for the host walk (on_device = 0, the sanitizer driver): the texel area, the reach, the prep.  include/pt_api.h
// states the definition; every operation is rounded once, in this order (the library is built without contraction).
//
// The three images a tap reads, 16 bytes each: cv = colour | variance, pa = P | texel area, nv = n | valid (1 / 0).  Every covered texel is a
// hit of one model, so pt_denoise's model test has nothing to do here.
#pragma once
#include <utility>
#include <vector>

#include "pt_filter.h"
#include "pt_lightmap.h"

namespace pt {

struct LmFilterK : DenoiseK
{
    float reach2; // reach * reach; may be +inf (the term is off)
};

// TEXEL AREA: the world area one texel of a w x h map covers on the triangle with object-space positions p9 and UVs uv
PT_HD float lm_texel_area(const float p9[9], const float uv[6], uint32_t w, uint32_t h)
{
    const f3 pa{p9[0], p9[1], p9[2]}, pb{p9[3], p9[4], p9[5]}, pc{p9[6], p9[7], p9[8]};
    const f3 X = cross3(pb - pa, pc - pa);
    const float A3 = sqrtf(dot3(X, X));
    const float A2 = (float)__builtin_fabs(lm_edge((double)uv[0], (double)uv[1], (double)uv[2], (double)uv[3], (double)uv[4], (double)uv[5]));
    return A3 / ((A2 * (float)w) * (float)h);
}

// REACH of the tap at texel offset (ox, oy) != (0, 0): the squared world distance of the two texels (the plane term's d2) against
// lim = (reach * reach) * area_p.  Written this way round: a NaN on the right rejects the tap, +inf accepts it
PT_HD bool lmf_reach(float lim, f4 xp, f4 xq, int ox, int oy)
{
    const float dx = xq.x - xp.x, dy = xq.y - xp.y, dz = xq.z - xp.z;
    return (dx * dx + dy * dy) + dz * dz <= lim * (float)(ox * ox + oy * oy);
}
// the texel filter's neighbour rule (pt_filter.h): a covered texel (nv.w != 0) within reach of the centre p; every centre is a hit
struct TexelRule
{
    const f4 *nv, *pa;
    f4 xp;
    float lim;
    PT_HD TexelRule(const LmFilterK& k, const f4* pa_, const f4* nv_, size_t p) : nv(nv_), pa(pa_), xp(pa_[p]), lim(k.reach2 * pa_[p].w) {}
    PT_HD bool neighbour(size_t q, int ox, int oy, f4& nq) const { nq = nv[q]; return nq.w != 0.0f && lmf_reach(lim, xp, pa[q], ox, oy); }
    PT_HD bool geometry() const { return true; }
};

// the three images' entries of texel k from the texel table (prim, P, n: pt_lightmap_texels'), the model's load-order positions and UVs and
// the sums; n = the texel's sample count as f32 (the map's n_samples, or its own: pt_lightmap_denoise_counts); sumsq null: variance 0, the spatial pass fills it in
PT_HD void lmf_prep(uint32_t k, uint32_t w, uint32_t h, const uint32_t* prim, const float* position, const float* normal, const float* positions9,
                    const float* uvs6, const float* sum, const float* sumsq, float n, f4* cv, f4* pa, f4* nv)
{
    const uint32_t t = prim[k];
    if (t == MISS_ID)
    {
        cv[k] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        pa[k] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        nv[k] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    const f4 a{sum[3u * (size_t)k], sum[3u * (size_t)k + 1u], sum[3u * (size_t)k + 2u], n};
    const float var = sumsq ? mean_variance(a, sumsq[k]) : 0.0f;
    float p9[9], uv[6];
    for (int q = 0; q < 9; ++q) p9[q] = positions9[9u * (size_t)t + q];
    for (int q = 0; q < 6; ++q) uv[q] = uvs6[6u * (size_t)t + q];
    cv[k] = f4{a.x / a.w, a.y / a.w, a.z / a.w, var};
    pa[k] = f4{position[3u * (size_t)k], position[3u * (size_t)k + 1u], position[3u * (size_t)k + 2u], lm_texel_area(p9, uv, w, h)};
    nv[k] = f4{normal[3u * (size_t)k], normal[3u * (size_t)k + 1u], normal[3u * (size_t)k + 2u], 1.0f};
}

// The whole filter on the host: the walk on_device = 0 does.  prim, position, normal: the texel table; positions9, uvs6: the model's
// load-order arrays; rgb_mean w * h * 3; texel_area w * h or null; counts (pt_lightmap_denoise_counts) w * h sample counts, or null: n_samples everywhere
inline void lmf_filter_host(uint32_t w, uint32_t h, const LmFilterK& p, const uint32_t* prim, const float* position, const float* normal,
                            const float* positions9, const float* uvs6, const float* sum, const float* sumsq, uint32_t n_samples, const uint32_t* counts,
                            float* rgb_mean, float* texel_area)
{
    const size_t px = (size_t)w * h;
    std::vector<f4> cv(px), other(px), pa(px), nv(px);
    for (size_t k = 0; k < px; ++k)
        lmf_prep((uint32_t)k, w, h, prim, position, normal, positions9, uvs6, sum, sumsq, (float)(counts ? counts[k] : n_samples), cv.data(), pa.data(), nv.data());
    if (texel_area)
        for (size_t k = 0; k < px; ++k) texel_area[k] = pa[k].w;
    const int iw = (int)w, ih = (int)h;
    if (!sumsq)
    {
        for (int y = 0; y < ih; ++y)
            for (int x = 0; x < iw; ++x)
            {
                const size_t i = (size_t)y * w + x;
                const f4 c = cv[i];
                other[i] = nv[i].w == 0.0f ? f4{0.0f, 0.0f, 0.0f, 0.0f} : f4{c.x, c.y, c.z, spatial_variance(TexelRule(p, pa.data(), nv.data(), i), iw, ih, p, cv.data(), pa.data(), nv.data(), x, y)};
            }
        std::swap(cv, other);
    }
    for (uint32_t it = 0; it < p.iterations; ++it)
    {
        for (int y = 0; y < ih; ++y)
            for (int x = 0; x < iw; ++x)
            {
                const size_t i = (size_t)y * w + x;
                other[i] = nv[i].w == 0.0f ? f4{0.0f, 0.0f, 0.0f, 0.0f} : atrous_level(TexelRule(p, pa.data(), nv.data(), i), iw, ih, 1 << it, p, cv.data(), pa.data(), nv.data(), x, y);
            }
        std::swap(cv, other);
    }
    for (size_t k = 0; k < px; ++k) { rgb_mean[3 * k] = cv[k].x; rgb_mean[3 * k + 1] = cv[k].y; rgb_mean[3 * k + 2] = cv[k].z; }
}

} // namespace pt
