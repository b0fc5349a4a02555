// The texel-space denoiser (pt_lightmap_denoise): pt_denoise's a-trous filter on a lightmap's texel table, with one added tap term, REACH,
// which keeps charts that are neighbours in UV space and far apart in the world from exchanging light.  The per-texel steps (prep, spatial
// variance, one level) are written once here for the gfx950 kernels (pt_lightmap.hip) and for the host walk (on_device = 0, the sanitizer
// driver); the tap terms are pt_filter.h's.  include/pt_api.h states the definition; every operation is rounded once, in this order (the
// library is built without contraction).
//
// The three images a tap reads, 16 bytes each: cv = colour | variance, pa = P | texel area, nv = n | valid (1 / 0).  Every covered texel is a
// hit of one model, so pt_denoise's model test has nothing to do here.
#pragma once
#include <utility>
#include <vector>

#include "pt_filter.h"
#include "pt_lightmap.h"

namespace pt {

struct LmFilterK
{
    float sigma_l, sigma_x;
    uint32_t log2_sigma_n;
    uint32_t iterations; // 1..8
    float reach2;        // reach * reach; may be +inf (the term is off)
};

constexpr float kLmFilterEps = 1e-6f; // pt_denoise's

// TEXEL AREA: the world area one texel of a w x h map covers on the triangle with object-space positions p9 and UVs uv
PT_HD float lm_texel_area(const float p9[9], const float uv[6], uint32_t w, uint32_t h)
{
    const f3 pa{p9[0], p9[1], p9[2]}, pb{p9[3], p9[4], p9[5]}, pc{p9[6], p9[7], p9[8]};
    const f3 X = cross3(pb - pa, pc - pa);
    const float A3 = sqrtf(dot3(X, X));
    const float A2 = (float)__builtin_fabs(lm_edge((double)uv[0], (double)uv[1], (double)uv[2], (double)uv[3], (double)uv[4], (double)uv[5]));
    return A3 / ((A2 * (float)w) * (float)h);
}

// squared world distance of two texels: the plane term's d2
PT_HD float lmf_d2(f4 xp, f4 xq)
{
    const float dx = xq.x - xp.x, dy = xq.y - xp.y, dz = xq.z - xp.z;
    return (dx * dx + dy * dy) + dz * dz;
}
// REACH of the tap at texel offset (ox, oy) != (0, 0); lim = (reach * reach) * area_p.  Written this way round: a NaN on the right rejects
// the tap, +inf accepts it
PT_HD bool lmf_reach(float lim, f4 xp, f4 xq, int ox, int oy) { return lmf_d2(xp, xq) <= lim * (float)(ox * ox + oy * oy); }

// the three images' entries of texel k from the texel table (prim, P, n: pt_lightmap_texels'), the model's load-order positions and UVs and
// the sums; n = (float)n_samples; sumsq null: variance 0, the spatial pass fills it in
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
    float var = 0.0f;
    if (sumsq)
    {
        const float m = lum(a) / a.w;
        float v = sumsq[k] / a.w - m * m;
        if (!(v > 0.0f)) v = 0.0f;
        var = v / a.w;
    }
    float p9[9], uv[6];
    for (int q = 0; q < 9; ++q) p9[q] = positions9[9u * (size_t)t + q];
    for (int q = 0; q < 6; ++q) uv[q] = uvs6[6u * (size_t)t + q];
    cv[k] = f4{a.x / a.w, a.y / a.w, a.z / a.w, var};
    pa[k] = f4{position[3u * (size_t)k], position[3u * (size_t)k + 1u], position[3u * (size_t)k + 2u], lm_texel_area(p9, uv, w, h)};
    nv[k] = f4{normal[3u * (size_t)k], normal[3u * (size_t)k + 1u], normal[3u * (size_t)k + 2u], 1.0f};
}

// pt_filter.h's spatial_variance of a covered texel (x, y) with the reach test on every neighbour
PT_HD float lmf_spatial_variance(int w, int h, const LmFilterK& p, const f4* cv, const f4* pa, const f4* nv, int x, int y)
{
    const size_t i = (size_t)y * w + x;
    const f4 np = nv[i], xp = pa[i];
    const float lim = p.reach2 * xp.w;
    float sw = 0.0f, sl = 0.0f, sll = 0.0f;
    for (int dy = -3; dy <= 3; ++dy)
    {
        const int yy = y + dy;
        if (yy < 0 || yy >= h) continue;
        for (int dx = -3; dx <= 3; ++dx)
        {
            const int xx = x + dx;
            if (xx < 0 || xx >= w) continue;
            const size_t q = (size_t)yy * w + xx;
            float wt = 1.0f;
            if (dx != 0 || dy != 0)
            {
                const f4 nq = nv[q];
                if (nq.w == 0.0f) continue;
                const f4 xq = pa[q];
                if (!lmf_reach(lim, xp, xq, dx, dy)) continue;
                wt = normal_w(np, nq, p.log2_sigma_n) * exp_det(-plane(np, xp, xq, p.sigma_x));
            }
            const float l = lum(cv[q]);
            sw = sw + wt;
            sl = sl + wt * l;
            sll = sll + wt * (l * l);
        }
    }
    const float mu = sl / sw;
    float v = sll / sw - mu * mu;
    if (!(v > 0.0f)) v = 0.0f;
    return v;
}

// one a-trous level, step s, of a covered texel (x, y): (c', var') as pt_denoise's level, a neighbour being a covered texel inside the map
// that passes the reach test
PT_HD f4 lmf_level(int w, int h, int s, const LmFilterK& p, const f4* cv, const f4* pa, const f4* nv, int x, int y)
{
    const size_t i = (size_t)y * w + x;
    const f4 cp = cv[i], np = nv[i], xp = pa[i];
    const float lim = p.reach2 * xp.w;
    const float kb[3] = {0.25f, 0.5f, 0.25f};
    float sg = 0.0f, sk = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
    {
        const int yy = y + dy;
        if (yy < 0 || yy >= h) continue;
        for (int dx = -1; dx <= 1; ++dx)
        {
            const int xx = x + dx;
            if (xx < 0 || xx >= w) continue;
            const size_t q = (size_t)yy * w + xx;
            if ((dx != 0 || dy != 0) && (nv[q].w == 0.0f || !lmf_reach(lim, xp, pa[q], dx, dy))) continue;
            const float k = kb[dx + 1] * kb[dy + 1];
            sg = sg + k * cv[q].w;
            sk = sk + k;
        }
    }
    const float g = sg / sk;
    const float inv = 1.0f / (p.sigma_l * sqrtf(g) + kLmFilterEps);
    const float lp = lum(cp);
    const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.0f, sr = 0.0f, sgc = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
    {
        const int yy = y + s * dy;
        if (yy < 0 || yy >= h) continue;
        for (int dx = -2; dx <= 2; ++dx)
        {
            const int xx = x + s * dx;
            if (xx < 0 || xx >= w) continue;
            const size_t q = (size_t)yy * w + xx;
            float e = 1.0f;
            if (dx != 0 || dy != 0)
            {
                const f4 nq = nv[q];
                if (nq.w == 0.0f) continue;
                const f4 xq = pa[q];
                if (!lmf_reach(lim, xp, xq, s * dx, s * dy)) continue;
                const float al = fabsf(lp - lum(cv[q])) * inv;
                e = normal_w(np, nq, p.log2_sigma_n) * exp_det(-(plane(np, xp, xq, p.sigma_x) + al));
            }
            const f4 cq = cv[q];
            const float wt = (hk[dx + 2] * hk[dy + 2]) * e;
            sw = sw + wt;
            sr = sr + wt * cq.x;
            sgc = sgc + wt * cq.y;
            sb = sb + wt * cq.z;
            sv = sv + (wt * wt) * cq.w;
        }
    }
    return f4{sr / sw, sgc / sw, sb / sw, sv / (sw * sw)};
}

// The whole filter on the host: the walk on_device = 0 does.  prim, position, normal: the texel table; positions9, uvs6: the model's
// load-order arrays; rgb_mean w * h * 3; texel_area w * h or null
inline void lmf_filter_host(uint32_t w, uint32_t h, const LmFilterK& p, const uint32_t* prim, const float* position, const float* normal,
                            const float* positions9, const float* uvs6, const float* sum, const float* sumsq, uint32_t n_samples, float* rgb_mean,
                            float* texel_area)
{
    const size_t px = (size_t)w * h;
    std::vector<f4> cv(px), other(px), pa(px), nv(px);
    for (size_t k = 0; k < px; ++k) lmf_prep((uint32_t)k, w, h, prim, position, normal, positions9, uvs6, sum, sumsq, (float)n_samples, cv.data(), pa.data(), nv.data());
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
                other[i] = nv[i].w == 0.0f ? f4{0.0f, 0.0f, 0.0f, 0.0f} : f4{c.x, c.y, c.z, lmf_spatial_variance(iw, ih, p, cv.data(), pa.data(), nv.data(), x, y)};
            }
        std::swap(cv, other);
    }
    for (uint32_t it = 0; it < p.iterations; ++it)
    {
        for (int y = 0; y < ih; ++y)
            for (int x = 0; x < iw; ++x)
            {
                const size_t i = (size_t)y * w + x;
                other[i] = nv[i].w == 0.0f ? f4{0.0f, 0.0f, 0.0f, 0.0f} : lmf_level(iw, ih, 1 << it, p, cv.data(), pa.data(), nv.data(), x, y);
            }
        std::swap(cv, other);
    }
    for (size_t k = 0; k < px; ++k) { rgb_mean[3 * k] = cv[k].x; rgb_mean[3 * k + 1] = cv[k].y; rgb_mean[3 * k + 2] = cv[k].z; }
}

} // namespace pt
