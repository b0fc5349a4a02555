// The a-trous core of every denoiser (pt_denoise, pt_denoise_albedo, the temporal stage, pt_lightmap_denoise): the tap terms, the 7 x 7
// spatial variance and one level of include/pt_api.h, written once for the gfx950 kernels (pt_post.hip, pt_lightmap.hip) and the host paths
// (pt_temporal.h, pt_lightmap_filter.h).  Every operation is an explicit binary32 operation in the order the header states; build with
// -ffp-contract=off.
//
// What differs between the filters is the NEIGHBOUR RULE, a small struct built per centre pixel p:
//   neighbour(q, ox, oy, nq)   is the tap q inside the image, at offset (ox, oy) != (0, 0) from p, a neighbour?  (the centre always is.)
//                              nq <- the neighbour's normal where geometry() holds: the rule reads it, since where the valid word comes with
//                              the normal the two are one 16-byte load, made before the rule's other tests
//   geometry()                 do the normal and plane terms apply to p's taps?  Where not, no tap's position is read
// ScreenRule, ScreenAllValidRule (below) and TexelRule (pt_lightmap_filter.h) are the three there are.
#pragma once
#include "pt_math.h"
#include "pt_types.h"

namespace pt {

// the filter's parameters (pt_denoise_params, validated by the host)
struct DenoiseK
{
    float sigma_l, sigma_x;
    uint32_t log2_sigma_n; // max(0, n_p . n_q) is squared this many times
    uint32_t iterations;   // 1..8
};
constexpr float kFilterEps = 1e-6f;

PT_HD float lum(f4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
// max(0, n_p . n_q)^(2^log2_sn) and the plane term a_x = |n_p . (x_q - x_p)| / (sigma_x * |x_q - x_p|) (0 where x_q == x_p) of two hits
PT_HD float normal_w(f4 np, f4 nq, uint32_t log2_sn)
{
    const float nd = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    float wn = nd > 0.0f ? nd : 0.0f;
    for (uint32_t k = 0; k < log2_sn; ++k) wn = wn * wn;
    return wn;
}
PT_HD float plane(f4 np, f4 xp, f4 xq, float sigma_x)
{
    const float dx = xq.x - xp.x, dy = xq.y - xp.y, dz = xq.z - xp.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 > 0.0f ? fabsf((np.x * dx + np.y * dy) + np.z * dz) / (sigma_x * sqrtf(d2)) : 0.0f;
}

// pt_denoise_albedo's divisor: (1, 1, 1) for a miss, else the albedo floored at 2^-10 per channel
constexpr float kAlbedoFloor = 0x1p-10f;
PT_HD f4 divisor(uint32_t model, f4 A)
{
    if (model == MISS_ID) return f4{1.0f, 1.0f, 1.0f, 0.0f};
    return f4{A.x > kAlbedoFloor ? A.x : kAlbedoFloor, A.y > kAlbedoFloor ? A.y : kAlbedoFloor, A.z > kAlbedoFloor ? A.z : kAlbedoFloor, 0.0f};
}

// the variance of the mean of a.w samples from their sums: a = the colour sums | n, q = the sum of l * l (the adaptive criterion's e2)
PT_HD float mean_variance(f4 a, float q)
{
    const float m = lum(a) / a.w;
    float v = q / a.w - m * m;
    if (!(v > 0.0f)) v = 0.0f;
    return v / a.w;
}

// the frame filters' rule: a neighbour is a valid pixel (nv.w != 0) of the centre's model; a miss centre has no geometry
struct ScreenRule
{
    const f4* nv;
    const uint32_t* model;
    uint32_t mp;
    PT_HD ScreenRule(const f4* nv_, const uint32_t* model_, size_t p) : nv(nv_), model(model_), mp(model_[p]) {}
    PT_HD bool neighbour(size_t q, int, int, f4& nq) const { nq = nv[q]; return nq.w != 0.0f && model[q] == mp; }
    PT_HD bool geometry() const { return mp != MISS_ID; }
};
// the same where every pixel is valid (the temporal stage, whose nv is the plain normal guide): the normal is read at a hit only
struct ScreenAllValidRule
{
    const f4* nv;
    const uint32_t* model;
    uint32_t mp;
    PT_HD ScreenAllValidRule(const f4* nv_, const uint32_t* model_, size_t p) : nv(nv_), model(model_), mp(model_[p]) {}
    PT_HD bool neighbour(size_t q, int, int, f4& nq) const
    {
        if (model[q] != mp) return false;
        if (geometry()) nq = nv[q];
        return true;
    }
    PT_HD bool geometry() const { return mp != MISS_ID; }
};

// variance of l(c) over the 7 x 7 neighbourhood of pixel (x, y), taps weighted by the normal and plane terms (no luminance term)
template <class Rule>
PT_HD float spatial_variance(const Rule& rule, int w, int h, const DenoiseK& k, const f4* c, const f4* pos, const f4* nv, int x, int y)
{
    const size_t i = (size_t)y * w + x;
    const bool geo = rule.geometry();
    const f4 np = nv[i], xp = pos[i];
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
                f4 nq{0.0f, 0.0f, 0.0f, 0.0f};
                if (!rule.neighbour(q, dx, dy, nq)) continue;
                if (geo) wt = normal_w(np, nq, k.log2_sigma_n) * exp_det(-plane(np, xp, pos[q], k.sigma_x));
            }
            const float l = lum(c[q]);
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

// one a-trous level, step s, of pixel (x, y) of cv = colour | variance: (c', var').  g = the 3 x 3 binomial blur of the variance over the
// neighbours, then the 5 x 5 B3-spline taps p + s (dx, dy) with edge-stopping weights; the centre tap has e = 1 and is always taken.  The
// per-pixel divisor is hoisted out of the tap loop; one exp_det per tap.
template <class Rule>
PT_HD f4 atrous_level(const Rule& rule, int w, int h, int s, const DenoiseK& k, const f4* cv, const f4* pos, const f4* nv, int x, int y)
{
    const size_t i = (size_t)y * w + x;
    const bool geo = rule.geometry();
    const f4 cp = cv[i], np = nv[i], xp = pos[i];
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
            f4 nq{0.0f, 0.0f, 0.0f, 0.0f};
            if ((dx != 0 || dy != 0) && !rule.neighbour(q, dx, dy, nq)) continue;
            const float b = kb[dx + 1] * kb[dy + 1];
            sg = sg + b * cv[q].w;
            sk = sk + b;
        }
    }
    const float g = sg / sk;
    const float inv = 1.0f / (k.sigma_l * sqrtf(g) + kFilterEps);
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
            const f4 cq = cv[q];
            float e = 1.0f;
            if (dx != 0 || dy != 0)
            {
                f4 nq{0.0f, 0.0f, 0.0f, 0.0f};
                if (!rule.neighbour(q, s * dx, s * dy, nq)) continue;
                const float al = fabsf(lp - lum(cq)) * inv;
                e = geo ? normal_w(np, nq, k.log2_sigma_n) * exp_det(-(plane(np, xp, pos[q], k.sigma_x) + al)) : exp_det(-al);
            }
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

} // namespace pt
