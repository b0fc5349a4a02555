// What a tap of the denoiser is (pt_denoise, pt_denoise_albedo, the temporal stage): the terms of include/pt_api.h written once for the
// gfx950 kernels (pt_post.hip) and the host path (pt_temporal.h).  Every operation is an explicit binary32 operation in the order the header
// states; build with -ffp-contract=off.
#pragma once
#include "pt_math.h"
#include "pt_types.h"

namespace pt {

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

// variance of l(c) over the 7 x 7 neighbourhood of pixel (x, y), taps weighted by the model, normal and plane terms (no luminance term).
// VALID_IN_W: a neighbour counts only where nv.w != 0 (the spatial filter's normal | valid image); else every pixel is valid (the temporal
// stage, whose nv is the plain normal guide).  np = nv at (x, y), which the caller has read and found valid.
template <bool VALID_IN_W>
PT_HD float spatial_variance(int w, int h, const f4* c, const f4* pos, const f4* nv, const uint32_t* model, uint32_t log2_sn, float sigma_x, int x, int y, f4 np)
{
    const size_t i = (size_t)y * w + x;
    const uint32_t mp = model[i];
    const bool hit = mp != MISS_ID;
    const f4 xp = pos[i];
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
                if (VALID_IN_W) // the valid word comes with the normal, in one load before the model test; else the normal is read at a hit only
                {
                    const f4 nq = nv[q];
                    if (nq.w == 0.0f || model[q] != mp) continue;
                    if (hit) wt = normal_w(np, nq, log2_sn) * exp_det(-plane(np, xp, pos[q], sigma_x));
                }
                else
                {
                    if (model[q] != mp) continue;
                    if (hit) wt = normal_w(np, nv[q], log2_sn) * exp_det(-plane(np, xp, pos[q], sigma_x));
                }
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

} // namespace pt
