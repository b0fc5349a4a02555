// The temporal stage of the denoiser (pt_frame_temporal / pt_post_temporal): the per-pixel steps of include/pt_api.h, written once for the
// host path and the gfx950 kernels (pt_post.hip), as pt_materials.h is.  Every operation is an explicit binary32 operation in the order the
// header states; build with -ffp-contract=off.
//
// Records of the previous call, one per pixel, each read with one 16-byte (M: 8-byte) load:
//   hist : C.rgb | N          mom : mu1, mu2          xq : X'.xyz | t'          gq : n'.xyz | the bits of m'
// A tap is tested on m' and N (gq, hist) before xq and mom are touched.
//
// The options of pt_temporal_params are template parameters, so that the plain stage compiles to what it was: RESCUE (step 3b: a pixel whose
// listed taps all failed searches the 3 x 3 around its reprojected position), MEAN (PT_TEMPORAL_LENGTH_MEAN: the history length is the taps'
// weighted mean, not their least) and DEMOD (cur is divided by the pixel's divisor kdiv, pt_filter.h's, where it is loaded).
#pragma once
#include <type_traits>

#include "pt_filter.h"

namespace pt {

struct f2 { float x, y; };

struct TemporalK
{
    float alpha, alpha_moments, normal_min, plane_max; // defaults filled in
};
constexpr float kTemporalMaxN = 65535.0f;
constexpr float kTemporalMomentsN = 4.0f; // history length from which the moments carry the variance

struct TemporalImages
{
    int w, h;
    const f4* hist;  // previous call
    const f2* mom;
    const f4* xq;
    const f4* gq;
    const f4* cur;   // this frame: sample, position | t, normal, model
    const f4* pos;
    const f4* nrm;
    const uint32_t* model;
    const f4* xprev; // carried back (the position / the normal where nothing moved)
    const f4* nprev;
    const f2* vel;   // null: at rest
};
struct TemporalOut
{
    f4 h; // C.rgb | N
    f2 m; // mu1, mu2
};

// n carried back by the linear parts of the instance's inverse and previous forward matrix (rows of the 3x4s), as X_PREV carries the point
PT_HD f4 motion_normal(const float inv[12], const float prv[12], f4 n)
{
    float o[3], q[3];
    for (int k = 0; k < 3; ++k) o[k] = (inv[4 * k] * n.x + inv[4 * k + 1] * n.y) + inv[4 * k + 2] * n.z;
    for (int k = 0; k < 3; ++k) q[k] = (prv[4 * k] * o[0] + prv[4 * k + 1] * o[1]) + prv[4 * k + 2] * o[2];
    return f4{q[0], q[1], q[2], n.w};
}

// a tap's geometry test on a hit (ok: what it passed so far): its normal n' against the carried-back normal np, and its point X' within `bound` = plane_max * t of the
// plane through the carried-back point xp
PT_HD bool tap_geometry_ok(bool ok, f4 np, f4 xp, f4 ng, f4 xq, float normal_min, float bound)
{
    const float nd = (np.x * ng.x + np.y * ng.y) + np.z * ng.z;
    const float dx = xq.x - xp.x, dy = xq.y - xp.y, dz = xq.z - xp.z;
    const float pd = fabsf((np.x * dx + np.y * dy) + np.z * dz);
    return ok && nd >= normal_min && pd <= bound;
}

// steps 1-4 for pixel (x, y): the taps, their tests, the fold (3b: the rescue walk) and the blend
template <bool RESCUE = false, bool MEAN = false, bool DEMOD = false>
PT_HD TemporalOut temporal_pixel(const TemporalImages& im, const TemporalK& k, int x, int y, f4 kdiv = f4{1.0f, 1.0f, 1.0f, 0.0f})
{
    const int w = im.w, h = im.h;
    const size_t i = (size_t)y * w + x;
    // the list as four slots in list order; a slot that is not in the list has b = 0 and fails the b > 0 test
    int qx[4] = {x, x, x, x}, qy[4] = {y, y, y, y};
    float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    [[maybe_unused]] int cx = x, cy = y; // RESCUE: the centre of the 3 x 3, and whether step 1's list has any entry
    [[maybe_unused]] bool listed = true;
    if (!im.vel) b[0] = 1.0f;
    else
    {
        const f2 v = im.vel[i];
        const float cu = ((float)x + 0.5f) / (float)w, cv = ((float)y + 0.5f) / (float)h;
        const float pu = cu - v.x, pv = cv - v.y;
        const float fx = pu * (float)w - 0.5f, fy = pv * (float)h - 0.5f;
        if (fx >= -1.0f && fx < (float)w && fy >= -1.0f && fy < (float)h) // in float: a NaN or infinite velocity fails here
        {
            const float bx = floorf(fx), by = floorf(fy);
            const float tx = fx - bx, ty = fy - by;
            const int x0 = (int)bx, y0 = (int)by; // -1 .. w - 1, -1 .. h - 1
            for (int j = 0; j < 2; ++j)
                for (int ii = 0; ii < 2; ++ii)
                {
                    qx[2 * j + ii] = x0 + ii;
                    qy[2 * j + ii] = y0 + j;
                    b[2 * j + ii] = (ii ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                }
            if (RESCUE)
            {
                cx = x0 + (tx >= 0.5f ? 1 : 0);
                cy = y0 + (ty >= 0.5f ? 1 : 0);
            }
        }
        else listed = false;
    }
    const uint32_t mp = im.model[i];
    const bool hit = mp != MISS_ID;
    size_t q[4];
    bool ok[4];
    f4 hq[4], gq[4];
    for (int t = 0; t < 4; ++t)
    {
        const bool inside = qx[t] >= 0 && qx[t] < w && qy[t] >= 0 && qy[t] < h;
        q[t] = inside ? (size_t)qy[t] * w + qx[t] : i; // an outside tap reads p's record and is not valid
        ok[t] = inside && b[t] > 0.0f;
        hq[t] = im.hist[q[t]];
        gq[t] = im.gq[q[t]];
    }
    for (int t = 0; t < 4; ++t) ok[t] = ok[t] && hq[t].w > 0.0f && bits(gq[t].w) == mp;
    if (hit)
    {
        const f4 np = im.nprev[i], xp = im.xprev[i];
        const float bound = k.plane_max * im.pos[i].w;
        f4 xq[4];
        for (int t = 0; t < 4; ++t) xq[t] = ok[t] ? im.xq[q[t]] : f4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = 0; t < 4; ++t) ok[t] = tap_geometry_ok(ok[t], np, xp, gq[t], xq[t], k.normal_min, bound);
    }
    f2 mq[4];
    for (int t = 0; t < 4; ++t) mq[t] = ok[t] ? im.mom[q[t]] : f2{0.0f, 0.0f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, nmin = INFINITY;
    [[maybe_unused]] float sn = 0.0f;
    for (int t = 0; t < 4; ++t)
    {
        if (!ok[t]) continue;
        sw = sw + b[t];
        sr = sr + b[t] * hq[t].x;
        sg = sg + b[t] * hq[t].y;
        sb = sb + b[t] * hq[t].z;
        s1 = s1 + b[t] * mq[t].x;
        s2 = s2 + b[t] * mq[t].y;
        nmin = nmin < hq[t].w ? nmin : hq[t].w;
        if (MEAN) sn = sn + b[t] * hq[t].w;
    }
    if (RESCUE)
    {
        // step 3b, a row of the 3 x 3 at a time under the loads' discipline above; every tap has b = 1, and 1 * v is v
        if (listed && sw == 0.0f)
        {
            const f4 np = hit ? im.nprev[i] : f4{0.0f, 0.0f, 0.0f, 0.0f}, xp = hit ? im.xprev[i] : f4{0.0f, 0.0f, 0.0f, 0.0f};
            const float bound = hit ? k.plane_max * im.pos[i].w : 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
            {
                size_t rq[3];
                bool rok[3];
                f4 rh[3], rg[3];
                for (int t = 0; t < 3; ++t)
                {
                    const int rx = cx + (t - 1), ry = cy + dy;
                    const bool inside = rx >= 0 && rx < w && ry >= 0 && ry < h;
                    rq[t] = inside ? (size_t)ry * w + rx : i;
                    rh[t] = im.hist[rq[t]];
                    rg[t] = im.gq[rq[t]];
                    rok[t] = inside;
                }
                for (int t = 0; t < 3; ++t) rok[t] = rok[t] && rh[t].w > 0.0f && bits(rg[t].w) == mp;
                if (hit)
                {
                    f4 rx4[3];
                    for (int t = 0; t < 3; ++t) rx4[t] = rok[t] ? im.xq[rq[t]] : f4{0.0f, 0.0f, 0.0f, 0.0f};
                    for (int t = 0; t < 3; ++t) rok[t] = tap_geometry_ok(rok[t], np, xp, rg[t], rx4[t], k.normal_min, bound);
                }
                f2 rm[3];
                for (int t = 0; t < 3; ++t) rm[t] = rok[t] ? im.mom[rq[t]] : f2{0.0f, 0.0f};
                for (int t = 0; t < 3; ++t)
                {
                    if (!rok[t]) continue;
                    sw = sw + 1.0f;
                    sr = sr + rh[t].x;
                    sg = sg + rh[t].y;
                    sb = sb + rh[t].z;
                    s1 = s1 + rm[t].x;
                    s2 = s2 + rm[t].y;
                    nmin = nmin < rh[t].w ? nmin : rh[t].w;
                    if (MEAN) sn = sn + rh[t].w;
                }
            }
        }
    }
    f4 cur = im.cur[i];
    if (DEMOD) cur = f4{cur.x / kdiv.x, cur.y / kdiv.y, cur.z / kdiv.z, cur.w};
    const float l = lum(cur);
    TemporalOut o;
    if (sw > 0.0f)
    {
        const float hr = sr / sw, hg = sg / sw, hb = sb / sw, m1 = s1 / sw, m2 = s2 / sw;
        const float n1 = (MEAN ? floorf(sn / sw + 0.5f) : nmin) + 1.0f;
        const float n = n1 < kTemporalMaxN ? n1 : kTemporalMaxN;
        const float rn = 1.0f / n;
        const float a = k.alpha > rn ? k.alpha : rn, am = k.alpha_moments > rn ? k.alpha_moments : rn;
        o.h = f4{hr * (1.0f - a) + cur.x * a, hg * (1.0f - a) + cur.y * a, hb * (1.0f - a) + cur.z * a, n};
        o.m = f2{m1 * (1.0f - am) + l * am, m2 * (1.0f - am) + (l * l) * am};
    }
    else
    {
        o.h = f4{cur.x, cur.y, cur.z, 1.0f};
        o.m = f2{l, l * l};
    }
    return o;
}

// the instantiation of the options: f(std::bool_constant<RESCUE>, std::bool_constant<MEAN>) for the runtime (rescue, mean_length)
template <class Fn>
auto with_temporal_options(bool rescue, bool mean_length, Fn&& f)
{
    if (rescue) return mean_length ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return mean_length ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// step 5 for pixel (x, y): the variance handed to the levels.  cn = this call's C | N, mom its moments.  From kTemporalMomentsN on the
// moments answer at once; only younger pixels walk pt_denoise's 7 x 7 spatial variance of C under the current guides (every pixel valid).
PT_HD float temporal_variance(int w, int h, const DenoiseK& p, float alpha, const f4* cn, const f2* mom, const f4* pos, const f4* nrm, const uint32_t* model,
                              int x, int y)
{
    const size_t i = (size_t)y * w + x;
    const f4 cp = cn[i];
    if (cp.w >= kTemporalMomentsN)
    {
        const f2 m = mom[i];
        float v = m.y - m.x * m.x;
        if (!(v > 0.0f)) v = 0.0f;
        const float rn = 1.0f / cp.w;
        return v * (alpha > rn ? alpha : rn);
    }
    return spatial_variance(ScreenAllValidRule(nrm, model, i), w, h, p, cn, pos, nrm, x, y);
}

} // namespace pt
