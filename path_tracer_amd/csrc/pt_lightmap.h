// Lightmap texels: which triangle of a model's UV layout covers a texel centre, the surface point and normal there under one instance
// matrix, the cosine-distributed sample directions over it and one dilation step.  One definition for the gfx950 kernels (pt_lightmap.hip)
// and for the host evaluations (pt_lightmap_texels with on_device = 0, pt_lightmap_ray).  include/pt_api.h, pt_bake_lightmap, states it
// operation for operation; every operation is rounded once, in this order (the library is built without contraction).
#pragma once
#include <vector>

#include "pt_materials.h"
#include "pt_types.h"

namespace pt {

// E(p, q, r) of the coverage rule: twice the signed area of (p, q, r), binary64
PT_HD double lm_edge(double ps, double pt_, double qs, double qt, double rs, double rt) { return (qs - ps) * (rt - pt_) - (qt - pt_) * (rs - ps); }

// centre of texel column i of a map w wide (rows alike)
PT_HD double lm_centre(uint32_t i, uint32_t w) { return ((double)i + 0.5) / (double)w; }

// does the UV triangle uv (a.s a.t b.s b.t c.s c.t) contain p?  u, v: its barycentrics of p (valid when A != 0)
PT_HD bool lm_contains(const float uv[6], double ps, double pt_, double* u, double* v)
{
    const double as = (double)uv[0], at = (double)uv[1], bs = (double)uv[2], bt = (double)uv[3], cs = (double)uv[4], ct = (double)uv[5];
    const double A = lm_edge(as, at, bs, bt, cs, ct);
    if (A == 0.0) return false;
    *u = lm_edge(as, at, ps, pt_, cs, ct) / A;
    *v = lm_edge(as, at, bs, bt, ps, pt_) / A;
    return *u >= 0.0 && *v >= 0.0 && *u + *v <= 1.0;
}

// The texel rectangle a triangle's centres are looked for in: columns floor(min s * w) - 1 .. floor(max s * w) + 1 and the rows alike, clamped
// to the map; false when it is empty.  floor(x * w) is the column x lies in, so the rectangle holds every centre of the UV bounding box and a
// ring of one texel around it.
struct LmBox { uint32_t i0, j0, bw, bh; };
PT_HD bool lm_span(double lo, double hi, uint32_t n, uint32_t* first, uint32_t* count)
{
    double a = __builtin_floor(lo * (double)n) - 1.0, b = __builtin_floor(hi * (double)n) + 1.0;
    if (!(b >= 0.0) || !(a <= (double)(n - 1u))) return false;
    if (a < 0.0) a = 0.0;
    if (b > (double)(n - 1u)) b = (double)(n - 1u);
    *first = (uint32_t)a;
    *count = (uint32_t)b - (uint32_t)a + 1u;
    return true;
}
PT_HD bool lm_box(const float uv[6], uint32_t w, uint32_t h, LmBox* box)
{
    const double s0 = (double)min_sse(min_sse(uv[0], uv[2]), uv[4]), s1 = (double)max_sse(max_sse(uv[0], uv[2]), uv[4]);
    const double t0 = (double)min_sse(min_sse(uv[1], uv[3]), uv[5]), t1 = (double)max_sse(max_sse(uv[1], uv[3]), uv[5]);
    return lm_span(s0, s1, w, &box->i0, &box->bw) && lm_span(t0, t1, h, &box->j0, &box->bh);
}

// surface point and normal of barycentrics (u, v) on the triangle with load-order positions p9 and normals n9 (a b c, xyz each), under
// the instance's forward matrix m
PT_HD void lm_surface(const float p9[9], const float n9[9], const xf34& m, float u, float v, f3* P, f3* n)
{
    const f3 pa{p9[0], p9[1], p9[2]}, pb{p9[3], p9[4], p9[5]}, pc{p9[6], p9[7], p9[8]};
    const f3 na{n9[0], n9[1], n9[2]}, nb{n9[3], n9[4], n9[5]}, nc{n9[6], n9[7], n9[8]};
    const f3 p_obj = (pa + u * (pb - pa)) + v * (pc - pa);
    const float wgt = 1.0f - u - v;
    const f3 n_obj = unit3((na * wgt + nb * u) + nc * v);
    *P = xf_point(m, p_obj);
    *n = xf_vector(m, n_obj);
}

// The texel table on the host (pt_lightmap_texels with on_device = 0, pt_lightmap_denoise's host walk), over a model's load-order arrays.
// owner[k] = the lowest triangle index whose UVs contain the centre of texel k, MISS_ID where none does: the walk k_lm_cover does, triangle by
// triangle over its texel rectangle, with a running minimum in the atomic's place
inline void lm_owner_host(const float* uvs, uint32_t n_tris, uint32_t w, uint32_t h, std::vector<uint32_t>& owner)
{
    owner.assign((size_t)w * h, MISS_ID);
    for (uint32_t t = 0; t < n_tris; ++t)
    {
        const float* uv = uvs + 6u * (size_t)t;
        LmBox box;
        if (!lm_box(uv, w, h, &box)) continue;
        for (uint32_t j = box.j0; j < box.j0 + box.bh; ++j)
            for (uint32_t i = box.i0; i < box.i0 + box.bw; ++i)
            {
                double u, v;
                uint32_t& o = owner[(size_t)j * w + i];
                if (t < o && lm_contains(uv, lm_centre(i, w), lm_centre(j, h), &u, &v)) o = t;
            }
    }
}
// what k_lm_resolve writes for texel k owned by triangle t (MISS_ID: zeros)
inline void lm_resolve_host(const float* uvs, const float* positions, const float* normals, const xf34& m, uint32_t w, uint32_t h, size_t k, uint32_t t,
                            float* u32, float* v32, f3* P, f3* n)
{
    *u32 = 0.0f; *v32 = 0.0f;
    *P = f3{0.0f, 0.0f, 0.0f}; *n = f3{0.0f, 0.0f, 0.0f};
    if (t == MISS_ID) return;
    double u = 0.0, v = 0.0;
    (void)lm_contains(uvs + 6u * (size_t)t, lm_centre((uint32_t)(k % w), w), lm_centre((uint32_t)(k / w), h), &u, &v);
    *u32 = (float)u; *v32 = (float)v;
    lm_surface(positions + 9u * (size_t)t, normals + 9u * (size_t)t, m, *u32, *v32, P, n);
}

// origin of a texel's rays
PT_HD f3 lm_origin(f3 P, f3 n, float bias) { return P + bias * n; }

// direction of sample `sample` of the texel whose stream is pixel `key`, over the normal n: cosine_vector's arithmetic on the Sobol point seeded
// by the stream's draw 0 (as a camera ray's jitter, main.rs:193-194).  ONE draw of the stream is consumed.
PT_HD f3 lightmap_ray(uint64_t seed, uint32_t n_sobol, uint32_t key, uint32_t sample, f3 n)
{
    Stream rng{stream_key(seed, key, sample), 0u};
    const uint32_t seed0 = rng.u32();
    float u1, u2;
    ss_sobol(n_sobol, sample, seed0, &u1, &u2);
    const float r = sqrtf(u1);
    const float z = sqrtf(1.0f - r * r);
    const float phi = 6.2831855f * u2;
    float sn, cs;
    sincos_det(phi, &sn, &cs);
    return mul(onb_from_normal(n), f3{cs * r, sn * r, z});
}

// ---- direct light sampled at the texel (pt_bake_lightmap_direct; include/pt_api.h states it)
// what a texel's light sample reads: the light table and the per-triangle and material tables the shading pass samples lights from, over the
// device's copies (the kernel) or the host's (FlatScene: the hook's host evaluation)
struct LmLightView
{
    const DLight* lights;
    const DTriVerts* tri_pos;
    const DTriVerts* tri_shade;
    const DTriIsect* tri_isect;
    const DMaterial* materials;
    uint32_t n_lights;
    TexView tex;
};
// light: the chosen entry of the light table; (dir, t_max): the shadow ray from the texel's origin, cast only when `cast`; ce: what the
// sample adds when that ray is not blocked (zeros without a ray)
struct LmLightSample
{
    f3 dir, ce;
    float t_max;
    uint32_t light;
    bool cast;
};
PT_HD f3 lm_xyz(f4 v) { return f3{v.x, v.y, v.z}; }
// the finite check and length clamp every sample ends with (finalise, pt_kernels.hip)
PT_HD f3 lm_finalise(f3 v)
{
    if (!finite3(v)) return f3{0.0f, 0.0f, 0.0f};
    return clamp_len_max(v, 100.0f);
}
// Light sample `sample` of the texel whose light stream is pixel `key`, at origin o under normal n (used as given): k_shade_surface's
// estimate_direct_explicit for a Lambertian surface of colour 1 with the MIS weight replaced by 1, in its operation order.  THREE draws of
// the stream are consumed.  Requires n_lights > 0.
PT_HD LmLightSample lm_light_sample(const LmLightView& lv, uint64_t seed, uint32_t key, uint32_t sample, f3 o, f3 n)
{
    Stream rng{stream_key(seed, key, sample), 0u};
    const float x = rng.f32();
    uint32_t li = 0, hi = lv.n_lights;
    const int32_t xk = total_order_key(x);
    while (li < hi)
    {
        const uint32_t mid = (li + hi) >> 1;
        if (total_order_key(lv.lights[mid].cdf) < xk) li = mid + 1u; else hi = mid;
    }
    if (li >= lv.n_lights) li = lv.n_lights - 1u;
    const DLight L = lv.lights[li];
    float lu = rng.f32();
    float lv_ = rng.f32();
    if (lu + lv_ > 1.0f) { lu = 1.0f - lu; lv_ = 1.0f - lv_; }
    const float lw = 1.0f - lu - lv_;
    const DTriVerts lp = lv.tri_pos[L.tri], ln = lv.tri_shade[L.tri];
    const f3 point = mul(m33{lm_xyz(lp.a), lm_xyz(lp.b), lm_xyz(lp.c)}, f3{lw, lu, lv_});
    const f3 lnormal = unit3(mul(m33{lm_xyz(ln.a), lm_xyz(ln.b), lm_xyz(ln.c)}, f3{lw, lu, lv_}));
    const f3 d = point - o;
    const float dist2 = len_sq(d);
    const float dist = sqrtf(dist2);
    LmLightSample out;
    out.dir = unit3(d);
    out.t_max = (1.0f - PT_EPSILON) * dist;
    out.light = li;
    out.ce = f3{0.0f, 0.0f, 0.0f};
    const float c = dot3(out.dir, n);
    out.cast = c > 0.0f;
    if (!out.cast) return out;
    const DTriIsect ti = lv.tri_isect[L.tri];
    const float sample_pdf = L.pdf / (0.5f * len3(lm_xyz(ti.n0)));
    const float cosl = fabsf(dot3(out.dir, lnormal));
    const float light_pdf = sample_pdf * (dist2 / cosl);
    const DMaterial& lm = lv.materials[L.material];
    const f3 emitted = surface_colour(lv.tex, lm.texture, f3{lm.colour[0], lm.colour[1], lm.colour[2]}, L.tri, lu, lv_);
    out.ce = lm_finalise(((emitted * fabsf(c)) * 0.31830987f) / light_pdf);
    return out;
}
// one sample of a direct bake: X = G + D per channel, G the gather ray's radiance unless its first hit is on an emissive model (then the
// light sample stands for it), D the light sample unless its shadow ray was blocked
PT_HD float lm_direct_x(float radiance, bool first_hit_emissive, float ce, bool blocked)
{
    const float g = first_hit_emissive ? 0.0f : radiance;
    const float dl = blocked ? 0.0f : ce;
    return g + dl;
}

// The tangential gradient of a covered texel (pt_lightmap_gradient; include/pt_api.h states it): dir9 the texel's first-moment sums
// [axis][channel] over n_samples cosine-distributed samples, n the texel table's normal, used as given.  Per channel m = dir / n_samples,
// q = m . n, G = (8/3) * (m - q * n); grad9 in the same layout.  Shared by k_lm_gradient and the host evaluation.
PT_HD void lm_gradient(const float dir9[9], f3 n, float n_samples, float grad9[9])
{
    for (uint32_t c = 0; c < 3u; ++c)
    {
        const f3 m{dir9[c] / n_samples, dir9[3u + c] / n_samples, dir9[6u + c] / n_samples};
        const float q = (m.x * n.x + m.y * n.y) + m.z * n.z;
        grad9[c] = 2.6666667f * (m.x - q * n.x);
        grad9[3u + c] = 2.6666667f * (m.y - q * n.y);
        grad9[6u + c] = 2.6666667f * (m.z - q * n.z);
    }
}

// One dilation step of texel (i, j): false when the texel keeps its value (it is covered, or none of its eight neighbours is); otherwise the
// mean of the neighbours with a non-zero coverage byte, added dy = -1..1 outer, dx = -1..1 inner
PT_HD bool lm_dilate(const float* rgb, const uint8_t* cov, uint32_t w, uint32_t h, uint32_t i, uint32_t j, float out[3])
{
    if (cov[(size_t)j * w + i]) return false;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t count = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
        {
            const int64_t x = (int64_t)i + dx, y = (int64_t)j + dy;
            if ((dx == 0 && dy == 0) || x < 0 || y < 0 || x >= (int64_t)w || y >= (int64_t)h) continue;
            const size_t q = (size_t)y * w + (size_t)x;
            if (!cov[q]) continue;
            s0 = s0 + rgb[3 * q]; s1 = s1 + rgb[3 * q + 1]; s2 = s2 + rgb[3 * q + 2];
            ++count;
        }
    if (!count) return false;
    const float n = (float)count;
    out[0] = s0 / n; out[1] = s1 / n; out[2] = s2 / n;
    return true;
}

} // namespace pt
