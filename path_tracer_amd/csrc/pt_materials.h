// MaterialTrait implementations for the shading kernels (src/tlas/tlas_bvh/blas/primitive/material.rs,
// src/utility.rs, material/onb.rs).  Each routine consumes RNG draws in the reference's program order.
#pragma once
#include "pt_types.h"

namespace pt {

#define PT_PI 3.14159265358979323846f
#define PT_TAU 6.28318530717958647692f
#define PT_FRAC_1_PI 0.318309886183790671537767526745028724f
#define PT_EPSILON 5e-04f /* utility.rs:4 */

struct BsdfSample { f3 bsdf; float pdf; };

PT_HD f3 reflect_rs(f3 i, f3 n) { return i - 2.0f * dot3(n, i) * n; }                           // utility.rs:21
PT_HD f3 refract_rs(f3 i, f3 n, float eta)                                                    // utility.rs:23-36
{
    float ndi = dot3(n, i);
    float k = 1.0f - eta * eta * (1.0f - ndi * ndi);
    if (k <= 0.0f) { float q = from_bits(0x7fc00000u); return f3{q, q, q}; }
    return eta * i - (eta * ndi + sqrtf(k)) * n;
}
PT_HD f3 cosine_vector(Stream& rng)                                                          // utility.rs:7-19
{
    float r = sqrtf(rng.f32());
    float z = sqrtf(1.0f - r * r);
    float phi = PT_TAU * rng.f32();
    float s, c;
    sincos_det(phi, &s, &c);
    return f3{c * r, s * r, z};
}
PT_HD m33 onb_ggx(f3 v)                                                                      // onb.rs:9-27
{
    if (v.z > 0.99999f) return m33{f3{1.0f, 0.0f, 0.0f}, f3{-0.0f, -1.0f, -0.0f}, f3{0.0f, 0.0f, 1.0f}};
    f3 t1 = unit3(cross3(v, f3{0.0f, 0.0f, 1.0f}));
    f3 t2 = cross3(t1, v);
    return m33{t1, t2, v};
}
PT_HD m33 transpose33(const m33& m) { return m33{f3{m.c0.x, m.c1.x, m.c2.x}, f3{m.c0.y, m.c1.y, m.c2.y}, f3{m.c0.z, m.c1.z, m.c2.z}}; }

struct MatView
{
    uint32_t kind;
    f3 colour;
    float alpha, ior;
};
PT_HD MatView load_material(const DMaterial* mats, uint32_t idx)
{
    const DMaterial& m = mats[idx];
    return MatView{m.kind, f3{m.colour[0], m.colour[1], m.colour[2]}, m.alpha, m.ior};
}
PT_HD bool mat_is_delta(uint32_t kind) { return kind == MAT_SPECULAR || kind == MAT_DIELECTRIC; }    // material.rs:151,494
PT_HD float mat_weakening(uint32_t kind, f3 wo, f3 n) { return mat_is_delta(kind) ? 1.0f : fabsf(dot3(wo, n)); } // material.rs:67-77

// ---- GGX pieces, material.rs:189-284
PT_HD float ggx_d(float a, f3 h)
{
    if (h.z <= 0.0f) return 0.0f;
    float c2 = h.z * h.z;
    float tan_sq = sqrtf(1.0f - c2) / c2; // as written, material.rs:197
    float x = (a * a) + tan_sq;
    return a * a / (PT_PI * c2 * c2 * x * x);
}
PT_HD float schlick(float v_dot_h, float f0) { return fma_rs(pow5(1.0f - v_dot_h), 1.0f - f0, f0); }  // material.rs:205
PT_HD f3 schlick_rgb(float v_dot_h, f3 f0)                                                            // material.rs:207
{
    f3 om{1.0f - f0.x, 1.0f - f0.y, 1.0f - f0.z};
    return f0 + (om * pow5(1.0f - v_dot_h));
}
PT_HD float ggx_g1(float a, f3 v, f3 h)                                                               // material.rs:210-221
{
    if (v.z * dot3(h, v) <= 0.0f) return 0.0f;
    float tan2 = inv_sq(v.z) - 1.0f;
    return 2.0f / (1.0f + sqrtf(1.0f + a * a * tan2));
}
PT_HD float ggx_g_uncorrelated(float a, f3 wi, f3 wo)                                                 // material.rs:227-244
{
    if (wi.z <= 0.0f || wo.z <= 0.0f) return 0.0f;
    float a2 = a * a;
    float x = 2.0f * wi.z * wo.z;
    float y = 1.0f - a2;
    float z = wo.z * hypot_det(a, wi.z * sqrtf(y));
    float w = wi.z * hypot_det(a, wo.z * sqrtf(y));
    return x / (z + w);
}
PT_HD f3 ggx_half_vector(float a, Stream& rng, f3 incoming, f3 normal)                                // material.rs:248-284
{
    m33 onb_a = onb_from_normal(normal);
    f3 v_ = mul(transpose33(onb_a), -incoming);
    f3 v = unit3(v_ * f3{a, a, 1.0f});
    m33 onb_b = onb_ggx(v);
    float u1 = rng.f32();
    float u2 = rng.f32();
    float a_ = 1.0f / (1.0f + v.z);
    bool cond = u2 < a_;
    float r = min_num(sqrtf(u1), 0.9999f);
    float phi = cond ? (PT_PI * u2 / a_) : (PT_PI + ((u2 - a_) / (1.0f - a_)) * PT_PI);
    float sn, cs;
    sincos_det(phi, &sn, &cs);
    float p1 = r * cs;
    float p2 = r * sn * (cond ? 1.0f : v.z);
    f3 h_ = mul(onb_b, f3{p1, p2, sqrtf(1.0f - p1 * p1 - p2 * p2)});
    return mul(onb_a, unit3(h_ * f3{a, a, 1.0f}));
}
PT_HD float dielectric_fresnel(float cosine, float eta)                                               // material.rs:477-489
{
    if (eta * eta * (1.0f - cosine * cosine) > 1.0f) return 1.0f;
    float f0 = sq((eta - 1.0f) / (eta + 1.0f));
    return fma_rs(pow5(1.0f - cosine), 1.0f - f0, f0);
}

// ---- participating media, material/volume.rs
// VolumeScatter::scatter_direction (Henyey-Greenstein)  volume.rs:32-60
PT_HD f3 hg_direction(float g, Stream& rng, f3 incoming)
{
    float u0 = rng.f32();
    float u1 = rng.f32();
    float phi = 2.0f * PT_PI * u0;
    float z;
    if (g == 0.0f) z = 1.0f - 2.0f * u1;
    else
    {
        float x = (1.0f - g * g) / (1.0f + g * (1.0f - 2.0f * u1));
        z = (1.0f + g * g - x * x) / (2.0f * g);
    }
    float sn, cs;
    sincos_det(phi, &sn, &cs);
    float r = sqrtf(1.0f - z * z);
    return mul(onb_from_normal(-incoming), f3{r * cs, r * sn, z});
}
// VolumeAbsorption::get_transmission  volume.rs:113
PT_HD f3 beer_lambert(f3 absorption, float dist)
{
    f3 e = (-absorption) * dist;
    return f3{exp_det(e.x), exp_det(e.y), exp_det(e.z)};
}
// Equirect lookup of the environment on a miss  integrator.rs:256-262, image_helper.rs:61-88
struct EnvView { const f4* data; uint32_t w, h, pad0, pad1; };
PT_HD uint32_t sat_u32(float f) { return !(f > 0.0f) ? 0u : (f >= 4294967296.0f ? 0xffffffffu : (uint32_t)f); } // Rust `as u32`
// get_pixel_bilinear(u, v) of a w x h image (image_helper.rs:61-88): the one lookup the environment and the textures share.  Its two halves:
// the four texels with the fractions, and their blend
struct BilinearTap { f3 a, b, c, e; float xf, yf; };
PT_HD BilinearTap bilinear_fetch(const f4* data, uint32_t w, uint32_t h, float u, float v)
{
    float x = (float)w * u, y = (float)h * v;
    uint32_t x0 = sat_u32(x), y0 = sat_u32(y);
    float xf = x - truncf(x), yf = y - truncf(y);
    const uint32_t xa = x0 % w, xb = (x0 + 1u) % w, ya = y0 % h, yb = (y0 + 1u) % h;
    const f4 c00 = data[(size_t)ya * w + xa], c01 = data[(size_t)yb * w + xa];
    const f4 c10 = data[(size_t)ya * w + xb], c11 = data[(size_t)yb * w + xb];
    return BilinearTap{f3{c00.x, c00.y, c00.z}, f3{c01.x, c01.y, c01.z}, f3{c10.x, c10.y, c10.z}, f3{c11.x, c11.y, c11.z}, xf, yf};
}
PT_HD f3 bilinear_blend(const BilinearTap& t)
{
    return (((1.0f - t.xf) * (1.0f - t.yf)) * t.a + ((1.0f - t.xf) * t.yf) * t.b + (t.xf * (1.0f - t.yf)) * t.c) + (t.xf * t.yf) * t.e;
}
PT_HD f3 bilinear_rgb(const f4* data, uint32_t w, uint32_t h, float u, float v) { return bilinear_blend(bilinear_fetch(data, w, h, u, v)); }
PT_HD f3 env_lookup(const EnvView& env, f3 d)
{
    float u = fma_rs(atan2_det(d.x, d.z), PT_FRAC_1_PI * 0.5f, 0.5f);
    float v = fma_rs(asin_det(d.y), -PT_FRAC_1_PI, 0.5f);
    return bilinear_rgb(env.data, env.w, env.h, u, v);
}

// Surface colour of a hit (the definition is include/pt_api.h's): `colour` of the hit's material, times the bilinear texel at the hit's
// interpolated, repeat-addressed UV when the material references a texture (`texture` = DMaterial::texture, index + 1).  tri: leaf order.
// Every operation rounded once, in the order written (the library is built without contraction).
PT_HD f3 surface_colour(const TexView& tv, uint32_t texture, f3 colour, uint32_t tri, float u, float v)
{
    if (texture == 0u) return colour;
    const DTriUV uv = tv.tri_uv[tri];
    const DTexture t = tv.table[texture - 1u];
    float s = (uv.a[0] + u * (uv.b[0] - uv.a[0])) + v * (uv.c[0] - uv.a[0]);
    float w = (uv.a[1] + u * (uv.b[1] - uv.a[1])) + v * (uv.c[1] - uv.a[1]);
    s = s - floorf(s);
    w = w - floorf(w);
    return colour * bilinear_rgb(tv.texels + t.offset, t.w, t.h, s, w);
}

// The lightmap lookup (pt_set_lightmap; the definition is include/pt_api.h's): the w x h map `texels` at the hit's interpolated UV, which is
// surface_colour's s, t WITHOUT the repeat addressing.  Texel (i, j) has its centre at ((i + .5) / w, (j + .5) / h), the bake's p (lm_centre,
// pt_lightmap.h), so the texel coordinate is w * s - 0.5, clamped to the edge (a NaN gives 0: no index leaves the map whatever the UVs are);
// the blend is bilinear_blend's.  uv: the triangle's UVs at load-order vertices 0, 1, 2.  Every operation rounded once, in the order written.
// Shared by the baked view's kernel, the unit hook's kernel and the hook's host evaluation.
PT_HD f3 lightmap_lookup(const f4* texels, uint32_t w, uint32_t h, const DTriUV& uv, float u, float v)
{
    const float s = (uv.a[0] + u * (uv.b[0] - uv.a[0])) + v * (uv.c[0] - uv.a[0]);
    const float t = (uv.a[1] + u * (uv.b[1] - uv.a[1])) + v * (uv.c[1] - uv.a[1]);
    float x = (float)w * s - 0.5f, y = (float)h * t - 0.5f;
    const float xm = (float)(w - 1u), ym = (float)(h - 1u);
    x = !(x > 0.0f) ? 0.0f : (x > xm ? xm : x);
    y = !(y > 0.0f) ? 0.0f : (y > ym ? ym : y);
    const uint32_t x0 = (uint32_t)x, y0 = (uint32_t)y;
    const float xf = x - truncf(x), yf = y - truncf(y);
    const uint32_t x1 = x0 + 1u < w ? x0 + 1u : x0, y1 = y0 + 1u < h ? y0 + 1u : y0;
    const f4 c00 = texels[(size_t)y0 * w + x0], c01 = texels[(size_t)y1 * w + x0];
    const f4 c10 = texels[(size_t)y0 * w + x1], c11 = texels[(size_t)y1 * w + x1];
    return bilinear_blend(BilinearTap{f3{c00.x, c00.y, c00.z}, f3{c01.x, c01.y, c01.z}, f3{c10.x, c10.y, c10.z}, f3{c11.x, c11.y, c11.z}, xf, yf});
}
// ... of a hit on world-TLAS leaf `inst`, leaf-order triangle `tri`; *mapped <- the leaf has a map (else the result is 0)
PT_HD f3 lightmap_at(const LmView& lm, uint32_t inst, uint32_t tri, float u, float v, bool* mapped)
{
    const DLightmap r = lm.leaf[inst];
    *mapped = r.w != 0u;
    if (!*mapped) return f3{0.0f, 0.0f, 0.0f};
    return lightmap_lookup(lm.texels + r.offset, r.w, r.h, lm.tri_uv[tri + r.uv_add], u, v);
}

// The normal map's lookup: bilinear_rgb, except that four EQUAL texels (rgb) are that texel, with no arithmetic.  The four bilinear weights do
// not always sum to exactly 1 in binary32, so a constant region of a map would otherwise come back an ulp off at some UVs, and a flat map
// would not be the plain normal bit for bit there.
PT_HD f3 bilinear_rgb_const(const f4* data, uint32_t w, uint32_t h, float u, float v)
{
    const BilinearTap t = bilinear_fetch(data, w, h, u, v);
    const f3 a = t.a, b = t.b, c = t.c, e = t.e;
    if (a.x == b.x && a.x == c.x && a.x == e.x && a.y == b.y && a.y == c.y && a.y == e.y && a.z == b.z && a.z == c.z && a.z == e.z) return a;
    return bilinear_blend(t);
}

// Roughness maps (pt_set_material_roughness_texture; the definition is include/pt_api.h's): the GGX alpha of a hit.  `roughness_texture` =
// DMaterial::roughness_texture (index + 1), `alpha` = DMaterial::alpha, returned with no arithmetic without a map; tri: leaf order.  With a
// map: the first component of the bilinear texel (the normal map's lookup: a constant region is its texel) at surface_colour's s, t is the
// linear roughness, squared and clamped as HostScene::add_material does (material.rs:294,309), so a constant map of rho is the material of
// roughness rho bit for bit.  Shared by the GGX surface pass, the baked view's SPEC ending, the unit hook's kernel and its host evaluation.
PT_HD float surface_alpha(const TexView& tv, uint32_t roughness_texture, float alpha, uint32_t tri, float u, float v)
{
    if (roughness_texture == 0u) return alpha;
    const DTriUV uv = tv.tri_uv[tri];
    const DTexture t = tv.table[roughness_texture - 1u];
    float s = (uv.a[0] + u * (uv.b[0] - uv.a[0])) + v * (uv.c[0] - uv.a[0]);   // surface_colour's s, t
    float w = (uv.a[1] + u * (uv.b[1] - uv.a[1])) + v * (uv.c[1] - uv.a[1]);
    s = s - floorf(s);
    w = w - floorf(w);
    const float rho = bilinear_rgb_const(tv.texels + t.offset, t.w, t.h, s, w).x;
    return clamp_rs(sq(rho), 0.0001f, 0.9999f);
}
// ... of a hit on world-TLAS leaf `inst` (pt_surface_roughness): 0 on a kind that is not GGX
PT_HD float surface_roughness_at(const DInstance* instances, const DMaterial* materials, const TexView& tex, uint32_t inst, uint32_t tri, float u, float v)
{
    const DMaterial& dm = materials[instances[inst].material];
    if (dm.kind != MAT_GGX_METAL && dm.kind != MAT_GGX_DIELECTRIC) return 0.0f;
    return surface_alpha(tex, dm.roughness_texture, dm.alpha, tri, u, v);
}

// Normal maps (pt_set_material_normal_texture; the definition is include/pt_api.h's).  n: the object-space unit3(interpolated vertex normals)
// of the hit, before face-forwarding; `normal_texture` = DMaterial::normal_texture (index + 1); tri: leaf order.  Returns the object-space
// N': n itself, bit for bit, without a normal texture, at a flat texel (x == 0 and y == 0) and on a triangle without a tangent (T == 0).
// Every operation rounded once, in the order written.
PT_HD f3 perturbed_normal(const TexNView& tv, uint32_t normal_texture, f3 n, uint32_t tri, float u, float v)
{
    if (normal_texture == 0u) return n;
    const DTriUV uv = tv.tri_uv[tri];
    const DTexture t = tv.table[normal_texture - 1u];
    float s = (uv.a[0] + u * (uv.b[0] - uv.a[0])) + v * (uv.c[0] - uv.a[0]);   // surface_colour's s, t
    float w = (uv.a[1] + u * (uv.b[1] - uv.a[1])) + v * (uv.c[1] - uv.a[1]);
    s = s - floorf(s);
    w = w - floorf(w);
    const f3 c = bilinear_rgb_const(tv.texels + t.offset, t.w, t.h, s, w);
    const float x = 2.0f * c.x - 1.0f, y = 2.0f * c.y - 1.0f, z = 2.0f * c.z - 1.0f;
    if (x == 0.0f && y == 0.0f) return n;
    const f4 tan = tv.tri_tan[tri];
    const f3 tg{tan.x, tan.y, tan.z};
    if (tg.x == 0.0f && tg.y == 0.0f && tg.z == 0.0f) return n;                // degenerate UVs, or a model without UVs
    const f3 tp = unit3(tg - n * dot3(n, tg));                                 // Gram-Schmidt at the hit
    const f3 bp = cross3(n, tp) * tan.w;                                       // tan.w = +1 / -1, handedness of (T, B, geometric normal)
    return unit3((tp * x + bp * y) + n * z);
}
// The shading normal of a hit in world space: hit_normal (pt_kernels.hip: Triangle::get_normal, face-forward in object space, the deferred
// instance transform) with N' = perturbed_normal in place of N.  `front` is the flag of the UNPERTURBED N; a back-face hit flips N'.  Shared by
// the normal-map variants of the surface passes, the unit hook's kernel and the hook's host evaluation.
PT_HD f3 shading_normal(const DTriVerts* tri_shade, const DInstance* instances, const DMaterial* materials, const TexNView& tv, uint32_t inst,
                        uint32_t tri, float u, float v, f3 dir_world, bool& front)
{
    const DTriVerts tv3 = tri_shade[tri];
    const float wgt = 1.0f - u - v;
    const m33 nm{f3{tv3.a.x, tv3.a.y, tv3.a.z}, f3{tv3.b.x, tv3.b.y, tv3.b.z}, f3{tv3.c.x, tv3.c.y, tv3.c.z}};
    const f3 n = unit3(mul(nm, f3{wgt, u, v}));
    const DInstance& in = instances[inst];
    const f3 d_obj{(in.inv[0] * dir_world.x + in.inv[1] * dir_world.y) + in.inv[2] * dir_world.z,
                   (in.inv[4] * dir_world.x + in.inv[5] * dir_world.y) + in.inv[6] * dir_world.z,
                   (in.inv[8] * dir_world.x + in.inv[9] * dir_world.y) + in.inv[10] * dir_world.z};
    front = dot3(d_obj, n) < 0.0f;
    f3 m = perturbed_normal(tv, materials[in.material].normal_texture, n, tri, u, v);
    if (!front) m = -m;
    return f3{(in.fwd[0] * m.x + in.fwd[1] * m.y) + in.fwd[2] * m.z, (in.fwd[4] * m.x + in.fwd[5] * m.y) + in.fwd[6] * m.z,
              (in.fwd[8] * m.x + in.fwd[9] * m.y) + in.fwd[10] * m.z};
}

// The directional lightmap lookup (pt_set_lightmap_directional; the definition is include/pt_api.h's): lightmap_lookup's s, t, clamp and
// bilinear weights on the map's texel M0 and on its three gradient texels G_x, G_y, G_z (grad: three f4 per texel), each blended with
// bilinear_blend's expression, one after the other so that one blend's texels are live at a time; then, with delta = n' - n,
//     I = max(0, (M0 - (0.5 * (delta . delta)) * M0) + ((G_x * delta.x + G_y * delta.y) + G_z * delta.z))        per channel
// the max written so that a NaN gives 0.  delta = 0 returns lightmap_lookup's bits: M0 - 0 * M0 and + (+-0) change nothing of a finite M0 >= 0.
// Shared by the baked view's DIR kernels, the unit hook's kernel and the hook's host evaluation.
// (The addressing lines are lightmap_lookup's, and unperturbed_normal below is shading_normal's first half, restated and not factored out
// of them on purpose: lightmap_lookup, shading_normal and every kernel over them stay instruction for instruction what they were.)
PT_HD f3 lightmap_lookup_directional(const f4* texels, const f4* grad, uint32_t w, uint32_t h, const DTriUV& uv, float u, float v, f3 delta)
{
    const float s = (uv.a[0] + u * (uv.b[0] - uv.a[0])) + v * (uv.c[0] - uv.a[0]);
    const float t = (uv.a[1] + u * (uv.b[1] - uv.a[1])) + v * (uv.c[1] - uv.a[1]);
    float x = (float)w * s - 0.5f, y = (float)h * t - 0.5f;
    const float xm = (float)(w - 1u), ym = (float)(h - 1u);
    x = !(x > 0.0f) ? 0.0f : (x > xm ? xm : x);
    y = !(y > 0.0f) ? 0.0f : (y > ym ? ym : y);
    const uint32_t x0 = (uint32_t)x, y0 = (uint32_t)y;
    const float xf = x - truncf(x), yf = y - truncf(y);
    const uint32_t x1 = x0 + 1u < w ? x0 + 1u : x0, y1 = y0 + 1u < h ? y0 + 1u : y0;
    const size_t i00 = (size_t)y0 * w + x0, i01 = (size_t)y1 * w + x0, i10 = (size_t)y0 * w + x1, i11 = (size_t)y1 * w + x1;
    f3 out;
    {
        const f4 c00 = texels[i00], c01 = texels[i01], c10 = texels[i10], c11 = texels[i11];
        const f3 m0 = bilinear_blend(BilinearTap{f3{c00.x, c00.y, c00.z}, f3{c01.x, c01.y, c01.z}, f3{c10.x, c10.y, c10.z}, f3{c11.x, c11.y, c11.z}, xf, yf});
        out = m0 - (0.5f * dot3(delta, delta)) * m0;
    }
    f3 g[3];
#pragma unroll
    for (uint32_t a = 0; a < 3u; ++a)
    {
        const f4 c00 = grad[3u * i00 + a], c01 = grad[3u * i01 + a], c10 = grad[3u * i10 + a], c11 = grad[3u * i11 + a];
        g[a] = bilinear_blend(BilinearTap{f3{c00.x, c00.y, c00.z}, f3{c01.x, c01.y, c01.z}, f3{c10.x, c10.y, c10.z}, f3{c11.x, c11.y, c11.z}, xf, yf});
    }
    out = out + ((g[0] * delta.x + g[1] * delta.y) + g[2] * delta.z);
    return f3{!(out.x > 0.0f) ? 0.0f : out.x, !(out.y > 0.0f) ? 0.0f : out.y, !(out.z > 0.0f) ? 0.0f : out.z};
}
// The face-forwarded world normal of the UNPERTURBED N of a hit: hit_normal's arithmetic (pt_kernels.hip), stated here for the host; it is
// shading_normal's result on a material without a normal texture, bit for bit.
PT_HD f3 unperturbed_normal(const DTriVerts* tri_shade, const DInstance* instances, uint32_t inst, uint32_t tri, float u, float v, f3 dir_world, bool& front)
{
    const DTriVerts tv3 = tri_shade[tri];
    const float wgt = 1.0f - u - v;
    const m33 nm{f3{tv3.a.x, tv3.a.y, tv3.a.z}, f3{tv3.b.x, tv3.b.y, tv3.b.z}, f3{tv3.c.x, tv3.c.y, tv3.c.z}};
    f3 n = unit3(mul(nm, f3{wgt, u, v}));
    const DInstance& in = instances[inst];
    const f3 d_obj{(in.inv[0] * dir_world.x + in.inv[1] * dir_world.y) + in.inv[2] * dir_world.z,
                   (in.inv[4] * dir_world.x + in.inv[5] * dir_world.y) + in.inv[6] * dir_world.z,
                   (in.inv[8] * dir_world.x + in.inv[9] * dir_world.y) + in.inv[10] * dir_world.z};
    front = dot3(d_obj, n) < 0.0f;
    if (!front) n = -n;
    return f3{(in.fwd[0] * n.x + in.fwd[1] * n.y) + in.fwd[2] * n.z, (in.fwd[4] * n.x + in.fwd[5] * n.y) + in.fwd[6] * n.z,
              (in.fwd[8] * n.x + in.fwd[9] * n.y) + in.fwd[10] * n.z};
}
// n' of a hit whose unperturbed world normal is n (ChainEnd::nrm): shading_normal's result; n itself, with no arithmetic, where the hit's
// material has no normal texture, so that delta = n' - n is zero there by construction and not by subtraction.  *delta <- n' - n.
PT_HD f3 shading_normal_delta(const DTriVerts* tri_shade, const DInstance* instances, const DMaterial* materials, const TexNView& tv, uint32_t inst,
                              uint32_t tri, float u, float v, f3 dir_world, f3 n, f3* delta)
{
    *delta = f3{0.0f, 0.0f, 0.0f};
    if (materials[instances[inst].material].normal_texture == 0u) return n;
    bool front;
    const f3 np = shading_normal(tri_shade, instances, materials, tv, inst, tri, u, v, dir_world, front);
    *delta = np - n;
    return np;
}
// ... of a hit on world-TLAS leaf `inst`: lightmap_at where the leaf's map has no gradient (or there is no gradient at all)
PT_HD f3 lightmap_at_directional(const LmView& lm, const LmDirView& ld, uint32_t inst, uint32_t tri, float u, float v, f3 delta, bool* mapped)
{
    const DLightmap r = lm.leaf[inst];
    *mapped = r.w != 0u;
    if (!*mapped) return f3{0.0f, 0.0f, 0.0f};
    if (!ld.grad || !ld.leaf_dir[inst]) return lightmap_lookup(lm.texels + r.offset, r.w, r.h, lm.tri_uv[tri + r.uv_add], u, v);
    return lightmap_lookup_directional(lm.texels + r.offset, ld.grad + 3u * (size_t)r.offset, r.w, r.h, lm.tri_uv[tri + r.uv_add], u, v, delta);
}

// MaterialTrait::scatter_direction
PT_HD f3 mat_scatter(const MatView& m, Stream& rng, f3 incoming, f3 normal, bool front)
{
    switch (m.kind)
    {
    case MAT_LAMBERTIAN: return mul(onb_from_normal(normal), cosine_vector(rng));                     // material.rs:104-107
    case MAT_SPECULAR: return reflect_rs(incoming, normal);                                           // material.rs:153
    case MAT_GGX_METAL: { f3 h = ggx_half_vector(m.alpha, rng, incoming, normal); return reflect_rs(incoming, h); } // material.rs:325
    case MAT_GGX_DIELECTRIC:                                                                          // material.rs:326-346
    {
        f3 h = ggx_half_vector(m.alpha, rng, incoming, normal);
        float eta = front ? (1.0f / m.ior) : m.ior;
        float f0 = sq((eta - 1.0f) / (eta + 1.0f));
        float f = schlick(-dot3(incoming, h), f0);
        f3 refracted = refract_rs(incoming, h, eta);
        bool reflected = anynan3(refracted);
        if (!reflected) reflected = rng.f32() < f; // the draw happens only when refraction is possible, material.rs:335
        return reflected ? reflect_rs(incoming, h) : refracted;
    }
    case MAT_DIELECTRIC:                                                                              // material.rs:496-509
    {
        float eta = front ? (1.0f / m.ior) : m.ior;
        float cosine = -dot3(incoming, normal);
        if (rng.f32() < dielectric_fresnel(cosine, eta)) return reflect_rs(incoming, normal);
        return refract_rs(incoming, normal, eta);
    }
    default: return f3{0.0f, 0.0f, 0.0f};                                                             // Emissive, material.rs:133
    }
}

// pt_render_guides_followed: where the guide chain goes on from a hit (include/pt_api.h).  A mirror reflects; glass refracts, without the
// Fresnel coin (no draw), and reflects only where refraction is impossible; every other kind ends the chain.  Shared by k_guide_follow,
// the unit hook's kernel and the hook's host evaluation.
struct FollowDir { f3 wo; bool followed; };
PT_HD FollowDir guide_follow_dir(uint32_t kind, float ior, f3 incoming, f3 normal, bool front)
{
    if (kind == MAT_SPECULAR) return FollowDir{reflect_rs(incoming, normal), true};
    if (kind == MAT_DIELECTRIC)
    {
        const float eta = front ? (1.0f / ior) : ior;
        const f3 refracted = refract_rs(incoming, normal, eta);
        return FollowDir{anynan3(refracted) ? reflect_rs(incoming, normal) : refracted, true};
    }
    return FollowDir{f3{0.0f, 0.0f, 0.0f}, false};
}

// MaterialTrait::get_bsdf_pdf(incoming, outgoing, hit)
PT_HD BsdfSample mat_bsdf_pdf(const MatView& m, f3 incoming, f3 outgoing, f3 normal, bool front)
{
    switch (m.kind)
    {
    case MAT_LAMBERTIAN:                                                                              // material.rs:109-115
    {
        float cosine = dot3(outgoing, normal);
        return BsdfSample{m.colour * PT_FRAC_1_PI, cosine * PT_FRAC_1_PI};
    }
    case MAT_EMISSIVE:
    case MAT_SPECULAR: return BsdfSample{m.colour, 1.0f};                                             // material.rs:134,155
    case MAT_DIELECTRIC:                                                                              // material.rs:511-527
    {
        float cosine = -dot3(incoming, outgoing);
        float eta = front ? (1.0f / m.ior) : m.ior;
        float f = dielectric_fresnel(cosine, eta);
        if (dot3(outgoing, normal) > 0.0f) return BsdfSample{bc3(f), f};
        float b = (1.0f - f) / (eta * eta);
        return BsdfSample{m.colour * b, 1.0f - f};
    }
    default:                                                                                          // GGX, material.rs:349-450
    {
        const bool transmissive = m.kind == MAT_GGX_DIELECTRIC;
        const float a = m.alpha;
        m33 onb_inv = transpose33(onb_from_normal(normal));
        f3 wi = mul(onb_inv, outgoing);
        f3 wo = mul(onb_inv, incoming);
        bool transmitted = wi.z < 0.0f;
        float eta = front ? m.ior : (1.0f / m.ior);
        f3 h;
        if (transmissive && transmitted) { f3 h_ = unit3(eta * wi + wo); h = h_ * signum_rs(h_.z); }
        else { h = unit3(wi + wo); }
        float i_dot_h = dot3(wi, h), o_dot_h = dot3(wo, h);
        float d = ggx_d(a, h);
        float f, g;
        if (!transmissive) { f = 1.0f; g = ggx_g_uncorrelated(a, wi, wo); }
        else
        {
            float f0 = sq((eta - 1.0f) / (eta + 1.0f));
            f = schlick(fabsf(i_dot_h), f0);
            g = ggx_g1(a, wi, h) * ggx_g1(a, wo, h);                                                   // material.rs:224
        }
        if (transmitted)
        {
            if (!transmissive) return BsdfSample{f3{0.0f, 0.0f, 0.0f}, 0.0f};                          // BsdfPdf::invalid()
            float x = fabsf(i_dot_h * o_dot_h);
            float y = fabsf(wi.z * wo.z);
            float z = (1.0f - f) * g * d;
            float w = (eta * i_dot_h) + o_dot_h;
            float btdf = (x * z) / (y * w * w);
            float jac = fabsf(o_dot_h) / (w * w);
            float pdf = d * (1.0f - f) * fabsf(h.z) * jac;
            return BsdfSample{m.colour * btdf * eta * eta, pdf};
        }
        float brdf = f * g * d / (4.0f * fabsf(wi.z * wo.z));
        float jac = 1.0f / (4.0f * fabsf(o_dot_h));
        float pdf = d * h.z * f * jac;
        f3 tint = transmissive ? f3{1.0f, 1.0f, 1.0f} : schlick_rgb(fabsf(i_dot_h), m.colour);
        return BsdfSample{brdf * tint, pdf};
    }
    }
}

} // namespace pt
