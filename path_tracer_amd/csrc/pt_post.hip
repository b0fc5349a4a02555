// The step after the path: what the reference's State::update / State::render do to a finished frame
// (src/state.rs:505-586, 629-667) as gfx950 kernels working on the framebuffers that are already in HBM.
//
//   k_post_accumulate   src/shaders/accumulate.wgsl:20-23     static camera: accumulation += (rgb, 1)
//   k_post_velocity     src/shaders/velocity.wgsl:16-39       per-pixel motion vector from the first-hit position
//   k_post_motion       (no reference counterpart) where a pixel's first hit was in the previous frame, by its instance's motion
//   k_post_reproject    src/shaders/compute.wgsl:103-212      3x3 YCoCg variance clip, Catmull-Rom history, id disocclusion, 15 % blend
//   k_post_tonemap      src/shaders/shader.wgsl:3-33,59-64    Uchimura "GT" curve on accumulation.rgb / accumulation.w
//   k_post_rgb8         src/image_helper.rs:41-48 + src/image_helper/tonemapping.rs   the 8-bit gamma-2.2 image write_image saves
//   k_dn_*              (no reference counterpart) pt_denoise's edge-aware a-trous filter on the accumulation and the first-hit guides
//
// WGSL leaves bilinear filter weights, mat*vec summation order, pow/exp precision and out-of-range casts to the GPU.  Here
// they are exact binary32 operations in the written order, pow(x, c) = exp(c ln x) with pt_math.h's routines, saturating
// casts, out-of-bounds textureLoad = 0 — the same definitions the oracle uses, so the two agree bit for bit.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "pt_kernels.h"

namespace pt {
namespace {

struct Tex
{
    const f4* p;
    int w, h;
    __device__ __forceinline__ f4 at(int x, int y) const { return p[(size_t)y * w + x]; }
};
__device__ __forceinline__ f4 add4(f4 a, f4 b) { return f4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ f4 mul4(f4 a, float s) { return f4{a.x * s, a.y * s, a.z * s, a.w * s}; }
__device__ __forceinline__ int to_i32_sat(float f)
{
    return isnan_f(f) ? 0 : (f >= 2147483648.0f ? 2147483647 : (f <= -2147483648.0f ? (-2147483647 - 1) : (int)f));
}
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// textureSampleLevel(tex, sampler{linear, clamp-to-edge}, uv, 0)  (sampler: src/state.rs:169-178)
__device__ f4 bilinear(const Tex& t, float u, float v)
{
    const float x = u * (float)t.w - 0.5f, y = v * (float)t.h - 0.5f;
    const float bx = floorf(x), by = floorf(y);
    const float fx = x - bx, fy = y - by;
    const int x0 = to_i32_sat(bx), y0 = to_i32_sat(by);
    const int xa = clampi(x0, t.w), xb = clampi(x0 < 2147483647 ? x0 + 1 : x0, t.w);
    const int ya = clampi(y0, t.h), yb = clampi(y0 < 2147483647 ? y0 + 1 : y0, t.h);
    const f4 top = add4(mul4(t.at(xa, ya), 1.0f - fx), mul4(t.at(xb, ya), fx));
    const f4 bot = add4(mul4(t.at(xa, yb), 1.0f - fx), mul4(t.at(xb, yb), fx));
    return add4(mul4(top, 1.0f - fy), mul4(bot, fy));
}
__device__ __forceinline__ f3 w_divide(f4 v) // v.xyz / max(v.w, 1.0)
{
    const float d = v.w > 1.0f ? v.w : 1.0f;
    return f3{v.x / d, v.y / d, v.z / d};
}
__device__ __forceinline__ f3 to_ycocg(f3 c) // compute.wgsl:64-71 (mat3x3 columns times vector)
{
    return f3{(0.25f * c.x + 0.5f * c.y) + -0.25f * c.z, (0.5f * c.x + 0.0f * c.y) + 0.5f * c.z, (0.25f * c.x + -0.5f * c.y) + -0.25f * c.z};
}
__device__ __forceinline__ f3 from_ycocg(f3 c) // compute.wgsl:73-80
{
    return f3{(1.0f * c.x + 1.0f * c.y) + 1.0f * c.z, (1.0f * c.x + 0.0f * c.y) + -1.0f * c.z, (-1.0f * c.x + 1.0f * c.y) + -1.0f * c.z};
}
__device__ __forceinline__ float maxf_w(float a, float b) { return a > b ? a : b; }
__device__ f3 clip_to_box(f3 mn, f3 mx, f3 q) // clip_aabb  compute.wgsl:82-101
{
    const f3 centre = 0.5f * (mx + mn), extent = 0.5f * (mx - mn);
    const f3 v = q - centre;
    const f3 unit{v.x / extent.x, v.y / extent.y, v.z / extent.z};
    const float m = maxf_w(fabsf(unit.x), maxf_w(fabsf(unit.y), fabsf(unit.z)));
    if (m > 1.0f) return centre + v / m;
    return q;
}
__device__ f3 catmull_rom(const Tex& tex, float ux, float uy) // sample_catmull_rom  compute.wgsl:16-62
{
    const float sx = (float)tex.w, sy = (float)tex.h;
    const float px = ux * sx + 0.5f, py = uy * sy + 0.5f;
    const float t1x = floorf(px - 0.5f) + 0.5f, t1y = floorf(py - 0.5f) + 0.5f;
    const float fx = px - t1x, fy = py - t1y;
    const float w0x = fx * (-0.5f + fx * (1.0f - 0.5f * fx)), w0y = fy * (-0.5f + fy * (1.0f - 0.5f * fy));
    const float w1x = 1.0f + fx * fx * (-2.5f + 1.5f * fx), w1y = 1.0f + fy * fy * (-2.5f + 1.5f * fy);
    const float w2x = fx * (0.5f + fx * (2.0f - 1.5f * fx)), w2y = fy * (0.5f + fy * (2.0f - 1.5f * fy));
    const float w3x = fx * fx * (-0.5f + 0.5f * fx), w3y = fy * fy * (-0.5f + 0.5f * fy);
    const float w12x = w1x + w2x, w12y = w1y + w2y;
    const float o12x = w2x / (w1x + w2x), o12y = w2y / (w1y + w2y);
    const float p0x = (t1x - 1.0f) / sx, p0y = (t1y - 1.0f) / sy, p3x = (t1x + 2.0f) / sx, p3y = (t1y + 2.0f) / sy;
    const float p12x = (t1x + o12x) / sx, p12y = (t1y + o12y) / sy;
    const float us[3] = {p0x, p12x, p3x}, vs[3] = {p0y, p12y, p3y}, wu[3] = {w0x, w12x, w3x}, wv[3] = {w0y, w12y, w3y};
    f3 c{0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) c = c + w_divide(bilinear(tex, us[i], vs[j])) * wu[i] * wv[j];
    return c;
}
__device__ __forceinline__ float pow_det(float x, float c) { return exp_det(c * ln_det(x)); }
__device__ float gt_curve(float x, float p, float a, float m, float l, float c, float b) // gt_tonemap  shader.wgsl:3-33
{
    const float l0 = (p - m) * l / a;
    const float t = clamp_rs((x - 0.0f) / (m - 0.0f), 0.0f, 1.0f); // smoothstep(0, m, x)
    const float w0 = 1.0f - t * t * (3.0f - 2.0f * t);
    const float w2 = x >= m + l0 ? 1.0f : 0.0f;                    // step(m + l0, x)
    const float w1 = 1.0f - w0 - w2;
    const float toe = m * pow_det(x / m, c) + b;
    const float lin = m + a * (x - m);
    const float s0 = m + l0, s1 = m + a * l0, c2 = a * p / (p - s1);
    const float shoulder = p - (p - s1) * exp_det(-c2 * (x - s0) / p);
    const float r = (toe * w0 + lin * w1) + shoulder * w2;
    return maxf_w(r, 0.0f);
}

// tonemapping.rs:1-96 — the CPU-side curve differs from shader.wgsl in its branches (x < 0 -> b, branchy smoothstep, and the
// shoulder weight gt_lerp(x, e, e) which is 0/0 = NaN at x == e exactly); restated as written.
__device__ float gt_curve_rs(float x, float p, float a, float m, float l, float c, float b)
{
    if (x < 0.0f) return b;
    const float l0 = (p - m) * l / a;
    float sm;                                                      // gt_smoothstep(x, 0, m)  :36-52
    if (x < 0.0f) sm = 0.0f;
    else if (x > m) sm = 1.0f;
    else { const float q = (x - 0.0f) / (m - 0.0f); const float r = 3.0f - 2.0f * q; sm = q * q * r; }
    const float w0 = 1.0f - sm;
    const float e = m + l0;
    float w2;                                                      // gt_lerp(x, e, e)  :20-34
    if (x < e) w2 = 0.0f;
    else if (x > e) w2 = 1.0f;
    else w2 = (x - e) / (e - e);
    const float w1 = 1.0f - w0 - w2;
    const float t = (m * pow_det(x / m, c) + b) * w0;              // gt_toe
    const float u = (m + a * (x - m)) * w1;                        // gt_linear
    const float s0 = m + l0, s1 = m + a * l0, c2 = a * p / (p - s1);
    const float v = (p - (p - s1) * exp_det(-c2 * (x - s0) / p)) * w2; // gt_shoulder
    return t + u + v;
}
__device__ __forceinline__ uint32_t to_u8_sat(float f) { return isnan_f(f) ? 0u : (f >= 255.0f ? 255u : (f <= 0.0f ? 0u : (uint32_t)f)); } // Rust `as u8`

__global__ void __launch_bounds__(256) k_post_accumulate(uint32_t n, const f4* __restrict__ input, f4* __restrict__ accum)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 a = accum[i], c = input[i];
    accum[i] = f4{a.x + c.x, a.y + c.y, a.z + c.z, a.w + 1.0f};
}

struct Mat4 { float m[16]; };

__global__ void __launch_bounds__(256) k_post_velocity(int w, int h, const f4* __restrict__ position, const Mat4 M, float2* __restrict__ velocity)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    const int x = i % w, y = i / w;
    const f4 P = position[i];
    const float cu = ((float)x + 0.5f) / (float)w, cv = ((float)y + 0.5f) / (float)h;
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = ((M.m[k] * P.x + M.m[4 + k] * P.y) + M.m[8 + k] * P.z) + M.m[12 + k] * 1.0f;
    const f3 d = w_divide(f4{r[0], r[1], r[2], r[3]});
    velocity[i] = make_float2(cu - (d.x * 0.5f + 0.5f), cv - (d.y * 0.5f + 0.5f));
}

// pt_frame_moving: the first-hit point of every pixel carried back to where its instance had it in the previous frame: into object space
// with the instance's inverse matrix, out again with its previous forward matrix (glam's transform_point3, twice).  A miss, an instance
// without a previous matrix or one that did not move passes the point on untouched, bit for bit.  w (the hit distance) is kept.
__global__ void __launch_bounds__(256) k_post_motion(uint32_t n, const f4* __restrict__ position, const uint32_t* __restrict__ instance, uint32_t n_instances,
                                                      const MotionRow* __restrict__ rows, f4* __restrict__ x_prev)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f4 P = position[i];
    const uint32_t inst = instance[i];
    if (inst < n_instances && rows[inst].moved)
    {
        const MotionRow& m = rows[inst];
        float o[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = ((m.inv[4 * k] * P.x + m.inv[4 * k + 1] * P.y) + m.inv[4 * k + 2] * P.z) + m.inv[4 * k + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = ((m.prv[4 * k] * o[0] + m.prv[4 * k + 1] * o[1]) + m.prv[4 * k + 2] * o[2]) + m.prv[4 * k + 3];
        P = f4{q[0], q[1], q[2], P.w};
    }
    x_prev[i] = P;
}

__global__ void __launch_bounds__(256) k_post_reproject(int w, int h, const f4* __restrict__ input, const f4* __restrict__ accum,
                                                         const float2* __restrict__ velocity, const uint32_t* __restrict__ id, f4* __restrict__ output)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    const int cx = i % w, cy = i / w;
    const Tex in{input, w, h}, acc{accum, w, h};
    const f4 cur4 = in.at(cx, cy);
    const f3 current{cur4.x, cur4.y, cur4.z};
    f3 m1{0.0f, 0.0f, 0.0f}, m2{0.0f, 0.0f, 0.0f};
    float closest_depth = 1e20f;
    int vx = 0, vy = 0;
    const int x0 = cx - 1 > 0 ? cx - 1 : 0, y0 = cy - 1 > 0 ? cy - 1 : 0;
    const int x1 = cx + 1 < w - 1 ? cx + 1 : w - 1, y1 = cy + 1 < h - 1 ? cy + 1 : h - 1;
    const int n = (x1 + 1 - x0) * (y1 + 1 - y0);
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y)
        {
            const f4 dd = in.at(x, y);
            const f3 d = to_ycocg(f3{dd.x, dd.y, dd.z});
            m1 = m1 + d;
            m2 = m2 + d * d;
            if (dd.w < closest_depth) { closest_depth = dd.w; vx = x; vy = y; }
        }
    const float dx = (float)w, dy = (float)h;
    const float cu = ((float)cx + 0.5f) / dx, cv = ((float)cy + 0.5f) / dy;
    const float2 vel = velocity[(size_t)vy * w + vx];
    const float pu = cu - vel.x, pv = cv - vel.y;
    const int px = to_i32_sat(floorf(pu * dx)), py = to_i32_sat(floorf(pv * dy));
    const bool oob = px < 0 || py < 0 || px >= w || py >= h;
    const uint32_t current_id = id[i] & 0xffffu;
    const uint32_t old_id = oob ? 0u : ((id[(size_t)py * w + px] >> 16) & 0xffffu);
    if (current_id != old_id || oob)
    {
        // disocclusion: average of four bilinear taps at the texel corners  compute.wgsl:170-181
        const float c0x = (float)cx / dx, c0y = (float)cy / dy, c1x = c0x + 1.0f / dx, c1y = c0y + 1.0f / dy;
        const f4 s = add4(add4(add4(bilinear(in, c0x, c0y), bilinear(in, c0x, c1y)), bilinear(in, c1x, c0y)), bilinear(in, c1x, c1y));
        output[i] = f4{s.x / 4.0f, s.y / 4.0f, s.z / 4.0f, s.w / 4.0f};
        return;
    }
    const float fn = (float)n;
    const f3 mu = m1 / fn;
    const f3 var = m2 / fn - mu * mu;
    const f3 sigma{sqrtf(var.x), sqrtf(var.y), sqrtf(var.z)};
    const f3 mn = mu - 1.0f * sigma, mx = mu + 1.0f * sigma;
    const f3 prev = catmull_rom(acc, pu, pv);
    const f3 clamped = from_ycocg(clip_to_box(mn, mx, to_ycocg(prev)));
    const f3 o = clamped * (1.0f - 0.15f) + current * 0.15f; // mix(clamped, current, 0.15)
    output[i] = f4{o.x, o.y, o.z, 1.0f};
}

__global__ void __launch_bounds__(256) k_post_tonemap(uint32_t n, const f4* __restrict__ accum, f4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 a = accum[i];
    out[i] = f4{gt_curve(a.x / a.w, 1.0f, 1.0f, 0.22f, 0.4f, 1.33f, 0.0f), gt_curve(a.y / a.w, 1.0f, 1.0f, 0.22f, 0.4f, 1.33f, 0.0f),
                gt_curve(a.z / a.w, 1.0f, 1.0f, 0.22f, 0.4f, 1.33f, 0.0f), 1.0f};
}

// one thread per pixel writes 3 bytes; a wave's 192 bytes are contiguous
__global__ void __launch_bounds__(256) k_post_rgb8(uint32_t n, const f4* __restrict__ accum, uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 a = accum[i];
    const float g = 1.0f / 2.2f;
    const float ch[3] = {a.x / a.w, a.y / a.w, a.z / a.w};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        out[(size_t)i * 3u + k] = (uint8_t)to_u8_sat(pow_det(gt_curve_rs(ch[k], 1.0f, 1.0f, 0.22f, 0.4f, 1.33f, 0.0f), g) * 255.0f);
}

// strips gathered from `world` ranks (rank r's rows, padded to pad_rows, at parts + r * pad_rows * w) -> the whole frame, row-major:
// global row y belongs to rank (y / strip) % world and is that rank's local row (y / strip / world) * strip + y % strip  (compute_rows)
__global__ void __launch_bounds__(256) k_post_deinterleave(uint32_t w, uint32_t h, uint32_t world, uint32_t strip, uint32_t pad_rows,
                                                            const f4* __restrict__ parts, f4* __restrict__ full)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    const uint32_t y = i / w, x = i - y * w;
    const uint32_t st = y / strip, rank = st % world, ly = (st / world) * strip + (y - st * strip);
    full[i] = parts[((size_t)rank * pad_rows + ly) * w + x];
}

// ---- edge-aware a-trous denoiser (pt_denoise / pt_post_denoise): SVGF's spatial filter, every operation in the order include/pt_api.h
// states.  The per-pixel arithmetic is pt_filter.h's core under the screen rule; the kernels are its shells.  One thread per pixel in
// 16 x 16 workgroups; what a tap reads is three 16-byte loads (colour | variance, position | t, normal | valid) and the model word.

// the prep kernel's albedo: none (pt_denoise), the albedo image (pt_denoise_albedo's guide, a caller's image) or the mean-albedo sums S (A = S.rgb / S.w)
enum class AlbedoFrom { None, Image, Sums };
struct NoAlbedo {};
struct AlbedoImages
{
    const uint32_t* model;
    const f4* albedo;
    f4* kd;
};

// colour = acc.rgb / acc.w, variance = the adaptive criterion's e2 (moments) or 0 (the spatial pass fills it in), valid = acc.w != 0.
// With an albedo A (pt_denoise_albedo): k = pt_filter.h's divisor of A; colour c' = (acc / k) / acc.w; with moments the variance e2 of the
// modulated colour scaled by r * r, r = l(c') / l(c) (1 where l(c) is not positive), which keeps the relative error.  k goes to kd for the
// last level.
template <AlbedoFrom SRC>
__global__ void __launch_bounds__(256) k_dn_prep(uint32_t n, const f4* __restrict__ accum, const float* __restrict__ moments, const f4* __restrict__ normal,
                                                 f4* __restrict__ cv, f4* __restrict__ nv,
                                                 const std::conditional_t<SRC == AlbedoFrom::None, NoAlbedo, AlbedoImages> al)
{
    constexpr bool ALBEDO = SRC != AlbedoFrom::None;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 a = accum[i];
    if (a.w == 0.0f)
    {
        cv[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        nv[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (ALBEDO) al.kd[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    f4 c{a.x / a.w, a.y / a.w, a.z / a.w, 0.0f};
    [[maybe_unused]] f4 k;
    if constexpr (ALBEDO)
    {
        const uint32_t mp = al.model[i];
        k = divisor(MISS_ID, f4{0.0f, 0.0f, 0.0f, 0.0f}); // a miss does not read the albedo
        if (mp != MISS_ID)
        {
            f4 A = al.albedo[i];
            if (SRC == AlbedoFrom::Sums) A = f4{A.x / A.w, A.y / A.w, A.z / A.w, 0.0f};
            k = divisor(mp, A);
        }
        c = f4{(a.x / k.x) / a.w, (a.y / k.y) / a.w, (a.z / k.z) / a.w, 0.0f};
    }
    float var = 0.0f;
    if (moments)
    {
        var = mean_variance(a, moments[i]);
        if constexpr (ALBEDO)
        {
            const float lc = lum(f4{a.x / a.w, a.y / a.w, a.z / a.w, 0.0f});
            const float r = lc > 0.0f ? lum(c) / lc : 1.0f;
            var = (var * r) * r;
        }
    }
    const f4 nr = normal[i];
    cv[i] = f4{c.x, c.y, c.z, var};
    nv[i] = f4{nr.x, nr.y, nr.z, 1.0f};
    if constexpr (ALBEDO) al.kd[i] = k;
}

// variance of l over the 7 x 7 neighbourhood (pt_filter.h's walk, a neighbour valid where nv.w says so)
__global__ void __launch_bounds__(256) k_dn_spatial_var(int w, int h, const DenoiseK p, const f4* __restrict__ cv_in, const f4* __restrict__ pos,
                                                        const f4* __restrict__ nv, const uint32_t* __restrict__ model, f4* __restrict__ cv_out)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const f4 cp = cv_in[i], np = nv[i];
    if (np.w == 0.0f) { cv_out[i] = f4{0.0f, 0.0f, 0.0f, 0.0f}; return; }
    cv_out[i] = f4{cp.x, cp.y, cp.z, spatial_variance(ScreenRule(nv, model, i), w, h, p, cv_in, pos, nv, x, y)};
}

// one a-trous level, step s (pt_filter.h's atrous_level).  FINAL writes the result (c', 1) / (0, 0, 0, 0) instead of (c', var'); REMOD
// (pt_denoise_albedo's last level, FINAL) multiplies that result by the divisor k the prep kernel kept in kmul, per channel (kmul is not
// read otherwise)
template <bool FINAL, bool REMOD = false>
__global__ void __launch_bounds__(256) k_dn_level(int w, int h, int s, const DenoiseK p, const f4* __restrict__ cv_in, const f4* __restrict__ pos,
                                                  const f4* __restrict__ nv, const uint32_t* __restrict__ model, f4* __restrict__ cv_out,
                                                  const f4* __restrict__ kmul)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    if (nv[i].w == 0.0f) { cv_out[i] = f4{0.0f, 0.0f, 0.0f, 0.0f}; return; }
    const f4 c = atrous_level(ScreenRule(nv, model, i), w, h, s, p, cv_in, pos, nv, x, y);
    static_assert(FINAL || !REMOD, "");
    if (REMOD)
    {
        const f4 k = kmul[i];
        cv_out[i] = f4{c.x * k.x, c.y * k.y, c.z * k.z, 1.0f};
    }
    else cv_out[i] = FINAL ? f4{c.x, c.y, c.z, 1.0f} : c;
}

// ---- temporal stage (pt_frame_temporal / pt_post_temporal): the per-pixel steps are pt_temporal.h's, shared with the host path.  One thread
// per pixel in 16 x 16 workgroups.  k_tp_reproject is gather-bound: per tap two 16-byte loads (C | N, n' | m') decide whether the other two
// (X' | t', the moments) are made at all, and the four taps' loads stand before the first use.
__global__ void __launch_bounds__(256) k_tp_motion_normal(uint32_t n, const f4* __restrict__ normal, const uint32_t* __restrict__ instance, uint32_t n_instances,
                                                          const MotionRow* __restrict__ rows, f4* __restrict__ n_prev)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    f4 N = normal[i];
    const uint32_t inst = instance[i];
    if (inst < n_instances && rows[inst].moved) N = motion_normal(rows[inst].inv, rows[inst].prv, N);
    n_prev[i] = N;
}

// RESCUE, MEAN: pt_temporal.h's options.  DEMOD (pt_frame_temporal's demodulate): the pixel's divisor k from its albedo guide goes to kd for
// the last level's multiplication, and cur is divided by it where temporal_pixel loads it; albedo and kd are not touched otherwise
template <bool RESCUE, bool MEAN, bool DEMOD>
__global__ void __launch_bounds__(256) k_tp_reproject(const TemporalImages im, const TemporalK k, f4* __restrict__ hist_out, f2* __restrict__ mom_out,
                                                      const f4* __restrict__ albedo, f4* __restrict__ kd)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= im.w || y >= im.h) return;
    const size_t i = (size_t)y * im.w + x;
    TemporalOut o;
    if (DEMOD)
    {
        const f4 kdiv = divisor(im.model[i], albedo[i]);
        kd[i] = kdiv;
        o = temporal_pixel<RESCUE, MEAN, true>(im, k, x, y, kdiv);
    }
    else o = temporal_pixel<RESCUE, MEAN>(im, k, x, y);
    hist_out[i] = o.h;
    mom_out[i] = o.m;
}

// the variance of every pixel and the filter's input images; a pixel whose history is long enough returns before the 49-tap loop
__global__ void __launch_bounds__(256) k_tp_variance(int w, int h, const DenoiseK p, float alpha, const f4* __restrict__ cn, const f2* __restrict__ mom,
                                                     const f4* __restrict__ pos, const f4* __restrict__ nrm, const uint32_t* __restrict__ model,
                                                     f4* __restrict__ cv, f4* __restrict__ nv, float* __restrict__ var)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float v = temporal_variance(w, h, p, alpha, cn, mom, pos, nrm, model, x, y);
    var[i] = v;
    if (cv)
    {
        const f4 c = cn[i];
        cv[i] = f4{c.x, c.y, c.z, v};
    }
    if (nv)
    {
        const f4 n = nrm[i];
        nv[i] = f4{n.x, n.y, n.z, 1.0f};
    }
}

// step 7: the current guides become the history's; lvl0 (feedback) replaces the history's colour, null leaves C
__global__ void __launch_bounds__(256) k_tp_store(uint32_t n, const f4* __restrict__ pos, const f4* __restrict__ nrm, const uint32_t* __restrict__ model,
                                                  const f4* __restrict__ lvl0, f4* __restrict__ hist, f4* __restrict__ xq, f4* __restrict__ gq)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 nr = nrm[i];
    xq[i] = pos[i];
    gq[i] = f4{nr.x, nr.y, nr.z, from_bits(model[i])};
    if (lvl0)
    {
        const f4 c = lvl0[i];
        hist[i] = f4{c.x, c.y, c.z, hist[i].w};
    }
}

// pt_frame_temporal's demodulate with one level and feedback: the store above took level 0's output, which is the result; now the multiplication
// k_dn_level<true, true> would have done (the same single operation per channel)
__global__ void __launch_bounds__(256) k_tp_remodulate(uint32_t n, const f4* __restrict__ kmul, f4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f4 c = out[i], k = kmul[i];
    out[i] = f4{c.x * k.x, c.y * k.y, c.z * k.z, 1.0f};
}

// the temporal stage's step 7 between the levels: after level 0, k_tp_store of the current guides, with feedback also of level 0's output
struct Level0Store
{
    const f4* normal;
    bool feedback;
    f4 *hist, *xq, *gq;
};

// the spatial variance where there are no moments, then the levels, on the prepared (colour | variance) in cv_a; kmul: the result, and only
// the result, is multiplied by it (pt_denoise_albedo, demodulate), null: it is not; store: null for the spatial filter
void denoise_levels(hipStream_t s, int w, int h, const DenoiseK& p, bool moments, const f4* position, const uint32_t* model, f4* cv_a, f4* cv_b, f4* nv,
                    const f4* kmul, f4* out, const Level0Store* store = nullptr)
{
    const dim3 tile(16, 16), grid((w + 15) / 16, (h + 15) / 16);
    const uint32_t n = (uint32_t)w * (uint32_t)h;
    f4* cur = cv_a;
    f4* other = cv_b;
    if (!moments)
    {
        hipLaunchKernelGGL(k_dn_spatial_var, grid, tile, 0, s, w, h, p, (const f4*)cv_a, position, (const f4*)nv, model, cv_b);
        std::swap(cur, other);
    }
    // the history keeps level 0's output BEFORE the multiplication: where level 0 is also the last, the multiplication follows the store
    const bool remod_after = kmul && store && store->feedback && p.iterations == 1u;
    for (uint32_t it = 0; it < p.iterations; ++it)
    {
        const bool last = it + 1u == p.iterations, remod = last && kmul && !remod_after;
        f4* dst = last ? out : other;
        const auto level = !last ? k_dn_level<false> : remod ? k_dn_level<true, true> : k_dn_level<true>;
        hipLaunchKernelGGL(level, grid, tile, 0, s, w, h, 1 << it, p, (const f4*)cur, position, (const f4*)nv, model, dst, remod ? kmul : (const f4*)nullptr);
        if (it == 0u && store)
            hipLaunchKernelGGL(k_tp_store, dim3((n + 255u) / 256u), dim3(256), 0, s, n, position, store->normal, model,
                               store->feedback ? (const f4*)dst : (const f4*)nullptr, store->hist, store->xq, store->gq);
        if (!last) std::swap(cur, other);
    }
    if (remod_after) hipLaunchKernelGGL(k_tp_remodulate, dim3((n + 255u) / 256u), dim3(256), 0, s, n, kmul, out);
}
} // namespace

void launch_temporal_motion_normal(hipStream_t s, uint32_t n, const f4* normal, const uint32_t* instance, uint32_t n_instances, const MotionRow* rows, f4* n_prev)
{
    hipLaunchKernelGGL(k_tp_motion_normal, dim3((n + 255u) / 256u), dim3(256), 0, s, n, normal, instance, n_instances, rows, n_prev);
}
void launch_temporal_reproject(hipStream_t s, const TemporalImages& im, const TemporalK& k, bool rescue, bool mean_length, const f4* albedo, f4* kd, f4* hist_out,
                               f2* mom_out)
{
    const dim3 grid((im.w + 15) / 16, (im.h + 15) / 16), tile(16, 16);
    with_temporal_options(rescue, mean_length, [&](auto R, auto M) {
        if (albedo) hipLaunchKernelGGL((k_tp_reproject<R.value, M.value, true>), grid, tile, 0, s, im, k, hist_out, mom_out, albedo, kd);
        else hipLaunchKernelGGL((k_tp_reproject<R.value, M.value, false>), grid, tile, 0, s, im, k, hist_out, mom_out, albedo, kd);
    });
}
void launch_temporal_variance(hipStream_t s, int w, int h, const DenoiseK& p, float alpha, const f4* cn, const f2* mom, const f4* position, const f4* normal,
                              const uint32_t* model, f4* cv, f4* nv, float* var)
{
    hipLaunchKernelGGL(k_tp_variance, dim3((w + 15) / 16, (h + 15) / 16), dim3(16, 16), 0, s, w, h, p, alpha, cn, mom, position, normal, model, cv, nv, var);
}
void launch_temporal_filter(hipStream_t s, int w, int h, const DenoiseK& p, bool feedback, const f4* position, const f4* normal, const uint32_t* model, f4* cv_a,
                            f4* cv_b, f4* nv, const f4* kmul, f4* out, f4* hist, f4* xq, f4* gq)
{
    const Level0Store store{normal, feedback, hist, xq, gq};
    denoise_levels(s, w, h, p, true, position, model, cv_a, cv_b, nv, kmul, out, &store);
}

void launch_denoise(hipStream_t s, int w, int h, const DenoiseK& p, const DenoiseImages& im)
{
    const uint32_t n = (uint32_t)w * (uint32_t)h;
    const dim3 grid((n + 255u) / 256u), block(256);
    const AlbedoImages al{im.model, im.albedo, im.kd};
    if (!im.albedo) hipLaunchKernelGGL(k_dn_prep<AlbedoFrom::None>, grid, block, 0, s, n, im.accum, im.moments, im.normal, im.cv_a, im.nv, NoAlbedo{});
    else if (im.albedo_is_sum) hipLaunchKernelGGL(k_dn_prep<AlbedoFrom::Sums>, grid, block, 0, s, n, im.accum, im.moments, im.normal, im.cv_a, im.nv, al);
    else hipLaunchKernelGGL(k_dn_prep<AlbedoFrom::Image>, grid, block, 0, s, n, im.accum, im.moments, im.normal, im.cv_a, im.nv, al);
    denoise_levels(s, w, h, p, im.moments != nullptr, im.position, im.model, im.cv_a, im.cv_b, im.nv, im.albedo ? (const f4*)im.kd : nullptr, im.out);
}

void launch_post_deinterleave(hipStream_t s, uint32_t w, uint32_t h, uint32_t world, uint32_t strip, uint32_t pad_rows, const f4* parts, f4* full)
{
    hipLaunchKernelGGL(k_post_deinterleave, dim3((w * h + 255u) / 256u), dim3(256), 0, s, w, h, world, strip, pad_rows, parts, full);
}
void launch_post_rgb8(hipStream_t s, uint32_t n, const f4* accum, uint8_t* out)
{
    hipLaunchKernelGGL(k_post_rgb8, dim3((n + 255u) / 256u), dim3(256), 0, s, n, accum, out);
}
void launch_post_accumulate(hipStream_t s, uint32_t n, const f4* input, f4* accum)
{
    hipLaunchKernelGGL(k_post_accumulate, dim3((n + 255u) / 256u), dim3(256), 0, s, n, input, accum);
}
void launch_post_velocity(hipStream_t s, int w, int h, const f4* position, const float* m16, float* velocity_xy)
{
    Mat4 M;
    for (int i = 0; i < 16; ++i) M.m[i] = m16[i];
    hipLaunchKernelGGL(k_post_velocity, dim3((w * h + 255) / 256), dim3(256), 0, s, w, h, position, M, reinterpret_cast<float2*>(velocity_xy));
}
void launch_post_motion(hipStream_t s, uint32_t n, const f4* position, const uint32_t* instance, uint32_t n_instances, const MotionRow* rows, f4* x_prev)
{
    hipLaunchKernelGGL(k_post_motion, dim3((n + 255u) / 256u), dim3(256), 0, s, n, position, instance, n_instances, rows, x_prev);
}
void launch_post_reproject(hipStream_t s, int w, int h, const f4* input, const f4* accum, const float* velocity_xy, const uint32_t* id, f4* output)
{
    hipLaunchKernelGGL(k_post_reproject, dim3((w * h + 255) / 256), dim3(256), 0, s, w, h, input, accum, reinterpret_cast<const float2*>(velocity_xy), id, output);
}
void launch_post_tonemap(hipStream_t s, uint32_t n, const f4* accum, f4* out)
{
    hipLaunchKernelGGL(k_post_tonemap, dim3((n + 255u) / 256u), dim3(256), 0, s, n, accum, out);
}

} // namespace pt
