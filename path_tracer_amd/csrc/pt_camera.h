// The camera ray of (pixel, sample): one definition for the gfx950 kernels and for the host evaluation (pt_primary_ray).
// Pinhole: main.rs:193-199 + Camera::create_ray camera.rs:94-105.  Thin lens: include/pt_api.h, pt_set_lens.
#pragma once
#include "pt_types.h"

namespace pt {

// point - eye of Camera::create_ray (the pinhole ray before it is normalised) for the jittered position of `sample` inside pixel
// (gx, gy); rng is the stream of (pixel, sample) with nothing drawn yet and comes back with the seed draw taken (main.rs:193)
PT_HD f3 camera_ray_unnormalised(const RenderParams& rp, const CameraView& cam, uint32_t gx, uint32_t gy, uint32_t sample, Stream& rng)
{
    const uint32_t seed = rng.u32();                                       // main.rs:193 (the stream's draw 0)
    float jx, jy;
    ss_sobol(rp.n_sobol, sample, seed, &jx, &jy);                          // main.rs:194
    const float ox = jx - 0.5f, oy = jy - 0.5f;
    const float u = ((float)gx + ox) / (float)rp.width;                    // main.rs:196
    const float v = ((float)gy + oy) / (float)rp.height;                   // main.rs:197
    // Camera::create_ray  camera.rs:94-105  (Mat4::project_point3, then normalise)
    const float nx = u * 2.0f - 1.0f, ny = v * 2.0f - 1.0f, nz = 0.0f;
    const float* M = cam.ray_matrix;
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        float t = M[i] * nx;
        t = M[4 + i] * ny + t;
        t = M[8 + i] * nz + t;
        t = M[12 + i] + t;
        r[i] = t;
    }
    const float rw = 1.0f / r[3];
    const f3 eye{cam.eye[0], cam.eye[1], cam.eye[2]};
    return f3{r[0] * rw, r[1] * rw, r[2] * rw} - eye;
}

// direction of the pinhole camera ray of (pixel gx, gy; sample); its origin is the eye and ONE draw of the stream is consumed
PT_HD f3 camera_ray_dir(const RenderParams& rp, const CameraView& cam, uint32_t gx, uint32_t gy, uint32_t sample)
{
    Stream rng{stream_key(rp.seed, gy * rp.width + gx, sample), 0u};
    return unit3(camera_ray_unnormalised(rp, cam, gx, gy, sample, rng));
}

// thin lens: the ray from a point of the lens disk (polar map of a second Sobol point, seeded by the stream's draw 1) through the point
// where the pinhole ray meets the plane of focus.  TWO draws of the stream are consumed.  Every operation rounded once, in this order.
PT_HD f3 camera_ray(const RenderParams& rp, const CameraView& cam, const LensView& lens, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    Stream rng{stream_key(rp.seed, gy * rp.width + gx, sample), 0u};
    const f3 q = camera_ray_unnormalised(rp, cam, gx, gy, sample, rng);
    const uint32_t seed2 = rng.u32();
    float lx, ly;
    ss_sobol(rp.n_sobol, sample, seed2, &lx, &ly);
    const float rad = lens.radius * sqrtf(lx), phi = 6.2831855f * ly;
    float sn, cs;
    sincos_det(phi, &sn, &cs);
    const float a = rad * cs, b = rad * sn;
    const f3 eye{cam.eye[0], cam.eye[1], cam.eye[2]};
    const f3 c0{lens.c0[0], lens.c0[1], lens.c0[2]}, c1{lens.c1[0], lens.c1[1], lens.c1[2]};
    const f3 o = eye + (c0 * a + c1 * b);
    const f3 f = q * lens.focus + eye;
    *origin = o;
    return unit3(f - o);
}

} // namespace pt
