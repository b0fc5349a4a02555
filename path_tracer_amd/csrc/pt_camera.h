// The camera ray of (pixel, sample): one definition for the gfx950 kernels and for the host evaluation (pt_primary_ray).
// Pinhole: main.rs:193-199 + Camera::create_ray camera.rs:94-105.  Thin lens: include/pt_api.h, pt_set_lens.  Panoramic and orthographic:
// include/pt_api.h, pt_set_projection.  primary_ray at the end is the one entry the kernels use: the camera's kind is the type of its view.
#pragma once
#include <type_traits>
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

// Panoramic and orthographic cameras (include/pt_api.h, pt_set_projection).  Both take the jittered position of the pinhole ray
// (main.rs:193-197, camera.rs:96: ndc in [-1, 1], row 0 = bottom), consume ONE draw of the stream and round every operation once, in
// the order written.  (The pinhole's own lines above stay as they are: its kernels keep their instruction streams.)
PT_HD void camera_ndc(const RenderParams& rp, uint32_t gx, uint32_t gy, uint32_t sample, float* nx, float* ny)
{
    Stream rng{stream_key(rp.seed, gy * rp.width + gx, sample), 0u};
    const uint32_t seed = rng.u32();
    float jx, jy;
    ss_sobol(rp.n_sobol, sample, seed, &jx, &jy);
    const float ox = jx - 0.5f, oy = jy - 0.5f;
    const float u = ((float)gx + ox) / (float)rp.width;
    const float v = ((float)gy + oy) / (float)rp.height;
    *nx = u * 2.0f - 1.0f;
    *ny = v * 2.0f - 1.0f;
}

// PANORAMA: azimuth phi = ax * nx about the camera's y axis, elevation theta = ay * ny; the ray leaves the eye
PT_HD f3 camera_ray_panorama(const RenderParams& rp, const CameraView& cam, const ProjView& proj, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    float nx, ny;
    camera_ndc(rp, gx, gy, sample, &nx, &ny);
    const float phi = proj.sx * nx, theta = proj.sy * ny;
    float sp, cp, st, ct;
    sincos_det(phi, &sp, &cp);
    sincos_det(theta, &st, &ct);
    const float dx = ct * sp, dy = st, dz = -(ct * cp);
    const f3 c0{proj.c0[0], proj.c0[1], proj.c0[2]}, c1{proj.c1[0], proj.c1[1], proj.c1[2]}, c2{proj.c2[0], proj.c2[1], proj.c2[2]};
    const f3 w = (c0 * dx + c1 * dy) + c2 * dz;
    *origin = f3{cam.eye[0], cam.eye[1], cam.eye[2]};
    return unit3(w);
}

// ORTHOGRAPHIC: every ray runs along the view axis (proj.c2 holds -c2 normalised) from its point of the view volume's near face
PT_HD f3 camera_ray_orthographic(const RenderParams& rp, const CameraView& cam, const ProjView& proj, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    float nx, ny;
    camera_ndc(rp, gx, gy, sample, &nx, &ny);
    const float a = proj.sx * nx, b = proj.sy * ny;
    const f3 eye{cam.eye[0], cam.eye[1], cam.eye[2]};
    const f3 c0{proj.c0[0], proj.c0[1], proj.c0[2]}, c1{proj.c1[0], proj.c1[1], proj.c1[2]};
    *origin = eye + (c0 * a + c1 * b);
    return f3{proj.c2[0], proj.c2[1], proj.c2[2]};
}

// either, by the view's kind (launch-invariant: where a kernel calls this the branch is uniform)
PT_HD f3 camera_ray_projected(const RenderParams& rp, const CameraView& cam, const ProjView& proj, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    return proj.kind == PROJ_PANORAMA ? camera_ray_panorama(rp, cam, proj, gx, gy, sample, origin)
                                      : camera_ray_orthographic(rp, cam, proj, gx, gy, sample, origin);
}

// ---- the camera kind as one axis.  A kernel that makes camera rays takes ONE camera argument whose type says which ray it makes: the
// pinhole's CameraView alone, or the view with the lens or the projection constants behind it (all float / uint32_t: the argument lays out as
// the pair of views would).  The host derives the kind from CameraOptics (camera_kind, pt_kernels.h) once per launch.
enum CameraKind : uint32_t { CAM_PINHOLE, CAM_LENS, CAM_PANORAMA, CAM_ORTHOGRAPHIC, CAM_KINDS, CAM_BY_VIEW = CAM_KINDS };
struct CameraLensView : CameraView { LensView lens; };
struct CameraProjView : CameraView { ProjView proj; };
template <uint32_t KIND>
using CameraArg = std::conditional_t<KIND == CAM_PINHOLE, CameraView, std::conditional_t<KIND == CAM_LENS, CameraLensView, CameraProjView>>;

// The camera ray of (pixel gx, gy; sample) by the type of `cam`: its direction, and its origin in *origin (the pinhole's and the panorama's is
// the eye).  KIND is read by the projection overload only: CAM_PANORAMA / CAM_ORTHOGRAPHIC where the caller was built for one of them (the
// panorama's two sincos_det are then not in the orthographic kernel), CAM_BY_VIEW to go by cam.proj.kind (launch-invariant: the branch is uniform)
template <uint32_t KIND = CAM_BY_VIEW>
PT_HD f3 primary_ray(const RenderParams& rp, const CameraView& cam, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    *origin = f3{cam.eye[0], cam.eye[1], cam.eye[2]};
    return camera_ray_dir(rp, cam, gx, gy, sample);
}
template <uint32_t KIND = CAM_BY_VIEW>
PT_HD f3 primary_ray(const RenderParams& rp, const CameraLensView& cam, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    return camera_ray(rp, cam, cam.lens, gx, gy, sample, origin);
}
template <uint32_t KIND = CAM_BY_VIEW>
PT_HD f3 primary_ray(const RenderParams& rp, const CameraProjView& cam, uint32_t gx, uint32_t gy, uint32_t sample, f3* origin)
{
    if (KIND == CAM_PANORAMA) return camera_ray_panorama(rp, cam, cam.proj, gx, gy, sample, origin);
    if (KIND == CAM_ORTHOGRAPHIC) return camera_ray_orthographic(rp, cam, cam.proj, gx, gy, sample, origin);
    return camera_ray_projected(rp, cam, cam.proj, gx, gy, sample, origin);
}

} // namespace pt
