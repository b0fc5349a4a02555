// The sample direction of an irradiance probe and the real spherical harmonics of bands 0-2 in it: one definition for the gfx950 kernels
// (k_probe_rays, k_probe_project) and for the host evaluation (pt_probe_ray).  include/pt_api.h, pt_bake_probes, states it operation for
// operation; every operation is rounded once, in this order (the library is built without contraction).
#pragma once
#include "pt_types.h"

namespace pt {

// y0..y8 of direction d (used as given, not renormalised)
PT_HD void probe_sh9(const float d[3], float y[9])
{
    const float x = d[0], yy = d[1], z = d[2];
    y[0] = 0.2820948f;
    y[1] = 0.48860252f * yy;
    y[2] = 0.48860252f * z;
    y[3] = 0.48860252f * x;
    y[4] = 1.0925484f * (x * yy);
    y[5] = 1.0925484f * (yy * z);
    y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
    y[7] = 1.0925484f * (x * z);
    y[8] = 0.54627424f * (x * x - yy * yy);
}

// direction of sample `sample` of the probe whose stream is pixel `key`: the uniform sphere map of the Sobol point seeded by the stream's
// draw 0 (as a camera ray's jitter, main.rs:193-194).  ONE draw of the stream is consumed.
PT_HD void probe_ray(uint64_t seed, uint32_t n_sobol, uint32_t key, uint32_t sample, float d[3], float y[9])
{
    Stream rng{stream_key(seed, key, sample), 0u};
    const uint32_t seed0 = rng.u32();
    float u1, u2;
    ss_sobol(n_sobol, sample, seed0, &u1, &u2);
    const float z = 1.0f - 2.0f * u1;
    const float r2 = 1.0f - z * z;
    const float r = sqrtf(r2 > 0.0f ? r2 : 0.0f);
    const float phi = 6.2831855f * u2;
    float sn, cs;
    sincos_det(phi, &sn, &cs);
    d[0] = r * cs;
    d[1] = r * sn;
    d[2] = z;
    probe_sh9(d, y);
}

} // namespace pt
