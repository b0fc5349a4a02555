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

// ---- probe visibility (pt_set_probe_grid_depth; include/pt_api.h states all of it operation for operation)
// The texel of direction v (used as given, not normalised: the map is scale-free) in an R x R octahedral map.  A NaN lands on texel 0.
PT_HD uint32_t probe_oct_texel(const float v[3], uint32_t R)
{
    const float s = (fabsf(v[0]) + fabsf(v[1])) + fabsf(v[2]);
    float px = v[0] / s, py = v[1] / s;
    if (v[2] < 0.0f)
    {
        const float qx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f), qy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = qx;
        py = qy;
    }
    const float u = px * 0.5f + 0.5f, w = py * 0.5f + 0.5f, fr = (float)R;
    const float ur = u * fr, wr = w * fr; // in [0, R] or NaN
    const uint32_t ix = !(ur > 0.0f) ? 0u : ((uint32_t)ur < R - 1u ? (uint32_t)ur : R - 1u);
    const uint32_t iy = !(wr > 0.0f) ? 0u : ((uint32_t)wr < R - 1u ? (uint32_t)wr : R - 1u);
    return iy * R + ix;
}
// v = P' - Q of the node (ix, iy, iz), Q_a = origin_a + (float)i_a * cell_a
PT_HD void probe_corner_vector(const ProbeGridView& g, const float pp[3], uint32_t ix, uint32_t iy, uint32_t iz, float v[3])
{
    v[0] = pp[0] - (g.origin[0] + (float)ix * g.cell[0]);
    v[1] = pp[1] - (g.origin[1] + (float)iy * g.cell[1]);
    v[2] = pp[2] - (g.origin[2] + (float)iz * g.cell[2]);
}
// the moments node `node` = (ix, iy, iz) holds in the direction of P' (the index stays inside the node's R * R texels whatever P' is)
PT_HD DProbeDepth probe_corner_moments(const ProbeGridView& g, const ProbeDepthView& dv, const float pp[3], uint32_t ix, uint32_t iy, uint32_t iz, uint32_t node)
{
    float v[3];
    probe_corner_vector(g, pp, ix, iy, iz, v);
    return dv.moments[(size_t)node * (dv.res * dv.res) + probe_oct_texel(v, dv.res)];
}

// The probe grid's lookup (pt_set_probe_grid; the definition is include/pt_api.h's, operation for operation): the irradiance over pi that the
// grid's SH9 radiance probes give a surface at p with normal n, trilinear over the cell's eight corners with the invalid ones left out and
// the rest renormalised.  Each corner is EVALUATED before it is blended: three running sums instead of 27 blended coefficients, and a corner
// is seven 16-byte loads that are issued one corner ahead of the arithmetic.  Returns lit (some valid corner has weight); *out is the clamped
// I where lit and 0 where not.  No index leaves the grid whatever p is (a NaN coordinate lands on node 0 of its axis).
// Shared by the baked view's probe ending, the unit hook's kernel and the hook's host evaluation.
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_PROBE_PIN(a, b, c, d) __asm__ volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : : "memory")
#else
#define PT_PROBE_PIN(a, b, c, d) ((void)0)
#endif
// VIS (pt_set_probe_grid_depth): every corner's weight is multiplied by the Chebyshev visibility of P' from the node, read from the node's
// depth moments in the texel of the direction node -> P', and with PT_PROBE_VIS_FACING by a factor that prefers nodes the surface faces.
// The moments of a corner are one 8-byte load whose address depends on P' alone: it is issued one corner ahead with the corner's record.
// Without VIS the function is what it was, operation for operation (dv is not read).
template <bool VIS = false>
PT_HD bool probe_grid_lookup(const ProbeGridView& g, f3 p, f3 n, f3* out, const ProbeDepthView* dv = nullptr)
{
    const float pp[3] = {p.x + g.bias * n.x, p.y + g.bias * n.y, p.z + g.bias * n.z};
    uint32_t i0[3], i1[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
        float x = (pp[a] - g.origin[a]) / g.cell[a];
        const float top = (float)(g.count[a] - 1u);
        x = !(x > 0.0f) ? 0.0f : (x > top ? top : x);
        i0[a] = (uint32_t)x;
        f[a] = x - truncf(x);
        i1[a] = i0[a] + 1u < g.count[a] ? i0[a] + 1u : i0[a];
    }
    const float d[3] = {n.x, n.y, n.z};
    float yc[9];
    probe_sh9(d, yc);
#pragma unroll
    for (int m = 1; m < 4; ++m) yc[m] = 0.6666667f * yc[m];
#pragma unroll
    for (int m = 4; m < 9; ++m) yc[m] = 0.25f * yc[m];
    const uint32_t row[2] = {i0[2] * g.count[1], i1[2] * g.count[1]};
    const uint32_t line[4] = {(row[0] + i0[1]) * g.count[0], (row[0] + i1[1]) * g.count[0], (row[1] + i0[1]) * g.count[0], (row[1] + i1[1]) * g.count[0]};
    float W = 0.0f, E[3] = {0.0f, 0.0f, 0.0f};
    DProbe r = g.nodes[line[0] + i0[0]];
    DProbeDepth mr{};
    if (VIS) mr = probe_corner_moments(g, *dv, pp, i0[0], i0[1], i0[2], line[0] + i0[0]);
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
    {
        const DProbe cur = r;
        const DProbeDepth mcur = mr;
        if (k < 7u)
        {
            const uint32_t node = line[(k + 1u) >> 1] + (((k + 1u) & 1u) ? i1[0] : i0[0]);
            r = g.nodes[node];
            if (VIS) mr = probe_corner_moments(g, *dv, pp, ((k + 1u) & 1u) ? i1[0] : i0[0], ((k + 1u) & 2u) ? i1[1] : i0[1], ((k + 1u) & 4u) ? i1[2] : i0[2], node);
        }
        const float wx = (k & 1u) ? f[0] : 1.0f - f[0], wy = (k & 2u) ? f[1] : 1.0f - f[1], wz = (k & 4u) ? f[2] : 1.0f - f[2];
        float w = ((wx * wy) * wz) * (cur.valid != 0.0f ? 1.0f : 0.0f);
        if (VIS)
        {
            float v[3];
            probe_corner_vector(g, pp, (k & 1u) ? i1[0] : i0[0], (k & 2u) ? i1[1] : i0[1], (k & 4u) ? i1[2] : i0[2], v);
            const float rr = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            const float var = fabsf(mcur.m2 - mcur.m1 * mcur.m1), dl = rr - mcur.m1;
            const float ch = var / (var + dl * dl), c3 = (ch * ch) * ch;
            const float vis = rr > mcur.m1 ? (c3 > dv->vis_floor ? c3 : dv->vis_floor) : 1.0f; // (a NaN c3 is never selected)
            w = w * vis;
            if (dv->facing)
            {
                const float cs = ((v[0] * n.x + v[1] * n.y) + v[2] * n.z) / rr, h = (1.0f - cs) * 0.5f;
                w = w * (rr > 0.0f ? h * h + 0.2f : 1.0f);
            }
        }
        W = k ? W + w : w;
#pragma unroll
        for (int c = 0; c < 3; ++c)
        {
            float e = yc[0] * cur.sh[c] + yc[1] * cur.sh[3 + c];
#pragma unroll
            for (int m = 2; m < 9; ++m) e = e + yc[m] * cur.sh[3 * m + c];
            E[c] = k ? E[c] + w * e : w * e;
        }
        PT_PROBE_PIN(W, E[0], E[1], E[2]);
    }
    const bool lit = W > 0.0f;
    float I[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
    {
        const float v = E[c] / W;
        I[c] = lit && v > 0.0f ? v : 0.0f;
    }
    *out = f3{I[0], I[1], I[2]};
    return lit;
}

} // namespace pt
