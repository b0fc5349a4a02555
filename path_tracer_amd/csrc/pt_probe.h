// The sample direction of an irradiance probe and the real spherical harmonics of bands 0-2 in it: one definition for the gfx950 kernels
// (k_probe_rays, k_probe_project) and for the host evaluation (pt_probe_ray).  include/pt_api.h, pt_bake_probes, states it operation for
// operation; every operation is rounded once, in this order (the library is built without contraction).
#pragma once
#include "pt_types.h"
#include "pt_materials.h"

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

// ---- reflection probes (pt_set_probe_grid_radiance; include/pt_api.h states all of it operation for operation)
// The unit direction of the centre of texel `texel` of an R x R octahedral map, the inverse of probe_oct_texel there, and the texel's relative
// solid angle omega = 1 / |v|^3, v the centre's point on the unit octahedron (the map's area element is dA / |v|^3; the fold is an isometry).
PT_HD void probe_oct_dir(uint32_t texel, uint32_t R, float dir[3], float* omega)
{
    const uint32_t iy = texel / R, ix = texel - iy * R;
    const float fr = (float)R;
    float px = 2.0f * (((float)ix + 0.5f) / fr) - 1.0f, py = 2.0f * (((float)iy + 0.5f) / fr) - 1.0f;
    const float z = (1.0f - fabsf(px)) - fabsf(py);
    if (z < 0.0f)
    {
        const float qx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f), qy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = qx;
        py = qy;
    }
    const float len = sqrtf((px * px + py * py) + z * z);
    dir[0] = px / len;
    dir[1] = py / len;
    dir[2] = z / len;
    *omega = 1.0f / ((len * len) * len);
}
// what the prefilter reads of input texel j: {mean r, g, b, filled}: sums / (float)count, one division per channel; an empty texel is zeros
PT_HD f4 probe_radiance_mean(const float sums[3], uint32_t count)
{
    if (count == 0u) return f4{0.0f, 0.0f, 0.0f, 0.0f};
    const float n = (float)count;
    return f4{sums[0] / n, sums[1] / n, sums[2] / n, 1.0f};
}
// Output texel i of one probe's map prefiltered by the GGX lobe of `alpha` around the texel's own direction (V = N = R): a quadrature over the
// rr input texels in ascending order.  dirw[j] = {probe_oct_dir(j), omega_j}, mean[j] = probe_radiance_mean of texel j.  One function for the
// host evaluation and k_probe_radiance_prefilter, whose lanes read dirw and mean from LDS, every lane the same j at a time.
PT_HD f4 probe_prefilter_texel(const f4* dirw, const f4* mean, uint32_t rr, float alpha, uint32_t i)
{
    const f4 ni = dirw[i];
    const f3 n{ni.x, ni.y, ni.z};
    float A[3] = {0.0f, 0.0f, 0.0f}, Wt = 0.0f;
    for (uint32_t j = 0; j < rr; ++j)
    {
        const f4 m = mean[j];
        if (m.w == 0.0f) continue;
        const f4 lj = dirw[j];
        const f3 l{lj.x, lj.y, lj.z};
        const float nl = dot3(n, l);
        if (!(nl > 0.0f)) continue;
        const f3 h = unit3(n + l);
        float nh = dot3(n, h);
        nh = nh > 1.0f ? 1.0f : nh; // (rounding takes the cosine of j = i past 1, where ggx_d's sqrtf(1 - c2) is a NaN)
        const float w = (ggx_d(alpha, f3{h.x, h.y, nh}) * nl) * lj.w;
        A[0] = A[0] + w * m.x;
        A[1] = A[1] + w * m.y;
        A[2] = A[2] + w * m.z;
        Wt = Wt + w;
    }
    if (!(Wt > 0.0f)) return f4{0.0f, 0.0f, 0.0f, 0.0f};
    return f4{A[0] / Wt, A[1] / Wt, A[2] / Wt, 0.0f};
}

// The specular lookup (pt_probe_grid_specular): the prefiltered radiance the grid's reflection probes hold in the direction of the mirror
// reflection of `incoming` about n, at roughness a.  The texel is the nearest one, computed once; the level pair and its blend t come from a;
// the corner weights are probe_grid_lookup<VIS>'s, restated here so that the existing instantiations stay what they are.  Returns lit; *out is
// S / W where lit and 0 where not.  No index leaves the tables whatever p, n, incoming and a are.
template <bool VIS = false>
PT_HD bool probe_grid_specular(const ProbeGridView& g, const ProbeRadianceView& rv, f3 p, f3 n, f3 incoming, float a, f3* out, const ProbeDepthView* dv = nullptr)
{
    const float pp[3] = {p.x + g.bias * n.x, p.y + g.bias * n.y, p.z + g.bias * n.z};
    uint32_t i0[3], i1[3];
    float f[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
    {
        float x = (pp[ax] - g.origin[ax]) / g.cell[ax];
        const float top = (float)(g.count[ax] - 1u);
        x = !(x > 0.0f) ? 0.0f : (x > top ? top : x);
        i0[ax] = (uint32_t)x;
        f[ax] = x - truncf(x);
        i1[ax] = i0[ax] + 1u < g.count[ax] ? i0[ax] + 1u : i0[ax];
    }
    const f3 r = reflect_rs(incoming, n);
    const float rd[3] = {r.x, r.y, r.z};
    const uint32_t rr = rv.res * rv.res, texel = probe_oct_texel(rd, rv.res);
    // the level: l the last one with alpha[l] <= a (a clamped into the levels' range, a NaN to the lowest), hi the next one's alpha
    uint32_t l = 0u;
    float lo = rv.alpha[0], hi = rv.alpha[0];
    bool at_top = true;
    if (!(a > lo)) a = lo;
#pragma unroll
    for (uint32_t k = 1u; k < 8u; ++k)
        if (k < rv.n_levels)
        {
            if (rv.alpha[k] <= a) { l = k; lo = rv.alpha[k]; }
            else if (at_top) { hi = rv.alpha[k]; at_top = false; }
        }
    const float t = at_top ? 0.0f : (a - lo) / (hi - lo), t1 = 1.0f - t;
    const uint32_t l1 = at_top ? l : l + 1u;
    float W = 0.0f, S[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)
    {
        const uint32_t cx = (k & 1u) ? i1[0] : i0[0], cy = (k & 2u) ? i1[1] : i0[1], cz = (k & 4u) ? i1[2] : i0[2];
        const uint32_t node = (cz * g.count[1] + cy) * g.count[0] + cx;
        const float wx = (k & 1u) ? f[0] : 1.0f - f[0], wy = (k & 2u) ? f[1] : 1.0f - f[1], wz = (k & 4u) ? f[2] : 1.0f - f[2];
        float w = ((wx * wy) * wz) * (g.nodes[node].valid != 0.0f ? 1.0f : 0.0f);
        if (VIS)
        {
            const DProbeDepth mcur = probe_corner_moments(g, *dv, pp, cx, cy, cz, node);
            float v[3];
            probe_corner_vector(g, pp, cx, cy, cz, v);
            const float dist = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            const float var = fabsf(mcur.m2 - mcur.m1 * mcur.m1), dl = dist - mcur.m1;
            const float ch = var / (var + dl * dl), c3 = (ch * ch) * ch;
            const float vis = dist > mcur.m1 ? (c3 > dv->vis_floor ? c3 : dv->vis_floor) : 1.0f;
            w = w * vis;
            if (dv->facing)
            {
                const float cs = ((v[0] * n.x + v[1] * n.y) + v[2] * n.z) / dist, hh = (1.0f - cs) * 0.5f;
                w = w * (dist > 0.0f ? hh * hh + 0.2f : 1.0f);
            }
        }
        const size_t base = (size_t)node * rv.n_levels;
        const f4 T0 = rv.table[(base + l) * rr + texel], T1 = rv.table[(base + l1) * rr + texel];
        S[0] = S[0] + w * (t1 * T0.x + t * T1.x);
        S[1] = S[1] + w * (t1 * T0.y + t * T1.y);
        S[2] = S[2] + w * (t1 * T0.z + t * T1.z);
        W = W + w;
    }
    const bool lit = W > 0.0f;
    *out = lit ? f3{S[0] / W, S[1] / W, S[2] / W} : f3{0.0f, 0.0f, 0.0f};
    return lit;
}

} // namespace pt
