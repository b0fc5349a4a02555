// CPU-only driver of libptmi's HOST code (pt_scene.cpp: OBJ reader, SAH / agglomerative builders, flattening, camera; pt_png.cpp: PNG
// encoder) for the sanitizer build `make -C path_tracer_amd/csrc host-asan` (g++ -fsanitize=address,undefined; no HIP involved: GPU
// ASan does not exist on this pool, and these files are where user-supplied bytes enter the library).  tests/test_host_sanitizer.py
// feeds it valid, malformed and byte-mutated OBJ files and a camera random walk; any sanitizer report fails the test.
//   host_sanitize obj <file>...        Model::new(path) + Scene::new for each file (parse errors are an expected outcome)
//   host_sanitize walk <events> <seed> Camera::input random walk with create_ray after every event
//   host_sanitize png <w> <h> <file>   encode a test image
//   host_sanitize soup <n> <seed>      Scene::new over n random triangles (PTMI_BUILD_THREADS forks the SAH sweep: also built with
//                                      -fsanitize=thread by `make host-tsan`); prints a checksum of the BLAS arena
//   host_sanitize moves <n> <seed>     pt_set_instances' host side: n random moves (translations, quarter turns, instance counts 0..3) of the models
//                                      of a small scene, an incremental build after each; the flattened scene must equal, byte for byte, the one
//                                      a scene built from nothing with the same matrices flattens to; prints how many builds kept the BLAS part
//   host_sanitize plan <row>...        pt_batch_plan.h: each row "b:free,held,classes,volumes" (max_paths_for) or
//                                      "p:n_samples,act_pixels,samples_out,pipelines,batch_spp,lds_scene,max_paths,cap0,cap1,cap2,cap3"
//                                      (plan_batches); prints a JSON list: max_paths, or [batch, n_batches, n_pipes] ([0, 0, 0]: refused)
//   host_sanitize normals <n> <seed>   normal maps' host side: n random triangles with random UVs (degenerate, huge and mirrored ones among them) under a
//                                      normal texture, Scene::new, then shading_normal (pt_materials.h) at random hits over the flattened tables;
//                                      prints how many triangles got a tangent and a checksum of the normals
//   host_sanitize roughness <n> <seed> roughness maps' host side: the setter's refusals (kinds that are not GGX, bad indices: nothing changes), then n
//                                      random triangles with mirrored, negative, exactly-1 and 1e6 UVs under a 5 x 3 map, a model without UVs under a
//                                      1 x 1 map and one under an 8 x 4 map, and surface_alpha (pt_materials.h) at random hits: every map's values lie in
//                                      a range of its own and no alpha may leave its map's; clearing the maps gives the never-mapped scene's bytes
//   host_sanitize lightmaps <n> <seed> lightmaps' host side: n random triangles with random UVs (far outside [0, 1], huge, mirrored and overflowing ones
//                                      among them) under three placements, random maps of several sizes on two of them, then lightmap_lookup
//                                      (pt_materials.h) at random hits; prints how many lookups met a map and a checksum of the results
//   host_sanitize lightmaps_dir <n> <seed> directional lightmaps' host side: the same hostile UVs under a normal texture and three placements; gradients by
//                                      lm_gradient (pt_lightmap.h) from random first-moment sums, denormal ones and zero normals among them, in tables
//                                      that fill their allocation exactly; then lightmap_lookup_directional (pt_materials.h) under shading_normal_delta
//                                      at random hits; prints the lookups and a checksum (nonzero exit for a negative or NaN result)
//   host_sanitize lightmap_direct <n> <seed> direct light sampled at the texel: lm_light_sample (pt_lightmap.h, the function the kernels run) and the host
//                                      fold of X = G + D over n random texels and four designed ones, against light tables that fill their
//                                      allocations exactly: a light point exactly at o, cosl == 0, a zero-area light triangle (weight 0 when n is
//                                      odd), a cdf that ends below 1 so that a draw lands past the last entry, and x == 1.0; no index leaves its
//                                      table and no D is negative, a NaN or longer than 100 (nonzero exit otherwise); prints counts and a checksum
//   host_sanitize texelfilter <n> <seed> the texel filter's host side (pt_lightmap_filter.h, the functions the kernels run): n random triangles with the
//                                      same hostile UVs, their texel tables on maps from 1 x 1 up, sides that are no multiple of 16 among them, random
//                                      positive sums, then the whole filter with 8 levels (step 128 exceeds every map), with and without second
//                                      moments, under the default reach, a tiny one and one whose square overflows; prints a checksum of the means
//   host_sanitize screenfilter <seed>  the a-trous core (pt_filter.h: spatial_variance, atrous_level) under the screen rule: random images of 1 x 1,
//                                      5 x 3, 16 x 16 and 37 x 19 pixels with miss pixels, invalid pixels and two models, the 7 x 7 variance and
//                                      8 levels (step 128 leaves every map); then the rules' defining property: with one model, every pixel a valid
//                                      hit and reach2 = +inf the texel rule gives the screen rule's bits (nonzero exit if not); prints a checksum
//   host_sanitize probegrid <n> <seed> the probe grid's host side: random grids of 1 x 1 x 1, 2 x 2 x 2, 3 x 2 x 4, 5 x 1 x 3 and two with a single line of
//                                      nodes, a fifth of the nodes invalid, then probe_grid_lookup (pt_probe.h, the function the kernels run) at n
//                                      points each: inside, far outside, huge, infinite and NaN positions, NaN normals; prints how many were lit and
//                                      a checksum of the results
//   host_sanitize probedepth <n> <seed> probe visibility's host side: the same grids, each with a random depth table of side 2..16 that fills its
//                                      allocation exactly, random flags and floor, then probe_grid_lookup<true> at the same kinds of points, and
//                                      probe_oct_texel alone over zero, huge, infinite and NaN directions; prints how many were lit, a checksum
//                                      and the largest texel seen against the map's size
//   host_sanitize proberadiance <n> <seed> reflection probes' host side: the same grids, each with raw radiance maps of side 2..16 with empty texels
//                                      (every third probe empty altogether) run through probe_prefilter_texel at 1..8 levels into a table that
//                                      fills its allocation exactly, then probe_grid_specular with and without a random depth table at the same
//                                      kinds of points, with zero, huge, infinite and NaN directions and alphas; probe_oct_dir's round trip
//                                      through probe_oct_texel; prints how many were lit, checksums, and whether every filtered value was finite
//   host_sanitize queues <seed>        pt_queue_plan.h, the integer arithmetic under the hot kernels, swept over ray counts 1..4200, every 2^k - 1, 2^k, 2^k + 1
//                                      below 2^29 and log-uniform ones: (P1) the static ranges and the accepted claims of fetch_plan / chunk_of / claim_range
//                                      cover [0, n) exactly once for every grid, waves per workgroup, chunk divisor and taper; (P2) the striped regions of
//                                      stripes_for are disjoint, stripe_valid and stripe_extent agree with what producers reserved, a region past the capacity
//                                      is refused; (P3) region_size's bounds; (P4) fastdiv against `/`; (P5) pid_split / pid_join are inverse bijections
//                                      under pid_block_layout.  Prints one JSON line of counts; nonzero exit on the first few failures (stderr names them)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt_batch_plan.h"
#include "pt_lightmap_filter.h"
#include "pt_materials.h"
#include "pt_png.h"
#include "pt_probe.h"
#include "pt_queue_plan.h"
#include "pt_scene.h"

using namespace pt;

static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

static int light_scene(HostScene& sc)
{
    const float white[3] = {0.7f, 0.7f, 0.7f}, emit[3] = {10.0f, 10.0f, 10.0f}, zero[3] = {0, 0, 0};
    const int m0 = sc.add_material(0, white, 0.0f, 1.0f, false, zero, 0, 0, 0);
    const int m1 = sc.add_material(1, emit, 0.0f, 1.0f, false, zero, 0, 0, 0);
    const float quad[18] = {-50, 300, -50, 50, 300, -50, 50, 300, 50, -50, 300, -50, 50, 300, 50, -50, 300, 50};
    const float nrm[18] = {0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1, 0};
    if (sc.add_model(quad, nrm, 2, m1, kIdentity, 1) < 0) return -1;
    return m0;
}

// screenfilter's walk: the 7 x 7 variance (pass 0), then k.iterations levels, of prepared images under the rule make(i) builds for centre i
template <class MakeRule>
static std::vector<f4> core_filter_host(int w, int h, const DenoiseK& k, std::vector<f4> cv, const f4* pos, const f4* nv, MakeRule make)
{
    std::vector<f4> other(cv.size());
    for (uint32_t pass = 0; pass <= k.iterations; ++pass)
    {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
            {
                const size_t i = (size_t)y * w + x;
                const f4 c = cv[i];
                if (nv[i].w == 0.0f) other[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
                else if (pass == 0) other[i] = f4{c.x, c.y, c.z, spatial_variance(make(i), w, h, k, cv.data(), pos, nv, x, y)};
                else other[i] = atrous_level(make(i), w, h, 1 << (pass - 1), k, cv.data(), pos, nv, x, y);
            }
        std::swap(cv, other);
    }
    return cv;
}

#include "host_sanitize_queues.h"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "obj")
    {
        int parsed = 0, rejected = 0;
        for (int i = 2; i < argc; ++i)
        {
            HostScene sc;
            const int mat = light_scene(sc);
            if (mat < 0) return 3;
            std::string err;
            const int r = sc.add_model_obj(argv[i], mat, kIdentity, 1, &err);
            if (r < 0) { ++rejected; continue; }
            if (sc.build(&err) != 0) { ++rejected; continue; }
            const float eye[3] = {0, 50, 1000}, tgt[3] = {0, 50, 0};
            sc.set_camera(eye, tgt, 60.0f, 1.5f);
            float o[3], d[3];
            sc.create_ray(0.25f, 0.75f, o, d);
            ++parsed;
        }
        std::printf("{\"parsed\": %d, \"rejected\": %d}\n", parsed, rejected);
        return 0;
    }
    if (cmd == "walk" && argc >= 4)
    {
        HostScene sc;
        const float eye[3] = {0, 50, 1000}, tgt[3] = {0, 50, 0};
        sc.set_camera(eye, tgt, 60.0f, 16.0f / 9.0f);
        uint64_t s = std::strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        double acc = 0;
        for (int e = 0, n = std::atoi(argv[2]); e < n; ++e)
        {
            const float dt = 1e-6f + rnd() * 5e-6f;
            switch ((int)(rnd() * 5.0f) % 5)
            {
            case 0: sc.camera_rotate(rnd() * 8.0f - 4.0f, rnd() * 8.0f - 4.0f, dt); break;
            case 1: sc.camera_move(0.0f, 1.0f, dt); break;
            case 2: sc.camera_move(0.0f, -1.0f, dt); break;
            case 3: sc.camera_move(-1.0f, 0.0f, dt); break;
            default: sc.camera_move(1.0f, 0.0f, dt); break;
            }
            float o[3], d[3], m[16];
            sc.create_ray(rnd(), rnd(), o, d);
            sc.inv_projection(m);
            acc += d[0] + d[1] + d[2] + m[5];
        }
        std::printf("{\"checksum\": %.6f}\n", acc);
        return 0;
    }
    if (cmd == "soup" && argc >= 4)
    {
        HostScene sc;
        const int mat = light_scene(sc);
        if (mat < 0) return 3;
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = std::strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        std::vector<float> p((size_t)n * 9), nr((size_t)n * 9, 0.0f);
        for (uint32_t i = 0; i < n; ++i)
        {
            const float c[3] = {rnd() * 200.0f - 100.0f, rnd() * 200.0f - 100.0f, rnd() * 200.0f - 100.0f};
            for (int k = 0; k < 9; ++k) p[(size_t)i * 9 + k] = c[k % 3] + rnd() * 4.0f - 2.0f;
            for (int k = 0; k < 3; ++k) nr[(size_t)i * 9 + k * 3 + 1] = 1.0f;
        }
        if (sc.add_model(p.data(), nr.data(), n, mat, kIdentity, 1) < 0) return 4;
        std::string err;
        if (sc.build(&err) != 0) { std::printf("{\"error\": \"%s\"}\n", err.c_str()); return 0; }
        const HostBlas& b = sc.blas.back();
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](uint32_t v) { h = (h ^ v) * 1099511628211ull; };
        for (const HostNode& nd : b.nodes)
        {
            uint32_t w[6];
            std::memcpy(w, &nd.box, sizeof(w));
            for (uint32_t v : w) mix(v);
            mix(nd.kind); mix(nd.a); mix(nd.b);
        }
        for (uint32_t v : b.prim_ids) mix(v);
        std::printf("{\"nodes\": %zu, \"depth\": %u, \"arena\": \"%016llx\"}\n", b.nodes.size(), b.depth, (unsigned long long)h);
        return 0;
    }
    if (cmd == "moves" && argc >= 4)
    {
        uint64_t s = std::strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        // the light of light_scene, a soup with leaves of several sizes and a quad
        std::vector<float> p(400 * 9), nr(400 * 9, 0.0f);
        for (size_t i = 0; i < 400; ++i)
        {
            const float c[3] = {rnd() * 200.0f - 100.0f, rnd() * 200.0f - 100.0f, rnd() * 200.0f - 100.0f};
            for (int k = 0; k < 9; ++k) p[i * 9 + k] = c[k % 3] + rnd() * 4.0f - 2.0f;
            for (int k = 0; k < 3; ++k) nr[i * 9 + k * 3 + 1] = 1.0f;
        }
        const float quad[18] = {-80, 0, -80, 80, 0, -80, 80, 0, 80, -80, 0, -80, 80, 0, 80, -80, 0, 80};
        std::vector<std::vector<float>> mats(3, std::vector<float>(kIdentity, kIdentity + 12));
        auto make = [&](HostScene& sc) -> bool {
            const int mat = light_scene(sc);
            if (mat < 0 || sc.add_model(p.data(), nr.data(), 400, mat, kIdentity, 1) < 0 || sc.add_model(quad, nr.data(), 2, mat, kIdentity, 1) < 0) return false;
            return true;
        };
        HostScene moved;
        std::string err;
        if (!make(moved) || moved.build(&err) != 0) return 3;
        auto same = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); };
        int kept = 0;
        for (int e = 0, n = std::atoi(argv[2]); e < n; ++e)
        {
            const int model = (int)(rnd() * 3.0f) % 3;
            const uint32_t count = rnd() < 0.7f ? (uint32_t)(mats[model].size() / 12) : (uint32_t)(rnd() * 4.0f) % 4u;
            std::vector<float> m;
            for (uint32_t i = 0; i < count; ++i)
            {
                static const float turn[12] = {0, 0, 1, 0, 0, 1, 0, 0, -1, 0, 0, 0};
                const float* rot = rnd() < 0.5f ? kIdentity : turn;
                for (int k = 0; k < 12; ++k) m.push_back(k % 4 == 3 ? std::floor(rnd() * 100.0f) - 50.0f : rot[k]);
            }
            if (model == 0 && count == 0) continue; // (keep a light: nothing here depends on it, the scene stays the usual kind)
            const uint64_t epoch = moved.layout_epoch;
            if (moved.set_instances(model, m.data(), count) != 0 || moved.build(&err) != 0) return 4;
            kept += moved.layout_epoch == epoch ? 1 : 0;
            mats[model] = m;
            HostScene fresh;
            if (!make(fresh)) return 3;
            for (int k = 0; k < 3; ++k)
                if (fresh.set_instances(k, mats[k].data(), (uint32_t)(mats[k].size() / 12)) != 0) return 5;
            if (fresh.build(&err) != 0) return 6;
            const FlatScene &a = moved.flat, &b = fresh.flat;
            const bool ok = same(a.nodes, b.nodes) && same(a.tri_isect, b.tri_isect) && same(a.tri_shade, b.tri_shade) && same(a.tri_pos, b.tri_pos) &&
                            same(a.tri_orig, b.tri_orig) && same(a.instances, b.instances) && same(a.big_leaves, b.big_leaves) && same(a.materials, b.materials) &&
                            same(a.lights, b.lights) && same(a.tri_base, b.tri_base) && same(a.inst_base, b.inst_base) && a.world_root == b.world_root &&
                            a.lights_root == b.lights_root && a.prim_bits == b.prim_bits && a.stack_entries == b.stack_entries && a.ident_tlas == b.ident_tlas &&
                            std::memcmp(&a.light_weight_sum, &b.light_weight_sum, 4) == 0 && a.has_volumes == b.has_volumes;
            if (!ok) { std::printf("{\"error\": \"move %d: the incremental build differs from a build from nothing\"}\n", e); return 7; }
        }
        std::printf("{\"moves\": %d, \"kept_blas_part\": %d, \"blas_builds\": %llu}\n", std::atoi(argv[2]), kept, (unsigned long long)moved.blas_builds);
        return 0;
    }
    if (cmd == "normals" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        HostScene sc;
        const int mat = light_scene(sc);
        if (mat < 0 || n == 0) return 3;
        std::vector<float> p, nr, uv, texels;
        for (uint32_t t = 0; t < n; ++t)
        {
            const float c[3] = {200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) { p.push_back(c[k] + 10.0f * rnd() - 5.0f); nr.push_back(k == 1 ? 1.0f : 0.2f * rnd() - 0.1f); }
            const uint32_t shape = t % 5u; // general, all equal, collinear, around 1e6, mirrored
            const float a[2] = {4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 2; ++k)
                    uv.push_back(shape == 1u ? a[k] : shape == 2u ? a[0] + 0.25f * (float)v : shape == 3u ? 1.0e6f + 3.0f * rnd() : (shape == 4u && v ? -1.0f : 1.0f) * (a[k] + rnd()));
        }
        for (int k = 0; k < 5 * 3; ++k) { texels.push_back(rnd()); texels.push_back(rnd()); texels.push_back(0.5f + 0.5f * rnd()); }
        const int model = sc.add_model(p.data(), nr.data(), n, mat, kIdentity, 1);
        const int tex = sc.add_texture(5, 3, texels.data());
        if (model < 0 || tex < 0 || sc.set_model_uvs(model, uv.data(), n) != 0) return 4;
        if (sc.set_material_normal_texture(1, tex) != -1 || sc.set_material_normal_texture(mat, 7) != -1 || sc.set_material_normal_texture(mat, tex) != 0) return 5;
        std::string err;
        if (sc.build(&err) != 0) { std::printf("{\"error\": \"%s\"}\n", err.c_str()); return 0; }
        const FlatScene& f = sc.flat;
        if (!f.has_normal_maps || f.tri_tan.size() != f.tri_orig.size() || f.tri_uv.size() != f.tri_orig.size()) return 6;
        uint32_t with_tangent = 0;
        for (const f4& t : f.tri_tan) with_tangent += (t.x != 0.0f || t.y != 0.0f || t.z != 0.0f) ? 1u : 0u;
        const TexNView tv = f.texn_view();
        double acc = 0.0;
        for (uint32_t q = 0; q < 4u * n; ++q)
        {
            const uint32_t inst = (uint32_t)(rnd() * 1.999f) % (uint32_t)sc.world.instances.size();
            const uint32_t mi = sc.world.instances[inst].model;
            const uint32_t tri = f.tri_base[mi] + (uint32_t)(rnd() * (float)sc.blas[mi].tris.size()) % (uint32_t)sc.blas[mi].tris.size();
            const float u = rnd(), v = rnd() * (1.0f - u);
            bool front;
            const f3 nn = shading_normal(f.tri_shade.data(), f.instances.data(), f.materials.data(), tv, inst, tri, u, v, f3{rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f}, front);
            if (std::isfinite(nn.x) && std::isfinite(nn.y) && std::isfinite(nn.z)) acc += nn.x + 2.0 * nn.y + 3.0 * nn.z + (front ? 1.0 : 0.0);
        }
        // clearing takes the tangents out again
        if (sc.set_material_normal_texture(mat, -1) != 0 || sc.build(&err) != 0 || !sc.flat.tri_tan.empty() || sc.flat.has_textures) return 7;
        std::printf("{\"triangles\": %u, \"with_tangent\": %u, \"checksum\": %.6f}\n", n, with_tangent, acc);
        return 0;
    }
    if (cmd == "roughness" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        HostScene sc;
        const int lam = light_scene(sc), light = 1;
        if (lam < 0 || n == 0) return 3;
        const float tint[3] = {0.9f, 0.8f, 0.7f}, zero[3] = {0, 0, 0};
        const int metal = sc.add_material(MAT_GGX_METAL, tint, 0.3f, 1.0f, false, zero, 0, 0, 0);
        const int glass = sc.add_material(MAT_GGX_DIELECTRIC, tint, 0.4f, 1.5f, false, zero, 0, 0, 0);
        const int mirror = sc.add_material(MAT_SPECULAR, tint, 0.0f, 1.0f, false, zero, 0, 0, 0);
        const int smooth = sc.add_material(MAT_DIELECTRIC, tint, 0.0f, 1.5f, false, zero, 0, 0, 0);
        const int metal2 = sc.add_material(MAT_GGX_METAL, tint, 0.2f, 1.0f, false, zero, 0, 0, 0);
        // three models: n triangles under a 5 x 3 map with hostile UVs (general, mirrored, negative, exactly 1, around 1e6), a few WITHOUT UVs
        // under a 1 x 1 map, a few under an 8 x 4 map.  Every map's r values lie in a range of its own (g and b are loud), so a texel that left
        // its texture shows in the alpha even where the sanitizer sees one allocation
        auto soup = [&](uint32_t tris, std::vector<float>& p, std::vector<float>& nr) {
            for (uint32_t t = 0; t < tris; ++t)
            {
                const float c[3] = {200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f};
                for (int v = 0; v < 3; ++v)
                    for (int k = 0; k < 3; ++k) { p.push_back(c[k] + 10.0f * rnd() - 5.0f); nr.push_back(k == 1 ? 1.0f : 0.2f * rnd() - 0.1f); }
            }
        };
        std::vector<float> p0, n0, p1, n1, p2, n2, uv0, uv2;
        soup(n, p0, n0); soup(7, p1, n1); soup(9, p2, n2);
        for (uint32_t t = 0; t < n; ++t)
        {
            const uint32_t shape = t % 5u;
            const float a[2] = {4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 2; ++k)
                    uv0.push_back(shape == 1u ? (v ? -1.0f : 1.0f) * (a[k] + rnd()) : shape == 2u ? -3.0f * rnd() : shape == 3u ? (float)((v + k) & 1) : shape == 4u ? 1.0e6f + 3.0f * rnd() : a[k] + rnd());
        }
        for (uint32_t t = 0; t < 9u * 6u; ++t) uv2.push_back(t % 3u == 0u ? 1.0f : 5.0f * rnd() - 2.5f);
        const float range[3][2] = {{0.1f, 0.2f}, {0.5f, 0.5f}, {0.8f, 0.9f}};
        auto map = [&](uint32_t w, uint32_t h, const float* r) {
            std::vector<float> texels;
            for (uint32_t k = 0; k < w * h; ++k) { texels.push_back(r[0] + (r[1] - r[0]) * rnd()); texels.push_back(50.0f); texels.push_back(1.0e6f); }
            return sc.add_texture(w, h, texels.data());
        };
        const int models[3] = {sc.add_model(p0.data(), n0.data(), n, metal, kIdentity, 1), sc.add_model(p1.data(), n1.data(), 7, glass, kIdentity, 1),
                               sc.add_model(p2.data(), n2.data(), 9, metal2, kIdentity, 1)};
        const int tex[3] = {map(5, 3, range[0]), map(1, 1, range[1]), map(8, 4, range[2])};
        if (models[0] < 0 || models[1] < 0 || models[2] < 0 || tex[0] < 0 || tex[1] < 0 || tex[2] < 0) return 4;
        if (sc.set_model_uvs(models[0], uv0.data(), n) != 0 || sc.set_model_uvs(models[2], uv2.data(), 9) != 0) return 4;
        std::string err;
        if (sc.build(&err) != 0) { std::printf("{\"error\": \"%s\"}\n", err.c_str()); return 0; }
        if (sc.flat.has_textures || !sc.flat.tri_uv.empty()) return 5; // textures nobody references: no textured scene
        const std::vector<DMaterial> never = sc.flat.materials, before = sc.materials;
        // the refusals: a kind that is not GGX, a bad material, a bad texture; each changes nothing and leaves the scene built
        const int refused[][2] = {{lam, tex[0]}, {light, tex[0]}, {mirror, tex[0]}, {smooth, tex[0]}, {lam, -1}, {light, -1}, {-1, tex[0]}, {99, tex[0]}, {metal, 3}, {metal, -2}, {glass, 99}};
        for (const auto& rf : refused)
            if (sc.set_material_roughness_texture(rf[0], rf[1]) != -1 || !sc.built || std::memcmp(sc.materials.data(), before.data(), before.size() * sizeof(DMaterial)) != 0) return 6;
        const int mats[3] = {metal, glass, metal2};
        for (int k = 0; k < 3; ++k)
            if (sc.set_material_roughness_texture(mats[k], tex[k]) != 0 || sc.built) return 7;
        const uint64_t blas_builds = sc.blas_builds;
        if (sc.build(&err) != 0 || sc.blas_builds != blas_builds) return 8;
        const FlatScene& f = sc.flat;
        if (!f.has_textures || f.has_normal_maps || f.tri_uv.size() != f.tri_orig.size() || !f.tri_tan.empty()) return 9;
        const TexView tv = f.tex_view();
        double acc = 0.0;
        uint32_t outside = 0, per_model[3] = {0, 0, 0};
        for (uint32_t q = 0; q < 4u * n + 64u; ++q)
        {
            const uint32_t inst = (uint32_t)(rnd() * 3.999f) % (uint32_t)sc.world.instances.size();
            const uint32_t mi = sc.world.instances[inst].model;
            const uint32_t tri = f.tri_base[mi] + (uint32_t)(rnd() * (float)sc.blas[mi].tris.size()) % (uint32_t)sc.blas[mi].tris.size();
            const uint32_t corner = q % 7u; // the vertices and an edge among the hits
            const float u = corner == 0u ? 1.0f : corner == 1u ? 0.0f : rnd(), v = corner < 2u ? 0.0f : corner == 2u ? 1.0f - u : rnd() * (1.0f - u);
            const float a = surface_roughness_at(f.instances.data(), f.materials.data(), tv, inst, tri, u, v);
            int k = -1;
            for (int j = 0; j < 3; ++j) if ((int)mi == models[j]) k = j;
            if (k < 0) { if (a != 0.0f) ++outside; continue; } // the light: not GGX
            ++per_model[k];
            const float lo = range[k][0] * range[k][0], hi = range[k][1] * range[k][1];
            if (!(a >= lo * 0.9999f && a <= hi * 1.0001f)) ++outside;
            acc += a;
        }
        if (outside) { std::printf("{\"error\": \"%u alphas outside their texture's range\"}\n", outside); return 10; }
        // clearing every map gives the bytes of the scene that never had one
        for (int k = 0; k < 3; ++k)
            if (sc.set_material_roughness_texture(mats[k], -1) != 0) return 11;
        if (sc.build(&err) != 0 || sc.flat.has_textures || !sc.flat.tri_uv.empty() || sc.flat.materials.size() != never.size() ||
            std::memcmp(sc.flat.materials.data(), never.data(), never.size() * sizeof(DMaterial)) != 0)
            return 12;
        const float own = surface_roughness_at(sc.flat.instances.data(), sc.flat.materials.data(), sc.flat.tex_view(), 1u, sc.flat.tri_base[models[0]], 0.25f, 0.25f);
        if (own != clamp_rs(sq(0.3f), 0.0001f, 0.9999f)) return 13;
        std::printf("{\"triangles\": %u, \"hits\": [%u, %u, %u], \"refused\": %zu, \"checksum\": %.6f}\n", n, per_model[0], per_model[1], per_model[2],
                    sizeof(refused) / sizeof(refused[0]), acc);
        return 0;
    }
    if (cmd == "lightmaps" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        HostScene sc;
        const int mat = light_scene(sc);
        if (mat < 0 || n == 0) return 3;
        std::vector<float> p, nr, uv;
        for (uint32_t t = 0; t < n; ++t)
        {
            const float c[3] = {200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) { p.push_back(c[k] + 10.0f * rnd() - 5.0f); nr.push_back(k == 1 ? 1.0f : 0.2f * rnd() - 0.1f); }
            const uint32_t shape = t % 6u; // inside, far outside, all equal, around 1e6, mirrored, the largest finite values (their differences overflow)
            const float a[2] = {rnd(), rnd()};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 2; ++k)
                    uv.push_back(shape == 0u ? rnd() : shape == 1u ? 40.0f * rnd() - 20.0f : shape == 2u ? a[k] : shape == 3u ? 1.0e6f + 3.0f * rnd()
                                 : shape == 4u ? (v ? -1.0f : 1.0f) * (a[k] + rnd()) : (rnd() < 0.5f ? -3.0e38f : 3.0e38f));
        }
        // three placements of the soup; a map of its own on the first two, sizes from one texel to a few hundred
        const float turn[12] = {0, 0, 1, 30, 0, 1, 0, -20, -1, 0, 0, 10};
        std::vector<float> mats(kIdentity, kIdentity + 12);
        mats.insert(mats.end(), turn, turn + 12);
        mats.insert(mats.end(), kIdentity, kIdentity + 12);
        mats[2 * 12 + 3] = 500.0f;
        const int model = sc.add_model(p.data(), nr.data(), n, mat, mats.data(), 3);
        if (model < 0 || sc.set_model_uvs(model, uv.data(), n) != 0) return 4;
        std::string err;
        if (sc.build(&err) != 0) { std::printf("{\"error\": \"%s\"}\n", err.c_str()); return 0; }
        if (sc.flat.has_textures || !sc.flat.tri_uv.empty()) return 5; // a scene with lightmaps is no textured scene
        struct Map { uint32_t w, h; std::vector<f4> texels; };
        std::vector<Map> maps(2);
        const uint32_t sizes[4][2] = {{1, 1}, {5, 3}, {16, 16}, {2, 37}};
        for (Map& m : maps)
        {
            const uint32_t* wh = sizes[(uint32_t)(rnd() * 3.999f) % 4u];
            m.w = wh[0];
            m.h = wh[1];
            for (uint32_t k = 0; k < m.w * m.h; ++k) m.texels.push_back(f4{rnd(), rnd(), rnd(), 0.0f});
        }
        double acc = 0.0;
        uint32_t mapped = 0;
        for (uint32_t q = 0; q < 8u * n; ++q)
        {
            const uint32_t inst = (uint32_t)(rnd() * 3.999f) % (uint32_t)sc.world.instances.size();
            const uint32_t mi = sc.world.instances[inst].model;
            if ((int)mi != model) continue;                                      // the light: no UVs, no map
            uint32_t ordinal = 0;
            for (uint32_t k = 0; k < inst; ++k) ordinal += sc.world.instances[k].model == mi ? 1u : 0u;
            if (ordinal >= maps.size()) continue;                                // the third placement: no map
            const uint32_t prim = (uint32_t)(rnd() * (float)n) % n;
            const float u = rnd(), v = rnd() * (1.0f - u);
            const float* t = &sc.models[mi].uvs[(size_t)prim * 6];
            const Map& m = maps[ordinal];
            const f3 c = lightmap_lookup(m.texels.data(), m.w, m.h, DTriUV{{t[0], t[1]}, {t[2], t[3]}, {t[4], t[5]}}, u, v);
            const float top = 1.0001f;                                           // a blend of texels in [0, 1]: the weights sum to 1 within rounding
            if (!(c.x >= 0.0f && c.x <= top && c.y >= 0.0f && c.y <= top && c.z >= 0.0f && c.z <= top)) return 6;
            acc += c.x + 2.0 * c.y + 3.0 * c.z;
            ++mapped;
        }
        std::printf("{\"triangles\": %u, \"lookups\": %u, \"checksum\": %.6f}\n", n, mapped, acc);
        return 0;
    }
    if (cmd == "lightmaps_dir" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        HostScene sc;
        const int mat = light_scene(sc);
        if (mat < 0 || n == 0) return 3;
        std::vector<float> p, nr, uv, ntex;
        for (uint32_t t = 0; t < n; ++t)
        {
            const float c[3] = {200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) { p.push_back(c[k] + 10.0f * rnd() - 5.0f); nr.push_back(k == 1 ? 1.0f : 0.2f * rnd() - 0.1f); }
            const uint32_t shape = t % 6u; // lightmaps' six: inside, far outside, all equal, around 1e6, mirrored, the largest finite values
            const float a[2] = {rnd(), rnd()};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 2; ++k)
                    uv.push_back(shape == 0u ? rnd() : shape == 1u ? 40.0f * rnd() - 20.0f : shape == 2u ? a[k] : shape == 3u ? 1.0e6f + 3.0f * rnd()
                                 : shape == 4u ? (v ? -1.0f : 1.0f) * (a[k] + rnd()) : (rnd() < 0.5f ? -3.0e38f : 3.0e38f));
        }
        for (int k = 0; k < 5 * 3; ++k) { ntex.push_back(rnd()); ntex.push_back(rnd()); ntex.push_back(0.5f + 0.5f * rnd()); }
        const float turn[12] = {0, 0, 1, 30, 0, 1, 0, -20, -1, 0, 0, 10};
        std::vector<float> mats(kIdentity, kIdentity + 12);
        mats.insert(mats.end(), turn, turn + 12);
        mats.insert(mats.end(), kIdentity, kIdentity + 12);
        mats[2 * 12 + 3] = 500.0f;
        const int model = sc.add_model(p.data(), nr.data(), n, mat, mats.data(), 3);
        const int tex = sc.add_texture(5, 3, ntex.data());
        if (model < 0 || tex < 0 || sc.set_model_uvs(model, uv.data(), n) != 0 || sc.set_material_normal_texture(mat, tex) != 0) return 4;
        std::string err;
        if (sc.build(&err) != 0) { std::printf("{\"error\": \"%s\"}\n", err.c_str()); return 0; }
        const FlatScene& f = sc.flat;
        if (!f.has_normal_maps) return 5;
        // a map and a gradient on the first two placements: the gradient of random sums under random normals, a tenth of the normals zero
        // and a tenth of the sums denormal
        struct Map { uint32_t w, h; std::vector<f4> texels, grad; };
        std::vector<Map> maps(2);
        const uint32_t sizes[4][2] = {{1, 1}, {5, 3}, {16, 16}, {2, 37}};
        for (Map& m : maps)
        {
            const uint32_t* wh = sizes[(uint32_t)(rnd() * 3.999f) % 4u];
            m.w = wh[0];
            m.h = wh[1];
            for (uint32_t k = 0; k < m.w * m.h; ++k)
            {
                m.texels.push_back(f4{rnd(), rnd(), rnd(), 0.0f});
                float dir9[9], g9[9];
                const bool tiny = rnd() < 0.1f;
                for (float& d : dir9) d = tiny ? 1.0e-42f * (rnd() - 0.5f) : 64.0f * (rnd() - 0.5f);
                const f3 nn = rnd() < 0.1f ? f3{0.0f, 0.0f, 0.0f} : unit3(f3{rnd() - 0.5f, rnd() - 0.5f, rnd() + 0.1f});
                lm_gradient(dir9, nn, 64.0f, g9);
                for (int a = 0; a < 3; ++a) m.grad.push_back(f4{g9[3 * a], g9[3 * a + 1], g9[3 * a + 2], 0.0f});
            }
            m.texels.shrink_to_fit();
            m.grad.shrink_to_fit();
        }
        const TexNView tv = f.texn_view();
        double acc = 0.0;
        uint32_t mapped = 0, moved = 0;
        for (uint32_t q = 0; q < 8u * n; ++q)
        {
            const uint32_t inst = (uint32_t)(rnd() * 3.999f) % (uint32_t)sc.world.instances.size();
            const uint32_t mi = sc.world.instances[inst].model;
            if ((int)mi != model) continue;
            uint32_t ordinal = 0;
            for (uint32_t k = 0; k < inst; ++k) ordinal += sc.world.instances[k].model == mi ? 1u : 0u;
            if (ordinal >= maps.size()) continue;
            const uint32_t leaf_tri = (uint32_t)(rnd() * (float)n) % n, tri = f.tri_base[mi] + leaf_tri;
            const uint32_t prim = sc.blas[mi].prim_ids[leaf_tri];
            const float u = rnd(), v = rnd() * (1.0f - u);
            const f3 d{rnd() - 0.5f, rnd() - 0.5f, rnd() - 0.5f};
            bool front;
            const f3 nrm = unperturbed_normal(f.tri_shade.data(), f.instances.data(), inst, tri, u, v, d, front);
            f3 delta;
            (void)shading_normal_delta(f.tri_shade.data(), f.instances.data(), f.materials.data(), tv, inst, tri, u, v, d, nrm, &delta);
            const float* t = &sc.models[mi].uvs[(size_t)prim * 6];
            const Map& m = maps[ordinal];
            const f3 c = lightmap_lookup_directional(m.texels.data(), m.grad.data(), m.w, m.h, DTriUV{{t[0], t[1]}, {t[2], t[3]}, {t[4], t[5]}}, u, v, delta);
            if (!(c.x >= 0.0f && c.y >= 0.0f && c.z >= 0.0f)) return 6;                // never negative, never a NaN
            if (std::isfinite(c.x) && std::isfinite(c.y) && std::isfinite(c.z)) acc += c.x + 2.0 * c.y + 3.0 * c.z;
            moved += (delta.x != 0.0f || delta.y != 0.0f || delta.z != 0.0f) ? 1u : 0u;
            ++mapped;
        }
        std::printf("{\"triangles\": %u, \"lookups\": %u, \"moved\": %u, \"checksum\": %.6f}\n", n, mapped, moved, acc);
        return 0;
    }
    if (cmd == "lightmap_direct" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        if (n == 0) return 3;
        // the light tables written out by hand, each filling its allocation exactly: random triangles, then three designed ones.  Z: zero
        // area with all vertices at one point (a light point exactly at o when o is that point); P: in the plane z = 0 with normals along
        // z (cosl == 0 exactly for an origin in that plane); the cdf stops at 0.75, so a draw above it runs off the table's end and is
        // clamped to the last entry, which is the ordinary triangle T
        const uint32_t n_random = 1u + n % 7u, n_lights = n_random + 3u, Z = n_random, P = n_random + 1u;
        std::vector<DLight> lights(n_lights);
        std::vector<DTriVerts> pos(n_lights), shade(n_lights);
        std::vector<DTriIsect> isect(n_lights);
        std::vector<DTriUV> uvs(n_lights);
        std::vector<DMaterial> mats(2);
        std::memset(mats.data(), 0, 2 * sizeof(DMaterial));
        for (uint32_t m = 0; m < 2u; ++m)
        {
            mats[m].kind = MAT_EMISSIVE;
            mats[m].colour[0] = 5.0f + m; mats[m].colour[1] = 4.0f; mats[m].colour[2] = 3.0f;
        }
        mats[1].texture = 1u;
        std::vector<DTexture> table{DTexture{0u, 5u, 3u, 0u}};
        std::vector<f4> texels(15);
        for (f4& t : texels) t = f4{4.0f * rnd(), 4.0f * rnd(), 4.0f * rnd(), 0.0f};
        const f3 zp{3.0f, -2.0f, 1.5f};
        float run = 0.0f;
        for (uint32_t i = 0; i < n_lights; ++i)
        {
            f3 a{20.0f * rnd() - 10.0f, 20.0f * rnd() - 10.0f, 5.0f + 5.0f * rnd()};
            f3 b = a + f3{2.0f * rnd() + 0.1f, rnd() - 0.5f, rnd() - 0.5f}, c = a + f3{rnd() - 0.5f, 2.0f * rnd() + 0.1f, rnd() - 0.5f};
            f3 nn = unit3(cross3(b - a, c - a));
            if (i == Z) { a = b = c = zp; nn = f3{0.0f, 0.0f, 1.0f}; }
            if (i == P) { a = f3{1.0f, 0.0f, 0.0f}; b = f3{2.0f, 0.0f, 0.0f}; c = f3{1.0f, 1.0f, 0.0f}; nn = f3{0.0f, 0.0f, 1.0f}; }
            pos[i] = DTriVerts{f4{a.x, a.y, a.z, 0.0f}, f4{b.x, b.y, b.z, 0.0f}, f4{c.x, c.y, c.z, 0.0f}};
            shade[i] = DTriVerts{f4{nn.x, nn.y, nn.z, 0.0f}, f4{nn.x, nn.y, nn.z, 0.0f}, f4{nn.x, nn.y, nn.z, 0.0f}};
            const f3 n0 = cross3(b - a, c - a);
            isect[i] = DTriIsect{f4{n0.x, n0.y, n0.z, 0.0f}, f4{0.0f, 0.0f, 0.0f, 0.0f}, f4{0.0f, 0.0f, 0.0f, 0.0f}};
            uvs[i] = DTriUV{{40.0f * rnd() - 20.0f, rnd()}, {rnd(), 1.0e6f * rnd()}, {-rnd(), rnd()}};
            const float pdf = i == Z && (n & 1u) ? 0.0f : 0.75f / (float)n_lights; // (a zero-area triangle's weight is 0: 0 / 0 as well as x / 0)
            run += pdf;
            lights[i] = DLight{i, i & 1u, pdf, run};
        }
        const LmLightView lv{lights.data(), pos.data(), shade.data(), isect.data(), mats.data(), n_lights, TexView{texels.data(), table.data(), uvs.data()}};
        const uint64_t seed = 0x5EED5EEDull;
        // the samples: random texels, then the designed ones.  Key 480975 is a stream whose draw 0 is exactly 1.0 under this seed
        const uint32_t n_texels = n + 4u, total = 4u * n + 4u * 64u; // four samples of a random texel, 64 of a designed one
        std::vector<uint32_t> key(n_texels);
        std::vector<f3> org(n_texels), nrm(n_texels);
        for (uint32_t k = 0; k < n_texels; ++k)
        {
            key[k] = (uint32_t)(rnd() * 65535.0f) * 65536u + (uint32_t)(rnd() * 65535.0f);
            org[k] = f3{10.0f * rnd() - 5.0f, 10.0f * rnd() - 5.0f, rnd()};
            nrm[k] = f3{0.4f * rnd() - 0.2f, 0.4f * rnd() - 0.2f, 1.0f};
        }
        org[n] = zp;                                   // every sample that picks Z has its light point exactly at o
        org[n + 1u] = f3{0.0f, 0.25f, 0.0f}; nrm[n + 1u] = f3{1.0f, 0.0f, 0.0f};  // in P's plane, facing it: cosl == 0, light_pdf = +inf
        key[n + 2u] = 480975u;                         // x == 1.0 at sample 0
        nrm[n + 3u] = f3{0.0f, 0.0f, 0.0f};            // c == 0: nothing is cast
        {
            Stream probe{stream_key(seed, 480975u, 0u), 0u};
            if (probe.f32() != 1.0f) return 7;
        }
        std::vector<uint8_t> emissive(256, 0);
        emissive[1] = 1;
        std::vector<float> sum(3 * (size_t)n_texels, 0.0f), sumsq(n_texels, 0.0f);
        uint32_t picked[4] = {0, 0, 0, 0}, cast = 0, at_o = 0, grazing = 0, last = 0;
        double acc = 0.0;
        for (uint32_t k = 0; k < n_texels; ++k)
            for (uint32_t sm = 0; sm < (k < n ? 4u : 64u); ++sm)
            {
                const LmLightSample ls = lm_light_sample(lv, seed, key[k], sm, org[k], nrm[k]);
                if (ls.light >= n_lights) return 8;
                if (!(ls.ce.x >= 0.0f && ls.ce.y >= 0.0f && ls.ce.z >= 0.0f)) return 6;                 // never negative, never a NaN
                if (!(std::sqrt((double)ls.ce.x * ls.ce.x + (double)ls.ce.y * ls.ce.y + (double)ls.ce.z * ls.ce.z) <= 100.0 * (1.0 + 1e-6))) return 9;
                if (!ls.cast && (ls.ce.x != 0.0f || ls.ce.y != 0.0f || ls.ce.z != 0.0f)) return 10;
                picked[ls.light == Z ? 0 : ls.light == P ? 1 : ls.light == n_lights - 1u ? 2 : 3] += 1u;
                cast += ls.cast ? 1u : 0u;
                at_o += (k == n && ls.light == Z) ? 1u : 0u;
                grazing += (k == n + 1u && ls.light == P && ls.cast) ? 1u : 0u;
                last += (k == n + 2u && sm == 0u && ls.light == n_lights - 1u) ? 1u : 0u;
                // the host fold: X = G + D under a random gather radiance, id byte and shadow-ray result
                const uint8_t id = (uint8_t)(rnd() * 2.999f);
                const bool blocked = rnd() < 0.3f;
                const float g[3] = {rnd(), rnd(), rnd()}, ce[3] = {ls.ce.x, ls.ce.y, ls.ce.z};
                f4 x{0.0f, 0.0f, 0.0f, 0.0f};
                float* xs = &x.x;
                for (int c = 0; c < 3; ++c)
                {
                    xs[c] = lm_direct_x(g[c], emissive[id] != 0, ce[c], blocked);
                    sum[3 * (size_t)k + c] = sum[3 * (size_t)k + c] + xs[c];
                }
                const float l = lum(x);
                sumsq[k] = sumsq[k] + l * l;
                if (!(l >= 0.0f) || !std::isfinite(l)) return 11;
            }
        for (uint32_t k = 0; k < n_texels; ++k) acc += sum[3 * (size_t)k] + 2.0 * sum[3 * (size_t)k + 1] + 3.0 * sum[3 * (size_t)k + 2] + sumsq[k];
        if (last != 1u) return 12;
        std::printf("{\"texels\": %u, \"lights\": %u, \"samples\": %u, \"cast\": %u, \"zero_area\": %u, \"at_origin\": %u, \"grazing\": %u, \"last_entry\": %u, \"checksum\": %.6f}\n",
                    n_texels, n_lights, total, cast, picked[0], at_o, grazing, picked[2], acc);
        return 0;
    }
    if (cmd == "texelfilter" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        if (n == 0) return 3;
        std::vector<float> p, nr, uv;
        for (uint32_t t = 0; t < n; ++t)
        {
            const float c[3] = {200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f, 200.0f * rnd() - 100.0f};
            const uint32_t shape = t % 7u; // lightmaps' six, and a triangle whose three positions are equal (A3 = 0) under UVs inside the map
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 3; ++k) { p.push_back(shape == 6u ? c[k] : c[k] + 10.0f * rnd() - 5.0f); nr.push_back(k == 1 ? 1.0f : 0.2f * rnd() - 0.1f); }
            const float a[2] = {rnd(), rnd()};
            for (int v = 0; v < 3; ++v)
                for (int k = 0; k < 2; ++k)
                    uv.push_back(shape == 0u || shape == 6u ? rnd() : shape == 1u ? 40.0f * rnd() - 20.0f : shape == 2u ? a[k] : shape == 3u ? 1.0e6f + 3.0f * rnd()
                                 : shape == 4u ? (v ? -1.0f : 1.0f) * (a[k] + rnd()) : (rnd() < 0.5f ? -3.0e38f : 3.0e38f));
        }
        const xf34 turn{m33{f3{0, 0, -1}, f3{0, 1, 0}, f3{1, 0, 0}}, f3{30, -20, 10}};
        const uint32_t sizes[6][2] = {{1, 1}, {5, 3}, {16, 16}, {37, 19}, {2, 37}, {48, 32}};
        const float reaches[3] = {2.0f, 1.0e-3f, 1.0e30f};
        double acc = 0.0;
        uint32_t covered = 0, finite = 0;
        for (const uint32_t* wh : sizes)
        {
            const uint32_t w = wh[0], h = wh[1];
            const size_t px = (size_t)w * h;
            std::vector<uint32_t> owner;
            lm_owner_host(uv.data(), n, w, h, owner);
            std::vector<float> P(px * 3), N(px * 3), sum(px * 3), sq(px), mean(px * 3), area(px);
            for (size_t k = 0; k < px; ++k)
            {
                float u32, v32;
                f3 x, nn;
                lm_resolve_host(uv.data(), p.data(), nr.data(), turn, w, h, k, owner[k], &u32, &v32, &x, &nn);
                P[3 * k] = x.x; P[3 * k + 1] = x.y; P[3 * k + 2] = x.z;
                N[3 * k] = nn.x; N[3 * k + 1] = nn.y; N[3 * k + 2] = nn.z;
                for (int ch = 0; ch < 3; ++ch) sum[3 * k + ch] = 40.0f * rnd();
                sq[k] = 200.0f * rnd();
                covered += owner[k] != MISS_ID ? 1u : 0u;
            }
            for (int pass = 0; pass < 6; ++pass)
            {
                const float reach = reaches[pass % 3];
                const LmFilterK k{{4.0f, 1.0f, 7u, 8u}, reach * reach};
                lmf_filter_host(w, h, k, owner.data(), P.data(), N.data(), p.data(), uv.data(), sum.data(), pass < 3 ? sq.data() : nullptr, 16u, nullptr, mean.data(), area.data());
                for (size_t k2 = 0; k2 < px; ++k2)
                {
                    if (owner[k2] == MISS_ID && (mean[3 * k2] != 0.0f || mean[3 * k2 + 1] != 0.0f || mean[3 * k2 + 2] != 0.0f || area[k2] != 0.0f)) return 6;
                    for (int ch = 0; ch < 3; ++ch)
                        if (std::isfinite(mean[3 * k2 + ch])) { acc += (ch + 1.0) * mean[3 * k2 + ch]; ++finite; }
                }
            }
        }
        std::printf("{\"triangles\": %u, \"covered\": %u, \"finite\": %u, \"checksum\": %.6f}\n", n, covered, finite, acc);
        return 0;
    }
    if (cmd == "screenfilter" && argc >= 3)
    {
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[2]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        const LmFilterK k{{4.0f, 1.0f, 7u, 8u}, INFINITY};
        const uint32_t sizes[4][2] = {{1, 1}, {5, 3}, {16, 16}, {37, 19}};
        double acc = 0.0;
        uint32_t pixels = 0, finite = 0;
        auto tally = [&](const std::vector<f4>& out) {
            for (const f4& c : out)
                for (float v : {c.x, c.y, c.z, c.w})
                    if (std::isfinite(v)) { acc += v; ++finite; }
        };
        for (const uint32_t* wh : sizes)
        {
            const int w = (int)wh[0], h = (int)wh[1];
            const size_t px = (size_t)w * h;
            pixels += (uint32_t)px;
            // a floor and a wall under noisy colour; pos.w is the texel rule's area (positive: +inf * area is +inf)
            std::vector<f4> cv(px), pos(px), nv(px);
            std::vector<uint32_t> model(px);
            for (size_t i = 0; i < px; ++i)
            {
                const bool wall = rnd() < 0.4f;
                cv[i] = f4{4.0f * rnd(), 4.0f * rnd(), 4.0f * rnd(), 0.0f};
                pos[i] = f4{10.0f * rnd(), wall ? 10.0f * rnd() : 0.0f, wall ? 0.0f : 10.0f * rnd(), 0.5f + rnd()};
                nv[i] = f4{0.2f * rnd() - 0.1f, wall ? 0.0f : 1.0f, wall ? 1.0f : 0.0f, 1.0f};
                model[i] = rnd() < 0.15f ? (uint32_t)MISS_ID : rnd() < 0.5f ? 0u : 1u;
            }
            // the screen rule on what the prep kernel would leave: zeros at an invalid pixel
            std::vector<f4> cvi = cv, nvi = nv;
            for (size_t i = 0; i < px; ++i)
                if (rnd() < 0.1f) cvi[i] = nvi[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
            tally(core_filter_host(w, h, k, cvi, pos.data(), nvi.data(), [&](size_t i) { return ScreenRule(nvi.data(), model.data(), i); }));
            // one model, every pixel a valid hit, no reach: the two rules are one filter
            std::fill(model.begin(), model.end(), 0u);
            const std::vector<f4> screen = core_filter_host(w, h, k, cv, pos.data(), nv.data(), [&](size_t i) { return ScreenRule(nv.data(), model.data(), i); });
            const std::vector<f4> texel = core_filter_host(w, h, k, cv, pos.data(), nv.data(), [&](size_t i) { return TexelRule(k, pos.data(), nv.data(), i); });
            if (std::memcmp(screen.data(), texel.data(), px * sizeof(f4)) != 0)
            {
                std::printf("{\"error\": \"%d x %d: the texel rule without reach differs from the screen rule\"}\n", w, h);
                return 7;
            }
            tally(screen);
        }
        std::printf("{\"pixels\": %u, \"finite\": %u, \"checksum\": %.6f}\n", pixels, finite, acc);
        return 0;
    }
    if (cmd == "probegrid" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        const uint32_t counts[6][3] = {{1, 1, 1}, {2, 2, 2}, {3, 2, 4}, {5, 1, 3}, {1, 7, 1}, {1, 1, 6}};
        double acc = 0.0;
        uint32_t lookups = 0, lit = 0;
        for (const uint32_t* cnt : counts)
        {
            const size_t nodes = (size_t)cnt[0] * cnt[1] * cnt[2];
            std::vector<DProbe> rec(nodes); // exactly the grid: a node index past it is a heap overflow
            for (DProbe& r : rec)
            {
                r.valid = rnd() < 0.8f ? 1.0f : 0.0f;
                for (float& v : r.sh) v = r.valid != 0.0f ? 4.0f * rnd() - 1.0f : 0.0f;
            }
            const ProbeGridView g{rec.data(), {4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f},
                                  {0.25f + rnd(), 0.25f + rnd(), 0.25f + rnd()}, {cnt[0], cnt[1], cnt[2]}, rnd() < 0.5f ? 0.0f : 0.125f};
            for (uint32_t i = 0; i < n; ++i)
            {
                // inside, a little outside, far outside, huge, infinite and NaN positions; unit, zero and NaN normals
                const uint32_t kind = i % 8u;
                const float reach = kind == 0u ? 1.0f : kind == 1u ? 3.0f : kind == 2u ? 1e4f : kind == 3u ? 1e30f : 1.0f;
                float p[3], nn[3];
                for (int a = 0; a < 3; ++a)
                {
                    p[a] = g.origin[a] + reach * (2.0f * rnd() - 0.5f) * g.cell[a] * (float)cnt[a];
                    nn[a] = 2.0f * rnd() - 1.0f;
                }
                if (kind == 4u) p[i % 3u] = NAN;
                if (kind == 5u) p[i % 3u] = i & 8u ? INFINITY : -INFINITY;
                if (kind == 6u) nn[i % 3u] = NAN;
                if (kind == 7u) p[0] = p[1] = p[2] = 3.0e38f;
                f3 c;
                if (probe_grid_lookup(g, f3{p[0], p[1], p[2]}, f3{nn[0], nn[1], nn[2]}, &c)) ++lit;
                for (float v : {c.x, c.y, c.z})
                    if (std::isfinite(v)) acc += v;
                ++lookups;
            }
        }
        std::printf("{\"lookups\": %u, \"lit\": %u, \"checksum\": %.6f}\n", lookups, lit, acc);
        return 0;
    }
    if (cmd == "probedepth" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        const uint32_t counts[6][3] = {{1, 1, 1}, {2, 2, 2}, {3, 2, 4}, {5, 1, 3}, {1, 7, 1}, {1, 1, 6}};
        double acc = 0.0;
        uint32_t lookups = 0, lit = 0, texels_ok = 1;
        for (const uint32_t* cnt : counts)
        {
            const size_t nodes = (size_t)cnt[0] * cnt[1] * cnt[2];
            std::vector<DProbe> rec(nodes);
            for (DProbe& r : rec)
            {
                r.valid = rnd() < 0.8f ? 1.0f : 0.0f;
                for (float& v : r.sh) v = r.valid != 0.0f ? 4.0f * rnd() - 1.0f : 0.0f;
            }
            const ProbeGridView g{rec.data(), {4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f},
                                  {0.25f + rnd(), 0.25f + rnd(), 0.25f + rnd()}, {cnt[0], cnt[1], cnt[2]}, rnd() < 0.5f ? 0.0f : 0.125f};
            const uint32_t res = 2u + (uint32_t)(rnd() * 14.99f);
            std::vector<DProbeDepth> table(nodes * res * res); // exactly the table: a texel past a node's map, or a node past the grid, is a heap overflow
            for (DProbeDepth& m : table)
            {
                m.m1 = 3.0f * rnd();
                m.m2 = rnd() < 0.8f ? m.m1 * m.m1 + rnd() : m.m1 * m.m1 * rnd(); // (both signs of m2 - m1^2; zero variance where rnd() is 0)
            }
            const ProbeDepthView dv{table.data(), res, rnd() < 0.5f ? 1u : 0u, rnd() < 0.5f ? 0.0f : 0.05f};
            for (uint32_t i = 0; i < n; ++i)
            {
                const uint32_t kind = i % 8u;
                const float reach = kind == 0u ? 1.0f : kind == 1u ? 3.0f : kind == 2u ? 1e4f : kind == 3u ? 1e30f : 1.0f;
                float p[3], nn[3];
                for (int a = 0; a < 3; ++a)
                {
                    p[a] = g.origin[a] + reach * (2.0f * rnd() - 0.5f) * g.cell[a] * (float)cnt[a];
                    nn[a] = 2.0f * rnd() - 1.0f;
                }
                if (kind == 4u) p[i % 3u] = NAN;
                if (kind == 5u) p[i % 3u] = i & 8u ? INFINITY : -INFINITY;
                if (kind == 6u) nn[i % 3u] = NAN;
                if (kind == 7u) p[0] = p[1] = p[2] = 3.0e38f;
                f3 c;
                if (probe_grid_lookup<true>(g, f3{p[0], p[1], p[2]}, f3{nn[0], nn[1], nn[2]}, &c, &dv)) ++lit;
                for (float v : {c.x, c.y, c.z})
                    if (std::isfinite(v)) acc += v;
                ++lookups;
                // the texel alone, of what a lookup can form and more
                const float odd[6] = {0.0f, -0.0f, 3.0e38f, INFINITY, -INFINITY, NAN};
                const float dir[3] = {kind < 6u ? odd[kind] : p[0], i & 16u ? p[1] : odd[(i >> 5) % 6u], p[2]};
                if (probe_oct_texel(dir, res) >= res * res) texels_ok = 0;
            }
        }
        std::printf("{\"lookups\": %u, \"lit\": %u, \"checksum\": %.6f, \"texels_inside\": %u}\n", lookups, lit, acc, texels_ok);
        return 0;
    }
    if (cmd == "proberadiance" && argc >= 4)
    {
        const uint32_t n = (uint32_t)std::atoi(argv[2]);
        uint64_t s = 0x9E3779B97F4A7C15ull ^ (uint64_t)std::atoll(argv[3]);
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((s >> 40) & 0xffff) / 65535.0f; };
        const uint32_t counts[6][3] = {{1, 1, 1}, {2, 2, 2}, {3, 2, 4}, {5, 1, 3}, {1, 7, 1}, {1, 1, 6}};
        double acc = 0.0, filtered = 0.0;
        uint32_t lookups = 0, lit = 0, round_trip = 1, finite = 1;
        for (const uint32_t* cnt : counts)
        {
            const size_t nodes = (size_t)cnt[0] * cnt[1] * cnt[2];
            std::vector<DProbe> rec(nodes);
            for (DProbe& r : rec)
            {
                r.valid = rnd() < 0.8f ? 1.0f : 0.0f;
                for (float& v : r.sh) v = r.valid != 0.0f ? 4.0f * rnd() - 1.0f : 0.0f;
            }
            const ProbeGridView g{rec.data(), {4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f, 4.0f * rnd() - 2.0f},
                                  {0.25f + rnd(), 0.25f + rnd(), 0.25f + rnd()}, {cnt[0], cnt[1], cnt[2]}, rnd() < 0.5f ? 0.0f : 0.125f};
            const uint32_t res = 2u + (uint32_t)(rnd() * 14.99f), rr = res * res, levels = 1u + (uint32_t)(rnd() * 7.99f);
            // the prefilter over raw maps with empty texels, one probe's worth of exactly rr entries at a time, into a table that is exactly
            // nodes * levels * rr texels: a texel past a map, a level past the levels or a node past the grid is a heap overflow
            ProbeRadianceView rv{nullptr, res, levels, {}};
            for (uint32_t l = 0; l < levels; ++l) rv.alpha[l] = (float)(l + 1u) / (float)levels;
            std::vector<f4> table(nodes * levels * rr), dirw(rr), mean(rr);
            for (uint32_t j = 0; j < rr; ++j)
            {
                float d[3], om;
                probe_oct_dir(j, res, d, &om);
                dirw[j] = f4{d[0], d[1], d[2], om};
                if (probe_oct_texel(d, res) != j) round_trip = 0;
            }
            for (size_t node = 0; node < nodes; ++node)
            {
                const float empty = node % 3u == 0u ? 1.0f : 0.3f; // (every third probe saw nothing at all)
                for (uint32_t j = 0; j < rr; ++j)
                {
                    const uint32_t k = rnd() < empty ? 0u : 1u + (uint32_t)(rnd() * 30.0f);
                    const float sums[3] = {5.0f * rnd() * (float)k, 5.0f * rnd() * (float)k, 5.0f * rnd() * (float)k};
                    mean[j] = probe_radiance_mean(sums, k);
                }
                for (uint32_t l = 0; l < levels; ++l)
                    for (uint32_t i = 0; i < rr; ++i)
                    {
                        const f4 o = probe_prefilter_texel(dirw.data(), mean.data(), rr, rv.alpha[l], i);
                        table[(node * levels + l) * rr + i] = o;
                        for (float v : {o.x, o.y, o.z})
                        {
                            if (!std::isfinite(v) || v < 0.0f) finite = 0;
                            filtered += v;
                        }
                    }
            }
            rv.table = table.data();
            const uint32_t dres = 2u + (uint32_t)(rnd() * 14.99f);
            std::vector<DProbeDepth> moments(nodes * dres * dres);
            for (DProbeDepth& m : moments)
            {
                m.m1 = 3.0f * rnd();
                m.m2 = rnd() < 0.8f ? m.m1 * m.m1 + rnd() : m.m1 * m.m1 * rnd();
            }
            const ProbeDepthView dv{moments.data(), dres, rnd() < 0.5f ? 1u : 0u, rnd() < 0.5f ? 0.0f : 0.05f};
            for (uint32_t i = 0; i < n; ++i)
            {
                // inside, a little outside, far outside, huge, infinite and NaN positions; unit, zero, huge, infinite and NaN normals and
                // directions; alphas below, inside and above the levels, infinite and NaN
                const uint32_t kind = i % 8u;
                const float reach = kind == 0u ? 1.0f : kind == 1u ? 3.0f : kind == 2u ? 1e4f : kind == 3u ? 1e30f : 1.0f;
                float p[3], nn[3], dd[3];
                for (int a = 0; a < 3; ++a)
                {
                    p[a] = g.origin[a] + reach * (2.0f * rnd() - 0.5f) * g.cell[a] * (float)cnt[a];
                    nn[a] = 2.0f * rnd() - 1.0f;
                    dd[a] = 2.0f * rnd() - 1.0f;
                }
                if (kind == 4u) p[i % 3u] = NAN;
                if (kind == 5u) p[i % 3u] = i & 8u ? INFINITY : -INFINITY;
                if (kind == 6u) nn[i % 3u] = NAN;
                if (kind == 7u) p[0] = p[1] = p[2] = 3.0e38f;
                const float odd[6] = {0.0f, -0.0f, 3.0e38f, INFINITY, -INFINITY, NAN};
                if ((i >> 3) % 4u == 1u) dd[i % 3u] = odd[(i >> 5) % 6u];
                if ((i >> 3) % 4u == 2u) dd[0] = dd[1] = dd[2] = 0.0f;
                const float alphas[6] = {-1.0f, 0.0f, 1.5f * rnd(), 2.0f, INFINITY, NAN};
                const float a = alphas[(i >> 4) % 6u];
                f3 c;
                const bool has = i & 1u ? probe_grid_specular<true>(g, rv, f3{p[0], p[1], p[2]}, f3{nn[0], nn[1], nn[2]}, f3{dd[0], dd[1], dd[2]}, a, &c, &dv)
                                        : probe_grid_specular(g, rv, f3{p[0], p[1], p[2]}, f3{nn[0], nn[1], nn[2]}, f3{dd[0], dd[1], dd[2]}, a, &c);
                if (has) ++lit;
                for (float v : {c.x, c.y, c.z})
                    if (std::isfinite(v)) acc += v;
                ++lookups;
            }
        }
        std::printf("{\"lookups\": %u, \"lit\": %u, \"checksum\": %.6f, \"filtered\": %.6f, \"round_trip\": %u, \"finite\": %u}\n", lookups, lit, acc, filtered,
                    round_trip, finite);
        return 0;
    }
    if (cmd == "queues" && argc >= 3) return qsweep::queues_sweep((uint64_t)std::strtoull(argv[2], nullptr, 10));
    if (cmd == "plan")
    {
        std::printf("[");
        for (int i = 2; i < argc; ++i)
        {
            unsigned long long v[11] = {};
            const char* sep = i > 2 ? ", " : "";
            if (std::sscanf(argv[i], "b:%llu,%llu,%llu,%llu", v, v + 1, v + 2, v + 3) == 4)
                std::printf("%s%zu", sep, max_paths_for(v[0], v[1], (uint32_t)v[2], v[3] != 0));
            else if (std::sscanf(argv[i], "p:%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9,
                                 v + 10) == 11)
            {
                const PlanRequest q{(uint32_t)v[0], v[1], v[2] != 0, (uint32_t)v[3], (uint32_t)v[4], v[5] != 0, v[6], {v[7], v[8], v[9], v[10]}};
                const BatchPlan p = plan_batches(q);
                std::printf("%s[%u, %u, %u]", sep, p.batch, p.n_batches, p.n_pipes);
            }
            else return 2;
        }
        std::printf("]\n");
        return 0;
    }
    if (cmd == "png" && argc >= 5)
    {
        const uint32_t w = (uint32_t)std::atoi(argv[2]), h = (uint32_t)std::atoi(argv[3]);
        std::vector<uint8_t> rgb((size_t)w * h * 3);
        for (size_t i = 0; i < rgb.size(); ++i) rgb[i] = (uint8_t)((i * 2654435761u) >> 24);
        std::string err;
        if (!write_png_rgb8(argv[4], rgb.data(), w, h, &err)) { std::printf("{\"error\": \"%s\"}\n", err.c_str()); return 0; }
        std::printf("{\"bytes\": %zu}\n", rgb.size());
        return 0;
    }
    return 2;
}
