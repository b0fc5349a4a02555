// Headless driver: src/main.rs's run() without the window — scene set-up (:75-137), then the event loop's MainEventsCleared
// body (:179-216) for a number of frames, optionally with scripted camera input, and ImageHelper::write_image at the end.
// Everything goes through include/ptmi.hpp, i.e. the C-ABI of libptmi.
//
//   examples/headless [--width W] [--height H] [--frames N] [--bounces B] [--move] [--models DIR] [--out file.png]
//   examples/headless --gpus N [--devices a,b,..] --spp S ...   the same scene, S samples per pixel on N GPUs of this process (pt_multi)
//   examples/headless --render FIRST COUNT [--load-state in.bin] [--save-state out.bin] ...   samples [FIRST, FIRST + COUNT) accumulated
//       without the temporal pass; the frame's state (accumulation, first-hit position, id history) can be saved and picked up by another
//       process: a long render stopped and continued (pt_read_frame / pt_write_accumulation)
//   examples/headless ... --aperture A --focus F   thin lens of diameter A focused at distance F (default: the reference's pinhole, 0 and 950)
//   examples/headless ... --projection panorama[:SX:SY] | ortho:HEIGHT   a panoramic camera covering SX x SY degrees (default 360 x 180) or an orthographic one
//                                          whose view volume is HEIGHT world units high (pt_set_projection); not with --aperture, --move or --slide
//   examples/headless ... --slide DX DZ   frame f >= 1 first moves the short box to the translation (f * DX, 0, f * DZ) (pt_set_instances + pt_build:
//                                          the BLASes are kept, the resident scene is patched) and the loop drives frame_moving instead of frame
//   examples/headless ... --temporal out.png   the loop drives frame_temporal instead: the scripted frames (--move, --slide) go through the temporal
//                                          stage of the denoiser (reprojected history, history length, luminance moments, then the a-trous levels) and the
//                                          last frame's result is written; --temporal-rescue, --temporal-mean-length and --temporal-demodulate (only
//                                          with --temporal) switch on pt_temporal_options' rescue, length_rule and demodulate
//   examples/headless ... --denoise den.png   also writes the final frame through the edge-aware denoiser (guides of the last frame's sample)
//   examples/headless ... --denoise-albedo den.png   the same through the demodulated filter (pt_denoise_albedo): the mean albedo of every pixel
//                                        is accumulated over the samples that were rendered, the frame divided by it, filtered and multiplied back,
//                                        so textures (--checker) stay sharp; also with --render
//   examples/headless ... --follow K   --denoise and --denoise-albedo take their guides (and the mean albedo) through mirrors and glass, up to K
//                                        of them per pixel, to the first rough surface (pt_render_guides_followed); K = 0..8, default 0
//   examples/headless ... --mirror-glass   the tall box is a mirror (main.rs:90) and the short box glass (main.rs:89): what --follow is for
//   examples/headless ... --bake-probes NX NY NZ SPP probes.txt   after the usual render, bakes SPP samples into an NX x NY x NZ grid of
//       irradiance probes spanning the scene's bounds shrunk by 5 % per side (x fastest, then y, then z; stream keys 0, 1, ...) and
//       writes one line per probe: its 27 raw spherical-harmonics sums [k][c] as hexadecimal floats (%a)
//   examples/headless ... --bake-lightmap W H SPP PASSES map.txt   after the usual render, bakes SPP samples per texel into a W x H lightmap of the floor,
//       ceiling and back wall (cb_main.obj, model 1) under --checker's planar UVs, in which floor and ceiling overlap and the lower triangle index
//       wins (rays start 0.25 off the surface, stream keys = texel indices), dilates it PASSES times and writes one line per texel:
//       its coverage byte (1 baked, 2 dilated, 0 neither) and the three raw sums as hexadecimal floats (%a)
//   examples/headless ... --bake-lightmap ... --baked-view SPP out.png   sets the dilated map it just baked, sum / its SPP, on the shell
//       (pt_set_lightmap) and writes the baked view (pt_render_baked: SPP samples per pixel, chains followed --follow K hops, unmapped
//       surfaces black)
//   examples/headless ... --probe-grid NX NY NZ SPP --baked-view SPP out.png   alone or beside --bake-lightmap: bakes an NX x NY x NZ irradiance volume
//       spanning the scene's bounds inset by half a cell (SPP samples per probe; probes that see back faces in more than a quarter of their rays
//       are left out: pt_probe_backfaces), sets it (pt_set_probe_grid) and writes the baked view, in which the grid lights every final surface
//       that no map lights
//   examples/headless ... --probe-grid NX NY NZ SPP --probe-depth R --baked-view SPP out.png   also bakes the nodes' R x R octahedral depth moments
//       from the same rays (pt_bake_probe_depth, distances clamped to 1.5 cell diagonals) and sets them (pt_set_probe_grid_depth), so that the
//       grid's lookup weighs every node by its visibility and light stops leaking through walls
//   examples/headless ... --probe-grid NX NY NZ SPP --probe-radiance R --baked-view SPP out.png   also bakes the nodes' R x R octahedral radiance maps
//       from the same rays (pt_bake_probe_radiance), prefilters them on the device at the GGX alphas 0.1, 0.2, 0.4, 0.7 and 1 and sets them
//       (pt_set_probe_grid_radiance), so that GGX metal in the baked view reflects its surroundings; --metal-box makes the tall box such a metal
//   examples/headless ... --bake-lightmap ... --lightmap-denoise [--baked-view ...]   bakes with second moments (pt_bake_lightmap_moments), runs the
//       texel-space filter on the sums (pt_lightmap_denoise, default parameters) and dilates its texel MEANS: map.txt then holds means, not sums,
//       and --baked-view sets them as they are
//   examples/headless ... --bake-lightmap W H SPP PASSES map.txt --adaptive REL MAX [--lightmap-denoise] [--baked-view ...]   bakes adaptively
//       (pt_bake_lightmap_adaptive): rounds of SPP samples for the texels whose mean luminance is not yet known to the relative error REL, at
//       most MAX samples per texel (0: no cap), until a round selects no texel; prints the rays spent and the mean count.  Every texel is
//       divided by its own count before the means are dilated (or filtered with the counts, pt_lightmap_denoise_counts, then dilated), so
//       map.txt holds means, and --baked-view sets them as they are
//   examples/headless ... --bake-lightmap ... --direct [--adaptive REL MAX] [--lightmap-denoise] [--baked-view ...]   takes one light sample with a
//       shadow ray at the texel beside every gather sample (pt_bake_lightmap_direct, pt_bake_lightmap_adaptive_direct; the light samples'
//       streams follow the gather samples': light_key_base = W * H); everything after the bake is what it is without the option
//   examples/headless ... --bake-lightmap ... --gather ITERATIONS [--direct] [--baked-view ...]   bakes by final gather (pt_bake_lightmap_gather):
//       ITERATIONS passes, each from the map the pass before set on the shell, the gather rays ending in it; with --direct pass k holds the
//       direct light and k bounces between the shell's own surfaces
//   examples/headless ... --bake-lightmap ... --directional [--normal-ripples N] [--baked-view ...]   bakes the first moments beside the sums
//       (pt_bake_lightmap_directional), takes their tangential gradient (pt_lightmap_gradient), dilates it plane by plane and, under --baked-view,
//       sets it beside the map (pt_set_lightmap_directional): with --normal-ripples, which then lie under the bake's planar UVs (the floor and the
//       ceiling have a tangent frame in them, the back wall has none and stays flat), the baked view shades the ripples.  map.txt is unchanged
//   examples/headless ... --checker N   an N x N checker (texels 1 and 0.2, bilinear, repeating) on the floor, ceiling and back wall (cb_main.obj) with
//                                        planar UVs: a vertex's (x, z) over the model's own extent in x and z
//   examples/headless ... --emission-checker N   the same N x N checker as the EMISSION texture of the light (cb_light.obj) under the same planar UVs:
//                                        a textured area light (pt_set_material_emission_texture)
//   examples/headless ... --normal-ripples N   an N x N procedural ripple NORMAL map (pt_set_material_normal_texture) on cb_main.obj: texel (i, j) is the
//                                        tangent-space vector (0.3 * tri((i + 0.5) / N), 0.3 * tri((j + 0.5) / N), z), tri(a) = 4 * |a - 0.5| - 1, z making it
//                                        a unit vector, encoded 0.5 * v + 0.5 (every step one binary32 operation).  UVs: s = x, t = y + z over the model's own
//                                        extents, so that the floor, the ceiling and the back wall all have a tangent frame
//   examples/headless ... --metal-box --roughness-checker N   an N x N checker of linear roughness 0.1 / 0.6 (texel (i, j): 0.6 where i + j is odd) as
//                                        the ROUGHNESS map (pt_set_material_roughness_texture) of the tall box --metal-box turns to GGX metal, under
//                                        planar UVs set the way --checker sets cb_main.obj's: the GGX alpha of a hit is its bilinear texel's first
//                                        component squared, and the material's own roughness 0.4 is not read
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptmi.hpp"

using namespace ptmi;

int main(int argc, char** argv)
{
    uint32_t width = 1920, height = 1080, frames = 64, bounces = 8; // IMAGE_WIDTH/HEIGHT main.rs:44-45; the reference's MAX_BOUNCES is 1024
    bool move = false, slide = false, mirror_glass = false;
    float slide_dx = 0.0f, slide_dz = 0.0f;
    uint32_t gpus = 0, spp = 64;
    std::vector<int32_t> devices;
    std::string models_dir = "models/cornell", out = "", load_state = "", save_state = "", denoise_out = "", denoise_albedo_out = "", temporal_out = "";
    bool render_mode = false;
    pt_temporal_options temporal{};
    bool temporal_option = false;
    uint32_t render_first = 0, render_count = 0;
    float aperture = 0.0f, focus = 950.0f; // main.rs:127's values: a pinhole
    uint32_t probes[3] = {0, 0, 0}, probe_spp = 0, checker = 0, emission_checker = 0, normal_ripples = 0, roughness_checker = 0, follow = 0;
    std::string probes_out = "";
    uint32_t lightmap[4] = {0, 0, 0, 0}; // W H SPP PASSES
    std::string lightmap_out = "";
    uint32_t baked_spp = 0;
    uint32_t probe_grid[4] = {0, 0, 0, 0}; // --probe-grid NX NY NZ SPP
    uint32_t probe_depth = 0;              // --probe-depth R
    bool probe_depth_given = false;
    uint32_t probe_radiance = 0;           // --probe-radiance R
    bool probe_radiance_given = false, metal_box = false;
    bool lightmap_denoise = false, directional = false, adaptive = false, direct = false;
    uint32_t gather = 0;
    bool gather_given = false;
    float adaptive_rel = 0.0f;
    uint32_t adaptive_max = 0;
    std::string baked_out = "";
    pt_projection projection{}; // PT_PROJ_PERSPECTIVE
    for (int i = 1; i < argc; ++i)
    {
        const std::string a = argv[i];
        auto next = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", what); std::exit(2); }
            return argv[++i];
        };
        if (a == "--width") width = (uint32_t)std::atoi(next("--width"));
        else if (a == "--height") height = (uint32_t)std::atoi(next("--height"));
        else if (a == "--frames") frames = (uint32_t)std::atoi(next("--frames"));
        else if (a == "--bounces") bounces = (uint32_t)std::atoi(next("--bounces"));
        else if (a == "--models") models_dir = next("--models");
        else if (a == "--out") out = next("--out");
        else if (a == "--denoise") denoise_out = next("--denoise");
        else if (a == "--temporal") temporal_out = next("--temporal");
        else if (a == "--temporal-rescue") { temporal.rescue = 1; temporal_option = true; }
        else if (a == "--temporal-mean-length") { temporal.length_rule = PT_TEMPORAL_LENGTH_MEAN; temporal_option = true; }
        else if (a == "--temporal-demodulate") { temporal.demodulate = 1; temporal_option = true; }
        else if (a == "--denoise-albedo") denoise_albedo_out = next("--denoise-albedo");
        else if (a == "--follow") follow = (uint32_t)std::atoi(next("--follow"));
        else if (a == "--mirror-glass") mirror_glass = true;
        else if (a == "--move") move = true;
        else if (a == "--slide") { slide = true; slide_dx = (float)std::atof(next("--slide")); slide_dz = (float)std::atof(next("--slide")); }
        else if (a == "--aperture") aperture = (float)std::atof(next("--aperture"));
        else if (a == "--focus") focus = (float)std::atof(next("--focus"));
        else if (a == "--projection")
        {
            const std::string v = next("--projection");
            float x = 0.0f, y = 0.0f;
            if (v == "perspective") projection = pt_projection{};
            else if (v == "panorama") { projection = pt_projection{}; projection.kind = PT_PROJ_PANORAMA; }
            else if (std::sscanf(v.c_str(), "panorama:%f:%f", &x, &y) == 2) { projection = pt_projection{}; projection.kind = PT_PROJ_PANORAMA; projection.span_x_deg = x; projection.span_y_deg = y; }
            else if (std::sscanf(v.c_str(), "ortho:%f", &x) == 1) { projection = pt_projection{}; projection.kind = PT_PROJ_ORTHOGRAPHIC; projection.ortho_height = x; }
            else { std::fprintf(stderr, "--projection takes perspective, panorama, panorama:SX:SY or ortho:HEIGHT\n"); return 2; }
        }
        else if (a == "--gpus") gpus = (uint32_t)std::atoi(next("--gpus"));
        else if (a == "--checker") checker = (uint32_t)std::atoi(next("--checker"));
        else if (a == "--normal-ripples") normal_ripples = (uint32_t)std::atoi(next("--normal-ripples"));
        else if (a == "--roughness-checker") roughness_checker = (uint32_t)std::atoi(next("--roughness-checker"));
        else if (a == "--emission-checker") emission_checker = (uint32_t)std::atoi(next("--emission-checker"));
        else if (a == "--spp") spp = (uint32_t)std::atoi(next("--spp"));
        else if (a == "--render") { render_mode = true; render_first = (uint32_t)std::atoi(next("--render")); render_count = (uint32_t)std::atoi(next("--render")); }
        else if (a == "--bake-probes")
        {
            for (uint32_t& n : probes) n = (uint32_t)std::atoi(next("--bake-probes"));
            probe_spp = (uint32_t)std::atoi(next("--bake-probes"));
            probes_out = next("--bake-probes");
        }
        else if (a == "--bake-lightmap")
        {
            for (uint32_t& n : lightmap) n = (uint32_t)std::atoi(next("--bake-lightmap"));
            lightmap_out = next("--bake-lightmap");
        }
        else if (a == "--probe-grid")
        {
            for (uint32_t& n : probe_grid) n = (uint32_t)std::atoi(next("--probe-grid"));
        }
        else if (a == "--probe-depth")
        {
            probe_depth = (uint32_t)std::atoi(next("--probe-depth"));
            probe_depth_given = true;
        }
        else if (a == "--probe-radiance")
        {
            probe_radiance = (uint32_t)std::atoi(next("--probe-radiance"));
            probe_radiance_given = true;
        }
        else if (a == "--metal-box") metal_box = true;
        else if (a == "--baked-view")
        {
            baked_spp = (uint32_t)std::atoi(next("--baked-view"));
            baked_out = next("--baked-view");
        }
        else if (a == "--lightmap-denoise") lightmap_denoise = true;
        else if (a == "--direct") direct = true;
        else if (a == "--gather") { gather = (uint32_t)std::atoi(next("--gather")); gather_given = true; }
        else if (a == "--directional") directional = true;
        else if (a == "--adaptive")
        {
            adaptive = true;
            adaptive_rel = (float)std::atof(next("--adaptive"));
            adaptive_max = (uint32_t)std::atoi(next("--adaptive"));
        }
        else if (a == "--load-state") load_state = next("--load-state");
        else if (a == "--save-state") save_state = next("--save-state");
        else if (a == "--devices")
        {
            const std::string list = next("--devices");
            for (size_t p0 = 0; p0 < list.size();) { const size_t p1 = list.find(',', p0); devices.push_back(std::atoi(list.substr(p0, p1 - p0).c_str())); if (p1 == std::string::npos) break; p0 = p1 + 1; }
        }
        else if (a == "--help" || a == "-h")
        {
            std::printf("usage: %s [--width W] [--height H] [--frames N] [--bounces B] [--move] [--slide DX DZ] [--models DIR] [--out file.png] [--temporal file.png [--temporal-rescue] [--temporal-mean-length] [--temporal-demodulate]] [--denoise file.png] [--denoise-albedo file.png] [--follow K] [--mirror-glass] [--aperture A --focus F] [--projection panorama[:SX:SY]|ortho:HEIGHT] [--bake-probes NX NY NZ SPP file.txt] [--bake-lightmap W H SPP PASSES file.txt [--direct] [--adaptive REL MAX] [--lightmap-denoise | --directional] [--baked-view SPP file.png]] [--probe-grid NX NY NZ SPP [--probe-depth R] [--probe-radiance R] --baked-view SPP file.png] [--metal-box] [--checker N] [--emission-checker N] [--normal-ripples N] [--metal-box --roughness-checker N]\n", argv[0]);
            return 0;
        }
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    const bool with_grid = probe_grid[0] && probe_grid[1] && probe_grid[2] && probe_grid[3];
    if (!baked_out.empty() && (((lightmap_out.empty() || !lightmap[2]) && !with_grid) || !baked_spp))
    {
        std::fprintf(stderr, "--baked-view shows the map --bake-lightmap bakes or the volume --probe-grid bakes: it needs one of them, and samples for both\n");
        return 2;
    }
    if ((probe_grid[0] || probe_grid[1] || probe_grid[2] || probe_grid[3]) && (!with_grid || baked_out.empty()))
    {
        std::fprintf(stderr, "--probe-grid NX NY NZ SPP takes four non-zero numbers and lights --baked-view\n");
        return 2;
    }
    if (probe_depth_given && (!with_grid || probe_depth < 2 || probe_depth > 16))
    {
        std::fprintf(stderr, "--probe-depth R takes a map side of 2..16 and goes with --probe-grid\n");
        return 2;
    }
    if (probe_radiance_given && (!with_grid || probe_radiance < 2 || probe_radiance > 16))
    {
        std::fprintf(stderr, "--probe-radiance R takes a map side of 2..16 and goes with --probe-grid\n");
        return 2;
    }
    if (lightmap_denoise && (lightmap_out.empty() || !lightmap[2]))
    {
        std::fprintf(stderr, "--lightmap-denoise filters the map --bake-lightmap bakes: it needs that option, and samples\n");
        return 2;
    }
    if (directional && (lightmap_out.empty() || !lightmap[2] || lightmap_denoise))
    {
        std::fprintf(stderr, "--directional bakes a direction beside the map --bake-lightmap bakes: it needs that option, and samples, and does not go with --lightmap-denoise\n");
        return 2;
    }
    if (direct && (lightmap_out.empty() || !lightmap[2] || directional))
    {
        std::fprintf(stderr, "--direct samples the lights at the texels of the map --bake-lightmap bakes: it needs that option, and samples, and does not go with --directional\n");
        return 2;
    }
    if (gather_given && (!gather || lightmap_out.empty() || !lightmap[2] || directional || adaptive || lightmap_denoise))
    {
        std::fprintf(stderr, "--gather ITERATIONS bakes the map --bake-lightmap bakes by final gather, ITERATIONS >= 1 passes: it needs that option, and samples, and goes with --direct and --baked-view only\n");
        return 2;
    }
    if (adaptive && (lightmap_out.empty() || !lightmap[2] || directional || !(adaptive_rel >= 0.0f) || (adaptive_max != 0 && adaptive_max < 2) ||
                     (adaptive_rel == 0.0f && adaptive_max == 0)))
    {
        std::fprintf(stderr, "--adaptive REL MAX bakes the map --bake-lightmap bakes in rounds of its SPP: it needs that option, and samples, REL >= 0 and MAX of 0 or at least 2 (not both 0: the rounds would not end), and does not go with --directional\n");
        return 2;
    }
    if (normal_ripples && (checker || (!lightmap_out.empty() && !directional)))
    {
        // both want the UVs of cb_main.obj: the checker and the lightmap the planar (x, z) ones, the ripples (x, y + z).  Under --directional
        // the ripples take the bake's planar UVs
        std::fprintf(stderr, "--normal-ripples cannot be combined with --checker, or with --bake-lightmap unless --directional: each sets the UVs of cb_main.obj\n");
        return 2;
    }
    if (roughness_checker && (!metal_box || mirror_glass))
    {
        // the map goes on the GGX metal --metal-box makes of the tall box (a mirror has no roughness), whose UVs no other option sets
        std::fprintf(stderr, "--roughness-checker N puts a roughness map on the box --metal-box turns to metal: it needs that option, and does not go with --mirror-glass\n");
        return 2;
    }
    if (!temporal_out.empty() && (!out.empty() || !denoise_out.empty() || !denoise_albedo_out.empty() || render_mode || gpus > 0 || !devices.empty()))
    {
        // frame_temporal leaves the accumulation alone: there is nothing in it for these to write
        std::fprintf(stderr, "--temporal cannot be combined with --out, --denoise, --denoise-albedo, --render or --gpus: its frames do not accumulate\n");
        return 2;
    }
    if (temporal_option && temporal_out.empty())
    {
        std::fprintf(stderr, "--temporal-rescue, --temporal-mean-length and --temporal-demodulate are options of --temporal\n");
        return 2;
    }
    try
    {
        // Materials  main.rs:77-92
        const Material diffuse_gray = Lambertian::New({0.73f, 0.73f, 0.73f});
        const Material diffuse_green = Lambertian::New({0.12f, 0.45f, 0.15f});
        const Material diffuse_red = Lambertian::New({0.65f, 0.05f, 0.05f});
        const Material light = Emissive::New(Vec3A::splat(15.0f));
        Material main_gray = diffuse_gray, lamp = light;
        auto checker_texture = [](uint32_t n) {
            std::vector<float> texels;
            for (uint32_t j = 0; j < n; ++j)
                for (uint32_t i = 0; i < n; ++i) texels.insert(texels.end(), 3, ((i + j) & 1u) ? 0.2f : 1.0f);
            return Texture::New(n, n, std::move(texels));
        };
        if (checker) main_gray = diffuse_gray.Textured(checker_texture(checker));
        if (emission_checker) lamp = light.EmissionTextured(checker_texture(emission_checker));
        if (normal_ripples)
        {
            const uint32_t n = normal_ripples;
            std::vector<float> texels;
            auto tri = [n](uint32_t i) { const float a = ((float)i + 0.5f) / (float)n; return 0.3f * (4.0f * std::fabs(a - 0.5f) - 1.0f); };
            for (uint32_t j = 0; j < n; ++j)
                for (uint32_t i = 0; i < n; ++i)
                {
                    const float x = tri(i), y = tri(j);
                    const float z = std::sqrt((1.0f - x * x) - y * y);
                    const float v[3] = {x, y, z};
                    for (float c : v) texels.push_back(0.5f * c + 0.5f);
                }
            main_gray = main_gray.NormalMapped(Texture::New(n, n, std::move(texels)));
        }

        Material box_metal = GGX::NewMetal(Vec3A{0.9f, 0.8f, 0.6f}, 0.4f);
        if (roughness_checker)
        {
            const uint32_t n = roughness_checker;
            std::vector<float> texels;
            for (uint32_t j = 0; j < n; ++j)
                for (uint32_t i = 0; i < n; ++i) texels.insert(texels.end(), 3, ((i + j) & 1u) ? 0.6f : 0.1f);
            box_metal = box_metal.RoughnessMapped(Texture::New(n, n, std::move(texels)));
        }

        // Models and BVHs  main.rs:94-117 (the two blocks the reference has commented out stand in for its dragon, whose file it does not ship)
        const std::vector<Affine3A> one{Affine3A::IDENTITY()};
        const Scene scene = Scene::New({
            Model::New(models_dir + "/cb_light.obj", lamp, one),
            Model::New(models_dir + "/cb_main.obj", main_gray, one),
            Model::New(models_dir + "/cb_right.obj", diffuse_red, one),
            Model::New(models_dir + "/cb_left.obj", diffuse_green, one),
            Model::New(models_dir + "/cb_box_tall.obj", mirror_glass ? Specular::New(Vec3A::splat(1.0f)) : metal_box ? box_metal : diffuse_gray, one),
            Model::New(models_dir + "/cb_box_short.obj", mirror_glass ? Dielectric::New(Vec3A::splat(0.95f), 1.5f, std::nullopt) : diffuse_gray, one),
        });

        // Camera  main.rs:119-128
        const Vec3A look_from{0.0f, 50.0f, 1000.0f}, look_at{0.0f, 50.0f, 0.0f};
        const Camera cam = Camera::New(look_from, look_at, 60.0f, (float)width / (float)height, aperture, focus);
        if (gpus > 0 || !devices.empty())
        {
            // several GPUs, one process: rows dealt to the devices in strips, one RCCL gather of the framebuffer (pt_multi)
            if (devices.empty()) for (uint32_t d = 0; d < gpus; ++d) devices.push_back((int32_t)d);
            MultiRenderer multi(scene, cam, width, height, bounces, devices);
            multi.set_projection(projection);
            multi.render(0, 1);                                  // scene upload, RCCL communicator set-up
            multi.reset_accumulation();
            const auto m0 = std::chrono::steady_clock::now();
            multi.render(0, spp);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - m0).count();
            const pt_stats st = multi.stats();
            const double rays = (double)st.rays_closest + (double)st.rays_any + (double)st.rays_light_closest;
            std::printf("{\"gpus\": %zu, \"rccl\": %s, \"spp\": %u, \"width\": %u, \"height\": %u, \"ms\": %.3f, \"Mray_per_s\": %.1f}\n", devices.size(),
                        multi.used_rccl() ? "true" : "false", spp, width, height, 1e3 * sec, rays * (double)spp / (double)(spp + 1) / sec / 1e6);
            if (!out.empty()) multi.write_image(out);
            return 0;
        }
        Renderer renderer(scene, cam, width, height, bounces);
        renderer.set_projection(projection);
        // planar UVs: a vertex's (x, z) over the model's own extent in x and z
        auto planar_uvs = [&](int model) {
            const std::vector<float> p = renderer.model_positions(model);
            float lo[2] = {p[0], p[2]}, hi[2] = {p[0], p[2]};
            for (size_t v = 0; v < p.size() / 3; ++v)
                for (int k = 0; k < 2; ++k) { lo[k] = std::min(lo[k], p[3 * v + 2 * k]); hi[k] = std::max(hi[k], p[3 * v + 2 * k]); }
            std::vector<float> uv;
            for (size_t v = 0; v < p.size() / 3; ++v)
                for (int k = 0; k < 2; ++k) uv.push_back((p[3 * v + 2 * k] - lo[k]) / (hi[k] - lo[k]));
            renderer.set_model_uvs(model, uv);
        };
        if (checker || !lightmap_out.empty()) planar_uvs(1);
        if (emission_checker) planar_uvs(0);
        if (roughness_checker) planar_uvs(4);
        if (normal_ripples && lightmap_out.empty())
        {
            // s = x, t = y + z, each over the model's own extent: no face of the room is degenerate in them
            const std::vector<float> p = renderer.model_positions(1);
            auto st = [&](size_t v, int k) { return k == 0 ? p[3 * v] : p[3 * v + 1] + p[3 * v + 2]; };
            float lo[2] = {st(0, 0), st(0, 1)}, hi[2] = {st(0, 0), st(0, 1)};
            for (size_t v = 0; v < p.size() / 3; ++v)
                for (int k = 0; k < 2; ++k) { lo[k] = std::min(lo[k], st(v, k)); hi[k] = std::max(hi[k], st(v, k)); }
            std::vector<float> uv;
            for (size_t v = 0; v < p.size() / 3; ++v)
                for (int k = 0; k < 2; ++k) uv.push_back((st(v, k) - lo[k]) / (hi[k] - lo[k]));
            renderer.set_model_uvs(1, uv);
        }
        // light probes for a run-time consumer: a regular grid inside the scene's bounds, baked by the path tracer
        auto bake_probes = [&]() -> bool {
            if (probes_out.empty()) return true;
            const std::array<float, 6> box = renderer.root_box();
            std::vector<float> pos;
            float axis[3][2];
            for (int k = 0; k < 3; ++k)
            {
                const float ext = box[3 + k] - box[k], margin = 0.05f * ext;
                axis[k][0] = box[k] + margin;
                axis[k][1] = box[3 + k] - margin;
            }
            auto at = [&](int k, uint32_t i) {
                if (probes[k] < 2) return 0.5f * (axis[k][0] + axis[k][1]);
                const float t = (float)i / (float)(probes[k] - 1), span = axis[k][1] - axis[k][0], step = span * t;
                return axis[k][0] + step;
            };
            for (uint32_t z = 0; z < probes[2]; ++z)
                for (uint32_t y = 0; y < probes[1]; ++y)
                    for (uint32_t x = 0; x < probes[0]; ++x) { pos.push_back(at(0, x)); pos.push_back(at(1, y)); pos.push_back(at(2, z)); }
            std::vector<float> sh;
            renderer.bake_probes(pos, probe_spp, sh);
            std::FILE* f = std::fopen(probes_out.c_str(), "w");
            if (!f) { std::fprintf(stderr, "cannot write %s\n", probes_out.c_str()); return false; }
            for (size_t j = 0; j < pos.size() / 3; ++j)
                for (int k = 0; k < 27; ++k) std::fprintf(f, "%a%c", (double)sh[j * 27 + k], k == 26 ? '\n' : ' ');
            std::fclose(f);
            return true;
        };
        // a lightmap for a run-time consumer: the room's shell under the planar UVs above, baked by the path tracer and dilated
        auto bake_lightmap = [&]() -> bool {
            if (lightmap_out.empty()) return true;
            std::vector<float> sums, grad;
            std::vector<uint8_t> cov;
            const uint32_t light_keys = lightmap[0] * lightmap[1]; // --direct: the light samples' streams, behind the gather samples' [0, W * H)
            if (directional)
            {
                // the first moments beside the sums, their gradient, and its dilation with a coverage of its own (the map's is dilated below)
                std::vector<float> dirs;
                cov = renderer.bake_lightmap_directional(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, dirs, 0, 0, 0.25f);
                grad = renderer.lightmap_gradient(1, 0, lightmap[0], lightmap[1], lightmap[2], dirs, true);
                std::vector<uint8_t> grad_cov = cov;
                renderer.dilate_lightmap_directional(lightmap[0], lightmap[1], lightmap[3], grad, grad_cov);
            }
            else if (adaptive)
            {
                // rounds of SPP samples for the texels the criterion still selects; the means are each texel's sums over ITS OWN count, taken
                // before anything is dilated (a dilated raw sum would mix neighbours with different denominators)
                std::vector<float> sumsq;
                std::vector<uint32_t> counts;
                const pt_adaptive crit{adaptive_rel, 0.0f, 2u, adaptive_max};
                uint64_t rays = 0, rounds = 0;
                for (uint32_t n = 1; n != 0; ++rounds)
                {
                    n = direct ? renderer.bake_lightmap_adaptive_direct(1, 0, lightmap[0], lightmap[1], lightmap[2], crit, sums, sumsq, counts, light_keys, &cov, 0, 0.25f)
                               : renderer.bake_lightmap_adaptive(1, 0, lightmap[0], lightmap[1], lightmap[2], crit, sums, sumsq, counts, &cov, 0, 0.25f);
                    rays += (uint64_t)n * lightmap[2];
                }
                uint64_t covered = 0, total = 0;
                for (size_t k = 0; k < cov.size(); ++k) { covered += cov[k] ? 1u : 0u; total += cov[k] ? counts[k] : 0u; }
                std::printf("{\"adaptive_rounds\": %llu, \"rays\": %llu, \"covered\": %llu, \"mean_count\": %.3f}\n", (unsigned long long)(rounds - 1),
                            (unsigned long long)rays, (unsigned long long)covered, covered ? (double)total / (double)covered : 0.0);
                sums = lightmap_denoise ? renderer.denoise_lightmap_counts(1, 0, lightmap[0], lightmap[1], sums, sumsq, counts) : ptmi::Renderer::lightmap_means(sums, counts);
            }
            else if (lightmap_denoise)
            {
                // the moments steer the filter's luminance term; what it returns are texel means, and those are what is dilated, written and set
                std::vector<float> sumsq;
                cov = direct ? renderer.bake_lightmap_direct(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, &sumsq, light_keys, 0, 0, 0.25f)
                             : renderer.bake_lightmap_moments(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, sumsq, 0, 0, 0.25f);
                sums = renderer.denoise_lightmap(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, sumsq);
            }
            else if (gather)
            {
                // the final-gather loop on the one placement: every pass bakes the shell from the map set by the pass before (the first from
                // whatever is set: nothing), its gather rays ending in that map after at most two mirror or glass hops, black where no map
                // is; all but the last pass are divided, dilated and set here, the last below like every other bake
                for (uint32_t pass = 0; pass < gather; ++pass)
                {
                    sums.clear();
                    cov = renderer.bake_lightmap_gather(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, nullptr, direct, direct ? light_keys : 0u, 2u, {0.0f, 0.0f, 0.0f}, 0,
                                                        0, 0.25f);
                    if (pass + 1 == gather) break;
                    std::vector<float> means = sums;
                    std::vector<uint8_t> filled = cov;
                    for (float& m : means) m = m / (float)lightmap[2];
                    renderer.dilate_lightmap(lightmap[0], lightmap[1], lightmap[3], means, filled);
                    renderer.set_lightmap(1, 0, lightmap[0], lightmap[1], means);
                }
            }
            else if (direct) cov = renderer.bake_lightmap_direct(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, nullptr, light_keys, 0, 0, 0.25f);
            else cov = renderer.bake_lightmap(1, 0, lightmap[0], lightmap[1], lightmap[2], sums, 0, 0, 0.25f);
            renderer.dilate_lightmap(lightmap[0], lightmap[1], lightmap[3], sums, cov);
            std::FILE* f = std::fopen(lightmap_out.c_str(), "w");
            if (!f) { std::fprintf(stderr, "cannot write %s\n", lightmap_out.c_str()); return false; }
            for (size_t k = 0; k < cov.size(); ++k) std::fprintf(f, "%u %a %a %a\n", (unsigned)cov[k], (double)sums[3 * k], (double)sums[3 * k + 1], (double)sums[3 * k + 2]);
            std::fclose(f);
            if (baked_out.empty()) return true;
            // ... and its consumer: the map's texel means on the shell (baked_view shades the followed first hits from it)
            if (!lightmap_denoise && !adaptive)
                for (float& s : sums) s = s / (float)lightmap[2];
            renderer.set_lightmap(1, 0, lightmap[0], lightmap[1], sums);
            if (directional) renderer.set_lightmap_directional(1, 0, lightmap[0], lightmap[1], grad);
            return true;
        };
        // the baked view, after bake_lightmap: under --probe-grid an irradiance volume over the scene's bounds inset by half a cell lights
        // what the map (if any) does not
        auto baked_view = [&]() {
            if (baked_out.empty()) return;
            if (with_grid)
            {
                const std::array<float, 6> box = renderer.root_box();
                pt_probe_grid g{};
                for (int k = 0; k < 3; ++k)
                {
                    g.count[k] = probe_grid[k];
                    g.cell[k] = (box[3 + k] - box[k]) / (float)probe_grid[k];
                    g.origin[k] = box[k] + 0.5f * g.cell[k];
                }
                renderer.bake_probe_grid(g, probe_grid[3], 0.25f, probe_depth, 0.0f, 0.0f, false, probe_radiance);
            }
            renderer.render_baked(0, baked_spp, follow);
            renderer.write_baked_image(baked_out);
        };
        // the demodulated denoiser on samples [first, first + count) of the frame: guides of the last sample, the mean albedo of all of them
        auto denoise_albedo = [&](uint32_t first, uint32_t count) {
            renderer.render_guides_followed(first + count - 1, follow);
            renderer.accumulate_albedo_followed(first, count, follow);
            renderer.denoise_albedo(PT_ALBEDO_MEAN);
            renderer.write_denoised_image(denoise_albedo_out);
        };
        if (render_mode)
        {
            // checkpoint / resume: the state file is {width, height, data rgba, position xyzt, id} of the frame as it lies on the device
            if (!load_state.empty())
            {
                std::FILE* f = std::fopen(load_state.c_str(), "rb");
                uint32_t wh[2] = {0, 0};
                Frame fr;
                const size_t px = (size_t)width * height;
                fr.data.resize(px * 4); fr.position.resize(px * 4); fr.id.resize(px);
                const bool ok = f && std::fread(wh, 4, 2, f) == 2 && wh[0] == width && wh[1] == height && std::fread(fr.data.data(), 4, px * 4, f) == px * 4 &&
                                std::fread(fr.position.data(), 4, px * 4, f) == px * 4 && std::fread(fr.id.data(), 4, px, f) == px;
                if (f) std::fclose(f);
                if (!ok) { std::fprintf(stderr, "cannot read a %ux%u frame state from %s\n", width, height, load_state.c_str()); return 1; }
                renderer.write_accumulation(fr);
            }
            renderer.render(render_first, render_count);
            if (!save_state.empty())
            {
                const Frame fr = renderer.read_frame();
                std::FILE* f = std::fopen(save_state.c_str(), "wb");
                const uint32_t wh[2] = {width, height};
                const size_t px = (size_t)width * height;
                const bool ok = f && std::fwrite(wh, 4, 2, f) == 2 && std::fwrite(fr.data.data(), 4, px * 4, f) == px * 4 && std::fwrite(fr.position.data(), 4, px * 4, f) == px * 4 &&
                                std::fwrite(fr.id.data(), 4, px, f) == px;
                if (f) std::fclose(f);
                if (!ok) { std::fprintf(stderr, "cannot write %s\n", save_state.c_str()); return 1; }
            }
            std::printf("{\"first_sample\": %u, \"samples\": %u, \"width\": %u, \"height\": %u}\n", render_first, render_count, width, height);
            if (!out.empty()) renderer.write_image(out);
            if (!denoise_albedo_out.empty() && render_count) denoise_albedo(render_first, render_count);
            if (!bake_probes() || !bake_lightmap()) return 1;
            baked_view();
            return 0;
        }
        Mat4 last_inv_proj = renderer.inv_projection();

        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t frame = 0; frame < frames; ++frame)
        {
            if (move && frame >= frames / 2)
            {
                // what Camera::input would receive from winit: a key held down and a slow mouse drag, dt = 1/60 s scaled to the
                // reference's sensitivities (camera.rs:35,43)
                renderer.input(PT_EV_KEY_W, 0.0f, 0.0f, 2.0e-6f);
                renderer.input(PT_EV_MOUSE_MOTION, 1.0f, 0.25f, 1.0e-6f);
            }
            if (slide && frame >= 1)
            {
                // a pure translation passes Model::new's rigid assert whatever its size (model.rs:40-44)
                const float f = (float)frame;
                renderer.set_instances(5, {Affine3A{{1, 0, 0, f * slide_dx, 0, 1, 0, 0.0f, 0, 0, 1, f * slide_dz}}});
            }
            if (!temporal_out.empty() && temporal_option) renderer.frame_temporal(frame, last_inv_proj, temporal);
            else if (!temporal_out.empty()) renderer.frame_temporal(frame, last_inv_proj);
            else if (slide) renderer.frame_moving(frame, last_inv_proj);
            else renderer.frame(frame, last_inv_proj);       // the pixel loop + state.update   main.rs:181-215
            last_inv_proj = renderer.inv_projection();       // main.rs:216
        }
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const pt_stats st = renderer.stats();
        const double rays = (double)st.rays_closest + (double)st.rays_any + (double)st.rays_light_closest;
        std::printf("{\"frames\": %u, \"width\": %u, \"height\": %u, \"ms_per_frame\": %.3f, \"Mray_per_s\": %.1f}\n", frames, width, height,
                    1e3 * seconds / (frames ? frames : 1), rays / seconds / 1e6);
        if (!out.empty()) renderer.write_image(out);         // ImageHelper::write_image
        if (!temporal_out.empty() && frames) renderer.write_denoised_image(temporal_out);
        if (!denoise_out.empty() && frames)
        {
            // the interactive recipe: guides of the last frame's sample, then the filter (pt_api.h)
            renderer.render_guides_followed(frames - 1, follow);
            renderer.denoise();
            renderer.write_denoised_image(denoise_out);
        }
        if (!denoise_albedo_out.empty() && frames) denoise_albedo(0, frames);
        if (!bake_probes() || !bake_lightmap()) return 1;
        baked_view();
    }
    catch (const Error& e)
    {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
