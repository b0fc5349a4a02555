// Helper of tools/rays_bench.py: one timed measurement in one process, against the libptmi.so named on the command line (loaded with
// dlopen, so that the same binary times another build's library, e.g. the parent commit's, which lacks the newer entry points).
//
//   rays_bench_helper LIB MODELS_DIR render W H SPP REPS          pt_render_device of the Cornell frame under the lens 40 / 950, no primary cull
//   rays_bench_helper LIB MODELS_DIR rays   W H SPP REPS [shuffle] [check]
//                                                                  the same frame's camera rays (pt_primary_ray, pixel-major, a pixel's samples
//                                                                  consecutive) through pt_integrate_rays_device; shuffle: in random order;
//                                                                  check: first compare the radiance with pt_render_samples word for word
//   rays_bench_helper LIB MODELS_DIR probes N SPP                  pt_bake_probes of an N x N x N grid, SPP samples each
// Prints one JSON line.  Each timed window is REPS calls after one warm-up call and ends in pt_synchronize.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../include/pt_api.h"

static void* g_lib = nullptr;
template <class F> static F sym(const char* name, bool required = true)
{
    void* p = dlsym(g_lib, name);
    if (!p && required) { std::fprintf(stderr, "%s: not in the library\n", name); std::exit(3); }
    return reinterpret_cast<F>(p);
}
#define PT_FN(name) static auto name##_ = sym<decltype(&name)>(#name)
static void ok(int r, pt_ctx* c, const char* what)
{
    if (r >= 0) return;
    std::fprintf(stderr, "%s: %d %s\n", what, r, sym<decltype(&pt_last_error)>("pt_last_error")(c));
    std::exit(1);
}
static void hip_ok(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e));
    std::exit(1);
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv)
{
    if (argc < 6) { std::fprintf(stderr, "usage: see the head of tools/rays_bench.cpp\n"); return 2; }
    const std::string lib = argv[1], models = argv[2], mode = argv[3];
    g_lib = dlopen(lib.c_str(), RTLD_NOW | RTLD_GLOBAL);
    if (!g_lib) { std::fprintf(stderr, "%s\n", dlerror()); return 3; }
    PT_FN(pt_create); PT_FN(pt_destroy); PT_FN(pt_add_material); PT_FN(pt_add_model_obj); PT_FN(pt_build); PT_FN(pt_set_camera); PT_FN(pt_set_lens);
    PT_FN(pt_render_device); PT_FN(pt_synchronize); PT_FN(pt_primary_ray); PT_FN(pt_render_samples); PT_FN(pt_active_pixels); PT_FN(pt_get_stats);
    PT_FN(pt_reset_stats);
    const bool probes = mode == "probes";
    const uint32_t W = probes ? 64u : (uint32_t)std::atoi(argv[4]), H = probes ? 64u : (uint32_t)std::atoi(argv[5]);
    pt_config cfg{};
    cfg.width = W; cfg.height = H; cfg.max_bounces = 8; cfg.n_sobol = 512; cfg.enable_nee = 1; cfg.seed = 0x5EED5EEDull; cfg.world_size = 1; cfg.strip_rows = 4;
    cfg.device = -1; cfg.flags = PT_FLAG_NO_PRIMARY_CULL;
    pt_ctx* c = pt_create_(&cfg);
    if (!c) return 1;
    // the Cornell box of examples/headless.cpp
    const char* files[6] = {"cb_light", "cb_main", "cb_right", "cb_left", "cb_box_tall", "cb_box_short"};
    const float colours[4][3] = {{15.0f, 15.0f, 15.0f}, {0.73f, 0.73f, 0.73f}, {0.65f, 0.05f, 0.05f}, {0.12f, 0.45f, 0.15f}};
    const int mat_of[6] = {0, 1, 2, 3, 1, 1};
    for (int m = 0; m < 4; ++m)
    {
        pt_material_desc d{};
        d.kind = m == 0 ? 1 : 0; // emissive, lambertian (pt_types.h: MAT_*)
        std::memcpy(d.colour, colours[m], 12);
        d.ior = 1.0f;
        ok(pt_add_material_(c, &d), c, "pt_add_material");
    }
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int m = 0; m < 6; ++m) ok(pt_add_model_obj_(c, (models + "/" + files[m] + ".obj").c_str(), mat_of[m], identity, 1), c, "pt_add_model_obj");
    ok(pt_build_(c), c, "pt_build");
    const float eye[3] = {0.0f, 50.0f, 1000.0f}, target[3] = {0.0f, 50.0f, 0.0f};
    ok(pt_set_camera_(c, eye, target, 60.0f, (float)W / (float)H), c, "pt_set_camera");
    ok(pt_set_lens_(c, 40.0f, 950.0f), c, "pt_set_lens");

    if (mode == "render")
    {
        const uint32_t spp = (uint32_t)std::atoi(argv[6]), reps = (uint32_t)std::atoi(argv[7]);
        ok(pt_render_device_(c, 0, spp), c, "pt_render_device");
        ok(pt_synchronize_(c), c, "pt_synchronize");
        const double t0 = now_ms();
        for (uint32_t r = 0; r < reps; ++r) ok(pt_render_device_(c, 0, spp), c, "pt_render_device");
        ok(pt_synchronize_(c), c, "pt_synchronize");
        const double ms = (now_ms() - t0) / reps;
        std::printf("{\"mode\": \"render\", \"width\": %u, \"height\": %u, \"spp\": %u, \"reps\": %u, \"paths\": %llu, \"ms_per_call\": %.4f}\n", W, H, spp, reps,
                    (unsigned long long)W * H * spp, ms);
    }
    else if (mode == "rays")
    {
        const uint32_t spp = (uint32_t)std::atoi(argv[6]), reps = (uint32_t)std::atoi(argv[7]);
        bool shuffle = false, check = false;
        for (int i = 8; i < argc; ++i) { shuffle |= !std::strcmp(argv[i], "shuffle"); check |= !std::strcmp(argv[i], "check"); }
        auto integrate = sym<int (*)(pt_ctx*, uint64_t, const float*, const float*, const uint32_t*, const uint32_t*, const pt_rays_params*, float*, float*, uint8_t*)>(
            "pt_integrate_rays_device");
        const size_t px = (size_t)W * H, n = px * spp;
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        if (shuffle) std::shuffle(order.begin(), order.end(), std::mt19937_64(12345));
        std::vector<float> o(3 * n), d(3 * n);
        std::vector<uint32_t> key(n), sample(n);
        uint32_t draws = 0;
        for (size_t i = 0; i < n; ++i)
        {
            const uint32_t p = order[i] / spp, s = order[i] % spp; // pixel-major, a pixel's samples consecutive
            key[i] = p; sample[i] = s;
            ok(pt_primary_ray_(c, p, s, &o[3 * i], &d[3 * i], &draws), c, "pt_primary_ray");
        }
        float *d_o, *d_d, *d_rad;
        uint32_t *d_key, *d_sample;
        hip_ok(hipMalloc(&d_o, n * 12), "hipMalloc"); hip_ok(hipMalloc(&d_d, n * 12), "hipMalloc"); hip_ok(hipMalloc(&d_rad, n * 16), "hipMalloc");
        hip_ok(hipMalloc(&d_key, n * 4), "hipMalloc"); hip_ok(hipMalloc(&d_sample, n * 4), "hipMalloc");
        hip_ok(hipMemcpy(d_o, o.data(), n * 12, hipMemcpyHostToDevice), "hipMemcpy"); hip_ok(hipMemcpy(d_d, d.data(), n * 12, hipMemcpyHostToDevice), "hipMemcpy");
        hip_ok(hipMemcpy(d_key, key.data(), n * 4, hipMemcpyHostToDevice), "hipMemcpy"); hip_ok(hipMemcpy(d_sample, sample.data(), n * 4, hipMemcpyHostToDevice), "hipMemcpy");
        pt_rays_params prm{};
        prm.draws_consumed = draws;
        ok(integrate(c, n, d_o, d_d, d_key, d_sample, &prm, d_rad, nullptr, nullptr), c, "pt_integrate_rays_device"); // warm-up
        long long differing = -1;
        if (check)
        {
            std::vector<uint32_t> got(4 * n), want(4 * n);
            hip_ok(hipMemcpy(got.data(), d_rad, n * 16, hipMemcpyDeviceToHost), "hipMemcpy");
            ok(pt_render_samples_(c, 0, spp, reinterpret_cast<float*>(want.data())), c, "pt_render_samples");
            differing = 0;
            for (size_t i = 0; i < n; ++i)
                differing += std::memcmp(&got[4 * i], &want[4 * ((size_t)sample[i] * px + key[i])], 16) != 0;
            if (differing) { std::fprintf(stderr, "%lld of %zu rays differ from pt_render_samples\n", differing, n); return 1; }
        }
        ok(pt_synchronize_(c), c, "pt_synchronize");
        const double t0 = now_ms();
        for (uint32_t r = 0; r < reps; ++r) ok(integrate(c, n, d_o, d_d, d_key, d_sample, &prm, d_rad, nullptr, nullptr), c, "pt_integrate_rays_device");
        ok(pt_synchronize_(c), c, "pt_synchronize");
        const double ms = (now_ms() - t0) / reps;
        std::printf("{\"mode\": \"%s\", \"width\": %u, \"height\": %u, \"spp\": %u, \"reps\": %u, \"paths\": %zu, \"ms_per_call\": %.4f, \"rays_differing_from_render_samples\": %lld}\n",
                    shuffle ? "rays_shuffled" : "rays", W, H, spp, reps, n, ms, differing);
    }
    else if (probes)
    {
        const uint32_t N = (uint32_t)std::atoi(argv[4]), spp = (uint32_t)std::atoi(argv[5]);
        auto bake = sym<int (*)(pt_ctx*, uint32_t, const float*, const pt_probe_params*, float*)>("pt_bake_probes");
        uint32_t rect[4];
        float box[6];
        ok(pt_active_pixels_(c, rect, box), c, "pt_active_pixels");
        std::vector<float> pos;
        for (uint32_t z = 0; z < N; ++z)
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t x = 0; x < N; ++x)
                {
                    const uint32_t g[3] = {x, y, z};
                    for (int k = 0; k < 3; ++k)
                    {
                        const float ext = box[3 + k] - box[k], lo = box[k] + 0.05f * ext, hi = box[3 + k] - 0.05f * ext;
                        pos.push_back(N > 1 ? lo + (hi - lo) * ((float)g[k] / (float)(N - 1)) : 0.5f * (lo + hi));
                    }
                }
        const uint32_t n_probes = N * N * N;
        std::vector<float> sh((size_t)n_probes * 27, 0.0f);
        pt_probe_params warm{0, 16, 0, 0}, prm{0, spp, 0, 0};
        ok(bake(c, n_probes, pos.data(), &warm, sh.data()), c, "pt_bake_probes");
        std::fill(sh.begin(), sh.end(), 0.0f);
        ok(pt_reset_stats_(c), c, "pt_reset_stats");
        const double t0 = now_ms();
        ok(bake(c, n_probes, pos.data(), &prm, sh.data()), c, "pt_bake_probes");
        const double ms = now_ms() - t0;
        pt_stats st{};
        ok(pt_get_stats_(c, &st), c, "pt_get_stats");
        const double rays = (double)st.rays_closest + (double)st.rays_any + (double)st.rays_light_closest;
        std::printf("{\"mode\": \"probes\", \"probes\": %u, \"samples\": %u, \"paths\": %llu, \"ms\": %.3f, \"Mray_per_s\": %.1f, \"sh0_of_probe0\": [%g, %g, %g]}\n", n_probes, spp,
                    (unsigned long long)n_probes * spp, ms, rays / ms / 1e3, sh[0], sh[1], sh[2]);
    }
    else { std::fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
    pt_destroy_(c);
    return 0;
}
