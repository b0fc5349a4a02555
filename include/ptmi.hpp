// ptmi.hpp — C++17 host side above the C-ABI (include/pt_api.h), mirroring the reference's own setup and per-frame calls so that a
// driver reads like src/main.rs.  Header-only; link with -lptmi.  The reference is Rust: `Type::new(..)` becomes `Type::New(..)`
// (`new` is a C++ keyword), `Result`/`unwrap` panics become ptmi::Error.  Everything here is plumbing: no arithmetic of the path.
//
//   reference (file:line)                                   here
//   Volume::new(absorption, k, c, g)      volume.rs:136      ptmi::Volume::New
//   Lambertian::new(albedo)               material.rs:99     ptmi::Lambertian::New
//   Emissive::new(emitted)                material.rs:126    ptmi::Emissive::New
//   Specular::new(colour)                 material.rs:146    ptmi::Specular::New
//   GGX::new_metal / new_dielectric       material.rs:290,305 ptmi::GGX::NewMetal / NewDielectric
//   Dielectric::new(colour, ior, volume)  material.rs:475    ptmi::Dielectric::New
//   Model::new(path, material, matrices)  model.rs:36        ptmi::Model::New            (+ Model::FromTriangles for triangle soups)
//   Scene::new(models)                    scene.rs:21        ptmi::Scene::New
//   Camera::new(origin, target, fov, aspect, aperture, focus)  camera.rs:17   ptmi::Camera::New (the thin lens the reference reserves)
//   Camera::input(event, window, dt)      camera.rs:56       ptmi::Renderer::input
//   the pixel loop + state.update(..)     main.rs:181-216    ptmi::Renderer::frame
//   (cam.matrix * cam.inv_projection).inverse()  main.rs:128 ptmi::Renderer::inv_projection
//   state.render()                        state.rs:629       ptmi::Renderer::present
//   ImageHelper::write_image              image_helper.rs:37 ptmi::Renderer::write_image
// The library's own additions have no line of the reference: ptmi::Texture with Material::Textured and Model::WithUVs (pt_add_texture),
// Material::EmissionTextured (pt_set_material_emission_texture), Material::NormalMapped (pt_set_material_normal_texture),
// Material::RoughnessMapped (pt_set_material_roughness_texture).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pt_api.h"

namespace ptmi {

struct Error : std::runtime_error
{
    int code;
    Error(int c, const std::string& what) : std::runtime_error("libptmi error " + std::to_string(c) + ": " + what), code(c) {}
};

struct Vec3A
{
    float x, y, z;
    static Vec3A splat(float v) { return {v, v, v}; }
};

// row-major 3x4, as pt_add_model takes it (glam::Affine3A)
struct Affine3A
{
    std::array<float, 12> m;
    static Affine3A IDENTITY() { return {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}}; }
};
using Mat4 = std::array<float, 16>; // column-major, as glam::Mat4

struct Volume
{
    Vec3A absorption;
    float k, c, g;
    static Volume New(Vec3A absorption, float k, float c, float g) { return {absorption, k, c, g}; }
};

// w x h linear-RGB texels, row-major (pt_add_texture).  Copies share the texels, and two textures are the same texture when they share
// them: materials that were given the same Texture reference one texture of the scene.
struct Texture
{
    uint32_t w = 0, h = 0;
    std::shared_ptr<const std::vector<float>> rgb; // w * h * 3
    static Texture New(uint32_t w, uint32_t h, std::vector<float> rgb_linear) { return {w, h, std::make_shared<const std::vector<float>>(std::move(rgb_linear))}; }
};

struct Material
{
    pt_material_desc d{};
    std::optional<Texture> texture; // surface colour = colour * bilinear texel at the hit's UV; any kind but Emissive
    Material Textured(const Texture& t) const { Material m = *this; m.texture = t; return m; }
    std::optional<Texture> emission_texture; // Emissive only: emitted colour = colour * bilinear texel at the light's UV (a textured area light)
    Material EmissionTextured(const Texture& t) const { Material m = *this; m.emission_texture = t; return m; }
    std::optional<Texture> normal_texture; // tangent-space normal map: the shading normal is perturbed by its bilinear texel; any kind but Emissive
    Material NormalMapped(const Texture& t) const { Material m = *this; m.normal_texture = t; return m; }
    std::optional<Texture> roughness_texture; // the hit's linear roughness = its bilinear texel's first component, `roughness` is not read; the two GGX kinds only
    Material RoughnessMapped(const Texture& t) const { Material m = *this; m.roughness_texture = t; return m; }
    bool operator==(const Material& o) const
    {
        return (texture ? texture->rgb : nullptr) == (o.texture ? o.texture->rgb : nullptr) &&
               (normal_texture ? normal_texture->rgb : nullptr) == (o.normal_texture ? o.normal_texture->rgb : nullptr) &&
               (roughness_texture ? roughness_texture->rgb : nullptr) == (o.roughness_texture ? o.roughness_texture->rgb : nullptr) &&
               (emission_texture ? emission_texture->rgb : nullptr) == (o.emission_texture ? o.emission_texture->rgb : nullptr) && d.kind == o.d.kind && d.colour[0] == o.d.colour[0] && d.colour[1] == o.d.colour[1] && d.colour[2] == o.d.colour[2] &&
               d.roughness == o.d.roughness && d.ior == o.d.ior && d.has_volume == o.d.has_volume &&
               (!d.has_volume || (d.vol_absorption[0] == o.d.vol_absorption[0] && d.vol_absorption[1] == o.d.vol_absorption[1] &&
                                  d.vol_absorption[2] == o.d.vol_absorption[2] && d.vol_k == o.d.vol_k && d.vol_c == o.d.vol_c && d.vol_g == o.d.vol_g));
    }
};
namespace detail {
inline Material material(int kind, Vec3A colour, float roughness = 0.0f, float ior = 1.0f, const std::optional<Volume>& v = std::nullopt)
{
    Material m;
    m.d.kind = kind;
    m.d.colour[0] = colour.x; m.d.colour[1] = colour.y; m.d.colour[2] = colour.z;
    m.d.roughness = roughness;
    m.d.ior = ior;
    if (v)
    {
        m.d.has_volume = 1;
        m.d.vol_absorption[0] = v->absorption.x; m.d.vol_absorption[1] = v->absorption.y; m.d.vol_absorption[2] = v->absorption.z;
        m.d.vol_k = v->k; m.d.vol_c = v->c; m.d.vol_g = v->g;
    }
    return m;
}
} // namespace detail
struct Lambertian { static Material New(Vec3A albedo) { return detail::material(PT_LAMBERTIAN, albedo); } };
struct Emissive { static Material New(Vec3A emitted) { return detail::material(PT_EMISSIVE, emitted); } };
struct Specular { static Material New(Vec3A colour) { return detail::material(PT_SPECULAR, colour); } };
struct GGX
{
    static Material NewMetal(Vec3A colour, float roughness) { return detail::material(PT_GGX_METAL, colour, roughness); }
    static Material NewDielectric(Vec3A colour, float roughness, float ior, std::optional<Volume> volume)
    {
        return detail::material(PT_GGX_DIELECTRIC, colour, roughness, ior, volume);
    }
};
struct Dielectric
{
    static Material New(Vec3A colour, float ior, std::optional<Volume> volume) { return detail::material(PT_DIELECTRIC, colour, 0.0f, ior, volume); }
};

struct Model
{
    std::string path;                     // OBJ file read by the library's load_obj (blas.rs:44-131) ...
    std::vector<float> positions, normals; // ... or a triangle soup, 9 floats per triangle each
    Material material;
    std::vector<Affine3A> matrices;
    std::vector<float> uvs;               // 6 floats per triangle (three UVs, load order), or empty: (0, 0) everywhere, or the OBJ's `vt`
    static Model New(std::string file_path, Material material, std::vector<Affine3A> matrices) { return {std::move(file_path), {}, {}, material, std::move(matrices), {}}; }
    static Model FromTriangles(std::vector<float> positions, std::vector<float> normals, Material material, std::vector<Affine3A> matrices)
    {
        return {"", std::move(positions), std::move(normals), material, std::move(matrices), {}};
    }
    Model WithUVs(std::vector<float> uv) const { Model m = *this; m.uvs = std::move(uv); return m; }
};

struct Scene
{
    std::vector<Model> models;
    static Scene New(std::vector<Model> models) { return {std::move(models)}; }
};

struct Camera
{
    Vec3A origin, target;
    float fov, aspect_ratio;
    float aperture, focus; // thin lens (pt_set_lens): lens DIAMETER in world units, 0 = pinhole; distance of the plane of focus
    static Camera New(Vec3A origin, Vec3A target, float fov, float aspect_ratio, float aperture, float focus) { return {origin, target, fov, aspect_ratio, aperture, focus}; }
};

struct Frame
{
    std::vector<float> data, position; // W*H*4 each: this frame's (rgb, 1) and first-hit (xyz, t)   main.rs:135-136
    std::vector<uint32_t> id;          // W*H: (old << 16) | new                                        main.rs:137,206
};

// what Renderer::integrate_rays returns, per ray: the finalised sample (rgb, 1), the first hit (xyz, t) and its id byte (255 = miss)
struct RayResults
{
    std::vector<float> radiance, position; // n * 4 each
    std::vector<uint8_t> id;               // n
};

// what Renderer::baked_rays returns, per ray: the baked sample and the hop its chain ended at (r, g, b, hop), and the first hit's id byte
struct BakedRays
{
    std::vector<float> rgbh; // n * 4
    std::vector<uint8_t> id; // n
};
inline pt_baked_params baked_params(uint32_t max_hops, const std::array<float, 3>& unlit)
{
    pt_baked_params p{};
    p.max_hops = max_hops;
    p.unlit[0] = unlit[0]; p.unlit[1] = unlit[1]; p.unlit[2] = unlit[2];
    return p;
}

// Scene::new on a context: materials in first-use order, models, pt_build
inline void upload(pt_ctx* ctx_, const Scene& scene)
{
    auto check = [&](int r) { if (r < 0) throw Error(r, pt_last_error(ctx_)); return r; };
        std::vector<Material> mats; // distinct materials in first-use order
        std::vector<std::shared_ptr<const std::vector<float>>> texs; // distinct textures in first-use order
        for (const Model& m : scene.models)
        {
            size_t idx = 0;
            while (idx < mats.size() && !(mats[idx] == m.material)) ++idx;
            if (idx == mats.size())
            {
                mats.push_back(m.material);
                check(pt_add_material(ctx_, &m.material.d));
                auto texture_index = [&](const Texture& t) {
                    size_t ti = 0;
                    while (ti < texs.size() && texs[ti] != t.rgb) ++ti;
                    if (ti == texs.size())
                    {
                        if (!t.rgb || t.rgb->size() != (size_t)t.w * t.h * 3) throw Error(PT_ERR_ARG, "Texture: not w * h * 3 floats");
                        texs.push_back(t.rgb);
                        check(pt_add_texture(ctx_, t.w, t.h, t.rgb->data()));
                    }
                    return (int)ti;
                };
                if (m.material.texture) check(pt_set_material_texture(ctx_, (int)idx, texture_index(*m.material.texture)));
                if (m.material.emission_texture) check(pt_set_material_emission_texture(ctx_, (int)idx, texture_index(*m.material.emission_texture)));
                if (m.material.normal_texture) check(pt_set_material_normal_texture(ctx_, (int)idx, texture_index(*m.material.normal_texture)));
                if (m.material.roughness_texture) check(pt_set_material_roughness_texture(ctx_, (int)idx, texture_index(*m.material.roughness_texture)));
            }
            const float* mat = m.matrices.empty() ? nullptr : m.matrices[0].m.data();
            const uint32_t n_inst = (uint32_t)m.matrices.size();
            int model;
            if (!m.path.empty()) model = check(pt_add_model_obj(ctx_, m.path.c_str(), (int)idx, mat, n_inst));
            else model = check(pt_add_model(ctx_, m.positions.data(), m.normals.data(), (uint32_t)(m.positions.size() / 9), (int)idx, mat, n_inst));
            if (!m.uvs.empty()) check(pt_set_model_uvs(ctx_, model, m.uvs.data(), (uint32_t)(m.uvs.size() / 6)));
        }
        check(pt_build(ctx_));
}

// owns a pt_ctx: Scene::new + the wavefront state of main.rs's loop
class Renderer
{
public:
    Renderer(const Scene& scene, const Camera& cam, uint32_t width, uint32_t height, uint32_t max_bounces, uint32_t n_sobol = 512, bool enable_nee = true,
             uint64_t seed = 0x5EED5EEDull, int device = -1, uint32_t flags = 0)
    {
        pt_config cfg{};
        cfg.width = width; cfg.height = height; cfg.max_bounces = max_bounces; cfg.n_sobol = n_sobol; cfg.enable_nee = enable_nee ? 1u : 0u;
        cfg.seed = seed; cfg.rank = 0; cfg.world_size = 1; cfg.strip_rows = 4; cfg.batch_spp = 0; cfg.device = device; cfg.flags = flags;
        ctx_ = pt_create(&cfg);
        if (!ctx_) throw Error(PT_ERR_ARG, "pt_create failed (bad configuration)");
        width_ = width; height_ = height;
        upload(ctx_, scene);
        set_camera(cam);
    }
    ~Renderer() { if (ctx_) pt_destroy(ctx_); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void set_camera(const Camera& c)
    {
        const float eye[3] = {c.origin.x, c.origin.y, c.origin.z}, tgt[3] = {c.target.x, c.target.y, c.target.z};
        check(pt_set_camera(ctx_, eye, tgt, c.fov, c.aspect_ratio));
        check(pt_set_lens(ctx_, c.aperture, c.focus));
    }
    // panoramic / orthographic camera (pt_set_projection); the projection survives set_camera and input, and excludes a lens
    void set_projection(const pt_projection& p) { check(pt_set_projection(ctx_, &p)); }
    void set_panorama(float span_x_deg = 0.0f, float span_y_deg = 0.0f) { pt_projection p{}; p.kind = PT_PROJ_PANORAMA; p.span_x_deg = span_x_deg; p.span_y_deg = span_y_deg; set_projection(p); }
    void set_orthographic(float height) { pt_projection p{}; p.kind = PT_PROJ_ORTHOGRAPHIC; p.ortho_height = height; set_projection(p); }
    void set_perspective() { check(pt_set_projection(ctx_, nullptr)); }
    pt_projection projection() const { pt_projection p{}; check(pt_get_projection(ctx_, &p)); return p; }
    // Camera::input: true where the reference's returns true
    bool input(pt_event event, float a, float b, float dt) { return check(pt_camera_input(ctx_, event, a, b, dt)) == 1; }
    Mat4 inv_projection() const { Mat4 m{}; check(pt_inv_projection(ctx_, m.data())); return m; }
    void set_environment(uint32_t w, uint32_t h, const float* rgb_linear) { check(pt_set_environment(ctx_, w, h, rgb_linear)); }

    // one MainEventsCleared iteration: the pixel loop for sample `frame_index`, then State::update  (main.rs:179-216)
    void frame(uint32_t frame_index, const Mat4& last_inv_projection, Frame* out = nullptr)
    {
        if (out)
        {
            out->data.resize((size_t)width_ * height_ * 4); out->position.resize((size_t)width_ * height_ * 4); out->id.resize((size_t)width_ * height_);
            check(pt_frame(ctx_, frame_index, last_inv_projection.data(), out->data.data(), out->position.data(), out->id.data()));
        }
        else check(pt_frame(ctx_, frame_index, last_inv_projection.data(), nullptr, nullptr, nullptr));
    }
    // frame() with a world that may have moved since the previous frame_moving (set_instances): the history is reprojected by the camera's
    // and the instances' motion; leaves this sample's guides valid (frame_moving(k), then denoise)
    void frame_moving(uint32_t frame_index, const Mat4& last_inv_projection, Frame* out = nullptr)
    {
        if (out)
        {
            out->data.resize((size_t)width_ * height_ * 4); out->position.resize((size_t)width_ * height_ * 4); out->id.resize((size_t)width_ * height_);
            check(pt_frame_moving(ctx_, frame_index, last_inv_projection.data(), out->data.data(), out->position.data(), out->id.data()));
        }
        else check(pt_frame_moving(ctx_, frame_index, last_inv_projection.data(), nullptr, nullptr, nullptr));
    }
    // frame_moving's render, guides and velocity, then the temporal stage of the denoiser instead of State::update (pt_frame_temporal): the
    // history is reprojected through geometry tests, blended by its length and filtered with the variance the pixels observed over time.  The
    // result stays on the device for write_denoised_image; filtered (W*H*4 floats) receives it too
    void frame_temporal(uint32_t frame_index, const Mat4& last_inv_projection, const pt_temporal_params& t = pt_temporal_params{},
                        const pt_denoise_params& d = pt_denoise_params{}, std::vector<float>* filtered = nullptr)
    {
        if (filtered) filtered->resize((size_t)width_ * height_ * 4);
        check(pt_frame_temporal(ctx_, frame_index, last_inv_projection.data(), &t, &d, nullptr, nullptr, nullptr, filtered ? filtered->data() : nullptr));
    }
    // the same under the stage's options (pt_frame_temporal_options): o.rescue, a 3 x 3 rescue search for pixels that lost every tap;
    // o.length_rule, PT_TEMPORAL_LENGTH_MEAN; o.demodulate, the stage on the sample divided by its albedo guide
    void frame_temporal(uint32_t frame_index, const Mat4& last_inv_projection, const pt_temporal_options& o, const pt_temporal_params& t = pt_temporal_params{},
                        const pt_denoise_params& d = pt_denoise_params{}, std::vector<float>* filtered = nullptr)
    {
        if (filtered) filtered->resize((size_t)width_ * height_ * 4);
        check(pt_frame_temporal_options(ctx_, frame_index, last_inv_projection.data(), &t, &o, &d, nullptr, nullptr, nullptr, filtered ? filtered->data() : nullptr));
    }
    void reset_temporal() { check(pt_reset_temporal(ctx_)); }
    // replaces the instance matrices of model `model` (index in Scene::models) and rebuilds: BLASes are kept, the TLASes are built again and,
    // when the instance count is unchanged, the next render patches the resident scene in place
    void set_instances(int model, const std::vector<Affine3A>& matrices)
    {
        check(pt_set_instances(ctx_, model, matrices.empty() ? nullptr : matrices[0].m.data(), (uint32_t)matrices.size()));
        check(pt_build(ctx_));
    }
    pt_scene_info scene_info() const { pt_scene_info s{}; check(pt_get_scene_info(ctx_, &s)); return s; }
    // the triangle soup of model `model` as loaded (9 floats per triangle): what UVs for an OBJ model are computed from
    std::vector<float> model_positions(int model) const
    {
        uint32_t n = 0;
        check(pt_model_vertices(ctx_, model, nullptr, nullptr, 0, &n));
        std::vector<float> p((size_t)n * 9), nr((size_t)n * 9);
        check(pt_model_vertices(ctx_, model, p.data(), nr.data(), n, &n));
        return p;
    }
    // replaces (empty: clears) the UVs of a model, 6 floats per triangle, and rebuilds: no BLAS and no TLAS is built again
    void set_model_uvs(int model, const std::vector<float>& uvs)
    {
        check(pt_set_model_uvs(ctx_, model, uvs.empty() ? nullptr : uvs.data(), (uint32_t)(uvs.size() / 6)));
        check(pt_build(ctx_));
    }
    // the fifth guide of render_guides: surface colour at the first hit, W*H*3
    std::vector<float> read_guide_albedo() const { std::vector<float> v((size_t)width_ * height_ * 3); check(pt_read_guide_albedo(ctx_, v.data())); return v; }
    // n_samples per pixel accumulated without the temporal pass (what the loop converges to for a camera at rest)
    void render(uint32_t first_sample, uint32_t n_samples) { check(pt_render_device(ctx_, first_sample, n_samples)); check(pt_synchronize(ctx_)); }
    void reset_accumulation() { check(pt_reset_accumulation(ctx_)); }
    Frame read_frame() const
    {
        Frame f;
        f.data.resize((size_t)width_ * height_ * 4); f.position.resize((size_t)width_ * height_ * 4); f.id.resize((size_t)width_ * height_);
        check(pt_read_frame(ctx_, f.data.data(), f.position.data(), f.id.data()));
        return f;
    }
    // checkpoint / resume: put a frame's state (as frame() / pt_render returned it) back, e.g. in another process
    void write_accumulation(const Frame& f)
    {
        // pt_write_accumulation copies width * height texels from each pointer: a frame saved at another size must not be read past its end
        const size_t px = (size_t)width_ * height_;
        if (f.data.size() != px * 4 || (!f.position.empty() && f.position.size() != px * 4) || (!f.id.empty() && f.id.size() != px))
            throw Error(PT_ERR_ARG, "write_accumulation: the frame was not saved at this renderer's " + std::to_string(width_) + "x" + std::to_string(height_));
        check(pt_write_accumulation(ctx_, f.data.data(), f.position.empty() ? nullptr : f.position.data(), f.id.empty() ? nullptr : f.id.data()));
    }
    // adaptive sampling (flags with PT_FLAG_ADAPTIVE): n_samples more samples for every pixel the criterion selects, each continuing from
    // its own count; returns how many pixels were selected.  Blocking; the frame stays on the device (read_frame).
    uint32_t render_adaptive(const pt_adaptive& crit, uint32_t n_samples)
    {
        uint32_t n = 0;
        check(pt_render_adaptive(ctx_, &crit, n_samples, &n));
        return n;
    }
    // the selection alone: 1 per pixel that render_adaptive would render
    std::vector<uint8_t> adaptive_mask(const pt_adaptive& crit) const
    {
        std::vector<uint8_t> m((size_t)width_ * height_);
        check(pt_adaptive_mask(ctx_, &crit, m.data(), nullptr));
        return m;
    }
    // Q per pixel (sum of squared sample luminance): saved and restored beside read_frame / write_accumulation for a checkpoint
    std::vector<float> read_moments() const { std::vector<float> q((size_t)width_ * height_); check(pt_read_moments(ctx_, q.data())); return q; }
    void write_moments(const std::vector<float>& q)
    {
        if (q.size() != (size_t)width_ * height_) throw Error(PT_ERR_ARG, "write_moments: not one value per pixel of this renderer's frame");
        check(pt_write_moments(ctx_, q.data()));
    }
    std::vector<float> present() const { std::vector<float> v((size_t)width_ * height_ * 4); check(pt_present(ctx_, v.data())); return v; }
    std::vector<uint8_t> present_rgb8() const { std::vector<uint8_t> v((size_t)width_ * height_ * 3); check(pt_present_rgb8(ctx_, v.data())); return v; }
    void write_image(const std::string& path) const { check(pt_write_image(ctx_, path.c_str())); }
    // denoising: first-hit guides of one sample, then the edge-aware a-trous filter of the accumulation (pt_denoise); the result stays on
    // the device for write_denoised_image
    void render_guides(uint32_t sample) { check(pt_render_guides(ctx_, sample)); }
    // the same with mirrors and glass followed, up to max_hops of them per pixel, to the first rough surface (pt_render_guides_followed):
    // the guides are that surface's, the model guide carries the hops in bits 31..28.  frame_moving writes first-hit guides: call this after it
    void render_guides_followed(uint32_t sample, uint32_t max_hops)
    {
        pt_guide_params p{};
        p.max_hops = max_hops;
        check(pt_render_guides_followed(ctx_, sample, &p));
    }
    // the hop guide: how many mirror / glass surfaces every pixel's chain followed, W*H bytes (zeros after render_guides)
    std::vector<uint8_t> read_guide_hops() const { std::vector<uint8_t> v((size_t)width_ * height_); check(pt_read_guide_hops(ctx_, v.data())); return v; }
    void denoise(const pt_denoise_params& p = pt_denoise_params{}) { check(pt_denoise(ctx_, &p, nullptr)); }
    void write_denoised_image(const std::string& path) const { check(pt_write_denoised_image(ctx_, path.c_str())); }
    // the demodulated filter (pt_denoise_albedo): the mean albedo of samples [first, first + n) of every pixel, then denoise() on the
    // accumulation divided by it (or by the albedo guide: PT_ALBEDO_GUIDE) and multiplied back; the result is written like denoise()'s
    void accumulate_albedo(uint32_t first_sample, uint32_t n_samples) { check(pt_accumulate_albedo(ctx_, first_sample, n_samples)); }
    // ... of the followed chains' albedo products: what denoise_albedo(PT_ALBEDO_MEAN) wants beside render_guides_followed(.., max_hops)
    void accumulate_albedo_followed(uint32_t first_sample, uint32_t n_samples, uint32_t max_hops)
    {
        pt_guide_params p{};
        p.max_hops = max_hops;
        check(pt_accumulate_albedo_followed(ctx_, first_sample, n_samples, &p));
    }
    void reset_albedo() { check(pt_reset_albedo(ctx_)); }
    std::vector<float> read_albedo() const { std::vector<float> v((size_t)width_ * height_ * 4); check(pt_read_albedo(ctx_, v.data())); return v; }
    void denoise_albedo(uint32_t albedo_source = PT_ALBEDO_MEAN, const pt_denoise_params& p = pt_denoise_params{})
    {
        check(pt_denoise_albedo(ctx_, &p, albedo_source, nullptr));
    }
    // caller-supplied rays (pt_integrate_rays): o, d 3 floats per ray (d is used as given), key and sample one word per ray naming each path's
    // stream.  Consecutive rays share a wave: order them coherently for speed; the results do not depend on the order.
    RayResults integrate_rays(const std::vector<float>& o, const std::vector<float>& d, const std::vector<uint32_t>& key, const std::vector<uint32_t>& sample,
                              uint32_t draws_consumed = 1, uint32_t batch_rays = 0)
    {
        const size_t n = key.size();
        if (o.size() != 3 * n || d.size() != 3 * n || sample.size() != n) throw Error(PT_ERR_ARG, "integrate_rays: o, d, key and sample do not describe the same number of rays");
        RayResults out;
        out.radiance.resize(n * 4); out.position.resize(n * 4); out.id.resize(n);
        pt_rays_params p{};
        p.draws_consumed = draws_consumed; p.batch_rays = batch_rays;
        check(pt_integrate_rays(ctx_, n, o.data(), d.data(), key.data(), sample.data(), &p, out.radiance.data(), out.position.data(), out.id.data()));
        return out;
    }
    // irradiance probes (pt_bake_probes): adds samples [first_sample, first_sample + n_samples) of every probe (3 floats each) to the raw
    // spherical-harmonics sums sh27 (27 floats per probe, [k][c]); an empty sh27 starts a fresh bake from zero
    void bake_probes(const std::vector<float>& positions, uint32_t n_samples, std::vector<float>& sh27, uint32_t first_sample = 0, uint32_t key_base = 0)
    {
        if (positions.size() % 3 != 0) throw Error(PT_ERR_ARG, "bake_probes: positions are 3 floats per probe");
        const size_t n = positions.size() / 3;
        if (sh27.empty()) sh27.assign(n * 27, 0.0f);
        if (sh27.size() != n * 27 || n > 0xffffffffull) throw Error(PT_ERR_ARG, "bake_probes: sh27 does not hold 27 values per probe");
        pt_probe_params p{};
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base;
        check(pt_bake_probes(ctx_, (uint32_t)n, positions.data(), &p, sh27.data()));
    }
    // direction and y0..y8 of a probe sample as bake_probes makes them (host evaluation)
    void probe_ray(uint32_t key, uint32_t sample, float d[3], float y9[9]) const { check(pt_probe_ray(ctx_, key, sample, d, y9)); }
    // a lightmap of one placement of a model over its UVs (pt_bake_lightmap): adds samples [first_sample, first_sample + n_samples) of every
    // covered texel to the raw sums rgb_sum (w * h * 3; empty: a fresh bake from zero) and returns the coverage bytes (1 covered, 0 not)
    std::vector<uint8_t> bake_lightmap(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, std::vector<float>& rgb_sum,
                                       uint32_t first_sample = 0, uint32_t key_base = 0, float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (rgb_sum.size() != px * 3) throw Error(PT_ERR_ARG, "bake_lightmap: rgb_sum does not hold 3 values per texel");
        std::vector<uint8_t> coverage(px);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        check(pt_bake_lightmap(ctx_, &p, rgb_sum.data(), coverage.data()));
        return coverage;
    }
    // bake_lightmap that also folds the second moment of every sample's luminance into sumsq (w * h; empty: from zero), for denoise_lightmap
    // (pt_bake_lightmap_moments)
    std::vector<uint8_t> bake_lightmap_moments(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, std::vector<float>& rgb_sum,
                                               std::vector<float>& sumsq, uint32_t first_sample = 0, uint32_t key_base = 0, float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (sumsq.empty()) sumsq.assign(px, 0.0f);
        if (rgb_sum.size() != px * 3 || sumsq.size() != px) throw Error(PT_ERR_ARG, "bake_lightmap_moments: rgb_sum holds 3 values per texel and sumsq one");
        std::vector<uint8_t> coverage(px);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        check(pt_bake_lightmap_moments(ctx_, &p, rgb_sum.data(), sumsq.data(), coverage.data()));
        return coverage;
    }
    // the texel-space filter (pt_lightmap_denoise) on a bake's raw sums over n_samples samples: the texel means (w * h * 3, zeros where
    // uncovered: dilate afterwards).  sumsq empty: the spatial variance; filter and reach 0: the defaults
    std::vector<float> denoise_lightmap(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, const std::vector<float>& rgb_sum,
                                        const std::vector<float>& sumsq = {}, pt_denoise_params filter = {}, float reach = 0.0f, bool on_device = true,
                                        std::vector<float>* texel_area = nullptr) const
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.size() != px * 3 || (!sumsq.empty() && sumsq.size() != px)) throw Error(PT_ERR_ARG, "denoise_lightmap: rgb_sum holds 3 values per texel and sumsq one");
        pt_lightmap_denoise_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.n_samples = n_samples; p.filter = filter; p.reach = reach;
        std::vector<float> mean(px * 3);
        if (texel_area) texel_area->assign(px, 0.0f);
        check(pt_lightmap_denoise(ctx_, on_device ? 1 : 0, &p, rgb_sum.data(), sumsq.empty() ? nullptr : sumsq.data(), mean.data(), texel_area ? texel_area->data() : nullptr));
        return mean;
    }
    // one round of an adaptive bake (pt_bake_lightmap_adaptive): the texels of the map that crit selects from (rgb_sum, sumsq, counts) get
    // n_samples more samples each, continuing from their own counts.  The three are IN/OUT (empty: a fresh bake from zeros); returns the
    // number of texels selected, and the coverage bytes if asked.  Call until it returns 0.
    uint32_t bake_lightmap_adaptive(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, const pt_adaptive& crit, std::vector<float>& rgb_sum,
                                    std::vector<float>& sumsq, std::vector<uint32_t>& counts, std::vector<uint8_t>* coverage = nullptr, uint32_t key_base = 0,
                                    float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (sumsq.empty()) sumsq.assign(px, 0.0f);
        if (counts.empty()) counts.assign(px, 0u);
        if (rgb_sum.size() != px * 3 || sumsq.size() != px || counts.size() != px)
            throw Error(PT_ERR_ARG, "bake_lightmap_adaptive: rgb_sum holds 3 values per texel, sumsq and counts one");
        if (coverage) coverage->assign(px, 0);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        uint32_t n = 0;
        check(pt_bake_lightmap_adaptive(ctx_, &p, &crit, rgb_sum.data(), sumsq.data(), counts.data(), coverage ? coverage->data() : nullptr, &n));
        return n;
    }
    // bake_lightmap with direct light sampled at the texel (pt_bake_lightmap_direct): a sample is the gather radiance, zero when the gather
    // ray's first hit is a lamp, plus one light sample with a shadow ray.  sumsq null: no moments; otherwise as bake_lightmap_moments'.  The
    // light samples draw from the streams of pixels light_key_base + texel: keep them apart from [key_base, key_base + w * h)
    std::vector<uint8_t> bake_lightmap_direct(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, std::vector<float>& rgb_sum,
                                              std::vector<float>* sumsq, uint32_t light_key_base, uint32_t first_sample = 0, uint32_t key_base = 0, float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (sumsq && sumsq->empty()) sumsq->assign(px, 0.0f);
        if (rgb_sum.size() != px * 3 || (sumsq && sumsq->size() != px)) throw Error(PT_ERR_ARG, "bake_lightmap_direct: rgb_sum holds 3 values per texel and sumsq one");
        std::vector<uint8_t> coverage(px);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        pt_lightmap_direct dp{};
        dp.light_key_base = light_key_base;
        check(pt_bake_lightmap_direct(ctx_, &p, &dp, rgb_sum.data(), sumsq ? sumsq->data() : nullptr, coverage.data()));
        return coverage;
    }
    // one round of bake_lightmap_adaptive over bake_lightmap_direct's samples (pt_bake_lightmap_adaptive_direct)
    uint32_t bake_lightmap_adaptive_direct(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, const pt_adaptive& crit, std::vector<float>& rgb_sum,
                                           std::vector<float>& sumsq, std::vector<uint32_t>& counts, uint32_t light_key_base, std::vector<uint8_t>* coverage = nullptr,
                                           uint32_t key_base = 0, float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (sumsq.empty()) sumsq.assign(px, 0.0f);
        if (counts.empty()) counts.assign(px, 0u);
        if (rgb_sum.size() != px * 3 || sumsq.size() != px || counts.size() != px)
            throw Error(PT_ERR_ARG, "bake_lightmap_adaptive_direct: rgb_sum holds 3 values per texel, sumsq and counts one");
        if (coverage) coverage->assign(px, 0);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        pt_lightmap_direct dp{};
        dp.light_key_base = light_key_base;
        uint32_t n = 0;
        check(pt_bake_lightmap_adaptive_direct(ctx_, &p, &dp, &crit, rgb_sum.data(), sumsq.data(), counts.data(), coverage ? coverage->data() : nullptr, &n));
        return n;
    }
    // the selection alone (pt_lightmap_adaptive_mask): 1 per texel that bake_lightmap_adaptive would give samples
    std::vector<uint8_t> lightmap_adaptive_mask(int model, uint32_t instance, uint32_t w, uint32_t h, const pt_adaptive& crit, const std::vector<float>& rgb_sum,
                                                const std::vector<float>& sumsq, const std::vector<uint32_t>& counts, bool on_device = false) const
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.size() != px * 3 || sumsq.size() != px || counts.size() != px)
            throw Error(PT_ERR_ARG, "lightmap_adaptive_mask: rgb_sum holds 3 values per texel, sumsq and counts one");
        std::vector<uint8_t> mask(px);
        uint32_t n = 0;
        check(pt_lightmap_adaptive_mask(ctx_, on_device ? 1 : 0, model, instance, w, h, &crit, rgb_sum.data(), sumsq.data(), counts.data(), mask.data(), &n));
        return mask;
    }
    // denoise_lightmap with a sample count per texel (pt_lightmap_denoise_counts): an adaptive bake's sums, moments and counts
    std::vector<float> denoise_lightmap_counts(int model, uint32_t instance, uint32_t w, uint32_t h, const std::vector<float>& rgb_sum, const std::vector<float>& sumsq,
                                               const std::vector<uint32_t>& counts, pt_denoise_params filter = {}, float reach = 0.0f, bool on_device = true) const
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.size() != px * 3 || (!sumsq.empty() && sumsq.size() != px) || counts.size() != px)
            throw Error(PT_ERR_ARG, "denoise_lightmap_counts: rgb_sum holds 3 values per texel, sumsq and counts one");
        pt_lightmap_denoise_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.filter = filter; p.reach = reach;
        std::vector<float> mean(px * 3);
        check(pt_lightmap_denoise_counts(ctx_, on_device ? 1 : 0, &p, rgb_sum.data(), sumsq.empty() ? nullptr : sumsq.data(), counts.data(), mean.data(), nullptr));
        return mean;
    }
    // the texel means of an adaptive bake: every texel's sums over ITS OWN count, zero where the count is 0.  Divide first, dilate the means
    // afterwards: a dilated raw sum would mix neighbours with different denominators
    static std::vector<float> lightmap_means(const std::vector<float>& rgb_sum, const std::vector<uint32_t>& counts)
    {
        if (rgb_sum.size() != counts.size() * 3) throw Error(PT_ERR_ARG, "lightmap_means: rgb_sum holds 3 values per texel and counts one");
        std::vector<float> mean(rgb_sum.size(), 0.0f);
        for (size_t k = 0; k < counts.size(); ++k)
            for (size_t ch = 0; counts[k] && ch < 3; ++ch) mean[3 * k + ch] = rgb_sum[3 * k + ch] / (float)counts[k];
        return mean;
    }
    // `passes` dilation passes over a w x h map and its coverage bytes (pt_lightmap_dilate); filled texels carry the byte 2
    void dilate_lightmap(uint32_t w, uint32_t h, uint32_t passes, std::vector<float>& rgb, std::vector<uint8_t>& coverage)
    {
        const size_t px = (size_t)w * h;
        if (rgb.size() != px * 3 || coverage.size() != px) throw Error(PT_ERR_ARG, "dilate_lightmap: rgb holds 3 values and coverage one byte per texel");
        check(pt_lightmap_dilate(ctx_, w, h, passes, rgb.data(), coverage.data()));
    }
    // the finished map of one placement (pt_set_lightmap): rgb holds w * h * 3 texel means (sum / n_samples after dilation); empty with
    // w == h == 0 clears it.  lightmap_info: {w, h}, 0 x 0 where there is none
    void set_lightmap(int model, uint32_t instance, uint32_t w, uint32_t h, const std::vector<float>& rgb)
    {
        if (rgb.size() != (size_t)w * h * 3) throw Error(PT_ERR_ARG, "set_lightmap: rgb does not hold 3 values per texel");
        check(pt_set_lightmap(ctx_, model, instance, w, h, rgb.empty() ? nullptr : rgb.data()));
    }
    std::array<uint32_t, 2> lightmap_info(int model, uint32_t instance) const
    {
        std::array<uint32_t, 2> wh{};
        check(pt_get_lightmap_info(ctx_, model, instance, &wh[0], &wh[1]));
        return wh;
    }
    // the lightmap at n hits {world-TLAS leaf, load-order primitive, u, v} (pt_lightmap_lookup): rgb (n * 3) and the mapped bytes
    std::vector<float> lightmap_lookup(const std::vector<uint32_t>& instance, const std::vector<uint32_t>& prim, const std::vector<float>& u,
                                       const std::vector<float>& v, std::vector<uint8_t>& mapped, bool on_device = false) const
    {
        const size_t n = instance.size();
        if (prim.size() != n || u.size() != n || v.size() != n) throw Error(PT_ERR_ARG, "lightmap_lookup: the four arrays differ in length");
        std::vector<float> rgb(n * 3);
        mapped.assign(n, 0);
        check(pt_lightmap_lookup(ctx_, on_device ? 1 : 0, (uint32_t)n, instance.data(), prim.data(), u.data(), v.data(), rgb.data(), mapped.data()));
        return rgb;
    }
    // directional lightmaps: bake_lightmap that also folds every sample's radiance times its direction into dir_sum (w * h * 9 as
    // [texel][axis][channel]; empty: from zero) (pt_bake_lightmap_directional) ...
    std::vector<uint8_t> bake_lightmap_directional(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, std::vector<float>& rgb_sum,
                                                   std::vector<float>& dir_sum, uint32_t first_sample = 0, uint32_t key_base = 0, float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (dir_sum.empty()) dir_sum.assign(px * 9, 0.0f);
        if (rgb_sum.size() != px * 3 || dir_sum.size() != px * 9) throw Error(PT_ERR_ARG, "bake_lightmap_directional: rgb_sum holds 3 values per texel and dir_sum 9");
        std::vector<uint8_t> coverage(px);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        check(pt_bake_lightmap_directional(ctx_, &p, rgb_sum.data(), dir_sum.data(), coverage.data()));
        return coverage;
    }
    // ... the tangential gradient of those sums over n_samples samples (pt_lightmap_gradient; w * h * 9, zeros where uncovered) ...
    std::vector<float> lightmap_gradient(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, const std::vector<float>& dir_sum,
                                         bool on_device = false) const
    {
        if (dir_sum.size() != (size_t)w * h * 9) throw Error(PT_ERR_ARG, "lightmap_gradient: dir_sum does not hold 9 values per texel");
        std::vector<float> grad(dir_sum.size());
        check(pt_lightmap_gradient(ctx_, on_device ? 1 : 0, model, instance, w, h, n_samples, dir_sum.data(), grad.data()));
        return grad;
    }
    // ... its dilation: dilate_lightmap on each of the three axis planes, each with a fresh copy of the coverage, which comes back dilated ...
    void dilate_lightmap_directional(uint32_t w, uint32_t h, uint32_t passes, std::vector<float>& grad, std::vector<uint8_t>& coverage)
    {
        const size_t px = (size_t)w * h;
        if (grad.size() != px * 9 || coverage.size() != px) throw Error(PT_ERR_ARG, "dilate_lightmap_directional: grad holds 9 values and coverage one byte per texel");
        std::vector<uint8_t> out = coverage;
        for (size_t a = 0; a < 3; ++a)
        {
            std::vector<float> plane(px * 3);
            for (size_t k = 0; k < px; ++k)
                for (size_t c = 0; c < 3; ++c) plane[3 * k + c] = grad[(3 * k + a) * 3 + c];
            out = coverage;
            dilate_lightmap(w, h, passes, plane, out);
            for (size_t k = 0; k < px; ++k)
                for (size_t c = 0; c < 3; ++c) grad[(3 * k + a) * 3 + c] = plane[3 * k + c];
        }
        coverage = out;
    }
    // ... and the gradient of one placement beside its map (pt_set_lightmap_directional): w * h * 9 values of the map's size; empty with
    // w == h == 0 clears it.  lightmap_directional_info: whether the placement has one
    void set_lightmap_directional(int model, uint32_t instance, uint32_t w, uint32_t h, const std::vector<float>& grad)
    {
        if (grad.size() != (size_t)w * h * 9) throw Error(PT_ERR_ARG, "set_lightmap_directional: grad does not hold 9 values per texel");
        check(pt_set_lightmap_directional(ctx_, model, instance, w, h, grad.empty() ? nullptr : grad.data()));
    }
    bool lightmap_directional_info(int model, uint32_t instance) const
    {
        uint32_t has = 0;
        check(pt_get_lightmap_directional_info(ctx_, model, instance, &has));
        return has != 0;
    }
    // the lightmap under the perturbed normal at n hits made by rays of world direction dir (n * 3) (pt_lightmap_lookup_directional)
    std::vector<float> lightmap_lookup_directional(const std::vector<uint32_t>& instance, const std::vector<uint32_t>& prim, const std::vector<float>& u,
                                                   const std::vector<float>& v, const std::vector<float>& dir, std::vector<uint8_t>& mapped,
                                                   bool on_device = false) const
    {
        const size_t n = instance.size();
        if (prim.size() != n || u.size() != n || v.size() != n || dir.size() != n * 3) throw Error(PT_ERR_ARG, "lightmap_lookup_directional: the arrays differ in length");
        std::vector<float> rgb(n * 3);
        mapped.assign(n, 0);
        check(pt_lightmap_lookup_directional(ctx_, on_device ? 1 : 0, (uint32_t)n, instance.data(), prim.data(), u.data(), v.data(), dir.data(), rgb.data(),
                                             mapped.data()));
        return rgb;
    }
    // the baked view (pt_render_baked): adds samples [first_sample, first_sample + n_samples) of every pixel's followed first hit, shaded
    // from the lightmaps, to the baked sums and returns them (sum r, sum g, sum b, n per pixel)
    std::vector<float> render_baked(uint32_t first_sample, uint32_t n_samples, uint32_t max_hops = 0, std::array<float, 3> unlit = {0.0f, 0.0f, 0.0f})
    {
        pt_baked_params p{};
        p.max_hops = max_hops;
        p.unlit[0] = unlit[0]; p.unlit[1] = unlit[1]; p.unlit[2] = unlit[2];
        std::vector<float> v((size_t)width_ * height_ * 4);
        check(pt_render_baked(ctx_, first_sample, n_samples, &p, v.data()));
        return v;
    }
    std::vector<float> read_baked() const { std::vector<float> v((size_t)width_ * height_ * 4); check(pt_read_baked(ctx_, v.data())); return v; }
    void reset_baked() { check(pt_reset_baked(ctx_)); }
    void write_baked_image(const std::string& path) const { check(pt_write_baked_image(ctx_, path.c_str())); }
    // the baked view's chain for caller-supplied rays (pt_baked_rays): o, d 3 floats per ray (d is used as given); rgbh gets (B.r, B.g, B.b,
    // the hop the chain ended at) per ray and id the first hit's id byte (255 = miss).  window_rays 0: the library's window
    BakedRays baked_rays(const std::vector<float>& o, const std::vector<float>& d, uint32_t max_hops = 0, std::array<float, 3> unlit = {0.0f, 0.0f, 0.0f},
                         uint32_t window_rays = 0)
    {
        if (o.size() != d.size() || o.size() % 3 != 0) throw Error(PT_ERR_ARG, "baked_rays: o and d are 3 floats per ray for the same rays");
        const size_t n = o.size() / 3;
        BakedRays out;
        out.rgbh.resize(n * 4); out.id.resize(n);
        pt_baked_rays_params p{};
        p.baked = baked_params(max_hops, unlit);
        p.window_rays = window_rays;
        check(pt_baked_rays(ctx_, n, o.data(), d.data(), &p, out.rgbh.data(), out.id.data()));
        return out;
    }
    // the final-gather bake (pt_bake_lightmap_gather): bake_lightmap whose gather ray is one baked chain (max_hops, unlit as render_baked)
    // ended in the maps, grid and probes set on this renderer; with direct the texel's light sample is added and a gather ray whose first hit
    // is a lamp counts zero, as bake_lightmap_direct (light_key_base likewise; 0 without direct).  sumsq null: no moments.  Sets nothing.
    std::vector<uint8_t> bake_lightmap_gather(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, std::vector<float>& rgb_sum,
                                              std::vector<float>* sumsq, bool direct, uint32_t light_key_base, uint32_t max_hops = 0,
                                              std::array<float, 3> unlit = {0.0f, 0.0f, 0.0f}, uint32_t first_sample = 0, uint32_t key_base = 0, float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (sumsq && sumsq->empty()) sumsq->assign(px, 0.0f);
        if (rgb_sum.size() != px * 3 || (sumsq && sumsq->size() != px)) throw Error(PT_ERR_ARG, "bake_lightmap_gather: rgb_sum holds 3 values per texel and sumsq one");
        std::vector<uint8_t> coverage(px);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        pt_lightmap_gather g{};
        g.baked = baked_params(max_hops, unlit);
        g.direct = direct ? 1u : 0u; g.light_key_base = light_key_base;
        check(pt_bake_lightmap_gather(ctx_, &p, &g, rgb_sum.data(), sumsq ? sumsq->data() : nullptr, coverage.data()));
        return coverage;
    }
    // one round of bake_lightmap_adaptive over bake_lightmap_gather's samples (pt_bake_lightmap_adaptive_gather)
    uint32_t bake_lightmap_adaptive_gather(int model, uint32_t instance, uint32_t w, uint32_t h, uint32_t n_samples, const pt_adaptive& crit, std::vector<float>& rgb_sum,
                                           std::vector<float>& sumsq, std::vector<uint32_t>& counts, bool direct, uint32_t light_key_base, uint32_t max_hops = 0,
                                           std::array<float, 3> unlit = {0.0f, 0.0f, 0.0f}, std::vector<uint8_t>* coverage = nullptr, uint32_t key_base = 0,
                                           float bias = 0.0f)
    {
        const size_t px = (size_t)w * h;
        if (rgb_sum.empty()) rgb_sum.assign(px * 3, 0.0f);
        if (sumsq.empty()) sumsq.assign(px, 0.0f);
        if (counts.empty()) counts.assign(px, 0u);
        if (rgb_sum.size() != px * 3 || sumsq.size() != px || counts.size() != px)
            throw Error(PT_ERR_ARG, "bake_lightmap_adaptive_gather: rgb_sum holds 3 values per texel, sumsq and counts one");
        if (coverage) coverage->assign(px, 0);
        pt_lightmap_params p{};
        p.model = model; p.instance = instance; p.w = w; p.h = h;
        p.n_samples = n_samples; p.key_base = key_base; p.bias = bias;
        pt_lightmap_gather g{};
        g.baked = baked_params(max_hops, unlit);
        g.direct = direct ? 1u : 0u; g.light_key_base = light_key_base;
        uint32_t n = 0;
        check(pt_bake_lightmap_adaptive_gather(ctx_, &p, &g, &crit, rgb_sum.data(), sumsq.data(), counts.data(), coverage ? coverage->data() : nullptr, &n));
        return n;
    }
    // the irradiance volume (pt_set_probe_grid): g places the nodes, sh27 holds 27 RADIANCE coefficients per node (node (ix, iy, iz) at
    // (iz * ny + iy) * nx + ix), valid a byte per node (empty: all valid).  An empty sh27 with counts of 0 clears the grid.
    void set_probe_grid(const pt_probe_grid& g, const std::vector<float>& sh27, const std::vector<uint8_t>& valid = {})
    {
        const size_t n = (size_t)g.count[0] * g.count[1] * g.count[2];
        if (sh27.size() != n * 27 || (!valid.empty() && valid.size() != n)) throw Error(PT_ERR_ARG, "set_probe_grid: sh27 holds 27 values per node and valid one byte");
        check(pt_set_probe_grid(ctx_, &g, sh27.empty() ? nullptr : sh27.data(), valid.empty() ? nullptr : valid.data()));
    }
    // ... of bake_probes' raw sums over n_samples samples: the factor 4 pi / n_samples is applied here
    void set_probe_grid_sums(const pt_probe_grid& g, const std::vector<float>& sums, uint32_t n_samples, const std::vector<uint8_t>& valid = {})
    {
        if (n_samples == 0) throw Error(PT_ERR_ARG, "set_probe_grid_sums: n_samples must be positive");
        const float scale = 12.566371f / (float)n_samples;
        std::vector<float> sh(sums);
        for (float& v : sh) v *= scale;
        set_probe_grid(g, sh, valid);
    }
    // the grid in force (counts of 0: none); n_valid: its valid nodes
    pt_probe_grid probe_grid_info(uint32_t* n_valid = nullptr) const { pt_probe_grid g{}; check(pt_get_probe_grid_info(ctx_, &g, n_valid)); return g; }
    // the grid's lookup at n world positions and normals (3 floats each; pt_probe_grid_lookup): rgb (n * 3) and the lit bytes
    std::vector<float> probe_grid_lookup(const std::vector<float>& position, const std::vector<float>& normal, std::vector<uint8_t>& lit, bool on_device = false) const
    {
        if (position.size() % 3 != 0 || normal.size() != position.size()) throw Error(PT_ERR_ARG, "probe_grid_lookup: positions and normals are 3 floats per query");
        const size_t n = position.size() / 3;
        std::vector<float> rgb(n * 3);
        lit.assign(n, 0);
        check(pt_probe_grid_lookup(ctx_, on_device ? 1 : 0, (uint32_t)n, position.data(), normal.data(), rgb.data(), lit.data()));
        return rgb;
    }
    // the census of probes inside geometry (pt_probe_backfaces): per probe, bake_probes' rays that hit anything and those that hit a back face
    void probe_backfaces(const std::vector<float>& positions, uint32_t n_samples, std::vector<uint32_t>& hits, std::vector<uint32_t>& back,
                         uint32_t first_sample = 0, uint32_t key_base = 0)
    {
        if (positions.size() % 3 != 0 || positions.size() / 3 > 0xffffffffull) throw Error(PT_ERR_ARG, "probe_backfaces: positions are 3 floats per probe");
        const size_t n = positions.size() / 3;
        hits.assign(n, 0u); back.assign(n, 0u);
        pt_probe_params p{};
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base;
        check(pt_probe_backfaces(ctx_, (uint32_t)n, positions.data(), &p, hits.data(), back.data()));
    }
    // the usual policy over probe_backfaces: a probe is usable while at most max_back_fraction of its rays see a back face
    std::vector<uint8_t> probe_validity(const std::vector<float>& positions, uint32_t n_samples, float max_back_fraction = 0.25f)
    {
        std::vector<uint32_t> hits, back;
        probe_backfaces(positions, n_samples, hits, back);
        std::vector<uint8_t> valid(back.size());
        for (size_t i = 0; i < back.size(); ++i) valid[i] = (float)back[i] <= max_back_fraction * (float)n_samples ? 1 : 0;
        return valid;
    }
    // bakes and sets a grid: the node positions, bake_probes, probe_validity and set_probe_grid_sums; returns the valid bytes
    // depth_res > 0 also bakes the nodes' depth moments from the same rays and sets them (bake_probe_depth, set_probe_grid_depth_sums);
    // max_distance <= 0: the cell's diagonal times 1.5.  radiance_res > 0 also bakes the nodes' radiance maps from the same rays, prefilters
    // them at radiance_alphas on the device and sets them (bake_probe_radiance, set_probe_grid_radiance_sums)
    std::vector<uint8_t> bake_probe_grid(const pt_probe_grid& g, uint32_t n_samples, float max_back_fraction = 0.25f, uint32_t depth_res = 0,
                                         float max_distance = 0.0f, float vis_floor = 0.0f, bool facing = false, uint32_t radiance_res = 0,
                                         const std::vector<float>& radiance_alphas = {0.1f, 0.2f, 0.4f, 0.7f, 1.0f})
    {
        std::vector<float> pos;
        for (uint32_t z = 0; z < g.count[2]; ++z)
            for (uint32_t y = 0; y < g.count[1]; ++y)
                for (uint32_t x = 0; x < g.count[0]; ++x)
                    for (float v : {g.origin[0] + (float)x * g.cell[0], g.origin[1] + (float)y * g.cell[1], g.origin[2] + (float)z * g.cell[2]}) pos.push_back(v);
        std::vector<float> sums;
        bake_probes(pos, n_samples, sums);
        const std::vector<uint8_t> valid = probe_validity(pos, n_samples, max_back_fraction);
        set_probe_grid_sums(g, sums, n_samples, valid);
        if (depth_res)
        {
            if (!(max_distance > 0.0f))
                max_distance = (float)(1.5 * std::sqrt((double)g.cell[0] * g.cell[0] + (double)g.cell[1] * g.cell[1] + (double)g.cell[2] * g.cell[2]));
            std::vector<float> dsums;
            std::vector<uint32_t> dcounts;
            bake_probe_depth(pos, n_samples, depth_res, max_distance, dsums, dcounts);
            set_probe_grid_depth_sums(depth_res, dsums, dcounts, max_distance, vis_floor, facing);
        }
        if (radiance_res)
        {
            std::vector<float> rsums;
            std::vector<uint32_t> rcounts;
            bake_probe_radiance(pos, n_samples, radiance_res, rsums, rcounts);
            set_probe_grid_radiance_sums(radiance_res, rsums, rcounts, radiance_alphas);
        }
        return valid;
    }
    // probe visibility.  The texel of every direction (3 floats each, any values) in an octahedral map of side res (pt_probe_depth_texel)
    static std::vector<uint32_t> probe_depth_texel(const std::vector<float>& directions, uint32_t res)
    {
        if (directions.size() % 3 != 0 || directions.size() / 3 > 0xffffffffull) throw Error(PT_ERR_ARG, "probe_depth_texel: directions are 3 floats each");
        std::vector<uint32_t> texel(directions.size() / 3);
        const int r = pt_probe_depth_texel(res, (uint32_t)texel.size(), directions.data(), texel.data());
        if (r != PT_OK) throw Error(r, "probe_depth_texel: res is 2..16");
        return texel;
    }
    // depth moments (pt_bake_probe_depth): adds the clamped distances bake_probes' rays see to the raw sums (res * res * 2 floats per probe)
    // and counts (res * res per probe) per octahedral texel, in sample order; empty vectors start a fresh bake from zero
    void bake_probe_depth(const std::vector<float>& positions, uint32_t n_samples, uint32_t res, float max_distance, std::vector<float>& sums,
                          std::vector<uint32_t>& counts, uint32_t first_sample = 0, uint32_t key_base = 0)
    {
        if (positions.size() % 3 != 0 || positions.size() / 3 > 0xffffffffull) throw Error(PT_ERR_ARG, "bake_probe_depth: positions are 3 floats per probe");
        const size_t n = positions.size() / 3, texels = n * res * res;
        if (sums.empty() && counts.empty()) { sums.assign(texels * 2, 0.0f); counts.assign(texels, 0u); }
        if (res >= 2 && res <= 16 && (sums.size() != texels * 2 || counts.size() != texels))
            throw Error(PT_ERR_ARG, "bake_probe_depth: sums hold res * res * 2 values and counts res * res per probe");
        pt_probe_depth_params p{};
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.res = res; p.max_distance = max_distance;
        check(pt_bake_probe_depth(ctx_, (uint32_t)n, positions.data(), &p, sums.data(), counts.data()));
    }
    // depth on the grid in force (pt_set_probe_grid_depth): per node and texel the mean distance and the mean squared distance; empty
    // moments with res 0 clear it
    void set_probe_grid_depth(uint32_t res, const std::vector<float>& moments, float vis_floor = 0.0f, bool facing = false)
    {
        pt_probe_depth v{};
        v.res = res; v.flags = facing ? PT_PROBE_VIS_FACING : 0u; v.vis_floor = vis_floor;
        uint32_t n_valid = 0;
        const pt_probe_grid g = probe_grid_info(&n_valid);
        const size_t nodes = (size_t)g.count[0] * g.count[1] * g.count[2];
        if (res >= 2 && res <= 16 && moments.size() != nodes * res * res * 2) throw Error(PT_ERR_ARG, "set_probe_grid_depth: moments hold res * res * 2 values per node");
        check(pt_set_probe_grid_depth(ctx_, &v, moments.empty() ? nullptr : moments.data()));
    }
    // ... of bake_probe_depth's raw sums and counts: the means are taken here, and a texel without a sample gets (max_distance, its square)
    void set_probe_grid_depth_sums(uint32_t res, const std::vector<float>& sums, const std::vector<uint32_t>& counts, float max_distance, float vis_floor = 0.0f,
                                   bool facing = false)
    {
        if (sums.size() != counts.size() * 2) throw Error(PT_ERR_ARG, "set_probe_grid_depth_sums: two sums per count");
        std::vector<float> m(sums.size());
        for (size_t i = 0; i < counts.size(); ++i)
        {
            m[2 * i] = counts[i] ? sums[2 * i] / (float)counts[i] : max_distance;
            m[2 * i + 1] = counts[i] ? sums[2 * i + 1] / (float)counts[i] : max_distance * max_distance;
        }
        set_probe_grid_depth(res, m, vis_floor, facing);
    }
    pt_probe_depth probe_grid_depth_info() const { pt_probe_depth v{}; check(pt_get_probe_grid_depth_info(ctx_, &v)); return v; }
    // reflection probes.  The unit direction (3 floats each) and relative solid angle of every texel centre of an octahedral map of side res,
    // in the texels' order (pt_probe_radiance_dir)
    static std::vector<float> probe_radiance_dir(uint32_t res, std::vector<float>& omega)
    {
        if (res < 2 || res > 16) throw Error(PT_ERR_LIMIT, "probe_radiance_dir: res is 2..16");
        std::vector<uint32_t> texel(res * res);
        for (uint32_t i = 0; i < res * res; ++i) texel[i] = i;
        std::vector<float> dir(texel.size() * 3);
        omega.assign(texel.size(), 0.0f);
        const int r = pt_probe_radiance_dir(res, (uint32_t)texel.size(), texel.data(), dir.data(), omega.data());
        if (r != PT_OK) throw Error(r, "probe_radiance_dir");
        return dir;
    }
    // radiance maps (pt_bake_probe_radiance): adds the radiance of bake_probes' rays, the full path each, to the raw sums (res * res * 3 floats
    // per probe) and counts (res * res per probe) per octahedral texel, in sample order; empty vectors start a fresh bake from zero
    void bake_probe_radiance(const std::vector<float>& positions, uint32_t n_samples, uint32_t res, std::vector<float>& sums, std::vector<uint32_t>& counts,
                             uint32_t first_sample = 0, uint32_t key_base = 0)
    {
        if (positions.size() % 3 != 0 || positions.size() / 3 > 0xffffffffull) throw Error(PT_ERR_ARG, "bake_probe_radiance: positions are 3 floats per probe");
        const size_t n = positions.size() / 3, texels = n * res * res;
        if (sums.empty() && counts.empty()) { sums.assign(texels * 3, 0.0f); counts.assign(texels, 0u); }
        if (res >= 2 && res <= 16 && (sums.size() != texels * 3 || counts.size() != texels))
            throw Error(PT_ERR_ARG, "bake_probe_radiance: sums hold res * res * 3 values and counts res * res per probe");
        pt_probe_radiance_params p{};
        p.first_sample = first_sample; p.n_samples = n_samples; p.key_base = key_base; p.res = res;
        check(pt_bake_probe_radiance(ctx_, (uint32_t)n, positions.data(), &p, sums.data(), counts.data()));
    }
    // the GGX prefilter of raw radiance maps (pt_probe_radiance_prefilter): the table [probe][level][texel] of 4 floats each, one level per alpha
    std::vector<float> probe_radiance_prefilter(uint32_t res, const std::vector<float>& sums, const std::vector<uint32_t>& counts, const std::vector<float>& alphas,
                                                bool on_device = true)
    {
        if (res < 2 || res > 16 || alphas.empty() || alphas.size() > 8 || counts.size() % (res * res) != 0 || sums.size() != counts.size() * 3)
            throw Error(PT_ERR_ARG, "probe_radiance_prefilter: res 2..16, 1..8 alphas, res * res counts and three sums per count per probe");
        pt_probe_radiance_filter f{};
        f.res = res; f.n_probes = (uint32_t)(counts.size() / (res * res)); f.n_levels = (uint32_t)alphas.size();
        for (size_t l = 0; l < alphas.size(); ++l) f.alpha[l] = alphas[l];
        std::vector<float> table(counts.size() * alphas.size() * 4);
        check(pt_probe_radiance_prefilter(ctx_, on_device ? 1 : 0, &f, sums.data(), counts.data(), table.data()));
        return table;
    }
    // radiance on the grid in force (pt_set_probe_grid_radiance): probe_radiance_prefilter's table over the grid's nodes; an empty table clears it
    void set_probe_grid_radiance(uint32_t res, const std::vector<float>& table, const std::vector<float>& alphas)
    {
        if (table.empty()) { check(pt_set_probe_grid_radiance(ctx_, nullptr, nullptr)); return; }
        if (alphas.empty() || alphas.size() > 8) throw Error(PT_ERR_ARG, "set_probe_grid_radiance: 1..8 alphas");
        pt_probe_radiance v{};
        v.res = res; v.n_levels = (uint32_t)alphas.size();
        for (size_t l = 0; l < alphas.size(); ++l) v.alpha[l] = alphas[l];
        const pt_probe_grid g = probe_grid_info();
        const size_t nodes = (size_t)g.count[0] * g.count[1] * g.count[2];
        if (res >= 2 && res <= 16 && table.size() != nodes * alphas.size() * res * res * 4)
            throw Error(PT_ERR_ARG, "set_probe_grid_radiance: the table holds levels * res * res * 4 values per node");
        check(pt_set_probe_grid_radiance(ctx_, &v, table.data()));
    }
    // ... of bake_probe_radiance's raw sums and counts: the prefilter, then the setter
    void set_probe_grid_radiance_sums(uint32_t res, const std::vector<float>& sums, const std::vector<uint32_t>& counts, const std::vector<float>& alphas,
                                      bool on_device = true)
    {
        set_probe_grid_radiance(res, probe_radiance_prefilter(res, sums, counts, alphas, on_device), alphas);
    }
    pt_probe_radiance probe_grid_radiance_info() const { pt_probe_radiance v{}; check(pt_get_probe_grid_radiance_info(ctx_, &v)); return v; }
    // the reflection probes' lookup at n world positions, normals and incoming directions (3 floats each) and GGX alphas (one each;
    // pt_probe_grid_specular): rgb (n * 3) and the lit bytes
    std::vector<float> probe_grid_specular(const std::vector<float>& position, const std::vector<float>& normal, const std::vector<float>& incoming,
                                           const std::vector<float>& alpha, std::vector<uint8_t>& lit, bool on_device = false) const
    {
        if (position.size() % 3 != 0 || normal.size() != position.size() || incoming.size() != position.size() || alpha.size() * 3 != position.size())
            throw Error(PT_ERR_ARG, "probe_grid_specular: positions, normals and incoming directions are 3 floats and alpha one per query");
        const size_t n = alpha.size();
        std::vector<float> rgb(n * 3);
        lit.assign(n, 0);
        check(pt_probe_grid_specular(ctx_, on_device ? 1 : 0, (uint32_t)n, position.data(), normal.data(), incoming.data(), alpha.data(), rgb.data(), lit.data()));
        return rgb;
    }
    // the world TLAS's root box: min xyz, max xyz
    std::array<float, 6> root_box() const { uint32_t rect[4]; std::array<float, 6> b{}; check(pt_active_pixels(ctx_, rect, b.data())); return b; }
    pt_stats stats() const { pt_stats s{}; check(pt_get_stats(ctx_, &s)); return s; }
    pt_ctx* handle() const { return ctx_; }

private:
    int check(int r) const
    {
        if (r < 0) throw Error(r, pt_last_error(ctx_));
        return r;
    }
    pt_ctx* ctx_ = nullptr;
    uint32_t width_ = 0, height_ = 0;
};

// owns a pt_multi: the same pixel loop fanned out over several GPUs of one process (the reference fans it out over the threads of
// one rayon pool, main.rs:72,181); rows are dealt to the devices in strips, one RCCL gather per render
class MultiRenderer
{
public:
    MultiRenderer(const Scene& scene, const Camera& cam, uint32_t width, uint32_t height, uint32_t max_bounces, const std::vector<int32_t>& devices,
                  uint32_t n_sobol = 512, bool enable_nee = true, uint64_t seed = 0x5EED5EEDull)
    {
        pt_config cfg{};
        cfg.width = width; cfg.height = height; cfg.max_bounces = max_bounces; cfg.n_sobol = n_sobol; cfg.enable_nee = enable_nee ? 1u : 0u;
        cfg.seed = seed; cfg.strip_rows = 4; cfg.device = -1;
        m_ = pt_multi_create(&cfg, devices.data(), (uint32_t)devices.size());
        if (!m_) throw Error(PT_ERR_ARG, "pt_multi_create failed (bad configuration)");
        width_ = width; height_ = height;
        pt_ctx* c0 = pt_multi_ctx(m_, 0);
        upload(c0, scene);
        const float eye[3] = {cam.origin.x, cam.origin.y, cam.origin.z}, tgt[3] = {cam.target.x, cam.target.y, cam.target.z};
        if (pt_set_camera(c0, eye, tgt, cam.fov, cam.aspect_ratio) < 0) throw Error(PT_ERR_STATE, pt_last_error(c0));
        if (pt_set_lens(c0, cam.aperture, cam.focus) < 0) throw Error(PT_ERR_ARG, pt_last_error(c0));
    }
    ~MultiRenderer() { if (m_) pt_multi_destroy(m_); }
    MultiRenderer(const MultiRenderer&) = delete;
    MultiRenderer& operator=(const MultiRenderer&) = delete;
    // samples [first_sample, first_sample + n_samples) of every pixel on all devices, gathered on the first; `out` (W*H*4) optional
    void render(uint32_t first_sample, uint32_t n_samples, std::vector<float>* out = nullptr)
    {
        if (out) out->resize((size_t)width_ * height_ * 4);
        check(pt_multi_render(m_, first_sample, n_samples, out ? out->data() : nullptr));
    }
    // the projection of rank 0's camera, replicated to every device by the next render (pt_set_projection)
    void set_projection(const pt_projection& p)
    {
        pt_ctx* c0 = pt_multi_ctx(m_, 0);
        const int r = pt_set_projection(c0, &p);
        if (r < 0) throw Error(r, pt_last_error(c0));
    }
    void reset_accumulation() { check(pt_multi_reset_accumulation(m_)); }
    void write_image(const std::string& path) { check(pt_multi_write_image(m_, path.c_str())); }
    bool used_rccl() const { return pt_multi_used_rccl(m_) == 1; }
    pt_stats stats() const { pt_stats s{}; check(pt_multi_get_stats(m_, &s)); return s; }
    pt_multi* handle() const { return m_; }

private:
    int check(int r) const
    {
        if (r < 0) throw Error(r, pt_multi_last_error(m_));
        return r;
    }
    pt_multi* m_ = nullptr;
    uint32_t width_ = 0, height_ = 0;
};

} // namespace ptmi
