// Host side of Scene::new (src/scene.rs:21-35): BLAS / TLAS builders, light sampler, camera matrices and the
// flattening into the device layout of pt_types.h.  Runs once per scene on the CPU, no GPU involved.
#pragma once
#include <string>
#include <vector>

#include "pt_types.h"

namespace pt {

struct HostBox { f3 mn, mx; };

struct HostNode
{
    HostBox box;
    uint32_t kind; // NODE_BRANCH / NODE_TRIS / NODE_INSTANCE
    uint32_t a, b; // branch: left,right (arena-local); tris: first,count into prim_ids; instance: instance index, blas index
};

struct HostTriangle
{
    f3 p[3], n[3];
    f4 n0, n1, n2; // primitive.rs:20-26
};

struct HostBlas
{
    std::vector<HostTriangle> tris;   // load order (Id<Triangle>)
    std::vector<HostNode> nodes;      // arena order (children before parents)
    std::vector<uint32_t> prim_ids;   // leaf contents, in leaf order
    uint32_t root = 0;
    uint32_t depth = 0;               // nodes on the longest root->leaf path
    int material = 0;
};

struct HostInstance
{
    uint32_t blas;  // arena index inside the owning TLAS
    uint32_t model; // model index (== world blas index)
    xf34 fwd, inv;
};

struct HostTlas
{
    std::vector<HostNode> nodes;
    std::vector<HostInstance> instances; // leaf allocation order
    uint32_t root = MISS_ID;
    uint32_t depth = 0;
    std::vector<uint32_t> models;        // arena index -> model index
};

struct HostModel
{
    std::vector<float> positions, normals; // n_tris * 9
    std::vector<float> uvs;                // n_tris * 6 (three UVs per triangle, load order), or empty: (0, 0) at every vertex
    uint32_t n_tris = 0;
    int material = 0;
    std::vector<xf34> matrices;
};

struct HostTexture
{
    uint32_t w = 0, h = 0;
    std::vector<float> rgb;                // w * h * 3, linear, row-major
};

struct HostLight { uint32_t blas, prim; float pdf, cdf; };

struct HostCamera
{
    bool set = false;
    float yaw = 0, pitch = 0; // as the reference names them: pitch is the Y angle, yaw the X angle of EulerRot::YXZ (camera.rs:23)
    xf34 matrix;          // camera-to-world
    float inv_proj[16];   // column-major
    float ray_matrix[16]; // matrix * inv_projection, column-major
    // thin lens (Camera::new's 5th and 6th argument, camera.rs:17; pt_set_lens).  aperture 0 = pinhole.  Not touched by set_camera or the input
    float aperture = 0, focus = 0;
    // panoramic / orthographic projection (pt_set_projection): kind PROJ_PERSPECTIVE = the camera above.  Not touched by set_camera or the input
    // either; aspect is set_camera's (the orthographic view volume's width is its height times it)
    uint32_t proj_kind = PROJ_PERSPECTIVE;
    float span_x_deg = 0, span_y_deg = 0, ortho_height = 0;
    float aspect = 1;
};

struct FlatScene
{
    std::vector<DNode> nodes;
    std::vector<DTriIsect> tri_isect;
    std::vector<DTriVerts> tri_shade, tri_pos;
    std::vector<uint32_t> tri_orig;
    std::vector<DTriUV> tri_uv;         // leaf order like tri_shade; empty unless some material references a texture (has_textures)
    std::vector<DTexture> tex_table;    // ... and so are the texture table and the texels (every texture, in pt_add_texture order)
    std::vector<f4> tex_texels;
    std::vector<f4> tri_tan;            // per-triangle tangent.xyz | handedness, leaf order like tri_uv; empty unless some material references a normal map (has_normal_maps)
    std::vector<DInstance> instances;
    std::vector<uint32_t> big_leaves;   // {first, count} pairs of the leaves NODE_TRIS cannot encode
    std::vector<DMaterial> materials;
    std::vector<DLight> lights;
    std::vector<uint32_t> tri_base;     // per model: absolute index of its first triangle
    std::vector<uint32_t> inst_base;    // [0] world instances start, [1] lights instances start
    uint32_t world_root = MISS_ID, lights_root = MISS_ID;
    uint32_t prim_bits = 0;
    uint32_t stack_entries = 0;
    uint32_t ident_tlas = 0;            // IDENT_TLAS_WORLD / IDENT_TLAS_LIGHTS: every instance of that TLAS carries INSTANCE_IDENTITY
    float light_weight_sum = 0;
    bool has_volumes = false;
    bool has_textures = false;          // some material references a texture, as its surface colour, its emission, its normal map or its roughness map: the shading passes are the TEX variants
    bool has_emission_textures = false; // ... and some EMISSIVE material does (pt_set_material_emission_texture)
    bool has_normal_maps = false;       // some material references a normal texture (pt_set_material_normal_texture): has_textures too, and tri_tan is written
    TexView tex_view() const { return TexView{tex_texels.data(), tex_table.data(), tri_uv.data()}; } // over the host copies
    TexNView texn_view() const { return TexNView{tex_view(), tri_tan.data()}; }
    // bytes of every table an upload copies (pt_scene_info::scene_bytes)
    size_t table_bytes() const
    {
        return nodes.size() * sizeof(DNode) + tri_isect.size() * sizeof(DTriIsect) + instances.size() * sizeof(DInstance) + (big_leaves.size() * 4 + 15) / 16 * 16 +
               (tri_shade.size() + tri_pos.size()) * sizeof(DTriVerts) + tri_orig.size() * 4 + materials.size() * sizeof(DMaterial) + lights.size() * sizeof(DLight) +
               tri_uv.size() * sizeof(DTriUV) + tex_table.size() * sizeof(DTexture) + tex_texels.size() * sizeof(f4) + tri_tan.size() * sizeof(f4);
    }
};

class HostScene
{
public:
    std::vector<DMaterial> materials;
    std::vector<HostModel> models;
    std::vector<HostTexture> textures;
    std::vector<HostBlas> blas;         // one per model
    HostTlas world, lights;
    std::vector<HostLight> light_items;
    float light_weight_sum = 0;
    HostCamera camera;
    FlatScene flat;
    bool built = false;
    // Incremental builds (pt_set_instances): BLASes live in object space, so one is built once per model and kept; layout_epoch counts the
    // edits that move offsets in the flattened scene (a model or material added, an instance count changed) — an upload that finds the
    // epoch it last saw can patch the TLAS nodes and instance records in place.
    uint64_t layout_epoch = 0;
    uint64_t blas_builds = 0, tlas_builds = 0;
    bool tlas_valid = false;    // the two TLASes and the light sampler are those of the current models, materials and matrices: an edit that
                                // touches none of them (a texture, a material's texture reference, a model's UVs) leaves them standing
    bool lights_valid = false;  // the light sampler's weights are current: an emission texture, or new UVs on a model that has one, ends that
    bool flat_valid = false;    // `flat` is a finished flatten of layout_epoch flat_epoch: its BLAS nodes and per-triangle tables can be kept
    uint64_t flat_epoch = 0;

    int add_material(int kind, const float colour[3], float roughness, float ior, bool has_volume, const float vol_abs[3], float k, float c,
                     float g);
    int add_model(const float* positions, const float* normals, uint32_t n_tris, int material, const float* affines, uint32_t n_inst);
    // (the OBJ reader's: with the UVs it read, empty for a file without `vt`)
    int add_model(const float* positions, const float* normals, uint32_t n_tris, int material, const float* affines, uint32_t n_inst, std::vector<float>&& uvs);
    // load_obj (blas.rs:44-131) + add_model; returns the model index, -1 bad argument, -4 non-rigid, -6 unreadable file, -7 parse error
    int add_model_obj(const char* path, int material, const float* affines, uint32_t n_inst, std::string* err);
    // replaces the instance matrices of a model (checked as add_model checks them); -1 bad argument, -4 non-rigid: nothing changed
    int set_instances(int model, const float* affines, uint32_t n_inst);
    // textures (the definition is include/pt_api.h's).  Each returns -1 for a bad argument, -5 for the packing limit; nothing changed then
    enum : uint64_t { kMaxTextureSide = 16384u, kMaxTexels = 1ull << 28 }; // per side; texels of all textures together (32-bit f4 offsets, 4 GiB)
    int add_texture(uint32_t w, uint32_t h, const float* rgb);
    int set_material_texture(int material, int texture);             // -1 clears
    int set_material_emission_texture(int material, int texture);    // -1 clears; EMISSIVE materials only (the light sampler is rebuilt)
    int set_material_normal_texture(int material, int texture);      // -1 clears; any kind but EMISSIVE
    int set_material_roughness_texture(int material, int texture);   // -1 clears; the two GGX kinds only
    int set_model_uvs(int model, const float* uv, uint32_t n_tris);  // nullptr, 0 clears
    int build(std::string* err);
    void set_camera(const float eye[3], const float target[3], float fov_deg, float aspect);
    void create_ray(float s, float t, float o[3], float d[3]) const;
    // what the kernels are given of the camera (CameraView) and of its lens (LensView; radius 0 = pinhole)
    CameraView camera_view() const;
    LensView lens_view() const;
    ProjView proj_view() const; // (kind PROJ_PERSPECTIVE: nothing else is read)
    CameraOptics optics_view() const { return CameraOptics{lens_view(), proj_view()}; }
    // the camera ray of (pixel, sample) as the kernels make it (pt_camera.h), pinhole, lens, panoramic or orthographic; returns the stream draws it consumed
    uint32_t primary_ray(uint32_t width, uint32_t height, uint32_t n_sobol, uint64_t seed, uint32_t pixel, uint32_t sample, float o[3], float d[3]) const;
    void inv_projection(float out16[16]) const; // (matrix * inv_projection).inverse()  main.rs:128
    void camera_move(float dx, float dz, float dt);   // Camera::update_origin    camera.rs:33-39
    void camera_rotate(float dx, float dy, float dt); // Camera::update_rotation  camera.rs:41-54

private:
    void build_blas(HostBlas& out, const HostModel& m);
    void build_tlas(HostTlas& out, const std::vector<uint32_t>& model_ids);
    void build_lights();
    int flatten(std::string* err);
    void refresh_ray_matrix();
};

} // namespace pt
