// rbrt.hpp — C++ host-side mirror of the reference's public interface around the hot path.
//
// The reference is a Rust crate; this image has no Rust toolchain, so the host that sits above
// the C ABI (include/rbrt_hip.h) is restated in C++ with the reference's names and argument
// meaning, so a user of rbrt_lib finds the same pieces:
//
//   rbrt_lib::vec3::Vec3                         -> rbrt::Vec3                 (vec3.rs)
//   rbrt_lib::cam::Camera::new                   -> rbrt::Camera::create      (cam.rs:22-62)
//   rbrt_lib::blueprints::*Blueprint             -> rbrt::*Blueprint          (blueprints.rs:15-48)
//   load_blueprints_from_yaml_file               -> same name                 (blueprints.rs:76-92)
//   create_scene_from_scene_blueprint            -> same name                 (blueprints.rs:132-158)
//   rbrt_lib::mesh::TriangleMesh::new            -> rbrt::TriangleMesh::create (mesh.rs:41-74)
//   rbrt_lib::render_scene(cam, samples, scene)  -> rbrt::render_scene        (lib.rs:75-79)
//   image::ImageBuffer<Rgb<u8>>::save            -> rbrt::ImageBuffer::save   (src/main.rs:86)
//
// Where the reference panics (bad YAML, unreadable .obj, unsaveable image) these throw
// rbrt::Error; the CLI turns that into a message and a non-zero exit code.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rbrt_hip.h"

namespace rbrt {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// ---- vec3.rs -----------------------------------------------------------------------------------
struct Vec3 {
    float x = 0, y = 0, z = 0;
    Vec3() = default;
    Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    static Vec3 zero() { return Vec3(); }
    float length() const { return std::sqrt(x * x + y * y + z * z); }
    float sum() const { return x + y + z; }
    Vec3 normalize() const {
        float len = length();
        return Vec3(x / len, y / len, z / len);
    }
    Vec3 cross_product(const Vec3& o) const {
        return Vec3(y * o.z - z * o.y, z * o.x - x * o.z, x * o.y - y * o.x);
    }
    float dot(const Vec3& o) const { return Vec3(x * o.x, y * o.y, z * o.z).sum(); }
    Vec3 rotate_point(const Vec3& rot) const;  // Z-X-Z Euler, vec3.rs:139-155
};
inline Vec3 operator+(Vec3 a, Vec3 b) { return Vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Vec3 operator-(Vec3 a, Vec3 b) { return Vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline Vec3 operator*(Vec3 a, Vec3 b) { return Vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline Vec3 operator*(float s, Vec3 b) { return Vec3(s * b.x, s * b.y, s * b.z); }
inline Vec3 operator*(Vec3 a, float s) { return Vec3(a.x * s, a.y * s, a.z * s); }
inline bool operator==(Vec3 a, Vec3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// ---- cam.rs ------------------------------------------------------------------------------------
struct Camera {
    float hor_fov_rad, vert_fov_rad;
    uint32_t img_width_pix, img_height_pix;
    float img_width_mm, img_height_mm, focal_len_mm;
    Vec3 position, look_at, up, right, img_center_point;
    float mm_per_pix_hor, mm_per_pix_vert;
    // A thin lens (RBRT_FLAG_THIN_LENS; the reference's camera is a pinhole): set_lens fills these, thin_lens stays false
    // for an aperture of 0.
    bool thin_lens = false;
    Vec3 lens_u, lens_v;
    float focus_scale = 0.0f;
    // Camera::new(position, look_at, up, img_height_pix, img_width_pix, focal_len_mm)
    static Camera create(Vec3 position, Vec3 look_at, Vec3 up, uint32_t img_height_pix, uint32_t img_width_pix,
                         float focal_len_mm);
    // aperture_mm: the lens diameter (0: pinhole); focus_distance: scene units from the position to the focus plane along
    // look_at. Throws Error for a negative or non-finite value, or a positive aperture without a focus distance (<= 0).
    void set_lens(float aperture_mm, float focus_distance);
    rbrt_camera_t to_abi() const;
    rbrt_camera_lens_t to_abi_lens() const;  // cam = to_abi(); the lens words are zero for a pinhole
};

// ---- materials (blueprints.rs:50-74) -------------------------------------------------------------
struct Material {
    rbrt_material_t abi{};
    static Material lambertian(Vec3 albedo);
    static Material metal(Vec3 albedo, float roughness);
    static Material dielectric(float ref_idx);
    static Material emissive(Vec3 radiance);  // RBRT_MAT_EMISSIVE: emits `radiance`, scatters nothing
};
// None when the type string matches none of metal / lambert / dielectric (the object is dropped).
std::optional<Material> create_material_from_description(const std::string& mat_type, std::optional<Vec3> albedo,
                                                         std::optional<float> material_param);

// A solid checker (not in the reference; include/rbrt_hip.h rbrt_pattern_t): YAML `checker_albedo`, `checker_size` and
// `checker_origin` on a sphere or mesh blueprint whose material is lambertian.
struct Checker {
    Vec3 albedo2;
    float size = 0;
    Vec3 origin;
    rbrt_pattern_t to_abi() const;
};

// ---- blueprints.rs:15-48 -------------------------------------------------------------------------
struct TriangleMeshBlueprint {
    std::string obj_filepath;
    float scale = 1.0f;
    Vec3 translation, rotation_rad;
    std::string material_type;
    std::optional<Vec3> albedo;
    std::optional<float> material_param;
    bool smooth = false;  // `shading: smooth` (not in the reference): shade with corner normals, rbrt_scene_shading_t
    std::optional<Checker> checker;
    // `shutter_travel: [dx, dy, dz]` (not in the reference): the mesh's translation while the shutter is open, in scene units
    // (include/rbrt_hip.h "Moving meshes"); absent: the mesh stays -- and a scene none of whose meshes has the key has no mesh
    // motion at all
    std::optional<Vec3> shutter_travel;
};
struct SphereBlueprint {
    float radius = 0;
    Vec3 center;
    std::string material_type;
    std::optional<Vec3> albedo;
    std::optional<float> material_param;
    std::optional<Checker> checker;
    // `shutter_travel: [dx, dy, dz]` (not in the reference): the sphere's translation while the shutter is open, in scene
    // units (include/rbrt_hip.h "Moving spheres"); absent: the sphere stays -- and a scene none of whose spheres has the key has
    // no motion at all
    std::optional<Vec3> shutter_travel;
};
struct CameraBluePrint {
    Vec3 camera_up, camera_look_at, camera_position;
    float camera_focal_length_mm = 0;
    std::optional<float> camera_aperture_mm;     // lens diameter in mm; absent or 0: pinhole
    std::optional<float> camera_focus_distance;  // scene units from the position to the focus plane, along look_at
    // `camera_shutter_travel: [dx, dy, dz]` (not in the reference): the camera's translation while the shutter is open, in
    // scene units (include/rbrt_hip.h "Camera shutter"); absent: no shutter
    std::optional<Vec3> camera_shutter_travel;
};
// Camera::create from a blueprint, with its lens (Camera::set_lens) when the blueprint has an aperture.
Camera camera_from_blueprint(const CameraBluePrint& bp, uint32_t img_height_pix, uint32_t img_width_pix);
// `environment_blueprint` (not in the reference): a latitude/longitude radiance image that lights the scene in place of the
// sky gradient (include/rbrt_hip.h "Environment lighting").
struct EnvironmentBlueprint {
    std::string file;           // a colour PFM; row 0 is +y and its middle column looks along -z
    float rotation_deg = 0.0f;  // turns the map about +y
    float intensity = 1.0f;     // finite, >= 0
    uint32_t resolution = 1024; // N of the node grid, 1..4096
};
struct SceneBlueprint {
    CameraBluePrint camera_blueprint;
    std::vector<TriangleMeshBlueprint> mesh_blueprints;
    std::vector<SphereBlueprint> sphere_blueprints;
    std::optional<EnvironmentBlueprint> environment_blueprint;
};
SceneBlueprint load_blueprints_from_yaml_file(const std::string& filepath);
SceneBlueprint load_blueprints_from_yaml_text(const std::string& text);

// ---- sphere.rs / mesh.rs / scene.rs ---------------------------------------------------------------
struct Sphere {
    Vec3 center;
    float radius = 0;
    Material material;
    std::optional<Checker> checker;  // lambertian only
    std::optional<Vec3> shutter_travel;  // the YAML's shutter_travel: absent, the sphere stays
};

// triangle.rs:9-34: a single triangle as a scene element (the reference's second Intersectable). The YAML factory
// never creates one; a C++ caller may (Scene::basic_triangles / element_order below).
struct BasicTriangle {
    std::array<Vec3, 3> corners;  // counter-clockwise
    Material material;
    std::optional<Checker> checker;  // lambertian only
};

struct TriangleMesh {
    // mesh.rs:12-25; vertices[1], vertices[2] are kept like the reference keeps them, although
    // nothing on the hot path reads them.
    std::vector<float> vertices[3][3];
    std::vector<float> edges[2][3];
    std::vector<float> normals[3];
    std::vector<uint8_t> is_padding_triangle;
    Vec3 bbox_lower, bbox_upper;
    Material material;
    uint32_t num_triangles = 0;  // before padding
    std::optional<Checker> checker;  // lambertian only
    std::optional<Vec3> shutter_travel;  // the YAML's shutter_travel: absent, the mesh stays
    // Smooth shading (not in the reference): corner_normals[k][c] = component c of corner k's normal of every SoA entry
    // (padding entries copy entry 0's, as the other arrays do); all empty = a flat mesh.
    std::vector<float> corner_normals[3][3];
    bool smooth() const { return !corner_normals[0][0].empty(); }
    // TriangleMesh::new(filepath, translation, rotation, scale, material), mesh.rs:41-74; smooth: with corner normals
    // (load_mesh_from_file)
    static TriangleMesh create(const std::string& filepath, Vec3 translation, Vec3 rotation, float scale,
                               Material material, bool smooth = false);
    // pre_normals: null (flat) or the three corner normals of every triangle
    static TriangleMesh from_triangles(std::vector<std::array<Vec3, 3>> pre_vertices, Material material,
                                       const std::vector<std::array<Vec3, 3>>* pre_normals = nullptr);
    rbrt_mesh_t to_abi() const;
    rbrt_mesh_normals_t to_abi_normals() const;  // all nine NULL for a flat mesh
};
constexpr uint32_t kNumVectorLanes = 8;  // mesh.rs:28-30: the AVX layout is the one restated

// tobj::load_obj with default LoadOptions, reduced to what mesh.rs:92-114 consumes:
// per-face vertex triples in file order, then scale -> rotate -> translate (mesh.rs:102-112).
std::vector<std::array<Vec3, 3>> load_mesh_vertices_from_file(const std::string& filepath, Vec3 translation,
                                                              Vec3 rotation, float scale);
// The same triangles (and the same stdout line) and, with smooth, every corner's normal, per model (tobj's): the file's
// `vn` transformed as rotate_point(sign(scale) n) when every corner of the model names one, else the area-weighted vertex
// normals of the transformed triangles (scene.cpp smooth_model_normals).
struct ObjMesh {
    std::vector<std::array<Vec3, 3>> triangles;
    std::vector<std::array<Vec3, 3>> corner_normals;  // empty unless smooth
};
ObjMesh load_mesh_from_file(const std::string& filepath, Vec3 translation, Vec3 rotation, float scale, bool smooth);
Vec3 get_triangle_normal(const std::array<Vec3, 3>& corners);                             // triangle.rs:30-34
void compute_min_max_3d(const std::vector<std::array<Vec3, 3>>& tris, Vec3& lo, Vec3& hi);  // aabbox.rs:62-88

// ---- environment lighting (environment.cpp) -------------------------------------------------------
struct PfmImage {
    uint32_t width = 0, height = 0;
    std::vector<float> rgb;  // row-major, TOP row first (the file stores the bottom row first), 3 floats per texel
};
// A colour (`PF`) Portable Float Map, either byte order (the sign of the scale). Throws Error, with the reason, for anything
// else: a grey `Pf`, a bad size or scale, a truncated file, bytes after the pixels, a texel that is not finite or is negative.
// any_value: texels are taken as they are (what write_pfm wrote, NaN and negative values included), bit for bit.
PfmImage read_pfm(const std::string& path, bool any_value = false);
// A colour PFM of a row-major image, top row first: `PF`, little-endian (scale -1.0), rows bottom to top. Linear radiance leaves
// the host this way (--radiance); ImageBuffer::save stays with the reference's 8-bit formats. Throws Error.
void write_pfm(const std::string& path, const float* rgb, uint32_t width, uint32_t height);
// The (n + 1) x (n + 1) x 3 nodes of rbrt_environment_t from a latitude/longitude image (DESIGN.md "Environment lighting").
std::vector<float> environment_nodes_from_latlong(const PfmImage& img, uint32_t n, double rotation_deg, double intensity);
struct Environment {
    uint32_t n = 0;            // 0: none
    std::vector<float> nodes;  // float[n+1][n+1][3]
    std::string file;          // where it came from (--report)
    rbrt_environment_t to_abi() const { return rbrt_environment_t{n, 0u, nodes.data()}; }
};
// Reads the blueprint's image and converts it. create_scene_from_scene_blueprint mirrors the reference and knows nothing of
// environments: a host assigns the result to Scene::environment itself (main.cpp, c_api.cpp).
Environment load_environment(const EnvironmentBlueprint& bp);
// What a checkpoint of a render with an environment must match besides the scene: `h` itself when there is none.
uint64_t environment_fingerprint(const Environment& e, uint64_t h);

struct Scene {
    // scene.rs:12-16: `elements: Vec<Box<dyn Intersectable + Sync>>` holds Spheres and BasicTriangles. Here the two
    // kinds sit in their own vectors; `element_order` gives the order Scene::hit tests them in (scene.rs:23-31: an
    // earlier element keeps a tie) as entries (index, or 0x80000000 | index for a triangle) -- empty = all spheres,
    // then all triangles, which is what every scene the YAML factory can build looks like.
    std::vector<Sphere> elements;
    std::vector<BasicTriangle> basic_triangles;
    std::vector<uint32_t> element_order;
    std::vector<TriangleMesh> triangle_meshes;
    Environment environment;  // n == 0: rays that hit nothing see the background (render_scene sets it on every rank's handle)
    // POD view for the C ABI; valid while this Scene is alive and unmodified.
    struct AbiView {
        std::vector<rbrt_sphere_t> spheres;
        std::vector<rbrt_triangle_t> triangles;
        std::vector<rbrt_mesh_t> meshes;
        rbrt_scene_t scene{};
        std::vector<rbrt_mesh_normals_t> normals;  // [mesh]
        rbrt_scene_shading_t shading{};
        bool any_smooth = false;
        // what rbrt_hip_scene_create_shaded gets: NULL when no mesh is smooth
        const rbrt_scene_shading_t* shading_ptr() const { return any_smooth ? &shading : nullptr; }
        std::vector<rbrt_pattern_t> pattern_of;  // [object id]: the elements in their order, then the meshes
        rbrt_scene_patterns_t patterns{};
        bool any_pattern = false;
        // what rbrt_hip_scene_create_patterned gets: NULL when no object carries a checker
        const rbrt_scene_patterns_t* patterns_ptr() const { return any_pattern ? &patterns : nullptr; }
    };
    AbiView to_abi() const;
    // The scene's motion (rbrt_motion_t::travel): [elements.size()][3], zeros for the spheres without a shutter_travel; EMPTY
    // when no sphere has one (no motion: no draw is made for it). A key with a zero vector counts: its scene has a motion.
    std::vector<float> motion_travels() const;
    // The scene's mesh motion (rbrt_mesh_motion_t::travel): [triangle_meshes.size()][3], zeros for the meshes without a
    // shutter_travel; EMPTY when no mesh has one (no mesh motion). A key with a zero vector counts.
    std::vector<float> mesh_motion_travels() const;
};
Scene create_scene_from_scene_blueprint(const SceneBlueprint& bp);
// Where create_scene_from_scene_blueprint spent its time, summed over the meshes of the calling thread's scenes (--report).
struct LoadTimes {
    double obj_load_s = 0;   // reading and parsing the .obj files, transforming the vertices (mesh.rs:78-121)
    double soa_prep_s = 0;   // edges, normals, padding, SoA arrays, bounding box (mesh.rs:41-74, :123-181)
};
LoadTimes& load_times();

// ---- image + render --------------------------------------------------------------------------------
struct ImageBuffer {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> rgb;        // row-major, 3 bytes per pixel
    std::vector<float> radiance;     // row-major fp32 pre-gamma mean (extra to the reference); linear whatever the display transform
    std::vector<uint8_t> sample_map; // an adaptive render: one byte per pixel, its tile's sample count * 255 / samples (else empty)
    std::vector<uint8_t> noisy_rgb;  // a denoised render with RenderConfig::keep_noisy: the unfiltered image, like rgb (else empty)
    // a render with RenderConfig::features: the feature buffers of the primary rays, row-major (else empty)
    std::vector<float> feature_albedo, feature_normal;  // 3 floats per pixel
    std::vector<float> feature_motion;                  // 3 floats per pixel; empty unless the scene has a motion, of spheres or meshes (PREFIX.motion.pfm)
    std::vector<float> feature_depth, feature_coverage; // 1 float per pixel
    std::vector<uint8_t> history_map;  // a render with RenderConfig::frames: one byte per pixel, the last frame's len * 255 / max_history (else empty)
    std::vector<uint8_t> spike_map;  // a render with RenderConfig::despike: one byte per traced pixel of the last frame, 0 none, 85 A, 170 B, 255 both (else empty)
    uint32_t spike_map_width = 0, spike_map_height = 0;  // ... and its size: the traced one, which RenderConfig::upscale makes smaller than the image's
    void save_features(const std::string& prefix) const;  // PREFIX.albedo.pfm, .normal.pfm, .depth.pfm, .coverage.pfm (colour PFMs; grey as three equal channels)
    void save(const std::string& path) const;  // .png (8-bit RGB) or .ppm by extension
    void save_sample_map(const std::string& path) const;  // the sample map as a grey image, through the same writers
    void save_noisy(const std::string& path) const;       // the unfiltered image of a denoised render, through the same writers
};
void write_png(const std::string& path, const uint8_t* rgb, uint32_t width, uint32_t height);

// What render_scene measured (wall clock; with several GPUs the slowest rank's figure). The reference prints only
// "Starting rendering..." and a progress line (lib.rs:80,105-110); a 4 ms render needs more than that to be understood.
struct RenderReport {
    double upload_build_s = 0;   // rbrt_hip_scene_create + the render's buffers, the slowest rank's (= the four below + buffers_s)
    double hip_init_s = 0;       // the HIP runtime's start-up (the process's first HIP call) + device selection
    double upload_s = 0;         // scene arrays to the device
    double bvh_build_s = 0;      // BVH construction (whichever builder made the first trees)
    double lanes_s = 0;          // the library's streams, events, per-wave scratch, device code
    double buffers_s = 0;        // this host's stream and image buffers
    double release_s = 0;        // buffers and scene released
    double render_s = 0;         // all passes, incl. checkpoint writes
    double gather_s = 0;         // image to host memory (and the merge of the ranks' tiles)
    uint32_t passes = 0, pass_spp = 0, checkpoints_written = 0, resumed_from_sample = 0;
    int n_gpus = 1;
    std::string gather = "none";    // none (one GPU) | host | rccl
    std::string builder = "none";   // who built the BVHs: host | device | mixed | none (no mesh)
    uint64_t bvh_nodes = 0, bvh_triangles = 0;
    // an adaptive render (RenderConfig::adaptive): rbrt_adaptive_result_t and the tiles active at the start of each round
    uint32_t adaptive_rounds = 0;
    uint64_t adaptive_samples = 0, adaptive_samples_fixed = 0;
    std::vector<uint32_t> adaptive_active_tiles;
    double denoise_ms = 0.0;  // a denoised render (RenderConfig::denoise): rbrt_hip_scene_denoise on the GPU, between two events
    // a render with the display transform (RenderConfig::tonemap): e and w as used, the pixels the luminance histogram counted
    // (0 when nothing was automatic) and rbrt_hip_tonemap on the GPU, between two events
    float tonemap_exposure = 1.0f, tonemap_white = 1.0f;
    uint32_t luminance_counted = 0;
    double tonemap_ms = 0.0;
    double glare_ms = 0.0;  // a render with glare (RenderConfig::glare): rbrt_hip_glare on the GPU, between two events
    double guided_ms = 0.0;  // a render with the guided filter (RenderConfig::denoise_guided): rbrt_hip_scene_denoise_guided, between two events
    double features_ms = 0.0;  // a render with feature buffers (RenderConfig::features): rbrt_hip_render_features, between two events
    double upsample_ms = 0.0;  // a render with guided upsampling (RenderConfig::upscale): rbrt_hip_upsample_halves between two events, the mean per frame
    uint32_t render_width = 0, render_height = 0;  // ... and the size that was traced
    double despike_ms = 0.0;  // a render with spike removal (RenderConfig::despike): rbrt_hip_despike_halves between two events, the mean per frame
    double spikes_a = 0.0, spikes_b = 0.0;  // ... and the pixels it limited in either half image, the mean per frame
    double temporal_ms = 0.0;  // a render of several frames (RenderConfig::frames): rbrt_hip_temporal_accumulate between two events, the mean per frame
};

struct RenderConfig {  // additions that the reference hard-codes or lacks
    uint64_t seed = 1;
    int n_gpus = 1;
    bool quiet = false;
    uint32_t pass_spp = 0;            // samples per pass (progress line / checkpoint granularity); 0 = automatic
    std::string checkpoint_path;      // non-empty: resume from / write per-pass checkpoints of the running sums here
    int checkpoint_every = 1;         // ... after every n-th pass
    // multi-GPU: "host" (every rank copies its tiles over its own PCIe link, merged on the host: the image has to
    // end up there anyway) or "rccl" (device-to-device over xGMI to GPU 0, then one copy; librccl is dlopen'ed)
    std::string gather = "host";
    bool oversubscribe = false;       // rank r runs on device r % n_devices (rehearsal of N ranks on fewer GPUs; host gather only)
    RenderReport* report = nullptr;   // filled in when not null
    bool constant_background = false; // RBRT_FLAG_CONSTANT_BACKGROUND: escaped rays return `background` (the CLI's --background)
    float background[3] = {0.0f, 0.0f, 0.0f};
    // Adaptive sampling (rbrt_hip_render_adaptive; the CLI's --adaptive): num_samples is the limit, a tile stops once its error
    // estimate is below the threshold. One GPU, no checkpoint, no passes: render_scene refuses the combination by name.
    bool adaptive = false;
    float adaptive_threshold = 0.0f;
    uint32_t adaptive_min_samples = 16, adaptive_step = 64;  // (the step: profiles/adaptive_config2.txt)
    // Denoising (rbrt_hip_scene_denoise; the CLI's --denoise): the image is the dual-buffer non-local-means filter of the
    // render's two half sums. It works on the sums of the adaptive path: without `adaptive` the render goes through that path
    // with threshold 0 and min_samples = step = num_samples, which is one round and bit for bit the fixed render. Inherits
    // every refusal of `adaptive`; num_samples must be at least 2 (a half would be empty).
    bool denoise = false;
    uint32_t denoise_window_radius = 5, denoise_patch_radius = 3;  // (rbrt_denoise_opts_default)
    float denoise_strength = 0.7f;
    bool keep_noisy = false;  // also keep the unfiltered RGB8 image (ImageBuffer::noisy_rgb)
    // The display transform (rbrt_hip_tonemap; the CLI's --exposure, --tonemap, --white): ImageBuffer::rgb (and noisy_rgb, with
    // the same e and w) is the quantisation of the transformed image; ImageBuffer::radiance stays linear. It runs once, on the
    // complete image, on rank 0's device: on the radiance that is there already, or on the gathered image.
    bool tonemap = false;
    uint32_t tonemap_curve = RBRT_TONE_LINEAR;
    float tonemap_exposure = 1.0f;  // the multiplier; 0: automatic, the luminance at tonemap_key's rank is mapped to tonemap_key
    float tonemap_key = 0.18f;
    float tonemap_white = 0.0f;     // Reinhard's white point; 0: automatic
    // Glare (rbrt_hip_glare; the CLI's --glare, --glare-threshold, --glare-levels, --glare-spread): it runs once, on the complete
    // image, directly in front of the display transform (denoise -> glare -> display transform), so automatic exposure sees
    // the glared image. Without a display transform ImageBuffer::rgb is the glare call's own rgb8. ImageBuffer::radiance
    // stays the scene's radiance without glare.
    bool glare = false;
    float glare_intensity = 0.1f, glare_threshold = 1.0f, glare_spread = 1.0f;  // (rbrt_glare_opts_default)
    uint32_t glare_levels = 5;
    // Feature buffers (rbrt_hip_render_features; the CLI's --features, --feature-samples): after the render, on the same
    // handle, the albedo, normal, depth and coverage of the primary rays, feature_samples samples a pixel, into
    // ImageBuffer::feature_*. One GPU: render_scene refuses the combination with more by name.
    bool features = false;
    uint32_t feature_samples = 4;  // 1..65536
    // Guided denoising (rbrt_hip_scene_denoise_guided; the CLI's --denoise-guided, --guided-*): the image is the edge-avoiding
    // a-trous filter of the render's two half sums, guided by the feature buffers, which are made on the same handle with
    // feature_samples samples a pixel whether `features` is set or not. Goes through the adaptive path like `denoise`, inherits
    // its refusals, and cannot be combined with it; keep_noisy works as with `denoise`.
    bool denoise_guided = false;
    uint32_t guided_levels = 5;  // (rbrt_guided_opts_default)
    float guided_colour = 2.0f, guided_normal = 0.35f, guided_depth = 0.05f, guided_albedo = 0.1f;
    bool guided_demodulate = true;  // false: RBRT_GUIDED_NO_DEMODULATION
    // Temporal accumulation (rbrt_hip_temporal_accumulate; the CLI's --frames, --camera-step, --temporal-*): `frames` frames are
    // rendered and the last one is the image. Frame k has the camera's position and image centre moved by float(k) * camera_step
    // (float32, per component) and renders with seed + k; each frame goes through the adaptive path's one round that stops
    // nothing, gives its half images and its feature buffers (feature_samples a pixel), and is accumulated onto the history of
    // the frames before it. The accumulated halves of the last frame then go through the guided filter (denoise_guided), the
    // non-local-means filter (denoise) or, with neither, their plain mix. Inherits the adaptive path's refusals; not with
    // `adaptive` itself; num_samples must be at least 2. 0: one frame without any of this.
    uint32_t frames = 0;
    float camera_step[3] = {0.0f, 0.0f, 0.0f};
    // The camera shutter (rbrt_hip_scene_set_shutter; the YAML's camera_shutter_travel, the CLI's --shutter-travel and
    // --shutter): every rank's handle gets it, so every frame, pass and round and the feature buffers are exposed while the
    // camera moves by shutter_travel. With --frames, frame k opens at k * camera_step as without a shutter, and the
    // accumulation reprojects through the frames' opening cameras.
    bool shutter = false;
    float shutter_travel[3] = {0.0f, 0.0f, 0.0f};
    // Moving spheres (rbrt_hip_scene_set_motion): the spheres' shutter_travel keys go to every rank's handle like the shutter,
    // with which they share the draw; with --frames every frame exposes the same sweep (objects do not advance from frame to
    // frame). no_motion (the CLI's --no-motion): the keys are ignored, the scene renders as if it had none.
    bool no_motion = false;
    // Animation (rbrt_hip_scene_set_motion_phase; the CLI's --motion-step, which needs --frames): frame k runs at the phase
    // float(k) * motion_step, and with a motion and a step other than 0 the frame loop asks the features call for the motion
    // buffer and accumulates with rbrt_hip_temporal_accumulate_moving. 0: every frame exposes the same sweep, as without the flag.
    float motion_step = 0.0f;
    float temporal_max_history = 32.0f, temporal_depth = 0.05f, temporal_normal = 0.35f;  // (rbrt_temporal_opts_default)
    // Guided upsampling (rbrt_hip_upsample_halves; the CLI's --upscale, --upscale-*): the image is traced with the low camera of
    // rbrt_hip_upsample_camera (1 / upscale of the size in each direction) through the adaptive path's one round that stops
    // nothing, its two half images are brought to full size under the guidance of the full camera's feature buffers
    // (feature_samples a pixel), and everything behind that -- `frames`, the filters, glare, the display transform -- runs at
    // full size as it does without. With keep_noisy the unfiltered image is the plain mix of the upsampled halves (of the last
    // frame, before its accumulation). Inherits the adaptive path's refusals; not with `adaptive` itself; num_samples must be at
    // least 2. 0: the image is traced at its own size.
    uint32_t upscale = 0;  // 0, or 2..RBRT_UPSAMPLE_MAX_FACTOR
    float upscale_normal = 0.5f, upscale_depth = 0.1f, upscale_albedo = 0.2f;  // (rbrt_upsample_opts_default)
    // Spike removal (rbrt_hip_despike_halves; the CLI's --despike, --despike-*): the render goes through the adaptive path's one
    // round that stops nothing, like `frames` and `upscale`, and its two half images are limited right behind the handle, at the
    // size that was traced, in front of upsampling, accumulation and either filter. keep_noisy keeps its meaning: the render's own
    // image, in front of the stage (with `upscale`: the upsampled halves' mix). Inherits the adaptive path's refusals; not with
    // `adaptive` itself; num_samples must be at least 2. ImageBuffer::spike_map is the last frame's mask.
    bool despike = false;
    uint32_t despike_radius = 2, despike_rank = 2;  // (rbrt_despike_opts_default; the floor stays the library's)
    float despike_threshold = 4.0f;
};
// What compare_images found (rbrt_hip.h "Image comparison"): the stage's result as it left the device, the means of it with a peak
// of 1, the stage's time between two events, and the maps that were asked for, one float per pixel (else empty).
struct ImageComparison {
    uint32_t width = 0, height = 0;
    rbrt_compare_result_t result{};
    rbrt_compare_summary_t summary{};
    double ms = 0.0;
    std::vector<float> rel_map, ssim_map;
};
// The image's linear radiance against a reference of the same size (the CLI's --compare, --compare-epsilon, --error-map,
// --ssim-map): uploads both to device 0, runs rbrt_hip_compare_images between two events and brings back what it made.
// Throws Error: another size, a bad epsilon, anything the device refuses.
ImageComparison compare_images(const ImageBuffer& img, const PfmImage& ref, float epsilon = 0.01f, bool want_rel_map = false, bool want_ssim_map = false);
// rbrt_lib::render_scene (lib.rs:75-79): blocks until the image is complete. Runs on the GPU(s)
// through the C ABI; there is no CPU path.
ImageBuffer render_scene(const Camera& cam, uint32_t num_samples, const Scene& scene, const RenderConfig& cfg = {});

}  // namespace rbrt
