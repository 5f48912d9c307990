// scene.cpp — cold path of the reference restated for the C++ host: Vec3::rotate_point, Camera::new,
// the YAML blueprints, the material factory, the .obj loader and the SoA mesh conversion with its
// padding rule. Arithmetic keeps the reference's f32 evaluation order: what is computed here is
// the exact triangle set and camera the kernel sees.
#include <chrono>
#include <algorithm>
#include <array>
#include <cctype>
#include <charconv>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>

#include "rbrt.hpp"
#include "yaml_lite.hpp"

namespace rbrt {

// vec3.rs:139-155
Vec3 Vec3::rotate_point(const Vec3& rot) const {
    float s_x = std::sin(rot.x), s_y = std::sin(rot.y), s_z = std::sin(rot.z);
    float c_x = std::cos(rot.x), c_y = std::cos(rot.y), c_z = std::cos(rot.z);
    return Vec3((c_x * c_z - c_y * s_x * s_z) * x - (c_x * s_z + c_y * c_z * s_x) * y + s_x * s_y * z,
                (c_z * s_x + c_x * c_y * s_z) * x + (c_x * c_y * c_z - s_x * s_z) * y - c_x * s_y * z,
                s_y * s_z * x + c_z * s_y * y + c_y * z);
}

// cam.rs:22-62
Camera Camera::create(Vec3 position, Vec3 look_at, Vec3 up, uint32_t img_height_pix, uint32_t img_width_pix,
                      float focal_len_mm) {
    Camera c;
    c.right = look_at.normalize().cross_product(up.normalize()).normalize();
    c.img_width_mm = 35.0f;  // full frame sensor
    c.mm_per_pix_hor = c.img_width_mm / float(img_width_pix);
    c.img_height_mm = float(img_height_pix) * c.mm_per_pix_hor;
    c.mm_per_pix_vert = c.img_height_mm / float(img_height_pix);
    c.img_center_point = position + focal_len_mm / 1000.0f * look_at.normalize();
    c.hor_fov_rad = 2.0f * std::atan(2.0f * focal_len_mm / c.img_width_mm);
    c.vert_fov_rad = 2.0f * std::atan(2.0f * focal_len_mm / c.img_height_mm);
    c.img_width_pix = img_width_pix;
    c.img_height_pix = img_height_pix;
    c.position = position;
    c.focal_len_mm = focal_len_mm;
    c.up = up;
    c.look_at = look_at;
    return c;
}

// The thin lens, in float, unfused, in this order:
//   r = aperture_mm / 2000;  lens_u = r right;  lens_v = r normalize(right x normalize(look_at));
//   focus_scale = focus_distance / (focal_len_mm / 1000)
// The image plane lies focal_len_mm / 1000 from the position along look_at, so scaling it about the position by
// focus_scale puts the focus plane focus_distance from the position.
void Camera::set_lens(float aperture_mm, float focus_distance) {
    if (!std::isfinite(aperture_mm) || aperture_mm < 0.0f)
        throw Error("camera_aperture_mm must be a finite number >= 0 (the lens diameter in mm; 0 = pinhole)");
    thin_lens = false, lens_u = Vec3(), lens_v = Vec3(), focus_scale = 0.0f;
    if (aperture_mm == 0.0f) return;
    if (!std::isfinite(focus_distance) || !(focus_distance > 0.0f))
        throw Error("a camera with camera_aperture_mm > 0 needs camera_focus_distance, a finite distance > 0 from the position "
                    "to the plane in focus");
    const float r = aperture_mm / 2000.0f;
    lens_u = r * right;
    lens_v = r * right.cross_product(look_at.normalize()).normalize();
    focus_scale = focus_distance / (focal_len_mm / 1000.0f);
    if (!std::isfinite(focus_scale) || !(focus_scale > 0.0f))
        throw Error("camera_focus_distance / camera_focal_length_mm gives no finite focus scale > 0");
    thin_lens = true;
}

Camera camera_from_blueprint(const CameraBluePrint& bp, uint32_t img_height_pix, uint32_t img_width_pix) {
    Camera c = Camera::create(bp.camera_position, bp.camera_look_at, bp.camera_up, img_height_pix, img_width_pix,
                              bp.camera_focal_length_mm);
    if (bp.camera_aperture_mm) c.set_lens(*bp.camera_aperture_mm, bp.camera_focus_distance ? *bp.camera_focus_distance : 0.0f);
    return c;
}

static void put3(float* dst, Vec3 v) { dst[0] = v.x, dst[1] = v.y, dst[2] = v.z; }

rbrt_camera_lens_t Camera::to_abi_lens() const {
    rbrt_camera_lens_t l{};
    l.cam = to_abi();
    if (thin_lens) {
        put3(l.lens_u, lens_u);
        put3(l.lens_v, lens_v);
        l.focus_scale = focus_scale;
    }
    return l;
}

rbrt_camera_t Camera::to_abi() const {
    rbrt_camera_t a{};
    put3(a.position, position);
    put3(a.right, right);
    put3(a.up, up);
    put3(a.img_center_point, img_center_point);
    a.mm_per_pix_hor = mm_per_pix_hor;
    a.mm_per_pix_vert = mm_per_pix_vert;
    a.img_width_pix = img_width_pix;
    a.img_height_pix = img_height_pix;
    return a;
}

// ---- materials -----------------------------------------------------------------------------------
Material Material::lambertian(Vec3 albedo) {
    Material m;
    m.abi.kind = RBRT_MAT_LAMBERTIAN;
    put3(m.abi.albedo, albedo);
    return m;
}
Material Material::metal(Vec3 albedo, float roughness) {
    Material m;
    m.abi.kind = RBRT_MAT_METAL;
    put3(m.abi.albedo, albedo);
    m.abi.param = roughness;
    return m;
}
Material Material::dielectric(float ref_idx) {
    Material m;
    m.abi.kind = RBRT_MAT_DIELECTRIC;
    m.abi.param = ref_idx;
    return m;
}
Material Material::emissive(Vec3 radiance) {
    Material m;
    m.abi.kind = RBRT_MAT_EMISSIVE;
    put3(m.abi.albedo, radiance);
    return m;
}

// blueprints.rs:50-74: substring match on the lower-cased type, in the order metal, lambert, dielectric; then emissive (not in
// the reference), last so that every name the reference accepts keeps its meaning ("emissive metal" is a metal).
std::optional<Material> create_material_from_description(const std::string& mat_type, std::optional<Vec3> albedo,
                                                         std::optional<float> material_param) {
    std::string t = mat_type;
    std::transform(t.begin(), t.end(), t.begin(), [](unsigned char c) { return char(std::tolower(c)); });
    if (t.find("metal") != std::string::npos) {
        if (!albedo) throw Error("you forgot to specify an albedo vector for metal");
        if (!material_param) throw Error("you forgot to specify a roughness (i.e. material_param: 0.1) for metal");
        return Material::metal(*albedo, *material_param);
    }
    if (t.find("lambert") != std::string::npos) {
        if (!albedo) throw Error("you forgot to specify an albedo vector for lambertian");
        return Material::lambertian(*albedo);
    }
    if (t.find("dielectric") != std::string::npos) {
        if (!material_param)
            throw Error("you forgot to specify a refractory index vector (i.e. material_param: 1.8) dielectric");
        return Material::dielectric(*material_param);
    }
    if (t.find("emissive") != std::string::npos) {
        if (!albedo) throw Error("you forgot to specify an albedo vector (the emitted radiance) for emissive");
        return Material::emissive(*albedo);
    }
    std::printf("Cannot figure out material_type from %s, material_type must be one of metal, lambertian, dielectric or emissive!\n",
                mat_type.c_str());
    return std::nullopt;
}

// ---- YAML -> blueprints ----------------------------------------------------------------------------
namespace {

using yaml_lite::Node;

const Node& need(const Node& m, const char* key, const char* where) {
    if (m.kind != Node::Map) throw Error(std::string(where) + ": expected a mapping");
    const Node* n = m.find(key);
    if (!n) throw Error(std::string(where) + ": missing field `" + key + "`");
    return *n;
}

// Decimal text to a float or double, correctly rounded, whatever LC_NUMERIC the host process has set (strtod and strtof
// obey it): std::from_chars. The text is a number already checked by its caller; false when it is not read to its end.
template <class T>
bool parse_decimal(const char* b, const char* e, T& out) {
    if (b != e && *b == '+') ++b;
    const std::from_chars_result r = std::from_chars(b, e, out, std::chars_format::general);
    if (r.ec == std::errc::result_out_of_range && r.ptr == e) {
        // strtod's answers: +-inf past the largest, +-0 below the smallest. Which of the two: the decimal exponent of the
        // first significant digit, d.ddd x 10^(exp10 + lead - 1), is far from 0 on either side.
        const bool neg = *b == '-';
        const char* ex = std::find_if(b, e, [](char c) { return c == 'e' || c == 'E'; });
        const char* dot = std::find(b, ex, '.');
        const char* p = b + (neg ? 1 : 0);
        while (p != ex && (*p == '0' || *p == '.')) ++p;
        long exp10 = ex != e ? std::strtol(std::string(ex + 1, e).c_str(), nullptr, 10) : 0;
        exp10 = std::max(-1000000L, std::min(1000000L, exp10));
        const long lead = p < dot ? long(dot - p) : -long(p - dot);
        out = exp10 + lead > 0 ? std::numeric_limits<T>::infinity() : T(0);
        if (neg) out = -out;
        return true;
    }
    return r.ec == std::errc() && r.ptr == e;
}

// A number of the YAML 1.2 core schema: [-+]? ( . digits | digits ( . digits* )? ) ( [eE] [-+]? digits )?, 0x / 0o integers,
// [-+]? .inf | .Inf | .INF and .nan | .NaN | .NAN; one `_` between two digits is dropped (YAML 1.1's digit grouping, which
// this reader has always taken). Everything else that strtod would take is refused: hex floats, `inf`, `nan`, `1e_5`.
// serde_yaml hands a YAML float to an f32 field as f64 -> `as f32` (two roundings); mirrored here.
float as_f32(const Node& n, const char* what) {
    if (n.kind != Node::Scalar || n.quoted || n.scalar.empty()) throw Error(std::string(what) + ": expected a number");
    const std::string& t = n.scalar;
    auto invalid = [&]() -> Error { return Error(std::string(what) + ": invalid number `" + t + "`"); };
    {
        const std::string u = (t[0] == '+' || t[0] == '-') ? t.substr(1) : t;
        if (u == ".inf" || u == ".Inf" || u == ".INF")
            return t[0] == '-' ? -std::numeric_limits<float>::infinity() : std::numeric_limits<float>::infinity();
    }
    if (t == ".nan" || t == ".NaN" || t == ".NAN") return std::numeric_limits<float>::quiet_NaN();
    auto digit = [](char c) { return c >= '0' && c <= '9'; };
    if (t.size() > 2 && t[0] == '0' && (t[1] == 'x' || t[1] == 'o')) {  // core-schema hexadecimal and octal integers
        unsigned long long v = 0;
        const std::from_chars_result r = std::from_chars(t.data() + 2, t.data() + t.size(), v, t[1] == 'x' ? 16 : 8);
        if (r.ec != std::errc() || r.ptr != t.data() + t.size()) throw invalid();
        return float(double(v));
    }
    std::string s;
    for (size_t i = 0; i < t.size(); ++i) {
        if (t[i] == '_') {
            if (i == 0 || i + 1 == t.size() || !digit(t[i - 1]) || !digit(t[i + 1])) throw invalid();
            continue;
        }
        s += t[i];
    }
    size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0, int_digits = 0, frac_digits = 0;
    while (i < s.size() && digit(s[i])) ++i, ++int_digits;
    if (i < s.size() && s[i] == '.') {
        ++i;
        while (i < s.size() && digit(s[i])) ++i, ++frac_digits;
    }
    if (int_digits + frac_digits == 0) throw invalid();
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
        size_t exp_digits = 0;
        while (i < s.size() && digit(s[i])) ++i, ++exp_digits;
        if (exp_digits == 0) throw invalid();
    }
    if (i != s.size()) throw invalid();
    double d = 0.0;
    if (!parse_decimal(s.data(), s.data() + s.size(), d)) throw invalid();
    return float(d);
}

Vec3 as_vec3(const Node& n, const char* what) {
    return Vec3(as_f32(need(n, "x", what), what), as_f32(need(n, "y", what), what), as_f32(need(n, "z", what), what));
}

std::string as_string(const Node& n, const char* what) {
    if (n.kind != Node::Scalar) throw Error(std::string(what) + ": expected a string");
    return n.scalar;
}

std::optional<Vec3> opt_vec3(const Node& m, const char* key, const char* what) {
    const Node* n = m.find(key);
    if (!n || n->is_null()) return std::nullopt;
    return as_vec3(*n, what);
}
std::optional<float> opt_f32(const Node& m, const char* key, const char* what) {
    const Node* n = m.find(key);
    if (!n || n->is_null()) return std::nullopt;
    return as_f32(*n, what);
}

const std::vector<Node>& as_list(const Node& n, const char* what) {
    static const std::vector<Node> empty;
    if (n.kind == Node::List) return n.list;
    throw Error(std::string(what) + ": expected a sequence");
}

// A travel `key` of `m` (the camera's camera_shutter_travel, a sphere's shutter_travel; not in the reference): [dx, dy, dz], or
// x / y / z like the other vectors; absent or null: none. `what` ends the message of a vector that is not finite.
std::optional<Vec3> opt_travel(const Node& m, const char* key, const char* what) {
    const Node* tr = m.find(key);
    if (!tr || tr->is_null()) return std::nullopt;
    Vec3 v;
    if (tr->kind == Node::List) {
        if (tr->list.size() != 3) throw Error(std::string(key) + ": expected [dx, dy, dz], three numbers");
        v = Vec3(as_f32(tr->list[0], key), as_f32(tr->list[1], key), as_f32(tr->list[2], key));
    } else {
        v = as_vec3(*tr, key);
    }
    if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z))
        throw Error(std::string(key) + " must be three finite numbers (" + what + ")");
    return v;
}

// The optional checker keys of a sphere or mesh blueprint `m` (not in the reference). The pair checker_albedo / checker_size
// makes one; checker_origin defaults to 0. Whether the material can carry it is decided with the material
// (create_scene_from_scene_blueprint).
std::optional<Checker> opt_checker(const Node& m) {
    const std::optional<Vec3> albedo = opt_vec3(m, "checker_albedo", "checker_albedo");
    const std::optional<float> size = opt_f32(m, "checker_size", "checker_size");
    const std::optional<Vec3> origin = opt_vec3(m, "checker_origin", "checker_origin");
    if (albedo && !size) throw Error("checker_albedo needs checker_size (the edge of a cell, in world units)");
    if (size && !albedo) throw Error("checker_size needs checker_albedo (the albedo of the odd cells)");
    if (origin && !albedo) throw Error("checker_origin needs checker_albedo and checker_size");
    if (!albedo) return std::nullopt;
    if (!std::isfinite(*size) || !(*size > 0.0f) || !std::isfinite(1.0f / *size))
        throw Error("checker_size must be a finite number > 0 whose reciprocal is finite");
    for (const float c : {albedo->x, albedo->y, albedo->z})
        if (!std::isfinite(c) || c < 0.0f) throw Error("checker_albedo must be finite and >= 0");
    Checker ck;
    ck.albedo2 = *albedo, ck.size = *size;
    if (origin) {
        for (const float c : {origin->x, origin->y, origin->z})
            if (!std::isfinite(c)) throw Error("checker_origin must be finite");
        ck.origin = *origin;
    }
    return ck;
}

// A checker goes on a lambertian object only: anything else keeps its one albedo (and a metal's param is its roughness).
void need_lambertian_for_checker(const std::optional<Checker>& ck, const Material& mat, const std::string& material_type) {
    if (ck && mat.abi.kind != RBRT_MAT_LAMBERTIAN)
        throw Error("checker_albedo: a checker needs a lambertian material, not `" + material_type + "`");
}

}  // namespace

rbrt_pattern_t Checker::to_abi() const {
    rbrt_pattern_t p{};
    p.kind = RBRT_PATTERN_CHECKER;
    put3(p.albedo2, albedo2);
    put3(p.origin, origin);
    p.size = size;
    return p;
}

SceneBlueprint load_blueprints_from_yaml_text(const std::string& text) {
    Node root;
    try {
        root = yaml_lite::parse(text);
    } catch (const std::exception& e) {
        throw Error(std::string("Unable to parse content to scene blueprint: ") + e.what());
    }
    SceneBlueprint bp;
    const Node& cam = need(root, "camera_blueprint", "scene");
    bp.camera_blueprint.camera_up = as_vec3(need(cam, "camera_up", "camera_blueprint"), "camera_up");
    bp.camera_blueprint.camera_look_at = as_vec3(need(cam, "camera_look_at", "camera_blueprint"), "camera_look_at");
    bp.camera_blueprint.camera_position = as_vec3(need(cam, "camera_position", "camera_blueprint"), "camera_position");
    bp.camera_blueprint.camera_focal_length_mm =
        as_f32(need(cam, "camera_focal_length_mm", "camera_blueprint"), "camera_focal_length_mm");
    bp.camera_blueprint.camera_aperture_mm = opt_f32(cam, "camera_aperture_mm", "camera_aperture_mm");
    bp.camera_blueprint.camera_focus_distance = opt_f32(cam, "camera_focus_distance", "camera_focus_distance");
    bp.camera_blueprint.camera_shutter_travel = opt_travel(cam, "camera_shutter_travel", "the camera's translation during the exposure");
    {  // (checked here, so that a bad lens is a load error; the CLI's --aperture / --focus-distance are checked again)
        const CameraBluePrint& cb = bp.camera_blueprint;
        const float ap = cb.camera_aperture_mm ? *cb.camera_aperture_mm : 0.0f;
        if (!std::isfinite(ap) || ap < 0.0f)
            throw Error("camera_aperture_mm must be a finite number >= 0 (the lens diameter in mm; 0 = pinhole)");
        if (cb.camera_focus_distance && !(std::isfinite(*cb.camera_focus_distance) && *cb.camera_focus_distance > 0.0f))
            throw Error("camera_focus_distance must be a finite distance > 0");
        if (ap > 0.0f && !cb.camera_focus_distance)
            throw Error("camera_aperture_mm > 0 needs camera_focus_distance (the distance from the position to the plane in focus)");
    }
    for (const Node& m : as_list(need(root, "mesh_blueprints", "scene"), "mesh_blueprints")) {
        TriangleMeshBlueprint b;
        b.obj_filepath = as_string(need(m, "obj_filepath", "mesh blueprint"), "obj_filepath");
        b.scale = as_f32(need(m, "scale", "mesh blueprint"), "scale");
        b.translation = as_vec3(need(m, "translation", "mesh blueprint"), "translation");
        b.rotation_rad = as_vec3(need(m, "rotation_rad", "mesh blueprint"), "rotation_rad");
        b.material_type = as_string(need(m, "material_type", "mesh blueprint"), "material_type");
        b.albedo = opt_vec3(m, "albedo", "albedo");
        b.material_param = opt_f32(m, "material_param", "material_param");
        if (const Node* sh = m.find("shading"); sh && !sh->is_null()) {  // (not in the reference; absent = flat)
            const std::string v = as_string(*sh, "shading");
            if (v != "flat" && v != "smooth") throw Error("shading: expected `flat` or `smooth`, got `" + v + "`");
            b.smooth = v == "smooth";
        }
        b.checker = opt_checker(m);
        try {
            b.shutter_travel = opt_travel(m, "shutter_travel", "the mesh's translation during the exposure");
        } catch (const Error& e) {  // (a message that names the mesh, as the sphere's names the sphere)
            throw Error("mesh " + std::to_string(bp.mesh_blueprints.size()) + ": " + e.what());
        }
        bp.mesh_blueprints.push_back(b);
    }
    for (const Node& s : as_list(need(root, "sphere_blueprints", "scene"), "sphere_blueprints")) {
        SphereBlueprint b;
        b.radius = as_f32(need(s, "radius", "sphere blueprint"), "radius");
        b.center = as_vec3(need(s, "center", "sphere blueprint"), "center");
        b.material_type = as_string(need(s, "material_type", "sphere blueprint"), "material_type");
        b.albedo = opt_vec3(s, "albedo", "albedo");
        b.material_param = opt_f32(s, "material_param", "material_param");
        b.checker = opt_checker(s);
        b.shutter_travel = opt_travel(s, "shutter_travel", "the sphere's translation during the exposure");
        if (b.shutter_travel) {  // (what rbrt_hip_scene_set_motion would refuse, as a load error that names the sphere)
            const Vec3 end(b.center.x + b.shutter_travel->x, b.center.y + b.shutter_travel->y, b.center.z + b.shutter_travel->z);
            if (!std::isfinite(end.x) || !std::isfinite(end.y) || !std::isfinite(end.z))
                throw Error("shutter_travel: center + shutter_travel of sphere " + std::to_string(bp.sphere_blueprints.size()) + " is not finite");
        }
        bp.sphere_blueprints.push_back(b);
    }
    if (const Node* en = root.find("environment_blueprint"); en && !en->is_null()) {  // (not in the reference; absent = none)
        EnvironmentBlueprint e;
        e.file = as_string(need(*en, "file", "environment_blueprint"), "environment_blueprint file");
        if (const auto r = opt_f32(*en, "rotation_deg", "rotation_deg")) e.rotation_deg = *r;
        if (const auto v = opt_f32(*en, "intensity", "intensity")) e.intensity = *v;
        if (const auto v = opt_f32(*en, "resolution", "resolution")) {
            if (!(*v >= 1.0f && *v <= 4096.0f) || *v != std::floor(*v)) throw Error("environment_blueprint: resolution must be an integer between 1 and 4096");
            e.resolution = uint32_t(*v);
        }
        if (e.file.empty()) throw Error("environment_blueprint: file must name a PFM image");
        if (!std::isfinite(e.rotation_deg)) throw Error("environment_blueprint: rotation_deg must be finite");
        if (!std::isfinite(e.intensity) || e.intensity < 0.0f) throw Error("environment_blueprint: intensity must be a finite number >= 0");
        bp.environment_blueprint = e;
    }
    return bp;
}

SceneBlueprint load_blueprints_from_yaml_file(const std::string& filepath) {
    std::ifstream f(filepath, std::ios::binary);
    if (!f) throw Error("Failed to open \"" + filepath + "\" to load content.");
    std::stringstream ss;
    ss << f.rdbuf();
    try {
        return load_blueprints_from_yaml_text(ss.str());
    } catch (const Error& e) {
        throw Error("Unable to parse content of file \"" + filepath + "\" to scene blueprint: " + e.what());
    }
}

// ---- .obj ---------------------------------------------------------------------------------------
namespace {

// One "model" in tobj's sense: a run of faces between o / g / usemtl statements. Its flat index list
// is cut into triples (mesh.rs:96-113 assumes triangles; with tobj's default triangulate=false a
// polygon's indices simply continue the list, and that is reproduced).
struct ObjModel {
    std::vector<uint32_t> indices;
    std::vector<int64_t> normal_indices;  // per index: the corner's `vn` (0-based), or -1 when it names none (or a bad one)
};

// 1-based, negative = relative to the end; -1 when out of range
long obj_index(long v, long n) {
    const long idx = v > 0 ? v - 1 : n + v;
    return (v == 0 || idx < 0 || idx >= n) ? -1 : idx;
}

// One face corner: v, v/vt, v//vn or v/vt/vn, each part an integer or empty, the token read to its end (`1abc` is not `1`).
// Only the position decides whether the face is read (what the loader has always accepted, it still accepts); a missing
// or bad vn leaves normal_out = -1.
bool parse_index(const char*& p, long n_vertices, long n_normals, uint32_t& out, int64_t& normal_out) {
    const char* e = p;
    while (*e && *e != ' ' && *e != '\t' && *e != '\r') ++e;
    long part[3] = {0, 0, 0};
    bool have[3] = {false, false, false};
    int k = 0;
    for (const char* q = p;; ++k) {
        if (k == 3) return false;
        const char* stop = std::find(q, e, '/');
        if (stop != q) {
            const char* digits = (*q == '+' || *q == '-') ? q + 1 : q;  // (from_chars takes no '+')
            const std::from_chars_result r = std::from_chars(*q == '+' ? q + 1 : q, stop, part[k], 10);
            if (digits == stop || *digits < '0' || *digits > '9' || r.ec != std::errc() || r.ptr != stop) return false;
            have[k] = true;
        }
        if (stop == e) break;
        q = stop + 1;
    }
    p = e;
    if (!have[0]) return false;
    normal_out = have[2] ? obj_index(part[2], n_normals) : -1;
    const long idx = obj_index(part[0], n_vertices);
    if (idx < 0) return false;
    out = uint32_t(idx);
    return true;
}

// One number of a `v` or `vn` line: the blank-delimited token, read to its end the way Rust's str::parse::<f32> reads it
// (correctly rounded, `inf` / `nan` / `infinity` in any case, no hex), independent of LC_NUMERIC. False: no such token.
bool parse_obj_float(const char*& p, float& out) {
    while (*p == ' ' || *p == '\t') ++p;
    const char* e = p;
    while (*e && *e != ' ' && *e != '\t' && *e != '\r') ++e;
    if (e == p) return false;
    const char* b = p;
    p = e;
    if ((*b == '+' || *b == '-') && e - b > 1 && (b[1] == '+' || b[1] == '-')) return false;
    return parse_decimal(b, e, out);
}

// Area-weighted vertex normals of one model's transformed triangles: per position index, the unnormalised cross(e1, e2)
// of every triangle corner that uses it, summed in float in face order (corners 0, 1, 2), then normalised. A corner whose
// sum does not normalise to a finite vector (a zero sum) gets its face normal, and a corner of a degenerate triangle whose
// face normal is not finite either gets (0, 0, 0), which the library answers with the stored face normal.
void smooth_model_normals(const std::vector<uint32_t>& idx, const std::array<Vec3, 3>* tris, size_t n_faces,
                          std::vector<Vec3>& acc, std::vector<std::array<Vec3, 3>>& out) {
    for (size_t f = 0; f < n_faces; ++f) {
        const Vec3 c = (tris[f][1] - tris[f][0]).cross_product(tris[f][2] - tris[f][0]);
        for (int k = 0; k < 3; ++k) acc[idx[3 * f + k]] = acc[idx[3 * f + k]] + c;
    }
    auto finite = [](Vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
    for (size_t f = 0; f < n_faces; ++f) {
        std::array<Vec3, 3> cn;
        const Vec3 face = get_triangle_normal(tris[f]);
        for (int k = 0; k < 3; ++k) {
            const Vec3 n = acc[idx[3 * f + k]].normalize();
            cn[k] = finite(n) ? n : finite(face) ? face : Vec3();
        }
        out.push_back(cn);
    }
    for (size_t f = 0; f < n_faces; ++f)
        for (int k = 0; k < 3; ++k) acc[idx[3 * f + k]] = Vec3();
}

}  // namespace

std::vector<std::array<Vec3, 3>> load_mesh_vertices_from_file(const std::string& filepath, Vec3 translation,
                                                              Vec3 rotation, float scale) {
    return load_mesh_from_file(filepath, translation, rotation, scale, false).triangles;
}

ObjMesh load_mesh_from_file(const std::string& filepath, Vec3 translation, Vec3 rotation, float scale, bool smooth) {
    std::ifstream f(filepath, std::ios::binary);
    if (!f) throw Error("assertion failed: loaded_mesh.is_ok() (cannot open " + filepath + ")");
    std::vector<float> positions;
    std::vector<float> normals;        // vn x y z
    std::vector<uint8_t> normal_ok;    // ... read as three finite numbers
    std::vector<ObjModel> models(1);
    std::string line;
    size_t line_no = 0;
    while (std::getline(f, line)) {
        ++line_no;
        const char* p = line.c_str();
        while (*p == ' ' || *p == '\t') ++p;
        if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
            p += 2;
            float v[3] = {0.0f, 0.0f, 0.0f};
            for (int k = 0; k < 3; ++k)
                if (!parse_obj_float(p, v[k])) throw Error(filepath + ":" + std::to_string(line_no) + ": bad vertex");
            positions.insert(positions.end(), v, v + 3);
        } else if (p[0] == 'v' && p[1] == 'n' && (p[2] == ' ' || p[2] == '\t')) {
            p += 3;
            float v[3] = {0.0f, 0.0f, 0.0f};
            bool ok = true;
            for (int k = 0; k < 3; ++k) ok = ok && parse_obj_float(p, v[k]) && std::isfinite(v[k]);
            normals.insert(normals.end(), v, v + 3);
            normal_ok.push_back(ok ? 1 : 0);
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            p += 2;
            const long nv = long(positions.size() / 3), nn = long(normal_ok.size());
            for (;;) {
                while (*p == ' ' || *p == '\t' || *p == '\r') ++p;
                if (!*p) break;
                uint32_t idx;
                int64_t nidx;
                if (!parse_index(p, nv, nn, idx, nidx)) throw Error(filepath + ":" + std::to_string(line_no) + ": bad face index");
                if (nidx >= 0 && !normal_ok[size_t(nidx)]) nidx = -1;
                models.back().indices.push_back(idx);
                models.back().normal_indices.push_back(nidx);
            }
        } else if ((p[0] == 'o' || p[0] == 'g') && (p[1] == ' ' || p[1] == '\t' || p[1] == '\0' || p[1] == '\r')) {
            if (!models.back().indices.empty()) models.emplace_back();
        } else if (std::strncmp(p, "usemtl", 6) == 0) {
            if (!models.back().indices.empty()) models.emplace_back();
        }
    }
    std::vector<std::array<Vec3, 3>> model_vertices;
    std::vector<std::array<Vec3, 3>> corner_normals;
    std::vector<Vec3> acc(smooth ? positions.size() / 3 : 0);
    const float sign = scale > 0.0f ? 1.0f : scale < 0.0f ? -1.0f : 0.0f;  // the normal transform of a uniform scale
    for (const ObjModel& m : models) {
        const size_t first = model_vertices.size(), n_faces = m.indices.size() / 3;
        for (size_t fidx = 0; fidx < n_faces; ++fidx) {
            std::array<Vec3, 3> tri;
            for (int k = 0; k < 3; ++k) {
                const uint32_t i = m.indices[3 * fidx + k];
                Vec3 scaled(positions[3 * i] * scale, positions[3 * i + 1] * scale, positions[3 * i + 2] * scale);
                tri[k] = scaled.rotate_point(rotation) + translation;  // mesh.rs:102-112
            }
            model_vertices.push_back(tri);
        }
        if (!smooth || n_faces == 0) continue;
        bool file_normals = true;
        for (size_t k = 0; k < 3 * n_faces; ++k) file_normals = file_normals && m.normal_indices[k] >= 0;
        if (file_normals) {
            for (size_t fidx = 0; fidx < n_faces; ++fidx) {
                std::array<Vec3, 3> cn;
                for (int k = 0; k < 3; ++k) {
                    const size_t i = size_t(m.normal_indices[3 * fidx + k]);
                    cn[k] = (sign * Vec3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2])).rotate_point(rotation);
                }
                corner_normals.push_back(cn);
            }
        } else {
            smooth_model_normals(m.indices, model_vertices.data() + first, n_faces, acc, corner_normals);
        }
    }
    std::printf("Successfully loaded %zu triangles from file %s!\n", model_vertices.size(), filepath.c_str());
    return ObjMesh{std::move(model_vertices), std::move(corner_normals)};
}

Vec3 get_triangle_normal(const std::array<Vec3, 3>& c) {
    Vec3 edge1 = c[1] - c[0], edge2 = c[2] - c[0];
    return edge1.cross_product(edge2).normalize();
}

void compute_min_max_3d(const std::vector<std::array<Vec3, 3>>& tris, Vec3& lo, Vec3& hi) {
    const float fmax = std::numeric_limits<float>::max();
    lo = Vec3(fmax, fmax, fmax);
    hi = Vec3(-fmax, -fmax, -fmax);
    for (const auto& tri : tris)
        for (const Vec3& v : tri) {
            if (v.x < lo.x) lo.x = v.x;
            if (v.y < lo.y) lo.y = v.y;
            if (v.z < lo.z) lo.z = v.z;
            if (v.x > hi.x) hi.x = v.x;
            if (v.y > hi.y) hi.y = v.y;
            if (v.z > hi.z) hi.z = v.z;
        }
}

// mesh.rs:41-74 + convert_to_soa_mesh (mesh.rs:123-181) including its padding rule: N % lanes copies
// of triangle 0 are appended (not lanes - N % lanes); the kernel side then drops the incomplete chunk.
TriangleMesh TriangleMesh::from_triangles(std::vector<std::array<Vec3, 3>> pre_vertices, Material material,
                                          const std::vector<std::array<Vec3, 3>>* pre_corner_normals) {
    if (pre_corner_normals && pre_corner_normals->size() != pre_vertices.size())
        throw Error("TriangleMesh::from_triangles: one set of corner normals per triangle");
    TriangleMesh m;
    m.material = material;
    m.num_triangles = uint32_t(pre_vertices.size());
    std::vector<Vec3> pre_normals;
    std::vector<std::array<Vec3, 2>> pre_edges;
    for (const auto& t : pre_vertices) pre_normals.push_back(get_triangle_normal(t));
    for (const auto& t : pre_vertices) pre_edges.push_back({t[1] - t[0], t[2] - t[0]});
    compute_min_max_3d(pre_vertices, m.bbox_lower, m.bbox_upper);
    // mesh.rs:27-38 determine_num_vector_lanes(): the reference announces the SIMD layout it picked, once per mesh,
    // after the "Successfully loaded" line. This host always lays meshes out 8 lanes wide (the AVX layout is the one
    // the GPU path restates); on a CPU without AVX the line says so instead of claiming a capability.
    if (__builtin_cpu_supports("avx"))
        std::printf("AVX capability detected!\n");
    else
        std::printf("AVX capability not detected - the GPU path uses the 8-lane (AVX) mesh layout regardless!\n");
    const size_t n = pre_vertices.size();
    const size_t n_pad = n % kNumVectorLanes;
    m.is_padding_triangle.assign(n, 0);
    for (size_t i = 0; i < n_pad; ++i) {
        pre_normals.push_back(pre_normals[0]);
        pre_edges.push_back(pre_edges[0]);
        pre_vertices.push_back(pre_vertices[0]);
        m.is_padding_triangle.push_back(1);
    }
    for (const auto& t : pre_vertices)
        for (int k = 0; k < 3; ++k) {
            m.vertices[k][0].push_back(t[k].x);
            m.vertices[k][1].push_back(t[k].y);
            m.vertices[k][2].push_back(t[k].z);
        }
    for (const auto& e : pre_edges)
        for (int k = 0; k < 2; ++k) {
            m.edges[k][0].push_back(e[k].x);
            m.edges[k][1].push_back(e[k].y);
            m.edges[k][2].push_back(e[k].z);
        }
    for (const Vec3& nn : pre_normals) {
        m.normals[0].push_back(nn.x);
        m.normals[1].push_back(nn.y);
        m.normals[2].push_back(nn.z);
    }
    if (pre_corner_normals && n != 0) {
        for (size_t i = 0; i < n + n_pad; ++i) {
            const std::array<Vec3, 3>& cn = (*pre_corner_normals)[i < n ? i : 0];  // (padding: entry 0's)
            for (int k = 0; k < 3; ++k) {
                m.corner_normals[k][0].push_back(cn[k].x);
                m.corner_normals[k][1].push_back(cn[k].y);
                m.corner_normals[k][2].push_back(cn[k].z);
            }
        }
    }
    return m;
}

LoadTimes& load_times() {
    thread_local LoadTimes t;
    return t;
}

TriangleMesh TriangleMesh::create(const std::string& filepath, Vec3 translation, Vec3 rotation, float scale,
                                  Material material, bool smooth) {
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto t0 = now();
    ObjMesh obj = load_mesh_from_file(filepath, translation, rotation, scale, smooth);
    const auto t1 = now();
    TriangleMesh m = from_triangles(std::move(obj.triangles), material, smooth ? &obj.corner_normals : nullptr);
    load_times().obj_load_s += std::chrono::duration<double>(t1 - t0).count();
    load_times().soa_prep_s += std::chrono::duration<double>(now() - t1).count();
    return m;
}

rbrt_mesh_t TriangleMesh::to_abi() const {
    rbrt_mesh_t a{};
    a.n_total = uint32_t(is_padding_triangle.size());
    a.n_real = num_triangles;
    a.v0x = vertices[0][0].data(), a.v0y = vertices[0][1].data(), a.v0z = vertices[0][2].data();
    a.e1x = edges[0][0].data(), a.e1y = edges[0][1].data(), a.e1z = edges[0][2].data();
    a.e2x = edges[1][0].data(), a.e2y = edges[1][1].data(), a.e2z = edges[1][2].data();
    a.nx = normals[0].data(), a.ny = normals[1].data(), a.nz = normals[2].data();
    a.is_padding = is_padding_triangle.data();
    put3(a.bbox_lo, bbox_lower);
    put3(a.bbox_hi, bbox_upper);
    a.mat = material.abi;
    return a;
}

rbrt_mesh_normals_t TriangleMesh::to_abi_normals() const {
    rbrt_mesh_normals_t a{};
    if (!smooth()) return a;
    a.n0x = corner_normals[0][0].data(), a.n0y = corner_normals[0][1].data(), a.n0z = corner_normals[0][2].data();
    a.n1x = corner_normals[1][0].data(), a.n1y = corner_normals[1][1].data(), a.n1z = corner_normals[1][2].data();
    a.n2x = corner_normals[2][0].data(), a.n2y = corner_normals[2][1].data(), a.n2z = corner_normals[2][2].data();
    return a;
}

Scene::AbiView Scene::to_abi() const {
    AbiView v;
    for (const Sphere& s : elements) {
        rbrt_sphere_t a{};
        put3(a.center, s.center);
        a.radius = s.radius;
        a.mat = s.material.abi;
        v.spheres.push_back(a);
    }
    for (const BasicTriangle& t : basic_triangles) {
        rbrt_triangle_t a{};
        for (int k = 0; k < 3; ++k) put3(a.corners[k], t.corners[k]);
        a.mat = t.material.abi;
        v.triangles.push_back(a);
    }
    for (const TriangleMesh& m : triangle_meshes) {
        v.meshes.push_back(m.to_abi());
        v.normals.push_back(m.to_abi_normals());
        v.any_smooth = v.any_smooth || m.smooth();
    }
    {   // solid patterns, by object id: the elements in their order (element_order, else spheres then triangles), then the meshes
        const size_t n_elem = elements.size() + basic_triangles.size();
        for (size_t e = 0; e < n_elem; ++e) {
            const uint32_t d = element_order.size() == n_elem ? element_order[e] : uint32_t(e < elements.size() ? e : (0x80000000u | (e - elements.size())));
            const size_t idx = d & 0x7FFFFFFFu;
            const std::optional<Checker>* ck = nullptr;
            if ((d >> 31) && idx < basic_triangles.size()) ck = &basic_triangles[idx].checker;
            if (!(d >> 31) && idx < elements.size()) ck = &elements[idx].checker;
            v.pattern_of.push_back(ck && *ck ? (*ck)->to_abi() : rbrt_pattern_t{});
        }
        for (const TriangleMesh& m : triangle_meshes) v.pattern_of.push_back(m.checker ? m.checker->to_abi() : rbrt_pattern_t{});
        for (const rbrt_pattern_t& p : v.pattern_of) v.any_pattern = v.any_pattern || p.kind != RBRT_PATTERN_NONE;
        v.patterns.n_objects = uint32_t(v.pattern_of.size());
        v.patterns.objects = v.pattern_of.data();
    }
    v.shading.n_meshes = uint32_t(v.meshes.size());
    v.shading.meshes = v.normals.data();
    v.scene.n_spheres = uint32_t(v.spheres.size());
    v.scene.spheres = v.spheres.data();
    v.scene.n_triangles = uint32_t(v.triangles.size());
    v.scene.triangles = v.triangles.data();
    if (!element_order.empty()) {
        if (element_order.size() != elements.size() + basic_triangles.size())
            throw Error("Scene::element_order must name every sphere and triangle exactly once");
        v.scene.element_order = element_order.data();
    }
    v.scene.n_meshes = uint32_t(v.meshes.size());
    v.scene.meshes = v.meshes.data();
    return v;
}

std::vector<float> Scene::mesh_motion_travels() const {
    bool any = false;
    for (const TriangleMesh& m : triangle_meshes) any = any || m.shutter_travel.has_value();
    std::vector<float> out;
    if (!any) return out;
    out.assign(triangle_meshes.size() * 3u, 0.0f);
    for (size_t i = 0; i < triangle_meshes.size(); ++i)
        if (const auto& tr = triangle_meshes[i].shutter_travel) out[3 * i] = tr->x, out[3 * i + 1] = tr->y, out[3 * i + 2] = tr->z;
    return out;
}

std::vector<float> Scene::motion_travels() const {
    bool any = false;
    for (const Sphere& s : elements) any = any || s.shutter_travel.has_value();
    std::vector<float> out;
    if (!any) return out;
    out.assign(elements.size() * 3u, 0.0f);
    for (size_t i = 0; i < elements.size(); ++i)
        if (const auto& tr = elements[i].shutter_travel) out[3 * i] = tr->x, out[3 * i + 1] = tr->y, out[3 * i + 2] = tr->z;
    return out;
}

// blueprints.rs:132-158: meshes first (loading the files), then spheres; objects whose material
// cannot be built are dropped.
Scene create_scene_from_scene_blueprint(const SceneBlueprint& bp) {
    Scene scene;
    for (const TriangleMeshBlueprint& mb : bp.mesh_blueprints) {
        auto mat = create_material_from_description(mb.material_type, mb.albedo, mb.material_param);
        if (!mat) {
            std::printf("Failed to parse material info provided with mesh!\n");
            continue;
        }
        need_lambertian_for_checker(mb.checker, *mat, mb.material_type);
        scene.triangle_meshes.push_back(
            TriangleMesh::create(mb.obj_filepath, mb.translation, mb.rotation_rad, mb.scale, *mat, mb.smooth));
        scene.triangle_meshes.back().checker = mb.checker;
        if (mb.shutter_travel) {  // (what rbrt_hip_scene_set_mesh_motion would refuse, as a load error that names the mesh)
            const TriangleMesh& tm = scene.triangle_meshes.back();
            const float corners[6] = {tm.bbox_lower.x, tm.bbox_lower.y, tm.bbox_lower.z, tm.bbox_upper.x, tm.bbox_upper.y, tm.bbox_upper.z};
            const float tv[3] = {mb.shutter_travel->x, mb.shutter_travel->y, mb.shutter_travel->z};
            for (int k = 0; k < 6; ++k) {
                const volatile float end = corners[k] + tv[k % 3];  // (float32, as the library adds it)
                if (std::isfinite(corners[k]) && !std::isfinite(end))
                    throw Error("shutter_travel: box + shutter_travel of mesh " + std::to_string(scene.triangle_meshes.size() - 1) + " is not finite");
            }
            scene.triangle_meshes.back().shutter_travel = mb.shutter_travel;
        }
    }
    for (const SphereBlueprint& sb : bp.sphere_blueprints) {
        auto mat = create_material_from_description(sb.material_type, sb.albedo, sb.material_param);
        if (!mat) continue;
        need_lambertian_for_checker(sb.checker, *mat, sb.material_type);
        scene.elements.push_back(Sphere{sb.center, sb.radius, *mat, sb.checker, sb.shutter_travel});
    }
    return scene;
}

}  // namespace rbrt
