// c_api.cpp — C entry points of the host library for non-C++ callers (Python ctypes in tests/bench).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "checkpoint.hpp"
#include "rbrt.hpp"
#include "yaml_lite.hpp"

namespace {
thread_local std::string g_err;

void json_string(std::string& out, const std::string& s) {
    out += '"';
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') {
            out += '\\';
            out += char(c);
        } else if (c < 0x20 || c == 0x7f) {
            char buf[8];
            std::snprintf(buf, sizeof buf, "\\u%04x", unsigned(c));
            out += buf;
        } else {
            out += char(c);  // (UTF-8 passes through)
        }
    }
    out += '"';
}

void json_node(std::string& out, const yaml_lite::Node& n) {
    using yaml_lite::Node;
    switch (n.kind) {
        case Node::Null: out += "null"; break;
        case Node::Scalar:
            out += "{\"s\": ";
            json_string(out, n.scalar);
            out += n.quoted ? ", \"q\": true}" : ", \"q\": false}";
            break;
        case Node::List:
            out += "{\"list\": [";
            for (size_t i = 0; i < n.list.size(); ++i) {
                if (i) out += ", ";
                json_node(out, n.list[i]);
            }
            out += "]}";
            break;
        case Node::Map:
            out += "{\"map\": [";
            for (size_t i = 0; i < n.map.size(); ++i) {
                if (i) out += ", ";
                out += '[';
                json_string(out, n.map[i].first);
                out += ", ";
                json_node(out, n.map[i].second);
                out += ']';
            }
            out += "]}";
            break;
    }
}
}  // namespace

struct rbrt_host_scene {
    rbrt::Camera cam;
    rbrt::Scene scene;
    rbrt::Scene::AbiView view;
    rbrt_camera_t cam_abi;
    rbrt_camera_lens_t lens_abi;
    bool shutter = false;
    float travel[3] = {0.0f, 0.0f, 0.0f};
    std::vector<float> motion;  // Scene::motion_travels
    std::vector<float> mesh_motion;  // Scene::mesh_motion_travels
};

extern "C" {

const char* rbrt_host_last_error(void) { return g_err.c_str(); }

// src/main.rs:70-80: YAML -> blueprints -> Camera::new(.., height, width, ..) + scene. 0 on success.
int rbrt_host_scene_load(const char* yaml_path, uint32_t height, uint32_t width, rbrt_host_scene** out) {
    try {
        rbrt::SceneBlueprint bp = rbrt::load_blueprints_from_yaml_file(yaml_path);
        auto* h = new rbrt_host_scene();
        h->cam = rbrt::camera_from_blueprint(bp.camera_blueprint, height, width);
        h->scene = rbrt::create_scene_from_scene_blueprint(bp);
        if (bp.environment_blueprint) h->scene.environment = rbrt::load_environment(*bp.environment_blueprint);
        h->view = h->scene.to_abi();
        h->cam_abi = h->cam.to_abi();
        h->lens_abi = h->cam.to_abi_lens();
        if (const auto& tr = bp.camera_blueprint.camera_shutter_travel) h->shutter = true, h->travel[0] = tr->x, h->travel[1] = tr->y, h->travel[2] = tr->z;
        h->motion = h->scene.motion_travels();
        h->mesh_motion = h->scene.mesh_motion_travels();
        *out = h;
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
const rbrt_camera_t* rbrt_host_scene_camera(const rbrt_host_scene* h) { return &h->cam_abi; }
// The camera with its thin lens (camera_aperture_mm > 0), or NULL for a pinhole camera.
const rbrt_camera_lens_t* rbrt_host_scene_lens(const rbrt_host_scene* h) { return h->cam.thin_lens ? &h->lens_abi : nullptr; }
// The scene's camera_shutter_travel (three floats, what rbrt_shutter_t::travel takes), or NULL when it has none.
const float* rbrt_host_scene_shutter_travel(const rbrt_host_scene* h) { return h->shutter ? h->travel : nullptr; }
// The spheres' shutter_travel keys as rbrt_motion_t::travel takes them, [n_spheres][3] with zeros for the spheres without one, or
// NULL when no sphere has the key (no motion).
const float* rbrt_host_scene_motion(const rbrt_host_scene* h) { return h->motion.empty() ? nullptr : h->motion.data(); }
// The meshes' shutter_travel keys as rbrt_mesh_motion_t::travel takes them, [n_meshes][3] with zeros for the meshes without one,
// or NULL when no mesh has the key (no mesh motion).
const float* rbrt_host_scene_mesh_motion(const rbrt_host_scene* h) { return h->mesh_motion.empty() ? nullptr : h->mesh_motion.data(); }
const rbrt_scene_t* rbrt_host_scene_scene(const rbrt_host_scene* h) { return &h->view.scene; }
// The corner normals of the smooth meshes (YAML `shading: smooth`), or NULL when every mesh is flat.
const rbrt_scene_shading_t* rbrt_host_scene_shading(const rbrt_host_scene* h) { return h->view.shading_ptr(); }
// The solid patterns of the scene's objects (YAML `checker_albedo` / `checker_size`), or NULL when no object carries one.
const rbrt_scene_patterns_t* rbrt_host_scene_patterns(const rbrt_host_scene* h) { return h->view.patterns_ptr(); }
// The nodes made of the scene's environment_blueprint: float[*n + 1][*n + 1][3], what rbrt_environment_t::nodes takes; NULL
// (and *n = 0) when the scene has none. Valid until rbrt_host_scene_free.
const float* rbrt_host_scene_environment(const rbrt_host_scene* h, uint32_t* n) {
    if (n) *n = h->scene.environment.n;
    return h->scene.environment.n ? h->scene.environment.nodes.data() : nullptr;
}
void rbrt_host_scene_free(rbrt_host_scene* h) { delete h; }

// TEST HOOKS (tests/test_environment_host.py). The PFM reader: the image's size and, when `rgb` is not NULL, its
// width * height * 3 floats, top row first (call once for the size, once for the texels).
int rbrt_host_read_pfm(const char* path, uint32_t* width, uint32_t* height, float* rgb) {
    try {
        const rbrt::PfmImage img = rbrt::read_pfm(path);
        *width = img.width, *height = img.height;
        if (rgb) std::memcpy(rgb, img.rgb.data(), img.rgb.size() * sizeof(float));
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
// TEST HOOKS (tests/test_tonemap_host.py). The PFM writer of --radiance, and the reader with any_value: what the writer wrote
// comes back bit for bit, NaN and negative texels included.
int rbrt_host_write_pfm(const char* path, const float* rgb, uint32_t width, uint32_t height) {
    try {
        rbrt::write_pfm(path, rgb, width, height);
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
int rbrt_host_read_pfm_any(const char* path, uint32_t* width, uint32_t* height, float* rgb) {
    try {
        const rbrt::PfmImage img = rbrt::read_pfm(path, true);
        *width = img.width, *height = img.height;
        if (rgb) std::memcpy(rgb, img.rgb.data(), img.rgb.size() * sizeof(float));
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
// The conversion alone: a latitude/longitude image (top row first) -> nodes_out float[n + 1][n + 1][3].
int rbrt_host_environment_nodes(const float* rgb, uint32_t width, uint32_t height, uint32_t n, double rotation_deg, double intensity,
                                float* nodes_out) {
    try {
        rbrt::PfmImage img;
        img.width = width, img.height = height;
        img.rgb.assign(rgb, rgb + size_t(width) * height * 3);
        const std::vector<float> nodes = rbrt::environment_nodes_from_latlong(img, n, rotation_deg, intensity);
        std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(float));
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
// What the environment adds to a checkpoint's fingerprint `h` (n == 0 or nodes NULL: none).
uint64_t rbrt_host_environment_fingerprint(const float* nodes, uint32_t n, uint64_t h) {
    rbrt::Environment e;
    if (nodes && n) e.n = n, e.nodes.assign(nodes, nodes + size_t(n + 1) * (n + 1) * 3);
    return rbrt::environment_fingerprint(e, h);
}

// What a shutter adds to a checkpoint's fingerprint `h` (travel NULL: none, h itself).
uint64_t rbrt_host_shutter_fingerprint(const float* travel, uint64_t h) { return rbrt::shutter_fingerprint(travel, h); }
// What a motion adds to it (travels NULL: none, h itself).
uint64_t rbrt_host_motion_fingerprint(const float* travels, uint32_t n_spheres, uint64_t h) { return rbrt::motion_fingerprint(travels, n_spheres, h); }

// What a mesh motion adds to it (travels NULL: none, h itself).
uint64_t rbrt_host_mesh_motion_fingerprint(const float* travels, uint32_t n_meshes, uint64_t h) { return rbrt::mesh_motion_fingerprint(travels, n_meshes, h); }

int rbrt_host_write_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height) {
    try {
        rbrt::write_png(path, rgb, width, height);
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

// ImageBuffer::save (src/main.rs:86): the encoder is picked from the extension.
int rbrt_host_save_image(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height) {
    try {
        rbrt::ImageBuffer img;
        img.width = width, img.height = height;
        img.rgb.assign(rgb, rgb + size_t(width) * height * 3);
        img.save(path);
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

// TEST HOOK ONLY (tests/test_yaml_differential.py): the tree yaml_lite::parse builds from `text`, as JSON in a string the
// caller releases with rbrt_host_free. null: a null node; {"s": text, "q": quoted}: a scalar; {"list": [..]}: a sequence;
// {"map": [[key, value], ..]}: a mapping as pairs in file order. Nonzero when the reader refuses the text; the message is in
// rbrt_host_last_error.
int rbrt_host_yaml_dump(const char* text, size_t len, char** json_out) {
    try {
        const yaml_lite::Node root = yaml_lite::parse(std::string(text, len));
        std::string out;
        json_node(out, root);
        char* p = static_cast<char*>(std::malloc(out.size() + 1));
        if (!p) throw std::runtime_error("out of memory");
        std::memcpy(p, out.c_str(), out.size() + 1);
        *json_out = p;
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
void rbrt_host_free(void* p) { std::free(p); }

// Camera::new alone (cam.rs:22-62), for parity tests against the oracle's restatement.
void rbrt_host_camera_new(const float position[3], const float look_at[3], const float up[3], uint32_t height,
                          uint32_t width, float focal_len_mm, rbrt_camera_t* out) {
    rbrt::Camera c = rbrt::Camera::create(rbrt::Vec3(position[0], position[1], position[2]),
                                          rbrt::Vec3(look_at[0], look_at[1], look_at[2]),
                                          rbrt::Vec3(up[0], up[1], up[2]), height, width, focal_len_mm);
    *out = c.to_abi();
}

}  // extern "C"
