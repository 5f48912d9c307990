// checkpoint.cpp — fingerprint, reader and writer of a render's checkpoint file (checkpoint.hpp). No GPU code: the CPU
// self-test (tests/cpp/host_selftest.cpp) runs all of it under the sanitizers.
#include "checkpoint.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>

namespace rbrt {
namespace {

uint64_t fnv1a(const void* p, size_t n, uint64_t h) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

uint64_t scene_fingerprint(const rbrt_camera_t& cam, const rbrt_scene_t& sc) {
    uint64_t h = 0xCBF29CE484222325ull;
    h = fnv1a(&cam, sizeof(cam), h);
    for (uint32_t i = 0; i < sc.n_spheres; ++i) h = fnv1a(&sc.spheres[i], sizeof(rbrt_sphere_t), h);
    for (uint32_t i = 0; i < sc.n_meshes; ++i) {
        const rbrt_mesh_t& m = sc.meshes[i];
        h = fnv1a(&m.n_total, sizeof(m.n_total), h);
        h = fnv1a(&m.mat, sizeof(m.mat), h);
        const float* arrs[12] = {m.v0x, m.v0y, m.v0z, m.e1x, m.e1y, m.e1z, m.e2x, m.e2y, m.e2z, m.nx, m.ny, m.nz};
        for (const float* a : arrs) h = fnv1a(a, size_t(m.n_total) * sizeof(float), h);
        h = fnv1a(m.is_padding, m.n_total, h);
    }
    return h;
}

// ... and the corner normals of smooth meshes, only when there are any (a flat scene's checkpoints keep their fingerprint).
uint64_t shading_fingerprint(const rbrt_scene_t& sc, const rbrt_scene_shading_t* sh, uint64_t h) {
    if (!sh || !sh->meshes) return h;
    for (uint32_t i = 0; i < sh->n_meshes; ++i) {
        const rbrt_mesh_normals_t& mn = sh->meshes[i];
        const uint32_t smooth = mn.n0x != nullptr;
        h = fnv1a(&smooth, sizeof(smooth), h);
        if (!smooth) continue;
        const float* arrs[9] = {mn.n0x, mn.n0y, mn.n0z, mn.n1x, mn.n1y, mn.n1z, mn.n2x, mn.n2y, mn.n2z};
        for (const float* a : arrs) h = fnv1a(a, size_t(sc.meshes[i].n_total) * sizeof(float), h);
    }
    return h;
}

// ... and the solid patterns, only when there are any (an unpatterned scene's checkpoints keep their fingerprint).
uint64_t patterns_fingerprint(const rbrt_scene_patterns_t* pt, uint64_t h) {
    if (!pt || !pt->objects) return h;
    bool any = false;
    for (uint32_t i = 0; i < pt->n_objects; ++i) any = any || pt->objects[i].kind != RBRT_PATTERN_NONE;
    if (!any) return h;
    for (uint32_t i = 0; i < pt->n_objects; ++i) {
        const rbrt_pattern_t& p = pt->objects[i];
        h = fnv1a(&p.kind, sizeof(p.kind), h);
        if (p.kind == RBRT_PATTERN_NONE) continue;
        h = fnv1a(p.albedo2, sizeof(p.albedo2), h);
        h = fnv1a(p.origin, sizeof(p.origin), h);
        h = fnv1a(&p.size, sizeof(p.size), h);
    }
    return h;
}

}  // namespace

uint64_t checkpoint_fingerprint(const std::string& path, const rbrt_camera_lens_t& lens, const rbrt_render_opts_t& opts, const rbrt_scene_t& sc,
                                const rbrt_scene_shading_t* sh, const Environment& env, const rbrt_scene_patterns_t* pt, const float* travel,
                                const std::vector<float>* motion, float motion_step, const std::vector<float>* mesh_motion) {
    if (path.empty()) return 0;
    uint64_t h = patterns_fingerprint(pt, shading_fingerprint(sc, sh, scene_fingerprint(lens.cam, sc)));
    if (opts.flags & RBRT_FLAG_CONSTANT_BACKGROUND) {
        const uint32_t flags = opts.flags & ~RBRT_FLAG_THIN_LENS;  // (the word as it was hashed before there was a lens bit)
        h = fnv1a(&flags, sizeof(flags), h);
        h = fnv1a(opts.bg, sizeof(opts.bg), h);
    }
    h = environment_fingerprint(env, h);
    if (opts.flags & RBRT_FLAG_THIN_LENS) {
        const uint32_t bit = RBRT_FLAG_THIN_LENS;
        h = fnv1a(&bit, sizeof(bit), h);
        h = fnv1a(lens.lens_u, sizeof(lens.lens_u), h);
        h = fnv1a(lens.lens_v, sizeof(lens.lens_v), h);
        h = fnv1a(&lens.focus_scale, sizeof(lens.focus_scale), h);
    }
    h = shutter_fingerprint(travel, h);
    const bool spheres_move = motion && !motion->empty(), meshes_move = mesh_motion && !mesh_motion->empty();
    if (!spheres_move && !meshes_move) return h;
    if (spheres_move) h = motion_fingerprint(motion->data(), uint32_t(motion->size() / 3u), h);
    if (meshes_move) h = mesh_motion_fingerprint(mesh_motion->data(), uint32_t(mesh_motion->size() / 3u), h);
    if (motion_step != 0.0f) {  // (the spheres and meshes advance between frames: other sums)
        const char tag[8] = {'m', 's', 't', 'e', 'p', 0, 0, 0};
        h = fnv1a(&motion_step, sizeof(motion_step), fnv1a(tag, sizeof(tag), h));
    }
    return h;
}

uint64_t motion_fingerprint(const float* travels, uint32_t n_spheres, uint64_t h) {
    if (!travels) return h;
    const char tag[8] = {'m', 'o', 't', 'i', 'o', 'n', 0, 0};
    h = fnv1a(tag, sizeof(tag), h);
    h = fnv1a(&n_spheres, sizeof(n_spheres), h);
    return fnv1a(travels, size_t(n_spheres) * 3u * sizeof(float), h);
}

uint64_t mesh_motion_fingerprint(const float* travels, uint32_t n_meshes, uint64_t h) {
    if (!travels) return h;
    const char tag[8] = {'m', 'e', 's', 'h', 'm', 'o', 't', 0};
    h = fnv1a(tag, sizeof(tag), h);
    h = fnv1a(&n_meshes, sizeof(n_meshes), h);
    return fnv1a(travels, size_t(n_meshes) * 3u * sizeof(float), h);
}

uint64_t shutter_fingerprint(const float* travel, uint64_t h) {
    if (!travel) return h;
    const char tag[8] = {'s', 'h', 'u', 't', 't', 'e', 'r', 0};
    h = fnv1a(tag, sizeof(tag), h);
    return fnv1a(travel, 3 * sizeof(float), h);
}

CheckpointHeader checkpoint_header(uint32_t width, uint32_t height, uint32_t spp, uint32_t world, uint64_t seed, uint64_t fingerprint) {
    CheckpointHeader h{};
    std::memcpy(h.magic, "RBRTCKP1", 8);
    h.width = width, h.height = height, h.spp = spp, h.world = world;
    h.seed = seed, h.fingerprint = fingerprint;
    return h;
}

CheckpointRead read_checkpoint(const std::string& path, const CheckpointHeader& want, const std::vector<size_t>& counts) {
    CheckpointRead res;
    std::ifstream in(path, std::ios::binary);
    CheckpointHeader h{};
    if (!in || !in.read(reinterpret_cast<char*>(&h), sizeof(h))) return res;
    res.found = true;
    bool ok = !std::memcmp(h.magic, want.magic, 8) && h.width == want.width && h.height == want.height && h.spp == want.spp &&
              h.world == want.world && h.seed == want.seed && h.fingerprint == want.fingerprint && h.samples_done > 0 &&
              h.samples_done < want.spp && counts.size() == want.world;
    res.sums.resize(counts.size());
    for (size_t r = 0; ok && r < counts.size(); ++r) {
        uint64_t cnt = 0;
        ok = bool(in.read(reinterpret_cast<char*>(&cnt), sizeof(cnt))) && cnt == counts[r];  // (checked before anything is sized by it)
        if (ok) {
            res.sums[r].resize(counts[r]);
            ok = bool(in.read(reinterpret_cast<char*>(res.sums[r].data()), std::streamsize(counts[r] * sizeof(float))));
        }
    }
    if (ok) res.samples_done = h.samples_done;
    else for (auto& v : res.sums) v.clear();
    return res;
}

bool write_checkpoint(const std::string& path, const CheckpointHeader& want, uint32_t samples_done, const std::vector<std::vector<float>>& sums) {
    const std::string tmp = path + ".tmp";
    std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
    CheckpointHeader h = want;
    h.samples_done = samples_done;
    out.write(reinterpret_cast<const char*>(&h), sizeof(h));
    for (const std::vector<float>& s : sums) {
        const uint64_t cnt = s.size();
        out.write(reinterpret_cast<const char*>(&cnt), sizeof(cnt));
        out.write(reinterpret_cast<const char*>(s.data()), std::streamsize(cnt * sizeof(float)));
    }
    out.close();
    return out && std::rename(tmp.c_str(), path.c_str()) == 0;
}

}  // namespace rbrt
