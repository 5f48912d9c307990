// checkpoint.hpp — the checkpoint of a render in passes (internal to the host: render.cpp uses it, tests/cpp checks it).
// A file is the header below, then for every rank a uint64 count and that many floats: the rank's running sums. Nothing
// here needs a GPU or the HIP library.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rbrt.hpp"

namespace rbrt {

struct CheckpointHeader {
    char magic[8];  // "RBRTCKP1"
    uint32_t width, height, spp, world;
    uint64_t seed, fingerprint;
    uint32_t samples_done, reserved;
};

// The header a checkpoint of this render must carry to be resumed (samples_done left at 0).
CheckpointHeader checkpoint_header(uint32_t width, uint32_t height, uint32_t spp, uint32_t world, uint64_t seed, uint64_t fingerprint);

// FNV-1a of everything the running sums depend on besides the header's own fields: camera, spheres, mesh arrays; then, each
// only where the render has it (so that a render without it keeps the fingerprint its checkpoints were written with), the
// corner normals of smooth meshes, the solid patterns (pt), the constant background (opts.flags, opts.bg), the environment, the thin lens
// (opts.flags says whether `lens` has one), the shutter (`travel`: null without one), the motion (`motion`: null or empty
// without one) and, with a motion, a motion_step other than 0 (RenderConfig::motion_step). 0 for an empty path: there is no
// checkpoint to match.
uint64_t checkpoint_fingerprint(const std::string& path, const rbrt_camera_lens_t& lens, const rbrt_render_opts_t& opts, const rbrt_scene_t& sc,
                                const rbrt_scene_shading_t* sh, const Environment& env, const rbrt_scene_patterns_t* pt = nullptr,
                                const float* travel = nullptr, const std::vector<float>* motion = nullptr, float motion_step = 0.0f,
                                const std::vector<float>* mesh_motion = nullptr);
// The shutter's part of it: h itself without a shutter (travel null), else h continued over a tag and the three floats -- a
// zero travel included, whose draw makes its sums another render's.
uint64_t shutter_fingerprint(const float* travel, uint64_t h);
// The motion's part of it (Scene::motion_travels; `motion` null or empty: none, h itself): h continued over a tag, the number of
// spheres and their travels -- an all-zero motion included, whose draw makes its sums another render's.
uint64_t motion_fingerprint(const float* travels, uint32_t n_spheres, uint64_t h);
// The mesh motion's part of it (Scene::mesh_motion_travels; null: none, h itself): h continued over a tag, the number of meshes
// and their travels. Only a scene one of whose meshes has the key comes here, so every other fingerprint keeps its bytes.
uint64_t mesh_motion_fingerprint(const float* travels, uint32_t n_meshes, uint64_t h);

struct CheckpointRead {
    bool found = false;         // the file is there and as long as a header
    uint32_t samples_done = 0;  // 0: start over; else resume at this sample, with ...
    std::vector<std::vector<float>> sums;  // ... [rank] the running sums (empty vectors when starting over)
};
// `want`: checkpoint_header of this render; counts[rank]: the floats that rank's sums must have. Anything that differs, a
// samples_done outside (0, spp) or a file that ends early means "start over"; no more than counts[rank] floats are ever read.
CheckpointRead read_checkpoint(const std::string& path, const CheckpointHeader& want, const std::vector<size_t>& counts);

// Header with samples_done, then every rank's count and sums, to path + ".tmp", renamed over `path`. False when that failed.
bool write_checkpoint(const std::string& path, const CheckpointHeader& want, uint32_t samples_done, const std::vector<std::vector<float>>& sums);

}  // namespace rbrt
