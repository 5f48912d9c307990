// cli.hpp — the `rbrt` command line behind main(): the options, their parser, the combination checks, what they make of a scene
// blueprint and a RenderConfig, the files a run leaves and its --report. No GPU call; main.cpp has usage() and the order of it all.
#pragma once
#include <chrono>
#include <optional>
#include <string>

#include "rbrt.hpp"

// One member per option, with the option's default; an optional where the checks or the config ask "given or not".
struct CliOptions {
    std::string target = "dbg_out.png", config = "scenes/example_scene.yaml";
    uint32_t height = 600, width = 800, samples = 5, gpus = 1, pass_samples = 0, checkpoint_every = 1;
    std::string gather = "host", checkpoint, report_path;
    unsigned long long seed = 1;
    bool oversubscribe = false, constant_background = false;
    float background[3] = {0.0f, 0.0f, 0.0f};
    std::optional<float> aperture, focus_distance;
    std::optional<bool> smooth;
    std::optional<float> adaptive;
    // (the step: every round ends in a drain and a read-back, 1.0 ms at 1024x768 whatever the round renders; with rounds of
    // 16 a 256-spp render that traces a tenth of the samples took as long as the fixed one, with rounds of 64 half as long
    // for 1 % more samples: profiles/adaptive_config2.txt)
    uint32_t min_samples = 16, adaptive_step = 64;
    std::string sample_map;
    bool denoise = false;
    std::optional<uint32_t> denoise_radius, denoise_patch;
    std::optional<float> denoise_strength;
    std::string noisy;
    bool denoise_guided = false, guided_no_demodulation = false;
    std::optional<uint32_t> guided_levels;
    std::optional<float> guided_colour, guided_normal, guided_depth, guided_albedo;
    std::optional<std::string> environment;  // a file, or "none"
    std::optional<float> environment_rotation, environment_intensity;
    std::optional<uint32_t> environment_resolution;
    float exposure = 1.0f, exposure_key = 0.18f;  // the multiplier (0: automatic) and the key
    uint32_t tone_curve = RBRT_TONE_LINEAR;
    std::optional<float> white;  // given: the white point (0: automatic)
    std::string radiance_file;
    std::optional<float> glare, glare_threshold, glare_spread;  // --glare turns the stage on; the others need it
    std::optional<uint32_t> glare_levels;
    std::optional<std::string> features;  // the prefix of the four files
    std::optional<uint32_t> feature_samples;
    std::optional<uint32_t> frames;  // --frames turns temporal accumulation on; the options below need it
    std::optional<float> temporal_max_history, temporal_depth, temporal_normal;
    float camera_step[3] = {0.0f, 0.0f, 0.0f};
    bool camera_step_given = false;
    std::optional<float> shutter;  // --shutter S: the travel is S * camera_step
    float shutter_travel[3] = {0.0f, 0.0f, 0.0f};
    bool shutter_travel_given = false;
    bool no_motion = false;  // --no-motion: the spheres' shutter_travel keys are ignored
    std::optional<float> motion_step;  // --motion-step P: the moving spheres advance P exposures a frame (needs --frames)
    std::string history_map;
    std::optional<uint32_t> upscale;  // --upscale turns guided upsampling on; the options below need it
    std::optional<float> upscale_normal, upscale_depth, upscale_albedo;
    bool despike = false;  // --despike turns spike removal on; the options below need it
    std::optional<float> despike_threshold;
    std::optional<uint32_t> despike_rank, despike_radius;
    std::string spike_map;
    std::string compare_file, error_map, ssim_map;  // --compare turns the comparison on; the maps and the epsilon need it
    std::optional<float> compare_epsilon;

    // (0 EV and no curve is the identity: such a run makes no tonemap call at all and writes what it always wrote)
    bool transformed() const { return exposure != 1.0f || tone_curve != RBRT_TONE_LINEAR; }
    // every stage that renders through one round of the adaptive path on one handle
    bool adaptive_path() const { return adaptive || denoise || denoise_guided || frames || upscale || despike; }
};

// What parse_cli and check_cli answer where they do not answer with the process's exit code (0 or 2).
enum : int { CLI_RUN = -1, CLI_HELP = -2 };

// The arguments into o, the first refusal in argv's order on stderr. CLI_HELP: main prints usage() and exits with 0.
int parse_cli(int argc, char** argv, CliOptions& o);
// The options against each other, in a fixed order, before anything is loaded; reads --compare's reference.
int check_cli(const CliOptions& o, rbrt::PfmImage& compare_ref);

void apply_overrides(rbrt::SceneBlueprint& bp, const CliOptions& o);  // throws what the scene file and the options cannot be together
rbrt::RenderConfig config_of(const CliOptions& o, const rbrt::SceneBlueprint& bp);
void save_outputs(const CliOptions& o, const rbrt::ImageBuffer& img, const rbrt::ImageComparison& cmp);

// parse_s (t0..t1), the scene's preparation (t1..t2), encode_s (t3..t4) and total_s (t0..t4) of the report
using CliClock = std::chrono::steady_clock;
struct CliTimes {
    CliClock::time_point t0, t1, t2, t3, t4;
};
void write_report(const CliOptions& o, const rbrt::RenderConfig& cfg, const rbrt::RenderReport& rep, const rbrt::Scene& scene,
                  const rbrt::ImageComparison& cmp, const CliTimes& t);
