// cli.cpp — the `rbrt` command line's options: parser, combination checks, scene overrides, RenderConfig and output files.
#include "cli.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

namespace {

bool parse_u32(const char* s, uint32_t& out) {
    char* end = nullptr;
    unsigned long v = std::strtoul(s, &end, 10);
    if (end == s || *end != '\0' || v > 0xFFFFFFFFul || s[0] == '-') return false;
    out = uint32_t(v);
    return true;
}

bool parse_f32(const char* s, float& out) {
    char* end = nullptr;
    const float v = std::strtof(s, &end);
    if (end == s || *end != '\0') return false;
    out = v;
    return true;
}

// "X,Y,Z": three finite floats, non_negative: none of them below 0
bool parse_triple(const char* s, float out[3], bool non_negative) {
    const char* p = s;
    for (int c = 0; c < 3; ++c) {
        char* end = nullptr;
        const float v = std::strtof(p, &end);
        if (end == p || !std::isfinite(v) || (non_negative && v < 0.0f)) return false;
        out[c] = v;
        if (c < 2) {
            if (*end != ',') return false;
            p = end + 1;
        } else if (*end != '\0') {
            return false;
        }
    }
    return true;
}

bool ends_in_pfm(const std::string& path) { return path.size() >= 4 && path.compare(path.size() - 4, 4, ".pfm") == 0; }

// what a float option admits
bool any_number(float) { return true; }
bool finite(float f) { return std::isfinite(f); }
bool at_least_0(float f) { return std::isfinite(f) && f >= 0.0f; }
bool above_0(float f) { return std::isfinite(f) && f > 0.0f; }
bool at_least_1(float f) { return std::isfinite(f) && f >= 1.0f; }
bool share(float f) { return above_0(f) && f <= 1.0f; }
bool stops(float ev) { return std::isfinite(ev) && above_0(float(std::exp2(double(ev)))); }

// The argument under the cursor, "--name=value" split, and one typed reader per kind of option. A reader takes the value (the
// next argument, whatever it starts with, unless "=value" gave one), says on stderr why it refuses it and answers false then.
struct Cursor {
    const int argc;
    char** const argv;
    int i = 0;
    std::string name, val;
    bool has_val = false;

    Cursor(int argc, char** argv) : argc(argc), argv(argv) {}
    bool next() {
        if (++i >= argc) return false;
        name = argv[i], val.clear(), has_val = false;
        const size_t eq = name.find('=');
        if (name.rfind("--", 0) == 0 && eq != std::string::npos) val = name.substr(eq + 1), name = name.substr(0, eq), has_val = true;
        return true;
    }
    bool is(const char* long_name, const char* short_name = nullptr) const { return name == long_name || (short_name && name == short_name); }
    const char* value() {
        if (has_val) return val.c_str();
        if (i + 1 < argc) return argv[++i];
        std::fprintf(stderr, "error: a value is required for '%s' but none was supplied\n", name.c_str());
        return nullptr;
    }
    bool invalid(const char* v, const char* expected) const {
        std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected %s)\n", v, name.c_str(), expected);
        return false;
    }
    bool text(std::string& dst, const char* expected_if_not_empty = nullptr) {
        const char* v = value();
        if (!v) return false;
        dst = v;
        return !(expected_if_not_empty && dst.empty()) || invalid("", expected_if_not_empty);
    }
    bool text(std::optional<std::string>& dst, const char* expected_if_not_empty) { return text(dst.emplace(), expected_if_not_empty); }
    bool word(std::string& dst, std::initializer_list<const char*> words) {
        if (!text(dst)) return false;
        std::string all;
        for (const char* w : words) {
            if (dst == w) return true;
            all += (all.empty() ? "" : ", ") + std::string(w);
        }
        std::fprintf(stderr, "error: invalid value '%s' for '%s' [possible values: %s]\n", dst.c_str(), name.c_str(), all.c_str());
        return false;
    }
    bool u32(uint32_t& dst) {
        const char* v = value();
        if (!v) return false;
        if (parse_u32(v, dst)) return true;
        std::fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, name.c_str());
        return false;
    }
    bool u32(std::optional<uint32_t>& dst, uint32_t least, uint32_t most = UINT32_MAX) {  // (no `most`: "at least")
        uint32_t v = 0;
        if (!u32(v)) return false;
        const std::string given = std::to_string(v), range = std::to_string(least) + " to " + std::to_string(most);
        if (v < least || v > most) return invalid(given.c_str(), most == UINT32_MAX ? ("at least " + std::to_string(least)).c_str() : range.c_str());
        dst = v;
        return true;
    }
    bool f32(float& dst, bool (*admits)(float), const char* expected, const char* or_word = nullptr, float word_value = 0.0f) {
        const char* v = value();
        if (!v) return false;
        float f = 0.0f;
        if (or_word && std::string(v) == or_word) f = word_value;
        else if (!parse_f32(v, f) || !admits(f)) return invalid(v, expected);
        dst = f;
        return true;
    }
    bool f32(std::optional<float>& dst, bool (*admits)(float), const char* expected, const char* or_word = nullptr) {
        float f = 0.0f;
        if (!f32(f, admits, expected, or_word)) return false;
        dst = f;
        return true;
    }
    bool f32_unsigned_zero(std::optional<float>& dst, bool (*admits)(float), const char* expected) {  // "-0" is stored as 0
        if (!f32(dst, admits, expected)) return false;
        dst = *dst + 0.0f;
        return true;
    }
    bool triple(float dst[3], bool& given, bool non_negative, const char* expected) {
        const char* v = value();
        if (!v) return false;
        if (!parse_triple(v, dst, non_negative)) return invalid(v, expected);
        return given = true;
    }
    bool flag(bool& dst, bool takes_no_value = true) {  // (--oversubscribe and --despike let "=value" pass: DESIGN.md)
        if (has_val && takes_no_value) {
            std::fprintf(stderr, "error: '%s' takes no value\n", name.c_str());
            return false;
        }
        return dst = true;
    }
};

}  // namespace

int parse_cli(int argc, char** argv, CliOptions& o) {
    const char *const number = "a finite number", *const positive = "a finite number > 0", *const unsigned_number = "a finite number >= 0";
    const char *const step = "DX,DY,DZ: three finite numbers";
    std::string w;
    float ev = 0.0f;
    bool ok = true;
    for (Cursor a(argc, argv); ok && a.next();) {
        if (a.is("--help", "-h")) return CLI_HELP;
        else if (a.is("--version", "-V")) return std::printf("rbrt 0.1\n"), 0;
        else if (a.is("--target_file", "-t")) ok = a.text(o.target);
        else if (a.is("--height")) ok = a.u32(o.height);
        else if (a.is("--width", "-w")) ok = a.u32(o.width);
        else if (a.is("--config", "-c")) ok = a.text(o.config);
        else if (a.is("--samples", "-s")) ok = a.u32(o.samples);
        else if (a.is("--gpus")) ok = a.u32(o.gpus);
        else if (a.is("--pass-samples")) ok = a.u32(o.pass_samples);
        else if (a.is("--checkpoint-every")) ok = a.u32(o.checkpoint_every);
        else if (a.is("--checkpoint")) ok = a.text(o.checkpoint);
        else if (a.is("--gather")) ok = a.word(o.gather, {"rccl", "host"});
        else if (a.is("--oversubscribe")) ok = a.flag(o.oversubscribe, false);
        else if (a.is("--report")) ok = a.text(o.report_path);
        else if (a.is("--background")) ok = a.triple(o.background, o.constant_background, true, "R,G,B: three non-negative numbers");
        else if (a.is("--aperture")) ok = a.f32(o.aperture, any_number, "a number");
        else if (a.is("--focus-distance")) ok = a.f32(o.focus_distance, any_number, "a number");
        else if (a.is("--adaptive")) ok = a.f32(o.adaptive, at_least_0, "a finite threshold >= 0");
        else if (a.is("--min-samples")) ok = a.u32(o.min_samples);
        else if (a.is("--adaptive-step")) ok = a.u32(o.adaptive_step);
        else if (a.is("--sample-map")) ok = a.text(o.sample_map);
        else if (a.is("--denoise")) ok = a.flag(o.denoise);
        else if (a.is("--denoise-radius")) ok = a.u32(o.denoise_radius, 0, 10);
        else if (a.is("--denoise-patch")) ok = a.u32(o.denoise_patch, 0, 4);
        else if (a.is("--denoise-strength")) ok = a.f32(o.denoise_strength, above_0, positive);
        else if (a.is("--noisy")) ok = a.text(o.noisy);
        else if (a.is("--denoise-guided")) ok = a.flag(o.denoise_guided);
        else if (a.is("--guided-no-demodulation")) ok = a.flag(o.guided_no_demodulation);
        else if (a.is("--guided-levels")) ok = a.u32(o.guided_levels, 1, RBRT_GUIDED_MAX_LEVELS);
        else if (a.is("--guided-colour")) ok = a.f32(o.guided_colour, above_0, positive);
        else if (a.is("--guided-normal")) ok = a.f32(o.guided_normal, above_0, positive);
        else if (a.is("--guided-depth")) ok = a.f32(o.guided_depth, above_0, positive);
        else if (a.is("--guided-albedo")) ok = a.f32(o.guided_albedo, above_0, positive);
        else if (a.is("--environment")) ok = a.text(o.environment, "a PFM file or `none`");
        else if (a.is("--environment-rotation")) ok = a.f32(o.environment_rotation, finite, number);
        else if (a.is("--environment-intensity")) ok = a.f32(o.environment_intensity, at_least_0, unsigned_number);
        else if (a.is("--environment-resolution")) ok = a.u32(o.environment_resolution, 1, 4096);
        else if (a.is("--exposure")) {  // stops, or 0 as the multiplier: automatic
            if ((ok = a.f32(ev, stops, "a number of stops whose 2^EV is a finite float above 0, or auto", "auto", NAN)))
                o.exposure = std::isnan(ev) ? 0.0f : float(std::exp2(double(ev)));
        } else if (a.is("--exposure-key")) ok = a.f32(o.exposure_key, above_0, positive);
        else if (a.is("--tonemap")) {
            if ((ok = a.word(w, {"none", "reinhard", "aces"}))) o.tone_curve = w == "none" ? RBRT_TONE_LINEAR : w == "reinhard" ? RBRT_TONE_REINHARD : RBRT_TONE_ACES;
        } else if (a.is("--white")) ok = a.f32(o.white, above_0, "a finite number > 0, or auto", "auto");
        else if (a.is("--glare")) ok = a.f32(o.glare, share, "a number above 0 and at most 1");
        else if (a.is("--glare-threshold")) ok = a.f32_unsigned_zero(o.glare_threshold, at_least_0, unsigned_number);
        else if (a.is("--glare-spread")) ok = a.f32_unsigned_zero(o.glare_spread, at_least_0, unsigned_number);
        else if (a.is("--glare-levels")) ok = a.u32(o.glare_levels, 1, RBRT_GLARE_MAX_LEVELS);
        else if (a.is("--radiance")) ok = a.text(o.radiance_file);
        else if (a.is("--features")) ok = a.text(o.features, "the prefix of the four files it writes");
        else if (a.is("--feature-samples")) ok = a.u32(o.feature_samples, 1, 65536);
        else if (a.is("--frames")) ok = a.u32(o.frames, 1);
        else if (a.is("--camera-step")) ok = a.triple(o.camera_step, o.camera_step_given, false, step);
        else if (a.is("--shutter-travel")) ok = a.triple(o.shutter_travel, o.shutter_travel_given, false, step);
        else if (a.is("--no-motion")) ok = a.flag(o.no_motion);
        else if (a.is("--motion-step")) ok = a.f32(o.motion_step, finite, "a finite number: the exposures the moving spheres advance from one frame to the next");
        else if (a.is("--shutter"))
            ok = a.f32_unsigned_zero(o.shutter, at_least_0, "a finite number >= 0: the part of a frame's camera step the shutter is open for");
        else if (a.is("--temporal-max-history")) ok = a.f32_unsigned_zero(o.temporal_max_history, at_least_1, "a finite number >= 1");
        else if (a.is("--temporal-depth")) ok = a.f32_unsigned_zero(o.temporal_depth, at_least_0, unsigned_number);
        else if (a.is("--temporal-normal")) ok = a.f32_unsigned_zero(o.temporal_normal, at_least_0, unsigned_number);
        else if (a.is("--history-map")) ok = a.text(o.history_map);
        else if (a.is("--upscale")) ok = a.u32(o.upscale, 2, RBRT_UPSAMPLE_MAX_FACTOR);
        else if (a.is("--upscale-normal")) ok = a.f32(o.upscale_normal, above_0, positive);
        else if (a.is("--upscale-depth")) ok = a.f32(o.upscale_depth, above_0, positive);
        else if (a.is("--upscale-albedo")) ok = a.f32(o.upscale_albedo, above_0, positive);
        else if (a.is("--despike")) ok = a.flag(o.despike, false);
        else if (a.is("--despike-threshold")) ok = a.f32(o.despike_threshold, at_least_1, "a finite number >= 1");
        else if (a.is("--despike-rank")) ok = a.u32(o.despike_rank, 1, RBRT_DESPIKE_MAX_RANK);
        else if (a.is("--despike-radius")) ok = a.u32(o.despike_radius, 1, RBRT_DESPIKE_MAX_RADIUS);
        else if (a.is("--spike-map")) ok = a.text(o.spike_map);
        else if (a.is("--compare")) ok = a.text(o.compare_file, "a PFM file");
        else if (a.is("--compare-epsilon")) ok = a.f32(o.compare_epsilon, above_0, "a finite number above 0");
        else if (a.is("--error-map")) ok = a.text(o.error_map, "a file");
        else if (a.is("--ssim-map")) ok = a.text(o.ssim_map, "a file");
        else if (a.is("--shading")) {
            if ((ok = a.word(w, {"flat", "smooth"}))) o.smooth = w == "smooth";
        } else if (a.is("--seed")) {  // (whatever strtoull makes of it: DESIGN.md)
            if ((ok = a.text(w))) o.seed = std::strtoull(w.c_str(), nullptr, 10);
        } else {
            std::fprintf(stderr, "error: unexpected argument '%s' found\n\nFor more information, try '--help'.\n", a.name.c_str());
            ok = false;
        }
    }
    return ok ? CLI_RUN : 2;
}

namespace {

struct Given {
    const char* name;
    bool given;
};

const char* first_given(std::initializer_list<Given> options) {
    for (const Given& g : options)
        if (g.given) return g.name;
    return nullptr;
}

int refuse(const char* format, const char* a = "", const char* b = "") {
    std::fprintf(stderr, format, a, b);
    return 2;
}

// A stage that renders through one round of the adaptive path: on, it names the first of its conflicts, then needs a sample for
// each half image; off, it names the first of the options that need it.
int check_stage(const char* owner, bool on, std::initializer_list<Given> conflicts, uint32_t samples, std::initializer_list<Given> dependants) {
    if (!on) {
        const char* alone = first_given(dependants);
        return alone ? refuse("error: '%s' needs '%s'\n", alone, owner) : CLI_RUN;
    }
    if (const char* with = first_given(conflicts)) return refuse("error: '%s' cannot be combined with '%s'\n", owner, with);
    if (samples < 2) return refuse("error: '%s' needs '--samples' of at least 2 (each half image needs a sample)\n", owner);
    return CLI_RUN;
}

}  // namespace

int check_cli(const CliOptions& o, rbrt::PfmImage& compare_ref) {
    // one GPU, one blocking call: what the adaptive path refuses, every stage on it refuses by name before anything is loaded
    const Given gpus{"--gpus > 1", o.gpus > 1}, checkpoint{"--checkpoint", !o.checkpoint.empty()}, pass_samples{"--pass-samples", o.pass_samples != 0};
    const Given adaptive{"--adaptive", o.adaptive.has_value()}, sample_map{"--sample-map", !o.sample_map.empty()};
    int rc = CLI_RUN;
    if (o.adaptive) {
        if (const char* with = first_given({gpus, checkpoint, pass_samples})) return refuse("error: '--adaptive' cannot be combined with '%s'\n", with);
        if (o.min_samples < 2 || o.adaptive_step < 1) return refuse("error: '--min-samples' must be at least 2 and '--adaptive-step' at least 1\n");
    } else if (sample_map.given && !o.upscale && !o.despike) {  // (with --upscale or --despike the refusal below names both)
        return refuse("error: '--sample-map' needs '--adaptive'\n");
    }
    // the filter's input is the adaptive path's sums; --noisy is also what the three stages below it leave unfiltered
    rc = check_stage("--denoise", o.denoise, {gpus, checkpoint, pass_samples}, o.samples,
                     {{"--denoise-radius", o.denoise_radius.has_value()}, {"--denoise-patch", o.denoise_patch.has_value()},
                      {"--denoise-strength", o.denoise_strength.has_value()}, {"--noisy", !o.noisy.empty() && !o.denoise_guided && !o.upscale && !o.despike}});
    if (rc != CLI_RUN) return rc;
    // the same sums as --denoise, and the feature buffers of one handle
    rc = check_stage("--denoise-guided", o.denoise_guided, {{"--denoise", o.denoise}, gpus, checkpoint, pass_samples}, o.samples,
                     {{"--guided-levels", o.guided_levels.has_value()}, {"--guided-colour", o.guided_colour.has_value()},
                      {"--guided-normal", o.guided_normal.has_value()}, {"--guided-depth", o.guided_depth.has_value()},
                      {"--guided-albedo", o.guided_albedo.has_value()}, {"--guided-no-demodulation", o.guided_no_demodulation}});
    if (rc != CLI_RUN) return rc;
    // every frame is one round of the adaptive path on one handle
    rc = check_stage("--frames", o.frames.has_value(), {adaptive, gpus, checkpoint, pass_samples}, o.samples,
                     {{"--camera-step", o.camera_step_given}, {"--temporal-max-history", o.temporal_max_history.has_value()},
                      {"--temporal-depth", o.temporal_depth.has_value()}, {"--temporal-normal", o.temporal_normal.has_value()},
                      {"--history-map", !o.history_map.empty()}});
    if (rc != CLI_RUN) return rc;
    if (o.motion_step && !o.frames)
        return refuse("error: '--motion-step' needs '--frames' (the spheres advance that many exposures from one frame to the next)\n");
    if (o.motion_step && !std::isfinite(float(*o.frames - 1u) * *o.motion_step))  // (the last frame's phase, float32: the render loop makes the same product)
        return refuse("error: '--motion-step' times the last frame's number is not finite\n");
    if (o.shutter && o.shutter_travel_given) return refuse("error: '--shutter' cannot be combined with '--shutter-travel' (either is the whole travel)\n");
    if (o.shutter && !o.camera_step_given)
        return refuse("error: '--shutter' needs '--camera-step' (the travel is that part of the step; '--shutter-travel' takes a travel itself)\n");
    if (o.shutter)  // travel = S * camera_step, float32: config_of makes the same product
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(*o.shutter * o.camera_step[c])) return refuse("error: '--shutter' times '--camera-step' is not finite\n");
    // a small render through one round of the adaptive path on one handle
    rc = check_stage("--upscale", o.upscale.has_value(), {adaptive, gpus, checkpoint, pass_samples, sample_map}, o.samples,
                     {{"--upscale-normal", o.upscale_normal.has_value()}, {"--upscale-depth", o.upscale_depth.has_value()},
                      {"--upscale-albedo", o.upscale_albedo.has_value()}});
    if (rc != CLI_RUN) return rc;
    // the half images of one round of the adaptive path on one handle
    rc = check_stage("--despike", o.despike, {adaptive, gpus, checkpoint, pass_samples, sample_map}, o.samples,
                     {{"--despike-threshold", o.despike_threshold.has_value()}, {"--despike-rank", o.despike_rank.has_value()},
                      {"--despike-radius", o.despike_radius.has_value()}, {"--spike-map", !o.spike_map.empty()}});
    if (rc != CLI_RUN) return rc;
    if (o.compare_file.empty()) {
        const char* alone = first_given({{"--compare-epsilon", o.compare_epsilon.has_value()}, {"--error-map", !o.error_map.empty()}, {"--ssim-map", !o.ssim_map.empty()}});
        if (alone) return refuse("error: '%s' needs '--compare'\n", alone);
    } else {  // the reference is read, and its size checked, before anything is loaded or rendered
        try {
            compare_ref = rbrt::read_pfm(o.compare_file, true);
        } catch (const std::exception& e) {
            return refuse("error: '--compare': cannot read the reference: %s\n", e.what());
        }
        if (compare_ref.width != o.width || compare_ref.height != o.height) {
            std::fprintf(stderr, "error: '--compare': the reference '%s' is %u x %u, the image %u x %u\n", o.compare_file.c_str(), compare_ref.width,
                         compare_ref.height, o.width, o.height);
            return 2;
        }
    }
    if (!o.glare) {
        const char* alone = first_given({{"--glare-threshold", o.glare_threshold.has_value()}, {"--glare-levels", o.glare_levels.has_value()},
                                         {"--glare-spread", o.glare_spread.has_value()}});
        if (alone) return refuse("error: '%s' needs '--glare'\n", alone);
    }
    if (o.features) {  // of the whole frame, on the render's handle
        if (gpus.given) return refuse("error: '--features' cannot be combined with '--gpus > 1'\n");
    } else if (o.feature_samples && !o.denoise_guided && !o.frames && !o.upscale) {
        return refuse("error: '--feature-samples' needs '--features'\n");
    }
    if (o.white && o.tone_curve != RBRT_TONE_REINHARD) return refuse("error: '--white' needs '--tonemap reinhard' (the other curves have no white point)\n");
    if (!o.radiance_file.empty() && !ends_in_pfm(o.radiance_file))
        return refuse("error: invalid value '%s' for '--radiance' (the linear radiance is written as a colour PFM: the name must end in .pfm)\n", o.radiance_file.c_str());
    if (o.environment && *o.environment != "none" && o.constant_background)
        return refuse("error: '--background' cannot be combined with '--environment' (the environment is the background)\n");
    return CLI_RUN;
}

void apply_overrides(rbrt::SceneBlueprint& bp, const CliOptions& o) {
    if (o.aperture) bp.camera_blueprint.camera_aperture_mm = o.aperture;
    if (o.focus_distance) bp.camera_blueprint.camera_focus_distance = o.focus_distance;
    if (o.smooth)
        for (rbrt::TriangleMeshBlueprint& mb : bp.mesh_blueprints) mb.smooth = *o.smooth;
    if (o.environment) {
        if (*o.environment == "none") {
            bp.environment_blueprint.reset();
        } else {
            if (!bp.environment_blueprint) bp.environment_blueprint = rbrt::EnvironmentBlueprint();
            bp.environment_blueprint->file = *o.environment;
        }
    }
    if (bp.environment_blueprint) {
        if (o.environment_rotation) bp.environment_blueprint->rotation_deg = *o.environment_rotation;
        if (o.environment_intensity) bp.environment_blueprint->intensity = *o.environment_intensity;
        if (o.environment_resolution) bp.environment_blueprint->resolution = *o.environment_resolution;
        if (o.constant_background)
            throw rbrt::Error("'--background' cannot be combined with an environment (the scene file has an environment_blueprint; "
                              "'--environment none' switches it off)");
    } else if (o.environment_rotation || o.environment_intensity || o.environment_resolution) {
        throw rbrt::Error("'--environment-rotation', '--environment-intensity' and '--environment-resolution' need an environment "
                          "('--environment FILE' or the scene file's environment_blueprint)");
    }
}

rbrt::RenderConfig config_of(const CliOptions& o, const rbrt::SceneBlueprint& bp) {
    rbrt::RenderConfig cfg;
    cfg.oversubscribe = o.oversubscribe;
    cfg.seed = o.seed;
    cfg.n_gpus = int(o.gpus);
    cfg.pass_spp = o.pass_samples;
    cfg.checkpoint_path = o.checkpoint;
    cfg.checkpoint_every = int(o.checkpoint_every);
    cfg.gather = o.gather;
    cfg.constant_background = o.constant_background;
    for (int c = 0; c < 3; ++c) cfg.background[c] = o.background[c];
    if (o.adaptive) cfg.adaptive = true, cfg.adaptive_threshold = *o.adaptive, cfg.adaptive_min_samples = o.min_samples, cfg.adaptive_step = o.adaptive_step;
    if (o.denoise) {
        cfg.denoise = true, cfg.keep_noisy = !o.noisy.empty();
        if (o.denoise_radius) cfg.denoise_window_radius = *o.denoise_radius;
        if (o.denoise_patch) cfg.denoise_patch_radius = *o.denoise_patch;
        if (o.denoise_strength) cfg.denoise_strength = *o.denoise_strength;
    }
    if (o.denoise_guided) {
        cfg.denoise_guided = true, cfg.keep_noisy = !o.noisy.empty(), cfg.guided_demodulate = !o.guided_no_demodulation;
        if (o.guided_levels) cfg.guided_levels = *o.guided_levels;
        if (o.guided_colour) cfg.guided_colour = *o.guided_colour;
        if (o.guided_normal) cfg.guided_normal = *o.guided_normal;
        if (o.guided_depth) cfg.guided_depth = *o.guided_depth;
        if (o.guided_albedo) cfg.guided_albedo = *o.guided_albedo;
    }
    if (o.glare) {
        cfg.glare = true, cfg.glare_intensity = *o.glare;
        if (o.glare_threshold) cfg.glare_threshold = *o.glare_threshold;
        if (o.glare_levels) cfg.glare_levels = *o.glare_levels;
        if (o.glare_spread) cfg.glare_spread = *o.glare_spread;
    }
    if (o.transformed()) {
        cfg.tonemap = true, cfg.tonemap_curve = o.tone_curve, cfg.tonemap_exposure = o.exposure, cfg.tonemap_key = o.exposure_key;
        cfg.tonemap_white = o.white ? *o.white : 0.0f;
    }
    cfg.no_motion = o.no_motion;
    if (o.motion_step) cfg.motion_step = *o.motion_step;
    if (o.shutter || o.shutter_travel_given) {  // (the flags override the YAML's camera_shutter_travel)
        cfg.shutter = true;
        for (int c = 0; c < 3; ++c) cfg.shutter_travel[c] = o.shutter ? *o.shutter * o.camera_step[c] : o.shutter_travel[c];
    } else if (const auto& tr = bp.camera_blueprint.camera_shutter_travel) {
        cfg.shutter = true, cfg.shutter_travel[0] = tr->x, cfg.shutter_travel[1] = tr->y, cfg.shutter_travel[2] = tr->z;
    }
    if (o.frames) {
        cfg.frames = *o.frames;
        for (int c = 0; c < 3; ++c) cfg.camera_step[c] = o.camera_step[c];
        if (o.temporal_max_history) cfg.temporal_max_history = *o.temporal_max_history;
        if (o.temporal_depth) cfg.temporal_depth = *o.temporal_depth;
        if (o.temporal_normal) cfg.temporal_normal = *o.temporal_normal;
    }
    if (o.upscale) {
        cfg.upscale = *o.upscale, cfg.keep_noisy = !o.noisy.empty();
        if (o.upscale_normal) cfg.upscale_normal = *o.upscale_normal;
        if (o.upscale_depth) cfg.upscale_depth = *o.upscale_depth;
        if (o.upscale_albedo) cfg.upscale_albedo = *o.upscale_albedo;
    }
    if (o.despike) {
        cfg.despike = true, cfg.keep_noisy = !o.noisy.empty();
        if (o.despike_threshold) cfg.despike_threshold = *o.despike_threshold;
        if (o.despike_rank) cfg.despike_rank = *o.despike_rank;
        if (o.despike_radius) cfg.despike_radius = *o.despike_radius;
    }
    if (o.features) cfg.features = true;
    if (o.features || o.denoise_guided || o.frames || o.upscale) cfg.feature_samples = o.feature_samples ? *o.feature_samples : std::max(1u, std::min(o.samples, 8u));
    return cfg;
}

namespace {

// a grey image through the target's writers
void save_grey(const std::string& path, const std::vector<uint8_t>& grey, uint32_t width, uint32_t height) {
    rbrt::ImageBuffer img;
    img.width = width, img.height = height;
    img.rgb.resize(grey.size() * 3);
    for (size_t k = 0; k < grey.size(); ++k) img.rgb[3 * k] = img.rgb[3 * k + 1] = img.rgb[3 * k + 2] = grey[k];
    img.save(path);
}

// a map of the comparison: .pfm gets the floats (three equal channels, like the feature buffers' grey files), every other
// name an 8-bit grey: v clipped to [0, 1], times 255, rounded to nearest; NaN is black
void save_map(const std::string& path, const std::vector<float>& m, uint32_t width, uint32_t height) {
    if (m.size() != size_t(width) * height) throw rbrt::Error("no map to save to " + path);
    if (ends_in_pfm(path)) {
        std::vector<float> three(m.size() * 3);
        for (size_t k = 0; k < m.size(); ++k) three[3 * k] = three[3 * k + 1] = three[3 * k + 2] = m[k];
        rbrt::write_pfm(path, three.data(), width, height);
        return;
    }
    std::vector<uint8_t> grey(m.size());
    for (size_t k = 0; k < m.size(); ++k) {
        const float t = m[k] > 0.0f ? std::min(m[k], 1.0f) : 0.0f;
        grey[k] = uint8_t(std::floor((t * 255.0f) + 0.5f));
    }
    save_grey(path, grey, width, height);
}

}  // namespace

void save_outputs(const CliOptions& o, const rbrt::ImageBuffer& img, const rbrt::ImageComparison& cmp) {
    img.save(o.target);
    if (!o.sample_map.empty()) img.save_sample_map(o.sample_map);
    if (!o.noisy.empty()) img.save_noisy(o.noisy);
    if (!o.radiance_file.empty()) rbrt::write_pfm(o.radiance_file, img.radiance.data(), img.width, img.height);
    if (o.features) img.save_features(*o.features);
    if (!o.spike_map.empty()) {  // at the size that was traced
        if (img.spike_map.empty() || img.spike_map.size() != size_t(img.spike_map_width) * img.spike_map_height) throw rbrt::Error("no spike map to save to " + o.spike_map);
        save_grey(o.spike_map, img.spike_map, img.spike_map_width, img.spike_map_height);
    }
    if (!o.error_map.empty()) save_map(o.error_map, cmp.rel_map, img.width, img.height);
    if (!o.ssim_map.empty()) save_map(o.ssim_map, cmp.ssim_map, img.width, img.height);
    if (!o.history_map.empty()) {  // like the sample map
        if (img.history_map.size() != size_t(img.width) * img.height) throw rbrt::Error("no history map to save to " + o.history_map);
        save_grey(o.history_map, img.history_map, img.width, img.height);
    }
}
