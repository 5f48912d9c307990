// main.cpp — the `rbrt` command line, same flags and defaults as the reference (src/main.rs:10-50):
//   -t/--target_file dbg_out.png   --height 600   -w/--width 800
//   -c/--config scenes/example_scene.yaml   -s/--samples 5   -h/--help   -V/--version
// plus, not in the reference: --seed N (default 1), --gpus N (default 1), --gather host|rccl, --oversubscribe,
// --pass-samples N, --checkpoint FILE, --checkpoint-every N, --report FILE (machine-readable timing of the run),
// --background R,G,B (a constant background instead of the reference's sky gradient), --aperture MM and
// --focus-distance D (a thin lens: they override the YAML's camera_aperture_mm / camera_focus_distance), --shading flat|smooth
// (overrides every mesh blueprint's `shading`), --adaptive THRESHOLD with --min-samples N and --adaptive-step K (adaptive sampling:
// --samples is the limit), --sample-map FILE (the per-pixel sample count of an adaptive render, scaled to 0-255), --denoise with
// --denoise-radius R, --denoise-patch P and --denoise-strength K (the target file gets the dual-buffer non-local-means filter of
// the render's two half images), --noisy FILE (also the unfiltered image), --environment FILE.pfm | none with
// --environment-rotation DEG, --environment-intensity X and --environment-resolution N (environment lighting: they override
// the YAML's environment_blueprint), --exposure EV|auto with --exposure-key X, --tonemap none|reinhard|aces and --white X|auto
// (the display transform between the radiance and the 8-bit target file: exposure in stops or chosen from the image's
// luminance histogram, and a tone curve that rolls highlights off), --radiance FILE.pfm (the linear radiance, untransformed).
// --glare INTENSITY with --glare-threshold T, --glare-levels L and --glare-spread S (glare: that share of the light above the
// threshold is moved into a bright pixel's surroundings through a pyramid of blurs, in front of the display transform).
// --features PREFIX with --feature-samples N (the feature buffers of the primary rays -- albedo, normal, depth, coverage -- as
// four colour PFMs, made after the render on the same handle). --denoise-guided with --guided-levels L, --guided-colour K,
// --guided-normal K, --guided-depth K, --guided-albedo K and --guided-no-demodulation (the target file gets the edge-avoiding
// a-trous filter of the render's two half images, guided by those feature buffers). --frames N with --camera-step DX,DY,DZ,
// --temporal-max-history M, --temporal-depth K, --temporal-normal K and --history-map FILE (a stream of N frames from a moving
// camera: every frame's half images are accumulated onto the reprojected ones of the frames before it, the last frame is written).
// --upscale F with --upscale-normal K, --upscale-depth K and --upscale-albedo K (the image is traced at 1 / F of its size in each
// direction and its two half images are brought to full size under the guidance of the full-size feature buffers).
// --despike with --despike-threshold T, --despike-rank K, --despike-radius R and --spike-map FILE (a pixel of either half image
// that is far brighter than its neighbours in that half and than the same pixel of the other half is limited, in front of
// every stage that reads the half images).
// --compare REF.pfm with --compare-epsilon E, --error-map FILE and --ssim-map FILE (the frame's final linear radiance against a
// reference image of the same size: MSE, MAE, relative MSE, PSNR and SSIM, on the GPU, in a fixed order of summation).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>

#include "rbrt.hpp"

namespace {

void usage() {
    std::printf(
        "a lighweight raytracer written in rust\n\n"
        "Usage: rbrt [OPTIONS]\n\n"
        "Options:\n"
        "  -t, --target_file <target_file>  file that will be created witht he rendered output [default: dbg_out.png]\n"
        "      --height <height>            target image resolution height [default: 600]\n"
        "  -w, --width <width>              target image resolution width [default: 800]\n"
        "  -c, --config <config>            YAML file that specifies the scene layout and camera specification. "
        "[default: scenes/example_scene.yaml]\n"
        "  -s, --samples <samples>          number of rays per pixel [default: 5]\n"
        "      --seed <seed>                seed of the per-(pixel,sample) random streams [default: 1]\n"
        "      --gpus <gpus>                number of MI355X GPUs to shard pixel tiles over [default: 1]\n"
        "      --gather <how>               multi-GPU image gather: host (each GPU over its own PCIe link) or rccl (GPU to GPU\n"
        "                                   over xGMI, then one copy) [default: host]\n"
        "      --oversubscribe              allow more ranks than GPUs (rank r on GPU r mod n; rehearsal, host gather only)\n"
        "      --report <file>              write a JSON timing report of the run there (- for stdout)\n"
        "      --pass-samples <n>           samples per pass (a progress line, and a checkpoint, per pass) [default: automatic]\n"
        "      --checkpoint <file>          write the running per-pixel sums there after passes and resume from it\n"
        "      --checkpoint-every <n>       checkpoint after every n-th pass [default: 1]\n"
        "      --background <r,g,b>         constant linear background radiance of rays that hit nothing, e.g. 0,0,0 for a scene\n"
        "                                   lit by emissive objects only [default: the sky gradient]\n"
        "      --environment <file|none>    light the scene from a latitude/longitude radiance image (a colour PFM; its top row\n"
        "                                   is +y, its middle column looks along -z) instead of the background; overrides the\n"
        "                                   YAML's environment_blueprint, `none` switches that off. Not with --background\n"
        "      --environment-rotation <deg> turns the environment about +y [default: the YAML's, else 0]\n"
        "      --environment-intensity <x>  scales the environment's radiance, a finite number >= 0 [default: the YAML's, else 1]\n"
        "      --environment-resolution <n> size of the octahedral map made of the image, 1 to 4096 [default: the YAML's, else 1024]\n"
        "      --aperture <mm>              lens diameter in mm, overrides the YAML's camera_aperture_mm; 0 = pinhole\n"
        "                                   [default: the YAML's, else 0]\n"
        "      --focus-distance <d>         distance from the camera position to the plane in focus, along the view\n"
        "                                   direction, in scene units; overrides the YAML's camera_focus_distance\n"
        "      --shading <how>              flat (face normals) or smooth (corner normals: the .obj's vn, else area-weighted\n"
        "                                   vertex normals) for every mesh; overrides the YAML's `shading` [default: the YAML's]\n"
        "      --adaptive <threshold>       adaptive sampling: every 8x8 tile is sampled in rounds until its error estimate\n"
        "                                   falls below the threshold (0 stops nothing early); --samples is the limit.\n"
        "                                   Cannot be combined with --gpus > 1, --checkpoint or --pass-samples\n"
        "      --min-samples <n>            adaptive: samples of the first round, at least 2 [default: 16]\n"
        "      --adaptive-step <k>          adaptive: samples of every later round, at least 1 [default: 64]\n"
        "      --sample-map <file>          adaptive: write the per-pixel sample count there, scaled to 0-255 (same formats as\n"
        "                                   the target file)\n"
        "      --denoise                    filter the image: a dual-buffer non-local-means filter on the images of the even and\n"
        "                                   the odd samples; the target file gets the filtered image. Renders through the adaptive\n"
        "                                   path (without --adaptive: one round, the fixed render), so it cannot be combined with\n"
        "                                   --gpus > 1, --checkpoint or --pass-samples; --samples must be at least 2\n"
        "      --denoise-radius <r>         denoise: radius of the search window, 0 to 10 [default: 5]\n"
        "      --denoise-patch <p>          denoise: radius of the compared patches, 0 to 4 [default: 3]\n"
        "      --denoise-strength <k>       denoise: filter strength, above 0; larger smooths more [default: 0.7]\n"
        "      --noisy <file>               denoise: also write the unfiltered image there (same formats as the target file); with\n"
        "                                   --despike that is the image in front of spike removal (with --upscale as well: the\n"
        "                                   plain mix of the upsampled half images, behind it)\n"
        "      --denoise-guided             filter the image with the feature buffers as guides: an edge-avoiding a-trous filter\n"
        "                                   on the images of the even and the odd samples, which smooths only where albedo,\n"
        "                                   normal and depth of the primary rays agree. Renders like --denoise and cannot be\n"
        "                                   combined with it or with --gpus > 1; --samples must be at least 2; --noisy and\n"
        "                                   --feature-samples apply\n"
        "      --guided-levels <l>          denoise-guided: levels of the filter, 1 to 6; each doubles its reach [default: 5]\n"
        "      --guided-colour <k>          denoise-guided: colour tolerance in standard deviations, above 0 [default: 2]\n"
        "      --guided-normal <k>          denoise-guided: tolerance of the normal's difference, above 0 [default: 0.35]\n"
        "      --guided-depth <k>           denoise-guided: tolerance of the relative depth difference, above 0 [default: 0.05]\n"
        "      --guided-albedo <k>          denoise-guided: tolerance of the albedo's difference, above 0 [default: 0.1]\n"
        "      --guided-no-demodulation     denoise-guided: filter the radiance itself instead of radiance / albedo\n"
        "      --frames <n>                 render a stream of n frames, at least 1, and write the last one: every frame's two half\n"
        "                                   images are mixed with those of the frames before it, reprojected through the depth\n"
        "                                   and normal of the primary rays (temporal accumulation). Frame k renders with seed + k.\n"
        "                                   Renders like --denoise and cannot be combined with --adaptive, --gpus > 1,\n"
        "                                   --checkpoint or --pass-samples; --samples must be at least 2; --denoise or\n"
        "                                   --denoise-guided filter the accumulated image; --feature-samples applies\n"
        "      --camera-step <dx,dy,dz>     frames: frame k's camera position and image centre are moved by k times this\n"
        "                                   [default: 0,0,0]\n"
        "      --shutter-travel <dx,dy,dz>  a camera shutter: the whole camera moves by this, in scene units, while a frame is exposed\n"
        "                                   (motion blur of a translating camera); every sample starts somewhere on the way. Overrides\n"
        "                                   the YAML's camera_shutter_travel; works with --gpus, --adaptive, --features, --upscale,\n"
        "                                   --pass-samples and --checkpoint (a checkpoint resumes only with the same travel)\n"
        "      --shutter <s>                frames: the travel is s times --camera-step, s 0 or more (0.5: open for half the step);\n"
        "                                   frame k still opens at k times the step, and the accumulation reprojects through the\n"
        "                                   opening cameras. Needs --camera-step; not together with --shutter-travel\n"
        "      --temporal-max-history <m>   frames: the longest history a pixel keeps, at least 1 [default: 32]\n"
        "      --temporal-depth <k>         frames: tolerance of the relative depth difference, 0 or more [default: 0.05]\n"
        "      --temporal-normal <k>        frames: tolerance of the normal's difference, 0 or more [default: 0.35]\n"
        "      --history-map <file>         frames: write the last frame's history length over --temporal-max-history there as a\n"
        "                                   grey image (same formats as the target file)\n"
        "      --upscale <f>                trace the image at 1 / f of its width and height, f 2 to 4, and reconstruct the full size:\n"
        "                                   the two half images of the small render are interpolated to --width x --height with\n"
        "                                   weights from the feature buffers of the full-size primary rays (guided upsampling).\n"
        "                                   Renders like --denoise and cannot be combined with --adaptive, --gpus > 1,\n"
        "                                   --checkpoint, --pass-samples or --sample-map; --samples must be at least 2;\n"
        "                                   --frames, --denoise or --denoise-guided work on the full-size half images;\n"
        "                                   --noisy writes their plain mix; --feature-samples applies\n"
        "      --upscale-normal <k>         upscale: tolerance of the normal's difference, above 0 [default: 0.5]\n"
        "      --upscale-depth <k>          upscale: tolerance of the relative depth difference, above 0 [default: 0.1]\n"
        "      --upscale-albedo <k>         upscale: tolerance of the albedo's difference, above 0 [default: 0.2]\n"
        "      --despike                    remove spikes (fireflies): a pixel of either half image whose luminance is above\n"
        "                                   --despike-threshold times the larger of the --despike-rank-th largest luminance among\n"
        "                                   its neighbours in that half and its own luminance in the other half is scaled down to\n"
        "                                   that limit, in front of --upscale, --frames, --denoise and --denoise-guided. Renders\n"
        "                                   like --denoise and cannot be combined with --adaptive, --gpus > 1, --checkpoint,\n"
        "                                   --pass-samples or --sample-map; --samples must be at least 2; --noisy applies\n"
        "      --despike-threshold <t>      despike: the factor above the witnesses, at least 1 [default: 4]\n"
        "      --despike-rank <k>           despike: which of the neighbours' luminances counts, 1 to 4: k + 1 equally bright\n"
        "                                   pixels next to each other are kept [default: 2]\n"
        "      --despike-radius <r>         despike: radius of the neighbourhood, 1 or 2 [default: 2]\n"
        "      --spike-map <file>           despike: write where pixels were limited there as a grey image at the size that was\n"
        "                                   traced: 0 none, 85 the first half image, 170 the second, 255 both\n"
        "      --compare <ref.pfm>          compare the final linear radiance (what --radiance writes; with --frames the last\n"
        "                                   frame) with this colour PFM of the same size, on the GPU, after the frame: prints the\n"
        "                                   MSE, MAE, relative MSE, PSNR (peak 1) and mean SSIM; --report gains compare_*. The\n"
        "                                   sums take a fixed order: the same images give the same bits. Works with every other\n"
        "                                   flag; pixels with a channel that is not finite are skipped and counted\n"
        "      --compare-epsilon <e>        compare: the epsilon of the relative error (x - r)^2 / (r^2 + e), above 0\n"
        "                                   [default: 0.01]\n"
        "      --error-map <file>           compare: write the relative error of every pixel there: .pfm as floats (a colour PFM\n"
        "                                   of three equal channels), any other target format as 8-bit grey, 0 black to 1 and\n"
        "                                   above white\n"
        "      --ssim-map <file>            compare: write the SSIM of every pixel there, likewise: 8-bit grey from 0 and below\n"
        "                                   black to 1 (identical) white\n"
        "      --exposure <EV|auto>         exposure of the target image in stops (the radiance is multiplied by 2^EV), or auto:\n"
        "                                   the median luminance of the image is mapped to --exposure-key [default: 0]\n"
        "      --exposure-key <x>           automatic exposure: what the median luminance is mapped to, above 0 [default: 0.18]\n"
        "      --tonemap <curve>            tone curve of the target image: none (values above 1 clip), reinhard (extended\n"
        "                                   Reinhard on the luminance) or aces (Narkowicz's fit) [default: none]\n"
        "      --white <x|auto>             reinhard only: the exposed luminance that becomes white, above 0, or auto: the\n"
        "                                   image's 99th percentile [default: auto]\n"
        "      --glare <intensity>          glare: move this share, above 0 and at most 1, of the light of pixels brighter than\n"
        "                                   --glare-threshold into their surroundings, before exposure and tone curve\n"
        "      --glare-threshold <t>        glare: the luminance above which a pixel is bright, 0 or more [default: 1]\n"
        "      --glare-levels <l>           glare: levels of the blur pyramid, 1 to 8; each doubles the widest halo [default: 5]\n"
        "      --glare-spread <s>           glare: weight of each coarser level against the one below it, 0 or more [default: 1]\n"
        "      --radiance <file.pfm>        also write the linear radiance there as a colour PFM: before glare, exposure and\n"
        "                                   tone curve, filtered if --denoise is on\n"
        "      --features <prefix>          also write the feature buffers of the primary rays: <prefix>.albedo.pfm, .normal.pfm,\n"
        "                                   .depth.pfm and .coverage.pfm (colour PFMs; depth and coverage as three equal\n"
        "                                   channels). Cannot be combined with --gpus > 1\n"
        "      --feature-samples <n>        features: primary rays per pixel, 1 to 65536 [default: --samples, at most 8]\n"
        "  -h, --help                       Print help\n"
        "  -V, --version                    Print version\n");
}

uint32_t samples_arg_for_report(uint32_t s) { return s ? s : 1u; }

std::string json_escape(const std::string& in) {
    std::string out;
    for (unsigned char ch : in) {
        if (ch == '"' || ch == '\\') {
            out += '\\', out += char(ch);
        } else if (ch < 0x20) {
            char b[8];
            std::snprintf(b, sizeof(b), "\\u%04x", ch);
            out += b;
        } else {
            out += char(ch);
        }
    }
    return out;
}

bool parse_u32(const char* s, uint32_t& out) {
    char* end = nullptr;
    unsigned long v = std::strtoul(s, &end, 10);
    if (end == s || *end != '\0' || v > 0xFFFFFFFFul || s[0] == '-') return false;
    out = uint32_t(v);
    return true;
}

// "R,G,B": three finite, non-negative floats
bool parse_f32(const char* s, float& out) {
    char* end = nullptr;
    const float v = std::strtof(s, &end);
    if (end == s || *end != '\0') return false;
    out = v;
    return true;
}

// "DX,DY,DZ": three finite floats
bool parse_vec3(const char* s, float out[3]) {
    const char* p = s;
    for (int c = 0; c < 3; ++c) {
        char* end = nullptr;
        const float v = std::strtof(p, &end);
        if (end == p || !std::isfinite(v)) return false;
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

bool parse_rgb(const char* s, float out[3]) {
    const char* p = s;
    for (int c = 0; c < 3; ++c) {
        char* end = nullptr;
        const float v = std::strtof(p, &end);
        if (end == p || !std::isfinite(v) || v < 0.0f) return false;
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

}  // namespace

int main(int argc, char** argv) {
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
    std::string history_map;
    std::optional<uint32_t> upscale;  // --upscale turns guided upsampling on; the options below need it
    std::optional<float> upscale_normal, upscale_depth, upscale_albedo;
    bool despike = false;  // --despike turns spike removal on; the options below need it
    std::optional<float> despike_threshold;
    std::optional<uint32_t> despike_rank, despike_radius;
    std::string spike_map;
    std::string compare_file, error_map, ssim_map;  // --compare turns the comparison on; the maps and the epsilon need it
    std::optional<float> compare_epsilon;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        std::string val;
        bool has_val = false;
        size_t eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
            val = a.substr(eq + 1);
            a = a.substr(0, eq);
            has_val = true;
        }
        auto value = [&]() -> const char* {
            if (has_val) return val.c_str();
            if (i + 1 >= argc) {
                std::fprintf(stderr, "error: a value is required for '%s' but none was supplied\n", a.c_str());
                std::exit(2);
            }
            return argv[++i];
        };
        auto u32 = [&](uint32_t& dst) {
            const char* v = value();
            if (!parse_u32(v, dst)) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, a.c_str());
                std::exit(2);
            }
        };
        if (a == "-h" || a == "--help") {
            usage();
            return 0;
        } else if (a == "-V" || a == "--version") {
            std::printf("rbrt 0.1\n");
            return 0;
        } else if (a == "-t" || a == "--target_file") {
            target = value();
        } else if (a == "--height") {
            u32(height);
        } else if (a == "-w" || a == "--width") {
            u32(width);
        } else if (a == "-c" || a == "--config") {
            config = value();
        } else if (a == "-s" || a == "--samples") {
            u32(samples);
        } else if (a == "--gpus") {
            u32(gpus);
        } else if (a == "--pass-samples") {
            u32(pass_samples);
        } else if (a == "--checkpoint-every") {
            u32(checkpoint_every);
        } else if (a == "--checkpoint") {
            checkpoint = value();
        } else if (a == "--gather") {
            gather = value();
            if (gather != "rccl" && gather != "host") {
                std::fprintf(stderr, "error: invalid value '%s' for '--gather' [possible values: rccl, host]\n", gather.c_str());
                return 2;
            }
        } else if (a == "--oversubscribe") {
            oversubscribe = true;
        } else if (a == "--report") {
            report_path = value();
        } else if (a == "--background") {
            const char* v = value();
            if (!parse_rgb(v, background)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--background' (expected R,G,B: three non-negative numbers)\n", v);
                return 2;
            }
            constant_background = true;
        } else if (a == "--aperture" || a == "--focus-distance") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected a number)\n", v, a.c_str());
                return 2;
            }
            (a == "--aperture" ? aperture : focus_distance) = f;
        } else if (a == "--adaptive") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || f < 0.0f) {
                std::fprintf(stderr, "error: invalid value '%s' for '--adaptive' (expected a finite threshold >= 0)\n", v);
                return 2;
            }
            adaptive = f;
        } else if (a == "--min-samples") {
            u32(min_samples);
        } else if (a == "--adaptive-step") {
            u32(adaptive_step);
        } else if (a == "--sample-map") {
            sample_map = value();
        } else if (a == "--denoise") {
            if (has_val) {
                std::fprintf(stderr, "error: '--denoise' takes no value\n");
                return 2;
            }
            denoise = true;
        } else if (a == "--denoise-radius" || a == "--denoise-patch") {
            const bool radius = a == "--denoise-radius";
            uint32_t v = 0;
            u32(v);
            if (v > (radius ? 10u : 4u)) {
                std::fprintf(stderr, "error: invalid value '%u' for '%s' (expected 0 to %u)\n", v, a.c_str(), radius ? 10u : 4u);
                return 2;
            }
            (radius ? denoise_radius : denoise_patch) = v;
        } else if (a == "--denoise-strength") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f > 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--denoise-strength' (expected a finite number > 0)\n", v);
                return 2;
            }
            denoise_strength = f;
        } else if (a == "--noisy") {
            noisy = value();
        } else if (a == "--denoise-guided" || a == "--guided-no-demodulation") {
            if (has_val) {
                std::fprintf(stderr, "error: '%s' takes no value\n", a.c_str());
                return 2;
            }
            (a == "--denoise-guided" ? denoise_guided : guided_no_demodulation) = true;
        } else if (a == "--guided-levels") {
            uint32_t v = 0;
            u32(v);
            if (v < 1u || v > RBRT_GUIDED_MAX_LEVELS) {
                std::fprintf(stderr, "error: invalid value '%u' for '--guided-levels' (expected 1 to %u)\n", v, RBRT_GUIDED_MAX_LEVELS);
                return 2;
            }
            guided_levels = v;
        } else if (a == "--guided-colour" || a == "--guided-normal" || a == "--guided-depth" || a == "--guided-albedo") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f > 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected a finite number > 0)\n", v, a.c_str());
                return 2;
            }
            (a == "--guided-colour" ? guided_colour : a == "--guided-normal" ? guided_normal : a == "--guided-depth" ? guided_depth : guided_albedo) = f;
        } else if (a == "--environment") {
            environment = std::string(value());
            if (environment->empty()) {
                std::fprintf(stderr, "error: invalid value '' for '--environment' (expected a PFM file or `none`)\n");
                return 2;
            }
        } else if (a == "--environment-rotation" || a == "--environment-intensity") {
            const bool rot = a == "--environment-rotation";
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || (!rot && f < 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected a finite number%s)\n", v, a.c_str(), rot ? "" : " >= 0");
                return 2;
            }
            (rot ? environment_rotation : environment_intensity) = f;
        } else if (a == "--environment-resolution") {
            uint32_t v = 0;
            u32(v);
            if (v < 1u || v > 4096u) {
                std::fprintf(stderr, "error: invalid value '%u' for '--environment-resolution' (expected 1 to 4096)\n", v);
                return 2;
            }
            environment_resolution = v;
        } else if (a == "--exposure") {
            const std::string v = value();
            float ev = 0.0f;
            if (v == "auto") {
                exposure = 0.0f;
            } else if (parse_f32(v.c_str(), ev) && std::isfinite(ev) && std::isfinite(exposure = float(std::exp2(double(ev)))) && exposure > 0.0f) {
            } else {
                std::fprintf(stderr, "error: invalid value '%s' for '--exposure' (expected a number of stops whose 2^EV is a finite float above 0, or auto)\n", v.c_str());
                return 2;
            }
        } else if (a == "--exposure-key") {
            const char* v = value();
            if (!parse_f32(v, exposure_key) || !std::isfinite(exposure_key) || !(exposure_key > 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--exposure-key' (expected a finite number > 0)\n", v);
                return 2;
            }
        } else if (a == "--tonemap") {
            const std::string v = value();
            if (v != "none" && v != "reinhard" && v != "aces") {
                std::fprintf(stderr, "error: invalid value '%s' for '--tonemap' [possible values: none, reinhard, aces]\n", v.c_str());
                return 2;
            }
            tone_curve = v == "none" ? RBRT_TONE_LINEAR : v == "reinhard" ? RBRT_TONE_REINHARD : RBRT_TONE_ACES;
        } else if (a == "--white") {
            const std::string v = value();
            float f = 0.0f;
            if (v == "auto") {
                white = 0.0f;
            } else if (parse_f32(v.c_str(), f) && std::isfinite(f) && f > 0.0f) {
                white = f;
            } else {
                std::fprintf(stderr, "error: invalid value '%s' for '--white' (expected a finite number > 0, or auto)\n", v.c_str());
                return 2;
            }
        } else if (a == "--glare") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f > 0.0f) || f > 1.0f) {
                std::fprintf(stderr, "error: invalid value '%s' for '--glare' (expected a number above 0 and at most 1)\n", v);
                return 2;
            }
            glare = f;
        } else if (a == "--glare-threshold" || a == "--glare-spread") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || f < 0.0f) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected a finite number >= 0)\n", v, a.c_str());
                return 2;
            }
            (a == "--glare-threshold" ? glare_threshold : glare_spread) = f + 0.0f;
        } else if (a == "--glare-levels") {
            uint32_t v = 0;
            u32(v);
            if (v < 1u || v > RBRT_GLARE_MAX_LEVELS) {
                std::fprintf(stderr, "error: invalid value '%u' for '--glare-levels' (expected 1 to %u)\n", v, RBRT_GLARE_MAX_LEVELS);
                return 2;
            }
            glare_levels = v;
        } else if (a == "--radiance") {
            radiance_file = value();
        } else if (a == "--features") {
            features = std::string(value());
            if (features->empty()) {
                std::fprintf(stderr, "error: invalid value '' for '--features' (expected the prefix of the four files it writes)\n");
                return 2;
            }
        } else if (a == "--feature-samples") {
            uint32_t v = 0;
            u32(v);
            if (v < 1u || v > 65536u) {
                std::fprintf(stderr, "error: invalid value '%u' for '--feature-samples' (expected 1 to 65536)\n", v);
                return 2;
            }
            feature_samples = v;
        } else if (a == "--frames") {
            uint32_t v = 0;
            u32(v);
            if (v < 1u) {
                std::fprintf(stderr, "error: invalid value '%u' for '--frames' (expected at least 1)\n", v);
                return 2;
            }
            frames = v;
        } else if (a == "--camera-step") {
            const char* v = value();
            if (!parse_vec3(v, camera_step)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--camera-step' (expected DX,DY,DZ: three finite numbers)\n", v);
                return 2;
            }
            camera_step_given = true;
        } else if (a == "--shutter-travel") {
            const char* v = value();
            if (!parse_vec3(v, shutter_travel)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--shutter-travel' (expected DX,DY,DZ: three finite numbers)\n", v);
                return 2;
            }
            shutter_travel_given = true;
        } else if (a == "--shutter") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f >= 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--shutter' (expected a finite number >= 0: the part of a frame's camera step the shutter is open for)\n", v);
                return 2;
            }
            shutter = f + 0.0f;
        } else if (a == "--temporal-max-history" || a == "--temporal-depth" || a == "--temporal-normal") {
            const bool history = a == "--temporal-max-history";
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f >= (history ? 1.0f : 0.0f))) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected a finite number >= %d)\n", v, a.c_str(), history ? 1 : 0);
                return 2;
            }
            (history ? temporal_max_history : a == "--temporal-depth" ? temporal_depth : temporal_normal) = f + 0.0f;
        } else if (a == "--history-map") {
            history_map = value();
        } else if (a == "--upscale") {
            uint32_t v = 0;
            u32(v);
            if (v < 2u || v > RBRT_UPSAMPLE_MAX_FACTOR) {
                std::fprintf(stderr, "error: invalid value '%u' for '--upscale' (expected 2 to %u)\n", v, RBRT_UPSAMPLE_MAX_FACTOR);
                return 2;
            }
            upscale = v;
        } else if (a == "--upscale-normal" || a == "--upscale-depth" || a == "--upscale-albedo") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f > 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '%s' (expected a finite number > 0)\n", v, a.c_str());
                return 2;
            }
            (a == "--upscale-normal" ? upscale_normal : a == "--upscale-depth" ? upscale_depth : upscale_albedo) = f;
        } else if (a == "--despike") {
            despike = true;
        } else if (a == "--despike-threshold") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f >= 1.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--despike-threshold' (expected a finite number >= 1)\n", v);
                return 2;
            }
            despike_threshold = f;
        } else if (a == "--despike-rank" || a == "--despike-radius") {
            const bool rank = a == "--despike-rank";
            const uint32_t most = rank ? RBRT_DESPIKE_MAX_RANK : RBRT_DESPIKE_MAX_RADIUS;
            uint32_t v = 0;
            u32(v);
            if (v < 1u || v > most) {
                std::fprintf(stderr, "error: invalid value '%u' for '%s' (expected 1 to %u)\n", v, a.c_str(), most);
                return 2;
            }
            (rank ? despike_rank : despike_radius) = v;
        } else if (a == "--spike-map") {
            spike_map = value();
        } else if (a == "--compare") {
            compare_file = value();
            if (compare_file.empty()) {
                std::fprintf(stderr, "error: invalid value '' for '--compare' (expected a PFM file)\n");
                return 2;
            }
        } else if (a == "--compare-epsilon") {
            const char* v = value();
            float f = 0.0f;
            if (!parse_f32(v, f) || !std::isfinite(f) || !(f > 0.0f)) {
                std::fprintf(stderr, "error: invalid value '%s' for '--compare-epsilon' (expected a finite number above 0)\n", v);
                return 2;
            }
            compare_epsilon = f;
        } else if (a == "--error-map" || a == "--ssim-map") {
            const std::string v = value();
            if (v.empty()) {
                std::fprintf(stderr, "error: invalid value '' for '%s' (expected a file)\n", a.c_str());
                return 2;
            }
            (a == "--error-map" ? error_map : ssim_map) = v;
        } else if (a == "--shading") {
            const std::string v = value();
            if (v != "flat" && v != "smooth") {
                std::fprintf(stderr, "error: invalid value '%s' for '--shading' [possible values: flat, smooth]\n", v.c_str());
                return 2;
            }
            smooth = v == "smooth";
        } else if (a == "--seed") {
            seed = std::strtoull(value(), nullptr, 10);
        } else {
            std::fprintf(stderr, "error: unexpected argument '%s' found\n\nFor more information, try '--help'.\n",
                         a.c_str());
            return 2;
        }
    }
    if (adaptive) {  // one GPU, one blocking call: refused by name before anything is loaded
        const char* with = gpus > 1 ? "--gpus > 1" : !checkpoint.empty() ? "--checkpoint" : pass_samples != 0 ? "--pass-samples" : nullptr;
        if (with) {
            std::fprintf(stderr, "error: '--adaptive' cannot be combined with '%s'\n", with);
            return 2;
        }
        if (min_samples < 2 || adaptive_step < 1) {
            std::fprintf(stderr, "error: '--min-samples' must be at least 2 and '--adaptive-step' at least 1\n");
            return 2;
        }
    } else if (!sample_map.empty() && !upscale && !despike) {  // (with --upscale or --despike the refusal below names both)
        std::fprintf(stderr, "error: '--sample-map' needs '--adaptive'\n");
        return 2;
    }
    if (denoise) {  // the filter's input is the adaptive path's sums: it inherits that path's refusals, by name, before anything is loaded
        const char* with = gpus > 1 ? "--gpus > 1" : !checkpoint.empty() ? "--checkpoint" : pass_samples != 0 ? "--pass-samples" : nullptr;
        if (with) {
            std::fprintf(stderr, "error: '--denoise' cannot be combined with '%s'\n", with);
            return 2;
        }
        if (samples < 2) {
            std::fprintf(stderr, "error: '--denoise' needs '--samples' of at least 2 (each half image needs a sample)\n");
            return 2;
        }
    } else {
        const char* alone = denoise_radius ? "--denoise-radius" : denoise_patch ? "--denoise-patch" : denoise_strength ? "--denoise-strength"
                            : !noisy.empty() && !denoise_guided && !upscale && !despike ? "--noisy" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--denoise'\n", alone);
            return 2;
        }
    }
    if (denoise_guided) {  // the same sums as --denoise, and the feature buffers of one handle: refused by name before anything is loaded
        const char* with = denoise ? "--denoise" : gpus > 1 ? "--gpus > 1" : !checkpoint.empty() ? "--checkpoint" : pass_samples != 0 ? "--pass-samples" : nullptr;
        if (with) {
            std::fprintf(stderr, "error: '--denoise-guided' cannot be combined with '%s'\n", with);
            return 2;
        }
        if (samples < 2) {
            std::fprintf(stderr, "error: '--denoise-guided' needs '--samples' of at least 2 (each half image needs a sample)\n");
            return 2;
        }
    } else {
        const char* alone = guided_levels ? "--guided-levels" : guided_colour ? "--guided-colour" : guided_normal ? "--guided-normal"
                            : guided_depth ? "--guided-depth" : guided_albedo ? "--guided-albedo" : guided_no_demodulation ? "--guided-no-demodulation" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--denoise-guided'\n", alone);
            return 2;
        }
    }
    if (frames) {  // every frame is one round of the adaptive path on one handle: refused by name before anything is loaded
        const char* with = adaptive ? "--adaptive" : gpus > 1 ? "--gpus > 1" : !checkpoint.empty() ? "--checkpoint" : pass_samples != 0 ? "--pass-samples" : nullptr;
        if (with) {
            std::fprintf(stderr, "error: '--frames' cannot be combined with '%s'\n", with);
            return 2;
        }
        if (samples < 2) {
            std::fprintf(stderr, "error: '--frames' needs '--samples' of at least 2 (each half image needs a sample)\n");
            return 2;
        }
    } else {
        const char* alone = camera_step_given ? "--camera-step" : temporal_max_history ? "--temporal-max-history" : temporal_depth ? "--temporal-depth"
                            : temporal_normal ? "--temporal-normal" : !history_map.empty() ? "--history-map" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--frames'\n", alone);
            return 2;
        }
    }
    if (shutter && shutter_travel_given) {
        std::fprintf(stderr, "error: '--shutter' cannot be combined with '--shutter-travel' (either is the whole travel)\n");
        return 2;
    }
    if (shutter && !camera_step_given) {
        std::fprintf(stderr, "error: '--shutter' needs '--camera-step' (the travel is that part of the step; '--shutter-travel' takes a travel itself)\n");
        return 2;
    }
    if (shutter) {  // travel = S * camera_step, float32
        for (int c = 0; c < 3; ++c) shutter_travel[c] = *shutter * camera_step[c];
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(shutter_travel[c])) {
                std::fprintf(stderr, "error: '--shutter' times '--camera-step' is not finite\n");
                return 2;
            }
    }
    if (upscale) {  // a small render through one round of the adaptive path on one handle: refused by name before anything is loaded
        const char* with = adaptive ? "--adaptive" : gpus > 1 ? "--gpus > 1" : !checkpoint.empty() ? "--checkpoint" : pass_samples != 0 ? "--pass-samples"
                           : !sample_map.empty() ? "--sample-map" : nullptr;
        if (with) {
            std::fprintf(stderr, "error: '--upscale' cannot be combined with '%s'\n", with);
            return 2;
        }
        if (samples < 2) {
            std::fprintf(stderr, "error: '--upscale' needs '--samples' of at least 2 (each half image needs a sample)\n");
            return 2;
        }
    } else {
        const char* alone = upscale_normal ? "--upscale-normal" : upscale_depth ? "--upscale-depth" : upscale_albedo ? "--upscale-albedo" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--upscale'\n", alone);
            return 2;
        }
    }
    if (despike) {  // the half images of one round of the adaptive path on one handle: refused by name before anything is loaded
        const char* with = adaptive ? "--adaptive" : gpus > 1 ? "--gpus > 1" : !checkpoint.empty() ? "--checkpoint" : pass_samples != 0 ? "--pass-samples"
                           : !sample_map.empty() ? "--sample-map" : nullptr;
        if (with) {
            std::fprintf(stderr, "error: '--despike' cannot be combined with '%s'\n", with);
            return 2;
        }
        if (samples < 2) {
            std::fprintf(stderr, "error: '--despike' needs '--samples' of at least 2 (each half image needs a sample)\n");
            return 2;
        }
    } else {
        const char* alone = despike_threshold ? "--despike-threshold" : despike_rank ? "--despike-rank" : despike_radius ? "--despike-radius"
                            : !spike_map.empty() ? "--spike-map" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--despike'\n", alone);
            return 2;
        }
    }
    rbrt::PfmImage compare_ref;  // read, and its size checked, before anything is loaded or rendered
    if (compare_file.empty()) {
        const char* alone = compare_epsilon ? "--compare-epsilon" : !error_map.empty() ? "--error-map" : !ssim_map.empty() ? "--ssim-map" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--compare'\n", alone);
            return 2;
        }
    } else {
        try {
            compare_ref = rbrt::read_pfm(compare_file, true);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "error: '--compare': cannot read the reference: %s\n", e.what());
            return 2;
        }
        if (compare_ref.width != width || compare_ref.height != height) {
            std::fprintf(stderr, "error: '--compare': the reference '%s' is %u x %u, the image %u x %u\n", compare_file.c_str(), compare_ref.width, compare_ref.height,
                         width, height);
            return 2;
        }
    }
    if (!glare) {
        const char* alone = glare_threshold ? "--glare-threshold" : glare_levels ? "--glare-levels" : glare_spread ? "--glare-spread" : nullptr;
        if (alone) {
            std::fprintf(stderr, "error: '%s' needs '--glare'\n", alone);
            return 2;
        }
    }
    if (features) {  // of the whole frame, on the render's handle: refused by name before anything is loaded
        if (gpus > 1) {
            std::fprintf(stderr, "error: '--features' cannot be combined with '--gpus > 1'\n");
            return 2;
        }
    } else if (feature_samples && !denoise_guided && !frames && !upscale) {
        std::fprintf(stderr, "error: '--feature-samples' needs '--features'\n");
        return 2;
    }
    if (white && tone_curve != RBRT_TONE_REINHARD) {
        std::fprintf(stderr, "error: '--white' needs '--tonemap reinhard' (the other curves have no white point)\n");
        return 2;
    }
    if (!radiance_file.empty() && (radiance_file.size() < 4 || radiance_file.compare(radiance_file.size() - 4, 4, ".pfm") != 0)) {
        std::fprintf(stderr, "error: invalid value '%s' for '--radiance' (the linear radiance is written as a colour PFM: the name must end in .pfm)\n",
                     radiance_file.c_str());
        return 2;
    }
    // (0 EV and no curve is the identity: such a run makes no tonemap call at all and writes what it always wrote)
    const bool transformed = exposure != 1.0f || tone_curve != RBRT_TONE_LINEAR;
    if (environment && *environment != "none" && constant_background) {
        std::fprintf(stderr, "error: '--background' cannot be combined with '--environment' (the environment is the background)\n");
        return 2;
    }
    using clock = std::chrono::steady_clock;
    const auto secs = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    try {
        const auto t0 = clock::now();
        rbrt::SceneBlueprint bp = rbrt::load_blueprints_from_yaml_file(config);
        if (aperture) bp.camera_blueprint.camera_aperture_mm = aperture;
        if (focus_distance) bp.camera_blueprint.camera_focus_distance = focus_distance;
        if (smooth)
            for (rbrt::TriangleMeshBlueprint& mb : bp.mesh_blueprints) mb.smooth = *smooth;
        if (environment) {
            if (*environment == "none") {
                bp.environment_blueprint.reset();
            } else {
                if (!bp.environment_blueprint) bp.environment_blueprint = rbrt::EnvironmentBlueprint();
                bp.environment_blueprint->file = *environment;
            }
        }
        if (bp.environment_blueprint) {
            if (environment_rotation) bp.environment_blueprint->rotation_deg = *environment_rotation;
            if (environment_intensity) bp.environment_blueprint->intensity = *environment_intensity;
            if (environment_resolution) bp.environment_blueprint->resolution = *environment_resolution;
            if (constant_background)
                throw rbrt::Error("'--background' cannot be combined with an environment (the scene file has an environment_blueprint; "
                                  "'--environment none' switches it off)");
        } else if (environment_rotation || environment_intensity || environment_resolution) {
            throw rbrt::Error("'--environment-rotation', '--environment-intensity' and '--environment-resolution' need an environment "
                              "('--environment FILE' or the scene file's environment_blueprint)");
        }
        rbrt::Camera cam = rbrt::camera_from_blueprint(bp.camera_blueprint, height, width);  // (checks the lens again)
        const auto t1 = clock::now();
        rbrt::Scene scene = rbrt::create_scene_from_scene_blueprint(bp);  // .obj parse, transform, SoA conversion (mesh.rs:41-181)
        if (bp.environment_blueprint) scene.environment = rbrt::load_environment(*bp.environment_blueprint);  // PFM read, conversion
        const auto t2 = clock::now();
        rbrt::RenderConfig cfg;
        rbrt::RenderReport rep;
        cfg.report = &rep;
        cfg.oversubscribe = oversubscribe;
        cfg.seed = seed;
        cfg.n_gpus = int(gpus);
        cfg.pass_spp = pass_samples;
        cfg.checkpoint_path = checkpoint;
        cfg.checkpoint_every = int(checkpoint_every);
        cfg.gather = gather;
        cfg.constant_background = constant_background;
        for (int c = 0; c < 3; ++c) cfg.background[c] = background[c];
        if (adaptive) cfg.adaptive = true, cfg.adaptive_threshold = *adaptive, cfg.adaptive_min_samples = min_samples, cfg.adaptive_step = adaptive_step;
        if (denoise) {
            cfg.denoise = true, cfg.keep_noisy = !noisy.empty();
            if (denoise_radius) cfg.denoise_window_radius = *denoise_radius;
            if (denoise_patch) cfg.denoise_patch_radius = *denoise_patch;
            if (denoise_strength) cfg.denoise_strength = *denoise_strength;
        }
        if (denoise_guided) {
            cfg.denoise_guided = true, cfg.keep_noisy = !noisy.empty(), cfg.guided_demodulate = !guided_no_demodulation;
            if (guided_levels) cfg.guided_levels = *guided_levels;
            if (guided_colour) cfg.guided_colour = *guided_colour;
            if (guided_normal) cfg.guided_normal = *guided_normal;
            if (guided_depth) cfg.guided_depth = *guided_depth;
            if (guided_albedo) cfg.guided_albedo = *guided_albedo;
        }
        if (glare) {
            cfg.glare = true, cfg.glare_intensity = *glare;
            if (glare_threshold) cfg.glare_threshold = *glare_threshold;
            if (glare_levels) cfg.glare_levels = *glare_levels;
            if (glare_spread) cfg.glare_spread = *glare_spread;
        }
        if (transformed) {
            cfg.tonemap = true, cfg.tonemap_curve = tone_curve, cfg.tonemap_exposure = exposure, cfg.tonemap_key = exposure_key;
            cfg.tonemap_white = white ? *white : 0.0f;
        }
        if (shutter || shutter_travel_given) {  // (the flags override the YAML's camera_shutter_travel)
            cfg.shutter = true;
            for (int c = 0; c < 3; ++c) cfg.shutter_travel[c] = shutter_travel[c];
        } else if (const auto& tr = bp.camera_blueprint.camera_shutter_travel) {
            cfg.shutter = true, cfg.shutter_travel[0] = tr->x, cfg.shutter_travel[1] = tr->y, cfg.shutter_travel[2] = tr->z;
        }
        if (frames) {
            cfg.frames = *frames;
            for (int c = 0; c < 3; ++c) cfg.camera_step[c] = camera_step[c];
            if (temporal_max_history) cfg.temporal_max_history = *temporal_max_history;
            if (temporal_depth) cfg.temporal_depth = *temporal_depth;
            if (temporal_normal) cfg.temporal_normal = *temporal_normal;
        }
        if (upscale) {
            cfg.upscale = *upscale, cfg.keep_noisy = !noisy.empty();
            if (upscale_normal) cfg.upscale_normal = *upscale_normal;
            if (upscale_depth) cfg.upscale_depth = *upscale_depth;
            if (upscale_albedo) cfg.upscale_albedo = *upscale_albedo;
        }
        if (despike) {
            cfg.despike = true, cfg.keep_noisy = !noisy.empty();
            if (despike_threshold) cfg.despike_threshold = *despike_threshold;
            if (despike_rank) cfg.despike_rank = *despike_rank;
            if (despike_radius) cfg.despike_radius = *despike_radius;
        }
        if (features) cfg.features = true;
        if (features || denoise_guided || frames || upscale) cfg.feature_samples = feature_samples ? *feature_samples : std::max(1u, std::min(samples, 8u));
        rbrt::ImageBuffer img = rbrt::render_scene(cam, samples, scene, cfg);
        // the comparison: after the frame, on device 0, whatever made the frame (its time on the host is a part of the report's other_s)
        rbrt::ImageComparison cmp;
        if (!compare_file.empty()) {
            cmp = rbrt::compare_images(img, compare_ref, compare_epsilon ? *compare_epsilon : 0.01f, !error_map.empty(), !ssim_map.empty());
            std::printf("Compared with %s: mse %.9g, mae %.9g, relmse %.9g, psnr %.4f dB, ssim %.6f, max abs %.9g, %u pixels usable, %u skipped\n", compare_file.c_str(),
                        cmp.summary.mse, cmp.summary.mae, cmp.summary.relmse, cmp.summary.psnr_db, cmp.summary.ssim, double(cmp.result.max_abs), cmp.result.usable,
                        cmp.result.skipped);
        }
        std::printf("Saving rendered image to %s\n", target.c_str());
        const auto t3 = clock::now();
        img.save(target);
        if (!sample_map.empty()) img.save_sample_map(sample_map);
        if (!noisy.empty()) img.save_noisy(noisy);
        if (!radiance_file.empty()) rbrt::write_pfm(radiance_file, img.radiance.data(), img.width, img.height);
        if (features) img.save_features(*features);
        if (!spike_map.empty()) {  // a grey image through the same writers, at the size that was traced
            if (img.spike_map.empty() || img.spike_map.size() != size_t(img.spike_map_width) * img.spike_map_height) throw rbrt::Error("no spike map to save to " + spike_map);
            rbrt::ImageBuffer grey;
            grey.width = img.spike_map_width, grey.height = img.spike_map_height;
            grey.rgb.resize(img.spike_map.size() * 3);
            for (size_t k = 0; k < img.spike_map.size(); ++k) grey.rgb[3 * k] = grey.rgb[3 * k + 1] = grey.rgb[3 * k + 2] = img.spike_map[k];
            grey.save(spike_map);
        }
        // a map of the comparison: .pfm gets the floats (three equal channels, like the feature buffers' grey files), every other
        // name an 8-bit grey through the target's writers: v clipped to [0, 1], times 255, rounded to nearest; NaN is black
        const auto save_map = [&](const std::string& path, const std::vector<float>& m) {
            if (m.size() != size_t(img.width) * img.height) throw rbrt::Error("no map to save to " + path);
            if (path.size() >= 4 && path.compare(path.size() - 4, 4, ".pfm") == 0) {
                std::vector<float> three(m.size() * 3);
                for (size_t k = 0; k < m.size(); ++k) three[3 * k] = three[3 * k + 1] = three[3 * k + 2] = m[k];
                rbrt::write_pfm(path, three.data(), img.width, img.height);
                return;
            }
            rbrt::ImageBuffer grey;
            grey.width = img.width, grey.height = img.height;
            grey.rgb.resize(m.size() * 3);
            for (size_t k = 0; k < m.size(); ++k) {
                const float t = m[k] > 0.0f ? std::min(m[k], 1.0f) : 0.0f;
                grey.rgb[3 * k] = grey.rgb[3 * k + 1] = grey.rgb[3 * k + 2] = uint8_t(std::floor((t * 255.0f) + 0.5f));
            }
            grey.save(path);
        };
        if (!error_map.empty()) save_map(error_map, cmp.rel_map);
        if (!ssim_map.empty()) save_map(ssim_map, cmp.ssim_map);
        if (!history_map.empty()) {  // a grey image through the same writers, like the sample map
            if (img.history_map.size() != size_t(img.width) * img.height) throw rbrt::Error("no history map to save to " + history_map);
            rbrt::ImageBuffer grey;
            grey.width = img.width, grey.height = img.height;
            grey.rgb.resize(img.history_map.size() * 3);
            for (size_t k = 0; k < img.history_map.size(); ++k) grey.rgb[3 * k] = grey.rgb[3 * k + 1] = grey.rgb[3 * k + 2] = img.history_map[k];
            grey.save(history_map);
        }
        const auto t4 = clock::now();
        if (!report_path.empty()) {
            uint64_t triangles = 0;
            for (const auto& m : scene.triangle_meshes) triangles += m.num_triangles;
            const uint32_t spp = samples_arg_for_report(samples);
            const double rendered = adaptive || denoise || denoise_guided || frames || upscale || despike ? double(rep.adaptive_samples)
                                             : double(width) * double(height) * double(spp - rep.resumed_from_sample);  // path samples of THIS run
            std::string js = "{";
            const auto str = [&](const char* k, const std::string& v) { js += std::string("\"") + k + "\": \"" + json_escape(v) + "\", "; };
            const auto num = [&](const char* k, double v, const char* fmt = "%.6f") {
                char b[64];
                std::snprintf(b, sizeof(b), fmt, v);
                js += std::string("\"") + k + "\": " + b + ", ";
            };
            str("config", config), str("target_file", target);
            num("width", width, "%.0f"), num("height", height, "%.0f"), num("samples", samples, "%.0f"), num("seed", double(seed), "%.0f");
            num("gpus", rep.n_gpus, "%.0f"), str("gather", rep.gather);
            num("spheres", double(scene.elements.size()), "%.0f"), num("meshes", double(scene.triangle_meshes.size()), "%.0f");
            num("triangles", double(triangles), "%.0f");
            str("bvh_builder", rep.builder), num("bvh_nodes", double(rep.bvh_nodes), "%.0f"), num("bvh_triangles", double(rep.bvh_triangles), "%.0f");
            num("passes", rep.passes, "%.0f"), num("pass_samples", rep.pass_spp, "%.0f");
            num("checkpoints_written", rep.checkpoints_written, "%.0f"), num("resumed_from_sample", rep.resumed_from_sample, "%.0f");
            if (adaptive) {  // rounds, samples traced, samples a fixed render would trace, tiles active at the start of each round
                num("adaptive_threshold", *adaptive, "%.9g"), num("min_samples", min_samples, "%.0f"), num("adaptive_step", adaptive_step, "%.0f");
                num("adaptive_rounds", rep.adaptive_rounds, "%.0f"), num("samples_traced", double(rep.adaptive_samples), "%.0f");
                num("samples_fixed", double(rep.adaptive_samples_fixed), "%.0f");
                js += "\"active_tiles_per_round\": [";
                for (size_t k = 0; k < rep.adaptive_active_tiles.size(); ++k) js += (k ? ", " : "") + std::to_string(rep.adaptive_active_tiles[k]);
                js += "], ";
            }
            if (scene.environment.n != 0u)  // the map that lit the scene
                str("environment_file", scene.environment.file), num("environment_resolution", scene.environment.n, "%.0f");
            if (denoise) {  // the filter's parameters and its time on the GPU (a part of render_s)
                num("denoise_window_radius", cfg.denoise_window_radius, "%.0f"), num("denoise_patch_radius", cfg.denoise_patch_radius, "%.0f");
                num("denoise_strength", cfg.denoise_strength, "%.9g"), num("denoise_ms", rep.denoise_ms, "%.4f");
            }
            if (denoise_guided) {  // the guided filter's parameters and its time on the GPU (a part of gather_s, behind the feature buffers)
                num("guided_levels", cfg.guided_levels, "%.0f"), num("guided_colour", cfg.guided_colour, "%.9g"), num("guided_normal", cfg.guided_normal, "%.9g");
                num("guided_depth", cfg.guided_depth, "%.9g"), num("guided_albedo", cfg.guided_albedo, "%.9g"), num("guided_ms", rep.guided_ms, "%.4f");
            }
            if (frames) {  // the stream of frames: its options and the accumulation's time on the GPU, the mean per frame (a part of render_s)
                num("frames", cfg.frames, "%.0f"), num("temporal_max_history", cfg.temporal_max_history, "%.9g"), num("temporal_depth", cfg.temporal_depth, "%.9g");
                num("temporal_normal", cfg.temporal_normal, "%.9g"), num("temporal_ms", rep.temporal_ms, "%.4f");
                js += "\"camera_step\": [";
                for (int c = 0; c < 3; ++c) {
                    char b[32];
                    std::snprintf(b, sizeof(b), "%s%.9g", c ? ", " : "", double(cfg.camera_step[c]));
                    js += b;
                }
                js += "], ";
            }
            if (cfg.shutter) {  // the camera's translation while the shutter was open
                js += "\"shutter_travel\": [";
                for (int c = 0; c < 3; ++c) {
                    char b[32];
                    std::snprintf(b, sizeof(b), "%s%.9g", c ? ", " : "", double(cfg.shutter_travel[c]));
                    js += b;
                }
                js += "], ";
            }
            if (upscale) {  // guided upsampling: its options, the size that was traced and the stage's time on the GPU, the mean per frame (a part of render_s)
                num("upscale", cfg.upscale, "%.0f"), num("render_width", rep.render_width, "%.0f"), num("render_height", rep.render_height, "%.0f");
                num("upscale_normal", cfg.upscale_normal, "%.9g"), num("upscale_depth", cfg.upscale_depth, "%.9g"), num("upscale_albedo", cfg.upscale_albedo, "%.9g");
                num("upsample_ms", rep.upsample_ms, "%.4f");
            }
            if (despike) {  // spike removal: its options, the stage's time on the GPU and what it limited in either half image, the means per frame
                num("despike_threshold", cfg.despike_threshold, "%.9g"), num("despike_rank", cfg.despike_rank, "%.0f"), num("despike_radius", cfg.despike_radius, "%.0f");
                num("despike_ms", rep.despike_ms, "%.4f"), num("spikes_a", rep.spikes_a, "%.9g"), num("spikes_b", rep.spikes_b, "%.9g");
            }
            if (glare) {  // the glare stage: its options and its time on the GPU
                num("glare", cfg.glare_intensity, "%.9g"), num("glare_levels", cfg.glare_levels, "%.0f"), num("glare_ms", rep.glare_ms, "%.4f");
            }
            if (transformed) {  // the display transform: what it chose and its time on the GPU
                str("tonemap", tone_curve == RBRT_TONE_LINEAR ? "none" : tone_curve == RBRT_TONE_REINHARD ? "reinhard" : "aces");
                num("exposure", rep.tonemap_exposure, "%.9g"), num("white", rep.tonemap_white, "%.9g");
                num("luminance_counted", rep.luminance_counted, "%.0f"), num("tonemap_ms", rep.tonemap_ms, "%.4f");
            }
            if (!compare_file.empty()) {  // the comparison with the reference: doubles with 17 digits, so that they read back bit for bit;
                                          // one that is not finite (the PSNR of identical images) as a string, "inf", "-inf" or "nan"
                const auto dbl = [&](const char* k, double v) {
                    if (std::isfinite(v)) num(k, v, "%.17g");
                    else str(k, std::isnan(v) ? "nan" : v > 0 ? "inf" : "-inf");
                };
                str("compare_file", compare_file), num("compare_epsilon", compare_epsilon ? *compare_epsilon : 0.01f, "%.9g");
                dbl("compare_mse", cmp.summary.mse), dbl("compare_mae", cmp.summary.mae), dbl("compare_relmse", cmp.summary.relmse);
                dbl("compare_psnr_db", cmp.summary.psnr_db), dbl("compare_ssim", cmp.summary.ssim), dbl("compare_max_abs", double(cmp.result.max_abs));
                num("compare_usable", cmp.result.usable, "%.0f"), num("compare_skipped", cmp.result.skipped, "%.0f"), num("compare_ms", cmp.ms, "%.4f");
            }
            if (features) {  // the feature buffers: their samples a pixel and their time on the GPU (a part of gather_s)
                char b[96];
                std::snprintf(b, sizeof(b), "\"features\": {\"samples\": %u, \"ms\": %.4f}, ", cfg.feature_samples, rep.features_ms);
                js += b;
            }
            // where the run's time went; the parts add up to total_s (other_s is what none of them covers: thread start,
            // checkpoint look-up, the report itself)
            const rbrt::LoadTimes lt = rbrt::load_times();
            const double parse_s = secs(t0, t1), prep_s = std::max(0.0, secs(t1, t2) - lt.obj_load_s), encode_s = secs(t3, t4), total_s = secs(t0, t4);
            const double named = parse_s + lt.obj_load_s + prep_s + rep.hip_init_s + rep.upload_s + rep.bvh_build_s + rep.lanes_s + rep.buffers_s +
                                 rep.render_s + rep.gather_s + rep.release_s + encode_s;
            num("parse_s", parse_s), num("obj_load_s", lt.obj_load_s), num("prep_s", prep_s), num("hip_init_s", rep.hip_init_s);
            num("upload_s", rep.upload_s), num("bvh_build_s", rep.bvh_build_s), num("lanes_s", rep.lanes_s), num("buffers_s", rep.buffers_s);
            num("render_s", rep.render_s), num("gather_s", rep.gather_s), num("release_s", rep.release_s), num("encode_s", encode_s);
            num("other_s", std::max(0.0, total_s - named)), num("total_s", total_s);
            num("upload_build_s", rep.upload_build_s);  // (= hip_init_s' library part + upload_s + bvh_build_s + lanes_s + buffers_s: the name earlier reports used)
            num("mray_samples_per_s", rep.render_s > 0 ? rendered / rep.render_s / 1e6 : 0.0, "%.3f");
            js.resize(js.size() - 2);
            js += "}\n";
            if (report_path == "-") {
                std::fputs(js.c_str(), stdout);
            } else {
                FILE* f = std::fopen(report_path.c_str(), "w");
                if (!f) throw rbrt::Error("cannot write report " + report_path);
                std::fputs(js.c_str(), f);
                std::fclose(f);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rbrt: %s\n", e.what());
        return 101;  // the exit code of a Rust panic
    }
    return 0;
}
