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
#include <cstdio>

#include "cli.hpp"

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

}  // namespace

int main(int argc, char** argv) {
    CliOptions o;
    rbrt::PfmImage compare_ref;
    int rc = parse_cli(argc, argv, o);
    if (rc == CLI_HELP) return usage(), 0;
    if (rc == CLI_RUN) rc = check_cli(o, compare_ref);
    if (rc != CLI_RUN) return rc;
    try {
        CliTimes t;
        t.t0 = CliClock::now();
        rbrt::SceneBlueprint bp = rbrt::load_blueprints_from_yaml_file(o.config);
        apply_overrides(bp, o);
        rbrt::Camera cam = rbrt::camera_from_blueprint(bp.camera_blueprint, o.height, o.width);  // (checks the lens again)
        t.t1 = CliClock::now();
        rbrt::Scene scene = rbrt::create_scene_from_scene_blueprint(bp);  // .obj parse, transform, SoA conversion (mesh.rs:41-181)
        if (bp.environment_blueprint) scene.environment = rbrt::load_environment(*bp.environment_blueprint);  // PFM read, conversion
        t.t2 = CliClock::now();
        rbrt::RenderConfig cfg = config_of(o, bp);
        rbrt::RenderReport rep;
        cfg.report = &rep;
        rbrt::ImageBuffer img = rbrt::render_scene(cam, o.samples, scene, cfg);
        // the comparison: after the frame, on device 0, whatever made the frame (its time on the host is a part of the report's other_s)
        rbrt::ImageComparison cmp;
        if (!o.compare_file.empty()) {
            cmp = rbrt::compare_images(img, compare_ref, o.compare_epsilon ? *o.compare_epsilon : 0.01f, !o.error_map.empty(), !o.ssim_map.empty());
            std::printf("Compared with %s: mse %.9g, mae %.9g, relmse %.9g, psnr %.4f dB, ssim %.6f, max abs %.9g, %u pixels usable, %u skipped\n", o.compare_file.c_str(),
                        cmp.summary.mse, cmp.summary.mae, cmp.summary.relmse, cmp.summary.psnr_db, cmp.summary.ssim, double(cmp.result.max_abs), cmp.result.usable,
                        cmp.result.skipped);
        }
        std::printf("Saving rendered image to %s\n", o.target.c_str());
        t.t3 = CliClock::now();
        save_outputs(o, img, cmp);
        t.t4 = CliClock::now();
        if (!o.report_path.empty()) write_report(o, cfg, rep, scene, cmp, t);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rbrt: %s\n", e.what());
        return 101;  // the exit code of a Rust panic
    }
    return 0;
}
