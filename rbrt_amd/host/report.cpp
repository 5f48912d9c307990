// report.cpp — the `rbrt` command line's --report: one line of JSON about the run, to a file or to stdout.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "cli.hpp"

namespace {

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

// One JSON object on one line: every member is followed by ", ", close() takes the last one back.
struct JsonLine {
    std::string js = "{";

    void raw(const char* k, const std::string& json) { js += std::string("\"") + k + "\": " + json + ", "; }
    void str(const char* k, const std::string& v) { raw(k, "\"" + json_escape(v) + "\""); }
    static std::string text(double v, const char* fmt) {
        char b[64];
        std::snprintf(b, sizeof(b), fmt, v);
        return b;
    }
    void num(const char* k, double v, const char* fmt = "%.6f") { raw(k, text(v, fmt)); }
    // a double with 17 digits, so that it reads back bit for bit; one that is not finite (the PSNR of identical images) as a
    // string, "inf", "-inf" or "nan"
    void dbl(const char* k, double v) {
        if (std::isfinite(v)) num(k, v, "%.17g");
        else str(k, std::isnan(v) ? "nan" : v > 0 ? "inf" : "-inf");
    }
    void vec3(const char* k, const float v[3]) { raw(k, "[" + text(v[0], "%.9g") + ", " + text(v[1], "%.9g") + ", " + text(v[2], "%.9g") + "]"); }
    std::string close() {
        js.resize(js.size() - 2);
        return js + "}\n";
    }
};

}  // namespace

void write_report(const CliOptions& o, const rbrt::RenderConfig& cfg, const rbrt::RenderReport& rep, const rbrt::Scene& scene,
                  const rbrt::ImageComparison& cmp, const CliTimes& t) {
    const auto secs = [](CliClock::time_point a, CliClock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    uint64_t triangles = 0;
    for (const auto& m : scene.triangle_meshes) triangles += m.num_triangles;
    const uint32_t spp = o.samples ? o.samples : 1u;
    const double rendered = o.adaptive_path() ? double(rep.adaptive_samples)
                                              : double(o.width) * double(o.height) * double(spp - rep.resumed_from_sample);  // path samples of THIS run
    JsonLine j;
    j.str("config", o.config), j.str("target_file", o.target);
    j.num("width", o.width, "%.0f"), j.num("height", o.height, "%.0f"), j.num("samples", o.samples, "%.0f"), j.num("seed", double(o.seed), "%.0f");
    j.num("gpus", rep.n_gpus, "%.0f"), j.str("gather", rep.gather);
    j.num("spheres", double(scene.elements.size()), "%.0f"), j.num("meshes", double(scene.triangle_meshes.size()), "%.0f");
    j.num("triangles", double(triangles), "%.0f");
    j.str("bvh_builder", rep.builder), j.num("bvh_nodes", double(rep.bvh_nodes), "%.0f"), j.num("bvh_triangles", double(rep.bvh_triangles), "%.0f");
    j.num("passes", rep.passes, "%.0f"), j.num("pass_samples", rep.pass_spp, "%.0f");
    j.num("checkpoints_written", rep.checkpoints_written, "%.0f"), j.num("resumed_from_sample", rep.resumed_from_sample, "%.0f");
    if (o.adaptive) {  // rounds, samples traced, samples a fixed render would trace, tiles active at the start of each round
        j.num("adaptive_threshold", *o.adaptive, "%.9g"), j.num("min_samples", o.min_samples, "%.0f"), j.num("adaptive_step", o.adaptive_step, "%.0f");
        j.num("adaptive_rounds", rep.adaptive_rounds, "%.0f"), j.num("samples_traced", double(rep.adaptive_samples), "%.0f");
        j.num("samples_fixed", double(rep.adaptive_samples_fixed), "%.0f");
        std::string tiles;
        for (size_t k = 0; k < rep.adaptive_active_tiles.size(); ++k) tiles += (k ? ", " : "") + std::to_string(rep.adaptive_active_tiles[k]);
        j.raw("active_tiles_per_round", "[" + tiles + "]");
    }
    if (scene.environment.n != 0u)  // the map that lit the scene
        j.str("environment_file", scene.environment.file), j.num("environment_resolution", scene.environment.n, "%.0f");
    if (o.denoise) {  // the filter's parameters and its time on the GPU (a part of render_s)
        j.num("denoise_window_radius", cfg.denoise_window_radius, "%.0f"), j.num("denoise_patch_radius", cfg.denoise_patch_radius, "%.0f");
        j.num("denoise_strength", cfg.denoise_strength, "%.9g"), j.num("denoise_ms", rep.denoise_ms, "%.4f");
    }
    if (o.denoise_guided) {  // the guided filter's parameters and its time on the GPU (a part of gather_s, behind the feature buffers)
        j.num("guided_levels", cfg.guided_levels, "%.0f"), j.num("guided_colour", cfg.guided_colour, "%.9g"), j.num("guided_normal", cfg.guided_normal, "%.9g");
        j.num("guided_depth", cfg.guided_depth, "%.9g"), j.num("guided_albedo", cfg.guided_albedo, "%.9g"), j.num("guided_ms", rep.guided_ms, "%.4f");
    }
    if (o.frames) {  // the stream of frames: its options and the accumulation's time on the GPU, the mean per frame (a part of render_s)
        j.num("frames", cfg.frames, "%.0f"), j.num("temporal_max_history", cfg.temporal_max_history, "%.9g"), j.num("temporal_depth", cfg.temporal_depth, "%.9g");
        j.num("temporal_normal", cfg.temporal_normal, "%.9g"), j.num("temporal_ms", rep.temporal_ms, "%.4f");
        j.vec3("camera_step", cfg.camera_step);
    }
    if (cfg.shutter) j.vec3("shutter_travel", cfg.shutter_travel);  // the camera's translation while the shutter was open
    if (const std::vector<float> mv = scene.motion_travels(); !mv.empty() && !cfg.no_motion) {  // the spheres that moved meanwhile: index and travel
        std::string list;
        for (size_t i = 0; i < scene.elements.size(); ++i)
            if (scene.elements[i].shutter_travel)
                list += std::string(list.empty() ? "" : ", ") + "{\"sphere\": " + std::to_string(i) + ", \"travel\": [" + JsonLine::text(mv[3 * i], "%.9g") + ", " +
                        JsonLine::text(mv[3 * i + 1], "%.9g") + ", " + JsonLine::text(mv[3 * i + 2], "%.9g") + "]}";
        j.raw("moving_spheres", "[" + list + "]");
        if (o.motion_step) j.num("motion_step", cfg.motion_step, "%.9g");  // the exposures they advance from one frame to the next
    }
    if (const std::vector<float> mw = scene.mesh_motion_travels(); !mw.empty() && !cfg.no_motion) {  // ... and the meshes: index and travel
        std::string list;
        for (size_t i = 0; i < scene.triangle_meshes.size(); ++i)
            if (scene.triangle_meshes[i].shutter_travel)
                list += std::string(list.empty() ? "" : ", ") + "{\"mesh\": " + std::to_string(i) + ", \"travel\": [" + JsonLine::text(mw[3 * i], "%.9g") + ", " +
                        JsonLine::text(mw[3 * i + 1], "%.9g") + ", " + JsonLine::text(mw[3 * i + 2], "%.9g") + "]}";
        j.raw("moving_meshes", "[" + list + "]");
        if (o.motion_step && scene.motion_travels().empty()) j.num("motion_step", cfg.motion_step, "%.9g");
    }
    if (o.upscale) {  // guided upsampling: its options, the size that was traced and the stage's time on the GPU, the mean per frame (a part of render_s)
        j.num("upscale", cfg.upscale, "%.0f"), j.num("render_width", rep.render_width, "%.0f"), j.num("render_height", rep.render_height, "%.0f");
        j.num("upscale_normal", cfg.upscale_normal, "%.9g"), j.num("upscale_depth", cfg.upscale_depth, "%.9g"), j.num("upscale_albedo", cfg.upscale_albedo, "%.9g");
        j.num("upsample_ms", rep.upsample_ms, "%.4f");
    }
    if (o.despike) {  // spike removal: its options, the stage's time on the GPU and what it limited in either half image, the means per frame
        j.num("despike_threshold", cfg.despike_threshold, "%.9g"), j.num("despike_rank", cfg.despike_rank, "%.0f"), j.num("despike_radius", cfg.despike_radius, "%.0f");
        j.num("despike_ms", rep.despike_ms, "%.4f"), j.num("spikes_a", rep.spikes_a, "%.9g"), j.num("spikes_b", rep.spikes_b, "%.9g");
    }
    if (o.glare)  // the glare stage: its options and its time on the GPU
        j.num("glare", cfg.glare_intensity, "%.9g"), j.num("glare_levels", cfg.glare_levels, "%.0f"), j.num("glare_ms", rep.glare_ms, "%.4f");
    if (o.transformed()) {  // the display transform: what it chose and its time on the GPU
        j.str("tonemap", o.tone_curve == RBRT_TONE_LINEAR ? "none" : o.tone_curve == RBRT_TONE_REINHARD ? "reinhard" : "aces");
        j.num("exposure", rep.tonemap_exposure, "%.9g"), j.num("white", rep.tonemap_white, "%.9g");
        j.num("luminance_counted", rep.luminance_counted, "%.0f"), j.num("tonemap_ms", rep.tonemap_ms, "%.4f");
    }
    if (!o.compare_file.empty()) {  // the comparison with the reference
        j.str("compare_file", o.compare_file), j.num("compare_epsilon", o.compare_epsilon ? *o.compare_epsilon : 0.01f, "%.9g");
        j.dbl("compare_mse", cmp.summary.mse), j.dbl("compare_mae", cmp.summary.mae), j.dbl("compare_relmse", cmp.summary.relmse);
        j.dbl("compare_psnr_db", cmp.summary.psnr_db), j.dbl("compare_ssim", cmp.summary.ssim), j.dbl("compare_max_abs", double(cmp.result.max_abs));
        j.num("compare_usable", cmp.result.usable, "%.0f"), j.num("compare_skipped", cmp.result.skipped, "%.0f"), j.num("compare_ms", cmp.ms, "%.4f");
    }
    if (o.features)  // the feature buffers: their samples a pixel and their time on the GPU (a part of gather_s)
        j.raw("features", "{\"samples\": " + std::to_string(cfg.feature_samples) + ", \"ms\": " + JsonLine::text(rep.features_ms, "%.4f") + "}");
    // where the run's time went; the parts add up to total_s (other_s is what none of them covers: thread start,
    // checkpoint look-up, the report itself)
    const rbrt::LoadTimes lt = rbrt::load_times();
    const double parse_s = secs(t.t0, t.t1), prep_s = std::max(0.0, secs(t.t1, t.t2) - lt.obj_load_s), encode_s = secs(t.t3, t.t4), total_s = secs(t.t0, t.t4);
    const double named = parse_s + lt.obj_load_s + prep_s + rep.hip_init_s + rep.upload_s + rep.bvh_build_s + rep.lanes_s + rep.buffers_s +
                         rep.render_s + rep.gather_s + rep.release_s + encode_s;
    j.num("parse_s", parse_s), j.num("obj_load_s", lt.obj_load_s), j.num("prep_s", prep_s), j.num("hip_init_s", rep.hip_init_s);
    j.num("upload_s", rep.upload_s), j.num("bvh_build_s", rep.bvh_build_s), j.num("lanes_s", rep.lanes_s), j.num("buffers_s", rep.buffers_s);
    j.num("render_s", rep.render_s), j.num("gather_s", rep.gather_s), j.num("release_s", rep.release_s), j.num("encode_s", encode_s);
    j.num("other_s", std::max(0.0, total_s - named)), j.num("total_s", total_s);
    j.num("upload_build_s", rep.upload_build_s);  // (= hip_init_s' library part + upload_s + bvh_build_s + lanes_s + buffers_s: the name earlier reports used)
    j.num("mray_samples_per_s", rep.render_s > 0 ? rendered / rep.render_s / 1e6 : 0.0, "%.3f");
    const std::string line = j.close();
    if (o.report_path == "-") {
        std::fputs(line.c_str(), stdout);
    } else {
        FILE* f = std::fopen(o.report_path.c_str(), "w");
        if (!f) throw rbrt::Error("cannot write report " + o.report_path);
        std::fputs(line.c_str(), f);
        std::fclose(f);
    }
}
