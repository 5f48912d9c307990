// render.cpp — rbrt::render_scene: the call the reference makes at src/main.rs:82, routed through the C ABI to the
// GPU(s).
//
// One worker thread per GPU. Every GPU holds the scene + BVH and renders its interleaved 8x8 pixel tiles
// (rbrt_render_opts_t::tile_rank / tile_world) in PASSES of samples (rbrt_hip_render_pass: per-pixel sums in sample
// order, so the image does not depend on how the samples are cut into passes). After each pass the reference's
// progress line is printed (lib.rs:105-110 prints one per finished column; here a pass is the unit of progress) and,
// if asked for, a checkpoint is written: the running sums of every rank plus the number of samples done. A later run
// with the same scene, size, sample count, seed and GPU count resumes from it.
// When all samples are in, the image has to reach HOST memory (the caller saves a file: src/main.rs:86). Default
// (`--gather host`): every rank copies its own packed tiles over its own PCIe link and de-interleaves them on the host --
// N parallel transfers of 1/N of the image each. `--gather rccl`: the packed fp32 radiance of ranks 1..N-1 goes to rank
// 0's GPU with ONE grouped RCCL send/recv (each peer over its own xGMI link: SURVEY 8(e)), rank 0 de-interleaves it
// with rbrt_hip_unpack_tiles and quantises, then the whole image crosses ONE PCIe link; that is the shape bench.py's
// device-resident gather has, kept here for hosts that want the image on GPU 0. librccl is loaded with dlopen the first
// time that path is asked for: a single-GPU run, or the host gather, does not depend on it.
// RenderConfig::oversubscribe (CLI --oversubscribe) maps rank r to device r % n_devices, so that every line of the
// N-rank path except the RCCL calls themselves (which need distinct devices) runs on a box with fewer GPUs.
//
// How the file reads: render_scene, at the end, is the list of steps. make_plan refuses what cannot be rendered and starts the
// HIP runtime; the checkpoint's fingerprint, reader and writer are checkpoint.cpp (no GPU code); bring_up_rccl makes the
// communicators. A rank is a `Rank`: setup, render_adaptive (with denoise) or render_passes, one of gather_single /
// gather_rccl / gather_host, release -- the four timed regions of Rank::run. What the ranks only read is the `Job`, what they
// share and write is `Shared` (errors and failure counters, the barrier, checkpoint staging, the report, the timers, rank 0's
// slots). `display` is glare and the display transform of the target and the unfiltered image; a rank calls it on its own
// device, display_after_host_gather after uploading the merged image. Device memory, events, streams and first-error-wins
// are the four small owners at the top; nothing else frees or destroys.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is not linked

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#include "checkpoint.hpp"
#include "rbrt.hpp"
#include "../../include/rbrt_hip_debug.h"

namespace rbrt {
namespace {

class Barrier {  // all-ranks rendezvous between passes (checkpoint consistency, RCCL group entry)
  public:
    explicit Barrier(int n) : n_(n) {}
    void wait() {
        std::unique_lock<std::mutex> lk(m_);
        const uint64_t gen = gen_;
        if (++count_ == n_) {
            count_ = 0;
            ++gen_;
            cv_.notify_all();
        } else {
            cv_.wait(lk, [&] { return gen_ != gen; });
        }
    }

  private:
    std::mutex m_;
    std::condition_variable cv_;
    int n_, count_ = 0;
    uint64_t gen_ = 0;
};

// librccl, loaded on first use (`--gather rccl` with more than one GPU).
struct RcclApi {
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    void* handle = nullptr;

    static const RcclApi& get() {  // throws rbrt::Error when the library or a symbol is missing
        static const RcclApi api = load();
        return api;
    }

  private:
    static RcclApi load() {
        RcclApi a;
        for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            a.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (a.handle) break;
        }
        if (!a.handle) throw Error(std::string("--gather rccl: cannot load librccl.so (") + dlerror() + "); use --gather host");
        auto sym = [&](const char* n) {
            void* p = dlsym(a.handle, n);
            if (!p) throw Error(std::string("--gather rccl: librccl.so lacks ") + n);
            return p;
        };
        a.CommInitAll = reinterpret_cast<decltype(a.CommInitAll)>(sym("ncclCommInitAll"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
        a.CommAbort = reinterpret_cast<decltype(a.CommAbort)>(sym("ncclCommAbort"));
        a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(sym("ncclGroupStart"));
        a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(sym("ncclGroupEnd"));
        a.Send = reinterpret_cast<decltype(a.Send)>(sym("ncclSend"));
        a.Recv = reinterpret_cast<decltype(a.Recv)>(sym("ncclRecv"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
        return a;
    }
};

size_t npix_tiles(uint32_t width, uint32_t height) {
    return size_t((width + RBRT_TILE - 1) / RBRT_TILE) * ((height + RBRT_TILE - 1) / RBRT_TILE);
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The display transform's options of a render (rbrt_hip.h "Display transform"). Only the Reinhard curve reads the white point:
// the other curves get a manual one, so that no histogram is made on its account.
rbrt_tonemap_opts_t tonemap_opts_of(const RenderConfig& cfg) {
    rbrt_tonemap_opts_t t;
    rbrt_tonemap_opts_default(&t);
    t.curve = cfg.tonemap_curve, t.exposure = cfg.tonemap_exposure, t.key = cfg.tonemap_key;
    t.white = cfg.tonemap_curve == RBRT_TONE_REINHARD ? cfg.tonemap_white : 1.0f;
    return t;
}

// The glare stage's options of a render (rbrt_hip.h "Glare").
rbrt_glare_opts_t glare_opts_of(const RenderConfig& cfg) {
    rbrt_glare_opts_t g;
    rbrt_glare_opts_default(&g);
    g.threshold = cfg.glare_threshold, g.intensity = cfg.glare_intensity, g.levels = cfg.glare_levels, g.spread = cfg.glare_spread;
    return g;
}

// ---- the owners: what is created here ends with its owner, by reset() where the moment matters, else with the scope ---------
// The first error of a sequence of calls; later ones are dropped. `count`, where given, is raised once, with that first error.
class FirstError {
  public:
    explicit FirstError(std::atomic<int>* count = nullptr) : count_(count) {}
    void set(const std::string& m) {
        if (failed_) return;
        failed_ = true;
        msg_ = m.empty() ? "unknown error" : m;
        if (count_) count_->fetch_add(1);
    }
    bool ok(hipError_t e, const char* what) {
        if (e != hipSuccess) set(std::string(what) + ": " + hipGetErrorString(e));
        return e == hipSuccess;
    }
    bool lib_ok(int rbrt_status) {  // of a call into the HIP library, which keeps its own message (rbrt_hip_last_error)
        if (rbrt_status != RBRT_OK) set(rbrt_hip_last_error());
        return rbrt_status == RBRT_OK;
    }
    bool failed() const { return failed_; }
    const std::string& message() const { return msg_; }

  private:
    std::atomic<int>* count_;
    bool failed_ = false;
    std::string msg_;
};

class DeviceBuffer {  // move-only device memory: hipMalloc on request, hipFree at reset() or at the end of its life
  public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) reset(), p_ = o.p_, o.p_ = nullptr;
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    bool alloc(size_t bytes, FirstError& err, const char* what) {
        reset();
        if (!err.ok(hipMalloc(&p_, bytes), what)) p_ = nullptr;
        return p_ != nullptr;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T>
    T* as() const { return static_cast<T*>(p_); }

  private:
    void* p_ = nullptr;
};

class EventTimer {  // two events around one call on a stream: create, start, the call, stop, the caller's synchronise, elapsed
  public:
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
    ~EventTimer() {
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
    }
    bool create(FirstError& err) { return err.ok(hipEventCreate(&e0_), "hipEventCreate") && err.ok(hipEventCreate(&e1_), "hipEventCreate"); }
    void start(hipStream_t s, FirstError& err) { err.ok(hipEventRecord(e0_, s), "hipEventRecord"); }
    void stop(hipStream_t s, FirstError& err) { err.ok(hipEventRecord(e1_, s), "hipEventRecord"); }
    bool elapsed(float* ms, FirstError& err) {  // only of a sequence without an error
        return !err.failed() && err.ok(hipEventElapsedTime(ms, e0_, e1_), "hipEventElapsedTime");
    }

  private:
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

class Stream {  // a rank's non-blocking stream: destroyed at reset() or at the end of its life
  public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { reset(); }
    bool create(FirstError& err) { return err.ok(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), "hipStreamCreate"); }
    void reset() {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }
    hipStream_t get() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};

// ---- display: glare, then the display transform, of one complete image -------------------------------------------------------
struct DisplaySite {  // where: the device and stream, the image's size, 8-bit staging memory of that device for one image
    int dev;
    hipStream_t stream;
    uint32_t w, h;
    uint8_t* d_rgb8;
};
struct DisplayStats {
    rbrt_tonemap_result_t chosen{};  // what rbrt_hip_tonemap chose
    float tonemap_ms = 0.0f, glare_ms = 0.0f;  // each call between two events
};

// rbrt_hip_glare on d_src. The stage that ends the chain writes the 8-bit image: without a display transform that is this one,
// through site.d_rgb8 to host_rgb; with one, the glared radiance goes to *d_glared, memory of this call's making.
void glare_stage(const RenderConfig& cfg, const DisplaySite& site, const float* d_src, DeviceBuffer* d_glared, uint8_t* host_rgb, float* ms,
                 FirstError& err) {
    const rbrt_glare_opts_t g = glare_opts_of(cfg);
    const size_t n_pixels = size_t(site.w) * site.h;
    DeviceBuffer ws;
    EventTimer timer;
    if (!(err.ok(hipSetDevice(site.dev), "hipSetDevice") &&
          ws.alloc(rbrt_hip_glare_workspace_bytes(site.w, site.h, g.levels), err, "hipMalloc(glare workspace)") &&
          (!cfg.tonemap || d_glared->alloc(n_pixels * 3 * sizeof(float), err, "hipMalloc(glared radiance)")) && timer.create(err)))
        return;
    timer.start(site.stream, err);
    err.lib_ok(rbrt_hip_glare(site.dev, site.stream, d_src, site.w, site.h, &g, ws.as<void>(), d_glared->as<float>(), cfg.tonemap ? nullptr : site.d_rgb8));
    timer.stop(site.stream, err);
    if (!cfg.tonemap) err.ok(hipMemcpyAsync(host_rgb, site.d_rgb8, n_pixels * 3, hipMemcpyDeviceToHost, site.stream), "download of the glared image");
    err.ok(hipStreamSynchronize(site.stream), "glare");
    timer.elapsed(ms, err);
}

// rbrt_hip_tonemap on d_src with the options `t`: the quantised result through site.d_rgb8 to host_rgb, what the call chose
// and its time to *st.
void tonemap_stage(const DisplaySite& site, const float* d_src, const rbrt_tonemap_opts_t& t, uint8_t* host_rgb, DisplayStats* st, FirstError& err) {
    const size_t n_pixels = size_t(site.w) * site.h;
    DeviceBuffer ws;
    EventTimer timer;
    if (!(err.ok(hipSetDevice(site.dev), "hipSetDevice") && ws.alloc(RBRT_TONEMAP_WORKSPACE_BYTES, err, "hipMalloc(tonemap workspace)") &&
          timer.create(err)))
        return;
    timer.start(site.stream, err);
    err.lib_ok(rbrt_hip_tonemap(site.dev, site.stream, d_src, n_pixels, &t, ws.as<void>(), nullptr, site.d_rgb8));
    timer.stop(site.stream, err);
    err.ok(hipMemcpyAsync(&st->chosen, ws.as<char>() + RBRT_TONEMAP_RESULT_OFFSET, sizeof(st->chosen), hipMemcpyDeviceToHost, site.stream),
           "download of the tonemap result");
    err.ok(hipMemcpyAsync(host_rgb, site.d_rgb8, n_pixels * 3, hipMemcpyDeviceToHost, site.stream), "download of the transformed image");
    err.ok(hipStreamSynchronize(site.stream), "tonemap");
    timer.elapsed(&st->tonemap_ms, err);
}

// What stands between the complete image's radiance d_src and its 8-bit image in host_rgb: the glare stage, where the render
// has one, then the display transform, where it has one. `err` must come in clean.
void display_one(const RenderConfig& cfg, const DisplaySite& site, const float* d_src, const rbrt_tonemap_opts_t& t, uint8_t* host_rgb,
                 DisplayStats* st, FirstError& err) {
    DeviceBuffer d_glared;
    if (cfg.glare) glare_stage(cfg, site, d_src, &d_glared, host_rgb, &st->glare_ms, err);
    if (!err.failed() && cfg.tonemap) tonemap_stage(site, d_glared ? d_glared.as<float>() : d_src, t, host_rgb, st, err);
}

// The target image, then the unfiltered image where one is kept (d_noisy: its radiance, else null): img.rgb becomes the
// quantisation of the result (img.radiance stays linear and without glare); the unfiltered image goes through the same glare
// options and, as manual values, the exposure and white chosen for the target. The report's display figures are the target's.
void display(const RenderConfig& cfg, const DisplaySite& site, const float* d_src, const float* d_noisy, ImageBuffer& img, RenderReport& rep,
             FirstError& err) {
    DisplayStats st;
    display_one(cfg, site, d_src, tonemap_opts_of(cfg), img.rgb.data(), &st, err);
    if (err.failed()) return;
    if (cfg.tonemap) {
        rep.tonemap_exposure = st.chosen.exposure, rep.tonemap_white = st.chosen.white, rep.luminance_counted = st.chosen.counted;
        rep.tonemap_ms = st.tonemap_ms;
    }
    rep.glare_ms = st.glare_ms;
    if (!d_noisy) return;
    rbrt_tonemap_opts_t t = tonemap_opts_of(cfg);
    t.exposure = st.chosen.exposure, t.white = st.chosen.white;
    DisplayStats unreported;
    display_one(cfg, site, d_noisy, t, img.noisy_rgb.data(), &unreported, err);
}

// ---- the plan: everything decided before a rank starts -----------------------------------------------------------------------
struct Plan {
    int n_dev = 0, world = 1;
    bool oversubscribe = false;
    double hip_start_s = 0.0;  // what the process's first HIP call took
    uint32_t pass_spp = 0, ckpt_every = 1;
    int stop_after = 0;  // test hook: give up after this many passes of THIS run (as an interrupted run would), checkpoint left on disk
    // --gather rccl is a request, not a condition: whatever keeps RCCL from doing the gather -- the library is not there, two
    // ranks share a device, the communicators do not come up, the exchange itself fails -- sends the ranks to the host gather
    // in the same process (their tiles are still in their own memories), and the run says so on stderr and in --report.
    // `rccl_note` is the reason, once there is one.
    bool want_rccl = false;
    std::string rccl_note;
    int device_of(int rank) const { return oversubscribe ? rank % n_dev : rank; }
};

// Refuses what cannot be rendered, in this order, and starts the HIP runtime: nothing that calls HIP may exist before this.
// adaptive_by: the option that sent the render down the adaptive path, for the messages.
Plan make_plan(const RenderConfig& cfg, const std::string& adaptive_by, bool cfg_adaptive_given, const Camera& cam, const Scene& scene, uint32_t num_samples) {
    if (num_samples == 0) throw Error("the number of samples must be at least 1");
    if (cfg.adaptive) {  // (one blocking call of one GPU: rbrt_hip.h "Adaptive sampling")
        if (cfg.n_gpus > 1) throw Error(adaptive_by + " cannot be combined with --gpus > 1");
        if (!cfg.checkpoint_path.empty()) throw Error(adaptive_by + " cannot be combined with --checkpoint");
        if (cfg.pass_spp != 0) throw Error(adaptive_by + " cannot be combined with --pass-samples");
    }
    if (cfg.denoise && num_samples < 2) throw Error("--denoise needs at least 2 samples (each half image needs one)");
    if (cfg.denoise_guided) {  // (rbrt_hip.h "Guided denoising": the same sums, and the feature buffers of the same handle)
        if (cfg.denoise) throw Error("--denoise-guided cannot be combined with --denoise");
        if (num_samples < 2) throw Error("--denoise-guided needs at least 2 samples (each half image needs one)");
        if (cfg.guided_levels == 0 || cfg.guided_levels > RBRT_GUIDED_MAX_LEVELS) throw Error("--guided-levels must be 1 to 6");
        for (const float k : {cfg.guided_colour, cfg.guided_normal, cfg.guided_depth, cfg.guided_albedo})
            if (!std::isfinite(k) || !(k > 0.0f)) throw Error("--guided-colour, --guided-normal, --guided-depth and --guided-albedo must be finite and above 0");
        if (cfg.feature_samples == 0 || cfg.feature_samples > 65536u) throw Error("--feature-samples must be 1 to 65536");
    }
    if (cfg.shutter)
        for (const float s : cfg.shutter_travel)
            if (!std::isfinite(s)) throw Error("the shutter's travel must be three finite numbers");
    if (cfg.frames) {  // (rbrt_hip.h "Temporal accumulation": every frame is one round of the adaptive path on one handle)
        if (cfg_adaptive_given) throw Error("--frames cannot be combined with --adaptive");
        if (num_samples < 2) throw Error("--frames needs at least 2 samples (each half image needs one)");
        for (const float s : cfg.camera_step)
            if (!std::isfinite(s)) throw Error("--camera-step must be three finite numbers");
        if (!std::isfinite(cfg.temporal_max_history) || !(cfg.temporal_max_history >= 1.0f)) throw Error("--temporal-max-history must be finite and at least 1");
        for (const float k : {cfg.temporal_depth, cfg.temporal_normal})
            if (!std::isfinite(k) || !(k >= 0.0f)) throw Error("--temporal-depth and --temporal-normal must be finite and at least 0");
        if (cfg.feature_samples == 0 || cfg.feature_samples > 65536u) throw Error("--feature-samples must be 1 to 65536");
    }
    if (cfg.upscale) {  // (rbrt_hip.h "Guided upsampling": a small render through one round of the adaptive path on one handle)
        if (cfg_adaptive_given) throw Error("--upscale cannot be combined with --adaptive");
        if (cfg.upscale < 2u || cfg.upscale > RBRT_UPSAMPLE_MAX_FACTOR) throw Error("--upscale must be 2 to 4");
        if (num_samples < 2) throw Error("--upscale needs at least 2 samples (each half image needs one)");
        for (const float k : {cfg.upscale_normal, cfg.upscale_depth, cfg.upscale_albedo})
            if (!std::isfinite(k) || !(k > 0.0f)) throw Error("--upscale-normal, --upscale-depth and --upscale-albedo must be finite and above 0");
        if (cfg.feature_samples == 0 || cfg.feature_samples > 65536u) throw Error("--feature-samples must be 1 to 65536");
    }
    if (cfg.despike) {  // (rbrt_hip.h "Spike removal": on the half images of one round of the adaptive path on one handle)
        if (cfg_adaptive_given) throw Error("--despike cannot be combined with --adaptive");
        if (num_samples < 2) throw Error("--despike needs at least 2 samples (each half image needs one)");
        if (cfg.despike_radius == 0u || cfg.despike_radius > RBRT_DESPIKE_MAX_RADIUS) throw Error("--despike-radius must be 1 or 2");
        if (cfg.despike_rank == 0u || cfg.despike_rank > RBRT_DESPIKE_MAX_RANK) throw Error("--despike-rank must be 1 to 4");
        if (!std::isfinite(cfg.despike_threshold) || !(cfg.despike_threshold >= 1.0f)) throw Error("--despike-threshold must be finite and at least 1");
    }
    if (cfg.features) {  // (of the whole frame, on one handle: rbrt_hip.h "Feature buffers")
        if (cfg.n_gpus > 1) throw Error("--features cannot be combined with --gpus > 1");
        if (cfg.feature_samples == 0 || cfg.feature_samples > 65536u) throw Error("--feature-samples must be 1 to 65536");
    }
    Plan p;
    const auto t_hip0 = std::chrono::steady_clock::now();
    p.n_dev = rbrt_hip_device_count();  // (the process's first HIP call: the runtime starts here)
    p.hip_start_s = seconds_since(t_hip0);
    if (p.n_dev < 1) throw Error(std::string("no HIP device: ") + rbrt_hip_last_error());
    p.world = cfg.n_gpus < 1 ? 1 : cfg.n_gpus;
    p.oversubscribe = cfg.oversubscribe;
    if (p.world > p.n_dev && !cfg.oversubscribe)
        throw Error("requested " + std::to_string(p.world) + " GPUs, " + std::to_string(p.n_dev) + " present");
    p.want_rccl = p.world > 1 && cfg.gather == "rccl";
    if (p.want_rccl && p.world > p.n_dev) {
        p.rccl_note = "--gather rccl needs one GPU per rank (RCCL cannot put two ranks on one device)";
        p.want_rccl = false;
    }
    // samples per pass: what was asked for, else passes of about 2^31 path samples each (a second or so of one GPU's
    // share), so that long renders report progress and can checkpoint; a short render is one pass
    p.pass_spp = cfg.pass_spp;
    if (p.pass_spp == 0) {
        const uint64_t per_spp = uint64_t(cam.img_width_pix) * cam.img_height_pix / uint64_t(p.world) + 1u;
        p.pass_spp = uint32_t(std::min<uint64_t>(num_samples, std::max<uint64_t>(1, (1ull << 31) / per_spp)));
    }
    p.ckpt_every = cfg.checkpoint_every < 1 ? 1u : uint32_t(cfg.checkpoint_every);
    if (const char* e = std::getenv("RBRT_TEST_STOP_AFTER_PASS")) p.stop_after = std::atoi(e);
    if (scene.environment.n != 0u && cfg.constant_background)
        throw Error("--background cannot be combined with an environment (the environment is the background)");
    if (cam.thin_lens && !(rbrt_hip_supported_flags() & RBRT_FLAG_THIN_LENS)) throw Error("the HIP library does not support a thin lens");
    return p;
}

rbrt_render_opts_t render_opts_of(const RenderConfig& cfg, const Camera& cam, uint32_t num_samples) {
    rbrt_render_opts_t opts;
    rbrt_render_opts_default(&opts);
    opts.spp = num_samples;
    opts.seed = cfg.seed;
    if (cfg.constant_background) {
        opts.flags |= RBRT_FLAG_CONSTANT_BACKGROUND;
        for (int c = 0; c < 3; ++c) opts.bg[c] = cfg.background[c];
    }
    if (cam.thin_lens) opts.flags |= RBRT_FLAG_THIN_LENS;
    return opts;
}

// ---- what the ranks share -----------------------------------------------------------------------------------------------------
// What every rank reads and none changes, but for `img`, where the ranks write disjoint pixels.
struct Job {
    const RenderConfig& cfg;
    const Plan& plan;
    const rbrt_camera_lens_t& lens;  // (every call gets &lens.cam, the camera inside its lens: with RBRT_FLAG_THIN_LENS the library reads the lens past it)
    const Scene::AbiView& view;
    const rbrt_environment_t* env;  // null: none
    rbrt_render_opts_t opts;
    uint32_t num_samples;
    CheckpointHeader want;
    CheckpointRead resume;
    ImageBuffer& img;
    std::vector<float> motion;  // Scene::motion_travels, empty without one or with RenderConfig::no_motion: every rank's handle gets it
    std::vector<float> mesh_motion;  // Scene::mesh_motion_travels, likewise
    bool moves() const { return !motion.empty() || !mesh_motion.empty(); }
    size_t n() const { return size_t(img.width) * img.height * 3; }  // values of the complete image
    size_t rank_pixels(int rank) const {  // the pixels a rank renders: its packed tiles, or the image as it is
        return plan.world > 1 ? rbrt_hip_packed_pixels(img.width, img.height, uint32_t(rank), uint32_t(plan.world)) : size_t(img.width) * img.height;
    }
    // A rank's running sums (rbrt_hip_render_pass's d_accum, a checkpoint's share): ALWAYS its packed tiles, one rank included,
    // which is more than the image where its last tiles are ragged.
    size_t sum_floats(int rank) const { return rbrt_hip_packed_pixels(img.width, img.height, uint32_t(rank), uint32_t(plan.world)) * 3; }
};

// Errors: a rank records its first failure in its own FirstError, which raises n_failed. Ranks never have to agree on
// whether to go on rendering (a failed rank keeps meeting the barriers, idle); they DO have to agree on entering the RCCL
// group, and that decision is read between two barriers, when nobody can be failing.
struct Shared {
    explicit Shared(const Plan& plan)
        : errors(plan.world, FirstError(&n_failed)), barrier(plan.world), ckpt_acc(plan.world), comms(plan.world, nullptr), use_rccl(plan.want_rccl),
          rccl_note(plan.rccl_note), t_setup(plan.world, 0.0), t_render(plan.world, 0.0), t_gather(plan.world, 0.0), t_release(plan.world, 0.0),
          t_create(plan.world) {}
    std::atomic<int> n_failed{0};
    std::atomic<int> rccl_failed{0};  // ranks whose part of the RCCL exchange failed: not a failure of the run (host gather instead)
    std::vector<FirstError> errors;   // [rank], each written by its rank alone and read after the ranks have joined
    Barrier barrier;
    std::vector<std::vector<float>> ckpt_acc;  // host copies of the running sums for the checkpoint writer
    const RcclApi* rccl = nullptr;
    std::vector<ncclComm_t> comms;
    bool use_rccl;
    std::mutex note_mutex;  // rccl_note, once the ranks run
    std::string rccl_note;
    DeviceBuffer d_slots;  // rank 0's, RCCL gather: world equal-size slots of packed tiles
    RenderReport rep;
    bool displayed = false;  // rank 0 has run glare and the display transform on its device (else, where either is wanted, they run after the host gather)
    std::vector<double> t_setup, t_render, t_gather, t_release;
    std::vector<rbrt_hip_call_times_t> t_create;
};

// The communicators of `--gather rccl` (one process, one communicator per GPU). Those that do not come up are aborted, the
// note says why, and the run gathers through the host.
void bring_up_rccl(const Plan& plan, Shared& sh) {
    if (sh.use_rccl) {
        try {
            sh.rccl = &RcclApi::get();
            std::vector<int> devs(plan.world);
            for (int r = 0; r < plan.world; ++r) devs[r] = plan.device_of(r);
            const ncclResult_t rc = sh.rccl->CommInitAll(sh.comms.data(), plan.world, devs.data());
            if (rc != ncclSuccess) sh.rccl_note = std::string("ncclCommInitAll: ") + sh.rccl->GetErrorString(rc);
        } catch (const Error& e) {
            sh.rccl_note = e.what();
        }
        if (!sh.rccl_note.empty()) {
            for (ncclComm_t& cm : sh.comms) {
                if (cm && sh.rccl) (void)sh.rccl->CommAbort(cm);
                cm = nullptr;
            }
            sh.use_rccl = false;
        }
    }
    if (!sh.rccl_note.empty()) std::fprintf(stderr, "warning: %s; gathering through host memory instead\n", sh.rccl_note.c_str());
}

// A rank's packed tiles into the row-major image and its quantisation (lib.rs:116-122 on the host): tile tl of the rank is
// tile number tl * world + rank. Ranks write disjoint pixels.
void merge_rank_tiles(const float* packed, size_t n_tiles, uint32_t rank, uint32_t world, uint32_t width, uint32_t height, float* radiance,
                      uint8_t* rgb) {
    const uint32_t tiles_x = (width + RBRT_TILE - 1) / RBRT_TILE;
    for (size_t tl = 0; tl < n_tiles; ++tl) {
        uint32_t ty, tx;
        rbrt_hip_tile_xy(uint32_t(tl) * world + rank, tiles_x, &ty, &tx);
        for (uint32_t p = 0; p < 64; ++p) {
            const uint32_t row = ty * RBRT_TILE + p / 8, col = tx * RBRT_TILE + p % 8;
            if (row >= height || col >= width) continue;
            const size_t src = (tl * 64 + p) * 3, dst = (size_t(row) * width + col) * 3;
            for (int k = 0; k < 3; ++k) {
                const float v = packed[src + k];
                radiance[dst + k] = v;
                const float q = std::sqrt(v) * 256.0f;
                rgb[dst + k] = !(q == q) || q <= 0.0f ? 0 : q >= 255.0f ? 255 : uint8_t(q);
            }
        }
    }
}

// ---- one rank: a thread, a device, its tiles ----------------------------------------------------------------------------------
// Every rank meets every barrier, failed or not: a failed rank skips the work between them, never a wait().
struct Rank {
    Rank(const Job& job_, Shared& sh_, int rank_)
        : job(job_), sh(sh_), cfg(job_.cfg), img(job_.img), rank(rank_), world(job_.plan.world), dev(job_.plan.device_of(rank_)), o(job_.opts),
          npix(job_.rank_pixels(rank_)), err(sh_.errors[rank_]) {
        o.tile_rank = uint32_t(rank);
        o.tile_world = uint32_t(world);
    }
    void run();
    void setup();
    void render_adaptive();
    void keep_noisy();
    void denoise();
    void denoise_guided();
    void render_passes();
    void features();
    void download_features();
    void temporal();
    void gather_single();
    void gather_rccl();
    void gather_host();
    void display_here(const float* d_src);
    void release();

    const Job& job;
    Shared& sh;
    const RenderConfig& cfg;
    ImageBuffer& img;
    const int rank, world, dev;
    rbrt_render_opts_t o;
    const size_t npix;
    FirstError& err;  // this rank's
    uint32_t pass_no = 0;
    rbrt_hip_scene_t* hs = nullptr;
    Stream stream;
    DeviceBuffer d_acc, d_rad, d_rgb, d_img;
    // the motion buffer (rbrt_hip_render_features_motion), 3 floats a pixel: on a scene with a motion, where --features writes it
    // or the frames' accumulation follows the spheres
    DeviceBuffer d_motion;
    bool animated() const { return job.moves() && cfg.frames && cfg.motion_step != 0.0f; }
    bool want_motion() const { return job.moves() && (cfg.features || animated()); }
    DeviceBuffer d_features;  // a render with feature buffers: albedo, normal, depth, coverage (3 + 3 + 1 + 1 floats a pixel)
    DeviceBuffer d_noisy;  // a denoised, glared or transformed render that keeps the unfiltered image: that image's radiance
};

// The four timed regions of a rank; the display stages of a one-GPU render are inside the gather region.
void Rank::run() {
    const auto t_start = std::chrono::steady_clock::now();
    setup();
    sh.t_setup[rank] = seconds_since(t_start);
    const auto t_passes = std::chrono::steady_clock::now();
    if (cfg.frames || cfg.upscale || cfg.despike) temporal();
    else if (cfg.adaptive) render_adaptive();
    else render_passes();
    if (rank == 0) sh.rep.passes = pass_no;
    // the reference would have panicked on a NaN discriminant (sphere.rs:33): surface it
    if (hs && !err.failed()) err.lib_ok(rbrt_hip_scene_check(hs));
    sh.t_render[rank] = seconds_since(t_passes);
    const auto t_g = std::chrono::steady_clock::now();
    // (a render of several frames, an upsampled or a despiked one has made its feature buffers and filtered its image frame by frame: temporal())
    const bool by_frames = cfg.frames || cfg.upscale || cfg.despike;
    if (world == 1 && !by_frames && (cfg.features || cfg.denoise_guided)) features();
    if (world == 1 && !by_frames && cfg.denoise_guided) denoise_guided();  // (in front of glare and the display transform, like denoise)
    if (world == 1) gather_single();
    else if (sh.use_rccl) gather_rccl();
    else gather_host();
    sh.t_gather[rank] = seconds_since(t_g);
    const auto t_rel = std::chrono::steady_clock::now();
    release();
    sh.t_release[rank] = seconds_since(t_rel);
}

void Rank::setup() {
    err.lib_ok(rbrt_hip_scene_create_patterned(&job.view.scene, job.view.shading_ptr(), job.view.patterns_ptr(), dev, &hs));
    std::memset(&sh.t_create[rank], 0, sizeof(sh.t_create[rank]));
    if (!hs) return;
    (void)rbrt_hip_scene_create_times(hs, &sh.t_create[rank]);
    // (every pass is followed by a synchronisation here: only the sample batches INSIDE a pass overlap, on three lanes;
    // the library's default of eight is for streams of frames)
    (void)rbrt_hip_scene_set_pipeline(hs, 3);
    if (job.env) err.lib_ok(rbrt_hip_scene_set_environment(hs, job.env));  // (every rank's handle)
    if (cfg.shutter) {  // (every rank's handle as well: every pass, round and frame and the feature buffers read it from there)
        rbrt_shutter_t sht{};
        for (int c = 0; c < 3; ++c) sht.travel[c] = cfg.shutter_travel[c];
        err.lib_ok(rbrt_hip_scene_set_shutter(hs, &sht));
    }
    if (!job.motion.empty()) {  // (and the spheres' travels, which share the shutter's draw)
        rbrt_motion_t mo{};
        mo.n_spheres = uint32_t(job.motion.size() / 3u), mo.travel = job.motion.data();
        err.lib_ok(rbrt_hip_scene_set_motion(hs, &mo));
    }
    if (!job.mesh_motion.empty()) {  // (and the meshes', on the same draw)
        rbrt_mesh_motion_t mm{};
        mm.n_meshes = uint32_t(job.mesh_motion.size() / 3u), mm.travel = job.mesh_motion.data();
        err.lib_ok(rbrt_hip_scene_set_mesh_motion(hs, &mm));
    }
    rbrt_hip_scene_info_t info;
    if (rank == 0 && rbrt_hip_scene_info(hs, &info) == RBRT_OK) {
        sh.rep.bvh_nodes = info.n_nodes, sh.rep.bvh_triangles = info.n_triangles;
        sh.rep.builder = info.n_meshes == 0 ? "none" : info.n_meshes_device_built == info.n_meshes ? "device" : info.n_meshes_device_built == 0 ? "host" : "mixed";
    }
    if (!npix) return;
    err.ok(hipSetDevice(dev), "hipSetDevice");
    stream.create(err);
    d_acc.alloc(job.sum_floats(rank) * sizeof(float), err, "hipMalloc(sums)");
    d_rad.alloc(npix * 3 * sizeof(float), err, "hipMalloc(radiance)");
    if (world == 1) d_rgb.alloc(npix * 3, err, "hipMalloc(rgb8)");
    if (rank == 0 && sh.use_rccl) {
        sh.d_slots.alloc(size_t(world) * job.rank_pixels(0) * 3 * sizeof(float), err, "hipMalloc(slots)");
        d_img.alloc(job.n() * sizeof(float), err, "hipMalloc(image)");
        d_rgb.alloc(job.n(), err, "hipMalloc(rgb8)");
    }
    if (!err.failed() && job.resume.samples_done != 0)
        err.ok(hipMemcpy(d_acc.as<float>(), job.resume.sums[rank].data(), job.sum_floats(rank) * sizeof(float), hipMemcpyHostToDevice), "upload of the checkpoint");
}

// One blocking call instead of the passes: the library's rounds are the passes (one rank: the plan refused anything else).
// Then the sample map, and the denoise stage where the render has one.
void Rank::render_adaptive() {
    if (err.failed() || !npix) return;
    const rbrt_adaptive_opts_t ao = {cfg.adaptive_threshold, cfg.adaptive_min_samples, cfg.adaptive_step, 0u};
    rbrt_adaptive_result_t ar{};
    const size_t n_tiles = npix_tiles(img.width, img.height);
    std::vector<uint32_t> counts(n_tiles);
    {
        DeviceBuffer d_counts;
        if (d_counts.alloc(n_tiles * sizeof(uint32_t), err, "hipMalloc(tile samples)") &&
            err.lib_ok(rbrt_hip_render_adaptive(hs, &job.lens.cam, &o, &ao, stream.get(), d_rad.as<float>(), d_rgb.as<uint8_t>(), d_counts.as<uint32_t>(), nullptr, &ar)))
            err.ok(hipMemcpy(counts.data(), d_counts.as<uint32_t>(), n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost), "download of the tile samples");
    }
    if (err.failed()) return;
    RenderReport& rep = sh.rep;
    rep.adaptive_rounds = ar.rounds, rep.adaptive_samples = ar.samples, rep.adaptive_samples_fixed = ar.samples_fixed;
    rep.adaptive_active_tiles.resize(ar.rounds);
    uint32_t n_rounds = 0;
    (void)rbrt_hip_scene_adaptive_rounds(hs, rep.adaptive_active_tiles.data(), rep.adaptive_active_tiles.size(), &n_rounds);
    pass_no = ar.rounds;
    img.sample_map.assign(size_t(img.width) * img.height, 0);
    const uint32_t tiles_x = (img.width + RBRT_TILE - 1) / RBRT_TILE;
    for (uint32_t row = 0; row < img.height; ++row)
        for (uint32_t col = 0; col < img.width; ++col) {
            const uint32_t t = rbrt_hip_tile_number(row / RBRT_TILE, col / RBRT_TILE, tiles_x);
            img.sample_map[size_t(row) * img.width + col] = uint8_t(uint64_t(counts[t]) * 255u / job.num_samples);
        }
    if (cfg.denoise) denoise();
}

// The unfiltered image, where it is wanted, before a filter writes over it.
void Rank::keep_noisy() {
    const size_t n = job.n();
    if (cfg.keep_noisy) {
        img.noisy_rgb.resize(n);
        err.ok(hipMemcpy(img.noisy_rgb.data(), d_rgb.as<uint8_t>(), n, hipMemcpyDeviceToHost), "download of the unfiltered image");
        if ((cfg.tonemap || cfg.glare) && d_noisy.alloc(n * sizeof(float), err, "hipMalloc(unfiltered radiance)"))
            err.ok(hipMemcpy(d_noisy.as<float>(), d_rad.as<float>(), n * sizeof(float), hipMemcpyDeviceToDevice), "copy of the unfiltered radiance");
    }
}

// The filter works on the handle's sums and writes over the unfiltered image (kept first where it is wanted).
void Rank::denoise() {
    keep_noisy();
    const rbrt_denoise_opts_t dn = {cfg.denoise_window_radius, cfg.denoise_patch_radius, cfg.denoise_strength, 0u};
    EventTimer timer;
    if (!timer.create(err)) return;
    timer.start(stream.get(), err);
    err.lib_ok(rbrt_hip_scene_denoise(hs, &dn, stream.get(), d_rad.as<float>(), d_rgb.as<uint8_t>(), nullptr, nullptr));
    timer.stop(stream.get(), err);
    float ms = 0.0f;
    err.ok(hipStreamSynchronize(stream.get()), "denoise");
    if (timer.elapsed(&ms, err)) sh.rep.denoise_ms = ms;
}

// The guided filter: the handle's sums again, and the feature buffers features() has left on the device.
void Rank::denoise_guided() {
    if (err.failed() || !npix) return;
    keep_noisy();
    const size_t n_pixels = size_t(img.width) * img.height;
    const rbrt_guided_opts_t g = {cfg.guided_levels, cfg.guided_colour, cfg.guided_normal, cfg.guided_depth, cfg.guided_albedo,
                                  cfg.guided_demodulate ? 0u : RBRT_GUIDED_NO_DEMODULATION, {0u, 0u}};
    const float* const d_albedo = d_features.as<float>();
    const float *const d_normal = d_albedo + n_pixels * 3, *const d_depth = d_normal + n_pixels * 3, *const d_coverage = d_depth + n_pixels;
    DeviceBuffer d_workspace;
    EventTimer timer;
    if (!(d_workspace.alloc(rbrt_hip_guided_workspace_bytes(img.width, img.height), err, "hipMalloc(guided workspace)") && timer.create(err))) return;
    timer.start(stream.get(), err);
    err.lib_ok(rbrt_hip_scene_denoise_guided(hs, &g, stream.get(), d_albedo, d_normal, d_depth, d_coverage, d_workspace.as<void>(),
                                             d_rad.as<float>(), d_rgb.as<uint8_t>()));
    timer.stop(stream.get(), err);
    float ms = 0.0f;
    err.ok(hipStreamSynchronize(stream.get()), "guided denoise");
    if (timer.elapsed(&ms, err)) sh.rep.guided_ms = ms;
}

// The passes, from the checkpoint's sample on. The loop bounds are the same for every rank, so every rank meets every barrier.
void Rank::render_passes() {
    const uint32_t num_samples = job.num_samples, pass_spp = job.plan.pass_spp;
    for (uint64_t b = job.resume.samples_done; b < num_samples; b += pass_spp, ++pass_no) {
        const uint32_t e = uint32_t(std::min<uint64_t>(num_samples, b + pass_spp));
        const bool last = e == num_samples;
        if (!err.failed() && npix &&
            err.lib_ok(rbrt_hip_render_pass(hs, &job.lens.cam, &o, stream.get(), uint32_t(b), e, d_acc.as<float>(), last ? d_rad.as<float>() : nullptr,
                                        last && world == 1 ? d_rgb.as<uint8_t>() : nullptr)))
            err.ok(hipStreamSynchronize(stream.get()), "render pass");
        const bool ckpt_now = !cfg.checkpoint_path.empty() && !last && (pass_no + 1) % job.plan.ckpt_every == 0;
        if (ckpt_now && !err.failed() && npix) {
            sh.ckpt_acc[rank].resize(job.sum_floats(rank));
            err.ok(hipMemcpy(sh.ckpt_acc[rank].data(), d_acc.as<float>(), job.sum_floats(rank) * sizeof(float), hipMemcpyDeviceToHost), "download of the running sums");
        }
        if (world > 1 && (ckpt_now || !cfg.quiet)) sh.barrier.wait();  // every rank has finished the pass
        if (rank == 0) {
            if (!cfg.quiet) {  // lib.rs:105-110
                std::printf("\rRendering %.1f%% complete!", double(e) / double(num_samples) * 100.0);
                std::fflush(stdout);
            }
            // (between the two barriers of a checkpointing pass no other rank is running: the counter is stable)
            if (ckpt_now && sh.n_failed.load() == 0) {
                if (!write_checkpoint(cfg.checkpoint_path, job.want, e, sh.ckpt_acc)) err.set("cannot write checkpoint " + cfg.checkpoint_path);
                if (!err.failed()) ++sh.rep.checkpoints_written;
            }
        }
        if (world > 1 && ckpt_now) sh.barrier.wait();  // the sums may change again only after they are on disk
        if (job.plan.stop_after > 0 && int(pass_no) + 1 == job.plan.stop_after && !last)
            err.set("stopped after pass " + std::to_string(job.plan.stop_after) + " (RBRT_TEST_STOP_AFTER_PASS)");
    }
}

// The feature buffers of the frame, after the render, on the same handle and stream: one call between two events, into memory of
// the rank's, then, where --features asked for them, to the image.
void Rank::features() {
    if (err.failed() || !npix) return;
    const size_t n_pixels = size_t(img.width) * img.height;
    rbrt_feature_opts_t fo;
    rbrt_feature_opts_default(&fo);
    fo.samples = cfg.feature_samples;
    EventTimer timer;  // (d_features lives until release: the guided filter reads it)
    if (!(d_features.alloc(n_pixels * 8 * sizeof(float), err, "hipMalloc(feature buffers)") && timer.create(err))) return;
    if (want_motion() && !d_motion.alloc(n_pixels * 3 * sizeof(float), err, "hipMalloc(motion buffer)")) return;
    float* const d_albedo = d_features.as<float>();
    float *const d_normal = d_albedo + n_pixels * 3, *const d_depth = d_normal + n_pixels * 3, *const d_coverage = d_depth + n_pixels;
    timer.start(stream.get(), err);
    if (want_motion())
        err.lib_ok(rbrt_hip_render_features_motion(hs, &job.lens.cam, &o, &fo, stream.get(), d_albedo, d_normal, d_depth, d_coverage, nullptr, d_motion.as<float>()));
    else
        err.lib_ok(rbrt_hip_render_features(hs, &job.lens.cam, &o, &fo, stream.get(), d_albedo, d_normal, d_depth, d_coverage, nullptr));
    timer.stop(stream.get(), err);
    err.ok(hipStreamSynchronize(stream.get()), "feature buffers");
    float ms = 0.0f;
    if (timer.elapsed(&ms, err)) sh.rep.features_ms = ms;
    if (err.failed()) return;
    download_features();
    if (hs && !err.failed()) err.lib_ok(rbrt_hip_scene_check(hs));  // (a NaN discriminant is counted here as in a render)
}

// d_features to the image, where --features asked for them (the filters alone read them on the device: nothing comes to the host).
void Rank::download_features() {
    const size_t n_pixels = size_t(img.width) * img.height;
    const float* const d_albedo = d_features.as<float>();
    const float *const d_normal = d_albedo + n_pixels * 3, *const d_depth = d_normal + n_pixels * 3, *const d_coverage = d_depth + n_pixels;
    if (cfg.features && !err.failed()) {
        img.feature_albedo.resize(n_pixels * 3), img.feature_normal.resize(n_pixels * 3), img.feature_depth.resize(n_pixels), img.feature_coverage.resize(n_pixels);
        err.ok(hipMemcpy(img.feature_albedo.data(), d_albedo, n_pixels * 3 * sizeof(float), hipMemcpyDeviceToHost), "download of the albedo");
        err.ok(hipMemcpy(img.feature_normal.data(), d_normal, n_pixels * 3 * sizeof(float), hipMemcpyDeviceToHost), "download of the normals");
        err.ok(hipMemcpy(img.feature_depth.data(), d_depth, n_pixels * sizeof(float), hipMemcpyDeviceToHost), "download of the depth");
        err.ok(hipMemcpy(img.feature_coverage.data(), d_coverage, n_pixels * sizeof(float), hipMemcpyDeviceToHost), "download of the coverage");
        if (want_motion()) {
            img.feature_motion.resize(n_pixels * 3);
            err.ok(hipMemcpy(img.feature_motion.data(), d_motion.as<float>(), n_pixels * 3 * sizeof(float), hipMemcpyDeviceToHost), "download of the motion buffer");
        }
    }
}

// A stream of cfg.frames frames from a camera that moves by cfg.camera_step a frame; the last one is the image. Per frame: the
// adaptive path's one round that stops nothing (seed + k), its two half images, its feature buffers, and the accumulation onto
// the history the frame before left; two histories alternate. The accumulated halves of the last frame then go through the
// guided filter, the non-local-means filter or, with neither, their plain mix (window radius 0), all with the one mix wa every
// pixel of a one-round render has. The unfiltered image and the feature buffers are the last frame's.
// With cfg.upscale every frame is traced with the low camera of rbrt_hip_upsample_camera, its half images are low size, the
// feature buffers are the full camera's, and rbrt_hip_upsample_halves makes the full-size halves everything behind it reads;
// the unfiltered image is then the plain mix of the last frame's upsampled halves. Without cfg.frames there is one frame and no
// accumulation.
// With cfg.despike rbrt_hip_despike_halves runs right behind the handle's half images, at the size that was traced, in front of
// upsampling, accumulation and either filter: the handle's halves go to two buffers of their own and the stage writes where they
// went without it. The unfiltered image stays the render's own, in front of the stage (with cfg.upscale: the upsampled halves'
// mix, behind it). With cfg.despike alone the feature buffers are made only where something asks for them.
void Rank::temporal() {
    if (err.failed() || !npix) return;
    const size_t n_pixels = size_t(img.width) * img.height, n = job.n();
    const uint32_t num_samples = job.num_samples, n_frames = cfg.frames ? cfg.frames : 1u, factor = cfg.upscale;
    const rbrt_adaptive_opts_t ao = {cfg.adaptive_threshold, cfg.adaptive_min_samples, cfg.adaptive_step, 0u};
    rbrt_denoise_opts_t dn = {cfg.denoise_window_radius, cfg.denoise_patch_radius, cfg.denoise_strength, 0u};
    const rbrt_denoise_opts_t plain_mix = {0u, cfg.denoise_patch_radius, cfg.denoise_strength, 0u};  // exactly A * wa + B * (1 - wa)
    rbrt_feature_opts_t fo;
    rbrt_feature_opts_default(&fo);
    fo.samples = cfg.feature_samples;
    rbrt_temporal_opts_t to;
    rbrt_temporal_opts_default(&to);
    to.max_history = cfg.temporal_max_history, to.depth = cfg.temporal_depth, to.normal = cfg.temporal_normal;
    rbrt_upsample_opts_t uo;
    rbrt_upsample_opts_default(&uo);
    uo.factor = factor ? factor : 1u, uo.normal = cfg.upscale_normal, uo.depth = cfg.upscale_depth, uo.albedo = cfg.upscale_albedo;
    const size_t history_bytes = cfg.frames ? rbrt_hip_temporal_history_bytes(img.width, img.height) : 0;
    if (cfg.frames && history_bytes == 0) {
        err.set("--frames: the image is too large for temporal accumulation (2^31 pixels or more)");
        return;
    }
    const size_t upsample_bytes = factor ? rbrt_hip_upsample_workspace_bytes(img.width, img.height, factor) : 0;
    if (factor && upsample_bytes == 0) {
        err.set("--upscale: the image is too large for guided upsampling (2^31 pixels or more)");
        return;
    }
    const size_t n_low = factor ? size_t((img.width + factor - 1u) / factor) * ((img.height + factor - 1u) / factor) * 3u : 0;  // values of a low half image
    rbrt_despike_opts_t so;
    rbrt_despike_opts_default(&so);
    so.radius = cfg.despike_radius, so.rank = cfg.despike_rank, so.threshold = cfg.despike_threshold;
    const bool need_features = cfg.frames || factor || cfg.denoise_guided || cfg.features;
    DeviceBuffer d_half_a, d_half_b, d_history[2], d_length, d_wa, d_low_a, d_low_b, d_upsample, d_raw_a, d_raw_b, d_spike_mask, d_spike_result;
    EventTimer timer, up_timer, spike_timer;
    if (!(d_features.alloc(n_pixels * 8 * sizeof(float), err, "hipMalloc(feature buffers)") && d_half_a.alloc(n * sizeof(float), err, "hipMalloc(half image)") &&
          d_half_b.alloc(n * sizeof(float), err, "hipMalloc(half image)") && d_wa.alloc(n_pixels * sizeof(float), err, "hipMalloc(mix)") && timer.create(err) &&
          up_timer.create(err)))
        return;
    if (cfg.frames && !(d_history[0].alloc(history_bytes, err, "hipMalloc(history)") && d_history[1].alloc(history_bytes, err, "hipMalloc(history)") &&
                        d_length.alloc(n_pixels * sizeof(float), err, "hipMalloc(history length)")))
        return;
    if (factor && !(d_low_a.alloc(n_low * sizeof(float), err, "hipMalloc(low half image)") && d_low_b.alloc(n_low * sizeof(float), err, "hipMalloc(low half image)") &&
                    d_upsample.alloc(upsample_bytes, err, "hipMalloc(upsampling workspace)")))
        return;
    if (need_features && want_motion() && !d_motion.alloc(n_pixels * 3 * sizeof(float), err, "hipMalloc(motion buffer)")) return;
    float* const d_albedo = d_features.as<float>();
    float *const d_normal = d_albedo + n_pixels * 3, *const d_depth = d_normal + n_pixels * 3, *const d_coverage = d_depth + n_pixels;
    const size_t n_traced = factor ? n_low : n;  // values of a half image at the size that is traced
    if (cfg.despike && !(d_raw_a.alloc(n_traced * sizeof(float), err, "hipMalloc(half image)") && d_raw_b.alloc(n_traced * sizeof(float), err, "hipMalloc(half image)") &&
                         d_spike_mask.alloc(n_traced / 3u, err, "hipMalloc(spike mask)") && d_spike_result.alloc(sizeof(rbrt_despike_result_t), err, "hipMalloc(spike counts)") &&
                         spike_timer.create(err)))
        return;
    // every pixel of a one-round render has the same count n: h = (n + 1) / 2 samples in A, so wa = float(h) * (1.0f / float(n))
    const float inv_n = 1.0f / float(num_samples);
    const std::vector<float> wa(n_pixels, float((num_samples + 1u) / 2u) * inv_n);
    if (!err.ok(hipMemcpy(d_wa.as<float>(), wa.data(), n_pixels * sizeof(float), hipMemcpyHostToDevice), "upload of the mix")) return;
    RenderReport& rep = sh.rep;
    rbrt_camera_lens_t lens_prev = job.lens;
    double ms_sum = 0.0, up_ms_sum = 0.0, spike_ms_sum = 0.0, spikes_a_sum = 0.0, spikes_b_sum = 0.0;
    for (uint32_t k = 0; k < n_frames && !err.failed(); ++k) {
        rbrt_camera_lens_t lens = job.lens;  // (with a thin lens the lens moves with its camera)
        for (int c = 0; c < 3; ++c) {
            const float shift = float(k) * cfg.camera_step[c];
            lens.cam.position[c] = job.lens.cam.position[c] + shift;
            lens.cam.img_center_point[c] = job.lens.cam.img_center_point[c] + shift;
        }
        // (with a shutter -- the handle's state, Rank::setup -- frame k is exposed from this camera on, over cfg.shutter_travel; the
        // accumulation below reprojects through these opening cameras, as it does without one)
        // Animation: frame k exposes the spheres from the phase float(k) * step on, one phase for the low render and the full-size
        // features of the frame (without the flag, or with a step of 0, the handle keeps the phase 0 it was made with)
        if (animated() && !err.lib_ok(rbrt_hip_scene_set_motion_phase(hs, float(k) * cfg.motion_step))) break;
        rbrt_camera_lens_t traced = lens;  // (the low camera keeps the lens: lens_u, lens_v and focus_scale; the travel is in scene units and stays, too)
        if (factor && !err.lib_ok(rbrt_hip_upsample_camera(&lens.cam, factor, &traced.cam))) break;
        rep.render_width = traced.cam.img_width_pix, rep.render_height = traced.cam.img_height_pix;
        rbrt_render_opts_t ok = o;
        ok.seed = o.seed + k;  // (the same seed would accumulate the same noise)
        rbrt_adaptive_result_t ar{};
        // (d_rad and d_rgb are full size: a low image fits)
        if (!err.lib_ok(rbrt_hip_render_adaptive(hs, &traced.cam, &ok, &ao, stream.get(), d_rad.as<float>(), d_rgb.as<uint8_t>(), nullptr, nullptr, &ar))) break;
        rep.adaptive_rounds = ar.rounds, rep.adaptive_samples += ar.samples, rep.adaptive_samples_fixed += ar.samples_fixed;
        float *const d_traced_a = (factor ? d_low_a : d_half_a).as<float>(), *const d_traced_b = (factor ? d_low_b : d_half_b).as<float>();
        if (!err.lib_ok(rbrt_hip_scene_denoise(hs, &dn, stream.get(), nullptr, nullptr, cfg.despike ? d_raw_a.as<float>() : d_traced_a,
                                               cfg.despike ? d_raw_b.as<float>() : d_traced_b)))
            break;
        if (cfg.despike) {
            spike_timer.start(stream.get(), err);
            err.lib_ok(rbrt_hip_despike_halves(dev, stream.get(), d_raw_a.as<float>(), d_raw_b.as<float>(), traced.cam.img_width_pix, traced.cam.img_height_pix, &so,
                                               d_traced_a, d_traced_b, d_spike_mask.as<uint8_t>(), d_spike_result.as<rbrt_despike_result_t>()));
            spike_timer.stop(stream.get(), err);
        }
        if (need_features && want_motion()) {
            if (!err.lib_ok(rbrt_hip_render_features_motion(hs, &lens.cam, &ok, &fo, stream.get(), d_albedo, d_normal, d_depth, d_coverage, nullptr, d_motion.as<float>()))) break;
        } else if (need_features && !err.lib_ok(rbrt_hip_render_features(hs, &lens.cam, &ok, &fo, stream.get(), d_albedo, d_normal, d_depth, d_coverage, nullptr))) {
            break;
        }
        if (factor) {
            up_timer.start(stream.get(), err);
            err.lib_ok(rbrt_hip_upsample_halves(dev, stream.get(), d_low_a.as<float>(), d_low_b.as<float>(), nullptr, d_albedo, d_normal, d_depth, d_coverage,
                                                img.width, img.height, &uo, d_upsample.as<void>(), d_half_a.as<float>(), d_half_b.as<float>(), nullptr));
            up_timer.stop(stream.get(), err);
            if (cfg.keep_noisy && k + 1u == n_frames)  // the unfiltered image: the upsampled halves' plain mix, before the accumulation
                err.lib_ok(rbrt_hip_denoise_halves(dev, stream.get(), d_half_a.as<float>(), d_half_b.as<float>(), d_wa.as<float>(), img.width, img.height,
                                                   &plain_mix, d_rad.as<float>(), d_rgb.as<uint8_t>()));
        }
        if (animated()) {  // the history is looked up where the spheres were a step ago
            timer.start(stream.get(), err);
            err.lib_ok(rbrt_hip_temporal_accumulate_moving(dev, stream.get(), d_half_a.as<float>(), d_half_b.as<float>(), d_normal, d_depth, d_coverage,
                                                           d_motion.as<float>(), cfg.motion_step, &lens.cam, k ? &lens_prev.cam : nullptr, &to,
                                                           k ? d_history[(k - 1u) & 1u].as<void>() : nullptr, d_history[k & 1u].as<void>(), d_half_a.as<float>(),
                                                           d_half_b.as<float>(), k + 1u == cfg.frames ? d_length.as<float>() : nullptr));
            timer.stop(stream.get(), err);
        } else if (cfg.frames) {
            timer.start(stream.get(), err);
            err.lib_ok(rbrt_hip_temporal_accumulate(dev, stream.get(), d_half_a.as<float>(), d_half_b.as<float>(), d_normal, d_depth, d_coverage, &lens.cam,
                                                    k ? &lens_prev.cam : nullptr, &to, k ? d_history[(k - 1u) & 1u].as<void>() : nullptr,
                                                    d_history[k & 1u].as<void>(), d_half_a.as<float>(), d_half_b.as<float>(),
                                                    k + 1u == cfg.frames ? d_length.as<float>() : nullptr));
            timer.stop(stream.get(), err);
        }
        err.ok(hipStreamSynchronize(stream.get()), "frame");
        float ms = 0.0f;
        if (cfg.frames && timer.elapsed(&ms, err)) ms_sum += ms;
        if (factor && up_timer.elapsed(&ms, err)) up_ms_sum += ms;
        if (cfg.despike && !err.failed()) {
            if (spike_timer.elapsed(&ms, err)) spike_ms_sum += ms;
            rbrt_despike_result_t found{};
            if (err.ok(hipMemcpy(&found, d_spike_result.as<void>(), sizeof(found), hipMemcpyDeviceToHost), "download of the spike counts"))
                spikes_a_sum += double(found.spikes_a), spikes_b_sum += double(found.spikes_b);
        }
        if (hs && !err.failed()) err.lib_ok(rbrt_hip_scene_check(hs));
        lens_prev = lens;
        ++pass_no;
        if (!cfg.quiet) {
            std::printf("\rRendering %.1f%% complete!", double(k + 1u) / double(n_frames) * 100.0);
            std::fflush(stdout);
        }
    }
    if (err.failed()) return;
    if (cfg.frames) rep.temporal_ms = ms_sum / double(n_frames);
    if (factor) rep.upsample_ms = up_ms_sum / double(n_frames);
    if (cfg.despike) {  // the means per frame; the mask of the last frame, at the size that was traced
        rep.despike_ms = spike_ms_sum / double(n_frames), rep.spikes_a = spikes_a_sum / double(n_frames), rep.spikes_b = spikes_b_sum / double(n_frames);
        std::vector<uint8_t> mask(n_traced / 3u);
        if (err.ok(hipMemcpy(mask.data(), d_spike_mask.as<void>(), mask.size(), hipMemcpyDeviceToHost), "download of the spike mask")) {
            img.spike_map.resize(mask.size());
            for (size_t i = 0; i < mask.size(); ++i) img.spike_map[i] = uint8_t((mask[i] & 3u) * 85u);  // 0 none, 85 A, 170 B, 255 both
            img.spike_map_width = factor ? (img.width + factor - 1u) / factor : img.width;
            img.spike_map_height = factor ? (img.height + factor - 1u) / factor : img.height;
        }
    }
    keep_noisy();
    if (need_features) download_features();
    if (cfg.frames) {  // the history length of the last frame, as a share of the longest there can be
        std::vector<float> length(n_pixels);
        if (err.ok(hipMemcpy(length.data(), d_length.as<float>(), n_pixels * sizeof(float), hipMemcpyDeviceToHost), "download of the history length")) {
            img.history_map.resize(n_pixels);
            for (size_t i = 0; i < n_pixels; ++i) {
                const float v = (length[i] / cfg.temporal_max_history) * 255.0f;
                img.history_map[i] = !(v == v) || v <= 0.0f ? 0 : v >= 255.0f ? 255 : uint8_t(v);
            }
        }
    }
    if (cfg.denoise_guided) {
        const rbrt_guided_opts_t g = {cfg.guided_levels, cfg.guided_colour, cfg.guided_normal, cfg.guided_depth, cfg.guided_albedo,
                                      cfg.guided_demodulate ? 0u : RBRT_GUIDED_NO_DEMODULATION, {0u, 0u}};
        DeviceBuffer d_workspace;
        if (!d_workspace.alloc(rbrt_hip_guided_workspace_bytes(img.width, img.height), err, "hipMalloc(guided workspace)")) return;
        timer.start(stream.get(), err);
        err.lib_ok(rbrt_hip_denoise_guided(dev, stream.get(), d_half_a.as<float>(), d_half_b.as<float>(), d_wa.as<float>(), d_albedo, d_normal, d_depth,
                                           d_coverage, img.width, img.height, &g, d_workspace.as<void>(), d_rad.as<float>(), d_rgb.as<uint8_t>()));
        timer.stop(stream.get(), err);
        err.ok(hipStreamSynchronize(stream.get()), "guided denoise");
        float ms = 0.0f;
        if (timer.elapsed(&ms, err)) rep.guided_ms = ms;
    } else {
        if (!cfg.denoise) dn.window_radius = 0u;  // exactly A * wa + B * (1 - wa)
        timer.start(stream.get(), err);
        err.lib_ok(rbrt_hip_denoise_halves(dev, stream.get(), d_half_a.as<float>(), d_half_b.as<float>(), d_wa.as<float>(), img.width, img.height, &dn,
                                           d_rad.as<float>(), d_rgb.as<uint8_t>()));
        timer.stop(stream.get(), err);
        err.ok(hipStreamSynchronize(stream.get()), "denoise");
        float ms = 0.0f;
        if (timer.elapsed(&ms, err) && cfg.denoise) rep.denoise_ms = ms;
    }
}

// Glare and the display transform on this rank's device, of the complete image that is d_src there.
void Rank::display_here(const float* d_src) {
    if (!(cfg.tonemap || cfg.glare) || err.failed()) return;
    display(cfg, DisplaySite{dev, stream.get(), img.width, img.height, d_rgb.as<uint8_t>()}, d_src, d_noisy.as<float>(), img, sh.rep, err);
    sh.displayed = true;
}

void Rank::gather_single() {
    if (err.failed() || !npix) return;
    err.ok(hipMemcpy(img.radiance.data(), d_rad.as<float>(), job.n() * sizeof(float), hipMemcpyDeviceToHost), "download");
    err.ok(hipMemcpy(img.rgb.data(), d_rgb.as<uint8_t>(), job.n(), hipMemcpyDeviceToHost), "download");
    display_here(d_rad.as<float>());  // on the radiance that is here already
}

// --gather host: every rank's tiles over its own PCIe link, merged on the host (also where a failed RCCL gather ends).
void Rank::gather_host() {
    if (err.failed() || !npix) return;
    std::vector<float> hr(npix * 3);
    if (err.ok(hipMemcpy(hr.data(), d_rad.as<float>(), hr.size() * sizeof(float), hipMemcpyDeviceToHost), "download"))
        merge_rank_tiles(hr.data(), npix / 64, uint32_t(rank), uint32_t(world), img.width, img.height, img.radiance.data(), img.rgb.data());
}

// --gather rccl: one grouped exchange, rank r > 0 sends its packed tiles, rank 0 receives each into that rank's slot,
// de-interleaves and downloads the image.
void Rank::gather_rccl() {
    const RcclApi* rccl = sh.rccl;
    float* d_slots = sh.d_slots.as<float>();
    const size_t slot_pixels = job.rank_pixels(0);
    // INVARIANT all enter the group or none: the decision is taken ONCE, between two barriers. Before the first every rank
    // has recorded what it had to record, and until the second nobody runs code that can fail.
    sh.barrier.wait();
    const bool go = sh.n_failed.load() == 0;
    sh.barrier.wait();
    if (!go) return;
    bool copied = true;
    if (rank == 0) copied = err.ok(hipMemcpyAsync(d_slots, d_rad.as<float>(), npix * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream.get()), "own tiles");
    // INVARIANT every GroupStart has its GroupEnd, whatever the calls between them return: a rank that left the bracket
    // open would block the others' GroupEnd.
    ncclResult_t rc = rccl->GroupStart();
    if (rank == 0) {
        for (int r = 1; r < world && rc == ncclSuccess; ++r) {
            const size_t cnt = job.rank_pixels(r) * 3;
            if (cnt) rc = rccl->Recv(d_slots + size_t(r) * slot_pixels * 3, cnt, ncclFloat, r, sh.comms[0], stream.get());
        }
    } else if (npix && rc == ncclSuccess) {
        rc = rccl->Send(d_rad.as<float>(), npix * 3, ncclFloat, 0, sh.comms[rank], stream.get());
    }
    const ncclResult_t rc2 = rccl->GroupEnd();
    bool rccl_bad = false;  // this rank's part of the exchange failed: not an error of the run, the host gather takes over
    auto rccl_fail = [&](const std::string& m) {
        rccl_bad = true;
        std::lock_guard<std::mutex> lk(sh.note_mutex);
        if (sh.rccl_note.empty()) sh.rccl_note = m;
        sh.rccl_failed.fetch_add(1);
    };
    if (rc != ncclSuccess || rc2 != ncclSuccess) rccl_fail(std::string("RCCL gather: ") + rccl->GetErrorString(rc != ncclSuccess ? rc : rc2));
    if (rank == 0 && !err.failed() && !rccl_bad && copied)
        err.lib_ok(rbrt_hip_unpack_tiles_strided(dev, stream.get(), d_slots, img.width, img.height, uint32_t(world), slot_pixels, d_img.as<float>(), d_rgb.as<uint8_t>()));
    // INVARIANT no rank waits for ever: if a peer failed inside the group (its send or receive was never enqueued) this
    // rank's side can not complete; it polls, and then aborts its communicator instead of hanging.
    for (;;) {
        const hipError_t q = hipStreamQuery(stream.get());
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) {
            err.ok(q, "gather");
            break;
        }
        if (sh.n_failed.load() != 0 || sh.rccl_failed.load() != 0) {
            if (!rccl_bad) rccl_fail("RCCL gather abandoned: another rank's part of it failed");
            (void)rccl->CommAbort(sh.comms[rank]);
            sh.comms[rank] = nullptr;
            break;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    // INVARIANT all fall back or none: did the exchange work for everyone is again one decision between two barriers. If
    // not, the tiles are still where they were rendered: every rank takes the host path, in this same process.
    sh.barrier.wait();
    const bool fell_back = sh.rccl_failed.load() != 0;
    sh.barrier.wait();
    if (fell_back) return gather_host();
    if (rank != 0 || err.failed()) return;
    err.ok(hipMemcpy(img.radiance.data(), d_img.as<float>(), job.n() * sizeof(float), hipMemcpyDeviceToHost), "download");
    err.ok(hipMemcpy(img.rgb.data(), d_rgb.as<uint8_t>(), job.n(), hipMemcpyDeviceToHost), "download");
    display_here(d_img.as<float>());  // on the gathered image
}

// The lifetimes end here, in this order, inside the release region: nothing is left to fall off the end of the thread.
void Rank::release() {
    d_acc.reset();
    d_rad.reset();
    d_rgb.reset();
    d_img.reset();
    d_noisy.reset();
    d_features.reset();
    d_motion.reset();
    if (rank == 0) sh.d_slots.reset();
    stream.reset();
    rbrt_hip_scene_destroy(hs);
    hs = nullptr;
}

// ---- the steps of render_scene that are not a rank's --------------------------------------------------------------------------
CheckpointRead resume_from_checkpoint(const Job& job) {
    const std::string& path = job.cfg.checkpoint_path;
    if (path.empty()) return CheckpointRead();
    std::vector<size_t> counts(job.plan.world);
    for (int r = 0; r < job.plan.world; ++r) counts[r] = job.sum_floats(r);
    CheckpointRead res = read_checkpoint(path, job.want, counts);
    if (res.found && !job.cfg.quiet) {
        if (res.samples_done != 0)
            std::printf("Resuming from checkpoint %s at sample %u of %u\n", path.c_str(), res.samples_done, job.num_samples);
        else
            std::printf("Checkpoint %s does not match this render (scene, size, samples, seed or GPU count): starting over\n", path.c_str());
    }
    return res;
}

// The ranks' tiles were merged on the host: the complete image goes up to rank 0's device once, so that the target file
// does not depend on how many GPUs rendered it or on how their tiles were gathered. On the null stream.
void display_after_host_gather(const Job& job, RenderReport& rep) {
    const int dev = job.plan.device_of(0);
    FirstError err;
    DeviceBuffer d_src, d_out8;
    if (err.ok(hipSetDevice(dev), "hipSetDevice") && d_src.alloc(job.n() * sizeof(float), err, "hipMalloc(image)") &&
        d_out8.alloc(job.n(), err, "hipMalloc(rgb8)") &&
        err.ok(hipMemcpy(d_src.as<float>(), job.img.radiance.data(), job.n() * sizeof(float), hipMemcpyHostToDevice), "upload of the gathered image"))
        display(job.cfg, DisplaySite{dev, nullptr, job.img.width, job.img.height, d_out8.as<uint8_t>()}, d_src.as<float>(), nullptr, job.img, rep, err);
    if (err.failed()) throw Error("GPU " + std::to_string(dev) + ": " + err.message());
}

// The report's times: each region is its slowest rank's; the set-up is split into the parts of ONE rank, so that they add up.
void report_times(const Plan& plan, const Shared& sh, RenderReport& rep) {
    const size_t slow = size_t(std::max_element(sh.t_setup.begin(), sh.t_setup.end()) - sh.t_setup.begin());
    const rbrt_hip_call_times_t& ct = sh.t_create[slow];
    rep.upload_build_s = sh.t_setup[slow];
    rep.hip_init_s = plan.hip_start_s + ct.hip_init_s, rep.upload_s = ct.upload_s, rep.bvh_build_s = ct.bvh_build_s;
    rep.lanes_s = ct.lanes_s + std::max(0.0, ct.create_s - ct.hip_init_s - ct.upload_s - ct.bvh_build_s - ct.lanes_s);
    rep.buffers_s = std::max(0.0, sh.t_setup[slow] - ct.create_s);
    rep.release_s = *std::max_element(sh.t_release.begin(), sh.t_release.end());
    rep.render_s = *std::max_element(sh.t_render.begin(), sh.t_render.end());
    rep.gather_s = *std::max_element(sh.t_gather.begin(), sh.t_gather.end());
}

}  // namespace

ImageBuffer render_scene(const Camera& cam, uint32_t num_samples, const Scene& scene, const RenderConfig& cfg_in) {
    RenderConfig cfg = cfg_in;
    if ((cfg.denoise || cfg.denoise_guided || cfg.frames || cfg.upscale || cfg.despike) && !cfg.adaptive)  // (the filter's input is the adaptive path's sums: one round that stops nothing)
        cfg.adaptive = true, cfg.adaptive_threshold = 0.0f, cfg.adaptive_min_samples = cfg.adaptive_step = std::max(num_samples, 2u);
    if (!cfg.quiet) std::printf("Starting rendering...\n");
    ImageBuffer img;
    img.width = cam.img_width_pix;
    img.height = cam.img_height_pix;
    img.rgb.assign(size_t(img.width) * img.height * 3, 0);
    img.radiance.assign(img.rgb.size(), 0.0f);

    // ---- plan, job, resume, communicators --------------------------------------------------------------------------------
    const rbrt_camera_lens_t lens = cam.to_abi_lens();
    const Scene::AbiView view = scene.to_abi();
    const rbrt_environment_t env_abi = scene.environment.to_abi();
    const Plan plan = make_plan(cfg, cfg_in.adaptive ? "--adaptive" : cfg_in.upscale ? "--upscale" : cfg_in.despike ? "--despike" : cfg_in.frames ? "--frames" : cfg_in.denoise_guided ? "--denoise-guided" : "--denoise", cfg_in.adaptive,
                                cam, scene, num_samples);
    Job job{cfg, plan, lens, view, scene.environment.n != 0u ? &env_abi : nullptr, render_opts_of(cfg, cam, num_samples), num_samples, {}, {}, img, {}, {}};
    if (!cfg.no_motion) job.motion = scene.motion_travels(), job.mesh_motion = scene.mesh_motion_travels();
    job.want = checkpoint_header(img.width, img.height, num_samples, uint32_t(plan.world), cfg.seed,
                                 checkpoint_fingerprint(cfg.checkpoint_path, lens, job.opts, view.scene, view.shading_ptr(), scene.environment, view.patterns_ptr(),
                                                        cfg.shutter ? cfg.shutter_travel : nullptr, &job.motion, cfg.motion_step, &job.mesh_motion));
    job.resume = resume_from_checkpoint(job);
    Shared sh(plan);
    bring_up_rccl(plan, sh);
    RenderReport& rep = sh.rep;
    rep.n_gpus = plan.world;
    rep.pass_spp = plan.pass_spp;
    rep.gather = plan.world > 1 ? (sh.use_rccl ? "rccl" : "host") : "none";
    if (!sh.rccl_note.empty()) rep.gather = "host (rccl was asked for: " + sh.rccl_note + ")";

    // ---- the ranks: one thread per GPU, rank 0 on this one ------------------------------------------------------------------
    const auto worker = [&](int rank) { Rank(job, sh, rank).run(); };
    std::vector<std::thread> threads;
    for (int r = 1; r < plan.world; ++r) threads.emplace_back(worker, r);
    worker(0);
    for (auto& t : threads) t.join();

    // ---- what the ranks left --------------------------------------------------------------------------------------------------
    for (ncclComm_t cm : sh.comms)
        if (cm) (void)sh.rccl->CommDestroy(cm);
    if (sh.rccl_failed.load() != 0) {
        std::fprintf(stderr, "warning: %s; gathered through host memory instead\n", sh.rccl_note.c_str());
        rep.gather = "host (rccl was asked for: " + sh.rccl_note + ")";
    }
    for (int r = 0; r < plan.world; ++r)
        if (sh.errors[r].failed())
            throw Error("GPU " + std::to_string(plan.device_of(r)) + (cfg.oversubscribe ? " (rank " + std::to_string(r) + ")" : "") + ": " + sh.errors[r].message());
    if (!cfg.checkpoint_path.empty()) std::remove(cfg.checkpoint_path.c_str());  // (only reached when the render is complete)
    if ((cfg.tonemap || cfg.glare) && !sh.displayed) display_after_host_gather(job, rep);
    if (!cfg.quiet) std::printf("\rRendering 100%% complete!\n");
    rep.resumed_from_sample = job.resume.samples_done;
    report_times(plan, sh, rep);
    if (cfg.report) *cfg.report = rep;
    return img;
}

// rbrt_hip_compare_images on the image's linear radiance and a reference of its size, on device 0: both are uploaded, the stage
// runs between two events on a stream of this call's making, and the result, the means and the maps that were asked for come
// back. Every device object is this call's own and ends with it.
ImageComparison compare_images(const ImageBuffer& img, const PfmImage& ref, float epsilon, bool want_rel_map, bool want_ssim_map) {
    if (img.width == 0u || img.height == 0u || img.radiance.size() != size_t(img.width) * img.height * 3u) throw Error("compare: the image holds no radiance");
    if (ref.width != img.width || ref.height != img.height || ref.rgb.size() != img.radiance.size())
        throw Error("compare: the reference is " + std::to_string(ref.width) + " x " + std::to_string(ref.height) + ", the image " + std::to_string(img.width) + " x " +
                    std::to_string(img.height));
    if (!std::isfinite(epsilon) || !(epsilon > 0.0f)) throw Error("--compare-epsilon must be finite and above 0");
    rbrt_compare_opts_t o;
    rbrt_compare_opts_default(&o);
    o.epsilon = epsilon;
    const size_t n_pixels = size_t(img.width) * img.height, image_bytes = n_pixels * 3u * sizeof(float), map_bytes = n_pixels * sizeof(float);
    ImageComparison out;
    out.width = img.width, out.height = img.height;
    FirstError err;
    Stream stream;
    EventTimer timer;
    DeviceBuffer d_x, d_ref, d_ws, d_rel, d_ssim, d_result;
    float ms = 0.0f;
    if (err.ok(hipSetDevice(0), "hipSetDevice") && stream.create(err) && timer.create(err) && d_x.alloc(image_bytes, err, "hipMalloc(compared image)") &&
        d_ref.alloc(image_bytes, err, "hipMalloc(reference image)") &&
        d_ws.alloc(rbrt_hip_compare_workspace_bytes(img.width, img.height), err, "hipMalloc(compare workspace)") &&
        d_result.alloc(sizeof(rbrt_compare_result_t), err, "hipMalloc(compare result)") && (!want_rel_map || d_rel.alloc(map_bytes, err, "hipMalloc(error map)")) &&
        (!want_ssim_map || d_ssim.alloc(map_bytes, err, "hipMalloc(ssim map)")) &&
        err.ok(hipMemcpyAsync(d_x.as<void>(), img.radiance.data(), image_bytes, hipMemcpyHostToDevice, stream.get()), "upload of the image") &&
        err.ok(hipMemcpyAsync(d_ref.as<void>(), ref.rgb.data(), image_bytes, hipMemcpyHostToDevice, stream.get()), "upload of the reference")) {
        timer.start(stream.get(), err);
        err.lib_ok(rbrt_hip_compare_images(0, stream.get(), d_x.as<float>(), d_ref.as<float>(), img.width, img.height, &o, d_ws.as<void>(), d_rel.as<float>(),
                                           d_ssim.as<float>(), d_result.as<rbrt_compare_result_t>()));
        timer.stop(stream.get(), err);
        if (!err.failed()) err.ok(hipStreamSynchronize(stream.get()), "hipStreamSynchronize(compare)");
        if (timer.elapsed(&ms, err)) out.ms = double(ms);
        if (!err.failed()) err.ok(hipMemcpy(&out.result, d_result.as<void>(), sizeof(out.result), hipMemcpyDeviceToHost), "download of the comparison");
        if (want_rel_map && !err.failed()) {
            out.rel_map.resize(n_pixels);
            err.ok(hipMemcpy(out.rel_map.data(), d_rel.as<void>(), map_bytes, hipMemcpyDeviceToHost), "download of the error map");
        }
        if (want_ssim_map && !err.failed()) {
            out.ssim_map.resize(n_pixels);
            err.ok(hipMemcpy(out.ssim_map.data(), d_ssim.as<void>(), map_bytes, hipMemcpyDeviceToHost), "download of the ssim map");
        }
    }
    if (err.failed()) throw Error("compare: " + err.message());
    rbrt_compare_summary(&out.result, img.width, img.height, 1.0, &out.summary);
    return out;
}

}  // namespace rbrt
