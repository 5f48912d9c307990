// frame_stages.cpp — the image stages of the frame pipeline in the C ABI of include/rbrt_hip.h: denoise, guided denoise, temporal
// accumulation, guided upsampling, spike removal, image comparison, display transform and glare. Each takes a device index, a
// stream and the caller's pointers; none needs a scene handle (the two calls that denoise a handle's last adaptive render are in
// api.cpp). Every call checks its arguments first, in the order written here, then takes the device (ensure_device), and only
// then returns early when no output was asked for. Host C++ only, compiled with -ffp-contract=off like api.cpp: the constants
// of the rules are computed here in float, one operation a statement.
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>

#include "api_common.h"

using namespace rbrt;

namespace {

template <class Params>
Params zeroed() {  // a kernel's parameter block with every field, and the padding, 0
    Params p;
    std::memset(&p, 0, sizeof(p));
    return p;
}

template <size_t N>
bool all_zero(const uint32_t (&reserved)[N]) {
    for (const uint32_t r : reserved)
        if (r != 0u) return false;
    return true;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16u == 0u; }
bool positive_finite(float x) { return std::isfinite(x) && x > 0.0f; }

}  // namespace

extern "C" {

// ---- Denoising (the rule: include/rbrt_hip.h; the kernels: denoise.hip) ----------------------------------------------------
void rbrt_denoise_opts_default(rbrt_denoise_opts_t* o) {
    if (!o) return;
    o->window_radius = 5, o->patch_radius = 3, o->strength = 0.7f, o->reserved = 0;
}

}  // extern "C"

int rbrt::check_denoise_opts(const rbrt_denoise_opts_t* d) {
    if (d->reserved != 0u) return fail(RBRT_ERR_INVALID_ARG, "denoise: reserved must be 0");
    if (d->window_radius > 10u) return fail(RBRT_ERR_INVALID_ARG, "denoise: window_radius must be 0..10");
    if (d->patch_radius > 4u) return fail(RBRT_ERR_INVALID_ARG, "denoise: patch_radius must be 0..4");
    if (!positive_finite(d->strength)) return fail(RBRT_ERR_INVALID_ARG, "denoise: strength must be finite and > 0");
    return RBRT_OK;
}

DenoiseParams rbrt::denoise_params(const float* a, const float* b, const float* wa, uint32_t width, uint32_t height,
                                   const rbrt_denoise_opts_t* d, float* d_radiance, uint8_t* d_rgb8) {
    DenoiseParams D = zeroed<DenoiseParams>();
    D.a = a, D.b = b, D.wa = wa, D.width = width, D.height = height;
    D.window_radius = int32_t(d->window_radius), D.patch_radius = int32_t(d->patch_radius), D.k2 = d->strength * d->strength;
    D.out_radiance = d_radiance, D.out_rgb8 = d_rgb8;
    return D;
}

extern "C" {

int rbrt_hip_denoise_halves(int device, void* stream, const float* d_a, const float* d_b, const float* d_wa, uint32_t width,
                            uint32_t height, const rbrt_denoise_opts_t* d, float* d_radiance, uint8_t* d_rgb8) {
    if (!d_a || !d_b || !d) return fail(RBRT_ERR_INVALID_ARG, "denoise_halves: null argument");
    if (int rc = check_denoise_opts(d)) return rc;
    if (width == 0 || height == 0) return fail(RBRT_ERR_INVALID_ARG, "denoise_halves: width and height must be >= 1");
    // (the one refusal of a stage without the call's name in front: the text is part of the ABI and stays)
    if (uint64_t(width) * height >= (1ull << 32)) return fail(RBRT_ERR_UNSUPPORTED, "image has 2^32 or more pixels");
    if (int rc = ensure_device(device)) return rc;
    if (!d_radiance && !d_rgb8) return RBRT_OK;
    HIP_TRY(launch_denoise(denoise_params(d_a, d_b, d_wa, width, height, d, d_radiance, d_rgb8), static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

// ---- Guided denoising (the rule: include/rbrt_hip.h; the kernels: guided.hip) ------------------------------------------------
void rbrt_guided_opts_default(rbrt_guided_opts_t* o) {
    if (!o) return;
    o->levels = 5u, o->colour = 2.0f, o->normal = 0.35f, o->depth = 0.05f, o->albedo = 0.1f, o->flags = 0u;
    o->reserved[0] = o->reserved[1] = 0u;
}

// The levels whose step is at most this stage their tile in LDS; the others read global memory (profiles/guided_config2.txt
// has the comparison). rbrt_hip_debug_guided_staging changes it for the process.
static std::atomic<uint32_t> g_guided_staged_max_step{RBRT_GUIDED_STAGED_MAX_STEP};

int rbrt_hip_debug_guided_staging(int max_step) {
    if (max_step < -1 || max_step > 4) return fail(RBRT_ERR_INVALID_ARG, "debug_guided_staging: max_step must be -1 (ask) or 0..4");
    if (max_step >= 0) g_guided_staged_max_step.store(uint32_t(max_step));
    return int(g_guided_staged_max_step.load());
}

size_t rbrt_hip_guided_workspace_bytes(uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u || uint64_t(width) * height >= (1ull << 31)) return 0;
    return size_t(width) * height * 96u;  // (the layout of launch_guided: six planes of one float4 a pixel)
}

}  // extern "C"

uint32_t rbrt::guided_staged_max_step() { return g_guided_staged_max_step.load(); }

int rbrt::check_guided_args(const rbrt_guided_opts_t* g, const float* d_albedo, const float* d_normal, const float* d_depth,
                            const float* d_coverage, const void* d_workspace) {
    if (!g || !d_albedo || !d_normal || !d_depth || !d_coverage || !d_workspace) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: null argument");
    if (g->levels == 0u || g->levels > RBRT_GUIDED_MAX_LEVELS) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: levels must be 1..6");
    for (const float k : {g->colour, g->normal, g->depth, g->albedo})
        if (!positive_finite(k)) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: colour, normal, depth and albedo must be finite and > 0");
    if (g->flags & ~RBRT_GUIDED_NO_DEMODULATION) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: unknown flag bit");
    if (!all_zero(g->reserved)) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: reserved must be 0");
    if (!aligned16(d_workspace)) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: the workspace must be 16-byte aligned");
    return RBRT_OK;
}

GuidedParams rbrt::guided_params(const float* a, const float* b, const float* wa, const float* d_albedo, const float* d_normal,
                                 const float* d_depth, const float* d_coverage, uint32_t width, uint32_t height,
                                 const rbrt_guided_opts_t* g, void* d_workspace, float* d_radiance, uint8_t* d_rgb8) {
    GuidedParams G = zeroed<GuidedParams>();
    G.a = a, G.b = b, G.wa = wa, G.albedo = d_albedo, G.normal = d_normal, G.depth = d_depth, G.coverage = d_coverage;
    G.width = width, G.height = height, G.levels = g->levels, G.flags = g->flags;
    // the rule's host-side values, in float, one operation a statement (this file is compiled with -ffp-contract=off)
    const float kn2 = g->normal * g->normal, ka2 = g->albedo * g->albedo;
    G.kc2 = g->colour * g->colour, G.kz2 = g->depth * g->depth;
    G.in = 1.0f / kn2, G.ia = 1.0f / ka2;
    G.workspace = d_workspace, G.out_radiance = d_radiance, G.out_rgb8 = d_rgb8;
    return G;
}

extern "C" {

int rbrt_hip_denoise_guided(int device, void* stream, const float* d_a, const float* d_b, const float* d_wa, const float* d_albedo,
                            const float* d_normal, const float* d_depth, const float* d_coverage, uint32_t width, uint32_t height,
                            const rbrt_guided_opts_t* g, void* d_workspace, float* d_radiance, uint8_t* d_rgb8) {
    if (!d_a || !d_b) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: null argument");
    if (int rc = check_guided_args(g, d_albedo, d_normal, d_depth, d_coverage, d_workspace)) return rc;
    if (width == 0u || height == 0u) return fail(RBRT_ERR_INVALID_ARG, "denoise_guided: width and height must be >= 1");
    if (uint64_t(width) * height >= (1ull << 31)) return fail(RBRT_ERR_UNSUPPORTED, "denoise_guided: 2^31 or more pixels");
    if (int rc = ensure_device(device)) return rc;
    if (!d_radiance && !d_rgb8) return RBRT_OK;
    HIP_TRY(launch_guided(guided_params(d_a, d_b, d_wa, d_albedo, d_normal, d_depth, d_coverage, width, height, g, d_workspace, d_radiance, d_rgb8),
                          guided_staged_max_step(), static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

// ---- Temporal accumulation (the rule: include/rbrt_hip.h; the kernel: temporal.hip) -----------------------------------------
void rbrt_temporal_opts_default(rbrt_temporal_opts_t* o) {
    if (!o) return;
    o->max_history = 32.0f, o->depth = 0.05f, o->normal = 0.35f, o->flags = 0u;
    for (uint32_t& r : o->reserved) r = 0u;
}

size_t rbrt_hip_temporal_history_bytes(uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u || uint64_t(width) * height >= (1ull << 31)) return 0;
    return size_t(width) * height * 48u;  // (the layout of temporal.hip: three planes of one float4 a pixel)
}

static float dot3(const float* a, const float* b) {  // the rule's dot, one operation a statement
    const float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    const float xy = x + y;
    return xy + z;
}

int rbrt_hip_temporal_accumulate(int device, void* stream, const float* d_a, const float* d_b, const float* d_normal,
                                 const float* d_depth, const float* d_coverage, const rbrt_camera_t* cam, const rbrt_camera_t* prev,
                                 const rbrt_temporal_opts_t* o, const void* d_history_in, void* d_history_out, float* d_out_a,
                                 float* d_out_b, float* d_out_length) {
    return rbrt_hip_temporal_accumulate_moving(device, stream, d_a, d_b, d_normal, d_depth, d_coverage, nullptr, 0.0f, cam, prev, o, d_history_in,
                                               d_history_out, d_out_a, d_out_b, d_out_length);
}

// (d_motion NULL: the plain rule and the kernel's build that has always run it; phase_step is then not read)
int rbrt_hip_temporal_accumulate_moving(int device, void* stream, const float* d_a, const float* d_b, const float* d_normal,
                                        const float* d_depth, const float* d_coverage, const float* d_motion, float phase_step,
                                        const rbrt_camera_t* cam, const rbrt_camera_t* prev, const rbrt_temporal_opts_t* o,
                                        const void* d_history_in, void* d_history_out, float* d_out_a, float* d_out_b, float* d_out_length) {
    if (!d_a || !d_b || !d_normal || !d_depth || !d_coverage || !cam || !o) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: null argument");
    if (d_history_in && !prev) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: a history needs cam_prev");
    if (d_history_in && d_history_in == d_history_out)
        return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: d_history_in and d_history_out must differ (keep two and alternate)");
    if (!aligned16(d_history_in) || !aligned16(d_history_out)) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: a history must be 16-byte aligned");
    const uint32_t width = cam->img_width_pix, height = cam->img_height_pix;
    if (width == 0u || height == 0u) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: width and height must be >= 1");
    if (d_history_in && (prev->img_width_pix != width || prev->img_height_pix != height))
        return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: cam_prev's image size differs from cam's");
    if (!std::isfinite(o->max_history) || !(o->max_history >= 1.0f)) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: max_history must be finite and >= 1");
    for (const float k : {o->depth, o->normal})
        if (!std::isfinite(k) || !(k >= 0.0f)) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: depth and normal must be finite and >= 0");
    if (o->flags != 0u) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: unknown flag bit");
    if (!all_zero(o->reserved)) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: reserved must be 0");
    if (!positive_finite(cam->mm_per_pix_hor) || !positive_finite(cam->mm_per_pix_vert))
        return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: cam's mm_per_pix must be finite and > 0");
    if (d_motion && !std::isfinite(phase_step)) return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate_moving: phase_step is not finite");

    TemporalParams T = zeroed<TemporalParams>();
    T.a = d_a, T.b = d_b, T.normal = d_normal, T.depth = d_depth, T.coverage = d_coverage;
    T.history_in = d_history_in, T.history_out = d_history_out, T.out_a = d_out_a, T.out_b = d_out_b, T.out_length = d_out_length;
    if (d_motion) T.motion = d_motion, T.phase_step = phase_step;
    T.width = width, T.height = height;
    T.max_history = o->max_history, T.kz = o->depth, T.kn2 = o->normal * o->normal;
    for (int k = 0; k < 3; ++k)
        T.pos[k] = cam->position[k], T.right[k] = cam->right[k], T.up[k] = cam->up[k], T.center[k] = cam->img_center_point[k];
    T.mm_hor = cam->mm_per_pix_hor, T.mm_vert = cam->mm_per_pix_vert;
    T.hx = float(width / 2u), T.hy = float(height / 2u);
    if (d_history_in) {
        if (!positive_finite(prev->mm_per_pix_hor) || !positive_finite(prev->mm_per_pix_vert))
            return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: cam_prev's mm_per_pix must be finite and > 0");
        // the rule's constants of K', in float, one operation a statement (this file is compiled with -ffp-contract=off)
        const float* r = prev->right;
        const float* u = prev->up;
        for (int k = 0; k < 3; ++k) {
            const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            const float m0 = r[k1] * u[k2], m1 = r[k2] * u[k1];
            T.n[k] = m0 - m1;
            T.w[k] = prev->img_center_point[k] - prev->position[k];
            T.pos_prev[k] = prev->position[k], T.right_prev[k] = r[k], T.up_prev[k] = u[k];
        }
        T.wn = dot3(T.w, T.n);
        T.rr = dot3(r, r), T.uu = dot3(u, u), T.ru = dot3(r, u);
        const float d0 = T.rr * T.uu, d1 = T.ru * T.ru;
        T.det = d0 - d1;
        T.sx = 0.001f * prev->mm_per_pix_hor, T.sy = 0.001f * prev->mm_per_pix_vert;
        if (!std::isfinite(T.det) || T.det == 0.0f || !std::isfinite(T.wn) || T.wn == 0.0f)
            return fail(RBRT_ERR_INVALID_ARG, "temporal_accumulate: cam_prev is degenerate (right x up, or its distance to the image plane, is 0 or not finite)");
    }
    if (uint64_t(width) * height >= (1ull << 31)) return fail(RBRT_ERR_UNSUPPORTED, "temporal_accumulate: 2^31 or more pixels");
    if (int rc = ensure_device(device)) return rc;
    if (!d_history_out && !d_out_a && !d_out_b && !d_out_length) return RBRT_OK;
    HIP_TRY(launch_temporal(T, static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

// ---- Guided upsampling (the rule: include/rbrt_hip.h; the kernels: upsample.hip) ----------------------------------------------
void rbrt_upsample_opts_default(rbrt_upsample_opts_t* o) {
    if (!o) return;
    o->factor = 2u, o->normal = 0.5f, o->depth = 0.1f, o->albedo = 0.2f, o->flags = 0u;
    for (uint32_t& r : o->reserved) r = 0u;
}

int rbrt_hip_upsample_camera(const rbrt_camera_t* full, uint32_t factor, rbrt_camera_t* low) {
    if (!full || !low) return fail(RBRT_ERR_INVALID_ARG, "upsample_camera: null argument");
    if (factor == 0u || factor > RBRT_UPSAMPLE_MAX_FACTOR) return fail(RBRT_ERR_INVALID_ARG, "upsample_camera: factor must be 1..4");
    const uint32_t W = full->img_width_pix, H = full->img_height_pix;
    if (W == 0u || H == 0u) return fail(RBRT_ERR_INVALID_ARG, "upsample_camera: width and height must be >= 1");
    if (!std::isfinite(full->mm_per_pix_hor) || !std::isfinite(full->mm_per_pix_vert))
        return fail(RBRT_ERR_INVALID_ARG, "upsample_camera: mm_per_pix must be finite");
    const uint32_t f = factor;
    const uint32_t w = uint32_t((uint64_t(W) + f - 1u) / f), h = uint32_t((uint64_t(H) + f - 1u) / f);
    // the rule's shift, in float, one operation a statement (this file is compiled with -ffp-contract=off)
    const float half = 0.5f * float(f - 1u);
    const float dx = float(f * (w / 2u)) - float(W / 2u), dy = float(f * (h / 2u)) - float(H / 2u);
    const float kx = dx + half, ky = dy + half;
    const float mx = kx * full->mm_per_pix_hor, my = ky * full->mm_per_pix_vert;
    const float sx = 0.001f * mx, sy = 0.001f * my;
    rbrt_camera_t out = *full;
    for (int k = 0; k < 3; ++k) {
        const float r = sx * full->right[k], u = sy * full->up[k];
        const float cr = full->img_center_point[k] + r;
        out.img_center_point[k] = cr - u;
    }
    out.mm_per_pix_hor = float(f) * full->mm_per_pix_hor, out.mm_per_pix_vert = float(f) * full->mm_per_pix_vert;
    out.img_width_pix = w, out.img_height_pix = h;
    *low = out;
    return RBRT_OK;
}

size_t rbrt_hip_upsample_workspace_bytes(uint32_t width, uint32_t height, uint32_t factor) {
    if (width == 0u || height == 0u || factor == 0u || factor > RBRT_UPSAMPLE_MAX_FACTOR || uint64_t(width) * height >= (1ull << 31)) return 0;
    const size_t w = (size_t(width) + factor - 1u) / factor, h = (size_t(height) + factor - 1u) / factor;
    return w * h * 64u;  // (the layout of upsample.hip: four planes of one float4 a low pixel)
}

int rbrt_hip_upsample_halves(int device, void* stream, const float* d_a, const float* d_b, const float* d_wa, const float* d_albedo,
                             const float* d_normal, const float* d_depth, const float* d_coverage, uint32_t width, uint32_t height,
                             const rbrt_upsample_opts_t* o, void* d_workspace, float* d_out_a, float* d_out_b, float* d_out_wa) {
    if (!d_a || !d_b || !d_albedo || !d_normal || !d_depth || !d_coverage || !o || !d_workspace)
        return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: null argument");
    if (width == 0u || height == 0u) return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: width and height must be >= 1");
    if (o->factor == 0u || o->factor > RBRT_UPSAMPLE_MAX_FACTOR) return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: factor must be 1..4");
    for (const float k : {o->normal, o->depth, o->albedo})
        if (!positive_finite(k)) return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: normal, depth and albedo must be finite and > 0");
    if ((o->flags & ~RBRT_UPSAMPLE_NO_DEMODULATION) != 0u) return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: unknown flag bit");
    if (!all_zero(o->reserved)) return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: reserved must be 0");
    if (!aligned16(d_workspace)) return fail(RBRT_ERR_INVALID_ARG, "upsample_halves: the workspace must be 16-byte aligned");
    if (uint64_t(width) * height >= (1ull << 31)) return fail(RBRT_ERR_UNSUPPORTED, "upsample_halves: 2^31 or more pixels");

    UpsampleParams U = zeroed<UpsampleParams>();
    U.a = d_a, U.b = d_b, U.wa = d_wa, U.albedo = d_albedo, U.normal = d_normal, U.depth = d_depth, U.coverage = d_coverage;
    U.workspace = d_workspace, U.out_a = d_out_a, U.out_b = d_out_b, U.out_wa = d_out_wa;
    U.width = width, U.height = height, U.factor = o->factor, U.flags = o->flags;
    U.low_width = (width + o->factor - 1u) / o->factor, U.low_height = (height + o->factor - 1u) / o->factor;
    // the rule's constants, in float, one operation a statement
    const float kn2 = o->normal * o->normal, ka2 = o->albedo * o->albedo;
    U.in = 1.0f / kn2, U.ia = 1.0f / ka2, U.kz2 = o->depth * o->depth, U.invf = 1.0f / float(o->factor);
    if (int rc = ensure_device(device)) return rc;
    if (!d_out_a && !d_out_b && !d_out_wa) return RBRT_OK;
    HIP_TRY(launch_upsample(U, static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

// ---- Spike removal (the rule: include/rbrt_hip.h; the kernel: despike.hip) -----------------------------------------------------
void rbrt_despike_opts_default(rbrt_despike_opts_t* o) {
    if (!o) return;
    o->radius = 2u, o->rank = 2u, o->threshold = 4.0f, o->floor = 0.01f, o->flags = 0u;
    for (uint32_t& r : o->reserved) r = 0u;
}

int rbrt_hip_despike_halves(int device, void* stream, const float* d_a, const float* d_b, uint32_t width, uint32_t height,
                            const rbrt_despike_opts_t* o, float* d_out_a, float* d_out_b, uint8_t* d_mask, rbrt_despike_result_t* d_result) {
    if (!d_a || !d_b || !o) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: null argument");
    if (width == 0u || height == 0u) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: width and height must be >= 1");
    if (o->radius == 0u || o->radius > RBRT_DESPIKE_MAX_RADIUS) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: radius must be 1..2");
    if (o->rank == 0u || o->rank > RBRT_DESPIKE_MAX_RANK) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: rank must be 1..4");
    if (!std::isfinite(o->threshold) || !(o->threshold >= 1.0f)) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: threshold must be finite and >= 1");
    if (!std::isfinite(o->floor) || !(o->floor >= 0.0f)) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: floor must be finite and >= 0");
    if (o->flags != 0u) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: unknown flag bit");
    if (!all_zero(o->reserved)) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: reserved must be 0");
    for (const void* out : {static_cast<const void*>(d_out_a), static_cast<const void*>(d_out_b), static_cast<const void*>(d_mask),
                            static_cast<const void*>(d_result)})
        if (out && (out == d_a || out == d_b)) return fail(RBRT_ERR_INVALID_ARG, "despike_halves: an output must not be an input");
    if (uint64_t(width) * height >= (1ull << 31)) return fail(RBRT_ERR_UNSUPPORTED, "despike_halves: 2^31 or more pixels");

    DespikeParams D = zeroed<DespikeParams>();
    D.a = d_a, D.b = d_b, D.out_a = d_out_a, D.out_b = d_out_b, D.mask = d_mask, D.counts = reinterpret_cast<uint32_t*>(d_result);
    D.width = width, D.height = height, D.radius = o->radius, D.rank = o->rank, D.threshold = o->threshold, D.floor = o->floor;
    if (int rc = ensure_device(device)) return rc;
    if (!d_out_a && !d_out_b && !d_mask && !d_result) return RBRT_OK;
    HIP_TRY(launch_despike(D, static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

// ---- Image comparison (the rule: include/rbrt_hip.h; the kernels: compare.hip) -------------------------------------------------
void rbrt_compare_opts_default(rbrt_compare_opts_t* o) {
    if (!o) return;
    o->epsilon = 0.01f, o->flags = 0u;
    for (uint32_t& r : o->reserved) r = 0u;
}

static uint64_t compare_tiles(uint32_t width, uint32_t height) {
    return uint64_t((width + RBRT_COMPARE_TILE_W - 1u) / RBRT_COMPARE_TILE_W) * ((height + RBRT_COMPARE_TILE_H - 1u) / RBRT_COMPARE_TILE_H);
}

size_t rbrt_hip_compare_workspace_bytes(uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u || uint64_t(width) * height >= (1ull << 31)) return 0;
    return size_t(compare_tiles(width, height)) * sizeof(CompareTilePartial);
}

int rbrt_hip_compare_images(int device, void* stream, const float* d_x, const float* d_ref, uint32_t width, uint32_t height,
                            const rbrt_compare_opts_t* o, void* d_workspace, float* d_rel_map, float* d_ssim_map, rbrt_compare_result_t* d_result) {
    if (!d_x || !d_ref || !o) return fail(RBRT_ERR_INVALID_ARG, "compare_images: null argument");
    if (d_result && !d_workspace) return fail(RBRT_ERR_INVALID_ARG, "compare_images: a result needs a workspace (null argument)");
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 7u) != 0u || (reinterpret_cast<uintptr_t>(d_result) & 7u) != 0u)
        return fail(RBRT_ERR_INVALID_ARG, "compare_images: the workspace and the result must be 8-byte aligned");
    if (width == 0u || height == 0u) return fail(RBRT_ERR_INVALID_ARG, "compare_images: width and height must be >= 1");
    if (!positive_finite(o->epsilon)) return fail(RBRT_ERR_INVALID_ARG, "compare_images: epsilon must be finite and above 0");
    if (o->flags != 0u) return fail(RBRT_ERR_INVALID_ARG, "compare_images: unknown flag bit");
    if (!all_zero(o->reserved)) return fail(RBRT_ERR_INVALID_ARG, "compare_images: reserved must be 0");
    const void* const outs[4] = {d_rel_map, d_ssim_map, d_result, d_result ? d_workspace : nullptr};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        if (outs[i] == d_x || outs[i] == d_ref) return fail(RBRT_ERR_INVALID_ARG, "compare_images: an output must not be an input");
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return fail(RBRT_ERR_INVALID_ARG, "compare_images: an output must not be another output");
    }
    if (uint64_t(width) * height >= (1ull << 31)) return fail(RBRT_ERR_UNSUPPORTED, "compare_images: 2^31 or more pixels");

    CompareParams P = zeroed<CompareParams>();
    P.x = d_x, P.ref = d_ref, P.rel_map = d_rel_map, P.ssim_map = d_ssim_map;
    P.partials = d_result ? static_cast<CompareTilePartial*>(d_workspace) : nullptr, P.result = d_result;
    P.width = width, P.height = height, P.epsilon = o->epsilon;
    P.tiles_x = (width + RBRT_COMPARE_TILE_W - 1u) / RBRT_COMPARE_TILE_W, P.tiles = uint32_t(compare_tiles(width, height));
    if (int rc = ensure_device(device)) return rc;
    if (!d_rel_map && !d_ssim_map && !d_result) return RBRT_OK;
    HIP_TRY(launch_compare(P, static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

void rbrt_compare_summary(const rbrt_compare_result_t* r, uint32_t width, uint32_t height, double peak, rbrt_compare_summary_t* out) {
    if (!out) return;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out->mse = out->mae = out->relmse = out->psnr_db = out->ssim = nan;
    if (!r || r->usable == 0u) return;
    const double n = 3.0 * double(r->usable);
    out->mse = r->sum_se / n, out->mae = r->sum_ae / n, out->relmse = r->sum_rel / n;
    out->ssim = r->sum_ssim / (double(width) * double(height));
    out->psnr_db = 10.0 * std::log10((peak * peak) / out->mse);
}

// ---- Display transform (the rule: include/rbrt_hip.h; the kernels: tonemap.hip) ----------------------------------------------
void rbrt_tonemap_opts_default(rbrt_tonemap_opts_t* o) {
    if (!o) return;
    o->curve = RBRT_TONE_LINEAR, o->exposure = 1.0f, o->key = 0.18f, o->key_permille = 500u;
    o->white = 0.0f, o->white_permille = 990u, o->reserved[0] = o->reserved[1] = 0u;
}

int rbrt_hip_tonemap(int device, void* stream, const float* d_radiance, size_t n_pixels, const rbrt_tonemap_opts_t* o,
                     void* d_workspace, float* d_out_radiance, uint8_t* d_rgb8) {
    if (!d_radiance || !o) return fail(RBRT_ERR_INVALID_ARG, "tonemap: null argument");
    if (n_pixels == 0) return fail(RBRT_ERR_INVALID_ARG, "tonemap: n_pixels must be >= 1");
    if (o->curve > RBRT_TONE_ACES) return fail(RBRT_ERR_INVALID_ARG, "tonemap: unknown curve");
    if (!all_zero(o->reserved)) return fail(RBRT_ERR_INVALID_ARG, "tonemap: reserved must be 0");
    if (!std::isfinite(o->exposure) || !std::isfinite(o->key) || !std::isfinite(o->white))
        return fail(RBRT_ERR_INVALID_ARG, "tonemap: exposure, key and white must be finite");
    if (o->exposure < 0.0f || o->white < 0.0f) return fail(RBRT_ERR_INVALID_ARG, "tonemap: exposure and white must be >= 0");
    const bool automatic = o->exposure == 0.0f || o->white == 0.0f;
    if (o->exposure == 0.0f && !(o->key > 0.0f)) return fail(RBRT_ERR_INVALID_ARG, "tonemap: key must be > 0 for automatic exposure");
    if (o->key_permille > 1000u || o->white_permille > 1000u) return fail(RBRT_ERR_INVALID_ARG, "tonemap: a permille must be 0..1000");
    if (automatic && !d_workspace) return fail(RBRT_ERR_INVALID_ARG, "tonemap: automatic exposure or white needs a workspace");
    if (!aligned16(d_workspace)) return fail(RBRT_ERR_INVALID_ARG, "tonemap: the workspace must be 16-byte aligned");
    if (uint64_t(n_pixels) >= (1ull << 32)) return fail(RBRT_ERR_UNSUPPORTED, "tonemap: 2^32 or more pixels (the bins are 32-bit)");
    if (int rc = ensure_device(device)) return rc;
    TonemapParams T = zeroed<TonemapParams>();
    T.in = d_radiance, T.n = uint32_t(n_pixels), T.curve = o->curve;
    T.exposure = o->exposure + 0.0f, T.white = o->white + 0.0f;  // (-0 is 0: automatic)
    T.key = o->key, T.key_permille = o->key_permille, T.white_permille = o->white_permille;
    T.hist = static_cast<uint32_t*>(d_workspace), T.out_radiance = d_out_radiance, T.out_rgb8 = d_rgb8;
    HIP_TRY(launch_tonemap(T, static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

// ---- Glare (the rule: include/rbrt_hip.h; the kernels: glare.hip) -------------------------------------------------------------
void rbrt_glare_opts_default(rbrt_glare_opts_t* o) {
    if (!o) return;
    o->threshold = 1.0f, o->intensity = 0.1f, o->levels = 5u, o->spread = 1.0f;
    o->reserved[0] = o->reserved[1] = o->reserved[2] = o->reserved[3] = 0u;
}

size_t rbrt_hip_glare_workspace_bytes(uint32_t width, uint32_t height, uint32_t levels) {
    if (width == 0u || height == 0u || levels == 0u || levels > RBRT_GLARE_MAX_LEVELS) return 0;
    if (uint64_t(width) * height >= (1ull << 31)) return 0;
    size_t pixels = 0;  // (levels 1..L, the layout of launch_glare: float4 a pixel, level after level)
    uint32_t w = width, h = height;
    for (uint32_t l = 1; l <= levels; ++l) {
        w = (w + 1u) / 2u, h = (h + 1u) / 2u;
        pixels += size_t(w) * h;
    }
    return pixels * 16u;
}

int rbrt_hip_glare(int device, void* stream, const float* d_radiance, uint32_t width, uint32_t height, const rbrt_glare_opts_t* o,
                   void* d_workspace, float* d_out_radiance, uint8_t* d_rgb8) {
    if (!d_radiance || !o || !d_workspace) return fail(RBRT_ERR_INVALID_ARG, "glare: null argument");
    if (width == 0u || height == 0u) return fail(RBRT_ERR_INVALID_ARG, "glare: width and height must be >= 1");
    if (o->levels == 0u || o->levels > RBRT_GLARE_MAX_LEVELS) return fail(RBRT_ERR_INVALID_ARG, "glare: levels must be 1..8");
    if (!all_zero(o->reserved)) return fail(RBRT_ERR_INVALID_ARG, "glare: reserved must be 0");
    if (!std::isfinite(o->threshold) || !std::isfinite(o->intensity) || !std::isfinite(o->spread))
        return fail(RBRT_ERR_INVALID_ARG, "glare: threshold, intensity and spread must be finite");
    if (o->threshold < 0.0f) return fail(RBRT_ERR_INVALID_ARG, "glare: threshold must be >= 0");
    if (!(o->intensity > 0.0f) || o->intensity > 1.0f) return fail(RBRT_ERR_INVALID_ARG, "glare: intensity must be above 0 and at most 1");
    if (o->spread < 0.0f) return fail(RBRT_ERR_INVALID_ARG, "glare: spread must be >= 0");
    if (!aligned16(d_workspace)) return fail(RBRT_ERR_INVALID_ARG, "glare: the workspace must be 16-byte aligned");
    if (uint64_t(width) * height >= (1ull << 31)) return fail(RBRT_ERR_UNSUPPORTED, "glare: 2^31 or more pixels");
    if (int rc = ensure_device(device)) return rc;
    GlareParams G = zeroed<GlareParams>();
    G.in = d_radiance, G.width = width, G.height = height, G.levels = o->levels;
    G.threshold = o->threshold + 0.0f, G.intensity = o->intensity, G.spread = o->spread + 0.0f;  // (-0 is 0)
    // the rule's normalisation, in float, one operation a statement (this file is compiled with -ffp-contract=off)
    float n = 1.0f, p = 1.0f;
    for (uint32_t l = 2; l <= G.levels; ++l) {
        p = p * G.spread;
        n = n + p;
    }
    const float inv = 1.0f / n;
    G.a = G.intensity * inv;
    G.workspace = d_workspace, G.out_radiance = d_out_radiance, G.out_rgb8 = d_rgb8;
    HIP_TRY(launch_glare(G, static_cast<hipStream_t>(stream)));
    return RBRT_OK;
}

}  // extern "C"
