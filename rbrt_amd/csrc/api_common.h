// api_common.h — what the files that implement the C ABI share: api.cpp (everything that needs a scene handle), frame_stages.cpp
// (the image stages of the frame pipeline) and selftests.cpp (the self tests that need no scene). Nothing of the scene handle
// is in here. fail, hip_fail, hook_result and ensure_device are defined once, in api.cpp, in front of the one thread-local
// message that rbrt_hip_last_error() returns.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "device_types.h"
#include "../../include/rbrt_hip_debug.h"

namespace rbrt {

// Launch wrappers of the kernel files that frame_stages.cpp and selftests.cpp call (api.cpp has the prototypes of the others).
hipError_t launch_denoise(const DenoiseParams& D, hipStream_t stream);                 // denoise.hip
hipError_t launch_tonemap(const TonemapParams& T, hipStream_t stream);                 // tonemap.hip
hipError_t launch_glare(const GlareParams& G, hipStream_t stream);                     // glare.hip
hipError_t launch_guided(const GuidedParams& G, uint32_t staged_max_step, hipStream_t stream);  // guided.hip
hipError_t launch_temporal(const TemporalParams& T, hipStream_t stream);                // temporal.hip
hipError_t launch_upsample(const UpsampleParams& U, hipStream_t stream);                // upsample.hip
hipError_t launch_despike(const DespikeParams& D, hipStream_t stream);                  // despike.hip
hipError_t launch_compare(const CompareParams& C, hipStream_t stream);                  // compare.hip
hipError_t launch_gate_selftest(const float* d_box, const float* d_rays, size_t n, uint8_t* d_fast, uint8_t* d_exact);
hipError_t launch_ieee_selftest(uint64_t seed, size_t n, unsigned long long* d_counts);
hipError_t launch_ieee_debug(const float* d_x, size_t n, const float* d_v, size_t m, float* d_sqrt, uint8_t* d_sqrt_short,
                             float* d_norm, uint8_t* d_norm_short);
hipError_t launch_sqrt_sweep(uint32_t first, uint64_t n, unsigned long long* d_counts);

// Sets the calling thread's message (rbrt_hip_last_error) and hands `code` back.
int fail(int code, const std::string& msg);
// A failed HIP call as the ABI reports it: the one place that maps a hipError_t to an error code.
int hip_fail(hipError_t e, const std::string& what);
// What a test hook returns after its chain of HIP calls. `who`: the hook, for the message.
int hook_result(hipError_t e, const char* who);
// Makes `device` the thread's device; refuses an index that is out of range, or a machine without a device.
int ensure_device(int device);

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t _e = (expr);                                \
        if (_e != hipSuccess) return rbrt::hip_fail(_e, #expr); \
    } while (0)

// A hipMalloc'ed array that lives as long as its scope: the temporaries of the builders and of the test hooks.
template <class T>
struct DevBuf {
    T* p = nullptr;
    explicit DevBuf(T* owned = nullptr) : p(owned) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)); }
    T* get() const { return p; }
    hipError_t from_host(const T* h, size_t n) { return hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice); }
    hipError_t upload(const T* h, size_t n) { const hipError_t e = alloc(n); return e != hipSuccess ? e : from_host(h, n); }
    hipError_t to_host(T* h, size_t n) const { return hipMemcpy(h, p, n * sizeof(T), hipMemcpyDeviceToHost); }
};

// The five internals of frame_stages.cpp that rbrt_hip_scene_denoise and rbrt_hip_scene_denoise_guided (api.cpp: they read the
// handle's adaptive state) share with rbrt_hip_denoise_halves and rbrt_hip_denoise_guided.
int check_denoise_opts(const rbrt_denoise_opts_t* d);
DenoiseParams denoise_params(const float* a, const float* b, const float* wa, uint32_t width, uint32_t height,
                             const rbrt_denoise_opts_t* d, float* d_radiance, uint8_t* d_rgb8);
int check_guided_args(const rbrt_guided_opts_t* g, const float* d_albedo, const float* d_normal, const float* d_depth,
                      const float* d_coverage, const void* d_workspace);
GuidedParams guided_params(const float* a, const float* b, const float* wa, const float* d_albedo, const float* d_normal,
                           const float* d_depth, const float* d_coverage, uint32_t width, uint32_t height,
                           const rbrt_guided_opts_t* g, void* d_workspace, float* d_radiance, uint8_t* d_rgb8);
uint32_t guided_staged_max_step();  // the value rbrt_hip_debug_guided_staging set (one for the process)

}  // namespace rbrt
