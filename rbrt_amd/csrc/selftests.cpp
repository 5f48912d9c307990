// selftests.cpp — the test hooks of include/rbrt_hip_debug.h that need no scene: the kernels' box gate and their short forms of
// IEEE sqrt / normalize, run on device 0 on host arrays. (The hooks that take a scene, the scatter hook and the BVH builders'
// hooks are in api.cpp, next to what they share with scene creation.) Host C++ only.
#include <algorithm>

#include "api_common.h"

using namespace rbrt;

namespace {

// The self tests' three counters: zeroed on device 0, filled by `launch`, handed back in counts. `who`: the hook.
template <class Launch>
int device_counts3(const char* who, uint64_t counts[3], Launch launch) {
    if (int rc = ensure_device(0)) return rc;
    DevBuf<unsigned long long> d;
    HIP_TRY(d.alloc(3));
    hipError_t e = hipMemset(d.get(), 0, 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = launch(d.get());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied out as they are");
    if (e == hipSuccess) e = d.to_host(reinterpret_cast<unsigned long long*>(counts), 3);
    return hook_result(e, who);
}

}  // namespace

extern "C" {

// Test hook: BoundingBox::hit (aabbox.rs:28-58) on n rays against one box, by the division-free form the megakernel
// uses (out_fast) and by the verbatim IEEE form (out_exact). Host arrays.
int rbrt_hip_selftest_gate(const float lo[3], const float hi[3], const float* rays, size_t n, uint8_t* out_fast,
                           uint8_t* out_exact) {
    if (!lo || !hi || (!rays && n) || !out_fast || !out_exact) return fail(RBRT_ERR_INVALID_ARG, "selftest_gate: null argument");
    if (n == 0) return RBRT_OK;
    if (int rc = ensure_device(0)) return rc;
    DevBuf<float> d_box, d_rays;
    DevBuf<uint8_t> d_f, d_e;
    const float box[6] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    hipError_t e = d_box.upload(box, 6);
    if (e == hipSuccess) e = d_rays.upload(rays, n * 6);
    if (e == hipSuccess) e = d_f.alloc(n);
    if (e == hipSuccess) e = d_e.alloc(n);
    if (e == hipSuccess) e = launch_gate_selftest(d_box.get(), d_rays.get(), n, d_f.get(), d_e.get());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = d_f.to_host(out_fast, n);
    if (e == hipSuccess) e = d_e.to_host(out_exact, n);
    return hook_result(e, "selftest_gate");
}

// Test hook: the kernels' short forms of IEEE sqrt / normalize against the compiler's, on n pseudo-random operands.
int rbrt_hip_selftest_ieee(uint64_t seed, size_t n, uint64_t counts[3]) {
    if (!counts) return fail(RBRT_ERR_INVALID_ARG, "selftest_ieee: null argument");
    if (n >= (1ull << 32) * 256ull) return fail(RBRT_ERR_INVALID_ARG, "selftest_ieee: n too large");
    return device_counts3("selftest_ieee", counts, [&](unsigned long long* d) { return launch_ieee_selftest(seed, n, d); });
}

// Test hook: ieee_sqrt / normalize of the kernels on caller-supplied operands, with the path each element's wave took.
int rbrt_hip_debug_ieee(const float* x, size_t n, const float* v, size_t m, float* out_sqrt, uint8_t* out_sqrt_short,
                        float* out_norm, uint8_t* out_norm_short) {
    if ((n && (!x || !out_sqrt || !out_sqrt_short)) || (m && (!v || !out_norm || !out_norm_short)))
        return fail(RBRT_ERR_INVALID_ARG, "debug_ieee: null argument");
    if (n >= (1ull << 32) * 256ull || m >= (1ull << 32) * 256ull) return fail(RBRT_ERR_INVALID_ARG, "debug_ieee: n or m too large");
    if (n == 0 && m == 0) return RBRT_OK;
    if (int rc = ensure_device(0)) return rc;
    DevBuf<float> d_x, d_v, d_s, d_q;
    DevBuf<uint8_t> d_sf, d_qf;
    const size_t nx = std::max<size_t>(n, 1), nv = std::max<size_t>(m, 1);
    hipError_t e = d_x.alloc(nx);
    if (e == hipSuccess) e = d_s.alloc(nx);
    if (e == hipSuccess) e = d_sf.alloc(nx);
    if (e == hipSuccess) e = d_v.alloc(nv * 3);
    if (e == hipSuccess) e = d_q.alloc(nv * 3);
    if (e == hipSuccess) e = d_qf.alloc(nv);
    if (e == hipSuccess && n) e = d_x.from_host(x, n);
    if (e == hipSuccess && m) e = d_v.from_host(v, m * 3);
    if (e == hipSuccess) e = launch_ieee_debug(d_x.get(), n, d_v.get(), m, d_s.get(), d_sf.get(), d_q.get(), d_qf.get());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && n) e = d_s.to_host(out_sqrt, n);
    if (e == hipSuccess && n) e = d_sf.to_host(out_sqrt_short, n);
    if (e == hipSuccess && m) e = d_q.to_host(out_norm, m * 3);
    if (e == hipSuccess && m) e = d_qf.to_host(out_norm_short, m);
    return hook_result(e, "debug_ieee");
}

// Test hook: ieee_sqrt of every float with bits in [first_bits, first_bits + n), checked on the device.
int rbrt_hip_selftest_sqrt_sweep(uint32_t first_bits, uint64_t n, uint64_t counts[3]) {
    if (!counts) return fail(RBRT_ERR_INVALID_ARG, "selftest_sqrt_sweep: null argument");
    if (first_bits < 0x00800000u || n > uint64_t(0x7F800000u - first_bits))
        return fail(RBRT_ERR_INVALID_ARG, "selftest_sqrt_sweep: the range must hold positive normal floats only");
    return device_counts3("selftest_sqrt_sweep", counts, [&](unsigned long long* d) { return launch_sqrt_sweep(first_bits, n, d); });
}

}  // extern "C"
