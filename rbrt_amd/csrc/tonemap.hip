// tonemap.hip — the display transform of include/rbrt_hip.h "Display transform" for gfx950 (MI355X / CDNA4): exposure, automatic
// exposure and white point from an integer histogram of the luminance's float bits, and the tone curves.
//
// A translation unit of its own: nothing here is seen by kernels.hip, megakernel.inl or denoise.hip, whose code stays as it is.
// The arithmetic is the header's rule operation by operation: f32, no FMA (-ffp-contract=off and the pragma below), the
// compiler's correctly rounded `/` and sqrt (-fno-fast-math). Everything the automatic part decides comes from INTEGER counts,
// which do not depend on the order the atomics arrive in: the result is the rule's, bit for bit, on every run.
//
// Three kernels, all on the caller's stream:
//   luminance_histogram_kernel  a capped grid (RBRT_TONEMAP_MAX_BLOCKS workgroups of 256) strides over groups of four pixels,
//     a thread taking one group per stride: three dwordx4 loads. One histogram of 4096 words per workgroup in LDS (16 KiB),
//     filled with LDS atomics; at the end the non-zero bins go out with one global atomic each. The lanes of a wave that share
//     the bin of the wave's first counted lane add once, by their number (a flat image or a background sends every lane to
//     one bin: one LDS atomic a wave instead of 64 that the LDS would serialise); the other lanes add one each.
//   tonemap_select_kernel       one wave. A lane sums 64 consecutive bins, a shuffle scan runs across the wave, the lane in
//     which the prefix sum passes rank k walks its own 64 bins; both ranks; then e and w by the rule and the result struct.
//   tonemap_apply_kernel        the same grid and groups: three dwordx4 loads, the curve, three dwordx4 stores and / or twelve
//     bytes of rgb8. e and w come from the result struct when either was automatic (no host round trip), else from the arguments.
// The vector forms need the pixel pointers 16-byte aligned (rgb8: 4-byte); a pointer that is not sends the call through the
// same kernels instantiated with scalar accesses. Same bits, slower.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kGroup = 4;  // pixels a thread takes per stride
constexpr uint32_t kBins = RBRT_TONEMAP_BINS;
static_assert(RBRT_TONEMAP_BLOCK_PIXELS == kThreads * kGroup, "a workgroup's stride");
static_assert(kBins == 64u * 64u, "tonemap_select_kernel: 64 lanes of 64 bins");
static_assert(sizeof(rbrt_tonemap_result_t) == 32 && RBRT_TONEMAP_RESULT_OFFSET == kBins * 4u, "workspace layout");

// lib.rs:116-122: (sqrt(c) * 256) as u8 -- the cast saturates and maps NaN to 0 (kernels.hip and denoise.hip have the same
// function; it is repeated here so that this file shares no code with those).
__device__ __forceinline__ uint32_t quantise(float c) {
    float v = __builtin_sqrtf(c) * 256.0f;
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return uint32_t(uint8_t(v));
}

__device__ __forceinline__ float luminance(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }

__device__ __forceinline__ rbrt_tonemap_result_t* result_of(uint32_t* hist) {
    return reinterpret_cast<rbrt_tonemap_result_t*>(hist + kBins);
}

// The four pixels of group g (twelve floats) into p; pixels at or beyond n are left as they are. Returns how many there were.
template <bool Vec>
__device__ __forceinline__ uint32_t load_group(const float* in, uint32_t g, uint32_t n, float p[12]) {
    const uint32_t first = g * kGroup, have = n - first < kGroup ? n - first : kGroup;
    const float* const src = in + size_t(g) * 12u;
    if (Vec && have == kGroup) {
        const float4* const v = reinterpret_cast<const float4*>(src);
        const float4 a = v[0], b = v[1], c = v[2];
        p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w, p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
        p[8] = c.x, p[9] = c.y, p[10] = c.z, p[11] = c.w;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 12u; ++i)  // (fixed indices: p stays in registers)
            if (i < have * 3u) p[i] = src[i];
    }
    return have;
}

template <bool Vec>
__global__ __launch_bounds__(kThreads) void luminance_histogram_kernel(const TonemapParams T) {
    __shared__ uint32_t bins[kBins];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t b = tid; b < kBins; b += kThreads) bins[b] = 0u;
    __syncthreads();
    const uint32_t n_groups = (T.n + kGroup - 1u) / kGroup;  // (n < 2^32: no overflow below either, g < 2^30 + the stride)
    for (uint32_t g = blockIdx.x * kThreads + tid; g < n_groups; g += gridDim.x * kThreads) {
        float p[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const uint32_t have = load_group<Vec>(T.in, g, T.n, p);
#pragma unroll
        for (uint32_t i = 0; i < kGroup; ++i) {
            const uint32_t u = __float_as_uint(luminance(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
            const bool counted = i < have && u >= 0x00800000u && u <= 0x7F7FFFFFu;
            const uint32_t bin = u >> 19;  // (< 4096 whenever `counted`)
            // the lanes that are here together: those that share the first counted lane's bin add once
            const uint64_t any = __ballot(counted);
            if (any == 0ull) continue;
            const int leader = __ffsll((unsigned long long)any) - 1;
            const uint32_t leader_bin = uint32_t(__shfl(int(bin), leader));
            const uint64_t same = __ballot(counted && bin == leader_bin);
            if (int(lane) == leader) atomicAdd(&bins[leader_bin], uint32_t(__popcll(same)));
            else if (counted && bin != leader_bin) atomicAdd(&bins[bin], 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = tid; b < kBins; b += kThreads) {
        const uint32_t c = bins[b];
        if (c != 0u) atomicAdd(&T.hist[b], c);
    }
}

// One wave. T.hist is complete (stream order).
__global__ __launch_bounds__(64) void tonemap_select_kernel(const TonemapParams T) {
    __shared__ uint32_t picked[2];
    const uint32_t lane = threadIdx.x;
    const uint32_t* const mine = T.hist + lane * 64u;
    uint32_t sum = 0u;
    for (uint32_t i = 0; i < 64u; ++i) sum += mine[i];
    uint32_t incl = sum;  // (M <= n < 2^32: 32 bits hold every prefix sum)
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t t = uint32_t(__shfl_up(int(incl), d));
        if (lane >= d) incl += t;
    }
    const uint32_t M = uint32_t(__shfl(int(incl), 63));
    const uint32_t excl = incl - sum;
    const bool auto_e = T.exposure == 0.0f, auto_w = T.white == 0.0f;
    if (lane < 2u) picked[lane] = 0u;
    __syncthreads();
    if (M > 0u) {
        for (uint32_t r = 0; r < 2u; ++r) {
            if (r == 0u ? !auto_e : !auto_w) continue;
            const uint64_t k = (uint64_t(M - 1u) * uint64_t(r == 0u ? T.key_permille : T.white_permille)) / 1000ull;
            if (uint64_t(excl) <= k && k < uint64_t(incl)) {  // (exactly one lane: sum > 0 there)
                uint32_t run = excl;
                for (uint32_t i = 0; i < 64u; ++i) {
                    run += mine[i];
                    if (uint64_t(run) > k) {
                        picked[r] = lane * 64u + i;
                        break;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (lane != 0u) return;
    rbrt_tonemap_result_t R;
    R.l_key = 0.0f, R.l_white = 0.0f, R.counted = M, R.reserved = 0u, R.pixels = uint64_t(T.n);
    if (auto_e && M > 0u) R.l_key = __uint_as_float((picked[0] << 19) | (1u << 18));
    if (auto_w && M > 0u) R.l_white = __uint_as_float((picked[1] << 19) | (1u << 18));
    R.exposure = auto_e ? (M > 0u ? T.key / R.l_key : 1.0f) : T.exposure;
    R.white = auto_w ? (M > 0u ? R.exposure * R.l_white : 1.0f) : T.white;
    *result_of(T.hist) = R;
}

// from_workspace: e and w are the result struct's (the select kernel wrote it); else they are the arguments, and with
// write_result the first thread writes the result struct of a call that chose nothing.
template <bool Vec>
__global__ __launch_bounds__(kThreads) void tonemap_apply_kernel(const TonemapParams T, const int from_workspace,
                                                                 const int write_result) {
    const uint32_t tid = threadIdx.x;
    float e = T.exposure, w = T.white;
    if (from_workspace) {
        const rbrt_tonemap_result_t* const R = result_of(T.hist);
        e = R->exposure, w = R->white;
    } else if (write_result && blockIdx.x == 0u && tid == 0u) {
        rbrt_tonemap_result_t R;
        R.exposure = e, R.white = w, R.l_key = 0.0f, R.l_white = 0.0f, R.counted = 0u, R.reserved = 0u, R.pixels = uint64_t(T.n);
        *result_of(T.hist) = R;
    }
    if (!T.out_radiance && !T.out_rgb8) return;
    const float ww = w * w;
    const uint32_t n_groups = (T.n + kGroup - 1u) / kGroup;
    for (uint32_t g = blockIdx.x * kThreads + tid; g < n_groups; g += gridDim.x * kThreads) {
        float p[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const uint32_t have = load_group<Vec>(T.in, g, T.n, p);
#pragma unroll
        for (uint32_t i = 0; i < kGroup; ++i) {
            const float r = e * p[3 * i], gr = e * p[3 * i + 1], b = e * p[3 * i + 2];
            float o[3] = {r, gr, b};
            if (T.curve == RBRT_TONE_REINHARD) {
                const float y = luminance(r, gr, b);
                float s = 1.0f;
                if (y > 0.0f) s = (1.0f + (y / ww)) / (1.0f + y);
                o[0] = r * s, o[1] = gr * s, o[2] = b * s;
            } else if (T.curve == RBRT_TONE_ACES) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float x = o[c] * 0.6f;
                    o[c] = (x * ((2.51f * x) + 0.03f)) / ((x * ((2.43f * x) + 0.59f)) + 0.14f);
                }
            }
            p[3 * i] = o[0], p[3 * i + 1] = o[1], p[3 * i + 2] = o[2];
        }
        const bool full = Vec && have == kGroup;
        if (T.out_radiance) {
            float* const dst = T.out_radiance + size_t(g) * 12u;
            if (full) {
                float4* const v = reinterpret_cast<float4*>(dst);
                v[0] = make_float4(p[0], p[1], p[2], p[3]);
                v[1] = make_float4(p[4], p[5], p[6], p[7]);
                v[2] = make_float4(p[8], p[9], p[10], p[11]);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 12u; ++i)
                    if (i < have * 3u) dst[i] = p[i];
            }
        }
        if (T.out_rgb8) {
            uint8_t* const dst = T.out_rgb8 + size_t(g) * 12u;
            if (full) {
                uint32_t q[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    q[k] = quantise(p[4 * k]) | (quantise(p[4 * k + 1]) << 8) | (quantise(p[4 * k + 2]) << 16) | (quantise(p[4 * k + 3]) << 24);
                uint32_t* const v = reinterpret_cast<uint32_t*>(dst);
                v[0] = q[0], v[1] = q[1], v[2] = q[2];
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 12u; ++i)
                    if (i < have * 3u) dst[i] = uint8_t(quantise(p[i]));
            }
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

}  // namespace

// (the arguments have been checked: rbrt_hip_tonemap)
hipError_t launch_tonemap(const TonemapParams& T, hipStream_t stream) {
    const bool automatic = T.exposure == 0.0f || T.white == 0.0f;
    const uint32_t n_groups = (T.n + kGroup - 1u) / kGroup;
    const uint32_t want = (n_groups + uint32_t(kThreads) - 1u) / uint32_t(kThreads);
    const dim3 grid(want < RBRT_TONEMAP_MAX_BLOCKS ? want : RBRT_TONEMAP_MAX_BLOCKS), block(kThreads);
    const bool vec_in = aligned(T.in, 16);
    const bool vec = vec_in && aligned(T.out_radiance, 16) && aligned(T.out_rgb8, 4);
    if (T.hist) {
        const hipError_t e = hipMemsetAsync(T.hist, 0, size_t(kBins) * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    if (automatic) {
        if (vec_in) hipLaunchKernelGGL(luminance_histogram_kernel<true>, grid, block, 0, stream, T);
        else hipLaunchKernelGGL(luminance_histogram_kernel<false>, grid, block, 0, stream, T);
        hipLaunchKernelGGL(tonemap_select_kernel, dim3(1), dim3(64), 0, stream, T);
        if (!T.out_radiance && !T.out_rgb8) return hipGetLastError();
    } else if (!T.hist && !T.out_radiance && !T.out_rgb8) {
        return hipSuccess;
    }
    const int from_workspace = automatic ? 1 : 0, write_result = T.hist ? 1 : 0;
    if (vec) hipLaunchKernelGGL(tonemap_apply_kernel<true>, grid, block, 0, stream, T, from_workspace, write_result);
    else hipLaunchKernelGGL(tonemap_apply_kernel<false>, grid, block, 0, stream, T, from_workspace, write_result);
    return hipGetLastError();
}

}  // namespace rbrt
