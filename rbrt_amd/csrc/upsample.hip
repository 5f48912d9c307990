// upsample.hip — the guided upsampling of include/rbrt_hip.h "Guided upsampling" for gfx950 (MI355X / CDNA4).
//
// A translation unit of its own: nothing here is seen by kernels.hip, megakernel.inl, features.inl, guided.hip or temporal.hip,
// whose code stays as it is. The arithmetic is the header's rule operation by operation: f32, no FMA (-ffp-contract=off and the
// pragma below), the compiler's correctly rounded `/` (-fno-fast-math; no reciprocal shortcut), every sum in the rule's order.
//
// The workspace holds four planes of one float4 a LOW pixel: {a~.rgb, wa_l}, {b~.rgb, z_l}, {N_l.xyz, c_l}, {m_l.rgb, 0}. A tap
// is then four aligned 16-byte loads instead of fourteen scalar ones.
//
// upsample_reduce_kernel: one thread per low pixel. Sums the eight feature channels over the pixel's block of f x f full pixels
//   (rows outer, columns inner), divides the albedo out of the low halves and writes the four records. It is the only kernel
//   that reads the low halves.
// upsample_gather_kernel: one thread per full pixel, a workgroup of 256 covers a tile of 32 x 8 full pixels
//   (RBRT_UPSAMPLE_TILE_W x RBRT_UPSAMPLE_TILE_H): a wave's 64 lanes are two rows of 32, so a row writes 384 contiguous bytes
//   of an output. A low pixel is read by f * f to 4 * f * f full pixels, so the tile's low pixels and a margin go to LDS first,
//   plane by plane, and the taps read LDS: neighbouring lanes of a row read the same or the next 16-byte slot (a broadcast or
//   consecutive slots, no bank conflict). The staged range comes from integers (the exact floor of the rule's coordinate at the
//   tile's first and last pixel, one more low pixel on either side for the float rule's rounding, clipped to the low image); a
//   tap outside it -- none at the sizes a float holds exactly -- is read from the workspace itself, which holds the same bits.
//   The four taps are accumulated sequentially in the rule's order: no atomics, no cross-lane sums. Every tap index is an
//   integer clamped into the low image before it is used: no read leaves the buffers whatever the floats are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kTileW = int(RBRT_UPSAMPLE_TILE_W), kTileH = int(RBRT_UPSAMPLE_TILE_H);
constexpr int kThreads = kTileW * kTileH;
constexpr int kMargin = 3;  // staged low pixels beyond (tile edge) / f: one for the second tap, one on either side for rounding
constexpr int kStagedMax = (kTileW + kMargin) * (kTileH + kMargin);  // at f = 1, the widest
constexpr float kEps = 1e-7f;
constexpr float kFloor = 0.01f;
constexpr float kMinDen = 0.01f;

static_assert(kThreads == 256 && kThreads % 64 == 0, "a workgroup of the gather kernel is four waves");
static_assert(size_t(kStagedMax) * 4u * sizeof(float4) <= 64u * 1024u, "the staged records fit the default LDS limit");

// floor(a / b) for b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__device__ __forceinline__ int clampi(long long v, int hi) { return v < 0 ? 0 : v > (long long)hi ? hi : int(v); }

__global__ __launch_bounds__(kThreads) void upsample_reduce_kernel(const UpsampleParams U) {
    const size_t nlow = size_t(U.low_width) * U.low_height;
    const size_t q = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (q >= nlow) return;
    const uint32_t f = U.factor, W = U.width, H = U.height;
    const uint32_t j = uint32_t(q / U.low_width), i = uint32_t(q - size_t(j) * U.low_width);
    const uint32_t y0 = j * f, x0 = i * f;
    const uint32_t y1 = y0 + f < H ? y0 + f : H, x1 = x0 + f < W ? x0 + f : W;
    float rho[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f}, z = 0.0f, c = 0.0f;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t x = x0; x < x1; ++x) {
            const size_t p = size_t(y) * W + x;
            for (int k = 0; k < 3; ++k) {
                rho[k] = rho[k] + U.albedo[p * 3 + k];
                n[k] = n[k] + U.normal[p * 3 + k];
            }
            z = z + U.depth[p];
            c = c + U.coverage[p];
        }
    const float inv = 1.0f / float((y1 - y0) * (x1 - x0));
    const bool demodulate = (U.flags & RBRT_UPSAMPLE_NO_DEMODULATION) == 0u;
    c = c * inv;
    const float bare = 1.0f - c;
    float m[3], a[3], b[3];
    for (int k = 0; k < 3; ++k) {
        m[k] = fmaxf((rho[k] * inv) + bare, kFloor);
        const float u = demodulate ? m[k] : 1.0f;
        a[k] = U.a[q * 3 + k] / u;
        b[k] = U.b[q * 3 + k] / u;
    }
    float4* const w = static_cast<float4*>(U.workspace);
    w[q] = make_float4(a[0], a[1], a[2], U.wa ? U.wa[q] : 0.5f);
    w[nlow + q] = make_float4(b[0], b[1], b[2], z * inv);
    w[2 * nlow + q] = make_float4(n[0] * inv, n[1] * inv, n[2] * inv, c);
    w[3 * nlow + q] = make_float4(m[0], m[1], m[2], 0.0f);
}

struct Sums {
    float den, na[3], nb[3], nw;
};

__global__ __launch_bounds__(kThreads) void upsample_gather_kernel(const UpsampleParams U, const uint32_t tiles_x) {
    __shared__ float4 lds4[4 * kStagedMax];
    const int W = int(U.width), H = int(U.height), w = int(U.low_width), h = int(U.low_height), f = int(U.factor);
    const size_t nlow = size_t(U.low_width) * U.low_height;
    const float4* const rec = static_cast<const float4*>(U.workspace);
    const int tid = int(threadIdx.x);
    const int tile_y = int(blockIdx.x / tiles_x), tile_x = int(blockIdx.x - uint32_t(tile_y) * tiles_x);
    const int y0 = tile_y * kTileH, x0 = tile_x * kTileW;
    const int yl = (y0 + kTileH < H ? y0 + kTileH : H) - 1, xl = (x0 + kTileW < W ? x0 + kTileW : W) - 1;  // the tile's last pixel
    // the staged low pixels [sy0, sy1] x [sx0, sx1]: floor(((C + 0.5) / f) - 0.5) = floor((2 C + 1 - f) / (2 f)), exactly
    const int sx0 = clampi(floor_div(2ll * x0 + 1 - f, 2 * f) - 1, w - 1), sx1 = clampi(floor_div(2ll * xl + 1 - f, 2 * f) + 2, w - 1);
    const int sy0 = clampi(floor_div(2ll * y0 + 1 - f, 2 * f) - 1, h - 1), sy1 = clampi(floor_div(2ll * yl + 1 - f, 2 * f) + 2, h - 1);
    const int SW = sx1 - sx0 + 1, SH = sy1 - sy0 + 1;  // (at most kTileW + kMargin and kTileH + kMargin)
    const int staged = SW * SH;
    for (int idx = tid; idx < staged; idx += kThreads) {
        const int sy = idx / SW, sx = idx - sy * SW;
        const size_t g = size_t(sy0 + sy) * size_t(w) + size_t(sx0 + sx);
        lds4[idx] = rec[g];
        lds4[kStagedMax + idx] = rec[nlow + g];
        lds4[2 * kStagedMax + idx] = rec[2 * nlow + g];
        lds4[3 * kStagedMax + idx] = rec[3 * nlow + g];
    }
    __syncthreads();
    const int ty = tid / kTileW, tx = tid - ty * kTileW;
    const int R = y0 + ty, C = x0 + tx;
    if (R >= H || C >= W) return;  // (behind the only barrier)
    const size_t p = size_t(R) * size_t(W) + size_t(C);
    const bool demodulate = (U.flags & RBRT_UPSAMPLE_NO_DEMODULATION) == 0u;
    const float z = U.depth[p], bare = 1.0f - U.coverage[p];
    float N[3], m[3], u[3];
    for (int k = 0; k < 3; ++k) {
        N[k] = U.normal[p * 3 + k];
        m[k] = fmaxf(U.albedo[p * 3 + k] + bare, kFloor);
        u[k] = demodulate ? m[k] : 1.0f;
    }
    const float xs = ((float(C) + 0.5f) * U.invf) - 0.5f, ys = ((float(R) + 0.5f) * U.invf) - 0.5f;
    const float fi = __builtin_floorf(xs), fj = __builtin_floorf(ys);
    const float fx = xs - fi, fy = ys - fj;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const long long i = (long long)fi, j = (long long)fj;  // (finite, below 2^32 in size)
    const float bw[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    Sums S = {0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qy = clampi(j + (k >> 1), h - 1), qx = clampi(i + (k & 1), w - 1);
        float4 ra, rb, rn, rm;
        if (qy >= sy0 && qy <= sy1 && qx >= sx0 && qx <= sx1) {
            const int idx = (qy - sy0) * SW + (qx - sx0);
            ra = lds4[idx], rb = lds4[kStagedMax + idx], rn = lds4[2 * kStagedMax + idx], rm = lds4[3 * kStagedMax + idx];
        } else {
            const size_t g = size_t(qy) * size_t(w) + size_t(qx);
            ra = rec[g], rb = rec[nlow + g], rn = rec[2 * nlow + g], rm = rec[3 * nlow + g];
        }
        const float nx = rn.x - N[0], ny = rn.y - N[1], nz = rn.z - N[2];
        const float Dn = (((nx * nx) + (ny * ny)) + (nz * nz)) * U.in;
        const float ar = rm.x - m[0], ag = rm.y - m[1], ab = rm.z - m[2];
        const float Da = (((ar * ar) + (ag * ag)) + (ab * ab)) * U.ia;
        const float dz = rb.w - z;
        const float Dz = (dz * dz) / (kEps + (U.kz2 * (z * rb.w)));
        const float D = (Dn + Dz) + Da;
        const float g = fmaxf(0.0f, 1.0f - 0.25f * fmaxf(D, 0.0f));
        const float wt = bw[k] * ((g * g) * (g * g));
        if (!(wt > 0.0f)) continue;  // (a NaN compares false)
        S.den = S.den + wt;
        S.na[0] = S.na[0] + wt * ra.x;
        S.na[1] = S.na[1] + wt * ra.y;
        S.na[2] = S.na[2] + wt * ra.z;
        S.nb[0] = S.nb[0] + wt * rb.x;
        S.nb[1] = S.nb[1] + wt * rb.y;
        S.nb[2] = S.nb[2] + wt * rb.z;
        S.nw = S.nw + wt * ra.w;
    }
    float A[3], B[3], wa;
    if (S.den >= kMinDen) {
        for (int k = 0; k < 3; ++k) {
            A[k] = (S.na[k] / S.den) * u[k];
            B[k] = (S.nb[k] / S.den) * u[k];
        }
        wa = S.nw / S.den;
    } else {  // the low pixel whose block holds this pixel; it is inside the low image by construction
        const size_t g = size_t(R / f) * size_t(w) + size_t(C / f);
        const float4 ra = rec[g], rb = rec[nlow + g];
        A[0] = ra.x * u[0], A[1] = ra.y * u[1], A[2] = ra.z * u[2];
        B[0] = rb.x * u[0], B[1] = rb.y * u[1], B[2] = rb.z * u[2];
        wa = ra.w;
    }
    if (U.out_a) {
        U.out_a[p * 3 + 0] = A[0];
        U.out_a[p * 3 + 1] = A[1];
        U.out_a[p * 3 + 2] = A[2];
    }
    if (U.out_b) {
        U.out_b[p * 3 + 0] = B[0];
        U.out_b[p * 3 + 1] = B[1];
        U.out_b[p * 3 + 2] = B[2];
    }
    if (U.out_wa) U.out_wa[p] = wa;
}

}  // namespace

// (the arguments have been checked: rbrt_hip_upsample_halves)
hipError_t launch_upsample(const UpsampleParams& U, hipStream_t stream) {
    const size_t npix = size_t(U.width) * U.height, nlow = size_t(U.low_width) * U.low_height;
    if (npix == 0 || npix >= (size_t(1) << 31) || U.factor == 0u || U.factor > RBRT_UPSAMPLE_MAX_FACTOR) return hipErrorInvalidValue;
    if (U.low_width != (U.width + U.factor - 1u) / U.factor || U.low_height != (U.height + U.factor - 1u) / U.factor) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample_reduce_kernel, dim3(uint32_t((nlow + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, U);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t tiles_x = (U.width + kTileW - 1) / kTileW, tiles_y = (U.height + kTileH - 1) / kTileH;
    if (uint64_t(tiles_x) * tiles_y >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsample_gather_kernel, dim3(tiles_x * tiles_y), dim3(kThreads), 0, stream, U, tiles_x);
    return hipGetLastError();
}

}  // namespace rbrt
