// denoise.hip — the dual-buffer non-local-means filter of include/rbrt_hip.h "Denoising" for gfx950 (MI355X / CDNA4).
//
// A translation unit of its own: nothing here is seen by kernels.hip or megakernel.inl, whose code stays as it is.
// The arithmetic is the header's rule operation by operation: f32, no FMA (-ffp-contract=off and the pragma below), the
// compiler's correctly rounded `/` (-fno-fast-math; no reciprocal shortcut), every sum in the rule's order.
//
// denoise_kernel<P>: one thread per output pixel, a workgroup of 256 covers a 16 x 16 pixel tile (RBRT_DENOISE_TILE).
//   Staging, once: A, B and the variance V of the tile plus a halo of R + P go to LDS, nine floats a pixel (an odd stride:
//   neighbouring pixels fall on different banks). V is computed here from the 3 x 3 neighbourhood in global memory, so the
//   filter needs no scratch buffer at all.
//   Then, per offset of the window in the rule's order (a pixel's accumulation is sequential by definition), for BOTH
//   directions of the filter at once -- the variance terms and the divisor of a delta do not depend on the guide:
//     1. delta for the tile plus a halo of P                        -> LDS      (the three divisions per delta: the cost)
//     2. the patch's row sums, (16 + 2P) rows of 16                 -> LDS
//     3. every pixel adds its 2P + 1 row sums, normalises, weighs and accumulates.
//   A barrier behind 1 and 2. The next offset's deltas may be written at once: they are read only in step 2, which every
//   thread has left; its row sums are written behind the next barrier, which every thread reaches after its step 3.
//   Offsets at which no pixel of the tile has its q inside the image are skipped by the whole workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kTile = int(RBRT_DENOISE_TILE);
constexpr int kThreads = kTile * kTile;
constexpr int kStagedFloats = 9;  // A rgb, B rgb, V rgb
constexpr float kEps = 1e-7f;
constexpr int kMaxPatch = 4, kMaxWindow = 10;
// (16 + 2 * 4)^2 = 576 delta positions at most: three per thread
constexpr int kDeltaRounds = ((kTile + 2 * kMaxPatch) * (kTile + 2 * kMaxPatch) + kThreads - 1) / kThreads;

// lib.rs:116-122: (sqrt(c) * 256) as u8 -- the cast saturates and maps NaN to 0 (kernels.hip has the same function; it is
// repeated here so that this file shares no code with that one).
__device__ __forceinline__ uint8_t quantise(float c) {
    float v = __builtin_sqrtf(c) * 256.0f;
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return uint8_t(v);
}

__device__ __forceinline__ bool inside(int y, int x, int h, int w) { return y >= 0 && y < h && x >= 0 && x < w; }

// how many j in -P..P have both c + j and c + j + d in [0, n)
__device__ __forceinline__ int patch_count(int c, int d, int n, int P) {
    const int lo = max(-P, max(-c, -c - d)), hi = min(P, min(n - 1 - c, n - 1 - c - d));
    return hi - lo + 1;
}

template <int P>
__global__ __launch_bounds__(kThreads) void denoise_kernel(const DenoiseParams D) {
    extern __shared__ float lds[];
    const int R = D.window_radius, H = int(D.height), W = int(D.width);
    const int halo = R + P, SW = kTile + 2 * halo;  // staged edge
    constexpr int EW = kTile + 2 * P;               // edge of the delta area
    float* const stage = lds;                                      // [SW][SW][9]
    float* const delta_b = stage + SW * SW * kStagedFloats;         // [EW][EW] guide B (for filtering A)
    float* const delta_a = delta_b + EW * EW;                       // [EW][EW] guide A (for filtering B)
    float* const rows_b = delta_a + EW * EW;                        // [EW][kTile]
    float* const rows_a = rows_b + EW * kTile;                      // [EW][kTile]
    const int tid = int(threadIdx.x);
    const int y0 = int(blockIdx.y) * kTile, x0 = int(blockIdx.x) * kTile;

    // ---- staging ----
    for (int idx = tid; idx < SW * SW; idx += kThreads) {
        const int sy = idx / SW, sx = idx - sy * SW;
        const int gy = y0 - halo + sy, gx = x0 - halo + sx;
        float v[kStagedFloats] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (inside(gy, gx, H, W)) {
            float sum[3] = {0.0f, 0.0f, 0.0f};
            int count = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int ny = gy + dy, nx = gx + dx;
                    if (!inside(ny, nx, H, W)) continue;
                    const size_t o = (size_t(ny) * size_t(W) + size_t(nx)) * 3u;
                    for (int c = 0; c < 3; ++c) {
                        const float a = D.a[o + c], b = D.b[o + c];
                        const float d = a - b;
                        sum[c] = sum[c] + d * d;
                        if (dy == 0 && dx == 0) v[c] = a, v[3 + c] = b;
                    }
                    ++count;
                }
            for (int c = 0; c < 3; ++c) v[6 + c] = (sum[c] / float(count)) * 0.5f;
        }
        for (int c = 0; c < kStagedFloats; ++c) stage[idx * kStagedFloats + c] = v[c];
    }

    // the delta positions of this thread (the same for every offset): index into the delta area, its staged pixel, its image pixel
    int d_idx[kDeltaRounds], d_gy[kDeltaRounds], d_gx[kDeltaRounds], d_stage[kDeltaRounds];
#pragma unroll
    for (int k = 0; k < kDeltaRounds; ++k) {
        const int idx = tid + k * kThreads;
        const int ey = idx / EW, ex = idx - ey * EW;
        d_idx[k] = idx < EW * EW ? idx : -1;
        d_gy[k] = y0 - P + ey, d_gx[k] = x0 - P + ex;
        d_stage[k] = ((ey + R) * SW + (ex + R)) * kStagedFloats;
    }
    const int ty = tid / kTile, tx = tid - ty * kTile;
    const int py = y0 + ty, px = x0 + tx;
    const bool alive = py < H && px < W;
    const int own_stage = ((ty + halo) * SW + (tx + halo)) * kStagedFloats;
    float num_a[3] = {0.0f, 0.0f, 0.0f}, num_b[3] = {0.0f, 0.0f, 0.0f}, den_a = 0.0f, den_b = 0.0f;
    __syncthreads();

    for (int dy = -R; dy <= R; ++dy) {
        if (y0 + dy + kTile - 1 < 0 || y0 + dy >= H) continue;  // (the whole workgroup: no q of the tile is inside)
        for (int dx = -R; dx <= R; ++dx) {
            if (x0 + dx + kTile - 1 < 0 || x0 + dx >= W) continue;
            const int to_q = (dy * SW + dx) * kStagedFloats;
            // ---- 1. delta ----
#pragma unroll
            for (int k = 0; k < kDeltaRounds; ++k) {
                if (d_idx[k] < 0) continue;
                float db = 0.0f, da = 0.0f;
                if (inside(d_gy[k], d_gx[k], H, W) && inside(d_gy[k] + dy, d_gx[k] + dx, H, W)) {
                    const float* const sp = stage + d_stage[k];
                    const float* const sq = sp + to_q;
                    float tb[3], ta[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float vp = sp[6 + c], vq = sq[6 + c];
                        const float sub = vp + fminf(vp, vq);
                        const float div = kEps + D.k2 * (vp + vq);
                        const float gb = sq[3 + c] - sp[3 + c];
                        const float ga = sq[c] - sp[c];
                        tb[c] = (gb * gb - sub) / div;
                        ta[c] = (ga * ga - sub) / div;
                    }
                    db = (tb[0] + tb[1]) + tb[2];
                    da = (ta[0] + ta[1]) + ta[2];
                }
                delta_b[d_idx[k]] = db;
                delta_a[d_idx[k]] = da;
            }
            __syncthreads();
            // ---- 2. row sums ----
            for (int idx = tid; idx < EW * kTile; idx += kThreads) {
                const int ey = idx / kTile, x = idx - ey * kTile;
                float sb = 0.0f, sa = 0.0f;
#pragma unroll
                for (int i = 0; i <= 2 * P; ++i) {
                    sb = sb + delta_b[ey * EW + x + i];
                    sa = sa + delta_a[ey * EW + x + i];
                }
                rows_b[idx] = sb;
                rows_a[idx] = sa;
            }
            __syncthreads();
            // ---- 3. the pixel's own sum, weight and accumulation ----
            if (alive && inside(py + dy, px + dx, H, W)) {
                float Db = 0.0f, Da = 0.0f;
#pragma unroll
                for (int j = 0; j <= 2 * P; ++j) {
                    Db = Db + rows_b[(ty + j) * kTile + tx];
                    Da = Da + rows_a[(ty + j) * kTile + tx];
                }
                const float norm = float(3 * patch_count(py, dy, H, P) * patch_count(px, dx, W, P));
                Db = Db / norm;
                Da = Da / norm;
                const float t_b = fmaxf(0.0f, 1.0f - 0.25f * fmaxf(Db, 0.0f));
                const float t_a = fmaxf(0.0f, 1.0f - 0.25f * fmaxf(Da, 0.0f));
                const float w_b = (t_b * t_b) * (t_b * t_b), w_a = (t_a * t_a) * (t_a * t_a);
                const float* const sq = stage + own_stage + to_q;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    num_a[c] = num_a[c] + w_b * sq[c];      // A is filtered with the weights of guide B
                    num_b[c] = num_b[c] + w_a * sq[3 + c];  // ... and B with those of guide A
                }
                den_a = den_a + w_b;
                den_b = den_b + w_a;
            }
        }
    }
    if (!alive) return;
    const size_t i = size_t(py) * size_t(W) + size_t(px);
    const float wa = D.wa ? D.wa[i] : 0.5f;
    const float wb = 1.0f - wa;
    float out[3];
    for (int c = 0; c < 3; ++c) out[c] = ((num_a[c] / den_a) * wa) + ((num_b[c] / den_b) * wb);
    if (D.out_radiance) {
        D.out_radiance[i * 3 + 0] = out[0];
        D.out_radiance[i * 3 + 1] = out[1];
        D.out_radiance[i * 3 + 2] = out[2];
    }
    if (D.out_rgb8) {
        D.out_rgb8[i * 3 + 0] = quantise(out[0]);
        D.out_rgb8[i * 3 + 1] = quantise(out[1]);
        D.out_rgb8[i * 3 + 2] = quantise(out[2]);
    }
}

// The packed running sums of an adaptive call -> the row-major half images and their mix ("From a handle's sums").
// One thread per pixel of the image.
__global__ __launch_bounds__(kThreads) void denoise_halves_kernel(const DenoiseHalvesParams Q) {
    const size_t i = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= size_t(Q.width) * Q.height) return;
    const uint32_t row = uint32_t(i / Q.width), col = uint32_t(i - size_t(row) * Q.width);
    const uint32_t tile = tile_number(row / RBRT_TILE, col / RBRT_TILE, Q.tiles_x);
    const size_t j = size_t(tile) * 64u + (row % RBRT_TILE) * RBRT_TILE + col % RBRT_TILE;
    const uint32_t n = Q.tile_samples[tile], h = (n + 1u) / 2u, g = n - h;
    const float inv_h = 1.0f / float(h), inv_g = 1.0f / float(g);
    for (int c = 0; c < 3; ++c) {
        const float s = Q.acc[j * 3 + c], e = Q.acc_even[j * 3 + c];
        const float a = e * inv_h, b = (s - e) * inv_g;
        Q.a[i * 3 + c] = a;
        Q.b[i * 3 + c] = b;
        if (Q.out_a) Q.out_a[i * 3 + c] = a;
        if (Q.out_b) Q.out_b[i * 3 + c] = b;
    }
    Q.wa[i] = float(h) * (1.0f / float(n));
}

template <int P>
hipError_t launch_denoise_p(const DenoiseParams& D, hipStream_t stream) {
    const int sw = kTile + 2 * (D.window_radius + P), ew = kTile + 2 * P;
    const size_t lds_bytes = size_t(sw * sw * kStagedFloats + 2 * ew * ew + 2 * ew * kTile) * sizeof(float);
    // (more than 64 KiB at the largest window: 77,376 B at R = 10, P = 4, of the CU's 160 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&denoise_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             int(lds_bytes));
    if (e != hipSuccess) return e;
    const dim3 grid((D.width + kTile - 1) / kTile, (D.height + kTile - 1) / kTile);
    hipLaunchKernelGGL(denoise_kernel<P>, grid, dim3(kThreads), lds_bytes, stream, D);
    return hipGetLastError();
}

}  // namespace

// (the arguments have been checked: rbrt_hip_denoise_halves)
hipError_t launch_denoise(const DenoiseParams& D, hipStream_t stream) {
    static_assert(kMaxPatch == 4, "one instantiation per patch radius");
    if (D.window_radius < 0 || D.window_radius > kMaxWindow) return hipErrorInvalidValue;
    if (D.height > 65535u * uint32_t(kTile)) return hipErrorInvalidValue;  // (grid.y)
    switch (D.patch_radius) {
        case 0: return launch_denoise_p<0>(D, stream);
        case 1: return launch_denoise_p<1>(D, stream);
        case 2: return launch_denoise_p<2>(D, stream);
        case 3: return launch_denoise_p<3>(D, stream);
        case 4: return launch_denoise_p<4>(D, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_denoise_halves(const DenoiseHalvesParams& Q, hipStream_t stream) {
    const size_t n = size_t(Q.width) * Q.height;
    hipLaunchKernelGGL(denoise_halves_kernel, dim3(uint32_t((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, Q);
    return hipGetLastError();
}

}  // namespace rbrt
