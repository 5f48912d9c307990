// despike.hip — the spike removal of include/rbrt_hip.h "Spike removal" for gfx950 (MI355X / CDNA4).
//
// A translation unit of its own: nothing here is seen by kernels.hip, megakernel.inl, features.inl, guided.hip, temporal.hip or
// upsample.hip, whose code stays as it is. The arithmetic is the header's rule operation by operation: f32, no FMA
// (-ffp-contract=off and the pragma below), the compiler's correctly rounded `/` (-fno-fast-math; no reciprocal shortcut).
//
// despike_kernel<R, K>: one thread per pixel, a workgroup of 256 covers a tile of 32 x 8 pixels (RBRT_DESPIKE_TILE_W x
//   RBRT_DESPIKE_TILE_H): a wave's 64 lanes are two rows of 32, so a row reads and writes 384 contiguous bytes of an image. A
//   pixel's luminance is read by (2 R + 1)^2 pixels, so the workgroup computes pos(Y) of both halves once over the tile and a
//   halo of R and stages it in LDS, two planes of at most 36 x 12 floats; a cell outside the image holds +0, which is what a
//   neighbour that takes no part stands for. Behind the one barrier a thread scans its window of each plane and keeps the K
//   largest values in K registers by a compare-exchange chain: R and K are template parameters, so both loops unroll and no
//   register array is indexed at run time (it would go to scratch). Neighbouring lanes of a row read neighbouring words of LDS
//   (no bank conflict; the two rows of a wave are served in different halves). The thread then loads its own two pixels again,
//   applies the rule and writes up to 25 bytes. The counts are reduced per wave by ballot and popcount: one vector atomic add
//   per wave and half, and only where the wave flagged something. A thread outside the image stages like the others and leaves
//   behind the barrier; it takes no part in the ballots, which count active lanes only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kTileW = int(RBRT_DESPIKE_TILE_W), kTileH = int(RBRT_DESPIKE_TILE_H);
constexpr int kThreads = kTileW * kTileH;
constexpr int kMaxR = int(RBRT_DESPIKE_MAX_RADIUS);
constexpr int kPlaneMax = (kTileW + 2 * kMaxR) * (kTileH + 2 * kMaxR);
constexpr float kMaxF = 3.4028235e38f;

static_assert(kThreads == 256 && kThreads % 64 == 0, "a workgroup is four waves");
static_assert(kTileW == 32, "a wave is two rows of the tile");
static_assert(sizeof(rbrt_despike_result_t) == 16, "the result is four words");

__device__ __forceinline__ bool fin(float x) { return x <= kMaxF && x >= -kMaxF; }
__device__ __forceinline__ float luminance(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }
__device__ __forceinline__ float pos(float x) { return fin(x) && x > 0.0f ? x : 0.0f; }

// The K largest of the window of `plane` around cell (cy, cx), the centre left out, merged into K zeros: top[K - 1] is r.
template <int R, int K>
__device__ __forceinline__ float kth_largest(const float* plane, int cy, int cx) {
    constexpr int SW = kTileW + 2 * R;
    float top[K];
#pragma unroll
    for (int j = 0; j < K; ++j) top[j] = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            float v = plane[(cy + dy) * SW + (cx + dx)];  // (finite and >= +0: the staging took pos())
#pragma unroll
            for (int j = 0; j < K; ++j) {  // top stays sorted, largest first; v carries the smaller on
                const float hi = fmaxf(top[j], v);
                v = fminf(top[j], v);
                top[j] = hi;
            }
        }
    }
    return top[K - 1];
}

// The rule for one half at one pixel: x is X[p] and y its luminance, r the window's rank value, yo the other half's luminance.
// -> flagged
__device__ __forceinline__ bool limit(float x[3], float y, float r, float yo, float t, float f) {
    const float base = fmaxf(r, pos(yo));
    const float lim = fminf((t * base) + f, kMaxF);
    if (!fin(y)) {
        x[0] = x[1] = x[2] = lim;
        return true;
    }
    if (y > lim) {
        const float s = lim / y;
        x[0] = x[0] * s, x[1] = x[1] * s, x[2] = x[2] * s;
        return true;
    }
    return false;
}

template <int R, int K>
__global__ __launch_bounds__(kThreads) void despike_kernel(const DespikeParams D, const uint32_t tiles_x) {
    constexpr int SW = kTileW + 2 * R, SH = kTileH + 2 * R;
    __shared__ float lum[2 * kPlaneMax];
    float* const lum_a = lum;
    float* const lum_b = lum + kPlaneMax;
    const int W = int(D.width), H = int(D.height);
    const int tid = int(threadIdx.x);
    const int tile_y = int(blockIdx.x / tiles_x), tile_x = int(blockIdx.x - uint32_t(tile_y) * tiles_x);
    const int y0 = tile_y * kTileH, x0 = tile_x * kTileW;
    for (int idx = tid; idx < SW * SH; idx += kThreads) {
        const int sy = idx / SW, sx = idx - sy * SW;
        const int gy = y0 - R + sy, gx = x0 - R + sx;
        float la = 0.0f, lb = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {  // (no read leaves the images)
            const size_t q = (size_t(gy) * size_t(W) + size_t(gx)) * 3u;
            la = pos(luminance(D.a[q], D.a[q + 1], D.a[q + 2]));
            lb = pos(luminance(D.b[q], D.b[q + 1], D.b[q + 2]));
        }
        lum_a[idx] = la;
        lum_b[idx] = lb;
    }
    __syncthreads();
    const int ty = tid / kTileW, tx = tid - ty * kTileW;
    const int py = y0 + ty, px = x0 + tx;
    if (py >= H || px >= W) return;  // (behind the only barrier)
    const float ra = kth_largest<R, K>(lum_a, ty + R, tx + R);
    const float rb = kth_largest<R, K>(lum_b, ty + R, tx + R);
    const size_t p = size_t(py) * size_t(W) + size_t(px);
    float xa[3] = {D.a[p * 3], D.a[p * 3 + 1], D.a[p * 3 + 2]};
    float xb[3] = {D.b[p * 3], D.b[p * 3 + 1], D.b[p * 3 + 2]};
    const float ya = luminance(xa[0], xa[1], xa[2]), yb = luminance(xb[0], xb[1], xb[2]);
    const bool fa = limit(xa, ya, ra, yb, D.threshold, D.floor);
    const bool fb = limit(xb, yb, rb, ya, D.threshold, D.floor);
    if (D.out_a) {
        D.out_a[p * 3 + 0] = xa[0];
        D.out_a[p * 3 + 1] = xa[1];
        D.out_a[p * 3 + 2] = xa[2];
    }
    if (D.out_b) {
        D.out_b[p * 3 + 0] = xb[0];
        D.out_b[p * 3 + 1] = xb[1];
        D.out_b[p * 3 + 2] = xb[2];
    }
    if (D.mask) D.mask[p] = uint8_t((fa ? 1u : 0u) | (fb ? 2u : 0u));
    if (D.counts) {  // (uniform; the ballots count the lanes that are here: those inside the image)
        const uint64_t ma = __ballot(fa), mb = __ballot(fb);
        const uint64_t here = __ballot(true);
        const bool first = (tid & 63) == __ffsll((unsigned long long)here) - 1;
        if (first && ma != 0ull) atomicAdd(&D.counts[0], uint32_t(__popcll(ma)));
        if (first && mb != 0ull) atomicAdd(&D.counts[1], uint32_t(__popcll(mb)));
    }
}

template <int R>
hipError_t launch_rank(const DespikeParams& D, uint32_t blocks, uint32_t tiles_x, hipStream_t stream) {
    switch (D.rank) {
        case 1u: hipLaunchKernelGGL((despike_kernel<R, 1>), dim3(blocks), dim3(kThreads), 0, stream, D, tiles_x); break;
        case 2u: hipLaunchKernelGGL((despike_kernel<R, 2>), dim3(blocks), dim3(kThreads), 0, stream, D, tiles_x); break;
        case 3u: hipLaunchKernelGGL((despike_kernel<R, 3>), dim3(blocks), dim3(kThreads), 0, stream, D, tiles_x); break;
        case 4u: hipLaunchKernelGGL((despike_kernel<R, 4>), dim3(blocks), dim3(kThreads), 0, stream, D, tiles_x); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

// (the arguments have been checked: rbrt_hip_despike_halves)
hipError_t launch_despike(const DespikeParams& D, hipStream_t stream) {
    const size_t npix = size_t(D.width) * D.height;
    if (npix == 0 || npix >= (size_t(1) << 31)) return hipErrorInvalidValue;
    const uint32_t tiles_x = (D.width + kTileW - 1) / kTileW, tiles_y = (D.height + kTileH - 1) / kTileH;
    if (uint64_t(tiles_x) * tiles_y >= (1ull << 31)) return hipErrorInvalidValue;
    if (D.counts) {
        const hipError_t e = hipMemsetAsync(D.counts, 0, sizeof(rbrt_despike_result_t), stream);
        if (e != hipSuccess) return e;
    }
    switch (D.radius) {
        case 1u: return launch_rank<1>(D, tiles_x * tiles_y, tiles_x, stream);
        case 2u: return launch_rank<2>(D, tiles_x * tiles_y, tiles_x, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rbrt
