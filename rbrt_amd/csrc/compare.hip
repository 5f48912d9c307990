// compare.hip — the image comparison of include/rbrt_hip.h "Image comparison" for gfx950 (MI355X / CDNA4).
//
// A translation unit of its own: nothing here is seen by the other kernel files, whose code stays as it is. The arithmetic is
// the header's rule operation by operation: f32 per pixel, f64 for the sums, no FMA (-ffp-contract=off and the pragma below),
// the compiler's correctly rounded `/` (-fno-fast-math; no reciprocal shortcut).
//
// compare_tile_kernel: one workgroup of 256 threads per tile of 16 x 16 pixels (RBRT_COMPARE_TILE_W x RBRT_COMPARE_TILE_H), one
//   thread per pixel. The workgroup stages u = T(Y(X)) and v = T(Y(R)) over the tile and a halo of 5 in LDS, two planes of
//   26 x 26 floats; a cell's coordinates are clamped to the image there, so that the passes behind it index LDS only. The row
//   pass makes the five planes' 11-tap sums for the tile's 16 columns over the 26 staged rows (416 cells, two trips of the 256
//   threads) into LDS, and the column pass reads 11 of them per plane: 13.7 KB of LDS in all. A wave's 64 lanes are four rows of
//   16, so the column pass reads 64 consecutive words (no bank conflict); the row pass reads rows 26 words apart, two rows to a
//   group of 32 lanes (at most 2-way). A thread then loads its own two pixels for the errors. The four sums go through the
//   rule's pairwise tree: t = ty * 16 + tx is the thread's index, the levels s = 1..32 are shuffles inside a wave (lane i takes
//   v[i] + v[i + s]; the lanes that are multiples of 2 s hold what the rule says, the others are never read), the levels 64 and
//   128 go through 4 words of LDS per sum. Thread 0 writes the tile's record into the caller's workspace. No atomics.
//   A thread outside the image does all of this on clamped data and contributes +0.0, no count and no store.
// compare_reduce_kernel: one workgroup of 256. Lane t adds the tiles t, t + 256, ... in ascending order onto +0.0, the same tree
//   follows, and thread 0 writes all 64 bytes of the result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kTile = int(RBRT_COMPARE_TILE_W);
constexpr int kThreads = kTile * int(RBRT_COMPARE_TILE_H);
constexpr int kTaps = 11, kHalo = 5;
constexpr int kSide = kTile + 2 * kHalo;  // 26: the staged planes' side
constexpr float kMaxF = 3.4028235e38f;
constexpr float kC1 = 0.0001f, kC2 = 0.0009f;

static_assert(RBRT_COMPARE_TILE_W == 16u && RBRT_COMPARE_TILE_H == 16u && kThreads == 256, "a workgroup is one tile, four waves");
static_assert(sizeof(rbrt_compare_result_t) == 64, "the result is 64 bytes");

__device__ __forceinline__ float tap(int i) {  // (i is a constant of an unrolled loop)
    constexpr float g[kTaps] = {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
                                0.213005543f,   0.109360687f,   0.0360007733f, 0.00759875821f, 0.00102838012f};
    return g[i];
}

__device__ __forceinline__ bool fin(float x) { return x <= kMaxF && x >= -kMaxF; }
__device__ __forceinline__ float luminance(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }
__device__ __forceinline__ float pos(float x) { return fin(x) && x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float tone(const float* c) {  // T(Y(c))
    const float y = pos(luminance(c[0], c[1], c[2]));
    return y / (1.0f + y);
}

struct Sums {
    double se, ae, rel, ssim;
    float mx;
    uint32_t usable, skipped;
};

// One level of the pairwise tree inside a wave: lane i takes v[i] + v[i + s].
__device__ __forceinline__ void wave_level(Sums& v, int s) {
    v.se = v.se + __shfl_down(v.se, unsigned(s), 64);
    v.ae = v.ae + __shfl_down(v.ae, unsigned(s), 64);
    v.rel = v.rel + __shfl_down(v.rel, unsigned(s), 64);
    v.ssim = v.ssim + __shfl_down(v.ssim, unsigned(s), 64);
    v.mx = fmaxf(v.mx, __shfl_down(v.mx, unsigned(s), 64));
    v.usable += __shfl_down(v.usable, unsigned(s), 64);
    v.skipped += __shfl_down(v.skipped, unsigned(s), 64);
}

// The tree over the workgroup's 256 values, v of thread t being v[t]: -> thread 0 holds v[0] of the rule. `across` is LDS for
// the four waves' results. Every thread of the workgroup calls it.
__device__ __forceinline__ void tree(Sums& v, Sums* across, int tid) {
#pragma unroll
    for (int s = 1; s < 64; s *= 2) wave_level(v, s);
    if ((tid & 63) == 0) across[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        const Sums &a = across[0], &b = across[1], &c = across[2], &d = across[3];
        v.se = (a.se + b.se) + (c.se + d.se);
        v.ae = (a.ae + b.ae) + (c.ae + d.ae);
        v.rel = (a.rel + b.rel) + (c.rel + d.rel);
        v.ssim = (a.ssim + b.ssim) + (c.ssim + d.ssim);
        v.mx = fmaxf(fmaxf(a.mx, b.mx), fmaxf(c.mx, d.mx));
        v.usable = (a.usable + b.usable) + (c.usable + d.usable);
        v.skipped = (a.skipped + b.skipped) + (c.skipped + d.skipped);
    }
}

__global__ __launch_bounds__(kThreads) void compare_tile_kernel(const CompareParams C) {
    __shared__ float su[kSide * kSide];
    __shared__ float sv[kSide * kSide];
    __shared__ float sh[5][kSide * kTile];
    __shared__ Sums across[4];
    const int W = int(C.width), H = int(C.height);
    const int tid = int(threadIdx.x);
    const int tile_y = int(blockIdx.x / C.tiles_x), tile_x = int(blockIdx.x - uint32_t(tile_y) * C.tiles_x);
    const int y0 = tile_y * kTile, x0 = tile_x * kTile;
    const int ty = tid / kTile, tx = tid - ty * kTile;
    const int py = y0 + ty, px = x0 + tx;
    const bool inside = py < H && px < W;
    const bool want_ssim = C.ssim_map != nullptr || C.partials != nullptr;  // (uniform)
    float ssim = 0.0f;
    if (want_ssim) {
        for (int idx = tid; idx < kSide * kSide; idx += kThreads) {
            const int sy = idx / kSide, sx = idx - sy * kSide;
            const int gy = min(max(y0 - kHalo + sy, 0), H - 1), gx = min(max(x0 - kHalo + sx, 0), W - 1);  // (no read leaves the images)
            const size_t q = (size_t(gy) * size_t(W) + size_t(gx)) * 3u;
            su[idx] = tone(C.x + q);
            sv[idx] = tone(C.ref + q);
        }
        __syncthreads();
        for (int idx = tid; idx < kSide * kTile; idx += kThreads) {  // rows: cell (sy, cx) of the five planes
            const int sy = idx / kTile, cx = idx - sy * kTile;
            const float* const ru = su + sy * kSide + cx;
            const float* const rv = sv + sy * kSide + cx;
            float hu = 0.0f, hv = 0.0f, huu = 0.0f, hvv = 0.0f, huv = 0.0f;
#pragma unroll
            for (int i = 0; i < kTaps; ++i) {
                const float u = ru[i], v = rv[i], g = tap(i);
                const float pu = g * u, pv = g * v, puu = g * (u * u), pvv = g * (v * v), puv = g * (u * v);
                if (i == 0) {
                    hu = pu, hv = pv, huu = puu, hvv = pvv, huv = puv;
                } else {
                    hu = hu + pu, hv = hv + pv, huu = huu + puu, hvv = hvv + pvv, huv = huv + puv;
                }
            }
            sh[0][idx] = hu, sh[1][idx] = hv, sh[2][idx] = huu, sh[3][idx] = hvv, sh[4][idx] = huv;
        }
        __syncthreads();
        float V[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {  // columns
            const float* const col = sh[m] + ty * kTile + tx;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < kTaps; ++j) {
                const float p = tap(j) * col[j * kTile];
                acc = j == 0 ? p : acc + p;
            }
            V[m] = acc;
        }
        const float mu = V[0], mv = V[1];
        const float vu = V[2] - (mu * mu), vv = V[3] - (mv * mv), vuv = V[4] - (mu * mv);
        ssim = (((2.0f * (mu * mv)) + kC1) * ((2.0f * vuv) + kC2)) / ((((mu * mu) + (mv * mv)) + kC1) * ((vu + vv) + kC2));
    }
    Sums s;
    s.se = s.ae = s.rel = s.ssim = 0.0;
    s.mx = 0.0f, s.usable = s.skipped = 0u;
    if (inside) {
        const size_t p = size_t(py) * size_t(W) + size_t(px);
        const float xr = C.x[p * 3], xg = C.x[p * 3 + 1], xb = C.x[p * 3 + 2];
        const float rr = C.ref[p * 3], rg = C.ref[p * 3 + 1], rb = C.ref[p * 3 + 2];
        float rel = 0.0f;
        if (fin(xr) && fin(xg) && fin(xb) && fin(rr) && fin(rg) && fin(rb)) {
            const float er = xr - rr, eg = xg - rg, eb = xb - rb;
            const float se = ((er * er) + (eg * eg)) + (eb * eb);
            const float ae = (fabsf(er) + fabsf(eg)) + fabsf(eb);
            rel = (((er * er) / ((rr * rr) + C.epsilon)) + ((eg * eg) / ((rg * rg) + C.epsilon))) + ((eb * eb) / ((rb * rb) + C.epsilon));
            s.se = double(se), s.ae = double(ae), s.rel = double(rel);
            s.mx = fmaxf(fmaxf(fabsf(er), fabsf(eg)), fabsf(eb));
            s.usable = 1u;
        } else {
            s.skipped = 1u;
        }
        s.ssim = double(ssim);
        if (C.rel_map) C.rel_map[p] = rel;
        if (C.ssim_map) C.ssim_map[p] = ssim;
    }
    if (C.partials) {  // (uniform: every thread takes part in the tree)
        tree(s, across, tid);
        if (tid == 0) {
            CompareTilePartial t;
            t.se = s.se, t.ae = s.ae, t.rel = s.rel, t.ssim = s.ssim, t.mx = s.mx, t.usable = s.usable, t.skipped = s.skipped, t.pad = 0u;
            C.partials[blockIdx.x] = t;
        }
    }
}

__global__ __launch_bounds__(kThreads) void compare_reduce_kernel(const CompareTilePartial* __restrict__ partials, const uint32_t tiles,
                                                                  rbrt_compare_result_t* __restrict__ result) {
    __shared__ Sums across[4];
    const int tid = int(threadIdx.x);
    Sums s;
    s.se = s.ae = s.rel = s.ssim = 0.0;
    s.mx = 0.0f, s.usable = s.skipped = 0u;
    for (uint32_t j = uint32_t(tid); j < tiles; j += uint32_t(kThreads)) {  // (every read is of a record the tile kernel wrote)
        const CompareTilePartial t = partials[j];
        s.se = s.se + t.se, s.ae = s.ae + t.ae, s.rel = s.rel + t.rel, s.ssim = s.ssim + t.ssim;
        s.mx = fmaxf(s.mx, t.mx);
        s.usable += t.usable, s.skipped += t.skipped;
    }
    tree(s, across, tid);
    if (tid == 0) {
        rbrt_compare_result_t r;
        r.sum_se = s.se, r.sum_ae = s.ae, r.sum_rel = s.rel, r.sum_ssim = s.ssim;
        r.max_abs = s.mx, r.usable = s.usable, r.skipped = s.skipped;
        for (uint32_t& w : r.reserved) w = 0u;
        *result = r;
    }
}

}  // namespace

// (the arguments have been checked: rbrt_hip_compare_images)
hipError_t launch_compare(const CompareParams& C, hipStream_t stream) {
    const size_t npix = size_t(C.width) * C.height;
    if (npix == 0 || npix >= (size_t(1) << 31) || C.tiles == 0u || C.tiles_x == 0u) return hipErrorInvalidValue;
    if ((C.result != nullptr) != (C.partials != nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compare_tile_kernel, dim3(C.tiles), dim3(kThreads), 0, stream, C);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !C.result) return e;
    hipLaunchKernelGGL(compare_reduce_kernel, dim3(1), dim3(kThreads), 0, stream, C.partials, C.tiles,
                       static_cast<rbrt_compare_result_t*>(C.result));
    return hipGetLastError();
}

}  // namespace rbrt
