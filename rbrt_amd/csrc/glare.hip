// glare.hip — the glare stage of include/rbrt_hip.h "Glare" for gfx950 (MI355X / CDNA4): a bright pass, a Burt-Adelson pyramid
// of it (REDUCE 1 4 6 4 1 / 16, EXPAND 1 6 1 / 8 and 1 1 / 2), its collapse, and the composite that moves a share of a bright
// pixel's light into its surroundings.
//
// A translation unit of its own: nothing here is seen by kernels.hip, megakernel.inl, denoise.hip or tonemap.hip, whose code
// stays as it is. The arithmetic is the header's rule operation by operation: f32, no FMA (-ffp-contract=off and the pragma
// below), the compiler's correctly rounded `/` and sqrt (-fno-fast-math). Every output pixel is computed by one thread from
// values that earlier launches completed: nothing depends on the order in which workgroups run.
//
// Three kernels, 2 * levels launches in stream order on the caller's stream. No workgroup hands anything to
// another inside a kernel. The pyramid's levels 1..L live in the caller's workspace, level after level, a pixel padded to
// 16 bytes (float4, w = 0): every access to them is one dwordx4.
//   glare_reduce_kernel<FIRST>  a workgroup of 256 makes one RBRT_GLARE_TILE_W x RBRT_GLARE_TILE_H tile of level l + 1. It
//     stages the (2 TW + 3) x (2 TH + 3) input pixels with CLAMPED INDICES (never a clamped address) in LDS -- FIRST reads the
//     image and applies the bright pass on the way --, writes the row sums of its 2 TH + 3 rows to LDS, and after a barrier
//     a thread does the column pass of its own pixel. LDS strides are odd numbers of words (3 a pixel, 3 * 35 a row or
//     column), so the lanes of a half wave fall on different banks in the row and column passes.
//   glare_expand_add_kernel     G_l = D_l + s * EXPAND(G_{l+1}), in place on level l, a thread a pixel: the coarse tile plus
//     a halo of 1 (10 x 10 pixels for 16 x 16) is staged in LDS, a thread reads its 2 or 3 coarse columns in 2 or 3 rows.
//   glare_composite_kernel      at full resolution, a thread takes four pixels next to each other in a row (a workgroup:
//     64 x 16): it stages G_1's 34 x 10 tile, reads its own X, recomputes B, and writes out and / or rgb8. With a width that
//     is a multiple of 4 and pointers aligned to 16 bytes (rgb8: 4) the four pixels are three dwordx4 each way and three
//     words of rgb8; else the same kernel with scalar accesses. Same bits, slower.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t TW = RBRT_GLARE_TILE_W, TH = RBRT_GLARE_TILE_H;  // a REDUCE workgroup's output tile
constexpr uint32_t IW = 2u * TW + 3u, IH = 2u * TH + 3u;            // ... and the input pixels it needs
constexpr uint32_t EW = 16u, EH = 16u;                              // an EXPAND workgroup's tile of the finer level
constexpr uint32_t ECW = EW / 2u + 2u, ECH = EH / 2u + 2u;          // ... and the coarse pixels it needs
constexpr uint32_t CW = 64u, CH = 16u, CGROUP = 4u;                 // the composite's tile; pixels a thread takes
constexpr uint32_t CCW = CW / 2u + 2u, CCH = CH / 2u + 2u;
static_assert(TW * TH == kThreads && EW * EH == kThreads && (CW / CGROUP) * CH == kThreads, "a thread a pixel (or a group)");
static_assert(IW % 2u == 1u && IH % 2u == 1u, "odd LDS strides");
static_assert(RBRT_GLARE_MAX_LEVELS <= 31u, "a level's size is shifted by its number");

// lib.rs:116-122: (sqrt(c) * 256) as u8 -- the cast saturates and maps NaN to 0 (kernels.hip, denoise.hip and tonemap.hip have
// the same function; it is repeated here so that this file shares no code with those).
__device__ __forceinline__ uint32_t quantise(float c) {
    float v = __builtin_sqrtf(c) * 256.0f;
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return uint32_t(uint8_t(v));
}

// cl(k, n) of the rule, on an index (64-bit: 2 * a tile's origin + 34 can pass 2^31 in an image one pixel high).
__device__ __forceinline__ uint32_t cl(int64_t k, uint32_t n) { return uint32_t(k < 0 ? 0 : (k > int64_t(n) - 1 ? int64_t(n) - 1 : k)); }

// The bright pass of one pixel.
__device__ __forceinline__ void bright(float r, float g, float b, float T, float o[3]) {
    const float y = ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b);
    const uint32_t u = __float_as_uint(y);
    o[0] = 0.0f, o[1] = 0.0f, o[2] = 0.0f;
    if (u >= 0x00800000u && u <= 0x7F7FFFFFu && y > T) {
        const float k = (y - T) / y;
        o[0] = r * k, o[1] = g * k, o[2] = b * k;
    }
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void glare_reduce_kernel(const float* __restrict__ image, const float4* __restrict__ src,
                                                                const uint32_t w, const uint32_t h, float4* __restrict__ dst,
                                                                const uint32_t w2, const uint32_t h2, const uint32_t tiles_x,
                                                                const float threshold) {
    __shared__ float in[IH * IW * 3u];    // [j][i][c]: input pixel (cl(y0 + j), cl(x0 + i))
    __shared__ float rows[TW * IH * 3u];  // [x'][j][c]: the row sum of input row j at output column x'
    const uint32_t tid = threadIdx.x;
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    const int64_t x0 = int64_t(bx * TW) * 2 - 2, y0 = int64_t(by * TH) * 2 - 2;
    for (uint32_t t = tid; t < IW * IH; t += kThreads) {
        const uint32_t j = t / IW, i = t - j * IW;
        const size_t p = size_t(cl(y0 + int64_t(j), h)) * w + cl(x0 + int64_t(i), w);
        float o[3];
        if (FIRST) {
            const float* const px = image + p * 3u;
            bright(px[0], px[1], px[2], threshold, o);
        } else {
            const float4 v = src[p];
            o[0] = v.x, o[1] = v.y, o[2] = v.z;
        }
        in[t * 3u] = o[0], in[t * 3u + 1u] = o[1], in[t * 3u + 2u] = o[2];
    }
    __syncthreads();
    for (uint32_t t = tid; t < TW * IH; t += kThreads) {  // (j runs fastest: lanes are 105 words apart in `in`, 3 in `rows`)
        const uint32_t xo = t / IH, j = t - xo * IH;
        const float* const f = in + (j * IW + 2u * xo) * 3u;
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c)
            rows[t * 3u + c] = ((((f[c] + (4.0f * f[3u + c])) + (6.0f * f[6u + c])) + (4.0f * f[9u + c])) + f[12u + c]) * 0.0625f;
    }
    __syncthreads();
    const uint32_t lx = tid % TW, ly = tid / TW;
    const uint32_t ox = bx * TW + lx, oy = by * TH + ly;
    if (ox >= w2 || oy >= h2) return;
    const float* const r = rows + (lx * IH + 2u * ly) * 3u;
    float o[3];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c)
        o[c] = ((((r[c] + (4.0f * r[3u + c])) + (6.0f * r[6u + c])) + (4.0f * r[9u + c])) + r[12u + c]) * 0.0625f;
    dst[size_t(oy) * w2 + ox] = make_float4(o[0], o[1], o[2], 0.0f);
}

// Coarse pixels (cl(ky0 + j), cl(kx0 + i)), j < rows, i < cols, to g[j][i][c].
__device__ __forceinline__ void stage_coarse(const float4* __restrict__ coarse, uint32_t cw, uint32_t ch, int64_t kx0, int64_t ky0,
                                             uint32_t cols, uint32_t rows, float* g) {
    for (uint32_t t = threadIdx.x; t < cols * rows; t += kThreads) {
        const uint32_t j = t / cols, i = t - j * cols;
        const float4 v = coarse[size_t(cl(ky0 + int64_t(j), ch)) * cw + cl(kx0 + int64_t(i), cw)];
        g[t * 3u] = v.x, g[t * 3u + 1u] = v.y, g[t * 3u + 2u] = v.z;
    }
}

// EXPAND at one pixel, rows first: g is a staged coarse tile of `cols` columns; (lk, lr) is the pixel's own coarse pixel
// (x >> 1, y >> 1) in it, with a staged neighbour on every side.
__device__ __forceinline__ void expand_at(const float* g, uint32_t cols, uint32_t lk, uint32_t lr, bool x_odd, bool y_odd, float e[3]) {
    float row[3][3];  // [which of the rows lr - 1, lr, lr + 1][c]
#pragma unroll
    for (uint32_t q = 0; q < 3u; ++q) {
        if (q == 0u && y_odd) continue;  // (an odd y reads rows lr and lr + 1 only)
        const float* const p = g + ((lr + q - 1u) * cols + lk) * 3u;
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c)
            row[q][c] = x_odd ? (p[c] + p[3u + c]) * 0.5f : ((p[int(c) - 3] + (6.0f * p[c])) + p[3u + c]) * 0.125f;
    }
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c)
        e[c] = y_odd ? (row[1][c] + row[2][c]) * 0.5f : ((row[0][c] + (6.0f * row[1][c])) + row[2][c]) * 0.125f;
}

__global__ __launch_bounds__(kThreads) void glare_expand_add_kernel(const float4* __restrict__ coarse, const uint32_t cw, const uint32_t ch,
                                                                    float4* __restrict__ fine, const uint32_t w, const uint32_t h,
                                                                    const uint32_t tiles_x, const float spread) {
    __shared__ float g[ECH * ECW * 3u];
    const uint32_t tid = threadIdx.x;
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    stage_coarse(coarse, cw, ch, int64_t(bx * (EW / 2u)) - 1, int64_t(by * (EH / 2u)) - 1, ECW, ECH, g);
    __syncthreads();
    const uint32_t lx = tid % EW, ly = tid / EW;
    const uint32_t x = bx * EW + lx, y = by * EH + ly;
    if (x >= w || y >= h) return;
    float e[3];
    expand_at(g, ECW, (lx >> 1) + 1u, (ly >> 1) + 1u, (lx & 1u) != 0u, (ly & 1u) != 0u, e);
    float4* const px = fine + (size_t(y) * w + x);
    const float4 d = *px;
    *px = make_float4(d.x + (spread * e[0]), d.y + (spread * e[1]), d.z + (spread * e[2]), 0.0f);
}

template <bool Vec>
__global__ __launch_bounds__(kThreads) void glare_composite_kernel(const GlareParams G, const float4* __restrict__ g1, const uint32_t cw,
                                                                   const uint32_t ch, const uint32_t tiles_x) {
    __shared__ float g[CCH * CCW * 3u];
    const uint32_t tid = threadIdx.x;
    const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
    stage_coarse(g1, cw, ch, int64_t(bx * (CW / 2u)) - 1, int64_t(by * (CH / 2u)) - 1, CCW, CCH, g);
    __syncthreads();
    const uint32_t lx = tid % (CW / CGROUP), ly = tid / (CW / CGROUP);
    const uint32_t x = bx * CW + lx * CGROUP, y = by * CH + ly;
    if (x >= G.width || y >= G.height) return;
    const uint32_t have = G.width - x < CGROUP ? G.width - x : CGROUP;  // (Vec: the width is a multiple of 4, have == 4)
    const size_t first = (size_t(y) * G.width + x) * 3u;
    float p[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // a thread reads its own X before it writes: the output may be the input
    if (Vec) {
        const float4* const v = reinterpret_cast<const float4*>(G.in + first);
        const float4 a = v[0], b = v[1], c = v[2];
        p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w, p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
        p[8] = c.x, p[9] = c.y, p[10] = c.z, p[11] = c.w;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 12u; ++i)  // (fixed indices: p stays in registers)
            if (i < have * 3u) p[i] = G.in[first + i];
    }
#pragma unroll
    for (uint32_t q = 0; q < CGROUP; ++q) {
        float b[3], e[3];
        bright(p[3u * q], p[3u * q + 1u], p[3u * q + 2u], G.threshold, b);
        expand_at(g, CCW, lx * 2u + (q >> 1) + 1u, (ly >> 1) + 1u, (q & 1u) != 0u, (ly & 1u) != 0u, e);
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) p[3u * q + c] = (p[3u * q + c] - (G.intensity * b[c])) + (G.a * e[c]);
    }
    if (G.out_radiance) {
        float* const dst = G.out_radiance + first;
        if (Vec) {
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
    if (G.out_rgb8) {
        uint8_t* const dst = G.out_rgb8 + first;
        if (Vec) {
            uint32_t* const v = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[k] = quantise(p[4 * k]) | (quantise(p[4 * k + 1]) << 8) | (quantise(p[4 * k + 2]) << 16) | (quantise(p[4 * k + 3]) << 24);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 12u; ++i)
                if (i < have * 3u) dst[i] = uint8_t(quantise(p[i]));
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

uint32_t tiles(uint32_t n, uint32_t tile) { return (n + tile - 1u) / tile; }

}  // namespace

// (the arguments have been checked: rbrt_hip_glare. width * height < 2^31, so no grid below reaches 2^31 workgroups.)
hipError_t launch_glare(const GlareParams& G, hipStream_t stream) {
    if (!G.out_radiance && !G.out_rgb8) return hipSuccess;
    uint32_t w[RBRT_GLARE_MAX_LEVELS + 1u], h[RBRT_GLARE_MAX_LEVELS + 1u];
    float4* level[RBRT_GLARE_MAX_LEVELS + 1u];
    w[0] = G.width, h[0] = G.height, level[0] = nullptr;
    float4* next = static_cast<float4*>(G.workspace);
    for (uint32_t l = 1; l <= G.levels; ++l) {
        w[l] = (w[l - 1u] + 1u) / 2u, h[l] = (h[l - 1u] + 1u) / 2u;
        level[l] = next;
        next += size_t(w[l]) * h[l];
    }
    const dim3 block(kThreads);
    for (uint32_t l = 1; l <= G.levels; ++l) {
        const uint32_t tx = tiles(w[l], TW);
        const dim3 grid(tx * tiles(h[l], TH));
        if (l == 1u)
            hipLaunchKernelGGL(glare_reduce_kernel<true>, grid, block, 0, stream, G.in, static_cast<const float4*>(nullptr), w[0], h[0], level[1],
                               w[1], h[1], tx, G.threshold);
        else
            hipLaunchKernelGGL(glare_reduce_kernel<false>, grid, block, 0, stream, static_cast<const float*>(nullptr),
                               static_cast<const float4*>(level[l - 1u]), w[l - 1u], h[l - 1u], level[l], w[l], h[l], tx, 0.0f);
    }
    for (uint32_t l = G.levels - 1u; l >= 1u; --l) {
        const uint32_t tx = tiles(w[l], EW);
        hipLaunchKernelGGL(glare_expand_add_kernel, dim3(tx * tiles(h[l], EH)), block, 0, stream, static_cast<const float4*>(level[l + 1u]),
                           w[l + 1u], h[l + 1u], level[l], w[l], h[l], tx, G.spread);
    }
    const uint32_t tx = tiles(G.width, CW);
    const dim3 grid(tx * tiles(G.height, CH));
    const bool vec = G.width % CGROUP == 0u && aligned(G.in, 16) && aligned(G.out_radiance, 16) && aligned(G.out_rgb8, 4);
    if (vec) hipLaunchKernelGGL(glare_composite_kernel<true>, grid, block, 0, stream, G, static_cast<const float4*>(level[1]), w[1], h[1], tx);
    else hipLaunchKernelGGL(glare_composite_kernel<false>, grid, block, 0, stream, G, static_cast<const float4*>(level[1]), w[1], h[1], tx);
    return hipGetLastError();
}

}  // namespace rbrt
