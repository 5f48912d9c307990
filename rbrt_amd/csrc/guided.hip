// guided.hip — the feature-guided a-trous filter of include/rbrt_hip.h "Guided denoising" for gfx950 (MI355X / CDNA4).
//
// A translation unit of its own: nothing here is seen by kernels.hip or megakernel.inl, whose code stays as it is.
// The arithmetic is the header's rule operation by operation: f32, no FMA (-ffp-contract=off and the pragma below), the
// compiler's correctly rounded `/` (-fno-fast-math; no reciprocal shortcut), every sum in the rule's order.
//
// The workspace holds six planes of one float4 a pixel: {N.xyz, z}, {m.rgb, 0}, and two sets of {I.rgb, 0}, {V.rgb, 0} which
// the levels read and write in turns. A tap is then four aligned 16-byte loads instead of thirteen scalar ones, and a wave's
// 16 pixels of a row read 256 contiguous bytes of each plane.
//
// guided_prepare_kernel: one thread per pixel. Packs the guides, divides the albedo out, mixes the halves into I and takes V
//   from the 3 x 3 neighbourhood of the halves in global memory. It is the only kernel that reads the caller's inputs, so an
//   output may lie on a half image.
// guided_level_kernel<LAST, STAGED>: one thread per output pixel, a workgroup of 256 covers a 16 x 16 pixel tile
//   (RBRT_GUIDED_TILE). The 25 taps of a pixel are accumulated sequentially in the rule's order: no atomics, no cross-lane
//   sums. STAGED: the tile plus its halo of 2 * step goes to LDS first, plane by plane (a row of 16 pixels reads 16
//   consecutive 16-byte slots: no bank conflict), and the taps read LDS; else the taps read global memory. Both forms feed
//   the same values to the same arithmetic. LAST multiplies the albedo back, quantises and skips V'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kTile = int(RBRT_GUIDED_TILE);
constexpr int kThreads = kTile * kTile;
constexpr float kEps = 1e-7f;
constexpr float kFloor = 0.01f;
constexpr int kMaxStagedStep = 4;  // (16 + 4 * 4)^2 pixels * 64 B = 64 KiB of the CU's 160 KiB

// lib.rs:116-122: (sqrt(c) * 256) as u8 -- the cast saturates and maps NaN to 0 (kernels.hip and denoise.hip have the same
// function; it is repeated here so that this file shares no code with them).
__device__ __forceinline__ uint8_t quantise(float c) {
    float v = __builtin_sqrtf(c) * 256.0f;
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return uint8_t(v);
}

__device__ __forceinline__ bool inside(int y, int x, int h, int w) { return y >= 0 && y < h && x >= 0 && x < w; }

struct Planes {
    float4* nz;     // {N.xyz, z}
    float4* m;      // {m.rgb, 0}
    float4* iv[4];  // I0, V0, I1, V1
};

__device__ __host__ __forceinline__ Planes planes_of(void* workspace, size_t npix) {
    float4* const w = static_cast<float4*>(workspace);
    Planes P;
    P.nz = w, P.m = w + npix;
    for (int k = 0; k < 4; ++k) P.iv[k] = w + npix * size_t(2 + k);
    return P;
}

__global__ __launch_bounds__(kThreads) void guided_prepare_kernel(const GuidedParams G) {
    const int W = int(G.width), H = int(G.height);
    const size_t npix = size_t(G.width) * G.height;
    const size_t i = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= npix) return;
    const int py = int(i / G.width), px = int(i - size_t(py) * G.width);
    const bool demodulate = (G.flags & RBRT_GUIDED_NO_DEMODULATION) == 0u;
    float sum[3] = {0.0f, 0.0f, 0.0f}, m[3] = {0.0f, 0.0f, 0.0f}, I[3] = {0.0f, 0.0f, 0.0f};
    int count = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int ny = py + dy, nx = px + dx;
            if (!inside(ny, nx, H, W)) continue;
            const size_t o = size_t(ny) * size_t(W) + size_t(nx);
            const float bare = 1.0f - G.coverage[o];
            const bool own = dy == 0 && dx == 0;
            for (int c = 0; c < 3; ++c) {
                const float mc = fmaxf(G.albedo[o * 3 + c] + bare, kFloor);
                const float u = demodulate ? mc : 1.0f;
                const float a = G.a[o * 3 + c] / u, b = G.b[o * 3 + c] / u;
                const float d = a - b;
                sum[c] = sum[c] + d * d;
                if (own) {
                    const float wa = G.wa ? G.wa[o] : 0.5f;
                    m[c] = mc;
                    I[c] = (a * wa) + (b * (1.0f - wa));
                }
            }
            ++count;
        }
    const Planes P = planes_of(G.workspace, npix);
    const float n = float(count);
    P.nz[i] = make_float4(G.normal[i * 3 + 0], G.normal[i * 3 + 1], G.normal[i * 3 + 2], G.depth[i]);
    P.m[i] = make_float4(m[0], m[1], m[2], 0.0f);
    P.iv[0][i] = make_float4(I[0], I[1], I[2], 0.0f);
    P.iv[1][i] = make_float4((sum[0] / n) * 0.25f, (sum[1] / n) * 0.25f, (sum[2] / n) * 0.25f, 0.0f);
}

struct Level {
    const float4* nz;
    const float4* m;
    const float4* in_i;
    const float4* in_v;
    float4* out_i;  // null in the last level
    float4* out_v;
    float* out_radiance;  // the last level's outputs, each may be null
    uint8_t* out_rgb8;
    uint32_t width, height, tiles_x;
    int32_t step;
    uint32_t flags;
    float kc2, kz2, in, ia;
};

struct Accum {
    float num[3], nv[3], den;
};

// One tap of the rule: the pixel's own records p*, the tap's q*, the B-spline weight hh.
template <bool LAST>
__device__ __forceinline__ void tap(const Level& L, float hh, const float4 pnz, const float4 pm, const float4 pi, const float4 pv,
                                    const float4 qnz, const float4 qm, const float4 qi, const float4 qv, Accum& S) {
    const float nx = qnz.x - pnz.x, ny = qnz.y - pnz.y, nzz = qnz.z - pnz.z;
    const float Dn = (((nx * nx) + (ny * ny)) + (nzz * nzz)) * L.in;
    const float ar = qm.x - pm.x, ag = qm.y - pm.y, ab = qm.z - pm.z;
    const float Da = (((ar * ar) + (ag * ag)) + (ab * ab)) * L.ia;
    const float dz = qnz.w - pnz.w;
    const float Dz = (dz * dz) / (kEps + (L.kz2 * (pnz.w * qnz.w)));
    const float gr = qi.x - pi.x, gg = qi.y - pi.y, gb = qi.z - pi.z;
    const float tr = (gr * gr) / (kEps + (L.kc2 * (pv.x + qv.x)));
    const float tg = (gg * gg) / (kEps + (L.kc2 * (pv.y + qv.y)));
    const float tb = (gb * gb) / (kEps + (L.kc2 * (pv.z + qv.z)));
    const float Dc = ((tr + tg) + tb) * 0.33333334f;
    const float D = ((Dn + Dz) + Da) + Dc;
    const float f = fmaxf(0.0f, 1.0f - 0.25f * fmaxf(D, 0.0f));
    const float w = hh * ((f * f) * (f * f));
    S.num[0] = S.num[0] + w * qi.x;
    S.num[1] = S.num[1] + w * qi.y;
    S.num[2] = S.num[2] + w * qi.z;
    if (!LAST) {
        const float w2 = w * w;
        S.nv[0] = S.nv[0] + w2 * qv.x;
        S.nv[1] = S.nv[1] + w2 * qv.y;
        S.nv[2] = S.nv[2] + w2 * qv.z;
    }
    S.den = S.den + w;
}

template <bool LAST, bool STAGED>
__global__ __launch_bounds__(kThreads) void guided_level_kernel(const Level L) {
    extern __shared__ float4 lds4[];
    const int H = int(L.height), W = int(L.width), s = L.step;
    const int tid = int(threadIdx.x);
    const int tile_y = int(blockIdx.x / L.tiles_x), tile_x = int(blockIdx.x - uint32_t(tile_y) * L.tiles_x);
    const int y0 = tile_y * kTile, x0 = tile_x * kTile;
    const int halo = 2 * s, SW = kTile + 2 * halo;  // (STAGED) the staged edge
    if (STAGED) {
        // four planes of SW * SW float4; pixels outside the image are left as they are and never read
        for (int idx = tid; idx < SW * SW; idx += kThreads) {
            const int sy = idx / SW, sx = idx - sy * SW;
            const int gy = y0 - halo + sy, gx = x0 - halo + sx;
            if (!inside(gy, gx, H, W)) continue;
            const size_t g = size_t(gy) * size_t(W) + size_t(gx);
            lds4[idx] = L.nz[g];
            lds4[SW * SW + idx] = L.m[g];
            lds4[2 * SW * SW + idx] = L.in_i[g];
            lds4[3 * SW * SW + idx] = L.in_v[g];
        }
        __syncthreads();
    }
    const int ty = tid / kTile, tx = tid - ty * kTile;
    const int py = y0 + ty, px = x0 + tx;
    if (py >= H || px >= W) return;  // (behind the only barrier)
    const size_t p = size_t(py) * size_t(W) + size_t(px);
    const float4 pnz = L.nz[p], pm = L.m[p], pi = L.in_i[p], pv = L.in_v[p];
    Accum S = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qy = py + j * s, qx = px + i * s;
            if (!inside(qy, qx, H, W)) continue;
            const float hh = h[j + 2] * h[i + 2];
            if (STAGED) {
                const int idx = (ty + halo + j * s) * SW + (tx + halo + i * s);
                tap<LAST>(L, hh, pnz, pm, pi, pv, lds4[idx], lds4[SW * SW + idx], lds4[2 * SW * SW + idx], lds4[3 * SW * SW + idx], S);
            } else {
                const size_t q = size_t(qy) * size_t(W) + size_t(qx);
                tap<LAST>(L, hh, pnz, pm, pi, pv, L.nz[q], L.m[q], L.in_i[q], L.in_v[q], S);
            }
        }
    }
    float I[3];
    for (int c = 0; c < 3; ++c) I[c] = S.num[c] / S.den;
    if (!LAST) {
        const float d2 = S.den * S.den;
        L.out_i[p] = make_float4(I[0], I[1], I[2], 0.0f);
        L.out_v[p] = make_float4(S.nv[0] / d2, S.nv[1] / d2, S.nv[2] / d2, 0.0f);
        return;
    }
    const bool demodulate = (L.flags & RBRT_GUIDED_NO_DEMODULATION) == 0u;
    const float u[3] = {demodulate ? pm.x : 1.0f, demodulate ? pm.y : 1.0f, demodulate ? pm.z : 1.0f};
    float out[3];
    for (int c = 0; c < 3; ++c) out[c] = I[c] * u[c];
    if (L.out_radiance) {
        L.out_radiance[p * 3 + 0] = out[0];
        L.out_radiance[p * 3 + 1] = out[1];
        L.out_radiance[p * 3 + 2] = out[2];
    }
    if (L.out_rgb8) {
        L.out_rgb8[p * 3 + 0] = quantise(out[0]);
        L.out_rgb8[p * 3 + 1] = quantise(out[1]);
        L.out_rgb8[p * 3 + 2] = quantise(out[2]);
    }
}

template <bool LAST, bool STAGED>
hipError_t launch_level(const Level& L, hipStream_t stream) {
    const int sw = kTile + 4 * L.step;
    const size_t lds_bytes = STAGED ? size_t(sw) * sw * 4u * sizeof(float4) : 0u;
    if (STAGED) {  // (64 KiB at step 4: above the default limit)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&guided_level_kernel<LAST, STAGED>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes));
        if (e != hipSuccess) return e;
    }
    const uint32_t tiles_y = (L.height + kTile - 1) / kTile;
    hipLaunchKernelGGL((guided_level_kernel<LAST, STAGED>), dim3(L.tiles_x * tiles_y), dim3(kThreads), lds_bytes, stream, L);
    return hipGetLastError();
}

}  // namespace

// (the arguments have been checked: rbrt_hip_denoise_guided). staged_max_step: the levels whose step is at most that stage
// their tile in LDS (0: none; at most 4).
hipError_t launch_guided(const GuidedParams& G, uint32_t staged_max_step, hipStream_t stream) {
    if (G.levels == 0u || G.levels > RBRT_GUIDED_MAX_LEVELS || staged_max_step > uint32_t(kMaxStagedStep)) return hipErrorInvalidValue;
    const size_t npix = size_t(G.width) * G.height;
    if (npix == 0 || npix >= (size_t(1) << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guided_prepare_kernel, dim3(uint32_t((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, G);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const Planes P = planes_of(G.workspace, npix);
    Level L;
    L.nz = P.nz, L.m = P.m;
    L.width = G.width, L.height = G.height, L.tiles_x = (G.width + kTile - 1) / kTile;
    L.flags = G.flags, L.kc2 = G.kc2, L.kz2 = G.kz2, L.in = G.in, L.ia = G.ia;
    for (uint32_t l = 0; l < G.levels; ++l) {
        const bool last = l + 1u == G.levels;
        const uint32_t from = l % 2u, to = 1u - from;
        L.in_i = P.iv[2 * from], L.in_v = P.iv[2 * from + 1];
        L.out_i = last ? nullptr : P.iv[2 * to], L.out_v = last ? nullptr : P.iv[2 * to + 1];
        L.out_radiance = last ? G.out_radiance : nullptr, L.out_rgb8 = last ? G.out_rgb8 : nullptr;
        L.step = int32_t(1u << l);
        const bool staged = uint32_t(L.step) <= staged_max_step;
        e = last ? (staged ? launch_level<true, true>(L, stream) : launch_level<true, false>(L, stream))
                 : (staged ? launch_level<false, true>(L, stream) : launch_level<false, false>(L, stream));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rbrt
