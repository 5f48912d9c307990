// temporal.hip — the temporal accumulation of include/rbrt_hip.h "Temporal accumulation" for gfx950 (MI355X / CDNA4).
//
// A translation unit of its own: nothing here is seen by kernels.hip, megakernel.inl, features.inl or guided.hip, whose code
// stays as it is. The arithmetic is the header's rule operation by operation: f32, no FMA (-ffp-contract=off and the pragma
// below), the compiler's correctly rounded `/` and sqrt (-fno-fast-math; no reciprocal shortcut), every sum in the rule's order.
//
// A history is three planes of one float4 a pixel: {A'.rgb, len}, {B'.rgb, c}, {N.xyz, z}. A tap is then three aligned 16-byte
// loads instead of twelve scalar ones.
//
// temporal_kernel: one thread per pixel, pixels in row-major order, a workgroup of 256 (RBRT_TEMPORAL_BLOCK) takes 256
//   consecutive ones. There is no tile: the 64 lanes of a wave read 768 contiguous bytes of A, B and N and write 1 KiB of each
//   history plane, which is the widest access there is (16 bytes a lane), and under a slow camera they reproject onto
//   neighbouring pixels of one or two rows, so the four taps of a wave fall into the same few cache lines of a plane. The taps
//   are accumulated sequentially in the rule's order: no atomics, no cross-lane sums, no LDS. A thread reads its own pixel of
//   A and B before it writes, so an output may lie on its input. Every tap index is tested against the image as an integer
//   before it is used: no read leaves the buffers whatever the floats are.
//   Two builds: temporal_kernel<false> is the rule of "Temporal accumulation" and what rbrt_hip_temporal_accumulate has always
//   launched; temporal_kernel<true> (rbrt_hip_temporal_accumulate_moving with a motion buffer) reads 12 more bytes a pixel, the
//   pixel's own mean travel, and looks the history up where the surface WAS: one division per component, a product and a
//   difference in front of v. Whatever the motion's floats are they only move xs and ys, which are tested as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"
#include "../../include/rbrt_hip.h"
#include "../../include/rbrt_hip_debug.h"

#pragma clang fp contract(off)

namespace rbrt {

namespace {

constexpr int kThreads = int(RBRT_TEMPORAL_BLOCK);

struct F3 {
    float x, y, z;
};
__device__ __forceinline__ F3 f3(const float* p) { return F3{p[0], p[1], p[2]}; }
__device__ __forceinline__ float dot(F3 a, F3 b) { return ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z); }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 operator*(float s, F3 a) { return F3{s * a.x, s * a.y, s * a.z}; }

struct Sums {
    float ws, sa[3], sb[3], sl;
};

template <bool MOVING>
__global__ __launch_bounds__(kThreads) void temporal_kernel(const TemporalParams T) {
    const size_t npix = size_t(T.width) * T.height;
    const size_t p = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (p >= npix) return;
    const int W = int(T.width), H = int(T.height);
    const float A[3] = {T.a[p * 3 + 0], T.a[p * 3 + 1], T.a[p * 3 + 2]};
    const float B[3] = {T.b[p * 3 + 0], T.b[p * 3 + 1], T.b[p * 3 + 2]};
    const F3 N = f3(T.normal + p * 3);
    const float z = T.depth[p], c = T.coverage[p];
    float oa[3] = {A[0], A[1], A[2]}, ob[3] = {B[0], B[1], B[2]}, len = 1.0f;

    if (T.history_in) {
        const float4* const h_a = static_cast<const float4*>(T.history_in);
        const float4* const h_b = h_a + npix;
        const float4* const h_n = h_b + npix;
        const int row = int(p / T.width), col = int(p - size_t(row) * T.width);
        // the centre ray of the pixel in K
        const F3 pos = f3(T.pos);
        const float cm = (float(col) - T.hx) * T.mm_hor, rm = (float(row) - T.hy) * T.mm_vert;
        const F3 target = (f3(T.center) + ((0.001f * cm) * f3(T.right))) - ((0.001f * rm) * f3(T.up));
        const F3 e = target - pos;
        const float elen = __builtin_sqrtf(dot(e, e));
        const F3 d = F3{e.x / elen, e.y / elen, e.z / elen};
        // the point
        const bool surface = c > 0.0f;
        F3 v = d;
        if (surface) {
            const float zbar = z / c;
            F3 P = pos + (zbar * d);
            if (MOVING) {  // "Animation": the point where it was when the last frame's shutter opened
                const F3 mv = f3(T.motion + p * 3);
                const F3 m = F3{mv.x / c, mv.y / c, mv.z / c};
                P = P - (T.phase_step * m);
            }
            v = P - f3(T.pos_prev);
        }
        // its projection into K'
        const float t = T.wn / dot(v, f3(T.n));
        const F3 Q = (t * v) - f3(T.w);
        const float qr = dot(Q, f3(T.right_prev)), qu = dot(Q, f3(T.up_prev));
        const float ca = ((qr * T.uu) - (qu * T.ru)) / T.det, cb = ((qr * T.ru) - (qu * T.rr)) / T.det;
        const float xs = (ca / T.sx) + T.hx, ys = (cb / T.sy) + T.hy;
        const bool projects = t > 0.0f && t < __builtin_inff() && xs > -1.0f && xs < float(W) && ys > -1.0f && ys < float(H);
        if (projects) {  // (every compare above is false for a NaN: xs and ys are finite and in (-1, W) x (-1, H) here)
            const float fi = __builtin_floorf(xs), fj = __builtin_floorf(ys);
            const int i = int(fi), j = int(fj);
            const float fx = xs - fi, fy = ys - fj;
            const float gx = 1.0f - fx, gy = 1.0f - fy;
            const float ze = __builtin_sqrtf(dot(v, v));
            const float ztol = T.kz * ze;
            const float bw[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
            Sums S = {0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qy = j + (k >> 1), qx = i + (k & 1);
                if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
                const size_t q = size_t(qy) * size_t(W) + size_t(qx);
                const float4 ra = h_a[q], rb = h_b[q], rn = h_n[q];
                const float cq = rb.w;
                bool accepted;
                if (surface) {
                    const float zq = rn.w / cq;
                    const F3 D = N - F3{rn.x, rn.y, rn.z};
                    accepted = cq > 0.0f && __builtin_fabsf(zq - ze) <= ztol && dot(D, D) <= T.kn2;
                } else {
                    accepted = cq == 0.0f;
                }
                if (!accepted) continue;
                S.ws = S.ws + bw[k];
                S.sa[0] = S.sa[0] + bw[k] * ra.x;
                S.sa[1] = S.sa[1] + bw[k] * ra.y;
                S.sa[2] = S.sa[2] + bw[k] * ra.z;
                S.sb[0] = S.sb[0] + bw[k] * rb.x;
                S.sb[1] = S.sb[1] + bw[k] * rb.y;
                S.sb[2] = S.sb[2] + bw[k] * rb.z;
                S.sl = S.sl + bw[k] * ra.w;
            }
            if (S.ws >= 0.01f) {
                const float hl = S.sl / S.ws;
                len = __builtin_fminf(hl + 1.0f, T.max_history);
                const float alpha = 1.0f / len;
                for (int ch = 0; ch < 3; ++ch) {
                    const float ha = S.sa[ch] / S.ws, hb = S.sb[ch] / S.ws;
                    oa[ch] = ha + (alpha * (A[ch] - ha));
                    ob[ch] = hb + (alpha * (B[ch] - hb));
                }
            }
        }
    }

    if (T.history_out) {
        float4* const o_a = static_cast<float4*>(T.history_out);
        float4* const o_b = o_a + npix;
        float4* const o_n = o_b + npix;
        o_a[p] = make_float4(oa[0], oa[1], oa[2], len);
        o_b[p] = make_float4(ob[0], ob[1], ob[2], c);
        o_n[p] = make_float4(N.x, N.y, N.z, z);
    }
    if (T.out_a) {
        T.out_a[p * 3 + 0] = oa[0];
        T.out_a[p * 3 + 1] = oa[1];
        T.out_a[p * 3 + 2] = oa[2];
    }
    if (T.out_b) {
        T.out_b[p * 3 + 0] = ob[0];
        T.out_b[p * 3 + 1] = ob[1];
        T.out_b[p * 3 + 2] = ob[2];
    }
    if (T.out_length) T.out_length[p] = len;
}

}  // namespace

// (the arguments have been checked: rbrt_hip_temporal_accumulate, rbrt_hip_temporal_accumulate_moving; T.motion chooses the build)
hipError_t launch_temporal(const TemporalParams& T, hipStream_t stream) {
    const size_t npix = size_t(T.width) * T.height;
    if (npix == 0 || npix >= (size_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 grid(uint32_t((npix + kThreads - 1) / kThreads));
    if (T.motion) hipLaunchKernelGGL(temporal_kernel<true>, grid, dim3(kThreads), 0, stream, T);
    else hipLaunchKernelGGL(temporal_kernel<false>, grid, dim3(kThreads), 0, stream, T);
    return hipGetLastError();
}

}  // namespace rbrt
