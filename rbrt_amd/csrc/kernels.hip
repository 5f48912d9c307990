// kernels.hip — gfx950 (MI355X / CDNA4) kernels of the rbrt path-tracing hot path.
//
// What runs here is the whole of the reference's L1 layer for one (pixel, sample):
//   camera ray        cam.rs:64-82
//   closest hit       scene.rs:19-43 -> sphere.rs:20-66, mesh.rs:225-267 (gate aabbox.rs:28-58,
//                     Moller-Trumbore triangle.rs:189-255, arg-min triangle.rs:392-410)
//   scatter           lambertian.rs:11-24, metal.rs:12-25, dielectric.rs:11-85, materials.rs:14-37
//   integrator        lib.rs:43-73 (depth 50, sky gradient), per-pixel mean lib.rs:95-101,
//                     quantisation lib.rs:116-122
// Arithmetic follows the reference operation by operation (f32, mul-then-add, no FMA on any value
// that reaches the image: this file is compiled with -ffp-contract=off, and IEEE-correct / and sqrt)
// so that the radiance matches the CPU restatement of the reference bit for bit. The only place
// the GPU does something the reference does not is culling: triangles are found through a BVH
// instead of a scan over all of them, with node boxes inflated by a per-ray error bound so that no
// triangle the scan would accept can be skipped (mesh_closest below).
//
// Wave64 only; no MFMA (there is no dense contraction on this path).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.h"

#pragma clang fp contract(off)

namespace rbrt {

// ---------------------------------------------------------------------------------------------
// Vec3 with the reference's evaluation order (vec3.rs:12-160)
// ---------------------------------------------------------------------------------------------
struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 mk(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 b) { return V3{s * b.x, s * b.y, s * b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// ---- IEEE square root and division, the short way ----------------------------------------------------------
// The image needs correctly rounded sqrt and / (the reference's f32::sqrt and `/`). hipcc's expansions are 17 and
// 13 instructions: v_sqrt / v_rcp plus correction steps, wrapped in range handling (input scaling for tiny
// operands, v_div_scale / v_div_fixup, class checks for 0 and inf). For operands in the everyday range that
// wrapping is the identity, and the correction steps -- reproduced below instruction for instruction -- give the same
// bits. A wave takes the short forms when EVERY active lane's operands are in range (one compare or two per call) and
// the compiler's forms otherwise. tests: test_short_ieee_forms_match_the_compilers (2^28 operands), test_ieee_domain.py (every
// float of sqrt_core's domain; normalize at the edges of its gate), test_ieee_model.py (the division in exact arithmetic).
__device__ __forceinline__ float sqrt_core(float x) {  // x in (2^-80, 2^100): hipcc's sqrt without its scaling / class steps
    const float r = __builtin_amdgcn_sqrtf(x);
    const float r_dn = __uint_as_float(__float_as_uint(r) - 1u), r_up = __uint_as_float(__float_as_uint(r) + 1u);
    const float e_dn = __builtin_fmaf(-r_dn, r, x), e_up = __builtin_fmaf(-r_up, r, x);
    float s = e_dn <= 0.0f ? r_dn : r;
    s = e_up > 0.0f ? r_up : s;
    return s;
}
__device__ __forceinline__ bool sqrt_in_range(float x) { return x > 0x1p-80f && x < 0x1p100f; }  // (false for NaN)
// short_path: whether this lane's wave took sqrt_core (test hooks read it; the other overload drops it)
__device__ __forceinline__ float ieee_sqrt(float x, bool& short_path) {
    short_path = __builtin_amdgcn_ballot_w64(!sqrt_in_range(x)) == 0ull;
    return short_path ? sqrt_core(x) : __builtin_sqrtf(x);
}
__device__ __forceinline__ float ieee_sqrt(float x) {
    bool short_path;
    return ieee_sqrt(x, short_path);
}
__device__ __forceinline__ float length(V3 a) { return ieee_sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); }
__device__ __attribute__((noinline)) V3 normalize_ieee(V3 a) {  // the compiler's forms, out of line: the rare path
    const float len = __builtin_sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z);
    return V3{a.x / len, a.y / len, a.z / len};
}
// normalize's gate: s = |a|^2 in (kNormSLo, kNormSHi) and every |component| > kNormMin. The upper bound is not
// sqrt_in_range's 2^100: the short division rounds a subnormal quotient on its own, and gets about half of the quotients on
// a subnormal midpoint wrong (x = (27 2^-104, 3 2^46, 27 2^-104): 5 2^-149 for 4 2^-149); the compiler's v_div_scale
// scales those. len < 2^26 keeps every quotient of the short path normal. (tests: test_ieee_model.py, test_ieee_domain.py)
constexpr float kNormSLo = 0x1p-80f, kNormSHi = 0x1p52f, kNormMin = 0x1p-100f;
__device__ __forceinline__ V3 normalize(V3 a, bool& short_path) {  // three divisions by the length, vec3.rs:119-126
    const float s = (a.x * a.x + a.y * a.y) + a.z * a.z;
    const float mn = __builtin_fminf(__builtin_fminf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z));
    // in range: no scaling in sqrt; len in [2^-40, 2^26); every |component| > 2^-100 and <= len, so |num/len| is in
    // (2^-126, 1]: normal, and the residuals of the refinement are exact; nothing is 0, inf or NaN
    const bool ok = s > kNormSLo && s < kNormSHi && mn > kNormMin;
    short_path = __builtin_amdgcn_ballot_w64(!ok) == 0ull;
    if (!short_path) return normalize_ieee(a);
    const float len = sqrt_core(s);
    // hipcc's fdiv, minus v_div_scale / v_div_fixup, the reciprocal refinement shared by the three numerators
    float rc = __builtin_amdgcn_rcpf(len);
    rc = __builtin_fmaf(__builtin_fmaf(-len, rc, 1.0f), rc, rc);
    V3 q;
    {
        float v = a.x * rc;
        v = __builtin_fmaf(__builtin_fmaf(-len, v, a.x), rc, v);
        q.x = __builtin_fmaf(__builtin_fmaf(-len, v, a.x), rc, v);
        v = a.y * rc;
        v = __builtin_fmaf(__builtin_fmaf(-len, v, a.y), rc, v);
        q.y = __builtin_fmaf(__builtin_fmaf(-len, v, a.y), rc, v);
        v = a.z * rc;
        v = __builtin_fmaf(__builtin_fmaf(-len, v, a.z), rc, v);
        q.z = __builtin_fmaf(__builtin_fmaf(-len, v, a.z), rc, v);
    }
    return q;
}
__device__ __forceinline__ V3 normalize(V3 a) {
    bool short_path;
    return normalize(a, short_path);
}
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// ---------------------------------------------------------------------------------------------
// Random stream: xoroshiro64** keyed by (seed, pixel, sample); see DESIGN.md "RNG".
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int k) {
    return __builtin_rotateleft32(x, k);
}
struct Rng {
    uint32_t s0, s1;
    __device__ __forceinline__ void init(uint64_t seed_key, uint32_t pixel, uint32_t sample) {
        uint64_t key = splitmix64(seed_key ^ ((uint64_t(pixel) << 32) | uint64_t(sample)));
        s0 = uint32_t(key);
        s1 = uint32_t(key >> 32);
        if ((s0 | s1) == 0) s0 = 1;
    }
    __device__ __forceinline__ uint32_t next_u32() {
        uint32_t r = rotl32(s0 * 0x9E3779BBu, 5) * 5u;
        uint32_t t = s1 ^ s0;
        s0 = rotl32(s0, 26) ^ t ^ (t << 9);
        s1 = rotl32(t, 13);
        return r;
    }
    // 24-bit uniform in [0,1): rand 0.8's Standard distribution for f32
    __device__ __forceinline__ float next_f32() {
        return float(next_u32() >> 8) * (1.0f / 16777216.0f);
    }
};

// ---------------------------------------------------------------------------------------------
// Per-thread counters (counting variant only)
// ---------------------------------------------------------------------------------------------
struct LocalCounters {
    uint32_t rays, gate, nodes, tris, mesh_hits;
};

// ---------------------------------------------------------------------------------------------
// Geometry
// ---------------------------------------------------------------------------------------------

// sphere.rs:20-66. Returns true on hit with the ray parameter and the distance.
__device__ __forceinline__ bool sphere_hit(V3 c, float radius, V3 o, V3 d, float min_dist,
                                           float max_dist, float& t_out, float& dist_out,
                                           DevCounters* counters) {
    float a = dot(d, d);
    V3 l = o - c;
    float b = dot(d * 2.0f, l);
    float cc = dot(l, l) - radius * radius;
    float sol = b * b - 4.0f * a * cc;
    if (!(sol >= 0.0f)) {  // negative: a miss. NaN: the reference panics here (sphere.rs:33); count it and miss
        if (sol != sol) atomicAdd(&counters->nan_discriminants, 1ull);
        return false;
    }
    // One square root and one 2a serve both roots (the reference writes them out twice; the second root's block runs
    // behind a wave vote, where the compiler does not merge them). The second division stays: choosing the numerator
    // by the sign of -b - s before a single division needs a gate on its operands, and every form of that gate cost
    // ten more scalar-register spills in the trace kernel (DESIGN.md §6 "Measured and dropped").
    const float s = ieee_sqrt(sol), den = 2.0f * a;
    float t = (-b - s) / den;
    if (sol > 0.0f && t < 0.0f) {
        t = (-b + s) / den;
        if (t < 0.0f) return false;
    }
    V3 p = o + t * d;
    float dist = length(o - p);
    if (dist < min_dist || dist > max_dist) return false;
    t_out = t;
    dist_out = dist;
    return true;
}

// triangle.rs:92-130 (basic_triangle_intersect_w_ray) + :412-441: one BasicTriangle element. Scalar Moller-Trumbore
// with the reference's tests in the reference's order; `(0.0..=1.0).contains(&u)` is false for a NaN u, the other
// compares are false for NaN operands, so a NaN t ends in `t > eps` being false. No upper bound on t but the
// distance window.
__device__ __forceinline__ bool basic_triangle_hit(const float* tri /* v0, e0, e1 */, V3 o, V3 d, float min_dist, float max_dist,
                                                   float& t_out, float& dist_out) {
    const float eps = min_dist;
    const V3 v0 = mk(tri), e0 = mk(tri + 3), e1 = mk(tri + 6);
    const V3 h = cross(d, e1);
    const float a = dot(e0, h);
    if (-eps < a && a < eps) return false;
    const float f = 1.0f / a;
    const V3 s = o - v0;
    const float u = f * dot(s, h);
    if (!(0.0f <= u && u <= 1.0f)) return false;
    const V3 q = cross(s, e0);
    const float v = f * dot(d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = f * dot(e1, q);
    if (!(t > eps)) return false;
    const V3 p = o + t * d;
    const float dist = length(o - p);
    if (dist < min_dist || dist > max_dist) return false;
    t_out = t;
    dist_out = dist;
    return true;
}

// aabbox.rs:28-58, verbatim: six true divisions, NaN-ignoring min/max (fminf/fmaxf = f32::min/max).
__device__ __forceinline__ bool bbox_gate(const float* lo, const float* hi, V3 o, V3 d) {
    float t_lower_x = (lo[0] - o.x) / d.x;
    float t_upper_x = (hi[0] - o.x) / d.x;
    float t_lower_y = (lo[1] - o.y) / d.y;
    float t_upper_y = (hi[1] - o.y) / d.y;
    float t_lower_z = (lo[2] - o.z) / d.z;
    float t_upper_z = (hi[2] - o.z) / d.z;
    float t_min_x = __builtin_fminf(t_lower_x, t_upper_x);
    float t_min_y = __builtin_fminf(t_lower_y, t_upper_y);
    float t_min_z = __builtin_fminf(t_lower_z, t_upper_z);
    float t_min = __builtin_fmaxf(__builtin_fmaxf(t_min_x, t_min_y), t_min_z);
    float t_max_x = __builtin_fmaxf(t_lower_x, t_upper_x);
    float t_max_y = __builtin_fmaxf(t_lower_y, t_upper_y);
    float t_max_z = __builtin_fmaxf(t_lower_z, t_upper_z);
    float t_max = __builtin_fminf(__builtin_fminf(t_max_x, t_max_y), t_max_z);
    if (t_max < 0.0f) return false;
    if (t_min > t_max) return false;
    return true;
}

// The same DECISION as bbox_gate for every input, without the six IEEE divisions on the common path: the quotients
// are formed as (bound - o) * v_rcp_f32(d) (1 ulp reciprocal), each within 2 * 2^-23 relative of the correctly
// rounded quotient bbox_gate computes (the subtraction is the same instruction in both). min / max are monotone, so
// t_min and t_max are within E = 4 * 2^-23 * (largest of the six magnitudes) of bbox_gate's values, and both of its
// tests -- t_max < 0, t_min > t_max -- come out the same whenever |t_max| > E and |t_min - t_max| > 2E. Otherwise
// (a ray grazing an edge of the box within a few ulp, a zero / tiny / huge direction component, non-finite
// quotients) the lane falls back to the IEEE form; the wave takes that branch only when one of its lanes needs it.
// `beyond`: a ray parameter past which no triangle of this mesh could be accepted any more (the ray's closest hit so
// far, relaxed as in the megakernel's refill; +inf when there is none). A box entered only past it is skipped: that is
// not a decision of the reference's gate, it is the traversal's first culling step done here, before the ray is parked.
__device__ __forceinline__ bool bbox_gate_fast(const float* lo, const float* hi, V3 o, V3 d, float beyond = __builtin_inff()) {
    const float rx = __builtin_amdgcn_rcpf(d.x), ry = __builtin_amdgcn_rcpf(d.y), rz = __builtin_amdgcn_rcpf(d.z);
    const float lx = (lo[0] - o.x) * rx, ux = (hi[0] - o.x) * rx;
    const float ly = (lo[1] - o.y) * ry, uy = (hi[1] - o.y) * ry;
    const float lz = (lo[2] - o.z) * rz, uz = (hi[2] - o.z) * rz;
    const float t_min = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(lx, ux), __builtin_fminf(ly, uy)), __builtin_fminf(lz, uz));
    const float t_max = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(lx, ux), __builtin_fmaxf(ly, uy)), __builtin_fmaxf(lz, uz));
    const float m = __builtin_fmaxf(
        __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(lx), __builtin_fabsf(ux)), __builtin_fmaxf(__builtin_fabsf(ly), __builtin_fabsf(uy))),
        __builtin_fmaxf(__builtin_fabsf(lz), __builtin_fabsf(uz)));
    const float E = m * (4.0f / 8388608.0f);
    const float dmin = __builtin_fminf(__builtin_fminf(__builtin_fabsf(d.x), __builtin_fabsf(d.y)), __builtin_fabsf(d.z));
    const float dmax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(d.x), __builtin_fabsf(d.y)), __builtin_fabsf(d.z));
    // every comparison below is false for a NaN operand: anything unusual lands in the exact branch
    const bool sure = (__builtin_fabsf(t_max) > E) && (__builtin_fabsf(t_min - t_max) > 2.0f * E) && (m < 1e30f) && (m > 1e-30f) &&
                      (dmin > 1e-30f) && (dmax < 1e30f) && (d.x == d.x) && (d.y == d.y) && (d.z == d.z);
    bool res = !(t_max < 0.0f) && !(t_min > t_max) && !(t_min - E > beyond);
    if (!sure) res = bbox_gate(lo, hi, o, d);
    return res;
}

// One lane of triangle.rs:189-255. Every compare is an ordered compare (false on NaN) and the
// accept expression has the reference's shape: !(c1 | c2 | c3) & c4.
__device__ __forceinline__ bool tri_test(V3 v0, V3 ea, V3 eb, V3 o, V3 d, float eps, float eps_frac,
                                         float& t_out) {
    V3 h = cross(d, eb);
    float a = dot(ea, h);
    bool c1 = (-eps < a) && (a < eps);
    float f = 1.0f / a;
    V3 s = o - v0;
    float u = f * dot(s, h);
    bool c2 = (u < 0.0f) || (u > 1.0f);
    V3 q = cross(s, ea);
    float v = f * dot(d, q);
    bool c3 = (v < 0.0f) || ((u + v) > 1.0f);
    float t = f * dot(eb, q);
    bool c4 = (t > eps) && (t < eps_frac);
    t_out = t;
    return !(c1 || c2 || c3) && c4;
}

// ---------------------------------------------------------------------------------------------
// BVH traversal pieces shared by the megakernel and the simple per-thread path.
//
// None of this arithmetic reaches the image: it only decides which triangles get tested. So it may
// use FMA and the fast reciprocal / sqrt. Why culling cannot change the result: a triangle accepted by
// tri_test with parameter t has its point o + t*d within
//     err <= ~18 * 2^-24 * (K*|d| + 1) * S        K = |e1||e2| / eps,  S >= |o - v0|
// of the triangle's exact surface (|a| >= eps bounds the amplification of the rounding errors in
// u, v and t). Child boxes are grown by pad = 64 * 2^-24 * (K_subtree*|d| + 1) * (S + |o|_inf), so
// that point is strictly inside every ancestor's grown box (the |o|_inf term covers the o*inv
// product of the FMA form), the slab interval contains t, and `tn <= best_t` (not <) keeps
// equal-t candidates with a lower index reachable.
// Where this has to hold is bounded by the reference itself: tri_test accepts only if |a| >= eps (a ~ twice the area
// times |d| times a cosine) and eps < t < 1 / eps, below the scan's 1e6; for triangle size L, direction length D and hit
// distance rho that is L^2 D >~ eps and eps D < rho < min(D / eps, 1e6 D). tests/cull_families.py sweep() walks that
// window -- meshes 3e-7 to 3.5e6 across, eps from 1e-17 to 1e-2, |d| from 1e-4 to 1e4, a far small mesh, slivers eps
// wide, the integer grid, a max_dist that cuts hits off -- through every tree, the megakernel and the tile pass.
// ---------------------------------------------------------------------------------------------
// n / d for a launch-constant divisor: m = floor(2^32 / d) (host, div_magic_of) under-estimates the quotient by
// at most 2, fixed by two conditional steps; ~8 instructions instead of the ~40 of a 32-bit division.
__device__ __forceinline__ uint32_t div_magic(uint32_t n, uint32_t d, uint32_t m) {
    uint32_t q = __umulhi(n, m);
    uint32_t r = n - q * d;
    if (r >= d) ++q, r -= d;
    if (r >= d) ++q;
    return q;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define RBRT_AS1(T, p) ((const __attribute__((address_space(1))) T*)(p))

struct RayCull {
    V3 inv, nod;  // 1/d and -(o/d)
    // Byte offsets inside a BvhNode4 of the planes the ray ENTERS through, per axis (lo_* where 1/d is
    // positive, hi_* otherwise); the exit planes are at offset ^ {48, 80, 112}.
    uint32_t near_x, near_y, near_z;
    float pad_base, pad_k;
};

__device__ __forceinline__ RayCull make_cull(V3 o, V3 d, const float* center, float radius, float eps_frac) {
    RayCull rc;
    const V3 oc = o - mk(center);
    const float S = __builtin_amdgcn_sqrtf(dot(oc, oc)) + radius;
    const float omax =
        __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
    rc.pad_base = (64.0f / 16777216.0f) * (S + omax);
    rc.pad_k = rc.pad_base * (__builtin_amdgcn_sqrtf(dot(d, d)) * eps_frac);
    rc.inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    rc.nod = mk(-(o.x * rc.inv.x), -(o.y * rc.inv.y), -(o.z * rc.inv.z));
    rc.near_x = (__float_as_uint(rc.inv.x) >> 31) ? 48u : 0u;
    rc.near_y = (__float_as_uint(rc.inv.y) >> 31) ? 64u : 16u;
    rc.near_z = (__float_as_uint(rc.inv.z) >> 31) ? 80u : 32u;
    return rc;
}

constexpr uint32_t kMissKey = 0xFFFFFFFFu;

// One child box of a 4-wide node, given its entry planes (nx, ny, nz) and exit planes (fx, fy, fz) for
// this ray's direction signs. Growing the box by the pad moves entry planes against the ray and exit planes
// with it; in the ray-parameter domain that is a constant per axis, folded into the FMA's addend by the
// caller (nodn = nod - pad|1/d|, nodf = nod + pad|1/d|), so one FMA per plane gives the padded plane's
// parameter. Returns the sort key of the child: kMissKey when the ray misses it, else its entry distance
// (two low mantissa bits replaced by the child slot).
// The three conditions of a hit -- tn <= tf, tf >= eps, tn <= best_t -- are ONE compare: with best_t >= eps (every
// search bound is: triangle.rs:398's 1e6, a sphere's distance relaxed upwards, an accepted t > eps) they are
// equivalent to max(tn, eps) <= min(tf, best_t). fmax / fmin ignore a NaN operand, so a NaN plane parameter (a
// zero direction component) can only make the test MORE permissive, which culling tolerates; an UNUSED slot has the
// empty box (lo = +inf, hi = -inf: its entry parameter is +inf or NaN on every axis, its exit parameter -inf or
// NaN) and misses unless all six are NaN, i.e. unless the ray itself is degenerate -- those rays never get here
// (ray_is_traversable below).
template <bool SLOT_BITS = true>
__device__ __forceinline__ uint32_t child_key(float nx, float ny, float nz, float fx, float fy, float fz, V3 inv, V3 nodn,
                                              V3 nodf, float eps, float best_t, uint32_t slot) {
    const float tnx = __builtin_fmaf(nx, inv.x, nodn.x);
    const float tny = __builtin_fmaf(ny, inv.y, nodn.y);
    const float tnz = __builtin_fmaf(nz, inv.z, nodn.z);
    const float tfx = __builtin_fmaf(fx, inv.x, nodf.x);
    const float tfy = __builtin_fmaf(fy, inv.y, nodf.y);
    const float tfz = __builtin_fmaf(fz, inv.z, nodf.z);
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz), eps);
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), best_t);
    // (tn >= eps > 0: the integer order of its bits is its order; a caller that sorts the links along with the keys has no
    // use for the slot number in the low bits)
    return tn <= tf ? (SLOT_BITS ? ((__float_as_uint(tn) & ~3u) | slot) : __float_as_uint(tn)) : kMissKey;
}
// A ray the slab arithmetic above can be trusted with: finite origin, finite non-zero direction. Anything else gets
// no mesh hit at all, which is what the reference's ordered compares give it (triangle.rs:190-241: every NaN compare
// is false) -- callers start such a ray's search at a bound below eps, so that every node test fails.
__device__ __forceinline__ bool ray_is_traversable(V3 o, V3 d) {
    const float dd = dot(d, d), oo = dot(o, o);
    return dd > 0.0f && dd < __builtin_inff() && oo < __builtin_inff();  // (false for NaN)
}

__device__ __forceinline__ void cswap(uint32_t& a, uint32_t& b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Fetch one 128-B node (8 x dwordx4 by this lane) and test its four children; k[] comes back sorted by
// entry distance (misses last) -- or, with SORTED = false, in slot order --, links = the four child links.
template <bool SORTED = true, bool SLOT_BITS = true>
__device__ __forceinline__ void node4_visit(const BvhNode4* node, const RayCull& rc, float eps, float best_t,
                                            uint32_t k[4], f32x4& links) {
    const char* nb = reinterpret_cast<const char*>(node);
    f32x4 nx, ny, nz, fx, fy, fz, me;
    nx = *RBRT_AS1(f32x4, nb + rc.near_x), ny = *RBRT_AS1(f32x4, nb + rc.near_y), nz = *RBRT_AS1(f32x4, nb + rc.near_z);
    fx = *RBRT_AS1(f32x4, nb + (rc.near_x ^ 48u)), fy = *RBRT_AS1(f32x4, nb + (rc.near_y ^ 80u));
    fz = *RBRT_AS1(f32x4, nb + (rc.near_z ^ 112u));
    me = *RBRT_AS1(f32x4, nb + 112);
    links = *RBRT_AS1(f32x4, nb + 96);
    // one pad for the node: the largest of its children's error terms (siblings have similar triangles)
    // (the error terms are products of lengths, >= +0: the order of their bits as integers is their order, and an integer
    // max3 needs no canonicalising v_max x, x, x in front of it, which fmaxf of a loaded value gets. A NaN -- a mesh with
    // non-finite vertices -- comes out as the maximum and makes every test of the node pass.)
    const uint32_t me_max = max(max(__float_as_uint(me.x), __float_as_uint(me.y)), max(__float_as_uint(me.z), __float_as_uint(me.w)));
    const float pad = __builtin_fmaf(rc.pad_k, __uint_as_float(me_max), rc.pad_base);
    // the pad in ray-parameter units, per axis (|1/d| may be inf: the plane parameters are then +-inf or NaN,
    // which only makes the test more permissive)
    const V3 pt = mk(pad * __builtin_fabsf(rc.inv.x), pad * __builtin_fabsf(rc.inv.y), pad * __builtin_fabsf(rc.inv.z));
    const V3 nodn = rc.nod - pt, nodf = rc.nod + pt;
    k[0] = child_key<SLOT_BITS>(nx.x, ny.x, nz.x, fx.x, fy.x, fz.x, rc.inv, nodn, nodf, eps, best_t, 0u);
    k[1] = child_key<SLOT_BITS>(nx.y, ny.y, nz.y, fx.y, fy.y, fz.y, rc.inv, nodn, nodf, eps, best_t, 1u);
    k[2] = child_key<SLOT_BITS>(nx.z, ny.z, nz.z, fx.z, fy.z, fz.z, rc.inv, nodn, nodf, eps, best_t, 2u);
    k[3] = child_key<SLOT_BITS>(nx.w, ny.w, nz.w, fx.w, fy.w, fz.w, rc.inv, nodn, nodf, eps, best_t, 3u);
    if (SORTED) {
        cswap(k[0], k[1]);
        cswap(k[2], k[3]);
        cswap(k[0], k[2]);
        cswap(k[1], k[3]);
        cswap(k[1], k[2]);
    }
}
// The same visit with the child LINKS sorted along with the keys (round 4). Sorting the keys alone costs two
// instructions per compare-exchange (v_min_u32 + v_max_u32), but every link then has to be picked out of four registers
// by the slot number in its key's low bits: and + 3 x (v_cmp, v_cndmask) = 7 VALU instructions and, with the compares
// writing VCC right ahead of the selects that read it, three s_nop each -- 28 + 12 per visit for the four links. A
// compare-exchange that carries the link along is one compare and four selects: 25 for the five exchanges, against
// 10 + 28, and five VCC hazards instead of twelve. Which child is walked first cannot change what is found (the tree only
// culls; the result cell keeps the lexicographic (t, index) minimum), so equal keys may come out in either order.
__device__ __forceinline__ void cswap_pair(uint32_t& ka, uint32_t& kb, int32_t& la, int32_t& lb) {
    const bool sw = kb < ka;
    const uint32_t k0 = sw ? kb : ka, k1 = sw ? ka : kb;
    const int32_t l0 = sw ? lb : la, l1 = sw ? la : lb;
    ka = k0, kb = k1, la = l0, lb = l1;
}
__device__ __forceinline__ void node4_visit_sorted(const BvhNode4* node, const RayCull& rc, float eps, float best_t,
                                                   uint32_t k[4], int32_t l[4]) {
    f32x4 links;
    node4_visit<false, false>(node, rc, eps, best_t, k, links);
    l[0] = __float_as_int(links.x), l[1] = __float_as_int(links.y), l[2] = __float_as_int(links.z), l[3] = __float_as_int(links.w);
    cswap_pair(k[0], k[1], l[0], l[1]);
    cswap_pair(k[2], k[3], l[2], l[3]);
    cswap_pair(k[0], k[2], l[0], l[2]);
    cswap_pair(k[1], k[3], l[1], l[3]);
    cswap_pair(k[1], k[2], l[1], l[2]);
}
__device__ __forceinline__ int32_t link_of(const f32x4& links, uint32_t key) {
    const uint32_t s = key & 3u;
    const float v = s == 0u ? links.x : (s == 1u ? links.y : (s == 2u ? links.z : links.w));
    return __float_as_int(v);
}

// All triangles of one leaf (<= kLeafMax), triangle.rs:189-255 + the arg-min rule of triangle.rs:400 (the simple
// one-thread-per-ray path; the megakernel deals the triangles of pending leaves out to all lanes instead).
template <bool STATS>
__device__ __forceinline__ void leaf_test(const BvhTri* tris, int32_t leaf_ref, V3 o, V3 d, float eps, float eps_frac,
                                          float& best_t, uint32_t& best_idx, LocalCounters& lc) {
    const uint32_t leaf = uint32_t(~leaf_ref);
    const uint32_t first = leaf >> kLeafBits, last = leaf & uint32_t(kLeafMax - 1);  // last = count - 1
    for (uint32_t i = 0; i <= last; ++i) {
        const auto* tp = RBRT_AS1(f32x4, tris + first + i);
        const f32x4 a = tp[0], b = tp[1];
        const f32x2 c = *RBRT_AS1(f32x2, tp + 2);  // the record's last 8 bytes are padding: not fetched
        if (STATS) ++lc.tris;
        float t;
        const bool hit = tri_test(mk(a.x, a.y, a.z), mk(a.w, b.x, b.y), mk(b.z, b.w, c.x), o, d, eps, eps_frac, t);
        const uint32_t idx = __float_as_uint(c.y);
        // strict < keeps the first (lowest) index among equal t
        if (hit && (t < best_t || (t == best_t && idx < best_idx))) {
            best_t = t;
            best_idx = idx;
        }
    }
}

// Closest accepted triangle of one mesh = triangle.rs:134-262 + 392-410, found through the BVH
// (simple one-thread-per-ray form with the whole stack in LDS; the megakernel has its own loop).
// Result contract (what the brute-force scan returns): the smallest accepted t below the scan's
// initial 1e6; among equal t the lowest reference index. best_t stays 1e6 when nothing is hit.
template <bool STATS>
__device__ __forceinline__ void mesh_closest(const DevMesh& M, V3 o, V3 d, float eps, float eps_frac,
                                             uint32_t* __restrict__ stack, uint32_t stride, float& best_t_out,
                                             uint32_t& best_idx_out, LocalCounters& lc) {
    const RayCull rc = make_cull(o, d, M.center, M.radius, eps_frac);
    float best_t = 1000000.0f;  // triangle.rs:398
    uint32_t best_idx = 0;
    int sp = 0;
    int32_t cur = ray_is_traversable(o, d) ? 0 : kNoChild;  // root
    while (cur != kNoChild) {
        bool pop = true;
        if (cur >= 0) {
            uint32_t k[4];
            f32x4 links;
            node4_visit(M.nodes + cur, rc, eps, best_t, k, links);
            if (STATS) ++lc.nodes;
            if (k[0] != kMissKey) {
                if (k[3] != kMissKey) stack[(sp++) * stride] = uint32_t(link_of(links, k[3]));
                if (k[2] != kMissKey) stack[(sp++) * stride] = uint32_t(link_of(links, k[2]));
                if (k[1] != kMissKey) stack[(sp++) * stride] = uint32_t(link_of(links, k[1]));
                cur = link_of(links, k[0]);
                pop = false;
            }
        } else {
            leaf_test<STATS>(M.tris, cur, o, d, eps, eps_frac, best_t, best_idx, lc);
        }
        if (pop) {
            if (sp == 0) break;
            cur = int32_t(stack[(--sp) * stride]);
        }
    }
    best_t_out = best_t;
    best_idx_out = best_idx;
}

struct HitRec {
    float dist;   // dist_from_ray_orig of the winner (lib.rs:35)
    float t;      // its ray parameter
    int32_t obj;  // -1 miss, [0, n_elem) an element of Scene::elements (sphere or BasicTriangle), n_elem + m mesh
    uint32_t tri;
};

// scene.rs:19-43: spheres in order, then meshes in order, strictly smaller distance wins.
// motion: null, or the spheres' travels [n_spheres][3] with the path's draw mt (sphere_centre_at, below).
// mesh_motion (MM builds only): the meshes' travels [n_meshes][3]; mesh m is tested with the origin mesh_origin_at(o, w_m, mt)
// in everything mesh.rs does with the ray, and its dist competes with the world-space distances of the others.
__device__ __forceinline__ V3 sphere_centre_at(const float* centre, const float* travel, float t);
__device__ __forceinline__ V3 mesh_origin_at(V3 o, const float* travel, float s);
template <bool STATS, bool MM = false>
__device__ __forceinline__ void scene_hit(const TraceParams& P, V3 o_world, V3 d, uint32_t* stack, uint32_t stride,
                                          HitRec& h, LocalCounters& lc, const float* motion = nullptr, float mt = 0.0f,
                                          const float* mesh_motion = nullptr) {
    const V3 o = o_world;
    float closest = 3.40282347e+38f;  // f32::MAX
    h.obj = -1;
    h.t = 0.0f;
    h.tri = 0;
    if (STATS) ++lc.rays;
    const uint32_t n_elem = P.n_spheres + P.n_elem_tris;
    for (uint32_t e = 0; e < n_elem; ++e) {  // Scene::elements in their order (scene.rs:23-31)
        const uint32_t desc = P.elems != nullptr ? P.elems[e] : e;
        float t, dist;
        bool hit;
        if (desc >> 31) {
            hit = basic_triangle_hit(P.elem_tris[desc & 0x7FFFFFFFu].v0, o, d, P.min_dist, P.max_dist, t, dist);
        } else {
            const DevSphere sp = P.spheres[desc];
            const V3 c = motion ? sphere_centre_at(sp.center, motion + desc * 3u, mt) : mk(sp.center);
            hit = sphere_hit(c, sp.radius, o, d, P.min_dist, P.max_dist, t, dist, P.counters);
        }
        if (hit && dist < closest) {
            closest = dist;
            h.t = t;
            h.obj = int32_t(e);
        }
    }
    for (uint32_t m = 0; m < P.n_meshes; ++m) {
        const DevMesh& M = P.meshes[m];
        const V3 o = MM ? mesh_origin_at(o_world, mesh_motion + m * 3u, mt) : o_world;  // (shadows the world origin: "Moving meshes")
        if (!bbox_gate(M.bbox_lo, M.bbox_hi, o, d)) continue;  // mesh.rs:233-235
        if (STATS) ++lc.gate;
        float t;
        uint32_t idx;
        mesh_closest<STATS>(M, o, d, P.min_dist, P.eps_frac, stack, stride, t, idx, lc);
        if (t > P.min_dist && t < 100000.0f) {  // triangle.rs:405
            V3 p = o + t * d;                    // mesh.rs:247-249
            float dist = length(o - p);
            if (dist > P.min_dist && dist < P.max_dist) {
                if (STATS) ++lc.mesh_hits;
                if (dist < closest) {
                    closest = dist;
                    h.t = t;
                    h.obj = int32_t(n_elem + m);
                    h.tri = idx;
                }
            }
        }
    }
    h.dist = closest;
}

// ---------------------------------------------------------------------------------------------
// Shading normal of a mesh hit (rbrt_hip.h rbrt_scene_shading_t): the stored face normal of entry `tri`, or, on a smooth
// mesh, the corner normals interpolated with the barycentrics of the Moller-Trumbore test that made it the closest hit
// (tri_test's u and v, operation for operation). Called by the megakernel's scatter pass and the debug hook alike.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ V3 smooth_normal(const SmoothRec* rec, V3 o, V3 d, V3 face) {
    const V3 v0 = mk(rec->v0), e1 = mk(rec->e1), e2 = mk(rec->e2);
    const V3 h = cross(d, e2);
    const float f = 1.0f / dot(e1, h);
    const V3 s = o - v0;
    const float u = f * dot(s, h);
    const V3 q = cross(s, e1);
    const float v = f * dot(d, q);
    const float w = (1.0f - u) - v;
    const V3 m = (w * mk(rec->n0) + u * mk(rec->n1)) + v * mk(rec->n2);
    const V3 n = normalize(m);  // (a zero m gives 0 / 0: not finite)
    const bool ok = __builtin_isfinite(n.x) && __builtin_isfinite(n.y) && __builtin_isfinite(n.z);
    return ok ? n : face;
}
__device__ __forceinline__ V3 mesh_shading_normal(const Normal4* normals, uint32_t tri, V3 o, V3 d) {
    const Normal4 nn = normals[tri];
    const V3 face = mk(nn.x, nn.y, nn.z);  // mesh.rs:253-257
    const uint32_t n_total = __float_as_uint(nn.w);
    if (n_total == 0u) return face;
    return smooth_normal(reinterpret_cast<const SmoothRec*>(normals + n_total) + tri, o, d, face);
}

// ---------------------------------------------------------------------------------------------
// Solid patterns (rbrt_hip.h rbrt_scene_patterns_t; device_types.h DevPattern)
// ---------------------------------------------------------------------------------------------
// Which entry of the material table a hit of object `obj` at p records: the object's own, or -- a patterned lambertian
// whose hit lies in an odd cell -- its second entry. `mat`: the table as dwords (in LDS or where the host put it); `link`:
// the object's pattern link (DevMaterial::param of a lambertian: 0 = no pattern, the one compare an unpatterned hit pays).
__device__ __forceinline__ int32_t checker_cell(float t) {
    const float u = __builtin_fminf(__builtin_fmaxf(t, -1e9f), 1e9f);  // (a NaN counts as -1e9)
    return int32_t(__builtin_floorf(u));
}
__device__ __forceinline__ uint32_t surface_entry(const uint32_t* mat, uint32_t obj, uint32_t link, V3 p) {
    if (link == 0u) return obj;
    const float* r = reinterpret_cast<const float*>(mat + (link >> kPatternLinkShift));  // DevPattern: origin, inv
    const float inv = r[3];
    const int32_t kx = checker_cell((p.x - r[0]) * inv), ky = checker_cell((p.y - r[1]) * inv), kz = checker_cell((p.z - r[2]) * inv);
    return ((kx ^ ky ^ kz) & 1) ? (link & 255u) : obj;
}
// The link of any object: only a lambertian's param word is one (a metal's is its roughness, a dielectric's its index).
__device__ __forceinline__ uint32_t surface_link(const uint32_t* mat, uint32_t obj) {
    return int32_t(mat[obj * 5u + 4u]) == RBRT_MAT_LAMBERTIAN ? mat[obj * 5u + 3u] : 0u;
}

// ---------------------------------------------------------------------------------------------
// Materials
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ V3 random_point_in_unit_sphere(Rng& rng) {  // materials.rs:14-30
    // The reference loops `while point.length() > 1.0`. With a correctly rounded sqrt,
    // sqrt(s) > 1.0f holds exactly when s > 0x1.000002p0f (the float after 1.0): sqrt(1 + 2^-23)
    // still rounds to 1.0, sqrt(1 + 2^-22) rounds to 1 + 2^-23. So the loop can compare the squared
    // length and skip an IEEE square root per iteration with bit-identical accept/reject decisions
    // (checked exhaustively around 1.0 in tests/test_oracle_kats.py).
    // A component is 2.0f * next_f32() - 1.0f with next_f32() = float(k) * 2^-24, k < 2^24: float(k), both products and the
    // difference (k - 2^23) * 2^-23 are all exact, so one fused multiply-add of float(k), exact as well, is the same float
    // for every k (tests/test_unit_sphere_point.py runs all 2^24) and two VALU instructions fewer per component.
    const auto component = [&]() { return __builtin_fmaf(float(rng.next_u32() >> 8), 0x1p-23f, -1.0f); };
    V3 p;
    float s;
    do {
        const float x = component();
        const float y = component();
        const float z = component();
        p = mk(x, y, z);
        s = (p.x * p.x + p.y * p.y) + p.z * p.z;
    } while (s > 1.00000011920928955078125f);
    return p;
}

__device__ __forceinline__ V3 reflect(V3 dir, V3 n) {  // materials.rs:32-37
    V3 du = normalize(dir);
    V3 nu = normalize(n);
    V3 r = du - 2.0f * nu * dot(du, nu);
    return normalize(r);
}

__device__ __forceinline__ float schlick(float cosine, float ref_index) {  // dielectric.rs:63-66
    float q = (1.0f - ref_index) / (1.0f + ref_index);
    float r0 = q * q;
    float x = 1.0f - cosine;
    float x2 = x * x;
    float x4 = x2 * x2;
    return r0 + (1.0f - r0) * (x * x4);  // powi(5) = x * (x^2)^2
}

// dielectric.rs:72-85: refract on unit vectors, v = normalize(dir), nu = normalize(n)
__device__ __forceinline__ bool refract_unit(V3 v, V3 nu, float ni_over_nt, V3& out) {
    float c = dot(v, nu);
    float discr = 1.0f - (ni_over_nt * ni_over_nt) * (1.0f - c * c);
    if (discr > 0.0f) {
        out = ni_over_nt * (v - nu * c) - __builtin_sqrtf(discr) * nu;
        return true;
    }
    return false;
}
__device__ __forceinline__ bool refract(V3 dir, V3 n, float ni_over_nt, V3& out) {  // dielectric.rs:68-85
    return refract_unit(normalize(dir), normalize(n), ni_over_nt, out);
}

// dielectric.rs:11-59. The reference normalises the incoming direction three times (in reflect, for the cosine, in refract)
// and the normal or its negation three times. Here du and nu are computed once when every active lane's operands pass
// normalize's gate, so that both came from its short path: there normalize(-1.0f * n) is -normalize(n) bit for bit, because
// every step (the squares, the square root and the reciprocal of an unchanged length, the products and fused residuals
// with a negated numerator) is odd-symmetric under round-to-nearest, and no component is 0 or NaN. A wave with a lane
// outside the gate (a zero, subnormal, huge or NaN operand) runs the reference's sequence as written.
__device__ __forceinline__ void scatter_dielectric(float ref_index, V3 in_d, V3 n, Rng& rng, V3& out_d) {
    bool short_d, short_n;
    const V3 du = normalize(in_d, short_d);
    const V3 nu = normalize(n, short_n);
    V3 reflected, refracted = mk(0.0f, 0.0f, 0.0f);
    float reflect_prob;
    if (short_d && short_n) {
        const float a = dot(du, nu);
        const bool leaving = a > 0.0f;
        const V3 outward = leaving ? mk(-nu.x, -nu.y, -nu.z) : nu;
        const float ni_over_nt = leaving ? ref_index : 1.0f / ref_index;
        const float cosine = leaving ? ref_index * a : -a;
        reflect_prob = refract_unit(du, outward, ni_over_nt, refracted) ? schlick(cosine, ref_index) : 1.0f;
        reflected = normalize(du - 2.0f * nu * a);  // reflect(in_d, n), last: du and nu end here
    } else {
        reflected = reflect(in_d, n);
        V3 outward;
        float ni_over_nt, cosine;
        float a = dot(normalize(in_d), normalize(n));
        if (a > 0.0f) {
            outward = -1.0f * n;
            ni_over_nt = ref_index;
            cosine = ref_index * a;
        } else {
            outward = n;
            ni_over_nt = 1.0f / ref_index;
            cosine = -a;
        }
        reflect_prob = refract(in_d, outward, ni_over_nt, refracted) ? schlick(cosine, ref_index) : 1.0f;
    }
    out_d = (rng.next_f32() < reflect_prob) ? reflected : refracted;
}

// RayScattering::scatter for the three materials that scatter (not for an emitter: callers never pass one). Returns the
// reference's bool; `records` says whether the attenuation is anything other than the exact identity (1,1,1).
__device__ __forceinline__ bool scatter(const DevMaterial& m, V3 in_d, V3 p, V3 n, Rng& rng, V3& out_d) {
    if (m.kind == RBRT_MAT_LAMBERTIAN) {  // lambertian.rs:11-24
        V3 target = (p + normalize(n)) + random_point_in_unit_sphere(rng);
        out_d = normalize(target - p);
        return true;
    } else if (m.kind == RBRT_MAT_METAL) {  // metal.rs:12-25
        V3 target = reflect(in_d, n);
        out_d = normalize(target + m.param * random_point_in_unit_sphere(rng));
        return dot(out_d, n) > 0.0f;
    } else {  // dielectric.rs:11-59
        scatter_dielectric(m.param, in_d, n, rng, out_d);
        return true;
    }
}

// cam.rs:64-82: the point of the image plane the camera ray of sample (pixel, stream state) passes through; the column
// jitter is drawn first.
__device__ __forceinline__ V3 camera_target(V3 center, V3 right, V3 up, float mm_hor, float mm_vert, uint32_t img_w, uint32_t img_h,
                                            uint32_t row, uint32_t col, Rng& rng) {
    const float col_off = float(col) - float(img_w / 2);
    const float row_off = float(row) - float(img_h / 2);
    const float u0 = rng.next_f32();
    const float col_mm = ((col_off + u0) - 0.5f) * mm_hor;
    const float u1 = rng.next_f32();
    const float row_mm = ((row_off + u1) - 0.5f) * mm_vert;
    return (center + (0.001f * col_mm) * right) - (0.001f * row_mm) * up;
}
// ... and the direction of the (pinhole) camera ray through it.
__device__ __forceinline__ V3 camera_ray_direction(V3 pos, V3 center, V3 right, V3 up, float mm_hor, float mm_vert, uint32_t img_w,
                                                   uint32_t img_h, uint32_t row, uint32_t col, Rng& rng) {
    return normalize(camera_target(center, right, up, mm_hor, mm_vert, img_w, img_h, row, col, rng) - pos);
}
// RBRT_FLAG_THIN_LENS (rbrt_hip.h rbrt_camera_lens_t): after the jitter draws that placed `target`, a
// point of the unit disc by rejection from [-1, 1)^2 (no sin / cos: a restatement reproduces it bit for bit), the origin
// on the lens and the direction to the focus surface's image of the target. `lens`: lens_u, lens_v, focus_scale.
// In: o = position, f = the target; out: o = the origin on the lens, f = the focus point F (the ray's direction is then
// normalize(f - o), as the pinhole's is normalize(target - position)).
__device__ __forceinline__ void lens_point(V3& o, V3& f, const float* lens, Rng& rng) {
    // (a wave-uniform loop: a lane whose point is accepted keeps it and its stream, by selects, while the others draw on)
    float lx = 0.0f, ly = 0.0f;
    bool pending = true;
    do {
        Rng t = rng;
        const float x = 2.0f * t.next_f32() - 1.0f;
        const float y = 2.0f * t.next_f32() - 1.0f;
        if (pending) rng = t, lx = x, ly = y;
        pending = pending && !(x * x + y * y < 1.0f);
    } while (__builtin_amdgcn_ballot_w64(pending) != 0ull);
    const V3 pos = o;
    o = pos + (lx * mk(lens) + ly * mk(lens + 3));
    f = pos + lens[6] * (f - pos);
}
constexpr uint32_t kLensDw = 8;  // lens words staged in the megakernel's LDS for a lens launch: lens_u, lens_v, focus_scale, pad
// The shutter (rbrt_hip.h "Camera shutter"): after the ray (o, d) of a sample has been made -- jitter,
// lens and normalize(f - o) included -- the next draw of its stream places the whole camera on its way from the opening to
// the closing position: o += t * travel, unfused, a product and a sum per component. d is NOT recomputed: a translation
// does not turn a ray. The bounce draws follow. A ray that hits nothing depends on d only, so the sky resolves never call this.
__device__ __forceinline__ void shutter_origin(V3& o, const float* travel, float t) { o = o + t * mk(travel); }
__device__ __forceinline__ void shutter_origin(V3& o, const float* travel, Rng& rng) { shutter_origin(o, travel, rng.next_f32()); }
constexpr uint32_t kShutterDw = 4;  // words staged in the megakernel's LDS for a shutter launch: travel, pad
// Moving spheres (rbrt_hip.h "Moving spheres"): the same draw t -- ONE draw for the shutter and the motion,
// camera and objects share an exposure -- belongs to the sample for its whole path, and wherever a path reads a sphere's
// centre it reads c(t) = c + (t * travel_i), unfused, a product and a sum per component: the hit test of every ray of the
// path and the normal p - c(t). The radius, the materials and everything that is not a sphere stay where they are.
__device__ __forceinline__ V3 sphere_centre_at(const float* centre, const float* travel, float t) { return mk(centre) + t * mk(travel); }
constexpr uint32_t kMotionDw = 3;  // words per sphere staged in the megakernel's LDS for a motion launch: its travel
// Moving meshes (rbrt_hip.h "Moving meshes"): a ray (o, d) meets a mesh displaced by v where the ray
// (o - v, d) meets the mesh at rest, so wherever a path tests mesh m it reads the origin o_m = o - (s * w_m), s = phase + t the
// sample's time: unfused, a product and a difference per component. The trees, the triangles and the normals stay untouched.
__device__ __forceinline__ V3 mesh_origin_at(V3 o, const float* travel, float s) { return o - s * mk(travel); }
constexpr uint32_t kMeshMotionDw = 3;  // words per mesh staged behind the spheres' travels and the phase in a launch with a mesh motion

// lib.rs:68-71: what a ray that hits nothing sees; the direction as it is (not re-normalised).
// `constant` (RBRT_FLAG_CONSTANT_BACKGROUND): bg itself.
__device__ __forceinline__ V3 background(float dy, const float* bg, uint32_t constant) {
    if (constant) return mk(bg);
    const float t = 0.5f * (dy + 1.0f);
    return t * mk(1.0f, 1.0f, 1.0f) + (1.0f - t) * mk(bg);
}

// The environment (rbrt_hip.h "Environment lighting"): what a ray that hits nothing sees while the handle has a
// map. `nodes`: (n + 1) x (n + 1) texels of 16 bytes, row j first; `d`: the direction as traced, not re-normalised. The
// octahedral fold and the bilinear weights use + - * /, abs, floor and comparisons only, unfused, in the written order: a
// numpy restatement gives the same bits. The cell index is clamped to [0, n - 1] whatever d is (a NaN compares false:
// index 0), so the four loads stay inside the map; a NaN or zero direction gives a NaN colour.
__device__ __forceinline__ V3 environment_radiance(const EnvTexel* __restrict__ nodes, uint32_t n, V3 d) {
    const float s = (__builtin_fabsf(d.x) + __builtin_fabsf(d.y)) + __builtin_fabsf(d.z);
    const float px = d.x / s, py = d.y / s, pz = d.z / s;
    float u = px, v = pz;
    if (!(py >= 0.0f)) {  // the lower hemisphere: folded over the diagonals
        u = (1.0f - __builtin_fabsf(pz)) * (px >= 0.0f ? 1.0f : -1.0f);
        v = (1.0f - __builtin_fabsf(px)) * (pz >= 0.0f ? 1.0f : -1.0f);
    }
    const float fn = float(n);
    const float x = ((u * 0.5f) + 0.5f) * fn, y = ((v * 0.5f) + 0.5f) * fn;
    const uint32_t i = x >= 0.0f ? (x < fn ? uint32_t(__builtin_floorf(x)) : n - 1u) : 0u;
    const uint32_t j = y >= 0.0f ? (y < fn ? uint32_t(__builtin_floorf(y)) : n - 1u) : 0u;
    const float fx = x - float(i), fy = y - float(j);
    const EnvTexel* row = nodes + size_t(j) * (n + 1u) + i;
    const EnvTexel e00 = row[0], e01 = row[1], e10 = row[n + 1u], e11 = row[n + 2u];
    const V3 a = mk(e00.r, e00.g, e00.b), b = mk(e01.r, e01.g, e01.b), c = mk(e10.r, e10.g, e10.b), e = mk(e11.r, e11.g, e11.b);
    const V3 top = a + fx * (b - a);
    const V3 bot = c + fx * (e - c);
    return top + fy * (bot - top);
}
// ... out of line, for the counting build of the trace kernel (it spills already; inlined, the lookup adds to that)
__device__ __noinline__ V3 environment_radiance_call(const EnvTexel* nodes, uint32_t n, V3 d) { return environment_radiance(nodes, n, d); }
constexpr uint32_t kEnvDw = 4;  // words staged in the megakernel's LDS for a launch with a map: the address (2), n, pad

__host__ __device__ inline uint32_t megakernel_lds_dwords(uint32_t stack_entries, uint32_t n_spheres, uint32_t n_meshes, uint32_t n_elem_tris,
                                                          uint32_t thin_lens, uint32_t environment, uint32_t pattern_dw, uint32_t shutter,
                                                          uint32_t motion, uint32_t mesh_motion);
#include "megakernel.inl"

// lib.rs:116-122: (sqrt(c) * 256) as u8 — Rust's float->int cast saturates and maps NaN to 0.
__device__ __forceinline__ uint8_t quantise(float c) {
    float v = __builtin_sqrtf(c) * 256.0f;
    if (!(v == v)) return 0;
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return uint8_t(v);
}

// The end of a pixel's batch: the running sum goes back to `acc`, or -- on the last batch -- the mean (lib.rs:101) and
// the optional quantisation go out. `j`: the pixel's place in the rank's packed tiles.
__device__ __forceinline__ void resolve_store(const ResolveParams& R, size_t j, uint32_t row, uint32_t col, bool valid, float ax, float ay,
                                              float az) {
    const bool packed = R.tile_world > 1;
    if (valid) {
        if (!R.last_batch) {
            R.acc[j * 3 + 0] = ax;
            R.acc[j * 3 + 1] = ay;
            R.acc[j * 3 + 2] = az;
            return;
        }
        ax = ax * R.inv_spp;
        ay = ay * R.inv_spp;
        az = az * R.inv_spp;
    } else if (!R.last_batch || !packed) {
        return;  // (a pixel slot beyond a ragged image edge: packed outputs carry it as zeros)
    }
    const size_t o = packed ? j * 3u : (size_t(row) * R.width + col) * 3u;
    if (R.out_radiance) {
        R.out_radiance[o + 0] = ax;
        R.out_radiance[o + 1] = ay;
        R.out_radiance[o + 2] = az;
    }
    if (R.out_rgb8) {
        R.out_rgb8[o + 0] = quantise(ax);
        R.out_rgb8[o + 1] = quantise(ay);
        R.out_rgb8[o + 2] = quantise(az);
    }
}

// Sequential per-pixel sum over the samples of this batch (lib.rs:95-100 adds them in sample
// order; keeping that order keeps the mean bit-identical), then on the last batch the multiply by
// 1/spp (lib.rs:101) and the optional quantisation.
__global__ __launch_bounds__(kSmallBlock) void resolve_kernel(const ResolveParams R) {
    // (with a tile pass the launch rendered the tiles of the work list only; the grid covers all of the rank's)
    const size_t npix = size_t(R.tile_lists ? R.tile_lists[0] : R.n_local_tiles) * 64u;
    const size_t i = size_t(blockIdx.x) * kSmallBlock + threadIdx.x;
    // the trace launch this resolves has ended: its work counters are reset for the lane's next launch (which
    // waits for this kernel), saving a memset launch that would have to queue behind the resident megakernels
    // Helper launches (api.cpp "Elastic launches") may have joined the launch: a helper wave that took work registered in
    // helper_words[0] before it drew from the counters, and leaves the count only when its samples are written. The launch
    // itself has ended (stream order), so nobody can TAKE work any more; what is waited for here is the waves that hold
    // some. Almost always the count is zero already. Bounded: a count that never returns raises the error flag instead of
    // hanging the GPU (rbrt_hip_scene_check reports it).
    if (R.helper_words) {
        // (the common case is a count of zero, read with a plain atomic load: an acquire here would invalidate the CU's L1
        // under the resident trace waves, once per workgroup of this kernel -- 12,288 times per 1024x768 frame: +3-5 % per
        // frame, measured. A count of zero means every helper wave that held work has written its samples back and left;
        // this kernel's caches were invalidated when it started and none of its waves reads a sample before this point.)
        if (threadIdx.x == 0 && __hip_atomic_load(R.helper_words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
            uint32_t spins = 0;
            while (__hip_atomic_load(R.helper_words, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                __builtin_amdgcn_s_sleep(16);
                if (++spins > (1u << 23)) {
                    atomicAdd(R.error_flag, 1ull);
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        // (first the launch's number -- from here on a helper wave of it draws nothing more --, then the counters)
        if (R.helper_words && threadIdx.x == 0) {
            __hip_atomic_store(R.helper_words + 1, R.helper_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < kWorkShards * kWorkCounterStride; w += kSmallBlock) R.work_counter[w] = 0ull;
    }
    if (i >= npix) return;
    const uint32_t p = uint32_t(i & 63u);
    const uint32_t tile_local = R.tile_lists ? R.tile_lists[kTileListHeader + (i >> 6)] : uint32_t(i >> 6);
    const size_t j = size_t(tile_local) * 64u + p;  // the pixel's place in the rank's packed tiles (acc, packed outputs)
    const uint32_t tile = tile_local * R.tile_world + R.tile_rank;
    uint32_t ty, tx;
    tile_xy(tile, R.tiles_x, ty, tx);
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    const bool valid = row < R.height && col < R.width;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (valid) {
        if (!R.first_batch) {
            ax = R.acc[j * 3 + 0];
            ay = R.acc[j * 3 + 1];
            az = R.acc[j * 3 + 2];
        }
        for (uint32_t s = 0; s < R.batch; ++s) {
            const float* sp = R.sample_buf + (size_t(s) * npix + i) * 3u;
            ax = ax + sp[0];
            ay = ay + sp[1];
            az = az + sp[2];
        }
    }
    resolve_store(R, j, row, col, valid, ax, ay, az);
}

// The pixels of the tiles that see only the background (TraceParams::tile_lists, second list): every sample of such a
// pixel is one camera ray that hits nothing (cam.rs:64-82, lib.rs:68-71), so its batch is generated, summed in sample
// order and stored right here -- the same streams, the same arithmetic, the same order as the trace kernel followed by
// resolve_kernel would produce -- and the trace kernel never sees these tiles. One thread per pixel.
__global__ __launch_bounds__(kSmallBlock) void sky_resolve_kernel(const TraceParams P, const ResolveParams R) {
    const size_t i = size_t(blockIdx.x) * kSmallBlock + threadIdx.x;
    if (i >= size_t(R.tile_lists[1]) * 64u) return;
    const uint32_t p = uint32_t(i & 63u);
    const uint32_t tile_local = R.tile_lists[kTileListHeader + R.n_local_tiles + (i >> 6)];
    const size_t j = size_t(tile_local) * 64u + p;
    const uint32_t tile = tile_local * R.tile_world + R.tile_rank;
    uint32_t ty, tx;
    tile_xy(tile, R.tiles_x, ty, tx);
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    const bool valid = row < R.height && col < R.width;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (valid) {
        if (!R.first_batch) {
            ax = R.acc[j * 3 + 0];
            ay = R.acc[j * 3 + 1];
            az = R.acc[j * 3 + 2];
        }
        const V3 pos = mk(P.cam.position), center = mk(P.cam.img_center_point), right = mk(P.cam.right), up = mk(P.cam.up);
        for (uint32_t s = 0; s < R.batch; ++s) {
            Rng rng;
            rng.init(P.seed_key, row * R.width + col, P.sample_base + s);
            V3 o = pos, f = camera_target(center, right, up, P.cam.mm_per_pix_hor, P.cam.mm_per_pix_vert, R.width, R.height, row, col, rng);
            if (P.thin_lens) {
                const float lens[7] = {P.lens_u[0], P.lens_u[1], P.lens_u[2], P.lens_v[0], P.lens_v[1], P.lens_v[2], P.focus_scale};
                lens_point(o, f, lens, rng);
            }
            const V3 d = normalize(f - o);
            const V3 c = P.env_nodes ? environment_radiance(P.env_nodes, P.env_n, d) : background(d.y, P.bg, P.constant_bg);
            ax = ax + c.x;
            ay = ay + c.y;
            az = az + c.z;
        }
        if (R.counters) {  // a counting launch: one ray, one sample, zero bounces each
            atomicAdd(&R.counters->rays, (unsigned long long)R.batch);
            atomicAdd(&R.counters->samples, (unsigned long long)R.batch);
            atomicAdd(&R.counters->diag[32], (unsigned long long)R.batch);
        }
    }
    resolve_store(R, j, row, col, valid, ax, ay, az);
}

// ---------------------------------------------------------------------------------------------
// The tile pass (DESIGN.md "The tile pass"). Every camera ray of an 8x8 tile starts at cam.position and passes through
// a small rectangle of the image plane (cam.rs:64-82), so which spheres and meshes the tile's rays can reach at all is
// known before a single ray is made. This kernel writes one word per tile (TraceParams::tile_cull); a tile whose rays
// can reach NOTHING sees the background only (lib.rs:68-71): tile_lists_kernel takes it off the trace kernel's work and
// sky_resolve_kernel finishes its pixels. A test declared out of reach is one the reference would have run and FAILED,
// so the image does not change; the proof obligation is that the rule never rules out a test that could succeed.
//
// Directions. The tile's exact ray directions are the unit vectors from the position to a (widened) rectangle of the
// image plane: a convex spherical quadrilateral, inside the cone of half-angle rho (largest angle to a corner) around
// the direction c of its middle. A sphere of radius R at distance l > R fills the cone of half-angle asin(R / l) around
// q = (centre - position) / l. So with the OUTER radius R_out (inflated, below):
//   forward rays miss it     when angle(c, q)  > asin(R_out / l) + rho,
//   backward lines miss it   when angle(-c, q) > asin(R_out / l) + rho,
//   backward lines cut DEEP  when all four corners k have angle(-corner_k, q) < asin(R_in / l) (R_in: deflated; a cap of
//                            less than a quarter turn is convex, so the corners speak for the tile; the position clearly outside).
// sphere.rs:20-66 needs the forward condition and one of the backward ones: it looks at the LINE first (discriminant),
// and with a discriminant of exactly zero it accepts a negative parameter (sphere.rs:41-49: the `sol > 0.0 &&` guard),
// so a line that grazes the sphere BEHIND the camera could be a hit; one that misses it there cannot, and one that cuts
// deep has a discriminant well above zero, takes the guarded branch and is rejected with both roots negative (b > 0 and
// 4 a c >= 8e-3 r^2 keep the larger root negative in float as well). This is what lets the sky tiles drop the ground
// sphere, which every line through the camera cuts somewhere. The box test (aabbox.rs:28-58) rejects `t_max < 0`
// first, so for a mesh the forward condition on the box's bounding sphere is enough.
//
// A second, independent rule catches long thin cases the cones cannot: with a = img_center - position, f_x(p) =
// [a + 0.001 x right, up, p - position] (triple product) vanishes on the plane of the camera lines of column
// coordinate x, and a point of the line of coordinate cm at parameter s has f_x = s 0.001 (cm - x) [a, up, right]:
// over the tile's interval [lo, hi] every point of every one of its lines has f_lo f_hi <= 0, whatever the signs. An
// object entirely inside {f_lo > 0, f_hi > 0} or {f_lo < 0, f_hi < 0} meets none of the lines at all. Same with rows.
//
// Margins. The kernel's rays are float: the target point carries an absolute error of a few ulp of |img_center| and
// |position| (target - position cancels), an angle of err / |target - position| against the exact line (taken as 16
// unit roundoffs of the magnitudes involved, twice over). The sphere test with u = 2^-24, a = d.d = 1 +- 4u: l = o - c
// carries u |l| per component, b = (2d).l at most 8u |l|, c = l.l - r r at most 6u (|l|^2 + r^2), and the discriminant
// b b - (4a) c at most 36u |l|^2 + 48u (|l|^2 + r^2) + 4u max(b^2, 4ac) <= 90u (|l|^2 + r^2) = 5.4e-6 (|l|^2 + r^2)
// against its exact value 4 (r^2 - m^2), m the distance of the line from the centre: a line is taken for a hit at most
// 0.7e-6 (|l|^2 + r^2) / r outside the sphere, and a line more than that inside has a discriminant above zero. Radii are
// inflated (deflated) by 1e-5 (|l|^2 + r^2) / r, 15x that, plus 1e-5 r + 1e-6 |l|; angles are widened by the direction
// error, the pixel interval by 1e-3 pixel plus the rounding of (col_off + u) - 0.5. The mesh boxes' slack is derived where
// it is used (16 u of the farthest corner for the box test itself; the traversal's own pad for the boxes of the tree). (A first version used 0.1 % of the
// radius: a full unit for the ground sphere, which made the band of tiles whose backward lines "might graze" it six tile
// rows high instead of two.) A degenerate camera makes the quantities NaN and
// every comparison false: nothing is culled. Non-finite or non-positive radii and non-finite boxes (a mesh without
// triangles has lo = +inf) are never culled: the reference's NaN panic (sphere.rs:33), reported through
// nan_discriminants, must still be reached. BasicTriangle elements are never culled (the YAML cannot describe them).
//
// Lens rays (RBRT_FLAG_THIN_LENS). A lens ray starts at o = position + lx lens_u + ly lens_v with lx^2 + ly^2 < 1 and
// heads for F = position + focus_scale (T - position), T the pinhole target of its sample. By Cauchy-Schwarz |o - position|
// <= sqrt(|lens_u|^2 + |lens_v|^2); with the float error of o (two roundings of the offset, one of the sum: 16 u of
// |position| + |lens_u| + |lens_v| covers them) that is `lens_a` = a. F - position is parallel to T - position and at least
// focus_scale * plane_dist long, so F - o, which differs from it by at most a, makes an angle of at most
// beta = asin(a / (focus_scale * plane_dist)) with the pinhole direction of T (the code takes tan beta, which is larger):
// every lens direction lies within beta of a pinhole direction of its tile. So a point of a lens line at parameter t, forward or backward, is within a + |t| sin beta
// of a line through the position whose direction is in the tile's cone. The rules grow by that much: sphere radii by a
// (R_out + a, R_in - a: a ray from o misses / cuts the ball as a ray from the position misses / cuts the ball moved by
// position - o), the cone rho and the deep-cut caps by beta, the slabs' reach and box_unreachable's by a + beta (l + r + a)
// resp. a + beta (far + a) (the parameter of a point of the object is at most its distance from the origin), and the
// float-error slacks that depend on the origin's distance from the object (the sphere test's, the box test's, the tree pad)
// take the distance plus a. F itself is float: on top of the error of T - position, focus_scale multiplies it and the
// product, the sum and F - o add roundings of at most |position| + 2 focus_scale |T - position|_max + a; that error over
// |F - o| >= focus_scale plane_dist - a replaces the pinhole's `angle`. With a >= focus_scale plane_dist (the lens may
// reach the focus surface), or a NaN anywhere, the angle is NaN and nothing is culled. For a pinhole a = beta = 0 and
// every rule is the one above, bit for bit.
//
// Shutter rays (rbrt_hip.h "Camera shutter"; TraceParams::shutter). A shutter ray is a pinhole or lens ray (o, d) whose origin
// moves to o' = o + t travel, 0 <= t < 1, and whose direction stays d, bit for bit. Two kinds of quantity used `a` above, and
// the shutter touches one of them only:
//   the ORIGIN's distance from the position: |o' - position| <= a + |travel|. In float, t travel_c is one rounding (at most
//     u |travel|) and the sum another (at most u (|o| + |travel|)); 16 u (|position| + a + |travel|), the lens's own u16 term,
//     covers both many times over. That is `org_a` = a + |travel| + 16 u (|position| + a + |travel|). It takes a's place
//     wherever a stood for where a ray STARTS: the radii R_out + org_a and R_in - org_a, the slabs' reach and
//     box_unreachable's (org_a + w (l + r + org_a), org_a + w (far + org_a): a point of the line o' + s d is within
//     org_a + |s| sin w of the line through the position with a direction of the tile's cone, as before), the box's bounding
//     sphere, and the float-error slacks that hold the origin's distance from the object (the sphere test's, the box test's,
//     the tree pad, whose |o|_inf grows by org_a).
//   the DIRECTION's angle to the tile's pinhole directions: beta = asin(a / (focus_scale plane_dist)) and the float error
//     `angle` of normalize(F - o), with |F - o| >= focus_scale plane_dist - a. d is the unshuttered ray's, so these keep `a`
//     (`lens_a`): the shutter widens neither the cone nor the deep-cut caps nor w. For a pinhole with a shutter beta = 0 and
//     `angle` is the pinhole's.
// The argument for backward lines is the lens's: a line from o' cuts (misses) the ball as a line from the position cuts (misses)
// the ball moved by position - o', which contains the ball of radius R - org_a (lies inside the one of radius R + org_a) around
// the same centre; the forward rule R_out < l keeps every origin outside the sphere. Without a shutter org_a = a exactly (the
// branch is not taken) and every rule is the one above, bit for bit. A travel so long that R_out >= l for every object, or
// a NaN, makes every comparison false: nothing is culled.
//
// Moving spheres (rbrt_hip.h "Moving spheres"; TraceParams::motion). The camera ray of a sample with the draw t tests sphere i
// at c_i(t) = fl(c_i + fl(t travel_i)), 0 <= t < 1. A line from o' meets the ball around c_i(t) as the line from
// o' - (c_i(t) - c_i), with the same direction, meets the ball around c_i: the argument above for a moved origin, per
// sphere. That origin is within org_a + |c_i(t) - c_i| of the position, and |c_i(t) - c_i| <= |travel_i| + the float error of
// the two operations: the product is one rounding per component (at most u |travel_i| in length), the sum another (at most
// u (|c_i| + |travel_i|)); 16 u (|c_i| + |travel_i|) covers both many times over. Hence, for sphere i alone,
//     org_a_i = org_a + |travel_i| + 16 u (|c_i| + |travel_i|)
// wherever org_a stands in its rule: lo, slack, reach, r_out, r_in. The direction is the unmoved ray's, so the cone, the
// caps and w keep their numbers, and mesh boxes -- which do not move -- keep org_a. The shutter's t and the motion's t are
// the same draw, which the bound never uses: it holds for every pair of them. Without a motion org_a_i = org_a exactly (the
// branch is not taken) and every word is what it was, bit for bit. The bit proves the CAMERA ray's test fails; a bounce ray
// of the path tests every sphere.
//
// A phase (rbrt_hip.h "Animation"; TraceParams::motion_phase = ph). The camera ray of a sample with the draw t tests sphere i at
// c_i(s) = fl(c_i + fl(s travel_i)), s = fl(ph + t). The bound follows the sphere: it is made around the ADVANCED centre
// C_i = c_i + ph travel_i, which the kernel has in double (the product of two floats is exact there, the sum rounds at 2^-53),
// not around c_i with (|ph| + 1) |travel_i| of margin, under which nothing would be culled at frame 40. What is left between
// C_i and c_i(s), with |s| <= (|ph| + 1)(1 + u):
//     s = ph + t + e_s, |e_s| <= u (|ph| + 1)                      the ONE rounding the phase adds
//     s travel_i - ph travel_i = (t + e_s) travel_i                 at most |travel_i| + u (|ph| + 1) |travel_i| long
//     fl(s travel_i): one rounding per component                    at most u |s| |travel_i| <= u (1 + u) (|ph| + 1) |travel_i|
//     fl(c_i + ...): one rounding per component                     at most u (|c_i| + (1 + 2u) (|ph| + 1) |travel_i|)
// together |c_i(s) - C_i| <= |travel_i| + 3 u (|c_i| + (|ph| + 1) |travel_i|) + O(u^2): the candidate
//     org_a_i = org_a + |travel_i| + 16 u (|c_i| + (|ph| + 1) |travel_i|)
// covers the float error five times over, C_i's own rounding in double included. q = (c_i - position) + ph travel_i, and l and
// qhat are taken from it (in that order, so that the centre's registers are free before the product is made). With
// ph = 0, C_i = c_i exactly and the margin is the one above: every word is what it was without a phase, bit for bit. The
// margin grows with |ph| only through the rounding term, 1e-6 (|ph| + 1) |travel_i|.
//
// Moving meshes (rbrt_hip.h "Moving meshes"; TraceParams::mesh_motion, w = w_m, ph the phase). The camera ray (o', d) of a sample
// with the draw t tests mesh m -- its box gate, and through make_cull the grown boxes of its tree -- as the ray (o_m, d),
// o_m = fl(o' - fl(s w)), s = fl(ph + t), 0 <= t < 1: the mesh, its box and its tree at rest, the direction bit for bit. So
// bit 24 + m and the descent ask the questions above of a ray that starts somewhere else, and, as for a sphere, the bound
// follows the object: mesh m gets its own position, advanced in double,
//     pos_m = position - ph w          (the product of two floats is exact in double; the difference rounds at 2^-53)
// and its own bound on where a ray starts relative to it. What is left between pos_m and o_m:
//     o' - position                                                 at most org_a long (lens and shutter, above)
//     s = ph + t + e_s, |e_s| <= u (|ph| + 1)                      so s w - ph w = (t + e_s) w: at most |w| + u (|ph| + 1) |w|
//     fl(s w): one rounding per component                           at most u |s| |w| <= u (1 + u) (|ph| + 1) |w|
//     fl(o' - ...): one rounding per component                      at most u (|position| + org_a + (1 + 2u) (|ph| + 1) |w|)
// together |o_m - pos_m| <= org_a + |w| + 3 u (|position| + org_a + (|ph| + 1) |w|) + O(u^2): the candidate
//     org_a_m = org_a + |w| + 16 u (|position| + org_a + (|ph| + 1) |w|)
// covers the float error five times over, pos_m's own rounding included. pos_m and org_a_m take the place of pos and org_a
// wherever they stand for mesh m: the corners' distances (`far`, the finiteness test), the box slack 16 u (far + org_a_m),
// box_unreachable's centre, bounding sphere, `reach` and corner vectors, and the tree pad's dlen(mc), |o|_inf (of pos_m, plus
// org_a_m) and org_a. The slabs' planes pass through pos_m with the normals they had and the cone keeps its axis and angles:
// those are made of DIRECTIONS, and d is the unmoved ray's. The time the bound never uses is the one draw the shutter and
// the spheres share: it holds for every t. Without a mesh motion pos_m = pos and org_a_m = org_a exactly (the branch is not
// taken) and every word of the table is what it was. The bit proves the CAMERA ray's test fails; a bounce ray tests every mesh.
// ---------------------------------------------------------------------------------------------
struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 d3(const float* p) { return D3{double(p[0]), double(p[1]), double(p[2])}; }
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return D3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dlen(D3 a) { return sqrt(ddot(a, a)); }
__device__ __forceinline__ D3 unit_or_nan(D3 v) { return (1.0 / dlen(v)) * v; }  // (a zero vector gives NaN: nothing is culled with it)
__device__ __forceinline__ double angle_between(D3 u, D3 v) {  // unit vectors; NaN stays NaN
    const double c = ddot(u, v);
    return acos(c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c);
}

// Two planes through the camera position (unit normals) bounding the camera lines of a pixel interval.
struct CullSlab {
    D3 n_lo, n_hi;
    // every point within `reach` of q (relative to the position) strictly on one and the same side of both planes?
    __device__ __forceinline__ bool outside(D3 q, double reach) const {
        const double g0 = ddot(n_lo, q), g1 = ddot(n_hi, q);
        return (g0 > reach && g1 > reach) || (g0 < -reach && g1 < -reach);  // (false for NaN)
    }
};
// The tile's ray directions: inside the cone of half-angle rho around mid (unit). The angle comparisons of the header are
// made on cosines (one square root per ball instead of an arc cosine and an arc sine): for t in [0, pi] and 0 <= a + rho
// <= pi, t > a + rho is cos t < cos a cos rho - sin a sin rho, with sin a = R / l.
struct CullCone {
    D3 mid;
    double cos_rho, sin_rho;  // rho < pi / 2 (else NaN: nothing is culled)
    // forward rays (sign +1) or backward extensions (sign -1) all miss the ball of radius R at q = l * qhat?
    __device__ __forceinline__ bool misses(D3 qhat, double l, double R, double sign) const {
        if (!(R < l)) return false;
        const double sa = R / l, ca = sqrt(1.0 - sa * sa);
        return sign * ddot(mid, qhat) < ca * cos_rho - sa * sin_rho;  // (false for NaN)
    }
    // (a cap of less than a quarter turn is convex on the sphere: the four corners inside it put the whole tile inside)
    D3 corner[4];
    double cos_w, sin_w;  // w: the float ray's direction error
    __device__ __forceinline__ bool backward_deep(D3 qhat, double l, double r_in) const {
        if (!(r_in > 0.0 && r_in < l)) return false;
        const double sa = r_in / l, ca = sqrt(1.0 - sa * sa);
        if (!(sa > sin_w)) return false;                 // the cap asin(r_in / l) - w must be a cap
        const double cos_cap = ca * cos_w + sa * sin_w;  // cos(asin(r_in / l) - w)
        bool in = true;
        for (uint32_t k = 0; k < 4u; ++k) in = in && -ddot(corner[k], qhat) > cos_cap;
        return in;
    }
};

// FOUR lanes per tile (round 4). The kernel's time was the longest walk over the top of a mesh's tree -- a tile at the
// mesh's silhouette tests the four child boxes of some twenty nodes one after the other, in double precision, a chain of
// ~40,000 dependent operations: 0.12 ms for 12,288 tiles, in front of every frame with a new camera. The four lanes of a
// tile compute the same prologue and the same sphere bits (cheap, redundant) and share the walk: every lane pops the same
// node and tests ONE of its four children, a wave vote brings the quad's four answers to each of its lanes, and every
// lane pushes the same entries on its own copy of the stack (no LDS, no hand-over).
constexpr int kCullBlock = 64;       // one wave per workgroup: the launch spreads over the CUs
constexpr uint32_t kCullLanes = 4;   // lanes per tile
// (at most 128 VGPRs, like a trace wave: a wave of this kernel then fits the slot ONE exiting trace wave leaves on its SIMD;
// at 140 it needed two of them to have left)
// (MM: the build for a launch with a mesh motion, "Moving meshes"; every other launch runs the code it always has)
template <bool MM>
__global__ __launch_bounds__(kCullBlock, 4) void primary_cull_kernel(const TraceParams P) {
    // (a rank of a multi-GPU render makes the words of ITS tiles only -- tile = local * world + rank, the only words its
    // lists and its launch read: an eighth of the pass for an eighth of the frame)
    const uint32_t cull_world = P.tile_world > 1u ? P.tile_world : 1u;
    const uint32_t tile_local = (blockIdx.x * kCullBlock + threadIdx.x) / kCullLanes;
    const uint32_t tile = tile_local * cull_world + (cull_world > 1u ? P.tile_rank : 0u);
    const uint32_t quad_lane = threadIdx.x % kCullLanes, quad_shift = threadIdx.x & ~(kCullLanes - 1u);
    if (tile >= P.n_tiles) return;  // (whole quads: the votes below count active lanes only)
    uint32_t ty, tx;
    tile_xy(tile, P.tiles_x, ty, tx);
    const rbrt_camera_t& c = P.cam;
    const uint32_t W = c.img_width_pix, H = c.img_height_pix;
    const D3 pos = d3(c.position), right = d3(c.right), up = d3(c.up), ctr = d3(c.img_center_point);
    const D3 a = ctr - pos;
    // the tile's pixel interval in the units of cam.rs:70-75, widened
    const double pad = 1e-3 + double(W > H ? W : H) * (1.0 / 4194304.0);
    const uint32_t c0 = tx * RBRT_TILE, r0 = ty * RBRT_TILE;
    const uint32_t c1 = (c0 + RBRT_TILE < W ? c0 + RBRT_TILE : W) - 1u, r1 = (r0 + RBRT_TILE < H ? r0 + RBRT_TILE : H) - 1u;
    const double mmh = double(c.mm_per_pix_hor), mmv = double(c.mm_per_pix_vert);
    const double cm0 = (double(c0) - double(W / 2u) - 0.5 - pad) * mmh, cm1 = (double(c1) - double(W / 2u) + 0.5 + pad) * mmh;
    const double rm0 = (double(r0) - double(H / 2u) - 0.5 - pad) * mmv, rm1 = (double(r1) - double(H / 2u) + 0.5 + pad) * mmv;
    // the float ray against the exact line: absolute error of (target - position), as an angle
    const double cm_abs = fabs(cm0) > fabs(cm1) ? fabs(cm0) : fabs(cm1), rm_abs = fabs(rm0) > fabs(rm1) ? fabs(rm0) : fabs(rm1);
    const double err = 8.0 * (1.0 / 8388608.0) * (dlen(ctr) + dlen(pos) + 0.001 * cm_abs * dlen(right) + 0.001 * rm_abs * dlen(up));
    const double plane_dist = fabs(ddot(a, unit_or_nan(dcross(right, up))));  // no target is closer to the position
    double angle = 2.0 * err / plane_dist + 1e-6;                                // (NaN or inf for a degenerate camera)
    // Lens rays (header, "Lens rays"): lens_a bounds |o - position|, lens_beta the angle between a lens ray's exact direction
    // and the pinhole direction of its target, `angle` becomes the float error of the lens ray's direction. 0 for a pinhole.
    double lens_a = 0.0, lens_beta = 0.0;
    if (P.thin_lens) {
        const D3 lu = d3(P.lens_u), lv = d3(P.lens_v);
        const double fs = double(P.focus_scale), nu = dlen(lu), nv = dlen(lv);
        const double u16 = 16.0 * (1.0 / 16777216.0);
        double tmax = 0.0;  // the farthest target: a corner (|T - position| is convex)
        for (uint32_t k = 0; k < 4u; ++k) {
            const double t = dlen(a + (0.001 * (k & 1u ? cm1 : cm0)) * right - (0.001 * (k & 2u ? rm1 : rm0)) * up);
            tmax = t > tmax || !(t == t) ? t : tmax;
        }
        lens_a = sqrt(nu * nu + nv * nv) + u16 * (dlen(pos) + nu + nv);
        const double f_min = fs * plane_dist;  // |F - position| >= focus_scale * plane_dist
        const double err_f = fs * err + u16 * (dlen(pos) + 2.0 * fs * tmax + lens_a);
        angle = 2.0 * err_f / (f_min - lens_a) + 1e-6;
        const double sb = lens_a / f_min;      // sin beta
        lens_beta = sb / sqrt(1.0 - sb * sb);  // tan beta >= beta (no asin: its code cost the pass VGPR spills)
        if (!(sb < 1.0) || !(lens_beta == lens_beta)) angle = __builtin_nan("");  // (nothing is culled)
    }
    // Shutter rays (header, "Shutter rays"): org_a bounds the distance of a ray's origin from the position, lens_a goes on
    // bounding what enters its direction. Without a shutter they are the same number.
    double org_a = lens_a;
    if (P.shutter) {
        const double tl = dlen(d3(P.travel));
        org_a = lens_a + tl + 16.0 * (1.0 / 16777216.0) * (dlen(pos) + lens_a + tl);
        if (!(org_a == org_a)) angle = __builtin_nan("");  // (nothing is culled)
    }
    CullSlab cols, rows;
    cols.n_lo = unit_or_nan(dcross(a + (0.001 * cm0) * right, up));
    cols.n_hi = unit_or_nan(dcross(a + (0.001 * cm1) * right, up));
    rows.n_lo = unit_or_nan(dcross(a - (0.001 * rm0) * up, right));
    rows.n_hi = unit_or_nan(dcross(a - (0.001 * rm1) * up, right));
    CullCone cone;
    cone.mid = unit_or_nan(a + (0.0005 * (cm0 + cm1)) * right - (0.0005 * (rm0 + rm1)) * up);
    double rho = 0.0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const D3 u = unit_or_nan(a + (0.001 * (k & 1u ? cm1 : cm0)) * right - (0.001 * (k & 2u ? rm1 : rm0)) * up);
        cone.corner[k] = u;
        const double t = angle_between(cone.mid, u);
        rho = t > rho || !(t == t) ? t : rho;  // (a NaN sticks)
    }
    const double w_dir = angle + lens_beta;  // a ray's direction: within this of the exact pinhole lines of the tile
    rho += w_dir;
    if (!(rho < 1.5)) rho = __builtin_nan("");  // (a tile a quarter turn wide: no rule applies)
    cone.cos_rho = cos(rho), cone.sin_rho = sin(rho);
    cone.cos_w = cos(w_dir), cone.sin_w = sin(w_dir);

    const double org_all = org_a;  // (the spheres shadow the name with their own: "Moving spheres")
    const uint32_t n_elem = P.n_spheres + P.n_elem_tris;
    uint32_t word = 0;
    bool all = n_elem <= 24u && P.n_meshes <= 7u && P.n_elem_tris == 0u;
    for (uint32_t e = 0; e < n_elem && e < 24u; ++e) {
        const uint32_t desc = P.elems ? P.elems[e] : e;
        bool out = false;
        if (!(desc >> 31)) {
            const DevSphere sp = P.spheres[desc];
            // Moving spheres (header, "Moving spheres", "A phase"): this sphere's own bound on where a ray starts RELATIVE TO IT,
            // around the centre the phase has advanced it to. Without a motion they are org_a and the centre themselves (the
            // branch is not taken).
            D3 q = d3(sp.center) - pos;
            double org_a = org_all;
            if (P.motion) {
                const D3 tv = d3(P.motion + desc * kMotionDw);
                const double ph = double(P.motion_phase), tl = dlen(tv);
                org_a = org_all + tl + 16.0 * (1.0 / 16777216.0) * (dlen(d3(sp.center)) + (fabs(ph) + 1.0) * tl);
                q = q + ph * tv;  // (C_i - position)
            }
            const double r = double(sp.radius), l = dlen(q);
            if (r > 0.0 && r < 1e30 && l < 1e30) {  // (false for NaN)
                // (the second term is the analysed one, 15x the bound in the header; the others are loose change on top)
                const double lo = l + org_a;  // (the distance of a ray's origin from the centre)
                const double slack = 1e-5 * r + 1e-5 * (lo * lo + r * r) / r + 1e-6 * lo;
                const double reach = r + slack + org_a + w_dir * (l + r + org_a);
                const double r_out = r + slack + org_a, r_in = r - slack - org_a;
                const D3 qhat = (1.0 / l) * q;
                out = cols.outside(q, reach) || rows.outside(q, reach) ||
                      (cone.misses(qhat, l, r_out, 1.0) && (cone.misses(qhat, l, r_out, -1.0) || cone.backward_deep(qhat, l, r_in)));
            }
        }
        if (out) word |= 1u << e;
        else all = false;
    }
    // can a forward camera ray of the tile enter this box? (bounding sphere against the cone; corners against the slabs)
    // (pos, org_a: the camera's, or mesh m's own in a launch with a mesh motion -- header, "Moving meshes")
    const auto box_unreachable = [&](D3 lo, D3 hi, double slack, double far, D3 pos, double org_a) -> bool {
        const D3 q = 0.5 * (lo + hi) - pos;
        const double l = dlen(q);
        if (cone.misses((1.0 / l) * q, l, 0.5 * dlen(hi - lo) * 1.001 + slack + org_a, 1.0)) return true;
        const double reach = slack + org_a + w_dir * (far + org_a);
        for (uint32_t slab = 0; slab < 2u; ++slab) {
            const CullSlab& sl = slab ? rows : cols;
            bool pos_side = true, neg_side = true;
            for (uint32_t k = 0; k < 8u; ++k) {
                const D3 v = D3{k & 1u ? hi.x : lo.x, k & 2u ? hi.y : lo.y, k & 4u ? hi.z : lo.z} - pos;
                const double g0 = ddot(sl.n_lo, v), g1 = ddot(sl.n_hi, v);
                pos_side = pos_side && g0 > reach && g1 > reach;
                neg_side = neg_side && g0 < -reach && g1 < -reach;
            }
            if (pos_side || neg_side) return true;
        }
        return false;
    };
    for (uint32_t m = 0; m < P.n_meshes && m < 7u; ++m) {
        const DevMesh& md = P.meshes[m];
        // Moving meshes (header): this mesh's own position and origin bound. Without a mesh motion they are the camera's.
        D3 pos = d3(c.position);
        double org_a = org_all;
        if (MM) {
            const D3 tv = d3(P.mesh_motion + m * kMeshMotionDw);
            const double ph = double(P.motion_phase), tl = dlen(tv);
            org_a = org_all + tl + 16.0 * (1.0 / 16777216.0) * (dlen(pos) + org_all + (fabs(ph) + 1.0) * tl);
            pos = pos - ph * tv;
        }
        double far = 0.0;
        bool finite = true;
        for (uint32_t k = 0; k < 8u; ++k) {
            const D3 q = D3{double(k & 1u ? md.bbox_hi[0] : md.bbox_lo[0]), double(k & 2u ? md.bbox_hi[1] : md.bbox_lo[1]),
                            double(k & 4u ? md.bbox_hi[2] : md.bbox_lo[2])} - pos;
            const double l = dlen(q);
            finite = finite && l < 1e30;
            far = l > far ? l : far;
        }
        // The mesh's own box, aabbox.rs:28-58 in float (u = 2^-24). Per axis the two quotients t = (plane - o) / d carry one
        // rounding of the difference and one of the division: t~ = t (1 + e), |e| <= 2u + u^2. If the float test passes
        // (t_max >= 0, t_min <= t_max) there is an s >= 0 with, on every axis, min(t~lo, t~hi) <= s <= max(t~lo, t~hi); the
        // point o + s d of the float ray then has every coordinate within 2u |plane - o| + u |plane - o| <= 3u far of the
        // interval [lo, hi] (o + t d = plane exactly for the exact t): it lies within 3 sqrt(3) u far = 3.1e-7 far of the
        // box, on the forward half of the ray. (A zero direction component makes the quotients +-inf or NaN; fmin / fmax
        // skip a NaN, and an axis whose line runs outside its slab gives t_min = +inf or t_max = -inf: a miss, as in
        // geometry.) The slack is 16 u far, three times that bound; the angle between the float ray and the exact
        // line of its pixel is added on top by box_unreachable (angle * far). Round 3 had a chosen 1e-4 far here.
        const double slack = 16.0 * (1.0 / 16777216.0) * (far + org_a);
        const bool out = finite && box_unreachable(d3(md.bbox_lo), d3(md.bbox_hi), slack, far, pos, org_a);
        if (out) word |= 1u << (24u + m);
        // A ray may pass the mesh's box and still have no triangle to hit: the tile is free of the mesh as well when
        // every box in the top kCullLevels levels of its tree is out of the tile's reach. Depth first, descending only where
        // a box is in reach. "Reach" for a tree box is what the TRAVERSAL grows it by (the header of this file's BVH section,
        // make_cull): a triangle the float Moller-Trumbore test accepts has its point within 18 u (K |d| + 1) S of the exact
        // triangle, K = |e1||e2| / eps -- the |a| >= eps rule bounds the amplification, and for a large triangle met at a
        // grazing angle that is far more than a few ulp -- so every child box is grown by the pad the trace kernel itself
        // would use for a ray from this position, 64 u (S + |o|_inf) (max|e1||e2| of the child's subtree * |d| / eps + 1)
        // with |d| <= 1.001: a camera ray that takes a triangle passes inside every ancestor's grown box, so a tile none
        // of whose rays enters a grown box of some level takes no triangle below it.
        const D3 mc = d3(md.center) - pos;
        const double o_inf = fmax(fmax(fabs(pos.x), fabs(pos.y)), fabs(pos.z));
        const double pad_base = 64.0 * (1.0 / 16777216.0) * (dlen(mc) + double(md.radius) + o_inf + org_a);
        bool mesh_free = out;
        if (!out && all && finite && md.n_nodes != 0u) {  // (only where the answer matters: nothing else is in reach so far)
            constexpr uint32_t kCullLevels = 6;
            uint32_t stack[3 * kCullLevels + 4];
            uint32_t sp = 0;
            stack[sp++] = 0u;  // (node index << 3 | level)
            mesh_free = true;
            while (sp != 0u && mesh_free) {  // (uniform over the tile's four lanes: they hold the same stack)
                const uint32_t e = stack[--sp];
                const BvhNode4& nd = md.nodes[e >> 3];
                // this lane's child: 0 = no box or out of reach, 1 = in reach and to be opened, 2 = in reach and not to be
                // opened (a leaf, the level limit, a full stack, a box this rule does not understand): the mesh stays
                const uint32_t c = quad_lane;
                const int32_t link = nd.child[c];
                uint32_t state = 0u;
                if (link != kNoChild) {
                    const D3 lo = D3{double(nd.lo_x[c]), double(nd.lo_y[c]), double(nd.lo_z[c])};
                    const D3 hi = D3{double(nd.hi_x[c]), double(nd.hi_y[c]), double(nd.hi_z[c])};
                    if (!(dlen(lo - pos) < 1e30 && dlen(hi - pos) < 1e30)) state = 2u;
                    else if (!box_unreachable(lo, hi, pad_base * (double(nd.max_e12[c]) * 1.001 * double(P.eps_frac) + 1.0), far, pos, org_a))
                        state = (link >= 0 && (e & 7u) + 1u < kCullLevels) ? 1u : 2u;
                }
                const uint32_t open = uint32_t(__builtin_amdgcn_ballot_w64(state == 1u) >> quad_shift) & 15u;
                const uint32_t stay = uint32_t(__builtin_amdgcn_ballot_w64(state == 2u) >> quad_shift) & 15u;
                if (stay != 0u) mesh_free = false;
                for (uint32_t k = 0; k < 4u && mesh_free; ++k) {
                    if (!((open >> k) & 1u)) continue;
                    if (sp < 3u * kCullLevels + 4u) stack[sp++] = (uint32_t(nd.child[k]) << 3) | ((e & 7u) + 1u);
                    else mesh_free = false;
                }
            }
        }
        if (!mesh_free) all = false;
    }
    if (all) word |= 1u << 31;
    if (quad_lane == 0u) P.tile_cull[tile] = word;
}

// The rank's tiles split by what primary_cull_kernel found, each list in ascending order (TraceParams::tile_lists): one
// workgroup, every thread a contiguous run of local tiles, an exclusive scan of the runs' counts in between.
// (ONE wave and no LDS -- the scan is made of wave shuffles: when the camera changes in the middle of a stream of frames this
// kernel has to find room beside resident trace waves, which hold every wave slot and all of every CU's LDS. A 1024-thread
// workgroup waited milliseconds for a whole free CU (round 3), the 256-thread one with its 2 KB of LDS that followed still
// needed four free slots on one CU at once (round 4's trace: up to 3 ms).)
// kListBlock = 256 (four waves, 32 bytes of LDS for their totals) is the form for a launch that has the GPU to itself -- nothing
// to fit beside, and a quarter of the table per wave: 0.075 -> 0.03 ms in front of a blocking frame of a new camera.
template <int kListBlock>
__global__ __launch_bounds__(kListBlock) void tile_lists_kernel(const TraceParams P) {
    const uint32_t n = P.n_local_tiles, t = threadIdx.x;
    const uint32_t per = (n + kListBlock - 1) / kListBlock;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    // class of a tile: 2 = background only; 1 = light (no mesh box in reach, at most one sphere); 0 = heavy
    const uint32_t el_mask = (1u << (P.n_spheres < 24u ? P.n_spheres : 24u)) - 1u, me_mask = (1u << (P.n_meshes < 7u ? P.n_meshes : 7u)) - 1u;
    const auto class_of = [&](uint32_t word) -> uint32_t {
        if (word >> 31) return 2u;
        if (P.tile_list_mode == 0u) return 0u;
        // (the table's element bits are indexed by position in Scene::elements and are only ever set for spheres: with
        // BasicTriangle elements in the scene, which are never culled, no tile is called light)
        const bool light = ((word >> 24) & me_mask) == me_mask && __popc(~word & el_mask) <= 1 && P.n_spheres <= 24u && P.n_meshes <= 7u &&
                           P.n_elem_tris == 0u;
        return light ? 1u : 0u;
    };
    // (one wave walks the whole table, every lane a run of it: the table's words are fetched eight at a time, so that a
    // lane's loads are in flight together instead of one dependent round trip per tile)
    constexpr uint32_t kBatch = 8;
    const auto load_batch = [&](uint32_t tl0, uint32_t (&w)[kBatch]) {
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) w[j] = tl0 + j < hi ? P.tile_cull[(tl0 + j) * P.tile_world + P.tile_rank] : 0x80000000u;
    };
    uint32_t mine[2] = {0u, 0u};  // heavy / light tiles of this run (both go to the trace kernel)
    for (uint32_t tl0 = lo; tl0 < hi; tl0 += kBatch) {
        uint32_t w[kBatch];
        load_batch(tl0, w);
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) {
            const uint32_t c = class_of(w[j]);
            if (tl0 + j < hi && c < 2u) ++mine[c];
        }
    }
    uint32_t incl[2] = {mine[0], mine[1]};
    const uint32_t wlane = t & 63u;
    for (uint32_t d = 1; d < 64u; d <<= 1) {  // inclusive scans over the wave
        const uint32_t v0 = uint32_t(__shfl_up(int(incl[0]), d, 64)), v1 = uint32_t(__shfl_up(int(incl[1]), d, 64));
        if (wlane >= d) incl[0] += v0, incl[1] += v1;
    }
    uint32_t n_heavy = uint32_t(__shfl(int(incl[0]), 63, 64)), n_light = uint32_t(__shfl(int(incl[1]), 63, 64));
    if (kListBlock > 64) {  // ... and over the workgroup's waves, through their totals
        __shared__ uint32_t wave_total[2][kListBlock / 64];
        if (wlane == 63u) wave_total[0][t >> 6] = n_heavy, wave_total[1][t >> 6] = n_light;
        __syncthreads();
        n_heavy = n_light = 0u;
        for (uint32_t w = 0; w < uint32_t(kListBlock / 64); ++w) {
            if (w < (t >> 6)) incl[0] += wave_total[0][w], incl[1] += wave_total[1][w];
            n_heavy += wave_total[0][w], n_light += wave_total[1][w];
        }
    }
    const uint32_t n_work = n_heavy + n_light;
    uint32_t r[2] = {incl[0] - mine[0], incl[1] - mine[1]};  // heavy / light tiles before this run
    uint32_t k = lo - r[0] - r[1];                                  // background-only tiles before it
    uint32_t* const work = P.tile_lists + kTileListHeader;
    uint32_t* const sky = work + n;
    // the work list (tile_list_mode; api.cpp list_mode_for): 0: ascending; 4: the image's row-major order in the direction it
    // is handed out in (P.tiles_reversed: from the last tile down), except that the LAST n_work / tile_tail_div light tiles
    // of that order are taken out of it and handed out at the very end: the bulk of the launch keeps row-major order's mix
    // of traversal-heavy and shading-heavy work in every wave, and the launch drains on light tiles whatever the image
    uint32_t n_tail = n_work / (P.tile_tail_div != 0u ? P.tile_tail_div : 8u);
    n_tail = n_tail < n_light ? n_tail : n_light;
    const uint32_t n_front_light = n_light - n_tail;  // light tiles that stay in row-major order
    for (uint32_t tl0 = lo; tl0 < hi; tl0 += kBatch) {
      uint32_t w[kBatch];
      load_batch(tl0, w);
#pragma unroll
      for (uint32_t j = 0; j < kBatch; ++j) {
        const uint32_t tl = tl0 + j;
        if (tl >= hi) continue;
        const uint32_t c = class_of(w[j]);
        if (c == 2u) {
            sky[k++] = tl;
            continue;
        }
        uint32_t pos;
        if (P.tile_list_mode == 4u) {
            // ranks in hand-out order: heavy and light tiles handed out BEFORE this one
            const bool rev = P.tiles_reversed != 0u;
            const uint32_t h = c == 0u ? (rev ? n_heavy - 1u - r[0] : r[0]) : (rev ? n_heavy - r[0] : r[0]);
            const uint32_t l = c == 1u ? (rev ? n_light - 1u - r[1] : r[1]) : (rev ? n_light - r[1] : r[1]);
            if (c == 1u && l >= n_front_light) pos = (n_work - n_tail) + (l - n_front_light);
            else pos = h + (l < n_front_light ? l : n_front_light);
            ++r[c];
        } else {
            pos = r[0]++;  // (mode 0 puts every tile in class 0)
        }
        work[pos] = tl;
      }
    }
    if (t == kListBlock - 1) {
        P.tile_lists[0] = n_work;
        P.tile_lists[1] = n - n_work;
        P.tile_lists[2] = n_light, P.tile_lists[3] = 0u;
    }
}

__host__ __device__ inline uint32_t local_tiles_of(uint32_t n_tiles, uint32_t rank, uint32_t world) {
    return rank < n_tiles ? (n_tiles - rank + world - 1u) / world : 0u;
}

// ---------------------------------------------------------------------------------------------
// Adaptive sampling (rbrt_hip_render_adaptive; the rule is stated in include/rbrt_hip.h and DESIGN.md section 9).
// A call is a series of rounds. Each round renders a few more samples of the tiles that are still active -- the trace
// kernel and the two resolves below walk the round's own tile lists --, then tile_error_kernel decides which of them go
// on. Every pixel keeps two running sums in sample order: S of all its samples, S_even of those with an even index.
// ---------------------------------------------------------------------------------------------

// resolve_kernel for a round: the batch is added to S and, sample by sample, to S_even; nothing goes out (the round never
// is a call's last batch: adaptive_finish_kernel writes the image). A kernel of its own, so that resolve_kernel stays the
// code it is. No wait for helper waves: the launches of an adaptive call get none (api.cpp issue_batches).
__global__ __launch_bounds__(kSmallBlock) void resolve_even_kernel(const ResolveParams R) {
    const size_t npix = size_t(R.tile_lists[0]) * 64u;
    const size_t i = size_t(blockIdx.x) * kSmallBlock + threadIdx.x;
    if (blockIdx.x == 0) {  // (as resolve_kernel: the launch's number, then its work counters for the lane's next launch)
        if (R.helper_words && threadIdx.x == 0) {
            __hip_atomic_store(R.helper_words + 1, R.helper_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < kWorkShards * kWorkCounterStride; w += kSmallBlock) R.work_counter[w] = 0ull;
    }
    if (i >= npix) return;
    const uint32_t p = uint32_t(i & 63u);
    const uint32_t tile_local = R.tile_lists[kTileListHeader + (i >> 6)];
    const size_t j = size_t(tile_local) * 64u + p;
    const uint32_t tile = tile_local * R.tile_world + R.tile_rank;
    uint32_t ty, tx;
    tile_xy(tile, R.tiles_x, ty, tx);
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    if (!(row < R.height && col < R.width)) return;  // (a slot beyond a ragged edge: its sums are never read)
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ex = 0.0f, ey = 0.0f, ez = 0.0f;
    if (!R.first_batch) {
        ax = R.acc[j * 3 + 0], ay = R.acc[j * 3 + 1], az = R.acc[j * 3 + 2];
        ex = R.acc_even[j * 3 + 0], ey = R.acc_even[j * 3 + 1], ez = R.acc_even[j * 3 + 2];
    }
    for (uint32_t s = 0; s < R.batch; ++s) {
        const float* sp = R.sample_buf + (size_t(s) * npix + i) * 3u;
        const float cx = sp[0], cy = sp[1], cz = sp[2];
        ax = ax + cx;
        ay = ay + cy;
        az = az + cz;
        if (((R.sample_base + s) & 1u) == 0u) {
            ex = ex + cx;
            ey = ey + cy;
            ez = ez + cz;
        }
    }
    R.acc[j * 3 + 0] = ax, R.acc[j * 3 + 1] = ay, R.acc[j * 3 + 2] = az;
    R.acc_even[j * 3 + 0] = ex, R.acc_even[j * 3 + 1] = ey, R.acc_even[j * 3 + 2] = ez;
}

// sky_resolve_kernel for a round: the same samples, the same order, into both sums.
__global__ __launch_bounds__(kSmallBlock) void sky_resolve_even_kernel(const TraceParams P, const ResolveParams R) {
    const size_t i = size_t(blockIdx.x) * kSmallBlock + threadIdx.x;
    if (i >= size_t(R.tile_lists[1]) * 64u) return;
    const uint32_t p = uint32_t(i & 63u);
    const uint32_t tile_local = R.tile_lists[kTileListHeader + R.n_local_tiles + (i >> 6)];
    const size_t j = size_t(tile_local) * 64u + p;
    const uint32_t tile = tile_local * R.tile_world + R.tile_rank;
    uint32_t ty, tx;
    tile_xy(tile, R.tiles_x, ty, tx);
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    if (!(row < R.height && col < R.width)) return;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ex = 0.0f, ey = 0.0f, ez = 0.0f;
    if (!R.first_batch) {
        ax = R.acc[j * 3 + 0], ay = R.acc[j * 3 + 1], az = R.acc[j * 3 + 2];
        ex = R.acc_even[j * 3 + 0], ey = R.acc_even[j * 3 + 1], ez = R.acc_even[j * 3 + 2];
    }
    const V3 pos = mk(P.cam.position), center = mk(P.cam.img_center_point), right = mk(P.cam.right), up = mk(P.cam.up);
    for (uint32_t s = 0; s < R.batch; ++s) {
        Rng rng;
        rng.init(P.seed_key, row * R.width + col, P.sample_base + s);
        V3 o = pos, f = camera_target(center, right, up, P.cam.mm_per_pix_hor, P.cam.mm_per_pix_vert, R.width, R.height, row, col, rng);
        if (P.thin_lens) {
            const float lens[7] = {P.lens_u[0], P.lens_u[1], P.lens_u[2], P.lens_v[0], P.lens_v[1], P.lens_v[2], P.focus_scale};
            lens_point(o, f, lens, rng);
        }
        const V3 d = normalize(f - o);
        const V3 c = P.env_nodes ? environment_radiance(P.env_nodes, P.env_n, d) : background(d.y, P.bg, P.constant_bg);
        ax = ax + c.x;
        ay = ay + c.y;
        az = az + c.z;
        if (((P.sample_base + s) & 1u) == 0u) {
            ex = ex + c.x;
            ey = ey + c.y;
            ez = ez + c.z;
        }
    }
    R.acc[j * 3 + 0] = ax, R.acc[j * 3 + 1] = ay, R.acc[j * 3 + 2] = az;
    R.acc_even[j * 3 + 0] = ex, R.acc_even[j * 3 + 1] = ey, R.acc_even[j * 3 + 2] = ez;
}

// The round's tile lists: the rank's ACTIVE tiles, those that see only the background (bit 31 of their culling word) on the
// second list, the others on the work list, both ascending; inactive tiles on neither. One wave and no LDS, as
// tile_lists_kernel<64>: every lane a contiguous run of local tiles, an exclusive scan of the runs' counts in between.
// Also zeroes the count tile_error_kernel adds to.
__global__ __launch_bounds__(64) void adaptive_lists_kernel(const AdaptiveParams A) {
    const uint32_t n = A.n_local_tiles, t = threadIdx.x;
    const uint32_t per = (n + 63u) / 64u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    // class of a tile: 0 = work list, 1 = background only, 2 = inactive
    const auto class_of = [&](uint32_t tl) -> uint32_t {
        if (!A.first_round && A.active[tl] == 0u) return 2u;
        return A.tile_cull ? A.tile_cull[tl * A.tile_world + A.tile_rank] >> 31 : 0u;
    };
    uint32_t mine[2] = {0u, 0u};
    for (uint32_t tl = lo; tl < hi; ++tl) {
        const uint32_t c = class_of(tl);
        if (c < 2u) ++mine[c];
    }
    uint32_t incl[2] = {mine[0], mine[1]};
    for (uint32_t d = 1; d < 64u; d <<= 1) {  // inclusive scans over the wave
        const uint32_t v0 = uint32_t(__shfl_up(int(incl[0]), d, 64)), v1 = uint32_t(__shfl_up(int(incl[1]), d, 64));
        if (t >= d) incl[0] += v0, incl[1] += v1;
    }
    const uint32_t n_work = uint32_t(__shfl(int(incl[0]), 63, 64)), n_sky = uint32_t(__shfl(int(incl[1]), 63, 64));
    uint32_t r[2] = {incl[0] - mine[0], incl[1] - mine[1]};  // tiles of either list before this run
    uint32_t* const work = A.tile_lists + kTileListHeader;
    uint32_t* const sky = work + n;
    for (uint32_t tl = lo; tl < hi; ++tl) {
        const uint32_t c = class_of(tl);
        if (c == 0u) work[r[0]++] = tl;
        else if (c == 1u) sky[r[1]++] = tl;
    }
    if (t == 63u) {
        A.tile_lists[0] = n_work;
        A.tile_lists[1] = n_sky;
        A.tile_lists[2] = 0u, A.tile_lists[3] = 0u;  // (no light tiles: the list is in mode 0's order)
        *A.n_active = 0u;
    }
}

// After a round: one wave per tile of the round's two lists, lane p = pixel p. The tile's error E by the half-buffer
// estimate (float32, unfused, in the order of the rule), its count and whether it goes on; the tiles that go on are
// counted, one atomic per wave.
__global__ __launch_bounds__(64) void tile_error_kernel(const AdaptiveParams A) {
    const uint32_t w = blockIdx.x, p = threadIdx.x;
    const uint32_t n_work = A.tile_lists[0], n_sky = A.tile_lists[1];
    if (w >= n_work + n_sky) return;  // (the grid is the host's count of active tiles: never smaller than the lists)
    const uint32_t tile_local = w < n_work ? A.tile_lists[kTileListHeader + w] : A.tile_lists[kTileListHeader + A.n_local_tiles + (w - n_work)];
    const size_t j = size_t(tile_local) * 64u + p;
    const uint32_t tile = tile_local * A.tile_world + A.tile_rank;
    uint32_t ty, tx;
    tile_xy(tile, A.tiles_x, ty, tx);
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    const uint32_t h = (A.n + 1u) / 2u;
    const float inv_n = 1.0f / float(A.n), inv_h = 1.0f / float(h);
    float q = 0.0f;
    if (row < A.height && col < A.width) {
        const float ir = A.acc[j * 3 + 0] * inv_n, ig = A.acc[j * 3 + 1] * inv_n, ib = A.acc[j * 3 + 2] * inv_n;
        const float ar = A.acc_even[j * 3 + 0] * inv_h, ag = A.acc_even[j * 3 + 1] * inv_h, ab = A.acc_even[j * 3 + 2] * inv_h;
        const float e = (__builtin_fabsf(ir - ar) + __builtin_fabsf(ig - ag)) + __builtin_fabsf(ib - ab);
        q = e / (__builtin_sqrtf((ir + ig) + ib) + 0.0001f);
    }
    float v = q;
    for (uint32_t d = 1; d < 64u; d <<= 1) v = v + __shfl_xor(v, int(d), 64);  // (a + b == b + a: every lane ends with the same bits)
    const uint32_t rows_in = A.height - ty * RBRT_TILE < RBRT_TILE ? A.height - ty * RBRT_TILE : RBRT_TILE;
    const uint32_t cols_in = A.width - tx * RBRT_TILE < RBRT_TILE ? A.width - tx * RBRT_TILE : RBRT_TILE;
    const float err = v / float(rows_in * cols_in);
    if (p == 0u) {
        const bool go_on = A.n < A.n_max && !(err < A.threshold);  // (a NaN goes on)
        A.tile_samples[tile_local] = A.n;
        A.tile_error[tile_local] = err;
        A.active[tile_local] = go_on ? 1u : 0u;
        if (go_on) atomicAdd(A.n_active, 1u);
    }
}

// The image of an adaptive call: every pixel its S times the reciprocal of its tile's count, then the quantisation;
// indexing and ragged edges as resolve_store's last batch. One thread per pixel slot of the rank.
__global__ __launch_bounds__(kSmallBlock) void adaptive_finish_kernel(const AdaptiveParams A) {
    const size_t i = size_t(blockIdx.x) * kSmallBlock + threadIdx.x;
    if (i >= size_t(A.n_local_tiles) * 64u) return;
    const uint32_t p = uint32_t(i & 63u), tile_local = uint32_t(i >> 6);
    const uint32_t tile = tile_local * A.tile_world + A.tile_rank;
    uint32_t ty, tx;
    tile_xy(tile, A.tiles_x, ty, tx);
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    const bool valid = row < A.height && col < A.width, packed = A.tile_world > 1;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (valid) {
        const float inv = 1.0f / float(A.tile_samples[tile_local]);
        ax = A.acc[i * 3 + 0] * inv;
        ay = A.acc[i * 3 + 1] * inv;
        az = A.acc[i * 3 + 2] * inv;
    } else if (!packed) {
        return;  // (a pixel slot beyond a ragged image edge: packed outputs carry it as zeros)
    }
    const size_t o = packed ? i * 3u : (size_t(row) * A.width + col) * 3u;
    if (A.out_radiance) {
        A.out_radiance[o + 0] = ax;
        A.out_radiance[o + 1] = ay;
        A.out_radiance[o + 2] = az;
    }
    if (A.out_rgb8) {
        A.out_rgb8[o + 0] = quantise(ax);
        A.out_rgb8[o + 1] = quantise(ay);
        A.out_rgb8[o + 2] = quantise(az);
    }
}

// Gathered per-rank packed tiles -> row-major image (rank r's block starts after the blocks of
// ranks < r; inside a block tiles are in ascending global tile order).
__global__ __launch_bounds__(kSmallBlock) void unpack_kernel(const float* __restrict__ gathered, uint32_t width,
                                                        uint32_t height, uint32_t tiles_x, uint32_t n_tiles,
                                                        uint32_t world, size_t rank_stride_pixels, float* out_radiance,
                                                        uint8_t* out_rgb8) {
    const size_t i = size_t(blockIdx.x) * kSmallBlock + threadIdx.x;
    if (i >= size_t(width) * height) return;
    const uint32_t row = uint32_t(i / width), col = uint32_t(i - size_t(row) * width);
    const uint32_t tile = tile_number(row / RBRT_TILE, col / RBRT_TILE, tiles_x);
    const uint32_t rank = tile % world, tile_local = tile / world;
    size_t base = 0;
    if (rank_stride_pixels != 0) {  // equal-size slots per rank (what a gather of equal-size tensors produces)
        base = size_t(rank) * rank_stride_pixels;
    } else {                        // tightly packed
        for (uint32_t r = 0; r < rank; ++r) base += size_t(local_tiles_of(n_tiles, r, world)) * 64u;
    }
    const size_t src = (base + size_t(tile_local) * 64u + (row % RBRT_TILE) * RBRT_TILE + col % RBRT_TILE) * 3u;
    const float x = gathered[src], y = gathered[src + 1], z = gathered[src + 2];
    if (out_radiance) {
        out_radiance[i * 3 + 0] = x;
        out_radiance[i * 3 + 1] = y;
        out_radiance[i * 3 + 2] = z;
    }
    if (out_rgb8) {
        out_rgb8[i * 3 + 0] = quantise(x);
        out_rgb8[i * 3 + 1] = quantise(y);
        out_rgb8[i * 3 + 2] = quantise(z);
    }
}

// Scene::hit for arbitrary rays (test / diagnostic hook behind rbrt_hip_trace_rays).
constexpr int kRaysBlock = 128;
__global__ __launch_bounds__(kRaysBlock) void trace_rays_kernel(const TraceParams P, const float* __restrict__ rays,
                                                            size_t n, float* out_t, int32_t* out_obj,
                                                            int32_t* out_tri, float* out_dist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const size_t i = size_t(blockIdx.x) * kRaysBlock + threadIdx.x;
    if (i >= n) return;
    const V3 o = mk(rays + 6 * i), d = mk(rays + 6 * i + 3);
    HitRec h;
    LocalCounters lc = {0, 0, 0, 0, 0};
    scene_hit<false>(P, o, d, stack, uint32_t(kRaysBlock), h, lc);
    const bool hit = h.obj >= 0;
    const float nanv = __int_as_float(0x7fc00000);
    if (out_t) out_t[i] = hit ? h.t : nanv;
    if (out_obj) out_obj[i] = h.obj;
    if (out_tri) out_tri[i] = (hit && uint32_t(h.obj) >= P.n_spheres + P.n_elem_tris) ? int32_t(h.tri) : -1;
    if (out_dist) out_dist[i] = hit ? h.dist : nanv;
}

// The normal the scatter pass would use at the closest hit of arbitrary rays (test hook behind rbrt_hip_debug_shading_normals).
__global__ __launch_bounds__(kRaysBlock) void shading_normals_kernel(const TraceParams P, const float* __restrict__ rays, size_t n,
                                                                 float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const size_t i = size_t(blockIdx.x) * kRaysBlock + threadIdx.x;
    if (i >= n) return;
    const V3 o = mk(rays + 6 * i), d = mk(rays + 6 * i + 3);
    HitRec h;
    LocalCounters lc = {0, 0, 0, 0, 0};
    scene_hit<false>(P, o, d, stack, uint32_t(kRaysBlock), h, lc);
    const float nanv = __int_as_float(0x7fc00000);
    V3 nrm = mk(nanv, nanv, nanv);
    const uint32_t n_elem = P.n_spheres + P.n_elem_tris;
    if (h.obj >= 0 && uint32_t(h.obj) < n_elem) {
        const uint32_t desc = P.elems != nullptr ? P.elems[h.obj] : uint32_t(h.obj);
        if (desc >> 31) nrm = mk(P.elem_tris[desc & 0x7FFFFFFFu].normal);  // triangle.rs:432
        else nrm = (o + h.t * d) - mk(P.spheres[desc].center);             // sphere.rs:56, unnormalised
    } else if (h.obj >= 0) {
        nrm = mesh_shading_normal(P.meshes[uint32_t(h.obj) - n_elem].normals, h.tri, o, d);
    }
    out[3 * i + 0] = nrm.x;
    out[3 * i + 1] = nrm.y;
    out[3 * i + 2] = nrm.z;
}

// The attenuation the scatter pass would record at the closest hit of arbitrary rays (test hook behind rbrt_hip_debug_surface_albedo).
__global__ __launch_bounds__(kRaysBlock) void surface_albedo_kernel(const TraceParams P, const float* __restrict__ rays, size_t n,
                                                                float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const size_t i = size_t(blockIdx.x) * kRaysBlock + threadIdx.x;
    if (i >= n) return;
    const V3 o = mk(rays + 6 * i), d = mk(rays + 6 * i + 3);
    HitRec h;
    LocalCounters lc = {0, 0, 0, 0, 0};
    scene_hit<false>(P, o, d, stack, uint32_t(kRaysBlock), h, lc);
    const float nanv = __int_as_float(0x7fc00000);
    V3 a = mk(nanv, nanv, nanv);
    if (h.obj >= 0) {
        const uint32_t* mat = reinterpret_cast<const uint32_t*>(P.materials);
        if (int32_t(mat[uint32_t(h.obj) * 5u + 4u]) == RBRT_MAT_DIELECTRIC) {
            a = mk(1.0f, 1.0f, 1.0f);  // dielectric.rs:18
        } else {
            const uint32_t ent = surface_entry(mat, uint32_t(h.obj), surface_link(mat, uint32_t(h.obj)), o + h.t * d);
            a = mk(reinterpret_cast<const float*>(mat + ent * 5u));
        }
    }
    out[3 * i + 0] = a.x;
    out[3 * i + 1] = a.y;
    out[3 * i + 2] = a.z;
}

// The environment lookup alone, for arbitrary directions (test hook behind rbrt_hip_debug_environment).
__global__ __launch_bounds__(kRaysBlock) void environment_lookup_kernel(const EnvTexel* __restrict__ nodes, uint32_t n_env,
                                                                    const float* __restrict__ dirs, size_t n, float* __restrict__ out) {
    const size_t i = size_t(blockIdx.x) * kRaysBlock + threadIdx.x;
    if (i >= n) return;
    const V3 c = environment_radiance(nodes, n_env, mk(dirs + 3 * i));
    out[3 * i + 0] = c.x;
    out[3 * i + 1] = c.y;
    out[3 * i + 2] = c.z;
}

// Test hook (rbrt_hip_selftest_ieee): the short IEEE forms (sqrt_core inside ieee_sqrt, normalize) against the
// compiler's on pseudo-random operands. Waves 0,1,2 (mod 4) draw every lane's operands from the whole domain the gates
// admit, so the short forms are what runs: x in (2^-80, 2^100); the largest component of a in [2^-40, 2^(kNormTopExp+1))
// (so |a|^2 is inside normalize's gate), the others from just above kNormMin up to its exponent (quotients down to the
// smallest the gate lets through, exponent gaps far beyond 96). Waves 3 (mod 4) mix in zeros, denormals, huge, inf and
// NaN: the ballot sends those waves through the compiler's forms, which must then be what comes out. counts[0] =
// mismatching sqrt results, counts[1] = mismatching normalize components, counts[2] = lanes whose sqrt and normalize
// both took the short path.
constexpr int kNormTopExp = 24;
static_assert(3.0f * float(1ull << (kNormTopExp + 1)) * float(1ull << (kNormTopExp + 1)) < kNormSHi,
              "kNormTopExp: the in-range draws must stay inside normalize's gate");
__global__ __launch_bounds__(kBlock) void ieee_selftest_kernel(uint64_t seed, size_t n, unsigned long long* counts) {
    const size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    Rng rng;
    rng.init(seed, uint32_t(i >> 20), uint32_t(i));
    const uint32_t mode = uint32_t(i >> 6) & 3u;
    auto draw = [&](int e_lo, int e_hi) {  // +-(1.m) * 2^e, e uniform in [e_lo, e_hi]; never exactly +-2^e_lo
        const uint32_t r = rng.next_u32(), q = rng.next_u32();
        const int e = e_lo + int(q % uint32_t(e_hi - e_lo + 1));
        const uint32_t m = (r & 0x007FFFFFu) == 0u && e == e_lo ? 1u : (r & 0x007FFFFFu);
        return __uint_as_float((r & 0x80000000u) | m | (uint32_t(e + 127) << 23));
    };
    V3 a;
    float x;
    if (mode != 3u) {
        const uint32_t top = rng.next_u32() % 3u;
        const int e_top = -40 + int(rng.next_u32() % uint32_t(kNormTopExp + 41));
        const float big = draw(e_top, e_top);
        a = mk(top == 0u ? big : draw(-100, e_top), top == 1u ? big : draw(-100, e_top), top == 2u ? big : draw(-100, e_top));
        x = __builtin_fabsf(draw(-80, 99));
    } else {
        const uint32_t pick = rng.next_u32();
        a = mk(draw(-126, 127), draw(-126, 127), draw(-126, 127));
        x = __builtin_fabsf(draw(-126, 127));
        const float specials[8] = {0.0f, -0.0f, __uint_as_float(1u), __uint_as_float(0x007FFFFFu), __uint_as_float(0x7F7FFFFFu),
                                   __uint_as_float(0x7F800000u), __uint_as_float(0xFF800000u), __uint_as_float(0x7FC00000u)};
        if ((pick & 3u) == 0u) a.x = specials[(pick >> 2) & 7u];
        if ((pick & 12u) == 0u) a.y = specials[(pick >> 5) & 7u];
        if ((pick & 48u) == 0u) x = __builtin_fabsf(specials[(pick >> 8) & 7u]);
    }
    auto same = [](float p, float q) { return __float_as_uint(p) == __float_as_uint(q) || (p != p && q != q); };
    bool s_short, n_short;
    const float s_fast = ieee_sqrt(x, s_short), s_ref = __builtin_sqrtf(x);
    const V3 n_fast = normalize(a, n_short), n_ref = normalize_ieee(a);
    unsigned long long bad_s = same(s_fast, s_ref) ? 0ull : 1ull;
    unsigned long long bad_n = (same(n_fast.x, n_ref.x) ? 0ull : 1ull) + (same(n_fast.y, n_ref.y) ? 0ull : 1ull) + (same(n_fast.z, n_ref.z) ? 0ull : 1ull);
    if (bad_s) atomicAdd(&counts[0], bad_s);
    if (bad_n) atomicAdd(&counts[1], bad_n);
    const unsigned long long n_both = __popcll(__builtin_amdgcn_ballot_w64(s_short && n_short));
    if (threadIdx.x % 64 == 0 && n_both) atomicAdd(&counts[2], n_both);
}

// Test hook (rbrt_hip_debug_ieee): ieee_sqrt and normalize on caller-supplied operands, element i in lane i % 64 of wave
// i / 64, with whether that wave took the short path.
__global__ __launch_bounds__(kBlock) void ieee_debug_kernel(const float* __restrict__ x, size_t n, const float* __restrict__ v, size_t m,
                                                            float* out_sqrt, uint8_t* out_sqrt_short, float* out_norm, uint8_t* out_norm_short) {
    const size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) {
        bool sh;
        out_sqrt[i] = ieee_sqrt(x[i], sh);
        out_sqrt_short[i] = sh ? 1 : 0;
    }
    if (i < m) {
        bool sh;
        const V3 q = normalize(mk(v + 3 * i), sh);
        out_norm[3 * i] = q.x, out_norm[3 * i + 1] = q.y, out_norm[3 * i + 2] = q.z;
        out_norm_short[i] = sh ? 1 : 0;
    }
}

// Test hook (rbrt_hip_selftest_sqrt_sweep): ieee_sqrt of every float whose bits are in [first, first + n), each lane kSweepPerLane
// of them, a wave 64 consecutive ones at a time. counts[0] = results that are not the correctly rounded square root by an
// exact integer test (with x = mx 2^ex and r = mr 2^er, mx and mr integers: (2 mr - 1)^2 < 4 mx 2^(ex - 2 er) < (2 mr + 1)^2;
// a square root is never a midpoint), counts[1] = results that differ from the compiler's sqrt, counts[2] = lanes that
// took the short path. Positive normal x only.
constexpr uint32_t kSweepPerLane = 32;
__global__ __launch_bounds__(kBlock) void sqrt_sweep_kernel(uint32_t first, uint64_t n, unsigned long long* counts) {
    const uint64_t lane = threadIdx.x % 64u, wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / 64u;
    unsigned long long bad_exact = 0, bad_ref = 0, n_short = 0;
    for (uint32_t j = 0; j < kSweepPerLane; ++j) {
        const uint64_t k = (wave * kSweepPerLane + j) * 64u + lane;
        if (k >= n) break;
        const uint32_t xb = first + uint32_t(k);
        const float x = __uint_as_float(xb);
        bool sh;
        const float r = ieee_sqrt(x, sh);
        n_short += sh ? 1u : 0u;
        const uint32_t rb = __float_as_uint(r);
        bad_ref += rb != __float_as_uint(__builtin_sqrtf(x)) ? 1u : 0u;
        const uint64_t mx = (xb & 0x007FFFFFu) | 0x00800000u, mr = (rb & 0x007FFFFFu) | 0x00800000u;
        const int d = (int(xb >> 23) - 150) - 2 * (int(rb >> 23) - 150);  // ex - 2 er
        bool ok = (rb >> 23) - 1u < 254u && d >= 0 && d <= 30;          // a positive normal r, and the scale the bounds need
        if (ok) {
            const uint64_t x4 = (mx << 2) << d;
            ok = (2u * mr - 1u) * (2u * mr - 1u) < x4 && x4 < (2u * mr + 1u) * (2u * mr + 1u);
        }
        bad_exact += ok ? 0u : 1u;
    }
    if (bad_exact) atomicAdd(&counts[0], bad_exact);
    if (bad_ref) atomicAdd(&counts[1], bad_ref);
    if (n_short) atomicAdd(&counts[2], n_short);
}

// Test hook (rbrt_hip_selftest_gate): both forms of the mesh gate on arbitrary rays against one box.
__global__ __launch_bounds__(kBlock) void gate_selftest_kernel(const float* __restrict__ box, const float* __restrict__ rays, size_t n,
                                                               uint8_t* out_fast, uint8_t* out_exact) {
    const size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const V3 o = mk(rays + 6 * i), d = mk(rays + 6 * i + 3);
    out_fast[i] = bbox_gate_fast(box, box + 3, o, d) ? 1 : 0;
    out_exact[i] = bbox_gate(box, box + 3, o, d) ? 1 : 0;
}

// Test hook (rbrt_hip_debug_scatter): one RayScattering::scatter event per thread, through the same device functions
// the megakernel's shading passes are built from (scatter / reflect / refract / schlick / random_point_in_unit_sphere).
__global__ __launch_bounds__(kBlock) void scatter_debug_kernel(const DevMaterial* __restrict__ mats, const float* __restrict__ in_dir,
                                                                const float* __restrict__ p, const float* __restrict__ normal,
                                                                const uint32_t* __restrict__ rng_state, size_t n, float* out_dir,
                                                                uint8_t* out_ok, uint32_t* out_rng_state) {
    const size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    Rng rng = {rng_state[2 * i], rng_state[2 * i + 1]};
    V3 nd = mk(0.0f, 0.0f, 0.0f);
    // an emitter scatters nothing and draws nothing (the megakernel never shades one: classify() ends its path)
    const bool ok = mats[i].kind != kDevMatEmissive && scatter(mats[i], mk(in_dir + 3 * i), mk(p + 3 * i), mk(normal + 3 * i), rng, nd);
    if (out_dir) out_dir[3 * i] = nd.x, out_dir[3 * i + 1] = nd.y, out_dir[3 * i + 2] = nd.z;
    if (out_ok) out_ok[i] = ok ? 1 : 0;
    if (out_rng_state) out_rng_state[2 * i] = rng.s0, out_rng_state[2 * i + 1] = rng.s1;
}

// ---------------------------------------------------------------------------------------------
// Launch wrappers (called from api.cpp, which is plain C++)
// ---------------------------------------------------------------------------------------------
size_t megakernel_gseq_bytes(uint32_t n_waves) { return size_t(n_waves) * kPool * kSeqWords * sizeof(uint32_t); }
size_t megakernel_gstack_bytes(uint32_t n_waves) { return size_t(n_waves) * kStackMax * 64u * sizeof(uint32_t); }
size_t megakernel_gtime_bytes(uint32_t n_waves) { return size_t(n_waves) * kPool * sizeof(float); }  // TraceParams::gtime

__host__ __device__ inline uint32_t megakernel_lds_dwords(uint32_t stack_entries, uint32_t n_spheres, uint32_t n_meshes, uint32_t n_elem_tris,
                                                          uint32_t thin_lens, uint32_t environment, uint32_t pattern_dw, uint32_t shutter,
                                                          uint32_t motion, uint32_t mesh_motion) {
    const uint32_t n_elem = n_spheres + n_elem_tris;
    const uint32_t scene = n_spheres * kSphDw + (n_elem + n_meshes) * kMatDw + n_meshes * kMeshDw + kGenDw +
                           pattern_dw +                                                // second entries and DevPatterns (nothing without patterns)
                           (thin_lens ? kLensDw : 0u) +                                // a lens launch's lens (nothing for a pinhole)
                           (environment ? kEnvDw : 0u) +                               // the map's address and size (nothing without one)
                           (shutter ? kShutterDw : 0u) +                               // a shutter launch's travel (nothing without a shutter)
                           (motion ? n_spheres * kMotionDw + 1u : 0u) +                // a motion launch's travels and phase (nothing without a motion)
                           (mesh_motion ? n_meshes * kMeshMotionDw : 0u) +             // the meshes' travels (nothing without a mesh motion)
                           (n_elem_tris != 0u ? n_elem_tris * kTriDw + n_elem : 0u);  // triangle table + element order
    const uint32_t pool_pad = (uint32_t(kPool) + 63u) & ~63u;  // status + list: one byte per (padded) slot each
    uint32_t dw = uint32_t(kFields * kPool) + kCellDw + kTqDw + kHelpDw + pool_pad / 2u + stack_entries * 64u + scene;
    if (RBRT_REGION_TIMERS) dw += uint32_t(kNumRegions);  // analysis build: a u32 cycle accumulator per region
    return dw;
}
size_t megakernel_lds_bytes(uint32_t stack_entries, uint32_t n_spheres, uint32_t n_meshes, uint32_t n_elem_tris, uint32_t thin_lens,
                            uint32_t environment, uint32_t pattern_dw, uint32_t shutter, uint32_t motion, uint32_t mesh_motion) {
    return size_t(megakernel_lds_dwords(stack_entries, n_spheres, n_meshes, n_elem_tris, thin_lens, environment, pattern_dw, shutter, motion, mesh_motion)) * sizeof(uint32_t);
}

// What the HIP runtime says fits: resident single-wave workgroups of the trace kernel per CU at this much LDS (0 on error).
int megakernel_occupancy_per_cu(size_t lds_bytes) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_megakernel<false>, 64, lds_bytes);
    return e == hipSuccess ? n : 0;
}

// Does the launch qualify for the PLAIN build of the trace kernel (megakernel.inl TraceView)? Every constant that build has
// in place of a parameter is compared with the parameter here, and nowhere else.
bool trace_params_are_plain(const TraceParams& P) {
    return P.n_meshes == 1u && P.n_elem_tris == 0u && P.thin_lens == 0u && P.shutter == 0u && P.motion == nullptr && P.mesh_motion == nullptr && P.env_nodes == nullptr && P.pattern_dw == 0u &&
           P.y_low_water == kDefaultKnobs.y_low_water && P.y_high_water == kDefaultKnobs.y_high_water &&
           P.y_high_min_parked == kDefaultKnobs.y_high_min_parked && P.leaf_round == kDefaultKnobs.leaf_round &&
           P.leaf_leaves == kDefaultKnobs.leaf_leaves && P.share_idle == kDefaultKnobs.share_idle &&
           P.shade_rounds == kDefaultKnobs.shade_rounds && P.shade_cont_min == kDefaultKnobs.shade_cont_min;
}

// n_waves single-wave workgroups; each loops until the global work counter (zeroed by the caller on
// this stream) runs out, so any grid size is correct and no wave ever waits on another.
// A helper launch (api.cpp "Elastic launches"): more waves for a launch that is already running -- the same parameters
// (work counters, sample buffer, tables), scratch slots from P.wave_base on.
hipError_t launch_trace_helper(const TraceParams& P, uint32_t n_waves, bool plain, hipStream_t stream) {
    if (P.n_items == 0 || n_waves == 0 || !P.helper_words) return hipSuccess;
    const size_t lds = megakernel_lds_bytes(P.stack_entries, P.n_spheres, P.n_meshes, P.n_elem_tris, P.thin_lens, P.env_nodes ? 1u : 0u, P.pattern_dw, P.shutter, P.motion ? 1u : 0u, P.mesh_motion ? 1u : 0u);
    if (P.mesh_motion)  // (a launch with a mesh motion is never plain: trace_params_are_plain)
        hipLaunchKernelGGL((trace_megakernel<false, true, false, true>), dim3(n_waves), dim3(64), lds, stream, P);
    else if (plain && trace_params_are_plain(P))
        hipLaunchKernelGGL((trace_megakernel<false, true, true>), dim3(n_waves), dim3(64), lds, stream, P);
    else
        hipLaunchKernelGGL((trace_megakernel<false, true, false>), dim3(n_waves), dim3(64), lds, stream, P);
    return hipGetLastError();
}

// `plain`: the caller allows the PLAIN build (megakernel.inl TraceView); it runs only if the parameters are what it has built
// in, whatever the caller says, and never for a counting launch.
hipError_t launch_trace_megakernel(const TraceParams& P, uint32_t n_waves, bool stats, bool plain, hipStream_t stream) {
    if (P.n_items == 0 || n_waves == 0) return hipSuccess;
    const size_t lds = megakernel_lds_bytes(P.stack_entries, P.n_spheres, P.n_meshes, P.n_elem_tris, P.thin_lens, P.env_nodes ? 1u : 0u, P.pattern_dw, P.shutter, P.motion ? 1u : 0u, P.mesh_motion ? 1u : 0u);
    if (P.mesh_motion && !P.motion) return hipErrorInvalidValue;  // (fill_trace_params gives such a launch the zero travels)
    if (stats && P.mesh_motion)
        hipLaunchKernelGGL((trace_megakernel<true, false, false, true>), dim3(n_waves), dim3(64), lds, stream, P);
    else if (P.mesh_motion)
        hipLaunchKernelGGL((trace_megakernel<false, false, false, true>), dim3(n_waves), dim3(64), lds, stream, P);
    else if (stats)
        hipLaunchKernelGGL((trace_megakernel<true, false, false>), dim3(n_waves), dim3(64), lds, stream, P);
    else if (plain && trace_params_are_plain(P))
        hipLaunchKernelGGL((trace_megakernel<false, false, true>), dim3(n_waves), dim3(64), lds, stream, P);
    else
        hipLaunchKernelGGL((trace_megakernel<false, false, false>), dim3(n_waves), dim3(64), lds, stream, P);
    return hipGetLastError();
}

// The tile pass: the culling table of P.cam, then (tile_lists given) the rank's two tile lists from it.
hipError_t launch_primary_cull(const TraceParams& P, hipStream_t stream) {
    if (P.n_tiles == 0 || !P.tile_cull) return hipSuccess;
    const uint32_t cull_tiles = P.tile_world > 1u ? local_tiles_of(P.n_tiles, P.tile_rank, P.tile_world) : P.n_tiles;
    if (cull_tiles == 0u) return hipSuccess;
    const size_t cull_threads = size_t(cull_tiles) * kCullLanes;
    if (P.mesh_motion) hipLaunchKernelGGL(primary_cull_kernel<true>, dim3(uint32_t((cull_threads + kCullBlock - 1) / kCullBlock)), dim3(kCullBlock), 0, stream, P);
    else hipLaunchKernelGGL(primary_cull_kernel<false>, dim3(uint32_t((cull_threads + kCullBlock - 1) / kCullBlock)), dim3(kCullBlock), 0, stream, P);
    if (P.tile_lists) {
        if (P.tile_lists_wide) hipLaunchKernelGGL(tile_lists_kernel<256>, dim3(1), dim3(256), 0, stream, P);
        else hipLaunchKernelGGL(tile_lists_kernel<64>, dim3(1), dim3(64), 0, stream, P);
    }
    return hipGetLastError();
}

// One empty launch: the HIP runtime loads a library's device code at the first launch of one of its kernels (7-8 ms for this
// one). rbrt_hip_scene_create does it, so that the first render of a process is a render.
__global__ void code_load_kernel() {}
hipError_t launch_code_load(hipStream_t stream) {
    hipLaunchKernelGGL(code_load_kernel, dim3(1), dim3(64), 0, stream);
    return hipGetLastError();
}

hipError_t launch_sky_resolve(const TraceParams& P, const ResolveParams& R, hipStream_t stream) {
    const size_t npix = size_t(R.n_local_tiles) * 64u;  // (an upper bound: the list's length is known on the device)
    if (npix == 0 || !R.tile_lists) return hipSuccess;
    hipLaunchKernelGGL(sky_resolve_kernel, dim3(uint32_t((npix + kSmallBlock - 1) / kSmallBlock)), dim3(kSmallBlock), 0, stream, P, R);
    return hipGetLastError();
}

hipError_t launch_resolve(const ResolveParams& R, hipStream_t stream) {
    const size_t npix = size_t(R.n_local_tiles) * 64u;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(resolve_kernel, dim3(uint32_t((npix + kSmallBlock - 1) / kSmallBlock)), dim3(kSmallBlock), 0, stream, R);
    return hipGetLastError();
}

// The kernels of an adaptive round. n_active_tiles: the host's count of the tiles on the round's two lists together
// (either list is at most that long: the grids are sized by it, not by the image).
hipError_t launch_resolve_even(const TraceParams& P, const ResolveParams& R, uint32_t n_active_tiles, hipStream_t stream) {
    const size_t npix = size_t(n_active_tiles) * 64u;
    if (npix == 0 || !R.tile_lists || !R.acc || !R.acc_even) return hipSuccess;
    const dim3 grid(uint32_t((npix + kSmallBlock - 1) / kSmallBlock));
    hipLaunchKernelGGL(resolve_even_kernel, grid, dim3(kSmallBlock), 0, stream, R);
    hipLaunchKernelGGL(sky_resolve_even_kernel, grid, dim3(kSmallBlock), 0, stream, P, R);
    return hipGetLastError();
}
hipError_t launch_adaptive_lists(const AdaptiveParams& A, hipStream_t stream) {
    if (A.n_local_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_lists_kernel, dim3(1), dim3(64), 0, stream, A);
    return hipGetLastError();
}
hipError_t launch_tile_error(const AdaptiveParams& A, uint32_t n_active_tiles, hipStream_t stream) {
    if (n_active_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(tile_error_kernel, dim3(n_active_tiles), dim3(64), 0, stream, A);
    return hipGetLastError();
}
hipError_t launch_adaptive_finish(const AdaptiveParams& A, hipStream_t stream) {
    const size_t npix = size_t(A.n_local_tiles) * 64u;
    if (npix == 0 || (!A.out_radiance && !A.out_rgb8)) return hipSuccess;
    hipLaunchKernelGGL(adaptive_finish_kernel, dim3(uint32_t((npix + kSmallBlock - 1) / kSmallBlock)), dim3(kSmallBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_unpack(const float* gathered, uint32_t width, uint32_t height, uint32_t world,
                         size_t rank_stride_pixels, float* out_radiance, uint8_t* out_rgb8, hipStream_t stream) {
    const uint32_t tiles_x = (width + RBRT_TILE - 1) / RBRT_TILE, tiles_y = (height + RBRT_TILE - 1) / RBRT_TILE;
    const size_t n = size_t(width) * height;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(unpack_kernel, dim3(uint32_t((n + kSmallBlock - 1) / kSmallBlock)), dim3(kSmallBlock), 0, stream, gathered,
                       width, height, tiles_x, tiles_x * tiles_y, world, rank_stride_pixels, out_radiance, out_rgb8);
    return hipGetLastError();
}

hipError_t launch_trace_rays(const TraceParams& P, const float* rays, size_t n, float* out_t, int32_t* out_obj,
                             int32_t* out_tri, float* out_dist, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(trace_rays_kernel, dim3(uint32_t((n + kRaysBlock - 1) / kRaysBlock)), dim3(kRaysBlock),
                       size_t(kStackMax) * kRaysBlock * sizeof(uint32_t), stream, P, rays, n, out_t, out_obj,
                       out_tri, out_dist);
    return hipGetLastError();
}

hipError_t launch_shading_normals(const TraceParams& P, const float* rays, size_t n, float* out_normal, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(shading_normals_kernel, dim3(uint32_t((n + kRaysBlock - 1) / kRaysBlock)), dim3(kRaysBlock),
                       size_t(kStackMax) * kRaysBlock * sizeof(uint32_t), stream, P, rays, n, out_normal);
    return hipGetLastError();
}

hipError_t launch_surface_albedo(const TraceParams& P, const float* rays, size_t n, float* out_albedo, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(surface_albedo_kernel, dim3(uint32_t((n + kRaysBlock - 1) / kRaysBlock)), dim3(kRaysBlock),
                       size_t(kStackMax) * kRaysBlock * sizeof(uint32_t), stream, P, rays, n, out_albedo);
    return hipGetLastError();
}

#include "features.inl"
#include "short_paths.inl"

hipError_t launch_environment_lookup(const EnvTexel* nodes, uint32_t n_env, const float* dirs, size_t n, float* out_rgb, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(environment_lookup_kernel, dim3(uint32_t((n + kRaysBlock - 1) / kRaysBlock)), dim3(kRaysBlock), 0, stream, nodes,
                       n_env, dirs, n, out_rgb);
    return hipGetLastError();
}

hipError_t launch_gate_selftest(const float* d_box, const float* d_rays, size_t n, uint8_t* d_fast, uint8_t* d_exact) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gate_selftest_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, d_box, d_rays, n,
                       d_fast, d_exact);
    return hipGetLastError();
}

hipError_t launch_ieee_selftest(uint64_t seed, size_t n, unsigned long long* d_counts) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ieee_selftest_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, seed, n, d_counts);
    return hipGetLastError();
}
hipError_t launch_ieee_debug(const float* d_x, size_t n, const float* d_v, size_t m, float* d_sqrt, uint8_t* d_sqrt_short,
                             float* d_norm, uint8_t* d_norm_short) {
    const size_t k = n > m ? n : m;
    if (k == 0) return hipSuccess;
    hipLaunchKernelGGL(ieee_debug_kernel, dim3(uint32_t((k + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, d_x, n, d_v, m, d_sqrt,
                       d_sqrt_short, d_norm, d_norm_short);
    return hipGetLastError();
}
hipError_t launch_sqrt_sweep(uint32_t first, uint64_t n, unsigned long long* d_counts) {
    if (n == 0) return hipSuccess;
    const uint64_t per_block = uint64_t(kBlock) * kSweepPerLane;
    hipLaunchKernelGGL(sqrt_sweep_kernel, dim3(uint32_t((n + per_block - 1) / per_block)), dim3(kBlock), 0, nullptr, first, n, d_counts);
    return hipGetLastError();
}
hipError_t launch_scatter_debug(const DevMaterial* d_mats, const float* d_in_dir, const float* d_p, const float* d_normal,
                                 const uint32_t* d_rng, size_t n, float* d_out_dir, uint8_t* d_out_ok, uint32_t* d_out_rng) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_debug_kernel, dim3(uint32_t((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, d_mats, d_in_dir, d_p,
                       d_normal, d_rng, n, d_out_dir, d_out_ok, d_out_rng);
    return hipGetLastError();
}

uint64_t host_splitmix64(uint64_t x) { return splitmix64(x); }

}  // namespace rbrt
