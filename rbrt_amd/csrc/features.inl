// features.inl — the feature buffers of the primary rays (include/rbrt_hip.h "Feature buffers"). Included by kernels.hip,
// whose device functions it shares: the render's own streams and cameras (Rng, camera_target, lens_point), Scene::hit
// (scene_hit) and the normal the scatter pass would use (mesh_shading_normal).
//
// One wave per 8x8 tile, lane p = (y % 8) * 8 + (x % 8): the primary rays of a tile are coherent, so the lanes of a wave walk
// the same part of a tree. Each lane loops over its own n samples, which keeps the sums in sample order without atomics. The
// traversal stack is per lane in dynamic LDS with stride 64, FeatureParams::stack_entries deep -- what the handle's deepest
// tree can need, not kStackMax, so a CU holds as many waves as it has slots for. A lane beyond a ragged edge leaves at once:
// nothing below exchanges data between lanes (the wave votes inside ieee_sqrt, normalize and lens_point only choose between
// forms that give the same bits, and see the active lanes only).
//
// Two builds: features_kernel<false> is what rbrt_hip_render_features has always launched; features_kernel<true> also sums
// the travel of the sphere each sample hits (rbrt_hip_render_features_motion with d_motion; include/rbrt_hip.h "Animation").
// Each exists a second time for a handle with a mesh motion (MM; "Moving meshes"): the mesh loop of scene_hit and the shading
// normal read the per-mesh origin, and a mesh hit adds the mesh's travel. A handle without one launches the builds it always has.

constexpr int kFeatureBlock = 64;

template <bool MOTION, bool MM = false>
__global__ __launch_bounds__(kFeatureBlock) void features_kernel(const TraceParams P, const FeatureParams F) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* stack = lds + threadIdx.x;
    const uint32_t width = P.cam.img_width_pix, height = P.cam.img_height_pix;
    const uint32_t ty = blockIdx.x / P.tiles_x, tx = blockIdx.x - ty * P.tiles_x;
    const uint32_t p = threadIdx.x;
    const uint32_t row = ty * RBRT_TILE + (p >> 3), col = tx * RBRT_TILE + (p & 7u);
    if (row >= height || col >= width) return;
    const V3 pos = mk(P.cam.position), center = mk(P.cam.img_center_point), right = mk(P.cam.right), up = mk(P.cam.up);
    const uint32_t n_elem = P.n_spheres + P.n_elem_tris;
    V3 a = mk(0.0f, 0.0f, 0.0f), nsum = mk(0.0f, 0.0f, 0.0f);
    float z = 0.0f, c = 0.0f;
    V3 mv = mk(0.0f, 0.0f, 0.0f);  // (MOTION only)
    int32_t first_obj = -1;
    for (uint32_t s = 0; s < F.samples; ++s) {
        Rng rng;
        rng.init(P.seed_key, row * width + col, s);
        V3 o = pos, f = camera_target(center, right, up, P.cam.mm_per_pix_hor, P.cam.mm_per_pix_vert, width, height, row, col, rng);
        if (P.thin_lens) {
            const float lens[7] = {P.lens_u[0], P.lens_u[1], P.lens_u[2], P.lens_v[0], P.lens_v[1], P.lens_v[2], P.focus_scale};
            lens_point(o, f, lens, rng);
        }
        const V3 d = normalize(f - o);
        // (the render's own camera rays: the handle's shutter moves them too, and its motion the spheres they see -- one draw)
        float mt = 0.0f;
        if (P.shutter || P.motion) mt = rng.next_f32();
        if (P.shutter) shutter_origin(o, P.travel, mt);
        if (P.motion) mt = P.motion_phase + mt;  // "Animation": s = phase + t, the spheres' time; the shutter kept the raw t
        HitRec h;
        LocalCounters lc = {0, 0, 0, 0, 0};
        scene_hit<false, MM>(P, o, d, stack, uint32_t(kFeatureBlock), h, lc, P.motion, mt, P.mesh_motion);
        if (s == 0) first_obj = h.obj;
        V3 sa = mk(0.0f, 0.0f, 0.0f), sn = mk(0.0f, 0.0f, 0.0f);  // a miss: every channel adds +0
        float sz = 0.0f, sc = 0.0f;
        V3 sm = mk(0.0f, 0.0f, 0.0f);  // ... and a mesh, a BasicTriangle and anything on a handle without a motion
        if (h.obj >= 0) {
            const DevMaterial m = P.materials[h.obj];
            sa = m.kind == RBRT_MAT_DIELECTRIC ? mk(1.0f, 1.0f, 1.0f) : mk(m.albedo);  // dielectric.rs:18: its attenuation
            if (m.kind == RBRT_MAT_LAMBERTIAN && __float_as_uint(m.param) != 0u) {  // a patterned object: the cell's colour
                const uint32_t* mat = reinterpret_cast<const uint32_t*>(P.materials);
                sa = mk(P.materials[surface_entry(mat, uint32_t(h.obj), __float_as_uint(m.param), o + h.t * d)].albedo);
            }
            V3 g;
            if (uint32_t(h.obj) < n_elem) {
                const uint32_t desc = P.elems != nullptr ? P.elems[h.obj] : uint32_t(h.obj);
                if (desc >> 31) g = mk(P.elem_tris[desc & 0x7FFFFFFFu].normal);  // triangle.rs:432
                else {
                    g = (o + h.t * d) - (P.motion ? sphere_centre_at(P.spheres[desc].center, P.motion + desc * kMotionDw, mt)
                                                  : mk(P.spheres[desc].center));  // sphere.rs:56
                    if (MOTION && P.motion) sm = mk(P.motion + desc * kMotionDw);
                }
            } else {
                const uint32_t hm = uint32_t(h.obj) - n_elem;
                g = mesh_shading_normal(P.meshes[hm].normals, h.tri, MM ? mesh_origin_at(o, P.mesh_motion + hm * kMeshMotionDw, mt) : o, d);
                if (MOTION && MM) sm = mk(P.mesh_motion + hm * kMeshMotionDw);
            }
            sn = normalize(g);  // not flipped towards the ray, no guard
            sz = h.dist;
            sc = 1.0f;
        }
        a = a + sa;
        nsum = nsum + sn;
        z = z + sz;
        c = c + sc;
        if (MOTION) mv = mv + sm;
    }
    const size_t i = size_t(row) * width + col;
    if (F.albedo) {
        F.albedo[i * 3 + 0] = a.x * F.inv_n;
        F.albedo[i * 3 + 1] = a.y * F.inv_n;
        F.albedo[i * 3 + 2] = a.z * F.inv_n;
    }
    if (F.normal) {
        F.normal[i * 3 + 0] = nsum.x * F.inv_n;
        F.normal[i * 3 + 1] = nsum.y * F.inv_n;
        F.normal[i * 3 + 2] = nsum.z * F.inv_n;
    }
    if (F.depth) F.depth[i] = z * F.inv_n;
    if (F.coverage) F.coverage[i] = c * F.inv_n;
    if (F.object) F.object[i] = first_obj;
    if (MOTION) {
        F.motion[i * 3 + 0] = mv.x * F.inv_n;
        F.motion[i * 3 + 1] = mv.y * F.inv_n;
        F.motion[i * 3 + 2] = mv.z * F.inv_n;
    }
}

// One single-wave workgroup per tile of the image, row-major; F.stack_entries * 64 words of LDS each.
hipError_t launch_features(const TraceParams& P, const FeatureParams& F, hipStream_t stream) {
    if (P.n_tiles == 0) return hipSuccess;
    const size_t lds = size_t(F.stack_entries) * kFeatureBlock * sizeof(uint32_t);  // (a multiple of 256 bytes: the base stays 16-byte aligned)
    if (P.mesh_motion && F.motion) hipLaunchKernelGGL((features_kernel<true, true>), dim3(P.n_tiles), dim3(kFeatureBlock), lds, stream, P, F);
    else if (P.mesh_motion) hipLaunchKernelGGL((features_kernel<false, true>), dim3(P.n_tiles), dim3(kFeatureBlock), lds, stream, P, F);
    else if (F.motion) hipLaunchKernelGGL(features_kernel<true>, dim3(P.n_tiles), dim3(kFeatureBlock), lds, stream, P, F);
    else hipLaunchKernelGGL(features_kernel<false>, dim3(P.n_tiles), dim3(kFeatureBlock), lds, stream, P, F);
    return hipGetLastError();
}
