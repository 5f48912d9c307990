// short_paths.inl — the short-path stage (DESIGN.md section 6 "The tile pass"). Included by kernels.hip behind
// megakernel.inl, whose device functions and work-item numbering it shares.
//
// A tile none of whose camera rays can pass a mesh box (the mesh bits 24 + m of its culling word are all set) and that
// is not background-only sees spheres: in the headline scene the ground outside the objects' silhouettes and the small
// spheres. Most of its samples are paths of two rays: the camera ray hits a sphere, scatters once, and the second ray
// hits nothing and passes no mesh gate. The trace kernel pays for such a sample a generation, two rounds of all sphere
// tests plus the gate plus parking, a scatter pass through the LDS pool and a TERM pass, at ~0.6 lane utilisation. This
// kernel runs in front of the trace launch and finishes those samples in straight-line code at full lanes: a wave works in
// CHUNKS of 64 work items (one tile's 64 pixels of one sample: the trace kernel's chunk, same numbering), lane p = pixel p.
//
// A sample is either FINISHED here -- the same three floats into the same sample_buf slot the trace kernel would have
// written -- or left to the trace kernel ENTIRELY: nothing is handed over but one bit. The wave stores the chunk's finished
// mask (a ballot) into TraceParams::short_masks[chunk]; the trace kernel's generation step hands out only the items whose
// bit is clear (megakernel.inl, WorkSource). Chunks of other tiles get a zero mask and are the trace kernel's as before.
// Every arithmetic step is the trace kernel's own device function on the same operands, so the finished samples carry the
// bits the trace kernel would have produced; which kernel finishes a sample never shows in the image.
//
// Finished here:  camera ray misses everything                                   -> background / environment
//                 camera ray hits an emitter, or max_depth is 0                  -> its radiance / black
//                 a metal scatter that fails (metal.rs:25)                       -> black
//                 second ray hits nothing and passes no mesh gate                -> attenuation * background
//                 second ray passes no gate and ends by classify() (depth 0, an emitter)
// Left alone:     second ray passes a mesh gate, or hits something it has to scatter from.
// A pixel slot beyond a ragged image edge counts as finished: the trace kernel would generate nothing for it either.
//
// The camera ray is tested against the elements whose culling bit is CLEAR only (a set bit proves the test fails) and
// against no mesh gate (the mesh bits prove it fails); BasicTriangle elements are never culled. The second ray gets the
// trace kernel's full treatment: every element in order with the strict `<`, then next_gated_mesh from mesh 0.

//
// Tiles that do not pay. A chunk costs the stage about the same whatever comes of it (some 1,000 VALU instructions a wave on
// the headline scene), and the trace kernel saves about 1,560 for a chunk finished whole: a tile where fewer than two thirds
// of the samples finish is cheaper left alone -- next to a large mesh most second rays pass its box, under an overhang they
// hit again. So a wave takes one TILE and its samples in turn, and after the tile's first kShortProbe samples it goes on
// only if at least kShortKeepNum / kShortKeepDen of their 64-sample slots finished; else the tile's remaining chunks get a
// zero mask. (The rule decides who does the work, never what comes out.)

constexpr int kShortBlock = 64;
constexpr uint32_t kShortProbe = 2;                        // samples of a tile the stage always does
constexpr uint32_t kShortKeepNum = 3, kShortKeepDen = 4;  // ... and the share of them that must finish for the rest

// The closest element hit of a ray (scene.rs:23-31): elements in their order, strict `<`. `skip`: culling bits of the
// elements (bit e < 24) whose test is known to fail -- 0 for any ray but a camera ray of the word's tile.
// mt: the sample's draw t; with a motion (P.motion) a sphere is tested where it is then (sphere_centre_at), and the skip bits are
// the tile pass's widened ones, which hold for every t.
__device__ __forceinline__ void short_closest_element(const TraceParams& P, const SceneLds& sc, uint32_t n_elem, uint32_t skip, V3 o, V3 d,
                                                      float mt, float& closest, float& ht, int32_t& obj) {
    closest = 3.40282347e+38f;  // f32::MAX (scene.rs:21)
    ht = 0.0f;
    obj = -1;
    for (uint32_t e = 0; e < n_elem; ++e) {
        const uint32_t desc = P.n_elem_tris != 0u ? sc.elem[e] : e;  // (wave-uniform)
        float t, dist;
        bool hit;
        if (desc >> 31) {
            hit = basic_triangle_hit(sc.tri + (desc & 0x7FFFFFFFu) * kTriDw, o, d, P.min_dist, P.max_dist, t, dist);
        } else {
            if (e < 24u && ((skip >> e) & 1u)) continue;
            const float* sp = sc.sph + desc * kSphDw;
            const V3 c = P.motion ? sphere_centre_at(sp, P.motion + desc * kMotionDw, mt) : mk(sp);
            hit = sphere_hit(c, sp[3], o, d, P.min_dist, P.max_dist, t, dist, P.counters);
        }
        if (hit && dist < closest) {
            closest = dist;
            ht = t;
            obj = int32_t(e);
        }
    }
}

// What a path that ends on `obj` (-1: nothing) with direction d sees before its attenuation: the TERM pass's rule.
__device__ __forceinline__ V3 short_end_colour(const TraceParams& P, const SceneLds& sc, int32_t obj, V3 d) {
    if (obj < 0) return P.env_nodes ? environment_radiance(P.env_nodes, P.env_n, d) : background(d.y, P.bg, P.constant_bg);  // lib.rs:68-71
    if (int32_t(sc.mat[uint32_t(obj) * kMatDw + 4]) == kDevMatEmissive) return mk(reinterpret_cast<const float*>(sc.mat + uint32_t(obj) * kMatDw));
    return mk(0.0f, 0.0f, 0.0f);  // a hit with depth 0: lib.rs:63-66
}

// One sample of a tile of the stage, pixel (row, col) inside the image: true if it is finished here (its colour stored at
// sample_buf[item]), false if it is the trace kernel's. `word`: the tile's culling word; s: the sample within the launch.
template <bool MM>
__device__ __forceinline__ bool short_path_sample(const TraceParams& P, const SceneLds& sc, const float* lens, uint32_t n_elem, uint32_t word,
                                                  uint32_t row, uint32_t col, uint32_t s, uint32_t item) {
    const uint32_t img_w = P.cam.img_width_pix, img_h = P.cam.img_height_pix;
    bool finished = true;
    Rng rng;
    rng.init(P.seed_key, row * img_w + col, P.sample_base + s);
    V3 o = mk(P.cam.position);
    V3 f = camera_target(mk(P.cam.img_center_point), mk(P.cam.right), mk(P.cam.up), P.cam.mm_per_pix_hor, P.cam.mm_per_pix_vert, img_w,
                         img_h, row, col, rng);
    if (P.thin_lens) lens_point(o, f, lens, rng);
    V3 d = normalize(f - o);
    float mt = 0.0f;  // one draw for the shutter and the motion; with a motion it stays the sample's for both rays
    if (P.shutter || P.motion) mt = rng.next_f32();
    if (P.shutter) shutter_origin(o, P.travel, mt);
    if (P.motion) mt = P.motion_phase + mt;  // "Animation": s = phase + t, the spheres' time; the shutter kept the raw t
    uint32_t depth = P.max_depth;
    float closest, ht;
    int32_t obj;
    short_closest_element(P, sc, n_elem, word, o, d, mt, closest, ht, obj);
    uint32_t next = classify(sc, obj, depth);
    V3 color = mk(0.0f, 0.0f, 0.0f);
    int32_t rec = -1;  // the bounce whose albedo attenuates the path (a dielectric's (1,1,1) is not recorded)
    if (next != ST_TERM) {
        const V3 p = o + ht * d;  // same expression as inside the intersection routines
        const uint32_t desc = P.n_elem_tris != 0u ? sc.elem[uint32_t(obj)] : uint32_t(obj);
        V3 n;
        if (desc >> 31) n = mk(sc.tri + (desc & 0x7FFFFFFFu) * kTriDw + 9);  // triangle.rs:432: the stored normal
        else n = p - (P.motion ? sphere_centre_at(sc.sph + desc * kSphDw, P.motion + desc * kMotionDw, mt) : mk(sc.sph + desc * kSphDw));  // sphere.rs:56, unnormalised
        const float param = __uint_as_float(sc.mat[uint32_t(obj) * kMatDw + 3]);
        V3 nd;
        bool ok;
        if (next == ST_LAMB) {  // lambertian.rs:11-24
            const V3 target = (p + normalize(n)) + random_point_in_unit_sphere(rng);
            nd = normalize(target - p);
            ok = true;
        } else if (next == ST_METAL) {  // metal.rs:12-25
            const V3 target = reflect(d, n);
            nd = normalize(target + param * random_point_in_unit_sphere(rng));
            ok = dot(nd, n) > 0.0f;
        } else {  // dielectric.rs:11-59
            scatter_dielectric(param, d, n, rng, nd);
            ok = true;
        }
        if (ok) {
            if (next != ST_DIEL)  // (the entry the trace kernel's scatter would record: a patterned lambertian's cell)
                rec = next == ST_LAMB ? int32_t(surface_entry(sc.mat, uint32_t(obj), __float_as_uint(param), p)) : obj;
            o = p;
            d = nd;
            depth -= 1u;
            short_closest_element(P, sc, n_elem, 0u, o, d, mt, closest, ht, obj);
            LocalCounters lc = {0, 0, 0, 0, 0};
            // (with a mesh motion the gate of mesh m reads o_m at the sample's time: "Moving meshes"; the camera ray went on
            // trusting the tile pass's mesh bits, which hold for every time of the exposure)
            const uint32_t gated = MM ? next_gated_mesh_moving<false>(sc, P.n_meshes, 0u, o, d, closest, lc, P.mesh_motion, mt)
                                                 : next_gated_mesh<false>(sc, P.n_meshes, 0u, o, d, closest, lc);
            next = gated < P.n_meshes ? uint32_t(ST_TRAV) : classify(sc, obj, depth);
            if (next == ST_TERM) color = short_end_colour(P, sc, obj, d);
            else finished = false;
        }  // (else metal.rs:25 returned false: the path is black, lib.rs:63-66, and nothing was recorded)
    } else {
        color = short_end_colour(P, sc, obj, d);
    }
    if (finished) {
        if (rec >= 0) color = mk(reinterpret_cast<const float*>(sc.mat + uint32_t(rec) * kMatDw)) * color;  // lib.rs:62
        float* out = P.sample_buf + size_t(item) * 3u;
        out[0] = color.x;
        out[1] = color.y;
        out[2] = color.z;
    }
    return finished;
}

// (MM: the build for a launch with a mesh motion; every other launch runs the code it always has)
template <bool MM>
__global__ __launch_bounds__(kShortBlock) void short_paths_kernel(const TraceParams P) {
    const uint32_t lane = threadIdx.x;
    const uint32_t n_work = uint32_t(__builtin_amdgcn_readfirstlane(int(P.tile_lists[0])));
    const uint32_t npix = n_work * 64u;
    const uint32_t n_elem = P.n_spheres + P.n_elem_tris;
    const uint32_t mesh_bits = (1u << P.n_meshes) - 1u;  // (n_meshes <= 7: api.cpp)
    // (the scene's arrays where they are: the tables are a few cache lines, read through the scalar cache)
    const SceneLds sc = {reinterpret_cast<const float*>(P.spheres), reinterpret_cast<const uint32_t*>(P.materials),
                         reinterpret_cast<const uint32_t*>(P.meshes), reinterpret_cast<const float*>(P.elem_tris), P.elems};
    const uint32_t img_w = P.cam.img_width_pix, img_h = P.cam.img_height_pix;
    const float lens[7] = {P.lens_u[0], P.lens_u[1], P.lens_u[2], P.lens_v[0], P.lens_v[1], P.lens_v[2], P.focus_scale};
    for (uint32_t tpos = blockIdx.x; tpos < n_work; tpos += gridDim.x) {
        // chunk tpos * batch + s = (position in the work list, sample of the batch): the trace kernel's generation step
        unsigned long long* const masks = P.short_masks + size_t(tpos) * P.batch;  // (chunks < 2^26: work items are 32-bit)
        const uint32_t widx = P.tiles_reversed ? n_work - 1u - tpos : tpos;
        const uint32_t tile_local = P.tile_lists[kTileListHeader + widx];
        const uint32_t tile = tile_local * P.tile_world + P.tile_rank;
        const uint32_t word = uint32_t(__builtin_amdgcn_readfirstlane(int(P.tile_cull[tile])));
        if (((word >> 24) & mesh_bits) != mesh_bits || (word >> 31) != 0u) {  // not this stage's tile
            for (uint32_t k = lane; k < P.batch; k += 64u) masks[k] = 0ull;
            continue;
        }
        const uint32_t ty = div_magic(tile, P.tiles_x, P.tiles_x_magic);
        uint32_t tx = tile - ty * P.tiles_x + RBRT_TILE_SKEW * ty;  // (rbrt_hip.h "How tiles are dealt to ranks")
        tx -= div_magic(tx, P.tiles_x, P.tiles_x_magic) * P.tiles_x;
        const uint32_t row = ty * RBRT_TILE + (lane >> 3), col = tx * RBRT_TILE + (lane & 7u);
        uint32_t probe_finished = 0;
        for (uint32_t s = 0; s < P.batch; ++s) {
            // the tile's first kShortProbe samples decide whether the stage goes on with it (header: "Tiles that do not pay")
            if (s == kShortProbe && probe_finished * kShortKeepDen < kShortProbe * 64u * kShortKeepNum) {
                for (uint32_t k = s + lane; k < P.batch; k += 64u) masks[k] = 0ull;
                break;
            }
            // (a slot beyond a ragged edge: nothing to write, nothing to hand out)
            const bool finished = !(row < img_h && col < img_w) || short_path_sample<MM>(P, sc, lens, n_elem, word, row, col, s, s * npix + widx * 64u + lane);
            const uint64_t mask = __builtin_amdgcn_ballot_w64(finished);
            if (s < kShortProbe) probe_finished += uint32_t(__popcll(mask));
            if (lane == 0) masks[s] = mask;
        }
    }
}

// `n_waves` single-wave workgroups that stride over the tiles of the launch's work list (their number is known on the device
// only: it depends on how many tiles the tile pass left). P.batch, P.sample_base, P.sample_buf, the tile tables and
// P.short_masks are those of the trace launch that follows on the same stream.
hipError_t launch_short_paths(const TraceParams& P, uint32_t n_waves, hipStream_t stream) {
    if (P.n_items == 0 || n_waves == 0 || !P.short_masks || !P.tile_cull || !P.tile_lists) return hipSuccess;
    if (P.mesh_motion) hipLaunchKernelGGL(short_paths_kernel<true>, dim3(n_waves), dim3(kShortBlock), 0, stream, P);
    else hipLaunchKernelGGL(short_paths_kernel<false>, dim3(n_waves), dim3(kShortBlock), 0, stream, P);
    return hipGetLastError();
}
