// device_types.h — HBM-resident data layout shared by the host-side builder and the gfx950 kernels.
#pragma once
#include <stdint.h>

#include "../../include/rbrt_hip.h"
#include "trace_knobs.h"

namespace rbrt {

// Compile-time limits.
// Tile number -> tile coordinates and back (rbrt_hip.h "How tiles are dealt to ranks": row ty is rotated by RBRT_TILE_SKEW * ty).
#if defined(__HIPCC__)
#define RBRT_HOST_DEVICE __host__ __device__
#else
#define RBRT_HOST_DEVICE  // (bvh.cpp alone under a host compiler: tests/cpp)
#endif
RBRT_HOST_DEVICE inline void tile_xy(uint32_t tile, uint32_t tiles_x, uint32_t& ty, uint32_t& tx) {
    ty = tile / tiles_x;
    tx = uint32_t((uint64_t(tile - ty * tiles_x) + uint64_t(RBRT_TILE_SKEW) * ty) % tiles_x);
}
RBRT_HOST_DEVICE inline uint32_t tile_number(uint32_t ty, uint32_t tx, uint32_t tiles_x) {
    const uint32_t rot = uint32_t((uint64_t(RBRT_TILE_SKEW) * ty) % tiles_x);
    return ty * tiles_x + (tx + tiles_x - rot) % tiles_x;
}
constexpr uint32_t kTileListHeader = 4;  // words ahead of the lists in TraceParams::tile_lists
constexpr int kBlock = 256;          // threads per workgroup of the test hooks' kernels
// Threads per workgroup of the short kernels that run BESIDE resident trace launches (resolve, sky_resolve, unpack, the tile
// pass): ONE wave. The persistent trace waves hold every wave slot and all of every CU's LDS until they exit, one by one; a
// 256-thread workgroup needs FOUR free slots on one CU at once, and a kernel on a higher-priority stream whose workgroups do
// not fit makes the dispatcher keep what frees up for it instead of handing it to the next trace launch's waves. Round 4's
// kernel trace (profiles/r04_trace_frames.txt): the resolve -- 50 us of work -- took 3.0-3.4 ms in EVERY frame of a stream,
// its lane waiting for it all the while. A one-wave workgroup runs in any slot a trace wave leaves.
constexpr int kSmallBlock = 64;
constexpr int kMaxBvhDepth = 20;     // deepest 4-wide node (root = 0) the builder may create
constexpr int kStackMax = 3 * (kMaxBvhDepth + 1) + 1;  // a visit defers at most 3 children per level
constexpr int kMaxPathDepth = 64;    // opts.max_depth limit (reference: 50, lib.rs:99)
constexpr int kMaxObjects = 255;     // spheres + meshes (object id is stored in one byte per bounce)
constexpr int kLeafBits = 2;              // width of the count field of a leaf link
constexpr int kLeafMax = 1 << kLeafBits;   // triangles per leaf
constexpr int kPool = 128;           // path slots per wave of the persistent megakernel (other sizes lost)
constexpr uint32_t kWorkShards = 8;         // work-item counters (one per XCD)
constexpr uint32_t kWorkCounterStride = 16;  // in u64: each counter on its own 128-B line
constexpr uint32_t kMaxShadeRounds = 64;  // hard bound of register-resident shading rounds per pass
constexpr int kLdsStack = 8;         // per-lane traversal stack entries kept in LDS by the megakernel; deeper
                                     // entries spill (exactly) to a per-wave global scratch

// One 4-wide BVH node = 128 B = one cache line, fetched as 8 x dwordx4 by ONE lane: the four child boxes
// as SoA (so the four slab tests are the same code on four registers), four child links and, per
// child, max |e1|*|e2| of its subtree (the error-bound term of the culling pad).
// child >= 0 : index of an inner node; child < 0 : leaf, ~child = (first_tri << kLeafBits) | (count - 1);
// kNoChild marks an unused slot, whose box is EMPTY (lo = +inf, hi = -inf) so that the slab test fails for every ray.
constexpr int32_t kNoChild = INT32_MIN;
struct alignas(128) BvhNode4 {
    float lo_x[4], lo_y[4], lo_z[4];
    float hi_x[4], hi_y[4], hi_z[4];
    int32_t child[4];
    float max_e12[4];
};
static_assert(sizeof(BvhNode4) == 128, "node must be 128 B");
// the traversal addresses planes by byte offset: lo_x 0, lo_y 16, lo_z 32, hi_x 48, hi_y 64, hi_z 80, child 96, max_e12 112

// One triangle record = 48 B (3 x dwordx4), stored in leaf order. The 9 fp32 values are exactly
// the 9 SoA streams the reference kernel reads (triangle.rs:177-187); `index` is the triangle's
// position in the reference arrays (ties in t resolve to the lowest index: triangle.rs:400).
struct alignas(16) BvhTri {
    float v0[3];
    float e1x;
    float e1yz[2];
    float e2xy[2];
    float e2z;
    uint32_t index;
    uint32_t pad[2];
};
static_assert(sizeof(BvhTri) == 48, "tri must be 48 B");

// The stored face normal of a mesh entry. w is 0 for a flat mesh. For a smooth mesh (rbrt_scene_shading_t) w holds the bits
// of n_total: the entry's smooth record (SmoothRec) is record [reference index] of the array that starts n_total Normal4s
// past the mesh's first Normal4, in the same allocation. The scatter pass loads the Normal4 anyway, so a flat hit pays one
// compare; the LDS layout of a launch does not depend on the shading.
struct alignas(16) Normal4 {
    float x, y, z, w;
};
// One smooth mesh entry: its geometry, bitwise the SoA arrays' (for the barycentrics), and its three corner normals.
struct alignas(16) SmoothRec {
    float v0[3], e1[3], e2[3];
    float n0[3], n1[3], n2[3];
    float pad[2];
};
static_assert(sizeof(SmoothRec) == 80 && sizeof(SmoothRec) % sizeof(Normal4) == 0, "smooth record must be 80 B");

struct DevSphere {
    float center[3];
    float radius;
};

// A BasicTriangle element (triangle.rs:9-34): first corner, the two edges from it, the stored normal.
struct DevTriangle {
    float v0[3], e0[3], e1[3], normal[3];
};

struct DevMaterial {
    float albedo[3];
    float param;   // a lambertian's: the bits of its pattern link (DevPattern below), 0 without a pattern
    int32_t kind;  // rbrt_material_kind_t, except that an emitter is stored as kDevMatEmissive
};
// Device code of RBRT_MAT_EMISSIVE. The megakernel's classify() turns a hit into status ST_LAMB + kind, and ST_LAMB - 1 is
// ST_TERM: an emitter's hit ends its path without a compare in the kernel (the TERM pass then starts the fold from L).
constexpr int32_t kDevMatEmissive = -1;
RBRT_HOST_DEVICE inline int32_t dev_material_kind(int32_t kind) { return kind == RBRT_MAT_EMISSIVE ? kDevMatEmissive : kind; }

// Solid patterns (rbrt_hip.h rbrt_scene_patterns_t). A scene with n_pat patterned objects has a material table of
// n_obj + n_pat entries, the k-th patterned object's albedo2 in entry n_obj + k, and n_pat DevPatterns right behind the table,
// in the same allocation: everything a kernel stages or reads as "the materials". A lambertian never reads its param, so
// the DEVICE copy of that word is the object's link: 0 for every unpatterned lambertian, whatever the caller passed, else
// (dword offset of its DevPattern from the table's start << kPatternLinkShift) | its second entry's number. A scatter
// records the entry's number where it recorded the object id (one byte per bounce), and the fold looks it up as it did.
struct DevPattern {
    float origin[3];
    float inv;  // 1.0f / size
};
constexpr uint32_t kPatternLinkShift = 8;
// dwords a scene's patterns add behind the n_obj materials: the second entries, then the DevPatterns
RBRT_HOST_DEVICE inline uint32_t pattern_table_dwords(uint32_t n_pat) {
    return n_pat * uint32_t((sizeof(DevMaterial) + sizeof(DevPattern)) / 4);
}
// Entry numbers are record bytes (<= 255); object ids also pass through pack_meta's 8-bit field as id + 1 (<= 254).
constexpr int kMaxMaterialEntries = 256;  // objects + patterned objects

struct DevMesh {
    const BvhNode4* nodes;
    const BvhTri* tris;      // the SCENE's triangle array (all meshes; this mesh's leaves point into its own part)
    const Normal4* normals;  // [reference index] -> (nx, ny, nz, 0), or (nx, ny, nz, bits of n_total) and the smooth records
    float bbox_lo[3];
    float bbox_hi[3];
    float center[3];  // of the bbox
    float radius;     // half diagonal of the bbox
    float max_e12;    // max |e1|*|e2| over the indexed triangles
    uint32_t n_nodes;
    uint32_t n_tris;
};

struct DevCounters {  // mirrors rbrt_hip_stats_t's counters
    unsigned long long rays, mesh_gate_pass, nodes_visited, tris_tested, mesh_hits, samples,
        nan_discriminants;
    // megakernel diagnostics (counting variant only; rbrt_hip_scene_debug_counters):
    // [0..5] passes per status kind, [6..11] lanes used per kind, [12] traversal wave-steps,
    // [13] active lane-steps, [14] refill rounds, [15] census rounds
    // [16] cycles in traversal steps, [17] cycles in shading passes, [18] total cycles (s_memtime, summed over waves)
    // [19] leaf rounds, [20] lanes with a leaf in those rounds, [21] node-walk rounds, [22] lanes walking in them
    // [23] waves that gave up on a bounded wait (must stay 0)
    // [24] min wave start, [25] max time work ran out, [26] max wave end, [27] sum of (end - start) (s_memrealtime, 100 MHz)
    unsigned long long diag[64];
};

// One node of an environment map: 16 bytes, so that a node is one load.
struct alignas(16) EnvTexel {
    float r, g, b, pad;
};

// Kernel arguments of one trace launch (passed by value).
struct TraceParams {
    rbrt_camera_t cam;
    float min_dist, max_dist, eps_frac;  // eps_frac = 1/min_dist (triangle.rs:146)
    float bg[3];
    uint32_t max_depth;
    uint32_t constant_bg;  // RBRT_FLAG_CONSTANT_BACKGROUND: a ray that hits nothing returns bg (in the padding ahead of seed_key)
    uint64_t seed_key;  // splitmix64(seed)
    uint32_t n_spheres, n_meshes;
    uint32_t n_elem_tris;          // BasicTriangle elements (rbrt_scene_t::triangles)
    const DevSphere* spheres;
    const DevTriangle* elem_tris;
    const uint32_t* elems;         // [n_spheres + n_elem_tris] Scene::elements order: bit 31 set = elem_tris[low bits], else spheres[..];
                                   // null when there are no triangles (element e is sphere e)
    const DevMaterial* materials;  // [object id]: the elements in their order, then the meshes
    const DevMesh* meshes;
    const BvhTri* tris;  // the triangle records of ALL meshes, one array; leaf links hold absolute positions in it
    // work decomposition
    uint32_t tiles_x, tiles_y, n_tiles;
    uint32_t tile_rank, tile_world, n_local_tiles;
    uint32_t sample_base;   // first sample index of this batch
    uint32_t batch;         // samples in this batch
    uint32_t tiles_reversed;  // 1: tiles are handed out last-to-first (scheduling only, see api.cpp empty_end_is_first)
    uint32_t batch_magic, tiles_x_magic;  // floor(2^32 / d) (d = 1: 2^32 - 1) for div_magic() in the kernels
    uint64_t n_items;       // n_local_tiles * 64 * batch
    float* sample_buf;      // [batch][n_local_tiles*64][3]
    DevCounters* counters;
    // persistent megakernel only
    unsigned long long* work_counter;  // [kWorkShards * kWorkCounterStride] next unclaimed item per shard (zeroed before every launch)
    uint32_t* gseq;                    // [n_waves][kPool][kMaxPathDepth/4] scatter records beyond the 4 kept in LDS
    uint32_t stack_entries;            // per-lane traversal stack entries kept in LDS (<= stack_need)
    uint32_t* gstack;                  // [n_waves][kStackMax][64] overflow of the LDS stacks
    uint32_t y_low_water;              // refill a traversal pass when fewer lanes than this are busy
    uint32_t y_high_water, y_high_min_parked;  // ... or fewer than y_high_water while at least that many rays are parked
    uint32_t leaf_round;               // test deferred leaves once this many lanes are stalled on one ...
    uint32_t share_idle;               // shared traversals: idle lanes needed for a round of giving (0: never)
    uint32_t leaf_leaves;              // ... or once this many leaves are pending (a leaf round deals their triangles out to all lanes)
    uint32_t work_stripes;             // chunks per stripe when the work shards interleave over the item range (0: contiguous eighths)
    uint32_t shade_rounds;             // shading pass: rounds a sphere-only bounce chain may stay in registers
    uint32_t shade_cont_min;           // ... as long as at least this many lanes continue (ignored once the work has run out)
    // The tile pass (kernels.hip primary_cull_kernel + tile_lists_kernel, run before the trace launch; both null: off).
    // tile_cull: one word per tile of the image: bit e < 24 = no camera ray of the tile can reach element e (a sphere),
    // bit 24 + m (m < 7) = none passes mesh m's box, bit 31 = all of them and the scene has nothing else: the tile sees
    // the background only. tile_lists: [0] = n_work, [1] = n_sky, then from [kTileListHeader] the rank's n_work local
    // tile numbers the trace kernel renders, ascending, and from [kTileListHeader + n_local_tiles] the n_sky
    // background-only ones, which sky_resolve_kernel finishes without the trace kernel ever seeing them.
    uint32_t* tile_cull;
    uint32_t* tile_lists;
    uint32_t tile_list_mode;  // order of the work list (tile_lists_kernel)
    uint32_t tile_tail_div;   // mode 4: the last n_work / this light tiles of the row-major order are handed out at the very end
    uint32_t tile_lists_wide;  // 1: tile_lists_kernel as four waves (a launch that has the GPU to itself); 0: as one wave
    // Helper launches (api.cpp "Elastic launches"): a second launch of the kernel that joins THIS launch's work -- same work
    // counters, same sample buffer -- when the GPU has room for more waves than the launch was issued with.
    // helper_words[0] = helper waves that may be holding work of the lane's launch, [1] = sequence number of the lane's
    // last launch that has been resolved (its counters are the next launch's by now); helper_seq = this launch's number.
    uint32_t* helper_words;
    uint32_t helper_seq;
    uint32_t wave_base;  // helper launches: first per-wave scratch slot (gseq / gstack) of this launch's waves; 0 for the launch itself
    uint32_t helper_min_items;  // helper launches: a helper wave joins only while at least this many work items per wave (the launch's and all its helpers') are left
    // RBRT_FLAG_THIN_LENS: thin_lens = 1 and the rbrt_camera_lens_t words past the camera; 0 (pinhole): the lens is never read
    uint32_t thin_lens;
    float lens_u[3], lens_v[3], focus_scale;
    // The handle's shutter (rbrt_hip_scene_set_shutter): shutter = 1 and the camera's translation during the exposure;
    // 0 (no shutter): the travel is never read and no draw is made for it
    uint32_t shutter;
    float travel[3];
    // The handle's motion (rbrt_hip_scene_set_motion): motion = [n_spheres][3], sphere i's translation during the exposure, on the
    // device; null (no motion): never read, and without a shutter no draw is made. gtime: [n_waves][kPool], the time s = phase + t
    // of the path in each pool slot of the trace kernel, beside gseq; allocated, written and read in a motion launch only
    const float* motion;
    float* gtime;
    uint32_t motion_gen;  // host only: the number of the rbrt_hip_scene_set_motion call the travels are from (the tile-table key)
    // The motion's phase (rbrt_hip_scene_set_motion_phase): a sample with the draw t sees sphere i at c_i + (s * travel_i),
    // s = motion_phase + t, one float32 addition. Read only where `motion` is not null; 0 gives s the bits of t
    float motion_phase;
    // The handle's environment (rbrt_hip_scene_set_environment): (env_n + 1)^2 texels of 16 bytes; null: bg / the sky gradient
    const EnvTexel* env_nodes;
    uint32_t env_n;
    // The short-path stage (short_paths.inl, run in front of the trace launch on its stream; null: off). One 64-bit word per
    // chunk of 64 work items, indexed by chunk number (work item >> 6): bit p set = item p of the chunk is finished -- its
    // sample is in sample_buf already, or its pixel lies beyond a ragged edge -- and the trace kernel hands it to nobody.
    // The stage writes every word of the launch: zero for the chunks of tiles it does not work on.
    unsigned long long* short_masks;
    // Solid patterns: the dwords behind the n_obj materials that belong to the table (pattern_table_dwords; 0: no patterns)
    uint32_t pattern_dw;
    // The handle's mesh motion (rbrt_hip_scene_set_mesh_motion): mesh_motion = [n_meshes][3], mesh m's translation during the
    // exposure, on the device; null (no mesh motion): never read. A launch with one always has `motion` too (the handle's, or
    // all zeros) and with it gtime and the phase: wherever a path tests mesh m it reads the origin o - (s * w_m), s = phase + t
    const float* mesh_motion;
    uint32_t mesh_motion_gen;  // host only: the number of the rbrt_hip_scene_set_mesh_motion call (the tile-table key)
};

struct ResolveParams {
    uint32_t width, height, tiles_x, n_tiles;
    uint32_t tile_rank, tile_world, n_local_tiles;
    uint32_t batch;
    uint32_t first_batch, last_batch;  // flags
    float inv_spp;                     // 1.0f / spp (lib.rs:101)
    const float* sample_buf;
    float* acc;           // [n_local_tiles*64][3] running sum
    float* out_radiance;  // row-major image if tile_world <= 1, else packed tiles; may be null
    uint8_t* out_rgb8;    // same indexing; may be null
    unsigned long long* work_counter;  // the finished launch's work counters, zeroed here for the lane's next launch
    const uint32_t* tile_lists;        // TraceParams::tile_lists (null: every local tile has samples in sample_buf)
    DevCounters* counters;             // sky_resolve_kernel in a counting launch: its samples and rays; else null
    uint32_t* helper_words;            // TraceParams::helper_words of the launch this resolves (null: none)
    uint32_t helper_seq;               // ... and its sequence number, published in helper_words[1]
    unsigned long long* error_flag;    // DevCounters::diag[57]: raised if helper waves of the launch never finish (bounded wait)
    // resolve_even_kernel / sky_resolve_even_kernel only (adaptive sampling; the plain resolves never read them)
    float* acc_even;       // [n_local_tiles*64][3] running sum of the samples with an even index
    uint32_t sample_base;  // index of the batch's first sample
};

// The feature buffers (include/rbrt_hip.h "Feature buffers"; features.inl): what one rbrt_hip_render_features call adds to the
// TraceParams of its camera and options (of which it reads the camera, the lens, the distances, the seed and the scene).
struct FeatureParams {
    uint32_t samples;        // n
    float inv_n;             // 1.0f / float(n)
    uint32_t stack_entries;  // per-lane traversal stack entries in LDS: the handle's bvh_stack_need
    float* albedo;           // [H][W][3] row-major; every output may be null
    float* normal;           // [H][W][3]
    float* depth;            // [H][W]
    float* coverage;         // [H][W]
    int32_t* object;         // [H][W]
    float* motion;           // [H][W][3]: the mean travel of what the samples hit (rbrt_hip_render_features_motion); null in
                             // every launch of the kernel's build without the channel
};

// Adaptive sampling (include/rbrt_hip.h "Adaptive sampling"): what adaptive_lists_kernel, tile_error_kernel and
// adaptive_finish_kernel need of one rbrt_hip_render_adaptive call. The arrays belong to the scene handle.
struct AdaptiveParams {
    uint32_t width, height, tiles_x;
    uint32_t tile_rank, tile_world, n_local_tiles;
    uint32_t n, n_max;            // n_k: samples of a tile that was active in this round; N = opts->spp
    float threshold;
    uint32_t first_round;         // 1: every tile is active, `active` is not read
    const uint32_t* tile_cull;    // TraceParams::tile_cull of the call's camera, or null (no tile pass: no tile is background only)
    uint32_t* tile_lists;         // the round's lists, laid out as TraceParams::tile_lists
    uint32_t* active;             // [n_local_tiles] 1: the tile takes part in the next round
    uint32_t* n_active;           // one word: tiles left active by the round (zeroed by adaptive_lists_kernel)
    uint32_t* tile_samples;       // [n_local_tiles] n_t
    float* tile_error;            // [n_local_tiles] the last E computed for the tile
    const float* acc;             // S and S_even: ResolveParams::acc, ::acc_even
    const float* acc_even;
    float* out_radiance;          // as ResolveParams (adaptive_finish_kernel); may be null
    uint8_t* out_rgb8;
};

// The denoiser (include/rbrt_hip.h "Denoising"; denoise.hip): one rbrt_hip_denoise_halves / rbrt_hip_scene_denoise call.
struct DenoiseParams {
    const float* a;        // [H][W][3] the two half images
    const float* b;
    const float* wa;       // [H][W] the share of `a`, or null: 0.5 everywhere
    uint32_t width, height;
    int32_t window_radius, patch_radius;
    float k2;              // strength * strength
    float* out_radiance;   // [H][W][3], may be null
    uint8_t* out_rgb8;     // [H][W][3], may be null
};

// ... and the step in front of it on a handle: the packed sums of the last adaptive call -> row-major A, B and wa.
struct DenoiseHalvesParams {
    const float* acc;             // S and S_even (AdaptiveParams::acc, ::acc_even), tile_world = 1
    const float* acc_even;
    const uint32_t* tile_samples; // [n_tiles] n_t
    uint32_t width, height, tiles_x;
    float* a;                     // [H][W][3]
    float* b;
    float* wa;                    // [H][W]
    float* out_a;                 // copies of a and b for the caller, may be null
    float* out_b;
};

// The display transform (include/rbrt_hip.h "Display transform"; tonemap.hip): one rbrt_hip_tonemap call.
struct TonemapParams {
    const float* in;          // [n][3] linear radiance
    uint32_t n;               // pixels, < 2^32
    uint32_t curve;           // RBRT_TONE_*
    float exposure, white;    // the manual values; 0: automatic
    float key;
    uint32_t key_permille, white_permille;
    uint32_t* hist;           // the workspace: [RBRT_TONEMAP_BINS] words, the rbrt_tonemap_result_t behind them; may be null
    float* out_radiance;      // [n][3], may be null or `in`
    uint8_t* out_rgb8;        // [n][3], may be null
};

// The glare stage (include/rbrt_hip.h "Glare"; glare.hip): one rbrt_hip_glare call.
struct GlareParams {
    const float* in;          // [height][width][3] linear radiance
    uint32_t width, height;   // width * height < 2^31
    uint32_t levels;          // 1..RBRT_GLARE_MAX_LEVELS
    float threshold, intensity, spread;
    float a;                  // intensity * (1 / n), the rule's normalisation, computed on the host
    void* workspace;          // the pyramid's levels 1..levels, float4 a pixel, level after level
    float* out_radiance;      // [height][width][3], may be null or `in`
    uint8_t* out_rgb8;        // [height][width][3], may be null
};

// The guided denoiser (include/rbrt_hip.h "Guided denoising"; guided.hip): one rbrt_hip_denoise_guided call.
struct GuidedParams {
    const float* a;          // [H][W][3] the two half images
    const float* b;
    const float* wa;         // [H][W] the share of `a`, or null: 0.5 everywhere
    const float* albedo;     // [H][W][3]
    const float* normal;     // [H][W][3]
    const float* depth;      // [H][W]
    const float* coverage;   // [H][W]
    uint32_t width, height;  // width * height < 2^31
    uint32_t levels;         // 1..RBRT_GUIDED_MAX_LEVELS
    uint32_t flags;          // RBRT_GUIDED_*
    float kc2, kz2, in, ia;  // the rule's host-side values
    void* workspace;         // six planes of width * height float4: {N, z}, {m, 0}, then {I, 0} and {V, 0} twice
    float* out_radiance;     // [H][W][3], may be null, `a` or `b`
    uint8_t* out_rgb8;       // [H][W][3], may be null
};

// Temporal accumulation (include/rbrt_hip.h "Temporal accumulation"; temporal.hip): one rbrt_hip_temporal_accumulate call.
struct TemporalParams {
    const float* a;             // [H][W][3] this frame's half images
    const float* b;
    const float* normal;        // [H][W][3]
    const float* depth;         // [H][W]
    const float* coverage;      // [H][W]
    const void* history_in;     // three planes of width * height float4: {A', len}, {B', c}, {N, z}; null: the first frame
    void* history_out;          // the same layout, may be null
    float* out_a;               // [H][W][3], may be null or `a`
    float* out_b;               // [H][W][3], may be null or `b`
    float* out_length;          // [H][W], may be null
    uint32_t width, height;     // width * height < 2^31
    float max_history, kz, kn2; // M, kz and kn * kn
    // this frame's camera K
    float pos[3], right[3], up[3], center[3];
    float mm_hor, mm_vert;
    // the last frame's camera K' and the rule's constants of it (unused without a history)
    float pos_prev[3], right_prev[3], up_prev[3];
    float n[3], w[3];
    float wn, rr, uu, ru, det, sx, sy, hx, hy;
    // rbrt_hip_temporal_accumulate_moving: [H][W][3] the motion buffer of this frame and this frame's phase minus the last
    // frame's; null in every launch of the kernel's build that follows no motion, which reads neither
    const float* motion;
    float phase_step;
};

// Guided upsampling (include/rbrt_hip.h "Guided upsampling"; upsample.hip): one rbrt_hip_upsample_halves call.
struct UpsampleParams {
    const float* a;             // [h][w][3] the low half images
    const float* b;
    const float* wa;            // [h][w], may be null: 0.5 everywhere
    const float* albedo;        // [H][W][3] the full-size features
    const float* normal;        // [H][W][3]
    const float* depth;         // [H][W]
    const float* coverage;      // [H][W]
    void* workspace;            // four planes of w * h float4: {a~, wa}, {b~, z_l}, {N_l, c_l}, {m_l, 0}
    float* out_a;               // [H][W][3], may be null
    float* out_b;               // [H][W][3], may be null
    float* out_wa;              // [H][W], may be null
    uint32_t width, height;     // W, H: W * H < 2^31
    uint32_t low_width, low_height;  // w = (W + f - 1) / f, h likewise
    uint32_t factor, flags;     // f in 1..RBRT_UPSAMPLE_MAX_FACTOR
    float in, ia, kz2, invf;    // 1 / (kn * kn), 1 / (ka * ka), kz * kz, 1 / float(f)
};

// Spike removal (include/rbrt_hip.h "Spike removal"; despike.hip): one rbrt_hip_despike_halves call.
struct DespikeParams {
    const float* a;             // [H][W][3] the half images
    const float* b;
    float* out_a;               // [H][W][3], may be null
    float* out_b;               // [H][W][3], may be null
    uint8_t* mask;              // [H][W], may be null
    uint32_t* counts;           // the rbrt_despike_result_t: {spikes_a, spikes_b, 0, 0}, zeroed on the stream; may be null
    uint32_t width, height;     // W, H: W * H < 2^31
    uint32_t radius, rank;      // R in 1..RBRT_DESPIKE_MAX_RADIUS, k in 1..RBRT_DESPIKE_MAX_RANK
    float threshold, floor;     // t, f
};

// Image comparison (include/rbrt_hip.h "Image comparison"; compare.hip): what one tile leaves in the workspace for the reduce
// kernel, and one rbrt_hip_compare_images call.
struct CompareTilePartial {
    double se, ae, rel, ssim;   // the tile's pairwise-tree sums
    float mx;                   // the fmaxf of the tile's mx
    uint32_t usable, skipped;   // the tile's pixels inside the image
    uint32_t pad;               // 0
};
static_assert(sizeof(CompareTilePartial) == 48, "the workspace holds 48 bytes a tile");

struct CompareParams {
    const float* x;             // [H][W][3] the image
    const float* ref;           // [H][W][3] the reference; may be x
    float* rel_map;             // [H][W], may be null
    float* ssim_map;            // [H][W], may be null
    CompareTilePartial* partials;  // [tiles] the caller's workspace; null without a result
    void* result;               // the rbrt_compare_result_t, may be null
    uint32_t width, height;     // W, H: W * H < 2^31
    uint32_t tiles_x, tiles;    // ceil(W / 16), and that times ceil(H / 16)
    float epsilon;              // eps
};

}  // namespace rbrt
