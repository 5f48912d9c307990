/*
 * rbrt_hip_debug.h — test hooks, diagnostics and lab knobs of librbrt_hip.so.
 *
 * NOT part of the drop-in boundary (that is rbrt_hip.h, which a Rust host binds): nothing here is needed to
 * replace rbrt_lib::render_scene (rbrt_lib/src/lib.rs:75-79). These entry points exist so that the parity tests
 * can look inside the hot path (one Scene::hit, one scatter event, the BVH builders alone, the two forms of the
 * mesh gate) and so that bench.py can time the trace kernel with events on the stream it really runs on.
 *
 * Lab knobs (environment, read by rbrt_hip_scene_create ONLY when RBRT_HIP_LAB=1; a value outside the stated range
 * makes scene_create fail with RBRT_ERR_INVALID_ARG instead of being clamped; none of them changes the image; the BVH
 * knobs are also read, with the same rules, by every call of the rbrt_hip_bvh_build_* entry points below):
 *   RBRT_LDS_STACK=1..64         stack entries per lane in LDS
 *   RBRT_Y_LOW / RBRT_Y_HIGH=1..64, RBRT_Y_HIGH_PARKED=1..256   refill water marks of the traversal lanes
 *   RBRT_LEAF_ROUND=1..64, RBRT_LEAF_LEAVES=1..128              when a leaf round runs
 *   RBRT_SHARE_IDLE=0..64        idle lanes needed for a round of shared traversals in the drain (4; 0: none)
 *   RBRT_WORK_STRIPES, RBRT_WORK_STRIPES_OVERLAP=0..65536, 0 or a power of two   chunks per stripe (0: contiguous shards)
 *   RBRT_SHADE_ROUNDS=1..64, RBRT_SHADE_CONT_MIN=1..64          register-resident shading rounds
 *   RBRT_WAVES_PER_CU=1..32      RBRT_PIPELINE=0..8
 *   RBRT_BVH_CT=(0, 1000]        SAH cost of a node visit, in triangle tests (4.0; a finite decimal number)
 *   RBRT_PLOC_RADIUS=1..256      the device builder's neighbour search (16)
 *   RBRT_BVH_DEVICE_MIN=0..1073741824   meshes of this many entries or more go to the device builder (instead of the cost rule)
 *   RBRT_BVH_DEVICE_ALGO=ploc|lbvh      RBRT_POISON_SAMPLES=0|1 (tests)
 *   RBRT_PRIMARY_CULL=0|1        the tile pass (1): tiles whose camera rays reach nothing bypass the trace kernel
 *   RBRT_TILE_TAIL_DIV=1..1024   a launch that has the GPU to itself: the share of the work list (1/n, 8) that is handed out
 *                                last, from light tiles (api.cpp list_mode_for)
 *   RBRT_OVERLAP_WAVES_PER_CU=0..16  waves per CU of a launch of a stream (0: 24 / launches side by side, rounded up, and
 *                                4 instead of 3 for a launch of 8 M work items or more)
 *   RBRT_TRACE_LAUNCHES=0|1      one stderr line per trace launch, tile pass and helper launch (which lane, grid, table set)
 *   RBRT_HELPERS=0|1|2           helper launches (elastic launches): never, by the watcher (1), one with every overlapped launch (tests)
 *   RBRT_HELPER_MIN_ITEMS=1..16777216   a helper wave joins only while n work items per wave are left (4096)
 *   RBRT_HELPER_ROUNDS=1..16     helper launches one launch can be given (4)
 *   RBRT_HELPER_MIN_LAUNCH_MI=0..4096   launches of n Mi work items or more get helper launches (16: smaller ones came out 1 % slower)
 *   RBRT_HELPER_MIN_FREE=1..16   helper launches only while this many wave slots per CU are free (1)
 *   RBRT_BVH_SPATIAL=[0, 0.6]    the host builder's budget of duplicated references (spatial splits), as a share of the triangles
 *   RBRT_TRACE_CREATE=0|1        one stderr line per rbrt_hip_scene_create: where its time went
 */
#ifndef RBRT_HIP_DEBUG_H
#define RBRT_HIP_DEBUG_H

#include "rbrt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the last rbrt_hip_render_device call on this scene split its samples: samples per batch (one trace launch
 * each, sized to the workspace cap $RBRT_HIP_WORKSPACE_MB and to the kernel's 32-bit work-item numbers) and the
 * number of batches. Diagnostic. */
int rbrt_hip_scene_last_batching(rbrt_hip_scene_t* scene, uint32_t* samples_per_batch, uint32_t* n_batches);

/* The rounds of the last rbrt_hip_render_adaptive call on this scene: *n_rounds = how many there were, and
 * active_tiles[k] (k < min(n, *n_rounds)) = the rank's tiles that were active at the start of round k. Diagnostic (the
 * C++ host's --report prints it). */
int rbrt_hip_scene_adaptive_rounds(rbrt_hip_scene_t* scene, uint32_t* active_tiles, size_t n, uint32_t* n_rounds);

/* Edge in pixels of the square pixel tile one workgroup of the denoising kernel covers (rbrt_amd/csrc/denoise.hip): image
 * sizes around it are where that kernel's edge handling changes (tests/test_denoise_gpu.py). */
#define RBRT_DENOISE_TILE 16u

/* Edge in pixels of the square pixel tile one workgroup of the guided denoiser's level kernel covers
 * (rbrt_amd/csrc/guided.hip): image sizes around it are where a workgroup is added (tests/test_guided_gpu.py). */
#define RBRT_GUIDED_TILE 16u
/* The levels of that kernel whose step is at most this stage their tile and its halo in LDS; the levels above read global
 * memory. Both forms compute the same bits. rbrt_hip_debug_guided_staging(0..4) changes it for the process and returns the
 * value in force, (-1) only asks (tools/guided_cost.py measures each; tests/test_guided_gpu.py compares their bits). The
 * switch is the process's, not a handle's or a stream's: every call of the filter reads it once when it starts, so changing it
 * while other threads call the filter changes only which form their next calls launch, never a result. */
#define RBRT_GUIDED_STAGED_MAX_STEP 4u
int rbrt_hip_debug_guided_staging(int max_step);

/* The temporal accumulation's kernel (rbrt_amd/csrc/temporal.hip) has no tile: a workgroup takes this many consecutive pixels
 * of the row-major image, so there is no RBRT_TEMPORAL_TILE. Pixel counts around it, as one row and as one column, are where a
 * workgroup is added (tests/test_temporal_gpu.py). */
#define RBRT_TEMPORAL_BLOCK 256u

/* The guided upsampling's gather kernel (rbrt_amd/csrc/upsample.hip): the tile of FULL pixels one workgroup makes, whose low
 * pixels it stages in LDS. Sizes around it, and twice it so that an interior workgroup exists, are where that kernel's paths
 * change (tests/test_upsample_gpu.py). The reduce kernel has no tile: a workgroup takes 256 consecutive low pixels. */
#define RBRT_UPSAMPLE_TILE_W 32u
#define RBRT_UPSAMPLE_TILE_H 8u

/* The spike removal's kernel (rbrt_amd/csrc/despike.hip): the tile of pixels one workgroup makes, whose luminances it stages in
 * LDS with a halo of the radius. Sizes around it, twice it, and three times it and a little where an interior workgroup has
 * halos on all four sides, and spikes either side of a tile's edge and the radius away from it, are where that kernel's
 * paths change (tests/test_despike_gpu.py, tests/despike_cases.py). */
#define RBRT_DESPIKE_TILE_W 32u
#define RBRT_DESPIKE_TILE_H 8u

/* The display transform's kernels (rbrt_amd/csrc/tonemap.hip): the pixels one workgroup takes per stride of its grid, and the
 * cap of that grid. Pixel counts around BLOCK_PIXELS, and around MAX_BLOCKS * BLOCK_PIXELS where a workgroup starts to stride a
 * second time, are where those kernels' paths change (tests/test_tonemap_gpu.py). */
#define RBRT_TONEMAP_BLOCK_PIXELS 1024u
#define RBRT_TONEMAP_MAX_BLOCKS 512u

/* The glare stage's kernels (rbrt_amd/csrc/glare.hip): the tile of a pyramid level that one workgroup of the REDUCE kernel
 * makes, from (2 * TILE_W + 3) x (2 * TILE_H + 3) pixels of the level above. Image sizes around twice the tile are where that
 * kernel's edge handling changes; the composite's workgroup takes 4 * TILE_W x TILE_H pixels (tests/test_glare_gpu.py). */
#define RBRT_GLARE_TILE_W 16u
#define RBRT_GLARE_TILE_H 16u

/* Test / diagnostic hook for Scene::hit (scene.rs:19-43): closest hit of n rays against the
 * resident scene. Host arrays. rays = n x {ox,oy,oz,dx,dy,dz}. Outputs (each may be NULL):
 *   out_t[n]      ray parameter of the winning object (NaN on miss)
 *   out_obj[n]    -1 on miss, sphere index in [0,n_spheres), or n_spheres + mesh index
 *   out_tri[n]    winning triangle index (reference numbering) for mesh hits, else -1
 *   out_dist[n]   dist_from_ray_orig of the winner (lib.rs:35)
 * The rays are traced as given: the handle's shutter (rbrt_hip_scene_set_shutter) does not move them, and they see the spheres
 * at their opening positions whatever motion the handle has (rbrt_hip_scene_set_motion): there is no sample stream to draw t from. */
int rbrt_hip_trace_rays(rbrt_hip_scene_t* scene, const float* rays, size_t n, float min_dist,
                        float max_dist, float* out_t, int32_t* out_obj, int32_t* out_tri,
                        float* out_dist);

/* Test hook for BoundingBox::hit (aabbox.rs:28-58): n rays against the box [lo, hi], decided by the division-free
 * form the megakernel uses (out_fast[n]) and by the verbatim form with six IEEE divisions (out_exact[n]); the two
 * must agree for every input. Host arrays. */
int rbrt_hip_selftest_gate(const float lo[3], const float hi[3], const float* rays, size_t n, uint8_t* out_fast,
                           uint8_t* out_exact);

/* Test hook: the image needs correctly rounded sqrt and / (vec3.rs:111-126); the kernels use short forms of them when
 * every lane's operands are in the everyday range (kernels.hip "IEEE square root and division, the short way"). Runs n
 * pseudo-random operands, three quarters of the waves drawn from the whole domain the gates admit, through the short forms
 * and the compiler's: counts[0] / counts[1] = differing sqrt results / normalize components (must be 0), counts[2] = lanes
 * whose sqrt and normalize both took the short path. */
int rbrt_hip_selftest_ieee(uint64_t seed, size_t n, uint64_t counts[3]);

/* Test hook: the kernels' ieee_sqrt of x[n] and normalize of v[m][3] (host arrays), element i in lane i % 64 of wave
 * i / 64 (a short form runs only when every lane of the wave is inside its gate). out_sqrt[n], out_norm[m][3]: the
 * results; out_sqrt_short[n] / out_norm_short[m]: 1 where the element's wave took the short form. */
int rbrt_hip_debug_ieee(const float* x, size_t n, const float* v, size_t m, float* out_sqrt, uint8_t* out_sqrt_short,
                        float* out_norm, uint8_t* out_norm_short);

/* Test hook: the kernels' ieee_sqrt of every float whose bits are in [first_bits, first_bits + n) (positive normal floats
 * only), 64 consecutive ones per wave, checked on the device: counts[0] = results that are not the correctly rounded
 * square root (an exact integer test), counts[1] = results that differ from the compiler's sqrt, counts[2] = lanes that
 * took the short form. */
int rbrt_hip_selftest_sqrt_sweep(uint32_t first_bits, uint64_t n, uint64_t counts[3]);

/* Diagnostic: pass statistics of the persistent megakernel from the last render with
 * RBRT_FLAG_COLLECT_STATS: out[0..5] passes per kind (empty, traverse, terminate, lambertian, metal,
 * dielectric), out[6..11] path slots handled per kind, out[12] traversal wave-steps, out[13] busy
 * lane-steps, out[14] refill rounds, out[15] scheduling rounds. */
int rbrt_hip_scene_debug_counters(rbrt_hip_scene_t* scene, uint64_t* out, size_t n);

/* Diagnostic: preset slot `index` (< 64) of the counters rbrt_hip_scene_debug_counters reads (analysis builds keep
 * minima there, which must start at all-ones). Synchronises the device. */
int rbrt_hip_scene_debug_set_counter(rbrt_hip_scene_t* scene, size_t index, uint64_t value);

/* Diagnostic: run the host-side BVH builder alone (needs no device). *nodes_out / *tris_out are
 * malloc'ed copies of the 128-B 4-wide node and 48-B triangle records (layout: rbrt_amd/csrc/device_types.h);
 * release them with rbrt_hip_free_host. */
int rbrt_hip_bvh_build_host(const rbrt_mesh_t* mesh, void** nodes_out, size_t* n_nodes, void** tris_out,
                            size_t* n_tris, uint32_t* max_depth, float* max_e12);
void rbrt_hip_free_host(void* p);
/* Diagnostic: the host builder over n 48-B triangle records (device_types.h BvhTri) in ANY order, `index` = the triangle's
 * position in the reference arrays: for the indexed records of a mesh, array for array the tree rbrt_hip_bvh_build_host
 * makes of that mesh. (It is what a scene handle's background thread runs on the device builder's output.) */
int rbrt_hip_bvh_build_host_records(const void* records, size_t n, void** nodes_out, size_t* n_nodes, void** tris_out,
                                    size_t* n_tris, uint32_t* max_depth, float* max_e12);
/* Diagnostic: the GPU-side BVH builder alone (rbrt_amd/csrc/bvh_device.hip; rbrt_hip_scene_create uses it wherever it costs the
 * call less than the host builder, $RBRT_BVH_BUILDER = host | device overrides). Same outputs as rbrt_hip_bvh_build_host;
 * *built = 0 when the builder declined the mesh (fewer than 8 entries, <= 4 indexed triangles, or a tree beyond the
 * traversal's depth budget), in which case scene_create falls back to the host builder. */
int rbrt_hip_bvh_build_device(const rbrt_mesh_t* mesh, void** nodes_out, size_t* n_nodes, void** tris_out,
                              size_t* n_tris, uint32_t* max_depth, float* max_e12, int* built);

/* Test hook for RayScattering::scatter (materials.rs:4-12; lambertian.rs:11-24, metal.rs:12-25, dielectric.rs:11-85):
 * n independent scatter events on the device code the megakernel shades with. Event i: incoming ray direction
 * in_dir[i], hit point p[i], hit normal normal[i] (as the intersection routines hand it over: unnormalised for
 * spheres), material mats[i], and the state of its random stream rng_state[i] = {s0, s1} (the xoroshiro64** words
 * of DESIGN.md "RNG contract"; the draws are consumed in the reference's order). Outputs (each may be NULL):
 *   out_dir[n][3]      direction of the scattered ray (its origin is p)
 *   out_ok[n]          the reference's bool (metal.rs:25 can return false)
 *   out_rng_state[n]   the stream's state afterwards (how many draws were consumed)
 * Host arrays. So that an image mismatch can be localised to one material without bisecting images. */
int rbrt_hip_debug_scatter(const rbrt_material_t* mats, const float* in_dir, const float* p, const float* normal,
                           const uint32_t* rng_state, size_t n, float* out_dir, uint8_t* out_ok, uint32_t* out_rng_state);

/* Test hook for the primary-ray culling table (DESIGN.md "The tile pass"): what the library computes on the trace
 * launch's stream before every launch for `cam`, one word per 8x8 tile of the image in row-major tile order
 * (n_words must be ceil(width/8) * ceil(height/8)): bit e < 24 = no camera ray of the tile can reach element e (spheres
 * only), bit 24 + m (m < 7) = none can pass the box of mesh m, bit 31 = the tile sees the background only (every sphere
 * out of reach, and every mesh: by its box, or by the boxes at the top of its tree). A set bit is a promise; tests check
 * it against the oracle's rays. Host array. */
int rbrt_hip_debug_primary_cull(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, uint32_t* out_words, size_t n_words);
/* The same table for the camera rays of a RBRT_FLAG_THIN_LENS render with `lens` (kernels.hip primary_cull_kernel, "Lens
 * rays"). The lens is validated like the render entry points' (RBRT_ERR_INVALID_ARG). */
int rbrt_hip_debug_primary_cull_lens(rbrt_hip_scene_t* scene, const rbrt_camera_lens_t* lens, uint32_t* out_words, size_t n_words);
/* The same table for the camera rays of a render with the shutter `travel` (rbrt_hip.h "Camera shutter"; kernels.hip
 * primary_cull_kernel, "Shutter rays"), whatever shutter the handle has, which the hook leaves as it is. cam: the camera;
 * lens: NULL for a pinhole, else the lens whose `cam` member is used and `cam` is ignored (it may be NULL). The lens is
 * validated like a render's, the travel like rbrt_hip_scene_set_shutter's (RBRT_ERR_INVALID_ARG). */
int rbrt_hip_debug_primary_cull_shutter(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, const rbrt_camera_lens_t* lens,
                                        const float travel[3], uint32_t* out_words, size_t n_words);
/* The same table as a render with `opts` computes it: the tree boxes the pass tests are grown by a pad that holds
 * 1 / opts->min_dist, so the table belongs to a distance window. opts->flags are honoured (with RBRT_FLAG_THIN_LENS `cam` is
 * the first member of a rbrt_camera_lens_t, as for a render) and validated like a render's (RBRT_ERR_INVALID_ARG). The two
 * hooks above are this one with rbrt_render_opts_default's options. */
int rbrt_hip_debug_primary_cull_opts(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, const rbrt_render_opts_t* opts,
                                     uint32_t* out_words, size_t n_words);

/* Test hook for smooth shading (rbrt_hip.h rbrt_scene_shading_t): for each of n rays (ox, oy, oz, dx, dy, dz; host array),
 * the normal the scatter of the megakernel would use at its closest hit (rbrt_hip_trace_rays' hit), computed by the same
 * device function: a sphere's unnormalised p - center, a BasicTriangle's or a flat mesh's stored normal, a smooth mesh's
 * n_s. out_normal: host float[n][3], NaN for a miss. */
int rbrt_hip_debug_shading_normals(rbrt_hip_scene_t* scene, const float* rays, size_t n, float min_dist, float max_dist,
                                   float* out_normal);

/* Test hook for solid patterns (rbrt_hip.h rbrt_scene_patterns_t): for each of n rays (ox, oy, oz, dx, dy, dz; host array),
 * the attenuation scatter would record at its closest hit (rbrt_hip_trace_rays' hit), the material entry chosen by the same
 * device function the scatter pass, the short-path stage and the feature buffers use: a patterned object gives its cell's
 * colour, other lambertians and metals their albedo, a dielectric (1, 1, 1), an emitter its radiance.
 * out_albedo: host float[n][3], NaN for a miss. */
int rbrt_hip_debug_surface_albedo(rbrt_hip_scene_t* scene, const float* rays, size_t n, float min_dist, float max_dist,
                                  float* out_albedo);

/* Test hook for environment lighting (rbrt_hip.h rbrt_environment_t): the lookup alone, for n directions (dx, dy, dz; host
 * array, used as they are), through the same device function the trace kernel and the background-only kernels call.
 * out_rgb: host float[n][3]. RBRT_ERR_INVALID_ARG when the handle has no environment. */
int rbrt_hip_debug_environment(rbrt_hip_scene_t* scene, const float* dirs, size_t n, float* out_rgb);

/* Kernel timing with HIP events recorded on the launch stream around every trace-kernel launch
 * (and the resolve kernel after it). set_timing(scene, 1) starts / restarts the accumulation;
 * kernel_ms sums the durations of all launches since then (it synchronises on the last event) and
 * returns how many trace launches that was. */
int rbrt_hip_scene_set_timing(rbrt_hip_scene_t* scene, int enable);
int rbrt_hip_scene_kernel_ms(rbrt_hip_scene_t* scene, float* trace_ms_total, float* resolve_ms_total,
                             uint32_t* n_trace_launches);

/* Trace launches since set_timing(scene, 1), by grid: the full grid, or the part of the wave slots a launch of a stream
 * takes (rbrt_hip_scene_set_pipeline; "half" is round 2's name for it), so the mix depends on host timing. */
int rbrt_hip_scene_launch_mix(rbrt_hip_scene_t* scene, uint32_t* n_full_grid, uint32_t* n_half_grid);

/* Helper launches since set_timing(scene, 1): more waves given to launches already running when the GPU has room and the
 * caller has stopped issuing (api.cpp "Elastic launches"; lab knob RBRT_HELPERS=0|1|2: never, automatic, with every launch). */
int rbrt_hip_scene_helper_launches(rbrt_hip_scene_t* scene, uint32_t* n);

/* Which build of the trace kernel the handle's last trace launch ran (its helper launches run the same one). The kernel
 * has a general build and a PLAIN one, which has the default values of the lab knobs RBRT_Y_LOW, RBRT_Y_HIGH,
 * RBRT_Y_HIGH_PARKED, RBRT_LEAF_ROUND, RBRT_LEAF_LEAVES, RBRT_SHARE_IDLE, RBRT_SHADE_ROUNDS and RBRT_SHADE_CONT_MIN
 * (rbrt_amd/csrc/trace_knobs.h) and the plain scene -- spheres and exactly one mesh, no BasicTriangle element, no lens, no
 * shutter, no environment map, no pattern -- built in as constants. A launch runs the PLAIN build when all of that holds for
 * it and it is not a counting launch (RBRT_FLAG_COLLECT_STATS). Both compute the same bits (tests/test_plain_build_gpu.py).
 * *build: RBRT_TRACE_BUILD_NONE before the first launch.
 * The choice has a lab control of its own, read and validated by rbrt_hip_scene_create under the rules of the lab knobs at
 * the top of this file: RBRT_TRACE_BUILD=auto (the default: as described) | general (the general build for every launch of
 * the handle, for A/B runs and the bit comparison); any other string is RBRT_ERR_INVALID_ARG. */
#define RBRT_TRACE_BUILD_NONE 0
#define RBRT_TRACE_BUILD_GENERAL 1
#define RBRT_TRACE_BUILD_PLAIN 2
int rbrt_hip_scene_last_trace_build(rbrt_hip_scene_t* scene, int* build);

/* The short-path stage (DESIGN.md "The tile pass"; short_paths.inl): a streaming kernel in front of every trace launch that
 * has tile tables finishes the two-ray paths of the tiles no camera ray of which can pass a mesh box, and the trace kernel
 * skips those samples. The image is the same bits either way. For the handle's later launches, mode 0: never (the A/B and
 * the tests need both); 1 (the default): in front of the launches that run beside others -- those of a stream of calls, and a
 * call's sample batches but the last -- where the stage's own latency is hidden, not in front of a blocking frame, which
 * would pay it in full; 2: in front of every launch; anything else is RBRT_ERR_INVALID_ARG. Counting launches
 * (RBRT_FLAG_COLLECT_STATS), the rounds of rbrt_hip_render_adaptive, renders without the tile pass and scenes of more than
 * seven meshes never have the stage. */
int rbrt_hip_scene_set_short_paths(rbrt_hip_scene_t* scene, int mode);
/* Test hook: the finished masks the stage wrote for the handle's LAST trace launch that had one, after waiting for the
 * device. One word per chunk of 64 work items in hand-out order -- chunk = (position in the launch's tile work list) *
 * (samples of the launch) + (sample within the launch), bit p = pixel p of the 8x8 tile -- a set bit: the stage finished
 * that sample (or its pixel lies beyond a ragged edge), a clear one: the trace kernel traced it; the chunks of tiles the
 * stage does not work on are zero. *n_chunks: the launch's chunks (0: no launch of the handle has had the stage); at most
 * n words are written to out_masks (host array; may be NULL with n = 0). */
int rbrt_hip_debug_short_masks(rbrt_hip_scene_t* scene, uint64_t* out_masks, size_t n, size_t* n_chunks);

/* Where the wall-clock time of rbrt_hip_scene_create (and, for the one-shot rbrt_hip_render, of the whole call) went, in
 * seconds. The parts of create_s: hip_init_s + upload_s + bvh_build_s + lanes_s (+ a remainder of validation and small
 * allocations); of total_s: create_s + render_s + copy_s + destroy_s. bench.py's one_shot leg and the CLI's --report read it. */
typedef struct rbrt_hip_call_times {
    double hip_init_s;  /* device selection: the HIP runtime's own start-up when this is a process's first HIP call */
    double upload_s;    /* the caller's scene arrays to the device */
    double bvh_build_s; /* BVH construction: the host builder's CPU time + upload of its tree, or the device builder's kernels */
    double lanes_s;     /* pipeline lanes (streams, events, per-wave scratch) and loading the device code */
    double create_s;    /* all of rbrt_hip_scene_create */
    double render_s;    /* rbrt_hip_render only: issue of the render to the synchronised device image */
    double copy_s;      /* rbrt_hip_render only: image to the caller's host buffers */
    double destroy_s;   /* rbrt_hip_render only: scene and buffers released */
    double total_s;     /* rbrt_hip_render only */
    uint32_t meshes_device_built, meshes_host_built;
} rbrt_hip_call_times_t;
int rbrt_hip_scene_create_times(rbrt_hip_scene_t* scene, rbrt_hip_call_times_t* out);
int rbrt_hip_last_render_times(rbrt_hip_call_times_t* out); /* of the calling thread's last rbrt_hip_render */

/* A scene handle starts with the trees that cost rbrt_hip_scene_create least -- the device builder's for all but small meshes
 * -- and a background thread makes the host builder's (better) trees of those meshes, which the first render call that
 * finds them ready adopts (api.cpp "The tree a scene STARTS with"; $RBRT_BVH_REFINE=0 turns it off). This waits up to
 * timeout_s for that thread and adopts its result now. *state: 0 = none was started, 1 = its trees are in use, 2 = it
 * failed or was cancelled (rbrt_hip_last_error says why; the first trees stay), 3 = still at work. *build_seconds: start of
 * the thread to its trees on the device. Either pointer may be NULL. Tests and bench.py (whose counting pass and timed
 * legs have to run on ONE tree) use it. */
int rbrt_hip_scene_refine_wait(rbrt_hip_scene_t* scene, double timeout_s, int* state, double* build_seconds);

#ifdef __cplusplus
}
#endif
#endif /* RBRT_HIP_DEBUG_H */
