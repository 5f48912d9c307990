/*
 * rbrt_hip.h — C ABI of the MI355X (gfx950) path-tracing hot path.
 *
 * This is the drop-in boundary for the ONE call the reference makes into its
 * render hot path:
 *
 *     rbrt_lib::render_scene(cam: Camera, num_samples: u32, scene: Scene)
 *         -> image::ImageBuffer<Rgb<u8>, Vec<u8>>          (rbrt_lib/src/lib.rs:75-79,
 *                                                           called at src/main.rs:82)
 *
 * Everything below is plain-old-data: borrowed pointers + sizes, no callbacks,
 * no C++/torch types. A Rust host binds it with an `extern "C"` block (see
 * INTEGRATION.md); the C++ host in rbrt_amd/host/ and the Python ctypes mirror
 * in rbrt_amd/abi.py bind the same symbols.
 *
 * Conventions
 *   - every entry point returns 0 (RBRT_OK) or a negative rbrt_status_t; it never
 *     aborts or throws across the boundary. rbrt_hip_last_error() returns a
 *     thread-local human-readable message for the last failure.
 *   - all pointers are borrowed for the duration of the call only (scene_create
 *     copies what it needs to the device before returning).
 *   - images are row-major, row 0 = TOP row, 3 channels interleaved (RGB):
 *       radiance: float[H][W][3]  — linear, pre-gamma mean over samples (lib.rs:95-101)
 *       rgb8    : uint8[H][W][3]  — (sqrt(c)*256) saturating cast (lib.rs:116-122)
 *   - there is NO CPU fallback: without a usable HIP device every render entry
 *     point fails with RBRT_ERR_NO_DEVICE.
 *   - environment: the library reads four variables, all optional --
 *       RBRT_HIP_WORKSPACE_MB   cap of one pipeline lane's sample workspace in MiB (default 1024)
 *       RBRT_BVH_BUILDER        host | device: force one BVH builder (default: a mesh's first tree by whichever builder
 *                               costs the call less, the host builder's tree following from a background thread)
 *       RBRT_BVH_REFINE         0: no background build, a handle keeps the tree it started with
 *       RBRT_BVH_THREADS        threads of the host BVH builder (default: the machine's, at most 16)
 *     and takes note of GPU_MAX_HW_QUEUES as the process had it when the library was loaded (the HIP runtime's own
 *     variable: the frame pipeline is planned for the hardware queues the runtime really has).
 *   - threads: besides the caller's, a scene handle may own a background BVH builder and, once it has seen a stream of
 *     calls, a watcher that gives launches still running the wave slots that have become free (rbrt_hip_scene_destroy
 *     ends both). A handle is still used by ONE calling thread at a time.
 *     Everything else that tunes the kernels' scheduling is a lab knob: ignored unless RBRT_HIP_LAB=1 is set, and
 *     documented with the test / diagnostic entry points in rbrt_hip_debug.h, not here. No knob changes the image.
 */
#ifndef RBRT_HIP_H
#define RBRT_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBRT_ABI_VERSION 2 /* 2: rbrt_scene_t grew n_triangles / triangles / element_order (appended: the v1 prefix is unchanged);
                              entry points added since (rbrt_hip_tile_xy / _tile_number) change no struct and no existing call;
                              neither do RBRT_MAT_EMISSIVE and RBRT_FLAG_CONSTANT_BACKGROUND, added since (a library without
                              them answers a kind-3 material with RBRT_ERR_INVALID_ARG), nor RBRT_FLAG_THIN_LENS with its
                              rbrt_camera_lens_t (rbrt_camera_t stays as it is: the lens wraps it) and
                              rbrt_hip_supported_flags, nor the smooth shading of meshes (rbrt_scene_shading_t and the
                              two *_shaded entry points: rbrt_mesh_t and rbrt_scene_t stay as they are), nor solid patterns
                              (rbrt_scene_patterns_t and the two *_patterned entry points, detected by the symbol), nor the camera shutter (rbrt_shutter_t and
                              rbrt_hip_scene_set_shutter: handle state like the environment, detected by the symbol), nor moving spheres (rbrt_motion_t and
                              rbrt_hip_scene_set_motion: handle state like the shutter, detected by the symbol), nor animation
                              (rbrt_hip_scene_set_motion_phase, rbrt_hip_render_features_motion and
                              rbrt_hip_temporal_accumulate_moving: added entry points, each detected by its symbol), nor moving
                              meshes (rbrt_mesh_motion_t and rbrt_hip_scene_set_mesh_motion: handle state, detected by the symbol), nor adaptive
                              sampling (rbrt_hip_render_adaptive with its two structs: an added entry point), nor the
                              denoiser (rbrt_denoise_opts_t, rbrt_denoise_opts_default, rbrt_hip_denoise_halves and
                              rbrt_hip_scene_denoise: added entry points), nor environment lighting (rbrt_environment_t and
                              rbrt_hip_scene_set_environment: an added struct and entry point, no new flag bit, every
                              existing struct untouched; a host detects it by the symbol), nor the display transform
                              (rbrt_tonemap_opts_t, rbrt_tonemap_result_t, rbrt_tonemap_opts_default and rbrt_hip_tonemap: added
                              structs and entry points, detected by the symbol), nor glare
                              (rbrt_glare_opts_t, rbrt_glare_opts_default, rbrt_hip_glare_workspace_bytes and rbrt_hip_glare:
                              an added struct and entry points, detected by the symbol), nor the feature buffers
                              (rbrt_feature_opts_t, rbrt_feature_opts_default and rbrt_hip_render_features: an added struct
                              and entry points, detected by the symbol), nor the guided denoiser
                              (rbrt_guided_opts_t, rbrt_guided_opts_default, rbrt_hip_guided_workspace_bytes,
                              rbrt_hip_denoise_guided and rbrt_hip_scene_denoise_guided: an added struct and entry points,
                              detected by the symbol), nor temporal accumulation (rbrt_temporal_opts_t,
                              rbrt_temporal_opts_default, rbrt_hip_temporal_history_bytes and rbrt_hip_temporal_accumulate:
                              an added struct and entry points, detected by the symbol), nor guided upsampling
                              (rbrt_upsample_opts_t, rbrt_upsample_opts_default, rbrt_hip_upsample_camera,
                              rbrt_hip_upsample_workspace_bytes and rbrt_hip_upsample_halves: an added struct and entry
                              points, detected by the symbol), nor spike removal (rbrt_despike_opts_t,
                              rbrt_despike_result_t, rbrt_despike_opts_default and rbrt_hip_despike_halves: added structs
                              and entry points, detected by the symbol), nor image comparison (rbrt_compare_opts_t,
                              rbrt_compare_result_t, rbrt_compare_summary_t, rbrt_compare_opts_default,
                              rbrt_hip_compare_workspace_bytes, rbrt_hip_compare_images and rbrt_compare_summary: added
                              structs and entry points, detected by the symbol) */

typedef enum rbrt_status {
    RBRT_OK = 0,
    RBRT_ERR_INVALID_ARG = -1,
    RBRT_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at init */
    RBRT_ERR_HIP = -3,         /* a HIP call failed; see rbrt_hip_last_error() */
    RBRT_ERR_OOM = -4,
    RBRT_ERR_UNSUPPORTED = -5, /* e.g. max_depth above the kernel's compiled limit */
    RBRT_ERR_NAN = -6          /* reference would have panicked: sphere.rs:33 "Encountered NAN" */
} rbrt_status_t;

/* Material = the closed set the reference's YAML factory can build
 * (blueprints.rs:50-74); replaces `Box<dyn RayScattering + Sync>` (materials.rs:4-12).
 * Emissive (no counterpart in the reference, whose only light is the background): a surface that emits radiance
 * `albedo` (linear, per channel, values above 1 allowed) from both sides and scatters nothing. Scene::hit treats it like
 * any other object (it occludes); when it is a path's closest hit, colorize returns `albedo` at every remaining depth,
 * depth 0 included, without drawing a random number, so a sample is a1 * (a2 * (... * (ak * L))) over the albedos of the
 * scattering bounces before it. scene_create / render reject a non-finite or negative component with
 * RBRT_ERR_INVALID_ARG. Every other kind value is rejected the same way. */
typedef enum rbrt_material_kind {
    RBRT_MAT_LAMBERTIAN = 0, /* lambertian.rs:11-24: albedo            */
    RBRT_MAT_METAL = 1,      /* metal.rs:12-25     : albedo, param=roughness */
    RBRT_MAT_DIELECTRIC = 2, /* dielectric.rs:11-59: param=ref_idx     */
    RBRT_MAT_EMISSIVE = 3    /* albedo = emitted radiance L, param unused */
} rbrt_material_kind_t;

typedef struct rbrt_material {
    int32_t kind;    /* rbrt_material_kind_t */
    float albedo[3]; /* ignored for dielectric (attenuation is (1,1,1), dielectric.rs:18); emissive: the emitted radiance */
    float param;     /* metal: roughness; dielectric: ref_idx; lambertian, emissive: unused */
} rbrt_material_t;

/* sphere.rs:6-10 */
typedef struct rbrt_sphere {
    float center[3];
    float radius;
    rbrt_material_t mat;
} rbrt_sphere_t;

/* mesh.rs:12-25 as produced by convert_to_soa_mesh (mesh.rs:123-181).
 * Every SoA array has n_total = N + N % 8 entries (the reference's padding rule,
 * mesh.rs:134-144, kept as is). The library applies the chunks_exact(8)
 * truncation of triangle.rs:166-167 itself: only the first 8*floor(n_total/8)
 * entries are ever tested, and entries with is_padding[i] != 0 never win
 * (triangle.rs:400). vertices[1], vertices[2] of the reference struct are never
 * read on the hot path and are not part of the ABI. */
typedef struct rbrt_mesh {
    uint32_t n_total;          /* length of each array below */
    uint32_t n_real;           /* N = triangles loaded from the .obj (informational) */
    const float* v0x;          /* vertices[0][0..2]  (triangle.rs:177-179) */
    const float* v0y;
    const float* v0z;
    const float* e1x;          /* edges[0][0..2] = v1 - v0 (mesh.rs:57-60) */
    const float* e1y;
    const float* e1z;
    const float* e2x;          /* edges[1][0..2] = v2 - v0 */
    const float* e2y;
    const float* e2z;
    const float* nx;           /* normals[0..2] = normalize(e1 x e2) (triangle.rs:30-34) */
    const float* ny;
    const float* nz;
    const uint8_t* is_padding; /* mesh.rs:138-144 */
    float bbox_lo[3];          /* BoundingBox of the N real triangles (mesh.rs:62, aabbox.rs:62-88) */
    float bbox_hi[3];
    rbrt_material_t mat;       /* one material per mesh (mesh.rs:24) */
} rbrt_mesh_t;

/* triangle.rs:9-34: BasicTriangle, the reference's second `Intersectable` (lib.rs:38-41) besides Sphere -- a single
 * triangle as a scene element, corners counter-clockwise. The YAML factory never creates one (blueprints.rs:132-158
 * builds spheres and meshes only), but Scene::elements is a Vec<Box<dyn Intersectable>> and admits it; a host that
 * fills it with triangles gets them rendered. Intersection: triangle.rs:92-130 (scalar Moller-Trumbore, |a| < min_dist
 * rejects, 0 <= u <= 1, v >= 0, u + v <= 1, t > min_dist, then the distance window) and :412-441; the hit normal is
 * normalize((c1 - c0) x (c2 - c0)) (triangle.rs:30-34), computed by the library, never flipped towards the ray. */
typedef struct rbrt_triangle {
    float corners[3][3];
    rbrt_material_t mat;
} rbrt_triangle_t;

/* scene.rs:12-16 (lights are always empty in the reference: blueprints.rs:151) */
typedef struct rbrt_scene {
    uint32_t n_spheres;
    const rbrt_sphere_t* spheres; /* the spheres of Scene::elements, YAML order (scene.rs:23-31) */
    uint32_t n_meshes;
    const rbrt_mesh_t* meshes;    /* Scene::triangle_meshes, YAML order (scene.rs:33-41) */
    uint32_t n_triangles;
    const rbrt_triangle_t* triangles; /* the BasicTriangles of Scene::elements */
    /* Order of Scene::elements (scene.rs:23-31 tests them in that order and the EARLIER element wins a tie in distance):
     * NULL = all spheres, then all triangles; else n_spheres + n_triangles entries, entry k = the k-th element:
     * bit 31 clear -> spheres[entry], bit 31 set -> triangles[entry & 0x7fffffff]; every object exactly once.
     * Object ids (rbrt_hip_trace_rays) follow this order: element k has id k, mesh m has id n_spheres + n_triangles + m. */
    const uint32_t* element_order;
} rbrt_scene_t;

/* Smooth shading of meshes (no counterpart in the reference, which shades every mesh hit with the stored face normal,
 * mesh.rs:253-257). A mesh can carry three corner normals per SoA entry: n0, n1, n2, at vertices[0], v0 + e1 and v0 + e2.
 * When the closest hit of a ray (o, d) -- the ray as it was traced for that segment -- is entry i of such a mesh,
 * scatter uses the shading normal n_s in place of the stored face normal, in float32, unfused, in this order:
 *     h = d x e2;  a = e1 . h;  f = 1 / a;  s = o - v0;  u = f (s . h)
 *     q = s x e1;  v = f (d . q)                  (x and . in the reference's order: dot = (x + y) + z)
 *     w = (1 - u) - v
 *     m_c = ((w n0_c) + (u n1_c)) + (v n2_c)      per component c
 *     n_s = normalize(m)                          (three divisions by the length)
 *     if m's length is 0 or n_s is not finite: n_s = the stored face normal of entry i
 * u and v are exactly those of the Moller-Trumbore test that made entry i the closest hit (triangle.rs:189-255). There is
 * no clamping, and n_s is not flipped towards the ray. Lambertian, metal and dielectric then run unchanged, with n_s
 * where they read the normal. Nothing else changes: spheres, BasicTriangles and meshes without normals, the random
 * stream and its draw order, emitters, what is hit (the BVH and the tile pass), the counters. A scene where no mesh
 * carries normals renders exactly as it does through rbrt_hip_scene_create / rbrt_hip_render. */
typedef struct rbrt_mesh_normals {
    /* corner normals of every SoA entry, n_total each (padding entries included); all nine NULL = the mesh is flat.
     * They need not have unit length. */
    const float *n0x, *n0y, *n0z;
    const float *n1x, *n1y, *n1z;
    const float *n2x, *n2y, *n2z;
} rbrt_mesh_normals_t;

typedef struct rbrt_scene_shading {
    uint32_t n_meshes;                  /* == scene->n_meshes */
    uint32_t reserved;                  /* 0 */
    const rbrt_mesh_normals_t* meshes;  /* [n_meshes], the scene's mesh order; NULL = every mesh flat */
} rbrt_scene_shading_t;

/* Solid patterns (no counterpart in the reference, where an object has one albedo). An object whose material is
 * RBRT_MAT_LAMBERTIAN may carry a 3-D checker in world space: two albedos, chosen by the cell the hit point lies in. When
 * scatter runs at the hit point p = o + t d of such an object (the point it scatters from anyway), in float32, unfused, in
 * this order, with inv = 1.0f / size computed once on the host, per component c:
 *     t_c = (p_c - origin_c) * inv
 *     u_c = min(max(t_c, -1e9f), 1e9f)        (fmaxf, fminf: the other operand when one is NaN, so a NaN counts as -1e9)
 *     k_c = int32(floor(u_c))
 *     odd = (k_x ^ k_y ^ k_z) & 1             (an xor of parities cannot overflow where a sum could)
 * A hit in an odd cell attenuates the path with albedo2, a hit in an even cell with the material's albedo. Nothing else
 * changes: the scatter direction and its draws, what is hit (the BVH, the tile pass), the order of the fold, the counters,
 * emitters, the lens, smooth shading, the environment. A scene without patterns renders bit for bit as it does through
 * the other entry points; a pattern whose albedo2 equals the material's albedo renders bit for bit as the scene without it.
 * The feature buffers' albedo (rbrt_hip_render_features) is the cell's colour, sample by sample. */
#define RBRT_PATTERN_NONE 0u
#define RBRT_PATTERN_CHECKER 1u
typedef struct rbrt_pattern {      /* 32 bytes */
    uint32_t kind;                 /* RBRT_PATTERN_* */
    float albedo2[3];              /* the odd cells' albedo; the even cells have the material's own */
    float origin[3];
    float size;                    /* a cell's edge, world units */
} rbrt_pattern_t;
typedef struct rbrt_scene_patterns {
    uint32_t n_objects;            /* == n_spheres + n_triangles + n_meshes */
    uint32_t reserved;             /* 0 */
    const rbrt_pattern_t* objects; /* [n_objects], by object id (rbrt_scene_t's numbering); NULL = none */
} rbrt_scene_patterns_t;

/* The 8 of Camera's 14 fields (cam.rs:4-19) that get_ray_through_pixel (cam.rs:64-82) reads. */
typedef struct rbrt_camera {
    float position[3];
    float right[3];
    float up[3]; /* raw YAML vector, not normalised (cam.rs:55,75) */
    float img_center_point[3];
    float mm_per_pix_hor;
    float mm_per_pix_vert;
    uint32_t img_width_pix;
    uint32_t img_height_pix;
} rbrt_camera_t;

/* Values the reference hard-codes are fields here with those defaults
 * (rbrt_render_opts_default): max depth 50 (lib.rs:99), min/max dist
 * (lib.rs:44-45), background (lib.rs:89-93). `seed` replaces the reference's
 * OS-seeded rand::random (cam.rs:69,71; materials.rs:17-19; dielectric.rs:48):
 * the random stream of sample s of pixel (row, col) is a pure function of
 * (seed, row*W+col, s), consumed in the reference's draw order. */
typedef struct rbrt_render_opts {
    uint32_t spp;       /* num_samples */
    uint32_t max_depth; /* 50 */
    float min_dist;     /* 0.001 */
    float max_dist;     /* 2000.0 */
    float bg[3];        /* (0.05, 0.05, 0.8) */
    uint64_t seed;
    /* pixel-tile sharding for multi-GPU: 8x8 tiles are dealt round-robin by tile NUMBER ("How tiles are
     * dealt to ranks", below), this call renders the tiles numbered t with t % tile_world == tile_rank.
     * tile_world <= 1 renders the whole image. */
    uint32_t tile_rank;
    uint32_t tile_world;
    uint32_t flags;     /* RBRT_FLAG_* */
    uint32_t reserved;
} rbrt_render_opts_t;

#define RBRT_FLAG_NONE 0u
#define RBRT_FLAG_COLLECT_STATS 1u /* run the counting variant of the kernel (slower); see rbrt_hip_stats_t */
/* A ray that hits nothing returns `bg` exactly, instead of the reference's sky gradient t*(1,1,1) + (1-t)*bg
 * (lib.rs:68-71), which is white at the zenith whatever bg is. For dark scenes lit by RBRT_MAT_EMISSIVE objects.
 * Honoured by rbrt_hip_render, _render_device and _render_pass; every pass of one rbrt_hip_render_pass series must use
 * the same flag and bg, as it must use the same seed -- and the same environment (rbrt_hip_scene_set_environment), which
 * takes the place of both while the handle has one. */
#define RBRT_FLAG_CONSTANT_BACKGROUND 2u
/* A thin lens (no counterpart in the reference, whose cam.rs:64-82 starts every ray at the position): camera rays start on
 * an elliptic disc around the position and all rays through one point of the image plane meet on the focus surface,
 * which gives defocus blur. With the flag, the `cam` argument of rbrt_hip_render, _render_device and _render_pass must
 * point at the `cam` member of an rbrt_camera_lens_t (below); without it nothing past rbrt_camera_t is ever read.
 * Every pass of one rbrt_hip_render_pass series must use the same flag and lens, as it must use the same seed.
 * A library that does not list the bit in rbrt_hip_supported_flags() ignores it: ask before relying on it. */
#define RBRT_FLAG_THIN_LENS 4u

/* The lens of a RBRT_FLAG_THIN_LENS render. The random stream of a sample, after the column and row jitter draws that
 * place the pinhole target T on the image plane (cam.rs:70-75), draws lens points in float32, unfused, in this order:
 *     repeat  lx = 2 u - 1; ly = 2 u - 1      (u: the next draws of the sample's stream, x first)
 *     until   lx lx + ly ly < 1               ((lx lx) + (ly ly), strict)
 *     o = position + (lx lens_u + ly lens_v)  (per component (lx u_c) + (ly v_c), then the sum)
 *     F = position + focus_scale (T - position)
 *     d = normalize(F - o)                    (three divisions by the length)
 * and the bounce draws follow. An all-zero lens still draws. rbrt_hip_render, _render_device and _render_pass reject a
 * non-finite lens_u or lens_v, a focus_scale that is not finite and > 0, or a non-zero `reserved` with
 * RBRT_ERR_INVALID_ARG before the device is touched. */
typedef struct rbrt_camera_lens {
    rbrt_camera_t cam;  /* first member: &lens.cam is what every render entry point receives */
    float lens_u[3];    /* lens half-axes in scene units (the aperture radius already applied) */
    float lens_v[3];
    float focus_scale;  /* focus surface = the image plane scaled about cam.position by this factor */
    uint32_t reserved;  /* 0 */
} rbrt_camera_lens_t;

#define RBRT_TILE 8u /* tile edge in pixels used for sharding and work ordering */
/* How tiles are dealt to ranks. Tile NUMBER t (0 <= t < tiles_x * tiles_y) belongs to rank t % tile_world, and a rank's packed
 * buffers hold its tiles in ascending number. Number t is the image tile in tile row ty = t / tiles_x at tile column
 * tx = (t % tiles_x + RBRT_TILE_SKEW * ty) % tiles_x: every tile row is rotated by RBRT_TILE_SKEW more than the one above, so
 * that a rank's tiles lie on skew lines through the image and not in fixed tile columns (with 8 ranks and a width of 128 or
 * 240 tiles a rank owned every 8th COLUMN, and the columns over the mesh made two ranks 5 % slower than the mean at
 * 1920 x 1080). rbrt_hip_unpack_tiles undoes it; rbrt_hip_tile_xy / rbrt_hip_tile_number (below) are the two directions for a
 * host that does its own gather. The image does not depend on the dealing. */
#define RBRT_TILE_SKEW 3u

/* Per-render work counters from the counting kernel variant: the inputs of the
 * algorithmic-bytes figure ("Measurement"). */
typedef struct rbrt_hip_stats {
    uint64_t rays;            /* Scene::hit calls (scene.rs:19) */
    uint64_t mesh_gate_pass;  /* rays x meshes that passed BoundingBox::hit (aabbox.rs:28-58) */
    uint64_t nodes_visited;   /* BVH node records fetched */
    uint64_t tris_tested;     /* Moller-Trumbore evaluations (triangle.rs:189-255 per lane) */
    uint64_t mesh_hits;       /* accepted mesh hits (normal fetch, mesh.rs:253-257) */
    uint64_t samples;         /* paths traced */
    uint64_t nan_discriminants; /* sphere.rs:33 would have panicked */
    uint32_t node_bytes;      /* size of one BVH node record */
    uint32_t tri_bytes;       /* size of one device triangle record */
} rbrt_hip_stats_t;

typedef struct rbrt_hip_scene rbrt_hip_scene_t; /* opaque: device-resident scene + BVH + workspace */

/* ---- one-shot convenience: the closest analogue of lib.rs:75-79 --------------------------- */

/* Renders the whole image (tile_world ignored unless > 1, then only this rank's tiles are
 * written and all other pixels are left untouched). out_radiance and out_rgb8 are HOST buffers of
 * H*W*3 elements; either may be NULL. The one-shot calls (this one, _render_shaded and _render_patterned) have no
 * shutter ("Camera shutter", below): the scene they make lives for the call only and nothing can set one on it. */
int rbrt_hip_render(const rbrt_camera_t* cam, const rbrt_scene_t* scene,
                    const rbrt_render_opts_t* opts, float* out_radiance, uint8_t* out_rgb8);
/* The same with smooth meshes (rbrt_hip_scene_create_shaded's checks); shading = NULL is rbrt_hip_render. */
int rbrt_hip_render_shaded(const rbrt_camera_t* cam, const rbrt_scene_t* scene, const rbrt_scene_shading_t* shading,
                           const rbrt_render_opts_t* opts, float* out_radiance, uint8_t* out_rgb8);
/* ... and with solid patterns (rbrt_hip_scene_create_patterned's checks); patterns = NULL is rbrt_hip_render_shaded. */
int rbrt_hip_render_patterned(const rbrt_camera_t* cam, const rbrt_scene_t* scene, const rbrt_scene_shading_t* shading,
                              const rbrt_scene_patterns_t* patterns, const rbrt_render_opts_t* opts, float* out_radiance,
                              uint8_t* out_rgb8);

/* ---- resident scene: upload + BVH build once, render many times --------------------------- */

int rbrt_hip_scene_create(const rbrt_scene_t* scene, int device, rbrt_hip_scene_t** out);
int rbrt_hip_scene_destroy(rbrt_hip_scene_t* scene);
/* rbrt_hip_scene_create with the corner normals of smooth meshes (rbrt_scene_shading_t above). shading = NULL behaves
 * exactly like rbrt_hip_scene_create. RBRT_ERR_INVALID_ARG, before the device is touched: shading->n_meshes !=
 * scene->n_meshes, reserved != 0, some but not all of a mesh's nine pointers NULL, or a non-finite component (padding
 * entries included). rbrt_hip_render_device and rbrt_hip_render_pass need nothing more on a handle made this way. */
int rbrt_hip_scene_create_shaded(const rbrt_scene_t* scene, const rbrt_scene_shading_t* shading, int device,
                                 rbrt_hip_scene_t** out);
/* rbrt_hip_scene_create_shaded with solid patterns (rbrt_scene_patterns_t above). patterns = NULL, or objects = NULL, or
 * every kind RBRT_PATTERN_NONE behaves exactly like rbrt_hip_scene_create_shaded: the same image, the same LDS per wave.
 * There is no flag bit: a host detects the capability by this symbol. The handle keeps its patterns for its lifetime and
 * every render call on it honours them. Before the device is touched, RBRT_ERR_INVALID_ARG: patterns->n_objects differs
 * from the scene's object count, reserved != 0, an unknown kind, a checker on an object that is not RBRT_MAT_LAMBERTIAN, a
 * size that is not finite or <= 0 or whose 1.0f / size is not finite, a non-finite origin, a non-finite or negative
 * albedo2 component. RBRT_ERR_UNSUPPORTED: more than 256 objects and patterned objects together (a path records one byte
 * per bounce, and a patterned object takes a second value of that byte for its odd cells; the scene's own limit of 255
 * objects stands). */
int rbrt_hip_scene_create_patterned(const rbrt_scene_t* scene, const rbrt_scene_shading_t* shading,
                                    const rbrt_scene_patterns_t* patterns, int device, rbrt_hip_scene_t** out);

/* Number of pixels this rank owns for a W x H image under (tile_rank, tile_world), counting
 * the padded pixels of partial edge tiles (each tile contributes RBRT_TILE*RBRT_TILE slots). */
size_t rbrt_hip_packed_pixels(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_world);

/* Tile number -> tile row / column and back ("How tiles are dealt to ranks", above); tiles_x = ceil(width / RBRT_TILE). */
void rbrt_hip_tile_xy(uint32_t tile, uint32_t tiles_x, uint32_t* tile_row, uint32_t* tile_col);
uint32_t rbrt_hip_tile_number(uint32_t tile_row, uint32_t tile_col, uint32_t tiles_x);

/* Renders into DEVICE memory on `stream` (a hipStream_t, may be NULL = default stream) and
 * returns without synchronising.
 * Threading rule: a scene handle is used by ONE host thread at a time and all its render_device calls go to the
 * SAME stream (the handle's accumulator, its pipeline lanes and their events are ordered through that stream);
 * use one handle per stream / thread otherwise (the reference's render_scene is not re-entrant either: it takes
 * Scene by value, lib.rs:75-79).
 *   d_radiance: if tile_world <= 1: float[H][W][3] row-major.
 *               else: this rank's tiles packed, float[n_local_tiles][64][3] (tile-local pixel
 *               p = (y%8)*8 + (x%8)); feed the gathered buffers to rbrt_hip_unpack_tiles.
 *   d_rgb8    : same indexing with uint8 elements; may be NULL. d_radiance may be NULL too. */
int rbrt_hip_render_device(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam,
                           const rbrt_render_opts_t* opts, void* stream, float* d_radiance,
                           uint8_t* d_rgb8);

/* Progressive / checkpointed rendering (no counterpart in the reference, whose sample loop lib.rs:95-101 runs to the
 * end or not at all; a 4096 x 4096 x 4096 spp render is 68.7 G paths). Renders samples [sample_begin, sample_end) of
 * the opts->spp samples of every pixel and adds them, in sample order, to the running sums in d_accum (device, fp32,
 * ALWAYS in the rank's packed tile order, tile_world <= 1 included: rbrt_hip_packed_pixels(...) * 3 floats, which is more
 * than H*W*3 when the image has ragged edge tiles; read unless sample_begin == 0). The call with sample_end == opts->spp also
 * writes the mean to d_radiance and its quantisation to d_rgb8 (either may be NULL). Calls must cover [0, spp) in
 * ascending, non-overlapping ranges; the final image is then bit-identical to one rbrt_hip_render_device call,
 * because the per-pixel additions happen in the same order. A checkpoint is d_accum plus sample_end. Every pass of one
 * series must use the same seed, lens, shutter and motion (rbrt_hip_scene_set_shutter, rbrt_hip_scene_set_motion: do not call
 * them between two passes). */
int rbrt_hip_render_pass(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, const rbrt_render_opts_t* opts,
                         void* stream, uint32_t sample_begin, uint32_t sample_end, float* d_accum,
                         float* d_radiance, uint8_t* d_rgb8);

/* ---- Adaptive sampling: tiles stop once their noise estimate converges -----------------------------------------------
 * No counterpart in the reference, which gives every pixel num_samples samples (lib.rs:95-101). opts->spp becomes the upper
 * limit N; each 8x8 tile is sampled in rounds until the estimate of its error falls below `threshold`. The random stream
 * of a sample does not depend on spp and a pixel's samples are added in sample order, so a tile that stops after n samples
 * is bit for bit the tile of rbrt_hip_render_device at spp = n.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; division and sqrt are correctly rounded.
 *   Rounds.  n_0 = min(min_samples, N), n_{k+1} = min(n_k + step, N). Every tile of the rank starts active with count 0.
 *     Round k renders samples [n_{k-1}, n_k) (round 0: [0, n_0)) of every tile that is active at its start. Each pixel's
 *     samples are added in sample order to two running sums: S gets every sample, S_even those with an even index.
 *     After the round each tile that was active sets its count n_t = n_k and computes its error E. It stays active iff
 *     n_k < N and not (E < threshold): a NaN keeps sampling, threshold = 0 stops nothing early. The call ends when no tile
 *     is active.
 *   Tile error after n samples, with h = (n + 1) / 2 (integer), inv_n = 1.0f / float(n), inv_h = 1.0f / float(h):
 *     per pixel p of the tile (p = (y % 8) * 8 + (x % 8)), per channel c:
 *         I_c = S_c * inv_n        A_c = S_even_c * inv_h
 *     e_p = (|I_r - A_r| + |I_g - A_g|) + |I_b - A_b|
 *     q_p = e_p / (sqrt((I_r + I_g) + I_b) + 0.0001f)
 *     a pixel beyond a ragged image edge has q_p = 0
 *     v = q;  for d in 1, 2, 4, 8, 16, 32:  v[p] = v[p] + v[p ^ d]     (all 64 at once; every p ends with the same bits)
 *     E = v / float(number of the tile's pixels inside the image)
 *     (the half-buffer estimate of Dammertz et al.: the image of all samples against the image of every other one)
 *   Image.  A pixel of a tile with count n_t is S * (1.0f / float(n_t)), then the usual quantisation. A tile with
 *     n_t == N is exactly what rbrt_hip_render_device writes; any tile is exactly the fixed render at spp = n_t. */
typedef struct rbrt_adaptive_opts {
    float threshold;      /* finite, >= 0 */
    uint32_t min_samples; /* >= 2 */
    uint32_t step;        /* >= 1 */
    uint32_t reserved;    /* 0 */
} rbrt_adaptive_opts_t;

typedef struct rbrt_adaptive_result {
    uint32_t rounds, reserved;
    uint64_t samples;        /* sum over the rank's pixels inside the image of their tile's count */
    uint64_t samples_fixed;  /* the same at spp everywhere */
} rbrt_adaptive_result_t;

/* Renders adaptively into DEVICE memory on `stream`. UNLIKE rbrt_hip_render_device THIS CALL BLOCKS: it reads the number of
 * active tiles back once per round, and all its outputs are complete when it returns. The threading rule of
 * rbrt_hip_render_device holds.
 *   d_radiance, d_rgb8: indexed as in rbrt_hip_render_device (packed when tile_world > 1).
 *   d_tile_samples, d_tile_error: [n_local_tiles] in the rank's ascending tile number (number -> image tile:
 *     rbrt_hip_tile_xy): the tile's final count and the last error computed for it.
 *   out: the call's totals. Every output pointer may be NULL.
 * Honours the thin lens, the constant background, smooth handles and tile_rank / tile_world. rbrt_hip_scene_check works
 * after it as after any render. The running sums and tile tables belong to the handle (grown on demand, released by
 * rbrt_hip_scene_destroy). The call's trace launches get no helper launches (rbrt_hip_debug.h RBRT_HELPERS).
 * RBRT_ERR_INVALID_ARG, before the device is touched: scene, cam, opts or adaptive NULL; adaptive->reserved != 0; a
 * threshold that is not finite or negative; min_samples < 2; step == 0; RBRT_FLAG_COLLECT_STATS set (counting stays with
 * the fixed paths); and whatever rbrt_hip_render_device rejects. */
int rbrt_hip_render_adaptive(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, const rbrt_render_opts_t* opts,
                             const rbrt_adaptive_opts_t* adaptive, void* stream, float* d_radiance, uint8_t* d_rgb8,
                             uint32_t* d_tile_samples, float* d_tile_error, rbrt_adaptive_result_t* out);

/* ---- Denoising: a dual-buffer non-local-means filter on the adaptive half sums -------------------------------------------
 * No counterpart in the reference. The filter of Rousselle, Knaus and Zwicker (2012) for images without feature buffers: the
 * image of the samples with an even index is filtered with weights taken from the image of the odd ones and the other way
 * round (weights taken from the same noise would reinforce it), and the two results are mixed by their sample shares.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; division and sqrt are correctly rounded. "Inside" means
 * inside the W x H image; a sum "from 0" starts at 0.0f and adds its terms one at a time in the stated order.
 *   Inputs.  Two half images A and B, float[H][W][3]; a per-pixel mix wa, float[H][W], the share of A; window_radius R,
 *     patch_radius P, strength k. eps = 1e-7f, k2 = k * k.
 *   Variance.  d_c[p] = (A_c[p] - B_c[p]) squared.  V_c[p] = (sum / float(count)) * 0.5f, where sum runs over the 3 x 3
 *     neighbourhood of p (dy outer -1..1, dx inner -1..1, from 0) of d_c, only pixels inside are added and count is how many.
 *   Pixel distance, for a guide image G, a pixel p and an offset o = (dy, dx), q = p + o: delta(p, o) = 0 if p or q is
 *     outside, else per channel
 *         t_c = (((G_c[q] - G_c[p]) squared) - (V_c[p] + min(V_c[p], V_c[q]))) / (eps + k2 * (V_c[p] + V_c[q]))
 *     and delta = (t_r + t_g) + t_b.
 *   Patch distance.  r_j = sum from 0 over i = -P..P, left to right, of delta(p + (j, i), o);  D = sum from 0 over
 *     j = -P..P, top to bottom, of r_j;  D = D / float(3 * cy * cx), where cy * cx is the number of patch positions at which
 *     both p + (j, i) and p + (j, i) + o are inside (both conditions are rectangles: the count is a product). Rows first,
 *     columns second, both orders fixed: a kernel may share row sums between pixels; a sliding-window update is not the rule.
 *   Weight.  t = max(0, 1 - 0.25f * max(D, 0)),  w = (t * t) * (t * t): the fourth power of a truncated line, which follows
 *     e^-D and has support up to D = 4 (exp has no correctly rounded form on both sides of a test). At o = 0 every delta
 *     is <= 0, so w = 1 exactly.
 *   Filter.  filter(F, G)[p]_c = num_c / den, num_c = sum from 0 of w(p, o) * F_c[p + o], den = sum from 0 of w(p, o), both
 *     over the window with dy outer -R..R and dx inner -R..R; offsets whose q is outside are skipped.
 *   Output.  Ah = filter(A, guide B), Bh = filter(B, guide A), out_c = (Ah_c * wa) + (Bh_c * (1 - wa)), then the usual
 *     quantisation for rgb8. With R = 0 the output is exactly (A * wa) + (B * (1 - wa)).
 *   From a handle's sums, for a tile with count n, h = (n + 1) / 2 (integer), g = n - h:
 *     A = S_even * (1.0f / float(h)),  B = (S - S_even) * (1.0f / float(g)),  wa = float(h) * (1.0f / float(n)).
 * Finite inputs with |x| <= 1e6 give no NaN. A non-finite input pixel gives unspecified values in the pixels whose window
 * holds it; it never faults. */
typedef struct rbrt_denoise_opts {
    uint32_t window_radius; /* R, 0..10 */
    uint32_t patch_radius;  /* P, 0..4 */
    float strength;         /* k, finite, > 0 */
    uint32_t reserved;      /* 0 */
} rbrt_denoise_opts_t;
void rbrt_denoise_opts_default(rbrt_denoise_opts_t* opts); /* R = 5, P = 3, k = 0.7 */

/* The filter on two half images in DEVICE memory (row-major float[H][W][3]; d_wa row-major float[H][W], NULL: 0.5
 * everywhere). Needs no scene, like rbrt_hip_unpack_tiles. Writes the row-major result to d_radiance and / or its quantisation
 * to d_rgb8 (either may be NULL). Asynchronous on `stream`. The call owns no device memory: the variance and everything else
 * the kernel stages live in the kernel's LDS, so calls on different streams share nothing.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_a, d_b or opts NULL; opts->reserved != 0; window_radius > 10;
 * patch_radius > 4; a strength that is not finite or <= 0; width or height 0. */
int rbrt_hip_denoise_halves(int device, void* stream, const float* d_a, const float* d_b, const float* d_wa,
                            uint32_t width, uint32_t height, const rbrt_denoise_opts_t* opts,
                            float* d_radiance, uint8_t* d_rgb8);

/* Denoises the image of the handle's last rbrt_hip_render_adaptive call, from that call's S, S_even and tile counts (the
 * handle remembers its width, height and tile_world). d_radiance, d_rgb8: row-major, as rbrt_hip_render_device's; d_half_a,
 * d_half_b: the two half images A and B the filter worked on, float[H][W][3]. Every output may be NULL. Asynchronous on
 * `stream`; the half images between the two kernels are the handle's memory (grown on demand, released by
 * rbrt_hip_scene_destroy), so the threading rule of rbrt_hip_render_device holds. A fixed render or another denoise call in
 * between changes nothing; the next adaptive call replaces the image.
 * A rank lacks its neighbours' pixels: multi-rank denoising is out of scope (gather, rbrt_hip_unpack_tiles and
 * rbrt_hip_denoise_halves on halves of one's own is the way).
 * RBRT_ERR_INVALID_ARG, before the device is touched: scene or opts NULL; what rbrt_hip_denoise_halves refuses in opts; no
 * adaptive render on the handle yet; the last one had opts->spp < 2 (a half would be empty).
 * RBRT_ERR_UNSUPPORTED: the last adaptive render had tile_world > 1. */
int rbrt_hip_scene_denoise(rbrt_hip_scene_t* scene, const rbrt_denoise_opts_t* opts, void* stream,
                           float* d_radiance, uint8_t* d_rgb8, float* d_half_a, float* d_half_b);

/* ---- Environment lighting: an octahedral radiance map for the rays that hit nothing ---------------------------------------
 * No counterpart in the reference, whose rays that hit nothing see the sky gradient (lib.rs:68-71). An environment of size N
 * (1 <= N <= 4096) is a square grid of (N + 1) x (N + 1) NODES E[j][i], j the row, each a linear RGB radiance. The nodes are
 * the corners of N x N cells, so the bilinear interpolation never reads outside the grid; the octahedral fold identifies the
 * boundary nodes that belong to the same direction (E[0][i] and E[0][N - i], E[N][i] and E[N][N - i], E[j][0] and E[N - j][0],
 * E[j][N] and E[N - j][N]: a map that is to be continuous holds equal values there). +y is up, as in the sky gradient.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / is correctly rounded. For the direction d of the ray
 * that hit nothing, as it was traced and not re-normalised:
 *     s  = (|dx| + |dy|) + |dz|
 *     px = dx / s;  py = dy / s;  pz = dz / s
 *     if py >= 0:  u = px;  v = pz
 *     else:        u = (1 - |pz|) * (px >= 0 ? 1 : -1);   v = (1 - |px|) * (pz >= 0 ? 1 : -1)
 *     x  = ((u * 0.5f) + 0.5f) * float(N);    y = ((v * 0.5f) + 0.5f) * float(N)
 *     i  = x >= 0 ? min(uint(floor(x)), N - 1) : 0      (a NaN compares false: i = 0);   j likewise from y
 *     fx = x - float(i);   fy = y - float(j)
 *     per channel c:
 *       top = E[j][i]   + fx * (E[j][i+1]   - E[j][i])
 *       bot = E[j+1][i] + fx * (E[j+1][i+1] - E[j+1][i])
 *       L_c = top + fy * (bot - top)
 * L takes the place of the background: colorize returns it for the ray that hit nothing (the path's fold a1 * (a2 * (... * L))
 * starts from it), in the trace kernel and in the kernels that finish background-only tiles alike. The a + f * (b - a) form
 * makes a constant map return its constant exactly. For every finite non-zero direction i and j stay in [0, N - 1] and fx, fy
 * in [0, 1]. Whatever d is, i and j stay in [0, N - 1] (a NaN compares false), so no read is ever outside the map; a NaN or
 * zero direction gives a NaN colour (an infinite component gives a NaN colour or, where the rule's quotients are 0, a node's).
 *
 * The environment is a STATE OF THE HANDLE. While one is set, every render on the handle uses it for the rays that hit nothing
 * -- rbrt_hip_render_device, _render_pass, _render_adaptive and through that rbrt_hip_scene_denoise -- and opts->bg and
 * RBRT_FLAG_CONSTANT_BACKGROUND are ignored. Every pass of one rbrt_hip_render_pass series must use the same environment, as
 * it must use the same seed, flag and bg. There is no flag bit: a host detects the capability by the symbol. The one-shot
 * rbrt_hip_render and rbrt_hip_trace_rays have no environment. Nothing else changes: what is hit, the random streams, the
 * scatter records, the tile pass, the order of the sums, the counters. */
typedef struct rbrt_environment {
    uint32_t n;         /* N, 1..4096 */
    uint32_t reserved;  /* 0 */
    const float* nodes; /* HOST, float[n+1][n+1][3], row j first; finite, >= 0 */
} rbrt_environment_t;

/* Sets, replaces (env != NULL) or clears (env == NULL: back to opts->bg) the handle's environment. THIS CALL BLOCKS: it waits for
 * the handle's outstanding work, copies the nodes to device memory the handle owns (16 bytes per node; released when the map
 * is replaced or cleared and by rbrt_hip_scene_destroy) and returns with the map in place. The threading rule of
 * rbrt_hip_render_device holds.
 * RBRT_ERR_INVALID_ARG, before the device is touched, the handle keeping the map it had: scene NULL; n == 0 or n > 4096;
 * reserved != 0; nodes NULL; a non-finite or negative component. */
int rbrt_hip_scene_set_environment(rbrt_hip_scene_t* scene, const rbrt_environment_t* env);

/* ---- Camera shutter: motion blur of a translating camera ------------------------------------------------------------------------
 * No counterpart in the reference, whose camera is exposed for an instant. A handle may carry a shutter: the vector `travel`
 * (scene units), the translation of the whole camera -- position and image plane alike -- between the opening and the closing
 * of the shutter. The `cam` of a render is the camera at the opening.
 *
 * The rule. For every sample of a render on such a handle the origin o and the direction d are made exactly as without a
 * shutter: after the jitter draws, after the lens draws when RBRT_FLAG_THIN_LENS is set, with d = normalize(F - o) computed.
 * Then, in float32, unfused:
 *     t   = the next draw of the sample's stream            (u in [0, 1))
 *     o_c = o_c + (t * travel_c)                            for c = x, y, z
 * and the bounce draws follow. d is NOT recomputed: a translation does not turn a ray, so d keeps the bits it has without a
 * shutter. A zero travel still draws (as an all-zero lens does): its image is not the shutterless one. A handle without a
 * shutter draws nothing and renders bit for bit what it renders without this section. A ray that hits nothing returns a
 * colour that depends on d only (the background, the gradient, the environment): the pixels of background-only tiles are what
 * they are without a shutter, and the kernels that finish them make no draw for it. Everything that reads the origin reads
 * the shifted one: the hit tests, the hit point p = o + t d of a pattern, the shading normal of a smooth mesh, the sphere normal.
 *
 * The shutter is a STATE OF THE HANDLE, like the environment. While one is set, rbrt_hip_render_device, _render_pass,
 * _render_adaptive (and through it rbrt_hip_scene_denoise) and rbrt_hip_render_features honour it, with and without a lens,
 * for every tile_rank / tile_world; the feature buffers trace the render's own camera rays, the shutter draw included. Every
 * pass of one rbrt_hip_render_pass series must use the same shutter, as it must use the same seed and lens. There is no flag
 * bit: a host detects the capability by the symbol. The one-shot rbrt_hip_render, rbrt_hip_render_shaded and
 * rbrt_hip_render_patterned and rbrt_hip_trace_rays have no shutter. The tile pass widens its margins by |travel| (tables made
 * for one travel never serve another); a travel longer than the distance to everything in the scene culls nothing. */
typedef struct rbrt_shutter {
    float travel[3];   /* scene units; finite */
    uint32_t reserved; /* 0 */
} rbrt_shutter_t;

/* Sets, replaces (shutter != NULL) or clears (shutter == NULL: no shutter) the handle's shutter. Nothing is copied to the
 * device: the travel goes with the launches issued after the call, launches in flight keep theirs. The threading rule of
 * rbrt_hip_render_device holds.
 * RBRT_ERR_INVALID_ARG, before the device is touched, the handle keeping the shutter it had: scene NULL; a travel that is not
 * finite; reserved != 0. */
int rbrt_hip_scene_set_shutter(rbrt_hip_scene_t* scene, const rbrt_shutter_t* shutter);

/* ---- Moving spheres: object motion blur on the shutter's time draw -------------------------------------------------------------
 * No counterpart in the reference. A handle may carry a motion: one vector travel_i (scene units) per sphere of the scene, the
 * sphere's translation between the opening and the closing of the shutter. The sphere's `center` in the scene is its position
 * at the opening.
 *
 * The draw. A sample's ray (o, d) is made exactly as without a motion: jitter, lens draws, d = normalize(F - o). If the handle
 * has a shutter OR a motion, the next draw of the stream is t (u in [0, 1)): ONE draw for both, because camera and objects
 * share one exposure. With a shutter, o += t * travel as in "Camera shutter". With a motion, t belongs to the sample for its
 * whole path. A handle with a shutter and no motion renders bit for bit what it renders without this section; so does a
 * handle with neither. A motion whose vectors are all zero still draws: its image is that of a zero-travel shutter.
 *
 * The sphere. Wherever a path of that sample reads sphere i's centre, it reads, in float32, unfused, a product and a sum per
 * component,
 *     c_i(t)_c = center_i_c + (t * travel_i_c)                 for c = x, y, z
 * in the hit test of every ray of the path, camera ray and bounces alike, and in the normal p - c_i(t). The radius, the
 * materials, meshes, BasicTriangle elements, the background and the environment do not move. A solid checker
 * (rbrt_scene_patterns_t) is a pattern of world space and stays where it is: the surface of a moving sphere moves through it.
 *
 * The motion is a STATE OF THE HANDLE, like the shutter. While one is set, rbrt_hip_render_device, _render_pass,
 * _render_adaptive (and the denoisers that read its halves) and rbrt_hip_render_features (the depth and the normal of the
 * moved sphere) honour it, for every tile_rank / tile_world, in helper launches and in the short-path stage. Every pass of one
 * rbrt_hip_render_pass series must use the same motion. rbrt_hip_trace_rays and the ray hooks have no sample stream and see
 * the spheres at their opening positions, as they see no shutter. The one-shot rbrt_hip_render* calls cannot carry a motion,
 * for the reason they cannot carry a shutter. There is no flag bit and the ABI version stays 2: a host detects the capability
 * by the symbol. The tile pass widens sphere i's margins by |travel_i| (kernels.hip primary_cull_kernel, "Moving spheres");
 * a scene with a motion never runs the trace kernel's plain build. Not built: moving BasicTriangles, rotation or
 * other paths than a straight line, a pattern that travels with its sphere, a time argument for rbrt_hip_trace_rays. (Spheres
 * that advance between the frames of a stream, and their travel as a feature buffer: "Animation", below.) */
typedef struct rbrt_motion {
    uint32_t n_spheres;  /* the scene's sphere count */
    uint32_t reserved;   /* 0 */
    const float* travel; /* [n_spheres][3], in the order of rbrt_scene_t::spheres; scene units; finite */
} rbrt_motion_t;

/* Sets, replaces (motion != NULL) or clears (motion == NULL: no motion) the handle's motion. The vectors are copied: the call
 * waits for the handle's launches in flight and puts them on the device. The threading rule of rbrt_hip_render_device holds.
 * RBRT_ERR_INVALID_ARG, before the device is touched, the handle keeping the motion it had: scene NULL; n_spheres other than
 * the scene's sphere count; reserved != 0; travel NULL with n_spheres > 0; a component that is not finite; a
 * center + travel that is not finite in float32. */
int rbrt_hip_scene_set_motion(rbrt_hip_scene_t* scene, const rbrt_motion_t* motion);

/* ---- Display transform: exposure, automatic exposure and tone mapping --------------------------------------------------------
 * No counterpart in the reference, whose only way from radiance to a picture is the quantisation (sqrt(c) * 256) as u8
 * (lib.rs:116-122): everything above 1.0 clips. The transform is a stage behind the image, like the denoiser: it reads n pixels
 * X (RGB, linear radiance; the layout does not matter) and writes the transformed radiance and / or its quantisation.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / is correctly rounded; a constant is the float32 nearest
 * to the decimal written.
 *   Luminance of a colour c.  Y(c) = ((0.2126f * c_r) + (0.7152f * c_g)) + (0.0722f * c_b)
 *   Histogram.  Made only when the exposure or the white point is automatic. A pixel is COUNTED iff the bits u of Y(X) satisfy
 *     0x00800000 <= u <= 0x7F7FFFFF: a positive, normal, finite value. Zeros, denormals, negatives, infinities and NaN are
 *     left out, and with them the zero padding of a packed tile buffer. A counted pixel's bin is u >> 19: 8 exponent bits and
 *     4 mantissa bits, RBRT_TONEMAP_BINS = 4096 bins, each 2^(1/16) wide -- a logarithmic scale without a logarithm. M is the
 *     number of counted pixels. The counts are integers: they do not depend on the order the pixels are visited in.
 *   Rank pick, for a permille q in 0..1000.  k = ((M - 1) * q) / 1000 in 64-bit integers; b_q is the smallest bin with
 *     hist[0] + ... + hist[b_q] > k; L_q is the float whose bits are (b_q << 19) | (1 << 18), the bin's midpoint in bits.
 *   Exposure e.  opts.exposure > 0: e = opts.exposure. opts.exposure == 0 (automatic): e = opts.key / L_{key_permille} if
 *     M > 0, else e = 1.0f.
 *   White point w (used by the Reinhard curve only).  opts.white > 0: w = opts.white. opts.white == 0 (automatic):
 *     w = e * L_{white_permille} if M > 0, else w = 1.0f. (white == 0 is automatic whatever the curve: a caller that wants
 *     no histogram for a curve that ignores w passes any positive white.)
 *   Per pixel, with c = (e * X_r, e * X_g, e * X_b):
 *     RBRT_TONE_LINEAR    out = c
 *     RBRT_TONE_REINHARD  extended Reinhard on the luminance: y = Y(c); s = (1.0f + (y / (w * w))) / (1.0f + y) if y > 0
 *                         (false for NaN), else s = 1.0f; out_c = c_c * s. A grey of luminance w comes out with luminance 1.
 *     RBRT_TONE_ACES      Narkowicz's rational fit, per channel: x = c_c * 0.6f;
 *                         out_c = (x * ((2.51f * x) + 0.03f)) / ((x * ((2.43f * x) + 0.59f)) + 0.14f)
 *   The float output is out; the 8-bit output is the usual quantisation of out.
 * Two consequences. With e = 1 and RBRT_TONE_LINEAR the outputs are bit for bit the input and the render's own rgb8 (1.0f * x
 * is x). Finite inputs with |e * X| <= 1e15 give no NaN (the squares in the ACES fit overflow to inf / inf near 3e38 / 0.6;
 * Reinhard's y / (w * w) needs w * w neither 0 nor inf, which a w in 1e-15..1e15 gives). */
#define RBRT_TONE_LINEAR 0u
#define RBRT_TONE_REINHARD 1u
#define RBRT_TONE_ACES 2u

typedef struct rbrt_tonemap_opts {
    uint32_t curve;          /* RBRT_TONE_LINEAR | _REINHARD | _ACES */
    float exposure;          /* > 0: the multiplier; 0: automatic */
    float key;               /* automatic exposure: what L_{key_permille} is mapped to; finite, > 0 */
    uint32_t key_permille;   /* 0..1000 */
    float white;             /* > 0: the white point; 0: automatic */
    uint32_t white_permille; /* 0..1000 */
    uint32_t reserved[2];    /* 0 */
} rbrt_tonemap_opts_t;
void rbrt_tonemap_opts_default(rbrt_tonemap_opts_t* opts); /* LINEAR, exposure 1, key 0.18, 500, white 0, 990 */

typedef struct rbrt_tonemap_result { /* what the call chose; lives in the workspace, in device memory */
    float exposure, white;           /* e and w as used */
    float l_key, l_white;            /* the two L_q (0 when not computed) */
    uint32_t counted, reserved;      /* M */
    uint64_t pixels;                 /* n */
} rbrt_tonemap_result_t;

#define RBRT_TONEMAP_BINS 4096u
#define RBRT_TONEMAP_RESULT_OFFSET (RBRT_TONEMAP_BINS * 4u)
#define RBRT_TONEMAP_WORKSPACE_BYTES (RBRT_TONEMAP_RESULT_OFFSET + 32u)

/* The transform on n_pixels pixels in DEVICE memory (float[n][3]; a row-major image is W * H pixels, a packed tile buffer
 * rbrt_hip_packed_pixels(...) pixels). Asynchronous on `stream`; needs no scene, like rbrt_hip_unpack_tiles and
 * rbrt_hip_denoise_halves, and owns no device memory. d_workspace: RBRT_TONEMAP_WORKSPACE_BYTES bytes of device memory of the
 * caller's, 16-byte aligned; it may be NULL when neither exposure nor white is automatic. The call zeroes the histogram itself,
 * in stream order. After the call the workspace holds the histogram as uint32[RBRT_TONEMAP_BINS] and, RBRT_TONEMAP_RESULT_OFFSET
 * bytes in, the rbrt_tonemap_result_t (a host reads it with a 32-byte copy behind the stream). With a workspace the result is
 * written even if nothing was automatic (counted, l_key and l_white are then 0 and so are the histogram's words). Two calls on
 * different streams must not share a workspace.
 * d_out_radiance (float[n][3]) may be exactly d_radiance (in place; any other overlap is undefined) or NULL; d_rgb8
 * (uint8[n][3]) may be NULL. The kernels use 16-byte accesses when d_radiance and d_out_radiance are 16-byte aligned and d_rgb8
 * 4-byte aligned; other pointers take a slower form that computes the same bits.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_radiance or opts NULL; n_pixels == 0; an unknown curve; a non-zero
 * reserved word; an exposure, key or white that is not finite; a negative exposure or white; key <= 0 while the exposure is
 * automatic; a permille above 1000; automatic exposure or white with a NULL workspace; a workspace that is not 16-byte aligned.
 * RBRT_ERR_UNSUPPORTED: n_pixels >= 2^32 (the bins are 32-bit). */
int rbrt_hip_tonemap(int device, void* stream, const float* d_radiance, size_t n_pixels,
                     const rbrt_tonemap_opts_t* opts, void* d_workspace,
                     float* d_out_radiance, uint8_t* d_rgb8);

/* ---- Glare: a pyramid bloom stage in front of the display transform ----------------------------------------------------------
 * No counterpart in the reference. After any tone curve a sun of radiance 50 and one of radiance 5000 are the same white disc;
 * a lens, or an eye, tells them apart by the share of a bright source's light that scatters into its surroundings (Spencer et
 * al. 1995). The stage reads an image X, float[H][W][3], row-major, W, H >= 1, and writes the image with that share moved.
 * It belongs between the radiance and the exposure: denoise -> glare -> display transform.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / is correctly rounded; a constant is the float32 nearest
 * to the decimal written. Options: threshold T, intensity i, levels L, spread s.
 *   Bright pass.  Y(c) is the display transform's luminance: ((0.2126f * c_r) + (0.7152f * c_g)) + (0.0722f * c_b). A pixel is
 *     BRIGHT iff the bits u of Y(X) satisfy 0x00800000 <= u <= 0x7F7FFFFF (the display transform's "counted" test) and Y > T.
 *     For a bright pixel k = (Y - T) / Y and B_c = X_c * k; every other pixel has B = 0. With T = 0, k is exactly 1. NaN,
 *     infinities, zero, denormals and negative luminance never enter the pyramid: a non-finite pixel stays a defect of its own
 *     pixel and poisons no neighbourhood.
 *   Pyramid sizes.  W_0 = W, H_0 = H; W_l = (W_{l-1} + 1) / 2 and H_l = (H_{l-1} + 1) / 2 in integers (never 0).
 *     cl(k, n) = min(max(k, 0), n - 1).
 *   REDUCE (Burt-Adelson, weights 1 4 6 4 1 over 16, edges replicated) maps F of size h x w to h' x w'. Rows first:
 *       r[y][x'] = ((((F[y][cl(2x'-2,w)] + (4.0f * F[y][cl(2x'-1,w)])) + (6.0f * F[y][cl(2x',w)])) + (4.0f * F[y][cl(2x'+1,w)]))
 *                   + F[y][cl(2x'+2,w)]) * 0.0625f
 *     then columns: D[y'][x'] is the same expression over r[cl(2y'-2,h)][x'] .. r[cl(2y'+2,h)][x'].
 *     D_0 = B, and D_l = REDUCE(D_{l-1}) for l = 1..L.
 *   EXPAND maps G of size h' x w' to h x w. Rows first, then columns with the same two forms. Along one axis, for the output
 *     index x with k = x >> 1 (cl against the size of G along that axis):
 *       even x:  ((G[cl(k-1)] + (6.0f * G[k])) + G[cl(k+1)]) * 0.125f
 *       odd x:   (G[k] + G[cl(k+1)]) * 0.5f
 *   Collapse.  G_L = D_L; for l = L-1 down to 1: G_l = D_l + (s * EXPAND(G_{l+1})); E = EXPAND(G_1) at H x W. D_0 is
 *     deliberately not added: unblurred light is not glare. So no full-resolution intermediate is stored: the composite
 *     recomputes B from X.
 *   Normalisation.  n = 1, p = 1; for l = 2..L: p = p * s, then n = n + p. inv = 1.0f / n; a = i * inv.
 *   Output.  out_c = (X_c - (i * B_c)) + (a * E_c). The 8-bit output is the usual quantisation of out.
 * Consequences. An image with nothing bright comes back equal as floats (a -0.0f becomes +0.0f), and its rgb8 is identical.
 * Light is moved, not added: for an impulse far from the edges each input's weights sum to 1/4 in REDUCE and to 4 in EXPAND,
 * so sum(E) = n * sum(B) up to rounding and sum(out) = sum(X). A constant image with T = 0 and s = 1 gives B == X, E == L * X
 * where the sums round exactly, and out == X. */
#define RBRT_GLARE_MAX_LEVELS 8u

typedef struct rbrt_glare_opts {
    float threshold;      /* T: luminance above which a pixel is bright; finite, >= 0 */
    float intensity;      /* i: the share of the bright light that is moved; in (0, 1] */
    uint32_t levels;      /* L: 1..RBRT_GLARE_MAX_LEVELS; the widest lobe is about 2^(L+1) pixels */
    float spread;         /* s: the weight of each coarser level against the one below it; finite, >= 0 */
    uint32_t reserved[4]; /* 0 */
} rbrt_glare_opts_t;
void rbrt_glare_opts_default(rbrt_glare_opts_t* opts); /* T = 1, i = 0.1, L = 5, s = 1 */

/* The bytes of device memory rbrt_hip_glare needs as its workspace: the pyramid's levels 1..levels, in the library's own layout
 * (a pixel padded to 16 bytes). 0 for arguments the call would refuse: a zero size, levels 0 or above the maximum,
 * width * height >= 2^31. */
size_t rbrt_hip_glare_workspace_bytes(uint32_t width, uint32_t height, uint32_t levels);

/* The stage on a row-major image in DEVICE memory. Asynchronous on `stream`; needs no scene and owns no device memory.
 * d_workspace: rbrt_hip_glare_workspace_bytes(width, height, opts->levels) bytes of device memory of the caller's, 16-byte
 * aligned; the call assumes nothing about its contents and leaves the pyramid in it. Two calls on different streams must not
 * share a workspace. d_out_radiance (float[H][W][3]) may be exactly d_radiance (in place: a thread reads its own X before it
 * writes; any other overlap is undefined) or NULL; d_rgb8 (uint8[H][W][3]) may be NULL; with both NULL nothing is launched.
 * The composite uses 16-byte accesses when the width is a multiple of 4, d_radiance and d_out_radiance are 16-byte aligned and
 * d_rgb8 is 4-byte aligned; anything else takes a slower form that computes the same bits.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_radiance, opts or d_workspace NULL; width or height 0; levels 0 or above
 * RBRT_GLARE_MAX_LEVELS; a non-zero reserved word; a threshold, intensity or spread that is not finite; threshold < 0;
 * intensity outside (0, 1]; spread < 0; a workspace that is not 16-byte aligned.
 * RBRT_ERR_UNSUPPORTED: width * height >= 2^31. */
int rbrt_hip_glare(int device, void* stream, const float* d_radiance, uint32_t width, uint32_t height,
                   const rbrt_glare_opts_t* opts, void* d_workspace, float* d_out_radiance, uint8_t* d_rgb8);

/* ---- Feature buffers: albedo, normal, depth and coverage of the primary rays ---------------------------------------------------
 * No counterpart in the reference, whose render_scene returns colour only. Every stage above sees colour only, too; these
 * buffers say which surface a pixel shows: what a feature-guided filter, a compositing mask or an external denoiser reads, or
 * a depth or normal pass of its own. They are made from the render's own primary rays, by a kernel of their own.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / and sqrt are correctly rounded.
 *   Rays.  For pixel (row, col) and sample s in 0..n-1 the primary ray (o, d) is the render's own: the stream keyed
 *     (opts->seed, row * W + col, s) draws the column jitter, then the row jitter, which place the target T (cam.rs:64-82); with
 *     RBRT_FLAG_THIN_LENS the lens draws follow exactly as rbrt_camera_lens_t documents, else o = position and F = T;
 *     d = normalize(F - o). A sample's stream does not depend on spp, so n is independent of opts->spp.
 *   Hit.  The closest hit is Scene::hit with opts->min_dist and opts->max_dist: what rbrt_hip_trace_rays returns.
 *   Per sample:             a ray that hits nothing    a hit of object k with material m
 *     albedo a              (0, 0, 0)                  lambertian, metal: m.albedo (a patterned lambertian: the colour of the hit's
 *                                                      cell, rbrt_pattern_t); dielectric: (1, 1, 1), its attenuation;
 *                                                      emissive: m.albedo, the emitted radiance, which may exceed 1
 *     normal N              (0, 0, 0)                  normalize(g): three divisions by the length. g is the normal the scatter pass
 *                                                      would use for this ray, what rbrt_hip_debug_shading_normals returns: a
 *                                                      sphere's (o + t d) - centre, a BasicTriangle's stored normal, a mesh's stored
 *                                                      face normal or the smooth one. Not flipped towards the ray; no guard.
 *     depth z               0                          dist_from_ray_orig of the winner (rbrt_hip_trace_rays' out_dist)
 *     coverage c            0                          1
 *   Sums.  Every channel of a pixel is a sum from 0 that adds sample 0, 1, ... in that order, then multiplied by
 *     inv_n = 1.0f / float(n). The normal's mean is not renormalised. The depth's mean includes the zeros of the rays that hit
 *     nothing; the coverage tells them apart.
 *   object is an int32: the object id of sample 0 in rbrt_hip_trace_rays' numbering (rbrt_scene_t), or -1 when it hits nothing.
 * Not read: opts->spp, max_depth, bg, RBRT_FLAG_CONSTANT_BACKGROUND and the handle's environment. A NaN sphere discriminant is
 * counted as in a render, so rbrt_hip_scene_check reports it.
 * Consequence. A scene made only of emitters, rendered with RBRT_FLAG_CONSTANT_BACKGROUND and bg = 0 at spp = n, has a radiance
 * image equal bit for bit to its albedo buffer: both are the same sums of L and +0 in sample order, times 1.0f / float(n). */
typedef struct rbrt_feature_opts {
    uint32_t samples;     /* n, 1..65536 */
    uint32_t reserved[3]; /* 0 */
} rbrt_feature_opts_t;
void rbrt_feature_opts_default(rbrt_feature_opts_t* opts); /* samples = 4 */

/* The feature buffers of `cam` into DEVICE memory, row-major: d_albedo and d_normal float[H][W][3], d_depth and d_coverage
 * float[H][W], d_object int32[H][W]. Every output may be NULL; with all of them NULL nothing is launched and the call returns
 * RBRT_OK. Asynchronous on `stream`; the threading rule of rbrt_hip_render_device holds. The call owns no device memory and does
 * not touch the handle's accumulators, adaptive sums, tile tables or pipeline lanes: renders, rbrt_hip_render_adaptive and
 * rbrt_hip_scene_denoise before and after it give what they give without it. It takes the handle's current tree, as
 * rbrt_hip_trace_rays does; the result does not depend on which tree. Works on smooth handles; honours element_order and
 * BasicTriangles. With RBRT_FLAG_THIN_LENS `cam` is the `cam` member of an rbrt_camera_lens_t, as for a render.
 * RBRT_ERR_INVALID_ARG, before the device is touched: scene, cam, opts or features NULL; samples 0 or above 65536; a non-zero
 * reserved word; RBRT_FLAG_COLLECT_STATS set; and what rbrt_hip_render_device rejects in the camera (an image without pixels), the
 * lens or the partition (tile_rank >= tile_world).
 * RBRT_ERR_UNSUPPORTED: tile_world > 1 (a host gathers the image, and the features of the whole frame cost one rank little);
 * an image of 2^32 pixels or more. */
int rbrt_hip_render_features(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, const rbrt_render_opts_t* opts,
                             const rbrt_feature_opts_t* features, void* stream, float* d_albedo, float* d_normal,
                             float* d_depth, float* d_coverage, int32_t* d_object);

/* ---- Guided denoising: an edge-avoiding a-trous filter on the half images, guided by the feature buffers ---------------------
 * No counterpart in the reference. The a-trous wavelet filter of Dammertz, Sewtz, Hanika and Lensch (2010): a 5 x 5 B-spline
 * kernel whose taps move apart by a factor of two from level to level, every tap weighed by how well the two pixels agree in
 * normal, depth, albedo and colour. Two additions: the albedo is divided out before the filter and multiplied back behind it
 * (texture is not noise), and a per-pixel variance, estimated from the difference of the two half images and carried from level
 * to level, scales the colour term, as the spatial part of SVGF does. The non-local-means filter above compares noisy patches
 * with noisy patches; this one asks the feature buffers where the edges are.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / is correctly rounded; a constant is the float32
 * nearest to the decimal written. "Inside" means inside the W x H image; a sum "from 0" starts at 0.0f and adds its terms one
 * at a time in the stated order.
 *   Inputs.  Half images A, B, float[H][W][3]; their mix wa, float[H][W] (NULL: 0.5 everywhere); albedo rho and normal N,
 *     float[H][W][3]; depth z and coverage c, float[H][W]; levels L; the sigmas colour kc, normal kn, depth kz, albedo ka; flags.
 *     eps = 1e-7f, floor = 0.01f. On the host, in float32: kc2 = kc * kc, kz2 = kz * kz, in = 1.0f / (kn * kn),
 *     ia = 1.0f / (ka * ka).
 *   Prepare, per pixel p and channel c.
 *     m_c = max(rho_c + (1.0f - c), floor): a ray that hit nothing counts as albedo 1, so a background pixel is not divided by 0
 *       and a partly covered pixel gets the mean of its samples' effective albedos.
 *     u_c = m_c, or 1.0f with RBRT_GUIDED_NO_DEMODULATION (m guides the weights either way).
 *     a_c = A_c / u_c;  b_c = B_c / u_c;  I_c = (a_c * wa) + (b_c * (1.0f - wa));  e_c = (a_c - b_c) squared.
 *     V_c[p] = (sum / float(count)) * 0.25f, where sum runs over the 3 x 3 neighbourhood of p (dy outer -1..1, dx inner -1..1,
 *       from 0) of e_c, only pixels inside are added and count is how many: the variance of the mean of two halves.
 *   Level l = 0..L-1, step s = 1 << l. Every level reads the previous level's I and V and writes new ones, never in place.
 *     h = (0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f). Taps: j outer -2..2, i inner -2..2, q = p + (j * s, i * s) (row, column);
 *     a tap whose q is outside is skipped. hh = h[j + 2] * h[i + 2] (exact).
 *       n = N[q] - N[p];       Dn = (((n_x * n_x) + (n_y * n_y)) + (n_z * n_z)) * in
 *       a = m[q] - m[p];       Da = (((a_r * a_r) + (a_g * a_g)) + (a_b * a_b)) * ia
 *       dz = z[q] - z[p];      Dz = (dz * dz) / (eps + (kz2 * (z[p] * z[q])))    (a relative depth: two zeros agree, a zero
 *                                                                                 against a hit does not)
 *       g_c = I_c[q] - I_c[p]; t_c = (g_c * g_c) / (eps + (kc2 * (V_c[p] + V_c[q])));  Dc = ((t_r + t_g) + t_b) * 0.33333334f
 *       D = ((Dn + Dz) + Da) + Dc;   f = max(0, 1 - 0.25f * max(D, 0));   w = hh * ((f * f) * (f * f))
 *     (the weight of "Denoising" above). Sums from 0 in tap order: num_c += w * I_c[q]; nv_c += (w * w) * V_c[q]; den += w.
 *     The centre tap has D = 0 and w = 0.140625, so den > 0 always. I'_c = num_c / den; V'_c = nv_c / (den * den). The last
 *     level's V' is not needed.
 *   Output.  out_c = I_c * u_c, then the usual quantisation for rgb8.
 * Finite inputs give no NaN when |A|, |B| <= 1e6, the features are finite and z >= 0. A non-finite input gives unspecified values
 * in the pixels whose taps reach it; it never faults. */
#define RBRT_GUIDED_NO_DEMODULATION 1u /* flags: filter the radiance itself (u = 1); the albedo still guides the weights */
#define RBRT_GUIDED_MAX_LEVELS 6u
typedef struct rbrt_guided_opts {
    uint32_t levels;                      /* L, 1..RBRT_GUIDED_MAX_LEVELS */
    float colour, normal, depth, albedo;  /* kc, kn, kz, ka: finite, > 0; larger lets more through */
    uint32_t flags;                       /* RBRT_GUIDED_* */
    uint32_t reserved[2];                 /* 0 */
} rbrt_guided_opts_t;
void rbrt_guided_opts_default(rbrt_guided_opts_t* opts); /* L = 5, kc = 2, kn = 0.35, kz = 0.05, ka = 0.1, flags 0 */

/* Bytes of workspace rbrt_hip_denoise_guided needs for a width x height image: the packed guides ({N, z} and {m, 0}, 16 bytes a
 * pixel each) and two sets of {I, 0} and {V, 0} planes, which the levels read and write in turns: 96 bytes a pixel. 0 for sizes
 * the call refuses. */
size_t rbrt_hip_guided_workspace_bytes(uint32_t width, uint32_t height);

/* The filter on two half images and four feature buffers in DEVICE memory, all row-major (d_a, d_b, d_albedo, d_normal
 * float[H][W][3]; d_wa, d_depth, d_coverage float[H][W]; d_wa NULL: 0.5 everywhere). Needs no scene. Writes the row-major result
 * to d_radiance and / or its quantisation to d_rgb8 (either may be NULL; with both NULL nothing is launched). Asynchronous on
 * `stream`. The call owns no device memory: d_workspace is the caller's, rbrt_hip_guided_workspace_bytes(width, height) bytes,
 * 16-byte aligned; nothing is assumed about its contents, and calls on different streams need different workspaces. An
 * output may be exactly d_a or d_b (the first kernel has consumed every input before an output is written); any other overlap
 * is undefined.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_a, d_b, d_albedo, d_normal, d_depth, d_coverage, opts or d_workspace
 * NULL; width or height 0; levels 0 or above 6; a sigma that is not finite or <= 0; an unknown flag bit; a non-zero reserved
 * word; a workspace that is not 16-byte aligned.
 * RBRT_ERR_UNSUPPORTED: width * height >= 2^31. */
int rbrt_hip_denoise_guided(int device, void* stream, const float* d_a, const float* d_b, const float* d_wa,
                            const float* d_albedo, const float* d_normal, const float* d_depth, const float* d_coverage,
                            uint32_t width, uint32_t height, const rbrt_guided_opts_t* opts, void* d_workspace,
                            float* d_radiance, uint8_t* d_rgb8);

/* The same filter on the image of the handle's last rbrt_hip_render_adaptive call: A, B and wa are made from that call's sums
 * into the handle's half-image memory exactly as rbrt_hip_scene_denoise makes them; the feature buffers (of the same camera:
 * rbrt_hip_render_features) and the workspace are the caller's. The two calls do not disturb each other. Either output may be
 * NULL; with both NULL the call checks its arguments and the handle's last render and then does nothing: no device is set, no
 * memory of the handle grows, nothing is launched. The threading rule of rbrt_hip_render_device holds.
 * RBRT_ERR_INVALID_ARG, before the device is touched: scene NULL; what rbrt_hip_denoise_guided refuses in opts, the feature
 * pointers and the workspace; no adaptive render on the handle yet; the last one had opts->spp < 2.
 * RBRT_ERR_UNSUPPORTED: the last adaptive render had tile_world > 1. */
int rbrt_hip_scene_denoise_guided(rbrt_hip_scene_t* scene, const rbrt_guided_opts_t* opts, void* stream,
                                  const float* d_albedo, const float* d_normal, const float* d_depth, const float* d_coverage,
                                  void* d_workspace, float* d_radiance, uint8_t* d_rgb8);

/* ---- Temporal accumulation: reproject the last frame's half images into this frame ------------------------------------------
 * No counterpart in the reference. In a stream of frames from a moving camera every pixel's point is projected into the last
 * frame's camera, the last frame's accumulated halves are read there (bilinear, four taps, each tap tested against this
 * pixel's depth and normal) and mixed with this frame's halves by the length of the history: the temporal part of SVGF. A is
 * only ever mixed with A's history and B with B's, so the halves stay independent estimates and what both denoisers derive
 * from A - B stays valid and shrinks as the history grows. The outputs go into rbrt_hip_denoise_halves or
 * rbrt_hip_denoise_guided unchanged.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / and sqrt are correctly rounded;
 * dot(a, b) = ((a_x * b_x) + (a_y * b_y)) + (a_z * b_z); a sum "from 0" starts at 0.0f and adds its terms one at a time in the
 * stated order; a constant is the float32 nearest to the decimal written; s * v and v +- w on vectors work per component.
 *   Inputs.  Half images A, B, float[H][W][3]; normal N, float[H][W][3]; depth z and coverage c, float[H][W], as
 *     rbrt_hip_render_features writes them; the camera K of this frame and K' of the last (only the pinhole part: with a thin
 *     lens the reprojection goes through the lens centre); max_history M, depth tolerance kz, normal tolerance kn; the history
 *     of the last frame, per pixel q: A'prev[q], B'prev[q], len'[q], N'[q], z'[q], c'[q].
 *   Camera constants of K' (host, one operation a statement).
 *     n = right x up: n_x = (r_y * u_z) - (r_z * u_y), and so on cyclically. w = img_center_point - position. wn = dot(w, n).
 *     rr = dot(right, right); uu = dot(up, up); ru = dot(right, up); det = (rr * uu) - (ru * ru).
 *     sx = 0.001f * mm_per_pix_hor; sy = 0.001f * mm_per_pix_vert. hx = float(W / 2), hy = float(H / 2), integer halving.
 *   Centre ray of pixel p = (row, col) in K: the render's own ray with both jitter draws at 0.5.
 *     cm = (float(col) - hx) * mm_per_pix_hor; rm = (float(row) - hy) * mm_per_pix_vert.
 *     T = (img_center_point + ((0.001f * cm) * right)) - ((0.001f * rm) * up).
 *     e = T - position; d = e / sqrt(dot(e, e)), three divisions by the length.
 *   Point.  If c[p] > 0 the pixel is a surface pixel: zbar = z[p] / c[p], P = position + (zbar * d), v = P - position'.
 *     Else it is a background pixel and v = d: a point at infinity, because sky and environment depend on direction only.
 *   Projection into K'.
 *     t = wn / dot(v, n). No history unless t > 0 and t < inf (a NaN compares false).
 *     Q = (t * v) - w. qr = dot(Q, right'). qu = dot(Q, up').
 *     a = ((qr * uu) - (qu * ru)) / det. b = ((qr * ru) - (qu * rr)) / det. (`up` is the raw YAML vector, neither normalised
 *     nor perpendicular to the view, so the image-plane coordinates come from a Gram solve.)
 *     xs = (a / sx) + hx. ys = (b / sy) + hy.
 *     No history unless xs > -1, xs < W, ys > -1 and ys < H; the tests are made on the floats, before any conversion.
 *     i = floor(xs), j = floor(ys). fx = xs - float(i), fy = ys - float(j). gx = 1 - fx, gy = 1 - fy.
 *   Taps, in this order: (j, i) with bw = gx * gy; (j, i + 1) with fx * gy; (j + 1, i) with gx * fy; (j + 1, i + 1) with
 *     fx * fy (row, column). A tap q is accepted iff it is inside the image and
 *       surface pixel: c'[q] > 0, and |zq - ze| <= kz * ze with zq = z'[q] / c'[q] and ze = sqrt(dot(v, v)), and
 *         dot(D, D) <= kn * kn with D = N[p] - N'[q];
 *       background pixel: c'[q] == 0.
 *   Sums from 0 over the accepted taps, in tap order: ws += bw; sa_c += bw * A'prev_c[q]; sb_c likewise; sl += bw * len'[q].
 *     The history is valid iff ws >= 0.01f.
 *   Result.  Without a valid history, or without any history at all (the first frame): A' = A and B' = B exactly, len = 1.
 *     Else HA_c = sa_c / ws, HB_c = sb_c / ws, hl = sl / ws; len = min(hl + 1, M); alpha = 1 / len;
 *     A'_c = HA_c + (alpha * (A_c - HA_c)); B' likewise.
 *   The next history holds A', B', len and this frame's N, z, c.
 * Consequences. A pixel with no valid history passes through bit for bit. A history value at a tap that is not accepted never
 * influences any output. A static camera and scene give the running mean of the frames, up to the bilinear footprint of
 * |xs - col|. Whatever the inputs are, NaN and infinities included, no read leaves the buffers. A non-finite input gives
 * unspecified values in the pixels whose taps reach it, and never a fault. */
typedef struct rbrt_temporal_opts {
    float max_history;     /* M: finite, >= 1 */
    float depth;           /* kz: finite, >= 0 */
    float normal;          /* kn: finite, >= 0 */
    uint32_t flags;        /* 0 */
    uint32_t reserved[4];  /* 0 */
} rbrt_temporal_opts_t;
void rbrt_temporal_opts_default(rbrt_temporal_opts_t* opts); /* M = 32, kz = 0.05, kn = 0.35, flags 0 */

/* Bytes of one history of a width x height image. The history is in the library's own layout: 48 bytes a pixel as three
 * 16-byte records {A', len}, {B', c}, {N, z}, three planes of width * height records, so that a tap is three aligned 16-byte
 * loads. 0 for sizes the call refuses. */
size_t rbrt_hip_temporal_history_bytes(uint32_t width, uint32_t height);

/* One frame of the rule on buffers in DEVICE memory, all row-major (d_a, d_b, d_normal float[H][W][3]; d_depth, d_coverage
 * float[H][W]); width and height are cam's. Asynchronous on `stream`; needs no scene and owns no device memory.
 * d_history_in is the history the last frame's call wrote (NULL: the first frame; cam_prev may then be NULL too and is not
 * read); d_history_out receives the next one. They must differ: the caller keeps two and alternates. Nothing is assumed about
 * the contents of d_history_out. Every output (d_history_out, d_out_a, d_out_b, d_out_length: float[H][W]) may be NULL; with
 * all four NULL nothing is launched. d_out_a may be exactly d_a and d_out_b exactly d_b (a thread reads its own pixel before
 * it writes); any other overlap is undefined.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_a, d_b, d_normal, d_depth, d_coverage, cam or opts NULL; cam_prev NULL
 * with a history; d_history_in == d_history_out (non-NULL); a history that is not 16-byte aligned; an image without pixels;
 * cam_prev's size differing from cam's; max_history not finite or < 1; depth or normal not finite or < 0; a non-zero flag or
 * reserved word; a cam_prev whose det or wn is 0 or not finite, or whose mm_per_pix is not finite and > 0; the same for
 * cam's mm_per_pix.
 * RBRT_ERR_UNSUPPORTED: 2^31 pixels or more. */
int rbrt_hip_temporal_accumulate(int device, void* stream, const float* d_a, const float* d_b, const float* d_normal,
                                 const float* d_depth, const float* d_coverage, const rbrt_camera_t* cam,
                                 const rbrt_camera_t* cam_prev, const rbrt_temporal_opts_t* opts, const void* d_history_in,
                                 void* d_history_out, float* d_out_a, float* d_out_b, float* d_out_length);

/* ---- Animation: spheres advance from frame to frame, and the accumulation follows them ------------------------------------------
 * No counterpart in the reference. Three additions on top of "Moving spheres", "Feature buffers" and "Temporal accumulation",
 * each detected by its symbol; the ABI version stays 2, no struct changes, and a host that calls none of them gets, bit for
 * bit, what it got before. All arithmetic is float32, unfused, in the written order.
 *
 * 1. The phase. A handle has a phase, a float, 0 until rbrt_hip_scene_set_motion_phase sets another. It has an effect only
 * while a motion is set, and it survives rbrt_hip_scene_set_motion (set, replace and clear). A sample's draw t is made exactly
 * as in "Moving spheres": one draw, shared with the shutter, which keeps the raw t (o += t * travel). Wherever a path of that
 * sample reads sphere i's centre it reads
 *     s        = phase + t                          (one addition)
 *     c_i(s)_c = center_i_c + (s * travel_i_c)      for c = x, y, z
 * in the trace kernel's motion launch (every park, resume, helper launch and scatter), in the short-path stage, in
 * rbrt_hip_render_features and in the tile pass, whose margins are made around the advanced centre center_i + phase * travel_i
 * (kernels.hip, "A phase"): a sphere that has left the view is culled again. With phase == 0, s has the bits of t (0.0f + t
 * with t >= +0): a handle that never calls the function, or sets 0, renders bit for bit what it renders without this section.
 * The phase counts exposures: frame k of a stream whose spheres advance P exposures a frame runs at phase float(k) * P.
 * Like the shutter's travel the phase goes with the launches issued after the call; launches in flight keep theirs. Nothing is
 * copied to the device and nothing waits: the call is meant to be made once a frame. One phase must serve every pass of one
 * rbrt_hip_render_pass series, every round of one rbrt_hip_render_adaptive call (the call reads it once a launch: do not
 * change it from another thread meanwhile), and the low render and the full-size features of one upscaled frame. The plain
 * build of the trace kernel is not involved: a scene with a motion never runs it.
 * RBRT_ERR_INVALID_ARG, before the device is touched, the handle keeping its phase: scene NULL; a phase that is not finite;
 * with a motion set, a center_i + ((phase + 1) * travel_i) that is not finite in float32. rbrt_hip_scene_set_motion makes the
 * same check of its travels against the handle's phase. */
int rbrt_hip_scene_set_motion_phase(rbrt_hip_scene_t* scene, float phase);

/* 2. The motion buffer. rbrt_hip_render_features with one more output, d_motion, float[H][W][3], which may be NULL like the
 * others; rbrt_hip_render_features is this call with d_motion NULL, and runs the kernel it has always run. Per sample: a hit
 * of sphere i on a handle with a motion contributes travel_i; a hit of mesh m on a handle with a mesh motion contributes w_m
 * ("Moving meshes"); a miss, a hit of a BasicTriangle, and any other hit contribute (+0, +0, +0). Per pixel each of the three sums starts from 0, adds sample 0, 1, ... in
 * that order and is then multiplied by inv_n, like the other channels. The buffer is in scene units per exposure and does not
 * depend on the phase. The ray, the hit and the other five outputs are what rbrt_hip_render_features gives; on a handle with a
 * phase they see the spheres at c_i(s). The refusals are those of rbrt_hip_render_features; with all six outputs NULL nothing
 * is launched. */
int rbrt_hip_render_features_motion(rbrt_hip_scene_t* scene, const rbrt_camera_t* cam, const rbrt_render_opts_t* opts,
                                    const rbrt_feature_opts_t* fopts, void* stream, float* d_albedo, float* d_normal, float* d_depth,
                                    float* d_coverage, int32_t* d_object, float* d_motion);

/* 3. Motion-aware accumulation. rbrt_hip_temporal_accumulate with two more arguments behind d_coverage: d_motion, the motion
 * buffer Mv of THIS frame, and phase_step, this frame's phase minus the last frame's (pass the step itself, not the difference
 * of two rounded products). The rule is that of "Temporal accumulation" with one insertion. For a surface pixel, after
 * P = position + (zbar * d):
 *     m_c    = Mv_c[p] / c[p]            per component: the mean travel of the samples that hit, as zbar is their mean depth
 *     P_last = P - (phase_step * m)      where the point was when the last frame's shutter opened
 *     v      = P_last - position'
 * and everything after v is the rule's: the projection, the four taps, the depth test against ze = sqrt(dot(v, v)), the
 * normal test, the sums and the mix. Background pixels are untouched. The motion is not stored: the history keeps its 48-byte
 * layout, and the histories of the two calls are interchangeable. A translation does not turn a normal, so the normal test
 * compares what it compared; that is why only translations are supported. Limits: only the primary hit is followed. The
 * shadow and the reflection of a moving sphere, and what is seen through glass, lag behind as they do under
 * rbrt_hip_temporal_accumulate; BasicTriangles do not move (a mesh's travel enters d_motion: "Moving meshes"). NaN and infinities in d_motion only move xs and ys,
 * which are tested as before: no read leaves the buffers.
 * d_motion NULL gives exactly rbrt_hip_temporal_accumulate -- the same kernel, the same outputs bit for bit -- and phase_step is
 * not read. Everything that call refuses is refused, and with d_motion a phase_step that is not finite (RBRT_ERR_INVALID_ARG).
 * The call reads 12 more bytes a pixel than the plain one. */
int rbrt_hip_temporal_accumulate_moving(int device, void* stream, const float* d_a, const float* d_b, const float* d_normal,
                                        const float* d_depth, const float* d_coverage, const float* d_motion, float phase_step,
                                        const rbrt_camera_t* cam, const rbrt_camera_t* cam_prev, const rbrt_temporal_opts_t* opts,
                                        const void* d_history_in, void* d_history_out, float* d_out_a, float* d_out_b,
                                        float* d_out_length);

/* ---- Moving meshes: a travel per mesh on the shutter's time draw ------------------------------------------------------------------
 * No counterpart in the reference. A rigid translation needs no moved geometry: a ray (o, d) meets a mesh displaced by v exactly
 * where the ray (o - v, d) meets the mesh at rest. The trees, the triangle records, the normals and both builders stay
 * untouched; what changes is which origin the mesh test reads. All arithmetic is float32, unfused, in the written order.
 *
 * State. A handle may carry a mesh motion: one vector w_m per mesh of rbrt_scene_t::meshes, in scene units, the mesh's
 * translation between the opening and the closing of the shutter. The mesh as uploaded is its position at the opening. It is
 * handle state like rbrt_hip_scene_set_motion: no struct changes, no flag bit, the ABI version stays 2 and a host detects the
 * capability by the symbol. The sphere motion and the mesh motion are set and cleared independently; each survives the
 * other's calls, and the phase ("Animation") survives both.
 *
 * The draw. A handle with a shutter OR a sphere motion OR a mesh motion makes the one draw t, in the place where it is made
 * today. The time is s = phase + t, as in "Animation". A handle with a mesh motion and no sphere motion behaves as one whose
 * sphere motion is all zeros: the existing rule with zero travels describes its spheres.
 *
 * The mesh. Wherever a path of that sample tests mesh m, on the camera ray and every bounce, it reads the origin
 *     o_m,c = o_c - (s * w_m,c)        for c = x, y, z   (a product, then a difference)
 * and everything mesh.rs does with the ray is done with (o_m, d): the box gate; the culling record of the traversal; the
 * triangle scan with its tie rule and its t > eps && t < 1e5; p_m = o_m + t * d, dist = length(o_m - p_m) and the distance
 * window; for a smooth mesh, the barycentrics of the shading normal. In world space, and what they were: the comparison of
 * dist against the closest hit so far (strict <, spheres first, meshes in order), and the hit point the path continues from,
 * p = o + t * d with the path's own o -- the expression the scatter pass uses for every object, and the point a solid checker
 * is evaluated at: the pattern stays in world space and the mesh moves through it. A translation does not turn a normal, so
 * the stored normals are read as they are.
 *
 * While a mesh motion is set, rbrt_hip_render_device, _render_pass, _render_adaptive and rbrt_hip_render_features honour it,
 * for every tile_rank / tile_world, in helper launches, in the short-path stage and in the tile pass (kernels.hip
 * primary_cull_kernel, "Moving meshes"). A scene with a mesh motion never runs the trace kernel's plain build; after a clear
 * a scene that ran it runs it again. rbrt_hip_trace_rays and the ray hooks have no sample stream and see the meshes at rest.
 * The one-shot rbrt_hip_render* calls cannot carry a mesh motion. In rbrt_hip_render_features_motion a sample that hits mesh m
 * on a handle with a mesh motion contributes w_m; nothing else changes in that call, so rbrt_hip_temporal_accumulate_moving
 * follows a moving mesh as it follows a moving sphere.
 * Not built: moving BasicTriangles, rotation, a pattern that travels with its mesh, a time argument for rbrt_hip_trace_rays. */
typedef struct rbrt_mesh_motion {
    uint32_t n_meshes;   /* the scene's mesh count */
    uint32_t reserved;   /* 0 */
    const float* travel; /* [n_meshes][3], in the order of rbrt_scene_t::meshes; finite */
} rbrt_mesh_motion_t;

/* Sets, replaces (motion != NULL) or clears (NULL) the handle's mesh motion. The vectors are copied: the call waits for the
 * handle's launches in flight and puts them on the device. The threading rule of rbrt_hip_scene_set_motion holds.
 * RBRT_ERR_INVALID_ARG, before the device is touched, the handle keeping what it had: scene NULL; n_meshes other than the
 * scene's mesh count; reserved != 0; travel NULL with n_meshes > 0; a component that is not finite; a mesh whose box corner
 * plus (phase + 1) * travel is not finite in float32. rbrt_hip_scene_set_motion_phase makes the same check of the mesh travels
 * against the new phase. */
int rbrt_hip_scene_set_mesh_motion(rbrt_hip_scene_t* scene, const rbrt_mesh_motion_t* motion);

/* ---- Guided upsampling: trace a smaller image, reconstruct the full one from the full-size feature buffers -------------------
 * No counterpart in the reference. The trace kernel's cost is proportional to the pixel count; the feature buffers are cheap.
 * So the image is traced with a camera of 1 / f the size in each direction (rbrt_hip_upsample_camera; an ordinary render), the
 * features are made at full size, and every full pixel takes its two half images from the four low pixels around it, each
 * weighed by its bilinear weight times how well the low pixel's features agree with the full pixel's: a joint bilateral
 * upsampling (Kopf, Cohen, Lischinski and Uyttendaele 2007) with the guided filter's distances and weight. The albedo is
 * divided out at low size and multiplied back at full size, so an albedo edge is as sharp as the feature buffers. A and B get
 * the same weights and the weights come from the features only, never from the noise: the halves stay independent estimates
 * and what both denoisers derive from A - B stays valid. The outputs go into rbrt_hip_temporal_accumulate,
 * rbrt_hip_denoise_halves or rbrt_hip_denoise_guided unchanged.
 *
 * The low camera. f in 1..RBRT_UPSAMPLE_MAX_FACTOR; w = (W + f - 1) / f, h = (H + f - 1) / f (integer division). `low` is `full`
 * except for the size (w, h), mm_per_pix_* = float(f) * mm_per_pix_*, and img_center_point, which is shifted so that low pixel
 * (j, i)'s footprint on the image plane is exactly the union of the footprints of the full pixels of its block (below; where W
 * or H is no multiple of f the last low pixels reach beyond the full image). The render centres pixel col on col - W / 2
 * (integer halving) and jitters by u - 0.5, so in float32, unfused, in this order:
 *     kx = (float(f * (w / 2)) - float(W / 2)) + (0.5f * float(f - 1));  ky likewise from h and H;
 *     c' = (c + ((0.001f * (kx * mm_per_pix_hor)) * right)) - ((0.001f * (ky * mm_per_pix_vert)) * up), per component.
 * Low pixel i's centre then lies on full coordinate i * f + (f - 1) / 2. A thin lens keeps lens_u, lens_v and focus_scale: the
 * caller wraps the low camera in its own rbrt_camera_lens_t.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / is correctly rounded; a constant is the float32
 * nearest to the decimal written; a sum "from 0" starts at 0.0f and adds its terms one at a time in the stated order;
 * max(x, y) is C's fmaxf: the other operand when one is a NaN.
 *   Inputs.  Low half images a, b, float[h][w][3]; their mix wa, float[h][w] (NULL: 0.5 everywhere); the full-size albedo rho
 *     and normal N, float[H][W][3], depth z and coverage c, float[H][W], as rbrt_hip_render_features writes them for the full
 *     camera; the factor f; the sigmas normal kn, depth kz, albedo ka; flags. On the host: in = 1.0f / (kn * kn),
 *     ia = 1.0f / (ka * ka), kz2 = kz * kz, invf = 1.0f / float(f). eps = 1e-7f, floor = 0.01f.
 *   Reduce, per low pixel q = (j, i) (row, column). Its block is the full pixels of the rows j * f .. min(j * f + f, H) - 1 and
 *     the columns i * f .. min(i * f + f, W) - 1; cnt is their number; inv = 1.0f / float(cnt).
 *     Each of the eight feature channels: x_l[q] = (the sum of x over the block, rows outer, columns inner, from 0) * inv. That
 *       gives rho_l, N_l, z_l, c_l: the features the low pixel's own samples would have seen, because the footprints coincide.
 *     m_l = max(rho_l + (1.0f - c_l), floor) per channel (the guided filter's effective albedo).
 *     u_l = m_l, or 1.0f with RBRT_UPSAMPLE_NO_DEMODULATION (m guides the weights either way).
 *     a~ = a / u_l;  b~ = b / u_l.
 *   Gather, per full pixel p = (R, C) (row, column).
 *     m = max(rho + (1.0f - c), floor) per channel; u = m, or 1.0f with the flag.
 *     xl = ((float(C) + 0.5f) * invf) - 0.5f;  i = floor(xl);  fx = xl - float(i);  gx = 1.0f - fx.
 *     Rows likewise from R: j, fy, gy.
 *     Four taps in this order, each with a bilinear weight bw: (j, i) with gx * gy; (j, i + 1) with fx * gy; (j + 1, i) with
 *     gx * fy; (j + 1, i + 1) with fx * fy. Each tap index is clamped into the low image as an integer (the edges are
 *     replicated): that is q.
 *       n = N_l[q] - N[p];     Dn = (((n_x * n_x) + (n_y * n_y)) + (n_z * n_z)) * in
 *       d = m_l[q] - m[p];     Da = (((d_r * d_r) + (d_g * d_g)) + (d_b * d_b)) * ia
 *       dz = z_l[q] - z[p];    Dz = (dz * dz) / (eps + (kz2 * (z[p] * z_l[q])))
 *       D = (Dn + Dz) + Da;    g = max(0, 1 - 0.25f * max(D, 0));    wt = bw * ((g * g) * (g * g))
 *     (the distances and the weight of "Guided denoising" above). A tap is added only if wt > 0 (a NaN compares false). Sums
 *     from 0 over the added taps, in tap order: den += wt; na_c += wt * a~_c[q]; nb_c += wt * b~_c[q]; nw += wt * wa[q].
 *   Result.  If den >= 0.01f: A_c = (na_c / den) * u_c; B_c = (nb_c / den) * u_c; wa' = nw / den.
 *     Else the fallback, with q0 = (R / f, C / f) by integer division, the low pixel whose block holds p:
 *     A_c = a~_c[q0] * u_c; B_c = b~_c[q0] * u_c; wa' = wa[q0].
 * Consequences. A tap with zero weight never influences any output, whatever it holds, NaN and infinities included; the
 * fallback pixel q0 of a pixel without enough weight does. Every index comes from integers and from floors of finite values
 * made from integers, clamped as integers, so no read leaves the buffers whatever the floats are. With f = 1, the flag set and
 * finite features the output is the input bit for bit (but for a -0 in a or b, which comes out as +0). Light does not cross
 * an edge of the features: changing the low pixels on one side changes nothing on the other but fallback pixels. */
#define RBRT_UPSAMPLE_MAX_FACTOR 4u
#define RBRT_UPSAMPLE_NO_DEMODULATION 1u /* flags: interpolate the radiance itself (u = 1); the albedo still guides the weights */
typedef struct rbrt_upsample_opts {
    uint32_t factor;              /* f, 1..RBRT_UPSAMPLE_MAX_FACTOR */
    float normal, depth, albedo;  /* kn, kz, ka: finite, > 0; larger lets more through */
    uint32_t flags;               /* RBRT_UPSAMPLE_* */
    uint32_t reserved[3];         /* 0 */
} rbrt_upsample_opts_t;
void rbrt_upsample_opts_default(rbrt_upsample_opts_t* opts); /* f = 2, kn = 0.5, kz = 0.1, ka = 0.2, flags 0 */

/* The low camera of the rule above, on the host alone: no device is touched.
 * RBRT_ERR_INVALID_ARG: full or low NULL; factor 0 or above RBRT_UPSAMPLE_MAX_FACTOR; an image without pixels; an mm_per_pix
 * that is not finite. `low` may be `full` itself. */
int rbrt_hip_upsample_camera(const rbrt_camera_t* full, uint32_t factor, rbrt_camera_t* low);

/* Bytes of workspace rbrt_hip_upsample_halves needs for a width x height (full-size) image at `factor`: the packed low
 * records in the library's own layout, four planes of one 16-byte record a low pixel, {a~, wa}, {b~, z_l}, {N_l, c_l},
 * {m_l, 0}: 64 bytes a low pixel, so that a tap is four aligned 16-byte loads. 0 for what the call refuses. */
size_t rbrt_hip_upsample_workspace_bytes(uint32_t width, uint32_t height, uint32_t factor);

/* The rule on buffers in DEVICE memory, all row-major. width and height are the FULL size W, H; d_a, d_b are float[h][w][3] and
 * d_wa float[h][w] at the low size of opts->factor (d_wa NULL: 0.5 everywhere); the feature buffers are full size; the outputs
 * are full size, d_out_a and d_out_b float[H][W][3], d_out_wa float[H][W]. Any output may be NULL; with all three NULL nothing
 * is launched. Needs no scene, owns no device memory, asynchronous on `stream`: d_workspace is the caller's,
 * rbrt_hip_upsample_workspace_bytes(width, height, factor) bytes, 16-byte aligned; nothing is assumed about its contents, and
 * calls on different streams need different workspaces. No input may overlap an output or the workspace.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_a, d_b, d_albedo, d_normal, d_depth, d_coverage, opts or d_workspace
 * NULL; width or height 0; factor 0 or above RBRT_UPSAMPLE_MAX_FACTOR; a sigma that is not finite or <= 0; an unknown flag bit;
 * a non-zero reserved word; a workspace that is not 16-byte aligned.
 * RBRT_ERR_UNSUPPORTED: width * height >= 2^31. */
int rbrt_hip_upsample_halves(int device, void* stream, const float* d_a, const float* d_b, const float* d_wa,
                             const float* d_albedo, const float* d_normal, const float* d_depth, const float* d_coverage,
                             uint32_t width, uint32_t height, const rbrt_upsample_opts_t* opts, void* d_workspace,
                             float* d_out_a, float* d_out_b, float* d_out_wa);

/* ---- Spike removal: a rank-order firefly clamp on the two half images ----------------------------------------------------------
 * No counterpart in the reference. A diffuse path that finds a small, very bright light by chance leaves one sample thousands
 * of times brighter than its neighbours (the lambertian has no pdf, so the light cannot be sampled). Every stage behind the
 * trace kernel takes a pixel's noise to be of moderate size: the denoisers spread such a pixel, the accumulation carries it,
 * upsampling enlarges it, glare blooms it. This stage runs in front of them all. A pixel of one half image is limited to a
 * multiple of the larger of two witnesses: the k-th largest luminance among its neighbours in its own half, and its own
 * luminance in the OTHER half, which holds an independent estimate of the same pixel. A highlight that both halves see, or
 * that k + 1 neighbouring pixels of one half share, therefore passes; a lone sample does not. No median, no sorting: only
 * comparisons and, in a limited pixel, one division.
 *
 * The rule. All arithmetic is float32, unfused, in the written order; / is correctly rounded; a constant is the float32
 * nearest to the decimal written; max and min are C's fmaxf and fminf. MAXF = 3.4028235e38f. fin(x) is
 * x <= MAXF && x >= -MAXF, so a NaN is not finite. Y(c) = ((0.2126f * c_r) + (0.7152f * c_g)) + (0.0722f * c_b), the display
 * transform's luminance. pos(x) = x if fin(x) && x > 0.0f, else +0.0f.
 *   Inputs.  Half images A and B, float[H][W][3]; the radius R in 1..RBRT_DESPIKE_MAX_RADIUS; the rank k in
 *     1..RBRT_DESPIKE_MAX_RANK; the threshold t, finite, >= 1; the floor f, finite, >= 0.
 *   For the half X with the other half O, at the pixel p:
 *     y = Y(X[p]);  yo = Y(O[p]).
 *     r = the k-th largest element of the multiset that holds pos(Y(X[q])) for every q = p + (dy, dx) with |dy|, |dx| <= R,
 *       q != p, q inside the image, and k zeros (+0.0f). Only values matter, so neither the scan's order nor ties do. A
 *       neighbour that is not finite, or not above 0, stands for one more zero, which changes nothing: k zeros are there
 *       already. So r >= +0.0f, and a pixel with fewer than k usable neighbours gets r = 0.
 *     base = max(r, pos(yo));  lim = min((t * base) + f, MAXF).
 *     If !fin(y): the pixel is flagged and X'[p] = (lim, lim, lim).
 *     Else if y > lim: the pixel is flagged, s = lim / y and X'_c[p] = X_c[p] * s per channel.
 *     Else X'[p] = X[p], bit for bit.
 *   mask[p] has bit 0 set when A was flagged at p and bit 1 set when B was; result.spikes_a and result.spikes_b count the
 *   flagged pixels of A and of B. The mix wa of the halves is not the stage's business: it stays what it was.
 * Consequences. An unflagged pixel passes bit for bit. A pixel's result depends only on its own half's window and on the other
 * half's same pixel. A flagged pixel comes out finite: lim is finite and at least 0, and a finite y above lim >= 0 has finite
 * channels and 0 <= s < 1. A value that both halves hold equally at p is never flagged: since t >= 1 and f >= 0,
 * y > (t * max(r, y)) + f is false. A cluster of k + 1 mutually adjacent equal spikes in one half survives (each has k equal
 * neighbours, so r = y); a cluster of k does not (each has k - 1). Swapping A and B swaps A' and B' and the mask's two bits.
 * With no flagged pixel the call is the identity and both counts are 0. */
#define RBRT_DESPIKE_MAX_RADIUS 2u
#define RBRT_DESPIKE_MAX_RANK 4u
typedef struct rbrt_despike_opts {
    uint32_t radius;       /* R, 1..RBRT_DESPIKE_MAX_RADIUS: the window is (2 R + 1) x (2 R + 1) */
    uint32_t rank;         /* k, 1..RBRT_DESPIKE_MAX_RANK */
    float threshold;       /* t: finite, >= 1 */
    float floor;           /* f: finite, >= 0 */
    uint32_t flags;        /* 0 */
    uint32_t reserved[3];  /* 0 */
} rbrt_despike_opts_t;
void rbrt_despike_opts_default(rbrt_despike_opts_t* opts); /* R = 2, k = 2, t = 4, f = 0.01, flags 0 */

typedef struct rbrt_despike_result { /* what the call found; lives in device memory */
    uint32_t spikes_a, spikes_b;     /* the flagged pixels of A and of B */
    uint32_t reserved[2];            /* 0 */
} rbrt_despike_result_t;

/* The rule on buffers in DEVICE memory, all row-major: d_a, d_b, d_out_a and d_out_b float[height][width][3] (4-byte alignment
 * is enough), d_mask uint8[height][width], d_result one rbrt_despike_result_t (a host reads it with a 16-byte copy behind the
 * stream). Any output may be NULL; with all four NULL nothing is launched. The call zeroes d_result on the stream before its
 * kernel adds to it: nothing is assumed about what it held. Needs no scene, owns no device memory, asynchronous on `stream`.
 * No input may overlap an output: other workgroups read a pixel's neighbours.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_a, d_b or opts NULL; width or height 0; radius outside
 * 1..RBRT_DESPIKE_MAX_RADIUS; rank outside 1..RBRT_DESPIKE_MAX_RANK; a threshold that is not finite or below 1; a floor that is
 * not finite or below 0; a non-zero flag or reserved word; an output that equals an input.
 * RBRT_ERR_UNSUPPORTED: width * height >= 2^31. */
int rbrt_hip_despike_halves(int device, void* stream, const float* d_a, const float* d_b, uint32_t width, uint32_t height,
                            const rbrt_despike_opts_t* opts, float* d_out_a, float* d_out_b, uint8_t* d_mask,
                            rbrt_despike_result_t* d_result);

/* ---- Image comparison: MSE, MAE, relative MSE and SSIM of an image against a reference ---------------------------------------
 * No counterpart in the reference. Every reconstruction stage trades samples for image quality; this stage says how far an
 * image X is from a reference R: the sums behind the mean squared, mean absolute and relative squared error, the largest
 * absolute difference, a mean structural similarity (SSIM) on tone-compressed luminance and, per pixel, the relative error
 * and the SSIM. The sums across workgroups take a fixed order (no float atomics: a slab of per-tile partials and a second
 * kernel that sums it), so two calls on the same inputs give the same 64 bytes, and so does a restatement on a CPU.
 *
 * The rule. All per-pixel arithmetic is float32, unfused, in the written order; / is correctly rounded; a constant is the
 * float32 nearest to the decimal written. fin, MAXF, Y(c) and pos(x) are those of "Spike removal" above. eps is the options'
 * epsilon.
 *   Usable pixels. A pixel p is usable when all six channels of X[p] and R[p] are fin.
 *   Errors of a usable pixel, with e_c = X_c - R_c:
 *     se  = ((e_r * e_r) + (e_g * e_g)) + (e_b * e_b)
 *     ae  = (|e_r| + |e_g|) + |e_b|
 *     rel = (((e_r * e_r) / ((R_r * R_r) + eps)) + ((e_g * e_g) / ((R_g * R_g) + eps))) + ((e_b * e_b) / ((R_b * R_b) + eps))
 *     mx  = max(max(|e_r|, |e_g|), |e_b|)
 *   A pixel that is not usable contributes nothing to these: it is counted in `skipped`, and its value in the rel map is +0.0f.
 *   SSIM, at every pixel, usable or not. u = T(Y(X[p])) and v = T(Y(R[p])) with T(y) = pos(y) / (1.0f + pos(y)): a luminance
 *   that is not finite or not above 0 stands as 0, and the range is [0, 1). The window is 11 taps, separable, with the weights
 *     g[0..5] = 0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,  g[10 - i] = g[i]
 *   (a Gaussian of sigma 1.5, normalised; the literals are the rule, no exp is evaluated). The five planes are
 *   m in {u, v, u * u, v * v, u * v}; coordinates are clamped to the image: cx(x) = min(max(x, 0), W - 1), cy likewise.
 *     rows:     h_m(y, x) = sum over i = 0..10 of g[i] * m(y, cx(x + i - 5)), added left to right from the first product;
 *     columns:  V_m(y, x) = sum over j = 0..10 of g[j] * h_m(cy(y + j - 5), x), added the same way.
 *     mu = V_u;  mv = V_v;  su = V_uu - (mu * mu);  sv = V_vv - (mv * mv);  suv = V_uv - (mu * mv);  C1 = 0.0001f;  C2 = 0.0009f
 *     ssim = (((2.0f * (mu * mv)) + C1) * ((2.0f * suv) + C2)) / ((((mu * mu) + (mv * mv)) + C1) * ((su + sv) + C2))
 *   Sums. se, ae, rel and ssim are converted to double, one value per pixel, and each is summed in double in this order. The
 *   image is cut into tiles of RBRT_COMPARE_TILE_W x RBRT_COMPARE_TILE_H pixels. A tile's 256 values are indexed
 *   t = ty * RBRT_COMPARE_TILE_W + tx; a pixel outside the image counts as +0.0, and so does an unusable one in se, ae and rel.
 *   They are summed by the pairwise tree: for s = 1, 2, 4, ..., 128: v[i] = v[i] + v[i + s] at every i that is a multiple of
 *   2 s; v[0] is the tile's sum. The tiles' sums, in row-major tile order j, are summed by 256 lanes: lane t adds the tiles
 *   j = t, t + 256, ... in ascending order onto +0.0, and the same tree over t follows. max_abs is the fmaxf of all mx (0 with
 *   no usable pixel); usable and skipped are integer counts.
 * Consequences. X equal to R bit for bit gives all sums 0, max_abs 0 and ssim exactly 1.0f at every pixel: the planes of u
 * and v are then equal, and 2 * (a * a) and (a * a) + (a * a) are the same float. Swapping X and R leaves se, ae, mx and ssim
 * unchanged (every product and sum of the SSIM is symmetric in u and v), but not rel. A pixel's ssim depends only on the
 * 11 x 11 clamped window around it. Squares that overflow give an infinite sum, which is not hidden. */
#define RBRT_COMPARE_TILE_W 16u
#define RBRT_COMPARE_TILE_H 16u
typedef struct rbrt_compare_opts {
    float epsilon;         /* eps of rel: finite, > 0 */
    uint32_t flags;        /* 0 */
    uint32_t reserved[2];  /* 0 */
} rbrt_compare_opts_t;
void rbrt_compare_opts_default(rbrt_compare_opts_t* opts); /* epsilon = 0.01, flags 0 */

typedef struct rbrt_compare_result {  /* what the call found; lives in device memory; 64 bytes */
    double sum_se, sum_ae, sum_rel;   /* over the usable pixels */
    double sum_ssim;                  /* over all pixels */
    float max_abs;
    uint32_t usable, skipped;         /* usable + skipped = width * height */
    uint32_t reserved[5];             /* 0 */
} rbrt_compare_result_t;

typedef struct rbrt_compare_summary { /* the means a host makes of a result: rbrt_compare_summary */
    double mse, mae, relmse, psnr_db, ssim;
} rbrt_compare_summary_t;

/* The bytes of the workspace one rbrt_hip_compare_images call at this size needs: a record of partial sums per tile. 0 where
 * width or height is 0 or width * height >= 2^31. */
size_t rbrt_hip_compare_workspace_bytes(uint32_t width, uint32_t height);

/* The rule on buffers in DEVICE memory, all row-major: d_x and d_ref float[height][width][3] (4-byte alignment is enough; they
 * may be the same buffer), d_rel_map and d_ssim_map float[height][width], d_result one rbrt_compare_result_t (8-byte aligned; a
 * host reads it with a 64-byte copy behind the stream), d_workspace rbrt_hip_compare_workspace_bytes(width, height) bytes of
 * the caller's, 8-byte aligned, needed only with d_result. Any output may be NULL; with all three NULL nothing is launched.
 * Nothing is assumed about what the workspace or the result held before: every byte that is read has been written by this
 * call. Needs no scene, owns no device memory, asynchronous on `stream`.
 * RBRT_ERR_INVALID_ARG, before the device is touched: d_x, d_ref or opts NULL; d_workspace NULL with a d_result; a d_workspace
 * or d_result that is not 8-byte aligned; width or height 0; an epsilon that is not finite or not above 0; a non-zero flag or
 * reserved word; an output that equals an input, another output or the workspace.
 * RBRT_ERR_UNSUPPORTED: width * height >= 2^31. */
int rbrt_hip_compare_images(int device, void* stream, const float* d_x, const float* d_ref, uint32_t width, uint32_t height,
                            const rbrt_compare_opts_t* opts, void* d_workspace, float* d_rel_map, float* d_ssim_map,
                            rbrt_compare_result_t* d_result);

/* Host only, needs no GPU: the means of a result that was copied to the host. With n = 3 * usable:
 * mse = sum_se / n, mae = sum_ae / n, relmse = sum_rel / n, ssim = sum_ssim / (width * height),
 * psnr_db = 10 * log10((peak * peak) / mse), which is +inf at an mse of 0. All five are NaN when usable is 0. */
void rbrt_compare_summary(const rbrt_compare_result_t* result, uint32_t width, uint32_t height, double peak,
                          rbrt_compare_summary_t* out);

/* De-interleave gathered per-rank packed tile buffers (concatenated rank 0..world-1, each
 * rbrt_hip_packed_pixels(...)*3 floats, device memory) into a row-major float[H][W][3] device
 * image and/or its uint8 quantisation. Runs on `stream`. */
int rbrt_hip_unpack_tiles(int device, void* stream, const float* d_gathered, uint32_t width,
                          uint32_t height, uint32_t tile_world, float* d_radiance, uint8_t* d_rgb8);

/* Same, for gathered buffers laid out in equal-size slots: rank r's tiles start at pixel slot
 * r * rank_stride_pixels (what a gather of equal-size tensors produces; rank_stride_pixels >=
 * rbrt_hip_packed_pixels(w, h, 0, world), the largest share). rank_stride_pixels = 0 means tightly packed. */
int rbrt_hip_unpack_tiles_strided(int device, void* stream, const float* d_gathered, uint32_t width,
                                  uint32_t height, uint32_t tile_world, size_t rank_stride_pixels,
                                  float* d_radiance, uint8_t* d_rgb8);

/* What scene_create built (informational; the C++ host's --report prints it). */
typedef struct rbrt_hip_scene_info {
    uint32_t n_spheres, n_meshes;
    uint32_t n_meshes_device_built; /* meshes whose BVH the GPU builder made (the host's SAH builder made the rest) */
    uint32_t bvh_stack_need;        /* traversal stack entries the deepest tree can need */
    uint64_t n_nodes;               /* 128-B BVH nodes, all meshes */
    uint64_t n_triangles;           /* indexed triangle records, all meshes (what the reference's scan can return) */
    uint32_t trace_waves;           /* resident single-wave workgroups of a full trace launch */
    uint32_t lds_bytes_per_wave;    /* LDS each of them uses */
    uint32_t occupancy_api_waves_per_cu; /* hipOccupancyMaxActiveBlocksPerMultiprocessor for that kernel and LDS size */
    uint32_t n_cus;
} rbrt_hip_scene_info_t;
int rbrt_hip_scene_info(rbrt_hip_scene_t* scene, rbrt_hip_scene_info_t* out);

/* Error state of the resident path. rbrt_hip_render_device returns before the kernels have run, so what they
 * detect cannot come back through its return value: a NaN sphere discriminant (the reference panics with
 * "Encountered NAN", sphere.rs:33; here those rays miss that sphere and are counted) or a corrupt path slot
 * (internal error). This call synchronises the device, returns RBRT_ERR_NAN / RBRT_ERR_HIP if either happened in
 * any render on this scene since the previous check, and clears the flags. The one-shot rbrt_hip_render does the
 * same check itself. Call it where the reference's render_scene would have returned (lib.rs:124). */
int rbrt_hip_scene_check(rbrt_hip_scene_t* scene);

/* Counters of the last render on this scene that had RBRT_FLAG_COLLECT_STATS set. */
int rbrt_hip_scene_stats(rbrt_hip_scene_t* scene, rbrt_hip_stats_t* out);

/* Frame pipeline depth of a scene handle: 1..8, or 0 = automatic (the default, or $RBRT_PIPELINE): 8 in a process that
 * has exported GPU_MAX_HW_QUEUES=8 before the HIP runtime started, else 4 (the runtime's four hardware queues run four
 * launches side by side). A launch issued into a stream of launches -- while another launch of the scene is still
 * running -- takes a part of the GPU's wave slots (3 or 4 of a CU's 16 at depth 8, 6 at depth 4), one that finds the
 * GPU idle takes them all, and the sample batches of one blocking call are sized by the batches behind them (api.cpp
 * grid_for). Lanes beyond the four made by rbrt_hip_scene_create, and every lane's sample buffer, are made when a
 * stream of calls is first seen; a blocking caller uses the lanes there are.
 * With depth d > 1 consecutive
 * trace launches -- the sample batches of one render and successive rbrt_hip_render_device calls -- alternate
 * over d internal streams and d sets of work buffers, so that a launch's last, poorly filled waves overlap
 * with the start of the next launch; the per-pixel resolve (and with it every write to the caller's output
 * buffers) stays on the caller's stream, in call order. No counterpart in the reference (its render_scene
 * is one blocking call, lib.rs:75-124); results are identical for every depth. */
int rbrt_hip_scene_set_pipeline(rbrt_hip_scene_t* scene, uint32_t depth);

/* ---- misc ---------------------------------------------------------------------------------- */

void rbrt_render_opts_default(rbrt_render_opts_t* opts); /* spp = 5 (src/main.rs:47), seed = 1 */
int rbrt_hip_device_count(void);                         /* >= 0, or negative status */
const char* rbrt_hip_last_error(void);
int rbrt_hip_abi_version(void);
/* Mask of the RBRT_FLAG_* bits this library honours (bits it does not know are ignored, not rejected): a host tests
 * RBRT_FLAG_THIN_LENS here before it renders with a lens. */
uint32_t rbrt_hip_supported_flags(void);
#ifdef __cplusplus
}
#endif
#endif /* RBRT_HIP_H */
