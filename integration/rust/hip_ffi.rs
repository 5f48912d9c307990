// Shipped as SOURCE ONLY: the build image has no Rust toolchain, so this file has never been compiled here.
// It is the binding INTEGRATION.md describes; the same C ABI (include/rbrt_hip.h) is exercised by the C++ host
// (rbrt_amd/host/render.cpp) and by the ctypes mirror (rbrt_amd/abi.py, checked against the header's layout).
//
// Goes to rbrt_lib/src/hip_ffi.rs (add `pub mod hip_ffi;` to rbrt_lib/src/lib.rs).

use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] #[derive(Copy, Clone)]
pub struct RbrtMaterial { pub kind: i32, pub albedo: [f32; 3], pub param: f32 }   // 0 lambertian, 1 metal, 2 dielectric, 3 emissive
pub const RBRT_MAT_EMISSIVE: i32 = 3;                  // albedo = emitted radiance (no counterpart in the reference)
pub const RBRT_FLAG_CONSTANT_BACKGROUND: u32 = 2;      // RbrtRenderOpts::flags: rays that hit nothing return `bg`
#[repr(C)] #[derive(Copy, Clone)]
pub struct RbrtSphere { pub center: [f32; 3], pub radius: f32, pub mat: RbrtMaterial }
#[repr(C)]
pub struct RbrtMesh {
    pub n_total: u32, pub n_real: u32,
    pub v0x: *const f32, pub v0y: *const f32, pub v0z: *const f32,      // vertices[0][0..3]
    pub e1x: *const f32, pub e1y: *const f32, pub e1z: *const f32,      // edges[0][0..3]
    pub e2x: *const f32, pub e2y: *const f32, pub e2z: *const f32,      // edges[1][0..3]
    pub nx: *const f32, pub ny: *const f32, pub nz: *const f32,         // normals[0..3]
    pub is_padding: *const u8,                                           // Vec<bool> is one byte per element
    pub bbox_lo: [f32; 3], pub bbox_hi: [f32; 3],
    pub mat: RbrtMaterial,
}
#[repr(C)] #[derive(Copy, Clone)]
pub struct RbrtTriangle { pub corners: [[f32; 3]; 3], pub mat: RbrtMaterial }       // BasicTriangle, triangle.rs:9-34
#[repr(C)]
pub struct RbrtScene {
    pub n_spheres: u32, pub spheres: *const RbrtSphere, pub n_meshes: u32, pub meshes: *const RbrtMesh,
    pub n_triangles: u32, pub triangles: *const RbrtTriangle,
    pub element_order: *const u32,   // null, or Scene::elements order: index, bit 31 set for a triangle (ABI version 2)
}
#[repr(C)]
pub struct RbrtCamera {
    pub position: [f32; 3], pub right: [f32; 3], pub up: [f32; 3], pub img_center_point: [f32; 3],
    pub mm_per_pix_hor: f32, pub mm_per_pix_vert: f32, pub img_width_pix: u32, pub img_height_pix: u32,
}
pub const RBRT_FLAG_THIN_LENS: u32 = 4;                // RbrtRenderOpts::flags: `cam` points at RbrtCameraLens::cam (defocus)
#[repr(C)]
pub struct RbrtCameraLens {                            // rbrt_camera_lens_t; pass &lens.cam with RBRT_FLAG_THIN_LENS
    pub cam: RbrtCamera,
    pub lens_u: [f32; 3], pub lens_v: [f32; 3],        // lens half-axes in scene units (radius applied)
    pub focus_scale: f32,                              // focus surface = image plane scaled about cam.position by this
    pub reserved: u32,                                 // 0
}
#[repr(C)] #[derive(Copy, Clone)]
pub struct RbrtMeshNormals {                           // rbrt_mesh_normals_t: corner normals of every SoA entry (n_total each)
    pub n0x: *const f32, pub n0y: *const f32, pub n0z: *const f32,      // at vertices[0]
    pub n1x: *const f32, pub n1y: *const f32, pub n1z: *const f32,      // at v0 + e1
    pub n2x: *const f32, pub n2y: *const f32, pub n2z: *const f32,      // at v0 + e2; all nine null = a flat mesh
}
#[repr(C)]
pub struct RbrtSceneShading {                          // rbrt_scene_shading_t: smooth shading of meshes
    pub n_meshes: u32,                                 // == RbrtScene::n_meshes
    pub reserved: u32,                                 // 0
    pub meshes: *const RbrtMeshNormals,                // one per mesh, or null = every mesh flat
}
#[repr(C)] #[derive(Copy, Clone)]
pub struct RbrtPattern {                               // rbrt_pattern_t: a solid pattern of one lambertian object, 32 bytes
    pub kind: u32,                                     // 0 none, 1 checker
    pub albedo2: [f32; 3],                             // the odd cells' albedo; the even cells have the material's own
    pub origin: [f32; 3],
    pub size: f32,                                     // a cell's edge, world units
}
#[repr(C)]
pub struct RbrtScenePatterns {                         // rbrt_scene_patterns_t
    pub n_objects: u32,                                // == n_spheres + n_triangles + n_meshes
    pub reserved: u32,                                 // 0
    pub objects: *const RbrtPattern,                   // by object id, or null = none
}
#[repr(C)]
pub struct RbrtRenderOpts {
    pub spp: u32, pub max_depth: u32, pub min_dist: f32, pub max_dist: f32, pub bg: [f32; 3],
    pub seed: u64, pub tile_rank: u32, pub tile_world: u32, pub flags: u32, pub reserved: u32,
}

#[repr(C)]
pub struct RbrtTonemapOpts {                           // rbrt_tonemap_opts_t: the display transform (exposure, tone curve)
    pub curve: u32,                                    // 0 linear, 1 extended Reinhard, 2 ACES (Narkowicz)
    pub exposure: f32,                                 // > 0: the multiplier; 0: automatic, from the luminance histogram
    pub key: f32, pub key_permille: u32,               // automatic exposure: the luminance at this rank is mapped to key
    pub white: f32, pub white_permille: u32,           // Reinhard's white point (> 0), or 0: the luminance at this rank
    pub reserved: [u32; 2],                            // 0
}
#[repr(C)] #[derive(Copy, Clone, Default)]
pub struct RbrtTonemapResult {                         // rbrt_tonemap_result_t: 32 bytes, 16 KiB into the device workspace
    pub exposure: f32, pub white: f32, pub l_key: f32, pub l_white: f32, pub counted: u32, pub reserved: u32, pub pixels: u64,
}
pub const RBRT_TONEMAP_WORKSPACE_BYTES: usize = 4096 * 4 + 32;

#[repr(C)]
pub struct RbrtGlareOpts {                             // rbrt_glare_opts_t: glare, a pyramid bloom in front of the display transform
    pub threshold: f32,                                // luminance above which a pixel is bright; >= 0
    pub intensity: f32,                                // the share of the bright light that is moved; in (0, 1]
    pub levels: u32,                                   // 1..=RBRT_GLARE_MAX_LEVELS
    pub spread: f32,                                   // weight of each coarser level against the one below it; >= 0
    pub reserved: [u32; 4],                            // 0
}
pub const RBRT_GLARE_MAX_LEVELS: u32 = 8;

#[repr(C)]
pub struct RbrtShutter {                               // rbrt_shutter_t: the camera's translation while the shutter is open, 16 bytes
    pub travel: [f32; 3],                              // scene units; finite
    pub reserved: u32,                                 // 0
}

#[repr(C)]
pub struct RbrtMotion {                                // rbrt_motion_t: a travel per sphere while the shutter is open, 16 bytes
    pub n_spheres: u32,                                // the scene's sphere count
    pub reserved: u32,                                 // 0
    pub travel: *const f32,                            // [n_spheres][3], scene units; finite; copied by the call
}

#[repr(C)]
pub struct RbrtMeshMotion {                            // rbrt_mesh_motion_t: a travel per mesh while the shutter is open, 16 bytes
    pub n_meshes: u32,                                 // the scene's mesh count
    pub reserved: u32,                                 // 0
    pub travel: *const f32,                            // [n_meshes][3], scene units; finite; copied by the call
}

#[link(name = "rbrt_hip")]
extern "C" {
    pub fn rbrt_render_opts_default(opts: *mut RbrtRenderOpts);
    pub fn rbrt_hip_render(cam: *const RbrtCamera, scene: *const RbrtScene, opts: *const RbrtRenderOpts,
                           out_radiance: *mut f32, out_rgb8: *mut u8) -> c_int;
    pub fn rbrt_hip_render_shaded(cam: *const RbrtCamera, scene: *const RbrtScene, shading: *const RbrtSceneShading,
                                  opts: *const RbrtRenderOpts, out_radiance: *mut f32, out_rgb8: *mut u8) -> c_int;
    // solid patterns: a host detects the capability by the symbol (no flag bit); patterns = null is rbrt_hip_render_shaded
    pub fn rbrt_hip_render_patterned(cam: *const RbrtCamera, scene: *const RbrtScene, shading: *const RbrtSceneShading,
                                     patterns: *const RbrtScenePatterns, opts: *const RbrtRenderOpts, out_radiance: *mut f32,
                                     out_rgb8: *mut u8) -> c_int;
    pub fn rbrt_hip_scene_create_patterned(scene: *const RbrtScene, shading: *const RbrtSceneShading, patterns: *const RbrtScenePatterns,
                                           device: c_int, out: *mut *mut c_void) -> c_int;
    // the camera shutter: a state of the handle, like the environment; shutter = null clears it. Detected by the symbol (no flag bit)
    pub fn rbrt_hip_scene_set_shutter(scene: *mut c_void, shutter: *const RbrtShutter) -> c_int;
    // moving spheres: a state of the handle that shares the shutter's draw; motion = null clears it. Detected by the symbol
    pub fn rbrt_hip_scene_set_motion(scene: *mut c_void, motion: *const RbrtMotion) -> c_int;
    // animation: the phase of the handle's motion (a sample with the draw t sees sphere i at center_i + (phase + t) * travel_i),
    // the motion buffer beside the feature buffers, and the accumulation that follows the spheres. Each detected by its symbol
    pub fn rbrt_hip_scene_set_motion_phase(scene: *mut c_void, phase: f32) -> c_int;
    // moving meshes: a state of the handle beside the spheres' motion, on the same draw and phase (wherever a path tests mesh m it
    // reads the origin o - (phase + t) * travel_m); motion = null clears it. Detected by the symbol
    pub fn rbrt_hip_scene_set_mesh_motion(scene: *mut c_void, motion: *const RbrtMeshMotion) -> c_int;
    pub fn rbrt_hip_render_features_motion(scene: *mut c_void, cam: *const RbrtCamera, opts: *const RbrtRenderOpts, fopts: *const c_void,
                                           stream: *mut c_void, d_albedo: *mut f32, d_normal: *mut f32, d_depth: *mut f32,
                                           d_coverage: *mut f32, d_object: *mut i32, d_motion: *mut f32) -> c_int;
    pub fn rbrt_hip_temporal_accumulate_moving(device: c_int, stream: *mut c_void, d_a: *const f32, d_b: *const f32, d_normal: *const f32,
                                               d_depth: *const f32, d_coverage: *const f32, d_motion: *const f32, phase_step: f32,
                                               cam: *const RbrtCamera, cam_prev: *const RbrtCamera, opts: *const c_void,
                                               d_history_in: *const c_void, d_history_out: *mut c_void, d_out_a: *mut f32,
                                               d_out_b: *mut f32, d_out_length: *mut f32) -> c_int;
    // device pointers; needs no scene handle. A host detects it by the symbol (the ABI version stays 2).
    pub fn rbrt_tonemap_opts_default(opts: *mut RbrtTonemapOpts);
    pub fn rbrt_hip_tonemap(device: c_int, stream: *mut c_void, d_radiance: *const f32, n_pixels: usize, opts: *const RbrtTonemapOpts,
                            d_workspace: *mut c_void, d_out_radiance: *mut f32, d_rgb8: *mut u8) -> c_int;
    // device pointers; needs no scene handle; the workspace is the caller's, rbrt_hip_glare_workspace_bytes(...) bytes, 16-byte aligned
    pub fn rbrt_glare_opts_default(opts: *mut RbrtGlareOpts);
    pub fn rbrt_hip_glare_workspace_bytes(width: u32, height: u32, levels: u32) -> usize;
    pub fn rbrt_hip_glare(device: c_int, stream: *mut c_void, d_radiance: *const f32, width: u32, height: u32, opts: *const RbrtGlareOpts,
                          d_workspace: *mut c_void, d_out_radiance: *mut f32, d_rgb8: *mut u8) -> c_int;
    pub fn rbrt_hip_last_error() -> *const c_char;
    pub fn rbrt_hip_device_count() -> c_int;
    pub fn rbrt_hip_supported_flags() -> u32;           // test RBRT_FLAG_THIN_LENS here before relying on it
}
