"""ctypes mirror of include/vimg_scene.h, include/vimg_host.h, include/vimg_hip.h, include/vimg_filter.h,
include/vimg_temporal.h, include/vimg_varfilter.h, include/vimg_moments.h, include/vimg_infill.h, include/vimg_wtemporal.h,
include/vimg_antilag.h, include/vimg_motion.h, include/vimg_despeckle.h, include/vimg_exposure.h, include/vimg_demand.h and
include/vimg_rectify.h.

Only declarations live here: struct layouts, library loading and argtypes.  The product
libraries are loaded from ``v-img_amd/lib`` (built in-tree by ``make``); a missing library is an
error, never a fallback (the HIP path must fail loudly when its extension is absent).
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
REPO_ROOT = os.path.dirname(PKG_DIR)

NO_UV = 255
MAX_UV_SETS = 4
MAX_MIP_LEVELS = 15

INTEGRATOR_S_NORMAL, INTEGRATOR_G_NORMAL, INTEGRATOR_MATERIAL, INTEGRATOR_MIS = 0, 1, 2, 3
INTEGRATOR_ALBEDO, INTEGRATOR_NORMAL, INTEGRATOR_DEPTH, INTEGRATOR_POSITION, INTEGRATOR_UV, INTEGRATOR_COVERAGE = 4, 5, 6, 7, 8, 9
INTEGRATORS = {"s_normal": 0, "g_normal": 1, "material": 2, "mis": 3,
               # first-hit feature integrators of the HIP library (include/vimg_hip.h, beside vimg_hip_render)
               "albedo": 4, "normal": 5, "depth": 6, "position": 7, "uv": 8, "coverage": 9}
FEATURES = ("albedo", "normal", "depth", "position", "uv", "coverage")
PRIM_TRIANGLE, PRIM_SPHERE = 0, 1
MAT_LAMBERTIAN, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_PRINCIPLED = 0, 1, 2, 3
TEX_CONST, TEX_CHECKER, TEX_IMAGE = 0, 1, 2
WRAP_CLAMP, WRAP_MIRROR, WRAP_REPEAT = 0, 1, 2
LIGHT_PRIM, LIGHT_BACKGROUND = 0, 1
BG_CONST, BG_ENVMAP = 0, 1
BVH_BINNED, BVH_SWEEP = 0, 1

f32, u32, i32, u64, i64 = C.c_float, C.c_uint32, C.c_int32, C.c_uint64, C.c_int64


class Camera(C.Structure):
    _fields_ = [("cam_to_world", f32 * 16), ("vfov_deg", f32), ("res_x", i32), ("res_y", i32),
                ("aperture_radius", f32), ("focal_dist", f32)]


class Prim(C.Structure):
    _fields_ = [("type", u32), ("index", u32)]


class Mesh(C.Structure):
    _fields_ = [("first_vertex", u32), ("num_vertices", u32), ("has_normals", u32),
                ("num_uv_sets", u32), ("uv_offset", u32 * MAX_UV_SETS), ("color_tex_uv", u32),
                ("normal_tex_uv", u32), ("metallic_roughness_tex_uv", u32), ("material", u32)]


class Sphere(C.Structure):
    _fields_ = [("center", f32 * 3), ("radius", f32), ("material", u32)]


class Material(C.Structure):
    _fields_ = [("type", u32), ("tex", i32), ("mr_tex", i32), ("normal_map", i32),
                ("emit", f32 * 3), ("ior", f32), ("metallic_factor", f32),
                ("roughness_factor", f32), ("specular_transmission", f32), ("subsurface", f32),
                ("specular", f32), ("specular_tint", f32), ("anisotropic", f32), ("sheen", f32),
                ("sheen_tint", f32), ("clearcoat", f32), ("clearcoat_gloss", f32), ("eta", f32)]


class Texture(C.Structure):
    _fields_ = [("type", u32), ("col_a", f32 * 3), ("col_b", f32 * 3), ("width", u32),
                ("height", u32), ("num_levels", u32), ("wrap_u", u32), ("wrap_v", u32),
                ("level_offset", u64 * MAX_MIP_LEVELS)]


class TextureRG(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("wrap_u", u32), ("wrap_v", u32),
                ("offset", u64)]


class Light(C.Structure):
    _fields_ = [("type", u32), ("prim", u32)]


class Background(C.Structure):
    _fields_ = [("type", u32), ("col", f32 * 3), ("env_tex", i32), ("world_to_env", f32 * 16),
                ("env_to_world", f32 * 16), ("radiance_scale", f32), ("row_cdf_offset", u64),
                ("col_cdf_offset", u64)]


class BVHNode(C.Structure):
    _fields_ = [("first_index", u32), ("obj_count", u32)]


class BVH(C.Structure):
    _fields_ = [("num_nodes", u32), ("max_depth", u32), ("nodes", C.POINTER(BVHNode)),
                ("bb_mins_maxes", C.POINTER(f32)), ("obj_indices", C.POINTER(u32))]


class Scene(C.Structure):
    _fields_ = [
        ("camera", Camera), ("background", Background),
        ("num_prims", u32), ("prims", C.POINTER(Prim)),
        ("num_tris", u32), ("tri_indices", C.POINTER(u32)), ("tri_mesh", C.POINTER(u32)),
        ("num_meshes", u32), ("meshes", C.POINTER(Mesh)),
        ("num_vertices", u32), ("vertices", C.POINTER(f32)), ("normals", C.POINTER(f32)),
        ("num_uvs", u64), ("uvs", C.POINTER(f32)),
        ("num_spheres", u32), ("spheres", C.POINTER(Sphere)),
        ("num_materials", u32), ("materials", C.POINTER(Material)),
        ("num_textures", u32), ("textures", C.POINTER(Texture)),
        ("num_texels", u64), ("texels", C.POINTER(f32)),
        ("num_rg_textures", u32), ("rg_textures", C.POINTER(TextureRG)),
        ("num_rg_texels", u64), ("rg_texels", C.POINTER(f32)),
        ("num_lights", u32), ("lights", C.POINTER(Light)),
        ("num_cdf", u64), ("cdf_pool", C.POINTER(f32)),
        ("bvh", BVH),
    ]


class RenderParams(C.Structure):
    _fields_ = [("integrator", u32), ("samples", u32), ("depth", u32), ("tile_rank", u32),
                ("tile_world", u32)]


class RenderStats(C.Structure):
    _fields_ = [("paths", u64), ("closest_rays", u64), ("shadow_rays", u64),
                ("internal_visits", u64), ("leaf_visits", u64), ("prim_tests", u64),
                ("sphere_tests", u64), ("nan_samples", u64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    @property
    def rays(self):
        return int(self.closest_rays) + int(self.shadow_rays)


class _Sized:
    """Mixin of the structs that open with ``struct_size``: it is filled at construction."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(type(self))


class TextureImage(C.Structure):
    """VimgTextureImage (include/vimg_hip.h): new level-0 texels (a DEVICE pointer) for one resident IMAGE texture."""
    _fields_ = [("texture", u32), ("reserved", u32), ("level0", C.c_void_p)]


class GeometryUpdateV1(_Sized, C.Structure):
    """The first 32 bytes of VimgGeometryUpdate, the whole struct before the material update: what an older caller
    passes (struct_size 32)."""
    _fields_ = [("struct_size", u32), ("vertices", C.c_void_p), ("normals", C.c_void_p), ("spheres", C.c_void_p)]


class GeometryUpdate(_Sized, C.Structure):
    """VimgGeometryUpdate (include/vimg_hip.h): device pointers to float32 tables, then host pointers to the new
    material, texture, light and background tables and the image list; NULL / 0 = unchanged."""
    _fields_ = GeometryUpdateV1._fields_ + [
        ("materials", C.POINTER(Material)), ("textures", C.POINTER(Texture)), ("lights", C.POINTER(Light)),
        ("num_lights", u32), ("set_lights", u32), ("background", C.POINTER(Background)),
        ("images", C.POINTER(TextureImage)), ("num_images", u32), ("reserved", u32)]


BUILDER_PLOC, BUILDER_LBVH = 0, 1
BUILDERS = {"ploc": BUILDER_PLOC, "lbvh": BUILDER_LBVH}


class RebuildOptions(_Sized, C.Structure):
    """VimgRebuildOptions (include/vimg_hip.h): the builder of vimg_hip_scene_rebuild_bvh."""
    _fields_ = [("struct_size", u32), ("builder", u32)]


class Ray(C.Structure):
    """VimgRay (include/vimg_hip.h): one query ray, 32 B."""
    _fields_ = [("org", f32 * 3), ("t_min", f32), ("dir", f32 * 3), ("t_max", f32)]


class RayHit(C.Structure):
    """VimgRayHit: closest hit of one ray, 16 B; prim == NO_HIT for a miss."""
    _fields_ = [("t", f32), ("prim", u32), ("b1", f32), ("b2", f32)]


class HitInfo(C.Structure):
    """VimgHitInfo: the hit's record, 48 B."""
    _fields_ = [("p", f32 * 3), ("ns", f32 * 3), ("ng", f32 * 3), ("uv", f32 * 2), ("mat", u32)]


NO_HIT = 0xFFFFFFFF

OPT_AUTO = -1
SCHED_LANE, SCHED_POOL, SCHED_STAGE, SCHED_POOL4, SCHED_POOL4G, SCHED_CU = 1, 2, 3, 4, 5, 6
SCHEDULERS = {"lane": SCHED_LANE, "pool": SCHED_POOL, "stage": SCHED_STAGE, "pool4": SCHED_POOL4, "pool4g": SCHED_POOL4G, "cu": SCHED_CU}


class HipOptions(C.Structure):
    """VimgHipOptions (include/vimg_hip.h): every field -1 = the library's policy."""
    _fields_ = [("struct_size", u32), ("scheduler", i32), ("waves_per_simd", i32),
                ("lds_budget_kb", i32), ("pool_slots", i32), ("pool_segments", i32),
                ("pool_refill", i32), ("pool_vbatch", i32), ("pool_classes", i32),
                ("pool_starve", i32), ("pool_boxmin", i32), ("lds_leaf", i32),
                ("stage_slots", i32), ("stage_seg_len", i32), ("stage_wchunk", i32),
                ("stage_walk_quota", i32), ("pool4_rays", i32), ("lds_stack", i32), ("pool_gbreak", i32),
                ("cu_waves", i32), ("cu_walkers", i32), ("cu_flex", i32), ("cu_lowwater", i32), ("cu_patience", i32),
                ("cu_join", i32), ("cu_sleep", i32)]

    def __init__(self, **kw):
        super().__init__()
        self.struct_size = C.sizeof(HipOptions)
        for name, _ in self._fields_[1:]:
            setattr(self, name, OPT_AUTO)
        for k, v in kw.items():
            if k == "scheduler" and isinstance(v, str):
                v = SCHEDULERS[v]
            if k not in dict(self._fields_):
                raise TypeError(f"unknown option {k}")
            setattr(self, k, v)


PScene = C.POINTER(Scene)
PParams = C.POINTER(RenderParams)
PStats = C.POINTER(RenderStats)
Pf32 = C.POINTER(f32)

# name -> (restype, argtypes); also the list of symbols include/vimg_host.h declares
HOST_SYMBOLS = {
    "vimg_host_scene_from_json_file": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "vimg_host_scene_from_json_text": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "vimg_host_scene_new": (C.c_void_p, []),
    "vimg_host_scene_free": (None, [C.c_void_p]),
    "vimg_host_set_camera_lookat": (None, [C.c_void_p, Pf32, Pf32, Pf32, f32, C.c_int, C.c_int,
                                           f32, f32]),
    "vimg_host_camera_lookat": (None, [Pf32, Pf32, Pf32, f32, C.c_int, C.c_int, f32, f32, C.POINTER(Camera)]),
    "vimg_host_set_render_defaults": (None, [C.c_void_p, u32, u32, u32]),
    "vimg_host_add_texture_const": (C.c_int, [C.c_void_p, Pf32]),
    "vimg_host_add_texture_checker": (C.c_int, [C.c_void_p, u32, u32, Pf32, Pf32]),
    "vimg_host_add_texture_image": (C.c_int, [C.c_void_p, u32, u32, Pf32, u32, u32]),
    "vimg_host_add_texture_rg": (C.c_int, [C.c_void_p, u32, u32, Pf32, u32, u32]),
    "vimg_host_add_material": (C.c_int, [C.c_void_p, C.POINTER(Material)]),
    "vimg_host_add_mesh": (C.c_int, [C.c_void_p, u32, Pf32, Pf32, u32, C.POINTER(Pf32), u32,
                                     C.POINTER(u32), u32, u32, u32, u32]),
    "vimg_host_add_quad": (C.c_int, [C.c_void_p, Pf32, u32]),
    "vimg_host_add_sphere": (C.c_int, [C.c_void_p, Pf32, f32, u32]),
    "vimg_host_set_background_const": (None, [C.c_void_p, Pf32, C.c_int]),
    "vimg_host_set_background_envmap": (C.c_int, [C.c_void_p, C.c_int, Pf32, Pf32, f32]),
    "vimg_host_set_precompute": (None, [C.c_void_p, C.c_void_p]),
    "vimg_host_srgb8_lut": (None, [Pf32]),
    "vimg_host_srgb8_to_linear": (None, [C.POINTER(C.c_uint8), C.c_uint64, Pf32]),
    "vimg_host_rgb8_to_normal": (None, [C.POINTER(C.c_uint8), C.c_uint64, f32, Pf32]),
    "vimg_host_build_bvh": (C.c_int, [C.c_void_p, C.c_int]),
    "vimg_host_build_bvh_with": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vimg_host_set_vertices": (C.c_int, [C.c_void_p, Pf32, Pf32]),
    "vimg_host_set_spheres": (C.c_int, [C.c_void_p, Pf32]),
    "vimg_host_refit_bvh": (C.c_int, [C.c_void_p]),
    "vimg_host_set_materials": (C.c_int, [C.c_void_p, C.POINTER(Material)]),
    "vimg_host_set_texture_colors": (C.c_int, [C.c_void_p, u32, Pf32, Pf32, u32, u32]),
    "vimg_host_set_texture_image": (C.c_int, [C.c_void_p, u32, Pf32]),
    "vimg_host_set_background": (C.c_int, [C.c_void_p, Pf32, Pf32, Pf32, f32]),
    "vimg_host_scene_view": (PScene, [C.c_void_p]),
    "vimg_host_default_params": (None, [C.c_void_p, PParams]),
    "vimg_host_tonemap_to_rgb8": (C.c_int, [Pf32, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_uint8)]),
    "vimg_host_write_png": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "vimg_host_last_error": (C.c_char_p, []),
}

# the list of symbols include/vimg_hip.h declares
HIP_SYMBOLS = {
    "vimg_hip_init": (C.c_int, [C.c_int]),
    "vimg_hip_device_count": (C.c_int, []),
    "vimg_hip_options_default": (None, [C.POINTER(HipOptions)]),
    "vimg_hip_scene_upload": (C.c_int, [PScene, C.POINTER(C.c_void_p)]),
    "vimg_hip_scene_upload_opts": (C.c_int, [PScene, C.POINTER(HipOptions), C.POINTER(C.c_void_p)]),
    "vimg_hip_scene_free": (C.c_int, [C.c_void_p]),
    "vimg_hip_scene_update_geometry": (C.c_int, [C.c_void_p, C.POINTER(GeometryUpdate), C.c_void_p]),
    "vimg_hip_scene_set_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "vimg_hip_scene_rebuild_bvh": (C.c_int, [C.c_void_p, C.POINTER(RebuildOptions), C.c_void_p]),
    "vimg_hip_scene_bvh_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "vimg_hip_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_hip_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "vimg_hip_camera_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "vimg_hip_shard_pixels": (i64, [C.c_void_p, PParams]),
    "vimg_hip_render": (C.c_int, [C.c_void_p, PParams, C.c_void_p, C.c_void_p, PStats]),
    "vimg_hip_render_async": (C.c_int, [C.c_void_p, PParams, C.c_void_p, C.c_void_p]),
    "vimg_hip_progressive_create": (C.c_int, [C.c_void_p, PParams, C.POINTER(C.c_void_p)]),
    "vimg_hip_progressive_render": (C.c_int, [C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, PStats]),
    "vimg_hip_progressive_samples": (C.c_uint64, [C.c_void_p]),
    "vimg_hip_progressive_reset": (C.c_int, [C.c_void_p]),
    "vimg_hip_progressive_free": (C.c_int, [C.c_void_p]),
    "vimg_hip_progressive_render_masked": (C.c_int, [C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, PStats]),
    "vimg_hip_progressive_launches": (C.c_uint64, [C.c_void_p]),
    "vimg_hip_progressive_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_hip_progressive_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_hip_progressive_select": (C.c_int, [C.c_void_p, f32, u32, C.c_void_p, C.c_void_p, C.POINTER(u32)]),
    "vimg_hip_check": (C.c_int, [C.c_void_p]),
    "vimg_hip_render_to_host": (C.c_int, [C.c_void_p, PParams, Pf32, PStats]),
    "vimg_hip_trace_pixel": (C.c_int, [C.c_void_p, PParams, C.c_int, C.c_int, Pf32]),
    "vimg_hip_render_heatmap": (C.c_int, [C.c_void_p, PParams, f32, C.c_void_p, C.c_void_p]),
    "vimg_hip_assemble_shards": (C.c_int, [C.c_void_p, u32, i64, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "vimg_hip_time_renders": (C.c_int, [C.c_void_p, PParams, C.c_void_p, C.c_int, Pf32]),
    "vimg_hip_post_rgb8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "vimg_hip_mip_chain_texels": (C.c_uint64, [u32, u32, C.POINTER(u32)]),
    "vimg_hip_build_mip_chain": (C.c_int, [u32, u32, Pf32, u32, u32, Pf32]),
    "vimg_hip_build_env_cdfs": (C.c_int, [Pf32, u32, u32, Pf32, Pf32]),
    "vimg_hip_lut8_to_float": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint64, Pf32, Pf32]),
    "vimg_hip_rgb8_to_normal": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint64, f32, Pf32]),
    "vimg_hip_build_lbvh": (C.c_int, [u32, Pf32, C.POINTER(u32), C.POINTER(u32), C.c_void_p, Pf32,
                                     C.POINTER(u32)]),
    "vimg_hip_build_ploc": (C.c_int, [u32, Pf32, C.POINTER(u32), C.POINTER(u32), C.c_void_p, Pf32,
                                     C.POINTER(u32)]),
    "vimg_hip_scene_bytes": (i64, [C.c_void_p]),
    "vimg_hip_scene_kernel": (C.c_char_p, [C.c_void_p]),
    "vimg_hip_launch_kernel": (C.c_char_p, [C.c_void_p, PParams]),
    "vimg_hip_last_error": (C.c_char_p, []),
}

# what the library exports without declaring it in include/vimg_hip.h: the unit-level test hook (csrc/vimg_hip.hip)
HIP_TEST_SYMBOLS = {
    "vimg_hip_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_int, Pf32, Pf32]),
}


class FilterFrames(_Sized, C.Structure):
    """VimgFilterFrames (include/vimg_filter.h): the frames of one picture, DEVICE pointers to float32 triples."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("color", C.c_void_p),
                ("normal", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p), ("albedo", C.c_void_p)]


class AtrousParams(C.Structure):
    """VimgAtrousParams (include/vimg_filter.h); vimg_filter_atrous_defaults fills it."""
    _fields_ = [("struct_size", u32), ("iterations", u32), ("sigma_color", f32), ("sigma_normal", f32),
                ("sigma_plane", f32), ("albedo_floor", f32)]


# the list of symbols include/vimg_filter.h declares: libvimg_filter.so, a library of its own beside libvimg_hip.so
FILTER_SYMBOLS = {
    "vimg_filter_atrous_defaults": (None, [C.POINTER(AtrousParams)]),
    "vimg_filter_atrous_workspace": (C.c_uint64, [u32, u32]),
    "vimg_filter_atrous": (C.c_int, [C.POINTER(FilterFrames), C.POINTER(AtrousParams), C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p]),
    "vimg_filter_last_error": (C.c_char_p, []),
}


class TemporalFrames(_Sized, C.Structure):
    """VimgTemporalFrames (include/vimg_temporal.h): the current picture, DEVICE pointers to float32 triples."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("color", C.c_void_p),
                ("normal", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p)]


class TemporalParams(C.Structure):
    """VimgTemporalParams (include/vimg_temporal.h); vimg_temporal_defaults fills it."""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("max_history", f32), ("current_weight", f32),
                ("sigma_normal", f32), ("sigma_plane", f32)]


TEMPORAL_HISTORY_PER_PIXEL = 48

# the list of symbols include/vimg_temporal.h declares: libvimg_temporal.so, the third scene-free library
TEMPORAL_SYMBOLS = {
    "vimg_temporal_defaults": (None, [C.POINTER(TemporalParams)]),
    "vimg_temporal_history_bytes": (C.c_uint64, [u32, u32]),
    "vimg_temporal_accumulate": (C.c_int, [C.POINTER(TemporalFrames), C.c_void_p, Pf32, C.POINTER(TemporalParams), C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "vimg_temporal_last_error": (C.c_char_p, []),
}


class VarFilterFrames(_Sized, C.Structure):
    """VimgVarFilterFrames (include/vimg_varfilter.h): VimgFilterFrames and the per-pixel variance frame (float32)."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("color", C.c_void_p),
                ("normal", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p), ("albedo", C.c_void_p),
                ("variance", C.c_void_p)]


class VarFilterParams(_Sized, C.Structure):
    """VimgVarFilterParams (include/vimg_varfilter.h); vimg_varfilter_defaults fills it."""
    _fields_ = [("struct_size", u32), ("iterations", u32), ("sigma_luminance", f32), ("sigma_normal", f32),
                ("sigma_plane", f32), ("albedo_floor", f32), ("variance_floor", f32)]


# the list of symbols include/vimg_varfilter.h declares: libvimg_varfilter.so, the variance-guided a-trous filter
VARFILTER_SYMBOLS = {
    "vimg_varfilter_defaults": (None, [C.POINTER(VarFilterParams)]),
    "vimg_varfilter_workspace": (C.c_uint64, [u32, u32]),
    "vimg_varfilter_atrous": (C.c_int, [C.POINTER(VarFilterFrames), C.POINTER(VarFilterParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.c_void_p]),
    "vimg_varfilter_variance": (C.c_int, [u32, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_varfilter_last_error": (C.c_char_p, []),
}


class MomentsFrames(_Sized, C.Structure):
    """VimgMomentsFrames (include/vimg_moments.h): VimgTemporalFrames and the per-pixel variance frame (float32)."""
    _fields_ = TemporalFrames._fields_ + [("variance", C.c_void_p)]


class MomentsParams(_Sized, C.Structure):
    """VimgMomentsParams (include/vimg_moments.h): VimgTemporalParams and min_history; vimg_moments_defaults fills it."""
    _fields_ = TemporalParams._fields_ + [("min_history", f32)]


MOMENTS_HISTORY_PER_PIXEL = 64

# the list of symbols include/vimg_moments.h declares: libvimg_moments.so, temporal accumulation with luminance moments
MOMENTS_SYMBOLS = {
    "vimg_moments_defaults": (None, [C.POINTER(MomentsParams)]),
    "vimg_moments_history_bytes": (C.c_uint64, [u32, u32]),
    "vimg_moments_accumulate": (C.c_int, [C.POINTER(MomentsFrames), C.c_void_p, Pf32, C.POINTER(MomentsParams), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_moments_last_error": (C.c_char_p, []),
}


class InfillFrames(_Sized, C.Structure):
    """VimgInfillFrames (include/vimg_infill.h): VimgFilterFrames and the per-pixel sample count (uint32)."""
    _fields_ = FilterFrames._fields_ + [("count", C.c_void_p)]


class InfillParams(_Sized, C.Structure):
    """VimgInfillParams (include/vimg_infill.h); vimg_infill_defaults fills it."""
    _fields_ = [("struct_size", u32), ("radius", u32), ("sigma_normal", f32), ("sigma_plane", f32), ("albedo_floor", f32)]


INFILL_WORKSPACE_PER_PIXEL = 48
INFILL_MAX_RADIUS = 4
INFILL_SAMPLED, INFILL_GUIDED, INFILL_UNGUIDED, INFILL_HOLE = 0, 1, 2, 3

# the list of symbols include/vimg_infill.h declares: libvimg_infill.so, reconstruction of sparsely sampled frames
INFILL_SYMBOLS = {
    "vimg_infill_defaults": (None, [C.POINTER(InfillParams)]),
    "vimg_infill_workspace": (C.c_uint64, [u32, u32]),
    "vimg_infill_reconstruct": (C.c_int, [C.POINTER(InfillFrames), C.POINTER(InfillParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.c_void_p]),
    "vimg_infill_last_error": (C.c_char_p, []),
}


class WTemporalFrames(_Sized, C.Structure):
    """VimgWTemporalFrames (include/vimg_wtemporal.h): VimgTemporalFrames and the per-pixel weight frame (float32)."""
    _fields_ = TemporalFrames._fields_ + [("weight", C.c_void_p)]


class WTemporalParams(_Sized, C.Structure):
    """VimgWTemporalParams (include/vimg_wtemporal.h): VimgTemporalParams without current_weight;
    vimg_wtemporal_defaults fills it."""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("max_history", f32), ("sigma_normal", f32), ("sigma_plane", f32)]


WTEMPORAL_DEAD, WTEMPORAL_STARTED, WTEMPORAL_BLENDED, WTEMPORAL_CARRIED, WTEMPORAL_SHOWN = 0, 1, 2, 3, 4

# the list of symbols include/vimg_wtemporal.h declares: libvimg_wtemporal.so, temporal accumulation with per-pixel
# weights on libvimg_temporal's history (TEMPORAL_HISTORY_PER_PIXEL)
WTEMPORAL_SYMBOLS = {
    "vimg_wtemporal_defaults": (None, [C.POINTER(WTemporalParams)]),
    "vimg_wtemporal_accumulate": (C.c_int, [C.POINTER(WTemporalFrames), C.c_void_p, Pf32, C.POINTER(WTemporalParams), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_wtemporal_last_error": (C.c_char_p, []),
}


class AntilagFrames(_Sized, C.Structure):
    """VimgAntilagFrames (include/vimg_antilag.h): VimgTemporalFrames, the CURRENT picture a history is compared with."""
    _fields_ = TemporalFrames._fields_


class AntilagParams(_Sized, C.Structure):
    """VimgAntilagParams (include/vimg_antilag.h); vimg_antilag_defaults fills it."""
    _fields_ = [("struct_size", u32), ("radius", u32), ("t_low", f32), ("t_high", f32), ("min_matches", f32),
                ("sigma_normal", f32), ("sigma_plane", f32)]


ANTILAG_WORKSPACE_PER_PIXEL = 8
ANTILAG_MAX_RADIUS = 8

# the list of symbols include/vimg_antilag.h declares: libvimg_antilag.so, which shortens a history (the first three
# planes: TEMPORAL_HISTORY_PER_PIXEL) where the current picture disagrees with it
ANTILAG_SYMBOLS = {
    "vimg_antilag_defaults": (None, [C.POINTER(AntilagParams)]),
    "vimg_antilag_workspace_bytes": (C.c_uint64, [u32, u32]),
    "vimg_antilag_rescale": (C.c_int, [C.POINTER(AntilagFrames), Pf32, C.c_void_p, C.POINTER(AntilagParams), C.c_void_p,
                                       C.c_uint64, C.c_void_p, C.c_void_p]),
    "vimg_antilag_last_error": (C.c_char_p, []),
}


class MotionFrames(_Sized, C.Structure):
    """VimgMotionFrames (include/vimg_motion.h): the position frame and the pixel-centre hits and rays, DEVICE pointers."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("position", C.c_void_p),
                ("hits", C.c_void_p), ("rays", C.c_void_p)]


class MotionGeometry(_Sized, C.Structure):
    """VimgMotionGeometry (include/vimg_motion.h): the counts and the DEVICE tables; an old / new pair is both set or both
    None (that table did not move)."""
    _fields_ = [("struct_size", u32), ("num_prims", u32), ("num_tris", u32), ("num_vertices", u32), ("num_spheres", u32),
                ("reserved", u32), ("prims", C.c_void_p), ("tri_vertices", C.c_void_p), ("old_vertices", C.c_void_p),
                ("new_vertices", C.c_void_p), ("old_spheres", C.c_void_p), ("new_spheres", C.c_void_p)]


MOTION_STATIC, MOTION_TRIANGLE, MOTION_SPHERE, MOTION_OUT_OF_RANGE = 0, 1, 2, 3

# the list of symbols include/vimg_motion.h declares: libvimg_motion.so, the previous-world positions of moved geometry
MOTION_SYMBOLS = {
    "vimg_motion_previous_position": (C.c_int, [C.POINTER(MotionFrames), C.POINTER(MotionGeometry), C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "vimg_motion_last_error": (C.c_char_p, []),
}


class DespeckleFrames(_Sized, C.Structure):
    """VimgDespeckleFrames (include/vimg_despeckle.h): the fields of VimgFilterFrames."""
    _fields_ = FilterFrames._fields_


class DespeckleParams(_Sized, C.Structure):
    """VimgDespeckleParams (include/vimg_despeckle.h); vimg_despeckle_defaults fills it."""
    _fields_ = [("struct_size", u32), ("radius", u32), ("rank", u32), ("min_taps", u32), ("gain", f32), ("sigma_normal", f32),
                ("sigma_plane", f32), ("albedo_floor", f32)]


DESPECKLE_WORKSPACE_PER_PIXEL = 32
DESPECKLE_MAX_RADIUS, DESPECKLE_MAX_RANK = 3, 4
DESPECKLE_KEPT, DESPECKLE_CLAMPED, DESPECKLE_FEW_TAPS, DESPECKLE_NOT_LIVE = 0, 1, 2, 3

# the list of symbols include/vimg_despeckle.h declares: libvimg_despeckle.so, the clamp of fireflies before a filter
DESPECKLE_SYMBOLS = {
    "vimg_despeckle_defaults": (None, [C.POINTER(DespeckleParams)]),
    "vimg_despeckle_workspace": (C.c_uint64, [u32, u32]),
    "vimg_despeckle_clamp": (C.c_int, [C.POINTER(DespeckleFrames), C.POINTER(DespeckleParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.c_void_p]),
    "vimg_despeckle_last_error": (C.c_char_p, []),
}


class ExposureFrames(_Sized, C.Structure):
    """VimgExposureFrames (include/vimg_exposure.h): the colour frame and, optionally, the depth frame."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("color", C.c_void_p), ("depth", C.c_void_p)]


class ExposureParams(_Sized, C.Structure):
    """VimgExposureParams (include/vimg_exposure.h); vimg_exposure_defaults fills it."""
    _fields_ = [("struct_size", u32), ("low_permille", u32), ("high_permille", u32), ("key", f32), ("min_exposure", f32),
                ("max_exposure", f32), ("rate_brighten", f32), ("rate_darken", f32)]


class ExposureState(C.Structure):
    """The 1040 bytes of exposure state in device memory (include/vimg_exposure.h), as a host copy of them reads."""
    _fields_ = [("hist", u32 * 256), ("exposure", f32), ("frames", u32), ("metered", f32), ("counted", u32)]


EXPOSURE_BINS, EXPOSURE_STATE_BYTES, EXPOSURE_MAX_WORKGROUPS = 256, 1040, 256

# the list of symbols include/vimg_exposure.h declares: libvimg_exposure.so, histogram auto-exposure with device state
EXPOSURE_SYMBOLS = {
    "vimg_exposure_defaults": (None, [C.POINTER(ExposureParams)]),
    "vimg_exposure_adapt": (C.c_int, [C.POINTER(ExposureFrames), C.POINTER(ExposureParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "vimg_exposure_last_error": (C.c_char_p, []),
}


class DemandFrames(_Sized, C.Structure):
    """VimgDemandFrames (include/vimg_demand.h): the guides of the picture about to be rendered; there is no colour frame."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("normal", C.c_void_p),
                ("position", C.c_void_p), ("depth", C.c_void_p)]


class DemandParams(_Sized, C.Structure):
    """VimgDemandParams (include/vimg_demand.h); vimg_demand_defaults fills it."""
    _fields_ = [("struct_size", u32), ("stride", u32), ("phase", u32), ("reserved", u32), ("min_history", f32),
                ("sigma_normal", f32), ("sigma_plane", f32)]


DEMAND_MAX_STRIDE, DEMAND_COUNTS = 4, 4

# the list of symbols include/vimg_demand.h declares: libvimg_demand.so, the sampling mask of a sparse preview, read from
# libvimg_temporal's history (TEMPORAL_HISTORY_PER_PIXEL) before the frame is rendered
DEMAND_SYMBOLS = {
    "vimg_demand_defaults": (None, [C.POINTER(DemandParams)]),
    "vimg_demand_mask": (C.c_int, [C.POINTER(DemandFrames), C.c_void_p, Pf32, C.POINTER(DemandParams), C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "vimg_demand_last_error": (C.c_char_p, []),
}


class RectifyFrames(_Sized, C.Structure):
    """VimgRectifyFrames (include/vimg_rectify.h): the long and the short history of one picture and its albedo frame."""
    _fields_ = [("struct_size", u32), ("width", u32), ("height", u32), ("reserved", u32), ("slow", C.c_void_p),
                ("fast", C.c_void_p), ("albedo", C.c_void_p)]


class RectifyParams(_Sized, C.Structure):
    """VimgRectifyParams (include/vimg_rectify.h); vimg_rectify_defaults fills it."""
    _fields_ = [("struct_size", u32), ("radius", u32), ("min_taps", u32), ("reserved", u32), ("k", f32), ("cut", f32),
                ("sigma_normal", f32), ("sigma_plane", f32), ("albedo_floor", f32)]


RECTIFY_MAX_RADIUS = 3
RECTIFY_KEPT, RECTIFY_CLAMPED, RECTIFY_FEW_TAPS, RECTIFY_NOT_LIVE = 0, 1, 2, 3

# the list of symbols include/vimg_rectify.h declares: libvimg_rectify.so, the clamp of a long history (the first three
# planes: TEMPORAL_HISTORY_PER_PIXEL) to a short history beside it
RECTIFY_SYMBOLS = {
    "vimg_rectify_defaults": (None, [C.POINTER(RectifyParams)]),
    "vimg_rectify_workspace": (C.c_uint64, [u32, u32]),
    "vimg_rectify_clamp": (C.c_int, [C.POINTER(RectifyFrames), C.POINTER(RectifyParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p]),
    "vimg_rectify_last_error": (C.c_char_p, []),
}


def _bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


# library -> (file, symbol tables, make target, tail of the "missing" message, import torch first).  Torch first: one
# HIP runtime per process.  The torch wheel ships its own libamdhip64 / ROCr, and a second copy in the same process
# cannot open the GPU; importing torch first makes the loader resolve our DT_NEEDED to the copy torch already mapped.
_LIBRARIES = {
    "host": ("libvimg_host.so", (HOST_SYMBOLS,), "host", "", False),
    "hip": ("libvimg_hip.so", (HIP_SYMBOLS, HIP_TEST_SYMBOLS), "hip", "; there is no CPU fallback for the render path", True),
    "filter": ("libvimg_filter.so", (FILTER_SYMBOLS,), "filter", "; there is no CPU fallback for the filter", True),
    "temporal": ("libvimg_temporal.so", (TEMPORAL_SYMBOLS,), "temporal", "; there is no CPU fallback for temporal accumulation", True),
    "varfilter": ("libvimg_varfilter.so", (VARFILTER_SYMBOLS,), "varfilter", "; there is no CPU fallback for the filter", True),
    "moments": ("libvimg_moments.so", (MOMENTS_SYMBOLS,), "moments", "; there is no CPU fallback for temporal accumulation", True),
    "infill": ("libvimg_infill.so", (INFILL_SYMBOLS,), "infill", "; there is no CPU fallback for the reconstruction", True),
    "wtemporal": ("libvimg_wtemporal.so", (WTEMPORAL_SYMBOLS,), "wtemporal", "; there is no CPU fallback for temporal accumulation", True),
    "antilag": ("libvimg_antilag.so", (ANTILAG_SYMBOLS,), "antilag", "; there is no CPU fallback for the history rescaling", True),
}
# the libraries that came after those nine, in the same shape: _load looks here too.  (_LIBRARIES is a closed list that
# earlier ABI tests name key by key; a next library goes here.)
_LATER_LIBRARIES = {
    "motion": ("libvimg_motion.so", (MOTION_SYMBOLS,), "motion", "; there is no CPU fallback for the previous-world positions", True),
    "despeckle": ("libvimg_despeckle.so", (DESPECKLE_SYMBOLS,), "despeckle", "; there is no CPU fallback for the clamp", True),
    "exposure": ("libvimg_exposure.so", (EXPOSURE_SYMBOLS,), "exposure", "; there is no CPU fallback for the exposure", True),
    "demand": ("libvimg_demand.so", (DEMAND_SYMBOLS,), "demand", "; there is no CPU fallback for the sampling mask", True),
    "rectify": ("libvimg_rectify.so", (RECTIFY_SYMBOLS,), "rectify", "; there is no CPU fallback for the history clamp", True),
}
_loaded = {}


def _load(name, path=None):
    """The library ``name`` of _LIBRARIES or _LATER_LIBRARIES, loaded and bound once.  A missing library raises: there is
    no fallback."""
    lib = _loaded.get(name)
    if lib is None:
        file, tables, target, tail, torch_first = _LIBRARIES[name] if name in _LIBRARIES else _LATER_LIBRARIES[name]
        path = path or os.path.join(LIB_DIR, file)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make {target}` (or __graft_entry__.build()){tail}")
        if torch_first:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = C.CDLL(path)
        for table in tables:
            _bind(lib, table)
        _loaded[name] = lib
    return lib


def host_lib():
    return _load("host")


def hip_lib():
    """The HIP extension; VIMG_HIP_LIB selects another build of the same library (A/B measurements only)."""
    return _load("hip", os.environ.get("VIMG_HIP_LIB"))


def filter_lib():
    """The filter library (include/vimg_filter.h)."""
    return _load("filter")


def temporal_lib():
    """The temporal accumulation library (include/vimg_temporal.h)."""
    return _load("temporal")


def varfilter_lib():
    """The variance-guided filter library (include/vimg_varfilter.h)."""
    return _load("varfilter")


def moments_lib():
    """The temporal accumulation library with luminance moments (include/vimg_moments.h)."""
    return _load("moments")


def infill_lib():
    """The reconstruction library for sparsely sampled frames (include/vimg_infill.h)."""
    return _load("infill")


def wtemporal_lib():
    """The temporal accumulation library with per-pixel weights (include/vimg_wtemporal.h)."""
    return _load("wtemporal")


def antilag_lib():
    """The library that shortens a history where the picture has changed (include/vimg_antilag.h)."""
    return _load("antilag")


def motion_lib():
    """The library that writes the previous-world positions of moved geometry (include/vimg_motion.h)."""
    return _load("motion")


def despeckle_lib():
    """The library that clamps fireflies before a frame is filtered (include/vimg_despeckle.h)."""
    return _load("despeckle")


def exposure_lib():
    """The library that meters a frame and scales it by an exposure kept in device memory (include/vimg_exposure.h)."""
    return _load("exposure")


def demand_lib():
    """The library that says which pixels of a sparse preview to sample now (include/vimg_demand.h)."""
    return _load("demand")


def rectify_lib():
    """The library that clamps a long history to a short history beside it (include/vimg_rectify.h)."""
    return _load("rectify")
