"""ctypes mirror of include/phx_xpu.h (the C ABI of the gfx950 device).

Field order and types must match the header exactly; tests/test_abi.py checks struct sizes against
`phx_abi_sizeof` exported by the library and that every declared symbol is exported.
"""
import ctypes as C

PHX_OK = 0
PHX_HIT, PHX_MASKED, PHX_SHADOW, PHX_SPECULAR = 1, 2, 4, 8
LOBE_EMISSIVE, LOBE_DIFFUSE, LOBE_OREN_NAYAR, LOBE_REFLECTION = 0, 1, 2, 4
LOBE_REFRACTION, LOBE_MICROFACET, LOBE_SHEEN, LOBE_BACKGROUND, LOBE_TRANSPARENT = 8, 16, 32, 64, 128
BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR, BSDF_REFLECT, BSDF_TRANSMIT = 1, 2, 4, 8, 16
MAX_LOBES = 8
FAC_NONE, FAC_MIX_B, FAC_MIX_A, FAC_TEX_B, FAC_TEX_A = 0, 1, 2, 3, 4


def fac_pack(mode, texture=0):
    """PHX_FAC_PACK: a phx_lobe.fac_mode word from a mode and, for the FAC_TEX_* modes, the mask image (1-based into the scene's textures)"""
    return (int(mode) & 0xff) | (int(texture) << 8)


def fac_mode(word):
    """PHX_FAC_MODE"""
    return int(word) & 0xff


def fac_texture(word):
    """PHX_FAC_TEXTURE"""
    return int(word) >> 8


BVH_AUTO, BVH_DEVICE_LBVH, BVH_HOST_SAH = 0, 1, 2
LIGHTS_REFERENCE, LIGHTS_BY_AREA = 0, 1  # Options.light_sampling: a light's triangle by index (the reference) or by area
LIGHT_SELECT_BY_POWER = 0x100  # bit 8 of the same word: the light by power, not uniformly (needs LIGHTS_BY_AREA in the low byte)
LIGHT_INCLUDE_ENVIRONMENT = 0x200  # bit 9: next-event estimation samples the environment image too (needs LIGHT_SELECT_BY_POWER: the word 0x301)
MESH_UV_PER_VERTEX, MESH_NORMALS_PER_VERTEX = 1, 2
TEX_LINEAR, TEX_CLOSEST = 0, 1
WRAP_PERIODIC, WRAP_CLAMP, WRAP_BLACK = 0, 1, 2
ENV_LATLONG_Y_UP, ENV_LATLONG_Z_UP = 0, 1
# Stats.shade_kernels: bit (family * SHADE_PASSES + pass) for every shade kernel the last frame launched (PHX_SHADE_*)
SHADE_PASS_LATER, SHADE_PASS_CAMERA, SHADE_PASS_LENS, SHADE_PASSES = 0, 1, 2, 3
SHADE_FAMILY_LAMBERT1, SHADE_FAMILY_LAMBERT, SHADE_FAMILY_GENERAL = 0, 1, 2  # k_shade<2>, k_shade<1>, k_shade_g: 2 + (PERHIT | TEX | ENV)
SHADE_G_PERHIT, SHADE_G_TEX, SHADE_G_ENV = 1, 2, 4
SHADE_FAMILY_MASK, SHADE_FAMILY_MASK_ENV, SHADE_FAMILIES, SHADE_KERNELS = 10, 11, 12, 36


def shade_kernel_bit(family, pass_):
    """the bit of Stats.shade_kernels (its index, not its mask) of `family` in pass `pass_`"""
    if not (0 <= family < SHADE_FAMILIES and 0 <= pass_ < SHADE_PASSES):
        raise ValueError(f"no shade kernel (family {family}, pass {pass_})")
    return family * SHADE_PASSES + pass_


def shade_kernel_name(bit):
    """the instantiation behind bit `bit` of Stats.shade_kernels, as launch_shade (shade_general.hip) spells it"""
    if not 0 <= bit < SHADE_KERNELS:
        raise ValueError(f"no shade kernel has bit {bit}")
    family, p = divmod(bit, SHADE_PASSES)
    first, lens = ("false", "false") if p == SHADE_PASS_LATER else ("true", "true" if p == SHADE_PASS_LENS else "false")
    if family < SHADE_FAMILY_GENERAL:
        return f"k_shade<{2 if family == SHADE_FAMILY_LAMBERT1 else 1}, {first}, {lens}>"
    g = family - SHADE_FAMILY_GENERAL
    perhit, tex, env, mask = bool(g & SHADE_G_PERHIT), bool(g & SHADE_G_TEX), bool(g & SHADE_G_ENV), False
    if family >= SHADE_FAMILY_MASK:
        perhit, tex, env, mask = True, True, family == SHADE_FAMILY_MASK_ENV, True
    b = lambda x: "true" if x else "false"
    tags = [t for t, on in (("PERHIT", perhit), ("TEX", tex), ("ENV", env), ("MASK", mask)) if on]
    return f"k_shade_g<{b(perhit)}, {first}, {lens}, {b(tex)}, {b(env)}, {b(mask)}>" + (f" ({' + '.join(tags)})" if tags else "")


def shade_kernel_names(mask):
    """the kernels of a Stats.shade_kernels word, for assertion messages"""
    return [shade_kernel_name(b) for b in range(SHADE_KERNELS) if int(mask) >> b & 1] + ([f"unknown bits {int(mask) >> SHADE_KERNELS:#x}"] if int(mask) >> SHADE_KERNELS else [])

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)


class Options(C.Structure):
    _fields_ = [
        ("samples_per_pixel", C.c_uint32), ("paths_per_sample", C.c_uint32), ("path_depth", C.c_uint32),
        ("single_threaded", C.c_uint32), ("host_only", C.c_uint32), ("render_normals", C.c_uint32),
        ("verbose", C.c_uint32), ("device_ordinal", C.c_int32), ("samples_in_flight", C.c_uint32),
        ("tiles_per_batch", C.c_uint32), ("bvh_builder", C.c_uint32), ("light_sampling", C.c_uint32), ("reserved", C.c_uint32 * 4),
    ]


class Lobe(C.Structure):
    _fields_ = [
        ("type", C.c_uint32), ("weight", C.c_float * 3), ("alpha", C.c_float), ("eta", C.c_float),
        ("xalpha", C.c_float), ("yalpha", C.c_float), ("refract", C.c_uint32), ("r", C.c_float),
        ("fac_mode", C.c_uint32), ("fac_ior", C.c_float), ("pre_weight", C.c_float * 3), ("texture", C.c_uint32),
    ]


class Material(C.Structure):
    _fields_ = [
        ("num_lobes", C.c_uint32), ("is_emitter", C.c_uint32), ("emission", C.c_float * 3),
        ("emission_texture", C.c_uint32), ("emission_mapping", C.c_uint32), ("emission_uv_texture", C.c_uint32), ("lobes", Lobe * MAX_LOBES),
    ]


class FaceSet(C.Structure):
    _fields_ = [("material", C.c_uint32), ("num_faces", C.c_uint32), ("faces", u32p)]


class Mesh(C.Structure):
    _fields_ = [
        ("vertices", f32p), ("num_vertices", C.c_uint32), ("normals", f32p), ("num_normals", C.c_uint32),
        ("faces", u32p), ("num_faces", C.c_uint32), ("smooth", u8p), ("flags", C.c_uint32),
        ("num_sets", C.c_uint32), ("sets", C.POINTER(FaceSet)), ("uvs", f32p), ("num_uvs", C.c_uint32),
    ]


class Texture(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("texels", f32p), ("filter", C.c_uint32),
        ("swrap", C.c_uint32), ("twrap", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


class Camera(C.Structure):
    _fields_ = [
        ("to_world", C.c_float * 16), ("fov", C.c_float), ("focal_distance", C.c_float),
        ("aperture_radius", C.c_float), ("film_width", C.c_uint32), ("film_height", C.c_uint32),
    ]


class Scene(C.Structure):
    _fields_ = [
        ("num_meshes", C.c_uint32), ("meshes", C.POINTER(Mesh)), ("num_materials", C.c_uint32),
        ("materials", C.POINTER(Material)), ("environment_material", C.c_int32), ("camera", Camera),
        ("num_textures", C.c_uint32), ("textures", C.POINTER(Texture)),
    ]


class Tile(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


NEXT_TILE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Tile))
ADD_TILE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, f32p, C.c_uint32, C.c_uint32)


class Frame(C.Structure):
    _fields_ = [
        ("tiles_user", C.c_void_p), ("next_tile", C.c_void_p), ("film_user", C.c_void_p), ("add_tile", C.c_void_p),
        ("sampler_seed", C.c_uint64), ("primary_components", C.c_uint32), ("normals_channel", C.c_uint32),
        ("device_film", C.c_void_p), ("host_film", C.c_void_p), ("moments_channel", C.c_uint32), ("reserved", C.c_uint32 * 1),
    ]


class Adaptive(C.Structure):
    """phx_adaptive: the setting of adaptive sampling (phx_dev_set_adaptive)"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_uint32), ("step", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class Denoise(C.Structure):
    """phx_denoise: the film denoiser's settings and the film's layout (phx_dev_denoise)"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("xstride", C.c_uint32), ("normals_offset", C.c_uint32), ("m2_offset", C.c_uint32),
        ("samples_offset", C.c_uint32), ("spp", C.c_uint32), ("iterations", C.c_uint32), ("sigma_l", C.c_float),
        ("normal_power_log2", C.c_uint32), ("on_device", C.c_uint32), ("reserved", C.c_uint32 * 5),
    ]


GUIDE_DEMODULATE, GUIDE_PLANE = 1, 2  # DenoiseGuides.flags (PHX_GUIDE_*)
GUIDE_FLOATS = 8  # a pixel of the guide film: albedo rgb, coverage, position xyz, distance


class Guides(C.Structure):
    """phx_guides: the first-hit guide pass (phx_dev_render_guides)"""
    _fields_ = [("sampler_seed", C.c_uint64), ("samples", C.c_uint32), ("on_device", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class DenoiseGuides(C.Structure):
    """phx_denoise_guides: the guide film of a guided denoise call and what it is used for (phx_dev_denoise_guided)"""
    _fields_ = [
        ("guides", C.c_void_p), ("xstride", C.c_uint32), ("flags", C.c_uint32), ("albedo_floor", C.c_float), ("sigma_x", C.c_float),
        ("plane_scale", C.c_float), ("reserved", C.c_uint32 * 4),
    ]


class Accumulate(C.Structure):
    """phx_accumulate: the two films' layouts and the summary's criterion (phx_dev_film_accumulate); _a is the accumulator, _b the frame film"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("xstride_a", C.c_uint32), ("normals_offset_a", C.c_uint32), ("m2_offset_a", C.c_uint32), ("samples_offset_a", C.c_uint32),
        ("xstride_b", C.c_uint32), ("normals_offset_b", C.c_uint32), ("m2_offset_b", C.c_uint32), ("samples_offset_b", C.c_uint32),
        ("spp_b", C.c_uint32), ("on_device", C.c_uint32), ("tau", C.c_float), ("floor", C.c_float), ("reserved", C.c_uint32 * 2),
    ]


class AccumulateSummary(C.Structure):
    """phx_accumulate_summary: the counters of a phx_dev_film_accumulate call"""
    _fields_ = [("pixels", C.c_uint64), ("invalid", C.c_uint64), ("converged", C.c_uint64), ("samples", C.c_uint64)]


class Reproject(C.Structure):
    """phx_reproject: the accumulator films' and the guide films' layout, the two cameras and the settings of phx_dev_film_reproject"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("xstride_a", C.c_uint32), ("normals_offset_a", C.c_uint32), ("m2_offset_a", C.c_uint32), ("samples_offset_a", C.c_uint32),
        ("xstride_g", C.c_uint32), ("on_device", C.c_uint32), ("from", Camera), ("to", Camera),  # (`from` is a keyword: getattr(q, "from"))
        ("sigma_plane", C.c_float), ("sigma_dist", C.c_float), ("max_history", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


class ReprojectSummary(C.Structure):
    """phx_reproject_summary: the counters of a phx_dev_film_reproject call"""
    _fields_ = [("pixels", C.c_uint64), ("reused", C.c_uint64), ("no_geometry", C.c_uint64), ("disoccluded", C.c_uint64), ("samples", C.c_uint64)]


OUTLIER_EXCLUDE_CENTRE, OUTLIER_UPPER_ONLY = 1, 2  # OutlierClamp.flags (PHX_OUTLIER_*)


class OutlierClamp(C.Structure):
    """phx_outlier_clamp: the layouts of the film (_a) and of the reference film (_b) and the settings of phx_dev_film_outlier_clamp"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("xstride_a", C.c_uint32), ("m2_offset_a", C.c_uint32), ("samples_offset_a", C.c_uint32),
        ("xstride_b", C.c_uint32), ("on_device", C.c_uint32), ("flags", C.c_uint32), ("radius", C.c_uint32), ("trim", C.c_uint32),
        ("min_taps", C.c_uint32), ("gamma", C.c_float), ("floor", C.c_float), ("clamped_history", C.c_uint32), ("reserved", C.c_uint32 * 2),
    ]


class OutlierClampSummary(C.Structure):
    """phx_outlier_clamp_summary: the counters of a phx_dev_film_outlier_clamp call"""
    _fields_ = [("pixels", C.c_uint64), ("skipped", C.c_uint64), ("unbounded", C.c_uint64), ("inside", C.c_uint64), ("clamped", C.c_uint64),
                ("capped", C.c_uint64)]


class TileMap(C.Structure):
    """phx_tile_map: the accumulator's layout, the tile grid and the criterion of the tile map (phx_dev_film_tile_map)"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("xstride", C.c_uint32), ("m2_offset", C.c_uint32), ("samples_offset", C.c_uint32),
        ("tile_width", C.c_uint32), ("tile_height", C.c_uint32), ("on_device", C.c_uint32), ("tau", C.c_float), ("floor", C.c_float),
        ("reserved", C.c_uint32 * 4),
    ]


class TileRecord(C.Structure):
    """phx_tile_record: what a phx_dev_film_tile_map call knows of one tile (40 bytes)"""
    _fields_ = [("tile", Tile), ("invalid", C.c_uint32), ("starved", C.c_uint32), ("converged", C.c_uint32), ("worst", C.c_float),
                ("samples", C.c_uint64)]


class TileMapSummary(C.Structure):
    """phx_tile_map_summary: the counters of a phx_dev_film_tile_map call"""
    _fields_ = [("pixels", C.c_uint64), ("invalid", C.c_uint64), ("converged", C.c_uint64), ("samples", C.c_uint64), ("tiles", C.c_uint64),
                ("open", C.c_uint64)]


UPDATE_REFIT, UPDATE_REBUILD = 0, 1  # GeometryUpdate.mode (PHX_UPDATE_*)


class GeometryUpdate(C.Structure):
    """phx_geometry_update: how phx_dev_update_geometry brings the tree up to date"""
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class GeometrySummary(C.Structure):
    """phx_geometry_summary: what a phx_dev_update_geometry call left behind"""
    _fields_ = [("mode", C.c_uint32), ("triangles", C.c_uint32), ("nodes", C.c_uint32), ("levels", C.c_uint32), ("lights", C.c_uint32),
                ("light_triangles", C.c_uint32), ("bounds", C.c_float * 6), ("delta", C.c_float)]


DISPLAY_DITHER, DISPLAY_AUTO_EXPOSURE = 1, 2  # Display.flags (PHX_DISPLAY_*)
TONE_CLAMP, TONE_REINHARD, TONE_ACES = 0, 1, 2  # Display.tone (PHX_TONE_*)


class Display(C.Structure):
    """phx_display: the film's and the image's layout, the exposure and the tone curve of the display pass (phx_dev_film_display)"""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("xstride", C.c_uint32), ("image_pitch", C.c_uint32), ("on_device", C.c_uint32),
        ("flags", C.c_uint32), ("tone", C.c_uint32), ("scale", C.c_float), ("white", C.c_float), ("key", C.c_float),
        ("low_q16", C.c_uint32), ("high_q16", C.c_uint32), ("min_scale", C.c_float), ("max_scale", C.c_float), ("reserved", C.c_uint32 * 2),
    ]


class DisplaySummary(C.Structure):
    """phx_display_summary: the counters and the scale of a phx_dev_film_display call"""
    _fields_ = [("pixels", C.c_uint64), ("invalid", C.c_uint64), ("unlit", C.c_uint64), ("counted", C.c_uint64), ("scale", C.c_float),
                ("from_histogram", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [
        ("camera_samples", C.c_uint64), ("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64),
        ("rays_masked", C.c_uint64), ("tiles", C.c_uint64), ("trace_launches", C.c_uint64),
        ("trace_ms", C.c_double), ("closest_ms", C.c_double), ("shadow_ms", C.c_double), ("shade_ms", C.c_double),
        ("frame_ms", C.c_double), ("bvh_nodes", C.c_uint64), ("bvh_bytes", C.c_uint64), ("triangles", C.c_uint64),
        ("preprocess_ms", C.c_double), ("bvh_build_ms", C.c_double),
        ("trace_block", C.c_uint64), ("trace_ntop", C.c_uint64), ("trace_levels", C.c_uint64), ("trace_waves_per_cu", C.c_uint64),
        ("bvh_depth", C.c_uint64), ("paths_in_flight", C.c_uint64),
        ("node_visits_lds", C.c_uint64 * 2), ("node_visits_mem", C.c_uint64 * 2), ("tri_tests", C.c_uint64 * 2),
        ("instrumented", C.c_uint64), ("wave_iters", C.c_uint64), ("node_block_execs", C.c_uint64), ("tri_block_execs", C.c_uint64),
        ("refills", C.c_uint64), ("idle_lane_iters", C.c_uint64), ("tri_pending_lane_iters", C.c_uint64), ("stack_pushes", C.c_uint64 * 8), ("bvh_cost_model", C.c_double), ("trace_lds_levels", C.c_uint64), ("bvh_built_on_device", C.c_uint64),
        ("shade_kernel_ms", C.c_double), ("shade_launches", C.c_uint64), ("shade_general", C.c_uint64), ("primary_ms", C.c_double), ("primary_launches", C.c_uint64),
        ("primary_packets", C.c_uint64), ("primary_fallbacks", C.c_uint64), ("primary_node_tests", C.c_uint64), ("primary_tri_tests", C.c_uint64), ("primary_tri_lanes_hit", C.c_uint64),
        ("device_bytes", C.c_uint64), ("tri_pairs_pending", C.c_uint64), ("tri_pairs_hist", C.c_uint64 * 8), ("trace_stack_packed", C.c_uint64),
        ("shade_kernels", C.c_uint64),
    ]


# every entry point include/phx_xpu.h declares
EXPORTS = [
    "phx_discover", "phx_dev_make", "phx_dev_preprocess", "phx_dev_start", "phx_dev_join", "phx_dev_destroy",
    "phx_last_error", "phx_dev_get_stats", "phx_tiles_make", "phx_tiles_next", "phx_tiles_count", "phx_tiles_reset",
    "phx_tiles_free", "phx_dev_trace", "phx_dev_bsdf_f", "phx_dev_bsdf_sample", "phx_dev_copy_bvh",
    "phx_dev_texture_lookup", "phx_dev_environment_lookup", "phx_dev_lobe_weights",
    "phx_dev_light_sample", "phx_dev_light_emission", "phx_dev_environment_sample", "phx_dev_film_moments",
    "phx_dev_set_adaptive", "phx_dev_adaptive_select", "phx_dev_denoise", "phx_dev_denoise_times",
    "phx_dev_render_guides", "phx_dev_guides_times", "phx_dev_denoise_guided",
    "phx_dev_film_accumulate", "phx_dev_accumulate_times", "phx_dev_film_display", "phx_dev_display_times",
    "phx_dev_set_camera", "phx_dev_film_reproject", "phx_dev_reproject_times",
    "phx_dev_film_outlier_clamp", "phx_dev_outlier_clamp_times",
    "phx_dev_film_tile_map", "phx_dev_tile_map_times", "phx_tiles_make_list",
    "phx_dev_update_geometry", "phx_dev_update_geometry_times",
]


def declare(lib):
    """Attach argtypes/restypes of the C ABI to a loaded libphx_hip.so."""
    vp = C.c_void_p
    lib.phx_discover.argtypes = [C.POINTER(Options), C.POINTER(C.c_int)]; lib.phx_discover.restype = C.c_int
    lib.phx_dev_make.argtypes = [C.POINTER(Options)]; lib.phx_dev_make.restype = vp
    lib.phx_dev_preprocess.argtypes = [vp, C.POINTER(Scene)]; lib.phx_dev_preprocess.restype = C.c_int
    lib.phx_dev_start.argtypes = [vp, C.POINTER(Frame)]; lib.phx_dev_start.restype = C.c_int
    lib.phx_dev_join.argtypes = [vp]; lib.phx_dev_join.restype = C.c_int
    lib.phx_dev_destroy.argtypes = [vp]; lib.phx_dev_destroy.restype = None
    lib.phx_last_error.argtypes = []; lib.phx_last_error.restype = C.c_char_p
    lib.phx_dev_get_stats.argtypes = [vp, C.POINTER(Stats)]; lib.phx_dev_get_stats.restype = C.c_int
    lib.phx_tiles_make.argtypes = [C.c_uint32] * 5; lib.phx_tiles_make.restype = vp
    lib.phx_tiles_make_list.argtypes = [C.POINTER(Tile), C.c_uint32]; lib.phx_tiles_make_list.restype = vp
    lib.phx_tiles_next.argtypes = [vp, C.POINTER(Tile)]; lib.phx_tiles_next.restype = C.c_int
    lib.phx_tiles_count.argtypes = [vp]; lib.phx_tiles_count.restype = C.c_uint32
    lib.phx_tiles_reset.argtypes = [vp]; lib.phx_tiles_reset.restype = None
    lib.phx_tiles_free.argtypes = [vp]; lib.phx_tiles_free.restype = None
    lib.phx_dev_trace.argtypes = [vp, C.c_uint32, f32p, f32p, f32p, C.c_int, f32p, f32p, f32p, u32p, u8p]
    lib.phx_dev_trace.restype = C.c_int
    lib.phx_dev_bsdf_f.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, f32p, f32p, f32p]; lib.phx_dev_bsdf_f.restype = C.c_int
    lib.phx_dev_film_moments.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, f32p, f32p]; lib.phx_dev_film_moments.restype = C.c_int
    lib.phx_dev_bsdf_sample.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, f32p, f32p, f32p, f32p, f32p, u32p]
    lib.phx_dev_bsdf_sample.restype = C.c_int
    lib.phx_dev_texture_lookup.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, f32p]; lib.phx_dev_texture_lookup.restype = C.c_int
    lib.phx_dev_environment_lookup.argtypes = [vp, C.c_uint32, f32p, f32p]; lib.phx_dev_environment_lookup.restype = C.c_int
    lib.phx_dev_lobe_weights.argtypes = [vp, C.c_uint32, C.c_uint32, f32p, f32p, f32p, f32p, u32p]; lib.phx_dev_lobe_weights.restype = C.c_int
    lib.phx_dev_light_sample.argtypes = [vp, C.c_uint32, f32p, u32p, u32p, f32p, f32p, f32p]; lib.phx_dev_light_sample.restype = C.c_int
    lib.phx_dev_light_emission.argtypes = [vp, C.c_uint32, f32p, f32p, f32p]; lib.phx_dev_light_emission.restype = C.c_int
    lib.phx_dev_environment_sample.argtypes = [vp, C.c_uint32, f32p, u32p, u32p, f32p, f32p, f32p, f32p]; lib.phx_dev_environment_sample.restype = C.c_int
    lib.phx_dev_set_adaptive.argtypes = [vp, C.POINTER(Adaptive)]; lib.phx_dev_set_adaptive.restype = C.c_int
    lib.phx_dev_adaptive_select.argtypes = [vp, C.c_uint32, u32p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, C.POINTER(Adaptive), u32p, u32p]
    lib.phx_dev_adaptive_select.restype = C.c_int
    lib.phx_dev_denoise.argtypes = [vp, C.POINTER(Denoise), vp, vp]; lib.phx_dev_denoise.restype = C.c_int  # the films: host or device addresses
    lib.phx_dev_denoise_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_denoise_times.restype = C.c_int
    lib.phx_dev_render_guides.argtypes = [vp, C.POINTER(Guides), vp]; lib.phx_dev_render_guides.restype = C.c_int  # the film: a host or device address
    lib.phx_dev_guides_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_guides_times.restype = C.c_int
    lib.phx_dev_denoise_guided.argtypes = [vp, C.POINTER(Denoise), C.POINTER(DenoiseGuides), vp, vp]; lib.phx_dev_denoise_guided.restype = C.c_int
    lib.phx_dev_film_accumulate.argtypes = [vp, C.POINTER(Accumulate), vp, vp, C.POINTER(AccumulateSummary)]; lib.phx_dev_film_accumulate.restype = C.c_int
    lib.phx_dev_accumulate_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_accumulate_times.restype = C.c_int
    lib.phx_dev_film_display.argtypes = [vp, C.POINTER(Display), vp, vp, C.POINTER(DisplaySummary), C.POINTER(C.c_uint64)]; lib.phx_dev_film_display.restype = C.c_int
    lib.phx_dev_display_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_display_times.restype = C.c_int
    lib.phx_dev_set_camera.argtypes = [vp, C.POINTER(Camera)]; lib.phx_dev_set_camera.restype = C.c_int
    lib.phx_dev_film_reproject.argtypes = [vp, C.POINTER(Reproject), vp, vp, vp, vp, C.POINTER(ReprojectSummary)]; lib.phx_dev_film_reproject.restype = C.c_int
    lib.phx_dev_reproject_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_reproject_times.restype = C.c_int
    lib.phx_dev_film_outlier_clamp.argtypes = [vp, C.POINTER(OutlierClamp), vp, vp, vp, C.POINTER(OutlierClampSummary)]; lib.phx_dev_film_outlier_clamp.restype = C.c_int
    lib.phx_dev_outlier_clamp_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_outlier_clamp_times.restype = C.c_int
    lib.phx_dev_film_tile_map.argtypes = [vp, C.POINTER(TileMap), vp, vp, C.POINTER(TileMapSummary)]; lib.phx_dev_film_tile_map.restype = C.c_int
    lib.phx_dev_tile_map_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_tile_map_times.restype = C.c_int
    lib.phx_dev_copy_bvh.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64), f32p]; lib.phx_dev_copy_bvh.restype = C.c_int
    lib.phx_dev_update_geometry.argtypes = [vp, C.POINTER(Scene), C.POINTER(GeometryUpdate), C.POINTER(GeometrySummary)]; lib.phx_dev_update_geometry.restype = C.c_int
    lib.phx_dev_update_geometry_times.argtypes = [vp, C.POINTER(C.c_double)]; lib.phx_dev_update_geometry_times.restype = C.c_int
    return lib
