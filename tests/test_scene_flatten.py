"""flatten_scene (csrc/scene_flatten.cpp), the host-only half of preprocess, on the CPU: every refusal the GPU suites provoke through
phx_dev_preprocess, the flattened arrays and the light table against numpy fp32 restatements bit for bit, the area CDF against the model
of tests/test_light_sampling.py, and the scene classification that selects the shade kernel.  tests/native/host_flatten.cpp wraps the
function for ctypes; the same source is a stand-alone program for a run under AddressSanitizer / UBSan."""
import copy
import ctypes as C

import numpy as np
import pytest

import native_lib as NL
from conftest import tri_abc
from native_lib import ERR_ARG
from phosphorus_mk2_amd import abi, scenes
from test_light_sampling import LightTable, striped_scene, two_lamp_scene

F = np.float32
SC_TEX_LOBES, SC_TEX_ENV, SC_TEX_MASK, SC_LIGHTS_BY_AREA = 1, 2, 4, 8  # kernels.h: DevScene::any_tex
LIGHT = np.dtype([("first_tri", "<u4"), ("num_tris", "<u4"), ("area", "<f4"), ("material", "<u4"), ("lpdf", "<f4"), ("e", "<f4", 3)])
LIGHT_TRI = np.dtype([("abc", "<f4", 9), ("n", "<f4", 3), ("prim", "<u4"), ("smooth", "<u4"), ("mesh_mat", "<u4"), ("face", "<u4")])
MAT_LITE = np.dtype([("w", "<f4", 3), ("lobes_flags", "<u4"), ("e", "<f4", 3), ("pad", "<u4")])
ARRAYS = {"abc": (0, F), "prim_material": (1, np.uint32), "prim_normals": (2, F), "prim_uv": (3, F), "lights": (4, LIGHT), "light_tris": (5, LIGHT_TRI),
          "light_cdf": (6, F), "mat_lite": (7, MAT_LITE), "mat_masked": (8, np.uint8), "lobe_tex": (9, np.uint32), "textures": (10, np.uint32), "texels": (11, F)}
WORDS = {"any_smooth": 0, "any_tex": 1, "diffuse_only": 2, "any_per_hit": 3, "num_lights": 4, "env_tex": 5, "num_materials": 6}


@pytest.fixture(scope="module")
def flat():
    """the host_flatten library, and flatten(scene, light_sampling, tweak) -> the status, the message and every array as numpy"""
    lib = NL.load("host_flatten")
    lib.hf_flatten.restype = C.c_void_p; lib.hf_flatten.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Options)]
    lib.hf_free.argtypes = [C.c_void_p]
    lib.hf_status.argtypes = [C.c_void_p]
    lib.hf_error.restype = C.c_char_p; lib.hf_error.argtypes = [C.c_void_p]
    lib.hf_array.restype = C.c_void_p; lib.hf_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.hf_word.restype = C.c_uint32; lib.hf_word.argtypes = [C.c_void_p, C.c_int]

    def flatten(scene, light_sampling=abi.LIGHTS_REFERENCE, tweak=None):
        s, keep = scene.pack()
        if tweak:
            tweak(s)
        opt = abi.Options(); opt.light_sampling = light_sampling; opt.path_depth = 9
        h = lib.hf_flatten(C.byref(s), C.byref(opt))
        try:
            out = {"status": lib.hf_status(h), "error": lib.hf_error(h).decode()}
            if out["status"] == 0:
                for name, (which, dtype) in ARRAYS.items():
                    n = C.c_uint64(0)
                    p = lib.hf_array(h, which, C.byref(n))
                    out[name] = np.frombuffer(C.string_at(p, n.value) if n.value else b"", dtype).copy()
                for name, which in WORDS.items():
                    out[name] = lib.hf_word(h, which)
            return out
        finally:
            lib.hf_free(h)
    return flatten


def same_bits(a, b):
    a = np.ascontiguousarray(a, F); b = np.ascontiguousarray(b, F)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. refusals ----------------------------------------------------------------------------------------------------------------------------
IMG43 = np.random.default_rng(7).uniform(0.0, 1.0, (3, 4, 3)).astype(F)
QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)


def _masked_box():  # test_gpu_masks.test_bad_mask_inputs_are_refused_and_the_device_stays_usable's good scene
    s = scenes.cornell(32, 32)
    s.textures = [scenes.TextureDesc(IMG43, abi.TEX_LINEAR)]
    s.meshes[0].uvs = QUAD_UV.copy()
    s.materials[0].lobes[0].fac_mode, s.materials[0].lobes[0].fac_texture = abi.FAC_TEX_A, 1
    return s


def _textured_box():  # test_gpu_textures.test_bad_texture_inputs_are_refused_and_the_device_stays_usable's good scene
    s = scenes.cornell(32, 32)
    s.textures = [scenes.TextureDesc(IMG43, abi.TEX_LINEAR)]
    s.meshes[0].uvs = QUAD_UV.copy()
    s.materials[0].lobes[0].texture = 1
    return s


def _env_box():  # test_gpu_environment.test_bad_environment_inputs_are_refused_and_the_device_stays_usable's good scene
    s = scenes.cornell(32, 32)
    s.meshes = s.meshes[:1] + s.meshes[2:]
    s.textures = [scenes.TextureDesc(np.full((8, 16, 3), 0.5, F), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)]
    s.materials.append(scenes.MaterialDesc([], (0.5, 0.5, 0.5), emission_texture=1, emission_mapping=0))
    s.environment_material = len(s.materials) - 1
    return s


def _set_mask(material, mode, texture):
    def f(s):
        s.materials[material].lobes[0].fac_mode, s.materials[material].lobes[0].fac_texture = mode, texture
    return f


def _masked_lobe():
    return scenes.LobeDesc(abi.LOBE_DIFFUSE, (1, 1, 1), fac_mode=abi.FAC_TEX_B, fac_texture=1)


def _textured_lobe():
    return scenes.LobeDesc(abi.LOBE_DIFFUSE, (1, 1, 1), texture=1)


def _as_environment(lobe):
    def f(s):
        s.materials.append(scenes.MaterialDesc([lobe()], emission=(0.1, 0.1, 0.1)))
        s.environment_material = len(s.materials) - 1
    return f


def _attr(pick, name, value):
    """pick(scene).<name> = value"""
    return lambda s: setattr(pick(s), name, value)


def _uv_per_corner(s):
    s.meshes[1].uvs = np.zeros((5, 2), F)  # per face corner: 6 are needed
    s.meshes[1].flags &= ~abi.MESH_UV_PER_VERTEX


def _smooth_without_normals(per_vertex):
    def f(s):
        m = s.meshes[5]  # the LAST mesh
        m.smooth = np.ones(2, np.uint8)
        m.normals = np.tile(np.array([[0, -1, 0]], F), (3 if per_vertex else 5, 1))  # vertex 3 / corner 5 has none
        if not per_vertex:
            m.flags &= ~abi.MESH_NORMALS_PER_VERTEX
    return f


def _lens(aperture, focal):
    def f(s):
        s.camera.aperture_radius, s.camera.focal_distance = aperture, focal
    return f


def _film(w, h):
    def f(s):
        s.camera.width, s.camera.height = w, h
    return f


def _packed_lobes(n):  # phx_material.lobes holds 8: a count above it can only be set on the packed struct
    def f(packed):
        packed.materials[0].num_lobes = n
    return f


# (name, good scene, change to the SceneDesc, change to the packed phx_scene, light_sampling, the fragment of the message that names the fault)
REFUSALS = [
    # tests/test_gpu_masks.py
    ("mask_index_zero", _masked_box, _set_mask(1, abi.FAC_TEX_B, 0), None, 0, "mask texture index out of range"),
    ("mask_index_past_the_table", _masked_box, _set_mask(1, abi.FAC_TEX_A, 2), None, 0, "mask texture index out of range"),
    ("mask_upper_bits_without_a_tex_mode", _masked_box, _set_mask(1, abi.FAC_MIX_B, 1), None, 0, "fac_mode names a mask texture but its mode is not PHX_FAC_TEX_*"),
    ("mask_upper_bits_on_fac_none", _masked_box, _set_mask(1, abi.FAC_NONE, 1), None, 0, "fac_mode names a mask texture but its mode is not PHX_FAC_TEX_*"),
    ("mask_unknown_mode", _masked_box, _set_mask(1, 5, 1), None, 0, "unknown fac_mode"),
    ("mask_unknown_mode_without_index", _masked_box, _set_mask(1, 255, 0), None, 0, "unknown fac_mode"),
    ("mask_on_emitter", _masked_box, _attr(lambda s: s.materials[3], "lobes", [_masked_lobe()]), None, 0, "masks on emitters / the environment are not supported"),
    ("mask_on_environment", _masked_box, _as_environment(_masked_lobe), None, 0, "masks on emitters / the environment are not supported"),
    # tests/test_gpu_textures.py
    ("texture_out_of_range", _textured_box, _attr(lambda s: s.materials[1].lobes[0], "texture", 2), None, 0, "lobe texture index out of range"),
    ("texture_on_emitter", _textured_box, _attr(lambda s: s.materials[3], "lobes", [_textured_lobe()]), None, 0, "textures on emitters / the environment are not supported"),
    ("texture_on_environment", _textured_box, _as_environment(_textured_lobe), None, 0, "textures on emitters / the environment are not supported"),
    ("texture_zero_size", _textured_box, lambda s: s.textures.append(scenes.TextureDesc(np.zeros((0, 4, 3), F))), None, 0, "texture 1 has zero size"),
    ("texture_too_large", _textured_box, lambda s: s.textures.append(scenes.TextureDesc(np.zeros((1, 70000, 3), F))), None, 0, "texture 1 too large"),
    ("uv_index_per_vertex", _textured_box, _attr(lambda s: s.meshes[0], "uvs", QUAD_UV[:3].copy()), None, 0, "uv index out of range"),
    ("uv_index_per_corner", _textured_box, _uv_per_corner, None, 0, "uv index out of range"),
    # tests/test_gpu_environment.py
    ("environment_image_on_emitter", _env_box, _attr(lambda s: s.materials[3], "emission_texture", 1), None, 0, "emission_texture is allowed only on the environment material"),
    ("environment_image_on_ordinary", _env_box, _attr(lambda s: s.materials[0], "emission_texture", 1), None, 0, "emission_texture is allowed only on the environment material"),
    ("environment_image_without_environment", _env_box, _attr(lambda s: s, "environment_material", -1), None, 0, "emission_texture is allowed only on the environment material"),
    ("environment_image_out_of_range", _env_box, _attr(lambda s: s.materials[4], "emission_texture", 2), None, 0, "emission_texture index out of range"),
    ("environment_bad_mapping", _env_box, _attr(lambda s: s.materials[4], "emission_mapping", 2), None, 0, "unknown emission_mapping"),
    # tests/test_gpu_parity.py::test_error_behaviour, tests/test_gpu_light_sampling.py, tests/test_abi.py
    ("no_emissive_face_set", scenes.cornell, lambda s: setattr(s, "meshes", s.meshes[:5]), None, 0, "scene has no emissive face set"),
    ("aperture_not_finite", scenes.cornell, _lens(float("inf"), 1.0), None, 0, "aperture radius / focal distance not finite"),
    ("focal_distance_not_finite_behind_a_lens", scenes.cornell, _lens(0.1, float("nan")), None, 0, "aperture radius / focal distance not finite"),
    ("face_index", scenes.cornell, _attr(lambda s: s.meshes[5], "sets", [(3, np.array([0, 2], np.uint32))]), None, 0, "face index out of range"),
    ("vertex_index", scenes.cornell, lambda s: s.meshes[5].faces.__setitem__((1, 2), 4), None, 0, "vertex index out of range"),
    ("normal_index_per_vertex", scenes.cornell, _smooth_without_normals(True), None, 0, "normal index out of range"),
    ("normal_index_per_corner", scenes.cornell, _smooth_without_normals(False), None, 0, "normal index out of range"),
    ("face_set_material", scenes.cornell, _attr(lambda s: s.meshes[5], "sets", [(4, np.array([0, 1], np.uint32))]), None, 0, "face set material out of range"),
    ("unknown_closure_id", scenes.cornell, _attr(lambda s: s.materials[1].lobes[0], "type", 99), None, 0, "material with an unknown closure id"),
    ("more_than_8_lobes", scenes.cornell, None, _packed_lobes(9), 0, "material with an unknown closure id"),
    ("film_size_0", scenes.cornell, _film(0, 32), None, 0, "film size out of range"),
    ("film_size_65536", scenes.cornell, _film(32, 65536), None, 0, "film size out of range"),
    ("unknown_light_sampling", scenes.cornell, None, None, 2, "unknown light_sampling"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_every_refusal_of_the_gpu_suites_is_refused_on_the_host(flat, case):
    name, good, change, tweak, light_sampling, fragment = case
    s = good()
    assert flat(s)["status"] == 0, "the scene the fault is put into is itself accepted"
    if change:
        change(s)
    r = flat(s, light_sampling, tweak)
    assert r["status"] == ERR_ARG and fragment in r["error"], r


def test_a_nan_focal_distance_means_nothing_without_a_lens(flat):
    s = scenes.cornell(32, 32)
    s.camera.focal_distance = float("nan")  # camera_t() leaves it uninitialised
    assert flat(s)["status"] == 0


def test_of_two_faults_the_one_tested_first_is_reported(flat):
    s = scenes.cornell(32, 32)
    s.meshes = s.meshes[:5]; s.camera.width = 0
    assert "film size out of range" in flat(s)["error"]
    s = _masked_box()
    s.materials[1].lobes[0].fac_mode = 255; s.meshes[0].sets = [(0, np.array([0, 2], np.uint32))]
    assert "unknown fac_mode" in flat(s)["error"]  # the materials are validated before the meshes are walked
    s = _textured_box()
    s.meshes[0].sets = [(0, np.array([0, 2], np.uint32))]; s.materials[1].lobes[0].type = 99
    assert "face index out of range" in flat(s)["error"]  # ... and baked after


# ---- 2. the flattened arrays --------------------------------------------------------------------------------------------------------------
def check_light_table(r, scene):
    """lights, and the integer words of their triangles, against tests/test_light_sampling.py's fp32 restatement, bit for bit"""
    t = LightTable(scene)
    L = r["lights"]
    assert len(L) == t.n == r["num_lights"]
    sets = [(mi, mat, faces) for mi, m in enumerate(scene.meshes) for mat, faces in m.sets if scene.materials[mat].is_emitter and len(faces)]
    first = np.concatenate([[0], np.cumsum([len(a) for a in t.tris])])
    assert L["first_tri"].tolist() == first[:-1].tolist() and L["num_tris"].tolist() == [len(a) for a in t.tris]
    assert same_bits(L["area"], np.array(t.area, F)) and same_bits(L["lpdf"], np.array(t.lpdf, F))
    assert L["material"].tolist() == [mat for _, mat, _ in sets]
    assert same_bits(L["e"], np.array([scene.materials[mat].emission for _, mat, _ in sets], F))
    T = r["light_tris"]
    assert len(T) == first[-1] and same_bits(T["abc"].reshape(-1, 3, 3), np.concatenate(t.tris))
    prim_of = {}  # (mesh, face) -> index in scene_t::triangles() order
    for mi, m in enumerate(scene.meshes):
        for _, faces in m.sets:
            for f in faces:
                prim_of[(mi, int(f))] = len(prim_of)
    k = 0
    for mi, mat, faces in sets:
        for f in faces:
            assert (T["prim"][k], T["mesh_mat"][k], T["face"][k]) == (prim_of[(mi, int(f))], mi | (mat << 16), 3 * int(f))
            assert T["smooth"][k] == scene.meshes[mi].smooth[f]
            k += 1
    n = T["n"].astype(np.float64); abc = T["abc"].reshape(-1, 3, 3).astype(np.float64)
    g = np.cross(abc[:, 1] - abc[:, 0], abc[:, 2] - abc[:, 0]); g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.abs(n - g).max() < 1e-6  # the geometric normal (its bits are the device's business: tests/test_gpu_parity.py)
    return t


def test_cornell_box_arrays(flat):
    sc = scenes.cornell(32, 32)
    r = flat(sc)
    assert r["status"] == 0
    assert same_bits(r["abc"].reshape(-1, 9), tri_abc(sc))
    assert r["prim_material"].tolist() == [mat for m in sc.meshes for mat, faces in m.sets for _ in faces]
    assert not r["any_smooth"] and r["prim_normals"].size == 0 and r["prim_uv"].size == 0 and r["light_cdf"].size == 0
    assert r["textures"].size == 0 and r["texels"].size == 0 and not r["mat_masked"].any() and r["num_materials"] == len(sc.materials)
    t = check_light_table(r, sc)
    assert t.n == 1 and r["lights"]["num_tris"][0] == 2


def _smooth_atlas():
    """test_gpu_masks.atlas_box (masks and a colour texture on a grid of quads, UVs per face corner) with smooth faces on the grid, a
    smooth lamp and a second light"""
    from test_gpu_masks import atlas_box
    sc = copy.deepcopy(atlas_box(False)[0])
    grid = sc.meshes[2]
    assert len(grid.faces) == 96 and len(grid.uvs) == 3 * len(grid.faces) and not (grid.flags & abi.MESH_UV_PER_VERTEX)
    rng = np.random.default_rng(3)
    grid.normals = rng.normal(size=(len(grid.vertices), 3)).astype(F)
    grid.smooth = (np.arange(len(grid.faces)) % 3 != 0).astype(np.uint8)
    lamp = sc.meshes[-1]
    assert sc.materials[lamp.sets[0][0]].is_emitter
    lamp.normals = rng.normal(size=(6, 3)).astype(F); lamp.smooth = np.array([0, 1], np.uint8); lamp.flags &= ~abi.MESH_NORMALS_PER_VERTEX
    sc.materials.append(scenes.emitter(0.5, 1.5, 4.0))
    sc.meshes.append(scenes._quad((-0.5, -0.99, -2.0), (0.5, -0.99, -2.0), (0.5, -0.99, -3.0), (-0.5, -0.99, -3.0), len(sc.materials) - 1))
    return sc


def test_smooth_textured_masked_scene_arrays(flat):
    sc = _smooth_atlas()
    r = flat(sc)
    assert r["status"] == 0, r
    assert same_bits(r["abc"].reshape(-1, 9), tri_abc(sc))
    want_mat, want_n, want_uv = [], [], []
    for m in sc.meshes:
        for mat, faces in m.sets:
            for f in faces:
                want_mat.append(mat | (0x80000000 if m.smooth[f] else 0))
                idx = m.faces[f] if m.flags & abi.MESH_NORMALS_PER_VERTEX else 3 * f + np.arange(3)
                want_n.append(m.normals[idx].reshape(9) if m.smooth[f] else np.zeros(9, F))
                ui = m.faces[f] if m.flags & abi.MESH_UV_PER_VERTEX else 3 * f + np.arange(3)
                want_uv.append(m.uvs[ui].reshape(6) if len(m.uvs) else np.zeros(6, F))
    assert r["prim_material"].tolist() == want_mat and (r["prim_material"] >> 31).sum() == 64 + 1  # the smooth bit
    assert r["any_smooth"] == 1 and same_bits(r["prim_normals"].reshape(-1, 9), np.array(want_n, F))
    assert same_bits(r["prim_uv"].reshape(-1, 6), np.array(want_uv, F))
    assert r["any_tex"] == SC_TEX_LOBES | SC_TEX_MASK and r["diffuse_only"] == 0 and r["any_per_hit"] == 1
    assert r["mat_masked"].tolist() == [int(any(l.fac_mode in (abi.FAC_TEX_A, abi.FAC_TEX_B) for l in m.lobes)) for m in sc.materials]
    assert r["mat_masked"].sum() == 3
    assert r["lobe_tex"].reshape(-1, 8).tolist() == [[l.texture for l in m.lobes] + [0] * (8 - len(m.lobes)) for m in sc.materials]
    # the texture table: offset, width, height, filter | swrap << 8 | twrap << 16; the texels RGB + 0
    tabs, off = [], 0
    for t in sc.textures:
        h, w = t.texels.shape[:2]
        tabs.append([off, w, h, t.filter | (t.swrap << 8) | (t.twrap << 16)]); off += w * h
    assert r["textures"].reshape(-1, 4).tolist() == tabs
    texels = r["texels"].reshape(-1, 4)
    assert same_bits(texels[:, :3], np.concatenate([t.texels.reshape(-1, 3) for t in sc.textures])) and not texels[:, 3].any()
    t = check_light_table(r, sc)
    assert t.n == 2 and r["light_tris"]["smooth"].tolist() == [0, 1, 0, 0]


# ---- 3. the area CDF --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [striped_scene, two_lamp_scene], ids=["striped_lamp", "two_lamps"])
def test_area_cdf_is_the_model_of_test_light_sampling(flat, scene):
    sc = scene()
    r = flat(sc, abi.LIGHTS_BY_AREA)
    assert r["status"] == 0 and r["any_tex"] == SC_LIGHTS_BY_AREA and r["diffuse_only"] == 0
    t = check_light_table(r, sc)
    assert same_bits(r["light_cdf"], np.concatenate(t.cdf)) and len(r["light_cdf"]) == len(r["light_tris"])
    for L in r["lights"]:
        cdf = r["light_cdf"][L["first_tri"]:L["first_tri"] + L["num_tris"]]
        assert (np.diff(cdf) >= 0).all() and cdf[0] > 0 and cdf[-1].tobytes() == F(1.0).tobytes()
    if len(r["lights"]) == 1:
        assert r["light_cdf"].tolist() == [0.25, 0.5, 0.625, 0.75, 0.8125, 0.875, 0.9375, 1.0]
    plain = flat(sc)
    assert plain["status"] == 0 and plain["light_cdf"].size == 0 and plain["any_tex"] == 0 and plain["diffuse_only"] == 2
    assert plain["lights"].tobytes() == r["lights"].tobytes() and plain["light_tris"].tobytes() == r["light_tris"].tobytes()


# ---- 4. which shade kernel the scene selects ---------------------------------------------------------------------------------------------------
def test_scene_classification(flat):
    D = abi.LOBE_DIFFUSE
    soup = scenes.soup(500, width=32, height=32)
    r = flat(soup)
    assert (r["diffuse_only"], r["any_per_hit"], r["any_tex"]) == (2, 0, 0)
    lite = r["mat_lite"]  # 32 bytes per material: the one Lambert lobe's weight, num_lobes | flags << 8, the emission
    assert len(lite) == len(soup.materials) and (lite["lobes_flags"] & 0xff).tolist() == [len(m.lobes) for m in soup.materials]
    assert lite["lobes_flags"][1] == 0 and lite["lobes_flags"][0] >> 8 != 0
    assert same_bits(lite["w"], np.array([m.lobes[0].weight if m.lobes else (0, 0, 0) for m in soup.materials], F))
    assert same_bits(lite["e"], np.array([m.emission for m in soup.materials], F))
    two = scenes.soup(500, width=32, height=32, materials=[scenes.MaterialDesc([scenes.LobeDesc(D, (0.4, 0.3, 0.2)), scenes.LobeDesc(D, (0.2, 0.3, 0.4))])])
    r = flat(two)
    assert (r["diffuse_only"], r["any_per_hit"], r["mat_lite"].size) == (1, 0, 0)
    lamp = scenes.cornell(32, 32)  # an emitter given as an emission closure (not a lobe): its row of the 32-byte table has no weight
    lamp.materials[3].lobes = [scenes.LobeDesc(abi.LOBE_EMISSIVE, (3.0, 2.0, 1.0))]
    r = flat(lamp)
    assert r["diffuse_only"] == 2 and r["mat_lite"]["lobes_flags"].tolist() == [r["mat_lite"]["lobes_flags"][0]] * 3 + [0]
    assert r["mat_lite"].tobytes() == flat(scenes.cornell(32, 32))["mat_lite"].tobytes() and not r["mat_lite"]["w"][3].any()
    r = flat(scenes.glass_blobs(32, 32))
    assert (r["diffuse_only"], r["any_per_hit"]) == (0, 1)
    r = flat(scenes.multi_material_soup(500, width=32, height=32))  # constant closures that are not Lambert
    assert (r["diffuse_only"], r["any_per_hit"]) == (0, 0)
    for sc, ls, bits in ((_textured_box(), 0, SC_TEX_LOBES), (_masked_box(), 0, SC_TEX_LOBES | SC_TEX_MASK), (_env_box(), 0, SC_TEX_ENV),
                         (scenes.cornell(32, 32), abi.LIGHTS_BY_AREA, SC_LIGHTS_BY_AREA)):
        r = flat(sc, ls)
        assert r["status"] == 0 and r["any_tex"] == bits and r["diffuse_only"] == 0 and r["mat_lite"].size == 0, bits
        assert (r["textures"].size != 0) == bool(bits & 7) and r["env_tex"] == (1 if bits & SC_TEX_ENV else 0)
    unused = _textured_box(); unused.materials[0].lobes[0].texture = 0  # a texture table no lobe uses is not packed
    r = flat(unused)
    assert (r["any_tex"], r["diffuse_only"], r["textures"].size, r["prim_uv"].size) == (0, 2, 0, 0)


# ---- 5. under AddressSanitizer and UBSan, stand-alone -------------------------------------------------------------------------------------
def test_out_of_range_indices_are_refused_before_they_are_used(tmp_path):
    """host_flatten.cpp's own main(): a good scene and one per index family with the bad index at the last face, in arrays of exactly
    their size.  A check that came after the read would stop the program with a sanitizer report."""
    stdout = NL.run_sanitized(tmp_path, "host_flatten", "HOST_FLATTEN_MAIN")
    assert stdout.split() == ["good", "0", "as-expected"] + [w for name in ("face", "vertex", "normal", "uv", "material") for w in (name, "1", "as-expected")]
