"""Geometry updates (phx_dev_update_geometry) without a GPU: the ABI and the header's text, the Python movers
(scenes.transformed, scenes.wobbled), and flatten_geometry (csrc/scene_flatten.cpp through tests/native/update_geometry_host.cpp): its tables
equal flatten_scene's of the moved scene word for word under every light_sampling, and every refusal returns PHX_ERR_ARG with its reason.
The tree's half is tests/test_bvh_refit.py; the device is held to both in tests/test_gpu_update_geometry.py."""
import ctypes as C
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import native_lib as NL
from conftest import bits_equal, tri_abc
from native_lib import CSRC, ERR_ARG, NATIVE

F = np.float32

# the host library of this module: a registry of its own, as tests/test_tile_map.py keeps one
REGISTRY = {"update_geometry_host": ([os.path.join(NATIVE, "update_geometry_host.cpp"), os.path.join(CSRC, "scene_flatten.cpp")], NL.FLATTEN)}

LIGHT = np.dtype([("first_tri", "u4"), ("num_tris", "u4"), ("area", "f4"), ("material", "u4"), ("lpdf", "f4"), ("e", "f4", 3)])
GEOMETRY_ARRAYS = {"abc": 0, "prim_material": 1, "prim_normals": 2, "lights": 4, "light_tris": 5, "light_cdf": 6}  # hf_array's indices
MODES = [0, 1, 0x101, 0x301]


# ---- 1. the ABI and the header ------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_field_offsets():
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.GeometryUpdate) == 16 and [f for f, _ in abi.GeometryUpdate._fields_] == ["mode", "reserved"]
    assert abi.GeometryUpdate.reserved.offset == 4 and abi.GeometryUpdate.reserved.size == 12
    fields = ["mode", "triangles", "nodes", "levels", "lights", "light_triangles", "bounds", "delta"]
    assert C.sizeof(abi.GeometrySummary) == 52 and [f for f, _ in abi.GeometrySummary._fields_] == fields
    assert [getattr(abi.GeometrySummary, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24, 48]
    assert (abi.UPDATE_REFIT, abi.UPDATE_REBUILD) == (0, 1)
    for name in ("phx_dev_update_geometry", "phx_dev_update_geometry_times"):
        assert name in abi.EXPORTS


def _library():
    from phosphorus_mk2_amd import xpu
    if not os.path.exists(xpu.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return xpu.load_library()


def test_struct_sizes_are_the_librarys_and_stats_did_not_grow():
    from phosphorus_mk2_amd import abi
    lib = _library()
    assert (lib.phx_abi_sizeof(28), lib.phx_abi_sizeof(29)) == (C.sizeof(abi.GeometryUpdate), C.sizeof(abi.GeometrySummary)) == (16, 52)
    assert lib.phx_abi_sizeof(9) == C.sizeof(abi.Stats) and lib.phx_abi_sizeof(27) == C.sizeof(abi.TileMapSummary)  # the earlier indices stay
    assert abi.Stats._fields_[-1][0] == "shade_kernels"


def test_the_structs_own_refusals_need_no_device():
    """mode and the reserved words are checked before the device is looked at: PHX_ERR_ARG with the field's name"""
    from phosphorus_mk2_amd import abi, scenes
    lib = _library()
    s, keep = scenes.cornell(8, 8).pack()
    call = lambda u: (lib.phx_dev_update_geometry(None, C.byref(s), C.byref(u), None), lib.phx_last_error().decode())
    for k in range(3):
        u = abi.GeometryUpdate(mode=abi.UPDATE_REFIT); u.reserved[k] = 1
        rc, why = call(u)
        assert rc == ERR_ARG and "reserved" in why and "must be 0" in why
    rc, why = call(abi.GeometryUpdate(mode=2))
    assert rc == ERR_ARG and "mode" in why
    rc, why = call(abi.GeometryUpdate(mode=abi.UPDATE_REBUILD))
    assert rc == ERR_ARG and "null device" in why
    assert lib.phx_dev_update_geometry(None, None, None, None) == ERR_ARG
    assert lib.phx_dev_update_geometry_times(None, None) == ERR_ARG


def test_header_states_the_structs_and_the_contract():
    hdr = NL.header()
    assert re.search(r"enum \{ PHX_UPDATE_REFIT = 0, PHX_UPDATE_REBUILD = 1 \};", hdr)
    assert re.findall(r"\b(\w+)(?:\[3\])?;", NL.struct_body("phx_geometry_update")) == ["mode", "reserved"]
    assert re.search(r"uint32_t\s+reserved\[3\];\s*/\* must be 0 \*/", NL.struct_body("phx_geometry_update", strip_comments=False))
    body = NL.struct_body("phx_geometry_summary")
    assert re.search(r"uint32_t\s+mode,\s*triangles,\s*nodes,\s*levels,\s*lights,\s*light_triangles;", body) and re.search(r"float\s+bounds\[6\];", body)
    assert re.search(r"float\s+delta;", body)
    assert re.search(r"int\s+phx_dev_update_geometry\(phx_device\* dev, const phx_scene\* moved, const phx_geometry_update\* u, phx_geometry_summary\* summary", hdr)
    assert re.search(r"int\s+phx_dev_update_geometry_times\(const phx_device\* dev, double\* ms /\* 4 \*/\);", hdr)
    text = NL.flat(hdr[hdr.index("geometry updates (DESIGN 27)"):hdr.index("enum { PHX_UPDATE_REFIT")])
    for phrase in ["`moved` is the committed scene with other vertex positions and normals", "v0, e0 = b - a, e1 = c - a", "the scene grid",
                   "the shade records (flat normals)", "the area CDF, the power selection table with the environment's entry",
                   "It does not re-read, re-bake or re-upload materials, lobes, textures and texels, the environment image and its CDF, UV values, options, or the camera",
                   "a triangle's box from its three vertices", "the fp32 min / max of its children's", "encoded again on the scene grid of the NEW bounds",
                   "Slot order and cuts are those of the OLD geometry", "when to rebuild is the caller's decision", "Films accumulated before an update are stale",
                   "Topology changes need phx_dev_preprocess", "the device untouched and still serving its old scene", "the triangle count",
                   "material | smooth << 31", "the number of lights or a light's triangle count", "whether any face is smooth", "the texture classes",
                   "a vertex that is not finite", "The face index arrays themselves are not compared: the triangles given are the triangles rendered",
                   "PHX_ERR_STATE without a preprocessed scene and while a frame is started and not joined",
                   "A failure after the first device write leaves the device without a scene", "no more memory after the call than before",
                   "returns after synchronising the device's stream"]:
        assert phrase in text, phrase
    assert "update_geometry" not in NL.struct_body("phx_stats")


# ---- 2. the movers ------------------------------------------------------------------------------------------------------------------------------
def test_transformed_and_wobbled_make_new_scenes_and_round_once_per_operation():
    from phosphorus_mk2_amd import scenes
    sc = scenes.smooth_blobs(16, 16)
    before = [(m.vertices.copy(), m.normals.copy()) for m in sc.meshes]
    m = np.array([[0.36, 0.0, 0.8, 0.3], [0.0, 1.0, 0.0, -0.2], [-0.8, 0.0, 0.36, 0.1]], F)
    k = max(range(len(sc.meshes)), key=lambda i: len(sc.meshes[i].normals))
    out = scenes.transformed(sc, {k: m})
    assert out is not sc and out.meshes[k] is not sc.meshes[k] and all(out.meshes[i] is sc.meshes[i] for i in range(len(sc.meshes)) if i != k)
    assert out.materials is sc.materials and out.camera is sc.camera and np.shares_memory(out.meshes[k].faces, sc.meshes[k].faces)
    assert all(np.array_equal(a.vertices, v) and np.array_equal(a.normals, n) for a, (v, n) in zip(sc.meshes, before)), "the input was changed"
    v = sc.meshes[k].vertices
    for row in range(3):  # (m0 x + m1 y) + m2 z + t, every operation rounded to float32 on its own
        want = F(F(F(m[row, 0] * v[:, 0]) + F(m[row, 1] * v[:, 1])) + F(m[row, 2] * v[:, 2])) + m[row, 3]
        assert bits_equal(out.meshes[k].vertices[:, row], want.astype(F))
        nn = sc.meshes[k].normals
        want_n = F(F(m[row, 0] * nn[:, 0]) + F(m[row, 1] * nn[:, 1])) + F(m[row, 2] * nn[:, 2])
        assert bits_equal(out.meshes[k].normals[:, row], want_n.astype(F))
    w = scenes.wobbled(sc, 0.05, seed=2)
    assert all(np.array_equal(a.vertices, v) for a, (v, _) in zip(sc.meshes, before))
    d = np.concatenate([a.vertices - b.vertices for a, b in zip(w.meshes, sc.meshes)])
    assert 0.0 < np.abs(d).max() <= 0.05 + 1e-6 and all(np.array_equal(a.normals, b.normals) and np.shares_memory(a.faces, b.faces) for a, b in zip(w.meshes, sc.meshes))
    assert np.array_equal(tri_abc(scenes.wobbled(sc, 0.05, seed=2)), tri_abc(w)) and not np.array_equal(tri_abc(scenes.wobbled(sc, 0.05, seed=3)), tri_abc(w))


# ---- 3. flatten_geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat():
    """-> (flatten(scene, light_sampling), flatten_geometry(committed, moved, light_sampling)): the status, the message and the geometry's tables"""
    from phosphorus_mk2_amd import abi
    lib = NL.load("update_geometry_host", registry=REGISTRY)
    lib.hf_flatten.restype = C.c_void_p; lib.hf_flatten.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Options)]
    lib.hg_flatten_geometry.restype = C.c_void_p; lib.hg_flatten_geometry.argtypes = [C.POINTER(abi.Scene), C.POINTER(abi.Scene), C.POINTER(abi.Options)]
    lib.hf_free.argtypes = [C.c_void_p]
    lib.hf_status.argtypes = [C.c_void_p]
    lib.hf_error.restype = C.c_char_p; lib.hf_error.argtypes = [C.c_void_p]
    lib.hf_array.restype = C.c_void_p; lib.hf_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.hg_power_table.restype = C.c_void_p; lib.hg_power_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.hg_environment.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)]

    def read(h):
        try:
            out = {"status": lib.hf_status(h), "error": lib.hf_error(h).decode()}
            if out["status"] == 0:
                n = C.c_uint64(0)
                for name, which in GEOMETRY_ARRAYS.items():
                    p = lib.hf_array(h, which, C.byref(n))
                    out[name] = np.frombuffer(C.string_at(p, n.value) if n.value else b"", np.uint32).copy()
                p = lib.hg_power_table(h, C.byref(n))
                out["light_pcdf"] = np.frombuffer(C.string_at(p, n.value) if n.value else b"", np.uint32).copy()
                env_p, env_w = C.c_float(0), C.c_double(0)
                lib.hg_environment(h, C.byref(env_p), C.byref(env_w))
                out["env"] = (np.float32(env_p.value).view(np.uint32), np.float64(env_w.value).view(np.uint64))
            return out
        finally:
            lib.hf_free(h)

    def options(light_sampling):
        opt = abi.Options(); opt.light_sampling = light_sampling; opt.path_depth = 9
        return opt

    def flatten(scene, light_sampling=0):
        s, keep = scene.pack()
        return read(lib.hf_flatten(C.byref(s), C.byref(options(light_sampling))))

    def flatten_geometry(committed, moved, light_sampling=0):
        a, keep_a = committed.pack(); b, keep_b = moved.pack()
        return read(lib.hg_flatten_geometry(C.byref(a), C.byref(b), C.byref(options(light_sampling))))
    return flatten, flatten_geometry


def lamp_room(env=False):
    """a floor, a smooth bump with vertex normals, two lamps that share ONE emitter material (2 + 2 triangles, two face sets of one mesh), a
    third lamp with an image on its emission; env: under an image sky"""
    from phosphorus_mk2_amd import abi, scenes
    rng = np.random.default_rng(11)
    floor = scenes._quad((-2, -1, -1), (2, -1, -1), (2, -1, -5), (-2, -1, -5), 0)
    v = np.array([(-0.5, -1, -2.5), (0.5, -1, -2.5), (0.5, -1, -3.5), (-0.5, -1, -3.5), (0, -0.4, -3)], F)
    n = v - np.array([0, -1.6, -3], F)
    bump = scenes.MeshDesc(vertices=v, faces=np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.uint32), sets=[(0, np.arange(4, dtype=np.uint32))],
                           normals=(n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F), smooth=np.array([1, 1, 0, 1], np.uint8))
    lv = np.array([(-1.2, 1, -2), (-1.2, 1, -2.6), (-0.6, 1, -2.6), (-0.6, 1, -2), (0.6, 1, -3), (0.6, 1, -3.9), (1.4, 1, -3.9), (1.4, 1, -3)], F)
    lamps = scenes.MeshDesc(vertices=lv, faces=np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32),
                            sets=[(1, np.array([0, 1], np.uint32)), (1, np.array([2, 3], np.uint32))])
    panel = scenes._quad((-0.3, 0.9, -4.2), (-0.3, 0.9, -4.8), (0.3, 0.9, -4.8), (0.3, 0.9, -4.2), 2)
    panel.uvs = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F)
    mats = [scenes.diffuse(0.7, 0.7, 0.7), scenes.emitter(5.0, 4.0, 3.0), scenes.MaterialDesc([], (1.0, 2.0, 9.0), True, emission_uv_texture=1)]
    tex = [scenes.TextureDesc(rng.uniform(0.1, 1.0, (4, 4, 3)).astype(F))]
    sc = scenes.SceneDesc([floor, bump, lamps, panel], mats, scenes.CameraDesc(16, 16), name="lamp_room", textures=tex)
    if env:
        sc.materials.append(scenes.MaterialDesc(lobes=[], emission=(1.0, 1.0, 1.0), emission_texture=2, emission_mapping=abi.ENV_LATLONG_Y_UP))
        sc.environment_material = 3
        sc.textures.append(scenes.TextureDesc(scenes.sun_and_sky(sun=30.0), abi.TEX_CLOSEST, abi.WRAP_PERIODIC, abi.WRAP_CLAMP))
    return sc


STRETCH = np.array([[1.7, 0.0, 0.3, 0.2], [0.0, 1.0, 0.0, -0.1], [-0.2, 0.0, 0.6, 0.4]], F)
TURN = np.array([[0.8, 0.0, 0.6, 0.1], [0.0, 1.0, 0.0, 0.2], [-0.6, 0.0, 0.8, -0.3]], F)


@pytest.mark.parametrize("light_sampling", MODES, ids=[hex(m) for m in MODES])
def test_flatten_geometry_equals_flatten_scene_of_the_moved_scene(flat, light_sampling):
    from phosphorus_mk2_amd import scenes
    flatten, flatten_geometry = flat
    sc = lamp_room(env=light_sampling == 0x301)
    for new in (sc, scenes.transformed(sc, {1: TURN, 2: STRETCH, 3: STRETCH}), scenes.wobbled(sc, 0.3, seed=4),
                scenes.transformed(sc, {k: np.array([[1, 0, 0, 1.0e4], [0, 1, 0, 0], [0, 0, 1, 0]], F) for k in range(4)})):
        want, got = flatten(new, light_sampling), flatten_geometry(sc, new, light_sampling)
        assert want["status"] == 0 and got["status"] == 0, (want["error"], got["error"])
        for name in list(GEOMETRY_ARRAYS) + ["light_pcdf"]:
            assert np.array_equal(got[name], want[name]), f"{name} differs from flatten_scene's of the moved scene"
        assert got["env"] == want["env"]
        assert len(want["light_pcdf"]) == {0: 0, 1: 0, 0x101: 3, 0x301: 4}[light_sampling] and len(want["light_cdf"]) == (6 if light_sampling else 0)
    # the stretch shows where it should: the lamps' areas and pick densities moved, their emission did not
    base, moved = flatten(sc, light_sampling), flatten_geometry(sc, scenes.transformed(sc, {2: STRETCH}), light_sampling)
    a, b = base["lights"].view(LIGHT), moved["lights"].view(LIGHT)
    assert (a["area"][:2] != b["area"][:2]).all() and (a["lpdf"][:2] != b["lpdf"][:2]).all() and a["area"][2] == b["area"][2]
    assert np.array_equal(a["e"], b["e"]) and np.array_equal(a["num_tris"], b["num_tris"])
    if light_sampling & 0x100:
        assert not np.array_equal(base["light_pcdf"], moved["light_pcdf"])


def test_every_refusal_is_err_arg_with_its_reason(flat):
    from phosphorus_mk2_amd import abi, scenes
    _, flatten_geometry = flat
    sc = lamp_room()
    mesh = lambda k, **kw: replace(sc, meshes=[replace(m, **kw) if i == k else m for i, m in enumerate(sc.meshes)])
    u32 = lambda *x: np.array(x, np.uint32)
    nan = sc.meshes[0].vertices.copy(); nan[2, 1] = np.nan
    inf = sc.meshes[3].vertices.copy(); inf[0, 0] = np.inf
    textured = [scenes.MaterialDesc(lobes=[scenes.LobeDesc(abi.LOBE_DIFFUSE, (0.7, 0.7, 0.7), fac_mode=abi.FAC_TEX_B, fac_texture=1)])] + sc.materials[1:]
    plain = replace(sc, materials=sc.materials[:2] + [scenes.emitter(1.0, 2.0, 9.0)])
    cases = [
        ("the triangle count", mesh(1, sets=[(0, u32(0, 1, 2))])),
        ("the material word of primitive 4", mesh(1, sets=[(0, u32(0, 1)), (1, u32(2)), (0, u32(3))])),   # (an emitter where none was: the word differs first)
        ("the material word of primitive 4", mesh(1, smooth=np.array([1, 1, 1, 1], np.uint8))),           # the smooth bit of one face
        ("the number of lights", mesh(2, sets=[(1, u32(0, 1, 2, 3))])),                                   # the two lamps as one light: same words, same count
        ("the triangle count of light 0", mesh(2, sets=[(1, u32(0, 1, 2)), (1, u32(3))])),                # 3 + 1 for 2 + 2
        ("any_smooth", mesh(1, smooth=np.zeros(4, np.uint8))),
        ("the texture classes", replace(sc, materials=textured)),                                         # a mask appears
        ("the texture classes", plain),                                                                   # the emitter's image goes
        ("is not finite", mesh(0, vertices=nan)),
        ("is not finite", mesh(3, vertices=inf)),
        ("face index out of range", mesh(0, sets=[(0, u32(0, 2))])),                                      # what flatten_scene refuses
        ("vertex index out of range", mesh(0, faces=np.array([[0, 1, 2], [0, 2, 4]], np.uint32))),
        ("material table", replace(sc, materials=sc.materials + [scenes.diffuse(0.1, 0.1, 0.1)])),
    ]
    for why, bad in cases:
        r = flatten_geometry(sc, bad)
        assert r["status"] == ERR_ARG and why in r["error"], (why, r)
    ok = flatten_geometry(sc, replace(sc, meshes=[replace(sc.meshes[0], faces=np.array([[0, 2, 3], [0, 1, 2]], np.uint32))] + sc.meshes[1:]))
    assert ok["status"] == 0, "the face index arrays are not compared: other faces over the same counts are other triangles, not a refusal"
