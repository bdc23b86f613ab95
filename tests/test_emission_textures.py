"""Textured surface emission (phx_material.emission_uv_texture), the parts that need no GPU: the ABI and its marshalling, flatten_scene's
routing and refusals, the baker's and the loader's opt-in, a numpy fp32 restatement of the rule in include/phx_xpu.h (the light sample's
(s, t) and e * texel; tests/test_gpu_emission_textures.py holds the device to it bit for bit), and the scenes and closed forms the device
is held to, checked here on the CPU oracle's twins first: the oracle knows no image, so a twin carries fp32(e * texel) as the constant
emission of one emitter material per texel."""
import copy
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from native_lib import ERR_ARG
from phosphorus_mk2_amd import abi, scenes
from test_analytic_direct_light import H_LAMP, LAMP, RHO, SPP, W
from test_gpu_textures import np_lookup
from test_light_sampling import (TWO_LAMPS, G_rect, LightTable, _camera, _floor, floor_points, light_sample, moments, rect_nodes, rects_mesh, tri_areas,
                                 z_scores)
from test_scene_flatten import SC_TEX_LOBES, flat  # noqa: F401  (flat: the fixture that loads the host_flatten library)

F = np.float32
SEED = 5  # the striped lamp's and the atlas room's renders


# ---- 1. layout and marshalling --------------------------------------------------------------------------------------------------------------
def test_abi_emission_uv_texture():
    hdr = open(os.path.join(ROOT, "include", "phx_xpu.h")).read()
    # the field took the word `pad` held: the material keeps its size and every other offset
    names = [n for n, _ in abi.Material._fields_]
    assert names == ["num_lobes", "is_emitter", "emission", "emission_texture", "emission_mapping", "emission_uv_texture", "lobes"]
    assert abi.Material.emission_uv_texture.offset == 28 and abi.Material.emission_mapping.offset == 24 and abi.Material.lobes.offset == 32
    assert C.sizeof(abi.Material) == 20 + 12 + 8 * 64 == 544
    m = re.search(r"typedef struct phx_material \{(.*?)\} phx_material;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)
    fields = re.findall(r"^\s*(\w+)\s+(\w+)(?:\[(\w+)\])?;", m.group(1), re.M)
    assert [f[1] for f in fields] == names and fields[5] == ("uint32_t", "emission_uv_texture", "")
    assert "phx_dev_light_emission" in abi.EXPORTS
    assert re.search(r"int phx_dev_light_emission\(phx_device\* dev, uint32_t n, const float\* u3, float\* st, float\* e\);", hdr)
    # ... and phx_dev_light_sample's signature is as it was
    assert "int phx_dev_light_sample(phx_device* dev, uint32_t n, const float* u3, uint32_t* light, uint32_t* tri, float* bary, float* P, float* pdf);" in hdr
    # zero-filled input is a scene without emitter images; scenes marshals the field
    assert abi.Material().emission_uv_texture == 0 and scenes.MaterialDesc().emission_uv_texture == 0
    sc = scenes.cornell(8, 8)
    sc.textures = [scenes.TextureDesc(np.ones((1, 2, 3), F))] * 3
    sc.materials[3].emission_uv_texture = 3
    s, keep = sc.pack()
    assert [s.materials[i].emission_uv_texture for i in range(4)] == [0, 0, 0, 3] and s.materials[3].emission_texture == 0


def test_the_library_exports_the_hook():
    from phosphorus_mk2_amd import xpu
    lib = xpu.load_library()
    assert hasattr(lib, "phx_dev_light_emission") and lib.phx_abi_sizeof(2) == C.sizeof(abi.Material)
    assert callable(xpu.HipDevice.light_emission)


# ---- 2. flatten_scene ---------------------------------------------------------------------------------------------------------------------------
IMG42 = np.random.default_rng(9).uniform(0.25, 2.0, (2, 4, 3)).astype(F)
QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)


def lamp_image_box(with_lobes=False):
    """the Cornell box whose lamp carries image 1 on its emission; with_lobes: the lamp also reflects (a Lambert lobe beside the emission)"""
    s = scenes.cornell(32, 32)
    s.textures = [scenes.TextureDesc(IMG42, abi.TEX_LINEAR)]
    s.meshes[5].uvs = QUAD_UV.copy()
    s.materials[3].emission_uv_texture = 1
    if with_lobes:
        s.materials[3].lobes = [scenes.LobeDesc(abi.LOBE_DIFFUSE, (0.5, 0.5, 0.5))]
    return s


@pytest.mark.parametrize("with_lobes", [False, True])
def test_an_emitter_image_is_accepted_and_routes_the_scene_to_the_tex_kernels(flat, with_lobes):
    plain = flat(scenes.cornell(32, 32))
    assert (plain["any_tex"], plain["diffuse_only"], plain["prim_uv"].size, plain["textures"].size) == (0, 2, 0, 0)
    sc = lamp_image_box(with_lobes)
    r = flat(sc)
    assert r["status"] == 0, r
    assert r["any_tex"] == SC_TEX_LOBES and r["diffuse_only"] == 0 and r["mat_lite"].size == 0  # no lobe is textured: the emitter alone routes it
    assert r["any_per_hit"] == 0 and not r["lobe_tex"].any()
    assert r["textures"].reshape(-1, 4).tolist() == [[0, 4, 2, abi.TEX_LINEAR]] and r["texels"].reshape(-1, 4)[:, :3].tobytes() == IMG42.tobytes()
    uv = r["prim_uv"].reshape(-1, 3, 2)  # corner UVs of every primitive: the lamp's two triangles last, zero on meshes without UVs
    assert len(uv) == 12 and not uv[:10].any() and uv[10].tolist() == QUAD_UV[[0, 1, 2]].tolist() and uv[11].tolist() == QUAD_UV[[0, 2, 3]].tolist()
    # the light table is the plain scene's: the image multiplies at the sample, not in the table
    assert r["lights"].tobytes() == plain["lights"].tobytes() and r["light_tris"].tobytes() == plain["light_tris"].tobytes()


def _env(s):
    s.materials.append(scenes.MaterialDesc([], (0.5, 0.5, 0.5), is_emitter=True, emission_uv_texture=1))
    s.environment_material = len(s.materials) - 1


REFUSALS = [
    ("not_an_emitter", lambda s: setattr(s.materials[0], "emission_uv_texture", 1), "material 0: emission_uv_texture is allowed only on emitters"),
    ("on_the_environment", _env, "material 4: emission_uv_texture is not allowed on the environment material"),
    ("past_the_table", lambda s: setattr(s.materials[3], "emission_uv_texture", 2), "material 3: emission_uv_texture index out of range"),
    ("past_an_empty_table", lambda s: setattr(s, "textures", []), "material 3: emission_uv_texture index out of range"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_of_flatten_scene(flat, case):
    name, change, message = case
    s = lamp_image_box()
    good = flat(s)
    assert good["status"] == 0
    change(s)
    r = flat(s)
    assert r["status"] == ERR_ARG and message in r["error"], r
    assert set(r) == {"status", "error"}  # nothing was flattened
    again = flat(lamp_image_box())  # flatten_scene keeps no state: the good scene flattens to the same arrays afterwards
    assert all(np.array_equal(again[k], good[k]) for k in good)


def test_the_environment_image_field_keeps_its_refusal_on_emitters(flat):
    s = lamp_image_box()
    s.materials[3].emission_texture = 1  # the lat-long field stays environment-only, with or without the new one
    r = flat(s)
    assert r["status"] == ERR_ARG and "emission_texture is allowed only on the environment material" in r["error"]


# ---- 3. baker and loader ------------------------------------------------------------------------------------------------------------------------
def _mat(shaders, connect):
    return {"shaders": shaders, "connect": [{"from": {"layer": a, "slot": s}, "to": {"layer": b, "slot": t}} for a, s, b, t in connect]}


def _p(name, value):
    t = "string" if isinstance(value, str) else "rgb" if isinstance(value, (list, tuple)) else "float"
    return {"name": name, "type": t, "value": value}


def _tex(layer="tex", **params):
    return {"name": "texture_node", "layer": layer, "parameters": [_p("filename", "panel.ppm")] + [_p(k, v) for k, v in params.items()]}


EMIT = {"name": "diffuse_emitter_node", "layer": "e", "parameters": [_p("power", 3.0)]}
PANEL = _mat([_tex(twrap="clamp"), EMIT], [("tex", "Cout", "e", "Cs")])


def test_the_default_still_raises_and_names_the_keyword():
    from phosphorus_mk2_amd import closures as cl
    with pytest.raises(ValueError, match="emitter_textures=True"):
        cl.bake_material(PANEL, [])
    with pytest.raises(ValueError, match="emitter_textures=True"):
        cl.bake_material(PANEL, [], emitter_textures=False)
    with pytest.raises(ValueError, match="emitter_textures=True"):
        cl.flatten(cl.diffuse_emitter_node(Cs=cl.texture_node(filename="panel.ppm")))


def test_with_the_keyword_the_graph_bakes_to_emission_and_image():
    from phosphorus_mk2_amd import closures as cl
    textures = [{"filename": "other.npy", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_PERIODIC}]
    m = cl.bake_material(PANEL, textures, emitter_textures=True)
    e = F(F(3.0) / F(math.pi))
    assert m.is_emitter and not m.lobes and m.emission == (float(e),) * 3 and m.emission_texture == 0
    assert m.emission_uv_texture == 2 and textures[1] == {"filename": "panel.ppm", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_CLAMP}
    assert cl.bake_material(PANEL, textures, emitter_textures=True).emission_uv_texture == 2 and len(textures) == 2  # one table entry per image
    # the constant weights above the emitter join the emission: (power / pi) under a mix's 1 - fac, beside an untextured lobe
    mixed = _mat([_tex(), EMIT, {"name": "diffuse_bsdf_node", "layer": "d"}, {"name": "mix_closure_node", "layer": "m", "parameters": [_p("fac", 0.25)]}],
                 [("tex", "Cout", "e", "Cs"), ("e", "Cout", "m", "A"), ("d", "Cout", "m", "B")])
    textures = []
    m = cl.bake_material(mixed, textures, emitter_textures=True)
    assert m.is_emitter and m.emission_uv_texture == 1 and [l.type for l in m.lobes] == [abi.LOBE_DIFFUSE] and m.lobes[0].texture == 0
    assert m.emission == (float(F(F(1) - F(0.25)) * e),) * 3
    # an image on a lobe of the same material stays refused, as flatten_scene refuses it (images on emitters' lobes are not supported)
    both = _mat([_tex(), EMIT, {"name": "diffuse_bsdf_node", "layer": "d"}, {"name": "add_node", "layer": "a"}],
                [("tex", "Cout", "e", "Cs"), ("tex", "Cout", "d", "Cs"), ("e", "Cout", "a", "A"), ("d", "Cout", "a", "B")])
    with pytest.raises(ValueError, match="lobes of an emitter"):
        cl.bake_material(both, [], emitter_textures=True)
    # without an image the keyword changes nothing
    plain = _mat([EMIT], [])
    assert cl.bake_material(plain, [], emitter_textures=True) == cl.bake_material(plain, [])


STILL_RAISES = {
    "texture_into_background": _mat([_tex(), {"name": "background_node", "layer": "b"}], [("tex", "Cout", "b", "Cs")]),
    "environment_into_emitter": _mat([{"name": "environment_node", "layer": "env", "parameters": [_p("filename", "sky.hdr")]}, EMIT], [("env", "Cout", "e", "Cs")]),
    "blur": _mat([_tex(sblur=0.5), EMIT], [("tex", "Cout", "e", "Cs")]),
    "mirror_wrap": _mat([_tex(swrap="mirror"), EMIT], [("tex", "Cout", "e", "Cs")]),
    "emitter_under_a_masked_mix": _mat([_tex(), _tex("mask"), {"name": "luminance_node", "layer": "lum"}, EMIT, {"name": "diffuse_bsdf_node", "layer": "d"},
                                        {"name": "mix_closure_node", "layer": "m"}],
                                       [("tex", "Cout", "e", "Cs"), ("mask", "Cout", "lum", "in"), ("lum", "out", "m", "fac"), ("e", "Cout", "m", "A"), ("d", "Cout", "m", "B")]),
    "emitter_under_a_fresnel_mix": _mat([_tex(), {"name": "fresnel_dielectric_node", "layer": "f"}, EMIT, {"name": "diffuse_bsdf_node", "layer": "d"},
                                         {"name": "mix_closure_node", "layer": "m"}],
                                        [("tex", "Cout", "e", "Cs"), ("f", "out", "m", "fac"), ("e", "Cout", "m", "A"), ("d", "Cout", "m", "B")]),
    "texture_into_power": _mat([_tex(), EMIT], [("tex", "Cout", "e", "power")]),
}


@pytest.mark.parametrize("case", list(STILL_RAISES))
def test_what_the_keyword_does_not_unlock_still_raises(case):
    from phosphorus_mk2_amd import closures as cl
    with pytest.raises(ValueError):
        cl.bake_material(STILL_RAISES[case], [], emitter_textures=True)


SCENE_YAML = """
materials:
  floor:
    shaders:
      - {name: diffuse_bsdf_node, layer: d, parameters: [{name: Cs, type: rgb, value: [0.7, 0.7, 0.7]}]}
  panel:
    shaders:
      - {name: texture_node, layer: tex, parameters: [{name: filename, type: string, value: panel.ppm}, {name: swrap, type: string, value: clamp}]}
      - {name: diffuse_emitter_node, layer: e, parameters: [{name: power, type: float, value: 6.0}]}
    connect:
      - {from: {layer: tex, slot: Cout}, to: {layer: e, slot: Cs}}
data:
  - {path: room.obj}
camera: {position: [0, 1, 3], at: [0, 1, 0], up: [0, 1, 0], film: {width: 16, height: 12}}
"""
SCENE_OBJ = """v -2 0 -2\nv 2 0 -2\nv 2 0 2\nv -2 0 2\nv -1 2 -1\nv 1 2 -1\nv 1 2 1\nv -1 2 1
vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1
usemtl floor\nf 1 4 3 2\nusemtl panel\nf 5/1 6/2 7/3 8/4
"""


def test_a_yaml_obj_ppm_scene_loads(tmp_path, flat):
    from phosphorus_mk2_amd import sceneio
    (tmp_path / "scene.yaml").write_text(SCENE_YAML)
    (tmp_path / "room.obj").write_text(SCENE_OBJ)
    (tmp_path / "panel.ppm").write_bytes(b"P6\n2 1\n255\n" + bytes([255, 0, 0, 0, 51, 255]))
    with pytest.raises(ValueError, match="emitter_textures=True"):
        sceneio.load_scene(str(tmp_path / "scene.yaml"))
    sc = sceneio.load_scene(str(tmp_path / "scene.yaml"), emitter_textures=True)
    panel = sc.materials[1]
    assert panel.is_emitter and panel.emission_uv_texture == 1 and panel.emission == (float(F(F(6.0) / F(math.pi))),) * 3
    assert len(sc.textures) == 1 and sc.textures[0].swrap == abi.WRAP_CLAMP and sc.textures[0].twrap == abi.WRAP_PERIODIC
    assert sc.textures[0].texels.shape == (1, 2, 3) and sc.textures[0].texels[0, 1].tolist() == [0.0, float(F(51) / F(255)), 1.0]
    assert len(sc.meshes[0].uvs) and (sc.camera.width, sc.camera.height) == (16, 12)
    r = flat(sc)
    assert r["status"] == 0 and r["any_tex"] == SC_TEX_LOBES and r["diffuse_only"] == 0 and r["num_lights"] == 1


# ---- 4. the rule, restated in numpy fp32 ------------------------------------------------------------------------------------------------------
def light_corner_uvs(scene):
    """per light (LightTable's order): the corner UVs of its triangles, (n, 3, 2) f32 -- per vertex or per face corner, (0, 0) without UVs --
    and its material"""
    uvs, mats = [], []
    for m in scene.meshes:
        for mat, faces in m.sets:
            if scene.materials[mat].is_emitter and len(faces):
                if not len(m.uvs):
                    uv = np.zeros((len(faces), 3, 2), F)
                elif m.flags & abi.MESH_UV_PER_VERTEX:
                    uv = m.uvs[m.faces[faces]]
                else:
                    uv = m.uvs[3 * faces.astype(np.int64)[:, None] + np.arange(3)]
                uvs.append(uv.astype(F)); mats.append(mat)
    return uvs, mats


def sample_st(uv, bary, rotated=False):
    """(s, t) of the light sample (bu, bv) on triangles of corner UVs uv (n, 3, 2): st = (bu uv_a + bv uv_b) + (1 - bu - bv) uv_c, fp32 in
    this order -- the weights P = bu a + bv b + (1 - bu - bv) c is built with.  rotated: the reference's reading of the same (bu, bv) as
    Moeller-Trumbore barycentrics, st = (w uv_a + bu uv_b) + bv uv_c (mesh.cpp:178-181, 256; light_st_rotated), which this project does not
    reproduce"""
    bu, bv = bary[:, 0:1].astype(F), bary[:, 1:2].astype(F)
    w = ((F(1) - bu) - bv).astype(F)
    if rotated:
        return ((w * uv[:, 0] + bu * uv[:, 1]) + bv * uv[:, 2]).astype(F)
    return ((bu * uv[:, 0] + bv * uv[:, 1]) + w * uv[:, 2]).astype(F)


def light_emission(scene, u3, by_area=False, rotated=False):
    """phx_dev_light_emission restated: (pick, lu, lv) -> st (n, 2), e (n, 3); a light without an image: its constant e, st = (0, 0)"""
    t = LightTable(scene)
    s = light_sample(t, u3, by_area)
    uvs, mats = light_corner_uvs(scene)
    st = np.zeros((len(s["light"]), 2), F); e = np.zeros((len(s["light"]), 3), F)
    for k in range(t.n):
        sel = s["light"] == k
        m = scene.materials[mats[k]]
        em = np.array([F(x) for x in m.emission], F)
        if not m.emission_uv_texture:
            e[sel] = em
            continue
        st[sel] = sample_st(uvs[k][s["tri"][sel]], s["bary"][sel], rotated)
        e[sel] = em[None, :] * np_lookup(scene.textures[m.emission_uv_texture - 1], st[sel])
    return {"st": st, "e": e}


def test_the_light_samples_st_is_the_uv_of_the_sampled_point():
    """on triangles whose UVs are an affine map of their positions, st of a sample is that map of P (to rounding) -- under the rule; under
    the reference's rotated reading it is the map of ANOTHER point of the triangle"""
    rng = np.random.default_rng(3)
    A = rng.uniform(-1, 1, (2, 3)); b = rng.uniform(-1, 1, 2)
    tris = rng.uniform(-1, 1, (64, 3, 3)).astype(F)
    uv = (tris.astype(np.float64) @ A.T + b).astype(F)
    u = rng.random((64, 2), dtype=F)
    x = np.sqrt(u[:, 0]); bary = np.stack([F(1) - x, u[:, 1] * x], -1).astype(F)
    w = (F(1) - bary[:, 0]) - bary[:, 1]
    P = (bary[:, 0:1] * tris[:, 0] + bary[:, 1:2] * tris[:, 1]) + w[:, None] * tris[:, 2]
    want = P.astype(np.float64) @ A.T + b
    assert np.abs(sample_st(uv, bary) - want).max() < 1e-5
    assert np.abs(sample_st(uv, bary, rotated=True) - want).max() > 0.1
    # at the corners of the sample domain the rule returns the corner's UV: bu = 1 -> a, bv = 1 -> b, neither -> c
    corners = np.array([[1, 0], [0, 1], [0, 0]], F)
    for k in range(3):
        assert sample_st(uv, np.tile(corners[k], (64, 1))).tobytes() == uv[:, k].tobytes()


def striped_quad(axis="s", filter=abi.TEX_CLOSEST):
    """item 5's lamp: the rectangular lamp of test_analytic_direct_light, two triangles, UVs over [0, 1]^2 (s along x, t along z), ONE
    light, under a 4 x 1 (axis "s": stripes along x) or 1 x 4 (axis "t": stripes along z, crossing the triangles' shared diagonal) image"""
    lamp = rects_mesh([LAMP], 1)
    lamp.uvs = np.array([[0, 1], [0, 0], [1, 0], [1, 1]], F)  # rects_mesh's corners: (x0, z1), (x0, z0), (x1, z0), (x1, z1)
    img = STRIPES[None, :, :] if axis == "s" else STRIPES[:, None, :]
    mats = [scenes.diffuse(RHO, RHO, RHO), scenes.MaterialDesc([], LE_PANEL, True, emission_uv_texture=1)]
    return scenes.SceneDesc(_floor() + [lamp], mats, _camera(), name=f"striped_quad_{axis}", textures=[scenes.TextureDesc(np.ascontiguousarray(img), filter)])


def test_emission_is_e_times_the_texel_at_that_st():
    sc = striped_quad("s")
    rng = np.random.default_rng(4)
    u3 = rng.random((4096, 3), dtype=F)
    got = light_emission(sc, u3)
    s = light_sample(LightTable(sc), u3, False)
    # s runs along x over the lamp: the stripe is the strip P.x lies in
    k = np.clip(np.floor((s["P"][:, 0].astype(np.float64) - LAMP[0]) / (LAMP[1] - LAMP[0]) * 4), 0, 3).astype(int)
    inside = np.abs((got["st"][:, 0].astype(np.float64) * 4) % 1 - 0.5) < 0.499  # not within rounding of a stripe's border
    want = np.array(LE_PANEL, F)[None, :] * STRIPES[k]
    assert inside.mean() > 0.99 and got["e"][inside].tobytes() == want[inside].astype(F).tobytes()
    assert set(np.unique(k)) == {0, 1, 2, 3}
    assert np.abs(got["st"][:, 0] - (s["P"][:, 0] - F(LAMP[0]))).max() < 1e-6
    # a light without an image: its constant e and st = (0, 0)
    sc.materials[1].emission_uv_texture = 0
    plain = light_emission(sc, u3)
    assert not plain["st"].any() and (plain["e"] == np.array(LE_PANEL, F)).all()
    # the rotated reading lights the floor from one point and colours it by another
    rot = light_emission(striped_quad("s"), u3, rotated=True)
    assert (rot["e"] != got["e"]).any(1).mean() > 0.4


# ---- 5. the closed form the device is held to -----------------------------------------------------------------------------------------------
# Constants of the striped lamp.  The four texels span more than a decade in every channel; e * c is exact in fp32 (powers of two).
LE_PANEL = (4.0, 2.0, 1.0)
STRIPES = np.array([[0.0625, 1.0, 0.25], [2.0, 0.0625, 0.5], [0.25, 0.5, 0.03125], [1.0, 0.125, 1.0]], F)
assert (STRIPES.max(0) / STRIPES.min(0) > 10).all()
X_CUTS = [LAMP[0] + k * (LAMP[1] - LAMP[0]) / 4 for k in range(5)]
Z_CUTS = [LAMP[2] + k * (LAMP[3] - LAMP[2]) / 4 for k in range(5)]
STRIPS_X = [(X_CUTS[k], X_CUTS[k + 1], LAMP[2], LAMP[3]) for k in range(4)]
STRIPS_Z = [(LAMP[0], LAMP[1], Z_CUTS[k], Z_CUTS[k + 1]) for k in range(4)]
INSET = 1.0 / 64  # the four-set lamp's UVs stay this far inside their stripe: no sample's st rounds onto a stripe's border


def stripe_emission(k):
    return tuple(float(F(e) * c) for e, c in zip(LE_PANEL, STRIPES[k]))


def striped_sets(textured=True):
    """the same lamp cut into its four stripes along x, two equal triangles each.  textured: four face sets of ONE emitter material under the
    4 x 1 CLOSEST image, each strip's UVs inside its stripe -- four lights.  Otherwise the oracle's twin: four emitter materials of emission
    fp32(e * c_k) on the same faces in the same order (the same lights, so the same picks)."""
    lamp = rects_mesh(STRIPS_X, 1)
    sets = [(1 if textured else 1 + k, np.array([2 * k, 2 * k + 1], np.uint32)) for k in range(4)]
    lamp.sets = sets
    mats = [scenes.diffuse(RHO, RHO, RHO)]
    textures = []
    if textured:
        s = np.array([[k / 4 + INSET, k / 4 + INSET, (k + 1) / 4 - INSET, (k + 1) / 4 - INSET] for k in range(4)]).reshape(-1)
        lamp.uvs = np.stack([s, np.tile([1.0, 0.0, 0.0, 1.0], 4)], -1).astype(F)
        mats.append(scenes.MaterialDesc([], LE_PANEL, True, emission_uv_texture=1))
        textures = [scenes.TextureDesc(STRIPES[None, :, :].copy(), abi.TEX_CLOSEST)]
    else:
        mats += [scenes.emitter(*stripe_emission(k)) for k in range(4)]
    return scenes.SceneDesc(_floor() + [lamp], mats, _camera(), name="striped_sets" if textured else "striped_twin", textures=textures)


def piecewise_moments(lights, n=64):
    """test_light_sampling.moments for lights whose emission is piecewise constant: lights = [[(rectangle, L_e), ...], ...], the pieces of a
    light tiling it.  One sample picks a light with probability 1/nl and a point uniformly on its area A_l, so per pixel centre and channel,
    in float64 from the closed-form integrand g = h^2 / d^4 alone: mean = sum_pieces k G_piece (closed form) and second moment
    sum_l nl A_l sum_pieces k^2 int_piece g^2 dA (midpoint rule), k = (rho / pi) 4 L_e of the piece.  No render enters it."""
    X, Z = floor_points()
    nl = len(lights)
    mean = np.zeros(X.shape + (3,)); m2 = np.zeros(X.shape + (3,))
    for pieces in lights:
        A = sum((r[1] - r[0]) * (r[3] - r[2]) for r, _ in pieces)
        for r, le in pieces:
            G = G_rect(X, Z, r)
            xs, zs, dA = rect_nodes(r, n)
            d2 = (xs[None, None, :] - X[..., None]) ** 2 + (zs[None, None, :] - Z[..., None]) ** 2 + H_LAMP ** 2
            g2 = ((H_LAMP * H_LAMP / (d2 * d2)) ** 2).sum(-1) * dA
            for c in range(3):
                k = RHO / math.pi * 4.0 * le[c]
                mean[..., c] += k * G
                m2[..., c] += nl * A * k * k * g2
    return mean, m2


def striped_moments(which):
    """the model of "sets" (four lights, one per stripe), of "s" (one light, stripes along x) and of "t" (one light, stripes along z)"""
    if which == "sets":
        return piecewise_moments([[(STRIPS_X[k], stripe_emission(k))] for k in range(4)])
    return piecewise_moments([[((STRIPS_X if which == "s" else STRIPS_Z)[k], stripe_emission(k)) for k in range(4)]])


def within_bounds(film, mean, m2, what):
    """tests/test_gpu_light_sampling.py's bounds for its two-lamp scene: the film mean within 4 of its standard errors per channel, every
    pixel within 5 of its own.  The pixel centre stands for the pixel, as there."""
    z_mean, z_pixel = z_scores(film, mean, m2, SPP)
    print(f"{what}: film mean off by {z_mean} standard errors, worst pixel {z_pixel.max():.2f}, rms {np.sqrt((z_pixel ** 2).mean()):.3f}")
    return bool((z_mean < 4.0).all() and z_pixel.max() < 5.0)


def test_the_piecewise_model_is_the_two_lamp_model_on_constant_lights():
    a = piecewise_moments([[(r, le) for r in rects] for rects, le in TWO_LAMPS], n=16)
    b = moments(TWO_LAMPS, n=16)
    assert np.allclose(a[0], b[0], rtol=1e-12) and np.allclose(a[1], b[1], rtol=1e-12)
    # the three striped models: "sets" and "s" are one estimator (four lights of a quarter of the area each, or one light of the whole area: either
    # way a point uniform on the lamp under the same stripes); "t" lights the floor differently
    (ms, vs), (m1, v1), (mt, _) = striped_moments("sets"), striped_moments("s"), striped_moments("t")
    assert np.allclose(ms, m1, rtol=1e-12) and np.allclose(v1, vs, rtol=1e-12) and np.abs(mt / m1 - 1).max() > 0.1


def test_the_striped_scenes_are_what_they_claim():
    for sc in (striped_sets(True), striped_sets(False)):
        t = LightTable(sc)
        assert t.n == 4 and all(a.tolist() == [0.125, 0.125] for a in t.areas) and t.equal_pairs_only()
    t, b = striped_sets(True), striped_sets(False)
    assert [m.vertices.tobytes() for m in t.meshes] == [m.vertices.tobytes() for m in b.meshes] and not b.textures
    # every sample of strip k reads stripe k, and e * c_k is the twin's emission bit for bit
    u3 = np.random.default_rng(6).random((1 << 14, 3), dtype=F)
    got = light_emission(t, u3)
    k = light_sample(LightTable(t), u3, False)["light"]
    assert got["e"].tobytes() == np.array([stripe_emission(i) for i in range(4)], F)[k].tobytes()
    assert (np.floor(got["st"][:, 0] * F(4)) == k).all()
    q = LightTable(striped_quad("s"))
    assert q.n == 1 and len(q.areas[0]) == 2 and abs(float(q.area[0]) - 1.0) < 1e-6


@pytest.fixture(scope="module")
def twin_film(orc):
    return orc.Oracle(striped_sets(False), spp=SPP, pps=1, depth=1).render(rng=orc.RNG_COUNTER, seed=SEED, threads=4)


def test_the_oracles_four_lamp_twin_meets_the_closed_form(twin_film):
    film, st = twin_film
    assert st["rays_shadow"] == st["rays_closest"] == W * W * SPP
    mean, m2 = striped_moments("sets")
    assert within_bounds(film, mean, m2, "the oracle's twin")
    # the stripes are seen: against the model of the lamp under the image's mean the same film is far outside the bounds
    flat_le = tuple(float(x) for x in np.array(LE_PANEL) * STRIPES.astype(np.float64).mean(0))
    fm, f2 = piecewise_moments([[(STRIPS_X[k], flat_le)] for k in range(4)])
    assert not within_bounds(film, fm, f2, "the oracle's twin against the lamp of the mean texel")


# ---- the atlas room (tests/test_gpu_emission_textures.py, item 7), its twins checked on the oracle first ------------------------------------
ATLAS = np.array([[4.0, 0.25, 0.5], [0.125, 2.0, 0.25], [1.0, 1.0, 4.0], [0.25, 3.0, 0.125], [2.0, 0.125, 1.0], [0.5, 0.5, 2.0], [3.0, 0.25, 0.25], [0.125, 1.0, 3.0]], F)
LE_ATLAS = (6.0, 5.0, 4.0)
ROOM_W, ROOM_H, ROOM_SPP, ROOM_DEPTH = 64, 48, 16, 9


def _sphere(centre, radius, material, nu=12, nv=8):
    v, f = [], []
    for j in range(nv + 1):
        for i in range(nu):
            th, ph = math.pi * j / nv, 2 * math.pi * i / nu
            v.append((centre[0] + radius * math.sin(th) * math.cos(ph), centre[1] + radius * math.cos(th), centre[2] + radius * math.sin(th) * math.sin(ph)))
    for j in range(nv):
        for i in range(nu):
            a, b, c, d = j * nu + i, j * nu + (i + 1) % nu, (j + 1) * nu + (i + 1) % nu, (j + 1) * nu + i
            f += [(a, b, c), (a, c, d)]
    f = np.array(f, np.uint32)
    return scenes.MeshDesc(vertices=np.array(v, F), faces=f, sets=[(material, np.arange(len(f), dtype=np.uint32))])


def atlas_room(mode="atlas", lens=False):
    """A room with a diffuse floor, a mirror for its back wall and a glass sphere, under a lamp of 8 quads on the ceiling: the camera sees
    the lamp directly and in the mirror.  mode "atlas": the quads are 8 face sets of ONE emitter material under an 8 x 1 CLOSEST atlas, each
    quad's UVs strictly inside one texel (per face corner).  "twin": 8 emitter materials of emission fp32(e * texel_k), no image (the
    oracle's scene).  "mean": the atlas replaced by its mean texel; "mean_twin": its twin."""
    box = scenes.cornell(ROOM_W, ROOM_H)
    mats = box.materials[:3] + [scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_REFLECTION, (0.9, 0.9, 0.9), eta=0.0)]), scenes.glass(1.45, 0.0, (0.95, 0.98, 0.95), (1.0, 1.0, 1.0))]
    meshes = box.meshes[:5]
    meshes[2].sets = [(3, meshes[2].sets[0][1])]  # the back wall is the mirror
    meshes.append(_sphere((0.45, -0.6, -2.4), 0.4, 4))
    image = ATLAS if mode in ("atlas", "twin") else np.broadcast_to(ATLAS.astype(np.float64).mean(0).astype(F), ATLAS.shape)
    textured = mode in ("atlas", "mean")
    v, f, uv, sets = [], [], [], []
    for k in range(8):
        qx, qz = k % 4, k // 4
        x0, x1, z0, z1 = -0.8 + 0.4 * qx, -0.8 + 0.4 * (qx + 1), -2.0 - 0.45 * qz, -2.0 - 0.45 * (qz + 1)
        b = len(v)
        v += [(x0, 0.99, z0), (x0, 0.99, z1), (x1, 0.99, z1), (x1, 0.99, z0)]  # n = -y, as the box's lamp
        f += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
        s0, s1 = (k + 0.2) / 8, (k + 0.8) / 8
        c = [(s0, 0.1), (s0, 0.9), (s1, 0.9), (s1, 0.1)]
        uv += [c[0], c[1], c[2], c[0], c[2], c[3]]
        if textured:
            sets.append((len(mats), np.array([2 * k, 2 * k + 1], np.uint32)))
        else:
            sets.append((len(mats) + k, np.array([2 * k, 2 * k + 1], np.uint32)))
    if textured:
        mats.append(scenes.MaterialDesc([], LE_ATLAS, True, emission_uv_texture=2))
        lamp = scenes.MeshDesc(np.array(v, F), np.array(f, np.uint32), sets, flags=abi.MESH_NORMALS_PER_VERTEX, uvs=np.array(uv, F))
        # the atlas is texture 2 behind a decoy no material names: an index read off by one changes the film
        textures = [scenes.TextureDesc(np.full((2, 2, 3), (0.3, 7.0, 0.01), F)), scenes.TextureDesc(np.ascontiguousarray(image[None, :, :]), abi.TEX_CLOSEST)]
    else:
        mats += [scenes.emitter(*(float(F(e) * c) for e, c in zip(LE_ATLAS, image[k]))) for k in range(8)]
        lamp = scenes.MeshDesc(np.array(v, F), np.array(f, np.uint32), sets)
        textures = []
    sc = scenes.SceneDesc(meshes + [lamp], mats, scenes.CameraDesc(ROOM_W, ROOM_H, box.camera.fov), name=f"atlas_room_{mode}", textures=textures)
    if lens:
        sc.camera.aperture_radius, sc.camera.focal_distance = 0.03, 3.0
    return sc


def pixels_differing(a, b):
    return float((np.ascontiguousarray(a[..., :3]).view(np.uint32) != np.ascontiguousarray(b[..., :3]).view(np.uint32)).any(-1).mean())


def test_the_atlas_rooms_twins_differ_where_the_device_films_must(orc):
    """every sample of quad k reads texel k (the restatement), and the oracle's twin of the atlas differs from its twin of the mean texel
    in at least a quarter of the pixels: the image reaches the film"""
    sc = atlas_room("atlas")
    t = LightTable(sc)
    assert t.n == 8 and t.equal_pairs_only()
    u3 = np.random.default_rng(8).random((1 << 14, 3), dtype=F)
    got = light_emission(sc, u3)
    k = light_sample(t, u3, False)["light"]
    assert got["e"].tobytes() == (np.array(LE_ATLAS, F)[None, :] * ATLAS[k]).astype(F).tobytes()
    orc.set_tie_rule(1)
    try:
        a, sa = orc.Oracle(atlas_room("twin"), spp=ROOM_SPP, pps=1, depth=ROOM_DEPTH).render(rng=orc.RNG_COUNTER, seed=SEED, threads=8)
        m, sm = orc.Oracle(atlas_room("mean_twin"), spp=ROOM_SPP, pps=1, depth=ROOM_DEPTH).render(rng=orc.RNG_COUNTER, seed=SEED, threads=8)
    finally:
        orc.set_tie_rule(0)
    assert np.isfinite(a).all() and a[..., :3].max() > 0.05
    assert all(sa[c] == sm[c] for c in ("camera_samples", "rays_closest", "rays_shadow", "rays_masked"))  # the same paths, another emission
    changed = pixels_differing(a, m)
    print(f"atlas against its mean texel: {changed:.1%} of the oracle's pixels differ")
    assert changed >= 0.25
    # the lamp is seen directly (the brightest texel's colour appears on the film as e * c itself) and through the mirror and the glass (depth > 1 paths exist)
    direct = (np.array(LE_ATLAS, F) * ATLAS[0]).astype(F)
    assert (np.abs(a[..., :3] / direct - 1).max(-1) < 1e-4).any()
    assert sa["rays_closest"] > 1.5 * sa["camera_samples"]
