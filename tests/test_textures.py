"""Image textures on BSDF colour inputs (phx_texture, phx_lobe.texture, phx_mesh.uvs): CPU checks of the C ABI's layout and of the
scene plumbing.  The device is checked in tests/test_gpu_textures.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from phosphorus_mk2_amd import xpu
    lib = C.CDLL(xpu.LIB_PATH)
    lib.phx_abi_sizeof.argtypes = [C.c_int]; lib.phx_abi_sizeof.restype = C.c_uint32
    return lib


def test_texture_structs_match_the_library(lib):
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Texture) == lib.phx_abi_sizeof(10) == 40
    assert C.sizeof(abi.Mesh) == lib.phx_abi_sizeof(4)
    assert C.sizeof(abi.Scene) == lib.phx_abi_sizeof(6)
    assert C.sizeof(abi.Lobe) == lib.phx_abi_sizeof(1) == 64  # `pad` became `texture`: the lobe keeps its size and layout
    assert C.sizeof(abi.Material) == lib.phx_abi_sizeof(2)


def test_texture_field_offsets_match_the_header(tmp_path):
    """offsets of every new field as a C99 compiler lays the header out, against the ctypes mirror"""
    from phosphorus_mk2_amd import abi
    fields = [("phx_texture", abi.Texture, f) for f, _ in abi.Texture._fields_]
    fields += [("phx_mesh", abi.Mesh, "uvs"), ("phx_mesh", abi.Mesh, "num_uvs"), ("phx_scene", abi.Scene, "num_textures"),
               ("phx_scene", abi.Scene, "textures"), ("phx_lobe", abi.Lobe, "texture"), ("phx_lobe", abi.Lobe, "pre_weight")]
    body = "".join(f'  printf("%zu\\n", offsetof({s}, {f}));\n' for s, _, f in fields)
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phx_xpu.h"\nint main(void){\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(t, f).offset for _, t, f in fields]


def test_pack_carries_textures_uvs_and_lobe_texture():
    from phosphorus_mk2_amd import abi, scenes
    sc = scenes.cornell(8, 8)
    img = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)  # H = 2, W = 3
    sc.textures = [scenes.TextureDesc(img, abi.TEX_CLOSEST, abi.WRAP_CLAMP, abi.WRAP_BLACK)]
    sc.materials[0].lobes[0].texture = 1
    sc.meshes[0].uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    s, keep = sc.pack()
    assert s.num_textures == 1
    t = s.textures[0]
    assert (t.width, t.height, t.filter, t.swrap, t.twrap) == (3, 2, abi.TEX_CLOSEST, abi.WRAP_CLAMP, abi.WRAP_BLACK)
    assert [t.texels[k] for k in range(18)] == list(img.reshape(-1))
    assert s.materials[0].lobes[0].texture == 1 and s.materials[1].lobes[0].texture == 0
    m0, m1 = s.meshes[0], s.meshes[1]
    assert m0.num_uvs == 4 and [m0.uvs[k] for k in range(8)] == [0, 0, 1, 0, 1, 1, 0, 1]
    assert m1.num_uvs == 0
    # a scene without textures packs exactly as before: no table, zero counts
    s2, keep2 = scenes.cornell(8, 8).pack()
    assert s2.num_textures == 0 and not s2.textures and all(s2.meshes[i].num_uvs == 0 for i in range(s2.num_meshes))


def test_texture_desc_wants_rgb_rows():
    from phosphorus_mk2_amd import scenes
    with pytest.raises(ValueError):
        scenes.TextureDesc(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        scenes.TextureDesc(np.zeros((4, 4, 4), np.float32))


def test_textured_showroom_drives_the_diffuse_recipes():
    from phosphorus_mk2_amd import abi, scenes
    s = scenes.textured_showroom(2000, 64, 48, tex_size=8)
    b = scenes.textured_showroom(2000, 64, 48, tex_size=8, baked=True)
    textured = [(i, m.lobes[0].texture) for i, m in enumerate(s.materials) if m.lobes and m.lobes[0].texture]
    assert len(textured) == len(s.textures) >= 5  # the room + the sphere recipes of one Lambert lobe
    assert all(s.materials[i].lobes[0].type == abi.LOBE_DIFFUSE and len(s.materials[i].lobes) == 1 for i, _ in textured)
    assert all(t.texels.shape == (8, 8, 3) for t in s.textures) and all(t.texels.shape == (1, 1, 3) for t in b.textures)
    assert np.allclose([t.texels.reshape(-1, 3).mean(0) for t in s.textures], [t.texels[0, 0] for t in b.textures], atol=1e-6)
    assert all(len(m.uvs) in (len(m.vertices), 3 * len(m.faces)) for m in s.meshes)


# ---- closures.py: texture_node -> Cs ---------------------------------------------------------------------------------------------------
def _mat(shaders, connect):
    return {"shaders": shaders, "connect": [{"from": {"layer": a, "slot": s}, "to": {"layer": b, "slot": t}} for a, s, b, t in connect]}


TEX = {"name": "texture_node", "layer": "tex", "parameters": [{"name": "filename", "type": "string", "value": "wood.ppm"},
                                                               {"name": "twrap", "type": "string", "value": "clamp"}]}


def test_texture_node_on_a_diffuse_colour_under_a_mix_bakes_into_weight_and_texture():
    from phosphorus_mk2_amd import abi, closures as cl
    f32 = np.float32
    desc = _mat([TEX,
                 {"name": "diffuse_bsdf_node", "layer": "d"},
                 {"name": "glossy_bsdf_node", "layer": "g", "parameters": [{"name": "Cs", "type": "rgb", "value": [0.5, 0.4, 0.3]},
                                                                           {"name": "roughness", "type": "float", "value": 0.2}]},
                 {"name": "mix_closure_node", "layer": "m", "parameters": [{"name": "fac", "type": "float", "value": 0.3}]}],
                [("tex", "Cout", "d", "Cs"), ("d", "Cout", "m", "A"), ("g", "Cout", "m", "B")])
    textures = [{"filename": "other.npy", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_PERIODIC}]
    m = cl.bake_material(desc, textures)
    assert [l.type for l in m.lobes] == [abi.LOBE_DIFFUSE, abi.LOBE_MICROFACET]
    d, g = m.lobes
    assert d.texture == 2 and g.texture == 0  # appended behind the spec that was already in the table
    assert textures[1] == {"filename": "wood.ppm", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_CLAMP}
    assert d.weight == tuple(float(x) for x in np.full(3, f32(1) - f32(0.3), f32))  # the constant weight ABOVE the texture: the mix's 1 - fac
    assert np.allclose(g.weight, np.float32(0.3) * np.array([0.5, 0.4, 0.3], np.float32), rtol=0, atol=0)
    # the same image twice in one scene is one table entry
    m2 = cl.bake_material(desc, textures)
    assert m2.lobes[0].texture == 2 and len(textures) == 2
    # under the glass node's Fresnel mix: the factor and the texture on one lobe
    glass = _mat([TEX, {"name": "refraction_bsdf_node", "layer": "r", "parameters": [{"name": "IoR", "type": "float", "value": 1.45}]},
                  {"name": "glossy_bsdf_node", "layer": "g"}, {"name": "fresnel_dielectric_node", "layer": "f"}, {"name": "mix_closure_node", "layer": "m"}],
                 [("tex", "Cout", "r", "Cs"), ("r", "Cout", "m", "A"), ("g", "Cout", "m", "B"), ("f", "out", "m", "fac")])
    gm = cl.bake_material(glass, textures)
    assert gm.lobes[0].texture == 2 and gm.lobes[0].fac_mode == abi.FAC_MIX_A and gm.lobes[1].texture == 0


@pytest.mark.parametrize("case", ["fac", "emission", "roughness", "texture_behind_texture", "mirror", "default", "blur"])
def test_texture_node_where_it_cannot_be_expressed_raises(case):
    from phosphorus_mk2_amd import closures as cl
    tex = dict(TEX, parameters=list(TEX["parameters"]))
    d = {"name": "diffuse_bsdf_node", "layer": "d"}
    if case == "fac":
        desc = _mat([tex, d, {"name": "glossy_bsdf_node", "layer": "g"}, {"name": "mix_closure_node", "layer": "m"}],
                    [("tex", "Cout", "m", "fac"), ("d", "Cout", "m", "A"), ("g", "Cout", "m", "B")])
    elif case == "emission":
        desc = _mat([tex, {"name": "diffuse_emitter_node", "layer": "e"}], [("tex", "Cout", "e", "Cs")])
    elif case == "roughness":
        desc = _mat([tex, d], [("tex", "Cout", "d", "roughness")])
    elif case == "texture_behind_texture":
        desc = _mat([tex, dict(tex, layer="tex2"), d], [("tex", "Cout", "tex2", "s"), ("tex2", "Cout", "d", "Cs")])
    else:
        extra = {"mirror": ("swrap", "string", "mirror"), "default": ("twrap", "string", "default"), "blur": ("sblur", "float", 0.5)}[case]
        tex["parameters"] = tex["parameters"] + [{"name": extra[0], "type": extra[1], "value": extra[2]}]
        desc = _mat([tex, d], [("tex", "Cout", "d", "Cs")])
    with pytest.raises(ValueError):
        cl.bake_material(desc, [])


# ---- sceneio: OBJ vt, images ----------------------------------------------------------------------------------------------------------
QUAD_V = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\n"


def test_obj_vt_per_vertex(tmp_path):
    from phosphorus_mk2_amd import abi, sceneio
    p = tmp_path / "q.obj"
    p.write_text(QUAD_V + "vt 0.1 0.2\nvt 0.3 0.4\nvt 0.5 0.6\nvt 0.7 0.8\nvn 0 0 1\nf 1/1/1 2/2/1 3/3/1 4/4/1\n")
    m = sceneio.load_obj(str(p), {})
    assert m.flags & abi.MESH_UV_PER_VERTEX and len(m.uvs) == 4
    assert np.array_equal(m.uvs, np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6], [0.7, 0.8]], np.float32))
    p.write_text(QUAD_V + "vt 0.1 0.2\nvt 0.3 0.4\nvt 0.5 0.6\nvt 0.7 0.8\nf 1/1 2/2 3/3\n")  # the v/vt form
    m = sceneio.load_obj(str(p), {})
    assert m.flags & abi.MESH_UV_PER_VERTEX and len(m.uvs) == 4
    p.write_text(QUAD_V + "f 1 2 3 4\n")  # no UVs at all
    assert len(sceneio.load_obj(str(p), {}).uvs) == 0


def test_obj_vt_per_corner(tmp_path):
    """UV seams: the file indexes UVs apart from positions -> one UV per face corner (3 f + k), the fan's corners in order"""
    from phosphorus_mk2_amd import abi, sceneio
    p = tmp_path / "q.obj"
    p.write_text(QUAD_V + "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.5 0.5\nvn 0 0 1\nf 1/5/1 2/2/1 3/3/1 4/4/1\n")
    m = sceneio.load_obj(str(p), {})
    assert not (m.flags & abi.MESH_UV_PER_VERTEX) and len(m.uvs) == 3 * len(m.faces) == 6
    assert np.array_equal(m.uvs, np.array([[0.5, 0.5], [1, 0], [1, 1], [0.5, 0.5], [1, 1], [0, 1]], np.float32))
    p.write_text(QUAD_V + "vt 0 0\nvt 1 0\nvt 1 1\nf 1/1 2/2 3/3\nf 1 3 4\n")  # a face without vt: (0, 0) at its corners
    m = sceneio.load_obj(str(p), {})
    assert not (m.flags & abi.MESH_UV_PER_VERTEX) and np.array_equal(m.uvs[3:], np.zeros((3, 2), np.float32))


def test_ppm_pfm_npy_images(tmp_path):
    from phosphorus_mk2_amd import sceneio
    rng = np.random.default_rng(1)
    img8 = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)  # H 3, W 5: asymmetric
    (tmp_path / "a.ppm").write_bytes(b"P6\n# a comment\n5 3\n255\n" + img8.tobytes())
    got = sceneio.load_image(str(tmp_path / "a.ppm"))
    assert got.dtype == np.float32 and got.shape == (3, 5, 3)
    assert np.array_equal(got, img8.astype(np.float32) / np.float32(255.0))
    # PFM stores the BOTTOM row first: the file's first row must come back as the last
    top_first = rng.uniform(-1, 2, (3, 5, 3)).astype(np.float32)
    (tmp_path / "b.pfm").write_bytes(b"PF\n5 3\n-1.0\n" + np.ascontiguousarray(top_first[::-1]).astype("<f4").tobytes())
    got = sceneio.load_image(str(tmp_path / "b.pfm"))
    assert got.shape == (3, 5, 3) and np.array_equal(got, top_first)
    (tmp_path / "c.pfm").write_bytes(b"PF\n5 3\n1.0\n" + np.ascontiguousarray(top_first[::-1]).astype(">f4").tobytes())  # big-endian
    assert np.array_equal(sceneio.load_image(str(tmp_path / "c.pfm")), top_first)
    sceneio.save_pfm(str(tmp_path / "d.pfm"), top_first)  # the module's own writer round-trips
    assert np.array_equal(sceneio.load_image(str(tmp_path / "d.pfm")), top_first)
    np.save(tmp_path / "e.npy", top_first)
    assert np.array_equal(sceneio.load_image(str(tmp_path / "e.npy")), top_first)
    (tmp_path / "f.ppm").write_bytes(b"P6\n1 1\n65535\n" + b"\0" * 6)
    with pytest.raises(ValueError):
        sceneio.load_image(str(tmp_path / "f.ppm"))


def test_yaml_scene_with_an_image_texture(tmp_path):
    """YAML + OBJ + PPM: the texture table, the lobe's texture index and the mesh's UVs arrive in the scene, and it packs"""
    import yaml
    from phosphorus_mk2_amd import abi, sceneio
    (tmp_path / "tex").mkdir()
    (tmp_path / "tex" / "wood.ppm").write_bytes(b"P6 2 1 255\n" + bytes([255, 0, 0, 0, 255, 0]))
    (tmp_path / "m.obj").write_text(QUAD_V + "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nusemtl wood\nf 1/1 2/2 3/3 4/4\n"
                                    "v 0 2 0\nv 1 2 0\nv 1 2 1\nusemtl lamp\nf 5 6 7\n")
    cfg = {"materials": {
        "wood": _mat([dict(TEX, parameters=[{"name": "filename", "type": "string", "value": "tex/wood.ppm"}]), {"name": "diffuse_bsdf_node", "layer": "d"}],
                     [("tex", "Cout", "d", "Cs")]),
        "lamp": {"shaders": [{"name": "diffuse_emitter_node", "layer": "e"}]}},
        "data": [{"path": "m.obj"}], "camera": {"film": {"width": 8, "height": 8}}}
    (tmp_path / "scene.yaml").write_text(yaml.safe_dump(cfg, sort_keys=False))  # material ids follow the map's order
    sc = sceneio.load_scene(str(tmp_path / "scene.yaml"))
    assert len(sc.textures) == 1 and sc.textures[0].filter == abi.TEX_LINEAR
    assert np.array_equal(sc.textures[0].texels, np.array([[[1, 0, 0], [0, 1, 0]]], np.float32))
    assert sc.materials[0].lobes[0].texture == 1 and sc.materials[1].is_emitter
    m = sc.meshes[0]  # the lamp's face has no vt: UVs per face corner, (0, 0) on the lamp
    assert not (m.flags & abi.MESH_UV_PER_VERTEX) and len(m.uvs) == 3 * len(m.faces) == 9
    assert np.array_equal(m.uvs[:6], np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32)) and not m.uvs[6:].any()
    s, keep = sc.pack()
    assert s.num_textures == 1 and s.materials[0].lobes[0].texture == 1 and s.meshes[0].num_uvs == len(sc.meshes[0].uvs) > 0
