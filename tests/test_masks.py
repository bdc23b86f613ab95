"""Image masks on closure mixes (phx_lobe.fac_mode = PHX_FAC_TEX_B / PHX_FAC_TEX_A + the mask image; texture_node -> luminance_node ->
mix_closure_node.fac): CPU checks of the C ABI, of the closure baker, of the image loaders and of the scene plumbing.  The device is
checked in tests/test_gpu_masks.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_lobe_and_material_keep_their_size_and_the_library_exports_the_hook():
    from phosphorus_mk2_amd import abi, xpu
    lib = C.CDLL(xpu.LIB_PATH)
    lib.phx_abi_sizeof.argtypes = [C.c_int]; lib.phx_abi_sizeof.restype = C.c_uint32
    assert C.sizeof(abi.Lobe) == lib.phx_abi_sizeof(1) == 64
    assert C.sizeof(abi.Material) == lib.phx_abi_sizeof(2) == 544
    assert "phx_dev_lobe_weights" in abi.EXPORTS and hasattr(lib, "phx_dev_lobe_weights")


def test_header_macros_and_enums_as_a_c99_compiler_sees_them(tmp_path):
    from phosphorus_mk2_amd import abi
    cases = [(abi.FAC_TEX_B, 1), (abi.FAC_TEX_A, 7), (abi.FAC_TEX_B, (1 << 24) - 1), (abi.FAC_MIX_A, 0), (abi.FAC_NONE, 0)]
    body = ('  printf("%zu %zu %zu %zu\\n", sizeof(phx_lobe), sizeof(phx_material), offsetof(phx_lobe, fac_mode), offsetof(phx_lobe, fac_ior));\n'
            '  printf("%d %d %d %d %d\\n", PHX_FAC_NONE, PHX_FAC_MIX_B, PHX_FAC_MIX_A, PHX_FAC_TEX_B, PHX_FAC_TEX_A);\n')
    for mode, k in cases:
        body += (f'  {{ uint32_t x = PHX_FAC_PACK({mode}, {k}u); printf("%u %u %u\\n", (unsigned)x, (unsigned)PHX_FAC_MODE(x), (unsigned)PHX_FAC_TEXTURE(x)); }}\n')
    src = tmp_path / "m.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phx_xpu.h"\nint main(void){\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    rows = [[int(x) for x in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert rows[0] == [64, 544, abi.Lobe.fac_mode.offset, abi.Lobe.fac_ior.offset] and rows[0][2:] == [40, 44]
    assert rows[1] == [abi.FAC_NONE, abi.FAC_MIX_B, abi.FAC_MIX_A, abi.FAC_TEX_B, abi.FAC_TEX_A] == [0, 1, 2, 3, 4]
    for (mode, k), row in zip(cases, rows[2:]):
        word = abi.fac_pack(mode, k)
        assert row == [word, mode, k] and (abi.fac_mode(word), abi.fac_texture(word)) == (mode, k)
    assert abi.fac_pack(abi.FAC_MIX_B) == abi.FAC_MIX_B  # a zero mask leaves the modes that existed as they were


def test_pack_puts_the_mask_into_fac_mode_and_lobedesc_stays_positional():
    from phosphorus_mk2_amd import abi, scenes
    # LobeDesc's positional order up to `texture` is what existing callers use; fac_texture comes after it
    l = scenes.LobeDesc(abi.LOBE_DIFFUSE, (1, 1, 1), 0.0, 0.0, 0.0, 0.0, 0, 0.0, abi.FAC_TEX_A, 0.0, (0.5, 0.5, 0.5), 2, 3)
    assert (l.texture, l.fac_texture, l.fac_mode) == (2, 3, abi.FAC_TEX_A)
    sc = scenes.cornell(8, 8)
    sc.textures = [scenes.TextureDesc(np.ones((1, 1, 3), F))] * 3
    sc.materials[0].lobes = [l, scenes.LobeDesc(abi.LOBE_REFLECTION, (1, 1, 1), fac_mode=abi.FAC_TEX_B, fac_texture=3)]
    s, keep = sc.pack()
    a, b = s.materials[0].lobes[0], s.materials[0].lobes[1]
    assert a.fac_mode == abi.fac_pack(abi.FAC_TEX_A, 3) == 4 | 3 << 8 and a.texture == 2 and b.fac_mode == 3 | 3 << 8
    assert all(s.materials[i].lobes[0].fac_mode == 0 for i in range(1, s.num_materials) if s.materials[i].num_lobes)


# ---- closures.py: texture_node -> luminance_node -> mix_closure_node.fac ----------------------------------------------------------------
def _mat(shaders, connect):
    return {"shaders": shaders, "connect": [{"from": {"layer": a, "slot": s}, "to": {"layer": b, "slot": t}} for a, s, b, t in connect]}


def _tex(layer="tex", filename="mask.pgm", **wraps):
    return {"name": "texture_node", "layer": layer,
            "parameters": [{"name": "filename", "type": "string", "value": filename}] + [{"name": k, "type": "string", "value": v} for k, v in wraps.items()]}


LUM = {"name": "luminance_node", "layer": "lum"}
DIFF = {"name": "diffuse_bsdf_node", "layer": "d", "parameters": [{"name": "Cs", "type": "rgb", "value": [0.8, 0.7, 0.6]}]}
GLOSS = {"name": "glossy_bsdf_node", "layer": "g", "parameters": [{"name": "Cs", "type": "rgb", "value": [0.5, 0.4, 0.3]},
                                                                  {"name": "roughness", "type": "float", "value": 0.2}]}
MIX = {"name": "mix_closure_node", "layer": "m"}
MASKED = [("tex", "Cout", "lum", "in"), ("lum", "out", "m", "fac"), ("d", "Cout", "m", "A"), ("g", "Cout", "m", "B")]


def _w(*x):
    return tuple(float(F(v)) for v in x)


def test_masked_mix_bakes_into_tex_modes_pre_weight_and_the_texture_list():
    from phosphorus_mk2_amd import abi, closures as cl
    # the masked mix sits under a constant mix (fac 0.25, B side) with a sheen lobe on the other side
    desc = _mat([_tex(twrap="clamp"), LUM, DIFF, GLOSS, MIX, {"name": "sheen_bsdf_node", "layer": "s"},
                 {"name": "mix_closure_node", "layer": "top", "parameters": [{"name": "fac", "type": "float", "value": 0.25}]}],
                MASKED + [("s", "Cout", "top", "A"), ("m", "Cout", "top", "B")])
    textures = [{"filename": "other.npy", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_PERIODIC}]
    m = cl.bake_material(desc, textures)
    assert [l.type for l in m.lobes] == [abi.LOBE_SHEEN, abi.LOBE_DIFFUSE, abi.LOBE_MICROFACET]
    s, d, g = m.lobes
    assert (s.fac_mode, s.fac_texture, s.weight) == (abi.FAC_NONE, 0, _w(0.75, 0.75, 0.75))
    assert (d.fac_mode, g.fac_mode) == (abi.FAC_TEX_A, abi.FAC_TEX_B) and d.fac_texture == g.fac_texture == 2
    assert d.pre_weight == g.pre_weight == _w(0.25, 0.25, 0.25)  # the constant weights above the mask
    assert d.weight == _w(0.8, 0.7, 0.6) and g.weight == _w(0.5, 0.4, 0.3) and d.texture == g.texture == 0
    assert d.fac_ior == g.fac_ior == 0.0
    assert textures[1] == {"filename": "mask.pgm", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_CLAMP} and len(textures) == 2
    # the same image with the same wraps elsewhere in the scene is one entry; other wraps are another
    m2 = cl.bake_material(_mat([_tex(twrap="clamp"), LUM, DIFF, GLOSS, MIX], MASKED), textures)
    assert len(textures) == 2 and m2.lobes[0].fac_texture == 2 and m2.lobes[0].pre_weight == (1.0, 1.0, 1.0)
    m3 = cl.bake_material(_mat([_tex(), LUM, DIFF, GLOSS, MIX], MASKED), textures)
    assert len(textures) == 3 and m3.lobes[0].fac_texture == m3.lobes[1].fac_texture == 3


def test_colour_texture_below_a_masked_mix_sets_both_indices():
    from phosphorus_mk2_amd import abi, closures as cl
    desc = _mat([_tex(), LUM, _tex("wood", "wood.ppm"), {"name": "diffuse_bsdf_node", "layer": "d"}, GLOSS, MIX],
                MASKED + [("wood", "Cout", "d", "Cs")])
    textures = []
    m = cl.bake_material(desc, textures)
    d, g = m.lobes
    assert [t["filename"] for t in textures] == ["mask.pgm", "wood.ppm"]
    assert (d.fac_mode, d.fac_texture, d.texture, d.weight) == (abi.FAC_TEX_A, 1, 2, (1.0, 1.0, 1.0))
    assert (g.fac_mode, g.fac_texture, g.texture) == (abi.FAC_TEX_B, 1, 0)
    # the mask image used as the colour too: one entry, both indices name it
    m = cl.bake_material(_mat([_tex(), LUM, {"name": "diffuse_bsdf_node", "layer": "d"}, GLOSS, MIX], MASKED + [("tex", "Cout", "d", "Cs")]), textures)
    assert len(textures) == 2 and (m.lobes[0].fac_texture, m.lobes[0].texture) == (1, 1)


def test_transparent_cut_out_and_one_sided_mixes():
    from phosphorus_mk2_amd import abi, closures as cl
    m = cl.bake_material(_mat([_tex(), LUM, {"name": "transparent_bsdf_node", "layer": "d"}, dict(DIFF, layer="g"), MIX], MASKED), [])
    assert [(l.type, l.fac_mode) for l in m.lobes] == [(abi.LOBE_TRANSPARENT, abi.FAC_TEX_A), (abi.LOBE_DIFFUSE, abi.FAC_TEX_B)]
    m = cl.bake_material(_mat([_tex(), LUM, GLOSS, MIX], [("tex", "Cout", "lum", "in"), ("lum", "out", "m", "fac"), ("g", "Cout", "m", "B")]), [])
    assert [(l.type, l.fac_mode) for l in m.lobes] == [(abi.LOBE_MICROFACET, abi.FAC_TEX_B)]


@pytest.mark.parametrize("rgb", [(0.25, 0.5, 0.75), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.9, 0.1, 0.33)])
def test_constant_colour_through_luminance_node_is_the_constant_fac_bake(rgb):
    from phosphorus_mk2_amd import closures as cl
    c = np.array(rgb, F)
    fac = F(F(F(c[0] * F(0.2126)) + F(c[1] * F(0.7152))) + F(c[2] * F(0.0722)))  # fp32, in the order the header states
    lum = dict(LUM, parameters=[{"name": "in", "type": "rgb", "value": list(rgb)}])
    a = cl.bake_material(_mat([lum, DIFF, GLOSS, MIX], MASKED[1:]), [])
    b = cl.bake_material(_mat([DIFF, GLOSS, dict(MIX, parameters=[{"name": "fac", "type": "float", "value": float(fac)}])], MASKED[2:]), [])
    assert a == b and all(l.fac_mode == 0 and l.fac_texture == 0 for l in a.lobes)
    if rgb == (1.0, 1.0, 1.0):
        assert fac == F(1.0) and [l.type for l in a.lobes] == [b.lobes[0].type] and len(a.lobes) == 1  # white: A's side is gone
    if rgb == (0.0, 0.0, 0.0):
        assert fac == F(0.0) and len(a.lobes) == 1


FRES = {"name": "fresnel_dielectric_node", "layer": "fr"}
REFR = {"name": "refraction_bsdf_node", "layer": "r"}
GLASS = [FRES, REFR, dict(GLOSS, layer="gg"), dict(MIX, layer="glass")]
GLASS_EDGES = [("fr", "out", "glass", "fac"), ("r", "Cout", "glass", "A"), ("gg", "Cout", "glass", "B")]


@pytest.mark.parametrize("case", ["mask_under_mask", "mask_over_fresnel", "mask_under_fresnel", "emission_under_mask", "background_under_mask",
                                  "luminance_into_cs", "luminance_into_roughness", "luminance_into_luminance", "environment_into_luminance",
                                  "closure_into_luminance", "fresnel_into_luminance", "texture_into_fac", "luminance_cout"])
def test_what_a_mask_cannot_express_raises(case):
    from phosphorus_mk2_amd import closures as cl
    if case == "mask_under_mask":
        desc = _mat([_tex(), LUM, DIFF, GLOSS, MIX, _tex("tex2", "m2.pgm"), dict(LUM, layer="lum2"), {"name": "sheen_bsdf_node", "layer": "s"}, dict(MIX, layer="top")],
                    MASKED + [("tex2", "Cout", "lum2", "in"), ("lum2", "out", "top", "fac"), ("s", "Cout", "top", "A"), ("m", "Cout", "top", "B")])
    elif case == "mask_over_fresnel":
        desc = _mat([_tex(), LUM, DIFF] + GLASS + [MIX], GLASS_EDGES + [("tex", "Cout", "lum", "in"), ("lum", "out", "m", "fac"), ("d", "Cout", "m", "A"), ("glass", "Cout", "m", "B")])
    elif case == "mask_under_fresnel":
        desc = _mat([_tex(), LUM, DIFF, GLOSS, MIX, FRES, REFR, dict(MIX, layer="glass")],
                    MASKED + [("fr", "out", "glass", "fac"), ("r", "Cout", "glass", "A"), ("m", "Cout", "glass", "B")])
    elif case == "emission_under_mask":
        desc = _mat([_tex(), LUM, DIFF, {"name": "diffuse_emitter_node", "layer": "g"}, MIX], MASKED)
    elif case == "background_under_mask":
        desc = _mat([_tex(), LUM, DIFF, {"name": "background_node", "layer": "g", "parameters": [{"name": "Cs", "type": "rgb", "value": [1, 1, 1]}]}, MIX], MASKED)
    elif case == "luminance_into_cs":
        desc = _mat([_tex(), LUM, DIFF], [("tex", "Cout", "lum", "in"), ("lum", "out", "d", "Cs")])
    elif case == "luminance_into_roughness":
        desc = _mat([_tex(), LUM, DIFF], [("tex", "Cout", "lum", "in"), ("lum", "out", "d", "roughness")])
    elif case == "luminance_into_luminance":
        desc = _mat([_tex(), LUM, dict(LUM, layer="lum2"), DIFF, GLOSS, MIX],
                    [("tex", "Cout", "lum2", "in"), ("lum2", "out", "lum", "in")] + MASKED[1:])
    elif case == "environment_into_luminance":
        desc = _mat([{"name": "environment_node", "layer": "tex", "parameters": [{"name": "filename", "type": "string", "value": "sky.hdr"}]}, LUM, DIFF, GLOSS, MIX], MASKED)
    elif case == "closure_into_luminance":
        desc = _mat([dict(DIFF, layer="tex"), LUM, DIFF, GLOSS, MIX], MASKED)
    elif case == "fresnel_into_luminance":
        desc = _mat([FRES, LUM, DIFF, GLOSS, MIX], [("fr", "out", "lum", "in")] + MASKED[1:])
    elif case == "texture_into_fac":  # a colour into a float: only the path through luminance_node is expressible
        desc = _mat([_tex(), DIFF, GLOSS, MIX], [("tex", "Cout", "m", "fac")] + MASKED[2:])
    else:  # luminance_node has no Cout
        desc = _mat([_tex(), LUM, DIFF, GLOSS, MIX], [MASKED[0], ("lum", "Cout", "m", "fac")] + MASKED[2:])
    with pytest.raises(ValueError):
        cl.bake_material(desc, [])


def test_two_factor_message_names_the_limit():
    from phosphorus_mk2_amd import closures as cl
    desc = _mat([_tex(), LUM, DIFF] + GLASS + [MIX], GLASS_EDGES + [("tex", "Cout", "lum", "in"), ("lum", "out", "m", "fac"), ("d", "Cout", "m", "A"), ("glass", "Cout", "m", "B")])
    with pytest.raises(ValueError, match="two hit-dependent factors on one closure"):
        cl.bake_material(desc, [])


def test_fresnel_and_masked_lobes_side_by_side_in_one_material():
    """different lobes of one material may take different factors: add(glass, masked mix)"""
    from phosphorus_mk2_amd import abi, closures as cl
    desc = _mat([_tex(), LUM, DIFF, GLOSS, MIX] + GLASS + [{"name": "add_node", "layer": "sum"}],
                MASKED + GLASS_EDGES + [("glass", "Cout", "sum", "A"), ("m", "Cout", "sum", "B")])
    m = cl.bake_material(desc, [])
    assert [l.fac_mode for l in m.lobes] == [abi.FAC_MIX_A, abi.FAC_MIX_B, abi.FAC_TEX_A, abi.FAC_TEX_B]
    assert [l.fac_texture for l in m.lobes] == [0, 0, 1, 1] and m.lobes[0].fac_ior == pytest.approx(1.45)


# ---- scenes: resolve_masks, masked_showroom ------------------------------------------------------------------------------------------------
def test_resolve_masks_is_the_devices_order_in_fp32():
    from phosphorus_mk2_amd import abi, scenes
    l = scenes.LobeDesc
    mat = scenes.MaterialDesc([l(abi.LOBE_DIFFUSE, (0.8, 0.7, 0.6), fac_mode=abi.FAC_TEX_A, pre_weight=(0.9, 0.5, 0.3), fac_texture=1),
                               l(abi.LOBE_REFLECTION, (0.3, 0.2, 0.1), fac_mode=abi.FAC_TEX_B, pre_weight=(0.9, 0.5, 0.3), fac_texture=1),
                               l(abi.LOBE_SHEEN, (0.1, 0.1, 0.1), r=0.4)])
    c = np.array([0.3, 0.9, 0.2], F)
    fac = F(F(F(c[0] * F(0.2126)) + F(c[1] * F(0.7152))) + F(c[2] * F(0.0722)))
    assert scenes.mask_luminance(c) == fac
    r = scenes.resolve_masks(mat, lambda k: c)
    assert [x.fac_mode for x in r.lobes] == [0, 0, 0] and [x.fac_texture for x in r.lobes] == [0, 0, 0]
    one_minus = F(F(1) - fac)
    assert r.lobes[0].weight == tuple(float(F(F(F(p) * one_minus) * F(w))) for p, w in zip((0.9, 0.5, 0.3), (0.8, 0.7, 0.6)))
    assert r.lobes[1].weight == tuple(float(F(F(F(p) * fac) * F(w))) for p, w in zip((0.9, 0.5, 0.3), (0.3, 0.2, 0.1)))
    assert r.lobes[2] == mat.lobes[2]
    for v in (0.25, 0.5, 0.75, 0.0, 1.0):  # grey texels come back exactly (what a black-and-white mask relies on)
        assert scenes.mask_luminance((v, v, v)) == F(v)
    white = scenes.resolve_masks(mat, lambda k: np.ones(3, F))
    black = scenes.resolve_masks(mat, lambda k: np.zeros(3, F))
    assert [x.type for x in white.lobes] == [abi.LOBE_REFLECTION, abi.LOBE_SHEEN] and [x.type for x in black.lobes] == [abi.LOBE_DIFFUSE, abi.LOBE_SHEEN]


def test_masked_showroom_modes():
    from phosphorus_mk2_amd import abi, scenes
    img, one, baked = (scenes.masked_showroom(2000, 64, 48, tex_size=8, mode=m) for m in ("image", "one_texel", "baked"))
    masked = [i for i, m in enumerate(img.materials) if any(l.fac_mode == abi.FAC_TEX_A for l in m.lobes)]
    assert len(masked) == len(img.textures) == len(one.textures) == 6 and baked.textures == []
    for i in masked:
        a, b = img.materials[i].lobes
        assert (a.type, a.fac_mode, b.type, b.fac_mode) == (abi.LOBE_DIFFUSE, abi.FAC_TEX_A, abi.LOBE_MICROFACET, abi.FAC_TEX_B)
        assert a.fac_texture == b.fac_texture and img.textures[a.fac_texture - 1].texels.shape == (8, 8, 3)
        t = one.textures[one.materials[i].lobes[0].fac_texture - 1].texels
        assert t.shape == (1, 1, 3)
        assert baked.materials[i] == scenes.resolve_masks(one.materials[i], lambda k: one.textures[k - 1].texels[0, 0])
        assert all(l.fac_mode == abi.FAC_NONE for l in baked.materials[i].lobes) and len(baked.materials[i].lobes) == 2
    assert all(len(m.uvs) in (len(m.vertices), 3 * len(m.faces)) for m in img.meshes) and all(len(m.uvs) == 0 for m in baked.meshes)
    m0 = scenes.procedural_mask(64)
    assert m0.min() == 0.0 and m0.max() == 1.0 and (m0[..., 0] == m0[..., 2]).all()
    with pytest.raises(ValueError):
        scenes.masked_showroom(2000, 64, 48, tex_size=8, mode="other")
    for s in (img, one, baked):
        s.pack()


# ---- sceneio: grey images, a YAML scene with a masked material --------------------------------------------------------------------------------
def test_grey_pgm_and_pfm_images(tmp_path):
    from phosphorus_mk2_amd import sceneio
    rng = np.random.default_rng(2)
    g8 = rng.integers(0, 256, (3, 5), dtype=np.uint8)  # H 3, W 5
    want8 = np.repeat((g8.astype(F) / F(255.0))[:, :, None], 3, axis=2)
    (tmp_path / "a.pgm").write_bytes(b"P5\n# a comment\n5 3\n255\n" + g8.tobytes())
    got = sceneio.load_image(str(tmp_path / "a.pgm"))
    assert got.dtype == F and got.shape == (3, 5, 3) and np.array_equal(got, want8)
    (tmp_path / "b.pgm").write_text("P2\n# plain\n5 3\n255\n" + "\n".join(" ".join(str(v) for v in row) for row in g8) + "\n")
    assert np.array_equal(sceneio.load_image(str(tmp_path / "b.pgm")), want8)
    g16 = rng.integers(0, 65536, (2, 4), dtype=np.uint16)
    (tmp_path / "c.pgm").write_bytes(b"P5 4 2 65535\n" + g16.astype(">u2").tobytes())
    assert np.array_equal(sceneio.load_image(str(tmp_path / "c.pgm")), np.repeat((g16.astype(F) / F(65535.0))[:, :, None], 3, axis=2))
    (tmp_path / "d.pgm").write_text("P2 2 2 4\n0 1\n3 4\n")  # maxval 4: 0, 0.25, 0.75, 1 exactly
    assert np.array_equal(sceneio.load_image(str(tmp_path / "d.pgm"))[..., 1], np.array([[0, 0.25], [0.75, 1]], F))
    top_first = rng.uniform(-1, 2, (3, 5)).astype(F)  # PFM stores the bottom row first
    (tmp_path / "e.pfm").write_bytes(b"Pf\n5 3\n-1.0\n" + np.ascontiguousarray(top_first[::-1]).astype("<f4").tobytes())
    got = sceneio.load_image(str(tmp_path / "e.pfm"))
    assert got.shape == (3, 5, 3) and all(np.array_equal(got[..., c], top_first) for c in range(3))
    (tmp_path / "f.pfm").write_bytes(b"Pf\n5 3\n1.0\n" + np.ascontiguousarray(top_first[::-1]).astype(">f4").tobytes())
    assert np.array_equal(sceneio.load_image(str(tmp_path / "f.pfm")), got)
    (tmp_path / "g.pgm").write_bytes(b"P6\n1 1\n255\n\0\0\0")  # a PPM under a PGM's name
    with pytest.raises(ValueError):
        sceneio.load_image(str(tmp_path / "g.pgm"))
    (tmp_path / "h.pgm").write_bytes(b"P5\n4 4\n255\n\0\0\0")  # a short raster
    with pytest.raises(ValueError):
        sceneio.load_image(str(tmp_path / "h.pgm"))


def test_yaml_scene_with_a_masked_material(tmp_path):
    import yaml
    from phosphorus_mk2_amd import abi, sceneio
    (tmp_path / "rust.pgm").write_bytes(b"P5 2 1 255\n" + bytes([255, 0]))
    (tmp_path / "m.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nusemtl paint\nf 1/1 2/2 3/3 4/4\n"
                                    "v 0 2 0\nv 1 2 0\nv 1 2 1\nusemtl lamp\nf 5 6 7\n")
    cfg = {"materials": {"paint": _mat([_tex(filename="rust.pgm", swrap="clamp"), LUM, DIFF, GLOSS, MIX], MASKED),
                         "lamp": {"shaders": [{"name": "diffuse_emitter_node", "layer": "e"}]}},
           "data": [{"path": "m.obj"}], "camera": {"film": {"width": 8, "height": 8}}}
    (tmp_path / "scene.yaml").write_text(yaml.safe_dump(cfg, sort_keys=False))
    sc = sceneio.load_scene(str(tmp_path / "scene.yaml"))
    assert len(sc.textures) == 1 and (sc.textures[0].swrap, sc.textures[0].twrap) == (abi.WRAP_CLAMP, abi.WRAP_PERIODIC)
    assert np.array_equal(sc.textures[0].texels, np.array([[[1, 1, 1], [0, 0, 0]]], F))
    d, g = sc.materials[0].lobes
    assert (d.fac_mode, d.fac_texture, g.fac_mode, g.fac_texture) == (abi.FAC_TEX_A, 1, abi.FAC_TEX_B, 1)
    s, keep = sc.pack()
    assert s.num_textures == 1 and s.materials[0].lobes[0].fac_mode == abi.fac_pack(abi.FAC_TEX_A, 1) and s.meshes[0].num_uvs > 0
