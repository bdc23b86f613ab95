"""Environment maps (phx_material.emission_texture / emission_mapping, environment_node, Radiance .hdr): CPU checks of the C ABI's layout
and of the scene plumbing.  The device is checked in tests/test_gpu_environment.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def lib():
    from phosphorus_mk2_amd import xpu
    lib = C.CDLL(xpu.LIB_PATH)
    lib.phx_abi_sizeof.argtypes = [C.c_int]; lib.phx_abi_sizeof.restype = C.c_uint32
    return lib


def test_material_keeps_its_size(lib):
    from phosphorus_mk2_amd import abi
    assert C.sizeof(abi.Material) == lib.phx_abi_sizeof(2) == 20 + 12 + 8 * 64  # two words of `pad` became fields
    assert hasattr(lib, "phx_dev_environment_lookup")
    assert (abi.ENV_LATLONG_Y_UP, abi.ENV_LATLONG_Z_UP) == (0, 1)


def test_material_field_offsets_match_the_header(tmp_path):
    from phosphorus_mk2_amd import abi
    fields = [f for f, _ in abi.Material._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(phx_material, {f}));\n' for f in fields)
    body += '  printf("%d %d\\n", (int)PHX_ENV_LATLONG_Y_UP, (int)PHX_ENV_LATLONG_Z_UP);\n  printf("%zu\\n", sizeof(phx_material));\n'
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "phx_xpu.h"\nint main(void){\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:len(fields)] == [getattr(abi.Material, f).offset for f in fields]
    assert got[len(fields):] == [abi.ENV_LATLONG_Y_UP, abi.ENV_LATLONG_Z_UP, C.sizeof(abi.Material)]
    assert abi.Material.emission_texture.offset == 20 and abi.Material.emission_mapping.offset == 24


def test_pack_carries_the_environment_fields():
    from phosphorus_mk2_amd import abi, scenes
    sc = scenes.cornell(8, 8)
    sc.textures = [scenes.TextureDesc(np.ones((2, 4, 3), F), abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)]
    sc.materials.append(scenes.MaterialDesc([], (0.5, 0.25, 2.0), emission_texture=1, emission_mapping=abi.ENV_LATLONG_Z_UP))
    sc.environment_material = len(sc.materials) - 1
    s, keep = sc.pack()
    m = s.materials[sc.environment_material]
    assert (m.emission_texture, m.emission_mapping) == (1, abi.ENV_LATLONG_Z_UP) and list(m.emission) == [0.5, 0.25, 2.0]
    assert all((s.materials[i].emission_texture, s.materials[i].emission_mapping) == (0, 0) for i in range(s.num_materials - 1))
    d = scenes.MaterialDesc()
    assert (d.emission_texture, d.emission_mapping) == (0, abi.ENV_LATLONG_Y_UP)


# ---- the baker -----------------------------------------------------------------------------------------------------------------------
def _sh(name, layer, **params):
    ps = []
    for k, v in params.items():
        if isinstance(v, str):
            ps.append({"name": k, "type": "string", "value": v})
        elif isinstance(v, (tuple, list)):
            ps.append({"name": k, "type": "rgb", "value": list(v)})
        else:
            ps.append({"name": k, "type": "float", "value": v})
    return {"name": name, "layer": layer, "parameters": ps}


def _edge(a, sa, b, sb):
    return {"from": {"layer": a, "slot": sa}, "to": {"layer": b, "slot": sb}}


def test_environment_node_bakes_into_the_background():
    from phosphorus_mk2_amd import abi, closures
    tex = []
    m = closures.bake_material({"shaders": [_sh("environment_node", "env", filename="sky.hdr"), _sh("background_node", "bg", power=2.5)],
                                "connect": [_edge("env", "Cout", "bg", "Cs")]}, tex)
    assert m.lobes == [] and not m.is_emitter
    assert m.emission == (2.5, 2.5, 2.5) and m.emission_texture == 1
    assert tex == [{"filename": "sky.hdr", "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_CLAMP}]
    # under a constant mix with another background: the mix weight joins `power`; the last emission assigned wins (material.cpp)
    tex = [{"filename": "other.ppm", "swrap": abi.WRAP_CLAMP, "twrap": abi.WRAP_CLAMP}]
    m = closures.bake_material({"shaders": [_sh("background_node", "plain", Cs=(1.0, 0.0, 0.0)), _sh("environment_node", "env", filename="sky.hdr"),
                                            _sh("background_node", "bg", power=4.0), _sh("mix_closure_node", "mix", fac=0.25)],
                                "connect": [_edge("env", "Cout", "bg", "Cs"), _edge("plain", "Cout", "mix", "A"), _edge("bg", "Cout", "mix", "B")]}, tex)
    assert m.emission == tuple(float(x) for x in np.array([1.0, 1.0, 1.0], F) * (F(4.0) * F(0.25))) and m.emission_texture == 2
    assert len(tex) == 2 and tex[1]["filename"] == "sky.hdr"
    # the environment visited first, the plain background last: the plain one overwrites it and carries no image
    m = closures.bake_material({"shaders": [_sh("environment_node", "env", filename="sky.hdr"), _sh("background_node", "bg"),
                                            _sh("background_node", "plain", Cs=(0.5, 0.5, 0.5)), _sh("add_node", "add")],
                                "connect": [_edge("env", "Cout", "bg", "Cs"), _edge("bg", "Cout", "add", "A"), _edge("plain", "Cout", "add", "B")]}, [])
    assert m.emission == (0.5, 0.5, 0.5) and m.emission_texture == 0


@pytest.mark.parametrize("case", ["sblur", "tblur", "into_diffuse", "into_emitter", "into_mix_fac", "texture_into_background", "no_file", "unknown_input"])
def test_bad_environment_graphs_raise(case):
    from phosphorus_mk2_amd import closures
    env = {"sblur": _sh("environment_node", "env", filename="a.hdr", sblur=0.1),
           "tblur": _sh("environment_node", "env", filename="a.hdr", tblur=0.2),
           "no_file": _sh("environment_node", "env"),
           "unknown_input": _sh("environment_node", "env", filename="a.hdr", width=2.0)}.get(case, _sh("environment_node", "env", filename="a.hdr"))
    graphs = {
        "into_diffuse": ([env, _sh("diffuse_bsdf_node", "d")], [_edge("env", "Cout", "d", "Cs")]),
        "into_emitter": ([env, _sh("diffuse_emitter_node", "e")], [_edge("env", "Cout", "e", "Cs")]),
        "into_mix_fac": ([env, _sh("background_node", "a"), _sh("background_node", "b"), _sh("mix_closure_node", "m")],
                         [_edge("env", "Cout", "m", "fac"), _edge("a", "Cout", "m", "A"), _edge("b", "Cout", "m", "B")]),
        "texture_into_background": ([_sh("texture_node", "t", filename="a.ppm"), _sh("background_node", "bg")], [_edge("t", "Cout", "bg", "Cs")]),
    }
    shaders, connect = graphs.get(case, ([env, _sh("background_node", "bg")], [_edge("env", "Cout", "bg", "Cs")]))
    with pytest.raises(ValueError):
        closures.bake_material({"shaders": shaders, "connect": connect}, [])


# ---- Radiance .hdr ---------------------------------------------------------------------------------------------------------------------
def _colr_color(rgbe):
    """Radiance's colr_color: (m + 0.5) * 2^(e - 136), e == 0 -> 0"""
    rgbe = np.asarray(rgbe, np.int64)
    e = rgbe[..., 3]
    f = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    return ((rgbe[..., :3] + 0.5) * f[..., None]).astype(F)


def _rle_component(vals):
    """new-style run-length encoding of one component of a scanline: runs of >= 3 equal bytes, literals between"""
    out, i, n = bytearray(), 0, len(vals)
    while i < n:
        j = i
        while j < n and vals[j] == vals[i] and j - i < 127:
            j += 1
        if j - i >= 3:
            out += bytes([128 + j - i, vals[i]]); i = j
            continue
        k = i
        while k < n and k - i < 128 and not (k + 2 < n and vals[k] == vals[k + 1] == vals[k + 2]):
            k += 1
        out += bytes([k - i]) + bytes(vals[i:k]); i = k
    return bytes(out)


def _write_hdr(path, rgbe, rle, magic=b"#?RADIANCE", fmt=b"32-bit_rle_rgbe", res=None):
    H, W = rgbe.shape[:2]
    head = magic + b"\n# written by the test\nFORMAT=" + fmt + b"\nEXPOSURE=1.0\n\n" + (res or b"-Y %d +X %d" % (H, W)) + b"\n"
    body = bytearray()
    for y in range(H):
        if rle:
            body += bytes([2, 2, W >> 8, W & 0xff])
            for c in range(4):
                body += _rle_component(rgbe[y, :, c].tolist())
        else:
            body += rgbe[y].astype(np.uint8).tobytes()
    path.write_bytes(head + bytes(body))


def _random_rgbe(H, W, seed):
    rng = np.random.default_rng(seed)
    rgbe = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    rgbe[..., 3] = rng.integers(100, 160, (H, W))
    rgbe[0, :5] = (200, 100, 50, 130)    # a run in every component
    rgbe[-1, -3:] = (7, 9, 11, 0)        # e == 0: black
    rgbe[..., :3][(rgbe[..., :3] == 1).all(-1)] = 2  # no accidental old-style run marker in the flat files
    return rgbe


@pytest.mark.parametrize("rle,H,W", [(False, 3, 5), (True, 4, 37), (True, 2, 300), (False, 6, 8)])
def test_hdr_reader_decodes_flat_and_rle_scanlines(tmp_path, rle, H, W):
    from phosphorus_mk2_amd import sceneio
    rgbe = _random_rgbe(H, W, H * W)
    p = tmp_path / "img.hdr"
    _write_hdr(p, rgbe, rle)
    img = sceneio.load_hdr(str(p))
    assert img.shape == (H, W, 3) and img.dtype == F
    want = _colr_color(rgbe)
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert (img[-1, -1] == 0).all() and img[0, 0, 0] == F((200 + 0.5) * 2.0 ** (130 - 136))  # row 0 of the file is row 0 of the image
    assert np.array_equal(sceneio.load_image(str(p)), img)


def test_hdr_reader_accepts_rgbe_magic(tmp_path):
    from phosphorus_mk2_amd import sceneio
    rgbe = _random_rgbe(2, 9, 3)
    p = tmp_path / "a.hdr"
    _write_hdr(p, rgbe, True, magic=b"#?RGBE")
    assert np.array_equal(sceneio.load_hdr(str(p)), _colr_color(rgbe))


@pytest.mark.parametrize("bad", ["magic", "format", "flipped", "sideways", "truncated", "old_rle"])
def test_hdr_reader_refuses_what_it_cannot_read(tmp_path, bad):
    from phosphorus_mk2_amd import sceneio
    rgbe = _random_rgbe(3, 10, 1)
    p = tmp_path / "bad.hdr"
    if bad == "magic":
        _write_hdr(p, rgbe, False, magic=b"#?PFM")
    elif bad == "format":
        _write_hdr(p, rgbe, False, fmt=b"32-bit_rle_xyze")
    elif bad == "flipped":
        _write_hdr(p, rgbe, False, res=b"+Y 3 +X 10")
    elif bad == "sideways":
        _write_hdr(p, rgbe, False, res=b"+X 10 -Y 3")
    elif bad == "truncated":
        _write_hdr(p, rgbe, True)
        p.write_bytes(p.read_bytes()[:-7])
    else:
        rgbe[1, 4] = (1, 1, 1, 3)
        _write_hdr(p, rgbe, False)
    with pytest.raises(ValueError):
        sceneio.load_hdr(str(p))


# ---- YAML --------------------------------------------------------------------------------------------------------------------------------
def _yaml_scene(tmp_path, up=None):
    from phosphorus_mk2_amd import sceneio
    rgbe = _random_rgbe(4, 16, 7)
    _write_hdr(tmp_path / "sky.hdr", rgbe, True)
    (tmp_path / "box.obj").write_text("v -1 -1 -3\nv 1 -1 -3\nv 1 1 -3\nv -1 1 -3\nusemtl grey\nf 1 2 3 4\n"
                                      "v -0.2 0.9 -2\nv 0.2 0.9 -2\nv 0.2 0.9 -2.4\nusemtl lamp\nf 5 6 7\n")
    world = "world:\n  environment: sky\n" + (f"  environment-up: {up}\n" if up else "")
    (tmp_path / "s.yaml").write_text(
        "materials:\n"
        "  grey:\n    shaders:\n      - {name: diffuse_bsdf_node, layer: d, parameters: [{name: Cs, type: rgb, value: [0.5, 0.5, 0.5]}]}\n"
        "  lamp:\n    shaders:\n      - {name: diffuse_emitter_node, layer: e, parameters: [{name: power, type: float, value: 3.0}]}\n"
        "  sky:\n    shaders:\n      - {name: environment_node, layer: env, parameters: [{name: filename, type: string, value: sky.hdr}]}\n"
        "      - {name: background_node, layer: bg, parameters: [{name: power, type: float, value: 0.5}]}\n"
        "    connect:\n      - {from: {layer: env, slot: Cout}, to: {layer: bg, slot: Cs}}\n"
        "data:\n  - {path: box.obj}\n" + world)
    return sceneio.load_scene(str(tmp_path / "s.yaml"), 16, 16), _colr_color(rgbe)


@pytest.mark.parametrize("up", [None, "y", "z"])
def test_yaml_world_with_an_environment_image_loads(tmp_path, up):
    from phosphorus_mk2_amd import abi
    sc, img = _yaml_scene(tmp_path, up)
    env = sc.materials[sc.environment_material]
    assert sc.environment_material == 2 and env.emission == (0.5, 0.5, 0.5) and env.emission_texture == 1
    assert env.emission_mapping == (abi.ENV_LATLONG_Z_UP if up == "z" else abi.ENV_LATLONG_Y_UP)
    t = sc.textures[0]
    assert (t.filter, t.swrap, t.twrap) == (abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)
    assert np.array_equal(t.texels, img)
    s, keep = sc.pack()
    assert s.materials[2].emission_texture == 1 and s.materials[2].emission_mapping == env.emission_mapping and s.num_textures == 1


def test_yaml_world_refuses_an_unknown_up_axis(tmp_path):
    with pytest.raises(ValueError):
        _yaml_scene(tmp_path, "x")


def test_environment_scenes():
    from phosphorus_mk2_amd import abi, scenes
    sky = scenes.procedural_sky(512, 256)
    assert sky.shape == (256, 512, 3) and sky.dtype == F and np.isfinite(sky).all() and sky.min() > 0
    assert sky.max() > 100 * np.median(sky)  # the sun
    img = scenes.environment_showroom(2000, 32, 24, (64, 32))
    mean = scenes.environment_showroom(2000, 32, 24, (64, 32), mode="mean")
    const = scenes.environment_showroom(2000, 32, 24, (64, 32), mode="constant")
    e = img.materials[img.environment_material]
    assert e.emission_texture == 1 and img.textures[0].texels.shape == (32, 64, 3) and img.textures[0].twrap == abi.WRAP_CLAMP
    assert mean.textures[0].texels.shape == (1, 1, 3)
    c = const.materials[const.environment_material]
    assert c.emission_texture == 0 and not const.textures
    assert np.array_equal(np.array(c.emission, F), mean.textures[0].texels.reshape(3))
