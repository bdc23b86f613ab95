"""Closure-recipe baker: turns a material's shader graph — the BSDF node shaders of the reference with
constant inputs — into the flat closure list (`scenes.MaterialDesc` -> `phx_material`) the device consumes.

This is the offline stand-in for what happens per hit in the reference: OSL executes the material's shader
group and `material_t::details_t::eval_closure` (src/material.cpp:218-305) flattens the resulting closure
tree (MUL multiplies the colour weight down the tree, ADD visits A then B, `emission`/`background` assign
`result.e`, every other component becomes one `bsdf_t` lobe with weight = accumulated weight x component
weight).  With constant node inputs that tree does not depend on the hit, so it can be baked once.

Node semantics follow the shader sources (file:line = reference src/shaders/):
  diffuse_bsdf_node.osl:20-25       roughness == 0 -> Cs * diffuse(N) else Cs * oren_nayar(N, roughness)
  glossy_bsdf_node.osl:26-34        "sharp" or roughness == 0 -> Cs * reflection(N, 0)
                                    else Cs * microfacet(dist, N, 0, r*r, r*r, 0, 0)
  refraction_bsdf_node.osl:30-39    eta = IoR; sharp -> Cs * refraction(N, eta) else Cs * microfacet(dist, N, 0, r, r, eta, 1)
  sheen_bsdf_node.osl:20            Cs * sheen(N, roughness)
  transparent_bsdf.node.osl:14      Cs * transparent()
  diffuse_emitter_node.osl:18       (power / M_PI) * Cs * emission()
  background_node.osl:14            Cs * power * background()
  mix_closure_node.osl:20           A * (1 - fac) + B * fac
  add_node.osl:16                   A + B
The material description accepted by `bake_material` is the reference's YAML material schema
(src/codecs/scene/material.hpp:44-96): `shaders: [{name, layer, parameters: [{name, type, value}]}]`,
`connect: [{from: {slot, layer}, to: {slot, layer}}]`; the LAST layer is the group's root (OSL convention).
  fresnel_dielectric_node.osl:16-20 out = fresnel_dielectric(dot(I, N), backfacing ? 1/max(1e-5, IoR) : max(1e-5, IoR))
All arithmetic is fp32, as in OSL.  Closures multiplied by an all-zero weight are dropped (OSL returns a null
closure for `closure * 0`).  ONE hit-dependent input is supported, the one the reference's own Blender exporter produces:
`fresnel_dielectric_node.out` driving `mix_closure_node.fac` (Blender's glass node = mix(refraction, glossy, fresnel),
plugins/blender/blender/shader.hpp:306-335).  It cannot be baked into a number, so the recipe records it: the closures under
that mix carry `fac_mode` / `fac_ior` / `pre_weight` and the device (bsdf.h: material_at_hit) and the oracle evaluate the factor
at every hit.  The second one is an image texture on a closure's colour: `texture_node.Cout` driving the `Cs` of a BSDF node
(what the exporter emits for every Image Texture node, plugins/blender/blender/shader.hpp:363-410).
  texture_node.osl                  Cout = texture(filename, u, v, "swrap", swrap, "twrap", twrap)
The closure's lobe records the constant weight accumulated ABOVE that point in `weight` and the image in `texture` (k + 1 for
entry k of the `textures` list handed to the baker: {filename, swrap, twrap}); the device multiplies the texel in at every hit.
`swrap` / `twrap` "periodic" (the default), "clamp" and "black" are expressible; "mirror" and "default" raise, and so do blur
and explicit s / t inputs (the lookup is at the mesh's UV).  A texture feeding anything but a BSDF node's Cs (a mix's fac, a
roughness, emission, another texture) raises.  The third is an environment map: `environment_node.Cout` driving `background_node.Cs`
(the exporter's Environment Texture node on the world, plugins/blender/blender/shader.hpp:376-377, 440).
  environment_node.osl              Cout = environment(filename, I, "sblur", sblur, "tblur", tblur)
It bakes into the material's `emission` (the constant weight accumulated above it, `power` included) and `emission_texture` (k + 1
for the spec {filename, swrap periodic, twrap clamp}: OpenImageIO's lat-long wrap); the device multiplies the texel at the ray's
direction in on a miss.  Blur, an environment_node anywhere but a background's Cs and a texture_node into a background (a miss has
no UV) raise.  The fourth is an image mask on a mix: `texture_node.Cout -> luminance_node.in`, `luminance_node.out -> mix_closure_node.fac`
(luminance_node is the node set's only colour -> float node, so the only way an image reaches a float input).
  luminance_node.osl                out = in[0] * 0.2126 + in[1] * 0.7152 + in[2] * 0.0722
The closures under that mix carry `fac_mode` FAC_TEX_A (A's side, 1 - fac) / FAC_TEX_B (B's side, fac), `fac_texture` (k + 1 in the
`textures` list, with the texture node's wrap modes) and `pre_weight`, like the Fresnel mix; the device looks the mask up at every hit.
A constant colour into luminance_node folds to a constant fac.  One closure takes ONE hit-dependent factor: a mask under a mask, a
mask over or under a Fresnel mix, emission or background under a masked mix raise, and so does luminance_node.out into anything but a
mix's fac or an environment_node into luminance_node.  A colour texture on a closure's Cs under a masked mix is fine (both indices on one
lobe).  Other hit-dependent inputs (noise, normal maps) raise.
"""
import math

import numpy as np

from . import abi
from .scenes import LobeDesc, MaterialDesc

f32 = np.float32
M_PI = f32(math.pi)  # OSL's M_PI is a float


def _color(v):
    if isinstance(v, dict):  # YAML {type: rgb, value: [r,g,b]}
        v = v["value"]
    if np.isscalar(v):
        return np.array([v, v, v], f32)
    a = np.asarray(v, f32)
    assert a.shape == (3,)
    return a


class Comp:
    """a closure component: id = bsdf_t::type_t (src/bsdf.hpp:14-24) + its parameter struct (src/bsdf/params.hpp)"""
    def __init__(self, cid, **params):
        self.cid, self.params = cid, params


class Mul:
    def __init__(self, weight, closure):
        self.weight, self.closure = _color(weight), closure


class Fac:
    """the output of a fresnel_dielectric_node: a float known only at the hit"""
    def __init__(self, ior):
        self.ior = f32(ior)


class Lum:
    """the output of a luminance_node driven by a texture_node: a float known only at the hit (the luminance of the image at the hit's UV)"""
    def __init__(self, tex):
        self.tex = tex


class MulFac:
    """closure * fac (mode FAC_MIX_B / FAC_TEX_B) or closure * (1 - fac) (mode FAC_MIX_A / FAC_TEX_A) with fac a Fac / a Lum"""
    def __init__(self, mode, fac, closure):
        self.mode, self.fac, self.closure = mode, fac, closure


class Add:
    def __init__(self, a, b):
        self.a, self.b = a, b


class Tex:
    """the output of a texture_node: a colour known only at the hit (the image at the hit's UV)"""
    def __init__(self, spec):
        self.spec = spec  # {"filename", "swrap", "twrap"}: abi.WRAP_* values


class MulTex:
    """closure * texel: the image multiplies the closure's colour weight at every hit"""
    def __init__(self, tex, closure):
        self.tex, self.closure = tex, closure


class Env:
    """the output of an environment_node: a colour known only on a miss (the image in the ray's direction)"""
    def __init__(self, spec):
        self.spec = spec  # {"filename", "swrap", "twrap"}: periodic / clamp


class MulEnv:
    """background closure * environment texel: the image multiplies the environment's emission on every miss"""
    def __init__(self, env, closure):
        self.env, self.closure = env, closure


def mul(weight, closure):
    if isinstance(weight, Env):
        raise ValueError("an environment_node can drive only the Cs of a background_node")
    if isinstance(weight, Tex):
        return None if closure is None else MulTex(weight, closure)
    w = _color(weight)
    if closure is None or not w.any():
        return None  # OSL: closure * 0 is the null closure
    return Mul(w, closure)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    return Add(a, b)


# ---- the node shaders ----------------------------------------------------------------------------------
def diffuse_bsdf_node(Cs=1.0, roughness=0.0, **_):
    r = f32(roughness)
    return mul(Cs, Comp(abi.LOBE_DIFFUSE) if r == 0 else Comp(abi.LOBE_OREN_NAYAR, alpha=r))


def glossy_bsdf_node(distribution="ggx", Cs=1.0, roughness=0.0, **_):
    r = f32(roughness)
    r2 = f32(r * r)
    if distribution == "sharp" or r == 0:
        return mul(Cs, Comp(abi.LOBE_REFLECTION, eta=f32(0)))
    return mul(Cs, Comp(abi.LOBE_MICROFACET, distribution=distribution, xalpha=r2, yalpha=r2, eta=f32(0), refract=0))


def refraction_bsdf_node(distribution="ggx", Cs=1.0, IoR=0.5, roughness=0.0, **_):
    r = f32(roughness)
    eta = f32(IoR)  # "backfacing() ? 1/f : f" is commented out in the shader
    if distribution == "sharp" or r == 0:
        return mul(Cs, Comp(abi.LOBE_REFRACTION, eta=eta))
    return mul(Cs, Comp(abi.LOBE_MICROFACET, distribution=distribution, xalpha=r, yalpha=r, eta=eta, refract=1))


def sheen_bsdf_node(Cs=1.0, roughness=0.0, **_):
    return mul(Cs, Comp(abi.LOBE_SHEEN, r=f32(roughness)))


def transparent_bsdf_node(Cs=1.0, **_):
    return mul(Cs, Comp(abi.LOBE_TRANSPARENT))


def diffuse_emitter_node(power=1.0, Cs=1.0, **_):
    if isinstance(Cs, Tex):  # (power / M_PI) * Cs * emission() with Cs the texel: power / M_PI joins the constant weight, the image multiplies at mesh UVs
        return MulTex(Cs, mul(f32(f32(power) / M_PI), Comp(abi.LOBE_EMISSIVE)))
    return mul(f32(f32(power) / M_PI) * _color(Cs), Comp(abi.LOBE_EMISSIVE))


def background_node(Cs=0.0, power=1.0, **_):
    if isinstance(Cs, Env):  # Cs * power * background() with Cs the texel: power joins the constant weight, the image multiplies on a miss
        c = mul(f32(power), Comp(abi.LOBE_BACKGROUND))
        return None if c is None else MulEnv(Cs, c)
    if isinstance(Cs, Tex):
        raise ValueError("texture_node into a background_node: a miss has no UV (use an environment_node)")
    return mul(_color(Cs) * f32(power), Comp(abi.LOBE_BACKGROUND))


def fresnel_dielectric_node(IoR=1.45, **_):
    return Fac(IoR)


def luminance_node(**inputs):
    """out = in[0] * 0.2126 + in[1] * 0.7152 + in[2] * 0.0722 in fp32, in this order (`in` is no Python identifier: it arrives by name)"""
    c = inputs.pop("in", 0.0)
    if isinstance(c, Env):
        raise ValueError("an environment_node can drive only the Cs of a background_node")
    if isinstance(c, Tex):
        return Lum(c)
    if inputs or not (np.isscalar(c) or isinstance(c, (dict, list, tuple, np.ndarray))):
        raise ValueError("luminance_node: its input `in` takes a constant colour or a texture_node")
    c = _color(c)
    return f32(f32(f32(c[0] * f32(0.2126)) + f32(c[1] * f32(0.7152))) + f32(c[2] * f32(0.0722)))


WRAPS = {"periodic": abi.WRAP_PERIODIC, "clamp": abi.WRAP_CLAMP, "black": abi.WRAP_BLACK}


def texture_node(filename="", swrap="periodic", twrap="periodic", sblur=0.0, tblur=0.0, **extra):
    if extra:
        raise ValueError(f"texture_node: inputs {sorted(extra)} cannot be expressed (the lookup is at the mesh's UV)")
    if f32(sblur) != 0 or f32(tblur) != 0:
        raise ValueError("texture_node: sblur / tblur are not supported")
    for name, w in (("swrap", swrap), ("twrap", twrap)):
        if w not in WRAPS:
            raise ValueError(f"texture_node: {name} {w!r} is not supported (periodic, clamp, black)")
    if not filename:
        raise ValueError("texture_node without a filename")
    return Tex({"filename": str(filename), "swrap": WRAPS[swrap], "twrap": WRAPS[twrap]})


def environment_node(filename="", sblur=0.0, tblur=0.0, **extra):
    if extra:
        raise ValueError(f"environment_node: inputs {sorted(extra)} cannot be expressed (the lookup is in the ray's direction)")
    if f32(sblur) != 0 or f32(tblur) != 0:
        raise ValueError("environment_node: sblur / tblur are not supported")
    if not filename:
        raise ValueError("environment_node without a filename")
    return Env({"filename": str(filename), "swrap": abi.WRAP_PERIODIC, "twrap": abi.WRAP_CLAMP})


def mix_closure_node(A=None, B=None, fac=0.5, **_):
    if isinstance(fac, Fac):  # Cout = A * (1 - fac) + B * fac with fac evaluated per hit
        return add(MulFac(abi.FAC_MIX_A, fac, A) if A is not None else None, MulFac(abi.FAC_MIX_B, fac, B) if B is not None else None)
    if isinstance(fac, Lum):  # the same mix with fac the luminance of an image at the hit
        return add(MulFac(abi.FAC_TEX_A, fac, A) if A is not None else None, MulFac(abi.FAC_TEX_B, fac, B) if B is not None else None)
    if not np.isscalar(fac) or isinstance(fac, (Tex, Env)):
        raise ValueError("mix_closure_node.fac is driven by a node this baker cannot express (hit-dependent)")
    fac = f32(fac)
    return add(mul(f32(f32(1) - fac), A), mul(fac, B))


def add_node(A=None, B=None, **_):
    return add(A, B)


NODES = {f.__name__: f for f in (diffuse_bsdf_node, glossy_bsdf_node, refraction_bsdf_node, sheen_bsdf_node, transparent_bsdf_node,
                                 diffuse_emitter_node, background_node, mix_closure_node, add_node, fresnel_dielectric_node, texture_node,
                                 environment_node, luminance_node)}
# the nodes whose Cs a texture may drive: their closure's weight is Cs
TEXTURABLE = {diffuse_bsdf_node, glossy_bsdf_node, refraction_bsdf_node, sheen_bsdf_node, transparent_bsdf_node}
UNBAKEABLE = {"fresnel_node", "normal_map_node", "random_noise_2d_node", "random_noise_3d_node",
              "musgrave_noise_3d_node", "mix_color_node", "blackbody_node"}


# ---- material.cpp:218-305 -------------------------------------------------------------------------------
def flatten(tree, textures=None, emitter_textures=False):
    """eval_closure: closure tree -> MaterialDesc (lobes in visiting order, e = last emission/background weight).  The tree is
    walked as material.cpp:218-305 walks it: MUL multiplies the weight down, ADD visits A then B.  A Fresnel-driven factor
    splits a closure's weight into the constant part above it (pre_weight), the factor itself (fac_mode, fac_ior) and the
    constant part below it (weight): at a hit the weight is (pre_weight * term) * weight, the same order of multiplications.
    A texture on a closure's colour: the lobe keeps the weight accumulated above it and `texture` = k + 1, k the texture's entry in
    `textures` (a list of {filename, swrap, twrap}, extended here by the ones not in it yet).  An image mask is a factor like the Fresnel
    one with the image in place of the ior: fac_mode FAC_TEX_*, `fac_texture` = k + 1 in the same list.  A texture on an emission closure's
    colour is baked only with `emitter_textures`: emission = the constant weight accumulated above it and `emission_uv_texture` = k + 1."""
    lobes, state = [], {"e": (0.0, 0.0, 0.0), "emitter": False, "env": 0, "emit_tex": 0}
    if textures is None:
        textures = []

    def texture_id(spec):
        if spec not in textures:
            textures.append(spec)
        return textures.index(spec) + 1

    def visit(c, w, fac=None, tex=0, env=0):
        # w: the constant weight accumulated so far BELOW the hit-dependent factor (or all of it when there is none);
        # fac = (mode, ior, pre, mask): the factor met on the way down (its ior, or its mask image k + 1) and the constant weight accumulated ABOVE it
        if c is None:
            return
        if isinstance(c, Mul):
            visit(c.closure, (w * c.weight).astype(f32), fac, tex, env)
        elif isinstance(c, MulEnv):
            visit(c.closure, w, fac, tex, texture_id(c.env.spec))
        elif isinstance(c, MulTex):
            if tex:
                raise ValueError("a texture behind another texture on one closure is not supported")
            visit(c.closure, w, fac, texture_id(c.tex.spec))
        elif isinstance(c, MulFac):
            masked = isinstance(c.fac, Lum)
            if fac is not None:
                if masked or fac[3]:
                    raise ValueError("an image-masked mix and another hit-dependent mix (a mask or a Fresnel factor) on one closure: "
                                     "two hit-dependent factors on one closure are not supported")
                raise ValueError("a Fresnel-driven mix below another one: two hit-dependent factors on one closure are not supported")
            if tex:
                raise ValueError("a Fresnel-driven mix below a texture is not supported")
            if masked:
                visit(c.closure, np.ones(3, f32), (c.mode, f32(0), w, texture_id(c.fac.tex.spec)))
            else:
                visit(c.closure, np.ones(3, f32), (c.mode, c.fac.ior, w, 0))
        elif isinstance(c, Add):
            visit(c.a, w, fac, tex, env)
            visit(c.b, w, fac, tex, env)
        else:
            if c.cid in (abi.LOBE_EMISSIVE, abi.LOBE_BACKGROUND):
                if fac is not None:
                    raise ValueError("emission under an image-masked mix is not supported" if fac[3] else "emission under a Fresnel-driven mix is not supported")
                if tex and (not emitter_textures or c.cid != abi.LOBE_EMISSIVE):
                    raise ValueError("textured emission is baked only on request: bake_material(..., emitter_textures=True) / load_scene(..., emitter_textures=True)")
                state["e"] = tuple(float(x) for x in w)  # assignment: a later emission overwrites an earlier one
                state["env"], state["emit_tex"] = env, tex
                state["emitter"] = state["emitter"] or c.cid == abi.LOBE_EMISSIVE  # material.cpp:205-211
                return
            p = c.params
            if c.cid == abi.LOBE_MICROFACET and p.get("distribution", "ggx") not in ("ggx", "beckmann"):
                raise ValueError(f"unsupported distribution {p['distribution']!r} (src/bsdf.cpp:53-71)")
            extra = {}
            if fac is not None:
                extra = {"fac_mode": int(fac[0]), "fac_ior": float(fac[1]), "pre_weight": tuple(float(x) for x in fac[2]), "fac_texture": int(fac[3])}
            lobes.append(LobeDesc(c.cid, tuple(float(x) for x in w), alpha=float(p.get("alpha", 0.0)), eta=float(p.get("eta", 0.0)),
                                  xalpha=float(p.get("xalpha", 0.0)), yalpha=float(p.get("yalpha", 0.0)), refract=int(p.get("refract", 0)),
                                  r=float(p.get("r", 0.0)), texture=tex, **extra))
    visit(tree, np.ones(3, f32))
    if state["emit_tex"] and any(l.texture or l.fac_texture for l in lobes):
        raise ValueError("a textured emitter whose own closures carry a texture or a mask: images on the lobes of an emitter are not supported")
    if len(lobes) > abi.MAX_LOBES:
        raise ValueError(f"{len(lobes)} lobes: bsdf_t holds at most {abi.MAX_LOBES} (src/bsdf.hpp:9)")
    return MaterialDesc(lobes=lobes, emission=state["e"], is_emitter=state["emitter"], emission_texture=state["env"], emission_uv_texture=state["emit_tex"])


def bake_material(desc, textures=None, emitter_textures=False):
    """`desc`: one entry of the reference's YAML `materials:` map (already parsed, e.g. by yaml.safe_load).  `textures`: the scene's
    list of texture specs {filename, swrap, twrap}, which the material's texture_nodes are added to (lobe.texture = index + 1).
    `emitter_textures`: also bake texture_node.Cout -> diffuse_emitter_node.Cs (MaterialDesc.emission_uv_texture: the image multiplies the
    emission at mesh UVs, with the light-sample UV rule of include/phx_xpu.h, a stated deviation from the reference); refused by default."""
    layers, order = {}, []
    for sh in desc["shaders"]:
        name, layer = sh["name"], sh["layer"]
        if name in UNBAKEABLE:
            raise ValueError(f"shader {name!r} depends on the hit (noise / view direction / normal map): not a closure recipe this baker can express")
        if name not in NODES:
            raise ValueError(f"unknown shader {name!r}")
        params = {}
        for p in sh.get("parameters", []) or []:
            t = p["type"]
            if t == "float":
                params[p["name"]] = float(p["value"])
            elif t == "rgb":
                params[p["name"]] = _color(p["value"])
            elif t == "string":
                params[p["name"]] = str(p["value"])
            else:
                raise ValueError("Unknown parameter type: " + t)  # material.hpp:79
        if NODES[name] in (texture_node, environment_node):
            NODES[name](**params)  # its parameters are checked whether or not the node is connected (a texture without an image raises)
        layers[layer] = (NODES[name], params)
        order.append(layer)
    edges = {}
    for e in desc.get("connect", []) or []:
        edges.setdefault(e["to"]["layer"], []).append((e["to"]["slot"], e["from"]["layer"], e["from"]["slot"]))
    cache = {}

    def evaluate(layer):
        if layer not in cache:
            fn, params = layers[layer]
            args = dict(params)
            for slot, src_layer, src_slot in edges.get(layer, []):
                if src_slot not in ("Cout", "out") or (src_slot == "out" and layers[src_layer][0] not in (fresnel_dielectric_node, luminance_node)):
                    raise ValueError(f"connection from {src_layer}.{src_slot}: only closure outputs (Cout), fresnel_dielectric_node.out and luminance_node.out can be expressed")
                if layers[src_layer][0] is luminance_node and (src_slot != "out" or slot != "fac" or fn is not mix_closure_node):
                    raise ValueError(f"luminance {src_layer}.{src_slot} into {layer}.{slot}: luminance_node.out can drive only the fac of a mix_closure_node")
                to_mask = fn is luminance_node and slot == "in"  # texture_node.Cout -> luminance_node.in: the one way an image reaches a mix's fac
                if layers[src_layer][0] is texture_node and not to_mask and (slot != "Cs" or (fn not in TEXTURABLE and not (emitter_textures and fn is diffuse_emitter_node))):
                    raise ValueError(f"texture {src_layer}.Cout into {layer}.{slot}: a texture can drive only the Cs of a BSDF node or a luminance_node"
                                     " (the Cs of a diffuse_emitter_node too with emitter_textures=True)")
                if layers[src_layer][0] is environment_node and (slot != "Cs" or fn is not background_node):
                    raise ValueError(f"environment {src_layer}.Cout into {layer}.{slot}: an environment map can drive only the Cs of a background_node")
                args[slot] = evaluate(src_layer)
            cache[layer] = fn(**args)
        return cache[layer]
    return flatten(evaluate(order[-1]), textures, emitter_textures)


def bake_materials(yaml_materials, textures=None, emitter_textures=False):
    """name -> MaterialDesc for a whole `materials:` map; ids follow insertion order (scene_t::add, src/scene.cpp:84-90).  The
    texture specs the materials use are collected in `textures` (see bake_material)."""
    return {name: bake_material(d, textures, emitter_textures) for name, d in yaml_materials.items()}
