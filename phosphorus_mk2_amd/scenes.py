"""Scene descriptions handed to a device: the host-side stand-in for what the reference builds through
`mesh_t::builder_t` (src/mesh.hpp:46-67) + `scene_t::add` (src/scene.cpp:64-90), and the synthetic
inputs of SURVEY §8(d): the Cornell box (C1) and Soup(N, seed) triangle soups (C2/C4).

A `SceneDesc` owns numpy arrays; `pack()` builds the ctypes `phx_scene` that points into them.
"""
import math
from dataclasses import dataclass, field, replace
from typing import List, Tuple

import numpy as np

from . import abi


@dataclass
class LobeDesc:
    type: int
    weight: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    alpha: float = 0.0
    eta: float = 0.0
    xalpha: float = 0.0
    yalpha: float = 0.0
    refract: int = 0
    r: float = 0.0
    fac_mode: int = 0          # abi.FAC_*: per-hit mix factor on this closure's weight: Fresnel (glass) or the luminance of an image (FAC_TEX_*)
    fac_ior: float = 0.0
    pre_weight: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    texture: int = 0           # 0: none; k: the weight is multiplied per hit by SceneDesc.textures[k - 1] at the hit's UV
    fac_texture: int = 0       # FAC_TEX_B / FAC_TEX_A: the mask image, k = SceneDesc.textures[k - 1] (its luminance at the hit's UV is the mix factor)


@dataclass
class MaterialDesc:
    lobes: List[LobeDesc] = field(default_factory=list)
    emission: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    is_emitter: bool = False
    emission_texture: int = 0   # environment map: k = textures[k - 1] (the environment material only), 0 = none
    emission_mapping: int = abi.ENV_LATLONG_Y_UP  # abi.ENV_LATLONG_*
    emission_uv_texture: int = 0  # emitters only: the emission is multiplied by textures[k - 1] at mesh UVs (hits and light samples), 0 = none


@dataclass
class MeshDesc:
    vertices: np.ndarray  # (n,3) f32
    faces: np.ndarray     # (k,3) u32
    sets: List[Tuple[int, np.ndarray]]  # (material, face indices u32)
    normals: np.ndarray = None  # (m,3) f32
    smooth: np.ndarray = None   # (k,) u8
    flags: int = abi.MESH_UV_PER_VERTEX | abi.MESH_NORMALS_PER_VERTEX
    uvs: np.ndarray = None      # (u,2) f32 (s, t): per vertex with MESH_UV_PER_VERTEX, else per face corner (3 f + k)

    def __post_init__(self):
        if self.uvs is None:
            self.uvs = np.zeros((0, 2), np.float32)
        self.uvs = np.ascontiguousarray(self.uvs, dtype=np.float32).reshape(-1, 2)
        self.vertices = np.ascontiguousarray(self.vertices, dtype=np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(self.faces, dtype=np.uint32).reshape(-1, 3)
        if self.normals is None:
            self.normals = np.zeros((0, 3), np.float32)
        self.normals = np.ascontiguousarray(self.normals, dtype=np.float32).reshape(-1, 3)
        if self.smooth is None:
            self.smooth = np.zeros(len(self.faces), np.uint8)
        self.smooth = np.ascontiguousarray(self.smooth, dtype=np.uint8)
        self.sets = [(int(m), np.ascontiguousarray(f, dtype=np.uint32)) for m, f in self.sets]


@dataclass
class TextureDesc:
    """An RGB image texture (phx_texture): texels (H, W, 3) linear f32, row 0 = the first scanline (t in [0, 1/H))."""
    texels: np.ndarray
    filter: int = abi.TEX_LINEAR
    swrap: int = abi.WRAP_PERIODIC
    twrap: int = abi.WRAP_PERIODIC

    def __post_init__(self):
        self.texels = np.ascontiguousarray(self.texels, dtype=np.float32)
        if self.texels.ndim != 3 or self.texels.shape[2] != 3:
            raise ValueError(f"texels must be (H, W, 3), not {self.texels.shape}")


@dataclass
class CameraDesc:
    width: int
    height: int
    fov: float = 1.9
    to_world: np.ndarray = None  # Imath M44f x[i][j], row-vector convention
    focal_distance: float = 1.0
    aperture_radius: float = 0.0

    def __post_init__(self):
        if self.to_world is None:
            self.to_world = np.eye(4, dtype=np.float32)
        self.to_world = np.ascontiguousarray(self.to_world, dtype=np.float32).reshape(4, 4)


@dataclass
class SceneDesc:
    meshes: List[MeshDesc]
    materials: List[MaterialDesc]
    camera: CameraDesc
    environment_material: int = -1
    name: str = "scene"
    textures: List[TextureDesc] = field(default_factory=list)

    @property
    def num_triangles(self):
        return sum(sum(len(f) for _, f in m.sets) for m in self.meshes)

    def pack(self):
        """-> (abi.Scene, keepalive).  The ctypes struct borrows the numpy buffers."""
        keep = []
        mats = (abi.Material * len(self.materials))()
        for i, m in enumerate(self.materials):
            mats[i].num_lobes = len(m.lobes)
            mats[i].is_emitter = 1 if m.is_emitter else 0
            mats[i].emission[:] = [np.float32(x) for x in m.emission]
            mats[i].emission_texture, mats[i].emission_mapping = m.emission_texture, m.emission_mapping
            mats[i].emission_uv_texture = m.emission_uv_texture
            for j, l in enumerate(m.lobes):
                d = mats[i].lobes[j]
                d.type = l.type
                d.weight[:] = [np.float32(x) for x in l.weight]
                d.alpha, d.eta, d.xalpha, d.yalpha, d.refract, d.r = l.alpha, l.eta, l.xalpha, l.yalpha, l.refract, l.r
                d.fac_mode, d.fac_ior = abi.fac_pack(l.fac_mode, l.fac_texture), l.fac_ior
                d.pre_weight[:] = [np.float32(x) for x in l.pre_weight]
                d.texture = l.texture
        meshes = (abi.Mesh * len(self.meshes))()
        for i, m in enumerate(self.meshes):
            sets = (abi.FaceSet * len(m.sets))()
            for k, (mat, faces) in enumerate(m.sets):
                sets[k].material = mat
                sets[k].num_faces = len(faces)
                sets[k].faces = faces.ctypes.data_as(abi.u32p)
            keep.append(sets)
            meshes[i].vertices = m.vertices.ctypes.data_as(abi.f32p)
            meshes[i].num_vertices = len(m.vertices)
            meshes[i].normals = m.normals.ctypes.data_as(abi.f32p)
            meshes[i].num_normals = len(m.normals)
            meshes[i].faces = m.faces.ctypes.data_as(abi.u32p)
            meshes[i].num_faces = len(m.faces)
            meshes[i].smooth = m.smooth.ctypes.data_as(abi.u8p)
            meshes[i].flags = m.flags
            meshes[i].num_sets = len(m.sets)
            meshes[i].sets = sets
            meshes[i].uvs = m.uvs.ctypes.data_as(abi.f32p)
            meshes[i].num_uvs = len(m.uvs)
        s = abi.Scene()
        s.num_meshes = len(self.meshes)
        s.meshes = meshes
        s.num_materials = len(self.materials)
        s.materials = mats
        s.environment_material = self.environment_material
        s.camera.to_world[:] = [float(x) for x in self.camera.to_world.reshape(-1)]
        s.camera.fov = self.camera.fov
        s.camera.focal_distance = self.camera.focal_distance
        s.camera.aperture_radius = self.camera.aperture_radius
        s.camera.film_width = self.camera.width
        s.camera.film_height = self.camera.height
        if self.textures:
            texs = (abi.Texture * len(self.textures))()
            for i, t in enumerate(self.textures):
                texs[i].height, texs[i].width = t.texels.shape[0], t.texels.shape[1]
                texs[i].texels = t.texels.ctypes.data_as(abi.f32p)
                texs[i].filter, texs[i].swrap, texs[i].twrap = t.filter, t.swrap, t.twrap
            s.num_textures = len(self.textures)
            s.textures = texs
            keep.append(texs)
        keep += [mats, meshes, self]
        return s, keep


def diffuse(r, g, b):
    return MaterialDesc(lobes=[LobeDesc(abi.LOBE_DIFFUSE, (r, g, b))])


def emitter(r, g, b):
    # diffuse_emitter_node.osl:18 -> only an emission() closure: 0 lobes, e = weight
    return MaterialDesc(lobes=[], emission=(r, g, b), is_emitter=True)


def _quad(a, b, c, d, material):
    """One quad = its own mesh, 4 vertices, two flat faces (a,b,c),(a,c,d), one face set."""
    v = np.array([a, b, c, d], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return MeshDesc(vertices=v, faces=f, sets=[(material, np.array([0, 1], np.uint32))])


LE = (17.0 / math.pi, 12.0 / math.pi, 4.0 / math.pi)


def cornell(width=256, height=256, fov=1.9):
    """C1: 5 diffuse quads + 1 emissive quad (12 triangles), camera at the origin looking down -z.

    Geometric normals ((b-a) x (c-a), never flipped: src/mesh.cpp:203-215) face into the box so that
    next-event estimation is not masked (src/kernels/cpu/spt.hpp:138-141).
    """
    W, R, G, L = 0, 1, 2, 3
    mats = [diffuse(0.73, 0.73, 0.73), diffuse(0.65, 0.05, 0.05), diffuse(0.12, 0.45, 0.15), emitter(*LE)]
    x0, x1, y0, y1, zf, zb = -1.0, 1.0, -1.0, 1.0, -1.5, -3.5
    meshes = [
        _quad((x0, y0, zf), (x1, y0, zf), (x1, y0, zb), (x0, y0, zb), W),   # floor, n = +y
        _quad((x0, y1, zf), (x0, y1, zb), (x1, y1, zb), (x1, y1, zf), W),   # ceiling, n = -y
        _quad((x0, y0, zb), (x1, y0, zb), (x1, y1, zb), (x0, y1, zb), W),   # back, n = +z
        _quad((x0, y0, zf), (x0, y0, zb), (x0, y1, zb), (x0, y1, zf), R),   # left, n = +x
        _quad((x1, y0, zf), (x1, y1, zf), (x1, y1, zb), (x1, y0, zb), G),   # right, n = -x
        _quad((-0.25, 0.99, -2.25), (-0.25, 0.99, -2.75), (0.25, 0.99, -2.75), (0.25, 0.99, -2.25), L),  # lamp, n = -y
    ]
    return SceneDesc(meshes, mats, CameraDesc(width, height, fov), name="cornell")


def _u01(idx, seed):
    """Counter-based uniform [0,1) with 24 bits: splitmix64 finaliser of (seed, idx).  numpy uint64 wraps."""
    with np.errstate(over="ignore"):
        x = (idx.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return ((x >> np.uint64(40)).astype(np.float64) * (1.0 / 16777216.0)).astype(np.float32)


def soup(n, seed=1234, width=1280, height=720, fov=1.9, light=True, materials=None):
    """Soup(N, seed), SURVEY §8(d): N triangles, centre uniform in [-0.98,0.98]^3 shifted to z=-2.5,
    vertices = centre + e*U(-1,1)^3 with e = 2*N^(-1/3); 12 draws per triangle in the order centre xyz,
    a xyz, b xyz, c xyz; flat faces, unshared vertices; one grey diffuse material (0.73) unless a list
    of materials is given (then triangle i uses material i % len).  Lit by a 4x4 emissive quad at
    y=+1.5 facing down, L_e=(17,12,4)/pi, outside the cloud.
    """
    n = int(n)
    e = np.float32(2.0 * n ** (-1.0 / 3.0))
    verts = np.empty((n, 3, 3), np.float32)
    step = 1 << 16  # triangles per block: the 64-bit hash temporaries of a block stay in cache (10 M triangles: 30 s -> 4 s)
    for t0 in range(0, n, step):
        t1 = min(n, t0 + step)
        idx = np.arange(t0 * 12, t1 * 12, dtype=np.uint64)
        u = (_u01(idx, seed) * np.float32(2.0) - np.float32(1.0)).reshape(t1 - t0, 12)
        centre = u[:, 0:3] * np.float32(0.98)
        centre[:, 2] -= np.float32(2.5)
        for k in range(3):
            verts[t0:t1, k, :] = centre + e * u[:, 3 + 3 * k:6 + 3 * k]
    faces = np.arange(n * 3, dtype=np.uint32).reshape(n, 3)
    mats = list(materials) if materials else [diffuse(0.73, 0.73, 0.73)]
    nm = len(mats)
    if nm == 1:
        sets = [(0, np.arange(n, dtype=np.uint32))]
    else:
        sets = [(m, np.arange(m, n, nm, dtype=np.uint32)) for m in range(nm)]
    meshes = [MeshDesc(vertices=verts.reshape(-1, 3), faces=faces, sets=sets)]
    if light:
        mats.append(emitter(*LE))
        meshes.append(_quad((-2.0, 1.5, -0.5), (-2.0, 1.5, -4.5), (2.0, 1.5, -4.5), (2.0, 1.5, -0.5), len(mats) - 1))
    return SceneDesc(meshes, mats, CameraDesc(width, height, fov), name=f"soup{n}")


def stress(seed=7, width=64, height=64):
    """Geometry chosen to break builders and box tests, not to look like anything: a small soup + zero-area triangles
    (collinear, repeated vertices) + ten coincident copies of each of 20 triangles (exact distance ties: the lowest
    primitive index must win) + a chain whose sizes fall from 1 to 2^-20 ("teapot in a stadium") + triangles with
    coordinates up to 1e4 + axis-aligned flat triangles (boxes of zero extent).  One grey material, the soup's light."""
    rng = np.random.default_rng(seed)
    def rnd(n, scale, centre=(0.0, 0.0, -2.5)):
        c = rng.uniform(-0.9, 0.9, (n, 1, 3)) + np.array(centre)
        return (c + rng.uniform(-scale, scale, (n, 3, 3))).astype(np.float32)
    parts = [rnd(600, 0.12)]
    deg = rnd(200, 0.2)
    deg[:100, 2] = deg[:100, 1]                                             # repeated vertex
    deg[100:, 2] = (0.25 * deg[100:, 0] + 0.75 * deg[100:, 1]).astype(np.float32)  # (nearly) collinear
    parts.append(deg)
    parts.append(np.repeat(rnd(20, 0.3), 10, axis=0))                          # coincident copies, interleaved below
    chain = np.zeros((63, 3, 3), np.float32)
    for k in range(63):
        sz = np.float32(2.0 ** -(k % 21))
        base = np.array([-0.9 + 0.028 * k, -0.5, -2.0 - 0.01 * k], np.float32)
        chain[k] = base + sz * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.25]], np.float32)
    parts.append(chain)
    parts.append((rnd(50, 1.0) * np.float32(1.0e4)).astype(np.float32))        # far away and huge
    flat = rnd(120, 0.25)
    flat[:40, :, 0] = flat[:40, :1, 0]; flat[40:80, :, 1] = flat[40:80, :1, 1]; flat[80:, :, 2] = flat[80:, :1, 2]
    parts.append(flat)
    verts = np.concatenate(parts).astype(np.float32)
    order = rng.permutation(len(verts))                                        # shuffle primitive ids
    verts = verts[order]
    n = len(verts)
    faces = np.arange(n * 3, dtype=np.uint32).reshape(n, 3)
    mats = [diffuse(0.73, 0.73, 0.73), emitter(*LE)]
    meshes = [MeshDesc(vertices=verts.reshape(-1, 3), faces=faces, sets=[(0, np.arange(n, dtype=np.uint32))]),
              _quad((-2.0, 1.5, -0.5), (-2.0, 1.5, -4.5), (2.0, 1.5, -4.5), (2.0, 1.5, -0.5), 1)]
    return SceneDesc(meshes, mats, CameraDesc(width, height, 1.9), name="stress")


def smooth_blobs(width=96, height=64, per_vertex=True):
    """Smooth-shaded geometry for the interpolated-normal path of mesh_t::shading_parameters
    (src/mesh.cpp:187-199): two subdivided octahedra ("blobs") with per-vertex normals — or per-face-corner
    normals when `per_vertex` is False (set_normals_per_vertex_per_face, src/mesh.hpp:64) — inside a
    flat-shaded floor/back wall, lit by TWO emissive quads (light pick by index, src/sampling.cpp:165) of
    which one is a 4-triangle strip (uniform triangle pick, src/light.cpp:55)."""
    def octa(centre, radius, levels):
        v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
        f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
        v = [np.array(x, np.float64) for x in v]
        for _ in range(levels):
            nf, cache = [], {}
            def mid(a, b):
                k = (min(a, b), max(a, b))
                if k not in cache:
                    m = v[a] + v[b]; v.append(m / np.linalg.norm(m)); cache[k] = len(v) - 1
                return cache[k]
            for a, b, c in f:
                ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
                nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
            f = nf
        n = np.array(v, np.float32)
        return (n * np.float32(radius) + np.array(centre, np.float32)).astype(np.float32), n, np.array(f, np.uint32)
    mats = [diffuse(0.73, 0.73, 0.73), diffuse(0.2, 0.5, 0.7),
            MaterialDesc([LobeDesc(abi.LOBE_DIFFUSE, (0.5, 0.4, 0.3)), LobeDesc(abi.LOBE_MICROFACET, (0.3, 0.3, 0.3), xalpha=0.09, yalpha=0.09)]),
            emitter(*LE), emitter(4.0, 4.0, 6.0)]
    meshes = [
        _quad((-2, -1, -1), (2, -1, -1), (2, -1, -4), (-2, -1, -4), 0),
        _quad((-2, -1, -4), (2, -1, -4), (2, 2, -4), (-2, 2, -4), 0),
    ]
    for centre, radius, mat in (((-0.6, -0.4, -2.6), 0.6, 1), ((0.7, -0.5, -2.2), 0.5, 2)):
        v, n, f = octa(centre, radius, 2)
        if per_vertex:
            m = MeshDesc(vertices=v, faces=f, normals=n, smooth=np.ones(len(f), np.uint8), sets=[(mat, np.arange(len(f), dtype=np.uint32))])
        else:  # one normal per face corner, indexed by 3*face + corner (mesh.cpp:188-192); every other face flat
            smooth = (np.arange(len(f)) % 2 == 0).astype(np.uint8)
            m = MeshDesc(vertices=v, faces=f, normals=n[f.reshape(-1)], smooth=smooth, sets=[(mat, np.arange(len(f), dtype=np.uint32))],
                         flags=abi.MESH_UV_PER_VERTEX)
        meshes.append(m)
    meshes.append(_quad((-0.5, 1.9, -2.0), (-0.5, 1.9, -3.0), (0.5, 1.9, -3.0), (0.5, 1.9, -2.0), 3))
    strip_v = np.array([(-1.9, 0.0, -1.2), (-1.9, 1.0, -1.2), (-1.9, 0.0, -2.0), (-1.9, 1.0, -2.0), (-1.9, 0.0, -2.8), (-1.9, 1.0, -2.8)], np.float32)
    strip_f = np.array([(0, 2, 1), (1, 2, 3), (2, 4, 3), (3, 4, 5)], np.uint32)  # normals +x
    meshes.append(MeshDesc(vertices=strip_v, faces=strip_f, sets=[(4, np.arange(4, dtype=np.uint32))]))
    return SceneDesc(meshes, mats, CameraDesc(width, height, 1.6), name="smooth_blobs")


def closure_zoo():
    """One material per lobe type of src/bsdf.hpp:14-24 plus mixes, mirroring the constant-input
    mappings of the BSDF-node shaders: used by the BSDF known-answer tests and
    the multi-material stand-in scenes."""
    D, ON, RF, RR, MF, SH, TR = (abi.LOBE_DIFFUSE, abi.LOBE_OREN_NAYAR, abi.LOBE_REFLECTION, abi.LOBE_REFRACTION,
                                 abi.LOBE_MICROFACET, abi.LOBE_SHEEN, abi.LOBE_TRANSPARENT)
    return [
        diffuse(0.73, 0.73, 0.73),                                                          # 0 diffuse_bsdf_node, roughness 0
        MaterialDesc([LobeDesc(ON, (0.6, 0.5, 0.4), alpha=0.5)]),                           # 1 oren_nayar(N, roughness)
        MaterialDesc([LobeDesc(RF, (0.9, 0.9, 0.9), eta=0.0)]),                             # 2 glossy sharp -> reflection(N,0)
        MaterialDesc([LobeDesc(RR, (0.95, 0.95, 0.95), eta=1.45)]),                         # 3 refraction sharp
        MaterialDesc([LobeDesc(MF, (0.8, 0.7, 0.3), xalpha=0.09, yalpha=0.09)]),            # 4 glossy r=0.3 -> microfacet(r^2)
        MaterialDesc([LobeDesc(MF, (0.9, 0.9, 0.9), eta=1.33, xalpha=0.2, yalpha=0.2, refract=1)]),  # 5 rough refraction
        MaterialDesc([LobeDesc(SH, (0.5, 0.2, 0.6), r=0.4)]),                               # 6 sheen
        MaterialDesc([LobeDesc(TR, (0.8, 0.9, 0.8))]),                                      # 7 transparent
        MaterialDesc([LobeDesc(D, (0.4, 0.3, 0.2)), LobeDesc(MF, (0.3, 0.3, 0.3), xalpha=0.04, yalpha=0.04)]),  # 8 mix diffuse+glossy
        MaterialDesc([LobeDesc(D, (0.3, 0.3, 0.5)), LobeDesc(SH, (0.3, 0.3, 0.3), r=0.4), LobeDesc(ON, (0.2, 0.2, 0.2), alpha=0.3)]),  # 9 three lobes
        MaterialDesc([LobeDesc(RR, (0.6, 0.6, 0.6), eta=1.5), LobeDesc(RF, (0.3, 0.3, 0.3))]),  # 10 glass-like constant mix
        MaterialDesc([LobeDesc(MF, (0.7, 0.7, 0.7), xalpha=0.25, yalpha=0.0625)]),          # 11 anisotropic glossy
    ]


def glass(ior=1.45, roughness=0.0, Cs_refraction=(1.0, 1.0, 1.0), Cs_reflection=(1.0, 1.0, 1.0)):
    """Blender's glass node as the reference's exporter builds it (plugins/blender/blender/shader.hpp:306-335):
    mix_closure_node(A = refraction_bsdf_node(IoR, roughness), B = glossy_bsdf_node(roughness), fac = fresnel_dielectric_node(IoR)),
    i.e. what closures.bake_material returns for that node group: two closures whose weights depend on the hit."""
    from . import closures as cl
    tree = cl.mix_closure_node(A=cl.refraction_bsdf_node(Cs=Cs_refraction, IoR=ior, roughness=roughness),
                               B=cl.glossy_bsdf_node(Cs=Cs_reflection, roughness=roughness), fac=cl.fresnel_dielectric_node(IoR=ior))
    return cl.flatten(tree)


def glass_blobs(width=96, height=64):
    """smooth_blobs() with one blob of sharp glass (IoR 1.45) and one of frosted glass (IoR 1.33, roughness 0.2)"""
    s = smooth_blobs(width, height)
    s.materials[1] = glass(1.45, 0.0, (0.95, 0.98, 0.95), (1.0, 1.0, 1.0))
    s.materials[2] = glass(1.33, 0.2, (0.9, 0.9, 1.0), (0.9, 0.9, 0.9))
    s.name = "glass_blobs"
    return s


def multi_material_soup(n, seed=1234, width=1280, height=720):
    """Declared stand-in for the BMW configs (no scene data ships with the reference):
    Soup(N) whose triangles cycle through closure_zoo() + 4 more diffuse tints = 16 closure recipes."""
    mats = closure_zoo() + [diffuse(0.7, 0.2, 0.2), diffuse(0.2, 0.7, 0.2), diffuse(0.2, 0.2, 0.7), diffuse(0.5, 0.5, 0.1)]
    s = soup(n, seed, width, height, materials=mats)
    s.name = f"zoo_soup{n}"
    return s


def showroom(n, seed=5, width=1280, height=720, materials=None, closed=False):
    """A non-uniform, mesh-like scene (connected surfaces, three orders of magnitude of triangle sizes): a closed grey room with a
    ceiling light holding 24 lat/long-tessellated spheres of radius 0.04..0.55 whose triangle counts are NOT proportional to their
    area (the smallest sphere gets as many triangles as the largest: "teapot in a stadium"), about n triangles in total.  Used to
    check both tree builders — and PHX_BVH_AUTO's choice between them — on something that is not the uniform soup of SURVEY §8(d).
    With `materials` the spheres cycle through that list (material 0 stays the room's).  The room is open towards the camera (which stands
    in front of it, at the origin); `closed` pulls floor, ceiling and side walls past the camera and adds the wall behind it: no path
    leaves the room, every path ends by roulette, the depth limit or absorption."""
    rng = np.random.default_rng(seed)
    mats = [diffuse(0.73, 0.73, 0.73)] + (list(materials) if materials else [diffuse(0.6, 0.3, 0.2), diffuse(0.2, 0.5, 0.7)])
    nm = len(mats)
    mats.append(emitter(*LE))
    X0, X1, Y0, Y1, Z0, Z1 = -2.0, 2.0, -1.0, 1.6, -4.6, (0.4 if closed else -0.4)
    meshes = [
        _quad((X0, Y0, Z1), (X1, Y0, Z1), (X1, Y0, Z0), (X0, Y0, Z0), 0),   # floor
        _quad((X0, Y0, Z0), (X1, Y0, Z0), (X1, Y1, Z0), (X0, Y1, Z0), 0),   # back
        _quad((X0, Y0, Z1), (X0, Y0, Z0), (X0, Y1, Z0), (X0, Y1, Z1), 0),   # left
        _quad((X1, Y0, Z0), (X1, Y0, Z1), (X1, Y1, Z1), (X1, Y1, Z0), 0),   # right
        _quad((X0, Y1, Z0), (X1, Y1, Z0), (X1, Y1, Z1), (X0, Y1, Z1), 0),   # ceiling
        _quad((-0.8, Y1 - 0.01, -1.7), (-0.8, Y1 - 0.01, -3.3), (0.8, Y1 - 0.01, -3.3), (0.8, Y1 - 0.01, -1.7), nm),
    ]
    if closed:
        meshes.append(_quad((X1, Y0, Z1), (X0, Y0, Z1), (X0, Y1, Z1), (X1, Y1, Z1), 0))   # the wall behind the camera, facing the room
    nspheres = 24
    per = max(8, int(n) // nspheres)
    for k in range(nspheres):
        radius = float(0.04 * (0.55 / 0.04) ** rng.random())
        centre = np.array([rng.uniform(X0 + radius, X1 - radius), rng.uniform(Y0 + radius, Y1 - 0.3 - radius), rng.uniform(Z0 + radius, -1.2 - radius)])
        rings = max(2, int(round(np.sqrt(per / 4.0))))          # 2*rings*segs triangles with segs = 2*rings
        segs = 2 * rings
        th = np.linspace(0.0, np.pi, rings + 1)[:, None]
        ph = np.linspace(0.0, 2.0 * np.pi, segs + 1)[None, :-1]
        p = np.stack([np.sin(th) * np.cos(ph), np.cos(th) * np.ones_like(ph), np.sin(th) * np.sin(ph)], -1)  # (rings+1, segs, 3)
        v = (centre + radius * p.reshape(-1, 3)).astype(np.float32)
        i = np.arange(rings)[:, None]; j = np.arange(segs)[None, :]
        a = (i * segs + j).ravel(); b = (i * segs + (j + 1) % segs).ravel()
        c = ((i + 1) * segs + j).ravel(); d = ((i + 1) * segs + (j + 1) % segs).ravel()
        f = np.concatenate([np.stack([a, b, d], 1), np.stack([a, d, c], 1)]).astype(np.uint32)  # outward-facing; the pole rows hold slivers of zero area
        meshes.append(MeshDesc(vertices=v, faces=f, sets=[(1 + k % (nm - 1), np.arange(len(f), dtype=np.uint32))]))
    return SceneDesc(meshes, mats, CameraDesc(width, height, 1.9), name=f"showroom{n}{'_closed' if closed else ''}")


def deep_comb(n=400, ratio=1.08, width=64, height=48, material=None, lamp=True):
    """A scene whose BVH is DEEP, so that k_trace's stack reaches the levels it keeps in HBM: a geometric comb of n triangles at
    x_i = ratio^i (i = 0 .. n - 1), each in the plane x = x_i, facing the origin (geometric normal -x) and 0.5 x_i across, so that every
    one subtends the same angle from the origin.  The binned SAH builder peels such a comb into a chain (depth 16 for 400 x 1.08 and for
    200 x 1.2), and a ray that travels +x along it pushes one pending sibling group per level.  Past x ~ 1e13 the fp32 products of the
    triangle test (~x^3) overflow, so rays that far out miss; keep ratio^n near the defaults'.  `material` is the comb's (default: sharp
    glass, IoR 1.45, whose refracted rays carry on down the comb); `lamp` adds a 2 x 2 emissive quad at x = -0.3 facing +x, behind the
    camera.  The camera stands at the origin and looks down +x (fov 0.6)."""
    x = (np.float64(ratio) ** np.arange(int(n), dtype=np.float64))[:, None]
    # equilateral, side 0.5 x_i, centred on the x axis; (b - a) x (c - a) points -x, towards the camera
    h, c = 0.25 * x, x / (4.0 * math.sqrt(3.0))  # half the side; the centre's distance from a side
    verts = np.stack([np.concatenate([x, h, -c], 1), np.concatenate([x, -h, -c], 1), np.concatenate([x, 0.0 * x, 2.0 * c], 1)], 1).astype(np.float32)
    faces = np.arange(3 * int(n), dtype=np.uint32).reshape(-1, 3)
    mats = [material if material is not None else glass(1.45)]
    meshes = [MeshDesc(vertices=verts.reshape(-1, 3), faces=faces, sets=[(0, np.arange(int(n), dtype=np.uint32))])]
    if lamp:
        mats.append(emitter(*LE))
        meshes.append(_quad((-0.3, -1.0, -1.0), (-0.3, 1.0, -1.0), (-0.3, 1.0, 1.0), (-0.3, -1.0, 1.0), 1))  # n = +x
    sc = SceneDesc(meshes, mats, CameraDesc(width, height, 0.6), name=f"deep_comb{int(n)}")
    # the camera turned a quarter turn to the right about y: (0, 0, -1) -> (1, 0, 0) (CameraDesc.to_world, Imath row-vector convention)
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32)
    sc.camera.to_world = M
    return sc


def deep_comb_rays(count, n=400, ratio=1.08, seed=0):
    """`count` rays of deep_comb(n, ratio) that travel +x along it: each starts just past a random triangle k of the comb with x_k <= 1e12,
    off the axis by up to a third of that triangle's inradius, so that it hits triangle k + 1.  (Further out the fp32 products of the
    triangle test, ~x^3, overflow: the device and the oracle then agree on a miss.)  -> (o, d, tmax = FLT_MAX) float32 arrays; a walk down
    the comb takes one stack level per level of the tree."""
    rng = np.random.default_rng(seed)
    kmax = min(int(n) - 1, int(math.floor(12.0 / math.log10(ratio))))
    x = np.float64(ratio) ** rng.integers(0, kmax, count)
    off = rng.uniform(-1.0, 1.0, (count, 2)) * (x / (12.0 * math.sqrt(3.0)))[:, None]
    o = np.concatenate([(x * (1.0 + 1e-3))[:, None], off], 1).astype(np.float32)
    d = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (count, 1))
    return o, d, np.full(count, np.finfo(np.float32).max, np.float32)


def showroom_materials(per_hit_glass=True):
    """the 16 closure recipes of the BMW stand-in (closure_zoo() + four diffuse tints) plus Blender's glass node twice — sharp
    (IoR 1.45) and frosted (IoR 1.33, roughness 0.2) — whose closure weights depend on the hit (k_shade_g<PERHIT>): 18 materials.
    per_hit_glass=False (A/B experiments only): the two glass materials as constant refraction + reflection mixes."""
    z = closure_zoo()
    g = [glass(1.45, 0.0, (0.95, 0.98, 0.95), (1.0, 1.0, 1.0)), glass(1.33, 0.2, (0.9, 0.9, 1.0), (0.9, 0.9, 0.9))] if per_hit_glass else [z[10], z[5]]
    return z + [diffuse(0.7, 0.2, 0.2), diffuse(0.2, 0.7, 0.2), diffuse(0.2, 0.2, 0.7), diffuse(0.5, 0.5, 0.1)] + g


def procedural_texture(size, seed=0):
    """A (size, size, 3) f32 image in [0.05, 0.95]: a smooth colour gradient under a checker of 16 x 16 squares and some noise."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0.0, 1.0, size, dtype=np.float32), np.linspace(0.0, 1.0, size, dtype=np.float32), indexing="ij")
    check = ((np.floor(x * 16) + np.floor(y * 16)) % 2).astype(np.float32)
    img = np.stack([0.2 + 0.6 * x, 0.2 + 0.6 * y, 0.5 + 0.3 * (check - 0.5)], -1) * (0.8 + 0.2 * check)[..., None]
    img += rng.uniform(-0.05, 0.05, img.shape).astype(np.float32)
    return np.clip(img, 0.05, 0.95).astype(np.float32)


def _sphere_uvs(m):
    """per-vertex lat/long UVs of a showroom sphere (its vertices are rings x segments around its centre)"""
    c = m.vertices.mean(0)
    d = m.vertices - c
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    s = (np.arctan2(d[:, 2], d[:, 0]) / (2.0 * np.pi)) % 1.0
    t = np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi
    return np.stack([s, t], 1).astype(np.float32)


def textured_showroom(n=500_000, width=1920, height=1080, tex_size=2048, baked=False, seed=0):
    """bmw_showroom() with the diffuse recipes (the room and the sphere materials of one Lambert lobe) driven by image textures: one
    procedural tex_size^2 LINEAR texture per recipe, per-vertex lat/long UVs on the spheres, per-corner UVs on the room's quads.
    baked=True: the same scene with 1 x 1 textures holding each image's mean, i.e. the per-hit path with constant texels (the cost
    of the texel gathers is the difference of the two)."""
    s = bmw_showroom(n, width, height)
    quad_uv = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32)  # _quad's two faces (a b c), (a c d)
    for m in s.meshes:
        if len(m.faces) == 2:
            m.uvs = quad_uv * 3.0  # the room's walls repeat the image 3 x 3 times (PERIODIC)
            m.flags = m.flags & ~abi.MESH_UV_PER_VERTEX
        else:
            m.uvs = _sphere_uvs(m)
    textures = []
    for i, mat in enumerate(s.materials):
        if mat.is_emitter or len(mat.lobes) != 1 or mat.lobes[0].type != abi.LOBE_DIFFUSE:
            continue
        img = procedural_texture(tex_size, seed + i)
        if baked:
            img = img.reshape(-1, 3).mean(0, dtype=np.float64).astype(np.float32).reshape(1, 1, 3)
        textures.append(TextureDesc(img, abi.TEX_LINEAR))
        mat.lobes[0].texture = len(textures)
    s.textures = textures
    s.name = f"textured_showroom{n}" + ("_baked" if baked else "")
    return s


def mask_luminance(rgb):
    """the mix factor an image texel gives (luminance_node.osl), fp32 in the device's order: (r * 0.2126 + g * 0.7152) + b * 0.0722"""
    c = np.asarray(rgb, np.float32)
    return np.float32(np.float32(np.float32(c[0] * np.float32(0.2126)) + np.float32(c[1] * np.float32(0.7152))) + np.float32(c[2] * np.float32(0.0722)))


def resolve_masks(mat, texel_of):
    """`mat` with its image-masked lobes (FAC_TEX_*) resolved for hits at which mask k reads the constant texel texel_of(k): FAC_NONE lobes
    of weight (pre_weight * term) * weight, computed in fp32 in the device's order, all-zero ones dropped — the material such a hit sees."""
    f32 = np.float32
    lobes = []
    for l in mat.lobes:
        if l.fac_mode not in (abi.FAC_TEX_B, abi.FAC_TEX_A):
            lobes.append(replace(l))
            continue
        if l.texture:
            raise ValueError("resolve_masks: a masked lobe with a colour texture has no constant weight")
        fac = mask_luminance(texel_of(l.fac_texture))
        term = fac if l.fac_mode == abi.FAC_TEX_B else f32(f32(1.0) - fac)
        w = tuple(float(f32(f32(f32(p) * term) * f32(x))) for p, x in zip(l.pre_weight, l.weight))
        if any(x != 0.0 for x in w):
            lobes.append(replace(l, weight=w, fac_mode=abi.FAC_NONE, fac_ior=0.0, pre_weight=(1.0, 1.0, 1.0), fac_texture=0))
    return replace(mat, lobes=lobes)


def procedural_mask(size, seed=0):
    """A (size, size, 3) f32 grey image in [0, 1] with regions of exactly 0 and exactly 1 (where a masked mix drops one side): the red
    channel of procedural_texture() stretched past both ends and clipped."""
    g = procedural_texture(size, seed)[..., 0]
    grey = np.clip((g - np.float32(0.35)) * np.float32(3.0), 0.0, 1.0).astype(np.float32)
    return np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))


def masked_showroom(n=500_000, width=1920, height=1080, tex_size=2048, mode="image", seed=0):
    """bmw_showroom() with its diffuse recipes (the room and the sphere materials of one Lambert lobe) turned into
    mix(diffuse, glossy, mask): the Lambert lobe on the mix's A side, a GGX lobe (roughness 0.3) on its B side, the factor the luminance of
    one procedural tex_size^2 LINEAR grey image per recipe (UVs as in textured_showroom()).
    mode "image": those masks.  "one_texel": 1 x 1 images holding each mask's mean — the same kernels (k_shade_g<.., MASK>) whose lookups
    hit one texel.  "baked": the mix each one_texel mask gives resolved into constant FAC_NONE weights (resolve_masks), no image, no UVs:
    today's kernels, and bit for bit the film of "one_texel"."""
    if mode not in ("image", "one_texel", "baked"):
        raise ValueError(f"masked_showroom: unknown mode {mode!r}")
    s = bmw_showroom(n, width, height)
    quad_uv = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], np.float32)
    if mode != "baked":
        for m in s.meshes:
            if len(m.faces) == 2:
                m.uvs = quad_uv * 3.0
                m.flags = m.flags & ~abi.MESH_UV_PER_VERTEX
            else:
                m.uvs = _sphere_uvs(m)
    textures = []
    for i, mat in enumerate(s.materials):
        if mat.is_emitter or len(mat.lobes) != 1 or mat.lobes[0].type != abi.LOBE_DIFFUSE:
            continue
        img = procedural_mask(tex_size, seed + i)
        if mode != "image":
            img = img.reshape(-1, 3).mean(0, dtype=np.float64).astype(np.float32).reshape(1, 1, 3)
        textures.append(TextureDesc(img, abi.TEX_LINEAR))
        k = len(textures)
        mat.lobes = [replace(mat.lobes[0], fac_mode=abi.FAC_TEX_A, fac_texture=k),
                     LobeDesc(abi.LOBE_MICROFACET, (0.9, 0.9, 0.9), xalpha=0.09, yalpha=0.09, fac_mode=abi.FAC_TEX_B, fac_texture=k)]
        if mode == "baked":
            mat.lobes = resolve_masks(mat, lambda j: textures[j - 1].texels[0, 0]).lobes
    s.textures = [] if mode == "baked" else textures
    s.name = f"masked_showroom{n}_{mode}"
    return s


def procedural_sky(width=2048, height=1024, sun_elevation=0.5, sun_azimuth=0.6, sun_radius=0.035, sun=(1500.0, 1350.0, 1100.0)):
    """A lat-long HDR sky (height, width, 3) f32 for abi.ENV_LATLONG_Y_UP: texel (i, j) holds the direction of s = (i + 0.5) / W,
    t = (j + 0.5) / H, elevation pi (0.5 - t) and azimuth 2 pi (s - 0.5) measured from +z towards -x.  A blue gradient from the
    horizon to the zenith, a darker ground below the horizon and a small, bright sun disc (`sun_radius` radians, radiance `sun`)."""
    s = (np.arange(width, dtype=np.float64) + 0.5) / width
    t = (np.arange(height, dtype=np.float64) + 0.5) / height
    el = np.pi * (0.5 - t)[:, None] * np.ones((1, width))
    az = 2.0 * np.pi * (s - 0.5)[None, :] * np.ones((height, 1))
    d = np.stack([-np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)], -1)
    up = np.clip(np.sin(el), 0.0, 1.0)[..., None]
    horizon, zenith, ground = np.array([0.9, 0.95, 1.0]), np.array([0.15, 0.35, 0.9]), np.array([0.25, 0.22, 0.2])
    img = np.where(el[..., None] >= 0.0, horizon + (zenith - horizon) * np.sqrt(up), ground * (1.0 + 0.5 * np.sin(el)[..., None]))
    sd = np.array([-np.cos(sun_elevation) * np.sin(sun_azimuth), np.sin(sun_elevation), np.cos(sun_elevation) * np.cos(sun_azimuth)])
    img = np.where((d @ sd >= np.cos(sun_radius))[..., None], np.asarray(sun, np.float64), img)
    return img.astype(np.float32)


def environment_showroom(n=500_000, width=1920, height=1080, sky=(2048, 1024), mode="image"):
    """The OPEN showroom (showroom() with showroom_materials() on its spheres, its ceiling light kept) lit through its open side by
    procedural_sky(*sky) as a Y-up lat-long environment map.  mode "image": the sky image; "mean": a 1 x 1 image of the sky's mean (the
    same kernels, whose lookups then read one texel); "constant": no image, the environment's emission is the sky's mean (the kernels
    without the environment lookup)."""
    s = showroom(n, width=width, height=height, materials=showroom_materials())
    img = procedural_sky(*sky)
    mean = img.reshape(-1, 3).mean(0, dtype=np.float64).astype(np.float32)
    if mode == "constant":
        s.materials.append(MaterialDesc(lobes=[], emission=tuple(float(x) for x in mean)))
    else:
        if mode == "mean":
            img = mean.reshape(1, 1, 3)
        elif mode != "image":
            raise ValueError(f"mode {mode!r}: image, mean or constant")
        s.textures = [TextureDesc(img, abi.TEX_LINEAR, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)]
        s.materials.append(MaterialDesc(lobes=[], emission=(1.0, 1.0, 1.0), emission_texture=1, emission_mapping=abi.ENV_LATLONG_Y_UP))
    s.environment_material = len(s.materials) - 1
    s.name = f"environment_showroom{n}_{mode}"
    return s


def bmw_showroom(n=500_000, width=1920, height=1080, per_hit_glass=True):
    """The mesh-geometry stand-in for BASELINE configs 3 / 5: the CLOSED showroom — connected surfaces, triangle sizes
    over three decades, no path escapes — with showroom_materials() on its 24 spheres.  multi_material_soup() stays the open, uniform one."""
    s = showroom(n, width=width, height=height, materials=showroom_materials(per_hit_glass), closed=True)
    s.name = f"bmw_showroom{n}" + ("" if per_hit_glass else "_constant_glass")
    return s


def lamp_showroom(n=500_000, lamps=64, width=1920, height=1080, side=0.05, emission=(1.0, 0.1, 0.1)):
    """bmw_showroom plus `lamps` small dim emissive quads (indicator LEDs of side `side`) in a grid on the back wall, each a mesh and a light of
    its own: one lamp delivers nearly all of the light, and uniform light selection sends lamps / (lamps + 1) of its shadow rays to the
    rest (light_selection="power")."""
    s = bmw_showroom(n, width, height)
    s.materials.append(emitter(*emission))
    cols = int(math.ceil(math.sqrt(lamps)))
    rows = (lamps + cols - 1) // cols
    z = -4.6 + 0.001  # a millimetre in front of the back wall, facing the room (+z)
    for k in range(lamps):
        x = -1.75 + 3.5 * ((k % cols) + 0.5) / cols; y = -0.7 + 2.0 * ((k // cols) + 0.5) / rows
        h = 0.5 * side
        s.meshes.append(_quad((x - h, y - h, z), (x + h, y - h, z), (x + h, y + h, z), (x - h, y + h, z), len(s.materials) - 1))
    s.name = f"lamp_showroom{n}_{lamps}"
    return s


def sun_and_sky(width=64, height=32, sky=0.1, sun=2000.0, sun_texel=(40, 8)):
    """A small lat-long sky (height, width, 3) f32: `sky` everywhere and ONE texel (column, row) of radiance `sun` -- row 8 of 32 is about
    42 degrees of elevation.  The image environment sampling is tested on: nearly all of its light comes from 1 texel of 2048."""
    img = np.full((height, width, 3), sky, np.float32)
    img[sun_texel[1], sun_texel[0]] = sun
    return img


SUN_FLOOR_RHO = (0.8, 0.5, 0.2)


def sun_floor(width=32, height=32, image=None, mapping=abi.ENV_LATLONG_Y_UP, look="down"):
    """A Lambert floor (y = 0, rho = SUN_FLOOR_RHO) that fills the view of a camera looking straight down from y = 1, under sun_and_sky() as a
    CLOSEST lat-long environment.  A black emitter triangle hides below the floor: a scene needs one emissive face set, and selection by power
    never samples it (w = 0).  Every floor point sees the whole upper hemisphere, so every pixel has the same closed-form expectation.
    look "horizon": the same eye looking along -z with a wide lens instead: sky above the horizon, floor below it."""
    floor = _quad((-4.0, 0.0, 4.0), (4.0, 0.0, 4.0), (4.0, 0.0, -4.0), (-4.0, 0.0, -4.0), 0)
    hidden = MeshDesc(vertices=np.array([(-0.5, -1.0, 0.5), (0.5, -1.0, 0.5), (0.0, -1.0, -0.5)], np.float32), faces=np.array([[0, 1, 2]], np.uint32),
                      sets=[(1, np.array([0], np.uint32))])
    mats = [diffuse(*SUN_FLOOR_RHO), emitter(0.0, 0.0, 0.0),
            MaterialDesc(lobes=[], emission=(1.0, 1.0, 1.0), emission_texture=1, emission_mapping=mapping)]
    to_world = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 1, 0, 1]], np.float32)  # -z of the camera is -y of the world; eye at (0, 1, 0)
    if look == "horizon":
        to_world = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 0, 1]], np.float32)
    elif look != "down":
        raise ValueError(f"look {look!r}: down or horizon")
    img = sun_and_sky() if image is None else image
    return SceneDesc([floor, hidden], mats, CameraDesc(width, height, 0.6 if look == "down" else 1.9, to_world), environment_material=2, name="sun_floor",
                     textures=[TextureDesc(img, abi.TEX_CLOSEST, abi.WRAP_PERIODIC, abi.WRAP_CLAMP)])


# ---- moved geometry (HipDevice.update_geometry) -----------------------------------------------------------------------------------
def _moved(scene, meshes, name):
    """a SceneDesc that shares everything of `scene` but its meshes"""
    return replace(scene, meshes=meshes, name=name)


def transformed(scene, transforms):
    """`scene` with the meshes named in `transforms` moved: {mesh index: 3 x 4 matrix [m0 m1 m2 t]} -> a new SceneDesc; the input is left alone
    and the meshes not named are shared with it.  Vertices are computed in float32 as (m0 x + m1 y) + m2 z + t, one rounding per
    operation and no contraction, so every host computes the same bits; normals by the rotation part m0 m1 m2 in the same order (a
    matrix that scales unevenly leaves them unnormalised and skewed: pass rotations, or recompute the normals)."""
    meshes = list(scene.meshes)
    for index, matrix in transforms.items():
        m = np.asarray(matrix, np.float32).reshape(3, 4)
        src = meshes[index]

        def apply(p, translate):
            out = ((p[:, 0:1] * m[None, :, 0]).astype(np.float32) + (p[:, 1:2] * m[None, :, 1]).astype(np.float32)).astype(np.float32)
            out = (out + (p[:, 2:3] * m[None, :, 2]).astype(np.float32)).astype(np.float32)
            return (out + m[None, :, 3]).astype(np.float32) if translate else out
        meshes[index] = replace(src, vertices=apply(src.vertices, True), normals=apply(src.normals, False) if len(src.normals) else src.normals)
    return _moved(scene, meshes, scene.name + "+moved")


def wobbled(scene, amplitude, seed=0):
    """`scene` with every vertex of every mesh displaced by an independent offset, uniform in [-amplitude, amplitude]^3 and drawn from
    `seed` -> a new SceneDesc; the input is left alone.  Vertices shared by faces stay shared (a mesh does not tear); normals are kept."""
    rng = np.random.default_rng(seed)
    meshes = []
    for src in scene.meshes:
        d = rng.uniform(-amplitude, amplitude, src.vertices.shape).astype(np.float32)
        meshes.append(replace(src, vertices=(src.vertices + d).astype(np.float32)))
    return _moved(scene, meshes, scene.name + "+wobbled")
