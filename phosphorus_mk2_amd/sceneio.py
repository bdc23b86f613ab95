"""Scene ingestion: the reference's YAML scene file (src/codecs/scene.cpp:41-76) with the
same top-level keys — `materials` (shader graphs, baked by closures.py), `data` (geometry files), `camera`,
`world.environment` — feeding the same `scene -> preprocess` step as the synthetic scenes.

Differences, by necessity: geometry comes from Wavefront OBJ instead of Alembic (`.abc` needs the Alembic library,
absent here); the camera block is completed into a look-at matrix (the reference's YAML camera decoder reads
position/at/up and then drops them, src/codecs/scene/entities.hpp:18-33) with the Alembic importer's convention
`fov = 2*atan2(sensor_width/2, focal_length)` (src/codecs/scene/alembic.hpp:69); an optional `dof: {fstop, focus-distance}` block
turns the thin lens on with the Blender importer's convention (plugins/blender/import.hpp:573-579).

OBJ subset: v, vt, vn, f (polygons are fan-triangulated; v, v/vt, v//vn and v/vt/vn index forms), usemtl NAME (one face set per
material, material ids = order of the YAML `materials` map, src/scene.cpp:84-90), `s off|0` / `s 1` (flat / smooth).  UVs are
per vertex when every corner's vt index is its v index, per face corner otherwise (mesh_t::flags_t UVPerVertex, src/mesh.hpp:20-23);
a corner without vt has UV (0, 0).

Image textures (texture_node, baked by closures.py): `filename` is resolved relative to the YAML file and read with numpy alone —
binary PPM (P6, 8 bit, value / 255), PFM (rows flipped to top first), Radiance `.hdr` (RGBE, flat or new-style run-length scanlines,
`-Y H +X W` only) or `.npy` ((H, W, 3) or (H, W) float) — as linear RGB.

Textured emitters (texture_node into a diffuse_emitter_node's Cs) load only with `load_scene(..., emitter_textures=True)`: the image
multiplies the emission at the mesh's UVs (phx_material.emission_uv_texture).

Environment maps (environment_node into the world material's background_node.Cs): `world: {environment: <material>, environment-up: y|z}`
selects OpenImageIO's lat-long layout with +y (the default) or +z up (phx_material.emission_mapping).
"""
import math
import os

import numpy as np
import yaml

from . import abi, closures
from .scenes import CameraDesc, MeshDesc, SceneDesc, TextureDesc


def load_obj(path, material_ids, default_material=0):
    verts, norms, texco, faces, fnorm, fuv, smooth, fmat = [], [], [], [], [], [], [], []
    cur_mat, cur_smooth = default_material, False
    for line in open(path):
        t = line.split()
        if not t or t[0].startswith("#"):
            continue
        if t[0] == "v":
            verts.append([float(x) for x in t[1:4]])
        elif t[0] == "vn":
            norms.append([float(x) for x in t[1:4]])
        elif t[0] == "vt":
            texco.append([float(x) for x in t[1:3]] + [0.0] * (3 - len(t)))
        elif t[0] == "usemtl":
            if t[1] not in material_ids:
                raise ValueError(f"{path}: usemtl {t[1]!r} is not in the scene's materials")
            cur_mat = material_ids[t[1]]
        elif t[0] == "s":
            cur_smooth = t[1] not in ("off", "0")
        elif t[0] == "f":
            idx = []
            for tok in t[1:]:
                p = tok.split("/")
                vi = int(p[0]); vi = vi - 1 if vi > 0 else len(verts) + vi
                ti = ni = None
                if len(p) >= 2 and p[1]:
                    ti = int(p[1]); ti = ti - 1 if ti > 0 else len(texco) + ti
                    if not 0 <= ti < len(texco):
                        raise ValueError(f"{path}: vt index {p[1]} out of range")
                if len(p) == 3 and p[2]:
                    ni = int(p[2]); ni = ni - 1 if ni > 0 else len(norms) + ni
                idx.append((vi, ni, ti))
            for k in range(1, len(idx) - 1):
                tri = (idx[0], idx[k], idx[k + 1])
                faces.append([v for v, _, _ in tri])
                fnorm.append([n for _, n, _ in tri])
                fuv.append([u for _, _, u in tri])
                smooth.append(1 if (cur_smooth and all(n is not None for _, n, _ in tri)) else 0)
                fmat.append(cur_mat)
    if not faces:
        raise ValueError(f"{path}: no faces")
    faces = np.array(faces, np.uint32)
    verts = np.array(verts, np.float32)
    fmat = np.array(fmat)
    # normals per face corner (mesh_t without NormalsPerVertex, src/mesh.cpp:188-192): index 3*face + corner
    nrm = np.zeros((len(faces) * 3, 3), np.float32)
    na = np.array(norms, np.float32) if norms else np.zeros((0, 3), np.float32)
    for f, tri in enumerate(fnorm):
        for c, n in enumerate(tri):
            if n is not None:
                nrm[3 * f + c] = na[n]
    sets = [(int(m), np.nonzero(fmat == m)[0].astype(np.uint32)) for m in sorted(set(fmat.tolist()))]
    # UVs: per vertex when the file indexes them like the positions (every corner's vt index is its v index), per face corner otherwise
    flags, uvs = abi.MESH_UV_PER_VERTEX, None
    if texco:
        ta = np.array(texco, np.float32)
        corner_uv = [u for tri in fuv for u in tri]
        corner_v = faces.reshape(-1).tolist()
        if len(ta) == len(verts) and all(u == v for u, v in zip(corner_uv, corner_v)):
            uvs = ta
        else:
            flags = 0
            uvs = np.zeros((len(corner_uv), 2), np.float32)
            for c, u in enumerate(corner_uv):
                if u is not None:
                    uvs[c] = ta[u]
    return MeshDesc(vertices=verts, faces=faces, normals=nrm, smooth=np.array(smooth, np.uint8), sets=sets, flags=flags, uvs=uvs)


def _ppm_tokens(data, n):
    """the first n whitespace-separated header tokens of a PNM file (comments skipped) and the offset right behind the last one"""
    toks, i = [], 0
    while len(toks) < n:
        while i < len(data) and data[i:i + 1].isspace():
            i += 1
        if data[i:i + 1] == b"#":
            while i < len(data) and data[i:i + 1] not in (b"\n", b"\r"):
                i += 1
            continue
        j = i
        while j < len(data) and not data[j:j + 1].isspace():
            j += 1
        if j == i:
            raise ValueError("truncated PPM header")
        toks.append(data[i:j]); i = j
    return toks, i + 1  # one whitespace character separates the header from the raster


def load_ppm(path):
    """binary PPM (P6) with 8-bit samples -> (H, W, 3) float32 value / 255, row 0 = the top row"""
    data = open(path, "rb").read()
    (magic, w, h, maxval), off = _ppm_tokens(data, 4)
    w, h, maxval = int(w), int(h), int(maxval)
    if magic != b"P6" or maxval != 255:
        raise ValueError(f"{path}: only binary 8-bit PPM (P6, maxval 255) is supported")
    raster = np.frombuffer(data, np.uint8, count=w * h * 3, offset=off)
    return (raster.astype(np.float32) / np.float32(255.0)).reshape(h, w, 3)


def load_pgm(path):
    """greyscale PGM, binary (P5) or plain (P2), maxval up to 65535 (P5: 16-bit samples are big-endian) -> (H, W, 3) float32 value /
    maxval replicated to RGB, row 0 = the top row: what a mask is usually painted as"""
    data = open(path, "rb").read()
    (magic, w, h, maxval), off = _ppm_tokens(data, 4)
    if magic not in (b"P2", b"P5"):
        raise ValueError(f"{path}: only greyscale PGM (P2, P5) is supported")
    w, h, maxval = int(w), int(h), int(maxval)
    if w <= 0 or h <= 0 or not 0 < maxval < 65536:
        raise ValueError(f"{path}: bad PGM header")
    if magic == b"P5":
        dt = np.uint8 if maxval < 256 else np.dtype(">u2")
        if len(data) - off < w * h * np.dtype(dt).itemsize:
            raise ValueError(f"{path}: truncated PGM raster")
        raster = np.frombuffer(data, dt, count=w * h, offset=off)
    else:
        vals = [t for line in data[off - 1:].split(b"\n") for t in line.split(b"#")[0].split()]
        if len(vals) < w * h:
            raise ValueError(f"{path}: truncated PGM raster")
        raster = np.array([int(t) for t in vals[:w * h]], np.int64)
    grey = (raster.astype(np.float32) / np.float32(maxval)).reshape(h, w)
    return np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))


def load_pfm(path):
    """PFM (PF: RGB, Pf: grey) -> (H, W, 3) float32, row 0 = the top row (the file stores the bottom row first)"""
    data = open(path, "rb").read()
    (magic, w, h, scale), off = _ppm_tokens(data, 4)
    w, h, scale = int(w), int(h), float(scale)
    if magic not in (b"PF", b"Pf"):
        raise ValueError(f"{path}: not a PFM file")
    c = 3 if magic == b"PF" else 1
    img = np.frombuffer(data, "<f4" if scale < 0 else ">f4", count=w * h * c, offset=off).astype(np.float32).reshape(h, w, c)
    img = img[::-1]
    return np.ascontiguousarray(np.repeat(img, 3, axis=2) if c == 1 else img)


def load_hdr(path):
    """Radiance picture (#?RADIANCE / #?RGBE, FORMAT=32-bit_rle_rgbe, resolution line `-Y H +X W`) -> (H, W, 3) float32, row 0 = the
    file's first scanline.  Scanlines are flat RGBE or new-style run-length encoded (per component; runs of count - 128 copies, else count
    literal bytes); old-style runs, other formats and orientations raise.  Decoding is Radiance's colr_color: (m + 0.5) * 2^(e - 136)
    per channel, and e = 0 is black."""
    data = open(path, "rb").read()
    lines, i = [], 0
    while True:  # header lines up to the first empty one
        j = data.find(b"\n", i)
        if j < 0:
            raise ValueError(f"{path}: truncated Radiance header")
        line = data[i:j].rstrip(b"\r"); i = j + 1
        if not line:
            break
        lines.append(line)
    if not lines or lines[0] not in (b"#?RADIANCE", b"#?RGBE"):
        raise ValueError(f"{path}: not a Radiance picture (#?RADIANCE / #?RGBE)")
    for line in lines[1:]:
        if line.startswith(b"FORMAT=") and line[7:].strip() != b"32-bit_rle_rgbe":
            raise ValueError(f"{path}: format {line[7:].decode(errors='replace')!r} is not supported (32-bit_rle_rgbe)")
    j = data.find(b"\n", i)
    res = data[i:j if j >= 0 else len(data)].split()
    if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X" or not res[1].isdigit() or not res[3].isdigit():
        raise ValueError(f"{path}: resolution {data[i:j].decode(errors='replace')!r}: only '-Y H +X W' is supported")
    H, W = int(res[1]), int(res[3])
    if H == 0 or W == 0 or j < 0:
        raise ValueError(f"{path}: empty or truncated picture")
    buf = np.frombuffer(data, np.uint8, offset=j + 1)
    out = np.zeros((H, W, 4), np.uint8)
    p = 0
    for y in range(H):
        if 8 <= W <= 0x7fff and p + 4 <= len(buf) and buf[p] == 2 and buf[p + 1] == 2 and buf[p + 2] < 128:
            if (int(buf[p + 2]) << 8 | int(buf[p + 3])) != W:
                raise ValueError(f"{path}: scanline {y}: run-length length does not match the width")
            p += 4
            for c in range(4):
                x = 0
                while x < W:
                    if p >= len(buf):
                        raise ValueError(f"{path}: truncated scanline {y}")
                    n = int(buf[p]); p += 1
                    if n > 128:
                        n -= 128
                        if x + n > W or p >= len(buf):
                            raise ValueError(f"{path}: scanline {y}: bad run")
                        out[y, x:x + n, c] = buf[p]; p += 1
                    else:
                        if n == 0 or x + n > W or p + n > len(buf):
                            raise ValueError(f"{path}: scanline {y}: bad literal run")
                        out[y, x:x + n, c] = buf[p:p + n]; p += n
                    x += n
        else:
            if p + 4 * W > len(buf):
                raise ValueError(f"{path}: truncated scanline {y}")
            row = buf[p:p + 4 * W].reshape(W, 4)
            if ((row[:, 0] == 1) & (row[:, 1] == 1) & (row[:, 2] == 1)).any():
                raise ValueError(f"{path}: scanline {y}: old-style run-length encoding is not supported")
            out[y] = row; p += 4 * W
    e = out[..., 3].astype(np.int64)
    f = np.where(e == 0, 0.0, np.ldexp(1.0, e - 136))
    return ((out[..., :3].astype(np.float64) + 0.5) * f[..., None]).astype(np.float32)


def load_image(path):
    """a texture's texels by the file's extension: .ppm, .pgm (grey, replicated to RGB), .pfm (PF, or Pf grey), .hdr or .npy"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".hdr":
        return load_hdr(path)
    if ext == ".ppm":
        return load_ppm(path)
    if ext == ".pgm":
        return load_pgm(path)
    if ext == ".pfm":
        return load_pfm(path)
    if ext == ".npy":
        a = np.load(path).astype(np.float32)
        if a.ndim == 2:
            a = np.repeat(a[:, :, None], 3, axis=2)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{path}: expected an (H, W, 3) or (H, W) array, not {a.shape}")
        return np.ascontiguousarray(a)
    raise ValueError(f"{path}: unsupported image format {ext!r} (.ppm, .pgm, .pfm, .hdr, .npy)")


def look_at(position, at, up):
    """camera-to-world in Imath's row-vector convention (v' = v * M): the camera looks down -z, +y is up (camera.hpp:86-88)"""
    p, a, u = (np.asarray(x, np.float64) for x in (position, at, up))
    z = p - a; z /= np.linalg.norm(z)
    x = np.cross(u, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3], m[3, :3] = x, y, z, p
    return m.astype(np.float32)


def load_scene(path, width=1280, height=720, emitter_textures=False):
    """emitter_textures: bake texture_node.Cout -> diffuse_emitter_node.Cs into MaterialDesc.emission_uv_texture (closures.bake_material);
    such a graph is refused by default."""
    cfg = yaml.safe_load(open(path))
    base = os.path.dirname(os.path.abspath(path))
    tex_specs = []
    baked = closures.bake_materials(cfg["materials"], tex_specs, emitter_textures)
    textures = [TextureDesc(load_image(os.path.join(base, t["filename"])), abi.TEX_LINEAR, t["swrap"], t["twrap"]) for t in tex_specs]
    names = list(baked)
    ids = {n: i for i, n in enumerate(names)}
    meshes = [load_obj(os.path.join(base, d["path"]), ids, ids.get(d.get("material", names[0]), 0)) for d in cfg.get("data", [])]
    cam = cfg.get("camera", {}) or {}
    focal, sensor = float(cam.get("focal-length", 35.0)), float(cam.get("sensor-width", 32.0))
    fov = 2.0 * math.atan2(sensor / 2.0, focal)
    to_world = look_at(cam.get("position", (0, 0, 0)), cam.get("at", (0, 0, -1)), cam.get("up", (0, 1, 0)))
    film = cam.get("film", {}) or {}
    camera = CameraDesc(int(film.get("width", width)), int(film.get("height", height)), fov, to_world)
    dof = cam.get("dof") or {}
    if dof:  # the Blender importer's depth of field (plugins/blender/import.hpp:573-579): focal length in mm, radius = lens / (2 f-stop) in m
        fstop = max(float(dof.get("fstop", 2.8)), 1e-5)
        camera.aperture_radius = (focal * 1e-3) / (2.0 * fstop)
        camera.focal_distance = float(dof.get("focus-distance", 1.0))
    env = -1
    world = cfg.get("world") or {}
    if "environment" in world:
        env = ids[world["environment"]]  # import_world_data, scene.cpp:30-36
    up = str(world.get("environment-up", "y"))
    if up not in ("y", "z"):
        raise ValueError(f"{path}: world environment-up {up!r}: y or z")
    mats = [baked[n] for n in names]
    for i, m in enumerate(mats):
        if m.emission_texture and i != env:
            raise ValueError(f"{path}: material {names[i]!r} has an environment map but is not the world's environment")
        if m.emission_uv_texture and i == env:
            raise ValueError(f"{path}: material {names[i]!r} has a textured emitter but is the world's environment (use an environment_node)")
    if env >= 0:
        mats[env].emission_mapping = abi.ENV_LATLONG_Z_UP if up == "z" else abi.ENV_LATLONG_Y_UP
    return SceneDesc(meshes, mats, camera, environment_material=env, name=os.path.basename(path), textures=textures)


def save_pfm(path, rgb):
    """film sink to disk (the reference writes EXR through OpenImageIO, src/film/file.cpp:43-46; PFM needs no library)"""
    img = np.ascontiguousarray(rgb[::-1, :, :3], np.float32)
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def save_ppm(path, image):
    """an 8-bit image (H, W, 3 or 4) uint8, as HipDevice.display returns it, as binary PPM (P6); alpha is dropped.  load_ppm reads it back."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError("save_ppm: the image must be (height, width, 3 or 4) uint8")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img[:, :, :3]).tobytes())


def save_exr(path, film):
    """film::file_t::finalize (src/film/file.cpp:27-46) writes the 4-component float image as OpenEXR through OpenImageIO;
    this writes the same image as an uncompressed scanline OpenEXR 2 file (FLOAT channels A, B, G, R; a film without
    alpha gets A = 1) with nothing but numpy.  `film`: H x W x (3|4+) float32, row 0 = top row."""
    import struct
    img = np.asarray(film, np.float32)
    h, w = img.shape[:2]
    planes = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2],
              "A": img[..., 3] if img.shape[2] >= 4 else np.ones((h, w), np.float32)}
    names = sorted(planes)  # the channel list is sorted by name and so is the data of a scanline

    def attr(name, typ, value):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", 2, 0, 1, 1) for n in names) + b"\0"  # 2 = FLOAT
    box = struct.pack("<iiii", 0, 0, w - 1, h - 1)
    header = (struct.pack("<ii", 20000630, 2) + attr("channels", "chlist", chlist) + attr("compression", "compression", b"\0") +
              attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") +
              attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) +
              attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")
    row_bytes = 4 * w * len(names)
    first = len(header) + 8 * h
    offsets = first + (8 + row_bytes) * np.arange(h, dtype=np.uint64)
    rows = np.stack([np.ascontiguousarray(planes[n], "<f4") for n in names], axis=1)  # h x channels x w
    with open(path, "wb") as f:
        f.write(header)
        f.write(offsets.astype("<u8").tobytes())
        for y in range(h):
            f.write(struct.pack("<ii", y, row_bytes))
            f.write(rows[y].tobytes())
