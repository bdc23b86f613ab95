"""First-hit guides and the guided denoiser on the device (phx_dev_render_guides: csrc/guides.hip; phx_dev_denoise_guided: csrc/denoise.hip), bit for bit.

The guide film is held to a COMPOSITION of hooks that are parity-tested elsewhere: the oracle's camera rays, the device's closest hits
(phx_dev_trace), the hit primitive's face set, the mesh UVs by the header's (s, t) expression, the same frame's "normals" channel, the device's lobe
weights (phx_dev_lobe_weights), and the header's sums in numpy fp32 (tests/guides64.py).  The guided filter is held to the float64 model there."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import denoise64 as dn
import frame_cases as FC
import guides64 as gd
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = np.finfo(F).max
PHX_ERR_STATE = 4  # include/phx_xpu.h
SHAPES = [(1, 1), (7, 5), (8, 8), (9, 65), (65, 67)]  # (width, height), around the 8 x 8 block of pixels a wave owns


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


def test_the_block_is_the_one_the_shapes_were_chosen_for():
    src = open(os.path.join(ROOT, "phosphorus_mk2_amd", "csrc", "guides.hip")).read()
    assert re.search(r"GUIDE_TILE = 8\b", src)
    widths, heights = {w for w, _ in SHAPES}, {h for _, h in SHAPES}
    assert {7, 8, 9} <= widths and {8, 65} <= heights


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def _uv_quad(material, lens=False, width=24, height=16):
    """a two-triangle quad with UVs that leave [0, 1] on both sides (the wraps matter), an emitter above it in view, and open sky around both"""
    from phosphorus_mk2_amd import scenes
    quad = scenes.MeshDesc(np.array([(-1.2, -0.9, -2.5), (1.2, -0.9, -2.2), (1.2, 0.7, -2.6), (-1.2, 0.7, -2.9)], F), np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                           [(0, np.array([0, 1], np.uint32))], uvs=np.array([(-0.6, -0.3), (1.7, -0.2), (1.9, 1.4), (-0.4, 1.6)], F))
    lamp = scenes._quad((-0.5, 1.3, -2.0), (-0.5, 1.3, -3.0), (0.5, 1.3, -3.0), (0.5, 1.3, -2.0), 1)
    cam = scenes.CameraDesc(width, height, 1.5, focal_distance=2.5, aperture_radius=0.05 if lens else 0.0)
    return scenes.SceneDesc([quad, lamp], [material, scenes.emitter(3.0, 3.0, 3.0)], cam, name="uv_quad")


def _images():
    from phosphorus_mk2_amd import abi, scenes
    rng = np.random.default_rng(41)
    return [scenes.TextureDesc(rng.uniform(0.05, 1.0, (4, 4, 3)).astype(F), abi.TEX_CLOSEST, abi.WRAP_PERIODIC, abi.WRAP_CLAMP),
            scenes.TextureDesc(rng.uniform(0.05, 1.0, (5, 3, 3)).astype(F), abi.TEX_LINEAR, abi.WRAP_CLAMP, abi.WRAP_PERIODIC)]  # 3 wide, 5 high


def scene_of(name, width=None, height=None):
    from phosphorus_mk2_amd import abi, scenes
    L = scenes.LobeDesc
    size = dict(width=width, height=height) if width else {}
    if name == "cornell":
        return scenes.cornell(width or 32, height or 32)
    if name == "lens":
        s = scenes.cornell(width or 32, height or 24)
        s.camera.aperture_radius, s.camera.focal_distance = 0.08, 2.5
        return s
    if name == "textured":
        s = _uv_quad(scenes.MaterialDesc([L(abi.LOBE_DIFFUSE, (0.9, 0.8, 0.7), texture=1), L(abi.LOBE_MICROFACET, (0.3, 0.4, 0.5), xalpha=0.1, yalpha=0.1, texture=2),
                                          L(abi.LOBE_DIFFUSE, (0.05, 0.05, 0.05))]), **size)
        s.textures = _images()
        return s
    if name == "textured-lens":
        s = scene_of("textured", width, height)
        s.camera.aperture_radius = 0.05
        return s
    if name == "masked":
        s = _uv_quad(scenes.MaterialDesc([L(abi.LOBE_DIFFUSE, (0.8, 0.75, 0.7), fac_mode=abi.FAC_TEX_A, pre_weight=(0.9, 1.0, 0.8), fac_texture=2),
                                          L(abi.LOBE_MICROFACET, (0.9, 0.9, 0.9), xalpha=0.2, yalpha=0.2, fac_mode=abi.FAC_TEX_B, texture=1, fac_texture=2)]), **size)
        s.textures = _images()
        return s
    if name == "glass":
        return scenes.glass_blobs(width or 48, height or 32)
    if name == "soup":
        return scenes.soup(200, width=width or 40, height=height or 24)
    raise KeyError(name)


# ---- the composition -------------------------------------------------------------------------------------------------------------------------
def film_rays(orc, scene, spp, sample, seed):
    """the oracle's camera rays of every film pixel at one sample index -> (o, d), each (H * W, 3), row-major.  The oracle hands them out per tile
    of a multiple of 8 columns and at most 1 024 pixels; columns past the film's edge are dropped."""
    from phosphorus_mk2_amd import scenes
    W, H = scene.camera.width, scene.camera.height
    O = orc.Oracle(scenes.SceneDesc(scenes.cornell(8, 8).meshes, scenes.cornell(8, 8).materials, scene.camera), spp=spp, pps=1, depth=2)
    o = np.zeros((H, W, 3), F); d = np.zeros((H, W, 3), F)
    try:
        for x0 in range(0, W, 8):
            for y0 in range(0, H, 128):
                h, w = min(128, H - y0), min(8, W - x0)
                to, td = O.camera_rays((x0, y0, 8, h), sample, seed)
                o[y0:y0 + h, x0:x0 + w] = to.reshape(h, 8, 3)[:, :w]; d[y0:y0 + h, x0:x0 + w] = td.reshape(h, 8, 3)[:, :w]
    finally:
        O.close()
    return o.reshape(-1, 3), d.reshape(-1, 3)


def prim_tables(scene):
    """per primitive, in scene_t::triangles() order (mesh, face set, face): its material and its three corner UVs ((0, 0) for a mesh without UVs)"""
    from phosphorus_mk2_amd import abi
    mats, uvs = [], []
    for m in scene.meshes:
        for mat, faces in m.sets:
            for f in faces:
                mats.append(mat)
                if m.uvs is None or len(m.uvs) == 0:
                    uvs.append(np.zeros((3, 2), F))
                elif m.flags & abi.MESH_UV_PER_VERTEX:
                    uvs.append(np.asarray(m.uvs, F)[m.faces[f]])
                else:
                    uvs.append(np.asarray(m.uvs, F)[3 * f:3 * f + 3])
    return np.array(mats, np.int64), np.array(uvs, F)


def sample_albedo(dev, scene, hit, d, normals, textured):
    """the rule's albedo of one sample of every pixel from the hit records: (n, 3) f32"""
    mats, uvs = prim_tables(scene)
    n = len(d)
    albedo = np.ones((n, 3), F)
    ok = hit["hit"]
    prim = np.where(ok, hit["prim"], 0).astype(np.int64)
    u, v = hit["u"], hit["v"]
    w = (F(1) - u) - v
    c = uvs[prim]  # header: st = (w * uv0 + u * uv1) + v * uv2, fp32, in this order
    st = ((w[:, None] * c[:, 0] + u[:, None] * c[:, 1]).astype(F) + (v[:, None] * c[:, 2]).astype(F)).astype(F)
    wi = (-d).astype(F)
    for mi, mat in enumerate(scene.materials):
        sel = ok & (mats[prim] == mi)
        if not sel.any() or mat.is_emitter:
            continue
        lw, kept = dev.lobe_weights(mi, normals[sel], wi[sel], st[sel] if textured else None)
        a = np.zeros((int(sel.sum()), 3), F)
        for k in range(lw.shape[1]):  # in lobe order, from (0, 0, 0); a lobe that is not there reports zeros
            a = (a + lw[:, k]).astype(F)
        albedo[sel] = a
    return albedo


def composed_guides(xpu, orc, dev, scene, spp, G, seed, normals=None):
    """the guide film of `scene` by the composition: -> (H, W, 8) f32.  normals: the frame's channel (H * W, 3) for G == 1, else zeros (the caller
    uses materials whose weights do not read the normal)"""
    from phosphorus_mk2_amd import abi
    W, H = scene.camera.width, scene.camera.height
    textured = any(l.texture or abi.fac_mode(l.fac_mode) >= abi.FAC_TEX_B for m in scene.materials for l in m.lobes)
    nrm = np.zeros((H * W, 3), F) if normals is None else normals
    samples = []
    for s in range(G):
        o, d = film_rays(orc, scene, spp, s, seed)
        hit = dev.trace(o, d, np.full(len(o), FLT_MAX, F))
        samples.append((sample_albedo(dev, scene, hit, d, nrm, textured), hit["hit"], o, d, hit["t"]))
    return gd.guide_sums(samples).reshape(H, W, 8)


def make_device(xpu, scene, spp):
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=spp, paths_per_sample=1, path_depth=3))
    d.preprocess(scene)
    return d


def differing(got, want):
    diff = got.view(np.uint32) != want.view(np.uint32)
    return f"{int(diff.sum())} of {diff.size} floats differ, first at {tuple(np.argwhere(diff)[0])}: {got[tuple(np.argwhere(diff)[0])]!r} != {want[tuple(np.argwhere(diff)[0])]!r}" if diff.any() else ""


# ---- 1. the guide film at G = 1 of spp = 1, with the frame's normals ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "textured", "masked", "glass", "soup", "lens", "textured-lens"])
def test_one_sample_is_the_composition(xpu, orc, name):
    scene = scene_of(name)
    W, H = scene.camera.width, scene.camera.height
    dev = make_device(xpu, scene, 1)
    try:
        frame, _ = xpu.render_on([dev], scene, seed=5, normals=True)
        got = dev.render_guides(5, 1)
        want = composed_guides(xpu, orc, dev, scene, 1, 1, 5, frame[..., 4:7].reshape(-1, 3).copy())
        st = dev.stats()
    finally:
        dev.close()
    assert got.shape == (H, W, 8)
    cov = got[..., 3]
    assert set(np.unique(cov)) <= {0.0, 1.0}
    if name != "soup":
        assert (cov == 0).any() and (cov == 1).any()  # misses and hits
    if name == "soup":
        assert st["bvh_built_on_device"] == 1  # at least 64 triangles: the device-built tree
    if name in ("textured", "masked", "textured-lens"):
        assert len(np.unique(got[..., 0][cov == 1])) > 20  # the image varies over the quad
        assert (got[..., 0:3][cov == 1] == 1.0).all(-1).any()  # the emitter is in view
    assert bits_equal(got[..., 3:8], want[..., 3:8]), "coverage / position / distance: " + differing(got[..., 3:8], want[..., 3:8])
    assert bits_equal(got[..., 0:3], want[..., 0:3]), "albedo: " + differing(got[..., 0:3], want[..., 0:3])
    assert bits_equal((frame[..., 4:7] == 0).all(-1), cov == 0)  # the frame missed where the guides missed


# ---- 2. several samples: sums in sample order, shapes around the block, host and device films ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _several(name, width, height, spp, G, seed):
    """-> (guide film by the device, by the composition, device_bytes before and after): one device per case, shared by the tests below"""
    from phosphorus_mk2_amd import xpu
    from oracle import oracle as orc
    orc.load()
    scene = scene_of(name, width, height)
    dev = make_device(xpu, scene, spp)
    try:
        before = dev.stats()["device_bytes"]
        got = dev.render_guides(seed, G)
        after = dev.stats()["device_bytes"]
        want = composed_guides(xpu, orc, dev, scene, spp, G, seed)
    finally:
        dev.close()
    got.setflags(write=False); want.setflags(write=False)
    return got, want, before, after


@pytest.mark.parametrize("spp,G", [(16, 3), (16, 16), (5, 5)])
@pytest.mark.parametrize("name", ["textured", "masked", "cornell"])
def test_several_samples_accumulate_in_sample_order(spp, G, name):
    """(5 spp is no square: the jitter table's last cell is the zero the host leaves there)"""
    got, want, before, after = _several(name, 24, 16, spp, G, 9)
    assert bits_equal(got, want), differing(got, want)
    assert before == after
    cov = np.unique(got[..., 3])
    assert name == "cornell" or len(cov) > 2  # pixels on the quad's edge are partly covered


@pytest.mark.parametrize("width,height", SHAPES)
def test_film_shapes(width, height):
    got, want, _, _ = _several("textured", width, height, 16, 3, 11)
    assert got.shape == (height, width, 8) and bits_equal(got, want), differing(got, want)


def test_device_film_repeats_and_seeds(xpu):
    scene = scene_of("textured", 9, 65)
    dev = make_device(xpu, scene, 16)
    tensor = FC.DeviceFilm(xpu, (65, 9, 8), FC.SENTINEL)
    try:
        host = dev.render_guides(11, 3)
        assert dev.render_guides(11, 3, device_ptr=tensor.ptr) is None
        assert bits_equal(tensor.numpy(), host) and bits_equal(host, _several("textured", 9, 65, 16, 3, 11)[0])
        assert bits_equal(dev.render_guides(11, 3), host)            # a repeated call is identical
        t = dev.guides_times()
        assert set(t) == {"kernel", "call"} and 0 < t["kernel"] <= t["call"]
        assert not bits_equal(dev.render_guides(12, 3), host)        # another seed: another jitter table
        assert not bits_equal(dev.render_guides(11, 4), host)
    finally:
        tensor.free()
        dev.close()


def test_a_call_the_check_refuses_leaves_film_times_and_device_alone(xpu):
    """behind a successful call, one the argument check refuses (on_device = 2): PHX_ERR_ARG with the check's text, the film bit for bit what it
    was, the times still the successful call's, and the caller's current HIP device what it was
    (On a machine with one GPU the current device is 0 before and after whatever the call does: that last assertion can fail only where
    there are several.)"""
    dev = make_device(xpu, scene_of("cornell", 8, 8), 4)
    try:
        dev.render_guides(1, 2)
        times = dev.guides_times()
        assert 0 < times["kernel"] <= times["call"]
        out = np.full((8, 8, 8), FC.SENTINEL, F)
        g = xpu.abi.Guides(sampler_seed=1, samples=2, on_device=2)
        current = FC.current_hip_device(xpu)
        rc = dev._lib.phx_dev_render_guides(dev._h, C.byref(g), out.ctypes.data)
        assert rc == 1 and dev._lib.phx_last_error().decode() == "render_guides: on_device is outside its range (phx_guides)"  # PHX_ERR_ARG
        assert bits_equal(out, np.full((8, 8, 8), FC.SENTINEL, F))
        assert dev.guides_times() == times
        assert FC.current_hip_device(xpu) == current
    finally:
        dev.close()


# ---- 3. state and memory -------------------------------------------------------------------------------------------------------------------------
def test_state_refusals_memory_and_the_next_frame(xpu):
    scene = scene_of("cornell")
    W = H = 32
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=5))
    out = np.zeros((H, W, 8), F)
    g = xpu.abi.Guides(sampler_seed=1, samples=2, on_device=0)
    try:
        rc = d._lib.phx_dev_render_guides(d._h, C.byref(g), out.ctypes.data)
        assert rc == PHX_ERR_STATE and "preprocess" in d._lib.phx_last_error().decode()
        d.preprocess(scene)
        ref, _ = xpu.render_on([d], scene, seed=1, normals=True, moments=True)
        before = d.stats()["device_bytes"]
        film = xpu.Film(W, H, 4, True, True)
        d.start(scene, xpu.FrameState(1, xpu.Tiles.make(W, H, 32), film, native_sink=True))
        rc = d._lib.phx_dev_render_guides(d._h, C.byref(g), out.ctypes.data)
        msg = d._lib.phx_last_error().decode()
        d.join()
        assert rc == PHX_ERR_STATE and "frame" in msg and not out.any()
        assert bits_equal(film.data, ref)  # the frame completed as ever
        guides = d.render_guides(1, 2)
        assert d.stats()["device_bytes"] == before
        for samples, field in ((0, "samples"), (5, "samples")):
            with pytest.raises(xpu.DeviceError, match=field):
                d.render_guides(1, samples)
        again, _ = xpu.render_on([d], scene, seed=1, normals=True, moments=True)
        assert bits_equal(again, ref) and d.stats()["device_bytes"] == before  # the next frame's bits are unchanged
        # and the guided call holds nothing either
        d.denoise(ref, 4, 4, True, False, guides=guides, plane=True)
        assert d.stats()["device_bytes"] == before
    finally:
        d.close()


# ---- 4. the guided filter against the model ------------------------------------------------------------------------------------------------------
SPP = 16
PLANE_SCALE = 0.002


@pytest.fixture(scope="module")
def dev(xpu):
    """a device without a scene: the filter needs none"""
    d = xpu.HipDevice.make(xpu.Options(samples_per_pixel=SPP, paths_per_sample=1, path_depth=5))
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def case(width, height, flags, pc=4, adaptive=True, iterations=5, gstride=8):
    """-> (film, offsets, guides, the model's answer), read-only and shared"""
    film, offs = dn.synthetic_film(height, width, pc, True, adaptive, SPP)
    guides = gd.synthetic_guides(height, width, xstride=gstride)
    want = gd.denoise(film, SPP, *offs, iterations=iterations, guides=guides, flags=flags, albedo_floor=0.01, sigma_x=1.0, plane_scale=PLANE_SCALE)
    for a in (film, guides, want):
        a.setflags(write=False)
    return film, offs, guides, want


def check(got, film, offs, want, what):
    """primary and m2 bit for bit the model's; every other float the input's"""
    no, mo, so = offs
    ours = [0, 1, 2, mo, mo + 1, mo + 2]
    rest = [c for c in range(film.shape[-1]) if c not in ours]
    assert got.shape == film.shape
    assert bits_equal(got[..., ours], want[..., ours]), f"{what}: " + differing(got[..., ours], want[..., ours])
    assert bits_equal(got[..., rest], film[..., rest]), f"{what}: a float outside primary and m2 changed"


def guided(dev, film, guides, flags, pc=4, adaptive=True, **kw):
    return dev.denoise(film, SPP, pc, True, adaptive, guides=guides, demodulate=bool(flags & 1), plane=bool(flags & 2), albedo_floor=0.01, sigma_x=1.0,
                       plane_scale=PLANE_SCALE, **kw)


def test_the_synthetic_guides_reach_every_branch():
    film, offs, guides, want = case(65, 67, 3)
    cov = guides[..., 3]
    assert (cov == 0).any() and (cov == 1).any() and ((cov > 0) & (cov < 1)).any() and (~np.isfinite(guides)).any(-1).sum() == 2
    assert ((cov > 0) & (guides[..., 7] == 0)).any() and (guides[..., 0:3] < 0.01).any()
    C_, V, N, valid, _ = gd.init_state(film, guides, 3, SPP, *offs, 0.01)
    weights = []
    gd.iterate(C_, V, N, valid, 1, 4.0, 7, guides, np.float64(F(1.0)) * np.float64(F(PLANE_SCALE)), weights)
    w = np.stack([np.where(ok, wt, np.nan) for dy, dx, ok, wt in weights if (dy, dx) != (0, 0)])
    assert (w == 0).any() and (w > 0.01).any()
    unguided = dn.denoise(film, SPP, *offs)
    for flags in (1, 2, 3):
        assert not bits_equal(case(65, 67, flags)[3][..., 0:3], unguided[..., 0:3])  # every flag changes the answer here


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("width,height", SHAPES)
def test_shapes_and_flags(dev, width, height, flags):
    film, offs, guides, want = case(width, height, flags)
    check(guided(dev, film, guides, flags), film, offs, want, f"{width} x {height}, flags {flags}")


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("iterations", [0, 1, 2, 5])
def test_iterations(dev, iterations, flags):
    film, offs, guides, want = case(9, 65, flags, iterations=iterations)
    check(guided(dev, film, guides, flags, iterations=iterations), film, offs, want, f"{iterations} iterations, flags {flags}")
    if iterations == 0:
        assert bits_equal(want, film)


@pytest.mark.parametrize("pc", [3, 4])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("flags", [1, 3])
def test_layouts_and_a_wider_guide_film(dev, pc, adaptive, flags):
    film, offs, guides, want = case(37, 29, flags, pc, adaptive, gstride=11)
    check(guided(dev, film, guides, flags, pc, adaptive), film, offs, want, f"{pc} components, adaptive {adaptive}, flags {flags}")


def test_flags_zero_and_null_guides_are_the_unguided_call(xpu, dev):
    film, offs, guides, _ = case(65, 67, 3)
    plain = dev.denoise(film, SPP, 4, True, True)
    check(plain, film, offs, dn.denoise(film, SPP, *offs), "unguided")
    assert bits_equal(guided(dev, film, guides, 0), plain)
    q = xpu.denoise_settings(film.shape, SPP, 4, True, True)
    out = np.zeros_like(film)
    assert dev._lib.phx_dev_denoise_guided(dev._h, C.byref(q), None, film.ctypes.data, out.ctypes.data) == 0
    assert bits_equal(out, plain)
    garbage = xpu.abi.DenoiseGuides(guides=0, xstride=0, flags=0, albedo_floor=float("nan"), sigma_x=-1.0, plane_scale=0.0)
    garbage.reserved[2] = 7  # flags == 0: nothing else of the struct is read
    out[:] = 0
    assert dev._lib.phx_dev_denoise_guided(dev._h, C.byref(q), C.byref(garbage), film.ctypes.data, out.ctypes.data) == 0
    assert bits_equal(out, plain)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("in_place", [False, True])
def test_host_and_device_films_in_and_out_of_place(xpu, dev, on_device, in_place):
    """straight through the C ABI: films and guides all host or all device memory, film_out == film_in or another film (prefilled with a sentinel)"""
    film, offs, guides, want = case(65, 67, 3)
    q = xpu.denoise_settings(film.shape, SPP, 4, True, True)
    q.on_device = on_device
    lib = dev._lib
    g = xpu.abi.DenoiseGuides(xstride=8, flags=3, albedo_floor=0.01, sigma_x=1.0, plane_scale=PLANE_SCALE)
    if on_device:
        src = FC.DeviceFilm(xpu, film.shape, film); gdev = FC.DeviceFilm(xpu, guides.shape, guides)
        dst = src if in_place else FC.DeviceFilm(xpu, film.shape, FC.SENTINEL)
        try:
            g.guides = gdev.ptr
            rc = lib.phx_dev_denoise_guided(dev._h, C.byref(q), C.byref(g), src.ptr, dst.ptr)
            assert rc == 0, lib.phx_last_error()
            got = dst.numpy()
            assert bits_equal(gdev.numpy(), guides)
            if not in_place:
                assert bits_equal(src.numpy(), film)  # film_in is read only
        finally:
            src.free(); dst.free(); gdev.free()
    else:
        a = film.copy(); gh = guides.copy()
        b = a if in_place else np.full(film.shape, FC.SENTINEL, F)
        g.guides = gh.ctypes.data
        rc = lib.phx_dev_denoise_guided(dev._h, C.byref(q), C.byref(g), a.ctypes.data, b.ctypes.data)
        assert rc == 0, lib.phx_last_error()
        got = b
        assert bits_equal(gh, guides) and (in_place or bits_equal(a, film))
    check(got, film, offs, want, f"on_device {on_device}, in place {in_place}")


def test_refusals_reach_the_caller(xpu, dev):
    film, offs, guides, _ = case(7, 5, 3)
    for kw, field in ((dict(albedo_floor=0.0), "albedo_floor"), (dict(plane=True, sigma_x=0.0, plane_scale=PLANE_SCALE), "sigma_x"), (dict(plane=True, plane_scale=-1.0), "plane_scale")):
        with pytest.raises(xpu.DeviceError, match=field):
            dev.denoise(film, SPP, 4, True, True, guides=guides, **kw)
    with pytest.raises(xpu.DeviceError, match="xstride"):
        dev.denoise(film, SPP, 4, True, True, guides=guides[..., :7])
    with pytest.raises(ValueError, match="plane_scale"):
        dev.denoise(film, SPP, 4, True, True, guides=guides, plane=True)  # no scene on this device, and no plane_scale given
    no_normals, offs2 = dn.synthetic_film(5, 7, 4, False, True, SPP)
    with pytest.raises(xpu.DeviceError, match="normals_offset"):
        dev.denoise(no_normals, SPP, 4, False, True, guides=guides, plane=True, plane_scale=PLANE_SCALE)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
RENDER = dict(spp=8, depth=4, normals=True, moments=True, seed=3)


@pytest.mark.parametrize("plane", [False, True])
def test_render_with_guides_is_the_model_on_the_plain_render(xpu, plane):
    scene = scene_of("textured")
    plain, st0 = xpu.render(scene, **RENDER)
    got, st1 = xpu.render(scene, denoise=dict(guides=dict(samples=4, plane=plane)), **RENDER)
    dev = make_device(xpu, scene, 8)
    try:
        guides = dev.render_guides(3, 4)
    finally:
        dev.close()
    xstride, no, mo, so = dn.layout(4, True, False)
    want = gd.denoise(plain, 8, no, mo, so, guides=guides, flags=1 | (2 if plane else 0), albedo_floor=0.01, sigma_x=1.0,
                      plane_scale=xpu.guide_plane_scale(scene.camera))
    check(got, plain, (no, mo, so), want, f"render(denoise=dict(guides=...)), plane {plane}")
    assert not bits_equal(got[..., 0:3], plain[..., 0:3])
    assert not bits_equal(got[..., 0:3], dn.denoise(plain, 8, no, mo, so)[..., 0:3])
    assert st0["camera_samples"] == st1["camera_samples"] and st0["rays_closest"] == st1["rays_closest"]


def test_the_c_example_with_the_guided_keyword(xpu, tmp_path):
    """examples/render_room.c denoise-guided: it writes the model's film of the frame it always rendered"""
    from test_gpu_parity import _room_scene
    exe = os.path.join(ROOT, "examples", "render_room")
    if not os.path.exists(exe):
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "examples")], check=True)
    out = str(tmp_path / "room.f32")
    r = subprocess.run([exe, out, "host-bvh", "denoise-guided"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    film = np.fromfile(out, F).reshape(96, 128, 4)
    scene = _room_scene()
    plain, _ = xpu.render(scene, spp=8, pps=1, depth=5, seed=7, native_sink=True, bvh_builder="host", moments=True)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=8, paths_per_sample=1, path_depth=5, bvh_builder="host"))
    try:
        dev.preprocess(scene)
        guides = dev.render_guides(7, 4)
    finally:
        dev.close()
    want = gd.denoise(plain, 8, 0, 4, 0, guides=guides, flags=1, albedo_floor=0.01)
    assert bits_equal(film, want[..., :4]) and not bits_equal(film, plain[..., :4])
    assert re.search(r"denoise-guided: 4 guide samples", r.stdout)
