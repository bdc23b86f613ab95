"""Environment maps on the device (k_shade_g<.., ENV>, phx_dev_environment_lookup).  The oracle knows only a constant environment: the
device's lookup is compared with the float64 numpy restatement below (sharing no code with the device), and films with environment
images with the oracle's films of scenes whose constant environment is what the image must give there."""
import copy

import numpy as np
import pytest

from conftest import aim_camera, bits_equal
from test_gpu_textures import grid_box, np_lookup

pytestmark = pytest.mark.gpu

F = np.float32
INV_2PI, INV_PI = float.fromhex("0x1.45f306dc9c883p-3"), float.fromhex("0x1.45f306dc9c883p-2")  # the doubles nearest 1/(2 pi), 1/pi


@pytest.fixture(scope="module")
def xpu():
    from phosphorus_mk2_amd import xpu
    xpu.load_library()
    return xpu


# ---- numpy restatement (include/phx_xpu.h: phx_material.emission_texture) --------------------------------------------------------------
def np_env_st(dirs, mapping):
    """(s, t) in float64 from the fp32 components, operation by operation, each rounded to fp32 once; ok = a finite, non-zero direction"""
    from phosphorus_mk2_amd import abi
    d = np.asarray(dirs, F).reshape(-1, 3)
    x, y, z = (d[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore"):
        if mapping == abi.ENV_LATLONG_Z_UP:
            s = 0.5 + np.arctan2(y, x) * INV_2PI
            t = 0.5 - np.arctan2(z, np.sqrt(x * x + y * y)) * INV_PI
        else:
            s = 0.5 + np.arctan2(-x, z) * INV_2PI
            t = 0.5 - np.arctan2(y, np.sqrt(z * z + x * x)) * INV_PI
    ok = np.isfinite(d).all(1) & (d != 0).any(1)
    return np.stack([np.where(ok, s, 0.0), np.where(ok, t, 0.0)], 1).astype(F), ok


def np_env(tex, emission, mapping, dirs):
    st, ok = np_env_st(dirs, mapping)
    c = np_lookup(tex, st)
    return np.where(ok[:, None], np.asarray(emission, F)[None, :] * c, F(0)).astype(F)


def _with_env(sc, img, emission=(1.0, 1.0, 1.0), mapping=0, filt=None, swrap=None, twrap=None):
    """sc plus an environment material whose image is `img` (appended to sc.textures)"""
    from phosphorus_mk2_amd import abi, scenes
    sc = copy.deepcopy(sc)
    sc.textures = list(sc.textures) + [scenes.TextureDesc(img, abi.TEX_LINEAR if filt is None else filt,
                                                          abi.WRAP_PERIODIC if swrap is None else swrap, abi.WRAP_CLAMP if twrap is None else twrap)]
    sc.materials.append(scenes.MaterialDesc([], tuple(emission), emission_texture=len(sc.textures), emission_mapping=mapping))
    sc.environment_material = len(sc.materials) - 1
    return sc


def _with_constant_env(sc, e):
    from phosphorus_mk2_amd import scenes
    sc = copy.deepcopy(sc)
    sc.materials.append(scenes.MaterialDesc([], tuple(float(x) for x in np.asarray(e, F))))
    sc.environment_material = len(sc.materials) - 1
    return sc


def open_box(width=32, height=32):
    """the open-top Cornell box of test_gpu_parity.py::test_normals_channel_and_env_light (no ceiling; the front is open too)"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell(width, height)
    sc.meshes = sc.meshes[:1] + sc.meshes[2:]
    return sc


# ---- 1. the lookup ------------------------------------------------------------------------------------------------------------------------
def _directions(mapping, n=100_000, seed=0):
    from phosphorus_mk2_amd import abi
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * np.exp(rng.uniform(-30, 30, (n, 1)))
    axes = np.concatenate([np.eye(3), -np.eye(3), 2.5 * np.eye(3)])
    if mapping == abi.ENV_LATLONG_Z_UP:  # the s seam is y = +-0 with x < 0; the poles are +-z
        seam = [(-1, 0.0, 0.3), (-1, -0.0, 0.3), (-1, 0.0, 0), (-1, -0.0, 0), (-2, 1e-30, -0.5), (-2, -1e-30, -0.5), (-1, 1e-7, 0), (-1, -1e-7, 0)]
        poles = [(0, 0, 1), (0, 0, -1), (1e-30, 0, 1), (0, -1e-30, -1), (1e-8, 1e-8, 1)]
    else:  # the s seam is x = +-0 with z < 0; the poles are +-y
        seam = [(0.0, 0.3, -1), (-0.0, 0.3, -1), (0.0, 0, -1), (-0.0, 0, -1), (1e-30, -0.5, -2), (-1e-30, -0.5, -2), (1e-7, 0, -1), (-1e-7, 0, -1)]
        poles = [(0, 1, 0), (0, -1, 0), (1e-30, 1, 0), (0, -1, -1e-30), (1e-8, 1, 1e-8)]
    bad = [(0, 0, 0), (-0.0, 0, -0.0), (np.nan, 1, 0), (0, np.inf, 0), (1, 0, -np.inf), (np.nan, np.nan, np.nan), (3e38, 3e38, 0), (1e-30, 0, 0)]
    return np.concatenate([d, axes, np.array(seam + poles + bad, np.float64)]).astype(F)


@pytest.mark.parametrize("mapping", [0, 1])
def test_lookup_is_bit_equal_to_the_restatement(xpu, mapping):
    from phosphorus_mk2_amd import abi
    rng = np.random.default_rng(3 + mapping)
    images = [rng.uniform(0.0, 4.0, (5, 11, 3)).astype(F), rng.uniform(0.0, 1.0, (16, 7, 3)).astype(F), rng.uniform(0.0, 9.0, (1, 3, 3)).astype(F)]
    emission = (0.75, 2.0, 1.3)
    dirs = _directions(mapping)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=2))
    try:
        for img in images:
            for filt in (abi.TEX_LINEAR, abi.TEX_CLOSEST):
                sc = _with_env(open_box(), img, emission, mapping, filt)
                dev.preprocess(sc)
                got = dev.environment_lookup(dirs)
                want = np_env(sc.textures[-1], emission, mapping, dirs)
                assert np.isfinite(got).all()
                assert bits_equal(got, want), (img.shape, filt, np.nonzero((got != want).any(1))[0][:10])
                assert (got[-8:] == 0).sum() >= 6 * 3  # zero and non-finite directions read black
    finally:
        dev.close()


# ---- 2. a constant image is the constant environment -----------------------------------------------------------------------------------
K = np.array([2.0, 0.5, 4.0], F)
C1 = np.array([0.3, 0.6, 0.2], F)   # K * C1 is exact in fp32 (powers of two)


def _oracle(orc, sc, spp, seed):
    return orc.Oracle(sc, spp=spp, pps=1, depth=9).render(rng=orc.RNG_COUNTER, seed=seed, threads=8)


@pytest.mark.parametrize("scene,lens,flight", [("box", False, 1), ("box", True, 4), ("glass", False, 4), ("glass", True, 1)])
def test_constant_image_equals_the_constant_environment(xpu, orc, scene, lens, flight):
    from phosphorus_mk2_amd import scenes
    base = open_box(48, 40) if scene == "box" else scenes.glass_blobs(48, 40)
    if lens:
        base.camera.aperture_radius, base.camera.focal_distance = 0.03, 3.0
    sc = _with_env(base, C1.reshape(1, 1, 3), K)
    film, st = xpu.render(sc, spp=8, pps=1, depth=9, seed=4, samples_in_flight=flight)
    ref, ost = _oracle(orc, _with_constant_env(base, K * C1), 8, 4)
    assert (st["rays_closest"], st["rays_shadow"], st["rays_masked"]) == (ost["rays_closest"], ost["rays_shadow"], ost["rays_masked"])
    assert st["shade_general"] == 1
    assert bits_equal(film[..., :3], ref[..., :3])
    plain, _ = xpu.render(base, spp=8, pps=1, depth=9, seed=4)
    assert not bits_equal(film[..., :3], plain[..., :3])  # the environment is seen


# ---- 3. an image with a region no escaping ray can take ----------------------------------------------------------------------------------
def closed_box_open_top(width=32, height=32):
    """a box around the camera (x, y in [-1, 1], z in [-3.5, 0.5]) closed on every side but the top, the Cornell lamp under the opening:
    a path can leave it only through the square at y = 1, i.e. with d.y > 0"""
    from phosphorus_mk2_amd import scenes
    q = scenes._quad
    x0, x1, y0, y1, zf, zb = -1.0, 1.0, -1.0, 1.0, 0.5, -3.5
    meshes = [q((x0, y0, zf), (x1, y0, zf), (x1, y0, zb), (x0, y0, zb), 0), q((x0, y0, zb), (x1, y0, zb), (x1, y1, zb), (x0, y1, zb), 0),
              q((x0, y0, zf), (x0, y0, zb), (x0, y1, zb), (x0, y1, zf), 1), q((x1, y0, zf), (x1, y1, zf), (x1, y1, zb), (x1, y0, zb), 2),
              q((x1, y0, zf), (x0, y0, zf), (x0, y1, zf), (x1, y1, zf), 0),
              q((-0.25, 0.99, -2.25), (-0.25, 0.99, -2.75), (0.25, 0.99, -2.75), (0.25, 0.99, -2.25), 3)]
    mats = [scenes.diffuse(0.73, 0.73, 0.73), scenes.diffuse(0.65, 0.05, 0.05), scenes.diffuse(0.12, 0.45, 0.15), scenes.emitter(*scenes.LE)]
    return scenes.SceneDesc(meshes, mats, scenes.CameraDesc(width, height, 1.9))


def test_unreachable_region_never_leaks(xpu, orc):
    from phosphorus_mk2_amd import abi
    base = closed_box_open_top()
    # no ray from inside the box with d.y <= 0 escapes: every one hits a wall (checked on 200 k rays)
    rng = np.random.default_rng(8)
    o = np.stack([rng.uniform(-0.99, 0.99, 200_000), rng.uniform(-0.99, 0.99, 200_000), rng.uniform(-3.49, 0.49, 200_000)], 1).astype(F)
    d = rng.normal(size=(200_000, 3)); d[:, 1] = -np.abs(d[:, 1]); d[:1000, 1] = 0.0
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=1, paths_per_sample=1, path_depth=9))
    try:
        dev.preprocess(base)
        h = dev.trace(o, d, np.full(len(o), np.finfo(F).max, F))
    finally:
        dev.close()
    assert h["hit"].all() and (h["t"] < 10).all()
    # Y_UP: d.y > 0 is t < 0.5; with H = 8 a LINEAR lookup there reads rows 0 .. 4 only.  Rows 5 .. 7 (below the horizon) are huge.
    img = np.broadcast_to(C1, (8, 6, 3)).copy()
    img[5:] = (1e6, 2e6, 3e6)
    for lens in (False, True):
        b = copy.deepcopy(base)
        if lens:
            b.camera.aperture_radius, b.camera.focal_distance = 0.03, 2.0
        sc = _with_env(b, img, (1.0, 1.0, 1.0), abi.ENV_LATLONG_Y_UP, abi.TEX_LINEAR)
        film, st = xpu.render(sc, spp=16, pps=1, depth=9, seed=6)
        ref, ost = _oracle(orc, _with_constant_env(b, C1), 16, 6)
        assert (st["rays_closest"], st["rays_shadow"]) == (ost["rays_closest"], ost["rays_shadow"])
        assert film[..., :3].max() < 100.0 and bits_equal(film[..., :3], ref[..., :3])


# ---- 4. what the camera sees ----------------------------------------------------------------------------------------------------------------
BW, BH = 8, 4


def _blocks():
    i, j = np.meshgrid(np.arange(BW), np.arange(BH))
    return np.stack([(i + 1) / 8.0, (j + 1) / 4.0, ((3 * i + 5 * j) % 7 + 1) / 8.0], -1).astype(F)  # 32 distinct colours, exact in fp32


def _far_geometry():
    """the Cornell box shrunk and moved 1000 units below the camera: it covers none of the views below"""
    from phosphorus_mk2_amd import scenes
    sc = scenes.cornell(32, 32)
    for m in sc.meshes:
        m.vertices = (m.vertices * F(0.5) + np.array([0, -1000, 0], F)).astype(F)
    return sc


@pytest.mark.parametrize("mapping,yaw,pitch", [(0, 0.0, 0.0), (0, 0.4, 1.5707963), (0, 2.2, -0.3), (1, 0.0, 0.0), (1, 1.5707963, 0.2), (1, -0.8, 0.5)])
def test_camera_sees_the_right_block(xpu, orc, mapping, yaw, pitch):
    """Y_UP (0, 0) looks across the s seam (-z), (0.4, pi/2) at the zenith pole; Z_UP (0, 0) looks at the -z pole, (pi/2, 0.2) across the
    seam (-x).  A pixel counts when every one of its camera rays (the camera model's rays, from the oracle) maps inside one CLOSEST block,
    at least 2e-3 from its edges in s and t; its film value must be the oracle's with that block's colour as the constant environment."""
    from phosphorus_mk2_amd import abi
    W = H = 32
    spp = 8
    base = aim_camera(_far_geometry(), yaw, pitch)
    img = _blocks()
    sc = _with_env(base, img, (1.0, 1.0, 1.0), mapping, abi.TEX_CLOSEST)
    film, _ = xpu.render(sc, spp=spp, pps=1, depth=9, seed=2)
    O = orc.Oracle(base, spp=spp, pps=1, depth=9)
    block = np.full(W * H, -1); good = np.ones(W * H, bool)
    for s in range(spp):
        o, d = O.camera_rays((0, 0, W, H), s, seed=2)
        st, ok = np_env_st(d, mapping)
        st = st.astype(np.float64)
        x, y = st[:, 0] * BW, st[:, 1] * BH
        i, j = np.floor(x) % BW, np.floor(y)
        margin = 2e-3 * np.array([BW, BH])
        inside = ok & (x - np.floor(x) > margin[0]) & (np.ceil(x) - x > margin[0]) & (y - np.floor(y) > margin[1]) & (np.ceil(y) - y > margin[1])
        k = (j * BW + i).astype(np.int64)
        good &= inside & ((block < 0) | (block == k))
        block = np.where(good, k, -1)
    assert good.sum() >= W * H // 3 and len(np.unique(block[good])) >= 3, (good.sum(), np.unique(block[good]))
    got = film[..., :3].reshape(-1, 3)
    for k in np.unique(block[good]):
        ref, _ = _oracle(orc, _with_constant_env(base, img[k // BW, k % BW]), spp, 2)
        sel = good & (block == k)
        assert bits_equal(got[sel], ref[..., :3].reshape(-1, 3)[sel]), (k, img[k // BW, k % BW])


# ---- 5. closed form --------------------------------------------------------------------------------------------------------------------------
def _smooth_map(w=64, h=32):
    s = (np.arange(w) + 0.5) / w; t = (np.arange(h) + 0.5) / h
    S, T = np.meshgrid(s, t)
    return np.stack([1.0 + 0.5 * np.sin(2 * np.pi * S), 0.8 + 0.6 * np.cos(np.pi * T), 0.6 + 0.3 * np.sin(2 * np.pi * S + 1.0) * np.sin(np.pi * T)], -1).astype(F)


@pytest.mark.parametrize("mapping", [0, 1])
def test_tilted_lambert_quad_matches_the_closed_form(xpu, mapping):
    """one large Lambertian quad of albedo a whose normal is tilted 0.6 rad from +y (part of its hemisphere lies below the horizon), seen
    from above along its normal, depth 2, a zero-emission lamp behind it: every pixel's expectation is a times the cosine-weighted mean of
    the map over the quad's hemisphere (quadrature in numpy with the restated lookup)"""
    from phosphorus_mk2_amd import abi, scenes, sceneio
    a = np.array([0.8, 0.5, 0.3], F)
    tilt = 0.6
    n = np.array([0.0, np.cos(tilt), np.sin(tilt)]); t1 = np.array([1.0, 0.0, 0.0]); t2 = np.cross(n, t1)
    R = 200.0
    quad = [tuple(c) for c in (-R * t1 - R * t2, R * t1 - R * t2, R * t1 + R * t2, -R * t1 + R * t2)]
    assert np.dot(np.cross(np.subtract(quad[1], quad[0]), np.subtract(quad[2], quad[0])), n) > 0
    lamp = [tuple(-5 * n + c) for c in (-t1 - t2, -t1 + t2, t1 + t2, t1 - t2)]  # behind the quad, facing away
    mats = [scenes.MaterialDesc([scenes.LobeDesc(abi.LOBE_DIFFUSE, tuple(float(x) for x in a))]), scenes.emitter(0.0, 0.0, 0.0)]
    cam = scenes.CameraDesc(64, 64, 1.2, sceneio.look_at(3.0 * n, (0, 0, 0), (1, 0, 0)))
    # the quad as a 4 x 4 grid of quads: a scene needs at least 8 triangles (SURVEY A-13)
    g = np.linspace(-R, R, 5)
    cells = [scenes._quad(*[tuple(a * t1 + b * t2) for a, b in ((g[i], g[j]), (g[i + 1], g[j]), (g[i + 1], g[j + 1]), (g[i], g[j + 1]))], 0)
             for i in range(4) for j in range(4)]
    base = scenes.SceneDesc(cells + [scenes._quad(*lamp, 1)], mats, cam)
    img = _smooth_map()
    sc = _with_env(base, img, (1.0, 1.0, 1.0), mapping, abi.TEX_LINEAR)
    spp = 16
    film, st = xpu.render(sc, spp=spp, pps=1, depth=2, seed=11)
    px = film[..., :3].reshape(-1, 3).astype(np.float64)
    # quadrature: cosine-weighted directions about n on a midpoint grid of (u1, u2)
    N = 1024
    u1, u2 = np.meshgrid((np.arange(N) + 0.5) / N, (np.arange(N) + 0.5) / N)
    r, ph = np.sqrt(u1.ravel()), 2 * np.pi * u2.ravel()
    dirs = (r * np.cos(ph))[:, None] * t1 + (r * np.sin(ph))[:, None] * t2 + np.sqrt(1 - u1.ravel())[:, None] * n
    assert (dirs[:, 1] < 0).mean() > 0.05  # part of the hemisphere is below the horizon
    want = a.astype(np.float64) * np_env(sc.textures[-1], (1.0, 1.0, 1.0), mapping, dirs.astype(F)).astype(np.float64).mean(0)
    mean, se = px.mean(0), px.std(0) / np.sqrt(len(px))
    assert (px > 0).all()
    assert (np.abs(mean - want) <= 4 * se).all(), (mean, want, se)


# ---- 6. textured lobes and an environment image together ---------------------------------------------------------------------------------
def test_textured_box_with_environment_image(xpu):
    st, _ = grid_box(True)
    c = np.array([0.25, 1.5, 0.75], F)
    with_img = _with_env(st, c.reshape(1, 1, 3))
    with_const = _with_constant_env(st, c)
    fa, sa = xpu.render(with_img, spp=8, pps=1, depth=9, seed=5)
    fb, sb = xpu.render(with_const, spp=8, pps=1, depth=9, seed=5)
    fn, _ = xpu.render(st, spp=8, pps=1, depth=9, seed=5)
    assert (sa["rays_closest"], sa["rays_shadow"], sa["rays_masked"]) == (sb["rays_closest"], sb["rays_shadow"], sb["rays_masked"])
    assert bits_equal(fa[..., :3], fb[..., :3])
    assert not bits_equal(fa[..., :3], fn[..., :3])
    assert sa["device_bytes"] >= sb["device_bytes"]
    from phosphorus_mk2_amd import abi  # PERHIT + TEX + ENV on the pinhole camera; tests/test_gpu_shade_kernels.py compares this family with the oracle
    family = abi.SHADE_FAMILY_GENERAL + (abi.SHADE_G_PERHIT | abi.SHADE_G_TEX | abi.SHADE_G_ENV)
    want = (1 << abi.shade_kernel_bit(family, abi.SHADE_PASS_CAMERA)) | (1 << abi.shade_kernel_bit(family, abi.SHADE_PASS_LATER))
    assert sa["shade_kernels"] == want, abi.shade_kernel_names(sa["shade_kernels"])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_bad_environment_inputs_are_refused_and_the_device_stays_usable(xpu):
    from phosphorus_mk2_amd import scenes
    good = _with_env(open_box(), _smooth_map(16, 8), (0.5, 0.5, 0.5))
    env = good.environment_material

    def on_emitter(s):
        s.materials[3].emission_texture = 1

    def on_ordinary(s):
        s.materials[0].emission_texture = 1

    def without_environment(s):  # the image stays on a material that is no longer the environment
        s.environment_material = -1

    def out_of_range(s):
        s.materials[env].emission_texture = 2

    def bad_mapping(s):
        s.materials[env].emission_mapping = 2

    dev = xpu.HipDevice.make(xpu.Options(samples_per_pixel=4, paths_per_sample=1, path_depth=9))
    try:
        with pytest.raises(xpu.DeviceError) as e:
            dev.environment_lookup(np.ones((4, 3), F))
        assert "(4)" in str(e.value)  # PHX_ERR_STATE before preprocess

        def frame():
            film = xpu.Film(32, 32, 4)
            dev.start(good, xpu.FrameState(1, xpu.Tiles.make(32, 32, 32), film)); dev.join()
            return film.data.copy()
        dev.preprocess(good)
        ref = frame()
        assert ref[..., :3].max() > 0.05
        look = dev.environment_lookup(np.eye(3, dtype=F))
        for bad in (on_emitter, on_ordinary, without_environment, out_of_range, bad_mapping):
            s = copy.deepcopy(good)
            bad(s)
            with pytest.raises(xpu.DeviceError) as e:
                dev.preprocess(s)
            assert "(1)" in str(e.value) and len(str(e.value).split(":", 1)[1].strip()) > 5, bad.__name__  # PHX_ERR_ARG with a message
            dev.preprocess(good)
            assert bits_equal(frame(), ref), bad.__name__
            assert bits_equal(dev.environment_lookup(np.eye(3, dtype=F)), look)
        dev.preprocess(open_box())  # no image: the hook refuses
        with pytest.raises(xpu.DeviceError) as e:
            dev.environment_lookup(np.ones((4, 3), F))
        assert "(1)" in str(e.value)
        dev.preprocess(_with_constant_env(open_box(), (0.5, 0.5, 0.5)))
        with pytest.raises(xpu.DeviceError):
            dev.environment_lookup(np.ones((4, 3), F))
        dev.preprocess(good)
        assert bits_equal(frame(), ref)
    finally:
        dev.close()
